"""compute_joints.cloud_fit on the GPU: the written URDF's meshes against raw clouds on an exact-kinematics input (fixture a),
with the file's zero pose where the registered link frames are unrotated and where they are not, and the command line's
--cloud_fit."""
import json
import math
import os
import sys
import types

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu
HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import _collide_ref as ref  # noqa: E402
from _ply import write_ascii_ply  # noqa: E402


def _links(g, tag):
    clusters = np.split(g[f"{tag}.link_cluster_idx"], np.cumsum(g[f"{tag}.link_cluster_sizes"])[:-1])
    return [{"id": int(i), "parent_id": None if p < 0 else int(p), "cluster_idx": [int(x) for x in c]}
            for i, p, c in zip(g[f"{tag}.link_id"], g[f"{tag}.link_parent_id"], clusters)]


def _surface(tri, n, rng):
    """n points on the triangles (F,3,3), by area."""
    area = np.linalg.norm(np.cross(tri[:, 1] - tri[:, 0], tri[:, 2] - tri[:, 0]), axis=1)
    f = rng.choice(len(tri), n, p=area / area.sum())
    u, v = rng.random(n), rng.random(n)
    s = np.sqrt(u)[:, None]
    return tri[f, 0] * (1 - s) + tri[f, 1] * (s * (1 - v[:, None])) + tri[f, 2] * (s * v[:, None])


def _exact_case(golden, tmp_path, ts):
    """Fixture a: six links, exact kinematics; the URDF's zero pose is (sequence 0, step ``ts``).  Every link gets a box mesh in
    its link frame; the raw cloud of (s, t) is sampled on the boxes moved as the registration saw the links move from (0, ts)."""
    from autourdf_amd import compute_joints, link, ops
    g = golden("joints_reference.npz")
    links, coords = _links(g, "a"), g["a.coords"]
    S, T = coords.shape[:2]
    cms = [types.SimpleNamespace(coords=c) for c in coords]
    jd = compute_joints.estimate_joint_axes_from_tree(links, cms, 0, T, 4)
    mesh_dir = tmp_path / "mesh"
    mesh_dir.mkdir()
    rng = np.random.default_rng(4)
    half = {l["id"]: rng.uniform(0.01, 0.03, 3) for l in links}
    for l in links:
        box = ref.box_mesh(*half[l["id"]])
        link.write_stl(str(mesh_dir / f"{l['id']:04}.stl"), np.concatenate([np.zeros((12, 1, 3)), box], 1))
    path = str(tmp_path / "robot.urdf")
    compute_joints.create_urdf(links, jd, cms[0], path, str(mesh_dir), ts)
    motion = compute_joints.estimate_joint_motion(links, jd, cms, 0, T, ts)
    compute_joints.set_joint_limits(path, motion)
    replay = compute_joints.replay_urdf(path, links, motion, cms, 0, T, ts)
    reg = ops.link_poses(torch.from_numpy(coords).cuda(), [l["cluster_idx"] for l in links]).cpu().numpy()
    frames = compute_joints.link_transforms(links, cms[0], ts)
    raw_dirs, truth = [], []
    for s in range(S):
        raw_dirs.append(str(tmp_path / f"raw/seq{s}") + "/")
        for t in range(T):
            parts, owner = [], []
            for i, l in enumerate(links):
                mesh = link.read_stl(str(mesh_dir / f"{l['id']:04}.stl"))[:, 1:4].astype(np.float64)
                X = reg[s, t, i] @ np.linalg.inv(reg[0, ts, i]) @ np.asarray(frames[l["id"]], np.float64)
                parts.append(_surface(mesh, 40, rng) @ X[:3, :3].T + X[:3, 3])
                owner.append(np.full(40, l["id"]))
            write_ascii_ply(raw_dirs[-1] + f"{t:04}/robot.ply", np.concatenate(parts))
            truth.append(np.concatenate(owner))
    fit = compute_joints.cloud_fit(path, links, motion, cms, raw_dirs, 0, T, ts)
    radius = max(float(np.linalg.norm(h)) for h in half.values())
    pos_max, rot_max = max(r["pos_max"] for r in replay), max(r["rot_max"] for r in replay)
    print(f"cloud_fit on fixture a, zero pose at step {ts}: rms {fit['all']['rms']:.3g}, max {fit['all']['max']:.3g}, zero pose alone: "
          f"rms {fit['poses'][ts]['rms']:.3g}; the replay: pos_max {pos_max:.3g}, rot_max {rot_max:.3g}")
    return dict(fit=fit, bound=pos_max + rot_max * radius + 1e-9, S=S, T=T, links=links, truth=truth, path=path, motion=motion,
                cms=cms, raw_dirs=raw_dirs)


def test_cloud_fit_on_exact_kinematics(golden, tmp_path):
    """The zero pose at step 0, where the registered link frames are unrotated: the meshes posed by the written joints at the
    recovered positions lie on the clouds to the accuracy of the replay -- a point is off by at most the link's replayed
    position error plus its rotation error times the mesh radius -- and the zero pose itself puts every link's mesh on that
    link's cloud of (0, 0): the frame check of the file as ``create_urdf`` writes it."""
    from autourdf_amd import compute_joints
    from autourdf_amd.cluster_icp import read_point_cloud
    c = _exact_case(golden, tmp_path, 0)
    fit, bound, S, T, links = c["fit"], c["bound"], c["S"], c["T"], c["links"]
    assert bound <= 1e-5 * 0.9 + 1e-5 * 0.06                      # what the replay test holds this fixture to
    assert len(fit["poses"]) == S * T and len(fit["sequences"]) == S and fit["all"]["n"] == S * T * 40 * len(links)
    assert fit["all"]["unexplained"] == 0 and fit["all"]["max"] <= bound and fit["poses"][0]["max"] <= bound
    assert all(p["max"] <= bound and p["n"] == 40 * len(links) for p in fit["poses"])
    assert [s["n"] for s in fit["sequences"]] == [T * 40 * len(links)] * S
    # the part segmentation: a point's link is the link it was sampled on, except where another link's box holds it too
    robot, link_T = compute_joints.cloud_fit_link_poses(c["path"], links, c["motion"], c["cms"], 0, T)
    names = [f"link_{i}" for i in np.concatenate(c["truth"])]
    got = [robot.links[i] for i in np.concatenate(fit["link"])]
    assert np.mean([a == b for a, b in zip(names, got)]) > 0.9
    step, row = fit["sequences"][1]["max_at"]
    assert fit["dist"][T + step][row] == fit["sequences"][1]["max"]
    # a limit below the displacement of a shifted cloud leaves it unexplained
    cloud = np.asarray(read_point_cloud(c["raw_dirs"][0] + "0000/robot.ply").points, np.float64)
    moved = compute_joints.cloud_fit_poses(robot, link_T[:1], [cloud + np.array([0.0, 0.0, 1.0])], 0.05)
    assert moved["all"]["unexplained"] == moved["all"]["n"] and np.isnan(moved["all"]["rms"]) and moved["all"]["max_at"] is None
    with pytest.raises(IndexError):
        compute_joints.cloud_fit(c["path"], links, c["motion"], c["cms"], c["raw_dirs"], 0, T + 1)


def test_cloud_fit_reports_a_zero_pose_with_rotated_link_frames(golden, tmp_path):
    """The zero pose at step 5, where the registered link frames are rotated: ``create_urdf``'s origin expressions add
    world-frame offsets to link-frame ones and no longer hold, the replay says so (errors of the scene's size), and the cloud fit
    says so as well -- it takes the file at its word."""
    c = _exact_case(golden, tmp_path, 5)
    assert c["bound"] > 1e-2 and c["fit"]["all"]["rms"] > 1e-2 and c["fit"]["poses"][5]["rms"] > 1e-2


def _layout(tmp_path, golden, robot, cams, step):
    """A data directory as the command line expects it: registered sequences, their raw frames, parameters.json."""
    M_ = golden("urdf_reference.npz")["a.matrices"]                            # (2,10,20,4,4), six links
    S, T, K = M_.shape[:3]
    (tmp_path / "parameters.json").write_text(json.dumps({robot: {"num_seg": K, "dof": 5}}))
    rng = np.random.default_rng(0)
    for s in range(S):
        part = tmp_path / f"data/part/{robot}_{K}_seg/{step}_deg_{cams}_cams/seq{s}"
        (part / "matrix").mkdir(parents=True)
        (part / "cluster").mkdir()
        for t in range(T):
            np.save(part / f"matrix/{t:04}.npy", M_[s, t])
            np.savez(part / f"cluster/{t:04}.npz", **{str(k): rng.normal(scale=0.02, size=(16, 3)).astype(np.float32)
                                                     for k in range(K)})
            raw = tmp_path / f"data/raw/{robot}/{step}_deg_{cams}_cams/seq{s}/{t:04}"
            raw.mkdir(parents=True)
            a = 0.9 / (2 * math.sqrt(3))                                      # AABB diagonal 0.9, as the fixture's
            write_ascii_ply(str(raw / "robot.ply"), np.vstack([rng.uniform(-a, a, size=(62, 3)), [[-a] * 3, [a] * 3]]))
    return S, T, K


@pytest.mark.filterwarnings("ignore:autourdf_amd.prefer_device_kernargs")     # main() in this process: the runtime is up already
def test_command_line_cloud_fit(golden, tmp_path, monkeypatch, capsys):
    """That fixture's clouds are random, so its distances are compared with a recomputation, not judged."""
    from autourdf_amd import compute_joints, coord_map, ops
    from autourdf_amd.cluster_icp import read_point_cloud
    from autourdf_amd.sim_data import UrdfRobot
    robot, cams, step = "testbot", 20, 4
    S, T, K = _layout(tmp_path, golden, robot, cams, step)
    out_dir = tmp_path / f"data/urdf/{robot}_{K}_seg"
    urdf = out_dir / f"{step}_deg_{cams}_cams.urdf"
    monkeypatch.chdir(tmp_path)
    base = ["--robot", robot, "--unknown_dof", "--end_video", "2", "--voxel_size", "0.01", "--joint_limits"]
    mesh_dir = tmp_path / f"data/mesh/{robot}_{K}_seg/{step}_deg_{cams}_cams/seq0"
    # without the option: what the command wrote before, and no point-mesh launch
    monkeypatch.setattr(ops, "point_mesh_distance", lambda *a, **k: pytest.fail("point_mesh_distance called without --cloud_fit"))
    coord_map.main(base)
    plain, listing, meshes = urdf.read_bytes(), sorted(os.listdir(out_dir)), sorted(os.listdir(mesh_dir))
    stem = f"{step}_deg_{cams}_cams"
    assert listing == [stem + ".joint_motion.json", stem + ".joint_positions.npy", stem + ".urdf"]
    monkeypatch.undo()
    monkeypatch.chdir(tmp_path)
    # with it
    seen = []
    poses = compute_joints.cloud_fit_link_poses
    monkeypatch.setattr(compute_joints, "cloud_fit_link_poses", lambda *a, **k: seen.append(poses(*a, **k)) or seen[-1])
    capsys.readouterr()
    coord_map.main(base + ["--cloud_fit", "--fit_max", "0.05"])
    text = capsys.readouterr().out
    assert urdf.read_bytes() == plain and sorted(os.listdir(mesh_dir)) == meshes
    assert sorted(os.listdir(out_dir)) == sorted(listing + [stem + ".cloud_fit.json"])
    report = json.loads((out_dir / (stem + ".cloud_fit.json")).read_text())
    assert report["fit_max"] == 0.05 and report["start_step"] == 0 and len(report["frames"]) == S * T
    assert len(report["sequences"]) == S and len(report["links"]) == 6
    lines = [x for x in text.splitlines() if x.startswith("cloud_fit seq")]
    assert len(lines) == S and all("rms" in x and "p95" in x and "unexplained" in x for x in lines)
    assert sum(x.startswith("cloud_fit: worst frame") for x in text.splitlines()) == 1
    assert text.index("replay: worst link") < text.index("cloud_fit seq0")              # it runs after the replay
    # the per-frame figures again, from the written URDF and meshes, the poses main used and the raw clouds
    (_, link_T), = seen
    r = UrdfRobot(str(urdf))
    raw = sorted((tmp_path / f"data/raw/{robot}/{step}_deg_{cams}_cams").iterdir())
    clouds = [np.asarray(read_point_cloud(str(raw[s] / f"{t:04}/robot.ply")).points, np.float64) for s in range(S) for t in range(T)]
    cut = np.concatenate([[0], np.cumsum([len(c) for c in clouds])])
    dist, _, link = ops.point_mesh_distance(torch.from_numpy(np.ascontiguousarray(r.tri)).cuda(), torch.from_numpy(r.tri_start).cuda(),
                                            link_T, torch.from_numpy(np.concatenate(clouds)).cuda(), torch.from_numpy(cut).cuda(), 0.05)
    dist, link = dist.cpu().numpy(), link.cpu().numpy()
    for p, f in enumerate(report["frames"]):
        d = dist[cut[p]:cut[p + 1]]
        ok = np.isfinite(d)
        assert (f["sequence"], f["step"], f["n"], f["unexplained"]) == (p // T, p % T, 64, int((~ok).sum()))
        if ok.any():
            assert f["rms"] == float(np.sqrt((d[ok] ** 2).sum() / ok.sum())) and f["max"] == float(d[ok].max())
            assert f["mean"] == float(d[ok].mean()) and f["max_at"] == int(np.flatnonzero(ok)[np.argmax(d[ok])])
        else:
            assert f["rms"] is None and f["max_at"] is None
    assert report["all"]["n"] == S * T * 64 and report["all"]["unexplained"] == int(np.isinf(dist).sum())
    assert [l["n"] for l in report["links"]] == [int((np.isfinite(dist) & (link == i)).sum()) for i in range(6)]
    # the keys of parameters.json: cloud_fit without the meshes or the positions, and a fit_max without it, before anything is written
    for entry, argv, word in (({"cloud_fit": True}, ["--joint_limits"], "voxel_size"), ({"cloud_fit": True, "voxel_size": 0.01}, [], "joint_limits"),
                              ({"fit_max": 0.1, "voxel_size": 0.01}, ["--joint_limits"], "cloud_fit"),
                              ({"cloud_fit": True, "fit_max": -1.0, "voxel_size": 0.01}, ["--joint_limits"], "fit_max")):
        (tmp_path / "parameters.json").write_text(json.dumps({robot: dict({"num_seg": K, "dof": 5}, **entry)}))
        os.remove(out_dir / (stem + ".cloud_fit.json")) if (out_dir / (stem + ".cloud_fit.json")).exists() else None
        with pytest.raises(ValueError, match=word):
            coord_map.main(["--robot", robot, "--unknown_dof", "--end_video", "2"] + argv)
        assert not (out_dir / (stem + ".cloud_fit.json")).exists()
