"""Joint motion on the GPU: creg_link_poses_f64, creg_joint_positions_f64 and creg_motion_error_f64 through ops against
the numpy restatement of their contracts (tests/_joint_motion_ref.py) on a synthetic tree with exact kinematics and on
fixture a; estimate_joint_motion / set_joint_limits / replay_urdf end to end; and the command line's --joint_limits."""
import functools
import json
import math
import os
import subprocess
import sys
import types
import xml.etree.ElementTree as ET

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu
HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
sys.path.insert(0, HERE)
import _joint_motion_ref as M  # noqa: E402

SUMMARY = ("lower", "upper", "tilt_rms", "tilt_max", "slip_rms", "slip_max")


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available()
    return torch.device("cuda")


@functools.lru_cache(maxsize=None)
def _tree(T):
    """The synthetic tree with three sequences of T steps, its restated link poses, and the device's (computed once)."""
    from autourdf_amd import ops
    t = M.synthetic_tree(S=3, T=T)
    t["link_T"] = M.link_poses(t["coords"], t["link_clusters"])
    t["link_T_dev"] = ops.link_poses(torch.from_numpy(t["coords"]).cuda(), t["link_clusters"])
    return t


def _links(g, tag):
    clusters = np.split(g[f"{tag}.link_cluster_idx"], np.cumsum(g[f"{tag}.link_cluster_sizes"])[:-1])
    return [{"id": int(i), "parent_id": None if p < 0 else int(p), "cluster_idx": [int(x) for x in c]}
            for i, p, c in zip(g[f"{tag}.link_id"], g[f"{tag}.link_parent_id"], clusters)]


def _np(out):
    return {k: v.cpu().numpy() for k, v in out.items()}


# ------------------------------------------------------------------------------------------------ link poses
@pytest.mark.parametrize("S", [1, 2])
@pytest.mark.parametrize("T", [1, 10])
def test_link_poses_vs_restatement(dev, golden, S, T):
    from autourdf_amd import ops
    g = golden("joints_reference.npz")
    coords = np.ascontiguousarray(g["a.coords"][:S, :T])
    clusters = [l["cluster_idx"] for l in _links(g, "a")]
    got = ops.link_poses(torch.from_numpy(coords).to(dev), clusters)
    assert got.shape == (S, T, 6, 4, 4) and got.dtype == torch.float64
    got = got.cpu().numpy()
    np.testing.assert_allclose(got, M.link_poses(coords, clusters), rtol=0, atol=1e-9)
    assert np.all(got[..., 3, :] == [0.0, 0.0, 0.0, 1.0])
    again = ops.link_poses(torch.from_numpy(coords).to(dev), clusters).cpu().numpy()
    assert got.tobytes() == again.tobytes()


def test_link_poses_on_the_tree_and_refusals(dev):
    from autourdf_amd import ops
    t = _tree(60)
    np.testing.assert_allclose(t["link_T_dev"].cpu().numpy(), t["link_T"], rtol=0, atol=1e-9)
    c = torch.from_numpy(t["coords"]).to(dev)
    with pytest.raises(ValueError):
        ops.link_poses(c, [[0], []])
    with pytest.raises(ValueError):
        ops.link_poses(c, [[0], [7]])
    with pytest.raises(ValueError):
        ops.link_poses(c[0], [[0]])


# ------------------------------------------------------------------------------------------------ joint positions
def _check_against_restatement(got, ref, want_q):
    for k in ("q", "tilt", "slip"):
        np.testing.assert_allclose(got[k], ref[k], rtol=0, atol=1e-8, err_msg=k)
    for k in SUMMARY:
        np.testing.assert_allclose(got[k], ref[k], rtol=0, atol=1e-8, err_msg=k)
    assert got["n_used"].tolist() == ref["n_used"].tolist()
    assert np.abs(got["q"] - want_q).max() <= 1e-9
    checked = 0
    for j in range(len(ref["lower"])):
        # an extreme within rounding of the runner-up names no sample: the ramp joint stands at 0 at step 0 of every sequence
        u = np.sort(ref["q"][j].reshape(-1))
        if len(u) > 1 and (u[1] - u[0] <= 1e-6 or u[-1] - u[-2] <= 1e-6):
            continue
        assert got["lower_at"][j].tolist() == ref["lower_at"][j].tolist()
        assert got["upper_at"][j].tolist() == ref["upper_at"][j].tolist()
        checked += 1
    assert checked >= 2


@pytest.mark.parametrize("S", [1, 2, 3])
@pytest.mark.parametrize("num_steps", [1, 2, 5, 70, 300])      # 70 crosses a wave, 300 the 256-sample tile of the unwrap
@pytest.mark.parametrize("start_step", [0, 3])
@pytest.mark.parametrize("ref_inside", [True, False])
def test_joint_positions_vs_restatement(dev, S, num_steps, start_step, ref_inside):
    from autourdf_amd import ops
    t = _tree(60 if num_steps <= 5 else 310)
    T = t["coords"].shape[1]
    ref_step = start_step + num_steps // 2 if ref_inside else T - 1
    args = (t["joints"], t["local_axis"], t["local_pos"], 0, ref_step, start_step, num_steps)
    got = _np(ops.joint_positions(t["link_T_dev"][:S].contiguous(), *args))
    ref = M.joint_positions(t["link_T"][:S], *args)
    assert got["q"].shape == (3, S, num_steps) and got["lower_at"].shape == (3, 2) and got["n_used"].dtype == np.int32
    _check_against_restatement(got, ref, M.expected_positions(t["q_true"][:, :S], 0, ref_step, start_step, num_steps))
    assert got["n_used"].tolist() == [S * num_steps] * 3
    assert max(got["tilt_max"].max(), got["slip_max"].max()) <= 1e-9          # exact kinematics: nothing is left over


def test_the_370_degree_joint_unwraps_to_its_true_series(dev):
    from autourdf_amd import ops
    t = _tree(60)
    got = _np(ops.joint_positions(t["link_T_dev"][:2].contiguous(), t["joints"], t["local_axis"], t["local_pos"]))
    r = M.RAMP_JOINT
    assert np.abs(got["q"][r] - t["q_true"][r, :2]).max() <= 1e-9
    assert abs(math.degrees(got["upper"][r] - got["lower"][r]) - 370.0) <= 1e-6
    assert got["q"][r].min() < -math.pi                                       # past the wrap
    assert got["lower_at"][r].tolist() == [0, 59] and got["upper_at"][r].tolist() == [1, 59]


def test_joint_positions_bits_repeat_and_do_not_depend_on_the_other_joints(dev):
    from autourdf_amd import ops
    t = _tree(310)
    lt = t["link_T_dev"]
    a = _np(ops.joint_positions(lt, t["joints"], t["local_axis"], t["local_pos"], 0, 5, 2, 300))
    b = _np(ops.joint_positions(lt, t["joints"], t["local_axis"], t["local_pos"], 0, 5, 2, 300))
    for k in a:
        assert a[k].tobytes() == b[k].tobytes(), k
    for j in range(3):
        alone = _np(ops.joint_positions(lt, t["joints"][j:j + 1], t["local_axis"][j:j + 1], t["local_pos"][j:j + 1], 0, 5, 2, 300))
        for k in a:
            assert alone[k][0].tobytes() == a[k][j].tobytes(), (j, k)
    # local_pos (J,3) is local_pos (J,4) without its homogeneous one
    c = _np(ops.joint_positions(lt, t["joints"], t["local_axis"], t["local_pos"][:, :3], 0, 5, 2, 300))
    assert all(a[k].tobytes() == c[k].tobytes() for k in a)


def test_joint_positions_without_joints_and_refusals(dev):
    from autourdf_amd import ops
    lt = _tree(60)["link_T_dev"]
    out = ops.joint_positions(lt, [], np.zeros((0, 3)), np.zeros((0, 4)), 0, 0, 0, 10)
    assert out["q"].shape == (0, 3, 10) and out["lower"].shape == (0,) and out["lower_at"].shape == (0, 2)
    torch.cuda.synchronize()
    t = _tree(60)
    args = (t["joints"], t["local_axis"], t["local_pos"])
    for bad in ((0, 0, 0, 61), (0, 0, 58, 3), (3, 0, 0, 5), (0, 60, 0, 5), (-1, 0, 0, 5)):
        with pytest.raises(IndexError):
            ops.joint_positions(lt, *args, *bad)
    with pytest.raises(ValueError):
        ops.joint_positions(lt, [(0, 4)], t["local_axis"][:1], t["local_pos"][:1])
    with pytest.raises(ValueError):
        ops.joint_positions(lt, t["joints"], t["local_axis"][:2], t["local_pos"])
    with pytest.raises(ValueError):
        ops.joint_positions(lt, *args, 0, 0, 0, 0)
    with pytest.raises(TypeError):
        ops.joint_positions(lt.float(), *args)


def test_a_nan_axis_stays_with_its_joint(dev):
    from autourdf_amd import ops
    t = _tree(60)
    clean = _np(ops.joint_positions(t["link_T_dev"], t["joints"], t["local_axis"], t["local_pos"]))
    ax = t["local_axis"].copy()
    ax[1] = np.nan
    got = _np(ops.joint_positions(t["link_T_dev"], t["joints"], ax, t["local_pos"]))
    assert got["n_used"].tolist() == [180, 0, 180]
    assert np.isnan(got["q"][1]).all() and np.isnan(got["tilt"][1]).all()
    assert all(np.isnan(got[k][1]) for k in SUMMARY)
    assert got["lower_at"][1].tolist() == [-1, -1] and got["upper_at"][1].tolist() == [-1, -1]
    for j in (0, 2):
        for k in clean:
            assert got[k][j].tobytes() == clean[k][j].tobytes(), (j, k)


def test_a_non_finite_cluster_pose_costs_only_the_samples_it_reaches(dev):
    from autourdf_amd import ops
    t = _tree(60)
    clean = _np(ops.joint_positions(t["link_T_dev"], t["joints"], t["local_axis"], t["local_pos"]))
    coords = t["coords"].copy()
    coords[1, 40, 6, 0] = np.nan                                              # cluster 6 is link 3: joint (1, 3), sequence 1, step 40
    lt = ops.link_poses(torch.from_numpy(coords).to(dev), t["link_clusters"])
    bad = ~torch.isfinite(lt).all(dim=4).all(dim=3).cpu().numpy()
    assert bad.sum() == 1 and bad[1, 40, 3]
    got = _np(ops.joint_positions(lt, t["joints"], t["local_axis"], t["local_pos"]))
    # the link's position is lost, its orientation is not: the turn is still seen, the slip of that one sample is not
    assert got["n_used"].tolist() == [180, 180, 179]
    assert np.isfinite(got["q"]).all() and np.isfinite(got["tilt"]).all()
    assert np.argwhere(~np.isfinite(got["slip"])).tolist() == [[2, 1, 40]]
    ref_lt = t["link_T"].copy()
    ref_lt[1, 40, 3, :3, 3] = np.nan
    _same_summary_and_untouched_rest(got, M.joint_positions(ref_lt, t["joints"], t["local_axis"], t["local_pos"]), clean)
    assert got["q"][2].tobytes() == clean["q"][2].tobytes()
    # a pose lost altogether: by the contract's recurrence u is not finite from that step to the end of its sequence
    lt = t["link_T_dev"].clone()
    lt[1, 40, 3] = float("nan")
    got = _np(ops.joint_positions(lt, t["joints"], t["local_axis"], t["local_pos"]))
    assert got["n_used"].tolist() == [180, 180, 160]
    assert np.isfinite(got["q"][2, 1, :40]).all() and not np.isfinite(got["q"][2, 1, 40:]).any()
    assert np.isfinite(got["slip"][2, 1, 41:]).all() and np.isfinite(got["tilt"][2, 1, 41:]).all()   # per-sample outputs stay as computed
    ref_lt[1, 40, 3] = np.nan
    _same_summary_and_untouched_rest(got, M.joint_positions(ref_lt, t["joints"], t["local_axis"], t["local_pos"]), clean)


def _same_summary_and_untouched_rest(got, ref, clean):
    for k in SUMMARY:
        np.testing.assert_allclose(got[k], ref[k], rtol=0, atol=1e-8, err_msg=k)
    assert got["lower_at"].tolist() == ref["lower_at"].tolist() and got["upper_at"].tolist() == ref["upper_at"].tolist()
    for j in (0, 1):                                                          # the joints that do not touch link 3
        for k in clean:
            assert got[k][j].tobytes() == clean[k][j].tobytes(), (j, k)
    for k in ("q", "tilt", "slip"):                                           # and the joint's other sequences
        assert got[k][2][[0, 2]].tobytes() == clean[k][2][[0, 2]].tobytes(), k


# ------------------------------------------------------------------------------------------------ motion error
@pytest.mark.parametrize("P", [1, 65])
@pytest.mark.parametrize("L", [1, 6])
def test_motion_error_vs_restatement(dev, P, L):
    from autourdf_amd import ops
    rng = np.random.default_rng(100 * P + L)
    A, B = (np.array([[M.random_rigid(rng) for _ in range(L)] for _ in range(P)]) for _ in range(2))
    A0, B0 = (np.array([M.random_rigid(rng) for _ in range(L)]) for _ in range(2))
    point = rng.normal(size=(L, 3))
    up = lambda x: torch.from_numpy(x).to(dev)
    rot, pos = ops.motion_error(up(A), up(A0), up(B), up(B0), up(point))
    assert rot.shape == (P, L) and pos.shape == (P, L)
    want_rot, want_pos = M.motion_error(A, A0, B, B0, point)
    np.testing.assert_allclose(rot.cpu().numpy(), want_rot, rtol=0, atol=1e-12)
    np.testing.assert_allclose(pos.cpu().numpy(), want_pos, rtol=0, atol=1e-12)
    rot, pos = ops.motion_error(up(A), up(A0), up(A), up(A0), up(point))
    bound = 1e-15 * (1.0 + np.linalg.norm(point, axis=1))
    assert np.all(rot.cpu().numpy() <= bound) and np.all(pos.cpu().numpy() <= bound)
    with pytest.raises(ValueError):
        ops.motion_error(up(A), up(A0), up(B), up(B0), up(point)[:, :2])


# ------------------------------------------------------------------------------------------------ end to end
def test_limits_and_replay_end_to_end_on_fixture_a(dev, golden, tmp_path):
    from autourdf_amd import compute_joints
    from autourdf_amd.sim_data import UrdfRobot
    g = golden("joints_reference.npz")
    links, coords = _links(g, "a"), g["a.coords"]
    S, T = coords.shape[:2]
    cms = [types.SimpleNamespace(coords=c) for c in coords]
    jd = compute_joints.estimate_joint_axes_from_tree(links, cms, 0, T, 4)
    path = str(tmp_path / "robot.urdf")
    compute_joints.create_urdf(links, jd, cms[0], path, "mesh/dir")
    motion = compute_joints.estimate_joint_motion(links, jd, cms, 0, T)
    assert [(m["parent_link"], m["child_link"]) for m in motion] == [(j["parent_link"], j["child_link"]) for j in jd]
    by_id = {l["id"]: i for i, l in enumerate(links)}
    ref = M.joint_positions(M.link_poses(coords, [l["cluster_idx"] for l in links]),
                            [(by_id[j["parent_link"]], by_id[j["child_link"]]) for j in jd],
                            [j["local_axis"] for j in jd], [j["local_pos"] for j in jd])
    for j, m in enumerate(motion):
        assert m["positions"].shape == (S, T) and m["n_used"] == S * T and m["positions"][0, 0] == 0.0
        assert abs(m["lower"] - ref["lower"][j]) <= 1e-8 and abs(m["upper"] - ref["upper"][j]) <= 1e-8
        assert list(m["lower_at"]) == ref["lower_at"][j].tolist() and list(m["upper_at"]) == ref["upper_at"][j].tolist()
        assert m["tilt_max"] <= 1e-6 and m["slip_max"] <= 1e-6
    compute_joints.set_joint_limits(path, motion)
    robot = UrdfRobot(path, load_meshes=False)
    for m in motion:
        (joint,) = [j for j in robot.joints if j["name"] == f"joint_{m['child_link']}"]
        assert joint["type"] == "revolute"
        assert joint["limit"] == [min(m["lower"], 0.0), max(m["upper"], 0.0)]   # str() round-trips a double
        assert joint["limit"][0] <= 0.0 <= joint["limit"][1] and joint["limit"][1] - joint["limit"][0] < 2.2
    replay = compute_joints.replay_urdf(path, links, motion, cms, 0, T)
    assert [r["link"] for r in replay] == [l["id"] for l in links] and all(r["n_used"] == S * T for r in replay)
    rot_max, pos_max = max(r["rot_max"] for r in replay), max(r["pos_max"] for r in replay)
    print(f"replay on fixture a: rot_max {rot_max:.3g} rad, pos_max {pos_max:.3g}")
    # the axes are within 1e-6 of the truth, the chain is 5 joints deep and no joint turns more than 1.03 rad: that product, doubled
    assert rot_max <= 1e-5 and pos_max <= 1e-5 * 0.9
    for r in replay:
        assert r["rot_rms"] <= r["rot_max"] and r["pos_rms"] <= r["pos_max"]
        assert 0 <= r["rot_max_at"][0] < S and 0 <= r["rot_max_at"][1] < T


def _layout(tmp_path, golden, robot, cams, step):
    """A data directory as the command line expects it: registered sequences, their raw frames, parameters.json."""
    from _ply import write_ascii_ply
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
def test_command_line_joint_limits(dev, golden, tmp_path, monkeypatch):
    from autourdf_amd import coord_map
    robot, cams, step = "testbot", 20, 4
    S, T, K = _layout(tmp_path, golden, robot, cams, step)
    stem = tmp_path / f"data/urdf/{robot}_{K}_seg/{step}_deg_{cams}_cams"
    urdf = stem.with_suffix(".urdf")
    # without the flag, in this process: the placeholder limits, no report
    monkeypatch.chdir(tmp_path)
    coord_map.main(["--robot", robot, "--unknown_dof", "--end_video", "2"])
    plain = urdf.read_bytes()
    assert plain.count(b'lower="-3.14159" upper="3.14159"') == 5
    assert not os.path.exists(str(stem) + ".joint_motion.json") and not os.path.exists(str(stem) + ".joint_positions.npy")
    with pytest.raises(ValueError, match="limit_pad"):
        (tmp_path / "parameters.json").write_text(json.dumps({robot: {"num_seg": K, "dof": 5, "limit_pad": 2.0}}))
        coord_map.main(["--robot", robot, "--unknown_dof", "--end_video", "2"])
    (tmp_path / "parameters.json").write_text(json.dumps({robot: {"num_seg": K, "dof": 5}}))
    # with it, as a command
    env = dict(os.environ, PYTHONPATH=ROOT + os.pathsep + os.environ.get("PYTHONPATH", ""))
    r = subprocess.run([sys.executable, "-m", "autourdf_amd.coord_map", "--robot", robot, "--unknown_dof", "--end_video", "2",
                        "--joint_limits", "--limit_pad", "1.5"], cwd=tmp_path, env=env, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-3000:]
    text = urdf.read_bytes()
    assert b"3.14159" not in text
    a, b = plain.splitlines(), text.splitlines()
    changed = [i for i, (x, y) in enumerate(zip(a, b)) if x != y]
    assert len(a) == len(b) and len(changed) == 5 and all(b"<limit " in a[i] and b"<limit " in b[i] for i in changed)
    report = json.loads(open(str(stem) + ".joint_motion.json").read())
    q = np.load(str(stem) + ".joint_positions.npy")
    assert q.shape == (5, S, T) and q.dtype == np.float64 and len(report["joints"]) == 5 and len(report["links"]) == 6
    assert report["limit_pad_deg"] == 1.5
    pad = math.radians(1.5)
    for j, m in zip(ET.parse(urdf).getroot().findall("joint"), report["joints"]):
        assert j.get("name") == f"joint_{m['child_link']}" and j.get("type") == "revolute"
        lim = j.find("limit")
        assert abs(float(lim.get("lower")) - min(m["lower"] - pad, 0.0)) <= 1e-15
        assert abs(float(lim.get("upper")) - max(m["upper"] + pad, 0.0)) <= 1e-15
        assert {"lower_at", "upper_at", "tilt_rms", "tilt_max", "slip_rms", "slip_max", "n_used", "parent_link"} <= set(m)
        assert m["n_used"] == S * T
    for l in report["links"]:
        assert {"link", "rot_rms", "rot_max", "pos_rms", "pos_max", "rot_max_at", "pos_max_at", "n_used"} <= set(l)
    lines = [x for x in r.stdout.splitlines() if x.startswith("joint_")]
    assert len(lines) == 5 and all("deg" in x and "tilt_rms" in x and "slip_rms" in x for x in lines)
    assert any(x.startswith("replay: worst link") for x in r.stdout.splitlines())
