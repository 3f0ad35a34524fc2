"""N4, joints / link clouds / URDF on the GPU: creg_joint_axes_f64 and creg_link_clouds_f64 through the C ABI and the
compute_joints / coord_map / link drop-ins, against the reference's own results (tests/golden/joints_reference.npz),
the true kinematics of the fixture's robots, a numpy restatement (tests/_joints_ref.py) and screw-axis edge cases;
save_links feeding refine_links_clusters; and the coord_map command line end to end."""
import math
import os
import subprocess
import sys
import types
import xml.etree.ElementTree as ET

import numpy as np
import pytest
import torch
from scipy.spatial.transform import Rotation

pytestmark = pytest.mark.gpu
HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
sys.path.insert(0, HERE)
import _joints_ref as JR  # noqa: E402

CASES = ["a", "b", "c"]


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available()
    return torch.device("cuda")


def _links(g, tag):
    clusters = np.split(g[f"{tag}.link_cluster_idx"], np.cumsum(g[f"{tag}.link_cluster_sizes"])[:-1])
    return [{"id": int(i), "parent_id": None if p < 0 else int(p), "cluster_idx": [int(x) for x in c]}
            for i, p, c in zip(g[f"{tag}.link_id"], g[f"{tag}.link_parent_id"], clusters)]


def _cms(coords):
    return [types.SimpleNamespace(coords=c) for c in coords]


def _pairs(links):
    by_id = {l["id"]: i for i, l in enumerate(links)}
    return [(by_id[l["parent_id"]], i) for i, l in enumerate(links) if l["parent_id"] is not None]


@pytest.mark.parametrize("tag", CASES)
def test_joint_axes_vs_reference_golden(dev, golden, tag):
    from autourdf_amd import compute_joints, ops
    g = golden("joints_reference.npz")
    links, coords = _links(g, tag), g[f"{tag}.coords"]
    T = coords.shape[1]
    jd = compute_joints.estimate_joint_axes_from_tree(links, _cms(coords), 0, T, 4)
    assert [j["parent_link"] for j in jd] == g[f"{tag}.joint_parent"].tolist()
    assert [j["child_link"] for j in jd] == g[f"{tag}.joint_child"].tolist()
    pairs = _pairs(links)
    raw = ops.joint_axes(torch.from_numpy(coords).to(dev), [l["cluster_idx"] for l in links], pairs, 0, T, 4)
    well_posed = 0
    for i, j in enumerate(jd):
        sg = 1.0 if j["local_axis"] @ g[f"{tag}.local_axis"][i] > 0 else -1.0          # one sign per joint
        np.testing.assert_allclose(j["local_axis"], sg * g[f"{tag}.local_axis"][i], rtol=0, atol=1e-9)
        np.testing.assert_allclose(j["global_axis"], sg * g[f"{tag}.global_axis"][i], rtol=0, atol=1e-9)
        p, c = pairs[i]
        smp = JR.samples(coords, links[p]["cluster_idx"], links[c]["cluster_idx"], 0, T, 4, reference=False)
        if max(x[3] for x in smp) <= JR.WELL_POSED:                  # the reference's eig point is defined
            np.testing.assert_allclose(j["global_pos"], g[f"{tag}.global_pos"][i], rtol=0, atol=1e-6)
            np.testing.assert_allclose(j["local_pos"], g[f"{tag}.local_pos"][i], rtol=0, atol=1e-6)
            well_posed += 1
        else:                                                         # it is rounding noise: the closed forms, restated
            poses = [[JR.pose_mean(coords[s, k], links[x]["cluster_idx"]) for s in range(coords.shape[0])
                      for a in range(4) for k in range(a, T, 4)] for x in (p, c)]
            ax, _, gp, lp = compute_joints.optimize_joint_axis(poses[0], poses[1], [x[0] for x in smp], [x[2] for x in smp])
            np.testing.assert_allclose(j["local_axis"], ax, rtol=0, atol=1e-9)
            np.testing.assert_allclose(j["global_pos"], gp, rtol=0, atol=1e-9)
            np.testing.assert_allclose(j["local_pos"], lp, rtol=0, atol=1e-9)
        # the convention: the first usable sample turns by a positive angle about local_axis
        use = raw["sample_usable"][i].cpu().numpy()
        f = int(np.argmax(use))
        assert use[f] and raw["sample_angle"][i, f].item() > 0
        assert j["local_axis"] @ raw["sample_axis"][i, f].cpu().numpy() > 0
        assert int(raw["count"][i]) == int(use.sum())
    assert well_posed >= {"a": 5, "b": 3, "c": 0}[tag]


@pytest.mark.parametrize("tag", ["a", "b"])
def test_joint_axes_recover_the_true_kinematics(dev, golden, tag):
    from autourdf_amd import compute_joints
    g, u = golden("joints_reference.npz"), golden("urdf_reference.npz")
    links = _links(g, tag)
    jd = compute_joints.estimate_joint_axes_from_tree(links, _cms(g[f"{tag}.coords"]), 0, g[f"{tag}.coords"].shape[1], 4)
    true_of = {l["id"]: int(u[f"{tag}.link_of"][l["cluster_idx"][0]]) for l in links}
    parents = u[f"{tag}.parents"]
    checked = 0
    for j in jd:
        p, c = true_of[j["parent_link"]], true_of[j["child_link"]]
        line = c if parents[c] == p else (p if parents[p] == c else None)    # a true joint, either direction
        if line is None:
            continue                                                          # the reference's tree has a cycle in b
        ta = u[f"{tag}.axes"][line]
        assert np.linalg.norm(np.cross(j["global_axis"], ta)) <= 1e-6
        assert np.linalg.norm(np.cross(j["global_pos"] - u[f"{tag}.joint_pos"][line], ta)) <= 1e-6
        checked += 1
    assert checked == {"a": 5, "b": 3}[tag]                                   # every true joint the tree holds


@pytest.mark.parametrize("S", [1, 2, 3])
@pytest.mark.parametrize("T", [2, 5, 10])
@pytest.mark.parametrize("interval", [1, 4])
def test_per_sample_outputs_vs_restatement(dev, golden, S, T, interval):
    from autourdf_amd import ops
    g = golden("joints_reference.npz")
    coords = np.concatenate([g["a.coords"], g["c.coords"]])[[0, 2, 1][:S], :T]      # (S,T,20,7)
    links = _links(g, "a")
    pairs = _pairs(links)[:2]
    out = ops.joint_axes(torch.from_numpy(np.ascontiguousarray(coords)).to(dev), [l["cluster_idx"] for l in links], pairs,
                         0, T, interval)
    NS = len(JR.sample_steps(S, T, interval))
    assert out["sample_angle"].shape == (len(pairs), NS) and ops.joint_samples(S, T, interval) == NS
    for j, (p, c) in enumerate(pairs):
        ref = JR.samples(coords, links[p]["cluster_idx"], links[c]["cluster_idx"], 0, T, interval)
        cf = JR.samples(coords, links[p]["cluster_idx"], links[c]["cluster_idx"], 0, T, interval, reference=False)
        for i, ((d, th, pt, shift), (_, _, pc, _)) in enumerate(zip(ref, cf)):
            assert bool(out["sample_usable"][j, i])
            got_d = out["sample_axis"][j, i].cpu().numpy()
            sg = 1.0 if got_d @ d > 0 else -1.0
            np.testing.assert_allclose(got_d, sg * d, rtol=0, atol=1e-9)
            assert abs(out["sample_angle"][j, i].item() - sg * th) <= 1e-8
            got_p = out["sample_point"][j, i].cpu().numpy()
            np.testing.assert_allclose(got_p, pc, rtol=0, atol=1e-9)
            if shift <= JR.WELL_POSED:
                np.testing.assert_allclose(got_p, pt, rtol=0, atol=1e-6)
        if NS == 0:
            assert int(out["count"][j]) == 0 and torch.isnan(out["local_axis"][j]).all()


def _two_link_coords(motions):
    """coords (1,T,2,7): cluster 0 (parent) fixed at the identity, cluster 1 (child) at I then each 4x4 in turn."""
    T = len(motions) + 1
    c = np.zeros((1, T, 2, 7))
    c[0, :, 0, 3] = 1.0
    mats = [np.eye(4)] + list(motions)
    for t, M in enumerate(mats):
        x, y, z, w = Rotation.from_matrix(M[:3, :3]).as_quat()
        c[0, t, 1] = [*M[:3, 3], w, x, y, z]
    return c


@pytest.mark.parametrize("angle", [1e-3, math.radians(4), math.pi / 2, math.radians(179.9), math.pi - 1e-6])
@pytest.mark.parametrize("shift", [0.0, 0.05])
def test_screw_axis_edge_cases(dev, angle, shift):
    from autourdf_amd import ops
    axis = np.array([0.3, -0.5, 0.8]) / np.linalg.norm([0.3, -0.5, 0.8])
    point = np.array([0.1, 0.2, -0.05])
    c = _two_link_coords([JR.screw(axis, angle, point, shift)])
    out = ops.joint_axes(torch.from_numpy(c).to(dev), [[0], [1]], [(0, 1)], 0, 2, 1)
    assert bool(out["sample_usable"][0, 0]) and int(out["count"][0]) == 1
    d = out["sample_axis"][0, 0].cpu().numpy()
    assert np.linalg.norm(np.cross(d, axis)) <= 1e-9
    assert abs(out["sample_angle"][0, 0].item() - angle) <= 1e-9
    np.testing.assert_allclose(out["sample_point"][0, 0].cpu().numpy(), JR.init_position(point, axis), rtol=0, atol=1e-8)
    np.testing.assert_allclose(out["local_axis"][0].cpu().numpy(), d, rtol=0, atol=1e-12)


def test_degenerate_steps_and_limits(dev):
    from autourdf_amd import compute_joints, ops
    axis, point = np.array([0.0, 0.6, 0.8]), np.array([0.1, 0.0, 0.0])
    motions = [np.eye(4), JR.screw(axis, 1e-6, point), JR.screw(axis, 0.3, point), JR.screw(axis, 0.3, point)]
    c = _two_link_coords(motions)                # steps: 0 -> I (0 rad), I -> 1e-6, 1e-6 -> 0.3, 0.3 -> 0.3 (0 rad)
    out = ops.joint_axes(torch.from_numpy(c).to(dev), [[0], [1]], [(0, 1)], 0, 5, 1)
    assert out["sample_usable"][0].cpu().tolist() == [False, False, True, False]
    assert int(out["count"][0]) == 1
    assert torch.isnan(out["sample_axis"][0, 0]).all() and torch.isnan(out["sample_point"][0, 3]).all()
    links = [{"id": 0, "parent_id": None, "cluster_idx": [0]}, {"id": 1, "parent_id": 0, "cluster_idx": [1]}]
    still = _two_link_coords([np.eye(4), np.eye(4)])
    with pytest.raises(ValueError, match="parent link 0 and child link 1"):
        compute_joints.estimate_joint_axes_from_tree(links, _cms(still), 0, 3, 1)
    with pytest.raises(IndexError):
        compute_joints.estimate_joint_axes_from_tree(links, _cms(c), 1, 5, 1)           # steps past T, as numpy
    big = torch.zeros(1, 3, 257, 7, dtype=torch.float64, device=dev)
    with pytest.raises(ValueError):
        ops.joint_axes(big, [[0], [1]], [(0, 1)], 0, 3, 1)


def _c2l_cm(g, u):
    from autourdf_amd.coord_map import CoordMap
    T, K = g["a.c2l_point_sizes"].shape
    cm = CoordMap.__new__(CoordMap)
    cm.coords = g["a.coords"][0]
    cm.matrices = u["a.matrices"][0]
    cm._M = torch.from_numpy(cm.matrices).cuda().contiguous()
    pts = np.split(g["a.c2l_points"], np.cumsum(g["a.c2l_point_sizes"].reshape(-1))[:-1])
    cm.clusters = [{str(k): pts[t * K + k] for k in range(K)} for t in range(T)]
    cidx = np.split(g["a.c2l_cluster_idx"], np.cumsum(g["a.c2l_cluster_sizes"])[:-1])
    return cm, [[int(x) for x in c] for c in cidx]


def test_cluster_to_link_vs_reference_golden(dev, golden):
    g, u = golden("joints_reference.npz"), golden("urdf_reference.npz")
    cm, cluster_idx = _c2l_cm(g, u)
    got = cm.cluster_to_link(cluster_idx)
    ref_m = g["a.c2l_matrices"]
    assert len(got) == len(ref_m)
    for l, ml in enumerate(got):
        assert ml["matrices"].dtype == np.float32
        # bit for bit: the fp64 mean and quaternion_to_matrix round to the same float32 values on this fixture (|q|^2
        # summed in another order than torch's could move an fp64 value by an ulp, which changes a float32 only at a tie)
        np.testing.assert_array_equal(ml["matrices"], ref_m[l])
        assert [len(c) for c in ml["clusters"]] == g["a.c2l_sizes"][l].tolist()
    lf = np.concatenate([c for ml in got for c in ml["clusters"]])
    wf = np.concatenate([c for ml in got for c in ml["clusters_wf"]])
    np.testing.assert_allclose(wf, g["a.c2l_wf"], rtol=0, atol=1e-12)
    np.testing.assert_allclose(lf, g["a.c2l_lf"], rtol=0, atol=1e-6)      # the reference inverts in float32


def test_cluster_to_link_raises_on_a_missing_cluster(dev, golden):
    g, u = golden("joints_reference.npz"), golden("urdf_reference.npz")
    cm, cluster_idx = _c2l_cm(g, u)
    del cm.clusters[3][str(cluster_idx[1][0])]
    with pytest.raises(KeyError):                                           # as the reference's dict lookup
        cm.cluster_to_link(cluster_idx)


def test_save_links_feeds_refine_links_clusters(dev, golden, tmp_path):
    from autourdf_amd import link
    g, u = golden("joints_reference.npz"), golden("urdf_reference.npz")
    cm, cluster_idx = _c2l_cm(g, u)
    T = cm.coords.shape[0]
    d = str(tmp_path / "seq0") + "/"
    link.save_links([cm], cluster_idx, [d], 0, T)
    L = len(cluster_idx)
    for sub, ext in (("matrix", ".npy"), ("cluster", ".npz"), ("cluster_wf", ".npz")):
        assert sorted(os.listdir(d + sub)) == [f"{t:04}{ext}" for t in range(T)]
    m = np.load(d + "matrix/0003.npy")
    assert m.dtype == np.float32 and m.shape == (L, 4, 4)
    with np.load(d + "cluster/0003.npz") as z:
        assert list(z.keys()) == [str(i) for i in range(L)] and all(z[k].dtype == np.float64 for k in z.keys())
    link.refine_links_clusters([d], 0, T, L - 1)
    assert sorted(os.listdir(d + "cluster_rf")) == [f"{t:04}.npz" for t in range(T)]
    with np.load(d + "cluster_rf/0000.npz") as z0, np.load(d + "cluster/0000.npz") as c0:
        assert list(z0.keys()) == [str(i) for i in range(L)]
        np.testing.assert_allclose(z0["0"], c0["0"], rtol=0, atol=1e-9)  # frame 0 registers onto itself


def _numbers(s):
    return np.array([float(x) for x in s.split()])


@pytest.mark.parametrize("tag", CASES)
def test_create_urdf_vs_reference_golden(dev, golden, tag, tmp_path):
    from autourdf_amd import compute_joints
    g = golden("joints_reference.npz")
    links = _links(g, tag)
    jd = [{"parent_link": int(p), "child_link": int(c), "local_axis": g[f"{tag}.local_axis"][i],
           "local_pos": g[f"{tag}.local_pos"][i], "global_pos": g[f"{tag}.global_pos"][i],
           "global_axis": g[f"{tag}.global_axis"][i]}
          for i, (p, c) in enumerate(zip(g[f"{tag}.joint_parent"], g[f"{tag}.joint_child"]))]
    cm = types.SimpleNamespace(coords=g[f"{tag}.coords"][0])
    path = str(tmp_path / "out" / "robot.urdf")
    compute_joints.create_urdf(links, jd, cm, path, str(g[f"{tag}.mesh_dir"]))
    text = open(path, "rb").read()
    ref = g[f"{tag}.urdf"].tobytes()
    assert text.splitlines()[0] == ref.splitlines()[0]                       # the XML declaration
    a, b = ET.fromstring(text), ET.fromstring(ref)
    ea, eb = list(a.iter()), list(b.iter())
    assert [e.tag for e in ea] == [e.tag for e in eb]
    for x, y in zip(ea, eb):
        assert sorted(x.attrib) == sorted(y.attrib), (x.tag, x.attrib, y.attrib)
        for k in x.attrib:
            if k in ("xyz", "rpy"):
                np.testing.assert_allclose(_numbers(x.attrib[k]), _numbers(y.attrib[k]), rtol=0, atol=1e-6)
            else:                                                            # names, mesh paths, colours, limits
                assert x.attrib[k] == y.attrib[k], (x.tag, k)
    assert len([l for l in text.splitlines()]) == len(ref.splitlines())     # ET.indent's layout


def test_command_line_end_to_end(dev, golden, tmp_path):
    import json
    from _ply import write_ascii_ply
    u = golden("urdf_reference.npz")
    M = u["a.matrices"]                                                        # (2,10,20,4,4), six links
    S, T, K = M.shape[:3]
    robot, cams, step = "testbot", 20, 4
    (tmp_path / "parameters.json").write_text(json.dumps({robot: {"num_seg": K, "dof": 5}}))
    rng = np.random.default_rng(0)
    for s in range(S):
        part = tmp_path / f"data/part/{robot}_{K}_seg/{step}_deg_{cams}_cams/seq{s}"
        (part / "matrix").mkdir(parents=True)
        (part / "cluster").mkdir()
        for t in range(T):
            np.save(part / f"matrix/{t:04}.npy", M[s, t] if t == 0 else M[s, t].astype(np.float32))
            np.savez(part / f"cluster/{t:04}.npz", **{str(k): rng.normal(scale=0.02, size=(16, 3)).astype(np.float32)
                                                     for k in range(K)})
            raw = tmp_path / f"data/raw/{robot}/{step}_deg_{cams}_cams/seq{s}/{t:04}"
            raw.mkdir(parents=True)
            a = 0.9 / (2 * math.sqrt(3))                                      # AABB diagonal 0.9, as the fixture's
            write_ascii_ply(str(raw / "robot.ply"), np.vstack([rng.uniform(-a, a, size=(62, 3)), [[-a] * 3, [a] * 3]]))
    env = dict(os.environ, PYTHONPATH=ROOT + os.pathsep + os.environ.get("PYTHONPATH", ""))
    r = subprocess.run([sys.executable, "-m", "autourdf_amd.coord_map", "--robot", robot, "--unknown_dof",
                        "--end_video", "2"], cwd=tmp_path, env=env, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-3000:]
    urdf = tmp_path / f"data/urdf/{robot}_{K}_seg/{step}_deg_{cams}_cams.urdf"
    assert urdf.exists()
    root = ET.parse(urdf).getroot()
    links, joints = root.findall("link"), root.findall("joint")
    assert len(links) == 6 and len(joints) == 5 and all(j.get("type") == "revolute" for j in joints)
    mesh_dir = f"data/mesh/{robot}_{K}_seg/{step}_deg_{cams}_cams/seq0/"
    assert root.find("link/visual/geometry/mesh").get("filename").startswith(mesh_dir)
    assert sorted(os.listdir(tmp_path / mesh_dir)) == ["cluster", "cluster_rf", "cluster_wf", "matrix"]
