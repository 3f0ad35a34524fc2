"""The mesh-cover restatement (tests/_mesh_cover_ref.py) against independent statements -- hand-computed cases, a long-double brute
force, the transposition relations with the point-to-mesh restatement -- and the host side of creg_mesh_cover_f64 that needs no
GPU: the symbols, ``subdivide_mesh``, the aggregation of ``surface_cover_poses`` and the command line's usage errors."""
import json
import math
import os

import numpy as np
import pytest
import torch

import _mesh_cover_ref as cref
import _point_mesh_ref as pref

INF = np.inf
EPS = np.finfo(np.float64).eps


def one_pose(mesh, pts, d_max=INF, labels=None):
    tri, start = pref.pack([mesh])
    pts = np.asarray(pts, np.float64).reshape(-1, 3)
    d2, idx, near, _ = cref.mesh_cover(tri, start, np.eye(4)[None], pts, [0, len(pts)], d_max, labels)
    return cref.wrapper(d2, d_max)[0], idx[0], near[0]


# ------------------------------------------------------------------------------------------ the restatement, independently
def test_symbols_and_version():
    import ctypes

    from autourdf_amd import _lib, build, ops
    lib = _lib.load(check_device=False)
    assert lib.creg_version() >= 2200 and hasattr(lib, "creg_mesh_cover_f64") and hasattr(lib, "creg_mesh_cover_workspace_bytes")
    assert "mesh_cover.hip" in build.SOURCES and os.path.exists(os.path.join(build.CSRC, "mesh_cover.hip")) and callable(ops.mesh_cover)
    res, args = _lib.SIGNATURES["creg_mesh_cover_f64"]
    assert res is ctypes.c_int and len(args) == 18 and args[9] is ctypes.c_int64 and args[10] is ctypes.c_double and args[16] is ctypes.c_size_t
    size = lib.creg_mesh_cover_workspace_bytes
    prefix = lib.creg_point_mesh_workspace_bytes
    for F, L, P, N in ((600, 5, 3, 1000), (0, 1, 1, 0), (257, 6, 70000, 63), (1, 1, 65537, 65537)):
        assert size(F, L, P, N) == prefix(F, L, P, N) + 48 * ((N >> 6) + P)              # 48 bytes per point-tile slot
    for bad in ((-1, 1, 1, 0), (1 << 31, 1, 1, 0), (1, 0, 1, 0), (1, 65536, 1, 0), (1, 1, 0, 0), (1, 1, 1, -1), (1, 1, 1, 1 << 31),
                ((1 << 31) - 1, 1, 1 << 40, 0), (1, 1, (1 << 31) - 1, 1 << 30)):
        assert size(*bad) == 0, bad


@pytest.mark.parametrize("name", sorted(pref.ONE_TRIANGLE))
def test_restatement_on_one_triangle_in_every_voronoi_region(name):
    p, expected = pref.ONE_TRIANGLE[name]
    dist, idx, near = one_pose([pref.TRI], [p])
    assert idx.tolist() == [0] and near.tolist() == [1] and abs(dist[0] - expected) <= 4 * EPS * 8.0
    if expected == 0.0:
        assert dist[0] == 0.0


def test_restatement_on_one_triangle_takes_the_nearest_of_all_regions_and_counts_the_near_ones():
    names = sorted(pref.ONE_TRIANGLE)
    pts = [pref.ONE_TRIANGLE[n][0] for n in names]
    want = np.array([pref.ONE_TRIANGLE[n][1] for n in names])
    dist, idx, near = one_pose([pref.TRI], pts)
    assert dist[0] == 0.0 and idx[0] == names.index("on_triangle") and near[0] == len(names)
    dist, idx, near = one_pose([pref.TRI], pts, 1.0)             # within 1.0: on the triangle (0) and the face point (0.75)
    assert dist[0] == 0.0 and near[0] == int((want <= 1.0).sum()) == 2
    labels = np.arange(len(names))[::-1] + 100
    assert one_pose([pref.TRI], pts, INF, labels)[1][0] == labels[names.index("on_triangle")]


@pytest.mark.parametrize("name", sorted(pref.CUBE_CASES))
def test_restatement_on_the_unit_cube(name):
    """The case point alone against the twelve triangles of [0,1]^3: the distance to every FACE by formula (per axis the excess over
    the face's extent), and the faces at the cube's distance are the covered ones at that d_max."""
    p, expected = pref.CUBE_CASES[name]
    p = np.array(p, np.float64)
    dist, idx, near = one_pose(pref.CUBE, [p])
    assert (idx == 0).all() and (near == 1).all()
    lo, hi = pref.CUBE.min(1), pref.CUBE.max(1)                  # a face's two triangles share its box, which is the face itself
    face = np.sqrt((np.maximum(0.0, np.maximum(lo - p, p - hi)) ** 2).sum(1))
    assert (dist >= face - 4 * EPS * 4.0).all() and abs(dist.min() - expected) <= 4 * EPS * 4.0
    for k in range(0, 12):                                       # the two triangles of a face: the nearer is at the face's distance
        mate = [j for j in range(12) if j != k and (lo[j] == lo[k]).all() and (hi[j] == hi[k]).all()]
        assert len(mate) == 1 and abs(min(dist[k], dist[mate[0]]) - face[k]) <= 4 * EPS * 4.0
    covered = one_pose(pref.CUBE, [p], expected * (1 + 1e-12))[0]
    assert np.isfinite(covered).any() and (np.isfinite(covered) == (dist <= expected * (1 + 1e-12))).all()


def test_restatement_gate_nan_infinite_and_the_smallest_label():
    far = [[9, 9, 9], [10, 9, 9], [9, 10, 9]]
    pts = [[1, 1, pref.H], [np.nan, 0, 0], [1, 1, pref.H], [9.25, 9.25, 9.0], [INF, 0, 0], [1, 1, 3.0]]
    dist, idx, near = one_pose([pref.TRI, far], pts, 1.0)
    assert idx.tolist() == [0, 3] and near.tolist() == [2, 1] and dist.tolist() == [pref.H, 0.0]
    dist, idx, near = one_pose([pref.TRI, far], pts, 1.0, [5, 1, 4, 9, 0, 2])        # the copy with the smaller label
    assert idx.tolist() == [4, 9]
    dist, idx, near = one_pose([pref.TRI, far], pts, INF)        # every live point with a finite d2 counts
    assert near.tolist() == [4, 4] and idx.tolist() == [0, 3]
    dist, idx, near = one_pose([pref.TRI], [[np.nan] * 3, [INF, 0, 0]])
    assert np.isinf(dist[0]) and idx[0] == -1 and near[0] == 0
    d2, idx, near, _ = cref.mesh_cover(*pref.pack([[pref.TRI]]), np.eye(4)[None], np.array([[3.0, 3.0, 0.0]]), [0, 1], 0.5)
    assert idx[0, 0] == 0 and d2[0, 0] == 2.0 and near[0, 0] == 0 and np.isinf(cref.wrapper(d2, 0.5)[0, 0])   # a small box gap, a larger distance
    d2, idx, near, _ = cref.mesh_cover(*pref.pack([[pref.TRI]]), np.eye(4)[None], np.zeros((0, 3)), [0, 0], 0.5)
    assert np.isinf(d2[0, 0]) and idx[0, 0] == -1 and near[0, 0] == 0


@pytest.fixture(scope="module")
def random_scene():
    rng = np.random.default_rng(5)
    tri, start = pref.pack([pref.uv_sphere(0.3, n=288), pref.box_mesh(0.1, 0.2, 0.15)])
    link_T = np.array([[pref.rigid(pref.random_rotation(rng), rng.uniform(-0.2, 0.2, 3)) for _ in range(2)] for _ in range(2)])
    pts = rng.uniform(-0.6, 0.6, (300, 3))
    pt_start = np.array([0, 120, 300])
    return tri, start, link_T, pts, pt_start


def test_restatement_against_the_long_double_brute_force(random_scene):
    """300 random points in two poses against a posed sphere cap and box, d_max = inf: another formulation, wider numbers; the scale
    of the bound is the point-mesh test's."""
    tri, start, link_T, pts, pt_start = random_scene
    d2, idx, near, _ = cref.mesh_cover(tri, start, link_T, pts, pt_start, INF)
    bound = 1e-12 * pref.scene_diagonal(tri, start, link_T, pts)
    for p in range(2):
        s, e = pt_start[p], pt_start[p + 1]
        W = pref.posed_mesh(tri, start, link_T[p])
        want = cref.brute_long_double(W, pts[s:e])
        assert np.abs(np.sqrt(d2[p]) - want).max() <= bound and (near[p] == e - s).all()
        assert ((idx[p] >= s) & (idx[p] < e)).all()
        assert np.array_equal(pref.tri_d2(W, np.arange(len(W)), pts[idx[p]]), d2[p])     # the labelled point attains the minimum, bit for bit


@pytest.mark.parametrize("d_max", [INF, 0.08])
def test_transposition_against_the_point_mesh_restatement(random_scene, d_max):
    tri, start, link_T, pts, pt_start = random_scene
    c2, cidx, _, cbox = cref.mesh_cover(tri, start, link_T, pts, pt_start, d_max)
    p2, pidx, pbox = pref.point_mesh(tri, start, link_T, pts, pt_start, d_max)
    assert cbox.tobytes() == pbox.tobytes()
    for p in range(2):
        s, e = pt_start[p], pt_start[p + 1]
        assert c2[p].min() == p2[s:e].min() and np.isfinite(c2[p].min())
        i = np.flatnonzero(pidx[s:e] >= 0) + s
        assert len(i) and (c2[p, pidx[i]] <= p2[i]).all()
        f = np.flatnonzero(cidx[p] >= 0)
        assert len(f) and (p2[cidx[p, f]] <= c2[p, f]).all()
    if d_max != INF:
        assert 0.05 < np.isinf(c2).mean() < 0.95


def test_the_edge_scene_has_no_ambiguous_triangle_for_the_restatement():
    """The GPU file compares pt_idx and n_near outside the triangles this marks; the condition is a property of the inputs, so the
    seed is checked here: nothing is excluded at any of the three d_max, in the three-pose scene and in the 64-point one."""
    for pose_points, sizes in ((cref.POSE_POINTS, cref.LINK_SIZES), ((64,), cref.LINK_SIZES), (cref.WIDTH_POINTS, cref.WIDTH_SIZES)):
        tri, start, link_T, pts, pt_start = cref.edge_scene(pose_points, link_sizes=sizes)
        assert len(tri) == sum(sizes) and np.isnan(pts).any() and np.isinf(pts).any()
        tol2 = 1e-12 * pref.scene_diagonal(tri, start, link_T, pts) ** 2
        for d_max in (0.0, cref.EDGE_D_MAX, INF):
            amb = cref.ambiguous(tri, start, link_T, pts, pt_start, d_max, tol2)
            assert not amb.any(), (pose_points, d_max, int(amb.sum()))
        d2 = cref.mesh_cover(tri, start, link_T, pts, pt_start, cref.EDGE_D_MAX)[0]
        if len(pose_points) == 3:
            assert np.isinf(d2[0]).all() and 0.05 < np.isfinite(d2[1:]).mean() < 0.95      # the gate cuts the scene, both ways


# ------------------------------------------------------------------------------------------ host helpers
def _areas(tri):
    return 0.5 * np.linalg.norm(np.cross(tri[:, 1] - tri[:, 0], tri[:, 2] - tri[:, 0]), axis=1)


def test_subdivide_mesh_keeps_the_surface_and_bounds_the_edges():
    from autourdf_amd.compute_joints import subdivide_mesh
    rng = np.random.default_rng(2)
    R = pref.random_rotation(rng)
    meshes = [pref.box_mesh(0.14, 0.05, 0.03) @ R.T, np.zeros((0, 3, 3)), pref.uv_sphere(0.1, n=100), [pref.TRI]]
    tri, start = pref.pack(meshes)
    for max_edge in (0.02, 0.05, 1.0):
        out, ostart, parent = subdivide_mesh(tri, start, max_edge)
        assert out.dtype == np.float64 and ostart.dtype == np.int64 and ostart[0] == 0 and ostart[-1] == len(out) == len(parent)
        edges = np.linalg.norm(out - np.roll(out, 1, axis=1), axis=2)
        assert edges.max() <= max_edge and len(out) > len(tri)
        assert (np.diff(parent) >= 0).all()                                        # the parts take their parent's place
        owner = np.searchsorted(start, parent, side="right") - 1
        for l in range(len(meshes)):
            rows = slice(ostart[l], ostart[l + 1])
            assert (owner[rows] == l).all()                                        # grouped by link
            a, b = math.fsum(_areas(out[rows])), math.fsum(_areas(tri[start[l]:start[l + 1]]))
            assert abs(a - b) <= 1e-15 * b, (l, a, b)
        for f in rng.integers(0, len(tri), 20):                                    # every part lies in its parent's plane, inside it
            a, b, c = tri[f]
            n = np.cross(b - a, c - a)
            part = out[parent == f].reshape(-1, 3)
            assert np.abs((part - a) @ n).max() <= 1e-15 * np.abs(n).max() + 1e-18
            coef = np.linalg.lstsq(np.stack([b - a, c - a], 1), (part - a).T, rcond=None)[0]
            assert (coef >= -1e-12).all() and (coef.sum(0) <= 1 + 1e-12).all()
            assert abs(math.fsum(_areas(out[parent == f])) - _areas(tri[f:f + 1])[0]) <= 4 * EPS * _areas(tri[f:f + 1])[0]
    fine, fstart, fparent = subdivide_mesh(tri, start, 10.0)                       # already fine: unchanged
    assert fine.tobytes() == tri.tobytes() and fstart.tolist() == start.tolist() and fparent.tolist() == list(range(len(tri)))
    one, ostart, parent = subdivide_mesh([pref.TRI], [0, 1], 2.5)                  # edges 4, 4, 5.66 -> 2, 2, 2.83 -> 1, 1, 1.41
    assert len(one) == 16 and (parent == 0).all() and ostart.tolist() == [0, 16]
    with pytest.raises(ValueError, match="max_edge"):
        subdivide_mesh(tri, start, 0.0)


class _Robot:
    """Four triangles of areas 1, 2, 3, 4 in two links."""
    links = ["a", "b"]
    tri_start = np.array([0, 1, 4], np.int64)
    tri = np.array([[[0, 0, 0], [s, 0, 0], [0, 2, 0]] for s in (1.0, 2.0, 3.0, 4.0)])


def test_surface_cover_poses_aggregates_by_area(monkeypatch):
    """4 triangles x 2 poses by hand, the kernel's outputs from a stub for ``ops.mesh_cover``."""
    from autourdf_amd import compute_joints, ops
    dist = np.array([[0.1, INF, 0.3, 0.2], [INF, INF, 0.4, INF]])
    near = np.array([[1, 0, 5, 1], [0, 0, 2, 0]], np.int32)
    calls = []

    def stub(tri, tri_start, link_T, pts, pt_start, d_max=INF, sort=True, want_boxes=False):
        calls.append((tuple(tri.shape), tri_start.tolist(), tuple(pts.shape), pt_start.tolist(), d_max))
        return torch.from_numpy(dist), torch.full((2, 4), -1, dtype=torch.int32), torch.from_numpy(near)

    monkeypatch.setattr(compute_joints, "ops", cref.OpsWith(ops, mesh_cover=stub))
    out = compute_joints.surface_cover_poses(_Robot(), torch.eye(4, dtype=torch.float64).repeat(2, 2, 1, 1), [np.zeros((3, 3)), np.zeros((0, 3))], 0.5)
    assert calls == [((4, 3, 3), [0, 1, 4], (3, 3), [0, 3, 3], 0.5)]
    assert out["area"].tolist() == [1.0, 2.0, 3.0, 4.0] and "parent_row" not in out
    p0, p1 = out["poses"]
    assert p0["area"] == p1["area"] == 10.0 and p0["uncovered"] == 0.2 and p1["uncovered"] == 0.7
    assert abs(p0["mean"] - (0.1 + 3 * 0.3 + 4 * 0.2) / 8) <= 1e-15 and abs(p0["rms"] - np.sqrt((0.01 + 3 * 0.09 + 4 * 0.04) / 8)) <= 1e-15
    assert p0["max"] == 0.3 and p0["max_at"] == 2 and p0["p95"] == 0.3 and p0["thin"] == 0.5       # rows 0 and 3: area 5 of 10
    assert abs(p1["mean"] - 0.4) <= 1e-15 and abs(p1["rms"] - 0.4) <= 1e-15 and p1["max"] == p1["p95"] == 0.4 and p1["max_at"] == 2 and p1["thin"] == 0.0
    a, b = out["links"]
    assert (a["link"], a["area"], a["uncovered"], a["never"]) == ("a", 1.0, 0.5, 0.0) and abs(a["rms"] - 0.1) <= 1e-15
    assert (b["link"], b["area"]) == ("b", 9.0) and abs(b["uncovered"] - (2 + 2 + 4) / 18) <= 1e-15 and abs(b["never"] - 2 / 9) <= 1e-15
    assert abs(b["rms"] - np.sqrt((3 * 0.09 + 4 * 0.04 + 3 * 0.16) / 10)) <= 1e-15
    al = out["all"]
    assert al["area"] == 10.0 and abs(al["uncovered"] - 9 / 20) <= 1e-15 and al["never"] == 0.2 and al["max"] == 0.4 and al["max_at"] == (1, 2)
    assert al["thin"] == 0.25 and al["p95"] == 0.4
    assert out["seen"].tolist() == [True, False, True, True] and out["dist"].shape == out["n_near"].shape == (2, 4)
    with pytest.raises(ValueError, match="poses"):
        compute_joints.surface_cover_poses(_Robot(), torch.eye(4, dtype=torch.float64).repeat(2, 2, 1, 1), [np.zeros((3, 3))])
    # nothing covered: shares stay shares, the distance figures are NaN
    dist[:], near[:] = INF, 0
    out = compute_joints.surface_cover_poses(_Robot(), torch.eye(4, dtype=torch.float64).repeat(2, 2, 1, 1), [np.zeros((3, 3)), np.zeros((0, 3))], 0.5)
    assert out["all"]["uncovered"] == 1.0 and out["all"]["never"] == 1.0 and np.isnan(out["all"]["rms"]) and out["all"]["max_at"] is None
    # subdividing: the stub sees the finer mesh, the dict names the parents
    seen = []
    fine = lambda tri, ts, T, pts, ps, d_max=INF: seen.append(tri.shape[0]) or (
        torch.zeros(2, tri.shape[0], dtype=torch.float64), torch.zeros(2, tri.shape[0], dtype=torch.int32),
        torch.ones(2, tri.shape[0], dtype=torch.int32))
    monkeypatch.setattr(compute_joints, "ops", cref.OpsWith(ops, mesh_cover=fine))
    out = compute_joints.surface_cover_poses(_Robot(), torch.eye(4, dtype=torch.float64).repeat(2, 2, 1, 1), [np.zeros((3, 3))] * 2, 0.5, max_edge=1.5)
    assert seen[0] == len(out["parent_row"]) > 4 and out["tri_start"][-1] == seen[0] and abs(out["all"]["area"] - 10.0) <= 1e-14
    assert out["all"]["uncovered"] == 0.0 and out["all"]["thin"] == 1.0


def test_coverage_flag_and_its_usage_errors(tmp_path, monkeypatch, capsys):
    import inspect

    from autourdf_amd import compute_joints, coord_map
    from autourdf_amd.sim_data import SimEnv
    parse = coord_map._cli_parser().parse_args
    assert parse(["--voxel_size", "0.01", "--joint_limits", "--cloud_fit", "--coverage"]).coverage is True
    assert parse(["--voxel_size", "0.01", "--joint_limits", "--cloud_fit"]).coverage is False and parse([]).coverage is False
    monkeypatch.chdir(tmp_path)
    for bad in (["--coverage"], ["--coverage", "--voxel_size", "0.01", "--joint_limits"]):
        with pytest.raises(SystemExit):
            parse(bad)
        with pytest.raises(SystemExit):
            coord_map.main(["--robot", "none"] + bad)
        assert os.listdir(tmp_path) == []
    assert "--coverage needs --cloud_fit" in capsys.readouterr().err
    with pytest.raises(SystemExit):
        coord_map._parser().parse_args(["--coverage"])               # not a flag of the reference
    (tmp_path / "parameters.json").write_text(json.dumps({"keyed": {"num_seg": 8, "dof": 3, "coverage": True, "voxel_size": 0.01,
                                                                    "joint_limits": True}}))
    monkeypatch.setenv("HIP_FORCE_DEV_KERNARG", os.environ.get("HIP_FORCE_DEV_KERNARG", "1"))
    monkeypatch.setattr(torch.cuda, "is_available", lambda: True)     # the check in front of parameters.json
    with pytest.raises(ValueError, match="coverage"):
        coord_map.main(["--robot", "keyed"])
    assert os.listdir(tmp_path) == ["parameters.json"]
    sig = inspect.signature(compute_joints.cloud_cover).parameters
    assert list(sig) == ["urdf_file", "links", "motion", "cm_list", "raw_dirs", "start_step", "num_steps", "time_step", "d_max"]
    assert sig["time_step"].default == 0 and sig["d_max"].default == INF
    for fn in (compute_joints.surface_cover_poses, SimEnv.surface_coverage):
        sig = inspect.signature(fn).parameters
        assert list(sig)[-4:] == ["link_T", "clouds", "d_max", "max_edge"] and sig["d_max"].default == INF and sig["max_edge"].default is None
