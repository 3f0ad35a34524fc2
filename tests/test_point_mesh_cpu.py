"""The point-to-mesh restatement (tests/_point_mesh_ref.py) against hand-computed cases and a long-double brute force, and the
host side of creg_point_mesh_f64 that needs no GPU: the signatures and the workspace arithmetic."""
import numpy as np
import pytest

import _point_mesh_ref as pref

INF = np.inf
EPS = np.finfo(np.float64).eps


def one_pose(mesh, pts, d_max=INF):
    tri, start = pref.pack([mesh])
    pts = np.asarray(pts, np.float64).reshape(-1, 3)
    d2, idx, _ = pref.point_mesh(tri, start, np.eye(4)[None], pts, [0, len(pts)], d_max)
    return pref.wrapper(d2, idx, start, d_max)


@pytest.mark.parametrize("name", sorted(pref.ONE_TRIANGLE))
def test_restatement_on_one_triangle_in_every_voronoi_region(name):
    p, expected = pref.ONE_TRIANGLE[name]
    dist, idx, link = one_pose([pref.TRI], [p])
    assert idx.tolist() == [0] and link.tolist() == [0]
    assert abs(dist[0] - expected) <= 4 * EPS * 8.0
    if expected == 0.0:
        assert dist[0] == 0.0


def test_the_regions_of_the_one_triangle_cases_are_the_named_ones():
    """Each case sits in the region its name says: the header's conditions, evaluated by hand here."""
    a, b, c = (np.array(v, np.float64) for v in pref.TRI)
    for name, (p, _) in pref.ONE_TRIANGLE.items():
        p = np.array(p, np.float64)
        d1, d2, d3, d4, d5, d6 = (b - a) @ (p - a), (c - a) @ (p - a), (b - a) @ (p - b), (c - a) @ (p - b), (b - a) @ (p - c), (c - a) @ (p - c)
        vc, vb, va = d1 * d4 - d3 * d2, d5 * d2 - d1 * d6, d3 * d6 - d5 * d4
        region = ("vertex_a" if d1 <= 0 and d2 <= 0 else "vertex_b" if d3 >= 0 and d4 <= d3 else "vertex_c" if d6 >= 0 and d5 <= d6
                  else "edge_ab" if vc <= 0 and d1 >= 0 and d3 <= 0 else "edge_ac" if vb <= 0 and d2 >= 0 and d6 <= 0
                  else "edge_bc" if va <= 0 and d4 - d3 >= 0 and d5 - d6 >= 0 else "face")
        assert region == ("face" if name == "on_triangle" else name)


@pytest.mark.parametrize("name", sorted(pref.CUBE_CASES))
def test_restatement_on_the_unit_cube(name):
    p, expected = pref.CUBE_CASES[name]
    dist, idx, _ = one_pose(pref.CUBE, [p])
    assert 0 <= idx[0] < 12 and abs(dist[0] - expected) <= 4 * EPS * 4.0


def test_restatement_gate_nan_and_the_smallest_index():
    # the same triangle at rows 0 and 2: the smaller row wins; a NaN point and a point beyond d_max get (inf, -1)
    far = [[9, 9, 9], [10, 9, 9], [9, 10, 9]]
    pts = [[1, 1, pref.H], [np.nan, 0, 0], [1, 1, 3.0], [9.25, 9.25, 9.0]]
    dist, idx, link = one_pose([pref.TRI, far, pref.TRI], pts, 1.0)
    assert idx.tolist() == [0, -1, -1, 1] and link.tolist() == [0, -1, -1, 0]
    assert dist[0] == pref.H and np.isinf(dist[1]) and np.isinf(dist[2]) and dist[3] == 0.0
    dist, idx, _ = one_pose([far, pref.TRI, pref.TRI], pts, INF)
    assert idx.tolist() == [1, -1, 1, 0] and dist[2] == 3.0
    # a zero-area triangle answers with a point of itself
    dist, idx, _ = one_pose([[[1, 1, 1], [1, 1, 1], [1, 1, 1]], [[0, 0, 0], [2, 0, 0], [1, 0, 0]]], [[1, 1, 3], [1, -2, 0]])
    assert idx.tolist() == [0, 1] and dist.tolist() == [2.0, 2.0]
    # a value above d_max from a small box gap is masked by the wrapper's rule, the row stays
    d2, idx, _ = pref.point_mesh(*pref.pack([[pref.TRI]]), np.eye(4)[None], np.array([[3.0, 3.0, 0.0]]), [0, 1], 0.5)
    assert idx.tolist() == [0] and d2[0] == 2.0
    assert np.isinf(pref.wrapper(d2, idx, [0, 1], 0.5)[0][0])


def test_restatement_against_the_long_double_brute_force():
    """200 random points against a posed 300-triangle sphere cap and box, d_max = inf: another formulation, wider numbers."""
    rng = np.random.default_rng(5)
    tri, start = pref.pack([pref.uv_sphere(0.3, n=288), pref.box_mesh(0.1, 0.2, 0.15)])
    assert len(tri) == 300
    link_T = np.array([[pref.rigid(pref.random_rotation(rng), rng.uniform(-0.2, 0.2, 3)) for _ in range(2)]])
    pts = rng.uniform(-0.6, 0.6, (200, 3))
    d2, idx, _ = pref.point_mesh(tri, start, link_T, pts, [0, 200], INF)
    W = pref.posed_mesh(tri, start, link_T[0])
    want = pref.brute_long_double(W, pts)
    bound = 1e-12 * pref.scene_diagonal(tri, start, link_T, pts)
    assert (idx >= 0).all() and np.abs(np.sqrt(d2) - want).max() <= bound
    assert np.array_equal(pref.tri_d2(W, idx, pts), d2)          # the row attains the minimum, bit for bit


def test_signatures_are_listed_with_their_argument_counts():
    import ctypes

    from autourdf_amd import _lib
    res, args = _lib.SIGNATURES["creg_point_mesh_workspace_bytes"]
    assert res is ctypes.c_size_t and args == [ctypes.c_int64, ctypes.c_int32, ctypes.c_int64, ctypes.c_int64]
    res, args = _lib.SIGNATURES["creg_point_mesh_f64"]
    assert res is ctypes.c_int and len(args) == 16
    assert args[2] is ctypes.c_int64 and args[4] is ctypes.c_int32 and args[5] is ctypes.c_int64 and args[8] is ctypes.c_int64
    assert args[9] is ctypes.c_double and args[14] is ctypes.c_size_t


def test_workspace_bytes_is_monotone_in_its_counts_and_zero_for_the_refused_ones():
    """Pure host arithmetic: the posing stage's prefix posed | chunk_box | link_box, nothing of its own; the point count is
    checked and does not enter."""
    from autourdf_amd import _lib
    lib = _lib.load(check_device=False)
    assert lib.creg_version() >= 1800 and hasattr(lib, "creg_point_mesh_f64")
    size = lib.creg_point_mesh_workspace_bytes
    assert size(600, 5, 3, 1000) >= 8 * 9 * 600 * 3 + 8 * 6 * 5 * 3 and size(600, 5, 3, 1000) % 256 == 0
    assert size(600, 5, 3, 0) == size(600, 5, 3, 1000) == size(600, 5, 3, (1 << 31) - 1)
    assert size(600, 5, 3, 0) == lib.creg_mesh_clearance_workspace_bytes(600, 5, 3, 0)       # the same prefix
    tris, links, poses = (0, 1, 255, 256, 257, 32768, 32769), (1, 2, 12), (1, 2, 3, 70000)
    for n_links in links:
        for n_poses in poses:
            row = [size(f, n_links, n_poses, 10) for f in tris]
            assert all(a > 0 for a in row) and row == sorted(row), (n_links, n_poses)
    for f in tris:
        assert [size(f, l, 2, 10) for l in links] == sorted(size(f, l, 2, 10) for l in links)
        assert [size(f, 3, p, 10) for p in poses] == sorted(size(f, 3, p, 10) for p in poses)
    for bad in ((-1, 1, 1, 0), (1 << 31, 1, 1, 0), (1, 0, 1, 0), (1, 1, 0, 0), (1, 1, 1, -1), (1, 1, 1, 1 << 31)):
        assert size(*bad) == 0, bad


def test_cloud_fit_flags_and_their_usage_errors(tmp_path, monkeypatch, capsys):
    """--cloud_fit needs --voxel_size and --joint_limits, --fit_max needs --cloud_fit: usage errors out of parse_args, before
    main reads or writes anything."""
    import inspect
    import os

    from autourdf_amd import compute_joints, coord_map
    parse = coord_map._cli_parser().parse_args
    args = parse(["--voxel_size", "0.01", "--joint_limits", "--cloud_fit", "--fit_max", "0.05"])
    assert args.cloud_fit is True and args.fit_max == 0.05
    args = parse(["--voxel_size", "0.01", "--joint_limits", "--cloud_fit"])
    assert args.cloud_fit is True and args.fit_max is None           # no default other than inf, applied in main
    args = parse([])
    assert args.cloud_fit is False and args.fit_max is None
    monkeypatch.chdir(tmp_path)
    for bad in (["--cloud_fit", "--joint_limits"], ["--cloud_fit", "--voxel_size", "0.01"], ["--cloud_fit"],
                ["--fit_max", "0.05"], ["--fit_max", "0.05", "--voxel_size", "0.01", "--joint_limits"]):
        with pytest.raises(SystemExit):
            parse(bad)
        with pytest.raises(SystemExit):
            coord_map.main(["--robot", "none"] + bad)
        assert os.listdir(tmp_path) == []
    assert "--cloud_fit needs --voxel_size" in capsys.readouterr().err
    with pytest.raises(SystemExit):
        coord_map._parser().parse_args(["--cloud_fit"])               # not a flag of the reference
    sig = inspect.signature(compute_joints.cloud_fit).parameters
    assert list(sig) == ["urdf_file", "links", "motion", "cm_list", "raw_dirs", "start_step", "num_steps", "time_step", "d_max"]
    assert sig["time_step"].default == 0 and sig["d_max"].default == INF
    sig = inspect.signature(compute_joints.cloud_fit_poses).parameters
    assert list(sig) == ["robot", "link_T", "clouds", "d_max"] and sig["d_max"].default == INF


def test_fit_figures_cover_the_finite_distances():
    from autourdf_amd.compute_joints import _fit_figures
    f = _fit_figures([0.3, INF, 0.4, 0.0, INF])
    assert f["n"] == 5 and f["unexplained"] == 2 and f["max"] == 0.4 and f["max_at"] == 2
    assert abs(f["mean"] - 0.7 / 3) <= 1e-16 and abs(f["rms"] - np.sqrt(0.25 / 3)) <= 1e-16 and f["p95"] == np.percentile([0.3, 0.4, 0.0], 95)
    f = _fit_figures([INF, np.nan])
    assert f["n"] == 2 and f["unexplained"] == 2 and f["max_at"] is None and np.isnan(f["rms"])
    assert _fit_figures([])["n"] == 0
