"""creg_mesh_cover_f64 on the GPU against the numpy restatement of its contract (tests/_mesh_cover_ref.py) and, exactly, against its
sibling creg_point_mesh_f64 on the device: the edges of the two tilings (256-triangle chunks, 64-point tiles), ties, order and
company, the 65535-pose slice, empty inputs, refusals -- then the measurement it exists for on the toy robot, and the command
line's --coverage.

The value bound is the sibling tests': 1e-12 on the scene's diagonal, here squared since squared distances are compared.  pt_idx
and n_near are compared outside the triangles the restatement itself marks ambiguous (a runner-up or the d_max^2 threshold within
that bound); tests/test_mesh_cover_cpu.py checks that the scene's seed leaves none."""
import ctypes
import json
import os

import numpy as np
import pytest
import torch

import _collide_ref as ref
import _mesh_cover_ref as cref
import _point_mesh_ref as pref
import _pose_fit_ref as pfref

pytestmark = pytest.mark.gpu
INF = np.inf


def dev(a):
    return torch.from_numpy(np.array(a)).to("cuda")              # a copy: the shared host arrays stay as they are


def run(tri, start, link_T, pts, pt_start, d_max, pt_row=None, pad=0, want_near=True):
    """dist2, pt_idx, n_near, link_box of the C entry.  ``pad`` rows of sentinels follow the outputs and the workspace's stated
    size; they must come back untouched."""
    from autourdf_amd import _lib
    lib = _lib.load()
    link_T = np.asarray(link_T, np.float64)
    link_T = link_T[None] if link_T.ndim == 3 else link_T
    pts = np.asarray(pts, np.float64).reshape(-1, 3)
    P, L, F, N = link_T.shape[0], link_T.shape[1], len(tri), len(pts)
    d_tri, d_start, d_T, d_pts, d_ps = dev(tri), dev(start), dev(link_T), dev(pts), dev(np.asarray(pt_start, np.int64))
    d_row = None if pt_row is None else dev(np.asarray(pt_row, np.int32))
    need = lib.creg_mesh_cover_workspace_bytes(F, L, P, N)
    assert need > 0 and need % 8 == 0
    ws = torch.full((need // 8 + pad,), -7.0, dtype=torch.float64, device="cuda")
    dist2 = torch.full((P * F + pad,), -7.0, dtype=torch.float64, device="cuda")
    idx = torch.full((P * F + pad,), -7, dtype=torch.int32, device="cuda")
    near = torch.full((P * F + pad,), -7, dtype=torch.int32, device="cuda")
    box = torch.full((P, L, 6), -7.0, dtype=torch.float64, device="cuda")
    ptr = lambda t: ctypes.c_void_p(t.data_ptr()) if t is not None and t.numel() else None
    rc = lib.creg_mesh_cover_f64(ptr(d_tri), ptr(d_start), F, ptr(d_T), L, P, ptr(d_pts), ptr(d_ps), ptr(d_row), N, float(d_max),
                                 ptr(dist2), ptr(idx), ptr(near) if want_near else None, ptr(box), ptr(ws), need, None)
    assert rc == 0, lib.creg_last_error()
    torch.cuda.synchronize()
    assert (dist2[P * F:] == -7.0).all() and (idx[P * F:] == -7).all() and (near[P * F:] == -7).all() and (ws[need // 8:] == -7.0).all()
    shape = lambda t: t[:P * F].cpu().numpy().reshape(P, F)
    return shape(dist2), shape(idx), shape(near), box.cpu().numpy()


def check(got, want, amb, tol2, what):
    g2, gi, gn, gbox = got
    w2, wi, wn, wbox = want
    assert g2.shape == w2.shape and g2.dtype == np.float64 and gi.dtype == np.int32 and gn.dtype == np.int32
    np.testing.assert_array_equal(gbox, wbox)
    np.testing.assert_array_equal(np.isinf(g2), np.isinf(w2))                   # the inf pattern, exactly
    assert ((gi == -1) == np.isinf(g2)).all() and not np.isnan(g2).any() and (g2 >= 0).all()
    fin = np.isfinite(w2)
    diff = np.abs(g2[fin] - w2[fin]).max() if fin.any() else 0.0
    print(f"{what}: {fin.sum()} finite of {fin.size}, largest |d2 - d2_ref| {diff:.3g} (bound {tol2:.3g}), bits identical: "
          f"{g2.tobytes() == w2.tobytes()}, ambiguous triangles: {int(amb.sum())}, equal pt_idx {np.mean(gi == wi):.4f}, "
          f"equal n_near {np.mean(gn == wn):.4f}")
    assert diff <= tol2
    assert amb.mean() <= 0.01
    np.testing.assert_array_equal(gi[~amb], wi[~amb])
    np.testing.assert_array_equal(gn[~amb], wn[~amb])


# ------------------------------------------------------------------------------------------ the edges of the two tilings
@pytest.fixture(scope="module")
def edges():
    out = cref.edge_scene()
    for a in out:
        a.setflags(write=False)
    tri, start, link_T, pts, pt_start = out
    return out + (1e-12 * pref.scene_diagonal(tri, start, link_T, pts) ** 2,)


@pytest.mark.parametrize("d_max", [0.0, cref.EDGE_D_MAX, INF])
def test_links_around_a_chunk_and_poses_around_a_tile(edges, d_max):
    """Links of 0, 1, 255, 256, 257 and 300 triangles, so that links start off a multiple of 256; poses of 0, 65 and 129 points in
    one call and one of exactly 64 in a second; a NaN point and a point with an infinite coordinate in every pose with points."""
    tri, start, link_T, pts, pt_start, tol2 = edges
    want = cref.mesh_cover(tri, start, link_T, pts, pt_start, d_max)
    amb = cref.ambiguous(tri, start, link_T, pts, pt_start, d_max, tol2)
    got = run(tri, start, link_T, pts, pt_start, d_max, pad=300)
    check(got, want, amb, tol2, f"edges d_max={d_max:.4g}")
    assert np.isinf(got[0][0]).all() and (got[1][0] == -1).all() and (got[2][0] == 0).all()       # the pose without points
    if d_max == INF:
        assert np.isfinite(got[0][1:]).all() and (got[2][1] == 65 - 2).all() and (got[2][2] == 129 - 2).all()
    without = run(tri, start, link_T, pts, pt_start, d_max, want_near=False)                      # n_near may be NULL
    assert without[0].tobytes() == got[0].tobytes() and without[1].tobytes() == got[1].tobytes() and (without[2] == -7).all()
    one = cref.edge_scene((64,))
    got = run(*one, d_max, pad=64)
    check(got, cref.mesh_cover(*one, d_max), cref.ambiguous(*one, d_max, tol2), tol2, f"one full tile d_max={d_max:.4g}")


def test_short_chunks_of_every_width():
    """Links of 16, 17, 32, 33, 64, 65, 128 and 129 triangles: a chunk of at most 128 is held 16, 8, 4 or 2 times and its copies
    share the points, one of 129 is held once."""
    scene = cref.edge_scene(cref.WIDTH_POINTS, link_sizes=cref.WIDTH_SIZES)
    tol2 = 1e-12 * pref.scene_diagonal(*scene[:4]) ** 2
    for d_max in (cref.EDGE_D_MAX, INF):
        got = run(*scene, d_max, pad=64)
        check(got, cref.mesh_cover(*scene, d_max), cref.ambiguous(*scene, d_max, tol2), tol2, f"widths d_max={d_max:.4g}")
        assert np.isfinite(got[0]).any()


# ------------------------------------------------------------------------------------------ exact identities with the sibling
@pytest.mark.parametrize("d_max", [cref.EDGE_D_MAX, INF])
def test_transposition_identities_with_point_mesh_distance_bit_for_bit(edges, d_max):
    """Both entries evaluate the same device function on the same posed vertices: per pose the two minima agree, a point's
    nearest triangle is at most as far from the cloud as the point from the mesh, and the other way round -- exactly."""
    from autourdf_amd import ops
    tri, start, link_T, pts, pt_start, _ = edges
    args = (dev(tri), dev(start), dev(link_T), dev(pts), dev(pt_start), d_max)
    pd, pf, _ = (o.cpu().numpy() for o in ops.point_mesh_distance(*args, sort=False))
    cd, ci, _ = (o.cpu().numpy() for o in ops.mesh_cover(*args, sort=False))
    assert cd.shape == (3, len(tri)) and ci.dtype == np.int32
    for p in range(3):
        s, e = int(pt_start[p]), int(pt_start[p + 1])
        if e == s:
            assert np.isinf(cd[p]).all()
            continue
        assert cd[p].min() == pd[s:e].min() and np.isfinite(cd[p].min())
        i = np.flatnonzero(pf[s:e] >= 0) + s
        assert len(i) and (cd[p, pf[i]] <= pd[i]).all()
        f = np.flatnonzero(ci[p] >= 0)
        assert len(f) and ((ci[p, f] >= s) & (ci[p, f] < e)).all() and (pd[ci[p, f]] <= cd[p, f]).all()


# ------------------------------------------------------------------------------------------ ties
def test_of_two_copies_of_a_point_the_smaller_row_wins(edges):
    from autourdf_amd import ops
    tri, start, link_T, pts, pt_start, _ = edges
    block = pts[int(pt_start[2]):int(pt_start[3])]
    n = len(block)
    twice = np.concatenate([block, block])
    for d_max in (cref.EDGE_D_MAX, INF):
        alone = run(tri, start, link_T[2], block, [0, n], d_max)
        both = run(tri, start, link_T[2], twice, [0, 2 * n], d_max)
        assert both[0].tobytes() == alone[0].tobytes() and both[1].tobytes() == alone[1].tobytes()      # every winner is a row of the first copy
        assert (both[1] < n).all() and (both[1] >= 0).any() and (both[2] == 2 * alone[2]).all()
        swapped = run(tri, start, link_T[2], twice, [0, 2 * n], d_max, pt_row=np.concatenate([np.arange(n) + n, np.arange(n)]))
        assert swapped[1].tobytes() == alone[1].tobytes() and swapped[0].tobytes() == alone[0].tobytes()   # now rows of the second
        for sort in (True, False):
            out = ops.mesh_cover(dev(tri), dev(start), dev(link_T[2]), dev(twice), dev(np.array([0, 2 * n])), d_max, sort=sort)
            assert out[1].cpu().numpy().tobytes() == alone[1].tobytes()


# ------------------------------------------------------------------------------------------ order and company
def test_sorted_or_not_permuted_alone_or_among_others_and_twice(edges):
    from autourdf_amd import ops
    tri, start, link_T, pts, pt_start, _ = edges
    rng = np.random.default_rng(3)
    for d_max in (cref.EDGE_D_MAX, INF):
        a, b = run(tri, start, link_T, pts, pt_start, d_max), run(tri, start, link_T, pts, pt_start, d_max)
        for x, y in zip(a, b):
            assert x.tobytes() == y.tobytes()
        perm = np.concatenate([rng.permutation(int(e - s)) + int(s) for s, e in zip(pt_start[:-1], pt_start[1:])])
        shuffled = run(tri, start, link_T, pts[perm], pt_start, d_max, pt_row=perm)
        for x, y in zip(a, shuffled):
            assert x.tobytes() == y.tobytes()
        args = (dev(tri), dev(start), dev(link_T), dev(pts), dev(pt_start), d_max)
        srt, raw = ops.mesh_cover(*args, sort=True, want_boxes=True), ops.mesh_cover(*args, sort=False, want_boxes=True)
        for x, y in zip(srt, raw):
            assert torch.equal(x, y)
        assert raw[1].cpu().numpy().tobytes() == a[1].tobytes() and raw[2].cpu().numpy().tobytes() == a[2].tobytes()
        assert torch.equal(raw[0], torch.where(dev(a[0]) > d_max * d_max, torch.full_like(raw[0], INF), torch.sqrt(dev(a[0]))))
        assert raw[3].cpu().numpy().tobytes() == a[3].tobytes()
        for p in (1, 2):                                         # a pose alone, its points labelled with their rows in the full call
            s, e = int(pt_start[p]), int(pt_start[p + 1])
            one = run(tri, start, link_T[p], pts[s:e], [0, e - s], d_max, pt_row=np.arange(s, e))
            for x, y in zip(one[:3], a[:3]):
                assert x[0].tobytes() == y[p].tobytes()


# ------------------------------------------------------------------------------------------ pose slices
def test_one_call_across_the_65535_pose_slice():
    """One triangle, 65537 poses each lifted by its own z, one point per pose above the face: the distance is the height by
    formula, the point is the pose's own row, one point is near."""
    from autourdf_amd import ops
    P = 65537
    k = np.arange(P)
    lift, height = k * 2.0 ** -10, 0.25 + (k % 7) * 0.125
    link_T = np.tile(np.eye(4), (P, 1, 1, 1))
    link_T[:, 0, 2, 3] = lift
    pts = np.stack([np.ones(P), np.ones(P), lift + height], 1)
    dist, idx, near = ops.mesh_cover(dev(np.array([pref.TRI], np.float64)), dev(np.array([0, 1])), dev(link_T), dev(pts),
                                     dev(np.arange(P + 1)), 1.5, sort=False)
    dist, idx, near = dist.cpu().numpy(), idx.cpu().numpy(), near.cpu().numpy()
    assert dist.shape == (P, 1) and np.abs(dist[:, 0] - height).max() <= 1e-12
    assert (idx[:, 0] == k).all() and (near == 1).all()


# ------------------------------------------------------------------------------------------ empty inputs
def test_no_points_and_no_triangles(edges):
    from autourdf_amd import ops
    tri, start, link_T, pts, pt_start, _ = edges
    none = run(tri, start, link_T, np.zeros((0, 3)), np.zeros(4, np.int64), 0.02, pad=64)
    assert np.isinf(none[0]).all() and (none[1] == -1).all() and (none[2] == 0).all()
    np.testing.assert_array_equal(none[3], cref.mesh_cover(tri, start, link_T, np.zeros((0, 3)), np.zeros(4, np.int64), 0.02)[3])
    assert np.isfinite(none[3][:, 1:]).all() and np.isinf(none[3][:, 0]).all()                      # the empty link's box is the empty box
    out = ops.mesh_cover(dev(np.zeros((0, 3, 3))), dev(np.zeros(3, np.int64)), dev(link_T[:, :2]), dev(pts), dev(pt_start), 0.02,
                         want_boxes=True)
    torch.cuda.synchronize()
    assert [tuple(o.shape) for o in out] == [(3, 0), (3, 0), (3, 0), (3, 2, 6)] and torch.isinf(out[3]).all()


# ------------------------------------------------------------------------------------------ refusals
def test_invalid_calls_return_einval_and_touch_nothing(edges):
    from autourdf_amd import _lib
    lib = _lib.load()
    tri, start, link_T, pts, pt_start, _ = edges
    P, L, F, N = link_T.shape[0], link_T.shape[1], len(tri), len(pts)
    d_tri, d_start, d_T, d_pts, d_ps = dev(tri), dev(start), dev(link_T), dev(pts), dev(pt_start)
    need = lib.creg_mesh_cover_workspace_bytes(F, L, P, N)
    ws = torch.empty(need // 8, dtype=torch.float64, device="cuda")
    dist2 = torch.full((P * F,), 77.0, dtype=torch.float64, device="cuda")
    idx = torch.full((P * F,), 77, dtype=torch.int32, device="cuda")
    near = torch.full((P * F,), 77, dtype=torch.int32, device="cuda")
    box = torch.full((P, L, 6), 77.0, dtype=torch.float64, device="cuda")
    ptr = lambda t: ctypes.c_void_p(t.data_ptr()) if t is not None else None

    def call(n_tri=F, n_links=L, n_poses=P, n_pts=N, d_max=0.02, ws_bytes=need, x=d_pts, ps=d_ps, d2=dist2, ix=idx, w=ws, t=d_tri):
        return lib.creg_mesh_cover_f64(ptr(t), ptr(d_start), n_tri, ptr(d_T), n_links, n_poses, ptr(x), ptr(ps), None, n_pts, d_max,
                                       ptr(d2), ptr(ix), ptr(near), ptr(box), ptr(w), ws_bytes, None)

    for kw in (dict(d_max=-0.01), dict(d_max=float("nan")), dict(d_max=-INF), dict(ws_bytes=need - 8), dict(ws_bytes=0), dict(d2=None),
               dict(ix=None), dict(x=None), dict(ps=None), dict(w=None), dict(t=None), dict(n_tri=1 << 31), dict(n_links=65536),
               dict(n_poses=0), dict(n_pts=-1), dict(n_pts=1 << 31), dict(n_links=0), dict(n_tri=-1), dict(n_poses=1 << 40), dict(n_tri=1 << 30, n_poses=1 << 27)):
        assert call(**kw) == -1, kw                               # CREG_EINVAL
        assert b"creg_mesh_cover_f64" in lib.creg_last_error()
        torch.cuda.synchronize()
        assert (dist2 == 77.0).all() and (idx == 77).all() and (near == 77).all() and (box == 77.0).all(), kw
    assert call() == 0                                           # and the same buffers with valid arguments
    torch.cuda.synchronize()
    assert not (dist2 == 77.0).any() and ((idx == -1) == torch.isinf(dist2)).all() and (idx < N).all()   # 77 is a row now


def test_wrapper_raises_before_any_launch(edges, monkeypatch):
    from autourdf_amd import _lib, ops
    tri, start, link_T, pts, pt_start, _ = edges

    class NoLaunch:
        def __getattr__(self, name):
            pytest.fail(f"{name} reached with arguments that must raise first")

    monkeypatch.setattr(_lib, "load", lambda *a, **k: NoLaunch())
    ok = dict(tri=dev(tri), tri_start=dev(start), link_T=dev(link_T), pts=dev(pts), pt_start=dev(pt_start))
    call = lambda d_max=0.01, **kw: ops.mesh_cover(*{**ok, **kw}.values(), d_max)
    for bad in (-1e-9, float("nan")):
        with pytest.raises(ValueError, match="d_max"):
            call(bad)
    with pytest.raises(ValueError, match="pt_start"):
        call(pt_start=dev(pt_start + 1))
    with pytest.raises(ValueError, match="tri_start"):
        call(tri_start=dev(start[::-1].copy()))
    with pytest.raises(ValueError, match="expected"):
        call(pts=dev(pts[:, :2]))
    with pytest.raises(TypeError):
        call(pts=dev(pts.astype(np.float32)))


# ------------------------------------------------------------------------------------------ the measurement
def test_a_link_without_points_shows_in_coverage_and_not_in_surface_distance(tmp_path):
    """The toy robot at the first two poses of DRIVER_Q_TRUE, 4000 surface samples per pose by area (one generator, seed 5), link
    l2's samples removed, d_max = 0.01, the meshes subdivided to max_edge = 0.02 (8376 triangles).  On the restatement, on the
    CPU, for this scene: l2 uncovered 0.884, never 0.864, every other link 0.000 both; with the full clouds every link 0.000.
    The forward direction explains every point of the thinned clouds within d_max: the blind spot, shown."""
    from autourdf_amd import ops
    env = ref.toy(tmp_path)
    r = env.robot
    q = r.q_rows(list(pfref.DRIVER_Q_TRUE[:2]))
    link_T = ops.urdf_fk(r.fk_table(), q, np.eye(4))
    T = link_T.cpu().numpy()
    rng = np.random.default_rng(5)
    l2 = r.link_index["l2"]
    full, cut = [], []
    for p in range(2):
        x, f = pfref.surface_points(pref.posed_mesh(r.tri, r.tri_start, T[p]), 4000, rng)
        full.append(x)
        cut.append(x[(f < r.tri_start[l2]) | (f >= r.tri_start[l2 + 1])])
    cover = env.surface_coverage(link_T, cut, 0.01, max_edge=0.02)
    assert cover["dist"].shape == cover["n_near"].shape == (2, len(cover["parent_row"])) and cover["dist"].shape[1] > len(r.tri)
    by = {l["link"]: l for l in cover["links"]}
    print("coverage without l2's points:", {k: (round(v["uncovered"], 3), round(v["never"], 3)) for k, v in by.items()})
    assert by["l2"]["uncovered"] > 0.5 and by["l2"]["never"] > 0.5
    assert all(v["uncovered"] < 0.05 for k, v in by.items() if k != "l2")
    assert abs(cover["all"]["area"] - sum(v["area"] for v in by.values())) <= 1e-12 and len(cover["poses"]) == 2
    dist, _, link = env.surface_distance(link_T, cut, 0.01)
    assert all(np.isfinite(d).all() for d in dist) and all((l >= 0).all() for l in link)          # every point explained
    whole = env.surface_coverage(link_T, full, 0.01, max_edge=0.02)
    print("coverage with the full clouds:", {l["link"]: round(l["uncovered"], 3) for l in whole["links"]})
    assert all(l["uncovered"] < 0.05 for l in whole["links"])
    coarse = env.surface_coverage(link_T, cut, 0.01)             # the triangle is the resolution: as loaded, l2's 12 hide most of it
    assert "parent_row" not in coarse and coarse["dist"].shape == (2, len(r.tri))
    assert {l["link"]: l for l in coarse["links"]}["l2"]["uncovered"] < by["l2"]["uncovered"]


# ------------------------------------------------------------------------------------------ the command line
@pytest.mark.filterwarnings("ignore:autourdf_amd.prefer_device_kernargs")     # main() in this process: the runtime is up already
def test_command_line_coverage(golden, tmp_path, monkeypatch, capsys):
    """test_command_line_cloud_fit's fixture layout.  Its clouds are random, so the figures are compared with a recomputation,
    not judged."""
    from test_gpu_cloud_fit import _layout

    from autourdf_amd import compute_joints, coord_map, ops
    robot, cams, step = "testbot", 20, 4
    S, T, K = _layout(tmp_path, golden, robot, cams, step)
    out_dir = tmp_path / f"data/urdf/{robot}_{K}_seg"
    stem = f"{step}_deg_{cams}_cams"
    monkeypatch.chdir(tmp_path)
    base = ["--robot", robot, "--unknown_dof", "--end_video", "2", "--voxel_size", "0.01", "--joint_limits", "--cloud_fit", "--fit_max", "0.05"]
    # without the option: no mesh-cover launch, no such key
    monkeypatch.setattr(compute_joints, "ops", cref.OpsWith(ops, mesh_cover=lambda *a, **k: pytest.fail("mesh_cover called without --coverage")))
    coord_map.main(base)
    plain = json.loads((out_dir / (stem + ".cloud_fit.json")).read_text())
    plain_bytes, listing = (out_dir / (stem + ".cloud_fit.json")).read_bytes(), sorted(os.listdir(out_dir))
    assert "coverage" not in plain
    monkeypatch.undo()
    monkeypatch.chdir(tmp_path)
    # with it
    seen = []
    cover = compute_joints.surface_cover_poses
    monkeypatch.setattr(compute_joints, "surface_cover_poses", lambda *a, **k: seen.append(cover(*a, **k)) or seen[-1])
    capsys.readouterr()
    coord_map.main(base + ["--coverage"])
    text = capsys.readouterr().out
    assert sorted(os.listdir(out_dir)) == listing
    report = json.loads((out_dir / (stem + ".cloud_fit.json")).read_text())
    block = report.pop("coverage")
    assert report == plain and json.dumps(report, indent=1).encode() == plain_bytes            # every other key, to the byte
    assert sorted(block) == ["all", "frames", "links", "sequences"]
    assert len(block["frames"]) == S * T and len(block["sequences"]) == S and len(block["links"]) == 6
    assert [(f["sequence"], f["step"]) for f in block["frames"]] == [(p // T, p % T) for p in range(S * T)]
    (got,) = seen
    for f, want in zip(block["frames"], got["poses"]):
        assert f["uncovered"] == want["uncovered"] and f["area"] == want["area"] and f["thin"] == want["thin"]
        assert f["rms"] == (want["rms"] if np.isfinite(want["rms"]) else None)
    assert [l["never"] for l in block["links"]] == [l["never"] for l in got["links"]] and block["all"]["never"] == got["all"]["never"]
    assert 0.0 <= block["all"]["uncovered"] <= 1.0 and got["dist"].shape[0] == S * T
    lines = [x for x in text.splitlines() if x.startswith("coverage seq")]
    assert len(lines) == S and all("uncovered" in x and "rms" in x for x in lines)
    lines = [x for x in text.splitlines() if x.startswith("coverage link_")]
    assert len(lines) == 6 and all("uncovered" in x and "never" in x for x in lines)
    assert text.index("cloud_fit seq0") < text.index("coverage seq0")                    # it runs after the cloud fit
    # the key of parameters.json without the cloud fit: before anything is read or written
    (tmp_path / "parameters.json").write_text(json.dumps({robot: {"num_seg": K, "dof": 5, "coverage": True}}))
    before = (out_dir / (stem + ".cloud_fit.json")).read_bytes()
    with pytest.raises(ValueError, match="coverage"):
        coord_map.main(["--robot", robot, "--unknown_dof", "--end_video", "2", "--voxel_size", "0.01", "--joint_limits"])
    assert (out_dir / (stem + ".cloud_fit.json")).read_bytes() == before
