"""creg_point_mesh_f64 on the GPU against the numpy restatement of its contract (tests/_point_mesh_ref.py): values on a distance
scale, the inf / -1 pattern, the chosen rows; analytic cases, links and poses of every size around a tile, the toy robot, determinism
bit for bit, NaN points, sentinels, invalid calls -- then SimEnv.surface_distance and compute_joints.cloud_fit_poses.

The value bound is the one the clearance tests hold the same arithmetic to: |dist - dist_ref| <= 1e-12 x the scene's diagonal.
Edge and vertex regions make exact ties between neighbouring triangles the common case, so a chosen row is checked by its restated
d2, not by equality with numpy's row; the share of equal rows is printed."""
import ctypes

import numpy as np
import pytest
import torch

import _collide_ref as ref
import _point_mesh_ref as pref

pytestmark = pytest.mark.gpu
INF = np.inf
EPS = np.finfo(np.float64).eps


def dev(a):
    return torch.from_numpy(np.array(a)).to("cuda")              # a copy: the shared host arrays stay as they are


def run(tri, start, link_T, pts, pt_start, d_max, pad=0):
    """dist2, tri_idx, link_box of the C entry (ops.point_mesh_distance returns distances, masked at d_max).  ``pad`` rows of
    sentinels follow the outputs and the workspace's stated size; they must come back untouched."""
    from autourdf_amd import _lib
    lib = _lib.load()
    link_T = np.asarray(link_T, np.float64)
    link_T = link_T[None] if link_T.ndim == 3 else link_T
    pts = np.asarray(pts, np.float64).reshape(-1, 3)
    P, L, F, N = link_T.shape[0], link_T.shape[1], len(tri), len(pts)
    d_tri, d_start, d_T, d_pts, d_ps = dev(tri), dev(start), dev(link_T), dev(pts), dev(np.asarray(pt_start, np.int64))
    need = lib.creg_point_mesh_workspace_bytes(F, L, P, N)
    assert need > 0 and need % 8 == 0
    ws = torch.full((need // 8 + pad,), -7.0, dtype=torch.float64, device="cuda")
    dist2 = torch.full((N + pad,), -7.0, dtype=torch.float64, device="cuda")
    idx = torch.full((N + pad,), -7, dtype=torch.int32, device="cuda")
    box = torch.full((P, L, 6), -7.0, dtype=torch.float64, device="cuda")
    ptr = lambda t: ctypes.c_void_p(t.data_ptr()) if t.numel() else None
    rc = lib.creg_point_mesh_f64(ptr(d_tri), ptr(d_start), F, ptr(d_T), L, P, ptr(d_pts), ptr(d_ps), N, float(d_max), ptr(dist2),
                                 ptr(idx), ptr(box), ptr(ws), need, None)
    assert rc == 0, lib.creg_last_error()
    torch.cuda.synchronize()
    assert (dist2[N:] == -7.0).all() and (idx[N:] == -7).all() and (ws[need // 8:] == -7.0).all()
    return dist2[:N].cpu().numpy(), idx[:N].cpu().numpy(), box.cpu().numpy()


def check(got, want, tri, start, link_T, pts, pt_start, d_max, what=""):
    """The value, inf-pattern and row checks of one call; `want` is the restatement's (dist2, tri_idx, box)."""
    tri = np.asarray(tri, np.float64).reshape(-1, 3, 3)
    link_T = np.asarray(link_T, np.float64)
    link_T = link_T[None] if link_T.ndim == 3 else link_T
    pts = np.asarray(pts, np.float64).reshape(-1, 3)
    bound = 1e-12 * pref.scene_diagonal(tri, start, link_T, pts)
    g2, gi, gbox = got
    w2, wi, wbox = want
    assert g2.shape == w2.shape and gi.shape == wi.shape and g2.dtype == np.float64 and gi.dtype == np.int32
    np.testing.assert_array_equal(gbox, wbox)
    np.testing.assert_array_equal(np.isinf(g2), np.isinf(w2))                   # the inf pattern, exactly
    np.testing.assert_array_equal(gi == -1, wi == -1)
    assert ((gi == -1) == np.isinf(g2)).all() and not np.isnan(g2).any() and (g2 >= 0).all()
    fin = np.isfinite(w2)
    diff = np.abs(np.sqrt(g2[fin]) - np.sqrt(w2[fin]))
    same = float((gi[fin] == wi[fin]).mean()) if fin.any() else 1.0
    print(f"{what}: {fin.sum()} finite of {fin.size}, largest |d - d_ref| {diff.max() if fin.any() else 0.0:.3g} (bound {bound:.3g}), "
          f"bits identical: {g2.tobytes() == w2.tobytes()}, share of equal rows: {same:.4f}")
    assert (diff <= bound).all()
    dmax2 = np.float64(d_max) * np.float64(d_max)
    for p in range(link_T.shape[0]):
        s, e = int(pt_start[p]), int(pt_start[p + 1])
        k = np.flatnonzero(fin[s:e]) + s
        if len(k) == 0:
            continue
        W = pref.posed_mesh(tri, start, link_T[p])
        f = gi[k]
        assert (f >= 0).all() and (f < len(tri)).all()
        assert (pref.point_gap2(pts[k], W[f].min(1), W[f].max(1)) <= dmax2).all()          # the chosen row contributes
        assert (np.abs(np.sqrt(pref.tri_d2(W, f, pts[k])) - np.sqrt(w2[k])) <= bound).all()  # and attains the restated minimum


# ------------------------------------------------------------------------------------------ analytic cases through ops
def through_ops(mesh, pts, d_max=INF, **kw):
    from autourdf_amd import ops
    tri, start = ref.pack([mesh])
    pts = np.asarray(pts, np.float64).reshape(-1, 3)
    out = ops.point_mesh_distance(dev(tri), dev(start), dev(np.eye(4)[None]), dev(pts), dev(np.array([0, len(pts)])), d_max, **kw)
    assert out[0].dtype == torch.float64 and out[1].dtype == torch.int32 and out[2].dtype == torch.int32
    assert all(tuple(o.shape) == (len(pts),) for o in out)
    return tuple(o.cpu().numpy() for o in out)


def test_one_triangle_in_every_voronoi_region_and_the_unit_cube():
    names = sorted(pref.ONE_TRIANGLE)
    dist, idx, link = through_ops([pref.TRI], [pref.ONE_TRIANGLE[n][0] for n in names])
    want = np.array([pref.ONE_TRIANGLE[n][1] for n in names])
    assert (idx == 0).all() and (link == 0).all()
    assert np.abs(dist - want).max() <= 4 * EPS * 8.0 and dist[names.index("on_triangle")] == 0.0
    names = sorted(pref.CUBE_CASES)
    dist, idx, link = through_ops(pref.CUBE, [pref.CUBE_CASES[n][0] for n in names])
    want = np.array([pref.CUBE_CASES[n][1] for n in names])
    assert ((idx >= 0) & (idx < 12)).all() and (link == 0).all() and np.abs(dist - want).max() <= 4 * EPS * 4.0


def test_tie_rule_gate_and_degenerate_triangles_as_the_restatement_has_them():
    far = [[9, 9, 9], [10, 9, 9], [9, 10, 9]]
    pts = [[1, 1, pref.H], [np.nan, 0, 0], [1, 1, 3.0], [9.25, 9.25, 9.0]]
    for sort in (True, False):
        dist, idx, link = through_ops([pref.TRI, far, pref.TRI], pts, 1.0, sort=sort)
        assert idx.tolist() == [0, -1, -1, 1] and link.tolist() == [0, -1, -1, 0]
        assert dist[0] == pref.H and np.isinf(dist[1]) and np.isinf(dist[2]) and dist[3] == 0.0
        dist, idx, _ = through_ops([far, pref.TRI, pref.TRI], pts, INF, sort=sort)
        assert idx.tolist() == [1, -1, 1, 0] and dist[2] == 3.0
    dist, idx, _ = through_ops([[[1, 1, 1], [1, 1, 1], [1, 1, 1]], [[0, 0, 0], [2, 0, 0], [1, 0, 0]]], [[1, 1, 3], [1, -2, 0]])
    assert idx.tolist() == [0, 1] and dist.tolist() == [2.0, 2.0]
    dist, idx, _ = through_ops([pref.TRI], [[3.0, 3.0, 0.0]], 0.5)                 # a small box gap, a larger distance: masked, the row stays
    assert idx.tolist() == [0] and np.isinf(dist[0])


# ------------------------------------------------------------------------------------------ the edges of the tiling
LINK_SIZES = (0, 1, 255, 256, 257, 513)
POSE_POINTS = (0, 1, 255, 256, 257, 63, 64, 65, 0)               # an empty first and last pose; around the 64-point tile as well


@pytest.fixture(scope="module")
def tiling():
    rng = np.random.default_rng(11)
    meshes = [np.zeros((0, 3, 3)) if n == 0 else np.array([[[-0.15, -0.1, 0.0], [0.15, -0.1, 0.0], [0.0, 0.2, 0.0]]]) if n == 1
              else ref.uv_sphere(0.1, n=n) for n in LINK_SIZES]
    tri, start = ref.pack(meshes)
    P, L = len(POSE_POINTS), len(LINK_SIZES)
    link_T = np.array([[ref.rigid(ref.random_rotation(rng), rng.uniform(-0.15, 0.15, 3)) for _ in range(L)] for _ in range(P)])
    pt_start = np.concatenate([[0], np.cumsum(POSE_POINTS)]).astype(np.int64)
    pts = []
    for p, n in enumerate(POSE_POINTS):
        W = pref.posed_mesh(tri, start, link_T[p])
        on = W[rng.integers(0, len(W), n), rng.integers(0, 3, n)]                  # posed vertices: inside their triangle's box
        off = rng.uniform(-0.3, 0.3, (n, 3))
        pts.append(np.where((np.arange(n) % 3 == 0)[:, None], on, off))
    pts = np.concatenate(pts)
    full = pref.point_mesh(tri, start, link_T, pts, pt_start, INF)
    half = float(np.median(np.sqrt(full[0])))
    out = (tri, start, link_T, pts, pt_start, half)
    for a in out[:5] + full:
        a.setflags(write=False)
    return out + (full,)


@pytest.mark.parametrize("which", ["zero", "half", "inf"])
def test_links_and_poses_of_every_size_around_a_tile(tiling, which):
    """Links of 0, 1, 255, 256, 257 and 513 triangles; poses owning 0, 1, 255, 256, 257, 63, 64, 65 and 0 points, every third point
    a posed vertex, the others anywhere in the scene."""
    tri, start, link_T, pts, pt_start, half, full = tiling
    d_max = {"zero": 0.0, "half": half, "inf": INF}[which]
    want = full if which == "inf" else pref.point_mesh(tri, start, link_T, pts, pt_start, d_max)
    got = run(tri, start, link_T, pts, pt_start, d_max, pad=300)
    check(got, want, tri, start, link_T, pts, pt_start, d_max, f"tiling d_max={d_max:.4g}")
    share = np.isfinite(want[0]).mean()
    assert {"zero": 0.2 < share < 0.5, "half": 0.35 < share < 0.8, "inf": share == 1.0}[which], share
    if which != "inf":                                           # a finite d_max equals +inf's result wherever that is within it
        inside = full[0] <= d_max * d_max
        np.testing.assert_array_equal(got[0][inside], full[0][inside])


def test_one_pose_from_a_3d_link_T_and_the_wrapper_s_own_rules(tiling):
    from autourdf_amd import ops
    tri, start, link_T, pts, pt_start, half, _ = tiling
    s, e = int(pt_start[4]), int(pt_start[5])
    one = np.array([0, e - s])
    want = pref.point_mesh(tri, start, link_T[4], pts[s:e], one, half)
    got = run(tri, start, link_T[4], pts[s:e], one, half)
    check(got, want, tri, start, link_T[4], pts[s:e], one, half, "one pose")
    for sort in (True, False):
        dist, idx, link, box = ops.point_mesh_distance(dev(tri), dev(start), dev(link_T[4]), dev(pts[s:e]), dev(one), half,
                                                       sort=sort, want_boxes=True)
        wd, wi, wl = pref.wrapper(got[0], got[1], start, half)
        np.testing.assert_allclose(dist.cpu().numpy(), wd, rtol=4e-16, atol=0)            # the wrapper's own sqrt
        np.testing.assert_array_equal(idx.cpu().numpy(), wi)
        np.testing.assert_array_equal(link.cpu().numpy(), wl)
        np.testing.assert_array_equal(box.cpu().numpy(), got[2])
        assert tuple(box.shape) == (1, len(LINK_SIZES), 6) and (wl >= 1).sum() > 0 and (wl == -1).sum() > 0 and not (wl == 0).any()
    none = run(tri, start, link_T, np.zeros((0, 3)), np.zeros(len(POSE_POINTS) + 1, np.int64), half)
    np.testing.assert_array_equal(none[2], pref.point_mesh(tri, start, link_T, np.zeros((0, 3)), np.zeros(len(POSE_POINTS) + 1, np.int64), half)[2])


# ------------------------------------------------------------------------------------------ determinism, bit for bit
def test_two_runs_alone_or_among_others_permuted_sorted_or_not(tiling):
    from autourdf_amd import ops
    tri, start, link_T, pts, pt_start, half, _ = tiling
    rng = np.random.default_rng(3)
    for d_max in (half, INF):
        a, b = run(tri, start, link_T, pts, pt_start, d_max), run(tri, start, link_T, pts, pt_start, d_max)
        for x, y in zip(a, b):
            assert x.tobytes() == y.tobytes()
        for p in (1, 3, 4, 6):                                   # a pose alone
            s, e = int(pt_start[p]), int(pt_start[p + 1])
            one = run(tri, start, link_T[p], pts[s:e], [0, e - s], d_max)
            assert one[0].tobytes() == a[0][s:e].tobytes() and one[1].tobytes() == a[1][s:e].tobytes()
        s, e = int(pt_start[3]), int(pt_start[4])
        for i in (s, s + 100, e - 1):                            # a point alone
            one = run(tri, start, link_T[3], pts[i:i + 1], [0, 1], d_max)
            assert one[0].tobytes() == a[0][i:i + 1].tobytes() and one[1].tobytes() == a[1][i:i + 1].tobytes()
        perm = np.concatenate([rng.permutation(int(n)) + int(s0) for s0, n in zip(pt_start[:-1], POSE_POINTS)])
        shuffled = run(tri, start, link_T, pts[perm], pt_start, d_max)
        assert shuffled[0].tobytes() == a[0][perm].tobytes() and shuffled[1].tobytes() == a[1][perm].tobytes()
        args = (dev(tri), dev(start), dev(link_T), dev(pts), dev(pt_start), d_max)
        srt, raw = ops.point_mesh_distance(*args, sort=True), ops.point_mesh_distance(*args, sort=False)
        for x, y in zip(srt, raw):
            assert torch.equal(x, y)
        assert raw[1].cpu().numpy().tobytes() == a[1].tobytes()
        assert torch.equal(raw[0], torch.where(dev(a[0]) > d_max * d_max, torch.full_like(raw[0], INF), torch.sqrt(dev(a[0]))))


# ------------------------------------------------------------------------------------------ hygiene
def test_a_nan_point_gets_inf_and_its_neighbours_keep_their_bits(tiling):
    tri, start, link_T, pts, pt_start, half, _ = tiling
    for d_max in (half, INF):
        clean = run(tri, start, link_T, pts, pt_start, d_max)
        dirty = np.array(pts)
        rows = [int(pt_start[2]) + 7, int(pt_start[3]), int(pt_start[4]) + 256, int(pt_start[4]) + 3]   # row 768, the 257th point of its pose, is a tile of its own
        for k, i in enumerate(rows):
            dirty[i, k % 3] = np.nan
        dirty[rows[3]] = np.nan
        got = run(tri, start, link_T, dirty, pt_start, d_max, pad=64)
        assert np.isinf(got[0][rows]).all() and (got[1][rows] == -1).all()
        keep = np.ones(len(pts), bool)
        keep[rows] = False
        assert got[0][keep].tobytes() == clean[0][keep].tobytes() and got[1][keep].tobytes() == clean[1][keep].tobytes()
        check(got, pref.point_mesh(tri, start, link_T, dirty, pt_start, d_max), tri, start, link_T, dirty, pt_start, d_max, "nan points")
    alone = run(tri, start, link_T[:1], np.full((3, 3), np.nan), [0, 3], INF)   # a tile without a live point
    assert np.isinf(alone[0]).all() and (alone[1] == -1).all()


class _NoLaunch:
    def __getattr__(self, name):
        pytest.fail(f"{name} reached with arguments that must raise first")


def test_wrapper_raises_before_any_launch(tiling, monkeypatch):
    from autourdf_amd import _lib, ops
    tri, start, link_T, pts, pt_start, _, _ = tiling
    monkeypatch.setattr(_lib, "load", lambda *a, **k: _NoLaunch())
    ok = dict(tri=dev(tri), tri_start=dev(start), link_T=dev(link_T), pts=dev(pts), pt_start=dev(pt_start))
    call = lambda d_max=0.01, **kw: ops.point_mesh_distance(*{**ok, **kw}.values(), d_max)
    for bad in (-1e-9, float("nan"), -INF):
        with pytest.raises(ValueError, match="d_max"):
            call(bad)
    down = np.array(pt_start)
    down[2], down[3] = down[3], down[2]
    for bad in (down, pt_start + 1, np.concatenate([[1], pt_start[1:]]), np.concatenate([pt_start[:-1], [len(pts) - 1]])):
        with pytest.raises(ValueError, match="pt_start"):
            call(pt_start=dev(bad))
    with pytest.raises(ValueError, match="tri_start"):
        call(tri_start=dev(start[::-1].copy()))
    for kw in (dict(pt_start=dev(pt_start[:-1])), dict(tri_start=dev(start[:-1])), dict(pts=dev(pts[:, :2])), dict(pts=dev(pts.reshape(-1))),
               dict(tri=dev(tri.reshape(-1, 9))), dict(link_T=dev(link_T[:, :, :3])), dict(link_T=dev(link_T[:3])),
               dict(link_T=dev(link_T[0]))):
        with pytest.raises(ValueError, match="expected"):
            call(**kw)
    for kw in (dict(pts=dev(pts.astype(np.float32))), dict(pt_start=dev(pt_start.astype(np.int32))), dict(tri=dev(tri.astype(np.float32))),
               dict(link_T=dev(link_T.astype(np.float32))), dict(tri_start=dev(start.astype(np.int32)))):
        with pytest.raises(TypeError):
            call(**kw)


def test_invalid_calls_return_einval_and_touch_nothing(tiling):
    """NaN or negative d_max, a short workspace, null pointers, the size limits: CREG_EINVAL, a message naming the entry,
    nothing launched.  A pt_start beyond [0, N] reaches the kernel only through the C ABI: it is clamped, nothing outside the
    arrays is touched."""
    from autourdf_amd import _lib
    lib = _lib.load()
    tri, start, link_T, pts, pt_start, half, full = tiling
    P, L, F, N = link_T.shape[0], link_T.shape[1], len(tri), len(pts)
    d_tri, d_start, d_T, d_pts, d_ps = dev(tri), dev(start), dev(link_T), dev(pts), dev(pt_start)
    need = lib.creg_point_mesh_workspace_bytes(F, L, P, N)
    ws = torch.empty(need // 8, dtype=torch.float64, device="cuda")
    dist2 = torch.full((N + 64,), 77.0, dtype=torch.float64, device="cuda")
    idx = torch.full((N + 64,), 77, dtype=torch.int32, device="cuda")
    box = torch.full((P, L, 6), 77.0, dtype=torch.float64, device="cuda")
    ptr = lambda t: ctypes.c_void_p(t.data_ptr()) if t is not None else None

    def call(n_tri=F, n_links=L, n_poses=P, n_pts=N, d_max=0.02, ws_bytes=need, x=d_pts, ps=d_ps, d2=dist2, ix=idx, w=ws, t=d_tri):
        return lib.creg_point_mesh_f64(ptr(t), ptr(d_start), n_tri, ptr(d_T), n_links, n_poses, ptr(x), ptr(ps), n_pts, d_max, ptr(d2),
                                       ptr(ix), ptr(box), ptr(w), ws_bytes, None)

    for kw in (dict(d_max=float("nan")), dict(d_max=-0.01), dict(d_max=-INF), dict(ws_bytes=need - 8), dict(ws_bytes=0), dict(d2=None),
               dict(ix=None), dict(x=None), dict(ps=None), dict(w=None), dict(t=None), dict(n_tri=1 << 31), dict(n_links=65536),
               dict(n_poses=0), dict(n_pts=-1), dict(n_pts=1 << 31), dict(n_links=0), dict(n_tri=-1)):
        assert call(**kw) == -1, kw                               # CREG_EINVAL
        assert b"creg_point_mesh_f64" in lib.creg_last_error()
        torch.cuda.synchronize()
        assert (dist2 == 77.0).all() and (idx == 77).all() and (box == 77.0).all(), kw
    wild = np.array(pt_start)
    wild[0], wild[-1] = -5, N + 1000                             # pose 0 now owns rows 0 .. pt_start[1] = 0: still none; the last pose runs to N
    assert call(d_max=INF, ps=dev(wild)) == 0
    torch.cuda.synchronize()
    assert (dist2[N:] == 77.0).all() and (idx[N:] == 77).all()
    assert dist2[:N].cpu().numpy().tobytes() == full[0].tobytes()
    assert call(d_max=INF, n_pts=0, x=None, d2=None, ix=None) == 0                # N = 0 needs no outputs and fills the boxes
    torch.cuda.synchronize()
    np.testing.assert_array_equal(box.cpu().numpy(), full[2])


# ------------------------------------------------------------------------------------------ the toy robot through the layers
@pytest.fixture(scope="module")
def env(tmp_path_factory):
    return ref.toy(tmp_path_factory.mktemp("toy"))


TOY_Q = [{}, {"waist": 0.7, "shoulder": -0.9, "slide": 0.03, "wrist": 1.1}, {"waist": -2.0, "shoulder": 0.8, "slide": 0.05, "wrist": -0.6}]


def toy_poses(env, shift=None):
    """link_T (3,L,4,4) on the device; ``shift`` (3,3) moves each pose's base."""
    from autourdf_amd import ops
    r = env.robot
    link_T = ops.urdf_fk(r.fk_table(), r.q_rows(TOY_Q), env.base)
    if shift is not None:
        move = torch.eye(4, dtype=torch.float64, device="cuda").repeat(3, 1, 1)
        move[:, :3, 3] = dev(np.asarray(shift, np.float64))
        link_T = move[:, None] @ link_T
    return link_T.contiguous()


def toy_samples(env, link_T, n, seed):
    rng = np.random.default_rng(seed)
    return [env.sample_surface(None, n, rng, link_T=link_T[p].contiguous()).cpu().numpy() for p in range(link_T.shape[0])]


def test_toy_surface_samples_lie_on_the_meshes_and_pushed_ones_match_the_restatement(env):
    r = env.robot
    assert len(r.tri) == 600
    link_T = toy_poses(env)
    clouds = toy_samples(env, link_T, 700, 0)                    # 700: three tiles per pose, the last one partial
    T = link_T.cpu().numpy()
    pts = np.concatenate(clouds)
    cut = np.arange(4) * 700
    bound = 1e-12 * pref.scene_diagonal(r.tri, r.tri_start, T, pts)
    dist, tri, link = env.surface_distance(link_T, clouds)
    assert len(dist) == len(tri) == len(link) == 3 and all(d.shape == (700,) for d in dist)
    print(f"toy, on the surface: largest distance {max(d.max() for d in dist):.3g} (bound {bound:.3g})")
    assert all((d <= bound).all() for d in dist) and all((l >= 0).all() and (l < len(r.links)).all() for l in link)
    assert all((r.tri_link[t] == l).all() for t, l in zip(tri, link))
    rng = np.random.default_rng(1)
    push = rng.normal(size=pts.shape)
    pushed = pts + 0.01 * push / np.linalg.norm(push, axis=1, keepdims=True)
    for d_max in (INF, 0.008):
        want = pref.point_mesh(r.tri, r.tri_start, T, pushed, cut, d_max)
        got = run(r.tri, r.tri_start, T, pushed, cut, d_max)
        check(got, want, r.tri, r.tri_start, T, pushed, cut, d_max, f"toy pushed, d_max={d_max}")
        wd = pref.wrapper(want[0], want[1], r.tri_start, d_max)[0]
        dist = np.concatenate(env.surface_distance(link_T, [pushed[cut[p]:cut[p + 1]] for p in range(3)], d_max)[0])
        np.testing.assert_array_equal(np.isinf(dist), np.isinf(wd))
        assert np.abs(dist[np.isfinite(wd)] - wd[np.isfinite(wd)]).max() <= bound and (wd[np.isfinite(wd)] <= 0.01 + bound).all()
        if d_max != INF:
            assert 0.05 < np.isinf(wd).mean() < 0.95              # 0.008 cuts the pushed set: inside corners are nearer than 0.01


def test_cloud_fit_poses_on_the_toy_robot_and_with_one_link_displaced(env):
    from autourdf_amd.compute_joints import cloud_fit_poses
    r = env.robot
    shift = np.array([[0.0, 0.0, 0.0], [0.011, -0.007, 0.004], [-0.009, 0.012, -0.006]])
    link_T = toy_poses(env, shift)
    T = link_T.cpu().numpy()
    clouds = toy_samples(env, link_T, 500, 2)
    pts, cut = np.concatenate(clouds), np.arange(4) * 500
    bound = 1e-12 * pref.scene_diagonal(r.tri, r.tri_start, T, pts)
    fit = cloud_fit_poses(r, link_T, clouds)
    want = pref.wrapper(*pref.point_mesh(r.tri, r.tri_start, T, pts, cut, INF)[:2], r.tri_start, INF)
    assert [p["n"] for p in fit["poses"]] == [500] * 3 and fit["all"]["n"] == 1500
    assert all(p["unexplained"] == 0 and p["rms"] <= bound and p["max"] <= bound for p in fit["poses"])
    assert fit["all"]["unexplained"] == 0 and fit["all"]["rms"] <= bound
    assert [l["link"] for l in fit["links"]] == list(r.links)
    assert [l["n"] for l in fit["links"]] == [int((want[2] == i).sum()) for i in range(len(r.links))]
    assert sum(l["n"] for l in fit["links"]) == 1500 and all(l["n"] > 0 for l in fit["links"])
    np.testing.assert_array_equal(np.concatenate(fit["link"]), want[2])
    assert np.abs(np.concatenate(fit["dist"]) - want[0]).max() <= bound
    # the unshifted poses do not explain the shifted clouds
    off = cloud_fit_poses(r, toy_poses(env), clouds)
    assert off["poses"][0]["rms"] <= bound and off["poses"][1]["rms"] > 1e-3 and off["poses"][2]["rms"] > 1e-3
    # link l2 displaced by 0.02 before sampling: its own figures move, and it is the worst link
    l2 = r.link_index["l2"]
    moved = link_T.clone()
    moved[:, l2, :3, 3] += dev(np.array([0.0, 0.02, 0.0]))
    clouds = toy_samples(env, moved.contiguous(), 500, 3)
    pts = np.concatenate(clouds)
    fit = cloud_fit_poses(r, link_T, clouds, 0.05)
    wd, _, wl = pref.wrapper(*pref.point_mesh(r.tri, r.tri_start, T, pts, cut, 0.05)[:2], r.tri_start, 0.05)
    for i, l in enumerate(fit["links"]):
        d = wd[np.isfinite(wd) & (wl == i)]
        assert l["n"] == len(d) and abs(l["rms"] - np.sqrt((d * d).sum() / len(d))) <= bound
    worst = max(fit["links"], key=lambda l: l["rms"])
    assert worst["link"] == "l2" and 0.002 < worst["rms"] <= 0.02 + bound
    p, row = fit["all"]["max_at"]
    assert fit["dist"][p][row] == fit["all"]["max"] == max(q["max"] for q in fit["poses"]) and fit["poses"][p]["max_at"] == row
    for q, d in zip(fit["poses"], fit["dist"]):
        ok = np.isfinite(d)
        assert q["unexplained"] == int((~ok).sum()) and abs(q["mean"] - d[ok].mean()) <= bound
        assert abs(q["p95"] - np.percentile(d[ok], 95)) <= bound
