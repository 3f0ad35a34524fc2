"""GPU: exact convex hulls of lattice point sets (hull.hip through ops.lattice_hull and the C ABI; DESIGN N4).  Every case
runs the full certificate of tests/_hull_ref.py on the host -- closed, oriented, genus 0, no flat face, no point above any
face, all in exact integers -- and where Qhull or the brute-force hull is at hand also the extreme set and the exact volume.
The face table of the kernel lives in the workspace, not in LDS, so there is no table size to cross; the cases above 256 face
slots (the workgroup's stride over the table) are the ball, the ellipsoid shell and the random sets of 1025 points."""
import ctypes
import os
import sys

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu
HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import _hull_ref as H  # noqa: E402


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available()
    return torch.device("cuda")


def ops():
    from autourdf_amd import ops as o
    return o


def run(links, dev, **kw):
    pts, off = H.pack(links)
    return ops().lattice_hull(torch.from_numpy(pts).to(dev), off, **kw)


def certified(P, res, extreme_xyz=None):
    """The full certificate of one link's result; returns (triangles, 6 x volume)."""
    assert res["status"] == 0
    T = res["triangles"].cpu().numpy()
    assert T.dtype == np.int32
    bad = H.certificate(P, T, extreme_xyz)
    assert bad == [], bad
    ids = res["vertex_ids"].cpu().numpy()
    assert (ids == np.unique(T)).all()
    return T, H.volume6(P, T)


@pytest.fixture(scope="module")
def ball():
    P = H.lattice_ball(12)
    T, ext = H.scipy_hull(P)
    return P, P[ext], H.volume6(P, T)


# ------------------------------------------------------------------------------------------------ smallest meshes
def test_one_voxel_two_voxels_a_tetrahedron_and_a_tetrahedron_with_its_centroid(dev):
    octa, two = H.voxel_verts(np.ones((1, 1, 1), bool)), H.voxel_verts(np.ones((2, 1, 1), bool))
    tet = np.array([[0, 0, 0], [4, 0, 0], [0, 4, 0], [0, 0, 4]], np.int32)
    tetc = np.concatenate([tet, [[1, 1, 1]]]).astype(np.int32)
    for P, faces, verts in ((octa, 8, 6), (two, 16, 10), (tet, 4, 4), (tetc, 4, 4)):
        Tb, eb = H.brute_hull(P)
        T, vol = certified(P, run([P], dev)[0], P[eb])
        print(len(P), "points:", len(T), "faces, 6 x volume", vol)
        assert len(T) == faces and len(np.unique(T)) == verts and vol == H.volume6(P, Tb)
    assert 4 not in run([tetc], dev)[0]["vertex_ids"].tolist()          # the centroid is no vertex


# ------------------------------------------------------------------------------------------------ ties
def test_filled_block_every_facet_flat_and_full_of_tied_points(dev):
    P = H.lattice_block(21, 11, 6)
    T, vol = certified(P, run([P], dev)[0], H.block_corners(21, 11, 6))
    print("block:", len(T), "faces on", len(np.unique(T)), "vertices, 6 x volume", vol)
    assert vol == 6 * 20 * 10 * 5


def test_lattice_ball_of_radius_12_plain_shuffled_and_duplicated(dev, ball):
    P, ext, vol6 = ball
    assert len(P) == 7153 and len(ext) == 222
    T, vol = certified(P, run([P], dev)[0], ext)
    print("ball:", len(T), "faces on", len(np.unique(T)), "vertices, 6 x volume", vol, "qhull", vol6)
    assert vol == vol6
    rng = np.random.default_rng(5)
    Q = np.concatenate([P, P[rng.integers(0, len(P), 3000)], ext, ext])   # every extreme point three times at least
    Q = Q[rng.permutation(len(Q))]
    T2, vol2 = certified(Q, run([Q], dev)[0], ext)
    assert vol2 == vol6
    first = {}
    for i, p in enumerate(map(tuple, Q.tolist())):
        first.setdefault(p, i)
    assert all(first[tuple(Q[i])] == i for i in np.unique(T2))            # of equal points the smallest index is the vertex


# ------------------------------------------------------------------------------------------------ exactness at the limit
@pytest.mark.parametrize("extra", ["out", "on", "in", "out on", "on in", "out on in", "on on out out"])
def test_unit_steps_off_a_face_of_the_largest_tetrahedron(dev, extra):
    """Face (0,1,2) of the tetrahedron with corners at +-16383 lies in x + y + z = -16383; its centroid is a lattice point.
    One unit outside must become a vertex, on the face or one unit inside must change nothing: float32, or a product
    contracted into an fma of rounded terms, gets the sign of these determinants (about 1e9 against 1e14) wrong."""
    tet = H.limit_tetra()
    c = -H.LIMIT // 3
    assert 3 * c == -H.LIMIT
    pt = {"out": [c, c, c - 1], "on": [c, c, c], "in": [c, c, c + 1]}
    P = np.concatenate([tet, [pt[w] for w in extra.split()]]).astype(np.int32)
    Tb, eb = H.brute_hull(P)
    T, vol = certified(P, run([P], dev)[0], P[eb])
    base = abs(H.volume6(tet, [[0, 1, 2], [0, 3, 1], [1, 3, 2], [2, 3, 0]]))
    print(extra, "6 x volume", vol, "tetrahedron", base)
    assert vol == H.volume6(P, Tb) and (vol > base) == ("out" in extra) and vol >= base
    used = {tuple(p) for p in P[np.unique(T)].tolist()}
    assert (tuple(pt["out"]) in used) == ("out" in extra) and tuple(pt["in"]) not in used and tuple(pt["on"]) not in used


# ------------------------------------------------------------------------------------------------ sizes
@pytest.mark.parametrize("n", [4, 5, 63, 64, 65, 255, 256, 257, 1025])
def test_random_lattice_points_around_the_wave_and_the_workgroup(dev, n):
    P = H.random_lattice(n, n)
    Ts, ext = H.scipy_hull(P)
    T, vol = certified(P, run([P], dev)[0], P[ext])
    print(n, "points:", len(T), "faces, 6 x volume", vol)
    assert vol == H.volume6(P, Ts)


def test_shells_with_thousands_of_faces_and_of_hull_points(dev):
    """The mesher's vertices of a filled ellipsoid (a shell: nearly every point is near the hull) and 1025 points ON a sphere
    of radius 16000 -- nearly every point extreme, so about a thousand insertions and two thousand faces, eight strides of the
    face table, with determinants near the top of the range."""
    S = H.voxel_verts(H.ellipsoid_occ(23, 17, 12))
    Ts, ext = H.scipy_hull(S)
    T, vol = certified(S, run([S], dev)[0], S[ext])
    print("ellipsoid shell:", len(S), "points,", len(T), "faces, 6 x volume", vol)
    assert vol == H.volume6(S, Ts) and len(T) > 256
    rng = np.random.default_rng(9)
    u = rng.normal(size=(1025, 3))
    Q = np.unique(np.rint(16000 * u / np.linalg.norm(u, axis=1, keepdims=True)).astype(np.int32), axis=0)
    Tq, extq = H.scipy_hull(Q)
    T, vol = certified(Q, run([Q], dev)[0], Q[extq])
    print("sphere:", len(Q), "points,", len(extq), "extreme,", len(T), "faces")
    assert vol == H.volume6(Q, Tq) and len(T) >= 2 * len(extq) - 4


# ------------------------------------------------------------------------------------------------ layout
def test_five_links_of_6_7153_4_1386_257_points_alone_and_together_twice(dev, ball):
    links = [H.voxel_verts(np.ones((1, 1, 1), bool)), ball[0], np.array([[0, 0, 0], [4, 0, 0], [0, 4, 0], [0, 0, 4]], np.int32),
             H.lattice_block(21, 11, 6), H.random_lattice(257, 257)]
    assert [len(p) for p in links] == [6, 7153, 4, 1386, 257]
    origin, vs = np.arange(15, dtype=np.float64).reshape(5, 3) * 0.37 - 2.0, 0.0123
    a = run(links, dev, origin=origin, voxel_size=vs)
    b = run(links, dev, origin=origin, voxel_size=vs)
    for l, P in enumerate(links):
        T, _ = certified(P, a[l], ball[1] if l == 1 else None)
        assert (b[l]["triangles"].cpu().numpy() == T).all()
        rec = a[l]["stl_records"].cpu().numpy()
        assert rec.tobytes() == b[l]["stl_records"].cpu().numpy().tobytes()       # two runs: the same bits
        alone = run([P], dev, origin=origin[l:l + 1], voxel_size=vs)[0]
        assert (alone["triangles"].cpu().numpy() == T).all() and alone["stl_records"].cpu().numpy().tobytes() == rec.tobytes()
        # the records: world = origin + (voxel_size / 2) * v in fp64, rounded to float32; the unit normal of the rounded vertices
        W = (origin[l] + (vs / 2) * P[T].astype(np.float64)).astype(np.float32)
        assert rec.shape == (len(T), 4, 3) and rec.dtype == np.float32 and (rec[:, 1:] == W).all()
        n = np.cross(W[:, 1].astype(np.float64) - W[:, 0], W[:, 2].astype(np.float64) - W[:, 0])
        n /= np.linalg.norm(n, axis=1, keepdims=True)
        err = np.abs(rec[:, 0] - n).max()
        print("link", l, "faces", len(T), "normal error", err)
        assert err <= 2.0 ** -22                                   # one float32 rounding of a component <= 1 (2^-24) and fp64 noise
    assert "stl_records" not in run(links[:1], dev)[0]


def test_degenerate_links_between_good_ones_get_their_status_and_leave_the_neighbours_alone(dev):
    good = [H.voxel_verts(np.ones((1, 1, 1), bool)), H.random_lattice(65, 65), H.random_lattice(64, 64), H.random_lattice(300, 7)]
    flat = np.array([[0, 0, 5], [9, 0, 5], [0, 9, 5], [9, 9, 5], [3, 4, 5], [3, 4, 5]], np.int32)
    line = np.array([[1, 2, 3], [2, 4, 6], [4, 8, 12], [-3, -6, -9], [2, 4, 6]], np.int32)
    three = np.array([[0, 0, 0], [1, 0, 0], [0, 1, 0]], np.int32)
    same = np.full((7, 3), 11, np.int32)
    links = [good[0], flat, good[1], line, three, np.zeros((0, 3), np.int32), good[2], same, good[3]]
    want = [0, 4, 0, 3, 1, 1, 0, 2, 0]
    res = run(links, dev, strict=False)
    assert [r["status"] for r in res] == want
    for r, w in zip(res, want):
        assert (len(r["triangles"]) == 0) == (w != 0) and (len(r["vertex_ids"]) == 0) == (w != 0)
    for l, g in zip((0, 2, 6, 8), good):
        T, _ = certified(g, res[l])
        assert (run([g], dev)[0]["triangles"].cpu().numpy() == T).all()
    with pytest.raises(ValueError, match=r"link 1 .*coplanar"):
        run(links, dev)
    with pytest.raises(ValueError, match=r"link 0 .*fewer than 4"):
        run([three], dev)
    assert [r["status"] for r in run([np.zeros((0, 3), np.int32)], dev, strict=False)] == [1]


def test_every_output_row_is_written_and_nothing_beyond(dev, ball):
    """The C ABI on sentinel-filled buffers with spare rows behind every output and a guarded workspace tail."""
    from autourdf_amd import _lib
    L_ = _lib.load()
    links = [H.random_lattice(257, 3), np.array([[0, 0, 0], [1, 0, 0], [0, 1, 0]], np.int32), ball[0], H.random_lattice(64, 4)]
    pn, off_h = H.pack(links)
    n, L, PAD, SENT = len(pn), len(links), 64, -(2 ** 31) + 5
    pts, off = torch.from_numpy(pn).to(dev), torch.from_numpy(off_h).to(dev)
    p = lambda t: ctypes.c_void_p(t.data_ptr())
    st = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
    wsb = int(L_.creg_lattice_hull_workspace_bytes(n, L))
    ws = torch.full((wsb + PAD,), 0x5a, dtype=torch.uint8, device=dev)
    status = torch.full((L + PAD,), SENT, dtype=torch.int32, device=dev)
    count = torch.full((L + PAD,), SENT, dtype=torch.int32, device=dev)
    assert L_.creg_lattice_hull_i32(p(pts), n, p(off), off_h.ctypes.data, L, -1, p(status), p(count), p(ws), wsb, st) == 0
    assert status[:L].cpu().tolist() == [0, 1, 0, 0] and (status[L:] == SENT).all() and (count[L:] == SENT).all()
    cnt = count[:L].cpu().numpy().astype(np.int64)
    assert cnt[1] == 0 and (cnt[[0, 2, 3]] >= 4).all() and (ws[wsb:] == 0x5a).all()
    toff_h = np.concatenate([[0], np.cumsum(cnt)]).astype(np.int64)
    F = int(toff_h[-1])
    toff = torch.from_numpy(toff_h).to(dev)
    tris = torch.full((F + PAD, 3), SENT, dtype=torch.int32, device=dev)
    rec = torch.full((F + PAD, 4, 3), -7e30, dtype=torch.float32, device=dev)
    origin = torch.zeros(L, 3, dtype=torch.float64, device=dev)
    assert L_.creg_lattice_hull_emit_i32(p(pts), n, p(off), L, p(toff), F, p(origin), 0.01, p(tris), p(rec), p(ws), wsb, st) == 0
    assert (tris[:F] != SENT).all() and (tris[F:] == SENT).all() and (rec[:F] != -7e30).all() and (rec[F:] == -7e30).all()
    assert (ws[wsb:] == 0x5a).all()
    tn = tris[:F].cpu().numpy()
    for l in (0, 2, 3):
        assert H.certificate(links[l], tn[toff_h[l]:toff_h[l + 1]]) == []
    # without records the same triangles, and the records untouched
    tris2 = torch.full((F + PAD, 3), SENT, dtype=torch.int32, device=dev)
    rec.fill_(-7e30)
    assert L_.creg_lattice_hull_emit_i32(p(pts), n, p(off), L, p(toff), F, None, 0.0, p(tris2), None, p(ws), wsb, st) == 0
    assert (tris2 == tris).all() and (rec == -7e30).all()
    torch.cuda.synchronize()


def test_refusals_launch_nothing_and_an_unknown_bound_is_a_status(dev):
    from autourdf_amd import _lib
    L_ = _lib.load()
    good, far = H.random_lattice(64, 1), H.random_lattice(64, 2)
    far[17, 1] = H.LIMIT + 1
    with pytest.raises(ValueError, match="beyond the limit"):
        run([good, far], dev)
    pn, off_h = H.pack([good, far])
    pts = torch.from_numpy(pn).to(dev)
    for bad_off in ([0, 70, 64, 128], [0, 64, 127], [1, 64, 128]):
        with pytest.raises(ValueError, match="offsets"):
            ops().lattice_hull(pts, np.array(bad_off, np.int64))
    with pytest.raises(RuntimeError):
        ops().lattice_hull(pts.cpu(), off_h)
    with pytest.raises(TypeError):
        ops().lattice_hull(pts.long(), off_h)
    with pytest.raises(ValueError, match="go together"):
        ops().lattice_hull(pts, off_h, origin=np.zeros((2, 3)))
    n, L, SENT = len(pn), 2, -(2 ** 31) + 5
    off = torch.from_numpy(off_h).to(dev)
    p = lambda t: ctypes.c_void_p(t.data_ptr())
    st = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
    wsb = int(L_.creg_lattice_hull_workspace_bytes(n, L))
    ws = torch.full((wsb,), 0x5a, dtype=torch.uint8, device=dev)
    status = torch.full((L,), SENT, dtype=torch.int32, device=dev)
    count = torch.full((L,), SENT, dtype=torch.int32, device=dev)
    down = np.array([0, 130, 128], np.int64)
    short = np.array([0, 64, 127], np.int64)
    for args, word in (((p(pts), n, p(off), off_h.ctypes.data, L, H.LIMIT + 1), b"beyond the limit"),
                       ((p(pts), n, p(off), down.ctypes.data, L, -1), b"decrease"),
                       ((p(pts), n, p(off), short.ctypes.data, L, -1), b"from 0 to n"),
                       ((p(pts), n, p(off), None, L, -1), b"null"), ((p(pts), -1, p(off), off_h.ctypes.data, L, -1), b"bad size"),
                       ((p(pts), n, p(off), off_h.ctypes.data, 0, -1), b"bad size")):
        assert L_.creg_lattice_hull_i32(*args, p(status), p(count), p(ws), wsb, st) == -1
        assert word in L_.creg_last_error(), L_.creg_last_error()
    assert L_.creg_lattice_hull_i32(p(pts), n, p(off), off_h.ctypes.data, L, -1, p(status), p(count), p(ws), wsb - 1, st) == -1
    tris = torch.full((8, 3), SENT, dtype=torch.int32, device=dev)
    rec = torch.full((8, 4, 3), -7e30, dtype=torch.float32, device=dev)
    origin = torch.zeros(L, 3, dtype=torch.float64, device=dev)
    toff = torch.zeros(L + 1, dtype=torch.int64, device=dev)
    for vs in (0.0, -1.0, float("nan"), float("inf")):
        assert L_.creg_lattice_hull_emit_i32(p(pts), n, p(off), L, p(toff), 8, p(origin), vs, p(tris), p(rec), p(ws), wsb, st) == -1
    assert L_.creg_lattice_hull_emit_i32(p(pts), n, p(off), L, p(toff), 2 * n + 1, None, 0.0, p(tris), None, p(ws), wsb, st) == -1
    torch.cuda.synchronize()
    assert (status == SENT).all() and (count == SENT).all() and (ws == 0x5a).all() and (tris == SENT).all() and (rec == -7e30).all()
    # the host does not know the bound: the link that holds the coordinate is refused on the device, its neighbour is not
    assert L_.creg_lattice_hull_i32(p(pts), n, p(off), off_h.ctypes.data, L, -1, p(status), p(count), p(ws), wsb, st) == 0
    assert status.cpu().tolist() == [0, 5] and count.cpu().tolist()[1] == 0 and count.cpu().tolist()[0] >= 4


# ------------------------------------------------------------------------------------------------ end to end
def _closed(rec):
    """A binary STL's records as an indexed surface: vertices matched by their exact float32 coordinates."""
    V, inv = np.unique(rec[:, 1:].reshape(-1, 3), axis=0, return_inverse=True)
    T = inv.reshape(-1, 3)
    E = np.concatenate([T[:, [0, 1]], T[:, [1, 2]], T[:, [2, 0]]])
    key, rev = E[:, 0] * len(V) + E[:, 1], E[:, 1] * len(V) + E[:, 0]
    return bool(len(np.unique(key)) == len(key) and np.isin(rev, key).all() and len(V) - len(key) // 2 + len(T) == 2)


def test_link_mesh_with_hulls_writes_closed_hulls_that_contain_their_meshes_and_the_urdf_can_name_them(dev, tmp_path):
    from autourdf_amd import link
    from autourdf_amd.compute_joints import set_collision_meshes
    from autourdf_amd.sim_data import UrdfRobot
    n_links, vs = 4, 0.01
    d = str(tmp_path / "links") + "/"
    os.makedirs(d)
    for i, c in enumerate(H.toy_link_clouds(n_links)):
        link.write_ply(d + f"{i:04}.ply", c)
    assert link.link_mesh([d], n_links - 1, vs, False) is None
    plain = {f: open(d + f, "rb").read() for f in sorted(os.listdir(d))}
    assert sorted(plain) == sorted([f"{i:04}.ply" for i in range(n_links)] + [f"{i:04}.stl" for i in range(n_links)])
    counts = link.link_mesh([d], n_links - 1, vs, False, hull=True)
    assert sorted(os.listdir(d)) == sorted(list(plain) + [f"{i:04}_hull.stl" for i in range(n_links)])
    assert all(open(d + f, "rb").read() == b for f, b in plain.items())              # today's files, byte for byte
    for i in range(n_links):
        mesh, hull = link.read_stl(d + f"{i:04}.stl"), link.read_stl(d + f"{i:04}_hull.stl")
        assert counts[0][i] == (len(mesh), len(hull)) and 4 <= len(hull) < len(mesh)
        assert _closed(hull) and np.isfinite(hull).all()
        a = hull[:, 1].astype(np.float64)
        n = np.cross(hull[:, 2].astype(np.float64) - a, hull[:, 3].astype(np.float64) - a)
        n /= np.linalg.norm(n, axis=1, keepdims=True)
        v = np.unique(mesh[:, 1:].reshape(-1, 3), axis=0).astype(np.float64)
        M = max(np.abs(mesh[:, 1:]).max(), np.abs(hull[:, 1:]).max())
        above = ((v @ n.T) - (n * a).sum(1)).max()
        print(f"link {i}: {len(mesh)} -> {len(hull)} triangles; highest mesh vertex above a hull face {above:.3e}, bound {16 * 2.0 ** -24 * M:.3e}")
        assert above <= 16 * 2.0 ** -24 * M
        assert np.abs(hull[:, 0] - n).max() <= 2.0 ** -22
    urdf = str(tmp_path / "toy.urdf")
    H.write_toy_urdf(urdf, d, n_links)
    visual = np.diff(UrdfRobot(urdf).tri_start).tolist()
    assert all(0 < v <= c[0] for v, c in zip(visual, counts[0]))           # (UrdfRobot drops facets without area)
    set_collision_meshes(urdf)
    assert np.diff(UrdfRobot(urdf, geometry="collision").tri_start).tolist() == [c[1] for c in counts[0]]
    assert np.diff(UrdfRobot(urdf).tri_start).tolist() == visual                       # the default still reads the visuals
