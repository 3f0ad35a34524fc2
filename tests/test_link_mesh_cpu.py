"""CPU: the link mesher's case table, its generator, the numpy restatement the GPU tests compare against (DESIGN N4), and the
host half of link.visualize_links / link.link_mesh (PLY and STL files, the voxel-grid limits)."""
import itertools
import os
import subprocess
import sys

import numpy as np
import pytest

import _link_mesh_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GEN = R.load_generator()


def test_committed_header_is_what_the_generator_emits():
    with open(os.path.join(ROOT, "autourdf_amd", "csrc", "mc_table.h")) as f:
        assert f.read() == GEN.render()
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "gen_mc_table.py"), "--check"])
    assert r.returncode == 0


def test_every_case_uses_exactly_its_active_edges_and_at_most_five_triangles():
    table = GEN.build_table()
    assert len(table) == 256 and sum(len(t) for t in table) == 820
    for m, tris in enumerate(table):
        active = {e for e in range(12) if ((m >> GEN.edge_corners(e)[0]) ^ (m >> GEN.edge_corners(e)[1])) & 1}
        used = {e for t in tris for e in t}
        assert used == active, (m, used, active)
        assert len(tris) <= 5
        assert all(len(set(t)) == 3 for t in tris)
    assert table[0] == [] and table[255] == []


def test_a_faces_segments_depend_on_its_own_four_corners_only():
    """What makes neighbouring cells agree: the segments on a face are a function of (face, its four corners' occupancy)."""
    seen = {}
    for m in range(256):
        by_face = {}
        for f, p, q in GEN.case_segments(m):
            by_face.setdefault(f, []).append((p, q))
        for f, quad in enumerate(GEN.FACES):
            key = (f, tuple((m >> c) & 1 for c in quad))
            segs = sorted(by_face.get(f, []))
            assert seen.setdefault(key, segs) == segs, (m, f)
    assert len(seen) == 6 * 16
    # the face x = 1 of a cell is the face x = 0 of its +x neighbour: same midpoints, opposite directions (each cell sees
    # the face from its own outside), which is what cancels the directed edges of the two cells' triangles there
    for a in range(3):
        lo_face, hi_face = 2 * a, 2 * a + 1
        for occ in itertools.product((0, 1), repeat=4):
            # corners of the low face in ITS order; the same physical corners seen from the other cell differ on axis a
            quad_lo, quad_hi = GEN.FACES[lo_face], GEN.FACES[hi_face]
            val = {c & ~(1 << a): o for c, o in zip(quad_lo, occ)}
            occ_hi = tuple(val[c & ~(1 << a)] for c in quad_hi)
            strip = lambda segs: sorted((GEN.edge_corners(p)[0] & ~(1 << a), GEN.edge_corners(p)[1] & ~(1 << a),
                                         GEN.edge_corners(q)[0] & ~(1 << a), GEN.edge_corners(q)[1] & ~(1 << a)) for p, q in segs)
            lo = strip(GEN.face_segments(quad_lo, occ))
            hi = strip((q, p) for p, q in GEN.face_segments(quad_hi, occ_hi))
            assert lo == hi, (a, occ)


def _check_closed_outward(vol):
    vh, tr = R.marching_cubes(vol)
    assert R.edge_balance(tr)
    if vol.any():
        assert R.six_volume(vh, tr) > 0
    else:
        assert len(tr) == 0 and len(vh) == 0
    if len(tr):
        assert tr.min() >= 0 and tr.max() < len(vh)
        assert len(np.unique(tr)) == len(vh)                         # every vertex is used
    return vh, tr


def test_exhaustive_two_cubed_volumes_are_closed_and_outward():
    for m in range(256):
        vol = np.zeros((4, 4, 4), np.uint8)
        for c in range(8):
            if (m >> c) & 1:
                vol[1 + (c & 1), 1 + ((c >> 1) & 1), 1 + ((c >> 2) & 1)] = 1
        _check_closed_outward(vol)


@pytest.mark.parametrize("seed", range(8))
def test_random_volumes_are_closed_and_outward(seed):
    rng = np.random.default_rng(seed)
    for fill in (0.05, 0.2, 0.5, 0.7, 0.95):
        d = rng.integers(1, 13, size=3)
        vol = np.zeros(tuple(d + 2), np.uint8)
        vol[1:-1, 1:-1, 1:-1] = rng.random(tuple(d)) < fill
        _check_closed_outward(vol)


def test_one_voxel_is_the_octahedron_and_two_voxels_have_two_thirds():
    vol = np.zeros((3, 3, 3), np.uint8)
    vol[1, 1, 1] = 1
    vh, tr = _check_closed_outward(vol)
    assert len(vh) == 6 and len(tr) == 8
    assert R.six_volume(vh, tr) == 8                                 # 8 / 6 half-voxels^3 = 1/6 voxel^3
    assert sorted(map(tuple, vh)) == sorted([(0, 1, 1), (2, 1, 1), (1, 0, 1), (1, 2, 1), (1, 1, 0), (1, 1, 2)])
    for axis in range(3):
        shape = [3, 3, 3]
        shape[axis] = 4
        vol = np.zeros(shape, np.uint8)
        idx = [1, 1, 1]
        for k in (1, 2):
            idx[axis] = k
            vol[tuple(idx)] = 1
        vh, tr = _check_closed_outward(vol)
        assert len(tr) == 16 and R.six_volume(vh, tr) == 32         # 32 / 6 / 8 = 2/3 voxel^3


def test_vertex_and_triangle_order_of_the_restatement():
    rng = np.random.default_rng(3)
    vol = np.zeros((7, 6, 8), np.uint8)
    vol[1:-1, 1:-1, 1:-1] = rng.random((5, 4, 6)) < 0.4
    vh, tr = R.marching_cubes(vol)
    X, Y, Z = vol.shape
    axis = np.argmax(vh % 2 == 0, axis=1)
    assert ((vh % 2 == 0).sum(axis=1) == 1).all()                    # one even coordinate: the edge's own axis
    own = (vh + 1 - (np.arange(3)[None] == axis[:, None])) // 2
    key = ((own[:, 0] * Y + own[:, 1]) * Z + own[:, 2]) * 3 + axis
    assert (np.diff(key) > 0).all()


def test_smoothing_neighbour_multiset_is_each_neighbour_once_on_a_manifold():
    vol = np.zeros((3, 3, 3), np.uint8)
    vol[1, 1, 1] = 1
    vh, tr = R.marching_cubes(vol)
    s, deg = R.smooth_sums(vh, tr)
    assert (deg == 4).all()
    for a in range(len(vh)):
        nb = sorted(set(tr[(tr == a).any(axis=1)].reshape(-1)) - {a})
        assert len(nb) == 4 and (vh[nb].sum(axis=0) == s[a]).all()
    w = R.world_vertices(vh, tr, np.array([1.0, 2.0, 3.0]), 0.5, smooth=True)
    np.testing.assert_allclose(w, np.array([1.0, 2.0, 3.0]) + 0.25 * (vh + s) / 5.0, rtol=0, atol=1e-15)
    w0 = R.world_vertices(vh, tr, np.array([1.0, 2.0, 3.0]), 0.5, smooth=False)
    np.testing.assert_array_equal(w0, np.array([1.0, 2.0, 3.0]) + 0.25 * vh)
    rec = R.stl_records(w0, tr)
    assert rec.shape == (8, 4, 3) and rec.dtype == np.float32
    np.testing.assert_allclose(np.linalg.norm(rec[:, 0], axis=1), 1.0, atol=1e-6)
    centre = w0.mean(axis=0)
    assert (np.einsum("ij,ij->i", rec[:, 0], rec[:, 1:].mean(axis=1) - centre) > 0).all()     # normals point outward
    flat = R.stl_records(np.zeros((3, 3)), np.array([[0, 1, 2]]))
    assert (flat[0, 0] == 0).all()


def _brute_avg(p, k):
    d = np.sqrt(((p[:, None] - p[None]) ** 2).sum(-1))
    return np.sort(d, axis=1)[:, :k].mean(axis=1)


def test_outlier_restatement_small_links_duplicates_and_one_point():
    rng = np.random.default_rng(5)
    clouds = [rng.normal(size=(7, 3)), rng.normal(size=(20, 3)), rng.normal(size=(1, 3)), rng.normal(size=(60, 3))]
    dup = rng.normal(size=(40, 3))
    dup[:20] = dup[0]                                                # one point with 20 copies: its 20 nearest are itself
    dup[30] = dup[31]                                                # a plain duplicate pair
    clouds.append(dup)
    off = np.concatenate([[0], np.cumsum([len(c) for c in clouds])])
    keep, avg, thr = R.statistical_outlier(np.concatenate(clouds), off)
    for l, c in enumerate(clouds):
        np.testing.assert_allclose(avg[off[l]:off[l + 1]], _brute_avg(c, min(20, len(c))), rtol=1e-13, atol=0)
    assert avg[off[2]] == 0 and keep[off[2]] == 0 and np.isnan(thr[2])          # the one-point link
    a = avg[off[4]:off[5]]
    assert (a[:20] == 0).all() and (keep[off[4]:off[4] + 20] == 0).all() and (a[20:] > 0).all()
    pos = a[a > 0]
    assert np.isclose(thr[4], pos.mean() + 2.0 * pos.std(ddof=1), rtol=1e-14)
    for l in (0, 1, 3):
        a = avg[off[l]:off[l + 1]]
        assert np.isclose(thr[l], a.mean() + 2.0 * a.std(ddof=1), rtol=1e-14)
        np.testing.assert_array_equal(keep[off[l]:off[l + 1]], (a < thr[l]).astype(np.uint8))
    far = np.vstack([rng.normal(size=(200, 3)), [[50.0, 0, 0]]])
    k2, _, _ = R.statistical_outlier(far, [0, 201])
    assert k2[-1] == 0 and k2[:200].sum() >= 180


def test_voxelize_restatement():
    vs = 0.25
    idx = np.array([[0, 0, 0], [3, 1, 0], [1, 2, 5]])
    pts = np.array([0.3, -1.0, 2.0]) + (idx + 0.5) * vs              # voxel centres of a grid whose origin is 0.3, -1, 2
    origin, dims, vol = R.voxelize(pts, vs)
    np.testing.assert_allclose(origin, pts.min(axis=0) - vs / 2)
    assert dims.tolist() == [4, 3, 6] and vol.shape == (6, 5, 8) and vol.sum() == 3
    assert vol[1, 1, 1] == 1 and vol[4, 2, 1] == 1 and vol[2, 3, 6] == 1
    assert vol[0].sum() == vol[-1].sum() == vol[:, 0].sum() == vol[:, -1].sum() == vol[:, :, 0].sum() == vol[:, :, -1].sum() == 0
    assert R.min_quotient_gap(pts, vs) > 0.49


def test_ply_and_stl_files_round_trip(tmp_path):
    from autourdf_amd import link
    from autourdf_amd.cluster_icp import read_point_cloud
    rng = np.random.default_rng(7)
    pts = rng.normal(size=(33, 3))
    link.write_ply(str(tmp_path / "a.ply"), pts)
    np.testing.assert_array_equal(read_point_cloud(str(tmp_path / "a.ply")).points, pts)
    raw = open(tmp_path / "a.ply", "rb").read()
    assert raw.startswith(b"ply\nformat binary_little_endian 1.0\nelement vertex 33\nproperty double x\n")
    assert len(raw) == raw.index(b"end_header\n") + 11 + 33 * 24
    rec = rng.normal(size=(5, 4, 3)).astype(np.float32)
    link.write_stl(str(tmp_path / "a.stl"), rec)
    assert os.path.getsize(tmp_path / "a.stl") == 84 + 50 * 5
    np.testing.assert_array_equal(link.read_stl(str(tmp_path / "a.stl")), rec)
    link.write_stl(str(tmp_path / "e.stl"), np.zeros((0, 4, 3), np.float32))
    assert link.read_stl(str(tmp_path / "e.stl")).shape == (0, 4, 3)
    with open(tmp_path / "bad.stl", "wb") as f:
        f.write(open(tmp_path / "a.stl", "rb").read()[:-1])
    with pytest.raises(IOError):
        link.read_stl(str(tmp_path / "bad.stl"))


def test_visualize_links_writes_the_concatenated_clouds_and_refuses_a_viewer(tmp_path):
    from autourdf_amd import link
    from autourdf_amd.cluster_icp import read_point_cloud
    from autourdf_amd.helper_functions import save_pc_npz
    rng = np.random.default_rng(9)
    d = str(tmp_path / "seq0") + "/"
    os.makedirs(d + "cluster")
    os.makedirs(d + "cluster_rf")
    T, L = 4, 3
    c = [[rng.normal(size=(rng.integers(1, 9), 3)) for _ in range(L)] for _ in range(T)]
    crf = [[x + 0.5 for x in f] for f in c]
    for t in range(T):
        save_pc_npz(c[t], d + f"cluster/{t:04}.npz")
        save_pc_npz(crf[t], d + f"cluster_rf/{t:04}.npz")
    with pytest.raises(NotImplementedError):
        link.visualize_links([d], 0, T, L - 1, True)
    assert sorted(os.listdir(d)) == ["cluster", "cluster_rf"]       # refused before anything is written
    with pytest.raises(NotImplementedError):
        link.link_mesh([d], L - 1, 0.1, True)
    link.visualize_links([d], 1, T, L - 1, False)
    assert sorted(os.listdir(d)) == ["0000.ply", "0000_og.ply", "0001.ply", "0001_og.ply", "0002.ply", "0002_og.ply", "cluster",
                                     "cluster_rf"]
    for i in range(L):
        np.testing.assert_array_equal(read_point_cloud(d + f"{i:04}.ply").points, np.concatenate([crf[t][i] for t in range(1, T)]))
        np.testing.assert_array_equal(read_point_cloud(d + f"{i:04}_og.ply").points, np.concatenate([c[t][i] for t in range(1, T)]))


def test_voxel_layout_offsets_and_refusals():
    """The limits are checked on the host by the library (creg_voxel_layout) before anything is allocated or launched."""
    from autourdf_amd import ops
    off = ops.voxel_layout([[1, 1, 1], [4, 3, 6], [1022, 1, 1]], [1, 5, 9])
    assert off.tolist() == [0, 27, 27 + 6 * 5 * 8, 27 + 240 + 1024 * 9]
    with pytest.raises(ValueError, match="link 1 has no point left"):
        ops.voxel_layout([[1, 1, 1], [0, 0, 0]], [3, 0])
    with pytest.raises(ValueError, match="larger voxel_size"):
        ops.voxel_layout([[1, 1023, 1]], [3])
    with pytest.raises(ValueError, match="2\\^28.*larger voxel_size"):
        ops.voxel_layout([[1022, 1022, 300]], [3])
    assert ops.voxel_layout([[1022, 1022, 254]], [3])[-1] == 1024 * 1024 * 256        # exactly 2^28 is accepted
    import torch
    with pytest.raises(RuntimeError):
        ops.statistical_outlier(torch.zeros(4, 3, dtype=torch.float64), torch.tensor([0, 4]))
    with pytest.raises(RuntimeError):
        ops.voxel_mesh(torch.zeros(4, 3, dtype=torch.float64), torch.tensor([0, 4]), 0.1)


def test_coord_map_has_the_voxel_size_option():
    from autourdf_amd import coord_map
    assert coord_map._cli_parser().parse_args([]).voxel_size is None
    assert coord_map._cli_parser().parse_args(["--voxel_size", "0.003", "--unknown_dof"]).voxel_size == 0.003
    assert not hasattr(coord_map._parser().parse_args([]), "voxel_size")         # the reference's own flags stay as they are
