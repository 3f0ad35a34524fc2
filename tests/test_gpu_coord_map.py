"""N2: pose-sequence distance maps on the GPU vs the reference's own loops (golden) and
the oracle, through the C ABI (creg_coord_dist_map_f64, creg_pose_coords_f64) and the CoordMap mirror."""
import os

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available()
    return torch.device("cuda")


@pytest.mark.parametrize("tag", ["a", "b"])
def test_coord_dist_map_vs_reference_golden(dev, golden, tag):
    from autourdf_amd import ops
    g = golden("coord_map_reference.npz")
    M = torch.from_numpy(g[f"{tag}.matrices"]).to(dev)
    bbox = float(g[f"{tag}.bounding_box"])
    np.testing.assert_allclose(ops.pose_coords(M).cpu().numpy(), g[f"{tag}.coords"], atol=1e-12)
    for diff in (True, False):
        d_map, s_map = ops.coord_dist_map(M, bbox, diff)
        # 1e-8 on maps of magnitude ~1: static clusters have relative rotations I + O(1e-8) (float32 files vs the
        # float64 frame 0), whose rotation vectors are pure rounding noise; asin / acos near 0 turn last-bit
        # differences of the 3x3 products into ~3e-9 (measured), in the reference as much as here
        np.testing.assert_allclose(d_map.cpu().numpy(), g[f"{tag}.diff{int(diff)}.map"], atol=1e-8)
        np.testing.assert_allclose(s_map.cpu().numpy(), g[f"{tag}.diff{int(diff)}.sum"], atol=1e-7)


@pytest.mark.parametrize("T,K", [(2, 1), (5, 20), (12, 64), (7, 65), (30, 128)])
def test_coord_dist_map_vs_oracle_sizes(dev, T, K):
    """LDS path (K <= 64), workspace path (K > 64), degenerate K = 1, identity rotations at step 0."""
    from scipy.spatial.transform import Rotation
    from autourdf_amd import ops
    from oracle import coord_map as ocm
    rng = np.random.default_rng(T * 1000 + K)
    M = np.tile(np.eye(4), (T, K, 1, 1))
    M[0, :, :3, 3] = rng.uniform(-0.5, 0.5, size=(K, 3))               # R = I at step 0 (cluster_icp.py:91-95)
    for t in range(1, T):
        dR = Rotation.from_rotvec(rng.normal(scale=0.05, size=(K, 3))).as_matrix()
        M[t, :, :3, :3] = dR @ M[t - 1, :, :3, :3]
        M[t, :, :3, 3] = M[t - 1, :, :3, 3] + rng.normal(scale=0.01, size=(K, 3))
    M[:, K // 2] = M[:, 0]                                             # two identical pose tracks
    for diff in (True, False):
        want_map, want_sum = ocm.coord_dist_map(M, 0.9, diff)
        d_map, s_map = ops.coord_dist_map(torch.from_numpy(M).to(dev), 0.9, diff)
        np.testing.assert_allclose(d_map.cpu().numpy(), want_map, atol=2e-8 if not diff else 1e-9)
        np.testing.assert_allclose(s_map.cpu().numpy(), want_sum, atol=2e-7 if not diff else 1e-8)
        # properties: symmetric, zero diagonal, identical tracks are at distance 0
        d = d_map.cpu().numpy()
        np.testing.assert_allclose(d, d.transpose(1, 0, 2), atol=1e-12)
        assert np.abs(d[np.arange(K), np.arange(K)]).max() < 1e-7
        assert np.abs(d[0, K // 2]).max() < 1e-7


def test_coord_map_class_from_match_layout(dev, golden, tmp_path):
    """The CoordMap mirror on the on-disk layout match() writes (matrix/%04d.npy, cluster/%04d.npz) plus raw PLYs."""
    from autourdf_amd.coord_map import CoordMap
    from autourdf_amd.helper_functions import save_pc_npz
    from oracle import coord_map as ocm
    g = golden("coord_map_reference.npz")
    M = g["a.matrices"]
    T, K = M.shape[:2]
    part, raw = tmp_path / "part" / "0", tmp_path / "raw" / "0"
    os.makedirs(part / "matrix"); os.makedirs(part / "cluster")
    rng = np.random.default_rng(0)
    for t in range(T):
        np.save(part / "matrix" / f"{t:04}.npy", M[t] if t == 0 else M[t].astype(np.float32))
        save_pc_npz([rng.normal(size=(5 + k, 3)) for k in range(K)], str(part / "cluster" / f"{t:04}.npz"))
        os.makedirs(raw / f"{t:04}")
        pts = rng.uniform(-0.4, 0.4, size=(50, 3))
        with open(raw / f"{t:04}" / "robot.ply", "w") as f:
            f.write("ply\nformat ascii 1.0\nelement vertex 50\nproperty float x\nproperty float y\nproperty float z\nend_header\n")
            f.write("\n".join(" ".join(f"{v:.9g}" for v in p) for p in pts) + "\n")
    cm = CoordMap(str(part) + "/", str(raw) + "/", start_steps=0, end_steps=T)
    assert cm.num_coords == K and len(cm.clusters) == T and cm.matrices.dtype == np.float64
    np.testing.assert_allclose(cm.coords, g["a.coords"], atol=1e-12)
    assert abs(cm.scale - float(g["a.scale"])) < 1e-12
    assert 0.5 < cm.bounding_box < 2.0
    for diff in (True, False):
        want_map, want_sum = ocm.coord_dist_map(M, cm.bounding_box, diff)
        d_map, s_map = cm.coord_dist_map(diff=diff)
        np.testing.assert_allclose(d_map, want_map, atol=1e-8)
        np.testing.assert_allclose(s_map, want_sum, atol=1e-7)
    lm, ls = cm.coord_dist_map_legacy(diff=False)
    np.testing.assert_allclose(lm, g["a.legacy.map"], atol=1e-12)
    np.testing.assert_allclose(ls, g["a.legacy.sum"], atol=1e-12)
    cm2 = CoordMap.from_arrays(M, cm.bounding_box)
    np.testing.assert_array_equal(cm2.coord_dist_map(True)[0], cm.coord_dist_map(True)[0])


# ---- large relative rotations, every decision-matrix branch, the Taylor switches, pi, float32-rounded steps, orientation fans,
# size edges, non-finite poses and argument checks, against the long-double statement of the contract (tests/_coord_map_ref.py).
#
# diff = 1 bounds: 8 x the fp64 oracle's own largest error against long double on the same input (the device contracts the
# row sums to fma and has its own sin / cos / atan2 / asin, each a few ulp off), rounded up to a power of two; the measured
# figures are C.ORACLE_ERR_DIFF1, printed by tests/test_coord_map_cpu.py; sum_map gets T' times the entry bound.
# diff = 0 bounds: the per-entry interval C.cos_interval derives from the rounding of the cosine.
import ctypes  # noqa: E402
import functools  # noqa: E402
import sys  # noqa: E402

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import _coord_map_ref as C  # noqa: E402


def _run(dev, M, diff):
    from autourdf_amd import ops
    d_map, s_map = ops.coord_dist_map(torch.from_numpy(M).to(dev), C.BBOX, bool(diff))
    return d_map.cpu().numpy(), s_map.cpu().numpy()


def _bits_equal(a, b):
    return np.array_equal(np.ascontiguousarray(a).view(np.int64), np.ascontiguousarray(b).view(np.int64))


@functools.lru_cache(maxsize=None)
def _inputs(name):
    if name == "fan":
        return C.fan()
    if isinstance(name, tuple):
        return C.ladder_sized(*name), {}
    return C.ladder(f32_steps=name == "ladder_f32", equal_levers=name == "ladder_equal_levers")


@functools.lru_cache(maxsize=None)
def _reference(name, diff):
    """(rows, long-double map and sum on those rows) for diff = 1, (rows, per-entry bounds lo, hi (rows,K,T)) for diff = 0:
    computed once per input and shared; every row below K = 481, the fixed sample of 64 from there."""
    M = _inputs(name)[0]
    T, K = M.shape[:2]
    rows = C.sample_rows(K) if K >= 481 else np.arange(K)
    if diff:
        return (rows,) + C.coord_dist_map_ref(M, C.BBOX, True, rows)
    lo, hi = (np.stack(x, -1) for x in zip(*[C.cos_interval(M, i, rows, np.arange(K)) for i in range(T)]))
    return rows, lo, hi


def _check_diff1(dev, name, M=None):
    """Device map and sum against long double within C.diff1_bound(name); bitwise symmetry; an exactly zero diagonal."""
    M = _inputs(name)[0] if M is None else M
    Tn = M.shape[0] - 1
    rows, ref, ref_sum = _reference(name, 1)
    d, s = _run(dev, M, 1)
    bound = C.diff1_bound(name)
    err, err_sum = float(np.abs(d[rows] - ref).max()), float(np.abs(s[rows] - ref_sum).max())
    print(f"{name} diff=1: device vs long double {err:.3g} (bound {bound:.3g}), sum {err_sum:.3g} (bound {Tn * bound:.3g})")
    assert err <= bound and err_sum <= Tn * bound
    assert _bits_equal(d, d.transpose(1, 0, 2)) and _bits_equal(s, s.T)
    assert not d[np.arange(len(d)), np.arange(len(d))].any()
    return d, s


def _check_diff0(dev, name, M=None):
    """Every device entry inside the interval its cosine's rounding admits; the sum inside the summed bounds; symmetry."""
    M = _inputs(name)[0] if M is None else M
    rows, lo, hi = _reference(name, 0)
    d, s = _run(dev, M, 0)
    ref = 0.5 * (lo + hi)
    print(f"{name} diff=0: device vs interval midpoint {float(np.abs(d[rows] - ref).max()):.3g}, widest interval "
          f"{float((hi - lo).max()):.3g}, narrowest {float((hi - lo).min()):.3g}")
    assert np.all((d[rows] >= lo) & (d[rows] <= hi))
    slo, shi = C.sum_interval(lo, hi)
    assert np.all((s[rows] >= slo) & (s[rows] <= shi))
    assert _bits_equal(d, d.transpose(1, 0, 2)) and _bits_equal(s, s.T)
    return d, s, lo, hi


def test_ladder_diff1(dev):
    """Ladder (a): relative rotations 0, 1e-9, either side of 1e-3, 0.3, 2 pi / 3, 2, 2.5, pi - 1e-6, pi - 1e-9, pi, and pi
    about x, y, z, (1,1,0)/sqrt2 exactly; all four decision-matrix branches and the q.w < 0 flip are taken.
    fp64 oracle vs long double on this input: 9.32e-16, so the device bound is 2^-46 = 1.43e-14 (map values up to 3.4).
    The copied tracks are at distance exactly 0 (bitwise equal rows)."""
    M, info = _inputs("ladder")
    assert set(info["branches"].ravel().tolist()) == {0, 1, 2, 3}
    d, s = _check_diff1(dev, "ladder")
    j, k = info["copy"]
    assert np.abs(d[j, k]).max() <= C.diff1_bound("ladder") and s[j, k] <= 3 * C.diff1_bound("ladder")
    assert _bits_equal(d[j], d[k])


def test_ladder_diff1_same_link_tracks(dev):
    """Two clusters of one rigid link: with equal lever arms their translations agree too, and what is left of the entry is
    the rotational term, 0.  fp64 oracle vs long double: 9.77e-16, device bound 2^-46 = 1.43e-14."""
    M, info = _inputs("ladder_equal_levers")
    d, s = _check_diff1(dev, "ladder_equal_levers")
    j, k = info["same_link"]
    assert np.abs(d[j, k]).max() <= C.diff1_bound("ladder_equal_levers")
    d2, _ = _run(dev, _inputs("ladder")[0], 1)
    assert d2[j, k].min() > 1e-3                              # the lever arms alone put the two clusters apart


def test_ladder_f32_steps_diff1(dev):
    """Ladder (b): steps 1.. rounded to float32, the on-disk layout; the rotations are orthonormal to ~1e-8 only and the
    reference is evaluated on the same rounded input.  fp64 oracle vs long double: 1.30e-15, device bound 2^-46 = 1.43e-14."""
    _check_diff1(dev, "ladder_f32")


@pytest.mark.parametrize("name", ["ladder", "ladder_equal_levers", "ladder_f32", "fan"])
def test_ladder_and_fan_diff0(dev, name):
    """diff = 0 on the ladders (link frames up to pi apart) and on the fan (c): pair angles 0, 1e-8, 1e-4, 1, pi / 2,
    pi - 1e-4, pi - 1e-8, pi, one computed cosine above 1 and one below -1.  Copies and same-link tracks have a rotational
    term inside the interval of a cosine of 1."""
    M, info = _inputs(name)
    d, s, lo, hi = _check_diff0(dev, name)
    K = len(d)
    if name.startswith("ladder") and name != "ladder_f32":    # orthonormal rotations:
        assert np.all(lo[np.arange(K), np.arange(K)] <= 0)    # the diagonal's interval starts at 0 ...
        assert d[np.arange(K), np.arange(K)].max() < 5e-8     # ... and ends at acos(1 - delta) / pi = 2.3e-8
        j, k = info["copy"]
        assert lo[j, k].max() <= 0 and d[j, k].max() < 5e-8
    if name == "fan":
        (j, k), (j2, k2) = info["over"], info["under"]
        t = np.linalg.norm(M[0, :, :3, 3][:, None] - M[0, :, :3, 3][None], axis=-1) / (2 * C.BBOX)
        assert abs(d[j, k, 0] - t[j, k]) <= 4 * np.spacing(t[j, k])             # clamped to acos(1) = 0
        assert abs(d[j2, k2, 0] - (t[j2, k2] + 1.0)) <= 4 * np.spacing(2.0)     # clamped to acos(-1) / pi = 1
    if name == "ladder_equal_levers":
        j, k = info["same_link"]
        assert d[j, k].max() < 5e-8


SIZE_EDGES = [(2, 1), (3, 32), (3, 33), (3, 481), (3, 482), (2, 1024), (1025, 3)]


@pytest.mark.parametrize("T,K", SIZE_EDGES)
def test_size_edges(dev, T, K):
    """K = 1; 32 | 33 (256 | 1024 threads); 481 | 482 (the dynamic LDS request 17 K 8 B passes 64 KB); the largest K with its
    32 MiB workspace; T - 1 = 1024 steps of three tracks (k_sum_map's serial loop, the p T' + i index).  Tracks cycle through
    the ladder's angles.  fp64 oracle vs long double, diff = 1, and the device bound it gives:
        (2,1) 0 -> 0 (exact);  (3,32) 1.74e-15 -> 2^-46;  (3,33) 1.81e-15 -> 2^-45;  (3,481) 1.11e-14 -> 2^-43;
        (3,482) 1.08e-14 -> 2^-43;  (2,1024) 2.93e-14 -> 2^-41 = 4.55e-13;  (1025,3) 1.48e-17 -> 2^-52 (map below 0.06)
    From K = 481 the long-double reference covers a fixed sample of 64 rows (0 and K - 1 among them) and every row is
    compared with the float64 row-loop statement, which is itself within bound / 8 of long double on the sample."""
    name = (T, K)
    M = _inputs(name)[0]
    for diff in (1, 0):
        d, s = (_check_diff1(dev, name) if diff else _check_diff0(dev, name)[:2])
        d2, s2 = _run(dev, M, diff)
        assert _bits_equal(d, d2) and _bits_equal(s, s2)     # no atomics: two calls give the same bits
        if K >= 481:
            want, want_sum = C.coord_dist_map_rows(M, C.BBOX, diff)
            if diff:
                tol = C.diff1_bound(name) * 1.125            # device within bound, the float64 statement within bound / 8
            else:                                            # both lie in the entry's interval: its width, sample's widest
                rows, lo, hi = _reference(name, 0)
                tol = float((hi - lo).max())
            err = float(np.abs(d - want).max())
            print(f"{name} diff={diff}: device vs float64 rows, all rows {err:.3g} (tolerance {tol:.3g})")
            assert err <= tol and float(np.abs(s - want_sum).max()) <= (T - diff) * tol


def test_non_finite_pose(dev):
    """One NaN in one track's rotation block at one step, translation finite.  diff = 0: exactly row and column k of that
    step (and of sum_map) are NaN -- acos(clamp(NaN)) is NaN, as torch.clamp and np.clip propagate it.  diff = 1: every entry
    sums over all tracks, so the steps that use the pose (i - 1 and i) are NaN throughout and the others are untouched.
    The pattern asserted is the one the oracle produces."""
    from oracle import coord_map as ocm
    M0, _ = _inputs("ladder")
    T, K = M0.shape[:2]
    step, k = 2, 3
    M = M0.copy()
    M[step, k, 0, 1] = np.nan
    assert np.isfinite(M[:, :, :3, 3]).all()
    with np.errstate(invalid="ignore"):
        want0, want0_sum = ocm.coord_dist_map(M, C.BBOX, False)
        want1, want1_sum = ocm.coord_dist_map(M, C.BBOX, True)
    nan0 = np.zeros((K, K, T), bool)
    nan0[k, :, step] = nan0[:, k, step] = True
    assert np.array_equal(np.isnan(want0), nan0) and np.array_equal(np.isnan(want0_sum), nan0.any(-1))
    nan1 = np.zeros((K, K, T - 1), bool)
    nan1[:, :, step - 1:step + 1] = True
    assert np.array_equal(np.isnan(want1), nan1) and np.isnan(want1_sum).all()

    d, s = _run(dev, M, 0)
    assert np.array_equal(np.isnan(d), nan0), "diff = 0: NaN pattern differs from the oracle's"
    assert np.array_equal(np.isnan(s), nan0.any(-1))
    rows, lo, hi = _reference("ladder", 0)                    # everything else: the bounds of the finite input
    assert np.all(((d >= lo) & (d <= hi))[~nan0])
    clean, clean_sum = _run(dev, M0, 0)
    assert _bits_equal(d[~nan0], clean[~nan0]) and _bits_equal(s[~nan0.any(-1)], clean_sum[~nan0.any(-1)])

    d, s = _run(dev, M, 1)
    assert np.array_equal(np.isnan(d), nan1) and np.isnan(s).all()
    rows, ref, _ = _reference("ladder", 1)
    assert float(np.abs(d - ref)[~nan1].max()) <= C.diff1_bound("ladder")
    assert _bits_equal(d[:, :, 0], _run(dev, M0, 1)[0][:, :, 0])


def test_argument_checks_do_not_launch(dev):
    """K = 1025, T = 1 with diff, bounding_box 0 and negative, a workspace one byte short: an error code (a RuntimeError
    through ops) and untouched outputs."""
    from autourdf_amd import _lib, ops
    L = _lib.load()
    vp = ctypes.c_void_p
    stream = vp(torch.cuda.current_stream().cuda_stream)

    def call(T, K, bbox, diff, short=0):
        M = np.tile(np.eye(4), (T, K, 1, 1))
        M[:, :, :3, 3] = np.arange(T * K * 3).reshape(T, K, 3) ** 2 % 7 / 10.0         # (pair matrices that are not all 0)
        M = torch.from_numpy(M).to(dev)
        Tn = max(T - diff, 1)
        d_map = torch.full((K, K, Tn), -7.0, dtype=torch.float64, device=dev)
        s_map = torch.full((K, K), -7.0, dtype=torch.float64, device=dev)
        need = L.creg_coord_dist_map_workspace_bytes(T, K)
        ws = torch.zeros(max(need, 256), dtype=torch.uint8, device=dev)
        rc = L.creg_coord_dist_map_f64(vp(M.data_ptr()), T, K, float(bbox), diff, vp(d_map.data_ptr()), vp(s_map.data_ptr()),
                                       vp(ws.data_ptr()), need - short, stream)
        torch.cuda.synchronize()
        return rc, bool((d_map == -7.0).all() and (s_map == -7.0).all()), bool((ws == 0).all())

    assert call(2, 65, 0.9, 1) == (0, False, False)                    # the harness itself: a good call launches
    for args in [(2, 1025, 0.9, 1), (2, 1025, 0.9, 0), (1, 4, 0.9, 1), (2, 4, 0.0, 1), (2, 4, -0.9, 0), (2, 65, 0.9, 1, 1),
                 (2, 4, 0.9, 1, 1)]:
        rc, outputs_untouched, ws_untouched = call(*args)
        assert rc != 0 and outputs_untouched and ws_untouched, args
        assert L.creg_last_error()
    eye = lambda T, K: torch.from_numpy(np.tile(np.eye(4), (T, K, 1, 1))).to(dev)      # noqa: E731
    for M, bbox, diff in [(eye(2, 1025), 0.9, True), (eye(1, 4), 0.9, True), (eye(2, 4), 0.0, True), (eye(2, 4), -1.0, False)]:
        with pytest.raises(RuntimeError):
            ops.coord_dist_map(M, bbox, diff)
    d_map, _ = ops.coord_dist_map(eye(1, 4), 0.9, False)                # T = 1 without diff is a valid call
    assert d_map.shape == (4, 4, 1) and not d_map.cpu().numpy().any()
