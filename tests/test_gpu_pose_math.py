"""The pose-conversion templates of creg_dev.h at rotation edge cases, on the GPU.

(a) the nine row kernels of se3.hip: bit-identical to the float32 restatements of tests/_pose_edges.py at tail sizes,
    nothing written past k, and the fp64 properties against oracle.transforms / oracle.dq;
(b) k_pose_coords (the float64 instantiation): bit-identical to the float64 restatement, 1e-15 of the oracle;
(c) coord_dist_map on pose tracks built to hit rotvec_roundtrip's and acos's switch points;
(d) the train plan's pose encoding / decoding at edge poses, end to end against oracle autograd.

Bounds below use u = 2^-24 (float32 unit roundoff) and e64 = 2^-53.
"""
import numpy as np
import pytest
import torch

import _pose_edges as E

pytestmark = pytest.mark.gpu

SIZES = (1, 63, 64, 65, 1000, 4099)
U = 2.0 ** -24
E64 = 2.0 ** -53
GUARD = 64                                    # sentinel rows after the k rows a launch may write
SENTINEL = np.array([0x7FC0DEAD], np.uint32).view(np.float32)[0]


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "GPU tests need the MI355X"
    from autourdf_amd import _lib
    _lib.load()
    return torch.device("cuda:0")


def _cuda(a, dev):
    return torch.from_numpy(np.ascontiguousarray(a)).to(dev)


def _assert_bits(got, want, labels, what):
    """Raw-bit equality (signed zeros count), reporting the family labels of the first differing rows."""
    got, want = np.ascontiguousarray(got), np.ascontiguousarray(want)
    assert got.shape == want.shape, (what, got.shape, want.shape)
    iv = np.int32 if got.dtype == np.float32 else np.int64
    g, w = got.reshape(len(got), -1).view(iv), want.reshape(len(want), -1).view(iv)
    both_nan = np.isnan(got.reshape(len(got), -1)) & np.isnan(want.reshape(len(want), -1))   # NaN payloads are not IEEE's
    bad = np.nonzero(((g != w) & ~both_nan).any(1))[0]
    if len(bad):
        r = bad[:4]
        raise AssertionError(f"{what}: {len(bad)} of {len(got)} rows differ from the restatement in their bits; first rows "
                             f"{r.tolist()} labels {[str(labels[i]) for i in r]}\n got  {got.reshape(len(got), -1)[r]}\n want "
                             f"{want.reshape(len(want), -1)[r]}")


# ------------------------------------------------------------------------------------------ inputs
_POOLS = {}


def _pools():
    """Edge rows first, the 4096 random rotations last; float32 inputs with their family labels."""
    if not _POOLS:
        lr, _, R32 = E.stack(E.rotation_families())
        rng = np.random.default_rng(11)
        t32 = rng.uniform(-1, 1, size=(len(R32), 3)).astype(np.float32)
        lq, _, q32 = E.stack(E.quaternion_families())
        ld, _, d32 = E.stack(E.dualquat_families())
        _POOLS.update(R=(lr, R32), M=(lr, E.poses(R32, t32)), q=(lq, q32), t=(lq, rng.uniform(-1, 1, (len(q32), 3)).astype(np.float32)),
                      d=(ld, d32), d2=(ld, d32[rng.permutation(len(d32))]), gM=(ld, rng.normal(size=(len(d32), 4, 4)).astype(np.float32)))
        _POOLS["n_edge_R"] = int(np.sum(lr != "random"))
    return _POOLS


# name -> (C symbol, inputs (pool keys), output row shapes, restatement)
OPS = {
    "se3_to_dq": ("creg_se3_to_dq_f32", ("M",), ((8,),), lambda M: (E.se3_to_dq(M, np.float32),)),
    "dq_to_se3": ("creg_dq_to_se3_f32", ("d",), ((4, 4),), lambda d: (E.dq_to_se3(d, np.float32),)),
    "dq_to_se3_bwd": ("creg_dq_to_se3_bwd_f32", ("d", "gM"), ((8,),), None),
    "dq_multiply": ("creg_dq_multiply_f32", ("d", "d2"), ((8,),), lambda a, b: (E.dq_multiply(a, b, np.float32),)),
    "dq_invert": ("creg_dq_invert_f32", ("d",), ((8,),), lambda d: (E.dq_invert(d, np.float32),)),
    "dq_to_quat_trans": ("creg_dq_to_quat_trans_f32", ("d",), ((4,), (3,)), lambda d: E.dq_to_quat_trans(d, np.float32)),
    "quat_trans_to_dq": ("creg_quat_trans_to_dq_f32", ("q", "t"), ((8,),), lambda q, t: (E.quat_trans_to_dq(q, t, np.float32),)),
    "matrix_to_quat": ("creg_matrix_to_quat_f32", ("R",), ((4,),), lambda R: (E.matrix_to_quat(R, np.float32),)),
    "quat_to_matrix": ("creg_quat_to_matrix_f32", ("q",), ((3, 3),), lambda q: (E.quat_to_matrix(q, np.float32),)),
}


def _inputs(op, n, layout):
    """n rows of each input.  layout 0 starts at the first edge row; layout 1 ends the batch on the last edge rows, so the
    tail block of the launch holds edge rows as well."""
    P = _pools()
    keys = OPS[op][1]
    labels, first = P[keys[0]]
    n_edge = P["n_edge_R"] if keys[0] in ("R", "M") else len(first)
    shift = 0 if layout == 0 else (n_edge - n) % len(first)
    return E.resize_rows(labels, n, shift), [E.resize_rows(P[k][1], n, shift) for k in keys]


def _launch(dev, op, ins, k, rows=None):
    """Call the C entry point with outputs pre-filled with a NaN sentinel and GUARD extra rows; returns the full buffers."""
    from autourdf_amd import _lib, ops
    L = _lib.load()
    sym, _, shapes, _ = OPS[op]
    rows = k if rows is None else rows
    outs = [torch.full((rows + GUARD,) + s, float("nan"), dtype=torch.float32, device=dev) for s in shapes]
    for o in outs:
        o.view(torch.int32).fill_(int(SENTINEL.view(np.int32)))
    a = [_cuda(x, dev) for x in ins]
    p = [ops._p(x) for x in a] + [None] * (2 - len(a))
    fn = getattr(L, sym)
    if len(shapes) == 2:
        rc = fn(p[0], k, ops._p(outs[0]), ops._p(outs[1]), ops._stream())
    elif len(a) == 2:
        rc = fn(p[0], p[1], k, ops._p(outs[0]), ops._stream())
    else:
        rc = fn(p[0], k, ops._p(outs[0]), ops._stream())
    _lib.check(rc, sym)
    return [o.cpu().numpy() for o in outs]


def _untouched(buf, start):
    tail = np.ascontiguousarray(buf[start:]).reshape(-1).view(np.int32)
    return bool((tail == SENTINEL.view(np.int32)).all())


# ------------------------------------------------------------------------------------------ (a) bit-exact rows
@pytest.mark.parametrize("n", SIZES)
@pytest.mark.parametrize("op", [o for o in OPS if OPS[o][3] is not None])
def test_rows_bit_exact_vs_float32_restatement(dev, op, n):
    """Same float32 operation order (-ffp-contract=off, IEEE division and sqrt): every output bit, signed zeros included,
    for every family at sizes around the 64-row block, and nothing written past row k."""
    for layout in (0, 1):
        labels, ins = _inputs(op, n, layout)
        outs = _launch(dev, op, ins, n)
        want = OPS[op][3](*ins)
        for i, (o, w) in enumerate(zip(outs, want)):
            assert _untouched(o, n), f"{op}: wrote past row k = {n}"
            _assert_bits(o[:n], w.reshape(o[:n].shape), labels, f"{op} (n={n}, layout {layout}, output {i})")


@pytest.mark.parametrize("op", list(OPS))
def test_rows_k0_is_a_noop(dev, op):
    labels, ins = _inputs(op, 8, 0)
    outs = _launch(dev, op, ins, 0, rows=8)
    assert all(_untouched(o, 0) for o in outs), f"{op}: k = 0 wrote its output"


def test_rows_wrappers_accept_empty_batches(dev):
    from autourdf_amd import ops
    z = lambda *s: torch.zeros(s, dtype=torch.float32, device=dev)
    assert ops.se3_to_dq(z(0, 4, 4)).shape == (0, 8)
    assert ops.dq_to_se3(z(0, 8)).shape == (0, 4, 4)
    assert ops.matrix_to_quat(z(0, 3, 3)).shape == (0, 4)
    q, t = ops.dq_to_quat_trans(z(0, 8))
    assert q.shape == (0, 4) and t.shape == (0, 3)


def _sign_dist(a, b):
    """Per-row min(|a - b|, |a + b|) (max norm): the distance between the rotations a and b stand for."""
    return np.minimum(np.abs(a - b).max(1), np.abs(a + b).max(1))


def test_matrix_to_quat_fp64_properties(dev):
    """Against oracle.transforms in fp64 on the float32 inputs widened (exact): each component is a ratio of a float32 sum of
    at most 4 terms of magnitude <= 4 (rounding <= 4 * 4u absolute) over a denominator 2 qa >= 2 (qa[c] >= 1: the four sqrt
    arguments sum to 4) with <= 3u relative error, so |dq| <= 16u / 2 + 3u = 11u up to the sign; and w >= 0 always."""
    from oracle import transforms as OT
    lab, R32 = _pools()["R"]
    q = _launch(dev, "matrix_to_quat", [R32], len(R32))[0][:len(R32)]
    q64 = OT.matrix_to_quaternion(torch.from_numpy(R32.astype(np.float64))).numpy()
    d = _sign_dist(q.astype(np.float64), q64)
    worst = int(np.argmax(d))
    assert d[worst] <= 11 * U, (str(lab[worst]), d[worst])
    assert (q[:, 0] >= 0).all()
    _, _, c, den, _ = E.matrix_to_quat_parts(R32, np.float32)
    assert (den >= np.float32(2) * (1 - 4 * U)).all()            # the 0.1 floor never binds for the chosen candidate


def test_quat_to_matrix_fp64_properties(dev):
    """Unit quaternions give orthonormal matrices to 1e-6 (entries <= 1, ~6 roundings each: 6u ~ 4e-7); every family,
    non-unit ones included (R is invariant to |q|), is within 8u of the fp64 oracle entrywise."""
    from oracle import transforms as OT
    lab, q32 = _pools()["q"]
    R = _launch(dev, "quat_to_matrix", [q32], len(q32))[0][:len(q32)].astype(np.float64)
    R64 = OT.quaternion_to_matrix(torch.from_numpy(q32.astype(np.float64))).numpy()
    err = np.abs(R - R64).reshape(len(R), -1).max(1)
    assert err.max() <= 8 * U, (str(lab[np.argmax(err)]), err.max())
    unit = np.abs(np.linalg.norm(q32.astype(np.float64), axis=1) - 1) < 1e-6
    assert unit.sum() > 300
    orth = np.abs(R[unit] @ np.swapaxes(R[unit], 1, 2) - np.eye(3)).reshape(unit.sum(), -1).max(1)
    assert orth.max() <= 1e-6, (str(lab[unit][np.argmax(orth)]), orth.max())


def test_se3_dq_roundtrip_and_fp64(dev):
    """se3_to_dq within 22u of the fp64 oracle up to the joint sign of real and dual (real: 11u as matrix_to_quat plus the
    renormalisation; dual = 0.5 (0,t) (x) real with |t| <= sqrt(3): 11u * sqrt(3) + 4u); M -> dq -> M reproduces M within 1e-6
    (rotation entries: 11u of q times the <= 4 |dR/dq| of a unit quaternion; t: 2 |dual| |real| with a few u each) on the
    orthonormal families, and within 4e-6 on R (1 +- 1e-6), which comes back orthonormal."""
    from oracle import dq as OD
    lab, M32 = _pools()["M"]
    n = len(M32)
    d = _launch(dev, "se3_to_dq", [M32], n)[0][:n]
    d64 = OD.transform_to_dualquat(torch.from_numpy(M32.astype(np.float64))).numpy()
    dist = _sign_dist(d.astype(np.float64), d64)
    assert dist.max() <= 22 * U, (str(lab[np.argmax(dist)]), dist.max())
    assert (d[:, 0] >= 0).all()
    back = _launch(dev, "dq_to_se3", [d], n)[0][:n].astype(np.float64)
    err = np.abs(back - M32.astype(np.float64)).reshape(n, -1).max(1)
    scaled = np.char.startswith(lab.astype(str), "scaled")
    assert err[~scaled].max() <= 1e-6, (str(lab[~scaled][np.argmax(err[~scaled])]), err[~scaled].max())
    assert err[scaled].max() <= 4e-6


def test_dual_quaternion_rows_fp64(dev):
    """dq_to_se3, dq_multiply, dq_to_quat_trans, quat_trans_to_dq and dq_invert (outside its clamp) against oracle.dq in fp64.
    Each output is a sum of at most 8 products (or a conjugate scaled by 1/|real|^2); rounding is bounded relative to the
    size of the products it sums: 16u * (sum of |factor| products) per row."""
    from oracle import dq as OD
    P = _pools()
    lab, d32 = P["d"]
    d2 = P["d2"][1]
    n = len(d32)
    w64 = lambda a: torch.from_numpy(a.astype(np.float64))
    nr, nd = np.linalg.norm(d32[:, :4].astype(np.float64), axis=1), np.linalg.norm(d32[:, 4:].astype(np.float64), axis=1)
    nr2, nd2 = np.linalg.norm(d2[:, :4].astype(np.float64), axis=1), np.linalg.norm(d2[:, 4:].astype(np.float64), axis=1)

    def check(got, want, scale, what):
        got = got.reshape(n, -1).astype(np.float64)
        want = want.reshape(n, -1)
        r = np.abs(got - want).max(1) / (16 * U * scale)
        assert r.max() <= 1, (what, str(lab[np.argmax(r)]), r.max())

    M = _launch(dev, "dq_to_se3", [d32], n)[0][:n]
    ok = nr > 1e-3                                                   # R = q2m(real) is scale-invariant, defined for real != 0
    M64 = OD.dualquat_to_transform(w64(d32)).numpy()
    got, want = M.reshape(n, 16), M64.reshape(n, 16)
    np.testing.assert_allclose(got[ok][:, [0, 1, 2, 4, 5, 6, 8, 9, 10]], want[ok][:, [0, 1, 2, 4, 5, 6, 8, 9, 10]], rtol=0, atol=8 * U)
    check(got[:, [3, 7, 11]], want[:, [3, 7, 11]], 2 * nr * nd * 2 + 1e-30, "dq_to_se3 t")
    check(_launch(dev, "dq_multiply", [d32, d2], n)[0][:n], OD.dualquat_multiply(w64(d32), w64(d2)).numpy(),
          2 * (nr * nr2 + nr * nd2 + nd * nr2) + 1e-30, "dq_multiply")
    q, t = _launch(dev, "dq_to_quat_trans", [d32], n)
    q64, t64 = OD.dualquat_to_quat_trans(w64(d32))
    check(q[:n], q64.numpy(), 2 * nr * nd + 1e-30, "dq_to_quat_trans q")
    check(t[:n], t64.numpy(), 4 * nr * nd + 1e-30, "dq_to_quat_trans t")
    lq, q32 = P["q"]
    t32 = P["t"][1]
    m = len(q32)
    got = _launch(dev, "quat_trans_to_dq", [q32, t32], m)[0][:m]
    want = OD.quat_trans_to_dualquat(w64(q32), w64(t32)).numpy()
    assert np.array_equal(got[:, :4], q32)
    sc = 2 * np.linalg.norm(q32.astype(np.float64), axis=1) * np.linalg.norm(t32.astype(np.float64), axis=1) + 1e-30
    assert (np.abs(got[:, 4:] - want[:, 4:]).max(1) <= 16 * U * sc).all()
    # dq_invert: the oracle clamps |real|^2 at float64's eps, the kernel at FLT_EPSILON -- compare where neither clamp binds
    inv = _launch(dev, "dq_invert", [d32], n)[0][:n]
    assert np.isfinite(inv).all()
    free = nr * nr > 2 * E.FLT_EPSILON
    inv64 = OD.dualquat_invert(w64(d32)).numpy()
    sc = (nr[free] + 3 * nd[free]) / (nr[free] * nr[free])
    r = np.abs(inv[free].astype(np.float64) - inv64[free]).max(1) / (32 * U * sc)
    assert r.max() <= 1, (str(lab[free][np.argmax(r)]), r.max())


@pytest.mark.parametrize("n", (63, 65, 1000))
def test_dq_to_se3_bwd_vs_fp64_autograd_nonunit_and_small_real(dev, n):
    """The VJP on non-unit real parts (norms 1e-4 .. 1e3) and real parts around sqrt(FLT_EPSILON), against fp64 autograd of
    oracle.dq.dualquat_to_transform.  The gradient's terms scale like |gM| (2/|r| + 2 |d|) (R depends on r / |r|; t on r and
    d bilinearly), and the kernel sums ~20 of them in float32, so the bound is 64u times that scale per row."""
    from oracle import dq as OD
    P = _pools()
    lab, d32 = P["d"]
    gM = P["gM"][1]
    pick = np.nonzero(np.char.startswith(lab.astype(str), "non_unit") | (np.char.startswith(lab.astype(str), "small_real")
                                                                      & (np.linalg.norm(d32[:, :4], axis=1) > 0)))[0]
    idx = E.resize_rows(pick, n)
    d, g = d32[idx], gM[idx]
    got = _launch(dev, "dq_to_se3_bwd", [d, g], n)[0]
    assert _untouched(got, n)
    got = got[:n].astype(np.float64)
    dd = torch.from_numpy(d.astype(np.float64)).requires_grad_(True)
    (OD.dualquat_to_transform(dd) * torch.from_numpy(g.astype(np.float64))).sum().backward()
    want = dd.grad.numpy()
    nr, nd = np.linalg.norm(d[:, :4].astype(np.float64), axis=1), np.linalg.norm(d[:, 4:].astype(np.float64), axis=1)
    scale = np.abs(g).reshape(n, -1).max(1) * (2 / nr + 2 * nd + 2 * nr)
    r = np.abs(got - want).max(1) / (64 * U * scale)
    assert r.max() <= 1, (str(lab[idx][np.argmax(r)]), r.max())


# ------------------------------------------------------------------------------------------ (b) k_pose_coords, fp64
@pytest.mark.parametrize("n", (1, 255, 257, 4099, None))
def test_pose_coords_bit_exact_vs_float64_restatement(dev, n):
    from autourdf_amd import ops
    from oracle import coord_map as OC
    lab, R64, _ = E.stack(E.rotation_families())
    t = np.random.default_rng(5).uniform(-1, 1, size=(len(R64), 3))
    M = E.poses(R64, t)
    if n is not None:
        M, lab = E.resize_rows(M, n, (np.sum(lab != "random") - n) % len(M)), E.resize_rows(lab, n, (np.sum(lab != "random") - n) % len(M))
    got = ops.pose_coords(_cuda(M, dev)).cpu().numpy()
    want = np.concatenate([M[:, :3, 3], E.matrix_to_quat(M[:, :3, :3], np.float64)], 1)
    _assert_bits(got, want, lab, f"pose_coords (n={len(M)})")
    np.testing.assert_allclose(got, OC.coords_from_matrices(M), rtol=0, atol=1e-15)


# ------------------------------------------------------------------------------------------ (c) coord_dist_map switch points
@pytest.mark.parametrize("K", (1, 64, 65))
def test_coord_dist_map_at_rotvec_and_acos_switch_points(dev, K):
    """Tracks whose steps sit at rotvec_roundtrip's decisions (no step, 1e-6, 1e-3 +- 1e-9 on both series branches, pi - 1e-6,
    exactly pi, past pi: the shortest-arc flip) and track pairs at relative rotation I and pi (acos at +1 and at the clamp -1).

    Tolerances from each point's conditioning:
      diff = 0: the kernel and the oracle sum tr(R_j^T R_k) in different orders; 9 products and 8 sums with partial sums
        <= 3 leave each trace within ~30 e64, so the two values of (tr - 1) / 2 differ by <= ~32 e64; ec = 64 e64 covers that
        twice.  acos is then off by at most the width of acos over [cos - ec, cos + ec] (clipped to [-1, 1]) -- near +-1 that
        is sqrt(2 ec) ~ 1.2e-7 (acos turns eps into sqrt(2 eps)), elsewhere ~ec / sin.  Plus
        lam_bbox * 8 e64 * |dt| for the translation part.
      diff = 1: every quaternion component of the rotation vectors' round trip carries ~64 e64 (rotmat_to_unitquat, atan2, sin, cos
        of ~1 ulp each, no cancellation: the decision matrix picks the best-conditioned branch, the flip keeps w >= 0); the
        geodesic 4 asin(0.5 min(...)) has asin's argument <= sqrt(2)/2 (slope <= sqrt(2)), so d_rpy is off by <= 4 sqrt(2) * 2 *
        64 e64 / pi ~ 1.6e-14; d_xyz by lam_bbox * 8 e64 * |dt|.  The map is a distance between K-vectors of these:
        |map - map'| <= 2 sqrt(K) * max entry error."""
    from autourdf_amd import ops
    from oracle import coord_map as OC
    T, bbox = 4, 0.9
    M, steps = E.coord_tracks(T, K, seed=K)
    lam_rot, lam_bbox = 1 / np.pi, 1 / (2 * bbox)
    for diff in (True, False):
        want, want_sum = OC.coord_dist_map(M, bbox, diff)
        got, got_sum = (x.cpu().numpy() for x in ops.coord_dist_map(_cuda(M, dev), bbox, diff))
        assert np.isfinite(got).all() and np.isfinite(got_sum).all()
        if diff:
            dt = np.abs(np.diff(M[:, :, :3, 3], axis=0)).max()
            entry = lam_rot * 4 * np.sqrt(2) * 2 * 64 * E64 + lam_bbox * 8 * E64 * 2 * dt
            tol = np.full(want.shape, 2 * np.sqrt(K) * entry)
        else:
            R = M[:, :, :3, :3]
            rel = np.einsum("tjab,tkac->tjkbc", R, R)                 # R_j^T R_k per step
            cs = (0.5 * (np.trace(rel, axis1=-2, axis2=-1) - 1.0)).transpose(1, 2, 0)
            ec = 64 * E64
            width = np.arccos(np.clip(cs - ec, -1, 1)) - np.arccos(np.clip(cs + ec, -1, 1))
            tol = lam_rot * width + lam_bbox * 8 * E64 * 2
        bad = np.abs(got - want) > tol
        assert not bad.any(), (diff, np.argwhere(bad)[:4].tolist(), np.abs(got - want).max(), [steps[j] for j in np.argwhere(bad)[:4, 0]])
        assert (np.abs(got_sum - want_sum) <= tol.sum(-1) + 1e-300).all(), (diff, np.abs(got_sum - want_sum).max())


# ------------------------------------------------------------------------------------------ (d) train plan at edge poses
def _edge_cluster_poses(K, rot, seed):
    """K poses from the edge families (pi exactly / signed-zero / trig / +-delta, pi/2 ties, near pi, small angles) with
    translations in [-0.5, 0.5]; for rpy the pitch rows at +-(pi/2 - delta) lead."""
    fams = {f[0]: f[2] for f in E.rotation_families()}
    order = ["pi_exact", "pi_signed_zero", "pi_trig", "pi_plus_1e-07", "pi_minus_1e-07", "pi_plus_1e-05", "half_pi_exact",
             "half_pi_trig", "half_pi_pm_1e-07", "near_pi_random", "small_angle", "f32_products"]
    R = np.concatenate([fams[k] for k in order])
    if rot == "rpy":
        e = np.concatenate([f[1] for f in E.rpy_families() if f[0] != "gimbal_lock"])
        R = np.concatenate([E.euler_xyz_to_rot64(e).astype(np.float32), R])
    R = R[:K]
    rng = np.random.default_rng(seed)
    return E.poses(R, rng.uniform(-0.5, 0.5, size=(K, 3)).astype(np.float32))


def _oracle_model(rot, hidden):
    from oracle import models
    return {"q": lambda: models.QRegMLP(True, hidden), "dq": lambda: models.DQRegMLP(hidden), "6d": lambda: models.RRegMLP(hidden),
            "rpy": lambda: models.RegMLP(True, hidden)}[rot]()


def _order(rot):
    from autourdf_amd import ops
    return ops.DQ_PARAM_ORDER if rot == "dq" else ops.Q_PARAM_ORDER


def _correctly_rounded_sqrt_pos(v):
    # the kernel's sqrt is IEEE-rounded; torch's CPU float32 sqrt is not (about 1 argument in 5 comes back 1 ulp off), and at the
    # near-ties these families build 1 ulp moves matrix_to_quaternion's argmax.  Rounding the fp64 root once is exact for sqrt.
    out = torch.zeros_like(v)
    pos = v > 0
    out[pos] = torch.sqrt(v[pos].double()).to(v.dtype)
    return out


def _probe_problem(rot, K, seed=0):
    rng = np.random.default_rng(seed)
    m = torch.from_numpy(_edge_cluster_poses(K, rot, seed))
    sizes = 6 + np.arange(K) % 5
    clusters = [torch.from_numpy(rng.normal(scale=0.08, size=(s, 3)).astype(np.float32)) for s in sizes]
    y = torch.cat([c @ mm[:3, :3].T + mm[:3, 3] for c, mm in zip(clusters, m)])
    y = y + torch.from_numpy(rng.normal(scale=0.02, size=tuple(y.shape)).astype(np.float32))
    return m, y, clusters


@pytest.mark.parametrize("K", (65, 130))
@pytest.mark.parametrize("rot", ["q", "dq", "6d", "rpy"])
def test_train_probe_at_edge_poses_vs_oracle(dev, rot, K, monkeypatch):
    """test_gpu_parity.py::test_train_probe_forward_and_pose_gradient_vs_oracle on cluster poses drawn from the edge
    families, over more than one 64-row group, at that test's tolerances.  A sign or candidate decision the plan takes
    differently from the oracle's float32 arithmetic moves the MLP input by O(1) (q and -q are different inputs)."""
    from autourdf_amd import ops
    from oracle import registration
    from oracle import transforms as OT
    from oracle.chamfer import chamfer_distance
    monkeypatch.setattr(OT, "_sqrt_pos", _correctly_rounded_sqrt_pos)
    m, y, clusters = _probe_problem(rot, K, seed=K)
    torch.manual_seed(3)
    model = _oracle_model(rot, 64)
    for p in model.parameters():
        p.data.mul_(0.2)
    m2 = registration.pose_forward(m, model, rot)
    m2.retain_grad()
    pred = torch.cat(registration.calculate_pc(clusters, m2))
    loss, _ = chamfer_distance(pred[None], y[None], norm=1)
    loss.backward()
    plan = ops.TrainPlan(rot, K, 64, pred.shape[0], y.shape[0], epochs=4, use_graph=False, device=dev)
    params = [model.state_dict()[k].clone().to(dev) for k in _order(rot)]
    pts, off = ops.pack_clusters(clusters, dev)
    gm2, gpred, gloss, ggrad = plan.probe(m.to(dev), y.to(dev), pts, off, params)
    np.testing.assert_allclose(gm2.cpu().numpy(), m2.detach().numpy(), atol=2e-6)
    np.testing.assert_allclose(gpred.cpu().numpy(), pred.detach().numpy(), atol=2e-6)
    assert abs(gloss.item() - loss.item()) <= 2e-6 * abs(loss.item())
    np.testing.assert_allclose(ggrad.cpu().numpy()[:, :3, :], m2.grad.numpy()[:, :3, :], rtol=1e-4, atol=2e-6)


def test_train_probe_rpy_at_gimbal_lock_is_finite(dev):
    """At pitch exactly +-pi/2 the roll / yaw split is undefined: only finiteness is asserted."""
    from autourdf_amd import ops
    K = 65
    e = np.resize(dict(E.rpy_families())["gimbal_lock"], (K, 3))
    m = torch.from_numpy(E.poses(E.euler_xyz_to_rot64(e).astype(np.float32), np.zeros((K, 3), np.float32)))
    rng = np.random.default_rng(1)
    clusters = [torch.from_numpy(rng.normal(scale=0.08, size=(6, 3)).astype(np.float32)) for _ in range(K)]
    y = torch.from_numpy(rng.normal(scale=0.3, size=(200, 3)).astype(np.float32))
    torch.manual_seed(3)
    model = _oracle_model("rpy", 64)
    plan = ops.TrainPlan("rpy", K, 64, 6 * K, 200, epochs=4, use_graph=False, device=dev)
    params = [model.state_dict()[k].clone().to(dev) for k in _order("rpy")]
    pts, off = ops.pack_clusters(clusters, dev)
    outs = plan.probe(m.to(dev), y.to(dev), pts, off, params)
    for o in outs:
        assert torch.isfinite(o).all()
