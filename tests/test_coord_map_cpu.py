"""CPU: the long-double statement of the pose distance maps (tests/_coord_map_ref.py) is itself checked -- against a
50-digit mpmath evaluation of the contract written out with scalar loops, and against scipy's rotation magnitudes -- its
builders reach the cases they are built for, and the fp64 oracle (oracle/coord_map.py) is measured against it: the
printed diff = 1 errors are the numbers the device bounds of tests/test_gpu_coord_map.py are derived from."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import _coord_map_ref as C  # noqa: E402

LD = np.longdouble
SIZES = [(2, 1), (3, 32), (3, 33), (3, 481), (3, 482), (2, 1024), (1025, 3)]


def _inputs(name):
    if name == "fan":
        return C.fan()[0]
    if isinstance(name, tuple):
        return C.ladder_sized(*name)
    return C.ladder(f32_steps=name == "ladder_f32", equal_levers=name == "ladder_equal_levers")[0]


# ------------------------------------------------------------------------------------------ builders
def test_ladder_reaches_every_branch_and_edge():
    for f32 in (False, True):
        M, info = C.ladder(f32_steps=f32)
        assert M.shape == (4, 17, 4, 4) and M.dtype == np.float64
        assert set(info["branches"].ravel().tolist()) == {0, 1, 2, 3}
        j, k = info["copy"]
        assert np.array_equal(M[:, j], M[:, k])
        j, k = info["same_link"]
        assert np.array_equal(M[:, j, :3, :3], M[:, k, :3, :3]) and not np.array_equal(M[:, j, :3, 3], M[:, k, :3, 3])
        rel = C.relative_rotations(M)
        for e, E in enumerate(C.EXACT_PI):                    # exact: argmax ties among the -1 (and the 0, 0 of the last)
            assert np.array_equal(rel[:, 11 + e].astype(np.float64), np.broadcast_to(E, (3, 3, 3)))
        assert info["branches"][0, 11:15].tolist() == [0, 1, 2, 0]
        q = C.rotmat_to_unitquat(rel)[0]
        angle = 2 * np.arctan2(np.sqrt((q[..., :3] ** 2).sum(-1)), np.abs(q[..., 3]))
        want = np.array([float(a) for a in C.ANGLES])
        # float32 rounding moves a relative rotation by ~1e-7 (and one within 3e-4 of pi by its square root)
        tol = np.where(want > 3.14, 1e-3, 1e-6) if f32 else np.where(want > 3.14, 1e-7, 1e-12)
        assert np.all(np.abs(angle[:, :11].astype(np.float64) - want) <= tol)
        assert (q[..., 3] < 0).any()                          # the flip to the shortest arc is taken
        orth = np.abs(np.swapaxes(M[1:, :, :3, :3], -1, -2) @ M[1:, :, :3, :3] - np.eye(3)).max()
        assert (1e-9 < orth < 1e-6) if f32 else orth < 1e-15
    Me, info = C.ladder(equal_levers=True)
    assert np.array_equal(Me[:, 7], Me[:, 16]) and np.array_equal(Me[:, :16], C.ladder()[0][:, :16])


def test_fan_reaches_every_angle_and_both_clamps():
    M, info = C.fan()
    assert M.shape == (1, 11, 4, 4)
    c = 0.5 * (np.einsum("ab,kab->k", M[0, 0, :3, :3].astype(LD), M[0, :8, :3, :3].astype(LD)) - 1)
    want = np.array([np.cos(a) for a in C.FAN_ANGLES])
    assert np.all(np.abs(c - want) <= 1e-15)
    assert info["cos_over"] > 1 + 1e-9 and info["cos_under"] < -1 - 1e-9
    for (j, k), key in ((info["over"], "cos_over"), (info["under"], "cos_under")):
        got = 0.5 * ((M[0, j, :3, :3] * M[0, k, :3, :3]).sum() - 1)               # the fp64 cosine is past the clamp too
        assert abs(got - float(info[key])) < 1e-14 and abs(got) > 1


def test_sized_ladder_cycles_the_angles():
    M = C.ladder_sized(3, 33)
    assert set(C.branches(M).ravel().tolist()) == {0, 1, 2, 3}


# ------------------------------------------------------------------------------------------ 50 digits
def _mp_maps(M, bbox, diff):
    """The contract of tests/_coord_map_ref.py's docstring with mpmath scalars, 50 digits: (K,K,T') nested lists."""
    mp = pytest.importorskip("mpmath")
    mp.mp.dps = 50
    f = mp.mpf
    T, K = M.shape[:2]
    lam, pi = 1 / (2 * f(bbox)), mp.pi
    R = [[[[f(float(M[t, k, a, b])) for b in range(3)] for a in range(3)] for k in range(K)] for t in range(T)]
    xyz = [[[f(float(M[t, k, a, 3])) for a in range(3)] for k in range(K)] for t in range(T)]

    def norm(v):
        return mp.sqrt(sum(x * x for x in v))

    def quat(m):
        tr = m[0][0] + m[1][1] + m[2][2]
        dec = [m[0][0], m[1][1], m[2][2], tr]
        c = max(range(4), key=lambda i: (dec[i], -i))                    # first maximum
        q = [None] * 4
        if c == 3:
            q = [m[2][1] - m[1][2], m[0][2] - m[2][0], m[1][0] - m[0][1], 1 + tr]
        else:
            i, j, k = c, (c + 1) % 3, (c + 2) % 3
            q[i], q[j], q[k], q[3] = 1 - tr + 2 * m[i][i], m[j][i] + m[i][j], m[k][i] + m[i][k], m[k][j] - m[j][k]
        n = norm(q)
        q = [x / n for x in q]
        if q[3] < 0:
            q = [-x for x in q]
        angle = 2 * mp.atan2(norm(q[:3]), q[3])
        scale = 2 + angle ** 2 / 12 + 7 * angle ** 4 / 2880 if abs(angle) <= f(1e-3) else angle / mp.sin(angle / 2)
        v = [scale * x for x in q[:3]]
        nv = norm(v)
        s2 = f(0.5) - nv ** 2 / 48 + nv ** 4 / 3840 if nv <= f(1e-3) else mp.sin(nv / 2) / nv
        return [s2 * x for x in v] + [mp.cos(nv / 2)]

    out = np.empty((K, K, T - 1 if diff else T), object)
    cosines = np.empty((K, K, T), object)
    for i in range(T - 1 if diff else T):
        if diff:
            t = [[b - a for a, b in zip(xyz[i][k], xyz[i + 1][k])] for k in range(K)]
            q = [quat([[sum(R[i][k][c][a] * R[i + 1][k][c][b] for c in range(3)) for b in range(3)] for a in range(3)])
                 for k in range(K)]
            dx = [[lam * norm([a - b for a, b in zip(t[j], t[k])]) for k in range(K)] for j in range(K)]
            dr = [[4 * mp.asin(min(norm([b - a for a, b in zip(q[j], q[k])]), norm([b + a for a, b in zip(q[j], q[k])])) / 2) / pi
                   for k in range(K)] for j in range(K)]
            for j in range(K):
                for k in range(K):
                    out[j, k, i] = norm([dx[j][m] - dx[k][m] for m in range(K)]) + norm([dr[j][m] - dr[k][m] for m in range(K)])
        else:
            for j in range(K):
                for k in range(K):
                    c = (sum(R[i][j][a][b] * R[i][k][a][b] for a in range(3) for b in range(3)) - 1) / 2
                    cosines[j, k, i] = c
                    out[j, k, i] = lam * norm([a - b for a, b in zip(xyz[i][j], xyz[i][k])]) + mp.acos(max(min(c, 1), -1)) / pi
    return out, cosines


def _ld(x):
    """mpmath array -> long double (through the leading 21 digits and a float64 remainder, both exact enough)."""
    hi = np.vectorize(float)(x)
    lo = np.vectorize(lambda v, h: float(v - h))(x, hi)
    return hi.astype(LD) + lo.astype(LD)


@pytest.mark.parametrize("name", ["ladder", "ladder_f32", "fan"])
def test_reference_vs_mpmath_50_digits(name):
    M = _inputs(name)
    K = M.shape[1]
    if name != "fan":
        want, _ = _mp_maps(M, C.BBOX, True)
        got, got_sum = C.coord_dist_map_ref(M, C.BBOX, True)
        err = float(np.abs(got - _ld(want)).max())
        print(f"{name} diff=1: long double vs 50 digits {err:.3g} (map up to {float(got.max()):.3g})")
        assert err <= 2.0 ** -60                               # 16 ulp of long double at 1: three decimal digits below fp64
        assert float(np.abs(got_sum - _ld(want).sum(-1)).max()) <= 2.0 ** -58
    # diff = 0: acos magnifies the last bits of a cosine next to +-1, in long double too, so the check is made on the cosine
    # (to 2^-60) and on the map through the interval the long-double cosine's own rounding (11 * 2^-64 (S + 1)) admits
    want, cosines = _mp_maps(M, C.BBOX, False)
    got, _ = C.coord_dist_map_ref(M, C.BBOX, False)
    idx = np.arange(K)
    for i in range(M.shape[0]):
        c, S = C._cos_terms(M, i, idx, idx)
        assert float(np.abs(c - _ld(cosines[:, :, i])).max()) <= 2.0 ** -60
        lo, hi = C.cos_interval(M, i, idx, idx, delta=11 * LD(2.0) ** -64 * (S + 1))
        w = np.vectorize(float)(want[:, :, i])
        assert np.all((w >= lo) & (w <= hi))
        g = got[:, :, i].astype(np.float64)
        assert np.all((g >= lo) & (g <= hi))
        far = np.abs(c) < 0.999                                # away from +-1 the map itself agrees to long-double accuracy
        assert float(np.abs(got[:, :, i] - _ld(want[:, :, i]))[far].max()) <= 2.0 ** -58


# ------------------------------------------------------------------------------------------ scipy
@pytest.mark.parametrize("name", ["ladder", "fan"])
def test_reference_vs_scipy_rotation_magnitudes(name):
    """Orthonormal inputs only: the rotational pair terms are the magnitudes of the relative rotations / pi."""
    from scipy.spatial.transform import Rotation
    M = _inputs(name)[:, :8] if name == "fan" else _inputs(name)          # (the fan's float32-rounded tracks left out)
    K = M.shape[1]
    idx = np.arange(K)
    M0 = M.copy()
    M0[:, :, :3, 3] = 0                                        # (the interval then holds the rotational term alone)
    for i in range(M.shape[0]):
        rot = Rotation.from_matrix(M[i, :, :3, :3])
        mag = np.array([(rot[j].inv() * rot).magnitude() for j in range(K)]) / np.pi
        lo, hi = C.cos_interval(M0, i, idx, idx)
        assert np.all((mag >= lo) & (mag <= hi))
        got = C.pair_matrices(M, i, C.BBOX, False)[1].astype(np.float64)
        assert np.all((got >= lo) & (got <= hi))
    for i in range(M.shape[0] - 1):
        rot = Rotation.from_matrix(C.relative_rotations(M, np.float64)[i])
        mag = np.array([(rot[j].inv() * rot).magnitude() for j in range(K)]) / np.pi
        got = C.pair_matrices(M, i, C.BBOX, True)[1].astype(np.float64)
        np.testing.assert_allclose(got, mag, rtol=0, atol=1e-14)


# ------------------------------------------------------------------------------------------ the fp64 oracle
@pytest.mark.parametrize("name", ["ladder", "ladder_equal_levers", "ladder_f32"] + SIZES, ids=str)
def test_oracle_diff1_error_is_the_quoted_one(name):
    """Largest |fp64 oracle - long double| per input, printed (pytest -s): the figure each device bound is 8 x of, rounded up
    to a power of two (C.ORACLE_ERR_DIFF1).  K >= 481 measures the row-loop oracle on the sampled rows."""
    from oracle import coord_map as ocm
    M = _inputs(name)
    K = M.shape[1]
    rows = C.sample_rows(K) if K >= 481 else None
    ref, ref_sum = C.coord_dist_map_ref(M, C.BBOX, True, rows)
    got, got_sum = (C.coord_dist_map_rows if K >= 481 else ocm.coord_dist_map)(M, C.BBOX, True)
    if rows is not None:
        got, got_sum = got[rows], got_sum[rows]
    err, err_sum = float(np.abs(got - ref).max()), float(np.abs(got_sum - ref_sum).max())
    bound = C.diff1_bound(name)
    print(f"{name} diff=1: oracle vs long double {err:.3g} (sum {err_sum:.3g}), quoted {C.ORACLE_ERR_DIFF1[name]:.3g}, "
          f"device bound {bound:.3g}, map up to {float(ref.max()):.3g}")
    assert bound == C.bound_from(C.ORACLE_ERR_DIFF1[name])
    assert K > 64 or bound <= 1e-12
    assert err <= bound and err_sum <= (M.shape[0] - 1) * bound      # another numpy build may move the last bits, not this
    if K < 481:                                                # the two fp64 statements agree with each other as well
        rows_map, _ = C.coord_dist_map_rows(M, C.BBOX, True)
        assert float(np.abs(rows_map - got).max()) <= bound


@pytest.mark.parametrize("name", ["ladder", "ladder_f32", "fan"] + SIZES, ids=str)
def test_oracle_diff0_lies_in_the_cosine_interval(name):
    from oracle import coord_map as ocm
    M = _inputs(name)
    T, K = M.shape[:2]
    got, got_sum = ocm.coord_dist_map(M, C.BBOX, False)
    idx = np.arange(K)
    lo, hi = (np.stack(x, -1) for x in zip(*[C.cos_interval(M, i, idx, idx) for i in range(T)]))
    assert np.all((got >= lo) & (got <= hi))
    slo, shi = C.sum_interval(lo, hi)
    assert np.all((got_sum >= slo) & (got_sum <= shi))
    ref, _ = C.coord_dist_map_ref(M, C.BBOX, False)
    print(f"{name} diff=0: oracle vs long double {float(np.abs(got - ref).max()):.3g}, widest interval {float((hi - lo).max()):.3g}")


def test_cos_interval_is_tight_away_from_the_clamp_and_catches_slips():
    """A float32 cosine, a dropped clamp and a 1e-13 slip fall outside; the interval is ~1e-15 wide at a right angle."""
    M, info = C.fan()
    idx = np.arange(M.shape[1])
    lo, hi = C.cos_interval(M, 0, idx, idx)
    assert (hi - lo)[0, 4] < 4e-15 and (hi - lo)[0, 3] < 4e-15            # pi / 2 and 1 rad
    R = M[0, :, :3, :3]
    t = np.linalg.norm(M[0, :, None, :3, 3] - M[0, None, :, :3, 3], axis=-1) / (2 * C.BBOX)
    cs = 0.5 * (np.einsum("jab,kab->jk", R, R) - 1)
    with np.errstate(invalid="ignore"):
        no_clamp = t + np.arccos(cs) / np.pi
    j, k = info["over"]
    assert np.isnan(no_clamp[j, k]) and not (no_clamp[j, k] >= lo[j, k])
    cs32 = 0.5 * (np.einsum("jab,kab->jk", R.astype(np.float32), R.astype(np.float32)).astype(np.float64) - 1)
    f32 = t + np.arccos(np.clip(cs32, -1, 1)) / np.pi
    assert not np.all((f32 >= lo) & (f32 <= hi))
    good = t + np.arccos(np.clip(cs, -1, 1)) / np.pi
    assert np.all((good >= lo) & (good <= hi))
    assert not (lo[0, 3] <= good[0, 3] + 1e-13 <= hi[0, 3])
    # NaN poses give NaN bounds: nothing compares inside them
    Mn = M.copy()
    Mn[0, 2, 0, 1] = np.nan
    lo, hi = C.cos_interval(Mn, 0, idx, idx)
    assert np.isnan(lo[2]).all() and np.isnan(lo[:, 2]).all() and np.isfinite(np.delete(np.delete(lo, 2, 0), 2, 1)).all()
