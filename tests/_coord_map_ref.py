"""High-precision statement of the pose distance maps (the contract in the header of csrc/coord_map.hip) for the tests
of creg_coord_dist_map_f64, written from the input matrices up in numpy.longdouble; independent of oracle/coord_map.py.

    diff = 1, per step i < T-1 and track k:
        rel_k = R_{i,k}^T R_{i+1,k};  q_k = unit quaternion of rel_k by the decision-matrix form (argmax of
        [m00, m11, m22, tr], first maximum: branches 0, 1, 2, 3), flipped to q.w >= 0, taken to the rotation vector
        (angle = 2 atan2(|q.xyz|, q.w); scale = angle / sin(angle / 2), its Taylor series when |angle| <= 1e-3) and back
        (sin(|v| / 2) / |v|, its Taylor series when |v| <= 1e-3;  w = cos(|v| / 2))
        d_xyz[j][k] = |dt_j - dt_k| / (2 bbox), dt = t_{i+1} - t_i;   d_rpy[j][k] = 4 asin(min(|q_k - q_j|, |q_k + q_j|) / 2) / pi
        map[j][k][i] = |d_xyz[j][:] - d_xyz[k][:]|_2 + |d_rpy[j][:] - d_rpy[k][:]|_2
    diff = 0, per step i < T:
        map[j][k][i] = |t_j - t_k| / (2 bbox) + acos(clamp((tr(R_j^T R_k) - 1) / 2, -1, 1)) / pi     (NaN stays NaN)
    sum_map[j][k] = sum_i |map[j][k][i]|
(The map itself does not depend on the flip to q.w >= 0: the round trip takes -q to -q and the distance takes the smaller
of |q_k - q_j| and |q_k + q_j|.  The flip fixes the rotation vector the reference's loops hold in between; a kernel
without it computes the same map to rounding, so no test of the map can tell.)

`coord_dist_map_ref` evaluates this in long double (`rows=` restricts the rows j, so K = 1024 needs no K x K x K array);
`coord_dist_map_rows` is the same arithmetic in float64, the fp64 yardstick for every row of the large cases.

The diff = 0 bound (`cos_interval`).  acos is ill-conditioned at +-1, so a blanket tolerance on the map either hides
errors where the cosine is far from +-1 or rejects correct results next to it.  The bound is set on the cosine instead.
c = 0.5 (tr - 1) with tr = sum of 9 products a_i b_i.  In any fp64 evaluation (any order, with or without fma) every
product is rounded at most once and then passes through at most 10 additions (8 inside the sum, one that may start from
an explicit 0, one for the - 1); the factor 0.5 is exact.  With u = 2^-53 and gamma_n = n u / (1 - n u) the standard
dot-product bound (Higham, Accuracy and Stability of Numerical Algorithms, 3.1) gives

    |fl(c) - c| <= 0.5 gamma_11 (sum_i |a_i b_i| + 1) =: delta        (`cos_delta`; about 2.4e-15 for rotations)

so a correct result lies in [acos(min(c + delta, 1)), acos(max(c - delta, -1))] / pi plus the translation term, both
evaluated in long double, widened by 4 ulp of the result for acos, the product with 1 / pi, the translation term's own
few roundings and the final addition.  (The long-double c carries 11 * 2^-64 (S + 1), which is added to delta.)

The builders produce the inputs the tests share: the step-rotation ladder (`ladder`, `ladder_sized`), its float32-rounded
form and the diff = 0 orientation fan (`fan`).
"""
from concurrent.futures import ThreadPoolExecutor

import numpy as np

LD = np.longdouble
if np.finfo(LD).eps >= 1e-18:
    raise RuntimeError("tests/_coord_map_ref.py needs a numpy.longdouble wider than float64 (eps < 1e-18), got eps = "
                       f"{np.finfo(LD).eps}")
PI = 4 * np.arctan(LD(1))
U = 2.0 ** -53
BBOX = 0.9                                    # the bounding box every builder's translations are scaled for


def _pi(dtype):
    return PI if dtype is LD else dtype(np.pi)


# ------------------------------------------------------------------------------------------ the contract
def rotmat_to_unitquat(m):
    """(...,3,3) -> ((...,4) xyzw, branch (...)) in m's dtype: the decision-matrix form."""
    tr = (m[..., 0, 0] + m[..., 1, 1]) + m[..., 2, 2]
    c = np.argmax(np.stack([m[..., 0, 0], m[..., 1, 1], m[..., 2, 2], tr], -1), -1)      # first maximum
    cand = np.empty(m.shape[:-2] + (4, 4), m.dtype)
    for i in range(3):
        j, k = (i + 1) % 3, (i + 2) % 3
        cand[..., i, i] = 1 - tr + 2 * m[..., i, i]
        cand[..., i, j] = m[..., j, i] + m[..., i, j]
        cand[..., i, k] = m[..., k, i] + m[..., i, k]
        cand[..., i, 3] = m[..., k, j] - m[..., j, k]
    cand[..., 3, 0] = m[..., 2, 1] - m[..., 1, 2]
    cand[..., 3, 1] = m[..., 0, 2] - m[..., 2, 0]
    cand[..., 3, 2] = m[..., 1, 0] - m[..., 0, 1]
    cand[..., 3, 3] = 1 + tr
    q = np.take_along_axis(cand, c[..., None, None], -2)[..., 0, :]
    return q / np.sqrt((q * q).sum(-1))[..., None], c


def rotvec_roundtrip(q):
    """unit quaternion -> shortest-arc rotation vector -> unit quaternion, with both Taylor switches at 1e-3."""
    q = np.where(q[..., 3:] < 0, -q, q)
    half = np.arctan2(np.sqrt((q[..., :3] ** 2).sum(-1)), q[..., 3])
    angle = 2 * half
    with np.errstate(divide="ignore", invalid="ignore"):
        scale = np.where(np.abs(angle) <= 1e-3, 2 + angle ** 2 / 12 + 7 * angle ** 4 / 2880, angle / np.sin(half))
        v = scale[..., None] * q[..., :3]
        nv = np.sqrt((v * v).sum(-1))
        s2 = np.where(nv <= 1e-3, 0.5 - nv ** 2 / 48 + nv ** 4 / 3840, np.sin(nv / 2) / nv)
    return np.concatenate([s2[..., None] * v, np.cos(nv / 2)[..., None]], -1)


def relative_rotations(M, dtype=LD):
    """(T,K,4,4) -> R_i^T R_{i+1} (T-1,K,3,3)."""
    R = np.asarray(M, np.float64)[..., :3, :3].astype(dtype)
    return np.swapaxes(R[:-1], -1, -2) @ R[1:]


def branches(M):
    """The decision-matrix branch of every relative rotation (T-1,K), decided in long double."""
    return rotmat_to_unitquat(relative_rotations(M))[1]


def pair_matrices(M, i, bounding_box, diff, dtype=LD):
    """(d_xyz, d_rpy), both (K,K), of step i: the two pair terms before they are combined."""
    M = np.asarray(M, np.float64)
    lam = 1 / (2 * dtype(bounding_box))
    xyz = M[:, :, :3, 3].astype(dtype)
    if diff:
        t = xyz[i + 1] - xyz[i]
        q = rotvec_roundtrip(rotmat_to_unitquat(relative_rotations(M[i:i + 2], dtype)[0])[0])
        sm = np.sqrt(((q[None] - q[:, None]) ** 2).sum(-1))
        sp = np.sqrt(((q[None] + q[:, None]) ** 2).sum(-1))
        d_rpy = 4 * np.arcsin(0.5 * np.minimum(sm, sp)) / _pi(dtype)
    else:
        t = xyz[i]
        R = M[i, :, :3, :3].astype(dtype)
        d_rpy = np.arccos(np.clip(0.5 * (np.einsum("jab,kab->jk", R, R) - 1), -1, 1)) / _pi(dtype)
    return lam * np.sqrt(((t[:, None] - t[None]) ** 2).sum(-1)), d_rpy


def _maps(M, bounding_box, diff, rows, dtype):
    M = np.asarray(M, np.float64)
    T, K = M.shape[:2]
    rows = np.arange(K) if rows is None else np.asarray(rows)
    Tn = T - 1 if diff else T
    out = np.empty((len(rows), K, Tn), dtype)
    for i in range(Tn):
        dx, dr = pair_matrices(M, i, bounding_box, diff, dtype)
        if not diff:
            out[:, :, i] = dx[rows] + dr[rows]
            continue

        def row(j):                                           # distance between ROWS j and k of each pair matrix
            ex, er = dx - dx[j], dr - dr[j]
            return np.sqrt(np.einsum("km,km->k", ex, ex)) + np.sqrt(np.einsum("km,km->k", er, er))
        if K < 256:
            out[:, :, i] = [row(j) for j in rows]
        else:                                                 # numpy drops the GIL inside each K x K pass
            with ThreadPoolExecutor(8) as pool:
                out[:, :, i] = list(pool.map(row, rows))
    return out, np.abs(out).sum(-1)


def coord_dist_map_ref(M, bounding_box, diff=True, rows=None):
    """(map (len(rows),K,T'), sum_map (len(rows),K)) in long double; rows = None is every row j."""
    return _maps(M, bounding_box, diff, rows, LD)


def coord_dist_map_rows(M, bounding_box, diff=True):
    """The same contract in float64, one row j at a time: (map (K,K,T'), sum_map (K,K)) without a K x K x K temporary."""
    return _maps(M, bounding_box, diff, None, np.float64)


# ------------------------------------------------------------------------------------------ the diff = 0 bound
def _cos_terms(M, i, j, k):
    R = np.asarray(M, np.float64)[i, :, :3, :3].astype(LD)
    Rj, Rk = R[np.atleast_1d(j)], R[np.atleast_1d(k)]
    return 0.5 * (np.einsum("jab,kab->jk", Rj, Rk) - 1), np.einsum("jab,kab->jk", np.abs(Rj), np.abs(Rk))


def cos_delta(M, i, j, k):
    """delta of the module docstring for rows j and columns k of step i: (len(j), len(k)) long double."""
    _, S = _cos_terms(M, i, j, k)
    return (0.5 * (11 * U / (1 - 11 * U)) + 11 * LD(2.0) ** -64) * (S + 1)


def cos_interval(M, i, j, k, delta=None, bounding_box=BBOX):
    """(lo, hi) float64, (len(j), len(k)): the interval a correct diff = 0 entry [j][k][i] lies in.  delta = None takes
    `cos_delta`; NaN poses give NaN bounds."""
    M = np.asarray(M, np.float64)
    c, _ = _cos_terms(M, i, j, k)
    delta = cos_delta(M, i, j, k) if delta is None else delta
    t = M[i, :, :3, 3].astype(LD)
    trans = np.sqrt(((t[np.atleast_1d(j)][:, None] - t[np.atleast_1d(k)][None]) ** 2).sum(-1)) / (2 * LD(bounding_box))
    lo = np.arccos(np.clip(c + delta, -1, 1)) / PI + trans
    hi = np.arccos(np.clip(c - delta, -1, 1)) / PI + trans
    lo64, hi64 = lo.astype(np.float64), hi.astype(np.float64)
    lo64 = np.where(lo64.astype(LD) > lo, np.nextafter(lo64, -np.inf), lo64)        # round outwards
    hi64 = np.where(hi64.astype(LD) < hi, np.nextafter(hi64, np.inf), hi64)
    w = 4 * np.spacing(hi64)
    return lo64 - w, hi64 + w


def sum_interval(lo, hi):
    """Bounds of sum_i |map| from per-step bounds (..., T'): the serial fp64 sum adds at most T' - 1 roundings."""
    n = lo.shape[-1]
    slo, shi = np.maximum(lo, 0).sum(-1), hi.sum(-1)           # lo >= 0 apart from its ulp widening at 0
    w = n * np.spacing(shi)
    return slo - w, shi + w


# ------------------------------------------------------------------------------------------ builders
ANGLES = [LD(0), LD(1e-9), LD(np.nextafter(1e-3, 0)), LD(np.nextafter(1e-3, 1)), LD(0.3), 2 * PI / 3, LD(2.0), LD(2.5),
          PI - LD(1e-6), PI - LD(1e-9), PI]
# rotations by pi about x, y, z and (1,1,0)/sqrt2 as exact matrices: dec = [1,-1,-1,-1] ... and the tie [0,0,-1,-1]
EXACT_PI = [np.diag([1.0, -1.0, -1.0]), np.diag([-1.0, 1.0, -1.0]), np.diag([-1.0, -1.0, 1.0]),
            np.array([[0.0, 1.0, 0.0], [1.0, 0.0, 0.0], [0.0, 0.0, -1.0]])]


def axis_angle_matrix(axis, angle):
    """Rodrigues in long double; 1 - cos as 2 sin^2(angle / 2), so 1e-9 rad keeps its bits."""
    n = np.asarray(axis, LD)
    n = n / np.sqrt((n * n).sum())
    a = LD(angle)
    Kx = np.array([[0, -n[2], n[1]], [n[2], 0, -n[0]], [-n[1], n[0], 0]], LD)
    return np.eye(3, dtype=LD) + np.sin(a) * Kx + 2 * np.sin(a / 2) ** 2 * (Kx @ Kx)


def _axis(rng, dominant):
    """A random axis whose component `dominant` is the largest by a margin: past 2 pi / 3 the branch taken is `dominant`."""
    a = rng.uniform(-0.5, 0.5, 3)
    a[dominant] = rng.choice([-1.0, 1.0])
    return a


def _tracks(rng, T, steps, start_identity):
    """Poses (T,K,4,4) of tracks that turn by steps[k] and back, alternately, from a random (or the identity) start, about
    a random pivot with a random lever arm, carried along a random walk.  Returns the float64 poses and the long-double
    parts (R (T,K,3,3), pivot (K,3), lever (K,3), walk (T,K,3)) so that tracks can be rebuilt with shared parts."""
    K = len(steps)
    R = np.empty((T, K, 3, 3), LD)
    for k in range(K):
        R0 = np.eye(3, dtype=LD) if start_identity[k] else axis_angle_matrix(rng.normal(size=3), rng.uniform(0, np.pi))
        R1 = R0 @ steps[k]
        R[0::2, k], R[1::2, k] = R0, R1
    pivot = rng.uniform(-0.3, 0.3, (K, 3)).astype(LD)
    lever = rng.uniform(-0.2, 0.2, (K, 3)).astype(LD)
    walk = np.cumsum(rng.normal(scale=0.01, size=(T, K, 3)), 0).astype(LD)
    return R, pivot, lever, walk


def _poses(R, pivot, lever, walk):
    T, K = R.shape[:2]
    M = np.tile(np.eye(4), (T, K, 1, 1))
    M[:, :, :3, :3] = R.astype(np.float64)
    M[:, :, :3, 3] = (pivot[None] + np.einsum("tkab,kb->tka", R, lever) + walk).astype(np.float64)
    return M


def round_steps_f32(M):
    """The on-disk layout: frame 0 float64, every later frame rounded to float32 (rotations no longer orthonormal)."""
    M = np.array(M, np.float64)
    M[1:] = M[1:].astype(np.float32).astype(np.float64)
    return M


def ladder(T=4, seed=0, f32_steps=False, equal_levers=False):
    """The step-rotation ladder: K = 17 tracks.
      0..10   relative rotation ANGLES[k] about a random axis whose dominant component is k % 3, from a random start
      11..14  EXACT_PI (pi about x, y, z and (1,1,0)/sqrt2), from the identity, so the relative rotations are exact
      15      an exact copy of track 6
      16      track 7's rotation, pivot and walk with another lever arm (two clusters of one rigid link); with
              equal_levers the lever arm is track 7's as well
    Returns (M (T,K,4,4) float64, info) with info['branches'] (T-1,K) decided in long double, info['copy'] = (6, 15),
    info['same_link'] = (7, 16)."""
    rng = np.random.default_rng(seed)
    steps = [axis_angle_matrix(_axis(rng, k % 3), a) for k, a in enumerate(ANGLES)] + [e.astype(LD) for e in EXACT_PI]
    n = len(steps)
    R, pivot, lever, walk = _tracks(rng, T, steps, [k >= len(ANGLES) for k in range(n)])
    lever16 = lever[7] if equal_levers else rng.uniform(-0.2, 0.2, 3).astype(LD)
    R = np.concatenate([R, R[:, [6, 7]]], 1)
    pivot = np.concatenate([pivot, pivot[[6, 7]]])
    lever = np.concatenate([lever, lever[[6]], lever16[None]])
    walk = np.concatenate([walk, walk[:, [6, 7]]], 1)
    M = _poses(R, pivot, lever, walk)
    if f32_steps:
        M = round_steps_f32(M)
    return M, {"branches": branches(M), "copy": (6, 15), "same_link": (7, 16), "angles": ANGLES}


def ladder_sized(T, K, seed=0):
    """Ladder-style poses (T,K,4,4) at any size: track k turns by ANGLES[k % 11] (dominant axis component k % 3) and back."""
    rng = np.random.default_rng(1000 * T + K + seed)
    steps = [axis_angle_matrix(_axis(rng, k % 3), ANGLES[k % len(ANGLES)]) for k in range(K)]
    return _poses(*_tracks(rng, T, steps, [False] * K))


FAN_ANGLES = [LD(0), LD(1e-8), LD(1e-4), LD(1), PI / 2, PI - LD(1e-4), PI - LD(1e-8), PI]


def fan(seed=0):
    """The diff = 0 orientation fan: one step, K = 11 tracks.
      0..7   R0 Rot(axis, FAN_ANGLES[k]): track 0 against track k stands at FAN_ANGLES[k]
      8, 9   one float32-rounded rotation twice: the cosine of the pair is (|A|_F^2 - 1) / 2 > 1
      10     the float32 rounding of that rotation turned by pi: the cosine of (8, 10) is below -1
    The float32 block's seed is searched upwards from `seed` until both cosines clear +-1 by 1e-9 (float32 rounding moves
    them by ~1e-7, the fp64 evaluation by ~1e-15).  Returns (M (1,11,4,4), info) with info['over'] = (8, 9),
    info['under'] = (8, 10), info['cos_over'], info['cos_under'] (long double) and info['f32_seed']."""
    rng = np.random.default_rng(seed)
    R0, axis = axis_angle_matrix(rng.normal(size=3), rng.uniform(0, np.pi)), rng.normal(size=3)
    R = [R0 @ axis_angle_matrix(axis, a) for a in FAN_ANGLES]
    for s in range(seed, seed + 1000):
        r2 = np.random.default_rng([s, 1])
        A = axis_angle_matrix(r2.normal(size=3), r2.uniform(0, np.pi))
        B = A @ axis_angle_matrix(r2.normal(size=3), PI)
        A32, B32 = (x.astype(np.float32).astype(LD) for x in (A, B))
        over, under = 0.5 * ((A32 * A32).sum() - 1), 0.5 * ((A32 * B32).sum() - 1)
        if over > 1 + 1e-9 and under < -1 - 1e-9:
            break
    else:
        raise RuntimeError("fan: no float32 block with cosines past +-1 found")
    R = np.array(R + [A32, A32, B32])[None]
    K = R.shape[1]
    M = _poses(R, rng.uniform(-0.3, 0.3, (K, 3)).astype(LD), np.zeros((K, 3), LD), np.zeros((1, K, 3), LD))
    return M, {"over": (8, 9), "under": (8, 10), "cos_over": over, "cos_under": under, "f32_seed": s, "angles": FAN_ANGLES}


def bound_from(measured):
    """The diff = 1 device bound from the fp64 oracle's own error against long double: 8 x, rounded up to a power of two."""
    return float(2.0 ** np.ceil(np.log2(8 * float(measured)))) if measured > 0 else 0.0


def sample_rows(K, n=64):
    """A fixed sample of n rows j, with 0 and K - 1 among them, for the long-double reference of the large cases."""
    rng = np.random.default_rng(K)
    return np.unique(np.concatenate([[0, K - 1], 1 + rng.choice(K - 2, n - 2, replace=False)]))


# Largest |fp64 oracle - long double| of the diff = 1 map per input, as tests/test_coord_map_cpu.py measures and prints it
# (oracle/coord_map.py; from K = 481 `coord_dist_map_rows` on `sample_rows`).  Keys: builder name or (T, K) of `ladder_sized`.
ORACLE_ERR_DIFF1 = {
    "ladder": 9.32e-16, "ladder_equal_levers": 9.77e-16, "ladder_f32": 1.30e-15,                  # bounds 2^-46 = 1.43e-14
    (2, 1): 0.0,                                    # K = 1: the map is exactly 0, here and on the device
    (3, 32): 1.74e-15, (3, 33): 1.81e-15,           # 2^-46, 2^-45 = 2.85e-14
    (3, 481): 1.11e-14, (3, 482): 1.08e-14,         # 2^-43 = 1.14e-13
    (2, 1024): 2.93e-14,                            # 2^-41 = 4.55e-13
    (1025, 3): 1.48e-17,                            # 2^-52 = 2.23e-16 (three tracks at 0, 1e-9 and 1e-3 rad: a map below 0.06)
}


def diff1_bound(name):
    """The device bound of a diff = 1 map entry for that input; sum_map gets T' times it."""
    return bound_from(ORACLE_ERR_DIFF1[name])
