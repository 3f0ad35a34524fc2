"""Rotation edge families and plain numpy restatements of the pose-conversion templates (test infrastructure).

The families are deterministic and seeded.  Every row carries a label naming the decision of
autourdf_amd/csrc/creg_dev.h (or coord_map.hip) it is built to reach: which `matrix_to_quat` candidate
wins (first maximum on ties), the `w >= 0` flip, the FLT_EPSILON clamps of `se3_to_dq` / DQ_INV, the
branch of `rotmat_to_unitquat_xyzw`.

The restatements follow the kernels' operation order and evaluate one elementwise op at a time in the
requested dtype (np.float32 for the row kernels and the train plan, np.float64 for k_pose_coords).  The
library is built with -ffp-contract=off and IEEE-rounded division and square root, so for these
functions (no transcendentals) a restatement and the kernel give the same bits.  They are written
independently of oracle/transforms.py and oracle/dq.py, which stay the fp64 reference.
"""
import numpy as np

FLT_EPSILON = float(np.finfo(np.float32).eps)
AXES = {"x": (1.0, 0.0, 0.0), "y": (0.0, 1.0, 0.0), "z": (0.0, 0.0, 1.0)}
DELTAS = (1e-7, 1e-5, 1e-3)


# ------------------------------------------------------------------------------------------ fp64 builders
def rodrigues(axis, theta):
    """(n,3) axes (normalised here), (n,) angles -> (n,3,3) fp64 rotations."""
    n = np.asarray(axis, np.float64).reshape(-1, 3)
    n = n / np.linalg.norm(n, axis=1, keepdims=True)
    th = np.broadcast_to(np.asarray(theta, np.float64), (len(n),))
    c, s = np.cos(th)[:, None, None], np.sin(th)[:, None, None]
    K = np.zeros((len(n), 3, 3))
    K[:, 0, 1], K[:, 0, 2], K[:, 1, 2] = -n[:, 2], n[:, 1], -n[:, 0]
    K[:, 1, 0], K[:, 2, 0], K[:, 2, 1] = n[:, 2], -n[:, 1], n[:, 0]
    return c * np.eye(3) + s * K + (1 - c) * (n[:, :, None] * n[:, None, :])


def quat_to_rot64(q):
    q = np.asarray(q, np.float64)
    q = q / np.linalg.norm(q, axis=1, keepdims=True)
    w, x, y, z = q.T
    return np.stack([1 - 2 * (y * y + z * z), 2 * (x * y - z * w), 2 * (x * z + y * w),
                     2 * (x * y + z * w), 1 - 2 * (x * x + z * z), 2 * (y * z - x * w),
                     2 * (x * z - y * w), 2 * (y * z + x * w), 1 - 2 * (x * x + y * y)], 1).reshape(-1, 3, 3)


def euler_xyz_to_rot64(e):
    """Rx(a) Ry(b) Rz(c), the XYZ convention of the train plan's rpy path."""
    a, b, c = np.asarray(e, np.float64).T
    ca, sa, cb, sb, cc, sc = np.cos(a), np.sin(a), np.cos(b), np.sin(b), np.cos(c), np.sin(c)
    return np.stack([cb * cc, -cb * sc, sb, ca * sc + sa * sb * cc, ca * cc - sa * sb * sc, -sa * cb,
                     sa * sc - ca * sb * cc, sa * cc + ca * sb * sc, ca * cb], 1).reshape(-1, 3, 3)


def _random_axes(rng, n):
    v = rng.normal(size=(n, 3))
    return v / np.linalg.norm(v, axis=1, keepdims=True)


def _matmul3_f32(A, B):
    """Batched 3x3 product in float32, one rounding per op, fixed order (independent of any BLAS)."""
    A, B = A.astype(np.float32), B.astype(np.float32)
    C = np.empty_like(A)
    for i in range(3):
        for j in range(3):
            C[:, i, j] = (A[:, i, 0] * B[:, 0, j] + A[:, i, 1] * B[:, 1, j]) + A[:, i, 2] * B[:, 2, j]
    return C


# ------------------------------------------------------------------------------------------ families
def rotation_families(seed=0, n_random=4096):
    """[(label, R64 (n,3,3), R32 (n,3,3))]; R32 is the float32 input, R64 the design (for the fp32-built
    families R64 = R32 widened)."""
    rng = np.random.default_rng(seed)
    fams = []

    def add(label, R64, R32=None):
        R64 = np.asarray(R64, np.float64).reshape(-1, 3, 3)
        fams.append((label, R64, (R64 if R32 is None else R32).astype(np.float32)))

    add("identity", np.eye(3))
    # exact pi turns: w = 0; x / y / z single candidates, (1,1,0) a qa[1] == qa[2] tie, (1,1,1) three near-equal ones
    pi_exact = [np.diag([1.0, -1.0, -1.0]), np.diag([-1.0, 1.0, -1.0]), np.diag([-1.0, -1.0, 1.0]),
                np.array([[0.0, 1.0, 0.0], [1.0, 0.0, 0.0], [0.0, 0.0, -1.0]])]
    n111 = np.full(3, 1 / np.sqrt(3.0))
    pi_exact.append(2 * np.outer(n111, n111) - np.eye(3))
    add("pi_exact", np.stack(pi_exact))
    # the same turns with a signed zero where cand[0] = m21 - m12 (resp. m02 - m20, m10 - m01) is formed:
    # (-0) - (+0) = -0, so w = -0.0 and the flip test `w < 0` must leave it alone
    sz = np.stack(pi_exact[:4]).copy()
    sz[0, 2, 1] = -0.0
    sz[1, 0, 2] = -0.0
    sz[2, 1, 0] = -0.0
    sz[3, 2, 1] = -0.0
    add("pi_signed_zero", sz)
    # pi from the trigonometric route (sin(pi) = 1.2e-16, not 0), about the axes and the two diagonals
    ax = np.array([AXES["x"], AXES["y"], AXES["z"], (1, 1, 0), (1, 1, 1), (-1, 1, 0), (1, -1, -1)], np.float64)
    add("pi_trig", rodrigues(ax, np.pi))
    for d in DELTAS:                          # pi +- delta: the sign boundary of w (w ~ -+delta / 2)
        add(f"pi_plus_{d:g}", rodrigues(ax, np.pi + d))
        add(f"pi_minus_{d:g}", rodrigues(ax, np.pi - d))
    # pi/2 exactly (qa[0] == qa[axis + 1]: 90 deg about x gives qa[0] == qa[1]) and pi/2 +- delta
    half = [np.array([[1.0, 0, 0], [0, 0, -1], [0, 1, 0]]), np.array([[0.0, 0, 1], [0, 1, 0], [-1, 0, 0]]),
            np.array([[0.0, -1, 0], [1, 0, 0], [0, 0, 1]])]
    add("half_pi_exact", np.stack(half + [h.T for h in half]))
    ax3 = np.array([AXES["x"], AXES["y"], AXES["z"], (-1, 0, 0), (0, -1, 0), (0, 0, -1)], np.float64)
    add("half_pi_trig", rodrigues(ax3, np.pi / 2))
    for d in DELTAS:
        add(f"half_pi_pm_{d:g}", np.concatenate([rodrigues(ax3, np.pi / 2 + d), rodrigues(ax3, np.pi / 2 - d)]))
    # random axes within 1e-5 of pi: the fraction whose w changes sign between float32 and float64 is ~2.5e-4 per row,
    # so the family is wide enough to meet f32/f64 sign disagreements of w, and the sign-invariant checks must hold there
    add("near_pi_random", rodrigues(_random_axes(rng, 512), np.pi + rng.uniform(-1e-5, 1e-5, 512)))
    # small angles across the series switch of rotvec_roundtrip (1e-3) and far below float32 resolution
    ang = np.concatenate([np.logspace(-9, -2, 22), 1e-3 * np.array([1 - 1e-6, 1 + 1e-6])])
    add("small_angle", rodrigues(_random_axes(rng, len(ang)), ang))
    add("small_angle_axes", np.concatenate([rodrigues(ax3[:3], a) for a in (1e-9, 1e-7, 1e-5, 1e-3)]))
    # float32 products of 2..6 rotations: not exactly orthonormal
    prods = []
    for i in range(96):
        P = quat_to_rot64(rng.normal(size=(1, 4))).astype(np.float32)
        for _ in range(1 + i % 5):
            P = _matmul3_f32(P, quat_to_rot64(rng.normal(size=(1, 4))))
        prods.append(P[0])
    prods = np.stack(prods)
    add("f32_products", prods.astype(np.float64), prods)
    # uniformly scaled rotations R (1 +- 1e-6)
    base = quat_to_rot64(rng.normal(size=(64, 4)))
    base = np.concatenate([base, rodrigues(ax[:3], np.pi), np.stack(half)])
    add("scaled_up", base * (1 + 1e-6))
    add("scaled_down", base * (1 - 1e-6))
    add("random", quat_to_rot64(rng.normal(size=(n_random, 4))))
    return fams


def quaternion_families(seed=1):
    """[(label, q64 (n,4), q32 (n,4))], real first: unit / non-unit (1e-4 .. 1e3) / w < 0 / w = +-0."""
    rng = np.random.default_rng(seed)
    fams = []

    def add(label, q64):
        q64 = np.asarray(q64, np.float64).reshape(-1, 4)
        q32 = q64.astype(np.float32)
        fams.append((label, q32.astype(np.float64), q32))

    u = rng.normal(size=(256, 4))
    u /= np.linalg.norm(u, axis=1, keepdims=True)
    add("unit", u)
    add("unit_axes", np.array([[1, 0, 0, 0], [0, 1, 0, 0], [0, 0, 1, 0], [0, 0, 0, 1], [-1, 0, 0, 0], [0, 0, 0, -1]], np.float64))
    norms = np.logspace(-4, 3, 64)
    add("non_unit", u[:64] * norms[:, None])
    neg = u[:64].copy()
    neg[:, 0] = -np.abs(neg[:, 0])
    add("w_negative", neg)
    wz = u[:32].copy()
    wz[:, 0] = 0.0
    wz[:, 1:] /= np.linalg.norm(wz[:, 1:], axis=1, keepdims=True)
    add("w_plus_zero", wz)
    wn = wz.copy()
    wn[:, 0] = -0.0
    add("w_minus_zero", wn)
    return fams


SMALL_REAL_NORMS = (0.0, 1e-6, 1e-5, 1e-4, 3e-4, 3.4e-4, 3.5e-4, 4e-4, 1e-3)   # sqrt(FLT_EPSILON) = 3.45e-4


def dualquat_families(seed=2):
    """[(label, d64 (n,8), d32 (n,8))]: unit real parts with consistent duals, non-unit real parts with free duals,
    real parts whose norm straddles sqrt(FLT_EPSILON) (the DQ_INV clamp of |real|^2 at FLT_EPSILON)."""
    rng = np.random.default_rng(seed)
    fams = []

    def add(label, d64):
        d32 = np.asarray(d64, np.float64).reshape(-1, 8).astype(np.float32)
        fams.append((label, d32.astype(np.float64), d32))

    for label, q64, _ in quaternion_families(seed + 10):
        t = rng.uniform(-1, 1, size=(len(q64), 3))
        if label.startswith("non_unit"):
            dual = rng.normal(size=(len(q64), 4)) * np.linalg.norm(q64, axis=1, keepdims=True)
        else:
            dual = 0.5 * quat_mul(np.concatenate([np.zeros((len(q64), 1)), t], 1), q64, np.float64)
        add(label, np.concatenate([q64, dual], 1))
    u = rng.normal(size=(len(SMALL_REAL_NORMS) * 4, 4))
    u /= np.linalg.norm(u, axis=1, keepdims=True)
    s = np.repeat(np.array(SMALL_REAL_NORMS), 4)
    add("small_real", np.concatenate([u * s[:, None], rng.normal(size=(len(u), 4))], 1))
    return fams


def rpy_families():
    """[(label, e (n,3) fp64)]: pitch at +-(pi/2 - delta), delta in {1e-3, 1e-2}, and at the exact gimbal lock."""
    out = []
    for d in (1e-3, 1e-2):
        for sgn in (1.0, -1.0):
            out.append((f"pitch_{'+' if sgn > 0 else '-'}{d:g}",
                        np.array([[0.3, sgn * (np.pi / 2 - d), -0.7], [-2.0, sgn * (np.pi / 2 - d), 1.1],
                                  [0.0, sgn * (np.pi / 2 - d), 0.0]])))
    out.append(("gimbal_lock", np.array([[0.3, np.pi / 2, -0.7], [0.5, -np.pi / 2, 0.2]])))
    return out


def stack(fams):
    """Concatenate families: (labels per row, arrays...)."""
    labels = np.concatenate([[f[0]] * len(f[1]) for f in fams])
    return (labels,) + tuple(np.concatenate([f[i] for f in fams]) for i in range(1, len(fams[0])))


def poses(R, t):
    """(n,3,3) rotations, (n,3) translations -> (n,4,4) in R's dtype."""
    M = np.zeros((len(R), 4, 4), R.dtype)
    M[:, :3, :3], M[:, :3, 3], M[:, 3, 3] = R, t, 1
    return M


def resize_rows(a, n, shift=0):
    """n rows of `a` taken cyclically from row `shift` (so the edge rows also land in a launch's tail block)."""
    return a[(np.arange(n) + shift) % len(a)]


# ------------------------------------------------------------------------------------------ restatements
def _cols(a, dt):
    a = np.asarray(a).astype(dt, copy=False)
    return [a[..., i] for i in range(a.shape[-1])]


def quat_mul(a, b, dt):
    """creg_dev.h quat_mul: Hamilton product, real first, left-to-right sums."""
    a0, a1, a2, a3 = _cols(a, dt)
    b0, b1, b2, b3 = _cols(b, dt)
    return np.stack([((a0 * b0 - a1 * b1) - a2 * b2) - a3 * b3,
                     ((a0 * b1 + a1 * b0) + a2 * b3) - a3 * b2,
                     ((a0 * b2 - a1 * b3) + a2 * b0) + a3 * b1,
                     ((a0 * b3 + a1 * b2) - a2 * b1) + a3 * b0], -1)


def _sqrt_pos(v, dt):
    return np.where(v > dt(0), np.sqrt(np.maximum(v, dt(0))), dt(0)).astype(dt)


def matrix_to_quat_parts(R, dt):
    """-> (q (n,4), qa (n,4), chosen candidate (n,), den (n,), cand[0] / den before the flip (n,))."""
    R = np.asarray(R).astype(dt, copy=False).reshape(-1, 9)
    m00, m01, m02, m10, m11, m12, m20, m21, m22 = (R[:, i] for i in range(9))
    one = dt(1)
    qa = np.stack([_sqrt_pos(((one + m00) + m11) + m22, dt), _sqrt_pos(((one + m00) - m11) - m22, dt),
                   _sqrt_pos(((one - m00) + m11) - m22, dt), _sqrt_pos(((one - m00) - m11) + m22, dt)], 1)
    c = np.zeros(len(R), np.int64)
    for i in range(1, 4):                                  # `if (qa[i] > qa[c]) c = i`: the first maximum wins
        c = np.where(qa[:, i] > qa[np.arange(len(R)), c], i, c)
    cands = np.stack([
        np.stack([qa[:, 0] * qa[:, 0], m21 - m12, m02 - m20, m10 - m01], 1),
        np.stack([m21 - m12, qa[:, 1] * qa[:, 1], m10 + m01, m02 + m20], 1),
        np.stack([m02 - m20, m10 + m01, qa[:, 2] * qa[:, 2], m12 + m21], 1),
        np.stack([m10 - m01, m20 + m02, m21 + m12, qa[:, 3] * qa[:, 3]], 1)], 1)
    cand = cands[np.arange(len(R)), c]
    qc = qa[np.arange(len(R)), c]
    floor = dt(0.1)
    den = dt(2) * np.where(qc > floor, qc, floor)
    v = cand / den[:, None]
    neg = v[:, 0] < dt(0)
    q = np.where(neg[:, None], -v, v)
    return q, qa, c, den, v[:, 0]


def matrix_to_quat(R, dt):
    return matrix_to_quat_parts(R, dt)[0]


def quat_to_matrix(q, dt):
    w, x, y, z = _cols(q, dt)
    with np.errstate(divide="ignore"):                      # q = 0 (a zero real part): inf, then NaN entries, as on the device
        s = dt(2) / (((w * w + x * x) + y * y) + z * z)
    one = dt(1)
    with np.errstate(invalid="ignore"):
        return np.stack([one - s * (y * y + z * z), s * (x * y - z * w), s * (x * z + y * w),
                         s * (x * y + z * w), one - s * (x * x + z * z), s * (y * z - x * w),
                         s * (x * z - y * w), s * (y * z + x * w), one - s * (x * x + y * y)], -1).reshape(-1, 3, 3)


def se3_to_dq(M, dt, eps=FLT_EPSILON):
    M = np.asarray(M).astype(dt, copy=False)
    q = matrix_to_quat(M[:, :3, :3], dt)
    n = np.sqrt(((q[:, 0] * q[:, 0] + q[:, 1] * q[:, 1]) + q[:, 2] * q[:, 2]) + q[:, 3] * q[:, 3])
    e = dt(eps)
    n = np.where(n > e, n, e)
    real = q / n[:, None]
    p = np.concatenate([np.zeros((len(M), 1), dt), M[:, :3, 3]], 1)
    return np.concatenate([real, dt(0.5) * quat_mul(p, real, dt)], 1)


def _conj(q):
    return np.stack([q[:, 0], -q[:, 1], -q[:, 2], -q[:, 3]], 1)


def dq_to_se3(d, dt):
    d = np.asarray(d).astype(dt, copy=False)
    R = quat_to_matrix(d[:, :4], dt)
    o = quat_mul(d[:, 4:], _conj(d[:, :4]), dt)
    M = np.zeros((len(d), 4, 4), dt)
    M[:, :3, :3], M[:, :3, 3], M[:, 3, 3] = R, dt(2) * o[:, 1:], 1
    return M


def dq_multiply(a, b, dt):
    a, b = np.asarray(a).astype(dt, copy=False), np.asarray(b).astype(dt, copy=False)
    return np.concatenate([quat_mul(a[:, :4], b[:, :4], dt),
                           quat_mul(a[:, :4], b[:, 4:], dt) + quat_mul(a[:, 4:], b[:, :4], dt)], 1)


def dq_invert(d, dt, eps=FLT_EPSILON):
    """se3.hip DQ_INV: conj(real) / n2 ; conj(dual) / n2 - 2 conj(real) <real, dual> / n2^2, n2 = max(|real|^2, eps)."""
    x = np.asarray(d).astype(dt, copy=False)
    nrm = np.sqrt(((x[:, 0] * x[:, 0] + x[:, 1] * x[:, 1]) + x[:, 2] * x[:, 2]) + x[:, 3] * x[:, 3])
    n2 = nrm * nrm
    e = dt(eps)
    n2 = np.where(n2 > e, n2, e)
    dot = (((x[:, 0] * x[:, 4] + x[:, 1] * x[:, 5]) + x[:, 2] * x[:, 6]) + x[:, 3] * x[:, 7]) / (n2 * n2)
    out = np.empty_like(x)
    for i in range(4):
        sg = dt(1) if i == 0 else dt(-1)
        out[:, i] = (sg * x[:, i]) / n2
        out[:, 4 + i] = (sg * x[:, 4 + i]) / n2 - (dt(2) * (sg * x[:, i])) * dot
    return out


def dq_to_quat_trans(d, dt):
    """se3.hip DQ_TO_QT: q = real (x) dual (the reference's quirk), t = 2 (dual (x) conj(real))[1:]."""
    d = np.asarray(d).astype(dt, copy=False)
    q = quat_mul(d[:, :4], d[:, 4:], dt)
    tt = quat_mul(d[:, 4:], _conj(d[:, :4]), dt)
    return q, dt(2) * tt[:, 1:]


def quat_trans_to_dq(q, t, dt):
    q, t = np.asarray(q).astype(dt, copy=False), np.asarray(t).astype(dt, copy=False)
    p = np.concatenate([np.zeros((len(q), 1), dt), t], 1)
    return np.concatenate([q, dt(0.5) * quat_mul(p, q, dt)], 1)


def rotmat_to_unitquat_xyzw(m):
    """coord_map.hip rotmat_to_unitquat_xyzw (fp64) -> (q xyzw (n,4), decision index (n,): 0..2 = diagonal, 3 = trace)."""
    m = np.asarray(m, np.float64).reshape(-1, 9)
    tr = (m[:, 0] + m[:, 4]) + m[:, 8]
    dec = np.stack([m[:, 0], m[:, 4], m[:, 8], tr], 1)
    c = np.zeros(len(m), np.int64)
    for i in range(1, 4):
        c = np.where(dec[:, i] > dec[np.arange(len(m)), c], i, c)
    q = np.empty((len(m), 4))
    for r in range(len(m)):
        a = m[r]
        if c[r] == 3:
            q[r] = (a[7] - a[5], a[2] - a[6], a[3] - a[1], 1 + tr[r])
        elif c[r] == 0:
            q[r] = (1 - tr[r] + 2 * a[0], a[3] + a[1], a[6] + a[2], a[7] - a[5])
        elif c[r] == 1:
            q[r] = (a[1] + a[3], 1 - tr[r] + 2 * a[4], a[7] + a[5], a[2] - a[6])
        else:
            q[r] = (a[2] + a[6], a[5] + a[7], 1 - tr[r] + 2 * a[8], a[3] - a[1])
    n = np.sqrt(((q[:, 0] * q[:, 0] + q[:, 1] * q[:, 1]) + q[:, 2] * q[:, 2]) + q[:, 3] * q[:, 3])
    return q / n[:, None], c


def rotvec_branches(q):
    """The decisions rotvec_roundtrip takes on xyzw unit quaternions: (flipped, angle series, norm series)."""
    q = np.asarray(q, np.float64)
    flip = q[:, 3] < 0
    q = np.where(flip[:, None], -q, q)
    half = np.arctan2(np.sqrt((q[:, 0] * q[:, 0] + q[:, 1] * q[:, 1]) + q[:, 2] * q[:, 2]), q[:, 3])
    angle = 2 * half
    a_series = np.abs(angle) <= 1e-3
    a2 = angle * angle
    with np.errstate(divide="ignore", invalid="ignore"):
        scale = np.where(a_series, 2 + a2 / 12 + 7 * (a2 * a2) / 2880, angle / np.sin(half))
    v = scale[:, None] * q[:, :3]
    nv = np.sqrt((v[:, 0] * v[:, 0] + v[:, 1] * v[:, 1]) + v[:, 2] * v[:, 2])
    return flip, a_series, nv <= 1e-3


# ------------------------------------------------------------------------------------------ pose tracks for coord_dist_map
# step rotations (angle, axis) aimed at rotvec_roundtrip's decisions: no step, 1e-6, both sides of the 1e-3 series switch,
# pi - 1e-6, exactly pi and pi + 1e-6 (the shortest-arc flip q[3] < 0: a turn past pi, or pi about a negated axis)
TRACK_STEPS = (("zero", 0.0, (1, 0, 0)), ("1e-6", 1e-6, (0.3, -0.2, 0.9)), ("1e-3-1e-9", 1e-3 - 1e-9, (1, 2, 3)),
               ("1e-3+1e-9", 1e-3 + 1e-9, (1, 2, 3)), ("pi-1e-6", np.pi - 1e-6, (0, 1, 0)), ("pi", np.pi, (0, 0, 1)),
               ("pi_neg_axis", np.pi - 1e-6, (-1, -1, 0)), ("pi+1e-6", np.pi + 1e-6, (1, 0, 1)), ("pi_diag", np.pi, (1, 1, 1)))


def coord_tracks(T, K, seed=0):
    """(T,K,4,4) fp64 pose tracks.  Track k turns by step TRACK_STEPS[k % 9] in its body frame every step, so
    R_i^T R_{i+1} is that step up to rounding.  Track k + 1 (k % 3 == 0) repeats track k (relative rotation I between
    them, acos(1)), track k + 2 is track k turned by pi (acos at the clamp -1).  Returns (M, step label per track)."""
    rng = np.random.default_rng(seed)
    M = np.tile(np.eye(4), (T, K, 1, 1))
    labels = []
    R0 = quat_to_rot64(rng.normal(size=(K, 4)))
    t0 = rng.uniform(-0.5, 0.5, size=(K, 3))
    flip = rodrigues(np.array([[0.0, 0.0, 1.0]]), np.pi)[0]
    for k in range(K):
        name, ang, axis = TRACK_STEPS[k % len(TRACK_STEPS)]
        S = rodrigues(np.array([axis], np.float64), ang)[0]
        R, t = R0[k].copy(), t0[k].copy()
        if k % 3 == 1:
            R, t = M[0, k - 1, :3, :3].copy(), t0[k - 1].copy()
        elif k % 3 == 2:
            R = M[0, k - 2, :3, :3] @ flip
        for i in range(T):
            M[i, k, :3, :3], M[i, k, :3, 3] = R, t
            R = R @ S
            t = t + rng.normal(scale=0.01, size=3)
        labels.append(name)
    return M, labels
