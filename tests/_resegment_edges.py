"""Input builders and plain references for the hand-off between training and ICP (test infrastructure): the stable grouping
by label with its change of frame (csrc/group.hip), the 4x4 inverse inside it (`inv4x4`) and the three copies of the box
mask (`k_icp_mask` ascending and binned in csrc/icp_large.hip, step 1 of `k_masked_icp` in csrc/icp_small.hip).

Everything here is numpy / fractions and importable without a GPU.  Nothing is measured from a kernel:

* grouping is compared bit for bit.  The exact inputs (integer points that encode their own index, signed permutation poses with
  integer translations) make every product and sum of `fma(I2,p2,fma(I1,p1,I0*p0)) + I3` exact, so integer arithmetic is the
  reference; for random doubles the expression is restated with a correctly rounded fma built on `fractions.Fraction`
  (the library is built with -ffp-contract=off: the one product outside the fma rounds on its own);
* the in-kernel inverse is compared with the exact rational inverse (Fraction Gauss-Jordan on the doubles, rounded once) within
  `inverse_tolerance`, a forward bound that is derived in its docstring; `emulate_inv4x4` restates the kernel's elimination
  in float64 without fma so that tests/test_resegment_edges_cpu.py can show what a correct implementation needs of it;
* boxes are restated in float32 one operation at a time, membership is oracle.icp.aabb_mask.
"""
import itertools
from fractions import Fraction

import numpy as np

EPS = 2.0 ** -52
GROUP_SMALL_MAX = 16384                      # creg_group_to_local_f64: n above this takes the count / scan / workgroup-per-cluster form
GROUP_ROUND = 4096                           # points per round of k_group_scatter_big (1024 threads x 4 consecutive points)


# ================================================================================================ A. grouping
def proper_signed_permutations():
    """The 24 signed 3x3 permutation matrices of determinant +1 (int64), in a fixed order."""
    out = []
    for perm in itertools.permutations(range(3)):
        for signs in itertools.product((1, -1), repeat=3):
            R = np.zeros((3, 3), np.int64)
            for r in range(3):
                R[r, perm[r]] = signs[r]
            if round(np.linalg.det(R)) == 1:
                out.append(R)
    assert len(out) == 24
    return out


def exact_points(n, start=0):
    """(n,3) float64 integer points that encode their own index: X[i] = (i, i % 7, -i) (shifted by `start`), n + start < 2^24."""
    assert n + start < 1 << 24
    i = np.arange(start, start + n, dtype=np.int64)
    return np.stack([i, i % 7, -i], 1).astype(np.float64)


def exact_poses(k, shift=0):
    """k poses M (k,4,4) float64 and their inverses I: signed permutations (cycling through the 24 proper ones) with small
    integer translations.  inv(M) = [R^T | -R^T t] is integer too."""
    perms = proper_signed_permutations()
    M, I = np.zeros((k, 4, 4), np.int64), np.zeros((k, 4, 4), np.int64)
    for j in range(k):
        R = perms[(j + shift) % 24]
        t = np.array([(j + shift) % 11 - 5, 3 * ((j + shift) % 5), -((j + 2 * shift) % 13)], np.int64)
        M[j, :3, :3], M[j, :3, 3], M[j, 3, 3] = R, t, 1
        I[j, :3, :3], I[j, :3, 3], I[j, 3, 3] = R.T, -(R.T @ t), 1
        assert (M[j] @ I[j] == np.eye(4, dtype=np.int64)).all()
    return M.astype(np.float64), I.astype(np.float64)


def group_offsets(lab, k):
    return np.concatenate([[0], np.cumsum(np.bincount(lab, minlength=k))]).astype(np.int32)


def group_reference_exact(X, lab, k, I):
    """Offsets and rows of the stable partition for EXACT inputs: inv(M_label) p in int64 (no rounding anywhere), as float64."""
    order = np.argsort(lab, kind="stable")
    Xi, Ii = X[order].astype(np.int64), I.astype(np.int64)
    assert (Xi == X[order]).all() and (Ii == I).all()
    L = lab[order]
    out = np.einsum("nac,nc->na", Ii[L, :3, :3], Xi) + Ii[L, :3, 3]
    assert np.abs(out).max() < 1 << 53
    return out.astype(np.float64), group_offsets(lab, k)


def fma_exact(a, b, c):
    """Correctly rounded a * b + c of three doubles (int / int true division rounds correctly)."""
    return float(Fraction(a) * Fraction(b) + Fraction(c))


def apply_pose_fma(I, p):
    """`fma(I2, p2, fma(I1, p1, I0 * p0)) + I3` per axis, the kernels' expression, with a correctly rounded fma."""
    return [fma_exact(I[a][2], p[2], fma_exact(I[a][1], p[1], float(I[a][0]) * float(p[0]))) + float(I[a][3]) for a in range(3)]


def group_reference_fma(X, lab, k, I):
    """Offsets and rows of the stable partition for arbitrary doubles, inverse poses `I` given (m_is_inverse=True)."""
    order = np.argsort(lab, kind="stable")
    Il = I.tolist()
    out = np.array([apply_pose_fma(Il[j], p) for j, p in zip(lab[order].tolist(), X[order].tolist())], np.float64).reshape(-1, 3)
    return out, group_offsets(lab, k)


def random_rigid(rng, k, t_scale=1.0):
    """k random rigid poses (k,4,4) float64 (QR of a normal matrix, determinant fixed to +1)."""
    M = np.zeros((k, 4, 4))
    for j in range(k):
        Q, R = np.linalg.qr(rng.normal(size=(3, 3)))
        Q = Q * np.sign(np.diag(R))
        if np.linalg.det(Q) < 0:
            Q[:, 0] = -Q[:, 0]
        M[j, :3, :3], M[j, :3, 3], M[j, 3, 3] = Q, t_scale * rng.normal(size=3), 1.0
    return M


def spread_labels(n, k, seed, cover=True):
    """Random labels in [0, k) -- with `cover` every label present at least once when n >= k, else as they fall (empty clusters)."""
    rng = np.random.default_rng(seed)
    lab = rng.integers(0, k, size=n)
    if cover and n >= k:
        lab[rng.permutation(n)[:k]] = np.arange(k)
    return lab.astype(np.int32)


def large_n_labels(n, last_carries, seed=5):
    """k = 5 labels for the large form (n > 16384).
    Label 1: ALL members in the last round of 4096 (the partial one unless n is a multiple of 4096); label 3: its only members
    are one thread's four consecutive points (thread 517 of round 1); labels 0, 2, 4 share the rest, label 2 from index 0 on.
    last_carries: the last point n - 1 has label 1 (the lanes past the end re-read it), else label 0."""
    assert n > GROUP_SMALL_MAX
    rng = np.random.default_rng(seed)
    lab = rng.choice(np.array([0, 2, 4]), size=n)
    lab[0] = 2
    r0 = (n - 1) // GROUP_ROUND * GROUP_ROUND
    tail = np.arange(r0, n)
    lab[tail[rng.random(len(tail)) < 0.5]] = 1
    lab[r0] = 1
    lab[n - 1] = 1 if last_carries else 0                  # (a last round of ONE point: label 1 is then empty without it)
    q0 = GROUP_ROUND + 4 * 517
    lab[q0:q0 + 4] = 3
    lab = lab.astype(np.int32)
    assert (np.nonzero(lab == 1)[0] >= r0).all() and ((lab == 1).any() or (n - r0 == 1 and not last_carries)) and list(np.nonzero(lab == 3)[0]) == [q0, q0 + 1, q0 + 2, q0 + 3]
    return lab


def large_k_labels(n, k, pattern, seed=9):
    """Label vectors for the k sweep of the large form: "first" (only label 0), "last" (only label k - 1), "spread" (all labels),
    "gap" (all labels but a run of empty clusters in the middle: several hundred of them for k >= 1024, a third of k otherwise)."""
    if pattern == "first":
        return np.zeros(n, np.int32)
    if pattern == "last":
        return np.full(n, k - 1, np.int32)
    lab = spread_labels(n, k, seed)
    if pattern == "gap" and k >= 3:
        a, b = k // 3, k // 3 + max(1, min(k // 3, 700))
        hole = (lab >= a) & (lab < b)
        lab[hole] = (lab[hole] % a) if a > 0 else b
    return lab.astype(np.int32)


# ================================================================================================ B. the in-kernel inverse
def exact_inverse(M):
    """inv(M) of one 4x4 of doubles by Gauss-Jordan in rationals; returns the Fractions (4x4 list)."""
    a = [[Fraction(float(M[r][c])) for c in range(4)] + [Fraction(int(r == c)) for c in range(4)] for r in range(4)]
    for c in range(4):
        p = next(r for r in range(c, 4) if a[r][c] != 0)
        a[c], a[p] = a[p], a[c]
        inv = 1 / a[c][c]
        a[c] = [v * inv for v in a[c]]
        for r in range(4):
            if r != c and a[r][c] != 0:
                f = a[r][c]
                a[r] = [v - f * w for v, w in zip(a[r], a[c])]
    return [row[4:] for row in a]


def exact_inverses(M):
    """(k,4,4) doubles -> (inverse rounded once to float64 (k,4,4), kappa (k,) = ||M||_inf ||inv(M)||_inf from the exact inverse)."""
    I, kap = np.empty_like(M), np.empty(len(M))
    for j, m in enumerate(M):
        F = exact_inverse(m)
        I[j] = [[float(v) for v in row] for row in F]
        kap[j] = np.abs(m).sum(1).max() * float(max(sum(abs(v) for v in row) for row in F))
    return I, kap


def emulate_inv4x4(M, pivot=True, log=None):
    """The elimination of `inv4x4` (csrc/group.hip) in numpy float64, one rounding per operation (no fma): first row of the largest
    |entry| in column c among rows c .. 3, exchange, scale the pivot row by 1 / pivot, eliminate the column from every other row.
    log: list that receives (column, pivot row, |a[c][c]| before the exchange) per column.  pivot=False: the mutant without search."""
    a = np.concatenate([np.asarray(M, np.float64).reshape(4, 4), np.eye(4)], 1)
    for c in range(4):
        p = c
        if pivot:
            best = abs(a[c, c])
            for r in range(c + 1, 4):
                if abs(a[r, c]) > best:
                    best, p = abs(a[r, c]), r
        if log is not None:
            log.append((c, p, abs(a[c, c])))
        if p != c:
            a[[c, p]] = a[[p, c]]
        with np.errstate(divide="ignore", invalid="ignore"):
            a[c] = a[c] * (np.float64(1.0) / a[c, c])
            for r in range(4):
                if r != c:
                    a[r] = a[r] - a[r, c] * a[c]
    return a[:, 4:].copy()


def perm_poses():
    """Exact poses that force row exchanges: (M, I) float64, both integer.
    * The 24 proper signed 3x3 permutations with integer translations.  Their last row is (0, 0, 0, 1), so they exchange rows at
      columns 0 and 1 only (row 3 never offers a pivot candidate before column 3).
    * The 18 signed 4x4 permutation matrices whose last row is NOT (0, 0, 0, 1): no pose, but `inv4x4` inverts the full 4x4 and
      rows 0..2 of the inverse are applied to (p, 1) all the same.  They exchange with row 3, at column 2 too."""
    M, I = exact_poses(24)
    M4 = []
    for n, perm in enumerate(p for p in itertools.permutations(range(4)) if p[3] != 3):
        A = np.zeros((4, 4))
        for r in range(4):
            A[r, perm[r]] = -1.0 if (n + r) % 3 == 0 else 1.0
        M4.append(A)
    M4 = np.stack(M4)
    I4 = np.transpose(M4, (0, 2, 1)).copy()
    assert len(M4) == 18 and (np.einsum("kab,kbc->kac", M4, I4) == np.eye(4)).all()
    return np.concatenate([M, M4]), np.concatenate([I, I4])


def tie_poses():
    """Rotations by 45 degrees about x, y, z with cos = sin = sqrt(0.5) to the bit (the pivot candidates tie), translations of order 10."""
    s = np.sqrt(0.5)
    M = np.stack([np.eye(4)] * 3)
    for ax in range(3):
        u, v = (ax + 1) % 3, (ax + 2) % 3
        M[ax, u, u], M[ax, u, v], M[ax, v, u], M[ax, v, v] = s, -s, s, s
        M[ax, :3, 3] = [10.0 + ax, -7.5, 3.25 * (ax + 1)]
    return M


def trained_poses(seed=41, count=200):
    """Random rotations rounded to float32 and cast back (what a trained pose is), translations of order 100."""
    rng = np.random.default_rng(seed)
    M = random_rigid(rng, count, t_scale=100.0)
    return M.astype(np.float32).astype(np.float64)


def affine_poses(seed=43):
    """U diag(1, c^-1/2, c^-1) V^T for c in {1e2, 1e4, 1e6, 1e8}, M[3,3] in {1, 2}, translations of order 1: 8 poses."""
    rng = np.random.default_rng(seed)
    out = []
    for c in (1e2, 1e4, 1e6, 1e8):
        for w in (1.0, 2.0):
            U, V = random_rigid(rng, 2)[:, :3, :3]
            M = np.eye(4)
            M[:3, :3] = U @ np.diag([1.0, c ** -0.5, 1.0 / c]) @ V.T
            M[:3, 3] = rng.normal(size=3)
            M[3, 3] = w
            out.append(M)
    return np.stack(out)


def tolerance_poses():
    """The families compared within `inverse_tolerance`: ties, trained, affine -- (k,4,4) and the family name of every pose."""
    fams = [("tie", tie_poses()), ("trained", trained_poses()), ("affine", affine_poses())]
    return np.concatenate([m for _, m in fams]), [nm for nm, m in fams for _ in m]


def points_for_poses(M, n, seed):
    """n world points and labels for the poses M: cluster j's points are M_j applied to order-one local points (so inv(M_j) p
    cancels the translation, as in the workload), labels random with every cluster present."""
    rng = np.random.default_rng(seed)
    k = len(M)
    lab = spread_labels(n, k, seed + 1)
    q = rng.normal(size=(n, 3))
    A = M[lab]
    X = np.einsum("nac,nc->na", A[:, :3, :3], q) + A[:, :3, 3]
    return X, lab


def inverse_reference(X, lab, k, I):
    """The exact inverses applied to the points in extended precision, rounded to float64, in group order."""
    order = np.argsort(lab, kind="stable")
    L = lab[order]
    Il = I.astype(np.longdouble)
    out = np.einsum("nac,nc->na", Il[L, :3, :3], X[order].astype(np.longdouble)) + Il[L, :3, 3]
    return out.astype(np.float64), group_offsets(lab, k)


def inverse_tolerance(X, lab, I, kappa):
    """Per output entry, in group order:  eps (8 kappa_j + 8) sum_c |I_j[a,c]| |(p_i, 1)[c]|,  eps = 2^-52.
    First term: the textbook forward bound of a backward-stable elimination of order 4 (|dI| <= c n eps kappa |I|, c n = 8);
    second: the four roundings of the product (one multiplication, two fma, one addition: at most 2 eps of the same sum) and
    the reference's own rounding to float64, with margin."""
    order = np.argsort(lab, kind="stable")
    L = lab[order]
    S = np.einsum("nac,nc->na", np.abs(I[L, :3, :3]), np.abs(X[order])) + np.abs(I[L, :3, 3])
    return EPS * (8.0 * kappa[L][:, None] + 8.0) * S


# ================================================================================================ C. the box mask
def restated_boxes(world, woff, scale):
    """(k,6) float32 boxes exactly as numpy evaluates them on the float32 clusters, one float32 operation at a time:
    ctr = (lo + hi) / 2, sz = hi - lo, ctr -/+ float32(0.5 * scale) * sz.  Empty clusters give NaN rows."""
    world = np.asarray(world, np.float32)
    k = len(woff) - 1
    box = np.full((k, 6), np.nan, np.float32)
    hs = np.float32(0.5 * scale)
    for c in range(k):
        w = world[woff[c]:woff[c + 1]]
        if len(w) == 0:
            continue
        lo, hi = w.min(0), w.max(0)
        ctr, sz = (lo + hi) / np.float32(2), hi - lo
        assert ctr.dtype == np.float32 and sz.dtype == np.float32
        box[c, :3], box[c, 3:] = ctr - hs * sz, ctr + hs * sz
    return box


def double_boxes(world, woff, scale):
    """The same boxes evaluated in float64 from the float32 points (what a kernel that widened too early would use)."""
    world = np.asarray(world, np.float32).astype(np.float64)
    box = np.full((len(woff) - 1, 6), np.nan)
    for c in range(len(woff) - 1):
        w = world[woff[c]:woff[c + 1]]
        if len(w):
            lo, hi = w.min(0), w.max(0)
            ctr, sz = (lo + hi) / 2.0, hi - lo
            box[c, :3], box[c, 3:] = ctr - 0.5 * scale * sz, ctr + 0.5 * scale * sz
    return box


def fused_boxes(world, woff, scale):
    """The float32 boxes with `ctr -/+ hs * sz` contracted into one fused multiply-add (exact product, one rounding)."""
    world = np.asarray(world, np.float32)
    box = np.full((len(woff) - 1, 6), np.nan, np.float32)
    hs = float(np.float32(0.5 * scale))
    for c in range(len(woff) - 1):
        w = world[woff[c]:woff[c + 1]]
        if len(w):
            lo, hi = w.min(0), w.max(0)
            ctr, sz = (lo + hi) / np.float32(2), hi - lo
            for d in range(3):
                prod = Fraction(hs) * Fraction(float(sz[d]))
                box[c, d] = _round_f32(Fraction(float(ctr[d])) - prod)
                box[c, 3 + d] = _round_f32(Fraction(float(ctr[d])) + prod)
    return box


def _round_f32(fr):
    """A rational rounded once to float32: the nearest of the double rounding's float32 and its two neighbours."""
    f = np.float32(float(fr))
    lo, hi = np.nextafter(f, np.float32(-np.inf)), np.nextafter(f, np.float32(np.inf))
    best = min((f, lo, hi), key=lambda v: abs(Fraction(float(v)) - fr))
    return best


def inside(box, pts):
    """Strict membership of float64 points in one (6,) box (any float dtype; compared in float64)."""
    b = np.asarray(box, np.float64)
    return np.all((pts > b[:3]) & (pts < b[3:]), axis=1)


def mask_reference(world, woff, frame, scale):
    """Per cluster the ascending frame indices strictly inside its box: oracle.icp.aabb_mask on the float32 cluster; an empty
    cluster lists nothing."""
    from oracle import icp as oicp
    world = np.asarray(world, np.float32)
    out = []
    for c in range(len(woff) - 1):
        w = world[woff[c]:woff[c + 1]]
        out.append(np.nonzero(oicp.aabb_mask(w, frame, scale))[0] if len(w) else np.zeros(0, np.int64))
    return out


def blob_clusters(k, seed, pts=40, centre=(0.0, 0.0, 0.0), spread=3.0):
    """k float32 blobs of `pts` points each, centres within `spread` of `centre`: (world (k*pts,3) f32, woff (k+1) i32)."""
    rng = np.random.default_rng(seed)
    ctr = np.asarray(centre) + rng.uniform(-spread, spread, size=(k, 3))
    w = (ctr[:, None, :] + rng.normal(scale=[0.4, 0.25, 0.1], size=(k, pts, 3))).astype(np.float32).reshape(-1, 3)
    return w, (np.arange(k + 1) * pts).astype(np.int32)


def frame_over_boxes(box, nf, seed):
    """nf random float64 points over about twice the union of the boxes (so counts are neither 0 nor nf)."""
    rng = np.random.default_rng(seed)
    b = np.asarray(box, np.float64)
    b = b[np.isfinite(b).all(1)]
    lo, hi = b[:, :3].min(0), b[:, 3:].max(0)
    c, h = (lo + hi) / 2, (hi - lo) / 2
    return rng.uniform(c - 1.26 * h, c + 1.26 * h, size=(nf, 3))            # 1.26^3 = 2.0 times the volume


def face_points(box):
    """For every finite box: per face three points (other two coordinates at the box centre, face coordinate exactly on the
    bound / one double inside / one double outside) and the eight exact corners.
    Returns (frame (m,3) f64, owner (m,) cluster, kind (m,) in {"on", "in", "out", "corner"})."""
    pts, owner, kind = [], [], []
    for c, b in enumerate(np.asarray(box, np.float64)):
        if not np.isfinite(b).all():
            continue
        mid = 0.5 * (b[:3] + b[3:])
        for d in range(3):
            for side in (0, 1):
                bound = b[3 * side + d]
                inward = mid[d]
                for nm, v in (("on", bound), ("in", np.nextafter(bound, inward)), ("out", np.nextafter(bound, 2 * bound - inward))):
                    p = mid.copy()
                    p[d] = v
                    pts.append(p); owner.append(c); kind.append(nm)
        for corner in itertools.product((0, 1), repeat=3):
            pts.append(np.array([b[3 * s + d] for d, s in enumerate(corner)])); owner.append(c); kind.append("corner")
    return np.array(pts), np.array(owner), np.array(kind)


def between_float32_neighbours(box, per_face, seed):
    """For every face of every box, `per_face` random doubles strictly between the two float32 neighbours of the bound (other
    coordinates at the box centre): the points a float32 comparison could not tell from the face."""
    rng = np.random.default_rng(seed)
    pts = []
    for b32 in np.asarray(box, np.float32):
        b = b32.astype(np.float64)
        mid = 0.5 * (b[:3] + b[3:])
        for d in range(3):
            for side in (0, 1):
                f = b32[3 * side + d]
                lo, hi = float(np.nextafter(f, np.float32(-np.inf))), float(np.nextafter(f, np.float32(np.inf)))
                for v in rng.uniform(lo, hi, size=per_face):
                    p = mid.copy()
                    p[d] = v
                    pts.append(p)
    return np.array(pts)


# ================================================================================================ D. the mask inside masked_icp
def surface_cluster(rng, n, centre):
    """n float64 points of a gently curved, slightly rough patch about `centre`."""
    xy = rng.uniform(-0.5, 0.5, size=(n, 2))
    z = 0.12 * np.sin(3.0 * xy[:, 0]) + 0.08 * np.cos(2.5 * xy[:, 1]) + 0.01 * rng.normal(size=n)
    return np.c_[xy, z] + np.asarray(centre)


def icp_case(sizes, scale=1.0, seed=3, n_outside=0):
    """One masked-ICP problem whose result depends on the strictness of the mask.

    Clusters: surface patches 3 apart, `local` in their own frames, rigid initial poses M, explicit float32 `world` = float32 of
    M . local -- so the boxes are `restated_boxes(world, off, scale)`.  scale = 1.0 puts the faces on the clusters' extreme points.
    Frame: (a) true targets: the world points moved by a small rigid motion about the cluster centre, those strictly inside the
    box only; (b) decoys: per face the 32 cluster points nearest it with the face coordinate replaced by the exact bound -- they
    sit within half of th = 1 of the sources (most within a few hundredths), and a non-strict face admits them; (c) `n_outside` points one
    double outside a face or well away from every box.
    Returns a dict: local (list), world (list f32), off, M, frame, kind ((nf,) "true" | "decoy" | "outside"), face ((nf,) 0..5 for
    decoys, else -1), owner, box, scale."""
    rng = np.random.default_rng(seed)
    k = len(sizes)
    local, world, Ms = [], [], np.stack([np.eye(4)] * k)
    for j, n in enumerate(sizes):
        centre = np.array([3.0 * j, -1.0 + 0.5 * j, 0.7])
        P = surface_cluster(rng, n, (0, 0, 0))
        # pose: a moderate rotation about z, then the centre
        a = 0.3 + 0.2 * j
        Ms[j, :3, :3] = [[np.cos(a), -np.sin(a), 0], [np.sin(a), np.cos(a), 0], [0, 0, 1]]
        Ms[j, :3, 3] = centre
        local.append(P)
        world.append((P @ Ms[j, :3, :3].T + Ms[j, :3, 3]).astype(np.float32))
    off = np.concatenate([[0], np.cumsum(sizes)]).astype(np.int32)
    box = restated_boxes(np.concatenate(world), off, scale)
    pts, kind, face, owner = [], [], [], []
    for j in range(k):
        w = world[j].astype(np.float64)
        b = box[j].astype(np.float64)
        ctr = 0.5 * (b[:3] + b[3:])
        th = 0.02
        Rm = np.array([[np.cos(th), -np.sin(th), 0], [np.sin(th), np.cos(th), 0], [0, 0, 1]]) @ \
            np.array([[1, 0, 0], [0, np.cos(0.5 * th), -np.sin(0.5 * th)], [0, np.sin(0.5 * th), np.cos(0.5 * th)]])
        sg = np.array([1.0, -1.0, 1.0]) * (1.0 if j % 2 == 0 else -1.0)       # the clusters move in opposite directions: between
        moved = (w - ctr) @ Rm.T + ctr + sg * np.array([0.012, 0.009, 0.006])   # them the motion pushes points across every face
        moved = moved[inside(b, moved)]
        pts.append(moved); kind += ["true"] * len(moved); face += [-1] * len(moved); owner += [j] * len(moved)
        for d in range(3):
            for side in (0, 1):
                bound = b[3 * side + d]
                near = np.argsort(np.abs(w[:, d] - bound), kind="stable")[:32]
                dec = w[near].copy()
                dec[:, d] = bound
                pts.append(dec); kind += ["decoy"] * len(dec); face += [3 * side + d] * len(dec); owner += [j] * len(dec)
        if n_outside:
            m = n_outside // k + (j < n_outside % k)
            out = np.tile(ctr, (m, 1))
            d = rng.integers(0, 3, size=m)
            side = rng.integers(0, 2, size=m)
            bound = b[3 * side + d]
            far = rng.random(m) < 0.5                      # half well away from every box, half one double outside the face
            just = np.nextafter(bound, np.where(side == 1, np.inf, -np.inf))
            away = bound + np.where(side == 1, 1.0, -1.0) * rng.uniform(0.01, 0.3, size=m)
            out[np.arange(m), d] = np.where(far, away, just)
            pts.append(out); kind += ["outside"] * m; face += [-1] * m; owner += [j] * m
    frame = np.concatenate(pts)
    perm = rng.permutation(len(frame))                      # the kinds interleaved: ascending index means nothing
    return dict(local=local, world=world, off=off, M=Ms, frame=frame[perm], kind=np.array(kind)[perm], face=np.array(face)[perm],
                owner=np.array(owner)[perm], box=box, scale=scale)


def lenient_mask(box, pts, faces=range(6)):
    """Membership with `<=` in place of `<` at the listed faces (0..2 = lower x, y, z; 3..5 = upper): the mutant mask."""
    b = np.asarray(box, np.float64)
    ok = np.ones(len(pts), bool)
    for d in range(3):
        ok &= (pts[:, d] >= b[d]) if d in faces else (pts[:, d] > b[d])
        ok &= (pts[:, d] <= b[3 + d]) if 3 + d in faces else (pts[:, d] < b[3 + d])
    return ok


def icp_with_mask(case, mask_fn, th=1.0, max_iteration=10000):
    """oracle.icp.registration_icp per cluster of `case` with the targets chosen by mask_fn(box_row, frame) -> bool mask."""
    from oracle import icp as oicp
    mats = []
    for j, (loc, M) in enumerate(zip(case["local"], case["M"])):
        tgt = case["frame"][mask_fn(case["box"][j], case["frame"])]
        mats.append(oicp.registration_icp(np.asarray(loc, np.float64), tgt, th, M, max_iteration)[0])
    return np.array(mats)
