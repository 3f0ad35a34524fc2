"""Case families for csrc/joints.hip (`k_link_clouds` through creg_link_clouds_f64 / ops.link_clouds), a plain float64
restatement of it, and a pure-Python model of its slice and stride loop (test infrastructure, no test functions, no torch).

The restatement (`link_clouds_ref`) follows the kernel one rounded operation at a time (the library is built with
-ffp-contract=off): the cluster coords summed in set order and divided by the count, quat_to_matrix as in creg_dev.h,
pose_to_f32_matrix, inv4 (Gauss-Jordan with partial pivoting, REPORTING WHICH ROW SWAPS IT TOOK), and
((x R0 + y R1) + z R2) + t for both clouds.  Every operation in it is one IEEE float64 (or float32) add, multiply or divide, so
it is expected to give the kernel's bits.  `lf_extended` evaluates clouds_lf from the same float32 link matrix and the same
world-frame rows in numpy.longdouble (the inverse refined by Newton steps) and `lf_error_eps` measures the restatement against
it row-wise in units of eps64 x |inv(Ml)_rot| (|w| + |t|); MEASURED_LF_EPS below is that measurement per family
(tests/test_link_clouds_cpu.py asserts it is current), and the GPU fallback bound of tests/test_gpu_link_clouds.py hangs on it.

`kernel_walk` is the specification the GPU run is held to: the kernel's loop over slices y, y + G, ... of LC_ROWS rows and,
inside a slice, over the link's clusters in set order with their rows clipped to the slice.  It counts how often every output
row is written and from which row of `points`.

Every family builder yields `(label, coords (T,K,7), matrices (T,K,4,4), links, points (N,3), point_offsets (T*K+1))`, float64,
seeded.  The x coordinate of points row i is i x 2^-s (s per case, so that the cloud stays a few centimetres wide): a shifted,
swapped, repeated or missing row cannot give the right bits.

  slice_cases      link row totals around the multiples of LC_ROWS, cluster boundaries at 1024 j - 1, 1024 j, 1024 j + 1,
                   a cluster across five slices, empty clusters first / in the middle / last, a link of empty clusters,
                   255 nine-point clusters at K = 256
  stride_cases     one (frame, link) of LC_MAX_SLICES x LC_ROWS + 1024 + 5 rows beside tiny links, T = 2
  layout_cases     L = K, L = 1, set order, a repeated and a shared cluster, clusters in no link that own points, T in {1, 10},
                   no points at all
  pose_cases       link matrices whose inversion swaps rows, translations of 1e3, quaternions of length 0.5 and 2, nearly
                   cancelling quaternions, cluster matrices that are not rigid
  antipodal_cases  q and exactly -q in one link: the mean quaternion is 0
"""
import math

import numpy as np

LC_NT, LC_ROWS, LC_MAX_SLICES = 256, 1024, 256           # csrc/joints.hip (tests/test_link_clouds_cpu.py reads them back)
MAX_K = 256
EPS = 2.0 ** -52

# ---------------------------------------------------------------------------------------------------------------------------
# Largest error of the RESTATEMENT's clouds_lf against lf_extended per family, in eps64 units of |inv(Ml)_rot| (|w| + |t|),
# rounded up to two digits, as measured by tests/test_link_clouds_cpu.py::test_restatement_lf_error_per_family (which fails
# if a figure is exceeded or recorded at more than twice what it measures).  Never measured against the kernel.  The figures
# are a few eps because -R^T t is formed inside the 4 x 4 elimination (three multiply-subtracts per entry of the inverse's
# last column) before the final dot product adds its own three roundings.
#
#   family     measured   GPU fallback bound = 4 x measured (one differently rounded division or subtraction in the elimination)
MEASURED_LF_EPS = {
    "slice":  1.9,   # 7.6
    "stride": 1.4,   # 5.6
    "layout": 1.7,   # 6.8
    "pose":   1.3,   # 5.2
}


def family_of(label):
    return label.split("/")[0]


def gpu_lf_bound(family):
    return 4.0 * MEASURED_LF_EPS[family]


# ------------------------------------------------------------------------------------------ the restatement
def quat_to_matrix(q):
    """creg_dev.h quat_to_matrix on q (..., 4) float64 [w, x, y, z] -> (..., 9), same operations in the same order."""
    q = np.asarray(q, np.float64)
    w, x, y, z = q[..., 0], q[..., 1], q[..., 2], q[..., 3]
    with np.errstate(divide="ignore", invalid="ignore"):
        s = 2.0 / (((w * w + x * x) + y * y) + z * z)
        R = [1.0 - s * (y * y + z * z), s * (x * y - z * w), s * (x * z + y * w),
             s * (x * y + z * w), 1.0 - s * (x * x + z * z), s * (y * z - x * w),
             s * (x * z - y * w), s * (y * z + x * w), 1.0 - s * (x * x + y * y)]
    return np.stack(R, axis=-1)


def pose_to_f32_matrix(t, R):
    """[R | t] rounded to float32, (..., 4, 4) float32 (the kernel keeps these values in doubles)."""
    t, R = np.asarray(t, np.float64), np.asarray(R, np.float64)
    M = np.zeros(R.shape[:-1] + (4, 4), np.float32)
    M[..., :3, :3] = R.reshape(R.shape[:-1] + (3, 3)).astype(np.float32)
    M[..., :3, 3] = t.astype(np.float32)
    M[..., 3, 3] = 1.0
    return M


def inv4(M, swaps=None):
    """joints.hip inv4 on a 4 x 4 (python floats: IEEE doubles); `swaps` collects the (column, pivot row) exchanges taken."""
    A = [[float(M[r][c]) for c in range(4)] + [1.0 if r == c else 0.0 for c in range(4)] for r in range(4)]
    for col in range(4):
        piv = col
        for r in range(col + 1, 4):
            if abs(A[r][col]) > abs(A[piv][col]):
                piv = r
        if piv != col:
            A[col], A[piv] = A[piv], A[col]
            if swaps is not None:
                swaps.add((col, piv))
        inv = _div(1.0, A[col][col])
        A[col] = [a * inv for a in A[col]]
        for r in range(4):
            if r == col:
                continue
            f = A[r][col]
            A[r] = [a - f * b for a, b in zip(A[r], A[col])]
    return np.array([row[4:] for row in A], np.float64)


def _div(a, b):
    return float(np.float64(a) / np.float64(b)) if b == 0.0 else a / b      # python raises where IEEE gives inf or NaN


def out_offsets_of(links, point_offsets, T, K):
    """Rows of every (frame, link), a cluster counted as often as the link names it: (T*L + 1) int64."""
    n = np.diff(np.asarray(point_offsets, np.int64)).reshape(T, K)
    per = np.array([[sum(int(n[t, k]) for k in link) for link in links] for t in range(T)], np.int64)
    return np.concatenate([[0], np.cumsum(per.reshape(-1))]).astype(np.int64)


def row_map(links, point_offsets, T, K):
    """For every output row: its row of `points`, its cluster, its (frame, link) block -- clusters concatenated in set order."""
    po = np.asarray(point_offsets, np.int64)
    src, clu, blk = [], [], []
    for t in range(T):
        for l, link in enumerate(links):
            for k in link:
                p0, p1 = int(po[t * K + k]), int(po[t * K + k + 1])
                src.append(np.arange(p0, p1, dtype=np.int64))
                clu.append(np.full(p1 - p0, k, np.int64))
                blk.append(np.full(p1 - p0, t * len(links) + l, np.int64))
    cat = lambda a: np.concatenate(a) if a else np.zeros(0, np.int64)
    return cat(src), cat(clu), cat(blk)


def _affine(P, M):
    """Rows of P through the 3 x 4 [R | t] of M: ((x R0 + y R1) + z R2) + t per component, as the kernel evaluates it."""
    x, y, z = P[:, 0], P[:, 1], P[:, 2]
    with np.errstate(invalid="ignore", over="ignore"):
        return np.stack([((x * M[r][0] + y * M[r][1]) + z * M[r][2]) + M[r][3] for r in range(3)], axis=1)


def link_clouds_ref(coords, matrices, links, points, point_offsets, swaps=None):
    """k_link_clouds: (link_matrices (T,L,4,4) f32, mean_matrices (T,L,4,4) f32, clouds_wf (M,3), clouds_lf (M,3),
    out_offsets (T*L+1) int64)."""
    coords, matrices = np.asarray(coords, np.float64), np.asarray(matrices, np.float64)
    points = np.asarray(points, np.float64).reshape(-1, 3)
    T, K = coords.shape[:2]
    L = len(links)
    oo = out_offsets_of(links, point_offsets, T, K)
    src, _, _ = row_map(links, point_offsets, T, K)
    lm = np.zeros((T, L, 4, 4), np.float32)
    mm = np.zeros((T, L, 4, 4), np.float32)
    wf = np.zeros((int(oo[-1]), 3), np.float64)
    lf = np.zeros((int(oo[-1]), 3), np.float64)
    Mk32 = pose_to_f32_matrix(coords[..., :3], quat_to_matrix(coords[..., 3:]))          # (T,K,4,4) float32
    po = np.asarray(point_offsets, np.int64)
    for l, link in enumerate(links):
        m = np.zeros((T, 7), np.float64)
        acc = np.zeros((T, 4, 4), np.float32)
        for k in link:                                            # set order, every frame at once
            m = m + coords[:, k]
            acc = acc + Mk32[:, k]
        m = m / np.float64(len(link))
        lm[:, l] = pose_to_f32_matrix(m[:, :3], quat_to_matrix(m[:, 3:]))
        mm[:, l] = acc / np.float32(len(link))
        for t in range(T):
            Ai = inv4(lm[t, l].astype(np.float64), swaps)
            o = int(oo[t * L + l])
            for k in link:
                n = int(po[t * K + k + 1] - po[t * K + k])
                if n:
                    w = _affine(points[src[o:o + n]], matrices[t, k])
                    wf[o:o + n] = w
                    lf[o:o + n] = _affine(w, Ai)
                o += n
    return lm, mm, wf, lf, oo


# ------------------------------------------------------------------------------------------ extended precision
def inverse_extended(M):
    """Inverse of a 4 x 4 (given in float32 or float64) in numpy.longdouble: numpy's float64 inverse, refined by Newton steps."""
    A = np.asarray(M, np.float64).astype(np.longdouble)
    X = np.linalg.inv(np.asarray(M, np.float64)).astype(np.longdouble)
    I2 = 2 * np.eye(4, dtype=np.longdouble)
    for _ in range(4):
        X = X @ (I2 - A @ X)
    return X


def lf_extended(link_matrices, clouds_wf, links, out_offsets):
    """clouds_lf from the float32 link matrices and the float64 world-frame rows, evaluated in numpy.longdouble, and the
    row-wise yardstick |inv(Ml)_rot| (|w| + |t|) (both (M,3) longdouble)."""
    T, L = link_matrices.shape[:2]
    w = np.asarray(clouds_wf, np.float64).astype(np.longdouble)
    lf, unit = np.zeros_like(w), np.zeros_like(w)
    for b in range(T * L):
        o0, o1 = int(out_offsets[b]), int(out_offsets[b + 1])
        if o0 == o1:
            continue
        Ml = link_matrices[b // L, b % L]
        X = inverse_extended(Ml)
        lf[o0:o1] = w[o0:o1] @ X[:3, :3].T + X[:3, 3]
        unit[o0:o1] = (np.abs(w[o0:o1]) + np.abs(Ml[:3, 3].astype(np.longdouble))) @ np.abs(X[:3, :3]).T
    return lf, unit


def lf_error_eps(clouds_lf, lf_ext, unit):
    """Largest |clouds_lf - lf_ext| / (eps64 x unit) over all rows and components (0 for no rows)."""
    if len(lf_ext) == 0:
        return 0.0
    err = np.abs(np.asarray(clouds_lf, np.float64).astype(np.longdouble) - lf_ext)
    assert (unit > 0).all()
    return float((err / (np.longdouble(EPS) * unit)).max())


# ------------------------------------------------------------------------------------------ the kernel's loops
MUTATIONS = ("source_without_o", "hi_one_short", "first_trip_only")


def launch_grid_y(max_link_rows, rows=LC_ROWS, max_slices=LC_MAX_SLICES):
    """grid.y of creg_link_clouds_f64."""
    slices = (int(max_link_rows) + rows - 1) // rows
    return min(max(slices, 1), max_slices)


def kernel_walk(out_offsets, point_offsets, links, T, K, G, rows=LC_ROWS, nt=None, mutation=None):
    """k_link_clouds' loops in plain Python: workgroup (b, y) takes slices y, y + G, ... of `rows` rows of block b and walks
    the link's clusters in set order, clipping each to the slice.  Returns (writes (n_out) how often a row is written,
    source (n_out) the row of `points` it was last written from, trips the largest number of slices one workgroup took,
    straddles how many (slice, cluster) visits were clipped by a slice boundary).  nt: walk dst = lo + tid, lo + tid + nt, ...
    thread by thread instead of at once.  mutation: one of MUTATIONS, a deliberately wrong walk (the tests show they are
    noticed)."""
    oo, po = [int(v) for v in out_offsets], [int(v) for v in point_offsets]
    L, n_out, n_pts = len(links), oo[-1], po[-1]
    writes, source = np.zeros(n_out, np.int64), np.full(n_out, -1, np.int64)
    trips, straddles = 0, 0
    for b in range(T * L):
        t, l = divmod(b, L)
        o_beg, o_end = max(oo[b], 0), min(oo[b + 1], n_out)
        for y in range(G):
            s0, trip = o_beg + y * rows, 0
            while s0 < o_end:
                trip += 1
                s1 = min(s0 + rows, o_end)
                o = o_beg
                for k in links[l]:
                    if not o < s1:
                        break
                    p0, p1 = po[t * K + k], min(po[t * K + k + 1], n_pts)
                    n = max(p1 - p0, 0)
                    lo, hi = max(o, s0), min(o + n, s1)
                    if mutation == "hi_one_short":
                        hi = min(o + n, s1 - 1)
                    if lo < hi:
                        straddles += (lo > o) + (hi < o + n)
                        dsts = (np.arange(lo, hi) if nt is None else
                                np.array([d for tid in range(nt) for d in range(lo + tid, hi, nt)], np.int64))
                        np.add.at(writes, dsts, 1)
                        source[dsts] = p0 + (dsts - (0 if mutation == "source_without_o" else o))
                    o += n
                s0 += G * rows
                if mutation == "first_trip_only":
                    break
            trips = max(trips, trip)
    return writes, source, trips, straddles


# ------------------------------------------------------------------------------------------ case builders
def _unit(v):
    v = np.asarray(v, np.float64)
    return v / np.linalg.norm(v, axis=-1, keepdims=True)


def _rigid(coords):
    """(T,K,4,4) float64 [R | t] of coords (T,K,7): the cluster poses as the pipeline would hold them."""
    M = np.zeros(coords.shape[:2] + (4, 4), np.float64)
    M[..., :3, :3] = quat_to_matrix(coords[..., 3:]).reshape(coords.shape[:2] + (3, 3))
    M[..., :3, 3] = coords[..., :3]
    M[..., 3, 3] = 1.0
    return M


def _points(sizes, rng):
    """Packed points for sizes (T,K): x = global row x 2^-s (exact), y and z random within 3 cm."""
    po = np.concatenate([[0], np.cumsum(np.asarray(sizes, np.int64).reshape(-1))]).astype(np.int64)
    n = int(po[-1])
    P = rng.uniform(-0.03, 0.03, size=(n, 3))
    s = max(int(math.ceil(math.log2(max(n, 2) / 0.05))), 0)
    P[:, 0] = np.arange(n, dtype=np.float64) * 2.0 ** -s
    return P, po


def _case(label, sizes, links, seed, coords=None, matrices=None):
    sizes = np.asarray(sizes, np.int64)
    T, K = sizes.shape
    rng = np.random.default_rng(seed)
    if coords is None:
        coords = np.concatenate([rng.uniform(-0.3, 0.3, size=(T, K, 3)), _unit(rng.normal(size=(T, K, 4)))], axis=2)
    if matrices is None:
        matrices = _rigid(coords)
    P, po = _points(sizes, rng)
    return label, np.ascontiguousarray(coords), np.ascontiguousarray(matrices), [list(l) for l in links], P, po


def _split(total, cuts):
    """Cluster sizes of a link of `total` rows with cluster boundaries at `cuts` (ascending, within [0, total])."""
    edges = [0] + list(cuts) + [total]
    return [b - a for a, b in zip(edges[:-1], edges[1:])]


SLICE_TOTALS = (0, 1, 1023, 1024, 1025, 2047, 2048, 2049, 3 * 1024 + 17)


def slice_cases():
    R = LC_ROWS
    # every total, three clusters per link, the totals rotated over the links from frame to frame; link 9 is always empty
    rng = np.random.default_rng(100)
    T, nl = 3, len(SLICE_TOTALS)
    sizes = np.zeros((T, 3 * nl + 2), np.int64)
    for t in range(T):
        for i in range(nl):
            total = SLICE_TOTALS[(i + t) % nl]
            cuts = sorted(int(c) for c in rng.integers(0, total + 1, size=2))
            sizes[t, 3 * i:3 * i + 3] = _split(total, cuts)
    links = [[3 * i, 3 * i + 1, 3 * i + 2] for i in range(nl)] + [[3 * nl, 3 * nl + 1]]
    yield _case("slice/totals", sizes, links, 101)
    # boundaries one row before, at and one row after the multiples of LC_ROWS; and three in a row around the first
    a = _split(7 * R + 300, [R - 1, 2 * R, 3 * R + 1, 4 * R, 5 * R - 1, 6 * R + 1])
    b = _split(2 * R + 2, [R - 1, R, R + 1, 2 * R - 1, 2 * R, 2 * R + 1])
    sizes = np.array([a + b, b + a[::-1]], np.int64)
    yield _case("slice/boundaries", sizes, [list(range(len(a))), list(range(len(a), len(a) + len(b)))], 102)
    # one cluster across five slices (rows 700 .. 700 + 3 * 1024 + 500), then a short one
    sizes = np.array([[700, 3 * R + 500, 40, 5], [3 * R + 500, 700, 5, 40]], np.int64)
    yield _case("slice/span", sizes, [[0, 1, 2], [3]], 103)
    # empty clusters first, in the middle and last; a link whose clusters are all empty
    sizes = np.array([[0, 600, 0, 0, 900, 0, 0, 0, 30], [0, R, 0, 0, R + 1, 0, 0, 0, 0]], np.int64)
    yield _case("slice/empties", sizes, [[0, 1, 2, 3, 4, 5], [6, 7], [8]], 104)
    # 255 nine-point clusters at the largest K: boundaries fall inside clusters 113 and 227
    sizes = np.full((2, MAX_K), 9, np.int64)
    sizes[1, 255] = 0
    order = list(np.random.default_rng(105).permutation(255))
    yield _case("slice/k256", sizes, [order, [255]], 105)


STRIDE_ROWS = LC_MAX_SLICES * LC_ROWS + LC_ROWS + 5


def stride_cases():
    # frame 1, link 1 (block 4 of 6) has 262 144 + 1024 + 5 rows: workgroups y = 0 and y = 1 take a second trip, the last
    # slice has 5 rows; every other (frame, link) has a handful, so most workgroups of the launch find nothing to do
    sizes = np.array([[5, 7, 3, 2, 4, 6],
                      [3, 100001, 63172, 100000, 2, 1]], np.int64)
    assert sizes[1, 1:4].sum() == STRIDE_ROWS
    yield _case("stride/big", sizes, [[0], [3, 1, 2], [4, 5]], 200)


def layout_cases():
    rng = np.random.default_rng(300)
    K = 12
    sizes = rng.integers(0, 60, size=(10, K))
    yield _case("layout/L=K_T10", sizes, [[int(k)] for k in rng.permutation(K)], 301)
    sizes = rng.integers(1, 400, size=(1, K))
    yield _case("layout/L=1_T1", sizes, [[int(k) for k in rng.permutation(K)]], 302)
    # cluster 3 twice in link 0, cluster 1 in links 0 and 1, clusters 2, 4, 6, 7 in no link but with points of their own
    sizes = rng.integers(1, 700, size=(10, 8))
    yield _case("layout/repeated_shared_unused", sizes, [[3, 1, 3], [1, 0], [5]], 303)
    sizes = rng.integers(200, 900, size=(1, 8))
    yield _case("layout/unused_T1", sizes, [[7, 2], [5, 0]], 304)
    # compute_joints.link_transforms' call: no points at all
    yield _case("layout/no_points", np.zeros((1, 7), np.int64), [[6, 0], [3], [2, 1, 4]], 305)


def _turn(axis, angle):
    q = np.zeros(4)
    q[0], q[1 + axis] = math.cos(angle / 2), math.sin(angle / 2)
    return q


# a generic rotation whose first column has its largest entry in row 2 and whose second then pivots on row 2 again
GENERIC_Q = (_unit([0.6, 0.1, -0.7, 0.2]), _unit([0.5, 0.5, 0.5, 0.5]), _unit([0.1, 0.7, 0.7, 0.1]), _unit([0.7, 0.1, 0.2, 0.7]))


def pose_cases():
    # frames = poses; links [0], [1, 2] (both clusters the same quaternion: the mean is exact), [3]
    quats = [_turn(a, s * math.pi / 2) for a in range(3) for s in (1, -1)] + [_turn(a, math.pi) for a in range(3)]
    quats += list(GENERIC_Q)
    for name, tr, qlen in (("turns", 0.1, 1.0), ("turns_t1e3", 1e3, 1.0), ("turns_q0.5", 1.0, 0.5), ("turns_q2", 1e3, 2.0)):
        rng = np.random.default_rng(400)
        T = len(quats)
        coords = np.zeros((T, 4, 7))
        coords[..., :3] = tr * rng.uniform(-1, 1, size=(T, 4, 3))
        coords[..., 3:] = np.array(quats)[:, None, :] * qlen
        yield _case(f"pose/{name}", rng.integers(5, 40, size=(T, 4)), [[0], [1, 2], [3]], 401, coords=coords)
    # nearly cancelling quaternions: q and -q + delta, |mean q| = |delta| / 2
    for mean_len in (1e-3, 1e-6):
        rng = np.random.default_rng(410)
        T = 12
        coords = np.zeros((T, 4, 7))
        coords[..., :3] = rng.uniform(-1, 1, size=(T, 4, 3))
        q = _unit(rng.normal(size=(T, 4)))
        coords[:, 0, 3:], coords[:, 1, 3:] = q, -q + 2 * mean_len * _unit(rng.normal(size=(T, 4)))
        coords[:, 2, 3:], coords[:, 3, 3:] = -q[::-1] + 2 * mean_len * _unit(rng.normal(size=(T, 4))), q[::-1]
        yield _case(f"pose/cancel_{mean_len:g}", rng.integers(5, 40, size=(T, 4)), [[0, 1], [2, 3]], 411, coords=coords)
    # cluster matrices that are not rigid: the kernel uses them as given
    label, coords, M, links, P, po = _case("pose/scaled", np.random.default_rng(420).integers(5, 40, size=(6, 4)),
                                           [[0], [1, 2], [3]], 421)
    M = M.copy()
    M[..., :3, :3] *= np.array([1.7, 0.4, 1.0])[None, None, None, :]
    M[:, 1, :3, :3] *= 3.0
    yield label, coords, M, links, P, po


ANTIPODAL_BLOCKS = ((0, 0), (1, 2))                        # the (frame, link) pairs whose quaternions cancel exactly


def antipodal_cases():
    rng = np.random.default_rng(500)
    T, K = 2, 5
    coords = np.concatenate([rng.uniform(-0.3, 0.3, size=(T, K, 3)), _unit(rng.normal(size=(T, K, 4)))], axis=2)
    coords[0, 1, 3:] = -coords[0, 0, 3:]                   # frame 0, link 0 = clusters (0, 1)
    coords[1, 4, 3:] = -coords[1, 3, 3:]                   # frame 1, link 2 = clusters (3, 4)
    yield _case("antipodal/two_links", rng.integers(20, 1500, size=(T, K)), [[0, 1], [2], [3, 4]], 501, coords=coords)


FAMILIES = {"slice": slice_cases, "stride": stride_cases, "layout": layout_cases, "pose": pose_cases,
            "antipodal": antipodal_cases}


def first_case(family, name):
    return next(c for c in FAMILIES[family]() if c[0] == f"{family}/{name}")
