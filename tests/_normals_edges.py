"""Edge families for csrc/normals.hip (`k_knn_normals`) and a plain float64 restatement of its covariance and eigen-solver
(test infrastructure, no test functions).

The families are deterministic and seeded; every builder returns cases `(label, P float64 (n,3), radius, max_nn)`:

  size_cases        random clouds at sizes around KNN_Q = 128 / KNN_TILE = 512 / max_nn, every max_nn edge, three radii
  tie_cases         shuffled integer lattices at spacing 1/8 (all squared distances exact, dozens of ties per query), radii whose
                    square is exactly a squared lattice distance (points AT the radius must be excluded)
  duplicate_cases   every point repeated 2, 31 or 40 times in one shuffled cloud
  island_cases      separated islands (spacing > radius + diameter, so an island is exactly the neighbourhood of each of its
                    points): the degenerate covariances the solver's branches are there for
  surface_cases     a sphere and an ellipsoid with their analytic outward normals (orientation against geometry)

The restatement (`raw_covariance`, `smallest_eigvec`, `kernel_normals`) follows the kernel's operation order one rounded
operation at a time (the library is built with -ffp-contract=off) and REPORTS WHICH BRANCHES IT TOOK.  It is not expected to
give the kernel's bits: the device's acos / cos may differ from libm's by an ulp.  It is the reference the GPU bound is derived
from: `rayleigh_excess` measures, against numpy.linalg.eigvalsh of the covariance computed in extended precision from centred
coordinates, how far the restatement's normal is from the smallest eigenvalue, (n^T C n - l0) / lmax.  Since
n^T C n - l0 >= (l1 - l0) sin^2(angle), that bounds the angle wherever the direction is defined and asks nothing where it is
not.  MEASURED_EXCESS below is that measurement per family (tests/test_normals_edges_cpu.py asserts it is current); the GPU
tests allow `gpu_bound(family)` = max(16 x measured, 64 x 2^-52): the device's acos / cos / sqrt may be a few ulp from libm's and
the excess is quadratic in the angle error (4 x the angle error is 16 x the excess).
"""
import math

import numpy as np

KNN_Q, KNN_TILE, KNN_MAX = 128, 512, 32
EPS = 2.0 ** -52
BOUND_FLOOR = 64 * EPS

# every decision of smallest_eigvec / eigvec_by_rows / eigvec_deflated / the kernel's final normalisation
BRANCHES = ("zero", "diagonal", "hd>=0", "hd<0", "rows01", "rows02", "rows12", "dm==0", "U_from_x", "U_from_y",
            "norm_a00_by_m00", "norm_a00_by_m01", "norm_a11_by_m11", "norm_a11_by_m01", "cu1_a00", "cu1_a11", "l2==0")
# not reachable from any real symmetric input, with the reason (tests/test_normals_edges_cpu.py checks the rest are reached)
UNREACHABLE = {
    "cu1_a11": "the else arm is entered only with a11 > a00 >= 0, so fmax(a11, a01) > 0 always holds there (finite inputs)",
}
# reachable, but not from a covariance of points through smallest_eigvec: reached by a constructed input fed to the
# restatement's eigvec_by_rows / eigvec_deflated directly (the trigonometric eigenvalues would have to be exact)
CONSTRUCTED_ONLY = ("dm==0", "cu1_a00")

# ---------------------------------------------------------------------------------------------------------------------------
# Largest Rayleigh excess (n^T C n - l0) / lmax of the RESTATEMENT per family, rounded up to two digits, as measured by
# tests/test_normals_edges_cpu.py::test_restatement_rayleigh_excess_per_family (which fails if a figure that matters -- one
# above a sixteenth of the floor -- is exceeded, or recorded at more than twice what it measures).  What the figures say:
#   * well-scaled neighbourhoods, exact planes and lines included, stay below 1e-15: the solver is as good as eigh there;
#   * blob_1e3 is the raw moments' cancellation (|x|^2 eps / lmax = 1e-6 of error in C), not the solver;
#   * needle_1e-4 / needle_1e-6: hd -> 1 when the two small eigenvalues nearly coincide, and acos(hd) turns the 1e-16 error of hd
#     into 1e-8 of error in the angle, so the two small eigenvalues carry ABSOLUTE errors near 1e-8 lmax.  At or below that
#     (thin variance 1e-8 and 1e-12 of lmax) the deflation step cannot tell them apart and the normal is some unit vector of
#     the thin plane: perpendicular to the needle to 1e-16, but up to (l1 - l0) / lmax in excess.  That is a property of the
#     non-iterative algorithm the kernel restates; the bound records it rather than hiding it.
#
#   family            measured   GPU bound = max(16 x measured, 64 x 2^-52 = 1.42e-14)
MEASURED_EXCESS = {
    "size":           8.4e-16,  # 1.42e-14
    "tie":            8.7e-16,  # 1.42e-14
    "duplicate":      2.3e-16,  # 1.42e-14
    "plane_axis":     0.0,      # 1.42e-14
    "line_axis":      0.0,      # 1.42e-14
    "plane_rot":      2.7e-16,  # 1.42e-14
    "line_rot":       3.0e-16,  # 1.42e-14
    "plane_noise":    1.7e-16,  # 1.42e-14
    "needle_5e-2":    2.0e-16,  # 1.42e-14
    "needle_1e-4":    3.4e-9,   # 5.44e-08
    "needle_1e-6":    7.8e-13,  # 1.25e-11
    "pancake":        1.7e-16,  # 1.42e-14
    "octahedron":     2.0e-15,  # 3.20e-14
    "lattice_uneq":   0.0,      # 1.42e-14
    "lattice_eq":     0.0,      # 1.42e-14
    "box_two_tie":    0.0,      # 1.42e-14
    "identical":      0.0,      # 1.42e-14
    "blob":           1.7e-16,  # 1.42e-14
    "blob_1e3":       1.3e-10,  # 2.08e-09
}


def family_of(label):
    return label.split("/")[0]


def gpu_bound(family):
    return max(16.0 * MEASURED_EXCESS[family], BOUND_FLOOR)


# ------------------------------------------------------------------------------------------ the restatement
def _cross(a, b):
    return [a[1] * b[2] - a[2] * b[1], a[2] * b[0] - a[0] * b[2], a[0] * b[1] - a[1] * b[0]]


def eigvec_by_rows(A, ev, taken):
    r0, r1, r2 = [A[0] - ev, A[1], A[2]], [A[1], A[3] - ev, A[4]], [A[2], A[4], A[5] - ev]
    c01, c02, c12 = _cross(r0, r1), _cross(r0, r2), _cross(r1, r2)
    d0 = c01[0] * c01[0] + c01[1] * c01[1] + c01[2] * c01[2]
    d1 = c02[0] * c02[0] + c02[1] * c02[1] + c02[2] * c02[2]
    d2 = c12[0] * c12[0] + c12[1] * c12[1] + c12[2] * c12[2]
    c, dm, which = c01, d0, "rows01"
    if d1 > dm:
        c, dm, which = c02, d1, "rows02"
    if d2 > dm:
        c, dm, which = c12, d2, "rows12"
    taken.add(which if dm > 0 else "dm==0")
    inv = 1.0 / math.sqrt(dm) if dm > 0 else 0.0
    return [c[0] * inv, c[1] * inv, c[2] * inv]


def eigvec_deflated(A, e0, ev1, taken):
    if abs(e0[0]) > abs(e0[1]):
        il = 1.0 / math.sqrt(e0[0] * e0[0] + e0[2] * e0[2])
        U = [-e0[2] * il, 0.0, e0[0] * il]
        taken.add("U_from_x")
    else:
        il = 1.0 / math.sqrt(e0[1] * e0[1] + e0[2] * e0[2])
        U = [0.0, e0[2] * il, -e0[1] * il]
        taken.add("U_from_y")
    V = _cross(e0, U)
    mul = lambda W: [A[0] * W[0] + A[1] * W[1] + A[2] * W[2], A[1] * W[0] + A[3] * W[1] + A[4] * W[2],
                     A[2] * W[0] + A[4] * W[1] + A[5] * W[2]]
    AU, AV = mul(U), mul(V)
    m00 = U[0] * AU[0] + U[1] * AU[1] + U[2] * AU[2] - ev1
    m01 = U[0] * AV[0] + U[1] * AV[1] + U[2] * AV[2]
    m11 = V[0] * AV[0] + V[1] * AV[1] + V[2] * AV[2] - ev1
    a00, a01, a11 = abs(m00), abs(m01), abs(m11)
    if a00 >= a11:
        if max(a00, a01) > 0:
            if a00 >= a01:
                m01 /= m00; m00 = 1.0 / math.sqrt(1.0 + m01 * m01); m01 *= m00
                taken.add("norm_a00_by_m00")
            else:
                m00 /= m01; m01 = 1.0 / math.sqrt(1.0 + m00 * m00); m00 *= m01
                taken.add("norm_a00_by_m01")
            cu, cv = m01, -m00
        else:
            cu, cv = 1.0, 0.0
            taken.add("cu1_a00")
    else:
        if max(a11, a01) > 0:
            if a11 >= a01:
                m01 /= m11; m11 = 1.0 / math.sqrt(1.0 + m01 * m01); m01 *= m11
                taken.add("norm_a11_by_m11")
            else:
                m11 /= m01; m01 = 1.0 / math.sqrt(1.0 + m11 * m11); m11 *= m01
                taken.add("norm_a11_by_m01")
            cu, cv = m11, -m01
        else:
            cu, cv = 1.0, 0.0
            taken.add("cu1_a11")
    return [cu * U[a] + cv * V[a] for a in range(3)]


def smallest_eigvec(C):
    """C = (c00, c01, c02, c11, c12, c22) -> (vector, set of branch names); the zero vector for C = 0, as the kernel's."""
    C = [float(c) for c in C]
    taken = set()
    mx = 0.0
    for c in C:
        mx = max(mx, abs(c))
    if not mx > 0:
        taken.add("zero")
        return [0.0, 0.0, 0.0], taken
    A = [c / mx for c in C]
    off2 = A[1] * A[1] + A[2] * A[2] + A[4] * A[4]
    if off2 > 0:
        q = (A[0] + A[3] + A[5]) / 3.0
        b00, b11, b22 = A[0] - q, A[3] - q, A[5] - q
        p = math.sqrt((b00 * b00 + b11 * b11 + b22 * b22 + 2.0 * off2) / 6.0)
        c00, c01, c02 = b11 * b22 - A[4] * A[4], A[1] * b22 - A[4] * A[2], A[1] * A[4] - b11 * A[2]
        det = (b00 * c00 - A[1] * c01 + A[2] * c02) / (p * p * p)
        hd = min(max(det * 0.5, -1.0), 1.0)
        ang = math.acos(hd) / 3.0
        beta2, beta0 = math.cos(ang) * 2.0, math.cos(ang + 2.09439510239319549) * 2.0
        beta1 = -(beta0 + beta2)
        e0, e1, e2 = q + p * beta0, q + p * beta1, q + p * beta2
        if hd >= 0:
            taken.add("hd>=0")
            v2 = eigvec_by_rows(A, e2, taken)
            v1 = eigvec_deflated(A, v2, e1, taken)
            return _cross(v1, v2), taken
        taken.add("hd<0")
        return eigvec_by_rows(A, e0, taken), taken
    taken.add("diagonal")
    return diagonal_axis(A[0], A[3], A[5]), taken


def diagonal_axis(a0, a3, a5):
    """The diagonal branch's rule: the axis of the smallest entry; z whenever z is among the smallest, y when only x and y tie."""
    n0 = 1.0 if (a0 < a3 and a0 < a5) else 0.0
    n1 = 1.0 if (n0 == 0.0 and a3 <= a0 and a3 < a5) else 0.0
    return [n0, n1, 1.0 if (n0 == 0.0 and n1 == 0.0) else 0.0]


def pad_lists(lists, width=None):
    """list of index arrays -> (idx (n,width) int64, -1 past the count; cnt (n))."""
    cnt = np.array([len(r) for r in lists], np.int64)
    width = int(cnt.max()) if width is None else width
    idx = np.full((len(lists), width), -1, np.int64)
    for i, r in enumerate(lists):
        idx[i, :len(r)] = r
    return idx, cnt


def raw_covariance(P, idx, cnt):
    """The kernel's covariance of every neighbour list: nine raw moments summed in list order, divided by the count, then
    c_ab = m_ab - m_a m_b.  (n,6) float64 in the order (c00, c01, c02, c11, c12, c22); rows with cnt == 0 are NaN."""
    n = len(idx)
    m = np.zeros((9, n))
    for p in range(idx.shape[1]):
        on = p < cnt
        x, y, z = (np.where(on, P[np.maximum(idx[:, p], 0), a], 0.0) for a in range(3))
        for a, t in enumerate((x, y, z, x * x, x * y, x * z, y * y, y * z, z * z)):
            m[a] = m[a] + t                                             # adding +0.0 past the count changes nothing
    with np.errstate(invalid="ignore", divide="ignore"):
        m = m / cnt.astype(np.float64)
    return np.stack([m[3] - m[0] * m[0], m[4] - m[0] * m[1], m[5] - m[0] * m[2], m[6] - m[1] * m[1], m[7] - m[1] * m[2],
                     m[8] - m[2] * m[2]], 1)


def kernel_normals(P, idx, cnt):
    """The kernel's normals from given neighbour lists: ((n,3) float64, list of branch-name sets)."""
    C = raw_covariance(P, idx, cnt)
    out = np.tile([0.0, 0.0, 1.0], (len(idx), 1))
    taken = []
    for i in range(len(idx)):
        if cnt[i] < 3:
            taken.append({"cnt<3"})
            continue
        v, t = smallest_eigvec(C[i])
        l2 = v[0] * v[0] + v[1] * v[1] + v[2] * v[2]
        if not l2 > 0:
            t.add("l2==0")
            v = [0.0, 0.0, 1.0]
        else:
            il = 1.0 / math.sqrt(l2)
            v = [v[0] * il, v[1] * il, v[2] * il]
        out[i] = v
        taken.append(t)
    return out, taken


# ------------------------------------------------------------------------------------------ the measurement
def exact_covariance(P, idx, cnt):
    """Covariance of every neighbour list from CENTRED coordinates in extended precision: (n,3,3) longdouble."""
    on = (np.arange(idx.shape[1])[None, :] < cnt[:, None])
    Q = P[np.maximum(idx, 0)].astype(np.longdouble) * on[:, :, None]
    k = np.maximum(cnt, 1).astype(np.longdouble)[:, None]
    d = (Q - (Q.sum(1) / k)[:, None, :]) * on[:, :, None]
    return np.einsum("nka,nkb->nab", d, d) / k[:, :, None]


def rayleigh_excess(P, idx, cnt, N):
    """(excess (n), identical (n) bool): (n^T C n - l0) / lmax with C the extended-precision covariance and l0 <= lmax from
    numpy.linalg.eigvalsh; `identical` marks neighbourhoods whose points are all the same point (C = 0 exactly: every unit
    vector is an eigenvector, excess reported as 0)."""
    C = exact_covariance(P, idx, cnt)
    scale = np.abs(C).max((1, 2))
    identical = scale == 0
    Cs = C / np.where(identical, 1, scale)[:, None, None]
    w = np.linalg.eigvalsh(Cs.astype(np.float64))
    Nl = np.asarray(N, np.longdouble)
    ray = np.einsum("na,nab,nb->n", Nl, Cs, Nl)
    lmax = np.where(identical, 1.0, w[:, 2])
    return np.where(identical, 0.0, (ray - w[:, 0]) / lmax).astype(np.float64), identical


# ------------------------------------------------------------------------------------------ families
TINY_RADIUS = 1e-9                     # below every distance between distinct points of the random clouds: only the point itself
SIZES = (1, 2, 3, 4, 29, 30, 31, 32, 33, 127, 128, 129, 511, 512, 513, 1024, 1537)
SIZE_MAX_NN = (1, 2, 3, 30, 32)
SIZE_RADII = (0.1, TINY_RADIUS, -1.0)


def size_cloud(n):
    """Uniform in a cube sized so that a ball of radius 0.1 holds about 15 points (lists partly full at max_nn = 30 / 32, full at
    3, and the radius cut binds); the small clouds sit in a cube of side 0.16."""
    side = max(0.16, 0.1 * (n / 3.6) ** (1.0 / 3.0))
    return np.random.default_rng(1000 + n).uniform(0.0, side, size=(n, 3))


def size_cases(sizes=SIZES):
    for n in sizes:
        P = size_cloud(n)
        for k in SIZE_MAX_NN:
            for r in SIZE_RADII:
                yield f"size/n{n}_k{k}_r{r:g}", P, r, k


def _lattice(shape, spacing, seed, offset=(0, 0, 0)):
    g = np.stack(np.meshgrid(*[np.arange(s) + o for s, o in zip(shape, offset)], indexing="ij"), -1).reshape(-1, 3)
    P = g.astype(np.float64) * spacing
    return P[np.random.default_rng(seed).permutation(len(P))]


def tie_cases():
    """Spacing 1/8: squared distances are k/64, exact.  radius 1/8: the six face neighbours sit AT the radius (only the point
    itself qualifies); radius 1/4: squared distances 0..3/64 qualify (27 in the interior), the six at 4/64 do not.  max_nn = 12
    cuts inside the twelve edge neighbours (a tie decides membership), 30 and 32 inside the 24 at 5/64 without a radius."""
    clouds = (("8x8x8", _lattice((8, 8, 8), 0.125, 1)),                       # n = 512 = KNN_TILE
              ("9x7x5_off", _lattice((9, 7, 5), 0.125, 2, (-3, 5, 2))),       # n = 315, negative and offset coordinates
              ("11x11x11", _lattice((11, 11, 11), 0.125, 3)))                 # n = 1331
    for name, P in clouds:
        for r, k in ((0.125, 30), (0.25, 30), (0.25, 32), (0.25, 12), (0.25, 3), (-1.0, 12), (-1.0, 30), (-1.0, 32),
                     (-1.0, 2), (0.375, 32)):
            yield f"tie/{name}_k{k}_r{r:g}", P, r, k


def duplicate_cases():
    rng = np.random.default_rng(7)
    base = rng.uniform(0.0, 0.3, size=(36, 3))
    reps = np.array([2] * 20 + [31] * 8 + [40] * 8)
    P = np.repeat(base, reps, axis=0)
    P = P[rng.permutation(len(P))]                                             # n = 608
    for r, k in ((0.1, 30), (0.1, 32), (-1.0, 30), (-1.0, 32), (-1.0, 3), (0.1, 1), (TINY_RADIUS, 30)):
        yield f"duplicate/c2_31_40_k{k}_r{r:g}", P, r, k


ISLAND_RADIUS = 0.1
ISLAND_PITCH = 0.25                    # centre to centre; islands stay inside a ball of radius 0.045 (diameter 0.09 < radius,
ISLAND_REACH = 0.045                   # and 0.25 - 0.09 > radius: an island is exactly the neighbourhood of each of its points)


def _centres(m):
    g = np.stack(np.meshgrid(*[np.arange(-2, 3)] * 3, indexing="ij"), -1).reshape(-1, 3)
    g = g[np.argsort((g * g).sum(1), kind="stable")]
    return g[:m].astype(np.float64) * ISLAND_PITCH                             # dyadic, |coordinate| <= 0.5


def _rotations(rng, m):
    q = rng.normal(size=(m, 4))
    q /= np.linalg.norm(q, axis=1, keepdims=True)
    w, x, y, z = q.T
    return np.stack([1 - 2 * (y * y + z * z), 2 * (x * y - z * w), 2 * (x * z + y * w), 2 * (x * y + z * w),
                     1 - 2 * (x * x + z * z), 2 * (y * z - x * w), 2 * (x * z - y * w), 2 * (y * z + x * w),
                     1 - 2 * (x * x + y * y)], 1).reshape(-1, 3, 3)


def _clip(L):
    r = np.linalg.norm(L, axis=-1, keepdims=True)
    return L * np.minimum(1.0, 0.04 / np.maximum(r, 1e-300))


def _gauss_islands(rng, m, k, sig, rotate=True):
    """m islands of k points, N(0, diag(sig)^2) in a local frame (clipped to the reach), randomly rotated."""
    L = _clip(rng.normal(size=(m, k, 3)) * np.asarray(sig))
    if rotate:
        L = np.einsum("mab,mkb->mka", _rotations(rng, m), L)
    return L


def _dyadic(rng, shape, bits=10, reach=0.025):
    """Random multiples of 2^-bits in [-reach, reach]: sums and products of a few dozen of them are exact in float64."""
    s = int(reach * 2 ** bits)
    return rng.integers(-s, s + 1, size=shape).astype(np.float64) / 2 ** bits


def _assemble(local, seed):
    """local: list of (k_i,3) island-local coordinates -> shuffled cloud, island centres on the dyadic grid."""
    c = _centres(len(local))
    P = np.concatenate([c[i] + np.asarray(L, np.float64) for i, L in enumerate(local)])
    assert max(np.linalg.norm(np.asarray(L), axis=1).max() for L in local) <= ISLAND_REACH
    return P[np.random.default_rng(seed).permutation(len(P))]


def _boxes(spacings, shape):
    out = []
    for s in spacings:
        g = np.stack(np.meshgrid(*[np.arange(n) - (n - 1) / 2 for n in shape], indexing="ij"), -1).reshape(-1, 3)
        out.append(g * np.asarray(s, np.float64))
    return out


_S = (1 / 64, 1 / 128, 1 / 256)
_PERMS = ((0, 1, 2), (0, 2, 1), (1, 0, 2), (1, 2, 0), (2, 0, 1), (2, 1, 0))


def expected_axis(spacing):
    """Axis of the smallest spacing of an axis-aligned symmetric box; z whenever z is among the smallest, y when x and y tie."""
    return np.array(diagonal_axis(*[float(s) for s in spacing]))


def island_cases():
    """(label, P, radius, max_nn) per island family; the families named in DIAGONAL_FAMILIES have exactly diagonal covariances
    and `diagonal_expected(label, P)` gives the axis every normal must equal."""
    rng = np.random.default_rng(11)
    R, K = ISLAND_RADIUS, 32
    m = 48
    # exact axis-aligned planes / lines, 16 points each (sums of dyadic numbers and the division by 16 are exact, so the
    # covariance has exactly zero rows for the constant axes: the smallest eigenvalue is exactly 0)
    planes, lines = [], []
    for i in range(m):
        L = _dyadic(rng, (16, 3))
        L[:, i % 3] = _dyadic(rng, ())
        planes.append(L)
        L = _dyadic(rng, (16, 3))
        L[:, [(i + 1) % 3, (i + 2) % 3]] = _dyadic(rng, (2,))
        lines.append(L)
    yield "plane_axis/16pts", _assemble(planes, 21), R, K
    yield "line_axis/16pts", _assemble(lines, 22), R, K
    # rotated planes / lines (zero thickness before rotation: the smallest eigenvalue is rounding noise)
    yield "plane_rot/20pts", _assemble(list(_gauss_islands(rng, m, 20, (0.015, 0.012, 0.0))), 23), R, K
    yield "line_rot/20pts", _assemble(list(_gauss_islands(rng, m, 20, (0.015, 0.0, 0.0))), 24), R, K
    noisy = _gauss_islands(rng, m, 20, (0.015, 0.012, 0.0)) + rng.normal(size=(m, 20, 3)) * 1e-9
    yield "plane_noise/1e-9", _assemble(list(noisy), 25), R, K
    for tag, s in (("5e-2", 0.05), ("1e-4", 1e-4), ("1e-6", 1e-6)):
        yield f"needle_{tag}/24pts", _assemble(list(_gauss_islands(rng, m, 24, (0.015, 0.015 * s, 0.015 * s))), 26), R, K
    pk = np.concatenate([_gauss_islands(rng, m // 3, 24, (0.015, 0.012, 0.015 * s)) for s in (1e-2, 1e-4, 1e-6)])
    yield "pancake/24pts", _assemble(list(pk), 27), R, K
    # the six-point octahedron, arms 0.02 (1 +- 1e-9): near-isotropic, axis-aligned and rotated
    arms = np.concatenate([np.eye(3), -np.eye(3)])[None] * 0.02 * (1 + 1e-9 * rng.uniform(-1, 1, size=(m, 6, 1)))
    arms[m // 2:] = np.einsum("mab,mkb->mka", _rotations(rng, m - m // 2), arms[m // 2:])
    yield "octahedron/6pts", _assemble(list(arms), 28), R, K
    # full 3x3x3 lattices: unequal spacings in every order (diagonal covariance, distinct entries) ...
    yield "lattice_uneq/3x3x3", _assemble(_boxes([[_S[j] for j in p] for p in _PERMS] * 4, (3, 3, 3)), 29), R, K
    # ... equal spacings (diagonal, all three tie -> z).  3x3x3 islands sit at (+-c, +-c, +-c), where the three diagonal
    # entries round alike (the division by 27 is inexact); the 2x2x2 cubes anywhere (the division by 8 is exact)
    eq = _boxes([[s] * 3 for s in _S] * 2 + [[_S[0]] * 3, [_S[1]] * 3], (3, 3, 3))
    corners = np.array([[a, b, c] for a in (-1, 1) for b in (-1, 1) for c in (-1, 1)], np.float64) * ISLAND_PITCH
    P = np.concatenate([corners[i] + L for i, L in enumerate(eq)] +
                       [(_centres(27)[i] + np.array([0, 0, 4 * ISLAND_PITCH])) + L
                        for i, L in enumerate(_boxes([[s] * 3 for s in _S] * 9, (2, 2, 2)))])
    yield "lattice_eq/3x3x3_2x2x2", P[np.random.default_rng(30).permutation(len(P))], R, K
    # ... and 2x2x2 boxes whose two SMALLEST spacings tie: x = y < z (-> y), x = z < y (-> z), y = z < x (-> z); with the two
    # largest tying the smallest is unique
    pairs = ((_S[1], _S[0]), (_S[2], _S[0]), (_S[2], _S[1]))                  # (a, b) with a < b
    two = [t for a, b in pairs for t in ((a, a, b), (a, b, a), (b, a, a))]
    big = [t for a, b in pairs for t in ((b, b, a), (b, a, b), (a, b, b))]
    yield "box_two_tie/2x2x2", _assemble(_boxes((two + big) * 2, (2, 2, 2)), 31), R, K
    # islands of identical points: dyadic coordinates (covariance exactly 0) and arbitrary ones (rounding noise)
    ident = [np.tile(_dyadic(rng, (1, 3)), (20, 1)) for _ in range(m // 2)] + \
            [np.tile(rng.uniform(-0.025, 0.025, size=(1, 3)), (20, 1)) for _ in range(m // 2)]
    yield "identical/20pts", _assemble(ident, 32), R, K
    # general blobs, and the same blobs moved to coordinates near 1e3 (cancellation in the raw moments)
    blobs = _assemble(list(_gauss_islands(rng, m, 28, (0.015, 0.008, 0.003))), 33)
    yield "blob/28pts", blobs, R, K
    yield "blob_1e3/28pts", blobs + np.array([1000.0, -1000.0, 1000.0]), R, K


DIAGONAL_FAMILIES = ("lattice_uneq", "lattice_eq", "box_two_tie")


def diagonal_expected(P, idx, cnt):
    """Expected normal of every point of an axis-aligned symmetric box island, from the island's own extents (not from any
    covariance): the box's spacing along an axis is proportional to its extent."""
    out = np.empty((len(P), 3))
    for i in range(len(P)):
        Q = P[idx[i, :cnt[i]]]
        out[i] = expected_axis(Q.max(0) - Q.min(0))
    return out


SPHERE = dict(centre=(0.4, -0.2, 0.3), axes=(0.3, 0.3, 0.3))
ELLIPSOID = dict(centre=(-0.3, 0.5, 0.2), axes=(0.35, 0.2, 0.12))


def surface_cases(n=1200):
    """(label, P, outward unit normals): points of a closed convex surface, off-centre, in shuffled order."""
    i = np.arange(n) + 0.5
    z = 1 - 2 * i / n
    phi = i * math.pi * (3 - math.sqrt(5))
    D = np.stack([np.sqrt(1 - z * z) * np.cos(phi), np.sqrt(1 - z * z) * np.sin(phi), z], 1)      # Fibonacci directions
    for s, (name, g) in enumerate((("sphere", SPHERE), ("ellipsoid", ELLIPSOID))):
        a = np.asarray(g["axes"])
        perm = np.random.default_rng(40 + s).permutation(n)
        L = (D * a)[perm]
        out = L / (a * a)
        yield name, L + np.asarray(g["centre"]), out / np.linalg.norm(out, axis=1, keepdims=True)


def all_list_cases():
    """Every case whose neighbour lists are compared with the oracle's, element for element."""
    yield from size_cases()
    yield from tie_cases()
    yield from duplicate_cases()
    yield from island_cases()
