"""numpy restatement of the link-clearance contract (include/creg.h, creg_mesh_clearance_f64), written from the header in its
operation order, plus the analytic cases the clearance tests share.

    gap2(a, b)   = (g_x^2 + g_y^2) + g_z^2,  g_k = max(0, max(lo_a[k] - hi_b[k], lo_b[k] - hi_a[k]))
    contributes  gap2(box_a, box_b) <= d_max * d_max
    d2(a, b)     0 when the pair collides by the mesh-collide predicate, else the minimum of 3 + 3 pt_tri2 and 9 seg_seg2 terms

Elementwise numpy operations are single IEEE operations, so the values are the kernel's; every branch of the header is a
``np.where`` over all lanes here (the divisions of the lanes that do not take a branch are computed and dropped)."""
import numpy as np

from _collide_ref import all_pairs, box_mesh, pack, pierces, pose, rigid, uv_sphere  # noqa: F401  (re-exported to the tests)

INF = np.inf
BLOCK = 8192                                                     # triangle pairs evaluated at a time: the temporaries stay in cache


# ------------------------------------------------------------------------------------------ the contract
# Points travel component-major, (3, n), so that every elementwise operation runs over contiguous rows.
def dot(u, v):
    return (u[0] * v[0] + u[1] * v[1]) + u[2] * v[2]


def clamp01(x):
    return np.where(x < 0, 0.0, np.where(x > 1, 1.0, x))


def gap2(lo_a, hi_a, lo_b, hi_b):
    """Boxes as (..., 3) arrays."""
    g = np.maximum(0.0, np.maximum(lo_a - hi_b, lo_b - hi_a))
    return (g[..., 0] * g[..., 0] + g[..., 1] * g[..., 1]) + g[..., 2] * g[..., 2]


def _cm(x):
    return np.ascontiguousarray(np.asarray(x, np.float64).T)


def pt_tri2(p, a, b, c):
    """Squared distance of points p (n,3) from triangles (a, b, c) (n,3 each)."""
    return _pt_tri2(_cm(p), _cm(a), _cm(b), _cm(c))


def seg_seg2(p1, q1, p2, q2):
    """Squared distance of segments (p1, q1) and (p2, q2), (n,3) each."""
    return _seg_seg2(_cm(p1), _cm(q1), _cm(p2), _cm(q2))


def _pt_tri2(p, a, b, c):
    """The header's seven cases, the first that holds; (3,n) operands."""
    with np.errstate(all="ignore"):
        ab, ac, ap, bp, cp = b - a, c - a, p - a, p - b, p - c
        d1, d2, d3, d4, d5, d6 = dot(ab, ap), dot(ac, ap), dot(ab, bp), dot(ac, bp), dot(ab, cp), dot(ac, cp)
        vc, vb, va = d1 * d4 - d3 * d2, d5 * d2 - d1 * d6, d3 * d6 - d5 * d4
        # 7 face
        s = (va + vb) + vc
        v, w = np.where(s > 0, vb / s, 0.0), np.where(s > 0, vc / s, 0.0)
        # 6 edge bc
        c6 = (va <= 0) & (d4 - d3 >= 0) & (d5 - d6 >= 0)
        den = (d4 - d3) + (d5 - d6)
        w6 = np.where(den > 0, (d4 - d3) / den, 0.0)
        v, w = np.where(c6, 1.0 - w6, v), np.where(c6, w6, w)
        # 5 edge ac
        c5 = (vb <= 0) & (d2 >= 0) & (d6 <= 0)
        den = d2 - d6
        v, w = np.where(c5, 0.0, v), np.where(c5, np.where(den > 0, d2 / den, 0.0), w)
        # 4 edge ab
        c4 = (vc <= 0) & (d1 >= 0) & (d3 <= 0)
        den = d1 - d3
        v, w = np.where(c4, np.where(den > 0, d1 / den, 0.0), v), np.where(c4, 0.0, w)
        q = p - ((a + ab * v) + ac * w)
        out = dot(q, q)
        out = np.where((d6 >= 0) & (d5 <= d6), dot(cp, cp), out)             # 3 vertex c
        out = np.where((d3 >= 0) & (d4 <= d3), dot(bp, bp), out)             # 2 vertex b
        out = np.where((d1 <= 0) & (d2 <= 0), dot(ap, ap), out)              # 1 vertex a
    return out


def _seg_seg2(p1, q1, p2, q2):
    """The header's four cases; (3,n) operands."""
    with np.errstate(all="ignore"):
        u, v, r = q1 - p1, q2 - p2, p1 - p2
        a, e, f, c, b = dot(u, u), dot(v, v), dot(v, r), dot(u, r), dot(u, v)
        # 4 both proper
        den = a * e - b * b
        s = np.where(den > 0, clamp01((b * f - c * e) / den), 0.0)
        t = (b * s + f) / e
        lo, hi = t < 0, t > 1
        s = np.where(lo, clamp01((0.0 - c) / a), np.where(hi, clamp01((b - c) / a), s))
        t = np.where(lo, 0.0, np.where(hi, 1.0, t))
        # 3 the second is a point
        c3 = e <= 0
        s, t = np.where(c3, clamp01((0.0 - c) / a), s), np.where(c3, 0.0, t)
        # 2 the first is a point
        c2 = a <= 0
        s, t = np.where(c2, 0.0, s), np.where(c2, clamp01(f / e), t)
        # 1 two points
        c1 = (a <= 0) & (e <= 0)
        s, t = np.where(c1, 0.0, s), np.where(c1, 0.0, t)
        x = (p1 + u * s) - (p2 + v * t)
    return dot(x, x)


def pair_d2(a, b):
    """d2 of triangle pairs a, b (n,3,3 each), whether or not they contribute."""
    loA, hiA, loB, hiB = a.min(1), a.max(1), b.min(1), b.max(1)
    zero = np.zeros(len(a), bool)
    k = np.flatnonzero(((loA <= hiB) & (loB <= hiA)).all(1))     # "collides" needs the boxes to meet: the edge tests run there only
    for E, T in ((a[k], b[k]), (b[k], a[k])):
        for e in range(3):
            zero[k] |= pierces(E[:, e], E[:, (e + 1) % 3], T[:, 0], T[:, 1], T[:, 2])
    av, bv = [_cm(a[:, i]) for i in range(3)], [_cm(b[:, i]) for i in range(3)]
    d = np.full(len(a), INF)
    for i in range(3):
        d = np.minimum(d, _pt_tri2(av[i], bv[0], bv[1], bv[2]))
        d = np.minimum(d, _pt_tri2(bv[i], av[0], av[1], av[2]))
    for i in range(3):
        for j in range(3):
            d = np.minimum(d, _seg_seg2(av[i], av[(i + 1) % 3], bv[j], bv[(j + 1) % 3]))
    return np.where(zero, 0.0, d)


def contributing(A, B, dmax2, chunk=1 << 22):
    """(ia, ib) of the contributing pairs of posed triangles A (na,3,3), B (nb,3,3), lexicographic; the box pre-filter of the
    contract, in row blocks so that the gap matrix stays small."""
    loA, hiA, loB, hiB = A.min(1), A.max(1), B.min(1), B.max(1)
    step = max(1, chunk // max(1, len(B)))
    ias, ibs = [], []
    for a0 in range(0, len(A), step):
        g = gap2(loA[a0:a0 + step, None], hiA[a0:a0 + step, None], loB[None], hiB[None])
        ia, ib = np.nonzero(g <= dmax2)
        ias.append(ia + a0)
        ibs.append(ib)
    return np.concatenate(ias), np.concatenate(ibs)


def link_clearance(A, B, dmax2):
    """(dist2, ia, ib, runner-up) of two posed links: the minimum d2 over the contributing pairs, the lexicographically
    smallest pair with exactly its bits, and the smallest d2 among the OTHER contributing pairs (+inf if there is none: the
    tests compare witnesses exactly where the minimum is unique); (+inf, -1, -1, +inf) when none contributes.  Links are
    culled by their boxes first (exact by contract)."""
    if len(A) == 0 or len(B) == 0:
        return INF, -1, -1, INF
    pa, pb = A.reshape(-1, 3), B.reshape(-1, 3)
    if not gap2(pa.min(0), pa.max(0), pb.min(0), pb.max(0)) <= dmax2:
        return INF, -1, -1, INF
    ia, ib = contributing(A, B, dmax2)
    if len(ia) == 0:
        return INF, -1, -1, INF
    d = np.concatenate([pair_d2(A[ia[k:k + BLOCK]], B[ib[k:k + BLOCK]]) for k in range(0, len(ia), BLOCK)])
    best = d.min()
    k = int(np.flatnonzero(d == best)[0])                        # (ia, ib) is in lexicographic order
    d[k] = INF
    return float(best), int(ia[k]), int(ib[k]), float(d.min())


def mesh_clearance(tri, tri_start, link_T, pairs, d_max, runner_up=False):
    """dist2 (P,M) f64, witness (P,M,2) int32, link_box (P,L,6) f64 of creg_mesh_clearance_f64; with ``runner_up`` also the
    (P,M) smallest d2 among the contributing pairs other than the witness."""
    tri = np.asarray(tri, np.float64).reshape(-1, 3, 3)
    link_T = np.asarray(link_T, np.float64)
    if link_T.ndim == 3:
        link_T = link_T[None]
    pairs = np.asarray(pairs, np.int64).reshape(-1, 2)
    P, L, M = link_T.shape[0], link_T.shape[1], len(pairs)
    dmax2 = np.float64(d_max) * np.float64(d_max)
    dist2, second = np.full((P, M), INF), np.full((P, M), INF)
    witness = np.full((P, M, 2), -1, np.int32)
    box = np.empty((P, L, 6))
    box[..., :3], box[..., 3:] = INF, -INF
    for p in range(P):
        posed = [pose(tri[tri_start[l]:tri_start[l + 1]], link_T[p, l]) for l in range(L)]
        for l in range(L):
            if len(posed[l]):
                box[p, l, :3], box[p, l, 3:] = posed[l].reshape(-1, 3).min(0), posed[l].reshape(-1, 3).max(0)
        done = {}
        for m, (la, lb) in enumerate(pairs):
            if not (0 <= la < L and 0 <= lb < L) or la == lb:
                continue
            if (la, lb) not in done:
                done[la, lb] = link_clearance(posed[la], posed[lb], dmax2)
            d, ia, ib, second[p, m] = done[la, lb]
            dist2[p, m] = d
            if ia >= 0:
                witness[p, m] = (tri_start[la] + ia, tri_start[lb] + ib)
    return (dist2, witness, box, second) if runner_up else (dist2, witness, box)


def tri_pair_d2(a, b):
    """d2 of one triangle against one triangle (3,3 each)."""
    return float(pair_d2(np.asarray(a, np.float64)[None], np.asarray(b, np.float64)[None])[0])


# ------------------------------------------------------------------------------------------ analytic cases: two triangles
# name -> (triangle a, triangle b, expected DISTANCE as a formula).  a is the contract's lattice base unless the case needs another.
BASE = [[0, 0, 0], [4, 0, 0], [0, 4, 0]]
H = 0.75
ANALYTIC = {
    # b's lowest vertex (1,1,H) hangs over the interior of the base
    "vertex_over_face": (BASE, [[1, 1, H], [1, 2, H + 1], [2, 1, H + 1]], H),
    # b's vertex (2,-1,H) is beside the edge y = 0: sqrt(1 + H^2)
    "vertex_over_edge": (BASE, [[2, -1, H], [2, -2, H + 1], [3, -2, H + 1]], np.sqrt(1.0 + H * H)),
    # b's vertex (-1,-2,-2) is nearest the corner (0,0,0): sqrt(1 + 4 + 4)
    "vertex_vertex": (BASE, [[-1, -2, -2], [-2, -3, -2], [-2, -2, -3]], np.sqrt(1.0 + 4.0 + 4.0)),
    # the edge y = 0 of the base and b's edge (2,-1,H)-(2,1,H) cross at height H; b rises away from the base
    "skew_edges": ([[0, 0, 0], [4, 0, 0], [2, -4, -3]], [[2, -1, H], [2, 1, H], [2, 0, H + 3]], H),
    # b's edge (1,-1,0)-(3,-1,0) runs parallel to the edge y = 0 at distance 1, in the same plane, b on the far side
    "parallel_edges": (BASE, [[1, -1, 0], [3, -1, 0], [2, -3, 0]], 1.0),
    # the prototype's cases
    "parallel_offset": ([[0, 0, 0], [1, 0, 0], [0, 1, 0]], [[0.2, 0.2, 0.37], [1.2, 0.2, 0.37], [0.2, 1.2, 0.37]], 0.37),
    "coplanar_disjoint": ([[0, 0, 0], [1, 0, 0], [0, 1, 0]], [[3, 0, 0], [4, 0, 0], [3, 1, 0]], 2.0),
    "coplanar_overlapping": (BASE, [[1, 1, 0], [5, 1, 0], [1, 5, 0]], 0.0),
    "pierced": (BASE, [[1, 1, -1], [1, 1, 1], [3, 3, 1]], 0.0),
    # a zero-length edge: b is the segment (1,1,H)-(1,2,H+1) with its first vertex twice
    "zero_length_edge": (BASE, [[1, 1, H], [1, 1, H], [1, 2, H + 1]], H),
    # a point: all three vertices the same
    "point_triangle": (BASE, [[1, 1, H], [1, 1, H], [1, 1, H]], H),
}


def two_links(a, b):
    """tri, tri_start, link_T (1,2,4,4) of two one-triangle links at the identity."""
    tri, start = pack([[a], [b]])
    return tri, start, np.tile(np.eye(4), (1, 2, 1, 1))


def scene_diagonal(tri, tri_start, link_T):
    """Diagonal of the box of all posed vertices of all poses: the scale of the value tolerance."""
    link_T = np.asarray(link_T, np.float64)
    if link_T.ndim == 3:
        link_T = link_T[None]
    pts = [pose(tri[tri_start[l]:tri_start[l + 1]], T[l]).reshape(-1, 3) for T in link_T for l in range(T.shape[0])]
    pts = np.concatenate(pts)
    return float(np.linalg.norm(pts.max(0) - pts.min(0)))
