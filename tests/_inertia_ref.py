"""Mass properties of closed triangle meshes: a numpy restatement of creg_mesh_inertia_f64's contract (include/creg.h) --
the same terms in the same operation order, the same summation tree, the same derived quantities -- an exact evaluation of
the sums in ``fractions.Fraction``, and the meshes the tests use.  No GPU, no project code."""
import math
from fractions import Fraction

import numpy as np

N_TERMS = 14
PAIRS = ((0, 0), (0, 1), (0, 2), (1, 1), (1, 2), (2, 2))          # xx xy xz yy yz zz
U = 2.0 ** -53


# ------------------------------------------------------------------------------------------------ the contract
def _cross(u, v):
    return np.stack([u[:, 1] * v[:, 2] - u[:, 2] * v[:, 1], u[:, 2] * v[:, 0] - u[:, 0] * v[:, 2],
                     u[:, 0] * v[:, 1] - u[:, 1] * v[:, 0]], 1)


def terms(tri):
    """(F,14) terms of one link's triangles tri (F,3,3) f64, in creg.h's operation order."""
    tri = np.asarray(tri, np.float64).reshape(-1, 3, 3)
    if len(tri) == 0:
        return np.zeros((0, N_TERMS))
    r = tri[0, 0]
    a, b, c = tri[:, 0] - r, tri[:, 1] - r, tri[:, 2] - r
    s = (a + b) + c
    n = _cross(b - a, c - a)
    g = _cross(b, c)
    d = (a[:, 0] * g[:, 0] + a[:, 1] * g[:, 1]) + a[:, 2] * g[:, 2]
    out = np.empty((len(tri), N_TERMS))
    out[:, 0:3] = n
    out[:, 3] = np.sqrt((n[:, 0] * n[:, 0] + n[:, 1] * n[:, 1]) + n[:, 2] * n[:, 2])
    out[:, 4] = d
    out[:, 5:8] = d[:, None] * s
    for k, (i, j) in enumerate(PAIRS):
        out[:, 8 + k] = d * (((s[:, i] * s[:, j] + a[:, i] * a[:, j]) + b[:, i] * b[:, j]) + c[:, i] * c[:, j])
    return out


def tree_sum(x):
    """The contract's tree over the rows of x (F,14): 256 leaves = four butterflies of 64, then ((w0 + w1) + w2) + w3; the
    results are the next level's leaves, until one is left (at least one level)."""
    x = np.asarray(x, np.float64).reshape(-1, N_TERMS)
    if len(x) == 0:
        return np.zeros(N_TERMS)
    lane = np.arange(64)
    while True:
        groups = -(-len(x) // 256)
        pad = np.zeros((groups * 256, N_TERMS))
        pad[:len(x)] = x
        w = pad.reshape(groups, 4, 64, N_TERMS)
        for off in (32, 16, 8, 4, 2, 1):
            w = w + w[:, :, lane ^ off]
        w = w[:, :, 0]
        x = ((w[:, 0] + w[:, 1]) + w[:, 2]) + w[:, 3]
        if groups == 1:
            return x[0]


def k_bound(F):
    """creg.h's k: 8 roundings on a term's longest path plus the tree's depth, 9 per level."""
    chunks = -(-max(int(F), 1) // 256)
    levels, n = 1, chunks
    while n > 256:
        n = -(-n // 256)
        levels += 1
    return 8 + 9 * (1 + levels)


def link_sums(tri):
    """sums (14) of one link as the entry point returns them: zeros for no triangle or a zero sum of d."""
    S = tree_sum(terms(tri))
    return S if S[4] != 0.0 else np.zeros(N_TERMS)


def derive(S, r, density):
    """volume, area, closure, mass, com, inertia (6), principal (3), axes (3,3) from sums S (14), the reference point r (3)
    and the density, in creg.h's order.  principal / axes by numpy's eigh (rows of axes = eigenvectors)."""
    S = np.asarray(S, np.float64)
    with np.errstate(all="ignore"):
        vol = S[4] / 6.0
        area = S[3] / 2.0
        closure = np.sqrt((S[0] * S[0] + S[1] * S[1]) + S[2] * S[2]) / S[3] if S[3] > 0 else 0.0
        mass = density * vol
        if not S[4] != 0.0:
            nan = float("nan")
            return dict(volume=vol, area=area, closure=closure, mass=mass, com=np.full(3, nan), inertia=np.full(6, nan),
                        principal=np.full(3, nan), axes=np.full((3, 3), nan))
        m = (S[5:8] / 24.0) / vol
        com = np.asarray(r, np.float64) + m
        C = {p: S[8 + k] / 120.0 - (vol * m[p[0]]) * m[p[1]] for k, p in enumerate(PAIRS)}
        J = np.array([density * (C[1, 1] + C[2, 2]), -(density * C[0, 1]), -(density * C[0, 2]),
                      density * (C[0, 0] + C[2, 2]), -(density * C[1, 2]), density * (C[0, 0] + C[1, 1])])
    w, V = np.linalg.eigh(full(J))
    return dict(volume=vol, area=area, closure=closure, mass=mass, com=com, inertia=J, principal=w, axes=V.T.copy())


def full(J):
    ixx, ixy, ixz, iyy, iyz, izz = J
    return np.array([[ixx, ixy, ixz], [ixy, iyy, iyz], [ixz, iyz, izz]])


def mesh_inertia(tri, tri_start, density=1.0):
    """The whole entry point: one dict of stacked arrays, keys as ops.mesh_inertia's."""
    tri = np.asarray(tri, np.float64).reshape(-1, 3, 3)
    L = len(tri_start) - 1
    density = np.broadcast_to(np.asarray(density, np.float64), (L,))
    rows = []
    for l in range(L):
        t = tri[tri_start[l]:tri_start[l + 1]]
        S = link_sums(t)
        rows.append(dict(derive(S, t[0, 0] if len(t) else np.zeros(3), density[l]), sums=S))
    return {k: np.stack([np.asarray(r[k]) for r in rows]) for k in rows[0]}


# ------------------------------------------------------------------------------------------------ exact sums
def _fsqrt(q, bits=160):
    """sqrt of the Fraction q >= 0 to a relative 2^-bits (far below 2^-53)."""
    if q == 0:
        return Fraction(0)
    shift = max(0, bits - (q.numerator.bit_length() - q.denominator.bit_length()) // 2)
    return Fraction(math.isqrt((q.numerator << (2 * shift)) * q.denominator), q.denominator << shift)


def exact_sums(tri):
    """(sum of the 14 terms, sum of their absolute values) of one link, exactly (term 3 to 2^-160), as lists of Fraction."""
    tri = np.asarray(tri, np.float64).reshape(-1, 3, 3)
    tot, tot_abs = [Fraction(0)] * N_TERMS, [Fraction(0)] * N_TERMS
    if len(tri) == 0:
        return tot, tot_abs
    fr = [[[Fraction(float(x)) for x in v] for v in t] for t in tri]
    r = fr[0][0]
    cross = lambda u, v: [u[1] * v[2] - u[2] * v[1], u[2] * v[0] - u[0] * v[2], u[0] * v[1] - u[1] * v[0]]
    for t in fr:
        a, b, c = ([v[k] - r[k] for k in range(3)] for v in t)
        s = [a[k] + b[k] + c[k] for k in range(3)]
        n = cross([b[k] - a[k] for k in range(3)], [c[k] - a[k] for k in range(3)])
        g = cross(b, c)
        d = a[0] * g[0] + a[1] * g[1] + a[2] * g[2]
        x = n + [_fsqrt(n[0] * n[0] + n[1] * n[1] + n[2] * n[2]), d] + [d * s[k] for k in range(3)]
        x += [d * (s[i] * s[j] + a[i] * a[j] + b[i] * b[j] + c[i] * c[j]) for i, j in PAIRS]
        tot = [p + q for p, q in zip(tot, x)]
        tot_abs = [p + abs(q) for p, q in zip(tot_abs, x)]
    return tot, tot_abs


def sum_errors(got, tri):
    """|got - exact| / (2^-53 sum|term|) per term of one link (0 where both vanish): what k_bound(F) bounds."""
    tot, tot_abs = exact_sums(tri)
    out = np.zeros(N_TERMS)
    for k in range(N_TERMS):
        err = abs(Fraction(float(got[k])) - tot[k])
        out[k] = float(err / (tot_abs[k] * Fraction(U))) if tot_abs[k] > 0 else (0.0 if err == 0 else float("inf"))
    return out


# ------------------------------------------------------------------------------------------------ meshes
def _outward(verts, tris):
    """Orient the faces of a mesh that is star-shaped about its vertex mean: normals away from it."""
    verts, tris = np.asarray(verts, np.float64), np.asarray(tris, np.int64).copy()
    t = verts[tris]
    n = np.cross(t[:, 1] - t[:, 0], t[:, 2] - t[:, 0])
    flip = np.einsum("ij,ij->i", n, t.mean(1) - verts.mean(0)) < 0
    tris[flip] = tris[flip][:, ::-1]
    return verts, tris


def tetrahedron(p0=(0, 0, 0), p1=(1, 0, 0), p2=(0, 1, 0), p3=(0, 0, 1)):
    """F = 4."""
    return _outward(np.array([p0, p1, p2, p3], np.float64), [[0, 1, 2], [0, 1, 3], [0, 2, 3], [1, 2, 3]])


def box(a=1.0, b=1.0, c=1.0, centre=(0, 0, 0)):
    """F = 12: edges a, b, c along x, y, z."""
    v = np.array([[x, y, z] for x in (-0.5, 0.5) for y in (-0.5, 0.5) for z in (-0.5, 0.5)]) * [a, b, c] + np.asarray(centre, np.float64)
    quads = [[0, 1, 3, 2], [4, 6, 7, 5], [0, 4, 5, 1], [2, 3, 7, 6], [0, 2, 6, 4], [1, 5, 7, 3]]
    return _outward(v, [[q[0], q[1], q[2]] for q in quads] + [[q[0], q[2], q[3]] for q in quads])


def bipyramid(n, radius=1.0, height=0.7):
    """F = 2 n: an n-gon in the xy plane with an apex above and below."""
    th = 2 * np.pi * np.arange(n) / n
    v = np.vstack([np.stack([radius * np.cos(th), radius * np.sin(th), np.zeros(n)], 1), [[0, 0, height], [0, 0, -height]]])
    i = np.arange(n)
    j = (i + 1) % n
    return _outward(v, np.vstack([np.stack([i, j, np.full(n, n)], 1), np.stack([j, i, np.full(n, n + 1)], 1)]))


def icosphere(s, stretch=(1.0, 1.0, 1.0), shift=(0.0, 0.0, 0.0)):
    """F = 20 * 4^s: an icosahedron subdivided s times on the unit sphere, then stretched along the axes and shifted."""
    p = (1 + 5 ** 0.5) / 2
    verts = [np.array(v, np.float64) / np.linalg.norm(v) for v in
             [(-1, p, 0), (1, p, 0), (-1, -p, 0), (1, -p, 0), (0, -1, p), (0, 1, p), (0, -1, -p), (0, 1, -p), (p, 0, -1), (p, 0, 1),
              (-p, 0, -1), (-p, 0, 1)]]
    tris = [(0, 11, 5), (0, 5, 1), (0, 1, 7), (0, 7, 10), (0, 10, 11), (1, 5, 9), (5, 11, 4), (11, 10, 2), (10, 7, 6), (7, 1, 8),
            (3, 9, 4), (3, 4, 2), (3, 2, 6), (3, 6, 8), (3, 8, 9), (4, 9, 5), (2, 4, 11), (6, 2, 10), (8, 6, 7), (9, 8, 1)]
    for _ in range(s):
        mid, nxt = {}, []

        def midpoint(i, j):
            key = (min(i, j), max(i, j))
            if key not in mid:
                m = verts[i] + verts[j]
                verts.append(m / np.linalg.norm(m))
                mid[key] = len(verts) - 1
            return mid[key]
        for a, b, c in tris:
            ab, bc, ca = midpoint(a, b), midpoint(b, c), midpoint(c, a)
            nxt += [(a, ab, ca), (b, bc, ab), (c, ca, bc), (ab, bc, ca)]
        tris = nxt
    return _outward(np.array(verts) * np.asarray(stretch, np.float64) + np.asarray(shift, np.float64), tris)


def triangles(mesh, shift=(0.0, 0.0, 0.0), f32=False):
    """(F,3,3) f64 of a (verts, tris) mesh, shifted; with f32 the VERTICES are rounded to float32 first, so shared ones stay shared."""
    verts, tris = mesh
    verts = verts + np.asarray(shift, np.float64)
    if f32:
        verts = verts.astype(np.float32).astype(np.float64)
    return verts[tris]


def pack(tri_list):
    """tri (F,3,3) and tri_start (L+1) int64 of a list of per-link (F_l,3,3) arrays."""
    start = np.concatenate([[0], np.cumsum([len(t) for t in tri_list])]).astype(np.int64)
    tri = np.concatenate([np.asarray(t, np.float64).reshape(-1, 3, 3) for t in tri_list]) if len(tri_list) else np.zeros((0, 3, 3))
    return np.ascontiguousarray(tri), start
