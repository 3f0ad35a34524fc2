"""numpy restatement of the mesh-collision contract (include/creg.h, creg_mesh_collide_f64), written from the contract in its
operation order, plus the meshes and scenes the collision tests share.

    posed vertex   w_i = ((R_i0 v_0 + R_i1 v_1) + R_i2 v_2) + t_i
    triangle pair  boxes (exact min / max of the posed vertices, closed comparisons) overlap AND some edge of one properly
                   pierces the other
    orient(p,q,r,s) = ((u x v)_x w_x + (u x v)_y w_y) + (u x v)_z w_z,  u = q - p, v = r - p, w = s - p

Elementwise numpy operations are single IEEE operations, so the decisions are the kernel's."""
import numpy as np


# ------------------------------------------------------------------------------------------ the contract
def pose(tri, T):
    """(n,3,3) link-frame triangles under the 4x4 pose T."""
    tri = np.asarray(tri, np.float64).reshape(-1, 3, 3)
    out = np.empty_like(tri)
    for i in range(3):
        out[..., i] = ((T[i, 0] * tri[..., 0] + T[i, 1] * tri[..., 1]) + T[i, 2] * tri[..., 2]) + T[i, 3]
    return out


def orient(p, q, r, s):
    u, v, w = q - p, r - p, s - p
    cx = u[..., 1] * v[..., 2] - u[..., 2] * v[..., 1]
    cy = u[..., 2] * v[..., 0] - u[..., 0] * v[..., 2]
    cz = u[..., 0] * v[..., 1] - u[..., 1] * v[..., 0]
    return (cx * w[..., 0] + cy * w[..., 1]) + cz * w[..., 2]


def pierces(p, q, a, b, c):
    """Edge (p,q) properly pierces triangle (a,b,c); a zero anywhere is no."""
    d1, d2 = orient(a, b, c, p), orient(a, b, c, q)
    opposite = ((d1 > 0) & (d2 < 0)) | ((d1 < 0) & (d2 > 0))
    s1, s2, s3 = orient(p, q, a, b), orient(p, q, b, c), orient(p, q, c, a)
    return opposite & (((s1 > 0) & (s2 > 0) & (s3 > 0)) | ((s1 < 0) & (s2 < 0) & (s3 < 0)))


def colliding_pairs(A, B):
    """Posed triangles A (na,3,3), B (nb,3,3) -> (ia, ib) of the colliding pairs in lexicographic order.  Box-prefiltered: the
    edge tests run on the pairs whose boxes overlap only (condition 1 of the contract)."""
    if len(A) == 0 or len(B) == 0:
        return np.zeros(0, np.int64), np.zeros(0, np.int64)
    loA, hiA, loB, hiB = A.min(1), A.max(1), B.min(1), B.max(1)
    meet = np.ones((len(A), len(B)), bool)
    for k in range(3):
        meet &= (loA[:, None, k] <= hiB[None, :, k]) & (loB[None, :, k] <= hiA[:, None, k])
    ia, ib = np.nonzero(meet)                                    # row-major: lexicographic in (ia, ib)
    a, b = A[ia], B[ib]
    hit = np.zeros(len(ia), bool)
    for E, T in ((a, b), (b, a)):
        for k in range(3):
            hit |= pierces(E[:, k], E[:, (k + 1) % 3], T[:, 0], T[:, 1], T[:, 2])
    return ia[hit], ib[hit]


def mesh_collide(tri, tri_start, link_T, pairs):
    """count (P,M) int32, first (P,M,2) int32, link_box (P,L,6) f64 of creg_mesh_collide_f64."""
    tri = np.asarray(tri, np.float64).reshape(-1, 3, 3)
    link_T = np.asarray(link_T, np.float64)
    if link_T.ndim == 3:
        link_T = link_T[None]
    pairs = np.asarray(pairs, np.int64).reshape(-1, 2)
    P, L, M = link_T.shape[0], link_T.shape[1], len(pairs)
    count = np.zeros((P, M), np.int32)
    first = np.full((P, M, 2), -1, np.int32)
    box = np.empty((P, L, 6))
    box[..., :3], box[..., 3:] = np.inf, -np.inf
    for p in range(P):
        posed = [pose(tri[tri_start[l]:tri_start[l + 1]], link_T[p, l]) for l in range(L)]
        for l in range(L):
            if len(posed[l]):
                box[p, l, :3], box[p, l, 3:] = posed[l].reshape(-1, 3).min(0), posed[l].reshape(-1, 3).max(0)
        for m, (la, lb) in enumerate(pairs):
            if not (0 <= la < L and 0 <= lb < L) or la == lb:
                continue
            ia, ib = colliding_pairs(posed[la], posed[lb])
            count[p, m] = len(ia)
            if len(ia):
                first[p, m] = (tri_start[la] + ia[0], tri_start[lb] + ib[0])
    return count, first, box


# ------------------------------------------------------------------------------------------ meshes
def box_mesh(hx, hy, hz):
    """12 triangles of the box [-hx,hx] x [-hy,hy] x [-hz,hz]."""
    c = np.array([[x, y, z] for x in (-hx, hx) for y in (-hy, hy) for z in (-hz, hz)], np.float64)
    quads = [(0, 1, 3, 2), (4, 6, 7, 5), (0, 4, 5, 1), (2, 3, 7, 6), (0, 2, 6, 4), (1, 5, 7, 3)]
    return np.array([[c[q[0]], c[q[a]], c[q[a + 1]]] for q in quads for a in (1, 2)])


def uv_sphere(r, seg=24, rings=13, n=None):
    """A UV sphere of 2 seg (rings - 1) proper triangles (one per quad at the poles), ring by ring from +z; the first ``n`` of
    them when given: a cap, an open mesh."""
    th = np.linspace(0, 2 * np.pi, seg + 1)
    ph = np.linspace(0, np.pi, rings + 1)
    pt = lambda t, p: [r * np.sin(p) * np.cos(t), r * np.sin(p) * np.sin(t), r * np.cos(p)]
    tris = []
    for i, (c0, c1) in enumerate(zip(ph[:-1], ph[1:])):
        for a, b in zip(th[:-1], th[1:]):
            if i > 0:
                tris.append([pt(a, c0), pt(b, c1), pt(b, c0)])
            if i < rings - 1:
                tris.append([pt(a, c0), pt(a, c1), pt(b, c1)])
    tris = np.asarray(tris, np.float64)
    assert len(tris) == 2 * seg * (rings - 1)
    return tris if n is None else tris[:n]


def random_rotation(rng):
    q, r = np.linalg.qr(rng.normal(size=(3, 3)))
    q = q * np.sign(np.diag(r))
    if np.linalg.det(q) < 0:
        q[:, 0] = -q[:, 0]
    return q


def rigid(R=None, t=(0, 0, 0)):
    T = np.eye(4)
    if R is not None:
        T[:3, :3] = R
    T[:3, 3] = t
    return T


def pack(meshes):
    """tri (F,3,3), tri_start (L+1) int64 of a list of (n_l,3,3) link meshes."""
    meshes = [np.asarray(m, np.float64).reshape(-1, 3, 3) for m in meshes]
    start = np.concatenate([[0], np.cumsum([len(m) for m in meshes])]).astype(np.int64)
    return np.concatenate(meshes), start


def all_pairs(L):
    return np.array([(i, j) for i in range(L) for j in range(i + 1, L)], np.int32).reshape(-1, 2)


# ------------------------------------------------------------------------------------------ the lattice cases of the contract
BASE = [[0, 0, 0], [4, 0, 0], [0, 4, 0]]
LATTICE = {                                                      # name -> (second triangle, colliding pairs)
    "pierce": ([[1, 1, -1], [1, 1, 1], [3, 3, 1]], 1),
    "vertex_on_face": ([[1, 1, 0], [1, 1, 2], [2, 1, 2]], 0),
    "coplanar": ([[1, 1, 0], [5, 1, 0], [1, 5, 0]], 0),
    "edge_through_vertex": ([[0, 0, -1], [0, 0, 1], [-1, -1, 0]], 0),
    "edge_through_edge": ([[2, 0, -1], [2, 0, 1], [2, -2, 0]], 0),
    "identical": (BASE, 0),
    "shared_edge": ([[0, 0, 0], [4, 0, 0], [0, 0, 4]], 0),
    "shared_vertex": ([[0, 0, 0], [-1, -1, 3], [-1, 1, 3]], 0),
    "point_on_face": ([[1, 1, 0]] * 3, 0),
    "collinear_piercing": ([[1, 1, -1], [1, 1, 1], [1, 1, 3]], 1),           # zero area, and its edge properly pierces the base
    "two_edges_pierce": ([[1, 1, -1], [2, 1, -1], [1.5, 1, 5]], 1),          # one pair, counted once
}


# ------------------------------------------------------------------------------------------ an independent test: OBB separating axes
def obb_separation(ha, Ra, ta, hb, Rb, tb):
    """Largest separation over the 15 candidate axes of two oriented boxes (half extents h, rotation R, centre t), each axis
    normalised: > 0 apart, < 0 overlapping.  Degenerate cross products (parallel edges) are skipped."""
    axes = [Ra[:, i] for i in range(3)] + [Rb[:, i] for i in range(3)]
    axes += [np.cross(Ra[:, i], Rb[:, j]) for i in range(3) for j in range(3)]
    d = np.asarray(tb, np.float64) - np.asarray(ta, np.float64)
    best = -np.inf
    for ax in axes:
        n = np.linalg.norm(ax)
        if n < 1e-9:
            continue
        ax = ax / n
        ra = sum(ha[i] * abs(ax @ Ra[:, i]) for i in range(3))
        rb = sum(hb[i] * abs(ax @ Rb[:, i]) for i in range(3))
        best = max(best, abs(ax @ d) - (ra + rb))
    return best


def obb_contains(ha, Ra, ta, hb, Rb, tb):
    """Box b lies wholly inside box a (all eight corners)."""
    corners = np.array([[x, y, z] for x in (-1, 1) for y in (-1, 1) for z in (-1, 1)]) * hb @ Rb.T + tb
    local = (corners - ta) @ Ra
    return bool((np.abs(local) <= np.asarray(ha)).all())


def random_box_pairs(n=400, seed=0):
    """The issue's box pairs: half extents U(0.05,0.3), random rotations, second box offset by U(-0.35,0.35)^3."""
    rng = np.random.default_rng(seed)
    out = []
    for _ in range(n):
        ha, hb = rng.uniform(0.05, 0.3, 3), rng.uniform(0.05, 0.3, 3)
        Ra, Rb = random_rotation(rng), random_rotation(rng)
        out.append((ha, Ra, np.zeros(3), hb, Rb, rng.uniform(-0.35, 0.35, 3)))
    return out


# ------------------------------------------------------------------------------------------ the toy robot
def toy(tmp, **env_kw):
    from _toy_urdf import write_toy_robot
    from autourdf_amd.sim_data import SimEnv
    path, _, _ = write_toy_robot(str(tmp))
    return SimEnv(path, dof=3, radius=1.2, num_cameras=3, **env_kw)


def toy_contacts(env, q):
    """[(link_a, link_b, count, tri_a, tri_b)] of the restatement for joint positions {name: value}."""
    r = env.robot
    pairs = r.collision_pairs()
    count, first, _ = mesh_collide(r.tri, r.tri_start, r.fk(q, env.base), pairs)
    return [(r.links[pairs[m, 0]], r.links[pairs[m, 1]], int(count[0, m]), int(first[0, m, 0]), int(first[0, m, 1]))
            for m in np.flatnonzero(count[0])]


# ------------------------------------------------------------------------------------------ scenes of the GPU tests
SIZES = (1, 63, 64, 65, 255, 256, 257, 552, 12, 0)               # one below, at and one above a wave (64) and a tile (256)


def sizes_scene(P=2, seed=7):
    """Links of SIZES triangles -- one large triangle, sphere caps of radius 0.1, a full sphere, a box, an empty link -- in P
    sets of random poses close enough for some pairs to intersect and some not; all pairs."""
    rng = np.random.default_rng(seed)
    meshes = []
    for n in SIZES:
        if n == 1:
            meshes.append(np.array([[[-0.15, -0.1, 0.0], [0.15, -0.1, 0.0], [0.0, 0.2, 0.0]]]))
        elif n == 12:
            meshes.append(box_mesh(0.06, 0.08, 0.1))
        else:
            meshes.append(uv_sphere(0.1, n=n))
    tri, start = pack(meshes)
    link_T = np.array([[rigid(random_rotation(rng), rng.uniform(-0.09, 0.09, 3)) for _ in SIZES] for _ in range(P)])
    return tri, start, link_T, all_pairs(len(SIZES))


def long_scene():
    """A link of 33 000 triangles -- 129 tiles, one more than the pair kernel's grid is wide, so its blocks take a second trip --
    crossed by a sphere of 552 and a box, and a far sphere; pairs in both orders."""
    big = uv_sphere(0.3, seg=150, rings=111)
    assert len(big) == 33000
    tri, start = pack([big, uv_sphere(0.1), box_mesh(0.05, 0.05, 0.05), uv_sphere(0.1)])
    link_T = np.array([rigid(None, (0, 0, 0)), rigid(None, (0.05, 0.02, -0.29)), rigid(None, (-0.3, 0.0, 0.01)), rigid(None, (1.0, 1.0, 1.0))])
    return tri, start, link_T, np.array([[0, 1], [1, 0], [0, 2], [2, 0], [0, 3], [1, 2]], np.int32)
