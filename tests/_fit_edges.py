"""Case builders and ordered restatements for the edge suite of creg_pose_fit_system_f64 (csrc/pose_fit.hip) and
creg_link_moments_f64 (csrc/link_moments.hip): tests/test_fit_edges_cpu.py checks them on the CPU, tests/test_gpu_fit_edges.py
compares the kernels with them bit for bit.

    ordered_system / ordered_moments   the header's "order" paragraph word for word, in float64: a pose's rows in tiles of 32 (64)
                 from its first row, every entry summed from 0.0 over the tile's rows ascending (pose fit: a row that does not
                 contribute adds its exact zeros; moments: the rows of other links are skipped), tile t into running sum t mod 4,
                 result (s0 + s1) + (s2 + s3).  The per-row terms are those of _pose_fit_ref.point_terms and
                 _link_moments_ref.row_terms, single IEEE operations in the header's order, so with the library built without
                 contraction the kernels must give exactly these bits.  pt_start is clamped as the header clamps it.
    chain_robot  a seeded serial chain of 59 links and 58 joints, every link a tetrahedron of 4 triangles, joint types from
                 {0, 1, 2, 3}; table_of_width cuts its joint table to the first J joints (D = 6 + J) and, at J = 58, gives two
                 joints an index outside [0, 59): the joints the forward kinematics skips.
    make_case    rows whose tri_idx the test chooses: a random triangle row each, the point a random point of the posed
                 triangle plus noise of 0.01 against d_max = 0.02, a NaN row and five rows without correspondence.
    layouts      A: every pose size around the tiles of 32 and 64 with empty poses first, last and in a run; B: 100 poses of one
                 row and one of 70; C: A with unowned rows in front and behind; D: three poses of 6, 7 and 8 tiles of 64 -- in A
                 no pose reaches the moments' main loop AND a tail of two or three tiles, and without both a tail tile added
                 into the wrong running sum gives the same bits.
    border_case, gate_case, zero_gate_case, last_link_case   the small table and link edges.

No input lies outside the header's contract: pt_start and tri_start never decrease, and values out of range stand only where the
header clamps them (the ends of pt_start and tri_start) or reads them as "no correspondence" (tri_idx)."""
import numpy as np

import _link_moments_ref as lm
import _point_mesh_ref as pref
import _pose_fit_ref as pf

PF_TILE, LM_TILE = 32, 64
N_LINKS, N_JOINTS, TRI_PER_LINK = 59, 58, 4
N_TRI = N_LINKS * TRI_PER_LINK
SKIPPED = (1, 3)                                                 # joints of the J = 58 table with an index outside [0, 59)
HIGH_BIT = 40                                                    # the chain bit the C-ABI test clears; a revolute joint
D_MAX, NOISE = 0.02, 0.01
INT32_MIN, INT32_MAX = -2 ** 31, 2 ** 31 - 1

LAYOUT_A = (0, 1, 31, 32, 33, 0, 0, 63, 64, 65, 129, 161, 225, 289, 0)
PF_TILES_A = (0, 1, 1, 1, 2, 0, 0, 2, 2, 3, 5, 6, 8, 10, 0)
LM_TILES_A = (0, 1, 1, 1, 1, 0, 0, 1, 1, 2, 3, 3, 4, 5, 0)
LAYOUT_B = (1,) * 100 + (70,)
LAYOUT_D = (321, 385, 449)                                       # 6, 7 and 8 tiles of 64: the moments' main loop with a tail of 2, 3 and 0
LM_TILES_D, PF_TILES_D = (6, 7, 8), (11, 13, 15)
FRONT, BACK = 5, 7                                               # layout C's unowned rows
LOOSE_FIRST, LOOSE_LAST = -3, 9                                  # its second call: pt_start[0] = -3, pt_start[P] = n_pts + 9
POSE_FIT_WIDTHS = (0, 9, 10, 57, 58)                             # J; D = 6, 15, 16, 63, 64
MOMENT_WIDTHS = (1, 15, 16, 59)                                  # L


# ------------------------------------------------------------------------------------------ the order, restated
def pose_rows(pt_start, n_pts):
    """(s (P), e (P)): the header's clamping of a pose's rows -- s into [0, n_pts], e into [s, n_pts]."""
    cut = np.asarray(pt_start, np.int64)
    s = np.clip(cut[:-1], 0, n_pts)
    return s, np.maximum(np.clip(cut[1:], 0, n_pts), s)


def _tiles(n, tile):
    return (n + tile - 1) // tile


def ordered_sum(terms, tile):
    """terms (n, ...) -> the header's sum over the rows: explicit loops over tiles and rows, vectorised over the entries."""
    n, shape = len(terms), terms.shape[1:]
    s = [np.zeros(shape) for _ in range(4)]
    zero = np.zeros(shape)
    for t in range(_tiles(n, tile)):
        acc = np.zeros(shape)
        for row in range(t * tile, (t + 1) * tile):
            acc = acc + (terms[row] if row < n else zero)        # a row past the pose's end adds an exact zero
        s[t % 4] = s[t % 4] + acc
    return (s[0] + s[1]) + (s[2] + s[3])


def ordered_system(tri, tri_start, link_T, pts, pt_start, tri_idx, table, center, d_max, chain=None):
    """H (P,D,D), g (P,D), cost (P), n (P) int64 in the header's order, and ok / link / case per row of pts."""
    link_T, pts = np.asarray(link_T, np.float64), np.asarray(pts, np.float64).reshape(-1, 3)
    P, D, N = len(link_T), 6 + len(table["parent"]), len(pts)
    chain = pf.chains(table) if chain is None else [int(x) for x in chain]
    dmax2 = np.float64(d_max) * np.float64(d_max)
    first, last = pose_rows(pt_start, N)
    out = {"H": np.zeros((P, D, D)), "g": np.zeros((P, D)), "cost": np.zeros(P), "n": np.zeros(P, np.int64),
           "ok": np.zeros(N, bool), "link": np.full(N, -1), "case": np.zeros(N, int)}
    for p in range(P):
        s, e = int(first[p]), int(last[p])
        ok, link, case, r, _, Jm = pf.point_terms(tri, tri_start, link_T[p], pts[s:e], np.asarray(tri_idx)[s:e], table, chain,
                                                  np.asarray(center, np.float64)[p], dmax2)
        out["ok"][s:e], out["link"][s:e], out["case"][s:e] = ok, link, case
        with np.errstate(all="ignore"):
            tH = (Jm[:, :, None, 0] * Jm[:, None, :, 0] + Jm[:, :, None, 1] * Jm[:, None, :, 1]) + Jm[:, :, None, 2] * Jm[:, None, :, 2]
            tg = (Jm[:, :, 0] * r[:, None, 0] + Jm[:, :, 1] * r[:, None, 1]) + Jm[:, :, 2] * r[:, None, 2]
            tc = (r[:, 0] * r[:, 0] + r[:, 1] * r[:, 1]) + r[:, 2] * r[:, 2]
        terms = np.concatenate([tH.reshape(e - s, D * D), tg, tc[:, None], ok.astype(np.float64)[:, None]], 1)
        total = ordered_sum(terms, PF_TILE)
        out["H"][p], out["g"][p], out["cost"][p] = total[:D * D].reshape(D, D), total[D * D:D * D + D], total[D * D + D]
        out["n"][p] = int(total[D * D + D + 1])
    return out


def ordered_moments(tri, tri_start, link_T, pts, pt_start, tri_idx, ref, d_max):
    """mom (P,L,16), cnt (P,L) int64 in the header's order, and ok / link / case per row of pts."""
    link_T, pts, ref = np.asarray(link_T, np.float64), np.asarray(pts, np.float64).reshape(-1, 3), np.asarray(ref, np.float64)
    P, L, N = len(link_T), link_T.shape[1], len(pts)
    table, chain = lm._no_joints(L), [0] * L
    dmax2 = np.float64(d_max) * np.float64(d_max)
    first, last = pose_rows(pt_start, N)
    out = {"mom": np.zeros((P, L, 16)), "cnt": np.zeros((P, L), np.int64), "ok": np.zeros(N, bool), "link": np.full(N, -1),
           "case": np.zeros(N, int)}
    for p in range(P):
        s, e = int(first[p]), int(last[p])
        ok, link, case, r, c, _ = pf.point_terms(tri, tri_start, link_T[p], pts[s:e], np.asarray(tri_idx)[s:e], table, chain, np.zeros(3), dmax2)
        out["ok"][s:e], out["link"][s:e], out["case"][s:e] = ok, link, case
        n = e - s
        terms = np.concatenate([lm.row_terms(r, c, ref[p][np.where(ok, link, 0)]), np.ones((n, 1))], 1)
        sums = [np.zeros((L, 17)) for _ in range(4)]
        for t in range(_tiles(n, LM_TILE)):
            acc = np.zeros((L, 17))
            for row in range(t * LM_TILE, min((t + 1) * LM_TILE, n)):
                if ok[row]:                                      # the rows of other links, and rows that do not contribute, are skipped
                    acc[link[row]] = acc[link[row]] + terms[row]
            sums[t % 4] = sums[t % 4] + acc
        total = (sums[0] + sums[1]) + (sums[2] + sums[3])
        out["mom"][p], out["cnt"][p] = total[:, :16], total[:, 16].astype(np.int64)
    return out


# ------------------------------------------------------------------------------------------ the chain robot
def chain_robot(seed=5):
    """59 links in a serial chain, joint j from link j to link j + 1.  Returns {"tri" (236,3,3), "tri_start" (60), "table"}."""
    rng = np.random.default_rng(seed)
    verts = rng.uniform(-0.03, 0.03, size=(N_LINKS, 4, 3))
    faces = np.array([(0, 1, 2), (0, 3, 1), (0, 2, 3), (1, 3, 2)])
    tri = np.ascontiguousarray(verts[:, faces].reshape(N_TRI, 3, 3))
    kinds = rng.integers(0, 4, size=N_JOINTS).astype(np.int32)
    kinds[[SKIPPED[0], SKIPPED[1], HIGH_BIT, HIGH_BIT + 1]] = (1, 2, 1, 2)   # the skipped joints would move points if they were not skipped
    origin = np.stack([pf.rigid_about(rng, rng.uniform(0.2, 3.0), 0.05) for _ in range(N_JOINTS)])
    axis = rng.normal(size=(N_JOINTS, 3))
    axis /= np.linalg.norm(axis, axis=1, keepdims=True)
    table = {"parent": np.arange(N_JOINTS, dtype=np.int32), "child": np.arange(1, N_LINKS, dtype=np.int32), "type": kinds,
             "origin": origin, "axis": axis, "names": [f"j{j}" for j in range(N_JOINTS)], "root": 0, "n_links": N_LINKS}
    return {"tri": tri, "tri_start": TRI_PER_LINK * np.arange(N_LINKS + 1, dtype=np.int64), "table": table}


def table_of_width(robot, J):
    """The first J joints with n_links kept at 59 (a fresh dict: ops.pose_fit_system keeps its upload in the dict it is given).
    At J = 58 joint 1 gets parent -1 and joint 3 child 59: skipped joints, no chain bit, frames of zeros."""
    full = robot["table"]
    table = {k: np.array(full[k][:J]) for k in ("parent", "child", "type", "origin", "axis")}
    table.update(names=list(full["names"][:J]), root=0, n_links=N_LINKS)
    if J == N_JOINTS:
        table["parent"][SKIPPED[0]] = -1
        table["child"][SKIPPED[1]] = N_LINKS
    return table


def link_states(robot, count=15, seed=6):
    """(count,59,4,4) link poses: _pose_fit_ref.fk of the full table at random joint values under a random base pose."""
    rng = np.random.default_rng(seed)
    table = robot["table"]
    scale = np.where(np.asarray(table["type"]) == 2, 0.05, 1.0)
    return np.stack([pf.fk(table, rng.uniform(-1.0, 1.0, size=N_JOINTS) * scale, pf.rigid_about(rng, 0.5, 0.2)) for _ in range(count)])


def _rows_near(rng, W, n):
    """n rows: a random triangle row of the posed mesh W (F,3,3) each, a random point of it plus noise."""
    f = rng.integers(0, len(W), size=n)
    u, v = rng.random(n), rng.random(n)
    su = np.sqrt(u)[:, None]
    x = W[f, 0] * (1 - su) + W[f, 1] * (su * (1 - v[:, None])) + W[f, 2] * (su * v[:, None])
    return x + rng.normal(scale=NOISE, size=(n, 3)), f.astype(np.int32)


def make_case(robot, sizes, seed, front=0, back=0):
    """One call's host arrays: len(sizes) poses of those row counts (pose p under link state p mod 15), ``front`` unowned rows
    before the first pose's and ``back`` after the last's (valid tri_idx, finite points).  The largest pose carries, from its row
    3 on, tri_idx -1, F, F + 1, INT32_MIN and INT32_MAX, and a NaN point at its row 40."""
    rng = np.random.default_rng(seed)
    states = link_states(robot)
    W = [pref.posed_mesh(robot["tri"], robot["tri_start"], T) for T in states]
    P = len(sizes)
    parts = [_rows_near(rng, W[0], front)] + [_rows_near(rng, W[p % len(W)], n) for p, n in enumerate(sizes)] \
        + [_rows_near(rng, W[(P - 1) % len(W)], back)]
    pts, idx = np.concatenate([x for x, _ in parts]), np.concatenate([f for _, f in parts])
    cut = (front + np.concatenate([[0], np.cumsum(sizes)])).astype(np.int64)
    big = int(np.argmax(sizes))
    assert sizes[big] >= 64
    bad = cut[big] + 3 + np.arange(5)
    idx[bad] = (-1, N_TRI, N_TRI + 1, INT32_MIN, INT32_MAX)
    pts[cut[big] + 40, 0] = np.nan
    center = rng.normal(scale=0.1, size=(P, 3))
    return {"tri": robot["tri"], "tri_start": robot["tri_start"], "link_T": np.ascontiguousarray(states[np.arange(P) % len(states)]),
            "pts": pts, "pt_start": cut, "tri_idx": idx, "center": center, "ref": center[:, None, :] + rng.normal(scale=0.05, size=(P, N_LINKS, 3)),
            "d_max": D_MAX, "bad_rows": bad, "nan_row": int(cut[big] + 40)}


def layout(robot, name):
    """Layout "A", "B", "C" or "D" as a case of make_case."""
    if name == "A":
        return make_case(robot, LAYOUT_A, 101)
    if name == "B":
        return make_case(robot, LAYOUT_B, 102)
    if name == "D":
        return make_case(robot, LAYOUT_D, 104)
    return make_case(robot, LAYOUT_A, 103, FRONT, BACK)


def loose_ends(case):
    """The case with pt_start[0] = -3 and pt_start[P] = n_pts + 9: the header clamps them, so pose 0 owns the rows from 0 and the
    last pose the rows up to n_pts."""
    cut = case["pt_start"].copy()
    cut[0], cut[-1] = LOOSE_FIRST, len(case["pts"]) + LOOSE_LAST
    return dict(case, pt_start=cut)


def one_pose(case, p):
    """Pose p of the case alone in a call, its rows from 0."""
    s, e = (int(x[p]) for x in pose_rows(case["pt_start"], len(case["pts"])))
    return dict(case, link_T=np.ascontiguousarray(case["link_T"][p:p + 1]), pts=np.ascontiguousarray(case["pts"][s:e]),
                tri_idx=np.ascontiguousarray(case["tri_idx"][s:e]), pt_start=np.array([0, e - s], np.int64),
                center=np.ascontiguousarray(case["center"][p:p + 1]), ref=np.ascontiguousarray(case["ref"][p:p + 1]))


def cut_links(case, L):
    """The first L links of the chain, tri cut to match: a tri_idx at or above 4 L now means no correspondence."""
    return dict(case, tri=np.ascontiguousarray(case["tri"][:TRI_PER_LINK * L]), tri_start=np.ascontiguousarray(case["tri_start"][:L + 1]),
                link_T=np.ascontiguousarray(case["link_T"][:, :L]), ref=np.ascontiguousarray(case["ref"][:, :L]))


def system_of(case, table, ordered=True, chain=None):
    args = (case["tri"], case["tri_start"], case["link_T"], case["pts"])
    if ordered:
        return ordered_system(*args, case["pt_start"], case["tri_idx"], table, case["center"], case["d_max"], chain)
    cut = np.concatenate([pose_rows(case["pt_start"], len(case["pts"]))[0], pose_rows(case["pt_start"], len(case["pts"]))[1][-1:]])
    return pf.system(*args, cut, case["tri_idx"], table, case["center"], case["d_max"], chain)


def moments_of(case, ordered=True):
    args = (case["tri"], case["tri_start"], case["link_T"], case["pts"])
    if ordered:
        return ordered_moments(*args, case["pt_start"], case["tri_idx"], case["ref"], case["d_max"])
    cut = np.concatenate([pose_rows(case["pt_start"], len(case["pts"]))[0], pose_rows(case["pt_start"], len(case["pts"]))[1][-1:]])
    return lm.moments(*args, cut, case["tri_idx"], case["ref"], case["d_max"])


# ------------------------------------------------------------------------------------------ table and link edges
BORDER_F = 16
BORDER_START = (-5, 4, 4, 4, 12, BORDER_F + 7)                   # clamped: 0 4 4 4 12 16 -- links 1 and 2 are empty and share a start
BORDER_FORCED = (0, 3, 4, 11, 12, 15)                            # the first and last row of links 0, 3 and 4
BORDER_BAD = (-1, BORDER_F, BORDER_F + 1, INT32_MIN, INT32_MAX)


def border_case(seed=7, bad=False):
    """One pose of five links over 16 random triangles, every link under its own pose, d_max = inf, 40 rows in two tiles of 32:
    rows 0 .. 5 at the forced triangles, the rest at random ones; with ``bad`` rows 8 .. 12 carry the five values that mean no
    correspondence.  Every other row contributes."""
    rng = np.random.default_rng(seed)
    tri = rng.normal(size=(BORDER_F, 3, 3))
    link_T = np.stack([pf.rigid_about(rng, rng.uniform(0.2, 3.0), 0.5) for _ in range(5)])[None]
    n = 40
    idx = rng.integers(0, BORDER_F, size=n).astype(np.int32)
    idx[:6] = BORDER_FORCED
    if bad:
        idx[8:13] = BORDER_BAD
    center = rng.normal(size=(1, 3))
    return {"tri": tri, "tri_start": np.array(BORDER_START, np.int64), "link_T": link_T, "pts": rng.normal(size=(n, 3)),
            "pt_start": np.array([0, n], np.int64), "tri_idx": idx, "center": center, "ref": center[:, None, :] + rng.normal(size=(1, 5, 3)),
            "d_max": np.inf}


def border_links(idx):
    """The link of each valid row of border_case, counted by hand from the clamped starts 0 4 4 4 12 16."""
    return [0 if f < 4 else 3 if f < 12 else 4 for f in idx if 0 <= f < BORDER_F]


def _unit_case(tri, pts, poses, d_max):
    n = len(pts)
    return {"tri": np.array(tri, np.float64).reshape(1, 3, 3), "tri_start": np.array([0, 1], np.int64),
            "link_T": np.tile(np.eye(4), (poses, 1, 1, 1)), "pts": np.array(pts, np.float64), "pt_start": np.arange(poses + 1, dtype=np.int64) * (n // poses),
            "tri_idx": np.zeros(n, np.int32), "center": np.zeros((poses, 3)), "ref": np.zeros((poses, 1, 3)), "d_max": d_max}


GATE = 0.25


def gate_case(d_max):
    """A vertex at the origin and the point (-0.25, 0, 0) in its vertex region: r = (-0.25, 0, 0), dot(r, r) = 0.0625 exactly."""
    return _unit_case([(0, 0, 0), (1, 0, 0), (0, 1, 0)], [(-GATE, 0.0, 0.0)], 1, d_max)


def zero_gate_case():
    """d_max = 0, two poses of one row: a point exactly on vertex a (r = 0), and one 2^-30 off it in the vertex region."""
    a = np.array([0.5, 0.25, 0.125])
    return _unit_case([a, a + (1, 0, 0), a + (0, 1, 0)], [a, a - (2.0 ** -30, 0, 0)], 2, 0.0)


def last_link_case(robot, seed=9, n=48):
    """One pose, 48 rows on the last link's four triangles, d_max = inf: every row contributes and carries the whole chain."""
    rng = np.random.default_rng(seed)
    T = link_states(robot, 1, seed)
    W = pref.posed_mesh(robot["tri"], robot["tri_start"], T[0])
    x, f = _rows_near(rng, W[N_TRI - TRI_PER_LINK:], n)
    center = rng.normal(scale=0.1, size=(1, 3))
    return {"tri": robot["tri"], "tri_start": robot["tri_start"], "link_T": T, "pts": x, "pt_start": np.array([0, n], np.int64),
            "tri_idx": (f + N_TRI - TRI_PER_LINK).astype(np.int32), "center": center, "ref": np.tile(center[:, None, :], (1, N_LINKS, 1)),
            "d_max": np.inf}
