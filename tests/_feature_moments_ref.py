"""numpy restatement of the feature-moments contract (include/creg.h, creg_feature_moments_f64), written from the header on top of
_pose_fit_ref.point_terms (r, c, the link, the case) and _point_mesh_ref.pose (the posed vertices), of the unpacking and assembly
of compute_joints.twist_system(fmom=...), and of the two drivers with the feature curvature.

    projector    Pi of a contributing row from pt_tri_vec's case and the posed vertices, + - * / only:
                 1..3 I | 4..6 delta_ij - (e_i e_j) / ee, e = b - a, c - a, c - b, when ee > 0 | 7 (N_i N_j) / NN, N = (b - a) x (c - a),
                 when NN > 0 | else I
    columns      A_0..2 = e_k x d with their zeros, A_3..5 = e_k;  B_k[i] = dot(Pi_i, A_k);  term (a, b) = dot(A_a, B_b), a <= b
    sums         in np.longdouble, with sum |term| beside each; mom and cnt are _link_moments_ref's
    assembly     H = sum_l Tw^T M6 Tw with M6 unpacked from the 21 sums; g and the cost from mom, as _link_moments_ref.assemble

Elementwise numpy operations are single IEEE operations, so every term has the kernel's bits; only the order of the sums differs,
and the tests bound that by (2 n + 8) 2^-53 sum |term| as the link-moments test does.

The drivers are _pose_fit_ref.fit and _link_moments_ref.refine themselves, run with their system swapped for the feature one:
the iteration, the cost, the accept rule and the stops are not restated twice."""
import contextlib

import numpy as np

import _link_moments_ref as lm
import _point_mesh_ref as pref
import _pose_fit_ref as pf
from _clearance_ref import dot

LD = np.longdouble
EPS = lm.EPS
UPPER = [(a, b) for a in range(6) for b in range(a, 6)]          # the order of the 21 sums
ITERS = 12                                                       # the steps the drivers are allowed in the tests
_link_moments = lm.moments                                       # the 16 sums, also while ``refine`` below swaps lm.moments


# ------------------------------------------------------------------------------------------ the contract
def projectors(case, W):
    """Pi (n,3,3) of rows with pt_tri_vec's case (n) and posed vertices W (n,3,3) = a | b | c."""
    case, W = np.asarray(case), np.asarray(W, np.float64).reshape(-1, 3, 3)
    n = len(case)
    a, b, c = W[:, 0], W[:, 1], W[:, 2]
    u, v = b - a, c - a
    Pi = np.tile(np.eye(3), (n, 1, 1))
    with np.errstate(all="ignore"):
        e = np.where((case == 4)[:, None], u, np.where((case == 5)[:, None], v, c - b))
        ee = dot(e.T, e.T)
        N = np.stack([u[:, 1] * v[:, 2] - u[:, 2] * v[:, 1], u[:, 2] * v[:, 0] - u[:, 0] * v[:, 2], u[:, 0] * v[:, 1] - u[:, 1] * v[:, 0]], 1)
        NN = dot(N.T, N.T)
        edge = np.eye(3)[None] - (e[:, :, None] * e[:, None, :]) / ee[:, None, None]
        face = (N[:, :, None] * N[:, None, :]) / NN[:, None, None]
    on_edge, on_face = (case >= 4) & (case <= 6) & (ee > 0), (case == 7) & (NN > 0)
    Pi[on_edge], Pi[on_face] = edge[on_edge], face[on_face]
    return Pi


def columns(d):
    """A (n,6,3): the six twist columns of rows with d (n,3), zeros and signs as the header writes them."""
    zero, one = np.zeros(len(d)), np.ones(len(d))
    x, y, z = d[:, 0], d[:, 1], d[:, 2]
    return np.stack([np.stack([zero, -z, y], 1), np.stack([z, zero, -x], 1), np.stack([-y, x, zero], 1),
                     np.stack([one, zero, zero], 1), np.stack([zero, one, zero], 1), np.stack([zero, zero, one], 1)], 1)


def _dot(u, v):
    return (u[..., 0] * v[..., 0] + u[..., 1] * v[..., 1]) + u[..., 2] * v[..., 2]


def row_terms(c, rho, Pi):
    """(n,21) terms of rows with closest point c (n,3) about rho (n,3) and projector Pi (n,3,3)."""
    with np.errstate(all="ignore"):
        A = columns(c - rho)
        B = _dot(Pi[:, None, :, :], A[:, :, None, :])                            # B[n, k, i] = dot(Pi_i, A_k)
        return np.stack([_dot(A[:, a], B[:, b]) for a, b in UPPER], 1)


def posed_rows(tri, T, rows, link):
    """(n,3,3) posed vertices of triangle rows ``rows`` under the poses T (L,4,4) of their links: the posing stage's bits."""
    tri = np.asarray(tri, np.float64).reshape(-1, 3, 3)
    W = np.empty((len(rows), 3, 3))
    for k in np.unique(link):
        W[link == k] = pref.pose(tri[rows[link == k]], T[k])
    return W


def moments(tri, tri_start, link_T, pts, pt_start, tri_idx, ref, d_max):
    """_link_moments_ref.moments' dict (mom, mom_abs, cnt, ok, link, case, r, c) with fmom (P,L,21) the long-double sums rounded to
    float64, fmom_abs the sums of |term|, and Pi (N,3,3) per point (the identity where the row does not contribute)."""
    out = _link_moments(tri, tri_start, link_T, pts, pt_start, tri_idx, ref, d_max)
    link_T = np.asarray(link_T, np.float64)
    if link_T.ndim == 3:
        link_T = link_T[None]
    ref, idx = np.asarray(ref, np.float64), np.asarray(tri_idx, np.int64)
    P, L, N = len(link_T), link_T.shape[1], len(out["ok"])
    out.update(fmom=np.zeros((P, L, 21)), fmom_abs=np.zeros((P, L, 21)), Pi=np.tile(np.eye(3), (N, 1, 1)))
    for p in range(P):
        s, e = int(pt_start[p]), int(pt_start[p + 1])
        at = s + np.flatnonzero(out["ok"][s:e])
        if len(at) == 0:
            continue
        link = out["link"][at]
        Pi = projectors(out["case"][at], posed_rows(tri, link_T[p], idx[at], link))
        out["Pi"][at] = Pi
        t = row_terms(out["c"][at], ref[p][link], Pi)
        for l in range(L):
            out["fmom"][p, l], out["fmom_abs"][p, l] = t[link == l].astype(LD).sum(0), np.abs(t[link == l]).astype(LD).sum(0)
    return out


# ------------------------------------------------------------------------------------------ unpacking and assembly
def unpack(fmom):
    """M6 (6,6) from its upper triangle (21), row-major over a <= b."""
    M = np.zeros((6, 6))
    for k, (a, b) in enumerate(UPPER):
        M[a, b] = M[b, a] = fmom[k]
    return M


def assemble(mom, cnt, fmom, Tw):
    """(H (M,M), g (M), cost) of one pose from mom (L,16), cnt (L), fmom (L,21) and Tw (L,6,M): the curvature from fmom, g and the
    cost from mom."""
    _, g, cost = lm.assemble(mom, cnt, Tw)
    H = np.zeros((Tw.shape[2],) * 2)
    for l in range(len(mom)):
        H += Tw[l].T @ unpack(fmom[l]) @ Tw[l]
    return H, g, cost


def system(tri, tri_start, link_T, pts, pt_start, tri_idx, table, center, d_max, chain=None):
    """What _pose_fit_ref.system returns for the drivers -- H (P,D,D) and g (P,D) -- with H = sum J^T Pi J: the feature moments
    about center_p under the pose-only twists."""
    link_T = np.asarray(link_T, np.float64)
    if link_T.ndim == 3:
        link_T = link_T[None]
    P, L, J = len(link_T), link_T.shape[1], len(table["parent"])
    chain = pf.chains(table) if chain is None else chain
    center = np.asarray(center, np.float64).reshape(P, 3)
    ref = np.broadcast_to(center[:, None, :], (P, L, 3))
    m = moments(tri, tri_start, link_T, pts, pt_start, tri_idx, ref, d_max)
    out = {"H": np.zeros((P, 6 + J, 6 + J)), "g": np.zeros((P, 6 + J)), "moments": m}
    for p in range(P):
        Tw = lm.twists(table, chain, link_T[p], np.zeros(J), center[p], ref[p])[:, :, :6 + J]
        out["H"][p], out["g"][p], _ = assemble(m["mom"][p], m["cnt"][p], m["fmom"][p], Tw)
    return out


# ------------------------------------------------------------------------------------------ the drivers
@contextlib.contextmanager
def _swapped(module, **names):
    old = {k: getattr(module, k) for k in names}
    for k, v in names.items():
        setattr(module, k, v)
    try:
        yield
    finally:
        for k, v in old.items():
            setattr(module, k, v)


def fit(*args, **kwargs):
    """_pose_fit_ref.fit with the feature system."""
    with _swapped(pf, system=system):
        return pf.fit(*args, **kwargs)


def _moments_with_fmom(*args):
    m = moments(*args)
    return dict(m, mom=np.concatenate([m["mom"], m["fmom"]], 2))                 # the driver hands mom[p] to moment_matrix below


def _feature_matrix(mom, cnt, absolute=False):
    return unpack(mom[16:37]), np.asarray(mom[9:15], np.float64)


def refine(*args, **kwargs):
    """_link_moments_ref.refine with the feature system: its moments carry the 21 sums behind the 16, and its 6 x 6 matrix is
    unpacked from them."""
    with _swapped(lm, moments=_moments_with_fmom, moment_matrix=_feature_matrix):
        return lm.refine(*args, **kwargs)


_RUNS = {}


def driver_run(robot, which, metric):
    """The restatement driver on pf.driver_case (``which`` = "fit") or lm.refine_case ("refine") of the toy robot at ``metric``,
    ITERS steps allowed, d_max = inf, the base locked -> (case, the driver's dict).  Computed once per session (the toy robot is
    the same wherever it was written) and shared by the CPU and the GPU tests; nobody changes the result."""
    key = (which, metric)
    if key not in _RUNS:
        if which == "fit":
            c = pf.driver_case(robot)
            args = (robot.tri, robot.tri_start, c["table"], c["clouds"], c["q0"], None, np.inf, ITERS, False, c["lock"])
            run = fit if metric == "feature" else pf.fit
        else:
            c = lm.refine_case(robot)
            args = (robot.tri, robot.tri_start, c["table"], c["clouds"], c["q0"], None, np.inf, ITERS, False, c["lock"], c["lock_frames"])
            run = refine if metric == "feature" else lm.refine
        _RUNS[key] = (c, run(*args))
    return _RUNS[key]


def driver_runs(robot):
    """{"fit": (case, point run, feature run), "refine": (case, point run, feature run)} of ``driver_run``."""
    return {w: (driver_run(robot, w, "point")[0], driver_run(robot, w, "point")[1], driver_run(robot, w, "feature")[1]) for w in ("fit", "refine")}


# ------------------------------------------------------------------------------------------ degenerate triangles
def degenerate_case():
    """One pose, two links under their own rigid poses, d_max = inf, tri_idx chosen by the test (the rows' "nearest" triangle):
    link 0 owns a proper triangle (row 0); link 1 a collinear one (row 1: c on the line ab, beyond b), a coincident one (row 2:
    a = b = c) and one with a = b and c apart (row 3).  A vertex is posed by one formula, so equal vertices stay equal in every bit
    under any pose.  Points: three off the proper triangle, four around the collinear one (off its middle, beyond each end, off the
    overlap), three about the coincident one, three about row 3.  Every zero-area row goes through pt_tri_vec's own guards first:
    the coincident row answers "vertex a" (Pi = I without a guard), the collinear row an edge of positive length, and row 3 the
    edge ab of length zero for a point that is not nearest a -- the ee > 0 guard, Pi = I.  The NN > 0 guard cannot be reached
    this way: pt_tri_vec sends a row to the face only with (va + vb) + vc > 0, which in exact arithmetic is N.N."""
    rng = np.random.default_rng(23)
    tri = np.array([[(0, 0, 0), (0.4, 0, 0), (0, 0.3, 0)],
                    [(0.1, 0.1, 0.1), (0.3, 0.2, 0.1), (0.5, 0.3, 0.1)],
                    [(0.2, -0.1, 0.3)] * 3,
                    [(-0.1, 0.2, 0.0), (-0.1, 0.2, 0.0), (0.2, 0.3, 0.1)]], np.float64)
    link_T = np.stack([pf.rigid_about(rng, 0.4, 0.1), pf.rigid_about(rng, 0.7, 0.1)])[None]
    local = np.array([(0.1, 0.1, 0.02), (0.5, -0.1, 0.01), (0.2, 0.2, -0.03),
                      (0.2, 0.17, 0.13), (0.0, 0.0, 0.1), (0.7, 0.42, 0.08), (0.4, 0.24, 0.12),
                      (0.21, -0.1, 0.3), (0.2, -0.12, 0.33), (0.2, -0.1, 0.3),
                      (0.05, 0.27, 0.03), (-0.2, 0.1, 0.0), (0.3, 0.35, 0.1)])
    idx = np.array([0, 0, 0, 1, 1, 1, 1, 2, 2, 2, 3, 3, 3], np.int32)
    owner = (idx > 0).astype(int)
    T = link_T[0][owner]
    pts = np.einsum("nij,nj->ni", T[:, :3, :3], local) + T[:, :3, 3]
    center = pts.mean(0)[None]
    return {"tri": tri, "tri_start": np.array([0, 1, 4], np.int64), "link_T": link_T, "pts": pts, "pt_start": np.array([0, len(pts)], np.int64),
            "tri_idx": idx, "ref": center[:, None, :] + rng.normal(scale=0.05, size=(1, 2, 3)), "d_max": np.inf}
