"""Time the link-clearance entry (creg_mesh_clearance_f64) on the GPU.  Event-timed back-to-back calls on device inputs built once:

* the toy robot of the tests at P = 10 poses, its 6 non-adjacent link pairs, and the synthetic robot of tools/time_collide.py
  (12 links x 20 000 triangles, UV spheres strung along a random walk, all 66 pairs, P = 10);
* at every margin d_max of --margins (default 0, 0.01, inf): the whole entry (pose pass + pair pass + finishing pass), the pose pass
  alone (the entry with n_pairs = 0), the link pairs within the margin and the triangle pairs the call covers per second;
* the yardsticks, timed the same way on the same input: creg_mesh_collide_f64 (the yes-or-no check the margin extends), and a
  chunked torch restatement of the clearance with the same link-box cull -- link boxes, the triangles of each link within d_max of
  the other's box, their gap matrix in chunks that fit --chunk_bytes, the 15 feature terms and the piercing predicate on the
  pairs that contribute.  The torch restatement is skipped for a case whose contributing triangle pairs exceed --torch_max_pairs
  (d_max = inf on the synthetic robot covers 2.6e11 of them) and the line says so.

Warm-up: every shape runs once before its window; a window holds at least --min_ms of work; each figure is the median of
--repeats windows with the spread beside it.

    python tools/time_clearance.py [--toy_only] [--margins 0 0.01 inf] [--repeats 5] [--min_ms 200]
"""
import argparse
import ctypes
import json
import os
import sys
import tempfile

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, os.path.join(ROOT, "tools"))
from autourdf_amd import _lib, ops, sim_data  # noqa: E402
from autourdf_amd.sim_data import SimEnv  # noqa: E402
from _toy_urdf import write_toy_robot  # noqa: E402
from time_collide import event_ms, synthetic_robot, t_pierces  # noqa: E402

p = lambda t: ctypes.c_void_p(t.data_ptr()) if t is not None else None
INF = float("inf")


# ------------------------------------------------------------------------------------------ the torch yardstick
def t_dot(u, v):
    return (u[0] * v[0] + u[1] * v[1]) + u[2] * v[2]


def t_clamp01(x):
    return x.clamp(0.0, 1.0)


def t_gap2(lo_a, hi_a, lo_b, hi_b):
    g = torch.maximum(lo_a - hi_b, lo_b - hi_a).clamp_min(0.0)
    return (g[..., 0] * g[..., 0] + g[..., 1] * g[..., 1]) + g[..., 2] * g[..., 2]


def t_pt_tri2(q, a, b, c):
    """include/creg.h's pt_tri2 on (3,n) operands."""
    ab, ac, ap, bp, cp = b - a, c - a, q - a, q - b, q - c
    d1, d2, d3, d4, d5, d6 = t_dot(ab, ap), t_dot(ac, ap), t_dot(ab, bp), t_dot(ac, bp), t_dot(ab, cp), t_dot(ac, cp)
    vc, vb, va = d1 * d4 - d3 * d2, d5 * d2 - d1 * d6, d3 * d6 - d5 * d4
    zero = torch.zeros_like(d1)
    s = (va + vb) + vc
    v, w = torch.where(s > 0, vb / s, zero), torch.where(s > 0, vc / s, zero)
    c6, den = (va <= 0) & (d4 - d3 >= 0) & (d5 - d6 >= 0), (d4 - d3) + (d5 - d6)
    w6 = torch.where(den > 0, (d4 - d3) / den, zero)
    v, w = torch.where(c6, 1.0 - w6, v), torch.where(c6, w6, w)
    c5, den = (vb <= 0) & (d2 >= 0) & (d6 <= 0), d2 - d6
    v, w = torch.where(c5, zero, v), torch.where(c5, torch.where(den > 0, d2 / den, zero), w)
    c4, den = (vc <= 0) & (d1 >= 0) & (d3 <= 0), d1 - d3
    v, w = torch.where(c4, torch.where(den > 0, d1 / den, zero), v), torch.where(c4, zero, w)
    x = q - ((a + ab * v) + ac * w)
    out = t_dot(x, x)
    out = torch.where((d6 >= 0) & (d5 <= d6), t_dot(cp, cp), out)
    out = torch.where((d3 >= 0) & (d4 <= d3), t_dot(bp, bp), out)
    return torch.where((d1 <= 0) & (d2 <= 0), t_dot(ap, ap), out)


def t_seg_seg2(p1, q1, p2, q2):
    """include/creg.h's seg_seg2 on (3,n) operands."""
    u, v, r = q1 - p1, q2 - p2, p1 - p2
    a, e, f, c, b = t_dot(u, u), t_dot(v, v), t_dot(v, r), t_dot(u, r), t_dot(u, v)
    zero, one = torch.zeros_like(a), torch.ones_like(a)
    den = a * e - b * b
    s = torch.where(den > 0, t_clamp01((b * f - c * e) / den), zero)
    t = (b * s + f) / e
    lo, hi = t < 0, t > 1
    s = torch.where(lo, t_clamp01((0.0 - c) / a), torch.where(hi, t_clamp01((b - c) / a), s))
    t = torch.where(lo, zero, torch.where(hi, one, t))
    c3 = e <= 0
    s, t = torch.where(c3, t_clamp01((0.0 - c) / a), s), torch.where(c3, zero, t)
    c2 = a <= 0
    s, t = torch.where(c2, zero, s), torch.where(c2, t_clamp01(f / e), t)
    c1 = (a <= 0) & (e <= 0)
    s, t = torch.where(c1, zero, s), torch.where(c1, zero, t)
    x = (p1 + u * s) - (p2 + v * t)
    return t_dot(x, x)


def t_pair_d2(a, b):
    """d2 of triangle pairs a, b (n,3,3)."""
    lo_a, hi_a, lo_b, hi_b = a.amin(1), a.amax(1), b.amin(1), b.amax(1)
    hit = torch.zeros(len(a), dtype=torch.bool, device=a.device)
    for E, T in ((a, b), (b, a)):
        for k in range(3):
            hit |= t_pierces(E[:, k], E[:, (k + 1) % 3], T[:, 0], T[:, 1], T[:, 2])
    hit &= ((lo_a <= hi_b) & (lo_b <= hi_a)).all(-1)
    av, bv = [a[:, i].T.contiguous() for i in range(3)], [b[:, i].T.contiguous() for i in range(3)]
    d = torch.full((len(a),), INF, dtype=a.dtype, device=a.device)
    for i in range(3):
        d = torch.minimum(d, t_pt_tri2(av[i], bv[0], bv[1], bv[2]))
        d = torch.minimum(d, t_pt_tri2(bv[i], av[0], av[1], av[2]))
    for i in range(3):
        for j in range(3):
            d = torch.minimum(d, t_seg_seg2(av[i], av[(i + 1) % 3], bv[j], bv[(j + 1) % 3]))
    return torch.where(hit, torch.zeros_like(d), d)


def torch_clearance(tri, start, link_T, pairs, d_max, chunk_bytes, max_pairs, count_only=False):
    """(dist2 (P,M), contributing triangle pairs) by the contract, in torch; None for dist2 when the contributing pairs exceed
    max_pairs (they are still counted) or with count_only."""
    P, L = link_T.shape[:2]
    dmax2 = d_max * d_max
    dist2 = torch.full((P, len(pairs)), INF, dtype=torch.float64, device=tri.device)
    tested, todo = 0, []
    for q in range(P):
        posed = []
        for l in range(L):
            v, T = tri[start[l]:start[l + 1]], link_T[q, l]
            posed.append(torch.stack([((T[i, 0] * v[..., 0] + T[i, 1] * v[..., 1]) + T[i, 2] * v[..., 2]) + T[i, 3] for i in range(3)], -1))
        lo, hi = [t.amin(1) for t in posed], [t.amax(1) for t in posed]
        for m, (la, lb) in enumerate(pairs):
            if not len(posed[la]) or not len(posed[lb]):
                continue
            box_a, box_b = (lo[la].amin(0), hi[la].amax(0)), (lo[lb].amin(0), hi[lb].amax(0))
            if not bool(t_gap2(*box_a, *box_b) <= dmax2):
                continue
            ka = (t_gap2(lo[la], hi[la], *box_b) <= dmax2).nonzero()[:, 0]
            kb = (t_gap2(lo[lb], hi[lb], *box_a) <= dmax2).nonzero()[:, 0]
            if not len(ka) or not len(kb):
                continue
            step = max(1, chunk_bytes // (8 * len(kb)))
            for a0 in range(0, len(ka), step):
                rows = ka[a0:a0 + step]
                near = t_gap2(lo[la][rows, None], hi[la][rows, None], lo[lb][kb][None], hi[lb][kb][None]) <= dmax2
                n = int(near.sum())
                tested += n
                if n == 0 or count_only or tested > max_pairs:
                    continue
                ia, ib = near.nonzero(as_tuple=True)
                block = max(1, chunk_bytes // (8 * 64))           # the feature terms hold some 60 temporaries per pair
                for k in range(0, n, block):
                    d = t_pair_d2(posed[la][rows[ia[k:k + block]]], posed[lb][kb[ib[k:k + block]]])
                    dist2[q, m] = torch.minimum(dist2[q, m], d.min())
    return (None if count_only or tested > max_pairs else dist2), tested


# ------------------------------------------------------------------------------------------ the kernel
def time_entry(name, tri, start, link_T, pairs, args):
    L, dev = _lib.load(), _lib.device()
    d_tri, d_start, d_T, d_pairs = (torch.as_tensor(np.ascontiguousarray(a), device=dev) for a in (tri, start, link_T, pairs))
    F, (P, n_links), M = len(tri), link_T.shape[:2], len(pairs)
    stream = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
    sizes = np.diff(start)
    covered = float(sum(int(sizes[a]) * int(sizes[b]) for a, b in pairs)) * P
    host_pairs = [tuple(int(x) for x in pr) for pr in pairs]
    host_start = [int(s) for s in start]
    # ---- the yes-or-no check on the same scene
    ws_c = torch.empty(L.creg_mesh_collide_workspace_bytes(F, n_links, P, M) // 8, dtype=torch.float64, device=dev)
    count = torch.empty(P, M, dtype=torch.int32, device=dev)
    first = torch.empty(P, M, 2, dtype=torch.int32, device=dev)
    collide = event_ms(lambda: _lib.check(L.creg_mesh_collide_f64(p(d_tri), p(d_start), F, p(d_T), n_links, P, p(d_pairs), M, p(count), p(first),
                                                                  None, p(ws_c), ws_c.numel() * 8, stream), "creg_mesh_collide_f64"),
                       args.repeats, args.min_ms)
    # ---- the clearance entry, margin by margin
    ws_bytes = L.creg_mesh_clearance_workspace_bytes(F, n_links, P, M)
    ws = torch.empty(ws_bytes // 8, dtype=torch.float64, device=dev)
    dist2 = torch.empty(P, M, dtype=torch.float64, device=dev)
    wit = torch.empty(P, M, 2, dtype=torch.int32, device=dev)
    call = lambda m, d: _lib.check(L.creg_mesh_clearance_f64(p(d_tri), p(d_start), F, p(d_T), n_links, P, p(d_pairs), m, d, p(dist2), p(wit), None,
                                                             p(ws), ws_bytes, stream), "creg_mesh_clearance_f64")
    pose = event_ms(lambda: call(0, 0.0), args.repeats, args.min_ms)
    for d_max in args.margins:
        whole = event_ms(lambda: call(M, d_max), args.repeats, args.min_ms)
        torch.cuda.synchronize()
        within = dist2 <= d_max * d_max
        out = {"robot": name, "d_max": d_max, "triangles": F, "links": int(n_links), "pairs": M, "poses": int(P),
               "workspace_MB": round(ws_bytes / 2 ** 20, 1), "pose_pass_ms": round(pose[0], 4),
               "whole_entry_ms": round(whole[0], 4), "whole_entry_ms_min_max": [round(whole[1], 4), round(whole[2], 4)],
               "pair_pass_ms": round(whole[0] - pose[0], 4), "link_pairs_within_margin": int(within.sum()),
               "link_pairs_at_zero": int((dist2 == 0).sum()), "colliding_link_pairs": int((count > 0).sum()),
               "triangle_pairs_covered": covered, "triangle_pairs_covered_per_s": covered / (whole[0] * 1e-3),
               "mesh_collide_ms": round(collide[0], 4), "mesh_collide_ms_min_max": [round(collide[1], 4), round(collide[2], 4)],
               "vs_mesh_collide": round(whole[0] / collide[0], 2)}
        run = lambda **kw: torch_clearance(d_tri, host_start, d_T, host_pairs, d_max, args.chunk_bytes, args.torch_max_pairs, **kw)
        tested = covered if d_max == INF else run(count_only=True)[1]    # every pair of two posed triangles contributes at +inf
        out.update({"contributing_triangle_pairs": tested, "contributing_pairs_per_s": tested / (whole[0] * 1e-3)})
        if tested > args.torch_max_pairs:
            out["torch_chunked_clearance_ms"] = f"not measured: {tested:.3g} contributing pairs exceed --torch_max_pairs"
        else:
            want, _ = run()
            t = event_ms(run, max(1, args.repeats // 2), 0.0)
            same = torch.isinf(want) == torch.isinf(dist2)
            fin = torch.isfinite(want) & torch.isfinite(dist2)
            out.update({"torch_chunked_clearance_ms": round(t[0], 3), "torch_chunked_clearance_ms_min_max": [round(t[1], 3), round(t[2], 3)],
                        "torch_chunk_bytes": args.chunk_bytes, "torch_inf_pattern_equal_kernel": bool(same.all()),
                        "torch_max_abs_distance_difference": float((want[fin].sqrt() - dist2[fin].sqrt()).abs().max()) if bool(fin.any()) else 0.0,
                        "speedup_vs_torch_clearance": round(t[0] / whole[0], 2)})
        print(json.dumps(out), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--min_ms", type=float, default=200.0)
    ap.add_argument("--margins", type=float, nargs="+", default=[0.0, 0.01, INF])
    ap.add_argument("--chunk_bytes", type=int, default=1 << 28, help="largest gap matrix of the torch yardstick")
    ap.add_argument("--torch_max_pairs", type=float, default=5e7, help="skip the torch yardstick above this many contributing triangle pairs")
    ap.add_argument("--toy_only", action="store_true", help="skip the synthetic robot")
    ap.add_argument("--synthetic_only", action="store_true", help="skip the toy robot")
    args = ap.parse_args()
    with tempfile.TemporaryDirectory() as d:
        if not args.synthetic_only:
            toy, _, _ = write_toy_robot(d)
            env = SimEnv(toy, dof=3, radius=1.2, num_cameras=3)
            r = env.robot
            rows = sim_data.angle_list(10, 4, 3, env.joint_limits, np.array([0.9] * 3), 0)
            link_T = ops.urdf_fk(r.fk_table(), r.q_rows([env.set_joint_positions(c) for c in rows]), env.base).cpu().numpy()
            time_entry("toy", r.tri, r.tri_start, link_T, r.collision_pairs(), args)
        if not args.toy_only:
            time_entry("12 spheres x 20000", *synthetic_robot(), args)


if __name__ == "__main__":
    main()
