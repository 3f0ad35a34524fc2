"""Time the mesh-cover entry (creg_mesh_cover_f64) on the GPU, in the manner of tools/time_point_mesh.py.  Event-timed back-to-back
calls on device inputs built once:

* the toy robot of the tests, the toy robot subdivided to max_edge = 0.02 (compute_joints.subdivide_mesh) and the synthetic robot of
  tools/time_collide.py (12 links x 20 000 triangles), each at P = 10 poses x 5000 points sampled on the posed surface by area with
  the generator's per-point noise N(0, 0.0005);
* at every d_max of --d_max (default 0.01, inf): the whole entry (pose pass, tile-box pass, cover pass) on the points as sampled and
  on the points in the wrapper's Morton order with their rows as labels, the wrapper ops.mesh_cover with sort=True (the key, the
  sort and the gather included), creg_point_mesh_f64 on the same Morton-ordered input in the same run, and the point-triangle terms
  the call covers per second (points x triangles of their pose);
* the yardstick, timed the same way on the same input: a chunked torch restatement -- the posed triangles, their boxes, the gate
  matrix in chunks of --chunk_terms, pt_tri2 on the contributing terms (on all of them at d_max = inf), a scatter-min over the
  triangles -- and the largest difference between its distances and the kernel's.  It is skipped for a case whose covered terms
  exceed --torch_max_terms and the line says so.

Not measured here: hardware counters, and the share of (block, tile) visits the tile-box test rejects.

Warm-up: every shape runs once before its window; a window holds at least --min_ms of work; each figure is the median of
--repeats windows with the spread beside it.

    python tools/time_mesh_cover.py [--cases toy toy_subdivided synthetic] [--d_max 0.01 inf] [--repeats 5] [--min_ms 200]
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
from autourdf_amd.compute_joints import subdivide_mesh  # noqa: E402
from autourdf_amd.sim_data import SimEnv  # noqa: E402
from _toy_urdf import write_toy_robot  # noqa: E402
from time_clearance import t_pt_tri2  # noqa: E402
from time_collide import event_ms, synthetic_robot  # noqa: E402
from time_point_mesh import sample_points, t_pose  # noqa: E402

p = lambda t: ctypes.c_void_p(t.data_ptr()) if t is not None else None
INF = float("inf")


def torch_mesh_cover(tri, start, link_T, pts, cut, d_max, chunk_terms):
    """(dist2 (P,F), contributing terms) by the contract, in torch."""
    dmax2 = d_max * d_max
    F = len(tri)
    dist2 = torch.full((len(link_T), F), INF, dtype=torch.float64, device=pts.device)
    terms = 0
    for q, T in enumerate(link_T):
        W = t_pose(tri, start, T)
        lo, hi = W.amin(1), W.amax(1)
        a, b, c = (W[:, i].T.contiguous() for i in range(3))
        step = max(1, chunk_terms // max(1, F))
        for i0 in range(int(cut[q]), int(cut[q + 1]), step):
            x = pts[i0:min(i0 + step, int(cut[q + 1]))]
            if d_max == INF:
                terms += len(x) * F
                dist2[q] = torch.minimum(dist2[q], t_pt_tri2(x.T[:, :, None], a[:, None], b[:, None], c[:, None]).amin(0))
                continue
            g = torch.maximum(lo[None] - x[:, None], x[:, None] - hi[None]).clamp_min(0.0)
            near = ((g[..., 0] * g[..., 0] + g[..., 1] * g[..., 1]) + g[..., 2] * g[..., 2]) <= dmax2
            ii, ff = near.nonzero(as_tuple=True)
            terms += len(ii)
            if len(ii):
                dist2[q].scatter_reduce_(0, ff, t_pt_tri2(x[ii].T, a[:, ff], b[:, ff], c[:, ff]), "amin")
    return dist2, terms


def time_entry(name, tri, start, link_T, n_per_pose, args):
    L, dev = _lib.load(), _lib.device()
    d_tri, d_start, d_T = (torch.as_tensor(np.ascontiguousarray(a), device=dev) for a in (tri, start, link_T))
    F, (P, n_links) = len(tri), link_T.shape[:2]
    host_start = [int(s) for s in start]
    rng = torch.Generator(device=dev)
    rng.manual_seed(0)
    pts = sample_points(d_tri, host_start, d_T, n_per_pose, rng)
    N = len(pts)
    cut = np.arange(P + 1, dtype=np.int64) * n_per_pose
    d_cut = torch.as_tensor(cut, device=dev)
    order = ops._morton_order(pts, d_cut, P)
    sorted_pts, rows = pts[order].contiguous(), order.to(torch.int32)
    stream = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
    ws_bytes = max(L.creg_mesh_cover_workspace_bytes(F, n_links, P, N), L.creg_point_mesh_workspace_bytes(F, n_links, P, N))
    ws = torch.empty(ws_bytes // 8, dtype=torch.float64, device=dev)
    dist2 = torch.empty(P, F, dtype=torch.float64, device=dev)
    idx = torch.empty(P, F, dtype=torch.int32, device=dev)
    near = torch.empty(P, F, dtype=torch.int32, device=dev)
    pm_d2 = torch.empty(N, dtype=torch.float64, device=dev)
    pm_idx = torch.empty(N, dtype=torch.int32, device=dev)
    cover = lambda x, r, d: _lib.check(L.creg_mesh_cover_f64(p(d_tri), p(d_start), F, p(d_T), n_links, P, p(x), p(d_cut), p(r), N, d, p(dist2),
                                                             p(idx), p(near), None, p(ws), ws_bytes, stream), "creg_mesh_cover_f64")
    sibling = lambda d: _lib.check(L.creg_point_mesh_f64(p(d_tri), p(d_start), F, p(d_T), n_links, P, p(sorted_pts), p(d_cut), N, d,
                                                         p(pm_d2), p(pm_idx), None, p(ws), ws_bytes, stream), "creg_point_mesh_f64")
    covered = float(N) * F
    for d_max in args.d_max:
        raw = event_ms(lambda: cover(pts, None, d_max), args.repeats, args.min_ms)
        torch.cuda.synchronize()
        raw_out = (dist2.clone(), idx.clone(), near.clone())
        srt = event_ms(lambda: cover(sorted_pts, rows, d_max), args.repeats, args.min_ms)
        torch.cuda.synchronize()
        kernel_d2 = dist2.clone()
        same = all(torch.equal(x, y) for x, y in zip(raw_out, (dist2, idx, near)))
        wrap = event_ms(lambda: ops.mesh_cover(d_tri, d_start, d_T, pts, d_cut, d_max, sort=True), args.repeats, args.min_ms)
        pm = event_ms(lambda: sibling(d_max), args.repeats, args.min_ms)
        out = {"robot": name, "d_max": d_max, "triangles": F, "links": int(n_links), "poses": int(P), "points": N,
               "chunk_slots_per_pose": int((F >> 8) + n_links + 1), "workspace_MB": round(ws_bytes / 2 ** 20, 1),
               "entry_unsorted_ms": round(raw[0], 4), "entry_unsorted_ms_min_max": [round(raw[1], 4), round(raw[2], 4)],
               "entry_morton_ms": round(srt[0], 4), "entry_morton_ms_min_max": [round(srt[1], 4), round(srt[2], 4)],
               "morton_outputs_equal_unsorted": bool(same),
               "wrapper_sort_true_ms": round(wrap[0], 4), "wrapper_sort_true_ms_min_max": [round(wrap[1], 4), round(wrap[2], 4)],
               "point_mesh_morton_ms": round(pm[0], 4), "point_mesh_morton_ms_min_max": [round(pm[1], 4), round(pm[2], 4)],
               "triangles_beyond_d_max": int((kernel_d2 > d_max * d_max).sum()),
               "terms_covered": covered, "terms_covered_per_s_morton": covered / (srt[0] * 1e-3),
               "terms_covered_per_s_unsorted": covered / (raw[0] * 1e-3)}
        run = lambda: torch_mesh_cover(d_tri, host_start, d_T, pts, cut, d_max, args.chunk_terms)
        if covered > args.torch_max_terms:
            out["torch_chunked_ms"] = f"not measured: {covered:.3g} covered terms exceed --torch_max_terms"
        else:
            want, terms = run()
            t = event_ms(run, max(1, args.repeats // 2), 0.0)
            fin = torch.isfinite(want) & torch.isfinite(kernel_d2)
            out.update({"contributing_terms": float(terms), "contributing_terms_per_s_morton": terms / (srt[0] * 1e-3),
                        "gate_rejects_share_of_covered": round(1.0 - terms / covered, 6),
                        "torch_chunked_ms": round(t[0], 3), "torch_chunked_ms_min_max": [round(t[1], 3), round(t[2], 3)],
                        "torch_chunk_terms": args.chunk_terms,
                        "torch_inf_pattern_equal_kernel": bool((torch.isinf(want) == torch.isinf(kernel_d2)).all()),
                        "torch_max_abs_distance_difference": float((want[fin].sqrt() - kernel_d2[fin].sqrt()).abs().max()) if bool(fin.any()) else 0.0,
                        "speedup_vs_torch_morton": round(t[0] / srt[0], 2), "speedup_vs_torch_wrapper": round(t[0] / wrap[0], 2)})
        print(json.dumps(out), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--min_ms", type=float, default=200.0)
    ap.add_argument("--d_max", type=float, nargs="+", default=[0.01, INF])
    ap.add_argument("--points", type=int, default=5000, help="points per pose")
    ap.add_argument("--max_edge", type=float, default=0.02, help="of the subdivided toy robot")
    ap.add_argument("--chunk_terms", type=int, default=1 << 22, help="point-triangle terms of one chunk of the torch yardstick")
    ap.add_argument("--torch_max_terms", type=float, default=2e10, help="skip the torch yardstick above this many covered terms")
    ap.add_argument("--cases", nargs="+", default=["toy", "toy_subdivided", "synthetic"], choices=["toy", "toy_subdivided", "synthetic"])
    args = ap.parse_args()
    with tempfile.TemporaryDirectory() as d:
        if "toy" in args.cases or "toy_subdivided" in args.cases:
            toy, _, _ = write_toy_robot(d)
            env = SimEnv(toy, dof=3, radius=1.2, num_cameras=3)
            r = env.robot
            rows = sim_data.angle_list(10, 4, 3, env.joint_limits, np.array([0.9] * 3), 0)
            link_T = ops.urdf_fk(r.fk_table(), r.q_rows([env.set_joint_positions(c) for c in rows]), env.base).cpu().numpy()
            if "toy" in args.cases:
                time_entry("toy", r.tri, r.tri_start, link_T, args.points, args)
            if "toy_subdivided" in args.cases:
                tri, start, _ = subdivide_mesh(r.tri, r.tri_start, args.max_edge)
                time_entry(f"toy, max_edge {args.max_edge}", tri, start, link_T, args.points, args)
        if "synthetic" in args.cases:
            tri, start, link_T, _ = synthetic_robot()
            time_entry("12 spheres x 20000", tri, start, link_T, args.points, args)


if __name__ == "__main__":
    main()
