"""Time the point-to-mesh entry (creg_point_mesh_f64) on the GPU.  Event-timed back-to-back calls on device inputs built once:

* the toy robot of the tests and the synthetic robot of tools/time_collide.py (12 links x 20 000 triangles, UV spheres strung along
  a random walk), each at P = 10 poses x 5000 points sampled on the posed surface by area, with the generator's per-point noise
  N(0, 0.0005) (the generator's per-frame translation is what cloud_fit takes out again, so it is not applied);
* at every d_max of --d_max (default 0.01, inf): the whole entry (pose pass + point pass) on the points as sampled and on the points in
  the wrapper's Morton order, the pose pass alone (the entry with n_pts = 0), the wrapper ops.point_mesh_distance with sort=True
  (the key, the sort, the gather and the scatter back included), the point-triangle terms the call covers per second (points x
  triangles of their pose) and the terms that contribute (box gate) per second;
* the yardstick, timed the same way on the same input: a chunked torch restatement -- the posed triangles, their boxes, the gate
  matrix in chunks of --chunk_terms, pt_tri2 on the contributing terms (on all of them at d_max = inf), a scatter-min -- and the largest
  difference between its distances and the kernel's.  It is skipped for a case whose covered terms exceed --torch_max_terms and the
  line says so.

Warm-up: every shape runs once before its window; a window holds at least --min_ms of work; each figure is the median of
--repeats windows with the spread beside it.

    python tools/time_point_mesh.py [--toy_only] [--d_max 0.01 inf] [--repeats 5] [--min_ms 200]
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
from time_clearance import t_pt_tri2  # noqa: E402
from time_collide import event_ms, synthetic_robot  # noqa: E402

p = lambda t: ctypes.c_void_p(t.data_ptr()) if t is not None else None
INF = float("inf")


def t_pose(tri, start, T):
    """(F,3,3) posed triangles of one pose, the header's vertex formula."""
    out = []
    for l in range(len(start) - 1):
        v, M = tri[start[l]:start[l + 1]], T[l]
        out.append(torch.stack([((M[i, 0] * v[..., 0] + M[i, 1] * v[..., 1]) + M[i, 2] * v[..., 2]) + M[i, 3] for i in range(3)], -1))
    return torch.cat(out)


def sample_points(tri, start, link_T, n, rng, noise=0.0005):
    """n points per pose on the posed surface, by area, plus N(0, noise) per coordinate -> pts (P*n,3) on the device."""
    out = []
    for T in link_T:
        W = t_pose(tri, start, T)
        area = torch.linalg.cross(W[:, 1] - W[:, 0], W[:, 2] - W[:, 0]).norm(dim=1)
        f = torch.multinomial(area / area.sum(), n, replacement=True, generator=rng)
        u = torch.rand(n, 2, dtype=torch.float64, device=W.device, generator=rng)
        s = u[:, :1].sqrt()
        x = W[f, 0] * (1 - s) + W[f, 1] * (s * (1 - u[:, 1:])) + W[f, 2] * (s * u[:, 1:])
        out.append(x + noise * torch.randn(n, 3, dtype=torch.float64, device=W.device, generator=rng))
    return torch.cat(out).contiguous()


def torch_point_mesh(tri, start, link_T, pts, cut, d_max, chunk_terms, count_only=False):
    """(dist2 (N), contributing terms) by the contract, in torch."""
    dmax2 = d_max * d_max
    dist2 = torch.full((len(pts),), INF, dtype=torch.float64, device=pts.device)
    terms = 0
    for q, T in enumerate(link_T):
        W = t_pose(tri, start, T)
        lo, hi = W.amin(1), W.amax(1)
        a, b, c = (W[:, i].T.contiguous() for i in range(3))
        step = max(1, chunk_terms // max(1, len(W)))
        for i0 in range(int(cut[q]), int(cut[q + 1]), step):
            x = pts[i0:min(i0 + step, int(cut[q + 1]))]
            if d_max == INF:
                terms += len(x) * len(W)
                if not count_only:
                    dist2[i0:i0 + len(x)] = t_pt_tri2(x.T[:, :, None], a[:, None], b[:, None], c[:, None]).amin(1)
                continue
            g = torch.maximum(lo[None] - x[:, None], x[:, None] - hi[None]).clamp_min(0.0)
            near = ((g[..., 0] * g[..., 0] + g[..., 1] * g[..., 1]) + g[..., 2] * g[..., 2]) <= dmax2
            ii, ff = near.nonzero(as_tuple=True)
            terms += len(ii)
            if len(ii) and not count_only:
                d = t_pt_tri2(x[ii].T, a[:, ff], b[:, ff], c[:, ff])
                dist2[i0:i0 + len(x)].scatter_reduce_(0, ii, d, "amin")
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
    sorted_pts = pts[order].contiguous()
    stream = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
    ws_bytes = L.creg_point_mesh_workspace_bytes(F, n_links, P, N)
    ws = torch.empty(ws_bytes // 8, dtype=torch.float64, device=dev)
    dist2 = torch.empty(N, dtype=torch.float64, device=dev)
    idx = torch.empty(N, dtype=torch.int32, device=dev)
    call = lambda x, n, d: _lib.check(L.creg_point_mesh_f64(p(d_tri), p(d_start), F, p(d_T), n_links, P, p(x), p(d_cut), n, d, p(dist2), p(idx),
                                                            None, p(ws), ws_bytes, stream), "creg_point_mesh_f64")
    pose = event_ms(lambda: call(None, 0, 0.0), args.repeats, args.min_ms)
    covered = float(N) * F
    for d_max in args.d_max:
        raw = event_ms(lambda: call(pts, N, d_max), args.repeats, args.min_ms)
        srt = event_ms(lambda: call(sorted_pts, N, d_max), args.repeats, args.min_ms)
        torch.cuda.synchronize()
        sorted_d2 = dist2.clone()
        wrap = event_ms(lambda: ops.point_mesh_distance(d_tri, d_start, d_T, pts, d_cut, d_max, sort=True), args.repeats, args.min_ms)
        kernel_d2 = torch.empty_like(sorted_d2).index_copy_(0, order, sorted_d2)
        out = {"robot": name, "d_max": d_max, "triangles": F, "links": int(n_links), "poses": int(P), "points": N,
               "workspace_MB": round(ws_bytes / 2 ** 20, 1), "pose_pass_ms": round(pose[0], 4),
               "entry_unsorted_ms": round(raw[0], 4), "entry_unsorted_ms_min_max": [round(raw[1], 4), round(raw[2], 4)],
               "entry_morton_ms": round(srt[0], 4), "entry_morton_ms_min_max": [round(srt[1], 4), round(srt[2], 4)],
               "wrapper_sort_true_ms": round(wrap[0], 4), "wrapper_sort_true_ms_min_max": [round(wrap[1], 4), round(wrap[2], 4)],
               "points_beyond_d_max": int((kernel_d2 > d_max * d_max).sum()),
               "terms_covered": covered, "terms_covered_per_s_morton": covered / (srt[0] * 1e-3),
               "terms_covered_per_s_unsorted": covered / (raw[0] * 1e-3)}
        run = lambda **kw: torch_point_mesh(d_tri, host_start, d_T, pts, cut, d_max, args.chunk_terms, **kw)
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
    ap.add_argument("--chunk_terms", type=int, default=1 << 22, help="point-triangle terms of one chunk of the torch yardstick")
    ap.add_argument("--torch_max_terms", type=float, default=2e10, help="skip the torch yardstick above this many covered terms")
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
            time_entry("toy", r.tri, r.tri_start, link_T, args.points, args)
        if not args.toy_only:
            tri, start, link_T, _ = synthetic_robot()
            time_entry("12 spheres x 20000", tri, start, link_T, args.points, args)


if __name__ == "__main__":
    main()
