"""Time the link-moments entry (creg_link_moments_f64) on the GPU, in the manner of tools/time_pose_fit.py and at its two shapes.
Event-timed back-to-back calls on device inputs built once:

* the toy robot of the tests (5 links, 4 joints) and the synthetic robot of tools/time_collide.py (12 links x 20 000 triangles)
  with time_pose_fit's serial joint table, each at P = 10 poses x 5000 points sampled on the posed surface by area; the
  correspondences are those of ops.point_mesh_distance at d_max = inf, computed once, outside the timed window; the moments are
  taken about every pose's mean point;
* the entry alone (tiles, finishing pass), and the wrapper ops.link_moments with its allocations;
* ops.pose_fit_system on the same input (the per-pose system only; the moments serve any parameter count);
* the yardstick, timed the same way on the same device input: a torch restatement of the 16 sums -- the link of every row by
  searchsorted, the row's triangle gathered and posed, pt_tri_vec, the 16 terms elementwise and one index_add_ per output -- and
  the largest difference of its sums from the kernel's, relative to the largest entry;
* the assembly compute_joints.link_twists + twist_system on the kernel's moments, with the frame parameters (M = 6 + 5 J);
* for the toy robot, one whole SimEnv.refine_joints (wall clock, synchronised): 8 poses x --fit_points points, q0 = q*, the base
  free, --fit_iters steps.  The synthetic robot has no URDF file, so there is no whole refinement for it.

Warm-up: every shape runs once before its window; a window holds at least --min_ms of work; each figure is the median of
--repeats windows with the spread beside it.

    python tools/time_link_moments.py [--toy_only] [--repeats 5] [--min_ms 200] [--fit_iters 10]
"""
import argparse
import ctypes
import json
import os
import sys
import tempfile
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, os.path.join(ROOT, "tools"))
from autourdf_amd import _lib, ops, sim_data  # noqa: E402
from autourdf_amd.compute_joints import link_twists, twist_system  # noqa: E402
from autourdf_amd.sim_data import SimEnv  # noqa: E402
from _toy_urdf import write_toy_robot  # noqa: E402
from time_clearance import t_dot  # noqa: E402
from time_collide import event_ms, synthetic_robot  # noqa: E402
from time_point_mesh import sample_points  # noqa: E402
from time_pose_fit import serial_table, t_pt_tri_vec  # noqa: E402

p = lambda t: ctypes.c_void_p(t.data_ptr()) if t is not None else None
INF = float("inf")


def torch_moments(tri, start, link_T, pts, cut, idx, ref, d_max):
    """(mom (P,L,16), cnt (P,L)) by the contract, in torch: gathers, elementwise terms, one index_add_ per output."""
    P, L = link_T.shape[:2]
    F = len(tri)
    pose_of = torch.repeat_interleave(torch.arange(P, device=pts.device), cut[1:] - cut[:-1])
    f = idx.to(torch.int64)
    ok = ~torch.isnan(pts).any(1) & (f >= 0) & (f < F)
    fs = f.clamp(0, max(F - 1, 0))
    l = (torch.searchsorted(start[:-1].contiguous(), fs, right=True) - 1).clamp(0, L - 1)
    ok &= (fs >= start[l]) & (fs < start[l + 1])
    T = link_T[pose_of, l]
    v = tri[fs]
    W = ((T[:, None, :3, 0] * v[:, :, None, 0] + T[:, None, :3, 1] * v[:, :, None, 1]) + T[:, None, :3, 2] * v[:, :, None, 2]) + T[:, None, :3, 3]
    r = t_pt_tri_vec(pts.T, W[:, 0].T, W[:, 1].T, W[:, 2].T).T
    rr = t_dot(r.T, r.T)
    ok &= rr <= d_max * d_max
    d = (pts - r) - ref[pose_of, l]
    x, y, z = d[:, 0], d[:, 1], d[:, 2]
    terms = torch.stack([x * x, x * y, x * z, y * y, y * z, z * z, x, y, z, y * r[:, 2] - z * r[:, 1], z * r[:, 0] - x * r[:, 2],
                         x * r[:, 1] - y * r[:, 0], r[:, 0], r[:, 1], r[:, 2], rr], 1)
    terms = torch.where(ok[:, None], terms, torch.zeros_like(terms))
    slot = pose_of * L + l
    mom = torch.zeros(P * L, 16, dtype=torch.float64, device=pts.device).index_add_(0, slot, terms)
    cnt = torch.zeros(P * L, dtype=torch.int64, device=pts.device).index_add_(0, slot, ok.to(torch.int64))
    return mom.reshape(P, L, 16), cnt.reshape(P, L)


def time_entry(name, tri, start, link_T, table, n_per_pose, args):
    L, dev = _lib.load(), _lib.device()
    d_tri, d_start, d_T = (torch.as_tensor(np.ascontiguousarray(a), device=dev) for a in (tri, start, link_T))
    d_tri = d_tri.reshape(-1, 3, 3)
    F, (P, n_links) = len(tri), link_T.shape[:2]
    rng = torch.Generator(device=dev)
    rng.manual_seed(0)
    pts = sample_points(d_tri, [int(s) for s in start], d_T, n_per_pose, rng)
    N, J = len(pts), len(table["parent"])
    d_cut = torch.as_tensor(np.arange(P + 1, dtype=np.int64) * n_per_pose, device=dev)
    center = pts.reshape(P, n_per_pose, 3).mean(1).contiguous()
    ref = center[:, None, :].expand(P, n_links, 3).contiguous()
    _, idx, _ = ops.point_mesh_distance(d_tri, d_start, d_T, pts, d_cut, INF)
    stream = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
    ws_bytes = L.creg_link_moments_workspace_bytes(P, N, n_links)
    ws = torch.empty(ws_bytes // 8, dtype=torch.float64, device=dev)
    mom = torch.empty(P, n_links, 16, dtype=torch.float64, device=dev)
    cnt = torch.empty(P, n_links, dtype=torch.int64, device=dev)
    call = lambda: _lib.check(L.creg_link_moments_f64(p(d_tri), p(d_start), F, p(d_T), n_links, P, p(pts), p(d_cut), N, INF, p(idx), p(ref),
                                                      p(mom), p(cnt), p(ws), ws_bytes, stream), "creg_link_moments_f64")
    entry = event_ms(call, args.repeats, args.min_ms)
    wrap = event_ms(lambda: ops.link_moments(d_tri, d_start, d_T, pts, d_cut, idx, ref, INF), args.repeats, args.min_ms)
    pose_fit = event_ms(lambda: ops.pose_fit_system(d_tri, d_start, d_T, pts, d_cut, idx, table, center, INF), args.repeats, args.min_ms)
    run = lambda: torch_moments(d_tri, d_start, d_T, pts, d_cut, idx, ref, INF)
    want = run()
    t = event_ms(run, args.repeats, args.min_ms)
    q = torch.zeros(P, J, dtype=torch.float64, device=dev)
    assemble = event_ms(lambda: twist_system(mom, cnt, link_twists(table, d_T, q, center, ref)), args.repeats, args.min_ms)
    torch.cuda.synchronize()
    rel = lambda a, b: float((a - b).abs().max() / b.abs().max().clamp_min(1e-300))
    ms = lambda x: [round(x[0], 4), [round(x[1], 4), round(x[2], 4)]]
    out = {"robot": name, "triangles": F, "links": int(n_links), "joints": J, "poses": int(P), "points": N,
           "workspace_MB": round(ws_bytes / 2 ** 20, 2), "pose_fit_workspace_MB": round(L.creg_pose_fit_workspace_bytes(P, N, J) / 2 ** 20, 2),
           "entry_ms": ms(entry)[0], "entry_ms_min_max": ms(entry)[1], "wrapper_ms": ms(wrap)[0], "wrapper_ms_min_max": ms(wrap)[1],
           "pose_fit_system_ms": ms(pose_fit)[0], "pose_fit_system_ms_min_max": ms(pose_fit)[1],
           "torch_ms": ms(t)[0], "torch_ms_min_max": ms(t)[1], "torch_over_entry": round(t[0] / entry[0], 2),
           "assembly_ms": ms(assemble)[0], "assembly_ms_min_max": ms(assemble)[1], "assembly_columns": 6 + 5 * J,
           "contributing": int(cnt.sum()), "cnt_equal": bool((cnt == want[1]).all()), "max_rel_difference_mom": rel(mom, want[0])}
    print(json.dumps(out), flush=True)


def time_refine(env, args):
    r = env.robot
    dev = _lib.device()
    rng = torch.Generator(device=dev)
    rng.manual_seed(1)
    rows = sim_data.angle_list(8, 4, 3, env.joint_limits, np.array([0.9] * 3), 0)
    q = r.q_rows([env.set_joint_positions(c) for c in rows])
    link_T = ops.urdf_fk(r.fk_table(), q, env.base)
    d_tri = torch.as_tensor(np.ascontiguousarray(r.tri), device=dev).reshape(-1, 3, 3)
    pts = sample_points(d_tri, [int(s) for s in r.tri_start], link_T, args.fit_points, rng).cpu().numpy()
    clouds = list(pts.reshape(len(q), args.fit_points, 3))
    walls = []
    for _ in range(args.repeats + 1):                                         # the first run is the warm-up
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        fit = env.refine_joints(clouds, q, max_iter=args.fit_iters)
        torch.cuda.synchronize()
        walls.append((time.perf_counter() - t0) * 1e3)
    walls = walls[1:]
    print(json.dumps({"robot": "toy", "whole_refine_joints_ms": round(float(np.median(walls)), 2),
                      "whole_refine_joints_ms_min_max": [round(min(walls), 2), round(max(walls), 2)], "poses": len(q), "points": len(pts),
                      "max_iter": args.fit_iters, "steps_tried": int(fit["iterations"]), "rms_all_before": fit["rms_all_before"],
                      "rms_all_after": fit["rms_all_after"]}), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--min_ms", type=float, default=200.0)
    ap.add_argument("--points", type=int, default=5000, help="points per pose")
    ap.add_argument("--fit_points", type=int, default=400, help="points per pose of the whole refinement")
    ap.add_argument("--fit_iters", type=int, default=10)
    ap.add_argument("--toy_only", action="store_true", help="skip the synthetic robot")
    ap.add_argument("--synthetic_only", action="store_true", help="skip the toy robot")
    args = ap.parse_args()
    with tempfile.TemporaryDirectory() as d:
        if not args.synthetic_only:
            toy, _, _ = write_toy_robot(d)
            env = SimEnv(toy, dof=3, radius=1.2, num_cameras=3)
            r = env.robot
            rows = sim_data.angle_list(10, 4, 3, env.joint_limits, np.array([0.9] * 3), 0)
            q = r.q_rows([env.set_joint_positions(c) for c in rows])
            link_T = ops.urdf_fk(r.fk_table(), q, env.base).cpu().numpy()
            table = {k: v for k, v in r.fk_table().items() if not k.startswith("_dev")}
            time_entry("toy", r.tri, r.tri_start, link_T, table, args.points, args)
            time_refine(env, args)
        if not args.toy_only:
            tri, start, link_T, _ = synthetic_robot()
            time_entry("12 spheres x 20000", tri, start, link_T, serial_table(link_T), args.points, args)


if __name__ == "__main__":
    main()
