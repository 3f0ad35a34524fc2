"""Time the link mesher on the GPU (DESIGN N4) at the README's two URDF-stage shapes -- K = 20 and K = 45 clusters in six
links, T = 10 steps, 400 points per cluster and frame -- and at one 100-step shape (K = 20): event-timed microseconds of
every entry point (back-to-back launches on prepared inputs, after a warm-up), of the two wrappers ops.statistical_outlier
and ops.voxel_mesh (which include their two host waits), and the wall time of link.link_mesh on a directory (PLY read, the
launches, STL write) around a device synchronise.  One JSON line per shape.

A link cloud here is what the stage produces: every cluster is a 2 cm Gaussian blob around its place on the link, seen in
T frames with 1 mm registration noise, float32-rounded.

    python tools/time_link_mesh.py [--reps 20] [--voxel_size 0.003]
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

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from autourdf_amd import _lib, link, ops  # noqa: E402

PTS, LINKS = 400, 6


def link_clouds(K, T, seed):
    rng = np.random.default_rng(seed)
    grp = np.sort(np.concatenate([np.arange(LINKS), rng.integers(0, LINKS, K - LINKS)]))
    cent = rng.uniform(-0.03, 0.03, (K, 3)) + np.array([0, 0, 0.06])
    clouds = []
    for l in range(LINKS):
        parts = [cent[k] + rng.normal(scale=0.02, size=(PTS, 3)) + rng.normal(scale=1e-3, size=3)
                 for _ in range(T) for k in np.flatnonzero(grp == l)]
        clouds.append(np.concatenate(parts).astype(np.float32).astype(np.float64))
    return clouds


def event_us(fn, reps):
    fn()
    torch.cuda.synchronize()
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(reps):
        fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) * 1000.0 / reps


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--voxel_size", type=float, default=0.003)
    ap.add_argument("--shapes", type=str, default="20x10,45x10,20x100")
    args = ap.parse_args()
    dev = torch.device("cuda")
    L_ = _lib.load()
    p = lambda t: ctypes.c_void_p(t.data_ptr())
    vs = args.voxel_size
    for shape in args.shapes.split(","):
        K, T = (int(x) for x in shape.split("x"))
        clouds = link_clouds(K, T, K + T)
        off_h = np.concatenate([[0], np.cumsum([len(c) for c in clouds])]).astype(np.int64)
        pts = torch.from_numpy(np.concatenate(clouds)).to(dev)
        off = torch.from_numpy(off_h).to(dev)
        n, L = len(pts), LINKS
        st = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
        reps = args.reps if n < 500000 else max(3, args.reps // 5)
        # prepared inputs of every entry point, as ops.voxel_mesh builds them
        avg = torch.empty(n, dtype=torch.float64, device=dev)
        thr = torch.empty(L, dtype=torch.float64, device=dev)
        keep = torch.empty(n, dtype=torch.uint8, device=dev)
        sor = event_us(lambda: _lib.check(L_.creg_statistical_outlier_f64(p(pts), n, p(off), L, 20, 2.0, p(avg), p(thr), p(keep), st)),
                       reps)
        origin = torch.empty(L, 3, dtype=torch.float64, device=dev)
        dims = torch.empty(L, 3, dtype=torch.int32, device=dev)
        kept = torch.empty(L, dtype=torch.int64, device=dev)
        bounds = event_us(lambda: _lib.check(L_.creg_voxel_bounds_f64(p(pts), n, p(off), L, p(keep), vs, p(origin), p(dims), p(kept), st)),
                          reps)
        node_off_h = ops.voxel_layout(dims.cpu().numpy(), kept.cpu().numpy())
        total = int(node_off_h[-1])
        node_off = torch.from_numpy(node_off_h).to(dev)
        occ = torch.empty(total, dtype=torch.uint8, device=dev)
        fill = event_us(lambda: _lib.check(L_.creg_voxel_fill_f64(p(pts), n, p(off), L, p(keep), vs, p(origin), p(dims), p(node_off),
                                                                  total, p(occ), st)), reps)
        wsb = int(L_.creg_mc_workspace_bytes(total))
        ws = torch.empty(wsb, dtype=torch.uint8, device=dev)
        voff = torch.empty(L + 1, dtype=torch.int64, device=dev)
        toff = torch.empty(L + 1, dtype=torch.int64, device=dev)
        count = event_us(lambda: _lib.check(L_.creg_mc_count_u8(p(occ), p(dims), p(node_off), L, total, p(voff), p(toff), p(ws), wsb, st)),
                         reps)
        V, F = int(voff[-1]), int(toff[-1])
        verts_h = torch.empty(V, 3, dtype=torch.int32, device=dev)
        tris = torch.empty(F, 3, dtype=torch.int32, device=dev)
        emit = event_us(lambda: _lib.check(L_.creg_mc_emit_i32(p(dims), p(node_off), L, total, p(voff), V, F, p(verts_h), p(tris), p(ws),
                                                               wsb, st)), reps)
        fb = int(L_.creg_mesh_finish_workspace_bytes(V))
        fws = torch.empty(fb, dtype=torch.uint8, device=dev)
        vertices = torch.empty(V, 3, dtype=torch.float64, device=dev)
        rec = torch.empty(F, 4, 3, dtype=torch.float32, device=dev)
        finish = event_us(lambda: _lib.check(L_.creg_mesh_finish_f64(p(verts_h), V, p(tris), F, p(voff), p(toff), L, p(origin), vs, 1,
                                                                     p(vertices), p(rec), p(fws), fb, st)), reps)
        sor_call = event_us(lambda: ops.statistical_outlier(pts, off), reps)
        mesh_call = event_us(lambda: ops.voxel_mesh(pts, off, vs, True, keep), reps)
        with tempfile.TemporaryDirectory() as d:
            d += "/"
            for i, c in enumerate(clouds):
                link.write_ply(d + f"{i:04}.ply", c)
            link.link_mesh([d], L - 1, vs, False)                   # warm-up
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            m = 3
            for _ in range(m):
                link.link_mesh([d], L - 1, vs, False)
            torch.cuda.synchronize()
            wall = (time.perf_counter() - t0) / m
        print(json.dumps({"K": K, "T": T, "links": L, "points": n, "largest_link": int(np.diff(off_h).max()), "voxel_size": vs,
                          "nodes": total, "vertices": V, "triangles": F, "kept": int(keep.sum()),
                          "statistical_outlier_us": round(sor, 1), "voxel_bounds_us": round(bounds, 1), "voxel_fill_us": round(fill, 1),
                          "mc_count_us": round(count, 1), "mc_emit_us": round(emit, 1), "mesh_finish_us": round(finish, 1),
                          "ops_statistical_outlier_call_us": round(sor_call, 1), "ops_voxel_mesh_call_us": round(mesh_call, 1),
                          "link_mesh_wall_ms": round(wall * 1e3, 2)}), flush=True)


if __name__ == "__main__":
    main()
