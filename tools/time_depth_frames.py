"""Time the depth-camera frame stage on the GPU.  Event-timed back-to-back launches on device inputs built once:

* creg_raster_depth_f64 and creg_depth_points_count_f64 + creg_depth_points_f64, at 3 cameras x 96 x 96 and 20 x 800 x 800, on the
  toy robot of the tests standing on its ground and, when the fixture meshes unpack, on the many-triangle franka;
* creg_segment_plane_f64 at the same two shapes with H = 1000 hypotheses of n = 6 samples on the toy's depth cloud (the whole
  entry: fit, count, select, mask, refit), reported as point-plane tests per second (sum over segments of points x H) and as a
  share of the fp64 vector peak -- 8 fp64 vector operations a test (3 mul, 3 add, |.| folded into the compare, 1 compare; no
  contraction), against AMD's published MI355X vector fp64 figure of 78.6 TFLOP/s, which counts a fused multiply-add as two: 39.3e12
  vector operations per second.  Compute bounds it: every point is read once per 1000 hypotheses;
* the yardstick, timed the same way on the same cloud: a chunked torch restatement ((P @ n) + d).abs() < th summed per
  hypothesis, the H hypotheses in chunks whose points x chunk matrix fits --chunk_bytes;
* one whole data_collection(source="depth", ground_flag=True) frame as wall time around a device synchronise.

Warm-up: every shape runs once before its window; a window holds at least --min_ms of work (the repeat count is raised until
it does); each figure is the median of --repeats windows with the spread beside it.

    python tools/time_depth_frames.py [--small_only] [--repeats 5] [--min_ms 200]
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
from autourdf_amd import _lib, ops  # noqa: E402
from autourdf_amd.sim_data import SimEnv, angle_list, data_collection  # noqa: E402
from _toy_urdf import write_toy_robot  # noqa: E402

FP64_VECTOR_OPS_PER_S = 78.6e12 / 2          # published vector fp64 peak, an FMA counted as two
OPS_PER_TEST = 8
p = lambda t: ctypes.c_void_p(t.data_ptr())


def event_ms(fn, repeats, min_ms):
    """Median and (min, max) milliseconds per call of fn over `repeats` windows of at least min_ms each."""
    fn()
    torch.cuda.synchronize()
    reps, out = 1, []
    while len(out) < repeats:
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        for _ in range(reps):
            fn()
        b.record()
        torch.cuda.synchronize()
        ms = a.elapsed_time(b)
        if ms < min_ms and reps < (1 << 20):
            reps = max(reps * 2, int(reps * min_ms / max(ms, 1e-3)) + 1)
            continue
        out.append(ms / reps)
    return float(np.median(out)), float(min(out)), float(max(out))


def scene(env, q, dev):
    tri, own = env._raster_mesh()
    T = torch.as_tensor(env.robot.fk(q, env.base), device=dev)
    if env.ground_tri is not None:
        T = torch.cat([T, torch.eye(4, dtype=T.dtype, device=dev)[None]])
    return tri, own, T.contiguous(), torch.as_tensor(env.cam_frames, device=dev)


def time_raster_and_points(name, env, q, pix, args):
    L, dev = _lib.load(), _lib.device()
    tri, own, T, cams = scene(env, q, dev)
    C, c = cams.shape[0], env.cameras[0]
    stream = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
    depth = torch.empty(C, pix, pix, dtype=torch.float64, device=dev)
    raster = lambda: L.creg_raster_depth_f64(p(tri), p(own), tri.shape[0], p(T), T.shape[0], p(cams), C, float(c['fov']), float(c['aspect']),
                                             float(c['near_val']), float(c['far_val']), pix, pix, p(depth), stream)
    r = event_ms(raster, args.repeats, args.min_ms)
    ws_bytes = L.creg_depth_points_workspace_bytes(C, pix, pix)
    ws = torch.empty(ws_bytes // 8, dtype=torch.int64, device=dev)
    off = torch.empty(C + 1, dtype=torch.int64, device=dev)
    L.creg_depth_points_count_f64(p(depth), C, pix, pix, p(off), p(ws), ws_bytes, stream)
    M = int(off[C].item())
    pts = torch.empty(max(M, 1), 3, dtype=torch.float64, device=dev)

    def points():
        L.creg_depth_points_count_f64(p(depth), C, pix, pix, p(off), p(ws), ws_bytes, stream)
        L.creg_depth_points_f64(p(depth), p(cams), C, float(c['fov']), float(c['aspect']), pix, pix, p(ws), ws_bytes, p(pts), M, stream)
    d = event_ms(points, args.repeats, args.min_ms)
    print(json.dumps({"robot": name, "triangles": int(tri.shape[0]), "cameras": C, "pix": pix, "points": M,
                      "raster_depth_ms": round(r[0], 4), "raster_depth_ms_min_max": [round(r[1], 4), round(r[2], 4)],
                      "depth_points_ms": round(d[0], 4), "depth_points_ms_min_max": [round(d[1], 4), round(d[2], 4)]}), flush=True)
    return pts[:M], off


def torch_counts(P, off, planes, th, chunk_bytes):
    """The yardstick: per segment ((P @ n) + d).abs() < th summed over the points, the hypotheses in chunks."""
    S, H = planes.shape[:2]
    out = torch.empty(S, H, dtype=torch.int64, device=P.device)
    o = off.tolist()
    for s in range(S):
        seg = P[o[s]:o[s + 1]]
        step = max(1, min(H, chunk_bytes // max(8 * seg.shape[0], 1)))
        for h0 in range(0, H, step):
            pl = planes[s, h0:h0 + step]
            out[s, h0:h0 + step] = ((seg @ pl[:, :3].T + pl[:, 3]).abs() < th).sum(0)
    return out


def time_segment_plane(pts, off, H, n, args):
    L, dev = _lib.load(), pts.device
    N, S = pts.shape[0], off.shape[0] - 1
    lens = np.diff(off.cpu().numpy())
    rng = np.random.default_rng(0)
    samples = torch.as_tensor(np.stack([rng.integers(0, max(int(m), 1), (H, n)) for m in lens]), device=dev)
    plane, count = torch.empty(S, 4, dtype=torch.float64, device=dev), torch.empty(S, dtype=torch.int64, device=dev)
    mask, best = torch.empty(N, dtype=torch.uint8, device=dev), torch.empty(S, dtype=torch.int32, device=dev)
    hp, hc = torch.empty(S, H, 4, dtype=torch.float64, device=dev), torch.empty(S, H, dtype=torch.int32, device=dev)
    ws_bytes = L.creg_segment_plane_workspace_bytes(N, S, H)
    ws = torch.empty((ws_bytes + 7) // 8, dtype=torch.float64, device=dev)
    stream = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
    run = lambda: L.creg_segment_plane_f64(p(pts), N, p(off), S, p(samples), H, n, 0.001, p(plane), p(mask), p(count), p(best), p(hp), p(hc),
                                           p(ws), ws_bytes, stream)
    k = event_ms(run, args.repeats, args.min_ms)
    torch.cuda.synchronize()
    planes = torch.nan_to_num(hp, nan=1e30)                           # an invalid plane: far from every point, like the NaN it stands for
    want = torch_counts(pts, off, planes, 0.001, args.chunk_bytes)
    same = bool((want == hc).all())
    t = event_ms(lambda: torch_counts(pts, off, planes, 0.001, args.chunk_bytes), args.repeats, args.min_ms)
    tests = float(lens.sum()) * H
    rate = tests / (k[0] * 1e-3)
    print(json.dumps({"segments": S, "points": N, "hypotheses": H, "ransac_n": n, "point_plane_tests": tests,
                      "segment_plane_ms": round(k[0], 4), "segment_plane_ms_min_max": [round(k[1], 4), round(k[2], 4)],
                      "tests_per_s": rate, "share_of_fp64_vector_peak": round(rate * OPS_PER_TEST / FP64_VECTOR_OPS_PER_S, 4),
                      "torch_chunked_counts_ms": round(t[0], 4), "torch_chunked_counts_ms_min_max": [round(t[1], 4), round(t[2], 4)],
                      "torch_chunk_bytes": args.chunk_bytes, "torch_counts_equal_kernel": same,
                      "speedup_vs_torch_counts": round(t[0] / k[0], 2)}), flush=True)


def time_frame(toy, pix, cameras, args):
    np.random.seed(0)
    env = SimEnv(toy, dof=3, radius=1.2, num_cameras=cameras, ground_flag=True)
    a = angle_list(1, 4, 3, env.joint_limits, np.array([0.9] * 3), seed_i=0)
    kw = dict(angle_list=a, noise_flag=False, num_points=5000, width=pix, height=pix, source="depth", ground_flag=True)
    data_collection(env, **kw)
    torch.cuda.synchronize()
    walls = []
    for _ in range(args.repeats):
        t0 = time.perf_counter()
        data_collection(env, **kw)
        torch.cuda.synchronize()
        walls.append(time.perf_counter() - t0)
    print(json.dumps({"robot": "toy", "cameras": cameras, "pix": pix, "num_points": 5000, "frame_wall_s": round(float(np.median(walls)), 4),
                      "frame_wall_s_min_max": [round(min(walls), 4), round(max(walls), 4)]}), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--min_ms", type=float, default=200.0)
    ap.add_argument("--chunk_bytes", type=int, default=1 << 30, help="largest points x hypotheses matrix of the torch yardstick")
    ap.add_argument("--small_only", action="store_true", help="3 cameras x 96 x 96 only")
    args = ap.parse_args()
    shapes = [(3, 96)] if args.small_only else [(3, 96), (20, 800)]
    with tempfile.TemporaryDirectory() as d:
        toy, _, _ = write_toy_robot(os.path.join(d, "toy"))
        franka = None
        try:
            from _robots import unpack_robots
            franka = os.path.join(unpack_robots(d), "franka", "franka_panda.urdf")
        except Exception as e:                                       # the fixture meshes are optional here
            print(json.dumps({"franka": f"not timed: {e}"}), flush=True)
        for cameras, pix in shapes:
            np.random.seed(0)                                        # the ring of 20 cameras draws from the global state
            env = SimEnv(toy, dof=3, radius=1.2, num_cameras=cameras, ground_flag=True)
            q = env.set_joint_positions([0.4, -0.6, 0.9])
            pts, off = time_raster_and_points("toy+ground", env, q, pix, args)
            time_segment_plane(pts, off, 1000, 6, args)
            if franka is not None and os.path.exists(franka):
                np.random.seed(0)
                fenv = SimEnv(franka, dof=6, radius=1.5, num_cameras=cameras, ground_flag=True)
                time_raster_and_points("franka+ground", fenv, fenv.set_joint_positions(np.zeros(len(fenv.joint_list))), pix, args)
            time_frame(toy, pix, cameras, args)


if __name__ == "__main__":
    main()
