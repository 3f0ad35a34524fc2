"""Time the evaluation stage's forward kinematics on the GPU: event-timed microseconds per launch of creg_urdf_fk_f64 at
P = 3 and P = 256 poses (link poses and joint lines) for the toy robot of the tests and the three fixture robots (wx200,
franka, allegro), back-to-back launches on device tables and device q built once; beside it the cost of one ops.urdf_fk
call (the wrapper with its q / base uploads) and the wall time of the same P poses through UrdfRobot.fk on the host, each
uploaded as the frame generator did before (torch.as_tensor(..., device=...)), around a device synchronise.  Last, the wall
time of one whole evaluation() on the toy robot at --num_points points (default 10000) after a warm-up call.
The launch is latency-bound (one wave per 64 poses): the figures say what a call costs, no throughput is claimed.

    python tools/time_evaluation.py [--reps 200] [--num_points 10000]
"""
import argparse
import contextlib
import ctypes
import io
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
from autourdf_amd import _lib, evaluation, ops  # noqa: E402
from autourdf_amd.ops._common import _table_on  # noqa: E402
from autourdf_amd.sim_data import UrdfRobot  # noqa: E402
from _robots import unpack_robots  # noqa: E402
from _toy_urdf import write_toy_robot  # noqa: E402


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


def time_fk(name, path, reps):
    dev = torch.device("cuda", torch.cuda.current_device())
    robot = UrdfRobot(path)
    table = robot.fk_table()
    L = _lib.load()
    rng = np.random.default_rng(0)
    base = np.eye(4)
    base[:3, 3] = [0.05, -0.02, 0.1]
    for P in (3, 256):
        rows = [{j["name"]: float(rng.uniform(*sorted(j["limit"]))) for j in robot.joints} for _ in range(P)]
        q = robot.q_rows(rows)
        ops.urdf_fk(table, q, base, want_lines=True)                     # the table goes up here
        parent, child, kind, origin, axis = _table_on(dev, table)
        qd, bd = torch.as_tensor(q, device=dev), torch.as_tensor(base, device=dev)
        J, nl = len(table["names"]), table["n_links"]
        link_T = torch.empty(P, nl, 4, 4, dtype=torch.float64, device=dev)
        lines = torch.empty(P, J, 6, dtype=torch.float64, device=dev)
        p = lambda t: ctypes.c_void_p(t.data_ptr())
        stream = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
        launch = lambda: L.creg_urdf_fk_f64(p(parent), p(child), p(kind), p(origin), p(axis), J, nl, int(table["root"]), p(qd), P, p(bd),
                                            p(link_T), p(lines), stream)
        kernel = event_us(launch, reps)
        call = event_us(lambda: ops.urdf_fk(table, q, base, want_lines=True), reps)

        def host():
            out = [torch.as_tensor(robot.fk(r, base), device=dev) for r in rows]
            torch.cuda.synchronize()
            return out
        host()
        n = max(1, min(20, 2000 // P))
        t0 = time.perf_counter()
        for _ in range(n):
            host()
        host_us = (time.perf_counter() - t0) / n * 1e6
        print(json.dumps({"robot": name, "links": nl, "joints": J, "P": P, "urdf_fk_us": round(kernel, 2),
                          "urdf_fk_wrapper_call_us": round(call, 2), "host_fk_and_upload_us": round(host_us, 1)}), flush=True)


def time_evaluation(toy, num_points):
    kw = dict(pred_urdf_path=toy, gt_urdf_path=toy, dof=3, radius=1.2, num_cameras=8, gui=False, visualize=False, visualize_result=False,
              offset=np.zeros(3), sim_ori=[0, 0, 0.3], pred_ori=[0, 0, 0.3], joint_map=np.arange(3), direction_map=[1, 1, 1])
    with tempfile.TemporaryDirectory() as d, contextlib.redirect_stdout(io.StringIO()):
        np.random.seed(2024)
        evaluation.evaluation(save_path=d + "/warm/", num_points=min(num_points, 2000), **kw)
        torch.cuda.synchronize()
        np.random.seed(2024)
        t0 = time.perf_counter()
        losses = evaluation.evaluation(save_path=d + "/run/", num_points=num_points, **kw)
        torch.cuda.synchronize()
        wall = time.perf_counter() - t0
    print(json.dumps({"robot": "toy", "num_poses": 3, "num_points": num_points, "num_cameras": 8, "pix": 800,
                      "evaluation_wall_s": round(wall, 3), "mean_loss": float(np.mean(losses))}), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=200)
    ap.add_argument("--num_points", type=int, default=10000)
    args = ap.parse_args()
    with tempfile.TemporaryDirectory() as d:
        toy, _, _ = write_toy_robot(os.path.join(d, "toy"))
        robots = unpack_robots(d)
        time_fk("toy", toy, args.reps)
        time_fk("wx200", os.path.join(robots, "interbotix_descriptions/urdf/wx200_real.urdf"), args.reps)
        time_fk("franka", os.path.join(robots, "franka/franka_panda.urdf"), args.reps)
        time_fk("allegro", os.path.join(robots, "allegro_hand_description/allegro_hand_description_left.urdf"), args.reps)
        time_evaluation(toy, args.num_points)


if __name__ == "__main__":
    main()
