"""Time the mass-property entry point (creg_mesh_inertia_f64) on the GPU.  Event-timed back-to-back calls on device inputs built once:

* the toy robot of the tests (its <visual> triangles, 5 links) and a synthetic robot of 12 links x 20 000 triangles (UV spheres of
  radius 0.1): the whole entry (chunk pass + finishing pass) and the bytes it has to read (72 per triangle) over that time;
* the yardstick, timed the same way on the same input: a torch restatement of the same 14 sums -- the reference point of every
  triangle's link gathered, the terms as whole-array expressions, one sum per link over its rows -- and the largest difference of its
  sums from the kernel's, relative to the sum of the terms' absolute values;
* one link_inertia call on the synthetic robot's meshes written as STL files (read, one launch, read back, checks, inertial.json)
  as wall time.

Warm-up: every shape runs once before its window; a window holds at least --min_ms of work; each figure is the median of
--repeats windows with the spread beside it.

    python tools/time_mesh_inertia.py [--toy_only] [--repeats 5] [--min_ms 200]
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
from autourdf_amd import _lib, link, ops  # noqa: E402
from autourdf_amd.sim_data import SimEnv  # noqa: E402
import _collide_ref as ref  # noqa: E402
from _toy_urdf import write_toy_robot  # noqa: E402

p = lambda t: ctypes.c_void_p(t.data_ptr()) if t is not None else None
PAIRS = ((0, 0), (0, 1), (0, 2), (1, 1), (1, 2), (2, 2))


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


def torch_sums(tri, first, link_of, bounds, want_abs=False):
    """sums (L,14) by the contract's terms, in torch: the reference point of every triangle's link gathered, the terms as
    whole-array expressions, one sum per link over its rows (the links are contiguous) -- and the sums of |term| when asked."""
    r = tri[first[link_of], 0]
    a, b, c = tri[:, 0] - r, tri[:, 1] - r, tri[:, 2] - r
    s = (a + b) + c
    n = torch.linalg.cross(b - a, c - a)
    d = (a * torch.linalg.cross(b, c)).sum(1)
    t = torch.cat([n, n.norm(dim=1, keepdim=True), d[:, None], d[:, None] * s] +
                  [(d * (s[:, i] * s[:, j] + a[:, i] * a[:, j] + b[:, i] * b[:, j] + c[:, i] * c[:, j]))[:, None] for i, j in PAIRS], 1)
    out = torch.stack([t[lo:hi].sum(0) for lo, hi in bounds])
    return (out, torch.stack([t[lo:hi].abs().sum(0) for lo, hi in bounds])) if want_abs else out


def time_entry(name, tri, start, args):
    L, dev = _lib.load(), _lib.device()
    d_tri = torch.as_tensor(np.ascontiguousarray(tri, np.float64).reshape(-1, 3, 3), device=dev)
    d_start = torch.as_tensor(np.ascontiguousarray(start, np.int64), device=dev)
    F, n_links = d_tri.shape[0], len(start) - 1
    density = torch.full((n_links,), 1000.0, dtype=torch.float64, device=dev)
    shapes = dict(sums=(14,), volume=(), area=(), closure=(), mass=(), com=(3,), inertia=(6,), principal=(3,), axes=(3, 3))
    out = {k: torch.empty((n_links,) + shapes[k], dtype=torch.float64, device=dev) for k in ops.MESH_INERTIA_KEYS}
    ws_bytes = L.creg_mesh_inertia_workspace_bytes(F, n_links)
    ws = torch.empty(ws_bytes // 8, dtype=torch.float64, device=dev)
    stream = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
    call = lambda: _lib.check(L.creg_mesh_inertia_f64(p(d_tri), p(d_start), F, n_links, p(density), *[p(out[k]) for k in ops.MESH_INERTIA_KEYS],
                                                      p(ws), ws_bytes, stream), "creg_mesh_inertia_f64")
    whole = event_ms(call, args.repeats, args.min_ms)
    wrapped = event_ms(lambda: ops.mesh_inertia(d_tri, d_start, density), args.repeats, args.min_ms)
    sizes = np.diff(start)
    link_of = torch.as_tensor(np.repeat(np.arange(n_links), sizes), device=dev)
    first = torch.as_tensor(np.minimum(np.asarray(start[:-1], np.int64), max(F - 1, 0)), device=dev)
    bounds = [(int(lo), int(hi)) for lo, hi in zip(start[:-1], start[1:])]
    yard = event_ms(lambda: torch_sums(d_tri, first, link_of, bounds), args.repeats, args.min_ms)
    want, want_abs = torch_sums(d_tri, first, link_of, bounds, want_abs=True)
    live = (out["sums"][:, 4] != 0)[:, None] & (want_abs > 0)
    diff = float(((out["sums"] - want).abs() / want_abs.clamp_min(1e-300))[live].max()) if bool(live.any()) else 0.0
    print(json.dumps({"robot": name, "triangles": int(F), "links": int(n_links), "largest_link": int(sizes.max()),
                      "workspace_KB": round(ws_bytes / 1024, 1), "bytes_read": 72 * int(F),
                      "whole_entry_ms": round(whole[0], 4), "whole_entry_ms_min_max": [round(whole[1], 4), round(whole[2], 4)],
                      "bytes_read_over_entry_time_GBps": round(72 * F / (whole[0] * 1e-3) / 1e9, 2),
                      "ops_mesh_inertia_ms": round(wrapped[0], 4), "ops_mesh_inertia_ms_min_max": [round(wrapped[1], 4), round(wrapped[2], 4)],
                      "torch_gather_link_sums_ms": round(yard[0], 4),
                      "torch_gather_link_sums_ms_min_max": [round(yard[1], 4), round(yard[2], 4)],
                      "torch_over_entry": round(yard[0] / whole[0], 2),
                      "max_sum_difference_over_sum_abs_terms": diff}), flush=True)


def synthetic_robot(links=12, per_link=20000):
    seg = int(round((per_link / 2) ** 0.5))
    mesh = ref.uv_sphere(0.1, seg=seg, rings=seg + 1)
    assert len(mesh) == per_link
    meshes = [mesh + np.array([0.15 * l, 0.0, 0.3]) for l in range(links)]
    tri, start = ref.pack(meshes)
    return tri, start, meshes


def time_link_inertia(meshes, args):
    with tempfile.TemporaryDirectory() as d:
        d = d + "/"
        for i, m in enumerate(meshes):
            rec = np.zeros((len(m), 4, 3), np.float32)
            rec[:, 1:] = m
            link.write_stl(d + f"{i:04}.stl", rec)
        link.link_inertia([d], len(meshes) - 1, 1000.0)
        walls = []
        for _ in range(args.repeats):
            t0 = time.perf_counter()
            res = link.link_inertia([d], len(meshes) - 1, 1000.0)
            walls.append(time.perf_counter() - t0)
    print(json.dumps({"links": len(meshes), "triangles": int(sum(len(m) for m in meshes)),
                      "link_inertia_wall_s": round(float(np.median(walls)), 5),
                      "link_inertia_wall_s_min_max": [round(min(walls), 5), round(max(walls), 5)],
                      "mass_of_link_0_kg": res[0]["link_0"]["mass"]}), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--min_ms", type=float, default=200.0)
    ap.add_argument("--toy_only", action="store_true", help="skip the synthetic robot")
    args = ap.parse_args()
    with tempfile.TemporaryDirectory() as d:
        toy, _, _ = write_toy_robot(d)
        r = SimEnv(toy, dof=3, radius=1.2, num_cameras=3).robot
        time_entry("toy", r.tri, r.tri_start, args)
    if not args.toy_only:
        tri, start, meshes = synthetic_robot()
        time_entry("12 spheres x 20000", tri, start, args)
        time_link_inertia(meshes, args)


if __name__ == "__main__":
    main()
