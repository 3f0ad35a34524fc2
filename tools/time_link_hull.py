"""Time the collision-hull entry points (creg_lattice_hull_i32 + creg_lattice_hull_emit_i32) on the GPU.  Event-timed back-to-back
calls on device inputs built once, at two shapes:

* the toy robot's link meshes: the unsmoothed marching-cubes vertices ``ops.voxel_mesh`` gives for the toy link clouds of the tests
  (4 links, a few hundred to a few thousand lattice points each);
* 12 synthetic links: the marching-cubes vertices of filled lattice ellipsoids and boxes, about 10^4 to 10^5 surface points each.

Per shape: the two entries with the face counts read back between them (the one host wait) on preallocated buffers, and the whole
``ops.lattice_hull`` call (allocation, the coordinate bound, the per-link results).  Beside them, as HOST WALL TIME ON ANOTHER
PROCESSOR, ``scipy.spatial.ConvexHull`` (Qhull) on the same points, link after link -- a yardstick for scale, not a race: the
hull is one workgroup per link here, and nothing in this project asserts a speed-up.

Warm-up: every shape runs once before its window; a window holds at least --min_ms of work; each figure is the median of
--repeats windows with the spread beside it.

    python tools/time_link_hull.py [--toy_only] [--repeats 5] [--min_ms 200]
"""
import argparse
import ctypes
import json
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
from autourdf_amd import _lib, link, ops  # noqa: E402
import _hull_ref as H  # noqa: E402

p = lambda t: ctypes.c_void_p(t.data_ptr()) if t is not None else None


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


def time_shape(name, links, args):
    L_, dev = _lib.load(), _lib.device()
    pn, off_h = H.pack(links)
    n, L = len(pn), len(links)
    pts, off = torch.from_numpy(pn).to(dev), torch.from_numpy(off_h).to(dev)
    max_abs = int(np.abs(pn).max())
    wsb = int(L_.creg_lattice_hull_workspace_bytes(n, L))
    ws = torch.empty(wsb, dtype=torch.uint8, device=dev)
    status = torch.empty(L, dtype=torch.int32, device=dev)
    count = torch.empty(L, dtype=torch.int32, device=dev)
    tris = torch.empty(2 * n, 3, dtype=torch.int32, device=dev)
    rec = torch.empty(2 * n, 4, 3, dtype=torch.float32, device=dev)
    origin = torch.zeros(L, 3, dtype=torch.float64, device=dev)
    toff = torch.empty(L + 1, dtype=torch.int64, device=dev)
    stream = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
    faces = [0]

    def build():
        _lib.check(L_.creg_lattice_hull_i32(p(pts), n, p(off), off_h.ctypes.data, L, max_abs, p(status), p(count), p(ws), wsb, stream),
                   "creg_lattice_hull_i32")

    def entry():
        build()
        c = count.cpu().numpy().astype(np.int64)                       # the one wait
        t = np.concatenate([[0], np.cumsum(c)])
        toff.copy_(torch.from_numpy(t))
        faces[0] = int(t[-1])
        _lib.check(L_.creg_lattice_hull_emit_i32(p(pts), n, p(off), L, p(toff), faces[0], p(origin), 0.01, p(tris), p(rec), p(ws), wsb,
                                                 stream), "creg_lattice_hull_emit_i32")

    built = event_ms(build, args.repeats, args.min_ms)
    whole = event_ms(entry, args.repeats, args.min_ms)
    assert not status.cpu().numpy().any()
    wrapped = event_ms(lambda: ops.lattice_hull(pts, off_h, origin, 0.01), args.repeats, args.min_ms)
    from scipy.spatial import ConvexHull
    walls = []
    for _ in range(args.repeats):
        t0 = time.perf_counter()
        for x in links:
            ConvexHull(x.astype(np.float64))
        walls.append((time.perf_counter() - t0) * 1e3)
    print(json.dumps({"shape": name, "links": L, "points": n, "largest_link": int(np.diff(off_h).max()), "hull_faces": faces[0],
                      "largest_hull": int(count.max()), "workspace_MB": round(wsb / 2 ** 20, 2),
                      "build_entry_ms": round(built[0], 4), "build_entry_ms_min_max": [round(built[1], 4), round(built[2], 4)],
                      "build_wait_emit_ms": round(whole[0], 4), "build_wait_emit_ms_min_max": [round(whole[1], 4), round(whole[2], 4)],
                      "ops_lattice_hull_ms": round(wrapped[0], 4), "ops_lattice_hull_ms_min_max": [round(wrapped[1], 4), round(wrapped[2], 4)],
                      "qhull_host_wall_ms_another_processor": round(float(np.median(walls)), 3),
                      "qhull_host_wall_ms_min_max": [round(min(walls), 3), round(max(walls), 3)]}), flush=True)


def toy_links():
    dev = _lib.device()
    clouds = H.toy_link_clouds(4)
    off = torch.as_tensor(np.concatenate([[0], np.cumsum([len(c) for c in clouds])]).astype(np.int64), device=dev)
    pts = torch.as_tensor(np.concatenate(clouds), device=dev).contiguous()
    keep, _, _ = ops.statistical_outlier(pts, off, link.NB_NEIGHBORS, link.STD_RATIO)
    return [m["verts_h"].cpu().numpy() for m in ops.voxel_mesh(pts, off, 0.01, smooth=True, keep=keep)]


def synthetic_links():
    out = []
    for k in range(6):
        s = 1.0 + 0.25 * k
        out.append(H.voxel_verts(H.ellipsoid_occ(int(36 * s), int(27 * s), int(20 * s))))
        out.append(H.voxel_verts(np.ones((int(50 * s), int(36 * s), int(24 * s)), bool)))
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--min_ms", type=float, default=200.0)
    ap.add_argument("--toy_only", action="store_true", help="skip the synthetic links")
    args = ap.parse_args()
    time_shape("toy robot's meshes", toy_links(), args)
    if not args.toy_only:
        time_shape("12 ellipsoids and boxes", synthetic_links(), args)


if __name__ == "__main__":
    main()
