"""Time the self-collision check (creg_mesh_collide_f64) on the GPU.  Event-timed back-to-back calls on device inputs built once:

* the toy robot of the tests at P = 10 poses, its 6 non-adjacent link pairs: the pose pass alone (the entry with n_pairs = 0: posed
  vertices, chunk and link boxes) and the whole entry (pose pass + pair pass + the keys -> first pass);
* a synthetic robot of 12 links x 20 000 triangles (UV spheres of radius 0.1 strung along a random walk, so that neighbours and
  some others intersect), all 66 pairs, P = 10: the same two figures, and the work the call decides per second -- triangle pairs
  covered (sum of n_a n_b over pairs and poses: what a brute-force count would test), triangle pairs whose boxes overlap (each of
  them goes through the six edge tests; counted by the yardstick) and colliding pairs;
* the yardstick, timed the same way on the same input: a chunked torch restatement of the count -- link boxes, the triangles of
  each link that meet the other's box, their box-overlap matrix in chunks that fit --chunk_bytes, the edge tests on its nonzeros;
* one collect(reject_collisions=True) seed of the toy as wall time, and its sequence check alone.

Warm-up: every shape runs once before its window; a window holds at least --min_ms of work; each figure is the median of
--repeats windows with the spread beside it.

    python tools/time_collide.py [--toy_only] [--repeats 5] [--min_ms 200]
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
from autourdf_amd import _lib, ops, sim_data  # noqa: E402
from autourdf_amd.sim_data import SimEnv  # noqa: E402
import _collide_ref as ref  # noqa: E402
from _toy_urdf import write_toy_robot  # noqa: E402

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


# ------------------------------------------------------------------------------------------ the torch yardstick
def t_orient(a, b, c, d):
    u, v, w = b - a, c - a, d - a
    cx = u[:, 1] * v[:, 2] - u[:, 2] * v[:, 1]
    cy = u[:, 2] * v[:, 0] - u[:, 0] * v[:, 2]
    cz = u[:, 0] * v[:, 1] - u[:, 1] * v[:, 0]
    return (cx * w[:, 0] + cy * w[:, 1]) + cz * w[:, 2]


def t_pierces(e0, e1, a, b, c):
    d1, d2 = t_orient(a, b, c, e0), t_orient(a, b, c, e1)
    s1, s2, s3 = t_orient(e0, e1, a, b), t_orient(e0, e1, b, c), t_orient(e0, e1, c, a)
    return (((d1 > 0) & (d2 < 0)) | ((d1 < 0) & (d2 > 0))) & (((s1 > 0) & (s2 > 0) & (s3 > 0)) | ((s1 < 0) & (s2 < 0) & (s3 < 0)))


def t_meet(lo_a, hi_a, lo_b, hi_b):
    return ((lo_a <= hi_b) & (lo_b <= hi_a)).all(-1)


def torch_counts(tri, start, link_T, pairs, chunk_bytes):
    """(count (P,M) int64, box-overlapping triangle pairs) by the contract, in torch."""
    P, L = link_T.shape[:2]
    count = torch.zeros(P, len(pairs), dtype=torch.int64, device=tri.device)
    tested = 0
    for q in range(P):
        posed = []
        for l in range(L):
            v, T = tri[start[l]:start[l + 1]], link_T[q, l]
            posed.append(torch.stack([((T[i, 0] * v[..., 0] + T[i, 1] * v[..., 1]) + T[i, 2] * v[..., 2]) + T[i, 3] for i in range(3)], -1))
        lo, hi = [t.amin(1) for t in posed], [t.amax(1) for t in posed]
        for m, (la, lb) in enumerate(pairs):
            if not len(posed[la]) or not len(posed[lb]) or not bool(t_meet(lo[la].amin(0), hi[la].amax(0), lo[lb].amin(0), hi[lb].amax(0))):
                continue
            ka = t_meet(lo[la], hi[la], lo[lb].amin(0), hi[lb].amax(0)).nonzero()[:, 0]
            kb = t_meet(lo[lb], hi[lb], lo[la].amin(0), hi[la].amax(0)).nonzero()[:, 0]
            if not len(ka) or not len(kb):
                continue
            A, B = posed[la][ka], posed[lb][kb]
            step = max(1, chunk_bytes // (8 * len(kb)))
            for a0 in range(0, len(ka), step):
                ia, ib = t_meet(lo[la][ka[a0:a0 + step], None], hi[la][ka[a0:a0 + step], None], lo[lb][kb][None], hi[lb][kb][None]).nonzero(as_tuple=True)
                tested += len(ia)
                if not len(ia):
                    continue
                a, b = A[a0:a0 + step][ia], B[ib]
                hit = torch.zeros(len(ia), dtype=torch.bool, device=tri.device)
                for E, T in ((a, b), (b, a)):
                    for k in range(3):
                        hit |= t_pierces(E[:, k], E[:, (k + 1) % 3], T[:, 0], T[:, 1], T[:, 2])
                count[q, m] += hit.sum()
    return count, tested


# ------------------------------------------------------------------------------------------ the kernel
def time_entry(name, tri, start, link_T, pairs, args, yardstick):
    L, dev = _lib.load(), _lib.device()
    d_tri, d_start, d_T, d_pairs = (torch.as_tensor(np.ascontiguousarray(a), device=dev) for a in (tri, start, link_T, pairs))
    F, (P, n_links), M = len(tri), link_T.shape[:2], len(pairs)
    ws_bytes = L.creg_mesh_collide_workspace_bytes(F, n_links, P, M)
    ws = torch.empty(ws_bytes // 8, dtype=torch.float64, device=dev)
    count = torch.empty(P, M, dtype=torch.int32, device=dev)
    first = torch.empty(P, M, 2, dtype=torch.int32, device=dev)
    box = torch.empty(P, n_links, 6, dtype=torch.float64, device=dev)
    stream = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
    call = lambda m: _lib.check(L.creg_mesh_collide_f64(p(d_tri), p(d_start), F, p(d_T), n_links, P, p(d_pairs), m, p(count), p(first), p(box),
                                                        p(ws), ws_bytes, stream), "creg_mesh_collide_f64")
    pose = event_ms(lambda: call(0), args.repeats, args.min_ms)
    whole = event_ms(lambda: call(M), args.repeats, args.min_ms)
    torch.cuda.synchronize()
    sizes = np.diff(start)
    covered = float(sum(int(sizes[a]) * int(sizes[b]) for a, b in pairs)) * P
    out = {"robot": name, "triangles": F, "links": int(n_links), "pairs": M, "poses": int(P), "workspace_MB": round(ws_bytes / 2 ** 20, 1),
           "pose_pass_ms": round(pose[0], 4), "pose_pass_ms_min_max": [round(pose[1], 4), round(pose[2], 4)],
           "whole_entry_ms": round(whole[0], 4), "whole_entry_ms_min_max": [round(whole[1], 4), round(whole[2], 4)],
           "pair_pass_ms": round(whole[0] - pose[0], 4), "colliding_link_pairs": int((count > 0).sum()),
           "colliding_triangle_pairs": int(count.sum()), "triangle_pairs_covered": covered,
           "triangle_pairs_covered_per_s": covered / (whole[0] * 1e-3)}
    if yardstick:
        host_pairs = [tuple(int(x) for x in pr) for pr in pairs]
        want, tested = torch_counts(d_tri, [int(s) for s in start], d_T, host_pairs, args.chunk_bytes)
        t = event_ms(lambda: torch_counts(d_tri, [int(s) for s in start], d_T, host_pairs, args.chunk_bytes), max(1, args.repeats // 2), 0.0)
        out.update({"box_overlapping_triangle_pairs": tested, "edge_tested_pairs_per_s": tested / (whole[0] * 1e-3),
                    "torch_chunked_counts_ms": round(t[0], 3), "torch_chunked_counts_ms_min_max": [round(t[1], 3), round(t[2], 3)],
                    "torch_chunk_bytes": args.chunk_bytes, "torch_counts_equal_kernel": bool((want == count).all()),
                    "speedup_vs_torch_counts": round(t[0] / whole[0], 2)})
    print(json.dumps(out), flush=True)


def synthetic_robot(links=12, per_link=20000, P=10, seed=0):
    rng = np.random.default_rng(seed)
    seg = int(round((per_link / 2) ** 0.5))
    mesh = ref.uv_sphere(0.1, seg=seg, rings=seg + 1)
    assert len(mesh) == per_link
    tri, start = ref.pack([mesh] * links)
    link_T = np.empty((P, links, 4, 4))
    for q in range(P):
        at = np.zeros(3)
        for l in range(links):
            step = rng.normal(size=3)
            at = at + 0.15 * step / np.linalg.norm(step)             # neighbours overlap (centres 0.15 apart, radius 0.1); the walk folds back
            link_T[q, l] = ref.rigid(ref.random_rotation(rng), at)
    return tri, start, link_T, ref.all_pairs(links)


def time_collect(toy_dir, args):
    params = {"gt": "toy.urdf", "dof": 3}
    kw = dict(num_step=10, epochs=1, num_points=5000, num_cameras=3, root=toy_dir, pix=96, reject_collisions=True)
    sim_data.collect("toy", params, **kw)
    torch.cuda.synchronize()
    walls, checks = [], []
    env = SimEnv(os.path.join(toy_dir, "toy.urdf"), dof=3, radius=1.5, num_cameras=3)
    a = sim_data.angle_list(10, 4, 3, env.joint_limits, np.array([0.9] * 3), 0)
    sim_data.sequence_collides(env, a)
    for _ in range(args.repeats):
        t0 = time.perf_counter()
        sim_data.collect("toy", params, **kw)
        torch.cuda.synchronize()
        walls.append(time.perf_counter() - t0)
        t0 = time.perf_counter()
        sim_data.sequence_collides(env, a)
        checks.append(time.perf_counter() - t0)
    print(json.dumps({"robot": "toy", "num_step": 10, "num_points": 5000, "cameras": 3, "pix": 96,
                      "collect_reject_collisions_seed_wall_s": round(float(np.median(walls)), 4),
                      "collect_wall_s_min_max": [round(min(walls), 4), round(max(walls), 4)],
                      "sequence_collides_wall_s": round(float(np.median(checks)), 5),
                      "sequence_collides_wall_s_min_max": [round(min(checks), 5), round(max(checks), 5)]}), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--min_ms", type=float, default=200.0)
    ap.add_argument("--chunk_bytes", type=int, default=1 << 28, help="largest box-overlap matrix of the torch yardstick")
    ap.add_argument("--toy_only", action="store_true", help="skip the synthetic robot")
    args = ap.parse_args()
    with tempfile.TemporaryDirectory() as d:
        toy, _, _ = write_toy_robot(d)
        env = SimEnv(toy, dof=3, radius=1.2, num_cameras=3)
        r = env.robot
        rows = sim_data.angle_list(10, 4, 3, env.joint_limits, np.array([0.9] * 3), 0)
        link_T = ops.urdf_fk(r.fk_table(), r.q_rows([env.set_joint_positions(c) for c in rows]), env.base).cpu().numpy()
        time_entry("toy", r.tri, r.tri_start, link_T, r.collision_pairs(), args, yardstick=True)
        if not args.toy_only:
            time_entry("12 spheres x 20000", *synthetic_robot(), args, yardstick=True)
        time_collect(d, args)


if __name__ == "__main__":
    main()
