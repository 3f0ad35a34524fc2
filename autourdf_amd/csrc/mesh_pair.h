// mesh_pair.h -- what the mesh pair queries share: collide.hip (do two posed link meshes intersect), clearance.hip (how far apart
// are they) and contain.hip (is one wholly inside the other).
//   posing stage   mesh_pose.hip: the workspace prefix posed | chunk_box | link_box (pose_layout), the argument checks of the three
//                  entries (mesh_pair_check) and the pose and link-box passes of one pose slice (mesh_pose_launch); the point
//                  queries (point_mesh.hip, pose_fit.hip, link_moments.hip) add their own checks (point_query_check)
//   device helpers boxes, the link's rows, the vertex formula (pose_tri), the chunk-box slots, the block compaction and the piercing predicate, for the pair kernels
#pragma once
#include <algorithm>
#include <cmath>
#include "creg_common.h"

namespace creg {

constexpr int COL_CHUNK = 256;
constexpr int COL_TILES_X = 128;                                 // cap of gridDim.x: blocks stride over a link's chunks

struct Box { double lo[3], hi[3]; };

__device__ __forceinline__ void box_empty(Box& b) {
#pragma unroll
    for (int k = 0; k < 3; ++k) { b.lo[k] = INFINITY; b.hi[k] = -INFINITY; }
}
__device__ __forceinline__ void box_of_tri(const double* w, Box& b) {
#pragma unroll
    for (int k = 0; k < 3; ++k) {
        b.lo[k] = fmin(fmin(w[k], w[3 + k]), w[6 + k]);
        b.hi[k] = fmax(fmax(w[k], w[3 + k]), w[6 + k]);
    }
}
__device__ __forceinline__ bool box_meet(const Box& a, const Box& b) {
    return a.lo[0] <= b.hi[0] && b.lo[0] <= a.hi[0] && a.lo[1] <= b.hi[1] && b.lo[1] <= a.hi[1] && a.lo[2] <= b.hi[2] &&
           b.lo[2] <= a.hi[2];
}
__device__ __forceinline__ void box_load(const double* p, Box& b) {
#pragma unroll
    for (int k = 0; k < 3; ++k) { b.lo[k] = p[k]; b.hi[k] = p[3 + k]; }
}
__device__ __forceinline__ void box_store(double* p, const Box& b) {
#pragma unroll
    for (int k = 0; k < 3; ++k) { p[k] = b.lo[k]; p[3 + k] = b.hi[k]; }
}
__device__ __forceinline__ void box_wave_reduce(Box& b) {
#pragma unroll
    for (int off = 32; off >= 1; off >>= 1) {
#pragma unroll
        for (int k = 0; k < 3; ++k) {
            b.lo[k] = fmin(b.lo[k], __shfl_xor(b.lo[k], off, 64));
            b.hi[k] = fmax(b.hi[k], __shfl_xor(b.hi[k], off, 64));
        }
    }
}
// min / max over the 256 threads of a block; every thread returns with the result.  s_red: 4 x 6 doubles + 6 for the result.
__device__ __forceinline__ void box_block_reduce(Box& b, double* s_red) {
    box_wave_reduce(b);
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    if (lane == 0) box_store(s_red + 6 * wave, b);
    __syncthreads();
    if (threadIdx.x == 0) {
        Box r;
        box_load(s_red, r);
        for (int w = 1; w < 4; ++w)
#pragma unroll
            for (int k = 0; k < 3; ++k) {
                r.lo[k] = fmin(r.lo[k], s_red[6 * w + k]);
                r.hi[k] = fmax(r.hi[k], s_red[6 * w + 3 + k]);
            }
        box_store(s_red + 24, r);
    }
    __syncthreads();
    box_load(s_red + 24, b);
}

// rows [s, e) of link l, clamped into [0, F] so that a broken tri_start reads nothing outside tri
__device__ __forceinline__ void link_rows(const int64_t* __restrict__ tri_start, int l, int64_t F, int64_t& s, int64_t& e) {
    s = tri_start[l];
    e = tri_start[l + 1];
    s = s < 0 ? 0 : (s > F ? F : s);
    e = e < s ? s : (e > F ? F : e);
}
// the posed triangle w (9 doubles, vertex-major) of the link-frame triangle v under the row-major 4x4 T: the one vertex formula
__device__ __forceinline__ void pose_tri(const double* T, const double* v, double* w) {
#pragma unroll
    for (int j = 0; j < 3; ++j)
#pragma unroll
        for (int a = 0; a < 3; ++a)
            w[3 * j + a] = ((T[4 * a] * v[3 * j] + T[4 * a + 1] * v[3 * j + 1]) + T[4 * a + 2] * v[3 * j + 2]) + T[4 * a + 3];
}
// the chunk boxes of link l start at this slot: distinct links never share one (floor(s / 256) + l is strictly increasing by at
// least the link's chunk count), and the last slot in use is below floor(F / 256) + L + 1
__device__ __forceinline__ int64_t chunk_slot(int64_t s, int l) { return (s >> 8) + l; }

// the workspace prefix of every query (its own buffers start at `end`), the chunk-box slots of a pose, gridDim.x of the passes
struct PoseLayout { size_t posed, chunk_box, link_box, end; int64_t n_slots; unsigned tiles; };
static inline PoseLayout pose_layout(int64_t n_tri, int32_t n_links, int64_t n_poses) {
    PoseLayout w;
    w.n_slots = (n_tri >> 8) + n_links + 1;
    w.tiles = (unsigned)std::min<int64_t>(std::max<int64_t>((n_tri + COL_CHUNK - 1) / COL_CHUNK, 1), COL_TILES_X);
    w.posed = 0;
    w.chunk_box = align_up(w.posed + sizeof(double) * 9 * (size_t)n_poses * (size_t)n_tri, 256);
    w.link_box = align_up(w.chunk_box + sizeof(double) * 6 * (size_t)n_poses * (size_t)w.n_slots, 256);
    w.end = align_up(w.link_box + sizeof(double) * 6 * (size_t)n_poses * (size_t)n_links, 256);
    return w;
}
// the counts for which the *_workspace_bytes calls answer with a size
static inline bool mesh_pair_counts_ok(int64_t n_tri, int32_t n_links, int64_t n_poses, int64_t n_pairs) {
    return n_tri >= 0 && n_tri < (1ll << 31) && n_links >= 1 && n_poses >= 1 && n_pairs >= 0;
}
// the entries' shared checks, `who` in every message: counts, limits, null pointers (`outs` names the two outputs), workspace size
int mesh_pair_check(const char* who, const void* tri, const void* tri_start, int64_t n_tri, const void* link_T, int32_t n_links,
                    int64_t n_poses, const void* pairs, int64_t n_pairs, const void* out_a, const void* out_b, const char* outs,
                    const void* workspace, size_t workspace_bytes, size_t need);
// the point queries' own checks (tiles of 1 << shift rows), before mesh_pair_check: d_max >= 0, 0 <= n_pts < 2^31, (n_pts >> shift)
// + n_poses < 2^31, pt_start and `rest` (the entry's other pointers, named in rest_names), `per_point` (its arrays of n_pts rows)
// unless n_pts is 0.  creg_point_mesh_f64 passes no rest_names: n_poses >= 1 is mesh_pair_check's there, one message for its nulls.
int point_query_check(const char* who, double d_max, int64_t n_pts, int64_t n_poses, int shift, const void* pt_start, bool rest,
                      const char* rest_names, bool per_point, const char* per_point_names);
// k_collide_pose and k_collide_boxes for the poses [p0, p0 + np), np <= 65535; link_box_out may be null
int mesh_pose_launch(hipStream_t s, const double* tri, const int64_t* tri_start, int64_t n_tri, const double* link_T, int32_t n_links,
                     int64_t p0, unsigned np, const PoseLayout& w, void* workspace, double* link_box_out);

__device__ __forceinline__ double orient(const double* p, const double* q, const double* r, const double* s) {
    const double ux = q[0] - p[0], uy = q[1] - p[1], uz = q[2] - p[2];
    const double vx = r[0] - p[0], vy = r[1] - p[1], vz = r[2] - p[2];
    const double wx = s[0] - p[0], wy = s[1] - p[1], wz = s[2] - p[2];
    const double cx = uy * vz - uz * vy, cy = uz * vx - ux * vz, cz = ux * vy - uy * vx;
    return (cx * wx + cy * wy) + cz * wz;
}
// some edge of triangle E properly pierces triangle T (both 9 doubles, vertex-major)
__device__ __forceinline__ bool edges_pierce(const double* E, const double* T) {
    double d[3];
#pragma unroll
    for (int k = 0; k < 3; ++k) d[k] = orient(T, T + 3, T + 6, E + 3 * k);
    bool hit = false;
#pragma unroll
    for (int k = 0; k < 3; ++k) {
        const int k1 = (k + 1) % 3;
        if ((d[k] > 0.0 && d[k1] < 0.0) || (d[k] < 0.0 && d[k1] > 0.0)) {
            const double* p = E + 3 * k;
            const double* q = E + 3 * k1;
            const double s1 = orient(p, q, T, T + 3), s2 = orient(p, q, T + 3, T + 6), s3 = orient(p, q, T + 6, T);
            hit = hit || (s1 > 0.0 && s2 > 0.0 && s3 > 0.0) || (s1 < 0.0 && s2 < 0.0 && s3 < 0.0);
        }
    }
    return hit;
}

// Stable compaction of the block's `keep` flags: the thread's slot among the kept (or -1) and their number.  s_cnt: 4 ints;
// the caller separates two calls by a barrier after the last read of the returned values' LDS (see the pair kernels).
__device__ __forceinline__ int block_compact(bool keep, int* s_cnt, int& total) {
    const unsigned long long m = __ballot(keep);
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    if (lane == 0) s_cnt[wave] = __popcll(m);
    __syncthreads();
    int base = 0, all = 0;
#pragma unroll
    for (int w = 0; w < 4; ++w) {
        const int c = s_cnt[w];
        base += w < wave ? c : 0;
        all += c;
    }
    total = all;
    return keep ? base + __popcll(m & ((1ull << lane) - 1ull)) : -1;
}

}  // namespace creg
