// collide_dev.h -- device helpers shared by collide.hip (do two posed link meshes intersect) and clearance.hip (how far apart are
// they): boxes, the link's rows, the chunk-box slots, the bodies of the pose and link-box passes, the block compaction and the
// piercing predicate.  Both files pose the same vertices in the same order and take the same exact min / max boxes of them.
#pragma once
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
// the chunk boxes of link l start at this slot: distinct links never share one (floor(s / 256) + l is strictly increasing by at
// least the link's chunk count), and the last slot in use is below floor(F / 256) + L + 1
__device__ __forceinline__ int64_t chunk_slot(int64_t s, int l) { return (s >> 8) + l; }
static inline int64_t collide_slots(int64_t n_tri, int32_t n_links) { return (n_tri >> 8) + n_links + 1; }

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

// The pose pass, grid (chunk, link, pose): posed vertices (P,F,9) and one box per chunk into the workspace.  A template, like the
// link-box pass below, only so that both translation units may hold it.
template <int kUnused = 0>
__global__ __launch_bounds__(256) void k_collide_pose(const double* __restrict__ tri, const int64_t* __restrict__ tri_start,
                                                      int64_t F, const double* __restrict__ link_T, int L, int64_t p0,
                                                      double* __restrict__ posed, double* __restrict__ chunk_box,
                                                      int64_t n_slots) {
    __shared__ double s_red[30];
    const int l = blockIdx.y;
    const int64_t p = p0 + blockIdx.z;
    int64_t s, e;
    link_rows(tri_start, l, F, s, e);
    const int64_t n_chunks = (e - s + COL_CHUNK - 1) / COL_CHUNK;
    const double* T = link_T + ((size_t)p * L + l) * 16;
    for (int64_t c = blockIdx.x; c < n_chunks; c += gridDim.x) {
        const int64_t f = s + c * COL_CHUNK + threadIdx.x;
        Box b;
        box_empty(b);
        if (f < e) {
            double v[9], w[9];
#pragma unroll
            for (int k = 0; k < 9; ++k) v[k] = tri[(size_t)f * 9 + k];
#pragma unroll
            for (int j = 0; j < 3; ++j)
#pragma unroll
                for (int i = 0; i < 3; ++i)
                    w[3 * j + i] = ((T[4 * i] * v[3 * j] + T[4 * i + 1] * v[3 * j + 1]) + T[4 * i + 2] * v[3 * j + 2]) + T[4 * i + 3];
            double* dst = posed + ((size_t)p * F + f) * 9;
#pragma unroll
            for (int k = 0; k < 9; ++k) dst[k] = w[k];
            box_of_tri(w, b);
        }
        box_block_reduce(b, s_red);
        const int64_t slot = chunk_slot(s, l) + c;
        if (threadIdx.x == 0 && slot < n_slots) box_store(chunk_box + ((size_t)p * n_slots + slot) * 6, b);
        __syncthreads();                                         // s_red is written again in the next trip
    }
}

// The link-box pass, one wave per (link, pose): the link box = min / max over its chunk boxes.
template <int kUnused = 0>
__global__ __launch_bounds__(64) void k_collide_boxes(const int64_t* __restrict__ tri_start, int64_t F, int L, int64_t p0,
                                                      const double* __restrict__ chunk_box, int64_t n_slots,
                                                      double* __restrict__ link_box_ws, double* __restrict__ link_box_out) {
    const int l = blockIdx.x;
    const int64_t p = p0 + blockIdx.y;
    int64_t s, e;
    link_rows(tri_start, l, F, s, e);
    const int64_t n_chunks = (e - s + COL_CHUNK - 1) / COL_CHUNK;
    Box b;
    box_empty(b);
    for (int64_t c = threadIdx.x; c < n_chunks; c += 64) {
        const int64_t slot = chunk_slot(s, l) + c;
        if (slot < n_slots) {
            const double* cb = chunk_box + ((size_t)p * n_slots + slot) * 6;
#pragma unroll
            for (int k = 0; k < 3; ++k) {
                b.lo[k] = fmin(b.lo[k], cb[k]);
                b.hi[k] = fmax(b.hi[k], cb[3 + k]);
            }
        }
    }
    box_wave_reduce(b);
    if (threadIdx.x == 0) {
        box_store(link_box_ws + ((size_t)p * L + l) * 6, b);
        if (link_box_out) box_store(link_box_out + ((size_t)p * L + l) * 6, b);
    }
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
