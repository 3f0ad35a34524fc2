// depth.hip -- depth-camera frames: what the reference does with its rendered depth images (Sim/sim_data.py:283-329).
//   creg_depth_points_*      every finite pixel of the per-camera depth buffers (sample.hip, creg_raster_depth_f64) back-projected
//                            to a world point, compacted camera-major / row-major by a count, scan and scatter (no atomics: the
//                            row of a point is a pure function of the buffers);
//   creg_segment_plane_f64   Open3D's segment_plane (distance_threshold, ransac_n, num_iterations) for S segments of one packed
//                            cloud at once -- the ground removal the reference runs per camera (:311-319).  The hypotheses' sample
//                            indices come from the caller; every hypothesis is tested against every point of its segment with the
//                            segment's planes staged in LDS and the points in registers, one wave ballot per (hypothesis, 64 points):
//                            the points x hypotheses matrix is never written.
// All arithmetic is spelled out in a fixed order without contraction; the sums of the refit are fixed trees.
#include <climits>
#include <cmath>
#include "creg_common.h"
#include "creg_dev.h"
#include "eig3.h"

namespace creg {

// ------------------------------------------------------------------------------------------ back-projection
constexpr int DP_NT = 256;            // pixels (threads) per block; one block never straddles two cameras

// grid (ceil(HW / DP_NT), C): blk[c * gridDim.x + b] = finite pixels of block b of camera c
__global__ __launch_bounds__(DP_NT) void k_depth_count(const double* __restrict__ depth, int64_t HW, int64_t* __restrict__ blk) {
    __shared__ int wc[DP_NT / 64];
    const int64_t px = (int64_t)blockIdx.x * DP_NT + threadIdx.x;
    const bool f = px < HW && isfinite(depth[(int64_t)blockIdx.y * HW + px]);
    const unsigned long long m = __ballot(f);
    if ((threadIdx.x & 63) == 0) wc[threadIdx.x >> 6] = __popcll(m);
    __syncthreads();
    if (threadIdx.x == 0) blk[(int64_t)blockIdx.y * gridDim.x + blockIdx.x] = (int64_t)((wc[0] + wc[1]) + (wc[2] + wc[3]));
}

// one block: exclusive scan of blk (nb entries, camera-major) in place, DP_NT entries a trip with the running total carried;
// offsets[c] = the scan at camera c's first block, offsets[C] = the total
__global__ __launch_bounds__(DP_NT) void k_depth_scan(int64_t* __restrict__ blk, int64_t nb, int gx, int C, int64_t* __restrict__ offsets) {
    __shared__ int64_t ws[DP_NT / 64];
    const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
    int64_t carry = 0;
    for (int64_t base = 0; base < nb; base += DP_NT) {
        const int64_t i = base + tid;
        const int64_t v = i < nb ? blk[i] : 0;
        int64_t x = v;
#pragma unroll
        for (int off = 1; off < 64; off <<= 1) {
            const int64_t y = __shfl_up(x, off, WAVE);
            if (lane >= off) x += y;
        }
        if (lane == 63) ws[w] = x;
        __syncthreads();
        int64_t before = 0, total = 0;
#pragma unroll
        for (int k = 0; k < DP_NT / 64; ++k) { if (k < w) before += ws[k]; total += ws[k]; }
        const int64_t excl = carry + before + (x - v);
        if (i < nb) {
            blk[i] = excl;
            if (i % gx == 0) offsets[i / gx] = excl;
        }
        carry += total;
        __syncthreads();
    }
    if (tid == 0) offsets[C] = carry;
}

struct BackProj { double tan_half, aspect; int W, H; };

// grid as k_depth_count; blk holds the scanned block offsets.  Row = block offset + finite pixels before this one in the block.
__global__ __launch_bounds__(DP_NT) void k_depth_scatter(const double* __restrict__ depth, const double* __restrict__ cams, BackProj c,
                                                         const int64_t* __restrict__ blk, double* __restrict__ out, int64_t cap) {
    __shared__ int wc[DP_NT / 64];
    const int64_t HW = (int64_t)c.W * c.H, px = (int64_t)blockIdx.x * DP_NT + threadIdx.x;
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    const double d = px < HW ? depth[(int64_t)blockIdx.y * HW + px] : INFINITY;
    const bool f = px < HW && isfinite(d);
    const unsigned long long m = __ballot(f);
    if (lane == 0) wc[w] = __popcll(m);
    __syncthreads();
    int before = __popcll(m & ((1ull << lane) - 1ull));
    for (int k = 0; k < w; ++k) before += wc[k];
    const int64_t row = blk[(int64_t)blockIdx.y * gridDim.x + blockIdx.x] + before;
    if (!f || row >= cap) return;                           // a capacity smaller than the count drops rows, it never writes past it
    const double* cam = cams + 12 * blockIdx.y;
    const double cx = (double)(px % c.W) + 0.5, cy = (double)(px / c.W) + 0.5;
    const double nx = (cx / (double)c.W - 0.5) * 2.0, ny = ((1.0 - cy / (double)c.H) - 0.5) * 2.0;     // cam_pixel, inverted
    const double xc = nx * ((d * c.tan_half) * c.aspect), yc = ny * (d * c.tan_half);
#pragma unroll
    for (int a = 0; a < 3; ++a) out[3 * row + a] = ((cam[a] + d * cam[3 + a]) + xc * cam[6 + a]) + yc * cam[9 + a];
}

// ------------------------------------------------------------------------------------------ RANSAC planes
constexpr int SP_NT = 256;                    // threads per block
constexpr int SP_PPT = 8;                     // points a thread of the counting kernel keeps in registers
constexpr int SP_TILE = SP_NT * SP_PPT;       // points per block and trip
constexpr int SP_HC = 1024;                   // hypotheses staged in LDS at a time (32 KB of planes + 4 KB of counters)
constexpr int SP_MAX_N = 16;                  // most samples per hypothesis
constexpr int SP_MAX_BLOCKS = 1024;           // blocks of the point passes over all segments (4 per CU fit by their LDS)
constexpr double SP_RANK_TOL = 1e-12;         // see creg.h: the rank test of a fit

__device__ __forceinline__ void seg_range(const int64_t* __restrict__ off, int s, int64_t N, int64_t& lo, int64_t& hi) {
    const int64_t a = off[s], b = off[s + 1];               // offsets that leave [0, N] or run backwards are clamped: nothing outside
    lo = a < 0 ? 0 : (a > N ? N : a);                       // the cloud is ever read
    hi = b < lo ? lo : (b > N ? N : b);
}

__device__ __forceinline__ bool plane_inlier(const double* pl, double x, double y, double z, double th) {
    return fabs(((pl[0] * x + pl[1] * y) + pl[2] * z) + pl[3]) < th;
}

// unit normal | d of the least-squares plane with centroid c and scatter C = (xx, xy, xz, yy, yz, zz); false when the points span
// less than a plane (the rank test of creg.h) or the moments are not finite
__device__ bool plane_from_moments(const double c[3], const double C[6], double* pl) {
    const double tr = (C[0] + C[3]) + C[5];
    const double m2 = ((C[0] * C[3] - C[1] * C[1]) + (C[0] * C[5] - C[2] * C[2])) + (C[3] * C[5] - C[4] * C[4]);
    if (!(m2 > SP_RANK_TOL * (tr * tr))) return false;
    double nv[3];
    smallest_eigvec(C, nv);
    const double l2 = (nv[0] * nv[0] + nv[1] * nv[1]) + nv[2] * nv[2];
    if (!(l2 > 0)) return false;
    const double il = 1.0 / sqrt(l2);
    int j = 0;                                              // the component of largest magnitude is positive, ties to the lowest index
    if (fabs(nv[1]) > fabs(nv[0])) j = 1;
    if (fabs(nv[2]) > fabs(nv[j])) j = 2;
    const double sg = nv[j] < 0 ? -il : il;
    pl[0] = nv[0] * sg; pl[1] = nv[1] * sg; pl[2] = nv[2] * sg;
    pl[3] = -((pl[0] * c[0] + pl[1] * c[1]) + pl[2] * c[2]);
    return true;
}

// grid (ceil(H / SP_NT), S): thread = (hypothesis, segment).  An invalid hypothesis gets a plane of NaN, which no point is within any
// distance of: the counting kernel needs no flag.  Also clears the counters.
__global__ __launch_bounds__(SP_NT) void k_plane_fit(const double* __restrict__ pts, int64_t N, const int64_t* __restrict__ off,
                                                     const int64_t* __restrict__ samples, int H, int n, double* __restrict__ hp,
                                                     int* __restrict__ hc) {
    const int h = blockIdx.x * SP_NT + threadIdx.x, s = blockIdx.y;
    if (h >= H) return;
    int64_t lo, hi;
    seg_range(off, s, N, lo, hi);
    const int64_t nseg = hi - lo;
    const int64_t* smp = samples + ((int64_t)s * H + h) * n;
    bool ok = nseg >= n;
    double c[3] = {0, 0, 0}, C[6] = {0, 0, 0, 0, 0, 0};
    for (int k = 0; k < n && ok; ++k) {
        const int64_t i = smp[k];
        if (i < 0 || i >= nseg) { ok = false; break; }      // an index outside the segment: the hypothesis is invalid, nothing is read
        const double* p = pts + 3 * (lo + i);
        c[0] += p[0]; c[1] += p[1]; c[2] += p[2];
    }
    if (ok) {
        c[0] /= (double)n; c[1] /= (double)n; c[2] /= (double)n;
        for (int k = 0; k < n; ++k) {
            const double* p = pts + 3 * (lo + smp[k]);
            const double dx = p[0] - c[0], dy = p[1] - c[1], dz = p[2] - c[2];
            C[0] += dx * dx; C[1] += dx * dy; C[2] += dx * dz; C[3] += dy * dy; C[4] += dy * dz; C[5] += dz * dz;
        }
    }
    double pl[4];
    if (!ok || !plane_from_moments(c, C, pl)) pl[0] = pl[1] = pl[2] = pl[3] = NAN;
    double* o = hp + 4 * ((int64_t)s * H + h);
    o[0] = pl[0]; o[1] = pl[1]; o[2] = pl[2]; o[3] = pl[3];
    hc[(int64_t)s * H + h] = 0;
}

// grid (B, S).  Per chunk of SP_HC hypotheses: the chunk's planes go to LDS, the block walks its tiles of the segment with SP_PPT
// points a thread in registers, and per hypothesis a wave adds the popcounts of its SP_PPT ballots to an LDS counter; the block
// hands each counter to hyp_counts with one integer atomic.  Integer sums: the result does not depend on any order.
__global__ __launch_bounds__(SP_NT) void k_plane_count(const double* __restrict__ pts, int64_t N, const int64_t* __restrict__ off, int H,
                                                       double th, const double* __restrict__ hp, int* __restrict__ hc) {
    __shared__ double sp[4 * SP_HC];
    __shared__ int lcnt[SP_HC];
    const int s = blockIdx.y, tid = threadIdx.x, lane = tid & 63;
    int64_t lo, hi;
    seg_range(off, s, N, lo, hi);
    const int64_t nseg = hi - lo;
    if ((int64_t)blockIdx.x * SP_TILE >= nseg) return;      // no tile for this block (block-uniform)
    for (int h0 = 0; h0 < H; h0 += SP_HC) {
        const int hn = min(SP_HC, H - h0);
        __syncthreads();
        for (int i = tid; i < 4 * hn; i += SP_NT) sp[i] = hp[4 * ((int64_t)s * H + h0) + i];
        for (int i = tid; i < hn; i += SP_NT) lcnt[i] = 0;
        __syncthreads();
        for (int64_t t0 = (int64_t)blockIdx.x * SP_TILE; t0 < nseg; t0 += (int64_t)gridDim.x * SP_TILE) {
            double x[SP_PPT], y[SP_PPT], z[SP_PPT];
#pragma unroll
            for (int k = 0; k < SP_PPT; ++k) {
                const int64_t i = t0 + k * SP_NT + tid;
                const bool in = i < nseg;                   // past the segment: NaN, inside no plane
                const double* p = pts + 3 * (lo + (in ? i : 0));
                x[k] = in ? p[0] : NAN; y[k] = in ? p[1] : NAN; z[k] = in ? p[2] : NAN;
            }
            for (int h = 0; h < hn; ++h) {
                const double pl[4] = {sp[4 * h], sp[4 * h + 1], sp[4 * h + 2], sp[4 * h + 3]};
                int tot = 0;
#pragma unroll
                for (int k = 0; k < SP_PPT; ++k) tot += __popcll(__ballot(plane_inlier(pl, x[k], y[k], z[k], th)));
                if (lane == 0 && tot) atomicAdd(&lcnt[h], tot);
            }
        }
        __syncthreads();
        for (int i = tid; i < hn; i += SP_NT)
            if (lcnt[i]) atomicAdd(&hc[(int64_t)s * H + h0 + i], lcnt[i]);
    }
}

// grid (S): the valid hypothesis with the most inliers, the smallest index among equals; -1 when none is valid
__global__ __launch_bounds__(SP_NT) void k_plane_select(int H, const double* __restrict__ hp, const int* __restrict__ hc, int* __restrict__ best) {
    __shared__ int sc[SP_NT], si[SP_NT];
    const int s = blockIdx.x, tid = threadIdx.x;
    int bc = -1, bi = INT_MAX;
    for (int h = tid; h < H; h += SP_NT) {                  // ascending h: `>` keeps the thread's smallest index
        if (isnan(hp[4 * ((int64_t)s * H + h)])) continue;
        const int c = hc[(int64_t)s * H + h];
        if (c > bc) { bc = c; bi = h; }
    }
    sc[tid] = bc; si[tid] = bi;
    __syncthreads();
    for (int st = SP_NT / 2; st >= 1; st >>= 1) {
        if (tid < st && (sc[tid + st] > sc[tid] || (sc[tid + st] == sc[tid] && si[tid + st] < si[tid]))) { sc[tid] = sc[tid + st]; si[tid] = si[tid + st]; }
        __syncthreads();
    }
    if (tid == 0) best[s] = sc[0] >= 0 ? si[0] : -1;
}

// grid (B, S): the mask of the best hypothesis and, per block, the coordinate sums of its inliers (fixed tree) -> part1 (S, B, 3)
__global__ __launch_bounds__(SP_NT) void k_plane_mask(const double* __restrict__ pts, int64_t N, const int64_t* __restrict__ off, int H, double th,
                                                      const double* __restrict__ hp, const int* __restrict__ best,
                                                      unsigned char* __restrict__ mask, double* __restrict__ part1) {
    __shared__ double scratch[SP_NT / 64];
    const int s = blockIdx.y, b = best[s];
    if (b < 0) return;                                      // block-uniform; the mask was cleared before
    int64_t lo, hi;
    seg_range(off, s, N, lo, hi);
    double pl[4];
    for (int a = 0; a < 4; ++a) pl[a] = hp[4 * ((int64_t)s * H + b) + a];
    double sum[3] = {0, 0, 0};
    for (int64_t i = lo + (int64_t)blockIdx.x * SP_NT + threadIdx.x; i < hi; i += (int64_t)gridDim.x * SP_NT) {
        const double x = pts[3 * i], y = pts[3 * i + 1], z = pts[3 * i + 2];
        const bool in = plane_inlier(pl, x, y, z, th);
        mask[i] = in ? 1 : 0;
        if (in) { sum[0] += x; sum[1] += y; sum[2] += z; }
    }
    for (int a = 0; a < 3; ++a) {
        const double r = block_sum<double, SP_NT>(sum[a], scratch);
        if (threadIdx.x == 0) part1[((int64_t)s * gridDim.x + blockIdx.x) * 3 + a] = r;
    }
}

// the inliers' centroid from the B block sums, in block order
__device__ __forceinline__ void plane_centroid(const double* __restrict__ part1, int s, int B, int cnt, double* c) {
    double sum[3] = {0, 0, 0};
    for (int b = 0; b < B; ++b)
        for (int a = 0; a < 3; ++a) sum[a] += part1[((int64_t)s * B + b) * 3 + a];
    for (int a = 0; a < 3; ++a) c[a] = sum[a] / (double)cnt;
}

// grid (B, S): per block the inliers' scatter about their centroid -> part2 (S, B, 6)
__global__ __launch_bounds__(SP_NT) void k_plane_scatter(const double* __restrict__ pts, int64_t N, const int64_t* __restrict__ off, int H,
                                                         const int* __restrict__ hc, const int* __restrict__ best,
                                                         const unsigned char* __restrict__ mask, const double* __restrict__ part1,
                                                         double* __restrict__ part2) {
    __shared__ double scratch[SP_NT / 64];
    __shared__ double cs[3];
    const int s = blockIdx.y, b = best[s];
    if (b < 0) return;
    int64_t lo, hi;
    seg_range(off, s, N, lo, hi);
    if (threadIdx.x == 0) plane_centroid(part1, s, gridDim.x, hc[(int64_t)s * H + b], cs);
    __syncthreads();
    const double c[3] = {cs[0], cs[1], cs[2]};
    double C[6] = {0, 0, 0, 0, 0, 0};
    for (int64_t i = lo + (int64_t)blockIdx.x * SP_NT + threadIdx.x; i < hi; i += (int64_t)gridDim.x * SP_NT) {
        if (!mask[i]) continue;
        const double dx = pts[3 * i] - c[0], dy = pts[3 * i + 1] - c[1], dz = pts[3 * i + 2] - c[2];
        C[0] += dx * dx; C[1] += dx * dy; C[2] += dx * dz; C[3] += dy * dy; C[4] += dy * dz; C[5] += dz * dz;
    }
    for (int a = 0; a < 6; ++a) {
        const double r = block_sum<double, SP_NT>(C[a], scratch);
        if (threadIdx.x == 0) part2[((int64_t)s * gridDim.x + blockIdx.x) * 6 + a] = r;
    }
}

// one thread per segment: the refit from the block sums in block order, the count, the plane of zeros of a segment without a plane
__global__ __launch_bounds__(64) void k_plane_final(int S, int H, int B, const double* __restrict__ hp, const int* __restrict__ hc,
                                                    const int* __restrict__ best, const double* __restrict__ part1,
                                                    const double* __restrict__ part2, double* __restrict__ plane, int64_t* __restrict__ count) {
    const int s = blockIdx.x * 64 + threadIdx.x;
    if (s >= S) return;
    const int b = best[s];
    double pl[4] = {0, 0, 0, 0};
    int cnt = 0;
    if (b >= 0) {
        cnt = hc[(int64_t)s * H + b];
        double c[3], C[6] = {0, 0, 0, 0, 0, 0};
        plane_centroid(part1, s, B, cnt, c);
        for (int k = 0; k < B; ++k)
            for (int a = 0; a < 6; ++a) C[a] += part2[((int64_t)s * B + k) * 6 + a];
        if (!plane_from_moments(c, C, pl))                  // the inliers span less than a plane (or there are none): the hypothesis itself
            for (int a = 0; a < 4; ++a) pl[a] = hp[4 * ((int64_t)s * H + b) + a];
    }
    for (int a = 0; a < 4; ++a) plane[4 * s + a] = pl[a];
    count[s] = cnt;
}

static int sp_blocks(int64_t N, int S) {
    return (int)std::max<int64_t>(1, std::min<int64_t>((N + SP_TILE - 1) / SP_TILE, SP_MAX_BLOCKS / S));
}

}  // namespace creg
using namespace creg;

extern "C" size_t creg_depth_points_workspace_bytes(int32_t n_cams, int32_t width, int32_t height) {
    if (n_cams < 1 || width < 1 || height < 1) return 0;
    return sizeof(int64_t) * (size_t)n_cams * (size_t)(((int64_t)width * height + DP_NT - 1) / DP_NT);
}

extern "C" int creg_depth_points_count_f64(const double* depth, int32_t n_cams, int32_t width, int32_t height, int64_t* offsets,
                                           void* workspace, size_t workspace_bytes, creg_stream_t stream) {
    CREG_REQUIRE(depth && offsets && workspace, "creg_depth_points_count_f64: null pointer");
    CREG_REQUIRE(n_cams >= 1 && n_cams <= 65535 && width >= 1 && height >= 1 && (int64_t)width * height < (1ll << 31),
                 "creg_depth_points_count_f64: needs 1 <= n_cams <= 65535 and 1 <= width * height < 2^31");
    const size_t need = creg_depth_points_workspace_bytes(n_cams, width, height);
    CREG_REQUIRE(workspace_bytes >= need, "creg_depth_points_count_f64: workspace too small (%zu < %zu)", workspace_bytes, need);
    const int64_t HW = (int64_t)width * height;
    const int gx = cdiv(HW, DP_NT);
    hipStream_t s = (hipStream_t)stream;
    hipLaunchKernelGGL(k_depth_count, dim3(gx, n_cams), dim3(DP_NT), 0, s, depth, HW, (int64_t*)workspace);
    hipLaunchKernelGGL(k_depth_scan, dim3(1), dim3(DP_NT), 0, s, (int64_t*)workspace, (int64_t)gx * n_cams, gx, (int)n_cams, offsets);
    CREG_LAUNCH_CHECK();
    return CREG_OK;
}

extern "C" int creg_depth_points_f64(const double* depth, const double* cams, int32_t n_cams, double fov_deg, double aspect, int32_t width,
                                     int32_t height, const void* workspace, size_t workspace_bytes, double* points, int64_t capacity,
                                     creg_stream_t stream) {
    CREG_REQUIRE(depth && cams && workspace, "creg_depth_points_f64: null pointer");
    CREG_REQUIRE(n_cams >= 1 && n_cams <= 65535 && width >= 1 && height >= 1 && (int64_t)width * height < (1ll << 31) && fov_deg > 0 &&
                 fov_deg < 180 && capacity >= 0, "creg_depth_points_f64: bad argument");
    const size_t need = creg_depth_points_workspace_bytes(n_cams, width, height);
    CREG_REQUIRE(workspace_bytes >= need, "creg_depth_points_f64: workspace too small (%zu < %zu)", workspace_bytes, need);
    if (capacity == 0) return CREG_OK;
    CREG_REQUIRE(points, "creg_depth_points_f64: null pointer");
    const int64_t HW = (int64_t)width * height;
    BackProj c{tan(fov_deg * 3.14159265358979323846 / 360.0), aspect, width, height};
    hipLaunchKernelGGL(k_depth_scatter, dim3(cdiv(HW, DP_NT), n_cams), dim3(DP_NT), 0, (hipStream_t)stream, depth, cams, c,
                       (const int64_t*)workspace, points, capacity);
    CREG_LAUNCH_CHECK();
    return CREG_OK;
}

extern "C" size_t creg_segment_plane_workspace_bytes(int64_t n, int32_t n_segments, int32_t n_hyp) {
    if (n < 1 || n_segments < 1 || n_hyp < 1) return 0;
    const size_t SH = (size_t)n_segments * n_hyp, SB = (size_t)n_segments * sp_blocks(n, n_segments);
    return sizeof(double) * (4 * SH + 9 * SB) + sizeof(int32_t) * SH;
}

extern "C" int creg_segment_plane_f64(const double* points, int64_t n, const int64_t* offsets, int32_t n_segments, const int64_t* samples,
                                      int32_t n_hyp, int32_t ransac_n, double threshold, double* plane, uint8_t* mask, int64_t* count,
                                      int32_t* best, double* hyp_planes, int32_t* hyp_counts, void* workspace, size_t workspace_bytes,
                                      creg_stream_t stream) {
    CREG_REQUIRE(points && offsets && samples && plane && mask && count && best && workspace, "creg_segment_plane_f64: null pointer");
    CREG_REQUIRE(n >= 1 && n < (1ll << 31) && n_segments >= 1 && n_segments <= 65535 && n_hyp >= 1 && ransac_n >= 3 && ransac_n <= SP_MAX_N &&
                 threshold > 0, "creg_segment_plane_f64: needs 1 <= n < 2^31, 1 <= segments <= 65535, hypotheses >= 1, 3 <= ransac_n <= %d "
                 "and threshold > 0 (n = %lld, segments = %d, hypotheses = %d, ransac_n = %d)", SP_MAX_N, (long long)n, (int)n_segments,
                 (int)n_hyp, (int)ransac_n);
    const size_t need = creg_segment_plane_workspace_bytes(n, n_segments, n_hyp);
    CREG_REQUIRE(workspace_bytes >= need, "creg_segment_plane_f64: workspace too small (%zu < %zu)", workspace_bytes, need);
    const int S = n_segments, H = n_hyp, B = sp_blocks(n, S);
    const size_t SH = (size_t)S * H;
    double* ws = (double*)workspace;
    double* hp = hyp_planes ? hyp_planes : ws;
    double* part1 = ws + 4 * SH;
    double* part2 = part1 + 3 * (size_t)S * B;
    int* hc = hyp_counts ? hyp_counts : (int*)(part2 + 6 * (size_t)S * B);
    hipStream_t s = (hipStream_t)stream;
    CREG_HIP(hipMemsetAsync(mask, 0, (size_t)n, s));
    hipLaunchKernelGGL(k_plane_fit, dim3(cdiv(H, SP_NT), S), dim3(SP_NT), 0, s, points, n, offsets, samples, H, (int)ransac_n, hp, hc);
    hipLaunchKernelGGL(k_plane_count, dim3(B, S), dim3(SP_NT), 0, s, points, n, offsets, H, threshold, (const double*)hp, hc);
    hipLaunchKernelGGL(k_plane_select, dim3(S), dim3(SP_NT), 0, s, H, (const double*)hp, (const int*)hc, best);
    hipLaunchKernelGGL(k_plane_mask, dim3(B, S), dim3(SP_NT), 0, s, points, n, offsets, H, threshold, (const double*)hp, (const int*)best, mask, part1);
    hipLaunchKernelGGL(k_plane_scatter, dim3(B, S), dim3(SP_NT), 0, s, points, n, offsets, H, (const int*)hc, (const int*)best,
                       (const unsigned char*)mask, (const double*)part1, part2);
    hipLaunchKernelGGL(k_plane_final, dim3(cdiv(S, 64)), dim3(64), 0, s, S, H, B, (const double*)hp, (const int*)hc, (const int*)best,
                       (const double*)part1, (const double*)part2, plane, count);
    CREG_LAUNCH_CHECK();
    return CREG_OK;
}
