// group.hip -- the stable grouping / change-of-frame step that follows the k-means of a resample (reference mlp_reg.py:208-217):
// the points of a frame gathered by label, in index order inside a label, each transformed by the inverse pose of its cluster.
#include "creg_common.h"
#include "creg_dev.h"

namespace creg {

// ---- grouping by label + inverse-pose change of frame ------------------------------------------
// Every index is a compile-time constant (round 5): the row exchange of the partial pivoting is a conditional swap of the pivot row
// with each later row in turn -- as a run-time row index it put the 4 x 8 matrix into scratch memory (272 bytes per lane, 93 scratch
// instructions in k_group_scatter / k_group_scatter_big).  Same operations in the same order: bit-identical.
__device__ __forceinline__ void inv4x4(const double* M, double* I) {      // Gauss-Jordan, partial pivoting
    double a[4][8];
#pragma unroll
    for (int r = 0; r < 4; ++r)
#pragma unroll
        for (int c = 0; c < 4; ++c) { a[r][c] = M[4 * r + c]; a[r][4 + c] = (r == c) ? 1.0 : 0.0; }
#pragma unroll
    for (int c = 0; c < 4; ++c) {
        int p = c;                                        // first row of the largest |entry| in column c, rows c .. 3
        double best = fabs(a[c][c]);
#pragma unroll
        for (int r = c + 1; r < 4; ++r) { const double v = fabs(a[r][c]); if (v > best) { best = v; p = r; } }
#pragma unroll
        for (int r = c + 1; r < 4; ++r) {
            const bool sw = p == r;
#pragma unroll
            for (int q = 0; q < 8; ++q) { const double t = a[c][q], u = a[r][q]; a[c][q] = sw ? u : t; a[r][q] = sw ? t : u; }
        }
        const double inv = 1.0 / a[c][c];
#pragma unroll
        for (int q = 0; q < 8; ++q) a[c][q] *= inv;
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            if (r == c) continue;
            const double fct = a[r][c];
#pragma unroll
            for (int q = 0; q < 8; ++q) a[r][q] = fma(-fct, a[c][q], a[r][q]);
        }
    }
#pragma unroll
    for (int r = 0; r < 4; ++r)
#pragma unroll
        for (int c = 0; c < 4; ++c) I[4 * r + c] = a[r][4 + c];
}

// grid.y = problem of a batch (the per-frame pointers come from the table)
constexpr int GRP_MAXB = 16;
struct GroupBatch { const double* X[GRP_MAXB]; const int* labels[GRP_MAXB]; const double* M[GRP_MAXB]; double* out[GRP_MAXB]; int* off[GRP_MAXB]; };

__global__ __launch_bounds__(1024) void k_group_offsets(GroupBatch G, int n, int k) {
    const int* __restrict__ labels = G.labels[blockIdx.y];
    int* __restrict__ off = G.off[blockIdx.y];
    extern __shared__ __attribute__((aligned(16))) char smem[];
    int* cnt = (int*)smem;
    for (int j = threadIdx.x; j <= k; j += 1024) cnt[j] = 0;
    __syncthreads();
    for (int i = threadIdx.x; i < n; i += 1024) atomicAdd(&cnt[labels[i]], 1);
    __syncthreads();
    if (threadIdx.x == 0) {
        int run = 0;
        for (int j = 0; j < k; ++j) { const int c = cnt[j]; off[j] = run; run += c; }
        off[k] = run;
    }
}

// one wave per cluster walks the labels in order: ballot + prefix popcount gives the stable slot
__global__ __launch_bounds__(64) void k_group_scatter(GroupBatch G, int n, int m_is_inverse) {
    const double* __restrict__ X = G.X[blockIdx.y];
    const int* __restrict__ labels = G.labels[blockIdx.y];
    const int* __restrict__ off = G.off[blockIdx.y];
    const double* __restrict__ M = G.M[blockIdx.y];
    double* __restrict__ out = G.out[blockIdx.y];
    const int j = blockIdx.x, lane = threadIdx.x;
    __shared__ double I[16];                              // inv(M_j), by one lane (no device scratch)
    if (m_is_inverse) { if (lane < 16) I[lane] = M[16 * j + lane]; }     // the caller inverted the pose (np.linalg.inv on the host)
    else if (lane == 0) inv4x4(M + 16 * j, I);
    __syncthreads();
    int pos = off[j];
    for (int base = 0; base < n; base += 64) {
        const int i = base + lane;
        const bool mine = (i < n) && (labels[i] == j);
        const unsigned long long m = __ballot(mine);
        if (mine) {
            const int slot = pos + __popcll(m & ((1ull << lane) - 1ull));
            const double p0 = X[3 * (size_t)i], p1 = X[3 * (size_t)i + 1], p2 = X[3 * (size_t)i + 2];
#pragma unroll
            for (int a = 0; a < 3; ++a)
                out[3 * (size_t)slot + a] = fma(I[4 * a + 2], p2, fma(I[4 * a + 1], p1, I[4 * a] * p0)) + I[4 * a + 3];
        }
        pos += __popcll(m);
    }
}

// ---- the same grouping for large frames (n > 16384): counts over many workgroups, one 1024-thread workgroup per cluster
// for the ordered compaction (the one-wave-per-cluster walk above took 1.85 ms at n = 262144, k = 128) ----
__global__ __launch_bounds__(1024) void k_group_count(const int* __restrict__ labels, int n, int k, int* __restrict__ off) {
    extern __shared__ __attribute__((aligned(16))) char smem[];
    int* cnt = (int*)smem;
    for (int j = threadIdx.x; j < k; j += 1024) cnt[j] = 0;
    __syncthreads();
    const int i0 = blockIdx.x * 4096 + threadIdx.x;
#pragma unroll
    for (int q = 0; q < 4; ++q) { const int i = i0 + 1024 * q; if (i < n) atomicAdd(&cnt[labels[i]], 1); }
    __syncthreads();
    for (int j = threadIdx.x; j < k; j += 1024) { const int c = cnt[j]; if (c) atomicAdd(&off[j + 1], c); }      // integers: order independent
}

// off[0] = 0, off[j + 1] = count of cluster j  ->  off[j + 1] = sum of the counts up to j  (k <= 4096: four per thread)
__global__ __launch_bounds__(1024) void k_group_excl(int* __restrict__ off, int k) {
    __shared__ int wsum[16];
    const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
    int c[4], run = 0;
#pragma unroll
    for (int q = 0; q < 4; ++q) { const int j = 4 * tid + q; c[q] = j < k ? off[j + 1] : 0; run += c[q]; }
    int inc = run;
    for (int o = 1; o < 64; o <<= 1) { const int t = __shfl_up(inc, o, 64); if (lane >= o) inc += t; }
    if (lane == 63) wsum[wv] = inc;
    __syncthreads();
    int base = inc - run;
    for (int w = 0; w < wv; ++w) base += wsum[w];
#pragma unroll
    for (int q = 0; q < 4; ++q) { const int j = 4 * tid + q; base += c[q]; if (j < k) off[j + 1] = base; }
    if (tid == 0) off[0] = 0;
}

__global__ __launch_bounds__(1024) void k_group_scatter_big(const double* __restrict__ X, int n, const int* __restrict__ labels,
                                                            const int* __restrict__ off, const double* __restrict__ M,
                                                            double* __restrict__ out, int m_is_inverse) {
    const int j = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
    __shared__ double I[16];
    __shared__ int wtot[2][16];
    if (m_is_inverse) { if (tid < 16) I[tid] = M[16 * j + tid]; }
    else if (tid == 0) inv4x4(M + 16 * j, I);
    __syncthreads();
    int pos = off[j];
    for (int base = 0, r = 0; base < n; base += 4096, ++r) {
        const int i0 = base + 4 * tid;                        // four consecutive points per thread: slots stay in index order
        bool fl[4];
        int c = 0;
#pragma unroll
        for (int q = 0; q < 4; ++q) { fl[q] = (i0 + q < n) && labels[min(i0 + q, n - 1)] == j; c += fl[q]; }
        int inc = c;
        for (int o = 1; o < 64; o <<= 1) { const int t = __shfl_up(inc, o, 64); if (lane >= o) inc += t; }
        if (lane == 63) wtot[r & 1][wv] = inc;
        __syncthreads();                                      // one barrier per round: the table alternates
        int before = 0, total = 0;
#pragma unroll
        for (int w = 0; w < 16; ++w) { const int v = wtot[r & 1][w]; before += w < wv ? v : 0; total += v; }
        int slot = pos + before + inc - c;
#pragma unroll
        for (int q = 0; q < 4; ++q)
            if (fl[q]) {
                const size_t i = (size_t)(i0 + q);
                const double p0 = X[3 * i], p1 = X[3 * i + 1], p2 = X[3 * i + 2];
#pragma unroll
                for (int a = 0; a < 3; ++a)
                    out[3 * (size_t)slot + a] = fma(I[4 * a + 2], p2, fma(I[4 * a + 1], p1, I[4 * a] * p0)) + I[4 * a + 3];
                ++slot;
            }
        pos += total;
    }
}

}  // namespace creg
using namespace creg;

extern "C" int creg_group_to_local_f64(const double* X, int64_t n, const int32_t* labels, int32_t k,
                                       const double* M, int32_t m_is_inverse, double* out_local,
                                       int32_t* seg_offsets, creg_stream_t stream) {
    CREG_REQUIRE(X && labels && M && out_local && seg_offsets && n >= 1 && n < (1ll << 31) && k >= 1 && k <= 4096,
                 "creg_group_to_local_f64: bad argument");
    hipStream_t s = (hipStream_t)stream;
    GroupBatch G;
    G.X[0] = X; G.labels[0] = labels; G.M[0] = M; G.out[0] = out_local; G.off[0] = seg_offsets;
    if (n > 16384) {                                           // large frames: many-workgroup count, workgroup-per-cluster compaction
        CREG_HIP(hipMemsetAsync(seg_offsets, 0, sizeof(int) * ((size_t)k + 1), s));
        hipLaunchKernelGGL(k_group_count, dim3(cdiv(n, 4096)), dim3(1024), sizeof(int) * k, s, labels, (int)n, k, seg_offsets);
        hipLaunchKernelGGL(k_group_excl, dim3(1), dim3(1024), 0, s, seg_offsets, k);
        hipLaunchKernelGGL(k_group_scatter_big, dim3(k), dim3(1024), 0, s, X, (int)n, labels, seg_offsets, M, out_local, m_is_inverse);
        CREG_LAUNCH_CHECK();
        return CREG_OK;
    }
    hipLaunchKernelGGL(k_group_offsets, dim3(1, 1), dim3(1024), sizeof(int) * (k + 1), s, G, (int)n, k);
    hipLaunchKernelGGL(k_group_scatter, dim3(k, 1), dim3(64), 0, s, G, (int)n, m_is_inverse);
    CREG_LAUNCH_CHECK();
    return CREG_OK;
}

extern "C" int creg_group_to_local_batch_f64(const double* const* X, int64_t n, const int32_t* const* labels, int32_t k,
                                             const double* const* M, int32_t m_is_inverse, int32_t batch,
                                             double* const* out_local, int32_t* const* seg_offsets, creg_stream_t stream) {
    CREG_REQUIRE(X && labels && M && out_local && seg_offsets && n >= 1 && n < (1ll << 31) && k >= 1 && k <= 4096,
                 "creg_group_to_local_batch_f64: bad argument");
    CREG_REQUIRE(batch >= 1 && batch <= GRP_MAXB, "creg_group_to_local_batch_f64: batch must be in 1..%d", GRP_MAXB);
    GroupBatch G;
    for (int b = 0; b < batch; ++b) {
        CREG_REQUIRE(X[b] && labels[b] && M[b] && out_local[b] && seg_offsets[b], "creg_group_to_local_batch_f64: null pointer in problem %d", b);
        G.X[b] = X[b]; G.labels[b] = labels[b]; G.M[b] = M[b]; G.out[b] = out_local[b]; G.off[b] = seg_offsets[b];
    }
    hipStream_t s = (hipStream_t)stream;
    hipLaunchKernelGGL(k_group_offsets, dim3(1, batch), dim3(1024), sizeof(int) * (k + 1), s, G, (int)n, k);
    hipLaunchKernelGGL(k_group_scatter, dim3(k, batch), dim3(64), 0, s, G, (int)n, m_is_inverse);
    CREG_LAUNCH_CHECK();
    return CREG_OK;
}
