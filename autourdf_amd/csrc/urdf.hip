// urdf.hip -- N4: the graph half of the reference's URDF stage, fp64.  Replaces the link-discovery loop of
// PointCloud/coord_map.py (coord_clustering :70-111 called by silhouette_score_method :114-128, once per candidate
// link count) and the spatial MST of CoordMap.coord_mst (:334-349).
//
// Link discovery.  The reference lowers a threshold t from 1 by repeated float64 subtraction of 1e-4 and, at every
// step, rebuilds the graph {(i, j) : i < j, d[i][j] < t} and its connected components, until there are at least nl
// of them.  The components of {d < t} are exactly the components of MST(d) restricted to edges of weight < t (cut
// property, any MST), so one Prim MST per map answers every nl: with s the ascending MST weights, the component count
// at t is >= nl iff t <= s[K - nl], and the threshold used is the first lattice point at or below that weight.  The
// lattice is walked binade by binade: inside one binade every fl(t - 1e-4) moves t by the same multiple of the ulp
// (the exact difference rounds to the grid the binade shares), so a binade is one integer division, and each binade
// crossing is one real subtraction -- the same float64 values the reference's loop visits, in ~30 steps, not 10^4.
// Components are numbered by their smallest node (networkx.connected_components order) and scored with
// scikit-learn's precomputed silhouette (bincount-order cluster sums, intra / (n_c - 1), min inter mean, singleton 0,
// NaN 0, numpy's pairwise mean).
//
// One workgroup, one thread per node (K <= 256): Prim keeps its keys in registers and finds each next node with a
// wave64 shuffle argmin plus a 4-entry cross-wave step.  The map sits in LDS (row stride K + 1) up to K = 128.
// Latency-bound by construction: O(K^2) flops on at most 512 KB.
#include <climits>
#include "creg_common.h"

namespace creg {

constexpr int LS_NT = 256;          // one thread per node
constexpr int LS_MAX_K = 256;
constexpr int LS_LDS_K = 128;       // K x (K + 1) doubles in LDS up to here: 129 KB
constexpr double LS_STEP = 0.0001;  // the reference's decrement

// Prim over K nodes from node 0; w(i, j) is the edge weight (any symmetric accessor).  Every thread j < K returns
// the weight / parent of the edge that attached it (root: +inf / -1) and the iteration at which it was attached.
// Ties: the smallest node index among equal keys is attached first; a key is replaced only by a strictly smaller
// weight, so among equal-weight edges to the tree the one from the earliest attached node is kept.
template <class W>
__device__ void prim(int K, W w, double& ew, int& ep, int& order, double* redk, int* redi) {
    const int j = threadIdx.x, lane = j & 63, wv = j >> 6, nw = (blockDim.x + 63) >> 6;
    bool done = j == 0 || j >= K;
    double key = done ? INFINITY : w(0, j);
    int par = 0;
    ew = INFINITY; ep = -1; order = 0;
    for (int it = 1; it < K; ++it) {
        double bk = (done || key != key) ? INFINITY : key;
        int bi = done ? INT_MAX : j;
#pragma unroll
        for (int off = 32; off >= 1; off >>= 1) {
            const double ok = __shfl_xor(bk, off);
            const int oi = __shfl_xor(bi, off);
            if (ok < bk || (ok == bk && oi < bi)) { bk = ok; bi = oi; }
        }
        double* rk = redk + 4 * (it & 1);                 // double-buffered: one barrier per node
        int* ri = redi + 4 * (it & 1);
        if (lane == 0) { rk[wv] = bk; ri[wv] = bi; }
        __syncthreads();
        bk = rk[0]; bi = ri[0];
        for (int q = 1; q < nw; ++q)
            if (rk[q] < bk || (rk[q] == bk && ri[q] < bi)) { bk = rk[q]; bi = ri[q]; }
        const int u = bi;
        if (j == u) { done = true; ew = key; ep = par; order = it; }
        if (!done) {
            const double wu = w(u, j);
            if (wu < key) { key = wu; par = u; }
        }
    }
}

// First point of the lattice t_0 = 1, t_{k+1} = fl(t_k - 1e-4) at or below w (w >= 0 finite): returns t_k.
__device__ double lattice_first_at_or_below(double w) {
    double t = 1.0;
    for (int guard = 0; guard < 4096; ++guard) {
        if (t <= w) return t;
        int e;
        frexp(t, &e);                                     // t in [2^(e-1), 2^e)
        const double lo = ldexp(0.5, e), u = ldexp(1.0, e - 53);
        const double r = LS_STEP / u;                     // exact (power-of-two scaling)
        if (t - LS_STEP >= lo && r - floor(r) != 0.5) {   // the next step stays in this binade and rounds one way
            const int64_t D = (int64_t)rint(r), A = (int64_t)((t - lo) / u);
            const int64_t nmax = A / D;
            const double d = (double)D * u;
            int64_t n = (int64_t)ceil((t - w) / d) - 1;
            if (n < 0) n = 0;
            while (n > 0 && t - (double)(n - 1) * d <= w) --n;
            while (n <= nmax && t - (double)n * d > w) ++n;
            if (n <= nmax) return t - (double)n * d;
            t -= (double)nmax * d;
        }
        t = t - LS_STEP;                                  // one real step of the reference's loop (binade crossing)
    }
    return t;                                             // unreachable for w >= 0
}

__global__ __launch_bounds__(LS_NT) void k_link_sweep(const double* __restrict__ gD, int K, int nl_lo, int n_nl,
                                                      int32_t* __restrict__ labels, int32_t* __restrict__ n_comp,
                                                      double* __restrict__ thresholds, double* __restrict__ scores,
                                                      int32_t* __restrict__ best) {
    extern __shared__ __attribute__((aligned(16))) double sD[];     // [K][K + 1] when K <= LS_LDS_K
    __shared__ double s_ew[LS_MAX_K], s_ws[LS_MAX_K], s_thr[LS_MAX_K], s_sil[LS_MAX_K], s_sc[LS_MAX_K], redk[8];
    __shared__ int s_ep[LS_MAX_K], s_up[2][LS_MAX_K], s_mn[LS_MAX_K], s_lmin[LS_MAX_K], s_lab[LS_MAX_K],
        s_ord[LS_MAX_K], s_sz[LS_MAX_K], redi[8];
    __shared__ unsigned long long s_mask[4];
    const int j = threadIdx.x, lane = j & 63, wv = j >> 6, nw = (blockDim.x + 63) >> 6;
    const bool lds = K <= LS_LDS_K;
    const int ld = lds ? K + 1 : K;
    const double* D = lds ? sD : gD;
    if (lds)
        for (int p = j; p < K * K; p += blockDim.x) sD[(p / K) * ld + p % K] = gD[p];
    __syncthreads();
    auto wup = [&](int a, int b) { return a < b ? D[a * ld + b] : D[b * ld + a]; };   // strict upper triangle

    double ew; int ep, ord;
    prim(K, wup, ew, ep, ord, redk, redi);
    if (j < K) { s_ew[j] = ew; s_ep[j] = ep; }
    __syncthreads();
    if (j >= 1 && j < K) {                                // ascending MST weights (stable rank sort)
        int r = 0;
        for (int i = 1; i < K; ++i) r += s_ew[i] < ew || (s_ew[i] == ew && i < j);
        s_ws[r] = ew;
    }
    __syncthreads();
    if (j < n_nl) {
        const int nl = nl_lo + j;
        const double t = nl <= 1 ? 1.0 : lattice_first_at_or_below(s_ws[K - nl]);
        s_thr[j] = t;
        thresholds[j] = t;
    }
    __syncthreads();

    bool invalid = false;
    for (int n = 0; n < n_nl; ++n) {
        const double t = s_thr[n];
        // components of MST edges < t: every node jumps to its topmost ancestor reachable through such edges
        if (j < K) { s_up[0][j] = (j != 0 && s_ew[j] < t) ? s_ep[j] : j; s_mn[j] = INT_MAX; }
        __syncthreads();
#pragma unroll 1
        for (int r = 0; r < 8; ++r) {                     // 2^8 >= the deepest path (K - 1)
            if (j < K) s_up[(r + 1) & 1][j] = s_up[r & 1][s_up[r & 1][j]];
            __syncthreads();
        }
        const int rep = j < K ? s_up[0][j] : 0;
        if (j < K) atomicMin(&s_mn[rep], j);
        __syncthreads();
        const int mn = j < K ? s_mn[rep] : INT_MAX;
        const unsigned long long m = __ballot(j < K && mn == j);
        if (lane == 0) s_mask[wv] = m;
        __syncthreads();
        int pre = 0, nc = 0;
        for (int q = 0; q < nw; ++q) {
            const int c = __popcll(s_mask[q]);
            nc += c;
            if (q < wv) pre += c;
        }
        pre += __popcll(m & ((1ull << lane) - 1ull));
        if (j < K && mn == j) { s_lmin[j] = pre; s_sz[pre] = 0; }
        __syncthreads();
        const int li = j < K ? s_lmin[mn] : 0;
        if (j < K) { s_lab[j] = li; labels[(size_t)n * K + j] = li; atomicAdd(&s_sz[li], 1); }
        if (j == 0) n_comp[n] = nc;
        __syncthreads();
        if (nc < 2 || nc >= K) {                          // sklearn: 2 <= n_labels <= n_samples - 1
            invalid = true;
            if (j == 0) s_sc[n] = NAN;
            continue;                                     // uniform: nc is the same in every thread
        }
        if (j < K) {                                      // (label, index) order: bincount's summation order per cluster
            int r = 0;
            for (int i = 0; i < K; ++i) r += s_lab[i] < li || (s_lab[i] == li && i < j);
            s_ord[r] = j;
        }
        __syncthreads();
        if (j < K) {
            double s = 0.0, intra = 0.0, inter = INFINITY;
            const double* row = D + (size_t)j * ld;
            for (int p = 0; p < K; ++p) {
                const int mm = s_ord[p], c = s_lab[mm];
                s += row[mm];
                if (p == K - 1 || s_lab[s_ord[p + 1]] != c) {
                    if (c == li) intra = s;
                    else inter = fmin(inter, s / (double)s_sz[c]);
                    s = 0.0;
                }
            }
            const int nli = s_sz[li];
            const double a = intra / (double)(nli - 1);
            double sil = (inter - a) / (a > inter ? a : inter);
            if (nli <= 1 || sil != sil) sil = 0.0;
            s_sil[j] = sil;
        }
        __syncthreads();
        if (j == 0) {                                     // np.mean: numpy's pairwise sum (blocks of 128, 8 accumulators)
            double tot = 0.0;
            const int n2 = K <= 128 ? K : ((K / 2) - (K / 2) % 8);
            for (int part = 0; part < (K <= 128 ? 1 : 2); ++part) {
                const double* a = s_sil + (part ? n2 : 0);
                const int len = part ? K - n2 : n2;
                double res;
                if (len < 8) {
                    res = -0.0;
                    for (int i = 0; i < len; ++i) res += a[i];
                } else {
                    double rr[8];
                    for (int q = 0; q < 8; ++q) rr[q] = a[q];
                    int i = 8;
                    for (; i < len - (len % 8); i += 8)
                        for (int q = 0; q < 8; ++q) rr[q] += a[i + q];
                    res = ((rr[0] + rr[1]) + (rr[2] + rr[3])) + ((rr[4] + rr[5]) + (rr[6] + rr[7]));
                    for (; i < len; ++i) res += a[i];
                }
                tot = part ? tot + res : res;
            }
            s_sc[n] = tot / (double)K;
        }
        __syncthreads();
    }
    if (j == 0) {
        int b = 0;
        for (int n = 0; n < n_nl; ++n) {
            scores[n] = s_sc[n];
            if (s_sc[n] > s_sc[b]) b = n;                 // np.argmax: first maximum
        }
        *best = invalid ? -1 : b;
    }
}

// coord_mst: xyz summed over the T steps, Euclidean distances, Prim.  Edges come out in the order Prim attaches them.
__global__ __launch_bounds__(LS_NT) void k_coord_mst(const double* __restrict__ coords, int T, int K,
                                                     int32_t* __restrict__ edges, double* __restrict__ weights) {
    __shared__ double P[LS_MAX_K][3], redk[8];
    __shared__ int redi[8];
    const int j = threadIdx.x;
    if (j < K) {
        double x = 0.0, y = 0.0, z = 0.0;
        for (int t = 0; t < T; ++t) {
            const double* c = coords + ((size_t)t * K + j) * 7;
            x += c[0]; y += c[1]; z += c[2];
        }
        P[j][0] = x; P[j][1] = y; P[j][2] = z;
    }
    __syncthreads();
    auto wd = [&](int a, int b) {
        const double dx = P[a][0] - P[b][0], dy = P[a][1] - P[b][1], dz = P[a][2] - P[b][2];
        return sqrt((dx * dx + dy * dy) + dz * dz);
    };
    double ew; int ep, ord;
    prim(K, wd, ew, ep, ord, redk, redi);
    if (j >= 1 && j < K) {
        edges[2 * (ord - 1)] = ep;
        edges[2 * (ord - 1) + 1] = j;
        weights[ord - 1] = ew;
    }
}

}  // namespace creg
using namespace creg;

extern "C" int creg_link_sweep_f64(const double* d_map, int32_t K, int32_t nl_lo, int32_t nl_hi, int32_t* labels,
                                   int32_t* n_comp, double* thresholds, double* scores, int32_t* best,
                                   creg_stream_t stream) {
    CREG_REQUIRE(d_map && labels && n_comp && thresholds && scores && best, "creg_link_sweep_f64: null pointer");
    CREG_REQUIRE(K >= 2 && K <= LS_MAX_K, "creg_link_sweep_f64: K must be in [2, %d] (K=%d)", LS_MAX_K, K);
    CREG_REQUIRE(nl_lo >= 1 && nl_lo < nl_hi && nl_hi <= K + 1, "creg_link_sweep_f64: bad link-count range [%d, %d) for K=%d",
                 nl_lo, nl_hi, K);
    const size_t smem = K <= LS_LDS_K ? sizeof(double) * (size_t)K * (K + 1) : 0;
    // per device, not per process: set on every call (a cached flag would leave a second GPU at the 64 KB default)
    CREG_HIP(hipFuncSetAttribute((const void*)k_link_sweep, hipFuncAttributeMaxDynamicSharedMemorySize,
                                 (int)(sizeof(double) * LS_LDS_K * (LS_LDS_K + 1))));
    hipLaunchKernelGGL(k_link_sweep, dim3(1), dim3(K <= 64 ? 64 : LS_NT), smem, (hipStream_t)stream, d_map, K, nl_lo,
                       nl_hi - nl_lo, labels, n_comp, thresholds, scores, best);
    CREG_LAUNCH_CHECK();
    return CREG_OK;
}

extern "C" int creg_coord_mst_f64(const double* coords, int32_t T, int32_t K, int32_t* edges, double* weights,
                                  creg_stream_t stream) {
    CREG_REQUIRE(coords && edges && weights, "creg_coord_mst_f64: null pointer");
    CREG_REQUIRE(K >= 2 && K <= LS_MAX_K && T >= 1, "creg_coord_mst_f64: bad size (T=%d, K=%d)", T, K);
    hipLaunchKernelGGL(k_coord_mst, dim3(1), dim3(K <= 64 ? 64 : LS_NT), 0, (hipStream_t)stream, coords, T, K, edges,
                       weights);
    CREG_LAUNCH_CHECK();
    return CREG_OK;
}
