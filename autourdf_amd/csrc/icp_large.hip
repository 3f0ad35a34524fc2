// icp_large.hip -- K4, many-workgroup regime: the seven kernels, the host driver of one problem, and the entries that read
// this unit's __device__ symbols (the counters hook, the debug builds' read-backs) or launch its kernels (creg_aabb_mask_f64).
#include <type_traits>
#include "icp_dev.h"

namespace creg {

// =================================================================================================================
// Large regime (clusters of more than ICP_SRC_LDS points, or frames whose masked targets do not fit a CU's LDS: the
// BASELINE configs[4] shape has 2048-point clusters against ~3000 masked targets each): the same ICP as k_masked_icp's
// fast path -- binned targets and sources, exact search pruned by the previous match, one-pass shifted moments --
// iteration by iteration over MANY workgroups instead of one workgroup per cluster.  The bins are a 16 x 16 grid over the
// box's two longest edges (a cluster is a surface patch: slabs along one axis pruned 2.5x at this size, the grid ~12x).
//   k_icp_mask    (cluster)           box; frame indices inside it, grouped by grid cell (count pass + scatter pass), or in
//                                     ascending order for creg_aabb_mask_f64
//   k_icp_init    (cluster)           sources into the world frame with the initial pose, stable-sorted by cell
//   k_icp_pool    (cluster, slices)   the masked targets' coordinates, in cell order, into a pool (coalesced staging)
//   k_icp_nn      (64-source chunk)   applies the pending rigid update to its sources; nearest masked target of each: a wave =
//                                     16 consecutive sorted sources x 4 lanes, the lanes of a source walking the grid rows of
//                                     the cell rectangle the wave's (x - r, x + r) squares touch (r = distance to the
//                                     previous match); the chunk's moments; and, in the cluster's LAST chunk to finish, the
//                                     fit (one wave): chunk moments in chunk order -> fitness / RMSE, open3d's convergence
//                                     test against the previous ones, else Horn's closed form: new pose, pending update
//   k_icp_compact (one workgroup)     between batches: the chunks of the clusters still iterating (the next batch's grid)
//   k_icp_finish  (cluster)           outputs
// The host enqueues the search in batches of 16 and reads "clusters / chunks still running" between batches.
typedef float nn_f2 __attribute__((ext_vector_type(2)));          // (v_pk_* float32 pairs: the screen of k_icp_nn)
struct IcpLarge {                          // per problem
    const double* local; const float* world; const int* off; const int* woff; const double* frame; const double* Min;
    const int* toff;                           // point-to-point mode: cluster c's targets are frame[toff[c] .. toff[c + 1]), no mask; null = masked mode
    double* Mout; double* world_out; int* n_iter_out;
    double* srcw; int* tidx; int* tcount; float* box; int* nn; double* part; double* state; int* running;
    int* chunk0;                               // [k + 1] first source chunk of every cluster (k_icp_nn's block -> cluster map)
    int* tst;                                  // [k][ICP_NCELL + 1] first target of every cell, row-major in (a, b), g x g used (binned mode)
    int* chunk_cl;                             // [chunks] cluster of every chunk (k_icp_nn's block -> cluster map)
    double* prevt;                             // [n][3] coordinates of every source's current match (the next search's bound)
    double* tcx; double* tcy; double* tcz;     // pool of the clusters' masked target coordinates in cell order (coalesced staging)
    float4* tcf;                               // the same entries as (float32 coordinates relative to the cluster's box centre, frame index): what the screen stages
    unsigned* tlmax;                           // [k] bits of the largest |coordinate - box centre| among a cluster's masked targets (float32, rounded up)
    int* tbase;                                // [k] a cluster's first pool entry, -1: did not fit (its targets are gathered through tidx)
    int* arrive;                               // [k] chunks of the cluster that have finished the running search
    int* live;                                 // [chunks] chunks of the clusters still iterating (k_icp_compact), read when `use_live`
    int use_live;
    int pool_cap;
    int screen;                                // k_icp_nn: float32 screen in front of the fp64 scan (0: measurement / identity knob)
};
constexpr int ICP_CH = 64;                 // sources per k_icp_nn workgroup (4 waves of 16)
#ifndef ICP_LG
#define ICP_LG 2                           // log2 of the lanes that share one source point in k_icp_nn (measured at configs[4], 12 frames:
                                           // 4 lanes 38.5 ms per frame, 8 lanes (-DICP_LG=3) 43.6)
#endif
constexpr int ICP_G = 1 << ICP_LG;         // lane groups of a wave = lanes per source
constexpr int ICP_SPW = 64 >> ICP_LG;      // sources per wave
constexpr int ICP_NNW = ICP_CH / ICP_SPW;  // waves of a k_icp_nn workgroup
#ifndef ICP_SB_N
#define ICP_SB_N 64
#endif
constexpr int ICP_SB = ICP_SB_N;           // targets a lane group stages per batch (128 measured no better)
constexpr int ICP_ST = 48;                 // doubles of per-cluster state: T[16] U[16] prev_fit prev_rmse done n_updates | a: x0 inv_w axis | shc[3] | b: x0 inv_w axis | g
constexpr int ICP_NM = 17;                 // moments per chunk: count, sum d2, sum (s - shc), sum (d - shc), sum (s - shc)(d - shc)^T
constexpr int ICP_GMAX = 64;               // the grid over the box's longest (a) and second longest (b) edge has g x g cells, g per
constexpr int ICP_NCELL = ICP_GMAX * ICP_GMAX;      // cluster by its size: ~8 sources (~12 targets) per cell, 8 <= g <= 64
__device__ __forceinline__ int icp_grid_dim(int ns) {
    int g = (int)ceil(sqrt((double)ns / 8.0));
    return g < 8 ? 8 : (g > ICP_GMAX ? ICP_GMAX : g);
}
__device__ __forceinline__ int icp_bin(double x, double x0, double inv_w, int nbin) { return (int)fmin(fmax((x - x0) * inv_w, 0.0), (double)(nbin - 1)); }

// binned = 0: ascending compaction into tidx / tcount (creg_aabb_mask_f64, the G9 golden).
// binned = 1: tidx holds the same indices grouped by slab (any order inside one), tst the slab starts, state the binning.
__global__ __launch_bounds__(1024) void k_icp_mask(IcpLarge P, int nf, float half_scale, int from_pose, int binned) {
    __shared__ float wl[16][3], wh[16][3];
    __shared__ float s_lo[3], s_hi[3];
    __shared__ int s_wofs[16];
    __shared__ int cnt[ICP_NCELL + 1], fill[ICP_NCELL];
    const int k = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
    const int b = P.off[k], e = P.off[k + 1];
    float lo[3] = {INFINITY, INFINITY, INFINITY}, hi[3] = {-INFINITY, -INFINITY, -INFINITY};
    const int* toff = P.toff;                  // block-uniform
    if (toff) {                                // point-to-point mode: no mask; the cells need the extent of the cluster's own target segment
        for (int j = toff[k] + tid; j < toff[k + 1]; j += 1024)           // (any box is correct: the binning clamps and is monotone)
            for (int d = 0; d < 3; ++d) { const float v = (float)P.frame[3 * (size_t)j + d]; lo[d] = fminf(lo[d], v); hi[d] = fmaxf(hi[d], v); }
    } else if (!from_pose) {
        const int* woff = P.woff ? P.woff : P.off;
        for (int i = woff[k] + tid; i < woff[k + 1]; i += 1024)
            for (int d = 0; d < 3; ++d) { const float v = P.world[3 * (size_t)i + d]; lo[d] = fminf(lo[d], v); hi[d] = fmaxf(hi[d], v); }
    } else {                                   // boxes of float32(M) . float32(local), creg_cluster_transform_f32's arithmetic
        float Tf[12];
        for (int q = 0; q < 12; ++q) Tf[q] = (float)P.Min[16 * k + q];
        for (int i = b + tid; i < e; i += 1024) {
            const float p0 = (float)P.local[3 * (size_t)i], p1 = (float)P.local[3 * (size_t)i + 1], p2 = (float)P.local[3 * (size_t)i + 2];
            for (int d = 0; d < 3; ++d) {
                const float v = fmaf(p2, Tf[4 * d + 2], fmaf(p1, Tf[4 * d + 1], p0 * Tf[4 * d])) + Tf[4 * d + 3];
                lo[d] = fminf(lo[d], v); hi[d] = fmaxf(hi[d], v);
            }
        }
    }
    for (int d = 0; d < 3; ++d) {
        for (int o = 32; o >= 1; o >>= 1) { lo[d] = fminf(lo[d], __shfl_xor(lo[d], o, 64)); hi[d] = fmaxf(hi[d], __shfl_xor(hi[d], o, 64)); }
        if (lane == 0) { wl[wv][d] = lo[d]; wh[wv][d] = hi[d]; }
    }
    for (int q = tid; q <= ICP_NCELL; q += 1024) cnt[q] = 0;
    for (int q = tid; q < ICP_NCELL; q += 1024) fill[q] = 0;
    __syncthreads();
    if (tid < 3) {
        const int d = tid;
        float l = wl[0][d], h = wh[0][d];
        for (int w = 1; w < 16; ++w) { l = fminf(l, wl[w][d]); h = fmaxf(h, wh[w][d]); }
        if (toff) {
            //  point-to-point mode: l / h are float32 ROUNDINGS of the fp64 targets, which can lie half an ulp outside them -- the
            // float32 screen of k_icp_nn takes its length bound from this box ("the box holds the targets"): one ulp outwards makes that true;
            // an EMPTY target segment (+inf / -inf) would give a NaN centre and an infinite bound: a point box at the origin instead
            if (!(l <= h)) { l = 0.f; h = 0.f; }
            else { l = nextafterf(l, -INFINITY); h = nextafterf(h, INFINITY); }
        }
        const float c = (l + h) / 2.0f, sz = h - l;
        s_lo[d] = toff ? l : c - half_scale * sz; s_hi[d] = toff ? h : c + half_scale * sz;
        if (P.box) { P.box[6 * k + d] = s_lo[d]; P.box[6 * k + 3 + d] = s_hi[d]; }
    }
    __syncthreads();
    const double blo0 = (double)s_lo[0], blo1 = (double)s_lo[1], blo2 = (double)s_lo[2];
    const double bhi0 = (double)s_hi[0], bhi1 = (double)s_hi[1], bhi2 = (double)s_hi[2];
    int* tidx = P.tidx + (size_t)k * nf;
    if (binned) {
        // cells over the two longest edges of the box (a surface patch is two-dimensional: the third edge prunes nothing)
        float ext[3] = {s_hi[0] - s_lo[0], s_hi[1] - s_lo[1], s_hi[2] - s_lo[2]};
        int axa = 0;
        for (int d = 1; d < 3; ++d) if (ext[d] > ext[axa]) axa = d;
        int axb = axa == 0 ? 1 : 0;
        for (int d = 0; d < 3; ++d) if (d != axa && ext[d] > ext[axb]) axb = d;
        const int gd = icp_grid_dim(e - b), ncell = gd * gd;
        const double x0a = (double)s_lo[axa], inv_a = ext[axa] > 0.f && ext[axa] < INFINITY ? (double)gd / (double)ext[axa] : 0.0;
        const double x0b = (double)s_lo[axb], inv_b = ext[axb] > 0.f && ext[axb] < INFINITY ? (double)gd / (double)ext[axb] : 0.0;
        const int j0 = toff ? toff[k] : 0, nfe = e > b ? (toff ? toff[k + 1] : nf) : j0;
        __shared__ int wsum[16];
        for (int pass = 0; pass < 2; ++pass) {
            for (int j = j0 + tid; j < nfe; j += 1024) {
                const double p[3] = {P.frame[3 * (size_t)j], P.frame[3 * (size_t)j + 1], P.frame[3 * (size_t)j + 2]};
                if (toff || (p[0] > blo0 && p[0] < bhi0 && p[1] > blo1 && p[1] < bhi1 && p[2] > blo2 && p[2] < bhi2)) {
                    const double ca = axa == 0 ? p[0] : (axa == 1 ? p[1] : p[2]), cb = axb == 0 ? p[0] : (axb == 1 ? p[1] : p[2]);
                    const int cell = icp_bin(ca, x0a, inv_a, gd) * gd + icp_bin(cb, x0b, inv_b, gd);
                    if (pass == 0) atomicAdd(&cnt[cell], 1);
                    else tidx[cnt[cell] + atomicAdd(&fill[cell], 1)] = j;
                }
            }
            __syncthreads();
            if (pass == 0) {                          // exclusive prefix over the cells: four per thread, wave scans, wave totals
                int c4[4], run4 = 0;
                for (int q = 0; q < 4; ++q) { c4[q] = 4 * tid + q < ncell ? cnt[4 * tid + q] : 0; run4 += c4[q]; }
                int inc = run4;
                for (int o = 1; o < 64; o <<= 1) { const int t = __shfl_up(inc, o, 64); if (lane >= o) inc += t; }
                if (lane == 63) wsum[wv] = inc;
                __syncthreads();
                int acc = inc - run4, total = 0;
                for (int w = 0; w < 16; ++w) { const int t = wsum[w]; acc += w < wv ? t : 0; total += t; }
                for (int q = 0; q < 4; ++q) { if (4 * tid + q < ncell) cnt[4 * tid + q] = acc; acc += c4[q]; }
                if (tid == 0) cnt[ncell] = total;
                __syncthreads();
            }
        }
        for (int q = tid; q <= ncell; q += 1024) P.tst[(size_t)k * (ICP_NCELL + 1) + q] = cnt[q];
        if (tid == 0) {
            P.tcount[k] = cnt[ncell];
            double* st = P.state + ICP_ST * k;
            st[36] = x0a; st[37] = inv_a; st[38] = (double)axa;
            st[39] = 0.5 * (blo0 + bhi0); st[40] = 0.5 * (blo1 + bhi1); st[41] = 0.5 * (blo2 + bhi2);
            st[42] = x0b; st[43] = inv_b; st[44] = (double)axb; st[45] = (double)gd;
        }
        return;
    }
    int run = 0;
    for (int base = 0; base < nf; base += 1024) {
        const int j = base + tid;
        bool in = false;
        if (j < nf && e > b) {
            const double x = P.frame[3 * (size_t)j], y = P.frame[3 * (size_t)j + 1], z = P.frame[3 * (size_t)j + 2];
            in = x > blo0 && x < bhi0 && y > blo1 && y < bhi1 && z > blo2 && z < bhi2;
        }
        const unsigned long long m = __ballot(in);
        __syncthreads();
        if (lane == 0) s_wofs[wv] = __popcll(m);
        __syncthreads();
        int before = run, total = 0;
        for (int w = 0; w < 16; ++w) { const int c = s_wofs[w]; before += w < wv ? c : 0; total += c; }
        if (in) tidx[before + __popcll(m & ((1ull << lane) - 1ull))] = j;
        run += total;
    }
    if (tid == 0) P.tcount[k] = run;
}

// one workgroup per cluster: sources with the initial pose, stable-sorted by grid cell into srcw (k_icp_mask ran before).
// Two stable counting sorts of <= 64 bins each -- by column into the (still unused) match-coordinate buffer, then by row
// into srcw: least-significant-digit radix, so the final order is row-major by cell with the original order inside a cell.
__global__ __launch_bounds__(1024) void k_icp_init(IcpLarge P, int k_total) {
    __shared__ int base[ICP_GMAX], run[ICP_GMAX];
    __shared__ int wcnt[16][ICP_GMAX];
    const int k = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
    const int b = P.off[k], e = P.off[k + 1], ns = e - b;
    double* st = P.state + ICP_ST * k;
    const double x0a = st[36], inv_a = st[37], x0b = st[42], inv_b = st[43];
    const int axa = (int)st[38], axb = (int)st[44], gd = (int)st[45];
    double T[12];
    for (int q = 0; q < 12; ++q) T[q] = P.Min[16 * k + q];
    for (int pass = 0; pass < 2; ++pass) {
        // pass 0: local -> world, key = column (b axis), into prevt; pass 1: prevt -> srcw, key = row (a axis)
        const double* src = pass == 0 ? P.local : P.prevt;
        double* dst = pass == 0 ? P.prevt : P.srcw;
        auto point = [&](int i, double (&w)[3]) -> int {
            const double p0 = src[3 * (size_t)(b + i)], p1 = src[3 * (size_t)(b + i) + 1], p2 = src[3 * (size_t)(b + i) + 2];
            if (pass == 0) { for (int a = 0; a < 3; ++a) w[a] = fma(T[4 * a + 2], p2, fma(T[4 * a + 1], p1, T[4 * a] * p0)) + T[4 * a + 3]; }
            else { w[0] = p0; w[1] = p1; w[2] = p2; }
            const int ax = pass == 0 ? axb : axa;
            const double cc = ax == 0 ? w[0] : (ax == 1 ? w[1] : w[2]);
            return pass == 0 ? icp_bin(cc, x0b, inv_b, gd) : icp_bin(cc, x0a, inv_a, gd);
        };
        __syncthreads();                              // the previous pass has written its output
        if (tid < ICP_GMAX) { base[tid] = 0; run[tid] = 0; }
        __syncthreads();
        for (int i = tid; i < ns; i += 1024) {
            double w[3];
            atomicAdd(&base[point(i, w)], 1);
        }
        __syncthreads();
        if (wv == 0) {
            const int c = base[lane];
            int inc = c;
            for (int o = 1; o < 64; o <<= 1) { const int t = __shfl_up(inc, o, 64); if (lane >= o) inc += t; }
            base[lane] = inc - c;
        }
        for (int r0 = 0; r0 < ns; r0 += 1024) {
            __syncthreads();                          // base / run of the previous round are final; wcnt may be rewritten
            for (int q = tid; q < 16 * ICP_GMAX; q += 1024) (&wcnt[0][0])[q] = 0;
            __syncthreads();
            const int i = r0 + tid;
            const bool valid = i < ns;
            double w[3] = {0, 0, 0};
            int sl = 0;
            if (valid) sl = point(i, w);
            unsigned long long rem = __ballot(valid);
            int rank = 0;
            while (rem) {                             // rank among the wave's lower lanes of the same bin; the wave's count per bin
                const int lead = __ffsll((long long)rem) - 1;
                const int lsl = __builtin_amdgcn_readlane(sl, lead);
                const unsigned long long m = __ballot(valid && sl == lsl);
                if (valid && sl == lsl) rank = __popcll(m & ((1ull << lane) - 1ull));
                if (lane == lead) wcnt[wv][lsl] = __popcll(m);
                rem &= ~m;
            }
            __syncthreads();
            if (tid < ICP_GMAX) {                     // per bin: exclusive prefix over the waves, then the round's total
                int acc = 0;
                for (int w2 = 0; w2 < 16; ++w2) { const int t = wcnt[w2][tid]; wcnt[w2][tid] = acc; acc += t; }
                const int r = run[tid];
                run[tid] = r + acc;
                for (int w2 = 0; w2 < 16; ++w2) wcnt[w2][tid] += r;
            }
            __syncthreads();
            if (valid) {
                const size_t pos = (size_t)b + base[sl] + wcnt[wv][sl] + rank;
                dst[3 * pos] = w[0]; dst[3 * pos + 1] = w[1]; dst[3 * pos + 2] = w[2];
                if (pass == 1) P.nn[pos] = -1;
            }
        }
    }
    if (tid < 16) { st[tid] = P.Min[16 * k + tid]; st[16 + tid] = (tid % 5 == 0) ? 1.0 : 0.0; }      // pose; pending update = identity
    if (tid == 0) {
        st[32] = 0.0; st[33] = 0.0; st[34] = 0.0; st[35] = 0.0;       // prev fitness, prev rmse, done, updates applied
        P.arrive[k] = 0;
        // a cluster without points has no chunk to run its fit: what two fits would leave (identity update, then converged)
        if (ns == 0) { st[34] = 1.0; st[35] = 1.0; }
        if (k == 0) {
            int live_clusters = 0;
            for (int j = 0; j < k_total; ++j) live_clusters += P.off[j + 1] > P.off[j];
            *P.running = live_clusters;
            int c = 0;                                                // chunks of ICP_CH sources, never across clusters
            for (int j = 0; j < k_total; ++j) { P.chunk0[j] = c; c += (P.off[j + 1] - P.off[j] + ICP_CH - 1) / ICP_CH; }
            P.chunk0[k_total] = c;
            int pb = 0;                                               // pool offsets of the clusters' cell-sorted target coordinates
            for (int j = 0; j < k_total; ++j) {
                const int ntj = P.tcount[j];
                if (pb + ntj <= P.pool_cap) { P.tbase[j] = pb; pb += ntj; } else P.tbase[j] = -1;
                P.tlmax[j] = 0u;
            }
        }
    }
    // the cluster of each of this cluster's chunks (the same count, recomputed here: no wait for thread 0 of cluster 0)
    {
        int c0 = 0;
        for (int j = tid; j < k; j += 1024) c0 += (P.off[j + 1] - P.off[j] + ICP_CH - 1) / ICP_CH;
        __shared__ int s_part[16];
        c0 = wave_sum(c0);
        __syncthreads();
        if (lane == 0) s_part[wv] = c0;
        __syncthreads();
        int first = 0;
        for (int w2 = 0; w2 < 16; ++w2) first += s_part[w2];
        const int mine = (ns + ICP_CH - 1) / ICP_CH;
        for (int q = tid; q < mine; q += 1024) P.chunk_cl[first + q] = k;
    }
}

// grid (cluster, slices): the cluster's masked targets, in cell order, into the coordinate pool (one gather per frame
// instead of one per search: k_icp_nn stages them with coalesced loads)
__global__ __launch_bounds__(256) void k_icp_pool(IcpLarge P, int nf) {
    const int c = blockIdx.x, tb = P.tbase[c];
    if (tb < 0) return;
    const int nt = P.tcount[c];
    const int* tidx = P.tidx + (size_t)c * nf;
    const float* bx6 = P.box + 6 * c;
    const double oc0 = 0.5 * ((double)bx6[0] + (double)bx6[3]), oc1 = 0.5 * ((double)bx6[1] + (double)bx6[4]), oc2 = 0.5 * ((double)bx6[2] + (double)bx6[5]);
    float lm = 0.f;
    for (int t = blockIdx.y * 256 + threadIdx.x; t < nt; t += gridDim.y * 256) {
        const int j = tidx[t];
        const double x = P.frame[3 * (size_t)j], y = P.frame[3 * (size_t)j + 1], z = P.frame[3 * (size_t)j + 2];
        P.tcx[tb + t] = x; P.tcy[tb + t] = y; P.tcz[tb + t] = z;
        const float fx = (float)(x - oc0), fy = (float)(y - oc1), fz = (float)(z - oc2);
        P.tcf[tb + t] = make_float4(fx, fy, fz, __int_as_float(j));
        lm = fmaxf(lm, fmaxf(fabsf(fx), fmaxf(fabsf(fy), fabsf(fz))));
    }
    lm = -wave_min_fast(-lm);
    if ((threadIdx.x & 63) == 0 && lm > 0.f) atomicMax(P.tlmax + c, __float_as_uint(lm));      // (non-negative floats order like their bits)
}

// Before the first iteration of a frame no source has a previous match, and a search without one scans its cluster's whole grid
// (one launch of 350-1100 us at configs[4]).  This gives every source SOME target to start from: the nearest one of its own grid
// cell, or of the nearest ring of cells (up to 3) that holds any.  Any target of the list is a valid start -- k_icp_nn's result is the
// lexicographic minimum over a square that contains the nearest target, whatever it starts from -- and a near one makes that square small.
__global__ __launch_bounds__(256) void k_icp_seed(IcpLarge P, int nf) {
    const int c = blockIdx.x;
    const double* st = P.state + ICP_ST * c;
    const double x0a = st[36], inv_a = st[37], x0b = st[42], inv_b = st[43];
    const int axa = (int)st[38], axb = (int)st[44], gd = (int)st[45];
    const int* tst = P.tst + (size_t)c * (ICP_NCELL + 1);
    const int* tidx = P.tidx + (size_t)c * nf;
    const int tb = P.tbase[c];
    for (int i = P.off[c] + blockIdx.y * 256 + threadIdx.x; i < P.off[c + 1]; i += gridDim.y * 256) {
        const double s[3] = {P.srcw[3 * (size_t)i], P.srcw[3 * (size_t)i + 1], P.srcw[3 * (size_t)i + 2]};
        const int ia = icp_bin(s[axa], x0a, inv_a, gd), ib = icp_bin(s[axb], x0b, inv_b, gd);
        // (round 4: the NEAREST target of the first ring that holds any, not the first one listed -- a cell is a column along the
        //  box's shortest edge, and its first entry can be the cluster's whole thickness away: the first search of a frame scanned
        //  1.1 ms worth of cells around such seeds)
        int t = -1;
        double td = INFINITY;
        for (int e = 0; e <= 3 && t < 0; ++e)
            for (int r = max(ia - e, 0); r <= min(ia + e, gd - 1); ++r) {
                const int q0 = tst[r * gd + max(ib - e, 0)], q1 = tst[r * gd + min(ib + e, gd - 1) + 1];
                for (int q = q0; q < q1; ++q) {
                    double x, y, z;
                    if (tb >= 0) { x = P.tcx[tb + q]; y = P.tcy[tb + q]; z = P.tcz[tb + q]; }
                    else { const size_t j = (size_t)tidx[q]; x = P.frame[3 * j]; y = P.frame[3 * j + 1]; z = P.frame[3 * j + 2]; }
                    const double dx = s[0] - x, dy = s[1] - y, dz = s[2] - z;
                    const double d = (dx * dx + dy * dy) + dz * dz;
                    if (d < td) { td = d; t = q; }
                }
            }
        if (t >= 0) {
            const int j = tidx[t];
            P.nn[i] = j;
            if (tb >= 0) { P.prevt[3 * (size_t)i] = P.tcx[tb + t]; P.prevt[3 * (size_t)i + 1] = P.tcy[tb + t]; P.prevt[3 * (size_t)i + 2] = P.tcz[tb + t]; }
            else { P.prevt[3 * (size_t)i] = P.frame[3 * (size_t)j]; P.prevt[3 * (size_t)i + 1] = P.frame[3 * (size_t)j + 1]; P.prevt[3 * (size_t)i + 2] = P.frame[3 * (size_t)j + 2]; }
        }
    }
}

// One workgroup: the chunks of the clusters that have not converged, in order, into P.live; their number behind the
// "clusters still running" word the host reads between batches (the next batch of searches launches only those chunks:
// in the tail of a frame a few clusters iterate on, and the thousands of workgroups that would only find "done" and leave
// delayed the live ones by 10-40 us per search).
__global__ __launch_bounds__(1024) void k_icp_compact(IcpLarge P, int k_total) {
    __shared__ int wsum[16];
    __shared__ int s_run;
    const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
    if (tid == 0) s_run = 0;
    __syncthreads();
    for (int c0 = 0; c0 < k_total; c0 += 1024) {
        const int c = c0 + tid;
        const bool lv = c < k_total && P.state[ICP_ST * c + 34] == 0.0;
        const int nch = lv ? P.chunk0[c + 1] - P.chunk0[c] : 0;
        int inc = nch;
        for (int o = 1; o < 64; o <<= 1) { const int t = __shfl_up(inc, o, 64); if (lane >= o) inc += t; }
        if (lane == 63) wsum[wv] = inc;
        __syncthreads();
        int base = s_run + inc - nch, total = 0;
        for (int w = 0; w < 16; ++w) { const int t = wsum[w]; base += w < wv ? t : 0; total += t; }
        for (int q = 0; q < nch; ++q) P.live[base + q] = P.chunk0[c] + q;
        __syncthreads();
        if (tid == 0) s_run += total;
        __syncthreads();
    }
    if (tid == 0) P.running[1] = s_run;
}

__device__ __forceinline__ double ld_agent_f64(const double* p) {
    return __longlong_as_double((long long)__hip_atomic_load((const unsigned long long*)p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT));
}
__device__ __forceinline__ void st_agent_f64(double* p, double v) {
    __hip_atomic_store((unsigned long long*)p, (unsigned long long)__double_as_longlong(v), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

// One wave, run by the LAST chunk of cluster k to finish its search (k_icp_nn): moments of the chunks in chunk order ->
// fitness / RMSE, open3d's convergence test against the previous ones, else Horn's closed form: new pose, pending update.
// The other chunks' moments were stored with agent-scope stores and are read with agent-scope loads (no fences:
// MI355X_MICROARCH.md, "sc1 stores and loads both sides"); everything else the wave reads was written by earlier launches.
__device__ void icp_fit_cluster(const IcpLarge& P, int k, int max_iter, int lane) {
    double* st = P.state + ICP_ST * k;
    const int ns = P.off[k + 1] - P.off[k];
    double v = 0.0;
    if (lane < ICP_NM) {
        const int c0 = P.chunk0[k], c1 = P.chunk0[k + 1];
        for (int ch = c0; ch < c1; ch += 8) {                         // chunk order; a group's loads are issued together
            double pv[8];
#pragma unroll
            for (int u = 0; u < 8; ++u) pv[u] = ld_agent_f64(P.part + (size_t)min(ch + u, c1 - 1) * ICP_NM + lane);
#pragma unroll
            for (int u = 0; u < 8; ++u) if (ch + u < c1) v += pv[u];
        }
    }
    double cm[ICP_NM];
#pragma unroll
    for (int a = 0; a < ICP_NM; ++a) cm[a] = __hiloint2double(__builtin_amdgcn_readlane(__double2hiint(v), a), __builtin_amdgcn_readlane(__double2loint(v), a));
    if (lane != 0) return;
    // fitness / inlier RMSE of the correspondences the last k_icp_nn produced (registration_icp's GetRegistrationResult)
    const double ncorr = cm[0];
    const double fit = ns > 0 ? cm[0] / (double)ns : 0.0, rmse = cm[0] > 0 ? sqrt(cm[1] / cm[0]) : 0.0;
    const double pf = st[32], pr = st[33];
    const int updates = (int)st[35];
    const bool converged = updates >= 1 && fabs(pf - fit) < 1e-6 && fabs(pr - rmse) < 1e-6;
    if (converged || updates >= max_iter) { st[34] = 1.0; atomicSub(P.running, 1); return; }
    double U[16], T[16], Vp[16];
    for (int i = 0; i < 16; ++i) { U[i] = (i % 5 == 0) ? 1.0 : 0.0; Vp[i] = U[i]; T[i] = st[i]; }
    if (ncorr > 0) {
        const double shc[3] = {st[39], st[40], st[41]};
        double ms[3], md[3], msr[3], mdr[3];
        for (int a = 0; a < 3; ++a) { msr[a] = cm[2 + a] / ncorr; mdr[a] = cm[5 + a] / ncorr; ms[a] = shc[a] + msr[a]; md[a] = shc[a] + mdr[a]; }
        double C[9];
        for (int a = 0; a < 3; ++a) for (int c = 0; c < 3; ++c) C[3 * a + c] = fma(-ncorr * msr[a], mdr[c], cm[8 + 3 * a + c]);
        const double Sxx = C[0], Sxy = C[1], Sxz = C[2], Syx = C[3], Syy = C[4], Syz = C[5], Szx = C[6], Szy = C[7], Szz = C[8];
        double N[4][4] = {{Sxx + Syy + Szz, Syz - Szy, Szx - Sxz, Sxy - Syx},
                          {Syz - Szy, Sxx - Syy - Szz, Sxy + Syx, Szx + Sxz},
                          {Szx - Sxz, Sxy + Syx, -Sxx + Syy - Szz, Syz + Szy},
                          {Sxy - Syx, Szx + Sxz, Syz + Szy, -Sxx - Syy + Szz}};
        double q[4], R[9];
        horn_max_eigvec(N, q, Vp);
        quat_to_matrix(q, R);
        for (int a = 0; a < 3; ++a) {
            U[4 * a] = R[3 * a]; U[4 * a + 1] = R[3 * a + 1]; U[4 * a + 2] = R[3 * a + 2];
            U[4 * a + 3] = md[a] - (R[3 * a] * ms[0] + R[3 * a + 1] * ms[1] + R[3 * a + 2] * ms[2]);
        }
        st[39] = md[0]; st[40] = md[1]; st[41] = md[2];              // the matched sources' centroid lands here
    }
    for (int r = 0; r < 4; ++r) for (int c = 0; c < 4; ++c) {
        double s = 0;
        for (int m = 0; m < 4; ++m) s = fma(U[4 * r + m], T[4 * m + c], s);
        st[4 * r + c] = s;
    }
    for (int i = 0; i < 16; ++i) st[16 + i] = U[i];                   // k_icp_nn applies it to the sources
    st[32] = fit; st[33] = rmse; st[35] = (double)(updates + 1);
}

// Block = one chunk of ICP_CH = 64 sorted sources of ONE cluster (chunk0 maps blocks to clusters; blocks past the last
// chunk exit), 256 threads: the tail of a frame's ICP is a few clusters iterating on, and small chunks put their work on
// many CUs (1024-thread chunks of 256 sources: 59 us per search whatever the number of live clusters).  A wave owns 16 consecutive sorted sources -- about two cells' worth -- and four lanes share one
// source: lane group g scans grid row ra0 + g of the cell rectangle [ra0, ra1] x [cb0, cb1] that the wave's sources'
// (x - r, x + r) squares touch, r = distance to the previous match.  A row of the rectangle is one contiguous run of the
// cell-sorted target list; the runs are staged 16 targets per row at a time in the wave's own LDS slice (no block barrier
// in the scan), entries past a run's end as far-away points.
// debug build only (tests/measure/icp_tail_blocks.py): per workgroup of the launches with at most 4 clusters iterating -- [0] start
// [1] end of the search (10 ns wall ticks) [2] entries per lane group scanned by wave 0 [3] rows << 16 | columns of wave 0's
// rectangle [4] cluster [5] launch grid
ICP_BLK(__device__ unsigned long long g_icp_blk[6][8192];)
#ifdef CREG_STAMPS
// debug build only (tests/measure/icp_large_stamps.py): the tail launches' wall times, folded after every launch
__device__ unsigned long long g_icp_wall[8];      // tail launches: sums of [0] first live block start - launch start [1] last search end - launch start [2] fit end - launch start (100 MHz ticks) [3] launches
__device__ unsigned long long g_icp_wmin[4];      // scratch of the running launch: launch start, first live start, last search end, fit end
__global__ void k_icp_wall_fold() {
    if (g_icp_wmin[0] != ~0ull && g_icp_wmin[3] != 0ull) {
        g_icp_wall[0] += g_icp_wmin[1] - g_icp_wmin[0]; g_icp_wall[1] += g_icp_wmin[2] - g_icp_wmin[0]; g_icp_wall[2] += g_icp_wmin[3] - g_icp_wmin[0]; g_icp_wall[3] += 1;
    }
    g_icp_wmin[0] = ~0ull; g_icp_wmin[1] = ~0ull; g_icp_wmin[2] = 0ull; g_icp_wmin[3] = 0ull;
}
#endif
#ifndef ICP_NN_WPS
#define ICP_NN_WPS 3                       // minimum waves per SIMD the register allocation of k_icp_nn is held to
#endif
// Always-on work counters of the search (round 6: the roofline of the configs[4] frame names THIS kernel): [0] waves that searched,
// [1] float32 screen trips (a trip = 8 staged targets x the wave's 64 lanes = 512 pair evaluations), [2] trips that went on to the fp64
// evaluation, [3] live sources (source-iterations), [4] tie rescans.  Wave-uniform tallies in SGPRs, one atomic per counter and wave.
// 256 shards (blockIdx & 255): ~2 800 waves of a launch adding to ONE word serialise in the L2 -- 88 atomics per microsecond and word, which
// doubled the launch (50 -> 116 us, measured) when the tallies were first added unsharded.
constexpr int ICP_CT_SHARDS = 256;
__device__ unsigned long long g_icp_nn_ct[ICP_CT_SHARDS][8];
__global__ __launch_bounds__(64 * ICP_NNW, ICP_NN_WPS) void k_icp_nn(IcpLarge P, int n, int k_total, int nf, double th2, int max_iter) {
    constexpr int SB = ICP_SB, SR = ICP_SB + 2;                       // staged targets per lane group and batch; slice stride
                                                                      // (+2: the four groups' equal slots fall into different LDS banks)
    extern __shared__ __attribute__((aligned(16))) char smem[];
    double* tx = (double*)smem;                                       // [waves][4 rows][SR] x | y | z, then the frame indices
    double* ty = tx + ICP_NNW * ICP_G * SR; double* tz = ty + ICP_NNW * ICP_G * SR;
    int* tj = (int*)(tz + ICP_NNW * ICP_G * SR);
    float* txf = (float*)(tj + ICP_NNW * ICP_G * SR);                  // the same targets relative to the wave's origin, float32 (the screen)
    float* tyf = txf + ICP_NNW * ICP_G * SR; float* tzf = tyf + ICP_NNW * ICP_G * SR;
    __shared__ double sc[ICP_NNW * ICP_NM];
    const int tid = threadIdx.x, lane = tid & 63;
    // (the host sizes the grid from the live-chunk count it knew one batch of launches ago -- an upper bound, the list only shrinks --
    //  so workgroups past the CURRENT count leave: what lies behind it in `live` are leftovers of longer lists, possibly duplicates)
    if (P.use_live && (int)blockIdx.x >= P.running[1]) return;
    const int blk = P.use_live ? P.live[blockIdx.x] : (int)blockIdx.x;     // the chunk this workgroup takes
    const int wv = __builtin_amdgcn_readfirstlane(tid >> 6);
    ICP_STAMPED(const bool tailonly = *P.running <= 4;                // stamps of the tail of the frame only: few clusters still iterating
                if (tid == 0 && tailonly) atomicMin(&g_icp_wmin[0], wall_clock64());
                unsigned long long nst = clock64();)
    ICP_BLK(const bool blk_rec = *P.running <= 4 && blockIdx.x < 8192;
            unsigned long long blk_per = 0;
            const unsigned long long blk_t0 = wall_clock64();)
    if (blk >= P.chunk0[k_total]) return;
    const int c = P.chunk_cl[blk];
    const double* st = P.state + ICP_ST * c;
    if (st[34] != 0.0) return;                                        // converged cluster: nothing moves any more
    const int g = lane / ICP_SPW, l16 = lane % ICP_SPW;               // lane group (the grid rows of the rectangle it scans), source in the wave
    ICP_STAMPED(if (tid == 0 && tailonly) atomicMin(&g_icp_wmin[1], wall_clock64());)
    const int i = P.off[c] + (blk - P.chunk0[c]) * ICP_CH + wv * ICP_SPW + l16;
    const bool live = i < P.off[c + 1];
    const double x0a = st[36], inv_a = st[37], x0b = st[42], inv_b = st[43];
    const int axa = (int)st[38], axb = (int)st[44], gd = (int)st[45];
    const double shc0 = st[39], shc1 = st[40], shc2 = st[41];
    double s0 = 0, s1 = 0, s2 = 0, alo = INFINITY, ahi = -INFINITY, blo = INFINITY, bhi = -INFINITY;
    double seed = 1e299;                                              // 1e299: below the staged padding's 3e300, above any real squared distance
    double pd2 = 0, pq0 = 0, pq1 = 0, pq2 = 0; int pmv = -2;          // the previous match: its squared distance now, its coordinates, its frame index
    if (live) {
        // the rigid update the last fit left pending (identity before the first one); the four lanes of a source agree,
        // lane group 0 stores
        const double p0 = P.srcw[3 * (size_t)i], p1 = P.srcw[3 * (size_t)i + 1], p2 = P.srcw[3 * (size_t)i + 2];
        const int pm = P.nn[i];                                       // -1 before the first search (k_icp_init)
        const double q0 = P.prevt[3 * (size_t)i], q1 = P.prevt[3 * (size_t)i + 1], q2 = P.prevt[3 * (size_t)i + 2];
        s0 = fma(st[16 + 2], p2, fma(st[16 + 1], p1, st[16] * p0)) + st[16 + 3];
        s1 = fma(st[16 + 6], p2, fma(st[16 + 5], p1, st[16 + 4] * p0)) + st[16 + 7];
        s2 = fma(st[16 + 10], p2, fma(st[16 + 9], p1, st[16 + 8] * p0)) + st[16 + 11];
        alo = -INFINITY; ahi = INFINITY; blo = -INFINITY; bhi = INFINITY;
        if (pm >= 0) {
            const double dx = s0 - q0, dy = s1 - q1, dz = s2 - q2;
            const double sa = axa == 0 ? s0 : (axa == 1 ? s1 : s2), sb = axb == 0 ? s0 : (axb == 1 ? s1 : s2);
            const double d2p = (dx * dx + dy * dy) + dz * dz;
            const double r0 = (d2p > 1e-280 ? d2p * fast_rsqrt(d2p) : 1e-140) * (1.0 + 1e-12) + 1e-300;
            const double ra = r0 + 4e-16 * fabs(sa), rb = r0 + 4e-16 * fabs(sb);
            alo = sa - ra; ahi = sa + ra; blo = sb - rb; bhi = sb + rb;
            // the previous match lies inside the rectangle and will be scanned with exactly this value (same operands, same
            // association): starting `best` a hair above it changes no result -- the match itself still passes the strict `<` --
            // and lets the float32 screen below reject almost every other target from the first trip on
            if (P.screen) seed = d2p * (1.0 + 0x1p-40) + 1e-300;
            pd2 = d2p; pq0 = q0; pq1 = q1; pq2 = q2; pmv = pm;
        }
    }
    NN_STAMP(8);
    if (live && g == 0) { P.srcw[3 * (size_t)i] = s0; P.srcw[3 * (size_t)i + 1] = s1; P.srcw[3 * (size_t)i + 2] = s2; }
    const bool any = __ballot(live) != 0;
    const int ra0 = __builtin_amdgcn_readfirstlane(icp_bin(wave_min_fast(alo), x0a, inv_a, gd));
    const int ra1 = __builtin_amdgcn_readfirstlane(icp_bin(wave_max_fast(ahi), x0a, inv_a, gd));
    const int cb0 = __builtin_amdgcn_readfirstlane(icp_bin(wave_min_fast(blo), x0b, inv_b, gd));
    const int cb1 = __builtin_amdgcn_readfirstlane(icp_bin(wave_max_fast(bhi), x0b, inv_b, gd));
    const int* tst = P.tst + (size_t)c * (ICP_NCELL + 1);
    const int* tidx = P.tidx + (size_t)c * nf;
    const int nrows_all = any ? ra1 - ra0 + 1 : 0;
    ICP_STAMPED(const int nrows = nrows_all;
                if (lane == 0 && any && tailonly) { atomicAdd(&g_icp_stamps[1], 1ull); atomicAdd(&g_icp_stamps[3], (unsigned long long)P.tcount[c]); atomicAdd(&g_icp_stamps[5], (unsigned long long)nrows); atomicAdd(&g_icp_stamps[6], (unsigned long long)(cb1 - cb0 + 1)); }
                const unsigned long long stt = clock64();)
    double* px = tx + (wv * ICP_G + g) * SR; double* py = ty + (wv * ICP_G + g) * SR; double* pz = tz + (wv * ICP_G + g) * SR;
    int* pj = tj + (wv * ICP_G + g) * SR;
    float* pxf = txf + (wv * ICP_G + g) * SR; float* pyf = tyf + (wv * ICP_G + g) * SR; float* pzf = tzf + (wv * ICP_G + g) * SR;
    // ---- float32 screen ----------------------------------------------------------------------------------------------
    // Coordinates relative to a wave origin o (the first live source), rounded to float32; d_f = the float32 squared distance.
    // With u = 2^-24, L >= every |coordinate - o| (the mask box holds the targets, the sources are measured) and D the
    // fp64 squared distance:  d_f <= D + 8 u (L sqrt(D) + D) + 13 u^2 L^2   (input rounding 2 u L per difference, three
    // roundings of the sum).  So D <= best implies d_f <= thr = best + 2^-20 (L sqrt(best) + best) + 2^-43 L^2 (twice the
    // bound), and a trip whose smallest d_f exceeds thr (rounded up to float32) in EVERY lane cannot change `best`, the slot
    // or the tie flag: it is skipped; every other trip runs the fp64 code below unchanged.  The screen only ever skips work.
    const int flive = __builtin_ctzll(__ballot(live) | (1ull << 63));
    const double o0 = __shfl(s0, flive, 64), o1 = __shfl(s1, flive, 64), o2 = __shfl(s2, flive, 64);
    const float sf0 = (float)(s0 - o0), sf1 = (float)(s1 - o1), sf2 = (float)(s2 - o2);
    double Lb = 0.0;
    {
        const float* bx6 = P.box + 6 * c;
        const double od[3] = {o0, o1, o2};
        for (int d = 0; d < 3; ++d) Lb = fmax(Lb, fmax(fabs((double)bx6[d] - od[d]), fabs((double)bx6[3 + d] - od[d])));
        const double ls = live ? fmax(fabs(s0 - o0), fmax(fabs(s1 - o1), fabs(s2 - o2))) : 0.0;
        Lb = fmax(Lb, wave_max_fast(ls)) * (1.0 + 0x1p-20) + 1e-30;   // (box corners are float32: slack for their rounding)
    }
    auto screen_thr = [&](double b) -> float {
        if (!(b < 1e290)) return INFINITY;
        const double rt = (double)sqrtf((float)b) * (1.0 + 0x1p-20);
        return (float)((b + 0x1p-20 * (Lb * rt + b) + 0x1p-43 * Lb * Lb) * (1.0 + 0x1p-22));
    };
    const int tb = P.tbase[c];                                        // >= 0: coordinates in the pool, in the order of tidx
    // Lane group g walks the runs of grid rows rb + g, + 4, + 8, + 12 of a band of <= 16 rows as ONE sequence of L entries
    // (entry p -> run and offset by three compares), so the scan is a flat loop over batches of SB entries and the four groups
    // carry nearly equal loads whatever the number of rows.  A rectangle of more than 16 rows (the first search of a large
    // cluster: the whole grid) takes several bands.
    int rs0 = 0, rs1 = 0, rs2 = 0, rs3 = 0, c1 = 0, c2 = 0, c3 = 0, L = 0, per = 0;
    auto band = [&](int rb) {
        const int nrows = min(16, ra1 - rb + 1);
        int q0v = 0, q1v = 0;                         // lane l < rows: the run of grid row rb + l
        if (lane < nrows) { q0v = tst[(rb + lane) * gd + cb0]; q1v = tst[(rb + lane) * gd + cb1 + 1]; }
        const int r0 = g, r1 = g + ICP_G, r2 = g + 2 * ICP_G, r3 = g + 3 * ICP_G;   // this group's rows of the band (those < 16)
        const int a0 = __shfl(q0v, r0 & 63, 64), e0 = __shfl(q1v, r0 & 63, 64), a1 = __shfl(q0v, r1 & 63, 64), e1 = __shfl(q1v, r1 & 63, 64);
        const int a2 = __shfl(q0v, r2 & 63, 64), e2 = __shfl(q1v, r2 & 63, 64), a3 = __shfl(q0v, r3 & 63, 64), e3 = __shfl(q1v, r3 & 63, 64);
        rs0 = a0; rs1 = a1; rs2 = a2; rs3 = a3;
        c1 = r0 < nrows ? e0 - a0 : 0;
        c2 = c1 + (r1 < nrows ? e1 - a1 : 0);
        c3 = c2 + (r2 < nrows ? e2 - a2 : 0);
        L = c3 + (r3 < nrows ? e3 - a3 : 0);
        int pr = L;
        for (int o = ICP_SPW; o < 64; o <<= 1) pr = max(pr, __shfl_xor(pr, o, 64));
        per = __builtin_amdgcn_readfirstlane(pr);                     // the longest of the four sequences
        ICP_BLK(blk_per += per;)
        ICP_STAMPED(if (lane == 0 && tailonly) { atomicAdd(&g_icp_stamps[0], (unsigned long long)per); atomicAdd(&g_icp_stamps[4], 1ull); })
    };
    constexpr int EPL = SB / ICP_SPW;                                 // staged entries per lane and batch
    int ct_f32 = 0, ct_f64 = 0, ct_tie = 0;                           // (wave-uniform: the trips' branches are ballots)
    double best = seed; int bslot = -1, bj = 0x7fffffff;
    double bx = 0, by = 0, bz = 0;                                    // the best target's coordinates
    bool tief = false;
    NN_STAMP(9);
    if (P.screen && tb >= 0) {
        // ---- pool path: only what the screen needs is staged ---------------------------------------------------------------
        // The pool holds every masked target of the cluster as (float32 coordinates relative to the box centre oc, frame index):
        // one 16-byte load per entry, 16 bytes of LDS, and TWO batches of loads in flight (16 VGPRs a batch instead of 28).
        // The fp64 coordinates stay in the pool: the rare trip that passes the screen reads its eight entries from there (L2).
        // Same bound as above with o = oc and L from the cluster's own extent (k_icp_pool) and the wave's sources.
        const float* bxc = P.box + 6 * c;
        const double oc0 = 0.5 * ((double)bxc[0] + (double)bxc[3]), oc1 = 0.5 * ((double)bxc[1] + (double)bxc[4]), oc2 = 0.5 * ((double)bxc[2] + (double)bxc[5]);
        const float cf0 = (float)(s0 - oc0), cf1 = (float)(s1 - oc1), cf2 = (float)(s2 - oc2);
        const double lsrc = live ? fmax(fabs(s0 - oc0), fmax(fabs(s1 - oc1), fabs(s2 - oc2))) : 0.0;
        const double Lc = fmax((double)__uint_as_float(P.tlmax[c]), wave_max_fast(lsrc)) * (1.0 + 0x1p-20) + 1e-30;
        auto thr_of = [&](double b) -> float {
            if (!(b < 1e290)) return INFINITY;
            const double rt = (double)sqrtf((float)b) * (1.0 + 0x1p-20);
            return (float)((b + 0x1p-20 * (Lc * rt + b) + 0x1p-43 * Lc * Lc) * (1.0 + 0x1p-22));
        };
        // The previous match is a target of this very list, and its squared distance from the moved source is pd2 exactly as the scan
        // would compute it: the search STARTS from it (best = pd2, its index and coordinates) and leaves that one entry out (the
        // screen would let it through in every scan: a trip's fp64 operands come from L2, ~1.5 us).  Any other target at exactly
        // pd2 passes the screen and raises the tie flag as before; the rescan of pass 1 starts from nothing.
        if (pmv >= 0) { best = pd2; bj = pmv; bx = pq0; by = pq1; bz = pq2; bslot = 0; }
        float thr = thr_of(best);
        const float4* tcf = P.tcf + tb;
        const double* gx = P.tcx + tb; const double* gy = P.tcy + tb; const double* gz = P.tcz + tb;
        auto seqpos = [&](int pq) { return pq < c1 ? rs0 + pq : (pq < c2 ? rs1 + (pq - c1) : (pq < c3 ? rs2 + (pq - c2) : rs3 + (pq - c3))); };
        float4 v2[2][EPL];
        auto fetchp = [&](auto SET, int t0) {
#pragma unroll
            for (int u = 0; u < EPL; ++u) {
                const int pq = t0 + ICP_SPW * u + l16;
                const bool in = pq < L;
                const float4 v = tcf[in ? seqpos(pq) : 0];
                v2[decltype(SET)::value][u] = in ? v : make_float4(1e30f, 1e30f, 1e30f, __int_as_float(0x7fffffff));
            }
        };
        auto publishp = [&](auto SET) {
#pragma unroll
            for (int u = 0; u < EPL; ++u) {
                const int e = ICP_SPW * u + l16;
                const float4 v = v2[decltype(SET)::value][u];
                pxf[e] = v.x; pyf[e] = v.y; pzf[e] = v.z; pj[e] = __float_as_int(v.w);
            }
        };
        for (int pass = 0; pass < 2; ++pass) {                        // pass 1 only after a tie was seen: frame-index tie-break
          for (int rb = ra0; rb < ra0 + nrows_all; rb += 16) {
            band(rb);
            using S0 = std::integral_constant<int, 0>; using S1 = std::integral_constant<int, 1>;
            if (per > 0) fetchp(S0{}, 0);
            if (per > SB) fetchp(S1{}, SB);
            auto scan_batch = [&](int t0) {
                const int cnt = min(SB, per - t0);
                int bm = -1;
                if (pass == 0) {
                    for (int t = 0; t < cnt; t += 8) {
                        float mf = INFINITY, ef[8];
#pragma unroll
                        for (int u = 0; u < 8; u += 2) {
                            const nn_f2 X = *(const nn_f2*)(pxf + t + u), Y = *(const nn_f2*)(pyf + t + u), Z = *(const nn_f2*)(pzf + t + u);
                            const nn_f2 fx = nn_f2{cf0, cf0} - X, fy = nn_f2{cf1, cf1} - Y, fz = nn_f2{cf2, cf2} - Z;
                            const nn_f2 e = __builtin_elementwise_fma(fz, fz, __builtin_elementwise_fma(fy, fy, fx * fx));
                            ef[u] = e.x; ef[u + 1] = e.y;
                            mf = fminf(mf, fminf(e.x, e.y));
                        }
                        ++ct_f32;
                        if (!__ballot(mf <= thr)) continue;
                        // Round 6: only the entries that PASSED the screen are evaluated in fp64 -- a lane's candidates of a trip (usually one), two
                        // at a time, their pool coordinates requested together and kept: ONE dependent L2 round trip per passing trip where there were
                        // three (operands of entries 0-3, of 4-7, then the winner's coordinates again).  An entry the screen rejects has D > best, so it
                        // can neither win nor tie: the minimum, the tie flag and the slot are what the eight-entry evaluation gave.
                        unsigned cm = 0;                                  // bit u: entry u passed this lane's screen and is not its previous match
#pragma unroll
                        for (int u = 0; u < 8; ++u) cm |= (ef[u] <= thr && pj[t + u] != pmv) ? 1u << u : 0u;
                        if (!__ballot(cm != 0)) continue;                 // only previous matches came through
                        ++ct_f64;
                        bool any_lt = false;
                        while (__ballot(cm != 0)) {                        // four candidates per round: one round unless a lane has more
                            int uu[4]; double X[4], Y[4], Z[4], dd[4];
#pragma unroll
                            for (int c4 = 0; c4 < 4; ++c4) {
                                uu[c4] = cm ? __builtin_ctz(cm) : -1; cm &= cm - 1;
                                const int pq = t0 + t + max(uu[c4], 0);
                                const bool in = uu[c4] >= 0 && pq < L;
                                const int tp = in ? seqpos(pq) : 0;
                                X[c4] = gx[tp]; Y[c4] = gy[tp]; Z[c4] = gz[tp];
                                if (!in) uu[c4] = -1;
                            }
#pragma unroll
                            for (int c4 = 0; c4 < 4; ++c4) {
                                const double dx = s0 - X[c4], dy = s1 - Y[c4], dz = s2 - Z[c4];
                                dd[c4] = uu[c4] >= 0 ? (dx * dx + dy * dy) + dz * dz : 1e300;
                            }
                            // the earliest of the smallest, by selects (an index into the register arrays would send them to scratch)
                            const bool s01 = dd[1] < dd[0], s23 = dd[3] < dd[2];
                            const double m01 = s01 ? dd[1] : dd[0], m23 = s23 ? dd[3] : dd[2];
                            const int u01 = s01 ? uu[1] : uu[0], u23 = s23 ? uu[3] : uu[2];
                            const double x01 = s01 ? X[1] : X[0], y01 = s01 ? Y[1] : Y[0], z01 = s01 ? Z[1] : Z[0];
                            const double x23 = s23 ? X[3] : X[2], y23 = s23 ? Y[3] : Y[2], z23 = s23 ? Z[3] : Z[2];
                            const bool sh = m23 < m01;
                            const double m = sh ? m23 : m01;
                            const int eq = (dd[0] == m) + (dd[1] == m) + (dd[2] == m) + (dd[3] == m);
                            const bool lt = m < best;
                            tief |= m == best || (lt && eq > 1);
                            bm = lt ? t + (sh ? u23 : u01) : bm;
                            bx = lt ? (sh ? x23 : x01) : bx; by = lt ? (sh ? y23 : y01) : by; bz = lt ? (sh ? z23 : z01) : bz;
                            best = lt ? m : best;
                            any_lt |= lt;
                        }
                        if (__ballot(any_lt)) thr = thr_of(best);
                    }
                    if (bm >= 0) { bj = pj[bm]; bslot = bm; }
                } else {
                    for (int t = 0; t < cnt; ++t) {
                        const int pq = t0 + t;
                        const bool in = pq < L;
                        const int tp = in ? seqpos(pq) : 0;
                        const double x = in ? gx[tp] : 1e150, y = in ? gy[tp] : 1e150, z = in ? gz[tp] : 1e150;
                        const double dx = s0 - x, dy = s1 - y, dz = s2 - z;
                        const double d2 = (dx * dx + dy * dy) + dz * dz;
                        const int j = pj[t];
                        if (d2 < best || (d2 == best && j < bj)) { best = d2; bj = j; bx = x; by = y; bz = z; bslot = t; }
                    }
                }
                __builtin_amdgcn_wave_barrier();
            };
            for (int t0 = 0; t0 < per; t0 += 2 * SB) {
                publishp(S0{});
                __builtin_amdgcn_wave_barrier();
                if (t0 + 2 * SB < per) fetchp(S0{}, t0 + 2 * SB);
                scan_batch(t0);
                if (t0 + SB < per) {
                    publishp(S1{});
                    __builtin_amdgcn_wave_barrier();
                    if (t0 + 3 * SB < per) fetchp(S1{}, t0 + 3 * SB);
                    scan_batch(t0 + SB);
                }
            }
          }
          if (pass == 0) {
              if (!__ballot(tief)) break;
              ++ct_tie;
              best = 1e299; bslot = -1; bj = 0x7fffffff;
          }
        }
    } else {
    float thr_f = screen_thr(best);
    // staging registers of one batch: the loads of batch b + 1 are in flight while batch b is scanned from LDS
    int jv[EPL];
    double cx[EPL], cy[EPL], cz[EPL];
    auto fetch = [&](int t0) {
#pragma unroll
        for (int u = 0; u < EPL; ++u) {
            const int pq = t0 + ICP_SPW * u + l16;                         // entry of the group's sequence
            const int t = pq < c1 ? rs0 + pq : (pq < c2 ? rs1 + (pq - c1) : (pq < c3 ? rs2 + (pq - c2) : rs3 + (pq - c3)));
            const bool in = pq < L;
            const int j = in ? tidx[t] : -1;
            jv[u] = j;
            if (tb >= 0) {                            // block-uniform: consecutive lanes read consecutive pool entries
                const int tt = in ? t : 0;
                cx[u] = P.tcx[tb + tt]; cy[u] = P.tcy[tb + tt]; cz[u] = P.tcz[tb + tt];
            }
        }
        if (tb < 0) {                                 // the pool was full: gather through the frame indices
#pragma unroll
            for (int u = 0; u < EPL; ++u) {
                const size_t jj = (size_t)max(jv[u], 0);
                cx[u] = P.frame[3 * jj]; cy[u] = P.frame[3 * jj + 1]; cz[u] = P.frame[3 * jj + 2];
            }
        }
    };
    auto publish = [&]() {                            // registers -> the lane group's LDS slice; entries past the sequence as far-away points
#pragma unroll
        for (int u = 0; u < EPL; ++u) {
            const int e = ICP_SPW * u + l16;
            const bool in = jv[u] >= 0;
            px[e] = in ? cx[u] : 1e150; py[e] = in ? cy[u] : 1e150; pz[e] = in ? cz[u] : 1e150; pj[e] = in ? jv[u] : 0x7fffffff;
            pxf[e] = in ? (float)(cx[u] - o0) : 1e30f; pyf[e] = in ? (float)(cy[u] - o1) : 1e30f; pzf[e] = in ? (float)(cz[u] - o2) : 1e30f;
        }
    };
    for (int pass = 0; pass < 2; ++pass) {                            // pass 1 only after a tie was seen: frame-index tie-break
      for (int rb = ra0; rb < ra0 + nrows_all; rb += 16) {
        band(rb);
        if (per > 0) fetch(0);
        for (int t0 = 0; t0 < per; t0 += SB) {
            publish();
            __builtin_amdgcn_wave_barrier();
            if (t0 + SB < per) fetch(t0 + SB);
            NN_STAMP(10);
            const int cnt = min(SB, per - t0);                        // uniform; rounded up to a multiple of 8 (padding is harmless)
            int bm = -1;                                              // slot of this batch's improvement
            if (pass == 0) {
                // Eight entries per step, their distances independent of one another and of `best`; one comparison of the
                // step's minimum with `best`.  (One entry at a time -- compare, select, min against the running best -- is a
                // chain of dependent fp64 operations: 75 ns per entry when a wave has its SIMD to itself, which is the tail
                // of a frame, tests/measure/icp_tail_blocks.py; 60 ns this way.)  bm = the first slot of the batch's minimum
                // if it beats `best` strictly, as before; the tie flag is raised whenever the minimum is attained twice --
                // inside a step, or again in a later step or batch -- which is all the rescan needs.
                for (int t = 0; t < cnt; t += 8) {
                    if (P.screen) {
                        float mf = INFINITY;
#pragma unroll
                        for (int u = 0; u < 8; u += 2) {
                            const nn_f2 X = *(const nn_f2*)(pxf + t + u), Y = *(const nn_f2*)(pyf + t + u), Z = *(const nn_f2*)(pzf + t + u);
                            const nn_f2 fx = nn_f2{sf0, sf0} - X, fy = nn_f2{sf1, sf1} - Y, fz = nn_f2{sf2, sf2} - Z;
                            const nn_f2 e = __builtin_elementwise_fma(fz, fz, __builtin_elementwise_fma(fy, fy, fx * fx));
                            mf = fminf(mf, fminf(e.x, e.y));
                        }
                        ++ct_f32;
                        if (!__ballot(mf <= thr_f)) continue;             // no lane has a target that could matter in this trip
                    }
                    ++ct_f64;
                    double d[8];
#pragma unroll
                    for (int u = 0; u < 8; ++u) {
                        const double dx = s0 - px[t + u], dy = s1 - py[t + u], dz = s2 - pz[t + u];
                        d[u] = (dx * dx + dy * dy) + dz * dz;
                    }
                    const double m = vmin_f64(vmin_f64(vmin_f64(d[0], d[1]), vmin_f64(d[2], d[3])), vmin_f64(vmin_f64(d[4], d[5]), vmin_f64(d[6], d[7])));
                    int first = 7, eq = 0;
#pragma unroll
                    for (int u = 7; u >= 0; --u) { const bool e = d[u] == m; first = e ? u : first; eq += e ? 1 : 0; }
                    const bool lt = m < best;
                    tief |= m == best || (lt && eq > 1);
                    bm = lt ? t + first : bm;
                    best = lt ? m : best;
                    if (P.screen && __ballot(lt)) thr_f = screen_thr(best);
                }
            } else {
                for (int t = 0; t < cnt; ++t) {
                    const double dx = s0 - px[t], dy = s1 - py[t], dz = s2 - pz[t];
                    const double d2 = (dx * dx + dy * dy) + dz * dz;
                    const int j = pj[t];
                    if (d2 < best || (d2 == best && j < bj)) { best = d2; bm = t; bj = j; }
                }
            }
            if (bm >= 0) { bx = px[bm]; by = py[bm]; bz = pz[bm]; bj = pj[bm]; bslot = bm; }
            NN_STAMP(11);
            __builtin_amdgcn_wave_barrier();
        }
      }
        if (pass == 0) {
            if (!__ballot(tief)) break;
            ++ct_tie;
            best = 1e299; bslot = -1; bj = 0x7fffffff;
        }
    }
    }
    if (any) {
        const int nlive = __popcll(__ballot(live && g == 0));
        if (lane == 0) {
            unsigned long long* ct = g_icp_nn_ct[blockIdx.x & (ICP_CT_SHARDS - 1)];
            atomicAdd(ct + 0, 1ull); atomicAdd(ct + 3, (unsigned long long)nlive);
            if (ct_f32) atomicAdd(ct + 1, (unsigned long long)ct_f32);
            if (ct_f64) atomicAdd(ct + 2, (unsigned long long)ct_f64);
            if (ct_tie) atomicAdd(ct + 4, (unsigned long long)ct_tie);
        }
    }
    ICP_BLK(if (tid == 0 && blk_rec) { g_icp_blk[0][blockIdx.x] = blk_t0; g_icp_blk[5][blockIdx.x] = gridDim.x;
                                       g_icp_blk[1][blockIdx.x] = wall_clock64(); g_icp_blk[2][blockIdx.x] = blk_per;
                                       g_icp_blk[3][blockIdx.x] = ((unsigned long long)nrows_all << 16) | (unsigned)(cb1 - cb0 + 1); g_icp_blk[4][blockIdx.x] = c; })
    if (bslot < 0) { best = INFINITY; bj = 0x7fffffff; }              // a lane group whose rows were all empty has no candidate
    ICP_STAMPED(if (lane == 0 && any && tailonly) { atomicAdd(&g_icp_stamps[7], clock64() - stt); if (tief) atomicAdd(&g_icp_stamps[2], 1ull); })
    // the four lane groups of a source: (distance, frame index) lexicographic minimum, the winner's coordinates along
    for (int o = ICP_SPW; o < 64; o <<= 1) {
        const double od = __shfl_xor(best, o, 64); const int oj = __shfl_xor(bj, o, 64);
        const double ox = __shfl_xor(bx, o, 64), oy = __shfl_xor(by, o, 64), oz = __shfl_xor(bz, o, 64);
        if (od < best || (od == best && oj < bj)) { best = od; bj = oj; bx = ox; by = oy; bz = oz; }
    }
    NN_STAMP(12);
#ifdef CREG_ICP_RECT_STATS
    {   // measurement build (tests/measure/icp_rect_stats.py): the entries of the cell rectangle this wave SCANNED (from the distances to the
        // previous matches) against those of the rectangle its FINAL nearest distances would have needed -- what a centre-out scan with a
        // shrinking radius could save at most
        double fal = INFINITY, fah = -INFINITY, fbl = INFINITY, fbh = -INFINITY;
        if (live) {
            const double sa = axa == 0 ? s0 : (axa == 1 ? s1 : s2), sb = axb == 0 ? s0 : (axb == 1 ? s1 : s2);
            if (bj != 0x7fffffff) { const double r1 = sqrt(best) * (1.0 + 1e-12) + 1e-300; fal = sa - r1; fah = sa + r1; fbl = sb - r1; fbh = sb + r1; }
            else { fal = -INFINITY; fah = INFINITY; fbl = -INFINITY; fbh = INFINITY; }
        }
        const int fa0 = __builtin_amdgcn_readfirstlane(icp_bin(wave_min_fast(fal), x0a, inv_a, gd)), fa1 = __builtin_amdgcn_readfirstlane(icp_bin(wave_max_fast(fah), x0a, inv_a, gd));
        const int fb0 = __builtin_amdgcn_readfirstlane(icp_bin(wave_min_fast(fbl), x0b, inv_b, gd)), fb1 = __builtin_amdgcn_readfirstlane(icp_bin(wave_max_fast(fbh), x0b, inv_b, gd));
        int e1 = 0, e0 = 0;
        if (any) {
            if (lane <= fa1 - fa0) e1 = tst[(fa0 + lane) * gd + fb1 + 1] - tst[(fa0 + lane) * gd + fb0];
            if (lane <= ra1 - ra0) e0 = tst[(ra0 + lane) * gd + cb1 + 1] - tst[(ra0 + lane) * gd + cb0];
            for (int o = 32; o >= 1; o >>= 1) { e1 += __shfl_xor(e1, o, 64); e0 += __shfl_xor(e0, o, 64); }
            if (lane == 0) {
                unsigned long long* ct = g_icp_nn_ct[blockIdx.x & (ICP_CT_SHARDS - 1)];
                atomicAdd(ct + 5, (unsigned long long)e1); atomicAdd(ct + 6, (unsigned long long)e0);
                atomicAdd(ct + 7, (unsigned long long)((ra1 - ra0 + 1) * (cb1 - cb0 + 1)) | ((unsigned long long)((fa1 - fa0 + 1) * (fb1 - fb0 + 1)) << 32));
            }
        }
    }
#endif
    double cm[ICP_NM];
    for (int a = 0; a < ICP_NM; ++a) cm[a] = 0;
    if (live && g == 0) {
        const bool ok = bj != 0x7fffffff && best < th2;
        P.nn[i] = ok ? bj : -1;
        if (ok) {
            P.prevt[3 * (size_t)i] = bx; P.prevt[3 * (size_t)i + 1] = by; P.prevt[3 * (size_t)i + 2] = bz;
            const double sv[3] = {s0 - shc0, s1 - shc1, s2 - shc2};
            const double dv[3] = {bx - shc0, by - shc1, bz - shc2};
            cm[0] = 1.0; cm[1] = best;
            for (int a = 0; a < 3; ++a) { cm[2 + a] = sv[a]; cm[5 + a] = dv[a]; }
            for (int a = 0; a < 3; ++a) for (int q = 0; q < 3; ++q) cm[8 + 3 * a + q] = sv[a] * dv[q];
        }
    }
    // the chunk's moments: DPP wave sums, then 0 + w0 + w1 + w2 + w3 (fixed association)
#pragma unroll
    for (int a = 0; a < ICP_NM; ++a) cm[a] = wave_sum_fast(cm[a]);
    if (lane == 0) {
#pragma unroll
        for (int a = 0; a < ICP_NM; ++a) sc[wv * ICP_NM + a] = cm[a];
    }
    NN_STAMP(13);
    __syncthreads();
    NN_STAMP(14);
    if (tid < ICP_NM) {
        double r = 0.0;
        for (int w = 0; w < ICP_NNW; ++w) r += sc[w * ICP_NM + tid];
        st_agent_f64(P.part + (size_t)blk * ICP_NM + tid, r);
    }
    // the cluster's last chunk to get here runs the fit.  A bare s_barrier does not wait for the st_agent_f64 stores
    // above: the storing wave drains its vmcnt explicitly before the barrier, so the partial moments are acknowledged by
    // the memory side before thread 0 bumps the arrival counter (P.part is reused by every iteration launch: without the
    // drain the last chunk could read the previous iteration's moments).
    __shared__ int s_last;
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    __syncthreads();
    if (tid == 0) {
        const int nch = P.chunk0[c + 1] - P.chunk0[c];
        const int last = atomicAdd(&P.arrive[c], 1) == nch - 1;
        if (last) P.arrive[c] = 0;                                    // for the next launch
        s_last = last;
    }
    __syncthreads();
    ICP_STAMPED(if (tid == 0 && tailonly) atomicMax(&g_icp_wmin[2], wall_clock64());)
    if (s_last && wv == 0) icp_fit_cluster(P, c, max_iter, lane);
    ICP_STAMPED(if (s_last && tid == 0 && tailonly) atomicMax(&g_icp_wmin[3], wall_clock64());
                if (tid == 0 && tailonly) atomicAdd(&g_icp_stamps[15], 1ull);)
}

__global__ __launch_bounds__(256) void k_icp_finish(IcpLarge P, int keep_t) {
    __shared__ double T[16];
    const int k = blockIdx.x, tid = threadIdx.x;
    const double* st = P.state + ICP_ST * k;
    if (tid < 16) T[tid] = st[tid];
    __syncthreads();
    if (tid == 0 && keep_t) { T[3] = P.Min[16 * k + 3]; T[7] = P.Min[16 * k + 7]; T[11] = P.Min[16 * k + 11]; }
    __syncthreads();
    if (tid < 16) P.Mout[16 * k + tid] = T[tid];
    if (tid == 0) P.n_iter_out[k] = (int)st[35];
    const int b = P.off[k], e = P.off[k + 1];
    for (int i = b + tid; i < e; i += 256) {
        const double* p = P.local + 3 * (size_t)i;
        for (int a = 0; a < 3; ++a)
            P.world_out[3 * (size_t)i + a] = fma(T[4 * a + 2], p[2], fma(T[4 * a + 1], p[1], T[4 * a] * p[0])) + T[4 * a + 3];
    }
}

// The workspace of one problem, described once: with a base it binds P's buffers (and pool_cap), with a null base it only
// measures.  Returns the bytes either way.  Every buffer starts on a multiple of 256.
static size_t icp_large_carve(int64_t n, int64_t nf, int k, char* base, IcpLarge& P) {
    size_t o = 0;
    auto take = [&](auto*& p, size_t count) {
        p = base ? (std::remove_reference_t<decltype(p)>)(base + o) : nullptr;
        o = align_up(o + sizeof(*p) * count, 256);
    };
    const size_t chunks = (size_t)(n / ICP_CH + k + 1);               // an upper bound of sum_c ceil(ns_c / ICP_CH)
    take(P.srcw, 3 * (size_t)n); take(P.tidx, (size_t)k * nf); take(P.tcount, k); take(P.box, 6 * (size_t)k); take(P.nn, n);
    take(P.part, ICP_NM * chunks); take(P.state, ICP_ST * (size_t)k); take(P.running, 4); take(P.chunk0, k + 1);
    take(P.tst, (size_t)k * (ICP_NCELL + 1)); take(P.chunk_cl, chunks); take(P.prevt, 3 * (size_t)n);
    // coordinate pool: room for 4 nf masked targets over all clusters (they overlap by the box scale: ~1.5 nf in practice);
    // clusters beyond it fall back to gathering
    const int64_t cap = 4 * nf < (int64_t)k * nf ? 4 * nf : (int64_t)k * nf;
    P.pool_cap = (int)(cap < (1ll << 30) ? cap : (1ll << 30));
    take(P.tcx, P.pool_cap); take(P.tcy, P.pool_cap); take(P.tcz, P.pool_cap);
    take(P.tbase, k); take(P.arrive, k); take(P.live, chunks); take(P.tcf, P.pool_cap); take(P.tlmax, k);
    return o;
}
size_t icp_large_workspace_bytes(int64_t n, int64_t nf, int k) { IcpLarge P; return icp_large_carve(n, nf, k, nullptr, P); }

// The host follows the device one batch of launches behind: after every batch the two counters {clusters still iterating, their
// chunks} are copied into a slot of this pinned ring, and the host reads slot b - 1 once batch b is in the queue.  One ring per
// host thread, used from whichever stream and device the thread's calls run on (hipHostMallocPortable).  The rule it keeps: a
// call returns with its last copy still in flight, so the NEXT call on this thread must not reuse the slots before that copy has
// landed -- a late copy would overwrite the new call's counters, typically with "0 clusters running", and end its loop early.
// Released when the thread ends (a thread's objects go before the process's atexit handlers and static destructors, so the HIP
// runtime is still loaded for the main thread's, too); never from a static destructor.
struct IcpLagRing {
    static constexpr int SLOTS = 4;
    int* h = nullptr;                                                // pinned: SLOTS x {clusters running, live chunks}
    hipEvent_t last = nullptr;                                       // behind the LAST copy into h of this thread's previous call
    IcpLagRing() = default;
    IcpLagRing(const IcpLagRing&) = delete;
    ~IcpLagRing() { wait_previous(); if (h) (void)hipHostFree(h); }
    hipError_t acquire() { return h ? hipSuccess : hipHostMalloc((void**)&h, sizeof(int) * 2 * SLOTS, hipHostMallocPortable); }
    void wait_previous() { if (last) { (void)hipEventSynchronize(last); (void)hipEventDestroy(last); last = nullptr; } }
    int* slot(int b) { return h + 2 * (b % SLOTS); }
    // after the call's last copy is enqueued on s; if no event can stand behind it, the copy is waited for here
    void mark_last(hipStream_t s) {
        if (hipEventCreateWithFlags(&last, hipEventDisableTiming) != hipSuccess) last = nullptr;
        else if (hipEventRecord(last, s) != hipSuccess) { (void)hipEventDestroy(last); last = nullptr; }
        if (!last) (void)hipStreamSynchronize(s);
    }
};

// creg_icp_nn_counters (measurement hook, for one host thread and the current device: plain host state): while `on` is set every
// k_icp_nn launch is bracketed by two HIP events on the launch stream and the call ends with a stream synchronisation that adds
// their elapsed times to the two tallies.
static struct { bool on = false; double us = 0.0; long long launches = 0; } g_icp_nn_timing;

// One problem through the multi-launch path.  The host follows the device one batch of iterations behind (no stream synchronisation;
// it returns when the convergence it has read back says so, with the last launches and k_icp_finish still in the queue).
int icp_large_run(const creg_icp_problem& q, int64_t n, int32_t k, int64_t nf, double scale, double th, int32_t max_iteration,
                  int32_t keep_translation, int screen, char* ws, hipStream_t s) {
    IcpLarge P;
    P.local = q.local; P.world = q.world; P.off = q.seg_offsets; P.woff = q.world_offsets; P.frame = q.frame; P.Min = q.M;
    P.toff = q.tgt_offsets;                          // point-to-point mode: the cluster's own target segment, no mask
    P.Mout = q.M_out; P.world_out = q.world_out; P.n_iter_out = q.n_iter_out;
    P.use_live = 0; P.screen = screen;
    icp_large_carve(n, nf, k, ws, P);
    const int nn_smem = ICP_NNW * ICP_G * (ICP_SB + 2) * 40;  // k_icp_nn: per wave 4 lane groups x ICP_SB (+2: bank offset) staged targets (x, y, z fp64, frame index, x, y, z float32)
    // ---- set-up, in the queue before the host waits for anything.  Nothing below touches the ring until the loop's first
    // copy is enqueued, so a failure up to there is a plain return.
    CREG_HIP(hipFuncSetAttribute((const void*)k_icp_nn, hipFuncAttributeMaxDynamicSharedMemorySize, nn_smem));
    hipLaunchKernelGGL(k_icp_mask, dim3(k), dim3(1024), 0, s, P, (int)nf, (float)(0.5 * scale), q.world ? 0 : 1, 1);
    hipLaunchKernelGGL(k_icp_init, dim3(k), dim3(1024), 0, s, P, k);
    hipLaunchKernelGGL(k_icp_pool, dim3(k, 8), dim3(256), 0, s, P, (int)nf);
    if (P.screen) hipLaunchKernelGGL(k_icp_seed, dim3(k, 8), dim3(256), 0, s, P, (int)nf);
    CREG_LAUNCH_CHECK();
    static thread_local IcpLagRing ring;
    CREG_HIP(ring.acquire());
    ring.wait_previous();
    ScopedEvents ev(IcpLagRing::SLOTS), tev;                         // (tev: timing mode only)
    for (auto& e : ev.v) CREG_HIP(hipEventCreateWithFlags(&e, hipEventDisableTiming));
    auto time_mark = [&] {                                           // one end of a timed launch's bracket
        hipEvent_t e;
        if (g_icp_nn_timing.on && hipEventCreate(&e) == hipSuccess) { (void)hipEventRecord(e, s); tev.v.push_back(e); }
    };
    // ---- the loop.  Every launch is one search + (last chunk of each cluster) one fit = one convergence test and, unless
    // converged, one update; max_iteration updates need one launch more.  After every batch of 16 launches the live chunks are
    // compacted on the device and the two counters come back through the ring -- but the host does not wait for a batch before
    // it enqueues the next one: it reads the counters of batch b - 1 after batch b is in the queue, so the device always has a
    // batch ahead; the price is at most one surplus batch of launches whose workgroups all leave at once.
    FirstError fe;
    int grid = cdiv(n, ICP_CH) + k;                                  // live chunks as of the last batch whose counters were read; at first
                                                                     // an upper bound of sum_c ceil(ns_c / ICP_CH): the surplus blocks exit
    bool converged = false;
    int64_t done = 0;
    for (int b = 0; fe.ok() && !converged && done <= (int64_t)max_iteration; ++b) {
        for (int i = 0; i < 16; ++i, ++done) {
            time_mark();
            hipLaunchKernelGGL(k_icp_nn, dim3(grid), dim3(64 * ICP_NNW), nn_smem, s, P, (int)n, k, (int)nf, th * th, max_iteration);
            time_mark();
            ICP_STAMPED(hipLaunchKernelGGL(k_icp_wall_fold, dim3(1), dim3(1), 0, s);)
        }
        hipLaunchKernelGGL(k_icp_compact, dim3(1), dim3(1024), 0, s, P, k);
        CREG_TRY(fe, hipGetLastError());
        CREG_TRY(fe, hipMemcpyAsync(ring.slot(b), P.running, 2 * sizeof(int), hipMemcpyDeviceToHost, s));
        CREG_TRY(fe, hipEventRecord(ev[b % IcpLagRing::SLOTS], s));
        P.use_live = 1;
        if (b >= 1) CREG_TRY(fe, hipEventSynchronize(ev[(b - 1) % IcpLagRing::SLOTS]));
        if (b >= 1 && fe.ok()) {                                     // the counters of the batch BEFORE the one just enqueued
            const int* r = ring.slot(b - 1);
            converged = r[0] <= 0;
            grid = r[1] > 0 ? r[1] : 1;
        }
    }
    // (the last batch's counters are not read: nothing is left to decide, k_icp_finish reads the device state)
    ring.mark_last(s);                                               // from the first copy on, every way out passes here
    if (!fe.ok()) { set_error("creg_masked_icp: HIP error in the iteration loop: %s", hipGetErrorString(fe.err)); return CREG_EHIP; }
    hipLaunchKernelGGL(k_icp_finish, dim3(k), dim3(256), 0, s, P, keep_translation);
    CREG_LAUNCH_CHECK();
    if (!tev.v.empty()) {
        (void)hipStreamSynchronize(s);
        for (size_t i = 0; i + 1 < tev.v.size(); i += 2) {
            float ms = 0.f;
            if (hipEventElapsedTime(&ms, tev[i], tev[i + 1]) == hipSuccess) { g_icp_nn_timing.us += 1e3 * ms; ++g_icp_nn_timing.launches; }
        }
    }
    return CREG_OK;
}

}  // namespace creg
using namespace creg;

extern "C" int creg_icp_nn_counters(double* out8, int32_t reset, int32_t timing) {
    if (out8) {
        static unsigned long long c[ICP_CT_SHARDS][8];
        CREG_HIP(hipMemcpyFromSymbol(c, HIP_SYMBOL(creg::g_icp_nn_ct), sizeof(c)));
        for (int i = 0; i < 5; ++i) { double t = 0.0; for (int sh = 0; sh < ICP_CT_SHARDS; ++sh) t += (double)c[sh][i]; out8[i] = t; }
        out8[5] = g_icp_nn_timing.us; out8[6] = (double)g_icp_nn_timing.launches; out8[7] = 0.0;
    }
    if (reset) {
        static const unsigned long long z[ICP_CT_SHARDS][8] = {};
        CREG_HIP(hipMemcpyToSymbol(HIP_SYMBOL(creg::g_icp_nn_ct), z, sizeof(z)));
        g_icp_nn_timing.us = 0.0; g_icp_nn_timing.launches = 0;
    }
    if (timing >= 0) g_icp_nn_timing.on = timing != 0;
    return CREG_OK;
}

extern "C" int creg_aabb_mask_f64(const float* world, const int32_t* world_offsets, int32_t k, const double* frame, int64_t nf,
                                  double scale, int32_t* mask_idx, int32_t* mask_count, float* boxes, creg_stream_t stream) {
    CREG_REQUIRE(world && world_offsets && frame && mask_idx && mask_count && k >= 1 && nf >= 1 && nf < (1ll << 31),
                 "creg_aabb_mask_f64: bad argument");
    IcpLarge P{};
    P.world = world; P.off = world_offsets; P.woff = world_offsets; P.frame = frame; P.toff = nullptr;
    P.tidx = mask_idx; P.tcount = mask_count; P.box = boxes;
    hipLaunchKernelGGL(k_icp_mask, dim3(k), dim3(1024), 0, (hipStream_t)stream, P, (int)nf, (float)(0.5 * scale), 0, 0);
    CREG_LAUNCH_CHECK();
    return CREG_OK;
}

// ---- read-backs of the measurement builds (tests/measure/)
#ifdef CREG_ICP_RECT_STATS
extern "C" int creg_debug_icp_rect(double* out4) {      // entries of the final-distance rectangles, of the scanned ones, cells scanned, cells needed (sums over waves)
    static unsigned long long c[ICP_CT_SHARDS][8];
    CREG_HIP(hipMemcpyFromSymbol(c, HIP_SYMBOL(creg::g_icp_nn_ct), sizeof(c)));
    out4[0] = out4[1] = out4[2] = out4[3] = 0.0;
    for (int sh = 0; sh < ICP_CT_SHARDS; ++sh) { out4[0] += (double)c[sh][5]; out4[1] += (double)c[sh][6]; out4[2] += (double)(c[sh][7] & 0xffffffffull); out4[3] += (double)(c[sh][7] >> 32); }
    return CREG_OK;
}
#endif
#ifdef CREG_ICP_BLK
extern "C" int creg_debug_icp_blk(unsigned long long* out) {
    CREG_HIP(hipMemcpyFromSymbol(out, HIP_SYMBOL(creg::g_icp_blk), sizeof(unsigned long long) * 6 * 8192));
    return CREG_OK;
}
#endif
#ifdef CREG_STAMPS
extern "C" int creg_debug_icp_wall(unsigned long long* out8, int reset) {
    if (out8) CREG_HIP(hipMemcpyFromSymbol(out8, HIP_SYMBOL(creg::g_icp_wall), sizeof(unsigned long long) * 8));
    if (reset) { unsigned long long z[8] = {0, 0, 0, 0, 0, 0, 0, 0}; CREG_HIP(hipMemcpyToSymbol(HIP_SYMBOL(creg::g_icp_wall), z, sizeof(z)));
                 unsigned long long m[4] = {~0ull, ~0ull, 0ull, 0ull}; CREG_HIP(hipMemcpyToSymbol(HIP_SYMBOL(creg::g_icp_wmin), m, sizeof(m))); }
    return CREG_OK;
}
// the stamps of both regimes' kernels (a run is in one regime: the other unit's copy holds zeros)
extern "C" int creg_debug_icp_stamps(unsigned long long* out8, int reset) {
    if (out8) for (int i = 0; i < 512 * 16; ++i) out8[i] = 0;
    const int rc = icp_stamps_add(out8, reset);
    return rc ? rc : icp_small_stamps(out8, reset);
}
#endif
