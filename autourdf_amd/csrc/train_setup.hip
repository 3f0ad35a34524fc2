// train_setup.hip -- the train plan's once-per-train launches: the problems' inputs into their workspaces (k_copy_table, k_prep, k_l1),
// the k-d leaves of the two clouds (k_sort_y, k_sort_p), and the state in / out of a resumed run (k_set_state, k_get_state,
// k_params_home).  None of them is inside the epoch loop.
#include <cfloat>
#include <cmath>
#include <cstring>
#include "train_dev.h"

namespace creg {

// ------------------------------------------------------------------------------------------ prep
// per-problem inputs of a batch (grid.z): one launch stages all of them
constexpr int PREP_MAXB = 64;
static_assert(PREP_MAXB == BATCH_MAX, "k_prep's tables hold a whole batch");
struct PrepBatch { const float* m[PREP_MAXB]; const float* y[PREP_MAXB]; const float* pts[PREP_MAXB]; Hyper hy[PREP_MAXB]; };
__global__ __launch_bounds__(256) void k_prep(Dims D, Ws W0, size_t bstride, PrepBatch pb) {
    const Ws W = ws_shift(W0, blockIdx.z * bstride);
    const Hyper hy = pb.hy[blockIdx.z];
    const float* __restrict__ m = pb.m[blockIdx.z];
    const float* __restrict__ y = pb.y[blockIdx.z];
    const float* __restrict__ pts = pb.pts[blockIdx.z];
    const int t = blockIdx.x * 256 + threadIdx.x;
    const int stride = gridDim.x * 256;
    for (int n = t; n < D.NP; n += stride) {
        const int c = seg_of(W.off, D.K, n);
        W.pts4[n] = make_float4(pts[3 * (size_t)n], pts[3 * (size_t)n + 1], pts[3 * (size_t)n + 2], __int_as_float(c));
    }
    for (int j = t; j < D.NT; j += stride)
        W.y4[j] = make_float4(y[3 * (size_t)j], y[3 * (size_t)j + 1], y[3 * (size_t)j + 2], 0.f);
    for (int i = t; i < D.NPAR; i += stride) { W.AM[i] = 0.f; W.AV[i] = 0.f; }
    for (int i = t; i < D.epochs; i += stride) { W.loss_hist[i] = NAN; W.lr_hist[i] = NAN; }
    // pose rows K .. KP-1 of the K-row matrices: zero for the whole train (k_bd's D role contracts over KP rows; nobody writes them)
    for (int i = t; i < (D.KP - D.K) * D.H; i += stride) { W.x1[0][D.K * D.H + i] = 0.f; W.x1[1][D.K * D.H + i] = 0.f; }
    for (int i = t; i < (D.KP - D.K) * D.H2; i += stride) { W.h2[0][D.K * D.H2 + i] = 0.f; W.h2[1][D.K * D.H2 + i] = 0.f; W.g_h2[D.K * D.H2 + i] = 0.f; }
    for (int i = t; i < (D.KP - D.K) * 16; i += stride) W.g_out[D.K * 16 + i] = 0.f;
    for (int i = t; i <= D.epochs; i += stride) { W.bc1[i] = 1.0 - pow(0.9, (double)i); W.bc2s[i] = (float)sqrt(1.0 - pow(0.999, (double)i)); }
    if (blockIdx.x == 0) {
        for (int r = threadIdx.x; r < D.K; r += 256) {
            const float* M = m + 16 * r;
            const float R[9] = {M[0], M[1], M[2], M[4], M[5], M[6], M[8], M[9], M[10]};
            const float tr[3] = {M[3], M[7], M[11]};
            float in[POSE_IN];
            for (int i = 0; i < POSE_IN; ++i) in[i] = 0.f;
            int nin;
            if (D.rot == ROT_Q) {                 // cat([t, matrix_to_quaternion(R)])  mlp_reg.py:65-66
                float q[4];
                matrix_to_quat(R, q);
                in[0] = tr[0]; in[1] = tr[1]; in[2] = tr[2]; in[3] = q[0]; in[4] = q[1]; in[5] = q[2]; in[6] = q[3];
                nin = 7;
            } else if (D.rot == ROT_DQ) {         // transform_to_dualquat  mlp_reg.py:80
                se3_to_dq(R, tr, in, FLT_EPSILON);
                nin = 8;
            } else if (D.rot == ROT_6D) {         // cat([t, matrix_to_rotation_6d(R)]): the first two rows  mlp_reg.py:87-88
                in[0] = tr[0]; in[1] = tr[1]; in[2] = tr[2];
                for (int i = 0; i < 6; ++i) in[3 + i] = R[i];
                nin = 9;
            } else {                              // cat([t, matrix_to_euler_angles(R, "XYZ")])  mlp_reg.py:73-74
                in[0] = tr[0]; in[1] = tr[1]; in[2] = tr[2];
                matrix_to_euler_xyz(R, in + 3);
                nin = 6;
            }
            for (int i = 0; i < POSE_IN; ++i) W.pose_in[POSE_IN * r + i] = in[i];
            // [sin x, cos x, sin 2x, cos 2x, sin 4x, cos 4x, sin 8x, cos 8x]  model_utils.py:141-150
            float* e = W.enc + (size_t)r * D.IN;
            for (int f = 0; f < 4; ++f) {
                const float mul = (float)(1 << f);
                for (int i = 0; i < nin; ++i) {
                    e[(2 * f) * nin + i] = sinf(mul * in[i]);
                    e[(2 * f + 1) * nin + i] = cosf(mul * in[i]);
                }
            }
        }
        if (threadIdx.x == 0) {
            TrainState s;
            *W.hyper = hy;
            s.lr = (double)hy.lr; s.sched_best = INFINITY; s.sched_bad = 0; s.count = 0; s.stopped = 0;
            s.step = 0; s.min_loss = 1000.f; s.epochs_run = 0; s.best_epoch = -1; s.step_size = 0.f;
            s.bc2_sqrt = 1.f; s.last_loss = NAN;
            s.next_bc1 = 1.0 - 0.9; s.next_bc2s = (float)sqrt(1.0 - 0.999);         // step 1 (the tables are filled by this launch)
            W.state[0] = s; W.state[1] = s;
        }
    }
}

// ------------------------------------------------------------------------------------------ layer 1 (epoch 0 only)
__global__ __launch_bounds__(256) void k_l1(Dims D, Ws W0, int par, size_t bstride) {
    const Ws W = ws_shift(W0, blockIdx.z * bstride);
    const int lane = threadIdx.x & 63;
    const int o = blockIdx.x * 4 + (threadIdx.x >> 6);
    if (o >= D.H) return;
    const float w = lane < D.IN ? W.P[D.oW1 + (size_t)o * D.IN + lane] : 0.f;
    const float w2 = 64 + lane < D.IN ? W.P[D.oW1 + (size_t)o * D.IN + 64 + lane] : 0.f;      // ('6d': 72 features)
    const float b = W.P[D.ob1 + o];
    for (int r = 0; r < D.K; ++r) {
        float t = lane < D.IN ? w * W.enc[(size_t)r * D.IN + lane] : 0.f;
        if (64 + lane < D.IN) t = fmaf(w2, W.enc[(size_t)r * D.IN + 64 + lane], t);
        const float v = wave_sum_fast(t) + b;
        if (lane == 0) (par ? W.x1[1] : W.x1[0])[(size_t)r * D.H + o] = act_f(v, D.slope);      // (a runtime index into the shifted struct put all of it -- 312 bytes a lane -- into scratch)
    }
}

// ------------------------------------------------------------------------------------------ target blocks
// Once per train: the target frame (it does not move during the 300 epochs) cut into blocks of BS = 64 * D.ppl
// points with an axis-aligned box each, for nn_l1_block_pruned.  The blocks are the leaves of a balanced k-d tree
// -- sort all slots on x and halve, sort each half on y and halve, ... (x,y,z,x,y,z: a 4 x 4 x 4 grid in rank
// space for 64 leaves) -- so the boxes of different blocks do not overlap and a query usually has to look into one
// to three of them (Morton-curve blocks, tried first, overlapped enough to need eight).  One workgroup per problem;
// every level is a bitonic sort of the slots in LDS restricted to segments of npow >> level, keys = (order-preserving
// bits of the coordinate, original index): unique, so the layout is deterministic.  Slots past n_tgt hold +inf keys
// and stay at the end through every level.  Any permutation gives the same search result -- ties are broken on the
// original index stored with the point -- so none of this is visible in the plan's outputs.
__device__ __forceinline__ unsigned ordered_bits(float c) {                // total order of the floats, below 0xFFFFFFFF
    unsigned u = (unsigned)__float_as_int(c);
    u = (u & 0x80000000u) ? ~u : (u | 0x80000000u);
    return u == 0xFFFFFFFFu ? 0xFFFFFFFEu : u;
}
// ascending bitonic sort of key[0, npow) restricted to aligned segments of `seg` slots.
// A wave's 64 compare-exchanges of a stage with stride <= 64 stay inside its own 128 consecutive slots (and so do
// those of its later trips), so runs of such stages need no workgroup barrier -- the wave's DS instructions execute
// in order; only stages with a longer stride, and the hand-over to / from them, synchronise the workgroup: 35 barrier
// pairs instead of 308 stages with one for the six k-d levels of 4096 slots.
__device__ __forceinline__ void bitonic_segments(unsigned long long* key, int npow, int seg, int tid, int nthreads) {
    bool wide_before = true;                                   // the caller's writes count as a wide stage
    for (int size = 2; size <= seg; size <<= 1)
        for (int stride = size >> 1; stride >= 1; stride >>= 1) {
            const bool wide = stride > 64;
            if (wide || wide_before) __syncthreads();
            else { __builtin_amdgcn_fence(__ATOMIC_SEQ_CST, "wavefront"); __builtin_amdgcn_wave_barrier(); }
            for (int t = tid; t < (npow >> 1); t += nthreads) {
                const int i = ((t & ~(stride - 1)) << 1) | (t & (stride - 1)), j = i | stride;
                const unsigned long long a = key[i], b = key[j];
                const bool up = size == seg || (i & size) == 0;            // every segment ends ascending
                if ((a > b) == up) { key[i] = b; key[j] = a; }
            }
            wide_before = wide;
        }
    __syncthreads();
}
static int pow2_at_least(int n) { int p = 64; while (p < n) p <<= 1; return p; }

// Frames above YS_CHUNK = 16384 points (the keys of one workgroup's LDS) are cut in index order into chunks of that size,
// one workgroup (grid.x) and one set of 64 leaves of 256 points each: every chunk is a sample of the whole frame, so a
// query has to look into at least one block per chunk -- a few times the work of a single tree, still a small fraction of
// the exhaustive sweep (round 2 fell back to it above 16384 targets).
// check != 0 (round 5): the caller says the frame is the one the leaves were built from (creg_train_args.y_unchanged) -- the
// workgroup first compares a position-dependent 64-bit fingerprint of its chunk of the staged frame with the one stored when the leaves
// were built and returns if they agree (a launch of a few microseconds instead of the sort: 145 us at 4096 points, 657 at 16384);
// a frame that differs -- a buffer reused for the next frame, two registrars sharing a plan -- is sorted again instead of being
// searched through stale leaves.
__global__ __launch_bounds__(1024) void k_sort_y(Dims D, Ws W0, size_t bstride, int npow, int check) {
    const Ws W = ws_shift(W0, blockIdx.z * bstride);
    extern __shared__ __attribute__((aligned(16))) char smem_raw[];
    unsigned long long* key = (unsigned long long*)smem_raw;               // npow keys
    const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
    const int BS = 64 * D.ppl;
    const int base = blockIdx.x * YS_CHUNK, nc = min(YS_CHUNK, D.NT - base);        // this chunk's targets [base, base + nc)
    const int blk0 = base / BS, nblk = (nc + BS - 1) / BS;                            // its blocks [blk0, blk0 + nblk)
    __shared__ unsigned long long s_fp;
    {
        if (tid == 0) s_fp = 0ull;
        __syncthreads();
        unsigned long long h = 0ull;
        for (int j = tid; j < nc; j += 1024) {
            const float4 p = W.y4[base + j];
            const unsigned long long a = (unsigned)__float_as_int(p.x), b = (unsigned)__float_as_int(p.y), c = (unsigned)__float_as_int(p.z);
            unsigned long long v = a ^ (b << 21) ^ (c << 42) ^ (c >> 22);
            v *= 0x9E3779B97F4A7C15ull;                                               // (mix, then weigh by the position: a permuted frame differs)
            h += (v ^ (v >> 29)) * (2ull * (unsigned long long)j + 1ull);
        }
        atomicAdd(&s_fp, h);                                                          // integer sum: order independent
        __syncthreads();
        const unsigned long long fp = s_fp ^ ((unsigned long long)nc << 48) ^ (unsigned long long)D.ppl ^ ((unsigned long long)D.rows << 8);
        if (check && W.ysum[blockIdx.x] == fp) return;                                // workgroup-uniform: the leaves are this frame's
        __syncthreads();
        if (tid == 0) W.ysum[blockIdx.x] = fp;
    }
    for (int j = tid; j < npow; j += 1024) key[j] = j < nc ? (unsigned long long)j : ~0ull;
    __syncthreads();
    int level = 0;
    // (D.rows: the sixteen-queries-per-wave search takes its QUERIES from these slots too, 16 consecutive ones per wave -- two more
    //  levels make every aligned group of 16 slots a k-d cell of its leaf: the fewer target blocks the sixteen need between them)
    for (int seg = npow; seg > (D.rows ? 16 : BS); seg >>= 1, ++level) {
        const int axis = level % 3;
        for (int j = tid; j < npow; j += 1024) {
            const unsigned long long k = key[j];
            if (k != ~0ull) {
                const int idx = (int)(k & 0xFFFFull);
                const float4 p = W.y4[base + idx];
                key[j] = ((unsigned long long)ordered_bits(axis == 0 ? p.x : axis == 1 ? p.y : p.z) << 32) | (unsigned)idx;
            }
        }
        __syncthreads();
        bitonic_segments(key, npow, seg, tid, 1024);
    }
    // sorted slots + per-block boxes: wave w handles the 64-slot groups w, w + 16, ...; a block is D.ppl groups
    float* boxes = (float*)(key + npow);                                   // [group][6] scratch behind the keys
    const int groups = nblk * D.ppl;
    for (int gq = wv; gq < groups; gq += 16) {
        const unsigned long long k = key[gq * 64 + lane];
        float4 p = make_float4(INFINITY, INFINITY, INFINITY, __int_as_float(0x7fffffff));
        float l[3] = {INFINITY, INFINITY, INFINITY}, h[3] = {-INFINITY, -INFINITY, -INFINITY};
        if (k != ~0ull) {
            const int j = base + (int)(k & 0xFFFFull);
            const float4 y = W.y4[j];
            p = make_float4(y.x, y.y, y.z, __int_as_float(j));
            l[0] = h[0] = y.x; l[1] = h[1] = y.y; l[2] = h[2] = y.z;
        }
        W.ys4[(size_t)blk0 * BS + gq * 64 + lane] = p;
#pragma unroll
        for (int c = 0; c < 3; ++c)
            for (int off = 32; off >= 1; off >>= 1) {
                l[c] = fminf(l[c], __shfl_xor(l[c], off, 64));
                h[c] = fmaxf(h[c], __shfl_xor(h[c], off, 64));
            }
        if (lane == 0) {
            float* o = boxes + 6 * gq;
            o[0] = l[0]; o[1] = l[1]; o[2] = l[2]; o[3] = h[0]; o[4] = h[1]; o[5] = h[2];
        }
    }
    __syncthreads();
    for (int b = tid; b < nblk; b += 1024) {
        float o[6] = {INFINITY, INFINITY, INFINITY, -INFINITY, -INFINITY, -INFINITY};
        for (int g = 0; g < D.ppl; ++g)
            for (int c = 0; c < 3; ++c) {
                o[c] = fminf(o[c], boxes[6 * (b * D.ppl + g) + c]);
                o[3 + c] = fmaxf(o[3 + c], boxes[6 * (b * D.ppl + g) + 3 + c]);
            }
        for (int c = 0; c < 6; ++c) W.ybox[c * 64 * D.nbt + blk0 + b] = o[c];     // six planes of 64 nbt boxes
    }
}

// The same for the predicted cloud, whose points move rigidly with their cluster every epoch: each cluster's
// LOCAL points are cut into k-d leaves of BS once per train (a cluster of n points owns ceil(n / BS) blocks, the
// last one padded), and k_head, which transforms cluster r's points anyway, walks them in slot order and reduces
// each block's box from the transformed coordinates it has just computed.  One workgroup per cluster; all segments
// of a level are split by ONE bitonic sort over the cluster's slots with key = (first block of the slot's segment,
// coordinate, index): segments hold exactly BS * blocks slots, so after the sort each one sits in its own slot range
// again, ordered on the level's axis, and is halved at a block boundary (padding sorts last inside its segment and
// so stays in the cluster's last block).  psl4[slot] = (local xyz, bits(point index)), padding = index INT_MAX;
// sb[c] = first block of cluster c, sb[K] = blocks in use.
__global__ __launch_bounds__(512) void k_sort_p(Dims D, Ws W0, size_t bstride) {
    const Ws W = ws_shift(W0, blockIdx.z * bstride);
    extern __shared__ __attribute__((aligned(16))) char smem_raw[];
    unsigned long long* key = (unsigned long long*)smem_raw;
    __shared__ unsigned short sf[PS_MAXB], sm[PS_MAXB];                 // per block of this cluster: its segment's first block, block count
    __shared__ int s_more;
    const int tid = threadIdx.x, c = blockIdx.x;
    const int BS = 64 * D.ppl, bshift = D.ppl == 1 ? 6 : 8;
    int first = 0;                                                       // blocks of the clusters before this one
    for (int i = 0; i < c; ++i) first += (W.off[i + 1] - W.off[i] + BS - 1) >> bshift;
    const int p0 = W.off[c], n = W.off[c + 1] - p0, m = (n + BS - 1) >> bshift;
    if (tid == 0) {
        W.sb[c] = first;
        if (c == D.K - 1) W.sb[D.K] = first + m;
    }
    if (m == 0) return;
    const int ns = m * BS;
    int npow = 64;
    while (npow < ns) npow <<= 1;
    if (npow > YS_CHUNK) {
        // a cluster above 16384 slots does not fit one workgroup's LDS: its blocks keep the points' given order (any
        // permutation gives the same search result -- the boxes are reduced from whatever a block holds -- it only prunes less)
        for (int sl = tid; sl < ns; sl += 512) {
            float4 o = make_float4(0.f, 0.f, 0.f, __int_as_float(0x7fffffff));
            if (sl < n) { const float4 p = W.pts4[p0 + sl]; o = make_float4(p.x, p.y, p.z, __int_as_float(p0 + sl)); }
            W.psl4[(size_t)first * BS + sl] = o;
        }
        return;
    }
    for (int sl = tid; sl < npow; sl += 512) key[sl] = sl >= ns ? ~0ull : sl < n ? (unsigned long long)(p0 + sl) : 0xFFFFull;
    for (int b = tid; b < m; b += 512) { sf[b] = 0; sm[b] = (unsigned short)m; }
    __syncthreads();
    int levels = 0;
    for (int level = 0; level < 9; ++level) {
        if (tid == 0) s_more = 0;
        __syncthreads();
        for (int b = tid; b < m; b += 512) if (sm[b] > 1) s_more = 1;
        __syncthreads();
        if (!s_more) break;
        levels = level + 1;
        const int axis = level % 3;
        for (int sl = tid; sl < ns; sl += 512) {
            const unsigned idx = (unsigned)(key[sl] & 0xFFFFull);
            unsigned u = 0xFFFFFFFFu;
            if (idx != 0xFFFFu) {
                const float4 p = W.pts4[idx];
                u = ordered_bits(axis == 0 ? p.x : axis == 1 ? p.y : p.z);
            }
            key[sl] = ((unsigned long long)sf[sl >> bshift] << 48) | ((unsigned long long)u << 16) | idx;
        }
        __syncthreads();
        bitonic_segments(key, npow, npow, tid, 512);
        unsigned short nf = 0, nm = 0;
        const bool mine = tid < m;
        if (mine) {
            const int f = sf[tid], mm = sm[tid];
            nf = (unsigned short)f; nm = (unsigned short)mm;
            if (mm >= 2) {
                const int ml = mm >> 1;
                if (tid < f + ml) nm = (unsigned short)ml;
                else { nf = (unsigned short)(f + ml); nm = (unsigned short)(mm - ml); }
            }
        }
        __syncthreads();
        if (mine) { sf[tid] = nf; sm[tid] = nm; }
        __syncthreads();
    }
    if (D.rows)            // two more levels inside every 64-slot block: aligned groups of 16 slots are k-d cells (see k_sort_y)
        for (int sub = 0; sub < 2; ++sub) {
            const int axis = (levels + sub) % 3;
            __syncthreads();
            for (int sl = tid; sl < ns; sl += 512) {
                const unsigned idx = (unsigned)(key[sl] & 0xFFFFull);
                unsigned u = 0xFFFFFFFFu;                     // padding sorts last inside its segment
                if (idx != 0xFFFFu) {
                    const float4 p = W.pts4[idx];
                    u = ordered_bits(axis == 0 ? p.x : axis == 1 ? p.y : p.z);
                }
                key[sl] = ((unsigned long long)u << 16) | idx;
            }
            __syncthreads();
            bitonic_segments(key, npow, 64 >> sub, tid, 512);
        }
    for (int sl = tid; sl < ns; sl += 512) {
        const unsigned idx = (unsigned)(key[sl] & 0xFFFFull);
        float4 o = make_float4(0.f, 0.f, 0.f, __int_as_float(0x7fffffff));
        if (idx != 0xFFFFu) { const float4 p = W.pts4[idx]; o = make_float4(p.x, p.y, p.z, __int_as_float((int)idx)); }
        W.psl4[(size_t)first * BS + sl] = o;
    }
}

// ------------------------------------------------------------------------------------------ parameters home, state in / out
// after the last epoch: the parameters of an odd number of optimizer steps sit in the second buffer; the copy-out reads the first
// The parameters change buffer with every optimizer step: after a run that took an odd number of them they sit in P1.  `sidx`: the
// state the run ended in (epochs enqueued & 1), `step0`: the step count it started from (0 unless resumed from a caller's state).
__global__ __launch_bounds__(256) void k_params_home(Dims D, Ws W0, size_t bstride, int sidx, int step0) {
    const Ws W = ws_shift(W0, blockIdx.z * bstride);
    if (((W.state[sidx].step - step0) & 1) == 0) return;
    for (int i = blockIdx.x * 256 + threadIdx.x; i < D.NPAR; i += gridDim.x * 256) W.P[i] = W.P1[i];
}

// creg_train_plan_resume: the caller's optimizer / control state over what k_prep staged (both copies of the double-buffered struct),
// and the state a run ended in as twelve doubles (the layout include/creg.h documents).
struct ResumeState { double lr, sched_best; int step, epochs_run, sched_bad, count, best_epoch, stopped; float min_loss; };
__global__ void k_set_state(Dims D, Ws W, ResumeState rs) {
    if (threadIdx.x || blockIdx.x) return;
    TrainState s = W.state[0];
    s.lr = rs.lr; s.sched_best = rs.sched_best; s.sched_bad = rs.sched_bad; s.count = rs.count; s.stopped = rs.stopped; s.step = rs.step;
    s.min_loss = rs.min_loss; s.epochs_run = rs.epochs_run; s.best_epoch = rs.best_epoch;
    s.next_bc1 = W.bc1[min(rs.step + 1, D.epochs)]; s.next_bc2s = W.bc2s[min(rs.step + 1, D.epochs)];       // (k_prep, the launch before, filled the tables)
    W.state[0] = s; W.state[1] = s;
    W.result[0] = s.min_loss; W.result[1] = (float)s.epochs_run; W.result[2] = (float)s.lr; W.result[3] = (float)s.best_epoch;
}
__global__ void k_get_state(Ws W, int sidx, double* out) {
    if (threadIdx.x || blockIdx.x) return;
    const TrainState s = W.state[sidx];
    out[0] = s.step; out[1] = s.epochs_run; out[2] = s.lr; out[3] = s.sched_best; out[4] = s.sched_bad; out[5] = s.count;
    out[6] = (double)s.min_loss; out[7] = s.best_epoch; out[8] = s.stopped; out[9] = (double)s.last_loss; out[10] = 0.0; out[11] = 0.0;
}

// ------------------------------------------------------------------------------------------ host side
// One launch copies up to 16 (source, destination, dword count) ranges: a problem's 10 parameter tensors + offsets in,
// parameters + results out -- instead of one hipMemcpyAsync (a ~2.5 us blit kernel each) per tensor, 270 per frame round.
__global__ __launch_bounds__(256) void k_copy_table(CopyTable T) {
    const unsigned* __restrict__ s = T.src[blockIdx.y]; unsigned* __restrict__ d = T.dst[blockIdx.y];
    const int n = T.n[blockIdx.y];
    for (int i = blockIdx.x * 256 + threadIdx.x; i < n; i += gridDim.x * 256) d[i] = s[i];
}
void copy_table_launch(CopyTable& T, hipStream_t s) {
    if (T.count) hipLaunchKernelGGL(k_copy_table, dim3(32, T.count), dim3(256), 0, s, T);
    T.count = 0;
}
void copy_table_add(CopyTable& T, const void* src, void* dst, size_t bytes, hipStream_t s) {   // launches when full
    if (T.count == COPY_MAX) copy_table_launch(T, s);
    T.src[T.count] = (const unsigned*)src; T.dst[T.count] = (unsigned*)dst; T.n[T.count] = (int)(bytes / 4); ++T.count;
}

int param_map(const Dims& D, ParamMap* pm) {
    if (D.rot != ROT_DQ) {                 // QRegMLP / RRegMLP / RegMLP: encoder, decoder_1 (two layers), decoder_2 (two layers)
        const ParamMap m[10] = {{D.oW1, D.H * D.IN}, {D.ob1, D.H}, {D.oW2, D.HA * D.H}, {D.ob2, D.HA},
                                {D.oW3A, D.OA * D.HA}, {D.ob3A, D.OA}, {D.oW2 + D.HA * D.H, D.HB * D.H},
                                {D.ob2 + D.HA, D.HB}, {D.oW3B, D.OB * D.HB}, {D.ob3B, D.OB}};
        memcpy(pm, m, sizeof(m));
        return 10;
    }
    const ParamMap m[6] = {{D.oW1, D.H * D.IN}, {D.ob1, D.H}, {D.oW2, D.HB * D.H}, {D.ob2, D.HB}, {D.oW3B, D.OB * D.HB}, {D.ob3B, D.OB}};
    memcpy(pm, m, sizeof(m));
    return 6;
}

// After the problems' inputs are staged: the once-per-train block layouts of the two clouds, all problems in one launch each.
static int ys_sort_npow(const Dims& D) { return pow2_at_least(D.NT < YS_CHUNK ? D.NT : YS_CHUNK); }
static int ys_sort_smem(const Dims& D) {       // keys + [group][6] box scratch of ONE chunk's blocks
    const int per_chunk = YS_CHUNK / (64 * D.ppl);
    return ys_sort_npow(D) * 8 + 6 * 4 * (D.nyb < per_chunk ? D.nyb : per_chunk) * D.ppl;
}
static int ps_sort_smem(const Dims& D) {       // a cluster can hold every point
    const int BS = 64 * D.ppl;
    const int np = pow2_at_least((D.NP + BS - 1) / BS * BS);
    return (np < YS_CHUNK ? np : YS_CHUNK) * 8;
}
// the most either can come to: a full chunk of keys, 256 blocks' boxes behind the target frame's
constexpr int YS_SORT_LDS_MAX = YS_CHUNK * 8 + 6 * 4 * (YS_CHUNK / 64), PS_SORT_LDS_MAX = YS_CHUNK * 8;
// The limit is per kernel, not per plan: always raised to the largest any plan can ask for, so that a small plan created later
// does not lower it under a large one.
int setup_raise_lds(const Dims& D) {
    if (D.npb) CREG_HIP(hipFuncSetAttribute((const void*)k_sort_p, hipFuncAttributeMaxDynamicSharedMemorySize, PS_SORT_LDS_MAX));
    if (D.nyb) CREG_HIP(hipFuncSetAttribute((const void*)k_sort_y, hipFuncAttributeMaxDynamicSharedMemorySize, YS_SORT_LDS_MAX));
    return CREG_OK;
}
void launch_sorts(const Dims& D, const Slice& S, size_t bstride, hipStream_t s, bool keep_target_blocks) {
    // (keep_target_blocks: the launch only verifies the caller's claim -- see k_sort_y)
    if (D.nyb) hipLaunchKernelGGL(k_sort_y, dim3(cdiv(D.NT, YS_CHUNK), 1, S.nz), dim3(1024), ys_sort_smem(D), s, D, S.W, bstride, ys_sort_npow(D), keep_target_blocks ? 1 : 0);
    if (D.npb) hipLaunchKernelGGL(k_sort_p, dim3(D.K, 1, S.nz), dim3(512), ps_sort_smem(D), s, D, S.W, bstride);
}

// Inputs of the slice's problems into their workspaces: the parameter / offset copies of all of them in one launch (per
// COPY_MAX ranges), then one k_prep and one k_l1 launch with the problems in grid.z.  (Null pointers: the entries' argument check.)
int stage_inputs(const Dims& D, const Slice& S, size_t bstride, const creg_train_args* args, hipStream_t s) {
    const int n = S.nz;
    ParamMap pm[10];
    const int np = param_map(D, pm);
    CopyTable T;
    PrepBatch pb;
    for (int b = 0; b < n; ++b) {
        const creg_train_args* a = args + b;
        const Ws W = ws_shift(S.W, (size_t)b * bstride);
        for (int i = 0; i < np; ++i) copy_table_add(T, a->params[i], W.P + pm[i].off, sizeof(float) * pm[i].count, s);
        copy_table_add(T, a->seg_offsets, W.off, sizeof(int) * (D.K + 1), s);
        pb.m[b] = a->m; pb.y[b] = a->y; pb.pts[b] = a->local_pts;
        pb.hy[b] = Hyper{a->lr, a->sched_factor, a->sched_patience, a->stop};
    }
    copy_table_launch(T, s);
    const int mx = D.NP > D.NT ? D.NP : D.NT;
    int blocks = cdiv(mx > D.NPAR ? mx : D.NPAR, 256);
    if (blocks > 2048) blocks = 2048;
    hipLaunchKernelGGL(k_prep, dim3(blocks, 1, n), dim3(256), 0, s, D, S.W, bstride, pb);
    hipLaunchKernelGGL(k_l1, dim3(cdiv(D.H, 4), 1, n), dim3(256), 0, s, D, S.W, 0, bstride);
    launch_l2(D, S, bstride, 0, s);      // the first epoch's hidden activation (later ones: the k_l2 launch that ends every epoch)
    CREG_LAUNCH_CHECK();
    return CREG_OK;
}

void launch_params_home(const Dims& D, const Slice& S, size_t bstride, int sidx, int step0, hipStream_t s) {
    hipLaunchKernelGGL(k_params_home, dim3(64, 1, S.nz), dim3(256), 0, s, D, S.W, bstride, sidx, step0);
}
void launch_set_state(const Dims& D, const Ws& W, const creg_train_state& from, hipStream_t s) {
    const ResumeState rs{from.lr, from.sched_best, from.step, from.epochs_run, from.sched_bad, from.count, from.best_epoch, from.stopped ? 1 : 0, from.min_loss};
    hipLaunchKernelGGL(k_set_state, dim3(1), dim3(64), 0, s, D, W, rs);
}
void launch_get_state(const Ws& W, int sidx, double* out, hipStream_t s) { hipLaunchKernelGGL(k_get_state, dim3(1), dim3(64), 0, s, W, sidx, out); }

}  // namespace creg
