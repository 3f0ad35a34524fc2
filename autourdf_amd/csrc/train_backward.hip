// train_backward.hip -- the train plan's backward launches: k_gradc (loss, control state, the clusters' pose gradients back through
// the output layers) and k_bd (backward to the encoder side by side with the hidden / output rows' weight gradients, Adam merged
// into both), and the phase stamps of k_bd's measurement build.
#include <cmath>
#include <cstddef>
#include <cstring>
#include "train_dev.h"

namespace creg {

// ------------------------------------------------------------------------------------------ control + cluster grads
// K blocks.  Every block derives the same loss and the same decisions from the same inputs; block 0
// advances the double-buffered state.  Then block k reduces cluster k's point gradients to
// [dL/dR | dL/dt] in a fixed order and thread 0 pulls them back through the pose head.
// bc1 / bc2_sqrt: the bias corrections of step S.step + 1 (k_prep's table)
__device__ __forceinline__ TrainState advance_state(const TrainState& S, float loss, const Hyper& hy, double bc1, float bc2_sqrt) {
    TrainState N = S;
    const bool improved = loss < S.min_loss;
    N.last_loss = loss;
    N.epochs_run = S.epochs_run + 1;
    // (selects of values, not conditional stores into N: hipcc turned those into ONE store through a computed address into a stack
    //  copy of the struct -- 16 bytes of scratch per lane and a scratch round trip in the middle of the kernel)
    const int count = improved ? 0 : S.count + 1;
    N.min_loss = improved ? loss : S.min_loss;
    N.best_epoch = improved ? S.epochs_run : S.best_epoch;
    N.count = count;
    N.stopped = (!improved && count > hy.stop) ? 1 : S.stopped;                      // mlp_reg.py:107-111
    if (!N.stopped) {
        // optimizer.step() of this epoch uses S.lr (torch.optim.Adam, betas (0.9, 0.999), eps 1e-8)
        N.step = S.step + 1;
        N.step_size = (float)(S.lr / bc1);
        N.bc2_sqrt = bc2_sqrt;
        // scheduler.step(loss): ReduceLROnPlateau(mode='min', threshold 1e-4 rel, cooldown 0, min_lr 0, eps 1e-8)
        const double cur = (double)loss;
        if (cur < S.sched_best * (1.0 - 1e-4)) { N.sched_best = cur; N.sched_bad = 0; }
        else N.sched_bad = S.sched_bad + 1;
        if (N.sched_bad > hy.patience) {
            const double nl = fmax(S.lr * (double)hy.factor, 0.0);
            if (S.lr - nl > 1e-8) N.lr = nl;
            N.sched_bad = 0;
        }
    }
    return N;
}

constexpr int GC_QMAX = 3;             // hidden units per thread of k_gradc's last phase: H2 <= 768 = 3 x 256
__device__ __forceinline__ void gradc_role(const Dims& D, const Ws& W, int epoch, int nbx, int nby, int k) {
    __shared__ float red[4][14];
    __shared__ float s_loss;
    __shared__ float s_go[16];
    const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
    // ONE round trip for everything that does not depend on another load: the state (with the bias corrections of the
    // coming step), the cluster bounds, the hyper-parameters, the NN launch's loss partials, the pose row, and the
    // operands of the last phase (this thread's hidden units of pose row k and their output-layer weights) -- round 2
    // waited for the state first (the early exit of a stopped train) and then for the table entries it indexes
    const TrainState S = W.state[epoch & 1];
    const int b0 = W.off[k], e0 = W.off[k + 1];
    const Hyper hy = *W.hyper;
    float a = tid < nbx ? W.lossp_x[tid] : 0.f, b = tid < nby ? W.lossp_y[tid] : 0.f;
    const float m2v = W.m2[16 * k + (tid & 15)];
    float sv[16];
#pragma unroll
    for (int i = 0; i < 16; ++i) sv[i] = W.head_save[16 * k + i];
    const float* h2cur = (epoch & 1) ? W.h2[1] : W.h2[0];
    float w3v[GC_QMAX][8], h2v[GC_QMAX];
#pragma unroll
    for (int q = 0; q < GC_QMAX; ++q) {
        const int o = min(q * 256 + tid, D.H2 - 1);
        const bool isA = o < D.HA;
        const float* Pc = (epoch & 1) ? W.P1 : W.P;
        const float* wb = isA ? Pc + D.oW3A + o : Pc + D.oW3B + (o - D.HA);
        const int stride = isA ? D.HA : D.HB, nj = isA ? D.OA : D.OB;
#pragma unroll
        for (int j = 0; j < 8; ++j) w3v[q][j] = wb[(size_t)min(j, nj - 1) * stride];
        h2v[q] = h2cur[(size_t)k * D.H2 + o];
    }
    // hipcc sinks a load into the block that uses it -- here past the early exit below, i.e. BEHIND the state's round trip: a use it
    // cannot move keeps the whole batch above in one round trip with the state
    asm volatile("" :: "v"(a), "v"(b), "v"(m2v), "v"(sv[0]), "v"(sv[1]), "v"(sv[2]), "v"(sv[3]), "v"(sv[4]), "v"(sv[5]), "v"(sv[6]), "v"(sv[7]),
                 "v"(sv[8]), "v"(sv[9]), "v"(sv[10]), "v"(sv[11]), "v"(sv[12]), "v"(sv[13]), "v"(sv[14]), "v"(sv[15]), "v"(b0), "v"(e0), "v"(hy.lr));
#pragma unroll
    for (int q = 0; q < GC_QMAX; ++q)
        asm volatile("" :: "v"(h2v[q]), "v"(w3v[q][0]), "v"(w3v[q][1]), "v"(w3v[q][2]), "v"(w3v[q][3]), "v"(w3v[q][4]), "v"(w3v[q][5]), "v"(w3v[q][6]),
                     "v"(w3v[q][7]));
    if (S.stopped) {
        if (k == 0 && tid == 0) {
            TrainState E = S; E.stopped = 1;
            W.state[(epoch + 1) & 1] = E;
        }
        return;
    }
    // second round trip: this thread's first point of the cluster (the loss reduction runs in its shadow)
    const int n_first = min(b0 + tid, D.NP - 1);
    const float4 p_first = W.pts4[n_first];
    const int4 c_first = W.cnt4[n_first];
    const int s_first = W.sgn_x[n_first];
    const float4 pr_first = W.pred4[n_first];
    // ---- loss = sum_x / NP + sum_y / NT from the NN launch's per-block partials (fixed order)
    for (int i = tid + 256; i < nbx; i += 256) a += W.lossp_x[i];
    for (int i = tid + 256; i < nby; i += 256) b += W.lossp_y[i];
    a = wave_sum_fast(a); b = wave_sum_fast(b);
    if (lane == 0) { red[wv][0] = a; red[wv][1] = b; }
    __syncthreads();
    if (tid == 0) {
        const float sa = ((red[0][0] + red[1][0]) + red[2][0]) + red[3][0];
        const float sb = ((red[0][1] + red[1][1]) + red[2][1]) + red[3][1];
        s_loss = sa / (float)D.NP + sb / (float)D.NT;
    }
    __syncthreads();
    const float loss = s_loss;
    TrainState N = advance_state(S, loss, hy, S.next_bc1, S.next_bc2s);
    const bool improved = loss < S.min_loss;
    if (improved) {                                     // best_pcd / best_m  (mlp_reg.py:102-106)
        for (int n = b0 + tid; n < e0; n += 256) {
            const float4 p = (n == b0 + tid) ? pr_first : W.pred4[n];
            W.best_pred[3 * (size_t)n] = p.x; W.best_pred[3 * (size_t)n + 1] = p.y; W.best_pred[3 * (size_t)n + 2] = p.z;
        }
        if (tid < 16) W.best_m[16 * k + tid] = m2v;
    }
    if (k == 0 && tid == 0) {
        N.next_bc1 = W.bc1[min(N.step + 1, D.epochs)];          // for the next epoch (another launch): off this one's critical path
        N.next_bc2s = W.bc2s[min(N.step + 1, D.epochs)];
        W.state[(epoch + 1) & 1] = N;
        W.loss_hist[S.epochs_run] = loss;
        W.lr_hist[S.epochs_run] = (float)S.lr;
        W.result[0] = N.min_loss; W.result[1] = (float)N.epochs_run; W.result[2] = (float)N.lr; W.result[3] = (float)N.best_epoch;
    }
    if (N.stopped) return;                              // the reference breaks before backward()
    // ---- per-cluster reduction of the point gradients
    const float gx = 1.0f / (float)D.NP, gy = 1.0f / (float)D.NT;
    float acc[12];
#pragma unroll
    for (int i = 0; i < 12; ++i) acc[i] = 0.f;
    for (int n = b0 + tid; n < e0; n += 256) {
        const bool first = n == b0 + tid;
        const float4 p = first ? p_first : W.pts4[n];
        const int4 c = first ? c_first : W.cnt4[n];
        const int sb = first ? s_first : W.sgn_x[n];
        const float g[3] = {((sb & 1) ? gx : -gx) + gy * (float)c.x, ((sb & 2) ? gx : -gx) + gy * (float)c.y,
                            ((sb & 4) ? gx : -gx) + gy * (float)c.z};
#pragma unroll
        for (int q = 0; q < 3; ++q) {
            acc[4 * q] = fmaf(g[q], p.x, acc[4 * q]); acc[4 * q + 1] = fmaf(g[q], p.y, acc[4 * q + 1]);
            acc[4 * q + 2] = fmaf(g[q], p.z, acc[4 * q + 2]); acc[4 * q + 3] += g[q];
        }
    }
    __syncthreads();
#pragma unroll
    for (int i = 0; i < 12; ++i) { const float r = wave_sum_fast(acc[i]); if (lane == 0) red[wv][i] = r; }
    __syncthreads();
    if (tid == 0) {
        float G12[12];
        for (int i = 0; i < 12; ++i) G12[i] = ((red[0][i] + red[1][i]) + red[2][i]) + red[3][i];
        for (int i = 0; i < 16; ++i) W.gm2[16 * k + i] = i < 12 ? G12[i] : 0.f;
        const float G[9] = {G12[0], G12[1], G12[2], G12[4], G12[5], G12[6], G12[8], G12[9], G12[10]};
        const float gt[3] = {G12[3], G12[7], G12[11]};
        float go[16];                          // [0..2] branch A, [4..11] branch B
        for (int i = 0; i < 16; ++i) go[i] = 0.f;
        if (D.rot == ROT_6D) {
            go[0] = gt[0]; go[1] = gt[1]; go[2] = gt[2];
            rot6d_to_matrix_vjp(sv, G, go + 4);
        } else if (D.rot == ROT_RPY) {
            go[0] = gt[0]; go[1] = gt[1]; go[2] = gt[2];
            float ge[3];
            euler_xyz_to_matrix_vjp(sv, G, ge);
            for (int i = 0; i < 3; ++i) go[4 + i] = ge[i] * (1.f - sv[4 + i] * sv[4 + i]);      // through the Tanh that ends decoder_2
        } else if (D.rot == ROT_Q) {
            go[0] = gt[0]; go[1] = gt[1]; go[2] = gt[2];
            float gu[4];
            quat_to_matrix_vjp(sv, G, gu);
            const float nrm = sv[4];
            if (nrm > 1e-12f) {
                const float dot = sv[0] * gu[0] + sv[1] * gu[1] + sv[2] * gu[2] + sv[3] * gu[3];
#pragma unroll
                for (int i = 0; i < 4; ++i) go[4 + i] = (gu[i] - sv[i] * dot) / nrm;
            } else {
#pragma unroll
                for (int i = 0; i < 4; ++i) go[4 + i] = gu[i] / 1e-12f;
            }
        } else {
            float gdq[8];
            dq_to_se3_vjp(sv, G, gt, gdq);
            for (int i = 0; i < 8; ++i) go[4 + i] = gdq[i];
        }
        for (int i = 0; i < 12; ++i) { W.g_out[16 * k + i] = go[i]; s_go[i] = go[i]; }
    }
    __syncthreads();
    // ---- pose row k of dL/d(hidden pre-activation): g_h2[k][o] = act'(h2[k][o]) * sum_j g_out[k][j] W3[j][o]
    // (a row needs only its own g_out, so it is final here: both roles of k_bd read the finished matrix)
#pragma unroll
    for (int q = 0; q < GC_QMAX; ++q) {
        const int o = q * 256 + tid;
        if (o < D.H2) {
            const bool isA = o < D.HA;
            const int nj = isA ? D.OA : D.OB, gofs = isA ? 0 : 4;
            float sum = 0.f;
#pragma unroll
            for (int j = 0; j < 8; ++j) if (j < nj) sum = fmaf(s_go[gofs + j], w3v[q][j], sum);
            W.g_h2[(size_t)k * D.H2 + o] = sum * act_grad(h2v[q], D.slope);
        }
    }
}

__global__ __launch_bounds__(256) void k_gradc(Dims D, Ws W0, int epoch, int nbx, int nby, size_t bstride) {
    // every kernel argument in the entry block, one wait (see k_bd)
    asm volatile("" :: "s"(W0.P), "s"(W0.P1), "s"(W0.h2[0]), "s"(W0.h2[1]), "s"(W0.head_save), "s"(W0.m2), "s"(W0.gm2), "s"(W0.pts4), "s"(W0.pred4),
                 "s"(W0.sgn_x), "s"(W0.cnt4), "s"(W0.lossp_x), "s"(W0.lossp_y), "s"(W0.g_out), "s"(W0.g_h2), "s"(W0.state), "s"(W0.bc1), "s"(W0.bc2s),
                 "s"(W0.best_m), "s"(W0.best_pred), "s"(W0.loss_hist), "s"(W0.lr_hist), "s"(W0.result), "s"(W0.off), "s"(W0.hyper),
                 "s"(D.rot), "s"(D.K), "s"(D.H2), "s"(D.HA), "s"(D.HB), "s"(D.OA), "s"(D.OB), "s"(D.NP), "s"(D.NT), "s"(D.epochs), "s"(D.slope),
                 "s"(D.oW3A), "s"(D.oW3B), "s"(epoch), "s"(nbx), "s"(nby), "s"(bstride));
    const Ws W = ws_shift(W0, blockIdx.z * bstride);
    gradc_role(D, W, epoch, nbx, nby, blockIdx.x);
}

// ------------------------------------------------------------------------------------------ Adam
__device__ __forceinline__ float adam_value(float p, float& mm, float& vv, float g, float step_size, float bc2_sqrt) {
    // torch single-tensor Adam: exp_avg.lerp_(g, 1-b1); exp_avg_sq.mul_(b2).addcmul_(g, g, 1-b2);
    // denom = sqrt(v)/sqrt(bc2) + eps; p.addcdiv_(exp_avg, denom, value=-step_size)
    const float b1w = (float)(1.0 - 0.9), b2 = 0.999f, b2w = (float)(1.0 - 0.999);
    mm = mm + b1w * (g - mm);
    vv = vv * b2 + (b2w * g) * g;
    const float denom = sqrtf(vv) / bc2_sqrt + 1e-8f;
    return p + (-step_size * mm) / denom;
}

// ------------------------------------------------------------------------------------------ backward to x1 + encoder update
// g_x1 = act'(x1) * (g_h2 . W2), COMPLETE per column block: a workgroup owns B2_CB = 16 hidden units of the encoder,
// i.e. 16 columns of W2 over all H2 rows, so nothing is left to reduce across workgroups (round 2 wrote 16 partial slabs
// of g_x1 -- 0.65 MB per problem -- that k_dw's encoder blocks gathered with 4-byte loads, every 128-byte line fetched by
// four workgroups on different XCDs: the 1.6x read amplification of that kernel).  The same workgroup then owns the 16
// encoder rows W1[c0 .. c0+16): weight gradients, Adam, and the NEXT epoch's encoder activation of its 16 units from the
// registers that hold the updated rows (the MLP input is the same every epoch: m.clone() of the same m, mlp_reg.py:62).
// Threads: 8 column pairs x (8 AW) row slices of W2; a thread keeps its OPS rows of its two columns in registers (all
// loads in flight at once, 64-byte row segments), g_h2 comes from LDS (LDS-DMA, RB pose rows per pass, broadcast reads);
// the slice partials of a (pose row, column) are summed in a fixed tree: the 8 slices of a wave (row_ror DPP, two lane
// permutes), then the waves in order through LDS.  The rows of a pass are straight-line code (rows past the end repeat the
// last one and are not stored): per-row branches kept hipcc from overlapping the rows' LDS reads and lane permutes.
#ifdef CREG_BD_STAMPS
// Measurement build (tests/measure/bd_stamps.py): where the two roles of k_bd spend a launch.  Thread 0 of every workgroup reads the
// 100 MHz wall clock at its phase boundaries; per launch slot (epoch & 255) the earliest start and the latest end of each role, per
// role the summed phase durations and workgroup counts.  Recorded only while the host has armed it (the back-to-back leg of
// creg_train_plan_profile).
struct BdStamps {
    unsigned long long first[256], endB[256], endD[256], startB[256], startD[256];
    unsigned long long phase[2][8], blocks[2];
    int armed;
};
__device__ BdStamps g_bd_st;
#endif
constexpr int BD_THREADS = 512;       // workgroups of the backward launch k_bd (both roles)
constexpr int B2_THREADS = BD_THREADS;
constexpr int B2_WAVES = B2_THREADS / 64;
constexpr int B2_CB = 16;             // columns of W2 (= hidden units of the encoder) per workgroup: ONE 16-wide MFMA tile
constexpr int B2_RB = 32;             // pose rows per pass: two 16-row MFMA tiles (K <= 32: one pass)
__host__ __device__ inline int b2_smem_floats(int K, int IN, int H2) {
    // the per-wave partial tiles [8][32][16], the features [K][IN], g_x1 [K][16] and the next-activation tile [K][16] of this block's
    // columns, the block's slab of W2 [H2][16]
    return B2_WAVES * B2_RB * B2_CB + K * IN + 2 * K * B2_CB + H2 * B2_CB;
}
// sum over the 16 lanes of a DPP row; every lane of the row receives it
__device__ __forceinline__ float row_sum16(float v) {
    CREG_DPP_STEP(v, 0xB1, 0xF);    // quad_perm [1,0,3,2]
    CREG_DPP_STEP(v, 0x4E, 0xF);    // quad_perm [2,3,0,1]
    CREG_DPP_STEP(v, 0x141, 0xF);   // row_half_mirror
    CREG_DPP_STEP(v, 0x140, 0xF);   // row_mirror
    return v;
}

// Round 4: the product g_h2 . W2 of a block is a [K x H2] . [H2 x 16] GEMM and runs on the matrix cores as
// v_mfma_f32_16x16x4_f32 tiles -- exact float32, bit for bit a k-ordered fmaf chain (cdna_hip_programming.md section 3), so the
// plan stays deterministic and bit-reproducible; only the association of the sum over the hidden rows differs from round 3's
// (8 lane slices x 8 waves then, 8 waves x one in-order chain of H2 / 8 rows now).  Tiles: M = 16 pose rows (K = 20: two tiles, the
// second one mostly padding -- rows past K repeat row K - 1 and land in accumulator rows nobody reads), N = the block's 16 columns,
// contraction over the hidden rows o: wave w owns rows [w KW, (w + 1) KW), KW / 4 k-steps.  MFMA operand layout: lane l holds
// A[i = l & 15][k = l >> 4] and B[k = l >> 4][j = l & 15]; D[i = 4 (l >> 4) + v][j = l & 15] in accumulator register v.
//   B operand = W2[o][c0 + j]: the block's slab W2[:, c0 .. c0 + 16) goes to LDS by LDS-DMA, 16 bytes per lane (a wave-instruction
//     moves 16 rows of 64 bytes), each wave staging exactly the rows it multiplies -- so its own vmcnt wait is all the
//     synchronisation the slab needs -- and is read back one dword per lane and k-step.  (First build: one global dword load per
//     lane and k-step.  A CU's address path takes ~16 cycles per wave-instruction whatever its width, so those 24 quarter-width
//     loads per lane cost 3 000 cycles per workgroup: the block spent 2.5 us just ISSUING its loads.)
//   A operand = g_h2[r][o]: straight from global memory too (k_gradc wrote it a launch earlier) -- with the rows of a wave ordered
//     o(g, i, kk) = 16 g + 4 kk + i (k-step 4 g + i, k index kk: any bijection works as long as A and B agree) a lane's operands of
//     four consecutive k-steps are ONE 16-byte load g_h2[r][16 g + 4 kk .. + 3] (KW % 16 == 0: hidden 256 / 512); narrower shapes
//     load a dword per k-step with o(s, kk) = 4 s + kk.
// Nothing of the GEMM is staged in LDS any more (round 3 staged all of g_h2, 61 KB per workgroup, and waited for ALL of it before the
// first FMA): every load is in flight at once and the MFMAs start on the first operands that land.  The per-wave partial tiles are
// summed over the waves in wave order through LDS as before.  Then, unchanged: activation gradient, the 16 encoder rows' weight
// gradients + Adam, and the NEXT epoch's encoder activation of the block's 16 units from the registers that hold the updated rows.
template <int KW, bool X>              // W2 rows per wave: H2 = 8 KW; X: more than 64 input features ('6d': 72) -- lanes i4 < 2 of a row take a second float4
__device__ __forceinline__ void bwd2_role(const Dims& D, const Ws& W, int epoch, int blk, float* sh, unsigned long long bd_entry) {
    constexpr int NS = KW / 4;                 // k-steps of a wave
    constexpr bool V4 = KW % 16 == 0;          // A operand as 16-byte loads
    constexpr int NA = V4 ? NS / 4 : NS;       // A loads per tile and lane
    float* red = sh;                                   // [8][32][16] per-wave partial tiles of the pass
    float* encs = red + B2_WAVES * B2_RB * B2_CB;      // [K][IN] MLP input features
    float* gxs = encs + D.K * D.IN;                    // [K][16] g_x1 of this block's columns,
    float* xt = gxs + D.K * B2_CB;                     // [K][16] next encoder activation of this block's units
    float* w2s = xt + D.K * B2_CB;                     // [H2][16] the block's slab of W2 (16-byte aligned: every size above is a multiple of 4 floats)
    // (no early exit on `stopped` before the loads are issued: every store below is gated; an exit branch here would let hipcc
    //  sink the loads below it and serialise them)
    const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6, lj = lane & 15, kk = lane >> 4;
    // The two roles are one function to hipcc: its wait-count pass lets the OTHER role's requests count as possibly pending here and
    // put a vmcnt(0) in the middle of this role's own requests (before the first redefinition of a register the other role loads
    // into).  A wait it can see -- free at run time: nothing is outstanding when a role starts -- clears that state.
    __builtin_amdgcn_s_waitcnt(0x0F70);                // vmcnt(0)
    const int c0 = blk * B2_CB, par = epoch & 1;
    const float* x1cur = par ? W.x1[1] : W.x1[0];     // (a runtime index into the shifted struct would go to scratch)
    float* x1next = par ? W.x1[0] : W.x1[1];
    const float* Pc = par ? W.P1 : W.P;               // this epoch's parameters; the updated rows go to the other buffer
    float* Pn = par ? W.P : W.P1;
    BD_T0
    // every load of the first pass is requested before the first wait
    {   // this wave's KW rows of the slab: lane l moves the 16 bytes W2[row 16 i + (l >> 2)][c0 + 4 (l & 3) ..] to slab row-major
        const float* src = Pc + D.oW2 + (size_t)(wv * KW + (lane >> 2)) * D.H + c0 + 4 * (lane & 3);
        float* dst = w2s + wv * KW * B2_CB;
#pragma unroll
        for (int i = 0; i < KW; i += 16)
            if (i + (lane >> 2) < KW)                  // (KW = 8, 12, 24: the last instruction is partial; inactive lanes write nothing)
                __builtin_amdgcn_global_load_lds((const __attribute__((address_space(1))) void*)(src + (size_t)i * D.H),
                                                 (__attribute__((address_space(3))) void*)(dst + i * B2_CB), 16, 0, 0);
    }
    const float* gbase = W.g_h2 + wv * KW + (V4 ? 4 * kk : kk);        // + row * H2 (+ 16 g | 4 s)
    auto load_a = [&](int row, float* dst) {                           // one tile's A operands of this lane: pose row `row` (clamped)
        const float* g = gbase + (size_t)min(row, D.K - 1) * D.H2;
#pragma unroll
        for (int q = 0; q < NA; ++q) {
            if constexpr (V4) { const float4 v = *(const float4*)(g + 16 * q); dst[4 * q] = v.x; dst[4 * q + 1] = v.y; dst[4 * q + 2] = v.z; dst[4 * q + 3] = v.w; }
            else dst[q] = g[4 * q];
        }
    };
    float a0[NS], a1[NS];
    const bool two0 = D.K > 16;                        // workgroup-uniform
    load_a(lj, a0);
    if (two0) load_a(16 + lj, a1);
    // encoder rows: thread = (half, row of the block, float4 of its IN inputs); both halves hold the row (same operands,
    // same Adam result) and share the pose rows of the next-activation loop
    const int half = tid >> 8, t2 = tid & 255, row = t2 >> 4, i4 = t2 & 15, hu = c0 + row;
    const bool ain = 4 * i4 < D.IN;
    const int ei = min(4 * i4, D.IN - 4);
    const size_t wi = (size_t)D.oW1 + (size_t)hu * D.IN + ei;
    float4 pw = *(const float4*)(Pc + wi), pm = *(const float4*)(W.AM + wi), pv = *(const float4*)(W.AV + wi);
    const bool ain2 = X && 64 + 4 * i4 < D.IN;         // the features past 64
    const int ei2 = min(64 + 4 * i4, D.IN - 4);
    const size_t wi2 = (size_t)D.oW1 + (size_t)hu * D.IN + ei2;
    float4 pw2, pm2, pv2;
    if constexpr (X) { pw2 = *(const float4*)(Pc + wi2); pm2 = *(const float4*)(W.AM + wi2); pv2 = *(const float4*)(W.AV + wi2); }
    float pb = Pc[D.ob1 + hu], mb = W.AM[D.ob1 + hu], vb = W.AV[D.ob1 + hu];
    float xv0 = x1cur[(size_t)min(tid >> 4, D.K - 1) * D.H + c0 + (tid & 15)];      // post-activation of this thread's (pose row, column) output of pass 0
    {   // the features [K][IN] by LDS-DMA, straight-line (at most eight 16-byte pieces per thread: K x IN <= 16384 values; K = 20 needs one) and AFTER the other requests:
        // behind stage_issue's loop hipcc puts a full vmcnt(0) -- in front of everything requested after it
        const int n = D.K * D.IN / 4;
        constexpr int NPC = 8;                         // 16-byte pieces per thread: K * IN / 4 <= 512 NPC (round 4: 5 / 6 pieces, K <= 160; a piece past the end costs one branch)
#pragma unroll
        for (int c = 0; c < NPC; ++c) {
            const int i = c * B2_THREADS + tid;
            if (i < n)
                __builtin_amdgcn_global_load_lds((const __attribute__((address_space(1))) void*)((const float4*)W.enc + i),
                                                 (__attribute__((address_space(3))) void*)((float4*)encs + c * B2_THREADS + (tid & ~63)), 16, 0, 0);
        }
    }
    __builtin_amdgcn_sched_barrier(0);                 // the loads above stay above
    // the state is requested LAST: hipcc makes `stopped` wave-uniform (v_readfirstlane) the moment it can, i.e. it waits for this load
    // right where it is issued -- at the top of the role that put a whole memory round trip in front of every other request
    const TrainState S = W.state[(epoch + 1) & 1];
    const bool live = !S.stopped;
    __builtin_amdgcn_sched_barrier(0);
    BD_T                                               // B1: everything requested
    stage_wait();                                      // this wave's slab rows (and the features, and its A operands) have landed
    float wb[NS];                                      // B operands: this wave's W2 rows, column c0 + lj
#pragma unroll
    for (int s = 0; s < NS; ++s) {
        const int o = V4 ? 16 * (s >> 2) + 4 * kk + (s & 3) : 4 * s + kk;
        wb[s] = w2s[(wv * KW + o) * B2_CB + lj];
    }
    for (int r0 = 0; r0 < D.K; r0 += B2_RB) {          // K <= 32: one pass
        const int nr = min(B2_RB, D.K - r0);
        const bool two = nr > 16;                      // workgroup-uniform
        float xv = xv0;
        if (r0) {
            load_a(r0 + lj, a0);
            if (two) load_a(r0 + 16 + lj, a1);
            xv = x1cur[(size_t)min(r0 + (tid >> 4), D.K - 1) * D.H + c0 + (tid & 15)];
        }
        f32x4 acc0 = {0.f, 0.f, 0.f, 0.f}, acc1 = {0.f, 0.f, 0.f, 0.f};
        if (two) {
#pragma unroll
            for (int s = 0; s < NS; ++s) {
                acc0 = __builtin_amdgcn_mfma_f32_16x16x4f32(a0[s], wb[s], acc0, 0, 0, 0);
                acc1 = __builtin_amdgcn_mfma_f32_16x16x4f32(a1[s], wb[s], acc1, 0, 0, 0);
            }
        } else {
#pragma unroll
            for (int s = 0; s < NS; ++s) acc0 = __builtin_amdgcn_mfma_f32_16x16x4f32(a0[s], wb[s], acc0, 0, 0, 0);
        }
        if (r0) __syncthreads();                       // the previous pass has read red
        {   // D[4 kk + v][lj] of tile t -> red[wave][16 t + 4 kk + v][lj]
            float* o = red + (wv * B2_RB + 4 * kk) * B2_CB + lj;
#pragma unroll
            for (int v = 0; v < 4; ++v) { o[v * B2_CB] = acc0[v]; if (two) o[(16 + v) * B2_CB] = acc1[v]; }
        }
        stage_wait();                                  // (the features' LDS-DMA; every other load has been consumed)
        __syncthreads();
        if (r0 == 0) { BD_T }                          // B2: operands landed, MFMAs, partial tiles in LDS
        if (!live) return;                             // a stopped train: nothing below may be stored (workgroup-uniform)
        if (tid < nr * B2_CB) {                        // tid = (pose row of the pass) * 16 + column
            float sum = red[tid];
#pragma unroll
            for (int w2 = 1; w2 < B2_WAVES; ++w2) sum += red[w2 * B2_RB * B2_CB + tid];
            gxs[r0 * B2_CB + tid] = sum * act_grad(xv, D.slope);
        }
    }
    __syncthreads();
    BD_T                                               // B3: cross-wave reduction, activation gradient, g_x1 into LDS (+ further passes at K > 32)
    // ---- encoder rows: dW1 = g_x1^T enc, Adam, next x1
    float4 ag = make_float4(0.f, 0.f, 0.f, 0.f), ag2 = make_float4(0.f, 0.f, 0.f, 0.f);
    float gsum = 0.f;
    for (int r = 0; r < D.K; ++r) {
        const float g = gxs[r * B2_CB + row];
        const float4 e = *(const float4*)(encs + r * D.IN + ei);
        ag.x = fmaf(g, e.x, ag.x); ag.y = fmaf(g, e.y, ag.y); ag.z = fmaf(g, e.z, ag.z); ag.w = fmaf(g, e.w, ag.w);
        if constexpr (X) {
            const float4 e2 = *(const float4*)(encs + r * D.IN + ei2);
            ag2.x = fmaf(g, e2.x, ag2.x); ag2.y = fmaf(g, e2.y, ag2.y); ag2.z = fmaf(g, e2.z, ag2.z); ag2.w = fmaf(g, e2.w, ag2.w);
        }
        gsum += g;
    }
    float4 nw;
    nw.x = adam_value(pw.x, pm.x, pv.x, ag.x, S.step_size, S.bc2_sqrt);
    nw.y = adam_value(pw.y, pm.y, pv.y, ag.y, S.step_size, S.bc2_sqrt);
    nw.z = adam_value(pw.z, pm.z, pv.z, ag.z, S.step_size, S.bc2_sqrt);
    nw.w = adam_value(pw.w, pm.w, pv.w, ag.w, S.step_size, S.bc2_sqrt);
    float4 nw2 = make_float4(0.f, 0.f, 0.f, 0.f);
    if constexpr (X) {
        nw2.x = adam_value(pw2.x, pm2.x, pv2.x, ag2.x, S.step_size, S.bc2_sqrt);
        nw2.y = adam_value(pw2.y, pm2.y, pv2.y, ag2.y, S.step_size, S.bc2_sqrt);
        nw2.z = adam_value(pw2.z, pm2.z, pv2.z, ag2.z, S.step_size, S.bc2_sqrt);
        nw2.w = adam_value(pw2.w, pm2.w, pv2.w, ag2.w, S.step_size, S.bc2_sqrt);
    }
    pb = adam_value(pb, mb, vb, gsum, S.step_size, S.bc2_sqrt);        // every lane of the row (same operands, same result)
    if (live && half == 0) {
        if (ain) { st4_wt(Pn, wi, nw); st4_wt(W.AM, wi, pm); st4_wt(W.AV, wi, pv); }
        if constexpr (X) if (ain2) { st4_wt(Pn, wi2, nw2); st4_wt(W.AM, wi2, pm2); st4_wt(W.AV, wi2, pv2); }
        if (i4 == 0) { Pn[D.ob1 + hu] = pb; W.AM[D.ob1 + hu] = mb; W.AV[D.ob1 + hu] = vb; }
    }
    BD_T                                               // B4: dW1 over the pose rows, Adam, the encoder rows' stores issued
    for (int r = half; r < D.K; r += 2) {
        const float4 e = *(const float4*)(encs + r * D.IN + ei);
        float v = ain ? fmaf(nw.w, e.w, fmaf(nw.z, e.z, fmaf(nw.y, e.y, nw.x * e.x))) : 0.f;
        if constexpr (X) {
            const float4 e2 = *(const float4*)(encs + r * D.IN + ei2);
            if (ain2) v = fmaf(nw2.w, e2.w, fmaf(nw2.z, e2.z, fmaf(nw2.y, e2.y, fmaf(nw2.x, e2.x, v))));
        }
        v = row_sum16(v) + pb;
        if (i4 == 0) xt[r * B2_CB + row] = act_f(v, D.slope);
    }
    __syncthreads();
    if (live)                                   // the tile goes out as 64-byte row segments, 8 bytes per lane
        for (int t = tid; t < D.K * (B2_CB / 2); t += B2_THREADS) {
            const int r = t >> 3, c2 = 2 * (t & 7);
            *(nn_f2*)(x1next + (size_t)r * D.H + c0 + c2) = nn_f2{xt[r * B2_CB + c2], xt[r * B2_CB + c2 + 1]};
        }
    BD_TEND(0, epoch);                                 // B5: the next activation tile, its stores and the encoder rows' stores acknowledged
}


// ------------------------------------------------------------------------------------------ dW + Adam of the hidden / output rows
// Round 4: the weight gradient of a block of rows, dW[u][i] = sum_r g[r][u] act[r][i], is a [inputs x K] . [K x units] GEMM and runs
// on the matrix cores (v_mfma_f32_16x16x4_f32: exact float32, a k-ordered fmaf chain over the pose rows -- the same order as round 3's
// per-row VALU chain).  A workgroup owns 16 units (parameter rows), wave w their inputs [64 w, 64 w + 64) as four 16 x 16 tiles with
// M = inputs, N = units, contraction over the pose rows r: lane l holds D[i = 4 (l >> 4) + v][j = l & 15], gradients of unit
// u0 + (l & 15) -- the very bytes of the row it loads, updates (Adam, torch's arithmetic) and stores (write-through) as dwordx4 (how
// tiles map to inputs: in the body).  Operands straight from global memory: A = act[r = 4 s + (l >> 4)][..] (the K-row
// activation matrix, 40 KB per problem, L2-resident after the first touch), B[k][j] = g[r][u0 + (l & 15)] (rows K .. KP-1 are zero:
// the contraction is padded to a multiple of 20 rows).  Round 3 staged the whole activation matrix in LDS per workgroup (40 KB LDS-DMA, a wait
// for ALL loads, a barrier) and then ran 20 dependent steps of 2 ds_read_b128 + 8 FMA per wave; now there is no LDS, no barrier, and
// a wave's tiles are consumed in the order their loads were issued, so the stores of its first tiles overlap the loads of its last.
// Blocks of a problem: H2 / 16 hidden blocks, then one for the output rows of decoder_1 (width HA, 'q' only) and one for those of
// decoder_2 / the single decoder (width HB): the same code with fewer than 16 live units.
constexpr int DW_UNITS = 16;          // parameter rows per block (one MFMA N-tile)
constexpr int DW_TILES = 4;           // 16-input tiles per wave: 8 waves x 64 inputs = 512
constexpr int DW_KC = 5;              // k-steps (4 pose rows each) per chunk of operand loads: K = 20 is one chunk
__host__ __device__ inline int dw_blocks(const Dims& D) { return D.H2 / DW_UNITS + 2; }

__device__ __forceinline__ void dw_role(const Dims& D, const Ws& W, int epoch, int blk, unsigned long long bd_entry) {
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6, lj = lane & 15, q = lane >> 4;
    __builtin_amdgcn_s_waitcnt(0x0F70);             // vmcnt(0): see bwd2_role
    const int par = epoch & 1;
    const float* Pc = par ? W.P1 : W.P;             // this epoch's parameters; the updated rows go to the other buffer
    float* Pn = par ? W.P : W.P1;
    // (two selects of values, kept apart: hipcc folds a nested select over the four neighbouring members of the shifted
    //  struct into ONE load with a computed offset -- which puts the whole struct, 40 pointers, into scratch memory)
    const float* x1cur = par ? W.x1[1] : W.x1[0];
    const float* h2cur = par ? W.h2[1] : W.h2[0];
    asm volatile("" : "+s"(x1cur), "+s"(h2cur));
    // block -> (units, width, parameter offsets, activation matrix, gradient matrix); everything block-uniform
    const int nb2 = D.H2 / DW_UNITS;
    int u0, nu, n_in, oW, ob, astride, gstride;
    const float *amat, *gmat;
    if (blk < nb2) { u0 = blk * DW_UNITS; nu = DW_UNITS; n_in = D.H; oW = D.oW2 + u0 * D.H; ob = D.ob2 + u0; amat = x1cur; astride = D.H; gmat = W.g_h2 + u0; gstride = D.H2; }
    else if (blk == nb2) { u0 = 0; nu = D.OA; n_in = D.HA; oW = D.oW3A; ob = D.ob3A; amat = h2cur; astride = D.H2; gmat = W.g_out; gstride = 16; }
    else { u0 = 0; nu = D.OB; n_in = D.HB; oW = D.oW3B; ob = D.ob3B; amat = h2cur + D.HA; astride = D.H2; gmat = W.g_out + 4; gstride = 16; }
    if (nu == 0) return;                            // no decoder_1 ('dq'): block-uniform
    if (64 * wv >= n_in) return;                    // a wave past the row's width (wave-uniform)
    BD_T0
    const int unit = min(lj, nu - 1);               // lanes past the live units mirror the last one and store nothing
    const bool ulive = lj < nu;
    // Every load is a raw buffer load (base in SGPRs, one byte offset per lane and matrix, pose rows as scalar offsets): with 64-bit
    // global addresses the loads of a lane needed so many address pairs that hipcc split them into two batches with a full wait in
    // between.  And every load but the gradients' is 16 bytes wide: a CU's address path takes ~16 cycles per wave-instruction
    // whatever its width (first build: 20 dword loads of the activations per lane -- the workgroup spent 2.2 us ISSUING its loads).
    // Hence the tiles are INTERLEAVED: a lane's A operands of one k-step are ONE float4 of the activation row, component t going to
    // tile t.  Which float4: the accumulator register v of tile t in lane (q, j) is M index 4 q + v of that tile, and it has to be
    // the gradient of input i0 + 16 v + 4 q + t of unit j -- then float4 v = (acc[0][v] .. acc[3][v]) of the lane sits at inputs
    // i0 + 16 v + 4 q .. + 3, and the four lanes q of a unit cover 64 CONTIGUOUS bytes per load / store instruction.  (A lane owning 64
    // consecutive bytes instead -- float4 v at i0 + 16 q + 4 v -- makes every instruction touch 64 different 64-byte segments, 16 bytes
    // of each: the write-through stores then took 7 us instead of 3.6.)  So M index a = 4 q + v loads the float4 at i0 + 16 (a & 3) +
    // 4 (a >> 2): the 16 lanes of a k index read the wave's 256 bytes of the row in a permuted order.
    const int i0 = 64 * wv;                         // this wave's first input
    const int po = (oW + unit * n_in + i0 + 4 * q) * 4;              // byte offset of this lane's float4 0 in the parameter arrays; float4 v is 64 v bytes on
    const __amdgpu_buffer_rsrc_t rP = buf_rsrc(Pc, D.NPAR * 4), rM = buf_rsrc(W.AM, D.NPAR * 4), rV = buf_rsrc(W.AV, D.NPAR * 4);
    // Request order = order of use, because requests return in order: (1) the MFMA operands of the first 20 pose rows, (2) the
    // state, (3) the biases, (4) the parameter / moment float4s v = 0 .. 3.  The MFMAs then run as soon as the few operand bytes
    // are in, and float4 v is updated and STORED while the later ones are still arriving -- the workgroup's write-through stores
    // (48 KB) overlap its loads (first build: parameters first, operands last, every store behind the last load: 2.0 us of loads,
    // then 4.7 us of Adam + stores).
    f32x4 acc[DW_TILES];
#pragma unroll
    for (int t = 0; t < DW_TILES; ++t) acc[t] = f32x4{0.f, 0.f, 0.f, 0.f};
    float gb = 0.f;                                 // this lane's share of the bias gradient: sum over its pose rows r = 4 s + q
    // the contraction runs over KP rows: rows K .. KP-1 of g are zero (k_prep), those of the activations finite (zero) -- no select
    // after a load (it made hipcc wait for every gradient load on the spot) and no clamp
    const __amdgpu_buffer_rsrc_t rA = buf_rsrc(amat, (D.KP * astride - (int)(amat - (blk < nb2 ? x1cur : h2cur))) * 4);
    const __amdgpu_buffer_rsrc_t rG = buf_rsrc(gmat, (D.KP * gstride - (blk < nb2 ? u0 : (blk == nb2 ? 0 : 4))) * 4);
    const int aoff = (q * astride + i0 + 16 * (lj & 3) + 4 * (lj >> 2)) * 4, goff = (q * gstride + unit) * 4;
    float bop[DW_KC];
    float4 aop[DW_KC];
    auto load_ops = [&](int s0) {
#pragma unroll
        for (int s = 0; s < DW_KC; ++s) {
            const int r4 = 4 * (s0 + s);             // scalar: rows r4 + q
            bop[s] = __uint_as_float(__builtin_amdgcn_raw_buffer_load_b32(rG, goff, r4 * gstride * 4, 0));
            aop[s] = ld_buf4(rA, aoff, r4 * astride * 4);   // (inputs past the row's width read the next row or 0: their gradients are not used)
        }
    };
    auto mfma_ops = [&]() {
#pragma unroll
        for (int s = 0; s < DW_KC; ++s) {
            acc[0] = __builtin_amdgcn_mfma_f32_16x16x4f32(aop[s].x, bop[s], acc[0], 0, 0, 0);
            acc[1] = __builtin_amdgcn_mfma_f32_16x16x4f32(aop[s].y, bop[s], acc[1], 0, 0, 0);
            acc[2] = __builtin_amdgcn_mfma_f32_16x16x4f32(aop[s].z, bop[s], acc[2], 0, 0, 0);
            acc[3] = __builtin_amdgcn_mfma_f32_16x16x4f32(aop[s].w, bop[s], acc[3], 0, 0, 0);
        }
#pragma unroll
        for (int s = 0; s < DW_KC; ++s) gb += bop[s];
    };
    load_ops(0);
    __builtin_amdgcn_sched_barrier(0);              // (the scheduler otherwise interleaves requests with the MFMAs and their waits)
    const TrainState S = W.state[(epoch + 1) & 1];
    float pb = Pc[ob + unit], mb = W.AM[ob + unit], vb = W.AV[ob + unit];
    __builtin_amdgcn_sched_barrier(0);
    float4 pw[DW_TILES], pm[DW_TILES], pv[DW_TILES];
    bool vl[DW_TILES];
#pragma unroll
    for (int v = 0; v < DW_TILES; ++v) {
        vl[v] = ulive && i0 + 16 * v + 4 * q < n_in;                 // (HA = 32 at hidden 64: half a wave's inputs exist)
        pw[v] = ld_buf4(rP, po + 64 * v, 0); pm[v] = ld_buf4(rM, po + 64 * v, 0); pv[v] = ld_buf4(rV, po + 64 * v, 0);      // (past the arrays: 0)
        __builtin_amdgcn_sched_barrier(0);
    }
    BD_T                                            // D1: everything requested
    mfma_ops();
    for (int s0 = DW_KC; 4 * s0 < D.KP; s0 += DW_KC) {               // K > 20: further chunks of 20 pose rows (a round trip each)
        load_ops(s0);
        __builtin_amdgcn_sched_barrier(0);
        mfma_ops();
    }
    BD_T                                            // D2: operands landed, MFMAs
    if (S.stopped) return;                          // a stopped train: nothing below may be stored (block-uniform)
#pragma unroll
    for (int v = 0; v < DW_TILES; ++v) {
        float4 nw;
        nw.x = adam_value(pw[v].x, pm[v].x, pv[v].x, acc[0][v], S.step_size, S.bc2_sqrt);
        nw.y = adam_value(pw[v].y, pm[v].y, pv[v].y, acc[1][v], S.step_size, S.bc2_sqrt);
        nw.z = adam_value(pw[v].z, pm[v].z, pv[v].z, acc[2][v], S.step_size, S.bc2_sqrt);
        nw.w = adam_value(pw[v].w, pm[v].w, pv[v].w, acc[3][v], S.step_size, S.bc2_sqrt);
        if (vl[v]) { const int e = po / 4 + 16 * v; st4_wt(Pn, e, nw); st4_wt(W.AM, e, pm[v]); st4_wt(W.AV, e, pv[v]); }
    }
    if (wv == 0) {                                  // the units' biases: gradient = sum over the pose rows of g[r][u], the four lane groups q in order
        float sum = gb;
        sum += __shfl_xor(gb, 16, 64);              // (q, q ^ 1)
        sum += __shfl_xor(sum, 32, 64);             // ((0,1), (2,3))
        pb = adam_value(pb, mb, vb, sum, S.step_size, S.bc2_sqrt);
        if (q == 0 && ulive) { Pn[ob + unit] = pb; W.AM[ob + unit] = mb; W.AV[ob + unit] = vb; }
    }
    BD_TEND(1, epoch);                              // D3: Adam, the write-through stores acknowledged
}

// ------------------------------------------------------------------------------------------ the backward launch: k_bd
// The backward to the encoder (B, H / 16 blocks per problem) and the weight gradients + Adam of the hidden / output rows (D,
// H2 / 8 + 1 blocks per problem) both need only what k_gradc leaves (g_out, g_h2, the advanced state) and this epoch's
// parameters, which nobody overwrites (the updates go to the other parameter buffer): two INDEPENDENT roles, so they are one
// launch of 512-thread workgroups told apart by their block index -- nothing is handed over inside it.  Round 3 first ran them
// as k_bwd2 (11.7 us) -> k_dw (14.9 us, which also computed the next hidden activation from the rows in its registers); side by
// side the launch takes what the longer role takes, and the next hidden activation, the one thing that needs BOTH results (the
// next encoder activation from B, the updated hidden rows from D), is k_l2 again, a launch boundary later.
// grid.x = (H / 16 + H2 / 8 + 1) * problems: the B blocks of ALL problems first (the longer chain of dependent phases).
template <int NC, int KW, bool X = false>
__global__ __launch_bounds__(BD_THREADS, 4) void k_bd(Dims D, Ws W0, int epoch, size_t bstride, int nz) {
    extern __shared__ __attribute__((aligned(16))) char smem[];
#ifdef CREG_BD_STAMPS
    const unsigned long long bd_entry = wall_clock64();
#else
    const unsigned long long bd_entry = 0;
#endif
#ifndef CREG_BD_NO_TOUCH
    // Every kernel argument the roles read, fetched in the ENTRY block with one wait: hipcc otherwise loads arguments where a basic
    // block first needs them -- three dependent scalar round trips to the argument buffer (cold for every node of a replayed graph)
    // before the first request of a role went out.
    asm volatile("" :: "s"(W0.P), "s"(W0.P1), "s"(W0.AM), "s"(W0.AV), "s"(W0.enc), "s"(W0.x1[0]), "s"(W0.x1[1]), "s"(W0.h2[0]), "s"(W0.h2[1]),
                 "s"(W0.g_out), "s"(W0.g_h2), "s"(W0.state), "s"(D.K), "s"(D.KP), "s"(D.IN), "s"(D.H), "s"(D.H2), "s"(D.HA), "s"(D.HB), "s"(D.OA),
                 "s"(D.OB), "s"(D.oW1), "s"(D.ob1), "s"(D.oW2), "s"(D.ob2), "s"(D.oW3A), "s"(D.ob3A), "s"(D.oW3B), "s"(D.ob3B), "s"(D.NPAR),
                 "s"(D.slope), "s"(epoch), "s"(bstride), "s"(nz));
#endif
    const int nB = D.H / B2_CB, nD = dw_blocks(D);
    int i = blockIdx.x;
    const bool roleB = i < nB * nz;
    if (!roleB) i -= nB * nz;
    const int n = roleB ? nB : nD, z = i / n, blk = i - z * n;
    const Ws W = ws_shift(W0, (size_t)z * bstride);
#ifdef CREG_BD_ONLY                                   // measurement build: one role alone (1: backward to the encoder, 2: dW + Adam)
    if ((CREG_BD_ONLY == 1) != roleB) return;
#endif
    if (roleB) bwd2_role<KW, X>(D, W, epoch, blk, (float*)smem, bd_entry);
    else dw_role(D, W, epoch, blk, bd_entry);
}
// ------------------------------------------------------------------------------------------ host side
// What the two launches ask of a shape (make_dims): k_bd's B role stages the [K][IN] features with at most eight 16-byte pieces per
// thread ('6d', 72 features: K <= 227) and keeps them in one CU's LDS beside its slab of W2; whole column blocks; k_gradc's last phase
// takes GC_QMAX hidden units per thread.  '6d' at hidden 512 stops at K = 193: the limit include/creg.h has stated since the plan took
// up to 256 clusters.  The LDS sum alone let 194..227 through (146 to 160 KB of dynamic LDS), shapes past the stated limit that nothing
// has ever run; the stated limit is the one that holds.
constexpr int BD_K_MAX_6D_512 = 193;
constexpr int BD_LDS_MAX = 160 * 1024;         // the dynamic LDS k_bd may ask for (its limit is raised to this: bd_raise_lds)
static int bd_lds_bytes(const Dims& D) { return (int)sizeof(float) * b2_smem_floats(D.K, D.IN, D.H2); }      // the B role's (71 KB at K = 20, hidden 512: its 48 KB slab of W2 + 23 KB; the D role uses none)
bool backward_fits(const Dims& D) {
    if (D.rot == ROT_6D && D.H == 512 && D.K > BD_K_MAX_6D_512) return false;
    return D.K * D.IN / 4 <= 8 * BD_THREADS && bd_lds_bytes(D) <= BD_LDS_MAX && D.H2 % 32 == 0 && D.H % B2_CB == 0 && D.H2 <= 256 * GC_QMAX;
}
void launch_gradc(const Dims& D, const Slice& S, size_t bstride, int epoch, hipStream_t s) {
    hipLaunchKernelGGL(k_gradc, dim3(D.K, 1, S.nz), dim3(256), 0, s, D, S.W, epoch, D.nbx, D.nby, bstride);
}
// the k_bd instance of a shape: NC = H / 64; the B role's 8 waves own KW = H2 / 8 rows of W2 each ('q': H2 = 96 NC, 'dq': 64 NC)
template <typename F>
static void by_bd(const Dims& D, F f) {
    by_nc(D.H, [&](auto nc) {
        constexpr int NC = decltype(nc)::value;
        if (D.IN > 64) f(k_bd<NC, 12 * NC, true>);             // '6d': 72 input features
        else if (D.HA) f(k_bd<NC, 12 * NC>);                   // two decoders ('q', 'rpy'): H2 = H / 2 + H
        else f(k_bd<NC, 8 * NC>);
    });
}
// the dynamic-LDS limit is per kernel AND per device: raised at every plan creation (a process may drive several GPUs; a cached
// "already set" flag would leave the second device at 64 KB)
int bd_raise_lds(const Dims& D) {
    hipError_t e = hipSuccess;
    by_bd(D, [&](auto kern) { e = hipFuncSetAttribute((const void*)kern, hipFuncAttributeMaxDynamicSharedMemorySize, BD_LDS_MAX); });
    if (e != hipSuccess) {
        set_error("creg_train_plan_create: cannot raise the dynamic LDS limit of k_bd: %s", hipGetErrorString(e));
        return CREG_EHIP;
    }
    return CREG_OK;
}
void launch_bd(const Dims& D, const Slice& S, size_t bstride, int epoch, hipStream_t s) {
    const int per = D.H / B2_CB + dw_blocks(D);
    by_bd(D, [&](auto kern) { hipLaunchKernelGGL(kern, dim3(per * S.nz), dim3(BD_THREADS), bd_lds_bytes(D), s, D, S.W, epoch, bstride, S.nz); });
}

// clear and arm (the back-to-back k_bd leg of creg_train_plan_profile) / disarm the stamps
int bd_stamps_arm(bool on) {
#ifdef CREG_BD_STAMPS
    static BdStamps z;                     // (44 KB: not on the stack)
    if (on) {
        memset(&z, 0, sizeof(z)); memset(z.first, 0xff, sizeof(z.first)); memset(z.startB, 0xff, sizeof(z.startB)); memset(z.startD, 0xff, sizeof(z.startD));
        z.armed = 1;
        CREG_HIP(hipMemcpyToSymbol(HIP_SYMBOL(g_bd_st), &z, sizeof(z)));
    } else {
        z.armed = 0;
        CREG_HIP(hipMemcpyToSymbol(HIP_SYMBOL(g_bd_st), &z.armed, sizeof(int), offsetof(BdStamps, armed)));
    }
#endif
    return CREG_OK;
}

}  // namespace creg
using namespace creg;

#ifdef CREG_BD_STAMPS
// out[0..4]: mean launch span, B start, B end, D start, D end relative to the launch's first workgroup (us); out[5], out[6]: B / D
// workgroups per launch; out[8..15] / out[16..23]: mean phase durations of a B / D workgroup (us)
extern "C" int creg_debug_bd_stamps(double* out) {
    BdStamps* z = new BdStamps;
    if (hipMemcpyFromSymbol(z, HIP_SYMBOL(g_bd_st), sizeof(*z)) != hipSuccess) { delete z; return CREG_EHIP; }
    for (int i = 0; i < 24; ++i) out[i] = 0.0;
    int n = 0;
    for (int sl = 0; sl < 256; ++sl) {
        if (z->first[sl] == ~0ull || !z->endB[sl] || !z->endD[sl]) continue;
        ++n;
        const double f = (double)z->first[sl];
        out[0] += ((double)(z->endB[sl] > z->endD[sl] ? z->endB[sl] : z->endD[sl]) - f) / 100.0;
        out[1] += ((double)z->startB[sl] - f) / 100.0; out[2] += ((double)z->endB[sl] - f) / 100.0;
        out[3] += ((double)z->startD[sl] - f) / 100.0; out[4] += ((double)z->endD[sl] - f) / 100.0;
    }
    for (int i = 0; i < 5; ++i) out[i] /= n ? n : 1;
    out[5] = n ? (double)z->blocks[0] / n : 0; out[6] = n ? (double)z->blocks[1] / n : 0; out[7] = n;
    for (int r = 0; r < 2; ++r)
        for (int k = 0; k < 8; ++k) out[8 + 8 * r + k] = z->blocks[r] ? (double)z->phase[r][k] / (double)z->blocks[r] / 100.0 : 0.0;
    delete z;
    return CREG_OK;
}
#endif
