// train_forward.hip -- the train plan's forward launches: k_l2, the hidden activation (the launch that ENDS an epoch, and once
// before the first), and k_head, output layers + pose assembly + the rigid transform of the clusters (the launch that begins one).
#include <cmath>
#include "train_dev.h"

namespace creg {

// ------------------------------------------------------------------------------------------ layer 2
// The hidden activation h2 = act(x1 . W2^T + b2), [K x H] . [H x H2]: once for epoch 0 and at the end of every epoch (the next
// epoch's activation from the freshly updated rows and the next encoder activation).  Round 4: on the matrix cores
// (v_mfma_f32_16x16x4_f32, exact float32: a k-ordered fmaf chain).  A workgroup owns 16 hidden units (one N-tile), its 8 waves split
// the H inputs (wave w: inputs [KW w, KW (w + 1)), KW = H / 8), M-tiles = 16 pose rows, two per pass.  Operands straight from
// global memory, 16 bytes per lane where the width allows (KW % 16 == 0; k order inside a wave o(g, i, kk) = 16 g + 4 kk + i as in
// k_bd's B role): B[k][j] = W2[u0 + j][o], A[i][k] = x1[r][o] (rows past K repeat row K - 1 into accumulator rows nobody reads).
// The eight partial tiles are summed in wave order through LDS, + bias, activation.  (Round 3: 1024-thread workgroups staged all of
// x1 in LDS -- LDS-DMA, a full wait, a barrier -- then every wave ran 20 dependent steps of two ds_read_b128, 8 FMAs and a DPP wave sum.)
constexpr int L2_THREADS = 512;
constexpr int L2_RB = 32;             // pose rows per pass (two M-tiles)
template <int NC>
__device__ __forceinline__ void l2_body(const Dims& D, const Ws& W, int par, int blk) {
    constexpr int KW = 8 * NC, NS = KW / 4;
    constexpr bool V4 = KW % 16 == 0;
    constexpr int NL = V4 ? NS / 4 : NS;           // loads per operand tile and lane
    __shared__ __attribute__((aligned(16))) float red[(L2_THREADS / 64) * L2_RB * 16];
    const float* Pc = par ? W.P1 : W.P;
    const float* x1cur = par ? W.x1[1] : W.x1[0];     // (a runtime index into the shifted struct would go to scratch)
    float* h2out = par ? W.h2[1] : W.h2[0];
    const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6, lj = lane & 15, kk = lane >> 4;
    const int u0 = blk * 16, H = D.H;                // grid covers H2 exactly (H2 % 32 == 0)
    auto load_t = [&](const float* rowp, float* dst) {     // one operand tile of this lane: its wave's KW inputs of row `rowp`
        const float* p = rowp + wv * KW + (V4 ? 4 * kk : kk);
#pragma unroll
        for (int q = 0; q < NL; ++q) {
            if constexpr (V4) { const float4 v = *(const float4*)(p + 16 * q); dst[4 * q] = v.x; dst[4 * q + 1] = v.y; dst[4 * q + 2] = v.z; dst[4 * q + 3] = v.w; }
            else dst[q] = p[4 * q];
        }
    };
    float bw[NS], a0[NS], a1[NS];
    load_t(Pc + D.oW2 + (size_t)(u0 + lj) * H, bw);
    load_t(x1cur + (size_t)min(lj, D.K - 1) * H, a0);
    const bool two0 = D.K > 16;                        // workgroup-uniform
    if (two0) load_t(x1cur + (size_t)min(16 + lj, D.K - 1) * H, a1);
    const float bias = Pc[D.ob2 + u0 + (tid & 15)];
    __builtin_amdgcn_sched_barrier(0);
    const int stopped = W.state[par].stopped;          // requested LAST (hipcc waits for it where it is issued: see k_bd); the state
                                                       //   the epoch that ENDS with this launch has produced
    __builtin_amdgcn_sched_barrier(0);
    for (int r0 = 0; r0 < D.K; r0 += L2_RB) {          // K <= 32: one pass
        const int nr = min(L2_RB, D.K - r0);
        const bool two = nr > 16;
        if (r0) {
            load_t(x1cur + (size_t)min(r0 + lj, D.K - 1) * H, a0);
            if (two) load_t(x1cur + (size_t)min(r0 + 16 + lj, D.K - 1) * H, a1);
        }
        f32x4 acc0 = {0.f, 0.f, 0.f, 0.f}, acc1 = {0.f, 0.f, 0.f, 0.f};
        if (two) {
#pragma unroll
            for (int s = 0; s < NS; ++s) {
                acc0 = __builtin_amdgcn_mfma_f32_16x16x4f32(a0[s], bw[s], acc0, 0, 0, 0);
                acc1 = __builtin_amdgcn_mfma_f32_16x16x4f32(a1[s], bw[s], acc1, 0, 0, 0);
            }
        } else {
#pragma unroll
            for (int s = 0; s < NS; ++s) acc0 = __builtin_amdgcn_mfma_f32_16x16x4f32(a0[s], bw[s], acc0, 0, 0, 0);
        }
        if (r0) __syncthreads();                       // the previous pass has read red
        {   // D[4 kk + v][lj] of tile t -> red[wave][16 t + 4 kk + v][lj]
            float* o = red + (wv * L2_RB + 4 * kk) * 16 + lj;
#pragma unroll
            for (int v = 0; v < 4; ++v) { o[v * 16] = acc0[v]; if (two) o[(16 + v) * 16] = acc1[v]; }
        }
        __syncthreads();
        if (stopped) return;                           // a stopped train keeps its activations (workgroup-uniform)
        if (tid < nr * 16) {                           // tid = (pose row of the pass) * 16 + unit
            float sum = red[tid];
#pragma unroll
            for (int w2 = 1; w2 < L2_THREADS / 64; ++w2) sum += red[w2 * L2_RB * 16 + tid];
            h2out[(size_t)(r0 + (tid >> 4)) * D.H2 + u0 + (tid & 15)] = act_f(sum + bias, D.slope);
        }
    }
}
template <int NC>
__global__ __launch_bounds__(L2_THREADS) void k_l2(Dims D, Ws W0, int par, size_t bstride) {
    // every kernel argument in the entry block, one wait (see k_bd)
    asm volatile("" :: "s"(W0.P), "s"(W0.P1), "s"(W0.x1[0]), "s"(W0.x1[1]), "s"(W0.h2[0]), "s"(W0.h2[1]), "s"(W0.state), "s"(D.K), "s"(D.H),
                 "s"(D.H2), "s"(D.oW2), "s"(D.ob2), "s"(D.slope), "s"(par), "s"(bstride));
    const Ws W = ws_shift(W0, blockIdx.z * bstride);
    l2_body<NC>(D, W, par, blockIdx.x);
}

// ------------------------------------------------------------------------------------------ head + transform
// Block r: output layer for pose row r (one wave per output unit), pose assembly, then the rigid
// transform of cluster r's points (clusters are stored back to back) -- calculate_pc needs no
// launch of its own and nothing is recomputed.
// X: nine output units ('6d': 3 + 6) -- wave 0 takes the ninth as a second dot product.
template <int NC, bool X = false>
__global__ __launch_bounds__(512) void k_head(Dims D, Ws W0, int par, size_t bstride) {
    // every kernel argument in the entry block, one wait (see k_bd)
    asm volatile("" :: "s"(W0.P), "s"(W0.P1), "s"(W0.h2[0]), "s"(W0.h2[1]), "s"(W0.pose_in), "s"(W0.head_save), "s"(W0.m2), "s"(W0.pts4), "s"(W0.pred4),
                 "s"(W0.psl4), "s"(W0.ps4), "s"(W0.pbox), "s"(W0.sb), "s"(W0.cnt4), "s"(W0.state), "s"(W0.off), "s"(D.rot), "s"(D.K), "s"(D.H2), "s"(D.HA),
                 "s"(D.HB), "s"(D.OA), "s"(D.OB), "s"(D.NP), "s"(D.npb), "s"(D.ppl), "s"(D.nbp), "s"(D.oW3A), "s"(D.ob3A), "s"(D.oW3B), "s"(D.ob3B), "s"(par),
                 "s"(bstride));
    const Ws W = ws_shift(W0, blockIdx.z * bstride);
    const float* h2cur = par ? W.h2[1] : W.h2[0];
    const float* Pc = par ? W.P1 : W.P;
    __shared__ float outs[12];
    __shared__ float m2s[12];
    const int r = blockIdx.x, lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int NO = D.OA + D.OB;
    // Request order.  Round 3 issued, in this order, the pose row, the cluster's bounds, its first block, the first point (which needs
    // the block index) and only then the operands of the dot products -- hipcc turned the wave-uniform ones into scalar loads and
    // waited for them one after the other: FOUR dependent memory round trips in front of the dot products' loads.  Now the dot
    // products' operands go out first (every wave: waves past the output units mirror the last one), then everything scalar.
    const int o = min(wave, (X ? 8 : NO) - 1);
    const float *w, *a; int n;
    if (o < D.OA) { w = Pc + D.oW3A + (size_t)o * D.HA; a = h2cur + (size_t)r * D.H2; n = D.HA; }
    else { w = Pc + D.oW3B + (size_t)(o - D.OA) * D.HB; a = h2cur + (size_t)r * D.H2 + D.HA; n = D.HB; }
    float wv[NC], av[NC];                          // n <= 64 NC: every load of the dot in flight at once
#pragma unroll
    for (int c = 0; c < NC; ++c) { const int i = min(c * 64 + lane, n - 1); wv[c] = w[i]; av[c] = a[i]; }
    const float bias = o < D.OA ? Pc[D.ob3A + o] : Pc[D.ob3B + o - D.OA];
    float wv9[NC], av9[NC], bias9 = 0.f;           // X: output unit 8 (branch B's last), every wave requests it, wave 0 uses it
    if constexpr (X) {
        const float* w9 = Pc + D.oW3B + (size_t)(8 - D.OA) * D.HB;
        const float* a9 = h2cur + (size_t)r * D.H2 + D.HA;
#pragma unroll
        for (int c = 0; c < NC; ++c) { const int i = min(c * 64 + lane, D.HB - 1); wv9[c] = w9[i]; av9[c] = a9[i]; }
        bias9 = Pc[D.ob3B + 8 - D.OA];
    }
    __builtin_amdgcn_sched_barrier(0);
    const int stopped = W.state[par].stopped;      // early stop (mlp_reg.py:107-111): the remaining epochs of a captured graph
                                                   // return at their first barrier
    float pin[POSE_IN];
#pragma unroll
    for (int i = 0; i < POSE_IN; ++i) pin[i] = W.pose_in[POSE_IN * r + i];
    const int b = W.off[r], e = W.off[r + 1];
    // block-sorted walk (D.npb): cluster r owns the slots of blocks [sb[r], sb[r + 1])
    const int BS = 64 * D.ppl;
    const int sb0 = W.sb[r], sb1 = W.sb[r + 1];    // (unconditional, so that both come in the batch above: behind `D.npb ? ... : 0` they were two more dependent round trips)
    const int s0 = D.npb ? BS * sb0 : 0, s1 = D.npb ? BS * sb1 : 0;
    const float4 p_first = D.npb ? W.psl4[min(s0 + (int)threadIdx.x, BS * D.npb - 1)] : W.pts4[min(b + (int)threadIdx.x, D.NP - 1)];
    {
        float s = 0.f;
#pragma unroll
        for (int c = 0; c < NC; ++c) s = fmaf(c * 64 + lane < n ? wv[c] : 0.f, av[c], s);
        s = wave_sum_fast(s) + bias;
        if (lane == 0 && wave < NO) outs[o] = s;
        if constexpr (X) {
            float s9 = 0.f;
#pragma unroll
            for (int c = 0; c < NC; ++c) s9 = fmaf(c * 64 + lane < D.HB ? wv9[c] : 0.f, av9[c], s9);
            s9 = wave_sum_fast(s9) + bias9;
            if (lane == 0 && wave == 0) outs[8] = s9;
        }
    }
    __syncthreads();
    if (stopped) return;
    if (threadIdx.x == 0) {
        const float* in = pin;
        float R[9], t[3], save[16];
        for (int i = 0; i < 16; ++i) save[i] = 0.f;
        if (D.rot == ROT_6D) {
            // xyz + orig[:, :3], r6d + orig[:, 3:]  model_utils.py:214 ; rotation_6d_to_matrix  mlp_reg.py:89
            for (int i = 0; i < 3; ++i) t[i] = outs[i] + in[i];
            float d6[6];
            for (int i = 0; i < 6; ++i) { d6[i] = outs[3 + i] + in[3 + i]; save[i] = d6[i]; }
            rot6d_to_matrix(d6, R);
        } else if (D.rot == ROT_RPY) {
            // xyz + orig[:, :3], tanh(.) + orig[:, 3:]  model_utils.py:237-242,274 ; euler_angles_to_matrix(r, "XYZ")  mlp_reg.py:75
            for (int i = 0; i < 3; ++i) t[i] = outs[i] + in[i];
            float e3[3];
            for (int i = 0; i < 3; ++i) { const float th = tanhf(outs[3 + i]); e3[i] = th + in[3 + i]; save[i] = e3[i]; save[4 + i] = th; }
            euler_xyz_to_matrix(e3, R);
        } else if (D.rot == ROT_Q) {
            // xyz + orig[:, :3] ; normalize(q + orig[:, 3:])   model_utils.py:159
            for (int i = 0; i < 3; ++i) t[i] = outs[i] + in[i];
            float v[4], n2 = 0.f;
            for (int i = 0; i < 4; ++i) { v[i] = outs[3 + i] + in[3 + i]; n2 = fmaf(v[i], v[i], n2); }
            const float nrm = sqrtf(n2), den = fmaxf(nrm, 1e-12f);
            float u[4];
            for (int i = 0; i < 4; ++i) u[i] = v[i] / den;
            quat_to_matrix(u, R);
            for (int i = 0; i < 4; ++i) save[i] = u[i];
            save[4] = nrm;
        } else {
            float dq[8];
            for (int i = 0; i < 8; ++i) dq[i] = outs[i] + in[i];              // x + orig  model_utils.py:99
            dq_to_se3(dq, R, t);
            for (int i = 0; i < 8; ++i) save[i] = dq[i];
        }
        for (int a = 0; a < 3; ++a) { m2s[4 * a] = R[3 * a]; m2s[4 * a + 1] = R[3 * a + 1]; m2s[4 * a + 2] = R[3 * a + 2]; m2s[4 * a + 3] = t[a]; }
        for (int i = 0; i < 12; ++i) W.m2[16 * r + i] = m2s[i];
        W.m2[16 * r + 12] = 0.f; W.m2[16 * r + 13] = 0.f; W.m2[16 * r + 14] = 0.f; W.m2[16 * r + 15] = 1.f;
        for (int i = 0; i < 16; ++i) W.head_save[16 * r + i] = save[i];
    }
    __syncthreads();
    if (D.npb) {
        // slot order: a wave covers 64 consecutive slots per trip, so a block's box is a wave reduction of the
        // coordinates just computed (exact: the search compares against these very values); with 256-point blocks
        // the four waves of a block combine through LDS
        __shared__ float wbox[8][6];
        for (int base = s0; base < s1; base += 512) {            // trip count uniform over the workgroup
            const int sl = base + threadIdx.x;
            const bool in = sl < s1;
            const float4 p = !in ? make_float4(0.f, 0.f, 0.f, __int_as_float(0x7fffffff)) : (base == s0 ? p_first : W.psl4[sl]);
            const int n = __float_as_int(p.w);
            const bool real = n != 0x7fffffff;
            float o[3];
#pragma unroll
            for (int a = 0; a < 3; ++a) o[a] = fmaf(p.z, m2s[4 * a + 2], fmaf(p.y, m2s[4 * a + 1], p.x * m2s[4 * a])) + m2s[4 * a + 3];
            if (real) {
                W.pred4[n] = make_float4(o[0], o[1], o[2], 0.f);
                W.cnt4[n] = make_int4(0, 0, 0, 0);
            }
            if (in) W.ps4[sl] = real ? make_float4(o[0], o[1], o[2], p.w) : make_float4(INFINITY, INFINITY, INFINITY, p.w);
            float bx[6];
#pragma unroll
            for (int a = 0; a < 3; ++a) {
                bx[a] = wave_min_fast(real ? o[a] : INFINITY);
                bx[3 + a] = -wave_min_fast(real ? -o[a] : INFINITY);
            }
            if (D.ppl == 1) {
                if (lane == 0 && in) {
                    float* pb = W.pbox + (sl >> 6);            // six planes of 64 nbp boxes
#pragma unroll
                    for (int a = 0; a < 6; ++a) pb[a * 64 * D.nbp] = bx[a];
                }
            } else {                                             // 4 waves per block, 2 blocks per trip
                if (lane == 0) {
#pragma unroll
                    for (int a = 0; a < 6; ++a) wbox[wave][a] = bx[a];
                }
                __syncthreads();
                if (threadIdx.x < 12) {
                    const int hb = threadIdx.x / 6, a = threadIdx.x % 6;
                    if (base + 256 * hb < s1) {
                        float v = wbox[4 * hb][a];
                        for (int w = 1; w < 4; ++w) v = a < 3 ? fminf(v, wbox[4 * hb + w][a]) : fmaxf(v, wbox[4 * hb + w][a]);
                        W.pbox[a * 64 * D.nbp + (base >> 8) + hb] = v;
                    }
                }
                __syncthreads();
            }
        }
        return;
    }
    for (int n = b + threadIdx.x; n < e; n += 512) {
        const float4 p = (n == b + (int)threadIdx.x) ? p_first : W.pts4[n];
        float o[3];
#pragma unroll
        for (int a = 0; a < 3; ++a) o[a] = fmaf(p.z, m2s[4 * a + 2], fmaf(p.y, m2s[4 * a + 1], p.x * m2s[4 * a])) + m2s[4 * a + 3];
        W.pred4[n] = make_float4(o[0], o[1], o[2], 0.f);
        W.cnt4[n] = make_int4(0, 0, 0, 0);
    }
}

// ------------------------------------------------------------------------------------------ host side
void launch_l2(const Dims& D, const Slice& S, size_t bstride, int par, hipStream_t s) {
    by_nc(D.H, [&](auto nc) {
        hipLaunchKernelGGL((k_l2<decltype(nc)::value>), dim3(D.H2 / 16, 1, S.nz), dim3(L2_THREADS), 0, s, D, S.W, par, bstride); });
}
void launch_head(const Dims& D, const Slice& S, size_t bstride, int par, hipStream_t s) {
    by_nc(D.H, [&](auto nc) {
        if (D.OA + D.OB > 8) hipLaunchKernelGGL((k_head<decltype(nc)::value, true>), dim3(D.K, 1, S.nz), dim3(512), 0, s, D, S.W, par, bstride);
        else hipLaunchKernelGGL((k_head<decltype(nc)::value>), dim3(D.K, 1, S.nz), dim3(512), 0, s, D, S.W, par, bstride);
    });
}

}  // namespace creg
