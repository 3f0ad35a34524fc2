// icp_dev.h -- what the ICP translation units share (icp.hip: public entries and the regime switch; icp_small.hip: the
// one-workgroup kernel; icp_large.hip: the many-workgroup regime; kabsch.hip: the closed-form fit alone): the Horn / Jacobi
// solver, the fp64 DPP minimum / maximum, the constants the regime rule needs, the switches of the measurement builds and the
// two regimes' host interface.  This build has no relocatable device code: every unit that includes the solver gets its own
// copy of it, inlined into its kernels.
#pragma once
#include "creg_common.h"
#include "creg_dev.h"

namespace creg {

constexpr int ICP_BATCH_MAX = 16;                     // problems of one creg_masked_icp_batch_f64 call
constexpr int ICP_SRC_LDS = 1024;                     // source points of a cluster kept in LDS (28 B each); the regime rule's cluster size

// ---- the two regimes, as the dispatcher (icp.hip) sees them.  Arguments are checked by the dispatcher; `ws` is the problem's
//      (large) or the batch's (small) share of the caller's workspace.
size_t icp_small_workspace_bytes(int64_t n, int64_t nf, int k);
size_t icp_large_workspace_bytes(int64_t n, int64_t nf, int k);
// one launch of k_masked_icp for the whole batch; problem i uses ws + i * ws_stride
int icp_small_launch(const creg_icp_problem* pr, int batch, int64_t n, int32_t k, int64_t nf, double scale, double th,
                     int32_t max_iteration, int32_t keep_translation, char* ws, size_t ws_stride, hipStream_t s);
// one problem through the many-workgroup launches; `screen`: the float32 screen of k_icp_nn (the CREG_ICP_SCREEN knob)
int icp_large_run(const creg_icp_problem& q, int64_t n, int32_t k, int64_t nf, double scale, double th, int32_t max_iteration,
                  int32_t keep_translation, int screen, char* ws, hipStream_t s);

// ---- measurement builds (CREG_EXTRA_FLAGS=-DCREG_STAMPS / -DCREG_ICP_BLK, tests/measure/README.md): the kernels carry
//      ICP_STAMPED(...) / ICP_BLK(...) statements, which the default build drops before it parses them.
#ifdef CREG_STAMPS
#define ICP_STAMPED(...) __VA_ARGS__
// shader-clock cycles of the phases of every k_masked_icp workgroup, accumulated over its iterations: [workgroup (x + gridDim.x * y)
// % 512][slot]: [0] mask + setup [1] NN scan [2] combine + sums of the means [3] covariance sums [4] Horn on lane 0 [5] move
// [6] iterations [7] targets scanned per wave and iteration (fast path); 8.. = finer split of the NN scan (wave 0's view): [8]
// bounds + range [9] scan [10] rescans [11] wait for the other waves.  k_icp_nn adds its own slots to [0 .. 15] (tail launches
// only).  One copy per translation unit: a run is in one regime, so creg_debug_icp_stamps adds the two copies.
static __device__ unsigned long long g_icp_stamps[512 * 16];
static inline int icp_stamps_add(unsigned long long* out, int reset) {
    static unsigned long long h[512 * 16];
    if (out) { CREG_HIP(hipMemcpyFromSymbol(h, HIP_SYMBOL(g_icp_stamps), sizeof(h))); for (int i = 0; i < 512 * 16; ++i) out[i] += h[i]; }
    if (reset) { static const unsigned long long z[512 * 16] = {}; CREG_HIP(hipMemcpyToSymbol(HIP_SYMBOL(g_icp_stamps), z, sizeof(z))); }
    return CREG_OK;
}
int icp_small_stamps(unsigned long long* out, int reset);
// k_masked_icp: ICP_STAMP_BEGIN() once, then ICP_STAMP(slot) at the end of every phase
#define ICP_STAMP_BEGIN() const int stamp_b = (blockIdx.x + gridDim.x * blockIdx.y) % 512; unsigned long long stamp_t = clock64()
#define ICP_STAMP(slot) do { if (threadIdx.x == 0) { const unsigned long long now_ = clock64(); g_icp_stamps[stamp_b * 16 + slot] += now_ - stamp_t; stamp_t = now_; } } while (0)
// k_icp_nn (reads its `tid`, `tailonly` and `nst`)
#define NN_STAMP(slot) do { const unsigned long long now_ = clock64(); if (tid == 0 && tailonly) atomicAdd(&g_icp_stamps[slot], now_ - nst); nst = now_; } while (0)
#else
#define ICP_STAMPED(...)
#define ICP_STAMP_BEGIN() do { } while (0)
#define ICP_STAMP(slot) do { } while (0)
#define NN_STAMP(slot) do { } while (0)
#endif
#ifdef CREG_ICP_BLK
#define ICP_BLK(...) __VA_ARGS__
#else
#define ICP_BLK(...)
#endif

// 1/x and 1/sqrt(x) from the hardware seeds (v_rcp_f64 / v_rsq_f64, ~2^-23) + two Newton steps (~2^-90
// before rounding): a few ulp, ~6 instructions instead of the ~30 of the IEEE division / sqrt expansions.
// Used only inside the Jacobi rotations (x finite, away from 0 and inf), where a few-ulp angle is as good
// as a correctly rounded one: every rotation is re-orthogonalising by construction.
__device__ __forceinline__ double fast_rcp(double x) {
    double r = __builtin_amdgcn_rcp(x);
    r = fma(fma(-x, r, 1.0), r, r);
    return fma(fma(-x, r, 1.0), r, r);
}
__device__ __forceinline__ double fast_rsqrt(double x) {
    double r = __builtin_amdgcn_rsq(x);
    r = fma(0.5 * r, fma(-x * r, r, 1.0), r);
    return fma(0.5 * r, fma(-x * r, r, 1.0), r);
}

// dominant eigenvector of a symmetric 4x4 (cyclic Jacobi with the usual small-element skip, warm started),
// returned as a unit quaternion.  Runs on one lane: the rotation chain is serial, so it is written for few
// instructions (fast_rcp / fast_rsqrt, skipped negligible rotations, eps-level stopping rule).
// Vp (LDS, in/out): the eigenvector basis of the previous call.  Successive ICP iterations have nearly
// the same profile matrix, so Vp^T N Vp is almost diagonal and one or two sweeps finish the job instead
// of five or six; the first call passes the identity.
__device__ inline void sym4_max_eigvec(const double N[4][4], double q[4], double* Vp) {
    double V[4][4], A[4][4];
    {
        double M[4][4];
#pragma unroll
        for (int i = 0; i < 4; ++i)
#pragma unroll
            for (int j = 0; j < 4; ++j) V[i][j] = Vp[4 * i + j];
#pragma unroll
        for (int i = 0; i < 4; ++i)
#pragma unroll
            for (int j = 0; j < 4; ++j) M[i][j] = fma(N[i][3], V[3][j], fma(N[i][2], V[2][j], fma(N[i][1], V[1][j], N[i][0] * V[0][j])));
#pragma unroll
        for (int i = 0; i < 4; ++i)
#pragma unroll
            for (int j = i; j < 4; ++j) {
                A[i][j] = fma(V[3][i], M[3][j], fma(V[2][i], M[2][j], fma(V[1][i], M[1][j], V[0][i] * M[0][j])));
                A[j][i] = A[i][j];
            }
    }
    for (int sweep = 0; sweep < 60; ++sweep) {
        double off = 0, diag = 0;
        for (int i = 0; i < 4; ++i) { diag += A[i][i] * A[i][i]; for (int j = i + 1; j < 4; ++j) off += A[i][j] * A[i][j]; }
        if (off <= 1e-60 + 1e-31 * diag) break;            // |off-diagonal| <= 3e-16 |diagonal|
#pragma unroll
        for (int p = 0; p < 3; ++p)
#pragma unroll
            for (int r = p + 1; r < 4; ++r) {
                const double apr = A[p][r];
                if (fabs(apr) <= 1e-22 * (fabs(A[p][p]) + fabs(A[r][r]))) { A[p][r] = 0.0; A[r][p] = 0.0; continue; }
                const double theta = 0.5 * (A[r][r] - A[p][p]) * fast_rcp(apr);
                const double th2p1 = fma(theta, theta, 1.0);
                const double t = (theta >= 0 ? 1.0 : -1.0) * fast_rcp(fabs(theta) + th2p1 * fast_rsqrt(th2p1));
                const double c = fast_rsqrt(fma(t, t, 1.0)), s = t * c;
#pragma unroll
                for (int k = 0; k < 4; ++k) { const double akp = A[k][p], akr = A[k][r]; A[k][p] = c * akp - s * akr; A[k][r] = s * akp + c * akr; }
#pragma unroll
                for (int k = 0; k < 4; ++k) { const double apk = A[p][k], ark = A[r][k]; A[p][k] = c * apk - s * ark; A[r][k] = s * apk + c * ark; }
#pragma unroll
                for (int k = 0; k < 4; ++k) { const double vkp = V[k][p], vkr = V[k][r]; V[k][p] = c * vkp - s * vkr; V[k][r] = s * vkp + c * vkr; }
            }
    }
    // column of the largest eigenvalue, selected with static indices only (a runtime column index would
    // push A and V to scratch)
    double lam = A[0][0], v0 = V[0][0], v1 = V[1][0], v2 = V[2][0], v3 = V[3][0];
#pragma unroll
    for (int c = 1; c < 4; ++c) {
        const bool gt = A[c][c] > lam;
        lam = gt ? A[c][c] : lam;
        v0 = gt ? V[0][c] : v0; v1 = gt ? V[1][c] : v1; v2 = gt ? V[2][c] : v2; v3 = gt ? V[3][c] : v3;
    }
#pragma unroll
    for (int i = 0; i < 4; ++i)
#pragma unroll
        for (int j = 0; j < 4; ++j) Vp[4 * i + j] = V[i][j];
    const double n = sqrt(((v0 * v0 + v1 * v1) + v2 * v2) + v3 * v3);
    const double sg = v0 < 0 ? -1.0 : 1.0;
    q[0] = sg * v0 / n; q[1] = sg * v1 / n; q[2] = sg * v2 / n; q[3] = sg * v3 / n;
}

// adjugate of a symmetric 4x4 (Laplace expansion over the 2x2 minors of its row pairs): adj(M) = det(M) inv(M), and for a
// singular M with a one-dimensional null space, adj(M) = (product of the non-zero eigenvalues) v v^T with v the null vector.
__device__ __forceinline__ void adj4(const double (&a)[4][4], double (&r)[4][4]) {
    const double s0 = a[0][0] * a[1][1] - a[0][1] * a[1][0], s1 = a[0][0] * a[1][2] - a[0][2] * a[1][0], s2 = a[0][0] * a[1][3] - a[0][3] * a[1][0];
    const double s3 = a[0][1] * a[1][2] - a[0][2] * a[1][1], s4 = a[0][1] * a[1][3] - a[0][3] * a[1][1], s5 = a[0][2] * a[1][3] - a[0][3] * a[1][2];
    const double c5 = a[2][2] * a[3][3] - a[2][3] * a[3][2], c4 = a[2][1] * a[3][3] - a[2][3] * a[3][1], c3 = a[2][1] * a[3][2] - a[2][2] * a[3][1];
    const double c2 = a[2][0] * a[3][3] - a[2][3] * a[3][0], c1 = a[2][0] * a[3][2] - a[2][2] * a[3][0], c0 = a[2][0] * a[3][1] - a[2][1] * a[3][0];
    r[0][0] = (a[1][1] * c5 - a[1][2] * c4) + a[1][3] * c3;  r[0][1] = (-a[0][1] * c5 + a[0][2] * c4) - a[0][3] * c3;
    r[0][2] = (a[3][1] * s5 - a[3][2] * s4) + a[3][3] * s3;  r[0][3] = (-a[2][1] * s5 + a[2][2] * s4) - a[2][3] * s3;
    r[1][0] = (-a[1][0] * c5 + a[1][2] * c2) - a[1][3] * c1; r[1][1] = (a[0][0] * c5 - a[0][2] * c2) + a[0][3] * c1;
    r[1][2] = (-a[3][0] * s5 + a[3][2] * s2) - a[3][3] * s1; r[1][3] = (a[2][0] * s5 - a[2][2] * s2) + a[2][3] * s1;
    r[2][0] = (a[1][0] * c4 - a[1][1] * c2) + a[1][3] * c0;  r[2][1] = (-a[0][0] * c4 + a[0][1] * c2) - a[0][3] * c0;
    r[2][2] = (a[3][0] * s4 - a[3][1] * s2) + a[3][3] * s0;  r[2][3] = (-a[2][0] * s4 + a[2][1] * s2) - a[2][3] * s0;
    r[3][0] = (-a[1][0] * c3 + a[1][1] * c1) - a[1][2] * c0; r[3][1] = (a[0][0] * c3 - a[0][1] * c1) + a[0][2] * c0;
    r[3][2] = (-a[3][0] * s3 + a[3][1] * s1) - a[3][2] * s0; r[3][3] = (a[2][0] * s3 - a[2][1] * s1) + a[2][2] * s0;
}

// Dominant eigenvector of Horn's symmetric, traceless 4x4 profile matrix as a unit quaternion (q0 >= 0).
// Fast path (a few hundred mostly independent flops instead of the serial Jacobi chain, which was 6-7 us of every ICP iteration
// on one lane): the largest root of the characteristic polynomial  l^4 + c2 l^2 + c1 l + c0  by Newton from the upper bound
// sqrt(-1.5 c2) (monotone from above), then  v = a column of adj(N - l I),  refined by Rayleigh-quotient rounds
// (l <- v^T N v / v^T v, new adjugate) until l stops moving at the 1e-15 level: each round squares the eigenvalue error, so
// two or three rounds reach what the conditioning of the eigenvector (eps / gap) allows.  When the dominant eigenvalue is
// (nearly) repeated -- too few or degenerate correspondences -- the adjugate vanishes and the warm-started Jacobi sweep
// below takes over.
__device__ inline void horn_max_eigvec(const double N[4][4], double q[4], double* Vp) {
    double nn2 = 0;
#pragma unroll
    for (int i = 0; i < 4; ++i)
#pragma unroll
        for (int j = 0; j < 4; ++j) nn2 = fma(N[i][j], N[i][j], nn2);
    bool ok = nn2 > 0 && nn2 < 1e300;
    if (ok) {
        double A[4][4], R[4][4];
#pragma unroll
        for (int i = 0; i < 4; ++i)
#pragma unroll
            for (int j = 0; j < 4; ++j) A[i][j] = N[i][j];
        // characteristic polynomial of a traceless symmetric matrix: c2 = -tr(N^2)/2, c1 = -tr(N^3)/3, c0 = det N
        const double c2 = -0.5 * nn2;
        double t3 = 0;
#pragma unroll
        for (int i = 0; i < 4; ++i)
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                const double n2ij = fma(N[i][3], N[3][j], fma(N[i][2], N[2][j], fma(N[i][1], N[1][j], N[i][0] * N[0][j])));
                t3 = fma(n2ij, N[j][i], t3);
            }
        const double c1 = -t3 / 3.0;
        adj4(A, R);
        const double c0 = fma(N[0][3], R[3][0], fma(N[0][2], R[2][0], fma(N[0][1], R[1][0], N[0][0] * R[0][0])));   // det = row 0 . column 0 of adj
        double lam = sqrt(-1.5 * c2) * (1.0 + 1e-12);
        for (int it = 0; it < 16; ++it) {                       // ~8 steps; the Rayleigh rounds below finish the job
            const double l2 = lam * lam;
            const double P = fma(fma(l2 + c2, lam, c1), lam, c0), dP = fma(fma(4.0, l2, 2.0 * c2), lam, c1);
            if (!(dP > 0)) break;
            const double step = P * fast_rcp(dP);             // Newton corrects itself: a few-ulp quotient is as good
            lam -= step;
            if (fabs(step) <= 1e-11 * fabs(lam)) break;
        }
        const double thr = 1e-9 * nn2 * sqrt(nn2);          // |adj| ~ (product of the gaps to the other three eigenvalues)
        double v0 = 0, v1 = 0, v2 = 0, v3 = 0;
        for (int round = 0; round < 6 && ok; ++round) {
#pragma unroll
            for (int i = 0; i < 4; ++i) A[i][i] = N[i][i] - lam;
            adj4(A, R);
            // the column of the largest diagonal cofactor (static indices only)
            double d = fabs(R[0][0]);
            v0 = R[0][0]; v1 = R[1][0]; v2 = R[2][0]; v3 = R[3][0];
#pragma unroll
            for (int c = 1; c < 4; ++c) {
                const bool gt = fabs(R[c][c]) > d;
                d = gt ? fabs(R[c][c]) : d;
                v0 = gt ? R[0][c] : v0; v1 = gt ? R[1][c] : v1; v2 = gt ? R[2][c] : v2; v3 = gt ? R[3][c] : v3;
            }
            if (!(d > thr)) { ok = false; break; }
            const double w0 = fma(N[0][3], v3, fma(N[0][2], v2, fma(N[0][1], v1, N[0][0] * v0)));
            const double w1 = fma(N[1][3], v3, fma(N[1][2], v2, fma(N[1][1], v1, N[1][0] * v0)));
            const double w2 = fma(N[2][3], v3, fma(N[2][2], v2, fma(N[2][1], v1, N[2][0] * v0)));
            const double w3 = fma(N[3][3], v3, fma(N[3][2], v2, fma(N[3][1], v1, N[3][0] * v0)));
            const double vv = fma(v3, v3, fma(v2, v2, fma(v1, v1, v0 * v0)));
            const double ray = fma(v3, w3, fma(v2, w2, fma(v1, w1, v0 * w0))) * fast_rcp(vv);
            const bool settled = fabs(ray - lam) <= 1e-15 * fabs(ray);
            lam = ray;
            if (settled) break;
        }
        if (ok) {
            const double rn = (v0 < 0 ? -1.0 : 1.0) * fast_rsqrt(((v0 * v0 + v1 * v1) + v2 * v2) + v3 * v3);
            q[0] = v0 * rn; q[1] = v1 * rn; q[2] = v2 * rn; q[3] = v3 * rn;
            return;
        }
    }
    sym4_max_eigvec(N, q, Vp);
}

// one v_min_f64 (fmin() lowers to canonicalising v_max pairs around it); neither operand is ever NaN here
__device__ __forceinline__ double vmin_f64(double a, double b) {
    double r;
    asm("v_min_f64 %0, %1, %2" : "=v"(r) : "v"(a), "v"(b));
    return r;
}
// wave-uniform minimum / maximum through the DPP row moves of wave_sum_fast (no LDS-crossbar permutes)
__device__ __forceinline__ double vmax_f64(double a, double b) {
    double r;
    asm("v_max_f64 %0, %1, %2" : "=v"(r) : "v"(a), "v"(b));
    return r;
}
#define CREG_DPP_MINMAX_F64(v, ctrl, mask, OP)                                                                                    \
    {                                                                                                                             \
        const int lo_ = __builtin_amdgcn_update_dpp(__double2loint(v), __double2loint(v), ctrl, mask, 0xF, false);                  \
        const int hi_ = __builtin_amdgcn_update_dpp(__double2hiint(v), __double2hiint(v), ctrl, mask, 0xF, false);                  \
        v = OP(v, __hiloint2double(hi_, lo_));                                                                                    \
    }
__device__ __forceinline__ double wave_min_fast(double v) {
    CREG_DPP_MINMAX_F64(v, 0xB1, 0xF, vmin_f64) CREG_DPP_MINMAX_F64(v, 0x4E, 0xF, vmin_f64) CREG_DPP_MINMAX_F64(v, 0x141, 0xF, vmin_f64)
    CREG_DPP_MINMAX_F64(v, 0x140, 0xF, vmin_f64) CREG_DPP_MINMAX_F64(v, 0x142, 0xA, vmin_f64) CREG_DPP_MINMAX_F64(v, 0x143, 0xC, vmin_f64)
    return __hiloint2double(__builtin_amdgcn_readlane(__double2hiint(v), 63), __builtin_amdgcn_readlane(__double2loint(v), 63));
}
__device__ __forceinline__ double wave_max_fast(double v) {
    CREG_DPP_MINMAX_F64(v, 0xB1, 0xF, vmax_f64) CREG_DPP_MINMAX_F64(v, 0x4E, 0xF, vmax_f64) CREG_DPP_MINMAX_F64(v, 0x141, 0xF, vmax_f64)
    CREG_DPP_MINMAX_F64(v, 0x140, 0xF, vmax_f64) CREG_DPP_MINMAX_F64(v, 0x142, 0xA, vmax_f64) CREG_DPP_MINMAX_F64(v, 0x143, 0xC, vmax_f64)
    return __hiloint2double(__builtin_amdgcn_readlane(__double2hiint(v), 63), __builtin_amdgcn_readlane(__double2loint(v), 63));
}

}  // namespace creg
