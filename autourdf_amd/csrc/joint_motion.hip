// joint_motion.hip -- what the registration knows about every joint beyond its axis, fp64 (this project's own; the
// reference writes a placeholder limit and stops).  Four entries, creg.h has their contracts:
//
// Link poses (k_link_poses, one thread per (sequence, step, link)): link_mean_pose of joints_dev.h, the very pose
// k_joint_axes works with, written as a rigid 4x4 in fp64.
//
// Joint positions (k_joint_samples, workgroups over (joint, sequence), threads over steps; then k_joint_summary, one
// workgroup per joint).  With X(s,t) = P^-1 C the child's pose in the parent's frame and X0 the same at the reference
// pose, D = X0^-1 X(s,t) is, for a revolute joint, the rotation by the joint position about local_axis through
// local_pos in the child's frame.  Per sample: the wrapped turn about the axis w = atan2(v . a, c), the tilt (the angle
// of what is left of D's rotation once the turn is taken out) and the slip (how far the point of the axis moves).  The
// unwrap along the steps is a serial recurrence: the workgroup's thread 0 runs it over each tile of JM_NT wrapped
// values the other threads left in LDS.  The summary is a second launch, so it reads what the first one wrote across a
// kernel boundary; its sums go per thread in stride order, then the xor butterfly, then the waves in order -- an order
// (S, num_steps) alone decides.  No atomics anywhere: two runs give the same bits, a joint alone the bits it gives
// among others.  Both launches are latency-bound (J x S workgroups of a few hundred samples).
//
// Joint slides (k_slide_samples, then the same k_joint_summary): the same D read as a prismatic or a fixed joint -- the
// slide along local_axis (a zero axis for a fixed joint), the whole rotation as tilt, the motion off the axis as slip.
//
// Motion error (k_motion_error, one thread per (pose, link)): how differently a link moved from its reference pose under
// two descriptions, Ma = A A0^-1 against Mb = B B0^-1, as an angle and as the distance between the images of one point.
//
// Every angle here is atan2 of skew_and_cos and norm3 of joints_dev.h, the expressions k_joint_axes and k_joint_types
// use.  The two series entries differ in their samples kernel only and share the rest as joint_series below.
#include <climits>
#include "creg_common.h"
#include "joints_dev.h"

namespace creg {

constexpr int JM_NT = 256;
constexpr double JM_TWO_PI = 6.283185307179586476925286766559;

// rows 0..2 of a row-major 4x4 -> R (3x3 row-major), t
__device__ inline void load_rigid(const double* __restrict__ M, double R[9], double t[3]) {
#pragma unroll
    for (int r = 0; r < 3; ++r) {
#pragma unroll
        for (int c = 0; c < 3; ++c) R[3 * r + c] = M[4 * r + c];
        t[r] = M[4 * r + 3];
    }
}

__global__ __launch_bounds__(JM_NT) void k_link_poses(const double* __restrict__ coords, int n_poses, int K, int L,
                                                      const int32_t* __restrict__ cl, const int32_t* __restrict__ off,
                                                      int n_cl, double* __restrict__ link_T) {
    const int idx = blockIdx.x * JM_NT + threadIdx.x;
    if (idx >= n_poses * L) return;
    const int st = idx / L, l = idx - st * L;
    const LinkSpan sp = link_span(cl, off, n_cl, l);
    double pos[3], q[4], R[9];
    link_mean_pose(coords + (size_t)st * K * 7, K, sp.idx, sp.n, pos, q, R);
    double* o = link_T + (size_t)idx * 16;
#pragma unroll
    for (int r = 0; r < 3; ++r) {
#pragma unroll
        for (int c = 0; c < 3; ++c) o[4 * r + c] = R[3 * r + c];
        o[4 * r + 3] = pos[r];
    }
    o[12] = 0.0; o[13] = 0.0; o[14] = 0.0; o[15] = 1.0;
}

// X = P^-1 C of links pl and cl at pose `at` (a (L,4,4) block of link_T)
__device__ inline void joint_pose(const double* __restrict__ at, int pl, int cl, double t[3], double R[9]) {
    double tp[3], Rp[9], tc[3], Rc[9];
    load_rigid(at + (size_t)pl * 16, Rp, tp);
    load_rigid(at + (size_t)cl * 16, Rc, tc);
    child_in_parent(tp, Rp, tc, Rc, t, R);
}

__global__ __launch_bounds__(JM_NT) void k_joint_samples(
    const double* __restrict__ link_T, int T, int L, const int32_t* __restrict__ joints, const double* __restrict__ local_axis,
    const double* __restrict__ local_pos, int ref_seq, int ref_step, int start, int num_steps, int S, double* __restrict__ q,
    double* __restrict__ tilt, double* __restrict__ slip) {
    __shared__ double s_w[JM_NT];
    const int j = blockIdx.x, s = blockIdx.y, tid = threadIdx.x;
    const int pl = joints[2 * j], cl = joints[2 * j + 1];
    if (pl < 0 || pl >= L || cl < 0 || cl >= L) return;          // uniform: the joint is skipped, nothing of it is read or written
    const double a[3] = {local_axis[3 * j], local_axis[3 * j + 1], local_axis[3 * j + 2]};
    const double p[3] = {local_pos[4 * j], local_pos[4 * j + 1], local_pos[4 * j + 2]};
    double t0[3], R0[9];
    joint_pose(link_T + ((size_t)ref_seq * T + ref_step) * L * 16, pl, cl, t0, R0);
    const size_t row = ((size_t)j * S + s) * num_steps;
    double u = 0.0, w_prev = 0.0;                                 // thread 0's recurrence state
    for (int base = 0; base < num_steps; base += JM_NT) {
        const int i = base + tid;
        if (i < num_steps) {
            double tx[3], Rx[9], td[3], R[9];
            joint_pose(link_T + ((size_t)s * T + (start + i)) * L * 16, pl, cl, tx, Rx);
            child_in_parent(t0, R0, tx, Rx, td, R);               // D = X0^-1 X
            double v[3], c;
            skew_and_cos(R, v, c);
            const double w = atan2((v[0] * a[0] + v[1] * a[1]) + v[2] * a[2], c);
            // E = Rot(a, -w) R, Rot(a, x) = I + sin x K + (1 - cos x) K K with K = [a]x and K K = a a^T - |a|^2 I
            const double sn = -sin(w), c1 = 1.0 - cos(w);
            const double k00 = -(a[2] * a[2]) - a[1] * a[1], k11 = -(a[2] * a[2]) - a[0] * a[0], k22 = -(a[1] * a[1]) - a[0] * a[0];
            const double k01 = a[0] * a[1], k02 = a[0] * a[2], k12 = a[1] * a[2];
            const double M[9] = {1.0 + c1 * k00,        -sn * a[2] + c1 * k01, sn * a[1] + c1 * k02,
                                 sn * a[2] + c1 * k01,  1.0 + c1 * k11,        -sn * a[0] + c1 * k12,
                                 -sn * a[1] + c1 * k02, sn * a[0] + c1 * k12,  1.0 + c1 * k22};
            double E[9];
#pragma unroll
            for (int r = 0; r < 3; ++r)
#pragma unroll
                for (int cc = 0; cc < 3; ++cc) E[3 * r + cc] = (M[3 * r] * R[cc] + M[3 * r + 1] * R[3 + cc]) + M[3 * r + 2] * R[6 + cc];
            double ve[3], ce;
            skew_and_cos(E, ve, ce);
            double e[3];
#pragma unroll
            for (int r = 0; r < 3; ++r) e[r] = (((R[3 * r] * p[0] + R[3 * r + 1] * p[1]) + R[3 * r + 2] * p[2]) + td[r]) - p[r];
            s_w[tid] = w;
            tilt[row + i] = atan2(norm3(ve), ce);
            slip[row + i] = norm3(e);
        }
        __syncthreads();
        if (tid == 0) {                                           // the unwrap: one serial pass over the tile
            const int n = num_steps - base < JM_NT ? num_steps - base : JM_NT;
            for (int k = 0; k < n; ++k) {
                const double w = s_w[k];
                if (base + k == 0) {
                    u = w;
                } else {
                    const double d = w - w_prev;
                    u = u + (d - JM_TWO_PI * rint(d / JM_TWO_PI));
                }
                w_prev = w;
                q[row + base + k] = u;
            }
        }
        __syncthreads();                                          // the tile is free again
    }
}

// The prismatic / fixed counterpart of k_joint_samples: the same D = X0^-1 X = [R d], read as a slide along `a`.  No
// unwrap, so no serial pass: every thread writes its own three figures.
__global__ __launch_bounds__(JM_NT) void k_slide_samples(
    const double* __restrict__ link_T, int T, int L, const int32_t* __restrict__ joints, const double* __restrict__ local_axis,
    int ref_seq, int ref_step, int start, int num_steps, int S, double* __restrict__ q, double* __restrict__ tilt,
    double* __restrict__ slip) {
    const int j = blockIdx.x, s = blockIdx.y, tid = threadIdx.x;
    const int pl = joints[2 * j], cl = joints[2 * j + 1];
    if (pl < 0 || pl >= L || cl < 0 || cl >= L) return;          // uniform: the joint is skipped, nothing of it is read or written
    const double a[3] = {local_axis[3 * j], local_axis[3 * j + 1], local_axis[3 * j + 2]};
    double t0[3], R0[9];
    joint_pose(link_T + ((size_t)ref_seq * T + ref_step) * L * 16, pl, cl, t0, R0);
    const size_t row = ((size_t)j * S + s) * num_steps;
    for (int i = tid; i < num_steps; i += JM_NT) {
        double tx[3], Rx[9], d[3], R[9];
        joint_pose(link_T + ((size_t)s * T + (start + i)) * L * 16, pl, cl, tx, Rx);
        child_in_parent(t0, R0, tx, Rx, d, R);                    // D = X0^-1 X
        double v[3], c;
        skew_and_cos(R, v, c);
        const double u = (d[0] * a[0] + d[1] * a[1]) + d[2] * a[2];
        const double e[3] = {d[0] - u * a[0], d[1] - u * a[1], d[2] - u * a[2]};
        q[row + i] = u;
        tilt[row + i] = atan2(norm3(v), c);                       // the whole rotation is unexplained
        slip[row + i] = norm3(e);
    }
}

__global__ __launch_bounds__(JM_NT) void k_joint_summary(const double* __restrict__ q, const double* __restrict__ tilt,
                                                         const double* __restrict__ slip, const int32_t* __restrict__ joints,
                                                         int L, int S, int num_steps, double* __restrict__ summary,
                                                         int32_t* __restrict__ where) {
    constexpr int NW = JM_NT / WAVE;
    __shared__ double s_lo[NW], s_hi[NW], s_f[NW][4];
    __shared__ int s_lo_at[NW], s_hi_at[NW], s_n[NW];
    const int j = blockIdx.x, tid = threadIdx.x;
    const int pl = joints[2 * j], cl = joints[2 * j + 1];
    if (pl < 0 || pl >= L || cl < 0 || cl >= L) return;          // uniform, as in k_joint_samples
    const int N = S * num_steps;
    const size_t row = (size_t)j * N;
    double lo = INFINITY, hi = -INFINITY, t2 = 0.0, tmax = 0.0, s2 = 0.0, smax = 0.0;
    int lo_at = INT_MAX, hi_at = INT_MAX, n = 0;
    for (int i = tid; i < N; i += JM_NT) {                        // (s, i) order within the thread: < and > keep the first
        const double u = q[row + i], ti = tilt[row + i], sl = slip[row + i];
        if (!(isfinite(u) && isfinite(ti) && isfinite(sl))) continue;
        ++n;
        if (u < lo) { lo = u; lo_at = i; }
        if (u > hi) { hi = u; hi_at = i; }
        t2 += ti * ti; s2 += sl * sl;
        tmax = ti > tmax ? ti : tmax;
        smax = sl > smax ? sl : smax;
    }
#pragma unroll
    for (int o = 32; o >= 1; o >>= 1) {                           // xor butterfly: every lane ends with the wave's result
        const double olo = __shfl_xor(lo, o, WAVE), ohi = __shfl_xor(hi, o, WAVE);
        const int olo_at = __shfl_xor(lo_at, o, WAVE), ohi_at = __shfl_xor(hi_at, o, WAVE);
        if (olo < lo || (olo == lo && olo_at < lo_at)) { lo = olo; lo_at = olo_at; }
        if (ohi > hi || (ohi == hi && ohi_at < hi_at)) { hi = ohi; hi_at = ohi_at; }
        const double otm = __shfl_xor(tmax, o, WAVE), osm = __shfl_xor(smax, o, WAVE);
        tmax = otm > tmax ? otm : tmax;
        smax = osm > smax ? osm : smax;
    }
    t2 = wave_sum(t2); s2 = wave_sum(s2); n = wave_sum(n);
    const int wv = tid / WAVE;
    if ((tid & (WAVE - 1)) == 0) {
        s_lo[wv] = lo; s_hi[wv] = hi; s_lo_at[wv] = lo_at; s_hi_at[wv] = hi_at; s_n[wv] = n;
        s_f[wv][0] = t2; s_f[wv][1] = tmax; s_f[wv][2] = s2; s_f[wv][3] = smax;
    }
    __syncthreads();
    if (tid != 0) return;
    for (int w = 1; w < NW; ++w) {                                // wave order: deterministic
        if (s_lo[w] < lo || (s_lo[w] == lo && s_lo_at[w] < lo_at)) { lo = s_lo[w]; lo_at = s_lo_at[w]; }
        if (s_hi[w] > hi || (s_hi[w] == hi && s_hi_at[w] < hi_at)) { hi = s_hi[w]; hi_at = s_hi_at[w]; }
        n += s_n[w];
        t2 += s_f[w][0]; s2 += s_f[w][2];
        tmax = s_f[w][1] > tmax ? s_f[w][1] : tmax;
        smax = s_f[w][3] > smax ? s_f[w][3] : smax;
    }
    double* sm = summary + 6 * (size_t)j;
    int32_t* wh = where + 5 * (size_t)j;
    wh[0] = n;
    if (n == 0) {
        for (int r = 0; r < 6; ++r) sm[r] = NAN;
        for (int r = 1; r < 5; ++r) wh[r] = -1;
        return;
    }
    const double dn = (double)n;
    sm[0] = lo; sm[1] = hi; sm[2] = sqrt(t2 / dn); sm[3] = tmax; sm[4] = sqrt(s2 / dn); sm[5] = smax;
    wh[1] = lo_at / num_steps; wh[2] = lo_at % num_steps; wh[3] = hi_at / num_steps; wh[4] = hi_at % num_steps;
}

// M = X X0^-1 (rigid inverse): R = Rx R0^T, t = tx - R t0
__device__ inline void motion_from(const double* __restrict__ X, const double* __restrict__ X0, double R[9], double t[3]) {
    double Rx[9], tx[3], R0[9], t0[3];
    load_rigid(X, Rx, tx);
    load_rigid(X0, R0, t0);
#pragma unroll
    for (int r = 0; r < 3; ++r)
#pragma unroll
        for (int c = 0; c < 3; ++c) R[3 * r + c] = (Rx[3 * r] * R0[3 * c] + Rx[3 * r + 1] * R0[3 * c + 1]) + Rx[3 * r + 2] * R0[3 * c + 2];
#pragma unroll
    for (int r = 0; r < 3; ++r) t[r] = tx[r] - ((R[3 * r] * t0[0] + R[3 * r + 1] * t0[1]) + R[3 * r + 2] * t0[2]);
}

__global__ __launch_bounds__(JM_NT) void k_motion_error(const double* __restrict__ A, const double* __restrict__ A0,
                                                        const double* __restrict__ B, const double* __restrict__ B0,
                                                        const double* __restrict__ point, int P, int L,
                                                        double* __restrict__ rot_err, double* __restrict__ pos_err) {
    const int idx = blockIdx.x * JM_NT + threadIdx.x;
    if (idx >= P * L) return;
    const int l = idx % L;
    double Ra[9], ta[3], Rb[9], tb[3];
    motion_from(A + (size_t)idx * 16, A0 + (size_t)l * 16, Ra, ta);
    motion_from(B + (size_t)idx * 16, B0 + (size_t)l * 16, Rb, tb);
    double Rr[9];                                                 // Ma^T Mb
#pragma unroll
    for (int r = 0; r < 3; ++r)
#pragma unroll
        for (int c = 0; c < 3; ++c) Rr[3 * r + c] = (Ra[r] * Rb[c] + Ra[3 + r] * Rb[3 + c]) + Ra[6 + r] * Rb[6 + c];
    double v[3], c;
    skew_and_cos(Rr, v, c);
    rot_err[idx] = atan2(norm3(v), c);
    const double x[3] = {point[3 * l], point[3 * l + 1], point[3 * l + 2]};
    double e[3];
#pragma unroll
    for (int r = 0; r < 3; ++r)
        e[r] = (((Ra[3 * r] * x[0] + Ra[3 * r + 1] * x[1]) + Ra[3 * r + 2] * x[2]) + ta[r]) -
               (((Rb[3 * r] * x[0] + Rb[3 * r + 1] * x[1]) + Rb[3 * r + 2] * x[2]) + tb[r]);
    pos_err[idx] = norm3(e);
}

}  // namespace creg
using namespace creg;

extern "C" int creg_link_poses_f64(const double* coords, int32_t S, int32_t T, int32_t K, const int32_t* link_clusters,
                                   const int32_t* link_offsets, int32_t n_link_clusters, int32_t L, double* link_T,
                                   creg_stream_t stream) {
    CREG_REQUIRE(coords && link_clusters && link_offsets && link_T, "creg_link_poses_f64: null pointer");
    CREG_REQUIRE(S >= 1 && T >= 1 && K >= 1 && K <= JOINT_MAX_K && L >= 1 && n_link_clusters >= 1 && (int64_t)S * T * L <= INT_MAX,
                 "creg_link_poses_f64: bad size (S=%d, T=%d, K=%d, L=%d; K <= %d, S*T*L < 2^31)", S, T, K, L, JOINT_MAX_K);
    hipLaunchKernelGGL(k_link_poses, dim3(cdiv((int64_t)S * T * L, JM_NT)), dim3(JM_NT), 0, (hipStream_t)stream, coords, S * T, K, L,
                       link_clusters, link_offsets, n_link_clusters, link_T);
    CREG_LAUNCH_CHECK();
    return CREG_OK;
}

// creg_joint_positions_f64 and creg_joint_slides_f64 but for their samples kernel: the checks, the J == 0 return before
// any pointer is looked at, the entry's own samples launch (`samples(grid, stream)`, over (joint, sequence)) and
// k_joint_summary.  `inputs` says that the entry's own input pointers are set.
template <class Samples>
static int joint_series(const char* who, int32_t S, int32_t T, int32_t L, const int32_t* joints, int32_t J, int32_t ref_seq,
                        int32_t ref_step, int32_t start_step, int32_t num_steps, bool inputs, double* q, double* tilt,
                        double* slip, double* summary, int32_t* where, creg_stream_t stream, Samples samples) {
    CREG_REQUIRE(S >= 1 && S <= 65535 && T >= 1 && L >= 1 && J >= 0, "%s: bad size (S=%d, T=%d, L=%d, J=%d; S <= 65535)", who, S, T, L, J);
    CREG_REQUIRE(start_step >= 0 && num_steps >= 1 && (int64_t)start_step + num_steps <= T && (int64_t)S * num_steps <= INT_MAX,
                 "%s: steps [%d, %d + %d) out of range for T=%d", who, start_step, start_step, num_steps, T);
    CREG_REQUIRE(ref_seq >= 0 && ref_seq < S && ref_step >= 0 && ref_step < T, "%s: reference pose (%d, %d) outside (S=%d, T=%d)", who,
                 ref_seq, ref_step, S, T);
    if (J == 0) return CREG_OK;
    CREG_REQUIRE(inputs && joints && q && tilt && slip && summary && where, "%s: null pointer", who);
    samples(dim3(J, S), (hipStream_t)stream);
    CREG_LAUNCH_CHECK();
    hipLaunchKernelGGL(k_joint_summary, dim3(J), dim3(JM_NT), 0, (hipStream_t)stream, q, tilt, slip, joints, L, S, num_steps, summary,
                       where);
    CREG_LAUNCH_CHECK();
    return CREG_OK;
}

extern "C" int creg_joint_positions_f64(const double* link_T, int32_t S, int32_t T, int32_t L, const int32_t* joints, int32_t J,
                                        const double* local_axis, const double* local_pos, int32_t ref_seq, int32_t ref_step,
                                        int32_t start_step, int32_t num_steps, double* q, double* tilt, double* slip,
                                        double* summary, int32_t* where, creg_stream_t stream) {
    return joint_series("creg_joint_positions_f64", S, T, L, joints, J, ref_seq, ref_step, start_step, num_steps,
                        link_T && local_axis && local_pos, q, tilt, slip, summary, where, stream, [&](dim3 grid, hipStream_t st) {
        hipLaunchKernelGGL(k_joint_samples, grid, dim3(JM_NT), 0, st, link_T, T, L, joints, local_axis, local_pos, ref_seq, ref_step,
                           start_step, num_steps, S, q, tilt, slip);
    });
}

extern "C" int creg_joint_slides_f64(const double* link_T, int32_t S, int32_t T, int32_t L, const int32_t* joints, int32_t J,
                                     const double* local_axis, int32_t ref_seq, int32_t ref_step, int32_t start_step,
                                     int32_t num_steps, double* q, double* tilt, double* slip, double* summary, int32_t* where,
                                     creg_stream_t stream) {
    return joint_series("creg_joint_slides_f64", S, T, L, joints, J, ref_seq, ref_step, start_step, num_steps, link_T && local_axis, q,
                        tilt, slip, summary, where, stream, [&](dim3 grid, hipStream_t st) {
        hipLaunchKernelGGL(k_slide_samples, grid, dim3(JM_NT), 0, st, link_T, T, L, joints, local_axis, ref_seq, ref_step, start_step,
                           num_steps, S, q, tilt, slip);
    });
}

extern "C" int creg_motion_error_f64(const double* A, const double* A0, const double* B, const double* B0, const double* point,
                                     int32_t P, int32_t L, double* rot_err, double* pos_err, creg_stream_t stream) {
    CREG_REQUIRE(A && A0 && B && B0 && point && rot_err && pos_err, "creg_motion_error_f64: null pointer");
    CREG_REQUIRE(P >= 1 && L >= 1 && (int64_t)P * L <= INT_MAX, "creg_motion_error_f64: bad size (P=%d, L=%d; P*L < 2^31)", P, L);
    hipLaunchKernelGGL(k_motion_error, dim3(cdiv((int64_t)P * L, JM_NT)), dim3(JM_NT), 0, (hipStream_t)stream, A, A0, B, B0, point, P, L,
                       rot_err, pos_err);
    CREG_LAUNCH_CHECK();
    return CREG_OK;
}
