// joint_types.hip -- which kind of joint every edge of the kinematic tree is, fp64 (this project's own; the reference
// handles revolute joints only).  The companion of k_joint_axes (joints.hip) with its launch shape and its samples: one
// workgroup of 256 threads per joint, thread tid taking samples tid, tid + 256, ... of the sequence-major / phase / step
// enumeration (sample_steps of joints_dev.h).
//
// Per sample the relative motion D = X_{i-1}^-1 X_i = [R t] is joint_sample_motion of joints_dev.h, the function
// k_joint_axes calls, and its angle theta = atan2(|v(R)|, c(R)) comes from skew_and_cos and norm3 of the same header,
// which screw_axis calls too, so sample_angle has k_joint_axes' bits.  A sample turns
// (theta >= turn_min), slides (it does not turn and |t| >= slide_min), stands still, or is bad (not finite).  A joint with
// a turning sample is revolute, else one with a sliding sample prismatic, else one with a still sample fixed.  The slide
// direction is the top eigenvector of sum t t^T over the slide samples, signed by the first of them; its six sums run per
// thread in stride order, then the xor butterfly, then the four waves in order.  No atomics on floating-point data: two
// runs give the same bits, a joint alone the bits it gives among others.  Latency-bound (J workgroups, NS <= 4096 samples).
#include <climits>
#include <cmath>
#include "creg_common.h"
#include "creg_dev.h"
#include "joints_dev.h"
#include "joints_host.h"

namespace creg {

constexpr int JT_NT = 256;

__global__ __launch_bounds__(JT_NT) void k_joint_types(
    const double* __restrict__ coords, int S, int T, int K, const int32_t* __restrict__ cl, const int32_t* __restrict__ off,
    int n_cl, int L, const int32_t* __restrict__ joints, int start, int num_steps, int interval, int per_seq, int NS,
    double turn_min, double slide_min, double* __restrict__ s_angle, double* __restrict__ s_slide, int32_t* __restrict__ s_kind,
    int32_t* __restrict__ counts, int32_t* __restrict__ type, double* __restrict__ slide_axis, double* __restrict__ global_axis,
    double* __restrict__ global_pos) {
    constexpr int NW = JT_NT / WAVE;
    __shared__ double s_part[NW][6], s_t0[3];
    __shared__ int s_cnt[NW][4], s_first[NW];
    const int jt = blockIdx.x, tid = threadIdx.x;
    const int pl = joints[2 * jt], chl = joints[2 * jt + 1];
    if (pl < 0 || pl >= L || chl < 0 || chl >= L) return;        // uniform: the joint is skipped, nothing of it is read or written
    const LinkSpan P = link_span(cl, off, n_cl, pl), C = link_span(cl, off, n_cl, chl);
    const size_t base = (size_t)jt * NS;
    double acc[6] = {0, 0, 0, 0, 0, 0};                           // xx xy xz yy yz zz of the slide samples
    int n[4] = {0, 0, 0, 0};                                      // still, turn, slide, bad
    int first = INT_MAX;                                          // this thread's first slide sample
    for (int i = tid; i < NS; i += JT_NT) {
        double t[3], R[9], v[3], c;                               // X_{i-1}^-1 X_i of sample i (sample_steps() order)
        joint_sample_motion(coords, T, K, P, C, i, per_seq, start, num_steps, interval, t, R);
        skew_and_cos(R, v, c);                                    // as screw_axis (joints.hip): the angle has its bits
        const double th = atan2(norm3(v), c);
        const double len = norm3(t);
        int kind;
        if (!(isfinite(th) && isfinite(t[0]) && isfinite(t[1]) && isfinite(t[2]))) kind = -1;
        else if (th >= turn_min) kind = 1;
        else if (len >= slide_min) kind = 2;
        else kind = 0;
        s_angle[base + i] = th;
        s_kind[base + i] = kind;
#pragma unroll
        for (int r = 0; r < 3; ++r) s_slide[3 * (base + i) + r] = t[r];
        ++n[kind < 0 ? 3 : kind];
        if (kind == 2) {
            acc[0] += t[0] * t[0]; acc[1] += t[0] * t[1]; acc[2] += t[0] * t[2];
            acc[3] += t[1] * t[1]; acc[4] += t[1] * t[2]; acc[5] += t[2] * t[2];
            if (i < first) first = i;
        }
    }
#pragma unroll
    for (int r = 0; r < 6; ++r) acc[r] = wave_sum(acc[r]);       // xor butterfly: every lane holds the same bits
#pragma unroll
    for (int r = 0; r < 4; ++r) n[r] = wave_sum(n[r]);
#pragma unroll
    for (int o = 32; o >= 1; o >>= 1) {
        const int other = __shfl_xor(first, o, WAVE);
        first = other < first ? other : first;
    }
    const int wv = tid / WAVE;
    if ((tid & (WAVE - 1)) == 0) {
        for (int r = 0; r < 6; ++r) s_part[wv][r] = acc[r];
        for (int r = 0; r < 4; ++r) s_cnt[wv][r] = n[r];
        s_first[wv] = first;
    }
    __syncthreads();
    int f = s_first[0];
    for (int w = 1; w < NW; ++w) f = s_first[w] < f ? s_first[w] : f;
    if (f != INT_MAX && f % JT_NT == tid)                         // the owner of the first slide sample reads back its own write
        for (int r = 0; r < 3; ++r) s_t0[r] = s_slide[3 * (base + f) + r];
    __syncthreads();
    if (tid != 0) return;
    for (int w = 1; w < NW; ++w) {                                // wave order: deterministic
        for (int r = 0; r < 6; ++r) acc[r] += s_part[w][r];
        for (int r = 0; r < 4; ++r) n[r] += s_cnt[w][r];
    }
    for (int r = 0; r < 4; ++r) counts[4 * jt + r] = n[r];
    type[jt] = n[1] > 0 ? 1 : (n[2] > 0 ? 2 : (n[0] > 0 ? 0 : -1));
    // the child's mean pose at the first pose (sequence 0, step start): the frame k_joint_axes reports in
    double tc[3], qc[4], Rc[9];
    link_mean_pose(coords + (size_t)start * K * 7, K, C.idx, C.n, tc, qc, Rc);
    for (int r = 0; r < 3; ++r) global_pos[3 * jt + r] = (double)(float)tc[r];   // as pose_to_f32_matrix holds it
    if (n[2] == 0) {
        for (int r = 0; r < 3; ++r) { slide_axis[3 * jt + r] = NAN; global_axis[3 * jt + r] = NAN; }
        return;
    }
    double M[3][3] = {{acc[0], acc[1], acc[2]}, {acc[1], acc[3], acc[4]}, {acc[2], acc[4], acc[5]}}, ax[3];
    jacobi_top<3>(M, ax);
    const double nax = sqrt((ax[0] * ax[0] + ax[1] * ax[1]) + ax[2] * ax[2]);
    const double sg = ((ax[0] * s_t0[0] + ax[1] * s_t0[1]) + ax[2] * s_t0[2]) < 0.0 ? -1.0 : 1.0;
    for (int r = 0; r < 3; ++r) ax[r] = sg * ax[r] / nax;
    for (int r = 0; r < 3; ++r) {
        slide_axis[3 * jt + r] = ax[r];
        global_axis[3 * jt + r] = (Rc[3 * r] * ax[0] + Rc[3 * r + 1] * ax[1]) + Rc[3 * r + 2] * ax[2];
    }
}

}  // namespace creg
using namespace creg;

extern "C" int creg_joint_types_f64(const double* coords, int32_t S, int32_t T, int32_t K, const int32_t* link_clusters,
                                    const int32_t* link_offsets, int32_t n_link_clusters, int32_t L, const int32_t* joints,
                                    int32_t J, int32_t start_step, int32_t num_steps, int32_t interval, double turn_min,
                                    double slide_min, double* sample_angle, double* sample_slide, int32_t* sample_kind,
                                    int32_t* counts, int32_t* type, double* slide_axis, double* global_axis,
                                    double* global_pos, creg_stream_t stream) {
    const int NS = joint_sample_count("creg_joint_types_f64", S, T, K, &L, J, n_link_clusters, start_step, num_steps, interval);
    if (NS < 0) return CREG_EINVAL;
    CREG_REQUIRE(std::isfinite(turn_min) && turn_min >= 0.0 && std::isfinite(slide_min) && slide_min >= 0.0,
                 "creg_joint_types_f64: turn_min and slide_min must be finite and >= 0 (got %g, %g)", turn_min, slide_min);
    if (J == 0) return CREG_OK;
    CREG_REQUIRE(coords && link_clusters && link_offsets && joints && counts && type && slide_axis && global_axis && global_pos,
                 "creg_joint_types_f64: null pointer");
    CREG_REQUIRE(NS == 0 || (sample_angle && sample_slide && sample_kind), "creg_joint_types_f64: null sample output");
    hipLaunchKernelGGL(k_joint_types, dim3(J), dim3(JT_NT), 0, (hipStream_t)stream, coords, S, T, K, link_clusters, link_offsets,
                       n_link_clusters, L, joints, start_step, num_steps, interval, NS / S, NS, turn_min, slide_min,
                       sample_angle, sample_slide, sample_kind, counts, type, slide_axis, global_axis, global_pos);
    CREG_LAUNCH_CHECK();
    return CREG_OK;
}
