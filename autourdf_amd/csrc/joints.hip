// joints.hip -- N4, the geometric half of the URDF stage, fp64.  Replaces estimate_joint_axes_from_tree of the reference's
// PointCloud/compute_joints.py (:216-268, with get_cluster_pose_mean, average_quaternions, relative_transform,
// calculate_joint_axis_relative and optimize_joint_axis, :10-214) and CoordMap.cluster_to_link (coord_map.py:443-502).
//
// Joint axes (k_joint_axes, one workgroup per joint, one thread per sample).  A sample is one pair of consecutive steps
// (i - interval, i) of one phase of one sequence.  Per step, a link's mean pose is the mean xyz of its clusters plus the
// top eigenvector of (1/n) sum q q^T (cyclic Jacobi in registers; the sign is irrelevant, quaternion_to_matrix divides by
// |q|^2).  With X_i = P_i^-1 C_i the child's pose in the parent's frame, the relative motion of the reference's T_r1 is
// X_{i-1}^-1 X_i (joint_sample_motion of joints_dev.h, which k_joint_types shares; the limits JOINT_* and the argument
// checks of joints_host.h are shared likewise).  Its screw axis comes in closed form (direction from the skew part, from the symmetric part past 90 deg;
// angle atan2(|vee|, (tr - 1) / 2) in [0, pi]; the point of the axis closest to the origin
// 1/2 (t_perp + cot(theta/2) d x t_perp)), canonicalised as init_position does.  DESIGN N4 has why this equals the
// reference's eig of the 4x4 wherever that is well-posed.  The principal axis is the top eigenvector of sum a a^T over the
// usable samples, the point their mean, and refine_position's Brent search its closed form.
//
// Link clouds (k_link_clouds, workgroups (frame, link) x row slices of LC_ROWS rows).  The link matrix is quaternion_to_matrix of the fp64
// mean of the link's cluster coords, rounded to float32 as xyzquant2matrix_torch's torch.eye(4) rounds it; every
// cluster's local points go to the world frame by its own pose and back to the link frame by the fp64 inverse of that
// float32 matrix.  The only part of the stage whose work grows with the point count: 24 B read, 48 B written per point.
#include <climits>
#include "creg_common.h"
#include "creg_dev.h"
#include "joints_dev.h"
#include "joints_host.h"

namespace creg {

constexpr int JA_NT = 256;
constexpr int LC_NT = 256;
constexpr int LC_ROWS = 4 * LC_NT;      // output rows per workgroup slice of one (frame, link)
constexpr int LC_MAX_SLICES = 256;      // grid.y cap; a workgroup strides over slices y, y + G, ...

// Screw axis of [R t]: unit direction d and angle theta in [0, pi] with R = rot(d, theta), and the canonical point
// of the axis (init_position of compute_joints.py:68-77 applied to the point closest to the origin).
__device__ void screw_axis(const double R[9], const double t[3], double d[3], double& theta, double p[3]) {
    double v[3], c;                                       // sin(theta) d, cos(theta)
    skew_and_cos(R, v, c);
    const double s = norm3(v);
    theta = atan2(s, c);
    if (c >= 0.0) {
        d[0] = v[0] / s; d[1] = v[1] / s; d[2] = v[2] / s;
    } else {                                              // (R + R^T)/2 - cos(theta) I = (1 - cos(theta)) d d^T
        const double B[9] = {R[0] - c, (R[1] + R[3]) * 0.5, (R[2] + R[6]) * 0.5,
                             (R[1] + R[3]) * 0.5, R[4] - c, (R[5] + R[7]) * 0.5,
                             (R[2] + R[6]) * 0.5, (R[5] + R[7]) * 0.5, R[8] - c};
        int m = 0;
        if (B[4] > B[3 * m + m]) m = 1;
        if (B[8] > B[3 * m + m]) m = 2;
        const double col[3] = {B[m], B[3 + m], B[6 + m]};
        const double nc = sqrt((col[0] * col[0] + col[1] * col[1]) + col[2] * col[2]);
        const double sg = ((col[0] * v[0] + col[1] * v[1]) + col[2] * v[2]) < 0.0 ? -1.0 : 1.0;
        d[0] = sg * col[0] / nc; d[1] = sg * col[1] / nc; d[2] = sg * col[2] / nc;
    }
    const double ax = (d[0] * t[0] + d[1] * t[1]) + d[2] * t[2];
    const double tp[3] = {t[0] - ax * d[0], t[1] - ax * d[1], t[2] - ax * d[2]};
    const double cot = 1.0 / tan(0.5 * theta);
    const double dx[3] = {d[1] * tp[2] - d[2] * tp[1], d[2] * tp[0] - d[0] * tp[2], d[0] * tp[1] - d[1] * tp[0]};
    double q[3];
#pragma unroll
    for (int i = 0; i < 3; ++i) q[i] = 0.5 * (tp[i] + cot * dx[i]);
    int m = 0;                                            // np.argmax(np.abs(axis)): the first maximum
    if (fabs(d[1]) > fabs(d[m])) m = 1;
    if (fabs(d[2]) > fabs(d[m])) m = 2;
    const double nn = q[m] / d[m];
#pragma unroll
    for (int i = 0; i < 3; ++i) p[i] = q[i] - nn * d[i];
}

// General 4x4 inverse (Gauss-Jordan with partial pivoting, fp64), row-major.
__device__ void inv4(const double M[16], double Inv[16]) {
    double A[4][8];
#pragma unroll
    for (int r = 0; r < 4; ++r)
#pragma unroll
        for (int c = 0; c < 4; ++c) { A[r][c] = M[4 * r + c]; A[r][4 + c] = r == c ? 1.0 : 0.0; }
#pragma unroll
    for (int col = 0; col < 4; ++col) {
        int piv = col;
#pragma unroll
        for (int r = col + 1; r < 4; ++r)
            if (fabs(A[r][col]) > fabs(A[piv][col])) piv = r;
#pragma unroll
        for (int r = col; r < 4; ++r)                     // swap rows col and piv with constant indices only
            if (r == piv && r != col)
#pragma unroll
                for (int c = 0; c < 8; ++c) { const double tmp = A[col][c]; A[col][c] = A[r][c]; A[r][c] = tmp; }
        const double inv = 1.0 / A[col][col];
#pragma unroll
        for (int c = 0; c < 8; ++c) A[col][c] *= inv;
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            if (r == col) continue;
            const double f = A[r][col];
#pragma unroll
            for (int c = 0; c < 8; ++c) A[r][c] -= f * A[col][c];
        }
    }
#pragma unroll
    for (int r = 0; r < 4; ++r)
#pragma unroll
        for (int c = 0; c < 4; ++c) Inv[4 * r + c] = A[r][4 + c];
}

// xyzquant2matrix_torch: [R | t] written into a float32 torch.eye(4).
__device__ void pose_to_f32_matrix(const double t[3], const double R[9], double M[16]) {
#pragma unroll
    for (int r = 0; r < 3; ++r) {
#pragma unroll
        for (int c = 0; c < 3; ++c) M[4 * r + c] = (double)(float)R[3 * r + c];
        M[4 * r + 3] = (double)(float)t[r];
    }
    M[12] = 0.0; M[13] = 0.0; M[14] = 0.0; M[15] = 1.0;
}

__global__ __launch_bounds__(JA_NT) void k_joint_axes(
    const double* __restrict__ coords, int S, int T, int K, const int32_t* __restrict__ cl, const int32_t* __restrict__ off,
    int n_cl, const int32_t* __restrict__ joints, int start, int num_steps, int interval, int per_seq, int NS,
    double* __restrict__ s_axis, double* __restrict__ s_angle, double* __restrict__ s_point, int32_t* __restrict__ s_usable,
    double* __restrict__ local_axis, double* __restrict__ local_pos, double* __restrict__ global_pos,
    double* __restrict__ global_axis, int32_t* __restrict__ count, double* __restrict__ first_pose) {
    __shared__ int s_first;
    __shared__ double s_a0[3], s_part[JA_NT / WAVE][10];
    const int jt = blockIdx.x, tid = threadIdx.x;
    const LinkSpan P = link_span(cl, off, n_cl, joints[2 * jt]), C = link_span(cl, off, n_cl, joints[2 * jt + 1]);
    if (tid == 0) s_first = INT_MAX;
    __syncthreads();
    const size_t base = (size_t)jt * NS;
    int first = INT_MAX;
    for (int i = tid; i < NS; i += blockDim.x) {
        double t[3], R[9];                                        // X_{i-1}^-1 X_i of sample i (sample_steps() order)
        joint_sample_motion(coords, T, K, P, C, i, per_seq, start, num_steps, interval, t, R);
        double d[3], th, p[3];
        screw_axis(R, t, d, th, p);
        const bool ok = th >= JOINT_THETA_MIN && isfinite(th) && isfinite(p[0]) && isfinite(p[1]) && isfinite(p[2]) &&
                        isfinite(d[0]) && isfinite(d[1]) && isfinite(d[2]);
        s_angle[base + i] = th;
        s_usable[base + i] = ok;
#pragma unroll
        for (int r = 0; r < 3; ++r) {
            s_axis[3 * (base + i) + r] = ok ? d[r] : NAN;
            s_point[3 * (base + i) + r] = ok ? p[r] : NAN;
        }
        if (ok && i < first) {
            first = i;
            atomicMin(&s_first, i);
        }
    }
    __syncthreads();
    const int f = s_first;
    // the parent's and child's mean poses at the first pose (sequence 0, step start): optimize_joint_axis's frame
    const double* c0 = coords + (size_t)start * K * 7;
    double tp[3], tc[3], Rp[9], Rc[9], qp[4], qc[4];
    if (tid == 0) {
        link_mean_pose(c0, K, P.idx, P.n, tp, qp, Rp);
        link_mean_pose(c0, K, C.idx, C.n, tc, qc, Rc);
        if (first_pose)
            for (int r = 0; r < 7; ++r) {
                first_pose[14 * jt + r] = r < 3 ? tp[r] : qp[r - 3];
                first_pose[14 * jt + 7 + r] = r < 3 ? tc[r] : qc[r - 3];
            }
    }
    if (f == INT_MAX) {                                   // no usable step: NaN outputs, count 0 (uniform branch)
        if (tid == 0) {
            for (int r = 0; r < 3; ++r) {
                local_axis[3 * jt + r] = NAN; global_pos[3 * jt + r] = NAN; global_axis[3 * jt + r] = NAN;
            }
            for (int r = 0; r < 4; ++r) local_pos[4 * jt + r] = NAN;
            count[jt] = 0;
        }
        return;
    }
    if (f % blockDim.x == tid)                            // the owner of the first usable sample reads back its own write
        for (int r = 0; r < 3; ++r) s_a0[r] = s_axis[3 * (base + f) + r];
    __syncthreads();
    double acc[10] = {0, 0, 0, 0, 0, 0, 0, 0, 0, 0};       // xx xy xz yy yz zz, point xyz, count
    for (int i = tid; i < NS; i += blockDim.x) {
        if (!s_usable[base + i]) continue;
        double a[3];
        for (int r = 0; r < 3; ++r) a[r] = s_axis[3 * (base + i) + r];
        if ((a[0] * s_a0[0] + a[1] * s_a0[1]) + a[2] * s_a0[2] < 0.0) { a[0] = -a[0]; a[1] = -a[1]; a[2] = -a[2]; }
        acc[0] += a[0] * a[0]; acc[1] += a[0] * a[1]; acc[2] += a[0] * a[2];
        acc[3] += a[1] * a[1]; acc[4] += a[1] * a[2]; acc[5] += a[2] * a[2];
        for (int r = 0; r < 3; ++r) acc[6 + r] += s_point[3 * (base + i) + r];
        acc[9] += 1.0;
    }
#pragma unroll
    for (int r = 0; r < 10; ++r) acc[r] = wave_sum(acc[r]);   // xor butterfly: every lane holds the same bits
    if ((tid & (WAVE - 1)) == 0)
        for (int r = 0; r < 10; ++r) s_part[tid / WAVE][r] = acc[r];
    __syncthreads();
    if (tid != 0) return;
    for (int w = 1; w < (int)blockDim.x / WAVE; ++w)      // wave order: deterministic
        for (int r = 0; r < 10; ++r) acc[r] += s_part[w][r];
    double M[3][3] = {{acc[0], acc[1], acc[2]}, {acc[1], acc[3], acc[4]}, {acc[2], acc[4], acc[5]}}, ax[3];
    jacobi_top<3>(M, ax);
    const double nax = sqrt((ax[0] * ax[0] + ax[1] * ax[1]) + ax[2] * ax[2]);
    const double sg = ((ax[0] * s_a0[0] + ax[1] * s_a0[1]) + ax[2] * s_a0[2]) < 0.0 ? -1.0 : 1.0;
    for (int r = 0; r < 3; ++r) ax[r] = sg * ax[r] / nax;
    const double ppos[3] = {acc[6] / acc[9], acc[7] / acc[9], acc[8] / acc[9]};

    // optimize_joint_axis's frame bookkeeping at the first pose
    double Tc[16], Ti[16], gax[3];
    for (int r = 0; r < 3; ++r) gax[r] = (Rc[3 * r] * ax[0] + Rc[3 * r + 1] * ax[1]) + Rc[3 * r + 2] * ax[2];
    pose_to_f32_matrix(tc, Rc, Tc);
    double g[3];
    for (int r = 0; r < 3; ++r) g[r] = ((Tc[4 * r] * ppos[0] + Tc[4 * r + 1] * ppos[1]) + Tc[4 * r + 2] * ppos[2]) + Tc[4 * r + 3];
    // refine_position: argmin_t |P - (g + t d)| + |C - (g + t d)| in closed form
    const double u[3] = {tp[0] - g[0], tp[1] - g[1], tp[2] - g[2]}, v[3] = {tc[0] - g[0], tc[1] - g[1], tc[2] - g[2]};
    const double su = (u[0] * ax[0] + u[1] * ax[1]) + u[2] * ax[2], sv = (v[0] * ax[0] + v[1] * ax[1]) + v[2] * ax[2];
    double ru = 0.0, rv = 0.0;
    for (int r = 0; r < 3; ++r) {
        const double eu = u[r] - su * ax[r], ev = v[r] - sv * ax[r];
        ru += eu * eu; rv += ev * ev;
    }
    ru = sqrt(ru); rv = sqrt(rv);
    const double ts = ru + rv > 0.0 ? su + (sv - su) * (ru / (ru + rv)) : 0.5 * (su + sv);
    const double gp[4] = {g[0] + ts * ax[0], g[1] + ts * ax[1], g[2] + ts * ax[2], 1.0};
    inv4(Tc, Ti);
    double lp[4];
    for (int r = 0; r < 4; ++r) lp[r] = ((Ti[4 * r] * gp[0] + Ti[4 * r + 1] * gp[1]) + Ti[4 * r + 2] * gp[2]) + Ti[4 * r + 3] * gp[3];
    for (int r = 0; r < 3; ++r) {
        local_axis[3 * jt + r] = ax[r];
        global_axis[3 * jt + r] = gax[r];
        global_pos[3 * jt + r] = ((Tc[4 * r] * lp[0] + Tc[4 * r + 1] * lp[1]) + Tc[4 * r + 2] * lp[2]) + Tc[4 * r + 3] * lp[3];
    }
    for (int r = 0; r < 4; ++r) local_pos[4 * jt + r] = lp[r];
    count[jt] = (int32_t)acc[9];
}

__global__ __launch_bounds__(LC_NT) void k_link_clouds(
    const double* __restrict__ coords, const double* __restrict__ mats, int T, int K, int L, const int32_t* __restrict__ cl,
    const int32_t* __restrict__ off, int n_cl, const double* __restrict__ pts, const int64_t* __restrict__ pt_off, int64_t n_pts,
    const int64_t* __restrict__ out_off, int64_t n_out, float* __restrict__ link_mats, float* __restrict__ mean_mats,
    double* __restrict__ wf, double* __restrict__ lf) {
    __shared__ double s_inv[12];
    const int b = blockIdx.x, t = b / L, l = b % L, tid = threadIdx.x;
    const bool lead = blockIdx.y == 0;                    // writes the matrices; every slice recomputes the inverse
    const LinkSpan S = link_span(cl, off, n_cl, l);
    const double* ct = coords + (size_t)t * K * 7;
    if (tid == 0) {
        double m[7] = {0, 0, 0, 0, 0, 0, 0};
        float acc[16];
        for (int e = 0; e < 16; ++e) acc[e] = 0.0f;
        for (int c = 0; c < S.n; ++c) {
            const int k = S.idx[c];
            if (k < 0 || k >= K) continue;
            const double* p = ct + (size_t)k * 7;
            for (int e = 0; e < 7; ++e) m[e] += p[e];
            double R[9], Mk[16];
            quat_to_matrix(p + 3, R);
            pose_to_f32_matrix(p, R, Mk);
            for (int e = 0; e < 16; ++e) acc[e] += (float)Mk[e];
        }
        const double dn = (double)S.n;
        for (int e = 0; e < 7; ++e) m[e] /= dn;
        double R[9], Ml[16], Mi[16];
        quat_to_matrix(m + 3, R);
        pose_to_f32_matrix(m, R, Ml);
        inv4(Ml, Mi);
        for (int e = 0; e < 12; ++e) s_inv[e] = Mi[e];
        float* lm = link_mats + (size_t)b * 16;
        if (lead)
            for (int e = 0; e < 16; ++e) lm[e] = (float)Ml[e];
        if (lead && mean_mats) {
            float* mm = mean_mats + (size_t)b * 16;
            for (int e = 0; e < 16; ++e) mm[e] = acc[e] / (float)S.n;
        }
    }
    __syncthreads();
    double Ai[12];
    for (int e = 0; e < 12; ++e) Ai[e] = s_inv[e];
    const int64_t o_beg = out_off[b] > 0 ? out_off[b] : 0;
    const int64_t o_end = out_off[b + 1] < n_out ? out_off[b + 1] : n_out;
    // this workgroup's rows: slices blockIdx.y, blockIdx.y + gridDim.y, ... of LC_ROWS rows each
    for (int64_t s0 = o_beg + (int64_t)blockIdx.y * LC_ROWS; s0 < o_end; s0 += (int64_t)gridDim.y * LC_ROWS) {
        const int64_t s1 = s0 + LC_ROWS < o_end ? s0 + LC_ROWS : o_end;
        int64_t o = o_beg;                                // first row of cluster c: its clusters in set order
        for (int c = 0; c < S.n && o < s1; ++c) {
            const int k = S.idx[c];
            if (k < 0 || k >= K) continue;
            const int64_t p0 = pt_off[(size_t)t * K + k];
            int64_t p1 = pt_off[(size_t)t * K + k + 1];
            p1 = p1 < n_pts ? p1 : n_pts;
            const int64_t n = p1 > p0 ? p1 - p0 : 0;
            const int64_t lo = o > s0 ? o : s0, hi = o + n < s1 ? o + n : s1;
            if (lo < hi) {
                const double* Mk = mats + ((size_t)t * K + k) * 16;
                const double R[9] = {Mk[0], Mk[1], Mk[2], Mk[4], Mk[5], Mk[6], Mk[8], Mk[9], Mk[10]};
                const double tt[3] = {Mk[3], Mk[7], Mk[11]};
                for (int64_t dst = lo + tid; dst < hi; dst += blockDim.x) {
                    const int64_t p = p0 + (dst - o);
                    const double x = pts[3 * p], y = pts[3 * p + 1], z = pts[3 * p + 2];
                    double w[3];
                    for (int r = 0; r < 3; ++r) w[r] = ((x * R[3 * r] + y * R[3 * r + 1]) + z * R[3 * r + 2]) + tt[r];
                    for (int r = 0; r < 3; ++r) {
                        wf[3 * dst + r] = w[r];
                        lf[3 * dst + r] = ((w[0] * Ai[4 * r] + w[1] * Ai[4 * r + 1]) + w[2] * Ai[4 * r + 2]) + Ai[4 * r + 3];
                    }
                }
            }
            o += n;
        }
    }
}

}  // namespace creg
using namespace creg;

extern "C" int creg_joint_axes_samples(int32_t S, int32_t num_steps, int32_t interval) {
    if (S < 1 || num_steps < 1 || interval < 1) return 0;
    int64_t per = 0;
    for (int a = 0; a < interval && a < num_steps; ++a) {
        const int64_t na = (num_steps - a + interval - 1) / interval;
        per += na > 1 ? na - 1 : 0;
    }
    const int64_t ns = per * S;
    return ns > INT_MAX ? INT_MAX : (int32_t)ns;
}

extern "C" int creg_joint_axes_f64(const double* coords, int32_t S, int32_t T, int32_t K, const int32_t* link_clusters,
                                   const int32_t* link_offsets, int32_t n_link_clusters, const int32_t* joints, int32_t J,
                                   int32_t start_step, int32_t num_steps, int32_t interval, double* sample_axis,
                                   double* sample_angle, double* sample_point, int32_t* sample_usable, double* local_axis,
                                   double* local_pos, double* global_pos, double* global_axis, int32_t* count,
                                   double* first_pose, creg_stream_t stream) {
    CREG_REQUIRE(coords && link_clusters && link_offsets && joints && local_axis && local_pos && global_pos && global_axis &&
                 count, "creg_joint_axes_f64: null pointer");
    const int NS = joint_sample_count("creg_joint_axes_f64", S, T, K, nullptr, J, n_link_clusters, start_step, num_steps, interval);
    if (NS < 0) return CREG_EINVAL;
    CREG_REQUIRE(NS == 0 || (sample_axis && sample_angle && sample_point && sample_usable),
                 "creg_joint_axes_f64: null sample output");
    if (J == 0) return CREG_OK;
    hipLaunchKernelGGL(k_joint_axes, dim3(J), dim3(JA_NT), 0, (hipStream_t)stream, coords, S, T, K, link_clusters,
                       link_offsets, n_link_clusters, joints, start_step, num_steps, interval, NS / S, NS, sample_axis,
                       sample_angle, sample_point, sample_usable, local_axis, local_pos, global_pos, global_axis, count,
                       first_pose);
    CREG_LAUNCH_CHECK();
    return CREG_OK;
}

extern "C" int creg_link_clouds_f64(const double* coords, const double* matrices, int32_t T, int32_t K,
                                    const int32_t* link_clusters, const int32_t* link_offsets, int32_t n_link_clusters,
                                    int32_t L, const double* points, const int64_t* point_offsets, int64_t n_points,
                                    const int64_t* out_offsets, int64_t n_out, int64_t max_link_rows, float* link_matrices,
                                    float* mean_matrices, double* clouds_wf, double* clouds_lf, creg_stream_t stream) {
    CREG_REQUIRE(coords && matrices && link_clusters && link_offsets && point_offsets && out_offsets && link_matrices,
                 "creg_link_clouds_f64: null pointer");
    CREG_REQUIRE(T >= 1 && K >= 1 && K <= JOINT_MAX_K && L >= 1 && L <= K && n_link_clusters >= 1 && n_points >= 0 && n_out >= 0,
                 "creg_link_clouds_f64: bad size (T=%d, K=%d, L=%d; K <= %d)", T, K, L, JOINT_MAX_K);
    CREG_REQUIRE((n_points == 0 || points) && (n_out == 0 || (clouds_wf && clouds_lf)), "creg_link_clouds_f64: null cloud");
    CREG_REQUIRE(max_link_rows >= 0, "creg_link_clouds_f64: max_link_rows < 0");
    const int64_t slices = (max_link_rows + LC_ROWS - 1) / LC_ROWS;
    const int G = slices < 1 ? 1 : (slices > LC_MAX_SLICES ? LC_MAX_SLICES : (int)slices);
    hipLaunchKernelGGL(k_link_clouds, dim3(T * L, G), dim3(LC_NT), 0, (hipStream_t)stream, coords, matrices, T, K, L,
                       link_clusters, link_offsets, n_link_clusters, points, point_offsets, n_points, out_offsets, n_out,
                       link_matrices, mean_matrices, clouds_wf, clouds_lf);
    CREG_LAUNCH_CHECK();
    return CREG_OK;
}
