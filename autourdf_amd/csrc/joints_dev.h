// joints_dev.h -- what the joint part of the URDF stage shares, fp64: joints.hip (joint axes, link clouds), joint_types.hip
// (joint kinds) and joint_motion.hip (link poses, joint positions, slides, motion error) all start from here, and so does
// a new joint kind.  Limits of the stage (ops.py holds the same figures for its own checks); the top eigenvector by cyclic
// Jacobi; a link's mean pose (get_cluster_pose_mean); the child's pose in the parent's frame; a link's span of the flat
// cluster list; sin(angle) axis, cos(angle) and |.| of a rotation matrix, whose bits every angle of the stage has; the
// enumeration of a joint's samples and the relative motion of one of them, which k_joint_axes and k_joint_types both
// classify.  The host side of those two entries shares its argument checks in joints_host.h.
// quat_to_matrix is creg_dev.h's, which this header brings in.
#pragma once
#include <cstdint>
#include "creg_dev.h"

namespace creg {

// ops.py repeats these as LINK_SWEEP_MAX_K, JOINT_MAX_SAMPLES and JOINT_THETA_MIN for the checks it makes before a launch.
constexpr int JOINT_MAX_K = 256;             // clusters per pose table
constexpr int JOINT_MAX_SAMPLES = 4096;      // samples per joint of k_joint_axes / k_joint_types
constexpr double JOINT_THETA_MIN = 2e-4;     // see creg.h: below ~1.4e-4 rad the reference's own 4x4 eigen test breaks down

// Top eigenvector of a symmetric N x N matrix (cyclic Jacobi, fp64, registers).  Ties: the first largest diagonal.
// A matrix with an entry that is not finite gives NaN.
template <int N>
__device__ void jacobi_top(double A[N][N], double v[N]) {
    double V[N][N];
#pragma unroll
    for (int i = 0; i < N; ++i)
#pragma unroll
        for (int j = 0; j < N; ++j) V[i][j] = i == j ? 1.0 : 0.0;
    for (int sweep = 0; sweep < 16; ++sweep) {
        double off = 0.0, diag = 0.0;
#pragma unroll
        for (int p = 0; p < N; ++p) {
            diag += A[p][p] * A[p][p];
#pragma unroll
            for (int q = p + 1; q < N; ++q) off += A[p][q] * A[p][q];
        }
        if (!isfinite(off + diag)) {                      // a NaN or Inf entry: no eigenvector, not the unit vector the
#pragma unroll
            for (int i = 0; i < N; ++i) v[i] = NAN;       // comparisons below would pick from the untouched V
            return;
        }
        if (!(off > 1e-36 * diag)) break;
#pragma unroll
        for (int p = 0; p < N; ++p)
#pragma unroll
            for (int q = p + 1; q < N; ++q) {
                const double apq = A[p][q];
                if (apq == 0.0) continue;
                const double th = (A[q][q] - A[p][p]) / (2.0 * apq);
                const double t = (th >= 0.0 ? 1.0 : -1.0) / (fabs(th) + sqrt(th * th + 1.0));
                const double c = 1.0 / sqrt(t * t + 1.0), s = t * c;
#pragma unroll
                for (int k = 0; k < N; ++k) {
                    const double akp = A[k][p], akq = A[k][q];
                    A[k][p] = c * akp - s * akq;
                    A[k][q] = s * akp + c * akq;
                }
#pragma unroll
                for (int k = 0; k < N; ++k) {
                    const double apk = A[p][k], aqk = A[q][k];
                    A[p][k] = c * apk - s * aqk;
                    A[q][k] = s * apk + c * aqk;
                }
#pragma unroll
                for (int k = 0; k < N; ++k) {
                    const double vkp = V[k][p], vkq = V[k][q];
                    V[k][p] = c * vkp - s * vkq;
                    V[k][q] = s * vkp + c * vkq;
                }
            }
    }
    int b = 0;
#pragma unroll
    for (int i = 1; i < N; ++i)
        if (A[i][i] > A[b][b]) b = i;
#pragma unroll
    for (int i = 0; i < N; ++i) v[i] = V[i][b];
}

// get_cluster_pose_mean of one link at one step: mean xyz, average quaternion, and its rotation matrix (fp64).
// Sums run in the list's order, as numpy's axis-0 reductions and the outer-product loop do.
__device__ inline void link_mean_pose(const double* __restrict__ step, int K, const int32_t* __restrict__ idx, int n,
                               double pos[3], double q[4], double R[9]) {
    double x = 0.0, y = 0.0, z = 0.0, A[4][4];
#pragma unroll
    for (int a = 0; a < 4; ++a)
#pragma unroll
        for (int b = 0; b < 4; ++b) A[a][b] = 0.0;
    for (int c = 0; c < n; ++c) {
        const int k = idx[c];
        if (k < 0 || k >= K) continue;                    // the host rejects these; never read out of range
        const double* p = step + (size_t)k * 7;
        x += p[0]; y += p[1]; z += p[2];
        const double qq[4] = {p[3], p[4], p[5], p[6]};
#pragma unroll
        for (int a = 0; a < 4; ++a)
#pragma unroll
            for (int b = 0; b < 4; ++b) A[a][b] += qq[a] * qq[b];
    }
    const double dn = (double)n;
    pos[0] = x / dn; pos[1] = y / dn; pos[2] = z / dn;
#pragma unroll
    for (int a = 0; a < 4; ++a)
#pragma unroll
        for (int b = 0; b < 4; ++b) A[a][b] /= dn;
    jacobi_top<4>(A, q);
    quat_to_matrix(q, R);
}

// Child pose in the parent's frame: X = P^-1 C (rigid inverse; R_P is orthonormal to rounding).
__device__ inline void child_in_parent(const double tp[3], const double Rp[9], const double tc[3], const double Rc[9],
                                double t[3], double R[9]) {
    const double d[3] = {tc[0] - tp[0], tc[1] - tp[1], tc[2] - tp[2]};
#pragma unroll
    for (int r = 0; r < 3; ++r) {
        t[r] = (Rp[r] * d[0] + Rp[3 + r] * d[1]) + Rp[6 + r] * d[2];
#pragma unroll
        for (int c = 0; c < 3; ++c) R[3 * r + c] = (Rp[r] * Rc[c] + Rp[3 + r] * Rc[3 + c]) + Rp[6 + r] * Rc[6 + c];
    }
}

struct LinkSpan {
    const int32_t* idx;
    int n;
};

__device__ inline LinkSpan link_span(const int32_t* cl, const int32_t* off, int n_cl, int l) {
    int a = off[l], b = off[l + 1];
    a = a < 0 ? 0 : (a > n_cl ? n_cl : a);
    b = b < a ? a : (b > n_cl ? n_cl : b);
    return {cl + a, b - a};
}

// sin(angle) axis and cos(angle) of a rotation matrix: v = vee of the skew part, c = (trace - 1) / 2
__device__ inline void skew_and_cos(const double R[9], double v[3], double& c) {
    v[0] = (R[7] - R[5]) * 0.5; v[1] = (R[2] - R[6]) * 0.5; v[2] = (R[3] - R[1]) * 0.5;
    c = (((R[0] + R[4]) + R[8]) - 1.0) * 0.5;
}

__device__ inline double norm3(const double v[3]) { return sqrt((v[0] * v[0] + v[1] * v[1]) + v[2] * v[2]); }

// Sample r of a sequence -> (step_prev, step): phases a = 0..interval-1, then steps, as the reference's loops.
__device__ inline void sample_steps(int r, int start, int num_steps, int interval, int& i0, int& i1) {
    for (int a = 0; a < interval; ++a) {
        const int na = a < num_steps ? (num_steps - a + interval - 1) / interval : 0;
        const int ns = na > 1 ? na - 1 : 0;
        if (r < ns) {
            i1 = start + a + (r + 1) * interval;
            i0 = i1 - interval;
            return;
        }
        r -= ns;
    }
    i0 = i1 = start;                                      // unreachable: r < samples per sequence
}

// Relative motion [R t] = X_{i-1}^-1 X_i of sample i of a joint (sequence-major, then sample_steps' order), with
// X = P^-1 C the child link's mean pose in the parent's frame: the reference's T_r1.
__device__ inline void joint_sample_motion(const double* __restrict__ coords, int T, int K, LinkSpan P, LinkSpan C, int i,
                                           int per_seq, int start, int num_steps, int interval, double t[3], double R[9]) {
    const int seq = i / per_seq;
    int i0, i1;
    sample_steps(i - seq * per_seq, start, num_steps, interval, i0, i1);
    const double* c0 = coords + ((size_t)seq * T + i0) * K * 7;
    const double* c1 = coords + ((size_t)seq * T + i1) * K * 7;
    double tp0[3], tc0[3], tp1[3], tc1[3], Rp0[9], Rc0[9], Rp1[9], Rc1[9], q[4];
    link_mean_pose(c0, K, P.idx, P.n, tp0, q, Rp0);
    link_mean_pose(c0, K, C.idx, C.n, tc0, q, Rc0);
    link_mean_pose(c1, K, P.idx, P.n, tp1, q, Rp1);
    link_mean_pose(c1, K, C.idx, C.n, tc1, q, Rc1);
    double x0t[3], x0R[9], x1t[3], x1R[9];
    child_in_parent(tp0, Rp0, tc0, Rc0, x0t, x0R);
    child_in_parent(tp1, Rp1, tc1, Rc1, x1t, x1R);
    child_in_parent(x0t, x0R, x1t, x1R, t, R);
}

}  // namespace creg
