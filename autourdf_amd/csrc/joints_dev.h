// joints_dev.h -- device helpers of the URDF stage's pose arithmetic, fp64, shared by joints.hip (joint axes, link clouds),
// joint_types.hip (joint kinds) and joint_motion.hip (link poses, joint positions, slides): the top eigenvector by cyclic Jacobi, a link's mean pose
// (get_cluster_pose_mean), the child's pose in the parent's frame, a link's span of the flat cluster list and the
// enumeration of a joint's samples, which joint_types.hip shares with joints.hip.
// quat_to_matrix is creg_dev.h's, which this header brings in.
#pragma once
#include <cstdint>
#include "creg_dev.h"

namespace creg {

// Top eigenvector of a symmetric N x N matrix (cyclic Jacobi, fp64, registers).  Ties: the first largest diagonal.
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

}  // namespace creg
