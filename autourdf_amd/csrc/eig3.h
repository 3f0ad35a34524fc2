// eig3.h -- symmetric 3x3 eigenvector of the smallest eigenvalue (device, fp64), shared by the normal estimation
// (normals.hip) and the plane fits of the RANSAC segmentation (depth.hip).
#pragma once
#include <hip/hip_runtime.h>

namespace creg {

__device__ __forceinline__ void cross3(const double* a, const double* b, double* o) {
    o[0] = a[1] * b[2] - a[2] * b[1]; o[1] = a[2] * b[0] - a[0] * b[2]; o[2] = a[0] * b[1] - a[1] * b[0];
}
// unit eigenvector of A for eigenvalue ev from the largest of the three row cross products of A - ev I
__device__ inline void eigvec_by_rows(const double A[6], double ev, double* v) {   // A = (a00, a01, a02, a11, a12, a22)
    const double r0[3] = {A[0] - ev, A[1], A[2]}, r1[3] = {A[1], A[3] - ev, A[4]}, r2[3] = {A[2], A[4], A[5] - ev};
    double c01[3], c02[3], c12[3];
    cross3(r0, r1, c01); cross3(r0, r2, c02); cross3(r1, r2, c12);
    const double d0 = c01[0] * c01[0] + c01[1] * c01[1] + c01[2] * c01[2];
    const double d1 = c02[0] * c02[0] + c02[1] * c02[1] + c02[2] * c02[2];
    const double d2 = c12[0] * c12[0] + c12[1] * c12[1] + c12[2] * c12[2];
    const double* c = c01; double dm = d0;
    if (d1 > dm) { dm = d1; c = c02; }
    if (d2 > dm) { dm = d2; c = c12; }
    const double inv = dm > 0 ? 1.0 / sqrt(dm) : 0.0;
    v[0] = c[0] * inv; v[1] = c[1] * inv; v[2] = c[2] * inv;
}
// second eigenvector (eigenvalue ev1) in the plane orthogonal to the unit eigenvector e0
__device__ inline void eigvec_deflated(const double A[6], const double* e0, double ev1, double* v) {
    double U[3], V[3];
    if (fabs(e0[0]) > fabs(e0[1])) { const double il = 1.0 / sqrt(e0[0] * e0[0] + e0[2] * e0[2]); U[0] = -e0[2] * il; U[1] = 0; U[2] = e0[0] * il; }
    else { const double il = 1.0 / sqrt(e0[1] * e0[1] + e0[2] * e0[2]); U[0] = 0; U[1] = e0[2] * il; U[2] = -e0[1] * il; }
    cross3(e0, U, V);
    const double AU[3] = {A[0] * U[0] + A[1] * U[1] + A[2] * U[2], A[1] * U[0] + A[3] * U[1] + A[4] * U[2], A[2] * U[0] + A[4] * U[1] + A[5] * U[2]};
    const double AV[3] = {A[0] * V[0] + A[1] * V[1] + A[2] * V[2], A[1] * V[0] + A[3] * V[1] + A[4] * V[2], A[2] * V[0] + A[4] * V[1] + A[5] * V[2]};
    double m00 = U[0] * AU[0] + U[1] * AU[1] + U[2] * AU[2] - ev1, m01 = U[0] * AV[0] + U[1] * AV[1] + U[2] * AV[2],
           m11 = V[0] * AV[0] + V[1] * AV[1] + V[2] * AV[2] - ev1;
    const double a00 = fabs(m00), a01 = fabs(m01), a11 = fabs(m11);
    double cu, cv;                                      // v = cu U + cv V in the null space of the 2x2 [[m00, m01], [m01, m11]]
    if (a00 >= a11) {
        if (fmax(a00, a01) > 0) {
            if (a00 >= a01) { m01 /= m00; m00 = 1.0 / sqrt(1.0 + m01 * m01); m01 *= m00; } else { m00 /= m01; m01 = 1.0 / sqrt(1.0 + m00 * m00); m00 *= m01; }
            cu = m01; cv = -m00;
        } else { cu = 1; cv = 0; }
    } else {
        if (fmax(a11, a01) > 0) {
            if (a11 >= a01) { m01 /= m11; m11 = 1.0 / sqrt(1.0 + m01 * m01); m01 *= m11; } else { m11 /= m01; m01 = 1.0 / sqrt(1.0 + m11 * m11); m11 *= m01; }
            cu = m11; cv = -m01;
        } else { cu = 1; cv = 0; }
    }
    for (int a = 0; a < 3; ++a) v[a] = cu * U[a] + cv * V[a];
}
// unit eigenvector of the SMALLEST eigenvalue of the symmetric 3x3 C = (c00, c01, c02, c11, c12, c22); zero vector for C = 0
__device__ inline void smallest_eigvec(const double Cin[6], double* nrm) {
    double mx = 0;
    for (int i = 0; i < 6; ++i) mx = fmax(mx, fabs(Cin[i]));
    if (!(mx > 0)) { nrm[0] = nrm[1] = nrm[2] = 0; return; }
    double A[6];
    for (int i = 0; i < 6; ++i) A[i] = Cin[i] / mx;
    const double off2 = A[1] * A[1] + A[2] * A[2] + A[4] * A[4];
    if (off2 > 0) {
        const double q = (A[0] + A[3] + A[5]) / 3.0;
        const double b00 = A[0] - q, b11 = A[3] - q, b22 = A[5] - q;
        const double p = sqrt((b00 * b00 + b11 * b11 + b22 * b22 + 2.0 * off2) / 6.0);
        const double c00 = b11 * b22 - A[4] * A[4], c01 = A[1] * b22 - A[4] * A[2], c02 = A[1] * A[4] - b11 * A[2];
        const double det = (b00 * c00 - A[1] * c01 + A[2] * c02) / (p * p * p);
        const double hd = fmin(fmax(det * 0.5, -1.0), 1.0);
        const double ang = acos(hd) / 3.0;
        const double beta2 = cos(ang) * 2.0, beta0 = cos(ang + 2.09439510239319549) * 2.0, beta1 = -(beta0 + beta2);
        const double e0 = q + p * beta0, e1 = q + p * beta1, e2 = q + p * beta2;        // e0 <= e1 <= e2
        if (hd >= 0) {                                  // e2 is the well-separated one: start there, deflate, finish by a cross product
            double v2[3], v1[3];
            eigvec_by_rows(A, e2, v2);
            eigvec_deflated(A, v2, e1, v1);
            cross3(v1, v2, nrm);
        } else eigvec_by_rows(A, e0, nrm);
    } else {                                            // diagonal matrix: the axis of the smallest entry; z whenever z is among the
        // smallest, y when only x and y tie (`<=` below: z there would be the LARGEST eigenvalue's axis, e.g. for an exact line
        // along z, C = diag(0, 0, c))
        nrm[0] = (A[0] < A[3] && A[0] < A[5]) ? 1.0 : 0.0;
        nrm[1] = (nrm[0] == 0.0 && A[3] <= A[0] && A[3] < A[5]) ? 1.0 : 0.0;
        nrm[2] = (nrm[0] == 0.0 && nrm[1] == 0.0) ? 1.0 : 0.0;
    }
}

// All three eigenpairs of the symmetric 3x3 A = (a00, a01, a02, a11, a12, a22) by cyclic Jacobi rotations: w ascending, row k of
// V (row-major 3x3) the unit eigenvector of w[k], its largest component positive for k = 0, 1 and row 2 = row 0 x row 1.
// smallest_eigvec's closed form keeps half the digits of two nearly equal eigenvalues (acos near +-1), which every symmetric
// body has; rotations keep all of them.  Eight sweeps of (0,1), (0,2), (1,2), a zero pivot skipped; a NaN in A gives NaNs.
__device__ inline void sym3_eig_jacobi(const double A[6], double* w, double* V) {
    double a[3][3] = {{A[0], A[1], A[2]}, {A[1], A[3], A[4]}, {A[2], A[4], A[5]}};
    double v[3][3] = {{1, 0, 0}, {0, 1, 0}, {0, 0, 1}};         // columns: eigenvectors
    for (int sweep = 0; sweep < 8; ++sweep) {
#pragma unroll
        for (int pq = 0; pq < 3; ++pq) {
            const int p = pq == 2 ? 1 : 0, q = pq == 0 ? 1 : 2, r = 3 - p - q;
            const double apq = a[p][q];
            if (apq == 0.0) continue;
            const double theta = (a[q][q] - a[p][p]) / (2.0 * apq);
            const double t = (theta < 0.0 ? -1.0 : 1.0) / (fabs(theta) + sqrt(theta * theta + 1.0));
            const double c = 1.0 / sqrt(t * t + 1.0), s = t * c;
            a[p][p] = a[p][p] - t * apq;
            a[q][q] = a[q][q] + t * apq;
            a[p][q] = a[q][p] = 0.0;
            const double arp = a[r][p], arq = a[r][q];
            a[r][p] = a[p][r] = c * arp - s * arq;
            a[r][q] = a[q][r] = s * arp + c * arq;
#pragma unroll
            for (int k = 0; k < 3; ++k) {
                const double vkp = v[k][p], vkq = v[k][q];
                v[k][p] = c * vkp - s * vkq;
                v[k][q] = s * vkp + c * vkq;
            }
        }
    }
    int o0 = 0, o1 = 1, o2 = 2, tmp;                             // ascending, ties keep their column order
    if (a[o1][o1] < a[o0][o0]) { tmp = o0; o0 = o1; o1 = tmp; }
    if (a[o2][o2] < a[o1][o1]) { tmp = o1; o1 = o2; o2 = tmp; }
    if (a[o1][o1] < a[o0][o0]) { tmp = o0; o0 = o1; o1 = tmp; }
    const int order[3] = {o0, o1, o2};
    for (int k = 0; k < 3; ++k) {
        const int col = order[k];
        w[k] = a[col][col];
        double e[3] = {v[0][col], v[1][col], v[2][col]};
        int big = fabs(e[1]) > fabs(e[0]) ? 1 : 0;
        if (fabs(e[2]) > fabs(e[big])) big = 2;
        const double sign = e[big] < 0.0 ? -1.0 : 1.0;
        for (int i = 0; i < 3; ++i) V[3 * k + i] = sign * e[i];
    }
    cross3(V, V + 3, V + 6);
}

}  // namespace creg
