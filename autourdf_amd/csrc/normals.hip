// normals.hip -- the `--normal` branch of the reference (PointCloud/mlp_reg.py:190-192, cluster_icp.py:49-51):
//   pc.estimate_normals(search_param=KDTreeSearchParamHybrid(radius=0.1, max_nn=30))
//   pc.orient_normals_consistent_tangent_plane(30)
// open3d 0.18 is not vendored by the reference and absent from this image: what is restated here is its published
// behaviour.  estimate_normals: per point the (up to) max_nn nearest points with squared distance < radius^2 (the point
// itself included; KDTreeFlann::SearchHybrid = knnSearch + cut at the radius), their covariance from the nine raw moments
// (sum x, ..., sum zz) / count in neighbour order, the unit eigenvector of its smallest eigenvalue (Eberly's non-iterative
// symmetric 3x3 eigensolver: trigonometric eigenvalues of the scaled matrix, the best-conditioned eigenvector from row cross
// products, the others by deflation), (0,0,1) with fewer than three neighbours.  The sign of an eigenvector is the solver's
// business; orient_normals_consistent_tangent_plane fixes it afterwards (host: autourdf_amd/normals.py) and needs the k
// nearest neighbours of every point: the same search without the radius, exported as index lists.
//
// The search is exhaustive (n = 4096-16384 points per frame, once per frame): a block of KNN_Q queries, one thread each,
// sweeps the cloud through LDS tiles; a thread keeps its (distance, index)-sorted list of the max_nn best in LDS.
#include <cfloat>
#include "creg_common.h"
#include "creg_dev.h"
#include "eig3.h"

namespace creg {

constexpr int KNN_Q = 128;            // queries (threads) per block
constexpr int KNN_TILE = 512;         // candidates staged per LDS tile
constexpr int KNN_MAX = 32;           // most neighbours a list holds

// grid = ceil(n / KNN_Q) blocks of KNN_Q threads.  r2 < 0: no radius (plain k nearest).  idx_out (n, max_nn) / cnt_out (n)
// optional; normals (n,3) optional.
__global__ __launch_bounds__(KNN_Q) void k_knn_normals(const double* __restrict__ X, int n, double r2, int max_nn,
                                                       int* __restrict__ idx_out, int* __restrict__ cnt_out, double* __restrict__ normals) {
    extern __shared__ __attribute__((aligned(16))) char smem[];
    double* tile = (double*)smem;                                 // [KNN_TILE][3]
    double* ld = tile + 3 * KNN_TILE;                             // [KNN_MAX][KNN_Q] distances, list position major (no bank conflicts)
    int* li = (int*)(ld + KNN_MAX * KNN_Q);                       // [KNN_MAX][KNN_Q] indices
    const int tid = threadIdx.x, q = blockIdx.x * KNN_Q + tid;
    const bool live = q < n;
    const double qx = live ? X[3 * (size_t)q] : 0, qy = live ? X[3 * (size_t)q + 1] : 0, qz = live ? X[3 * (size_t)q + 2] : 0;
    int cnt = 0;
    double worst = r2 >= 0 ? r2 : DBL_MAX;                        // a candidate must beat this (strictly, like the radius cut) to enter
    for (int t0 = 0; t0 < n; t0 += KNN_TILE) {
        const int nt = min(KNN_TILE, n - t0);
        __syncthreads();
        for (int i = tid; i < 3 * nt; i += KNN_Q) tile[i] = X[3 * (size_t)t0 + i];
        __syncthreads();
        if (!live) continue;
        for (int j = 0; j < nt; ++j) {
            const double dx = tile[3 * j] - qx, dy = tile[3 * j + 1] - qy, dz = tile[3 * j + 2] - qz;
            const double d = dx * dx + dy * dy + dz * dz;
            if (cnt == max_nn ? !(d < worst) : !(r2 < 0 || d < r2)) continue;
            // insert (d, t0 + j) into the sorted list (ascending distance, then index: candidates arrive in index order, so an
            // equal distance goes BEHIND the entries already there)
            int p = cnt < max_nn ? cnt : max_nn - 1;
            while (p > 0 && ld[(p - 1) * KNN_Q + tid] > d) { ld[p * KNN_Q + tid] = ld[(p - 1) * KNN_Q + tid]; li[p * KNN_Q + tid] = li[(p - 1) * KNN_Q + tid]; --p; }
            ld[p * KNN_Q + tid] = d; li[p * KNN_Q + tid] = t0 + j;
            if (cnt < max_nn) ++cnt;
            if (cnt == max_nn) worst = ld[(max_nn - 1) * KNN_Q + tid];
        }
    }
    if (!live) return;
    if (cnt_out) cnt_out[q] = cnt;
    if (idx_out) for (int p = 0; p < max_nn; ++p) idx_out[(size_t)q * max_nn + p] = p < cnt ? li[p * KNN_Q + tid] : -1;
    if (!normals) return;
    double nv[3] = {0.0, 0.0, 1.0};
    if (cnt >= 3) {
        double m[9] = {0, 0, 0, 0, 0, 0, 0, 0, 0};
        for (int p = 0; p < cnt; ++p) {
            const int i = li[p * KNN_Q + tid];
            const double x = X[3 * (size_t)i], y = X[3 * (size_t)i + 1], z = X[3 * (size_t)i + 2];
            m[0] += x; m[1] += y; m[2] += z; m[3] += x * x; m[4] += x * y; m[5] += x * z; m[6] += y * y; m[7] += y * z; m[8] += z * z;
        }
        for (int a = 0; a < 9; ++a) m[a] /= (double)cnt;
        const double C[6] = {m[3] - m[0] * m[0], m[4] - m[0] * m[1], m[5] - m[0] * m[2], m[6] - m[1] * m[1], m[7] - m[1] * m[2], m[8] - m[2] * m[2]};
        smallest_eigvec(C, nv);
        const double l2 = nv[0] * nv[0] + nv[1] * nv[1] + nv[2] * nv[2];
        if (!(l2 > 0)) { nv[0] = 0; nv[1] = 0; nv[2] = 1; }
        else { const double il = 1.0 / sqrt(l2); nv[0] *= il; nv[1] *= il; nv[2] *= il; }
    }
    normals[3 * (size_t)q] = nv[0]; normals[3 * (size_t)q + 1] = nv[1]; normals[3 * (size_t)q + 2] = nv[2];
}

}  // namespace creg
using namespace creg;

extern "C" int creg_knn_normals_f64(const double* X, int64_t n, double radius, int32_t max_nn, int32_t* idx_out, int32_t* cnt_out,
                                    double* normals, creg_stream_t stream) {
    CREG_REQUIRE(n >= 1 && n < (1ll << 31) && max_nn >= 1 && max_nn <= KNN_MAX,
                 "creg_knn_normals_f64: needs 1 <= n < 2^31 and 1 <= max_nn <= %d (n = %lld, max_nn = %d)", KNN_MAX, (long long)n, (int)max_nn);
    CREG_REQUIRE(X && (idx_out || cnt_out || normals), "creg_knn_normals_f64: null pointer");
    const int smem = (int)(sizeof(double) * 3 * KNN_TILE + (sizeof(double) + sizeof(int)) * KNN_MAX * KNN_Q);
    hipLaunchKernelGGL(k_knn_normals, dim3(cdiv(n, KNN_Q)), dim3(KNN_Q), smem, (hipStream_t)stream, X, (int)n,
                       radius > 0 ? radius * radius : -1.0, (int)max_nn, idx_out, cnt_out, normals);
    CREG_LAUNCH_CHECK();
    return CREG_OK;
}
