// feature_moments.hip -- link_moments.hip's 16 sums and count per (pose, link), and beside them the 21 sums of the curvature of the
// matched feature, fp64: half the squared distance to a flat feature (a vertex, an edge's line, a face's plane) has an exact Hessian,
// the projector Pi onto the feature's normal space -- I, I - t t^T, n n^T.  Pi r = r, so the gradient, the cost and every reported
// figure of a fit are those of the 16 sums; only the curvature H = sum J^T Pi J differs from the point-to-point sum J^T J, and
// restricted to one link it is again a 6 x 6 matrix between twists:
//   M6 = sum A^T Pi A,  A = [e_0 x d, e_1 x d, e_2 x d, e_0, e_1, e_2],  d = c - ref[p, l]          (upper triangle, 21 sums)
// (compute_joints.twist_system(fmom=...) puts it between the twist tables; fit_cloud_poses and refine_joint_frames take it with
// metric="feature").  The contract is in include/creg.h in full under "Feature moments"; contributes, r, c and the link are those of
// creg_link_moments_f64 by the same function (matched_feature_row of point_rows.h, which also hands out pt_tri_vec's case and the posed
// vertices), and the first 16 terms and the count are link_moments.hip's text, so mom and cnt have that entry's bits.
//
// Passes (FM_TILE = 64 points, FM_E = 38 entries: the 16 sums, the 21 sums and the count as a double), the shape of link_moments.hip:
//   k_feature_moments_tiles   one launch, 256 threads, one block per (pose, tile of 64 of that pose's rows), found by find_tile.  Wave
//                             0 computes r, c, the link, Pi and the row's 38 terms into LDS ([row][38], 19 KiB: a row's terms are 304
//                             bytes apart, so the 38 stores of that wave are two-way bank conflicts, and the readers below, which
//                             are the loop, take consecutive entries of one row without any).  Then thread (l, e), l over ALL links,
//                             sums entry e over the tile's rows 0 .. 63 in ascending order, skipping the rows of other links, into
//                             the tile slot's partial [slot][l][e]; a link absent from the tile gets exact zeros.
//   k_feature_moments_finish  thread per (pose, link, entry): tile_sum4 over the pose's tile partials.
// No atomics.  The order of every sum is a function of the pose's own row count and of which rows belong to the link, as in
// link_moments.hip.  Pi takes + - x / only (no square root), so a numpy restatement has the kernel's bits term by term.
#include "point_rows.h"

namespace creg {

constexpr int FM_SHIFT = 6, FM_TILE = 1 << FM_SHIFT;
constexpr int FM_MOM = 16, FM_F = 21;
constexpr int FM_E = FM_MOM + FM_F + 1;                          // 38

// Pi (xx xy xz yy yz zz) of the feature pt_tri_vec named, from the posed vertices w = a | b | c
__device__ __forceinline__ void feature_projector(int which, const double* w, double* pi) {
    pi[0] = 1.0; pi[1] = 0.0; pi[2] = 0.0; pi[3] = 1.0; pi[4] = 0.0; pi[5] = 1.0;
    if (which < 4) return;                                       // a vertex
    double u[3], v[3];
#pragma unroll
    for (int k = 0; k < 3; ++k) { u[k] = w[3 + k] - w[k]; v[k] = w[6 + k] - w[k]; }              // b - a, c - a
    if (which == 7) {                                            // the face: N N^T / N.N
        const double n[3] = {u[1] * v[2] - u[2] * v[1], u[2] * v[0] - u[0] * v[2], u[0] * v[1] - u[1] * v[0]};
        const double nn = dot3(n, n);
        if (nn > 0.0) {
            pi[0] = (n[0] * n[0]) / nn; pi[1] = (n[0] * n[1]) / nn; pi[2] = (n[0] * n[2]) / nn;
            pi[3] = (n[1] * n[1]) / nn; pi[4] = (n[1] * n[2]) / nn; pi[5] = (n[2] * n[2]) / nn;
        }
        return;
    }
    double e[3];                                                 // an edge: I - e e^T / e.e
#pragma unroll
    for (int k = 0; k < 3; ++k) e[k] = which == 4 ? u[k] : (which == 5 ? v[k] : w[6 + k] - w[3 + k]);
    const double ee = dot3(e, e);
    if (ee > 0.0) {
        pi[0] = 1.0 - (e[0] * e[0]) / ee; pi[1] = 0.0 - (e[0] * e[1]) / ee; pi[2] = 0.0 - (e[0] * e[2]) / ee;
        pi[3] = 1.0 - (e[1] * e[1]) / ee; pi[4] = 0.0 - (e[1] * e[2]) / ee; pi[5] = 1.0 - (e[2] * e[2]) / ee;
    }
}

__global__ __launch_bounds__(256) void k_feature_moments_tiles(const double* __restrict__ tri, const int64_t* __restrict__ tri_start,
                                                               int64_t F, const double* __restrict__ link_T, int L,
                                                               const double* __restrict__ pts, const int64_t* __restrict__ pt_start,
                                                               int64_t N, int64_t P, double dmax2, const int32_t* __restrict__ tri_idx,
                                                               const double* __restrict__ ref, double* __restrict__ part) {
    __shared__ double s_term[FM_TILE * FM_E];                    // [row][entry]
    __shared__ int s_link[FM_TILE];                              // the row's link, -1 where it does not contribute
    const int tid = threadIdx.x;
    const int64_t blk = blockIdx.x;
    int64_t p, ps, pe, tile;                                     // the same for every thread
    if (!find_tile<FM_SHIFT>(pt_start, N, P, blk, p, ps, pe, tile)) return;
    if (tid < FM_TILE) {
        const int64_t i = ps + tile * FM_TILE + tid;
        int link = -1;
        double t[FM_E];
#pragma unroll
        for (int k = 0; k < FM_E; ++k) t[k] = 0.0;
        if (i < pe) {
            double x[3];
#pragma unroll
            for (int k = 0; k < 3; ++k) x[k] = pts[(size_t)i * 3 + k];
            matched_feature_row(tri, tri_start, F, link_T, L, p, x, tri_idx[i], dmax2,
                                [&](int l, const double* r, double rr, int which, const double* w) {
                link = l;
                const double* rf = ref + ((size_t)p * L + l) * 3;
                double d[3];
#pragma unroll
                for (int k = 0; k < 3; ++k) d[k] = (x[k] - r[k]) - rf[k];
                t[0] = d[0] * d[0]; t[1] = d[0] * d[1]; t[2] = d[0] * d[2];
                t[3] = d[1] * d[1]; t[4] = d[1] * d[2]; t[5] = d[2] * d[2];
                t[6] = d[0]; t[7] = d[1]; t[8] = d[2];
                t[9] = d[1] * r[2] - d[2] * r[1];
                t[10] = d[2] * r[0] - d[0] * r[2];
                t[11] = d[0] * r[1] - d[1] * r[0];
                t[12] = r[0]; t[13] = r[1]; t[14] = r[2];
                t[15] = rr;
                double pi[6];
                feature_projector(which, w, pi);
                const double Pi[3][3] = {{pi[0], pi[1], pi[2]}, {pi[1], pi[3], pi[4]}, {pi[2], pi[4], pi[5]}};
                // the six twist columns A_k and B_k = Pi A_k, component i a dot3 of Pi's row i with A_k (zeros included, as written)
                const double A[6][3] = {{0.0, -d[2], d[1]}, {d[2], 0.0, -d[0]}, {-d[1], d[0], 0.0},
                                        {1.0, 0.0, 0.0}, {0.0, 1.0, 0.0}, {0.0, 0.0, 1.0}};
                double B[6][3];
#pragma unroll
                for (int k = 0; k < 6; ++k)
#pragma unroll
                    for (int i3 = 0; i3 < 3; ++i3) B[k][i3] = dot3(Pi[i3], A[k]);
                int at = FM_MOM;
#pragma unroll
                for (int a = 0; a < 6; ++a)
#pragma unroll
                    for (int b = a; b < 6; ++b) t[at++] = dot3(A[a], B[b]);
                t[FM_E - 1] = 1.0;
            });
        }
#pragma unroll
        for (int k = 0; k < FM_E; ++k) s_term[tid * FM_E + k] = t[k];
        s_link[tid] = link;
    }
    __syncthreads();
    // ---- the tile's partial of every (link, entry): rows 0 .. 63 in ascending order, the rows of other links skipped
    double* out = part + (size_t)blk * L * FM_E;
    for (int at = tid; at < L * FM_E; at += 256) {
        const int l = at / FM_E, e = at - l * FM_E;
        double s = 0.0;
        for (int row = 0; row < FM_TILE; ++row)
            if (s_link[row] == l) s += s_term[row * FM_E + e];
        out[at] = s;
    }
}

__global__ __launch_bounds__(256) void k_feature_moments_finish(const int64_t* __restrict__ pt_start, int64_t N, int64_t P, int L,
                                                                const double* __restrict__ part, double* __restrict__ mom,
                                                                int64_t* __restrict__ cnt, double* __restrict__ fmom) {
    const int64_t at = (int64_t)blockIdx.x * 256 + threadIdx.x;
    const int64_t per_pose = (int64_t)L * FM_E;
    if (at >= P * per_pose) return;
    const int64_t p = at / per_pose;
    const int64_t le = at - p * per_pose;                        // l * FM_E + e
    const int64_t l = le / FM_E;
    const int e = (int)(le - l * FM_E);
    int64_t ps, pe;
    pose_rows(pt_start, p, N, ps, pe);
    const int64_t tiles = (pe - ps + FM_TILE - 1) / FM_TILE;
    const size_t E = (size_t)per_pose;
    const double v = tile_sum4(part + (size_t)tile_slot<FM_SHIFT>(pt_start, p, N) * E + le, E, tiles);
    if (e < FM_MOM) mom[((size_t)p * L + l) * FM_MOM + e] = v;
    else if (e < FM_MOM + FM_F) fmom[((size_t)p * L + l) * FM_F + (e - FM_MOM)] = v;
    else cnt[(size_t)p * L + l] = (int64_t)v;
}

static inline bool feature_moments_counts_ok(int64_t n_poses, int64_t n_pts, int32_t n_links) {
    return n_poses >= 1 && n_pts >= 0 && n_pts < (1ll << 31) && n_links >= 1 && n_links <= 65535 &&
           (n_pts >> FM_SHIFT) + n_poses < (1ll << 31);
}
static inline int64_t feature_moments_blocks(int64_t n_poses, int64_t n_pts) { return (n_pts >> FM_SHIFT) + n_poses; }   // past the last slot in use
static inline size_t feature_moments_bytes(int64_t n_poses, int64_t n_pts, int32_t n_links) {
    return align_up(sizeof(double) * (size_t)feature_moments_blocks(n_poses, n_pts) * (size_t)n_links * FM_E, 256);
}

}  // namespace creg
using namespace creg;

extern "C" size_t creg_feature_moments_workspace_bytes(int64_t n_poses, int64_t n_pts, int32_t n_links) {
    if (!feature_moments_counts_ok(n_poses, n_pts, n_links)) return 0;
    return feature_moments_bytes(n_poses, n_pts, n_links);
}

extern "C" int creg_feature_moments_f64(const double* tri, const int64_t* tri_start, int64_t n_tri, const double* link_T, int32_t n_links,
                                        int64_t n_poses, const double* pts, const int64_t* pt_start, int64_t n_pts, double d_max,
                                        const int32_t* tri_idx, const double* ref, double* mom, int64_t* cnt, double* fmom,
                                        void* workspace, size_t workspace_bytes, creg_stream_t stream) {
    const char* who = "creg_feature_moments_f64";
    if (const int rc = point_query_check(who, d_max, n_pts, n_poses, FM_SHIFT, pt_start, ref && mom && cnt && fmom,
                                         "ref, mom, cnt or fmom", pts && tri_idx, "pts / tri_idx"))
        return rc;
    CREG_REQUIRE(n_links >= 1 && n_links <= 65535, "%s: 1 <= n_links <= 65535 (got %d)", who, (int)n_links);
    const size_t need = feature_moments_bytes(n_poses, n_pts, n_links);
    if (const int rc = mesh_pair_check(who, tri, tri_start, n_tri, link_T, n_links, n_poses, nullptr, 0, nullptr, nullptr,
                                       "tri_idx", workspace, workspace_bytes, need))
        return rc;
    const int64_t finish_blocks = (n_poses * (int64_t)n_links * FM_E + 255) / 256;
    CREG_REQUIRE(finish_blocks < (1ll << 31), "%s: too many (pose, link) pairs (%lld x %d)", who, (long long)n_poses, (int)n_links);
    hipStream_t s = (hipStream_t)stream;
    double* part = (double*)workspace;
    if (n_pts > 0) {
        hipLaunchKernelGGL(k_feature_moments_tiles, dim3((unsigned)feature_moments_blocks(n_poses, n_pts)), dim3(256), 0, s, tri, tri_start,
                           n_tri, link_T, (int)n_links, pts, pt_start, n_pts, n_poses, d_max * d_max, tri_idx, ref, part);
        CREG_LAUNCH_CHECK();
    }
    hipLaunchKernelGGL(k_feature_moments_finish, dim3((unsigned)finish_blocks), dim3(256), 0, s, pt_start, n_pts, n_poses, (int)n_links, (const double*)part, mom, cnt, fmom);
    CREG_LAUNCH_CHECK();
    return CREG_OK;
}
