// link_moments.hip -- the 16 moment sums per (pose, link) that every rigid-twist least-squares problem over the correspondences of
// creg_point_mesh_f64 is a small product around, fp64: restricted to the points of one link, every column of such a problem (base
// pose, joint value, joint frame) is a twist field Omega x (c - rho) + V, so the normal system H, g, cost follows from
//   sum d d^T (6) | sum d (3) | sum d x r (3) | sum r (3) | sum r.r (1),  d = c - ref[p, l],  and the count
// whatever the parameter count is (compute_joints.twist_system assembles it in torch; compute_joints.refine_joint_frames is the
// bundle adjustment on top).  The contract is in include/creg.h in full; contributes, r and c are those of
// creg_pose_fit_system_f64 by the same function (matched_row of point_rows.h), so dot(r, r) has the bits of creg_point_mesh_f64's dist2.
//
// Passes (LM_TILE = 64 points, LM_E = 17 entries: the 16 sums and the count as a double):
//   k_link_moments_tiles   one launch, 256 threads, one block per (pose, tile of 64 of that pose's rows), found by find_tile of
//                          point_rows.h.  Wave 0 computes r, c, the link and the row's 17 terms into LDS ([row][17]: a row's terms
//                          are 136 bytes apart, and the readers below take consecutive entries of one row).  Then thread (l, e),
//                          l over ALL links, sums entry e over the tile's rows 0 .. 63 in ascending order, skipping the rows of
//                          other links, into the tile slot's partial [slot][l][e]: a link absent from the tile gets exact zeros, so
//                          the finishing pass needs no list of present links.  4.4 KiB of LDS.
//   k_link_moments_finish  thread per (pose, link, entry): the pose's tile partials in ascending tile order into four running sums
//                          (tile t into sum t mod 4), result (s0 + s1) + (s2 + s3): tile_sum4.  Adding the +0.0 of a tile without the link
//                          changes no bit (a running sum starts from +0.0 and never becomes -0.0).
// No atomics.  The order of every sum is a function of the pose's own row count and of which rows belong to the link: two runs give
// the same bits, a pose alone in a call gives the bits it has among others, and the rows of other links do not enter.  fp64 VALU work;
// no MFMA shape is hidden in 17 running sums.
#include "point_rows.h"

namespace creg {

constexpr int LM_SHIFT = 6, LM_TILE = 1 << LM_SHIFT;
constexpr int LM_E = 17;

__global__ __launch_bounds__(256) void k_link_moments_tiles(const double* __restrict__ tri, const int64_t* __restrict__ tri_start, int64_t F,
                                                            const double* __restrict__ link_T, int L, const double* __restrict__ pts,
                                                            const int64_t* __restrict__ pt_start, int64_t N, int64_t P, double dmax2,
                                                            const int32_t* __restrict__ tri_idx, const double* __restrict__ ref,
                                                            double* __restrict__ part) {
    __shared__ double s_term[LM_TILE * LM_E];                    // [row][entry]
    __shared__ int s_link[LM_TILE];                              // the row's link, -1 where it does not contribute
    const int tid = threadIdx.x;
    const int64_t blk = blockIdx.x;
    int64_t p, ps, pe, tile;                                     // the same for every thread
    if (!find_tile<LM_SHIFT>(pt_start, N, P, blk, p, ps, pe, tile)) return;
    if (tid < LM_TILE) {
        const int64_t i = ps + tile * LM_TILE + tid;
        int link = -1;
        double t[LM_E];
#pragma unroll
        for (int k = 0; k < LM_E; ++k) t[k] = 0.0;
        if (i < pe) {
            double x[3];
#pragma unroll
            for (int k = 0; k < 3; ++k) x[k] = pts[(size_t)i * 3 + k];
            matched_row(tri, tri_start, F, link_T, L, p, x, tri_idx[i], dmax2, [&](int l, const double* r, double rr) {
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
                t[16] = 1.0;
            });
        }
#pragma unroll
        for (int k = 0; k < LM_E; ++k) s_term[tid * LM_E + k] = t[k];
        s_link[tid] = link;
    }
    __syncthreads();
    // ---- the tile's partial of every (link, entry): rows 0 .. 63 in ascending order, the rows of other links skipped
    double* out = part + (size_t)blk * L * LM_E;
    for (int at = tid; at < L * LM_E; at += 256) {
        const int l = at / LM_E, e = at - l * LM_E;
        double s = 0.0;
        for (int row = 0; row < LM_TILE; ++row)
            if (s_link[row] == l) s += s_term[row * LM_E + e];
        out[at] = s;
    }
}

__global__ __launch_bounds__(256) void k_link_moments_finish(const int64_t* __restrict__ pt_start, int64_t N, int64_t P, int L,
                                                             const double* __restrict__ part, double* __restrict__ mom,
                                                             int64_t* __restrict__ cnt) {
    const int64_t at = (int64_t)blockIdx.x * 256 + threadIdx.x;
    const int64_t per_pose = (int64_t)L * LM_E;
    if (at >= P * per_pose) return;
    const int64_t p = at / per_pose;
    const int64_t le = at - p * per_pose;                        // l * LM_E + e
    const int64_t l = le / LM_E;
    const int e = (int)(le - l * LM_E);
    int64_t ps, pe;
    pose_rows(pt_start, p, N, ps, pe);
    const int64_t tiles = (pe - ps + LM_TILE - 1) / LM_TILE;
    const size_t E = (size_t)per_pose;
    const double v = tile_sum4(part + (size_t)tile_slot<LM_SHIFT>(pt_start, p, N) * E + le, E, tiles);
    if (e < 16) mom[((size_t)p * L + l) * 16 + e] = v;
    else cnt[(size_t)p * L + l] = (int64_t)v;
}

static inline bool link_moments_counts_ok(int64_t n_poses, int64_t n_pts, int32_t n_links) {
    return n_poses >= 1 && n_pts >= 0 && n_pts < (1ll << 31) && n_links >= 1 && n_links <= 65535 &&
           (n_pts >> LM_SHIFT) + n_poses < (1ll << 31);
}
static inline int64_t link_moments_blocks(int64_t n_poses, int64_t n_pts) { return (n_pts >> LM_SHIFT) + n_poses; }   // past the last slot in use
static inline size_t link_moments_bytes(int64_t n_poses, int64_t n_pts, int32_t n_links) {
    return align_up(sizeof(double) * (size_t)link_moments_blocks(n_poses, n_pts) * (size_t)n_links * LM_E, 256);
}

}  // namespace creg
using namespace creg;

extern "C" size_t creg_link_moments_workspace_bytes(int64_t n_poses, int64_t n_pts, int32_t n_links) {
    if (!link_moments_counts_ok(n_poses, n_pts, n_links)) return 0;
    return link_moments_bytes(n_poses, n_pts, n_links);
}

extern "C" int creg_link_moments_f64(const double* tri, const int64_t* tri_start, int64_t n_tri, const double* link_T, int32_t n_links,
                                     int64_t n_poses, const double* pts, const int64_t* pt_start, int64_t n_pts, double d_max,
                                     const int32_t* tri_idx, const double* ref, double* mom, int64_t* cnt, void* workspace,
                                     size_t workspace_bytes, creg_stream_t stream) {
    const char* who = "creg_link_moments_f64";
    if (const int rc = point_query_check(who, d_max, n_pts, n_poses, LM_SHIFT, pt_start, ref && mom && cnt, "ref, mom or cnt",
                                         pts && tri_idx, "pts / tri_idx"))
        return rc;
    CREG_REQUIRE(n_links >= 1 && n_links <= 65535, "%s: 1 <= n_links <= 65535 (got %d)", who, (int)n_links);
    const size_t need = link_moments_bytes(n_poses, n_pts, n_links);
    if (const int rc = mesh_pair_check(who, tri, tri_start, n_tri, link_T, n_links, n_poses, nullptr, 0, nullptr, nullptr,
                                       "tri_idx", workspace, workspace_bytes, need))
        return rc;
    const int64_t finish_blocks = (n_poses * (int64_t)n_links * LM_E + 255) / 256;
    CREG_REQUIRE(finish_blocks < (1ll << 31), "%s: too many (pose, link) pairs (%lld x %d)", who, (long long)n_poses, (int)n_links);
    hipStream_t s = (hipStream_t)stream;
    double* part = (double*)workspace;
    if (n_pts > 0) {
        hipLaunchKernelGGL(k_link_moments_tiles, dim3((unsigned)link_moments_blocks(n_poses, n_pts)), dim3(256), 0, s, tri, tri_start, n_tri,
                           link_T, (int)n_links, pts, pt_start, n_pts, n_poses, d_max * d_max, tri_idx, ref, part);
        CREG_LAUNCH_CHECK();
    }
    hipLaunchKernelGGL(k_link_moments_finish, dim3((unsigned)finish_blocks), dim3(256), 0, s, pt_start, n_pts, n_poses, (int)n_links,
                       (const double*)part, mom, cnt);
    CREG_LAUNCH_CHECK();
    return CREG_OK;
}
