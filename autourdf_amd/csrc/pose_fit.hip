// pose_fit.hip -- the Gauss-Newton system of fitting a URDF's base pose and joint values to clouds, fp64: from the correspondences
// of creg_point_mesh_f64 (every point's nearest triangle, hence its link), per pose the normal equations H = sum J^T J, g = sum J^T r,
// the cost sum r.r and the number of contributing points.  The driver on top of it (compute_joints.fit_cloud_poses, SimEnv.fit_pose)
// poses the robot with creg_urdf_fk_f64, finds the correspondences with creg_point_mesh_f64, calls this entry and solves the damped
// system on the device.  The contract is in include/creg.h in full; in short
//   frames      per pose, once: W_j = link_T[p, parent[j]] * origin[j] (affine 3x4), o_j = W_j[:3,3], a_j = W_j[:3,:3] axis[j]
//   point i     contributes iff live, 0 <= f = tri_idx[i] < n_tri, row f in a link l's rows, dot(r, r) <= d_max^2, where r is
//               pt_tri_vec of mesh_dist.h against the row's three vertices posed in the thread by pose_tri of mesh_pair.h, the
//               posing stage's formula, so dot(r, r) has the bits of creg_point_mesh_f64's dist2 (matched_row of point_rows.h,
//               which link_moments.hip calls too); c = p_i - r
//   columns     e_k x (c - center_p) | e_k | a_j x (c - o_j) (revolute) or a_j (prismatic) where bit j of chain[l] is set, else 0
//
// Passes (PF_TILE = 32 points):
//   k_pose_fit_frames   one thread per (pose, joint): o_j | a_j into the workspace
//   k_pose_fit_tiles    one launch, 256 threads, one block per (pose, tile of 32 of that pose's points), found by find_tile of
//                       point_rows.h: block b belongs to the pose p with the largest (pt_start[p] >> 5) + p not above b.  Lanes 0 .. 31
//                       compute r, c and the link of the tile's points while the other threads fetch the pose's frames into LDS; then
//                       all 256 threads fill the tile's 32 x D x 3 Jacobian in LDS ([point][column][xyz]: consecutive lanes write
//                       consecutive columns, 24 bytes apart, no bank conflict), and thread e, e + 256, ... sums entry e of H | g | cost
//                       | n over the tile's points 0 .. 31 in ascending order (every thread reads the same point at once: column b
//                       at a stride of 24 bytes, column a mostly a broadcast) into the tile's slot of the workspace.  A point that
//                       does not contribute, and a row past the pose's end, has r = 0 and J = 0: its terms are exact zeros.  H's
//                       upper triangle is summed and stored to both halves.
//   k_pose_fit_finish   thread per (pose, entry): the pose's tile partials in ascending tile order into four running sums (tile t
//                       into sum t mod 4), result (s0 + s1) + (s2 + s3): tile_sum4 of point_rows.h.
// No atomics.  The order of every sum is a function of the pose's own row count alone: two runs give the same bits, and a pose alone in
// a call gives the bits it has among others.  fp64 VALU work with partials in LDS and in the workspace; the Jacobian of a tile is
// 3 x D x 32 doubles, 48 KiB at D = 64 (dynamic LDS, 52.6 KiB in all at D = 64, 8.6 KiB at the toy robot's D = 10).  Nothing here has
// the shape of an MFMA product worth forcing: K = 32 x 3 per tile against D x D outputs that are reduced again across tiles.
#include "point_rows.h"

namespace creg {

constexpr int PF_SHIFT = 5, PF_TILE = 1 << PF_SHIFT;
constexpr int PF_MAX_D = 64;

__global__ __launch_bounds__(64) void k_pose_fit_frames(const double* __restrict__ link_T, int L, int64_t P, const int* __restrict__ parent,
                                                        const int* __restrict__ child, const double* __restrict__ origin,
                                                        const double* __restrict__ axis, int J, double* __restrict__ frames) {
    const int64_t at = (int64_t)blockIdx.x * 64 + threadIdx.x;
    if (at >= P * J) return;
    const int64_t p = at / J;
    const int j = (int)(at % J);
    double* out = frames + (size_t)at * 6;
    const int pa = parent[j], ch = child[j];
    if (pa < 0 || pa >= L || ch < 0 || ch >= L) {                // the joint the forward kinematics skips: no link has its bit
#pragma unroll
        for (int k = 0; k < 6; ++k) out[k] = 0.0;
        return;
    }
    const double* T = link_T + ((size_t)p * L + pa) * 16;
    const double* O = origin + (size_t)j * 16;
    double W[12];
#pragma unroll
    for (int r = 0; r < 3; ++r) {
#pragma unroll
        for (int c = 0; c < 4; ++c) {
            double v = (T[4 * r] * O[c] + T[4 * r + 1] * O[4 + c]) + T[4 * r + 2] * O[8 + c];
            if (c == 3) v += T[4 * r + 3];
            W[4 * r + c] = v;
        }
    }
    const double a0 = axis[3 * j], a1 = axis[3 * j + 1], a2 = axis[3 * j + 2];
#pragma unroll
    for (int r = 0; r < 3; ++r) {
        out[r] = W[4 * r + 3];
        out[3 + r] = (W[4 * r] * a0 + W[4 * r + 1] * a1) + W[4 * r + 2] * a2;
    }
}

__global__ __launch_bounds__(256) void k_pose_fit_tiles(const double* __restrict__ tri, const int64_t* __restrict__ tri_start, int64_t F,
                                                        const double* __restrict__ link_T, int L, const double* __restrict__ pts,
                                                        const int64_t* __restrict__ pt_start, int64_t N, int64_t P, double dmax2,
                                                        const int32_t* __restrict__ tri_idx, const int* __restrict__ type, int J,
                                                        const unsigned long long* __restrict__ chain, const double* __restrict__ center,
                                                        const double* __restrict__ frames, double* __restrict__ part) {
    extern __shared__ double s_mem[];
    const int D = 6 + J, DD = D * D, E = DD + D + 2;
    double* s_J = s_mem;                                         // [PF_TILE][D][3]
    double* s_r = s_J + PF_TILE * D * 3;                         // [PF_TILE][3], zero where the point does not contribute
    double* s_c = s_r + PF_TILE * 3;                             // [PF_TILE][3]
    double* s_f = s_c + PF_TILE * 3;                             // [J][6]: o_j | a_j
    int* s_link = (int*)(s_f + J * 6);                           // [PF_TILE]: the point's link, -1 where it does not contribute
    int* s_type = s_link + PF_TILE;                              // [J]
    const int tid = threadIdx.x;
    const int64_t blk = blockIdx.x;
    int64_t p, ps, pe, tile;                                     // the same for every thread
    if (!find_tile<PF_SHIFT>(pt_start, N, P, blk, p, ps, pe, tile)) return;
    if (tid < PF_TILE) {
        const int64_t i = ps + tile * PF_TILE + tid;
        double r[3] = {0.0, 0.0, 0.0}, c[3] = {0.0, 0.0, 0.0};
        int link = -1;
        if (i < pe) {
            double x[3];
#pragma unroll
            for (int k = 0; k < 3; ++k) x[k] = pts[(size_t)i * 3 + k];
            matched_row(tri, tri_start, F, link_T, L, p, x, tri_idx[i], dmax2, [&](int l, const double* rr, double) {
                link = l;
#pragma unroll
                for (int k = 0; k < 3; ++k) { r[k] = rr[k]; c[k] = x[k] - rr[k]; }
            });
        }
#pragma unroll
        for (int k = 0; k < 3; ++k) { s_r[tid * 3 + k] = r[k]; s_c[tid * 3 + k] = c[k]; }
        s_link[tid] = link;
    } else {
        for (int at = tid - PF_TILE; at < J * 6; at += 256 - PF_TILE) s_f[at] = frames[(size_t)p * J * 6 + at];
        for (int at = tid - PF_TILE; at < J; at += 256 - PF_TILE) s_type[at] = type[at];
    }
    __syncthreads();
    // ---- the tile's Jacobian
    const double c0 = center[(size_t)p * 3], c1 = center[(size_t)p * 3 + 1], c2 = center[(size_t)p * 3 + 2];
    for (int at = tid; at < PF_TILE * D; at += 256) {
        const int pt = at / D, k = at - pt * D;
        const int l = s_link[pt];
        double o[3] = {0.0, 0.0, 0.0};
        if (l >= 0) {
            const double* c = s_c + pt * 3;
            if (k < 3) {
                const double v[3] = {c[0] - c0, c[1] - c1, c[2] - c2};
                if (k == 0) { o[1] = -v[2]; o[2] = v[1]; }
                else if (k == 1) { o[0] = v[2]; o[2] = -v[0]; }
                else { o[0] = -v[1]; o[1] = v[0]; }
            } else if (k < 6) {
                o[k - 3] = 1.0;
            } else {
                const int j = k - 6;
                const int ty = s_type[j];
                if (((chain[l] >> j) & 1ull) != 0ull && (ty == 1 || ty == 2)) {
                    const double* fr = s_f + j * 6;
                    if (ty == 1) {
                        const double v[3] = {c[0] - fr[0], c[1] - fr[1], c[2] - fr[2]};
                        o[0] = fr[4] * v[2] - fr[5] * v[1];
                        o[1] = fr[5] * v[0] - fr[3] * v[2];
                        o[2] = fr[3] * v[1] - fr[4] * v[0];
                    } else {
                        o[0] = fr[3]; o[1] = fr[4]; o[2] = fr[5];
                    }
                }
            }
        }
        double* dst = s_J + (size_t)at * 3;
        dst[0] = o[0]; dst[1] = o[1]; dst[2] = o[2];
    }
    __syncthreads();
    // ---- the tile's partial of every entry: points 0 .. 31 in ascending order
    double* out = part + (size_t)blk * E;
    for (int e = tid; e < E; e += 256) {
        double s = 0.0;
        if (e < DD) {
            const int a = e / D, b = e - a * D;
            if (a > b) continue;                                 // written by the thread of (b, a)
            for (int pt = 0; pt < PF_TILE; ++pt) s += dot3(s_J + (pt * D + a) * 3, s_J + (pt * D + b) * 3);
            out[e] = s;
            out[b * D + a] = s;
        } else if (e < DD + D) {
            const int a = e - DD;
            for (int pt = 0; pt < PF_TILE; ++pt) s += dot3(s_J + (pt * D + a) * 3, s_r + pt * 3);
            out[e] = s;
        } else if (e == DD + D) {
            for (int pt = 0; pt < PF_TILE; ++pt) s += dot3(s_r + pt * 3, s_r + pt * 3);
            out[e] = s;
        } else {
            for (int pt = 0; pt < PF_TILE; ++pt) s += s_link[pt] >= 0 ? 1.0 : 0.0;
            out[e] = s;
        }
    }
}

__global__ __launch_bounds__(256) void k_pose_fit_finish(const int64_t* __restrict__ pt_start, int64_t N, int D, int chunks,
                                                         const double* __restrict__ part, double* __restrict__ H, double* __restrict__ g,
                                                         double* __restrict__ cost, int64_t* __restrict__ n) {
    const int DD = D * D, E = DD + D + 2;
    const int64_t p = blockIdx.x / chunks;
    const int e = (int)(blockIdx.x % chunks) * 256 + threadIdx.x;
    if (e >= E) return;
    int64_t ps, pe;
    pose_rows(pt_start, p, N, ps, pe);
    const int64_t tiles = (pe - ps + PF_TILE - 1) / PF_TILE;
    const double v = tile_sum4(part + (size_t)tile_slot<PF_SHIFT>(pt_start, p, N) * E + e, E, tiles);
    if (e < DD) H[(size_t)p * DD + e] = v;
    else if (e < DD + D) g[(size_t)p * D + (e - DD)] = v;
    else if (e == DD + D) cost[p] = v;
    else n[p] = (int64_t)v;
}

struct PoseFitLayout { size_t frames, part, end; int64_t blocks; int E; };
static inline bool pose_fit_counts_ok(int64_t n_poses, int64_t n_pts, int32_t n_joints) {
    return n_poses >= 1 && n_pts >= 0 && n_pts < (1ll << 31) && n_joints >= 0 && 6 + n_joints <= PF_MAX_D &&
           (n_pts >> PF_SHIFT) + n_poses < (1ll << 31);
}
static inline PoseFitLayout pose_fit_layout(int64_t n_poses, int64_t n_pts, int32_t n_joints) {
    PoseFitLayout w;
    const int D = 6 + n_joints;
    w.E = D * D + D + 2;
    w.blocks = (n_pts >> PF_SHIFT) + n_poses;               // past the last tile slot in use
    w.frames = 0;
    w.part = align_up(w.frames + sizeof(double) * 6 * (size_t)n_poses * (size_t)n_joints, 256);
    w.end = align_up(w.part + sizeof(double) * (size_t)w.blocks * (size_t)w.E, 256);
    return w;
}

}  // namespace creg
using namespace creg;

extern "C" size_t creg_pose_fit_workspace_bytes(int64_t n_poses, int64_t n_pts, int32_t n_joints) {
    if (!pose_fit_counts_ok(n_poses, n_pts, n_joints)) return 0;
    return pose_fit_layout(n_poses, n_pts, n_joints).end;
}

extern "C" int creg_pose_fit_system_f64(const double* tri, const int64_t* tri_start, int64_t n_tri, const double* link_T, int32_t n_links,
                                        int64_t n_poses, const double* pts, const int64_t* pt_start, int64_t n_pts, double d_max,
                                        const int32_t* tri_idx, const int32_t* parent, const int32_t* child, const int32_t* type,
                                        const double* origin, const double* axis, int32_t n_joints, const uint64_t* chain,
                                        const double* center, double* H, double* g, double* cost, int64_t* n, void* workspace,
                                        size_t workspace_bytes, creg_stream_t stream) {
    const char* who = "creg_pose_fit_system_f64";
    if (const int rc = point_query_check(who, d_max, n_pts, n_poses, PF_SHIFT, pt_start, chain && center && H && g && cost && n,
                                         "chain, center, H, g, cost or n", pts && tri_idx, "pts / tri_idx"))
        return rc;
    CREG_REQUIRE(n_joints >= 0 && 6 + n_joints <= PF_MAX_D, "%s: 0 <= n_joints and D = 6 + n_joints <= %d (got n_joints %d)", who,
                 PF_MAX_D, (int)n_joints);
    const PoseFitLayout w = pose_fit_layout(n_poses, n_pts, n_joints);
    if (const int rc = mesh_pair_check(who, tri, tri_start, n_tri, link_T, n_links, n_poses, nullptr, 0, nullptr, nullptr,
                                       "tri_idx", workspace, workspace_bytes, w.end))
        return rc;
    CREG_REQUIRE(n_joints == 0 || (parent && child && type && origin && axis), "%s: null joint table with n_joints %d", who, (int)n_joints);
    const int D = 6 + n_joints;
    const int chunks = (w.E + 255) / 256;
    CREG_REQUIRE(n_poses * chunks < (1ll << 31) && n_poses * (int64_t)n_joints < (1ll << 36), "%s: too many poses (%lld)", who, (long long)n_poses);
    hipStream_t s = (hipStream_t)stream;
    char* ws = (char*)workspace;
    double* frames = (double*)(ws + w.frames);
    double* part = (double*)(ws + w.part);
    if (n_joints > 0) {
        hipLaunchKernelGGL(k_pose_fit_frames, dim3((unsigned)((n_poses * n_joints + 63) / 64)), dim3(64), 0, s, link_T, (int)n_links, n_poses,
                           parent, child, origin, axis, (int)n_joints, frames);
        CREG_LAUNCH_CHECK();
    }
    if (n_pts > 0) {
        const size_t lds = sizeof(double) * ((size_t)PF_TILE * D * 3 + PF_TILE * 6 + (size_t)n_joints * 6) + sizeof(int) * (PF_TILE + (size_t)n_joints);
        hipLaunchKernelGGL(k_pose_fit_tiles, dim3((unsigned)w.blocks), dim3(256), lds, s, tri, tri_start, n_tri, link_T, (int)n_links, pts,
                           pt_start, n_pts, n_poses, d_max * d_max, tri_idx, type, (int)n_joints, (const unsigned long long*)chain, center,
                           (const double*)frames, part);
        CREG_LAUNCH_CHECK();
    }
    hipLaunchKernelGGL(k_pose_fit_finish, dim3((unsigned)(n_poses * chunks)), dim3(256), 0, s, pt_start, n_pts, D, chunks,
                       (const double*)part, H, g, cost, n);
    CREG_LAUNCH_CHECK();
    return CREG_OK;
}
