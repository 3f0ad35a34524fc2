// point_mesh.hip -- distance from points to a posed, articulated triangle mesh, fp64: for every point of every pose in one call, the
// minimum squared distance to the pose's triangles and the triangle that attains it.  The check of a written URDF against the raw
// clouds rests on it (ops.point_mesh_distance, SimEnv.surface_distance, compute_joints.cloud_fit).  The contract is in include/creg.h
// in full; in short, with the posed vertices and the exact min / max boxes of the posing stage (mesh_pose.hip) and gap2, pt_tri2 of
// mesh_dist.h (clearance's):
//   a point      is live iff none of its coordinates is NaN; its box is lo = hi = the point
//   triangle f   contributes to live point i of the same pose iff gap2(box_f, box_i) <= d_max * d_max
//   d2(i, f)     = pt_tri2(p_i; a, b, c), squared, no square root
//   result       best = +inf, idx = -1; the contributing triangles in ascending row order replace them when d2 < best
// so dist2 is the minimum and tri_idx the smallest row with exactly its bits.  By the monotonicity argument at the top of
// clearance.hip, culling by link box, 256-triangle chunk box and the union box of a tile of points with the same formula and the same
// d_max^2 drops no contributing triangle, and because "contributes" is part of the contract, culling changes no output.  Nothing is
// pruned by a running best: the computed d2 and the computed gap2 are different formulas.  d_max is the cull.
//
// Passes (CHUNK = 256 triangles, tile = PM_TILE = 64 points):
//   posing stage     mesh_pose.hip, every pose slice: posed vertices (P,F,9), chunk boxes and link boxes into the workspace
//   k_point_mesh     one launch, 256 threads, one block per (pose, tile of that pose's points): block b belongs to the pose p with
//                    the largest tile_slot(p) = (pt_start[p] >> 6) + p not above b (find_tile of point_rows.h, by bisection; the slots
//                    of distinct poses never overlap, as chunk_slot's), and to tile b - tile_slot(p) of it.  Lane l of each of the four waves holds
//                    point l of the tile and that wave's running (d2, idx) in registers.  The block forms the union box of its live
//                    points, walks the links and their chunks, skips those beyond d_max of the union box, ballot-compacts the
//                    surviving chunk's triangles within d_max of the union box into LDS as SoA (stable, so rows stay ascending), and
//                    wave w walks the survivors w, w + 4, ... at a wave-uniform LDS address (a broadcast read): the per-point gate,
//                    then pt_tri2, then a strict <.  At the end the four waves' (d2, idx) of a point meet in LDS: the smaller d2,
//                    the smaller row on equal bits -- the result of one ascending walk.  A tile of 64 keeps the union box tight and
//                    gives a cloud of a few thousand points per pose enough blocks to fill the card; a chunk's 256 triangles are
//                    still fetched and tested by 256 threads.
// No atomics.  A point's result is a function of its coordinates and its pose's mesh alone: not of the other points or poses of the
// call, their order, or scheduling.  fp64 VALU work throughout; nothing here has the shape of a matrix product.
#include "point_rows.h"

namespace creg {

constexpr int PM_SHIFT = 6, PM_TILE = 1 << PM_SHIFT;             // points per block: one per lane, the four waves split the triangles

__global__ __launch_bounds__(256) void k_point_mesh(const int64_t* __restrict__ tri_start, int64_t F, int L,
                                                    const double* __restrict__ pts, const int64_t* __restrict__ pt_start, int64_t N,
                                                    int64_t P, const double* __restrict__ posed, const double* __restrict__ chunk_box,
                                                    int64_t n_slots, const double* __restrict__ link_box, double dmax2,
                                                    double* __restrict__ dist2, int32_t* __restrict__ tri_idx) {
    __shared__ double s_t[9][COL_CHUNK];                         // kept triangles of the current chunk, component-major
    __shared__ int s_i[COL_CHUNK];                               // their rows in tri
    __shared__ double s_red[30];
    __shared__ int s_cnt[4];
    __shared__ double s_bd[4][PM_TILE];                          // the four waves' results, merged at the end
    __shared__ int s_bi[4][PM_TILE];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    int64_t p, ps, pe, tile;                                     // the same for every thread
    if (!find_tile<PM_SHIFT>(pt_start, N, P, blockIdx.x, p, ps, pe, tile)) return;
    // ---- this lane's point (the same in all four waves)
    const int64_t i = ps + tile * PM_TILE + lane;
    const bool has = i < pe;
    double x[3] = {0.0, 0.0, 0.0};
    if (has) {
#pragma unroll
        for (int k = 0; k < 3; ++k) x[k] = pts[(size_t)i * 3 + k];
    }
    const bool live = has && x[0] == x[0] && x[1] == x[1] && x[2] == x[2];
    Box mine;
    box_empty(mine);
    if (live) {
#pragma unroll
        for (int k = 0; k < 3; ++k) { mine.lo[k] = x[k]; mine.hi[k] = x[k]; }
    }
    Box uni = mine;
    box_block_reduce(uni, s_red);
    const bool gated = dmax2 < INFINITY;                         // with d_max = +inf every gate of a live point holds
    const double* cbox_p = chunk_box + (size_t)p * n_slots * 6;
    const double* posed_p = posed + (size_t)p * F * 9;
    double best = INFINITY;
    int32_t idx = -1;

    for (int l = 0; l < L; ++l) {
        Box lb;
        box_load(link_box + ((size_t)p * L + l) * 6, lb);
        if (!(gap2(lb, uni) <= dmax2)) continue;                 // the same for every thread; an empty link or tile leaves here
        int64_t sl, el;
        link_rows(tri_start, l, F, sl, el);
        const int64_t chunks = (el - sl + COL_CHUNK - 1) / COL_CHUNK;
        for (int64_t c = 0; c < chunks; ++c) {
            const int64_t slot = chunk_slot(sl, l) + c;
            Box cb;
            box_empty(cb);
            if (slot < n_slots) box_load(cbox_p + slot * 6, cb);
            if (!(gap2(cb, uni) <= dmax2)) continue;             // uniform
            const int64_t f = sl + c * COL_CHUNK + tid;
            double w[9];
            bool keep = false;
            if (f < el) {
                Box b;
#pragma unroll
                for (int k = 0; k < 9; ++k) w[k] = posed_p[(size_t)f * 9 + k];
                box_of_tri(w, b);
                keep = gap2(b, uni) <= dmax2;
            }
            __syncthreads();                                     // the previous chunk's readers of s_t / s_i / s_cnt are done
            int n;
            const int at = block_compact(keep, s_cnt, n);
            if (at >= 0) {
#pragma unroll
                for (int k = 0; k < 9; ++k) s_t[k][at] = w[k];
                s_i[at] = (int)f;
            }
            __syncthreads();
            if (!live) continue;                                 // no barrier follows inside this trip
            for (int j = wave; j < n; j += 4) {
                double T[9];
#pragma unroll
                for (int k = 0; k < 9; ++k) T[k] = s_t[k][j];
                if (gated) {
                    Box tb;
                    box_of_tri(T, tb);
                    if (!(gap2(tb, mine) <= dmax2)) continue;    // the triangle does not contribute to this point
                }
                const double d = pt_tri2(x, T, T + 3, T + 6);
                if (d < best) { best = d; idx = s_i[j]; }
            }
        }
    }
    // ---- the four waves' results of a point: smaller d2, then the smaller row
    s_bd[wave][lane] = best;
    s_bi[wave][lane] = idx;
    __syncthreads();
    if (wave == 0 && has) {
#pragma unroll
        for (int w = 1; w < 4; ++w) {
            const double od = s_bd[w][lane];
            const int oi = s_bi[w][lane];
            if (od < best || (od == best && oi >= 0 && (idx < 0 || oi < idx))) { best = od; idx = oi; }
        }
        dist2[i] = best;
        tri_idx[i] = idx;
    }
}

}  // namespace creg
using namespace creg;

static inline bool point_mesh_counts_ok(int64_t n_tri, int32_t n_links, int64_t n_poses, int64_t n_pts) {
    return mesh_pair_counts_ok(n_tri, n_links, n_poses, 0) && n_pts >= 0 && n_pts < (1ll << 31);
}

extern "C" size_t creg_point_mesh_workspace_bytes(int64_t n_tri, int32_t n_links, int64_t n_poses, int64_t n_pts) {
    if (!point_mesh_counts_ok(n_tri, n_links, n_poses, n_pts)) return 0;
    return pose_layout(n_tri, n_links, n_poses).end;
}

extern "C" int creg_point_mesh_f64(const double* tri, const int64_t* tri_start, int64_t n_tri, const double* link_T, int32_t n_links,
                                   int64_t n_poses, const double* pts, const int64_t* pt_start, int64_t n_pts, double d_max,
                                   double* dist2, int32_t* tri_idx, double* link_box, void* workspace, size_t workspace_bytes,
                                   creg_stream_t stream) {
    const char* who = "creg_point_mesh_f64";
    if (const int rc = point_query_check(who, d_max, n_pts, n_poses, PM_SHIFT, pt_start, true, nullptr, pts && dist2 && tri_idx,
                                         "pts / dist2 / tri_idx"))
        return rc;
    const PoseLayout w = pose_layout(n_tri, n_links, n_poses);
    if (const int rc = mesh_pair_check(who, tri, tri_start, n_tri, link_T, n_links, n_poses, nullptr, 0, nullptr, nullptr,
                                       "dist2 / tri_idx", workspace, workspace_bytes, w.end))
        return rc;
    const int64_t blocks = (n_pts >> PM_SHIFT) + n_poses;          // past the last tile slot in use
    hipStream_t s = (hipStream_t)stream;
    char* ws = (char*)workspace;
    for (int64_t p0 = 0; p0 < n_poses; p0 += 65535) {              // gridDim.y / .z hold at most 65535
        const unsigned np = (unsigned)std::min<int64_t>(n_poses - p0, 65535);
        if (const int rc = mesh_pose_launch(s, tri, tri_start, n_tri, link_T, n_links, p0, np, w, ws, link_box)) return rc;
    }
    if (n_pts > 0) {
        hipLaunchKernelGGL(k_point_mesh, dim3((unsigned)blocks), dim3(256), 0, s, tri_start, n_tri, (int)n_links, pts, pt_start, n_pts,
                           n_poses, (const double*)(ws + w.posed), (const double*)(ws + w.chunk_box), w.n_slots,
                           (const double*)(ws + w.link_box), d_max * d_max, dist2, tri_idx);
        CREG_LAUNCH_CHECK();
    }
    return CREG_OK;
}
