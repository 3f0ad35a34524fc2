// mesh_cover.hip -- the cloud fit's other direction, fp64: for every posed triangle of every pose in one call, the minimum squared
// distance to the pose's points, the point that attains it and the number of points within d_max.  Mesh surface that no point lies
// near shows here and nowhere in point_mesh.hip's direction (ops.mesh_cover, SimEnv.surface_coverage, compute_joints.cloud_cover).
// The contract is in include/creg.h in full; in short it is the transposed reduction of point_mesh.hip's gated matrix:
//   live, box gap, contributes, d2(i, f)   word for word those of creg_point_mesh_f64 (gap2, pt_tri2 of mesh_dist.h)
//   label(i)     pt_row ? pt_row[i] : (int32) i
//   result of row f   best = +inf, idx = -1, near = 0; every live point i of the pose to which f contributes replaces (best, idx) by
//                (d2, label) iff d2 < best || (d2 == best && idx >= 0 && label < idx), and near += (d2 < +inf && d2 <= d_max^2)
// so dist2 is the minimum, pt_idx the smallest label with exactly its bits and n_near the number of supporting points: a
// lexicographic minimum over (d2, label), hence a function of the pose's set of (point, label) pairs and of the posed mesh alone.
// Culling is by d_max alone, with the formula of the gate (the monotonicity argument at the top of clearance.hip): the box of a tile
// of 64 points against the 256-triangle chunk box, then the per-point gate against the triangle's exact box.  A block is one chunk,
// and a chunk box lies inside its link's box, so a test against the link box could skip nothing the chunk test keeps.
//
// Passes (CHUNK = 256 triangles, tile = 64 points):
//   posing stage        mesh_pose.hip, every pose slice: posed vertices (P,F,9), chunk boxes and link boxes into the workspace
//   k_cover_tile_boxes  one wave per tile slot (find_tile<6> of point_rows.h): the min / max box of the tile's live points into the
//                       workspace after the posing stage's prefix, the empty box (+inf | -inf) for a slot without live points
//   k_mesh_cover        256 threads, one block per (chunk slot of the posing stage, pose), poses in slices of 65535.  Block s finds
//                       the link l with the largest chunk_slot(start_l, l) not above s by bisection (the slots of distinct links
//                       never overlap, mesh_pair.h) and is chunk s - chunk_slot(start_l, l) of it; a slot no chunk uses leaves.
//                       Thread t holds triangle start_l + 256 chunk + t: nine posed coordinates, its exact box and (best, idx, near)
//                       in registers.  The block walks the pose's tiles in ascending order, skips (uniformly) a tile whose box is
//                       beyond d_max of the chunk box, and for a surviving tile wave 0 ballot-compacts the live points and their
//                       labels into LDS.  Every thread with a triangle then walks them at an LDS address its wave shares (a broadcast
//                       read; with copies narrower than a wave, below, 2 or 4 addresses per wave): the gate, pt_tri2, the lexicographic replace, the count.  A full chunk's triangle lives in one
//                       thread: no reduction across threads.  A chunk of at most 128 triangles (a small link, a link's last chunk)
//                       would leave most of the block idle while one wave walks every point, so its triangles are held 2 .. 16
//                       times, each copy walks every G-th staged point, and the copies' (d2, label, near) meet in LDS at the end:
//                       the lexicographic minimum again, and the sum.  No finishing pass, no workspace of its own.
// No atomics.  fp64 VALU work throughout; nothing here has the shape of a matrix product.
#include "point_rows.h"

namespace creg {

constexpr int MC_SHIFT = 6, MC_TILE = 1 << MC_SHIFT;             // points per tile: one box, one staging round

__global__ __launch_bounds__(64) void k_cover_tile_boxes(const double* __restrict__ pts, const int64_t* __restrict__ pt_start, int64_t N,
                                                         int64_t P, double* __restrict__ tile_box) {
    const int lane = threadIdx.x;
    Box b;
    box_empty(b);
    int64_t p, ps, pe, tile;                                     // the same for every lane
    if (find_tile<MC_SHIFT>(pt_start, N, P, blockIdx.x, p, ps, pe, tile)) {
        const int64_t i = ps + tile * MC_TILE + lane;
        if (i < pe) {
            double x[3];
#pragma unroll
            for (int k = 0; k < 3; ++k) x[k] = pts[(size_t)i * 3 + k];
            if (x[0] == x[0] && x[1] == x[1] && x[2] == x[2]) {
#pragma unroll
                for (int k = 0; k < 3; ++k) { b.lo[k] = x[k]; b.hi[k] = x[k]; }
            }
        }
    }
    box_wave_reduce(b);
    if (lane == 0) box_store(tile_box + (size_t)blockIdx.x * 6, b);
}

__global__ __launch_bounds__(256) void k_mesh_cover(const int64_t* __restrict__ tri_start, int64_t F, int L,
                                                    const double* __restrict__ pts, const int64_t* __restrict__ pt_start,
                                                    const int32_t* __restrict__ pt_row, int64_t N, int64_t p0,
                                                    const double* __restrict__ posed, const double* __restrict__ chunk_box,
                                                    int64_t n_slots, const double* __restrict__ tile_box, double dmax2,
                                                    double* __restrict__ dist2, int32_t* __restrict__ pt_idx,
                                                    int32_t* __restrict__ n_near) {
    __shared__ double s_x[3][MC_TILE];                           // the live points of the current tile, component-major
    __shared__ int32_t s_lab[MC_TILE];                           // their labels
    __shared__ int s_n;
    __shared__ double s_md[COL_CHUNK];                           // the groups' results of a short chunk, merged at the end
    __shared__ int32_t s_mi[COL_CHUNK], s_mn[COL_CHUNK];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int64_t slot = blockIdx.x, p = p0 + blockIdx.y;        // the same for every thread
    // ---- this block's link and chunk
    if (chunk_slot(clamped_start(tri_start, 0, F), 0) > slot) return;
    int lo = 0, up = L;                                          // chunk_slot(lo) <= slot < chunk_slot(up), with chunk_slot(L) = +inf
    while (up - lo > 1) {
        const int mid = lo + ((up - lo) >> 1);
        if (chunk_slot(clamped_start(tri_start, mid, F), mid) <= slot) lo = mid; else up = mid;
    }
    int64_t sl, el;
    link_rows(tri_start, lo, F, sl, el);
    const int64_t c = slot - chunk_slot(sl, lo);
    if (c >= (el - sl + COL_CHUNK - 1) / COL_CHUNK) return;      // a slot no chunk uses; uniform, before any barrier
    // ---- this thread's triangle, and its share of the points: a chunk of n <= 128 triangles (a link's last one, or all of a small
    // link) is held G = 256 / W times, W = n rounded up to a power of two and to 16 at least, and copy g walks the staged points
    // g, g + G, ...; the copies meet in LDS at the end.  G is the same for the whole block.
    const int64_t base = sl + c * COL_CHUNK;
    const int n_chunk = (int)(el - base < COL_CHUNK ? el - base : COL_CHUNK);
    int W = 16;
    while (W < n_chunk) W <<= 1;
    const int G = COL_CHUNK / W, tl = tid & (W - 1), g = tid / W;
    const int64_t f = base + tl;
    const bool has = tl < n_chunk;
    double w[9];
    Box tb;
    box_empty(tb);
    if (has) {
#pragma unroll
        for (int k = 0; k < 9; ++k) w[k] = posed[((size_t)p * F + f) * 9 + k];
        box_of_tri(w, tb);
    } else {
#pragma unroll
        for (int k = 0; k < 9; ++k) w[k] = 0.0;
    }
    Box cb;
    box_load(chunk_box + ((size_t)p * n_slots + slot) * 6, cb);  // slot < n_slots: the grid has n_slots blocks
    const bool gated = dmax2 < INFINITY;                         // with d_max = +inf every gate of a live point holds
    double best = INFINITY;
    int32_t idx = -1, near = 0;

    int64_t ps, pe;
    pose_rows(pt_start, p, N, ps, pe);
    const int64_t tiles = (pe - ps + MC_TILE - 1) / MC_TILE;
    const double* tbox_p = tile_box + (size_t)tile_slot<MC_SHIFT>(pt_start, p, N) * 6;
    for (int64_t t = 0; t < tiles; ++t) {
        Box ub;
        box_load(tbox_p + t * 6, ub);
        if (!(gap2(cb, ub) <= dmax2)) continue;                  // the same for every thread; a tile without live points leaves here when gated
        __syncthreads();                                         // the previous tile's readers of s_x / s_lab / s_n are done
        if (wave == 0) {
            const int64_t i = ps + t * MC_TILE + lane;
            double x[3] = {0.0, 0.0, 0.0};
            if (i < pe) {
#pragma unroll
                for (int k = 0; k < 3; ++k) x[k] = pts[(size_t)i * 3 + k];
            }
            const bool live = i < pe && x[0] == x[0] && x[1] == x[1] && x[2] == x[2];
            const unsigned long long m = __ballot(live);
            if (live) {
                const int at = __popcll(m & ((1ull << lane) - 1ull));
#pragma unroll
                for (int k = 0; k < 3; ++k) s_x[k][at] = x[k];
                s_lab[at] = pt_row ? pt_row[i] : (int32_t)i;
            }
            if (lane == 0) s_n = __popcll(m);
        }
        __syncthreads();
        if (!has) continue;                                      // no barrier follows inside this trip
        const int n = s_n;
        for (int j = g; j < n; j += G) {
            const double x[3] = {s_x[0][j], s_x[1][j], s_x[2][j]};
            if (gated) {
                Box mine;
#pragma unroll
                for (int k = 0; k < 3; ++k) { mine.lo[k] = x[k]; mine.hi[k] = x[k]; }
                if (!(gap2(tb, mine) <= dmax2)) continue;        // this triangle does not contribute to the point
            }
            const double d = pt_tri2(x, w, w + 3, w + 6);
            const int32_t lab = s_lab[j];
            if (d < best || (d == best && idx >= 0 && lab < idx)) { best = d; idx = lab; }
            near += (d < INFINITY && d <= dmax2) ? 1 : 0;
        }
    }
    if (G > 1) {                                                 // the same for every thread
        s_md[tid] = best;
        s_mi[tid] = idx;
        s_mn[tid] = near;
        __syncthreads();
        if (g == 0 && has) {
            for (int k = 1; k < G; ++k) {                        // the lexicographic minimum over (d2, label); an empty copy is (+inf, -1)
                const double od = s_md[k * W + tl];
                const int32_t oi = s_mi[k * W + tl];
                if (od < best || (od == best && oi >= 0 && (idx < 0 || oi < idx))) { best = od; idx = oi; }
                near += s_mn[k * W + tl];
            }
        }
    }
    if (g == 0 && has) {
        const size_t o = (size_t)p * F + f;
        dist2[o] = best;
        pt_idx[o] = idx;
        if (n_near) n_near[o] = near;
    }
}

}  // namespace creg
using namespace creg;

// n_poses * n_tri <= 2^56: the (pose, row) offsets and the posed vertices' byte offsets (72 each) stay inside 64 bits
static inline bool mesh_cover_counts_ok(int64_t n_tri, int32_t n_links, int64_t n_poses, int64_t n_pts) {
    return mesh_pair_counts_ok(n_tri, n_links, n_poses, 0) && n_links <= 65535 && n_pts >= 0 && n_pts < (1ll << 31) &&
           (n_pts >> MC_SHIFT) + n_poses < (1ll << 31) && (n_tri == 0 || n_poses <= (1ll << 56) / n_tri);
}
static inline size_t mesh_cover_tile_bytes(int64_t n_poses, int64_t n_pts) {
    return sizeof(double) * 6 * (size_t)((n_pts >> MC_SHIFT) + n_poses);     // 48 bytes per point-tile slot
}

extern "C" size_t creg_mesh_cover_workspace_bytes(int64_t n_tri, int32_t n_links, int64_t n_poses, int64_t n_pts) {
    if (!mesh_cover_counts_ok(n_tri, n_links, n_poses, n_pts)) return 0;
    return pose_layout(n_tri, n_links, n_poses).end + mesh_cover_tile_bytes(n_poses, n_pts);
}

extern "C" int creg_mesh_cover_f64(const double* tri, const int64_t* tri_start, int64_t n_tri, const double* link_T, int32_t n_links,
                                   int64_t n_poses, const double* pts, const int64_t* pt_start, const int32_t* pt_row, int64_t n_pts,
                                   double d_max, double* dist2, int32_t* pt_idx, int32_t* n_near, double* link_box, void* workspace,
                                   size_t workspace_bytes, creg_stream_t stream) {
    const char* who = "creg_mesh_cover_f64";
    if (const int rc = point_query_check(who, d_max, n_pts, n_poses, MC_SHIFT, pt_start, true, nullptr, pts != nullptr, "pts")) return rc;
    CREG_REQUIRE(n_tri <= 0 || n_poses <= (1ll << 56) / n_tri, "%s: n_poses * n_tri <= 2^56 (got %lld, %lld)", who, (long long)n_poses,
                 (long long)n_tri);
    const bool counts = mesh_cover_counts_ok(n_tri, n_links, n_poses, n_pts);   // false: mesh_pair_check names the count
    const PoseLayout w = pose_layout(counts ? n_tri : 0, counts ? n_links : 1, counts ? n_poses : 1);
    if (const int rc = mesh_pair_check(who, tri, tri_start, n_tri, link_T, n_links, n_poses, nullptr, 0, nullptr, nullptr,
                                       "dist2 / pt_idx", workspace, workspace_bytes, w.end + mesh_cover_tile_bytes(n_poses, n_pts)))
        return rc;
    CREG_REQUIRE(n_tri == 0 || (dist2 && pt_idx), "%s: null dist2 / pt_idx with n_tri %lld", who, (long long)n_tri);
    hipStream_t s = (hipStream_t)stream;
    char* ws = (char*)workspace;
    double* tile_box = (double*)(ws + w.end);
    const int64_t tile_slots = (n_pts >> MC_SHIFT) + n_poses;    // past the last tile slot in use
    hipLaunchKernelGGL(k_cover_tile_boxes, dim3((unsigned)tile_slots), dim3(64), 0, s, pts, pt_start, n_pts, n_poses, tile_box);
    CREG_LAUNCH_CHECK();
    for (int64_t p0 = 0; p0 < n_poses; p0 += 65535) {              // gridDim.y / .z hold at most 65535
        const unsigned np = (unsigned)std::min<int64_t>(n_poses - p0, 65535);
        if (const int rc = mesh_pose_launch(s, tri, tri_start, n_tri, link_T, n_links, p0, np, w, ws, link_box)) return rc;
        hipLaunchKernelGGL(k_mesh_cover, dim3((unsigned)w.n_slots, np), dim3(256), 0, s, tri_start, n_tri, (int)n_links, pts, pt_start,
                           pt_row, n_pts, p0, (const double*)(ws + w.posed), (const double*)(ws + w.chunk_box), w.n_slots,
                           (const double*)tile_box, d_max * d_max, dist2, pt_idx, n_near);
        CREG_LAUNCH_CHECK();
    }
    return CREG_OK;
}
