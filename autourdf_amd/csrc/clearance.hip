// clearance.hip -- link clearance of an articulated triangle mesh, fp64: for every listed link pair of every pose in one call, the
// minimum squared distance between the two posed triangle meshes and the triangle pair that attains it.  The collision margin of the
// frame generator is built on it (SimEnv.clearance / collisions(margin=...)); collide.hip answers only yes or no.  The contract is in
// include/creg.h in full; in short, with the posed vertices and the exact min / max boxes of the posing stage (mesh_pose.hip):
//   gap2(a, b)     = (g_x^2 + g_y^2) + g_z^2,  g_k = max(0, max(lo_a[k] - hi_b[k], lo_b[k] - hi_a[k]))
//   triangle pair  contributes iff gap2(box_a, box_b) <= d_max * d_max
//   d2(a, b)       = 0 when the pair collides by the mesh-collide predicate (boxes meet and an edge properly pierces), else the
//                    minimum of 15 feature terms: 3 + 3 vertex-triangle (pt_tri2: Voronoi regions of the triangle) and 9 edge-edge
//                    (seg_seg2: clamped closest points of two segments); squared distances, no square root
//   result         the minimum of d2 over the contributing pairs and the lexicographically smallest (a, b) with exactly its bits
// Plain IEEE operations in the header's order (the library is built with -ffp-contract=off).  Floating-point subtraction, max,
// the square of a non-negative and a sum in a fixed order are all monotone, so in floating point the gap between two enclosing boxes
// never exceeds the gap between the boxes they enclose: culling by link box, 256-triangle chunk box and tile union box with the same
// formula and the same d_max^2 drops no contributing pair, and because "contributes" is part of the contract, culling changes no
// output.  Nothing is pruned by a running best: the computed d2 and the computed gap2 are different formulas.
//
// Passes (CHUNK = 256 triangles):
//   posing stage     mesh_pose.hip: posed vertices (P,F,9), chunk boxes and link boxes into the workspace
//   k_clear_pairs    grid (tile of link A, pair, pose), 256 threads, the shape of k_collide_pairs with every box_meet turned into
//                    gap2 <= d_max^2 (except the one inside "collides -> 0"): the tile's triangles within d_max of link B's box are
//                    ballot-compacted into LDS as SoA and their union box formed; link B is streamed chunk by chunk, chunks beyond
//                    d_max of the union box skipped, the others compacted into LDS.  Thread t owns A triangle t & (n2 - 1) and
//                    walks the B survivors with stride 256 / n2.  The nine edge-edge terms and the six vertex terms run in rolled
//                    loops over the LDS-resident vertices, so the branchy fp64 routines exist once in the code.  The thread's
//                    running (d2, key) -- smaller d2, then smaller key = a << 32 | b -- is reduced by wave shuffles, then over the
//                    four waves, and the block writes ONE partial into the slot (pose, pair, blockIdx.x); a block that leaves
//                    early writes the identity (+inf, ~0).  No floating-point atomics, no atomics at all.
//   k_clear_finish   one thread per (pose, pair): the lexicographic minimum over the at most 128 slots -> dist2, witness
// The minimum over a set does not depend on the order, so the outputs do not depend on scheduling or on the other pairs of a call.
// fp64 VALU work throughout; nothing here has the shape of a matrix product.
#include "mesh_dist.h"                                           // gap2, dot3 and pt_tri2, shared with point_mesh.hip

namespace creg {

__device__ __forceinline__ double clamp01(double x) { return x < 0.0 ? 0.0 : (x > 1.0 ? 1.0 : x); }

// squared distance of the segments (p1, q1) and (p2, q2): closest points clamped into both
__device__ __forceinline__ double seg_seg2(const double* p1, const double* q1, const double* p2, const double* q2) {
    double u[3], v[3], r[3], x[3];
#pragma unroll
    for (int k = 0; k < 3; ++k) { u[k] = q1[k] - p1[k]; v[k] = q2[k] - p2[k]; r[k] = p1[k] - p2[k]; }
    const double a = dot3(u, u), e = dot3(v, v), f = dot3(v, r), c = dot3(u, r), b = dot3(u, v);
    double s, t;
    if (a <= 0.0 && e <= 0.0) {                                             // two points
        s = 0.0;
        t = 0.0;
    } else if (a <= 0.0) {                                                  // the first is a point
        s = 0.0;
        t = clamp01(f / e);
    } else if (e <= 0.0) {                                                  // the second is a point
        t = 0.0;
        s = clamp01((0.0 - c) / a);
    } else {
        const double den = a * e - b * b;
        s = den > 0.0 ? clamp01((b * f - c * e) / den) : 0.0;               // parallel (or rounding made it so): any s will do
        t = (b * s + f) / e;
        if (t < 0.0) {
            t = 0.0;
            s = clamp01((0.0 - c) / a);
        } else if (t > 1.0) {
            t = 1.0;
            s = clamp01((b - c) / a);
        }
    }
#pragma unroll
    for (int k = 0; k < 3; ++k) x[k] = (p1[k] + u[k] * s) - (p2[k] + v[k] * t);
    return dot3(x, x);
}

constexpr unsigned long long CLEAR_NO_KEY = ~0ull;

__device__ __forceinline__ void best_take(double& d, unsigned long long& k, double od, unsigned long long ok) {
    if (od < d || (od == d && ok < k)) { d = od; k = ok; }
}

__global__ __launch_bounds__(256) void k_clear_pairs(const int64_t* __restrict__ tri_start, int64_t F, int L,
                                                     const int32_t* __restrict__ pairs, int64_t M, int64_t m0, int64_t p0,
                                                     const double* __restrict__ posed, const double* __restrict__ chunk_box,
                                                     int64_t n_slots, const double* __restrict__ link_box, double dmax2,
                                                     double* __restrict__ part_d, unsigned long long* __restrict__ part_k) {
    __shared__ double s_a[9][COL_CHUNK];                         // kept A triangles, component-major
    __shared__ double s_b[9][COL_CHUNK];                         // kept B triangles of the current chunk
    __shared__ double s_bb[6][COL_CHUNK];                        // their boxes
    __shared__ int s_ia[COL_CHUNK], s_ib[COL_CHUNK];             // their rows in tri, relative to the link's first
    __shared__ double s_red[30];
    __shared__ int s_cnt[4];
    __shared__ double s_pd[4];
    __shared__ unsigned long long s_pk[4];
    const int tid = threadIdx.x;
    const int64_t m = m0 + blockIdx.y, p = p0 + blockIdx.z;
    const size_t part = ((size_t)p * M + m) * gridDim.x + blockIdx.x;      // this block's slot: every block writes its own
    const int la = pairs[2 * m], lb = pairs[2 * m + 1];
    bool skip = la < 0 || la >= L || lb < 0 || lb >= L || la == lb;
    Box boxA, boxB;
    box_empty(boxA);
    box_empty(boxB);
    if (!skip) {
        box_load(link_box + ((size_t)p * L + la) * 6, boxA);
        box_load(link_box + ((size_t)p * L + lb) * 6, boxB);
        skip = !(gap2(boxA, boxB) <= dmax2);
    }
    if (skip) {                                                  // the same for every thread: +inf, (-1,-1) unless another block finds one
        if (tid == 0) { part_d[part] = INFINITY; part_k[part] = CLEAR_NO_KEY; }
        return;
    }
    int64_t sa, ea, sb, eb;
    link_rows(tri_start, la, F, sa, ea);
    link_rows(tri_start, lb, F, sb, eb);
    const int64_t tiles_a = (ea - sa + COL_CHUNK - 1) / COL_CHUNK, chunks_b = (eb - sb + COL_CHUNK - 1) / COL_CHUNK;
    const double* cbox_p = chunk_box + (size_t)p * n_slots * 6;
    const double* posed_p = posed + (size_t)p * F * 9;
    double my_d = INFINITY;
    unsigned long long my_key = CLEAR_NO_KEY;

    for (int64_t tile = blockIdx.x; tile < tiles_a; tile += gridDim.x) {
        const int64_t slot_a = chunk_slot(sa, la) + tile;
        Box tb;
        box_empty(tb);
        if (slot_a < n_slots) box_load(cbox_p + slot_a * 6, tb);
        if (!(gap2(tb, boxB) <= dmax2)) continue;                // the same for every thread
        // ---- the tile's triangles within d_max of link B's box
        const int64_t fa = sa + tile * COL_CHUNK + tid;
        double w[9];
        Box b;
        box_empty(b);
        bool keep = false;
        if (fa < ea) {
#pragma unroll
            for (int k = 0; k < 9; ++k) w[k] = posed_p[(size_t)fa * 9 + k];
            box_of_tri(w, b);
            keep = gap2(b, boxB) <= dmax2;
        }
        if (!keep) box_empty(b);
        __syncthreads();                                         // the previous tile's readers of s_a / s_cnt are done
        int nA;
        const int at = block_compact(keep, s_cnt, nA);
        if (at >= 0) {
#pragma unroll
            for (int k = 0; k < 9; ++k) s_a[k][at] = w[k];
            s_ia[at] = (int)(tile * COL_CHUNK + tid);
        }
        if (nA == 0) continue;                                   // uniform: nA comes from LDS
        Box uni = b;
        box_block_reduce(uni, s_red);                            // two barriers: s_a / s_ia are visible after it
        // ---- this thread's A triangle
        int sh = 0;
        while ((1 << sh) < nA) ++sh;
        const int n2 = 1 << sh, ia = tid & (n2 - 1), grp = tid >> sh, stride = COL_CHUNK >> sh;
        const bool live = ia < nA;
        double A[9];
        Box mine;
        box_empty(mine);
        long long rowA = 0;
#pragma unroll
        for (int k = 0; k < 9; ++k) A[k] = 0.0;
        if (live) {
#pragma unroll
            for (int k = 0; k < 9; ++k) A[k] = s_a[k][ia];
            box_of_tri(A, mine);
            rowA = (long long)(sa + s_ia[ia]);
        }
        // ---- link B, chunk by chunk
        for (int64_t c = 0; c < chunks_b; ++c) {
            const int64_t slot_b = chunk_slot(sb, lb) + c;
            Box cb;
            box_empty(cb);
            if (slot_b < n_slots) box_load(cbox_p + slot_b * 6, cb);
            if (!(gap2(cb, uni) <= dmax2)) continue;             // uniform
            const int64_t fb = sb + c * COL_CHUNK + tid;
            double v[9];
            Box bb;
            bool keep_b = false;
            if (fb < eb) {
#pragma unroll
                for (int k = 0; k < 9; ++k) v[k] = posed_p[(size_t)fb * 9 + k];
                box_of_tri(v, bb);
                keep_b = gap2(bb, uni) <= dmax2;
            }
            __syncthreads();                                     // the previous chunk's readers of s_b / s_cnt are done
            int nB;
            const int bt = block_compact(keep_b, s_cnt, nB);
            if (bt >= 0) {
#pragma unroll
                for (int k = 0; k < 9; ++k) s_b[k][bt] = v[k];
#pragma unroll
                for (int k = 0; k < 3; ++k) { s_bb[k][bt] = bb.lo[k]; s_bb[3 + k][bt] = bb.hi[k]; }
                s_ib[bt] = (int)(c * COL_CHUNK + tid);
            }
            __syncthreads();
            if (!live) continue;                                 // no barrier follows inside this trip
            for (int ib = grp; ib < nB; ib += stride) {
                Box other;
#pragma unroll
                for (int k = 0; k < 3; ++k) { other.lo[k] = s_bb[k][ib]; other.hi[k] = s_bb[3 + k][ib]; }
                if (!(gap2(mine, other) <= dmax2)) continue;     // the pair does not contribute
                double B[9];
#pragma unroll
                for (int k = 0; k < 9; ++k) B[k] = s_b[k][ib];
                double d = 0.0;
                if (!(box_meet(mine, other) && (edges_pierce(A, B) || edges_pierce(B, A)))) {
                    d = INFINITY;
#pragma unroll 1
                    for (int i = 0; i < 3; ++i) {                // vertex i of each against the other triangle
                        const double pa[3] = {s_a[3 * i][ia], s_a[3 * i + 1][ia], s_a[3 * i + 2][ia]};
                        const double pb[3] = {s_b[3 * i][ib], s_b[3 * i + 1][ib], s_b[3 * i + 2][ib]};
                        const double ta = pt_tri2(pa, B, B + 3, B + 6), tb2 = pt_tri2(pb, A, A + 3, A + 6);
                        d = ta < d ? ta : d;
                        d = tb2 < d ? tb2 : d;
                    }
#pragma unroll 1
                    for (int i = 0; i < 3; ++i) {                // edge (i, i+1) of A against the three edges of B
                        const int i1 = i == 2 ? 0 : i + 1;
                        const double p1[3] = {s_a[3 * i][ia], s_a[3 * i + 1][ia], s_a[3 * i + 2][ia]};
                        const double q1[3] = {s_a[3 * i1][ia], s_a[3 * i1 + 1][ia], s_a[3 * i1 + 2][ia]};
#pragma unroll 1
                        for (int j = 0; j < 3; ++j) {
                            const int j1 = j == 2 ? 0 : j + 1;
                            const double p2[3] = {s_b[3 * j][ib], s_b[3 * j + 1][ib], s_b[3 * j + 2][ib]};
                            const double q2[3] = {s_b[3 * j1][ib], s_b[3 * j1 + 1][ib], s_b[3 * j1 + 2][ib]};
                            const double ts = seg_seg2(p1, q1, p2, q2);
                            d = ts < d ? ts : d;
                        }
                    }
                }
                best_take(my_d, my_key, d, ((unsigned long long)rowA << 32) | (unsigned long long)(sb + s_ib[ib]));
            }
        }
    }
    // ---- the block's one partial: wave shuffles, then the four waves
#pragma unroll
    for (int off = 32; off >= 1; off >>= 1) {
        const double od = __shfl_xor(my_d, off, 64);
        const unsigned long long ok = __shfl_xor(my_key, off, 64);
        best_take(my_d, my_key, od, ok);
    }
    if ((tid & 63) == 0) { s_pd[tid >> 6] = my_d; s_pk[tid >> 6] = my_key; }
    __syncthreads();
    if (tid == 0) {
        for (int wv = 1; wv < 4; ++wv) best_take(my_d, my_key, s_pd[wv], s_pk[wv]);
        part_d[part] = my_d;
        part_k[part] = my_key;
    }
}

__global__ __launch_bounds__(256) void k_clear_finish(const double* __restrict__ part_d, const unsigned long long* __restrict__ part_k,
                                                      int64_t n, int tiles, double* __restrict__ dist2, int32_t* __restrict__ witness) {
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    double d = INFINITY;
    unsigned long long k = CLEAR_NO_KEY;
    for (int t = 0; t < tiles; ++t) best_take(d, k, part_d[(size_t)i * tiles + t], part_k[(size_t)i * tiles + t]);
    dist2[i] = d;
    witness[2 * i] = k == CLEAR_NO_KEY ? -1 : (int32_t)(k >> 32);
    witness[2 * i + 1] = k == CLEAR_NO_KEY ? -1 : (int32_t)(k & 0xffffffffull);
}

struct ClearLayout { PoseLayout pose; size_t part_d, part_k, total; };
static inline ClearLayout clear_layout(int64_t n_tri, int32_t n_links, int64_t n_poses, int64_t n_pairs) {
    ClearLayout w;
    w.pose = pose_layout(n_tri, n_links, n_poses);
    const size_t slots = (size_t)n_poses * (size_t)n_pairs * w.pose.tiles;
    w.part_d = w.pose.end;
    w.part_k = align_up(w.part_d + sizeof(double) * slots, 256);
    w.total = align_up(w.part_k + sizeof(unsigned long long) * slots, 256);
    return w;
}

}  // namespace creg
using namespace creg;

extern "C" size_t creg_mesh_clearance_workspace_bytes(int64_t n_tri, int32_t n_links, int64_t n_poses, int64_t n_pairs) {
    if (!mesh_pair_counts_ok(n_tri, n_links, n_poses, n_pairs)) return 0;
    return clear_layout(n_tri, n_links, n_poses, n_pairs).total;
}

extern "C" int creg_mesh_clearance_f64(const double* tri, const int64_t* tri_start, int64_t n_tri, const double* link_T,
                                       int32_t n_links, int64_t n_poses, const int32_t* pairs, int64_t n_pairs, double d_max,
                                       double* dist2, int32_t* witness, double* link_box, void* workspace, size_t workspace_bytes,
                                       creg_stream_t stream) {
    CREG_REQUIRE(d_max >= 0.0, "creg_mesh_clearance_f64: d_max must be >= 0 (+inf allowed), got %g", d_max);   // NaN fails too
    const ClearLayout w = clear_layout(n_tri, n_links, n_poses, n_pairs);
    if (const int rc = mesh_pair_check("creg_mesh_clearance_f64", tri, tri_start, n_tri, link_T, n_links, n_poses, pairs, n_pairs, dist2,
                                       witness, "dist2 / witness", workspace, workspace_bytes, w.total))
        return rc;
    hipStream_t s = (hipStream_t)stream;
    char* ws = (char*)workspace;
    double* part_d = (double*)(ws + w.part_d);
    unsigned long long* part_k = (unsigned long long*)(ws + w.part_k);
    const double dmax2 = d_max * d_max;
    for (int64_t p0 = 0; p0 < n_poses; p0 += 65535) {              // gridDim.y / .z hold at most 65535
        const unsigned np = (unsigned)std::min<int64_t>(n_poses - p0, 65535);
        if (const int rc = mesh_pose_launch(s, tri, tri_start, n_tri, link_T, n_links, p0, np, w.pose, ws, link_box)) return rc;
        for (int64_t m0 = 0; m0 < n_pairs; m0 += 65535) {
            const unsigned nm = (unsigned)std::min<int64_t>(n_pairs - m0, 65535);
            hipLaunchKernelGGL(k_clear_pairs, dim3(w.pose.tiles, nm, np), dim3(256), 0, s, tri_start, n_tri, (int)n_links, pairs, n_pairs,
                               m0, p0, (const double*)(ws + w.pose.posed), (const double*)(ws + w.pose.chunk_box), w.pose.n_slots,
                               (const double*)(ws + w.pose.link_box), dmax2, part_d, part_k);
            CREG_LAUNCH_CHECK();
        }
    }
    if (n_pairs > 0) {
        const int64_t n = n_poses * n_pairs;
        hipLaunchKernelGGL(k_clear_finish, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, s, part_d, part_k, n, (int)w.pose.tiles, dist2,
                           witness);
        CREG_LAUNCH_CHECK();
    }
    return CREG_OK;
}
