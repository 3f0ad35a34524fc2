// collide.hip -- self-collision of an articulated triangle mesh, fp64: every listed link pair of every pose in one call,
// triangle mesh against triangle mesh.  The reference's frame generator asks PyBullet for self contacts (Sim/sim_data.py:200-208,
// :276-281: convex hulls of the <collision> geometry with Bullet's margins, after a physics step); PyBullet is not part of
// this build and that check is not imitated.  The contract here is this project's own (include/creg.h has it in full):
//   posed vertex   w_i = ((R_i0 v_0 + R_i1 v_1) + R_i2 v_2) + t_i
//   triangle pair  collides iff the posed boxes (exact min / max of the three vertices, closed comparisons) overlap AND an
//                  edge of one properly pierces the other (3 + 3 edge tests)
//   orient(p,q,r,s) = ((u x v)_x w_x + (u x v)_y w_y) + (u x v)_z w_z,  u = q - p, v = r - p, w = s - p
//   edge (p,q) properly pierces (a,b,c) iff orient(a,b,c,p), orient(a,b,c,q) have strictly opposite signs and
//                  orient(p,q,a,b), orient(p,q,b,c), orient(p,q,c,a) are all > 0 or all < 0; a zero anywhere is "no"
// Plain IEEE operations in this order (the library is built with -ffp-contract=off), so a numpy restatement reaches the same
// decisions.  Because the box test is part of the contract, every cull below -- link box, chunk box, tile union box, all
// exact min / max of the same posed vertices -- is exactly conservative: culling changes no output.
//
// Passes (CHUNK = 256 triangles, counted from the link's first triangle; the device helpers are in mesh_pair.h):
//   posing stage     mesh_pose.hip: posed vertices (P,F,9), one box per chunk and one per link into the workspace
//   k_collide_pairs  grid (tile of link A, pair, pose), 256 threads.  Exits when the link boxes, or the tile's chunk box and
//                    link B's box, are disjoint.  Keeps the tile's triangles whose box meets link B's box, ballot-compacted
//                    into LDS as SoA (component-major: lane i reads word i, no bank conflict), forms their union box, then
//                    streams link B chunk by chunk: a chunk whose box misses the union box is skipped, the others keep the
//                    triangles that meet the union box, compacted into LDS.  Thread t owns A triangle t & (n2 - 1), n2 the
//                    power of two >= the kept count, and walks the B survivors with stride 256 / n2: box test against the
//                    registers, then the edge tests.  One integer atomic add and one 64-bit atomic min per wave that found
//                    something, at the end of the block: the outputs do not depend on scheduling.
//   k_collide_first  (a << 32 | b) keys -> first (a, b) or (-1, -1)
// fp64 VALU work throughout; nothing here has the shape of a matrix product.
#include "mesh_pair.h"

namespace creg {

__global__ __launch_bounds__(256) void k_collide_pairs(const int64_t* __restrict__ tri_start, int64_t F, int L,
                                                       const int32_t* __restrict__ pairs, int64_t M, int64_t m0, int64_t p0,
                                                       const double* __restrict__ posed, const double* __restrict__ chunk_box,
                                                       int64_t n_slots, const double* __restrict__ link_box,
                                                       int32_t* __restrict__ count, unsigned long long* __restrict__ keys) {
    __shared__ double s_a[9][COL_CHUNK];                         // kept A triangles, component-major
    __shared__ double s_b[9][COL_CHUNK];                         // kept B triangles of the current chunk
    __shared__ double s_bb[6][COL_CHUNK];                        // their boxes
    __shared__ int s_ia[COL_CHUNK], s_ib[COL_CHUNK];             // their rows in tri, relative to the link's first
    __shared__ double s_red[30];
    __shared__ int s_cnt[4];
    const int tid = threadIdx.x;
    const int64_t m = m0 + blockIdx.y, p = p0 + blockIdx.z;
    const int la = pairs[2 * m], lb = pairs[2 * m + 1];
    if (la < 0 || la >= L || lb < 0 || lb >= L || la == lb) return;       // count stays 0, first (-1,-1)
    Box boxA, boxB;
    box_load(link_box + ((size_t)p * L + la) * 6, boxA);
    box_load(link_box + ((size_t)p * L + lb) * 6, boxB);
    if (!box_meet(boxA, boxB)) return;
    int64_t sa, ea, sb, eb;
    link_rows(tri_start, la, F, sa, ea);
    link_rows(tri_start, lb, F, sb, eb);
    const int64_t tiles_a = (ea - sa + COL_CHUNK - 1) / COL_CHUNK, chunks_b = (eb - sb + COL_CHUNK - 1) / COL_CHUNK;
    const double* cbox_p = chunk_box + (size_t)p * n_slots * 6;
    const double* posed_p = posed + (size_t)p * F * 9;
    int my_count = 0;
    unsigned long long my_key = ~0ull;

    for (int64_t tile = blockIdx.x; tile < tiles_a; tile += gridDim.x) {
        const int64_t slot_a = chunk_slot(sa, la) + tile;
        Box tb;
        box_empty(tb);
        if (slot_a < n_slots) box_load(cbox_p + slot_a * 6, tb);
        if (!box_meet(tb, boxB)) continue;                       // the same for every thread
        // ---- the tile's triangles that meet link B's box
        const int64_t fa = sa + tile * COL_CHUNK + tid;
        double w[9];
        Box b;
        box_empty(b);
        bool keep = false;
        if (fa < ea) {
#pragma unroll
            for (int k = 0; k < 9; ++k) w[k] = posed_p[(size_t)fa * 9 + k];
            box_of_tri(w, b);
            keep = box_meet(b, boxB);
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
        Box mine;
        box_empty(mine);
        long long rowA = 0;
        if (live) {
#pragma unroll
            for (int k = 0; k < 3; ++k) {
                mine.lo[k] = fmin(fmin(s_a[k][ia], s_a[3 + k][ia]), s_a[6 + k][ia]);
                mine.hi[k] = fmax(fmax(s_a[k][ia], s_a[3 + k][ia]), s_a[6 + k][ia]);
            }
            rowA = (long long)(sa + s_ia[ia]);
        }
        // ---- link B, chunk by chunk
        for (int64_t c = 0; c < chunks_b; ++c) {
            const int64_t slot_b = chunk_slot(sb, lb) + c;
            Box cb;
            box_empty(cb);
            if (slot_b < n_slots) box_load(cbox_p + slot_b * 6, cb);
            if (!box_meet(cb, uni)) continue;                    // uniform
            const int64_t fb = sb + c * COL_CHUNK + tid;
            double v[9];
            Box bb;
            bool keep_b = false;
            if (fb < eb) {
#pragma unroll
                for (int k = 0; k < 9; ++k) v[k] = posed_p[(size_t)fb * 9 + k];
                box_of_tri(v, bb);
                keep_b = box_meet(bb, uni);
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
                if (!(mine.lo[0] <= s_bb[3][ib] && s_bb[0][ib] <= mine.hi[0] && mine.lo[1] <= s_bb[4][ib] &&
                      s_bb[1][ib] <= mine.hi[1] && mine.lo[2] <= s_bb[5][ib] && s_bb[2][ib] <= mine.hi[2]))
                    continue;
                double A[9], B[9];
#pragma unroll
                for (int k = 0; k < 9; ++k) { A[k] = s_a[k][ia]; B[k] = s_b[k][ib]; }
                if (edges_pierce(A, B) || edges_pierce(B, A)) {
                    ++my_count;
                    const unsigned long long key = ((unsigned long long)rowA << 32) | (unsigned long long)(sb + s_ib[ib]);
                    my_key = key < my_key ? key : my_key;
                }
            }
        }
    }
    // ---- one add and one min per wave that found something
#pragma unroll
    for (int off = 32; off >= 1; off >>= 1) {
        my_count += __shfl_xor(my_count, off, 64);
        const unsigned long long o = __shfl_xor(my_key, off, 64);
        my_key = o < my_key ? o : my_key;
    }
    if ((tid & 63) == 0 && my_count > 0) {
        atomicAdd(count + (size_t)p * M + m, my_count);
        atomicMin(keys + (size_t)p * M + m, my_key);
    }
}

__global__ __launch_bounds__(256) void k_collide_first(const unsigned long long* __restrict__ keys, int64_t n,
                                                       int32_t* __restrict__ first) {
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    const unsigned long long k = keys[i];
    first[2 * i] = k == ~0ull ? -1 : (int32_t)(k >> 32);
    first[2 * i + 1] = k == ~0ull ? -1 : (int32_t)(k & 0xffffffffull);
}

struct CollideLayout { PoseLayout pose; size_t keys, total; };
static inline CollideLayout collide_layout(int64_t n_tri, int32_t n_links, int64_t n_poses, int64_t n_pairs) {
    CollideLayout w;
    w.pose = pose_layout(n_tri, n_links, n_poses);
    w.keys = w.pose.end;
    w.total = align_up(w.keys + sizeof(unsigned long long) * (size_t)n_poses * (size_t)n_pairs, 256);
    return w;
}

}  // namespace creg
using namespace creg;

extern "C" size_t creg_mesh_collide_workspace_bytes(int64_t n_tri, int32_t n_links, int64_t n_poses, int64_t n_pairs) {
    if (!mesh_pair_counts_ok(n_tri, n_links, n_poses, n_pairs)) return 0;
    return collide_layout(n_tri, n_links, n_poses, n_pairs).total;
}

extern "C" int creg_mesh_collide_f64(const double* tri, const int64_t* tri_start, int64_t n_tri, const double* link_T,
                                     int32_t n_links, int64_t n_poses, const int32_t* pairs, int64_t n_pairs, int32_t* count,
                                     int32_t* first, double* link_box, void* workspace, size_t workspace_bytes,
                                     creg_stream_t stream) {
    const CollideLayout w = collide_layout(n_tri, n_links, n_poses, n_pairs);
    if (const int rc = mesh_pair_check("creg_mesh_collide_f64", tri, tri_start, n_tri, link_T, n_links, n_poses, pairs, n_pairs, count,
                                       first, "count / first", workspace, workspace_bytes, w.total))
        return rc;
    hipStream_t s = (hipStream_t)stream;
    char* ws = (char*)workspace;
    unsigned long long* keys = (unsigned long long*)(ws + w.keys);
    if (n_pairs > 0) {
        CREG_HIP(hipMemsetAsync(count, 0, sizeof(int32_t) * (size_t)n_poses * (size_t)n_pairs, s));
        CREG_HIP(hipMemsetAsync(keys, 0xff, sizeof(unsigned long long) * (size_t)n_poses * (size_t)n_pairs, s));
    }
    for (int64_t p0 = 0; p0 < n_poses; p0 += 65535) {              // gridDim.y / .z hold at most 65535
        const unsigned np = (unsigned)std::min<int64_t>(n_poses - p0, 65535);
        if (const int rc = mesh_pose_launch(s, tri, tri_start, n_tri, link_T, n_links, p0, np, w.pose, ws, link_box)) return rc;
        for (int64_t m0 = 0; m0 < n_pairs; m0 += 65535) {
            const unsigned nm = (unsigned)std::min<int64_t>(n_pairs - m0, 65535);
            hipLaunchKernelGGL(k_collide_pairs, dim3(w.pose.tiles, nm, np), dim3(256), 0, s, tri_start, n_tri, (int)n_links, pairs,
                               n_pairs, m0, p0, (const double*)(ws + w.pose.posed), (const double*)(ws + w.pose.chunk_box),
                               w.pose.n_slots, (const double*)(ws + w.pose.link_box), count, keys);
            CREG_LAUNCH_CHECK();
        }
    }
    if (n_pairs > 0) {
        const int64_t n = n_poses * n_pairs;
        hipLaunchKernelGGL(k_collide_first, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, s, keys, n, first);
        CREG_LAUNCH_CHECK();
    }
    return CREG_OK;
}
