// point_rows.h -- a pose's rows of points, in tiles: what the kernels over (pose, tile of that pose's points) share.  A header of its
// own beside mesh_dist.h, which it includes; point_mesh.hip, pose_fit.hip, link_moments.hip and feature_moments.hip include this one.
//   rows and tiles   pose_rows (the one clamp of pt_start), tile_slot and find_tile (block -> pose and tile), for tiles of 1 << SHIFT
//   matched_row      does a row with a nearest triangle contribute, with which link, r and r.r (pose_fit.hip, link_moments.hip)
//   matched_feature_row   the same, with pt_tri_vec's case and the posed vertices as well (feature_moments.hip)
//   tile_sum4        a pose's tile partials into one sum, in the order include/creg.h fixes
// The contract of every function is in include/creg.h under creg_point_mesh_f64 and creg_pose_fit_system_f64.
#pragma once
#include "mesh_dist.h"

namespace creg {

// rows [s, e) of pose p, clamped into [0, N] as link_rows clamps tri_start
__device__ __forceinline__ void pose_rows(const int64_t* __restrict__ pt_start, int64_t p, int64_t N, int64_t& s, int64_t& e) {
    s = pt_start[p];
    e = pt_start[p + 1];
    s = s < 0 ? 0 : (s > N ? N : s);
    e = e < s ? s : (e > N ? N : e);
}
// the tiles of pose p start at this block: the slots of distinct poses never overlap, as chunk_slot's
template <int SHIFT>
__device__ __forceinline__ int64_t tile_slot(const int64_t* __restrict__ pt_start, int64_t p, int64_t N) {
    int64_t s = pt_start[p];
    s = s < 0 ? 0 : (s > N ? N : s);
    return (s >> SHIFT) + p;
}
// block blk belongs to the pose p with the largest tile_slot(p) not above it (the same for every thread) and to tile
// blk - tile_slot(p) of its rows [ps, pe); false for a block before the first slot or past the pose's last tile
template <int SHIFT>
__device__ __forceinline__ bool find_tile(const int64_t* __restrict__ pt_start, int64_t N, int64_t P, int64_t blk, int64_t& p, int64_t& ps,
                                          int64_t& pe, int64_t& tile) {
    constexpr int TILE = 1 << SHIFT;
    if (tile_slot<SHIFT>(pt_start, 0, N) > blk) return false;
    int64_t lo = 0, hi = P;                                      // tile_slot(lo) <= blk < tile_slot(hi), with tile_slot(P) = +inf
    while (hi - lo > 1) {
        const int64_t mid = lo + ((hi - lo) >> 1);
        if (tile_slot<SHIFT>(pt_start, mid, N) <= blk) lo = mid; else hi = mid;
    }
    p = lo;
    pose_rows(pt_start, p, N, ps, pe);
    tile = blk - tile_slot<SHIFT>(pt_start, p, N);
    return tile < (pe - ps + TILE - 1) / TILE;
}

__device__ __forceinline__ int64_t clamped_start(const int64_t* __restrict__ tri_start, int l, int64_t F) {
    const int64_t s = tri_start[l];
    return s < 0 ? 0 : (s > F ? F : s);
}
// Calls use(l, r, rr) iff the row of pose p with point x and nearest triangle f contributes: x live, 0 <= f < F, row f among the
// rows of a link l (the largest l whose clamped start is not above f), rr = dot3(r, r) <= dmax2 for r = pt_tri_vec of x against
// the row's vertices posed by pose_tri, so rr has the bits of creg_point_mesh_f64's dist2.  The caller's code runs inside the gate,
// where the kernels had it: a returned link tested again by the caller cost k_link_moments_tiles two SGPRs.
// matched_feature_row is the same gate handing out more: use(l, r, rr, which, w) with which = the case pt_tri_vec returned (1 .. 7) and
// w (9) the posed vertices a | b | c it was computed from (feature_moments.hip builds the feature's projector from them).
template <class Use>
__device__ __forceinline__ void matched_feature_row(const double* __restrict__ tri, const int64_t* __restrict__ tri_start, int64_t F,
                                                    const double* __restrict__ link_T, int L, int64_t p, const double* x, int64_t f,
                                                    double dmax2, Use use) {
    const bool live = x[0] == x[0] && x[1] == x[1] && x[2] == x[2];
    if (!(live && f >= 0 && f < F)) return;
    int lo = 0, up = L;
    while (up - lo > 1) {
        const int mid = lo + ((up - lo) >> 1);
        if (clamped_start(tri_start, mid, F) <= f) lo = mid; else up = mid;
    }
    int64_t sl, el;
    link_rows(tri_start, lo, F, sl, el);
    if (!(f >= sl && f < el)) return;
    double v[9], w[9], r[3];
#pragma unroll
    for (int k = 0; k < 9; ++k) v[k] = tri[(size_t)f * 9 + k];
    pose_tri(link_T + ((size_t)p * L + lo) * 16, v, w);
    const int which = pt_tri_vec(x, w, w + 3, w + 6, r);
    const double rr = dot3(r, r);
    if (rr <= dmax2) use(lo, r, rr, which, w);
}
template <class Use>
__device__ __forceinline__ void matched_row(const double* __restrict__ tri, const int64_t* __restrict__ tri_start, int64_t F,
                                            const double* __restrict__ link_T, int L, int64_t p, const double* x, int64_t f, double dmax2,
                                            Use use) {
    matched_feature_row(tri, tri_start, F, link_T, L, p, x, f, dmax2,
                        [&](int l, const double* r, double rr, int, const double*) { use(l, r, rr); });
}

// a pose's tile partials src[t * stride], t = 0 .. tiles - 1 in ascending order, into four running sums (tile t into sum t mod 4)
__device__ __forceinline__ double tile_sum4(const double* src, size_t stride, int64_t tiles) {
    double s0 = 0.0, s1 = 0.0, s2 = 0.0, s3 = 0.0;
    int64_t t = 0;
    for (; t + 4 <= tiles; t += 4) {
        s0 += src[t * stride];
        s1 += src[(t + 1) * stride];
        s2 += src[(t + 2) * stride];
        s3 += src[(t + 3) * stride];
    }
    if (t < tiles) s0 += src[t * stride];
    if (t + 1 < tiles) s1 += src[(t + 1) * stride];
    if (t + 2 < tiles) s2 += src[(t + 2) * stride];
    return (s0 + s1) + (s2 + s3);
}

}  // namespace creg
