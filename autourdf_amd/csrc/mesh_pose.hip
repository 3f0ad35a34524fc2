// mesh_pose.hip -- the posing stage of the mesh pair queries (collide.hip, clearance.hip, contain.hip; mesh_pair.h declares it): the
// argument checks the three entries share, those the three point queries add, and the two passes that fill the workspace prefix posed | chunk_box | link_box with
// w_i = ((R_i0 v_0 + R_i1 v_1) + R_i2 v_2) + t_i and the exact min / max boxes of it per 256-triangle chunk and per link.
#include "mesh_pair.h"

namespace creg {

// The pose pass, grid (chunk, link, pose): posed vertices (P,F,9) and one box per chunk into the workspace.
__global__ __launch_bounds__(256) void k_collide_pose(const double* __restrict__ tri, const int64_t* __restrict__ tri_start,
                                                      int64_t F, const double* __restrict__ link_T, int L, int64_t p0,
                                                      double* __restrict__ posed, double* __restrict__ chunk_box,
                                                      int64_t n_slots) {
    __shared__ double s_red[30];
    const int l = blockIdx.y;
    const int64_t p = p0 + blockIdx.z;
    int64_t s, e;
    link_rows(tri_start, l, F, s, e);
    const int64_t n_chunks = (e - s + COL_CHUNK - 1) / COL_CHUNK;
    const double* T = link_T + ((size_t)p * L + l) * 16;
    for (int64_t c = blockIdx.x; c < n_chunks; c += gridDim.x) {
        const int64_t f = s + c * COL_CHUNK + threadIdx.x;
        Box b;
        box_empty(b);
        if (f < e) {
            double v[9], w[9];
#pragma unroll
            for (int k = 0; k < 9; ++k) v[k] = tri[(size_t)f * 9 + k];
            pose_tri(T, v, w);
            double* dst = posed + ((size_t)p * F + f) * 9;
#pragma unroll
            for (int k = 0; k < 9; ++k) dst[k] = w[k];
            box_of_tri(w, b);
        }
        box_block_reduce(b, s_red);
        const int64_t slot = chunk_slot(s, l) + c;
        if (threadIdx.x == 0 && slot < n_slots) box_store(chunk_box + ((size_t)p * n_slots + slot) * 6, b);
        __syncthreads();                                         // s_red is written again in the next trip
    }
}

// The link-box pass, one wave per (link, pose): the link box = min / max over its chunk boxes.
__global__ __launch_bounds__(64) void k_collide_boxes(const int64_t* __restrict__ tri_start, int64_t F, int L, int64_t p0,
                                                      const double* __restrict__ chunk_box, int64_t n_slots,
                                                      double* __restrict__ link_box_ws, double* __restrict__ link_box_out) {
    const int l = blockIdx.x;
    const int64_t p = p0 + blockIdx.y;
    int64_t s, e;
    link_rows(tri_start, l, F, s, e);
    const int64_t n_chunks = (e - s + COL_CHUNK - 1) / COL_CHUNK;
    Box b;
    box_empty(b);
    for (int64_t c = threadIdx.x; c < n_chunks; c += 64) {
        const int64_t slot = chunk_slot(s, l) + c;
        if (slot < n_slots) {
            const double* cb = chunk_box + ((size_t)p * n_slots + slot) * 6;
#pragma unroll
            for (int k = 0; k < 3; ++k) {
                b.lo[k] = fmin(b.lo[k], cb[k]);
                b.hi[k] = fmax(b.hi[k], cb[3 + k]);
            }
        }
    }
    box_wave_reduce(b);
    if (threadIdx.x == 0) {
        box_store(link_box_ws + ((size_t)p * L + l) * 6, b);
        if (link_box_out) box_store(link_box_out + ((size_t)p * L + l) * 6, b);
    }
}

int mesh_pair_check(const char* who, const void* tri, const void* tri_start, int64_t n_tri, const void* link_T, int32_t n_links,
                    int64_t n_poses, const void* pairs, int64_t n_pairs, const void* out_a, const void* out_b, const char* outs,
                    const void* workspace, size_t workspace_bytes, size_t need) {
    CREG_REQUIRE(n_poses >= 1 && n_pairs >= 0 && n_links >= 1 && n_tri >= 0,
                 "%s: bad argument (n_tri %lld, n_links %d, n_poses %lld, n_pairs %lld)", who, (long long)n_tri, (int)n_links,
                 (long long)n_poses, (long long)n_pairs);
    CREG_REQUIRE(n_tri < (1ll << 31) && n_links <= 65535, "%s: n_tri < 2^31 and n_links <= 65535 (got %lld, %d)", who, (long long)n_tri,
                 (int)n_links);
    CREG_REQUIRE(tri_start && link_T && workspace && (tri || n_tri == 0), "%s: null pointer", who);
    CREG_REQUIRE(n_pairs == 0 || (pairs && out_a && out_b), "%s: null pairs / %s with n_pairs %lld", who, outs, (long long)n_pairs);
    CREG_REQUIRE(workspace_bytes >= need, "%s: workspace of %zu bytes, %zu needed", who, workspace_bytes, need);
    return CREG_OK;
}

int point_query_check(const char* who, double d_max, int64_t n_pts, int64_t n_poses, int shift, const void* pt_start, bool rest,
                      const char* rest_names, bool per_point, const char* per_point_names) {
    CREG_REQUIRE(d_max >= 0.0, "%s: d_max must be >= 0 (+inf allowed), got %g", who, d_max);                    // NaN fails too
    CREG_REQUIRE(n_pts >= 0 && n_pts < (1ll << 31), "%s: 0 <= n_pts < 2^31 (got %lld)", who, (long long)n_pts);
    const int64_t slots = (n_pts >> shift) + n_poses;              // past the last tile slot in use
    if (!rest_names) {
        CREG_REQUIRE(slots < (1ll << 31), "%s: (n_pts >> %d) + n_poses < 2^31 (got %lld)", who, shift, (long long)slots);
        CREG_REQUIRE(pt_start && (n_pts == 0 || per_point), "%s: null pt_start, or null %s with n_pts %lld", who, per_point_names,
                     (long long)n_pts);
        return CREG_OK;
    }
    CREG_REQUIRE(n_poses >= 1 && slots < (1ll << 31), "%s: n_poses >= 1 and (n_pts >> %d) + n_poses < 2^31 (got %lld)", who, shift,
                 (long long)n_poses);
    CREG_REQUIRE(pt_start && rest, "%s: null pt_start, %s", who, rest_names);
    CREG_REQUIRE(n_pts == 0 || per_point, "%s: null %s with n_pts %lld", who, per_point_names, (long long)n_pts);
    return CREG_OK;
}

int mesh_pose_launch(hipStream_t s, const double* tri, const int64_t* tri_start, int64_t n_tri, const double* link_T, int32_t n_links,
                     int64_t p0, unsigned np, const PoseLayout& w, void* workspace, double* link_box_out) {
    char* ws = (char*)workspace;
    double* chunk_box = (double*)(ws + w.chunk_box);
    hipLaunchKernelGGL(k_collide_pose, dim3(w.tiles, (unsigned)n_links, np), dim3(256), 0, s, tri, tri_start, n_tri, link_T, (int)n_links,
                       p0, (double*)(ws + w.posed), chunk_box, w.n_slots);
    CREG_LAUNCH_CHECK();
    hipLaunchKernelGGL(k_collide_boxes, dim3((unsigned)n_links, np), dim3(64), 0, s, tri_start, n_tri, (int)n_links, p0, chunk_box,
                       w.n_slots, (double*)(ws + w.link_box), link_box_out);
    CREG_LAUNCH_CHECK();
    return CREG_OK;
}

}  // namespace creg
