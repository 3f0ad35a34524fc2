// contain.hip -- is a link wholly inside another: generalized winding numbers of posed link meshes at a few points of other
// links, fp64, every listed link pair of every pose in both directions in one call.  creg_mesh_collide_f64 and
// creg_mesh_clearance_f64 cannot see a mesh wholly inside another (no edge pierces a face); the reference rejects such a pose
// because Bullet's hulls overlap (Sim/sim_data.py:200-208).  The contract is this project's own (include/creg.h has it in full):
//   posed point    x = the vertex formula of mesh-collide with the point's own link's pose
//   gate           x is evaluated against link b iff lo_b[k] <= x[k] <= hi_b[k] on all three axes (the exact link box); otherwise
//                  its winding is exactly 0.0 and nothing is summed.  The only cull: a chunk box cannot cull a winding sum.
//   term           a = v0 - x, b = v1 - x, c = v2 - x, la = sqrt(dot(a,a)) ..., det = dot(a, cross(b,c)),
//                  den = (((la*lb)*lc + dot(a,b)*lc) + dot(b,c)*la) + dot(c,a)*lb, omega = 2*atan2(det, den)
//                  (van Oosterom and Strackee's solid angle of a triangle)
//   sum            the tree of creg_mesh_inertia_f64 over link b's triangles; w = S / (4 pi); inside iff fabs(w) > 0.5
// Plain IEEE operations in this order (the library is built with -ffp-contract=off); atan2 and sqrt are the library's.
//
// Passes (CHUNK = 256 triangles, counted from the link's first triangle):
//   posing stage      mesh_pose.hip: posed vertices and the exact link boxes (the chunk boxes are not used here)
//   k_contain_pairs   grid (chunk stride of the container, pair x direction, pose), 256 threads.  The block poses the <= 16 points
//                     of its inner link, gates them against the container's box and leaves when none passes -- the common
//                     case.  Otherwise a thread keeps one posed triangle of the chunk in registers and walks the gated points
//                     in LDS: one term, a butterfly over the wave, the wave sum into LDS; then one thread per gated point adds
//                     the four wave sums and stores the chunk's partial into its own workspace slot (pose, pair, direction,
//                     point, chunk).  Ordinary stores, no atomics.
//   k_contain_finish  one workgroup per (pair x direction, pose): the same gate, the upper levels of the tree per gated point
//                     (groups of 256 partials, in place, until one is left), then the counts, the first inside row and the
//                     winding numbers.  Every output element is written, whatever the gate said.
// fp64 VALU work, dominated by atan2 and three square roots per term; nothing here has the shape of a matrix product.
#include <vector>
#include "mesh_pair.h"

namespace creg {

constexpr int CON_MAX_PTS = 16;
constexpr double CON_FOUR_PI = 12.566370614359172;              // 4 * M_PI: the product by 4 is exact

__device__ __forceinline__ double con_dot(const double* u, const double* v) { return (u[0] * v[0] + u[1] * v[1]) + u[2] * v[2]; }

// the solid angle of the posed triangle w (9 doubles, vertex-major) seen from x, signed by its orientation
__device__ __forceinline__ double con_omega(const double* w, const double* x) {
    double a[3], b[3], c[3], g[3];
#pragma unroll
    for (int k = 0; k < 3; ++k) {
        a[k] = w[k] - x[k];
        b[k] = w[3 + k] - x[k];
        c[k] = w[6 + k] - x[k];
    }
    g[0] = b[1] * c[2] - b[2] * c[1];
    g[1] = b[2] * c[0] - b[0] * c[2];
    g[2] = b[0] * c[1] - b[1] * c[0];
    const double la = sqrt(con_dot(a, a)), lb = sqrt(con_dot(b, b)), lc = sqrt(con_dot(c, c));
    const double det = con_dot(a, g);
    const double den = (((la * lb) * lc + con_dot(a, b) * lc) + con_dot(b, c) * la) + con_dot(c, a) * lb;
    return 2.0 * atan2(det, den);
}

// The 256-leaf tree of inertia.hip for one value: a butterfly over each wave (both partners form the same sum), then
// ((w0 + w1) + w2) + w3; every thread returns with the total.  s_w: 4 doubles; the caller puts a barrier before the next call.
__device__ __forceinline__ double con_block_sum(double x, double* s_w) {
#pragma unroll
    for (int off = 32; off >= 1; off >>= 1) x += __shfl_xor(x, off, 64);
    if ((threadIdx.x & 63) == 0) s_w[threadIdx.x >> 6] = x;
    __syncthreads();
    return ((s_w[0] + s_w[1]) + s_w[2]) + s_w[3];
}

// Threads 0 .. n-1 pose the n = min(count, Q) points of link `inner` and gate them against `box`; s_x and s_gate are visible to
// the block on return.  `row0` is the link's first row of pts.  Both passes call this, so both see the same gate.
__device__ __forceinline__ int contain_gate(const double* __restrict__ pts, const int64_t* __restrict__ pt_start, int64_t NQ,
                                            const double* __restrict__ link_T, int L, int64_t p, int inner, const Box& box, int Q,
                                            double (*s_x)[3], int* s_gate, int64_t& row0) {
    int64_t s, e;
    link_rows(pt_start, inner, NQ, s, e);
    row0 = s;
    const int n = (int)(e - s < (int64_t)Q ? e - s : (int64_t)Q);
    if ((int)threadIdx.x < n) {
        const double* v = pts + (size_t)(s + threadIdx.x) * 3;
        const double* T = link_T + ((size_t)p * L + inner) * 16;
        bool in = true;
#pragma unroll
        for (int i = 0; i < 3; ++i) {
            const double x = ((T[4 * i] * v[0] + T[4 * i + 1] * v[1]) + T[4 * i + 2] * v[2]) + T[4 * i + 3];
            s_x[threadIdx.x][i] = x;
            in = in && box.lo[i] <= x && x <= box.hi[i];
        }
        s_gate[threadIdx.x] = in ? 1 : 0;
    }
    __syncthreads();
    return n;
}

// blockIdx.y = 2 * (pair - m0) + direction.  part: (P, M, 2, Q, C) chunk partials, C the chunk count of the longest possible link.
__global__ __launch_bounds__(256) void k_contain_pairs(const int64_t* __restrict__ tri_start, int64_t F,
                                                       const double* __restrict__ pts, const int64_t* __restrict__ pt_start,
                                                       int64_t NQ, const double* __restrict__ link_T, int L,
                                                       const int32_t* __restrict__ pairs, int64_t M, int64_t m0, int64_t p0,
                                                       const double* __restrict__ posed, const double* __restrict__ link_box, int Q,
                                                       int64_t C, double* __restrict__ part) {
    __shared__ double s_x[CON_MAX_PTS][3];
    __shared__ int s_gate[CON_MAX_PTS], s_list[CON_MAX_PTS], s_n;
    __shared__ double s_red[4][CON_MAX_PTS];
    const int tid = threadIdx.x;
    const int64_t m = m0 + (blockIdx.y >> 1), p = p0 + blockIdx.z;
    const int dir = blockIdx.y & 1;
    const int la = pairs[2 * m], lb = pairs[2 * m + 1];
    if (la < 0 || la >= L || lb < 0 || lb >= L || la == lb) return;
    const int inner = dir ? lb : la, outer = dir ? la : lb;
    int64_t so, eo;
    link_rows(tri_start, outer, F, so, eo);
    const int64_t n_chunks = (eo - so + COL_CHUNK - 1) / COL_CHUNK;
    if ((int64_t)blockIdx.x >= n_chunks) return;                   // uniform; covers the container without triangles
    Box box;
    box_load(link_box + ((size_t)p * L + outer) * 6, box);
    int64_t row0;
    const int n = contain_gate(pts, pt_start, NQ, link_T, L, p, inner, box, Q, s_x, s_gate, row0);
    if (tid == 0) {
        int k = 0;
        for (int j = 0; j < n; ++j)
            if (s_gate[j]) s_list[k++] = j;
        s_n = k;
    }
    __syncthreads();
    const int nq = s_n;
    if (nq == 0) return;                                         // uniform: nq comes from LDS
    const double* posed_p = posed + (size_t)p * F * 9;
    double* part_md = part + (((size_t)p * M + m) * 2 + dir) * (size_t)Q * (size_t)C;
    for (int64_t c = blockIdx.x; c < n_chunks; c += gridDim.x) {
        const int64_t f = so + c * COL_CHUNK + tid;
        const bool have = f < eo;
        double w[9];
#pragma unroll
        for (int k = 0; k < 9; ++k) w[k] = have ? posed_p[(size_t)f * 9 + k] : 0.0;
#pragma unroll 1
        for (int k = 0; k < nq; ++k) {
            double om = 0.0;                                     // a missing triangle is a zero leaf
            if (have) {
                const int j = s_list[k];
                const double x[3] = {s_x[j][0], s_x[j][1], s_x[j][2]};
                om = con_omega(w, x);
            }
#pragma unroll
            for (int off = 32; off >= 1; off >>= 1) om += __shfl_xor(om, off, 64);
            if ((tid & 63) == 0) s_red[tid >> 6][k] = om;
        }
        __syncthreads();
        if (tid < nq) part_md[(size_t)s_list[tid] * (size_t)C + c] = ((s_red[0][tid] + s_red[1][tid]) + s_red[2][tid]) + s_red[3][tid];
        __syncthreads();                                         // s_red is written again in the next trip
    }
}

// blockIdx.x = 2 * (pair - m0) + direction.  `part` is read and written by this workgroup alone (its own slots), across
// barriers: no __restrict__, no const.
__global__ __launch_bounds__(256) void k_contain_finish(const int64_t* __restrict__ tri_start, int64_t F,
                                                        const double* __restrict__ pts, const int64_t* __restrict__ pt_start,
                                                        int64_t NQ, const double* __restrict__ link_T, int L,
                                                        const int32_t* __restrict__ pairs, int64_t M, int64_t m0, int64_t p0,
                                                        const double* __restrict__ link_box, int Q, int64_t C, double* part,
                                                        int32_t* __restrict__ inside, int32_t* __restrict__ first,
                                                        double* __restrict__ winding) {
    __shared__ double s_x[CON_MAX_PTS][3];
    __shared__ int s_gate[CON_MAX_PTS];
    __shared__ double s_w[4];
    const int tid = threadIdx.x;
    const int64_t m = m0 + (blockIdx.x >> 1), p = p0 + blockIdx.y;
    const int dir = blockIdx.x & 1;
    const size_t out = ((size_t)p * M + m) * 2 + dir;
    const int la = pairs[2 * m], lb = pairs[2 * m + 1];
    double my_w = 0.0;                                           // thread j < Q ends with the winding number of point j
    int64_t row0 = 0;
    if (!(la < 0 || la >= L || lb < 0 || lb >= L || la == lb)) { // uniform
        const int inner = dir ? lb : la, outer = dir ? la : lb;
        int64_t so, eo;
        link_rows(tri_start, outer, F, so, eo);
        const int64_t n_chunks = (eo - so + COL_CHUNK - 1) / COL_CHUNK;
        Box box;
        box_load(link_box + ((size_t)p * L + outer) * 6, box);
        const int n = contain_gate(pts, pt_start, NQ, link_T, L, p, inner, box, Q, s_x, s_gate, row0);
        for (int j = 0; j < n; ++j) {
            if (!s_gate[j] || n_chunks < 1) continue;            // uniform: LDS and tri_start
            double* leaf = part + (out * (size_t)Q + (size_t)j) * (size_t)C;
            int64_t cnt = n_chunks;
            double tot = 0.0;
            while (true) {
                const int64_t groups = (cnt + 255) / 256;
                for (int64_t g = 0; g < groups; ++g) {
                    const int64_t i = g * 256 + tid;
                    tot = con_block_sum(i < cnt ? leaf[i] : 0.0, s_w);   // its barrier: every read of the group is done
                    if (tid == 0) leaf[g] = tot;                 // g <= every i read later
                    __syncthreads();                             // s_w, and the slot just written, before the next reads
                }
                if (groups == 1) break;
                cnt = groups;
            }
            if (tid == j) my_w = tot / CON_FOUR_PI;
        }
    }
    if (winding && tid < Q) winding[out * (size_t)Q + tid] = my_w;
    if (tid < 64) {                                              // the first wave holds every point
        const unsigned long long in = __ballot(tid < Q && fabs(my_w) > 0.5);
        if (tid == 0) {
            inside[out] = __popcll(in);
            first[out] = in ? (int32_t)(row0 + (__ffsll((long long)in) - 1)) : -1;
        }
    }
}

static inline int64_t contain_chunks(int64_t n_tri) { return std::max<int64_t>((n_tri + COL_CHUNK - 1) / COL_CHUNK, 1); }
struct ContainLayout { PoseLayout pose; size_t part, total; };
static inline ContainLayout contain_layout(int64_t n_tri, int32_t n_links, int64_t n_poses, int64_t n_pairs, int32_t q_stride) {
    ContainLayout w;
    w.pose = pose_layout(n_tri, n_links, n_poses);
    w.part = w.pose.end;
    w.total = align_up(w.part + sizeof(double) * (size_t)n_poses * (size_t)n_pairs * 2 * (size_t)q_stride * (size_t)contain_chunks(n_tri), 256);
    return w;
}

}  // namespace creg
using namespace creg;

extern "C" size_t creg_mesh_contain_workspace_bytes(int64_t n_tri, int32_t n_links, int64_t n_poses, int64_t n_pairs, int32_t q_stride) {
    if (!mesh_pair_counts_ok(n_tri, n_links, n_poses, n_pairs) || q_stride < 1 || q_stride > CON_MAX_PTS) return 0;
    return contain_layout(n_tri, n_links, n_poses, n_pairs, q_stride).total;
}

extern "C" int creg_mesh_contain_f64(const double* tri, const int64_t* tri_start, int64_t n_tri, const double* pts,
                                     const int64_t* pt_start, int64_t n_pts, const double* link_T, int32_t n_links, int64_t n_poses,
                                     const int32_t* pairs, int64_t n_pairs, int32_t q_stride, int32_t* inside, int32_t* first,
                                     double* winding, double* link_box, void* workspace, size_t workspace_bytes,
                                     creg_stream_t stream) {
    CREG_REQUIRE(n_pts >= 0 && n_pts < (1ll << 31), "creg_mesh_contain_f64: 0 <= n_pts < 2^31 (got %lld)", (long long)n_pts);
    CREG_REQUIRE(q_stride >= 1 && q_stride <= CON_MAX_PTS, "creg_mesh_contain_f64: q_stride must be 1 .. %d, got %d", CON_MAX_PTS,
                 (int)q_stride);
    CREG_REQUIRE(pt_start && (pts || n_pts == 0), "creg_mesh_contain_f64: null pointer");
    const ContainLayout w = contain_layout(n_tri, n_links, n_poses, n_pairs, q_stride);
    if (const int rc = mesh_pair_check("creg_mesh_contain_f64", tri, tri_start, n_tri, link_T, n_links, n_poses, pairs, n_pairs, inside,
                                       first, "inside / first", workspace, workspace_bytes, w.total))
        return rc;
    hipStream_t s = (hipStream_t)stream;
    // the points per link are read back before anything is launched: the one host synchronisation of this entry
    std::vector<int64_t> h_start((size_t)n_links + 1);
    CREG_HIP(hipMemcpyAsync(h_start.data(), pt_start, sizeof(int64_t) * h_start.size(), hipMemcpyDefault, s));
    CREG_HIP(hipStreamSynchronize(s));
    for (int32_t l = 0; l < n_links; ++l) {
        int64_t a = h_start[l], b = h_start[l + 1];
        a = a < 0 ? 0 : (a > n_pts ? n_pts : a);
        b = b < a ? a : (b > n_pts ? n_pts : b);
        CREG_REQUIRE(b - a <= (int64_t)q_stride, "creg_mesh_contain_f64: link %d owns %lld points, q_stride is %d (at most %d per link)",
                     (int)l, (long long)(b - a), (int)q_stride, CON_MAX_PTS);
    }
    char* ws = (char*)workspace;
    const double* posed = (const double*)(ws + w.pose.posed);
    const double* lbox = (const double*)(ws + w.pose.link_box);
    double* part = (double*)(ws + w.part);
    const int64_t C = contain_chunks(n_tri);
    for (int64_t p0 = 0; p0 < n_poses; p0 += 65535) {              // gridDim.y / .z hold at most 65535
        const unsigned np = (unsigned)std::min<int64_t>(n_poses - p0, 65535);
        if (const int rc = mesh_pose_launch(s, tri, tri_start, n_tri, link_T, n_links, p0, np, w.pose, ws, link_box)) return rc;
        for (int64_t m0 = 0; m0 < n_pairs; m0 += 32767) {          // two directions per pair in gridDim.y
            const unsigned nm = (unsigned)std::min<int64_t>(n_pairs - m0, 32767);
            hipLaunchKernelGGL(k_contain_pairs, dim3(w.pose.tiles, 2 * nm, np), dim3(256), 0, s, tri_start, n_tri, pts, pt_start, n_pts,
                               link_T, (int)n_links, pairs, n_pairs, m0, p0, posed, lbox, (int)q_stride, C, part);
            CREG_LAUNCH_CHECK();
            hipLaunchKernelGGL(k_contain_finish, dim3(2 * nm, np), dim3(256), 0, s, tri_start, n_tri, pts, pt_start, n_pts, link_T,
                               (int)n_links, pairs, n_pairs, m0, p0, lbox, (int)q_stride, C, part, inside, first, winding);
            CREG_LAUNCH_CHECK();
        }
    }
    return CREG_OK;
}
