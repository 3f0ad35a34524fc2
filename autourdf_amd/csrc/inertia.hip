// inertia.hip -- mass properties of closed link meshes, fp64: volume, area, centre of mass, inertia tensor and principal axes of
// every link in one set of launches.  The reference writes a placeholder <inertial> block (PointCloud/compute_joints.py:334-339,
// "example values, adjust as needed"); the contract here is this project's own (include/creg.h has it in full).
//   reference point  r = first vertex of the link's first triangle; a = v0 - r, b = v1 - r, c = v2 - r
//   per triangle     14 terms: n = (b-a) x (c-a) | |n| | d = a . (b x c) | d s, s = (a+b)+c | d (s_i s_j + a_i a_j + b_i b_j + c_i c_j)
//   per link         their sums in a fixed tree, then volume, area, closure, com, inertia, mass, principal moments and axes
// Plain IEEE operations in the order creg.h states (the library is built with -ffp-contract=off).
//
// Passes (CHUNK = 256 triangles, counted from the link's first triangle, as in collide.hip):
//   k_inertia_chunks  grid (chunk, link), 256 threads: a thread per triangle (a missing one contributes zeros), a butterfly
//                     over each wave, the four wave sums through LDS, one 14-double partial per chunk into the workspace
//                     with ordinary stores.  No atomics.
//   k_inertia_finish  one workgroup per link: groups of 256 partials go through the same 256-leaf tree, in place, until one is
//                     left, then thread 0 derives the outputs.
// The tree of a link depends on its own triangle count alone: neither on the grid, nor on the other links of the call.
// 72 bytes per triangle are read once; fp64 VALU work, nothing here has the shape of a matrix product.
#include <algorithm>
#include <cmath>
#include "creg_common.h"
#include "eig3.h"

namespace creg {

constexpr int INR_CHUNK = 256;
constexpr int INR_TILES_X = 128;                                 // cap of gridDim.x: blocks stride over a link's chunks
constexpr int INR_TERMS = 14;

// rows [s, e) of link l, clamped into [0, F] so that a broken tri_start reads nothing outside tri
__device__ __forceinline__ void inr_link_rows(const int64_t* __restrict__ tri_start, int l, int64_t F, int64_t& s, int64_t& e) {
    s = tri_start[l];
    e = tri_start[l + 1];
    s = s < 0 ? 0 : (s > F ? F : s);
    e = e < s ? s : (e > F ? F : e);
}
// the partials of link l start at this slot: distinct links never share one (floor(s / 256) + l grows by at least the link's
// chunk count from one link to the next), and the last slot in use is below floor(F / 256) + L + 1
__device__ __forceinline__ int64_t inr_slot(int64_t s, int l) { return (s >> 8) + l; }

// The 256-leaf tree: leaf t is thread t's x.  Butterfly over each wave (lane i adds lane i ^ 32, then ^ 16 ... ^ 1: both
// partners form the same sum), then ((w0 + w1) + w2) + w3.  Threads 0..13 return with component threadIdx.x of the total in
// x[0] -- the others with a wave sum.  s_red: 4 x 14 doubles; the caller puts a barrier before the next call.
__device__ __forceinline__ void inr_block_sum(double* x, double (*s_red)[INR_TERMS]) {
#pragma unroll
    for (int off = 32; off >= 1; off >>= 1)
#pragma unroll
        for (int k = 0; k < INR_TERMS; ++k) x[k] += __shfl_xor(x[k], off, 64);
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    if (lane == 0)
#pragma unroll
        for (int k = 0; k < INR_TERMS; ++k) s_red[wave][k] = x[k];
    __syncthreads();
    if (threadIdx.x < INR_TERMS) {
        const int k = threadIdx.x;
        x[0] = ((s_red[0][k] + s_red[1][k]) + s_red[2][k]) + s_red[3][k];
    }
}

__device__ __forceinline__ void inr_terms(const double* v, const double* r, double* x) {
    double a[3], b[3], c[3], e1[3], e2[3], n[3], bc[3], s[3];
#pragma unroll
    for (int k = 0; k < 3; ++k) {
        a[k] = v[k] - r[k];
        b[k] = v[3 + k] - r[k];
        c[k] = v[6 + k] - r[k];
        e1[k] = b[k] - a[k];
        e2[k] = c[k] - a[k];
        s[k] = (a[k] + b[k]) + c[k];
    }
    cross3(e1, e2, n);
    cross3(b, c, bc);
    const double d = (a[0] * bc[0] + a[1] * bc[1]) + a[2] * bc[2];
    x[0] = n[0]; x[1] = n[1]; x[2] = n[2];
    x[3] = sqrt((n[0] * n[0] + n[1] * n[1]) + n[2] * n[2]);
    x[4] = d;
    x[5] = d * s[0]; x[6] = d * s[1]; x[7] = d * s[2];
    int at = 8;
#pragma unroll
    for (int i = 0; i < 3; ++i)
#pragma unroll
        for (int j = i; j < 3; ++j) x[at++] = d * (((s[i] * s[j] + a[i] * a[j]) + b[i] * b[j]) + c[i] * c[j]);
}

__global__ __launch_bounds__(256) void k_inertia_chunks(const double* __restrict__ tri, const int64_t* __restrict__ tri_start,
                                                        int64_t F, double* __restrict__ partial, int64_t n_slots) {
    __shared__ double s_red[4][INR_TERMS];
    const int l = blockIdx.y;
    int64_t s, e;
    inr_link_rows(tri_start, l, F, s, e);
    const int64_t n_chunks = (e - s + INR_CHUNK - 1) / INR_CHUNK;
    if ((int64_t)blockIdx.x >= n_chunks) return;                  // uniform; covers the empty link (no read of tri below)
    double r[3];
#pragma unroll
    for (int k = 0; k < 3; ++k) r[k] = tri[(size_t)s * 9 + k];
    for (int64_t c = blockIdx.x; c < n_chunks; c += gridDim.x) {
        const int64_t f = s + c * INR_CHUNK + threadIdx.x;
        double x[INR_TERMS];
#pragma unroll
        for (int k = 0; k < INR_TERMS; ++k) x[k] = 0.0;
        if (f < e) {
            double v[9];
#pragma unroll
            for (int k = 0; k < 9; ++k) v[k] = tri[(size_t)f * 9 + k];
            inr_terms(v, r, x);
        }
        inr_block_sum(x, s_red);
        const int64_t slot = inr_slot(s, l) + c;
        if (threadIdx.x < INR_TERMS && slot < n_slots) partial[(size_t)slot * INR_TERMS + threadIdx.x] = x[0];
        __syncthreads();                                         // s_red is written again in the next trip
    }
}

// `partial` is read and written by this workgroup alone (the link's own slots), across barriers: no __restrict__, no const
__global__ __launch_bounds__(256) void k_inertia_finish(const double* __restrict__ tri, const int64_t* __restrict__ tri_start,
                                                        int64_t F, const double* __restrict__ density, double* partial,
                                                        int64_t n_slots, double* __restrict__ sums, double* __restrict__ volume,
                                                        double* __restrict__ area, double* __restrict__ closure,
                                                        double* __restrict__ mass, double* __restrict__ com,
                                                        double* __restrict__ inertia, double* __restrict__ principal,
                                                        double* __restrict__ axes) {
    __shared__ double s_red[4][INR_TERMS];
    __shared__ double s_tot[INR_TERMS];
    const int l = blockIdx.x;
    int64_t s, e;
    inr_link_rows(tri_start, l, F, s, e);
    int64_t n = (e - s + INR_CHUNK - 1) / INR_CHUNK;
    const int64_t base = inr_slot(s, l);
    if (threadIdx.x < INR_TERMS) s_tot[threadIdx.x] = 0.0;
    __syncthreads();
    while (n >= 1) {                                             // uniform: n comes from tri_start
        const int64_t groups = (n + 255) / 256;
        for (int64_t g = 0; g < groups; ++g) {
            const int64_t i = g * 256 + threadIdx.x;
            double x[INR_TERMS];
#pragma unroll
            for (int k = 0; k < INR_TERMS; ++k) x[k] = (i < n && base + i < n_slots) ? partial[(size_t)(base + i) * INR_TERMS + k] : 0.0;
            inr_block_sum(x, s_red);                             // its barrier: every read of the group is done
            if (threadIdx.x < INR_TERMS) {
                s_tot[threadIdx.x] = x[0];
                if (base + g < n_slots) partial[(size_t)(base + g) * INR_TERMS + threadIdx.x] = x[0];   // g <= every i read later
            }
            __syncthreads();                                     // s_red, and the slot just written, before the next reads
        }
        if (groups == 1) break;
        n = groups;
    }
    if (threadIdx.x != 0) return;
    double S[INR_TERMS];
#pragma unroll
    for (int k = 0; k < INR_TERMS; ++k) S[k] = s_tot[k];
    const bool none = !(S[4] != 0.0);                            // no triangle, or zero volume: zero sums
    if (none)
#pragma unroll
        for (int k = 0; k < INR_TERMS; ++k) S[k] = 0.0;
#pragma unroll
    for (int k = 0; k < INR_TERMS; ++k) sums[(size_t)l * INR_TERMS + k] = S[k];
    const double rho = density[l];
    const double vol = S[4] / 6.0;
    volume[l] = vol;
    area[l] = S[3] / 2.0;
    closure[l] = S[3] > 0.0 ? sqrt((S[0] * S[0] + S[1] * S[1]) + S[2] * S[2]) / S[3] : 0.0;
    mass[l] = rho * vol;
    double* o_com = com + (size_t)l * 3;
    double* o_in = inertia + (size_t)l * 6;
    double* o_pr = principal + (size_t)l * 3;
    double* o_ax = axes + (size_t)l * 9;
    if (none) {
        for (int k = 0; k < 3; ++k) o_com[k] = o_pr[k] = NAN;
        for (int k = 0; k < 6; ++k) o_in[k] = NAN;
        for (int k = 0; k < 9; ++k) o_ax[k] = NAN;
        return;
    }
    double m[3], C[6], J[6];
#pragma unroll
    for (int k = 0; k < 3; ++k) {
        m[k] = (S[5 + k] / 24.0) / vol;
        o_com[k] = tri[(size_t)s * 9 + k] + m[k];
    }
    int at = 0;
#pragma unroll
    for (int i = 0; i < 3; ++i)
#pragma unroll
        for (int j = i; j < 3; ++j, ++at) C[at] = S[8 + at] / 120.0 - (vol * m[i]) * m[j];
    J[0] = rho * (C[3] + C[5]); J[1] = -(rho * C[1]); J[2] = -(rho * C[2]);
    J[3] = rho * (C[0] + C[5]); J[4] = -(rho * C[4]); J[5] = rho * (C[0] + C[3]);
#pragma unroll
    for (int k = 0; k < 6; ++k) o_in[k] = J[k];
    double w[3], V[9];
    sym3_eig_jacobi(J, w, V);
#pragma unroll
    for (int k = 0; k < 3; ++k) o_pr[k] = w[k];
#pragma unroll
    for (int k = 0; k < 9; ++k) o_ax[k] = V[k];
}

static inline int64_t inertia_slots(int64_t n_tri, int32_t n_links) { return (n_tri >> 8) + n_links + 1; }

}  // namespace creg
using namespace creg;

extern "C" size_t creg_mesh_inertia_workspace_bytes(int64_t n_tri, int32_t n_links) {
    if (n_tri < 0 || n_links < 1) return 0;
    return align_up(sizeof(double) * INR_TERMS * (size_t)inertia_slots(n_tri, n_links), 256);
}

extern "C" int creg_mesh_inertia_f64(const double* tri, const int64_t* tri_start, int64_t n_tri, int32_t n_links,
                                     const double* density, double* sums, double* volume, double* area, double* closure,
                                     double* mass, double* com, double* inertia, double* principal, double* axes,
                                     void* workspace, size_t workspace_bytes, creg_stream_t stream) {
    CREG_REQUIRE(n_links >= 1 && n_tri >= 0, "creg_mesh_inertia_f64: bad argument (n_tri %lld, n_links %d)", (long long)n_tri,
                 (int)n_links);
    CREG_REQUIRE(n_tri < (1ll << 31) && n_links <= 65535, "creg_mesh_inertia_f64: n_tri < 2^31 and n_links <= 65535 (got %lld, %d)",
                 (long long)n_tri, (int)n_links);
    CREG_REQUIRE(tri_start && density && workspace && (tri || n_tri == 0), "creg_mesh_inertia_f64: null pointer");
    CREG_REQUIRE(sums && volume && area && closure && mass && com && inertia && principal && axes,
                 "creg_mesh_inertia_f64: null output");
    const size_t need = creg_mesh_inertia_workspace_bytes(n_tri, n_links);
    CREG_REQUIRE(workspace_bytes >= need, "creg_mesh_inertia_f64: workspace of %zu bytes, %zu needed", workspace_bytes, need);
    hipStream_t s = (hipStream_t)stream;
    double* partial = (double*)workspace;
    const int64_t n_slots = inertia_slots(n_tri, n_links);
    const unsigned tiles = (unsigned)std::min<int64_t>(std::max<int64_t>((n_tri + INR_CHUNK - 1) / INR_CHUNK, 1), INR_TILES_X);
    hipLaunchKernelGGL(k_inertia_chunks, dim3(tiles, (unsigned)n_links), dim3(256), 0, s, tri, tri_start, n_tri, partial, n_slots);
    CREG_LAUNCH_CHECK();
    hipLaunchKernelGGL(k_inertia_finish, dim3((unsigned)n_links), dim3(256), 0, s, tri, tri_start, n_tri, density, partial, n_slots,
                       sums, volume, area, closure, mass, com, inertia, principal, axes);
    CREG_LAUNCH_CHECK();
    return CREG_OK;
}
