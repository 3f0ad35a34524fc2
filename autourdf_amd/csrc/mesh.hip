// mesh.hip -- N4: the meshing half of the reference's URDF stage (PointCloud/link.py:204-314, link_mesh), all links of one
// directory per launch.  The contract is this project's own (DESIGN N4): statistical outlier removal restated from Open3D's
// published rule, a voxel grid padded by one empty layer, marching cubes at level 0.5 on the 0/1 volume (every vertex the
// midpoint of a lattice edge: integers in half-voxel units), one pass of simple smoothing with integer sums, STL records.
//
// Every array is the links' concatenation with an (L+1) offset table beside it; a thread finds its link by bisection.
// Prefix sums are three launches (tile sums, one workgroup over the tile sums, apply): no workgroup waits for another.
// No floating-point atomics: the per-link statistics are fixed-order trees in one workgroup, the smoothing sums are integers.
#include <cmath>
#include "creg_common.h"
#define MC_TABLE_QUAL static __device__ const
#include "mc_table.h"

namespace creg {

constexpr int MS_NT = 256;
constexpr int MS_ITEMS = 8;                       // nodes per thread in the scan kernels
constexpr int MS_TILE = MS_NT * MS_ITEMS;         // one scan block's reach
constexpr int MS_MAX_AXIS = 1024;                 // padded nodes per axis
constexpr int64_t MS_MAX_NODES = (int64_t)1 << 28;

// l with off[l] <= i < off[l + 1] (empty segments are skipped); i must lie in [off[0], off[L])
__device__ __forceinline__ int find_seg(const int64_t* __restrict__ off, int L, int64_t i) {
    int lo = 0, hi = L;                           // invariant: off[lo] <= i < off[hi]
    while (hi - lo > 1) {
        const int mid = (lo + hi) >> 1;
        if (off[mid] <= i) lo = mid; else hi = mid;
    }
    return lo;
}

// ---------------------------------------------------------------------------------------------- (a) outliers
// All-pairs scan over the links a block's 256 queries belong to, 256 candidates per LDS tile (every lane reads the same
// address: a broadcast); each thread keeps the K smallest squared distances of its own link, ascending, in registers.
template <int K>
__global__ __launch_bounds__(MS_NT) void k_sor_knn(const double* __restrict__ P, int64_t n, const int64_t* __restrict__ off,
                                                   int L, int nb, double* __restrict__ avg) {
    __shared__ double sx[MS_NT], sy[MS_NT], sz[MS_NT];
    const int tid = threadIdx.x;
    const int64_t b0 = (int64_t)blockIdx.x * MS_NT, b1 = (b0 + MS_NT < n ? b0 + MS_NT : n) - 1;
    const int64_t i = b0 + tid;
    const bool live = i < n;
    const int l = find_seg(off, L, live ? i : b1);
    const int64_t lo = off[l], hi = off[l + 1];
    const int64_t rlo = off[find_seg(off, L, b0)], rhi = off[find_seg(off, L, b1) + 1];
    double px = 0.0, py = 0.0, pz = 0.0;
    if (live) { px = P[3 * i]; py = P[3 * i + 1]; pz = P[3 * i + 2]; }
    double best[K];
#pragma unroll
    for (int q = 0; q < K; ++q) best[q] = INFINITY;
    for (int64_t base = rlo; base < rhi; base += MS_NT) {
        const int64_t j = base + tid;
        if (j < rhi) { sx[tid] = P[3 * j]; sy[tid] = P[3 * j + 1]; sz[tid] = P[3 * j + 2]; }
        __syncthreads();
        const int cnt = rhi - base < MS_NT ? (int)(rhi - base) : MS_NT;
        // this thread's own link inside the tile: [ta, tb)
        const int64_t a64 = lo - base, b64 = hi - base;
        const int ta = !live ? cnt : (a64 < 0 ? 0 : (a64 > cnt ? cnt : (int)a64));
        const int tb = !live ? 0 : (b64 < 0 ? 0 : (b64 > cnt ? cnt : (int)b64));
        for (int t = 0; t < cnt; ++t) {
            const double dx = sx[t] - px, dy = sy[t] - py, dz = sz[t] - pz;
            const double d = (dx * dx + dy * dy) + dz * dz;
            if (t >= ta && t < tb && d < best[K - 1]) {
                best[K - 1] = d;
#pragma unroll
                for (int q = K - 1; q > 0; --q) {                  // static indices: the list stays in registers
                    const double u = best[q - 1], v = best[q];
                    best[q - 1] = fmin(u, v);
                    best[q] = fmax(u, v);
                }
            }
        }
        __syncthreads();
    }
    if (live) {
        const int64_t nl = hi - lo;
        const int kp = nl < nb ? (int)nl : nb;
        double s = 0.0;
#pragma unroll
        for (int q = 0; q < K; ++q)
            if (q < kp) s += sqrt(best[q]);
        avg[i] = s / (double)kp;
    }
}

// fixed-order block sum: thread partials, then a halving tree in LDS (same bits on every run)
__device__ double block_sum(double v, double* red) {
    const int tid = threadIdx.x;
    red[tid] = v;
    __syncthreads();
    for (int s = MS_NT / 2; s > 0; s >>= 1) {
        if (tid < s) red[tid] += red[tid + s];
        __syncthreads();
    }
    const double r = red[0];
    __syncthreads();
    return r;
}

// one workgroup per link: mean and sample deviation of the positive averages, the threshold, the keep mask
__global__ __launch_bounds__(MS_NT) void k_sor_stats(const double* __restrict__ avg, const int64_t* __restrict__ off,
                                                     double std_ratio, double* __restrict__ thr, uint8_t* __restrict__ keep) {
    __shared__ double red[MS_NT];
    const int l = blockIdx.x, tid = threadIdx.x;
    const int64_t lo = off[l], hi = off[l + 1];
    double s = 0.0, c = 0.0;
    for (int64_t i = lo + tid; i < hi; i += MS_NT) {
        const double a = avg[i];
        if (a > 0.0) { s += a; c += 1.0; }
    }
    const double cnt = block_sum(c, red);
    const double mean = block_sum(s, red) / cnt;
    double q = 0.0;
    for (int64_t i = lo + tid; i < hi; i += MS_NT) {
        const double a = avg[i];
        if (a > 0.0) q += (a - mean) * (a - mean);
    }
    const double ss = block_sum(q, red);
    const double t = cnt >= 2.0 ? mean + std_ratio * sqrt(ss / (cnt - 1.0)) : NAN;
    if (tid == 0) thr[l] = t;
    for (int64_t i = lo + tid; i < hi; i += MS_NT) {
        const double a = avg[i];
        keep[i] = (a > 0.0 && a < t) ? 1 : 0;
    }
}

// ---------------------------------------------------------------------------------------------- (b) occupancy
__global__ __launch_bounds__(MS_NT) void k_vox_bounds(const double* __restrict__ P, const int64_t* __restrict__ off,
                                                      const uint8_t* __restrict__ keep, double vs, double* __restrict__ origin,
                                                      int32_t* __restrict__ dims, int64_t* __restrict__ n_kept) {
    __shared__ double smn[3][MS_NT], smx[3][MS_NT];
    __shared__ int scnt[MS_NT];
    const int l = blockIdx.x, tid = threadIdx.x;
    const int64_t lo = off[l], hi = off[l + 1];
    double mn[3] = {INFINITY, INFINITY, INFINITY}, mx[3] = {-INFINITY, -INFINITY, -INFINITY};
    int c = 0;
    for (int64_t i = lo + tid; i < hi; i += MS_NT) {
        if (keep && !keep[i]) continue;
        ++c;
#pragma unroll
        for (int a = 0; a < 3; ++a) { const double v = P[3 * i + a]; mn[a] = fmin(mn[a], v); mx[a] = fmax(mx[a], v); }
    }
#pragma unroll
    for (int a = 0; a < 3; ++a) { smn[a][tid] = mn[a]; smx[a][tid] = mx[a]; }
    scnt[tid] = c;
    __syncthreads();
    for (int s = MS_NT / 2; s > 0; s >>= 1) {
        if (tid < s) {
#pragma unroll
            for (int a = 0; a < 3; ++a) {
                smn[a][tid] = fmin(smn[a][tid], smn[a][tid + s]);
                smx[a][tid] = fmax(smx[a][tid], smx[a][tid + s]);
            }
            scnt[tid] += scnt[tid + s];                             // (a link has fewer than 2^31 points)
        }
        __syncthreads();
    }
    if (tid < 3) {
        const double o = smn[tid][0] - vs / 2;
        double d = floor((smx[tid][0] - o) / vs) + 1.0;             // floor((p - o) / vs) is monotone in p: the largest index
        if (!(d >= 0.0)) d = 0.0;                                   // (an empty link, or NaN input)
        if (d > 1e9) d = 1e9;
        origin[3 * l + tid] = o;
        dims[3 * l + tid] = (int32_t)d;
    }
    if (tid == 0) n_kept[l] = scnt[0];
}

__global__ __launch_bounds__(MS_NT) void k_vox_fill(const double* __restrict__ P, int64_t n, const int64_t* __restrict__ off,
                                                    int L, const uint8_t* __restrict__ keep, double vs,
                                                    const double* __restrict__ origin, const int32_t* __restrict__ dims,
                                                    const int64_t* __restrict__ node_off, uint8_t* __restrict__ occ) {
    const int64_t i = (int64_t)blockIdx.x * MS_NT + threadIdx.x;
    if (i >= n || (keep && !keep[i])) return;
    const int l = find_seg(off, L, i);
    int c[3];
#pragma unroll
    for (int a = 0; a < 3; ++a) {
        const double q = floor((P[3 * i + a] - origin[3 * l + a]) / vs);
        if (!(q >= 0.0 && q < (double)dims[3 * l + a])) return;    // cannot happen for the bounds kernel's own output
        c[a] = (int)q + 1;
    }
    const int64_t Y = dims[3 * l + 1] + 2, Z = dims[3 * l + 2] + 2;
    const int64_t g = node_off[l] + ((int64_t)c[0] * Y + c[1]) * Z + c[2];
    if (g < node_off[l + 1]) occ[g] = 1;                            // racing stores of the same byte
}

// ---------------------------------------------------------------------------------------------- (c) marching cubes
// Case mask of the cell whose low corner is node g; corners beyond the volume count as empty, and since the outer layer is
// empty a cell that does not exist gets mask 0.  A node's three owned edges are read off the same mask.
__device__ __forceinline__ int cell_mask(const uint8_t* __restrict__ occ, int64_t g, int x, int y, int z, int X, int Y, int Z) {
    int m = 0;
#pragma unroll
    for (int c = 0; c < 8; ++c) {
        const int dx = c & 1, dy = (c >> 1) & 1, dz = (c >> 2) & 1;
        if (x + dx < X && y + dy < Y && z + dz < Z && occ[g + ((int64_t)dx * Y + dy) * Z + dz]) m |= 1 << c;
    }
    return m;
}
__device__ __forceinline__ int mask_nverts(int m) { return ((m ^ (m >> 1)) & 1) + ((m ^ (m >> 2)) & 1) + ((m ^ (m >> 4)) & 1); }
// vertices the node owns on axes below `a`
__device__ __forceinline__ int mask_rank(int m, int a) {
    return (a > 0 ? ((m ^ (m >> 1)) & 1) : 0) + (a > 1 ? ((m ^ (m >> 2)) & 1) : 0);
}

struct NodeRef { int l, x, y, z, X, Y, Z; };
__device__ __forceinline__ NodeRef node_ref(const int64_t* __restrict__ node_off, const int32_t* __restrict__ dims, int L,
                                            int64_t g) {
    NodeRef r;
    r.l = find_seg(node_off, L, g);
    r.X = dims[3 * r.l] + 2; r.Y = dims[3 * r.l + 1] + 2; r.Z = dims[3 * r.l + 2] + 2;
    const uint32_t loc = (uint32_t)(g - node_off[r.l]);            // < 2^28
    r.z = loc % (uint32_t)r.Z;
    const uint32_t xy = loc / (uint32_t)r.Z;
    r.y = xy % (uint32_t)r.Y;
    r.x = xy / (uint32_t)r.Y;
    return r;
}

// counts of a tile's thread (vertices in the low half, triangles in the high half) -> exclusive scan over the block
__device__ __forceinline__ uint32_t block_excl_scan(uint32_t v, uint32_t* s, uint32_t* total) {
    const int tid = threadIdx.x;
    s[tid] = v;
    __syncthreads();
    for (int d = 1; d < MS_NT; d <<= 1) {
        const uint32_t add = tid >= d ? s[tid - d] : 0;
        __syncthreads();
        s[tid] += add;
        __syncthreads();
    }
    const uint32_t incl = s[tid];
    *total = s[MS_NT - 1];
    __syncthreads();
    return incl - v;
}

// launch 1: classify every node's cell, keep the mask, sum the tile
__global__ __launch_bounds__(MS_NT) void k_mc_classify(const uint8_t* __restrict__ occ, const int32_t* __restrict__ dims,
                                                       const int64_t* __restrict__ node_off, int L, int64_t total,
                                                       uint8_t* __restrict__ mask, uint32_t* __restrict__ tile_v,
                                                       uint32_t* __restrict__ tile_t) {
    __shared__ uint32_t s[MS_NT];
    __shared__ uint8_t ntri[256];
    ntri[threadIdx.x] = MC_TABLE[threadIdx.x][15];
    __syncthreads();
    const int64_t g0 = ((int64_t)blockIdx.x * MS_NT + threadIdx.x) * MS_ITEMS;
    uint32_t packed = 0;
    for (int k = 0; k < MS_ITEMS; ++k) {
        const int64_t g = g0 + k;
        if (g >= total) break;
        const NodeRef r = node_ref(node_off, dims, L, g);
        const int m = cell_mask(occ, g, r.x, r.y, r.z, r.X, r.Y, r.Z);
        mask[g] = (uint8_t)m;
        packed += (uint32_t)mask_nverts(m) + ((uint32_t)ntri[m] << 16);
    }
    uint32_t tot;
    block_excl_scan(packed, s, &tot);
    if (threadIdx.x == 0) { tile_v[blockIdx.x] = tot & 0xffffu; tile_t[blockIdx.x] = tot >> 16; }
}

// launch 2: one workgroup turns the tile sums into exclusive prefixes and leaves the grand totals behind them
__global__ __launch_bounds__(MS_NT) void k_mc_scan_tiles(uint32_t* __restrict__ tile_v, uint32_t* __restrict__ tile_t, int nt) {
    __shared__ uint32_t sv[MS_NT], st[MS_NT];
    const int tid = threadIdx.x, per = (nt + MS_NT - 1) / MS_NT;
    const int a = tid * per < nt ? tid * per : nt, b = a + per < nt ? a + per : nt;
    uint32_t v = 0, t = 0;
    for (int i = a; i < b; ++i) { v += tile_v[i]; t += tile_t[i]; }
    sv[tid] = v; st[tid] = t;
    __syncthreads();
    if (tid == 0) {
        uint32_t rv = 0, rt = 0;
        for (int i = 0; i < MS_NT; ++i) {
            const uint32_t cv = sv[i], ct = st[i];
            sv[i] = rv; st[i] = rt;
            rv += cv; rt += ct;
        }
        tile_v[nt] = rv; tile_t[nt] = rt;
    }
    __syncthreads();
    v = sv[tid]; t = st[tid];
    for (int i = a; i < b; ++i) {
        const uint32_t cv = tile_v[i], ct = tile_t[i];
        tile_v[i] = v; tile_t[i] = t;
        v += cv; t += ct;
    }
}

// launch 3: per-node exclusive prefixes (global over the concatenated links)
__global__ __launch_bounds__(MS_NT) void k_mc_apply(const uint8_t* __restrict__ mask, int64_t total,
                                                    const uint32_t* __restrict__ tile_v, const uint32_t* __restrict__ tile_t,
                                                    uint32_t* __restrict__ vpre, uint32_t* __restrict__ tpre) {
    __shared__ uint32_t s[MS_NT];
    __shared__ uint8_t ntri[256];
    ntri[threadIdx.x] = MC_TABLE[threadIdx.x][15];
    __syncthreads();
    const int64_t g0 = ((int64_t)blockIdx.x * MS_NT + threadIdx.x) * MS_ITEMS;
    int m[MS_ITEMS];
    uint32_t packed = 0;
#pragma unroll
    for (int k = 0; k < MS_ITEMS; ++k) {
        m[k] = g0 + k < total ? mask[g0 + k] : 0;
        packed += (uint32_t)mask_nverts(m[k]) + ((uint32_t)ntri[m[k]] << 16);
    }
    uint32_t tot;
    const uint32_t ex = block_excl_scan(packed, s, &tot);
    uint32_t v = tile_v[blockIdx.x] + (ex & 0xffffu), t = tile_t[blockIdx.x] + (ex >> 16);
#pragma unroll
    for (int k = 0; k < MS_ITEMS; ++k) {
        if (g0 + k < total) { vpre[g0 + k] = v; tpre[g0 + k] = t; }
        v += mask_nverts(m[k]);
        t += ntri[m[k]];
    }
}

__global__ void k_mc_link_totals(const int64_t* __restrict__ node_off, int L, int64_t total, const uint32_t* __restrict__ vpre,
                                 const uint32_t* __restrict__ tpre, const uint32_t* __restrict__ tile_v,
                                 const uint32_t* __restrict__ tile_t, int nt, int64_t* __restrict__ vert_off,
                                 int64_t* __restrict__ tri_off) {
    const int l = blockIdx.x * blockDim.x + threadIdx.x;
    if (l > L) return;
    const int64_t g = node_off[l];
    vert_off[l] = g < total ? vpre[g] : tile_v[nt];
    tri_off[l] = g < total ? tpre[g] : tile_t[nt];
}

// one thread per node: its owned vertices, then its cell's triangles
__global__ __launch_bounds__(MS_NT) void k_mc_emit(const uint8_t* __restrict__ mask, const int32_t* __restrict__ dims,
                                                   const int64_t* __restrict__ node_off, int L, int64_t total,
                                                   const uint32_t* __restrict__ vpre, const uint32_t* __restrict__ tpre,
                                                   const int64_t* __restrict__ vert_off, int64_t V, int64_t F,
                                                   int32_t* __restrict__ verts_h, int32_t* __restrict__ tris) {
    __shared__ uint8_t tab[256][16];
    for (int q = threadIdx.x; q < 256 * 16; q += MS_NT) tab[q >> 4][q & 15] = MC_TABLE[q >> 4][q & 15];
    __syncthreads();
    const int64_t g = (int64_t)blockIdx.x * MS_NT + threadIdx.x;
    if (g >= total) return;
    const int m = mask[g];
    if (m == 0 || m == 255) return;
    const NodeRef r = node_ref(node_off, dims, L, g);
    int64_t v = vpre[g];
    const int h[3] = {2 * r.x - 1, 2 * r.y - 1, 2 * r.z - 1};      // the node itself, half-voxel units, unpadded frame
#pragma unroll
    for (int a = 0; a < 3; ++a) {
        if (((m ^ (m >> (1 << a))) & 1) && v < V) {
            verts_h[3 * v] = h[0] + (a == 0); verts_h[3 * v + 1] = h[1] + (a == 1); verts_h[3 * v + 2] = h[2] + (a == 2);
            ++v;
        }
    }
    const int nt = tab[m][15];
    const int64_t t0 = tpre[g], v0 = vert_off[r.l];
    for (int t = 0; t < nt && t0 + t < F; ++t) {
#pragma unroll
        for (int c = 0; c < 3; ++c) {
            const int e = tab[m][3 * t + c], a = e >> 2, j = e & 3;
            const int ob = j & 1, oc = j >> 1;                      // offsets on the two other axes, in increasing order
            const int ox = a == 0 ? 0 : ob, oy = a == 0 ? ob : (a == 1 ? 0 : oc), oz = a == 2 ? 0 : oc;
            const int64_t og = g + ((int64_t)ox * r.Y + oy) * r.Z + oz;
            tris[3 * (t0 + t) + c] = (int32_t)((int64_t)vpre[og] + mask_rank(mask[og], a) - v0);
        }
    }
}

// ---------------------------------------------------------------------------------------------- (d) smoothing, (e) STL
// for every triangle (a, b, c): b joins a's neighbour multiset, c b's, a c's -- integer atomics, exact in any order
__global__ __launch_bounds__(MS_NT) void k_smooth_accum(const int32_t* __restrict__ verts_h, const int32_t* __restrict__ tris,
                                                        int64_t F, const int64_t* __restrict__ vert_off,
                                                        const int64_t* __restrict__ tri_off, int L, int64_t V,
                                                        int32_t* __restrict__ acc) {
    const int64_t f = (int64_t)blockIdx.x * MS_NT + threadIdx.x;
    if (f >= F) return;
    const int64_t v0 = vert_off[find_seg(tri_off, L, f)];
    int64_t id[3];
#pragma unroll
    for (int c = 0; c < 3; ++c) id[c] = v0 + tris[3 * f + c];
#pragma unroll
    for (int c = 0; c < 3; ++c) {
        const int64_t a = id[c], b = id[(c + 1) % 3];
        if (a < 0 || a >= V || b < 0 || b >= V) continue;
        atomicAdd(&acc[4 * a], verts_h[3 * b]);
        atomicAdd(&acc[4 * a + 1], verts_h[3 * b + 1]);
        atomicAdd(&acc[4 * a + 2], verts_h[3 * b + 2]);
        atomicAdd(&acc[4 * a + 3], 1);
    }
}

__global__ __launch_bounds__(MS_NT) void k_vertex_world(const int32_t* __restrict__ verts_h, int64_t V,
                                                        const int64_t* __restrict__ vert_off, int L,
                                                        const double* __restrict__ origin, double vs,
                                                        const int32_t* __restrict__ acc, double* __restrict__ out) {
    const int64_t v = (int64_t)blockIdx.x * MS_NT + threadIdx.x;
    if (v >= V) return;
    const int l = find_seg(vert_off, L, v);
    const double half = vs / 2;
#pragma unroll
    for (int a = 0; a < 3; ++a) {
        double h = (double)verts_h[3 * v + a];
        if (acc) h = (double)(verts_h[3 * v + a] + acc[4 * v + a]) / (double)(1 + acc[4 * v + 3]);
        out[3 * v + a] = origin[3 * l + a] + half * h;
    }
}

__global__ __launch_bounds__(MS_NT) void k_stl_records(const double* __restrict__ verts, const int32_t* __restrict__ tris,
                                                       int64_t F, const int64_t* __restrict__ vert_off,
                                                       const int64_t* __restrict__ tri_off, int L, int64_t V,
                                                       float* __restrict__ rec) {
    const int64_t f = (int64_t)blockIdx.x * MS_NT + threadIdx.x;
    if (f >= F) return;
    const int64_t v0 = vert_off[find_seg(tri_off, L, f)];
    float p[3][3];
#pragma unroll
    for (int c = 0; c < 3; ++c) {
        int64_t id = v0 + tris[3 * f + c];
        if (id < 0 || id >= V) id = 0;
#pragma unroll
        for (int a = 0; a < 3; ++a) p[c][a] = (float)verts[3 * id + a];
    }
    const double ux = (double)p[1][0] - (double)p[0][0], uy = (double)p[1][1] - (double)p[0][1], uz = (double)p[1][2] - (double)p[0][2];
    const double wx = (double)p[2][0] - (double)p[0][0], wy = (double)p[2][1] - (double)p[0][1], wz = (double)p[2][2] - (double)p[0][2];
    double nx = uy * wz - uz * wy, ny = uz * wx - ux * wz, nz = ux * wy - uy * wx;
    const double ln = sqrt((nx * nx + ny * ny) + nz * nz);
    if (ln > 0.0) { nx /= ln; ny /= ln; nz /= ln; } else { nx = ny = nz = 0.0; }
    float* o = rec + 12 * f;
    o[0] = (float)nx; o[1] = (float)ny; o[2] = (float)nz;
#pragma unroll
    for (int c = 0; c < 3; ++c)
#pragma unroll
        for (int a = 0; a < 3; ++a) o[3 + 3 * c + a] = p[c][a];
}

static int mc_tiles(int64_t total) { return (int)((total + MS_TILE - 1) / MS_TILE); }

struct McWorkspace { uint8_t* mask; uint32_t *vpre, *tpre, *tile_v, *tile_t; };
static size_t mc_layout(int64_t total, void* base, McWorkspace* w) {
    const size_t nt = (size_t)mc_tiles(total) + 1;
    size_t o = 0;
    auto take = [&](size_t bytes) { const size_t at = o; o += align_up(bytes, 256); return (char*)base + at; };
    char* a = take((size_t)total);
    char* b = take((size_t)total * 4);
    char* c = take((size_t)total * 4);
    char* d = take(nt * 4);
    char* e = take(nt * 4);
    if (w) { w->mask = (uint8_t*)a; w->vpre = (uint32_t*)b; w->tpre = (uint32_t*)c; w->tile_v = (uint32_t*)d; w->tile_t = (uint32_t*)e; }
    return o;
}

}  // namespace creg
using namespace creg;

extern "C" int creg_statistical_outlier_f64(const double* points, int64_t n, const int64_t* offsets, int32_t L,
                                            int32_t nb_neighbors, double std_ratio, double* avg, double* thr, uint8_t* keep,
                                            creg_stream_t stream) {
    CREG_REQUIRE(offsets && avg && thr && keep && (points || n == 0), "creg_statistical_outlier_f64: null pointer");
    CREG_REQUIRE(n >= 0 && L >= 1, "creg_statistical_outlier_f64: bad size (n=%lld, L=%d)", (long long)n, L);
    CREG_REQUIRE(nb_neighbors >= 1 && nb_neighbors <= 32, "creg_statistical_outlier_f64: nb_neighbors must be in [1, 32] (got %d)",
                 nb_neighbors);
    CREG_REQUIRE(std_ratio == std_ratio, "creg_statistical_outlier_f64: std_ratio is NaN");
    hipStream_t s = (hipStream_t)stream;
    if (n > 0) {
        const dim3 grid(cdiv(n, MS_NT)), block(MS_NT);
        if (nb_neighbors <= 8) hipLaunchKernelGGL(k_sor_knn<8>, grid, block, 0, s, points, n, offsets, L, nb_neighbors, avg);
        else if (nb_neighbors <= 16) hipLaunchKernelGGL(k_sor_knn<16>, grid, block, 0, s, points, n, offsets, L, nb_neighbors, avg);
        else if (nb_neighbors <= 20) hipLaunchKernelGGL(k_sor_knn<20>, grid, block, 0, s, points, n, offsets, L, nb_neighbors, avg);
        else hipLaunchKernelGGL(k_sor_knn<32>, grid, block, 0, s, points, n, offsets, L, nb_neighbors, avg);
        CREG_LAUNCH_CHECK();
    }
    hipLaunchKernelGGL(k_sor_stats, dim3(L), dim3(MS_NT), 0, s, avg, offsets, std_ratio, thr, keep);
    CREG_LAUNCH_CHECK();
    return CREG_OK;
}

extern "C" int creg_voxel_bounds_f64(const double* points, int64_t n, const int64_t* offsets, int32_t L, const uint8_t* keep,
                                     double voxel_size, double* origin, int32_t* dims, int64_t* n_kept, creg_stream_t stream) {
    CREG_REQUIRE(offsets && origin && dims && n_kept && (points || n == 0), "creg_voxel_bounds_f64: null pointer");
    CREG_REQUIRE(n >= 0 && L >= 1, "creg_voxel_bounds_f64: bad size (n=%lld, L=%d)", (long long)n, L);
    CREG_REQUIRE(voxel_size > 0.0 && std::isfinite(voxel_size), "creg_voxel_bounds_f64: voxel_size must be positive and finite (got %g)",
                 voxel_size);
    hipLaunchKernelGGL(k_vox_bounds, dim3(L), dim3(MS_NT), 0, (hipStream_t)stream, points, offsets, keep, voxel_size, origin, dims,
                       n_kept);
    CREG_LAUNCH_CHECK();
    return CREG_OK;
}

extern "C" int creg_voxel_layout(const int32_t* dims, const int64_t* n_kept, int32_t L, int64_t* node_offsets) {
    CREG_REQUIRE(dims && n_kept && node_offsets && L >= 1, "creg_voxel_layout: bad argument");
    int64_t total = 0;
    node_offsets[0] = 0;
    for (int l = 0; l < L; ++l) {
        CREG_REQUIRE(n_kept[l] > 0, "creg_voxel_layout: link %d has no point left after the outlier filter", l);
        int64_t nodes = 1;
        for (int a = 0; a < 3; ++a) {
            const int64_t d = (int64_t)dims[3 * l + a] + 2;
            CREG_REQUIRE(dims[3 * l + a] >= 1 && d <= MS_MAX_AXIS,
                         "creg_voxel_layout: link %d needs %lld nodes on axis %d (limit %d): use a larger voxel_size", l, (long long)d,
                         a, MS_MAX_AXIS);
            nodes *= d;
        }
        total += nodes;
        CREG_REQUIRE(total <= MS_MAX_NODES, "creg_voxel_layout: more than 2^28 grid nodes in total (at link %d): use a larger voxel_size",
                     l);
        node_offsets[l + 1] = total;
    }
    return CREG_OK;
}

extern "C" int creg_voxel_fill_f64(const double* points, int64_t n, const int64_t* offsets, int32_t L, const uint8_t* keep,
                                   double voxel_size, const double* origin, const int32_t* dims, const int64_t* node_offsets,
                                   int64_t total_nodes, uint8_t* occ, creg_stream_t stream) {
    CREG_REQUIRE(points && offsets && origin && dims && node_offsets && occ, "creg_voxel_fill_f64: null pointer");
    CREG_REQUIRE(n >= 1 && L >= 1 && total_nodes >= 1 && total_nodes <= MS_MAX_NODES, "creg_voxel_fill_f64: bad size (n=%lld, L=%d, nodes=%lld)",
                 (long long)n, L, (long long)total_nodes);
    CREG_REQUIRE(voxel_size > 0.0 && std::isfinite(voxel_size), "creg_voxel_fill_f64: voxel_size must be positive and finite (got %g)",
                 voxel_size);
    CREG_HIP(hipMemsetAsync(occ, 0, (size_t)total_nodes, (hipStream_t)stream));
    hipLaunchKernelGGL(k_vox_fill, dim3(cdiv(n, MS_NT)), dim3(MS_NT), 0, (hipStream_t)stream, points, n, offsets, L, keep, voxel_size,
                       origin, dims, node_offsets, occ);
    CREG_LAUNCH_CHECK();
    return CREG_OK;
}

extern "C" size_t creg_mc_workspace_bytes(int64_t total_nodes) {
    return total_nodes >= 1 && total_nodes <= MS_MAX_NODES ? mc_layout(total_nodes, nullptr, nullptr) : 0;
}

extern "C" int creg_mc_count_u8(const uint8_t* occ, const int32_t* dims, const int64_t* node_offsets, int32_t L,
                                int64_t total_nodes, int64_t* vert_offsets, int64_t* tri_offsets, void* workspace,
                                size_t workspace_bytes, creg_stream_t stream) {
    CREG_REQUIRE(occ && dims && node_offsets && vert_offsets && tri_offsets && workspace, "creg_mc_count_u8: null pointer");
    CREG_REQUIRE(L >= 1 && total_nodes >= 1 && total_nodes <= MS_MAX_NODES, "creg_mc_count_u8: bad size (L=%d, nodes=%lld)", L,
                 (long long)total_nodes);
    McWorkspace w;
    CREG_REQUIRE(workspace_bytes >= mc_layout(total_nodes, workspace, &w), "creg_mc_count_u8: workspace too small");
    hipStream_t s = (hipStream_t)stream;
    const int nt = mc_tiles(total_nodes);
    hipLaunchKernelGGL(k_mc_classify, dim3(nt), dim3(MS_NT), 0, s, occ, dims, node_offsets, L, total_nodes, w.mask, w.tile_v, w.tile_t);
    CREG_LAUNCH_CHECK();
    hipLaunchKernelGGL(k_mc_scan_tiles, dim3(1), dim3(MS_NT), 0, s, w.tile_v, w.tile_t, nt);
    CREG_LAUNCH_CHECK();
    hipLaunchKernelGGL(k_mc_apply, dim3(nt), dim3(MS_NT), 0, s, w.mask, total_nodes, w.tile_v, w.tile_t, w.vpre, w.tpre);
    CREG_LAUNCH_CHECK();
    hipLaunchKernelGGL(k_mc_link_totals, dim3(cdiv(L + 1, 64)), dim3(64), 0, s, node_offsets, L, total_nodes, w.vpre, w.tpre, w.tile_v,
                       w.tile_t, nt, vert_offsets, tri_offsets);
    CREG_LAUNCH_CHECK();
    return CREG_OK;
}

extern "C" int creg_mc_emit_i32(const int32_t* dims, const int64_t* node_offsets, int32_t L, int64_t total_nodes,
                                const int64_t* vert_offsets, int64_t V, int64_t F, int32_t* verts_h, int32_t* tris,
                                void* workspace, size_t workspace_bytes, creg_stream_t stream) {
    CREG_REQUIRE(dims && node_offsets && vert_offsets && workspace && (verts_h || V == 0) && (tris || F == 0),
                 "creg_mc_emit_i32: null pointer");
    CREG_REQUIRE(L >= 1 && total_nodes >= 1 && total_nodes <= MS_MAX_NODES && V >= 0 && F >= 0, "creg_mc_emit_i32: bad size");
    McWorkspace w;
    CREG_REQUIRE(workspace_bytes >= mc_layout(total_nodes, workspace, &w), "creg_mc_emit_i32: workspace too small");
    hipLaunchKernelGGL(k_mc_emit, dim3(cdiv(total_nodes, MS_NT)), dim3(MS_NT), 0, (hipStream_t)stream, w.mask, dims, node_offsets, L,
                       total_nodes, w.vpre, w.tpre, vert_offsets, V, F, verts_h, tris);
    CREG_LAUNCH_CHECK();
    return CREG_OK;
}

extern "C" size_t creg_mesh_finish_workspace_bytes(int64_t V) { return V > 0 ? (size_t)V * 16 : 0; }

extern "C" int creg_mesh_finish_f64(const int32_t* verts_h, int64_t V, const int32_t* tris, int64_t F, const int64_t* vert_offsets,
                                    const int64_t* tri_offsets, int32_t L, const double* origin, double voxel_size, int32_t smooth,
                                    double* vertices, float* stl_records, void* workspace, size_t workspace_bytes,
                                    creg_stream_t stream) {
    CREG_REQUIRE(vert_offsets && tri_offsets && origin && L >= 1 && V >= 0 && F >= 0, "creg_mesh_finish_f64: bad argument");
    CREG_REQUIRE((V == 0 || (verts_h && vertices)) && (F == 0 || (tris && stl_records && V > 0)), "creg_mesh_finish_f64: null pointer");
    CREG_REQUIRE(voxel_size > 0.0 && std::isfinite(voxel_size), "creg_mesh_finish_f64: voxel_size must be positive and finite (got %g)",
                 voxel_size);
    CREG_REQUIRE(!smooth || V == 0 || (workspace && workspace_bytes >= (size_t)V * 16), "creg_mesh_finish_f64: workspace too small");
    hipStream_t s = (hipStream_t)stream;
    int32_t* acc = smooth ? (int32_t*)workspace : nullptr;
    if (V == 0) return CREG_OK;
    if (smooth) {
        CREG_HIP(hipMemsetAsync(acc, 0, (size_t)V * 16, s));
        if (F > 0) {
            hipLaunchKernelGGL(k_smooth_accum, dim3(cdiv(F, MS_NT)), dim3(MS_NT), 0, s, verts_h, tris, F, vert_offsets, tri_offsets, L, V,
                               acc);
            CREG_LAUNCH_CHECK();
        }
    }
    hipLaunchKernelGGL(k_vertex_world, dim3(cdiv(V, MS_NT)), dim3(MS_NT), 0, s, verts_h, V, vert_offsets, L, origin, voxel_size, acc,
                       vertices);
    CREG_LAUNCH_CHECK();
    if (F > 0) {
        hipLaunchKernelGGL(k_stl_records, dim3(cdiv(F, MS_NT)), dim3(MS_NT), 0, s, vertices, tris, F, vert_offsets, tri_offsets, L, V,
                           stl_records);
        CREG_LAUNCH_CHECK();
    }
    return CREG_OK;
}
