// hull.hip -- N4: exact convex hulls of lattice point sets, every link of a call in one launch (DESIGN N4, "collision hulls").
// The mesher's unsmoothed vertices are integers in half-voxel units, so every predicate here is an exact int64 determinant:
// |v| <= 16383 keeps a normal component below 2^31, a determinant below 6 * 2^45.  No floating point decides anything; the only
// floating-point work is the STL record of a finished face.  The contract is this project's own (include/creg.h has it in full).
//
// Quickhull, one workgroup of 256 threads per link, everything but a few words of LDS in the link's own slice of the workspace:
//   seed      p0 = the lexicographically smallest point, p1 = the farthest from p0, p2 = the farthest from the line p0 p1,
//             p3 = the farthest from the plane p0 p1 p2 -- each an exact integer maximum, ties to the smallest index.  A zero
//             maximum is the link's status (identical / collinear / coplanar points).
//   outside   a point strictly above a face (det > 0) is kept in the live list with that face and its determinant; a point
//             above no face is inside for good and leaves the list.  The list stays in ascending point order.
//   round     apex = the live point of the lowest face slot with the largest determinant (ties: smallest index).  Every live
//             face with det(apex) >= 0 is visible -- coplanar faces are absorbed, so a new face (a, b, apex) over a horizon edge
//             (a, b) cannot be collinear: its other side has det < 0.  The horizon edges, in (face slot, edge) order, take the
//             slots of the dead faces in ascending order, then fresh ones.  Neighbours across (b, apex) and (apex, a) come from
//             two per-vertex tables and are verified.  Only the points of dead faces are tested again, against the new faces only.
//   bounds    a round removes its apex from the list, so a link of n points runs at most n rounds; a visible region of v faces
//             is a disk with at most v + 2 boundary edges, so at most 2 fresh slots per round: 2 n + 4 slots never run out.
//             Every one of these is checked and has a status of its own; no loop waits on another thread's progress.
// Ordered compaction (ballot + popcount ranks) keeps every list in a fixed order; there are no atomics at all.
#include <climits>
#include <cmath>
#include "creg_common.h"

namespace creg {

constexpr int HL_NT = 256;
constexpr int HL_NW = HL_NT / 64;
constexpr int HL_MAX_COORD = 16383;
constexpr int64_t HL_MAX_POINTS = (int64_t)1 << 28;
constexpr int HL_MAX_LINKS = 1 << 20;

// 64 bytes.  Edge k runs v[k] -> v[(k+1)%3], nb[k] is the face across it.  det(p) = n . p - d0 = det(b-a, c-a, p-a).
struct HullFace {
    int32_t v[3], nb[3], alive, mark;
    int64_t nx, ny, nz, d0;
};

struct HullWs {
    int32_t *li, *lf;       // live list: point, its face slot
    int64_t* ld;            //            its determinant there
    int32_t *sof, *eof;     // per vertex: the new face whose horizon edge starts / ends there
    HullFace* face;
    int32_t *vlist, *hslot; // visible slots of the round; the slot of each new face
    int32_t* hrec;          // 4 per horizon edge: a, b, the face beyond, its edge back
    int32_t* meta;          // 2 per link: slots in use, status
    size_t total;
};

static inline size_t hull_slots(int64_t n, int64_t L) { return (size_t)(2 * n + 4 * L); }
static HullWs hull_layout(int64_t n, int64_t L, void* base) {
    HullWs w;
    size_t o = 0;
    auto take = [&](size_t bytes) { const size_t at = o; o += align_up(bytes, 256); return (char*)base + at; };
    const size_t np = (size_t)(n > 0 ? n : 1), ns = hull_slots(n, L);
    w.li = (int32_t*)take(np * 4);
    w.lf = (int32_t*)take(np * 4);
    w.ld = (int64_t*)take(np * 8);
    w.sof = (int32_t*)take(np * 4);
    w.eof = (int32_t*)take(np * 4);
    w.face = (HullFace*)take(ns * sizeof(HullFace));
    w.vlist = (int32_t*)take(ns * 4);
    w.hslot = (int32_t*)take(ns * 4);
    w.hrec = (int32_t*)take(ns * 16);
    w.meta = (int32_t*)take((size_t)L * 8);
    w.total = o;
    return w;
}

// The workgroup's barrier for this file.  Every list here lives in global memory and is handed from thread to thread across
// barriers, so the barrier is stated with fences over every address space at workgroup scope: the compiler may move neither
// a global store below it nor a global load above it (the waves of a workgroup share one vector L1, which keeps their order).
__device__ __forceinline__ void hull_sync() {
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "workgroup");
    __builtin_amdgcn_s_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "workgroup");
}

// minimise a, then maximise b, then minimise i
struct HullKey { unsigned long long a; long long b; int i; };
__device__ __forceinline__ bool hull_better(const HullKey& x, const HullKey& y) {
    if (x.a != y.a) return x.a < y.a;
    if (x.b != y.b) return x.b > y.b;
    return x.i < y.i;
}
__device__ __forceinline__ HullKey hull_no_key() { return HullKey{~0ull, LLONG_MIN, INT_MAX}; }

// the best key of the block, in every thread.  s_k: HL_NW keys.
__device__ HullKey hull_best(HullKey k, HullKey* s_k) {
#pragma unroll
    for (int off = 32; off >= 1; off >>= 1) {
        HullKey o;
        o.a = __shfl_xor(k.a, off, 64);
        o.b = __shfl_xor(k.b, off, 64);
        o.i = __shfl_xor(k.i, off, 64);
        if (hull_better(o, k)) k = o;
    }
    if ((threadIdx.x & 63) == 0) s_k[threadIdx.x >> 6] = k;
    hull_sync();
    HullKey r = s_k[0];
#pragma unroll
    for (int w = 1; w < HL_NW; ++w)
        if (hull_better(s_k[w], r)) r = s_k[w];
    hull_sync();
    return r;
}

// the number of flagged threads below this one, and the block's count.  s_c: HL_NW ints.  Two barriers: what a thread wrote
// before the call is visible to the block after it.
__device__ int hull_rank(bool flag, int* s_c, int& total) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const unsigned long long mask = __ballot(flag);
    if (lane == 0) s_c[wave] = __popcll(mask);
    hull_sync();
    int base = 0, tot = 0;
#pragma unroll
    for (int w = 0; w < HL_NW; ++w) {
        if (w < wave) base += s_c[w];
        tot += s_c[w];
    }
    hull_sync();
    total = tot;
    return base + __popcll(mask & ((1ull << lane) - 1ull));
}

// whether any thread of the block passes a non-zero flag, in every thread.  s_c: HL_NW ints.  Two barriers, as hull_rank.
__device__ bool hull_any(int flag, int* s_c) {
    const unsigned long long mask = __ballot(flag != 0);
    if ((threadIdx.x & 63) == 0) s_c[threadIdx.x >> 6] = mask != 0ull;
    hull_sync();
    int any = 0;
#pragma unroll
    for (int w = 0; w < HL_NW; ++w) any |= s_c[w];
    hull_sync();
    return any != 0;
}

__device__ __forceinline__ void hull_plane(HullFace& f, const int32_t* __restrict__ P) {
    const int32_t *A = P + 3 * (int64_t)f.v[0], *B = P + 3 * (int64_t)f.v[1], *C = P + 3 * (int64_t)f.v[2];
    const int64_t ux = (int64_t)B[0] - A[0], uy = (int64_t)B[1] - A[1], uz = (int64_t)B[2] - A[2];
    const int64_t wx = (int64_t)C[0] - A[0], wy = (int64_t)C[1] - A[1], wz = (int64_t)C[2] - A[2];
    f.nx = uy * wz - uz * wy;
    f.ny = uz * wx - ux * wz;
    f.nz = ux * wy - uy * wx;
    f.d0 = f.nx * A[0] + f.ny * A[1] + f.nz * A[2];
}
__device__ __forceinline__ int64_t hull_det(const HullFace* f, int64_t x, int64_t y, int64_t z) {
    return f->nx * x + f->ny * y + f->nz * z - f->d0;
}

// One workgroup per link.  The workspace pointers are read and written across barriers by this workgroup: no __restrict__.
__global__ __launch_bounds__(HL_NT) void k_hull_build(const int32_t* __restrict__ pts, int64_t n, const int64_t* __restrict__ off,
                                                      HullWs w, int32_t* __restrict__ status, int32_t* __restrict__ face_count) {
    __shared__ HullKey s_k[HL_NW];
    __shared__ int s_c[HL_NW];
    const int tid = threadIdx.x, l = blockIdx.x;
    const int64_t lo = off[l], hi = off[l + 1];
    int st = CREG_HULL_OK, nslots = 0, nalive = 0;
    if (lo < 0 || hi < lo || hi > n) st = CREG_HULL_EOFFSETS;      // uniform
    else if (hi - lo < 4) st = CREG_HULL_EFEW;
    if (st == CREG_HULL_OK) {
        const int nl = (int)(hi - lo);
        const int32_t* P = pts + 3 * lo;
        int32_t *li = w.li + lo, *lf = w.lf + lo, *sof = w.sof + lo, *eof = w.eof + lo;
        int64_t* ld = w.ld + lo;
        const int64_t fbase = 2 * lo + 4 * (int64_t)l;
        const int cap = 2 * nl + 4;
        HullFace* F = w.face + fbase;
        int32_t *vlist = w.vlist + fbase, *hslot = w.hslot + fbase, *hrec = w.hrec + 4 * fbase;
        do {                                                       // left by break with st set; every condition is uniform
            int bad = 0;
            for (int i = tid; i < nl; i += HL_NT)
#pragma unroll
                for (int a = 0; a < 3; ++a) bad |= (P[3 * i + a] > HL_MAX_COORD || P[3 * i + a] < -HL_MAX_COORD);
            if (hull_any(bad, s_c)) { st = CREG_HULL_ERANGE; break; }
            // ---- seed
            HullKey k = hull_no_key();
            for (int i = tid; i < nl; i += HL_NT) {
                const HullKey c{((unsigned long long)(P[3 * i] + 16384) << 32) | ((unsigned long long)(P[3 * i + 1] + 16384) << 16) |
                                    (unsigned long long)(P[3 * i + 2] + 16384), 0, i};
                if (hull_better(c, k)) k = c;
            }
            const int p0 = hull_best(k, s_k).i;
            const int64_t ax = P[3 * p0], ay = P[3 * p0 + 1], az = P[3 * p0 + 2];
            k = hull_no_key();
            for (int i = tid; i < nl; i += HL_NT) {
                const int64_t dx = P[3 * i] - ax, dy = P[3 * i + 1] - ay, dz = P[3 * i + 2] - az;
                const HullKey c{~(unsigned long long)(dx * dx + dy * dy + dz * dz), 0, i};
                if (hull_better(c, k)) k = c;
            }
            k = hull_best(k, s_k);
            if (~k.a == 0ull) { st = CREG_HULL_EIDENTICAL; break; }
            int p1 = k.i;
            const int64_t ux = P[3 * p1] - ax, uy = P[3 * p1 + 1] - ay, uz = P[3 * p1 + 2] - az;
            k = hull_no_key();
            for (int i = tid; i < nl; i += HL_NT) {
                const int64_t dx = P[3 * i] - ax, dy = P[3 * i + 1] - ay, dz = P[3 * i + 2] - az;
                const int64_t cx = uy * dz - uz * dy, cy = uz * dx - ux * dz, cz = ux * dy - uy * dx;     // each below 2^31
                const HullKey c{~((unsigned long long)(cx * cx) + (unsigned long long)(cy * cy) + (unsigned long long)(cz * cz)), 0, i};
                if (hull_better(c, k)) k = c;
            }
            k = hull_best(k, s_k);
            if (~k.a == 0ull) { st = CREG_HULL_ECOLLINEAR; break; }
            int p2 = k.i;
            int64_t nx, ny, nz;
            {
                const int64_t wx = P[3 * p2] - ax, wy = P[3 * p2 + 1] - ay, wz = P[3 * p2 + 2] - az;
                nx = uy * wz - uz * wy; ny = uz * wx - ux * wz; nz = ux * wy - uy * wx;
            }
            k = hull_no_key();
            for (int i = tid; i < nl; i += HL_NT) {
                const int64_t d = nx * (P[3 * i] - ax) + ny * (P[3 * i + 1] - ay) + nz * (P[3 * i + 2] - az);
                const HullKey c{~(unsigned long long)(d < 0 ? -d : d), 0, i};
                if (hull_better(c, k)) k = c;
            }
            k = hull_best(k, s_k);
            if (~k.a == 0ull) { st = CREG_HULL_ECOPLANAR; break; }
            const int p3 = k.i;
            if (nx * (P[3 * p3] - ax) + ny * (P[3 * p3 + 1] - ay) + nz * (P[3 * p3 + 2] - az) > 0) { const int t = p1; p1 = p2; p2 = t; }
            // p3 is now strictly below (p0, p1, p2): the faces (a,b,c), (a,d,b), (b,d,c), (c,d,a) are outward
            if (tid < 4) {
                const int a = p0, b = p1, c = p2, d = p3;
                const int V[4][3] = {{a, b, c}, {a, d, b}, {b, d, c}, {c, d, a}};
                const int N[4][3] = {{1, 2, 3}, {3, 2, 0}, {1, 3, 0}, {2, 1, 0}};
                HullFace f;
#pragma unroll
                for (int q = 0; q < 3; ++q) { f.v[q] = V[tid][q]; f.nb[q] = N[tid][q]; }
                f.alive = 1;
                f.mark = 0;
                hull_plane(f, P);
                F[tid] = f;
            }
            nslots = nalive = 4;
            hull_sync();
            int m = 0;
            for (int base = 0; base < nl; base += HL_NT) {
                const int i = base + tid;
                int fs = -1;
                int64_t fd = 0;
                if (i < nl) {
                    const int64_t x = P[3 * i], y = P[3 * i + 1], z = P[3 * i + 2];
                    for (int s = 0; s < 4 && fs < 0; ++s) {
                        const int64_t d = hull_det(&F[s], x, y, z);
                        if (d > 0) { fs = s; fd = d; }
                    }
                }
                int tot;
                const int pos = m + hull_rank(fs >= 0, s_c, tot);
                if (fs >= 0) { li[pos] = i; lf[pos] = fs; ld[pos] = fd; }
                m += tot;
            }
            hull_sync();
            // ---- rounds
            for (int round = 1; m > 0; ++round) {
                if (round > nl) { st = CREG_HULL_EBOUND; break; }
                k = hull_no_key();
                for (int j = tid; j < m; j += HL_NT) {
                    const HullKey c{(unsigned long long)lf[j], ld[j], li[j]};
                    if (hull_better(c, k)) k = c;
                }
                const int apex = hull_best(k, s_k).i;
                const int64_t px = P[3 * apex], py = P[3 * apex + 1], pz = P[3 * apex + 2];
                int v = 0;
                for (int base = 0; base < nslots; base += HL_NT) {
                    const int s = base + tid;
                    bool vis = false;
                    if (s < nslots && F[s].alive && hull_det(&F[s], px, py, pz) >= 0) { vis = true; F[s].mark = round; }
                    int tot;
                    const int pos = v + hull_rank(vis, s_c, tot);
                    if (vis) vlist[pos] = s;
                    v += tot;
                }
                hull_sync();
                int h = 0;
                bad = 0;
                for (int64_t base = 0; base < 3 * (int64_t)v; base += HL_NT) {
                    const int64_t j = base + tid;
                    bool hor = false;
                    int f = 0, e = 0, g = 0;
                    if (j < 3 * (int64_t)v) {
                        f = vlist[j / 3]; e = (int)(j % 3); g = F[f].nb[e];
                        if (g < 0 || g >= nslots || !F[g].alive) bad = 1;
                        else hor = F[g].mark != round;
                    }
                    int tot;
                    const int pos = h + hull_rank(hor, s_c, tot);
                    if (hor) {
                        const int a = F[f].v[e], b = F[f].v[(e + 1) % 3];
                        int kg = -1;
#pragma unroll
                        for (int q = 0; q < 3; ++q)
                            if (F[g].v[q] == b && F[g].v[(q + 1) % 3] == a) kg = q;
                        if (kg < 0 || pos >= cap) bad = 1;
                        else { hrec[4 * pos] = a; hrec[4 * pos + 1] = b; hrec[4 * pos + 2] = g; hrec[4 * pos + 3] = kg; }
                    }
                    h += tot;
                }
                if (hull_any(bad, s_c) || h < 3 || h > v + 2) { st = CREG_HULL_ETOPOLOGY; break; }
                const int grown = nslots + (h > v ? h - v : 0);
                if (grown > cap) { st = CREG_HULL_EWORKSPACE; break; }
                for (int r = tid; r < h; r += HL_NT) {
                    const int s = r < v ? vlist[r] : nslots + (r - v);
                    const int a = hrec[4 * r], b = hrec[4 * r + 1], g = hrec[4 * r + 2], kg = hrec[4 * r + 3];
                    HullFace f;
                    f.v[0] = a; f.v[1] = b; f.v[2] = apex;
                    f.nb[0] = g; f.nb[1] = -1; f.nb[2] = -1;
                    f.alive = 1;
                    f.mark = round;
                    hull_plane(f, P);
                    F[s] = f;
                    F[g].nb[kg] = s;
                    hslot[r] = s;
                    sof[a] = s;
                    eof[b] = s;
                }
                for (int r = h + tid; r < v; r += HL_NT) F[vlist[r]].alive = 0;
                hull_sync();
                bad = 0;
                for (int r = tid; r < h; r += HL_NT) {
                    const int s = hslot[r], a = hrec[4 * r], b = hrec[4 * r + 1];
                    const int n1 = sof[b], n2 = eof[a];
                    if (n1 < 0 || n1 >= grown || n2 < 0 || n2 >= grown) { bad = 1; continue; }
                    if (!F[n1].alive || F[n1].v[0] != b || F[n1].v[2] != apex || !F[n2].alive || F[n2].v[1] != a || F[n2].v[2] != apex) bad = 1;
                    F[s].nb[1] = n1;
                    F[s].nb[2] = n2;
                }
                if (hull_any(bad, s_c)) { st = CREG_HULL_ETOPOLOGY; break; }
                nalive += h - v;
                nslots = grown;
                int m2 = 0;
                for (int base = 0; base < m; base += HL_NT) {
                    const int j = base + tid;
                    bool keep = false;
                    int i = 0, f = 0;
                    int64_t d = 0;
                    if (j < m) {
                        i = li[j]; f = lf[j]; d = ld[j];
                        if (F[f].mark != round) keep = true;
                        else if (i != apex) {
                            const int64_t x = P[3 * i], y = P[3 * i + 1], z = P[3 * i + 2];
                            for (int r = 0; r < h && !keep; ++r) {
                                const int s = hslot[r];
                                const int64_t t = hull_det(&F[s], x, y, z);
                                if (t > 0) { f = s; d = t; keep = true; }
                            }
                        }
                    }
                    int tot;
                    const int pos = m2 + hull_rank(keep, s_c, tot);      // its barriers: the chunk is read before it is written
                    if (keep) { li[pos] = i; lf[pos] = f; ld[pos] = d; }
                    m2 += tot;
                }
                hull_sync();
                m = m2;
            }
        } while (false);
    }
    if (tid == 0) {
        status[l] = st;
        face_count[l] = st == CREG_HULL_OK ? nalive : 0;
        w.meta[2 * l] = st == CREG_HULL_OK ? nslots : 0;
        w.meta[2 * l + 1] = st;
    }
}

// One workgroup per link: the live faces in slot order -> triangles and, with an origin, STL records.
__global__ __launch_bounds__(HL_NT) void k_hull_emit(const int32_t* __restrict__ pts, int64_t n, const int64_t* __restrict__ off,
                                                     HullWs w, const int64_t* __restrict__ tri_off, int64_t F_total,
                                                     const double* __restrict__ origin, double vs, int32_t* __restrict__ tris,
                                                     float* __restrict__ rec) {
    __shared__ int s_c[HL_NW];
    const int tid = threadIdx.x, l = blockIdx.x;
    const int64_t lo = off[l], hi = off[l + 1];
    if (lo < 0 || hi < lo || hi > n) return;
    const int nslots = w.meta[2 * l];
    int64_t t0 = tri_off[l], t1 = tri_off[l + 1];
    if (t0 < 0 || t1 < t0 || t1 > F_total) return;
    if (nslots < 0 || nslots > 2 * (hi - lo) + 4) return;
    const int32_t* P = pts + 3 * lo;
    const HullFace* F = w.face + (2 * lo + 4 * (int64_t)l);
    const double half = vs / 2;
    int cnt = 0;
    for (int base = 0; base < nslots; base += HL_NT) {
        const int s = base + tid;
        const bool live = s < nslots && F[s].alive;
        int tot;
        const int64_t t = t0 + cnt + hull_rank(live, s_c, tot);
        cnt += tot;
        if (!live || t >= t1) continue;
        int id[3];
#pragma unroll
        for (int c = 0; c < 3; ++c) { id[c] = F[s].v[c]; tris[3 * t + c] = id[c]; }
        if (!rec) continue;
        float p[3][3];
#pragma unroll
        for (int c = 0; c < 3; ++c)
#pragma unroll
            for (int a = 0; a < 3; ++a) p[c][a] = (float)(origin[3 * l + a] + half * (double)P[3 * (int64_t)id[c] + a]);
        const double ux = (double)p[1][0] - (double)p[0][0], uy = (double)p[1][1] - (double)p[0][1], uz = (double)p[1][2] - (double)p[0][2];
        const double wx = (double)p[2][0] - (double)p[0][0], wy = (double)p[2][1] - (double)p[0][1], wz = (double)p[2][2] - (double)p[0][2];
        double nx = uy * wz - uz * wy, ny = uz * wx - ux * wz, nz = ux * wy - uy * wx;
        const double ln = sqrt((nx * nx + ny * ny) + nz * nz);
        if (ln > 0.0) { nx /= ln; ny /= ln; nz /= ln; } else { nx = ny = nz = 0.0; }
        float* o = rec + 12 * t;
        o[0] = (float)nx; o[1] = (float)ny; o[2] = (float)nz;
#pragma unroll
        for (int c = 0; c < 3; ++c)
#pragma unroll
            for (int a = 0; a < 3; ++a) o[3 + 3 * c + a] = p[c][a];
    }
}

static bool hull_sizes_ok(int64_t n, int32_t L) { return n >= 0 && n <= HL_MAX_POINTS && L >= 1 && L <= HL_MAX_LINKS; }

}  // namespace creg
using namespace creg;

extern "C" size_t creg_lattice_hull_workspace_bytes(int64_t n, int32_t n_links) {
    return hull_sizes_ok(n, n_links) ? hull_layout(n, n_links, nullptr).total : 0;
}

extern "C" int creg_lattice_hull_i32(const int32_t* pts, int64_t n, const int64_t* offsets, const int64_t* offsets_host,
                                     int32_t n_links, int64_t max_abs, int32_t* status, int32_t* face_count, void* workspace,
                                     size_t workspace_bytes, creg_stream_t stream) {
    CREG_REQUIRE(hull_sizes_ok(n, n_links), "creg_lattice_hull_i32: bad size (n=%lld, limit 2^28; n_links=%d, limit 2^20)", (long long)n,
                 (int)n_links);
    CREG_REQUIRE(offsets && offsets_host && status && face_count && workspace && (pts || n == 0), "creg_lattice_hull_i32: null pointer");
    CREG_REQUIRE(offsets_host[0] == 0 && offsets_host[n_links] == n,
                 "creg_lattice_hull_i32: offsets must run from 0 to n (got %lld .. %lld, n=%lld)", (long long)offsets_host[0],
                 (long long)offsets_host[n_links], (long long)n);
    for (int32_t l = 0; l < n_links; ++l)
        CREG_REQUIRE(offsets_host[l + 1] >= offsets_host[l], "creg_lattice_hull_i32: offsets decrease at link %d (%lld after %lld)", (int)l,
                     (long long)offsets_host[l + 1], (long long)offsets_host[l]);
    CREG_REQUIRE(max_abs <= HL_MAX_COORD, "creg_lattice_hull_i32: a coordinate of magnitude %lld is beyond the limit of %d",
                 (long long)max_abs, HL_MAX_COORD);
    const HullWs w = hull_layout(n, n_links, workspace);
    CREG_REQUIRE(workspace_bytes >= w.total, "creg_lattice_hull_i32: workspace of %zu bytes, %zu needed", workspace_bytes, w.total);
    hipLaunchKernelGGL(k_hull_build, dim3((unsigned)n_links), dim3(HL_NT), 0, (hipStream_t)stream, pts, n, offsets, w, status, face_count);
    CREG_LAUNCH_CHECK();
    return CREG_OK;
}

extern "C" int creg_lattice_hull_emit_i32(const int32_t* pts, int64_t n, const int64_t* offsets, int32_t n_links,
                                          const int64_t* tri_offsets, int64_t n_tri, const double* origin, double voxel_size,
                                          int32_t* triangles, float* stl_records, void* workspace, size_t workspace_bytes,
                                          creg_stream_t stream) {
    CREG_REQUIRE(hull_sizes_ok(n, n_links) && n_tri >= 0 && n_tri <= 2 * n, "creg_lattice_hull_emit_i32: bad size (n=%lld, n_links=%d, n_tri=%lld)",
                 (long long)n, (int)n_links, (long long)n_tri);
    CREG_REQUIRE(offsets && tri_offsets && workspace && (pts || n == 0) && (triangles || n_tri == 0),
                 "creg_lattice_hull_emit_i32: null pointer");
    CREG_REQUIRE(!stl_records || (origin && voxel_size > 0.0 && std::isfinite(voxel_size)),
                 "creg_lattice_hull_emit_i32: stl_records need an origin and a positive, finite voxel_size (got %g)", voxel_size);
    const HullWs w = hull_layout(n, n_links, workspace);
    CREG_REQUIRE(workspace_bytes >= w.total, "creg_lattice_hull_emit_i32: workspace of %zu bytes, %zu needed", workspace_bytes, w.total);
    if (n_tri == 0) return CREG_OK;
    hipLaunchKernelGGL(k_hull_emit, dim3((unsigned)n_links), dim3(HL_NT), 0, (hipStream_t)stream, pts, n, offsets, w, tri_offsets, n_tri,
                       origin, voxel_size, triangles, stl_records);
    CREG_LAUNCH_CHECK();
    return CREG_OK;
}
