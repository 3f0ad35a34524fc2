// mesh_dist.h -- the distance arithmetic that clearance.hip (mesh against mesh) and point_mesh.hip (points against a mesh) share:
// the box gap both cull and gate by, and the vertex-triangle term.  The text is clearance.hip's, moved here unchanged; the contract
// of every function is in include/creg.h under "Link clearance".
#pragma once
#include "mesh_pair.h"

namespace creg {

__device__ __forceinline__ double gap2(const Box& a, const Box& b) {
    double g[3];
#pragma unroll
    for (int k = 0; k < 3; ++k) g[k] = fmax(0.0, fmax(a.lo[k] - b.hi[k], b.lo[k] - a.hi[k]));
    return (g[0] * g[0] + g[1] * g[1]) + g[2] * g[2];
}
__device__ __forceinline__ double dot3(const double* u, const double* v) { return (u[0] * v[0] + u[1] * v[1]) + u[2] * v[2]; }

// squared distance of p from the triangle (a, b, c): the point's Voronoi region picks a vertex, an edge or the face
__device__ __forceinline__ double pt_tri2(const double* p, const double* a, const double* b, const double* c) {
    double ab[3], ac[3], ap[3], bp[3], cp[3], q[3];
#pragma unroll
    for (int k = 0; k < 3; ++k) { ab[k] = b[k] - a[k]; ac[k] = c[k] - a[k]; ap[k] = p[k] - a[k]; bp[k] = p[k] - b[k]; cp[k] = p[k] - c[k]; }
    const double d1 = dot3(ab, ap), d2 = dot3(ac, ap), d3 = dot3(ab, bp), d4 = dot3(ac, bp), d5 = dot3(ab, cp), d6 = dot3(ac, cp);
    if (d1 <= 0.0 && d2 <= 0.0) return dot3(ap, ap);                       // vertex a
    if (d3 >= 0.0 && d4 <= d3) return dot3(bp, bp);                         // vertex b
    if (d6 >= 0.0 && d5 <= d6) return dot3(cp, cp);                         // vertex c
    const double vc = d1 * d4 - d3 * d2, vb = d5 * d2 - d1 * d6, va = d3 * d6 - d5 * d4;
    double v, w;                                                            // the closest point is q = (a + ab v) + ac w
    if (vc <= 0.0 && d1 >= 0.0 && d3 <= 0.0) {                              // edge ab
        const double den = d1 - d3;
        v = den > 0.0 ? d1 / den : 0.0;
        w = 0.0;
    } else if (vb <= 0.0 && d2 >= 0.0 && d6 <= 0.0) {                       // edge ac
        const double den = d2 - d6;
        v = 0.0;
        w = den > 0.0 ? d2 / den : 0.0;
    } else if (va <= 0.0 && d4 - d3 >= 0.0 && d5 - d6 >= 0.0) {             // edge bc
        const double den = (d4 - d3) + (d5 - d6);
        w = den > 0.0 ? (d4 - d3) / den : 0.0;
        v = 1.0 - w;
    } else {                                                                // face
        const double s = (va + vb) + vc;
        v = s > 0.0 ? vb / s : 0.0;
        w = s > 0.0 ? vc / s : 0.0;
    }
#pragma unroll
    for (int k = 0; k < 3; ++k) q[k] = p[k] - ((a[k] + ab[k] * v) + ac[k] * w);
    return dot3(q, q);
}

// pt_tri2 with the vector kept: r = the vector whose dot3 pt_tri2 returns (ap, bp, cp or q), chosen by the same seven cases in the
// same order with the same operations, so dot3(r, r) has pt_tri2's bits; the closest point of the triangle is p - r.  Returns the
// case, 1 .. 7 in the header's numbering (vertex a, b, c, edge ab, ac, bc, face).
__device__ __forceinline__ int pt_tri_vec(const double* p, const double* a, const double* b, const double* c, double* r) {
    double ab[3], ac[3], ap[3], bp[3], cp[3];
#pragma unroll
    for (int k = 0; k < 3; ++k) { ab[k] = b[k] - a[k]; ac[k] = c[k] - a[k]; ap[k] = p[k] - a[k]; bp[k] = p[k] - b[k]; cp[k] = p[k] - c[k]; }
    const double d1 = dot3(ab, ap), d2 = dot3(ac, ap), d3 = dot3(ab, bp), d4 = dot3(ac, bp), d5 = dot3(ab, cp), d6 = dot3(ac, cp);
    if (d1 <= 0.0 && d2 <= 0.0) { r[0] = ap[0]; r[1] = ap[1]; r[2] = ap[2]; return 1; }
    if (d3 >= 0.0 && d4 <= d3) { r[0] = bp[0]; r[1] = bp[1]; r[2] = bp[2]; return 2; }
    if (d6 >= 0.0 && d5 <= d6) { r[0] = cp[0]; r[1] = cp[1]; r[2] = cp[2]; return 3; }
    const double vc = d1 * d4 - d3 * d2, vb = d5 * d2 - d1 * d6, va = d3 * d6 - d5 * d4;
    double v, w;
    int which;
    if (vc <= 0.0 && d1 >= 0.0 && d3 <= 0.0) {
        const double den = d1 - d3;
        v = den > 0.0 ? d1 / den : 0.0;
        w = 0.0;
        which = 4;
    } else if (vb <= 0.0 && d2 >= 0.0 && d6 <= 0.0) {
        const double den = d2 - d6;
        v = 0.0;
        w = den > 0.0 ? d2 / den : 0.0;
        which = 5;
    } else if (va <= 0.0 && d4 - d3 >= 0.0 && d5 - d6 >= 0.0) {
        const double den = (d4 - d3) + (d5 - d6);
        w = den > 0.0 ? (d4 - d3) / den : 0.0;
        v = 1.0 - w;
        which = 6;
    } else {
        const double s = (va + vb) + vc;
        v = s > 0.0 ? vb / s : 0.0;
        w = s > 0.0 ? vc / s : 0.0;
        which = 7;
    }
#pragma unroll
    for (int k = 0; k < 3; ++k) r[k] = p[k] - ((a[k] + ab[k] * v) + ac[k] * w);
    return which;
}

}  // namespace creg
