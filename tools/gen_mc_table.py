#!/usr/bin/env python3
"""Generate autourdf_amd/csrc/mc_table.h: the marching-cubes triangle table of the link mesher (DESIGN N4).

    python tools/gen_mc_table.py            # rewrite the header
    python tools/gen_mc_table.py --check    # exit 1 if the committed header differs

Conventions (shared with mesh.hip and tests/_link_mesh_ref.py):
  corner c of a cell sits at offset (dx, dy, dz) = (c & 1, (c >> 1) & 1, (c >> 2) & 1); bit c of the case mask is its occupancy;
  edge e runs along axis a = e >> 2 from the corner whose offset is 0 on a and (j & 1, j >> 1), j = e & 3, on the two other axes
  taken in increasing order; its vertex is the edge midpoint.

Recipe.  On each of the six faces, seen from outside, a directed segment joins the midpoints of two active edges (edges whose
ends differ) so that the occupied corner it separates lies on its right.  A face with two active edges gets one segment; a face
with four (occupied corners on a diagonal) gets two, each cutting off one occupied corner -- the choice depends on the face's
own four corners only, so the two cells sharing a face draw the same segments.  The segments of a case close into loops (they
are the oriented boundary of the occupied part of the cube's surface); each loop is rotated to start at its lowest edge id and
fan-triangulated from there, loops in order of that id.  With "occupied on the right, seen from outside" a loop runs
clockwise around the occupied region, so the fan's normals point from occupied to empty and the enclosed signed volume is
positive (tests/test_link_mesh_cpu.py); the opposite direction gives the same surface turned inside out.
"""
import os
import sys

AXES_OTHER = ((1, 2), (0, 2), (0, 1))


def corner_offset(c):
    return (c & 1, (c >> 1) & 1, (c >> 2) & 1)


def corner_id(o):
    return o[0] | (o[1] << 1) | (o[2] << 2)


def edge_corners(e):
    """(corner at the low end, corner at the high end) of edge e."""
    a, j = e >> 2, e & 3
    b, c = AXES_OTHER[a]
    o = [0, 0, 0]
    o[b], o[c] = j & 1, j >> 1
    lo = corner_id(o)
    o[a] = 1
    return lo, corner_id(o)


EDGE_OF = {frozenset(edge_corners(e)): e for e in range(12)}


def faces():
    """The six faces as four corner ids each, counter-clockwise seen from outside."""
    out = []
    for a in range(3):
        b, c = AXES_OTHER[a]
        for side in (0, 1):
            # (e_b, e_c, e_a) is right-handed for a = 0, 2 and left-handed for a = 1; the outward normal is +e_a on side 1
            ccw = [(0, 0), (1, 0), (1, 1), (0, 1)]
            right_handed = a != 1
            if right_handed != (side == 1):
                ccw = ccw[::-1]
            quad = []
            for u, v in ccw:
                o = [0, 0, 0]
                o[a], o[b], o[c] = side, u, v
                quad.append(corner_id(o))
            out.append(tuple(quad))
    return out


FACES = faces()


def face_segments(quad, occ):
    """Directed segments (edge id -> edge id) a face carries, from the occupancy of its four corners in ccw order."""
    segs = []
    act = [occ[i] != occ[(i + 1) % 4] for i in range(4)]          # act[i]: the edge from quad[i] to quad[i + 1]
    eid = [EDGE_OF[frozenset((quad[i], quad[(i + 1) % 4]))] for i in range(4)]
    n = sum(act)
    if n == 0:
        return segs
    if n == 4:                                                     # cut off every occupied corner on its own
        for i in range(4):
            if occ[i]:
                segs.append((eid[(i - 1) % 4], eid[i]))           # from the edge before corner i to the edge after: i on the right
        return segs
    # n == 2: the occupied corners are one ccw run quad[s..t]; the segment goes from the edge before the run's first corner
    # to the edge after its last, which keeps the run on the right
    s = next(i for i in range(4) if occ[i] and not occ[(i - 1) % 4])
    t = next(i for i in range(4) if occ[i] and not occ[(i + 1) % 4])
    segs.append((eid[(s - 1) % 4], eid[t]))
    return segs


def case_segments(mask):
    """[(face index, from edge, to edge)] of one case."""
    out = []
    for f, quad in enumerate(FACES):
        occ = [(mask >> c) & 1 for c in quad]
        out += [(f, p, q) for p, q in face_segments(quad, occ)]
    return out


def case_triangles(mask):
    nxt = {}
    for _, p, q in case_segments(mask):
        assert p not in nxt, (mask, p)
        nxt[p] = q
    loops, seen = [], set()
    for start in sorted(nxt):
        if start in seen:
            continue
        loop, e = [], start
        while e not in seen:
            seen.add(e)
            loop.append(e)
            e = nxt[e]
        assert e == start, (mask, loop)
        loops.append(loop)                                         # starts at its lowest edge id: `start` ascends
    tris = []
    for loop in loops:
        for i in range(1, len(loop) - 1):
            tris.append((loop[0], loop[i], loop[i + 1]))
    return tris


def build_table():
    """256 lists of (e0, e1, e2) edge-id triangles."""
    return [case_triangles(m) for m in range(256)]


def render():
    table = build_table()
    total, most = sum(len(t) for t in table), max(len(t) for t in table)
    lines = ["// mc_table.h -- GENERATED by tools/gen_mc_table.py; do not edit.  Marching-cubes cases of the link mesher:",
             "// corner c at offset (c & 1, (c >> 1) & 1, (c >> 2) & 1); edge e along axis e >> 2 from the corner at",
             "// (j & 1, j >> 1), j = e & 3, on the two other axes in increasing order.  Row m: up to MC_MAX_TRI triangles",
             "// as edge ids, 0xff-padded; byte 15 is the triangle count.  %d triangles over the 256 cases, at most %d."
             % (total, most),
             "// A device translation unit defines MC_TABLE_QUAL (static __device__ const) before including this file.",
             "#pragma once", "#include <cstdint>", "", "#ifndef MC_TABLE_QUAL", "#define MC_TABLE_QUAL static const", "#endif",
             "#define MC_MAX_TRI %d" % most, "", "MC_TABLE_QUAL uint8_t MC_TABLE[256][16] = {"]
    for m, tris in enumerate(table):
        flat = [e for t in tris for e in t]
        row = flat + [255] * (15 - len(flat)) + [len(tris)]
        lines.append("    {" + ", ".join("%3d" % v for v in row) + "},  // %3d" % m)
    lines += ["};", ""]
    return "\n".join(lines)


HEADER = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "autourdf_amd", "csrc", "mc_table.h")

if __name__ == "__main__":
    text = render()
    if "--check" in sys.argv:
        sys.exit(0 if open(HEADER).read() == text else 1)
    with open(HEADER, "w") as f:
        f.write(text)
    print("wrote", HEADER)
