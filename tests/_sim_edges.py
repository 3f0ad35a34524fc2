"""Edge families for csrc/sample.hip (`k_sample_mesh`, `k_raster_depth`, `k_visible`) and csrc/fps.hip (`k_fps`), with references
that do NOT restate the kernels (test infrastructure, no test functions).

References
  exact_raster      rational arithmetic (fractions.Fraction) from the posed float64 triangles: exact projection, coverage at pixel
                    centres by exact barycentrics (inside = all three >= 0), exact perspective-correct depth, exact minimum.  Per
                    pixel it also gives the DECISION MARGIN (smallest |barycentric| over the facets whose pixel box holds the pixel)
                    and the relative distance of every covering depth from near and far.  It states the kernel's two documented
                    conventions: a facet with a vertex nearer than `near` is not drawn (no clipping), zero screen area is not drawn.
  plane_depth       the analytic depth of the plane z = 0 along the ray of a pixel centre, rational (checks exact_raster itself)
  exact_visible     the same projection for points: inclusive near / far, floor of the exact pixel coordinates, the image bounds,
                    d <= fl(zb + eps) against a given buffer (the threshold is the rounded sum the kernel documents), any camera
  exact_sample      bisect.bisect_right on the exact product u0 * cum_area[-1]; the point in rationals from fl(sqrt(u1))
  plain_fps         a numpy loop with argmax (first maximum); on integer lattices every squared distance is exact, so any correct
                    implementation agrees bit for bit whatever its operation order

`restated_*` is a small float64 restatement of the kernels written for this file (it shares nothing with oracle/sim_data.py); with
`variant=None` it equals the oracle bit for bit, and every name in VARIANTS is one plausible way of being subtly wrong.  The
comparisons the GPU test makes (`check_raster`, `check_visible`, `check_sample`, `check_fps`) live here so that
tests/test_sim_edges_cpu.py can show that each wrong variant is rejected by them -- which stands in for mutating the kernel.

A pixel is DECIDED when its margin is >= MARGIN = 1e-9 and every covering depth is >= 1e-9 (relative) from near and far: screen
coordinates carry a few ulp x W of rounding (1e-14 at W <= 32), a facet is at least 1e-3 pixel high, so a barycentric is wrong by
1e-11 at most.  On decided pixels drawn / empty must agree exactly; undecided pixels are at most CAP of a case's pixels (none in
the plane and launch families).  The shared_edge family is the exception, on purpose: see EVERY_PIXEL.  MEASURED_DEV records, per family, the restatement's largest relative deviation from the exact
depth / point as measured by tests/test_sim_edges_cpu.py; the GPU bound is max(4 x that, 2^-50) -- the 4 absorbs another libm's
tan / sqrt on the GPU host -- and never anything measured from the kernel.
"""
import bisect
import functools
import math
from fractions import Fraction as Fr
from types import SimpleNamespace as NS

import numpy as np

MARGIN = 1e-9
CAP = 0.005
BOUND_FLOOR = 2.0 ** -50
HALF = Fr(1, 2)

VARIANTS = ("near_strict", "vis_trunc", "zb_strict", "bisect_left", "no_link_clamp", "bary_rot", "fps_last_tie", "near_per_pixel",
            "contracted")

# every kernel decision the families are built to reach (tests/test_sim_edges_cpu.py asserts the union over the cases is this)
DECISIONS = ("near_drop", "far_drop", "clamp_left", "clamp_right", "clamp_top", "clamp_bottom", "off_left", "off_right", "off_top",
             "off_bottom", "cast_overflow", "zero_area", "link_clamp_lo", "link_clamp_hi",
             "vis_at_near", "vis_below_near", "vis_at_far", "vis_beyond_far", "vis_behind", "vis_px_0", "vis_px_W", "vis_py_0",
             "vis_py_H", "vis_px_neg_frac", "vis_py_neg_frac", "vis_occluded", "vis_zb_edge", "vis_zb_edge_ulp", "vis_later_camera",
             "vis_no_camera", "sample_boundary", "sample_zero_run", "sample_u0_one", "sample_rounding", "sample_link_clamp_lo",
             "sample_link_clamp_hi", "fps_tie_slot", "fps_tie_lane", "fps_tie_wave", "fps_tie_crossed")

# ---------------------------------------------------------------------------------------------------------------------------
# Largest relative deviation of the RESTATEMENT from the exact reference per family, rounded up to two digits, as measured by
# tests/test_sim_edges_cpu.py::test_measured_deviation_per_family (which fails when a figure is exceeded).  Raster families:
# |depth - exact| / exact over decided drawn pixels.  Sampler families: max |point - exact| / max(|exact point|, |translation|,
# |local point|) in the infinity norm.
#   family            measured     GPU bound = max(4 x measured, 2^-50 = 8.9e-16)
MEASURED_DEV = {
    "plane":          6.4e-16,   # 2.56e-15
    "plane_links":    6.4e-16,   # 2.56e-15
    "near":           4.5e-16,   # 1.80e-15
    "far":            5.1e-16,   # 2.04e-15
    "border":         6.3e-16,   # 2.52e-15
    "huge":           3.7e-16,   # 1.48e-15
    "tiny_image":     4.5e-16,   # 1.80e-15
    "degenerate":     7.4e-13,   # 2.96e-12
    "launch":         4.5e-16,   # 1.80e-15
    "link_clamp":     3.0e-16,   # 1.20e-15
    "stack":          2.6e-16,   # 1.04e-15
    "shared_edge":    1.3e-15,   # 5.20e-15
    "table":          1.2e-15,   # 4.80e-15
    "zero_run":       2.5e-16,   # 1.00e-15
    "u0_one":         1.0e-16,   # 8.88e-16
    "rounding":       1.3e-15,   # 5.20e-15
    "corner":         0.0,       # 8.88e-16
    "pose":           3.7e-16,   # 1.48e-15
    "sample_links":   3.6e-16,   # 1.44e-15
    "sample_launch":  6.0e-16,   # 2.40e-15
}
# families that may have no undecided pixel at all
NO_UNDECIDED = ("plane", "plane_links", "launch")
# the one family made of undecided pixels ON PURPOSE: every pixel centre lies, to within rounding, on the edge two facets share.
# Exact arithmetic draws such a pixel (inside is >= 0 on both sides); the kernel draws it only because the edge function of a
# shared edge is an exact negation in the two facets, which holds without contraction of a * b - c * d into an fma and is what
# -ffp-contract=off is there for.  The decided-pixel rule and its cap do not apply to it: EVERY pixel must be drawn.
EVERY_PIXEL = ("shared_edge",)


def family_of(label):
    return label.split("/")[0]


def gpu_bound(family):
    return max(4.0 * MEASURED_DEV[family], BOUND_FLOOR)


# ------------------------------------------------------------------------------------------ cameras
AXIS_CAM = np.array([0, 0, 0, 1, 0, 0, 0, 1, 0, 0, 0, 1], np.float64)              # d = x, xc = y, yc = z: depths are coordinates
CONFIGS = ((23, 17, 1.0, 60.0), (32, 24, 32 / 24, 35.0), (16, 12, 0.5, 120.0), (17, 23, 17 / 23, 60.0))  # W, H, aspect, fov
NEAR, FAR = 0.125, 4.0


def tan_half(fov):
    return float(np.tan(fov * 3.14159265358979323846 / 360.0))


def look_at(eye, target, up=(0.0, 0.0, 1.0)):
    e = np.asarray(eye, np.float64)
    f = np.asarray(target, np.float64) - e
    f /= np.linalg.norm(f)
    s = np.cross(f, up)
    s /= np.linalg.norm(s)
    return np.concatenate([e, f, s, np.cross(s, f)])


def at_pixels(cfg, d, pix, cam=AXIS_CAM):
    """World points that an axis-permuting camera (unit axes, any eye) projects to the pixel coordinates `pix` (k,2) at depth d."""
    W, H, asp, fov = cfg
    th = tan_half(fov)
    pix = np.asarray(pix, np.float64).reshape(-1, 2)
    d = np.broadcast_to(np.asarray(d, np.float64), (len(pix),))
    xc = (2.0 * pix[:, 0] / W - 1.0) * ((d * th) * asp)
    yc = (1.0 - 2.0 * pix[:, 1] / H) * (d * th)
    return cam[0:3] + d[:, None] * cam[3:6] + xc[:, None] * cam[6:9] + yc[:, None] * cam[9:12]


def raster_case(label, tri, cfg, cams=AXIS_CAM, near=NEAR, far=FAR, tri_link=None, link_T=None):
    tri = np.ascontiguousarray(np.asarray(tri, np.float64).reshape(-1, 3, 3))
    W, H, asp, fov = cfg
    return NS(label=label, tri=tri, cams=np.ascontiguousarray(np.asarray(cams, np.float64).reshape(-1, 12)), W=int(W), H=int(H),
              aspect=float(asp), fov=float(fov), near=float(near), far=float(far),
              tri_link=np.zeros(len(tri), np.int32) if tri_link is None else np.asarray(tri_link, np.int32),
              link_T=np.eye(4)[None].copy() if link_T is None else np.ascontiguousarray(link_T, np.float64))


def posed(tri, tri_link, link_T, clamp=True):
    """The posed triangles as the kernels compute them ((T0 q0 + T1 q1) + T2 q2) + T3, link index clamped into [0, L)."""
    L = len(link_T)
    l = np.clip(tri_link, 0, L - 1) if clamp else np.asarray(tri_link) % L
    T = link_T[l]
    out = np.empty_like(tri)
    for a in range(3):
        out[:, :, a] = ((T[:, None, a, 0] * tri[:, :, 0] + T[:, None, a, 1] * tri[:, :, 1]) + T[:, None, a, 2] * tri[:, :, 2]) \
            + T[:, None, a, 3]
    return out


# ------------------------------------------------------------------------------------------ exact references
def _fr(v):
    return [Fr(float(x)) for x in v]


def _exact_project(cam, p, th, asp, W, H):
    """cam, p, th, asp: Fractions.  -> (px, py, d); px, py None when d == 0."""
    r = [p[a] - cam[a] for a in range(3)]
    d = r[0] * cam[3] + r[1] * cam[4] + r[2] * cam[5]
    if d == 0:
        return None, None, d
    xc = r[0] * cam[6] + r[1] * cam[7] + r[2] * cam[8]
    yc = r[0] * cam[9] + r[1] * cam[10] + r[2] * cam[11]
    nx, ny = xc / (d * th * asp), yc / (d * th)
    return (nx / 2 + HALF) * W, (1 - (ny / 2 + HALF)) * H, d


def exact_raster(world, cam, th, aspect, W, H, near, far):
    """One camera.  world (F,3,3) float64 posed triangles; everything else floats taken as the exact rationals they are.
    -> NS(depth: H x W list of Fraction or None, margin (H,W), rng (H,W), taken: set of DECISIONS)."""
    camF, thF, aspF, nearF, farF = _fr(cam), Fr(float(th)), Fr(float(aspect)), Fr(float(near)), Fr(float(far))
    depth = [[None] * W for _ in range(H)]
    margin, rng, taken = np.full((H, W), np.inf), np.full((H, W), np.inf), set()
    for f in range(len(world)):
        P = []
        for v in range(3):
            px, py, d = _exact_project(camF, _fr(world[f, v]), thF, aspF, W, H)
            if d < nearF:
                P = None
                break
            P.append((px, py, d))
        if P is None:
            taken.add("near_drop")
            continue
        (x0, y0, d0), (x1, y1, d1), (x2, y2, d2) = P
        area = (x1 - x0) * (y2 - y0) - (x2 - x0) * (y1 - y0)
        if area == 0:
            taken.add("zero_area")
            continue
        xs, ys = (x0, x1, x2), (y0, y1, y2)
        if max(abs(c) for c in xs + ys) >= 2 ** 31:
            taken.add("cast_overflow")
        bx0, bx1 = math.floor(min(xs) - HALF), math.ceil(max(xs) - HALF)
        by0, by1 = math.floor(min(ys) - HALF), math.ceil(max(ys) - HALF)
        off = [n for n, c in (("off_right", bx0 > W - 1), ("off_left", bx1 < 0), ("off_bottom", by0 > H - 1), ("off_top", by1 < 0)) if c]
        if off:
            taken.update(off)
            continue
        taken.update(n for n, c in (("clamp_left", bx0 < 0), ("clamp_right", bx1 > W - 1), ("clamp_top", by0 < 0),
                                    ("clamp_bottom", by1 > H - 1)) if c)
        # barycentrics and 1 / depth are affine in the pixel centre: b_i = A_i + B_i cx + C_i cy
        V = ((x1, y1, x2, y2), (x2, y2, x0, y0), (x0, y0, x1, y1))
        co = [((xa * yb - xb * ya) / area, (ya - yb) / area, (xb - xa) / area) for xa, ya, xb, yb in V]
        iv = [1 / d0, 1 / d1, 1 / d2]
        ico = [sum(co[i][k] * iv[i] for i in range(3)) for k in range(3)]
        for y in range(max(by0, 0), min(by1, H - 1) + 1):
            cy = Fr(2 * y + 1, 2)
            for x in range(max(bx0, 0), min(bx1, W - 1) + 1):
                cx = Fr(2 * x + 1, 2)
                b = [c[0] + c[1] * cx + c[2] * cy for c in co]
                m = float(min(abs(t) for t in b))
                if m < margin[y, x]:
                    margin[y, x] = m
                if b[0] < 0 or b[1] < 0 or b[2] < 0:
                    continue
                d = 1 / (ico[0] + ico[1] * cx + ico[2] * cy)
                rng[y, x] = min(rng[y, x], float(abs(d - nearF) / nearF), float(abs(d - farF) / farF))
                if d > farF:
                    taken.add("far_drop")
                elif d >= nearF and (depth[y][x] is None or d < depth[y][x]):
                    depth[y][x] = d
    return NS(depth=depth, margin=margin, rng=rng, taken=taken,
              drawn=np.array([[c is not None for c in row] for row in depth], bool).reshape(H, W))


def plane_depth(cam, th, aspect, W, H, x, y):
    """Exact depth of the plane z = 0 along the ray through the centre of pixel (x, y): the point q + eye of the plane with
    xc = a d and yc = b d, from the 2 x 2 linear system in its two free coordinates."""
    c, thF, aspF = _fr(cam), Fr(float(th)), Fr(float(aspect))
    a = (Fr(2 * x + 1, W) - 1) * thF * aspF
    b = (1 - Fr(2 * y + 1, H)) * thF
    f, r, u = c[3:6], c[6:9], c[9:12]
    g1, g2 = [r[k] - a * f[k] for k in range(3)], [u[k] - b * f[k] for k in range(3)]
    qz = -c[2]
    det = g1[0] * g2[1] - g1[1] * g2[0]
    r1, r2 = -g1[2] * qz, -g2[2] * qz
    qx, qy = (r1 * g2[1] - g1[1] * r2) / det, (g1[0] * r2 - r1 * g2[0]) / det
    return qx * f[0] + qy * f[1] + qz * f[2]


@functools.lru_cache(maxsize=None)
def _exact_of(label):
    case = RASTER_CASES[label]
    world = posed(case.tri, case.tri_link, case.link_T)
    th = tan_half(case.fov)
    ex = [exact_raster(world, cam, th, case.aspect, case.W, case.H, case.near, case.far) for cam in case.cams]
    taken = set().union(*[e.taken for e in ex])
    if (case.tri_link < 0).any():
        taken.add("link_clamp_lo")
    if (case.tri_link >= len(case.link_T)).any():
        taken.add("link_clamp_hi")
    return ex, taken


def exact_of(case):
    return _exact_of(case.label)


def exact_visible(cams, pts, th, aspect, W, H, near, far, depth, eps):
    """-> (visible (n) bool, tags: list of sets).  depth (C,H,W) float64 is GIVEN (the buffer the points are tested against)."""
    thF, aspF, nearF, farF = Fr(float(th)), Fr(float(aspect)), Fr(float(near)), Fr(float(far))
    camsF = [_fr(c) for c in cams]
    vis, tags = np.zeros(len(pts), bool), []
    for i, p in enumerate(pts):
        pF, t = _fr(p), set()
        for k, cam in enumerate(camsF):
            px, py, d = _exact_project(cam, pF, thF, aspF, W, H)
            if d <= 0:
                t.add("vis_behind")
                continue
            t.update(n for n, c in (("vis_at_near", d == nearF), ("vis_at_far", d == farF),
                                    ("vis_below_near", nearF * (1 - Fr(1, 2 ** 50)) < d < nearF),
                                    ("vis_beyond_far", farF < d < farF * (1 + Fr(1, 2 ** 50)))) if c)
            if d < nearF or d > farF:
                continue
            t.update(n for n, c in (("vis_px_0", px == 0), ("vis_px_W", px == W), ("vis_py_0", py == 0), ("vis_py_H", py == H),
                                    ("vis_px_neg_frac", -1 < px < 0), ("vis_py_neg_frac", -1 < py < 0)) if c)
            x, y = math.floor(px), math.floor(py)
            if x < 0 or x >= W or y < 0 or y >= H:
                continue
            zb = float(depth[k, y, x])
            thr = zb + float(eps)                                              # fl(zb + eps): the documented threshold
            if np.isfinite(thr):
                t.update(n for n, c in (("vis_zb_edge", d == Fr(thr)), ("vis_zb_edge_ulp", d == Fr(float(np.nextafter(thr, np.inf))))) if c)
            if np.isinf(thr) or d <= Fr(thr):
                vis[i] = True
                if k > 0:
                    t.add("vis_later_camera")
                break
            t.add("vis_occluded")
        if not vis[i] and len(cams) > 1:
            t.add("vis_no_camera")
        tags.append(t)
    return vis, tags


def exact_sample(tri, cum_area, tri_link, link_T, u):
    """-> (points: list of 3 Fractions per sample, pick (n) int, link (n) int, rounded_pick (n) int, taken set).  The pick is
    bisect_right on the exact product; rounded_pick uses the kernel's rounded product fl(u0 * cum_area[-1])."""
    table = [Fr(float(c)) for c in cum_area]
    ftable = [float(c) for c in cum_area]
    F, L = len(table), len(link_T)
    pts, pick, link, rpick, taken = [], [], [], [], set()
    for u0, u1, u2 in np.asarray(u, np.float64):
        target = Fr(float(u0)) * table[-1]
        f = min(bisect.bisect_right(table, target), F - 1)
        rf = min(bisect.bisect_right(ftable, float(u0) * ftable[-1]), F - 1)
        lo = bisect.bisect_left(table, target)
        if lo < F and table[lo] == target:
            taken.add("sample_boundary")
            if f - lo > 1:
                taken.add("sample_zero_run")
        if target >= table[-1]:
            taken.add("sample_u0_one")
        if rf != f:
            taken.add("sample_rounding")
        f_used = rf                                                            # the geometry follows the documented (rounded) pick
        s = Fr(math.sqrt(float(u1)))
        b0, b1, b2 = 1 - s, s * (1 - Fr(float(u2))), s * Fr(float(u2))
        A, B, C = (_fr(tri[f_used, v]) for v in range(3))
        p = [b0 * A[a] + b1 * B[a] + b2 * C[a] for a in range(3)]
        tl = int(tri_link[f_used])
        if tl < 0:
            taken.add("sample_link_clamp_lo")
        if tl >= L:
            taken.add("sample_link_clamp_hi")
        l = min(max(tl, 0), L - 1)
        T = [_fr(row) for row in link_T[l]]
        pts.append(([T[a][0] * p[0] + T[a][1] * p[1] + T[a][2] * p[2] + T[a][3] for a in range(3)], p, [T[a][3] for a in range(3)]))
        pick.append(f)
        rpick.append(rf)
        link.append(l)
    return pts, np.array(pick), np.array(link), np.array(rpick), taken


FPS_NT = 1024


def plain_fps(X, m, last_tie=False, want_ties=False):
    """Start at 0, then the point with the largest squared distance to the selected set, FIRST maximum.  With want_ties also the
    set of tie stages met: the relation between the winner and every other index at the maximum (same thread and another register
    slot, same wave and another lane, another wave; `crossed` when the loser sits in a lower thread than the winner)."""
    X = np.asarray(X, np.float64)
    n = len(X)
    dmin = np.full(n, np.inf)
    sel, cur, ties = np.empty(m, np.int64), 0, set()
    for s in range(m):
        sel[s] = cur
        a, b, c = X[:, 0] - X[cur, 0], X[:, 1] - X[cur, 1], X[:, 2] - X[cur, 2]
        dmin = np.minimum(dmin, (a * a + b * b) + c * c)
        cur = int(n - 1 - np.argmax(dmin[::-1])) if last_tie else int(np.argmax(dmin))
        if want_ties and s + 1 < m:
            win = int(np.argmax(dmin))
            for j in np.nonzero(dmin == dmin[win])[0][1:65]:
                tw, tj = win % FPS_NT, int(j) % FPS_NT
                ties.add("fps_tie_slot" if tw == tj else "fps_tie_lane" if tw // 64 == tj // 64 else "fps_tie_wave")
                if tj < tw:
                    ties.add("fps_tie_crossed")
    return (sel, ties) if want_ties else sel


# ------------------------------------------------------------------------------------------ the restatement and its wrong variants
def _fms(a, b, c, d):
    """fl(a * b - fl(c * d)) element by element: what a compiler that contracts a * b - c * d makes of it (fma(a, b, -(c * d)))."""
    a, b, c, d = np.broadcast_arrays(a, b, c, d)
    cd = c * d
    return np.array([float(Fr(float(p)) * Fr(float(q)) - Fr(float(r))) for p, q, r in zip(a.ravel(), b.ravel(), cd.ravel())]).reshape(a.shape)


def restated_raster(case, variant=None):
    """(C,H,W) float64 depth buffers in the kernel's operation order, +inf where nothing is drawn."""
    W, H = case.W, case.H
    th, asp, near, far = np.float64(tan_half(case.fov)), np.float64(case.aspect), np.float64(case.near), np.float64(case.far)
    world = posed(case.tri, case.tri_link, case.link_T, clamp=variant != "no_link_clamp")
    out = np.full((len(case.cams), H, W), np.inf)
    with np.errstate(all="ignore"):
        for ci, cam in enumerate(case.cams):
            r = world - cam[0:3]
            D = (r[..., 0] * cam[3] + r[..., 1] * cam[4]) + r[..., 2] * cam[5]
            xc = (r[..., 0] * cam[6] + r[..., 1] * cam[7]) + r[..., 2] * cam[8]
            yc = (r[..., 0] * cam[9] + r[..., 1] * cam[10]) + r[..., 2] * cam[11]
            X = ((xc / ((D * th) * asp)) * 0.5 + 0.5) * np.float64(W)
            Y = (1.0 - ((yc / (D * th)) * 0.5 + 0.5)) * np.float64(H)
            for f in range(len(world)):
                x, y, d = X[f], Y[f], D[f]
                if variant == "near_strict":
                    if not (d > near).all():
                        continue
                elif variant != "near_per_pixel" and not (d >= near).all():
                    continue
                area = (x[1] - x[0]) * (y[2] - y[0]) - (x[2] - x[0]) * (y[1] - y[0])
                if area == 0.0:
                    continue
                xmin, xmax, ymin, ymax = x.min(), x.max(), y.min(), y.max()
                if not (xmin - 0.5 <= W) or not (ymin - 0.5 <= H) or not (xmax >= -1.0) or not (ymax >= -1.0):
                    continue                                                    # off screen / NaN, before any integer conversion
                x0, x1 = int(max(0.0, math.floor(xmin - 0.5))), int(min(float(W - 1), math.ceil(xmax - 0.5)))
                y0, y1 = int(max(0.0, math.floor(ymin - 0.5))), int(min(float(H - 1), math.ceil(ymax - 0.5)))
                if x1 < x0 or y1 < y0:
                    continue
                cx, cy = np.arange(x0, x1 + 1)[None, :] + 0.5, np.arange(y0, y1 + 1)[:, None] + 0.5
                ia = 1.0 / area
                if variant == "contracted":
                    b0, b1, b2 = (_fms(x[i] - cx, y[j] - cy, x[j] - cx, y[i] - cy) * ia for i, j in ((1, 2), (2, 0), (0, 1)))
                else:
                    b0 = ((x[1] - cx) * (y[2] - cy) - (x[2] - cx) * (y[1] - cy)) * ia
                    b1 = ((x[2] - cx) * (y[0] - cy) - (x[0] - cx) * (y[2] - cy)) * ia
                    b2 = ((x[0] - cx) * (y[1] - cy) - (x[1] - cx) * (y[0] - cy)) * ia
                i0, i1, i2 = 1.0 / d[0], 1.0 / d[1], 1.0 / d[2]
                if variant == "bary_rot":
                    i0, i1, i2 = i1, i2, i0
                z = 1.0 / ((b0 * i0 + b1 * i1) + b2 * i2)
                ok = ~((b0 < 0.0) | (b1 < 0.0) | (b2 < 0.0)) & (z >= near) & (z <= far)
                sub = out[ci, y0:y1 + 1, x0:x1 + 1]
                sub[ok] = np.minimum(sub[ok], z[ok])
    return out


def restated_visible(case, pts, depth, eps, variant=None):
    W, H = case.W, case.H
    th, asp, near, far = np.float64(tan_half(case.fov)), np.float64(case.aspect), np.float64(case.near), np.float64(case.far)
    vis = np.zeros(len(pts), bool)
    with np.errstate(all="ignore"):
        for i, p in enumerate(np.asarray(pts, np.float64)):
            for k, cam in enumerate(case.cams):
                r0, r1, r2 = p[0] - cam[0], p[1] - cam[1], p[2] - cam[2]
                d = (r0 * cam[3] + r1 * cam[4]) + r2 * cam[5]
                if not ((d > near if variant == "near_strict" else d >= near) and d <= far):
                    continue
                xc = (r0 * cam[6] + r1 * cam[7]) + r2 * cam[8]
                yc = (r0 * cam[9] + r1 * cam[10]) + r2 * cam[11]
                px = ((xc / ((d * th) * asp)) * 0.5 + 0.5) * np.float64(W)
                py = (1.0 - ((yc / (d * th)) * 0.5 + 0.5)) * np.float64(H)
                rnd = math.trunc if variant == "vis_trunc" else math.floor
                x, y = rnd(px), rnd(py)
                if x < 0 or x >= W or y < 0 or y >= H:
                    continue
                zb = depth[k, y, x]
                if (d < zb + eps) if variant == "zb_strict" else (d <= zb + eps):
                    vis[i] = True
                    break
    return vis


def restated_sample(tri, cum_area, tri_link, link_T, u, variant=None):
    tri, cum_area, link_T, u = (np.asarray(a, np.float64) for a in (tri, cum_area, link_T, u))
    table, F, L = [float(c) for c in cum_area], len(cum_area), len(link_T)
    side = bisect.bisect_left if variant == "bisect_left" else bisect.bisect_right
    f = np.array([min(side(table, float(u0 * cum_area[-1])), F - 1) for u0 in u[:, 0]])
    s = np.sqrt(u[:, 1])
    b0, b1, b2 = 1.0 - s, s * (1.0 - u[:, 2]), s * u[:, 2]
    if variant == "bary_rot":
        b0, b1, b2 = b2, b0, b1
    t = tri[f]
    p = (b0[:, None] * t[:, 0] + b1[:, None] * t[:, 1]) + b2[:, None] * t[:, 2]
    l = np.asarray(tri_link)[f] % L if variant == "no_link_clamp" else np.clip(np.asarray(tri_link)[f], 0, L - 1)
    T = link_T[l]
    out = np.stack([((T[:, a, 0] * p[:, 0] + T[:, a, 1] * p[:, 1]) + T[:, a, 2] * p[:, 2]) + T[:, a, 3] for a in range(3)], 1)
    return out, l.astype(np.int32)


# ------------------------------------------------------------------------------------------ the comparisons (GPU test and teeth)
def check_raster(case, depth):
    """depth (C,H,W) float64 from the kernel (or a restatement) against the exact reference: drawn / empty equal on every decided
    pixel, relative depth deviation within the family's bound there, the family's own expectations.  -> (largest deviation,
    undecided share)."""
    fam = family_of(case.label)
    ex, _ = exact_of(case)
    assert depth.shape == (len(case.cams), case.H, case.W), case.label
    worst, undecided = 0.0, 0
    for c, e in enumerate(ex):
        got = np.isfinite(depth[c])
        assert (np.isposinf(depth[c]) | got).all(), (case.label, "a pixel is neither a depth nor +inf")
        decided = (e.margin >= MARGIN) & (e.rng >= MARGIN)
        undecided += int((~decided).sum())
        if fam in EVERY_PIXEL:
            assert e.drawn.all() and got.all(), (case.label, c, "a pixel on a shared edge fell through", np.argwhere(~got)[:4].tolist())
            decided = np.ones_like(decided)
        bad = decided & (got != e.drawn)
        assert not bad.any(), (case.label, c, "drawn / empty differs on decided pixels", np.argwhere(bad)[:4].tolist())
        for y, x in np.argwhere(decided & got & e.drawn):
            dev = float(abs(Fr(float(depth[c, y, x])) - e.depth[y][x]) / e.depth[y][x])
            worst = max(worst, dev)
        if fam in ("plane", "plane_links"):
            assert got.all(), (case.label, c, "hole in a closed surface", np.argwhere(~got)[:4].tolist())
            th = tan_half(case.fov)
            for y in range(case.H):
                for x in range(case.W):
                    want = plane_depth(case.cams[c], th, case.aspect, case.W, case.H, x, y)
                    worst = max(worst, float(abs(Fr(float(depth[c, y, x])) - want) / want))
        if fam == "degenerate":
            assert not (got & ~e.drawn).any(), (case.label, c, "a degenerate facet wrote a pixel the exact reference leaves empty")
    assert worst <= gpu_bound(fam), (case.label, "depth deviation", worst, gpu_bound(fam))
    return worst, undecided / (len(ex) * case.H * case.W)


def check_visible(case, pts, expect, exact_ok, depth, eps, vis):
    """vis (n) bool against what the points were built to be, and against exact_visible on the points whose construction is
    exact in rationals too (exact_ok)."""
    vis = np.asarray(vis, bool)
    assert vis.shape == (len(pts),), case.label
    assert (vis == expect).all(), (case.label, "built expectation", np.nonzero(vis != expect)[0][:6].tolist())
    ev, _ = exact_visible(case.cams, pts, tan_half(case.fov), case.aspect, case.W, case.H, case.near, case.far, depth, eps)
    assert (vis == ev)[exact_ok].all(), (case.label, "exact visibility", np.nonzero((vis != ev) & exact_ok)[0][:6].tolist())


def sample_deviation(exact_pts, out):
    worst = 0.0
    for (want, p, t), got in zip(exact_pts, np.asarray(out, np.float64)):
        scale = max(max(abs(v) for v in want), max(abs(v) for v in p), max(abs(v) for v in t))
        err = max(abs(Fr(float(g)) - w) for g, w in zip(got, want))
        if err:
            worst = max(worst, float(err / scale))
    return worst


def check_sample(case, out, links):
    """out (n,3), links (n) against exact_sample: the link of every point exactly, the pick through the rounded product where the
    family is `rounding` and through the exact product everywhere else, the point within the family's bound; the exact vertex
    at the barycentric corners."""
    fam = family_of(case.label)
    pts, pick, link, rpick, _ = exact_sample(case.tri, case.cum_area, case.tri_link, case.link_T, case.u)
    if fam != "rounding":
        assert (pick == rpick).all(), (case.label, "the case's targets are not exact")
    assert (np.asarray(links) == link).all(), (case.label, "link of the picked facet")
    if case.expect_pick is not None:
        assert (rpick == case.expect_pick).all(), (case.label, "the helper's own expectation")
    worst = sample_deviation(pts, out)
    assert worst <= gpu_bound(fam), (case.label, "point deviation", worst, gpu_bound(fam))
    if case.expect_exact is not None:
        assert (np.asarray(out) == case.expect_exact).all(), (case.label, "corner vertices are returned exactly")
    return worst


def check_fps(X, m, sel):
    want = plain_fps(X, m)
    assert np.asarray(sel).shape == (m,) and (np.asarray(sel) == want).all(), ("fps", len(X), m, np.nonzero(np.asarray(sel) != want)[0][:4])


# ------------------------------------------------------------------------------------------ rasteriser families
def _quad(cfg, d, x0, y0, x1, y1, cam=AXIS_CAM):
    """Two facets filling the pixel rectangle [x0,x1] x [y0,y1] at depth d (a scalar, or one depth per corner)."""
    # (corners nudged off the rectangle so that no edge or diagonal runs through a row of pixel centres)
    P = at_pixels(cfg, d, [(x0 + 0.013, y0 + 0.007), (x1 - 0.011, y0 + 0.019), (x1 + 0.017, y1 - 0.005), (x0 - 0.003, y1 + 0.023)], cam)
    return [P[[0, 1, 2]], P[[0, 2, 3]]]


def _plane_cases():
    """A jittered grid of quads in the plane z = 0, split in two, facets and vertex order shuffled, overfilling every image."""
    setups = (("perp", 0, [np.array([0.1, -0.05, 1.5, 0, 0, -1, 1, 0, 0, 0, 1, 0], np.float64)]),
              ("tilted", 1, [look_at((0.9, -0.6, 1.1), (0.05, 0.02, 0.0))]),
              ("tilted_wide", 2, [look_at((0.12, -0.1, 0.8), (0.02, 0.01, 0.0), up=(0.0, 1.0, 0.0))]),
              ("three_cams", 3, [look_at((0.7, 0.4, 1.2), (0.0, 0.0, 0.0)), look_at((-0.5, 0.6, 0.9), (0.1, 0.0, 0.0)),
                                 np.array([-0.2, 0.1, 1.0, 0, 0, -1, 0, 1, 0, 1, 0, 0], np.float64)]))
    for name, ci, cams in setups:
        cfg = CONFIGS[ci]
        W, H, asp, fov = cfg
        th = tan_half(fov)
        S = 0.0
        for cam in cams:                                   # where the rays of the image corners (one pixel outside) meet the plane
            for px in (-1.0, W + 1.0):
                for py in (-1.0, H + 1.0):
                    dr = cam[3:6] + (2 * px / W - 1) * th * asp * cam[6:9] + (1 - 2 * py / H) * th * cam[9:12]
                    assert dr[2] < 0, name
                    hit = cam[0:3] - cam[2] / dr[2] * dr
                    S = max(S, float(np.abs(hit[:2]).max()))
        S *= 1.25
        rng = np.random.default_rng(100 + ci)
        n = 14
        g = np.linspace(-S, S, n)
        V = np.stack(np.meshgrid(g, g, indexing="ij"), -1)
        V[1:-1, 1:-1] += rng.uniform(-0.3, 0.3, size=(n - 2, n - 2, 2)) * (2 * S / (n - 1))
        V = np.concatenate([V, np.zeros((n, n, 1))], -1)
        tri = []
        for i in range(n - 1):
            for j in range(n - 1):
                a, b, c, d = V[i, j], V[i + 1, j], V[i + 1, j + 1], V[i, j + 1]
                tri += [[a, b, c], [a, c, d]] if rng.integers(2) else [[a, b, d], [b, c, d]]
        tri = np.array(tri)[rng.permutation(len(tri))]
        tri = np.stack([t[rng.permutation(3)] for t in tri])
        far = 1000.0
        yield raster_case(f"plane/{name}", tri, cfg, cams, near=0.05, far=far)
        yield raster_case(f"plane_links/{name}", tri, cfg, cams, near=0.05, far=far, tri_link=rng.integers(0, 3, len(tri)),
                          link_T=np.tile(np.eye(4), (3, 1, 1)))


def _near_cases():
    for ci in (0, 2):
        cfg = CONFIGS[ci]
        W, H = cfg[0], cfg[1]
        pix = [(1.3, 1.2), (W - 1.6, 2.4), (W / 2 + 0.2, H - 1.3)]
        for name, d0 in (("at_near", NEAR), ("ulp_nearer", float(np.nextafter(NEAR, 0.0))), ("behind", -1.0)):
            t = at_pixels(cfg, [max(d0, 0.5 * NEAR), 0.5, 0.75], pix)
            t[0, 0] = d0                                                       # (a vertex behind the camera keeps its lateral place)
            yield raster_case(f"near/{name}_{ci}", [t], cfg)
        # the dropped facet reaches behind the camera; a facet in front of it and one beyond it are still drawn
        dropped = at_pixels(cfg, [1.0, 1.0, 1.0], pix)
        dropped[0, 0] = -0.5
        yield raster_case(f"near/in_front_still_drawn_{ci}", [dropped] + _quad(cfg, 0.25, 2.2, 2.3, W / 2 + 0.4, H / 2 + 0.3)
                          + _quad(cfg, 2.0, W / 2 - 1.7, H / 2 - 1.6, W - 1.2, H - 1.4), cfg)


def _far_cases():
    for ci in (0, 1, 3):
        cfg = CONFIGS[ci]
        W, H = cfg[0], cfg[1]
        yield raster_case(f"far/straddle_{ci}", _quad(cfg, [2.0, 6.5, 5.75, 2.5], 0.7, 0.6, W - 0.4, H - 0.7), cfg)


def _border_cases():
    for ci in (0, 1, 2):
        cfg = CONFIGS[ci]
        W, H = cfg[0], cfg[1]
        mx, my = W / 2 + 0.3, H / 2 - 0.2
        off = {"left": (-9.3, my - 3, -2.2, my + 3), "right": (W + 1.7, my - 3, W + 8.1, my + 3), "top": (mx - 3, -7.4, mx + 3, -1.6),
               "bottom": (mx - 3, H + 1.2, mx + 3, H + 6.6), "left_within_one_pixel": (-0.9, my - 2, -0.2, my + 2),
               "top_within_one_pixel": (mx - 2, -0.8, mx + 2, -0.1)}
        for name, r in off.items():
            yield raster_case(f"border/off_{name}_{ci}", _quad(cfg, 1.0, *r), cfg)
        over = {"left": (-3.2, my - 2.3, 2.6, my + 2.2), "right": (W - 2.7, my - 2.3, W + 4.1, my + 2.2), "top": (mx - 2.4, -3.3, mx + 2.6, 2.4),
                "bottom": (mx - 2.4, H - 2.6, mx + 2.6, H + 3.3), "top_left": (-2.2, -3.1, 2.7, 2.3), "top_right": (W - 2.4, -2.2, W + 3.3, 2.6),
                "bottom_left": (-4.1, H - 2.3, 2.2, H + 2.7), "bottom_right": (W - 2.6, H - 2.7, W + 2.2, H + 3.1)}
        tri = []
        for k, r in enumerate(over.values()):
            tri += _quad(cfg, 1.0 + 0.125 * k, *r)
        yield raster_case(f"border/overlap_sides_and_corners_{ci}", tri, cfg)
        yield raster_case(f"border/covers_image_from_far_outside_{ci}",
                          [at_pixels(cfg, [1.0, 1.5, 2.0], [(-40.3, -30.2), (3 * W + 50.1, -20.7), (W / 2 - 3.3, 4 * H + 60.4)])], cfg)


def _huge_cases():
    """Projected coordinates of 1e6 and 1e12 pixels (vertices just beyond near, far out sideways): the pixel box must be clamped
    before it is converted to int.  At 1e6 two facets cross the image; at 1e12 the weight of the far vertex is 1e-12 all over the
    image (below the decision margin by definition), so the facets that reach the image there have a one-pixel box."""
    for ci in (0, 1):
        cfg = CONFIGS[ci]
        W, H = cfg[0], cfg[1]
        d = [0.126, 0.127, 0.128]
        for tag, big in (("1e6", 1e6), ("1e12", 1e12)):
            tri = [at_pixels(cfg, d, [(big, 3.3), (big * 1.5, 9.1), (big * 1.25, -big)]),           # wholly off to the right and top
                   at_pixels(cfg, d, [(-big, 3.3), (-big * 1.5, 9.1), (-big * 1.25, big)]),        # wholly off to the left and bottom
                   at_pixels(cfg, d, [(2.3, -big), (7.1, -big * 2), (-big, -big)]),                # off the top
                   at_pixels(cfg, d, [(2.3, big), (7.1, big * 2), (big, big)]),                    # off the bottom
                   # one-pixel boxes in the last pixel: xmax, then ymax, far beyond the range of int
                   at_pixels(cfg, [0.5, 0.126, 0.127], [(W - 0.4, H - 0.3), (big, H - 0.2), (big, H - 0.35)]),
                   at_pixels(cfg, [0.5, 0.126, 0.127], [(W - 0.3, H - 0.4), (W - 0.2, big), (W - 0.35, big)])]
            if ci == 1 or big < 1e9:                                                                # ... and xmin, ymin in the first pixel
                tri += [at_pixels(cfg, [0.5, 0.126, 0.127], [(0.4, 0.3), (-big, 0.2), (-big, 0.35)]),
                        at_pixels(cfg, [0.5, 0.126, 0.127], [(0.3, 0.4), (0.2, -big), (0.35, -big)])]
            if big < 1e9:                                                                           # across the image
                tri += [at_pixels(cfg, [0.5, 0.126, 0.5], [(1.3, 1.2), (big, H / 2 + 0.4), (2.4, H - 1.3)]),
                        at_pixels(cfg, [1.0, 0.126, 0.13], [(W - 1.4, H - 1.3), (-big, -big), (W + big, -big / 2)])]
            yield raster_case(f"huge/{tag}_{ci}", tri, cfg)


def _tiny_image_cases():
    for k, (W, H) in enumerate(((1, 1), (1, 24), (32, 1))):
        for asp, fov in ((1.0, 60.0), (W / H, 35.0), (0.5, 120.0)):
            cfg = (W, H, asp, fov)
            tri = _quad(cfg, 1.0, -2.3, -1.7, W + 2.2, H + 1.9) + _quad(cfg, 0.5, W * 0.3 - 0.4, H * 0.2 - 0.3, W * 0.6 + 0.1, H * 0.7 + 0.2) \
                + [at_pixels(cfg, [0.25, 0.3, 0.35], [(0.1, 0.2), (0.45, 0.15), (0.3, 0.45)])]          # misses the only centre nearby
            yield raster_case(f"tiny_image/{W}x{H}_fov{fov:g}", tri, cfg)


def _degenerate_cases():
    rng = np.random.default_rng(7)
    for ci in (0, 1, 2):
        cfg = CONFIGS[ci]
        W, H = cfg[0], cfg[1]
        p = at_pixels(cfg, [0.5, 0.7, 0.9], [(2.5, 3.5), (W - 2.5, 4.5), (W / 2, H - 2.5)])
        edge_on = np.array([[0.5, -0.2, 0.0], [1.5, 0.3, 0.0], [0.8, 0.1, 0.0]])                   # in a plane through the eye: yc = 0
        tri = [edge_on, [p[0], p[0], p[2]], [p[0], p[1], p[1]], [p[2], p[1], p[2]], [p[1], p[1], p[1]]]
        yield raster_case(f"degenerate/zero_area_{ci}", tri, cfg)
        tri = []
        for h in (1e-1, 1e-2, 1e-3):                                                                # slivers: the smallest height, in pixels
            for _ in range(12):
                a, b = rng.uniform([0.5, 0.5], [W - 0.5, H - 0.5], size=(2, 2))
                # through a pixel centre: the sliver's long edge passes h / 2 from the centre nearest its middle
                c = np.floor((a + b) / 2) + 0.5
                a, b = a + (c - (a + b) / 2), b + (c - (a + b) / 2)
                nrm = np.array([-(b - a)[1], (b - a)[0]]) / np.linalg.norm(b - a)
                s = rng.choice([-1.0, 1.0])
                tri.append(at_pixels(cfg, rng.uniform(0.3, 2.0, 3), [a - s * nrm * h / 2, b - s * nrm * h / 2, c + s * nrm * h / 2]))
        yield raster_case(f"degenerate/slivers_{ci}", tri, cfg)


def _launch_cases():
    cfg = CONFIGS[1]
    W, H, asp, fov = cfg
    rng = np.random.default_rng(11)
    step = (2.0 * (1.0 * tan_half(fov)) * asp) / W                                                 # one pixel at depth 1, in world units
    cams3 = np.stack([AXIS_CAM, AXIS_CAM, AXIS_CAM])
    cams3[1, 1], cams3[2, 2] = 3 * step, -2 * (2.0 * tan_half(fov) / H)                               # shifted by whole pixels
    for F in (1, 255, 256, 257, 513):
        k = rng.permutation(W * H)[:F]
        tri = []
        for q in k:
            c = np.array([q % W + 0.5, q // W + 0.5])
            tri.append(at_pixels(cfg, 1.0, c + np.array([(-0.36, -0.31), (0.38, -0.22), (-0.05, 0.41)]) + rng.uniform(-0.04, 0.04, (3, 2)))
                       [rng.permutation(3)])
        for C in (1, 3):
            yield raster_case(f"launch/F{F}_C{C}", tri, cfg, cams3[:C])


def _link_clamp_cases():
    cfg = CONFIGS[0]
    W, H = cfg[0], cfg[1]
    T = np.tile(np.eye(4), (3, 1, 1))
    T[0, 1, 3], T[1, 2, 3], T[2, 1, 3] = -0.25, 0.25, 0.25                                        # dyadic shifts: posed vertices stay exact sums
    tri = [q for k, d in enumerate((1.0, 1.5, 2.0, 0.75))                                         # four different quads: a swap of links shows
           for q in _quad(cfg, d, W / 2 - 2.3 - 0.4 * k, H / 2 - 2.2 + 0.3 * k, W / 2 + 2.4 - 0.2 * k, H / 2 + 2.1 + 0.5 * k)]
    yield raster_case("link_clamp/minus_one_and_n_links", tri, cfg, tri_link=[-1, -1, 3, 3, 0, 1, 2, -7], link_T=T)


def _stack_cases():
    rng = np.random.default_rng(13)
    for ci in (0, 1):
        cfg = CONFIGS[ci]
        W, H = cfg[0], cfg[1]
        depths = rng.permutation(np.linspace(0.3, 3.5, 300))
        pix = np.array([(W / 2 - 3.3, H / 2 - 2.4), (W / 2 + 3.4, H / 2 - 1.7), (W / 2 + 0.3, H / 2 + 3.2)])
        tri = [at_pixels(cfg, d, pix + rng.uniform(-0.2, 0.2, (3, 2))) for d in depths]
        yield raster_case(f"stack/300_parallel_{ci}", tri, cfg)


def _shared_edge_cases():
    """Per pixel a pair of facets (A, B, C1), (B, A, C2) whose shared edge A B runs through the pixel's centre to within the
    rounding of the vertices (A = c + v, B = c - l v), C1 and C2 a third of a pixel to either side; every pair at a depth of its
    own, vertex order shuffled.  Whichever side of A B the rounded centre falls, one of the two facets holds it."""
    rng = np.random.default_rng(17)
    for k, (asp, fov) in enumerate(((1.0, 60.0), (16 / 12, 35.0), (0.5, 120.0))):
        cfg = (16, 12, asp, fov)
        W, H = 16, 12
        tri = []
        for q in range(W * H):
            c = np.array([q % W + 0.5, q // W + 0.5])
            th = rng.uniform(0, 2 * np.pi)
            v = rng.uniform(1.5, 3.5) * np.array([np.cos(th), np.sin(th)])
            w = 0.35 * np.array([-np.sin(th), np.cos(th)])
            A, B = c + v, c - rng.uniform(0.5, 1.5) * v
            d = rng.uniform(0.5, 3.0)
            for f in ([A, B, c + w + 0.1 * v], [B, A, c - w - 0.07 * v]):
                tri.append(at_pixels(cfg, d, np.array(f))[rng.permutation(3)])
        yield raster_case(f"shared_edge/bows_{k}", np.array(tri)[rng.permutation(len(tri))], cfg)


def _all_raster():
    out = {}
    for gen in (_plane_cases, _near_cases, _far_cases, _border_cases, _huge_cases, _tiny_image_cases, _degenerate_cases, _launch_cases,
                _link_clamp_cases, _stack_cases, _shared_edge_cases):
        for c in gen():
            assert c.label not in out and len(c.tri) <= 600 and c.W <= 32 and c.H <= 32 and len(c.cams) <= 3, c.label
            for a in (c.tri, c.cams, c.tri_link, c.link_T):
                a.setflags(write=False)
            out[c.label] = c
    return out


RASTER_CASES = _all_raster()
RASTER_FAMILIES = ("plane", "plane_links", "near", "far", "border", "huge", "tiny_image", "degenerate", "launch", "link_clamp", "stack",
                   "shared_edge")


def raster_cases(family=None):
    return [c for c in RASTER_CASES.values() if family is None or family_of(c.label) == family]


# ------------------------------------------------------------------------------------------ visibility families
VIS_EPS = 0.004
CAM_BACK = np.array([4, 0, 0, -1, 0, 0, 0, -1, 0, 0, 0, 1], np.float64)                           # looks down -x from x = 4


def _dyadic(v):
    return math.frexp(v)[0] == 0.5


def vis_cases():
    """-> list of NS(case (a raster case: the occluders), pts, expect, exact_ok, tags).  zb-edge points depend on the buffer and
    are added by `with_zb_edge_points`."""
    out = []
    for ci in (0, 1, 2):
        cfg = CONFIGS[ci]
        W, H, asp, fov = cfg
        th = tan_half(fov)
        wall = raster_case(f"vis/edges_{ci}", _quad(cfg, 1.0, W // 4 + 0.3, H // 4 + 0.2, 3 * W // 4 + 0.4, 3 * H // 4 + 0.3), cfg)
        inside, outside = (W // 2 + 0.5, H // 2 + 0.5), (1.5, 1.5)
        d = 0.5
        rows = [(at_pixels(cfg, NEAR, [inside])[0], True, True), (at_pixels(cfg, float(np.nextafter(NEAR, 0)), [inside])[0], False, True),
                (at_pixels(cfg, FAR, [outside])[0], True, True), (at_pixels(cfg, float(np.nextafter(FAR, 9)), [outside])[0], False, True),
                ([d, -((d * th) * asp), 0.0], True, _dyadic(asp)), ([d, (d * th) * asp, 0.0], False, _dyadic(asp)),     # nx = -1 / +1
                ([d, 0.0, d * th], True, True), ([d, 0.0, -(d * th)], False, True),                                 # ny = +1 / -1
                (at_pixels(cfg, d, [(-0.5, H / 2 + 0.25)])[0], False, True), (at_pixels(cfg, d, [(W / 2 + 0.25, -0.5)])[0], False, True),
                (at_pixels(cfg, d, [(-0.03125, 2.5)])[0], False, True),
                ([-1.0, 0.01, 0.02], False, True), ([0.0, 0.01, 0.02], False, True),
                (at_pixels(cfg, 2.0, [inside])[0], False, True), (at_pixels(cfg, 0.875, [inside])[0], True, True),
                (at_pixels(cfg, 2.0, [outside])[0], True, True),
                (at_pixels(cfg, 0.126, [(1e12, 3.5)])[0], False, True), (at_pixels(cfg, 0.126, [(2.5, -1e12)])[0], False, True)]
        out.append(NS(case=wall, pts=np.array([r[0] for r in rows], np.float64), expect=np.array([r[1] for r in rows]),
                      exact_ok=np.array([r[2] for r in rows])))
    cfg = CONFIGS[0]
    cam1 = AXIS_CAM.copy()
    cam1[1] = 0.015625
    walls = raster_case("vis/three_cams", [[[1, -4, -4], [1, 4, -4], [1, 0, 6]], [[3, -4, -4], [3, 0, 6], [3, 4, -4]]], cfg,
                        np.stack([AXIS_CAM, cam1, CAM_BACK]))
    rows = [([3.5, 0.05, 0.04], True), ([2.0, 0.05, 0.04], False), ([0.5, 0.05, 0.04], True), ([3.5, 0.1, -0.1], True),
            ([2.5, -0.1, 0.1], False), ([-1.0, 0.0, 0.0], False), ([3.875, 0.0, 0.0], True)]
    three = NS(case=walls, pts=np.array([r[0] for r in rows], np.float64), expect=np.array([r[1] for r in rows]),
               exact_ok=np.ones(len(rows), bool))
    out.append(three)
    base = out[0]
    for n in (1, 255, 256, 257):
        k = (np.arange(n) * 7 + 3) % len(base.pts)
        c = raster_case(f"vis/n{n}", base.case.tri, CONFIGS[0])
        out.append(NS(case=c, pts=base.pts[k], expect=base.expect[k], exact_ok=base.exact_ok[k]))
    return out


def with_zb_edge_points(v, depth):
    """Adds, for up to four covered pixels of camera 0, a point at exactly fl(zb + eps) on the pixel's centre ray (visible) and one
    an ulp beyond (not), from the GIVEN buffer.  Only for axis-camera cases (d is the x coordinate)."""
    case = v.case
    if len(case.cams) != 1:
        return v
    cfg = (case.W, case.H, case.aspect, case.fov)
    yx = np.argwhere(np.isfinite(depth[0]))
    yx = yx[np.linspace(0, len(yx) - 1, 4).astype(int)]
    pts, exp = [], []
    for y, x in yx:
        thr = float(depth[0, y, x]) + VIS_EPS
        for d, e in ((thr, True), (float(np.nextafter(thr, np.inf)), False)):
            p = at_pixels(cfg, d, [(x + 0.5, y + 0.5)])[0]
            assert p[0] == d
            pts.append(p)
            exp.append(e)
    return NS(case=case, pts=np.concatenate([v.pts, pts]), expect=np.concatenate([v.expect, exp]),
              exact_ok=np.concatenate([v.exact_ok, np.ones(len(exp), bool)]))


# ------------------------------------------------------------------------------------------ sampler families
def _sample_case(label, cum_area, u, tri_link=None, link_T=None, seed=0, expect_pick=None, tri=None, expect_exact=None):
    F = len(cum_area)
    rng = np.random.default_rng(seed)
    tri = rng.uniform(-0.5, 0.5, size=(F, 3, 3)) if tri is None else np.asarray(tri, np.float64)
    c = NS(label=label, tri=np.ascontiguousarray(tri), cum_area=np.asarray(cum_area, np.float64),
           tri_link=np.zeros(F, np.int32) if tri_link is None else np.asarray(tri_link, np.int32),
           link_T=np.eye(4)[None].copy() if link_T is None else np.ascontiguousarray(link_T, np.float64),
           u=np.ascontiguousarray(np.asarray(u, np.float64).reshape(-1, 3)),
           expect_pick=None if expect_pick is None else np.asarray(expect_pick), expect_exact=expect_exact)
    assert np.all(np.diff(c.cum_area) >= 0) and 1 <= F <= 1025 and len(c.u) <= 8200
    return c


def _rot_z(a, t=(0.0, 0.0, 0.0)):
    T = np.eye(4)
    T[0, 0], T[0, 1], T[1, 0], T[1, 1] = math.cos(a), -math.sin(a), math.sin(a), math.cos(a)
    T[:3, 3] = t
    return T


def _dyadic_table(F, total):
    """F - 1 equal dyadic areas and a last one taking the rest: cum_area[-1] = total, a power of two."""
    step = total / (2 ** math.ceil(math.log2(F)) if F > 1 else 1) / (2 if F > 1 else 1)
    cum = step * np.arange(1, F + 1)
    cum[-1] = total
    return cum


def sample_cases():
    out = []
    rng = np.random.default_rng(21)
    # whole table: a u0 at the lower boundary and at the midpoint of every triangle, dyadic and exact
    for F, total in ((1, 1.0), (2, 0.5), (1000, 2.0), (1025, 1.0)):
        cum = _dyadic_table(F, total)
        lower = np.concatenate([[0.0], cum[:-1]])
        u0 = np.concatenate([lower, (lower + cum) / 2]) / total
        u = np.stack([u0, rng.uniform(0, 1, len(u0)), rng.uniform(0, 1, len(u0))], 1)
        out.append(_sample_case(f"table/F{F}", cum, u, seed=F, expect_pick=np.concatenate([np.arange(F), np.arange(F)])))
    # zero-area triangles: runs of equal cum_area at the start, in the middle, at the end
    areas = np.array([0, 0, 4, 0, 0, 0, 2, 1, 0, 1, 0, 0], np.float64) / 8
    cum = np.cumsum(areas)
    nz = np.nonzero(areas)[0]
    lower = cum[nz] - areas[nz]
    u0 = np.concatenate([lower, lower + areas[nz] / 2, [float(np.nextafter(1.0, 0.0))]])
    u = np.stack([u0, rng.uniform(0, 1, len(u0)), rng.uniform(0, 1, len(u0))], 1)
    out.append(_sample_case("zero_run/start_middle_end", cum, u, seed=3, expect_pick=np.concatenate([nz, nz, [nz[-1]]])))
    # u0 = 1.0: out of contract, bounded: the last triangle, whatever its area
    for name, cum in (("plain", _dyadic_table(5, 1.0)), ("zero_area_last", np.cumsum(areas)), ("single", np.array([0.75]))):
        out.append(_sample_case(f"u0_one/{name}", cum, [[1.0, 0.25, 0.5], [1.0, 1.0, 1.0]], seed=4, expect_pick=[len(cum) - 1] * 2))
    # rounding: a non-dyadic table and u0 an ulp or two around every boundary: the pick follows fl(u0 * total)
    cum = np.cumsum(np.random.default_rng(22).uniform(0.01, 1.0, 300))
    u0 = []
    for k in range(len(cum) - 1):
        c = cum[k] / cum[-1]
        for s in range(-3, 4):
            u0.append(float(c + s * np.spacing(c)))
    u = np.stack([np.array(u0), rng.uniform(0, 1, len(u0)), rng.uniform(0, 1, len(u0))], 1)
    out.append(_sample_case("rounding/non_dyadic", cum, u, seed=5))
    # barycentric corners through the identity pose: the vertex itself
    tri = np.random.default_rng(23).uniform(-1, 1, size=(4, 3, 3))
    cum = _dyadic_table(4, 1.0)
    mid = (np.concatenate([[0.0], cum[:-1]]) + cum) / 2
    u, want = [], []
    for f in range(4):
        for (u1, u2), v in (((0.0, 0.0), 0), ((0.0, 0.7), 0), ((1.0, 0.0), 1), ((1.0, 1.0), 2)):
            u.append([mid[f], u1, u2])
            want.append(tri[f, v])
    out.append(_sample_case("corner/identity", cum, u, tri=tri, expect_pick=np.repeat(np.arange(4), 4), expect_exact=np.array(want)))
    # link poses: a rotation by pi, a translation of 1e3, both
    T = np.stack([_rot_z(math.pi), _rot_z(0.3, (1e3, -1e3, 1e3)), _rot_z(math.pi, (1e3, 2.5, -1e3)), np.eye(4)])
    F = 64
    cum = _dyadic_table(F, 1.0)
    u = rng.uniform(0, 1, size=(300, 3))
    out.append(_sample_case("pose/pi_and_1e3", cum, u, tri_link=np.arange(F) % 4, link_T=T, seed=6))
    # link indices outside [0, L) behave as 0 and L - 1
    out.append(_sample_case("sample_links/out_of_range", cum, u, tri_link=np.tile([-1, 4, 0, 3, -5, 9, 1, 2], 8), link_T=T, seed=7))
    for n in (1, 255, 256, 257):
        out.append(_sample_case(f"sample_launch/n{n}", cum, rng.uniform(0, 1, size=(n, 3)), tri_link=np.arange(F) % 4, link_T=T, seed=8))
    return out


SAMPLE_FAMILIES = ("table", "zero_run", "u0_one", "rounding", "corner", "pose", "sample_links", "sample_launch")


# ------------------------------------------------------------------------------------------ FPS families
FPS_SIZES = (1, 2, 63, 64, 65, 1023, 1024, 1025, 8191, 8192, 8193, 8200)


def fps_ms(n):
    return sorted({1, n if n <= 1025 else 64})


def lattice_cloud(n, seed):
    """n DISTINCT points of the 32^3 integer lattice, shuffled."""
    k = np.random.default_rng(seed).permutation(32 ** 3)[:n]
    return np.stack([k % 32, (k // 32) % 32, k // 1024], 1).astype(np.float64)


def tie_pair_cloud(n, a, b, seed):
    """Point 0 at the origin, every other point in [0, 15]^3 except a and b, the two corners (31,0,0) and (0,31,0): the second
    selection is a tie between exactly a and b, wherever the kernel holds them."""
    X = np.random.default_rng(seed).integers(0, 16, size=(n, 3)).astype(np.float64)
    X[0] = 0.0
    X[a], X[b] = (31.0, 0.0, 0.0), (0.0, 31.0, 0.0)
    return X


def tie_pairs(n):
    """(name, a, b): indices of the tied pair by where k_fps holds them (index = slot * 1024 + thread, wave = thread / 64)."""
    pairs = [("lane", 64 * 3 + 5, 64 * 3 + 60), ("lane_swapped", 64 * 3 + 60, 64 * 3 + 5), ("wave", 64 * 2 + 7, 64 * 9 + 3),
             ("wave_swapped", 64 * 9 + 3, 64 * 2 + 7), ("last_wave", 64 * 15 + 63, 64 * 14), ("slot", 5 + 1024, 5 + 3 * 1024),
             ("slot_last", 77 + 1024 * 2, 77 + 1024 * 7), ("crossed_slot_wave", 1000, 1024 + 2), ("crossed_slot_lane", 70, 1024 + 65),
             ("global_only", 8192 + 3, 8192 + 5), ("global_crossed", 8000, 8192 + 1)]
    return [(nm, a, b) for nm, a, b in pairs if max(a, b) < n]


def fps_cases():
    """-> list of (label, X, m)."""
    out = []
    for n in FPS_SIZES:
        X = lattice_cloud(n, 300 + n)
        for m in fps_ms(n):
            out.append((f"fps_lattice/n{n}_m{m}", X, m))
        out.append((f"fps_identical/n{n}", np.tile([3.0, 5.0, 7.0], (n, 1)), min(n, 64)))
        if n >= 1023:
            for nm, a, b in tie_pairs(n):
                out.append((f"fps_tie/{nm}_n{n}", tie_pair_cloud(n, a, b, n), 4))
            # a coarse lattice: 4^3 distinct points repeated all over the cloud, ties at every selection and in every stage
            k = np.random.default_rng(n).integers(0, 64, size=n)
            out.append((f"fps_coarse/n{n}", np.stack([k % 4, (k // 4) % 4, k // 16], 1).astype(np.float64) * 8.0, 64))
    blk = lattice_cloud(300, 9)
    out.append(("fps_blocks/4x300", np.tile(blk, (4, 1)), 300))
    out.append(("fps_blocks/9x1000", np.tile(lattice_cloud(1000, 10), (9, 1))[:8200], 64))
    return out


def fps_path_pair():
    """(X of 8192 distinct lattice points, the same with a copy of point 0 appended, m): the register kernel and the global
    memory kernel on the same data -- the appended point ties with point 0 at distance 0 and is never the first maximum."""
    X = lattice_cloud(8192, 77)
    return X, np.concatenate([X, X[:1]]), 64
