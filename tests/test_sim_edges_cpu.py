"""CPU: the families and references of tests/_sim_edges.py are kept honest without a GPU.

The oracle restatements the GPU results are compared with bit for bit (oracle.sim_data.visibility / sample_mesh, the compiled
oracle.kmeans.farthest_point_sample) go through every family and through the very comparisons tests/test_gpu_sim_edges.py makes
against the exact rational references; that run also produces the figures recorded in _sim_edges.MEASURED_DEV and the undecided
shares.  The families reach every kernel decision they are built for, and every named wrong variant of the helper's own
restatement is rejected by those comparisons -- the stand-in for mutating the kernels."""
import functools
from fractions import Fraction as Fr

import numpy as np
import pytest

import _sim_edges as E


def _oracle_depth(c, pts=None):
    from oracle import sim_data as osim
    return osim.visibility(c.tri, c.tri_link, c.link_T, c.cams, np.zeros((1, 3)) if pts is None else pts, fov_deg=c.fov,
                           aspect=c.aspect, near=c.near, far=c.far, width=c.W, height=c.H, eps=E.VIS_EPS)


@functools.lru_cache(maxsize=None)
def _raster_runs():
    """Every raster case through the oracle and the comparison: {label: (oracle depth, deviation, undecided share)}."""
    out = {}
    for c in E.raster_cases():
        depth = _oracle_depth(c)[1]
        out[c.label] = (depth,) + E.check_raster(c, depth)
    return out


@functools.lru_cache(maxsize=None)
def _vis_runs():
    out = []
    for v in E.vis_cases():
        depth = _oracle_depth(v.case)[1]
        v = E.with_zb_edge_points(v, depth)
        out.append((v, depth, _oracle_depth(v.case, v.pts)[0]))
    return out


@functools.lru_cache(maxsize=None)
def _sample_runs():
    from oracle import sim_data as osim
    return [(c,) + osim.sample_mesh(c.tri, c.cum_area, c.tri_link, c.link_T, c.u) for c in E.sample_cases()]


def _bits(a):
    return np.ascontiguousarray(a, np.float64).view(np.int64)


# ------------------------------------------------------------------------------------------ references against each other
def test_helper_restatement_equals_the_oracle_bit_for_bit():
    """With no variant the helper's own restatement IS the oracle's (two independent restatements of the same kernels)."""
    for c in E.raster_cases():
        assert (_bits(E.restated_raster(c)) == _bits(_raster_runs()[c.label][0])).all(), c.label
    for v, depth, ovis in _vis_runs():
        assert (E.restated_visible(v.case, v.pts, depth, E.VIS_EPS) == ovis).all(), v.case.label
    for c, out, links in _sample_runs():
        own, own_links = E.restated_sample(c.tri, c.cum_area, c.tri_link, c.link_T, c.u)
        assert (_bits(own) == _bits(out)).all() and (own_links == links).all(), c.label


def test_exact_rasteriser_gives_the_analytic_plane_depth_exactly():
    """Perspective-correct interpolation over coplanar facets is exact in rationals: exact_raster must EQUAL the ray / plane
    intersection computed another way, on every pixel, and leave none empty."""
    for c in E.raster_cases("plane"):
        ex, _ = E.exact_of(c)
        for cam, e in zip(c.cams, ex):
            assert e.drawn.all(), c.label
            for y in range(c.H):
                for x in range(c.W):
                    assert e.depth[y][x] == E.plane_depth(cam, E.tan_half(c.fov), c.aspect, c.W, c.H, x, y), (c.label, x, y)


def test_exact_rasteriser_states_the_documented_conventions():
    """What the near / far / border / degenerate cases are built to show, asserted on the exact reference itself."""
    ex = {c.label: E.exact_of(c)[0] for c in E.raster_cases() if E.family_of(c.label) in ("near", "far", "border", "degenerate", "stack",
                                                                                          "link_clamp", "launch")}
    for label, e in ex.items():
        drawn = sum(int(k.drawn.sum()) for k in e)
        if any(t in label for t in ("ulp_nearer", "behind", "border/off_", "zero_area")):
            assert drawn == 0, label
        if "at_near" in label:
            assert drawn > 20, label                                   # one vertex AT near: drawn
        if "in_front_still_drawn" in label:
            d = {k.depth[y][x] for k in e for y, x in np.argwhere(k.drawn)}
            assert d == {Fr(0.25), Fr(2.0)}, label                     # the facets before and beyond the dropped one, nothing of it
        if label.startswith("far/"):
            d = [k.depth[y][x] for k in e for y, x in np.argwhere(k.drawn)]
            assert max(d) <= Fr(E.FAR) and "far_drop" in e[0].taken and len(d) > 20, label
        if label.startswith("stack/"):
            c = E.RASTER_CASES[label]
            assert min(e[0].depth[y][x] for y, x in np.argwhere(e[0].drawn)) == Fr(float(c.tri[:, 0, 0].min())), label
        if label.startswith("launch/"):
            c = E.RASTER_CASES[label]
            assert int(e[0].drawn.sum()) == len(c.tri), label          # every thread's facet is visible in camera 0
    lc = E.RASTER_CASES["link_clamp/minus_one_and_n_links"]
    good = E.raster_case("x", lc.tri, (lc.W, lc.H, lc.aspect, lc.fov), tri_link=np.clip(lc.tri_link, 0, 2), link_T=lc.link_T)
    want = E.exact_raster(E.posed(good.tri, good.tri_link, good.link_T), good.cams[0], E.tan_half(lc.fov), lc.aspect, lc.W, lc.H, lc.near, lc.far)
    assert want.depth == ex[lc.label][0].depth and want.drawn.sum() > 20


# ------------------------------------------------------------------------------------------ oracle through the GPU comparisons
def test_oracle_passes_every_comparison_and_the_undecided_caps_hold():
    worst = {}
    for c in E.raster_cases():
        _, dev, und = _raster_runs()[c.label]
        fam = E.family_of(c.label)
        if fam in E.EVERY_PIXEL:                                       # all of its pixels sit on a shared edge: that is the family
            assert und >= 0.9, (c.label, und)
            continue
        assert und <= E.CAP, (c.label, und)
        if fam in E.NO_UNDECIDED:
            assert und == 0, (c.label, und)
        worst[fam] = max(worst.get(fam, 0.0), und)
    print({f: f"{100 * u:.2f}%" for f, u in worst.items()})
    assert set(worst) | set(E.EVERY_PIXEL) == set(E.RASTER_FAMILIES)
    for v, depth, ovis in _vis_runs():
        E.check_visible(v.case, v.pts, v.expect, v.exact_ok, depth, E.VIS_EPS, ovis)
    for c, out, links in _sample_runs():
        E.check_sample(c, out, links)


def test_oracle_fps_is_the_plain_loop_on_every_lattice():
    from oracle import kmeans as okm
    for label, X, m in E.fps_cases():
        E.check_fps(X, m, okm.farthest_point_sample(X, m))
        if label.startswith("fps_identical"):
            assert (E.plain_fps(X, m) == 0).all(), label
    A, B, m = E.fps_path_pair()
    assert len(A) == 8192 and len(B) == 8193 and len(np.unique(A, axis=0)) == 8192
    assert (E.plain_fps(A, m) == E.plain_fps(B, m)).all() and (okm.farthest_point_sample(B, m) == E.plain_fps(A, m)).all()
    for n in (1024, 8192, 8200):                                      # the designed pairs: the lower index first, then the other
        for nm, a, b in E.tie_pairs(n):
            sel = E.plain_fps(E.tie_pair_cloud(n, a, b, n), 3)
            assert sel.tolist() == [0, min(a, b), max(a, b)], (nm, n, sel)


def test_measured_deviation_per_family():
    """The restatement's largest relative deviation from the exact depth / point is what _sim_edges.MEASURED_DEV records: not
    above it, and the record not above twice the measurement where 4 x the record is over the floor of the GPU bound."""
    meas = {}
    for c in E.raster_cases():
        f = E.family_of(c.label)
        meas[f] = max(meas.get(f, 0.0), _raster_runs()[c.label][1])
    for c, out, links in _sample_runs():
        f = E.family_of(c.label)
        meas[f] = max(meas.get(f, 0.0), E.check_sample(c, out, links))
    assert set(meas) == set(E.MEASURED_DEV) == set(E.RASTER_FAMILIES) | set(E.SAMPLE_FAMILIES)
    for f, m in sorted(meas.items()):
        print(f"{f:14s} measured {m:.3e}  recorded {E.MEASURED_DEV[f]:.2e}  GPU bound {E.gpu_bound(f):.2e}")
        assert m <= E.MEASURED_DEV[f], (f, m)
        if 4 * E.MEASURED_DEV[f] > E.BOUND_FLOOR:
            assert E.MEASURED_DEV[f] <= 2 * m, (f, m)


# ------------------------------------------------------------------------------------------ the families reach what they are for
def test_families_reach_every_kernel_decision():
    reached = set()
    for c in E.raster_cases():
        reached |= E.exact_of(c)[1]
    for v, depth, _ in _vis_runs():
        c = v.case
        _, tags = E.exact_visible(c.cams, v.pts, E.tan_half(c.fov), c.aspect, c.W, c.H, c.near, c.far, depth, E.VIS_EPS)
        reached |= set().union(*tags)
    for c, _, _ in _sample_runs():
        reached |= E.exact_sample(c.tri, c.cum_area, c.tri_link, c.link_T, c.u)[4]
    for label, X, m in E.fps_cases():
        if len(X) >= 1024:
            reached |= E.plain_fps(X, m, want_ties=True)[1]
    assert reached == set(E.DECISIONS), (set(E.DECISIONS) - reached, reached - set(E.DECISIONS))
    # the rounding family really separates the rounded product from the exact one.  Rounding is monotonic and the entries are
    # floats, so an exact product at or above an entry stays there: the rounded pick can only be LATER (a product just below an
    # entry rounds up onto it, and the strict upper bound then passes that triangle over)
    c = next(c for c, _, _ in _sample_runs() if c.label.startswith("rounding"))
    _, pick, _, rpick, _ = E.exact_sample(c.tri, c.cum_area, c.tri_link, c.link_T, c.u)
    assert (rpick > pick).sum() > 50 and (rpick >= pick).all()
    # sizes and launch shapes the issue names
    assert {len(c.tri) for c in E.raster_cases("launch")} == {1, 255, 256, 257, 513}
    assert {len(c.cams) for c in E.raster_cases("launch")} == {1, 3}
    assert {(c.W, c.H) for c in E.raster_cases("tiny_image")} == {(1, 1), (1, 24), (32, 1)}
    assert {len(c.u) for c in E.sample_cases() if c.label.startswith("sample_launch")} == {1, 255, 256, 257}
    assert {len(c.cum_area) for c in E.sample_cases() if c.label.startswith("table")} == {1, 2, 1000, 1025}
    assert {len(X) for _, X, _ in E.fps_cases()} >= set(E.FPS_SIZES)
    assert max(len(X) for _, X, _ in E.fps_cases()) <= 8200


# ------------------------------------------------------------------------------------------ the cases have teeth
def _rejected(fn):
    try:
        fn()
    except AssertionError:
        return True
    return False


@pytest.mark.parametrize("variant", E.VARIANTS)
def test_every_wrong_variant_is_rejected(variant):
    """Each named way of being subtly wrong differs from the oracle somewhere AND is refused by the comparison with the exact
    references that the GPU test makes (never by bit-equality with a restatement alone)."""
    caught = []
    raster_for = {"near_strict": ("near",), "near_per_pixel": ("near",), "bary_rot": ("far", "stack"), "no_link_clamp": ("link_clamp",),
                  "contracted": ("shared_edge",)}
    for fam in raster_for.get(variant, ()):
        for c in E.raster_cases(fam):
            if _rejected(lambda: E.check_raster(c, E.restated_raster(c, variant))):
                caught.append(c.label)
    if variant in ("near_strict", "vis_trunc", "zb_strict"):
        for v, depth, _ in _vis_runs():
            vis = E.restated_visible(v.case, v.pts, depth, E.VIS_EPS, variant)
            if _rejected(lambda: E.check_visible(v.case, v.pts, v.expect, v.exact_ok, depth, E.VIS_EPS, vis)):
                caught.append(v.case.label)
    if variant in ("bisect_left", "no_link_clamp", "bary_rot"):
        for c, _, _ in _sample_runs():
            out, links = E.restated_sample(c.tri, c.cum_area, c.tri_link, c.link_T, c.u, variant)
            if _rejected(lambda: E.check_sample(c, out, links)):
                caught.append(c.label)
    if variant == "fps_last_tie":
        for label, X, m in E.fps_cases():
            if _rejected(lambda: E.check_fps(X, m, E.plain_fps(X, m, last_tie=True))):
                caught.append(label)
    print(variant, "rejected by", len(caught), "cases, e.g.", caught[:6])
    fams = {E.family_of(l) for l in caught}
    need = {"near_strict": {"near", "vis"}, "near_per_pixel": {"near"}, "bary_rot": {"far", "corner"}, "no_link_clamp": {"link_clamp", "sample_links"},
            "vis_trunc": {"vis"}, "zb_strict": {"vis"}, "bisect_left": {"table", "zero_run"}, "fps_last_tie": {"fps_lattice", "fps_tie", "fps_identical"},
            "contracted": {"shared_edge"}}
    assert need[variant] <= fams, (variant, fams)
