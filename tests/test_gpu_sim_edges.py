"""GPU: csrc/sample.hip (`k_sample_mesh`, `k_raster_depth`, `k_visible`) and csrc/fps.hip (`k_fps`) at their edges -- the families
of tests/_sim_edges.py.

Every result is compared (a) bit for bit with the oracle restatement (oracle.sim_data / the compiled oracle FPS): the existing
contract, now at the edges; and (b) with references that do not restate the kernel: the exact rational rasteriser, visibility
and sampler, and the plain FPS loop on integer lattices.  Against the exact rasteriser drawn / empty must agree on every decided
pixel (margin >= 1e-9), closed surfaces have no hole, and depths / points stay within `_sim_edges.gpu_bound(family)` = max(4 x
the deviation the float64 restatement itself measures on the CPU, 2^-50) -- never anything measured from the kernel.  Outputs
are also written through interior views of sentinel-filled buffers: nothing beyond them may change.
"""
import numpy as np
import pytest
import torch

import _sim_edges as E

pytestmark = pytest.mark.gpu

GUARD = 64                                     # sentinel elements (rows for the points) before and after what a launch may write
SENT64 = 0x7FF8DEAD7FC0DEAD
SENT32 = 0x7FC0DEAD
SENT8 = 0xA5


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "GPU tests need the MI355X"
    from autourdf_amd import _lib
    _lib.load()
    return torch.device("cuda:0")


def _t(a, dev):
    return torch.from_numpy(np.array(a)).to(dev)                               # a copy: the shared host arrays stay as they are


def _bits(a):
    return np.ascontiguousarray(a, np.float64).view(np.int64)


def _guarded(dev, n, dtype):
    """(buffer, interior view of n elements): the buffer holds a sentinel everywhere."""
    buf = torch.empty(n + 2 * GUARD, dtype=dtype, device=dev)
    if dtype == torch.float64:
        buf.view(torch.int64).fill_(SENT64)
    else:
        buf.fill_({torch.int64: SENT64, torch.int32: SENT32, torch.uint8: SENT8}[dtype])
    return buf, buf[GUARD:GUARD + n]


def _guards_intact(buf, n, inner_too=False):
    raw = buf.view(torch.int64) if buf.dtype == torch.float64 else buf
    sent = {torch.float64: SENT64, torch.int64: SENT64, torch.int32: SENT32, torch.uint8: SENT8}[buf.dtype]
    ok = bool((raw[:GUARD] == sent).all() and (raw[GUARD + n:] == sent).all())
    return ok and (not inner_too or bool((raw == sent).all()))


def _oracle_vis(c, pts):
    from oracle import sim_data as osim
    return osim.visibility(c.tri, c.tri_link, c.link_T, c.cams, pts, fov_deg=c.fov, aspect=c.aspect, near=c.near, far=c.far,
                           width=c.W, height=c.H, eps=E.VIS_EPS)


def _mesh(c, dev):
    return _t(c.tri, dev), _t(c.tri_link, dev), _t(c.link_T, dev)


def _cam_args(c):
    return dict(fov_deg=c.fov, aspect=c.aspect, near=c.near, far=c.far, width=c.W, height=c.H)


# ------------------------------------------------------------------------------------------ rasteriser
def _raster_direct(dev, c):
    """creg_raster_depth_f64 into an interior view of a sentinel-filled buffer."""
    from autourdf_amd import _lib, ops
    tri, own, T = _mesh(c, dev)
    cams = _t(c.cams, dev)
    n = len(c.cams) * c.H * c.W
    buf, view = _guarded(dev, n, torch.float64)
    rc = _lib.load().creg_raster_depth_f64(ops._p(tri), ops._p(own), len(c.tri), ops._p(T), len(c.link_T), ops._p(cams), len(c.cams),
                                           c.fov, c.aspect, c.near, c.far, c.W, c.H, ops._p(view), ops._stream())
    torch.cuda.synchronize()
    _lib.check(rc, "creg_raster_depth_f64")
    return buf, view.reshape(len(c.cams), c.H, c.W)


@pytest.mark.parametrize("family", E.RASTER_FAMILIES)
def test_raster_depth_against_the_oracle_and_the_exact_rasteriser(dev, family):
    """Per case: the buffers equal the oracle restatement's bit for bit; against the exact rasteriser drawn / empty agree on
    every decided pixel, every depth is within the family's bound, a tessellated plane has no hole and the analytic ray / plane
    depth, degenerate facets write nothing the exact reference leaves empty; nothing is written beyond the (C,H,W) buffer."""
    from autourdf_amd import ops
    cases = E.raster_cases(family)
    assert cases
    worst = 0.0
    for c in cases:
        tri, own, T = _mesh(c, dev)
        depth = ops.raster_depth(tri, own, T, _t(c.cams, dev), **_cam_args(c))
        assert depth.shape == (len(c.cams), c.H, c.W) and depth.dtype == torch.float64
        got = depth.cpu().numpy()
        buf, direct = _raster_direct(dev, c)
        assert _guards_intact(buf, got.size), c.label
        assert torch.equal(direct.view(torch.int64), depth.view(torch.int64)), c.label
        want = _oracle_vis(c, np.zeros((1, 3)))[1]
        assert (_bits(got) == _bits(want)).all(), (c.label, np.argwhere(_bits(got) != _bits(want))[:4].tolist())
        dev_c, _ = E.check_raster(c, got)
        worst = max(worst, dev_c)
        if family == "stack":                                                  # order independence: twice the same bits (the nearest: check_raster)
            again = ops.raster_depth(tri, own, T, _t(c.cams, dev), **_cam_args(c))
            assert torch.equal(again.view(torch.int64), depth.view(torch.int64)), c.label
    print(f"{family:12s} largest depth deviation on the GPU {worst:.3e}  bound {E.gpu_bound(family):.2e}")


# ------------------------------------------------------------------------------------------ visibility
def test_visibility_edges_against_the_oracle_and_exact_visibility(dev):
    """Points at near / far and an ulp outside, on nx = +-1 and ny = +-1, with px in (-1, 0), behind the camera, 1e12 pixels out,
    at fl(zb + eps) of the buffer READ BACK from the device and an ulp beyond, seen by the third camera only and by none, at
    n = 1, 255, 256, 257: what they were built to be, the oracle's answer, and exact visibility where the construction is exact."""
    from autourdf_amd import _lib, ops
    L = _lib.load()
    n_cases = 0
    for v in E.vis_cases():
        c = v.case
        tri, own, T = _mesh(c, dev)
        cams = _t(c.cams, dev)
        _, depth = ops.visibility(tri, own, T, cams, _t(v.pts, dev), eps=E.VIS_EPS, return_depth=True, **_cam_args(c))
        depth = depth.cpu().numpy()
        v = E.with_zb_edge_points(v, depth)
        pts = _t(v.pts, dev)
        vis, depth2 = ops.visibility(tri, own, T, cams, pts, eps=E.VIS_EPS, return_depth=True, **_cam_args(c))
        assert vis.dtype == torch.bool and (_bits(depth2.cpu().numpy()) == _bits(depth)).all(), c.label
        ovis, odepth = _oracle_vis(c, v.pts)
        assert (_bits(depth) == _bits(odepth)).all(), c.label
        vis = vis.cpu().numpy()
        assert (vis == ovis).all(), (c.label, np.nonzero(vis != ovis)[0][:6].tolist())
        E.check_visible(c, v.pts, v.expect, v.exact_ok, depth, E.VIS_EPS, vis)
        # the same call with `visible` and the workspace as interior views of sentinel-filled buffers
        n, npx = len(v.pts), len(c.cams) * c.H * c.W
        vbuf, vview = _guarded(dev, n, torch.uint8)
        wbuf, wview = _guarded(dev, npx, torch.float64)
        rc = L.creg_visibility_f64(ops._p(tri), ops._p(own), len(c.tri), ops._p(T), len(c.link_T), ops._p(cams), len(c.cams), c.fov, c.aspect,
                                   c.near, c.far, c.W, c.H, ops._p(pts), n, E.VIS_EPS, ops._p(vview), ops._p(wview), 8 * npx, ops._stream())
        torch.cuda.synchronize()
        _lib.check(rc, "creg_visibility_f64")
        assert _guards_intact(vbuf, n) and _guards_intact(wbuf, npx), c.label
        assert (vview.cpu().numpy().astype(bool) == vis).all() and (_bits(wview.cpu().numpy()) == _bits(depth.ravel())).all(), c.label
        n_cases += 1
    assert n_cases == 8


# ------------------------------------------------------------------------------------------ sampler
@pytest.mark.parametrize("family", E.SAMPLE_FAMILIES)
def test_sample_mesh_against_the_oracle_and_the_exact_sampler(dev, family):
    """Per case: points and links equal the oracle restatement's bit for bit; the link of every point and the point itself (within
    the family's bound) equal the exact sampler's -- bisect_right on the exact product, or on the kernel's rounded product in the
    rounding family; corner barycentrics return the vertex itself; nothing is written beyond out (n,3) and link_out (n)."""
    from autourdf_amd import _lib, ops
    from oracle import sim_data as osim
    cases = [c for c in E.sample_cases() if E.family_of(c.label) == family]
    assert cases
    worst = 0.0
    for c in cases:
        d = [_t(a, dev) for a in (c.tri, c.cum_area, c.tri_link, c.link_T, c.u)]
        out, links = ops.sample_mesh(*d, with_links=True)
        alone = ops.sample_mesh(*d)
        assert torch.equal(alone.view(torch.int64), out.view(torch.int64)), c.label
        got, got_links = out.cpu().numpy(), links.cpu().numpy()
        want, want_links = osim.sample_mesh(c.tri, c.cum_area, c.tri_link, c.link_T, c.u)
        assert (_bits(got) == _bits(want)).all() and (got_links == want_links).all(), c.label
        worst = max(worst, E.check_sample(c, got, got_links))
        n = len(c.u)
        obuf, oview = _guarded(dev, 3 * n, torch.float64)
        lbuf, lview = _guarded(dev, n, torch.int32)
        rc = _lib.load().creg_sample_mesh_f64(ops._p(d[0]), ops._p(d[1]), ops._p(d[2]), len(c.tri), ops._p(d[3]), len(c.link_T), ops._p(d[4]),
                                              n, ops._p(oview), ops._p(lview), ops._stream())
        torch.cuda.synchronize()
        _lib.check(rc, "creg_sample_mesh_f64")
        assert _guards_intact(obuf, 3 * n) and _guards_intact(lbuf, n), c.label
        assert torch.equal(oview.view(torch.int64), out.reshape(-1).view(torch.int64)) and torch.equal(lview, links), c.label
    print(f"{family:14s} largest point deviation on the GPU {worst:.3e}  bound {E.gpu_bound(family):.2e}")


# ------------------------------------------------------------------------------------------ FPS
def _fps_direct(dev, X, m):
    """creg_fps_f64 with sel and the scratch as interior views of sentinel-filled buffers."""
    from autourdf_amd import _lib, ops
    L = _lib.load()
    Xd = _t(X, dev)
    n = len(X)
    sbuf, sview = _guarded(dev, m, torch.int64)
    nscr = max(int(L.creg_fps_scratch_bytes(n)) // 8, 1)
    cbuf, cview = _guarded(dev, nscr, torch.float64)
    rc = L.creg_fps_f64(ops._p(Xd), n, m, ops._p(sview), ops._p(cview), ops._stream())
    torch.cuda.synchronize()
    _lib.check(rc, "creg_fps_f64")
    assert _guards_intact(sbuf, m) and _guards_intact(cbuf, nscr), (n, m)
    return sview.cpu().numpy()


def test_fps_sizes_ties_and_both_kernel_paths(dev):
    """Every size around 64 / 1024 / 8192 with m = 1, m = n (n <= 1025) and m = 64: the plain first-maximum loop on integer
    lattices (exact distances: any correct implementation agrees bit for bit), the compiled oracle, tied maxima placed in
    different register slots, lanes and waves (the lowest index wins), identical points (all zeros), duplicated blocks; sel and
    the scratch are written inside their bounds only."""
    from autourdf_amd.fps import farthest_point_sample
    from oracle import kmeans as okm
    n_cases = 0
    for label, X, m in E.fps_cases():
        sel = farthest_point_sample(X, m)
        assert sel.dtype == np.int64
        E.check_fps(X, m, sel)
        assert (sel == okm.farthest_point_sample(X, m)).all(), label
        if label.startswith("fps_identical"):
            assert (sel == 0).all(), label
        if label.startswith(("fps_lattice", "fps_tie/slot", "fps_tie/crossed", "fps_tie/global", "fps_blocks")):
            assert (_fps_direct(dev, X, m) == sel).all(), label
        n_cases += 1
    assert n_cases == len(E.fps_cases()) >= 3 * len(E.FPS_SIZES)
    for n in (1024, 8192, 8200):
        for nm, a, b in E.tie_pairs(n):
            assert farthest_point_sample(E.tie_pair_cloud(n, a, b, n), 3).tolist() == [0, min(a, b), max(a, b)], (nm, n)


def test_fps_register_path_equals_global_memory_path(dev):
    """8192 distinct lattice points run in registers; with a copy of point 0 appended (8193) the global-memory kernel runs on
    the same data, and the copy (distance 0 to the first selection) is never a first maximum: identical selections."""
    from autourdf_amd.fps import farthest_point_sample
    A, B, m = E.fps_path_pair()
    sa, sb = farthest_point_sample(A, m), farthest_point_sample(B, m)
    assert (sa == sb).all() and (sa == E.plain_fps(A, m)).all() and len(set(sa.tolist())) == m
    assert (farthest_point_sample(_t(A, dev), m) == sa).all()                  # a device tensor in: the same


# ------------------------------------------------------------------------------------------ refusals
class _NoLaunch:
    """Stands in for a C entry point: the wrapper must refuse before it gets here."""
    def __init__(self):
        self.calls = 0

    def __call__(self, *a):
        self.calls += 1
        return 0


def _sample_args(dev):
    c = next(c for c in E.sample_cases() if c.label == "pose/pi_and_1e3")
    return {k: _t(getattr(c, k), dev) for k in ("tri", "cum_area", "tri_link", "link_T", "u")}


def _vis_args(dev):
    v = E.vis_cases()[3]
    c = v.case
    return dict(tri=_t(c.tri, dev), tri_link=_t(c.tri_link, dev), link_T=_t(c.link_T, dev), cams=_t(c.cams, dev), pts=_t(v.pts, dev))


SAMPLE_BAD = {"cum_area_short": lambda a: a.update(cum_area=a["cum_area"][:-1]), "tri_link_short": lambda a: a.update(tri_link=a["tri_link"][:-1]),
              "tri_link_long": lambda a: a.update(tri_link=torch.cat([a["tri_link"], a["tri_link"]])),
              "tri_flat": lambda a: a.update(tri=a["tri"].reshape(-1, 9)), "tri_Fx3x2": lambda a: a.update(tri=a["tri"][:, :, :2]),
              "u_nx2": lambda a: a.update(u=a["u"][:, :2]), "u_empty": lambda a: a.update(u=a["u"][:0]), "u_flat": lambda a: a.update(u=a["u"].reshape(-1)),
              "link_T_4x4": lambda a: a.update(link_T=a["link_T"][0]), "link_T_Lx3x4": lambda a: a.update(link_T=a["link_T"][:, :3]),
              "link_T_empty": lambda a: a.update(link_T=a["link_T"][:0])}
VIS_BAD = {"tri_link_short": lambda a: a.update(tri_link=a["tri_link"][:-1]), "tri_flat": lambda a: a.update(tri=a["tri"].reshape(-1, 9)),
           "cams_width_11": lambda a: a.update(cams=a["cams"][:, :11]), "cams_flat": lambda a: a.update(cams=a["cams"].reshape(-1)),
           "cams_empty": lambda a: a.update(cams=a["cams"][:0]), "pts_nx2": lambda a: a.update(pts=a["pts"][:, :2]),
           "pts_empty": lambda a: a.update(pts=a["pts"][:0]), "link_T_4x4": lambda a: a.update(link_T=a["link_T"][0]),
           "width_0": lambda a: a.update(width=0), "height_0": lambda a: a.update(height=0)}


@pytest.mark.parametrize("what", sorted(SAMPLE_BAD))
def test_sample_mesh_refuses_wrong_shapes_before_any_launch(dev, monkeypatch, what):
    from autourdf_amd import _lib, ops
    a = _sample_args(dev)
    ops.sample_mesh(**a)                                                       # the unchanged arguments are accepted
    SAMPLE_BAD[what](a)
    stub = _NoLaunch()
    monkeypatch.setattr(_lib.load(), "creg_sample_mesh_f64", stub, raising=False)
    with pytest.raises(ValueError, match="sample_mesh: "):
        ops.sample_mesh(**a)
    assert stub.calls == 0


@pytest.mark.parametrize("what", sorted(VIS_BAD))
def test_visibility_refuses_wrong_shapes_before_any_launch(dev, monkeypatch, what):
    from autourdf_amd import _lib, ops
    a = _vis_args(dev)
    a.update(width=16, height=12)
    ops.visibility(**a)
    VIS_BAD[what](a)
    stub = _NoLaunch()
    monkeypatch.setattr(_lib.load(), "creg_visibility_f64", stub, raising=False)
    with pytest.raises(ValueError, match="visibility: "):
        ops.visibility(**a)
    assert stub.calls == 0
    if not what.startswith("pts"):                                             # raster_depth takes the same mesh / camera arguments
        stub = _NoLaunch()
        monkeypatch.setattr(_lib.load(), "creg_raster_depth_f64", stub, raising=False)
        a.pop("pts")
        with pytest.raises(ValueError, match="raster_depth: "):
            ops.raster_depth(**a)
        assert stub.calls == 0


def test_c_entry_points_refuse_empty_inputs_and_write_nothing(dev):
    """n = 0 / F = 0 at the C ABI: an error code, creg_last_error() set, the outputs still hold the sentinel."""
    from autourdf_amd import _lib, ops
    L = _lib.load()
    a = _sample_args(dev)
    obuf, oview = _guarded(dev, 30, torch.float64)
    lbuf, lview = _guarded(dev, 10, torch.int32)
    for F, n in ((64, 0), (0, 10)):
        rc = L.creg_sample_mesh_f64(ops._p(a["tri"]), ops._p(a["cum_area"]), ops._p(a["tri_link"]), F, ops._p(a["link_T"]), 4, ops._p(a["u"]), n,
                                    ops._p(oview), ops._p(lview), ops._stream())
        torch.cuda.synchronize()
        assert rc != 0 and b"creg_sample_mesh_f64" in L.creg_last_error()
    assert _guards_intact(obuf, 30, inner_too=True) and _guards_intact(lbuf, 10, inner_too=True)
    v = _vis_args(dev)
    vbuf, vview = _guarded(dev, 16, torch.uint8)
    wbuf, wview = _guarded(dev, 16 * 12, torch.float64)
    for n, W in ((0, 16), (7, 0)):
        rc = L.creg_visibility_f64(ops._p(v["tri"]), ops._p(v["tri_link"]), 2, ops._p(v["link_T"]), 1, ops._p(v["cams"]), 1, 60.0, 1.0, 0.125, 4.0,
                                   W, 12, ops._p(v["pts"]), n, 0.004, ops._p(vview), ops._p(wview), 8 * 16 * 12, ops._stream())
        torch.cuda.synchronize()
        assert rc != 0 and b"creg_visibility_f64" in L.creg_last_error()
    assert _guards_intact(vbuf, 16, inner_too=True) and _guards_intact(wbuf, 16 * 12, inner_too=True)
    sbuf, sview = _guarded(dev, 8, torch.int64)
    X = _t(E.lattice_cloud(8, 1), dev)
    for n, m in ((0, 1), (8, 0), (8, 9)):
        rc = L.creg_fps_f64(ops._p(X), n, m, ops._p(sview), ops._p(wview), ops._stream())
        torch.cuda.synchronize()
        assert rc != 0 and b"creg_fps_f64" in L.creg_last_error()
    assert _guards_intact(sbuf, 8, inner_too=True)
