"""The five batched mesh queries across their launch slices, on dirty workspaces and with loose table ends, through the C ABI:
creg_mesh_collide_f64, creg_mesh_clearance_f64, creg_mesh_contain_f64, creg_point_mesh_f64 and creg_mesh_cover_f64 (scenes and the
tiling scheme: tests/_mesh_slices.py; their conditions: tests/test_mesh_slices_cpu.py).

Every check has one shape.  The entry runs on the 7 pose templates (or the 11 base pairs), and that short call is held to the numpy
restatement by the `check` of the entry's own test file with its own bound -- the only inexact comparison here.  Then the long call
runs, 65544 poses or 65544 pairs, and its rows must be BIT IDENTICAL to the short call's rows tiled by p % 7 or m % 11: the header
makes a row a function of its own pose and pair alone, so no tolerance enters, and nothing long is restated on the CPU.

Why a lost offset cannot pass.  The host loops launch poses [p0, p0 + 65535) and pairs [m0, m0 + 65535) (contain: 32767), and the
kernels of a later launch index p = p0 + blockIdx.z, m = m0 + blockIdx.y in every place: the pose's matrices, `posed`, the chunk
and link boxes, the output row, collide's keys, clearance's and contain's partial slots.  65535 % 7 = 1, 65535 % 11 = 8 and
32767 % 11 = 9 (then 65534 % 11 = 7), so block 0 of a later launch stands for template 1, base pair 8, 9 or 7 -- never for the
template or pair that block 0 of the first launch stood for.  Drop `p0 +` or `m0 +` from any one read and the block computes with
template b % 7 or pair b % 11 where (b + 1) % 7, (b + 8) % 11 belong: the CPU file shows that all seven templates answer
differently and that on the two templates of the pair slice the base-pair answers differ from themselves rolled by 8 (contain: by
9 and by 7), so some row of the later launch differs.  Drop it from a write and the rows of the later launch keep their sentinel (or collide's memset zero, where the
tiled rows have counts) while rows of the first launch are written twice -- collide's count then doubles.  Drop it from
mesh_pose_launch's kernels and the later poses read `posed` and boxes that still hold the NaN pattern the workspace was filled
with.  Either way a byte differs.  link_box is compared tiled as well, so the posing stage is pinned on its own.

Every call here runs on a workspace filled with a NaN-with-payload pattern with 64 guard words behind its stated size, and writes
outputs that are pre-filled with sentinels and followed by 64 sentinel rows: the guards must come back untouched and no output
element may keep its sentinel.  A slot that is read without having been written would carry the NaN, or differ between the
zero-filled and the pattern-filled run.  tri_start[0] = -5, tri_start[L] = F + 7 (contain: pt_start likewise) are inside the
header's contract, which clamps them; no input here is outside it."""
import ctypes

import numpy as np
import pytest
import torch

import _mesh_cover_ref as mcref
import _mesh_slices as ms
from test_gpu_clearance import check as check_clearance
from test_gpu_collide import same as check_collide
from test_gpu_contain import check as check_contain
from test_gpu_mesh_cover import check as check_mesh_cover
from test_gpu_point_mesh import check as check_point_mesh

pytestmark = pytest.mark.gpu
INF = np.inf
ENTRIES = ("collide", "clearance", "contain", "point_mesh", "mesh_cover")
PAIR_ENTRIES = ENTRIES[:3]
GUARD = 64
NAN_WORD = -2251799813685247                                     # 0xFFF8000000000001: a NaN with a payload
INT_SENTINEL = -7                                                # no count, row or index is ever -7
NAMES = {"collide": ("count", "first", "link_box"), "clearance": ("dist2", "witness", "link_box"),
         "contain": ("inside", "first", "winding", "link_box"), "point_mesh": ("dist2", "tri_idx", "link_box"),
         "mesh_cover": ("dist2", "pt_idx", "n_near", "link_box")}


def dev(a):
    return a if isinstance(a, torch.Tensor) else torch.from_numpy(np.array(a)).to("cuda")   # a copy: the shared host arrays stay as they are


def ptr(t):
    return ctypes.c_void_p(t.data_ptr())


class Out:
    """An output of ``rows`` rows of ``width`` elements, pre-filled with its sentinel, GUARD sentinel rows behind it."""

    def __init__(self, rows, width, dtype):
        self.n, self.dtype = rows * width, dtype
        total = self.n + GUARD * width
        if dtype == torch.float64:
            self.raw = torch.full((total,), NAN_WORD, dtype=torch.int64, device="cuda")
            self.sentinel = NAN_WORD
        else:
            self.raw = torch.full((total,), INT_SENTINEL, dtype=torch.int32, device="cuda")
            self.sentinel = INT_SENTINEL
        self.ptr = ptr(self.raw)

    def take(self, shape, name):
        assert bool((self.raw[self.n:] == self.sentinel).all()), f"{name}: written past its stated size"
        assert not bool((self.raw[:self.n] == self.sentinel).any()), f"{name}: an element kept its sentinel"
        body = self.raw[:self.n].cpu().numpy()
        return (body.view(np.float64) if self.dtype == torch.float64 else body).reshape(shape)


def workspace(need, fill):
    assert need > 0 and need % 8 == 0
    ws = torch.full((need // 8 + GUARD,), NAN_WORD, dtype=torch.int64, device="cuda")
    if fill == "zero":
        ws[:need // 8] = 0
    return ws


def geometry(entry, loose=False):
    """The entry's scene as a dict of host arrays and its (7,L,4,4) templates; ``loose`` puts the table ends outside 0 .. n."""
    if entry == "contain":
        tri, start, pts, pt_start, templates = ms.contain_scene()
        if loose:
            start, pt_start = ms.loose(start, len(tri)), ms.loose(pt_start, len(pts), ms.LOOSE_PTS)
        return dict(tri=tri, start=start, pts=pts, pt_start=pt_start), templates
    tri, start, templates = ms.scene()
    return dict(tri=tri, start=ms.loose(start, len(tri)) if loose else start), templates


def run(entry, link_T, pairs=None, cloud=None, d_max=ms.D_MAX, fill="nan", loose=False):
    """The C entry on the entry's scene under ``link_T`` (P,L,4,4): its outputs in the header's order, link_box last, as numpy
    arrays.  Pair entries take ``pairs`` (default: the 6 valid pairs), point entries ``cloud`` = (pts, pt_start) (default: the
    templates' clouds).  Guards and sentinels are checked on the way out."""
    from autourdf_amd import _lib
    lib = _lib.load()
    g, _ = geometry(entry, loose)
    F = len(g["tri"])
    tri, start, link_T = dev(g["tri"]), dev(g["start"]), dev(link_T)
    P, L = int(link_T.shape[0]), int(link_T.shape[1])
    i32, f64 = torch.int32, torch.float64
    box = Out(P * L, 6, f64)
    if entry in PAIR_ENTRIES:
        pairs = dev(np.asarray(ms.VALID if pairs is None else pairs, np.int32))
        M = len(pairs)
    else:
        pts_h, ps_h = ms.clouds() if cloud is None else cloud
        pts, pt_start, N = dev(pts_h), dev(ps_h), len(pts_h)
    if entry == "collide":
        need = lib.creg_mesh_collide_workspace_bytes(F, L, P, M)
        ws = workspace(need, fill)
        outs, shapes = [Out(P * M, 1, i32), Out(P * M, 2, i32)], [(P, M), (P, M, 2)]
        rc = lib.creg_mesh_collide_f64(ptr(tri), ptr(start), F, ptr(link_T), L, P, ptr(pairs), M, outs[0].ptr, outs[1].ptr, box.ptr,
                                       ptr(ws), need, None)
    elif entry == "clearance":
        need = lib.creg_mesh_clearance_workspace_bytes(F, L, P, M)
        ws = workspace(need, fill)
        outs, shapes = [Out(P * M, 1, f64), Out(P * M, 2, i32)], [(P, M), (P, M, 2)]
        rc = lib.creg_mesh_clearance_f64(ptr(tri), ptr(start), F, ptr(link_T), L, P, ptr(pairs), M, float(d_max), outs[0].ptr, outs[1].ptr,
                                         box.ptr, ptr(ws), need, None)
    elif entry == "contain":
        Q, pts, pt_start = ms.CONTAIN_Q, dev(g["pts"]), dev(g["pt_start"])
        need = lib.creg_mesh_contain_workspace_bytes(F, L, P, M, Q)
        ws = workspace(need, fill)
        outs, shapes = [Out(P * M, 2, i32), Out(P * M, 2, i32), Out(P * M, 2 * Q, f64)], [(P, M, 2), (P, M, 2), (P, M, 2, Q)]
        rc = lib.creg_mesh_contain_f64(ptr(tri), ptr(start), F, ptr(pts), ptr(pt_start), len(g["pts"]), ptr(link_T), L, P, ptr(pairs), M, Q,
                                       outs[0].ptr, outs[1].ptr, outs[2].ptr, box.ptr, ptr(ws), need, None)
    elif entry == "point_mesh":
        need = lib.creg_point_mesh_workspace_bytes(F, L, P, N)
        ws = workspace(need, fill)
        outs, shapes = [Out(N, 1, f64), Out(N, 1, i32)], [(N,), (N,)]
        rc = lib.creg_point_mesh_f64(ptr(tri), ptr(start), F, ptr(link_T), L, P, ptr(pts), ptr(pt_start), N, float(d_max), outs[0].ptr,
                                     outs[1].ptr, box.ptr, ptr(ws), need, None)
    else:
        need = lib.creg_mesh_cover_workspace_bytes(F, L, P, N)
        ws = workspace(need, fill)
        outs, shapes = [Out(P * F, 1, f64), Out(P * F, 1, i32), Out(P * F, 1, i32)], [(P, F)] * 3
        rc = lib.creg_mesh_cover_f64(ptr(tri), ptr(start), F, ptr(link_T), L, P, ptr(pts), ptr(pt_start), None, N, float(d_max), outs[0].ptr,
                                     outs[1].ptr, outs[2].ptr, box.ptr, ptr(ws), need, None)
    assert rc == 0, lib.creg_last_error()
    torch.cuda.synchronize()
    assert bool((ws[need // 8:] == NAN_WORD).all()), f"{entry}: written past the workspace's stated size"
    return tuple(o.take(s, n) for o, s, n in zip(outs + [box], shapes + [(P, L, 6)], NAMES[entry]))


def verify(entry, got, link_T, want, pairs=ms.VALID, d_max=ms.D_MAX, what=""):
    """The short call against the restatement ``want``, by the check and the bound of the entry's own test file."""
    g, _ = geometry(entry)
    if entry == "collide":
        check_collide(got, want)                                 # exact
    elif entry == "clearance":
        check_clearance(got, want, g["tri"], g["start"], link_T, pairs, d_max, what)
    elif entry == "contain":
        check_contain(got, (g["tri"], g["start"], g["pts"], g["pt_start"], link_T, pairs), ms.CONTAIN_Q, what)
    elif entry == "point_mesh":
        check_point_mesh(got, want, g["tri"], g["start"], link_T, *ms.clouds(), d_max, what)
    else:
        tol2 = 1e-12 * ms.cloud_diagonal() ** 2
        check_mesh_cover(got, want, mcref.ambiguous(g["tri"], g["start"], link_T, *ms.clouds(), d_max, tol2), tol2, what)


def restated(entry, d_max=ms.D_MAX, base=False):
    if entry == "collide":
        return ms.want_collide(base)
    if entry == "clearance":
        return ms.want_clearance(base)
    if entry == "contain":
        return ms.want_contain(base)
    return ms.want_point_mesh(d_max) if entry == "point_mesh" else ms.want_mesh_cover(d_max)


_SHORT = {}


def short(entry, d_max=ms.D_MAX):
    """The entry on its 7 templates (6 valid pairs, the templates' clouds), checked against the restatement: once per module."""
    if (entry, d_max) not in _SHORT:
        templates = geometry(entry)[1]
        got = run(entry, templates, d_max=d_max)
        verify(entry, got, templates, restated(entry, d_max), d_max=d_max, what=f"{entry}, 7 templates, d_max={d_max}")
        for a in got:
            a.setflags(write=False)
        _SHORT[entry, d_max] = got
    return _SHORT[entry, d_max]


def same_bits(entry, got, want, what):
    assert len(got) == len(want) == len(NAMES[entry])
    for name, g, w in zip(NAMES[entry], got, want):
        assert g.shape == w.shape and g.dtype == w.dtype, (name, g.shape, w.shape, g.dtype, w.dtype)
        if g.tobytes() != w.tobytes():
            gb, wb = (np.ascontiguousarray(x).reshape(len(x), -1).view(np.uint8) for x in (g, w))
            bad = np.flatnonzero((gb != wb).any(1))
            pytest.fail(f"{entry} {what}: {name} differs in {len(bad)} of {len(g)} rows, the first at {bad[:8].tolist()}")
    print(f"{entry} {what}: {len(got[0])} rows of {' / '.join(NAMES[entry])} compared, bits identical")


# ------------------------------------------------------------------------------------------ pose slices
@pytest.mark.parametrize("entry", ENTRIES)
def test_pose_slice(entry):
    """P = 65544 = 65535 + 9 poses, pose p a copy of template p % 7: pose 65535, the head of the second launch, is template 1, and
    the second launch holds every template.  Every row, link_box included, carries the bits of the 7-template call's row p % 7;
    mesh-cover's pt_idx is a row of pts and moves with its pose's first row."""
    P = ms.P_LONG
    templates = geometry(entry)[1]
    link_T = dev(ms.tiled_poses(P, templates))
    cloud = None
    if entry in ("point_mesh", "mesh_cover"):
        pts, pt_start, src = ms.tiled_cloud(P)
        cloud = (pts, pt_start)
    for d_max in (ms.D_MAX, INF) if entry == "point_mesh" else (ms.D_MAX,):
        few = short(entry, d_max)
        many = run(entry, link_T, cloud=cloud, d_max=d_max)
        if entry == "point_mesh":
            want = (few[0][src], few[1][src], ms.tiled(few[2], P))
        elif entry == "mesh_cover":
            first_row = ms.clouds()[1][:-1]                      # of each template's cloud, and of each long pose's copy of it
            idx = ms.tiled(few[1] - first_row[:, None].astype(np.int32), P) + pt_start[:-1, None].astype(np.int32)
            want = (ms.tiled(few[0], P), np.where(ms.tiled(few[1], P) >= 0, idx, -1).astype(np.int32), ms.tiled(few[2], P), ms.tiled(few[3], P))
        else:
            want = tuple(ms.tiled(a, P) for a in few)
        same_bits(entry, many, want, f"pose slice, d_max={d_max}")


# ------------------------------------------------------------------------------------------ pair slices
@pytest.mark.parametrize("entry", PAIR_ENTRIES)
def test_pair_slice(entry):
    """M = 65544 pairs, pair m a copy of base pair m % 11, on two templates whose answers differ: pair 65535 is base pair 8 and pair
    32767 base pair 9, so collide and clearance start their second launch, and contain its second and third, on another base pair
    than the first.  Invalid, same-link and empty-link entries give 0 / (-1,-1) / +inf / 0.0 in every launch."""
    M = ms.M_LONG
    templates = geometry(entry)[1]
    full = restated(entry, base=True)
    two = ms.differing_templates(full[2], ms.CONTAIN_SHIFTS) if entry == "contain" else ms.differing_templates(full[0])
    link_T = templates[two]
    few = run(entry, link_T, pairs=ms.BASE_PAIRS)
    verify(entry, few, link_T, tuple(a[two] for a in full), pairs=ms.BASE_PAIRS, what=f"{entry}, 11 base pairs")
    assert few[0][0].tobytes() != few[0][1].tobytes() or few[-2][0].tobytes() != few[-2][1].tobytes()    # the two templates differ on the device too
    many = run(entry, link_T, pairs=ms.tiled_pairs(M))
    col = np.arange(M) % len(ms.BASE_PAIRS)
    same_bits(entry, [np.ascontiguousarray(np.swapaxes(a, 0, 1)) for a in many[:-1]] + [many[-1]],
              [np.ascontiguousarray(np.swapaxes(a[:, col], 0, 1)) for a in few[:-1]] + [few[-1]], "pair slice")
    off = ms.NOT_EVALUATED[col]
    assert off.sum() >= 7 * (M // 11) and off[[ms.HALF_SLICE, ms.SLICE]].all() and off[ms.SLICE:].sum() == 6   # in every launch
    if entry == "collide":
        assert (many[0][:, off] == 0).all() and (many[1][:, off] == -1).all()
    elif entry == "clearance":
        assert np.isposinf(many[0][:, off]).all() and (many[1][:, off] == -1).all()
    else:
        assert (many[0][:, off] == 0).all() and (many[1][:, off] == -1).all() and (many[2][:, off] == 0.0).all()


# ------------------------------------------------------------------------------------------ stale workspace
@pytest.mark.parametrize("entry", PAIR_ENTRIES)
def test_dirty_workspace_changes_no_bit(entry):
    """The 7-template call on a zero-filled and on a NaN-pattern-filled workspace: the same bytes, so no slot -- clearance's
    per-block partials, contain's chunk partials behind its gate, collide's keys -- is read before the call wrote it."""
    clean = run(entry, geometry(entry)[1], fill="zero")
    same_bits(entry, clean, short(entry), "zero-filled against NaN-filled workspace")
    assert not any(np.isnan(a).any() for a in clean if a.dtype == np.float64)


# ------------------------------------------------------------------------------------------ clamped ends
@pytest.mark.parametrize("entry", ENTRIES)
def test_loose_ends_of_tri_start_are_clamped(entry):
    """tri_start[0] = -5 and tri_start[L] = F + 7 -- the last link is the empty one, so unclamped it would own seven rows past tri --
    and for contain pt_start[0] = -3, pt_start[L] = n_pts + 9 as well: every output carries the bytes of the call with the
    clamped table, and run() has checked that nothing past the outputs' and the workspace's stated sizes was written."""
    g, templates = geometry(entry, loose=True)
    assert g["start"][0] == -5 and g["start"][-1] == len(g["tri"]) + 7
    if entry == "contain":
        assert g["pt_start"][0] == -3 and g["pt_start"][-1] == len(g["pts"]) + 9
    for d_max in (ms.D_MAX, INF) if entry == "point_mesh" else (ms.D_MAX,):
        same_bits(entry, run(entry, templates, d_max=d_max, loose=True), short(entry, d_max), f"loose table ends, d_max={d_max}")
