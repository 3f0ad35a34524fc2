"""GPU: csrc/joints.hip (`k_link_clouds` through creg_link_clouds_f64 / ops.link_clouds and the coord_map / link /
compute_joints wrappers) across row slices, grid strides, cluster layouts and degenerate link poses -- the families of
tests/_link_clouds_ref.py.

Every output is compared with the float64 restatement of the kernel BIT FOR BIT, as integer views (any NaN counts as one
value: IEEE 754 leaves the sign and payload of an invalid operation's NaN to the implementation, and the host's differs from
the device's).  The x coordinate of every points row carries its row number, so a shifted, swapped, repeated or missing row
fails that comparison, and the message names the first wrong output row and its slice.  tests/test_link_clouds_cpu.py holds
the restatement to the reference's own results and to an extended-precision evaluation, and shows that its model of the
kernel's slice and stride loop notices the slips these cases are built for.

clouds_lf is held to the restatement's bits like everything else: on the MI355X it came out bit-identical in every case of
every family (no operation of the elimination or of the final dot product rounds differently on the device), so the GPU's
error against `lf_extended` is the restatement's own 1.9 / 1.4 / 1.7 / 1.3 eps (slice / stride / layout / pose).  The bound
at 4 x MEASURED_LF_EPS (eps64 units of |inv(Ml)_rot| (|w| + |t|)) is asserted as well; it is implied by the equality and is
there so that a run which ever loses a last bit still says by how much.

Deliberately wrong kernels (built from scratch copies, never committed) fail this file on the MI355X while
tests/test_gpu_joints.py and tests/test_gpu_urdf.py stay green: the source row taken as p0 + (dst - lo), `hi` clipped to
s1 - 1 at interior slice ends, and the stride removed so that only the first trip runs.  The plainer forms of the first two
(p0 + dst, kept in bounds; `hi` clipped to s1 - 1 everywhere) fail this file too, and were already caught by
test_cluster_to_link_vs_reference_golden.
"""
import os

import numpy as np
import pytest
import torch

import _link_clouds_ref as E

pytestmark = pytest.mark.gpu

GUARD = 64                                     # sentinel rows before and after the rows a launch may write
SENT32 = 0x7FC0DEAD
SENT64 = 0x7FF8DEAD7FC0DEAD
CREG_EINVAL = -1


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "GPU tests need the MI355X"
    from autourdf_amd import _lib
    _lib.load()
    return torch.device("cuda:0")


def _bits(a):
    """Integer view of a float array, every NaN as the one canonical quiet NaN."""
    a = np.ascontiguousarray(a)
    if a.dtype == np.float32:
        return np.where(np.isnan(a), np.int32(0x7FC00000), a.view(np.int32))
    assert a.dtype == np.float64
    return np.where(np.isnan(a), np.int64(0x7FF8000000000000), a.view(np.int64))


def _same_rows(label, name, got, ref, oo, rows=E.LC_ROWS):
    """Bit equality of an (M,3) cloud; the failure names the first wrong output row, its (frame, link) block and its slice."""
    assert got.shape == ref.shape, (label, name, got.shape, ref.shape)
    bad = np.nonzero((_bits(got) != _bits(ref)).any(axis=1))[0]
    if len(bad):
        r = int(bad[0])
        b = int(np.searchsorted(oo, r, side="right") - 1)
        raise AssertionError(f"{label}: {name} differs in {len(bad)} of {len(ref)} rows; first at output row {r} = row "
                             f"{r - int(oo[b])} of block {b} (slice {(r - int(oo[b])) // rows}): got {got[r]}, want {ref[r]}")


def _same_matrices(label, name, got, ref):
    assert got.dtype == np.float32 and got.shape == ref.shape, (label, name, got.dtype, got.shape)
    bad = np.nonzero((_bits(got) != _bits(ref)).reshape(-1, 16).any(axis=1))[0]
    assert len(bad) == 0, (label, name, "blocks", bad[:8].tolist(), got.reshape(-1, 4, 4)[bad[0]], ref.reshape(-1, 4, 4)[bad[0]])


def _gpu(dev, case, mean_matrices=True):
    from autourdf_amd import ops
    _, coords, matrices, links, points, po = case
    lm, mm, wf, lf, oo = ops.link_clouds(torch.from_numpy(coords).to(dev), torch.from_numpy(matrices).to(dev), links,
                                         torch.from_numpy(points).to(dev), po, mean_matrices=mean_matrices)
    torch.cuda.synchronize()
    return lm.cpu().numpy(), None if mm is None else mm.cpu().numpy(), wf.cpu().numpy(), lf.cpu().numpy(), oo


def _check_against_restatement(label, got, ref):
    (lm, mm, wf, lf, oo), (rlm, rmm, rwf, rlf, roo) = got, ref
    assert isinstance(oo, np.ndarray) and oo.dtype == np.int64 and (oo == roo).all(), label
    _same_matrices(label, "link_matrices", lm, rlm)
    _same_matrices(label, "mean_matrices", mm, rmm)
    _same_rows(label, "clouds_wf", wf, rwf, roo)
    _same_rows(label, "clouds_lf", lf, rlf, roo)


@pytest.mark.parametrize("family", ["slice", "stride", "layout", "pose"])
def test_every_output_is_the_restatements_bit_for_bit(dev, family):
    """ops.link_clouds(..., mean_matrices=True) on every case of the family: link_matrices, mean_matrices, clouds_wf, clouds_lf
    and out_offsets equal to the restatement's, bit for bit; the GPU's clouds_lf error against lf_extended is printed in the
    units of MEASURED_LF_EPS and held to 4 x the family's figure."""
    worst, n_cases, raw_nan = 0.0, 0, True
    for case in E.FAMILIES[family]():
        label, links = case[0], case[3]
        ref = E.link_clouds_ref(*case[1:])
        got = _gpu(dev, case)
        ext, unit = E.lf_extended(ref[0], ref[2], links, ref[4])
        e = E.lf_error_eps(got[3], ext, unit) if got[3].shape == ext.shape else float("nan")
        print(f"{label:32s} rows {len(ref[3]):7d}  clouds_lf on the GPU {e:5.2f} eps, "
              f"{int((_bits(got[3]) != _bits(ref[3])).sum()) if got[3].shape == ref[3].shape else -1} elements off the restatement")
        worst = max(worst, e)
        _check_against_restatement(label, got, ref)
        n_cases += 1
    print(f"{family:8s} clouds_lf on the GPU: worst {worst:.2f} eps, fallback bound {E.gpu_lf_bound(family)} eps")
    assert worst <= E.gpu_lf_bound(family)
    assert n_cases == {"slice": 5, "stride": 1, "layout": 5, "pose": 7}[family]


def test_antipodal_quaternions_poison_their_own_link_only(dev):
    """include/creg.h: a link whose cluster quaternions sum to exactly zero has a NaN rotation block in link_matrices (its
    translation and last row stay finite) and NaN rows in clouds_lf; its clouds_wf and mean_matrices, and every output of every
    other (frame, link) of the launch, are what they are without it."""
    case = E.first_case("antipodal", "two_links")
    label, coords, matrices, links, points, po = case
    T, L = coords.shape[0], len(links)
    ref = E.link_clouds_ref(*case[1:])
    lm, mm, wf, lf, oo = got = _gpu(dev, case)
    _check_against_restatement(label, got, ref)
    mine = np.zeros(len(lf), bool)
    for t, l in E.ANTIPODAL_BLOCKS:
        assert np.isnan(lm[t, l, :3, :3]).all() and np.isfinite(lm[t, l, :3, 3]).all() and (lm[t, l, 3] == [0, 0, 0, 1]).all()
        assert oo[t * L + l + 1] > oo[t * L + l]
        mine[oo[t * L + l]:oo[t * L + l + 1]] = True
    assert np.isnan(lf[mine]).all() and np.isfinite(lf[~mine]).all() and np.isfinite(wf).all() and np.isfinite(mm).all()
    # the same launch with the cancelling partner turned away: every other block is bit for bit what it was
    healthy = coords.copy()
    for t, l in E.ANTIPODAL_BLOCKS:
        healthy[t, links[l][1], 3:] = healthy[t, links[l][1], [4, 3, 6, 5]] * [1, -1, 1, -1]
    lm2, mm2, wf2, lf2, oo2 = _gpu(dev, (label, healthy, matrices, links, points, po))
    others = [b for b in range(T * L) if divmod(b, L) not in E.ANTIPODAL_BLOCKS]
    assert np.isfinite(lm2).all() and np.isfinite(lf2).all() and (oo2 == oo).all()
    assert (_bits(lm2).reshape(-1, 16)[others] == _bits(lm).reshape(-1, 16)[others]).all()
    assert (_bits(mm2).reshape(-1, 16)[others] == _bits(mm).reshape(-1, 16)[others]).all()
    assert (_bits(wf2) == _bits(wf)).all() and (_bits(lf2)[~mine] == _bits(lf)[~mine]).all()


# ------------------------------------------------------------------------------------------ the C ABI, directly
def _guarded(dev, rows, cols, dtype):
    buf = torch.empty((rows + 2 * GUARD, cols), dtype=dtype, device=dev)
    if dtype == torch.float32:
        buf.view(torch.int32).fill_(SENT32)
    else:
        buf.view(torch.int64).fill_(SENT64)
    return buf


def _raw(buf):
    raw = buf.cpu().numpy()
    return (raw.view(np.int64), SENT64) if raw.dtype == np.float64 else (raw.view(np.int32), SENT32)


def _guards_intact(buf, rows):
    raw, sent = _raw(buf)
    return bool((raw[:GUARD] == sent).all() and (raw[GUARD + rows:] == sent).all())


def _all_written(buf, rows):
    raw, sent = _raw(buf)
    return bool((raw[GUARD:GUARD + rows] != sent).all())


def _inner(buf, rows):
    return buf[GUARD:GUARD + rows].cpu().numpy()


class _Direct:
    """One ctypes call of creg_link_clouds_f64 with all four outputs as interior views of sentinel-filled buffers.  Keyword
    arguments override what the launch is told (T, K, L, max_link_rows, ...), never the buffers behind it."""

    def __init__(self, dev, case, mean=True, null_points=False, null_clouds=False, null_link_matrices=False, **tell):
        from autourdf_amd import _lib, ops
        lib = _lib.load()
        _, coords, matrices, links, points, po = case
        T, K = coords.shape[:2]
        L = len(links)
        flat = [k for l in links for k in l]
        off = np.concatenate([[0], np.cumsum([len(l) for l in links])])
        oo = E.out_offsets_of(links, po, T, K)
        self.T, self.L, self.oo, self.n_out = T, L, oo, int(oo[-1])
        self.true_max = int(np.diff(oo).max())
        t = lambda a, dt: torch.from_numpy(np.ascontiguousarray(np.asarray(a, dt))).to(dev)
        self.keep = (t(coords, np.float64), t(matrices, np.float64), t(flat, np.int32), t(off, np.int32),
                     t(points, np.float64), t(po, np.int64), t(oo, np.int64))
        c, m, cl, lo, pts, po_d, oo_d = self.keep
        self.lm, self.mm = _guarded(dev, T * L, 16, torch.float32), _guarded(dev, T * L, 16, torch.float32)
        self.wf, self.lf = _guarded(dev, self.n_out, 3, torch.float64), _guarded(dev, self.n_out, 3, torch.float64)
        a = dict(T=T, K=K, n_cl=len(flat), L=L, n_points=len(points), n_out=self.n_out, max_link_rows=self.true_max)
        a.update(tell)
        if null_points:
            assert a["n_points"] == 0
        if null_clouds:
            assert a["n_out"] == 0
        self.rc = lib.creg_link_clouds_f64(
            ops._p(c), ops._p(m), a["T"], a["K"], ops._p(cl), ops._p(lo), a["n_cl"], a["L"],
            None if null_points else ops._p(pts), ops._p(po_d), a["n_points"], ops._p(oo_d), a["n_out"], a["max_link_rows"],
            None if null_link_matrices else ops._p(self.lm[GUARD:]), ops._p(self.mm[GUARD:]) if mean else None,
            None if null_clouds else ops._p(self.wf[GUARD:]), None if null_clouds else ops._p(self.lf[GUARD:]), ops._stream())
        torch.cuda.synchronize()
        self.error = lib.creg_last_error()

    def outputs(self):
        return (_inner(self.lm, self.T * self.L), _inner(self.mm, self.T * self.L), _inner(self.wf, self.n_out),
                _inner(self.lf, self.n_out))

    def untouched(self):
        return all(_guards_intact(b, 0) for b in (self.lm, self.mm, self.wf, self.lf))


def _same_outputs(label, a, b, skip=()):
    for i, name in enumerate(("link_matrices", "mean_matrices", "clouds_wf", "clouds_lf")):
        if name not in skip:
            assert (_bits(a[i]) == _bits(b[i])).all(), (label, name)


@pytest.mark.parametrize("which", ["slice/boundaries", "slice/totals", "stride/big", "layout/repeated_shared_unused"])
def test_every_row_is_written_and_nothing_outside(dev, which):
    """The four outputs as interior views of sentinel-filled buffers: the guards in front and behind stay intact, no sentinel
    is left inside, and the bits are the restatement's."""
    case = E.first_case(*which.split("/"))
    d = _Direct(dev, case)
    assert d.rc == 0, d.error
    for buf, rows in ((d.lm, d.T * d.L), (d.mm, d.T * d.L), (d.wf, d.n_out), (d.lf, d.n_out)):
        assert _guards_intact(buf, rows), which
        assert _all_written(buf, rows), which
    lm, mm, wf, lf = d.outputs()
    rlm, rmm, rwf, rlf, roo = E.link_clouds_ref(*case[1:])
    _same_matrices(which, "link_matrices", lm.reshape(rlm.shape), rlm)
    _same_matrices(which, "mean_matrices", mm.reshape(rmm.shape), rmm)
    _same_rows(which, "clouds_wf", wf, rwf, roo)
    _same_rows(which, "clouds_lf", lf, rlf, roo)


def test_max_link_rows_costs_speed_never_rows(dev):
    """include/creg.h: max_link_rows only sizes grid.y.  0, 1, 1024, the true maximum - 1, the true maximum and ten times it
    give identical bits in every output, on every case of the slice family."""
    for case in E.slice_cases():
        base = _Direct(dev, case)
        assert base.rc == 0, base.error
        want = base.outputs()
        _same_rows(case[0], "clouds_lf", want[3], E.link_clouds_ref(*case[1:])[3], base.oo)
        for mlr in (0, 1, 1024, base.true_max - 1, base.true_max, 10 * base.true_max):
            d = _Direct(dev, case, max_link_rows=mlr)
            assert d.rc == 0, d.error
            assert all(_guards_intact(b, r) for b, r in ((d.lm, d.T * d.L), (d.mm, d.T * d.L), (d.wf, d.n_out), (d.lf, d.n_out)))
            _same_rows(f"{case[0]} max_link_rows={mlr}", "clouds_wf", d.outputs()[2], want[2], base.oo)
            _same_outputs((case[0], mlr), d.outputs(), want)


def test_null_mean_matrices_and_null_points(dev):
    """mean_matrices = NULL leaves the other three outputs as they are and the buffer it was not given alone; points = NULL
    with n_points = 0 and n_out = 0 writes both matrix outputs and nothing else (with and without cloud pointers)."""
    case = E.first_case("slice", "span")
    with_mm, without = _Direct(dev, case), _Direct(dev, case, mean=False)
    assert with_mm.rc == 0 and without.rc == 0, (with_mm.error, without.error)
    _same_outputs(case[0], with_mm.outputs(), without.outputs(), skip=("mean_matrices",))
    assert _guards_intact(without.mm, 0)
    case = E.first_case("layout", "no_points")
    rlm, rmm, _, _, roo = E.link_clouds_ref(*case[1:])
    assert roo[-1] == 0
    for null_clouds in (False, True):
        d = _Direct(dev, case, null_points=True, null_clouds=null_clouds)
        assert d.rc == 0, d.error
        lm, mm, _, _ = d.outputs()
        _same_matrices(case[0], "link_matrices", lm.reshape(rlm.shape), rlm)
        _same_matrices(case[0], "mean_matrices", mm.reshape(rmm.shape), rmm)
        assert _guards_intact(d.lm, d.T * d.L) and _guards_intact(d.mm, d.T * d.L)
        assert _guards_intact(d.wf, 0) and _guards_intact(d.lf, 0)


@pytest.mark.parametrize("what", ["T=0", "K=257", "L>K", "max_link_rows<0", "null_link_matrices"])
def test_refusals_return_einval_and_launch_nothing(dev, what):
    """T < 1, K > 256, L > K, max_link_rows < 0 and a null link_matrices: CREG_EINVAL, creg_last_error() set, nothing launched
    (the sentinel buffers are untouched)."""
    case = E.first_case("layout", "unused_T1")
    K = case[1].shape[1]
    kw = {"T=0": dict(T=0), "K=257": dict(K=257), "L>K": dict(L=K + 1), "max_link_rows<0": dict(max_link_rows=-1),
          "null_link_matrices": dict(null_link_matrices=True)}[what]
    d = _Direct(dev, case, **kw)
    assert d.rc == CREG_EINVAL
    assert d.error.startswith(b"creg_link_clouds_f64: "), d.error
    assert d.untouched()
    ok = _Direct(dev, case)                                       # the same buffers and tables are fine when told the truth
    assert ok.rc == 0 and not ok.untouched()


def test_wrapper_raises_value_error_before_any_launch(dev):
    from autourdf_amd import ops
    _, coords, matrices, links, points, po = E.first_case("layout", "unused_T1")
    T, K = coords.shape[:2]
    c, m, p = (torch.from_numpy(a).to(dev) for a in (coords, matrices, points))
    dec = po.copy()
    dec[3] = dec[2] - 1
    short_end = po.copy()
    short_end[-1] -= 1
    big = torch.zeros(1, 257, 7, dtype=torch.float64, device=dev)
    big[..., 3] = 1.0
    for args in ((c, m, links, p, po[:-1]),                                    # point_offsets of the wrong length
                 (c, m, links, p, np.concatenate([po, po[-1:]])),
                 (c, m, links, p, dec),                                        # decreasing
                 (c, m, links, p, short_end),                                  # not ending at len(points)
                 (c, m, links, p[:-1], po),
                 (big, torch.eye(4, dtype=torch.float64, device=dev).repeat(1, 257, 1, 1), [[0]], p[:0], np.zeros(258, np.int64)),
                 (c, m, [links[0], []], p, po),                                # an empty link
                 (c, m, [links[0], [K]], p, po),                               # a cluster outside [0, K)
                 (c, m, [links[0], [-1]], p, po),
                 (c, m[:, :-1], links, p, po),                                 # matrices that do not match coords
                 (c, m[..., :3, :], links, p, po)):
        with pytest.raises(ValueError):
            ops.link_clouds(*args, mean_matrices=True)
    ops.link_clouds(c, m, links, p, po, mean_matrices=True)                    # (the unharmed call goes through)


# ------------------------------------------------------------------------------------------ the wrappers, at a size that slices
WRAP_LINKS = [[7, 2, 9, 0], [11, 4, 1], [3, 10, 6, 5]]           # set order; cluster 8 is in no link


def _wrap_case():
    sizes = np.random.default_rng(600).integers(700, 901, size=(4, 12))
    return E._case("wrap/T4_K12", sizes, WRAP_LINKS, 601)


def _coord_map(case):
    from autourdf_amd.coord_map import CoordMap
    _, coords, matrices, _, points, po = case
    T, K = coords.shape[:2]
    cm = CoordMap.__new__(CoordMap)
    cm.coords, cm.matrices = coords, matrices
    cm._M = torch.from_numpy(matrices).cuda().contiguous()
    cm.clusters = [{str(k): points[po[t * K + k]:po[t * K + k + 1]] for k in range(K)} for t in range(T)]
    return cm


def test_cluster_to_link_at_a_size_that_slices(dev):
    case = _wrap_case()
    rlm, _, rwf, rlf, oo = E.link_clouds_ref(*case[1:])
    T, L = rlm.shape[:2]
    assert np.diff(oo).min() > 2 * E.LC_ROWS
    got = _coord_map(case).cluster_to_link(WRAP_LINKS)
    assert len(got) == L
    for l, ml in enumerate(got):
        _same_matrices(case[0], f"link {l} matrices", ml["matrices"], rlm[:, l])
        assert len(ml["clusters"]) == T and len(ml["clusters_wf"]) == T
        for t in range(T):
            blk = slice(oo[t * L + l], oo[t * L + l + 1])
            _same_rows(f"{case[0]} link {l} frame {t}", "clusters_wf", ml["clusters_wf"][t], rwf[blk], [0])
            _same_rows(f"{case[0]} link {l} frame {t}", "clusters", ml["clusters"][t], rlf[blk], [0])


def test_save_links_writes_the_restatements_arrays(dev, tmp_path):
    from autourdf_amd import link
    case = _wrap_case()
    rlm, _, rwf, rlf, oo = E.link_clouds_ref(*case[1:])
    T, L = rlm.shape[:2]
    d = str(tmp_path / "seq0") + "/"
    link.save_links([_coord_map(case)], WRAP_LINKS, [d], 0, T)
    for sub, ext in (("matrix", ".npy"), ("cluster", ".npz"), ("cluster_wf", ".npz")):
        assert sorted(os.listdir(d + sub)) == [f"{t:04}{ext}" for t in range(T)]
    for t in range(T):
        m = np.load(d + f"matrix/{t:04}.npy")
        assert m.dtype == np.float32 and m.shape == (L, 4, 4)
        _same_matrices(case[0], f"matrix/{t:04}.npy", m, rlm[t])
        for sub, ref in (("cluster", rlf), ("cluster_wf", rwf)):
            with np.load(d + f"{sub}/{t:04}.npz") as z:
                assert list(z.keys()) == [str(i) for i in range(L)]
                for l in range(L):
                    a = z[str(l)]
                    assert a.dtype == np.float64
                    _same_rows(f"{case[0]} {sub}/{t:04}.npz[{l}]", sub, a, ref[oo[t * L + l]:oo[t * L + l + 1]], [0])


@pytest.mark.parametrize("time_step", [0, 3])
def test_link_transforms_are_the_restatements_mean_matrices(dev, time_step):
    from autourdf_amd import compute_joints
    case = _wrap_case()
    _, rmm, _, _, _ = E.link_clouds_ref(*case[1:])
    links = [{"id": 10 + i, "cluster_idx": set(c) if i == 1 else c} for i, c in enumerate(WRAP_LINKS)]
    order = [list(l["cluster_idx"]) for l in links]                # a set hands its clusters over in its own order
    if order != WRAP_LINKS:
        _, rmm, _, _, _ = E.link_clouds_ref(case[1], case[2], order, case[4], case[5])
    got = compute_joints.link_transforms(links, _coord_map(case), time_step)
    assert list(got) == [10, 11, 12]
    for i in range(3):
        _same_matrices(case[0], f"link_transforms[{10 + i}] at {time_step}", got[10 + i], rmm[time_step, i])
