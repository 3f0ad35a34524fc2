"""GPU: csrc/normals.hip (`k_knn_normals` through creg_knn_normals_f64 / ops.knn_normals) at distance ties, list edges and
degenerate fits -- the families of tests/_normals_edges.py.

Lists are compared with oracle.normals.hybrid_neighbours element for element (the build uses -ffp-contract=off, so the kernel's
squared distances are numpy's bit for bit; tests/test_normals_edges_cpu.py checks the oracle on the tie-heavy inputs).  Normals
are checked on EVERY point with three or more neighbours: unit length, and the Rayleigh excess (n^T C n - l0) / lmax against the
covariance of the returned list in extended precision, within `_normals_edges.gpu_bound(family)` -- 16 x what the float64
restatement of the solver itself measures against eigh (never anything measured from the kernel), floor 64 x 2^-52.  Only
neighbourhoods made of one repeated point are exempt from the excess (their covariance is 0: every unit vector is right).
"""
import numpy as np
import pytest
import torch

import _normals_edges as E

pytestmark = pytest.mark.gpu

GUARD = 64                                     # sentinel rows before and after the n rows a launch may write
SENT32 = 0x7FC0DEAD
SENT64 = 0x7FF8DEAD7FC0DEAD


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "GPU tests need the MI355X"
    from autourdf_amd import _lib
    _lib.load()
    return torch.device("cuda:0")


def _three_ways(X, radius, max_nn):
    """The three output combinations the ABI allows (cnt always): results must not depend on which are asked for."""
    from autourdf_amd import ops
    n_only, none_idx, c0 = ops.knn_normals(X, radius, max_nn, want_normals=True, want_idx=False)
    none_n, i_only, c1 = ops.knn_normals(X, radius, max_nn, want_normals=False, want_idx=True)
    nrm, idx, c2 = ops.knn_normals(X, radius, max_nn, want_normals=True, want_idx=True)
    assert none_idx is None and none_n is None
    nrm, idx, cnt = nrm.cpu().numpy(), idx.cpu().numpy(), c2.cpu().numpy()
    assert (c0.cpu().numpy() == cnt).all() and (c1.cpu().numpy() == cnt).all()
    assert (i_only.cpu().numpy() == idx).all()
    assert (n_only.cpu().numpy().view(np.int64) == nrm.view(np.int64)).all()
    return nrm, idx, cnt


def _check_case(dev, label, P, radius, max_nn, worst):
    from oracle import normals as onrm
    nrm, idx, cnt = _three_ways(torch.from_numpy(P).to(dev), radius, max_nn)
    ref_idx, ref_cnt = E.pad_lists(onrm.hybrid_neighbours(P, radius, max_nn), max_nn)
    # lists, exactly
    assert idx.shape == (len(P), max_nn) and (cnt == ref_cnt).all(), label
    assert (idx == ref_idx).all(), (label, np.nonzero((idx != ref_idx).any(1))[0][:5])       # (-1 past the count on both sides)
    # fewer than three neighbours
    few = cnt < 3
    assert (nrm[few] == [0.0, 0.0, 1.0]).all(), label
    if radius == E.TINY_RADIUS and "size" in label:
        assert (cnt == 1).all() and (idx[:, 0] == np.arange(len(P))).all(), label
    if max_nn < 3 or len(P) < 3:
        assert few.all(), label
    # normals, every point
    assert np.isfinite(nrm).all(), label
    assert (np.abs(np.linalg.norm(nrm, axis=1) - 1) <= 1e-12).all(), label
    fam = E.family_of(label)
    if not few.all():
        excess, identical = E.rayleigh_excess(P, idx.astype(np.int64), cnt.astype(np.int64), nrm)
        use = ~few & ~identical
        if fam == "identical":
            assert identical.all(), label
        elif fam not in ("duplicate", "tie", "size"):
            assert not identical.any(), label
        if use.any():
            worst[fam] = max(worst.get(fam, 0.0), float(excess[use].max()))
            bad = use & ~(excess <= E.gpu_bound(fam))
            assert not bad.any(), (label, int(bad.sum()), float(excess[use].max()), E.gpu_bound(fam))
        if fam in E.DIAGONAL_FAMILIES:
            want = E.diagonal_expected(P, idx.astype(np.int64), cnt.astype(np.int64))
            assert (nrm == want).all(), (label, np.nonzero((nrm != want).any(1))[0][:5])
    return nrm, idx, cnt


@pytest.mark.parametrize("group", ["size", "tie", "duplicate", "island"])
def test_lists_exact_and_every_normal_within_its_bound(dev, group):
    """Per case: cnt and idx equal to the oracle's lists element for element (ties by index, nothing at d^2 == r^2, -1 past the
    count), identical through the three output combinations; (0,0,1) below three neighbours; every other normal finite, unit
    to 1e-12 and within the family's Rayleigh bound; the exact axis for exactly diagonal covariances."""
    cases = {"size": E.size_cases, "tie": E.tie_cases, "duplicate": E.duplicate_cases, "island": E.island_cases}[group]
    worst, n_cases = {}, 0
    for label, P, radius, max_nn in cases():
        _check_case(dev, label, P, radius, max_nn, worst)
        n_cases += 1
    for fam, w in sorted(worst.items()):
        print(f"{fam:14s} largest excess on the GPU {w:.3e}  bound {E.gpu_bound(fam):.2e}")
    assert n_cases == {"size": len(E.SIZES) * 15, "tie": 30, "duplicate": 7, "island": 16}[group]


def test_duplicates_lists_may_leave_the_query_out(dev):
    """More copies than max_nn: the lowest-indexed copies fill the list, so later copies do not find themselves (the host's
    orientation pass filters `dst != src` and relies on the list being right, not on position 0 being the query)."""
    from autourdf_amd import ops
    label, P, radius, max_nn = next(c for c in E.duplicate_cases() if c[3] == 30 and c[2] < 0)
    _, idx, cnt = ops.knn_normals(torch.from_numpy(P).to(dev), radius, max_nn, want_normals=False, want_idx=True)
    idx = idx.cpu().numpy()
    out = [i for i in range(len(P)) if i not in idx[i]]
    assert len(out) >= 8 * 1 + 8 * 10
    for i in out:
        assert (idx[i] == np.nonzero((P == P[i]).all(1))[0][:max_nn]).all()


def _guarded(dev, rows, cols, dtype):
    buf = torch.empty((rows + 2 * GUARD, cols), dtype=dtype, device=dev)
    if dtype == torch.int32:
        buf.fill_(SENT32)
    else:
        buf.view(torch.int64).fill_(SENT64)
    return buf


def _guards_intact(buf, rows):
    raw = buf.cpu().numpy()
    raw = raw.view(np.int64) if raw.dtype == np.float64 else raw
    sent = SENT64 if raw.dtype == np.int64 else SENT32
    return bool((raw[:GUARD] == sent).all() and (raw[GUARD + rows:] == sent).all())


def _direct(dev, P, radius, max_nn):
    """One ctypes call with idx_out / cnt_out / normals as interior views of sentinel-filled buffers."""
    from autourdf_amd import _lib, ops
    L = _lib.load()
    n = len(P)
    X = torch.from_numpy(np.ascontiguousarray(P)).to(dev)
    bi, bc, bn = _guarded(dev, n, max_nn, torch.int32), _guarded(dev, n, 1, torch.int32), _guarded(dev, n, 3, torch.float64)
    # idx rows are max_nn wide in the ABI: GUARD * max_nn elements in front is a whole number of buffer rows
    rc = L.creg_knn_normals_f64(ops._p(X), n, float(radius), int(max_nn), ops._p(bi[GUARD:]), ops._p(bc[GUARD:]),
                                ops._p(bn[GUARD:]), ops._stream())
    torch.cuda.synchronize()
    return rc, bi, bc, bn


@pytest.mark.parametrize("group", ["size", "tie", "duplicate", "island"])
def test_nothing_written_outside_the_outputs(dev, group):
    from autourdf_amd import _lib, ops
    label, P, radius, max_nn = {
        "size": lambda: next(c for c in E.size_cases((129,)) if c[3] == 30 and c[2] == 0.1),
        "tie": lambda: next(c for c in E.tie_cases() if "8x8x8_k12_r0.25" in c[0]),          # n = 512: no dead thread, a full tile
        "duplicate": lambda: next(iter(E.duplicate_cases())),
        "island": lambda: next(c for c in E.island_cases() if c[0].startswith("octahedron")),
    }[group]()
    n = len(P)
    rc, bi, bc, bn = _direct(dev, P, radius, max_nn)
    _lib.check(rc, "creg_knn_normals_f64")
    assert _guards_intact(bi, n) and _guards_intact(bc, n) and _guards_intact(bn, n), label
    nrm, idx, cnt = ops.knn_normals(torch.from_numpy(P).to(dev), radius, max_nn, want_normals=True, want_idx=True)
    assert torch.equal(bi[GUARD:GUARD + n], idx) and torch.equal(bc[GUARD:GUARD + n, 0], cnt), label
    assert torch.equal(bn[GUARD:GUARD + n].view(torch.int64), nrm.view(torch.int64)), label


@pytest.mark.parametrize("what", ["max_nn_0", "max_nn_33", "empty_cloud"])
def test_refusals_raise_and_launch_nothing(dev, what):
    """include/creg.h: n < 1, max_nn < 1, max_nn > 32 return CREG_EINVAL with creg_last_error() set and launch nothing; the
    wrapper raises RuntimeError carrying that text."""
    from autourdf_amd import _lib, ops
    P = E.size_cloud(33) if what != "empty_cloud" else np.zeros((0, 3))
    max_nn = {"max_nn_0": 0, "max_nn_33": 33, "empty_cloud": 30}[what]
    with pytest.raises(RuntimeError, match=r"creg_knn_normals_f64: needs 1 <= n < 2\^31 and 1 <= max_nn <= 32"):
        ops.knn_normals(torch.from_numpy(P).to(dev), 0.1, max_nn, want_normals=True, want_idx=True)
    rows = 33
    bi, bc, bn = _guarded(dev, rows, 33, torch.int32), _guarded(dev, rows, 1, torch.int32), _guarded(dev, rows, 3, torch.float64)
    X = torch.from_numpy(E.size_cloud(33)).to(dev)
    rc = _lib.load().creg_knn_normals_f64(ops._p(X), len(P), 0.1, max_nn, ops._p(bi[GUARD:]), ops._p(bc[GUARD:]), ops._p(bn[GUARD:]),
                                          ops._stream())
    torch.cuda.synchronize()
    assert rc != 0 and b"creg_knn_normals_f64: needs" in _lib.load().creg_last_error()
    for b in (bi, bc, bn):                                       # nothing ran: the outputs themselves still hold the sentinel
        assert _guards_intact(b, 0)


def test_orientation_against_geometry(dev):
    """A closed convex surface has a known answer: after orient_normals_consistent_tangent_plane EVERY normal points outward
    (the oracle's walk achieves 100 % too, tests/test_normals_edges_cpu.py), and is no further from the analytic normal than
    the oracle's worst point (minus 1e-9)."""
    from autourdf_amd import normals as gn
    from oracle import normals as onrm
    for name, P, outward in E.surface_cases():
        feat, N = gn.point_features(P)
        _, oN = onrm.point_features(P)
        cos, ocos = (N * outward).sum(1), (oN * outward).sum(1)
        print(name, "outward", (cos > 0).mean(), "smallest cosine", cos.min(), "oracle", ocos.min())
        assert (ocos > 0).all()
        assert (cos > 0).all(), (name, (cos > 0).mean())
        assert cos.min() >= ocos.min() - 1e-9, (name, cos.min(), ocos.min())
        np.testing.assert_array_equal(feat[:, :3], P)
        np.testing.assert_array_equal(feat[:, 3:], 0.5 * N)


@pytest.mark.parametrize("n", [1, 2, 3, 4])
def test_orientation_of_fewer_than_five_points_returns_its_input(dev, n):
    """No Delaunay tetrahedralisation exists below five points (open3d raises there); the input comes back as it is."""
    from autourdf_amd import normals as gn
    rng = np.random.default_rng(n)
    P, N = 0.01 * rng.normal(size=(n, 3)), rng.normal(size=(n, 3))          # all within the radius of one another
    N /= np.linalg.norm(N, axis=1, keepdims=True)
    out = gn.orient_normals_consistent_tangent_plane(P, N)
    assert out is not N and (out == N).all()
    feat, fN = gn.point_features(P)
    assert (fN == gn.estimate_normals(P)).all() and (feat == np.hstack([P, 0.5 * fN])).all()
    if n < 3:
        assert (fN == [0.0, 0.0, 1.0]).all()
    else:
        assert (np.abs(np.linalg.norm(fN, axis=1) - 1) <= 1e-12).all()
