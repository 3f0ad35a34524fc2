"""CPU: the restatement of csrc/joints.hip's `k_link_clouds` in tests/_link_clouds_ref.py reproduces the reference's own
results, is measured against an extended-precision evaluation (the figures the GPU fallback bound of
tests/test_gpu_link_clouds.py hangs on), the case families reach the slices, strides, layouts and pivots they are built for, and
a pure-Python walk of the kernel's slice and stride loop visits every output row exactly once from the right source row."""
import functools
import os
import re

import numpy as np
import pytest

import _link_clouds_ref as E

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@functools.lru_cache(maxsize=None)
def _restated(family):
    """Every case of a family through the restatement: [(case, (lm, mm, wf, lf, oo))] and the row swaps inv4 took."""
    swaps, out = set(), []
    for case in E.FAMILIES[family]():
        out.append((case, E.link_clouds_ref(*case[1:], swaps=swaps)))
    return out, swaps


def test_kernel_constants_are_the_helpers():
    src = open(os.path.join(ROOT, "autourdf_amd", "csrc", "joints.hip")).read()
    nt = int(re.search(r"constexpr int LC_NT = (\d+);", src).group(1))
    mult = int(re.search(r"constexpr int LC_ROWS = (\d+) \* LC_NT;", src).group(1))
    slices = int(re.search(r"constexpr int LC_MAX_SLICES = (\d+);", src).group(1))
    hdr = open(os.path.join(ROOT, "autourdf_amd", "csrc", "joints_dev.h")).read()       # the joint stage's one set of limits
    max_k = int(re.search(r"constexpr int JOINT_MAX_K = (\d+);", hdr).group(1))
    assert "K <= JOINT_MAX_K" in src[src.index('extern "C" int creg_link_clouds_f64('):]
    assert (nt, mult * nt, slices, max_k) == (E.LC_NT, E.LC_ROWS, E.LC_MAX_SLICES, E.MAX_K)
    assert E.STRIDE_ROWS == slices * mult * nt + mult * nt + 5


def test_restatement_vs_reference_golden(golden):
    """Case `a` of joints_reference.npz (minted by the reference): link matrices and world-frame clouds bit for bit, link-frame
    clouds within the 1e-6 of test_cluster_to_link_vs_reference_golden (the reference inverts in float32)."""
    g, u = golden("joints_reference.npz"), golden("urdf_reference.npz")
    T, K = g["a.c2l_point_sizes"].shape
    links = [[int(x) for x in c] for c in np.split(g["a.c2l_cluster_idx"], np.cumsum(g["a.c2l_cluster_sizes"])[:-1])]
    po = np.concatenate([[0], np.cumsum(g["a.c2l_point_sizes"].reshape(-1))])
    lm, _, wf, lf, oo = E.link_clouds_ref(g["a.coords"][0], u["a.matrices"][0], links, g["a.c2l_points"].astype(np.float64), po)
    L = len(links)
    assert (lm.transpose(1, 0, 2, 3).view(np.int32) == g["a.c2l_matrices"].view(np.int32)).all()
    order = [b for l in range(L) for b in range(l, T * L, L)]                # the fixture is link-major, the kernel frame-major
    rows = np.concatenate([np.arange(oo[b], oo[b + 1]) for b in order])
    assert [[int(oo[t * L + l + 1] - oo[t * L + l]) for t in range(T)] for l in range(L)] == g["a.c2l_sizes"].tolist()
    assert (wf[rows].view(np.int64) == g["a.c2l_wf"].view(np.int64)).all()
    dist = float(np.abs(lf[rows] - g["a.c2l_lf"]).max())
    print(f"clouds_lf: restatement (fp64 inverse) vs reference (float32 inverse) {dist:.3e}")
    assert dist <= 1e-6


@pytest.mark.parametrize("family", sorted(E.MEASURED_LF_EPS))
def test_restatement_lf_error_per_family(family):
    """The restatement's clouds_lf against lf_extended over every case, in eps64 units of |inv(Ml)_rot| (|w| + |t|): the
    family's figure is the one recorded in _link_clouds_ref.MEASURED_LF_EPS (not above it, and the record not more than
    twice the measurement)."""
    worst = 0.0
    for case, (lm, _, wf, lf, oo) in _restated(family)[0]:
        assert np.isfinite(lm).all() and np.isfinite(lf).all() and np.isfinite(wf).all(), case[0]
        ext, unit = E.lf_extended(lm, wf, case[3], oo)
        e = E.lf_error_eps(lf, ext, unit)
        print(f"{case[0]:32s} rows {len(lf):7d}  lf error {e:6.2f} eps")
        worst = max(worst, e)
    rec = E.MEASURED_LF_EPS[family]
    print(f"{family:8s} worst {worst:.2f} eps  recorded {rec}  gpu fallback bound {E.gpu_lf_bound(family)} eps")
    assert worst <= rec, (family, worst)
    assert rec <= 2 * worst, (family, worst)


def test_extended_inverse_is_converged():
    """The yardstick's own inverse: residual |Ml X - I| of the Newton-refined longdouble inverse far below eps64, on the
    hardest matrices of the pose family."""
    assert np.finfo(np.longdouble).eps < 2.0 ** -60
    for case, (lm, *_) in _restated("pose")[0]:
        for Ml in lm.reshape(-1, 4, 4):
            X = E.inverse_extended(Ml)
            res = np.abs(Ml.astype(np.longdouble) @ X - np.eye(4, dtype=np.longdouble)).max()
            assert res <= 2.0 ** -58 * max(1.0, float(np.abs(Ml).max())), (case[0], float(res))


def _straddling(oo, po, links, T, K, rows):
    """Clusters with rows on both sides of a slice boundary of their (frame, link), from the offsets alone."""
    n, L = 0, len(links)
    for b in range(T * L):
        t, l = divmod(b, L)
        o = 0                                                     # relative to the block's first row
        for k in links[l]:
            size = int(po[t * K + k + 1] - po[t * K + k])
            if size and o // rows != (o + size - 1) // rows:
                n += 1
            o += size
    return n


def test_families_reach_what_they_are_for():
    # slice: totals, boundaries, straddling clusters, empties
    cases = {c[0]: (c, r) for f in E.FAMILIES for c, r in _restated(f)[0]}
    straddling, totals = 0, set()
    for label, (case, (_, _, _, _, oo)) in cases.items():
        if E.family_of(label) != "slice":
            continue
        _, coords, _, links, _, po = case
        T, K = coords.shape[:2]
        straddling += _straddling(oo, po, links, T, K, E.LC_ROWS)
        totals |= set(np.diff(oo).tolist())
    assert straddling >= 40, straddling
    assert totals >= set(E.SLICE_TOTALS)
    case, (_, _, _, _, oo) = cases["slice/boundaries"]
    po, links = case[5], case[3]
    cuts = set()
    for link in links:                                            # frame 0
        cuts |= set(np.cumsum([po[k + 1] - po[k] for k in link]).tolist())
    for j in (1, 2):
        assert {E.LC_ROWS * j - 1, E.LC_ROWS * j, E.LC_ROWS * j + 1} <= cuts
    case, (_, _, _, _, oo) = cases["slice/span"]
    sizes = np.diff(case[5])
    assert sizes.max() > 3 * E.LC_ROWS and sizes[0] % E.LC_ROWS != 0
    case = cases["slice/empties"][0]
    sizes = np.diff(case[5]).reshape(case[1].shape[:2])
    assert (sizes[:, [0, 2, 3, 5]] == 0).all() and (sizes[:, [1, 4]] > 0).all() and (sizes[:, [6, 7]] == 0).all()
    case = cases["slice/k256"][0]
    assert case[1].shape[1] == 256 and len(case[3][0]) == 255 and sorted(case[3][0]) == list(range(255))
    # stride: a link above LC_MAX_SLICES slices, not in block 0, in a launch of T = 2 whose other links are tiny
    case, (_, _, _, _, oo) = cases["stride/big"]
    per = np.diff(oo)
    assert case[1].shape[0] == 2 and per.max() == E.STRIDE_ROWS > E.LC_MAX_SLICES * E.LC_ROWS
    assert int(per.argmax()) != 0 and np.sort(per)[-2] < 16
    assert E.launch_grid_y(per.max()) == E.LC_MAX_SLICES
    # layout
    by = {l: cases[l][0] for l in cases if E.family_of(l) == "layout"}
    assert any(len(c[3]) == c[1].shape[1] for c in by.values()) and any(len(c[3]) == 1 and len(c[3][0]) > 1 for c in by.values())
    assert {c[1].shape[0] for c in by.values()} >= {1, 10}
    assert any(any(l != sorted(l) for l in c[3]) for c in by.values())
    rs = by["layout/repeated_shared_unused"]
    flat = [k for l in rs[3] for k in l]
    assert any(l.count(k) == 2 for l in rs[3] for k in l)                              # listed twice in one link
    assert any(sum(k in l for l in rs[3]) == 2 for k in set(flat))                      # in two links
    unused = sorted(set(range(rs[1].shape[1])) - set(flat))
    sizes = np.diff(rs[5]).reshape(rs[1].shape[:2])
    assert len(unused) >= 3 and (sizes[:, unused] > 0).all()
    assert len(by["layout/no_points"][4]) == 0 and by["layout/no_points"][5][-1] == 0
    # pose: every row exchange an affine matrix can ask of inv4 (row 3 is (0, 0, 0, 1): it is never the larger pivot)
    assert _restated("pose")[1] == {(0, 1), (0, 2), (1, 2)}
    for label in ("pose/cancel_0.001", "pose/cancel_1e-06"):
        case = cases[label][0]
        mean = np.linalg.norm(case[1][:, [0, 1], 3:].sum(1) / 2, axis=1)
        want = float(label.split("_")[1])
        assert (np.abs(mean / want - 1) < 1e-3).all(), (label, mean)
    M = cases["pose/scaled"][0][2][..., :3, :3]
    assert (np.abs(M @ M.transpose(0, 1, 3, 2) - np.eye(3)).max(axis=(2, 3)) > 0.5).all()
    assert np.abs(cases["pose/turns_t1e3"][0][1][..., :3]).max() > 900
    # antipodal: the sum of the two quaternions is exactly zero
    case, (lm, mm, wf, lf, oo) = cases["antipodal/two_links"]
    L = len(case[3])
    for t, l in E.ANTIPODAL_BLOCKS:
        assert (case[1][t, case[3][l], 3:].sum(0) == 0).all()
        assert np.isnan(lm[t, l, :3, :3]).all() and np.isfinite(lm[t, l, :3, 3]).all() and (lm[t, l, 3] == [0, 0, 0, 1]).all()
        assert oo[t * L + l + 1] > oo[t * L + l] and np.isnan(lf[oo[t * L + l]:oo[t * L + l + 1]]).all()
    keep = np.ones(len(lf), bool)
    for t, l in E.ANTIPODAL_BLOCKS:
        keep[oo[t * L + l]:oo[t * L + l + 1]] = False
    assert np.isfinite(lf[keep]).all() and np.isfinite(wf).all() and np.isfinite(mm).all()
    assert np.isfinite(lm.reshape(-1, 4, 4)[[b for b in range(2 * L) if divmod(b, L) not in E.ANTIPODAL_BLOCKS]]).all()


def _walk_case(case, oo, G, rows, nt=None, mutation=None):
    _, coords, _, links, _, po = case
    T, K = coords.shape[:2]
    return E.kernel_walk(oo, po, links, T, K, G, rows=rows, nt=nt, mutation=mutation)


@pytest.mark.parametrize("family", sorted(E.FAMILIES))
def test_coverage_model_at_the_kernels_constants(family):
    """The kernel's slice and stride loop, walked in Python with the launch's own grid.y: every output row written exactly once,
    from the row of `points` the restatement used."""
    trips, straddles = 0, 0
    for case, (_, _, _, _, oo) in _restated(family)[0]:
        T, K = case[1].shape[:2]
        src, _, _ = E.row_map(case[3], case[5], T, K)
        for G in {E.launch_grid_y(np.diff(oo).max()), 1}:         # max_link_rows as ops.link_clouds passes it, and 0
            writes, source, tr, st = _walk_case(case, oo, G, E.LC_ROWS)
            assert (writes == 1).all() and (source == src).all(), (case[0], G)
            if G > 1:
                trips, straddles = max(trips, tr), straddles + st
    if family == "stride":
        assert trips == 2
    if family == "slice":
        assert straddles >= 80 and trips == 1


def test_coverage_model_at_small_constants():
    """LC_ROWS = 4, G = 3, three threads: every branch of the walk on cases small enough to go thread by thread."""
    rng = np.random.default_rng(7)
    seen_trips = 0
    for i in range(40):
        T, K = int(rng.integers(1, 4)), int(rng.integers(1, 7))
        sizes = rng.integers(0, 12, size=(T, K)) * (rng.random((T, K)) < 0.7)
        links = [[int(k) for k in rng.integers(0, K, size=rng.integers(1, 5))] for _ in range(int(rng.integers(1, K + 1)))]
        po = np.concatenate([[0], np.cumsum(sizes.reshape(-1))]).astype(np.int64)
        oo = E.out_offsets_of(links, po, T, K)
        src, _, _ = E.row_map(links, po, T, K)
        for G in (1, 3):
            writes, source, trips, _ = E.kernel_walk(oo, po, links, T, K, G, rows=4, nt=3)
            assert (writes == 1).all() and (source == src).all(), (i, G)
            seen_trips = max(seen_trips, trips)
    assert seen_trips >= 3


@pytest.mark.parametrize("mutation", E.MUTATIONS)
def test_coverage_model_notices_a_wrong_walk(mutation):
    """The three slips the families are there for (the source row without `- o`, `hi` clipped one row short, no second trip):
    each one leaves a row unwritten or read from the wrong place in the slice and stride families."""
    caught = {}
    for family in ("slice", "stride"):
        for case, (_, _, _, _, oo) in _restated(family)[0]:
            T, K = case[1].shape[:2]
            src, _, _ = E.row_map(case[3], case[5], T, K)
            writes, source, _, _ = _walk_case(case, oo, E.launch_grid_y(np.diff(oo).max()), E.LC_ROWS, mutation=mutation)
            caught[case[0]] = int(((writes != 1) | (source != src)).sum())
    print(mutation, caught)
    assert caught["stride/big"] > 0
    if mutation != "first_trip_only":
        assert all(n > 0 for n in caught.values()), caught
