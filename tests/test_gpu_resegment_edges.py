"""GPU: the three small kernels between training and ICP at their edges -- the stable grouping by label with its change of frame
(csrc/group.hip: `k_group_offsets` / `k_group_scatter` up to 16384 points and for every batch, `k_group_count` / `k_group_excl` /
`k_group_scatter_big` above), the Gauss-Jordan `inv4x4` inside it, and the three copies of the strict float32 box mask
(`k_icp_mask` ascending through ops.aabb_mask, `k_icp_mask` binned and step 1 of `k_masked_icp` through ops.masked_icp).

References and tolerances come from tests/_resegment_edges.py (integer arithmetic, correctly rounded fma restatement, exact
rational inverse with a derived forward bound, float32 box restatement, oracle.icp) and are checked on the CPU by
tests/test_resegment_edges_cpu.py; nothing here is measured from a kernel.  No input carries a label outside [0, k) or offsets
that are not monotone.  Every test runs under its own watchdog, which ends the process: a hung kernel must not be waited on."""
import faulthandler

import numpy as np
import pytest
import torch

import _resegment_edges as E

pytestmark = pytest.mark.gpu


@pytest.fixture(autouse=True)
def _time_limit():
    faulthandler.dump_traceback_later(120, exit=True)
    yield
    faulthandler.cancel_dump_traceback_later()


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "GPU tests need the MI355X"
    from autourdf_amd import _lib
    _lib.load()
    return torch.device("cuda:0")


def _t(a, dev):
    return torch.from_numpy(np.ascontiguousarray(a)).to(dev)


def _group(dev, X, lab, M, inverse):
    from autourdf_amd import ops
    local, off = ops.group_to_local(_t(X, dev), _t(lab, dev), _t(M, dev), m_is_inverse=inverse)
    return local.cpu().numpy(), off.cpu().numpy()


def _group_exact(dev, n, k, lab, what):
    """Exact inputs through creg_group_to_local_f64 with the inverse poses given: offsets and every row, bit for bit."""
    X, (_, I) = E.exact_points(n), E.exact_poses(k)
    ref, ref_off = E.group_reference_exact(X, lab, k, I)
    out, off = _group(dev, X, lab, I, True)
    np.testing.assert_array_equal(off, ref_off, err_msg=what)
    np.testing.assert_array_equal(out, ref, err_msg=what)


# ================================================================================================ A. grouping
@pytest.mark.parametrize("n", [1, 63, 64, 65, 1023, 1024, 1025, 16384])
def test_group_small_form_sizes(dev, n):
    """k_group_offsets + k_group_scatter, one wave per cluster: the ballot / prefix-popcount slot at a partial last wave round
    (n = 63, 65, 1023, 1025), exactly full rounds (64, 1024), a single point, and the largest n of this form (16384), with one
    cluster, two and seventeen (more clusters than points at n = 1).  The integer points name their own index, so a wrong slot
    shows as a wrong row."""
    for k in (1, 2, 17):
        _group_exact(dev, n, k, E.spread_labels(n, k, 100 + n + k), f"n={n} k={k}")


def test_group_small_form_k_4096(dev):
    """k_group_offsets, k across its 1024 threads: k + 1 = 4097 counters zeroed by 1024 threads, the serial scan over 4096
    clusters of which about 1200 are empty and most hold one or two points; k_group_scatter with 4096 workgroups."""
    lab = E.spread_labels(5000, 4096, 3, cover=False)
    assert (np.bincount(lab, minlength=4096) == 0).sum() > 1000
    _group_exact(dev, 5000, 4096, lab, "n=5000 k=4096")


@pytest.mark.parametrize("last", [True, False], ids=["last_carries", "last_other"])
@pytest.mark.parametrize("n", [16385, 20479, 20480, 20481, 20483])
def test_group_large_form_sizes(dev, n, last):
    """k_group_count / k_group_scatter_big, lanes past n: n one above the switch, one below / at / above a multiple of 4096 and
    n % 4 == 3.  Cluster 1 has all its members in the last round (the partial one), cluster 3 its only members in one thread's four
    consecutive points.  The lanes past the end re-read labels[n - 1]: with the last point carrying label 1 they must not be
    counted for it, and with it carrying label 0 cluster 1 must not gain or lose a row either (cluster 2 follows it in the
    output and starts at index 0, so a row written past cluster 1's segment lands on rows that were written long before)."""
    _group_exact(dev, n, 5, E.large_n_labels(n, last), f"n={n} last={last}")


@pytest.mark.parametrize("k", [1, 3, 4, 5, 255, 256, 257, 4095, 4096])
def test_group_large_form_cluster_counts(dev, k):
    """k_group_excl, k across a thread (3, 4, 5), a wave (255, 256, 257: 64 threads x 4) and the block (4095, 4096): the
    exclusive scan's base per thread, per wave and the guarded last store; k_group_count's shared counters for k > 1024.
    Label vectors: only label 0, only label k - 1, all labels, and a run of empty clusters in the middle (700 of them at
    k >= 4095: whole waves of the scan carry zeros)."""
    for pattern in ("first", "last", "spread", "gap"):
        _group_exact(dev, 16385, k, E.large_k_labels(16385, k, pattern), f"k={k} {pattern}")


@pytest.mark.parametrize("n", [1025, 20483])
def test_group_random_doubles_match_the_fma_restatement(dev, n):
    """k_group_scatter (n = 1025) and k_group_scatter_big (n = 20483), the arithmetic: `fma(I2,p2,fma(I1,p1,I0*p0)) + I3` on
    random doubles with random inverse poses, against the same expression with a correctly rounded fma -- a contracted product,
    another association or a float32 intermediate changes bits."""
    rng = np.random.default_rng(n)
    k = 5
    X, lab = 3.0 * rng.normal(size=(n, 3)), E.spread_labels(n, k, n + 1)
    I = np.linalg.inv(E.random_rigid(rng, k, t_scale=2.0))
    ref, ref_off = E.group_reference_fma(X, lab, k, I)
    out, off = _group(dev, X, lab, I, True)
    np.testing.assert_array_equal(off, ref_off)
    np.testing.assert_array_equal(out, ref)


@pytest.mark.parametrize("exact", [True, False], ids=["exact", "random"])
def test_group_regime_switch_agrees_row_for_row(dev, exact):
    """creg_group_to_local_f64's switch at n = 16384 / 16385: the same labels, points and poses, then one point appended.  Every
    cluster's segment of the large form starts with the rows the small form gave it (k_group_scatter and k_group_scatter_big
    promise the same bits), and the appended row ends its cluster's segment.  Exact inputs: both also equal the integer
    reference; random doubles and rigid poses inverted in the kernel: the two forms' inv4x4 and products agree to the bit."""
    n, k = 16384, 17
    rng = np.random.default_rng(77)
    lab = E.spread_labels(n + 1, k, 78)
    if exact:
        X, (_, P) = E.exact_points(n + 1), E.exact_poses(k)
    else:
        X, P = rng.normal(size=(n + 1, 3)), E.random_rigid(rng, k, t_scale=5.0)
    a, a_off = _group(dev, X[:n], lab[:n], P, exact)
    b, b_off = _group(dev, X, lab, P, exact)
    np.testing.assert_array_equal(a_off, E.group_offsets(lab[:n], k))
    np.testing.assert_array_equal(b_off, E.group_offsets(lab, k))
    for j in range(k):
        cnt = a_off[j + 1] - a_off[j]
        np.testing.assert_array_equal(b[b_off[j]:b_off[j] + cnt], a[a_off[j]:a_off[j + 1]], err_msg=f"cluster {j}")
    j = int(lab[n])
    assert b_off[j + 1] - b_off[j] == a_off[j + 1] - a_off[j] + 1
    if exact:
        np.testing.assert_array_equal(a, E.group_reference_exact(X[:n], lab[:n], k, P)[0])
        np.testing.assert_array_equal(b, E.group_reference_exact(X, lab, k, P)[0])
    else:
        last = b[b_off[j + 1] - 1]
        want = np.linalg.solve(P[j], np.r_[X[n], 1.0])[:3]
        np.testing.assert_allclose(last, want, atol=1e-12)


@pytest.mark.parametrize("B", [1, 16])
def test_group_batch_small_frames(dev, B):
    """k_group_offsets / k_group_scatter with grid.y = problem: one frame and the full table of 16, every frame with its own
    points, labels and poses (exact inputs, n = 1025, k = 17), against the integer reference; group_to_local_each takes the
    same launch and gives the same bits."""
    from autourdf_amd import ops
    n, k = 1025, 17
    Xs = [E.exact_points(n, start=1000 * b) for b in range(B)]
    labs = [E.spread_labels(n, k, 300 + b) for b in range(B)]
    Is = [E.exact_poses(k, shift=b)[1] for b in range(B)]
    args = ([_t(x, dev) for x in Xs], [_t(l, dev) for l in labs], [_t(i, dev) for i in Is])
    got = ops.group_to_local_batch(*args, m_is_inverse=True)
    each = ops.group_to_local_each(*args, m_is_inverse=True)
    assert len(got) == len(each) == B
    for b in range(B):
        ref, ref_off = E.group_reference_exact(Xs[b], labs[b], k, Is[b])
        np.testing.assert_array_equal(got[b][1].cpu().numpy(), ref_off, err_msg=f"problem {b}")
        np.testing.assert_array_equal(got[b][0].cpu().numpy(), ref, err_msg=f"problem {b}")
        assert torch.equal(each[b][0], got[b][0]) and torch.equal(each[b][1], got[b][1])


@pytest.mark.parametrize("inverse", [True, False], ids=["inverse_given", "inverse_in_kernel"])
def test_group_batch_of_large_frames_equals_single_calls(dev, inverse):
    """A batch of frames above 16384 points runs k_group_offsets / k_group_scatter where the single call runs k_group_count /
    k_group_excl / k_group_scatter_big: B = 3 at n = 16385, k = 37, random doubles, must give the single calls' bits -- with the
    inverse poses given and with inv4x4 in the kernel; group_to_local_each the same."""
    from autourdf_amd import ops
    rng = np.random.default_rng(5)
    n, k, B = 16385, 37, 3
    Xs = [_t(rng.normal(size=(n, 3)), dev) for _ in range(B)]
    labs = [_t(E.spread_labels(n, k, 400 + b), dev) for b in range(B)]
    Ps = [E.random_rigid(rng, k, t_scale=3.0) for _ in range(B)]
    Ms = [_t(np.linalg.inv(p) if inverse else p, dev) for p in Ps]
    batch = ops.group_to_local_batch(Xs, labs, Ms, m_is_inverse=inverse)
    each = ops.group_to_local_each(Xs, labs, Ms, m_is_inverse=inverse)
    for b in range(B):
        loc, off = ops.group_to_local(Xs[b], labs[b], Ms[b], m_is_inverse=inverse)
        np.testing.assert_array_equal(off.cpu().numpy(), E.group_offsets(labs[b].cpu().numpy(), k))
        assert torch.equal(batch[b][1], off) and torch.equal(batch[b][0], loc), f"problem {b}"
        assert torch.equal(each[b][1], off) and torch.equal(each[b][0], loc), f"problem {b}"


# ================================================================================================ B. the in-kernel inverse
@pytest.mark.parametrize("n", [257, 16385])
def test_inverse_of_permutations_is_exact(dev, n):
    """inv4x4 in k_group_scatter (n = 257) and k_group_scatter_big (n = 16385), the pivot search and the compile-time row swaps:
    the 24 proper signed permutations with integer translations and the 18 signed 4x4 permutations whose last row is not
    (0, 0, 0, 1) force every (column, row) exchange on an exactly zero diagonal candidate; every step is exact, so the rows equal
    the integer reference bit for bit.  Without the search the elimination divides by that zero."""
    M, I = E.perm_poses()
    k = len(M)
    X, lab = E.exact_points(n), E.spread_labels(n, k, 500 + n)
    ref, ref_off = E.group_reference_exact(X, lab, k, I)
    out, off = _group(dev, X, lab, M, False)
    np.testing.assert_array_equal(off, ref_off)
    bad = np.nonzero((out != ref).any(1))[0]
    assert len(bad) == 0, ("clusters with wrong rows:", sorted(set(lab[np.argsort(lab, kind="stable")][bad].tolist())))


@pytest.fixture(scope="module")
def tolerance_family():
    P, fam = E.tolerance_poses()
    I, kappa = E.exact_inverses(P)
    return P, fam, I, kappa


def _check_inverse(out, off, X, lab, fam, I, kappa, what):
    ref, ref_off = E.inverse_reference(X, lab, len(I), I)
    tol = E.inverse_tolerance(X, lab, I, kappa)
    np.testing.assert_array_equal(off, ref_off, err_msg=what)
    ratio = np.abs(out - ref) / tol
    L = np.array(fam)[lab[np.argsort(lab, kind="stable")]]
    print(what, "worst |error| / tolerance per family:", {f: float(ratio[L == f].max()) for f in ("tie", "trained", "affine")})
    assert np.isfinite(out).all() and (ratio <= 1.0).all(), (what, float(ratio.max()), L[np.nonzero((ratio > 1).any(1))[0][:5]])


@pytest.mark.parametrize("form", ["small", "large", "batch"])
def test_inverse_families_within_the_derived_bound(dev, tolerance_family, form):
    """inv4x4, accuracy: rotations by 45 degrees (tied pivot candidates), 200 float32-rounded rotations with translations of order
    100, affine poses of condition 1e2 .. 1e8 with M[3,3] in {1, 2} -- against the exact rational inverse applied in extended
    precision, within eps (8 kappa + 8) sum |I| |(p, 1)| per entry (derivation: _resegment_edges.inverse_tolerance; the CPU test
    shows a float64 emulation of the elimination stays below a tenth of it).  k_group_scatter (n = 4099), k_group_scatter_big
    (n = 16385) and a batch of two frames."""
    from autourdf_amd import ops
    P, fam, I, kappa = tolerance_family
    if form == "batch":
        data = [E.points_for_poses(P, 4099, 11 + 10 * b) for b in range(2)]
        got = ops.group_to_local_batch([_t(x, dev) for x, _ in data], [_t(l, dev) for _, l in data], [_t(P, dev)] * 2)
        for b, ((X, lab), (out, off)) in enumerate(zip(data, got)):
            _check_inverse(out.cpu().numpy(), off.cpu().numpy(), X, lab, fam, I, kappa, f"batch problem {b}")
        return
    n = 4099 if form == "small" else 16385
    X, lab = E.points_for_poses(P, n, 7)
    out, off = _group(dev, X, lab, P, False)
    _check_inverse(out, off, X, lab, fam, I, kappa, form)


# ================================================================================================ C. ops.aabb_mask
def _check_mask(dev, world, woff, frame, scale, what):
    """ops.aabb_mask against the float32 box restatement (bit for bit, non-empty clusters) and oracle.icp.aabb_mask (count and
    the ascending indices; the cells beyond count are unspecified).  Returns (index rows cut to their counts, counts, boxes)."""
    from autourdf_amd import ops
    idx, cnt, boxes = ops.aabb_mask(_t(world, dev), _t(np.asarray(woff, np.int32), dev), _t(frame, dev), scale=scale)
    idx, cnt, boxes = idx.cpu().numpy(), cnt.cpu().numpy(), boxes.cpu().numpy()
    want_box = E.restated_boxes(world, woff, scale)
    full = np.diff(woff) > 0
    np.testing.assert_array_equal(boxes[full], want_box[full], err_msg=what)
    ref = E.mask_reference(world, woff, frame, scale)
    np.testing.assert_array_equal(cnt, [len(r) for r in ref], err_msg=what)
    rows = [idx[c, :cnt[c]] for c in range(len(ref))]
    for c, r in enumerate(ref):
        np.testing.assert_array_equal(rows[c], r, err_msg=f"{what} cluster {c}")
    return rows, cnt, boxes


@pytest.mark.parametrize("nf", [1, 63, 64, 65, 1023, 1024, 1025, 3073])
def test_mask_frame_sizes(dev, nf):
    """k_icp_mask binned = 0, the ordered compaction: frames that end inside a wave (63, 65), on one (64), inside the 1024-thread
    round (1023, 1025), on it (1024) and after three rounds and a point (3073), for 1, 3 and 70 clusters; random frames over
    twice the boxes' union, so rows are neither empty nor full."""
    for k in (1, 3, 70):
        world, woff = E.blob_clusters(k, 600 + k)
        frame = E.frame_over_boxes(E.restated_boxes(world, woff, 1.2), nf, 700 + nf + k)
        rows, cnt, _ = _check_mask(dev, world, woff, frame, 1.2, f"nf={nf} k={k}")
        if nf >= 1023:
            assert 0 < cnt.sum() < k * nf


@pytest.mark.parametrize("scale", [1.0, 1.2, 1.6])
def test_mask_faces_are_strict(dev, scale):
    """k_icp_mask binned = 0, strict faces: per cluster and face a point exactly on the bound, one double inside and one double
    outside (other coordinates at the box centre), and the eight exact corners -- built from the restated box, which the
    returned box must equal bit for bit.  Only the inside points of a cluster's own faces may be listed for it."""
    world, woff = E.blob_clusters(5, 21)
    frame, owner, kind = E.face_points(E.restated_boxes(world, woff, scale))
    rows, cnt, _ = _check_mask(dev, world, woff, frame, scale, f"scale={scale}")
    for c in range(5):
        listed = np.zeros(len(frame), bool)
        listed[rows[c]] = True
        mine = owner == c
        assert (listed[mine] == (kind[mine] == "in")).all(), (c, kind[mine][listed[mine]])


@pytest.mark.parametrize("scale", [1.0, 1.2, 1.6])
def test_mask_own_points_decided_by_float32_rounding(dev, scale):
    """k_icp_mask, the float32 evaluation order of `c -/+ half_scale * sz`: the clusters' own points (float32 -> float64) as the
    frame.  At scale 1.0 the extreme points lie within a float32 ulp of the faces and the roundings of c and c -/+ 0.5 sz decide
    them (a box evaluated in double lists other points: asserted on the CPU); at 1.2 and 1.6 a fused multiply-add moves box
    entries, which the bit-for-bit box comparison sees."""
    world, woff = E.blob_clusters(20, 11)
    rows, cnt, _ = _check_mask(dev, world, woff, world.astype(np.float64), scale, f"scale={scale}")
    own = np.diff(woff)
    assert (cnt >= own - 6).all()                          # at most the six extreme points of a cluster fall on its own faces
    if scale > 1.0:
        assert (cnt >= own).all()


def test_mask_zero_extent_boxes_list_nothing(dev):
    """k_icp_mask, zero-extent boxes: a one-point cluster and a cluster flat in z to the bit have lo == hi on an axis, so nothing is
    strictly inside -- not the point itself, not frame points at the degenerate coordinate, at any scale."""
    rng = np.random.default_rng(31)
    good, _ = E.blob_clusters(1, 32)
    flat = (np.array([2.0, 1.0, 0.0]) + rng.normal(scale=[0.3, 0.3, 0.0], size=(30, 3))).astype(np.float32)
    flat[:, 2] = np.float32(0.37)
    single = np.array([[-1.5, 0.25, 0.8125]], np.float32)
    world = np.concatenate([single, good, flat])
    woff = np.array([0, 1, 1 + len(good), 1 + len(good) + 30], np.int32)
    in_plane = flat.astype(np.float64) * [0.9, 0.9, 1.0] + [0.2, 0.1, 0.0]          # inside the flat cluster's x / y range, z exactly its z
    frame = np.concatenate([single.astype(np.float64), in_plane, flat.astype(np.float64), good.astype(np.float64),
                            rng.uniform(-3, 3, size=(200, 3))])
    assert (in_plane[:, 2] == float(np.float32(0.37))).all()
    for scale in (1.0, 1.2, 1.6):
        rows, cnt, boxes = _check_mask(dev, world, woff, frame, scale, f"scale={scale}")
        assert cnt[0] == 0 and cnt[2] == 0 and cnt[1] > 0
        assert (boxes[0, :3] == boxes[0, 3:]).all() and boxes[2, 2] == boxes[2, 5] == np.float32(0.37)


def test_mask_empty_cluster_between_two_good_ones(dev):
    """k_icp_mask, `e > b`: a cluster without points lists nothing (its box row is not compared), and its neighbours' counts, rows
    and boxes equal those of a call without it."""
    world, woff = E.blob_clusters(2, 41)
    frame = E.frame_over_boxes(E.restated_boxes(world, woff, 1.2), 1500, 42)
    with_empty = np.array([woff[0], woff[1], woff[1], woff[2]], np.int32)
    rows2, cnt2, box2 = _check_mask(dev, world, woff, frame, 1.2, "two clusters")
    rows3, cnt3, box3 = _check_mask(dev, world, with_empty, frame, 1.2, "empty cluster in the middle")
    assert cnt3[1] == 0 and cnt2.min() > 0
    for a, b in ((0, 0), (1, 2)):
        np.testing.assert_array_equal(rows3[b], rows2[a])
        np.testing.assert_array_equal(box3[b], box2[a])


def test_mask_far_cluster_compares_in_double(dev):
    """k_icp_mask, the comparison of float64 frame points with the float32 box widened to double: a cluster near
    (1000, -1000, 1000), where a float32 ulp is 6e-5, and frame points that are random doubles between the float32 neighbours
    of each face -- a comparison in float32, or of a rounded point, lists other points."""
    world, woff = E.blob_clusters(1, 31, pts=60, centre=(1000.0, -1000.0, 1000.0), spread=0.5)
    frame = E.between_float32_neighbours(E.restated_boxes(world, woff, 1.2), 16, 5)
    rows, cnt, _ = _check_mask(dev, world, woff, frame, 1.2, "far cluster")
    assert 10 < cnt[0] < 86


# ================================================================================================ D. the mask inside masked_icp
ICP_CASES = {"one_launch": ([200, 197, 203, 201], 60), "many_workgroups": ([1100, 1103], 500)}
ICP_KERNEL = {"one_launch": "k_masked_icp step 1", "many_workgroups": "k_icp_mask binned"}


@pytest.fixture(scope="module", params=list(ICP_CASES))
def icp_case(request):
    sizes, n_outside = ICP_CASES[request.param]
    return request.param, E.icp_case(sizes, scale=1.0, seed=3, n_outside=n_outside)


def _masked_icp(dev, case, frame):
    from autourdf_amd import ops
    local, world = np.concatenate(case["local"]), np.concatenate(case["world"])
    M_out, w_out, n_it = ops.masked_icp(_t(local, dev), _t(world, dev), _t(case["off"], dev), _t(frame, dev), _t(case["M"], dev),
                                        scale=case["scale"])
    return M_out.cpu().numpy(), w_out.cpu().numpy(), n_it.cpu().numpy()


def test_masked_icp_strict_faces(dev, icp_case):
    """k_masked_icp step 1 ("one_launch": 4 clusters of about 200 points) and k_icp_mask binned ("many_workgroups": 2 clusters of
    about 1100 points against about 3000 frame points), strict faces: the frame holds per face 32 decoys whose face coordinate is
    the exact bound, next to the true targets.  The oracle with a `<=` at any one face ends at least 1e-5 away (asserted on the
    CPU), so poses and moved points within the suite's 1e-8 of oracle.icp.masked_icp mean no decoy was admitted."""
    from autourdf_amd import ops
    from oracle import icp as oicp
    name, case = icp_case
    assert ops.masked_icp_regime(int(case["off"][-1]), len(case["frame"]), len(case["local"])) == name, ICP_KERNEL[name]
    M_out, w_out, n_it = _masked_icp(dev, case, case["frame"])
    ow, om = oicp.masked_icp(case["local"], case["world"], case["frame"], case["M"], scale=case["scale"])
    print(name, "largest pose / point difference from the oracle:", np.abs(M_out - om).max(), np.abs(w_out - np.concatenate(ow)).max())
    np.testing.assert_allclose(M_out, om, atol=1e-8)
    np.testing.assert_allclose(w_out, np.concatenate(ow), atol=1e-8)
    assert (n_it >= 1).all() and np.abs(M_out - case["M"]).max() > 1e-3


def test_masked_icp_decoys_only_leaves_the_poses_alone(dev, icp_case):
    """The same two kernels with a frame of decoys (on the faces) and outside points only: no target is strictly inside, so the
    poses come back bit for bit, as oracle.icp.masked_icp returns them (checked on the CPU) and as an empty box always did."""
    from autourdf_amd import ops
    name, case = icp_case
    frame = case["frame"][case["kind"] != "true"]
    assert ops.masked_icp_regime(int(case["off"][-1]), len(frame), len(case["local"])) == name, ICP_KERNEL[name]
    M_out, w_out, _ = _masked_icp(dev, case, frame)
    np.testing.assert_array_equal(M_out, case["M"])
    src = [loc @ M[:3, :3].T + M[:3, 3] for loc, M in zip(case["local"], case["M"])]
    np.testing.assert_allclose(w_out, np.concatenate(src), atol=1e-12)
