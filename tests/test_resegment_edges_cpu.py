"""CPU: the builders of tests/_resegment_edges.py reach what they are built for, and its references and tolerances hold for a
correct implementation.  No GPU, no kernel: every figure below comes from numpy / fractions restatements.

Figures recorded when this file was written (the assertions hold them to the stated bounds):
* exchanges forced by the permutation family: (column, pivot row) = (0,1) (0,2) (0,3) (1,2) (1,3) (2,3), the candidate a[c][c] is
  exactly 0 at each; the elimination WITHOUT the pivot search gets 38 of the 42 matrices wrong (it divides by that zero);
* emulated inverse (float64, no fma) against the exact one, worst |error| / tolerance over the tolerance families at n = 4099 and
  n = 16385: tie 5.8e-4, trained 6.0e-4, affine 6.9e-4 -- bound asserted: 0.1;
* scale 1.0, the clusters' own points as the frame: the float32 box and the float64 box decide differently for 11 points of the 20
  clusters; a fused `ctr -/+ hs * sz` gives the same box at 1.0 (hs = 0.5: the product is exact) and 29 / 27 different box
  entries at 1.2 / 1.6, which the bit-for-bit box comparison of the GPU test sees;
* decoy sensitivity (largest |pose entry| difference between the strict mask and a `<=` mask, oracle ICP): one-launch case
  6.4e-4 .. 3.8e-3 per cluster with all faces lenient, at least 5.6e-4 with any single face lenient; many-workgroup case
  4.2e-5 / 9.4e-5 per cluster and at least 3.0e-5 with a single face -- bound asserted: 1e-5, 1000 times the 1e-8 the GPU
  comparison allows.
"""
import numpy as np
import pytest

import _resegment_edges as E


# ---------------------------------------------------------------------------------------------------------- A. grouping
def test_exact_inputs_are_exact_and_self_describing():
    """The integer reference equals the float64 evaluation in ANY order (so no rounding happens in the kernels' order either),
    and the first coordinate of a point names its index: a wrong slot cannot hide behind an equal row."""
    n, k = 5000, 4096
    X, (M, I), lab = E.exact_points(n), E.exact_poses(k), E.spread_labels(5000, 4096, 3, cover=False)
    ref, off = E.group_reference_exact(X, lab, k, I)
    order = np.argsort(lab, kind="stable")
    L = lab[order]
    fwd = ((I[L, 0:3, 0] * X[order, 0:1] + I[L, 0:3, 1] * X[order, 1:2]) + I[L, 0:3, 2] * X[order, 2:3]) + I[L, 0:3, 3]
    bwd = I[L, 0:3, 3] + (I[L, 0:3, 2] * X[order, 2:3] + (I[L, 0:3, 1] * X[order, 1:2] + I[L, 0:3, 0] * X[order, 0:1]))
    np.testing.assert_array_equal(fwd, ref)
    np.testing.assert_array_equal(bwd, ref)
    assert len(np.unique(X[:, 0])) == n
    # M and I are inverse to each other, so applying M to the reference rows gives the points back, in group order
    back = np.einsum("nac,nc->na", M[L, :3, :3], ref) + M[L, :3, 3]
    np.testing.assert_array_equal(back, X[order])
    counts = np.diff(off)
    assert (counts == 0).sum() > 1000 and (counts == 1).sum() > 1000 and counts.max() >= 3        # k = 4096 at n = 5000: sparse clusters


def test_fma_restatement_is_correctly_rounded():
    """fma_exact against cases where the fused and the two-step result differ, and against exact products."""
    a, b = 1.0 + 2.0 ** -30, 1.0 - 2.0 ** -30
    assert a * b - 1.0 == 0.0 and E.fma_exact(a, b, -1.0) == -(2.0 ** -60)
    assert E.fma_exact(3.0, 5.0, 7.0) == 22.0 and E.fma_exact(0.1, 10.0, -1.0) == 2.0 ** -54
    rng = np.random.default_rng(0)
    x = rng.normal(size=(200, 3))
    differs = sum(E.fma_exact(p, q, r) != p * q + r for p, q, r in x.tolist())
    assert differs > 20                                     # random doubles do separate a fused from an unfused evaluation


@pytest.mark.parametrize("n", [16385, 20479, 20480, 20481, 20483])
@pytest.mark.parametrize("last", [True, False])
def test_large_n_labels_reach_the_last_round_and_one_thread(n, last):
    lab = E.large_n_labels(n, last)
    r0 = (n - 1) // E.GROUP_ROUND * E.GROUP_ROUND
    one = np.nonzero(lab == 1)[0]
    assert (lab[n - 1] == 1) == last
    if last or n - r0 > 1:
        assert one.min() == r0 and one.max() == (n - 1 if last else one.max()) < n
    else:
        assert len(one) == 0                                # the last round is one point: without it the cluster is empty
    three = np.nonzero(lab == 3)[0]
    assert len(three) == 4 and three[0] % 4 == 0 and (np.diff(three) == 1).all()
    assert lab[0] == 2 and set(np.unique(lab)) | {1} == {0, 1, 2, 3, 4}
    assert lab.min() >= 0 and lab.max() < 5


@pytest.mark.parametrize("k", [1, 3, 4, 5, 255, 256, 257, 4095, 4096])
def test_large_k_labels_patterns(k):
    n = 16385
    for pattern in ("first", "last", "spread", "gap"):
        lab = E.large_k_labels(n, k, pattern)
        assert lab.dtype == np.int32 and lab.min() >= 0 and lab.max() < k and len(lab) == n
        counts = np.bincount(lab, minlength=k)
        if pattern == "first":
            assert counts[0] == n
        if pattern == "last":
            assert counts[k - 1] == n
        if pattern == "spread":
            assert (counts > 0).all()
        if pattern == "gap" and k >= 3:
            empty = np.nonzero(counts == 0)[0]
            assert len(empty) == max(1, min(k // 3, 700)) and (np.diff(empty) == 1).all() and empty[0] == k // 3
            assert counts[0] > 0 and counts[k - 1] > 0
            if k >= 4095:
                assert len(empty) >= 500


# ---------------------------------------------------------------------------------------------------------- B. inverse
def test_permutation_family_forces_every_exchange_on_a_zero_pivot():
    """Every (column, later row) exchange the 4x4 elimination can make is forced by some matrix of the family, each time
    with an exactly zero candidate on the diagonal; the emulation with the search reproduces the integer inverses to the bit,
    the one without it does not."""
    M, I = E.perm_poses()
    seen, wrong = set(), 0
    for m, i in zip(M, I):
        log = []
        np.testing.assert_array_equal(E.emulate_inv4x4(m, log=log), i)
        for c, p, cand in log:
            if p != c:
                assert cand == 0.0
                seen.add((c, p))
        wrong += not np.array_equal(E.emulate_inv4x4(m, pivot=False), i)
    assert seen == {(0, 1), (0, 2), (0, 3), (1, 2), (1, 3), (2, 3)}
    assert {(c, p) for c, p in seen if p < 3} == {(0, 1), (0, 2), (1, 2)}            # ... the first three by genuine poses alone
    assert wrong >= 30                                                                # recorded: 38 of 42


def test_tie_poses_tie_the_pivot_candidates():
    for ax, m in enumerate(E.tie_poses()):
        u, v = (ax + 1) % 3, (ax + 2) % 3
        assert abs(m[u, u]) == abs(m[v, u]) == np.sqrt(0.5)
        np.testing.assert_allclose(m[:3, :3] @ m[:3, :3].T, np.eye(3), atol=1e-15)


def test_exact_inverse_is_an_inverse():
    P, fam = E.tolerance_poses()
    assert len(P) == 3 + 200 + 8 and fam.count("trained") == 200
    assert (P[3:203] == P[3:203].astype(np.float32)).all()                            # float32-representable entries
    I, kap = E.exact_inverses(P)
    for m, i, kp in zip(P, I, kap):
        np.testing.assert_allclose(m @ i, np.eye(4), atol=8 * E.EPS * kp)
    assert kap[203:].max() > 1e8 and kap[:203].max() < 1e6


@pytest.mark.parametrize("n", [4099, 16385])
def test_emulated_inverse_stays_within_a_tenth_of_the_tolerance(n):
    """The kernel's elimination restated in float64 without fma, applied to the committed families and points: its error
    against the exact-inverse reference is below 0.1 x inverse_tolerance everywhere (recorded worst ratio: 6.9e-4, affine
    family) -- the bound has room for any correct variant (fma or not, either choice at a tied pivot)."""
    P, fam = E.tolerance_poses()
    I, kap = E.exact_inverses(P)
    X, lab = E.points_for_poses(P, n, 7)
    ref, off = E.inverse_reference(X, lab, len(P), I)
    tol = E.inverse_tolerance(X, lab, I, kap)
    assert (np.diff(off) > 0).all() and (tol > 0).all()
    Iem = np.stack([E.emulate_inv4x4(m) for m in P])
    order = np.argsort(lab, kind="stable")
    L = lab[order]
    out = np.einsum("nac,nc->na", Iem[L, :3, :3], X[order]) + Iem[L, :3, 3]
    ratio = np.abs(out - ref) / tol
    print("worst emulated error / tolerance per family:", {f: float(ratio[np.array(fam)[L] == f].max()) for f in ("tie", "trained", "affine")})
    assert ratio.max() < 0.1
    # the other choice at a tied pivot is as good: exchange where the kernel would not
    for m, i in zip(E.tie_poses(), I[:3]):
        swapped = m.copy()
        ax = int(np.nonzero(np.diag(m[:3, :3]) == 1.0)[0][0])
        u, v = (ax + 1) % 3, (ax + 2) % 3
        swapped[[u, v]] = swapped[[v, u]]                                             # rows exchanged up front: inverse has columns exchanged
        alt = E.emulate_inv4x4(swapped)
        alt[:, [u, v]] = alt[:, [v, u]]
        assert np.abs(alt - i).max() <= 8 * E.EPS * np.abs(i).max()


# ---------------------------------------------------------------------------------------------------------- C. mask
def test_restated_boxes_are_float32_and_match_the_oracle_membership():
    """The restated box decides membership exactly as oracle.icp.aabb_mask does, on points one double either side of every face."""
    world, woff = E.blob_clusters(5, 21)
    for scale in (1.0, 1.2, 1.6):
        box = E.restated_boxes(world, woff, scale)
        assert box.dtype == np.float32
        frame, owner, kind = E.face_points(box)
        ref = E.mask_reference(world, woff, frame, scale)
        for c in range(5):
            np.testing.assert_array_equal(np.nonzero(E.inside(box[c], frame))[0], ref[c])
            mine = owner == c
            listed = np.zeros(len(frame), bool)
            listed[ref[c]] = True
            assert (listed[mine] == (kind[mine] == "in")).all()                       # only the inside points of its own faces
            assert (kind[mine] == "in").sum() == 6 and mine.sum() == 26


def test_scale_one_separates_float32_boxes_from_double_boxes():
    """With the clusters' own points as the frame at scale 1.0, whether an extreme point is listed is decided by the float32
    roundings of ctr and ctr -/+ 0.5 sz: the float64 box lists different points (recorded: 11 of 800).  A fused multiply-add
    cannot differ at 1.0 (0.5 sz is exact) but moves box entries at 1.2 and 1.6, where the boxes are compared bit for bit."""
    world, woff = E.blob_clusters(20, 11)
    frame = world.astype(np.float64)
    box, dbl = E.restated_boxes(world, woff, 1.0), E.double_boxes(world, woff, 1.0)
    differ = sum(int((E.inside(box[c], frame) != E.inside(dbl[c], frame)).sum()) for c in range(20))
    print("points the float32 and the float64 box decide differently at scale 1.0:", differ)
    assert differ >= 1
    for c in range(20):                                                               # the float64 box at 1.0 excludes its own extremes
        own = frame[woff[c]:woff[c + 1]]
        assert not E.inside(dbl[c], own)[[own[:, 0].argmin(), own[:, 0].argmax()]].any()
    np.testing.assert_array_equal(E.fused_boxes(world, woff, 1.0), box)
    for scale in (1.2, 1.6):
        moved = int((E.fused_boxes(world, woff, scale) != E.restated_boxes(world, woff, scale)).sum())
        print("box entries a fused multiply-add moves at scale", scale, ":", moved)
        assert moved >= 1


def test_far_cluster_points_lie_between_float32_neighbours():
    world, woff = E.blob_clusters(1, 31, pts=60, centre=(1000.0, -1000.0, 1000.0), spread=0.5)
    box = E.restated_boxes(world, woff, 1.2)
    assert np.spacing(np.float32(1000.0)) > 6e-5
    pts = E.between_float32_neighbours(box, 16, 5)
    assert len(pts) == 96
    ins = E.inside(box[0], pts)
    assert 10 < ins.sum() < 86                                                        # both sides of the faces are populated
    as32 = pts.astype(np.float32)                                                     # ... and a float32 comparison would get some wrong
    assert (np.all((as32 > box[0, :3]) & (as32 < box[0, 3:]), axis=1) != ins).any()


# ---------------------------------------------------------------------------------------------------------- D. masked ICP
ICP_CASES = {"one_launch": ([200, 197, 203, 201], 60), "many_workgroups": ([1100, 1103], 500)}


@pytest.fixture(scope="module", params=list(ICP_CASES))
def icp_case(request):
    sizes, n_outside = ICP_CASES[request.param]
    case = E.icp_case(sizes, scale=1.0, seed=3, n_outside=n_outside)
    case["strict"] = E.icp_with_mask(case, E.inside)
    return request.param, case


def test_icp_case_reference_mask_lists_true_targets_only(icp_case):
    name, case = icp_case
    n, nf, k = int(case["off"][-1]), len(case["frame"]), len(case["local"])
    regime = "many_workgroups" if n // k > 1024 or nf > 65536 else "one_launch"      # the rule ops.masked_icp_regime mirrors
    assert regime == name
    if name == "many_workgroups":
        assert 2800 <= nf <= 3300
    ref = E.mask_reference(np.concatenate(case["world"]), case["off"], case["frame"], case["scale"])
    for j, idx in enumerate(ref):
        kinds = case["kind"][idx]
        assert (kinds == "true").all() and (case["owner"][idx] == j).all() and len(idx) >= 10
        assert len(idx) == ((case["kind"] == "true") & (case["owner"] == j)).sum()    # every true target is strictly inside
    dec = case["kind"] == "decoy"
    assert dec.sum() == 6 * 32 * k
    for j in range(k):                                                                 # a decoy sits exactly on its face ...
        b = case["box"][j].astype(np.float64)
        for f in range(6):
            sel = dec & (case["owner"] == j) & (case["face"] == f)
            assert sel.sum() == 32 and (case["frame"][sel, f % 3] == b[f]).all()
            assert E.lenient_mask(b, case["frame"][sel], [f]).sum() >= 16             # ... and `<=` at that face admits most of them
    # ... within half of th = 1 of the sources at the initial pose
    for j in range(k):
        src = case["local"][j] @ case["M"][j][:3, :3].T + case["M"][j][:3, 3]
        d = case["frame"][dec & (case["owner"] == j)]
        assert np.sqrt(((d[:, None, :] - src[None, :, :]) ** 2).sum(-1).min(1)).max() < 0.5


def test_icp_case_is_sensitive_to_a_lenient_face(icp_case):
    """oracle ICP with the decoys wrongly admitted ends at least 1e-5 (largest pose entry) from the strict result: with every face
    lenient in EVERY cluster, with a single lenient face in at least one cluster -- 1000 times the GPU comparison's 1e-8."""
    from oracle import icp as oicp
    name, case = icp_case
    strict = case["strict"]
    _, om = oicp.masked_icp(case["local"], case["world"], case["frame"], case["M"], scale=case["scale"])
    np.testing.assert_array_equal(om, strict)                                         # the helper IS the oracle with another mask
    assert np.abs(strict - case["M"]).max() > 1e-3                                    # the true motion is found, not the input kept
    every = E.icp_with_mask(case, lambda b, f: E.lenient_mask(b, f))
    dev = np.abs(every - strict).reshape(len(strict), -1).max(1)
    print(name, "all faces lenient, per cluster:", dev)
    assert (dev >= 1e-5).all()
    for face in range(6):
        one = E.icp_with_mask(case, lambda b, f: E.lenient_mask(b, f, [face]))
        d = float(np.abs(one - strict).max())
        print(name, "face", face, "lenient:", d)
        assert d >= 1e-5


def test_oracle_leaves_the_pose_alone_without_targets(icp_case):
    """A frame of decoys and outside points only: the reference mask is empty and oracle.icp.masked_icp returns the input poses
    bit for bit (identity updates) -- what the GPU test asserts of the kernels."""
    from oracle import icp as oicp
    _, case = icp_case
    frame = case["frame"][case["kind"] != "true"]
    assert all(len(i) == 0 for i in E.mask_reference(np.concatenate(case["world"]), case["off"], frame, case["scale"]))
    ow, om = oicp.masked_icp(case["local"], case["world"], frame, case["M"], scale=case["scale"])
    np.testing.assert_array_equal(om, case["M"])
