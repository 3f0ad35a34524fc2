"""CPU: the cases of tests/_joint_axes_edges.py -- exactly those tests/test_gpu_joint_axes_edges.py runs on the kernel, both take
them from ``case(name)`` -- reach what they are built for, and the restatement could miss none of the failures the GPU file is
written for: with tol = 1e-9 the aggregates' bound there, leaving out a wave's share of a stride round (an aligned run of 64
samples), a wave's partial over all rounds, a whole round of 256, the first or the last sample, or taking local_axis' sign from another sample than the first
usable one moves local_axis or local_pos[:3] by at least 100 tol.

What the alignment can and cannot change.  a a^T is the same for a and -a, so which sample axes are negated before the sum moves
nothing: "leave the reversed sequence unflipped" and "align to sample 0" change sum a a^T by no bit.  What the alignment decides is
local_axis' sign, taken from the first usable sample's axis, and a wrong sign moves local_axis by 2.  So the sign is what is tested
here: in every case with a reversed sequence the sign taken from a sample of that sequence is the opposite one, and every
rest_then_move case comes forwards and backwards with opposite local_axis and the same scatter matrix to 1e-3 -- a kernel that reads
the NaN axis of sample 0, or none at all, gives both the sign of its eigen solver and is wrong for one.

No GPU, no kernel: every figure here comes from numpy."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import _joint_axes_edges as E  # noqa: E402
import _joints_ref as JR  # noqa: E402

COMPARED = tuple(E.SIZES) + E.REST_CASES + ("clean",) + E.BAD_CASES      # cases whose aggregates meet the restatement at tol


def moved(ref, j, var):
    """max |variant - restatement| over local_axis and local_pos[:3]; a variant without a sample has moved without bound."""
    if var["count"] == 0:
        return np.inf
    return max(np.abs(var["local_axis"] - ref["local_axis"][j]).max(), np.abs(var["local_pos"][:3] - ref["local_pos"][j, :3]).max())


def test_case_list_is_complete():
    assert set(E.ALL_CASES) == set(COMPARED) | {"below", "above", "on_the_line"}
    assert {E.SIZES[k][4] for k in E.SIZES} >= set(E.NS_TARGETS)
    assert any(E.SIZES[k][3] > 1 and E.SIZES[k][4] > E.NT for k in E.SIZES)


@pytest.mark.parametrize("name", E.ALL_CASES)
def test_sample_counts_hit_their_targets(name):
    from autourdf_amd import ops
    c = E.case(name)
    S, T = c["coords"].shape[:2]
    steps = JR.sample_steps(S, c["num_steps"], c["interval"])
    assert len(steps) == c["NS"] == ops.joint_samples(S, c["num_steps"], c["interval"]) <= E.MAX_SAMPLES
    assert c["num_steps"] <= T and E.reference(name)["sample_angle"].shape == (len(c["joints"]), c["NS"])
    if name in E.SIZES:
        assert c["NS"] == E.SIZES[name][4]
    if name == "ns296_interval4":
        assert (S, c["num_steps"], c["interval"], c["NS"]) == (1, 300, 4, 296)
    if name == "ns4096":
        assert len(c["joints"]) == 1 and c["NS"] == E.MAX_SAMPLES


def test_refused_neighbours():
    from autourdf_amd import ops
    for NS, (S, num_steps) in E.REFUSED.items():
        assert len(JR.sample_steps(S, num_steps, 1)) == NS == ops.joint_samples(S, num_steps, 1) > E.MAX_SAMPLES
    assert sorted(E.REFUSED) == [4097, 4098] and E.REFUSED[4097] == (1, 4098) and E.REFUSED[4098] == (2, 2050)


@pytest.mark.parametrize("name", E.ALL_CASES)
def test_no_angle_near_the_threshold(name):
    """No angle within a factor 1 +- 1e-6 of 2e-4, or a usable flag could flip on rounding; the threshold pair stands 1e-3 off,
    200 times the 1e-9 angle agreement the suite holds, on opposite sides."""
    ref = E.reference(name)
    th = ref["sample_angle"][np.isfinite(ref["sample_angle"])]
    assert not np.any((th > E.THETA_MIN * (1 - 1e-6)) & (th < E.THETA_MIN * (1 + 1e-6)))
    if name in ("below", "above"):
        want = E.THETA_MIN * (1 + E.THRESHOLD_MARGIN * (1 if name == "above" else -1))
        assert abs(th[0] - want) <= 1e-9 and E.THETA_MIN * E.THRESHOLD_MARGIN >= 100 * 1e-9
        assert bool(ref["sample_usable"][0, 0]) == (name == "above") and ref["count"][0] == (name == "above")
        assert np.isnan(ref["local_axis"][0]).all() == (name == "below") and np.isfinite(ref["first_pose"]).all()
    elif name in E.SIZES:
        assert ref["sample_usable"].all() and (ref["count"] == E.case(name)["NS"]).all()


@pytest.mark.parametrize("name", COMPARED + ("above", "on_the_line"))
def test_eigen_gap(name):
    ref = E.reference(name)
    for j in range(len(ref["count"])):
        w = E.scatter(ref["sample_axis"][j], ref["sample_usable"][j])[1]
        assert (w[2] - w[1]) / w[2] >= 0.9, (name, j, w)


@pytest.mark.parametrize("name", COMPARED)
def test_a_forgotten_wave_round_or_end_sample_moves_an_output(name):
    c, ref = E.case(name), E.reference(name)
    NS, floor = c["NS"], 100 * E.TOL
    for j in range(len(c["joints"])):
        usable = ref["sample_usable"][j]
        spans = [(a, a + E.WAVE) for a in range(0, NS, E.WAVE)] + [(a, a + E.NT) for a in range(0, NS, E.NT)]
        ends = np.flatnonzero(usable)[[0, -1]]
        spans += [(int(i), int(i) + 1) for i in ends]            # sample 0 and NS - 1, or the first and last usable one
        masks = [(f"samples {a}:{b}", (np.arange(NS) < a) | (np.arange(NS) >= b)) for a, b in spans]
        masks += [(f"partial of wave {w}", np.arange(NS) % E.NT // E.WAVE != w) for w in range(E.NT // E.WAVE)]
        for what, keep in masks:
            if not (usable & ~keep).any():
                continue                                         # only resting samples, or none at all: nothing to forget
            m = moved(ref, j, E.reaggregate(c, ref, j, keep=keep))
            assert m >= floor, (name, j, what, m)
        if name in E.SIZES:
            assert ends[0] == 0 and ends[1] == NS - 1


@pytest.mark.parametrize("name", [n for n in COMPARED if E.case(n)["reversed"] is not None])
def test_the_reversed_sequence_turns_the_other_way(name):
    """Every sample axis of the reversed sequence points against the first usable one, every other with it, so the alignment has
    work to do in every wave and round the sequence covers; and the sign taken from one of its samples is the wrong one."""
    c, ref = E.case(name), E.reference(name)
    S = c["coords"].shape[0]
    per = c["NS"] // S
    in_rev = np.arange(c["NS"]) // per == c["reversed"]
    for j in range(len(c["joints"])):
        use = ref["sample_usable"][j]
        dots = ref["sample_axis"][j] @ ref["sample_axis"][j, ref["first"][j]]
        assert (dots[use & in_rev] < -0.5).all() and (dots[use & ~in_rev] > 0.5).all(), (name, j)
        assert ref["local_axis"][j] @ ref["sample_axis"][j, ref["first"][j]] > 0.9
        wrong = int(np.flatnonzero(use & in_rev)[-1])
        assert moved(ref, j, E.reaggregate(c, ref, j, sign_from=wrong)) >= 1.0 >= 100 * E.TOL
    if name == "ns927":
        assert in_rev.sum() == 309 and (ref["sample_axis"][0] @ ref["sample_axis"][0, 0] < 0).sum() == 309
    if name == "ns4096":                                         # the reversed half covers rounds 8 .. 15, every wave of them
        assert in_rev[2048:].all() and not in_rev[:2048].any()


@pytest.mark.parametrize("n_rest", E.REST)
def test_rest_then_move_puts_the_first_usable_sample_where_it_says(n_rest):
    fwd, back = E.reference(f"rest{n_rest}"), E.reference(f"rest{n_rest}_back")
    c = E.case(f"rest{n_rest}")
    assert c["NS"] == n_rest + E.REST_MOVE - 2
    coords = c["coords"]
    assert all(coords[0, t].tobytes() == coords[0, 0].tobytes() for t in range(n_rest))
    f = n_rest - 1
    where = {70: (0, 1), 130: (0, 2), 200: (0, 3), 300: (1, 0), 520: (2, 0)}[n_rest]
    assert (f // E.NT, f % E.NT // E.WAVE) == where                 # (stride round, wave)
    for ref in (fwd, back):
        assert (ref["first"] == f).all() and (ref["count"] == E.REST_MOVE - 1).all()
        assert not ref["sample_usable"][:, :f].any() and ref["sample_usable"][:, f:].all()
        assert (ref["sample_angle"][:, :f] <= 1e-15).all()       # equal poses: 0 but for np.linalg.inv's rounding
        assert np.isnan(ref["sample_axis"][:, :f]).all() and np.isnan(ref["sample_point"][:, :f]).all()
    for j in range(4):
        # sample 0 is not the first usable one and has no axis; forwards and backwards, local_axis is opposite over the same scatter
        assert fwd["local_axis"][j] @ back["local_axis"][j] < -0.99
        Mf, Mb = (E.scatter(r["sample_axis"][j], r["sample_usable"][j])[0] for r in (fwd, back))
        assert np.abs(Mf - Mb).max() <= 1e-3 * (E.REST_MOVE - 1)


@pytest.mark.parametrize("name", E.BAD_CASES)
def test_non_finite_pose_costs_exactly_two_samples(name):
    c, ref, clean = E.case(name), E.reference(name), E.reference("clean")
    bad = E.bad_samples(c)
    assert bad == [274, 275] and all(E.NT <= i < 2 * E.NT for i in bad)      # stride round 1
    assert np.isfinite(np.delete(c["coords"].reshape(-1), np.flatnonzero(~np.isfinite(c["coords"].reshape(-1))))).all()
    assert (~np.isfinite(c["coords"])).sum() == 1 and E.BAD_CLUSTER in c["link_clusters"][E.BAD_LINK]
    assert len(c["link_clusters"][E.BAD_LINK]) == 3
    for j, pair in enumerate(c["joints"]):
        if E.BAD_LINK in pair:
            assert ref["count"][j] == clean["count"][j] - 2 == c["NS"] - 2
            assert list(np.flatnonzero(~ref["sample_usable"][j])) == bad
        else:
            for k in ("sample_axis", "sample_angle", "sample_point", "sample_usable") + E.OUTPUTS:
                assert ref[k][j].tobytes() == clean[k][j].tobytes()
    assert [j for j, pair in enumerate(c["joints"]) if E.BAD_LINK in pair] == [1, 3]   # once as the child, once as the parent


def test_on_the_line_takes_the_midpoint_branch():
    ref = E.reference("on_the_line")
    assert ref["midpoint"][0] and ref["count"][0] == 5 and ref["sample_usable"].all()
    np.testing.assert_array_equal(ref["local_axis"][0], [0.0, 0.0, 1.0])
    np.testing.assert_allclose(ref["global_pos"][0], [0.0, 0.0, 0.5 * (E.ON_LINE_PARENT_Z + E.ON_LINE_CHILD_Z)], rtol=0, atol=1e-15)
    assert np.isfinite(ref["local_pos"]).all()
    assert not any(E.reference(n)["midpoint"].any() for n in COMPARED)


def test_large_turns_take_the_far_branch():
    """Every sample of the large-turn case turns by more than 90 degrees: cos(theta) < 0, screw_axis' direction from the symmetric part."""
    ref = E.reference("large_turns")
    assert ref["sample_usable"].all() and (ref["sample_angle"] > 0.5 * np.pi + 0.1).all() and (ref["sample_angle"] < np.pi - 0.1).all()
