"""GPU: creg_joint_axes_f64 (k_joint_axes, csrc/joints.hip) past one wave, one stride round and at its limits, on the cases of
tests/_joint_axes_edges.py, whose own conditions tests/test_joint_axes_edges_cpu.py checks without a GPU: jittered trees and
two-link joints with 63 .. 4096 samples, a sequence reversed wherever there are two, so that every sample moves the aggregates
and the sign alignment has work in every wave and round; the first usable sample in waves 1 .. 3 and rounds 1 and 2; the
usable threshold from both sides; poses that are not finite; refine_position's midpoint branch; turns past 90 degrees.

Per sample the bounds are those of test_gpu_joints.py (1e-9), per joint E.TOL = 1e-9 against the restatement
_joint_axes_edges.joint_axes_ref; nothing here is measured from the kernel.  The maxima measured on an MI355X stand beside the
assertions in ``compare``.  Every test runs under its own watchdog, which ends the process: a hung kernel must not be waited on."""
import ctypes
import faulthandler
import functools
import os
import sys
import types

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import _joint_axes_edges as E  # noqa: E402
import _joints_ref as JR  # noqa: E402

pytestmark = pytest.mark.gpu

PER_SAMPLE = ("sample_axis", "sample_angle", "sample_point", "sample_usable")
EVERYTHING = PER_SAMPLE + E.OUTPUTS + ("count", "first_pose")
PAD, SENT = 64, -7


@pytest.fixture(autouse=True)
def _time_limit():
    faulthandler.dump_traceback_later(120, exit=True)
    yield
    faulthandler.cancel_dump_traceback_later()


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def run(c, joints=None):
    from autourdf_amd import ops
    out = ops.joint_axes(dev(c["coords"]), c["link_clusters"], c["joints"] if joints is None else joints, 0, c["num_steps"], c["interval"])
    return {k: v.cpu().numpy() for k, v in out.items()}


@functools.lru_cache(maxsize=None)
def got(name):
    return run(E.case(name))


def same_bits(a, b, keys=EVERYTHING, what=""):
    for k in keys:
        assert a[k].shape == b[k].shape and a[k].dtype == b[k].dtype and a[k].tobytes() == b[k].tobytes(), (what, k)


def compare(out, ref, what, angles_everywhere=True):
    """The kernel's outputs against the restatement's: per sample at 1e-9 with equal flags and NaN patterns, per joint at E.TOL,
    count exact, first_pose, and the sign convention.  Prints the maxima before it asserts."""
    use = ref["sample_usable"]
    J = len(ref["count"])
    top = {}
    for k in ("sample_axis", "sample_point"):
        top[k] = np.abs(out[k] - ref[k])[use].max(initial=0.0)
    known = np.isfinite(ref["sample_angle"])                     # all but the samples that touch a pose which is not finite
    top["sample_angle"] = np.abs(out["sample_angle"] - ref["sample_angle"])[known].max(initial=0.0)
    for k in E.OUTPUTS:
        diff = np.abs(out[k] - ref[k])
        top[k] = diff[np.isfinite(diff)].max(initial=0.0)
    fp = out["first_pose"].reshape(J, 2, 7)
    top["first_pose xyz"] = np.abs(fp[..., :3] - ref["first_pose"][..., :3]).max()
    sg = np.sign(np.sum(fp[..., 3:] * ref["first_pose"][..., 3:], axis=-1, keepdims=True))
    top["first_pose quat"] = np.abs(sg * fp[..., 3:] - ref["first_pose"][..., 3:]).max()
    print(f"{what}: max |kernel - restatement| " + ", ".join(f"{k} {v:.3g}" for k, v in top.items()))
    assert out["sample_usable"].dtype == np.bool_ and np.array_equal(out["sample_usable"], use), what
    for k in ("sample_axis", "sample_point"):
        assert np.array_equal(np.isnan(out[k]), np.isnan(ref[k])) and np.array_equal(np.isnan(out[k]).all(axis=-1), ~use), (what, k)
        assert top[k] <= 1e-9, (what, k, top[k])                 # measured: axis 5.0e-13 (ns4096), point 2.1e-13 (ns927)
    assert np.isfinite(out["sample_angle"][known]).all() and (known.all() or not angles_everywhere)
    assert top["sample_angle"] <= 1e-9, (what, top["sample_angle"])           # measured: 2.2e-15 (ns257)
    assert out["count"].dtype == np.int32 and np.array_equal(out["count"], ref["count"]), what
    assert np.array_equal(out["count"], use.sum(axis=1))
    assert top["first_pose xyz"] <= 1e-12 and top["first_pose quat"] <= 1e-9, what       # measured: 0 and 5.6e-16
    for k in E.OUTPUTS:
        assert np.array_equal(np.isnan(out[k]), np.isnan(ref[k])), (what, k)
        # measured over all cases: local_axis 1.0e-15, local_pos 5.7e-15, global_pos 5.8e-15 (ns65), global_axis 1.1e-15 (rest300_back);
        # at NS = 4096 4.4e-16, 6.7e-16, 6.7e-16, 4.4e-16.  All below 1e-10: the bound needs no further justification.
        assert top[k] <= E.TOL, (what, k, top[k])
    for j in range(J):
        if ref["count"][j]:
            f = int(np.argmax(out["sample_usable"][j]))
            assert f == ref["first"][j] and out["local_axis"][j] @ out["sample_axis"][j, f] > 0, (what, j)
    return top


# ================================================================================================ 1. sizes
@pytest.mark.parametrize("name", list(E.SIZES))
def test_sizes_against_the_restatement(name):
    """NS = 63, 64, 65 (one wave and its neighbours), 255, 256, 257 (one stride round), 296 at interval 4 and 511 at interval 2,
    513 (a third round of one sample), 927, 4096 (the limit: 16 rounds, one joint), and 66 samples that each turn by about 2 rad
    (cos < 0: screw_axis takes its direction from the symmetric part)."""
    c, out = E.case(name), got(name)
    assert out["sample_angle"].shape == (len(c["joints"]), c["NS"])
    compare(out, E.reference(name), name)
    assert out["sample_usable"].all()
    if name == "large_turns":
        assert (out["sample_angle"] > 0.5 * np.pi).all()


# ================================================================================================ 2. the first usable sample
@pytest.mark.parametrize("name", E.REST_CASES)
def test_first_usable_sample_in_a_later_wave_or_round(name):
    """The robot rests over the first n_rest steps: the first usable sample is n_rest - 1 = 69, 129, 199 (waves 1, 2, 3 of round 0),
    299 (round 1) and 519 (round 2), its owner thread another each time; forwards and backwards, which negates local_axis."""
    c, out, ref = E.case(name), got(name), E.reference(name)
    f = c["n_rest"] - 1
    assert not out["sample_usable"][:, :f].any() and out["sample_usable"][:, f:].all()
    assert np.isnan(out["sample_axis"][:, :f]).all() and np.isnan(out["sample_point"][:, :f]).all()
    assert (out["count"] == E.REST_MOVE - 1).all()
    compare(out, ref, name)
    if name.endswith("_back"):
        fwd = got(name[:-5])
        assert (np.sum(fwd["local_axis"] * out["local_axis"], axis=1) < -0.99).all()


# ================================================================================================ 3. the threshold
def test_threshold_pair():
    from autourdf_amd import compute_joints
    below, above = got("below"), got("above")
    compare(below, E.reference("below"), "below")
    compare(above, E.reference("above"), "above")
    assert not below["sample_usable"][0, 0] and below["count"][0] == 0
    assert all(np.isnan(below[k]).all() for k in E.OUTPUTS) and np.isfinite(below["first_pose"]).all()
    assert np.isnan(below["sample_axis"]).all() and np.isnan(below["sample_point"]).all() and np.isfinite(below["sample_angle"]).all()
    assert above["sample_usable"][0, 0] and above["count"][0] == 1 and all(np.isfinite(above[k]).all() for k in E.OUTPUTS)
    links = [{"id": 0, "parent_id": None, "cluster_idx": [0]}, {"id": 1, "parent_id": 0, "cluster_idx": [1]}]
    cms = lambda name: [types.SimpleNamespace(coords=x) for x in E.case(name)["coords"]]
    with pytest.raises(ValueError, match="no step turns the child"):
        compute_joints.estimate_joint_axes_from_tree(links, cms("below"), 0, 2, 1)
    jd = compute_joints.estimate_joint_axes_from_tree(links, cms("above"), 0, 2, 1)
    assert np.linalg.norm(np.cross(jd[0]["local_axis"], E.TWO_AXIS)) <= 1e-6


# ================================================================================================ 4. poses that are not finite
@pytest.mark.parametrize("name", E.BAD_CASES)
def test_a_pose_that_is_not_finite_costs_its_two_samples_and_nothing_else(name):
    """A NaN or an Inf in x or in a quaternion component of cluster 4 (one of link 2's three) at sequence 1, step 120 of 156:
    samples 274 and 275 (stride round 1) of joints (1, 2) and (2, 4) are unusable, every other sample keeps the clean run's bits,
    joints (0, 1) and (1, 3) keep all of theirs, and the aggregates meet the restatement without the two samples."""
    c, out, clean, ref = E.case(name), got(name), got("clean"), E.reference(name)
    bad = E.bad_samples(c)
    others = np.setdiff1d(np.arange(c["NS"]), bad)
    for j, pair in enumerate(c["joints"]):
        one = lambda d: {k: d[k][j] for k in EVERYTHING}
        if E.BAD_LINK not in pair:
            same_bits(one(out), one(clean), what=f"{name} joint {j}")
            continue
        assert not out["sample_usable"][j, bad].any() and out["sample_usable"][j, others].all()
        assert np.isnan(out["sample_axis"][j, bad]).all() and np.isnan(out["sample_point"][j, bad]).all()
        assert out["count"][j] == clean["count"][j] - 2 == c["NS"] - 2
        same_bits({k: out[k][j, others] for k in PER_SAMPLE}, {k: clean[k][j, others] for k in PER_SAMPLE}, PER_SAMPLE, f"{name} joint {j}")
        same_bits(one(out), one(clean), ("first_pose",))
    compare(out, ref, name, angles_everywhere=False)


# ================================================================================================ 5. the midpoint branch
def test_refine_position_when_both_links_stand_on_the_joint_line():
    out, ref = got("on_the_line"), E.reference("on_the_line")
    assert ref["midpoint"][0]
    compare(out, ref, "on_the_line")
    assert np.isfinite(out["global_pos"]).all() and np.isfinite(out["local_pos"]).all()
    np.testing.assert_allclose(out["global_pos"][0], [0.0, 0.0, 0.125], rtol=0, atol=1e-9)
    np.testing.assert_allclose(out["local_pos"][0], ref["local_pos"][0], rtol=0, atol=1e-9)


# ================================================================================================ 6. independence and bits
def test_a_joint_alone_among_four_and_300_times_has_the_same_bits():
    c, four = E.case("ns513"), got("ns513")
    same_bits(run(c), four, what="two runs")
    for j in (1, 3):
        one = {k: four[k][j:j + 1] for k in EVERYTHING}
        same_bits(run(c, [c["joints"][j]]), one, what=f"joint {j} alone")
        many = run(c, [c["joints"][j]] * 300)
        assert many["count"].shape == (300,)
        for k in EVERYTHING:
            assert many[k].tobytes() == np.repeat(one[k], 300, axis=0).tobytes(), (j, k)


# ================================================================================================ 7. the C ABI
def _ptr(t):
    return None if t is None else ctypes.c_void_p(t.data_ptr())


def _abi(c, J, first_pose=True):
    """creg_joint_axes_f64 on sentinel-filled buffers with PAD spare rows behind every output -> (rc, buffers, rows)."""
    from autourdf_amd import _lib
    lib = _lib.load()
    S, T, K = c["coords"].shape[:3]
    NS = lib.creg_joint_axes_samples(S, c["num_steps"], c["interval"])
    flat = [k for l in c["link_clusters"] for k in l]
    off = np.concatenate([[0], np.cumsum([len(l) for l in c["link_clusters"]])])
    i32 = lambda a: dev(np.asarray(a, np.int32))
    coords, cl, lo, jn = dev(c["coords"]), i32(flat), i32(off), i32(c["joints"][:J])
    full = lambda rows, tail, dt: torch.full((rows + PAD,) + tail, SENT, dtype=dt, device="cuda")
    f64, rows = torch.float64, min(J * NS, J * 300)                 # a refused call gets buffers it must leave alone
    bufs = {"sample_axis": full(rows, (3,), f64), "sample_angle": full(rows, (), f64), "sample_point": full(rows, (3,), f64),
            "sample_usable": full(rows, (), torch.int32), "local_axis": full(J, (3,), f64), "local_pos": full(J, (4,), f64),
            "global_pos": full(J, (3,), f64), "global_axis": full(J, (3,), f64), "count": full(J, (), torch.int32),
            "first_pose": full(J, (2, 7), f64) if first_pose else None}
    rc = lib.creg_joint_axes_f64(_ptr(coords), S, T, K, _ptr(cl), _ptr(lo), len(flat), _ptr(jn), J, 0, c["num_steps"], c["interval"],
                                 *[_ptr(bufs[k]) for k in EVERYTHING], None)
    torch.cuda.synchronize()
    return rc, {k: v for k, v in bufs.items() if v is not None}, {k: (rows if k in PER_SAMPLE else J) for k in bufs}


def test_every_output_row_is_written_and_nothing_beyond():
    """J = 3, NS = 257: every row of (J, NS) and of (J) is written, the 64 rows behind each are not; first_pose may be NULL."""
    c = E.case("ns257")
    J, NS = 3, 257
    want = run(c, c["joints"][:J])
    for first_pose in (True, False):
        rc, bufs, rows = _abi(c, J, first_pose)
        assert rc == 0 and ("first_pose" in bufs) == first_pose and rows["sample_axis"] == J * NS
        for k, b in bufs.items():
            n = rows[k]
            assert bool((b[n:] == SENT).all()), (k, "rows behind the output were written")
            written = b[:n].reshape(n, -1)
            assert bool((written != SENT).any(dim=1).all()), (k, "a row was not written")
            got_k = b[:n].cpu().numpy().reshape(want[k].shape)
            assert (got_k != 0 if k == "sample_usable" else got_k).tobytes() == want[k].tobytes(), k


# ================================================================================================ 8. the limits
@pytest.mark.parametrize("NS", sorted(E.REFUSED))
def test_one_sample_too_many_is_refused_before_anything_is_written(NS):
    from autourdf_amd import _lib, ops
    S, num_steps = E.REFUSED[NS]
    coords = np.zeros((S, num_steps, 2, 7))
    coords[..., 3] = 1.0
    with pytest.raises(ValueError, match=f"{NS} samples"):
        ops.joint_axes(dev(coords), E.TWO_LINKS, E.TWO_JOINT, 0, num_steps, 1)
    c = {"coords": coords, "link_clusters": E.TWO_LINKS, "joints": E.TWO_JOINT, "num_steps": num_steps, "interval": 1}
    rc, bufs, _ = _abi(c, 1)
    assert rc == -1
    msg = _lib.load().creg_last_error().decode()
    assert "creg_joint_axes_f64" in msg and f"{NS} samples" in msg and str(E.MAX_SAMPLES) in msg, msg
    for k, b in bufs.items():
        assert bool((b == SENT).all()), (k, "a refused call wrote")


def test_sample_count_over_a_grid():
    from autourdf_amd import _lib
    count = _lib.load().creg_joint_axes_samples
    for S in range(1, 5):
        for num_steps in range(1, 41):
            for interval in range(1, 10):
                assert count(S, num_steps, interval) == len(JR.sample_steps(S, num_steps, interval)), (S, num_steps, interval)
    assert count(2, 5, 9) == 0 and count(1, 1, 1) == 0                       # interval > num_steps: no phase has two steps
    for bad in ((0, 5, 1), (2, 0, 1), (2, 5, 0), (-1, 5, 1), (2, -3, 1), (2, 5, -2)):
        assert count(*bad) == 0, bad
    assert count(2, 2049, 1) == E.MAX_SAMPLES
