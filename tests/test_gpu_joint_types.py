"""Prismatic and fixed joints on the GPU: creg_joint_types_f64 and creg_joint_slides_f64 through ops against the numpy
restatement of their contracts (tests/_joint_types_ref.py) on the typed synthetic tree; the thresholds at their edges;
estimate_typed_joints_from_tree / create_urdf / estimate_joint_motion / set_joint_limits / replay_urdf end to end."""
import functools
import os
import sys
import types

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu
HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import _joint_motion_ref as M  # noqa: E402
import _joint_types_ref as JT  # noqa: E402

SUMMARY = ("lower", "upper", "tilt_rms", "tilt_max", "slip_rms", "slip_max")
OUTPUTS = ("sample_angle", "sample_slide", "sample_kind", "counts", "type", "slide_axis", "global_axis", "global_pos")
ALL_REVOLUTE = ("revolute",) * 4


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available()
    return torch.device("cuda")


@functools.lru_cache(maxsize=None)
def _tree(T, kinds=tuple(JT.TREE_TYPES), root_moves=True):
    """The typed tree with three sequences of T steps and its coordinates on the device (computed once)."""
    t = JT.typed_tree(S=3, T=T, types=list(kinds), root_moves=root_moves)
    t["coords_dev"] = torch.from_numpy(t["coords"]).cuda()
    return t


@functools.lru_cache(maxsize=None)
def _poses(T):
    from autourdf_amd import ops
    t = _tree(T)
    return M.link_poses(t["coords"], t["link_clusters"]), ops.link_poses(t["coords_dev"], t["link_clusters"])


def _np(out):
    return {k: v.cpu().numpy() for k, v in out.items()}


def _same_bits(a, b, keys=OUTPUTS, rows=slice(None)):
    for k in keys:
        assert a[k][rows].tobytes() == b[k][rows].tobytes(), k


# ------------------------------------------------------------------------------------------------ joint types
@pytest.mark.parametrize("S", [1, 3])
@pytest.mark.parametrize("num_steps,interval", [(2, 1), (5, 4), (66, 1), (301, 1), (3, 4), (1, 1)])   # the last two: no sample
def test_joint_types_vs_restatement(dev, S, num_steps, interval):
    from autourdf_amd import ops
    t = _tree(20 if num_steps <= 5 else 310)
    args = (t["link_clusters"], t["joints"], 2, num_steps, interval)
    got = _np(ops.joint_types(t["coords_dev"][:S].contiguous(), *args, JT.TURN_MIN, JT.SLIDE_MIN))
    ref = JT.joint_types(t["coords"][:S], *args, JT.TURN_MIN, JT.SLIDE_MIN)
    NS = ops.joint_samples(S, num_steps, interval)
    assert NS == ref["sample_kind"].shape[1] and (NS == 0) == ((num_steps, interval) in ((3, 4), (1, 1)))
    assert got["sample_angle"].shape == (4, NS) and got["sample_slide"].shape == (4, NS, 3) and got["sample_kind"].shape == (4, NS)
    assert got["sample_kind"].dtype == np.int32 and got["counts"].dtype == np.int32 and got["type"].dtype == np.int32
    assert JT.separation(ref)                                                 # or a kind could flip on rounding
    assert np.array_equal(got["sample_kind"], ref["sample_kind"]) and np.array_equal(got["counts"], ref["counts"])
    assert np.array_equal(got["type"], ref["type"])
    assert got["type"].tolist() == ([-1] * 4 if NS == 0 else [JT.KINDS[k] for k in t["types"]])
    for k in ("sample_angle", "sample_slide", "slide_axis", "global_axis", "global_pos"):
        assert np.array_equal(np.isnan(got[k]), np.isnan(ref[k])), k
        np.testing.assert_allclose(got[k], ref[k], rtol=0, atol=1e-8, err_msg=k)
    if NS:
        assert np.abs(got["slide_axis"][JT.PRISMATIC] - t["axes"][JT.PRISMATIC]).max() <= 1e-9
        assert got["sample_angle"][JT.PRISMATIC].max() <= 1e-6               # the prismatic joint's rotation residue
        print(f"S={S} num_steps={num_steps} interval={interval}: max |kernel - restatement| angle "
              f"{np.abs(got['sample_angle'] - ref['sample_angle']).max():.3g}, slide "
              f"{np.abs(got['sample_slide'] - ref['sample_slide']).max():.3g}, axis "
              f"{np.nanmax(np.abs(got['slide_axis'] - ref['slide_axis'])):.3g}")
    else:
        assert got["counts"].tolist() == [[0] * 4] * 4 and np.isnan(got["slide_axis"]).all() and np.isnan(got["global_axis"]).all()
    # the angle is creg_joint_axes_f64's, bit for bit
    axes = ops.joint_axes(t["coords_dev"][:S].contiguous(), *args)
    assert got["sample_angle"].tobytes() == axes["sample_angle"].cpu().numpy().tobytes()
    if NS:
        assert np.array_equal(axes["count"].cpu().numpy() > 0, got["type"] == 1)


def test_thresholds_at_their_edges(dev):
    from autourdf_amd import ops
    t = _tree(20)
    run = lambda **kw: _np(ops.joint_types(t["coords_dev"], t["link_clusters"], t["joints"], 0, 20, 4,
                                           **{"turn_min": JT.TURN_MIN, "slide_min": JT.SLIDE_MIN, **kw}))
    base = run()
    j, i = 0, 5                                                               # a turning sample of the first revolute joint
    theta = float(base["sample_angle"][j, i])
    assert base["sample_kind"][j, i] == 1
    assert run(turn_min=theta)["sample_kind"][j, i] == 1                      # theta >= turn_min
    assert run(turn_min=float(np.nextafter(theta, np.inf)))["sample_kind"][j, i] == 2
    j = JT.PRISMATIC
    length = JT.norm3(base["sample_slide"][j, i])                             # |t| as the contract states it, on the kernel's t
    assert base["sample_kind"][j, i] == 2
    below, above = float(np.nextafter(length, 0.0)), float(np.nextafter(length, np.inf))
    assert run(slide_min=below)["sample_kind"][j, i] == 2                     # the outer two hold even if the host is an ulp off
    assert run(slide_min=float(np.nextafter(above, np.inf)))["sample_kind"][j, i] == 0
    exact = run(slide_min=length)["sample_kind"][j, i] == 2 and run(slide_min=above)["sample_kind"][j, i] == 0
    print(f"theta {theta!r}, |t| {length!r}: the host's |t| is " + ("the kernel's" if exact else "one ulp off the kernel's"))
    with pytest.raises(ValueError):
        run(slide_min=None)
    with pytest.raises(ValueError):
        run(turn_min=-1.0)
    with pytest.raises(ValueError):
        run(slide_min=float("inf"))


def _two_links(turn_at=None, slide=0.01):
    """One joint between two single-cluster links over six steps: the parent rests, the child slides by ``slide`` per step and,
    from step ``turn_at`` on, stands turned by 1e-3 rad about its own origin -- one turning sample among slides."""
    coords = np.zeros((1, 6, 2, 7))
    axis = np.array([0.6, 0.0, 0.8])
    for i in range(6):
        C = np.eye(4)
        C[:3, 3] = [0.1, 0.2, 0.3] + axis * slide * i
        if turn_at is not None and i >= turn_at:
            C[:3, :3] = M.JR.rotation([0.0, 1.0, 0.0], 1e-3)
        coords[0, i, 0] = M._pose_row(np.eye(4), 1.0)
        coords[0, i, 1] = M._pose_row(C, -1.0 if i % 2 else 1.0)
    return coords, axis


def test_priority_of_the_kinds(dev):
    from autourdf_amd import ops
    coords, axis = _two_links(turn_at=3)
    run = lambda c, **kw: _np(ops.joint_types(torch.from_numpy(c).to(dev), [[0], [1]], [(0, 1)], 0, 6, 1, **kw))
    got = run(coords, turn_min=JT.TURN_MIN, slide_min=JT.SLIDE_MIN)
    assert got["sample_kind"].tolist() == [[2, 2, 1, 2, 2]] and got["counts"].tolist() == [[0, 1, 4, 0]]
    assert got["type"].tolist() == [1]                                        # one turn outweighs four slides
    got = run(coords, turn_min=1e-2, slide_min=JT.SLIDE_MIN)                   # above that turn: all slides
    assert got["sample_kind"].tolist() == [[2] * 5] and got["type"].tolist() == [2]
    # the turned child frame sees the slide direction turned back: the axis follows the majority within 1e-3
    assert np.abs(got["slide_axis"][0] - axis).max() <= 1e-3 and abs(np.linalg.norm(got["slide_axis"][0]) - 1.0) <= 1e-12
    got = run(coords, turn_min=1e-2, slide_min=1.0)                            # below both thresholds: fixed
    assert got["sample_kind"].tolist() == [[0] * 5] and got["counts"].tolist() == [[5, 0, 0, 0]] and got["type"].tolist() == [0]
    assert np.isnan(got["slide_axis"]).all() and np.isnan(got["global_axis"]).all()
    assert got["global_pos"][0].tolist() == [float(np.float32(x)) for x in (0.1, 0.2, 0.3)]
    # the sign: the first slide sample's t has a non-negative product with the axis, whichever way the child slides
    back, _ = _two_links(slide=-0.01)
    got = run(back, turn_min=JT.TURN_MIN, slide_min=JT.SLIDE_MIN)
    assert got["type"].tolist() == [2] and np.abs(got["slide_axis"][0] + axis).max() <= 1e-9
    assert got["sample_slide"][0, 0] @ got["slide_axis"][0] > 0.0


def test_a_non_finite_cluster_pose_costs_only_the_samples_it_reaches(dev):
    from autourdf_amd import ops
    t = _tree(20)
    args = (t["link_clusters"], t["joints"], 0, 20, 4, JT.TURN_MIN, JT.SLIDE_MIN)
    clean = _np(ops.joint_types(t["coords_dev"], *args))
    coords = t["coords"].copy()
    coords[1, 8, 7, 0] = np.nan                                               # cluster 7 is link 4: joint (2, 4), sequence 1, step 8
    got = _np(ops.joint_types(torch.from_numpy(coords).to(dev), *args))
    ref = JT.joint_types(coords, *args)
    assert np.array_equal(got["sample_kind"], ref["sample_kind"]) and np.array_equal(got["counts"], ref["counts"])
    bad = np.argwhere(got["sample_kind"] == -1).tolist()
    assert bad == [[3, 16 + 1], [3, 16 + 2]]                                   # samples (4, 8) and (8, 12) of sequence 1, phase 0
    assert got["counts"][3].tolist() == [0, 46, 0, 2] and got["type"].tolist() == clean["type"].tolist()
    _same_bits(got, clean, rows=slice(0, 3))                                  # the joints that do not touch link 4
    keep = np.ones(48, bool)
    keep[[17, 18]] = False
    for k in ("sample_angle", "sample_slide", "sample_kind"):
        assert got[k][3][keep].tobytes() == clean[k][3][keep].tobytes(), k


def test_joint_types_bits_repeat_and_do_not_depend_on_the_other_joints(dev):
    from autourdf_amd import ops
    t = _tree(310)
    args = (2, 301, 1, JT.TURN_MIN, JT.SLIDE_MIN)
    a = _np(ops.joint_types(t["coords_dev"], t["link_clusters"], t["joints"], *args))
    b = _np(ops.joint_types(t["coords_dev"], t["link_clusters"], t["joints"], *args))
    _same_bits(a, b)
    for j in range(4):
        alone = _np(ops.joint_types(t["coords_dev"], t["link_clusters"], t["joints"][j:j + 1], *args))
        for k in OUTPUTS:
            assert alone[k][0].tobytes() == a[k][j].tobytes(), (j, k)
    out = ops.joint_types(t["coords_dev"], t["link_clusters"], [], *args)      # no joint: no launch
    assert out["type"].shape == (0,) and out["sample_slide"].shape == (0, 900, 3) and out["counts"].shape == (0, 4)
    torch.cuda.synchronize()
    for bad in (dict(joints=[(0, 5)]), dict(link_clusters=[[0], []]), dict(link_clusters=[[0], [8]])):
        with pytest.raises(ValueError):
            ops.joint_types(t["coords_dev"], bad.get("link_clusters", t["link_clusters"]), bad.get("joints", t["joints"]), *args)
    with pytest.raises(IndexError):
        ops.joint_types(t["coords_dev"], t["link_clusters"], t["joints"], 10, 301, 1, JT.TURN_MIN, JT.SLIDE_MIN)
    with pytest.raises(ValueError):                                           # 3 x 1500 samples per joint
        ops.joint_types(torch.zeros(3, 1501, 8, 7, dtype=torch.float64, device=dev), t["link_clusters"], t["joints"], 0, 1501, 1,
                        JT.TURN_MIN, JT.SLIDE_MIN)
    with pytest.raises(TypeError):
        ops.joint_types(t["coords_dev"].float(), t["link_clusters"], t["joints"], *args)


# ------------------------------------------------------------------------------------------------ joint slides
def _slide_axes(t):
    return np.where(np.array(t["types"])[:, None] == "prismatic", t["axes"], 0.0)


@pytest.mark.parametrize("S", [1, 3])
@pytest.mark.parametrize("num_steps", [1, 2, 70, 300])                       # 70 crosses a wave, 300 the 256-thread stride
@pytest.mark.parametrize("ref_inside", [True, False])
def test_joint_slides_vs_restatement(dev, S, num_steps, ref_inside):
    from autourdf_amd import ops
    T = 20 if num_steps <= 2 else 310
    t, (link_T, link_T_dev) = _tree(T), _poses(T)
    start = 3
    ref_step = start + num_steps // 2 if ref_inside else T - 1
    joints, axes = t["joints"][1:3], _slide_axes(t)[1:3]                       # the prismatic and the fixed joint
    got = _np(ops.joint_slides(link_T_dev[:S].contiguous(), joints, axes, 0, ref_step, start, num_steps))
    ref = JT.joint_slides(link_T[:S], joints, axes, 0, ref_step, start, num_steps)
    assert got["q"].shape == (2, S, num_steps) and got["lower_at"].shape == (2, 2) and got["n_used"].dtype == np.int32
    for k in ("q", "tilt", "slip") + SUMMARY:
        np.testing.assert_allclose(got[k], ref[k], rtol=0, atol=1e-8, err_msg=k)
    assert got["n_used"].tolist() == [S * num_steps] * 2
    q_true = t["q_true"][JT.PRISMATIC]
    assert np.abs(got["q"][0] - (q_true[:S, start:start + num_steps] - q_true[0, ref_step])).max() <= 1e-9
    assert np.all(got["q"][1] == 0.0)                                         # the fixed joint: a zero axis
    assert got["tilt_max"].max() <= 1e-9 and got["slip_max"].max() <= 1e-9    # exact kinematics: nothing is left over
    u = np.sort(ref["q"][0].reshape(-1))
    if len(u) > 1 and u[1] - u[0] > 1e-6 and u[-1] - u[-2] > 1e-6:            # an extreme within rounding of the runner-up names no sample
        assert got["lower_at"][0].tolist() == ref["lower_at"][0].tolist() and got["upper_at"][0].tolist() == ref["upper_at"][0].tolist()


def test_joint_slides_tell_a_revolute_joint_and_repeat_their_bits(dev):
    from autourdf_amd import ops
    t, (link_T, lt) = _tree(310), _poses(310)
    axes = _slide_axes(t)
    axes[0] = t["axes"][0]                                                    # the first revolute joint, read as a slide
    a = _np(ops.joint_slides(lt, t["joints"][:3], axes[:3], 0, 5, 2, 300))
    assert a["tilt_max"][0] >= 0.5 and a["tilt_max"][1] <= 1e-9 and a["tilt_max"][2] <= 1e-9   # the residual tells the kinds apart
    b = _np(ops.joint_slides(lt, t["joints"][:3], axes[:3], 0, 5, 2, 300))
    _same_bits(a, b, keys=tuple(a))
    for j in range(3):
        alone = _np(ops.joint_slides(lt, t["joints"][j:j + 1], axes[j:j + 1], 0, 5, 2, 300))
        for k in a:
            assert alone[k][0].tobytes() == a[k][j].tobytes(), (j, k)


def test_joint_slides_without_joints_and_refusals(dev):
    from autourdf_amd import ops
    t, (_, lt) = _tree(20), _poses(20)
    out = ops.joint_slides(lt, [], np.zeros((0, 3)), 0, 0, 0, 10)
    assert out["q"].shape == (0, 3, 10) and out["lower"].shape == (0,) and out["lower_at"].shape == (0, 2)
    torch.cuda.synchronize()
    args = (t["joints"], _slide_axes(t))
    for bad in ((0, 0, 0, 21), (0, 0, 18, 3), (3, 0, 0, 5), (0, 20, 0, 5), (-1, 0, 0, 5)):
        with pytest.raises(IndexError):
            ops.joint_slides(lt, *args, *bad)
    with pytest.raises(ValueError):
        ops.joint_slides(lt, [(0, 5)], np.zeros((1, 3)))
    with pytest.raises(ValueError):
        ops.joint_slides(lt, t["joints"], np.zeros((3, 3)))
    with pytest.raises(ValueError):
        ops.joint_slides(lt, *args, 0, 0, 0, 0)
    with pytest.raises(TypeError):
        ops.joint_slides(lt.float(), *args)


def test_refusals_of_the_five_wrappers_keep_their_words(dev):
    """One fault per call on the typed tree (S=3, T=20, K=8, L=5, J=4): the exception's type and its whole text, as they were
    before the wrappers shared their checks.  Every call raises before any launch."""
    from autourdf_amd import ops
    t, (_, lt) = _tree(20), _poses(20)
    c, cl, jt = t["coords_dev"], t["link_clusters"], t["joints"]
    ax, lp = np.zeros((4, 3)), np.zeros((4, 4))
    past = [list(x) for x in cl[:4]] + [[8]]                                  # link 4 names cluster K
    empty = [list(x) for x in cl[:3]] + [[]] + [list(cl[4])]
    wide = torch.zeros(1, 2, 257, 7, dtype=torch.float64, device=dev)
    f32 = "must be torch.float64, got torch.float32"
    table = []
    for name, fn, more in (("joint_axes", ops.joint_axes, {}), ("joint_types", ops.joint_types, {"slide_min": 1e-6})):
        table += [
            (fn, (c, cl, jt, 0, 21, 1), more, IndexError, "index 20 is out of bounds for axis 0 with size 20"),
            (fn, (c, cl, [(0, 5)], 0, 20, 1), more, ValueError, f"{name}: joint (0, 5) names a link outside [0, 5)"),
            (fn, (c, past, jt, 0, 20, 1), more, ValueError, f"{name}: link 4 names clusters [8] outside [0, 8)"),
            (fn, (c, empty, jt, 0, 20, 1), more, ValueError, f"{name}: link 3 has no cluster"),
            (fn, (wide, cl, jt, 0, 2, 1), more, ValueError, f"{name} supports at most 256 clusters, got 257"),
            (fn, (c, cl, jt, 0, 0, 1), more, ValueError,
             f"{name}: need start_step >= 0, num_steps >= 1, interval >= 1 (got 0, 0, 1)"),
            (fn, (c.float(), cl, jt, 0, 20, 1), more, TypeError, "coords " + f32)]
    table += [
        (ops.link_poses, (c, past), {}, ValueError, "link_poses: link 4 names clusters [8] outside [0, 8)"),
        (ops.link_poses, (c, empty), {}, ValueError, "link_poses: link 3 has no cluster"),
        (ops.link_poses, (wide, cl), {}, ValueError, "link_poses supports at most 256 clusters, got 257"),
        (ops.link_poses, (c.float(), cl), {}, TypeError, "coords " + f32),
        (ops.joint_positions, (lt, jt, np.zeros((3, 3)), lp), {}, ValueError,
         "joint_positions: local_axis must be (4,3) and local_pos (4,3) or (4,4), got (3, 3) and (4, 4)"),
        (ops.joint_positions, (lt, jt, ax, np.zeros((4, 5))), {}, ValueError,
         "joint_positions: local_axis must be (4,3) and local_pos (4,3) or (4,4), got (4, 3) and (4, 5)"),
        (ops.joint_slides, (lt, jt, np.zeros((3, 3))), {}, ValueError, "joint_slides: local_axis must be (4,3), got (3, 3)")]
    for name, fn, rest in (("joint_positions", ops.joint_positions, (lp,)), ("joint_slides", ops.joint_slides, ())):
        one = tuple(x[:1] for x in (ax,) + rest)
        table += [
            (fn, (lt, jt, ax, *rest, 0, 0, 0, 21), {}, IndexError, "index 20 is out of bounds for axis 1 with size 20"),
            (fn, (lt, jt, ax, *rest, 3, 0, 0, 5), {}, IndexError, "index 3 is out of bounds for axis 0 with size 3"),
            (fn, (lt, jt, ax, *rest, 0, 20, 0, 5), {}, IndexError, "index 20 is out of bounds for axis 1 with size 20"),
            (fn, (lt, [(0, 5)], *one), {}, ValueError, f"{name}: joint (0, 5) names a link outside [0, 5)"),
            (fn, (lt, jt, ax, *rest, 0, 0, 0, 0), {}, ValueError, f"{name}: need start_step >= 0 and num_steps >= 1 (got 0, 0)"),
            (fn, (lt.float(), jt, ax, *rest), {}, TypeError, "link_T " + f32)]
    assert len(table) == 33
    for fn, args, more, kind, text in table:
        with pytest.raises(kind) as e:
            fn(*args, **more)
        assert type(e.value) is kind and str(e.value) == text, (fn.__name__, str(e.value), text)


# ------------------------------------------------------------------------------------------------ end to end
def _replay_worst(replay):
    return max(r["rot_max"] for r in replay), max(r["pos_max"] for r in replay)


def test_typed_joints_end_to_end(dev, tmp_path):
    from autourdf_amd import compute_joints
    from autourdf_amd.sim_data import UrdfRobot
    T = 20
    # the control: the same tree with four revolute joints through the unchanged path, under the same bound
    # (the replay holds the URDF's root still, so both trees keep theirs at rest)
    c = _tree(T, ALL_REVOLUTE, root_moves=False)
    cms = [types.SimpleNamespace(coords=x) for x in c["coords"]]
    jd = compute_joints.estimate_joint_axes_from_tree(c["links"], cms, 0, T, 4)
    path = str(tmp_path / "control.urdf")
    compute_joints.create_urdf(c["links"], jd, cms[0], path, "mesh/dir")
    motion = compute_joints.estimate_joint_motion(c["links"], jd, cms, 0, T)
    assert all("type" not in m and "unit" not in m for m in motion)
    compute_joints.set_joint_limits(path, motion)
    rot_max, pos_max = _replay_worst(compute_joints.replay_urdf(path, c["links"], motion, cms, 0, T))
    print(f"replay on the all-revolute control: rot_max {rot_max:.3g} rad, pos_max {pos_max:.3g}")
    assert rot_max <= 1e-5 and pos_max <= 1e-5 * 0.9                          # the bound of the fixture-a replay
    # the typed tree
    t = _tree(T, root_moves=False)
    cms = [types.SimpleNamespace(coords=x) for x in t["coords"]]
    with pytest.raises(ValueError, match="no step turns"):
        compute_joints.estimate_joint_axes_from_tree(t["links"], cms, 0, T, 4)
    with pytest.raises(ValueError, match="slide_min"):
        compute_joints.estimate_typed_joints_from_tree(t["links"], cms, 0, T, 4)
    jd = compute_joints.estimate_typed_joints_from_tree(t["links"], cms, 0, T, 4, slide_min=JT.SLIDE_MIN)
    assert [j["type"] for j in jd] == t["types"] and [(j["parent_link"], j["child_link"]) for j in jd] == t["joints"]
    assert [j["counts"] for j in jd] == [[0, 48, 0, 0], [0, 0, 48, 0], [48, 0, 0, 0], [0, 48, 0, 0]]
    p, f = jd[JT.PRISMATIC], jd[JT.FIXED]
    assert np.abs(p["local_axis"] - t["axes"][JT.PRISMATIC]).max() <= 1e-9 and np.abs(p["global_axis"] - t["axes"][JT.PRISMATIC]).max() <= 1e-9
    assert p["local_pos"].tolist() == [0.0, 0.0, 0.0, 1.0] and f["local_pos"].tolist() == [0.0, 0.0, 0.0, 1.0]
    assert np.isnan(f["local_axis"]).all() and np.isnan(f["global_axis"]).all() and np.isfinite(f["global_pos"]).all()
    # a revolute joint's entries are estimate_joint_axes_from_tree's, bit for bit: the tree without its other two joints
    sub = [l for l in t["links"] if l["id"] in (0, 1)]
    (plain,) = compute_joints.estimate_joint_axes_from_tree(sub, cms, 0, T, 4)
    for k in ("local_axis", "local_pos", "global_pos", "global_axis"):
        assert np.asarray(plain[k]).tobytes() == np.asarray(jd[0][k]).tobytes(), k
    path = str(tmp_path / "typed.urdf")
    compute_joints.create_urdf(t["links"], jd, cms[0], path, "mesh/dir")
    motion = compute_joints.estimate_joint_motion(t["links"], jd, cms, 0, T)
    assert [(m["type"], m["unit"]) for m in motion] == [("revolute", "rad"), ("prismatic", "length"), ("fixed", None), ("revolute", "rad")]
    assert [(m["parent_link"], m["child_link"]) for m in motion] == t["joints"] and all(m["n_used"] == 3 * T for m in motion)
    for j, m in enumerate(motion):
        assert m["positions"].shape == (3, T)
        assert np.abs(m["positions"] - t["q_true"][j]).max() <= 1e-9          # every joint stands at 0 at sequence 0, step 0
        assert m["tilt_max"] <= 1e-9 and m["slip_max"] <= 1e-9
    compute_joints.set_joint_limits(path, motion, pad=0.05)
    by_name = {j["name"]: j for j in UrdfRobot(path, load_meshes=False).joints}
    assert [by_name[f"joint_{c_}"]["type"] for _, c_ in t["joints"]] == t["types"]
    slide = motion[JT.PRISMATIC]
    assert by_name["joint_2"]["limit"] == [min(slide["lower"], 0.0), max(slide["upper"], 0.0)]   # the observed range, no pad
    assert by_name["joint_2"]["limit"][0] <= 0.0 <= by_name["joint_2"]["limit"][1]
    assert abs(by_name["joint_2"]["limit"][1] - t["q_true"][JT.PRISMATIC].max()) <= 1e-9
    assert by_name["joint_1"]["limit"] == [min(motion[0]["lower"] - 0.05, 0.0), max(motion[0]["upper"] + 0.05, 0.0)]
    replay = compute_joints.replay_urdf(path, t["links"], motion, cms, 0, T)
    assert [r["link"] for r in replay] == [l["id"] for l in t["links"]] and all(r["n_used"] == 3 * T for r in replay)
    rot_max, pos_max = _replay_worst(replay)
    print(f"replay on the typed tree: rot_max {rot_max:.3g} rad, pos_max {pos_max:.3g}")
    assert rot_max <= 1e-5 and pos_max <= 1e-5 * 0.9


# ------------------------------------------------------------------------------------------------ the command line
def _layout(tmp_path, tree, robot, cams, step):
    """A data directory as the command line expects it, built from the typed tree: registered sequences (the clusters' poses,
    one small cloud per cluster, the same in every frame), their raw frames, parameters.json."""
    import json
    from _ply import write_ascii_ply
    S, T, K = tree["coords"].shape[:3]
    (tmp_path / "parameters.json").write_text(json.dumps({robot: {"num_seg": K, "dof": len(tree["joints"])}}))
    rng = np.random.default_rng(0)
    clouds = {str(k): rng.normal(scale=0.02, size=(16, 3)).astype(np.float32) for k in range(K)}
    for s in range(S):
        part = tmp_path / f"data/part/{robot}_{K}_seg/{step}_deg_{cams}_cams/seq{s}"
        (part / "matrix").mkdir(parents=True)
        (part / "cluster").mkdir()
        for t in range(T):
            np.save(part / f"matrix/{t:04}.npy", np.array([M.JR.pose_matrix(c[:3], c[3:]) for c in tree["coords"][s, t]]))
            np.savez(part / f"cluster/{t:04}.npz", **clouds)
            raw = tmp_path / f"data/raw/{robot}/{step}_deg_{cams}_cams/seq{s}/{t:04}"
            raw.mkdir(parents=True)
            write_ascii_ply(str(raw / "robot.ply"), np.vstack([rng.uniform(-0.5, 0.5, size=(62, 3)), [[-0.5] * 3, [0.5] * 3]]))


@pytest.mark.filterwarnings("ignore:autourdf_amd.prefer_device_kernargs")     # main() in this process: the runtime is up already
def test_command_line_joint_types(dev, tmp_path, monkeypatch, capsys):
    """main() in this process on the typed tree's data.  Link discovery groups clusters by how they move, so on exact data it
    can never split the fixed link from its parent: the tree's own links stand in for coord_clustering and kinematics_tree, and
    everything after them -- the flags, the typed joints, the link clouds, the URDF, the limits, the replay, the report -- runs as
    the command runs it."""
    import json
    import xml.etree.ElementTree as ET
    from autourdf_amd import coord_map
    robot, cams, step, T = "typedbot", 20, 4, 10
    tree = JT.typed_tree(S=2, T=T, root_moves=False)
    _layout(tmp_path, tree, robot, cams, step)
    components = [set(c) for c in tree["link_clusters"]]
    g1 = coord_map.Graph()
    g1.add_nodes_from(range(8))
    g1.add_edges_from((c[0], k) for c in tree["link_clusters"] for k in c[1:])
    monkeypatch.setattr(coord_map, "coord_clustering", lambda num_coords, d_map, num_links: (components, g1, 0.0))
    monkeypatch.setattr(coord_map.CoordMap, "kinematics_tree", lambda self, g0, g1: [dict(l) for l in tree["links"]])
    monkeypatch.chdir(tmp_path)
    base = ["--robot", robot, "--end_video", "2"]
    urdf = tmp_path / f"data/urdf/{robot}_8_seg/{step}_deg_{cams}_cams.urdf"
    # without --joint_types: today's refusal for the child that never turns, and nothing written
    with pytest.raises(ValueError, match="no step turns the child"):
        coord_map.main(base + ["--joint_limits"])
    assert not urdf.exists()
    # usage errors of main's own (the keys of parameters.json), before anything is written
    params = {"num_seg": 8, "dof": 4}
    for extra, match in (({"joint_types": True, "slide_min": 1e-6}, "joint_limits"), ({"joint_types": True, "joint_limits": True}, "slide_min"),
                         ({"slide_min": 1e-6, "joint_limits": True}, "joint_types"), ({"turn_min": 1e-3}, "joint_types")):
        (tmp_path / "parameters.json").write_text(json.dumps({robot: dict(params, **extra)}))
        with pytest.raises(ValueError, match=match):
            coord_map.main(base)
    (tmp_path / "parameters.json").write_text(json.dumps({robot: params}))
    assert not urdf.exists()
    capsys.readouterr()
    assert coord_map.main(base + ["--joint_limits", "--joint_types", "--slide_min", "1e-6"]) == str(urdf.relative_to(tmp_path))
    out = capsys.readouterr().out
    joints = {j.get("name"): j for j in ET.parse(urdf).getroot().findall("joint")}
    assert [joints[f"joint_{c}"].get("type") for _, c in tree["joints"]] == tree["types"]
    assert joints["joint_3"].find("axis") is None and joints["joint_3"].find("limit") is None
    report = json.loads(open(str(urdf)[:-len(".urdf")] + ".joint_motion.json").read())
    assert [(m["type"], m["unit"]) for m in report["joints"]] == [("revolute", "rad"), ("prismatic", "length"), ("fixed", None),
                                                                  ("revolute", "rad")]
    slide = report["joints"][JT.PRISMATIC]
    lim = joints["joint_2"].find("limit")
    assert float(lim.get("lower")) == min(slide["lower"], 0.0) == 0.0 and float(lim.get("upper")) == slide["upper"]
    assert abs(slide["upper"] - tree["q_true"][JT.PRISMATIC].max()) <= 1e-9
    assert max(l["rot_max"] for l in report["links"]) <= 1e-5 and max(l["pos_max"] for l in report["links"]) <= 1e-5 * 0.9
    lines = [x for x in out.splitlines() if x.startswith("joint_")]
    assert len(lines) == 4 and "prismatic" in lines[1] and "length units" in lines[1] and "fixed" in lines[2]
    assert "revolute" in lines[0] and "deg" in lines[0] and all("tilt_rms" in x and "slip_rms" in x for x in lines)
