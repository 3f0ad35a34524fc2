"""No GPU: the three joint-motion entry points are declared, bound and built; the numpy restatement of their contracts
(tests/_joint_motion_ref.py) on the fixtures' own axes and on a synthetic tree with exact kinematics; set_joint_limits on
the fixture's URDF text; UrdfRobot without meshes; the command line's flags."""
import ctypes
import math
import os
import re
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
sys.path.insert(0, HERE)
import _joint_motion_ref as M  # noqa: E402

NAMES = {"creg_link_poses_f64": 10, "creg_joint_positions_f64": 18, "creg_motion_error_f64": 10}
# README.md's figures for fixture a: the observed range of each joint (parent, child), degrees
RANGES_A = {(1, 5): (-54.49, 51.43), (5, 0): (0.0, 57.36), (0, 2): (-52.73, 54.77), (2, 4): (0.0, 57.92), (4, 3): (-58.93, 56.66)}
TRUE_B = {(4, 3), (5, 0), (7, 1)}                   # the joints of fixture b's cyclic tree that are joints of the robot


def _fixture(g, tag):
    clusters = [[int(x) for x in c]
                for c in np.split(g[f"{tag}.link_cluster_idx"], np.cumsum(g[f"{tag}.link_cluster_sizes"])[:-1])]
    ids = g[f"{tag}.link_id"].tolist()
    pairs = list(zip(g[f"{tag}.joint_parent"].tolist(), g[f"{tag}.joint_child"].tolist()))
    joints = [(ids.index(p), ids.index(c)) for p, c in pairs]
    link_T = M.link_poses(g[f"{tag}.coords"], clusters)
    return pairs, M.joint_positions(link_T, joints, g[f"{tag}.local_axis"], g[f"{tag}.local_pos"])


@pytest.fixture(scope="module")
def fixture_a(golden):
    return _fixture(golden("joints_reference.npz"), "a")


@pytest.fixture(scope="module")
def tree():
    t = M.synthetic_tree(S=2, T=60)
    t["link_T"] = M.link_poses(t["coords"], t["link_clusters"])
    return t


# ------------------------------------------------------------------------------------------------ plumbing
def test_symbols_are_declared_bound_and_built():
    from autourdf_amd import _lib, build
    header = open(os.path.join(ROOT, "include", "creg.h")).read()
    assert "joint_motion.hip" in build.SOURCES and os.path.exists(os.path.join(build.CSRC, "joint_motion.hip"))
    assert os.path.exists(os.path.join(build.CSRC, "joints_dev.h"))
    L = ctypes.CDLL(build.build_lib())
    for name, n_args in NAMES.items():
        assert re.search(r"\b%s\s*\(" % name, header) and name in _lib.SIGNATURES
        assert getattr(L, name) is not None
        assert len(_lib.SIGNATURES[name][1]) == n_args
    assert _lib.load(check_device=False).creg_version() >= 1500
    # the header states the forms the kernels and the restatement share
    assert "atan2((v0 a0 + v1 a1) + v2 a2, c)" in header and "atan2(|v(E)|, c(E))" in header
    assert "u(i-1) + (d - 2pi * rint(d / 2pi))" in header and "half to even" in header


def test_shared_device_helpers_moved_to_the_header():
    src = open(os.path.join(ROOT, "autourdf_amd", "csrc", "joints.hip")).read()
    hdr = open(os.path.join(ROOT, "autourdf_amd", "csrc", "joints_dev.h")).read()
    assert '#include "joints_dev.h"' in src
    assert '#include "joints_dev.h"' in open(os.path.join(ROOT, "autourdf_amd", "csrc", "joint_motion.hip")).read()
    for name in ("jacobi_top", "link_mean_pose", "child_in_parent", "link_span"):
        assert re.search(r"__device__ (inline )?\w+ %s\(" % name, hdr), name
        assert not re.search(r"__device__ (inline )?\w+ %s\(" % name, src), name
    # the rotation's sine, cosine and norm, and a sample's relative motion: defined in the header and in no .hip file
    csrc = os.path.join(ROOT, "autourdf_amd", "csrc")
    text = {f: open(os.path.join(csrc, f)).read() for f in sorted(os.listdir(csrc)) if f.endswith((".hip", ".h"))}
    for name in ("skew_and_cos", "norm3", "joint_sample_motion"):
        assert re.search(r"__device__ inline \w+ %s\(" % name, hdr), name
        for f, body in text.items():
            if f.endswith(".hip"):
                assert not re.search(r"__device__ [\w ]*\b%s\(" % name, body), (name, f)
    for f in ("joints.hip", "joint_types.hip"):
        assert "joint_sample_motion(" in text[f] and "skew_and_cos(" in text[f] and "norm3(" in text[f], f
    assert sum(body.count("(R[7] - R[5]) * 0.5") for body in text.values()) == 1


def test_ops_need_device_tensors():
    import torch
    from autourdf_amd import ops
    with pytest.raises(RuntimeError):
        ops.link_poses(torch.zeros(1, 2, 3, 7, dtype=torch.float64), [[0], [1, 2]])
    with pytest.raises(RuntimeError):
        ops.joint_positions(torch.zeros(1, 2, 2, 4, 4, dtype=torch.float64), [(0, 1)], np.zeros((1, 3)), np.zeros((1, 4)))
    with pytest.raises(RuntimeError):
        z = torch.zeros(1, 2, 4, 4, dtype=torch.float64)
        ops.motion_error(z, z[0], z, z[0], torch.zeros(2, 3, dtype=torch.float64))


# ------------------------------------------------------------------------------------------------ the restatement
def test_fixture_a_is_revolute_and_its_ranges_are_the_listed_ones(fixture_a):
    pairs, out = fixture_a
    assert pairs == list(RANGES_A)
    assert out["tilt"].max() <= 1e-6 and out["slip"].max() <= 1e-6          # measured: 4.0e-8 and 3.0e-8
    assert np.all(out["q"][:, 0, 0] == 0.0)                                  # u(0, time_step) = 0
    assert out["n_used"].tolist() == [20] * 5
    for j, pc in enumerate(pairs):
        lo, hi = RANGES_A[pc]
        # README.md prints 0.01 degree; the recorded digits below are held to 1e-6 degree
        assert abs(math.degrees(out["lower"][j]) - lo) <= 0.005 + 1e-6 and abs(math.degrees(out["upper"][j]) - hi) <= 0.005 + 1e-6
    full = np.degrees(np.stack([out["lower"], out["upper"]], 1))
    ref = [[-54.49168058213753, 51.43353893677198], [0.0, 57.36022950702344], [-52.7259029084909, 54.77023073439231],
           [0.0, 57.91582565074569], [-58.92655844126086, 56.65539319004313]]
    np.testing.assert_allclose(full, ref, rtol=0, atol=1e-6)


def test_fixture_b_tells_the_true_joints_from_the_wrong_edges(golden):
    pairs, out = _fixture(golden("joints_reference.npz"), "b")
    assert TRUE_B <= set(pairs) and len(pairs) == 8
    for j, pc in enumerate(pairs):
        if pc in TRUE_B:
            assert out["tilt_max"][j] <= 1e-6 and out["slip_max"][j] <= 1e-6
        else:
            assert out["tilt_max"][j] >= 0.04, (pc, out["tilt_max"][j])     # the smallest measured: 0.046


def test_synthetic_tree_positions_are_recovered_through_the_unwrap(tree):
    out = M.joint_positions(tree["link_T"], tree["joints"], tree["local_axis"], tree["local_pos"])
    want = M.expected_positions(tree["q_true"], 0, 0, 0, 60)
    assert np.abs(out["q"] - want).max() <= 1e-12                            # measured 1.5e-15
    r = M.RAMP_JOINT
    assert np.abs(out["q"][r] - tree["q_true"][r]).max() <= 1e-12            # the ramp starts at its reference position
    assert abs(math.degrees(out["upper"][r] - out["lower"][r]) - 370.0) <= 1e-9
    assert out["lower_at"][r].tolist() == [0, 59] and out["upper_at"][r].tolist() == [1, 59]
    assert out["q"][r].min() < -math.pi and out["tilt"].max() <= 1e-12 and out["slip"].max() <= 1e-12


@pytest.mark.parametrize("ref_step,start,n", [(50, 0, 5), (59, 3, 20), (2, 3, 57)])
def test_synthetic_tree_reference_pose_inside_and_outside_the_used_steps(tree, ref_step, start, n):
    out = M.joint_positions(tree["link_T"], tree["joints"], tree["local_axis"], tree["local_pos"], 0, ref_step, start, n)
    assert np.abs(out["q"] - M.expected_positions(tree["q_true"], 0, ref_step, start, n)).max() <= 1e-12


def test_restated_summary_leaves_non_finite_samples_out(tree):
    link_T = tree["link_T"].copy()
    link_T[1, 40, 2] = np.nan                                                 # link 2 of sequence 1 from step 40 on
    out = M.joint_positions(link_T, tree["joints"], tree["local_axis"], tree["local_pos"])
    assert out["n_used"].tolist() == [120, 100, 120]                          # only joint (1, 2), steps 40..59 of sequence 1
    assert np.isnan(out["q"][1, 1, 40:]).all() and np.isfinite(out["q"][1, 1, :40]).all()
    ax = tree["local_axis"].copy()
    ax[0] = np.nan
    out = M.joint_positions(tree["link_T"], tree["joints"], ax, tree["local_pos"])
    assert out["n_used"].tolist() == [0, 120, 120] and np.isnan(out["lower"][0]) and out["lower_at"][0].tolist() == [-1, -1]


def test_restated_motion_error_is_free_of_frames():
    rng = np.random.default_rng(3)
    P, L = 4, 3
    A0, move = [M.random_rigid(rng) for _ in range(L)], [[M.random_rigid(rng) for _ in range(L)] for _ in range(P)]
    A = np.array([[move[p][l] @ A0[l] for l in range(L)] for p in range(P)])
    frames = [M.random_rigid(rng) for _ in range(L)]                          # another frame attached to each link
    B0 = np.array([A0[l] @ frames[l] for l in range(L)])
    B = np.array([[A[p, l] @ frames[l] for l in range(L)] for p in range(P)])
    rot, pos = M.motion_error(A, np.array(A0), B, B0, rng.normal(size=(L, 3)))
    assert rot.max() <= 1e-13 and pos.max() <= 1e-13                         # rounding only: the atan2 form has no sqrt(eps) floor
    for tw, want_rot, want_pos in ((M.JR.screw([0, 0, 1], 0.25, [0, 0, 0]), 0.25, None), (M.JR.screw([0, 0, 1], 0.0, [0, 0, 0], 0.5), 0.0, 0.5)):
        moved = np.array([[tw @ A[p, l] for l in range(L)] for p in range(P)])                # the same motion, then tw
        rot, pos = M.motion_error(A, np.array(A0), moved, np.array(A0), np.zeros((L, 3)))
        np.testing.assert_allclose(rot, want_rot, rtol=0, atol=1e-12)
        if want_pos is not None:
            np.testing.assert_allclose(pos, want_pos, rtol=0, atol=1e-12)


# ------------------------------------------------------------------------------------------------ set_joint_limits
def _motion(fixture_a):
    pairs, out = fixture_a
    return [{"parent_link": p, "child_link": c, "lower": float(out["lower"][j]), "upper": float(out["upper"][j]),
             "n_used": int(out["n_used"][j])} for j, (p, c) in enumerate(pairs)]


@pytest.fixture()
def urdf_a(golden, tmp_path):
    path = tmp_path / "robot.urdf"
    path.write_bytes(golden("joints_reference.npz")["a.urdf"].tobytes())
    return str(path)


def _limits(path):
    import xml.etree.ElementTree as ET
    return {j.get("name"): (j.get("type"), dict(j.find("limit").attrib)) for j in ET.parse(path).getroot().findall("joint")}


def test_set_joint_limits_rewrites_only_the_limits(fixture_a, urdf_a):
    from autourdf_amd import compute_joints
    motion = _motion(fixture_a)
    before = open(urdf_a, "rb").read().splitlines()
    compute_joints.set_joint_limits(urdf_a, motion[1:])                      # joint_5 is not named
    after = open(urdf_a, "rb").read().splitlines()
    assert len(after) == len(before)
    changed = [i for i, (x, y) in enumerate(zip(before, after)) if x != y]
    assert len(changed) == 4 and all(b"<limit " in before[i] and b"<limit " in after[i] for i in changed)
    lim = _limits(urdf_a)
    assert lim["joint_5"] == ("revolute", {"effort": "100", "velocity": "100", "lower": "-3.14159", "upper": "3.14159"})
    for m in motion[1:]:
        kind, a = lim[f"joint_{m['child_link']}"]
        assert kind == "revolute" and a["effort"] == "100" and a["velocity"] == "100"
        assert a["lower"] == str(min(m["lower"], 0.0)) and a["upper"] == str(max(m["upper"], 0.0))
        assert float(a["lower"]) <= 0.0 <= float(a["upper"])
    assert lim["joint_0"][1]["lower"] == "0.0"                               # the zero clamp: observed 0 .. 57.36 deg


def test_set_joint_limits_zero_clamp_pad_and_continuous(fixture_a, urdf_a):
    from autourdf_amd import compute_joints
    motion = _motion(fixture_a)
    motion[0].update(lower=0.2, upper=0.9)                                   # never at zero: the zero pose must stay valid
    motion[1].update(lower=-0.7, upper=-0.1)
    motion[2].update(lower=-3.2, upper=3.0)                                  # 6.2 + 2 * 0.05 >= 2 pi
    before = open(urdf_a, "rb").read().splitlines()
    compute_joints.set_joint_limits(urdf_a, motion, pad=0.05)
    lim = _limits(urdf_a)
    assert lim["joint_5"][1]["lower"] == "0.0" and lim["joint_5"][1]["upper"] == str(0.9 + 0.05)
    assert lim["joint_0"][1]["lower"] == str(-0.7 - 0.05) and lim["joint_0"][1]["upper"] == "0.0"
    assert lim["joint_2"] == ("continuous", {"effort": "100", "velocity": "100"})
    assert lim["joint_4"][0] == "revolute" and lim["joint_4"][1]["upper"] == str(motion[3]["upper"] + 0.05)
    after = open(urdf_a, "rb").read().splitlines()
    changed = [i for i, (x, y) in enumerate(zip(before, after)) if x != y]
    assert len(after) == len(before) and len(changed) == 6                   # five limits and one joint's type


def test_set_joint_limits_refusals_write_nothing(fixture_a, urdf_a):
    from autourdf_amd import compute_joints
    motion = _motion(fixture_a)
    text = open(urdf_a, "rb").read()
    with pytest.raises(KeyError):
        compute_joints.set_joint_limits(urdf_a, motion + [dict(motion[0], child_link=17)])
    assert open(urdf_a, "rb").read() == text
    with pytest.raises(ValueError, match="joint_2"):
        compute_joints.set_joint_limits(urdf_a, [motion[0], dict(motion[2], n_used=0, lower=math.nan, upper=math.nan)])
    assert open(urdf_a, "rb").read() == text
    stripped = re.sub(rb"\n\s*<limit [^>]*/>", b"", text, count=1)           # joint_5 loses its <limit>
    open(urdf_a, "wb").write(stripped)
    with pytest.raises(ValueError, match="joint_5"):
        compute_joints.set_joint_limits(urdf_a, motion)
    assert open(urdf_a, "rb").read() == stripped


# ------------------------------------------------------------------------------------------------ UrdfRobot, command line
def test_urdf_robot_without_meshes(urdf_a):
    from autourdf_amd.sim_data import UrdfRobot, _origin
    import xml.etree.ElementTree as ET
    with pytest.raises(FileNotFoundError):
        UrdfRobot(urdf_a)                                                    # the fixture's STL files do not exist
    rb = UrdfRobot(urdf_a, load_meshes=False)
    assert rb.tri.shape == (0, 3, 3) and len(rb.tri_link) == 0 and len(rb.cum_area) == 0
    assert rb.tri_start.tolist() == [0] * 7 and rb.collision_pairs().shape == (0, 2)
    assert rb.links == [f"link_{i}" for i in (1, 5, 0, 2, 4, 3)] and rb.root == "link_1"
    T = rb.fk({})
    origin = {j.get("name"): _origin(j) for j in ET.parse(urdf_a).getroot().findall("joint")}
    want = np.eye(4)
    np.testing.assert_array_equal(T[0], want)
    for i, child in enumerate((5, 0, 2, 4, 3)):                              # the chain 1 -> 5 -> 0 -> 2 -> 4 -> 3
        want = want @ origin[f"joint_{child}"]
        np.testing.assert_allclose(T[i + 1], want, rtol=0, atol=1e-15)
    assert rb.joints[0]["limit"] == [-3.14159, 3.14159]


def test_command_line_flags():
    import inspect
    from autourdf_amd import compute_joints, coord_map
    args = coord_map._cli_parser().parse_args(["--joint_limits", "--limit_pad", "2.5"])
    assert args.joint_limits and args.limit_pad == 2.5
    args = coord_map._cli_parser().parse_args([])
    assert args.joint_limits is False and args.limit_pad is None
    assert coord_map._cli_parser().parse_args(["--joint_limits"]).limit_pad is None
    with pytest.raises(SystemExit):
        coord_map._cli_parser().parse_args(["--limit_pad", "2.5"])
    with pytest.raises(SystemExit):
        coord_map._parser().parse_args(["--joint_limits"])                   # not a flag of the reference
    est = inspect.signature(compute_joints.estimate_joint_motion).parameters
    assert list(est) == ["links", "joint_data", "cm_list", "start_step", "num_steps", "time_step"]
    assert [est[k].default for k in ("start_step", "num_steps", "time_step")] == [0, 500, 0]
    assert list(inspect.signature(compute_joints.set_joint_limits).parameters) == ["urdf_file", "motion", "pad"]
    assert list(inspect.signature(compute_joints.replay_urdf).parameters) == [
        "urdf_file", "links", "motion", "cm_list", "start_step", "num_steps", "time_step"]
