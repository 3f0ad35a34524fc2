"""The host logic of the evaluation stage (autourdf_amd/evaluation.py; reference Sim/evaluation.py): joint_error on
constructed lines, map_commands, load_offset, the call surface, and the refusals that come before any GPU work.

Tolerances.  Positions: 1e-12 m (a handful of float64 operations on values below 1).  Directions: arccos near +-1
turns an error eps of the dot product into sqrt(2 eps) radians, so a few float64 ulps (eps ~ 1e-15) give up to about
3e-6 degrees: 1e-5 degrees where 0 or 180 degrees is expected; at 10 and 60 degrees the sensitivity is 1 / sin(theta)
(under 6), a few ulps stay far below 1e-9 degrees."""
import inspect
import os

import numpy as np
import pytest

POS_TOL = 1e-12
DIR_TOL_FLAT = 1e-5        # degrees, expected angle 0 or 180
DIR_TOL = 1e-9             # degrees, expected angle well inside (0, 180)


def _unit(v):
    v = np.asarray(v, np.float64)
    return v / np.linalg.norm(v)


def _perp(u):
    """Two unit vectors that complete `u` to a right-handed orthonormal frame."""
    h = np.array([1.0, 0, 0]) if abs(u[0]) < 0.9 else np.array([0, 1.0, 0])
    a = _unit(np.cross(u, h))
    return a, np.cross(u, a)


def test_joint_error_identical_lines():
    from autourdf_amd.evaluation import joint_error
    u = _unit([0.3, -0.5, 0.8])
    p = np.array([0.1, 0.2, -0.3])
    pos, ang = joint_error(p, u, p.copy(), u.copy())
    assert pos == 0.0 and abs(ang) <= DIR_TOL_FLAT
    # the same line through another of its points
    pos, ang = joint_error(p, u, p + 0.37 * u, u.copy())
    assert abs(pos) <= POS_TOL and abs(ang) <= DIR_TOL_FLAT


@pytest.mark.parametrize("d", [0.0125, 0.3, 1.7])
def test_joint_error_parallel_lines_give_their_distance(d):
    from autourdf_amd.evaluation import joint_error
    u = np.array([0.0, 0.0, 1.0])                     # exactly parallel: the cross product is exactly 0 (the parallel branch)
    a, _ = _perp(u)
    p = np.array([0.05, -0.02, 0.4])
    pos, ang = joint_error(p, u, p + d * a + 0.6 * u, u.copy())
    assert abs(pos - d) <= POS_TOL and abs(ang) <= DIR_TOL_FLAT


@pytest.mark.parametrize("theta_deg", [10.0, 60.0])
def test_joint_error_lines_through_one_point(theta_deg):
    from autourdf_amd.evaluation import joint_error
    u = _unit([1.0, 2.0, -0.5])
    a, _ = _perp(u)
    th = np.radians(theta_deg)
    v = np.cos(th) * u + np.sin(th) * a
    p = np.array([-0.2, 0.1, 0.3])
    pos, ang = joint_error(p + 0.4 * u, u, p - 0.9 * v, v)           # both pass through p
    assert abs(pos) <= POS_TOL and abs(ang - theta_deg) <= DIR_TOL


@pytest.mark.parametrize("dist,theta_deg", [(0.07, 60.0), (0.5, 10.0), (0.002, 85.0)])
def test_joint_error_skew_lines_give_the_common_normal_distance(dist, theta_deg):
    from autourdf_amd.evaluation import joint_error
    u = _unit([0.2, 0.9, 0.4])
    a, n = _perp(u)                                    # n is normal to both lines
    th = np.radians(theta_deg)
    v = np.cos(th) * u + np.sin(th) * a
    p = np.array([0.3, 0.3, -0.1])
    pos, ang = joint_error(p + 0.25 * u, u, p + dist * n - 0.8 * v, v)
    assert abs(pos - dist) <= POS_TOL and abs(ang - theta_deg) <= DIR_TOL


def test_joint_error_antiparallel_axes_give_180_degrees():
    from autourdf_amd.evaluation import joint_error
    u = _unit([0.3, -0.5, 0.8])
    a, _ = _perp(u)
    p = np.array([0.1, 0.2, -0.3])
    pos, ang = joint_error(p, u, p + 0.2 * a, -u)
    assert abs(pos - 0.2) <= POS_TOL and abs(ang - 180.0) <= DIR_TOL_FLAT


def test_joint_error_clips_a_dot_product_past_one():
    from autourdf_amd.evaluation import joint_error
    u = np.array([1.0, 0, 0]) * (1 + 4e-16)           # |u| a hair above 1: u.u > 1 would make arccos NaN without the clip
    pos, ang = joint_error(np.zeros(3), u, np.zeros(3), u)
    assert np.isfinite(ang) and ang == 0.0 and pos == 0.0


def test_map_commands_allegro_map_and_mixed_directions():
    from autourdf_amd.evaluation import map_commands
    joint_map = np.array([5, 6, 7, 8, 9, 10, 0, 1, 2, 3, 4])       # the reference's Sim/joint_map/allegro.txt
    direction = [1, -1, -1, 1, 1, -1, 1, 1, -1, 1, -1]
    a = np.random.default_rng(0).uniform(-1, 1, size=(3, 11))
    out = map_commands(a, joint_map, direction)
    assert out.shape == a.shape
    for i in range(11):
        np.testing.assert_array_equal(out[:, joint_map[i]], direction[i] * a[:, i])


def test_map_commands_identity():
    from autourdf_amd.evaluation import map_commands
    a = np.random.default_rng(1).uniform(-1, 1, size=(4, 5))
    np.testing.assert_array_equal(map_commands(a, np.arange(5), [1] * 5), a)


def test_load_offset_reads_the_first_sequences_first_frame(tmp_path):
    """The plain-text layout save_step_data writes: {seq}/{step:04}/joint_cfg.txt with 'name:value' per driven joint."""
    from autourdf_amd.evaluation import load_offset
    raw = tmp_path / "data" / "raw" / "toy" / "4_deg_20_cams"
    vals = {"V0000": {"0000": [0.25, -1.5, 0.000125], "0001": [9.0, 9.0, 9.0]}, "V0001": {"0000": [7.0, 7.0, 7.0]}}
    for seq, steps in vals.items():
        for step, v in steps.items():
            os.makedirs(raw / seq / step)
            with open(raw / seq / step / "joint_cfg.txt", "w") as f:
                for name, pos in zip(["waist", "shoulder", "wrist"], v):
                    f.write(f"{name}:{pos:,.6f}\n")
    off = load_offset(str(raw) + "/")
    assert isinstance(off, np.ndarray) and off.shape == (3,)
    np.testing.assert_allclose(off, [0.25, -1.5, 0.000125], atol=5e-7)       # six decimals on disk


def test_signatures_carry_the_reference_parameter_names_in_order():
    from autourdf_amd import evaluation as ev
    cj = list(inspect.signature(ev.compare_joints).parameters)
    assert cj[:7] == ["joint_map", "pred_urdf_path", "gt_urdf_path", "offset", "sim_ori", "pred_ori", "dof"]
    assert cj[7:] == ["global_scale"] and inspect.signature(ev.compare_joints).parameters["global_scale"].default == 1.0
    sig = inspect.signature(ev.evaluation).parameters
    assert list(sig)[:15] == ["pred_urdf_path", "gt_urdf_path", "pix", "dof", "radius", "num_cameras", "gui", "visualize",
                              "visualize_result", "save_path", "offset", "sim_ori", "pred_ori", "joint_map", "direction_map"]
    assert list(sig)[15:] == ["num_points", "num_poses", "global_scale"]
    assert (sig["pix"].default, sig["dof"].default, sig["radius"].default, sig["num_cameras"].default) == (800, 5, 1.5, 20)
    assert (sig["num_points"].default, sig["num_poses"].default, sig["global_scale"].default) == (10000, 3, 1.0)
    assert list(inspect.signature(ev.joint_error).parameters) == ["pos_a", "uv_a", "pos_b", "uv_b"]
    assert list(inspect.signature(ev.map_commands).parameters) == ["a_list", "joint_map", "direction_map"]
    assert list(inspect.signature(ev.load_offset).parameters) == ["raw_data_path"]


def test_main_help_exits_zero(capsys):
    from autourdf_amd.evaluation import main
    with pytest.raises(SystemExit) as e:
        main(["--help"])
    assert e.value.code == 0
    out = capsys.readouterr().out
    for flag in ("--robot", "--pix", "--num_cameras", "--num_cameras_eval", "--step_size", "--global_scale", "--num_poses",
                 "--num_points", "--joint_map"):
        assert flag in out
    for flag in ("--gui", "--vis_sim", "--vis "):
        assert flag not in out


@pytest.mark.parametrize("flag", ["gui", "visualize", "visualize_result"])
def test_evaluation_refuses_the_viewer_flags_before_any_work(tmp_path, flag):
    from autourdf_amd.evaluation import evaluation
    kw = dict(gui=False, visualize=False, visualize_result=False)
    kw[flag] = True
    with pytest.raises(NotImplementedError):
        evaluation(pred_urdf_path=str(tmp_path / "none.urdf"), gt_urdf_path=str(tmp_path / "none.urdf"), save_path=str(tmp_path) + "/out/",
                   offset=np.zeros(3), dof=3, joint_map=np.arange(3), direction_map=[1, 1, 1], **kw)
    assert not (tmp_path / "out").exists()             # refused before a directory was made or a URDF was read


def test_fk_table_is_topological_cached_and_scaled(tmp_path):
    """UrdfRobot.fk_table(): parents before children whatever the file order, unit axes, scaled origins, built once."""
    from _toy_urdf import write_toy_robot
    from autourdf_amd.sim_data import UrdfRobot
    path, links, joints = write_toy_robot(str(tmp_path))
    text = open(path).read()
    head, tail = text.index("  <joint"), text.index("</robot>")
    blocks = text[head:tail].split("  <joint")[1:]
    shuffled = str(tmp_path / "toy_shuffled.urdf")
    with open(shuffled, "w") as f:                     # joints in reverse file order: children before their parents
        f.write(text[:head] + "".join("  <joint" + b for b in reversed(blocks)) + text[tail:])
    for p, scale in ((path, 1.0), (shuffled, 0.5)):
        r = UrdfRobot(p, global_scale=scale)
        t = r.fk_table()
        assert t is r.fk_table()
        assert t["names"] == ["waist", "shoulder", "slide", "wrist"] and t["n_links"] == 5 and t["root"] == 0
        assert t["type"].tolist() == [1, 1, 2, 1] and t["type"].dtype == np.int32
        assert t["parent"].tolist() == [0, 1, 2, 3] and t["child"].tolist() == [1, 2, 3, 4]
        np.testing.assert_allclose(np.linalg.norm(t["axis"], axis=1), 1.0, atol=1e-15)
        np.testing.assert_allclose(t["axis"][3], np.array([1, 1, 0]) / np.sqrt(2), atol=1e-15)
        np.testing.assert_allclose(t["origin"][:, :3, 3], scale * np.array([j["xyz"] for j in joints]), atol=1e-15)
        q = r.q_rows([{"wrist": 0.5, "waist": -0.25}, {}])
        np.testing.assert_array_equal(q, [[-0.25, 0, 0, 0.5], [0, 0, 0, 0]])
