"""Joints, link clouds and URDF export, host side (no GPU): the drop-in surface against the reference's, the modules'
imports, the fixture's sanity (tests/golden/joints_reference.npz), the restated jet colours and the screw-axis
formulas of tests/_joints_ref.py."""
import inspect
import math
import os
import re
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import _joints_ref as J  # noqa: E402


def _sig(f):
    return list(inspect.signature(f).parameters)


def test_signatures_match_the_reference_surface():
    from autourdf_amd import compute_joints as cj, coord_map, link
    assert _sig(cj.get_cluster_pose_mean) == ["cm", "cluster", "step"]
    assert _sig(cj.average_quaternions) == ["quaternions"]
    assert _sig(cj.relative_transform) == ["pose_parent", "pose_child"]
    assert _sig(cj.calculate_joint_axis_relative) == ["poses_parent", "poses_child"]
    assert _sig(cj.optimize_joint_axis) == ["poses_parent", "poses_child", "axes", "poses"]
    est = inspect.signature(cj.estimate_joint_axes_from_tree).parameters
    assert list(est) == ["links", "cm_list", "start_step", "num_steps", "interval"]
    assert [est[k].default for k in ("start_step", "num_steps", "interval")] == [0, 500, 1]
    cu = inspect.signature(cj.create_urdf).parameters
    assert list(cu) == ["links", "joint_data", "cm", "output_file", "mesh_dir", "time_step"]
    assert [cu[k].default for k in ("output_file", "mesh_dir", "time_step")] == ["robot.urdf", "", 0]
    assert _sig(coord_map.CoordMap.cluster_to_link) == ["self", "cluster_idx"]
    assert _sig(link.save_links) == ["cm_list", "cluster_idx", "path_list", "start_steps", "end_steps"]
    assert _sig(coord_map.main) == ["argv"]


def test_command_line_flags_are_the_references():
    from autourdf_amd import coord_map
    p = coord_map._parser()
    flags = {a.dest: a.default for a in p._actions if a.dest != "help"}
    assert flags == {"robot": "wx200_5", "xyz_r": 0.5, "start_steps": 0, "end_steps": 10, "start_video": 0,
                     "end_video": 1, "unknown_dof": False, "vis_flow": False, "num_cameras": 20, "step_size": 4,
                     "diff": False, "legacy": False}
    a = p.parse_args(["--unknown_dof", "--end_video", "2"])
    assert a.unknown_dof and a.end_video == 2


def test_new_modules_import_no_reference_only_wheel():
    for fn in ("compute_joints.py", "coord_map.py", "link.py"):
        src = open(os.path.join(ROOT, "autourdf_amd", fn)).read()
        for wheel in ("networkx", "sklearn", "matplotlib", "transforms3d", "open3d", "pybullet"):
            assert not re.search(rf"^\s*(from|import)\s+{wheel}\b", src, re.M), (fn, wheel)


def test_fixture_case_a_reference_axes_are_the_true_axes(golden):
    g, u = golden("joints_reference.npz"), golden("urdf_reference.npz")
    ids = g["a.link_id"].tolist()
    clusters = np.split(g["a.link_cluster_idx"], np.cumsum(g["a.link_cluster_sizes"])[:-1])
    for j, child in enumerate(g["a.joint_child"]):
        true_link = u["a.link_of"][clusters[ids.index(child)][0]]
        ga, ta = g["a.global_axis"][j], u["a.axes"][true_link]
        assert np.linalg.norm(np.cross(ga, ta)) <= 1e-6
        assert np.linalg.norm(np.cross(g["a.global_pos"][j] - u["a.joint_pos"][true_link], ta)) <= 1e-6
    assert len(g["a.joint_child"]) == len(u["a.parents"]) - 1


def test_restated_jet_equals_matplotlib():
    matplotlib = pytest.importorskip("matplotlib")
    from autourdf_amd.compute_joints import _jet
    cmap = matplotlib.colormaps["jet"]
    for n in range(1, 40):
        for i in range(n):
            assert " ".join(map(str, _jet(i / n)[:3] + (1,))) == " ".join(map(str, cmap(i / n)[:3] + (1,)))


@pytest.mark.parametrize("angle", [1e-3, math.radians(4), 1.0, math.pi / 2, math.radians(179.9)])
def test_closed_form_screw_agrees_with_the_restated_transforms3d_on_pure_rotations(angle):
    rng = np.random.default_rng(int(angle * 1e6))
    for _ in range(5):
        axis = rng.normal(size=3)
        axis /= np.linalg.norm(axis)
        point = rng.normal(size=3) * 0.2
        T = J.screw(axis, angle, point)
        d_ref, th_ref, p_ref = J.aff2axangle(T)
        d, th, p = J.closed_form(T)
        sg = 1.0 if d @ d_ref > 0 else -1.0
        # the restated transforms3d loses digits at small angles (its sine comes from one matrix entry)
        assert np.abs(sg * d_ref - d).max() <= 1e-9
        assert abs(sg * th_ref - th) <= 1e-6 * angle
        assert np.abs(J.init_position(p_ref[:3], d_ref) - p).max() <= 1e-8
        # the closed form against the construction itself
        assert th >= 0 and abs(th - angle) <= 1e-12
        assert np.abs(d - axis).max() <= 1e-9
        assert np.abs(p - J.init_position(point, axis)).max() <= 1e-9


def test_sample_order_is_the_references():
    assert J.sample_steps(1, 5, 1) == [(0, 0, 1), (0, 1, 2), (0, 2, 3), (0, 3, 4)]
    assert J.sample_steps(2, 6, 4) == [(0, 0, 4), (0, 1, 5), (1, 0, 4), (1, 1, 5)]


@pytest.mark.parametrize("tag", ["a", "b", "c"])
def test_reference_point_is_rounding_noise_once_the_motion_screws(golden, tag):
    """Why test_gpu_joints compares joint points with the reference only where every step's axial shift |d . t| is at
    most WELL_POSED: perturbing the fixture's coords by 1e-15 (relative) moves the reference's eig point by 1e-4 and
    more on every joint whose steps screw, and by < 1e-6 elsewhere, while the closed form moves by rounding only."""
    g = golden("joints_reference.npz")
    coords = g[f"{tag}.coords"]
    T = coords.shape[1]
    pert = coords * (1 + 1e-15 * np.random.default_rng(0).standard_normal(coords.shape))
    clusters = np.split(g[f"{tag}.link_cluster_idx"], np.cumsum(g[f"{tag}.link_cluster_sizes"])[:-1])
    ids = g[f"{tag}.link_id"].tolist()
    screwing = 0
    for pid, cid in zip(g[f"{tag}.joint_parent"], g[f"{tag}.joint_child"]):
        p, c = clusters[ids.index(pid)], clusters[ids.index(cid)]
        moved = {}
        for ref in (True, False):
            a, b = J.samples(coords, p, c, 0, T, 4, ref), J.samples(pert, p, c, 0, T, 4, ref)
            moved[ref] = max(np.abs(x[2] - y[2]).max() for x, y in zip(a, b))
        shift = max(x[3] for x in J.samples(coords, p, c, 0, T, 4, False))
        assert moved[False] <= 1e-12
        if shift > J.WELL_POSED:
            assert moved[True] >= 1e-4, (pid, cid, shift, moved[True])
            screwing += 1
        else:
            assert moved[True] <= 1e-6, (pid, cid, shift, moved[True])
    assert screwing == {"a": 0, "b": 5, "c": 5}[tag]
