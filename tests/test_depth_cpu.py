"""Depth-camera frames, host side (no GPU): the new C-ABI symbols, the CLI flags, the ground mesh, and the numpy restatement
of the ground removal on oracle depth buffers -- the inputs the GPU tests use are ones the method solves."""
import os
import re

import numpy as np
import pytest

import _depth_ref as ref
from _toy_urdf import write_toy_robot

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("creg_raster_depth_f64", "creg_depth_points_workspace_bytes", "creg_depth_points_count_f64", "creg_depth_points_f64",
       "creg_segment_plane_workspace_bytes", "creg_segment_plane_f64")


def test_new_symbols_are_declared_bound_and_built():
    from autourdf_amd import _lib, build, ops
    header = open(os.path.join(ROOT, "include", "creg.h")).read()
    declared = set(re.findall(r"\b(creg_[a-z0-9_]+)\s*\(", header))
    for name in NEW:
        assert name in declared and name in _lib.SIGNATURES, name
    assert "depth.hip" in build.SOURCES
    for fn in ("raster_depth", "depth_points", "segment_plane"):
        assert callable(getattr(ops, fn))


def test_cli_parses_pix_ground_depth_and_rejects_ground_alone(capsys):
    from autourdf_amd import sim_data
    a = sim_data.parse_args(["--robot", "toy", "--depth", "--ground", "--pix", "200", "--num_points", "800"])
    assert (a.robot, a.depth, a.ground, a.pix, a.num_points) == ("toy", True, True, 200, 800)
    d = sim_data.parse_args([])
    assert (d.depth, d.ground, d.pix, d.num_cameras) == (False, False, 800, 20)
    with pytest.raises(SystemExit):
        sim_data.parse_args(["--ground"])
    assert "--ground needs --depth" in capsys.readouterr().err
    with pytest.raises(ValueError, match="ground"):
        sim_data.collect("toy", {"gt": "x.urdf", "dof": 3}, ground=True)           # raised before anything is read


def test_ground_mesh_and_env_keep_the_robot_apart(tmp_path):
    from autourdf_amd.sim_data import SimEnv, ground_mesh
    g = ground_mesh(1.5, 8)
    assert g.shape == (2 * 8 * 8, 3, 3) and (g[:, :, 2] == 0).all() and np.abs(g[:, :, :2]).max() == 1.5
    e1, e2 = g[:, 1] - g[:, 0], g[:, 2] - g[:, 0]
    area = 0.5 * np.cross(e1, e2)[:, 2]
    assert (area > 0).all() and abs(area.sum() - 9.0) < 1e-12                        # covers [-1.5, 1.5]^2 once, all facing up
    path, _, _ = write_toy_robot(str(tmp_path))
    plain = SimEnv(path, dof=3, radius=1.2)
    env = SimEnv(path, dof=3, radius=1.2, ground_flag=True, ground_cells=8)
    assert plain.ground_tri is None and env.ground_tri.shape == (128, 3, 3)
    assert np.abs(env.ground_tri[:, :, :2]).max() == 1.2                             # ground_size defaults to the camera radius
    assert SimEnv(path, dof=3, ground_flag=True, ground_size=0.7, ground_cells=2).ground_tri.shape == (8, 3, 3)
    np.testing.assert_array_equal(env.robot.tri, plain.robot.tri)
    np.testing.assert_array_equal(env.robot.tri_link, plain.robot.tri_link)
    np.testing.assert_array_equal(env.robot.cum_area, plain.robot.cum_area)
    with pytest.raises(ValueError):
        ground_mesh(1.0, 0)


def test_data_collection_rejects_a_ground_the_env_lacks_and_an_unknown_source(tmp_path):
    from autourdf_amd.sim_data import SimEnv, data_collection
    path, _, _ = write_toy_robot(str(tmp_path))
    env = SimEnv(path, dof=3)
    with pytest.raises(ValueError, match="ground_flag"):
        data_collection(env, angle_list=np.zeros((1, 3)), ground_flag=True, source="depth")
    with pytest.raises(ValueError, match="source"):
        data_collection(env, angle_list=np.zeros((1, 3)), source="render")


def test_restatement_removes_exactly_the_ground_from_oracle_depth_buffers(tmp_path):
    """Oracle depth buffers of the toy on a ground (64 x 64, 3 cameras, 8 x 8 cells), back-projected and segmented per camera by the
    numpy restatement at H = 64, n = 6: the refit plane is z = 0, its inliers are the pixels with |z| < 0.001, no robot point
    above z = 0.002 goes."""
    env, q, tri, own, T = ref.toy_on_ground(tmp_path, ground_cells=8)
    depth = ref.oracle_depth(tri, own, T, env.cam_frames, 64, 64)
    P, off = ref.back_project(depth, env.cam_frames)
    assert off[0] == 0 and off[-1] == len(P) == np.isfinite(depth).sum() and (np.diff(off) > 1000).all()
    ground = np.abs(P[:, 2]) < 0.001
    assert 0.5 < ground.mean() < 0.99 and (P[:, 2] > 0.002).sum() > 100              # a ground and a robot are both in view
    rng = np.random.default_rng(0)
    samples = np.stack([rng.integers(0, off[s + 1] - off[s], (64, 6)) for s in range(3)])
    plane, mask, count, best, hyp, counts = ref.segment_plane(P, off, samples, 0.001)
    assert (~np.isnan(hyp[..., 0])).mean() >= 0.9
    np.testing.assert_allclose(plane, np.tile([0.0, 0.0, 1.0, 0.0], (3, 1)), atol=1e-9)
    np.testing.assert_array_equal(mask, ground)
    assert not (mask & (P[:, 2] > 0.002)).any()
    assert (best >= 0).all() and (count == [ground[off[s]:off[s + 1]].sum() for s in range(3)]).all()
    # the steps on their own: a plane through its three samples, the sign rule, an invalid collinear fit
    pl = ref.fit_plane(np.array([[0.0, 0, 1], [1, 0, 1], [0, 1, 1]]))
    np.testing.assert_allclose(pl, [0, 0, 1, -1], atol=1e-15)
    assert ref.fit_plane(np.array([[0.0, 0, 2], [-1, 0, 2], [0, 3, 2], [5, 5, 2]]) * [1, 1, -1])[2] == 1.0
    assert np.isnan(ref.fit_plane(np.array([[0.0, 0, 0], [1, 1, 2], [2, 2, 4], [3, 3, 6]]))).all()
    assert np.isnan(ref.fit_plane(np.tile([0.3, 0.1, 0.7], (6, 1)))).all()


def test_segment_plane_hands_over_a_buffer_of_the_bytes_it_names(monkeypatch):
    """S = 1, H = 1, n = 3: creg_segment_plane_workspace_bytes is 8 (4 SH + 9 SB) + 4 SH = 108 bytes, an odd count of 4-byte
    words, so a buffer counted in whole doubles must round up.  A stub library, CPU tensors: the wrapper's own arithmetic alone."""
    import torch
    from autourdf_amd import _lib, ops
    seen, held = {}, {}

    class Stub:
        @staticmethod
        def creg_segment_plane_workspace_bytes(N, S, H):
            seen["size_args"] = (N, S, H)
            return 8 * (4 * S * H + 9 * S * 1) + 4 * S * H

        @staticmethod
        def creg_segment_plane_f64(*args):
            seen["ws"], seen["ws_bytes"] = args[14].value, args[15]
            return 0

    def need(t, dtype, name):
        assert isinstance(t, torch.Tensor) and t.dtype == dtype, name
        return t.contiguous()

    def pointer(t):                                                    # every pointer the wrapper extracts, with its tensor
        if t is not None:
            held[t.data_ptr()] = t
        return ops._p(t)
    monkeypatch.setattr(_lib, "load", lambda *a, **k: Stub())
    monkeypatch.setattr(ops.sim, "_need", need)
    monkeypatch.setattr(ops.sim, "_p", pointer)
    monkeypatch.setattr(ops.sim, "_stream", lambda: None)
    points = torch.tensor([[0.0, 0, 0], [1, 0, 0], [0, 1, 0], [1, 1, 0], [0.5, 0.5, 1]], dtype=torch.float64)
    out = ops.segment_plane(points, None, 0.01, ransac_n=3, samples=torch.tensor([[[0, 1, 2]]]))
    assert len(out) == 4 and seen["size_args"] == (5, 1, 1) and seen["ws_bytes"] == 108 and (seen["ws_bytes"] // 4) % 2 == 1
    ws = held[seen["ws"]]
    assert ws.numel() * ws.element_size() >= seen["ws_bytes"] and seen["ws"] % 8 == 0
