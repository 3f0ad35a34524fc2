"""Collision hulls, host side (no GPU): the new C-ABI symbols, the certificate checker of tests/_hull_ref.py against Qhull and
against an exact brute-force hull, ``set_collision_meshes`` and the command-line option."""
import json
import os
import re

import numpy as np
import pytest

import _hull_ref as H

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_new_symbols_are_declared_bound_and_built():
    import ctypes
    from autourdf_amd import _lib, build, compute_joints, link, ops, sim_data
    import inspect
    header = open(os.path.join(ROOT, "include", "creg.h")).read()
    declared = set(re.findall(r"\b(creg_[a-z0-9_]+)\s*\(", header))
    names = ("creg_lattice_hull_workspace_bytes", "creg_lattice_hull_i32", "creg_lattice_hull_emit_i32")
    for name in names:
        assert name in declared and name in _lib.SIGNATURES, name
    assert [len(_lib.SIGNATURES[n][1]) for n in names] == [2, 11, 13]
    assert "hull.hip" in build.SOURCES and callable(getattr(ops, "lattice_hull"))
    for word in ("16383", "6 * 2^45", "det(b-a, c-a, p-a) <= 0", "V - E + F = 2", "CREG_HULL_ECOPLANAR", "smallest point index",
                 "at most n_l rounds"):                                 # the contract is stated, not only declared
        assert word in header, word
    for status, value in (("OK", 0), ("EFEW", 1), ("EIDENTICAL", 2), ("ECOLLINEAR", 3), ("ECOPLANAR", 4), ("ERANGE", 5)):
        assert re.search(rf"CREG_HULL_{status} = {value}\b", header) and value in ops.HULL_STATUS
    lib = ctypes.CDLL(build.build_lib())                               # the built library exports all three
    assert all(hasattr(lib, n) for n in names) and lib.creg_version() >= 1600
    lib.creg_lattice_hull_workspace_bytes.restype = ctypes.c_size_t
    lib.creg_lattice_hull_workspace_bytes.argtypes = [ctypes.c_int64, ctypes.c_int32]
    assert lib.creg_lattice_hull_workspace_bytes(-1, 1) == 0 and lib.creg_lattice_hull_workspace_bytes(10, 0) == 0
    small, big = lib.creg_lattice_hull_workspace_bytes(1000, 3), lib.creg_lattice_hull_workspace_bytes(2000, 3)
    assert 0 < small < big <= 2 * small                                # linear in the points: 24 n + 88 (2 n + 4 L) and padding
    assert "hull" in inspect.signature(link.link_mesh).parameters and inspect.signature(link.link_mesh).parameters["hull"].default is False
    assert inspect.signature(compute_joints.set_collision_meshes).parameters["suffix"].default == "_hull"
    assert inspect.signature(sim_data.UrdfRobot.__init__).parameters["geometry"].default == "visual"


# ---------------------------------------------------------------------------------------------- the checker itself
@pytest.fixture(scope="module")
def ball():
    P = H.lattice_ball(12)
    T, ext = H.scipy_hull(P)
    return P, T, ext


def test_checker_accepts_qhull_on_a_lattice_ball_and_a_flat_sided_block(ball):
    P, T, ext = ball
    assert (len(P), len(ext), len(T)) == (7153, 222, 440)
    assert H.certificate(P, T, P[ext]) == []
    B = H.lattice_block(21, 11, 6)
    Tb, eb = H.scipy_hull(B)
    assert H.certificate(B, Tb, H.block_corners(21, 11, 6)) == [] and H.volume6(B, Tb) == 6 * 20 * 10 * 5
    assert sorted(map(tuple, B[eb].tolist())) == sorted(map(tuple, H.block_corners(21, 11, 6).tolist()))


def test_checker_rejects_a_dropped_a_flipped_and_a_flat_face_and_a_missing_extreme_point(ball):
    P, T, ext = ball
    assert any("without their reverse" in b for b in H.certificate(P, T[1:], P[ext]))
    flipped = T.copy()
    flipped[7] = flipped[7][[0, 2, 1]]
    bad = H.certificate(P, flipped, P[ext])
    assert any("more than once" in b for b in bad) and any("strictly above" in b or "strictly below" in b for b in bad)
    # the hull of everything but one extreme point is closed and convex, and one point of the full set lies outside it
    keep = np.ones(len(P), bool)
    keep[ext[5]] = False
    ids = np.nonzero(keep)[0]
    T2, _ = H.scipy_hull(P[ids])
    assert H.certificate(P[ids], T2) == []
    bad = H.certificate(P, ids[T2], P[ext])
    assert any("strictly above" in b for b in bad) and any("extreme points are no vertex" in b for b in bad)
    # a zero-area sliver: the face (a,b,c) split at b' = b (a duplicate row of b) leaves (a,b,b') flat
    Pd = np.concatenate([P, P[T[0, 1]][None]])
    a, b, c = T[0]
    flat = np.concatenate([T[1:], [[a, b, len(P)], [a, len(P), c]]])
    assert any("zero area" in b_ for b_ in H.certificate(Pd, flat))
    assert any("zero area" in b_ for b_ in H.certificate(P, np.concatenate([T, [[a, b, b]]])))
    assert any("outside 0" in b_ for b_ in H.certificate(P, np.concatenate([T, [[a, b, len(P)]]])))


# ---------------------------------------------------------------------------------------------- ground truth on the CPU
SMALL = {"octahedron": lambda: H.voxel_verts(np.ones((1, 1, 1), bool)), "two voxels": lambda: H.voxel_verts(np.ones((2, 1, 1), bool)),
         "tetrahedron": lambda: np.array([[0, 0, 0], [4, 0, 0], [0, 4, 0], [0, 0, 4]]),
         "tetrahedron and centroid": lambda: np.array([[0, 0, 0], [4, 0, 0], [0, 4, 0], [0, 0, 4], [1, 1, 1]]),
         "cube with face and edge points": lambda: H.lattice_block(3, 3, 3),
         "random 12": lambda: H.random_lattice(12, 1, span=3), "random 30": lambda: H.random_lattice(30, 2, span=4),
         "random 40": lambda: H.random_lattice(40, 3, span=20), "limit tetrahedron": H.limit_tetra}


@pytest.mark.parametrize("name", sorted(SMALL))
def test_qhull_volume_equals_brute_force_on_small_lattice_sets(name):
    P = SMALL[name]()
    Tb, eb = H.brute_hull(P)
    assert H.certificate(P, Tb, P[eb]) == []
    Ts, es = H.scipy_hull(P)
    print(name, "6 x volume: brute force", H.volume6(P, Tb), "qhull", H.volume6(P, Ts), "extreme", len(eb), len(es))
    assert H.certificate(P, Ts, P[eb]) == []
    assert H.volume6(P, Ts) == H.volume6(P, Tb) > 0
    assert {tuple(p) for p in P[eb].tolist()} == {tuple(p) for p in P[es].tolist()}
    assert {"octahedron": 8, "two voxels": 32, "tetrahedron": 64, "tetrahedron and centroid": 64, "cube with face and edge points": 48}.get(
        name, H.volume6(P, Tb)) == H.volume6(P, Tb)


def test_brute_force_refuses_flat_sets_and_builders_give_the_meshers_lattice():
    with pytest.raises(ValueError):
        H.brute_hull([[0, 0, 0], [1, 0, 0], [0, 1, 0], [1, 1, 0], [5, 2, 0]])
    octa = H.voxel_verts(np.ones((1, 1, 1), bool))
    assert sorted(map(tuple, octa.tolist())) == [(0, 1, 1), (1, 0, 1), (1, 1, 0), (1, 1, 2), (1, 2, 1), (2, 1, 1)]
    assert len(H.voxel_verts(np.ones((2, 1, 1), bool))) == 10
    T = H.limit_tetra()
    assert np.abs(T).max() == H.LIMIT and abs(H.volume6(T, [[0, 1, 2], [0, 3, 1], [1, 3, 2], [2, 3, 0]])) == 16 * H.LIMIT ** 3


# ---------------------------------------------------------------------------------------------- the URDF and the command
def test_set_collision_meshes_rewrites_the_collision_filenames_and_nothing_else(tmp_path):
    from autourdf_amd.compute_joints import set_collision_meshes
    urdf = tmp_path / "toy.urdf"
    H.write_toy_urdf(str(urdf), "data/mesh/toy/", 4)
    before = urdf.read_bytes()
    set_collision_meshes(str(urdf))
    after = urdf.read_bytes()
    want = re.sub(rb"(<collision>.*?</collision>)", lambda m: m.group(1).replace(b".stl", b"_hull.stl"), before, flags=re.S)
    assert after == want and after != before and after.count(b"_hull.stl") == 4
    assert after.startswith(b"<?xml version='1.0' encoding='utf-8'?>\n<robot name=\"estimated_robot\">\n  <link name=\"link_0\">\n    <visual>")
    diff = [(x, y) for x, y in zip(before.split(b"\n"), after.split(b"\n")) if x != y]
    assert len(diff) == 4 and all(b"<mesh filename=" in x and y == x.replace(b".stl", b"_hull.stl") for x, y in diff)
    set_collision_meshes(str(urdf), suffix="_b")
    assert urdf.read_bytes().count(b"_hull_b.stl") == 4


def test_set_collision_meshes_refuses_a_link_without_the_block_and_writes_nothing(tmp_path):
    from autourdf_amd.compute_joints import set_collision_meshes
    urdf = tmp_path / "toy.urdf"
    H.write_toy_urdf(str(urdf), "data/mesh/toy/", 4, skip_collision_of=2)
    before = urdf.read_bytes()
    with pytest.raises(ValueError, match="link_2"):
        set_collision_meshes(str(urdf))
    assert urdf.read_bytes() == before and os.listdir(tmp_path) == ["toy.urdf"]
    H.write_toy_urdf(str(urdf), "data/mesh/toy/", 4)
    urdf.write_bytes(urdf.read_bytes().replace(b"0003.stl", b"0003.obj"))   # a mesh that is no .stl cannot be renamed either
    with pytest.raises(ValueError, match="link_3"):
        set_collision_meshes(str(urdf))
    assert b"_hull" not in urdf.read_bytes()


def test_cli_collision_hull_without_a_voxel_size_raises_before_anything_is_written(tmp_path, monkeypatch):
    import torch
    from autourdf_amd import coord_map
    assert coord_map._cli_parser().parse_args(["--collision_hull"]).collision_hull is True
    assert coord_map._cli_parser().parse_args([]).collision_hull is False
    (tmp_path / "parameters.json").write_text(json.dumps({"toy": {"num_seg": 8, "dof": 3}, "keyed": {"num_seg": 8, "dof": 3, "collision_hull": True}}))
    monkeypatch.chdir(tmp_path)
    monkeypatch.setenv("HIP_FORCE_DEV_KERNARG", os.environ.get("HIP_FORCE_DEV_KERNARG", "1"))
    monkeypatch.setattr(torch.cuda, "is_available", lambda: True)     # the check in front of parameters.json
    for argv in (["--robot", "toy", "--collision_hull"], ["--robot", "keyed"], ["--robot", "toy", "--collision_hull", "--density", "900"]):
        with pytest.raises(ValueError, match="voxel_size"):
            coord_map.main(argv)
    assert os.listdir(tmp_path) == ["parameters.json"]
    with pytest.raises(FileNotFoundError):                             # with a voxel size the option passes the check and meets the missing data
        coord_map.main(["--robot", "toy", "--collision_hull", "--voxel_size", "0.01"])
    assert os.listdir(tmp_path) == ["parameters.json"]
