"""No GPU: the mass-property entry point is declared, bound and built; --density parses; the numpy restatement
(tests/_inertia_ref.py) against exact sums and closed forms; set_inertials on a hand-written URDF; link_inertia's refusals."""
import ctypes
import json
import os
import re
import sys
import xml.etree.ElementTree as ET

import numpy as np
import pytest
import torch
from scipy.spatial.transform import Rotation

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
sys.path.insert(0, HERE)
import _inertia_ref as I  # noqa: E402
import _link_mesh_ref as M  # noqa: E402

EPS = 2.0 ** -52
NAMES = ("creg_mesh_inertia_workspace_bytes", "creg_mesh_inertia_f64")


def one(tri, density=1.0):
    """The restatement on one link."""
    out = I.mesh_inertia(tri, np.array([0, len(tri)]), density)
    return {k: v[0] for k, v in out.items()}


# ------------------------------------------------------------------------------------------------ plumbing
def test_symbols_are_declared_bound_and_built():
    from autourdf_amd import _lib, build
    header = open(os.path.join(ROOT, "include", "creg.h")).read()
    assert "inertia.hip" in build.SOURCES and os.path.exists(os.path.join(build.CSRC, "inertia.hip"))
    L = ctypes.CDLL(build.build_lib())
    for name in NAMES:
        assert re.search(r"\b%s\s*\(" % name, header) and name in _lib.SIGNATURES
        assert getattr(L, name) is not None
    assert len(_lib.SIGNATURES["creg_mesh_inertia_f64"][1]) == 17
    lib = _lib.load(check_device=False)
    assert lib.creg_mesh_inertia_workspace_bytes(-1, 1) == 0 and lib.creg_mesh_inertia_workspace_bytes(10, 0) == 0
    # 14 doubles per slot, floor(F / 256) + L + 1 slots, rounded up to 256 bytes
    assert lib.creg_mesh_inertia_workspace_bytes(1000, 3) == -(-(14 * 8 * (3 + 3 + 1)) // 256) * 256
    assert lib.creg_mesh_inertia_workspace_bytes(0, 1) >= 14 * 8 * 2


def test_density_option_parses_and_is_not_a_reference_flag():
    from autourdf_amd import coord_map
    args = coord_map._cli_parser().parse_args(["--density", "1250.5", "--voxel_size", "0.01"])
    assert args.density == 1250.5 and args.voxel_size == 0.01
    assert coord_map._cli_parser().parse_args([]).density is None
    with pytest.raises(SystemExit):
        coord_map._parser().parse_args(["--density", "1000"])


def test_mesh_inertia_needs_device_tensors():
    from autourdf_amd import ops
    tri, start = I.pack([I.triangles(I.box())])
    with pytest.raises(RuntimeError):
        ops.mesh_inertia(torch.from_numpy(tri), torch.from_numpy(start))


# ------------------------------------------------------------------------------------------------ the restatement
def test_k_stays_inside_the_cap():
    for F in [1, 2, 4, 12, 255, 256, 257, 65536, 65537, 2 ** 24, 2 ** 24 + 1, 2 ** 31 - 1]:
        assert I.k_bound(F) <= 32 + int(np.ceil(np.log2(F))), F
    assert I.k_bound(4) == I.k_bound(65536) == 26 and I.k_bound(65537) == 35 and I.k_bound(2 ** 31 - 1) == 44


@pytest.mark.parametrize("name,mesh", [("tetrahedron", I.tetrahedron((0.1, 0.2, 0.3), (1.3, 0.1, 0.2), (0.2, 0.9, 0.1), (0.3, 0.4, 1.1))),
                                       ("box", I.box(0.3, 0.2, 0.5)), ("bipyramid 127", I.bipyramid(127, 0.05, 0.03)),
                                       ("bipyramid 129", I.bipyramid(129, 0.05, 0.03)),
                                       ("icosphere 80", I.icosphere(1, (0.05, 0.03, 0.08))),
                                       ("icosphere 1280", I.icosphere(3, (0.05, 0.03, 0.08)))])
def test_restatement_sums_within_k_roundings_of_the_exact_sums(name, mesh):
    tri = I.triangles(mesh, shift=(0.31, -0.42, 0.47), f32=True)
    got = I.tree_sum(I.terms(tri))
    err = I.sum_errors(got, tri)
    print(f"{name}: F={len(tri)} k={I.k_bound(len(tri))}, max |sum - exact| / (2^-53 sum|term|) = {err.max():.3f}")
    assert err.max() <= I.k_bound(len(tri))


def test_tree_sum_levels():
    """More than 256 chunks: a second level over the chunk results; integers keep every order exact."""
    x = np.arange(14 * (65536 + 300), dtype=np.float64).reshape(-1, 14) % 1024
    np.testing.assert_array_equal(I.tree_sum(x), x.sum(0))
    assert (I.tree_sum(np.zeros((0, 14))) == 0).all()


def test_box_closed_forms():
    a, b, c, rho = 0.3, 0.2, 0.5, 1200.0
    r = one(I.triangles(I.box(a, b, c, centre=(0.4, -0.3, 0.2))), rho)
    m = rho * a * b * c
    np.testing.assert_allclose(r["volume"], a * b * c, rtol=32 * EPS)
    np.testing.assert_allclose(r["area"], 2 * (a * b + b * c + a * c), rtol=32 * EPS)
    np.testing.assert_allclose(r["mass"], m, rtol=32 * EPS)
    np.testing.assert_allclose(r["com"], (0.4, -0.3, 0.2), rtol=0, atol=32 * EPS)
    want = np.array([m / 12 * (b * b + c * c), 0, 0, m / 12 * (a * a + c * c), 0, m / 12 * (a * a + b * b)])
    np.testing.assert_allclose(r["inertia"], want, rtol=0, atol=256 * EPS * want.max())
    np.testing.assert_allclose(r["principal"], np.sort(want[[0, 3, 5]]), rtol=256 * EPS)
    assert r["closure"] <= 8 * EPS


def test_tetrahedron_closed_forms():
    """The trirectangular tetrahedron with legs p, q, s at the origin: V = pqs/6, com = (p, q, s)/4,
    second moments about the origin int x^2 = V p^2 / 10 and int xy = V p q / 20."""
    p, q, s, rho = 0.3, 0.5, 0.2, 7.0
    r = one(I.triangles(I.tetrahedron((0, 0, 0), (p, 0, 0), (0, q, 0), (0, 0, s))), rho)
    V = p * q * s / 6
    np.testing.assert_allclose(r["volume"], V, rtol=32 * EPS)
    np.testing.assert_allclose(r["com"], np.array([p, q, s]) / 4, rtol=64 * EPS)
    e = np.array([p, q, s])
    P = V * np.outer(e, e) / 20 + np.diag(V * e * e / 20)              # xx: V p^2 / 10
    C = P - V * np.outer(e / 4, e / 4)
    J = rho * (np.trace(C) * np.eye(3) - C)
    np.testing.assert_allclose(I.full(r["inertia"]), J, rtol=0, atol=256 * EPS * np.abs(J).max())
    assert r["closure"] <= 8 * EPS


def test_inertia_is_invariant_under_translation_and_turns_with_the_mesh():
    mesh = I.icosphere(2, (0.05, 0.03, 0.08))
    base = one(I.triangles(mesh), 900.0)
    scale = np.abs(base["inertia"]).max()
    for shift in [(0.3, -0.4, 0.5), (1000.0, -1000.0, 1000.0)]:
        moved = one(I.triangles(mesh, shift=shift), 900.0)
        # the vertices themselves are rounded at |shift|: relative 2^-53 |shift| / extent on every coordinate
        tol = 64 * EPS * max(1.0, np.abs(shift).max() / 0.03)
        np.testing.assert_allclose(moved["inertia"], base["inertia"], rtol=0, atol=tol * scale)
        np.testing.assert_allclose(moved["com"] - np.asarray(shift), base["com"], rtol=0, atol=tol * 0.08)
    Rm = Rotation.from_euler("xyz", [0.3, -1.1, 2.0]).as_matrix()
    verts, tris = mesh
    turned = one((verts @ Rm.T)[tris], 900.0)
    np.testing.assert_allclose(I.full(turned["inertia"]), Rm @ I.full(base["inertia"]) @ Rm.T, rtol=0, atol=256 * EPS * scale)
    np.testing.assert_allclose(turned["principal"], base["principal"], rtol=256 * EPS)
    np.testing.assert_allclose(turned["com"], Rm @ base["com"], rtol=0, atol=64 * EPS * 0.08)


def test_degenerate_links_give_zeros_and_nans():
    flat = np.array([[[0, 0, 0], [1, 0, 0], [0, 1, 0]], [[0, 0, 0], [0, 1, 0], [1, 0, 0]]], np.float64)   # zero volume
    out = I.mesh_inertia(np.concatenate([flat, I.triangles(I.box())]), np.array([0, 0, 2, 14]), 2.0)
    for l in (0, 1):
        assert (out["sums"][l] == 0).all() and out["volume"][l] == 0 and out["area"][l] == 0 and out["closure"][l] == 0
        assert out["mass"][l] == 0
        for k in ("com", "inertia", "principal", "axes"):
            assert np.isnan(out[k][l]).all()
    np.testing.assert_allclose(out["volume"][2], 1.0, rtol=16 * EPS)


def test_meshes_of_the_mesher_are_closed_and_outward():
    rng = np.random.default_rng(5)
    for n, extent in ((60, (0.2, 0.15, 0.1)), (400, (0.3, 0.1, 0.25))):
        m = M.mesh_link(rng.uniform(0, 1, (n, 3)) * extent + 0.4, 0.0101, True)
        tri = m["vertices"].astype(np.float32).astype(np.float64)[m["triangles"]]          # as the STL file holds them
        r = one(tri)
        F = len(tri)
        print(f"mesher F={F}: closure {r['closure']:.3e} ({r['closure'] / EPS:.2f} x 2^-52), volume {r['volume']:.6e}")
        assert r["volume"] > 0 and r["closure"] <= np.sqrt(3) * I.k_bound(F) * I.U     # three components, each within k roundings


# ------------------------------------------------------------------------------------------------ set_inertials
URDF = """<?xml version='1.0' encoding='utf-8'?>
<robot name="estimated_robot">
  <link name="link_0">
    <visual>
      <origin xyz="0.1 -0.2 0.3" rpy="0.0 0.0 0.0" />
      <geometry>
        <mesh filename="m/0000.stl" scale="1 1 1" />
      </geometry>
    </visual>
    <inertial>
      <origin xyz="0.1 -0.2 0.3" rpy="0.0 0.0 0.0" />
      <mass value="1.0" />
      <inertia ixx="0.1" ixy="0.0" ixz="0.0" iyy="0.1" iyz="0.0" izz="0.1" />
    </inertial>
  </link>
  <link name="link_1">
    <visual>
      <origin xyz="0.5 0.25 -1.0" rpy="0.3 -0.4 1.2" />
      <geometry>
        <mesh filename="m/0001.stl" scale="1 1 1" />
      </geometry>
    </visual>
    <inertial>
      <origin xyz="0.5 0.25 -1.0" rpy="0.3 -0.4 1.2" />
      <mass value="1.0" />
      <inertia ixx="0.1" ixy="0.0" ixz="0.0" iyy="0.1" iyz="0.0" izz="0.1" />
    </inertial>
  </link>
  <link name="link_2">
    <visual>
      <origin xyz="1.0 2.0 3.0" rpy="0.0 0.0 0.0" />
    </visual>
    <inertial>
      <origin xyz="1.0 2.0 3.0" rpy="0.0 0.0 0.0" />
      <mass value="1.0" />
      <inertia ixx="0.1" ixy="0.0" ixz="0.0" iyy="0.1" iyz="0.0" izz="0.1" />
    </inertial>
  </link>
  <joint name="joint_1" type="revolute">
    <parent link="link_0" />
    <child link="link_1" />
    <origin xyz="0.0 0.0 0.1" rpy="0.0 0.0 0.0" />
    <axis xyz="0.0 0.0 1.0" />
    <limit effort="100" velocity="100" lower="-3.14159" upper="3.14159" />
  </joint>
</robot>"""


def _rpy_matrix(r, p, y):
    """URDF's fixed-axis roll, pitch, yaw: Rz(y) Ry(p) Rx(r), written out."""
    cr, sr, cp, sp, cy, sy = np.cos(r), np.sin(r), np.cos(p), np.sin(p), np.cos(y), np.sin(y)
    return np.array([[cy, -sy, 0], [sy, cy, 0], [0, 0, 1]]) @ np.array([[cp, 0, sp], [0, 1, 0], [-sp, 0, cp]]) @ \
        np.array([[1, 0, 0], [0, cr, -sr], [0, sr, cr]])


def test_set_inertials_rewrites_the_named_links_only(tmp_path):
    from autourdf_amd.compute_joints import set_inertials
    path = tmp_path / "r.urdf"
    path.write_text(URDF)
    set_inertials(str(path), {})                                     # nothing named: the file comes back byte for byte
    assert path.read_text() == URDF
    J0 = [2.0, 0.1, -0.2, 3.0, 0.3, 4.0]
    J1 = [0.02, 0.001, -0.002, 0.03, 0.003, 0.04]
    set_inertials(str(path), {"link_0": {"mass": 2.5, "com": [0.01, 0.02, 0.03], "inertia": J0},
                              "link_1": {"mass": 0.75, "com": [0.1, -0.2, 0.05], "inertia": J1}})
    text = path.read_text()
    before, after = URDF.split("\n"), text.split("\n")
    assert len(before) == len(after)
    changed = [i for i, (x, y) in enumerate(zip(before, after)) if x != y]
    assert changed == [10, 11, 12, 23, 24, 25]                        # the three lines of the two named <inertial> blocks
    for i in changed:
        assert len(after[i]) - len(after[i].lstrip()) == 6
    links = {l.get("name"): l for l in ET.fromstring(text).findall("link")}
    num = lambda s: np.array(s.split(), np.float64)
    in0 = links["link_0"].find("inertial")
    np.testing.assert_allclose(num(in0.find("origin").get("xyz")), [0.11, -0.18, 0.33], rtol=4 * EPS)
    assert in0.find("origin").get("rpy") == "0.0 0.0 0.0" and float(in0.find("mass").get("value")) == 2.5
    assert [float(in0.find("inertia").get(k)) for k in ("ixx", "ixy", "ixz", "iyy", "iyz", "izz")] == J0
    in1 = links["link_1"].find("inertial")
    Rm = _rpy_matrix(0.3, -0.4, 1.2)
    np.testing.assert_allclose(num(in1.find("origin").get("xyz")), Rm @ [0.1, -0.2, 0.05] + [0.5, 0.25, -1.0], rtol=0, atol=8 * EPS)
    assert in1.find("origin").get("rpy") == "0.0 0.0 0.0" and float(in1.find("mass").get("value")) == 0.75
    got = I.full([float(in1.find("inertia").get(k)) for k in ("ixx", "ixy", "ixz", "iyy", "iyz", "izz")])
    np.testing.assert_allclose(got, Rm @ I.full(J1) @ Rm.T, rtol=0, atol=16 * EPS * 0.04)
    np.testing.assert_allclose(np.linalg.eigvalsh(got), np.linalg.eigvalsh(I.full(J1)), rtol=64 * EPS)
    with pytest.raises(KeyError):
        set_inertials(str(path), {"link_9": {"mass": 1.0, "com": [0, 0, 0], "inertia": J0}})
    # a link without the block create_urdf writes is refused by name, and the file stays as it was
    bare = tmp_path / "bare.urdf"
    bare.write_text(URDF.replace('      <mass value="1.0" />\n', "", 1))
    kept = bare.read_text()
    with pytest.raises(ValueError, match="link_0"):
        set_inertials(str(bare), {"link_1": {"mass": 1.0, "com": [0, 0, 0], "inertia": J0},
                                  "link_0": {"mass": 1.0, "com": [0, 0, 0], "inertia": J0}})
    assert bare.read_text() == kept
    assert path.read_text() == text                                  # the KeyError above wrote nothing either


# ------------------------------------------------------------------------------------------------ link_inertia
def _write_links(tmp_path, tri_list):
    from autourdf_amd import link
    d = str(tmp_path) + "/"
    for i, tri in enumerate(tri_list):
        rec = np.zeros((len(tri), 4, 3), np.float32)
        rec[:, 1:] = tri
        link.write_stl(d + f"{i:04}.stl", rec)
    return d


@pytest.fixture
def host_mesh_inertia(monkeypatch):
    """link_inertia's file handling and refusals without a GPU: ops.mesh_inertia replaced by the restatement."""
    from autourdf_amd import link
    calls = []

    def fake(tri, tri_start, density=1.0):
        calls.append(tuple(tri.shape))
        out = I.mesh_inertia(tri.numpy(), tri_start.numpy(), density)
        return {k: torch.from_numpy(np.ascontiguousarray(v)) for k, v in out.items()}
    monkeypatch.setattr(link.ops, "mesh_inertia", fake)
    monkeypatch.setattr(link._lib, "device", lambda *a: torch.device("cpu"))
    return calls


def test_link_inertia_writes_and_returns_the_values(tmp_path, host_mesh_inertia):
    from autourdf_amd import link
    tris = [I.triangles(I.box(0.3, 0.2, 0.5, centre=(0.4, 0.1, 0.2)), f32=True), I.triangles(I.icosphere(1, (0.05, 0.03, 0.08)), f32=True)]
    d = _write_links(tmp_path, tris)
    out = link.link_inertia([d], 1, 1000.0)
    assert host_mesh_inertia == [(12 + 80, 3, 3)]                    # one call for the directory
    assert len(out) == 1 and sorted(out[0]) == ["link_0", "link_1"]
    assert json.load(open(d + "inertial.json")) == out[0]
    for i, tri in enumerate(tris):
        want = one(tri, 1000.0)
        got = out[0][f"link_{i}"]
        assert sorted(got) == ["com", "inertia", "mass", "principal", "volume"]
        for k in got:
            np.testing.assert_array_equal(np.asarray(got[k]), want[k])
        assert got["mass"] > 0


def test_link_inertia_refuses_open_and_inward_meshes(tmp_path, host_mesh_inertia):
    from autourdf_amd import link
    good = I.triangles(I.box(0.3, 0.2, 0.5, centre=(0.4, 0.1, 0.2)), f32=True)
    d = _write_links(tmp_path, [good, good[:-1]])                    # a facet missing
    with pytest.raises(ValueError, match=r"0001\.stl.*not closed"):
        link.link_inertia([d], 1, 1000.0)
    d = _write_links(tmp_path, [good, good[:, ::-1]])                # every facet turned inwards
    with pytest.raises(ValueError, match=r"0001\.stl.*not positive"):
        link.link_inertia([d], 1, 1000.0)
    d = _write_links(tmp_path, [good[:0], good])                     # an empty file
    with pytest.raises(ValueError, match=r"0000\.stl.*not positive"):
        link.link_inertia([d], 1, 1000.0)
    # a missing facet of a 1280-facet mesh is still far above the default tolerance
    ico = I.triangles(I.icosphere(3, (0.05, 0.03, 0.08)), f32=True)
    d = _write_links(tmp_path, [ico[1:]])
    with pytest.raises(ValueError, match="not closed"):
        link.link_inertia([d], 0, 1000.0)
