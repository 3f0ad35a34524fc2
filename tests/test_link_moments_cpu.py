"""The link-moments restatement (tests/_link_moments_ref.py) against finite differences of the host forward kinematics and against
the pose-fit restatement's long-double system; set_joint_frames on the toy URDF; the restatement's host driver; the torch twist
tables and assembly on CPU tensors; and the host side of creg_link_moments_f64 and of --refine_joints that needs no GPU:
signatures, the header's text, workspace arithmetic, argument errors, usage errors."""
import ctypes
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import _link_moments_ref as lm  # noqa: E402
import _point_mesh_ref as pref  # noqa: E402
import _pose_fit_ref as pf  # noqa: E402

INF = np.inf
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DRIVER_ITERS = 4                                                 # enough for both shoulder errors to fall; keeps the test quick


@pytest.fixture(scope="module")
def robot(tmp_path_factory):
    return pf.toy_robot(tmp_path_factory.mktemp("toy"))


def test_joint_basis_is_orthonormal_and_breaks_ties_by_the_lowest_index():
    from autourdf_amd.compute_joints import joint_frame_basis
    for a in ([0, 0, 1.0], [0, 1.0, 0], [1.0, 0, 0], np.array([1.0, 1.0, 0]) / np.sqrt(2), np.array([1.0, -2.0, 3.0]) / np.sqrt(14)):
        a = np.asarray(a, np.float64)
        u1, u2 = lm.joint_basis(a)
        np.testing.assert_allclose([u1 @ u1, u2 @ u2, u1 @ u2, u1 @ a, u2 @ a], [1, 1, 0, 0, 0], atol=1e-15)
        np.testing.assert_allclose(np.cross(u1, u2), a, atol=1e-15)
        np.testing.assert_array_equal(np.stack(joint_frame_basis(a[None]))[:, 0], [u1, u2])     # the package's is the restatement's
    np.testing.assert_array_equal(lm.joint_basis([0, 0, 1.0])[0], [0, 1.0, 0])           # k = 0: (0,0,1) x e_0
    np.testing.assert_array_equal(lm.joint_basis([0, 1.0, 0])[0], [0, 0, -1.0])          # k = 0 again: the lowest index at a tie


def test_structure_columns_against_finite_differences_of_the_conjugated_forward_kinematics(robot):
    """A point carried rigidly by its link moves by Omega x (c - rho) + V per unit of a frame parameter: every frame parameter of
    every joint at q != 0, central differences at two step sizes -- the error falls about fourfold when the step halves, or sits
    at the rounding floor.  A joint's frame moves exactly the links below it, and at q_j = 0 its columns are exactly zero."""
    rng = np.random.default_rng(7)
    table = robot.fk_table()
    J, L = len(table["names"]), int(table["n_links"])
    chain = pf.chains(table)
    q = robot.q_rows([{"waist": 0.7, "shoulder": -0.5, "slide": 0.02, "wrist": 0.9}])[0]
    G = pf.rigid_about(rng, 0.4, 0.1)
    eye = np.tile(np.eye(4), (J, 1, 1))
    T = lm.fk_conjugated(table, q, G, eye)
    np.testing.assert_allclose(T, G @ pf.fk(table, q, np.eye(4)), atol=1e-15)
    local = rng.normal(scale=0.1, size=(L, 5, 3))                                        # five points per link, in link frames
    world = lambda T: np.einsum("lij,lnj->lni", T[:, :3, :3], local) + T[:, None, :3, 3]
    c = world(T)
    ref = rng.normal(scale=0.2, size=(L, 3))
    center = rng.normal(scale=0.2, size=3)
    Tw = lm.twists(table, chain, T, q, center, ref)
    assert Tw.shape == (L, 6, 6 + 5 * J)
    field = lambda col: np.cross(Tw[:, None, :3, col], c - ref[:, None]) + Tw[:, None, 3:, col]
    for j in range(J):
        kind = int(table["type"][j])
        for m in range(4):
            col = 6 + J + 4 * j + m
            if kind == 2 and m >= 2:
                assert (Tw[:, :, col] == 0.0).all()
                continue
            errs = []
            for h in (2e-3, 1e-3):
                moved = []
                for sign in (1, -1):
                    s = np.zeros(4)
                    s[m] = sign * h
                    E = eye.copy()
                    E[j] = lm.frame_step(table["axis"][j], kind, s)
                    moved.append(world(lm.fk_conjugated(table, q, G, E)))
                errs.append(np.abs((moved[0] - moved[1]) / (2 * h) - field(col)).max())
            size = np.abs(field(col)).max()
            print(f"joint {j} frame parameter {m}: |central difference - column| {errs[0]:.3g} at h = 2e-3, {errs[1]:.3g} at 1e-3; column {size:.3g}")
            assert size > 1e-4
            assert errs[1] < 1e-9 or 3.0 < errs[0] / errs[1] < 5.0
            assert errs[1] < 1e-5 * max(size, 1e-2)
            below = np.array([(chain[l] >> j) & 1 for l in range(L)], bool)
            assert (np.abs(Tw[below][:, :, col]).max(1) > 0).all() and (Tw[~below][:, :, col] == 0.0).all()
    # the per-pose columns are the pose-fit entry's: one sided check of the joint columns against the plain forward kinematics
    for j in range(J):
        h = 1e-6
        q2 = q.copy()
        q2[j] += h
        fd = (world(G @ pf.fk(table, q2, np.eye(4))) - c) / h
        assert np.abs(fd - field(6 + j)).max() < 1e-5
    # exactly zero at q_j = 0
    q0 = q.copy()
    q0[[1, 2]] = 0.0
    Tw0 = lm.twists(table, chain, G @ pf.fk(table, q0, np.eye(4)), q0, center, ref)
    for j in (1, 2):
        assert (Tw0[:, :, 6 + J + 4 * j:6 + J + 4 * j + 4] == 0.0).all()
    assert (np.abs(Tw0[:, :, 6 + J:6 + J + 4]).max((0, 1)) > 0).all()
    # the package's tables (plain torch, here on CPU tensors) are these
    import torch

    from autourdf_amd.compute_joints import link_twists
    clean = {k: v for k, v in table.items() if not k.startswith("_dev")}
    for qq, want in ((q, Tw), (q0, Tw0)):
        got = link_twists(clean, torch.as_tensor(G @ pf.fk(table, qq, np.eye(4)))[None], torch.as_tensor(qq)[None], torch.as_tensor(center)[None],
                          torch.as_tensor(ref)[None])[0].numpy()
        np.testing.assert_allclose(got, want, rtol=0, atol=1e-15)
    assert (got[:, :, 6 + J + 4:6 + J + 12] == 0.0).all()


def test_pose_only_assembly_against_the_pose_fit_restatement(robot):
    """The moments about center_p, assembled with the per-pose twists, are the pose-fit system: H, g and cost against
    _pose_fit_ref.system's long-double sums on the GPU test's scene.  Both sides sum in long double; what differs is the
    rounding of the terms (a_j x (c - o_j) there, Omega x d + V here) and of the float64 assembly: at most 64 roundings of
    2^-53 on sum_l |Tw_a|^T |M6| |Tw_b| -- 6 x 6 products and sums per link, five links, and the terms' own few."""
    import torch

    from autourdf_amd.compute_joints import link_twists, twist_system
    sc = pf.system_scene(robot)
    _, idx, _ = pref.point_mesh(sc["tri"], sc["tri_start"], sc["link_T"], sc["pts"], sc["pt_start"], sc["d_max"])
    idx = idx.copy()
    idx[sc["drop"]] = -1
    table = {k: v for k, v in sc["table"].items() if not k.startswith("_dev")}
    want = pf.system(sc["tri"], sc["tri_start"], sc["link_T"], sc["pts"], sc["pt_start"], idx, table, sc["center"], sc["d_max"])
    P, L, J = len(sc["link_T"]), int(table["n_links"]), len(table["names"])
    ref = np.broadcast_to(sc["center"][:, None, :], (P, L, 3))
    m = lm.moments(sc["tri"], sc["tri_start"], sc["link_T"], sc["pts"], sc["pt_start"], idx, ref, sc["d_max"])
    np.testing.assert_array_equal(m["cnt"].sum(1), want["n"])
    np.testing.assert_array_equal(m["ok"], want["ok"])
    chain = pf.chains(table)
    # the package's assembly (plain torch, here on CPU tensors) from the same moments, held to the same bound
    Tt = link_twists(table, torch.as_tensor(sc["link_T"]), torch.zeros(P, J, dtype=torch.float64), torch.as_tensor(sc["center"]),
                     torch.as_tensor(np.ascontiguousarray(ref)), structure=False)
    Ht, gt, ct = (x.numpy() for x in twist_system(torch.as_tensor(m["mom"]), torch.as_tensor(m["cnt"]), Tt))
    worst = 0.0
    for p in range(P):
        Tw = lm.twists(table, chain, sc["link_T"][p], np.zeros(J), sc["center"][p], ref[p])[:, :, :6 + J]
        H, g, cost = lm.assemble(m["mom"][p], m["cnt"][p], Tw)
        Ha, ga, _ = lm.assemble(m["mom_abs"][p], m["cnt"][p], Tw, absolute=True)
        for name, a, b, s in (("H", H, want["H"][p], Ha), ("g", g, want["g"][p], ga), ("H, torch", Ht[p], want["H"][p], Ha),
                              ("g, torch", gt[p], want["g"][p], ga)):
            err, bound = np.abs(a - b), 64 * lm.EPS * s
            assert (err <= bound).all(), (p, name, float((err - bound).max()))
            with np.errstate(invalid="ignore", divide="ignore"):
                worst = max(worst, float(np.nanmax(np.where(bound > 0, err / bound, 0.0))))
        assert abs(cost - want["cost"][p]) <= 8 * lm.EPS * want["cost_abs"][p] and abs(ct[p] - want["cost"][p]) <= 8 * lm.EPS * want["cost_abs"][p]
    print(f"largest |assembled - pose-fit restatement| / bound: {worst:.3g}")
    assert (m["mom"][2] == 0).all() and (m["cnt"][2] == 0).all() and (m["cnt"][4, 1:] == 0).all() and m["cnt"][4, 0] > 50


def test_hand_case_one_triangle():
    """The pose-fit hand case: the triangle (0,0,0) (4,0,0) (0,4,0) of link 1, points (1,2,0.75) and (6,-1,2): c = (1,2,0), (4,0,0),
    r = (0,0,0.75), (2,-1,2); about rho = (1,0,0): d = (0,2,0), (3,0,0)."""
    tri, start = np.array([pref.TRI], np.float64), np.array([0, 0, 1])
    T = np.tile(np.eye(4), (1, 2, 1, 1))
    pts = np.array([[1.0, 2.0, 0.75], [6.0, -1.0, 2.0]])
    ref = np.array([[[9.0, 9.0, 9.0], [1.0, 0.0, 0.0]]])
    m = lm.moments(tri, start, T, pts, [0, 2], np.array([0, 0], np.int32), ref, INF)
    assert list(m["cnt"][0]) == [0, 2] and (m["mom"][0, 0] == 0).all()
    np.testing.assert_array_equal(m["mom"][0, 1], [9, 0, 0, 4, 0, 0, 3, 2, 0, 1.5, -6, -3, 2, -1, 2.75, 0.5625 + 9.0])
    # the system of the pose-fit hand case (one joint along z through (1,1,0), the base about the origin) from these moments:
    # every figure of that test, exactly -- the numbers are small integers and quarters
    import torch

    from autourdf_amd.compute_joints import link_twists, twist_system
    origin = np.eye(4)
    origin[:3, 3] = [1.0, 1.0, 0.0]
    table = {"parent": np.array([0], np.int32), "child": np.array([1], np.int32), "type": np.array([1], np.int32), "origin": origin[None],
             "axis": np.array([[0.0, 0.0, 1.0]]), "names": ["hinge"], "root": 0, "n_links": 2}
    Tw = link_twists(table, torch.as_tensor(T), torch.zeros(1, 1, dtype=torch.float64), torch.zeros(1, 3, dtype=torch.float64),
                     torch.as_tensor(ref), structure=False)
    H, g, cost = (x.numpy()[0] for x in twist_system(torch.as_tensor(m["mom"]), torch.as_tensor(m["cnt"]), Tw))
    assert H[6, 6] == 11.0 and g[6] == -1.0 and cost == 0.5625 + 9.0
    np.testing.assert_array_equal(H[3:6, 3:6], 2.0 * np.eye(3))
    np.testing.assert_array_equal(g[3:6], [2.0, -1.0, 2.75])
    np.testing.assert_array_equal(H[6, 3:6], [0.0, 3.0, 0.0])
    np.testing.assert_array_equal(g[:3], [1.5, -0.75 - 8.0, -4.0])
    assert H[2, 6] == 14.0 and H[6, 2] == 14.0
    m = lm.moments(tri, start, T, pts, [0, 2], np.array([0, -1], np.int32), ref, 0.75)
    assert list(m["cnt"][0]) == [0, 1] and m["mom"][0, 1, 15] == 0.5625


# ------------------------------------------------------------------------------------------ the host side
def test_signatures_header_text_and_version():
    from autourdf_amd import _lib
    res, args = _lib.SIGNATURES["creg_link_moments_workspace_bytes"]
    assert res is ctypes.c_size_t and args == [_lib.i64, _lib.i64, _lib.i32]
    res, args = _lib.SIGNATURES["creg_link_moments_f64"]
    assert res is ctypes.c_int and len(args) == 17
    assert args[2] is _lib.i64 and args[4] is _lib.i32 and args[5] is _lib.i64 and args[8] is _lib.i64 and args[9] is _lib.f64
    assert args[15] is _lib.sz and all(a is _lib.vp for i, a in enumerate(args) if i not in (2, 4, 5, 8, 9, 15))
    header = open(os.path.join(ROOT, "include", "creg.h")).read()
    decl = header[header.index("int creg_link_moments_f64("):]
    assert decl[:decl.index(";")].count(",") + 1 == 17
    text = header[header.index("Link moments:"):header.index("size_t creg_link_moments_workspace_bytes")]
    for word in ("d_x*d_x, d_x*d_y, d_x*d_z, d_y*d_y, d_y*d_z, d_z*d_z", "tiles of 64", "t mod 4", "(s0 + s1) + (s2 + s3)", "(n_pts >> 6) + n_poses",
                 "no floating-point atomics", "pt_tri_vec"):
        assert word in text, word
    lib = _lib.load(check_device=False)
    assert lib.creg_version() >= 2000 and hasattr(lib, "creg_link_moments_f64")


def test_workspace_bytes_is_monotone_and_zero_for_refused_counts():
    from autourdf_amd import _lib
    size = _lib.load(check_device=False).creg_link_moments_workspace_bytes
    for P, N, L in ((1, 0, 1), (3, 600, 5), (10, 50000, 12), (65536, 63, 2)):
        assert size(P, N, L) % 256 == 0 and size(P, N, L) >= 8 * 17 * L * ((N >> 6) + P)
        assert size(P + 1, N, L) > size(P, N, L) and size(P, N + 64, L) > size(P, N, L) and size(P, N + 1, L) >= size(P, N, L)
        assert size(P, N, L + 1) > size(P, N, L)
    for bad in ((0, 10, 4), (-1, 10, 4), (1, -1, 4), (1, 1 << 31, 4), (1, 10, 0), (1, 10, 65536), ((1 << 31), 0, 1)):
        assert size(*bad) == 0, bad


def test_entry_refuses_bad_arguments_before_any_device_call():
    """CREG_EINVAL with the entry's name in the text, from made-up addresses that are never dereferenced: there is no device here,
    a HIP call would answer CREG_EHIP."""
    from autourdf_amd import _lib
    lib = _lib.load(check_device=False)
    p, big = ctypes.c_void_p(0x1000), 1 << 40

    def call(n_tri=12, n_links=2, n_poses=3, n_pts=100, d_max=0.1, ws=p, ws_bytes=big, **null):
        a = {k: (None if k in null else p) for k in ("tri", "tri_start", "link_T", "pts", "pt_start", "tri_idx", "ref", "mom", "cnt")}
        return lib.creg_link_moments_f64(a["tri"], a["tri_start"], n_tri, a["link_T"], n_links, n_poses, a["pts"], a["pt_start"], n_pts,
                                         d_max, a["tri_idx"], a["ref"], a["mom"], a["cnt"], ws, ws_bytes, None)

    need = lib.creg_link_moments_workspace_bytes(3, 100, 2)
    cases = [dict(d_max=float("nan")), dict(d_max=-1.0), dict(n_poses=0), dict(n_links=0), dict(n_links=65536), dict(n_tri=-1),
             dict(n_tri=1 << 31), dict(n_pts=-1), dict(n_pts=1 << 31), dict(ws=None), dict(ws_bytes=need - 1), dict(ws_bytes=0)]
    cases += [{k: True} for k in ("tri", "tri_start", "link_T", "pts", "pt_start", "tri_idx", "ref", "mom", "cnt")]
    for kw in cases:
        assert call(**kw) == -1, kw
        assert b"creg_link_moments_f64" in lib.creg_last_error(), kw


# ------------------------------------------------------------------------------------------ the URDF writer, the driver, the command
def test_set_joint_frames_keeps_the_zero_pose_and_reloads(robot, tmp_path):
    """Every joint's frame of the toy URDF moved by its own E (a fixed one excepted there is none; the prismatic one turned only):
    the rewritten file reloads, its posed triangles at q = 0 equal the original's to 1e-12 of the bounding-box diagonal, its joint
    origins are E_pj^-1 O E_j, and axes, limits, names and meshes are untouched; the original file keeps every byte.  A posed
    robot differs: the frames did move."""
    import xml.etree.ElementTree as ET

    from autourdf_amd.compute_joints import set_joint_frames
    from autourdf_amd.sim_data import UrdfRobot
    table = robot.fk_table()
    names = list(table["names"])
    rng = np.random.default_rng(2)
    E = {n: lm.frame_step(table["axis"][j], int(table["type"][j]), rng.normal(scale=[0.05, 0.05, 0.01, 0.01])) for j, n in enumerate(names)}
    before = open(robot.path, "rb").read()
    out = os.path.join(os.path.dirname(robot.path), "moved.urdf")                   # beside the toy: its mesh names are relative
    set_joint_frames(robot.path, E, out)
    assert open(robot.path, "rb").read() == before
    moved = UrdfRobot(out)
    t2 = moved.fk_table()
    assert moved.links == robot.links and list(t2["names"]) == names
    np.testing.assert_array_equal(t2["axis"], table["axis"])
    np.testing.assert_array_equal(moved.tri_start, robot.tri_start)
    zero = np.zeros(len(names))
    a = pref.posed_mesh(robot.tri, robot.tri_start, pf.fk(table, zero, np.eye(4)))
    b = pref.posed_mesh(moved.tri, moved.tri_start, pf.fk(t2, zero, np.eye(4)))
    diag = float(np.linalg.norm(a.reshape(-1, 3).max(0) - a.reshape(-1, 3).min(0)))
    assert np.abs(a - b).max() <= 1e-12 * diag
    for j, n in enumerate(names):
        want = table["origin"][j] @ E[n]
        if j > 0:
            want = np.linalg.inv(E[names[j - 1]]) @ want              # a serial chain: the joint before is the parent's
        np.testing.assert_allclose(t2["origin"][j], want, atol=1e-14)
    q = robot.q_rows([{"waist": 0.7, "shoulder": -0.5, "slide": 0.02, "wrist": 0.9}])[0]
    a = pref.posed_mesh(robot.tri, robot.tri_start, pf.fk(table, q, np.eye(4)))
    b = pref.posed_mesh(moved.tri, moved.tri_start, pf.fk(t2, q, np.eye(4)))
    assert np.abs(a - b).max() > 1e-3
    # the conjugated forward kinematics is what the rewritten file does
    T = lm.fk_conjugated(table, q, np.eye(4), np.stack([E[n] for n in names]))
    np.testing.assert_allclose(pref.posed_mesh(robot.tri, robot.tri_start, T), b, atol=1e-13)
    old, new = ET.parse(robot.path).getroot(), ET.parse(out).getroot()
    rest = lambda root: [(e.tag, dict(e.attrib)) for e in root.iter() if e.tag != "origin"]
    assert rest(old) == rest(new)                                              # axes, limits, names, meshes: only origins differ
    # one joint only: the others' text is untouched
    set_joint_frames(robot.path, {"wrist": E["wrist"]}, out)
    one = ET.parse(out).getroot()
    for x, y in zip(old.findall("joint"), one.findall("joint")):
        if x.get("name") != "wrist":
            assert x.find("origin").attrib == y.find("origin").attrib
    # errors before anything is written
    target = str(tmp_path / "never.urdf")
    with pytest.raises(KeyError, match="elbow"):
        set_joint_frames(robot.path, {"shoulder": E["shoulder"], "elbow": np.eye(4)}, target)
    with pytest.raises(ValueError, match="4,4"):
        set_joint_frames(robot.path, {"shoulder": np.eye(3)}, target)
    assert not os.path.exists(target)


def test_restatement_driver_closes_in_on_the_true_shoulder_frame(robot):
    """The scene of the GPU test: clouds of the robot whose shoulder frame is off by 0.03 rad and 4 mm, q0 = q*, base and wrist
    locked.  The zero pose of the true robot is the toy's; the restatement's driver never raises the cost and lowers both the
    axis angle and the line distance of the shoulder within 4 steps (the GPU test runs this driver for its 12 beside the kernel's)."""
    c = lm.refine_case(robot)
    zero = np.zeros(4)
    a = pref.posed_mesh(robot.tri, robot.tri_start, pf.fk(c["table"], zero, np.eye(4)))
    b = pref.posed_mesh(c["true"].tri, c["true"].tri_start, pf.fk(c["true_table"], zero, np.eye(4)))
    assert np.abs(a - b).max() < 1e-15
    a0, d0 = lm.shoulder_errors(c, c["table"]["origin"])
    assert abs(a0 - lm.REFINE_TURN) < 1e-12 and abs(d0 - lm.REFINE_SHIFT) < 1e-5
    assert np.ptp(c["q_true"][:, 1]) == 1.8 and len({tuple(q) for q in c["q_true"]}) == 8
    out = lm.refine(robot.tri, robot.tri_start, c["table"], c["clouds"], c["q0"], None, INF, DRIVER_ITERS, False, c["lock"], c["lock_frames"])
    h = out["cost_history"]
    a1, d1 = lm.shoulder_errors(c, out["origin"])
    print(f"restatement driver: {out['iterations']} steps, cost {h[0]:.6g} -> {h[-1]:.6g}, shoulder axis angle {a0:.6g} -> {a1:.6g} rad, "
          f"line distance {d0:.6g} -> {d1:.6g}")
    assert all(y <= x for x, y in zip(h, h[1:])) and h[-1] < h[0] and len(h) == out["iterations"] + 1
    assert a1 < a0 and d1 < d0
    np.testing.assert_array_equal(out["frames"][3], np.eye(4))
    np.testing.assert_array_equal(out["q"][:, 3], c["q0"][:, 3])
    zero_after = pref.posed_mesh(out["tri"], robot.tri_start, pf.fk(dict(c["table"], origin=out["origin"]), zero, np.eye(4)))
    assert np.abs(zero_after - a).max() < 1e-12
    # the accumulated frames describe the whole result
    for j in range(4):
        want = c["table"]["origin"][j] @ out["frames"][j]
        if j > 0:
            want = np.linalg.inv(out["frames"][j - 1]) @ want
        np.testing.assert_allclose(out["origin"][j], want, atol=1e-13)


def test_torch_twists_and_assembly_are_the_restatement_on_the_host(robot):
    """compute_joints.link_twists and twist_system on CPU tensors (plain torch, no kernel) against the restatement's tables and
    assembly, structure columns included."""
    import torch

    from autourdf_amd.compute_joints import joint_frame_basis, link_twists, twist_system
    rng = np.random.default_rng(9)
    table = {k: v for k, v in robot.fk_table().items() if not k.startswith("_dev")}
    J, L, P = 4, 5, 3
    q = rng.uniform(-1, 1, size=(P, J)) * [1, 1, 0.04, 1]
    q[2, 1] = 0.0
    G = [pf.rigid_about(rng, 0.3, 0.1) for _ in range(P)]
    T = np.stack([G[p] @ pf.fk(table, q[p], np.eye(4)) for p in range(P)])
    center, ref = rng.normal(scale=0.2, size=(P, 3)), rng.normal(scale=0.2, size=(P, L, 3))
    u1, u2 = joint_frame_basis(table["axis"])
    for j in range(J):
        np.testing.assert_array_equal(np.stack(lm.joint_basis(table["axis"][j])), [u1[j], u2[j]])
    Tw = link_twists(table, torch.as_tensor(T), torch.as_tensor(q), torch.as_tensor(center), torch.as_tensor(ref)).numpy()
    chain = pf.chains(table)
    want = np.stack([lm.twists(table, chain, T[p], q[p], center[p], ref[p]) for p in range(P)])
    np.testing.assert_allclose(Tw, want, rtol=0, atol=1e-15)
    assert (Tw[2, :, :, 6 + J + 4:6 + J + 8] == 0.0).all()                      # q = 0 exactly: the shoulder's frame columns vanish
    mom = rng.normal(size=(P, L, 16))
    mom[..., [0, 3, 5, 15]] = np.abs(mom[..., [0, 3, 5, 15]]) + 1.0
    cnt = rng.integers(0, 50, size=(P, L))
    H, g, cost = (x.numpy() for x in twist_system(torch.as_tensor(mom), torch.as_tensor(cnt), torch.as_tensor(want)))
    for p in range(P):
        Hw, gw, cw = lm.assemble(mom[p], cnt[p], want[p])
        np.testing.assert_allclose(H[p], Hw, rtol=0, atol=1e-11 * np.abs(Hw).max())
        np.testing.assert_allclose(g[p], gw, rtol=0, atol=1e-11 * np.abs(gw).max())
        assert abs(cost[p] - cw) < 1e-12 * abs(cw)


def test_refine_joints_usage_errors_leave_an_empty_directory(tmp_path, monkeypatch, capsys):
    """--refine_joints without --cloud_fit, and --refine_iters without --refine_joints, end the command before anything is read
    or written (there is no parameters.json here to read)."""
    from autourdf_amd import coord_map
    monkeypatch.chdir(tmp_path)
    base = ["--robot", "testbot", "--voxel_size", "0.01", "--joint_limits"]
    for argv, word in ((base + ["--refine_joints"], "--refine_joints needs --cloud_fit"),
                       (base + ["--cloud_fit", "--refine_iters", "5"], "--refine_iters needs --refine_joints"),
                       (["--robot", "testbot", "--refine_joints"], "--refine_joints needs --cloud_fit")):
        with pytest.raises(SystemExit) as e:
            coord_map.main(argv)
        assert e.value.code == 2 and word in capsys.readouterr().err
        assert os.listdir(tmp_path) == []
    ns = coord_map._cli_parser().parse_args(base + ["--cloud_fit", "--refine_joints", "--refine_iters", "7"])
    assert ns.refine_joints and ns.refine_iters == 7
    assert coord_map._cli_parser().parse_args(base + ["--cloud_fit"]).refine_joints is False
