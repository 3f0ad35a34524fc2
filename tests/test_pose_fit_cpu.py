"""The pose-fit restatement (tests/_pose_fit_ref.py) against finite differences of the host forward kinematics, hand-computed cases and
its own driver on the toy robot, and the host side of creg_pose_fit_system_f64 and of --fit_positions that needs no GPU: signatures,
workspace arithmetic, argument errors, usage errors."""
import ctypes
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import _point_mesh_ref as pref  # noqa: E402
import _pose_fit_ref as pf  # noqa: E402

INF = np.inf
DRIVER_ITERS = 12                                                # enough for every free joint to close in; keeps the test quick


@pytest.fixture(scope="module")
def robot(tmp_path_factory):
    return pf.toy_robot(tmp_path_factory.mktemp("toy"))


def test_chain_masks_of_the_toy_robot(robot):
    """base - waist - l1 - shoulder - l2 - slide - l3 - wrist - tip: a serial chain, so link l carries the bits of joints 0 .. l-1;
    the wrapper's masks are the restatement's; a joint with an index outside the links sets no bit."""
    from autourdf_amd import ops
    table = robot.fk_table()
    assert list(table["names"]) == ["waist", "shoulder", "slide", "wrist"] and list(table["type"]) == [1, 1, 2, 1]
    assert pf.chains(table) == [0, 1, 3, 7, 15]
    assert [int(x) for x in ops.joint_chains(table)] == [0, 1, 3, 7, 15] and ops.joint_chains(table).dtype == np.uint64
    broken = dict(table, child=np.array([1, 2, 9, 4], np.int32))
    assert pf.chains(broken) == [0, 1, 3, 0, 8] and [int(x) for x in ops.joint_chains(broken)] == [0, 1, 3, 0, 8]
    tree = {"n_links": 4, "parent": np.array([0, 0, 2], np.int32), "child": np.array([1, 2, 3], np.int32)}
    assert pf.chains(tree) == [0, 1, 2, 6] and [int(x) for x in ops.joint_chains(tree)] == [0, 1, 2, 6]


def test_jacobian_against_finite_differences_of_the_host_forward_kinematics(robot):
    """A closest point carried rigidly by its link moves by J delta + O(|delta|^2): every base component about ``center`` and
    every joint, the prismatic one included, at two step sizes -- the error falls about fourfold when delta halves (or is at the
    rounding floor where the motion is linear: translations and the prismatic joint).  Pins the signs, the chain masks (a joint
    below a point's link, or on another branch, must not move it) and ``center``."""
    rng = np.random.default_rng(5)
    table = robot.fk_table()
    names = list(table["names"])
    q = {"waist": 0.7, "shoulder": -0.5, "slide": 0.02, "wrist": 0.9}
    G = pf.rigid_about(rng, 0.4, 0.1)
    T = robot.fk(q, G)
    np.testing.assert_allclose(T, G @ pf.fk(table, robot.q_rows([q])[0], np.eye(4)), atol=1e-15)     # the restated FK is the host's
    pts, _ = pf.surface_points(pref.posed_mesh(robot.tri, robot.tri_start, T), 300, rng)
    pts = pts + rng.normal(scale=0.003, size=pts.shape)
    center = pts.mean(0) + [0.05, -0.02, 0.03]                     # not the mean: a wrong centre must show
    cut = [0, len(pts)]
    _, idx, _ = pref.point_mesh(robot.tri, robot.tri_start, T[None], pts, cut, INF)
    s = pf.system(robot.tri, robot.tri_start, T[None], pts, cut, idx, table, center[None], INF)
    assert s["ok"].all() and set(s["link"]) == {0, 1, 2, 3, 4}
    np.testing.assert_array_equal(s["c"], pts - s["r"])
    Tinv = np.linalg.inv(T)
    local = np.einsum("nij,nj->ni", Tinv[s["link"]], np.concatenate([s["c"], np.ones((len(pts), 1))], 1))

    def moved(delta):
        q2 = dict(q)
        for j, name in enumerate(names):
            q2[name] = q[name] + delta[6 + j]
        T2 = robot.fk(q2, pf.base_step(delta[:6], center) @ G)
        return np.einsum("nij,nj->ni", T2[s["link"]], local)[:, :3]

    for k in range(6 + len(names)):
        col = s["J"][:, k]
        errs = []
        for h in (2e-3, 1e-3):
            delta = np.zeros(6 + len(names))
            delta[k] = h
            errs.append(np.abs(moved(delta) - s["c"] - col * h).max())
        curved = k < 3 or (k >= 6 and table["type"][k - 6] == 1)
        print(f"parameter {k}: |c' - c - J h| = {errs[0]:.3g} at h = 2e-3, {errs[1]:.3g} at h = 1e-3; largest |J| {np.abs(col).max():.3g}")
        assert np.abs(col).max() > 0.0
        if curved:
            assert errs[0] <= 0.5 * 2e-3 ** 2 * 1.01 * np.linalg.norm(col, axis=1).max() + 1e-13     # |c' - c - J h| <= h^2 |J| / 2 for a rotation
            assert 3.5 < errs[0] / errs[1] < 4.5
        else:
            assert max(errs) < 1e-13
    # the masks: a joint moves exactly the points of the links below it
    for j in range(len(names)):
        below = s["link"] > j
        assert (np.abs(s["J"][below, 6 + j]).max(1) > 0).all() and (s["J"][~below, 6 + j] == 0.0).all()


def _one_joint_table(kind=1):
    origin = np.eye(4)
    origin[:3, 3] = [1.0, 1.0, 0.0]
    return {"parent": np.array([0], np.int32), "child": np.array([1], np.int32), "type": np.array([kind], np.int32),
            "origin": origin[None], "axis": np.array([[0.0, 0.0, 1.0]]), "names": ["hinge"], "root": 0, "n_links": 2}


def test_hand_cases_one_triangle_one_joint():
    """The triangle (0,0,0) (4,0,0) (0,4,0), owned by link 1 whose pose is the identity, with one joint along z through (1,1,0).  A
    point over the face at (1,2,0.75): c = (1,2,0), r = (0,0,0.75), joint column z x (0,1,0) = (-1,0,0).  A point off vertex b at
    (6,-1,2): c = (4,0,0), r = (2,-1,2), joint column z x (3,-1,0) = (1,3,0).  About the centre (0,0,0)."""
    tri, start = np.array([pref.TRI], np.float64), np.array([0, 0, 1])
    T = np.tile(np.eye(4), (1, 2, 1, 1))
    pts = np.array([[1.0, 2.0, 0.75], [6.0, -1.0, 2.0]])
    idx = np.array([0, 0], np.int32)
    s = pf.system(tri, start, T, pts, [0, 2], idx, _one_joint_table(1), np.zeros((1, 3)), INF)
    assert list(s["case"]) == [7, 2] and list(s["link"]) == [1, 1] and s["n"][0] == 2
    np.testing.assert_array_equal(s["r"], [[0, 0, 0.75], [2, -1, 2]])
    np.testing.assert_array_equal(s["c"], [[1, 2, 0], [4, 0, 0]])
    np.testing.assert_array_equal(s["J"][0, 6], [-1, 0, 0])
    np.testing.assert_array_equal(s["J"][1, 6], [1, 3, 0])
    np.testing.assert_array_equal(s["J"][0, :3], [[0, 0, 2], [0, 0, -1], [-2, 1, 0]])          # e_k x (1,2,0)
    np.testing.assert_array_equal(s["J"][1, :3], [[0, 0, 0], [0, 0, -4], [0, 4, 0]])           # e_k x (4,0,0)
    H, g = s["H"][0], s["g"][0]
    assert H[6, 6] == 11.0 and g[6] == -1.0 and s["cost"][0] == 0.5625 + 9.0
    np.testing.assert_array_equal(H[3:6, 3:6], 2.0 * np.eye(3))
    np.testing.assert_array_equal(g[3:6], [2.0, -1.0, 2.75])
    np.testing.assert_array_equal(H[6, 3:6], [0.0, 3.0, 0.0])
    np.testing.assert_array_equal(g[:3], [1.5, -0.75 - 8.0, -4.0])                             # e_k x c . r
    assert H[2, 6] == (-2 * -1 + 0) + (0 + 4 * 3) and H[6, 2] == H[2, 6]
    # the same joint as a slide along z, as a fixed joint, and without its chain bit
    p = pf.system(tri, start, T, pts, [0, 2], idx, _one_joint_table(2), np.zeros((1, 3)), INF)
    np.testing.assert_array_equal(p["J"][:, 6], [[0, 0, 1], [0, 0, 1]])
    assert p["H"][0, 6, 6] == 2.0 and p["g"][0, 6] == 2.75
    for table, chain in ((_one_joint_table(0), None), (_one_joint_table(1), [0, 0])):
        z = pf.system(tri, start, T, pts, [0, 2], idx, table, np.zeros((1, 3)), INF, chain=chain)
        assert (z["H"][0, 6] == 0).all() and (z["H"][0, :, 6] == 0).all() and z["g"][0, 6] == 0 and z["n"][0] == 2
    # who contributes: a NaN point, no correspondence, a row outside tri, a row of no link, a point beyond d_max
    pts5 = np.array([[np.nan, 0, 0], [1, 2, 0.75], [1, 2, 0.75], [1, 2, 0.75], [1, 2, 0.75]])
    s = pf.system(tri, start, T, pts5, [0, 5], np.array([0, -1, 1, 0, 0], np.int32), _one_joint_table(1), np.zeros((1, 3)), 0.75)
    assert list(s["ok"]) == [False, False, False, True, True] and s["n"][0] == 2 and s["cost"][0] == 2 * 0.5625
    s = pf.system(tri, start, T, pts5, [0, 5], np.zeros(5, np.int32), _one_joint_table(1), np.zeros((1, 3)), 0.7499)
    assert s["n"][0] == 0 and (s["H"] == 0).all() and s["cost"][0] == 0.0
    s = pf.system(tri, np.array([0, 0, 0]), T, pts5, [0, 5], np.zeros(5, np.int32), _one_joint_table(1), np.zeros((1, 3)), INF)
    assert s["n"][0] == 0                                          # row 0 belongs to no link


def test_restatement_residual_has_the_bits_of_the_point_mesh_distance(robot):
    """dot(r, r) of every contributing point is the dist2 of the point-mesh restatement for the same row, bit for bit, and all
    seven cases occur among the contributing points of the scene the GPU test uses."""
    sc = pf.system_scene(robot)
    d2, idx, _ = pref.point_mesh(sc["tri"], sc["tri_start"], sc["link_T"], sc["pts"], sc["pt_start"], sc["d_max"])
    idx = idx.copy()
    idx[sc["drop"]] = -1
    s = pf.system(sc["tri"], sc["tri_start"], sc["link_T"], sc["pts"], sc["pt_start"], idx, sc["table"], sc["center"], sc["d_max"])
    r = s["r"]
    np.testing.assert_array_equal(((r[:, 0] * r[:, 0] + r[:, 1] * r[:, 1]) + r[:, 2] * r[:, 2])[s["ok"]], d2[s["ok"]])
    counts = np.bincount(s["case"][s["ok"]], minlength=8)[1:]
    print("cases among the contributing points:", dict(zip(pf.CASES, counts)))
    assert (counts >= 2).all()
    assert not s["ok"][sc["nan_row"]] and not s["ok"][sc["far_row"]] and not s["ok"][sc["drop"]]
    assert list(s["n"][:4]) == [253, 254, 0, 254] and s["n"][4] == sc["pt_start"][5] - sc["pt_start"][4] > 50
    assert set(s["link"][sc["pt_start"][4]:]) == {0}


@pytest.fixture(scope="module")
def driver(robot):
    c = pf.driver_case(robot)
    out = pf.fit(robot.tri, robot.tri_start, c["table"], c["clouds"], c["q0"], None, INF, DRIVER_ITERS, False, c["lock"])
    return c, out


def test_restatement_driver_closes_in_on_the_true_joint_values(driver):
    """The toy robot, 4 poses with distinct true q*, 400 noise-free surface samples each; q0 = q* with waist, shoulder and slide
    off by 0.05 rad / 5 mm; the base and ``wrist`` locked.  Every pose's cost falls strictly, its history never rises, and every
    perturbed joint ends nearer q* than it started."""
    c, out = driver
    for p in range(4):
        h = out["cost_history"][p]
        e0, e1 = np.abs(c["q0"][p] - c["q_true"][p])[c["free"]], np.abs(out["q"][p] - c["q_true"][p])[c["free"]]
        print(f"pose {p}: {out['iterations'][p]} steps, cost {h[0]:.4g} -> {h[-1]:.4g}, rms {out['rms_before'][p]:.4g} -> "
              f"{out['rms_after'][p]:.4g}, |q - q*| {e0} -> {e1}")
        assert h[-1] < h[0] and all(b <= a for a, b in zip(h, h[1:])) and len(h) == out["iterations"][p] + 1
        assert (e1 < e0).all()
        locked = [j for j in range(4) if j not in c["free"]]
        np.testing.assert_array_equal(out["q"][p][locked], c["q0"][p][locked])
        np.testing.assert_array_equal(out["base"][p], np.eye(4))
        assert not out["unobserved"][p].any() and out["n"][p] == 400


def test_restatement_driver_stays_at_the_truth(robot):
    """Started at q* the residuals and g are of rounding size: whatever the few steps do, the pose stays at the truth."""
    c = pf.driver_case(robot)
    out = pf.fit(robot.tri, robot.tri_start, c["table"], c["clouds"][:1], c["q_true"][:1], None, INF, 5, False, c["lock"], tol=1e-6)
    assert 1 <= out["iterations"][0] <= 5 and out["rms_after"][0] <= out["rms_before"][0] < 1e-12
    assert np.abs(out["q"][0] - c["q_true"][0]).max() < 1e-6


# ------------------------------------------------------------------------------------------ the host side
def test_signatures_and_argument_counts():
    from autourdf_amd import _lib
    res, args = _lib.SIGNATURES["creg_pose_fit_workspace_bytes"]
    assert res is ctypes.c_size_t and args == [_lib.i64, _lib.i64, _lib.i32]
    res, args = _lib.SIGNATURES["creg_pose_fit_system_f64"]
    assert res is ctypes.c_int and len(args) == 26
    assert args[2] is _lib.i64 and args[4] is _lib.i32 and args[5] is _lib.i64 and args[8] is _lib.i64 and args[9] is _lib.f64
    assert args[16] is _lib.i32 and args[24] is _lib.sz
    assert all(a is _lib.vp for i, a in enumerate(args) if i not in (2, 4, 5, 8, 9, 16, 24))
    header = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "creg.h")).read()
    decl = header[header.index("int creg_pose_fit_system_f64("):]
    assert decl[:decl.index(";")].count(",") + 1 == 26


def test_workspace_bytes_is_monotone_and_zero_for_refused_counts():
    from autourdf_amd import _lib
    lib = _lib.load(check_device=False)
    assert lib.creg_version() >= 1900 and hasattr(lib, "creg_pose_fit_system_f64")
    size = lib.creg_pose_fit_workspace_bytes
    assert size(1, 0, 0) > 0 and size(1, 0, 58) > 0
    for P, N, J in ((1, 0, 4), (3, 600, 4), (3, 600, 0), (10, 50000, 58), (65536, 31, 1)):
        assert size(P, N, J) % 256 == 0
        assert size(P, N, J) >= 8 * (6 * P * J + ((N >> 5) + P) * ((6 + J) ** 2 + (6 + J) + 2))
        assert size(P + 1, N, J) >= size(P, N, J) and size(P, N + 32, J) > size(P, N, J) and size(P, N + 1, J) >= size(P, N, J)
        if J < 58:
            assert size(P, N, J + 1) > size(P, N, J)
    for bad in ((0, 10, 4), (-1, 10, 4), (1, -1, 4), (1, 1 << 31, 4), (1, 10, -1), (1, 10, 59), ((1 << 31), 0, 1)):
        assert size(*bad) == 0, bad


def test_entry_refuses_bad_arguments_before_any_device_call():
    """CREG_EINVAL with the entry's name in the text, from made-up addresses that are never dereferenced: there is no device here,
    a HIP call would answer CREG_EHIP."""
    from autourdf_amd import _lib
    lib = _lib.load(check_device=False)
    p, big = ctypes.c_void_p(0x1000), 1 << 40

    def call(n_tri=12, n_links=2, n_poses=3, n_pts=100, d_max=0.1, n_joints=4, ws=p, ws_bytes=big, **null):
        a = {k: (None if k in null else p) for k in ("tri", "tri_start", "link_T", "pts", "pt_start", "tri_idx", "parent", "child", "type",
                                                      "origin", "axis", "chain", "center", "H", "g", "cost", "n")}
        return lib.creg_pose_fit_system_f64(a["tri"], a["tri_start"], n_tri, a["link_T"], n_links, n_poses, a["pts"], a["pt_start"], n_pts,
                                            d_max, a["tri_idx"], a["parent"], a["child"], a["type"], a["origin"], a["axis"], n_joints,
                                            a["chain"], a["center"], a["H"], a["g"], a["cost"], a["n"], ws, ws_bytes, None)

    need = lib.creg_pose_fit_workspace_bytes(3, 100, 4)
    cases = [dict(n_joints=59), dict(n_joints=-1), dict(d_max=float("nan")), dict(d_max=-1.0), dict(n_poses=0), dict(n_links=0),
             dict(n_links=65536), dict(n_tri=-1), dict(n_tri=1 << 31), dict(n_pts=-1), dict(n_pts=1 << 31), dict(ws=None),
             dict(ws_bytes=need - 1), dict(ws_bytes=0)]
    cases += [{k: True} for k in ("tri", "tri_start", "link_T", "pts", "pt_start", "tri_idx", "parent", "child", "type", "origin", "axis",
                                  "chain", "center", "H", "g", "cost", "n")]
    for kw in cases:
        assert call(**kw) == -1, kw
        assert b"creg_pose_fit_system_f64" in lib.creg_last_error(), kw


def test_fit_positions_usage_errors_leave_an_empty_directory(tmp_path, monkeypatch, capsys):
    """--fit_positions without --cloud_fit, and --fit_iters without --fit_positions, end the command before anything is read or
    written (there is no parameters.json here to read)."""
    from autourdf_amd import coord_map
    monkeypatch.chdir(tmp_path)
    base = ["--robot", "testbot", "--voxel_size", "0.01", "--joint_limits"]
    for argv, word in ((base + ["--fit_positions"], "--fit_positions needs --cloud_fit"),
                       (base + ["--cloud_fit", "--fit_iters", "5"], "--fit_iters needs --fit_positions"),
                       (["--robot", "testbot", "--fit_positions"], "--fit_positions needs --cloud_fit")):
        with pytest.raises(SystemExit) as e:
            coord_map.main(argv)
        assert e.value.code == 2 and word in capsys.readouterr().err
        assert os.listdir(tmp_path) == []
    ns = coord_map._cli_parser().parse_args(base + ["--cloud_fit", "--fit_positions", "--fit_iters", "7"])
    assert ns.fit_positions and ns.fit_iters == 7
    assert coord_map._cli_parser().parse_args(base + ["--cloud_fit"]).fit_positions is False


def test_restatement_driver_reports_an_unobserved_joint(robot):
    """No cloud point within d_max of the tip: the wrist's diagonal entry is exactly 0, it is reported and keeps its bits, the
    other joints close in."""
    c = pf.unobserved_case(robot)
    out = pf.fit(robot.tri, robot.tri_start, c["table"], c["clouds"], c["q0"], None, c["d_max"], 6, False)
    w = c["wrist"]
    assert w == 3 and all(len(x) > 300 for x in c["clouds"])
    assert out["unobserved"][:, 6 + w].all() and not out["unobserved"][:, :6 + w].any()
    np.testing.assert_array_equal(out["q"][:, w].view(np.int64), c["q0"][:, w].view(np.int64))
    for p in range(2):
        h = out["cost_history"][p]
        assert h[-1] < h[0] and all(b <= a for a, b in zip(h, h[1:])) and out["n"][p] == len(c["clouds"][p])
        assert (np.abs(out["q"][p] - c["q_true"][p])[:2] < np.abs(c["q0"][p] - c["q_true"][p])[:2]).all()      # the two turning joints
