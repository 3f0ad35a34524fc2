"""creg_pose_fit_system_f64 on the GPU against the numpy restatement of its contract (tests/_pose_fit_ref.py): values within the
summation bound, exact counts, symmetric bits, exact zeros, determinism and the argument errors; the Levenberg-Marquardt driver
(SimEnv.fit_pose) against the restatement's driver; an unobserved joint; and the command line's --fit_positions on fixture a."""
import ctypes
import json
import math
import os
import sys

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu
HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import _collide_ref as ref  # noqa: E402
import _point_mesh_ref as pref  # noqa: E402
import _pose_fit_ref as pf  # noqa: E402
from _ply import write_ascii_ply  # noqa: E402

INF = np.inf
DRIVER_ITERS = 12                                                # as in test_pose_fit_cpu.py


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def bits(a):
    return np.ascontiguousarray(a).view(np.int64)


@pytest.fixture(scope="module")
def env(tmp_path_factory):
    return ref.toy(tmp_path_factory.mktemp("toy"))


@pytest.fixture(scope="module")
def scene(env):
    """The shared scene on the device, the correspondences of the point-mesh entry (one of them removed), the entry's answer and
    the restatement's."""
    from autourdf_amd import ops
    sc = pf.system_scene(env.robot)
    d = {k: dev(sc[k]) for k in ("tri", "tri_start", "link_T", "pts", "pt_start", "center")}
    _, idx, _ = ops.point_mesh_distance(d["tri"], d["tri_start"], d["link_T"], d["pts"], d["pt_start"], sc["d_max"])
    idx = idx.clone()
    idx[sc["drop"]] = -1
    d["tri_idx"] = idx
    table = {k: v for k, v in sc["table"].items() if not k.startswith("_dev")}
    got = ops.pose_fit_system(d["tri"], d["tri_start"], d["link_T"], d["pts"], d["pt_start"], idx, table, d["center"], sc["d_max"])
    want = pf.system(sc["tri"], sc["tri_start"], sc["link_T"], sc["pts"], sc["pt_start"], idx.cpu().numpy(), table, sc["center"], sc["d_max"])
    return sc, d, table, [g.cpu().numpy() for g in got], want


def test_system_against_the_restatement(scene):
    """Five poses of the toy robot (600 triangles): three with about 250 points off the posed surface (the prismatic joint moved in
    one), an empty one and one whose points all match the base link; a NaN point, a point without correspondence and a point
    beyond d_max.  n exact; H, g and cost within (n + 64) 2^-53 sum |term| of the long-double sums, entry by entry -- the bound of
    any summation order plus the terms' own roundings."""
    sc, _, _, (H, g, cost, n), want = scene
    counts = np.bincount(want["case"][want["ok"]], minlength=8)[1:]
    assert (counts >= 2).all(), dict(zip(pf.CASES, counts))                   # all seven pt_tri2 cases among the contributing points
    assert not want["ok"][[sc["nan_row"], sc["far_row"], sc["drop"]]].any()
    assert n.dtype == np.int64 and list(n) == list(want["n"]) and list(n[:4]) == [253, 254, 0, 254] and n[4] > 50
    eps = 2.0 ** -53
    worst = 0.0
    for p in range(len(n)):
        k = (n[p] + 64) * eps
        for name, a, b, s in (("H", H[p], want["H"][p], want["H_abs"][p]), ("g", g[p], want["g"][p], want["g_abs"][p]),
                              ("cost", cost[p], want["cost"][p], want["cost_abs"][p])):
            err, bound = np.abs(a - b), k * s
            assert (err <= bound).all(), (p, name, float((err - bound).max()))
            with np.errstate(invalid="ignore", divide="ignore"):
                worst = max(worst, float(np.nanmax(np.where(bound > 0, err / bound, 0.0))))
    print(f"largest |kernel - long double| / bound over all entries: {worst:.3g}")
    assert (H[2] == 0).all() and (g[2] == 0).all() and cost[2] == 0.0 and n[2] == 0          # the pose without points
    assert (H[:, :3, :3].diagonal(axis1=1, axis2=2)[[0, 1, 3, 4]] > 0).all()


def test_h_is_symmetric_in_its_bits_and_zero_where_nothing_moves(scene):
    from autourdf_amd import ops
    sc, d, table, (H, g, cost, n), want = scene
    np.testing.assert_array_equal(bits(H), bits(H.transpose(0, 2, 1)))
    # a pose whose points all match the base link: every joint row and column is exactly 0.0
    assert set(want["link"][sc["pt_start"][4]:sc["pt_start"][5]]) == {0}
    assert (H[4, 6:, :] == 0.0).all() and (H[4, :, 6:] == 0.0).all() and (g[4, 6:] == 0.0).all() and H[4, 3, 3] == float(n[4])
    # the wrist as a fixed joint: its row and column are exactly 0.0, everything else keeps its bits
    fixed = dict({k: v for k, v in table.items() if not k.startswith("_dev")}, type=np.array([1, 1, 2, 0], np.int32))   # no cached upload
    Hf, gf, cf, nf = (x.cpu().numpy() for x in ops.pose_fit_system(d["tri"], d["tri_start"], d["link_T"], d["pts"], d["pt_start"],
                                                                    d["tri_idx"], fixed, d["center"], sc["d_max"]))
    assert (Hf[:, 9, :] == 0.0).all() and (Hf[:, :, 9] == 0.0).all() and (gf[:, 9] == 0.0).all()
    assert (H[[0, 1, 3], 9, 9] > 0).all()                                      # it did move points as a revolute joint
    np.testing.assert_array_equal(bits(Hf[:, :9, :9]), bits(H[:, :9, :9]))
    np.testing.assert_array_equal(bits(gf[:, :9]), bits(g[:, :9]))
    np.testing.assert_array_equal(bits(cf), bits(cost))
    np.testing.assert_array_equal(nf, n)
    # translation block: sum of e_a . e_b = n on the diagonal, exactly
    for p in range(5):
        np.testing.assert_array_equal(H[p, 3:6, 3:6], float(n[p]) * np.eye(3))


def test_two_runs_and_a_pose_alone_give_the_same_bits(scene):
    from autourdf_amd import ops
    sc, d, table, first, _ = scene
    again = [x.cpu().numpy() for x in ops.pose_fit_system(d["tri"], d["tri_start"], d["link_T"], d["pts"], d["pt_start"], d["tri_idx"],
                                                           table, d["center"], sc["d_max"])]
    for a, b in zip(first, again):
        np.testing.assert_array_equal(bits(a), bits(b))
    s, e = int(sc["pt_start"][1]), int(sc["pt_start"][2])
    alone = ops.pose_fit_system(d["tri"], d["tri_start"], d["link_T"][1:2].contiguous(), d["pts"][s:e].contiguous(),
                                dev(np.array([0, e - s], np.int64)), d["tri_idx"][s:e].contiguous(), table, d["center"][1:2].contiguous(),
                                sc["d_max"])
    for a, b in zip(first, alone):
        np.testing.assert_array_equal(bits(a[1]), bits(b.cpu().numpy()[0]))


def test_argument_errors_return_einval_and_write_nothing(scene):
    from autourdf_amd import _lib, ops
    sc, d, table, _, _ = scene
    lib = _lib.load()
    ptr = lambda t: ctypes.c_void_p(t.data_ptr())
    P, L, F, N, J = 5, 5, len(sc["tri"]), len(sc["pts"]), 4
    tdev = [dev(np.ascontiguousarray(table[k])) for k in ("parent", "child", "type", "origin", "axis")]
    chain = dev(ops.joint_chains(table).view(np.int64))
    need = lib.creg_pose_fit_workspace_bytes(P, N, J)
    ws = torch.zeros(need // 8, dtype=torch.float64, device="cuda")
    outs = [torch.full((P, 64, 64), -7.0, dtype=torch.float64, device="cuda"), torch.full((P, 64), -7.0, dtype=torch.float64, device="cuda"),
            torch.full((P,), -7.0, dtype=torch.float64, device="cuda"), torch.full((P,), -7, dtype=torch.int64, device="cuda")]

    def call(n_joints=J, d_max=sc["d_max"], ws_bytes=need):
        return lib.creg_pose_fit_system_f64(ptr(d["tri"]), ptr(d["tri_start"]), F, ptr(d["link_T"]), L, P, ptr(d["pts"]), ptr(d["pt_start"]),
                                            N, d_max, ptr(d["tri_idx"]), *[ptr(t) for t in tdev], n_joints, ptr(chain), ptr(d["center"]),
                                            *[ptr(o) for o in outs], ptr(ws), ws_bytes, None)

    for kw in (dict(n_joints=59), dict(d_max=float("nan")), dict(d_max=-0.5), dict(ws_bytes=need - 1)):
        assert call(**kw) == -1, kw
        assert b"creg_pose_fit_system_f64" in lib.creg_last_error()
        torch.cuda.synchronize()
        assert all(bool((o == -7).all()) for o in outs) and bool((ws == 0).all()), kw
    assert call() == 0                                                          # the same buffers, everything in order
    torch.cuda.synchronize()
    assert bool((outs[3] >= 0).all())
    # the wrapper: before any launch
    big = {"parent": np.zeros(59, np.int32), "child": np.ones(59, np.int32), "type": np.ones(59, np.int32), "origin": np.tile(np.eye(4), (59, 1, 1)),
           "axis": np.tile([0.0, 0.0, 1.0], (59, 1)), "names": [str(i) for i in range(59)], "root": 0, "n_links": 5}
    args = (d["tri"], d["tri_start"], d["link_T"], d["pts"], d["pt_start"], d["tri_idx"])
    with pytest.raises(ValueError, match="<= 64"):
        ops.pose_fit_system(*args, big, d["center"], 0.1)
    for bad in (float("nan"), -1.0):
        with pytest.raises(ValueError, match="d_max"):
            ops.pose_fit_system(*args, table, d["center"], bad)
    with pytest.raises(ValueError, match="expected"):
        ops.pose_fit_system(*args[:5], d["tri_idx"][:-1].contiguous(), table, d["center"], 0.1)
    with pytest.raises(TypeError):
        ops.pose_fit_system(*args[:5], d["tri_idx"].to(torch.int64), table, d["center"], 0.1)


def test_driver_against_the_restatement_driver(env):
    """The CPU test's case through SimEnv.fit_pose: 4 poses, 400 noise-free surface samples each, waist / shoulder / slide off by
    0.05 rad / 5 mm, base and wrist locked.  The cost history never rises; the final rms and the final max |q - q*| over the free
    joints are at most 2 x the restatement driver's, plus 1e-12 x the scene diagonal (one accept / reject decision flipped by
    rounding moves lambda by a factor of 10 for one iteration)."""
    r = env.robot
    c = pf.driver_case(r)
    want = pf.fit(r.tri, r.tri_start, c["table"], c["clouds"], c["q0"], None, INF, DRIVER_ITERS, False, c["lock"])
    got = env.fit_pose(c["clouds"], c["q0"], d_max=INF, max_iter=DRIVER_ITERS, fit_base=False, lock=c["lock"])
    diag = pref.scene_diagonal(r.tri, r.tri_start, np.stack([pf.fk(c["table"], q, np.eye(4)) for q in c["q_true"]]), np.concatenate(c["clouds"]))
    assert got["names"] == list(c["table"]["names"]) and got["q"].shape == (4, 4) and got["base"].shape == (4, 4, 4)
    for p in range(4):
        h = got["cost_history"][p]
        eg, ew = np.abs(got["q"][p] - c["q_true"][p])[c["free"]].max(), np.abs(want["q"][p] - c["q_true"][p])[c["free"]].max()
        print(f"pose {p}: kernel driver {got['iterations'][p]} steps, rms {got['rms_before'][p]:.6g} -> {got['rms_after'][p]:.6g}, max |q - q*| "
              f"{eg:.6g}; restatement driver {want['iterations'][p]} steps, rms {want['rms_after'][p]:.6g}, max |q - q*| {ew:.6g}")
        assert all(b <= a for a, b in zip(h, h[1:])) and len(h) == got["iterations"][p] + 1 and h[-1] < h[0]
        assert got["rms_after"][p] <= 2.0 * want["rms_after"][p] + 1e-12 * diag
        assert eg <= 2.0 * ew + 1e-12 * diag
        locked = [j for j in range(4) if j not in c["free"]]
        np.testing.assert_array_equal(bits(got["q"][p][locked]), bits(c["q0"][p][locked]))
        np.testing.assert_array_equal(got["base"][p], np.eye(4))
        assert got["n"][p] == 400 and not got["unobserved"][p].any()


def test_an_unobserved_joint_is_reported_and_keeps_its_bits(env):
    """The wrist unlocked, clouds without a point near the tip and a d_max below that gap: no tip point contributes, the wrist's
    diagonal entry is exactly 0, it is reported in ``unobserved`` and its q is unchanged, bit for bit."""
    r = env.robot
    c = pf.unobserved_case(r)
    got = env.fit_pose(c["clouds"], c["q0"], d_max=c["d_max"], max_iter=6, fit_base=False)
    w = c["wrist"]
    assert got["unobserved"][:, 6 + w].all() and not got["unobserved"][:, 6:6 + w].any() and not got["unobserved"][:, :6].any()
    np.testing.assert_array_equal(bits(got["q"][:, w]), bits(c["q0"][:, w]))
    assert (got["q"][:, :w] != c["q0"][:, :w]).all()                            # the others did move
    for p in range(len(c["clouds"])):
        h = got["cost_history"][p]
        assert all(b <= a for a, b in zip(h, h[1:])) and h[-1] < h[0]
        assert (np.abs(got["q"][p] - c["q_true"][p])[:2] < np.abs(c["q0"][p] - c["q_true"][p])[:2]).all()      # the two turning joints


def _layout(tmp_path, golden, robot, cams, step):
    """A data directory as the command line expects it (test_gpu_cloud_fit.py's): registered sequences, raw frames, parameters.json."""
    M_ = golden("urdf_reference.npz")["a.matrices"]                            # (2,10,20,4,4), six links
    S, T, K = M_.shape[:3]
    (tmp_path / "parameters.json").write_text(json.dumps({robot: {"num_seg": K, "dof": 5}}))
    rng = np.random.default_rng(0)
    for s in range(S):
        part = tmp_path / f"data/part/{robot}_{K}_seg/{step}_deg_{cams}_cams/seq{s}"
        (part / "matrix").mkdir(parents=True)
        (part / "cluster").mkdir()
        for t in range(T):
            np.save(part / f"matrix/{t:04}.npy", M_[s, t])
            np.savez(part / f"cluster/{t:04}.npz", **{str(k): rng.normal(scale=0.02, size=(16, 3)).astype(np.float32)
                                                     for k in range(K)})
            raw = tmp_path / f"data/raw/{robot}/{step}_deg_{cams}_cams/seq{s}/{t:04}"
            raw.mkdir(parents=True)
            a = 0.9 / (2 * math.sqrt(3))                                      # AABB diagonal 0.9, as the fixture's
            write_ascii_ply(str(raw / "robot.ply"), np.vstack([rng.uniform(-a, a, size=(62, 3)), [[-a] * 3, [a] * 3]]))
    return S, T, K


@pytest.mark.filterwarnings("ignore:autourdf_amd.prefer_device_kernargs")     # main() in this process: the runtime is up already
def test_command_line_fit_positions(golden, tmp_path, monkeypatch, capsys):
    """--cloud_fit --fit_positions on fixture a: fitted_positions.npy has joint_positions.npy's shape, every frame's rms after is
    at most its rms before, and everything the command wrote without the flag keeps its bytes -- cloud_fit.json gains only the
    "fitted" block -- with no pose-fit launch when the flag is absent."""
    from autourdf_amd import coord_map, ops
    robot, cams, step = "testbot", 20, 4
    S, T, K = _layout(tmp_path, golden, robot, cams, step)
    out_dir = tmp_path / f"data/urdf/{robot}_{K}_seg"
    stem = f"{step}_deg_{cams}_cams"
    monkeypatch.chdir(tmp_path)
    base = ["--robot", robot, "--unknown_dof", "--end_video", "2", "--voxel_size", "0.01", "--joint_limits", "--cloud_fit", "--fit_max", "0.05"]
    monkeypatch.setattr(ops, "pose_fit_system", lambda *a, **k: pytest.fail("pose_fit_system called without --fit_positions"))
    coord_map.main(base)
    before = {name: (out_dir / name).read_bytes() for name in sorted(os.listdir(out_dir))}
    assert sorted(before) == [stem + ".cloud_fit.json", stem + ".joint_motion.json", stem + ".joint_positions.npy", stem + ".urdf"]
    monkeypatch.undo()
    monkeypatch.chdir(tmp_path)
    capsys.readouterr()
    coord_map.main(base + ["--fit_positions", "--fit_iters", "6"])
    text = capsys.readouterr().out
    after = {name: (out_dir / name).read_bytes() for name in sorted(os.listdir(out_dir))}
    assert sorted(after) == sorted(list(before) + [stem + ".fitted_positions.npy"])
    for name in before:
        if not name.endswith(".cloud_fit.json"):
            assert after[name] == before[name], name
    report = json.loads(after[stem + ".cloud_fit.json"])
    fitted = report.pop("fitted")
    assert report == json.loads(before[stem + ".cloud_fit.json"])
    registered, fit = np.load(out_dir / (stem + ".joint_positions.npy")), np.load(out_dir / (stem + ".fitted_positions.npy"))
    assert fit.shape == registered.shape == (registered.shape[0], S, T) and fit.dtype == np.float64 and np.isfinite(fit).all()
    assert len(fitted["frames"]) == S * T and len(fitted["sequences"]) == S and len(fitted["joints"]) == registered.shape[0]
    for i, f in enumerate(fitted["frames"]):
        assert (f["sequence"], f["step"]) == (i // T, i % T) and 0 <= f["iterations"] <= 6
        assert f["rms_after"] <= f["rms_before"]
    assert fitted["all"]["rms_after"] <= fitted["all"]["rms_before"]
    for j, row in enumerate(fitted["joints"]):
        assert row["max_shift"] == float(np.abs(fit[j] - registered[j]).max())
    print("fit_positions on fixture a:", fitted["all"], [round(r["max_shift"], 4) for r in fitted["joints"]])
    lines = text.splitlines()
    assert sum(x.startswith("fit_positions seq") and "->" in x for x in lines) == S
    assert sum(x.startswith("fit_positions joint_") for x in lines) == registered.shape[0]
    assert text.index("cloud_fit seq0") < text.index("fit_positions seq0")    # it runs after the cloud fit
    # the keys of parameters.json: fit_positions without the cloud fit, a fit_iters without fit_positions: before anything is written
    for name in after:
        os.remove(out_dir / name)
    for entry, word in (({"fit_positions": True, "voxel_size": 0.01}, "cloud_fit"), ({"cloud_fit": True, "fit_iters": 3, "voxel_size": 0.01}, "fit_positions"),
                        ({"cloud_fit": True, "fit_positions": True, "fit_iters": -1, "voxel_size": 0.01}, "fit_iters")):
        (tmp_path / "parameters.json").write_text(json.dumps({robot: dict({"num_seg": K, "dof": 5}, **entry)}))
        with pytest.raises(ValueError, match=word):
            coord_map.main(["--robot", robot, "--unknown_dof", "--end_video", "2", "--joint_limits"])
        assert os.listdir(out_dir) == []
