"""creg_link_moments_f64 on the GPU against the numpy restatement of its contract (tests/_link_moments_ref.py): values within the
summation bound, exact counts, the pose-fit kernel's system from the moments, determinism in the bits, the argument errors; the
bundle adjustment (SimEnv.refine_joints) against the restatement's driver, the zero pose, an unobserved frame; and the command
line's --refine_joints on fixture a."""
import ctypes
import json
import os
import sys

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu
HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import _collide_ref as ref  # noqa: E402
import _link_moments_ref as lm  # noqa: E402
import _point_mesh_ref as pref  # noqa: E402
import _pose_fit_ref as pf  # noqa: E402
from test_gpu_pose_fit import _layout  # noqa: E402

INF = np.inf


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
    sc = lm.moments_scene(env.robot)
    d = {k: dev(sc[k]) for k in ("tri", "tri_start", "link_T", "pts", "pt_start", "center", "ref")}
    _, idx, _ = ops.point_mesh_distance(d["tri"], d["tri_start"], d["link_T"], d["pts"], d["pt_start"], sc["d_max"])
    idx = idx.clone()
    idx[sc["drop"]] = -1
    d["tri_idx"] = idx
    got = ops.link_moments(d["tri"], d["tri_start"], d["link_T"], d["pts"], d["pt_start"], idx, d["ref"], sc["d_max"])
    want = lm.moments(sc["tri"], sc["tri_start"], sc["link_T"], sc["pts"], sc["pt_start"], idx.cpu().numpy(), sc["ref"], sc["d_max"])
    return sc, d, [g.cpu().numpy() for g in got], want


def test_moments_against_the_restatement(scene):
    """Eight poses of the toy robot: the pose-fit scene's five (a NaN row, a row beyond d_max, a dropped correspondence, an empty
    pose, a pose touching one link), one of 330 rows (six tiles: all four running sums and the tail), one of exactly 64 rows and
    one of 65.  cnt exact; every sum within (2 n + 8) 2^-53 sum |term| of the long-double value, n the pair's count: at most n
    additions inside tiles, at most n non-zero partials, three additions to combine, and the terms' own roundings."""
    sc, _, (mom, cnt), want = scene
    assert mom.shape == (8, 5, 16) and cnt.shape == (8, 5) and cnt.dtype == np.int64
    counts = np.bincount(want["case"][want["ok"]], minlength=8)[1:]
    assert (counts >= 2).all(), dict(zip(pf.CASES, counts))                   # all seven pt_tri2 cases among the contributing rows
    assert not want["ok"][[sc["nan_row"], sc["far_row"], sc["drop"]]].any()
    sizes = np.diff(sc["pt_start"])
    assert list(sizes[[2, 5, 6, 7]]) == [0, 330, 64, 65]
    np.testing.assert_array_equal(cnt, want["cnt"])
    assert list(cnt.sum(1)[:4]) == [253, 254, 0, 254] and (cnt[4, 1:] == 0).all() and cnt[4, 0] > 50
    assert cnt[5].sum() > 300 and cnt[6].sum() == 64 and cnt[7].sum() == 65 and (cnt[[0, 1, 3, 5]] > 0).all()
    bound = (2.0 * cnt[:, :, None] + 8.0) * lm.EPS * want["mom_abs"]
    err = np.abs(mom - want["mom"])
    assert (err <= bound).all(), float((err - bound).max())
    with np.errstate(invalid="ignore", divide="ignore"):
        worst = float(np.nanmax(np.where(bound > 0, err / bound, 0.0)))
    print(f"largest |kernel - long double| / bound over all sums: {worst:.3g}")
    assert (mom[cnt == 0] == 0.0).all() and (mom[2] == 0.0).all()               # every (p, l) is written, zeros where nothing contributes
    assert (mom[cnt > 0][:, 15] > 0).all()


def test_pose_fit_system_from_the_moments(scene):
    """The pose-only H, g assembled from the kernel's moments (about center_p) against ops.pose_fit_system on the same input: they
    agree to the sum of both sides' bounds -- the pose-fit test's (n + 64) 2^-53 sum |term|, and (2 n + 56) 2^-53 sum_l
    |Tw_a|^T |M|_abs |Tw_b| for the moments and their assembly -- and sum_l cnt is its n."""
    from autourdf_amd import ops
    from autourdf_amd.compute_joints import link_twists, twist_system
    sc, d, _, _ = scene
    table = {k: v for k, v in sc["table"].items() if not k.startswith("_dev")}
    P, L, J = 8, 5, 4
    cref = d["center"][:, None, :].expand(P, L, 3).contiguous()
    mom, cnt = ops.link_moments(d["tri"], d["tri_start"], d["link_T"], d["pts"], d["pt_start"], d["tri_idx"], cref, sc["d_max"])
    Tw = link_twists(table, d["link_T"], torch.zeros(P, J, dtype=torch.float64, device="cuda"), d["center"], cref, structure=False)
    assert tuple(Tw.shape) == (P, L, 6, 6 + J)
    H, g, cost = (x.cpu().numpy() for x in twist_system(mom, cnt, Tw))
    Hk, gk, ck, nk = (x.cpu().numpy() for x in ops.pose_fit_system(d["tri"], d["tri_start"], d["link_T"], d["pts"], d["pt_start"],
                                                                    d["tri_idx"], table, d["center"], sc["d_max"]))
    np.testing.assert_array_equal(cnt.cpu().numpy().sum(1), nk)
    idx = d["tri_idx"].cpu().numpy()
    want = pf.system(sc["tri"], sc["tri_start"], sc["link_T"], sc["pts"], sc["pt_start"], idx, table, sc["center"], sc["d_max"])
    ours = lm.moments(sc["tri"], sc["tri_start"], sc["link_T"], sc["pts"], sc["pt_start"], idx, cref.cpu().numpy(), sc["d_max"])
    chain = pf.chains(table)
    worst = 0.0
    for p in range(P):
        Twp = lm.twists(table, chain, sc["link_T"][p], np.zeros(J), sc["center"][p], cref[p].cpu().numpy())[:, :, :6 + J]
        np.testing.assert_allclose(Tw[p].cpu().numpy(), Twp, rtol=0, atol=1e-14)
        Ha, ga, _ = lm.assemble(ours["mom_abs"][p], ours["cnt"][p], Twp, absolute=True)
        n = float(nk[p])
        for name, a, b, s1, s2 in (("H", H[p], Hk[p], want["H_abs"][p], Ha), ("g", g[p], gk[p], want["g_abs"][p], ga),
                                   ("cost", cost[p], ck[p], want["cost_abs"][p], want["cost_abs"][p])):
            err, bound = np.abs(a - b), (n + 64) * lm.EPS * s1 + (2 * n + 56) * lm.EPS * s2
            assert (err <= bound).all(), (p, name, float(np.max(err - bound)))
            with np.errstate(invalid="ignore", divide="ignore"):
                worst = max(worst, float(np.nanmax(np.where(bound > 0, err / bound, 0.0))))
    print(f"largest |assembled - pose-fit kernel| / bound: {worst:.3g}")
    assert (H[2] == 0).all() and (g[2] == 0).all()


def test_two_runs_a_pose_alone_and_other_links_removed_give_the_same_bits(scene):
    from autourdf_amd import ops
    sc, d, first, want = scene
    args = (d["tri"], d["tri_start"], d["link_T"], d["pts"], d["pt_start"])
    again = [x.cpu().numpy() for x in ops.link_moments(*args, d["tri_idx"], d["ref"], sc["d_max"])]
    for a, b in zip(first, again):
        np.testing.assert_array_equal(bits(a), bits(b))
    for p in (1, 5):
        s, e = int(sc["pt_start"][p]), int(sc["pt_start"][p + 1])
        alone = ops.link_moments(d["tri"], d["tri_start"], d["link_T"][p:p + 1].contiguous(), d["pts"][s:e].contiguous(),
                                 dev(np.array([0, e - s], np.int64)), d["tri_idx"][s:e].contiguous(), d["ref"][p:p + 1].contiguous(), sc["d_max"])
        for a, b in zip(first, alone):
            np.testing.assert_array_equal(bits(a[p]), bits(b.cpu().numpy()[0]))
    # a pose that starts in the middle of the tiles of the call (pose 7 starts at a row that is no multiple of 64)
    assert sc["pt_start"][7] % 64 != 0
    # all rows of the other links removed from tri_idx: link 2's sums keep their bits, the others become zero
    idx = d["tri_idx"].clone()
    link = torch.as_tensor(want["link"], device="cuda")
    idx[link != 2] = -1
    mom, cnt = (x.cpu().numpy() for x in ops.link_moments(*args, idx, d["ref"], sc["d_max"]))
    np.testing.assert_array_equal(bits(mom[:, 2]), bits(first[0][:, 2]))
    np.testing.assert_array_equal(cnt[:, 2], first[1][:, 2])
    assert (first[1][:, 2] > 0).sum() >= 4 and (mom[:, [0, 1, 3, 4]] == 0.0).all() and (cnt[:, [0, 1, 3, 4]] == 0).all()


def test_argument_errors_return_einval_and_write_nothing(scene):
    from autourdf_amd import _lib, ops
    sc, d, _, _ = scene
    lib = _lib.load()
    ptr = lambda t: ctypes.c_void_p(t.data_ptr())
    P, L, F, N = 8, 5, len(sc["tri"]), len(sc["pts"])
    need = lib.creg_link_moments_workspace_bytes(P, N, L)
    ws = torch.zeros(need // 8, dtype=torch.float64, device="cuda")
    outs = [torch.full((P, L, 16), -7.0, dtype=torch.float64, device="cuda"), torch.full((P, L), -7, dtype=torch.int64, device="cuda")]

    def call(d_max=sc["d_max"], ws_bytes=need, n_links=L, ref=d["ref"], n_pts=N):
        return lib.creg_link_moments_f64(ptr(d["tri"]), ptr(d["tri_start"]), F, ptr(d["link_T"]), n_links, P, ptr(d["pts"]), ptr(d["pt_start"]),
                                         n_pts, d_max, ptr(d["tri_idx"]), None if ref is None else ptr(ref), *[ptr(o) for o in outs], ptr(ws),
                                         ws_bytes, None)

    for kw in (dict(d_max=float("nan")), dict(d_max=-0.5), dict(ws_bytes=need - 1), dict(n_links=0), dict(ref=None), dict(n_pts=-1)):
        assert call(**kw) == -1, kw
        assert b"creg_link_moments_f64" in lib.creg_last_error()
        torch.cuda.synchronize()
        assert all(bool((o == -7).all()) for o in outs) and bool((ws == 0).all()), kw
    assert call() == 0                                                          # the same buffers, everything in order
    torch.cuda.synchronize()
    assert bool((outs[1] >= 0).all())
    # the wrapper: before any launch
    args = (d["tri"], d["tri_start"], d["link_T"], d["pts"], d["pt_start"], d["tri_idx"])
    for bad in (float("nan"), -1.0):
        with pytest.raises(ValueError, match="d_max"):
            ops.link_moments(*args, d["ref"], bad)
    with pytest.raises(ValueError, match="expected"):
        ops.link_moments(*args, d["ref"][:, :4].contiguous(), 0.1)
    with pytest.raises(ValueError, match="expected"):
        ops.link_moments(*args[:5], d["tri_idx"][:-1].contiguous(), d["ref"], 0.1)
    with pytest.raises(TypeError):
        ops.link_moments(*args[:5], d["tri_idx"].to(torch.int64), d["ref"], 0.1)
    # no triangles and no points: zeros
    mom, cnt = ops.link_moments(d["tri"][:0].contiguous(), torch.zeros(6, dtype=torch.int64, device="cuda"), d["link_T"], d["pts"][:0].contiguous(),
                                torch.zeros(9, dtype=torch.int64, device="cuda"), d["tri_idx"][:0].contiguous(), d["ref"], 0.1)
    assert bool((mom == 0).all()) and bool((cnt == 0).all())


@pytest.fixture(scope="module")
def refined(env):
    r = env.robot
    c = lm.refine_case(r)
    want = lm.refine(r.tri, r.tri_start, c["table"], c["clouds"], c["q0"], None, INF, lm.REFINE_ITERS, False, c["lock"], c["lock_frames"])
    got = env.refine_joints(c["clouds"], c["q0"], d_max=INF, max_iter=lm.REFINE_ITERS, fit_base=False, lock=c["lock"],
                            lock_frames=c["lock_frames"])
    return c, got, want


def test_driver_against_the_restatement_driver(env, refined):
    """The toy robot against clouds of the robot whose shoulder frame is off by 0.03 rad about u1 and 4 mm along u2: 8 poses, 400
    noise-free surface samples each, q0 = q*, the base and the wrist (position and frame) locked.  The cost history never rises;
    the shoulder's axis angle and line distance to the truth both end lower than they started, and each is at most 2 x what the
    restatement's host driver reaches with the same settings (one accept / reject decision flipped by rounding moves lambda by
    a factor of 10 for one iteration)."""
    c, got, want = refined
    h = got["cost_history"]
    a0, d0 = lm.shoulder_errors(c, c["table"]["origin"])
    ag, dg = lm.shoulder_errors(c, got["origin"])
    aw, dw = lm.shoulder_errors(c, want["origin"])
    print(f"shoulder axis angle {a0:.6g} -> kernel driver {ag:.6g}, restatement driver {aw:.6g} rad; line distance {d0:.6g} -> "
          f"{dg:.6g}, {dw:.6g}; cost {h[0]:.6g} -> {h[-1]:.6g} in {got['iterations']} steps, restatement {want['cost_history'][-1]:.6g} "
          f"in {want['iterations']}")
    assert all(b <= a for a, b in zip(h, h[1:])) and len(h) == got["iterations"] + 1 and h[-1] < h[0]
    assert aw < a0 and dw < d0                                                  # the restatement's driver lowers both
    assert ag < a0 and dg < d0
    assert ag <= 2.0 * aw and dg <= 2.0 * dw
    assert got["names"] == list(c["table"]["names"]) and got["frames"].shape == (4, 4, 4) and got["q"].shape == (8, 4)
    w = got["names"].index("wrist")
    np.testing.assert_array_equal(got["frames"][w], np.eye(4))
    np.testing.assert_array_equal(bits(got["q"][:, w]), bits(c["q0"][:, w]))
    np.testing.assert_array_equal(got["base"], np.tile(np.eye(4), (8, 1, 1)))
    assert not got["unobserved_frames"].any() and (got["n"] == 400).all()


def test_zero_pose_is_kept_and_the_written_urdf_reproduces_the_result(env, refined):
    """After the driver's steps the posed triangles at q = 0 equal the start's to 1e-12 of the bounding-box diagonal, and the robot
    reloaded from set_joint_frames(..., result["frames"]) reproduces the driver's final link_T-posed triangles to 1e-9 of it."""
    from autourdf_amd.compute_joints import set_joint_frames
    from autourdf_amd.sim_data import UrdfRobot
    c, got, _ = refined
    r, table = env.robot, c["table"]
    zero = np.zeros(4)
    start = pref.posed_mesh(r.tri, r.tri_start, pf.fk(table, zero, np.eye(4)))
    diag = float(np.linalg.norm(start.reshape(-1, 3).max(0) - start.reshape(-1, 3).min(0)))
    after = pref.posed_mesh(got["tri"], r.tri_start, pf.fk(dict(table, origin=got["origin"]), zero, np.eye(4)))
    assert np.abs(after - start).max() <= 1e-12 * diag
    assert np.abs(got["tri"] - r.tri).max() > 1e-6                              # the link-frame triangles did move
    path = os.path.join(os.path.dirname(r.path), "refined.urdf")                 # beside the toy: its mesh names are relative
    set_joint_frames(r.path, {n: got["frames"][j] for j, n in enumerate(got["names"])}, path)
    again = UrdfRobot(path)
    t2 = again.fk_table()
    assert list(t2["names"]) == got["names"]
    worst = 0.0
    for p in range(len(got["q"])):
        mine = pref.posed_mesh(got["tri"], r.tri_start, got["link_T"][p])
        theirs = pref.posed_mesh(again.tri, again.tri_start, got["base"][p] @ pf.fk(t2, got["q"][p], np.eye(4)))
        worst = max(worst, float(np.abs(mine - theirs).max()))
    print(f"reloaded URDF against the driver's final posed triangles: {worst:.3g} (diagonal {diag:.3g})")
    assert worst <= 1e-9 * diag


def test_a_frame_that_never_left_zero_is_reported_and_its_origin_keeps_its_bits(env):
    c = lm.unobserved_case(env.robot)
    got = env.refine_joints(c["clouds"], c["q0"], d_max=INF, max_iter=3, fit_base=False, lock=c["lock"], lock_frames=c["lock_frames"])
    j = c["joint"]
    assert got["unobserved_frames"][j].all() and not got["unobserved_frames"][[1, 2]][:, :2].any() and not got["unobserved_frames"][1].any()
    np.testing.assert_array_equal(bits(got["origin"][j]), bits(np.asarray(c["table"]["origin"])[j]))
    np.testing.assert_array_equal(got["frames"][j], np.eye(4))
    assert (got["q"][:, j] == 0.0).all()
    assert not np.array_equal(got["frames"][1], np.eye(4))                      # the shoulder's frame did step
    h = got["cost_history"]
    assert all(b <= a for a, b in zip(h, h[1:])) and h[-1] < h[0]


@pytest.mark.filterwarnings("ignore:autourdf_amd.prefer_device_kernargs")     # main() in this process: the runtime is up already
def test_command_line_refine_joints(golden, tmp_path, monkeypatch, capsys):
    """--cloud_fit --refine_joints on fixture a: the refined URDF loads, refined_positions.npy has joint_positions.npy's shape,
    the overall rms does not rise, the original URDF and everything else the command wrote without the flag keep their bytes --
    cloud_fit.json gains only the "refined" block -- with no link-moments launch when the flag is absent."""
    from autourdf_amd import coord_map, ops
    from autourdf_amd.sim_data import UrdfRobot
    robot, cams, step = "testbot", 20, 4
    S, T, K = _layout(tmp_path, golden, robot, cams, step)
    out_dir = tmp_path / f"data/urdf/{robot}_{K}_seg"
    stem = f"{step}_deg_{cams}_cams"
    monkeypatch.chdir(tmp_path)
    base = ["--robot", robot, "--unknown_dof", "--end_video", "2", "--voxel_size", "0.01", "--joint_limits", "--cloud_fit", "--fit_max", "0.05"]
    monkeypatch.setattr(ops, "link_moments", lambda *a, **k: pytest.fail("link_moments called without --refine_joints"))
    coord_map.main(base)
    before = {name: (out_dir / name).read_bytes() for name in sorted(os.listdir(out_dir))}
    assert sorted(before) == [stem + ".cloud_fit.json", stem + ".joint_motion.json", stem + ".joint_positions.npy", stem + ".urdf"]
    monkeypatch.undo()
    monkeypatch.chdir(tmp_path)
    capsys.readouterr()
    coord_map.main(base + ["--refine_joints", "--refine_iters", "5"])
    text = capsys.readouterr().out
    after = {name: (out_dir / name).read_bytes() for name in sorted(os.listdir(out_dir))}
    assert sorted(after) == sorted(list(before) + [stem + ".refined.urdf", stem + ".refined_positions.npy"])
    for name in before:
        if not name.endswith(".cloud_fit.json"):
            assert after[name] == before[name], name
    report = json.loads(after[stem + ".cloud_fit.json"])
    refined = report.pop("refined")
    assert report == json.loads(before[stem + ".cloud_fit.json"])
    registered, fit = np.load(out_dir / (stem + ".joint_positions.npy")), np.load(out_dir / (stem + ".refined_positions.npy"))
    assert fit.shape == registered.shape == (registered.shape[0], S, T) and fit.dtype == np.float64 and np.isfinite(fit).all()
    loaded = UrdfRobot(str(out_dir / (stem + ".refined.urdf")))
    original = UrdfRobot(str(out_dir / (stem + ".urdf")))
    assert loaded.links == original.links and [j["name"] for j in loaded.joints] == [j["name"] for j in original.joints]
    assert len(loaded.tri) == len(original.tri)
    assert 0 <= refined["iterations"] <= 5 and refined["all"]["rms_after"] <= refined["all"]["rms_before"]
    assert refined["urdf"].endswith(stem + ".refined.urdf") and len(refined["joints"]) == registered.shape[0]
    for j, row in enumerate(refined["joints"]):
        assert row["max_shift"] == float(np.abs(fit[j] - registered[j]).max()) and row["axis_angle"] >= 0.0
    print("refine_joints on fixture a:", refined["all"], [(round(r["axis_angle"], 5), r["line_distance"]) for r in refined["joints"]])
    lines = text.splitlines()
    assert sum(x.startswith("refine_joints joint_") for x in lines) == registered.shape[0]
    assert sum(x.startswith("refine_joints: rms") and "->" in x for x in lines) == 1
    assert text.index("cloud_fit seq0") < text.index("refine_joints: rms")      # it runs after the cloud fit
    # the keys of parameters.json: refine_joints without the cloud fit, a refine_iters without refine_joints: before anything is written
    for name in after:
        os.remove(out_dir / name)
    for entry, word in (({"refine_joints": True, "voxel_size": 0.01}, "cloud_fit"), ({"cloud_fit": True, "refine_iters": 3, "voxel_size": 0.01}, "refine_joints"),
                        ({"cloud_fit": True, "refine_joints": True, "refine_iters": -1, "voxel_size": 0.01}, "refine_iters")):
        (tmp_path / "parameters.json").write_text(json.dumps({robot: dict({"num_seg": K, "dof": 5}, **entry)}))
        with pytest.raises(ValueError, match=word):
            coord_map.main(["--robot", robot, "--unknown_dof", "--end_video", "2", "--joint_limits"])
        assert os.listdir(out_dir) == []
