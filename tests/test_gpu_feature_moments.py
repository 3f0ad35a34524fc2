"""creg_feature_moments_f64 on the GPU against the numpy restatement of its contract (tests/_feature_moments_ref.py): mom and cnt
bit for bit the link-moments entry's, the 21 sums within the summation bound, degenerate triangles, a link count past one trip of
256, determinism in the bits, workspace hygiene, the argument errors; the two drivers with metric="feature" (SimEnv.fit_pose,
SimEnv.refine_joints) against the restatement's drivers; and the command line's --fit_metric on fixture a."""
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
import _feature_moments_ref as fm  # noqa: E402
import _fit_edges as fe  # noqa: E402
import _link_moments_ref as lm  # noqa: E402
import _point_mesh_ref as pref  # noqa: E402
import _pose_fit_ref as pf  # noqa: E402
from test_gpu_pose_fit import _layout  # noqa: E402

INF = np.inf
FLOOR = 1e-12                                                    # both drivers end at rounding (7e-17 on a 0.6-wide robot): four orders above


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def bits(a):
    return np.ascontiguousarray(a).view(np.int64)


def on_a_grid(clouds):
    """The clouds rounded to multiples of 2^-20.  The drivers take every pose's centre -- the point the moments are about -- from a
    torch index_add_, whose order of additions is not fixed; on such coordinates every partial sum of 400 points is exact, so the
    centre, and with it every bit the drivers compute from the kernels, is the same in two runs.  (The costs are index_add_ sums
    too: their last bit only enters the accept test, which is no tie in the first steps.)"""
    return [np.round(np.asarray(x, np.float64) * 2.0 ** 20) / 2.0 ** 20 for x in clouds]


def call(case, idx=None, metric="feature"):
    """ops.link_moments on a dict of host arrays -> host arrays."""
    from autourdf_amd import ops
    idx = case["tri_idx"] if idx is None else idx
    out = ops.link_moments(dev(case["tri"]), dev(case["tri_start"]), dev(case["link_T"]), dev(case["pts"]), dev(case["pt_start"]),
                           dev(np.asarray(idx, np.int32)), dev(case["ref"]), case["d_max"], metric=metric)
    return [x.cpu().numpy() for x in out]


def within_bound(fmom, want):
    """fmom within (2 n + 8) 2^-53 sum |term| of the long-double sums -> the worst ratio."""
    bound = (2.0 * want["cnt"][:, :, None] + 8.0) * fm.EPS * want["fmom_abs"]
    err = np.abs(fmom - want["fmom"])
    assert (err <= bound).all(), float((err - bound).max())
    with np.errstate(invalid="ignore", divide="ignore"):
        return float(np.nanmax(np.where(bound > 0, err / bound, 0.0)))


@pytest.fixture(scope="module")
def env(tmp_path_factory):
    return ref.toy(tmp_path_factory.mktemp("toy"))


@pytest.fixture(scope="module")
def scene(env):
    """lm.moments_scene on the device, the correspondences of the point-mesh entry (one of them removed), the entry's answer, the
    sibling's and the restatement's."""
    from autourdf_amd import ops
    sc = lm.moments_scene(env.robot)
    d = {k: dev(sc[k]) for k in ("tri", "tri_start", "link_T", "pts", "pt_start", "center", "ref")}
    _, idx, _ = ops.point_mesh_distance(d["tri"], d["tri_start"], d["link_T"], d["pts"], d["pt_start"], sc["d_max"])
    idx = idx.clone()
    idx[sc["drop"]] = -1
    d["tri_idx"] = idx
    args = (d["tri"], d["tri_start"], d["link_T"], d["pts"], d["pt_start"], idx, d["ref"], sc["d_max"])
    got = [x.cpu().numpy() for x in ops.link_moments(*args, metric="feature")]
    sibling = [x.cpu().numpy() for x in ops.link_moments(*args)]
    want = fm.moments(sc["tri"], sc["tri_start"], sc["link_T"], sc["pts"], sc["pt_start"], idx.cpu().numpy(), sc["ref"], sc["d_max"])
    return sc, d, got, sibling, want


def test_sibling_bits_and_the_sums_against_the_restatement(scene):
    """Eight poses of the toy robot (0, 64, 65 and 330 rows among them, a pose starting mid-tile, five links, all seven cases among
    the contributing rows).  mom and cnt carry the bits of ops.link_moments' default.  Every one of the 21 sums within
    (2 n + 8) 2^-53 sum |term| of the long-double value, n the pair's count: at most n additions inside tiles, at most n non-zero
    partials, three additions to combine -- the terms themselves have the kernel's bits."""
    sc, _, (mom, cnt, fmom), (mom0, cnt0), want = scene
    assert fmom.shape == (8, 5, 21) and fmom.dtype == np.float64
    np.testing.assert_array_equal(bits(mom), bits(mom0))
    np.testing.assert_array_equal(cnt, cnt0)
    np.testing.assert_array_equal(cnt, want["cnt"])
    counts = np.bincount(want["case"][want["ok"]], minlength=8)[1:]
    assert (counts >= 2).all(), dict(zip(pf.CASES, counts))
    assert list(np.diff(sc["pt_start"])[[2, 5, 6, 7]]) == [0, 330, 64, 65] and sc["pt_start"][7] % 64 != 0
    worst = within_bound(fmom, want)
    print(f"largest |kernel - long double| / bound over the 21 sums: {worst:.3g}")
    assert (fmom[cnt == 0] == 0.0).all() and (fmom[2] == 0.0).all()             # every (p, l) is written, zeros where nothing contributes
    diag = [fm.UPPER.index((a, a)) for a in range(6)]
    assert (fmom[cnt > 0][:, diag] >= 0).all() and (fmom[cnt > 0][:, diag[3:]].sum(1) > 0).all()
    assert (fmom[..., diag[3:]].sum(-1) <= 3.0 * cnt + 1e-9).all()              # tr Pi <= 3 per row


def test_degenerate_triangles_take_the_guards():
    """The zero-area rows of fm.degenerate_case -- collinear, coincident, and a = b with c apart, whose edge ab has no length: the
    ee > 0 guard -- match the restatement; everything is finite."""
    d = fm.degenerate_case()
    want = fm.moments(d["tri"], d["tri_start"], d["link_T"], d["pts"], d["pt_start"], d["tri_idx"], d["ref"], d["d_max"])
    guard = (d["tri_idx"] == 3) & (want["case"] == 4)
    assert guard.any() and (want["Pi"][guard] == np.eye(3)).all() and (want["case"][d["tri_idx"] == 2] == 1).all()
    mom, cnt, fmom = call(d)
    mom0, cnt0 = call(d, metric="point")
    np.testing.assert_array_equal(bits(mom), bits(mom0))
    np.testing.assert_array_equal(cnt, want["cnt"])
    assert list(cnt[0]) == [3, 10] and np.isfinite(fmom).all()
    print(f"degenerate rows, worst ratio {within_bound(fmom, want):.3g}")
    # the rows of the coincident and the a = b triangle alone: Pi = I on each, so the 21 sums are those of A^T A
    only = np.where(np.isin(d["tri_idx"], (2,)) | guard, d["tri_idx"], -1)
    _, cnt1, f1 = call(d, only)
    w1 = fm.moments(d["tri"], d["tri_start"], d["link_T"], d["pts"], d["pt_start"], only, d["ref"], d["d_max"])
    assert cnt1[0, 1] == 3 + guard.sum() and f1[0, 1, fm.UPPER.index((3, 3))] == cnt1[0, 1] and f1[0, 1, fm.UPPER.index((3, 4))] == 0.0
    within_bound(f1, w1)


@pytest.mark.parametrize("links", [7, fe.N_LINKS])
def test_link_counts_past_one_trip_of_256(links):
    """7 and 59 links of the edge suite's chain robot: 266 and 2242 (link, entry) pairs, two and nine trips of the 256 threads.
    Poses of 70, 130, 1 and 0 rows with the suite's rows without correspondence and its NaN row."""
    case = fe.cut_links(fe.make_case(fe.chain_robot(), (70, 130, 1, 0), 105), links)
    want = fm.moments(case["tri"], case["tri_start"], case["link_T"], case["pts"], case["pt_start"], case["tri_idx"], case["ref"], case["d_max"])
    mom, cnt, fmom = call(case)
    mom0, cnt0 = call(case, metric="point")
    np.testing.assert_array_equal(bits(mom), bits(mom0))
    np.testing.assert_array_equal(cnt, cnt0)
    np.testing.assert_array_equal(cnt, want["cnt"])
    assert (cnt.sum(0) > 0).all() if links == 7 else (cnt.sum(0) > 0).sum() > 50       # links in both trips, and in the last one
    assert cnt[:, 256 * ((links * 38 - 1) // 256) // 38:].sum() > 0 and not want["ok"][case["bad_rows"]].any()
    print(f"{links} links, worst ratio {within_bound(fmom, want):.3g}")
    assert (fmom[cnt == 0] == 0.0).all()


def test_two_runs_a_pose_alone_and_other_links_removed_give_the_same_bits(scene):
    from autourdf_amd import ops
    sc, d, first, _, want = scene
    args = (d["tri"], d["tri_start"], d["link_T"], d["pts"], d["pt_start"])
    again = [x.cpu().numpy() for x in ops.link_moments(*args, d["tri_idx"], d["ref"], sc["d_max"], metric="feature")]
    for a, b in zip(first, again):
        np.testing.assert_array_equal(bits(a), bits(b))
    for p in (1, 5, 7):
        s, e = int(sc["pt_start"][p]), int(sc["pt_start"][p + 1])
        alone = ops.link_moments(d["tri"], d["tri_start"], d["link_T"][p:p + 1].contiguous(), d["pts"][s:e].contiguous(),
                                 dev(np.array([0, e - s], np.int64)), d["tri_idx"][s:e].contiguous(), d["ref"][p:p + 1].contiguous(), sc["d_max"],
                                 metric="feature")
        for a, b in zip(first, alone):
            np.testing.assert_array_equal(bits(a[p]), bits(b.cpu().numpy()[0]))
    idx = d["tri_idx"].clone()
    idx[torch.as_tensor(want["link"], device="cuda") != 2] = -1
    mom, cnt, fmom = (x.cpu().numpy() for x in ops.link_moments(*args, idx, d["ref"], sc["d_max"], metric="feature"))
    np.testing.assert_array_equal(bits(fmom[:, 2]), bits(first[2][:, 2]))
    np.testing.assert_array_equal(bits(mom[:, 2]), bits(first[0][:, 2]))
    assert (first[1][:, 2] > 0).sum() >= 4 and (fmom[:, [0, 1, 3, 4]] == 0.0).all() and (cnt[:, [0, 1, 3, 4]] == 0).all()


def _raw(lib, d, sc, outs, ws, ws_bytes, **kw):
    ptr = lambda t: None if t is None else ctypes.c_void_p(t.data_ptr())
    a = dict(d_max=sc["d_max"], n_links=5, ref=d["ref"], n_pts=len(sc["pts"]), fmom=outs[2])
    a.update(kw)
    return lib.creg_feature_moments_f64(ptr(d["tri"]), ptr(d["tri_start"]), len(sc["tri"]), ptr(d["link_T"]), a["n_links"], 8, ptr(d["pts"]),
                                        ptr(d["pt_start"]), a["n_pts"], a["d_max"], ptr(d["tri_idx"]), ptr(a["ref"]), ptr(outs[0]), ptr(outs[1]),
                                        ptr(a["fmom"]), ptr(ws), ws_bytes, None)


def test_workspace_and_outputs_prefilled_with_nan(scene):
    """The entry on a workspace and outputs filled with a NaN pattern, each with a guard behind it: the results carry the bits of
    the wrapper's call (no slot is read that the call did not write: a NaN would spread into a sum), and the guards keep the
    pattern (nothing is written past the stated sizes)."""
    from autourdf_amd import _lib
    sc, d, first, _, _ = scene
    lib = _lib.load()
    P, L, N, GUARD = 8, 5, len(sc["pts"]), 64
    need = lib.creg_feature_moments_workspace_bytes(P, N, L)
    assert need == (8 * ((N >> 6) + P) * L * 38 + 255) // 256 * 256
    pattern = torch.tensor([-2251799813685247], dtype=torch.int64, device="cuda")           # 0xFFF8000000000001: a NaN with a payload
    filled = lambda n: pattern.repeat(n + GUARD)
    ws = filled(need // 8)
    outs = [filled(P * L * 16), filled(P * L), filled(P * L * 21)]
    views = [outs[0].view(torch.float64), outs[1], outs[2].view(torch.float64)]
    assert bool(torch.isnan(views[0]).all())
    assert _raw(lib, d, sc, views, ws, need) == 0
    torch.cuda.synchronize()
    for o, n, want in zip(outs, (P * L * 16, P * L, P * L * 21), first):
        np.testing.assert_array_equal(o[:n].cpu().numpy(), bits(want).reshape(-1))
        assert bool((o[n:] == pattern).all())
    assert bool((ws[need // 8:] == pattern).all())
    used = (ws[:need // 8] != pattern)
    assert bool(used.any()) and not bool(torch.isnan(ws[:need // 8].view(torch.float64)[used]).any())


def test_argument_errors_return_einval_and_write_nothing(scene):
    from autourdf_amd import _lib, ops
    sc, d, _, _, _ = scene
    lib = _lib.load()
    P, L, N = 8, 5, len(sc["pts"])
    need = lib.creg_feature_moments_workspace_bytes(P, N, L)
    ws = torch.zeros(need // 8, dtype=torch.float64, device="cuda")
    outs = [torch.full((P, L, 16), -7.0, dtype=torch.float64, device="cuda"), torch.full((P, L), -7, dtype=torch.int64, device="cuda"),
            torch.full((P, L, 21), -7.0, dtype=torch.float64, device="cuda")]
    for kw in (dict(d_max=float("nan")), dict(d_max=-0.5), dict(ws_bytes=need - 1), dict(n_links=0), dict(ref=None), dict(fmom=None),
               dict(n_pts=-1)):
        ws_bytes = kw.pop("ws_bytes", need)
        assert _raw(lib, d, sc, outs, ws, ws_bytes, **kw) == -1, kw
        assert b"creg_feature_moments_f64" in lib.creg_last_error()
        torch.cuda.synchronize()
        assert all(bool((o == -7).all()) for o in outs) and bool((ws == 0).all()), kw
    assert _raw(lib, d, sc, outs, ws, need) == 0                                  # the same buffers, everything in order
    torch.cuda.synchronize()
    assert bool((outs[1] >= 0).all())
    args = (d["tri"], d["tri_start"], d["link_T"], d["pts"], d["pt_start"], d["tri_idx"])
    with pytest.raises(ValueError, match="metric"):
        ops.link_moments(*args, d["ref"], 0.1, metric="plane")
    with pytest.raises(ValueError, match="d_max"):
        ops.link_moments(*args, d["ref"], -1.0, metric="feature")
    with pytest.raises(ValueError, match="expected"):
        ops.link_moments(*args, d["ref"][:, :4].contiguous(), 0.1, metric="feature")
    out = ops.link_moments(d["tri"][:0].contiguous(), torch.zeros(6, dtype=torch.int64, device="cuda"), d["link_T"], d["pts"][:0].contiguous(),
                           torch.zeros(9, dtype=torch.int64, device="cuda"), d["tri_idx"][:0].contiguous(), d["ref"], 0.1, metric="feature")
    assert len(out) == 3 and all(bool((x == 0).all()) for x in out)             # no triangles and no points: zeros


# ------------------------------------------------------------------------------------------ the drivers
def test_fit_pose_with_the_feature_metric(env):
    """pf.driver_case through SimEnv.fit_pose(metric="feature"), 12 steps allowed: per pose the final rms and max |q - q*| over
    the free joints are at most max(2 x the restatement driver's, 1e-12) -- the factor for one flipped accept, the floor because
    both sides end at rounding -- and the rms is at most 1e-3 of the metric="point" run's.  Histories never rise.  The default
    metric gives the bits of a call without the argument."""
    r = env.robot
    c, want = fm.driver_run(r, "fit", "feature")
    kw = dict(d_max=INF, max_iter=fm.ITERS, fit_base=False, lock=c["lock"])
    got = env.fit_pose(c["clouds"], c["q0"], metric="feature", **kw)
    point = env.fit_pose(c["clouds"], c["q0"], **kw)
    for p in range(4):
        h = got["cost_history"][p]
        eg, ew = np.abs(got["q"][p] - c["q_true"][p])[c["free"]].max(), np.abs(want["q"][p] - c["q_true"][p])[c["free"]].max()
        print(f"pose {p}: feature {got['iterations'][p]} steps, rms {got['rms_before'][p]:.4g} -> {got['rms_after'][p]:.4g}, max |q - q*| {eg:.3g}; "
              f"restatement {want['iterations'][p]} steps, rms {want['rms_after'][p]:.4g}, max |q - q*| {ew:.3g}; point {point['iterations'][p]} "
              f"steps, rms {point['rms_after'][p]:.4g}, max |q - q*| {np.abs(point['q'][p] - c['q_true'][p])[c['free']].max():.3g}")
        assert all(b <= a for a, b in zip(h, h[1:])) and len(h) == got["iterations"][p] + 1 and h[-1] < h[0]
        assert got["rms_after"][p] <= max(2.0 * want["rms_after"][p], FLOOR)
        assert eg <= max(2.0 * ew, FLOOR)
        assert got["rms_after"][p] <= 1e-3 * point["rms_after"][p]
        locked = [j for j in range(4) if j not in c["free"]]
        np.testing.assert_array_equal(bits(got["q"][p][locked]), bits(c["q0"][p][locked]))
        np.testing.assert_array_equal(got["base"][p], np.eye(4))
        assert got["n"][p] == 400 and not got["unobserved"][p].any()
    named = env.fit_pose(on_a_grid(c["clouds"]), c["q0"], metric="point", **dict(kw, max_iter=3))
    plain = env.fit_pose(on_a_grid(c["clouds"]), c["q0"], **dict(kw, max_iter=3))
    for k in ("q", "base"):
        np.testing.assert_array_equal(bits(named[k]), bits(plain[k]))
    np.testing.assert_array_equal(named["iterations"], plain["iterations"])


def test_refine_joints_with_the_feature_metric(env):
    """lm.refine_case through SimEnv.refine_joints(metric="feature"), 12 steps allowed: the overall rms and both shoulder errors
    end at most max(2 x the restatement driver's, 1e-12), the rms at most 1e-3 of the metric="point" run's, the history never
    rises, and the posed triangles at q = 0 equal the start's to 1e-12 of the bounding-box diagonal."""
    r = env.robot
    c, want = fm.driver_run(r, "refine", "feature")
    kw = dict(d_max=INF, max_iter=fm.ITERS, fit_base=False, lock=c["lock"], lock_frames=c["lock_frames"])
    got = env.refine_joints(c["clouds"], c["q0"], metric="feature", **kw)
    point = env.refine_joints(c["clouds"], c["q0"], **kw)
    h = got["cost_history"]
    n_pts = sum(len(x) for x in c["clouds"])
    rms_want = float(np.sqrt(want["cost_history"][-1] / n_pts))
    (ag, dg), (aw, dw), (ap, dp) = (lm.shoulder_errors(c, x["origin"]) for x in (got, want, point))
    print(f"refine: feature {got['iterations']} steps, rms {got['rms_all_before']:.4g} -> {got['rms_all_after']:.4g}, shoulder axis angle / line "
          f"distance {ag:.3g} / {dg:.3g}; restatement {want['iterations']} steps, rms {rms_want:.4g}, {aw:.3g} / {dw:.3g}; point "
          f"{point['iterations']} steps, rms {point['rms_all_after']:.4g}, {ap:.3g} / {dp:.3g}")
    assert all(b <= a for a, b in zip(h, h[1:])) and len(h) == got["iterations"] + 1 and h[-1] < h[0]
    assert got["rms_all_after"] <= max(2.0 * rms_want, FLOOR)
    assert ag <= max(2.0 * aw, FLOOR) and dg <= max(2.0 * dw, FLOOR)
    assert got["rms_all_after"] <= 1e-3 * point["rms_all_after"]
    zero = np.zeros(4)
    start = pref.posed_mesh(r.tri, r.tri_start, pf.fk(c["table"], zero, np.eye(4)))
    diag = float(np.linalg.norm(start.reshape(-1, 3).max(0) - start.reshape(-1, 3).min(0)))
    after = pref.posed_mesh(got["tri"], r.tri_start, pf.fk(dict(c["table"], origin=got["origin"]), zero, np.eye(4)))
    assert np.abs(after - start).max() <= 1e-12 * diag
    w = got["names"].index("wrist")
    np.testing.assert_array_equal(got["frames"][w], np.eye(4))
    assert not got["unobserved_frames"].any() and (got["n"] == 400).all()
    named = env.refine_joints(on_a_grid(c["clouds"]), c["q0"], metric="point", **dict(kw, max_iter=2))
    plain = env.refine_joints(on_a_grid(c["clouds"]), c["q0"], **dict(kw, max_iter=2))
    for k in ("q", "origin", "frames", "tri"):
        np.testing.assert_array_equal(bits(named[k]), bits(plain[k]))
    assert named["iterations"] == plain["iterations"]


@pytest.mark.filterwarnings("ignore:autourdf_amd.prefer_device_kernargs")     # main() in this process: the runtime is up already
def test_command_line_fit_metric(golden, tmp_path, monkeypatch, capsys):
    """--fit_positions --refine_joints on fixture a, its raw clouds put on a grid (``on_a_grid``: two runs then compute the same
    bits), three times: without --fit_metric (no link-moments call asks for the feature metric, no "metric" entry is written),
    with --fit_metric point (every file keeps its bytes but cloud_fit.json, which gains the two "metric" entries and whose rms
    figures, torch index_add_ sums, agree to 1e-9), and with --fit_metric feature (it runs, writes "metric", no cost history
    rises, and what does not depend on the fits keeps its bytes).  A fit_metric key without a fit is a ValueError before anything
    is written."""
    from _ply import write_ascii_ply
    from autourdf_amd import compute_joints, coord_map, ops
    from autourdf_amd.cluster_icp import read_point_cloud
    robot, cams, step = "testbot", 20, 4
    S, T, K = _layout(tmp_path, golden, robot, cams, step)
    for ply in sorted((tmp_path / f"data/raw/{robot}").rglob("robot.ply")):
        write_ascii_ply(str(ply), on_a_grid([np.asarray(read_point_cloud(str(ply)).points)])[0])
    out_dir = tmp_path / f"data/urdf/{robot}_{K}_seg"
    stem = f"{step}_deg_{cams}_cams"
    monkeypatch.chdir(tmp_path)
    base = ["--robot", robot, "--unknown_dof", "--end_video", "2", "--voxel_size", "0.01", "--joint_limits", "--cloud_fit", "--fit_max", "0.05",
            "--fit_positions", "--fit_iters", "4", "--refine_joints", "--refine_iters", "4"]
    real, asked, histories = ops.link_moments, [], []

    def watched(*a, **k):
        asked.append(k.get("metric", "point"))
        return real(*a, **k)

    def recorded(driver):
        def run(*a, **k):
            out = driver(*a, **k)
            histories.append(out["cost_history"])
            return out
        return run

    monkeypatch.setattr(ops, "link_moments", watched)
    monkeypatch.setattr(compute_joints, "fit_cloud_poses", recorded(compute_joints.fit_cloud_poses))
    monkeypatch.setattr(compute_joints, "refine_joint_frames", recorded(compute_joints.refine_joint_frames))
    files = lambda: {name: (out_dir / name).read_bytes() for name in sorted(os.listdir(out_dir))}
    coord_map.main(base)
    plain = files()
    assert asked and set(asked) == {"point"}
    coord_map.main(base + ["--fit_metric", "point"])
    named = files()
    assert sorted(named) == sorted(plain) and set(asked) == {"point"}
    for name in plain:
        if not name.endswith(".cloud_fit.json"):
            assert named[name] == plain[name], name
    report, before = json.loads(named[stem + ".cloud_fit.json"]), json.loads(plain[stem + ".cloud_fit.json"])
    assert report["fitted"].pop("metric") == "point" and report["refined"].pop("metric") == "point"
    assert "metric" not in before["fitted"] and "metric" not in before["refined"]

    def same(a, b):
        if isinstance(a, dict):
            return isinstance(b, dict) and sorted(a) == sorted(b) and all(same(a[k], b[k]) for k in a)
        if isinstance(a, list):
            return isinstance(b, list) and len(a) == len(b) and all(same(x, y) for x, y in zip(a, b))
        if isinstance(a, float) and isinstance(b, float):
            return abs(a - b) <= 1e-9 * max(abs(a), abs(b))
        return a == b
    assert same(report, before)
    del asked[:], histories[:]
    capsys.readouterr()
    coord_map.main(base + ["--fit_metric", "feature"])
    text = capsys.readouterr().out
    feature = files()
    for name in (stem + ".urdf", stem + ".joint_motion.json", stem + ".joint_positions.npy"):
        assert feature[name] == plain[name], name
    report = json.loads(feature[stem + ".cloud_fit.json"])
    assert same({k: v for k, v in report.items() if k not in ("fitted", "refined")}, {k: v for k, v in before.items() if k not in ("fitted", "refined")})
    assert set(asked) == {"feature"} and report["fitted"]["metric"] == "feature" and report["refined"]["metric"] == "feature"
    per_pose, total = histories
    assert len(per_pose) == S * T and all(all(b <= a for a, b in zip(h, h[1:])) for h in per_pose + [total])
    assert all(f["rms_after"] <= f["rms_before"] for f in report["fitted"]["frames"])
    assert report["refined"]["all"]["rms_after"] <= report["refined"]["all"]["rms_before"]
    print("fit_metric feature on fixture a:", report["fitted"]["all"], report["refined"]["all"], report["refined"]["iterations"])
    assert "fit_positions seq0" in text and "refine_joints: rms" in text
    # the key of parameters.json without a fit, and a value that is no metric: before anything is written
    for name in os.listdir(out_dir):
        os.remove(out_dir / name)
    for entry, word in (({"cloud_fit": True, "fit_metric": "feature", "voxel_size": 0.01}, "fit_metric"),
                        ({"cloud_fit": True, "fit_positions": True, "fit_metric": "plane", "voxel_size": 0.01}, "fit_metric")):
        (tmp_path / "parameters.json").write_text(json.dumps({robot: dict({"num_seg": K, "dof": 5}, **entry)}))
        with pytest.raises(ValueError, match=word):
            coord_map.main(["--robot", robot, "--unknown_dof", "--end_video", "2", "--joint_limits"])
        assert os.listdir(out_dir) == []
