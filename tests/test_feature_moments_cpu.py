"""No GPU: the feature-moments restatement (tests/_feature_moments_ref.py) against the direct sum J^T Pi J of the pose-fit
restatement's columns; the restatement drivers at both metrics; the torch unpacking on CPU tensors; and the host side of
creg_feature_moments_f64, of ops.link_moments(metric=...) and of --fit_metric: the header's text, signatures, one-fault EINVAL texts
and workspace sizes through made-up pointers (as test_point_entries_cpu.py does), usage errors."""
import ctypes
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import _feature_moments_ref as fm  # noqa: E402
import _link_moments_ref as lm  # noqa: E402
import _point_mesh_ref as pref  # noqa: E402
import _pose_fit_ref as pf  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EINVAL = -1
PTR = ctypes.c_void_p(0x1000)
NAN = float("nan")
BIG = 2 ** 64 - 1
FM = "creg_feature_moments_f64"
# the entry's arguments by name, valid as they stand: F = 300 triangles in L = 3 links, P = 2 poses, N = 100 points
ARGS = dict(tri=PTR, tri_start=PTR, n_tri=300, link_T=PTR, n_links=3, n_poses=2, pts=PTR, pt_start=PTR, n_pts=100, d_max=0.5, tri_idx=PTR,
            ref=PTR, mom=PTR, cnt=PTR, fmom=PTR, workspace=PTR, workspace_bytes=2816, stream=None)
NULLS = "null pt_start, ref, mom, cnt or fmom"
FAULTS = [
    (dict(d_max=-1.0), "d_max must be >= 0 (+inf allowed), got -1"),
    (dict(d_max=NAN), "d_max must be >= 0 (+inf allowed), got nan"),
    (dict(n_pts=-1), "0 <= n_pts < 2^31 (got -1)"),
    (dict(n_pts=2 ** 31), "0 <= n_pts < 2^31 (got 2147483648)"),
    (dict(tri=None), "null pointer"), (dict(tri_start=None), "null pointer"), (dict(link_T=None), "null pointer"),
    (dict(workspace=None), "null pointer"),
    (dict(workspace_bytes=2815), "workspace of 2815 bytes, 2816 needed"),
    (dict(n_poses=0), "n_poses >= 1 and (n_pts >> 6) + n_poses < 2^31 (got 0)"),
    (dict(n_poses=2 ** 31 - (100 >> 6), workspace_bytes=BIG), "n_poses >= 1 and (n_pts >> 6) + n_poses < 2^31 (got 2147483647)"),
    (dict(n_links=0), "1 <= n_links <= 65535 (got 0)"),
    (dict(n_links=65536, workspace_bytes=BIG), "1 <= n_links <= 65535 (got 65536)"),
    (dict(n_tri=-1), "bad argument (n_tri -1, n_links 3, n_poses 2, n_pairs 0)"),
    (dict(n_tri=2 ** 31), "n_tri < 2^31 and n_links <= 65535 (got 2147483648, 3)"),
    (dict(n_poses=2 ** 25, n_links=65535, workspace_bytes=BIG), "too many (pose, link) pairs (33554432 x 65535)"),
    (dict(pt_start=None), NULLS), (dict(ref=None), NULLS), (dict(mom=None), NULLS), (dict(cnt=None), NULLS), (dict(fmom=None), NULLS),
    (dict(pts=None), "null pts / tri_idx with n_pts 100"), (dict(tri_idx=None), "null pts / tri_idx with n_pts 100"),
]
# align_up(8 ((n_pts >> 6) + n_poses) n_links 38, 256), worked out by hand from the header's formula; 0 for the refused counts
SIZES = [((2, 100, 3), 2816), ((1, 0, 1), 512), ((7, 12345, 65535), 3964605440), ((2 ** 31 - 2, 100, 1), 652835028736), ((8, 1141, 5), 38144),
         ((0, 100, 3), 0), ((2, -1, 3), 0), ((2, 2 ** 31, 3), 0), ((2, 100, 0), 0), ((2, 100, 65536), 0), ((2 ** 31 - 1, 100, 3), 0)]


@pytest.fixture(scope="module")
def lib():
    from autourdf_amd import _lib
    return _lib.load(check_device=False)


@pytest.fixture(scope="module")
def robot(tmp_path_factory):
    return pf.toy_robot(tmp_path_factory.mktemp("toy"))


# ------------------------------------------------------------------------------------------ the host side
def test_header_block_signatures_sources_and_version(lib):
    from autourdf_amd import _lib, build
    assert "feature_moments.hip" in build.SOURCES and os.path.exists(os.path.join(build.CSRC, "feature_moments.hip"))
    res, args = _lib.SIGNATURES["creg_feature_moments_workspace_bytes"]
    assert res is ctypes.c_size_t and args == [_lib.i64, _lib.i64, _lib.i32]
    res, args = _lib.SIGNATURES[FM]
    link = _lib.SIGNATURES["creg_link_moments_f64"][1]
    assert res is ctypes.c_int and len(args) == 18 == len(ARGS)
    assert args[:14] == link[:14] and args[14] is _lib.vp and args[15:] == link[14:]             # the sibling's, with fmom after cnt
    header = open(os.path.join(ROOT, "include", "creg.h")).read()
    decl = header[header.index("int creg_feature_moments_f64("):]
    assert decl[:decl.index(";")].count(",") + 1 == 18
    text = header[header.index("Feature moments:"):header.index("size_t creg_feature_moments_workspace_bytes")]
    for word in ("exactly those of creg_link_moments_f64", "pt_tri_vec", "delta_ij - (e_i*e_j)/ee", "(N_i*N_j)/NN", "when ee > 0", "when NN > 0",
                 "no square root", "A_0 = (0, -d_z, d_y), A_1 = (d_z, 0, -d_x), A_2 = (-d_y, d_x, 0)", "B_k[i] = dot(Pi_i, A_k)", "dot(A_a, B_b)",
                 "(n_poses,n_links,21)", "bits of", "tiles of 64", "t mod 4", "(s0 + s1) + (s2 + s3)", "(n_pts >> 6) + n_poses",
                 "no floating-point atomics", "38 doubles per tile slot and link", "CREG_EINVAL"):
        assert word in text, word
    assert header.index("Link moments:") < header.index("Feature moments:") < header.index("Containment:")
    assert lib.creg_version() >= 2100 and hasattr(lib, FM)


@pytest.mark.parametrize("fault,text", FAULTS, ids=[f"{'-'.join(f)}-{i}" for i, (f, _) in enumerate(FAULTS)])
def test_one_fault_gives_einval_and_the_text(lib, fault, text):
    """Made-up addresses that are never dereferenced: there is no device here, a HIP call would answer CREG_EHIP."""
    assert set(fault) <= set(ARGS), fault
    rc = getattr(lib, FM)(*dict(ARGS, **fault).values())
    assert (rc, lib.creg_last_error().decode()) == (EINVAL, f"{FM}: {text}")


def test_the_workspace_sizes(lib):
    for counts, size in SIZES:
        assert lib.creg_feature_moments_workspace_bytes(*counts) == size, counts
    assert ARGS["workspace_bytes"] == lib.creg_feature_moments_workspace_bytes(2, 100, 3)
    for P, N, L in ((1, 0, 1), (3, 600, 5), (10, 50000, 12)):
        assert lib.creg_feature_moments_workspace_bytes(P, N, L) > lib.creg_link_moments_workspace_bytes(P, N, L)


def test_link_moments_validates_metric_before_anything_else():
    from autourdf_amd import ops
    for bad in ("plane", "", None, "Feature", 1):
        with pytest.raises(ValueError, match="metric"):
            ops.link_moments(None, None, None, None, None, None, None, metric=bad)
    from autourdf_amd.compute_joints import FIT_METRICS, fit_cloud_poses, refine_joint_frames
    assert FIT_METRICS == ("point", "feature")
    for driver in (fit_cloud_poses, refine_joint_frames):
        with pytest.raises(ValueError, match="metric"):
            driver(None, [], None, metric="plane")


def test_fit_metric_usage_errors_leave_an_empty_directory(tmp_path, monkeypatch, capsys):
    """--fit_metric without --fit_positions or --refine_joints ends the command before anything is read or written (there is no
    parameters.json here to read); so does a value that is no metric."""
    from autourdf_amd import coord_map
    monkeypatch.chdir(tmp_path)
    base = ["--robot", "testbot", "--voxel_size", "0.01", "--joint_limits", "--cloud_fit"]
    for argv, word in ((base + ["--fit_metric", "feature"], "--fit_metric needs --fit_positions or --refine_joints"),
                       (["--robot", "testbot", "--fit_metric", "point"], "--fit_metric needs --fit_positions or --refine_joints"),
                       (base + ["--fit_positions", "--fit_metric", "plane"], "invalid choice")):
        with pytest.raises(SystemExit) as e:
            coord_map.main(argv)
        assert e.value.code == 2 and word in capsys.readouterr().err
        assert os.listdir(tmp_path) == []
    parse = coord_map._cli_parser().parse_args
    assert parse(base + ["--fit_positions", "--fit_metric", "feature"]).fit_metric == "feature"
    assert parse(base + ["--refine_joints", "--fit_metric", "point"]).fit_metric == "point"
    assert parse(base + ["--fit_positions"]).fit_metric is None


# ------------------------------------------------------------------------------------------ the restatement
def test_projector_of_each_case_by_hand():
    """The triangle (0,0,0) (4,0,0) (0,3,0): vertices I; edge ab along x, ac along y, bc along (-4,3,0)/5; the face's normal z.
    Small integers: every entry is exact.  Zero-area rows take the guards."""
    W = np.tile(np.array([[(0, 0, 0), (4, 0, 0), (0, 3, 0)]], np.float64), (7, 1, 1))
    Pi = fm.projectors(np.arange(1, 8), W)
    for k in range(3):
        np.testing.assert_array_equal(Pi[k], np.eye(3))
    np.testing.assert_array_equal(Pi[3], np.diag([0.0, 1.0, 1.0]))
    np.testing.assert_array_equal(Pi[4], np.diag([1.0, 0.0, 1.0]))
    np.testing.assert_array_equal(Pi[5], [[1 - 16 / 25, 12 / 25, 0], [12 / 25, 1 - 9 / 25, 0], [0, 0, 1]])
    np.testing.assert_array_equal(Pi[6], np.diag([0.0, 0.0, 1.0]))
    flat = np.tile(np.array([[(1, 1, 1), (1, 1, 1), (3, 1, 1)]], np.float64), (4, 1, 1))          # a = b: N = 0, ab has no length
    Pi = fm.projectors(np.array([4, 5, 6, 7]), flat)
    np.testing.assert_array_equal(Pi[0], np.eye(3))                                              # ee = 0
    np.testing.assert_array_equal(Pi[1], np.diag([0.0, 1.0, 1.0]))
    np.testing.assert_array_equal(Pi[2], np.diag([0.0, 1.0, 1.0]))
    np.testing.assert_array_equal(Pi[3], np.eye(3))                                              # NN = 0
    # the terms of one row by hand: d = (1, 2, 3), the face's Pi = diag(0, 0, 1): only the z components survive
    t = fm.row_terms(np.array([[1.0, 2.0, 3.0]]), np.zeros((1, 3)), np.diag([0.0, 0.0, 1.0])[None])[0]
    M = fm.unpack(t)
    A = np.array([[0, -3, 2], [3, 0, -1], [-2, 1, 0], [1, 0, 0], [0, 1, 0], [0, 0, 1]], np.float64)
    np.testing.assert_array_equal(M, np.outer(A[:, 2], A[:, 2]))


def test_restated_system_against_the_direct_sum_of_the_columns(robot):
    """On the pose-fit scene: H assembled from the 21 sums about center_p under the pose-only twists equals sum J^T Pi J with
    _pose_fit_ref.point_terms' J, to rounding.  Both sides round products whose magnitudes are bounded entry by entry by
    sum_rows |J|_a . (|Pi| |J|_b) with |J| = |A| |Tw| (not |A Tw|: a joint's column is Omega x d + V here, two terms that cancel near
    the joint's axis): 64 roundings of 2^-53 on that cover the few of a term, the 6 x 6 products
    per link and the long-double sums' final rounding.  |Pi r - r| stays at rounding of the coordinates (r is orthogonal to the
    feature only as far as its own subtraction p - q is exact): 64 x 2^-53 x the largest coordinate.  Every M6 is symmetric by
    construction and positive semidefinite to 64 x 2^-53 of its trace."""
    sc = pf.system_scene(robot)
    _, idx, _ = pref.point_mesh(sc["tri"], sc["tri_start"], sc["link_T"], sc["pts"], sc["pt_start"], sc["d_max"])
    idx = idx.copy()
    idx[sc["drop"]] = -1
    table = {k: v for k, v in sc["table"].items() if not k.startswith("_dev")}
    got = fm.system(sc["tri"], sc["tri_start"], sc["link_T"], sc["pts"], sc["pt_start"], idx, table, sc["center"], sc["d_max"])
    want = pf.system(sc["tri"], sc["tri_start"], sc["link_T"], sc["pts"], sc["pt_start"], idx, table, sc["center"], sc["d_max"])
    m = got["moments"]
    np.testing.assert_array_equal(m["ok"], want["ok"])
    counts = np.bincount(m["case"][m["ok"]], minlength=8)[1:]
    assert (counts >= 2).all(), dict(zip(pf.CASES, counts))
    ok, Pi, J, r = m["ok"], m["Pi"], want["J"], want["r"]
    pose_of = np.repeat(np.arange(len(sc["link_T"])), np.diff(sc["pt_start"]))
    chain = pf.chains(table)
    worst = 0.0
    for p in range(len(sc["link_T"])):
        rows = ok & (pose_of == p)
        direct = np.einsum("nai,nij,nbj->ab", J[rows].astype(fm.LD), Pi[rows].astype(fm.LD), J[rows].astype(fm.LD)).astype(np.float64)
        Tw = lm.twists(table, chain, sc["link_T"][p], np.zeros(4), sc["center"][p], np.tile(sc["center"][p], (5, 1)))[:, :, :10]
        mag = np.einsum("nki,nka->nai", np.abs(fm.columns(m["c"][rows] - sc["center"][p])), np.abs(Tw[m["link"][rows]]))      # |A| |Tw|
        size = np.einsum("nai,nij,nbj->ab", mag, np.abs(Pi[rows]), mag)
        err, bound = np.abs(got["H"][p] - direct), 64 * fm.EPS * size
        assert (err <= bound).all(), (p, float((err - bound).max()))
        with np.errstate(invalid="ignore", divide="ignore"):
            worst = max(worst, float(np.nanmax(np.where(bound > 0, err / bound, 0.0))))
        np.testing.assert_array_equal(got["g"][p], lm.assemble(m["mom"][p], m["cnt"][p], Tw)[1])      # g is the link moments'
        # the curvature never exceeds the point-to-point one: J^T (I - Pi) J is positive semidefinite too
        assert np.linalg.eigvalsh(want["H"][p] - got["H"][p]).min() >= -64 * fm.EPS * np.trace(want["H"][p])
    print(f"largest |assembled - direct sum J^T Pi J| / bound: {worst:.3g}")
    scale = max(np.nanmax(np.abs(sc["pts"])), np.abs(sc["tri"]).max() + np.abs(sc["link_T"][:, :, :3, 3]).max())
    off = np.abs(np.einsum("nij,nj->ni", Pi[ok], r[ok]) - r[ok]).max()
    print(f"largest |Pi r - r| {off:.3g} at a coordinate scale of {scale:.3g}")
    assert off <= 64 * fm.EPS * scale
    for p, l in np.ndindex(m["cnt"].shape):
        M6 = fm.unpack(m["fmom"][p, l])
        np.testing.assert_array_equal(M6, M6.T)
        assert np.linalg.eigvalsh(M6).min() >= -64 * fm.EPS * max(np.trace(M6), 0.0), (p, l)
        assert (M6 == 0).all() == (m["cnt"][p, l] == 0)
    # the package's unpacking (plain torch, here on CPU tensors) is the restatement's
    import torch

    from autourdf_amd.compute_joints import link_twists, twist_system
    P, L = m["cnt"].shape
    ref = np.ascontiguousarray(np.broadcast_to(sc["center"][:, None, :], (P, L, 3)))
    Tw = link_twists(table, torch.as_tensor(sc["link_T"]), torch.zeros(P, 4, dtype=torch.float64), torch.as_tensor(sc["center"]),
                     torch.as_tensor(ref), structure=False)
    mom, cnt, fmom = torch.as_tensor(m["mom"]), torch.as_tensor(m["cnt"]), torch.as_tensor(m["fmom"])
    H, g, cost = (x.numpy() for x in twist_system(mom, cnt, Tw, fmom))
    H0, g0, cost0 = (x.numpy() for x in twist_system(mom, cnt, Tw))
    np.testing.assert_array_equal(g, g0)
    np.testing.assert_array_equal(cost, cost0)
    for p in range(P):
        np.testing.assert_allclose(H[p], got["H"][p], rtol=0, atol=1e-13 * np.abs(got["H"][p]).max() + 1e-300)
    assert np.abs(H - H0).max() > 1e-3 * np.abs(H0).max()                        # and it is not the point-to-point matrix


def test_degenerate_triangles_take_the_guards():
    d = fm.degenerate_case()
    m = fm.moments(d["tri"], d["tri_start"], d["link_T"], d["pts"], d["pt_start"], d["tri_idx"], d["ref"], d["d_max"])
    assert m["ok"].all() and list(m["cnt"][0]) == [3, 10]
    eye = (m["Pi"] == np.eye(3)).all((1, 2))
    rows = d["tri_idx"]
    assert list(m["case"][rows == 2]) == [1, 1, 1] and eye[rows == 2].all()     # coincident: vertex a
    assert set(m["case"][rows == 1]) <= {1, 2, 3, 4, 5, 6} and (m["case"][rows == 1] >= 4).sum() >= 2
    assert not eye[(rows == 1) & (m["case"] >= 4)].any()                          # collinear: an edge of positive length
    guard = (rows == 3) & (m["case"] == 4)
    assert guard.sum() >= 1 and eye[guard].all()                                  # a = b: edge ab has no length, ee > 0 fails
    assert np.isfinite(m["fmom"]).all()


# ------------------------------------------------------------------------------------------ the drivers
def test_restatement_drivers_at_both_metrics(robot):
    """pf.driver_case and lm.refine_case, 12 steps allowed, the restatement drivers with the point-to-point and with the feature
    curvature: the feature run's final cost is at most 1e-3 of the point run's (measured: 1e-25 of it -- the margin only guards
    against a wrong projector), the shoulder errors of the refinement end below 1e-9, no history ever rises."""
    runs = fm.driver_runs(robot)
    c, point, feat = runs["fit"]
    for p in range(len(c["clouds"])):
        hp, hf = point["cost_history"][p], feat["cost_history"][p]
        print(f"pose {p}: cost {hp[0]:.4g} -> point {hp[-1]:.4g} in {point['iterations'][p]} steps, feature {hf[-1]:.4g} in {feat['iterations'][p]}; "
              f"max |q - q*| point {np.abs(point['q'][p] - c['q_true'][p])[c['free']].max():.3g}, "
              f"feature {np.abs(feat['q'][p] - c['q_true'][p])[c['free']].max():.3g}")
        assert hp[0] == hf[0] and hf[-1] <= 1e-3 * hp[-1]
        assert all(b <= a for a, b in zip(hp, hp[1:])) and all(b <= a for a, b in zip(hf, hf[1:]))
        assert feat["iterations"][p] <= fm.ITERS and len(hf) == feat["iterations"][p] + 1
    r, point, feat = runs["refine"]
    hp, hf = point["cost_history"], feat["cost_history"]
    ap, dp = lm.shoulder_errors(r, point["origin"])
    af, df = lm.shoulder_errors(r, feat["origin"])
    print(f"refine: cost {hp[0]:.4g} -> point {hp[-1]:.4g} in {point['iterations']} steps, feature {hf[-1]:.4g} in {feat['iterations']}; shoulder axis "
          f"angle / line distance point {ap:.3g} / {dp:.3g}, feature {af:.3g} / {df:.3g}")
    assert hp[0] == hf[0] and hf[-1] <= 1e-3 * hp[-1]
    assert af < 1e-9 and df < 1e-9
    assert all(b <= a for a, b in zip(hp, hp[1:])) and all(b <= a for a, b in zip(hf, hf[1:]))
