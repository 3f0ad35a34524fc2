"""Link clearance, host side (no GPU): the new C-ABI symbols, the numpy restatement of the contract (tests/_clearance_ref.py) on
analytic two-triangle cases and sandwiched between an OBB separating-axis bound and a surface sample, the margin semantics of
the restatement, the plumbing of ``margin=0.0`` (the old path, never ``ops.mesh_clearance``) and the CLI option."""
import os
import re

import numpy as np
import pytest

import _clearance_ref as cref
import _collide_ref as ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_new_symbols_are_declared_bound_and_built():
    from autourdf_amd import _lib, build, ops
    header = open(os.path.join(ROOT, "include", "creg.h")).read()
    declared = set(re.findall(r"\b(creg_[a-z0-9_]+)\s*\(", header))
    for name in ("creg_mesh_clearance_workspace_bytes", "creg_mesh_clearance_f64"):
        assert name in declared and name in _lib.SIGNATURES, name
    assert "clearance.hip" in build.SOURCES and "collide.hip" in build.SOURCES
    assert callable(getattr(ops, "mesh_clearance"))
    for word in ("gap2", "pt_tri2", "seg_seg2", "contributes"):   # the contract is stated, not only declared
        assert word in header, word


# ------------------------------------------------------------------------------------------ analytic cases
@pytest.mark.parametrize("name", sorted(cref.ANALYTIC))
def test_restatement_on_analytic_triangle_pairs(name):
    a, b, want = cref.ANALYTIC[name]
    tol = 4 * np.finfo(np.float64).eps * 8.0                      # a few roundings at the cases' coordinate scale (< 8)
    for x, y in ((a, b), (b, a)):
        d2 = cref.tri_pair_d2(x, y)
        assert np.isfinite(d2) and d2 >= 0.0, name               # a degenerate triangle gives no NaN
        assert abs(np.sqrt(d2) - want) <= tol, (name, np.sqrt(d2), want)
    tri, start, link_T = cref.two_links(a, b)
    dist2, wit, box = cref.mesh_clearance(tri, start, link_T, [[0, 1], [1, 0]], np.inf)
    assert abs(np.sqrt(dist2[0, 0]) - want) <= tol and dist2[0, 0] == dist2[0, 1]
    assert wit.tolist() == [[[0, 1], [1, 0]]]
    if want == 0.0:
        assert dist2[0, 0] == 0.0                                 # exactly: a pierced pair by the predicate, crossing edges by seg_seg2


def test_prototype_cases_are_among_the_analytic_ones():
    assert cref.ANALYTIC["parallel_offset"][2] == 0.37 and cref.ANALYTIC["coplanar_disjoint"][2] == 2.0
    assert cref.ANALYTIC["coplanar_overlapping"][2] == 0.0
    a, b, _ = cref.ANALYTIC["coplanar_overlapping"]              # not a collision by the predicate: zero through a crossing edge pair
    A, B = np.array([a], np.float64), np.array([b], np.float64)
    assert len(ref.colliding_pairs(A, B)[0]) == 0
    assert min(float(cref.seg_seg2(A[:, i], A[:, (i + 1) % 3], B[:, j], B[:, (j + 1) % 3])[0]) for i in range(3) for j in range(3)) == 0.0


def test_routines_have_no_nan_on_degenerate_input():
    p = np.array([[1.0, 2.0, 3.0]])
    z = np.zeros((1, 3))
    e = np.array([[1.0, 0.0, 0.0]])
    assert cref.pt_tri2(p, z, z, z)[0] == 14.0                    # a point
    assert cref.pt_tri2(p, z, z, e)[0] == 13.0                    # a == b: closest is the far end of (a, c)
    assert cref.pt_tri2(p, z, e, 2 * e)[0] == 13.0                # collinear
    assert cref.seg_seg2(p, p, z, z)[0] == 14.0
    assert cref.seg_seg2(p, p, z, 2 * e)[0] == 13.0 and cref.seg_seg2(z, 2 * e, p, p)[0] == 13.0
    assert cref.seg_seg2(z, e, z + [0, 1, 0], e + [0, 1, 0])[0] == 1.0   # parallel: the denominator is 0


# ------------------------------------------------------------------------------------------ sandwich on oriented boxes
def _surface_sample(h, R, t, n=9):
    g = np.linspace(-1.0, 1.0, n)
    u, v = (a.reshape(-1) for a in np.meshgrid(g, g, indexing="ij"))
    pts = []
    for axis in range(3):
        for sign in (-1.0, 1.0):
            c = np.empty((len(u), 3))
            c[:, axis], c[:, (axis + 1) % 3], c[:, (axis + 2) % 3] = sign, u, v
            pts.append(c)
    return np.concatenate(pts) * h @ R.T + t


def test_restatement_is_sandwiched_between_obb_separation_and_a_surface_sample():
    rng = np.random.default_rng(0)
    mesh = ref.box_mesh(1.0, 1.0, 1.0)
    separated, low, high = 0, -np.inf, -np.inf
    for _ in range(60):
        ha, hb = rng.uniform(0.05, 0.3, 3), rng.uniform(0.05, 0.3, 3)
        Ra, Rb = ref.random_rotation(rng), ref.random_rotation(rng)
        u = rng.normal(size=3)
        u = u / np.linalg.norm(u)
        tb = u * rng.uniform(0.3, 0.9)
        sep = ref.obb_separation(ha, Ra, np.zeros(3), hb, Rb, tb)
        if not sep > 0:
            continue
        separated += 1
        A, B = ref.pose(mesh * ha, ref.rigid(Ra)), ref.pose(mesh * hb, ref.rigid(Rb, tb))
        d = np.sqrt(cref.link_clearance(A, B, np.inf)[0])
        sa, sb = _surface_sample(ha, Ra, np.zeros(3)), _surface_sample(hb, Rb, tb)
        sampled = np.sqrt(((sa[:, None] - sb[None]) ** 2).sum(-1).min())
        low, high = max(low, sep - d), max(high, d - sampled)
        assert sep - 1e-12 <= d, (sep, d)
        assert d <= sampled, (d, sampled)
    assert separated >= 40                                       # 44 at seed 0
    print(f"separated {separated}, max(sep - d) {low:.3g}, max(d - sampled) {high:.3g}")


# ------------------------------------------------------------------------------------------ margin semantics
def small_scene():
    """Five small links (a triangle, two sphere caps, a box, an empty link) at poses where some pairs cross, some are near and
    some are far."""
    rng = np.random.default_rng(3)
    meshes = [np.array([[[-0.15, -0.1, 0.0], [0.15, -0.1, 0.0], [0.0, 0.2, 0.0]]]), ref.uv_sphere(0.1, n=63), ref.uv_sphere(0.1, n=65),
              ref.box_mesh(0.06, 0.08, 0.1), np.zeros((0, 3, 3))]
    tri, start = ref.pack(meshes)
    link_T = np.array([[ref.rigid(ref.random_rotation(rng), rng.uniform(-s, s, 3)) for _ in meshes] for s in (0.06, 0.12, 0.25)])
    return tri, start, link_T, ref.all_pairs(len(meshes))


def test_margin_semantics_of_the_restatement():
    tri, start, link_T, pairs = small_scene()
    full, wit_full, box = cref.mesh_clearance(tri, start, link_T, pairs, np.inf)
    empty = (pairs == 4).any(1)
    assert np.isinf(full[:, empty]).all() and (wit_full[:, empty] == -1).all() and np.isfinite(full[:, ~empty]).all()
    assert (full == 0).any() and (full > 0.05 ** 2).any()        # crossing and far pairs both occur
    np.testing.assert_array_equal(box, ref.mesh_collide(tri, start, link_T, pairs)[2])
    count = ref.mesh_collide(tri, start, link_T, pairs)[0]
    assert ((full == 0) >= (count > 0)).all()                    # a colliding pair has clearance 0
    for d_max in (0.0, 0.02, 0.05, 0.3):
        got, wit, _ = cref.mesh_clearance(tri, start, link_T, pairs, d_max)
        inside = full <= d_max * d_max
        np.testing.assert_array_equal(got[inside], full[inside])
        np.testing.assert_array_equal(wit[inside], wit_full[inside])
        assert (np.isinf(got[~inside]) | (got[~inside] > d_max * d_max)).all()
        assert ((wit[~inside] == -1).all(-1) == np.isinf(got[~inside])).all()
    assert (cref.mesh_clearance(tri, start, link_T, pairs, 0.0)[0] == 0).sum() == (full == 0).sum() > 0


# ------------------------------------------------------------------------------------------ plumbing
@pytest.fixture()
def env(tmp_path):
    return ref.toy(tmp_path)


def test_margin_zero_takes_the_old_path(env, monkeypatch):
    """Without a GPU the calls cannot run, so the device entry points are replaced: at margin 0.0 ``SimEnv.collisions`` and
    ``data_collection(check_collision=True)`` reach ``ops.mesh_collide`` with today's arguments and never ``ops.mesh_clearance``;
    with a margin it is the other way round.  (The behavioural half is in tests/test_gpu_clearance.py.)"""
    import torch
    from autourdf_amd import ops, sim_data
    r = env.robot
    calls = []

    def fake_collide(tri, tri_start, link_T, pairs, want_boxes=False):
        link_T = link_T[None] if link_T.dim() == 3 else link_T
        calls.append(("collide", tuple(link_T.shape), want_boxes))
        P, M, L = link_T.shape[0], pairs.shape[0], link_T.shape[1]
        count = torch.zeros(P, M, dtype=torch.int32)
        count[-1, 1] = 3                                          # the last row collides
        return count, torch.zeros(P, M, 2, dtype=torch.int32), torch.ones(P, L, 6, dtype=torch.float64)

    def fake_clearance(tri, tri_start, link_T, pairs, d_max, want_boxes=False):
        link_T = link_T[None] if link_T.dim() == 3 else link_T
        calls.append(("clearance", tuple(link_T.shape), d_max, want_boxes))
        P, M, L = link_T.shape[0], pairs.shape[0], link_T.shape[1]
        dist = torch.full((P, M), float("inf"), dtype=torch.float64)
        dist[-1, 2] = 0.004
        return dist, torch.full((P, M, 2), 7, dtype=torch.int32), torch.ones(P, L, 6, dtype=torch.float64)

    monkeypatch.setattr(sim_data.SimEnv, "_device_mesh", lambda self: (torch.as_tensor(r.tri), None, None))
    monkeypatch.setattr(ops, "mesh_collide", fake_collide)
    monkeypatch.setattr(ops, "mesh_clearance", lambda *a, **k: pytest.fail("mesh_clearance called at margin 0.0"))
    link_T = torch.as_tensor(np.stack([r.fk({}, env.base)] * 2))
    names = [(r.links[a], r.links[b]) for a, b in r.collision_pairs()]
    for kw in ({}, {"margin": 0.0}, {"margin": 0}):
        got = env.collisions(link_T, **kw)
        assert got == [([], []), ([(names[1][0], names[1][1], 3, 0, 0)], [])]
    assert env.self_collision_check({}, link_T=link_T[0]) == ([(names[1][0], names[1][1], 3, 0, 0)], [])
    for kw in ({}, {"collision_margin": 0.0}):                    # one row, which the fake calls colliding: no frame is made
        collision, record = sim_data.data_collection(env, angle_list=np.zeros((1, 3)), link_T=link_T[:1], check_collision=True, **kw)
        assert collision is True and record == []
    assert len(calls) == 6 and all(c[0] == "collide" and c[2] is True for c in calls)
    # with a margin: the clearance entry, d_max = the margin, and never mesh_collide
    calls.clear()
    monkeypatch.setattr(ops, "mesh_collide", lambda *a, **k: pytest.fail("mesh_collide called with a margin"))
    monkeypatch.setattr(ops, "mesh_clearance", fake_clearance)
    link_T = torch.as_tensor(np.stack([r.fk({}, env.base)] * 2))
    assert env.collisions(link_T, margin=0.01) == [([], []), ([(names[2][0], names[2][1], 0.004, 7, 7)], [])]
    assert env.collisions(link_T, margin=0.003) == [([], []), ([], [])]
    assert env.clearance(link_T, 0.01) == env.collisions(link_T, margin=0.01)
    assert len(env.clearance(link_T, np.inf)[0][0]) == len(names)         # margin = inf lists every tested pair
    collision, record = sim_data.data_collection(env, angle_list=np.zeros((1, 3)), link_T=link_T[1:], check_collision=True, collision_margin=0.01)
    assert collision is True and record == []
    assert [c[:3] for c in calls] == [("clearance", (2, 5, 4, 4), 0.01), ("clearance", (2, 5, 4, 4), 0.003), ("clearance", (2, 5, 4, 4), 0.01),
                                      ("clearance", (2, 5, 4, 4), 0.01), ("clearance", (2, 5, 4, 4), np.inf), ("clearance", (1, 5, 4, 4), 0.01)]
    for bad in (-0.01, float("nan")):
        with pytest.raises(ValueError, match="margin"):
            env.collisions(link_T, margin=bad)
        with pytest.raises(ValueError, match="margin"):
            env.clearance(link_T, bad)


def test_collect_carries_the_margin_down(tmp_path, monkeypatch, capsys):
    from _toy_urdf import write_toy_robot
    from autourdf_amd import sim_data
    for d in (tmp_path, tmp_path / "b"):
        write_toy_robot(str(d))
    params = {"gt": "toy.urdf", "dof": 3}
    seen = []

    def fake_collides(env, a_list, use_excluded=False, **kw):
        seen.append(kw)
        if kw and len(seen) == 1:
            kw["closest"].append((0.0042, 3, "base", "l3"))
            return [("base", "l3")]
        return []

    monkeypatch.setattr(sim_data, "sequence_collides", fake_collides)
    monkeypatch.setattr(sim_data, "data_collection", lambda env, data_path=None, **kw: (False, []))
    paths = sim_data.collect("toy", params, num_step=4, epochs=1, num_cameras=3, root=str(tmp_path), reject_collisions=True, collision_margin=0.01)
    assert [os.path.basename(p.rstrip("/")) for p in paths] == ["V0001"]
    assert [k.get("margin") for k in seen] == [0.01, 0.01]
    out = capsys.readouterr().out
    assert "seed 0" in out and "base - l3" in out and "0.0042" in out and "margin 0.01" in out
    seen.clear()                                                  # no margin: the call of before, without the keywords
    sim_data.collect("toy", params, num_step=4, epochs=1, num_cameras=3, root=str(tmp_path / "b"), reject_collisions=True)
    assert seen == [{}]
    with pytest.raises(ValueError, match="reject_collisions"):
        sim_data.collect("toy", params, num_step=4, epochs=1, num_cameras=3, root=str(tmp_path / "c"), collision_margin=0.01)


def test_cli_collision_margin_needs_reject_collisions(capsys):
    from autourdf_amd import sim_data
    args = sim_data.parse_args(["--robot", "toy", "--reject_collisions", "--collision_margin", "0.005"])
    assert args.collision_margin == 0.005 and args.reject_collisions is True
    assert sim_data.parse_args(["--reject_collisions"]).collision_margin is None
    assert sim_data.parse_args([]).collision_margin is None
    with pytest.raises(SystemExit):
        sim_data.parse_args(["--robot", "toy", "--collision_margin", "0.005"])
    assert "--reject_collisions" in capsys.readouterr().err
    with pytest.raises(SystemExit):
        sim_data.parse_args(["--reject_collisions", "--collision_margin", "-1"])


def test_cli_reads_the_margin_of_the_robots_entry_and_the_option_wins(tmp_path, monkeypatch):
    import json
    from autourdf_amd import sim_data
    (tmp_path / "parameters.json").write_text(json.dumps({"toy": {"gt": "toy.urdf", "dof": 3, "collision_margin": 0.02}}))
    monkeypatch.chdir(tmp_path)
    got = []
    monkeypatch.setattr(sim_data, "collect", lambda *a, **k: got.append(k) or [])
    sim_data.main(["--robot", "toy", "--reject_collisions"])
    sim_data.main(["--robot", "toy", "--reject_collisions", "--collision_margin", "0.005"])
    sim_data.main(["--robot", "toy", "--reject_collisions", "--collision_margin", "0"])
    sim_data.main(["--robot", "toy"])
    assert [k.get("collision_margin") for k in got] == [0.02, 0.005, None, None]
