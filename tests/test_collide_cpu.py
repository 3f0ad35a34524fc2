"""Self-collision rejection, host side (no GPU): the new C-ABI symbols, the numpy restatement of the contract on the lattice
cases and against an independent OBB separating-axis test, the link pairs of the toy robot, the poses the GPU tests use, the
CLI flag and collect()'s seed loop."""
import os
import re

import numpy as np
import pytest

import _collide_ref as ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_new_symbols_are_declared_bound_and_built():
    from autourdf_amd import _lib, build, ops
    header = open(os.path.join(ROOT, "include", "creg.h")).read()
    declared = set(re.findall(r"\b(creg_[a-z0-9_]+)\s*\(", header))
    for name in ("creg_mesh_collide_workspace_bytes", "creg_mesh_collide_f64"):
        assert name in declared and name in _lib.SIGNATURES, name
    assert "collide.hip" in build.SOURCES
    assert callable(getattr(ops, "mesh_collide"))


@pytest.mark.parametrize("name", sorted(ref.LATTICE))
def test_restatement_on_the_lattice_triangles(name):
    other, want = ref.LATTICE[name]
    A, B = np.array([ref.BASE], np.float64), np.array([other], np.float64)
    assert len(ref.colliding_pairs(A, B)[0]) == want
    assert len(ref.colliding_pairs(B, A)[0]) == want             # the pair test is symmetric
    tri, start = ref.pack([A, B])
    count, first, box = ref.mesh_collide(tri, start, np.tile(np.eye(4), (2, 1, 1)), [[0, 1], [1, 0]])
    assert count.tolist() == [[want, want]]
    assert first.tolist() == ([[[0, 1], [1, 0]]] if want else [[[-1, -1], [-1, -1]]])
    np.testing.assert_array_equal(box[0, 0], [0, 0, 0, 4, 4, 0])


def test_restatement_agrees_with_obb_separating_axes():
    mesh = ref.box_mesh(1.0, 1.0, 1.0)
    skipped = hits = free = 0
    for ha, Ra, ta, hb, Rb, tb in ref.random_box_pairs(400, seed=0):
        sep = ref.obb_separation(ha, Ra, ta, hb, Rb, tb)
        if abs(sep) <= 1e-6:
            skipped += 1
            continue
        contained = ref.obb_contains(ha, Ra, ta, hb, Rb, tb) or ref.obb_contains(hb, Rb, tb, ha, Ra, ta)
        want = sep < 0 and not contained
        A = ref.pose(mesh * ha, ref.rigid(Ra, ta))
        B = ref.pose(mesh * hb, ref.rigid(Rb, tb))
        got = len(ref.colliding_pairs(A, B)[0]) > 0
        assert got == want, (sep, contained)
        hits += want
        free += not want
    assert skipped == 0                                          # at most 5 % may be; at seed 0 none is
    assert hits >= 50 and free >= 50


@pytest.fixture(scope="module")
def env(tmp_path_factory):
    return ref.toy(tmp_path_factory.mktemp("toy"))


def test_collision_pairs_of_the_toy(env):
    r = env.robot
    assert r.tri_start.dtype == np.int64 and r.tri_start[0] == 0 and r.tri_start[-1] == len(r.tri)
    for l in range(len(r.links)):
        assert (r.tri_link[r.tri_start[l]:r.tri_start[l + 1]] == l).all()
    ix = r.link_index
    name = lambda pairs: {(r.links[a], r.links[b]) for a, b in pairs}
    pairs = r.collision_pairs()
    assert pairs.dtype == np.int32 and pairs.shape == (6, 2) and (pairs[:, 0] < pairs[:, 1]).all()
    assert name(pairs) == {("base", "l2"), ("base", "l3"), ("base", "tip"), ("l1", "l3"), ("l1", "tip"), ("l2", "tip")}
    assert ix["base"] == 0
    for excl in ([("base", "l3")], [("l3", "base")]):            # either order
        got = r.collision_pairs(excl)
        assert got.shape == (5, 2) and ("base", "l3") not in name(got)
    np.testing.assert_array_equal(r.collision_pairs([("base", "nosuch"), ("ghost", "l3")]), pairs)
    assert r.collision_pairs([("base", "l2"), ("base", "l3"), ("base", "tip"), ("l1", "l3"), ("l1", "tip"), ("tip", "l2")]).shape == (0, 2)


@pytest.mark.parametrize("q,want", [({}, []), ({"shoulder": 1.2}, []), ({"shoulder": -1.5}, []), ({"shoulder": 2.9}, [("base", "l3")]),
                                    ({"shoulder": -2.7, "wrist": 1.0}, [("base", "l3")])])
def test_toy_poses_cover_both_outcomes(env, q, want):
    got = ref.toy_contacts(env, q)
    assert [(a, b) for a, b, *_ in got] == want
    for _, _, count, ta, tb in got:
        assert count > 0 and env.robot.tri_link[ta] == 0 and env.robot.tri_link[tb] == 3


def test_toy_adjacent_links_intersect_or_sit_flush(env):
    """Why joined links are never tested: l1-l2 and l3-tip of the toy intersect at every pose (base-l1 sit flush and never do: touching
    is not a collision; l2-l3 touch too, which rounding turns into piercings at some poses)."""
    r = env.robot
    adj = np.array([[r.link_index[j["parent"]], r.link_index[j["child"]]] for j in r.joints], np.int32)
    for q in ({}, {"shoulder": 1.2}, {"shoulder": -1.5, "waist": 0.7}):
        count, _, _ = ref.mesh_collide(r.tri, r.tri_start, r.fk(q, env.base), adj)
        assert count[0, 0] == 0 and count[0, 1] > 0 and count[0, 3] > 0


def test_cli_parses_reject_collisions():
    from autourdf_amd import sim_data
    assert sim_data.parse_args(["--robot", "toy", "--reject_collisions"]).reject_collisions is True
    assert sim_data.parse_args([]).reject_collisions is False


def test_collect_skips_colliding_seeds_and_gives_up_at_max_seeds(tmp_path, monkeypatch, capsys):
    from _toy_urdf import write_toy_robot
    from autourdf_amd import sim_data
    for d in (tmp_path, tmp_path / "plain", tmp_path / "never"):
        write_toy_robot(str(d))
    params = {"gt": "toy.urdf", "dof": 3, "excluded_pairs": [["l1", "l3"]], "collision_exclusion": True}
    seen, made = [], []

    def fake_collides(env, a_list, use_excluded=False):
        seed = len(seen)
        seen.append((np.asarray(a_list).shape, use_excluded, env.excluded_pairs))
        return [("base", "l3")] if seed in (0, 2) else []

    def fake_collection(env, data_path=None, **kw):
        made.append(data_path)
        return False, []

    monkeypatch.setattr(sim_data, "sequence_collides", fake_collides)
    monkeypatch.setattr(sim_data, "data_collection", fake_collection)
    paths = sim_data.collect("toy", params, num_step=4, epochs=3, num_cameras=3, root=str(tmp_path), reject_collisions=True)
    base = os.path.join(str(tmp_path), "data/raw/toy/4_deg_3_cams")
    assert [os.path.basename(p.rstrip("/")) for p in paths] == ["V0001", "V0003", "V0004"] and made == paths
    assert sorted(os.listdir(base)) == ["V0001", "V0003", "V0004"]                   # nothing for seeds 0 and 2
    assert seen == [((4, 3), True, [("l1", "l3")])] * 5
    out = capsys.readouterr().out
    assert "seed 0" in out and "seed 2" in out and "base" in out and "seed 1" not in out
    # the default is today's range(epochs): the check is not even called
    seen.clear()
    monkeypatch.setattr(sim_data, "sequence_collides", lambda *a, **k: pytest.fail("called without reject_collisions"))
    paths = sim_data.collect("toy", params, num_step=4, epochs=2, num_cameras=3, root=str(tmp_path / "plain"))
    assert [os.path.basename(p.rstrip("/")) for p in paths] == ["V0000", "V0001"]
    # every seed collides: give up after max_seeds, naming the pair
    monkeypatch.setattr(sim_data, "sequence_collides", lambda *a, **k: [("base", "l3"), ("l1", "tip")] if k or a else [])
    with pytest.raises(RuntimeError, match=r"base.*l3"):
        sim_data.collect("toy", params, num_step=4, epochs=1, num_cameras=3, root=str(tmp_path / "never"), reject_collisions=True, max_seeds=4)
    assert not os.path.exists(str(tmp_path / "never" / "data"))
