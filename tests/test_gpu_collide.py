"""creg_mesh_collide_f64 on the GPU: count, first and link_box compared exactly with the numpy restatement of the contract
(tests/_collide_ref.py) -- the lattice cases, links of every size around a wave and a tile, pose and pair batches, containment,
invalid calls -- then the toy robot's contacts and data_collection(check_collision=True)."""
import ctypes
import os

import numpy as np
import pytest
import torch

import _collide_ref as ref

pytestmark = pytest.mark.gpu


def dev(a):
    return torch.from_numpy(np.array(a)).to("cuda")              # a copy: the shared host arrays stay as they are


def run(tri, start, link_T, pairs):
    from autourdf_amd import ops
    pairs = np.asarray(pairs, np.int32).reshape(-1, 2)
    count, first, box = ops.mesh_collide(dev(tri), dev(start), dev(link_T), dev(pairs), want_boxes=True)
    assert count.dtype == torch.int32 and first.dtype == torch.int32 and box.dtype == torch.float64
    return count.cpu().numpy(), first.cpu().numpy(), box.cpu().numpy()


def same(got, want):
    for g, w in zip(got, want):
        assert g.shape == w.shape
        np.testing.assert_array_equal(g, w)


@pytest.fixture(scope="module")
def sizes():
    tri, start, link_T, pairs = ref.sizes_scene(P=5)
    want = ref.mesh_collide(tri, start, link_T, pairs)
    for a in (tri, start, link_T, pairs) + want:
        a.setflags(write=False)
    return tri, start, link_T, pairs, want


# ------------------------------------------------------------------------------------------ the kernel against the restatement
@pytest.mark.parametrize("name", sorted(ref.LATTICE))
def test_lattice_cases_as_two_one_triangle_links(name):
    other, n = ref.LATTICE[name]
    tri, start = ref.pack([[ref.BASE], [other]])
    link_T = np.tile(np.eye(4), (1, 2, 1, 1))
    got = run(tri, start, link_T, [[0, 1], [1, 0]])
    same(got, ref.mesh_collide(tri, start, link_T, [[0, 1], [1, 0]]))
    assert got[0].tolist() == [[n, n]] and got[1].tolist() == ([[[0, 1], [1, 0]]] if n else [[[-1, -1]] * 2])


def test_links_of_every_size_around_a_wave_and_a_tile(sizes):
    """Links of 1, 63, 64, 65, 255, 256, 257 and 552 triangles, a box and an empty link, all 45 pairs, P = 2."""
    tri, start, link_T, pairs, want = sizes
    assert np.diff(start).tolist() == list(ref.SIZES)
    got = run(tri, start, link_T[:2], pairs)
    same(got, [w[:2] for w in want])
    hit = want[0][:2] > 0
    assert hit.sum() >= 20 and (~hit).sum() >= 20                # both outcomes
    for l, n in enumerate(ref.SIZES):                            # every link with triangles collides somewhere
        assert (hit[:, (pairs == l).any(1)].any()) == (n > 0)
    assert np.isinf(got[2][:, -1]).all() and (got[2][:, -1, :3] > 0).all() and (got[2][:, -1, 3:] < 0).all()


def test_one_pose_from_a_3d_input_and_five_poses(sizes):
    tri, start, link_T, pairs, want = sizes
    same(run(tri, start, link_T[3], pairs), [w[3:4] for w in want])
    same(run(tri, start, link_T, pairs), want)


def test_pair_lists_one_none_swapped_repeated_and_the_empty_link(sizes):
    tri, start, link_T, pairs, want = sizes
    m = int(np.flatnonzero(want[0][0] > 0)[0])
    i, j = pairs[m]
    one = run(tri, start, link_T[:1], [[i, j]])
    assert one[0][0, 0] == want[0][0, m] > 0 and one[1][0, 0].tolist() == want[1][0, m].tolist()
    none = run(tri, start, link_T[:2], np.zeros((0, 2), np.int32))
    assert none[0].shape == (2, 0) and none[1].shape == (2, 0, 2)
    np.testing.assert_array_equal(none[2], want[2][:2])          # M = 0 fills the link boxes only
    empty = len(ref.SIZES) - 1
    mixed = [[i, j], [j, i], [i, j], [i, empty], [empty, j]]
    got = run(tri, start, link_T[:1], mixed)
    same(got, ref.mesh_collide(tri, start, link_T[:1], mixed))
    assert got[0][0].tolist() == [one[0][0, 0]] * 3 + [0, 0]
    assert got[1][0, 1].tolist() != got[1][0, 0].tolist()        # the swapped pair has its own smallest (a, b) ...
    assert start[j] <= got[1][0, 1, 0] < start[j + 1] and start[i] <= got[1][0, 1, 1] < start[i + 1]


def test_a_long_link_takes_more_than_one_trip_of_the_tile_grid():
    tri, start, link_T, pairs = ref.long_scene()
    want = ref.mesh_collide(tri, start, link_T, pairs)
    same(run(tri, start, link_T, pairs), want)
    assert want[0][0].tolist()[:4] == [want[0][0, 0]] * 2 + [want[0][0, 2]] * 2 and (want[0][0, :4] > 0).all()
    assert want[0][0, 4:].tolist() == [0, 0]


def test_containment_is_not_detected_and_far_links_are_free():
    tri, start = ref.pack([ref.uv_sphere(0.2), ref.uv_sphere(0.05), ref.uv_sphere(0.05)])
    link_T = np.array([[ref.rigid(), ref.rigid(None, (0.02, 0.01, 0.0)), ref.rigid(None, (3.0, 0, 0))]])
    got = run(tri, start, link_T, ref.all_pairs(3))
    same(got, ref.mesh_collide(tri, start, link_T, ref.all_pairs(3)))
    assert got[0].tolist() == [[0, 0, 0]] and (got[1] == -1).all()
    box = got[2][0]
    assert (box[0, :3] < box[1, :3]).all() and (box[1, 3:] < box[0, 3:]).all()      # inside: the boxes do overlap
    assert box[2, 0] > box[0, 3]                                                     # far: they do not


def test_two_runs_are_identical(sizes):
    tri, start, link_T, pairs, _ = sizes
    a, b = run(tri, start, link_T, pairs), run(tri, start, link_T, pairs)
    for x, y in zip(a, b):
        assert x.tobytes() == y.tobytes()


def test_the_three_mesh_queries_return_the_same_link_boxes(sizes):
    """mesh_collide, mesh_clearance and mesh_contain run one posing stage: their link_box outputs agree byte for byte (P = 2)."""
    from autourdf_amd import ops
    tri, start, link_T, pairs, want = sizes
    d = [dev(x) for x in (tri, start, link_T[:2], pairs)]
    no_pts, no_rows = torch.zeros(0, 3, dtype=torch.float64, device="cuda"), torch.zeros(len(start), dtype=torch.int64, device="cuda")
    boxes = [ops.mesh_collide(*d, want_boxes=True)[-1], ops.mesh_clearance(*d, 0.02, want_boxes=True)[-1],
             ops.mesh_contain(d[0], d[1], no_pts, no_rows, d[2], d[3], want_boxes=True)[-1]]
    raw = [b.cpu().numpy().tobytes() for b in boxes]
    assert raw[0] == raw[1] == raw[2]
    np.testing.assert_array_equal(boxes[0].cpu().numpy(), want[2][:2])


def test_wrapper_raises_for_bad_pairs_and_shapes(sizes):
    from autourdf_amd import ops
    tri, start, link_T, pairs, _ = sizes
    L = link_T.shape[1]
    for bad in ([[0, L]], [[-1, 2]], [[3, 3]]):
        with pytest.raises(ValueError, match="pair"):
            ops.mesh_collide(dev(tri), dev(start), dev(link_T), dev(np.array(bad, np.int32)))
    with pytest.raises(ValueError):
        ops.mesh_collide(dev(tri), dev(start[:-1]), dev(link_T), dev(pairs))
    with pytest.raises(ValueError, match="tri_start"):
        ops.mesh_collide(dev(tri), dev(start[::-1].copy()), dev(link_T), dev(pairs))
    with pytest.raises(TypeError):
        ops.mesh_collide(dev(tri), dev(start.astype(np.int32)), dev(link_T), dev(pairs))
    with pytest.raises(RuntimeError):
        ops.mesh_collide(torch.from_numpy(np.array(tri)), dev(start), dev(link_T), dev(pairs))


def test_invalid_calls_return_einval_and_touch_nothing(sizes):
    """n_poses < 1, n_pairs < 0, n_links < 1, n_tri < 0, a short workspace: CREG_EINVAL, a message, nothing launched.  A pair that
    names a link outside [0, L) or one link twice reaches the kernel only through the C ABI: count 0, (-1,-1)."""
    from autourdf_amd import _lib
    lib = _lib.load()
    tri, start, link_T, pairs, want = sizes
    P, L, F, M = 1, link_T.shape[1], len(tri), len(pairs)
    d_tri, d_start, d_T, d_pairs = dev(tri), dev(start), dev(link_T[:1]), dev(pairs)
    need = lib.creg_mesh_collide_workspace_bytes(F, L, P, M)
    assert need >= 8 * 9 * F and need % 8 == 0
    ws = torch.empty(need // 8, dtype=torch.float64, device="cuda")
    count = torch.full((P, M), 77, dtype=torch.int32, device="cuda")
    first = torch.full((P, M, 2), 77, dtype=torch.int32, device="cuda")
    box = torch.full((P, L, 6), 77.0, dtype=torch.float64, device="cuda")
    ptr = lambda t: ctypes.c_void_p(t.data_ptr())

    def call(n_tri=F, n_links=L, n_poses=P, n_pairs=M, ws_bytes=need, pr=d_pairs):
        return lib.creg_mesh_collide_f64(ptr(d_tri), ptr(d_start), n_tri, ptr(d_T), n_links, n_poses, ptr(pr), n_pairs, ptr(count),
                                         ptr(first), ptr(box), ptr(ws), ws_bytes, None)

    for kw in (dict(n_poses=0), dict(n_poses=-3), dict(n_pairs=-1), dict(n_links=0), dict(n_tri=-1), dict(ws_bytes=need - 8), dict(ws_bytes=0)):
        assert call(**kw) == -1, kw                               # CREG_EINVAL
        assert b"creg_mesh_collide_f64" in lib.creg_last_error()
        torch.cuda.synchronize()
        assert (count == 77).all() and (first == 77).all() and (box == 77.0).all(), kw
    bad = np.array(pairs)
    bad[0], bad[1], bad[2] = (0, L), (-1, 1), (4, 4)
    assert call(pr=dev(bad)) == 0
    torch.cuda.synchronize()
    np.testing.assert_array_equal(count.cpu().numpy()[0, 3:], want[0][0, 3:])
    np.testing.assert_array_equal(first.cpu().numpy()[0, 3:], want[1][0, 3:])
    assert count[0, :3].tolist() == [0, 0, 0] and (first[0, :3] == -1).all()
    np.testing.assert_array_equal(box.cpu().numpy(), want[2][:1])


# ------------------------------------------------------------------------------------------ the toy robot
@pytest.fixture(scope="module")
def env(tmp_path_factory):
    return ref.toy(tmp_path_factory.mktemp("toy"))


def test_toy_self_collision_check(env):
    assert env.self_collision_check({}) == ([], [])
    q = {"shoulder": 2.9}
    self_c, floor_c = env.self_collision_check(q)
    want = ref.toy_contacts(env, q)
    assert self_c == want and [c[:2] for c in self_c] == [("base", "l3")] and self_c[0][2] > 0 and floor_c == []
    from autourdf_amd import ops
    r = env.robot
    rows = [{}, {"shoulder": 1.2}, q, {"shoulder": -1.5}, {"shoulder": -2.7, "wrist": 1.0}]
    link_T = ops.urdf_fk(r.fk_table(), r.q_rows(rows), env.base)
    hits = env.collisions(link_T)
    assert [bool(s) for s, _ in hits] == [False, False, True, False, True] and all(f == [] for _, f in hits)
    assert [c[:2] for c in hits[4][0]] == [("base", "l3")]
    excl = ref.toy(os.path.dirname(r.path), excluded_pairs=[("l3", "base"), ("nosuch", "l1")])
    assert excl.self_collision_check(q) == (self_c, []) and excl.self_collision_check(q, use_excluded=True) == ([], [])


def test_toy_floor_contact_needs_a_ground(env):
    grounded = ref.toy(os.path.dirname(env.robot.path), ground_flag=True, ground_cells=4)
    q = {"shoulder": 2.9}
    r = grounded.robot
    low = ref.mesh_collide(r.tri, r.tri_start, r.fk(q, grounded.base), r.collision_pairs())[2][0, :, 2]
    want = [r.links[l] for l in np.flatnonzero(low < 0) if r.links[l] != r.root]
    assert want == ["l3", "tip"]
    self_c, floor_c = grounded.self_collision_check(q)
    assert floor_c == want and self_c == ref.toy_contacts(grounded, q)
    assert grounded.self_collision_check({}) == ([], [])
    assert env.self_collision_check(q)[1] == []                  # the same pose without a ground


def _ply_points(path):
    raw = open(path, "rb").read()
    return np.frombuffer(raw[raw.index(b"end_header\n") + 11:], "<f8").reshape(-1, 3)


def test_data_collection_stops_at_the_first_colliding_row(env, tmp_path, capsys):
    from autourdf_amd.sim_data import data_collection
    kw = dict(width=96, height=96, num_points=256, noise_flag=True, seed=2)
    rows = np.array([[0.0, 0.0, 0.0], [0.2, 0.5, 0.1], [0.2, 2.9, 0.1], [0.4, -1.0, 0.3]])
    raw = str(tmp_path / "hit") + "/"
    collision, record = data_collection(env, data_path=raw, angle_list=rows, check_collision=True, **kw)
    assert collision is True and len(record) == 2
    assert sorted(os.listdir(raw)) == ["0000", "0001"]                             # no later step, no noise.txt
    out = capsys.readouterr().out
    assert "collision detected" in out and "base" in out and "l3" in out
    free = rows[[0, 1, 3, 1]]
    a, b = str(tmp_path / "checked") + "/", str(tmp_path / "plain") + "/"
    c1, rec1 = data_collection(env, data_path=a, angle_list=free, check_collision=True, **kw)
    c0, rec0 = data_collection(env, data_path=b, angle_list=free, **kw)
    assert c1 is False and c0 is False and len(rec1) == len(rec0) == 4
    for x, y in zip(rec1, rec0):
        assert np.asarray(x.points).tobytes() == np.asarray(y.points).tobytes()
    assert sorted(os.listdir(a)) == sorted(os.listdir(b)) == ["0000", "0001", "0002", "0003", "noise.txt"]
    for step in ("0000", "0003"):
        assert open(a + step + "/robot.ply", "rb").read() == open(b + step + "/robot.ply", "rb").read()
    assert open(a + "noise.txt", "rb").read() == open(b + "noise.txt", "rb").read()
    np.testing.assert_array_equal(_ply_points(raw + "0001/robot.ply"), _ply_points(a + "0001/robot.ply"))   # the steps before the stop are the plain ones
    # collision_flag=True applies the env's excluded pairs: with base-l3 excluded the same rows run through
    excl = ref.toy(os.path.dirname(env.robot.path), excluded_pairs=[("base", "l3")])
    assert data_collection(excl, angle_list=rows, check_collision=True, **kw)[0] is True
    collision, record = data_collection(excl, angle_list=rows, check_collision=True, collision_flag=True, **kw)
    assert collision is False and len(record) == 4
