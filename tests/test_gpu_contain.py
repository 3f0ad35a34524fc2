"""creg_mesh_contain_f64 on the GPU against the numpy restatement of its contract (tests/_contain_ref.py): analytic cubes,
containers of every size around a wave, a chunk, the grid stride and each tree level, point counts, pair lists, poses,
determinism, untouched outputs and invalid calls -- then the toy robot through ops / SimEnv.

The value bound is |w - w_longdouble| <= K * 2^-53 * sum|omega_i| / (4 pi) with K = 256: the fp64 restatement against the
long-double one on exactly these inputs gave a largest ratio of 44.2 on the CPU (the one-triangle and 65-triangle caps; 11.1 on
the 66 048-triangle sphere, 3.0 on the cubes); 4 x that, rounded up to a power of two, is 256.  The factor 4 covers a device
atan2 a few ulp off and the deeper tree.  On one MI355X the kernel's largest ratio on these inputs was 44.2 as well (11.9 on the
large sphere).  Integer outputs, gated zeros and the inside decision are asserted exactly; identical
bits are printed when seen, not asserted."""
import ctypes
import os

import numpy as np
import pytest
import torch

import _contain_ref as cref

pytestmark = pytest.mark.gpu
K = 256.0


def dev(a):
    return torch.from_numpy(np.array(a)).to("cuda")


def run(tri, start, pts, pt_start, link_T, pairs, q_stride, want_winding=True):
    """inside, first, winding, link_box of the C entry; the outputs are pre-filled with -7."""
    from autourdf_amd import _lib
    lib = _lib.load()
    pairs = np.asarray(pairs, np.int32).reshape(-1, 2)
    link_T = np.asarray(link_T, np.float64)
    link_T = link_T[None] if link_T.ndim == 3 else link_T
    P, L, F, M, N = link_T.shape[0], link_T.shape[1], len(tri), len(pairs), len(pts)
    d_tri, d_start, d_pts, d_ps, d_T, d_pairs = dev(tri), dev(start), dev(pts), dev(pt_start), dev(link_T), dev(pairs)
    need = lib.creg_mesh_contain_workspace_bytes(F, L, P, M, q_stride)
    assert need > 0
    ws = torch.empty(need // 8, dtype=torch.float64, device="cuda")
    inside = torch.full((P, M, 2), -7, dtype=torch.int32, device="cuda")
    first = torch.full((P, M, 2), -7, dtype=torch.int32, device="cuda")
    wind = torch.full((P, M, 2, q_stride), -7.0, dtype=torch.float64, device="cuda")
    box = torch.full((P, L, 6), -7.0, dtype=torch.float64, device="cuda")
    ptr = lambda t: ctypes.c_void_p(t.data_ptr()) if t.numel() else None
    rc = lib.creg_mesh_contain_f64(ptr(d_tri), ptr(d_start), F, ptr(d_pts), ptr(d_ps), N, ptr(d_T), L, P, ptr(d_pairs), M, q_stride,
                                   ptr(inside), ptr(first), ptr(wind) if want_winding else None, ptr(box), ptr(ws), need, None)
    assert rc == 0, lib.creg_last_error()
    torch.cuda.synchronize()
    return inside.cpu().numpy(), first.cpu().numpy(), wind.cpu().numpy(), box.cpu().numpy()


def check(got, scene, q_stride, what=""):
    """Integers, gated zeros, decisions and boxes exactly; values within the bound of the long-double restatement."""
    inside, first, wind, box = got
    w_in, w_first, w_wind, w_box, exact, mag = cref.mesh_contain(*scene, q_stride, truth=True)
    np.testing.assert_array_equal(box, w_box)
    assert not np.isnan(wind).any() and (wind != -7.0).all()
    gated = mag == 0
    assert (wind[gated] == 0.0).all()                            # exactly 0.0, never summed
    truth = exact if cref.WIDE else w_wind.astype(np.longdouble)
    err = np.abs(wind.astype(np.longdouble) - truth).astype(np.float64)
    bound = K * 2.0 ** -53 * mag
    ratio = (err[~gated] / (2.0 ** -53 * mag[~gated])).max() if (~gated).any() else 0.0
    print(f"{what}: {(~gated).sum()} evaluated of {gated.size}, largest error {err.max():.3g} = {ratio:.3g} x 2^-53 sum|omega|/4pi "
          f"(bound {K:g}), bits identical to numpy: {wind.tobytes() == w_wind.tobytes()}")
    assert (err <= bound).all()
    assert (np.abs(np.abs(w_wind[~gated]) - 0.5) > 1e-3).all()   # the inputs stay far from the decision
    np.testing.assert_array_equal(inside, w_in)
    np.testing.assert_array_equal(first, w_first)
    return w_in, w_first, mag


# ------------------------------------------------------------------------------------------ analytic
def test_a_small_cube_inside_a_large_one_is_seen_by_neither_older_entry():
    from autourdf_amd import ops
    scene = cref.nested_cubes(P=3)
    tri, start, pts, pt_start, link_T, pairs = scene
    count, _ = ops.mesh_collide(dev(tri), dev(start), dev(link_T), dev(pairs))
    dist, _ = ops.mesh_clearance(dev(tri), dev(start), dev(link_T), dev(pairs), np.inf)
    assert (count.cpu().numpy() == 0).all() and (dist.cpu().numpy() > 0).all()  # not touching: today's entries see nothing
    got = run(*scene, 9)
    check(got, scene, 9, "nested cubes")
    inside, first, wind, _ = got
    assert pairs[0].tolist() == [0, 1]
    assert (inside[:, 0] == [0, 9]).all() and (first[:, 0] == [-1, 9]).all()      # every point of link 1 is inside link 0, none the other way
    assert (inside[:, 1:] == 0).all() and (first[:, 1:] == -1).all()
    assert np.abs(wind[:, 0, 1] - 1.0).max() < 1e-14 and (wind[:, 0, 0] == 0.0).all()


def test_reversed_orientation_open_cube_and_a_point_outside():
    flipped = cref.nested_cubes(P=1, flip=True)
    got = run(*flipped, 9)
    check(got, flipped, 9, "inward-oriented")
    assert np.abs(got[2][0, 0, 1] + 1.0).max() < 1e-14 and got[0][0, 0].tolist() == [0, 9]
    opened = cref.nested_cubes(P=1, opened=True)
    got = run(*opened, 9)
    check(got, opened, 9, "open cube")
    assert ((got[2][0, 0, 1] > 0.8) & (got[2][0, 0, 1] < 0.95)).all() and got[0][0, 0].tolist() == [0, 9]
    # the centre of the open cube: 5/6; a point outside a closed one but inside its box's reach: 0
    tri, start = cref.pack([cref.open_cube(0.1), cref.box_mesh(0.1, 0.1, 0.1), np.zeros((0, 3, 3))])
    pts, pt_start = np.array([[0.0, 0.0, 0.0], [0.05, 0.0, 0.0]]), np.array([0, 0, 0, 2], np.int64)
    R = cref.random_rotation(np.random.default_rng(3))
    link_T = np.array([[np.eye(4), cref.rigid(R, (0.0, 0.0, 0.0)), np.eye(4)]])
    got = run(tri, start, pts, pt_start, link_T, [[2, 0], [2, 1]], 2)
    assert np.abs(got[2][0, 0, 0] - [5 / 6, cref.winding(tri[:10], pts[1])]).max() < 1e-14 and got[0][0, 0, 0] == 2
    corner = np.array([[0.099, 0.099, 0.099]])                   # inside the rotated cube's box, outside the cube
    got = run(tri, start, corner, np.array([0, 0, 0, 1], np.int64), link_T, [[2, 1]], 1)
    assert abs(got[2][0, 0, 0, 0]) < 1e-14 and got[0][0, 0].tolist() == [0, 0] and got[1][0, 0].tolist() == [-1, -1]


# ------------------------------------------------------------------------------------------ container sizes
@pytest.mark.parametrize("kind,size", [("sphere", 0), ("sphere", 1), ("sphere", 2)] + [("cap", n) for n in cref.CAPS])
def test_containers_around_a_wave_a_chunk_the_grid_stride_and_each_tree_level(kind, size):
    """Closed spheres of 64, 256 and 66 048 triangles (258 chunks: two trips of the 128-wide grid, two upper tree levels) and
    open caps of 1 .. 32 769 triangles.  Points: inside, outside but within the box, outside the box, exactly on a box face
    (evaluated) and one nextafter beyond it (gated)."""
    scene = cref.container_scene(cref.container_mesh(kind, size))
    got = run(*scene, 8)
    _, _, mag = check(got, scene, 8, f"{kind} {size}")
    ev = cref.EVALUATED
    assert (got[2][0, 0, 0][~ev] == 0.0).all() and (mag[0, 0, 0][ev] > 0.0).all()   # the face points are evaluated, their neighbours are not
    assert (got[2][0, 0, 1] == 0.0).all() and got[0][0, 0, 1] == 0                  # the container's own point is far from the cube
    if kind == "sphere":
        assert got[0][0, 0, 0] == 2 and got[1][0, 0, 0] == 1                        # rows 1 and 2 of pts are inside
        assert np.abs(got[2][0, 0, 0, :2] - 1.0).max() < 1e-12 and np.abs(got[2][0, 0, 0, [2, 4, 6]]).max() < 1e-12


# ------------------------------------------------------------------------------------------ points, pairs, poses
def test_zero_one_and_sixteen_points_a_wide_stride_and_seventeen():
    from autourdf_amd import _lib
    rng = np.random.default_rng(2)
    tri, start = cref.pack([cref.uv_sphere(0.1), cref.box_mesh(0.01, 0.01, 0.01), cref.box_mesh(0.01, 0.01, 0.01), cref.box_mesh(0.3, 0.3, 0.3)])
    p16 = rng.uniform(-0.12, 0.12, (16, 3))
    p16 = p16[np.abs(np.linalg.norm(p16, axis=1) - 0.1) > 0.01]
    p16 = np.concatenate([p16, rng.uniform(-0.03, 0.03, (16 - len(p16), 3))])
    pts = np.concatenate([p16, [[0.0, 0.0, 0.05]]])
    pt_start = np.array([0, 0, 16, 17, 17], np.int64)            # link 0: none, link 1: 16, link 2: one, link 3: none
    link_T = np.tile(np.eye(4), (1, 4, 1, 1))
    pairs = [[1, 0], [2, 0], [0, 3], [3, 1]]
    for q in (16,):
        scene = (tri, start, pts, pt_start, link_T, pairs)
        got = run(*scene, q)
        w_in, _, _ = check(got, scene, q, "0 / 1 / 16 points")
        assert 3 <= w_in[0, 0, 0] <= 15 and w_in[0, 1].tolist() == [1, 0] and w_in[0, 2].tolist() == [0, 0]
        assert (got[2][0, 1, 0, 1:] == 0.0).all()                # the unused slots of a one-point link
    # a stride larger than needed
    few = (tri, start, pts[14:], np.array([0, 0, 2, 3, 3], np.int64), link_T, pairs)
    a, b = run(*few, 2), run(*few, 7)
    check(b, few, 7, "wide stride")
    assert a[0].tobytes() == b[0].tobytes() and a[1].tobytes() == b[1].tobytes() and a[2].tobytes() == np.ascontiguousarray(b[2][..., :2]).tobytes()
    assert (b[2][..., 2:] == 0.0).all()
    # 17 points in one link, and a stride below a link's count: CREG_EINVAL
    lib = _lib.load()
    many = np.concatenate([p16, [[0.0, 0.0, 0.05]]])
    ptr = lambda t: ctypes.c_void_p(t.data_ptr())
    d = [dev(x) for x in (tri, start, many, np.array([0, 0, 17, 17, 17], np.int64), link_T, np.asarray(pairs, np.int32))]
    need = lib.creg_mesh_contain_workspace_bytes(len(tri), 4, 1, 4, 16)
    ws = torch.empty(need // 8, dtype=torch.float64, device="cuda")
    ins = torch.full((1, 4, 2), 77, dtype=torch.int32, device="cuda")
    fst = torch.full((1, 4, 2), 77, dtype=torch.int32, device="cuda")
    for stride, ps in ((16, d[3]), (15, dev(pt_start))):
        rc = lib.creg_mesh_contain_f64(ptr(d[0]), ptr(d[1]), len(tri), ptr(d[2]), ptr(ps), 17, ptr(d[4]), 4, 1, ptr(d[5]), 4, stride, ptr(ins),
                                       ptr(fst), None, None, ptr(ws), need, None)
        assert rc == -1 and b"creg_mesh_contain_f64" in lib.creg_last_error()
        torch.cuda.synchronize()
        assert (ins == 77).all() and (fst == 77).all()


def test_pair_lists_reversed_repeated_invalid_and_none():
    scene = cref.nested_cubes(P=3)
    tri, start, pts, pt_start, link_T, _ = scene
    pairs = [[0, 1], [1, 0], [0, 1], [0, 3], [-1, 1], [2, 2], [1, 2]]
    mixed = (tri, start, pts, pt_start, link_T, pairs)
    got = run(*mixed, 9)
    check(got, mixed, 9, "mixed pairs")
    inside, first, wind, box = got
    assert inside[:, 0].tobytes() == inside[:, 2].tobytes() and wind[:, 0].tobytes() == wind[:, 2].tobytes()
    assert wind[:, 1, 0].tobytes() == wind[:, 0, 1].tobytes() and (inside[:, 1] == [9, 0]).all() and (first[:, 1] == [9, -1]).all()
    assert (inside[:, 3:6] == 0).all() and (first[:, 3:6] == -1).all() and (wind[:, 3:6] == 0.0).all()   # invalid pairs: 0, -1, zeros
    none = run(tri, start, pts, pt_start, link_T, np.zeros((0, 2), np.int32), 9)
    assert none[0].shape == (3, 0, 2) and none[2].shape == (3, 0, 2, 9)
    np.testing.assert_array_equal(none[3], box)                  # n_pairs == 0 fills link_box only
    one = run(tri, start, pts, pt_start, link_T[0], pairs, 9, want_winding=False)                        # P = 1, no winding output
    assert one[0].tobytes() == inside[:1].tobytes() and one[1].tobytes() == first[:1].tobytes() and (one[2] == -7.0).all()


def test_two_runs_and_a_pair_alone_give_identical_bits():
    big = cref.container_scene(cref.container_mesh("sphere", 2))
    a, b = run(*big, 8), run(*big, 8)
    for x, y in zip(a, b):
        assert x.tobytes() == y.tobytes()
    scene = cref.nested_cubes(P=3, opened=True)
    tri, start, pts, pt_start, link_T, pairs = scene
    a, b = run(*scene, 9), run(*scene, 9)
    for x, y in zip(a, b):
        assert x.tobytes() == y.tobytes()
    for m in range(len(pairs)):
        one = run(tri, start, pts, pt_start, link_T, pairs[m:m + 1], 9)
        for x, y in zip(one[:3], a[:3]):
            assert x.tobytes() == np.ascontiguousarray(y[:, m:m + 1]).tobytes()


def test_invalid_calls_return_einval_and_touch_nothing():
    from autourdf_amd import _lib
    lib = _lib.load()
    tri, start, pts, pt_start, link_T, pairs = cref.nested_cubes(P=1)
    P, L, F, M, N, Q = 1, 3, len(tri), len(pairs), len(pts), 9
    d_tri, d_start, d_pts, d_ps, d_T, d_pairs = dev(tri), dev(start), dev(pts), dev(pt_start), dev(link_T), dev(pairs)
    need = lib.creg_mesh_contain_workspace_bytes(F, L, P, M, Q)
    assert need >= 8 * 9 * F + 8 * M * 2 * Q and need % 8 == 0
    ws = torch.empty(need // 8, dtype=torch.float64, device="cuda")
    ins = torch.full((P, M, 2), 77, dtype=torch.int32, device="cuda")
    fst = torch.full((P, M, 2), 77, dtype=torch.int32, device="cuda")
    wnd = torch.full((P, M, 2, Q), 77.0, dtype=torch.float64, device="cuda")
    box = torch.full((P, L, 6), 77.0, dtype=torch.float64, device="cuda")
    ptr = lambda t: ctypes.c_void_p(t.data_ptr()) if t is not None else None

    def call(n_tri=F, n_pts=N, n_links=L, n_poses=P, n_pairs=M, q=Q, ws_bytes=need, pr=d_pairs, i=ins, f=fst, x=d_pts, ps=d_ps):
        return lib.creg_mesh_contain_f64(ptr(d_tri), ptr(d_start), n_tri, ptr(x), ptr(ps), n_pts, ptr(d_T), n_links, n_poses, ptr(pr), n_pairs,
                                         q, ptr(i), ptr(f), ptr(wnd), ptr(box), ptr(ws), ws_bytes, None)

    for kw in (dict(q=0), dict(q=17), dict(q=8), dict(n_pts=-1), dict(x=None), dict(ps=None), dict(ws_bytes=need - 8), dict(ws_bytes=0),
               dict(i=None), dict(f=None), dict(pr=None), dict(n_tri=1 << 31), dict(n_links=65536), dict(n_poses=0), dict(n_pairs=-1),
               dict(n_links=0), dict(n_tri=-1)):
        assert call(**kw) == -1, kw                               # CREG_EINVAL
        assert b"creg_mesh_contain_f64" in lib.creg_last_error()
        torch.cuda.synchronize()
        assert (ins == 77).all() and (fst == 77).all() and (wnd == 77.0).all() and (box == 77.0).all(), kw
    assert lib.creg_mesh_contain_workspace_bytes(-1, L, P, M, Q) == 0 and lib.creg_mesh_contain_workspace_bytes(F, L, P, M, 17) == 0
    assert call() == 0
    torch.cuda.synchronize()
    assert (ins != 77).all() and (fst != 77).all() and (wnd != 77.0).all() and (box != 77.0).all()


# ------------------------------------------------------------------------------------------ through the Python layers
def test_toy_tip_inside_base_through_ops_and_simenv(tmp_path, monkeypatch):
    import _collide_ref as ref
    from autourdf_amd import ops
    env = ref.toy(tmp_path)
    r = env.robot
    link_T = ops.urdf_fk(r.fk_table(), r.q_rows([{}, {}]), env.base).clone()
    link_T[1, r.link_index["tip"]] = torch.as_tensor(ref.rigid(None, (0.0, 0.0, 0.02)), device="cuda")   # the sphere (r 0.015) at the centre of base (0.2 x 0.2 x 0.04)
    plain = env.collisions(link_T)
    assert plain == [([], []), ([], [])]                         # today's behaviour, and it stays: no (base, tip) entry
    flagged = env.collisions(link_T, containment=True)
    assert flagged[0] == ([], []) and flagged[1] == ([("base", "tip", 0, -1, -1)], [])
    found = env.containment(link_T)
    assert found[0] == [] and len(found[1]) == 1
    inner, outer, n, w = found[1][0]
    assert (inner, outer, n) == ("tip", "base", 1) and abs(abs(w) - 1.0) < 1e-12
    assert env.self_collision_check({}, link_T=link_T[1], containment=True)[0] == [("base", "tip", 0, -1, -1)]
    near = env.clearance(link_T, 0.01)[1][0]
    hit = [c for c in near if c[:2] == ("base", "tip")]
    assert len(hit) == 1 and 0.004 < hit[0][2] < 0.0051           # wholly inside: a positive clearance without the flag
    near_c = env.clearance(link_T, 0.01, containment=True)[1][0]
    assert [c for c in near_c if c[:2] == ("base", "tip")] == [("base", "tip", 0.0) + hit[0][3:]]   # 0.0, and the witness stays
    assert [c for c in near_c if c[:2] != ("base", "tip")] == [c for c in near if c[:2] != ("base", "tip")]
    tight = env.clearance(link_T, 0.001, containment=True)[1][0]
    assert ("base", "tip", 0.0, -1, -1) in tight                   # beyond the margin: added without a witness
    assert env.collisions(link_T, margin=0.001, containment=True)[1][0] == tight
    # wrapper: shapes, dtypes and the argument checks
    dev_in = env._collide_inputs(False)
    pts, pt_start, _ = env._contain_inputs()
    tri = env._device_mesh()[0]
    inside, first, wind, box = ops.mesh_contain(tri, dev_in[2], pts, pt_start, link_T, dev_in[1], want_winding=True, want_boxes=True)
    M = len(dev_in[0])
    assert inside.dtype == torch.int32 and tuple(inside.shape) == (2, M, 2) and tuple(first.shape) == (2, M, 2)
    assert wind.dtype == torch.float64 and tuple(wind.shape) == (2, M, 2, 1) and tuple(box.shape) == (2, len(r.links), 6)
    assert int(inside.sum()) == 1 and len(ops.mesh_contain(tri, dev_in[2], pts, pt_start, link_T, dev_in[1])) == 2
    with pytest.raises(ValueError, match="pt_start"):
        ops.mesh_contain(tri, dev_in[2], pts, pt_start.flip(0).contiguous(), link_T, dev_in[1])
    with pytest.raises(ValueError, match="16"):
        ops.mesh_contain(tri, dev_in[2], pts[:1].repeat(17, 1), torch.tensor([0] + [17] * len(r.links), device="cuda"), link_T, dev_in[1])
    # without the flag the new entry is never reached
    monkeypatch.setattr(ops, "mesh_contain", lambda *a, **k: pytest.fail("mesh_contain called without containment=True"))
    assert env.collisions(link_T) == plain and env.clearance(link_T, 0.01)[1][0] == near


THREE = """<?xml version="1.0"?>
<robot name="three">
  <link name="base"><visual><geometry><box size="0.4 0.4 0.4"/></geometry></visual></link>
  <link name="arm"><visual><origin xyz="0 0 0.15" rpy="0 0 0"/><geometry><box size="0.02 0.02 0.3"/></geometry></visual></link>
  <link name="cube"><visual><geometry><box size="0.04 0.04 0.04"/></geometry></visual></link>
  <joint name="swing" type="revolute"><parent link="base"/><child link="arm"/><origin xyz="0 0 0.2" rpy="0 0 0"/>
    <axis xyz="0 0 1"/><limit lower="-1" upper="1" effort="1" velocity="1"/></joint>
  <joint name="plunge" type="prismatic"><parent link="arm"/><child link="cube"/><origin xyz="0 0 -0.2" rpy="0 0 0"/>
    <axis xyz="0 0 1"/><limit lower="0" upper="0.6" effort="1" velocity="1"/></joint>
</robot>
"""


def test_three_link_robot_through_data_collection_and_collect(tmp_path, capsys):
    """The cube rides a prismatic joint on the arm: at 0.6 it hangs above the arm, at 0 it sits at the centre of the base, wholly
    inside it (the generator parks a prismatic joint at 0)."""
    from autourdf_amd import ops
    from autourdf_amd.sim_data import SimEnv, collect, data_collection
    (tmp_path / "three.urdf").write_text(THREE)
    env = SimEnv(str(tmp_path / "three.urdf"), dof=1, radius=1.5, num_cameras=3)
    r = env.robot
    assert r.collision_pairs().tolist() == [[0, 2]]
    rows = np.array([[0.0], [0.1], [0.2]])
    q = [{"swing": a, "plunge": s} for (a,), s in zip(rows, (0.6, 0.55, 0.0))]
    link_T = ops.urdf_fk(r.fk_table(), r.q_rows(q), env.base)
    kw = dict(width=96, height=96, num_points=256, angle_list=rows, link_T=link_T)
    collision, record = data_collection(env, check_collision=True, containment=True, **kw)
    out = capsys.readouterr().out
    assert collision is True and len(record) == 2 and "collision detected" in out and "cube inside base" in out
    collision, record = data_collection(env, check_collision=True, **kw)           # without the flag the sequence is kept
    assert collision is False and len(record) == 3 and "inside" not in capsys.readouterr().out
    params = {"gt": "three.urdf", "dof": 1}
    ckw = dict(num_step=3, epochs=1, num_points=256, num_cameras=3, root=str(tmp_path), pix=96, reject_collisions=True)
    with pytest.raises(RuntimeError, match="only 0 of 1"):
        collect("three", params, containment=True, max_seeds=2, **ckw)
    out = capsys.readouterr().out
    assert "seed 0: cube inside base (step 0)" in out and "seed 1: cube inside base" in out and out.count("skipped") == 2
    assert not os.path.exists(tmp_path / "data")                 # a skipped seed writes nothing
    paths = collect("three", params, max_seeds=2, **ckw)         # without the flag seed 0 is kept
    assert len(paths) == 1 and sorted(os.listdir(paths[0]))[:3] == ["0000", "0001", "0002"]
