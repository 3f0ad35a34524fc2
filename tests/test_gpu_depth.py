"""Depth-camera frames on the GPU: creg_raster_depth_f64 and creg_depth_points_f64 bit-exact against the numpy restatements,
creg_segment_plane_f64 step by step (fits as minimisers, counts / selection / mask exactly, degenerate hypotheses, the refit),
and the frames end to end with the ground removed."""
import os

import numpy as np
import pytest
import torch

import _depth_ref as ref

pytestmark = pytest.mark.gpu
TH = 0.001


def dev(a):
    return torch.from_numpy(np.array(a)).to("cuda")              # a copy: the shared host arrays stay as they are


@pytest.fixture(scope="module")
def scene(tmp_path_factory):
    env, q, tri, own, T = ref.toy_on_ground(tmp_path_factory.mktemp("toy"), ground_cells=8)
    return dict(env=env, q=q, tri=tri, own=own, T=T, cams=env.cam_frames)


@pytest.fixture(scope="module")
def cloud(scene):
    """The toy's depth cloud on its ground, 3 cameras at 96 x 96, from the oracle's buffers (host arrays, left unchanged)."""
    depth = ref.oracle_depth(scene["tri"], scene["own"], scene["T"], scene["cams"], 96, 96)
    P, off = ref.back_project(depth, scene["cams"])
    P.setflags(write=False)
    return depth, P, off


def _raster(scene, cams, W, H, aspect=1.0):
    from autourdf_amd import ops
    return ops.raster_depth(dev(scene["tri"]), dev(scene["own"]), dev(scene["T"]), dev(cams), aspect=aspect, width=W, height=H)


# ------------------------------------------------------------------------------------------ raster entry
def test_raster_depth_equals_the_visibility_buffers_and_the_oracle(scene, cloud):
    from autourdf_amd import ops
    depth = _raster(scene, scene["cams"], 96, 96)
    pts = dev(np.array([[0.0, 0.0, 0.1]]))
    _, vdepth = ops.visibility(dev(scene["tri"]), dev(scene["own"]), dev(scene["T"]), dev(scene["cams"]), pts, width=96, height=96,
                               return_depth=True)
    assert depth.shape == (3, 96, 96) and torch.equal(depth, vdepth)
    np.testing.assert_array_equal(depth.cpu().numpy(), cloud[0])
    assert np.isinf(cloud[0]).any() and np.isfinite(cloud[0]).any()


# ------------------------------------------------------------------------------------------ depth_points
@pytest.mark.parametrize("W,H", [(96, 96), (70, 45), (200, 200)])
def test_depth_points_bit_exact_vs_restatement(scene, W, H):
    """3 cameras at 96 x 96; 70 x 45 with aspect 70 / 45 (no multiple of a wave or a block); 3 x 200 x 200 = 120000 pixels in 471
    blocks, more than one trip of the block-offset scan."""
    from autourdf_amd import ops
    aspect = W / H
    odepth = ref.oracle_depth(scene["tri"], scene["own"], scene["T"], scene["cams"], W, H, aspect=aspect)
    depth = _raster(scene, scene["cams"], W, H, aspect)
    np.testing.assert_array_equal(depth.cpu().numpy(), odepth)
    want, want_off = ref.back_project(odepth, scene["cams"], aspect=aspect)
    pts, off = ops.depth_points(depth, dev(scene["cams"]), aspect=aspect)
    assert off.dtype == torch.int64 and off.is_cuda and pts.dtype == torch.float64
    np.testing.assert_array_equal(off.cpu().numpy(), want_off)
    np.testing.assert_array_equal(pts.cpu().numpy(), want)
    assert len(want) > 0.5 * 3 * W * H
    pts2, off2 = ops.depth_points(depth, dev(scene["cams"]), aspect=aspect)                      # two runs are identical
    assert torch.equal(pts, pts2) and torch.equal(off, off2)


def test_depth_points_empty_camera_and_full_image(scene):
    """The middle camera looks away from the robot and the ground: an empty segment, equal consecutive offsets.  A camera straight
    above a ground that fills its image: every pixel is a point."""
    from autourdf_amd import ops
    cams = scene["cams"].copy()
    cams[1, 3:9] = -cams[1, 3:9]                                   # forward and right reversed: still a right-handed frame, facing outwards
    depth = _raster(scene, cams, 96, 96)
    pts, off = ops.depth_points(depth, dev(cams))
    want, want_off = ref.back_project(depth.cpu().numpy(), cams)
    assert want_off[1] == want_off[2] and want_off[1] > 0 and want_off[3] > want_off[2]
    np.testing.assert_array_equal(off.cpu().numpy(), want_off)
    np.testing.assert_array_equal(pts.cpu().numpy(), want)
    top = np.array([[0, 0, 1.0, 0, 0, -1.0, 1.0, 0, 0, 0, 1.0, 0]])
    depth = _raster(scene, top, 70, 45, 70 / 45)
    pts, off = ops.depth_points(depth, dev(top), aspect=70 / 45)
    assert off.tolist() == [0, 70 * 45] and pts.shape == (70 * 45, 3)
    np.testing.assert_array_equal(pts.cpu().numpy(), ref.back_project(depth.cpu().numpy(), top, aspect=70 / 45)[0])
    p = pts.cpu().numpy()
    assert p[:, 2].min() > -1e-12 and p[:, 2].max() > 0.3 and np.abs(p[:, 0]).max() < 1.0 * np.tan(np.pi / 6) * 70 / 45 + 1e-9
    # all cameras blind: no point at all
    pts, off = ops.depth_points(torch.full((2, 5, 7), float("inf"), dtype=torch.float64, device="cuda"), dev(cams[:2]))
    assert pts.shape == (0, 3) and off.tolist() == [0, 0, 0]


# ------------------------------------------------------------------------------------------ segment_plane: hypotheses
@pytest.mark.parametrize("n", [3, 6])
def test_segment_plane_hypotheses_are_unit_signed_minimisers(cloud, n):
    from autourdf_amd import ops
    _, P, off = cloud
    rng = np.random.default_rng(11 + n)
    samples = np.stack([rng.integers(0, off[s + 1] - off[s], (64, n)) for s in range(3)])
    want_valid = ~np.isnan(ref.segment_plane(P, off, samples, TH)[4][..., 0])
    assert want_valid.mean() >= 0.9                                # the seed's hypotheses are mostly proper planes
    out = ops.segment_plane(dev(P), dev(off), TH, ransac_n=n, samples=dev(samples), want_hypotheses=True)
    hyp = out[4].cpu().numpy()
    valid = ~np.isnan(hyp[..., 0])
    np.testing.assert_array_equal(valid, want_valid)
    assert (np.isnan(hyp[~valid])).all()
    extent = float(np.linalg.norm(P.max(0) - P.min(0)))
    for s in range(3):
        seg = P[off[s]:off[s + 1]]
        for h in np.flatnonzero(valid[s]):
            nv, d = hyp[s, h, :3], hyp[s, h, 3]
            c, C = ref.scatter(seg[samples[s, h]])
            assert abs(np.linalg.norm(nv) - 1.0) <= 1e-12
            assert abs(nv @ c + d) <= 1e-12 * extent
            j = int(np.argmax(np.abs(nv)))
            assert nv[j] > 0
            assert nv @ C @ nv <= np.linalg.eigh(C)[0][0] + 1e-12 * np.trace(C)


# ------------------------------------------------------------------------------------------ segment_plane: counts, selection, mask
def _check_counts(P, off, samples, n):
    """Run the kernel, recompute counts / best / count / mask in numpy from ITS hypothesis planes: all exactly equal."""
    from autourdf_amd import ops
    plane, mask, count, best, hp, hc = ops.segment_plane(dev(P), dev(off), TH, ransac_n=n, samples=dev(samples), want_hypotheses=True)
    wc, wb, wn, wm = ref.recount(P, off, hp.cpu().numpy(), TH)
    np.testing.assert_array_equal(hc.cpu().numpy(), wc)
    np.testing.assert_array_equal(best.cpu().numpy(), wb)
    np.testing.assert_array_equal(count.cpu().numpy(), wn)
    np.testing.assert_array_equal(mask.cpu().numpy(), wm)
    assert hc.dtype == torch.int32 and best.dtype == torch.int32 and count.dtype == torch.int64 and mask.dtype == torch.bool
    short = np.flatnonzero(np.diff(off) < n)
    assert (best.cpu().numpy()[short] == -1).all() and (plane.cpu().numpy()[short] == 0).all() and (wn[short] == 0).all()
    return plane.cpu().numpy(), mask.cpu().numpy(), count.cpu().numpy(), best.cpu().numpy(), hp.cpu().numpy(), hc.cpu().numpy()


def _packed(P, lengths):
    """A packed cloud whose segments are consecutive slices of P of the given lengths."""
    off = np.concatenate([[0], np.cumsum(lengths)]).astype(np.int64)
    assert off[-1] <= len(P)
    return np.ascontiguousarray(P[:off[-1]]), off


def _draw(rng, off, H, n):
    return np.stack([rng.integers(0, max(int(m), 1), (H, n)) for m in np.diff(off)])


@pytest.mark.parametrize("n,H", [(3, 1), (6, 65), (6, 1030)])
def test_segment_plane_counts_selection_and_mask_are_exact(cloud, n, H):
    """Segments of 1, n - 1 and exactly n points, an empty one between two full ones, one longer than a block's tile of 2048 points
    and no multiple of 64; H = 1, H = 65, and H = 1030 (more than the 1024 hypotheses staged at a time)."""
    _, P, off0 = cloud
    ground = P[off0[1]:off0[2]]                                    # one camera's cloud: ground and robot
    lengths = [1, n - 1, n, 700, 0, 900, 2048 + 1000 + 37]
    if H > 1024:
        lengths = [n, 300, 0, 2048 + 37]                           # the hypothesis chunks are what this case is about
    pts, off = _packed(ground, lengths)
    samples = _draw(np.random.default_rng(5), off, H, n)
    plane, mask, count, best, hp, hc = _check_counts(pts, off, samples, n)
    if H > 1:
        assert (best[np.diff(off) >= 300] >= 0).all() and (count[np.diff(off) >= 300] > 100).all()


def test_segment_plane_many_segments_one_block_each_several_trips(cloud):
    """600 segments, most of them empty: one block per segment, which then walks the three tiles of a 5037-point segment itself."""
    _, P, off0 = cloud
    lengths = np.zeros(600, np.int64)
    lengths[[0, 17, 300, 599]] = [5037, 64, 2049, 400]
    pts, off = _packed(P, lengths)
    samples = _draw(np.random.default_rng(6), off, 8, 6)
    plane, mask, count, best, hp, hc = _check_counts(pts, off, samples, 6)
    assert (best[lengths == 0] == -1).all() and (best[[0, 300]] >= 0).all()


def test_segment_plane_tie_goes_to_the_lower_index(cloud):
    from autourdf_amd import ops
    _, P, off = cloud
    drawn = _draw(np.random.default_rng(7), off, 64, 6)
    first = ref.segment_plane(P, off, drawn, TH)
    samples = np.empty_like(drawn)
    for s in range(3):                                            # every row a loser, but rows 5 and 9: two copies of the winner
        loser = int(np.argmin(first[5][s]))
        assert first[5][s, loser] < first[2][s]
        samples[s] = drawn[s, loser]
        samples[s, 5] = samples[s, 9] = drawn[s, first[3][s]]
    plane, mask, count, best, hp, hc = _check_counts(P, off, samples, 6)
    assert (best == 5).all()
    for s in range(3):
        assert hc[s, 5] == hc[s, 9] == count[s] == first[2][s] and np.array_equal(hp[s, 5], hp[s, 9])
    again = ops.segment_plane(dev(P), dev(off), TH, samples=dev(samples), want_hypotheses=True)
    for a, b in zip(again, (plane, mask, count, best, hp, hc)):   # two runs are identical, the refit included
        np.testing.assert_array_equal(a.cpu().numpy(), b)


# ------------------------------------------------------------------------------------------ segment_plane: degenerate, refit
def test_segment_plane_degenerate_hypotheses_are_invalid():
    from autourdf_amd import ops
    line = np.array([[0, 0, 0], [1, 1, 2], [2, 2, 4], [3, 3, 6], [5, 5, 10], [7, 7, 14]], np.float64)
    rng = np.random.default_rng(8)
    flat = np.concatenate([rng.integers(-9, 10, (40, 2)), np.full((40, 1), 3)], 1).astype(np.float64)     # the plane z = 3
    pts = np.concatenate([line, flat, line + [1, 0, 0]])
    off = np.array([0, 46, 52], np.int64)
    samples = np.zeros((2, 4, 6), np.int64)
    samples[0, 0] = 9                                             # six copies of one index
    samples[0, 1] = [0, 1, 2, 3, 4, 5]                            # exactly collinear, small integers
    samples[0, 2] = [6, 9, 13, 20, 31, 45]                        # a proper plane
    samples[0, 3] = [1, 1, 4, 4, 1, 4]                            # two distinct points
    samples[1] = [[0, 1, 2, 3, 4, 5], [5, 5, 5, 5, 5, 5], [0, 0, 2, 2, 4, 4], [3, 1, 3, 1, 3, 1]]          # a segment that is one line
    plane, mask, count, best, hp, hc = (t.cpu().numpy() for t in ops.segment_plane(dev(pts), dev(off), TH, samples=dev(samples),
                                                                                   want_hypotheses=True))
    assert np.isnan(hp[0, [0, 1, 3]]).all() and (hc[0, [0, 1, 3]] == 0).all()
    np.testing.assert_allclose(hp[0, 2], [0, 0, 1, -3], atol=1e-12)
    assert best[0] == 2 and count[0] == 40 and hc[0, 2] == 40
    np.testing.assert_array_equal(mask, np.concatenate([np.zeros(6, bool), np.ones(40, bool), np.zeros(6, bool)]))
    np.testing.assert_allclose(plane[0], [0, 0, 1, -3], atol=1e-12)
    assert np.isnan(hp[1]).all() and (hc[1] == 0).all() and best[1] == -1 and count[1] == 0 and (plane[1] == 0).all()
    # an index outside its segment invalidates the hypothesis, nothing is read
    samples[0, 2, 5] = 46
    samples[0, 0] = [6, 9, 13, 20, 31, -1]
    out = ops.segment_plane(dev(pts), dev(off), TH, samples=dev(samples), want_hypotheses=True)
    assert torch.isnan(out[4][0]).all() and out[3].tolist() == [-1, -1] and not out[1].any()
    with pytest.raises(ValueError):
        ops.segment_plane(dev(pts), dev(off), TH, ransac_n=2, samples=dev(samples[:, :, :2]))
    with pytest.raises(ValueError):
        ops.segment_plane(dev(pts), dev(off), TH, samples=dev(samples[:1]))
    with pytest.raises(ValueError):
        ops.segment_plane(dev(pts[:, :2]), None, TH)


def test_segment_plane_refit_vs_eigh_of_the_same_inliers(cloud):
    """The refit against the restatement's eigh fit of the SAME inliers (the kernel's mask).  The tolerance is not fixed beforehand:
    the restatement is summed in two orders (left to right, and exactly rounded by math.fsum), and the device's tree, a third order of
    the same sums, may differ from either by 100 x their spread, or by 1e-12 if that is larger.
    Measured on these inputs (3 cameras at 96 x 96, 5890 / 5783 / 5783 inliers): spread 1.2e-16 at most, so the bound is 1e-12.
    (The inliers are the ground and the few robot pixels within 1 mm of it, over about 1 m: the refit tilts by less than 1e-3.)"""
    from autourdf_amd import ops
    _, P, off = cloud
    samples = _draw(np.random.default_rng(9), off, 64, 6)
    plane, mask, count, best = (t.cpu().numpy() for t in ops.segment_plane(dev(P), dev(off), TH, samples=dev(samples)))
    assert (best >= 0).all() and (count > 3000).all()
    for s in range(3):
        a = ref.refit(P, off, mask, s, np.zeros(4), order="plain")
        b = ref.refit(P, off, mask, s, np.zeros(4), order="fsum")
        spread = float(np.abs(a - b).max())
        print(f"segment {s}: inliers {count[s]}, spread of two CPU summation orders {spread:.3e}, device - fsum {np.abs(plane[s] - b).max():.3e}")
        assert np.abs(plane[s] - b).max() <= max(100 * spread, 1e-12)
        np.testing.assert_allclose(plane[s], [0, 0, 1, 0], atol=1e-3)             # and it is the ground


def test_segment_plane_draws_its_own_samples_deterministically(cloud):
    from autourdf_amd import ops
    _, P, off = cloud
    a = ops.segment_plane(dev(P), dev(off), TH, 6, 32, rng=np.random.default_rng(3), want_hypotheses=True)
    b = ops.segment_plane(dev(P), dev(off), TH, 6, 32, rng=np.random.default_rng(3), want_hypotheses=True)
    for x, y in zip(a, b):
        np.testing.assert_array_equal(x.cpu().numpy(), y.cpu().numpy())
    assert a[4].shape == (3, 32, 4) and a[5].shape == (3, 32)
    one = ops.segment_plane(dev(P[off[0]:off[1]]), num_iterations=32, rng=np.random.default_rng(4))    # offsets=None: one segment
    assert one[0].shape == (1, 4) and one[3].item() >= 0 and abs(one[0][0, 2].item() - 1.0) < 1e-9


# ------------------------------------------------------------------------------------------ end to end
def test_depth_cloud_loses_the_ground_and_keeps_the_robot(scene):
    from autourdf_amd.sim_data import SimEnv
    env, q = scene["env"], scene["q"]
    pts, off = env.depth_cloud(q, 96, 96, rng=np.random.default_rng(0))
    kept = pts.cpu().numpy()
    assert off.tolist()[0] == 0 and off.tolist()[-1] == len(kept) and (np.diff(off.cpu().numpy()) > 50).all()
    far = np.linalg.norm(kept[:, :2], axis=1) > 0.12
    assert not (far & (np.abs(kept[:, 2]) < 0.001)).any()                          # the ground is gone
    bare = SimEnv(env.robot.path, dof=3, radius=1.2, num_cameras=3)                # the same robot without a ground
    free, free_off = bare.depth_cloud(q, 96, 96)
    free = free.cpu().numpy()
    robot = free[free[:, 2] > 0.002]
    assert len(robot) > 300
    rows = {r.tobytes() for r in kept}
    assert all(r.tobytes() in rows for r in robot)                                 # exact rows: no robot point above 2 mm is missing
    with_ground, wg_off = env.depth_cloud(q, 96, 96, remove_ground=False)
    assert len(with_ground) > 10 * len(kept) and wg_off[-1].item() == len(with_ground)


def test_data_collection_from_depth_images_with_ground_removal(tmp_path, scene):
    from autourdf_amd.cluster_icp import Segments
    from autourdf_amd.sim_data import angle_list, data_collection
    env = scene["env"]
    a = angle_list(2, 4, 3, env.joint_limits, np.array([0.9] * 3), seed_i=0)
    raw = str(tmp_path / "raw" / "V0000") + "/"
    kw = dict(angle_list=a, noise_flag=True, num_points=400, width=200, height=200, seed=2)
    collision, rec = data_collection(env, data_path=raw, source="depth", ground_flag=True, **kw)
    assert collision is False and len(rec) == 2 and all(c.points.shape == (400, 3) for c in rec)
    assert sorted(os.listdir(raw)) == ["0000", "0001", "noise.txt"]
    seg = Segments(raw)
    assert seg.data_size == 2
    np.testing.assert_array_equal(np.asarray(seg.pc_list[1].points), rec[1].points)
    z0 = rec[0].points[:, 2]                                                       # the noise-free frame: the robot, not its ground
    assert (np.abs(z0) < 0.001).mean() < 0.1 and z0.max() > 0.3
    _, again = data_collection(env, source="depth", ground_flag=True, **kw)
    for x, y in zip(rec, again):
        np.testing.assert_array_equal(x.points, y.points)                          # identical for a seed
    _, surf = data_collection(env, source="surface", **kw)
    assert not np.array_equal(surf[0].points, rec[0].points)
    _, default = data_collection(env, **kw)                                        # the default IS the surface path, unchanged
    for x, y in zip(surf, default):
        np.testing.assert_array_equal(x.points, y.points)
    with pytest.raises(RuntimeError):
        data_collection(env, source="depth", ground_flag=True, angle_list=a[:1], num_points=10 ** 6, width=64, height=64)
