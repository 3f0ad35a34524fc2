"""CPU: the rotation edge families of tests/_pose_edges.py reach the decisions they are built for, and the float32 /
float64 restatements agree with the oracle's arithmetic (the anchor of the GPU bit-exactness tests in test_gpu_pose_math.py)."""
import numpy as np
import torch

import _pose_edges as E


def _correctly_rounded_sqrt_pos(v):
    out = torch.zeros_like(v)
    pos = v > 0
    out[pos] = torch.sqrt(v[pos].double()).to(v.dtype)
    return out


def test_families_reach_every_matrix_to_quat_decision():
    labels, R64, R32 = E.stack(E.rotation_families())
    q, qa, c, den, w = E.matrix_to_quat_parts(R32, np.float32)
    assert (np.bincount(c, minlength=4) > 0).all()                        # each of the four candidates wins somewhere
    top = np.sort(qa, 1)
    tie = top[:, 3] == top[:, 2]
    assert {"pi_exact", "half_pi_exact"} <= set(labels[tie].tolist())        # exact qa ties (first maximum taken)
    # ... including the tie 90 deg about x makes, qa[0] == qa[1], resolved to candidate 0
    hx = np.nonzero(labels == "half_pi_exact")[0][0]
    assert qa[hx, 0] == qa[hx, 1] and c[hx] == 0
    zero = q[:, 0] == 0
    assert (zero & ~np.signbit(q[:, 0])).any() and (zero & np.signbit(q[:, 0])).any()   # w = +0.0 and w = -0.0
    assert (w < 0).any() and (w > 0).any()                                   # the w >= 0 flip taken and not taken
    # the 0.1 floor: the four sqrt arguments sum to 4, so the chosen qa is >= 1 and its denominator is never floored; the
    # floor only binds for the candidates not chosen (which the oracle evaluates too), and those rows are here
    assert (qa <= np.float32(0.1)).any(1).sum() > 100
    assert (den >= np.float32(2) * (1 - 2.0 ** -22)).all()
    # f32 and f64 choose different signs of w near pi somewhere in the 1e-5 band? not required, but the band is there
    near = np.char.startswith(labels.astype(str), "near_pi")
    assert near.sum() >= 512 and (np.abs(w[near]) < 1e-5).all()


def test_restatements_equal_the_oracle_in_float32():
    """The float32 restatement is oracle.transforms evaluated in float32, bit for bit, on every row (ties included: both take
    the first maximum).  torch's CPU float32 sqrt is not correctly rounded (about 1 argument in 5 is 1 ulp off); the kernels'
    is, so the oracle is evaluated with a correctly rounded sqrt here -- the decision rule and the remaining arithmetic are
    the oracle's own."""
    from oracle import dq as OD
    from oracle import transforms as OT
    labels, R64, R32 = E.stack(E.rotation_families())
    orig = OT._sqrt_pos
    OT._sqrt_pos = _correctly_rounded_sqrt_pos
    try:
        o = OT.matrix_to_quaternion(torch.from_numpy(R32)).numpy()
        t = np.random.default_rng(0).uniform(-1, 1, size=(len(R32), 3)).astype(np.float32)
        M = E.poses(R32, t)
        odq = OD.transform_to_dualquat(torch.from_numpy(M)).numpy()
    finally:
        OT._sqrt_pos = orig
    np.testing.assert_array_equal(E.matrix_to_quat(R32, np.float32).view(np.int32), o.view(np.int32))
    np.testing.assert_array_equal(E.se3_to_dq(M, np.float32).view(np.int32), odq.view(np.int32))
    q = E.matrix_to_quat(R32, np.float32)
    np.testing.assert_array_equal(E.quat_to_matrix(q, np.float32), OT.quaternion_to_matrix(torch.from_numpy(q)).numpy())
    _, d64, d32 = E.stack(E.dualquat_families())
    d = torch.from_numpy(d32)
    np.testing.assert_array_equal(E.dq_to_se3(d32, np.float32)[:, :3, 3], OD.dualquat_to_transform(d).numpy()[:, :3, 3])
    np.testing.assert_array_equal(E.dq_invert(d32, np.float32), OD.dualquat_invert(d).numpy())
    np.testing.assert_array_equal(E.dq_multiply(d32, d32[::-1], np.float32), OD.dualquat_multiply(d, d.flip(0)).numpy())
    qq, tt = E.dq_to_quat_trans(d32, np.float32)
    oq, ot = OD.dualquat_to_quat_trans(d)
    np.testing.assert_array_equal(qq, oq.numpy())
    np.testing.assert_array_equal(tt, ot.numpy())
    # float64: k_pose_coords' instantiation against the oracle's coordinates
    from oracle import coord_map as OC
    M64 = E.poses(R64, t.astype(np.float64))
    np.testing.assert_allclose(E.matrix_to_quat(R64, np.float64), OC.coords_from_matrices(M64)[:, 3:], rtol=0, atol=1e-15)


def test_quaternion_and_dual_families():
    lq, q64, q32 = E.stack(E.quaternion_families())
    n = np.linalg.norm(q64, axis=1)
    assert n.min() < 2e-4 and n.max() > 5e2
    assert (q32[:, 0] < 0).any()
    assert ((q32[:, 0] == 0) & np.signbit(q32[:, 0])).any() and ((q32[:, 0] == 0) & ~np.signbit(q32[:, 0])).any()
    ld, d64, d32 = E.stack(E.dualquat_families())
    r2 = np.sum(d32[:, :4].astype(np.float64) ** 2, axis=1)
    # DQ_INV clamps |real|^2 at FLT_EPSILON: rows on both sides of it, and an exactly zero real part
    assert (r2 == 0).any() and ((r2 > 0) & (r2 < E.FLT_EPSILON)).any() and ((r2 > E.FLT_EPSILON) & (r2 < 2 * E.FLT_EPSILON)).any()
    # rpy: pitch near +-pi/2 on both sides, and the exact gimbal lock
    fams = dict(E.rpy_families())
    assert {"pitch_+0.001", "pitch_-0.001", "pitch_+0.01", "pitch_-0.01", "gimbal_lock"} <= set(fams)
    assert np.abs(E.euler_xyz_to_rot64(fams["gimbal_lock"])[:, 0, 2]).min() == 1.0


def test_coord_tracks_reach_rotvec_roundtrip_branches():
    """Relative step rotations of coord_tracks reach both series branches of rotvec_roundtrip (angle <= 1e-3 and above, on
    both sides of the switch), the shortest-arc flip, and every branch of rotmat_to_unitquat_xyzw."""
    for K in (1, 64, 65):
        M, steps = E.coord_tracks(4, K, seed=K)
        assert M.shape == (4, K, 4, 4)
    M, steps = E.coord_tracks(4, 65, seed=65)
    rel = np.swapaxes(M[:-1, :, :3, :3], -1, -2) @ M[1:, :, :3, :3]
    q, c = E.rotmat_to_unitquat_xyzw(rel.reshape(-1, 3, 3))
    flip, a_series, n_series = E.rotvec_branches(q)
    assert flip.any() and a_series.any() and (~a_series).any() and n_series.any() and (~n_series).any()
    assert (np.bincount(c, minlength=4) > 0).all()
    step = np.tile(np.array(steps), 3)
    assert a_series[step == "1e-3-1e-9"].all() and not a_series[step == "1e-3+1e-9"].any()
    from oracle import coord_map as OC
    np.testing.assert_allclose(q, OC.rotmat_to_unitquat(rel.reshape(-1, 3, 3)), rtol=0, atol=4e-16)
