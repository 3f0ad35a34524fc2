"""Score a written URDF against its ground truth (``Sim/evaluation.py`` of the reference), headless:

* ``compare_joints`` (:84-224): per-joint position error (normal distance of the two joint lines) and direction error
  (angle of the two axes, folded at 90 degrees with the sign kept in ``dir_map``);
* ``evaluation`` (:228-380): both robots posed at the same random commands, a cloud of each through the frame generator
  (``sim_data.data_collection``), the predicted one ICP-aligned (:358-362, point-to-point, threshold 0.01, identity start,
  max 20000 iterations), then ``torch_chamfer_distance`` (:69-81, L1 Chamfer in float32);
* ``main`` (:383-449): ``python -m autourdf_amd.evaluation --robot ...`` writes ``loss.txt``, ``loss_mean_std.txt``,
  ``pos_mean_std.txt`` and ``dir_mean_std.txt`` under ``data/evaluation2/``.

The robots are posed by one batched forward-kinematics launch per robot (``ops.urdf_fk``, creg_urdf_fk_f64): all link
poses of all commands, and every joint's world line.  A joint's line is the geometric one: the joint frame's origin
``(T_parent origin)[:3, 3]`` and the axis ``(T_parent origin)[:3, :3] axis``.  The reference composes its line from
PyBullet's inertial-frame link states; the two agree whenever the joint origin carries no rotation.
PyBullet, Open3D and pytorch3d are not needed; the viewer flags raise.  ``joint_error``, ``map_commands`` and
``load_offset`` are host logic; everything that touches a cloud or a pose runs on the GPU and has no CPU fallback."""
import glob
import os

import numpy as np
import torch

from . import _lib, ops
from .cluster_icp import PointCloud


def _points(p):
    return np.asarray(p.points if hasattr(p, "points") else p, dtype=np.float64).reshape(-1, 3)


def torch_chamfer_distance(p1, p2):
    """p1, p2: point clouds (objects with ``.points`` or arrays).  L1 Chamfer distance in float32 (K1)."""
    dev = _lib.device()
    a = torch.as_tensor(_points(p1), dtype=torch.float32, device=dev)
    b = torch.as_tensor(_points(p2), dtype=torch.float32, device=dev)
    return ops.chamfer_distance(a[None], b[None], norm=1)[0].item()


def icp_filter(pred_pcd, gt_pcd, threshold=0.01, max_iteration=20000):
    """registration_icp(pred, gt, threshold, I, point-to-point) and pred moved by the result.
    Returns (transformation (4,4) float64, moved PointCloud).  Clouds above 1024 source points / 65536 targets run in K4's
    many-workgroup regime (round 5: point-to-point mode there too -- 64 sources per workgroup, cell grid over the target cloud),
    smaller ones as one workgroup."""
    dev = _lib.device()
    src = torch.as_tensor(_points(pred_pcd), device=dev)
    tgt = torch.as_tensor(_points(gt_pcd), device=dev)
    soff = torch.tensor([0, src.shape[0]], dtype=torch.int32, device=dev)
    toff = torch.tensor([0, tgt.shape[0]], dtype=torch.int32, device=dev)
    init = torch.eye(4, dtype=torch.float64, device=dev).reshape(1, 4, 4)
    T, moved, _ = ops.icp_p2p(src, soff, tgt, toff, init, th=threshold, max_iteration=max_iteration)
    return T[0].cpu().numpy(), PointCloud(moved.cpu().numpy())


# ------------------------------------------------------------------------------------------ host logic
def load_offset(raw_data_path):
    """The driven joints' values of the first sequence's first frame (``*/0000/joint_cfg.txt``, evaluation.py:16-24)."""
    offset = []
    config_files = sorted(glob.glob(raw_data_path + '/*/'))
    for line in open(config_files[0] + '0000/joint_cfg.txt', 'r'):
        offset.append(float(line.split(':')[-1]))
    return np.array(offset)


def joint_error(pos_a, uv_a, pos_b, uv_b):
    """Normal distance of two lines (point + unit direction each) and the angle of their directions in degrees
    (evaluation.py:28-66): parallel lines give the distance of pos_b from line a; the dot product is clipped to [-1, 1]."""
    pos_a, uv_a, pos_b, uv_b = (np.asarray(v, np.float64) for v in (pos_a, uv_a, pos_b, uv_b))
    cross_product = np.cross(uv_a, uv_b)
    cross_product_magnitude = np.linalg.norm(cross_product)
    diff = pos_b - pos_a
    if cross_product_magnitude == 0:
        pos_error = np.linalg.norm(np.cross(diff, uv_a))
    else:
        pos_error = np.abs(np.dot(diff, cross_product)) / cross_product_magnitude
    dot_product = np.clip(np.dot(uv_a, uv_b), -1.0, 1.0)
    dir_error = np.degrees(np.arccos(dot_product))
    return pos_error, dir_error


def map_commands(a_list, joint_map, direction_map):
    """Ground-truth commands (P, dof) -> the predicted robot's commands (evaluation.py:259-264): multiply column i by
    direction_map[i], then reorder by the inverse permutation, so column joint_map[i] of the result drives the predicted
    joint that matches ground-truth joint i."""
    a_list = np.asarray(a_list, np.float64)
    joint_map = np.asarray(joint_map).astype(np.int64).reshape(-1)
    direction = np.array(direction_map)
    inv_map = np.empty_like(joint_map)
    inv_map[joint_map] = np.arange(len(joint_map))
    a_list_direction = a_list * direction
    a_list_mapped = a_list_direction[:, inv_map]
    return a_list_mapped


# ------------------------------------------------------------------------------------------ joints
def _joint_lines(env, q_by_joint):
    """{joint name: (world position (3,), unit world axis (3,))} of `env`'s robot at one joint state: one ops.urdf_fk call."""
    robot = env.robot
    table = robot.fk_table()
    _, lines = ops.urdf_fk(table, robot.q_rows([q_by_joint]), env.base, want_lines=True)
    lines = lines[0].cpu().numpy()
    return {name: (lines[i, :3], lines[i, 3:]) for i, name in enumerate(table["names"])}


def compare_joints(joint_map=None, pred_urdf_path=None, gt_urdf_path=None, offset=None, sim_ori=None, pred_ori=None,
                   dof=None, global_scale=1.0):
    """Per-joint position / direction error of the predicted URDF against the ground truth (evaluation.py:84-224).
    Revolute joints in file order, the first ``dof`` of each robot; the predicted robot at zero, the ground truth with its
    driven joints at ``offset`` and every other joint at 0; predicted revolute joint ``joint_map[i]`` against ground-truth
    revolute joint ``i``.  A direction error above 90 degrees becomes 180 - e with ``dir_map`` -1.
    ``global_scale`` scales the predicted robot (the reference's module global).
    Returns (pos_error_list, dir_error_list, dir_map)."""
    from .sim_data import SimEnv
    joint_map = np.asarray(joint_map).astype(np.int64).reshape(-1)
    zero = [0, 0, 0]
    env_pred = SimEnv(pred_urdf_path, base_orientation=zero if pred_ori is None else pred_ori, dof=dof, global_scale=global_scale)
    env_gt = SimEnv(gt_urdf_path, base_orientation=zero if sim_ori is None else sim_ori, dof=dof)
    if len(env_pred.joint_list) < dof or len(env_gt.joint_list) < dof:
        raise ValueError(f"compare_joints: dof = {dof} but the predicted URDF has {len(env_pred.joint_list)} revolute joints "
                         f"and the ground truth {len(env_gt.joint_list)}")
    if len(joint_map) < dof or joint_map[:dof].min() < 0 or joint_map[:dof].max() >= len(env_pred.joint_list):
        raise ValueError(f"compare_joints: joint_map {joint_map.tolist()} does not index the predicted URDF's "
                         f"{len(env_pred.joint_list)} revolute joints for dof = {dof}")
    lines_pred = _joint_lines(env_pred, {})
    lines_gt = _joint_lines(env_gt, {name: float(offset[i]) for i, name in enumerate(env_gt.dof_list)})
    pos_error_list, dir_error_list, dir_map = [], [], []
    for i in range(dof):
        pred_pos, pred_uv = lines_pred[env_pred.joint_list[joint_map[i]]]
        gt_pos, gt_uv = lines_gt[env_gt.joint_list[i]]
        pos_error, dir_error = joint_error(pred_pos, pred_uv, gt_pos, gt_uv)
        if dir_error > 90:
            dir_error = 180 - dir_error
            dir_map.append(-1)
        else:
            dir_map.append(1)
        pos_error_list.append(pos_error)
        dir_error_list.append(dir_error)
    return pos_error_list, dir_error_list, dir_map


# ------------------------------------------------------------------------------------------ posed clouds
def _collect(env, commands, data_path, pix, num_points):
    """One cloud per command row: all rows posed by one ops.urdf_fk launch, handed to data_collection as device poses."""
    from .sim_data import data_collection
    robot = env.robot
    q = robot.q_rows([env.set_joint_positions(cmd) for cmd in commands])
    link_T = ops.urdf_fk(robot.fk_table(), q, env.base)
    _, record = data_collection(env=env, data_path=data_path, width=pix, height=pix, visualize=False, angle_list=commands,
                                num_points=num_points, link_T=link_T)
    return record


def evaluation(pred_urdf_path=None, gt_urdf_path=None, pix=800, dof=5, radius=1.5, num_cameras=20, gui=True,
               visualize=True, visualize_result=True, save_path=None, offset=None, sim_ori=None, pred_ori=None,
               joint_map=None, direction_map=None, num_points=10000, num_poses=3, global_scale=1.0):
    """evaluation.py:228-380: ``num_poses`` random commands in [-1, 1) rad; the ground truth is driven at command + offset,
    the predicted robot at the commands mapped by ``map_commands``; ``num_points`` visible surface points of each
    (``pred/{i:04}/robot.ply``, ``gt/{i:04}/robot.ply``); per pair ``icp_filter`` then ``torch_chamfer_distance``.
    Writes command_rad.txt, command_deg.txt, loss.txt and loss_mean_std.txt under ``save_path`` and returns the losses.
    The draws keep the reference's order on numpy's global state: the commands, then the predicted robot's camera ring
    (20 or more cameras), then the ground truth's.  gui / visualize / visualize_result must be falsy."""
    if gui or visualize or visualize_result:
        raise NotImplementedError("gui / visualize / visualize_result need PyBullet's and Open3D's viewers (out of scope)")
    from .sim_data import SimEnv
    os.makedirs(save_path + 'pred/', exist_ok=True)
    os.makedirs(save_path + 'gt/', exist_ok=True)

    a_list = np.random.rand(num_poses, dof) * 2 - 1
    deg_list = np.degrees(a_list)
    np.savetxt(save_path + 'command_rad.txt', a_list)
    np.savetxt(save_path + 'command_deg.txt', deg_list)

    a_list_mapped = map_commands(a_list, joint_map, direction_map)
    print(np.array(direction_map))
    a_list_offset = a_list + np.asarray(offset, np.float64)

    env_pred = SimEnv(urdf_path=pred_urdf_path, gui=gui, dof=dof, radius=radius, num_cameras=num_cameras,
                      global_scale=global_scale, base_orientation=[0, 0, 0] if pred_ori is None else pred_ori)
    pred_list = _collect(env_pred, a_list_mapped, save_path + 'pred/', pix, num_points)
    env_pred.reset()

    env_gt = SimEnv(urdf_path=gt_urdf_path, gui=gui, dof=dof, radius=radius, num_cameras=num_cameras,
                    base_orientation=[0, 0, 0] if sim_ori is None else sim_ori)
    gt_list = _collect(env_gt, a_list_offset, save_path + 'gt/', pix, num_points)
    env_gt.reset()

    loss_record = []
    for pred_pcd, gt_pcd in zip(pred_list, gt_list):
        _, moved = icp_filter(pred_pcd, gt_pcd, threshold=0.01, max_iteration=20000)
        loss = torch_chamfer_distance(moved, gt_pcd)
        print(loss)
        loss_record.append(loss)
    np.savetxt(save_path + 'loss.txt', loss_record)
    np.savetxt(save_path + 'loss_mean_std.txt', (np.mean(loss_record), np.std(loss_record)))
    return loss_record


def main(argv=None):
    """python -m autourdf_amd.evaluation --robot wx200_5 [...]: the reference's flags (evaluation.py:383-449) minus the viewer
    ones, plus --global_scale / --num_poses / --num_points / --joint_map; run from the directory that holds
    parameters.json and data/."""
    import argparse
    import json
    ap = argparse.ArgumentParser(description="Score data/urdf/{robot}_{K}_seg/{step}_deg_{cams}_cams.urdf against the robot's "
                                             "ground-truth URDF: joint errors and posed-cloud Chamfer loss.")
    ap.add_argument('--robot', type=str, default='bolt')
    ap.add_argument('--pix', type=int, default=800)
    ap.add_argument('--num_cameras', type=int, default=20, help="names the raw-data and URDF files")
    ap.add_argument('--num_cameras_eval', type=int, default=20, help="fewer than 20: a fixed ring; 20 or more: a random one")
    ap.add_argument('--step_size', type=int, default=4)
    ap.add_argument('--global_scale', type=float, default=1.0, help="scale of the predicted URDF (the reference's GOBAL_SCALE)")
    ap.add_argument('--num_poses', type=int, default=3)
    ap.add_argument('--num_points', type=int, default=10000)
    ap.add_argument('--joint_map', type=str, default=None, help="default Sim/joint_map/{robot}.txt; the identity if absent")
    args = ap.parse_args(argv)
    np.random.seed(2024)
    with open('parameters.json') as f:
        robot_params = json.load(f)[args.robot]
    missing = [k for k in ('num_seg', 'dof', 'gt', 'ori', 'sim_ori', 'cam_dist') if k not in robot_params]
    if missing:
        raise SystemExit(f"parameters.json lacks {missing} for {args.robot!r} (use the reference's parameters.json)")
    num_seg, dof = robot_params['num_seg'], robot_params['dof']
    tag = f'{args.step_size}_deg_{args.num_cameras}_cams'
    offset = load_offset(f'data/raw/{args.robot}/{tag}/')
    sim_ori, pred_ori = robot_params['sim_ori'], robot_params['ori']
    map_path = args.joint_map or f'Sim/joint_map/{args.robot}.txt'
    if os.path.exists(map_path):
        joint_map = np.loadtxt(map_path, dtype=int).reshape(-1)
    elif args.joint_map:
        raise SystemExit(f"--joint_map {map_path}: no such file")
    else:
        joint_map = np.arange(dof)
        print(f"{map_path} not found: using the identity joint map")
    pred_urdf = f'data/urdf/{args.robot}_{num_seg}_seg/{tag}.urdf'
    pos_error_list, dir_error_list, dir_map = compare_joints(
        joint_map=joint_map, pred_urdf_path=pred_urdf, gt_urdf_path=robot_params['gt'], offset=offset, sim_ori=sim_ori,
        pred_ori=pred_ori, dof=dof, global_scale=args.global_scale)
    print(f"Position error: {pos_error_list}")
    print(f"Direction error: {dir_error_list}")
    save_path = f'data/evaluation2/{args.robot}_{num_seg}_seg/{tag}/'
    evaluation(pred_urdf_path=pred_urdf, gt_urdf_path=robot_params['gt'], pix=args.pix, radius=robot_params['cam_dist'],
               dof=dof, num_cameras=args.num_cameras_eval, gui=False, visualize=False, visualize_result=False,
               save_path=save_path, offset=offset, sim_ori=sim_ori, pred_ori=pred_ori, joint_map=joint_map,
               direction_map=dir_map, num_points=args.num_points, num_poses=args.num_poses, global_scale=args.global_scale)
    np.savetxt(save_path + 'pos_mean_std.txt', (np.mean(pos_error_list), np.std(pos_error_list)))
    np.savetxt(save_path + 'dir_mean_std.txt', (np.mean(dir_error_list), np.std(dir_error_list)))


if __name__ == "__main__":
    main()
