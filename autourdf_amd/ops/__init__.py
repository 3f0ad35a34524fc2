"""torch-facing wrappers over the C ABI: tensors in, tensors out, current CUDA(HIP) stream.

Only plumbing lives here (pointer extraction, output allocation, autograd glue); all arithmetic is
in libcreg.so.  Every function requires CUDA tensors and raises otherwise -- no CPU path exists.

One module per stage; `ops.<name>` reaches every stage's public names, as when this was one file.  A wrapper that calls another
(`kmeans_lloyd_each` -> `kmeans_lloyd_batch`) looks it up on its own stage's module: that is where a test replaces it.
"""
from ._common import _need, _p, _stream  # noqa: F401
from .chamfer import chamfer_distance, cluster_transform, nn_l1_bidir, pack_clusters  # noqa: F401
from .icp import (ICP_BATCH_MAX, aabb_mask, icp_nn_counters, icp_p2p, icp_p2p_batch, kabsch, masked_icp, masked_icp_batch,  # noqa: F401
                  masked_icp_each, masked_icp_regime)
from .mesh_query import (MESH_CONTAIN_MAX_POINTS, MESH_INERTIA_KEYS, POSE_FIT_MAX_D, _morton_order, joint_chains, link_moments,  # noqa: F401
                         mesh_clearance, mesh_collide, mesh_contain, mesh_inertia, point_mesh_distance, pose_fit_system, urdf_fk)
from .meshing import (HULL_MAX_COORD, HULL_STATUS, MESH_MAX_NEIGHBORS, lattice_hull, statistical_outlier, voxel_layout,  # noqa: F401
                      voxel_mesh)
from .pose_rows import (dq_invert, dq_multiply, dq_to_quat_trans, dq_to_se3, dq_to_se3_bwd, matrix_to_quat, quat_to_matrix,  # noqa: F401
                        quat_trans_to_dq, se3_to_dq)
from .segment import (GROUP_BATCH_MAX, KMEANS_BATCH_MAX, KMEANS_BATCH_MAX_K, KMEANS_BATCH_MAX_N, KMEANS_ND_MAX_K, KMEANS_ND_MAX_N,  # noqa: F401
                      group_to_local, group_to_local_batch, group_to_local_each, kmeans_assign, kmeans_lloyd, kmeans_lloyd_batch,
                      kmeans_lloyd_each, kmeans_lloyd_nd, knn_normals)
from .sim import depth_points, raster_depth, sample_mesh, segment_plane, visibility  # noqa: F401
from .train import DQ_PARAM_ORDER, Q_PARAM_ORDER, TRAIN_HIDDEN_TILES, TRAIN_ROT, TrainPlan  # noqa: F401
from .urdf_stage import (JOINT_MAX_SAMPLES, JOINT_THETA_MIN, LINK_SWEEP_MAX_K, coord_dist_map, coord_mst, joint_axes,  # noqa: F401
                         joint_axes_prepare, joint_positions, joint_samples, joint_slides, joint_types, link_clouds, link_clouds_bytes,
                         link_clouds_prepare, link_poses, link_sweep, motion_error, pose_coords)


#: public names added since this package was one file, and the stage that holds each.  They are looked up when first asked for
#: (`ops.mesh_cover`, `from autourdf_amd.ops import mesh_cover`), so the module's own namespace stays the one-file surface that
#: tests/test_host_cpu.py lists name by name; a test that replaces one does so on the stage's module or on the caller's `ops`.
_LATER = {"mesh_cover": "mesh_query"}


def __getattr__(name):
    if name in _LATER:
        from importlib import import_module
        return getattr(import_module("." + _LATER[name], __name__), name)
    raise AttributeError(f"module {__name__!r} has no attribute {name!r}")


def __dir__():
    return sorted(list(globals()) + list(_LATER))
