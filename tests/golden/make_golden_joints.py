"""Mint tests/golden/joints_reference.npz (run in the BUILD CONTAINER only).

    python tests/golden/make_golden_joints.py

Source of truth: the reference's own ``estimate_joint_axes_from_tree`` and ``create_urdf`` (PointCloud/compute_joints.py)
and ``CoordMap.cluster_to_link`` (PointCloud/coord_map.py).  The reference's coord_map is imported exactly as
make_golden_coord_map.py does it (ref_shims + roma + empty GUI / joint / link modules); compute_joints.py is then loaded
under its own module name with three more stubs: transforms3d (``axangles.aff2axangle`` restated in tests/_joints_ref.py
from the published library -- a restatement, like the pytorch3d arithmetic of ref_shims), pybullet and pybullet_data
(only visualize_urdf touches them).  matplotlib is used as installed for the link colours.

Cases a, b, c are those of urdf_reference.npz (same seeded robots, same links and tree, recomputed here through the
reference).  Recorded: the coords the reference read (S,T,K,7), its joint_data for estimate_joint_axes_from_tree(links,
cms, 0, T, 4), its URDF text (mesh_dir "mesh/dir"), and for case a the link matrices and clouds of cluster_to_link on
small seeded float32 per-cluster clouds whose sizes vary per frame.  The reference's CPU wall time for the joint step
is kept as data: it was taken on the fixture's build machine, not on the GPU machine.
"""
import contextlib
import importlib.util
import io
import os
import sys
import tempfile
import time
import types

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(HERE))
import make_golden_urdf as mu  # noqa: E402  (installs ref_shims and the coord_map stubs, imports the reference)
import _joints_ref  # noqa: E402

ref_cm = mu.ref_cm
REF = "/root/reference/PointCloud"

t3d = types.ModuleType("transforms3d")
t3d.axangles = types.SimpleNamespace(aff2axangle=_joints_ref.aff2axangle, mat2axangle=_joints_ref.mat2axangle)
sys.modules["transforms3d"] = t3d
sys.modules["pybullet"] = types.ModuleType("pybullet")
pbd = types.ModuleType("pybullet_data")
pbd.getDataPath = lambda: ""
sys.modules["pybullet_data"] = pbd
spec = importlib.util.spec_from_file_location("ref_compute_joints", os.path.join(REF, "compute_joints.py"))
ref_cj = importlib.util.module_from_spec(spec)
spec.loader.exec_module(ref_cj)

MESH_DIR = "mesh/dir"


def clouds(T, K, seed):
    rng = np.random.default_rng(seed)
    return [{str(k): rng.normal(scale=0.02, size=(int(rng.integers(2, 9)), 3)).astype(np.float32) for k in range(K)}
            for _ in range(T)]


def main():
    import torch
    from oracle import transforms
    out = {}
    cases = (("a", [-1, 0, 1, 2, 3, 4], 20, 2, 10, 0, 0.0, True),
             ("b", [-1, 0, 1, 1, 1, 2, 3, 4], 30, 1, 12, 1, 0.0, False),
             ("c", [-1, 0, 1, 2, 3, 4], 20, 2, 10, 0, 1e-3, True))
    urdf_g = np.load(os.path.join(HERE, "urdf_reference.npz"))
    for tag, parents, K, S, T, seed, noise, unknown in cases:
        M, link_of, axes, pos = mu.robot_sequences(parents, K, S, T, seed, noise)
        assert np.array_equal(M, urdf_g[f"{tag}.matrices"])
        sums, cms = [], []
        for s in range(S):
            cm = ref_cm.CoordMap.__new__(ref_cm.CoordMap)
            cm.matrices = M[s]
            q = transforms.matrix_to_quaternion(torch.from_numpy(M[s, :, :, :3, :3])).numpy()
            cm.coords = np.concatenate([M[s, :, :, :3, 3], q], axis=-1)
            cm.num_coords, cm.bounding_box = K, 0.9
            cm.clusters = clouds(T, K, 100 + 10 * seed + s)
            sums.append(cm.coord_dist_map(diff=True)[1])
            cms.append(cm)
        sum_map = np.mean(sums, axis=0)
        sum_map = (sum_map - np.min(sum_map)) / (np.max(sum_map) - np.min(sum_map))
        with contextlib.redirect_stdout(io.StringIO()):
            if unknown:
                cluster_idx, g1, _, _ = ref_cm.silhouette_score_method(K, sum_map, link_range=(4, min(25, K)))
            else:
                cluster_idx, g1, _ = ref_cm.coord_clustering(K, sum_map, num_links=len(parents))
            links = cms[0].kinematics_tree(cms[0].coord_mst(), g1)
            t0 = time.perf_counter()
            joint_data = ref_cj.estimate_joint_axes_from_tree(links, cms, 0, T, 4)
            wall = time.perf_counter() - t0
        assert [l["id"] for l in links] == urdf_g[f"{tag}.link_id"].tolist()
        assert [x for l in links for x in l["cluster_idx"]] == urdf_g[f"{tag}.link_cluster_idx"].tolist()
        with tempfile.TemporaryDirectory() as d:
            path = os.path.join(d, "urdf", "robot.urdf")
            with contextlib.redirect_stdout(io.StringIO()):
                ref_cj.create_urdf(links, joint_data, cms[0], path, MESH_DIR)
            with open(path, "rb") as f:
                urdf = f.read()
        out[f"{tag}.coords"] = np.stack([cm.coords for cm in cms])                 # (S,T,K,7), what the reference read
        out[f"{tag}.link_id"] = np.array([l["id"] for l in links])
        out[f"{tag}.link_parent_id"] = np.array([-1 if l["parent_id"] is None else l["parent_id"] for l in links])
        out[f"{tag}.link_cluster_idx"] = np.array([x for l in links for x in l["cluster_idx"]])
        out[f"{tag}.link_cluster_sizes"] = np.array([len(l["cluster_idx"]) for l in links])
        out[f"{tag}.joint_parent"] = np.array([j["parent_link"] for j in joint_data])
        out[f"{tag}.joint_child"] = np.array([j["child_link"] for j in joint_data])
        for key in ("local_axis", "local_pos", "global_pos", "global_axis"):
            out[f"{tag}.{key}"] = np.array([np.asarray(j[key], np.float64) for j in joint_data])
        out[f"{tag}.urdf"] = np.frombuffer(urdf, np.uint8)
        out[f"{tag}.mesh_dir"] = np.array(MESH_DIR)
        out[f"{tag}.ref_joint_wall_s"] = np.float64(wall)                          # reference CPU, build machine
        if tag == "a":
            cm = cms[0]
            mesh_links = cm.cluster_to_link(cluster_idx)
            out["a.c2l_cluster_idx"] = np.array([x for c in cluster_idx for x in c])
            out["a.c2l_cluster_sizes"] = np.array([len(c) for c in cluster_idx])
            sizes = np.array([[len(cm.clusters[t][str(k)]) for k in range(K)] for t in range(T)])
            out["a.c2l_point_sizes"] = sizes                                        # (T,K)
            out["a.c2l_points"] = np.concatenate([cm.clusters[t][str(k)] for t in range(T) for k in range(K)])
            out["a.c2l_matrices"] = np.stack([ml["matrices"] for ml in mesh_links])   # (L,T,4,4) float32
            out["a.c2l_lf"] = np.concatenate([c for ml in mesh_links for c in ml["clusters"]])      # link-major, then t
            out["a.c2l_wf"] = np.concatenate([c for ml in mesh_links for c in ml["clusters_wf"]])
            out["a.c2l_sizes"] = np.array([[len(c) for c in ml["clusters"]] for ml in mesh_links])  # (L,T)
        print(tag, "joints", len(joint_data), f"reference joint step {wall * 1e3:.1f} ms")
    path = os.path.join(HERE, "joints_reference.npz")
    np.savez_compressed(path, **out)
    print(f"joints_reference.npz {os.path.getsize(path) / 1024:.1f} KB")


if __name__ == "__main__":
    main()
