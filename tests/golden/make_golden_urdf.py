"""Mint tests/golden/urdf_reference.npz (run in the BUILD CONTAINER only).

    python tests/golden/make_golden_urdf.py

Source of truth: the reference's own ``coord_clustering``, ``silhouette_score_method``, ``CoordMap.coord_mst`` and
``CoordMap.kinematics_tree`` (PointCloud/coord_map.py) with the real networkx and scikit-learn, imported under the
same stubs as make_golden_coord_map.py (ref_shims + roma restated by the oracle; the GUI / joint / link modules the
file imports at its top are never called here).  Inputs are seeded pose sequences with known kinematics: clusters
rigidly attached to the links of a revolute tree, R = I at frame 0 at the cluster centroids (as Segments produces),
joint steps of 4 deg * (1 + U), frames >= 1 rounded to float32 (as match() writes them).

Cases: (a) serial 6-link chain, K = 20, S = 2 sequences, T = 10, link count searched (--unknown_dof);
(b) a branched hand-like tree (palm + 3 two-link fingers + base), K = 30, S = 1, T = 12, known dof;
(c) case (a) with 1e-3 pose noise, so the silhouettes are non-trivial.
Fixture = inputs (poses) + the reference's outputs only.
"""
import contextlib
import io
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import make_golden_coord_map as mg  # noqa: E402  (installs ref_shims + the roma / GUI stubs, imports the reference)
from scipy.spatial.transform import Rotation  # noqa: E402

ref_cm = mg.ref_cm


def rodrigues(axis, ang):
    return Rotation.from_rotvec(np.asarray(axis) * ang).as_matrix()


def robot_sequences(parents, K, S, T, seed, noise=0.0):
    """Poses (S,T,K,4,4) of K clusters on the links of a revolute tree (parents[l] = parent link, -1 for the base),
    with the true link of every cluster, joint axes (world, frame 0) and joint points."""
    rng = np.random.default_rng(seed)
    L = len(parents)
    pos = np.zeros((L, 3))
    for l in range(1, L):
        pos[l] = pos[parents[l]] + rng.uniform(-1, 1, 3) * np.array([0.06, 0.06, 0.02]) + np.array([0, 0, 0.12])
    axes = rng.normal(size=(L, 3))
    axes /= np.linalg.norm(axes, axis=1, keepdims=True)
    link_of = np.concatenate([np.arange(L), rng.integers(0, L, K - L)])
    rng.shuffle(link_of)
    cent = np.array([pos[l] + rng.uniform(-0.05, 0.05, 3) + np.array([0, 0, 0.05]) for l in link_of])
    out = np.zeros((S, T, K, 4, 4))
    for s in range(S):
        ang = np.zeros(L)
        sign = rng.choice([-1.0, 1.0], L)
        for t in range(T):
            if t:
                ang += sign * np.deg2rad(4.0) * (1 + rng.uniform(size=L))
            W = [None] * L                                             # link motion relative to frame 0
            for l in range(L):
                if parents[l] < 0:
                    W[l] = np.eye(4)
                    continue
                J = np.eye(4)
                J[:3, :3] = rodrigues(axes[l], ang[l])
                J[:3, 3] = pos[l] - J[:3, :3] @ pos[l]
                W[l] = W[parents[l]] @ J
            for k in range(K):
                M = np.eye(4)
                M[:3, 3] = cent[k]
                M = W[link_of[k]] @ M
                if noise and t:
                    M[:3, :3] = rodrigues(rng.normal(size=3), noise) @ M[:3, :3]
                    M[:3, 3] += rng.normal(scale=noise, size=3)
                out[s, t, k] = M
    out[:, 1:] = out[:, 1:].astype(np.float32).astype(np.float64)
    return out, link_of, axes, pos


def main():
    import torch
    from oracle import transforms
    out = {}
    cases = (("a", [-1, 0, 1, 2, 3, 4], 20, 2, 10, 0, 0.0, True),
             ("b", [-1, 0, 1, 1, 1, 2, 3, 4], 30, 1, 12, 1, 0.0, False),
             ("c", [-1, 0, 1, 2, 3, 4], 20, 2, 10, 0, 1e-3, True))
    for tag, parents, K, S, T, seed, noise, unknown in cases:
        M, link_of, axes, pos = robot_sequences(parents, K, S, T, seed, noise)
        bbox = 0.9
        sums, cms = [], []
        for s in range(S):
            cm = ref_cm.CoordMap.__new__(ref_cm.CoordMap)
            cm.matrices = M[s]
            q = transforms.matrix_to_quaternion(torch.from_numpy(M[s, :, :, :3, :3])).numpy()
            cm.coords = np.concatenate([M[s, :, :, :3, 3], q], axis=-1)          # load_matrix's (T,K,7)
            cm.num_coords, cm.bounding_box = K, bbox
            sums.append(cm.coord_dist_map(diff=True)[1])
            cms.append(cm)
        sum_map = np.mean(sums, axis=0)
        sum_map = (sum_map - np.min(sum_map)) / (np.max(sum_map) - np.min(sum_map))
        lo, hi = 4, min(25, K)
        thr, labels, scores, ncomp = [], [], [], []
        for nl in range(lo, hi):
            buf = io.StringIO()
            with contextlib.redirect_stdout(buf):
                try:
                    cidx, _, sc = ref_cm.coord_clustering(K, sum_map, nl)
                except ValueError:
                    cidx, sc = None, np.nan
            printed = [ln for ln in buf.getvalue().splitlines() if ln.startswith("Threshold:")]
            thr.append(float(printed[-1].split()[-1]) if printed else np.nan)
            lab = np.full(K, -1)
            for i, c in enumerate(cidx or []):
                lab[list(c)] = i
            labels.append(lab)
            ncomp.append(len(cidx) if cidx else -1)
            scores.append(sc)
        with contextlib.redirect_stdout(io.StringIO()):
            if unknown:
                cluster_idx, g1, _, nls = ref_cm.silhouette_score_method(K, sum_map, link_range=(lo, hi))
            else:
                cluster_idx, g1, _ = ref_cm.coord_clustering(K, sum_map, num_links=len(parents))
            g0 = cms[0].coord_mst()
            links = cms[0].kinematics_tree(g0, g1)
        out[f"{tag}.matrices"] = M
        out[f"{tag}.bounding_box"] = np.float64(bbox)
        out[f"{tag}.link_of"] = link_of
        out[f"{tag}.parents"] = np.array(parents)
        out[f"{tag}.axes"], out[f"{tag}.joint_pos"] = axes, pos
        out[f"{tag}.unknown_dof"] = np.int64(unknown)
        out[f"{tag}.coords0"] = cms[0].coords                           # what coord_mst / kinematics_tree read
        out[f"{tag}.sum_map"] = sum_map
        out[f"{tag}.nl_range"] = np.array([lo, hi])
        out[f"{tag}.thr_printed"] = np.array(thr)                       # t - 1e-4 as the reference prints it
        out[f"{tag}.labels"] = np.array(labels)
        out[f"{tag}.n_comp"] = np.array(ncomp)
        out[f"{tag}.scores"] = np.array(scores, np.float64)
        out[f"{tag}.num_links"] = np.int64(len(cluster_idx))
        out[f"{tag}.cluster_idx"] = np.array([x for c in cluster_idx for x in c])
        out[f"{tag}.cluster_sizes"] = np.array([len(c) for c in cluster_idx])
        out[f"{tag}.g1_edges"] = np.array(list(g1.edges), np.int64).reshape(-1, 2)
        out[f"{tag}.g0_edges"] = np.array(list(g0.edges), np.int64).reshape(-1, 2)
        out[f"{tag}.link_id"] = np.array([l["id"] for l in links])
        out[f"{tag}.link_tree_id"] = np.array([l["tree_id"] for l in links])
        out[f"{tag}.link_parent_id"] = np.array([-1 if l["parent_id"] is None else l["parent_id"] for l in links])
        out[f"{tag}.link_cluster_idx"] = np.array([x for l in links for x in l["cluster_idx"]])
        out[f"{tag}.link_connected"] = np.array([x for l in links for x in l["connected_links"]])
        out[f"{tag}.link_connected_sizes"] = np.array([len(l["connected_links"]) for l in links])
        print(tag, "num_links", len(cluster_idx), "scores", np.round(scores, 4), "tree", out[f"{tag}.link_parent_id"])
    path = os.path.join(HERE, "urdf_reference.npz")
    np.savez_compressed(path, **out)
    print(f"urdf_reference.npz {os.path.getsize(path) / 1024:.1f} KB")


if __name__ == "__main__":
    main()
