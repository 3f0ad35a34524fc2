"""Drop-in for the data side of the reference's ``PointCloud/coord_map.py``: the ``CoordMap`` that
consumes ``match()``'s ``matrix/*.npy`` / ``cluster/*.npz`` output.

Same constructor, attributes and method signatures as the reference class (coord_map.py:130-332):
``coords`` (T,K,7), ``matrices`` (T,K,4,4), ``clusters``, ``num_coords``, ``scale``, ``bounding_box``;
``load_matrix``, ``load_cluster``, ``get_scale``, ``get_bounding_box``, ``coord_dist_map(diff=True)``,
``coord_dist_map_legacy``.  The O(T K^2)/O(T K^3) Python loops with per-element torch / roma calls
(:250-301) are one launch of ``creg_coord_dist_map_f64``; the pose -> quaternion loop of
``load_matrix`` (:204-219) one launch of ``creg_pose_coords_f64``.  Everything is evaluated in fp64
(the reference's arrays are float64 whenever frame 0 -- saved as float64, mlp_reg.py:257-263 -- is in
the range; an all-float32 range is promoted, which only removes the reference's own float32 rounding).

The graph half of the URDF stage is here too: ``coord_clustering`` / ``silhouette_score_method``
(coord_map.py:70-128; every candidate link count in ONE launch of ``creg_link_sweep_f64``), ``CoordMap.coord_mst``
(:334-349, ``creg_coord_mst_f64``) and ``CoordMap.kinematics_tree`` (:351-441, host bookkeeping over <= 25 links).
Graphs are ``Graph``, a minimal stand-in for the networkx.Graph surface the reference uses (``nodes``, ``edges``,
``neighbors(n)``, insertion-ordered adjacency), and ``connected_components`` walks it exactly as networkx does, so
the component sets are built in the same insertion order and iterate identically.  ``CoordMap.cluster_to_link``
(:443-502) is one launch of ``creg_link_clouds_f64``; joint axes and the URDF writer are in compute_joints.py.  ``main``
is the headless part of the reference's command line (:641-792).  The GUI of the reference file is not part of this
module.
There is no CPU fallback: the methods need the HIP library and a GPU.
"""
import glob

import numpy as np
import torch

from . import _lib, ops
from .cluster_icp import read_point_cloud

THRESHOLD_STEP = 0.0001                     # the reference's lattice decrement (coord_map.py:94)


class Graph:
    """The part of networkx.Graph the URDF stage touches, with networkx's insertion-ordered adjacency, so that
    ``edges`` and ``connected_components`` iterate in networkx's order (as cluster_icp.PointCloud stands in for Open3D)."""

    def __init__(self):
        self._adj = {}

    def add_nodes_from(self, nodes):
        for n in nodes:
            self._adj.setdefault(n, {})

    def add_edge(self, u, v):
        self._adj.setdefault(u, {})
        self._adj.setdefault(v, {})
        self._adj[u][v] = self._adj[v][u] = {}

    def add_edges_from(self, edges):
        for u, v in edges:
            self.add_edge(u, v)

    @property
    def nodes(self):
        return list(self._adj)

    @property
    def edges(self):
        """networkx's EdgeView order: nodes in insertion order, each node's unseen neighbours in insertion order."""
        seen, out = set(), []
        for n, nbrs in self._adj.items():
            out.extend((n, m) for m in nbrs if m not in seen)
            seen.add(n)
        return out

    def neighbors(self, n):
        return iter(self._adj[n])

    def number_of_nodes(self):
        return len(self._adj)

    def number_of_edges(self):
        return len(self.edges)

    def __len__(self):
        return len(self._adj)

    def __iter__(self):
        return iter(self._adj)

    def __contains__(self, n):
        return n in self._adj


def connected_components(G):
    """networkx.connected_components: sets built by the same level-order BFS (same insertion order), yielded in
    node order."""
    seen, n = set(), len(G)
    for v in G:
        if v in seen:
            continue
        comp, nextlevel = {v}, [v]
        while nextlevel and len(comp) < n:
            thislevel, nextlevel = nextlevel, []
            for u in thislevel:
                for w in G._adj[u]:
                    if w not in comp:
                        comp.add(w)
                        nextlevel.append(w)
                if len(comp) == n:
                    break
        seen.update(comp)
        yield comp


def _check_map(num_coords, d_map):
    d = np.asarray(d_map.cpu().numpy() if isinstance(d_map, torch.Tensor) else d_map, dtype=np.float64)
    if d.shape != (num_coords, num_coords):
        raise ValueError(f"d_map must be ({num_coords},{num_coords}), got {d.shape}")
    if not np.all(np.isfinite(d)):
        raise ValueError("d_map contains NaN or infinity")            # sklearn's check_array
    if num_coords > ops.LINK_SWEEP_MAX_K:
        raise ValueError(f"link discovery supports at most {ops.LINK_SWEEP_MAX_K} clusters, got {num_coords}")
    return d


def _threshold_graph(num_coords, d, threshold):
    """G1 of coord_clustering: every node, the edges (i, j), i < j, d[i, j] < threshold in the reference's loop order."""
    G = Graph()
    G.add_nodes_from(range(num_coords))
    ii, jj = np.nonzero(np.triu(d < threshold, 1))
    G.add_edges_from(zip(ii.tolist(), jj.tolist()))
    return G


def _sweep(num_coords, d_map, lo, hi):
    d = _check_map(num_coords, d_map)
    labels, n_comp, thr, scores, best = ops.link_sweep(torch.as_tensor(d, device=_lib.device(d_map)), lo, hi)
    best, n_comp = int(best.item()), n_comp.cpu().numpy()
    if best < 0:
        bad = [lo + i for i, c in enumerate(n_comp) if not 1 < c < num_coords]
        raise ValueError(f"Number of labels is invalid for link counts {bad} (component counts "
                         f"{[int(n_comp[b - lo]) for b in bad]}); valid values are 2 to n_samples - 1 (inclusive)")
    return d, labels.cpu().numpy(), n_comp, thr.cpu().numpy(), scores.cpu().numpy(), best


def _clusters_at(num_coords, d, threshold, labels):
    G1 = _threshold_graph(num_coords, d, threshold)
    cluster_idx = list(connected_components(G1))
    host = np.empty(num_coords, np.int64)
    for cid, c in enumerate(cluster_idx):
        host[list(c)] = cid
    if not np.array_equal(host, labels):
        raise RuntimeError("creg_link_sweep_f64 components disagree with the threshold graph")
    return cluster_idx, G1


def coord_clustering(num_coords, d_map, num_links):
    """Cluster the coordinates based on the distance variance matrix (reference coord_map.py:70-111): the connected
    components of {d < t} at the first lattice threshold with >= num_links of them, and their silhouette score."""
    d, labels, _, thr, scores, _ = _sweep(num_coords, d_map, num_links, num_links + 1)
    print("Threshold: ", thr[0] - THRESHOLD_STEP)
    cluster_idx, G1 = _clusters_at(num_coords, d, thr[0], labels[0])
    silhouette_avg = np.float64(scores[0])
    print(f"n={num_links}, silhouette score:{silhouette_avg}")
    return cluster_idx, G1, silhouette_avg


def silhouette_score_method(num_coords, d_map, link_range=(3, 15)):
    """Silhouette Score Method (reference coord_map.py:114-128): every link count of the range in one launch."""
    nls = np.arange(link_range[0], link_range[1])
    d, labels, _, thr, scores, best = _sweep(num_coords, d_map, int(nls[0]), int(nls[-1]) + 1)
    s_score = [np.float64(s) for s in scores]
    for nl, t, s in zip(nls, thr, s_score):
        print("Threshold: ", t - THRESHOLD_STEP)
        print(f"n={nl}, silhouette score:{s}")
    cluster_idx, g1 = _clusters_at(num_coords, d, thr[best], labels[best])
    return cluster_idx, g1, s_score, nls


class CoordMap:
    """Coordinate correlation map (reference coord_map.py:130-150)."""

    def __init__(self, data_path, raw_path, gt_data=False, start_steps=0, end_steps=0):
        self.data_path = data_path
        self.gt_data = gt_data
        self.start_steps = start_steps
        self.end_steps = end_steps
        self.coords, self.matrices = self.load_matrix(start_steps, end_steps)
        self.clusters = self.load_cluster(start_steps, end_steps)
        self.num_coords = self.coords.shape[1]
        self.scale = self.get_scale()
        self.bounding_box = self.get_bounding_box(raw_path)

    @classmethod
    def from_arrays(cls, matrices, bounding_box, clusters=None):
        """Poses already in memory ((T,K,4,4) array or device tensor): no file round trip."""
        self = cls.__new__(cls)
        self.data_path, self.gt_data, self.start_steps, self.end_steps = None, False, 0, 0
        self._M = torch.as_tensor(matrices, dtype=torch.float64).to(_lib.device(matrices)).contiguous()
        self.matrices = self._M.cpu().numpy()
        self.coords = ops.pose_coords(self._M).cpu().numpy()
        self.clusters = clusters if clusters is not None else []
        self.num_coords = self.coords.shape[1]
        self.scale = self.get_scale()
        self.bounding_box = float(bounding_box)
        return self

    # ---- loading (coord_map.py:185-228) -------------------------------------------------------------
    def load_matrix(self, start_steps=0, end_steps=0):
        files = sorted(glob.glob(self.data_path + 'matrix/*.npy'))[start_steps:end_steps]
        if not files:
            raise FileNotFoundError(f"no matrix/*.npy under {self.data_path} in [{start_steps}:{end_steps}]")
        matrices = np.array([np.load(f) for f in files])           # (T,K,4,4); float64 as soon as one file is
        self._M = torch.as_tensor(matrices, dtype=torch.float64).to(_lib.device()).contiguous()
        coords = ops.pose_coords(self._M).cpu().numpy().astype(matrices.dtype, copy=False)
        return coords, matrices

    def load_cluster(self, start_steps=0, end_steps=0):
        files = sorted(glob.glob(self.data_path + 'cluster/*.npz'))[start_steps:end_steps]
        return [np.load(f) for f in files]

    def get_scale(self):
        return float(max(np.max(self.coords[0, :, i]) - np.min(self.coords[0, :, i]) for i in range(3)))

    def get_bounding_box(self, raw_path):
        """Diagonal of the AABB of every raw frame of the sequence (coord_map.py:153-173)."""
        lo, hi = np.full(3, np.inf), np.full(3, -np.inf)
        for path in sorted(glob.glob(str(raw_path) + '*/')):
            pts = np.asarray(read_point_cloud(path + 'robot.ply').points)
            if len(pts):
                lo, hi = np.minimum(lo, pts.min(0)), np.maximum(hi, pts.max(0))
        if not np.all(np.isfinite(lo)):
            raise FileNotFoundError(f"no */robot.ply under {raw_path}")
        return float(np.linalg.norm(hi - lo))

    # ---- the maps (coord_map.py:230-332) ------------------------------------------------------------
    def coord_dist_map(self, diff=True):
        """num_seg x num_seg x time-step matrix and its sum over time, numpy arrays like the reference."""
        d_map, s_map = ops.coord_dist_map(self._M, self.bounding_box, diff)
        return d_map.cpu().numpy(), s_map.cpu().numpy()

    def coord_dist_map_legacy(self, diff=True):
        """xyz relative to step 0 + remaining pose coordinates, Euclidean distance matrices per step
        (coord_map.py:309-332); `diff` is ignored there too.  Two cdist calls per step on the device."""
        c = torch.as_tensor(np.asarray(self.coords, np.float64), device=_lib.device(getattr(self, "_M", None)))
        xyz = c[:, :, :3] - c[:1, :, :3]
        mode = "donot_use_mm_for_euclid_dist"          # exact differences, not the |a|^2 + |b|^2 - 2ab expansion
        rest = c[:, :, 3:].contiguous()
        d = torch.cdist(xyz, xyz, compute_mode=mode) + torch.cdist(rest, rest, compute_mode=mode)
        cmap = d.permute(1, 2, 0).contiguous()
        s = cmap.abs().sum(dim=2)
        s = (s - s.min()) / (s.max() - s.min())
        return cmap.cpu().numpy(), s.cpu().numpy()

    # ---- the graph half (coord_map.py:334-441) ------------------------------------------------------
    def coord_mst(self):
        """Minimum Spanning Tree of the T-summed cluster xyz (coord_map.py:334-349), as the reference's G_MST: nodes
        0..K-1, then the tree's edges in networkx's order (Kruskal's weight order, ties row-major, re-read through
        EdgeView).  The tree itself is one launch of creg_coord_mst_f64."""
        K = self.num_coords
        coords = torch.as_tensor(np.asarray(self.coords, np.float64), device=_lib.device(getattr(self, "_M", None)))
        edges, w = ops.coord_mst(coords.contiguous())
        e, w = edges.cpu().numpy(), w.cpu().numpy()
        kruskal = sorted(((float(wt), min(a, b), max(a, b)) for (a, b), wt in zip(e.tolist(), w)))
        mst = Graph()
        mst.add_nodes_from(range(K))
        mst.add_edges_from((a, b) for _, a, b in kruskal)
        G_MST = Graph()
        G_MST.add_nodes_from(range(K))
        G_MST.add_edges_from(mst.edges)
        return G_MST

    def kinematics_tree(self, g0, g1):
        """Build the kinematics tree based on the cluster_idx (coord_map.py:351-441): links, their neighbours in the
        base graph g0, the root (least movement), a BFS for parent_id / tree_id, links sorted by tree_id."""
        links = []
        cluster_idx = list(connected_components(g1))
        for link_id, idx in enumerate(cluster_idx):
            link = {'id': link_id, 'tree_id': None, 'cluster_idx': idx, 'connected_links': set()}
            for cid in idx:
                connected_cid = list(g0.neighbors(cid))
                for i in range(len(cluster_idx)):
                    if i == link_id:
                        continue
                    for ccid in connected_cid:
                        if ccid in cluster_idx[i] and i not in link['connected_links']:
                            link['connected_links'].add(i)
            links.append(link)

        link_graph = Graph()
        link_graph.add_nodes_from(range(len(links)))
        for link in links:
            for connected_link in link['connected_links']:
                link_graph.add_edge(link['id'], connected_link)
        n_cc = len(list(connected_components(link_graph)))
        if n_cc == 1 and link_graph.number_of_edges() == len(links) - n_cc:
            print("The graph is connected and Acyclic")
        else:
            print("The graph is not connected or Acyclic")

        for link in links:                                        # the root: least movement of the mean coordinates
            centers = np.mean(self.coords[:, list(link['cluster_idx']), :], axis=1)
            centers_diff = np.diff(centers, axis=0)
            link['movement'] = np.sum(np.linalg.norm(centers_diff, axis=1))

        links = sorted(links, key=lambda x: x['movement'])
        for link in links:
            print(link)
        root_link = links[0]
        root_link['parent_id'] = None
        root_link['tree_id'] = 0
        tree_id_counter = 1
        current_layer = [root_link]
        count = 0
        while True:
            count += 1
            child_link_id = set()
            next_layer = []
            for current_link in current_layer:
                if current_link['parent_id'] is not None:
                    child = current_link['connected_links'] - {current_link['parent_id']}
                else:
                    child = current_link['connected_links']
                for i in child:
                    for link in links:
                        if link['id'] == i:
                            link['parent_id'] = current_link['id']
                            link['tree_id'] = tree_id_counter
                            tree_id_counter += 1
                            next_layer.append(link)
                            break
                child_link_id.update(child)
            print(child_link_id)
            current_layer = next_layer
            if len(child_link_id) == 0 or count > 100:           # no child link, or the reference's dead-loop cap
                break

        links = sorted(links, key=lambda x: x['tree_id'])
        for i, link in enumerate(links):
            print(f'Layer{i} ---', 'Real ID: ', link['id'], 'Tree ID: ', link['tree_id'], 'Parent Link', link['parent_id'])
        return links

    # ---- link clouds (coord_map.py:443-502) ----------------------------------------------------------
    def cluster_to_link(self, cluster_idx):
        """Combine the clusters to links: one dict per link with 'matrices' (T,4,4) float32, 'clusters' (T arrays (n,3),
        link frame) and 'clusters_wf' (T arrays (n,3), world frame), every frame and link in one launch of
        creg_link_clouds_f64."""
        T, K = self.coords.shape[:2]
        dev = _lib.device(getattr(self, "_M", None))
        M = getattr(self, "_M", None)
        if M is None:
            M = torch.as_tensor(np.asarray(self.matrices, np.float64))
        M = M.to(dev).contiguous()
        idx = [list(c) for c in cluster_idx]
        used = {int(k) for c in idx for k in c}
        clouds, sizes = [], np.zeros(T * K, np.int64)
        for t in range(T):
            for k in range(K):
                if k not in used:                                 # never read, as in the reference
                    continue
                c = np.asarray(self.clusters[t][str(k)], np.float64).reshape(-1, 3)    # KeyError when missing
                clouds.append(c)
                sizes[t * K + k] = len(c)
        pts = torch.as_tensor(np.concatenate(clouds) if clouds else np.zeros((0, 3)), device=dev).contiguous()
        coords = torch.as_tensor(np.asarray(self.coords, np.float64), device=dev).contiguous()
        lm, _, wf, lf, oo = ops.link_clouds(coords, M, idx, pts, np.concatenate([[0], np.cumsum(sizes)]))
        lm, wf, lf = lm.cpu().numpy(), wf.cpu().numpy(), lf.cpu().numpy()
        L = len(idx)
        return [{'matrices': lm[:, l],
                 'clusters': [lf[oo[t * L + l]:oo[t * L + l + 1]] for t in range(T)],
                 'clusters_wf': [wf[oo[t * L + l]:oo[t * L + l + 1]] for t in range(T)]} for l in range(L)]


def _parser():
    """The reference's flags (coord_map.py:738-751)."""
    import argparse
    parser = argparse.ArgumentParser()
    parser.add_argument('--robot', type=str, default='wx200_5')
    parser.add_argument('--xyz_r', type=float, default=0.5)
    parser.add_argument('--start_steps', type=int, default=0)
    parser.add_argument('--end_steps', type=int, default=10)  # number of frames/steps
    parser.add_argument('--start_video', type=int, default=0)
    parser.add_argument('--end_video', type=int, default=1)  # number of videos, each video is a sequence of frames
    parser.add_argument('--unknown_dof', action='store_true')
    parser.add_argument('--vis_flow', action='store_true')
    parser.add_argument('--num_cameras', type=int, default=20)  # number of cameras
    parser.add_argument('--step_size', type=int, default=4)  # motor step size
    parser.add_argument('--diff', action='store_true')
    parser.add_argument('--legacy', action='store_true')
    return parser


def _cli_parser():
    """The reference's flags plus this project's own: --voxel_size meshes the links and --density (kg/m^3) fills the URDF's
    inertial blocks from those meshes (each overrides parameters.json's key of the same name); --joint_limits estimates
    every joint's positions, writes the observed range as its limits and replays the sequences on the URDF, --limit_pad
    (degrees, default 0) widens that range.  --limit_pad without --joint_limits is a usage error.  --collision_hull writes
    every link's convex hull next to its mesh and names it in the URDF's <collision> blocks.  --joint_types tells revolute,
    prismatic and fixed joints apart: --slide_min (the clouds' unit, required with it) and --turn_min (rad, default 2e-4)
    are its two thresholds.  --joint_types without --joint_limits, and a threshold without --joint_types, are usage errors.
    --cloud_fit sets the written URDF's meshes, posed at the recovered joint positions, against the raw clouds and writes
    <name>.cloud_fit.json; --fit_max (the clouds' unit, default inf) is the distance beyond which a point counts as
    unexplained.  --cloud_fit without --voxel_size or without --joint_limits, and --fit_max without --cloud_fit, are usage
    errors.  --fit_positions fits every frame's joint positions and base pose to its raw cloud after the cloud fit and writes
    <name>.fitted_positions.npy; --fit_iters (default 30) caps its iterations.  --fit_positions without --cloud_fit, and
    --fit_iters without --fit_positions, are usage errors.  --refine_joints refines the URDF's joint frames against all loaded
    raw clouds after the cloud fit and writes <name>.refined.urdf and <name>.refined_positions.npy; --refine_iters (default
    30) caps its iterations.  --refine_joints without --cloud_fit, and --refine_iters without --refine_joints, are usage
    errors.  --fit_metric {point,feature} chooses the curvature of both fits (``compute_joints.fit_cloud_poses``); without
    --fit_positions or --refine_joints it is a usage error.  --coverage measures the other direction after the cloud fit --
    how much of the posed mesh surface has a raw point within --fit_max -- and adds a "coverage" block to
    <name>.cloud_fit.json; --coverage without --cloud_fit is a usage error."""
    parser = _parser()
    parser.add_argument('--voxel_size', type=float, default=None)
    parser.add_argument('--density', type=float, default=None)
    parser.add_argument('--joint_limits', action='store_true')
    parser.add_argument('--limit_pad', type=float, default=None)
    parser.add_argument('--collision_hull', action='store_true')
    parser.add_argument('--joint_types', action='store_true')
    parser.add_argument('--slide_min', type=float, default=None)
    parser.add_argument('--turn_min', type=float, default=None)
    parser.add_argument('--cloud_fit', action='store_true')
    parser.add_argument('--fit_max', type=float, default=None)
    parser.add_argument('--fit_positions', action='store_true')
    parser.add_argument('--fit_iters', type=int, default=None)
    parser.add_argument('--refine_joints', action='store_true')
    parser.add_argument('--refine_iters', type=int, default=None)
    parser.add_argument('--fit_metric', choices=('point', 'feature'), default=None)
    parser.add_argument('--coverage', action='store_true')
    parse = parser.parse_args

    def parse_args(args=None, namespace=None):
        ns = parse(args, namespace)
        if ns.limit_pad is not None and not ns.joint_limits:
            parser.error("--limit_pad needs --joint_limits")
        if ns.joint_types and not ns.joint_limits:
            parser.error("--joint_types needs --joint_limits: a prismatic joint has no placeholder range")
        if (ns.slide_min is not None or ns.turn_min is not None) and not ns.joint_types:
            parser.error("--slide_min and --turn_min need --joint_types")
        if ns.cloud_fit and ns.voxel_size is None:
            parser.error("--cloud_fit needs --voxel_size: it measures the raw clouds against the link meshes")
        if ns.cloud_fit and not ns.joint_limits:
            parser.error("--cloud_fit needs --joint_limits: the meshes are posed at the recovered joint positions")
        if ns.fit_max is not None and not ns.cloud_fit:
            parser.error("--fit_max needs --cloud_fit")
        if ns.fit_positions and not ns.cloud_fit:
            parser.error("--fit_positions needs --cloud_fit: it starts from the poses the cloud fit measures")
        if ns.fit_iters is not None and not ns.fit_positions:
            parser.error("--fit_iters needs --fit_positions")
        if ns.refine_joints and not ns.cloud_fit:
            parser.error("--refine_joints needs --cloud_fit: it starts from the poses the cloud fit measures")
        if ns.refine_iters is not None and not ns.refine_joints:
            parser.error("--refine_iters needs --refine_joints")
        if ns.fit_metric is not None and not (ns.fit_positions or ns.refine_joints):
            parser.error("--fit_metric needs --fit_positions or --refine_joints: it is the curvature of their steps")
        if ns.coverage and not ns.cloud_fit:
            parser.error("--coverage needs --cloud_fit: it measures the other direction at the poses and clouds of the cloud fit")
        return ns
    parser.parse_args = parse_args
    return parser


def _joint_motion_report(urdf_path, motion, replay, pad_deg, start_step):
    """Write <name>.joint_motion.json (per-joint and per-link figures) and <name>.joint_positions.npy (J,S,steps) next to
    the URDF and print one line per joint plus the worst replayed link.  Typed joints (``--joint_types``) carry their "type"
    and "unit" into the file, and their lines name the type and give a prismatic joint's range in the clouds' unit."""
    import json
    stem = urdf_path[:-len('.urdf')] if urdf_path.endswith('.urdf') else urdf_path
    np.save(stem + '.joint_positions.npy', np.array([m["positions"] for m in motion], np.float64))
    joints = [{k: v for k, v in m.items() if k != "positions"} for m in motion]
    with open(stem + '.joint_motion.json', 'w') as f:
        json.dump({"urdf": urdf_path, "limit_pad_deg": pad_deg, "start_step": start_step, "unit": "rad",
                   "joints": joints, "links": replay}, f, indent=1,
                  default=lambda o: o.item() if hasattr(o, "item") else str(o))     # numpy scalars (link ids)
    for m in motion:
        if "type" not in m:
            print(f"joint_{m['child_link']} ({m['parent_link']} -> {m['child_link']}): {np.degrees(m['lower']):.2f} .. "
                  f"{np.degrees(m['upper']):.2f} deg, tilt_rms {m['tilt_rms']:.3g} rad, slip_rms {m['slip_rms']:.3g}")
            continue
        span = {"revolute": f"{np.degrees(m['lower']):.2f} .. {np.degrees(m['upper']):.2f} deg",
                "prismatic": f"{m['lower']:.6g} .. {m['upper']:.6g} length units", "fixed": "no motion"}[m["type"]]
        print(f"joint_{m['child_link']} ({m['parent_link']} -> {m['child_link']}), {m['type']}: {span}, "
              f"tilt_rms {m['tilt_rms']:.3g} rad, slip_rms {m['slip_rms']:.3g}")
    seen = [r for r in replay if r["n_used"]]
    if seen:
        w = max(seen, key=lambda r: r["rot_max"])
        print(f"replay: worst link {w['link']}: rot_max {w['rot_max']:.3g} rad at {w['rot_max_at']}, "
              f"pos_max {w['pos_max']:.3g} at {w['pos_max_at']}")


def _cloud_fit_report(urdf_path, fit, fit_max, start_step, num_steps, seq_names, fitted=None, refined=None, coverage=None):
    """Write <name>.cloud_fit.json next to the URDF -- the per-frame, per-sequence, per-link and overall figures of
    ``cloud_fit``, without the per-point arrays -- and print one line per sequence (rms, p95, unexplained share) and the worst
    frame.  ``fit_max`` is written as null when it is inf.  A ``fitted`` or ``refined`` dict that carries a "metric" (the
    command line's --fit_metric or the fit_metric key, when given) has it written into its block.  With
    ``fitted`` (``fit_positions``' dict) the file gains a "fitted"
    block -- per frame the rms before and after the fit and the steps tried, per sequence and overall the rms before and
    after, per joint the largest |q_fit - q_registered| --, <name>.fitted_positions.npy (J,S,steps) is written beside
    joint_positions.npy, and one line per sequence and one per joint are printed.  With ``refined`` (``refine_urdf_joints``'
    dict, "urdf" naming the file it wrote) the file gains a "refined" block -- the overall rms before and after, the steps tried,
    per joint the angle between the old and the new axis, the distance of the old joint point from the new line and the largest
    |q - q_registered| --, <name>.refined_positions.npy (J,S,steps) is written, and one line per joint is printed.  With
    ``coverage`` (``cloud_cover``'s dict) the file gains a "coverage" block -- per frame, per sequence, per link and overall the
    figures of ``surface_cover_poses``, without the arrays --, and one line per sequence (uncovered share, rms) and one per link
    (uncovered, never) are printed."""
    import json
    stem = urdf_path[:-len('.urdf')] if urdf_path.endswith('.urdf') else urdf_path
    clean = lambda d: {k: (None if isinstance(v, float) and not np.isfinite(v) else v) for k, v in d.items()}
    frames = [dict(clean(f), sequence=i // num_steps, step=start_step + i % num_steps) for i, f in enumerate(fit["poses"])]
    report = {"urdf": urdf_path, "fit_max": None if np.isinf(fit_max) else fit_max, "start_step": start_step,
              "unit": "the clouds' unit", "all": clean(fit["all"]), "sequences": [clean(s) for s in fit["sequences"]],
              "links": [clean(l) for l in fit["links"]], "frames": frames}
    if fitted is not None:
        np.save(stem + '.fitted_positions.npy', fitted["positions"])
        S = len(fitted["rms_before"]) // num_steps
        live = np.array([f["n"] for f in fit["poses"]], np.float64)                 # weights: a frame's points
        pooled = lambda rms, rows: float(np.sqrt(np.nansum(rms[rows] ** 2 * live[rows]) / max(live[rows].sum(), 1.0)))
        rows_of = [np.arange(s * num_steps, (s + 1) * num_steps) for s in range(S)]
        report["fitted"] = {
            "frames": [clean({"sequence": i // num_steps, "step": start_step + i % num_steps, "rms_before": float(b), "rms_after": float(a),
                              "iterations": int(k)})
                       for i, (b, a, k) in enumerate(zip(fitted["rms_before"], fitted["rms_after"], fitted["iterations"]))],
            "sequences": [{"rms_before": pooled(fitted["rms_before"], r), "rms_after": pooled(fitted["rms_after"], r)} for r in rows_of],
            "all": {"rms_before": pooled(fitted["rms_before"], np.arange(S * num_steps)),
                    "rms_after": pooled(fitted["rms_after"], np.arange(S * num_steps))},
            "joints": [{"joint": name, "max_shift": float(d)} for name, d in zip(fitted["joint_names"], fitted["shift"])]}
        if "metric" in fitted:
            report["fitted"]["metric"] = fitted["metric"]
    if refined is not None:
        np.save(stem + '.refined_positions.npy', refined["positions"])
        report["refined"] = {"urdf": refined["urdf"], "iterations": int(refined["iterations"]),
                             "all": clean({"rms_before": float(refined["rms_all_before"]), "rms_after": float(refined["rms_all_after"])}),
                             "joints": [clean(dict(j)) for j in refined["joints"]]}
        if "metric" in refined:
            report["refined"]["metric"] = refined["metric"]
    if coverage is not None:
        report["coverage"] = {
            "all": clean(coverage["all"]), "sequences": [clean(s) for s in coverage["sequences"]],
            "links": [clean(l) for l in coverage["links"]],
            "frames": [dict(clean(f), sequence=i // num_steps, step=start_step + i % num_steps) for i, f in enumerate(coverage["poses"])]}
    with open(stem + '.cloud_fit.json', 'w') as f:
        json.dump(report, f, indent=1)
    for name, s in zip(seq_names, fit["sequences"]):
        print(f"cloud_fit {name}: rms {s['rms']:.3g}, p95 {s['p95']:.3g}, unexplained {s['unexplained'] / max(s['n'], 1):.2%} of {s['n']}")
    seen = [f for f in frames if f["rms"] is not None]
    if seen:
        w = max(seen, key=lambda f: f["rms"])
        print(f"cloud_fit: worst frame sequence {w['sequence']} step {w['step']}: rms {w['rms']:.3g}, max {w['max']:.3g} at point {w['max_at']}")
    if fitted is not None:
        for name, s in zip(seq_names, report["fitted"]["sequences"]):
            print(f"fit_positions {name}: rms {s['rms_before']:.3g} -> {s['rms_after']:.3g}")
        for j in report["fitted"]["joints"]:
            print(f"fit_positions {j['joint']}: largest |q_fit - q_registered| {j['max_shift']:.3g}")
    if refined is not None:
        r = report["refined"]
        print(f"refine_joints: rms {r['all']['rms_before']:.3g} -> {r['all']['rms_after']:.3g} in {r['iterations']} steps, {r['urdf']}")
        for j in r["joints"]:
            line = "no line" if j["line_distance"] is None else f"old point {j['line_distance']:.3g} from the new line"
            print(f"refine_joints {j['joint']}: axis turned by {j['axis_angle']:.3g} rad, {line}, "
                  f"largest |q - q_registered| {j['max_shift']:.3g}")
    if coverage is not None:
        for name, s in zip(seq_names, coverage["sequences"]):
            print(f"coverage {name}: uncovered {s['uncovered']:.2%} of the surface, rms {s['rms']:.3g}")
        for l in coverage["links"]:
            print(f"coverage {l['link']}: uncovered {l['uncovered']:.2%}, never covered {l['never']:.2%}")


def main(argv=None):
    """The reference's ``python coord_map.py`` (coord_map.py:641-792) without its viewers and plots: sum maps, MST, link
    discovery, kinematic tree, joint axes, link clouds, their ICP refinement, the link meshes and the URDF file.  Paths
    are the reference's, relative to the working directory, and ``parameters.json`` is read from there.  The links are
    meshed (``{i:04}.ply`` and ``{i:04}.stl`` in the link directory, the files the URDF names) when the robot's entry has a
    ``voxel_size`` or ``--voxel_size`` is given; the option wins.  With a ``density`` (the key or ``--density``, kg/m^3; the
    option wins) the meshes' mass properties replace the placeholder ``<inertial>`` blocks (``link_inertia``,
    ``set_inertials``); a density without a voxel size is a ValueError before anything is written.  With ``--joint_limits``
    (or a ``joint_limits`` key; ``--limit_pad`` / ``limit_pad`` in degrees, the option wins) every joint's positions over
    all loaded sequences are estimated, the observed range replaces the placeholder limits, the sequences are replayed on
    the written URDF, and ``<name>.joint_motion.json`` and ``<name>.joint_positions.npy`` are written next to it; a pad
    without joint limits is a ValueError before anything is written.  With ``--collision_hull`` (or a boolean
    ``collision_hull`` key; the option wins) every link's exact convex hull is written as ``{i:04}_hull.stl`` and the URDF's
    ``<collision>`` blocks name it (``link_mesh(..., hull=True)``, ``set_collision_meshes``), one line per link is printed --
    triangles of the visual mesh -> triangles of the hull -- and the inertials stay computed from the visual meshes; without a
    voxel size it is a ValueError before anything is written.  With ``--joint_types`` (or a boolean ``joint_types`` key;
    ``--slide_min`` / ``slide_min`` in the clouds' unit, ``--turn_min`` / ``turn_min`` in rad, the option wins) the joints
    come from ``estimate_typed_joints_from_tree``: a child that never turns against its parent becomes a prismatic or a fixed
    joint instead of a ValueError, the report names every joint's type and unit, and a prismatic joint's limits are its
    observed slide.  It needs the joint limits and a ``slide_min``, and a threshold needs it: ValueError before anything is
    written otherwise.  With ``--cloud_fit`` (or a boolean ``cloud_fit`` key; ``--fit_max`` / ``fit_max`` in the clouds' unit,
    default inf, the option wins) the written URDF's meshes, posed by its joints at the recovered positions, are set against
    every loaded raw cloud after the replay (``cloud_fit``: one ``ops.point_mesh_distance`` call), ``<name>.cloud_fit.json`` is
    written next to the URDF and one line per sequence and the worst frame are printed.  It needs the link meshes and the joint
    limits, and a ``fit_max`` needs it: ValueError before anything is written otherwise.  With ``--fit_positions`` (or a boolean
    ``fit_positions`` key; ``--fit_iters`` / ``fit_iters``, default 30, the option wins) every frame's joint positions and base
    pose are then fitted to its raw cloud (``fit_positions``: from the replay's positions and the registered root motion, the
    base free, ``fit_max`` as the distance limit), ``<name>.fitted_positions.npy`` (J,S,steps) is written beside
    ``joint_positions.npy``, ``cloud_fit.json`` gains a "fitted" block, and one line per sequence (rms before -> after) and per
    joint (the largest |q_fit - q_registered|) are printed; the URDF and its limits are not touched.  It needs the cloud fit,
    and a ``fit_iters`` needs it: ValueError before anything is written otherwise.  With ``--refine_joints`` (or a boolean
    ``refine_joints`` key; ``--refine_iters`` / ``refine_iters``, default 30, the option wins) the frames of the URDF's movable
    joints are then refined against all loaded raw clouds at once (``refine_urdf_joints``: from the cloud fit's poses, the base
    free, ``fit_max`` as the distance limit), ``<name>.refined.urdf`` and ``<name>.refined_positions.npy`` (J,S,steps) are
    written beside the URDF, ``cloud_fit.json`` gains a "refined" block and one line per joint is printed; the original URDF
    keeps every byte.  It needs the cloud fit, and a ``refine_iters`` needs it: ValueError before anything is written
    otherwise.  ``--fit_metric`` (or a ``fit_metric`` key, "point" or "feature"; the option wins) is the ``metric`` of both fits
    and is written into their blocks of ``cloud_fit.json``; without it nothing changes, and without ``fit_positions`` or
    ``refine_joints`` it is a ValueError before anything is written.  With ``--coverage`` (or a boolean ``coverage`` key; the
    option wins) the other direction is measured after the cloud fit (``cloud_cover``: one ``ops.mesh_cover`` call, ``fit_max`` as
    its ``d_max``): ``cloud_fit.json`` gains a "coverage" block and one line per sequence and per link is printed.  It needs the
    cloud fit: ValueError before anything is written otherwise.  Without it no such launch is made and every written byte stays."""
    import json
    import os

    from . import prefer_device_kernargs
    prefer_device_kernargs()                    # (the command-line entry point: before the first device call)
    from .compute_joints import (cloud_cover, cloud_fit, create_urdf, estimate_joint_axes_from_tree, estimate_joint_motion,
                                 estimate_typed_joints_from_tree, fit_positions, refine_urdf_joints, replay_urdf, set_collision_meshes,
                                 set_inertials, set_joint_limits)
    from .link import link_inertia, link_mesh, refine_links_clusters, save_links, visualize_links
    args = _cli_parser().parse_args(argv)
    if not torch.cuda.is_available():
        raise RuntimeError("autourdf_amd.coord_map needs an MI355X: no GPU is visible and there is no CPU path")
    with open('parameters.json') as f:
        robot_params = json.load(f)[args.robot]
    voxel_size = args.voxel_size if args.voxel_size is not None else robot_params.get('voxel_size')
    density = args.density if args.density is not None else robot_params.get('density')
    if density is not None and voxel_size is None:
        raise ValueError("a density needs the link meshes: give --voxel_size (or a voxel_size key in parameters.json) with it")
    collision_hull = bool(args.collision_hull or robot_params.get('collision_hull'))
    if collision_hull and voxel_size is None:
        raise ValueError("collision hulls need the link meshes: give --voxel_size (or a voxel_size key in parameters.json) with "
                         "--collision_hull")
    joint_limits = bool(args.joint_limits or robot_params.get('joint_limits'))
    limit_pad = args.limit_pad if args.limit_pad is not None else robot_params.get('limit_pad')
    if limit_pad is not None and not joint_limits:
        raise ValueError("a limit_pad needs the joint limits: give --joint_limits (or a joint_limits key in parameters.json) with it")
    limit_pad = 0.0 if limit_pad is None else float(limit_pad)
    if not limit_pad >= 0.0:
        raise ValueError(f"limit_pad must be >= 0 degrees, got {limit_pad}")
    joint_types = bool(args.joint_types or robot_params.get('joint_types'))
    slide_min = args.slide_min if args.slide_min is not None else robot_params.get('slide_min')
    turn_min = args.turn_min if args.turn_min is not None else robot_params.get('turn_min')
    if (slide_min is not None or turn_min is not None) and not joint_types:
        raise ValueError("slide_min and turn_min are the thresholds of the joint types: give --joint_types (or a joint_types key "
                         "in parameters.json) with them")
    if joint_types and not joint_limits:
        raise ValueError("joint types need the joint limits, a prismatic joint has no placeholder range: give --joint_limits "
                         "(or a joint_limits key in parameters.json) with --joint_types")
    if joint_types and slide_min is None:
        raise ValueError("joint types need a slide_min, a length in the clouds' unit: give --slide_min (or a slide_min key in "
                         "parameters.json) with --joint_types")
    for name, value in (("slide_min", slide_min), ("turn_min", turn_min)):
        if value is not None and not (np.isfinite(float(value)) and float(value) >= 0.0):
            raise ValueError(f"{name} must be finite and >= 0, got {value}")
    want_fit = bool(args.cloud_fit or robot_params.get('cloud_fit'))
    fit_max = args.fit_max if args.fit_max is not None else robot_params.get('fit_max')
    if fit_max is not None and not want_fit:
        raise ValueError("a fit_max is the cloud fit's distance limit: give --cloud_fit (or a cloud_fit key in parameters.json) with it")
    if want_fit and voxel_size is None:
        raise ValueError("the cloud fit needs the link meshes: give --voxel_size (or a voxel_size key in parameters.json) with "
                         "--cloud_fit")
    if want_fit and not joint_limits:
        raise ValueError("the cloud fit poses the meshes at the recovered joint positions: give --joint_limits (or a joint_limits "
                         "key in parameters.json) with --cloud_fit")
    fit_max = float("inf") if fit_max is None else float(fit_max)
    if not fit_max >= 0.0:
        raise ValueError(f"fit_max must be >= 0 (inf allowed), got {fit_max}")
    want_positions = bool(args.fit_positions or robot_params.get('fit_positions'))
    fit_iters = args.fit_iters if args.fit_iters is not None else robot_params.get('fit_iters')
    if want_positions and not want_fit:
        raise ValueError("fit_positions starts from the poses the cloud fit measures: give --cloud_fit (or a cloud_fit key in "
                         "parameters.json) with --fit_positions")
    if fit_iters is not None and not want_positions:
        raise ValueError("a fit_iters is the iteration cap of fit_positions: give --fit_positions (or a fit_positions key in "
                         "parameters.json) with it")
    fit_iters = 30 if fit_iters is None else int(fit_iters)
    if fit_iters < 0:
        raise ValueError(f"fit_iters must be >= 0, got {fit_iters}")
    want_refine = bool(args.refine_joints or robot_params.get('refine_joints'))
    refine_iters = args.refine_iters if args.refine_iters is not None else robot_params.get('refine_iters')
    if want_refine and not want_fit:
        raise ValueError("refine_joints starts from the poses the cloud fit measures: give --cloud_fit (or a cloud_fit key in "
                         "parameters.json) with --refine_joints")
    if refine_iters is not None and not want_refine:
        raise ValueError("a refine_iters is the iteration cap of refine_joints: give --refine_joints (or a refine_joints key in "
                         "parameters.json) with it")
    refine_iters = 30 if refine_iters is None else int(refine_iters)
    if refine_iters < 0:
        raise ValueError(f"refine_iters must be >= 0, got {refine_iters}")
    fit_metric = args.fit_metric if args.fit_metric is not None else robot_params.get('fit_metric')
    if fit_metric is not None and not (want_positions or want_refine):
        raise ValueError("a fit_metric is the curvature of fit_positions and refine_joints: give --fit_positions or --refine_joints "
                         "(or their keys in parameters.json) with it")
    if fit_metric not in (None, "point", "feature"):
        raise ValueError(f"fit_metric must be 'point' or 'feature', got {fit_metric!r}")
    metric = {} if fit_metric is None else {"metric": fit_metric}
    want_cover = bool(args.coverage or robot_params.get('coverage'))
    if want_cover and not want_fit:
        raise ValueError("coverage measures the other direction at the poses and clouds of the cloud fit: give --cloud_fit (or a "
                         "cloud_fit key in parameters.json) with --coverage")
    ROBOT, NUM_SEG = args.robot, robot_params['num_seg']
    STEP, CAMS, START, END = args.step_size, args.num_cameras, args.start_steps, args.end_steps
    part_path = f'data/part/{ROBOT}_{NUM_SEG}_seg/{STEP}_deg_{CAMS}_cams/'
    link_path = f'data/mesh/{ROBOT}_{NUM_SEG}_seg/{STEP}_deg_{CAMS}_cams/'
    raw_path_list = sorted(glob.glob(f'data/raw/{ROBOT}/{STEP}_deg_{CAMS}_cams/*/'))
    if len(raw_path_list) == 0:                                      # real data
        raw_path_list = sorted(glob.glob(f'data/raw/{ROBOT}/*/'))
    sub_part_path = sorted(glob.glob(part_path + '*/'))[args.start_video:args.end_video]
    sub_raw_path = raw_path_list[args.start_video:args.end_video]
    if not sub_part_path or len(sub_raw_path) < len(sub_part_path):
        raise FileNotFoundError(f"need registered sequences under {part_path} and their raw frames under data/raw/{ROBOT}/")
    print(sub_part_path)

    cm_list, sum_map_list = [], []
    for i, path in enumerate(sub_part_path):
        cm = CoordMap(path, sub_raw_path[i], start_steps=START, end_steps=END)
        if args.legacy:
            _, sum_map = cm.coord_dist_map_legacy(diff=False)
        else:
            _, sum_map = cm.coord_dist_map(diff=args.diff)
        cm_list.append(cm)
        sum_map_list.append(sum_map)
    sum_map = np.mean(sum_map_list, axis=0)
    sum_map = (sum_map - np.min(sum_map)) / (np.max(sum_map) - np.min(sum_map))

    g0 = cm_list[0].coord_mst()
    if args.unknown_dof:
        test_num_links = (4, min(25, cm_list[0].num_coords))
        cluster_idx, g1, s_score_list, nls = silhouette_score_method(cm_list[0].num_coords, sum_map,
                                                                     link_range=test_num_links)
        if len(sub_part_path) == 1:
            print("score folder", sub_part_path[0] + 'score/')
            os.makedirs(sub_part_path[0] + 'score/', exist_ok=True)
            with open(sub_part_path[0] + 'score/silhouette_score.txt', 'w') as f:
                f.write(f"Silhouette Score: {s_score_list}\n")
                f.write(f"Number of Links: {nls}\n")
        dof = len(cluster_idx) - 1
    else:
        dof = robot_params['dof']
        cluster_idx, g1, _ = coord_clustering(cm_list[0].num_coords, sum_map, num_links=dof + 1)

    links = cm_list[0].kinematics_tree(g0, g1)
    if joint_types:
        joint_data = estimate_typed_joints_from_tree(links, cm_list, START, END - START, 4, float(slide_min),
                                                     None if turn_min is None else float(turn_min))
    else:
        joint_data = estimate_joint_axes_from_tree(links, cm_list, START, END - START, 4)
    sub_link_path = [link_path + path.split('/')[-2] + '/' for path in sub_part_path][:1]
    save_links(cm_list, cluster_idx, sub_link_path, START, END)
    refine_links_clusters(sub_link_path, START, END, dof)
    if voxel_size is None:
        print("skipped (out of scope): the cluster / link viewers and plots, visualize_links, link_mesh (meshing), "
              "visualize_kinematic_tree and visualize_urdf")
    else:
        visualize_links(sub_link_path, START, END, dof, False)
        if collision_hull:
            for i, (nv, nh) in enumerate(link_mesh(sub_link_path, dof, voxel_size, False, hull=True)[0]):
                print(f"link_{i}: {nv} triangles -> hull of {nh} triangles")
        else:
            link_mesh(sub_link_path, dof, voxel_size, False)
        inertials = link_inertia(sub_link_path, dof, density) if density is not None else None
        print("skipped (out of scope): the cluster / link viewers and plots, visualize_kinematic_tree and visualize_urdf")
    os.makedirs(f'data/urdf/{ROBOT}_{NUM_SEG}_seg/', exist_ok=True)
    urdf_path = f'data/urdf/{ROBOT}_{NUM_SEG}_seg/{STEP}_deg_{CAMS}_cams.urdf'
    create_urdf(links, joint_data, cm_list[0], urdf_path, sub_link_path[0])
    if density is not None:
        set_inertials(urdf_path, inertials[0])
    if collision_hull:
        set_collision_meshes(urdf_path)
    if joint_limits:
        motion = estimate_joint_motion(links, joint_data, cm_list, START, END - START)
        set_joint_limits(urdf_path, motion, float(np.radians(limit_pad)))
        replay = replay_urdf(urdf_path, links, motion, cm_list, START, END - START)
        _joint_motion_report(urdf_path, motion, replay, limit_pad, START)
        if want_fit:
            fit = cloud_fit(urdf_path, links, motion, cm_list, sub_raw_path[:len(cm_list)], START, END - START, d_max=fit_max)
            fitted = None
            if want_positions:
                fitted = fit_positions(urdf_path, links, motion, cm_list, sub_raw_path[:len(cm_list)], START, END - START,
                                       d_max=fit_max, max_iter=fit_iters, **metric)
                fitted.update(metric)
                fitted["joint_names"] = [f"joint_{m['child_link']}" for m in motion]
            refined = None
            if want_refine:
                refined_path = urdf_path[:-len('.urdf')] + '.refined.urdf'
                refined = refine_urdf_joints(urdf_path, links, motion, cm_list, sub_raw_path[:len(cm_list)], START, END - START,
                                             refined_path, d_max=fit_max, max_iter=refine_iters, **metric)
                refined.update(metric)
                refined["urdf"] = refined_path
            cover = None
            if want_cover:
                cover = cloud_cover(urdf_path, links, motion, cm_list, sub_raw_path[:len(cm_list)], START, END - START, d_max=fit_max)
            _cloud_fit_report(urdf_path, fit, fit_max, START, END - START, [p.rstrip('/').split('/')[-1] for p in sub_raw_path], fitted,
                              refined, cover)
    return urdf_path


if __name__ == "__main__":
    main()
