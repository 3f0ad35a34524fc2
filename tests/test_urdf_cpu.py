"""URDF stage, host side (no GPU): the fixture's sanity, the drop-in surface, the networkx stand-in and the
kinematic-tree bookkeeping against the reference's own results (tests/golden/urdf_reference.npz)."""
import inspect
import os
import re

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CASES = ["a", "b", "c"]


def _split(flat, sizes):
    return np.split(np.asarray(flat), np.cumsum(sizes)[:-1])


def _graph(nodes, edges):
    from autourdf_amd.coord_map import Graph
    G = Graph()
    G.add_nodes_from(range(nodes))
    G.add_edges_from([tuple(int(v) for v in e) for e in edges])
    return G


def test_noise_free_case_recovers_the_true_links(golden):
    g = golden("urdf_reference.npz")
    got = {frozenset(c.tolist()) for c in _split(g["a.cluster_idx"], g["a.cluster_sizes"])}
    link_of = g["a.link_of"]
    want = {frozenset(np.nonzero(link_of == l)[0].tolist()) for l in range(len(g["a.parents"]))}
    assert got == want
    assert int(g["a.num_links"]) == len(g["a.parents"])


def test_drop_in_signatures_match_the_reference_surface():
    from autourdf_amd import coord_map, ops
    sig = lambda f: list(inspect.signature(f).parameters)
    assert sig(coord_map.coord_clustering) == ["num_coords", "d_map", "num_links"]
    assert sig(coord_map.silhouette_score_method) == ["num_coords", "d_map", "link_range"]
    assert inspect.signature(coord_map.silhouette_score_method).parameters["link_range"].default == (3, 15)
    assert sig(coord_map.CoordMap.coord_mst) == ["self"]
    assert sig(coord_map.CoordMap.kinematics_tree) == ["self", "g0", "g1"]
    G = coord_map.Graph()
    for name in ("nodes", "edges", "neighbors", "add_nodes_from", "add_edges_from", "add_edge"):
        assert hasattr(G, name)
    for name in ("link_sweep", "coord_mst"):
        assert callable(getattr(ops, name))


def test_new_code_imports_no_reference_only_wheel():
    src = open(os.path.join(ROOT, "autourdf_amd", "coord_map.py")).read()
    for mod in ("oracle", "networkx", "sklearn", "matplotlib", "transforms3d", "open3d", "pybullet"):
        assert not re.search(rf"^\s*(from|import)\s+{mod}\b", src, re.M), mod


@pytest.mark.parametrize("tag", CASES)
def test_connected_components_iterate_like_networkx(golden, tag):
    """The stand-in's components of the reference's g1, in order and in set iteration order."""
    from autourdf_amd.coord_map import connected_components
    g = golden("urdf_reference.npz")
    K = len(g[f"{tag}.sum_map"])
    comps = list(connected_components(_graph(K, g[f"{tag}.g1_edges"])))
    want = _split(g[f"{tag}.cluster_idx"], g[f"{tag}.cluster_sizes"])
    assert [list(c) for c in comps] == [w.tolist() for w in want]
    assert [tuple(e) for e in _graph(K, g[f"{tag}.g1_edges"]).edges] == [tuple(e) for e in g[f"{tag}.g1_edges"].tolist()]


@pytest.mark.parametrize("tag", CASES)
def test_kinematics_tree_bookkeeping_matches_the_reference(golden, tag, capsys):
    """Movement sort, BFS (incl. the count > 100 cap that case b's cyclic link graph hits), parent_id / tree_id,
    final sort, and every set's iteration order."""
    from autourdf_amd.coord_map import CoordMap
    g = golden("urdf_reference.npz")
    K = len(g[f"{tag}.sum_map"])
    cm = CoordMap.__new__(CoordMap)
    cm.coords, cm.num_coords = g[f"{tag}.coords0"], K
    links = cm.kinematics_tree(_graph(K, g[f"{tag}.g0_edges"]), _graph(K, g[f"{tag}.g1_edges"]))
    assert [l["id"] for l in links] == g[f"{tag}.link_id"].tolist()
    assert [l["tree_id"] for l in links] == g[f"{tag}.link_tree_id"].tolist()
    assert [-1 if l["parent_id"] is None else l["parent_id"] for l in links] == g[f"{tag}.link_parent_id"].tolist()
    assert [x for l in links for x in l["cluster_idx"]] == g[f"{tag}.link_cluster_idx"].tolist()
    assert [x for l in links for x in l["connected_links"]] == g[f"{tag}.link_connected"].tolist()
    assert [len(l["connected_links"]) for l in links] == g[f"{tag}.link_connected_sizes"].tolist()
