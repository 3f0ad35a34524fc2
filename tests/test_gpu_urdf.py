"""N4, the graph half of the URDF stage on the GPU: creg_link_sweep_f64 / creg_coord_mst_f64 and the coord_map
drop-ins against the reference's own results (tests/golden/urdf_reference.npz) and a numpy restatement
(tests/_urdf_ref.py) on random maps across the LDS (K <= 128) and global-memory paths."""
import os
import sys

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import _urdf_ref as R  # noqa: E402

CASES = ["a", "b", "c"]


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available()
    return torch.device("cuda")


def _split(flat, sizes):
    return [c.tolist() for c in np.split(np.asarray(flat), np.cumsum(sizes)[:-1])]


@pytest.mark.parametrize("tag", CASES)
def test_link_sweep_vs_reference_golden(dev, golden, tag):
    from autourdf_amd import ops
    g = golden("urdf_reference.npz")
    lo, hi = (int(x) for x in g[f"{tag}.nl_range"])
    labels, n_comp, thr, scores, best = (x.cpu().numpy() for x in ops.link_sweep(torch.from_numpy(g[f"{tag}.sum_map"]).to(dev), lo, hi))
    np.testing.assert_array_equal(labels, g[f"{tag}.labels"])
    np.testing.assert_array_equal(n_comp, g[f"{tag}.n_comp"])
    np.testing.assert_array_equal(thr - 0.0001, g[f"{tag}.thr_printed"])      # the value the reference prints, bit for bit
    np.testing.assert_allclose(scores, g[f"{tag}.scores"], rtol=0, atol=1e-12)
    if int(g[f"{tag}.unknown_dof"]):
        assert lo + int(best[0]) == int(g[f"{tag}.num_links"])
    # one partition, one score: equal partitions from different link counts give identical bits
    for i in range(len(labels)):
        for j in range(i):
            if np.array_equal(labels[i], labels[j]):
                assert scores[i].tobytes() == scores[j].tobytes()


@pytest.mark.parametrize("tag", CASES)
def test_drop_ins_vs_reference_golden(dev, golden, tag, capsys):
    from autourdf_amd import coord_map
    g = golden("urdf_reference.npz")
    d = g[f"{tag}.sum_map"]
    K = len(d)
    lo, hi = (int(x) for x in g[f"{tag}.nl_range"])
    if int(g[f"{tag}.unknown_dof"]):
        cluster_idx, g1, s_score, nls = coord_map.silhouette_score_method(K, d, link_range=(lo, hi))
        np.testing.assert_array_equal(nls, np.arange(lo, hi))
        np.testing.assert_allclose(s_score, g[f"{tag}.scores"], rtol=0, atol=1e-12)
    else:
        cluster_idx, g1, s = coord_map.coord_clustering(K, d, int(g[f"{tag}.num_links"]))
    assert [list(c) for c in cluster_idx] == _split(g[f"{tag}.cluster_idx"], g[f"{tag}.cluster_sizes"])
    assert [tuple(e) for e in g1.edges] == [tuple(e) for e in g[f"{tag}.g1_edges"].tolist()]
    cm = coord_map.CoordMap.__new__(coord_map.CoordMap)
    cm.coords, cm.num_coords = g[f"{tag}.coords0"], K
    g0 = cm.coord_mst()
    assert g0.nodes == list(range(K))
    assert [tuple(e) for e in g0.edges] == [tuple(e) for e in g[f"{tag}.g0_edges"].tolist()]
    links = cm.kinematics_tree(g0, g1)
    assert [l["tree_id"] for l in links] == g[f"{tag}.link_tree_id"].tolist()
    assert [-1 if l["parent_id"] is None else l["parent_id"] for l in links] == g[f"{tag}.link_parent_id"].tolist()
    assert [x for l in links for x in l["cluster_idx"]] == g[f"{tag}.link_cluster_idx"].tolist()


@pytest.mark.parametrize("K", [2, 5, 20, 45, 64, 128, 129, 256])
def test_link_sweep_vs_numpy_restatement(dev, K):
    from autourdf_amd import ops
    for symmetric in (True, False):
        d = R.random_map(K, K, symmetric)
        lo, hi = (1, 3) if K == 2 else (2, min(25, K))
        labels, n_comp, thr, scores, best = (x.cpu().numpy() for x in ops.link_sweep(torch.from_numpy(d).to(dev), lo, hi))
        want_scores, valid = [], True
        for i, nl in enumerate(range(lo, hi)):
            t, lab = R.clustering(d, nl)
            assert thr[i] == t, (K, nl)
            np.testing.assert_array_equal(labels[i], lab)
            assert n_comp[i] == lab.max() + 1
            s = R.silhouette(d, lab)
            valid &= s is not None
            if s is not None:
                assert abs(scores[i] - s) <= 1e-12, (K, nl, scores[i], s)
            else:
                assert np.isnan(scores[i])
            want_scores.append(-np.inf if s is None else s)
        assert int(best[0]) == (int(np.argmax(want_scores)) if valid else -1)


def test_invalid_label_counts_raise_value_error(dev):
    from autourdf_amd import coord_map
    d = R.random_map(12, 0)
    with pytest.raises(ValueError):
        coord_map.coord_clustering(12, d, 12)                 # every node its own link: sklearn's n_labels == n_samples
    with pytest.raises(ValueError):
        coord_map.coord_clustering(12, d, 1)                  # one link
    with pytest.raises(ValueError):
        coord_map.coord_clustering(2, R.random_map(2, 0), 2)
    with pytest.raises(ValueError):
        coord_map.coord_clustering(257, np.zeros((257, 257)), 4)
    cluster_idx, _, s = coord_map.coord_clustering(12, d, 11)
    assert len(cluster_idx) == 11 and np.isfinite(s)


def test_coord_mst_matches_a_dense_prim(dev):
    """Any K up to 256 (several waves): the tree's total weight and edge set equal scipy's MST on distinct weights."""
    from scipy.sparse.csgraph import minimum_spanning_tree
    from scipy.spatial import distance_matrix
    from autourdf_amd import ops
    for K in (2, 7, 65, 200, 256):
        rng = np.random.default_rng(K)
        coords = np.concatenate([rng.normal(size=(4, K, 3)), rng.normal(size=(4, K, 4))], axis=-1)
        edges, w = (x.cpu().numpy() for x in ops.coord_mst(torch.from_numpy(coords).to(dev)))
        P = coords[:, :, :3].sum(0)
        want = minimum_spanning_tree(distance_matrix(P, P)).tocoo()
        assert {tuple(sorted(e)) for e in edges.tolist()} == {tuple(sorted(e)) for e in zip(want.row.tolist(), want.col.tolist())}
        np.testing.assert_allclose(w.sum(), want.data.sum(), rtol=1e-12)


# ---- link discovery on the maps real sequences produce: unnormalised (weights above 1), exact ties (identical tracks are at
# distance exactly 0, equal MST weights) and weights on, or one ulp either side of, the threshold lattice ----------------
def _assert_sweep_matches_restatement(dev, d, what):
    """Every nl in [2, min(K, 25)): labels, n_comp and the threshold double exact, scores to 1e-12 (NaN where sklearn
    raises), best as silhouette_score_method chooses.  Returns the device results."""
    from autourdf_amd import ops
    K = len(d)
    lo, hi = 2, min(25, K)
    labels, n_comp, thr, scores, best = (x.cpu().numpy() for x in ops.link_sweep(torch.from_numpy(d).to(dev), lo, hi))
    want_scores, valid = [], True
    for i, nl in enumerate(range(lo, hi)):
        t, lab = R.clustering(d, nl)
        assert thr[i].tobytes() == np.float64(t).tobytes(), (what, K, nl, float(thr[i]), float(t))
        np.testing.assert_array_equal(labels[i], lab, err_msg=f"{what} K={K} nl={nl}")
        assert n_comp[i] == lab.max() + 1, (what, K, nl)
        s = R.silhouette(d, lab)
        valid &= s is not None
        if s is not None:
            assert abs(scores[i] - s) <= 1e-12, (what, K, nl, scores[i], s)
        else:
            assert np.isnan(scores[i]), (what, K, nl, scores[i])
        want_scores.append(-np.inf if s is None else s)
    assert int(best[0]) == (int(np.argmax(want_scores)) if valid else -1), (what, K)
    return labels, n_comp, thr, scores, best


def _both(d):
    return [("symmetric", d), ("upper triangle * (1 + 2^-40)", R.unsymmetric(d))]


SWEEP_K = [9, 64, 128, 129]                      # 128 | 129: the map in LDS | in global memory


def test_block_map_k9_pinned(dev):
    """Three groups of identical tracks, both inter-group MST weights LATTICE[1234]: nl = 2 and nl = 3 share that threshold
    (the component count jumps from 1 to 3), nl >= 4 walks to the first lattice point at or below 0, where every node is
    alone and sklearn raises."""
    d, grp = R.block_map(9, [R.LATTICE[1234]] * 2, R.LATTICE[1234], 0)
    labels, n_comp, thr, scores, best = _assert_sweep_matches_restatement(dev, d, "block")
    assert thr[0] == thr[1] == R.LATTICE[1234] and n_comp[0] == n_comp[1] == 3
    first = {}
    np.testing.assert_array_equal(labels[0], [first.setdefault(g, len(first)) for g in grp])
    assert np.all(thr[2:] == -9.999999990618245e-05) and np.all(n_comp[2:] == 9) and np.all(np.isnan(scores[2:]))
    assert abs(scores[0] - 1.0) <= 1e-12 and int(best[0]) == -1


@pytest.mark.parametrize("K", SWEEP_K)
def test_link_sweep_block_maps(dev, K):
    """Groups of identical tracks; the chain of inter-group weights is drawn from three values, so MST weights tie and the
    component count jumps past some nl; past the number of groups only the zero edges are left."""
    g = min(K // 3, 27)
    for seed in range(3):
        chain = np.random.default_rng([K, seed]).choice([0.25, 0.5, R.LATTICE[1234]], g - 1)
        for what, d in _both(R.block_map(K, chain, 0.9, seed)[0]):
            _, n_comp, thr, _, _ = _assert_sweep_matches_restatement(dev, d, "block, " + what)
            assert len(set(n_comp.tolist())) < len(n_comp)                # the count did jump over some nl
            if g < min(25, K) - 1:
                assert thr[-1] == -9.999999990618245e-05 and n_comp[-1] == K


@pytest.mark.parametrize("K", SWEEP_K)
def test_link_sweep_lattice_exact_weights(dev, K):
    """MST weights that are lattice points or their float64 neighbours (different binades, either side of two binade
    crossings): the strict d < t decides by one ulp, and a Prim / cut-property answer one lattice step off shows in the
    threshold double.  K = 9 holds two such weights per map, the larger K all of them in one map."""
    w = sorted(set(R.lattice_weights()))
    if K == 9:
        chains = [[w[i], w[(i + 1) % len(w)]] for i in range(len(w))] + [[x, x] for x in w[::3]]
    else:
        chains = [np.random.default_rng([K, s]).permutation(w) for s in range(2)]
    for seed, chain in enumerate(chains):
        for what, d in _both(R.block_map(K, chain, 1.25, seed)[0]):
            _assert_sweep_matches_restatement(dev, d, "lattice, " + what)


@pytest.mark.parametrize("K", SWEEP_K)
def test_link_sweep_weights_above_one(dev, K):
    """Unnormalised maps.  With some weights above 1 the walk starts among them; with all of them above 1 the threshold stays
    1.0, every node is its own component, the score is NaN and best = -1."""
    for what, d in _both(R.above_one_map(K, K, every=False)):
        assert (d > 1).any() and (d[d > 0] < 1).any()
        _assert_sweep_matches_restatement(dev, d, "some above 1, " + what)
    for what, d in _both(R.above_one_map(K, K, every=True)):
        _, n_comp, thr, scores, best = _assert_sweep_matches_restatement(dev, d, "all above 1, " + what)
        assert np.all(thr == 1.0) and np.all(n_comp == K) and np.all(np.isnan(scores)) and int(best[0]) == -1


def test_coord_clustering_on_a_block_map(dev):
    """The drop-in at a reachable and an unreachable link count: it returns or raises exactly as the restatement says."""
    from autourdf_amd import coord_map
    d, grp = R.block_map(9, [R.LATTICE[1234]] * 2, R.LATTICE[1234], 0)
    for nl in range(2, 9):
        t, lab = R.clustering(d, nl)
        s = R.silhouette(d, lab)
        if s is None:
            with pytest.raises(ValueError):
                coord_map.coord_clustering(9, d, nl)
            continue
        cluster_idx, g1, got = coord_map.coord_clustering(9, d, nl)
        assert [sorted(c) for c in cluster_idx] == [np.nonzero(lab == c)[0].tolist() for c in range(lab.max() + 1)]
        assert sorted(g1.edges) == [(i, j) for i in range(9) for j in range(i + 1, 9) if d[i, j] < t]
        assert abs(got - s) <= 1e-12
    assert R.silhouette(d, R.clustering(d, 3)[1]) is not None and R.silhouette(d, R.clustering(d, 4)[1]) is None
