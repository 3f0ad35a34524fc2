"""CPU: the restatement of tests/_kmeans_ref.py is pinned to LIVE scikit-learn on every case that can be compared with it, every
case meets the conditioning conditions that make it a fair demand on a kernel (test_gpu_kmeans_edges.py holds the Lloyd kernels of
csrc/kmeans.hip and csrc/kmeans_nd.hip to the restatement), the cases reach the branches they are built for, and the torch-facing
wrappers refuse n < k before the library is loaded."""
import warnings

import numpy as np
import pytest

import _kmeans_ref as R

ALL = [(name, dim) for name in R.CASE_NAMES for dim in R.DIMS]
SKLEARN = [(c.name, dim) for c in R.CASES if c.sklearn for dim in R.DIMS]
EXACT = [(c.name, dim) for c in R.CASES if c.exact for dim in R.DIMS]


@pytest.mark.parametrize("name,dim", SKLEARN)
def test_restatement_matches_live_sklearn(name, dim):
    from sklearn.cluster import k_means
    X, init, max_iter, tol, ref = R.reference(name, dim)
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")                               # ConvergenceWarning: duplicate points, max_iter reached
        c, lab, inertia, n_iter = k_means(X.copy(), n_clusters=len(init), init=init.copy(), n_init=1, max_iter=max_iter, tol=tol,
                                          return_n_iter=True)
    np.testing.assert_array_equal(ref.labels, lab)
    assert ref.n_iter == n_iter
    assert np.abs(ref.centers - c).max() <= R.center_bound(X)
    assert abs(ref.inertia - inertia) <= R.inertia_bound(X, inertia)


@pytest.mark.parametrize("name,dim", ALL)
def test_case_meets_the_conditioning_conditions(name, dim):
    """Conditions, not measurements: a case that misses one gets another seed, the condition stays."""
    case = R.BY_NAME[name]
    X, init, max_iter, tol, ref = R.reference(name, dim)
    if not case.exact:
        assert ref.label_gap > 1e-9, ref.label_gap
        assert ref.shift_margin > 1e-6, ref.shift_margin
    if case.sklearn and not case.benign_tie:
        assert not ref.reloc_tie
    if case.benign_tie:                                               # the tie is there, and it decides nothing
        other = R.k_means(X, init, max_iter, tol, ties_to_higher_index=True)
        assert ref.reloc_tie and other.reloc_tie
        np.testing.assert_array_equal(other.labels, ref.labels)
        np.testing.assert_array_equal(other.centers, ref.centers)
        assert other.n_iter == ref.n_iter and other.inertia == ref.inertia


@pytest.mark.parametrize("name,dim", EXACT)
def test_exact_case_gives_the_same_bits_in_longdouble(name, dim):
    X, init, max_iter, tol, ref = R.reference(name, dim)
    ld = R.k_means(X, init, max_iter, tol, dtype=np.longdouble)
    np.testing.assert_array_equal(ld.labels, ref.labels)
    assert ld.n_iter == ref.n_iter
    np.testing.assert_array_equal(ld.centers.astype(np.float64), ref.centers)


@pytest.mark.parametrize("name", R.CASE_NAMES)
def test_c_oracle_matches_the_restatement_at_dim3(name):
    """oracle/creg_oracle.c, the checker of the GPU parity tests, follows the same rules (the empty-cluster list fixed before the
    relocation moves anything among them: `emptied_later`)."""
    from oracle import kmeans
    X, init, max_iter, tol, ref = R.reference(name, 3)
    c, lab, inertia, n_iter = kmeans.k_means(X, init, max_iter=max_iter, tol=tol)
    np.testing.assert_array_equal(lab, ref.labels)
    assert n_iter == ref.n_iter
    assert np.abs(c - ref.centers).max() <= R.center_bound(X)
    assert abs(inertia - ref.inertia) <= R.inertia_bound(X, ref.inertia)


def test_cases_reach_the_branches_they_are_built_for():
    for dim in R.DIMS:
        ref = {name: R.reference(name, dim)[4] for name in R.CASE_NAMES}
        X = R.reference("stop_default", dim)[0]
        # the stop rules: max_iter reached (1, 2, mid-run), strict convergence, the shift test at the default and at a large tol
        strict = ref["stop_strict_tol0"].n_iter
        assert [ref[n].n_iter for n in ("stop_iter1", "stop_iter2", "stop_iter5_tol0")] == [1, 2, 5] and strict > 5
        assert ref["stop_default"].n_iter <= strict and 1 < ref["stop_large_tol"].n_iter < ref["stop_default"].n_iter
        assert (ref["stop_iter5_tol0"].labels != ref["stop_strict_tol0"].labels).any()
        # sizes: every point its own cluster; relocations that fill every empty cluster
        assert (ref["n5_k5_reversed"].labels == np.arange(5)[::-1]).all() and (ref["n9_k9_far7"].counts == 1).all()
        assert ref["n9_k9_far7"].relocations >= 1 and ref["n300_k128_far28"].relocations >= 1
        assert (ref["n300_k128_far28"].counts > 0).all()
        for name in ("n16384_k128", "n16385_k128"):
            assert ref[name].n_iter == 8 and ref[name].relocations >= 1 and (ref[name].counts > 0).all()
        # degenerate data: the skipped relocation, the empty cluster on the heaviest one's centre
        for name in ("allsame", "allsame_tol0"):
            r = ref[name]
            assert r.n_iter == 1 and r.relocations == 0 and r.relocations_skipped == 1 and r.still_empty
            assert list(r.counts) == [50, 0, 0] and (r.centers == r.centers[0]).all() and r.inertia == 0
        for name in R.CASE_NAMES:
            if name.startswith("twopts"):
                r = ref[name]
                assert r.relocations == 1 and r.relocations_skipped >= 1 and r.still_empty and sorted(r.counts) == [0, 0, 32, 32]
        assert (ref["offset"].labels == ref["stop_default"].labels).all() and ref["offset"].n_iter == ref["stop_default"].n_iter
        for name in ("outlier", "outlier_tol0"):
            assert ref[name].counts[0] == 1 and ref[name].centers[0, 0] == 1e6
        assert ref["outlier"].n_iter == 1 < ref["outlier_tol0"].n_iter
        r = ref["emptied_later"]
        assert r.relocations >= 2 and r.still_empty and (r.counts > 0).all() and r.counts[0] == 1 and r.centers[0, 0] == 40.0
        assert ref["ties_two_seeds"].n_iter == 3 and list(ref["ties_two_seeds"].counts) == [48, 16]
        np.testing.assert_array_equal(ref["ties_two_seeds"].centers[:, 0], [1.0, 5.0])
        r = ref["ties_duplicate_seeds"]
        assert r.relocations == 3 and list(r.counts) == [32, 16, 16, 0] and r.centers[3, 0] == 0.0
        assert np.abs(X).max() < 10                                   # (the 500 normal points the stop-rule cases share)


def test_the_batch_cases_share_one_shape():
    shapes = {(R.reference(name, 3)[0].shape, R.reference(name, 3)[1].shape) for name in R.BATCH_CASES}
    assert shapes == {((64, 3), (4, 3))}


@pytest.mark.parametrize("entry", ["kmeans_lloyd", "kmeans_lloyd_nd", "kmeans_lloyd_batch"])
def test_ops_refuse_fewer_points_than_clusters_before_the_library_loads(entry, monkeypatch):
    """sklearn's ValueError, in its words, with no GPU and no library: the Lloyd kernels' relocation would run out of points."""
    import torch
    from autourdf_amd import _lib, ops

    def no_load(*a, **k):
        raise AssertionError("the library was loaded before the shapes were checked")
    monkeypatch.setattr(_lib, "load", no_load)
    X, init = torch.zeros(3, 3, dtype=torch.float64), torch.zeros(5, 3, dtype=torch.float64)
    with pytest.raises(ValueError, match=r"n_samples=3 should be >= n_clusters=5\."):
        if entry == "kmeans_lloyd_batch":
            ops.kmeans_lloyd_batch([torch.zeros(8, 3, dtype=torch.float64), X], [init, init])
        else:
            getattr(ops, entry)(X, init)
    with pytest.raises(ValueError, match=r"n_samples=3 should be >= n_clusters=5\."):
        R.k_means(X.numpy(), init.numpy())
