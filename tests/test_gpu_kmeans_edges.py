"""GPU: the Lloyd kernels -- csrc/kmeans.hip's persistent VALU form, matrix-core form and one-workgroup batch form, csrc/kmeans_nd.hip's
N-D kernel with its labels in LDS and in the workspace -- against the plain float64 restatement of sklearn.cluster.k_means in
tests/_kmeans_ref.py, at the stop rules (max_iter 1, 2, mid-run; tol 0; a large tol), the sizes (n = 1, n = k, k = 128 on both sides of
the N-D kernel's label-buffer switch) and the degenerate data (identical points, more clusters than distinct points, exact distance
ties, a far frame, a far outlier, a cluster emptied by the relocation itself) of its case table.  test_kmeans_edges_cpu.py pins the
restatement to live scikit-learn and requires of every case the margins that make labels and n_iter a fair demand: they are compared
exactly, centres and inertia within the float64 bounds of an n-term sum."""
import ctypes
import functools

import numpy as np
import pytest
import torch

import _kmeans_ref as R

pytestmark = pytest.mark.gpu


@functools.lru_cache(maxsize=None)
def _gpu(entry, name, dim):
    """One run of a case through one entry, as numpy: (centres, labels, inertia, n_iter).  Shared by the tests that compare it."""
    from autourdf_amd import ops
    X, init, max_iter, tol, _ = R.reference(name, dim)
    Xd, Id = _dev(X), _dev(init)
    if entry == "nd":
        out = ops.kmeans_lloyd_nd(Xd, Id, max_iter=max_iter, tol=tol)
    else:
        out = ops.kmeans_lloyd(Xd, Id, max_iter=max_iter, tol=tol, use_mfma=entry == "mfma")
    return _host(out)


def _dev(a):
    return torch.from_numpy(a.copy()).cuda()                          # (the shared reference arrays are read-only)


def _host(out):
    c, lab, inertia, n_iter = out
    return c.cpu().numpy(), lab.cpu().numpy(), float(inertia.item()), int(n_iter.item())


def _assert_matches(out, name, dim, who):
    X, init, _, _, ref = R.reference(name, dim)
    c, lab, inertia, n_iter = out
    cerr, ierr = float(np.abs(c - ref.centers).max()), abs(inertia - float(ref.inertia))
    print(f"{who} {name} d{dim}: n_iter {n_iter} / {ref.n_iter}, labels differ {int((lab != ref.labels).sum())}, centres {cerr:.3e} "
          f"(bound {R.center_bound(X):.3e}), inertia {ierr:.3e} (bound {R.inertia_bound(X, ref.inertia):.3e})")
    assert n_iter == ref.n_iter
    np.testing.assert_array_equal(lab, ref.labels)
    np.testing.assert_array_equal(np.bincount(lab, minlength=len(init)), ref.counts)
    assert cerr <= R.center_bound(X)
    assert ierr <= R.inertia_bound(X, ref.inertia)


@pytest.mark.parametrize("dim", R.DIMS)
@pytest.mark.parametrize("name", R.CASE_NAMES)
def test_nd_kernel_matches_the_restatement(name, dim):
    """k_km_nd<3> and <6>; the boundary pair runs the labels-in-LDS form at its largest dynamic LDS (n = 16384, k = 128) and the
    labels-in-workspace form <3, true>, <6, true> one point above it."""
    _assert_matches(_gpu("nd", name, dim), name, dim, "nd")


@pytest.mark.parametrize("entry", ["valu", "mfma"])
@pytest.mark.parametrize("name", R.CASE_NAMES)
def test_lloyd_3d_matches_the_restatement(name, entry):
    _assert_matches(_gpu(entry, name, 3), name, 3, entry)


@pytest.mark.parametrize("name", R.CASE_NAMES)
def test_nd_kernel_at_dim3_and_the_3d_forms_agree_exactly(name):
    nd, valu, mfma = (_gpu(e, name, 3) for e in ("nd", "valu", "mfma"))
    for other in (valu, mfma):
        np.testing.assert_array_equal(nd[1], other[1])
        assert nd[3] == other[3]
    np.testing.assert_array_equal(valu[0], mfma[0])                   # (the two 3-D forms share the exact integer M-step)
    assert valu[2] == mfma[2]


def test_batch_entry_matches_the_restatement():
    """One launch of k_km_small, three problems of n = 64, k = 4: the exact ties with duplicate seeds and two orderings of the
    two-point frame (relocation in iteration 1, `largest distance is 0` and the heaviest cluster's centre afterwards)."""
    from autourdf_amd import ops
    refs = [R.reference(name, 3) for name in R.BATCH_CASES]
    assert len({(r[2], r[3]) for r in refs}) == 1
    outs = ops.kmeans_lloyd_batch([_dev(r[0]) for r in refs], [_dev(r[1]) for r in refs], max_iter=refs[0][2], tol=refs[0][3])
    for name, out in zip(R.BATCH_CASES, outs):
        _assert_matches(_host(out), name, 3, "batch")


@pytest.mark.parametrize("name", ["stop_iter2", "stop_large_tol", "n5_k5_reversed", "n9_k9_far7", "n300_k128_far28", "allsame",
                                  "offset", "outlier_tol0", "emptied_later"])
def test_batch_entry_single_problem_matches_the_restatement(name):
    """k_km_small alone on the cases of its size (n <= 16384, k <= 128, dim 3) that the three-problem launch above leaves out."""
    from autourdf_amd import ops
    X, init, max_iter, tol, _ = R.reference(name, 3)
    out, = ops.kmeans_lloyd_batch([_dev(X)], [_dev(init)], max_iter=max_iter, tol=tol)
    _assert_matches(_host(out), name, 3, "batch")


SENTINEL_F, SENTINEL_I, SENTINEL_B = -12345.5, -77, 0xAB


@pytest.mark.parametrize("entry", ["lloyd_valu", "lloyd_mfma", "batch", "nd3", "nd6"])
def test_c_entry_points_refuse_fewer_points_than_clusters(entry):
    """n = 3 < k = 5 with valid buffers straight through the C ABI (the torch wrappers refuse earlier): a nonzero status that names
    both numbers, and nothing launched -- outputs and workspace keep their sentinels."""
    from autourdf_amd import _lib
    L = _lib.load()
    n, k, dim = 3, 5, 6 if entry == "nd6" else 3
    dev = "cuda"
    X = torch.zeros(n, dim, dtype=torch.float64, device=dev)
    init = torch.ones(k, dim, dtype=torch.float64, device=dev)
    centers = torch.full((k, dim), SENTINEL_F, dtype=torch.float64, device=dev)
    labels = torch.full((n,), SENTINEL_I, dtype=torch.int32, device=dev)
    inertia = torch.full((1,), SENTINEL_F, dtype=torch.float64, device=dev)
    n_iter = torch.full((1,), SENTINEL_I, dtype=torch.int32, device=dev)
    ws_bytes = max(L.creg_kmeans_workspace_bytes(n, k), L.creg_kmeans_batch_workspace_bytes(n, k, 1), L.creg_kmeans_nd_workspace_bytes(n))
    ws = torch.full((ws_bytes,), SENTINEL_B, dtype=torch.uint8, device=dev)
    p = lambda t: ctypes.c_void_p(t.data_ptr())
    stream = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    if entry.startswith("lloyd"):
        rc = L.creg_kmeans_lloyd_f64(p(X), n, p(init), k, 300, 1e-4, int(entry == "lloyd_mfma"), p(centers), p(labels), p(inertia), p(n_iter),
                                     p(ws), ws_bytes, stream)
    elif entry == "batch":
        one = lambda t: (ctypes.c_void_p * 1)(t.data_ptr())
        rc = L.creg_kmeans_lloyd_batch_f64(one(X), n, one(init), k, 1, 300, 1e-4, one(centers), one(labels), one(inertia), one(n_iter),
                                           p(ws), ws_bytes, stream)
    else:
        rc = L.creg_kmeans_lloyd_nd_f64(p(X), n, dim, p(init), k, 300, 1e-4, p(centers), p(labels), p(inertia), p(n_iter), p(ws), ws_bytes, stream)
    msg = L.creg_last_error().decode()
    torch.cuda.synchronize()
    assert rc != 0
    assert "n_samples=3" in msg and "n_clusters=5" in msg, msg
    assert (centers == SENTINEL_F).all() and (inertia == SENTINEL_F).all()
    assert (labels == SENTINEL_I).all() and (n_iter == SENTINEL_I).all()
    assert (ws == SENTINEL_B).all()
