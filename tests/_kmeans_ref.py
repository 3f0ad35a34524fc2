"""Plain numpy restatement of sklearn.cluster.k_means(X, init=<array>, n_init=1, max_iter, tol) in any dimension, the table of
edge cases the Lloyd kernels (csrc/kmeans.hip, csrc/kmeans_nd.hip) are run at, and the bounds they are held to.

The restatement follows scikit-learn's dense Lloyd path step by step (_kmeans.py: centring by the mean, _tolerance, the loop
of _kmeans_single_lloyd with its two stops and the final E-step; _k_means_common.pyx: _relocate_empty_clusters_dense,
_average_centers, _center_shift) with no GPU, no C and no BLAS trick in it, and it reports its own conditioning: how close
any decision it took came to going the other way.  A kernel can only be asked to reproduce a decision that is not a coin toss
in float64, so the tests REQUIRE a margin from every case that is not exact arithmetic (test_kmeans_edges_cpu.py) and an
exact case to give the same bits in np.longdouble.

Where scikit-learn leaves an order open -- np.argpartition among equal distances in the relocation -- the restatement takes the
kernels' documented rule: descending distance, ties to the lower index."""
import functools
from types import SimpleNamespace

import numpy as np

EPS = 2.0 ** -52


def k_means(X, init, max_iter=300, tol=1e-4, dtype=np.float64, ties_to_higher_index=False, chunk=4096):
    """Returns a namespace: centers (k,d), labels (n) int32, inertia, n_iter, counts (k) int64 of the returned labels, and
       label_gap    smallest (d2 - d1) / d2 over all points of all E-steps (the final one included), d1 <= d2 the two smallest
                    squared distances of the point to DIFFERENT centres (inf when there is one; 0 for an exact tie).  Centres
                    with the same bits -- duplicate seeds, an empty cluster that took the heaviest one's centre -- are one
                    centre here: they give every point the same distance bits in any arithmetic, and the lower index wins;
       shift_margin smallest |shift - tol_abs| / tol_abs over the iterations that evaluated the shift test (tol_abs = 0: a
                    positive shift is infinitely far from it, a zero shift meets it exactly: margin 0);
       reloc_tie    a relocation had, among its n_empty + 1 largest distances, two equal ones of rows that are not identical
                    (copies of one row are interchangeable: the centres see coordinates, and a relocation changes no label);
       relocations / relocations_skipped  passes that moved points / that found the largest distance 0;
       still_empty  an iteration ended with an empty cluster taking the heaviest cluster's centre.
    ties_to_higher_index flips the relocation's tie rule (to show that a tie is harmless: both rules give one result)."""
    X = np.array(X, dtype=dtype)
    C = np.array(init, dtype=dtype)
    n, dim = X.shape
    k = len(C)
    if n < k:
        raise ValueError(f"n_samples={n} should be >= n_clusters={k}.")
    mean = X.mean(axis=0)
    tol_abs = np.mean(np.var(X, axis=0)) * dtype(tol)
    X = X - mean
    C = C - mean
    x2 = (X * X).sum(axis=1)
    rows = np.arange(n)
    out = SimpleNamespace(label_gap=np.inf, shift_margin=np.inf, reloc_tie=False, relocations=0, relocations_skipped=0,
                          still_empty=False)

    def e_step(C):
        labels = np.empty(n, np.int64)
        c2 = (C * C).sum(axis=1)
        Cu = np.unique(C, axis=0)                                     # the gap is taken between DIFFERENT centres (see label_gap)
        cu2 = (Cu * Cu).sum(axis=1)
        for a in range(0, n, chunk):
            D = c2[None, :] - 2 * (X[a:a + chunk] @ C.T)             # |x|^2 left out, as sklearn does: the same argmin
            lab = np.argmin(D, axis=1)                                # first minimum wins
            labels[a:a + chunk] = lab
            if len(Cu) > 1:
                Du = cu2[None, :] - 2 * (X[a:a + chunk] @ Cu.T)
                two = np.partition(Du, 1, axis=1)[:, :2] + x2[a:a + chunk, None]
                gap = np.where(two[:, 1] > 0, (two[:, 1] - two[:, 0]) / np.where(two[:, 1] > 0, two[:, 1], 1), 0)
                out.label_gap = min(out.label_gap, float(gap.min()))
        return labels

    labels_old = np.full(n, -1, np.int64)
    strict = False
    for it in range(max_iter):
        labels = e_step(C)
        sums = np.zeros((k, dim), dtype)
        np.add.at(sums, labels, X)
        w = np.bincount(labels, minlength=k).astype(dtype)
        empty = np.flatnonzero(w == 0)                                # fixed before anything moves
        if len(empty):
            t = X - C[labels]
            dist = (t * t).sum(axis=1)                                # to the OLD centres
            if dist.max() == 0:
                out.relocations_skipped += 1
            else:
                out.relocations += 1
                order = np.lexsort((-rows if ties_to_higher_index else rows, -dist))
                top = order[:len(empty) + 1]
                for p, q in zip(top[:-1], top[1:]):
                    if dist[p] == dist[q] and not (X[p] == X[q]).all():
                        out.reloc_tie = True
                for j, far in zip(empty, order):
                    old = labels[far]
                    sums[old] -= X[far]
                    sums[j] = X[far]
                    w[j] = 1
                    w[old] -= 1
        Cn = np.empty_like(C)
        heaviest = int(np.argmax(w))                                  # first cluster of maximal weight
        for j in range(k):
            if w[j] > 0:
                Cn[j] = sums[j] * (dtype(1) / w[j])
            else:
                Cn[j] = sums[heaviest] * (dtype(1) / w[heaviest])
                out.still_empty = True
        d = Cn - C
        shift = (np.sqrt((d * d).sum(axis=1)) ** 2).sum()             # sklearn squares the Euclidean shifts it stored
        C = Cn
        out.n_iter = it + 1
        if (labels == labels_old).all():
            strict = True
            break
        margin = abs(shift - tol_abs) / tol_abs if tol_abs > 0 else (np.inf if shift > 0 else 0.0)
        out.shift_margin = min(out.shift_margin, float(margin))
        if shift <= tol_abs:
            break
        labels_old = labels
    if not strict:
        labels = e_step(C)
    t = X - C[labels]
    out.inertia = (t * t).sum()
    out.centers = C + mean
    out.labels = labels.astype(np.int32)
    out.counts = np.bincount(labels, minlength=k)
    return out


# ---------------------------------------------------------------------------------------------------------------- the bounds
def center_bound(X):
    """1e-11 + n * 2^-52 * max|X - mean|: the standard bound of an n-term float64 sum."""
    X = np.asarray(X, np.float64)
    return 1e-11 + len(X) * EPS * float(np.abs(X - X.mean(axis=0)).max())


def inertia_bound(X, inertia):
    """1e-10 relative, with the floor 16 n (2^-52 max|X - mean|)^2 an inertia of (nearly) zero needs."""
    X = np.asarray(X, np.float64)
    return 1e-10 * abs(float(inertia)) + 16 * len(X) * (EPS * float(np.abs(X - X.mean(axis=0)).max())) ** 2


# ------------------------------------------------------------------------------------------------------------ the case table
def _normal(n, dim, seed):
    return np.random.default_rng(seed).normal(size=(n, dim))


def _stop(max_iter, tol):
    def build(dim):
        X = _normal(500, dim, 100 + dim)
        return X, X[:7].copy(), max_iter, tol
    return build


def _n1k1(dim):
    X = np.array([[0.5, -1.25, 2.0, 0.75, -0.5, 3.0][:dim]])
    return X, X.copy(), 300, 1e-4


def _n5k5(dim):
    X = _normal(5, dim, 200 + dim)
    return X, X[::-1].copy(), 300, 1e-4


def _n9k9(dim):
    X = _normal(9, dim, 210 + dim)
    init = X.copy()
    init[:7] += 50.0                                                  # seven seeds own nothing: 7 of the 9 points are relocated
    return X, init, 300, 1e-4


def _n300k128(dim):
    X = _normal(300, dim, 220 + dim)
    init = X[:128].copy()
    init[100:] += 40.0
    return X, init, 300, 1e-4


def _boundary(n):
    def build(dim):
        X = _normal(n, dim, 230 + dim)
        init = X[:128].copy()
        init[-4:] += 40.0
        return X, init, 8, 1e-4
    return build


def _allsame(tol):
    def build(dim):
        X = np.tile(np.array([0.5, -1.25, 2.0, 0.75, -0.5, 3.0][:dim]), (50, 1))
        return X, X[:3].copy(), 300, tol
    return build


_A6, _B6 = np.array([0.5, -0.25, 1.0, 0.75, -1.5, 0.25]), np.array([2.5, 1.75, -0.5, -0.25, 0.5, 1.25])


def _twopts(order):
    """Two dyadic points, 32 interleaved copies each; seeds: each point + 0.125 (near) and the first + 5, the second - 7 (far, own
    nothing), in `order` (0 1: near a, near b; 2 3: far a, far b).  Every sum, mean and product here is exact in float64."""
    def build(dim):
        a, b = _A6[:dim], _B6[:dim]
        X = np.empty((64, dim))
        X[0::2], X[1::2] = a, b
        seeds = np.array([a + 0.125, b + 0.125, a + 5.0, b - 7.0])
        return X, seeds[list(order)].copy(), 300, 1e-4
    return build


def _offset(dim):
    X = _normal(500, dim, 100 + dim) + np.array([1e4, -1e4, 1e3, 0, 0, 0][:dim])
    return X, X[:7].copy(), 300, 1e-4


def _outlier(tol):
    def build(dim):
        X = _normal(500, dim, 100 + dim)
        X[0] = 0.0
        X[0, 0] = 1e6                                                 # seeded as its own cluster (init row 0)
        return X, X[:7].copy(), 300, tol
    return build


def _emptied_later(dim):
    """A one-point cluster whose point is the farthest of all, listed AFTER two seeds that own nothing: the relocation takes
    the point and empties the cluster behind its back.  The list of empty clusters is fixed before anything moves, so the emptied
    cluster is not refilled in that pass: it takes the heaviest cluster's centre and is relocated in the next iteration.  (The
    heaviest cluster comes before it: scikit-learn 1.7.2 hands a still-empty cluster that comes BEFORE the heaviest one that
    cluster's not yet averaged sum, which no kernel here follows and no case here meets.)"""
    X = _normal(500, dim, 100 + dim)
    X[0] = 0.0
    X[0, 0] = 40.0
    lone = np.zeros((1, dim))
    lone[0, 0] = 30.0                                                 # the outlier is 10 away from its seed, all others nearer
    return X, np.vstack([X[6:8] + 1e3, X[1:6], lone]), 300, 1e-4


def _ties(seed_x):
    """Four dyadic locations x in {0, 1, 2, 5}, y = 0.25, 16 interleaved copies each.  Seeds at x = 0 and x = 2: the points at x = 1
    tie in iteration 1 and, the centres having moved to 0.5 and 3.5, the points at x = 2 in iteration 2; first minimum wins."""
    def build(dim):
        X = np.zeros((64, dim))
        X[:, 0] = np.tile([0.0, 1.0, 2.0, 5.0], 16)
        X[:, 1] = 0.25
        init = np.zeros((len(seed_x), dim))
        init[:, 0] = seed_x
        init[:, 1] = 0.25
        return X, init, 300, 1e-4
    return build


def _case(name, build, sklearn=True, exact=False, benign_tie=False):
    return SimpleNamespace(name=name, build=build, sklearn=sklearn, exact=exact, benign_tie=benign_tie)


# sklearn: comparable with live scikit-learn.  exact: dyadic data whose sums, means and products are exact in float64, so its ties
# and zero margins are decisions, not coin tosses (asserted: np.longdouble gives the same labels, n_iter and, rounded to float64,
# centres).  benign_tie: the one sklearn-comparable case whose relocation has a tie between different rows -- both relocated seeds
# land on a location that a lower cluster already holds, end empty and take cluster 0's centre, whichever of the tied points they
# were given (asserted: both tie rules give one result).
# NOT comparable with sklearn, held to the restatement only: its np.argpartition picks among equal distances arbitrarily, and
#   * in the twopts orderings that list a far seed before a near one the pick decides which cluster ends where;
#   * in ties_duplicate_seeds the third relocation (iteration 3, one empty cluster) finds the points at x = 0 and x = 1 equally far
#     (0.25) from their centre at x = 0.5, and the pick is the duplicate seed's final centre.
CASES = [
    _case("stop_iter1", _stop(1, 1e-4)),
    _case("stop_iter2", _stop(2, 1e-4)),
    _case("stop_iter5_tol0", _stop(5, 0.0)),
    _case("stop_strict_tol0", _stop(300, 0.0)),
    _case("stop_default", _stop(300, 1e-4)),
    _case("stop_large_tol", _stop(300, 0.5)),
    _case("n1_k1", _n1k1, exact=True),
    _case("n5_k5_reversed", _n5k5),
    _case("n9_k9_far7", _n9k9),
    _case("n300_k128_far28", _n300k128),
    _case("n16384_k128", _boundary(16384)),
    _case("n16385_k128", _boundary(16385)),
    _case("allsame", _allsame(1e-4), exact=True),
    _case("allsame_tol0", _allsame(0.0), exact=True),
    _case("twopts_near_first", _twopts((0, 1, 2, 3)), exact=True, benign_tie=True),
    _case("twopts_far_first", _twopts((2, 3, 0, 1)), sklearn=False, exact=True),
    _case("twopts_far_near_far_near", _twopts((2, 0, 3, 1)), sklearn=False, exact=True),
    _case("twopts_far_b_first", _twopts((3, 1, 0, 2)), sklearn=False, exact=True),
    _case("offset", _offset),
    _case("outlier", _outlier(1e-4)),
    _case("outlier_tol0", _outlier(0.0)),
    _case("emptied_later", _emptied_later),
    _case("ties_two_seeds", _ties((0.0, 2.0)), exact=True),
    _case("ties_duplicate_seeds", _ties((0.0, 2.0, 2.0, 0.0)), sklearn=False, exact=True),
]
CASE_NAMES = [c.name for c in CASES]
BY_NAME = {c.name: c for c in CASES}
DIMS = (3, 6)
BATCH_CASES = ("ties_duplicate_seeds", "twopts_near_first", "twopts_far_first")       # one launch: n = 64, k = 4, dim 3


@functools.lru_cache(maxsize=None)
def reference(name, dim):
    """(X, init, max_iter, tol, restatement result) of one case, computed once per session; callers must not write into it."""
    X, init, max_iter, tol = BY_NAME[name].build(dim)
    ref = k_means(X, init, max_iter, tol)
    for a in (X, init, ref.centers, ref.labels, ref.counts):
        a.setflags(write=False)
    return X, init, max_iter, tol, ref
