"""CPU: the families of tests/_normals_edges.py reach the decisions of csrc/normals.hip they are built for, the float64
restatement of its solver is measured against numpy.linalg.eigvalsh (the figures the GPU bounds of test_gpu_normals_edges.py are
taken from), and the oracle the GPU lists are compared with is itself checked on the tie-heavy inputs."""
import functools

import numpy as np

import _normals_edges as E


@functools.lru_cache(maxsize=None)
def _restated():
    """Every list case through the oracle's lists and the restatement: {family: (largest excess, largest | |n| - 1 |)}, the
    branches reached, and the per-case (label, normals, expected axes or None) of the diagonal families."""
    from oracle import normals as onrm
    fam, reached, diag = {}, set(), []
    for label, P, radius, max_nn in E.all_list_cases():
        idx, cnt = E.pad_lists(onrm.hybrid_neighbours(P, radius, max_nn), max_nn)
        N, taken = E.kernel_normals(P, idx, cnt)
        reached |= set().union(*taken)
        excess, identical = E.rayleigh_excess(P, idx, cnt, N)
        use = (cnt >= 3) & ~identical
        f = E.family_of(label)
        ex, un = fam.get(f, (0.0, 0.0))
        fam[f] = (max(ex, float(excess[use].max()) if use.any() else 0.0),
                  max(un, float(np.abs(np.linalg.norm(N, axis=1) - 1).max())))
        assert np.isfinite(N).all(), label
        assert (N[cnt < 3] == [0.0, 0.0, 1.0]).all(), label
        if f in E.DIAGONAL_FAMILIES:
            diag.append((label, N, E.diagonal_expected(P, idx, cnt), taken))
    return fam, reached, diag


def test_families_reach_every_solver_branch():
    _, reached, _ = _restated()
    reached = reached - {"cnt<3"}
    # the two that need an exact eigenvalue are reached by constructed inputs: A = diag(1, 1, 2) has the double eigenvalue 1
    A = [1.0, 0.0, 0.0, 1.0, 0.0, 2.0]
    t = set()
    assert E.eigvec_by_rows(A, 1.0, t) == [0.0, 0.0, 0.0] and t == {"dm==0"}          # A - I has rank 1: every cross product is 0
    t = set()
    v = E.eigvec_deflated(A, [0.0, 0.0, 1.0], 1.0, t)                                  # the 2x2 block is exactly 0: any vector does
    assert "cu1_a00" in t and v == [0.0, 1.0, 0.0]
    assert reached.isdisjoint(E.CONSTRUCTED_ONLY) and reached.isdisjoint(E.UNREACHABLE)  # (the lists in the helper stay honest)
    assert reached | set(E.CONSTRUCTED_ONLY) | set(E.UNREACHABLE) == set(E.BRANCHES), set(E.BRANCHES) - reached
    # cu1_a11 cannot be taken: no real 2x2 block enters the else arm with a11 = 0
    rng = np.random.default_rng(0)
    for _ in range(2000):
        S = rng.normal(size=(3, 3)) * 10.0 ** rng.integers(-8, 1, size=(3, 1))
        S = S @ S.T
        _, t = E.smallest_eigvec([S[0, 0], S[0, 1], S[0, 2], S[1, 1], S[1, 2], S[2, 2]])
        assert "cu1_a11" not in t


def test_restatement_rayleigh_excess_per_family():
    """Unit length to 1e-12 and the Rayleigh excess (n^T C n - l0) / lmax of the restatement, C in extended precision from
    centred coordinates, l from eigvalsh: every family's figure is the one recorded in _normals_edges.MEASURED_EXCESS (not above
    it, and the record not more than twice the measurement, wherever 16 x the figure is above the floor of the GPU bound)."""
    fam, _, _ = _restated()
    assert set(fam) == set(E.MEASURED_EXCESS)
    for f, (excess, unit) in sorted(fam.items()):
        print(f"{f:14s} excess {excess:.3e}  recorded {E.MEASURED_EXCESS[f]:.1e}  gpu bound {E.gpu_bound(f):.2e}  | |n|-1 | {unit:.1e}")
    for f, (excess, unit) in fam.items():
        assert unit <= 1e-12, (f, unit)
        assert excess <= max(E.MEASURED_EXCESS[f], E.BOUND_FLOOR / 16), (f, excess)
        assert 16 * E.MEASURED_EXCESS[f] <= max(32 * excess, E.BOUND_FLOOR), (f, excess)


def test_restatement_on_exactly_diagonal_covariances():
    """Axis-aligned symmetric boxes: the restatement takes the diagonal branch for every point and returns the axis of the
    smallest extent -- z whenever z is among the smallest, y when only x and y tie -- and never an axis of the largest."""
    _, _, diag = _restated()
    seen = set()
    for label, N, want, taken in diag:
        assert all(t == {"diagonal"} for t in taken), label
        assert (N == want).all(), label
        seen |= {tuple(w) for w in want}
    assert seen == {(1.0, 0.0, 0.0), (0.0, 1.0, 0.0), (0.0, 0.0, 1.0)}


def _rows_sorted(P):
    d2 = ((P[:, None, :] - P[None, :, :]) ** 2).sum(-1)
    return d2, np.sort(d2, axis=1)


def test_oracle_lists_on_tie_lattices():
    """oracle.normals.hybrid_neighbours on the lattices: distances non-decreasing, indices increasing within equal distances,
    nothing at d^2 == r^2 (or beyond) inside, nothing better left outside -- and the inputs do contain the ties: inside the
    lists, at the max_nn-th / (max_nn+1)-th boundary, and at exactly the radius."""
    from oracle import normals as onrm
    inner = boundary = at_radius = 0
    for label, P, radius, max_nn in E.tie_cases():
        d2, srt = _rows_sorted(P)
        assert (d2 * 64 == np.round(d2 * 64)).all()                               # exact: whole multiples of (1/8)^2
        r2 = radius * radius if radius > 0 else np.inf
        if radius > 0:
            assert r2 * 64 == round(r2 * 64)
            at_radius += int((d2 == r2).sum())
        ref = onrm.hybrid_neighbours(P, radius, max_nn)
        for i, row in enumerate(ref):
            d = d2[i, row]
            assert len(row) == min(max_nn, int((d2[i] < r2).sum())), label
            assert (d < r2).all() and (np.diff(d) >= 0).all(), label
            tied = np.diff(d) == 0
            assert (np.diff(row)[tied] > 0).all(), label
            inner += int(tied.sum())
            out = np.ones(len(P), bool)
            out[row] = False
            if len(row) == max_nn and out.any():                                  # what stayed outside is not better than the last one in
                j = np.nonzero(out)[0]
                assert ((d2[i, j] > d[-1]) | ((d2[i, j] == d[-1]) & (j > row[-1]))).all(), label
            if len(row) == max_nn and max_nn < len(P) and srt[i, max_nn] == d[-1] and srt[i, max_nn] < r2:
                boundary += 1                                                      # the tie decides who is in
    assert inner > 100000 and boundary > 5000 and at_radius > 10000, (inner, boundary, at_radius)


def test_oracle_lists_with_duplicated_points():
    """More copies of a point than max_nn: the list holds the lowest-indexed copies and need not contain the query."""
    from oracle import normals as onrm
    label, P, radius, max_nn = next(c for c in E.duplicate_cases() if c[3] == 30 and c[2] < 0)
    ref = onrm.hybrid_neighbours(P, radius, max_nn)
    without_self = [i for i, row in enumerate(ref) if i not in row]
    assert len(without_self) >= 8 * (31 - 30) + 8 * (40 - 30)
    for i in without_self:
        same = np.nonzero((P == P[i]).all(1))[0]
        assert (ref[i] == same[:max_nn]).all()


def test_oracle_orients_convex_surfaces_outward():
    from oracle import normals as onrm
    for name, P, outward in E.surface_cases():
        _, N = onrm.point_features(P)
        cos = (N * outward).sum(1)
        print(name, "outward", (cos > 0).mean(), "smallest cosine", cos.min())
        assert (cos > 0).all(), (name, (cos > 0).mean())
