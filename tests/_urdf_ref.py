"""numpy / scipy restatement of the reference's link discovery (coord_map.py:70-128) for the GPU tests: the float64
threshold lattice by repeated subtraction, components of {(i, j) : i < j, d[i, j] < t} straight from the map (no MST),
numbered by smallest node, and scikit-learn's precomputed silhouette written out.  Independent of the kernel's
method; needs neither networkx nor scikit-learn."""
import numpy as np
from scipy.sparse import csr_matrix
from scipy.sparse.csgraph import connected_components

STEP = 0.0001
# t_0 = 1, t_{k+1} = fl(t_k - 1e-4): ufunc accumulate subtracts sequentially, exactly the reference's loop
LATTICE = np.subtract.accumulate(np.concatenate([[1.0], np.full(10100, STEP)]))


def components(d, t):
    K = len(d)
    n, lab = connected_components(csr_matrix(np.triu(d < t, 1)), directed=False)
    first = {}
    for i in range(K):                                       # renumber by smallest node
        first.setdefault(lab[i], len(first))
    return n, np.array([first[x] for x in lab])


def clustering(d, nl):
    """(threshold t_k, labels) of coord_clustering(K, d, nl): the first lattice point with >= nl components."""
    lo, hi = 0, len(LATTICE) - 1                             # component count is non-decreasing along the lattice
    while lo < hi:
        mid = (lo + hi) // 2
        if components(d, LATTICE[mid])[0] >= nl:
            hi = mid
        else:
            lo = mid + 1
    return LATTICE[lo], components(d, LATTICE[lo])[1]


def silhouette(d, labels):
    """sklearn.metrics.silhouette_score(d, labels, metric='precomputed'); None where sklearn raises ValueError."""
    K = len(d)
    nc = labels.max() + 1
    if not 1 < nc < K:
        return None
    freq = np.bincount(labels, minlength=nc)
    sums = np.array([np.bincount(labels, weights=d[i], minlength=nc) for i in range(K)])
    intra = sums[np.arange(K), labels].copy()
    sums[np.arange(K), labels] = np.inf
    inter = (sums / freq).min(axis=1)
    with np.errstate(divide="ignore", invalid="ignore"):
        intra /= freq[labels] - 1
        s = (inter - intra) / np.maximum(intra, inter)
    return float(np.mean(np.nan_to_num(s * (freq[labels] > 1))))


def random_map(K, seed, symmetric=True):
    rng = np.random.default_rng(seed)
    x = rng.normal(size=(K, 3)) * rng.uniform(0.2, 2.0, size=(1, 3))
    d = np.sqrt(((x[:, None] - x[None]) ** 2).sum(-1))
    if not symmetric:
        d = d * rng.uniform(0.9, 1.1, size=d.shape)
        np.fill_diagonal(d, 0)
    return (d - d.min()) / (d.max() - d.min())


# ------------------------------------------------------------------------------------------ maps real sequences produce
# Summed maps are not normalised (weights above 1 occur) and tie exactly (identical tracks are at distance exactly 0).
def binade_crossings(n_cross=2):
    """[n, n + 1] for the first n_cross binade crossings of the lattice: LATTICE[n] >= 2^-b > LATTICE[n + 1]."""
    out = []
    for b in range(1, n_cross + 1):
        n = int(np.nonzero(LATTICE >= 2.0 ** -b)[0][-1])
        out += [n, n + 1]
    return out


def lattice_weights():
    """LATTICE[n] and its two float64 neighbours for n in different binades and either side of two binade crossings."""
    ns = [1, 1234, 5000, 9999] + binade_crossings()
    return [w for n in ns for w in (LATTICE[n], np.nextafter(LATTICE[n], np.inf), np.nextafter(LATTICE[n], -np.inf))]


def block_map(K, chain, far, seed):
    """g = len(chain) + 1 groups of identical tracks (distance exactly 0 inside a group, nodes of a group scattered over
    0..K-1); groups a and a + 1 are chain[a] apart and every other pair of groups `far` (>= max(chain)), so the MST
    weights are K - g zeros and exactly the chain weights: ties among them make the component count jump."""
    g = len(chain) + 1
    assert g <= K and far >= max(chain)
    rng = np.random.default_rng(seed)
    grp = rng.permutation(np.concatenate([np.arange(g), rng.integers(0, g, K - g)]))
    W = np.full((g, g), float(far))
    for a, w in enumerate(chain):
        W[a, a + 1] = W[a + 1, a] = w
    np.fill_diagonal(W, 0.0)
    return W[grp[:, None], grp[None]], grp


def unsymmetric(d):
    """Upper triangle scaled by 1 + 2^-40: link discovery reads i < j only."""
    return np.where(np.arange(len(d))[:, None] < np.arange(len(d))[None], d * (1 + 2.0 ** -40), d)


def above_one_map(K, seed, every):
    """An unnormalised map: off-diagonal weights in [0, 3] (every = False) or all above 1 (every = True)."""
    d = random_map(K, seed)
    off = ~np.eye(K, dtype=bool)
    return np.where(off, 1.001 + d, 0.0) if every else 3.0 * d
