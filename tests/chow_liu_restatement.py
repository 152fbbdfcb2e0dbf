"""The reference's categorical Chow-Liu learner (cirkit/templates/region_graph/algorithms/chow_liu.py:80-151) restated in
fp64 numpy, independent of the product code: the joint counts as the Gram matrix of the one-hot encoding, the Laplace
smoothing, the rule for the diagonal, and the scipy calls that turn the matrix into a rooted tree."""
import numpy as np


def joint_counts(data: np.ndarray, num_categories: int) -> np.ndarray:
    """(D, D, C, C) int64: counts[i, j, a, b] = #{n : x[n, i] = a, x[n, j] = b}."""
    x = np.asarray(data, dtype=np.int64)
    n, d = x.shape
    onehot = np.zeros((n, d, num_categories), dtype=np.int64)
    onehot[np.arange(n)[:, None], np.arange(d)[None, :], x] = 1
    flat = onehot.reshape(n, d * num_categories)
    gram = flat.T @ flat
    return gram.reshape(d, num_categories, d, num_categories).transpose(0, 2, 1, 3).copy()


def mutual_information(data: np.ndarray, num_categories: int | None = None, alpha: float = 0.01) -> np.ndarray:
    """(D, D) float64.  joint = (count + alpha) / (N + C^2 alpha); the marginal of a column is read off the diagonal of its
    own block, (count + C alpha) / (N + C^2 alpha); MI[i, j] = sum_ab joint (log joint - log m_i(a) m_j(b)) over ALL C^2
    cells (empty ones included); the diagonal is 0."""
    x = np.asarray(data, dtype=np.int64)
    n, d = x.shape
    c = int(x.max()) + 1 if num_categories is None else int(num_categories)
    counts = joint_counts(x, c)
    denom = n + c * c * alpha
    marg_counts = np.stack([np.diag(counts[i, i]) for i in range(d)])  # (D, C)
    marg = (marg_counts + c * alpha) / denom
    joint = (counts + alpha) / denom
    log_indep = np.log(marg)[:, None, :, None] + np.log(marg)[None, :, None, :]
    mi = (joint * (np.log(joint) - log_indep)).sum(axis=(2, 3))
    np.fill_diagonal(mi, 0.0)
    return mi


def tree_of(mi: np.ndarray, root: int | None = None) -> np.ndarray:
    """Predecessors (-1 at the root) of the maximum spanning tree of `mi`, rooted at the vertex of least eccentricity."""
    from scipy.sparse import csgraph

    mst = csgraph.minimum_spanning_tree(-(np.asarray(mi) + 1.0), overwrite=True)
    if root is None:
        dist = csgraph.dijkstra(abs(mst).todense(), directed=False, return_predecessors=False)
        root = int(np.argmin(np.max(dist, axis=1)))
    _, pred = csgraph.breadth_first_order(mst, directed=False, i_start=root, return_predecessors=True)
    pred[root] = -1
    return pred


def edges_of(pred) -> set:
    return {frozenset((v, int(p))) for v, p in enumerate(pred) if p >= 0}


def asymmetric_data(rng, n: int, d: int, c: int) -> np.ndarray:
    """Column j + 1 is column j plus one (mod C) on most rows: counts[i, j] != counts[i, j].T, so an exchange of rows and
    columns shows."""
    x = np.zeros((n, d), dtype=np.int64)
    x[:, 0] = rng.integers(0, c, n)
    for j in range(1, d):
        keep = rng.random(n) < 0.8
        x[:, j] = np.where(keep, (x[:, j - 1] + 1) % c, rng.integers(0, c, n))
    return x


def noisy_chain(rng, d: int, c: int, n: int):
    """A Markov chain over a shuffled variable order: each variable copies its predecessor with probability 0.7 and is
    uniform otherwise.  Returns the data and the chain's edge set."""
    order = rng.permutation(d)
    x = np.zeros((n, d), dtype=np.int64)
    x[:, order[0]] = rng.integers(0, c, n)
    for a, b in zip(order[:-1], order[1:]):
        copy = rng.random(n) < 0.7
        x[:, b] = np.where(copy, x[:, a], rng.integers(0, c, n))
    return x, {frozenset((int(a), int(b))) for a, b in zip(order[:-1], order[1:])}


CHAIN_CASES = [(12, 5, 257), (6, 40, 513), (70, 2, 300)]  # (D, C, N), drawn one after the other from default_rng(3)


def chain_cases():
    rng = np.random.default_rng(3)
    return [(dcn, *noisy_chain(rng, *dcn)) for dcn in CHAIN_CASES]
