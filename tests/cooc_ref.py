"""fp64 / int64 numpy reference of the item co-occurrence top-k (include/tagrec.h, csrc/cooc.hip), restated literally:

    c_ij = |N(i) n N(j)| (common users), c_ii = deg(i) -- zero_diagonal: c_ii counts as 0;  D_i = sum_j c_ij
    candidates of row i: every j with c_ij > 0, in descending fp64 key c_ij^2 / (D_j + 1), ties to the lower id
    nbr_id [n_item, k] int32: the first k, padded with -1;  nbr_w = c_ij sqrt(D_i + 1) / D_i / sqrt(D_j + 1) in fp64, 0 at pads

The counts are formed user by user with integer additions (no scipy): row i of A^T A is the sum of the item lists of i's users.
"""
import numpy as np


def unique_edges(edges, n_item):
    """[E, 2] int64 (user, item), sorted by (user, item), duplicates gone."""
    e = np.asarray(edges, dtype=np.int64).reshape(-1, 2)
    key = np.unique(e[:, 0] * np.int64(n_item) + e[:, 1])
    return np.stack([key // n_item, key % n_item], axis=1)


def zipf_edges(n_user, n_item, n_draw, alpha=0.8, seed=0):
    """Users uniform, items Zipf(alpha) over a random permutation of the ids, n_draw draws -> the unique edges [E, 2]."""
    rng = np.random.RandomState(seed)
    w = np.arange(1, n_item + 1, dtype=np.float64) ** (-alpha)
    perm = rng.permutation(n_item)
    u = rng.randint(0, n_user, size=n_draw)
    i = perm[rng.choice(n_item, size=n_draw, p=w / w.sum())]
    return unique_edges(np.stack([u, i], axis=1), n_item)


def small_graph():
    """64 users x 40 items, Zipf 0.8, seed 0, the least popular item emptied: an item without users (an all-pad row) and rows
    with fewer than 8 candidates.  -> (edges, n_user, n_item)"""
    e = zipf_edges(64, 40, 300, 0.8, 0)
    deg = np.bincount(e[:, 1], minlength=40)
    return e[e[:, 1] != int(np.argmin(deg))], 64, 40


def large_graph():
    """2 000 users x 3 000 items, Zipf 0.8, seed 0, 60 000 draws (about 56 000 unique edges): D_i reaches about 43 000 and a
    few dozen items lie above 4 096, so the default split uses both tiers.  -> (edges, n_user, n_item)"""
    return zipf_edges(2000, 3000, 60000, 0.8, 0), 2000, 3000


def lists(edges, n_user, n_item):
    """(items of every user, users of every item) as lists of sorted int64 arrays."""
    e = unique_edges(edges, n_item)
    by_u = [[] for _ in range(n_user)]
    by_i = [[] for _ in range(n_item)]
    for u, i in e:
        by_u[u].append(i)
        by_i[i].append(u)
    return [np.asarray(x, np.int64) for x in by_u], [np.asarray(x, np.int64) for x in by_i]


def count_rows(edges, n_user, n_item, zero_diagonal=False):
    """-> (rows: list of (ids int64 ascending, counts int64) per item, D int64 [n_item])."""
    by_u, by_i = lists(edges, n_user, n_item)
    rows, D = [], np.zeros(n_item, dtype=np.int64)
    for i in range(n_item):
        c = np.zeros(n_item, dtype=np.int64)
        for u in by_i[i]:
            c[by_u[u]] += 1
        if zero_diagonal:
            c[i] = 0
        ids = np.flatnonzero(c)
        rows.append((ids, c[ids]))
        D[i] = c.sum()
    return rows, D


def topk(edges, n_user, n_item, k, zero_diagonal=False):
    """-> (nbr_id int32 [n_item, k], nbr_w float64 [n_item, k], D int64 [n_item])."""
    rows, D = count_rows(edges, n_user, n_item, zero_diagonal)
    nbr_id = np.full((n_item, k), -1, dtype=np.int32)
    nbr_w = np.zeros((n_item, k), dtype=np.float64)
    for i, (ids, c) in enumerate(rows):
        if not len(ids):
            continue
        cf = c.astype(np.float64)
        key = (cf * cf) / (D[ids] + 1).astype(np.float64)
        order = np.lexsort((ids, -key))[:k]              # descending key, ties to the lower id
        j = ids[order]
        nbr_id[i, :len(j)] = j
        nbr_w[i, :len(j)] = cf[order] * np.sqrt(np.float64(D[i] + 1)) / np.float64(D[i]) / np.sqrt((D[j] + 1).astype(np.float64))
    return nbr_id, nbr_w, D
