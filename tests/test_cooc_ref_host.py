"""CPU: the numpy reference of the co-occurrence top-k (tests/cooc_ref.py) against scipy.sparse's A^T A on a toy graph and
against a hand-worked 4-item example with mathematically tied keys; the config surface of UltraGCN."""
import numpy as np
import pytest

import cooc_ref as R


def _dense_ata(edges, n_user, n_item):
    sp = pytest.importorskip("scipy.sparse")
    e = R.unique_edges(edges, n_item)
    A = sp.csr_matrix((np.ones(len(e), np.int64), (e[:, 0], e[:, 1])), shape=(n_user, n_item))
    return np.asarray((A.T @ A).todense())


@pytest.mark.parametrize("zero_diagonal", [False, True])
def test_counts_and_D_match_scipy(zero_diagonal):
    nu, ni = 64, 40
    edges = R.zipf_edges(nu, ni, 330, 0.8, 0)
    C = _dense_ata(edges, nu, ni)
    if zero_diagonal:
        np.fill_diagonal(C, 0)
    rows, D = R.count_rows(edges, nu, ni, zero_diagonal)
    assert np.array_equal(D, C.sum(1))
    # the two integer identities of the issue
    by_u, by_i = R.lists(edges, nu, ni)
    deg_u = np.array([len(x) for x in by_u])
    want = np.array([deg_u[us].sum() - (len(us) if zero_diagonal else 0) for us in by_i])
    assert np.array_equal(D, want)
    for i, (ids, c) in enumerate(rows):
        assert np.array_equal(ids, np.flatnonzero(C[i])) and np.array_equal(c, C[i][ids])


@pytest.mark.parametrize("zero_diagonal", [False, True])
def test_topk_matches_a_sort_of_the_dense_product(zero_diagonal):
    nu, ni, k = 64, 40, 8
    edges = R.zipf_edges(nu, ni, 330, 0.8, 0)
    C = _dense_ata(edges, nu, ni).astype(np.float64)
    if zero_diagonal:
        np.fill_diagonal(C, 0)
    D = C.sum(1)
    nbr_id, nbr_w, Dref = R.topk(edges, nu, ni, k, zero_diagonal)
    assert np.array_equal(Dref, D.astype(np.int64))
    for i in range(ni):
        cand = [j for j in range(ni) if C[i, j] > 0]
        cand.sort(key=lambda j: (-(C[i, j] * C[i, j]) / (D[j] + 1), j))
        cand = cand[:k]
        assert nbr_id[i, :len(cand)].tolist() == cand and (nbr_id[i, len(cand):] == -1).all()
        w = [C[i, j] * np.sqrt(D[i] + 1) / D[i] / np.sqrt(D[j] + 1) for j in cand]
        assert np.array_equal(nbr_w[i, :len(cand)], np.array(w)) and (nbr_w[i, len(cand):] == 0).all()


# users: u0 = {0, 1}, u1 = u2 = {0, 2, 3}, u3 = u4 = u5 = {2, 3}
HAND = [(0, 0), (0, 1), (1, 0), (1, 2), (1, 3), (2, 0), (2, 2), (2, 3), (3, 2), (3, 3), (4, 2), (4, 3), (5, 2), (5, 3)]


def test_hand_worked_example_zero_diagonal():
    """c_01 = 1, c_02 = c_03 = 2, c_23 = 5, c_12 = c_13 = 0;  D = (5, 1, 7, 7).
    Row 0: the keys are 1 / 2 (item 1), 4 / 8 (item 2), 4 / 8 (item 3) -- a mathematical three-way tie between a count of 1
    and counts of 2, so the order is by id: 1, 2, 3 (an order by count, or by a rounded sqrt of the key, gives 2, 3, 1).
    Row 1: item 0 alone.  Row 2: 25 / 8 (item 3) before 4 / 6 (item 0).  Row 3: 25 / 8 (item 2) before 4 / 6 (item 0)."""
    nbr_id, nbr_w, D = R.topk(HAND, 6, 4, 3, zero_diagonal=True)
    assert D.tolist() == [5, 1, 7, 7]
    assert nbr_id.tolist() == [[1, 2, 3], [0, -1, -1], [3, 0, -1], [2, 0, -1]]
    s = np.sqrt
    want = [[1 * s(6.0) / 5 / s(2.0), 2 * s(6.0) / 5 / s(8.0), 2 * s(6.0) / 5 / s(8.0)],
            [1 * s(2.0) / 1 / s(6.0), 0, 0],
            [5 * s(8.0) / 7 / s(8.0), 2 * s(8.0) / 7 / s(6.0), 0],
            [5 * s(8.0) / 7 / s(8.0), 2 * s(8.0) / 7 / s(6.0), 0]]
    assert np.array_equal(nbr_w, np.array(want, dtype=np.float64))
    assert (1.0 * 1.0) / 2.0 == (2.0 * 2.0) / 8.0            # the tie is exact in fp64 too


def test_hand_worked_example_with_diagonal():
    """c_ii = deg(i) = (3, 1, 5, 5);  D = (8, 2, 12, 12).  Row 0: 9 / 9, 1 / 3, 4 / 13, 4 / 13 -> 0, 1, 2, 3.  Row 1: 1 / 3 (itself)
    before 1 / 9.  Rows 2 and 3: 25 / 13 twice (tie -> 2 before 3), then 4 / 9."""
    nbr_id, _, D = R.topk(HAND, 6, 4, 4, zero_diagonal=False)
    assert D.tolist() == [8, 2, 12, 12]
    assert nbr_id.tolist() == [[0, 1, 2, 3], [1, 0, -1, -1], [2, 3, 0, -1], [2, 3, 0, -1]]


def test_the_issue_graphs_have_the_stated_shape():
    """What the GPU tests rely on: pads in the small graph, both tiers in the large one."""
    e, nu, ni = R.small_graph()
    rows, D = R.count_rows(e, nu, ni)
    assert (nu, ni) == (64, 40) and (D == 0).sum() == 1 and sum(0 < len(ids) < 8 for ids, _ in rows) >= 3
    e, nu, ni = R.large_graph()
    by_u, by_i = R.lists(e, nu, ni)
    deg_u = np.array([len(x) for x in by_u])
    D = np.array([deg_u[us].sum() for us in by_i])
    assert D.max() > 40000 and 30 <= (D > 4096).sum() <= 60 and (D <= 4096).sum() > 2000


def test_ultragcn_config_surface():
    import tagrec_amd as T
    cfg = T.get_config("ultragcn")
    assert cfg["ug_w"] == (1e-6, 1.0, 1e-6, 1.0) and cfg["ug_negative_weight"] == 10.0 and cfg["ug_lambda"] == 1.0
    assert cfg["ug_neighbors"] == 10 and cfg["ug_zero_diagonal"] is False and cfg["n_negatives"] == 16
    assert T.get_config("ultragcn", ug_neighbors=0)["ug_neighbors"] == 0
    for bad in (dict(ug_neighbors=65), dict(ug_neighbors=-1), dict(ug_w=(1.0, 1.0)), dict(ug_w=(1.0, 1.0, -1.0, 1.0)),
                dict(ug_lambda=float("inf")), dict(ug_negative_weight=-1.0), dict(ug_zero_diagonal=1), dict(n_negatives=64),
                dict(mul_loss_func="softmax"), dict(mul_loss_func="softmax", negatives="in_batch", n_negatives=1),
                dict(mul_loss_func="softmax", softmax_over="catalogue", n_negatives=1)):
        with pytest.raises(T.TagrecError):
            T.get_config("ultragcn", **bad)
    for model in ("lightgcn", "ngcf", "simgcl", "directau", "ncl", "tgcn", "dgcf", "disengcn", "kgat"):
        with pytest.raises(T.TagrecError, match="ug_lambda"):
            T.get_config(model, ug_lambda=0.5)
