"""GPU: the item co-occurrence top-k (csrc/cooc.hip through tagrec_amd.item_cooccurrence_topk) against the fp64 / int64
reference of tests/cooc_ref.py.

nbr_id and D are compared for EXACT equality: the counts are integers, the key c^2 / (D + 1) is an IEEE fp64 division of two
exact operands on both sides, so even mathematically tied keys order the same.  nbr_w is one fp32 rounding of the fp64 value:
rtol 1e-6 (2^-24 = 6e-8 with margin; nothing else enters it).  Every case runs for both zero_diagonal values; every path
(LDS table / dense counter rows) is forced through lds_limit and workspace_bytes."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import tagrec_amd as T
from tagrec_amd import cooc

import cooc_ref as R

DEV = torch.device("cuda:0")
ZD = (False, True)
_REF = {}


def _ref(name, zd, k):
    """The reference of a named graph, computed once per (graph, zero_diagonal) at k = 64: a smaller k is its prefix."""
    key = (name, zd)
    if key not in _REF:
        e, nu, ni = getattr(R, name)()
        _REF[key] = (e, nu, ni) + R.topk(e, nu, ni, 64, zd)
    e, nu, ni, nid, nw, D = _REF[key]
    return e, nu, ni, nid[:, :k], nw[:, :k], D


def _run(e, nu, ni, k, zd, **kw):
    return T.item_cooccurrence_topk(np.asarray(e), nu, ni, k, zero_diagonal=zd, device=DEV, **kw)


def _check(got, nid, nw, D, what=""):
    g_id, g_w, g_D = (t.cpu().numpy() for t in got)
    assert g_id.dtype == np.int32 and g_w.dtype == np.float32 and g_D.dtype == np.int64
    assert np.array_equal(g_D, D), f"{what}: D differs"
    assert np.array_equal(g_id, nid), f"{what}: nbr_id differs in rows {np.flatnonzero((g_id != nid).any(1))[:8]}"
    assert (g_w[nid < 0] == 0).all()
    np.testing.assert_allclose(g_w, nw, rtol=1e-6, atol=0, err_msg=what)


def _same(a, b):
    return all(torch.equal(x, y) for x, y in zip(a[:1] + a[2:], b[:1] + b[2:])) and \
        torch.equal(a[1].view(torch.int32), b[1].view(torch.int32))


@pytest.mark.parametrize("zd", ZD)
def test_small_graph_with_pads(zd):
    e, nu, ni, nid, nw, D = _ref("small_graph", zd, 8)
    assert (nid[:, 0] == -1).any() and ((nid[:, 0] >= 0) & (nid[:, -1] == -1)).sum() >= 3       # an empty row, short rows
    for kw in ({}, {"lds_limit": 0}):
        _check(_run(e, nu, ni, 8, zd, **kw), nid, nw, D, f"small {kw}")


@pytest.mark.parametrize("k", (1, 10, 64))
@pytest.mark.parametrize("zd", ZD)
def test_large_graph_every_split(zd, k):
    e, nu, ni, nid, nw, D = _ref("large_graph", zd, k)
    top = cooc.lds_limit_max()
    runs = []
    for kw, light in (({}, int((D <= top).sum())), ({"lds_limit": 0}, int((D <= 0).sum())), ({"lds_limit": 10 ** 9}, int((D <= top).sum())),
                      ({"lds_limit": 300}, int((D <= 300).sum()))):
        st = {}
        got = _run(e, nu, ni, k, zd, stats=st, **kw)
        assert st["n_light"] == light and st["n_heavy"] == ni - light, (kw, st)
        _check(got, nid, nw, D, f"large k={k} {kw}")
        runs.append(got)
    assert 0 < int((D > top).sum()) < ni                     # the default split used both tiers
    for other in runs[1:]:
        assert _same(runs[0], other)                         # every bit, weights included


@pytest.mark.parametrize("zd", ZD)
def test_single_counter_row_is_reused(zd):
    """workspace_bytes holds ONE dense row: every heavy item runs in the same block on the same row, one after the other --
    a row that was not left zeroed would leak counts into the next item."""
    e, nu, ni, nid, nw, D = _ref("large_graph", zd, 10)
    st = {}
    got = _run(e, nu, ni, 10, zd, lds_limit=0, workspace_bytes=4 * ni, stats=st)
    assert st["rows"] == 1 and st["n_heavy"] == int((D > 0).sum())
    _check(got, nid, nw, D, "one row")
    with pytest.raises(T.TagrecError, match="workspace_bytes"):
        _run(e, nu, ni, 10, zd, lds_limit=0, workspace_bytes=4 * ni - 1)


@pytest.mark.parametrize("zd", ZD)
def test_hub_items_cut_into_parts(zd):
    """A dense-path item above hub_limit is walked by several blocks that share its counter row (add, take and merge launches):
    parts of about 1 000 visits cut the largest items (D_i about 43 000) into dozens of blocks; the items at the limit stay whole.
    One counter row: the hubs run one after the other on the same row.  Every form equals the reference and the unsplit run
    in every bit."""
    e, nu, ni, nid, nw, D = _ref("large_graph", zd, 10)
    whole = _run(e, nu, ni, 10, zd, split_hubs=False)
    _check(whole, nid, nw, D, "hubs whole")
    limit = int(np.sort(D)[-20])                              # the 19 largest items are hubs, the 20th sits AT the limit
    for kw in ({}, {"workspace_bytes": 4 * ni}, {"lds_limit": 0, "hub_limit": 1, "hub_part_visits": 300}):
        st = {}
        kw = dict({"hub_limit": limit, "hub_part_visits": 1000}, **kw)
        got = _run(e, nu, ni, 10, zd, stats=st, **kw)
        want_hubs = int((D > kw["hub_limit"]).sum())
        assert st["n_hub"] == want_hubs and st["n_part"] > want_hubs + 100, st      # many hubs are cut
        _check(got, nid, nw, D, f"hubs {kw}")
        assert _same(got, whole)
    for bad in ({"hub_limit": 0}, {"hub_part_visits": 0}, {"hub_limit": 1.5}):
        with pytest.raises(T.TagrecError):
            _run(e, nu, ni, 10, zd, **bad)


def _two_cliques(a, b):
    """user 0 holds items 0 .. a - 1, user 1 items a .. a + b - 1: D_i = a (+ 0 / - 1) on the first, b on the second."""
    return np.array([(0, i) for i in range(a)] + [(1, a + i) for i in range(b)], dtype=np.int64), 2, a + b


@pytest.mark.parametrize("zd", ZD)
def test_tier_boundary(zd):
    """Items whose D_i sits exactly at lds_limit (LDS table, load exactly 1 / 2 at the kernel's own limit) and at lds_limit +
    1 (dense row).  Small limit: against the reference; the kernel's own limit: against the closed form -- every candidate of a
    clique has c = 1 and the same D, so a row is the clique's k lowest ids with weight 1 / D."""
    off = 1 if zd else 0                                     # zero_diagonal: D_i = clique size - 1
    e, nu, ni = _two_cliques(6 + off, 7 + off)
    nid, nw, D = R.topk(e, nu, ni, 4, zd)
    assert set(D.tolist()) == {6, 7}
    st = {}
    _check(_run(e, nu, ni, 4, zd, lds_limit=6, stats=st), nid, nw, D, "boundary 6 / 7")
    assert st["n_light"] == 6 + off and st["n_heavy"] == 7 + off
    top, k = cooc.lds_limit_max(), 5
    a, b = top + off, top + 1 + off
    e, nu, ni = _two_cliques(a, b)
    st = {}
    g_id, g_w, g_D = (t.cpu().numpy() for t in _run(e, nu, ni, k, zd, stats=st))
    assert st["n_light"] == a and st["n_heavy"] == b and st["max_D"] == top + 1
    assert np.array_equal(g_D, np.r_[np.full(a, top), np.full(b, top + 1)])
    for lo, n, d in ((0, a, top), (a, b, top + 1)):
        for i in (lo, lo + 1, lo + n // 2, lo + n - 1):
            want = [j for j in range(lo, lo + n) if not (zd and j == i)][:k]
            assert g_id[i].tolist() == want, (i, g_id[i])
            np.testing.assert_allclose(g_w[i], np.full(k, 1.0 / d), rtol=1e-6)


@pytest.mark.parametrize("zd", ZD)
def test_probe_chain(zd):
    """A row whose candidate ids are all congruent modulo the largest LDS table (and so modulo every smaller power of two):
    every insert after the first walks the probe chain.  The reference runs on the ids divided by the stride -- a monotone
    relabelling, so counts, D, order and ties are the same."""
    stride = 2 * cooc.lds_limit_max()
    small = np.array([(0, m) for m in range(8)] + [(1, 2), (1, 5), (2, 5), (2, 7), (2, 0)], dtype=np.int64)
    nid, nw, D = R.topk(small, 3, 8, 8, zd)
    e = small * np.array([1, stride])
    ni = 7 * stride + 1
    for kw in ({}, {"lds_limit": 0}):
        g_id, g_w, g_D = (t.cpu() for t in _run(e, 3, ni, 8, zd, **kw))
        rows = torch.arange(8) * stride
        want_id = np.where(nid >= 0, nid.astype(np.int64) * stride, -1).astype(np.int32)
        _check((g_id[rows], g_w[rows], g_D[rows]), want_id, nw, D, f"chain {kw}")
        rest = torch.ones(ni, dtype=torch.bool)
        rest[rows] = False
        assert (g_id[rest] == -1).all() and (g_w[rest] == 0).all() and (g_D[rest] == 0).all()


@pytest.mark.parametrize("zd", ZD)
def test_k_and_n_edges(zd):
    e = np.array([(0, 0), (0, 1), (1, 1), (1, 2), (2, 2), (2, 4), (3, 4), (3, 0)], dtype=np.int64)      # item 3 has no user
    nid, nw, D = R.topk(e, 4, 5, 8, zd)                      # k >= n_item
    for kw in ({}, {"lds_limit": 0}):
        _check(_run(e, 4, 5, 8, zd, **kw), nid, nw, D, f"k >= n {kw}")
    one = np.array([(0, 0)], dtype=np.int64)                 # n_item = 1
    nid, nw, D = R.topk(one, 1, 1, 3, zd)
    assert nid.tolist() == ([[-1, -1, -1]] if zd else [[0, -1, -1]])
    for kw in ({}, {"lds_limit": 0}):
        _check(_run(one, 1, 1, 3, zd, **kw), nid, nw, D, f"n = 1 {kw}")
    for bad in (0, 65, -1, 2.0, True):
        with pytest.raises(T.TagrecError, match="k must be"):
            _run(e, 4, 5, bad, zd)
    with pytest.raises(T.TagrecError, match="outside"):
        _run(np.array([(0, 5)]), 4, 5, 2, zd)
    with pytest.raises(T.TagrecError, match="lds_limit"):
        _run(e, 4, 5, 2, zd, lds_limit=-1)
    with pytest.raises(T.TagrecError, match="empty"):
        _run(np.zeros((0, 2), dtype=np.int64), 4, 5, 2, zd)


def test_two_runs_give_the_same_bits():
    e, nu, ni = R.large_graph()
    a, b = _run(e, nu, ni, 10, False), _run(e, nu, ni, 10, False)
    assert _same(a, b)
