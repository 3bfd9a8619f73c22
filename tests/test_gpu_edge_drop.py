"""GPU: edge dropout (`node_drop`, adj.py:170-191) evaluated inside the LightGCN products -- `Graph.edge_drop`, the
`_edrop` entry points, `node_drop_mode="kernel"`.

The mask is pinned against a numpy restatement; every product of the view is compared with the same product of the
materialised dropped matrix (`Graph.edge_drop_materialise`), which packs its sums per row where the in-kernel form packs per
64-entry batch -- so the comparisons use the project's tolerances (activations rtol 1e-5 / atol 1e-6,
losses rtol 1e-5, gradients rtol 1e-3), not bit equality.  Operands are drawn at embedding scale (0.1 * randn).

Fixture graph: 1200 users linked to item 0 (a row of 1200 entries: more than kLongRow = 1024, the chunk path), ~6000 further
random distinct interactions over 150 items, one more user (id 1200) and the last item without any interaction (empty
rows), bi_norm values, symmetric.  The model-level tests use the same construction with 3000 users: the compact restricted
step needs 3 * B * 16 <= N, which a batch of 64 triplets meets from N = 3072 on."""
import types

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import tagrec_amd as T
from tagrec_amd import graph as G, help as H
from spmm_ref import edge_kept as np_mask          # the numpy restatement of the mask

DEV = torch.device("cuda:0")
ACT = dict(rtol=1e-5, atol=1e-6)
GRAD = dict(rtol=1e-3, atol=1e-6)


# ------------------------------------------------------------------------------------------------------------- fixtures
def build_graph(n_user, n_item, n_inter, seed):
    """bi_norm user-item adjacency as CSR tensors: item 0 linked to users 0 .. n_user - 2, user n_user - 1 and item
    n_item - 1 without interactions."""
    rng = np.random.default_rng(seed)
    u = rng.integers(0, n_user - 1, n_inter)
    i = rng.integers(1, n_item - 1, n_inter)
    pair = np.unique(np.stack([u, i], 1), axis=0)
    hub = np.stack([np.arange(n_user - 1), np.zeros(n_user - 1, np.int64)], 1)
    pair = np.concatenate([hub, pair])
    rowptr, col, val, n = G.bipartite_norm_device(torch.from_numpy(pair[:, 0]).to(DEV), torch.from_numpy(pair[:, 1]).to(DEV),
                                                  n_user, n_item, "bi_norm")
    return T.Graph(rowptr, col, val, (n, n), symmetric=True)


class Fx:
    def __init__(self, g):
        self.g = g
        self.n = g.shape[0]
        self.rowptr = g.rowptr.cpu().numpy()
        self.col = g.col.cpu().numpy().astype(np.int64)
        self.val = g.val.cpu().numpy()
        self.rows = np.repeat(np.arange(self.n), np.diff(self.rowptr))


@pytest.fixture(scope="module")
def fx():
    f = Fx(build_graph(1201, 150, 6000, 5))
    deg = np.diff(f.rowptr)
    assert deg[1201] == 1200 and deg[1200] == 0 and deg[-1] == 0 and 13000 < f.g.nnz < 15000
    assert f.g.info()["n_long_rows"] == 1
    return f


@pytest.fixture(scope="module")
def fx_model():
    return build_graph(3001, 150, 7500, 6)


def _x(n, D, seed):
    return (torch.randn(n, D, generator=torch.Generator().manual_seed(seed)) * 0.1).to(DEV)


def _np(t):
    return t.detach().cpu().numpy()


# --------------------------------------------------------------------------------------------------------- 1. the mask
@pytest.mark.parametrize("seed", [1, 2, (2020 << 24) + 1])
@pytest.mark.parametrize("p", [0.1, 0.25, 0.5])
def test_mask_equals_numpy_restatement(fx, seed, p):
    got = _np(fx.g.edge_drop_mask(p, seed)).astype(bool)
    assert np.array_equal(got, np_mask(fx.rows, fx.col, p, seed))
    got_t = _np(fx.g.edge_drop_mask(p, seed, transposed=True)).astype(bool)
    assert np.array_equal(got_t, np_mask(fx.rows, fx.col, p, seed, transposed=True))
    # the transposed form at the stored entry (j, i) is the plain form at (i, j)
    key = fx.rows * fx.n + fx.col
    pos = np.searchsorted(key, fx.col * fx.n + fx.rows)
    assert np.array_equal(key[pos], fx.col * fx.n + fx.rows)
    assert np.array_equal(got_t, got[pos])


@pytest.mark.parametrize("seed", [1, 2, (2020 << 24) + 1])
@pytest.mark.parametrize("p", [0.1, 0.25, 0.5])
def test_mask_statistics(fx, seed, p):
    """Kept fraction, independence of (i, j) / (j, i), independence of consecutive seeds: each within 4 standard deviations
    of its binomial count (the mask is a pure function, so this is deterministic)."""
    m = _np(fx.g.edge_drop_mask(p, seed)).astype(bool)
    m1 = _np(fx.g.edge_drop_mask(p, seed + 1)).astype(bool)
    n = m.size

    def within(frac, q, count):
        sd = np.sqrt(q * (1 - q) / count)
        print(f"p={p} seed={seed}: {frac:.5f} vs {q:.5f} ({(frac - q) / sd:+.2f} sd)")
        return abs(frac - q) <= 4 * sd

    assert within(m.mean(), 1 - p, n)
    key = fx.rows * fx.n + fx.col
    pos = np.searchsorted(key, fx.col * fx.n + fx.rows)
    upper = fx.rows < fx.col                                   # each unordered pair once
    assert within((m & m[pos])[upper].mean(), (1 - p) ** 2, int(upper.sum()))
    assert within((m == m1).mean(), p * p + (1 - p) ** 2, n)


# -------------------------------------------------------------------------- 2. products against the materialised graph
def _flags(n, seed):
    f = torch.zeros(n, dtype=torch.uint8)
    f[torch.randperm(n, generator=torch.Generator().manual_seed(seed))[:n // 3]] = 1
    return f.to(DEV)


def _check_products(view, mat, D, hub, empty):
    """Every product of `view` against the same product of the ordinary Graph `mat`."""
    n = view.shape[0]
    x = _x(n, D, 1)
    nan = float("nan")
    # spmm
    np.testing.assert_allclose(_np(view.spmm(x)), _np(mat.spmm(x)), **ACT)
    # spmm_norm_acc with and without the accumulator
    outs = []
    for gr in (view, mat):
        y, inv, acc = torch.empty(n, D, device=DEV), torch.empty(n, device=DEV), x.clone()
        gr.spmm_norm_acc(x, y, inv, acc, 0.25)
        y2, inv2 = torch.empty(n, D, device=DEV), torch.empty(n, device=DEV)
        gr.spmm_norm_acc_rows(x, y2, inv2, None, 0.0, None)
        outs.append((y, inv, acc, y2, inv2))
    for a, b in zip(*outs):
        np.testing.assert_allclose(_np(a), _np(b), **ACT)
    assert torch.equal(outs[0][0], outs[0][3]) and torch.equal(outs[0][1], outs[0][4])
    # spmm_norm_acc_rows under a row mask: the other rows stay NaN
    mask = _flags(n, 2)
    mask[hub] = 1
    outs = []
    for gr in (view, mat):
        y, inv, acc = torch.full((n, D), nan, device=DEV), torch.full((n,), nan, device=DEV), torch.full((n, D), nan, device=DEV)
        acc[mask.bool()] = 0.5
        gr.spmm_norm_acc_rows(x, y, inv, acc, 0.25, mask)
        outs.append((y, inv, acc))
    off = ~mask.bool()
    for a, b in zip(*outs):
        assert torch.isnan(a[off]).all() and not torch.isnan(a[~off]).any()
        np.testing.assert_allclose(_np(a[~off]), _np(b[~off]), **ACT)
    # spmm_listed: repeated rows, the hub row, an empty row
    rows = torch.tensor([3, hub, 7, 3, empty, hub, n - 2, 0], dtype=torch.int64, device=DEV)
    got = view.spmm_listed(rows, x)
    np.testing.assert_allclose(_np(got), _np(mat.spmm_listed(rows, x)), **ACT)
    assert torch.equal(got[1], got[5]) and float(got[4].abs().sum()) == 0.0
    # backward hops on a row-sparse operand (flags on a third of the rows), as the non-compact step calls them ...
    fl = _flags(n, 3)
    fl[hub] = 1
    cnt = fl.sum().to(torch.int32).reshape(1)
    g_in = _x(n, D, 4) * fl[:, None]
    x_raw, dz = _x(n, D, 5), _x(n, D, 6)
    inv = 1.0 / x_raw.norm(dim=1).clamp_min(1e-12)
    dzf = _flags(n, 7)
    dzf[hub] = 1
    dz = dz * dzf[:, None]
    for row_mask, count in ((None, cnt), (mask, None), (mask, cnt)):      # ... and as the restricted step calls them
        outs = []
        for gr in (view, mat):
            go = torch.full((n, D), nan, device=DEV)
            fo, co = torch.zeros(n, dtype=torch.uint8, device=DEV), torch.zeros(1, dtype=torch.int32, device=DEV)
            gr.spmm_normbwd_sparse(g_in, fl, count, x_raw, inv, dz, 0.25, go, fo, co, row_mask=row_mask, dz_flags=dzf)
            ga = torch.full((n, D), nan, device=DEV)
            gr.spmm_axpy_sparse(g_in, fl, count, dz, 0.25, ga, row_mask=row_mask, b_flags=dzf)
            outs.append((go, fo, co, ga))
        sel = mask.bool() if row_mask is not None else torch.ones(n, dtype=torch.bool, device=DEV)
        (go, fo, co, ga), (go_r, fo_r, co_r, ga_r) = outs
        assert torch.isnan(go[~sel]).all() and torch.isnan(ga[~sel]).all() and not torch.isnan(go[sel]).any()
        np.testing.assert_allclose(_np(go[sel]), _np(go_r[sel]), **GRAD)
        np.testing.assert_allclose(_np(ga[sel]), _np(ga_r[sel]), **GRAD)
        assert torch.equal(fo, fo_r) and int(co) == int(co_r)
    # the dense forms
    outs = []
    for gr in (view, mat):
        go, ga = torch.empty(n, D, device=DEV), torch.empty(n, D, device=DEV)
        gr.spmm_normbwd(g_in, x_raw, inv, dz, 0.25, go)
        gr.spmm_axpy(g_in, dz, 0.25, ga)
        outs.append((go, ga))
    for a, b in zip(*outs):
        np.testing.assert_allclose(_np(a), _np(b), **GRAD)


@pytest.mark.parametrize("D", [8, 64, 256])
def test_products_match_materialised_graph(fx, D):
    view = fx.g.edge_drop(0.25, 11)
    mat = fx.g.edge_drop_materialise(0.25, 11)
    assert isinstance(mat, T.Graph) and not mat.symmetric and mat.nnz == int(np_mask(fx.rows, fx.col, 0.25, 11).sum())
    assert view.shape == fx.g.shape and view.nnz == fx.g.nnz and view.handle is fx.g.handle and not view.symmetric
    _check_products(view, mat, D, hub=1201, empty=1200)
    vt = view.transpose()
    assert vt.transposed and vt.handle is fx.g.handle and not vt.transpose().transposed
    _check_products(vt, mat.transpose(), D, hub=1201, empty=1200)


def test_explicit_transposed_handle(fx):
    """A Graph that is not flagged symmetric: the view's transpose walks the explicit transposed handle with swapped keys."""
    g = T.Graph(fx.g.rowptr, fx.g.col, fx.g.val, fx.g.shape, symmetric=False)
    view, mat = g.edge_drop(0.25, 11), g.edge_drop_materialise(0.25, 11)
    vt = view.transpose()
    assert vt.handle is not g.handle and vt.transposed
    x = _x(fx.n, 64, 9)
    np.testing.assert_allclose(_np(vt.spmm(x)), _np(mat.transpose().spmm(x)), **ACT)
    np.testing.assert_allclose(_np(vt.spmm(x)), _np(fx.g.edge_drop(0.25, 11).transpose().spmm(x)), **ACT)


@pytest.mark.parametrize("D", [8, 64, 256])
def test_rows_match_fp64_host_sum(fx, D):
    x = _x(fx.n, D, 12)
    x64 = _np(x).astype(np.float64)
    scale = np.float32(1.0) - np.float32(0.25)
    for transposed in (False, True):
        view = fx.g.edge_drop(0.25, 13)
        view = view.transpose() if transposed else view
        y = _np(view.spmm(x))
        keep = np_mask(fx.rows, fx.col, 0.25, 13, transposed)
        for r in (1201, 0, 1300):                                   # the hub row and two short rows
            a, b = fx.rowptr[r], fx.rowptr[r + 1]
            k = keep[a:b]
            w = (fx.val[a:b][k] / scale).astype(np.float64)
            np.testing.assert_allclose(y[r], (w[:, None] * x64[fx.col[a:b][k]]).sum(0), **ACT)


def test_heavy_drop_rows_without_survivors():
    """p = 0.9 on a tiny graph: rows that lose every entry give exact zeros and the clamped inverse norm of the plain kernel."""
    g = build_graph(41, 12, 60, 7)
    rp, col = g.rowptr.cpu().numpy(), g.col.cpu().numpy().astype(np.int64)
    rows = np.repeat(np.arange(g.shape[0]), np.diff(rp))
    kept = np.bincount(rows[np_mask(rows, col, 0.9, 21)], minlength=g.shape[0])
    dead = np.flatnonzero((np.diff(rp) > 0) & (kept == 0))
    assert dead.size > 5
    x = _x(g.shape[0], 8, 1)
    view, mat = g.edge_drop(0.9, 21), g.edge_drop_materialise(0.9, 21)
    y, inv, acc = torch.empty_like(x), torch.empty(g.shape[0], device=DEV), torch.zeros_like(x)
    view.spmm_norm_acc(x, y, inv, acc, 1.0)
    assert float(y[dead].abs().sum()) == 0.0 and float(acc[dead].abs().sum()) == 0.0
    y_r, inv_r, acc_r = torch.empty_like(x), torch.empty(g.shape[0], device=DEV), torch.zeros_like(x)
    mat.spmm_norm_acc(x, y_r, inv_r, acc_r, 1.0)
    assert torch.equal(inv[dead], inv_r[dead]) and bool((inv[dead] >= 1e12).all())     # 1 / max(0, 1e-12), as the plain kernel
    np.testing.assert_allclose(_np(y), _np(y_r), **ACT)
    np.testing.assert_allclose(_np(inv), _np(inv_r), rtol=1e-5)
    np.testing.assert_allclose(_np(acc), _np(acc_r), **ACT)


# -------------------------------------------------------------------------------- 3. one mask forward and backward
@pytest.mark.parametrize("D", [8, 64, 256])
def test_forward_and_transposed_products_are_adjoint(fx, D):
    view = fx.g.edge_drop(0.25, 17)
    x, y = _x(fx.n, D, 2), _x(fx.n, D, 3)
    ax = _np(view.spmm(x)).astype(np.float64)
    aty = _np(view.transpose().spmm(y)).astype(np.float64)
    lhs, rhs = (ax * _np(y).astype(np.float64)).sum(), (_np(x).astype(np.float64) * aty).sum()
    print(f"<Ax, y> = {lhs!r}, <x, A^T y> = {rhs!r}")
    assert abs(lhs - rhs) <= 1e-5 * max(abs(lhs), abs(rhs))
    # without the swapped key the transposed product would use the mask of (j, i): the plain view is NOT self-adjoint
    ay = _np(view.spmm(y)).astype(np.float64)
    wrong = (_np(x).astype(np.float64) * ay).sum()
    assert abs(lhs - wrong) > 1e-2 * abs(lhs)


# --------------------------------------------------------------------------------------------------- 4. model level
def _data(g):
    return types.SimpleNamespace(num={"user": g.shape[0] - 150, "item": 150})


def _cfg(n_layer, **kw):
    return T.get_config("lightgcn", use_tag=False, dim_latent=64, dim_layer_list=[64] * n_layer, device=DEV, **kw)


def _model(g, n_layer, **kw):
    torch.manual_seed(4)
    m = T.LightGCN(_data(g), config=_cfg(n_layer, **kw), graph=g)
    m.train()
    return m


def _batch(g, B=64):
    r = np.random.default_rng(8)
    nu = g.shape[0] - 150
    return torch.from_numpy(np.stack([r.integers(0, nu - 1, B), r.integers(0, 149, B), r.integers(0, 149, B)], 1)).to(DEV)


def _step(m, b):
    m.table.grad = None
    loss = m.loss(b)
    sum(loss).backward()
    return [float(v) for v in loss], m.table.grad.detach().clone()


@pytest.mark.parametrize("restrict", [True, False])
@pytest.mark.parametrize("n_layer", [2, 3])
def test_model_matches_model_on_materialised_graph(fx_model, n_layer, restrict):
    g = fx_model
    b = _batch(g)
    m = _model(g, n_layer, node_drop=0.25, node_drop_mode="kernel", restrict_forward=restrict, reg=1e-3)
    g.timing = {}
    loss, grad = _step(m, b)
    names, g.timing = set(g.timing), None
    assert ("spmm_listed" in names) == restrict              # the compact restricted step was (not) the path taken
    ref = _model(g.edge_drop_materialise(0.25, (2020 << 24) + 1), n_layer, node_drop=0.0, restrict_forward=restrict, reg=1e-3)
    assert torch.equal(ref.table, m.table)
    loss_r, grad_r = _step(ref, b)
    print(f"loss {loss} ref {loss_r}")
    np.testing.assert_allclose(loss, loss_r, rtol=1e-5)
    np.testing.assert_allclose(_np(grad), _np(grad_r), rtol=1e-3, atol=1e-8)


def test_model_message_dropout_path_honours_the_view(fx_model):
    """With message dropout the step takes the non-compact path: restricted and unrestricted forward agree, and both match
    the model on the materialised graph (same message-dropout seed, same edge mask)."""
    g = fx_model
    b = _batch(g)
    kw = dict(message_drop_list=[0.2, 0.2], reg=1e-3)
    res = [_step(_model(g, 2, node_drop=0.25, node_drop_mode="kernel", restrict_forward=r, **kw), b) for r in (True, False)]
    np.testing.assert_allclose(res[0][0], res[1][0], rtol=1e-5)
    np.testing.assert_allclose(_np(res[0][1]), _np(res[1][1]), rtol=1e-3, atol=1e-8)
    ref = _step(_model(g.edge_drop_materialise(0.25, (2020 << 24) + 1), 2, node_drop=0.0, **kw), b)
    np.testing.assert_allclose(res[0][0], ref[0], rtol=1e-5)
    np.testing.assert_allclose(_np(res[0][1]), _np(ref[1]), rtol=1e-3, atol=1e-8)


def test_model_consecutive_calls_draw_different_masks(fx_model):
    m = _model(fx_model, 2, node_drop=0.25, node_drop_mode="kernel")
    b = _batch(fx_model)
    l1, _ = _step(m, b)
    l2, _ = _step(m, b)
    assert l1[0] != l2[0]
    m._node_drop_calls = 0                                     # the same call counter: the same mask
    l3, _ = _step(m, b)
    assert l3 == l1
    # forward() in training mode draws a mask too
    with torch.no_grad():
        u1, u2 = m.forward()[0], m.forward()[0]
    assert not torch.equal(u1, u2)


def test_model_eval_is_bit_identical_to_no_node_drop(fx_model):
    m = _model(fx_model, 2, node_drop=0.25, node_drop_mode="kernel")
    ref = _model(fx_model, 2, node_drop=0.0)
    b = _batch(fx_model)
    m.eval(), ref.eval()
    with torch.no_grad():
        for a, c in zip(m.forward(), ref.forward()):
            assert torch.equal(a, c)
        for a, c in zip(m.loss(b), ref.loss(b)):
            assert torch.equal(a, c)


def test_model_step_does_not_read_stale_workspace(fx_model):
    """Poison: the StepWorkspace buffers filled with NaN / 0xFF before the step change nothing."""
    m = _model(fx_model, 3, node_drop=0.25, node_drop_mode="kernel")
    b = _batch(fx_model)
    l1, g1 = _step(m, b)
    assert m.step_ws._buf
    for t in m.step_ws._buf.values():
        t.fill_(float("nan")) if t.is_floating_point() else t.fill_(-1 if t.dtype != torch.uint8 else 255)
    m._node_drop_calls = 0
    l2, g2 = _step(m, b)
    assert l1 == l2 and bool(torch.isfinite(g2).all())
    # (the scatter of the batch gradient adds repeated rows with atomics: the last bits of a gradient may differ between runs)
    np.testing.assert_allclose(_np(g2), _np(g1), rtol=1e-5, atol=1e-9)


# --------------------------------------------------------------------------------------------- 5. refusals and defaults
def test_generic_width_is_refused(fx):
    view = fx.g.edge_drop(0.25, 1)
    with pytest.raises(T.TagrecError):
        view.spmm(_x(fx.n, 20, 1))
    # the library refuses it as well (the scalar kernel would multiply by the un-dropped matrix)
    x, y = _x(fx.n, 20, 1), torch.empty(fx.n, 20, device=DEV)
    rc = T._lib.load().tagrec_spmm_edrop_f32(fx.g.handle, T._lib.ptr(x), T._lib.ptr(y), 0.25, 1, 0, 20, T._lib.stream_ptr())
    assert rc != 0
    m = T.LightGCN(_data(fx.g), config=T.get_config("lightgcn", use_tag=False, dim_latent=20, dim_layer_list=[20, 20], device=DEV,
                                                    node_drop=0.25, node_drop_mode="kernel"), graph=fx.g)
    m.train()
    with pytest.raises(T.TagrecError):
        m.loss(_batch(fx.g))


def test_fold_list_is_refused(fx):
    ds = T.synth.make_cf_dataset(60, 50, 600, seed=3)
    folds = T.creat_adj(ds, False, "bi_norm", 2, DEV)
    with pytest.raises(T.TagrecError):
        H.node_drop(folds, 0.25, True, mode="kernel", seed=1)
    m = T.LightGCN(ds, config=T.get_config("lightgcn", use_tag=False, dim_latent=16, dim_layer_list=[16], device=DEV, split_adj_k=2,
                                           node_drop=0.25, node_drop_mode="kernel"))
    m.train()
    b = torch.from_numpy(T.synth.sample_bpr_epoch(ds, 0)[:32]).to(DEV)
    with pytest.raises(T.TagrecError):
        m.loss(b)
    with pytest.raises(T.TagrecError):
        T.LightGCN(ds, config=T.get_config("lightgcn", use_tag=False, device=DEV, node_drop_mode="bogus"))


def test_capture_is_refused_before_any_launch(fx_model):
    m = _model(fx_model, 2, node_drop=0.25, node_drop_mode="kernel")
    b = _batch(fx_model)
    _step(m, b)
    calls = m._node_drop_calls
    graph = torch.cuda.CUDAGraph()
    with pytest.raises(T.TagrecError, match="captured"):
        with torch.cuda.graph(graph):
            m.loss(b)
    assert m._node_drop_calls == calls
    torch.cuda.synchronize()
    l, _ = _step(m, b)                                         # the model is usable afterwards
    assert np.isfinite(l).all()


def test_default_mode_rebuilds_a_graph(fx):
    d = H.node_drop(fx.g, 0.25, True)
    assert type(d) is T.Graph and d is not fx.g and d.nnz < fx.g.nnz
    assert H.node_drop(fx.g, 0.25, True, mode="kernel", seed=3).handle is fx.g.handle
    assert H.node_drop(fx.g, 0.0, True, mode="kernel", seed=3) is fx.g and H.node_drop(fx.g, 0.25, False, mode="kernel") is fx.g
    m = _model(fx.g, 2, node_drop=0.25)
    assert m.node_drop_mode == "rebuild" and type(m._graph()) is T.Graph
