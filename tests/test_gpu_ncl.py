"""GPU: the two NCL terms (help.ncl_structure_loss / help.ncl_prototype_loss) against the fp64 restatement of
tests/ncl_torch.py on a dense fp64 copy of the adjacency, and the model T.NCL: parent parity, the switches, determinism, the
driver hook and the refusals.

Tolerances: the ones DESIGN section 2 states for composed passes -- losses rtol 1e-5, gradients rtol 1e-3 with atol 1e-5 of
the largest entry (what the LightGCN and SimGCL step tests use)."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import tagrec_amd as T
from tagrec_amd import help as H

import ncl_torch as NT

DEV = torch.device("cuda:0")
N_USER, N_ITEM, B = 300, 200, 48


@pytest.fixture(scope="module")
def ds():
    return T.synth.make_cf_dataset(N_USER, N_ITEM, 4000, seed=4)


def _cfg(D, L=2, model="ncl", **kw):
    base = dict(use_tag=False, device=DEV, reg=1e-3, train_batch=B, dim_latent=D, dim_layer_list=[D] * L)
    if model == "ncl":
        base.update(ncl_clusters=11, ncl_kmeans_iters=3, ncl_struct_rate=0.1, ncl_proto_rate=0.05, ncl_alpha=0.7, ncl_temperature=0.2)
    base.update(kw)
    return T.get_config(model, **base)


def _table(D, seed=9):
    return (torch.randn(N_USER + N_ITEM, D, generator=torch.Generator().manual_seed(seed)) * 0.1).float()


def _model(ds, D, L=2, **kw):
    torch.manual_seed(3)
    m = T.NCL(ds, config=_cfg(D, L, **kw)).train()
    with torch.no_grad():
        m.table.copy_(_table(D).to(DEV))
    return m


def _batch(ds, seed=1):
    """[B, 3] triplets from train edges; one user named three times and one item three times."""
    e = torch.from_numpy(T.synth.sample_bpr_epoch(ds, seed)[:B].copy())
    e[1:4, 0] = e[1, 0]
    e[5:8, 1] = e[5, 1]
    return e.to(DEV)


def _dense_adj(g):
    n = g.shape[0]
    rows = torch.repeat_interleave(torch.arange(n, device=DEV), g.rowptr[1:] - g.rowptr[:-1])
    A = torch.zeros(n, n, dtype=torch.float64)
    A.index_put_((rows.cpu(), g.col.long().cpu()), g.val.double().cpu(), accumulate=True)
    return A


def _grad_close(got, want):
    np.testing.assert_allclose(got.cpu().numpy(), want.float().numpy(), rtol=1e-3, atol=1e-5 * float(want.abs().max()))


class _Count:
    def __init__(self, monkeypatch, mod, fn):
        self.n, real = 0, getattr(mod, fn)

        def f(*a, **k):
            self.n += 1
            return real(*a, **k)
        monkeypatch.setattr(mod, fn, f)


@pytest.mark.parametrize("deterministic", (False, True))
@pytest.mark.parametrize("D", (16, 64))
def test_structure_term_against_fp64(ds, D, deterministic):
    m = _model(ds, D)
    batch = _batch(ds)
    tau, alpha = 0.2, 0.7
    x = m.table.detach().clone().requires_grad_()
    got = H.ncl_structure_loss(x, m.norm_adj, N_USER, N_ITEM, batch, tau, alpha, deterministic)
    got.backward()
    A = _dense_adj(m.norm_adj)
    x64 = m.table.detach().cpu().double().requires_grad_()
    want = NT.struct_loss(x64, A, N_USER, N_ITEM, batch.cpu(), tau, alpha)
    want.backward()
    print(f"[ncl] structure D={D}: {float(got)} vs {float(want)}")
    np.testing.assert_allclose(float(got), float(want), rtol=1e-5)
    _grad_close(x.grad, x64.grad)
    # the two paths of the gradient, one at a time: through y2 (T detached) and through T (y2 detached)
    for part in ("y2", "T"):
        xq = m.table.detach().clone().requires_grad_(part == "y2")
        xt = m.table.detach().clone().requires_grad_(part == "T")
        y2 = H.split_mm(m.norm_adj, H.split_mm(m.norm_adj, xq))
        ub, ib = batch[:, 0].contiguous(), batch[:, 1].contiguous()
        l = H._NodeContrast.apply(y2, xt[:N_USER], ub, ub, tau, False, None) \
            + alpha * H._NodeContrast.apply(y2, xt[N_USER:], ib + N_USER, ib, tau, False, None)
        l.backward()
        q64 = m.table.detach().cpu().double().requires_grad_(part == "y2")
        t64 = m.table.detach().cpu().double().requires_grad_(part == "T")
        y64 = A @ (A @ q64)
        bc = batch.cpu()
        F = torch.nn.functional
        w = F.cross_entropy(F.normalize(y64[bc[:, 0]], dim=1) @ F.normalize(t64[:N_USER], dim=1).T / tau, bc[:, 0]) \
            + alpha * F.cross_entropy(F.normalize(y64[N_USER + bc[:, 1]], dim=1) @ F.normalize(t64[N_USER:], dim=1).T / tau, bc[:, 1])
        w.backward()
        np.testing.assert_allclose(float(l), float(want), rtol=1e-5)
        _grad_close((xq if part == "y2" else xt).grad, (q64 if part == "y2" else t64).grad)


@pytest.mark.parametrize("deterministic", (False, True))
@pytest.mark.parametrize("D", (16, 64))
def test_prototype_term_against_fp64(ds, D, deterministic):
    """Centroids and assignments given by hand."""
    K, tau, alpha = 7, 0.2, 0.7
    g = torch.Generator().manual_seed(D)
    cu = torch.nn.functional.normalize(torch.randn(K, D, generator=g), dim=1).float()
    ci = torch.nn.functional.normalize(torch.randn(K, D, generator=g), dim=1).float()
    clu, cli = torch.randint(0, K, (N_USER,), generator=g), torch.randint(0, K, (N_ITEM,), generator=g)
    batch = _batch(ds)
    x = _table(D).to(DEV).requires_grad_()
    got = H.ncl_prototype_loss(x, N_USER, N_ITEM, batch, cu.to(DEV), ci.to(DEV), clu.to(DEV), cli.to(DEV), tau, alpha, deterministic)
    got.backward()
    x64 = _table(D).double().requires_grad_()
    want = NT.proto_loss(x64, N_USER, N_ITEM, batch.cpu(), cu.double(), ci.double(), clu, cli, tau, alpha)
    want.backward()
    print(f"[ncl] prototype D={D}: {float(got)} vs {float(want)}")
    np.testing.assert_allclose(float(got), float(want), rtol=1e-5)
    _grad_close(x.grad, x64.grad)
    touched = set(batch[:, 0].tolist()) | {N_USER + i for i in batch[:, 1].tolist()}
    assert set(torch.nonzero(x.grad.abs().sum(1)).flatten().tolist()) <= touched


def _parts_and_grads(m, batch):
    """loss() and the table gradient of each part taken alone, then of the sum."""
    grads = []
    for k in range(4):
        m.zero_grad()
        parts = m.loss(batch)
        if parts[k].requires_grad:
            parts[k].backward()
            grads.append(m.table.grad.detach().clone())
        else:
            grads.append(torch.zeros_like(m.table))
    m.zero_grad()
    parts = m.loss(batch)
    sum(parts).backward()
    return [p.detach().clone() for p in parts], grads, m.table.grad.detach().clone()


def test_model_parts_switches_and_gradient(ds, monkeypatch):
    D = 16
    batch = _batch(ds)
    s_calls, p_calls = _Count(monkeypatch, H, "ncl_structure_loss"), _Count(monkeypatch, H, "ncl_prototype_loss")
    m = _model(ds, D, deterministic=True)
    torch.manual_seed(3)
    twin = T.LightGCN(ds, config=_cfg(D, model="lightgcn", deterministic=True), graph=m.norm_adj).train()
    with torch.no_grad():
        twin.table.copy_(m.table)
    twin.zero_grad()
    lp = twin.loss(batch)
    sum(lp).backward()
    parts = m.loss(batch)
    assert len(parts) == 4 and len(lp) == 2
    assert torch.equal(parts[0], lp[0]) and torch.equal(parts[1], lp[1])              # the first two ARE LightGCN.loss
    assert float(parts[2]) > 0 and float(parts[3]) == 0.0 and not parts[3].requires_grad      # no e_step yet
    assert s_calls.n == 1 and p_calls.n == 0
    m.e_step()
    assert m.e_steps == 1 and int(m.cluster_u.max()) < 11 and int(m.cluster_i.max()) < 11
    np.testing.assert_allclose(m.cent_u.norm(dim=1).cpu().numpy(), 1.0, rtol=1e-5)
    parts, grads, total = _parts_and_grads(m, batch)
    assert all(bool(torch.isfinite(p)) for p in parts) and float(parts[2]) > 0 and float(parts[3]) > 0
    assert torch.equal(parts[0], lp[0]) and torch.equal(parts[1], lp[1])
    # the sum's gradient is the sum of the four parts' gradients within fp32 addition.  At most 8 gradient edges arrive at the
    # table (the step, two products' chain, two ego slices per term side); autograd adds them in its order, this sum in
    # ours: 7 roundings on either side, each on a partial sum no larger than the largest entry of sum_k |grad_k|
    ssum = grads[0] + grads[1] + grads[2] + grads[3]
    mag = float(sum(g.abs() for g in grads).max())
    worst = float((total - ssum).abs().max())
    print(f"[ncl] gradient of the sum vs sum of the gradients: worst {worst:.3e}, bound {14 * 2.0 ** -24 * mag:.3e}")
    assert worst <= 14 * 2.0 ** -24 * mag
    assert all(float(g.abs().max()) > 0 for g in grads)
    # the terms against the restatement, through the model (its own centroid buffers)
    A = _dense_adj(m.norm_adj)
    x64 = m.table.detach().cpu().double()
    want_s = m.ncl_struct_rate * NT.struct_loss(x64, A, N_USER, N_ITEM, batch.cpu(), m.ncl_temperature, m.ncl_alpha)
    want_p = m.ncl_proto_rate * NT.proto_loss(x64, N_USER, N_ITEM, batch.cpu(), m.cent_u.cpu().double(), m.cent_i.cpu().double(),
                                              m.cluster_u.cpu(), m.cluster_i.cpu(), m.ncl_temperature, m.ncl_alpha)
    np.testing.assert_allclose([float(parts[2]), float(parts[3])], [float(want_s), float(want_p)], rtol=1e-5)
    # eval mode: exact zeros, nothing launched for either term
    s0, p0 = s_calls.n, p_calls.n
    m.eval()
    with torch.no_grad():
        le = m.loss(batch)
    assert float(le[2]) == 0.0 and float(le[3]) == 0.0 and (s_calls.n, p_calls.n) == (s0, p0)
    m.train()
    # a zero rate launches nothing for that term; the other term is unchanged bit for bit
    for kw, idx in ((dict(ncl_struct_rate=0.0), 2), (dict(ncl_proto_rate=0.0), 3)):
        mz = _model(ds, D, deterministic=True, **kw)
        mz.e_step()
        s0, p0 = s_calls.n, p_calls.n
        lz = mz.loss(batch)
        assert float(lz[idx]) == 0.0 and not lz[idx].requires_grad
        assert (s_calls.n - s0, p_calls.n - p0) == ((0, 1) if idx == 2 else (1, 0))
        assert torch.equal(lz[5 - idx].detach(), parts[5 - idx])
    # both rates zero: the step is the parent's, gradient included
    m0 = _model(ds, D, deterministic=True, ncl_struct_rate=0.0, ncl_proto_rate=0.0)
    m0.begin_epoch(100)
    assert m0.e_steps == 0
    m0.zero_grad()
    l0 = m0.loss(batch)
    sum(l0).backward()
    assert torch.equal(l0[0], lp[0]) and torch.equal(l0[1], lp[1]) and torch.equal(m0.table.grad, twin.table.grad)


@pytest.mark.parametrize("D", (16, 64))
def test_deterministic_mode_gives_the_same_bits(ds, D):
    batch = _batch(ds)
    runs = []
    for _ in range(2):
        m = _model(ds, D, deterministic=True)
        out = []
        for _ in range(2):
            m.e_step()
            m.zero_grad()
            parts = m.loss(batch)
            sum(parts).backward()
            out += [p.detach().clone() for p in parts] + [m.table.grad.detach().clone(), m.cent_u.clone(), m.cent_i.clone(),
                                                          m.cluster_u.clone(), m.cluster_i.clone()]
        runs.append(out)
    assert all(bool(torch.isfinite(t.float()).all()) for t in runs[0])
    assert all(torch.equal(a, b) for a, b in zip(*runs))
    assert not torch.equal(runs[0][5], runs[0][14])                    # the second e-step drew another seed


def test_basic_train_calls_the_e_step_from_the_warm_up_on(ds, monkeypatch):
    cfg = _cfg(16, epochs=3, test_interval=100, ncl_warm_up=1, train_batch=512)
    torch.manual_seed(3)
    m = T.NCL(ds, config=cfg)
    seen, real_begin = [], m.begin_epoch
    monkeypatch.setattr(m, "begin_epoch", lambda ep: (seen.append((ep, m.e_steps)), real_begin(ep))[1])
    ids = [id(t) for t in (m.cent_u, m.cent_i, m.cluster_u, m.cluster_i)]
    ptrs = [t.data_ptr() for t in (m.cent_u, m.cent_i, m.cluster_u, m.cluster_i)]
    before = m.cent_u.clone()
    train = T.Basic_train([T.BPR_training_data(ds, config=cfg, seed=3)], [m.loss], [T.Adam(m.parameters(), lr=0.01)], None, None,
                          config=cfg)
    hist = train.run(m, verbose=False)
    assert seen == [(0, 0), (1, 0), (2, 1)] and m.e_steps == 2         # e_step ran exactly at epochs 1 and 2
    assert [id(t) for t in (m.cent_u, m.cent_i, m.cluster_u, m.cluster_i)] == ids
    assert [t.data_ptr() for t in (m.cent_u, m.cent_i, m.cluster_u, m.cluster_i)] == ptrs
    assert not torch.equal(m.cent_u, before)                           # changed in place
    assert len(hist) == 3 and all(np.isfinite(h[2]).all() for h in hist)
    assert sorted(m.state_dict()) == ["embed.0", "embed.1"]
    # a LightGCN run through the same driver is unchanged: it has no hook, and two runs give the same losses
    runs = []
    for _ in range(2):
        lcfg = _cfg(16, model="lightgcn", epochs=2, test_interval=100, train_batch=512, deterministic=True)
        torch.manual_seed(3)
        p = T.LightGCN(ds, config=lcfg)
        assert not hasattr(p, "begin_epoch")
        t = T.Basic_train([T.BPR_training_data(ds, config=lcfg, seed=3)], [p.loss], [T.Adam(p.parameters(), lr=0.01)], None, None,
                          config=lcfg)
        runs.append([h[2] for h in t.run(p, verbose=False)])
        # the same steps by hand, without the driver
        torch.manual_seed(3)
        q = T.LightGCN(ds, config=lcfg).train()
        opt, prod = T.Adam(q.parameters(), lr=0.01), T.BPR_training_data(ds, config=lcfg, seed=3)
        by_hand = [T.epoch_training(prod, q.loss, opt, verbose=False) for _ in range(2)]
        assert by_hand == runs[-1]
    assert runs[0] == runs[1]


def test_refusals(ds):
    for bad, word in ((dict(split_adj_k=2), "split_adj_k"), (dict(dim_layer_list=[16]), "layers"),
                      (dict(dim_latent=12 + 2, dim_layer_list=[14, 14]), "dim_latent"),
                      (dict(dim_latent=260, dim_layer_list=[260, 260]), "dim_latent"),
                      (dict(message_drop_list=[0.1, 0.0, 0.0]), "message_drop_list"), (dict(node_drop=0.1), "node_drop"),
                      (dict(ncl_clusters=N_ITEM + 1), "ncl_clusters")):
        with pytest.raises(T.TagrecError, match=word):
            T.NCL(ds, config=_cfg(16, **bad))
    m = _model(ds, 16)
    opt = T.Adam(m.parameters(), lr=0.01)
    with pytest.raises(T.TagrecError, match="fuse_into"):
        opt.fuse_into(m)
    batch = _batch(ds)
    m.loss(batch)
    graph = torch.cuda.CUDAGraph()
    with pytest.raises(T.TagrecError, match="captured"):
        with torch.cuda.graph(graph):
            m.loss(batch)
    torch.cuda.synchronize()
    parts = m.loss(batch)                                              # the model is usable afterwards
    assert all(bool(torch.isfinite(v)) for v in parts)
