"""GPU: the fused LightGCN / NGCF steps and the BPR producer with n_negatives = K (multi-negative ranking losses).

Graph: synthetic, 600 users x 400 items, ~6 k edges.  B = 8, K = 4: T = (2 + K) B = 48 and 16 T = 768 <= n = 1000, so the
compact restricted step is taken (asserted).  LightGCN: L = 3, D = 64; NGCF at toy widths (32 -> 32 -> 16).

Tolerances between the paths are those of test_restricted_forward_equals_full_forward_step (test_gpu_lightgcn.py: loss rtol
2e-6, gradient rtol 1e-3 + 1e-5 of the largest entry; test_gpu_ngcf.py: loss rtol 1e-6, gradient norm 1e-3 relative + 1e-6 of
the largest tensor's norm).  The loss parts of the plain-autograd path are held to the fp64 restatement
(tests/ranking_torch.py) applied to forward()'s output under the derived bound of test_gpu_rank_loss.py."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import tagrec_amd as T
from tagrec_amd import help as H, lightgcn as LG, ngcf as NG, rowops

import ranking_torch as R
from spmm_ref import Chk
from test_gpu_rank_loss import _fwd_ref

DEV = torch.device("cuda:0")
N_USER, N_ITEM, B, K = 600, 400, 8, 4
CLS = {"lightgcn": T.LightGCN, "ngcf": T.NGCF}
MOD = {"lightgcn": LG, "ngcf": NG}
SHAPE = {"lightgcn": dict(dim_latent=64, dim_layer_list=[64, 64, 64]), "ngcf": dict(dim_latent=32, dim_layer_list=[32, 16])}


@pytest.fixture(scope="module")
def ds():
    return T.synth.make_cf_dataset(N_USER, N_ITEM, 6000, seed=4)


def _cfg(name, **kw):
    base = dict(use_tag=False, device=DEV, reg=1e-3, train_batch=B, n_negatives=K, mul_loss_func="softmax", loss_temperature=0.5)
    base.update(SHAPE[name])
    base.update(kw)
    return T.get_config(name, **base)


def _model(ds, name, seed=3, **kw):
    cfg = _cfg(name, **kw)
    torch.manual_seed(seed)
    m = CLS[name](ds, config=cfg)
    return m.train(), cfg


def _tuples(ds, repeat=False, k=K, seed=1):
    """[B, 2 + k] tuples of the producer; repeat: one user four times, one item as positive, as a negative and twice in a tuple."""
    t = T.BPR_training_data(ds, config=_cfg("lightgcn", n_negatives=k), seed=seed).all_train_data[:B].clone()
    assert t.shape == (B, 2 + k)
    if repeat:
        t[:4, 0] = t[0, 0]
        t[1, 1], t[2, 2], t[3, 3] = t[0, 1], t[0, 1], t[0, 1]
        t[5, 2] = t[5, 3]
    return t


class _Count:
    def __init__(self, monkeypatch, mod, fn):
        self.n, real = 0, getattr(mod, fn)

        def f(*a, **k):
            self.n += 1
            return real(*a, **k)
        monkeypatch.setattr(mod, fn, f)


def _grads(m):
    return {k: p.grad.detach().clone() for k, p in m.named_parameters()}


def _close(name, l1, l0, g1, g0):
    if name == "lightgcn":
        np.testing.assert_allclose(l1, l0, rtol=2e-6)
        scale = float(g0["table"].abs().max())
        np.testing.assert_allclose(g1["table"].cpu().numpy(), g0["table"].cpu().numpy(), rtol=1e-3, atol=1e-5 * scale)
    else:
        np.testing.assert_allclose(l1, l0, rtol=1e-6)
        top = max(float(v.double().norm()) for v in g0.values())
        for k in g0:
            a, b = g0[k].double(), g1[k].double()
            assert float((a - b).norm()) <= 1e-3 * float(a.norm()) + 1e-6 * top, k


@pytest.mark.parametrize("loss,tau", [("softmax", 0.5), ("softplus", 1.0), ("logsigmoid", 1.0)])
@pytest.mark.parametrize("name", ["lightgcn", "ngcf"])
def test_compact_all_rows_and_autograd_steps_agree(ds, monkeypatch, name, loss, tau):
    m, cfg = _model(ds, name, mul_loss_func=loss, loss_temperature=tau)
    tup = _tuples(ds, repeat=True)
    n = m.table.shape[0]
    assert tup.shape[1] * B * 16 <= n
    calls = _Count(monkeypatch, MOD[name], "restricted_forward")
    res = {}
    # the compact restricted step
    m.zero_grad()
    lossx = m.loss(tup)
    sum(lossx).backward()
    assert calls.n == 1, "16 T <= n: the compact path must be taken"
    res["compact"] = ([float(v.detach()) for v in lossx], _grads(m))
    # every layer on all rows
    if name == "lightgcn":
        m.restrict_forward = False
    else:
        monkeypatch.setattr(NG, "RESTRICT_FORWARD", False)
    m.zero_grad()
    lossx = m.loss(tup)
    sum(lossx).backward()
    assert calls.n == 1
    res["all"] = ([float(v.detach()) for v in lossx], _grads(m))
    # forward() + help.ranking_loss under plain autograd
    m.zero_grad()
    U, I = m.forward()[:2]
    Ur, Ir = (m.embed[0], m.embed[1]) if name == "lightgcn" else (U, I)
    l, r = H.ranking_loss(U, I, Ur, Ir, tup, loss, tau)
    (l + cfg["reg"] * r).backward()
    res["autograd"] = ([float(l.detach()), float((cfg["reg"] * r).detach())], _grads(m))
    for k in ("compact", "all"):
        _close(name, res[k][0], res["autograd"][0], res[k][1], res["autograd"][1])
    _close(name, res["compact"][0], res["all"][0], res["compact"][1], res["all"][1])
    # the fp64 restatement on forward()'s output: the kernel's own inputs, so the derived bound of test_gpu_rank_loss.py holds
    chk = Chk(f"step {name} {loss}", tag="rank")
    rows = rowops.tuple_rows(tup, N_USER)
    out = torch.cat([U, I]).detach()
    ego = m.table.detach() if name == "lightgcn" else out
    want = R.ranking_loss64(U.detach().cpu(), I.detach().cpu(), ego[:N_USER].cpu(), ego[N_USER:].cpu(), tup.cpu(), loss, tau)
    ref = _fwd_ref(out.index_select(0, rows[:B]), out.index_select(0, rows[B:]), ego.index_select(0, rows[:B]),
                   ego.index_select(0, rows[B:]), K, loss, tau)
    assert abs(float(want[0]) - ref["loss"][0]) <= 1e-12 and abs(float(want[1]) - ref["reg"][0]) <= 1e-12
    chk.close("loss", l, *ref["loss"])
    chk.close("reg", r, *ref["reg"])
    chk.done()


def _one_step(m, opt, batch):
    lossx = m.loss(batch)
    opt.zero_grad()
    sum(lossx).backward()
    grads = [None if p.grad is None else p.grad.detach().clone() for p in m.parameters()]
    opt.step()
    return torch.stack([v.detach() for v in lossx]), grads


def _state(m, opt):
    out = [p.detach().clone() for p in m.parameters()]
    for p in m.parameters():
        st = opt.state.get(id(p), {})
        out += [st[k].clone() for k in ("m", "v") if k in st]
    return out


def _eq(a, b):
    return (a is None and b is None) or (a is not None and b is not None and torch.equal(a, b))


@pytest.mark.parametrize("restrict", [True, False])
@pytest.mark.parametrize("name", ["lightgcn", "ngcf"])
def test_deterministic_step_with_repeated_ids_gives_the_same_bits(ds, monkeypatch, name, restrict):
    """deterministic=True: two fresh models run step + Adam on a batch that repeats users and items; losses, gradients,
    parameters and moments are identical bit for bit (compact and all-rows paths)."""
    if not restrict:
        monkeypatch.setattr(NG, "RESTRICT_FORWARD", False)
    tup = _tuples(ds, repeat=True)
    runs = []
    for _ in range(2):
        m, _ = _model(ds, name, deterministic=True)
        m.restrict_forward = restrict
        opt = T.Adam(m.parameters(), lr=0.01)
        loss, grads = _one_step(m, opt, tup)
        runs.append([loss] + grads + _state(m, opt))
    assert all(bool(torch.isfinite(t).all()) for t in runs[0] if t is not None)
    assert len(runs[0]) == len(runs[1]) and all(_eq(a, b) for a, b in zip(*runs))


def test_fused_adam_gives_the_separate_update_bits(ds):
    """`Adam.fuse_into(model)` (LightGCN, reg = 0): the table after one K-negative step equals the separate update bit for bit."""
    tup = _tuples(ds)
    tabs = []
    for fuse in (False, True):
        m, _ = _model(ds, "lightgcn", reg=0.0, deterministic=True)
        opt = T.Adam(m.parameters(), lr=0.01)
        if fuse:
            opt.fuse_into(m)
        _one_step(m, opt, tup)
        if fuse:
            assert m.table.grad is None          # the update ran in the last hop's epilogue: no gradient tensor was written
        tabs.append(m.table.detach().clone())
    assert torch.equal(tabs[0], tabs[1])


@pytest.mark.parametrize("name", ["lightgcn", "ngcf"])
def test_graphed_step_replay_equals_the_eager_step(ds, name):
    """The K-negative loss stage reads nothing back to the host: GraphedStep captures the deterministic step and its replays
    give the eager steps' bits (the structure of test_gpu_deterministic.py::test_graphed_step_gives_the_eager_bits)."""
    all_t = T.BPR_training_data(ds, config=_cfg(name), seed=2).all_train_data
    batches = [all_t[i * B:(i + 1) * B].clone() for i in range(4)]

    def make():
        m, _ = _model(ds, name, reg=0.0, deterministic=True)
        opt = T.Adam(m.parameters(), lr=0.01, capturable=True)
        opt.fuse_into(m)
        return m, opt
    m0, opt0 = make()
    eager = [_one_step(m0, opt0, b)[0] for b in batches]
    m1, opt1 = make()
    for b in batches[:2]:
        _one_step(m1, opt1, b)
    gstep = T.GraphedStep(m1.loss, opt1, batches[2])
    got = [gstep(b) for b in batches[2:]]
    torch.cuda.synchronize()
    for a, b in zip(got, eager[2:]):
        assert torch.equal(a, b)
    for a, b in zip(_state(m0, opt0), _state(m1, opt1)):
        assert torch.equal(a, b)


@pytest.mark.parametrize("name", ["lightgcn", "ngcf"])
def test_batch_width_must_match_n_negatives(ds, name):
    m, _ = _model(ds, name)
    with pytest.raises(T.TagrecError, match="n_negatives"):
        m.loss(_tuples(ds, k=1))
    m1, _ = _model(ds, name, n_negatives=1, mul_loss_func="softplus")
    with pytest.raises(T.TagrecError, match="n_negatives"):
        m1.loss(_tuples(ds))


def test_softmax_with_one_negative_is_the_softplus_step(ds):
    """K = 1, tau = 1 through the model: the "softmax" step (multi-negative kernels) against the default softplus step
    (triplet kernels) -- the same function, within the path tolerances."""
    tup = _tuples(ds, k=1)
    res = []
    for loss in ("softplus", "softmax"):
        m, _ = _model(ds, "lightgcn", n_negatives=1, mul_loss_func=loss, loss_temperature=1.0)
        lossx = m.loss(tup)
        sum(lossx).backward()
        res.append(([float(v.detach()) for v in lossx], _grads(m)))
    _close("lightgcn", res[1][0], res[0][0], res[1][1], res[0][1])


# ====================================================================================================== producer
def _train_pairs(ds):
    e = np.asarray(ds.edge_index["train"])
    return set(zip(e[:, 0].tolist(), e[:, 1].tolist()))


@pytest.mark.parametrize("kw", [{}, {"neg_sampling": "popularity"}])
def test_producer_yields_rejection_tested_tuples(ds, kw):
    cfg = _cfg("lightgcn", **kw)
    prod = T.BPR_training_data(ds, config=cfg, seed=5)
    data = prod.all_train_data
    E = len(ds.edge_index["train"])
    assert data.shape == (E, 2 + K) and data.dtype == torch.int64
    d = data.cpu().numpy()
    pairs = _train_pairs(ds)
    assert set(zip(d[:, 0].tolist(), d[:, 1].tolist())) == pairs                    # every train edge once
    assert d[:, 2:].min() >= 0 and d[:, 2:].max() < N_ITEM
    for j in range(K):                                                             # no negative is a train item of its user
        assert not any((u, i) in pairs for u, i in zip(d[:, 0].tolist(), d[:, 2 + j].tolist())), j
    assert len({tuple(d[:, 2 + j].tolist()) for j in range(K)}) == K               # the columns are different streams
    prod.reset()
    assert prod.all_train_data.shape == (E, 2 + K) and not torch.equal(prod.all_train_data, data)


def test_producer_with_one_negative_is_the_old_epoch_array(ds):
    """n_negatives = 1 (and a config without the key): the epoch array is today's bit for bit -- the negative of stream
    (seed << 20) + epoch, stacked and shuffled by the producer's generator -- for two epochs."""
    cfg = _cfg("lightgcn", n_negatives=1, mul_loss_func="softplus")
    old = dict(cfg)
    del old["n_negatives"], old["loss_temperature"]
    for c in (cfg, old):
        prod = T.BPR_training_data(ds, config=c, seed=7)
        u, i = prod.pos_inter[:, 0].contiguous(), prod.pos_inter[:, 1]
        gen = torch.Generator(device=DEV)
        gen.manual_seed(7)
        got = [prod.all_train_data]
        prod.reset()
        got.append(prod.all_train_data)
        for epoch in range(2):
            neg = prod._pos.sample(u, (7 << 20) + epoch)
            want = torch.stack([u, i, neg], dim=1)
            want = want[torch.randperm(want.shape[0], device=DEV, generator=gen)].contiguous()
            assert got[epoch].shape == want.shape and torch.equal(got[epoch], want)


def test_first_negative_column_is_the_one_negative_stream(ds):
    """Column 2 of the K = 4 epoch, before the shuffle, equals the K = 1 negatives (uniform and popularity proposals), and
    the shuffle is the permutation K = 1 draws."""
    for kw in ({}, {"neg_sampling": "popularity"}):
        p4 = T.BPR_training_data(ds, config=_cfg("lightgcn", **kw), seed=5)
        p1 = T.BPR_training_data(ds, config=_cfg("lightgcn", n_negatives=1, **kw), seed=5)
        for epoch in (0, 3):
            n4, n1 = p4.negatives(epoch), p1.negatives(epoch)
            assert n4.shape == (p4.pos_inter.shape[0], K) and n1.shape == (p1.pos_inter.shape[0], 1)
            assert torch.equal(n4[:, 0], n1[:, 0])
        assert torch.equal(p4.all_train_data[:, :3], p1.all_train_data)


# ====================================================================================================== the triplet route
def test_default_step_is_still_the_triplet_route(ds, monkeypatch):
    """One default-config LightGCN step (K = 1, softplus) gives the loss and gradient bits of the triplet kernels driven by
    hand on the compact rows, as the step did before the multi-negative dispatch existed; the new kernels are not called.
    (A batch without repeated ids: the default mode's atomic folds are then order-free.)"""
    cfg = T.get_config("lightgcn", use_tag=False, device=DEV, reg=1e-3, train_batch=B, **SHAPE["lightgcn"])
    assert cfg["n_negatives"] == 1 and cfg["mul_loss_func"] == "softplus"
    torch.manual_seed(3)
    m = T.LightGCN(ds, config=cfg).train()
    trip = torch.tensor([[u, 2 * u + 1, 2 * u + 100] for u in range(10, 10 + B)], dtype=torch.int64, device=DEV)
    rows = rowops.batch_rows(trip, N_USER)
    assert rows.unique().numel() == 3 * B and 3 * B * 16 <= m.table.shape[0]
    fwd, bwd = _Count(monkeypatch, rowops, "rank_fwd"), _Count(monkeypatch, rowops, "rank_bwd")
    lossx = m.loss(trip)
    sum(lossx).backward()
    assert fwd.n == 0 and bwd.n == 0
    x0, g = m.table.detach(), m.norm_adj
    out_b, state = LG.restricted_forward(g, x0, 3, rows)
    ego_b = x0.index_select(0, rows)
    ctrip = rowops.compact_triplets(B, DEV)
    res, coef = rowops.bpr_fwd(out_b[:B], out_b[B:], ego_b[:B], ego_b[B:], ctrip, H.loss_kind_id("softplus"))
    assert torch.equal(lossx[0].detach(), res[0]) and torch.equal(lossx[1].detach(), cfg["reg"] * res[1])
    up = torch.tensor([1.0, cfg["reg"]], dtype=torch.float32, device=DEV)
    d_b = torch.zeros(2, 3 * B, 64, device=DEV)
    rowops.bpr_bwd(out_b[:B], out_b[B:], ego_b[:B], ego_b[B:], ctrip, coef, up, d_b[0][:B], d_b[0][B:], d_b[1][:B], d_b[1][B:])
    g0 = LG.restricted_backward(g.transpose(), rows, d_b[0], state, x0.shape)
    g0.index_add_(0, rows, d_b[1])
    assert torch.equal(m.table.grad, g0)
