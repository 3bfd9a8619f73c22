"""GPU: the fused LightGCN / NGCF steps and the BPR producer with softmax_over = "catalogue".

Graph: the synthetic one of tests/test_gpu_inbatch_step.py (1000 users x 700 items, ~9 k edges), B = 48 with repeated users
and items.  On it a batch of 48 WOULD take the compact restricted step; the catalogue stage is dense (every item row is a loss
row), so the all-rows step is what must run (asserted), with nothing row-masked.  LightGCN: L = 3 and L = 1, D = 64; NGCF at
toy widths, two layers (32 -> 32 -> 16, concatenated 80) and one (32 -> 32); "ngcf-wide" (concatenated 192) puts the kernels'
dynamic LDS past 64 KB under graph capture.

Tolerances between the paths are those of test_compact_all_rows_autograd_and_oracle_steps_agree in
tests/test_gpu_inbatch_step.py (its `_close`; the oracle's loss at rtol 1e-5 as in smoke()).  The loss parts of the
plain-autograd path are held to the fp64 restatement (tests/catsoftmax_torch.py) applied to forward()'s output under the
derived bound of test_gpu_catsoftmax.py."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import tagrec_amd as T
from tagrec_amd import help as H, lightgcn as LG, ngcf as NG, rowops
from oracle import adj as oadj, models as om

import catsoftmax_torch as CS
from spmm_ref import Chk
from test_gpu_catsoftmax import _fwd_ref, _splits
from test_gpu_inbatch_step import CLS, MOD, SHAPE, _close, _Count, _eq, _grads, _kind, _one_step, _state

DEV = torch.device("cuda:0")
N_USER, N_ITEM, B, TAU = 1000, 700, 48, 0.5
CAT = dict(softmax_over="catalogue", mul_loss_func="softmax")


@pytest.fixture(scope="module")
def ds():
    return T.synth.make_cf_dataset(N_USER, N_ITEM, 9000, seed=4)


def _cfg(name, **kw):
    base = dict(use_tag=False, device=DEV, reg=1e-3, train_batch=B, loss_temperature=TAU, **CAT)
    base.update(SHAPE[name])
    base.update(kw)
    return T.get_config(_kind(name), **base)


def _model(ds, name, seed=3, **kw):
    cfg = _cfg(name, **kw)
    torch.manual_seed(seed)
    m = CLS[_kind(name)](ds, config=cfg)
    return m.train(), cfg


def _pairs(ds, repeat=True, seed=1):
    """[B, 2] pairs of the producer; repeat: one user six times, one item five times, one (user, item) pair twice."""
    t = T.BPR_training_data(ds, config=_cfg("lightgcn"), seed=seed).all_train_data[:B].clone()
    assert t.shape == (B, 2)
    if repeat:
        t[:6, 0] = t[0, 0]
        t[4:9, 1] = t[4, 1]
        t[20] = t[21]
    return t


def _oracle_step(ds, name, m, pairs, reg):
    """The restatement applied to the CPU oracle's propagated tables -> ([loss, reg * l2], {parameter name: gradient})."""
    n_layer, name = len(SHAPE[name]["dim_layer_list"]), _kind(name)
    norm = "bi_norm" if name == "lightgcn" else "ngcf"
    csr = oadj.normalise(oadj.block_adjacency((ds.ui_adj.row, ds.ui_adj.col, ds.ui_adj.data, ds.ui_adj.shape)), norm)
    adj = om.csr_to_torch(csr)
    prm = {k: p.detach().cpu().clone().requires_grad_() for k, p in m.named_parameters()}
    x0 = prm["table"]
    if name == "lightgcn":
        out, ego = om.lightgcn_propagate(x0, adj, n_layer), x0
    else:
        mats = {k.split(".")[-1]: v for k, v in prm.items() if k != "table"}
        out = om.ngcf_propagate(x0, mats, adj, n_layer)
        ego = out
    l, r = CS.catalogue_tables64(out[:N_USER], out[N_USER:], ego[:N_USER], ego[N_USER:], pairs.cpu(), TAU)
    (l + reg * r).backward()
    return [float(l), float(reg * r)], {k: v.grad.float() for k, v in prm.items()}


@pytest.mark.parametrize("name", ["lightgcn", "ngcf", "lightgcn-1", "ngcf-1"])
def test_fused_autograd_and_oracle_steps_agree(ds, monkeypatch, name):
    m, cfg = _model(ds, name)
    full, name = name, _kind(name)
    pairs = _pairs(ds)
    assert 2 * B * 16 <= m.table.shape[0]                  # a gathered-rows stage would go compact on this batch
    calls = _Count(monkeypatch, MOD[name], "restricted_forward")
    fwd, bwd = _Count(monkeypatch, rowops, "catsoftmax_fwd"), _Count(monkeypatch, rowops, "catsoftmax_bwd")
    res = {}
    # the fused step: all rows, the stage on the tables
    m.zero_grad()
    lossx = m.loss(pairs)
    sum(lossx).backward()
    assert calls.n == 0, "a dense stage never takes the compact path"
    assert fwd.n == 1 and bwd.n == (2 if name == "lightgcn" else 1)       # LightGCN's L2 rows arrive after the last hop
    res["fused"] = ([float(v.detach()) for v in lossx], _grads(m))
    # forward() + help.catalogue_softmax_loss under plain autograd
    m.zero_grad()
    U, I = m.forward()[:2]
    Ur, Ir = (m.embed[0], m.embed[1]) if name == "lightgcn" else (U, I)
    l, r = H.catalogue_softmax_loss(U, I, Ur, Ir, pairs, TAU)
    (l + cfg["reg"] * r).backward()
    res["autograd"] = ([float(l.detach()), float((cfg["reg"] * r).detach())], _grads(m))
    _close(name, res["fused"][0], res["autograd"][0], res["fused"][1], res["autograd"][1])
    # the fp64 restatement on forward()'s output: the kernel's own inputs, so the derived bound of test_gpu_catsoftmax.py holds
    chk = Chk(f"catalogue step {full}", tag="catsoftmax")
    out = torch.cat([U, I]).detach()
    ego = m.table.detach() if name == "lightgcn" else out
    want = CS.catalogue_tables64(U.detach().cpu(), I.detach().cpu(), ego[:N_USER].cpu(), ego[N_USER:].cpu(), pairs.cpu(), TAU)
    ur, ir = pairs[:, 0].contiguous(), pairs[:, 1].contiguous()
    S, R = _splits(B, N_ITEM, out.shape[1], 0)
    ref = _fwd_ref(out[:N_USER].index_select(0, ur), out[N_USER:], ir, ego[:N_USER].index_select(0, ur),
                   ego[N_USER:].index_select(0, ir), TAU, S, R)
    assert abs(float(want[0]) - ref["loss"][0]) <= 1e-12 and abs(float(want[1]) - ref["reg"][0]) <= 1e-12
    chk.close("loss", l, *ref["loss"])
    chk.close("reg", r, *ref["reg"])
    chk.done()
    # the restatement on the CPU oracle's propagated tables
    ol, og = _oracle_step(ds, full, m, pairs, cfg["reg"])
    np.testing.assert_allclose(res["fused"][0], ol, rtol=1e-5, atol=1e-7)
    _close(name, ol, ol, res["fused"][1], {k: v.to(DEV) for k, v in og.items()})         # the gradients, at the paths' tolerance


@pytest.mark.parametrize("name", ["lightgcn", "ngcf"])
def test_step_reads_no_unwritten_value_and_every_item_row_gets_a_gradient(ds, monkeypatch, name):
    """Every float buffer the step allocates with torch.empty / empty_like is pre-filled with NaN: the result is finite and
    equals the unpoisoned step's, and EVERY item row of the table receives a non-zero gradient -- the compact path was not
    taken and no row of the forward pass was masked."""
    real_empty, real_empty_like = torch.empty, torch.empty_like

    def poisoned_empty(*a, **kw):
        t = real_empty(*a, **kw)
        return t.fill_(float("nan")) if t.is_floating_point() and t.is_cuda else t

    def poisoned_empty_like(*a, **kw):
        t = real_empty_like(*a, **kw)
        return t.fill_(float("nan")) if t.is_floating_point() and t.is_cuda else t

    pairs = _pairs(ds)
    runs = []
    for poison in (False, True):
        m, _ = _model(ds, name, deterministic=True)
        if poison:
            monkeypatch.setattr(torch, "empty", poisoned_empty)
            monkeypatch.setattr(torch, "empty_like", poisoned_empty_like)
        try:
            lossx = m.loss(pairs)
            sum(lossx).backward()
            torch.cuda.synchronize()
        finally:
            monkeypatch.undo()
        runs.append([torch.stack([v.detach() for v in lossx])] + [p.grad.detach().clone() for p in m.parameters()])
    assert all(bool(torch.isfinite(t).all()) for t in runs[1])
    assert all(torch.equal(a, b) for a, b in zip(*runs))
    g = dict(zip([k for k, _ in m.named_parameters()], runs[1][1:]))["table"]
    items = g[N_USER:N_USER + N_ITEM]
    assert items.shape[0] == N_ITEM and bool((items.abs().sum(1) > 0).all())
    assert int((g[:N_USER].abs().sum(1) > 0).sum()) > pairs[:, 0].unique().numel()     # and it spread over the graph


@pytest.mark.parametrize("name", ["lightgcn", "ngcf"])
def test_deterministic_step_with_repeated_ids_gives_the_same_bits(ds, name):
    """deterministic=True: two fresh models run step + Adam on a batch that repeats users and items; losses, gradients,
    parameters and moments are identical bit for bit."""
    pairs = _pairs(ds)
    runs = []
    for _ in range(2):
        m, _ = _model(ds, name, deterministic=True)
        opt = T.Adam(m.parameters(), lr=0.01)
        loss, grads = _one_step(m, opt, pairs)
        runs.append([loss] + grads + _state(m, opt))
    assert all(bool(torch.isfinite(t).all()) for t in runs[0] if t is not None)
    assert len(runs[0]) == len(runs[1]) and all(_eq(a, b) for a, b in zip(*runs))


def test_fused_adam_gives_the_separate_update_bits(ds):
    """`Adam.fuse_into(model)` (LightGCN, reg = 0): the table after three catalogue steps equals the separate update bit for
    bit (the rule of the fused-Adam tests: a deterministic step, equal bits)."""
    all_t = T.BPR_training_data(ds, config=_cfg("lightgcn"), seed=2).all_train_data
    batches = [all_t[i * B:(i + 1) * B].clone() for i in range(3)]
    tabs = []
    for fuse in (False, True):
        m, _ = _model(ds, "lightgcn", reg=0.0, deterministic=True)
        opt = T.Adam(m.parameters(), lr=0.01)
        if fuse:
            opt.fuse_into(m)
        for b in batches:
            _one_step(m, opt, b)
        if fuse:
            assert m.table.grad is None          # the update ran in the last hop's epilogue: no gradient tensor was written
        tabs.append(m.table.detach().clone())
    assert torch.equal(tabs[0], tabs[1])


@pytest.mark.parametrize("name", ["lightgcn", "ngcf", "ngcf-wide"])
def test_graphed_step_replay_equals_the_eager_step(ds, name):
    """The catalogue stage reads nothing back to the host: GraphedStep captures the deterministic step and three replays give
    the eager steps' bits (the structure of test_gpu_rank_step.py)."""
    all_t = T.BPR_training_data(ds, config=_cfg(name), seed=2).all_train_data
    batches = [all_t[i * B:(i + 1) * B].clone() for i in range(5)]

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
    assert len(got) == 3
    for a, b in zip(got, eager[2:]):
        assert torch.equal(a, b)
    for a, b in zip(_state(m0, opt0), _state(m1, opt1)):
        assert torch.equal(a, b)


# ====================================================================================================== producer
def test_producer_yields_the_pairs_of_the_default_epoch_array(ds):
    """softmax_over = "catalogue": [E, 2], bit-equal to columns 0:2 of the default producer's array for the same seed (the
    shuffle draws from the same generator), over two epochs; with neg_candidates > 1 no model is needed."""
    E = len(ds.edge_index["train"])
    pcat = T.BPR_training_data(ds, config=_cfg("lightgcn"), seed=7)
    pdef = T.BPR_training_data(ds, config=T.get_config("lightgcn", use_tag=False, device=DEV, train_batch=B), seed=7)
    phard = T.BPR_training_data(ds, config=_cfg("lightgcn", neg_candidates=4), seed=7)
    for _ in range(2):
        assert pcat.all_train_data.shape == (E, 2) and pcat.all_train_data.dtype == torch.int64
        assert pdef.all_train_data.shape == (E, 3)
        assert torch.equal(pcat.all_train_data, pdef.all_train_data[:, :2])
        assert torch.equal(phard.all_train_data, pcat.all_train_data)
        for p in (pcat, pdef, phard):
            p.reset()


def test_epoch_training_lowers_the_loss(ds):
    """Full epochs through epoch_training on [E, 2] batches; the mean loss falls from the first epoch to the third."""
    m, cfg = _model(ds, "lightgcn", train_batch=512, lr=0.01)
    prod = T.BPR_training_data(ds, config=cfg, seed=3)
    opt = T.Adam(m.parameters(), lr=0.01)
    losses = []
    for _ in range(3):
        out = T.epoch_training(prod, m.loss, opt, verbose=False)
        losses.append(float(np.mean(out)))
    assert all(np.isfinite(losses)) and losses[2] < losses[0]


# ====================================================================================================== other models, refusals
def test_simgcl_accepts_the_key_and_directau_refuses_it(ds):
    cfg = T.get_config("simgcl", device=DEV, dim_latent=64, dim_layer_list=[64, 64], reg=1e-3, loss_temperature=TAU, **CAT)
    torch.manual_seed(3)
    m = T.SimGCL(ds, config=cfg).train()
    pairs = _pairs(ds)
    parts = m.loss(pairs)
    assert len(parts) == 3 and all(bool(torch.isfinite(p)) for p in parts)
    sum(parts).backward()
    assert bool(torch.isfinite(m.table.grad).all())
    # its ranking part is LightGCN's catalogue step on the same table
    torch.manual_seed(3)
    ref = T.LightGCN(ds, config=T.get_config("lightgcn", use_tag=False, device=DEV, dim_latent=64, dim_layer_list=[64, 64], reg=1e-3,
                                             loss_temperature=TAU, **CAT)).train()
    with torch.no_grad():
        ref.table.copy_(m.table)
    want = ref.loss(pairs)
    assert torch.equal(parts[0].detach(), want[0].detach()) and torch.equal(parts[1].detach(), want[1].detach())
    with pytest.raises(T.TagrecError, match="softmax_over"):
        T.DirectAU(ds, config=T.get_config("directau", device=DEV, **CAT))


@pytest.mark.parametrize("name", ["lightgcn", "ngcf"])
def test_batch_width_must_be_two(ds, name):
    m, _ = _model(ds, name)
    trip = torch.cat([_pairs(ds), _pairs(ds)[:, 1:]], 1)
    assert trip.shape == (B, 3)
    with pytest.raises(T.TagrecError, match="catalogue"):
        m.loss(trip)
