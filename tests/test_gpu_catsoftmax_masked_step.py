"""GPU: the fused LightGCN / NGCF steps with softmax_over = "catalogue" and catalogue_mask = "train_positives".

Graph: synth.make_cf_dataset(40, 30, 300) -- a user has one to eight of the thirty items (5.6 on average), so the mask takes
about a sixth of a row's columns, and B = 48 pairs of the producer repeat users (rows of one user with different targets
exclude each other's).  The models, widths and tolerances between the paths are those of tests/test_gpu_catsoftmax_step.py (`_close` of
tests/test_gpu_inbatch_step.py; the oracle's loss at rtol 1e-5 as in smoke()); the restatement is
tests/catsoftmax_masked_torch.py."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import tagrec_amd as T
from tagrec_amd import help as H, rowops
from oracle import adj as oadj, models as om

import catsoftmax_masked_torch as CM
import catsoftmax_torch as CS
from test_gpu_inbatch_step import CLS, SHAPE, _close, _Count, _eq, _grads, _kind, _one_step, _state

DEV = torch.device("cuda:0")
N_USER, N_ITEM, B, TAU = 40, 30, 48, 0.5
CAT = dict(softmax_over="catalogue", mul_loss_func="softmax", catalogue_mask="train_positives")


@pytest.fixture(scope="module")
def ds():
    return T.synth.make_cf_dataset(N_USER, N_ITEM, 300, seed=4)


@pytest.fixture(scope="module")
def csr(ds):
    """The users' train items on the CPU, computed once."""
    return H.user_positives_csr(ds.edge_index["train"], N_USER, N_ITEM, "cpu")


def _cfg(name, **kw):
    base = dict(use_tag=False, device=DEV, reg=1e-3, train_batch=B, loss_temperature=TAU, **CAT)
    base.update(SHAPE[name])
    base.update(kw)
    return T.get_config(_kind(name), **base)


def _model(ds, name, seed=3, **kw):
    cfg = _cfg(name, **kw)
    torch.manual_seed(seed)
    return CLS[_kind(name)](ds, config=cfg).train(), cfg


def _batches(ds, n, seed=2):
    all_t = T.BPR_training_data(ds, config=_cfg("lightgcn"), seed=seed).all_train_data
    assert all_t.shape[1] == 2 and all_t.shape[0] >= n * B
    return [all_t[i * B:(i + 1) * B].clone() for i in range(n)]


def _oracle_step(ds, name, m, pairs, reg, csr):
    """The masked restatement applied to the CPU oracle's propagated tables -> ([loss, reg * l2], {parameter: gradient})."""
    n_layer, name = len(SHAPE[name]["dim_layer_list"]), _kind(name)
    norm = "bi_norm" if name == "lightgcn" else "ngcf"
    a = oadj.normalise(oadj.block_adjacency((ds.ui_adj.row, ds.ui_adj.col, ds.ui_adj.data, ds.ui_adj.shape)), norm)
    adj = om.csr_to_torch(a)
    prm = {k: p.detach().cpu().clone().requires_grad_() for k, p in m.named_parameters()}
    x0 = prm["table"]
    if name == "lightgcn":
        out, ego = om.lightgcn_propagate(x0, adj, n_layer), x0
    else:
        mats = {k.split(".")[-1]: v for k, v in prm.items() if k != "table"}
        out = om.ngcf_propagate(x0, mats, adj, n_layer)
        ego = out
    l, r = CM.masked_catalogue_tables64(out[:N_USER], out[N_USER:], ego[:N_USER], ego[N_USER:], pairs.cpu(), *csr, TAU)
    (l + reg * r).backward()
    return [float(l), float(reg * r)], {k: v.grad.float() for k, v in prm.items()}


@pytest.mark.parametrize("name", ["lightgcn", "ngcf"])
def test_fused_operator_and_oracle_steps_agree(ds, csr, monkeypatch, name):
    m, cfg = _model(ds, name)
    pairs = _batches(ds, 1)[0]
    users = pairs[:, 0]
    assert users.unique().numel() < B                      # some user comes twice: the rows exclude each other's targets
    # the model's CSR is the helper's, on the device
    assert torch.equal(m.positives[0].cpu(), csr[0]) and torch.equal(m.positives[1].cpu(), csr[1])
    assert m.positives[0].device.type == "cuda" and m.positives[1].dtype == torch.int32
    ex = CM.dense_mask(csr[0], csr[1], pairs[:, 1].cpu(), N_ITEM, users.cpu())
    assert int(ex.sum()) > 2 * B                           # the rows of the batch lose more than two columns each on average
    seen = []
    real_fwd, real_bwd = rowops.catsoftmax_fwd, rowops.catsoftmax_bwd
    monkeypatch.setattr(rowops, "catsoftmax_fwd", lambda *a, **k: (seen.append(("fwd", k.get("mask"))), real_fwd(*a, **k))[1])
    monkeypatch.setattr(rowops, "catsoftmax_bwd", lambda *a, **k: (seen.append(("bwd", k.get("mask"))), real_bwd(*a, **k))[1])
    res = {}
    m.zero_grad()
    lossx = m.loss(pairs)
    sum(lossx).backward()
    assert [w for w, _ in seen] == ["fwd"] + ["bwd"] * (2 if name == "lightgcn" else 1)
    assert all(mk is m.positives for _, mk in seen)        # every launch of the step carries the lists
    res["fused"] = ([float(v.detach()) for v in lossx], _grads(m))
    # forward() + help.catalogue_softmax_loss(positives=...) under plain autograd
    m.zero_grad()
    U, I = m.forward()[:2]
    Ur, Ir = (m.embed[0], m.embed[1]) if name == "lightgcn" else (U, I)
    l, r = H.catalogue_softmax_loss(U, I, Ur, Ir, pairs, TAU, positives=m.positives)
    (l + cfg["reg"] * r).backward()
    res["autograd"] = ([float(l.detach()), float((cfg["reg"] * r).detach())], _grads(m))
    _close(name, res["fused"][0], res["autograd"][0], res["fused"][1], res["autograd"][1])
    # the restatement on forward()'s own output (the loss parts), and on the CPU oracle's propagated tables (the step)
    out = torch.cat([U, I]).detach().cpu()
    ego = m.table.detach().cpu() if name == "lightgcn" else out
    want = CM.masked_catalogue_tables64(out[:N_USER], out[N_USER:], ego[:N_USER], ego[N_USER:], pairs.cpu(), *csr, TAU)
    np.testing.assert_allclose([float(l.detach()), float(r.detach())], [float(want[0]), float(want[1])], rtol=1e-5)
    ol, og = _oracle_step(ds, name, m, pairs, cfg["reg"], csr)
    np.testing.assert_allclose(res["fused"][0], ol, rtol=1e-5, atol=1e-7)
    _close(name, ol, ol, res["fused"][1], {k: v.to(DEV) for k, v in og.items()})
    # and the mask is at work: the unmasked restatement on the same tables is a larger loss
    plain = CS.catalogue_tables64(out[:N_USER], out[N_USER:], None, None, pairs.cpu(), TAU)[0]
    assert float(plain) > float(want[0]) * (1 + 1e-3)


@pytest.mark.parametrize("name", ["lightgcn", "ngcf"])
def test_deterministic_step_gives_the_same_bits(ds, name):
    pairs = _batches(ds, 1)[0]
    runs = []
    for _ in range(2):
        m, _ = _model(ds, name, deterministic=True)
        opt = T.Adam(m.parameters(), lr=0.01)
        loss, grads = _one_step(m, opt, pairs)
        runs.append([loss] + grads + _state(m, opt))
    assert all(bool(torch.isfinite(t).all()) for t in runs[0] if t is not None)
    assert len(runs[0]) == len(runs[1]) and all(_eq(a, b) for a, b in zip(*runs))


def test_fused_adam_gives_the_separate_update_bits(ds):
    """`Adam.fuse_into(model)` (LightGCN, reg = 0): the table after three masked steps equals the separate update bit for bit
    (the rule of the fused-Adam tests: a deterministic step, equal bits)."""
    batches = _batches(ds, 3)
    tabs = []
    for fuse in (False, True):
        m, _ = _model(ds, "lightgcn", reg=0.0, deterministic=True)
        opt = T.Adam(m.parameters(), lr=0.01)
        if fuse:
            opt.fuse_into(m)
        for b in batches:
            _one_step(m, opt, b)
        if fuse:
            assert m.table.grad is None
        tabs.append(m.table.detach().clone())
    assert torch.equal(tabs[0], tabs[1])


@pytest.mark.parametrize("name", ["lightgcn", "ngcf"])
def test_graphed_step_replay_equals_the_eager_step(ds, name):
    """The CSR is static and nothing is read on the host: GraphedStep captures the deterministic masked step, and a replay on
    another batch gives the eager step's bits."""
    batches = _batches(ds, 4)

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


def test_other_models_refuse_the_key_and_the_default_builds_no_csr(ds, monkeypatch):
    with pytest.raises(T.TagrecError):
        T.DirectAU(ds, config=T.get_config("directau", device=DEV, **CAT))
    cfg = T.get_config("directau", device=DEV)
    cfg["catalogue_mask"] = "train_positives"              # a hand-edited config that skipped get_config's check
    with pytest.raises(T.TagrecError, match="catalogue_mask"):
        T.DirectAU(ds, config=cfg)
    for cls, model in ((T.TGCN, "tgcn"), (T.DGCF, "dgcf")):
        with pytest.raises(T.TagrecError):
            cls(ds, config=T.get_config(model, device=DEV, **CAT))
        cfg = T.get_config(model, device=DEV)
        cfg["catalogue_mask"] = "train_positives"
        with pytest.raises(T.TagrecError, match="catalogue_mask"):
            cls(ds, config=cfg)
    calls = _Count(monkeypatch, H, "user_positives_csr")
    for name in ("lightgcn", "ngcf"):
        for kw in (dict(softmax_over="catalogue", mul_loss_func="softmax"), {}):
            base = dict(use_tag=False, device=DEV, **SHAPE[name], **kw)
            m = CLS[name](ds, config=T.get_config(name, **base))
            assert m.positives is None and m.mask_positives is False
    assert calls.n == 0
    m, _ = _model(ds, "lightgcn")
    assert calls.n == 1 and m.positives is not None
    # SimGCL's ranking part is LightGCN's masked step on the same table
    scfg = T.get_config("simgcl", device=DEV, dim_latent=64, dim_layer_list=[64, 64], reg=1e-3, loss_temperature=TAU, **CAT)
    torch.manual_seed(3)
    s = T.SimGCL(ds, config=scfg).train()
    torch.manual_seed(3)
    ref = T.LightGCN(ds, config=T.get_config("lightgcn", use_tag=False, device=DEV, dim_latent=64, dim_layer_list=[64, 64],
                                             reg=1e-3, loss_temperature=TAU, **CAT)).train()
    with torch.no_grad():
        ref.table.copy_(s.table)
    pairs = _batches(ds, 1)[0]
    parts, want = s.loss(pairs), ref.loss(pairs)
    assert torch.equal(parts[0].detach(), want[0].detach()) and torch.equal(parts[1].detach(), want[1].detach())
