"""GPU: the fused LightGCN / NGCF steps and the BPR producer with negatives = "in_batch".

Graph: synthetic, 1000 users x 700 items, ~9 k edges.  B = 48 with repeated users and items: T = 2 B = 96 rows and
16 T = 1536 <= n = 1700, so the compact restricted step is taken (asserted); this is the smallest graph on which a batch of
48 takes it.  LightGCN: L = 3 and L = 1 (the listed top layer is then also the first), D = 64; NGCF at toy widths, two layers
(32 -> 32 -> 16, concatenated 80) and one (32 -> 32); "ngcf-wide" (64 -> 64 -> 64, concatenated 192) puts the kernels' dynamic
LDS past 64 KB, where the launch needs a function attribute, under graph capture.

Tolerances between the paths are those of tests/test_gpu_rank_step.py (test_gpu_lightgcn.py: loss rtol 2e-6, gradient rtol
1e-3 + 1e-5 of the largest entry; test_gpu_ngcf.py: loss rtol 1e-6, gradient norm 1e-3 relative + 1e-6 of the largest
tensor's norm).  The loss parts of the plain-autograd path are held to the fp64 restatement (tests/inbatch_torch.py) applied
to forward()'s output under the derived bound of test_gpu_inbatch.py, and the whole step to the restatement applied to the
CPU oracle's propagated tables (loss rtol 1e-5 as in smoke(), gradients at the tolerance between the paths)."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import tagrec_amd as T
from tagrec_amd import dist, help as H, lightgcn as LG, ngcf as NG, rowops
from oracle import adj as oadj, models as om

import inbatch_torch as IB
from spmm_ref import Chk
from test_gpu_inbatch import _fwd_ref

DEV = torch.device("cuda:0")
N_USER, N_ITEM, B, TAU = 1000, 700, 48, 0.5
CLS = {"lightgcn": T.LightGCN, "ngcf": T.NGCF}
MOD = {"lightgcn": LG, "ngcf": NG}
SHAPE = {"lightgcn": dict(dim_latent=64, dim_layer_list=[64, 64, 64]), "ngcf": dict(dim_latent=32, dim_layer_list=[32, 16]),
         "lightgcn-1": dict(dim_latent=64, dim_layer_list=[64]), "ngcf-1": dict(dim_latent=32, dim_layer_list=[32]),
         "ngcf-wide": dict(dim_latent=64, dim_layer_list=[64, 64])}


def _kind(name):
    return name.split("-")[0]


@pytest.fixture(scope="module")
def ds():
    return T.synth.make_cf_dataset(N_USER, N_ITEM, 9000, seed=4)


def _cfg(name, **kw):
    base = dict(use_tag=False, device=DEV, reg=1e-3, train_batch=B, negatives="in_batch", mul_loss_func="softmax",
                loss_temperature=TAU)
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
    if _kind(name) == "lightgcn":
        np.testing.assert_allclose(l1, l0, rtol=2e-6)
        scale = float(g0["table"].abs().max())
        np.testing.assert_allclose(g1["table"].cpu().numpy(), g0["table"].cpu().numpy(), rtol=1e-3, atol=1e-5 * scale)
    else:
        np.testing.assert_allclose(l1, l0, rtol=1e-6)
        top = max(float(v.double().norm()) for v in g0.values())
        for k in g0:
            a, b = g0[k].double(), g1[k].double()
            assert float((a - b).norm()) <= 1e-3 * float(a.norm()) + 1e-6 * top, k


def _oracle_step(ds, name, m, pairs, reg, logq=None):
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
    l, r = IB.in_batch_tables64(out[:N_USER], out[N_USER:], ego[:N_USER], ego[N_USER:], pairs.cpu(), TAU, logq)
    (l + reg * r).backward()
    return [float(l), float(reg * r)], {k: v.grad.float() for k, v in prm.items()}


@pytest.mark.parametrize("name", ["lightgcn", "ngcf", "lightgcn-1", "ngcf-1"])
def test_compact_all_rows_autograd_and_oracle_steps_agree(ds, monkeypatch, name):
    m, cfg = _model(ds, name)
    full, name = name, _kind(name)
    pairs = _pairs(ds)
    n = m.table.shape[0]
    assert 2 * B * 16 <= n
    calls = _Count(monkeypatch, MOD[name], "restricted_forward")
    fwd, bwd = _Count(monkeypatch, rowops, "inbatch_fwd"), _Count(monkeypatch, rowops, "inbatch_bwd")
    res = {}
    # the compact restricted step
    m.zero_grad()
    lossx = m.loss(pairs)
    sum(lossx).backward()
    assert calls.n == 1, "16 T <= n: the compact path must be taken"
    assert fwd.n == 1 and bwd.n == 1
    res["compact"] = ([float(v.detach()) for v in lossx], _grads(m))
    # every layer on all rows
    if name == "lightgcn":
        m.restrict_forward = False
    else:
        monkeypatch.setattr(NG, "RESTRICT_FORWARD", False)
    m.zero_grad()
    lossx = m.loss(pairs)
    sum(lossx).backward()
    assert calls.n == 1 and fwd.n == 2 and bwd.n == 2
    res["all"] = ([float(v.detach()) for v in lossx], _grads(m))
    # forward() + help.in_batch_loss under plain autograd
    m.zero_grad()
    U, I = m.forward()[:2]
    Ur, Ir = (m.embed[0], m.embed[1]) if name == "lightgcn" else (U, I)
    l, r = H.in_batch_loss(U, I, Ur, Ir, pairs, TAU)
    (l + cfg["reg"] * r).backward()
    res["autograd"] = ([float(l.detach()), float((cfg["reg"] * r).detach())], _grads(m))
    for k in ("compact", "all"):
        _close(name, res[k][0], res["autograd"][0], res[k][1], res["autograd"][1])
    _close(name, res["compact"][0], res["all"][0], res["compact"][1], res["all"][1])
    # the fp64 restatement on forward()'s output: the kernel's own inputs, so the derived bound of test_gpu_inbatch.py holds
    chk = Chk(f"in-batch step {full}", tag="inbatch")
    out = torch.cat([U, I]).detach()
    ego = m.table.detach() if name == "lightgcn" else out
    want = IB.in_batch_tables64(U.detach().cpu(), I.detach().cpu(), ego[:N_USER].cpu(), ego[N_USER:].cpu(), pairs.cpu(), TAU)
    ur, ir = pairs[:, 0].contiguous(), pairs[:, 1].contiguous()
    ref = _fwd_ref(out[:N_USER].index_select(0, ur), out[N_USER:].index_select(0, ir), ego[:N_USER].index_select(0, ur),
                   ego[N_USER:].index_select(0, ir), TAU, ur, ir)
    assert abs(float(want[0]) - ref["loss"][0]) <= 1e-12 and abs(float(want[1]) - ref["reg"][0]) <= 1e-12
    chk.close("loss", l, *ref["loss"])
    chk.close("reg", r, *ref["reg"])
    chk.done()
    # the restatement on the CPU oracle's propagated tables
    ol, og = _oracle_step(ds, full, m, pairs, cfg["reg"])
    np.testing.assert_allclose(res["compact"][0], ol, rtol=1e-5, atol=1e-7)
    _close(name, ol, ol, res["compact"][1], {k: v.to(DEV) for k, v in og.items()})       # the gradients, at the paths' tolerance


@pytest.mark.parametrize("name", ["lightgcn", "ngcf"])
def test_in_batch_logq_changes_the_loss_as_the_restatement_says(ds, name):
    """in_batch_logq=True: the model's table is log(train degree / train edges), and the step's loss is the restatement's with
    that column bias -- and differs from the uncorrected loss."""
    m, cfg = _model(ds, name, in_batch_logq=True)
    m0, _ = _model(ds, name)
    pairs = _pairs(ds)
    e = np.asarray(ds.edge_index["train"].cpu() if torch.is_tensor(ds.edge_index["train"]) else ds.edge_index["train"])
    deg = np.bincount(e[:, 1], minlength=N_ITEM).astype(np.float64)
    want = np.where(deg > 0, np.log(np.maximum(deg, 1) / len(e)), 0.0).astype(np.float32)
    assert m0.item_logq is None and np.array_equal(m.item_logq.cpu().numpy(), want)
    lossx, loss0 = m.loss(pairs), m0.loss(pairs)
    sum(lossx).backward()
    ol, og = _oracle_step(ds, name, m, pairs, cfg["reg"], torch.from_numpy(want))
    np.testing.assert_allclose([float(v.detach()) for v in lossx], ol, rtol=1e-5, atol=1e-7)
    _close(name, ol, ol, _grads(m), {k: v.to(DEV) for k, v in og.items()})
    assert abs(float(lossx[0]) - float(loss0[0])) > 1e-3 and float(lossx[1]) == float(loss0[1])
    # and through the operator path
    U, I = m.forward()[:2]
    l, _ = H.in_batch_loss(U, I, None, None, pairs, TAU, m.item_logq)
    np.testing.assert_allclose(float(l), float(lossx[0]), rtol=2e-6)


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
    pairs = _pairs(ds)
    runs = []
    for _ in range(2):
        m, _ = _model(ds, name, deterministic=True)
        m.restrict_forward = restrict
        opt = T.Adam(m.parameters(), lr=0.01)
        loss, grads = _one_step(m, opt, pairs)
        runs.append([loss] + grads + _state(m, opt))
    assert all(bool(torch.isfinite(t).all()) for t in runs[0] if t is not None)
    assert len(runs[0]) == len(runs[1]) and all(_eq(a, b) for a, b in zip(*runs))


def test_fused_adam_gives_the_separate_update_bits(ds):
    """`Adam.fuse_into(model)` (LightGCN, reg = 0): the table after three in-batch steps equals the separate update bit for
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
    """The in-batch loss stage reads nothing back to the host: GraphedStep captures the deterministic step and three replays
    give the eager steps' bits (the structure of test_gpu_rank_step.py)."""
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
    """negatives = "in_batch": [E, 2], bit-equal to columns 0:2 of the default producer's array for the same seed (the shuffle
    draws from the same generator), over two epochs; with neg_candidates > 1 no model is needed."""
    E = len(ds.edge_index["train"])
    pin = T.BPR_training_data(ds, config=_cfg("lightgcn"), seed=7)
    pdef = T.BPR_training_data(ds, config=T.get_config("lightgcn", use_tag=False, device=DEV, train_batch=B), seed=7)
    phard = T.BPR_training_data(ds, config=_cfg("lightgcn", neg_candidates=4), seed=7)
    for _ in range(2):
        assert pin.all_train_data.shape == (E, 2) and pin.all_train_data.dtype == torch.int64
        assert pdef.all_train_data.shape == (E, 3)
        assert torch.equal(pin.all_train_data, pdef.all_train_data[:, :2])
        assert torch.equal(phard.all_train_data, pin.all_train_data)
        for p in (pin, pdef, phard):
            p.reset()


def test_epoch_training_lowers_the_loss(ds):
    """A full epoch through epoch_training on [E, 2] batches; the mean loss falls from the first epoch to the third."""
    m, cfg = _model(ds, "lightgcn", train_batch=512, lr=0.01)
    prod = T.BPR_training_data(ds, config=cfg, seed=3)
    opt = T.Adam(m.parameters(), lr=0.01)
    losses = []
    for _ in range(3):
        out = T.epoch_training(prod, m.loss, opt, verbose=False)
        assert len(out) == -(-len(ds.edge_index["train"]) // 512) or len(out) == len(ds.edge_index["train"]) // 512
        losses.append(float(np.mean(out)))
    assert all(np.isfinite(losses)) and losses[2] < losses[0]


# ====================================================================================================== refusals
@pytest.mark.parametrize("name", ["lightgcn", "ngcf"])
def test_batch_width_must_be_two(ds, name):
    m, _ = _model(ds, name)
    trip = torch.cat([_pairs(ds), _pairs(ds)[:, 1:]], 1)
    with pytest.raises(T.TagrecError, match="in_batch"):
        m.loss(trip)
    m1 = CLS[name](ds, config=T.get_config(name, use_tag=False, device=DEV, **SHAPE[name])).train()
    with pytest.raises(T.TagrecError, match="n_negatives"):
        m1.loss(_pairs(ds))


def test_refused_combinations_models_and_producers(ds):
    for bad in (dict(mul_loss_func="softplus"), dict(n_negatives=4)):
        with pytest.raises(T.TagrecError, match="in_batch"):
            _cfg("lightgcn", **bad)
    kw = dict(negatives="in_batch", mul_loss_func="softmax", device=DEV)
    for cls, make in ((T.TGCN, lambda: T.get_config("tgcn", **kw)), (T.DGCF, lambda: T.get_config("dgcf", **kw)),
                      (T.DisenGCN, lambda: T.get_config("disengcn", **kw)), (T.KGAT, lambda: T.get_config("kgat", **kw)),
                      (T.DisenHAN, lambda: T.disenhan_config(**kw)), (T.DGCF_training_data, lambda: T.get_config("dgcf", **kw))):
        with pytest.raises(T.TagrecError, match="in_batch"):
            cls(ds, config=make())
    for cls in (dist.ShardedLightGCN, dist.ShardedNGCF, dist.FeatureShardedLightGCN):
        with pytest.raises(T.TagrecError, match="in_batch"):
            cls(ds, T.get_config("lightgcn", **kw), None, None, None, 0)
