"""GPU: the DirectAU model (tagrec_amd.DirectAU) -- LightGCN's fused step with the alignment / uniformity loss stage -- and the
BPR producer with pair_batches = True.

Graph: synthetic, 2000 users x 1500 items, ~20 k edges.  B = 16 and 40 with repeated users and items: T = 2 B rows and
16 T = 512 / 1280 <= n = 3500, so the compact restricted step is taken (asserted); on the small graph (300 x 200) it is not.
L = 3, 2 and 1 (the listed top layer is then also the first), D = 64.

Tolerances between the paths are those of tests/test_gpu_inbatch_step.py (loss rtol 2e-6, gradient rtol 1e-3 + 1e-5 of the
largest entry).  The loss parts of the plain-autograd path are held to the fp64 restatement (tests/directau_torch.py) applied
to forward()'s output under the derived bound of test_gpu_directau.py, and the whole step to the restatement applied to the CPU
oracle's propagated tables (loss rtol 1e-5 as in smoke(), gradients at the tolerance between the paths).  mul_loss is a sum of
a positive part (align) and a negative one (gamma unif); it is compared at the configuration's default gamma and t."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import tagrec_amd as T
from tagrec_amd import dist, help as H, lightgcn as LG, rowops
from oracle import adj as oadj, models as om

import directau_torch as AU
from spmm_ref import Chk
from test_gpu_directau import _fwd_ref

DEV = torch.device("cuda:0")
N_USER, N_ITEM = 2000, 1500
AU_T, AU_GAMMA = 2.0, 1.0       # the configuration's defaults


@pytest.fixture(scope="module")
def ds():
    return T.synth.make_cf_dataset(N_USER, N_ITEM, 20000, seed=4)


@pytest.fixture(scope="module")
def ds_small():
    return T.synth.make_cf_dataset(300, 200, 3000, seed=5)


def _cfg(n_layer=3, B=40, **kw):
    base = dict(device=DEV, reg=1e-3, train_batch=B, dim_latent=64, dim_layer_list=[64] * n_layer, au_t=AU_T, au_gamma=AU_GAMMA)
    base.update(kw)
    return T.get_config("directau", **base)


def _model(ds, n_layer=3, B=40, seed=3, **kw):
    cfg = _cfg(n_layer, B, **kw)
    torch.manual_seed(seed)
    return T.DirectAU(ds, config=cfg).train(), cfg


def _pairs(ds, B=40, repeat=True, seed=1):
    """[B, 2] pairs of the producer; repeat: one user six times, one item five times, one (user, item) pair twice."""
    t = T.BPR_training_data(ds, config=_cfg(B=B), seed=seed).all_train_data[:B].clone()
    assert t.shape == (B, 2)
    if repeat:
        t[:6, 0] = t[0, 0]
        t[4:9, 1] = t[4, 1]
        t[12] = t[13]
    return t


class _Count:
    def __init__(self, monkeypatch, mod, fn):
        self.n, real = 0, getattr(mod, fn)

        def f(*a, **k):
            self.n += 1
            return real(*a, **k)
        monkeypatch.setattr(mod, fn, f)


def _close(l1, l0, g1, g0):
    np.testing.assert_allclose(l1, l0, rtol=2e-6)
    scale = float(g0.abs().max())
    np.testing.assert_allclose(g1.cpu().numpy(), g0.cpu().numpy(), rtol=1e-3, atol=1e-5 * scale)


def _step(m, pairs):
    m.zero_grad()
    lossx = m.loss(pairs)
    sum(lossx).backward()
    return [float(v.detach()) for v in lossx], m.table.grad.detach().clone()


def _operator_step(m, cfg, pairs):
    """forward() + help.align_uniform_loss under plain autograd -> ([loss, reg * l2], table gradient, U, I, parts)."""
    m.zero_grad()
    U, I = m.forward()[:2]
    parts = []
    l, r = H.align_uniform_loss(U, I, m.embed[0], m.embed[1], pairs, AU_T, AU_GAMMA, parts_out=parts)
    (l + cfg["reg"] * r).backward()
    return [float(l.detach()), float((cfg["reg"] * r).detach())], m.table.grad.detach().clone(), U, I, (l, r, parts[0])


def _oracle_step(ds, m, n_layer, pairs, reg):
    """The restatement applied to the CPU oracle's propagated tables -> ([loss, reg * l2], table gradient, parts)."""
    nu = ds.num["user"]
    csr = oadj.normalise(oadj.block_adjacency((ds.ui_adj.row, ds.ui_adj.col, ds.ui_adj.data, ds.ui_adj.shape)), "bi_norm")
    x0 = m.table.detach().cpu().clone().requires_grad_()
    out = om.lightgcn_propagate(x0, om.csr_to_torch(csr), n_layer)
    l, r, parts = AU.directau_tables64(out[:nu], out[nu:], x0[:nu], x0[nu:], pairs.cpu(), AU_T, float(np.float32(AU_GAMMA)))
    (l + reg * r).backward()
    return [float(l), float(reg * r)], x0.grad.float(), parts.detach()


@pytest.mark.parametrize("n_layer,B", [(3, 40), (2, 16), (1, 40)])
def test_compact_all_rows_autograd_and_oracle_steps_agree(ds, monkeypatch, n_layer, B):
    m, cfg = _model(ds, n_layer, B)
    pairs = _pairs(ds, B)
    assert 2 * B * 16 <= m.table.shape[0]
    calls = _Count(monkeypatch, LG, "restricted_forward")
    fwd, bwd = _Count(monkeypatch, rowops, "directau_fwd"), _Count(monkeypatch, rowops, "directau_bwd")
    res = {}
    res["compact"] = _step(m, pairs)
    assert calls.n == 1, "16 T <= n: the compact path must be taken"
    assert fwd.n == 1 and bwd.n == 1
    parts_c = m.last_au_parts.clone()
    assert parts_c.shape == (3,) and parts_c.is_cuda and not parts_c.requires_grad
    m.restrict_forward = False                                       # every layer on all rows
    res["all"] = _step(m, pairs)
    assert calls.n == 1 and fwd.n == 2 and bwd.n == 2
    ol, og, U, I, (l, r, parts_o) = _operator_step(m, cfg, pairs)
    res["autograd"] = (ol, og)
    for k in ("compact", "all"):
        _close(res[k][0], res["autograd"][0], res[k][1], res["autograd"][1])
    _close(res["compact"][0], res["all"][0], res["compact"][1], res["all"][1])
    np.testing.assert_allclose(parts_c.cpu().numpy(), parts_o.cpu().numpy(), rtol=2e-6, atol=2e-6)
    # the fp64 restatement on forward()'s output: the kernel's own inputs, so the derived bound of test_gpu_directau.py holds
    chk = Chk(f"directau step L={n_layer} B={B}", tag="directau")
    ur, ir = pairs[:, 0].contiguous(), pairs[:, 1].contiguous()
    ego = m.table.detach()
    ref = _fwd_ref(U.detach().index_select(0, ur), I.detach().index_select(0, ir), ego[:N_USER].index_select(0, ur),
                   ego[N_USER:].index_select(0, ir), AU_T, AU_GAMMA)
    chk.close("loss", l, *ref["loss"])
    chk.close("reg", r, *ref["reg"])
    chk.close("parts", parts_o, *ref["parts"])
    chk.done()
    # the restatement on the CPU oracle's propagated tables
    ol, og, oparts = _oracle_step(ds, m, n_layer, pairs, cfg["reg"])
    print(f"[directau] L={n_layer} B={B} compact {res['compact'][0]} oracle {ol} parts {parts_c.tolist()} oracle {oparts.tolist()}")
    np.testing.assert_allclose(res["compact"][0], ol, rtol=1e-5, atol=1e-7)
    np.testing.assert_allclose(parts_c.cpu().numpy(), oparts.numpy(), rtol=1e-5, atol=1e-6)
    _close(ol, ol, res["compact"][1], og.to(DEV))


def test_small_graph_takes_the_all_rows_path(ds_small, monkeypatch):
    """16 T > n: the step gathers the T rows of the all-rows propagation; it agrees with the operator form and the oracle."""
    B = 40
    m, cfg = _model(ds_small, 2, B)
    pairs = _pairs(ds_small, B)
    assert 2 * B * 16 > m.table.shape[0]
    calls = _Count(monkeypatch, LG, "restricted_forward")
    step = _step(m, pairs)
    assert calls.n == 0
    op = _operator_step(m, cfg, pairs)
    _close(step[0], op[0], step[1], op[1])
    ol, og, _ = _oracle_step(ds_small, m, 2, pairs, cfg["reg"])
    np.testing.assert_allclose(step[0], ol, rtol=1e-5, atol=1e-7)
    _close(ol, ol, step[1], og.to(DEV))
    # row folds (split_adj_k > 1): loss() itself takes the operator path
    m2, _ = _model(ds_small, 2, B, split_adj_k=2)
    assert torch.equal(m2.table, m.table) and not m2._fused_ok() and m2.last_au_parts is None
    fold = _step(m2, pairs)
    _close(fold[0], step[0], fold[1], step[1])
    np.testing.assert_allclose(m2.last_au_parts.cpu().numpy(), m.last_au_parts.cpu().numpy(), rtol=2e-6, atol=2e-6)


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
def test_deterministic_step_with_repeated_ids_gives_the_same_bits(ds, restrict):
    """deterministic=True: two fresh models run step + Adam on a batch that repeats users and items; losses, gradients,
    parameters and moments are identical bit for bit (compact and all-rows paths)."""
    pairs = _pairs(ds)
    runs = []
    for _ in range(2):
        m, _ = _model(ds, deterministic=True)
        m.restrict_forward = restrict
        opt = T.Adam(m.parameters(), lr=0.01)
        loss, grads = _one_step(m, opt, pairs)
        runs.append([loss, m.last_au_parts.clone()] + grads + _state(m, opt))
    assert all(bool(torch.isfinite(t).all()) for t in runs[0] if t is not None)
    assert len(runs[0]) == len(runs[1]) and all(_eq(a, b) for a, b in zip(*runs))


def _batches(ds, n, B=40, seed=2):
    all_t = T.BPR_training_data(ds, config=_cfg(B=B), seed=seed).all_train_data
    return [all_t[i * B:(i + 1) * B].clone() for i in range(n)]


def test_fused_adam_gives_the_separate_update_bits(ds):
    """`Adam.fuse_into(model)`, reg = 0: the table after one and after three steps equals the separate update bit for bit
    (the rule of the fused-Adam tests: a deterministic step, equal bits)."""
    batches = _batches(ds, 3)
    tabs = []
    for fuse in (False, True):
        m, _ = _model(ds, reg=0.0, deterministic=True)
        opt = T.Adam(m.parameters(), lr=0.01)
        if fuse:
            opt.fuse_into(m)
        snaps = []
        for b in batches:
            _one_step(m, opt, b)
            snaps.append(m.table.detach().clone())
        if fuse:
            assert m.table.grad is None          # the update ran in the last hop's epilogue: no gradient tensor was written
        tabs.append(snaps)
    assert torch.equal(tabs[0][0], tabs[1][0]) and torch.equal(tabs[0][2], tabs[1][2])


def test_fused_adam_with_l2_falls_back_to_the_unfused_update(ds):
    """reg != 0: the L2 rows are folded after the last hop, so the step hands the optimizer a gradient; the table equals the
    one of a model that never asked for the fused update."""
    batches = _batches(ds, 2)
    tabs = []
    for fuse in (False, True):
        m, _ = _model(ds, reg=1e-3, deterministic=True)
        opt = T.Adam(m.parameters(), lr=0.01)
        if fuse:
            opt.fuse_into(m)
        for b in batches:
            _one_step(m, opt, b)
        tabs.append(m.table.detach().clone())
    assert torch.equal(tabs[0], tabs[1])


def test_graphed_step_replay_equals_the_eager_step(ds):
    """The loss stage reads nothing back to the host: GraphedStep captures the deterministic step and three replays give the
    eager steps' bits (the structure of tests/test_gpu_inbatch_step.py)."""
    batches = _batches(ds, 5)

    def make():
        m, _ = _model(ds, reg=0.0, deterministic=True)
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


def test_step_workspace_off_gives_the_same_bits(ds):
    pairs = _pairs(ds)
    runs = []
    for ws in (True, False):
        m, _ = _model(ds, deterministic=True, step_workspace=ws)
        assert (m.step_ws is not None) == ws
        first = _step(m, pairs)
        second = _step(m, pairs)                                     # the second step reuses the workspace buffers
        assert first[0] == second[0] and torch.equal(first[1], second[1])
        runs.append(first)
    assert runs[0][0] == runs[1][0] and torch.equal(runs[0][1], runs[1][1])


def _reset_draws(m):
    m._drop_calls = 0
    m._node_drop_calls = 0


@pytest.mark.parametrize("kw", [dict(message_drop_list=[0.2, 0.2, 0.2]),
                                dict(node_drop=0.25, node_drop_mode="kernel"),
                                dict(node_drop=0.25, node_drop_mode="kernel", message_drop_list=[0.2, 0.2, 0.2]),
                                dict(node_drop=0.25, node_drop_mode="rebuild")],
                         ids=["message", "edge-kernel", "edge-kernel+message", "edge-rebuild"])
def test_dropout_steps_equal_the_masked_operator_form(ds, kw):
    """Message dropout and edge dropout: the fused step equals forward() + help.align_uniform_loss under plain autograd with
    the same masks (the per-call seed counters are put back; the rebuild mode draws its mask from torch's generator, which is
    re-seeded), at the tolerance between the paths; the dropped loss differs from the undropped one."""
    m, cfg = _model(ds, **kw)
    pairs = _pairs(ds)
    torch.manual_seed(11)
    step = _step(m, pairs)
    _reset_draws(m)
    torch.manual_seed(11)
    op = _operator_step(m, cfg, pairs)
    _close(step[0], op[0], step[1], op[1])
    m0, _ = _model(ds)
    plain = _step(m0, pairs)
    assert abs(plain[0][0] - step[0][0]) > 1e-4 and np.isfinite(step[0]).all() and bool(torch.isfinite(step[1]).all())
    m.eval()
    m0.eval()
    with torch.no_grad():                                            # eval mode: no dropout, the undropped model's bits
        assert all(torch.equal(a, b) for a, b in zip(m.loss(pairs), m0.loss(pairs)))


# ====================================================================================================== producer
def test_producer_yields_the_pairs_of_the_default_epoch_array(ds):
    """pair_batches = True: [E, 2], bit-equal to columns 0:2 of the default producer's array for the same seed (the shuffle
    draws from the same generator), over two epochs; with neg_candidates > 1 no model is needed."""
    E = len(ds.edge_index["train"])
    ppair = T.BPR_training_data(ds, config=_cfg(), seed=7)
    pdef = T.BPR_training_data(ds, config=T.get_config("lightgcn", use_tag=False, device=DEV, train_batch=40), seed=7)
    pkey = T.BPR_training_data(ds, config=T.get_config("lightgcn", use_tag=False, device=DEV, train_batch=40, pair_batches=True), seed=7)
    phard = T.BPR_training_data(ds, config=_cfg(neg_candidates=4), seed=7)
    for _ in range(2):
        assert ppair.all_train_data.shape == (E, 2) and ppair.all_train_data.dtype == torch.int64
        assert pdef.all_train_data.shape == (E, 3)
        assert torch.equal(ppair.all_train_data, pdef.all_train_data[:, :2])
        assert torch.equal(pkey.all_train_data, ppair.all_train_data) and torch.equal(phard.all_train_data, ppair.all_train_data)
        for p in (ppair, pdef, pkey, phard):
            p.reset()
    with pytest.raises(T.TagrecError, match="pair_batches"):
        T.BPR_training_data(ds, config=_cfg(pair_batches=1))


def test_other_producers_and_models_are_unchanged_by_the_key(ds_small):
    """pair_batches is read by BPR_training_data alone: DGCF_training_data draws the same triplets with the key present, and
    LightGCN / NGCF built from configs that carry it take [B, 3] batches and give the bits of models built without it."""
    kw = dict(use_tag=False, device=DEV, train_batch=32)
    a = T.DGCF_training_data(ds_small, config=T.get_config("dgcf", **kw), seed=5).mini_sample()
    b = T.DGCF_training_data(ds_small, config=T.get_config("dgcf", pair_batches=True, **kw), seed=5).mini_sample()
    assert a[0].shape == (32, 3) and torch.equal(a[0], b[0]) and torch.equal(a[1], b[1])
    trip = T.BPR_training_data(ds_small, config=T.get_config("lightgcn", **kw), seed=5).all_train_data[:32]
    for name, cls, shape in (("lightgcn", T.LightGCN, dict(dim_latent=64, dim_layer_list=[64, 64])),
                             ("ngcf", T.NGCF, dict(dim_latent=32, dim_layer_list=[32, 16]))):
        out = []
        for extra in ({}, {"pair_batches": True}):
            torch.manual_seed(3)
            m = cls(ds_small, config=T.get_config(name, reg=1e-3, deterministic=True, **kw, **shape, **extra)).train()
            lossx = m.loss(trip)
            sum(lossx).backward()
            out.append([v.detach() for v in lossx] + [p.grad.clone() for p in m.parameters()])
        assert all(torch.equal(x, y) for x, y in zip(*out))


def test_epoch_training_lowers_the_loss(ds):
    """A full epoch through epoch_training on [E, 2] batches; the mean loss falls from the first epoch to the third."""
    m, cfg = _model(ds, B=512, lr=0.01)
    prod = T.BPR_training_data(ds, config=cfg, seed=3)
    opt = T.Adam(m.parameters(), lr=0.01)
    losses = []
    for _ in range(3):
        out = T.epoch_training(prod, m.loss, opt, verbose=False)
        losses.append(float(np.mean(out)))
    assert all(np.isfinite(losses)) and losses[2] < losses[0]


# ====================================================================================================== refusals
def test_refusals(ds):
    m, _ = _model(ds)
    pairs = _pairs(ds)
    with pytest.raises(T.TagrecError, match=r"\[B, 2\]"):
        m.loss(torch.cat([pairs, pairs[:, 1:]], 1))
    with pytest.raises(T.TagrecError, match="B = 1"):
        m.loss(pairs[:1])
    lossx = m.loss(pairs)                                            # a refused batch leaves the model usable
    assert all(bool(torch.isfinite(v)) for v in lossx)
    for bad, word in ((dict(au_t=21), "au_t"), (dict(au_t=0.0), "au_t"), (dict(au_gamma=-1.0), "au_gamma"),
                      (dict(n_negatives=2), "n_negatives"), (dict(negatives="in_batch", mul_loss_func="softmax"), "negatives")):
        with pytest.raises(T.TagrecError, match=word):
            T.DirectAU(ds, config=_cfg(**bad))
    for cls in (dist.ShardedLightGCN, dist.ShardedNGCF, dist.FeatureShardedLightGCN):
        with pytest.raises(T.TagrecError, match="directau"):
            cls(ds, _cfg(), None, None, None, 0)
    with pytest.raises(T.TagrecError, match="n_negatives"):         # LightGCN itself still refuses a [B, 2] batch
        T.LightGCN(ds, config=T.get_config("lightgcn", use_tag=False, device=DEV, dim_layer_list=[64])).train().loss(pairs)
