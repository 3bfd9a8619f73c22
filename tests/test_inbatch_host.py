"""Host side of the in-batch softmax loss (no GPU): the fp64 restatement the GPU tests compare against
(tests/inbatch_torch.py) pinned three ways, the config keys and their refusals, and the logQ table."""
import math

import numpy as np
import pytest
import torch

import tagrec_amd as T
from tagrec_amd import config as C, dist, help as H

import inbatch_torch as IB
import ranking_torch as R


def _loops(Ub, Ib, tau, uid, iid, bias):
    """The definition with explicit Python loops -> (loss, [loss_b])."""
    B = len(Ub)
    rows = []
    for b in range(B):
        zs, zbb = [], None
        for j in range(B):
            z = sum(float(x) * float(y) for x, y in zip(Ub[b], Ib[j])) / tau - (0.0 if bias is None else float(bias[j]))
            if j == b:
                zbb = z
            elif uid is not None and (int(iid[j]) == int(iid[b]) or int(uid[j]) == int(uid[b])):
                continue
            zs.append(z)
        m = max(zs)
        rows.append(m + math.log(sum(math.exp(z - m) for z in zs)) - zbb)
    return sum(rows) / B, rows


@pytest.mark.parametrize("B", [1, 2, 3, 5])
@pytest.mark.parametrize("ids,bias", [(False, False), (True, False), (True, True)])
def test_restatement_against_explicit_loops(B, ids, bias):
    g = torch.Generator().manual_seed(10 * B + ids + 2 * bias)
    D, tau = 6, 0.5
    Ub, Ib = torch.randn(B, D, generator=g, dtype=torch.float64), torch.randn(B, D, generator=g, dtype=torch.float64)
    uid = torch.randint(0, 3, (B,), generator=g) if ids else None
    iid = torch.randint(0, 3, (B,), generator=g) if ids else None
    cb = torch.randn(B, generator=g, dtype=torch.float64) if bias else None
    got, reg = IB.in_batch_loss64(Ub, Ib, Ub, Ib, tau, uid, iid, cb)
    want, _ = _loops(Ub.tolist(), Ib.tolist(), tau, None if uid is None else uid.tolist(), None if iid is None else iid.tolist(),
                     None if cb is None else cb.tolist())
    assert abs(float(got) - want) <= 1e-13 * max(1.0, abs(want))
    assert abs(float(reg) - 0.5 * (float((Ub ** 2).sum()) + float((Ib ** 2).sum())) / B) <= 1e-13
    if B == 1:
        assert float(got) == 0.0


@pytest.mark.parametrize("B,tau", [(2, 1.0), (7, 0.05), (64, 0.5)])
def test_distinct_ids_without_bias_is_sampled_softmax_over_the_other_positives(B, tau):
    """In-batch softmax is sampled softmax with K = B - 1 whose negatives are the other positives: the restatement of the
    multi-negative losses on the rearranged scores (column 0 the diagonal) says the same."""
    g = torch.Generator().manual_seed(B)
    Ub, Ib = torch.randn(B, 8, generator=g), torch.randn(B, 8, generator=g)
    ar = torch.arange(B)
    a, _ = IB.in_batch_loss64(Ub, Ib, None, None, tau, ar, ar)
    b, _ = IB.in_batch_loss64(Ub, Ib, None, None, tau)
    s = IB.sampled_form(IB.logits64(Ub, Ib, 1.0))
    assert torch.equal(s[:, 0], torch.diagonal(IB.logits64(Ub, Ib, 1.0))) and s.shape == (B, B)
    want = R.mul_loss64(s, "softmax", tau)
    assert float(a) == float(b)
    assert abs(float(a) - float(want)) <= 1e-13 * max(1.0, abs(float(want)))


def test_fully_masked_row_has_zero_loss_and_zero_gradient():
    """Every pair names one item: every off-diagonal entry is masked, lse_b = z_bb, loss 0 and gradient 0 -- and one such row
    among normal rows contributes nothing."""
    g = torch.Generator().manual_seed(3)
    B, D = 6, 5
    Ub = torch.randn(B, D, generator=g, dtype=torch.float64).requires_grad_()
    Ib = torch.randn(B, D, generator=g, dtype=torch.float64).requires_grad_()
    loss, _ = IB.in_batch_loss64(Ub, Ib, None, None, 0.1, torch.arange(B), torch.zeros(B, dtype=torch.int64))
    loss.backward()
    assert float(loss) == 0.0 and float(Ub.grad.abs().max()) == 0.0 and float(Ib.grad.abs().max()) == 0.0
    # row 0 shares its user with rows 1, 2 and its item with rows 3 .. 5: fully masked; the others keep live columns
    uid, iid = torch.tensor([0, 0, 0, 3, 4, 5]), torch.tensor([0, 1, 2, 0, 0, 0])
    assert IB.mask(uid, iid)[0, 1:].all() and not IB.mask(uid, iid)[1:].all(1).any()
    Ub.grad = Ib.grad = None
    z = IB.logits64(Ub, Ib, 0.1)
    rows = IB.lse64(z, IB.mask(uid, iid)) - torch.diagonal(z)
    assert float(rows[0]) == 0.0 and float(rows[1:].min()) > 0.0
    g0 = torch.autograd.grad(rows[0], (Ub, Ib))
    assert float(g0[0].abs().max()) == 0.0 and float(g0[1].abs().max()) == 0.0


def test_defaults_and_accepted_values():
    for model in ("lightgcn", "ngcf", "tgcn", "dgcf", "disengcn", "kgat"):
        cfg = T.get_config(model)
        assert cfg["negatives"] == "sampled" and cfg["in_batch_logq"] is False
        assert C.check_negatives(cfg) == (False, False)
    assert T.disenhan_config()["negatives"] == "sampled"
    assert C.check_negatives({}) == (False, False)                    # a hand-built config without the keys: the defaults
    cfg = T.get_config("lightgcn", negatives="in_batch", mul_loss_func="softmax", loss_temperature=0.05, in_batch_logq=True)
    assert C.check_negatives(cfg) == (True, True) and C.check_ranking(cfg) == (1, "softmax", 0.05)
    assert C.check_negatives(T.get_config("ngcf", negatives="in_batch", mul_loss_func="softmax")) == (True, False)
    assert C.NEGATIVES_MODES == ("sampled", "in_batch")


@pytest.mark.parametrize("bad", [dict(negatives="in_batch"),                                           # softplus, the default
                                 dict(negatives="in_batch", mul_loss_func="softplus"),
                                 dict(negatives="in_batch", mul_loss_func="logsigmoid"),
                                 dict(negatives="in_batch", mul_loss_func="softmax", n_negatives=4),
                                 dict(negatives="in_batch", mul_loss_func="softmax", in_batch_logq=1),
                                 dict(negatives="batch", mul_loss_func="softmax"), dict(negatives=None), dict(negatives=True),
                                 dict(in_batch_logq=True), dict(in_batch_logq="yes")])
def test_bad_combinations_are_refused(bad):
    with pytest.raises(T.TagrecError):
        T.get_config("lightgcn", **bad)
    with pytest.raises(T.TagrecError):
        C.check_negatives(bad)


def test_in_batch_route():
    q = torch.zeros(5)
    assert H.in_batch_route("m", torch.zeros(8, 2, dtype=torch.int64), 0.5) == H.InBatchRoute(0.5, None)
    r = H.in_batch_route("m", torch.zeros(8, 2, dtype=torch.int64), 2, q)
    assert r.temperature == 2.0 and r.item_logq is q
    for batch in (torch.zeros(8, 3, dtype=torch.int64), torch.zeros(8, 1, dtype=torch.int64), torch.zeros(8, dtype=torch.int64)):
        with pytest.raises(T.TagrecError, match="in_batch"):
            H.in_batch_route("m", batch, 1.0)


IN_BATCH = dict(negatives="in_batch", mul_loss_func="softmax")
REFUSING = [(T.TGCN, lambda **kw: T.get_config("tgcn", **kw)), (T.DGCF, lambda **kw: T.get_config("dgcf", **kw)),
            (T.DisenGCN, lambda **kw: T.get_config("disengcn", **kw)), (T.KGAT, lambda **kw: T.get_config("kgat", **kw)),
            (T.DisenHAN, T.disenhan_config), (T.DGCF_training_data, lambda **kw: T.get_config("dgcf", **kw))]


@pytest.mark.parametrize("cls,make", REFUSING, ids=[c.__name__ for c, _ in REFUSING])
def test_models_without_the_loss_refuse_at_construction(cls, make):
    with pytest.raises(T.TagrecError, match="in_batch"):
        cls(None, config=make(**IN_BATCH))
    cfg = make()
    cfg["negatives"] = "in_batch"                                      # a hand-edited config that skipped get_config's check
    with pytest.raises(T.TagrecError, match="in_batch"):
        cls(None, config=cfg)


@pytest.mark.parametrize("cls", [dist.ShardedLightGCN, dist.ShardedNGCF, dist.FeatureShardedLightGCN])
def test_sharded_models_refuse_at_construction(cls):
    with pytest.raises(T.TagrecError, match="in_batch"):
        cls(None, T.get_config("lightgcn", **IN_BATCH), None, None, None, 0)


def test_item_logq_against_a_numpy_count():
    """log(train degree / train edges) in float64, rounded to fp32; degree 0 gives 0."""
    ds = T.synth.make_cf_dataset(30, 25, 200, seed=4)
    edges = np.asarray(ds.edge_index["train"].cpu() if torch.is_tensor(ds.edge_index["train"]) else ds.edge_index["train"])
    n_item = 25 + 3                                                    # three items no edge names
    got = H.item_logq_table(ds.edge_index["train"], n_item, "cpu")
    assert got.dtype == torch.float32 and got.shape == (n_item,)
    want = np.zeros(n_item)
    for i in range(n_item):
        d = int((edges[:, 1] == i).sum())
        want[i] = math.log(d / len(edges)) if d else 0.0
    assert np.array_equal(got.numpy(), want.astype(np.float32))
    assert (got[25:] == 0).all() and float(got[:25].max()) <= 0.0
    assert torch.equal(H.item_logq_table(torch.as_tensor(edges), n_item, "cpu"), got)      # an array or a tensor
