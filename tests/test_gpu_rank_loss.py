"""GPU: the multi-negative ranking kernels (csrc/rowops.hip rank_fwd_kernel / rank_bwd_kernel) through rowops.rank_fwd /
rank_bwd and help.ranking_loss, against the fp64 restatement of tests/ranking_torch.py.

Tolerance: this repository's rule (tests/test_gpu_rowops.py): |got - ref64| <= c * 2^-24 * mag + extra,
`c` counted off the new kernels and written beside each check; `extra` carries an error that enters through a slope (the
scores under the soft-max / the sigmoid) and is itself such a count.  The counts, once:

  score s_j           a D-term dot: D.  z_j = s_j * (1 / tau): the float 1 / tau and the product, D + 2.
  softmax             a_j = z_j - max (1), e_j = expf(a_j) (4 ulp = 8), S = sum of K + 1 such terms: relative error
                      8 + K + 1 plus, through the slope, sum_i p_i da_i.
     coef_j, j >= 1   e_j / S * (1 / tau): 8 + (K + 9) + divide + product + the float 1 / tau = K + 20; slope: p_j (da_j + sum_i p_i da_i) / tau
     coef_0           minus the sum of the K others: K more additions
     loss_b           logf(S) (8) + (max - z_0) (1) and their sum (1); the block partial, the float 1 / B and the cast: 5 -> 15
                      on |log S| + |max - z_0|; extra: S's relative error, and the errors of max and z_0
  pairwise            as the triplet kernel: coef 2 (add, divide), + 2 for the float 1 / K and its product; the gap's error
                      ((D + 1) on both dots' terms) and expf's 8 through the slope sigma (1 - sigma) / K.
     loss_b           17 per pair (triplet kernel), K additions, 2 for 1 / K, 5 as above
  L2                  (2 + K) Dreg fmas + 5
  backward            (g0 / B) coef_j: 3 roundings.  dI: one product more, 4.  dU: K + 1 fmas, K + 4.  L2 rows: g1 / B (2) and the
                      product, 3; into the SAME buffer it joins by one fma: dI 5, dU K + 5.
Each test prints its worst err / bound (`-s`)."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import tagrec_amd as T
from tagrec_amd import _lib, help as H, rowops

import ranking_torch as R
from spmm_ref import U32, Chk, f64 as _f64, randn as _randn, same_bits as _same_bits

DEV = torch.device("cuda:0")
KIND = {"softplus": _lib.LOSS_SOFTPLUS, "logsigmoid": _lib.LOSS_LOGSIGMOID, "softmax": _lib.LOSS_SOFTMAX}
KS = (1, 2, 15, 63)             # both ends, a non-power-of-two
BS = (1, 3, 4, 5, 130)          # around the four tuples of a block, a ragged last block, more than one partial
DS = (8, 64, 100, 256)          # below a wave, one trip, a ragged second trip, four trips (all held in registers)
# every loss kind; tau only enters the softmax
RUNS = (("softmax", 1.0), ("softmax", 0.05), ("softplus", 1.0), ("logsigmoid", 0.05))


def _t64(a):
    return torch.from_numpy(np.asarray(a, dtype=np.float64))


def _fwd_ref(Ub, Ib, Urb, Irb, K, name, tau):
    """fp64 loss parts and coef of compact operands, each with (mag, c, extra) of the rule above.
    -> {"coef": (ref, mag, c, extra), "loss": ..., "reg": ... or None}"""
    B, D = Ub.shape
    u, it = _f64(Ub), _f64(Ib).reshape(1 + K, B, D)
    terms = u[None] * it
    s, smag = terms.sum(-1).T, np.abs(terms).sum(-1).T                      # [B, 1 + K]
    out = {}
    if name == "softmax":
        tau = float(np.float32(tau))                                         # the float the ABI takes
        z, dz = s / tau, (D + 2) * U32 * smag / tau
        jm = z.argmax(1)
        m, dm = z.max(1), dz[np.arange(B), jm]
        a = z - m[:, None]
        da = dz + dm[:, None] + U32 * np.abs(a)
        e = np.exp(a)
        S = e.sum(1)
        p = e / S[:, None]
        pda = (p * da).sum(1)
        coef = p / tau
        coef[:, 0] = -(p[:, 1:].sum(1)) / tau
        cmag = np.abs(coef)
        cmag[:, 0] = np.abs(coef[:, 1:]).sum(1)
        c = np.full((B, 1 + K), K + 20.0)
        c[:, 0] = 2 * K + 20
        extra = p / tau * (da + pda[:, None])
        extra[:, 0] = extra[:, 1:].sum(1)
        out["coef"] = (coef, cmag, c, extra)
        lb = np.log(S) + (m - z[:, 0])
        ref = float(R.mul_loss64(_t64(s), "softmax", tau))
        assert abs(lb.mean() - ref) <= 1e-12 * max(1.0, abs(ref))           # the restatement (torch.logsumexp) says the same
        lmag = np.abs(np.log(S)) + np.abs(m - z[:, 0])
        lextra = (K + 9) * U32 + pda + dm + dz[:, 0]
        out["loss"] = (ref, lmag.mean(), 15, lextra.mean())
    else:
        x = s[:, 1:] - s[:, :1]
        dx = (D + 1) * U32 * (smag[:, 1:] + smag[:, :1])
        sig = 1.0 / (1.0 + np.exp(-x))
        cneg = R.coef64(_t64(s), name)[:, 1:].numpy()                        # autograd of the restatement: pass-through past 20
        slope = sig * (1 - sig) * (dx + 8 * U32) / K
        coef = np.concatenate([-cneg.sum(1, keepdims=True), cneg], 1)
        cmag = np.abs(coef)
        c = np.full((B, 1 + K), 4.0)
        c[:, 0] = 4 + K
        extra = np.concatenate([slope.sum(1, keepdims=True), slope], 1)
        out["coef"] = (coef, cmag, c, extra)
        ref = float(R.mul_loss64(_t64(s), name))
        f = R.pair_loss64(_t64(x), name).numpy()
        out["loss"] = (ref, f.mean(), K + 24, (sig * dx).mean())
    if Urb is not None:
        Dr = Urb.shape[1]
        ss = 0.5 * ((_f64(Urb) ** 2).sum(1) + (_f64(Irb).reshape(1 + K, B, Dr) ** 2).sum(-1).sum(0))
        out["reg"] = (ss.mean(), ss.mean(), (2 + K) * Dr + 5, 0.0)
    else:
        out["reg"] = None
    return out


def _check_fwd(chk, tag, ref, res, coef):
    chk.close(tag + "coef", coef, *ref["coef"])
    chk.close(tag + "loss", res[0], *ref["loss"])
    if ref["reg"] is None:
        assert float(res[1]) == 0.0
    else:
        chk.close(tag + "reg", res[1], *ref["reg"])


def _bwd_ref(Ub, Ib, Urb, Irb, K, coef, g, main=True, shared=False):
    """fp64 gradients from the kernel's own inputs (its coef included) -> {name: (ref, mag, c)}."""
    B, D = Ub.shape
    g0, g1 = (1.0, 1.0) if g is None else (float(np.float32(g[0])), float(np.float32(g[1])))
    u, it = _f64(Ub), _f64(Ib).reshape(1 + K, B, D)
    out = {}
    if main:
        cl = (g0 / B) * _f64(coef).T[:, :, None]                             # [1 + K, B, 1]
        out["dU"] = [(cl * it).sum(0), np.abs(cl * it).sum(0), K + 4]
        out["dI"] = [(cl * u[None]).reshape(-1, D), np.abs(cl * u[None]).reshape(-1, D), 4]
    if Urb is not None:
        cr = g1 / B
        ur, ir = cr * _f64(Urb), cr * _f64(Irb)
        if shared:
            for k, r in (("dU", ur), ("dI", ir)):
                out[k] = [out[k][0] + r, out[k][1] + np.abs(r), out[k][2] + 1]
        else:
            out["dUr"], out["dIr"] = [ur, np.abs(ur), 3], [ir, np.abs(ir), 3]
    return out


def _operands(B, K, D, seed, pad=0, scale=0.35, Dr=None):
    """Ub [B, D], Ib [(1 + K) B, D] (+ L2 operands of width Dr) on the GPU; pad > 0: slots of NaN-padded wider buffers."""
    def slot(n, d, sd):
        buf = torch.full((n, d + pad), float("nan"))
        buf[:, :d] = _randn(n, d, seed=sd, scale=scale)
        return buf.to(DEV)[:, :d]
    Ub, Ib = slot(B, D, seed), slot((1 + K) * B, D, seed + 1)
    if Dr is None:
        return Ub, Ib, None, None
    return Ub, Ib, slot(B, Dr, seed + 2), slot((1 + K) * B, Dr, seed + 3)


def _nan_like(t, pad=0):
    return torch.full((t.shape[0], t.shape[1] + pad), float("nan"), device=DEV)[:, :t.shape[1]]


def _run(chk, B, K, D, name, tau, seed, pad=0, g=(0.37, -2.0)):
    """Forward and the backward forms (distinct L2 rows, L2 only, one shared buffer, no L2) on one operand set."""
    tag = f"{name}/{tau} "
    Dr = D + 3
    Ub, Ib, Urb, Irb = _operands(B, K, D, seed, pad, Dr=Dr)
    res, coef = rowops.rank_fwd(Ub, Ib, Urb, Irb, KIND[name], tau)
    assert coef.shape == (B, K + 1)
    _check_fwd(chk, tag, _fwd_ref(Ub, Ib, Urb, Irb, K, name, tau), res, coef)
    gg = None if g is None else torch.tensor(g, dtype=torch.float32, device=DEV)
    # distinct L2 rows; every output pre-filled with NaN must be fully overwritten (chk.close refuses a non-finite value)
    dU, dI, dUr, dIr = _nan_like(Ub, pad), _nan_like(Ib, pad), _nan_like(Urb, pad), _nan_like(Irb, pad)
    rowops.rank_bwd(Ub, Ib, Urb, Irb, coef, gg, dU, dI, dUr, dIr)
    ref = _bwd_ref(Ub, Ib, Urb, Irb, K, coef, g)
    for k, got in (("dU", dU), ("dI", dI), ("dUr", dUr), ("dIr", dIr)):
        chk.close(tag + k, got, *ref[k])
    # two launches: the same bits (no atomics, nothing read from the outputs)
    dU2, dI2, dUr2, dIr2 = _nan_like(Ub, pad), _nan_like(Ib, pad), _nan_like(Urb, pad), _nan_like(Irb, pad)
    rowops.rank_bwd(Ub, Ib, Urb, Irb, coef, gg, dU2, dI2, dUr2, dIr2)
    assert all(_same_bits(a, b) for a, b in ((dU, dU2), (dI, dI2), (dUr, dUr2), (dIr, dIr2)))
    # dU = dI = None: the L2 part only, same bits as above
    dUr3, dIr3 = _nan_like(Urb, pad), _nan_like(Irb, pad)
    rowops.rank_bwd(Ub, Ib, Urb, Irb, coef, gg, None, None, dUr3, dIr3)
    assert _same_bits(dUr3, dUr) and _same_bits(dIr3, dIr)
    # no L2 part: the main part alone, same bits
    dU4, dI4 = _nan_like(Ub, pad), _nan_like(Ib, pad)
    rowops.rank_bwd(Ub, Ib, None, None, coef, gg, dU4, dI4, None, None)
    assert _same_bits(dU4, dU) and _same_bits(dI4, dI)
    # L2 on the score rows themselves, one buffer for both parts (NGCF)
    res5, coef5 = rowops.rank_fwd(Ub, Ib, Ub, Ib, KIND[name], tau)
    assert _same_bits(coef5, coef) and _same_bits(res5[0], res[0])
    dU5, dI5 = _nan_like(Ub, pad), _nan_like(Ib, pad)
    rowops.rank_bwd(Ub, Ib, Ub, Ib, coef, gg, dU5, dI5, dU5, dI5)
    ref5 = _bwd_ref(Ub, Ib, Ub, Ib, K, coef, g, shared=True)
    chk.close(tag + "dU(shared)", dU5, *ref5["dU"])
    chk.close(tag + "dI(shared)", dI5, *ref5["dI"])
    return (Ub, Ib, Urb, Irb), (dU, dI, dUr, dIr)


@pytest.mark.parametrize("D", DS)
@pytest.mark.parametrize("B", BS)
@pytest.mark.parametrize("K", KS)
def test_rank_kernels_against_fp64(K, B, D):
    chk = Chk(f"rank K={K} B={B} D={D}", tag="rank")
    for i, (name, tau) in enumerate(RUNS):
        _run(chk, B, K, D, name, tau, seed=1000 * K + 10 * B + D + i)
    chk.done()


@pytest.mark.parametrize("name,tau", RUNS)
def test_rank_strided_rows_nan_padding(name, tau):
    """ld > D: the operands and the gradient buffers are slots of wider buffers whose padding columns hold NaN; nothing reads
    or writes them."""
    chk = Chk(f"rank strided {name}/{tau}", tag="rank")
    B, K, D, pad = 5, 15, 100, 4
    ops, grads = _run(chk, B, K, D, name, tau, seed=77, pad=pad)
    for t in ops + grads:
        assert t.stride(0) == t.shape[1] + pad
        whole = torch.as_strided(t, (t.shape[0], t.shape[1] + pad), (t.stride(0), 1))
        assert torch.isnan(whole[:, t.shape[1]:]).all() and torch.isfinite(whole[:, :t.shape[1]]).all()
    chk.done()


def _forced(scores, D=4):
    """Compact operands whose scores are exactly `scores` [B, 1 + K] (fp32 values): user row 2 e_0, item row (s / 2) e_0."""
    s = torch.as_tensor(np.float32(scores))
    B, K1 = s.shape
    Ub = torch.zeros(B, D)
    Ub[:, 0] = 2.0
    Ib = torch.zeros(K1 * B, D)
    Ib[:, 0] = s.t().reshape(-1) / 2
    return Ub.to(DEV), Ib.to(DEV)


@pytest.mark.parametrize("tau", [1.0, 0.05])
def test_softmax_large_scores_are_finite_and_underflow_to_zero(tau):
    """Scores of magnitude 60 / tau (logits up to +-1200 at tau = 0.05): the maximum is subtracted, so loss and coef are
    finite, and a weight whose exponent lies below fp32's range is an exact zero."""
    chk = Chk(f"rank large scores tau={tau}", tag="rank")
    scores = np.float32([[-60.0, 60.0, 0.0, 59.0], [60.0, -60.0, 0.0, 59.5], [0.0, 0.0, 0.0, 0.0], [60.0, 60.0, -60.0, -60.0],
                         [-60.0, -59.0, -60.0, -60.0]])
    Ub, Ib = _forced(scores)
    res, coef = rowops.rank_fwd(Ub, Ib, None, None, _lib.LOSS_SOFTMAX, tau)
    assert torch.isfinite(res).all() and torch.isfinite(coef).all()
    _check_fwd(chk, "", _fwd_ref(Ub, Ib, None, None, 3, "softmax", tau), res, coef)
    z = scores.astype(np.float64) / float(np.float32(tau))
    under = (z - z.max(1, keepdims=True)) < -110.0                            # expf's range ends near -103.97
    under[:, 0] = False                                                        # (entry 0 is minus the sum of the others)
    assert under.any() and (coef.cpu().numpy()[under] == 0.0).all()
    assert float(res[0]) > 100.0 / 5                                          # row 0 alone contributes 120 / tau / 5
    dU, dI = _nan_like(Ub), _nan_like(Ib)
    rowops.rank_bwd(Ub, Ib, None, None, coef, None, dU, dI, None, None)
    assert torch.isfinite(dU).all() and torch.isfinite(dI).all()
    chk.done()


GAPS = (-100.0, -20.5, 0.0, 19.99, 20.0, 20.01, 25.0, 100.0)


@pytest.mark.parametrize("name", ["softplus", "logsigmoid"])
def test_pairwise_kinds_pass_the_gradient_through_past_20(name):
    """One tuple whose K negatives sit at the gaps above: past 20 softplus returns the gap and its gradient is exactly 1 / K
    (torch's threshold); the restatement's autograd says the same."""
    chk = Chk(f"rank gaps {name}", tag="rank")
    K = len(GAPS)
    scores = np.float32([[0.0] + list(GAPS), [3.0] + [3.0 + x for x in GAPS]])
    Ub, Ib = _forced(scores)
    res, coef = rowops.rank_fwd(Ub, Ib, None, None, KIND[name], 1.0)
    _check_fwd(chk, "", _fwd_ref(Ub, Ib, None, None, K, name, 1.0), res, coef)
    c = coef.cpu().numpy()
    past = np.float32(GAPS) > 20.0
    if name == "softplus":
        assert (c[0, 1:][past] == np.float32(1.0) / np.float32(K)).all()
        want = R.coef64(_t64(scores[:1]), "softplus").numpy()[0, 1:]
        assert (want[past] == 1.0 / K).all()
    assert (c[0, 1:][np.float32(GAPS) <= 0.0] <= np.float32(0.5) / np.float32(K)).all()
    chk.done()


@pytest.mark.parametrize("D,B", [(64, 130), (100, 5), (8, 1)])
@pytest.mark.parametrize("name", ["softplus", "logsigmoid", "softmax"])
def test_one_negative_agrees_with_the_triplet_kernels(name, D, B):
    """K = 1: rank_fwd / rank_bwd against rowops.bpr_fwd / bpr_bwd on compact triplets (softmax at tau = 1 against the
    softplus triplet kernel: the same function).  Both sides obey the rule against fp64, so their difference is bounded by
    the sum of the two bounds: the counts of this file's header plus those of tests/test_gpu_rowops.py (coef 2, loss 22,
    reg 3 Dreg + 5, dU 5 and dI 4 plus one atomic addition each)."""
    chk = Chk(f"rank K=1 vs bpr {name} D={D} B={B}", tag="rank")
    Ub, Ib, Urb, Irb = _operands(B, 1, D, seed=5 * D + B, Dr=D + 3)
    ctrip = rowops.compact_triplets(B, DEV)
    bkind = _lib.LOSS_LOGSIGMOID if name == "logsigmoid" else _lib.LOSS_SOFTPLUS
    res_b, coef_b = rowops.bpr_fwd(Ub, Ib, Urb, Irb, ctrip, bkind)
    res, coef = rowops.rank_fwd(Ub, Ib, Urb, Irb, KIND[name], 1.0)
    ref = _fwd_ref(Ub, Ib, Urb, Irb, 1, name, 1.0)
    u, it = _f64(Ub), _f64(Ib).reshape(2, B, D)
    smag = np.abs(u[None] * it).sum(-1).T
    x = (u[None] * it).sum(-1).T
    x = x[:, 1] - x[:, 0]
    sig = 1 / (1 + np.exp(-x))
    dx = (D + 1) * U32 * smag.sum(1)
    r, m, c, e = ref["coef"]
    chk.close("coef", coef[:, 1], _f64(coef_b), m[:, 1], c[:, 1] + 2, e[:, 1] + sig * (1 - sig) * (dx + 8 * U32))
    chk.close("coef0", coef[:, 0], -_f64(coef_b), m[:, 0], c[:, 0] + 2, e[:, 0] + sig * (1 - sig) * (dx + 8 * U32))
    r, m, c, e = ref["loss"]
    chk.close("loss", res[0], _f64(res_b[0]), m, c + 22, e + (sig * dx).mean())
    r, m, c, e = ref["reg"]
    chk.close("reg", res[1], _f64(res_b[1]), m, 2 * c)
    g = torch.tensor([0.37, -2.0], device=DEV)
    z = [torch.zeros_like(t) for t in (Ub, Ib, Urb, Irb)]
    rowops.bpr_bwd(Ub, Ib, Urb, Irb, ctrip, coef_b, g, *z)
    o = [_nan_like(t) for t in (Ub, Ib, Urb, Irb)]
    # the triplet kernel's coef drives both, so that only the two backward kernels are compared
    coef_in = torch.stack([-coef_b, coef_b], 1).contiguous()
    rowops.rank_bwd(Ub, Ib, Urb, Irb, coef_in, g, *o)
    bref = _bwd_ref(Ub, Ib, Urb, Irb, 1, coef_in, [0.37, -2.0])
    for k, got, want, cb in (("dU", o[0], z[0], 5 + 1), ("dI", o[1], z[1], 4 + 1), ("dUr", o[2], z[2], 3 + 1), ("dIr", o[3], z[3], 3 + 1)):
        chk.close(k, got, _f64(want), bref[k][1], bref[k][2] + cb)
    chk.done()


def test_rank_refuses_bad_arguments():
    Ub, Ib, _, _ = _operands(4, 2, 8, seed=1)
    with pytest.raises(T.TagrecError):
        rowops.rank_fwd(Ub, Ib[:11], None, None, _lib.LOSS_SOFTMAX)                       # (1 + K) B rows
    with pytest.raises(T.TagrecError):
        rowops.rank_fwd(Ub[:1], torch.zeros(65, 8, device=DEV), None, None, _lib.LOSS_SOFTMAX)  # K = 64
    with pytest.raises(T.TagrecError):
        rowops.rank_fwd(Ub, Ib, Ub, None, _lib.LOSS_SOFTMAX)
    with pytest.raises(T.TagrecError):
        rowops.rank_fwd(Ub, Ib, None, None, 7)
    for tau in (0.0, -1.0, float("inf"), float("nan")):
        with pytest.raises(T.TagrecError):
            rowops.rank_fwd(Ub, Ib, None, None, _lib.LOSS_SOFTMAX, tau)
    with pytest.raises(T.TagrecError):                                                     # one row stride for both tables
        rowops.rank_fwd(Ub, torch.zeros(12, 12, device=DEV)[:, :8], None, None, _lib.LOSS_SOFTMAX)
    res, coef = rowops.rank_fwd(Ub, Ib, None, None, _lib.LOSS_SOFTMAX)
    dU, dI = torch.empty_like(Ub), torch.empty_like(Ib)
    with pytest.raises(T.TagrecError):
        rowops.rank_bwd(Ub, Ib, None, None, coef[:, :2].contiguous(), None, dU, dI, None, None)
    with pytest.raises(T.TagrecError):
        rowops.rank_bwd(Ub, Ib, None, None, coef, None, dU, None, None, None)
    with pytest.raises(T.TagrecError):                                                     # a shared buffer needs Ureg = Ub
        rowops.rank_bwd(Ub, Ib, Ub.clone(), Ib.clone(), coef, None, dU, dI, dU, dI)
    with pytest.raises(T.TagrecError):                                                     # the triplet kernel has no softmax
        rowops.bpr_fwd(Ub, Ib, None, None, rowops.compact_triplets(4, DEV), _lib.LOSS_SOFTMAX)


# ====================================================================================================== help.ranking_loss
def _tables_and_tuples(nu=50, ni=60, D=64, B=40, K=3, seed=21):
    """Tables and a batch that names user 7 twenty times, item 3 as a positive, as two negatives of other tuples and twice
    within one tuple."""
    g = torch.Generator().manual_seed(seed)
    W = _randn(nu + ni, D, seed=seed, scale=0.35).to(DEV)
    E = _randn(nu + ni, D, seed=seed + 1, scale=0.35).to(DEV)
    tup = torch.cat([torch.randint(0, nu, (B, 1), generator=g), torch.randint(0, ni, (B, 1 + K), generator=g)], 1)
    tup[:20, 0] = 7
    tup[1, 1], tup[2, 2], tup[3, 3] = 3, 3, 3
    tup[4, 2], tup[4, 3] = 3, 3
    return W, E, tup


def _scatter64(n_rows, idx, terms, mags):
    out, mag, mult = np.zeros((n_rows, terms.shape[1])), np.zeros((n_rows, terms.shape[1])), np.zeros((n_rows, 1))
    np.add.at(out, idx, terms)
    np.add.at(mag, idx, mags)
    np.add.at(mult, idx, 1.0)
    return out, mag, mult


@pytest.mark.parametrize("name,tau", [("softmax", 0.5), ("softplus", 1.0)])
@pytest.mark.parametrize("same", [False, True])
def test_ranking_loss_on_tables(name, tau, same):
    """help.ranking_loss: loss parts against the restatement on the tables; gradients against the fp64 scatter of the
    compact kernel's terms (its own coef, as in the triplet tests), c = the compact count + the row's multiplicity (one
    addition of the fold per slot that names the row).  same: the L2 tables are the score tables (one buffer)."""
    chk = Chk(f"ranking_loss {name} same={same}", tag="rank")
    nu, ni, B, K = 50, 60, 40, 3
    W, E, tup = _tables_and_tuples(nu, ni, B=B, K=K)
    tg = tup.to(DEV)
    U, I = W[:nu].clone().requires_grad_(), W[nu:].clone().requires_grad_()
    Ur, Ir = (U, I) if same else (E[:nu].clone().requires_grad_(), E[nu:].clone().requires_grad_())
    loss, reg = H.ranking_loss(U, I, Ur, Ir, tg, name, tau)
    rows = rowops.tuple_rows(tg, nu)
    Ub, Ib = W.index_select(0, rows[:B]), W.index_select(0, rows[B:])
    Eb = W if same else E
    Urb, Irb = Eb.index_select(0, rows[:B]), Eb.index_select(0, rows[B:])
    ref = _fwd_ref(Ub, Ib, Urb, Irb, K, name, tau)
    want = R.ranking_loss64(W[:nu].cpu(), W[nu:].cpu(), Eb[:nu].cpu(), Eb[nu:].cpu(), tup, name, float(np.float32(tau)))
    assert abs(float(want[0]) - ref["loss"][0]) <= 1e-12 and abs(float(want[1]) - ref["reg"][0]) <= 1e-12
    chk.close("loss", loss, *ref["loss"])
    chk.close("reg", reg, *ref["reg"])
    g = [0.37, -2.0]
    (g[0] * loss + g[1] * reg).backward()
    _, coef = rowops.rank_fwd(Ub, Ib, Urb, Irb, KIND[name], tau)
    b = _bwd_ref(Ub, Ib, Urb, Irb, K, coef, g, shared=same)
    ur, ir = tup[:, 0].numpy(), tup[:, 1:].t().reshape(-1).numpy()
    checks = [("dU", U.grad, nu, ur), ("dI", I.grad, ni, ir)] + ([] if same else [("dUr", Ur.grad, nu, ur), ("dIr", Ir.grad, ni, ir)])
    for k, got, n, idx in checks:
        s, m, mult = _scatter64(n, idx, b[k][0], b[k][1])
        chk.close(k, got, s, m, b[k][2] + mult)
    assert float(np.max(_scatter64(nu, ur, b["dU"][0], b["dU"][1])[2])) >= 20.0     # user 7's multiplicity
    chk.done()


def test_ranking_loss_planned_fold_is_reproducible():
    """With plans the compact gradients are folded in a fixed order: the same bits on every run, within the same bound."""
    chk = Chk("ranking_loss planned", tag="rank")
    nu, ni, B, K = 50, 60, 40, 3
    W, E, tup = _tables_and_tuples(nu, ni, B=B, K=K)
    tg = tup.to(DEV)
    grads = []
    for _ in range(2):
        U, I = W[:nu].clone().requires_grad_(), W[nu:].clone().requires_grad_()
        Ur, Ir = E[:nu].clone().requires_grad_(), E[nu:].clone().requires_grad_()
        plans = H.ranking_plans(tg, nu, ni, W.shape[1])
        loss, reg = H.ranking_loss(U, I, Ur, Ir, tg, "softmax", 0.5, plans=plans)
        (loss + 0.1 * reg).backward()
        grads.append([t.grad.clone() for t in (U, I, Ur, Ir)] + [loss.detach().clone(), reg.detach().clone()])
    assert all(_same_bits(a, b) for a, b in zip(*grads))
    rows = rowops.tuple_rows(tg, nu)
    Ub, Ib = W.index_select(0, rows[:B]), W.index_select(0, rows[B:])
    Urb, Irb = E.index_select(0, rows[:B]), E.index_select(0, rows[B:])
    _, coef = rowops.rank_fwd(Ub, Ib, Urb, Irb, _lib.LOSS_SOFTMAX, 0.5)
    b = _bwd_ref(Ub, Ib, Urb, Irb, K, coef, [1.0, 0.1])
    ur, ir = tup[:, 0].numpy(), tup[:, 1:].t().reshape(-1).numpy()
    for k, got, n, idx in (("dU", grads[0][0], nu, ur), ("dI", grads[0][1], ni, ir), ("dUr", grads[0][2], nu, ur), ("dIr", grads[0][3], ni, ir)):
        s, m, mult = _scatter64(n, idx, b[k][0], b[k][1])
        chk.close(k, got, s, m, b[k][2] + mult)
    chk.done()
