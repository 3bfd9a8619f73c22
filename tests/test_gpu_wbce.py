"""GPU: the weighted pointwise BCE kernels (csrc/rowops.hip wbce_fwd_kernel / wbce_bwd_kernel) through rowops.wbce_fwd /
wbce_bwd, against the fp64 restatement of tests/ultragcn_torch.py.

Tolerance: this repository's rule (tests/test_gpu_rowops.py): |got - ref64| <= c * 2^-24 * mag + extra, `c`
counted off the new kernels; `extra` carries the score's error through a slope.  The counts, once:

  score s_j     a D-term dot: D (ds = D 2^-24 sum |u| |i|).  x = -t s is exact.
  softplus      expf (4 ulp = 8), log1pf (8), the sum with max(x, 0) (1): 17; times the weight: 18.  A tuple's terms are summed
                in fp64; the block partial's cast (1), the float 1 / B (1), the product (1) and the final cast (1): 22 -> 24 on
                mean_b sum_j w softplus; extra: the slope, mean_b sum_j w sigmoid(x) ds
  coef          expf (8), 1 + e (1), the divide (1), times -t w (1), times the float 1 / B (2): 13 -> 14; extra: w sigmoid
                (1 - sigmoid) ds / B
  L2            per row a Dreg-term sum of squares, rows and tuples summed in fp64, then as the loss: Dreg + 5
  backward      c = g0 coef (1).  dI = c u: 2 -> 3.  dU: S fmas: S + 2.  L2 rows: (g1 / B) x: 3; a neighbour slot's L2 row is an
                exact 0.  Into the SAME buffer the L2 term joins by one fma: dI 5, dU S + 4.
Each test prints its worst err / bound (`-s`)."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import tagrec_amd as T
from tagrec_amd import rowops

import ultragcn_torch as UT
from spmm_ref import U32, Chk, f64 as _f64, randn as _randn, same_bits as _same_bits

DEV = torch.device("cuda:0")
BS = (1, 3, 4, 5, 130)          # around the four tuples of a block, a ragged last block, more than one partial
DS = (8, 64, 100, 256)          # below a wave, one trip, a ragged second trip, four trips (all held in registers)
KS = (1, 15, 63, 200)           # one negative; below, at and far above the wave width the rank kernels are bound to
MS = (0, 3, 10)


def _operands(B, S, D, seed, pad=0, scale=0.35, Dr=None):
    """Ub [B, D], Ib [S B, D] (+ L2 operands of width Dr) on the GPU; pad > 0: slots of NaN-padded wider buffers."""
    def slot(n, d, sd):
        buf = torch.full((n, d + pad), float("nan"))
        buf[:, :d] = _randn(n, d, seed=sd, scale=scale)
        return buf.to(DEV)[:, :d]
    Ub, Ib = slot(B, D, seed), slot(S * B, D, seed + 1)
    if Dr is None:
        return Ub, Ib, None, None
    return Ub, Ib, slot(B, Dr, seed + 2), slot(S * B, Dr, seed + 3)


def _weights(B, S, seed, zeros=True):
    w = torch.rand(B, S, generator=torch.Generator().manual_seed(seed)) * 2
    if zeros:
        w[:, S - 1] = 0                                       # a zero-weight slot in every tuple (a padded neighbour)
        w[0, 0] = 0
    return w.to(DEV)


def _nan_like(t, pad=0):
    return torch.full((t.shape[0], t.shape[1] + pad), float("nan"), device=DEV)[:, :t.shape[1]]


def _check_fwd(chk, tag, Ub, Ib, Ur, Ir, w, K, M, res, coef):
    B, D = Ub.shape
    S = 1 + K + M
    mul, l2, cref, s = UT.wbce64(Ub.cpu(), Ib.cpu(), w.cpu(), K, M, None if Ur is None else Ur.cpu(), None if Ir is None else Ir.cpu())
    smag = (np.abs(_f64(Ub))[None] * np.abs(_f64(Ib).reshape(S, B, D))).sum(-1).T
    ds = D * U32 * smag
    x = -UT.labels(K, M).numpy()[None] * s.numpy()
    sig = 1.0 / (1.0 + np.exp(-x))
    w64 = _f64(w)
    sp = UT.softplus64(torch.from_numpy(x)).numpy()
    chk.close(tag + "coef", coef, cref.numpy(), np.abs(cref.numpy()), 14, w64 * sig * (1 - sig) * ds / B)
    chk.close(tag + "loss", res[0], float(mul), (w64 * sp).sum() / B, 24, (w64 * sig * ds).sum() / B)
    if Ur is None:
        assert float(res[1]) == 0.0
    else:
        chk.close(tag + "reg", res[1], float(l2), float(l2), Ur.shape[1] + 5)
    zero = (w64 == 0)
    assert (_f64(coef)[zero] == 0).all()                      # a zero weight is an exact zero coefficient
    return zero


def _bwd_ref(Ub, Ib, Urb, Irb, K, M, coef, g, main=True, shared=False):
    """fp64 gradients from the kernel's own inputs (its coef included) -> {name: [ref, mag, c]}."""
    B, D = Ub.shape
    S = 1 + K + M
    g0, g1 = (1.0, 1.0) if g is None else (float(np.float32(g[0])), float(np.float32(g[1])))
    u, it = _f64(Ub), _f64(Ib).reshape(S, B, D)
    out = {}
    if main:
        cl = g0 * _f64(coef).T[:, :, None]                    # [S, B, 1]
        out["dU"] = [(cl * it).sum(0), np.abs(cl * it).sum(0), S + 2]
        out["dI"] = [(cl * u[None]).reshape(-1, D), np.abs(cl * u[None]).reshape(-1, D), 3]
    if Urb is not None:
        cr = g1 / B
        ur, ir = cr * _f64(Urb), cr * _f64(Irb)
        ir[(1 + K) * B:] = 0                                  # the neighbour slots carry no L2
        if shared:
            for k, r in (("dU", ur), ("dI", ir)):
                out[k] = [out[k][0] + r, out[k][1] + np.abs(r), out[k][2] + 2]
        else:
            out["dUr"], out["dIr"] = [ur, np.abs(ur), 3], [ir, np.abs(ir), 3]
    return out


@pytest.mark.parametrize("D", DS)
@pytest.mark.parametrize("B", BS)
def test_forward_and_backward_every_shape(B, D):
    chk = Chk(f"wbce B={B} D={D}", "wbce")
    g = torch.tensor([0.7, 1.3], device=DEV)
    for K in KS:
        for M in MS:
            S = 1 + K + M
            Dr = (D, 24)[(K + M) % 2]                         # L2 rows of the same and of another width
            Ub, Ib, Ur, Ir = _operands(B, S, D, 100 * K + M, pad=3, Dr=Dr)
            w = _weights(B, S, K + 7 * M)
            res, coef = rowops.wbce_fwd(Ub, Ib, Ur, Ir, w, K, M)
            tag = f"K={K} M={M} "
            zero = _check_fwd(chk, tag, Ub, Ib, Ur, Ir, w, K, M, res, coef)
            res2, coef2 = rowops.wbce_fwd(Ub, Ib, Ur, Ir, w, K, M)                     # two launches, the same bits
            assert _same_bits(res, res2) and _same_bits(coef, coef2)
            dU, dI, dUr, dIr = _nan_like(Ub, 3), _nan_like(Ib, 3), _nan_like(Ur, 3), _nan_like(Ir, 3)
            rowops.wbce_bwd(Ub, Ib, Ur, Ir, coef, g, dU, dI, dUr, dIr, K, M)
            ref = _bwd_ref(Ub, Ib, Ur, Ir, K, M, coef, g.cpu().numpy())
            for nm, t in (("dU", dU), ("dI", dI), ("dUr", dUr), ("dIr", dIr)):
                chk.close(tag + nm, t, *ref[nm])                                        # (finite: every NaN was overwritten)
            dI3 = _f64(dI).reshape(S, B, D)
            assert (dI3[zero.T] == 0).all()                   # zero-weight slots: exactly zero rows
            assert (_f64(dIr).reshape(S, B, Dr)[1 + K:] == 0).all()
    chk.done()


def test_no_l2_and_single_slot_edges():
    chk = Chk("wbce no L2", "wbce")
    for B, D, K, M in ((5, 100, 1, 0), (3, 8, 2, 1)):
        S = 1 + K + M
        Ub, Ib, _, _ = _operands(B, S, D, 5)
        w = _weights(B, S, 3, zeros=False)
        res, coef = rowops.wbce_fwd(Ub, Ib, None, None, w, K, M)
        _check_fwd(chk, f"B={B} ", Ub, Ib, None, None, w, K, M, res, coef)
        dU, dI = _nan_like(Ub), _nan_like(Ib)
        rowops.wbce_bwd(Ub, Ib, None, None, coef, None, dU, dI, None, None, K, M)
        ref = _bwd_ref(Ub, Ib, None, None, K, M, coef, None)
        chk.close("dU", dU, *ref["dU"])
        chk.close("dI", dI, *ref["dI"])
    chk.done()


def test_scores_of_plus_minus_60_stay_finite():
    B, D, K, M = 4, 64, 3, 2
    S = 1 + K + M
    Ub = torch.full((B, D), 1.0, device=DEV)
    Ib = torch.full((S * B, D), 60.0 / D, device=DEV)
    Ib[B:2 * B] *= -1                                         # a negative scored -60, the others +60
    w = torch.ones(B, S, device=DEV)
    res, coef = rowops.wbce_fwd(Ub, Ib, Ub, Ib, w, K, M)
    mul, l2, cref, s = UT.wbce64(Ub.cpu(), Ib.cpu(), w.cpu(), K, M, Ub.cpu(), Ib.cpu())
    assert torch.isfinite(res).all() and torch.isfinite(coef).all()
    assert float(s.abs().min()) == 60.0
    chk = Chk("wbce +-60", "wbce")
    chk.close("loss", res[0], float(mul), float(mul), 24, 64 * U32 * 60 * S)      # the big terms are x itself: slope 1
    chk.close("coef", coef, cref.numpy(), np.abs(cref.numpy()), 14, np.abs(cref.numpy()) * 64 * U32 * 60)
    chk.done()


def test_the_four_aliasing_forms_agree():
    """Distinct L2 rows, L2 only, shared buffer, no L2: the main part's bits do not depend on the form, the L2 part's bits are
    the same whether it runs with the main part or alone (as rank_bwd), and the shared buffer holds the fp64 sum."""
    B, D, K, M = 5, 64, 15, 3
    S = 1 + K + M
    Ub, Ib, Ur, Ir = _operands(B, S, D, 11, Dr=D)
    w = _weights(B, S, 2)
    g = torch.tensor([0.9, 0.4], device=DEV)
    res, coef = rowops.wbce_fwd(Ub, Ib, Ur, Ir, w, K, M)
    new = lambda t: _nan_like(t)
    a = [new(Ub), new(Ib), new(Ur), new(Ir)]
    rowops.wbce_bwd(Ub, Ib, Ur, Ir, coef, g, *a, K, M)                                 # distinct L2 rows
    b = [new(Ur), new(Ir)]
    rowops.wbce_bwd(Ub, Ib, Ur, Ir, coef, g, None, None, *b, K, M)                     # L2 only
    c = [new(Ub), new(Ib)]
    rowops.wbce_bwd(Ub, Ib, None, None, coef, g, *c, None, None, K, M)                 # no L2
    assert _same_bits(a[0], c[0]) and _same_bits(a[1], c[1]) and _same_bits(a[2], b[0]) and _same_bits(a[3], b[1])
    res_s, coef_s = rowops.wbce_fwd(Ub, Ib, Ub, Ib, w, K, M)
    assert _same_bits(coef_s, coef) and _same_bits(res_s[:1], res[:1])
    d = [new(Ub), new(Ib)]
    rowops.wbce_bwd(Ub, Ib, Ub, Ib, coef, g, d[0], d[1], d[0], d[1], K, M)             # one buffer for both parts
    d2 = [new(Ub), new(Ib)]
    rowops.wbce_bwd(Ub, Ib, Ub, Ib, coef, g, d2[0], d2[1], d2[0], d2[1], K, M)
    assert _same_bits(d[0], d2[0]) and _same_bits(d[1], d2[1])
    ref = _bwd_ref(Ub, Ib, Ub, Ib, K, M, coef, g.cpu().numpy(), shared=True)
    chk = Chk("wbce shared", "wbce")
    chk.close("dU", d[0], *ref["dU"])
    chk.close("dI", d[1], *ref["dI"])
    chk.done()


def test_bad_arguments_are_refused():
    B, D, K, M = 3, 8, 2, 1
    S = 1 + K + M
    Ub, Ib, _, _ = _operands(B, S, D, 1)
    w = _weights(B, S, 1)
    for kw in (dict(K=0), dict(K=2, M=-1), dict(K=3, M=1), dict(K=4095, M=1), dict(K=2.0)):
        with pytest.raises(T.TagrecError):
            rowops.wbce_fwd(Ub, Ib, None, None, w, kw.get("K", K), kw.get("M", M))
    with pytest.raises(T.TagrecError, match="weight"):
        rowops.wbce_fwd(Ub, Ib, None, None, w[:, :S - 1], K, M)
    with pytest.raises(T.TagrecError):
        rowops.wbce_fwd(Ub, Ib, Ub, None, w, K, M)
    res, coef = rowops.wbce_fwd(Ub, Ib, None, None, w, K, M)
    with pytest.raises(T.TagrecError, match="coef"):
        rowops.wbce_bwd(Ub, Ib, None, None, coef[:, :2], None, _nan_like(Ub), _nan_like(Ib), None, None, K, M)
    with pytest.raises(T.TagrecError, match="rows"):
        rowops.wbce_bwd(Ub, Ib, None, None, coef, None, _nan_like(Ub), _nan_like(Ib)[:B], None, None, K, M)
    # the C entry point itself: L2 gradient buffers without L2 rows are refused (they would take the shared-buffer form)
    from tagrec_amd import _lib
    dU, dI = _nan_like(Ub), _nan_like(Ib)
    rc = _lib.load().tagrec_wbce_bwd_f32(Ub, Ib, Ub.stride(0), D, None, None, 0, 0, B, K, M, coef, None, dU, dI, dU, dI, _lib.stream_ptr())
    assert rc != 0 and "without Ureg" in _lib.load().tagrec_last_error().decode()
    assert torch.isnan(dU).all() and torch.isnan(dI).all()   # nothing was launched
    with pytest.raises(T.TagrecError):                        # a shared buffer needs the L2 rows to be the score rows
        other = torch.zeros_like(Ib)
        dU, dI = _nan_like(Ub), _nan_like(Ib)
        rowops.wbce_bwd(Ub, Ib, Ub.clone(), other, coef, None, dU, dI, dU, dI, K, M)
