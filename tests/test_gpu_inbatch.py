"""GPU: the in-batch softmax kernels (csrc/inbatch.hip) through rowops.inbatch_fwd / inbatch_bwd and help.in_batch_loss,
against the fp64 restatement of tests/inbatch_torch.py.

Tolerance: this repository's rule: |got - ref64| <= c * 2^-24 * mag + extra, `c` counted off the kernels as
built and written beside each check; `extra` carries what enters through the softmax slope and is itself such a count.
With u = 2^-24, the counts, once:

  score s_bj      a D-term MFMA dot: D on smag = sum |terms|.  z = fmaf(s, 1 / tau, -bias): the float 1 / tau and the fma, so
                  dz = (D + 2) u (smag / tau + |bias|).
  row sum S       lane q of a row sees the live columns j with (j % 16) / 4 == q in ascending order, n_q of them.  A term
                  enters by expf (4 ulp = 8) and an add; every later column adds once (n_q); every move of the running maximum
                  rescales by an expf and a product and adds: 9 per move.  Moves are counted on the fp64 logits, a column
                  within 2 max dz of the running maximum counting as one (the kernel may see it above).  The two merges of the
                  four lanes: 2 x (8 + 1 + 1) = 20.  c_S = max_q (8 + n_q + 9 moves_q) + 20, relative to S.  The roundings of
                  the exponents z - max add up to u |a_j| per term (the maximum only rises): sum_j p_j |a_j| u.
  lse_b           max + logf(S): logf's 8 and the add, 9 on |max| + |log S|; extra: u (c_S + sum p |a|) + sum_j p_j dz_bj.
  loss            (lse - z_bb): 1; the wave's shuffle tree 6, the four waves 2, the reduce kernel 1 + 8, the float 1 / B and
                  its product 2: 9 + 1 + 19 = 29 on mean(|max| + |log S| + |z_bb|); extra: lse's, and dz_bb.
  L2              ceil(Dreg / 64) fmas per lane, the tree 6, 32 row adds, the waves 2, the reduce 9, 1 / B 2: ceil(Dreg / 64) + 51
  C_bj            scale = (g0 (1 / tau)) (1 / B): 4; p = expf(z - lse) from the kernel's own lse: u |z - lse| and 8 on p, and dz
                  through the slope; (p - delta): 1; the product with scale: 1.  6 on |C|; extra |scale| p (u (8 + |z - lse|) + dz)
  dUb, dIb        a B-term MFMA chain on C's count: B + 6 on sum |C| |row|, plus C's extra through the same sum
  L2 rows         (g1 (1 / B)) x: 3; into the SAME buffer it joins by a product and an add: + 2
Each test prints its worst err / bound (`-s`)."""
import ctypes

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import tagrec_amd as T
from tagrec_amd import _lib, help as H, rowops

import inbatch_torch as IB
from spmm_ref import U32, Chk, f64 as _f64, randn as _randn, same_bits as _same_bits
from test_gpu_rank_loss import _bwd_ref as _rank_bwd_ref, _fwd_ref as _rank_fwd_ref

DEV = torch.device("cuda:0")
# 1, 2; both sides of the MFMA's 16 and of the block's row tile = column tile (64); 130: three blocks, three column tiles, a
# ragged last tile in both directions
BS = (1, 2, 15, 16, 17, 63, 64, 65, 130)
DS = (8, 16, 64, 100, 176, 256)     # every accumulator count the backward is built for (1, 1, 4, 8, 12, 16 tiles), two ragged
TAUS = (1.0, 0.05)


def _t64(a):
    return torch.from_numpy(np.asarray(a, dtype=np.float64))


def _cpu(t):
    return None if t is None else t.detach().cpu()


def _fwd_ref(Ub, Ib, Urb, Irb, tau, uid=None, iid=None, bias=None):
    """fp64 lse / loss / reg of compact operands, each with (ref, mag, c, extra) of the rule above, and what the backward's
    reference needs."""
    B, D = Ub.shape
    tau = float(np.float32(tau))                                              # the float the ABI takes
    u, it = _f64(Ub), _f64(Ib)
    b = np.zeros(B) if bias is None else _f64(bias)
    z = (u @ it.T) / tau - b[None, :]
    dz = (D + 2) * U32 * ((np.abs(u) @ np.abs(it).T) / tau + np.abs(b)[None, :])
    live = np.ones((B, B), bool) if uid is None else ~IB.mask(_cpu(uid), _cpu(iid)).numpy()
    zl = np.where(live, z, -np.inf)
    m = zl.max(1)
    a = np.where(live, z - m[:, None], 0.0)
    e = np.where(live, np.exp(a), 0.0)
    S = e.sum(1)
    p = e / S[:, None]
    lse = m + np.log(S)
    want = IB.lse64(_t64(z), None if uid is None else IB.mask(_cpu(uid), _cpu(iid))).numpy()
    assert np.abs(lse - want).max() <= 1e-12 * max(1.0, np.abs(want).max())  # the restatement (torch.logsumexp) says the same
    # the lanes' sums: columns of lane q in ascending order, potential moves of its running maximum
    tol = 2 * np.where(live, dz, 0.0).max(1)
    cS = np.zeros(B)
    for q in range(4):
        cols = np.nonzero((np.arange(B) % 16) // 4 == q)[0]
        if cols.size == 0:
            continue
        zq, lq = zl[:, cols], live[:, cols]
        prev = np.concatenate([np.full((B, 1), -np.inf), np.maximum.accumulate(zq, axis=1)[:, :-1]], axis=1)
        moves = (lq & (zq >= prev - tol[:, None])).sum(1)
        cS = np.maximum(cS, 8 + lq.sum(1) + 9 * moves)
    cS = cS + 20
    pa, pdz = (p * np.abs(a)).sum(1), (p * dz).sum(1)
    lextra = U32 * (cS + pa) + pdz
    lmag = np.abs(m) + np.abs(np.log(S))
    zd, dzd = np.diagonal(z), np.diagonal(dz)
    out = {"lse": (lse, lmag, 9, lextra), "loss": ((lse - zd).mean(), (lmag + np.abs(zd)).mean(), 29, (lextra + dzd).mean()),
           "z": z, "dz": dz, "live": live, "dlse": 9 * U32 * lmag + lextra}
    if Urb is not None:
        ss = 0.5 * ((_f64(Urb) ** 2).sum() + (_f64(Irb) ** 2).sum()) / B
        out["reg"] = (ss, ss, -(-Urb.shape[1] // 64) + 51, 0.0)
    else:
        out["reg"] = None
    return out


def _check_fwd(chk, tag, ref, res, lse):
    chk.close(tag + "lse", lse, *ref["lse"])
    chk.close(tag + "loss", res[0], *ref["loss"])
    if ref["reg"] is None:
        assert float(res[1]) == 0.0
    else:
        chk.close(tag + "reg", res[1], *ref["reg"])


def _bwd_ref(Ub, Ib, Urb, Irb, tau, fwd, lse, g, shared=False, dlse=None):
    """fp64 gradients from the kernel's own inputs (its lse included) -> {name: [ref, mag, c, extra]}.  dlse: the bound of
    lse itself, for a comparison that does not start from the kernel's lse."""
    B, D = Ub.shape
    tau = float(np.float32(tau))
    g0, g1 = (1.0, 1.0) if g is None else (float(np.float32(g[0])), float(np.float32(g[1])))
    u, it = _f64(Ub), _f64(Ib)
    z, dz, live = fwd["z"], fwd["dz"], fwd["live"]
    a = np.where(live, z - _f64(lse)[:, None], 0.0)
    p = np.where(live, np.exp(a), 0.0)
    scale = g0 / (tau * B)
    C = scale * (p - np.eye(B))
    E = abs(scale) * p * (U32 * (8 + np.abs(a)) + dz + (0.0 if dlse is None else dlse[:, None]))
    out = {"dU": [C @ it, np.abs(C) @ np.abs(it), B + 6, E @ np.abs(it)],
           "dI": [C.T @ u, np.abs(C).T @ np.abs(u), B + 6, E.T @ np.abs(u)]}
    if Urb is not None:
        ur, ir = g1 / B * _f64(Urb), g1 / B * _f64(Irb)
        if shared:
            for k, r in (("dU", ur), ("dI", ir)):
                out[k] = [out[k][0] + r, out[k][1] + np.abs(r), out[k][2] + 2, out[k][3]]
        else:
            out["dUr"], out["dIr"] = [ur, np.abs(ur), 3, 0.0], [ir, np.abs(ir), 3, 0.0]
    return out


def _slot(n, d, seed, pad=0, scale=0.35):
    """[n, d] on the GPU; pad > 0: a slot of a NaN-padded wider buffer (row stride d + pad)."""
    buf = torch.full((n, d + pad), float("nan"))
    buf[:, :d] = _randn(n, d, seed=seed, scale=scale)
    return buf.to(DEV)[:, :d]


def _nan_like(t, pad=0):
    return torch.full((t.shape[0], t.shape[1] + pad), float("nan"), device=DEV)[:, :t.shape[1]]


def _ids(B, seed, users=True, items=True):
    """uid, iid [B] with repeated users and / or repeated items (both: some pairs repeat both at once)."""
    g = torch.Generator().manual_seed(seed)
    uid = torch.randint(0, max(1, B // 2), (B,), generator=g) if users else torch.arange(B)
    iid = torch.randint(0, max(1, (2 * B) // 3), (B,), generator=g) if items else torch.arange(B)
    return uid.to(DEV), iid.to(DEV)


def _run(chk, tag, Ub, Ib, Urb, Irb, tau, uid=None, iid=None, bias=None, g=None, pad=0):
    """Forward, backward and the repeat of both on one operand set; Urb is Ub: one gradient buffer for both parts."""
    shared = Urb is Ub
    res, lse = rowops.inbatch_fwd(Ub, Ib, Urb, Irb, tau, uid, iid, bias)
    fwd = _fwd_ref(Ub, Ib, Urb, Irb, tau, uid, iid, bias)
    _check_fwd(chk, tag, fwd, res, lse)
    gg = None if g is None else torch.tensor(g, dtype=torch.float32, device=DEV)
    outs = []
    for _ in range(2):       # every output pre-filled with NaN must be fully overwritten (chk.close refuses a non-finite value)
        dU, dI = _nan_like(Ub, pad), _nan_like(Ib, pad)
        dUr, dIr = (dU, dI) if shared else ((_nan_like(Urb, pad), _nan_like(Irb, pad)) if Urb is not None else (None, None))
        rowops.inbatch_bwd(Ub, Ib, Urb, Irb, tau, lse, gg, dU, dI, dUr, dIr, uid, iid, bias)
        outs.append((dU, dI) if (shared or Urb is None) else (dU, dI, dUr, dIr))
    ref = _bwd_ref(Ub, Ib, Urb, Irb, tau, fwd, lse, g, shared)
    for k, got in zip(("dU", "dI", "dUr", "dIr"), outs[0]):
        chk.close(tag + k, got, *ref[k])
    # two launches: the same bits (no atomics, nothing read from the outputs), forward and backward
    res2, lse2 = rowops.inbatch_fwd(Ub, Ib, Urb, Irb, tau, uid, iid, bias)
    assert _same_bits(res, res2) and _same_bits(lse, lse2)
    assert all(_same_bits(x, y) for x, y in zip(*outs))
    return res, lse, outs[0], fwd


@pytest.mark.parametrize("D", DS)
@pytest.mark.parametrize("B", BS)
def test_inbatch_kernels_against_fp64(B, D):
    """Every (B, D) at both temperatures: (a) everything on -- distinct L2 rows of another width, upstream g != (1, 1), a
    column bias, repeated users and items; (b) everything off -- L2 on the score rows into one buffer, no g, no bias, no ids."""
    chk = Chk(f"inbatch B={B} D={D}", tag="inbatch")
    for i, tau in enumerate(TAUS):
        sd = 100 * B + D + 7 * i
        Ub, Ib = _slot(B, D, sd), _slot(B, D, sd + 1)
        Urb, Irb = _slot(B, D + 4, sd + 2), _slot(B, D + 4, sd + 3)
        uid, iid = _ids(B, sd)
        bias = _randn(B, seed=sd + 4, scale=1.5).to(DEV)
        _run(chk, f"a/{tau} ", Ub, Ib, Urb, Irb, tau, uid, iid, bias, g=(0.37, -2.0))
        _run(chk, f"b/{tau} ", Ub, Ib, Ub, Ib, tau)
    chk.done()


@pytest.mark.parametrize("pad", [4, 3])
def test_inbatch_strided_rows_nan_padding(pad):
    """ld > D: operands and gradient buffers are slots of wider buffers whose padding columns hold NaN; nothing reads or writes
    them.  pad = 4 keeps the rows 16-byte aligned (float4 staging), pad = 3 does not (scalar staging)."""
    chk = Chk(f"inbatch strided pad={pad}", tag="inbatch")
    B, D, tau = 70, 100, 0.05
    Ub, Ib = _slot(B, D, 11, pad), _slot(B, D, 12, pad)
    Urb, Irb = _slot(B, D, 13, pad), _slot(B, D, 14, pad)
    uid, iid = _ids(B, 15)
    _, _, grads, _ = _run(chk, "distinct ", Ub, Ib, Urb, Irb, tau, uid, iid, None, g=(0.37, -2.0), pad=pad)
    _, _, grads2, _ = _run(chk, "shared ", Ub, Ib, Ub, Ib, tau, uid, iid, None, g=(0.37, -2.0), pad=pad)
    for t in (Ub, Ib, Urb, Irb) + tuple(grads) + tuple(grads2):
        assert t.stride(0) == D + pad
        whole = torch.as_strided(t, (B, D + pad), (D + pad, 1))
        assert torch.isnan(whole[:, D:]).all() and torch.isfinite(whole[:, :D]).all()
    chk.done()


def _masked_ids(kind, B):
    ar = torch.arange(B)
    if kind == "items":
        return ar.clone(), ar // 3                       # every item three times, users distinct
    if kind == "users":
        return ar // 4, ar.clone()
    if kind == "both":
        return ar // 4, (ar + 1) // 3
    if kind == "one_item":
        return ar.clone(), torch.zeros(B, dtype=torch.int64)
    assert kind == "one_row"                             # row 5 shares its user with the rows below B / 2, its item with the rest
    uid, iid = ar.clone() + B, ar.clone() + B
    uid[:B // 2] = 0
    iid[B // 2:] = 0
    uid[5], iid[5] = 0, 0
    return uid, iid


@pytest.mark.parametrize("kind", ["items", "users", "both", "one_item", "one_row"])
def test_inbatch_masks(kind):
    """Repeated items, repeated users, both; one batch where every pair names one item (every off-diagonal entry masked: loss
    exactly 0, gradients exactly 0, nothing non-finite); one fully masked row among normal rows."""
    chk = Chk(f"inbatch mask {kind}", tag="inbatch")
    B, D, tau = 70, 16, 0.5          # logits of spread ~2: the softmax is not saturated, so a wrongly kept column shows
    uid, iid = _masked_ids(kind, B)
    M = IB.mask(uid, iid)
    assert M.any() and not torch.diagonal(M).any()
    Ub, Ib = _slot(B, D, 31, scale=0.5), _slot(B, D, 32, scale=0.5)
    bias = _randn(B, seed=33, scale=1.5).to(DEV)
    res, lse, (dU, dI), fwd = _run(chk, "", Ub, Ib, None, None, tau, uid.to(DEV), iid.to(DEV), bias)
    if kind == "one_item":
        assert M.sum() == B * (B - 1)
        assert float(res[0]) == 0.0 and float(dU.abs().max()) == 0.0 and float(dI.abs().max()) == 0.0
        assert torch.isfinite(lse).all()
    if kind == "one_row":
        assert M[5].sum() == B - 1 and not (M.sum(1) == B - 1)[torch.arange(B) != 5].any()
        assert float(dU[5].abs().max()) == 0.0           # lse_5 = z_55: exp(0) - 1
        assert abs(float(lse[5]) - fwd["z"][5, 5]) <= fwd["dz"][5, 5] + U32 * abs(fwd["z"][5, 5])
        assert float(dU.abs().sum()) > 0.0 and float(res[0]) > 0.0
    chk.done()


@pytest.mark.parametrize("tau", TAUS)
def test_inbatch_large_logits_stay_finite(tau):
    """Scores scaled so that |z| reaches 200: the running maximum is subtracted before every expf, so nothing overflows and
    nothing is NaN; the result stays within the bound."""
    chk = Chk(f"inbatch large tau={tau}", tag="inbatch")
    B, D = 70, 16
    Ub, Ib = _slot(B, D, 41, scale=1.0), _slot(B, D, 42, scale=1.0)
    s = (Ub.double() @ Ib.double().t()).abs().max().item()
    Ub = (Ub * (200.0 * tau / s)).contiguous()
    uid, iid = _ids(B, 43)
    res, lse, grads, fwd = _run(chk, "", Ub, Ib, Ub, Ib, tau, uid, iid)
    assert 190.0 <= np.abs(fwd["z"]).max() <= 210.0
    assert torch.isfinite(res).all() and torch.isfinite(lse).all() and all(torch.isfinite(t).all() for t in grads)
    assert float(res[0]) > 1.0
    chk.done()


@pytest.mark.parametrize("B,D,tau", [(2, 8, 1.0), (17, 64, 0.05), (64, 100, 1.0), (64, 256, 0.05)])
def test_inbatch_agrees_with_the_rank_kernels(B, D, tau):
    """Distinct ids, no bias: in-batch softmax is sampled softmax with K = B - 1 over the other positives.  The [B, 1 + K]
    operands of rowops.rank_fwd / rank_bwd are built by explicit gather (item j of tuple b = row (b + j) % B).  Both paths obey
    the rule against fp64, so their difference is bounded by the sum of the two bounds: this file's counts (lse's own bound
    carried into C) and those of tests/test_gpu_rank_loss.py (its coef bound carried into the gradients)."""
    chk = Chk(f"inbatch vs rank B={B} D={D} tau={tau}", tag="inbatch")
    K = B - 1
    Ub, Ib = _slot(B, D, 51 + B), _slot(B, D, 52 + B)
    ar = torch.arange(B, device=DEV)
    slots = ((ar[None, :] + torch.arange(1 + K, device=DEV)[:, None]) % B).reshape(-1)      # slot j B + b -> row (b + j) % B
    Ibr = Ib.index_select(0, slots)
    res, lse = rowops.inbatch_fwd(Ub, Ib, None, None, tau, ar, ar)
    res_r, coef = rowops.rank_fwd(Ub, Ibr, None, None, _lib.LOSS_SOFTMAX, tau)
    fwd, fwd_r = _fwd_ref(Ub, Ib, None, None, tau, ar, ar), _rank_fwd_ref(Ub, Ibr, None, None, K, "softmax", tau)
    assert abs(fwd["loss"][0] - fwd_r["loss"][0]) <= 1e-12 * max(1.0, abs(fwd["loss"][0]))

    def bound(r):
        return r[2] * U32 * r[1] + r[3]
    chk.close("loss", res[0], _f64(res_r[0]), 1.0, 0.0, bound(fwd["loss"]) + bound(fwd_r["loss"]))
    g = (0.37, -2.0)
    gg = torch.tensor(g, device=DEV)
    dU, dI, dUr, dIr = _nan_like(Ub), _nan_like(Ib), _nan_like(Ub), _nan_like(Ibr)
    rowops.inbatch_bwd(Ub, Ib, None, None, tau, lse, gg, dU, dI, None, None, ar, ar)
    rowops.rank_bwd(Ub, Ibr, None, None, coef, gg, dUr, dIr, None, None)
    mine = _bwd_ref(Ub, Ib, None, None, tau, fwd, lse, g, dlse=fwd["dlse"])
    rank = _rank_bwd_ref(Ub, Ibr, None, None, K, coef, g)
    # the rank path against the truth: its backward count on its own coef, plus coef's bound through (g0 / B) |row|
    cref, cmag, cc, cextra = fwd_r["coef"]
    dcoef = abs(g[0]) / B * (cc * U32 * cmag + cextra)                                     # [B, 1 + K]
    it = np.abs(_f64(Ibr)).reshape(1 + K, B, D)
    bU = rank["dU"][2] * U32 * rank["dU"][1] + (dcoef.T[:, :, None] * it).sum(0)
    bI = rank["dI"][2] * U32 * rank["dI"][1] + (dcoef.T[:, :, None] * np.abs(_f64(Ub))[None]).reshape(-1, D)
    fold = np.zeros((B, D)), np.zeros((B, D))
    np.add.at(fold[0], slots.cpu().numpy(), _f64(dIr))                                     # the fold itself in fp64
    np.add.at(fold[1], slots.cpu().numpy(), bI)
    chk.close("dU", dU, _f64(dUr), 1.0, 0.0, bound(mine["dU"]) + bU)
    chk.close("dI", dI, fold[0], 1.0, 0.0, bound(mine["dI"]) + fold[1])
    chk.done()


def test_inbatch_fwd_overwrites_a_poisoned_lse():
    """The C entry itself, with lse, partials and the result pre-filled with NaN: every element is overwritten."""
    B, D = 130, 64
    Ub, Ib = _slot(B, D, 61), _slot(B, D, 62)
    lse = torch.full((B,), float("nan"), device=DEV)
    partials = torch.full((2 * ((B + rowops.INBATCH_TILE - 1) // rowops.INBATCH_TILE),), float("nan"), device=DEV)
    res = torch.full((2,), float("nan"), device=DEV)
    p = _lib.ptr
    _lib.check(_lib.load().tagrec_inbatch_fwd_f32(p(Ub), p(Ib), D, D, p(None), p(None), p(None), p(Ub), p(Ib), D, D, B,
                                                  ctypes.c_float(0.5), p(lse), p(partials), p(res), _lib.stream_ptr()))
    assert torch.isfinite(lse).all() and torch.isfinite(partials).all() and torch.isfinite(res).all()
    res2, lse2 = rowops.inbatch_fwd(Ub, Ib, Ub, Ib, 0.5)
    assert _same_bits(res, res2) and _same_bits(lse, lse2)


def test_inbatch_refuses_bad_arguments():
    def ops(B, D):
        return torch.zeros(B, D, device=DEV), torch.zeros(B, D, device=DEV)
    ar = torch.arange(4, device=DEV)
    for D in (6, 260, 4):                                            # not a multiple of 4, past 256, below 8
        with pytest.raises(T.TagrecError, match="D must be"):
            rowops.inbatch_fwd(*ops(4, D), None, None, 1.0)
    Ub, Ib = ops(4, 8)
    with pytest.raises(T.TagrecError):
        rowops.inbatch_fwd(Ub, Ib, None, None, 1.0, uid=ar)          # one of uid / iid without the other
    with pytest.raises(T.TagrecError):
        rowops.inbatch_fwd(Ub, Ib, None, None, 1.0, iid=ar)
    with pytest.raises(T.TagrecError):
        rowops.inbatch_fwd(*ops(0, 8), None, None, 1.0)              # B = 0
    with pytest.raises(T.TagrecError):
        rowops.inbatch_fwd(Ub, Ib[:3], None, None, 1.0)
    with pytest.raises(T.TagrecError):
        rowops.inbatch_fwd(Ub, Ib, Ub, None, 1.0)
    with pytest.raises(T.TagrecError):
        rowops.inbatch_fwd(Ub, Ib, None, None, 1.0, ar[:3], ar[:3])
    with pytest.raises(T.TagrecError):
        rowops.inbatch_fwd(Ub, Ib, None, None, 1.0, ar.int(), ar.int())
    for tau in (0.0, -1.0, float("inf"), float("nan")):
        with pytest.raises(T.TagrecError):
            rowops.inbatch_fwd(Ub, Ib, None, None, tau)
    res, lse = rowops.inbatch_fwd(Ub, Ib, None, None, 1.0)
    dU, dI = torch.empty_like(Ub), torch.empty_like(Ib)
    with pytest.raises(T.TagrecError):
        rowops.inbatch_bwd(Ub, Ib, None, None, 1.0, lse[:3], None, dU, dI, None, None)
    with pytest.raises(T.TagrecError):
        rowops.inbatch_bwd(Ub, Ib, None, None, 1.0, lse, None, dU, None, None, None)
    with pytest.raises(T.TagrecError):                               # a shared buffer needs Ureg = Ub
        rowops.inbatch_bwd(Ub, Ib, Ub.clone(), Ib.clone(), 1.0, lse, None, dU, dI, dU, dI)
    with pytest.raises(T.TagrecError):
        rowops.inbatch_bwd(*ops(4, 6), None, None, 1.0, lse, None, *ops(4, 6), None, None)


# ====================================================================================================== help.in_batch_loss
def _tables_and_pairs(nu=50, ni=60, D=64, B=48, seed=21):
    """Tables and a [B, 2] batch that names user 7 twelve times and item 3 five times, once with user 7."""
    g = torch.Generator().manual_seed(seed)
    W = _randn(nu + ni, D, seed=seed, scale=0.35).to(DEV)
    E = _randn(nu + ni, D, seed=seed + 1, scale=0.35).to(DEV)
    pairs = torch.cat([torch.randint(0, nu, (B, 1), generator=g), torch.randint(0, ni, (B, 1), generator=g)], 1)
    pairs[:12, 0] = 7
    pairs[10:15, 1] = 3
    return W, E, pairs


def _scatter64(n_rows, idx, terms):
    out = np.zeros((n_rows, terms.shape[1]))
    np.add.at(out, idx, terms)
    return out


@pytest.mark.parametrize("same", [False, True])
@pytest.mark.parametrize("logq", [False, True])
@pytest.mark.parametrize("planned", [False, True])
def test_in_batch_loss_on_tables(same, logq, planned):
    """help.in_batch_loss: loss parts against the restatement on the tables; gradients against the fp64 scatter of the compact
    kernel's terms (its own lse), c = the compact count + the row's multiplicity (one addition of the fold per slot that names
    the row).  same: the L2 tables are the score tables (one buffer).  planned: the fold runs in a fixed order, the same bits
    on every run."""
    chk = Chk(f"in_batch_loss same={same} logq={logq} planned={planned}", tag="inbatch")
    nu, ni, B, tau = 50, 60, 48, 0.5
    W, E, pairs = _tables_and_pairs(nu, ni, B=B)
    pg = pairs.to(DEV)
    q = (_randn(ni, seed=5, scale=1.0) - 3.0).to(DEV) if logq else None
    Eb = W if same else E
    runs = []
    for _ in range(2 if planned else 1):
        U, I = W[:nu].clone().requires_grad_(), W[nu:].clone().requires_grad_()
        Ur, Ir = (U, I) if same else (E[:nu].clone().requires_grad_(), E[nu:].clone().requires_grad_())
        plans = H.in_batch_plans(pg, nu, ni, W.shape[1]) if planned else None
        loss, reg = H.in_batch_loss(U, I, Ur, Ir, pg, tau, q, plans)
        g = [0.37, -2.0]
        (g[0] * loss + g[1] * reg).backward()
        runs.append([loss.detach(), reg.detach(), U.grad, I.grad] + ([] if same else [Ur.grad, Ir.grad]))
    if planned:
        assert all(_same_bits(a, b) for a, b in zip(*runs))
    want = IB.in_batch_tables64(W[:nu].cpu(), W[nu:].cpu(), Eb[:nu].cpu(), Eb[nu:].cpu(), pairs, float(np.float32(tau)), _cpu(q))
    ur, ir = pg[:, 0].contiguous(), pg[:, 1].contiguous()
    Ub, Ib = W[:nu].index_select(0, ur), W[nu:].index_select(0, ir)
    Urb, Irb = Eb[:nu].index_select(0, ur), Eb[nu:].index_select(0, ir)
    bias = None if q is None else q.index_select(0, ir)
    fwd = _fwd_ref(Ub, Ib, Urb, Irb, tau, ur, ir, bias)
    assert abs(float(want[0]) - fwd["loss"][0]) <= 1e-12 and abs(float(want[1]) - fwd["reg"][0]) <= 1e-12
    chk.close("loss", runs[0][0], *fwd["loss"])
    chk.close("reg", runs[0][1], *fwd["reg"])
    _, lse = rowops.inbatch_fwd(Ub, Ib, Urb, Irb, tau, ur, ir, bias)
    b = _bwd_ref(Ub, Ib, Urb, Irb, tau, fwd, lse, g, shared=same)
    un, inn = pairs[:, 0].numpy(), pairs[:, 1].numpy()
    checks = [("dU", runs[0][2], nu, un), ("dI", runs[0][3], ni, inn)] + ([] if same else [("dUr", runs[0][4], nu, un), ("dIr", runs[0][5], ni, inn)])
    for k, got, n, idx in checks:
        mult = _scatter64(n, idx, np.ones((B, 1)))
        chk.close(k, got, _scatter64(n, idx, b[k][0]), _scatter64(n, idx, b[k][1]), b[k][2] + mult,
                  _scatter64(n, idx, np.broadcast_to(b[k][3], b[k][0].shape)))
    assert float(_scatter64(nu, un, np.ones((B, 1))).max()) >= 12.0       # user 7's multiplicity
    chk.done()


def test_in_batch_loss_refuses_a_wrong_batch():
    W, E, pairs = _tables_and_pairs()
    with pytest.raises(T.TagrecError):
        H.in_batch_loss(W[:50], W[50:], None, None, torch.cat([pairs, pairs[:, :1]], 1).to(DEV))
    with pytest.raises(T.TagrecError):
        H.in_batch_loss(W[:50].cpu(), W[50:].cpu(), None, None, pairs)
