"""GPU: the catalogue softmax kernels (csrc/catsoftmax.hip) through rowops.catsoftmax_fwd / catsoftmax_bwd and
help.catalogue_softmax_loss, against the fp64 restatement of tests/catsoftmax_torch.py.

Tolerance: this repository's rule: |got - ref64| <= c * 2^-24 * mag + extra, `c` counted off the kernels as
built and written beside each check; `extra` carries what enters through the softmax slope and is itself such a count.
With u = 2^-24, S the number of column ranges (n_split) and R = min(N, 64 ceil(ceil(N / 64) / S)) the columns of a range, the
counts, once:

  score s_bn      a D-term MFMA dot: D on smag = sum |terms|.  z = s * (1 / tau): the float 1 / tau and the product, so
                  dz = (D + 2) u smag / tau.  zt is such a z: bound dz at (b, target_b).
  lane sum        inside one range, lane q of a row sees the columns n with (n % 16) / 4 == q in ascending order, n_q of them.
                  A term enters by expf (4 ulp = 8) and an add; every later column adds once (n_q); every move of the running
                  maximum rescales by an expf and a product and adds: 9 per move.  Moves are counted on the fp64 logits, a
                  column within 2 max dz of the running maximum counting as one (the kernel may see it above).
  lane merge      two merges of the four lanes, each an expf, a product and an add on either side: 2 x (8 + 1 + 1) = 20.
  range merge     cat_combine_kernel folds the S pairs in ascending order from (sentinel, 0), one rescale (expf, product) and
                  one add per range, an empty range included: 10 S.
                  c_S = max over (range, q) of (8 + n_q + 9 moves_q) + 20 + 10 S, relative to S_b (a sum of positive terms: the
                  worst part's relative error bounds the whole's).  The roundings of the exponents z - max, m_old - m_new add
                  up to u |a_n| per term (a_n = z_n - max_b; the maximum only rises, the chain telescopes): sum_n p_n |a_n| u.
  lse_b           max + logf(S): logf's 8 and the add, 9 on |max| + |log S|; extra: u (c_S + sum p |a|) + sum_n p_n dz_bn.
  loss            (lse - zt): 1; the combine block's tree over 256 rows 8; the reduce kernel 1 + 8 (at most 256 blocks: one
                  partial per thread); the float 1 / B and its product 2: 9 + 1 + 19 = 29 on mean(|max| + |log S| + |zt|);
                  extra: lse's, and dz at the target.
  L2              ceil(Dreg / 64) fmas per lane, the tree 6, a wavefront's 2 x 64 row adds 128, the four wavefronts 2, the
                  reduce 9, 1 / B 2: ceil(Dreg / 64) + 147
  C_bn            scale = (g0 (1 / tau)) (1 / B): 4; p = expf(z - lse) from the kernel's own lse: u |z - lse| and 8 on p, and dz
                  through the slope; (p - delta): 1; the product with scale: 1.  6 on |C|; extra |scale| p (u (8 + |z - lse|) + dz)
  dT              the column tile walks all B rows, one MFMA chain: B + 6 on sum_b |C| |Q row|, plus C's extra through that sum
  dQ              one MFMA chain over the R columns of a range, then the S partial rows added in ascending order:
                  R + 6 + (S - 1) on sum_n |C| |T row|, plus C's extra through that sum
  L2 rows         (g1 (1 / B)) x: 3
  folds           help.catalogue_softmax_loss adds the compact rows onto the tables: + the row's multiplicity
Each test prints its worst err / bound (`-s`)."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import tagrec_amd as T
from tagrec_amd import _lib, help as H, rowops

import catsoftmax_torch as CS
from spmm_ref import U32, Chk, f64 as _f64, randn as _randn, same_bits as _same_bits
from test_gpu_inbatch import _bwd_ref as _ib_bwd_ref, _fwd_ref as _ib_fwd_ref
from test_gpu_rank_loss import _bwd_ref as _rank_bwd_ref, _fwd_ref as _rank_fwd_ref

DEV = torch.device("cuda:0")
BS = (1, 2, 17, 64, 65, 130)            # 1, 2; both sides of the row tile (64); 130: three row tiles, the last ragged
NS = (1, 5, 63, 64, 65, 130, 1000)      # both sides of the column tile (64); 130: three tiles; 1000: 16 tiles, default S = 4
DS = (8, 64, 100, 256)                  # 1, 4, 8, 16 accumulator tiles; 100 is ragged
TAUS = (1.0, 0.05)
SPLITS = (1, 2, 3, 7, 64)


def _cpu(t):
    return None if t is None else t.detach().cpu()


def _slot(n, d, seed, pad=0, scale=0.35):
    """[n, d] on the GPU; pad > 0: a slot of a NaN-padded wider buffer (row stride d + pad)."""
    buf = torch.full((n, d + pad), float("nan"))
    buf[:, :d] = _randn(n, d, seed=seed, scale=scale)
    return buf.to(DEV)[:, :d]


def _nan(n, d, pad=0):
    return torch.full((n, d + pad), float("nan"), device=DEV)[:, :d]


def _targets(B, N, seed):
    """target [B]: 0, N - 1 (in the ragged last tile), a repeated one at the start of the last tile, the rest random."""
    t = torch.randint(0, N, (B,), generator=torch.Generator().manual_seed(seed))
    t[0] = 0
    t[-1] = N - 1
    if B >= 4:
        t[1] = t[2] = 64 * ((N - 1) // 64)
    return t


def _qrows(B, nq, seed):
    """qrow [B] into a table of nq > B rows: a permutation with repeats."""
    q = torch.randperm(nq, generator=torch.Generator().manual_seed(seed))[:B].clone()
    if B >= 3:
        q[B // 2] = q[0]
    return q


def _splits(B, N, D, n_split):
    """(S, R): the ranges the kernels use and the columns of one range."""
    S = rowops.catsoftmax_splits(B, N, D) if n_split == 0 else n_split
    tiles = -(-N // 64)
    return S, min(N, 64 * -(-tiles // S))


def _fwd_ref(Qg, Tt, target, Qrg, Trg, tau, S, R):
    """fp64 lse / zt / loss / reg of the GATHERED rows Qg [B, D] (and the L2 rows Qrg, Trg [B, Dreg]) against T [N, D], each
    with (ref, mag, c, extra) of the rule above, and what the backward's reference needs."""
    B, D = Qg.shape
    N = Tt.shape[0]
    tau = float(np.float32(tau))                                              # the float the ABI takes
    u, t = _f64(Qg), _f64(Tt)
    tg = target.cpu().numpy()
    z = (u @ t.T) / tau
    dz = (D + 2) * U32 * ((np.abs(u) @ np.abs(t).T) / tau)
    m = z.max(1)
    a = z - m[:, None]
    e = np.exp(a)
    Ssum = e.sum(1)
    p = e / Ssum[:, None]
    lse = m + np.log(Ssum)
    zt, dzt = z[np.arange(B), tg], dz[np.arange(B), tg]
    want, _ = CS.catalogue_loss64(_cpu(Qg), _cpu(Tt), _cpu(target), None, None, tau)
    assert abs(float(want) - (lse - zt).mean()) <= 1e-12 * max(1.0, abs(float(want)))      # the restatement says the same
    tol = 2 * dz.max(1)
    cS = np.zeros(B)
    for c0 in range(0, N, R):                                                  # the non-empty ranges
        cols_r = np.arange(c0, min(N, c0 + R))
        for q in range(4):
            cols = cols_r[(cols_r % 16) // 4 == q]
            if cols.size == 0:
                continue
            zq = z[:, cols]
            prev = np.concatenate([np.full((B, 1), -np.inf), np.maximum.accumulate(zq, axis=1)[:, :-1]], axis=1)
            moves = (zq >= prev - tol[:, None]).sum(1)
            cS = np.maximum(cS, 8 + cols.size + 9 * moves)
    cS = cS + 20 + 10 * S
    pa, pdz = (p * np.abs(a)).sum(1), (p * dz).sum(1)
    lextra = U32 * (cS + pa) + pdz
    lmag = np.abs(m) + np.abs(np.log(Ssum))
    out = {"lse": (lse, lmag, 9, lextra), "zt": (zt, 0.0, 0, dzt),
           "loss": ((lse - zt).mean(), (lmag + np.abs(zt)).mean(), 29, (lextra + dzt).mean()),
           "z": z, "dz": dz, "tg": tg, "dlse": 9 * U32 * lmag + lextra}
    if Qrg is not None:
        ss = 0.5 * ((_f64(Qrg) ** 2).sum() + (_f64(Trg) ** 2).sum()) / B
        out["reg"] = (ss, ss, -(-Qrg.shape[1] // 64) + 147, 0.0)
    else:
        out["reg"] = None
    return out


def _bwd_ref(Qg, Tt, Qrg, Trg, tau, fwd, lse, g, S, R, dlse=None):
    """fp64 gradients from the kernel's own inputs (its lse included) -> {name: [ref, mag, c, extra]}.  dlse: the bound of
    lse itself, for a comparison that does not start from the kernel's lse."""
    B, D = Qg.shape
    tau = float(np.float32(tau))
    g0, g1 = (1.0, 1.0) if g is None else (float(np.float32(g[0])), float(np.float32(g[1])))
    u, t = _f64(Qg), _f64(Tt)
    z, dz = fwd["z"], fwd["dz"]
    a = z - _f64(lse)[:, None]
    p = np.exp(a)
    scale = g0 / (tau * B)
    hot = np.zeros_like(z)
    hot[np.arange(B), fwd["tg"]] = 1.0
    C = scale * (p - hot)
    E = abs(scale) * p * (U32 * (8 + np.abs(a)) + dz + (0.0 if dlse is None else dlse[:, None]))
    out = {"dQ": [C @ t, np.abs(C) @ np.abs(t), R + 6 + (S - 1), E @ np.abs(t)],
           "dT": [C.T @ u, np.abs(C).T @ np.abs(u), B + 6, E.T @ np.abs(u)]}
    if Qrg is not None:
        qr, tr = g1 / B * _f64(Qrg), g1 / B * _f64(Trg)
        out["dQr"], out["dTr"] = [qr, np.abs(qr), 3, 0.0], [tr, np.abs(tr), 3, 0.0]
    return out


def _check_fwd(chk, tag, ref, res, lse, zt):
    chk.close(tag + "lse", lse, *ref["lse"])
    chk.close(tag + "zt", zt, *ref["zt"])
    chk.close(tag + "loss", res[0], *ref["loss"])
    assert float((lse - zt).min()) >= 0.0                                     # loss_b >= 0, row by row
    if ref["reg"] is None:
        assert float(res[1]) == 0.0
    else:
        chk.close(tag + "reg", res[1], *ref["reg"])


def _run(chk, tag, Q, Tt, target, tau, qrow=None, Qreg=None, Treg=None, g=None, n_split=0, pad=0):
    """Forward, backward and the repeat of both on one operand set, every output pre-filled with NaN."""
    B, (N, D) = target.shape[0], Tt.shape
    S, R = _splits(B, N, D, n_split)
    Qg = Q if qrow is None else Q.index_select(0, qrow)
    Qrg = None if Qreg is None else (Qreg if qrow is None else Qreg.index_select(0, qrow))
    Trg = None if Treg is None else Treg.index_select(0, target)
    res, lse, zt = rowops.catsoftmax_fwd(Q, Tt, target, tau, qrow, Qreg, Treg, n_split)
    fwd = _fwd_ref(Qg, Tt, target, Qrg, Trg, tau, S, R)
    _check_fwd(chk, tag, fwd, res, lse, zt)
    gg = None if g is None else torch.tensor(g, dtype=torch.float32, device=DEV)
    outs = []
    for _ in range(2):       # NaN-filled outputs must be fully overwritten (chk.close refuses a non-finite value)
        dT, dQ = _nan(N, D, pad), _nan(B, D)
        dQr, dTr = (_nan(B, Qreg.shape[1]), _nan(B, Qreg.shape[1])) if Qreg is not None else (None, None)
        rowops.catsoftmax_bwd(Q, Tt, target, tau, lse, gg, dT, dQ, qrow, Qreg, Treg, dQr, dTr, n_split)
        outs.append((dQ, dT) if Qreg is None else (dQ, dT, dQr, dTr))
    ref = _bwd_ref(Qg, Tt, Qrg, Trg, tau, fwd, lse, g, S, R)
    for k, got in zip(("dQ", "dT", "dQr", "dTr"), outs[0]):
        chk.close(tag + k, got, *ref[k])
    # two launches: the same bits (no atomics, nothing read from the outputs), forward and backward
    res2, lse2, zt2 = rowops.catsoftmax_fwd(Q, Tt, target, tau, qrow, Qreg, Treg, n_split)
    assert _same_bits(res, res2) and _same_bits(lse, lse2) and _same_bits(zt, zt2)
    assert all(_same_bits(x, y) for x, y in zip(*outs))
    return res, lse, outs[0], fwd


@pytest.mark.parametrize("D", DS)
@pytest.mark.parametrize("B", BS)
def test_catsoftmax_kernels_against_fp64(B, D):
    """Every (B, N, D) at both temperatures, the options rotating with the case: (a) rows read through qrow (a permutation with
    repeats into a larger table), distinct L2 tables of another width, upstream g != (1, 1); (b) no qrow, no g, the L2 tables
    are the score tables; (c) no L2 term at all (loss_out[1] == 0.0 exactly)."""
    chk = Chk(f"catsoftmax B={B} D={D}", tag="catsoftmax")
    for i, N in enumerate(NS):
        for j, tau in enumerate(TAUS):
            sd = 1000 * B + 10 * N + D + j
            target = _targets(B, N, sd).to(DEV)
            Tt = _slot(N, D, sd + 1)
            kind = (i + j) % 3
            if kind == 0:
                nq = B + 5
                Q, qrow = _slot(nq, D, sd + 2), _qrows(B, nq, sd).to(DEV)
                _run(chk, f"a/N={N}/{tau} ", Q, Tt, target, tau, qrow, _slot(nq, D + 4, sd + 3), _slot(N, D + 4, sd + 4), (0.37, -2.0))
            elif kind == 1:
                Q = _slot(B, D, sd + 2)
                _run(chk, f"b/N={N}/{tau} ", Q, Tt, target, tau, None, Q, Tt)
            else:
                _run(chk, f"c/N={N}/{tau} ", _slot(B, D, sd + 2), Tt, target, tau, g=(-1.5, 0.0))
    chk.done()


@pytest.mark.parametrize("N", [130, 1000])
@pytest.mark.parametrize("n_split", SPLITS)
def test_catsoftmax_forced_splits(N, n_split):
    """Every merge shape at a small N: one range, ranges of unequal length, empty ranges, more ranges than column tiles
    (N = 130 has three).  Each stays within its bound (the counts follow S and R); `_run` repeats every launch for the bits."""
    chk = Chk(f"catsoftmax N={N} n_split={n_split}", tag="catsoftmax")
    for B, D, tau in ((17, 64, 0.05), (130, 100, 1.0)):
        sd = 7 * N + n_split + B
        nq = B + 3
        Q, qrow = _slot(nq, D, sd), _qrows(B, nq, sd).to(DEV)
        _run(chk, f"B={B} ", Q, _slot(N, D, sd + 1), _targets(B, N, sd).to(DEV), tau, qrow, Q, _slot(N, D, sd + 2), (0.37, -2.0),
             n_split=n_split)
    chk.done()


def test_catsoftmax_default_split_is_a_pure_function():
    for B, N, D in ((512, 1 << 20, 64), (2048, 1 << 20, 64), (1, 1, 8), (65536, 10, 256), (130, 1000, 100)):
        s = rowops.catsoftmax_splits(B, N, D)
        assert s >= 1 and s == rowops.catsoftmax_splits(B, N, D)
        assert s <= max(1, -(-N // 64))                                        # the default leaves no range empty
        assert rowops.catsoftmax_workspace(B, N, D) == rowops.catsoftmax_workspace(B, N, D, s) > 0
    tiles = -(-512 // 64)
    assert tiles * rowops.catsoftmax_splits(512, 1 << 20, 64) >= 2 * 256      # blocks: the 256 CUs at least twice over


@pytest.mark.parametrize("pad", [4, 3])
def test_catsoftmax_strided_rows_nan_padding(pad):
    """ld > D: operands, L2 tables and dT are slots of wider buffers whose padding columns hold NaN; nothing reads or writes
    them.  pad = 4 keeps the rows 16-byte aligned (float4 staging), pad = 3 does not (scalar staging)."""
    chk = Chk(f"catsoftmax strided pad={pad}", tag="catsoftmax")
    B, N, D, tau = 70, 130, 100, 0.05
    nq = B + 4
    Q, Tt = _slot(nq, D, 11, pad), _slot(N, D, 12, pad)
    Qr, Tr = _slot(nq, D, 13, pad), _slot(N, D, 14, pad)
    qrow, target = _qrows(B, nq, 15).to(DEV), _targets(B, N, 16).to(DEV)
    _, _, grads, _ = _run(chk, "", Q, Tt, target, tau, qrow, Qr, Tr, (0.37, -2.0), n_split=2, pad=pad)
    for t in (Q, Tt, Qr, Tr, grads[1]):
        assert t.stride(0) == D + pad
        whole = torch.as_strided(t, (t.shape[0], D + pad), (D + pad, 1))
        assert torch.isnan(whole[:, D:]).all() and torch.isfinite(whole[:, :D]).all()
    chk.done()


@pytest.mark.parametrize("tau", TAUS)
def test_catsoftmax_large_logits_stay_finite(tau):
    """Scores scaled so that |z| reaches 200: the running maximum is subtracted before every expf, so nothing overflows and
    nothing is NaN; the result stays within the bound and every row's loss is >= 0 (`_check_fwd`)."""
    chk = Chk(f"catsoftmax large tau={tau}", tag="catsoftmax")
    B, N, D = 70, 200, 16
    Q, Tt = _slot(B, D, 41, scale=1.0), _slot(N, D, 42, scale=1.0)
    s = (Q.double() @ Tt.double().t()).abs().max().item()
    Q = (Q * (200.0 * tau / s)).contiguous()
    res, lse, grads, fwd = _run(chk, "", Q, Tt, _targets(B, N, 43).to(DEV), tau, None, Q, Tt, n_split=3)
    assert 190.0 <= np.abs(fwd["z"]).max() <= 210.0
    assert torch.isfinite(res).all() and torch.isfinite(lse).all() and all(torch.isfinite(t).all() for t in grads)
    assert float(res[0]) > 1.0
    chk.done()


def _bound(r):
    return r[2] * U32 * r[1] + r[3]


@pytest.mark.parametrize("B,D,tau", [(2, 8, 1.0), (17, 64, 0.05), (65, 100, 1.0), (130, 256, 0.05)])
def test_catsoftmax_agrees_with_the_in_batch_kernels(B, D, tau):
    """T = Ib, target = arange(B), no ids and no bias: the square case is the in-batch softmax.  Both paths obey the rule
    against fp64, so their difference is bounded by the sum of the two bounds (lse's own bound carried into C on both sides)."""
    chk = Chk(f"catsoftmax vs inbatch B={B} D={D} tau={tau}", tag="catsoftmax")
    Ub, Ib = _slot(B, D, 51 + B), _slot(B, D, 52 + B)
    ar = torch.arange(B, device=DEV)
    S, R = _splits(B, B, D, 0)
    res, lse, _ = rowops.catsoftmax_fwd(Ub, Ib, ar, tau)
    res_i, lse_i = rowops.inbatch_fwd(Ub, Ib, None, None, tau)
    mine, theirs = _fwd_ref(Ub, Ib, ar, None, None, tau, S, R), _ib_fwd_ref(Ub, Ib, None, None, tau)
    assert abs(mine["loss"][0] - theirs["loss"][0]) <= 1e-12 * max(1.0, abs(mine["loss"][0]))
    chk.close("loss", res[0], _f64(res_i[0]), 1.0, 0.0, _bound(mine["loss"]) + _bound(theirs["loss"]))
    chk.close("lse", lse, _f64(lse_i), 1.0, 0.0, _bound(mine["lse"]) + _bound(theirs["lse"]))
    g = (0.37, -2.0)
    gg = torch.tensor(g, device=DEV)
    dT, dQ, dU, dI = _nan(B, D), _nan(B, D), _nan(B, D), _nan(B, D)
    rowops.catsoftmax_bwd(Ub, Ib, ar, tau, lse, gg, dT, dQ)
    rowops.inbatch_bwd(Ub, Ib, None, None, tau, lse_i, gg, dU, dI, None, None)
    bm = _bwd_ref(Ub, Ib, None, None, tau, mine, lse, g, S, R, dlse=mine["dlse"])
    bt = _ib_bwd_ref(Ub, Ib, None, None, tau, theirs, lse_i, g, dlse=theirs["dlse"])
    chk.close("dQ", dQ, _f64(dU), 1.0, 0.0, _bound(bm["dQ"]) + _bound(bt["dU"]))
    chk.close("dT", dT, _f64(dI), 1.0, 0.0, _bound(bm["dT"]) + _bound(bt["dI"]))
    chk.done()


@pytest.mark.parametrize("B,N,D,tau", [(2, 2, 8, 1.0), (17, 33, 64, 0.05), (65, 64, 100, 1.0)])
def test_catsoftmax_agrees_with_the_rank_kernels(B, N, D, tau):
    """The catalogue softmax is sampled softmax with K = N - 1 <= 63 whose negatives are every other item.  The [(1 + K) B, D]
    operand of rowops.rank_fwd / rank_bwd is built by explicit gather (item j of tuple b = row (target_b + j) % N).  The
    difference is bounded by the sum of this file's bound and that of tests/test_gpu_rank_loss.py (its coef bound carried
    into the gradients)."""
    chk = Chk(f"catsoftmax vs rank B={B} N={N} D={D} tau={tau}", tag="catsoftmax")
    K = N - 1
    Ub, Tt = _slot(B, D, 61 + B), _slot(N, D, 62 + B)
    target = _targets(B, N, 63 + B).to(DEV)
    slots = ((target[None, :] + torch.arange(1 + K, device=DEV)[:, None]) % N).reshape(-1)      # slot j B + b -> row (t_b + j) % N
    Ibr = Tt.index_select(0, slots)
    S, R = _splits(B, N, D, 0)
    res, lse, _ = rowops.catsoftmax_fwd(Ub, Tt, target, tau)
    res_r, coef = rowops.rank_fwd(Ub, Ibr, None, None, _lib.LOSS_SOFTMAX, tau)
    fwd, fwd_r = _fwd_ref(Ub, Tt, target, None, None, tau, S, R), _rank_fwd_ref(Ub, Ibr, None, None, K, "softmax", tau)
    assert abs(fwd["loss"][0] - fwd_r["loss"][0]) <= 1e-12 * max(1.0, abs(fwd["loss"][0]))
    chk.close("loss", res[0], _f64(res_r[0]), 1.0, 0.0, _bound(fwd["loss"]) + _bound(fwd_r["loss"]))
    g = (0.37, -2.0)
    gg = torch.tensor(g, device=DEV)
    dT, dQ, dUr, dIr = _nan(N, D), _nan(B, D), _nan(B, D), _nan((1 + K) * B, D)
    rowops.catsoftmax_bwd(Ub, Tt, target, tau, lse, gg, dT, dQ)
    rowops.rank_bwd(Ub, Ibr, None, None, coef, gg, dUr, dIr, None, None)
    mine = _bwd_ref(Ub, Tt, None, None, tau, fwd, lse, g, S, R, dlse=fwd["dlse"])
    rank = _rank_bwd_ref(Ub, Ibr, None, None, K, coef, g)
    cref, cmag, cc, cextra = fwd_r["coef"]
    dcoef = abs(g[0]) / B * (cc * U32 * cmag + cextra)                                     # [B, 1 + K]
    it = np.abs(_f64(Ibr)).reshape(1 + K, B, D)
    bU = rank["dU"][2] * U32 * rank["dU"][1] + (dcoef.T[:, :, None] * it).sum(0)
    bI = rank["dI"][2] * U32 * rank["dI"][1] + (dcoef.T[:, :, None] * np.abs(_f64(Ub))[None]).reshape(-1, D)
    fold = np.zeros((N, D)), np.zeros((N, D))
    np.add.at(fold[0], slots.cpu().numpy(), _f64(dIr))                                     # the fold itself in fp64
    np.add.at(fold[1], slots.cpu().numpy(), bI)
    chk.close("dQ", dQ, _f64(dUr), 1.0, 0.0, _bound(mine["dQ"]) + bU)
    chk.close("dT", dT, fold[0], 1.0, 0.0, _bound(mine["dT"]) + fold[1])
    chk.done()


def test_catsoftmax_l2_only_backward():
    """dT = dQ = None: the L2 rows alone, the bits of the full call's."""
    B, N, D = 70, 130, 64
    Q, Tt, target = _slot(B, D, 71), _slot(N, D, 72), _targets(B, N, 73).to(DEV)
    _, lse, _ = rowops.catsoftmax_fwd(Q, Tt, target, 0.5, None, Q, Tt)
    gg = torch.tensor([0.37, -2.0], device=DEV)
    full = _nan(B, D), _nan(B, D)
    rowops.catsoftmax_bwd(Q, Tt, target, 0.5, lse, gg, _nan(N, D), None, None, Q, Tt, *full)
    only = _nan(B, D), _nan(B, D)
    assert rowops.catsoftmax_bwd(Q, Tt, target, 0.5, lse, gg, None, None, None, Q, Tt, *only) is None
    assert _same_bits(full[0], only[0]) and _same_bits(full[1], only[1])


def test_catsoftmax_refuses_bad_arguments():
    def ops(B, N, D):
        return torch.zeros(B, D, device=DEV), torch.zeros(N, D, device=DEV), torch.zeros(B, dtype=torch.int64, device=DEV)
    for D in (6, 260, 4):                                            # not a multiple of 4, past 256, below 8
        with pytest.raises(T.TagrecError):
            rowops.catsoftmax_fwd(*ops(4, 9, D), 1.0)
        with pytest.raises(T.TagrecError):
            rowops.catsoftmax_splits(4, 9, D)
    with pytest.raises(T.TagrecError):
        rowops.catsoftmax_fwd(*ops(0, 9, 8), 1.0)                    # B = 0
    with pytest.raises(T.TagrecError):
        rowops.catsoftmax_fwd(*ops(4, 0, 8), 1.0)                    # N = 0
    with pytest.raises(T.TagrecError):
        rowops.catsoftmax_splits(70000, 9, 8)                        # B past 65536
    Q, Tt, target = ops(4, 9, 8)
    with pytest.raises(T.TagrecError):
        rowops.catsoftmax_fwd(Q[:3], Tt, target, 1.0)                # no qrow: one row of Q per target
    with pytest.raises(T.TagrecError):
        rowops.catsoftmax_fwd(Q, Tt, target.int(), 1.0)
    with pytest.raises(T.TagrecError):
        rowops.catsoftmax_fwd(Q, Tt, target, 1.0, qrow=target[:3])
    with pytest.raises(T.TagrecError):
        rowops.catsoftmax_fwd(Q, Tt, target, 1.0, Qreg=Q)            # one of Qreg / Treg without the other
    with pytest.raises(T.TagrecError):
        rowops.catsoftmax_fwd(Q, Tt, target, 1.0, n_split=-1)
    with pytest.raises(T.TagrecError):
        rowops.catsoftmax_fwd(Q, Tt, target, 1.0, workspace=torch.empty(8, dtype=torch.uint8, device=DEV))
    with pytest.raises(T.TagrecError):
        rowops.catsoftmax_fwd(Q.cpu(), Tt.cpu(), target.cpu(), 1.0)
    for tau in (0.0, -1.0, float("inf"), float("nan")):
        with pytest.raises(T.TagrecError):
            rowops.catsoftmax_fwd(Q, Tt, target, tau)
    _, lse, _ = rowops.catsoftmax_fwd(Q, Tt, target, 1.0)
    with pytest.raises(T.TagrecError):
        rowops.catsoftmax_bwd(Q, Tt, target, 1.0, lse[:3], None, torch.empty_like(Tt))
    with pytest.raises(T.TagrecError):
        rowops.catsoftmax_bwd(Q, Tt, target, 1.0, lse, None, torch.empty(8, 8, device=DEV))
    with pytest.raises(T.TagrecError):                               # L2 gradients without L2 operands
        rowops.catsoftmax_bwd(Q, Tt, target, 1.0, lse, None, torch.empty_like(Tt), None, None, None, None, torch.empty_like(Q),
                              torch.empty_like(Q))


# ============================================================================================ help.catalogue_softmax_loss
def _tables_and_pairs(nu=50, ni=150, D=64, B=48, seed=21):
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
@pytest.mark.parametrize("planned", [False, True])
def test_catalogue_softmax_loss_on_tables(same, planned):
    """help.catalogue_softmax_loss: loss parts against the restatement on the tables; gradients against the fp64 fold of the
    kernel's compact terms (its own lse), c = the kernel's count + the row's multiplicity (one addition of the fold per slot
    that names the row).  dI is the dense store (+ the folded L2 rows when `same`).  planned: the folds run in a fixed order,
    the same bits on every run."""
    chk = Chk(f"catalogue_softmax_loss same={same} planned={planned}", tag="catsoftmax")
    nu, ni, B, tau = 50, 150, 48, 0.5
    W, E, pairs = _tables_and_pairs(nu, ni, B=B)
    pg = pairs.to(DEV)
    Eb = W if same else E
    g = [0.37, -2.0]
    runs = []
    for _ in range(2 if planned else 1):
        U, I = W[:nu].clone().requires_grad_(), W[nu:].clone().requires_grad_()
        Ur, Ir = (U, I) if same else (E[:nu].clone().requires_grad_(), E[nu:].clone().requires_grad_())
        plans = H.in_batch_plans(pg, nu, ni, W.shape[1]) if planned else None
        loss, reg = H.catalogue_softmax_loss(U, I, Ur, Ir, pg, tau, plans)
        (g[0] * loss + g[1] * reg).backward()
        runs.append([loss.detach(), reg.detach(), U.grad, I.grad] + ([] if same else [Ur.grad, Ir.grad]))
    if planned:
        assert all(_same_bits(a, b) for a, b in zip(*runs))
    want = CS.catalogue_tables64(W[:nu].cpu(), W[nu:].cpu(), Eb[:nu].cpu(), Eb[nu:].cpu(), pairs, float(np.float32(tau)))
    ur, ir = pg[:, 0].contiguous(), pg[:, 1].contiguous()
    D = W.shape[1]
    S, R = _splits(B, ni, D, 0)
    Qg, Tt = W[:nu].index_select(0, ur), W[nu:]
    Qrg, Trg = Eb[:nu].index_select(0, ur), Eb[nu:].index_select(0, ir)
    fwd = _fwd_ref(Qg, Tt, ir, Qrg, Trg, tau, S, R)
    assert abs(float(want[0]) - fwd["loss"][0]) <= 1e-12 and abs(float(want[1]) - fwd["reg"][0]) <= 1e-12
    chk.close("loss", runs[0][0], *fwd["loss"])
    chk.close("reg", runs[0][1], *fwd["reg"])
    _, lse, _ = rowops.catsoftmax_fwd(W[:nu], Tt, ir, tau, ur)
    b = _bwd_ref(Qg, Tt, Qrg, Trg, tau, fwd, lse, g, S, R)
    un, inn = pairs[:, 0].numpy(), pairs[:, 1].numpy()
    mu, mi = _scatter64(nu, un, np.ones((B, 1))), _scatter64(ni, inn, np.ones((B, 1)))
    dU = [_scatter64(nu, un, b["dQ"][0]), _scatter64(nu, un, b["dQ"][1]), b["dQ"][2] + mu, _scatter64(nu, un, b["dQ"][3])]
    dI = [b["dT"][0], b["dT"][1], b["dT"][2] + 0.0 * mi, b["dT"][3]]
    dUr = [_scatter64(nu, un, b["dQr"][0]), _scatter64(nu, un, b["dQr"][1]), 3 + mu, 0.0]
    dIr = [_scatter64(ni, inn, b["dTr"][0]), _scatter64(ni, inn, b["dTr"][1]), 3 + mi, 0.0]
    if same:                                                           # the L2 rows are folded onto the same two gradients
        dU = [dU[0] + dUr[0], dU[1] + dUr[1], np.maximum(dU[2], dUr[2]) + mu, dU[3]]
        dI = [dI[0] + dIr[0], dI[1] + dIr[1], np.maximum(dI[2], dIr[2]) + mi, dI[3]]
    checks = [("dU", runs[0][2], dU), ("dI", runs[0][3], dI)] + ([] if same else [("dUr", runs[0][4], dUr), ("dIr", runs[0][5], dIr)])
    for k, got, r in checks:
        chk.close(k, got, *r)
    assert float(mu.max()) >= 12.0                                     # user 7's multiplicity
    assert float(runs[0][3].abs().min(1).values.max()) > 0.0 and bool((runs[0][3].abs().sum(1) > 0).all())   # dI is dense
    chk.done()


def test_catalogue_softmax_loss_refuses_a_wrong_batch():
    W, E, pairs = _tables_and_pairs()
    with pytest.raises(T.TagrecError):
        H.catalogue_softmax_loss(W[:50], W[50:], None, None, torch.cat([pairs, pairs[:, :1]], 1).to(DEV))
    with pytest.raises(T.TagrecError):
        H.catalogue_softmax_loss(W[:50].cpu(), W[50:].cpu(), None, None, pairs)
