"""GPU: the MASKED catalogue softmax kernels (csrc/catsoftmax.hip, tagrec_catsoftmax_masked_*) through rowops.catsoftmax_fwd /
catsoftmax_bwd with mask=(ptr, cols), against the fp64 restatement of tests/catsoftmax_masked_torch.py.

Tolerance: this repository's rule: |got - ref64| <= c * 2^-24 * mag + extra.  The counts are those of
tests/test_gpu_catsoftmax.py (its docstring derives each of them), taken over the LIVE columns of a row only -- an excluded
column is never pushed onto a running pair and its coefficient is a stored 0.0f, so it adds no rounding anywhere:

  score, zt       unchanged: dz = (D + 2) u smag / tau
  lane sum        n_q and the moves of the running maximum count the lane's LIVE columns; c_S = max over (range, q) of
                  (8 + n_q + 9 moves_q) + 20 + 10 S (the merges of empty or wholly excluded sides are kept in the count)
  lse_b           9 on |max| + |log S| over the live columns; extra: u (c_S + sum p |a|) + sum p dz, p = 0 where excluded
  loss            29 on mean(|max| + |log S| + |zt|); extra: lse's, and dz at the target
  C_bn            6 on |C|, extra |scale| p (u (8 + |z - lse|) + dz); an excluded C is exactly 0: c = 0, extra = 0
  dT[n]           (number of rows b for which n is live) + 6 on sum_b |C| |Q row|, plus C's extra through that sum
  dQ[b]           (the most live columns of row b inside one range) + 6 + (S - 1) on sum_n |C| |T row|, plus C's extra
  L2              unchanged
Each test prints its worst err / bound (`-s`).

The list sets (`_lists`) give the CSR rows these roles in turn (the row that batch row b reads first has role (b + seed) % 6, so
from B = 17 on every list set holds all six among the rows its batch reads -- asserted): 0 an empty list; 1 a list that
holds the targets of its batch rows (they stay live) among others; 2 a list without them that holds the columns 0, 63, 64,
N - 1 and the first and last column of every range; 3 the whole of range 0 (the batch row's target is moved to the last column
when there is a later range); 4 every column, so that the target is the row's only live column; 5 a random third of the
columns.  With qrow, batch rows 0 and B // 2 name one user (role 1) with different targets: each excludes the other's.  The
roles start at a case-dependent row, so a batch of one row takes a different one from case to case."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import tagrec_amd as T
from tagrec_amd import rowops

import catsoftmax_masked_torch as CM
from spmm_ref import U32, Chk, f64 as _f64, same_bits as _same_bits
from test_gpu_catsoftmax import _cpu, _nan, _qrows, _slot, _splits

DEV = torch.device("cuda:0")
BS = (1, 17, 65, 130)                   # 1; below, just past and twice past the row tile (64)
NS = (5, 64, 65, 130, 1000)             # below, at and past the column tile; three tiles; 16 tiles
DS = (8, 64, 100, 256)                  # 1, 4, 8, 16 accumulator tiles; 100 is ragged
TAUS = (1.0, 0.05)
SPLITS = (1, 2, 3, 7, 64)               # 64: more ranges than column tiles at both N of the forced-split test


def _ranges(N, S, R):
    return [(c0, min(N, c0 + R)) for c0 in range(0, N, R)]


def _lists(B, N, nq, qrow, target, S, R, seed):
    """(ptr, cols, roles [nq], target): the CSR over nq rows of Q with the roles of the module docstring; `target` comes back
    with the role-3 rows' targets moved past range 0 and, with qrow, rows 0 and B // 2 of one user on different targets."""
    rng = np.random.default_rng(seed)
    target = target.clone()
    rows_of = [[] for _ in range(nq)]
    qr = list(range(B)) if qrow is None else qrow.tolist()
    for b, r in enumerate(qr):
        rows_of[r].append(b)
    roles = (np.arange(nq) + seed) % 6                     # the rows no batch row reads
    for b in reversed(range(B)):                           # a row that is read: by the FIRST batch row that reads it
        roles[qr[b]] = (b + seed) % 6
    if qrow is not None and B >= 3:
        roles[qr[0]] = 1
        if N > 1:
            target[0], target[B // 2] = 0, N - 1
    if B >= 17:                                            # every list set holds every role among the rows its batch reads
        assert set(roles[qr].tolist()) == set(range(6))
    edge = sorted({c for lo, hi in _ranges(N, S, R) for c in (lo, hi - 1)} | {c for c in (0, 63, 64, N - 1) if c < N})
    lists = []
    for r in range(nq):
        tg = {int(target[b]) for b in rows_of[r]}
        some = set(rng.choice(N, size=max(1, N // 3), replace=False).tolist())
        if roles[r] == 0:
            l = set()
        elif roles[r] == 1:
            l = some | tg
        elif roles[r] == 2:
            l = (some | set(edge)) - tg
        elif roles[r] == 3:
            l = set(range(min(R, N)))
            if N > R:
                for b in rows_of[r]:
                    target[b] = N - 1
        elif roles[r] == 4:
            l = set(range(N))
        else:
            l = some
        lists.append(sorted(l))
    ptr = torch.tensor([0] + list(np.cumsum([len(l) for l in lists])), dtype=torch.int64)
    cols = torch.tensor([c for l in lists for c in l], dtype=torch.int32)
    return ptr.to(DEV), cols.to(DEV), roles, target


def _targets(B, N, seed):
    t = torch.randint(0, N, (B,), generator=torch.Generator().manual_seed(seed))
    t[0] = 0
    t[-1] = N - 1
    return t


def _fwd_ref(Qg, Tt, target, ex, Qrg, Trg, tau, S, R, want=None):
    """fp64 lse / zt / loss / reg of the gathered rows against T under the exclusion matrix ex (bool [B, N], False at the
    targets), each with (ref, mag, c, extra) of the rule above, and what the backward's reference needs."""
    B, D = Qg.shape
    N = Tt.shape[0]
    tau = float(np.float32(tau))
    u, t = _f64(Qg), _f64(Tt)
    tg = target.cpu().numpy()
    live = ~ex
    assert live[np.arange(B), tg].all()
    z = (u @ t.T) / tau
    dz = (D + 2) * U32 * ((np.abs(u) @ np.abs(t).T) / tau)
    zl = np.where(live, z, -np.inf)
    m = zl.max(1)
    a = np.where(live, z - m[:, None], 0.0)
    e = np.where(live, np.exp(a), 0.0)
    Ssum = e.sum(1)
    p = e / Ssum[:, None]
    lse = m + np.log(Ssum)
    zt, dzt = z[np.arange(B), tg], dz[np.arange(B), tg]
    if want is not None:                                                       # the restatement says the same
        assert abs(float(want) - (lse - zt).mean()) <= 1e-12 * max(1.0, abs(float(want)))
    tol = 2 * np.where(live, dz, 0.0).max(1)
    cS = np.zeros(B)
    for c0, c1 in _ranges(N, S, R):
        cols_r = np.arange(c0, c1)
        for q in range(4):
            cols = cols_r[(cols_r % 16) // 4 == q]
            if cols.size == 0:
                continue
            zq = zl[:, cols]
            prev = np.concatenate([np.full((B, 1), -np.inf), np.maximum.accumulate(zq, axis=1)[:, :-1]], axis=1)
            moves = ((zq >= prev - tol[:, None]) & live[:, cols]).sum(1)
            cS = np.maximum(cS, 8 + live[:, cols].sum(1) + 9 * moves)
    cS = cS + 20 + 10 * S
    pa, pdz = (p * np.abs(a)).sum(1), (p * dz).sum(1)
    lextra = U32 * (cS + pa) + pdz
    lmag = np.abs(m) + np.abs(np.log(Ssum))
    out = {"lse": (lse, lmag, 9, lextra), "zt": (zt, 0.0, 0, dzt),
           "loss": ((lse - zt).mean(), (lmag + np.abs(zt)).mean(), 29, (lextra + dzt).mean()),
           "z": z, "dz": dz, "tg": tg, "live": live}
    if Qrg is not None:
        ss = 0.5 * ((_f64(Qrg) ** 2).sum() + (_f64(Trg) ** 2).sum()) / B
        out["reg"] = (ss, ss, -(-Qrg.shape[1] // 64) + 147, 0.0)
    else:
        out["reg"] = None
    return out


def _bwd_ref(Qg, Tt, Qrg, Trg, tau, fwd, lse, g, S, R):
    """fp64 gradients from the kernel's own inputs (its lse included) -> {name: [ref, mag, c, extra]}."""
    B, D = Qg.shape
    N = Tt.shape[0]
    tau = float(np.float32(tau))
    g0, g1 = (1.0, 1.0) if g is None else (float(np.float32(g[0])), float(np.float32(g[1])))
    u, t = _f64(Qg), _f64(Tt)
    z, dz, live = fwd["z"], fwd["dz"], fwd["live"]
    a = np.where(live, z - _f64(lse)[:, None], 0.0)
    p = np.where(live, np.exp(a), 0.0)
    scale = g0 / (tau * B)
    hot = np.zeros_like(z)
    hot[np.arange(B), fwd["tg"]] = 1.0
    C = scale * (p - hot)
    E = abs(scale) * p * (U32 * (8 + np.abs(a)) + np.where(live, dz, 0.0))
    n_live_q = np.max([live[:, c0:c1].sum(1) for c0, c1 in _ranges(N, S, R)], axis=0)[:, None]      # [B, 1]
    n_live_t = live.sum(0)[:, None]                                                                # [N, 1]
    out = {"dQ": [C @ t, np.abs(C) @ np.abs(t), n_live_q + 6 + (S - 1), E @ np.abs(t)],
           "dT": [C.T @ u, np.abs(C).T @ np.abs(u), n_live_t + 6, E.T @ np.abs(u)], "C": C}
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


def _run(chk, tag, Q, Tt, target, tau, mask, qrow=None, Qreg=None, Treg=None, g=None, n_split=0, pad=0, roles=None):
    """Forward, backward and the repeat of both on one operand set, every output pre-filled with NaN; then the properties
    that need no reference: lse_masked <= lse_unmasked row by row, and the rows whose only live column is their target."""
    B, (N, D) = target.shape[0], Tt.shape
    S, R = _splits(B, N, D, n_split)
    Qg = Q if qrow is None else Q.index_select(0, qrow)
    Qrg = None if Qreg is None else (Qreg if qrow is None else Qreg.index_select(0, qrow))
    Trg = None if Treg is None else Treg.index_select(0, target)
    qc = None if qrow is None else qrow.cpu()
    ex = CM.dense_mask(mask[0], mask[1], target, N, qc).numpy()
    want, _ = CM.masked_catalogue_loss64(_cpu(Q), _cpu(Tt), _cpu(target), None, None, _cpu(mask[0]), _cpu(mask[1]),
                                         float(np.float32(tau)), qc)
    res, lse, zt = rowops.catsoftmax_fwd(Q, Tt, target, tau, qrow, Qreg, Treg, n_split, mask=mask)
    fwd = _fwd_ref(Qg, Tt, target, ex, Qrg, Trg, tau, S, R, want)
    _check_fwd(chk, tag, fwd, res, lse, zt)
    gg = None if g is None else torch.tensor(g, dtype=torch.float32, device=DEV)
    outs = []
    for _ in range(2):       # NaN-filled outputs must be fully overwritten (chk.close refuses a non-finite value)
        dT, dQ = _nan(N, D, pad), _nan(B, D)
        dQr, dTr = (_nan(B, Qreg.shape[1]), _nan(B, Qreg.shape[1])) if Qreg is not None else (None, None)
        rowops.catsoftmax_bwd(Q, Tt, target, tau, lse, gg, dT, dQ, qrow, Qreg, Treg, dQr, dTr, n_split, mask=mask)
        outs.append((dQ, dT) if Qreg is None else (dQ, dT, dQr, dTr))
    ref = _bwd_ref(Qg, Tt, Qrg, Trg, tau, fwd, lse, g, S, R)
    for k, got in zip(("dQ", "dT", "dQr", "dTr"), outs[0]):
        chk.close(tag + k, got, *ref[k])
    # two launches: the same bits (no atomics, nothing read from the outputs), forward and backward
    res2, lse2, zt2 = rowops.catsoftmax_fwd(Q, Tt, target, tau, qrow, Qreg, Treg, n_split, mask=mask)
    assert _same_bits(res, res2) and _same_bits(lse, lse2) and _same_bits(zt, zt2)
    assert all(_same_bits(x, y) for x, y in zip(*outs))
    # the device's own two answers, row by row; zt does not know the mask
    _, lse_u, zt_u = rowops.catsoftmax_fwd(Q, Tt, target, tau, qrow, Qreg, Treg, n_split)
    assert bool((lse <= lse_u).all()), tag
    assert _same_bits(zt, zt_u)
    # a column that no row keeps live has a dT row of exact zeros
    dead = torch.from_numpy(ex.all(0)).to(DEV)
    assert float(outs[0][1][dead].abs().sum()) == 0.0
    if roles is not None:
        qr = np.arange(B) if qrow is None else qrow.cpu().numpy()
        only = np.nonzero(roles[qr] == 4)[0]
        for b in only[:2]:
            assert ex[b].sum() == N - 1
            assert _same_bits(lse[b:b + 1], zt[b:b + 1]) and float(lse[b] - zt[b]) == 0.0
            assert float(outs[0][0][b].abs().max()) == 0.0                   # the dQ row
            # alone in a batch it gives dT nothing at all (and dQ, and a loss of exactly zero)
            one = slice(b, b + 1)
            q1 = (Q[one] if qrow is None else Q, None if qrow is None else qrow[one].contiguous())
            m1 = mask if qrow is not None else (torch.stack([mask[0][b], mask[0][b + 1]]) - mask[0][b], mask[1][mask[0][b]:mask[0][b + 1]])
            r1, lse1, zt1 = rowops.catsoftmax_fwd(q1[0], Tt, target[one], tau, q1[1], n_split=n_split, mask=m1)
            dT1, dQ1 = _nan(N, D), _nan(1, D)
            rowops.catsoftmax_bwd(q1[0], Tt, target[one], tau, lse1, gg, dT1, dQ1, q1[1], n_split=n_split, mask=m1)
            assert float(r1[0]) == 0.0 and _same_bits(lse1, zt1)
            assert float(dT1.abs().max()) == 0.0 and float(dQ1.abs().max()) == 0.0
    return res, lse, outs[0], fwd, ref


def _case(chk, tag, B, N, D, tau, kind, n_split, sd, pad=0):
    """kind 0: rows read through qrow (a permutation with repeats into a larger table), distinct L2 tables of another width,
    g != (1, 1); 1: no qrow, no g, the L2 tables are the score tables; 2: qrow, no L2 term."""
    S, R = _splits(B, N, D, n_split)
    target = _targets(B, N, sd)
    nq = B + 5 if kind != 1 else B
    qrow = _qrows(B, nq, sd) if kind != 1 else None
    ptr, cols, roles, target = _lists(B, N, nq, qrow, target, S, R, sd)
    target = target.to(DEV)
    qrow = None if qrow is None else qrow.to(DEV)
    Tt, Q = _slot(N, D, sd + 1, pad), _slot(nq, D, sd + 2, pad)
    if kind == 0:
        return _run(chk, tag, Q, Tt, target, tau, (ptr, cols), qrow, _slot(nq, D + 4, sd + 3, pad), _slot(N, D + 4, sd + 4, pad),
                    (0.37, -2.0), n_split, pad, roles)
    if kind == 1:
        return _run(chk, tag, Q, Tt, target, tau, (ptr, cols), None, Q, Tt, None, n_split, pad, roles)
    return _run(chk, tag, Q, Tt, target, tau, (ptr, cols), qrow, g=(-1.5, 0.0), n_split=n_split, pad=pad, roles=roles)


@pytest.mark.parametrize("D", DS)
@pytest.mark.parametrize("B", BS)
def test_masked_kernels_against_fp64(B, D):
    """Every (B, N, D) at both temperatures; the operand kind and n_split (1, 2, 3, 7 and the default) rotate with the case."""
    chk = Chk(f"catsoftmax masked B={B} D={D}", tag="catsoftmax-masked")
    for i, N in enumerate(NS):
        for j, tau in enumerate(TAUS):
            n_split = (1, 2, 3, 7, 0)[(i + 2 * j + B) % 5]
            _case(chk, f"N={N}/{tau}/S={n_split} ", B, N, D, tau, (i + j) % 3, n_split, 1000 * B + 10 * N + D + j)
    chk.done()


@pytest.mark.parametrize("N", [130, 1000])
@pytest.mark.parametrize("n_split", SPLITS)
def test_masked_forced_splits(N, n_split):
    """Every merge shape: one range, ranges of unequal length, empty ranges, more ranges than column tiles, and rows whose
    range 0 is wholly excluded while the target lies in the last range (role 3: `_lists` moves it there)."""
    chk = Chk(f"catsoftmax masked N={N} n_split={n_split}", tag="catsoftmax-masked")
    for B, D, tau, kind in ((17, 64, 0.05, 0), (130, 100, 1.0, 1)):
        _, lse, _, fwd, _ = _case(chk, f"B={B} ", B, N, D, tau, kind, n_split, 7 * N + n_split + B)
        S, R = _splits(B, N, D, n_split)
        if N > R:                                                              # some row has nothing live in range 0
            assert (~fwd["live"][:, :R]).all(1).any()
    chk.done()


@pytest.mark.parametrize("pad", [4, 3])
def test_masked_strided_rows_nan_padding(pad):
    """ld > D: operands, L2 tables and dT are slots of wider buffers whose padding columns hold NaN; nothing reads or writes
    them.  pad = 4 keeps the rows 16-byte aligned (float4 staging), pad = 3 does not (scalar staging)."""
    chk = Chk(f"catsoftmax masked strided pad={pad}", tag="catsoftmax-masked")
    D = 100
    _, _, grads, _, _ = _case(chk, "", 70, 130, D, 0.05, 0, 2, 11, pad=pad)
    whole = torch.as_strided(grads[1], (grads[1].shape[0], D + pad), (D + pad, 1))
    assert grads[1].stride(0) == D + pad and torch.isnan(whole[:, D:]).all() and torch.isfinite(whole[:, :D]).all()
    chk.done()


def test_reference_gradients_are_the_restatements():
    """The coefficient formulas the bounds are hung on, against autograd through the restatement (fp64 against fp64)."""
    B, N, D, tau = 17, 130, 8, 0.5
    S, R = 2, 128
    target = _targets(B, N, 5)
    ptr, cols, _, target = _lists(B, N, B, None, target, S, R, 5)
    Q, Tt = _slot(B, D, 6).cpu().double().requires_grad_(), _slot(N, D, 7).cpu().double().requires_grad_()
    loss, _ = CM.masked_catalogue_loss64(Q, Tt, target, None, None, ptr.cpu(), cols.cpu(), tau)
    loss.backward()
    ex = CM.dense_mask(ptr, cols, target, N).numpy()
    fwd = _fwd_ref(Q.detach().float(), Tt.detach().float(), target, ex, None, None, tau, S, R, loss.detach())
    ref = _bwd_ref(Q.detach().float(), Tt.detach().float(), None, None, tau, fwd, torch.from_numpy(fwd["lse"][0]), None, S, R)
    assert np.abs(ref["dQ"][0] - Q.grad.numpy()).max() <= 1e-12 and np.abs(ref["dT"][0] - Tt.grad.numpy()).max() <= 1e-12
    assert (ref["C"][ex] == 0.0).all()


@pytest.mark.parametrize("B,N,D,tau,n_split,with_qrow", [(1, 5, 8, 1.0, 1, False), (17, 65, 64, 0.05, 2, True),
                                                         (65, 130, 100, 1.0, 7, False), (130, 1000, 256, 0.05, 0, True)])
def test_empty_lists_give_the_unmasked_bits(B, N, D, tau, n_split, with_qrow):
    """Every list empty: lse, zt, the two loss parts, dT, dQ and the L2 rows are the unmasked entry points' bits."""
    nq = B + 5 if with_qrow else B
    Q, Tt, Qr, Tr = _slot(nq, D, 1), _slot(N, D, 2), _slot(nq, D + 4, 3), _slot(N, D + 4, 4)
    qrow = _qrows(B, nq, 5).to(DEV) if with_qrow else None
    target = _targets(B, N, 6).to(DEV)
    mask = (torch.zeros(nq + 1, dtype=torch.int64, device=DEV), torch.zeros(0, dtype=torch.int32, device=DEV))
    gg = torch.tensor([0.37, -2.0], device=DEV)
    got = []
    for m in (None, mask):
        res, lse, zt = rowops.catsoftmax_fwd(Q, Tt, target, tau, qrow, Qr, Tr, n_split, mask=m)
        dT, dQ, dQr, dTr = _nan(N, D), _nan(B, D), _nan(B, D + 4), _nan(B, D + 4)
        rowops.catsoftmax_bwd(Q, Tt, target, tau, lse, gg, dT, dQ, qrow, Qr, Tr, dQr, dTr, n_split, mask=m)
        got.append((res, lse, zt, dT, dQ, dQr, dTr))
    assert all(bool(torch.isfinite(t).all()) for t in got[1])
    assert all(_same_bits(a, b) for a, b in zip(*got))


@pytest.mark.parametrize("tau,n_split", [(1.0, 1), (0.05, 3)])
def test_hot_excluded_columns_never_leak(tau, n_split):
    """A handful of columns is excluded for EVERY row, and their T rows are scaled so that their logits overflow expf (finite
    values: 0 x NaN would poison the dQ product legitimately).  Loss, lse and dQ are finite and within the bound of the
    reference on those lists, the dT rows of those columns are exactly zero; a leaked column would show as inf or NaN."""
    chk = Chk(f"catsoftmax masked hot tau={tau}", tag="catsoftmax-masked")
    B, N, D = 70, 200, 16
    hot = [0, 63, 64, 127, 128, N - 1]
    Q = _slot(B, D, 41).abs().contiguous()
    Tt = _slot(N, D, 42).clone()
    Tt[hot] = 1000.0
    target = torch.randint(1, 63, (B,), generator=torch.Generator().manual_seed(43)).to(DEV)
    rng = np.random.default_rng(44)
    lists = [sorted(set(hot) | set(rng.choice(N, size=b % 7, replace=False).tolist())) for b in range(B)]
    ptr = torch.tensor([0] + list(np.cumsum([len(l) for l in lists])), dtype=torch.int64, device=DEV)
    cols = torch.tensor([c for l in lists for c in l], dtype=torch.int32, device=DEV)
    res, lse, grads, fwd, _ = _run(chk, "", Q, Tt, target, tau, (ptr, cols), None, Q, Tt, (0.37, -2.0), n_split)
    assert (fwd["z"][:, hot] > 200.0).all() and not fwd["live"][:, hot].any()
    with np.errstate(over="ignore"):
        assert np.exp(np.float32(fwd["z"][:, hot].min())) == np.inf          # expf of such a logit is inf
    assert torch.isfinite(res).all() and torch.isfinite(lse).all() and all(torch.isfinite(t).all() for t in grads)
    assert float(grads[1][hot].abs().max()) == 0.0                           # the dT rows of the hot columns
    # unmasked, the same operands drown every row in the hot columns
    r_u, lse_u, _ = rowops.catsoftmax_fwd(Q, Tt, target, tau, n_split=n_split)
    assert float(lse_u.min()) > 200.0 > float(lse.max())
    chk.done()


def test_mask_arguments_are_checked():
    B, N, D = 4, 9, 8
    Q, Tt, target = torch.zeros(B, D, device=DEV), torch.zeros(N, D, device=DEV), torch.zeros(B, dtype=torch.int64, device=DEV)
    ptr, cols = torch.zeros(B + 1, dtype=torch.int64, device=DEV), torch.zeros(0, dtype=torch.int32, device=DEV)
    rowops.catsoftmax_fwd(Q, Tt, target, 1.0, mask=(ptr, cols))
    for bad in ((ptr[:-1], cols), (ptr.int(), cols), (ptr, cols.long()), (ptr.cpu(), cols), (ptr, cols.cpu()),
                (torch.zeros(2 * B + 2, dtype=torch.int64, device=DEV)[::2], cols), ptr, (ptr, cols, cols), (ptr, None)):
        with pytest.raises(T.TagrecError):
            rowops.catsoftmax_fwd(Q, Tt, target, 1.0, mask=bad)
    _, lse, _ = rowops.catsoftmax_fwd(Q, Tt, target, 1.0, mask=(ptr, cols))
    with pytest.raises(T.TagrecError):
        rowops.catsoftmax_bwd(Q, Tt, target, 1.0, lse, None, torch.empty_like(Tt), mask=(ptr[:-1], cols))
    # with qrow the CSR runs over the rows of Q, not over the batch
    Qbig = torch.zeros(B + 3, D, device=DEV)
    with pytest.raises(T.TagrecError):
        rowops.catsoftmax_fwd(Qbig, Tt, target, 1.0, qrow=target, mask=(ptr, cols))
