"""GPU: the DirectAU kernels (csrc/directau.hip) through rowops.directau_fwd / directau_bwd and help.align_uniform_loss,
against the fp64 restatement of tests/directau_torch.py.

Tolerance: this repository's rule: |got - ref64| <= c * 2^-24 * mag + extra, `c` counted off the kernels as
built and written beside each check; `extra` carries what enters through a slope and is itself such a count.
With u = 2^-24, the counts, once (expf / logf: 4 ulp = 8, as in tests/test_gpu_inbatch.py):

  inv             ss: ceil(D / 64) fmas per lane and the 6-step tree, on a sum of squares (relative: halved by the root, kept
                  whole); sqrtf 2, the clamp 0, the division 1: c_inv = ceil(D / 64) + 9, relative.
  x^ (staged)     x inv: c_h = c_inv + 1, relative per element.
  score s_ij      a D-term MFMA dot on rounded operands: (D + 2 c_h) on smag = sum_c |x^_ic| |x^_jc| (<= 1).
  z_ij            t2 (s - 1): the subtraction and the product (t2 = 2 t is exact for the t used here):
                  dz = 2 t ds + 2 u |z|.
  term w_ij       expf(z): 8 on w, and dz through the slope: w (8 u + dz).
  S (one side)    a lane adds its entries one by one, at most 16 per walked tile: 16 n_tiles; the wavefront tree 6, the four
                  wavefronts 2, the reduce kernel ceil(n_tiles / 256) + 8; all terms positive: c_S = 16 n_tiles + 16 +
                  ceil(n_tiles / 256), relative.
  ls              logf(S): 8 on |ls|; extra: u c_S + sum p (8 u + dz), p = w / S.
  unif            ls + log_pairs: the constant's rounding and the add, 2 on |ls| + |log_pairs|: c = 10, extra as ls.
  align           d = u inv_u - i inv_i: (c_h + 1) u (|u^| + |i^|) per element, entering sum d^2 by 2 |d|; the sum: ceil(D / 64)
                  fmas, the tree 6, the wavefronts 2, the reduce ceil(n_prep / 256) + 8, the float 1 / B and its product 2:
                  c = ceil(D / 64) + 18 + ceil(n_prep / 256) on mean sum d^2; extra: mean_b sum_c 2 |d| (c_h + 1) u (|u^| + |i^|).
  L2              2 ceil(Dreg / 64) fmas per lane (both rows into one sum), then as align: 2 ceil(Dreg / 64) + 18 + ceil(n_prep / 256).
  mul_loss        (uu + ui): 1; the fma with gamma / 2: 1: c = max(c_align, 10) + 2 on the magnitudes' sum, the extras added.
  C_ij            coef = (g0 (gamma / 2)) t2: 2; (z - ls): 1 on |z - ls|, and dz; expf 8; the product 1: 11 on |C|, extra
                  |C| (u |z - ls| + dz) -- plus |C| d(ls) where the reference does not start from the kernel's ls.
  G (unif part)   a B-term MFMA chain on rounded operands: B + c_h + 11 on sum_j |C_ij| |x^_jc|.
  G (align part)  ascale = g0 (2 (1 / B)): 2; (x^ - p inv_p): c_h + 1 on |x^| + |p^|; the fma into the accumulator 1 and 1 on
                  the total: c_h + 5.  Together c_G = B + 2 c_h + 17 on Gm_c = sum_j |C_ij| |x^_jc| + |ascale| (|x^_c| + |p^_c|).
  row dot         NF fmas per lane and four shuffles on rounded x^: NF + 4 + c_h on dotm = sum_c Gm_c |x^_c|.
  dX              inv (G_c - x^_c dot): the fma 1, x^'s c_h, inv's c_inv and its product 1.  In all
                  c = c_G + NF + 4 + 2 c_h + c_inv + 2 on inv_i (Gm_c + |x^_c| dotm); extra: inv_i (E_c + |x^_c| sum_c' E_c' |x^_c'|),
                  E_c = sum_j |C_ij| (u |z - ls| + dz) |x^_jc|.
  L2 rows         (g1 (1 / B)) x: 3; into the SAME buffer it joins by a product and an add: + 2 on |dX| + |r|.
Gradients of rows whose norm is below the clamp are not specified: they are checked to be finite only.
Each test prints its worst err / bound (`-s`)."""
import ctypes
import math

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import tagrec_amd as T
from tagrec_amd import _lib, help as H, rowops

import directau_torch as AU
from spmm_ref import EPS, U32, Chk, f64 as _f64, randn as _randn, same_bits as _same_bits

DEV = torch.device("cuda:0")
# 2, 3; both sides of the MFMA's 16 and of the block's row tile (64); 130: three blocks, three walked tiles, a ragged last tile
BS = (2, 3, 15, 16, 17, 63, 64, 65, 130)
DS = (8, 16, 64, 100, 176, 256)     # every accumulator count the backward is built for (1, 1, 4, 8, 12, 16 tiles), two ragged
TS = (0.5, 2.0, 20.0)
NFS = (1, 2, 4, 8, 12, 16)


def _cdiv(a, b):
    return -(-a // b)


def _counts(B, D):
    c_inv = _cdiv(D, 64) + 9
    nt, n_prep = _cdiv(B, 64), _cdiv(B, 4)
    return dict(inv=c_inv, h=c_inv + 1, S=16 * nt + 16 + _cdiv(nt, 256), align=_cdiv(D, 64) + 18 + _cdiv(n_prep, 256),
                n_prep=n_prep, nf=next(nf for nf in NFS if 16 * nf >= D))


def _side(X, t, c):
    """fp64 quantities of one side: x^, inv, which rows are clamped, z, dz, w, S, ls and ls's extra."""
    x = _f64(X)
    nrm = np.linalg.norm(x, axis=1)
    inv = 1.0 / np.maximum(nrm, EPS)
    xh = x * inv[:, None]
    s, smag = xh @ xh.T, np.abs(xh) @ np.abs(xh).T
    z = 2 * t * (s - 1.0)
    dz = 2 * t * (x.shape[1] + 2 * c["h"]) * U32 * smag + 2 * U32 * np.abs(z)
    w = np.triu(np.exp(z), 1)
    S = w.sum()
    ls = math.log(S)
    ls_extra = U32 * c["S"] + float((w / S * (8 * U32 + dz)).sum())
    return dict(xh=xh, inv=inv, clamped=nrm < EPS, z=z, dz=dz, S=S, ls=ls, ls_extra=ls_extra)


def _fwd_ref(Ub, Ib, Urb, Irb, t, gamma):
    """fp64 inv / ls / parts / res of compact operands, each with (ref, mag, c, extra) of the rule above, and what the
    backward's reference needs."""
    B, D = Ub.shape
    c = _counts(B, D)
    gamma = float(np.float32(gamma))
    su, si = _side(Ub, t, c), _side(Ib, t, c)
    want = AU.directau_loss64(Ub.cpu(), Ib.cpu(), None if Urb is None else Urb.cpu(), None if Irb is None else Irb.cpu(), t, gamma)
    logc = math.log(2.0 / (B * (B - 1)))
    d = su["xh"] - si["xh"]
    al = (d * d).sum(1)
    al_extra = (2 * np.abs(d) * (c["h"] + 1) * U32 * (np.abs(su["xh"]) + np.abs(si["xh"]))).sum(1).mean()
    parts = np.array([al.mean(), su["ls"] + logc, si["ls"] + logc])
    assert np.abs(parts - want[2].numpy()).max() <= 1e-11 * max(1.0, np.abs(parts).max())      # the restatement says the same
    pmag = np.array([al.mean(), abs(su["ls"]) + abs(logc), abs(si["ls"]) + abs(logc)])
    pextra = np.array([al_extra, su["ls_extra"], si["ls_extra"]])
    out = {"c": c, "u": su, "i": si, "gamma": gamma,
           "inv": (np.concatenate([su["inv"], si["inv"]]), np.concatenate([su["inv"], si["inv"]]), c["inv"], 0.0),
           "ls": (np.array([su["ls"], si["ls"]]), np.abs([su["ls"], si["ls"]]), 8, np.array([su["ls_extra"], si["ls_extra"]])),
           "parts": (parts, pmag, np.array([c["align"], 10, 10]), pextra),
           "loss": (float(want[0]), pmag[0] + gamma / 2 * (pmag[1] + pmag[2]), max(c["align"], 10) + 2,
                    pextra[0] + gamma / 2 * (pextra[1] + pextra[2]))}
    if Urb is not None:
        ss = float(want[1])
        out["reg"] = (ss, ss, 2 * _cdiv(Urb.shape[1], 64) + 18 + _cdiv(c["n_prep"], 256), 0.0)
    else:
        out["reg"] = None
    return out


def _check_fwd(chk, tag, ref, res, parts, state):
    chk.close(tag + "inv", state.inv, *ref["inv"])
    chk.close(tag + "ls", state.ls, *ref["ls"])
    chk.close(tag + "parts", parts, *ref["parts"])
    chk.close(tag + "loss", res[0], *ref["loss"])
    if ref["reg"] is None:
        assert float(res[1]) == 0.0
    else:
        chk.close(tag + "reg", res[1], *ref["reg"])


def _autograd64(Ub, Ib, Urb, Irb, t, gamma, g, ls, shared):
    """Gradients of the restatement under autograd.  ls given (the kernel's own, two floats): log S is linearised there --
    d log S = dS / exp(ls) -- which is what a backward that starts from the forward's ls computes; None: from scratch."""
    g0, g1 = (1.0, 1.0) if g is None else (float(np.float32(g[0])), float(np.float32(g[1])))
    U, I = Ub.detach().cpu().double().requires_grad_(), Ib.detach().cpu().double().requires_grad_()
    if ls is None:
        un = AU.uniform64(U, t) + AU.uniform64(I, t)
    else:
        un = AU.pair_terms64(U, t).sum() * math.exp(-float(ls[0])) + AU.pair_terms64(I, t).sum() * math.exp(-float(ls[1]))
    loss = g0 * (AU.align64(U, I) + gamma * un / 2)
    leaves = [U, I]
    if Urb is not None:
        Ur, Ir = (U, I) if shared else (Urb.detach().cpu().double().requires_grad_(), Irb.detach().cpu().double().requires_grad_())
        loss = loss + g1 * 0.5 * (Ur.pow(2).sum() + Ir.pow(2).sum()) / Ub.shape[0]
        if not shared:
            leaves += [Ur, Ir]
    return [x.numpy() for x in torch.autograd.grad(loss, leaves)]


def _bwd_ref(Ub, Ib, Urb, Irb, t, fwd, ls, g, shared=False, scratch=False):
    """{name: [ref, mag, c, extra]} of the gradients, the reference by autograd of the restatement (from the kernel's ls, or
    from scratch: ls's own bound then enters C), the bound from the counts above; rows below the clamp are listed in "skip"."""
    B, D = Ub.shape
    c, gamma = fwd["c"], fwd["gamma"]
    g0, g1 = (1.0, 1.0) if g is None else (float(np.float32(g[0])), float(np.float32(g[1])))
    refs = _autograd64(Ub, Ib, Urb, Irb, t, gamma, g, None if scratch else _f64(ls), shared)
    cc = (B + 2 * c["h"] + 17) + c["nf"] + 4 + 2 * c["h"] + c["inv"] + 2
    out, skip = {}, {}
    for k, (sd, other, ref) in enumerate(((fwd["u"], fwd["i"], refs[0]), (fwd["i"], fwd["u"], refs[1]))):
        name = ("dU", "dI")[k]
        lsv = sd["ls"] if scratch else float(_f64(ls)[k])
        a = sd["z"] - lsv
        C = np.abs(g0) * gamma * t * np.exp(a)
        np.fill_diagonal(C, 0.0)
        dls = (8 * U32 * abs(sd["ls"]) + sd["ls_extra"]) if scratch else 0.0
        xa, pa = np.abs(sd["xh"]), np.abs(other["xh"])
        Gm = C @ xa + abs(g0) * 2.0 / B * (xa + pa)
        E = (C * (U32 * np.abs(a) + sd["dz"] + dls)) @ xa
        dotm, Ed = (Gm * xa).sum(1, keepdims=True), (E * xa).sum(1, keepdims=True)
        inv = sd["inv"][:, None]
        out[name] = [ref, inv * (Gm + xa * dotm), cc, inv * (E + xa * Ed)]
        skip[name] = sd["clamped"]
    if Urb is not None:
        ur, ir = g1 / B * _f64(Urb), g1 / B * _f64(Irb)
        if shared:
            for k, r in (("dU", ur), ("dI", ir)):
                out[k] = [out[k][0], out[k][1] + np.abs(r), out[k][2] + 5, out[k][3]]
        else:
            assert np.abs(refs[2] - ur).max() <= 1e-15 + 1e-12 * np.abs(ur).max()
            out["dUr"], out["dIr"] = [ur, np.abs(ur), 3, 0.0], [ir, np.abs(ir), 3, 0.0]
    return out, skip


def _check_bwd(chk, tag, ref, skip, outs):
    for k, got in zip(("dU", "dI", "dUr", "dIr"), outs):
        assert torch.isfinite(got).all(), tag + k
        r = ref[k]
        if k in skip and skip[k].any():
            keep = ~skip[k]
            r = [r[0][keep], r[1][keep], r[2], r[3][keep]]
            got = got[torch.from_numpy(keep).to(got.device)]
        chk.close(tag + k, got, *r)


def _slot(n, d, seed, pad=0, scale=0.35):
    """[n, d] on the GPU; pad > 0: a slot of a NaN-padded wider buffer (row stride d + pad)."""
    buf = torch.full((n, d + pad), float("nan"))
    buf[:, :d] = _randn(n, d, seed=seed, scale=scale)
    return buf.to(DEV)[:, :d]


def _nan_like(t, pad=0):
    return torch.full((t.shape[0], t.shape[1] + pad), float("nan"), device=DEV)[:, :t.shape[1]]


def _run(chk, tag, Ub, Ib, Urb, Irb, t, gamma=1.0, g=None, pad=0, scratch=False):
    """Forward, backward and the repeat of both on one operand set; Urb is Ub: one gradient buffer for both parts."""
    shared = Urb is Ub
    res, parts, state = rowops.directau_fwd(Ub, Ib, Urb, Irb, t, gamma)
    fwd = _fwd_ref(Ub, Ib, Urb, Irb, t, gamma)
    _check_fwd(chk, tag, fwd, res, parts, state)
    gg = None if g is None else torch.tensor(g, dtype=torch.float32, device=DEV)
    outs = []
    for _ in range(2):       # every output pre-filled with NaN must be fully overwritten
        dU, dI = _nan_like(Ub, pad), _nan_like(Ib, pad)
        dUr, dIr = (dU, dI) if shared else ((_nan_like(Urb, pad), _nan_like(Irb, pad)) if Urb is not None else (None, None))
        rowops.directau_bwd(Ub, Ib, Urb, Irb, state, gg, dU, dI, dUr, dIr)
        outs.append((dU, dI) if (shared or Urb is None) else (dU, dI, dUr, dIr))
    ref, skip = _bwd_ref(Ub, Ib, Urb, Irb, t, fwd, state.ls, g, shared)
    _check_bwd(chk, tag, ref, skip, outs[0])
    if scratch:
        ref, skip = _bwd_ref(Ub, Ib, Urb, Irb, t, fwd, None, g, shared, scratch=True)
        _check_bwd(chk, tag + "scratch ", ref, skip, outs[0])
    # two launches: the same bits (no atomics, nothing read from the outputs), forward and backward
    res2, parts2, state2 = rowops.directau_fwd(Ub, Ib, Urb, Irb, t, gamma)
    assert _same_bits(res, res2) and _same_bits(parts, parts2) and _same_bits(state.inv, state2.inv) and _same_bits(state.ls, state2.ls)
    assert all(_same_bits(x, y) for x, y in zip(*outs))
    return res, parts, state, outs[0], fwd


@pytest.mark.parametrize("D", DS)
@pytest.mark.parametrize("B", BS)
def test_directau_kernels_against_fp64(B, D):
    """Every (B, D) at the three t: (a) everything on -- distinct L2 rows of another width, upstream g = (0.3, -2), gamma != 1,
    repeated users and items; (b) everything off -- L2 on the score rows into one buffer, no g.  At t = 2 the gradients are
    also held to the restatement from scratch."""
    chk = Chk(f"directau B={B} D={D}", tag="directau")
    for i, t in enumerate(TS):
        sd = 100 * B + D + 7 * i
        Ub, Ib = _slot(B, D, sd), _slot(B, D, sd + 1)
        if B >= 15:                      # repeated ids: the gathered rows repeat (their pair term is exp(0))
            Ub[B // 2], Ub[B - 1], Ib[3] = Ub[0], Ub[0], Ib[B - 2]
        Urb, Irb = _slot(B, D + 4, sd + 2), _slot(B, D + 4, sd + 3)
        _run(chk, f"a/{t} ", Ub, Ib, Urb, Irb, t, gamma=0.7, g=(0.3, -2.0), scratch=(t == 2.0))
        _run(chk, f"b/{t} ", Ub, Ib, Ub, Ib, t)
    chk.done()


@pytest.mark.parametrize("B", [130, 200])
def test_triangular_sum_against_brute_force(B):
    """exp(ls) against a brute-force fp64 sum over all i < j of exp(-t |x^_i - x^_j|^2) (differences, not the Gram form): a
    tile walked twice or skipped moves S by whole terms."""
    chk = Chk(f"directau triangular B={B}", tag="directau")
    D, t = 16, 0.5                       # a flat potential: every pair carries weight
    Ub, Ib = _slot(B, D, 5 + B), _slot(B, D, 6 + B)
    _, _, state = rowops.directau_fwd(Ub, Ib, None, None, t, 1.0)
    fwd = _fwd_ref(Ub, Ib, None, None, t, 1.0)
    for k, X in enumerate((Ub, Ib)):
        xh = AU.normalize64(X.cpu())
        S = 0.0
        for i in range(B - 1):
            S += float(torch.exp(-t * (xh[i + 1:] - xh[i]).pow(2).sum(1)).sum())
        assert abs(S - fwd["ui"[k]]["S"]) <= 1e-12 * S
        chk.close(f"ls[{k}]", state.ls[k], math.log(S), abs(math.log(S)), 8, fwd["ui"[k]]["ls_extra"])
        assert float((AU.pair_terms64(X.cpu(), t) / S).min()) > 0.1 / (B * B)      # no pair is negligible
    chk.done()


@pytest.mark.parametrize("pad", [4, 3])
def test_directau_strided_rows_nan_padding(pad):
    """ld > D: operands and gradient buffers are slots of wider buffers whose padding columns hold NaN; nothing reads or writes
    them.  pad = 4 keeps the rows 16-byte aligned (float4 staging), pad = 3 does not (scalar staging)."""
    chk = Chk(f"directau strided pad={pad}", tag="directau")
    B, D, t = 70, 100, 2.0
    Ub, Ib = _slot(B, D, 11, pad), _slot(B, D, 12, pad)
    Urb, Irb = _slot(B, D, 13, pad), _slot(B, D, 14, pad)
    *_, grads, _ = _run(chk, "distinct ", Ub, Ib, Urb, Irb, t, g=(0.3, -2.0), pad=pad)
    *_, grads2, _ = _run(chk, "shared ", Ub, Ib, Ub, Ib, t, g=(0.3, -2.0), pad=pad)
    for x in (Ub, Ib, Urb, Irb) + tuple(grads) + tuple(grads2):
        assert x.stride(0) == D + pad
        whole = torch.as_strided(x, (B, D + pad), (D + pad, 1))
        assert torch.isnan(whole[:, D:]).all() and torch.isfinite(whole[:, :D]).all()
    chk.done()


def test_shared_l2_buffer_equals_the_separate_one():
    """dUreg is dUb: each row receives the sum of what the separate buffers receive (one more rounding: the add)."""
    chk = Chk("directau shared L2", tag="directau")
    B, D, t = 70, 64, 2.0
    Ub, Ib = _slot(B, D, 21), _slot(B, D, 22)
    g = torch.tensor([0.3, -2.0], device=DEV)
    _, _, state = rowops.directau_fwd(Ub, Ib, Ub, Ib, t, 1.0)
    sep = [torch.empty_like(Ub) for _ in range(4)]
    rowops.directau_bwd(Ub, Ib, Ub, Ib, state, g, *sep)
    sh = [torch.empty_like(Ub) for _ in range(2)]
    rowops.directau_bwd(Ub, Ib, Ub, Ib, state, g, sh[0], sh[1], sh[0], sh[1])
    for k in range(2):
        want = _f64(sep[k]) + _f64(sep[2 + k])
        chk.close(("dU", "dI")[k], sh[k], want, np.abs(_f64(sep[k])) + np.abs(_f64(sep[2 + k])), 2)   # the product is re-formed: 1; the add: 1
    chk.done()


def test_antipodal_pair_at_the_largest_t():
    """B = 2, x_1 = -2.5 x_0, t = 20: the one term is e^-80 = 1.8e-35, a normal float; unif is -80 within the bound and every
    gradient is finite."""
    chk = Chk("directau antipodal", tag="directau")
    D, t = 16, 20.0
    x = _randn(1, D, seed=3, scale=0.5)
    Ub = torch.cat([x, -2.5 * x]).to(DEV)
    Ib = torch.cat([-0.5 * x, 3.0 * x]).to(DEV)
    res, parts, state, grads, fwd = _run(chk, "", Ub, Ib, Ub, Ib, t)
    # s = -1 up to (D + 2 c_h) u: z = -80 up to dz; unif = ls + log(1): 10 on 80 and the extra of ls
    for k in (1, 2):
        assert abs(float(parts[k]) + 80.0) <= 10 * U32 * 80.0 + fwd["ui"[k - 1]]["ls_extra"]
    assert 1e-35 < math.exp(float(state.ls[0])) < 3e-35
    assert torch.isfinite(res).all() and all(torch.isfinite(x).all() for x in grads)
    chk.done()


def test_a_zero_row_leaves_everything_finite():
    """One all-zero user row and one item row of norm 1e-13 (both below the clamp): x^ is 0 / short of unit length, so the
    Gram form 2 - 2 s is no longer the squared distance and the value is not the restatement's -- what is asked is that every
    output is finite, inv is the clamp's 1e12 and two launches give the same bits."""
    chk = Chk("directau zero row", tag="directau")
    B, D, t = 20, 16, 2.0
    Ub, Ib = _slot(B, D, 31), _slot(B, D, 32)
    Ub[5] = 0.0
    Ib[7] = Ib[7] / Ib[7].double().norm().float() * 1e-13
    g = torch.tensor([0.3, -2.0], device=DEV)
    runs = []
    for _ in range(2):
        res, parts, state = rowops.directau_fwd(Ub, Ib, Ub, Ib, t, 1.0)
        dU, dI = _nan_like(Ub), _nan_like(Ib)
        rowops.directau_bwd(Ub, Ib, Ub, Ib, state, g, dU, dI, dU, dI)
        runs.append((res, parts, state.inv, state.ls, dU, dI))
    for x in runs[0]:
        assert torch.isfinite(x).all()
    assert all(_same_bits(a, b) for a, b in zip(*runs))
    c = _counts(B, D)
    ref = np.concatenate([_side(Ub, t, c)["inv"], _side(Ib, t, c)["inv"]])
    assert ref[5] == 1e12 and ref[B + 7] == 1e12 and (ref < 1e3).sum() == 2 * B - 2
    chk.close("inv", runs[0][2], ref, ref, c["inv"])
    chk.done()


def test_directau_fwd_overwrites_poisoned_outputs_and_leaves_the_guard_row():
    """The C entries themselves with every output pre-filled with NaN: every element of rows < B is overwritten; a guard row
    past B in the gradient buffers and a guard element past inv, ls, parts and the result keep their bits."""
    B, D, t, gamma = 130, 64, 2.0, 1.0
    Ub, Ib = _slot(B, D, 61), _slot(B, D, 62)
    n_part = 2 * ((B + rowops.AU_PREP_ROWS - 1) // rowops.AU_PREP_ROWS) + 2 * ((B + rowops.AU_TILE - 1) // rowops.AU_TILE)
    nan = float("nan")
    inv, ls, parts, res = (torch.full((n,), nan, device=DEV) for n in (2 * B + 1, 3, 4, 3))
    partials = torch.full((n_part + 1,), nan, device=DEV)
    p, f = _lib.ptr, ctypes.c_float
    _lib.check(_lib.load().tagrec_directau_fwd_f32(p(Ub), p(Ib), D, D, p(Ub), p(Ib), D, D, B, f(t), f(gamma), p(inv), p(ls),
                                                   p(partials), p(parts), p(res), _lib.stream_ptr()))
    for x in (inv, ls, parts, res, partials):
        assert torch.isfinite(x[:-1]).all() and torch.isnan(x[-1])
    res2, parts2, state = rowops.directau_fwd(Ub, Ib, Ub, Ib, t, gamma)
    assert _same_bits(res[:2], res2) and _same_bits(parts[:3], parts2) and _same_bits(inv[:-1], state.inv) and _same_bits(ls[:2], state.ls)
    bufs = [torch.full((B + 1, D), nan, device=DEV) for _ in range(4)]
    _lib.check(_lib.load().tagrec_directau_bwd_f32(p(Ub), p(Ib), D, D, p(Ub), p(Ib), D, D, B, f(t), f(gamma), p(state.inv),
                                                   p(state.ls), p(None), *(p(b) for b in bufs), _lib.stream_ptr()))
    for b in bufs:
        assert torch.isfinite(b[:B]).all() and torch.isnan(b[B]).all()


def test_directau_refuses_bad_arguments():
    def ops(B, D):
        return torch.ones(B, D, device=DEV), torch.ones(B, D, device=DEV)
    for D in (6, 260, 4):                                            # not a multiple of 4, past 256, below 8
        with pytest.raises(T.TagrecError, match="D must be"):
            rowops.directau_fwd(*ops(4, D), None, None, 2.0, 1.0)
    Ub, Ib = ops(4, 8)
    for B in (0, 1):
        with pytest.raises(T.TagrecError):
            rowops.directau_fwd(*ops(B, 8), None, None, 2.0, 1.0)
    with pytest.raises(T.TagrecError):
        rowops.directau_fwd(Ub, Ib[:3], None, None, 2.0, 1.0)
    with pytest.raises(T.TagrecError):
        rowops.directau_fwd(Ub, Ib, Ub, None, 2.0, 1.0)
    for t in (0.0, -1.0, 20.5, float("inf"), float("nan")):
        with pytest.raises(T.TagrecError, match="t must be"):
            rowops.directau_fwd(Ub, Ib, None, None, t, 1.0)
    for gamma in (-0.5, float("inf"), float("nan")):
        with pytest.raises(T.TagrecError, match="gamma"):
            rowops.directau_fwd(Ub, Ib, None, None, 2.0, gamma)
    res, parts, state = rowops.directau_fwd(Ub, Ib, None, None, 20.0, 0.0)
    assert torch.isfinite(res).all() and torch.isfinite(parts).all()
    dU, dI = torch.empty_like(Ub), torch.empty_like(Ib)
    with pytest.raises(T.TagrecError):
        rowops.directau_bwd(Ub, Ib, None, None, rowops.AuState(2.0, 1.0, state.inv[:7], state.ls, None), None, dU, dI, None, None)
    with pytest.raises(T.TagrecError):
        rowops.directau_bwd(Ub, Ib, None, None, state, None, dU, None, None, None)
    with pytest.raises(T.TagrecError):                               # a shared buffer needs Ureg = Ub
        rowops.directau_bwd(Ub, Ib, Ub.clone(), Ib.clone(), state, None, dU, dI, dU, dI)


# ================================================================================================ help.align_uniform_loss
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
@pytest.mark.parametrize("planned", [False, True])
def test_align_uniform_loss_on_tables(same, planned):
    """help.align_uniform_loss: loss parts against the restatement on the tables; gradients against the fp64 scatter of the
    compact reference (the kernel's own ls), c = the compact count + the row's multiplicity (one addition of the fold per slot
    that names the row).  same: the L2 tables are the score tables (one buffer).  planned: the fold runs in a fixed order, the
    same bits on every run."""
    chk = Chk(f"align_uniform_loss same={same} planned={planned}", tag="directau")
    nu, ni, B, t, gamma = 50, 60, 48, 2.0, 0.7
    W, E, pairs = _tables_and_pairs(nu, ni, B=B)
    pg = pairs.to(DEV)
    Eb = W if same else E
    runs, g = [], [0.3, -2.0]
    for _ in range(2 if planned else 1):
        U, I = W[:nu].clone().requires_grad_(), W[nu:].clone().requires_grad_()
        Ur, Ir = (U, I) if same else (E[:nu].clone().requires_grad_(), E[nu:].clone().requires_grad_())
        plans = H.in_batch_plans(pg, nu, ni, W.shape[1]) if planned else None
        parts = []
        loss, reg = H.align_uniform_loss(U, I, Ur, Ir, pg, t, gamma, plans, parts_out=parts)
        (g[0] * loss + g[1] * reg).backward()
        runs.append([loss.detach(), reg.detach(), parts[0], U.grad, I.grad] + ([] if same else [Ur.grad, Ir.grad]))
    if planned:
        assert all(_same_bits(a, b) for a, b in zip(*runs))
    want = AU.directau_tables64(W[:nu].cpu(), W[nu:].cpu(), Eb[:nu].cpu(), Eb[nu:].cpu(), pairs, t, float(np.float32(gamma)))
    ur, ir = pg[:, 0].contiguous(), pg[:, 1].contiguous()
    Ub, Ib = W[:nu].index_select(0, ur), W[nu:].index_select(0, ir)
    Urb, Irb = (Ub, Ib) if same else (Eb[:nu].index_select(0, ur), Eb[nu:].index_select(0, ir))
    fwd = _fwd_ref(Ub, Ib, Urb, Irb, t, gamma)
    assert abs(float(want[0]) - fwd["loss"][0]) <= 1e-12 and abs(float(want[1]) - fwd["reg"][0]) <= 1e-12
    chk.close("loss", runs[0][0], *fwd["loss"])
    chk.close("reg", runs[0][1], *fwd["reg"])
    chk.close("parts", runs[0][2], *fwd["parts"])
    _, _, state = rowops.directau_fwd(Ub, Ib, Urb, Irb, t, gamma)
    b, _ = _bwd_ref(Ub, Ib, Urb, Irb, t, fwd, state.ls, g, shared=same)
    un, inn = pairs[:, 0].numpy(), pairs[:, 1].numpy()
    checks = [("dU", runs[0][3], nu, un), ("dI", runs[0][4], ni, inn)] + ([] if same else [("dUr", runs[0][5], nu, un), ("dIr", runs[0][6], ni, inn)])
    for k, got, n, idx in checks:
        mult = _scatter64(n, idx, np.ones((B, 1)))
        chk.close(k, got, _scatter64(n, idx, b[k][0]), _scatter64(n, idx, b[k][1]), b[k][2] + mult,
                  _scatter64(n, idx, np.broadcast_to(b[k][3], b[k][0].shape)))
    assert float(_scatter64(nu, un, np.ones((B, 1))).max()) >= 12.0       # user 7's multiplicity
    chk.done()


def test_align_uniform_loss_refuses_a_wrong_batch():
    W, E, pairs = _tables_and_pairs()
    with pytest.raises(T.TagrecError):
        H.align_uniform_loss(W[:50], W[50:], None, None, torch.cat([pairs, pairs[:, :1]], 1).to(DEV))
    with pytest.raises(T.TagrecError):
        H.align_uniform_loss(W[:50], W[50:], None, None, pairs[:1].to(DEV))
    with pytest.raises(T.TagrecError):
        H.align_uniform_loss(W[:50].cpu(), W[50:].cpu(), None, None, pairs)
