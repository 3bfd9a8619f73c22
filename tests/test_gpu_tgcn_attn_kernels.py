"""GPU: every entry point of the TGCN neighbour attention -- csrc/tgcn.hip (attn_fwd, attn_bwd in its scatter and dh forms,
attn_bwd_ds, attn_seg_dq, attn_keys, attn_invert_fill, nbr_gather, inv_filter) and the two destination-centric pulls of
csrc/spmm.hip (attn_pull_da, attn_pull_dq) -- each against the plain fp64 restatement of its own operation in
tests/tgcn_attn_ref.py (held to torch autograd in fp64 and to the oracle by test_tgcn_attn_ref_host.py).

Tolerance: the convention of test_gpu_spmm.py (spmm_ref.Chk): |got - ref64| <= c * 2^-24 * mag + extra + 1e-30, the counts `c`
those of the header of tgcn_attn_ref.py, written beside each check; a destination of more than 1024 pairs is held to two (pairs
+ chunks, and the depth of its lane tree).  A backward kernel is compared from ITS OWN inputs (the attention weights, da, comp
as the previous kernel stored them), so no error is carried from one kernel into the next one's bound.  Every test prints its
worst err / bound (`-s`); DESIGN section 2 carries the table.

Inputs (tgcn_attn_ref.make_case): P, Q, WT on the grid 2^-8 Z, so h = P + WT + Q is exact in fp32, [h > 0] is the same set in
the kernel and in fp64 and h == 0 occurs exactly (planted): no element is left out of any comparison, the relu bits of `comp`
and the zeros of dh are asserted bit for bit.  Tables with pads in every slot, an all-pad row, a destination listed twice / k
times by one row, an unlisted destination, destinations of 1100 and 2 * 512 + 1 pairs (long rows of the pulls), weight ids at
pad slots, WT[0] != 0.  Every output a kernel documents as written starts as NaN.

NOT bit-reproducible, and not asserted to be: dWT and dv (LDS float atomics form the per-block partial sums; the fold after
them is in fixed order), dQ / dEj of the scatter form and dQ of attn_seg_dq (global float atomics).  They are held to their
bounds only.  attn_fwd, dP / dh / comp, attn_pull_da and attn_pull_dq are run twice and must agree bit for bit."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from tagrec_amd import _lib
from tagrec_amd import tgcn_step as TS
from tagrec_amd.graph import Graph

import tgcn_attn_ref as AR
from spmm_ref import Chk as _Chk, f64, same_bits
from test_gpu_spmm import DEV, dev, nan_like

E_INVALID, E_UNSUPPORTED = -1, -3
FLOATS = ("P", "Q", "WT", "v", "Ej", "dOut")


def Chk(name):
    chk = _Chk(name, tag="tgcn_attn")
    chk.exact = []
    return chk


def _done(chk):
    chk.done()
    for what, holds in chk.exact:
        assert holds, f"{chk.name}: {what}"


def _exact(chk, what, holds):
    chk.exact.append((what, bool(holds)))


def _np(t):
    return t.detach().cpu().numpy()


def _all_nan(*ts):
    return all(bool(torch.isnan(t).all()) for t in ts)


def _case(n, n_dst, k, D, A, n_wt, seed, **kw):
    c = AR.make_case(n, n_dst, k, D, A, n_wt, seed, **kw)
    c["g"] = {kk: dev(c[kk]) for kk in FLOATS + ("idx", "widx")}
    return c


# ========================================================================================================= direct calls
def _ws(n_wt, A):
    n = _lib.load().tagrec_tgcn_attn_workspace(n_wt, A)
    return nan_like(n), n


def _fwd(c, g=None, rc=False, k=None, D=None, A=None, attn=None, out=None):
    g = g or c["g"]
    attn = nan_like(c["n"], c["k"]) if attn is None else attn
    out = nan_like(c["n"], c["D"]) if out is None else out
    r = _lib.load().tagrec_tgcn_attn_fwd_f32(_lib.ptr(g["P"]), _lib.ptr(g["Q"]), _lib.ptr(g["WT"]), _lib.ptr(g["v"]), _lib.ptr(g["Ej"]),
                                             _lib.ptr(g["idx"]), _lib.ptr(g["widx"]), c["n"], c["k"] if k is None else k,
                                             c["D"] if D is None else D, c["A"] if A is None else A, _lib.ptr(attn), _lib.ptr(out),
                                             _lib.stream_ptr())
    if rc:
        return r, (attn, out)
    _lib.check(r, "attn_fwd")
    return attn, out


def _bwd(c, attn, pull, g=None, rc=False, k=None, D=None, A=None, n_wt=None, ws=None):
    """attn_bwd -> dict; the scatter form adds into zeroed dQ / dEj, the dh form writes dh"""
    g = g or c["g"]
    n, kk, AA = c["n"], c["k"], c["A"]
    o = {"dP": nan_like(n, AA), "dWT": nan_like(c["n_wt"], AA), "dv": nan_like(AA)}
    if pull:
        o["dh"] = nan_like(n, kk, AA)
    else:
        o["dQ"], o["dEj"] = torch.zeros(c["n_dst"], AA, device=DEV), torch.zeros(c["n_dst"], c["D"], device=DEV)
    w, w_n = _ws(c["n_wt"], AA) if ws is None else ws
    r = _lib.load().tagrec_tgcn_attn_bwd_f32(_lib.ptr(g["P"]), _lib.ptr(g["Q"]), _lib.ptr(g["WT"]), _lib.ptr(g["v"]), _lib.ptr(g["Ej"]),
                                             _lib.ptr(g["idx"]), _lib.ptr(g["widx"]), _lib.ptr(attn), _lib.ptr(g["dOut"]), n,
                                             kk if k is None else k, c["D"] if D is None else D, AA if A is None else A,
                                             c["n_wt"] if n_wt is None else n_wt, _lib.ptr(o["dP"]), _lib.ptr(o.get("dQ")),
                                             _lib.ptr(o.get("dEj")), _lib.ptr(o.get("dh")), _lib.ptr(o["dWT"]), _lib.ptr(o["dv"]),
                                             _lib.ptr(w), w_n, _lib.stream_ptr())
    if rc:
        return r, o
    _lib.check(r, "attn_bwd")
    return o


def _bwd_ds(c, attn, da, w_major=-1, g=None, rc=False, k=None, A=None, n_wt=None, ws=None, comp=None):
    g = g or c["g"]
    n, kk, AA = c["n"], c["k"], c["A"]
    o = {"dP": nan_like(n, AA), "dWT": nan_like(c["n_wt"], AA), "dv": nan_like(AA),
         "comp": nan_like(n * kk, 2) if comp is None else comp}
    w, w_n = _ws(c["n_wt"], AA) if ws is None else ws
    r = _lib.load().tagrec_tgcn_attn_bwd_ds_f32(_lib.ptr(g["P"]), _lib.ptr(g["Q"]), _lib.ptr(g["WT"]), _lib.ptr(g["v"]), _lib.ptr(g["idx"]),
                                                _lib.ptr(g["widx"]), _lib.ptr(attn), _lib.ptr(da), n, kk if k is None else k,
                                                AA if A is None else A, c["n_wt"] if n_wt is None else n_wt, int(w_major),
                                                _lib.ptr(o["dP"]), _lib.ptr(o["comp"]), _lib.ptr(o["dWT"]), _lib.ptr(o["dv"]),
                                                _lib.ptr(w), w_n, _lib.stream_ptr())
    if rc:
        return r, o
    _lib.check(r, "attn_bwd_ds")
    return o


class Inv:
    """A table inverted on the device the way attn_bwd_pulls does it (attn_keys, a stable sort, attn_invert_fill), every
    integer array held to its restatement bit for bit; `g`: rows = destinations, col = source rows, val = attention weights."""

    def __init__(self, chk, c, attn):
        lib, n, k, n_dst = _lib.load(), c["n"], c["k"], c["n_dst"]
        idx = c["g"]["idx"]
        key = torch.full((n * k,), -7, dtype=torch.int32, device=DEV)
        _lib.check(lib.tagrec_attn_keys_i32(_lib.ptr(idx), n * k, n_dst, _lib.ptr(key), _lib.stream_ptr()), "attn_keys")
        self.skey, order = torch.sort(key, stable=True)
        self.pair = torch.full((n * k,), -7, dtype=torch.int32, device=DEV)
        self.src = torch.full((n * k,), -7, dtype=torch.int32, device=DEV)
        self.val = nan_like(n * k)
        _lib.check(lib.tagrec_attn_invert_fill(_lib.ptr(order), _lib.ptr(attn), k, n * k, _lib.ptr(self.pair), _lib.ptr(self.src),
                                               _lib.ptr(self.val), _lib.stream_ptr()), "attn_invert_fill")
        self.rowptr = torch.searchsorted(self.skey, torch.arange(n_dst + 1, dtype=torch.int32, device=DEV))
        skey, order_h, rowptr = AR.invert(c["idx"], n_dst)
        pair, src, val = AR.attn_invert_fill(order_h, _np(attn), k)
        _exact(chk, "attn_keys == its restatement", np.array_equal(_np(key), AR.attn_keys(c["idx"], n_dst)))
        _exact(chk, "sorted keys, row pointer", np.array_equal(_np(self.skey), skey) and np.array_equal(_np(self.rowptr), rowptr))
        _exact(chk, "attn_invert_fill == its restatement", np.array_equal(_np(self.pair), pair) and np.array_equal(_np(self.src), src)
               and np.array_equal(_np(self.val).view(np.int32), val.view(np.int32)))
        self.total = int(rowptr[-1])
        _exact(chk, "no pad pair in the listed part of pair / src",
               (c["idx"].reshape(-1)[_np(self.pair)[:self.total]] > 0).all() and self.total == (c["idx"] > 0).sum())
        self.deg, self.rowptr_h = np.diff(rowptr), rowptr
        self.g = Graph(self.rowptr, self.src, self.val, (n_dst, n), workspace=True, deferred=True)
        self.gq = None

    def pairs_graph(self):
        if self.gq is None:
            self.gq = self.g.like(self.pair, self.val, self.pair.numel())
        return self.gq


def _pull_da(c, inv, B=None, out=None, g=None, rc=False, D=None):
    g = g or c["g"]
    dEj = nan_like(c["n_dst"], c["D"]) if out is None else out
    da = nan_like(c["n"] * c["k"])
    r = _lib.load().tagrec_attn_pull_da_f32(inv.g.handle, _lib.ptr(inv.pair), _lib.ptr(g["dOut"]), _lib.ptr(g["Ej"]), _lib.ptr(B),
                                            _lib.ptr(dEj), _lib.ptr(da), c["D"] if D is None else D, _lib.stream_ptr())
    if rc:
        return r, (dEj, da)
    _lib.check(r, "attn_pull_da")
    return dEj, da


def _pull_dq(c, inv, comp, B=None, rc=False, A=None, v=None):
    dQ = nan_like(c["n_dst"], c["A"])
    r = _lib.load().tagrec_attn_pull_dq_f32(inv.pairs_graph().handle, _lib.ptr(comp), _lib.ptr(c["g"]["v"] if v is None else v),
                                            c["A"] if A is None else A, _lib.ptr(B), _lib.ptr(dQ), _lib.stream_ptr())
    if rc:
        return r, (dQ,)
    _lib.check(r, "attn_pull_dq")
    return dQ


def _seg_dq(dest, pair, n_dst, comp, v, A, dQ, rc=False):
    r = _lib.load().tagrec_attn_seg_dq_f32(_lib.ptr(dest), _lib.ptr(pair), dest.numel(), n_dst, _lib.ptr(comp), _lib.ptr(v), A,
                                           _lib.ptr(dQ), _lib.stream_ptr())
    if rc:
        return r
    _lib.check(r, "attn_seg_dq")
    return dQ


def _comp_host(comp, n, k):
    """(ds [n, k] float32, relu bits [n, k] as non-negative int64) of a stored comp [n k, 2]"""
    h = _np(comp).reshape(n, k, 2)
    return h[:, :, 0], h[:, :, 1].copy().view(np.int32).astype(np.int64) & 0xFFFFFFFF


# =============================================================================================================== checks
def _check_fwd(chk, tag, c, attn, out):
    k, D = c["k"], c["D"]
    f = AR.attn_fwd(c["P"], c["Q"], c["WT"], c["v"], c["Ej"], c["idx"], c["widx"])
    a, a_mag, a_extra = f["attn"]
    chk.close(tag + " attn", attn, a, a_mag, AR.c_attn(k), a_extra)                      # 17 + ceil(log2 k), the slope as extra
    o, o_mag, o_extra = f["out"]
    chk.close(tag + " out", out, o, o_mag, AR.c_out(k, D), o_extra)                      # fma chain + tree; a's error as extra
    chk.close(tag + " sum attn", f64(attn).sum(1), np.ones(c["n"]), a_mag.sum(1), AR.c_attn(k), a_extra.sum(1))
    at, ot = _np(attn), _np(out)
    _exact(chk, tag + ": out of the all-pad row == 0", (ot[3] == 0).all())
    _exact(chk, tag + ": equal logits, bit-equal weights", (at[5].view(np.int32) == at[5].view(np.int32)[0]).all())
    if k == 1:
        _exact(chk, tag + ": attn == 1 at k = 1", (at == 1.0).all())
    return f


def _check_source_side(chk, tag, c, got, r, c_ds, ds_form):
    """dP, dWT, dv of either backward kernel against the restatement `r`; c_ds: the count of ds in that kernel"""
    n, k, A = c["n"], c["k"], c["A"]
    c_dh = c_ds + 1
    chk.close(tag + " dP", got["dP"], *r["dP"], c_dh + AR.c_dp(k, A))                                # lane chain + group tree
    chk.close(tag + " dWT", got["dWT"], *r["dWT"], c_dh + AR.c_dwt(c["widx"], c["n_wt"], A, ds_form))  # block's entries (+ copies) + fold
    chk.close(tag + " dv", got["dv"], *r["dv"], c_ds + 1 + AR.c_dv(n, k, A))                        # lane chain, tree, 4 waves, fold
    if k == 1:
        _exact(chk, tag + ": dP == 0 at k = 1", (_np(got["dP"]) == 0).all())


def _check_bwd(chk, tag, c, attn, got):
    """attn_bwd (either form) from the stored attention weights"""
    k, D = c["k"], c["D"]
    r = AR.attn_bwd(c["P"], c["Q"], c["WT"], c["v"], c["Ej"], c["idx"], c["widx"], _np(attn), c["dOut"])
    c_ds = AR.c_da(D) + AR.c_ds(k)                                                        # da formed in the kernel
    _check_source_side(chk, tag, c, got, r, c_ds, False)
    if "dh" in got:
        chk.close(tag + " dh", got["dh"], *r["dh"], c_ds + 1)
        dh = _np(got["dh"])
        _exact(chk, tag + ": dh is +0 wherever h <= 0", (dh.view(np.int32)[r["h"] <= 0] == 0).all())
        _exact(chk, tag + ": dh != 0 wherever its bound excludes 0",
               (dh != 0)[np.abs(r["dh"][0]) > (c_ds + 1) * AR.U32 * r["dh"][1] + 1e-30].all())
        if k == 1:
            _exact(chk, tag + ": dh == 0 at k = 1", (dh == 0).all())
    else:
        m = AR.multiplicity(c["idx"], c["n_dst"]).astype(np.float64)[:, None]
        chk.close(tag + " dQ", got["dQ"], *r["dQ"], c_ds + 1 + m)                         # m_j atomic additions of dh
        chk.close(tag + " dEj", got["dEj"], *r["dEj"], 1 + m)                             # the product a dOut, m_j additions
        _exact(chk, tag + ": unlisted destination untouched", (_np(got["dQ"])[-1] == 0).all() and (_np(got["dEj"])[-1] == 0).all())
    return r


def _check_bwd_ds(chk, tag, c, attn, da, got):
    """attn_bwd_ds from the stored attention weights and da (a pad slot of da holds garbage)"""
    n, k, A = c["n"], c["k"], c["A"]
    r = AR.attn_bwd_ds(c["P"], c["Q"], c["WT"], c["v"], c["idx"], c["widx"], _np(attn), _np(da).reshape(n, k))
    ds, bits = _comp_host(got["comp"], n, k)
    chk.close(tag + " comp.ds", ds, *r["ds"], AR.c_ds(k))                                 # 3 + ceil(log2 k)
    _exact(chk, tag + ": relu bits of comp", np.array_equal(bits, r["bits"]))
    _check_source_side(chk, tag, c, got, r, AR.c_ds(k), True)
    if k == 1:
        _exact(chk, tag + ": ds == 0 at k = 1", (ds == 0).all())
    return r


def _check_pull_da(chk, tag, c, inv, attn, got, B=None):
    dEj, da = got
    D, b = c["D"], int(B is not None)
    (y, m), (dar, dam) = AR.attn_pull_da(c["Ej"], c["idx"], _np(attn), c["dOut"], None if B is None else _np(B))
    flat, tree = AR.pull_counts(inv.deg, 256 // D, 256 // D)
    chk.close(tag + " dEj", dEj, y, m, flat + b)                                          # pairs + chunks (+ B)
    long = inv.deg > AR.K_LONG
    if long.any():
        chk.close(tag + " dEj (long, tree depth)", f64(dEj)[long], y[long], m[long], (tree + b)[long])
    pad = c["idx"].reshape(-1) == 0
    dag = _np(da)
    _exact(chk, tag + ": da of a pad pair is not written", np.isnan(dag[pad]).all())
    chk.close(tag + " da", dag[~pad], dar.reshape(-1)[~pad], dam.reshape(-1)[~pad], AR.c_da(D))   # 4 + log2(D / 4)
    _exact(chk, tag + ": unlisted destination exactly 0 / B",
           np.array_equal(_np(dEj)[-1], np.zeros(D, np.float32) if B is None else _np(B)[-1]))


def _check_dq(chk, tag, c, inv, comp, dQ, B, seg):
    """dQ of attn_pull_dq (seg = False: B added in the epilogue) or attn_seg_dq (seg = True: B is what dQ held) from the stored comp"""
    A, n_dst, b = c["A"], c["n_dst"], int(B is not None)
    ds, bits = _comp_host(comp, c["n"], c["k"])
    y, m = AR.attn_dq_from_comp(c["idx"], ds, bits, c["v"], n_dst, None if B is None else _np(B))
    if seg:                                                                               # pairs + segments spanned + 1 (v)
        chk.close(tag + " dQ", dQ, y, m, (inv.deg + AR.seg_spans(inv.rowptr_h) + 1).astype(np.float64)[:, None])
    else:
        flat, tree = AR.pull_counts(inv.deg, 64 // A, 256 // A)
        chk.close(tag + " dQ", dQ, y, m, flat + 1 + b)                                    # pairs + chunks, v (+ B)
        long = inv.deg > AR.K_LONG
        if long.any():
            chk.close(tag + " dQ (long, tree depth)", f64(dQ)[long], y[long], m[long], (tree + 1 + b)[long])
    _exact(chk, tag + ": unlisted destination exactly 0 / B",
           np.array_equal(_np(dQ)[-1], np.zeros(A, np.float32) if B is None else _np(B)[-1]))


# ============================================================================= forward, scatter / dh backward: every shape
@pytest.mark.parametrize("A", AR.AS)
@pytest.mark.parametrize("D", AR.DS)
def test_forward_and_backward_every_shape(D, A):
    """D x A x k in {1, 2, 3, 9, 25, 63, 64} (k = 9 at A = 64 crosses the 8-deep unroll of the score loop, k = 25 at A = 32 its
    16-per-pass boundary, k = 5 -- added at D = 256 -- and k = 9 the 4-deep gather), n_wt in {1, 7}, and once with the logits
    spread to +-80."""
    chk = Chk(f"fwd / bwd D={D} A={A}")
    zeros = ones = 0
    for k in sorted(AR.KS + ((5,) if D == 256 else ())):
        for n_wt, spread in ((1, False), (7, False), (7, True)):
            c = _case(70, 40, k, D, A, n_wt, seed=1000 * k + D + A + n_wt, spread=spread)
            tag = f"k={k} n_wt={n_wt}{' spread' if spread else ''}"
            attn, out = _fwd(c)
            _check_fwd(chk, tag, c, attn, out)
            if spread:
                zeros, ones = zeros + int((attn == 0).sum()), ones + int((attn == 1).sum())
            for pull in (True, False):
                _check_bwd(chk, tag + (" dh" if pull else " scatter"), c, attn, _bwd(c, attn, pull))
    _exact(chk, "spread logits: weights underflow to exact 0, lone maxima get exact 1", zeros > 0 and ones > 0)
    _done(chk)


# ============================================================================================== attn_bwd_ds: every shape
@pytest.mark.parametrize("A", (4, 8, 16, 32))
def test_bwd_ds_every_shape(A):
    """A x k x n_wt in {1, 7, 40, 41}: 4 * 64 / A private copies of dWT while copies * n_wt * A * 4 <= 40 KiB, i.e. n_wt <= 40
    for every A (copies * A = 256), one shared copy from 41; da is NaN at every pad slot."""
    chk = Chk(f"bwd_ds A={A}")
    D = 16
    for k in AR.KS:
        for n_wt, spread in ((1, False), (7, False), (7, True), (40, False), (41, False)):
            c = _case(70, 40, k, D, A, n_wt, seed=2000 * k + A + n_wt, spread=spread)
            tag = f"k={k} n_wt={n_wt}{' spread' if spread else ''}"
            attn, _ = _fwd(c)
            da = AR.dot_da(c["Ej"], c["idx"], c["dOut"])[0].astype(np.float32)
            da[c["idx"] == 0] = np.nan
            da = dev(da)
            _check_bwd_ds(chk, tag, c, attn, da, _bwd_ds(c, attn, da))
    _done(chk)


@pytest.mark.parametrize("A", (4, 8, 16, 32))
@pytest.mark.parametrize("n_wt", (7, 41))
def test_bwd_ds_w_major_is_only_a_hint(A, n_wt):
    """w_major in {-1, the most frequent id, a rare id, n_wt, 10^9}: dWT within its bound every time; dP and comp bit-identical.
    dv is held to its bound: it goes through LDS float atomics and is not bit-reproducible."""
    chk = Chk(f"bwd_ds w_major A={A} n_wt={n_wt}")
    c = _case(300, 40, 25, 16, A, n_wt, seed=77 + A + n_wt)
    rng = np.random.default_rng(5)
    c["widx"][rng.random(c["widx"].shape) < 0.6] = 2
    c["widx"][17, 3] = 5
    c["g"]["widx"] = dev(c["widx"])
    cnt = np.bincount(c["widx"].reshape(-1), minlength=n_wt)
    major, rare = int(cnt.argmax()), int(np.where(cnt > 0, cnt, cnt.max() + 1).argmin())
    assert major == 2 and rare != major and cnt[rare] > 0
    attn, _ = _fwd(c)
    da = dev(np.where(c["idx"] > 0, AR.dot_da(c["Ej"], c["idx"], c["dOut"])[0], np.nan).astype(np.float32))
    first = None
    for wm in (-1, major, rare, n_wt, 10 ** 9):
        got = _bwd_ds(c, attn, da, w_major=wm)
        _check_bwd_ds(chk, f"w_major={wm}", c, attn, da, got)
        first = first or got
        _exact(chk, f"w_major={wm}: dP and comp bit-identical to w_major=-1",
               same_bits(got["dP"], first["dP"]) and same_bits(got["comp"], first["comp"]))
    _done(chk)


@pytest.mark.parametrize("A", (4, 32))
def test_bwd_weight_table_at_the_lds_limit(A):
    """(n_wt + 1) * A * 4 = 48 KiB is accepted by attn_bwd and attn_bwd_ds (and right); one more row is refused."""
    chk = Chk(f"LDS limit A={A}")
    n_wt = 48 * 1024 // (4 * A) - 1
    c = _case(70, 40, 3, 16, A, n_wt, seed=9 + A)
    attn, _ = _fwd(c)
    da = dev(np.where(c["idx"] > 0, AR.dot_da(c["Ej"], c["idx"], c["dOut"])[0], np.nan).astype(np.float32))
    _check_bwd(chk, "dh", c, attn, _bwd(c, attn, True))
    _check_bwd_ds(chk, "ds", c, attn, da, _bwd_ds(c, attn, da))
    big = {**c["g"], "WT": dev(np.concatenate([c["WT"], c["WT"][:1]]))}
    ws = _ws(n_wt + 1, A)
    r, o = _bwd(c, attn, True, g=big, rc=True, n_wt=n_wt + 1, ws=ws)
    _exact(chk, "attn_bwd refuses one more row", r == E_INVALID and _all_nan(o["dP"], o["dWT"], o["dv"], o["dh"]))
    r, o = _bwd_ds(c, attn, da, g=big, rc=True, n_wt=n_wt + 1, ws=ws)
    _exact(chk, "attn_bwd_ds refuses one more row", r == E_INVALID and _all_nan(o["dP"], o["dWT"], o["dv"], o["comp"]))
    _done(chk)


# ========================================================================== the pull chain, long destinations, determinism
@pytest.mark.parametrize("D,A,k", [(16, 4, 2), (32, 8, 9), (64, 16, 25), (128, 32, 3), (256, 32, 5), (64, 32, 64)])
def test_pull_chain_with_long_destinations(D, A, k):
    """n = 1117 with destinations of 1100 and 2 * 512 + 1 pairs: forward, both attn_bwd forms, then attn_pull_da (with and
    without B, dEj aliased to B as the step does it) -> attn_bwd_ds (da exactly as pull_da left it: NaN at the pads) ->
    attn_pull_dq (A in {16, 32}; with and without B) and attn_seg_dq (zero and non-zero dQ), each from its own inputs; the
    wrappers of tgcn_step give the same; two runs of the deterministic kernels agree bit for bit."""
    chk = Chk(f"pull chain D={D} A={A} k={k}")
    c = _case(AR.N_LONG, 50, k, D, A, 5, seed=D + A + k, long=True)
    g, n, n_dst = c["g"], c["n"], c["n_dst"]
    attn, out = _fwd(c)
    _check_fwd(chk, "fwd", c, attn, out)
    dh_form = _bwd(c, attn, True)
    _check_bwd(chk, "dh", c, attn, dh_form)
    _check_bwd(chk, "scatter", c, attn, _bwd(c, attn, False))
    inv = Inv(chk, c, attn)
    assert inv.deg[AR.LONG_A] == 1100 and inv.deg[AR.LONG_B] == 2 * AR.K_CHUNK + 1 and inv.deg[-1] == 0
    B, BQ = dev(np.random.default_rng(1).standard_normal((n_dst, D)).astype(np.float32)), None
    dEj, da = _pull_da(c, inv)
    _check_pull_da(chk, "pull_da", c, inv, attn, (dEj, da))
    dEjB, daB = _pull_da(c, inv, B=B)
    _check_pull_da(chk, "pull_da + B", c, inv, attn, (dEjB, daB), B)
    alias = B.clone()
    dEjA, _ = _pull_da(c, inv, B=alias, out=alias)
    _exact(chk, "pull_da: dEj aliased to B gives the same bits", same_bits(dEjA, dEjB))
    ds_form = _bwd_ds(c, attn, da, w_major=1)
    _check_bwd_ds(chk, "bwd_ds", c, attn, da, ds_form)
    comp = ds_form["comp"]
    BQ = dev(np.random.default_rng(2).standard_normal((n_dst, A)).astype(np.float32))
    dq_runs = []
    if A in (16, 32):
        for b in (None, BQ):
            dQ = _pull_dq(c, inv, comp, B=b)
            _check_dq(chk, "pull_dq" + (" + B" if b is not None else ""), c, inv, comp, dQ, b, seg=False)
            dq_runs.append((dQ, _pull_dq(c, inv, comp, B=b)))
    else:
        r, (dQ,) = _pull_dq(c, inv, comp, rc=True)
        _exact(chk, "pull_dq refuses A = 4 / 8", r == E_UNSUPPORTED and _all_nan(dQ))
    for b in (None, BQ):
        dQ0 = torch.zeros(n_dst, A, device=DEV) if b is None else b.clone()
        _check_dq(chk, "seg_dq" + (" + dQ" if b is not None else ""), c, inv, comp, _seg_dq(inv.skey, inv.pair, n_dst, comp, g["v"], A, dQ0),
                  b, seg=True)
    # the wrappers of tgcn_step: same kernels, same bits where the kernels are deterministic
    w_out, w_attn = TS.attn_fwd(g["P"], g["Q"], g["WT"], g["v"], g["Ej"], g["idx"], g["widx"])
    _exact(chk, "TS.attn_fwd: same bits", same_bits(w_out, out) and same_bits(w_attn, attn))
    w_dh = nan_like(n, k, A)
    w_dP, w_dWT, w_dv = TS.attn_bwd(g["P"], g["Q"], g["WT"], g["v"], g["Ej"], g["idx"], g["widx"], attn, g["dOut"], None, None, w_dh)
    _exact(chk, "TS.attn_bwd (dh): same bits of dP and dh", same_bits(w_dP, dh_form["dP"]) and same_bits(w_dh, dh_form["dh"]))
    _check_bwd(chk, "TS.attn_bwd", c, attn, {"dP": w_dP, "dWT": w_dWT, "dv": w_dv, "dh": w_dh})
    old = TS.SEGMENTED_DQ
    try:
        for seg in (True, False) if A in (16, 32) else (True,):
            TS.SEGMENTED_DQ = seg
            p_dP, p_dWT, p_dv, p_dQ, p_dEj = TS.attn_bwd_pulls(g["P"], g["Q"], g["WT"], g["v"], g["Ej"], g["idx"], g["widx"], attn,
                                                               g["dOut"], BQ.clone(), B, w_major=1)
            _exact(chk, f"TS.attn_bwd_pulls seg={seg}: dEj, dP same bits", same_bits(p_dEj, dEjB) and same_bits(p_dP, ds_form["dP"]))
            _check_source_side(chk, f"TS.attn_bwd_pulls seg={seg}", c, {"dP": p_dP, "dWT": p_dWT, "dv": p_dv},
                               AR.attn_bwd_ds(c["P"], c["Q"], c["WT"], c["v"], c["idx"], c["widx"], _np(attn), _np(da).reshape(n, k)),
                               AR.c_ds(k), True)
            _check_dq(chk, f"TS.attn_bwd_pulls seg={seg}", c, inv, comp, p_dQ, BQ, seg=seg)
    finally:
        TS.SEGMENTED_DQ = old
    # two runs
    attn2, out2 = _fwd(c)
    dh2, ds2 = _bwd(c, attn, True), _bwd_ds(c, attn, da, w_major=1)
    dEj2, da2 = _pull_da(c, inv)
    pad = torch.from_numpy(c["idx"].reshape(-1) == 0).to(DEV)
    _exact(chk, "two runs: attn_fwd", same_bits(attn, attn2) and same_bits(out, out2))
    _exact(chk, "two runs: dP, dh of the dh form", same_bits(dh_form["dP"], dh2["dP"]) and same_bits(dh_form["dh"], dh2["dh"]))
    _exact(chk, "two runs: dP, comp of attn_bwd_ds", same_bits(ds_form["dP"], ds2["dP"]) and same_bits(comp, ds2["comp"]))
    _exact(chk, "two runs: attn_pull_da", same_bits(dEj, dEj2) and same_bits(da.masked_fill(pad, 0), da2.masked_fill(pad, 0)))
    _exact(chk, "two runs: attn_pull_dq", all(same_bits(a, b) for a, b in dq_runs))
    _done(chk)


# ================================================================================================== attn_seg_dq: layouts
SEG_LAYOUTS = {                       # name: (pairs per listed destination in sorted order, pad entries behind them)
    "1": ((1,), 0),
    "255": ((100, 155), 0),
    "256": ((256,), 0),
    "256 + pads from the boundary": ((200, 56), 70),
    "257, a destination across two waves, pads mid-wave": ((250, 7), 30),
    "3 * 256 + 5, three whole segments": ((768, 5), 0),
    "3 * 256 + 5, a destination across four waves": ((130, 600, 43), 0),
    "two and a half segments of singletons": (tuple([1] * 640), 11),
}


@pytest.mark.parametrize("A", (4, 8, 16, 32))
def test_seg_dq_layouts(A):
    """attn_seg_dq on hand-made sorted lists: 1, 255, 256, 257 and 3 * 256 + 5 entries, a destination that straddles two waves,
    one of three whole segments, the pad tail from mid-wave and from a 256 boundary; dQ starts non-zero.  Destination ids with
    gaps: the unlisted ones keep their bits."""
    chk = Chk(f"seg_dq A={A}")
    rng = np.random.default_rng(A)
    v = (rng.standard_normal(A) * 0.5).astype(np.float32)
    for name, (mult, n_pad) in SEG_LAYOUTS.items():
        n_list = len(mult)
        ids = np.sort(rng.permutation(2 * n_list + 3)[:n_list])                           # listed destinations, with gaps
        n_dst = int(ids.max()) + 2
        dest = np.concatenate([np.repeat(ids, mult), np.full(n_pad, n_dst)]).astype(np.int32)
        n_e = len(dest)
        n_pairs = n_e + 37
        pair = rng.permutation(n_pairs)[:n_e].astype(np.int32)
        ds = (rng.standard_normal(n_pairs) * 0.5).astype(np.float32)
        bits = rng.integers(0, 2 ** A, n_pairs, dtype=np.int64)
        comp = np.stack([ds, (bits & 0xFFFFFFFF).astype(np.uint32).view(np.float32)], 1)
        dQ0 = (rng.standard_normal((n_dst, A)) * 0.5).astype(np.float32)
        got = _seg_dq(dev(dest), dev(pair), n_dst, dev(comp), dev(v), A, dev(dQ0))
        y, m = AR.dq_from_list(dest, pair, ds, bits, v, n_dst, dQ0)
        rowptr = np.searchsorted(dest, np.arange(n_dst + 1))
        cnt = np.diff(rowptr) + AR.seg_spans(rowptr) + 1                                  # pairs + segments spanned + 1 (v)
        chk.close(name, got, y, m, cnt.astype(np.float64)[:, None])
        unlisted = np.setdiff1d(np.arange(n_dst), ids)
        _exact(chk, name + ": unlisted destinations keep their bits", np.array_equal(_np(got)[unlisted], dQ0[unlisted]))
    _done(chk)


# ===================================================================================================== grid-stride loop
def test_persistent_loop_second_and_ragged_third_iteration():
    """n = 2 * 8192 + 3 (k = 3, A = 4, D = 16): the 2048 x 4 waves of the backward kernels walk a second node and three of them a
    third, attn_bwd_ds with its scalars fetched one node ahead; every row against fp64."""
    chk = Chk("grid stride n=16387")
    n = 2 * AR.ATTN_BLOCKS * AR.ATTN_WAVES + 3
    c = _case(n, 3000, 3, 16, 4, 7, seed=16387)
    assert AR.attn_blocks(n) == AR.ATTN_BLOCKS and -(-n // (AR.ATTN_BLOCKS * AR.ATTN_WAVES)) == 3
    attn, out = _fwd(c)
    _check_fwd(chk, "fwd", c, attn, out)
    _check_bwd(chk, "dh", c, attn, _bwd(c, attn, True))
    _check_bwd(chk, "scatter", c, attn, _bwd(c, attn, False))
    da = dev(np.where(c["idx"] > 0, AR.dot_da(c["Ej"], c["idx"], c["dOut"])[0], np.nan).astype(np.float32))
    _check_bwd_ds(chk, "bwd_ds", c, attn, da, _bwd_ds(c, attn, da, w_major=3))
    _done(chk)


# ====================================================================================================== integer kernels
def _nbr_gather(c, rows, pos):
    n_rows, k = len(rows), c["k"]
    out = torch.full((n_rows, k), -7, dtype=torch.int32, device=DEV)
    wout = torch.full((n_rows, k), -7, dtype=torch.int32, device=DEV)
    rows_d, pos_d = dev(rows), None if pos is None else dev(pos)          # (held: a temporary's memory is reused at once)
    _lib.check(_lib.load().tagrec_nbr_gather_i32(_lib.ptr(c["g"]["idx"]), _lib.ptr(c["g"]["widx"]), _lib.ptr(rows_d), _lib.ptr(pos_d),
                                                 n_rows, k, _lib.ptr(out), _lib.ptr(wout), _lib.stream_ptr()), "nbr_gather")
    return out, wout


def test_integer_kernels_equal_their_restatements():
    """attn_keys / attn_invert_fill (inside Inv), nbr_gather with and without `pos`, inv_filter on a static list of more than two
    4096-entry blocks with a ragged tail for half the rows, no row and every row, with and without renumbered destinations:
    equal to the restatement and to the sorted path on the gathered table, bit for bit."""
    chk = Chk("integer kernels")
    lib = _lib.load()
    c = _case(1500, 300, 7, 16, 4, 3, seed=4)
    n, k, n_dst = c["n"], c["k"], c["n_dst"]
    attn_all = dev(np.random.default_rng(1).random((n, k)).astype(np.float32))
    inv = Inv(chk, c, attn_all)
    total = inv.total
    assert total > 2 * 4096 and total % 4096 != 0
    perm32, dest32 = inv.pair[:total].contiguous(), inv.skey[:total].contiguous()
    rng = np.random.default_rng(2)
    keep = np.sort(rng.permutation(n_dst)[:200])
    pos_dst = np.zeros(n_dst + 1, np.int32)
    pos_dst[keep + 1] = np.arange(1, len(keep) + 1)
    for name, rows in (("half", np.sort(rng.permutation(n)[:n // 2])), ("none", np.arange(0)), ("all", np.arange(n))):
        rows = rows.astype(np.int64)
        for pos in (None, rng.permutation(n_dst + 1).astype(np.int32)):
            if pos is not None:
                pos[pos == 0] = pos[0]
                pos[0] = 0
            o, w = _nbr_gather(c, rows, pos)
            ro, rw = AR.nbr_gather(c["idx"], c["widx"], rows, pos)
            _exact(chk, f"nbr_gather {name} pos={pos is not None}", np.array_equal(_np(o), ro) and np.array_equal(_np(w), rw))
        pos_src = np.zeros(n + 1, np.int32)
        pos_src[rows + 1] = np.arange(1, len(rows) + 1)
        sub_attn = np.random.default_rng(3).random((max(len(rows), 1), k)).astype(np.float32)
        for pd in (None, pos_dst):
            if pd is not None:                        # destinations outside `keep` are not listed by the compact table: drop them
                sub_idx = np.where(np.isin(c["idx"][rows] - 1, keep), c["idx"][rows], 0)
                sel = np.isin(_np(dest32), keep)
                p32, d32 = perm32[torch.from_numpy(sel).to(DEV)].contiguous(), dest32[torch.from_numpy(sel).to(DEV)].contiguous()
                nd = len(keep)
            else:
                sub_idx, p32, d32, nd = c["idx"][rows], perm32, dest32, n_dst
            cap = len(rows) * k
            skey = torch.full((max(cap, 1),), -7, dtype=torch.int32, device=DEV)
            pair, src = torch.full_like(skey, -7), torch.full_like(skey, -7)
            val = nan_like(max(cap, 1))
            fw_n = lib.tagrec_inv_filter_workspace(p32.numel())
            fw = torch.full((fw_n,), -1, dtype=torch.int32, device=DEV)
            ps_d, pd_d, at_d = dev(pos_src), None if pd is None else dev(pd), dev(sub_attn)
            _lib.check(lib.tagrec_inv_filter_i32(_lib.ptr(p32), _lib.ptr(d32), p32.numel(), k, _lib.ptr(ps_d), _lib.ptr(pd_d),
                                                 _lib.ptr(at_d), nd, cap, _lib.ptr(skey), _lib.ptr(pair), _lib.ptr(src), _lib.ptr(val),
                                                 _lib.ptr(fw), fw_n, _lib.stream_ptr()), "inv_filter")
            rk, rp, rs, rv, tot = AR.inv_filter(_np(p32), _np(d32), k, pos_src, pd, sub_attn, nd, cap)
            what = f"inv_filter {name} renumbered={pd is not None}"
            _exact(chk, what + ": total", int(fw[1]) == tot)
            _exact(chk, what + ": skey", np.array_equal(_np(skey)[:cap], rk))
            _exact(chk, what + ": pair, src, val", np.array_equal(_np(pair)[:tot], rp) and np.array_equal(_np(src)[:tot], rs)
                   and np.array_equal(_np(val)[:tot].view(np.int32), rv.view(np.int32)))
            _exact(chk, what + ": nothing written behind the total",
                   (_np(pair)[tot:] == -7).all() and (_np(src)[tot:] == -7).all() and np.isnan(_np(val)[tot:]).all())
            if pd is None:                            # the sorted path on the gathered table gives the same list
                sk2, or2, _ = AR.invert(sub_idx, nd)
                p2, s2, v2 = AR.attn_invert_fill(or2, sub_attn[:len(rows)], k)
                _exact(chk, what + ": equals the sorted path", np.array_equal(rk, sk2) and np.array_equal(rp, p2[:tot])
                       and np.array_equal(rs, s2[:tot]) and np.array_equal(rv, v2[:tot]))
    _done(chk)


# ============================================================================================================= refusals
def test_refusals_leave_the_outputs_untouched():
    """Unsupported shapes, a short workspace and misaligned buffers: the error code, and every NaN-filled output still NaN.  (No
    case reads or writes out of bounds: every buffer has the size of the largest shape named.)"""
    chk = Chk("refusals")
    c = _case(70, 40, 3, 16, 4, 7, seed=3)
    g = c["g"]
    big = dict(g)                       # buffers large enough for A = 128, D = 48 ... 256, k = 65, should a refusal fail
    big.update({"P": torch.zeros(70, 128, device=DEV), "Q": torch.zeros(40, 128, device=DEV), "WT": torch.zeros(7, 128, device=DEV),
                "v": torch.zeros(128, device=DEV), "Ej": torch.zeros(40, 256, device=DEV), "dOut": torch.zeros(70, 256, device=DEV),
                "idx": torch.zeros(70, 65, dtype=torch.int32, device=DEV), "widx": torch.zeros(70, 65, dtype=torch.int32, device=DEV)})
    attn_big, da_big = torch.zeros(70, 65, device=DEV), torch.zeros(70 * 65, device=DEV)
    ws_big = (nan_like(2048 * 8 * 128), 2048 * 8 * 128)
    cb = {**c, "k": 65, "D": 256, "A": 128}                    # output sizes of the largest shape

    def refused(what, r, outs, code):
        _exact(chk, f"{what}: code {r}, wanted {code}", r == code)
        _exact(chk, f"{what}: outputs untouched", _all_nan(*outs))

    for what, kw in (("k = 0", {"k": 0}), ("k = 65", {"k": 65}), ("A = 2", {"A": 2}), ("A = 128", {"A": 128}), ("D = 48", {"D": 48})):
        r, o = _fwd(cb, g=big, rc=True, **{"k": 3, "D": 16, "A": 4, **kw})
        refused("attn_fwd " + what, r, o, E_UNSUPPORTED)
        for pull in (True, False):
            r, o = _bwd(cb, attn_big, pull, g=big, rc=True, ws=ws_big, **{"k": 3, "D": 16, "A": 4, **kw})
            refused(f"attn_bwd pull={pull} " + what, r, [o["dP"], o["dWT"], o["dv"]] + ([o["dh"]] if pull else []), E_UNSUPPORTED)
            if not pull:
                _exact(chk, "attn_bwd " + what + ": dQ, dEj untouched", not o["dQ"].any() and not o["dEj"].any())
    for what, kw in (("k = 0", {"k": 0}), ("k = 65", {"k": 65}), ("A = 2", {"A": 2}), ("A = 64", {"A": 64}), ("A = 128", {"A": 128})):
        r, o = _bwd_ds(cb, attn_big, da_big, g=big, rc=True, ws=ws_big, **{"k": 3, "A": 4, **kw})
        refused("attn_bwd_ds " + what, r, o.values(), E_INVALID)
    # a workspace one float short
    attn, _ = _fwd(c)
    da = torch.zeros(70 * 3, device=DEV)
    w_n = _lib.load().tagrec_tgcn_attn_workspace(7, 4)
    short = (nan_like(w_n - 1), w_n - 1)
    r, o = _bwd(c, attn, True, rc=True, ws=short)
    refused("attn_bwd short workspace", r, list(o.values()) + [short[0]], E_INVALID)
    r, o = _bwd_ds(c, attn, da, rc=True, ws=short)
    refused("attn_bwd_ds short workspace", r, list(o.values()) + [short[0]], E_INVALID)
    # misaligned comp (4 bytes off), Ej / out / dOut (4 bytes off)
    off = lambda t: torch.cat([t.reshape(-1)[:1], t.reshape(-1)])[1:].view(t.shape)
    comp_off = off(nan_like(70 * 3, 2))
    assert comp_off.data_ptr() % 8 == 4
    r, o = _bwd_ds(c, attn, da, rc=True, comp=comp_off)
    refused("attn_bwd_ds misaligned comp", r, o.values(), E_INVALID)
    dQ = nan_like(40, 4)
    dest, pair = torch.zeros(10, dtype=torch.int32, device=DEV), torch.arange(10, dtype=torch.int32, device=DEV)
    refused("attn_seg_dq misaligned comp", _seg_dq(dest, pair, 40, comp_off, g["v"], 4, dQ, rc=True), [dQ], E_INVALID)
    comp_ok = torch.zeros(70 * 3, 2, device=DEV)
    refused("attn_seg_dq A = 64", _seg_dq(dest, pair, 40, comp_ok, big["v"], 64, dQ, rc=True), [dQ], E_UNSUPPORTED)
    ej_off = {**g, "Ej": off(g["Ej"])}
    assert ej_off["Ej"].data_ptr() % 16 == 4
    r, o = _fwd(c, g=ej_off, rc=True)
    refused("attn_fwd misaligned Ej", r, o, E_INVALID)
    out_off = off(nan_like(70, 16))
    r, o = _fwd(c, rc=True, out=out_off)
    refused("attn_fwd misaligned out", r, o, E_INVALID)
    for name, gg in (("Ej", ej_off), ("dOut", {**g, "dOut": off(g["dOut"])})):
        r, o = _bwd(c, attn, True, g=gg, rc=True)
        refused("attn_bwd misaligned " + name, r, o.values(), E_INVALID)
    inv = Inv(chk, c, attn)
    r, o = _pull_da(c, inv, rc=True, D=48)
    refused("attn_pull_da D = 48", r, o, E_UNSUPPORTED)
    r, o = _pull_da(c, inv, g=ej_off, rc=True)
    refused("attn_pull_da misaligned Ej", r, o, E_INVALID)
    r, o = _pull_da(c, inv, rc=True, out=off(nan_like(40, 16)))
    refused("attn_pull_da misaligned dEj", r, o, E_INVALID)
    r, o = _pull_dq({**c, "A": 32}, inv, comp_ok, rc=True, A=8, v=big["v"])
    refused("attn_pull_dq A = 8", r, o, E_UNSUPPORTED)
    r, o = _pull_dq({**c, "A": 32}, inv, comp_off, rc=True, A=32, v=big["v"])
    refused("attn_pull_dq misaligned comp", r, o, E_INVALID)
    _done(chk)
