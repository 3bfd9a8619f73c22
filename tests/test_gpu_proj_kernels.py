"""GPU: every entry point of the tall-skinny products of the TGCN step (csrc/proj.hip: tall_mm, tall_mm_adam, tall_wgrad, small_mm,
row_add_at, masked_colsum) called directly, each against the plain fp64 restatement of its own operation in tests/dense_ref.py
(held to plain fp64 `@` and torch.optim.Adam, and its bounds to planted defects, by test_dense_ref_host.py).

Tolerance: the convention of test_gpu_spmm.py (spmm_ref.Chk): |got - ref64| <= c * 2^-24 * mag + extra + 1e-30, the counts `c`
those of the header of dense_ref.py, every output with its OWN magnitude.  Every output and every workspace starts as NaN (or as
the non-zero values an accumulating form adds to).  Every test prints its worst err / bound (`-s`); DESIGN section 2 carries the
table.  Every kernel here is atomic-free with a fixed-order fold: each call is run twice and must agree bit for bit."""
import pytest
import torch

pytestmark = pytest.mark.gpu

from tagrec_amd import _lib

import dense_ref as DR
from spmm_ref import Chk as _Chk, same_bits
from test_gpu_spmm import DEV, nan_like

E_INVALID = -1
LR, B1, B2, EPS = 0.01, 0.9, 0.999, 1e-8


def Chk(name):
    return _Chk(name, tag="proj")


def _close(chk, what, got, o):
    chk.close(what, got, o.ref, o.mag, o.c, extra=o.extra.cpu().numpy())


def _all_nan(*ts):
    return all(bool(torch.isnan(t).all()) for t in ts)


def _rn(gen, *shape, sc=0.1):
    return (torch.randn(*shape, generator=gen) * sc).to(DEV)


# ========================================================================================================= direct calls
def _tall(c, rc=False, **kw):
    """one tagrec_tall_mm_f32 call of a dense_ref.tall_case -> Y [n, NO] (the two outputs side by side)"""
    g = {**c, **kw}
    n, NO = c["n"], c["NO"]
    acc = c["old1"] is not None
    if c["split_out"]:
        Y1, Y2 = nan_like(n, NO // 2), nan_like(n, NO // 2)
    else:
        Y1, Y2 = (c["old1"].clone() if acc else nan_like(n, NO)), None
    W1, W2 = g["W1"], g["W2"]
    assert W2 is None or W2.stride() == W1.stride()
    r = _lib.load().tagrec_tall_mm_f32(g["X1"], g["X2"], g["sel"], g["n"], g["K"], g["NO"], W1, W2, W1.stride(0), W1.stride(1), g["w_split"],
                                       g["b1"], g["b2"], Y1, g.get("Y2", Y2), int(acc), _lib.stream_ptr())
    Y = Y1 if Y2 is None else torch.cat([Y1, Y2], dim=1)
    if rc:
        return r, Y
    _lib.check(r, "tall_mm")
    return Y


def _check_tall(chk, c):
    Y = _tall(c)
    _close(chk, f"{c['form']} n={c['n']}", Y, DR.tall_ref(c))
    assert same_bits(Y, _tall(c)), f"{chk.name}: tall_mm {c['form']} is not reproducible"


def _adam_rowops(p, grad, m, v, step):
    _lib.check(_lib.load().tagrec_adam_f32(_lib.ptr(p), _lib.ptr(grad), _lib.ptr(m), _lib.ptr(v), p.numel(), LR, B1, B2, EPS, step,
                                           _lib.stream_ptr()), "adam")


def _tall_wgrad(X, dY1, dY2, dW, db1, db2, acc_w, acc_b, rc=False, ws_floats=None, KI=None, NO=None):
    n = X.shape[0]
    KI = X.shape[1] if KI is None else KI
    NO = dY1.shape[1] * (2 if dY2 is not None else 1) if NO is None else NO
    lib = _lib.load()
    ws_n = lib.tagrec_tall_wgrad_workspace(KI, NO)
    ws = nan_like(ws_n)
    r = lib.tagrec_tall_wgrad_f32(X, dY1, dY2, n, KI, NO, dW, db1, db2, int(acc_w), int(acc_b), ws, ws_n if ws_floats is None else ws_floats,
                                  _lib.stream_ptr())
    if rc:
        return r
    _lib.check(r, "tall_wgrad")


def _colsum(dOut, out, D=None, rc=False, ws_floats=None):
    n = dOut.shape[0]
    D = dOut.shape[1] if D is None else D
    lib = _lib.load()
    ws_n = lib.tagrec_masked_colsum_workspace(D)
    ws, res = nan_like(ws_n), nan_like(dOut.shape[1])
    r = lib.tagrec_masked_colsum_f32(dOut, out, n, D, res, ws, ws_n if ws_floats is None else ws_floats, _lib.stream_ptr())
    if rc:
        return r, res
    _lib.check(r, "masked_colsum")
    return res


# ================================================================================================================ tests
@pytest.mark.parametrize("K,NO", DR.SHAPES, ids=lambda v: str(v))
def test_tall_mm_every_shape_ragged_ladder(K, NO):
    """all 16 instantiations x n in {1, 15, 16, 17, 63, 64, 65} x every form that applies to the shape (dense_ref.tall_case):
    plain; bias + accumulate; a transposed stride pair; a row-sliced W; X2 (K >= 32); Y2 + b2 (NO >= 32); w_split 1 and 2; sel"""
    chk = Chk(f"tall_mm ladder K={K} NO={NO}")
    for n in DR.TALL_LADDER:
        for i, form in enumerate(DR.TALL_FORMS):
            if DR.form_applies(form, K, NO):
                _check_tall(chk, DR.tall_case(form, n, K, NO, seed=1000 * i + 7 * K + NO + n, device=DEV))
    chk.done()


@pytest.mark.parametrize("K,NO,form", [(16, 16, "plain"), (128, 32, "sel_y2")], ids=["plain", "sel_y2"])
def test_tall_mm_second_loop_iteration(K, NO, form):
    """the grid-stride loop's second pass (1280 blocks x 4 waves x 16 rows) with a ragged last tile"""
    n = DR.TALL_LOOP2_N
    assert n > 1280 * 4 * 16 and n % 16
    chk = Chk(f"tall_mm loop2 K={K} NO={NO} {form}")
    _check_tall(chk, DR.tall_case(form, n, K, NO, seed=K + NO, device=DEV))
    chk.done()


@pytest.mark.parametrize("n", DR.ADAM_NS)
@pytest.mark.parametrize("K,NO", DR.ADAM_SHAPES, ids=lambda v: str(v))
def test_tall_mm_adam(K, NO, n):
    """p, m, v against the fp64 restatement (torch.optim.Adam's step on the fp64 gradient, the gradient's bound propagated) and,
    bit for bit, against tagrec_tall_mm_f32 into a gradient buffer followed by tagrec_adam_f32: both go through adam_update of
    csrc/common.h.  G_in NULL and given, W plain and transposed, steps 1 and 7."""
    chk = Chk(f"tall_mm_adam K={K} NO={NO} n={n}")
    i = DR.ADAM_NS.index(n) + DR.ADAM_SHAPES.index((K, NO))
    lib = _lib.load()
    for with_g, transposed, step in ((i % 2 == 0, i % 4 >= 2, 1 if i % 3 else 7), (i % 2 == 1, i % 4 < 2, 7 if i % 3 else 1)):
        gen = torch.Generator().manual_seed(100 * K + NO + n + step)
        X = _rn(gen, n, K)
        W = _rn(gen, NO, K, sc=0.3).t() if transposed else _rn(gen, K, NO, sc=0.3)
        G_in = _rn(gen, n, NO) if with_g else None
        p0 = _rn(gen, n, NO)
        m0, v0 = (torch.zeros_like(p0), torch.zeros_like(p0)) if step == 1 else (_rn(gen, n, NO, sc=0.01), _rn(gen, n, NO, sc=0.01).abs())
        p, m, v = p0.clone(), m0.clone(), v0.clone()
        _lib.check(lib.tagrec_tall_mm_adam_f32(X, n, K, NO, W, W.stride(0), W.stride(1), G_in, p, m, v, LR, B1, B2, EPS, step,
                                               _lib.stream_ptr()), "tall_mm_adam")
        r = DR.tall_mm_adam(X, W, G_in, p0, m0, v0, LR, B1, B2, EPS, step)
        tag = f"G_in={with_g} T={transposed} step={step}"
        for k, got in (("p", p), ("m", m), ("v", v)):
            _close(chk, f"{k} {tag}", got, r[k])
        assert not same_bits(p, p0)
        # the same update as a gradient buffer + the Adam kernel of rowops
        grad = G_in.clone() if with_g else nan_like(n, NO)
        _lib.check(lib.tagrec_tall_mm_f32(X, None, None, n, K, NO, W, None, W.stride(0), W.stride(1), 0, None, None, grad, None, int(with_g),
                                          _lib.stream_ptr()), "tall_mm")
        _close(chk, f"g {tag}", grad, r["g"])
        p2, m2, v2 = p0.clone(), m0.clone(), v0.clone()
        _adam_rowops(p2, grad, m2, v2, step)
        assert same_bits(m, m2) and same_bits(v, v2) and same_bits(p, p2), f"{chk.name} {tag}: not the bits of tall_mm + adam"
    chk.done()


@pytest.mark.parametrize("KI,NO", DR.TWG_SHAPES, ids=lambda v: str(v))
def test_tall_wgrad_split_edges(KI, NO):
    """n in {1, 3, 5, 63, 65, 257} (a ragged last step, one wave, a second wave) and, at 16 x 16, n = 4 (16 * 2048 + 1): spw = 17.
    A single dY into NaN-filled dW / db1, then dW += / db += on non-zero destinations -- with the split dY and db1 / db2 where
    NO >= 32"""
    chk = Chk(f"tall_wgrad KI={KI} NO={NO}")
    ns = DR.TWG_NS + ((DR.TWG_SPW17_N,) if (KI, NO) == (16, 16) else ())
    assert (KI, NO) != (16, 16) or DR.tall_wgrad_split(ns[-1])[0] == 17
    for n in ns:
        gen = torch.Generator().manual_seed(KI + NO + n)
        X, dY = _rn(gen, n, KI), _rn(gen, n, NO, sc=1.0)

        def single():
            dW, db = nan_like(KI, NO), nan_like(NO)
            _tall_wgrad(X, dY, None, dW, db, None, False, False)
            return dW, db
        dW, db = single()
        w = DR.tall_wgrad(X, dY)
        _close(chk, f"dW n={n}", dW, w["dW"])
        _close(chk, f"db n={n}", db, w["db"])
        assert all(same_bits(a, b) for a, b in zip((dW, db), single()))
        oldW, oldb = _rn(gen, KI, NO, sc=1.0), _rn(gen, NO, sc=1.0)
        split = NO >= 32
        d1, d2 = (dY[:, :NO // 2].contiguous(), dY[:, NO // 2:].contiguous()) if split else (dY, None)

        def accumulated():
            dW, db = oldW.clone(), oldb.clone()
            if split:
                b1, b2 = db[:NO // 2].clone(), db[NO // 2:].clone()
                _tall_wgrad(X, d1, d2, dW, b1, b2, True, True)
                return dW, torch.cat([b1, b2])
            _tall_wgrad(X, d1, None, dW, db, None, True, True)
            return dW, db
        dW, db = accumulated()
        w = DR.tall_wgrad(X, d1, d2, old_W=oldW, old_b=oldb)
        _close(chk, f"dW += n={n}", dW, w["dW"])
        _close(chk, f"db += n={n}", db, w["db"])
        assert all(same_bits(a, b) for a, b in zip((dW, db), accumulated()))
    chk.done()


def test_small_ops():
    """small_mm on strided views, K = 0 and K = 1 included; masked_colsum at n in {1, 7, 1025 rpp + 1} with exact 0.0 and -0.0 in
    `out` (the mask is > 0); row_add_at exact"""
    chk = Chk("small ops")
    lib = _lib.load()
    gen = torch.Generator().manual_seed(2)
    big, W = _rn(gen, 18, 20, sc=0.5), _rn(gen, 138, 32, sc=0.5)
    for K in (0, 1, 10):
        for acc in (False, True):
            A, B = big[:, ::2], W[128:]                       # A(i, k) = big[i, 2 k]: strides (20, 2)
            old = _rn(gen, 18, 32, sc=0.5)
            C = old.clone() if acc else nan_like(18, 32)
            _lib.check(lib.tagrec_small_mm_f32(A, B, C, 18, 32, K, A.stride(0), A.stride(1), B.stride(0), B.stride(1), int(acc),
                                               _lib.stream_ptr()), "small_mm")
            _close(chk, f"small_mm K={K} acc={acc}", C, DR.small_mm(A[:, :K], B[:K], old=old if acc else None))
            At = big[:, 1::2].t()                             # transposed view [10, 18]: strides (2, 20)
            Bt = old
            C = nan_like(10, 32)
            _lib.check(lib.tagrec_small_mm_f32(At, Bt, C, 10, 32, 18, At.stride(0), At.stride(1), Bt.stride(0), Bt.stride(1), 0,
                                               _lib.stream_ptr()), "small_mm")
            _close(chk, "small_mm A^T", C, DR.small_mm(At, Bt))
    for D in (16, 128):
        rpp = 256 // (D // 4)
        for n in (1, 7, 1025 * rpp + 1):
            d, o = _rn(gen, n, D, sc=1.0), _rn(gen, n, D, sc=1.0)
            o[:, 0::5] = 0.0
            o[:, 1::5] = -0.0
            res = _colsum(d, o)
            r = DR.masked_colsum(d, o)
            _close(chk, f"masked_colsum D={D} n={n}", res, r)
            assert bool((res[0::5] == 0).all()) and bool((res[1::5] == 0).all()), "0.0 and -0.0 are not > 0"
            assert same_bits(res, _colsum(d, o))
    dst = _rn(gen, 1000, 64, sc=0.5)
    pos = torch.randperm(1000, generator=gen)[:300].to(DEV)
    src = _rn(gen, 300, 64, sc=0.5)
    want = dst.clone()
    want[pos] += src
    _lib.check(lib.tagrec_row_add_at_f32(dst, pos, src, 300, 64, _lib.stream_ptr()), "row_add_at")
    assert same_bits(dst, want)
    chk.done()


# ============================================================================================================= refusals
def test_refusals():
    """bad arguments return TAGREC_E_INVALID and leave the NaN-filled outputs untouched"""
    lib = _lib.load()
    c = DR.tall_case("plain", 40, 16, 32, seed=1, device=DEV)
    half = torch.zeros(40, 8, device=DEV)
    b = torch.zeros(16, device=DEV)
    for kw in ({"X2": half},                                         # a split operand needs at least 32 columns
               {"b2": b},                                            # a second bias goes with a second output
               {"w_split": 1}, {"w_split": 2}, {"W2": c["W1"]},      # W2 goes with w_split 1 or 2, and only with them
               {"w_split": 3, "W2": c["W1"]}, {"K": 24}, {"NO": 48}, {"n": -1}):
        r, Y = _tall(c, rc=True, **kw)
        assert r == E_INVALID and _all_nan(Y), kw
    c16 = DR.tall_case("plain", 40, 32, 16, seed=1, device=DEV)
    r, Y = _tall(c16, rc=True, Y2=torch.full((40, 8), float("nan"), device=DEV))      # a split output needs at least 32 columns
    assert r == E_INVALID and _all_nan(Y)
    X, W = c["X1"], c["W1"]
    p, m, v = nan_like(40, 32), nan_like(40, 32), nan_like(40, 32)
    for step in (0, -1):
        r = lib.tagrec_tall_mm_adam_f32(X, 40, 16, 32, W, W.stride(0), W.stride(1), None, p, m, v, LR, B1, B2, EPS, step, _lib.stream_ptr())
        assert r == E_INVALID and _all_nan(p, m, v)
    dY = torch.zeros(40, 32, device=DEV)
    dW, db = nan_like(16, 32), nan_like(32)
    ws_n = lib.tagrec_tall_wgrad_workspace(16, 32)
    assert _tall_wgrad(X, dY, None, dW, db, None, False, False, rc=True, ws_floats=ws_n - 1) == E_INVALID
    assert _tall_wgrad(X, dY, None, dW, None, db, False, False, rc=True) == E_INVALID            # db2 without a second dY
    assert _tall_wgrad(X, dY, None, dW, db, None, False, False, rc=True, KI=24) == E_INVALID
    d16 = torch.zeros(40, 8, device=DEV)
    assert _tall_wgrad(X, d16, d16, nan_like(16, 16), db, db, False, False, rc=True) == E_INVALID  # a split dY needs 32 columns
    assert _all_nan(dW, db)
    C = nan_like(8)
    r = lib.tagrec_small_mm_f32(X, W, C, 2049, 2048, 1, 0, 0, 0, 0, 0, _lib.stream_ptr())          # past 2^22 elements
    assert r == E_INVALID and _all_nan(C)
    d24 = torch.zeros(40, 24, device=DEV)
    r, res = _colsum(d24, d24, rc=True)                                                              # D / 4 = 6 does not divide 256
    assert r == E_INVALID and _all_nan(res)
    r, res = _colsum(dY, dY, rc=True, ws_floats=lib.tagrec_masked_colsum_workspace(32) - 1)
    assert r == E_INVALID and _all_nan(res)
    torch.cuda.synchronize()
