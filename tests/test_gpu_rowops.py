"""GPU: the kernels of csrc/rowops.hip, each against a plain restatement of its own operation -- torch / numpy fp64 on the
CPU for the float kernels, numpy uint64 and Python integers for the two counter-based generators.

Tolerance.  A float result is accepted iff

    |got - ref64| <= c * 2^-24 * mag + extra + 1e-30

`mag` is the fp64 sum of the absolute values of the terms that form the output (the magnitude of the result for a ratio),
`c` the number of rounded fp32 operations on the longest path to it, read off the kernel and written beside each check: a
D-term dot counts D whatever order it is summed in, an atomic scatter adds the row's multiplicity in the batch, and a result
of expf / log1pf carries 4 ulp = 8 * 2^-24 of its value.  `extra` is only used where an error enters through a function's
slope instead of a term (the score gap under the sigmoid, a distance under 1 / distance) and is itself such a count.  Each
test prints its worst err / bound ratio (`-s`); the table in DESIGN section 2 is filled from them.  Integer, flag and mask
outputs are compared exactly.  Operands are drawn at embedding scale (0.1 * randn) unless the case says otherwise."""
import ctypes

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import tagrec_amd as T
from tagrec_amd import _lib, help as H, rowops, train_data
from tagrec_amd.dist import HipOps
from tagrec_amd.rowops import VEC_WIDTHS

from spmm_ref import U32, Chk, f64 as _f64, norm_rows as _norm_rows, np_drop, randn as _randn, ref_norm_bwd as _ref_norm_bwd, \
    same_bits as _same_bits

DEV = torch.device("cuda:0")
OPS = HipOps()
SCALAR_WIDTHS = (4, 12, 48, 100, 260)  # below a wave .. more than one trip of the scalar kernels' lane loop
WIDTHS = VEC_WIDTHS + SCALAR_WIDTHS
ROW_COUNTS = (1, 127, 129, 1031)       # around the vector kernel's rows per block (128 at D = 8, 4 at D = 256)
S = float(np.float32(1.0 / 3.0))       # a scale that is exact as the float the ABI takes


# ====================================================================================================== row normalise
def test_fp64_normalize_backward_formula_is_torch_autograd():
    """The reference of the backward tests (above) is F.normalize's autograd in fp64, clamped rows included."""
    x, dz, clamped = _norm_rows(64, 12, seed=3)
    xr = x.double().requires_grad_()
    (torch.nn.functional.normalize(xr, p=2, dim=1) * (S * dz.double())).sum().backward()
    inv = 1.0 / torch.clamp(x.double().norm(dim=1), min=1e-12)
    ref = _ref_norm_bwd(x, inv, dz, S, clamped)[0]
    np.testing.assert_allclose(ref, xr.grad.numpy(), rtol=1e-12, atol=0)


@pytest.mark.parametrize("n", ROW_COUNTS)
@pytest.mark.parametrize("D", WIDTHS)
def test_rownorm_fwd(D, n):
    chk = Chk(f"rownorm_fwd D={D} n={n}")
    x, _, _ = _norm_rows(n, D, seed=D + n)
    den = np.maximum(np.linalg.norm(_f64(x), axis=1), 1e-12)
    z_ref, inv_ref = _f64(x) / den[:, None], 1.0 / den
    z, inv = rowops.rownorm_fwd(x.to(DEV))
    # c = D + 3: D fmas of the sum of squares (halved by the square root), sqrtf, the float eps constant, the divide
    chk.close("z", z, z_ref, np.abs(z_ref), D + 3)
    chk.close("inv", inv, inv_ref, inv_ref, D + 3)
    # a slot of a wider buffer (ldz > D): the other columns are not written
    wide = torch.full((n, D + 5), float("nan"), device=DEV)
    z2, inv2 = rowops.rownorm_fwd(x.to(DEV), z=wide[:, 2:2 + D])
    assert _same_bits(z2, z) and _same_bits(inv2, inv)
    assert torch.isnan(wide[:, :2]).all() and torch.isnan(wide[:, 2 + D:]).all()
    chk.done()


@pytest.mark.parametrize("n", ROW_COUNTS)
@pytest.mark.parametrize("D", WIDTHS)
def test_rownorm_bwd_and_flags(D, n):
    chk = Chk(f"rownorm_bwd D={D} n={n}")
    x, dz, clamped = _norm_rows(n, D, seed=7 * D + n)
    xg, dzg = x.to(DEV), dz.to(DEV)
    _, inv = rowops.rownorm_fwd(xg)
    ref, mag, _, _ = _ref_norm_bwd(x, inv, dz, S, clamped)
    out = rowops.rownorm_bwd(xg, inv, dzg, S, torch.full((n, D), float("nan"), device=DEV))
    # c = D + 6, the path through the dot: D fmas over terms of two rounded products (x inv, dz s: + 2), then x inv,
    # (.) dot, the subtraction and the product with inv
    chk.close("dx", out, ref, mag, D + 6)
    zero_dz = (dz == 0).all(1)
    assert (out[zero_dz.to(DEV)] == 0).all()                        # exact zeros, -0.0 in dz included
    # dz as a slot of a wider buffer (lddz > D; 16-byte aligned, so the vector widths stay on the vector kernel) and as a
    # misaligned slot (every width on the scalar kernel)
    for off, pad in ((4, 4), (1, 2)):
        wide = torch.full((n, off + D + pad), float("nan"), device=DEV)
        wide[:, off:off + D] = dzg
        o2 = rowops.rownorm_bwd(xg, inv, wide[:, off:off + D], S, torch.full((n, D), float("nan"), device=DEV))
        chk.close(f"dx(lddz={off + D + pad})", o2, ref, mag, D + 6)
        if off == 4:
            assert _same_bits(o2, out)
    # the flag-writing form: same bits, flags = rows of out with a non-zero, count = their number
    o3 = torch.full((n, D), float("nan"), device=DEV)
    flags, count = rowops.rownorm_bwd_flags(xg, inv, dzg, S, o3)
    assert _same_bits(o3, out)
    want = (out != 0).any(1)
    assert torch.equal(flags.bool(), want) and int(count) == int(want.sum())
    assert not flags.bool()[zero_dz.to(DEV)].any()
    chk.done()


@pytest.mark.parametrize("D", [64, 48])
def test_rownorm_bwd_accumulate(D):
    """accumulate=True adds to `out` (at a vector width too: the vector kernel does not accumulate, the scalar one runs)."""
    n = 129
    chk = Chk(f"rownorm_bwd accumulate D={D}")
    x, dz, clamped = _norm_rows(n, D, seed=11 + D)
    old = _randn(n, D, seed=12 + D)
    _, inv = rowops.rownorm_fwd(x.to(DEV))
    ref, mag, _, _ = _ref_norm_bwd(x, inv, dz, S, clamped)
    out = rowops.rownorm_bwd(x.to(DEV), inv, dz.to(DEV), S, old.to(DEV), accumulate=True)
    chk.close("dx", out, ref + _f64(old), mag + np.abs(_f64(old)), D + 7)        # D + 6 and the addition to `out`
    chk.done()


def _sharded_forms(chk, x, dz, clamped, D):
    """row_dot, rownorm_bwd_dot and row_scale_acc on one operand set (inv and dot are inputs of the last two)."""
    n = x.shape[0]
    xg, dzg = x.to(DEV), dz.to(DEV)
    _, inv = rowops.rownorm_fwd(xg)
    inv64 = _f64(inv)
    got = torch.full((n,), float("nan"), device=DEV)
    OPS.row_dot(xg, inv, dzg, S, got)
    terms = _f64(x) * _f64(dz)
    # c = D + 2: D fmas, then inv * s and (.) * d
    chk.close("row_dot", got, inv64 * S * terms.sum(1), np.abs(inv64 * S) * np.abs(terms).sum(1), D + 2)
    dot = _randn(n, seed=n + D)
    dx = torch.full((n, D), float("nan"), device=DEV)
    OPS.rownorm_bwd_dot(xg, inv, dzg, dot.to(DEV), S, dx)
    dt = np.where(clamped, 0.0, _f64(dot))[:, None]
    sdz, xi = S * _f64(dz), _f64(x) * inv64[:, None]
    # c = 4: X iv, (.) dt, the subtraction, the product with iv
    chk.close("rownorm_bwd_dot", dx, inv64[:, None] * (sdz - xi * dt), np.abs(inv64)[:, None] * (np.abs(sdz) + np.abs(xi * dt)), 4)
    y, acc = _randn(n, D, seed=n + D + 1), _randn(n, D, seed=n + D + 2)
    inv_n = (_randn(n, seed=n + D + 3).abs() + 0.5).to(DEV)         # ordinary inverse norms (the clamped 1e12 is row_dot's case)
    accg = acc.to(DEV)
    OPS.row_scale_acc(y.to(DEV), inv_n, S, accg)
    t = S * _f64(inv_n)[:, None] * _f64(y)
    chk.close("row_scale_acc", accg, _f64(acc) + t, np.abs(_f64(acc)) + np.abs(t), 2)       # c = 2: s * inv, one fma


@pytest.mark.parametrize("n", ROW_COUNTS)
@pytest.mark.parametrize("D", WIDTHS)
def test_column_sharded_row_forms(D, n):
    chk = Chk(f"row_dot / rownorm_bwd_dot / row_scale_acc D={D} n={n}")
    _sharded_forms(chk, *_norm_rows(n, D, seed=13 * D + n), D)
    chk.done()


def test_column_sharded_row_forms_grid_stride():
    """16 400 x 64 elements: one block more than the 4096-block cap of row_scale_acc / rownorm_bwd_dot."""
    chk = Chk("row forms, grid-stride loop (16400 x 64)")
    _sharded_forms(chk, *_norm_rows(16400, 64, seed=5), 64)
    chk.done()


# ================================================================================================================= BPR
def _softplus64(x):
    return np.where(x > 20.0, x, np.log1p(np.exp(np.minimum(x, 20.0))))


def _neg_logsigmoid64(y):
    return -(np.minimum(y, 0.0) - np.log1p(np.exp(-np.abs(y))))


def _sigmoid64(x):
    with np.errstate(over="ignore"):
        return 1.0 / (1.0 + np.exp(-x))


def _slots(n_rows, D, pad, seed, scale=0.1):
    """A [n_rows, D] table as the first D columns of a NaN-filled [n_rows, D + pad] buffer (row stride D + pad)."""
    buf = torch.full((n_rows, D + pad), float("nan"))
    buf[:, :D] = _randn(n_rows, D, seed=seed, scale=scale)
    return buf.to(DEV)


def _triplets(B, nu, ni, seed):
    """Random triplets; from 41 on, user 7 in the first 40; item 3 positive of triplet 1 and negative of triplet 2;
    triplet 0 has pos == neg (whenever B allows)."""
    g = torch.Generator().manual_seed(seed)
    t = torch.stack([torch.randint(0, nu, (B,), generator=g), torch.randint(0, ni, (B,), generator=g),
                     torch.randint(0, ni, (B,), generator=g)], 1)
    if B >= 41:
        t[:40, 0] = 7
    if B >= 3:
        t[1, 1], t[2, 2] = 3, 3
    if B >= 2:
        t[0, 2] = t[0, 1]
    return t


def _bpr_fwd_check(chk, U, I, Ur, Ir, trip, kind, res, coef):
    """Loss parts and the per-triplet sigmoid coefficient against fp64.  -> fp64 score gaps."""
    B, D = trip.shape[0], U.shape[1]
    t = trip.numpy()
    u, p, n = _f64(U)[t[:, 0]], _f64(I)[t[:, 1]], _f64(I)[t[:, 2]]
    x = (u * n).sum(1) - (u * p).sum(1)
    # error of the gap: two D-term dots and the subtraction, c = D + 1 on the sum of |terms|
    dx = (D + 1) * U32 * (np.abs(u * n).sum(1) + np.abs(u * p).sum(1))
    soft = kind == _lib.LOSS_SOFTPLUS
    f = _softplus64(x) if soft else _neg_logsigmoid64(-x)
    sig = _sigmoid64(x)
    c_ref = np.where(x > 20.0, 1.0, sig) if soft else sig
    # coef = 1 / (1 + expf(-x)): c = 2 (add, divide) on coef; the gap's error and expf's 4 ulp enter through the slope
    # d coef / d x = coef (1 - coef)
    chk.close("coef", coef, c_ref, c_ref, 2, extra=sig * (1 - sig) * (dx + 8 * U32))
    # per triplet: expf and log1pf, 4 ulp each, and the last subtraction of the logsigmoid form: 17 on f; the gap's error
    # through the slope sigmoid(x) <= 1.  Then 3 additions in the block partial, the float 1 / B and the cast: c = 22
    chk.close("loss", res[0], f.mean(), f.mean(), 22, extra=(sig * dx).mean())
    if Ur is None:
        assert float(res[1]) == 0.0
    else:
        Dr = Ur.shape[1]
        ss = 0.5 * ((_f64(Ur)[t[:, 0]] ** 2).sum(1) + (_f64(Ir)[t[:, 1]] ** 2).sum(1) + (_f64(Ir)[t[:, 2]] ** 2).sum(1))
        # c = 3 Dreg + 5: 3 Dreg fmas, the same 3 + 2 of the two-stage sum (0.5 * is exact)
        chk.close("reg", res[1], ss.mean(), ss.mean(), 3 * Dr + 5)
    assert coef.shape == (B,)
    return x


def _scatter64(n_rows, D, idx, terms):
    """(sum, sum of |.|, multiplicity) of the rows `terms` [k, D] scattered to rows `idx` of an [n_rows, D] buffer."""
    out, mag, mult = np.zeros((n_rows, D)), np.zeros((n_rows, D)), np.zeros((n_rows, 1))
    np.add.at(out, idx, terms)
    np.add.at(mag, idx, np.abs(terms))
    np.add.at(mult, idx, 1.0)
    return out, mag, mult


def _bpr_bwd_ref(U, I, Ur, Ir, trip, coef, g, main=True):
    """fp64 gradients of g0 * mean(loss) + g1 * reg from the kernel's own inputs (the coefficient included).
    -> {"U": (sum, mag, mult), "I": ..., "Ur": ..., "Ir": ...}; mag takes |nv| + |pv| for the difference nv - pv."""
    t = trip.numpy()
    B = t.shape[0]
    g0, g1 = (1.0, 1.0) if g is None else (float(np.float32(g[0])), float(np.float32(g[1])))
    out = {}
    if main:
        u, p, n = _f64(U)[t[:, 0]], _f64(I)[t[:, 1]], _f64(I)[t[:, 2]]
        c = (g0 * _f64(coef) / B)[:, None]
        su, mu, ku = _scatter64(U.shape[0], U.shape[1], t[:, 0], c * (n - p))
        _, mu2, _ = _scatter64(U.shape[0], U.shape[1], t[:, 0], np.abs(c) * (np.abs(n) + np.abs(p)))
        out["U"] = (su, mu2, ku)
        out["I"] = _scatter64(I.shape[0], I.shape[1], np.concatenate([t[:, 1], t[:, 2]]), np.concatenate([-c * u, c * u]))
    if Ur is not None:
        cr = g1 / B
        out["Ur"] = _scatter64(Ur.shape[0], Ur.shape[1], t[:, 0], cr * _f64(Ur)[t[:, 0]])
        out["Ir"] = _scatter64(Ir.shape[0], Ir.shape[1], np.concatenate([t[:, 1], t[:, 2]]),
                               cr * np.concatenate([_f64(Ir)[t[:, 1]], _f64(Ir)[t[:, 2]]]))
    return out


def _grad_slots(buf, D):
    """Zeroed gradient slots laid out as the table slots of `buf` (same shape and row stride), NaN everywhere else."""
    d = torch.full_like(buf, float("nan"))
    d[:, :D] = 0
    return d


# c of the scatters, + one per atomic addition into the element (its multiplicity).  User rows: g0 * coef * (1 / B) is 3
# roundings (the float 1 / B included), the difference nv - pv, the product: 5.  Item rows: no difference: 4.  L2 part:
# g1 * (1 / B) is 2 (reg = 1 is exact), the product with the row: 3.
C_BPR = {"U": 5, "I": 4, "Ur": 3, "Ir": 3}


def _run_bpr(chk, D, B, kind, mode, g, seed):
    """mode: 'distinct' reg tables of another width and row stride, 'none', 'same' (reg tables are U / I and share their
    gradient buffers), 'regonly' (dU = dI = None).  Tables are slots of wider NaN-padded buffers: ld = D + 8."""
    nu, ni = 50, 60
    W = _slots(nu + ni, D, 8, seed)
    U, I = W[:nu, :D], W[nu:, :D]
    assert U.stride(0) == D + 8 and I.stride(0) == D + 8
    Dr = D + 3
    R = _slots(nu + ni, Dr, 4, seed + 1)
    Ur, Ir = (R[:nu, :Dr], R[nu:, :Dr]) if mode in ("distinct", "regonly") else (U, I) if mode == "same" else (None, None)
    trip = _triplets(B, nu, ni, seed + 2)
    tg = trip.to(DEV)
    res, coef = rowops.bpr_fwd(U, I, Ur, Ir, tg, kind)
    _bpr_fwd_check(chk, U, I, Ur, Ir, trip, kind, res, coef)
    gg = None if g is None else torch.tensor(g, dtype=torch.float32, device=DEV)
    dW, dR = _grad_slots(W, D), _grad_slots(R, Dr)
    dU, dI = (None, None) if mode == "regonly" else (dW[:nu, :D], dW[nu:, :D])
    dUr, dIr = {"distinct": (dR[:nu, :Dr], dR[nu:, :Dr]), "regonly": (dR[:nu, :Dr], dR[nu:, :Dr]), "same": (dU, dI),
                "none": (None, None)}[mode]
    rowops.bpr_bwd(U, I, Ur, Ir, tg, coef, gg, dU, dI, dUr, dIr)
    ref = _bpr_bwd_ref(U, I, Ur, Ir, trip, coef, g, main=mode != "regonly")
    g1 = 1.0 if g is None else g[1]
    if mode == "same":                                               # both parts land in one buffer
        for k, kr, got in (("U", "Ur", dU), ("I", "Ir", dI)):
            s, m, mult = (ref[k][i] + (ref[kr][i] if g1 != 0 else 0) for i in range(3))
            chk.close("d" + k, got, s, m, C_BPR[k] + mult)
    else:
        for k, got in (("U", dU), ("I", dI), ("Ur", dUr), ("Ir", dIr)):
            if got is None:
                continue
            s, m, mult = ref[k] if (k[-1] != "r" or g1 != 0) else (np.zeros_like(ref[k][0]),) * 3
            chk.close("d" + k, got, s, m, C_BPR[k] + mult)
    # nothing else written: the padding columns of the gradient buffers, and all of an unused buffer, are still NaN
    assert torch.isnan(dW[:, D:]).all() and torch.isnan(dR[:, Dr:]).all()
    if mode == "regonly":
        assert (dW[:, :D] == 0).all()
    if mode in ("none", "same"):
        assert (dR[:, :Dr] == 0).all()
    assert torch.isnan(W[:, D:]).all() and torch.isnan(R[:, Dr:]).all()


@pytest.mark.parametrize("kind", [_lib.LOSS_SOFTPLUS, _lib.LOSS_LOGSIGMOID])
@pytest.mark.parametrize("B", [1, 5, 64, 257])
@pytest.mark.parametrize("D", [4, 48, 64, 200])
def test_bpr_strided_tables_distinct_reg(D, B, kind):
    chk = Chk(f"bpr D={D} B={B} kind={kind}")
    _run_bpr(chk, D, B, kind, "distinct", [0.37, -2.0], seed=D + B)
    chk.done()


@pytest.mark.parametrize("g", [[0.37, -2.0], [1.0, 0.0], None])
@pytest.mark.parametrize("mode", ["none", "same", "regonly", "distinct"])
@pytest.mark.parametrize("D,B", [(48, 257), (200, 5), (4, 64), (64, 1)])
def test_bpr_reg_modes_and_upstream_gradients(D, B, mode, g):
    chk = Chk(f"bpr D={D} B={B} mode={mode} g={g}")
    _run_bpr(chk, D, B, _lib.LOSS_SOFTPLUS if D != 200 else _lib.LOSS_LOGSIGMOID, mode, g, seed=3 * D + B)
    chk.done()


def test_bpr_same_buffers_one_addition_per_slot():
    """mode 'same' (the L2 part on the main tables, into the main gradient buffers: the models that regularise the propagated
    rows): a slot adds its main and its L2 term as ONE value, so a row that two triplets name is a sum of two atomics -- the
    same bits in either order.  Every user is named by triplets b and b + 128 (different blocks), every item as the positive
    of one triplet and the negative of another; 25 runs must agree bit for bit, and the first is held to the fp64 gradients."""
    chk = Chk("bpr same buffers, rows named twice")
    B, nu, ni, D = 256, 128, 256, 64
    W = _slots(nu + ni, D, 8, seed=5)
    U, I = W[:nu, :D], W[nu:, :D]
    b = torch.arange(B)
    trip = torch.stack([b % nu, b, (b + 37) % ni], 1)
    tg = trip.to(DEV)
    res, coef = rowops.bpr_fwd(U, I, U, I, tg, _lib.LOSS_SOFTPLUS)
    g = [0.37, -2.0]
    gg = torch.tensor(g, dtype=torch.float32, device=DEV)
    runs = []
    for _ in range(25):
        dW = _grad_slots(W, D)
        rowops.bpr_bwd(U, I, U, I, tg, coef, gg, dW[:nu, :D], dW[nu:, :D], dW[:nu, :D], dW[nu:, :D])
        runs.append(dW)
    ref = _bpr_bwd_ref(U, I, U, I, trip, coef, g)
    for k, kr, got in (("U", "Ur", runs[0][:nu, :D]), ("I", "Ir", runs[0][nu:, :D])):
        s, m, mult = (ref[k][i] + ref[kr][i] for i in range(3))
        assert (mult == 4).all()                                     # two slots, a main and an L2 term each
        chk.close("d" + k, got, s, m, C_BPR[k] + mult)
    assert all(_same_bits(runs[0][:, :D], r[:, :D]) for r in runs[1:]), "a row named by two triplets changed from run to run"
    chk.done()


# the issue's gaps, and two between 10 and 20 where softplus still differs from x by more than fp32 resolves
GAPS = (-100.0, -20.5, -1e-4, 0.0, 10.5, 15.0, 19.99, 20.0, 20.01, 100.0)


@pytest.mark.parametrize("kind", [_lib.LOSS_SOFTPLUS, _lib.LOSS_LOGSIGMOID])
def test_bpr_forced_score_gaps(kind):
    """x = neg - pos forced exactly: the user row is 2 e_0, the positive row zero, the negative row (x / 2) e_0 (a row of
    unit score scaled to the gap).  Each gap alone (B = 1: the loss IS that triplet's) and all in one batch."""
    chk = Chk(f"bpr forced gaps kind={kind}")
    D = 4
    xs = np.float32(GAPS)
    U = torch.zeros(1, D)
    U[0, 0] = 2.0
    I = torch.zeros(1 + len(xs), D)
    I[1:, 0] = torch.from_numpy(xs) / 2
    Ug, Ig = U.to(DEV), I.to(DEV)
    allt = torch.tensor([[0, 0, 1 + j] for j in range(len(xs))])
    for trip in [allt[j:j + 1] for j in range(len(xs))] + [allt]:
        res, coef = rowops.bpr_fwd(Ug, Ig, None, None, trip.to(DEV), kind)
        x = _bpr_fwd_check(chk, U, I, None, None, trip, kind, res, coef)
        assert np.array_equal(x, xs.astype(np.float64)[trip[:, 2].numpy() - 1])
    chk.done()


@pytest.mark.parametrize("D", [48, 64])
def test_bpr_dots_column_halves(D):
    chk = Chk(f"bpr_dots D={D}")
    nu, ni, B = 50, 60, 257
    U, I = _randn(nu, D, seed=D).to(DEV), _randn(ni, D, seed=D + 1).to(DEV)
    trip = _triplets(B, nu, ni, D + 2)
    tg = trip.to(DEV)
    t = trip.numpy()

    def ref(Uc, Ic):
        u, p, n = _f64(Uc)[t[:, 0]], _f64(Ic)[t[:, 1]], _f64(Ic)[t[:, 2]]
        val = np.stack([(u * p).sum(1), (u * n).sum(1), 0.5 * (u * u + p * p + n * n).sum(1)], 1)
        mag = np.stack([np.abs(u * p).sum(1), np.abs(u * n).sum(1), val[:, 2]], 1)
        return val, mag

    h = D // 2 + 2                                                    # unequal halves; column slices: ld = D > width
    full = rowops.bpr_dots(U, I, U, I, tg)
    halves = [rowops.bpr_dots(U[:, a:b], I[:, a:b], U[:, a:b], I[:, a:b], tg) for a, b in ((0, h), (h, D))]
    for nm, got, (a, b) in (("full", full, (0, D)), ("left", halves[0], (0, h)), ("right", halves[1], (h, D))):
        val, mag = ref(U[:, a:b], I[:, a:b])
        chk.close(nm, got, val, mag, 3 * (b - a) + 1)               # at most 3 width fmas (the squares), 0.5 * exact: + 1 spare
    val, mag = ref(U, I)
    chk.close("left + right", halves[0].double() + halves[1].double(), val, mag, 3 * D + 1)
    assert float(rowops.bpr_dots(U, I, None, None, tg)[:, 2].abs().max()) == 0.0
    chk.done()


def test_bpr_refuses_bad_arguments():
    nu, ni, D = 6, 7, 8
    U, I = _randn(nu, D, seed=1).to(DEV), _randn(ni, D, seed=2).to(DEV)
    trip = _triplets(5, nu, ni, 3).to(DEV)
    res, coef = rowops.bpr_fwd(U, I, None, None, trip, _lib.LOSS_SOFTPLUS)
    g = torch.ones(2, device=DEV)
    with pytest.raises(_lib.TagrecError):
        rowops.bpr_fwd(U, I, None, None, trip[:0], _lib.LOSS_SOFTPLUS)                  # B = 0
    with pytest.raises(_lib.TagrecError):
        rowops.bpr_fwd(U, I, None, None, trip, 7)                                       # unknown loss kind
    wide = _randn(ni, 2 * D, seed=4).to(DEV)
    Iw, In = wide[:, :D], _randn(ni, D + 4, seed=5).to(DEV)
    bad = {"row stride of I": (U, Iw, None, None), "width of I": (U, In, None, None),
           "row stride of Ireg": (U, I, U, Iw), "width of Ireg": (U, I, U, In),
           "inner stride of I": (U[:, ::2], wide[:, ::2][:, :D // 2], None, None), "Ireg missing": (U, I, U, None)}
    for a, b, c, d in bad.values():
        for fn in (lambda: rowops.bpr_fwd(a, b, c, d, trip, _lib.LOSS_SOFTPLUS), lambda: rowops.bpr_dots(a, b, c, d, trip),
                   lambda: rowops.bpr_bwd(a, b, c, d, trip, coef, g, torch.zeros_like(a), torch.zeros_like(b),
                                          None if c is None else torch.zeros_like(c), None if d is None else torch.zeros_like(d))):
            with pytest.raises(_lib.TagrecError):
                fn()
    # gradient buffers that do not share their operand's row stride: a column slice of a wider table and the contiguous
    # buffer zeros_like makes for it.  Refused before any launch (the scatter would index it with the operand's stride).
    Us, Is = wide[:nu, :D], wide[:ni, D:]
    assert Us.stride(0) == 2 * D and torch.zeros_like(Us).stride(0) == D
    for args in ((Us, Is, None, None, torch.zeros_like(Us), torch.zeros_like(Is), None, None),
                 (U, I, Us, Is, torch.zeros_like(U), torch.zeros_like(I), torch.zeros_like(Us), torch.zeros_like(Is)),
                 (U, I, Us, Is, None, None, torch.zeros_like(Us), torch.zeros_like(Is))):
        with pytest.raises(_lib.TagrecError):
            rowops.bpr_bwd(*args[:4], trip, coef, g, *args[4:])
    # the autograd operator refuses a strided reg table outright (its backward would allocate such a buffer)
    with pytest.raises(_lib.TagrecError):
        H.triplet_loss(U.clone().requires_grad_(), I, Us, Is, trip, "softplus")
    torch.cuda.synchronize()


# ============================================================================================================ TransTag
def _transtag_tables(D, seed):
    """20 users, 15 tags, 30 items.  item 0 = user 0 + tag 0 exactly (entries on a 2^-12 grid: the sum is exact in fp32),
    item 1 far away (quads with it as the negative are dead at margin 1), item 2 close to item 0 (the quad (0, 0, 0, 2) is live at
    margin 1 with ps = 0)."""
    Eu, Et, Ei = _randn(20, D, seed=seed), _randn(15, D, seed=seed + 1), _randn(30, D, seed=seed + 2)
    Eu[0], Et[0] = torch.round(Eu[0] * 4096) / 4096, torch.round(Et[0] * 4096) / 4096
    Ei[0] = Eu[0] + Et[0]
    Ei[1] = _randn(D, seed=seed + 3, scale=10.0)
    Ei[2] = Ei[0] + _randn(D, seed=seed + 4, scale=0.01)
    return Eu, Ei, Et


def _quads(B, seed):
    g = torch.Generator().manual_seed(seed)
    q = torch.stack([torch.randint(0, 20, (B,), generator=g), torch.randint(0, 15, (B,), generator=g),
                     torch.randint(2, 30, (B,), generator=g), torch.randint(2, 30, (B,), generator=g)], 1)
    q[0] = torch.tensor([0, 0, 0, 2])                 # u + t == p: ps = 0
    if B >= 7:
        q[1] = torch.tensor([3, 4, 6, 6])             # p == n
        q[2] = torch.tensor([3, 4, 7, 1])             # far negative: dead
        q[3] = torch.tensor([0, 0, 8, 1])             # dead; repeats user 0 / tag 0
        q[4] = torch.tensor([3, 2, 1, 9])             # far positive: live
        q[5] = torch.tensor([5, 4, 6, 7])             # item 6, 7 again
    return q


@pytest.mark.parametrize("margin", [0.0, 1.0])
@pytest.mark.parametrize("B", [1, 7, 130])
@pytest.mark.parametrize("D", [16, 128, 100])
def test_transtag_batch_loss(D, B, margin):
    chk = Chk(f"transtag D={D} B={B} margin={margin}")
    Eu, Ei, Et = _transtag_tables(D, seed=D + B)
    quad = _quads(B, seed=D + B + 9)
    g = [0.37, -2.0]
    # reference: torch fp64 autograd of the operator form (transtag_loss + l2reg_loss)
    ru, ri, rt = (t.double().requires_grad_() for t in (Eu, Ei, Et))
    u, t, p, n = ru[quad[:, 0]], rt[quad[:, 1]], ri[quad[:, 2]], ri[quad[:, 3]]
    ps, ns = torch.norm(u + t - p, p=2, dim=1), torch.norm(u + t - n, p=2, dim=1)
    loss = torch.relu(margin + ps - ns).mean()
    reg = 0.5 * (u.norm(2).pow(2) + t.norm(2).pow(2) + p.norm(2).pow(2) + n.norm(2).pow(2)) / B
    (g[0] * loss + g[1] * reg).backward()
    gap = (margin + ps - ns).detach().numpy()
    assert float(ps[0].detach()) == 0.0 and (gap[0] > 0) == (margin > 0) and (B < 7 or (gap[1:] < 0).any())
    gu, gi, gt = (x.to(DEV).requires_grad_() for x in (Eu, Ei, Et))
    got_loss, got_reg = H.transtag_batch_loss(gu, gi, gt, quad.to(DEV), margin)
    (got_loss * g[0] + got_reg * g[1]).backward()

    u, t, p, n = (_f64(x) for x in (u, t, p, n))
    ps, ns = _f64(ps), _f64(ns)
    ap, an = np.abs(u) + np.abs(t) + np.abs(p), np.abs(u) + np.abs(t) + np.abs(n)     # |terms| of h - p and h - n
    # a distance: h = u + t and h - p (2 roundings on |u| + |t| + |p|, which reach the norm as 2 ||a||), D fmas halved by the
    # square root, sqrtf: error <= u32 (2 ||a|| + (D / 2 + 1) ps)
    eps_p = U32 * (2 * np.linalg.norm(ap, axis=1) + (D / 2 + 1) * ps)
    eps_n = U32 * (2 * np.linalg.norm(an, axis=1) + (D / 2 + 1) * ns)
    # no quad within fp32's reach of the kink of the relu (p == n at margin 0 sits exactly on it, in fp32 as in fp64)
    assert ((np.abs(gap) > 2 * (eps_p + eps_n + 2 * U32 * (margin + ps + ns))) | (gap == 0)).all()
    # loss: the two distance errors, 2 additions on margin + ps + ns, then the two-stage mean (3 + 2): c = 7
    chk.close("loss", got_loss, float(loss.detach()), (margin + ps + ns).mean(), 7, extra=(eps_p + eps_n).mean())
    chk.close("reg", got_reg, float(reg.detach()), float(reg.detach()), 4 * D + 5)    # 4 D fmas, 3 + 2 of the two-stage sum
    live = gap > 0
    g0, g1 = g[0] / B, g[1] / B
    with np.errstate(divide="ignore", invalid="ignore"):
        cp = np.where(live & (ps > 0), g0 / ps, 0.0)[:, None]
        cn = np.where(live & (ns > 0), g0 / ns, 0.0)[:, None]
        rp = np.where(ps > 0, eps_p / ps, 0.0)[:, None]             # relative error of 1 / ps, from the forward's ps
        rn = np.where(ns > 0, eps_n / ns, 0.0)[:, None]
    q = quad.numpy()
    # c = 8: g * (1 / B) with the float 1 / B (2), the divide by the distance, h, h - p, the product, the second product's
    # subtraction, the fma with g1 * row; + the element's multiplicity for the atomic additions
    for nm, got, ref, n_rows, idx, mags, slopes in (
            ("dEu", gu.grad, ru.grad, 20, q[:, 0], np.abs(cp) * ap + np.abs(cn) * an + np.abs(g1 * u), rp * np.abs(cp) * ap + rn * np.abs(cn) * an),
            ("dEt", gt.grad, rt.grad, 15, q[:, 1], np.abs(cp) * ap + np.abs(cn) * an + np.abs(g1 * t), rp * np.abs(cp) * ap + rn * np.abs(cn) * an),
            ("dEi", gi.grad, ri.grad, 30, np.concatenate([q[:, 2], q[:, 3]]),
             np.concatenate([np.abs(cp) * ap + np.abs(g1 * p), np.abs(cn) * an + np.abs(g1 * n)]),
             np.concatenate([rp * np.abs(cp) * ap, rn * np.abs(cn) * an]))):
        mag, _, mult = _scatter64(n_rows, D, idx, mags)
        extra, _, _ = _scatter64(n_rows, D, idx, slopes)
        chk.close(nm, got, ref, mag, 8 + mult, extra=extra)
    chk.done()


# ==================================================================================================== message dropout
DROP_N4 = 1048576 + 5                   # float4 elements: five more than the 4096 x 256 threads of the capped grid
SEEDS = (1, 2, (2020 << 24) + 1)


@pytest.fixture(scope="module")
def drop_x():
    x = _randn(4 * DROP_N4, seed=77)
    return x.to(DEV), x.numpy().reshape(-1, 4)


@pytest.mark.parametrize("seed", SEEDS)
@pytest.mark.parametrize("p", [1e-6, 0.1, 0.5, 0.999])
def test_message_drop_equals_numpy_restatement(drop_x, p, seed):
    xg, xn = drop_x
    want = np_drop(xn, np.arange(DROP_N4), p, seed)
    got = H.message_drop(xg, p, seed)
    assert np.array_equal(got.cpu().numpy().reshape(-1, 4).view(np.uint32), want.view(np.uint32))
    kept = float((want != 0).mean())
    assert abs(kept - (1 - int(np.float32(p) * 65536) / 65536)) < 4 * np.sqrt(0.25 / want.size) + 1e-3
    if p == 1e-6:
        assert (want != 0).sum() == (xn != 0).sum()                  # threshold 0: nothing dropped, still scaled
    inplace = xg.clone()
    assert H.message_drop(inplace, p, seed, out=inplace) is inplace and _same_bits(inplace, got)


@pytest.mark.parametrize("D,T_", [(4, 500), (64, 500), (64, 65600)])
def test_message_drop_rows_equals_rows_of_the_full_mask(D, T_):
    """A row list with repeats, out of order; 65 600 x 16 float4 is past the block cap (the grid-stride loop runs)."""
    N, p, seed = 3000, 0.3, SEEDS[2]
    full = _randn(N, D, seed=D)
    rows = torch.randint(0, N, (T_,), generator=torch.Generator().manual_seed(T_))
    rows[:4] = torch.tensor([N - 1, 0, N - 1, 17])
    x = full[rows].contiguous()
    d4 = D // 4
    idx4 = rows.numpy()[:, None] * d4 + np.arange(d4)[None, :]
    want = np_drop(x.numpy().reshape(T_, d4, 4), idx4, p, seed).reshape(T_, D)
    got = H.message_drop(x.to(DEV), p, seed, rows=rows.to(DEV))
    assert np.array_equal(got.cpu().numpy().view(np.uint32), want.view(np.uint32))
    whole = H.message_drop(full.to(DEV), p, seed)
    assert _same_bits(got, whole[rows.to(DEV)])
    inplace = x.to(DEV)
    H.message_drop(inplace, p, seed, out=inplace, rows=rows.to(DEV))
    assert _same_bits(inplace, got)


# ============================================================================================================= sampler
M64 = (1 << 64) - 1


def py_mix64(z):
    z = (z + 0x9E3779B97F4A7C15) & M64
    z = ((z ^ (z >> 30)) * 0xBF58476D1CE4E5B9) & M64
    z = ((z ^ (z >> 27)) * 0x94D049BB133111EB) & M64
    return z ^ (z >> 31)


def py_sample(left, rows, n_right, seed):
    """Python-int restatement: draw t of entry e is mix64(mix64(seed ^ mix64(e)) + t) * n_right >> 64, re-drawn while it is
    a positive of the entry's left id (at most 4096 times)."""
    out = []
    for e, l in enumerate(left):
        base = py_mix64(seed ^ py_mix64(e))
        for t in range(4096):
            draw = (py_mix64((base + t) & M64) * n_right) >> 64
            if draw not in rows[l]:
                break
        out.append(draw)
    return out


def _positives(rows, n_right):
    pairs = [(l, r) for l, rs in enumerate(rows) for r in sorted(rs)]
    lr = torch.tensor(pairs, dtype=torch.int64, device=DEV).reshape(-1, 2)
    return train_data._Positives(lr[:, 0], lr[:, 1], len(rows), n_right)


@pytest.mark.parametrize("seed", [5, (2020 << 20) + 3])
def test_sampler_equals_python_restatement(seed):
    # 1000 entries (not a multiple of the 256-thread block), left ids repeat; rows: empty, {0, n_right - 1}, all but id 17,
    # a few ids, empty
    n_right = 48
    rows = [set(), {0, 47}, set(range(48)) - {17}, {3, 4, 5, 30}, set()]
    left = torch.randint(0, 5, (1000,), generator=torch.Generator().manual_seed(1))
    pos = _positives(rows, n_right)
    got = pos.sample(left.to(DEV), seed).cpu().tolist()
    assert got == py_sample(left.tolist(), rows, n_right, seed)
    assert all(g == 17 for g, l in zip(got, left.tolist()) if l == 2)
    # n_right = 1: the only id, whatever the word; n_right = 2^40 + 7: draws past 32 bits (empty rows: nothing to hold
    # in the int32 column list for them)
    for n_right in (1, 2 ** 40 + 7):
        rows = [set(), {0}, set()]
        left = torch.tensor([0, 2, 2, 0, 0, 2] * 50)
        got = _positives(rows, n_right).sample(left.to(DEV), seed).cpu().tolist()
        assert got == py_sample(left.tolist(), rows, n_right, seed)
        assert n_right == 1 or max(got) > 2 ** 32


# ================================================================================================================ Adam
ADAM_N = 4 * (2 * 1048576 + 524288 + 3) + 3      # threads of the capped grid with different main-loop / remainder trips, + tail
LR = 0.01


def _adam_grads(n, steps, seed):
    """Per step, by element index mod 3: scale 1, scale 1e-8, exact zero -- interleaved, so that every part of every loop of
    the kernel meets all three."""
    scale = torch.tensor([1.0, 1e-8, 0.0]).repeat(n // 3 + 1)[:n]
    return [torch.randn(n, generator=torch.Generator().manual_seed(seed + k)) * scale for k in range(steps)]


def _run_adam(p0, grads, **kw):
    p = torch.nn.Parameter(p0)
    opt = T.Adam([p], lr=LR, **kw)
    for g in grads:
        p.grad = g.to(DEV)
        opt.step()
    return p.detach()


def _ref_adam(p0, grads):
    p = p0.double().clone().requires_grad_()
    opt = torch.optim.Adam([p], lr=LR)
    for g in grads:
        p.grad = g.double()
        opt.step()
    return p.detach()


def test_adam_two_in_flight_loop_against_torch_fp64():
    chk = Chk(f"adam n={ADAM_N}, 4 steps")
    p0, grads = _randn(ADAM_N, seed=1), _adam_grads(ADAM_N, 4, seed=2)
    ref = _ref_adam(p0, grads)
    got = _run_adam(p0.to(DEV), grads)
    # c = 12 (the bound the update is held to): m 2 + the float 1 - b1; v 3 + the float 1 - b2, halved by sqrtf, the float
    # sqrt(bc2), the divide, + eps; m / denom; the float step size; the last fma
    chk.close("p", got, ref, np.abs(_f64(ref)) + LR, 12)
    assert (got[2::3].cpu() == p0[2::3]).all() and (got[0::3].cpu() != p0[0::3]).all()      # zero gradient: untouched
    cap = _run_adam(p0.to(DEV), grads, capturable=True)
    assert _same_bits(cap, got)
    chk.done()


def test_adam_unaligned_parameter_against_torch_fp64():
    """A view 4 bytes into its buffer: not 16-byte aligned, every element goes through the scalar kernel."""
    chk = Chk("adam, 4-byte-offset view")
    n = 1003
    p0, grads = _randn(n, seed=3), _adam_grads(n, 4, seed=4)
    buf = torch.zeros(n + 1, device=DEV)
    view = buf[1:]
    view.copy_(p0)
    assert view.data_ptr() % 16 == 4
    for kw in ({}, {"capturable": True}):
        view.copy_(p0)
        got = _run_adam(view, grads, **kw)
        assert got.data_ptr() == view.data_ptr()
        chk.close("p", got, _ref_adam(p0, grads), np.abs(_f64(_ref_adam(p0, grads))) + LR, 12)
    assert float(buf[0]) == 0.0
    chk.done()


def test_adam_multi_70_tensors_same_bits_as_one_launch_each():
    lib = _lib.load()
    sizes = [(0, 1, 3, 5, 4097)[i % 5] for i in range(70)]           # 70 > the 64 tensors of one launch
    mk = lambda seed, scale: [_randn(n, seed=seed + i, scale=scale).to(DEV) for i, n in enumerate(sizes)]
    P, G, M, V = mk(0, 0.1), mk(100, 1.0), mk(200, 0.01), [t.abs() for t in mk(300, 0.01)]
    P1, M1, V1 = ([t.clone() for t in ts] for ts in (P, M, V))
    k = len(sizes)
    arr = [(ctypes.c_void_p * k)(*[t.data_ptr() for t in ts]) for ts in (P, G, M, V)]
    n = (ctypes.c_int64 * k)(*sizes)
    _lib.check(lib.tagrec_adam_multi_f32(k, arr[0], arr[1], arr[2], arr[3], n, LR, 0.9, 0.999, 1e-8, 3, _lib.stream_ptr()), "adam_multi")
    for p, g, m, v in zip(P1, G, M1, V1):
        if p.numel():
            _lib.check(lib.tagrec_adam_f32(_lib.ptr(p), _lib.ptr(g), _lib.ptr(m), _lib.ptr(v), p.numel(), LR, 0.9, 0.999, 1e-8, 3,
                                           _lib.stream_ptr()), "adam")
    torch.cuda.synchronize()
    for a, b in zip(P + M + V, P1 + M1 + V1):
        assert _same_bits(a, b)
    assert not _same_bits(P[4], mk(0, 0.1)[4])                       # and it did update
