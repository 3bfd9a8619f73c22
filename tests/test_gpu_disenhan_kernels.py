"""GPU: every entry point of csrc/disenhan.hip -- the edge softmax (forward; backward row pass and column pass), the relation
epilogue (forward; backward with dZ, with dr, with both, with neither) and the combine (forward, backward) -- each against the
plain fp64 restatement of its own operation in tests/disenhan_ref.py (held to fp64 torch autograd of tests/disenhan_torch.py by
test_disenhan_ref_host.py, which also asserts that the inputs below hold the edges they are meant to hold).

Tolerance: the convention of test_gpu_spmm.py (spmm_ref.Chk): |got - ref64| <= c * 2^-24 * mag + extra + 1e-30, the counts `c`
those of the header of disenhan_ref.py, derived from the kernels' operation sequences and written beside each check.  A backward
pass is fed the forward kernel's own fp32 outputs; what a kernel forms from a value it has just stored (g, dZt, x, dx) is held to
the reference evaluated at that stored float.  Guard rows, exact zeros, alpha == fl(1 / deg) on closed rows, the clamped 1e12,
refused calls and "two launches have the same bits" are exact; no element is left out of any comparison.  Every test prints its
worst err / bound (`-s`); DESIGN section 2 carries the table.

Edge passes: one hand-built merged relation, 303 x 201 (neither a multiple of the 4 wavefronts of a block), multiplicities
1 ... 4, row degrees 0, 1, 2, 63, 64, 65, 128, 129, 190 and column degrees 0, 1, 63, 64, 65 and a hub, a block of entries with
sL + sR == 0 exactly, rows whose every gate is closed; `big` scales the scores so that the logits span beyond +-80.
Row passes: all 20 (D, K) pairs at n in {1, RB + 1, 5 RB - 1} (RB = 256 / D rows per block), and at n = 4096 RB + RB + 1 for
D in {16, 64, 256} -- more groups than the grid's cap, so blocks 0 and 1 take a second trip of the grid-stride loop, which
nothing else in the suite does."""
import functools

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from tagrec_amd import _lib
from tagrec_amd import disenhan as DH

import disenhan_ref as RD
import spmm_ref as R
from spmm_ref import Chk as _Chk, f64, same_bits
from test_gpu_spmm import DEV, dev, nan_like, twice

GUARD = 3                                                                # NaN rows / entries kept after every output
OK, E_INVALID, E_UNSUPPORTED = 0, -1, -3                                 # TAGREC_OK, TAGREC_E_INVALID, TAGREC_E_UNSUPPORTED
SHAPES = tuple((D, K) for D in (16, 32, 64, 128, 256) for K in (1, 2, 4, 8))      # all 20 pairs the row passes accept
assert SHAPES == RD.SHAPES and len(SHAPES) == 20
SECOND_TRIP = ((256, 8), (256, 1), (16, 8), (16, 1), (64, 4), (64, 1))   # dk = 32 | 256, 2 | 16, 16 | 64: W in LDS and not
ROW_ENTRY = {"rel_epi_fwd": "tagrec_dh_rel_epi_fwd_f32", "rel_epi_bwd": "tagrec_dh_rel_epi_bwd_f32",
             "combine_fwd": "tagrec_dh_combine_fwd_f32", "combine_bwd": "tagrec_dh_combine_bwd_f32"}


def Chk(name):
    chk = _Chk(name, tag="disenhan")
    chk.exact = []                                                       # (what, holds) of exact properties: asserted by _done
    return chk


def _done(chk):
    """Print and assert the worst err / bound first, then the exact properties collected on the way."""
    chk.done()
    for what, holds in chk.exact:
        assert holds, f"{chk.name}: {what}"


def _id(s):
    return f"D{s[0]}K{s[1]}"


def _guarded(n, *w):
    """NaN-filled output of n rows (entries) and GUARD more: the kernel is given its start and n"""
    return nan_like(n + GUARD, *w)


def _untouched(t):
    return same_bits(t, torch.full_like(t, float("nan")))


def _split(chk, what, t, n):
    """the first n rows of a guarded output; the rows after them must still hold the fill's bits"""
    chk.exact.append((f"{what}: the rows after row {n} are untouched", _untouched(t[n:])))
    return t[:n]


def _stream():
    return _lib.stream_ptr()


# ============================================================================================================ edge passes
class DevRel:
    def __init__(self, rel):
        self.rowptr, self.col, self.mult = dev(rel.rowptr), dev(rel.col, torch.int32), dev(rel.mult)
        self.rowptr_t, self.col_t = dev(rel.rowptr_t), dev(rel.col_t, torch.int32)
        self.perm = dev(rel.perm, torch.int32)
        self.wrapped = DH.Relation(torch.from_numpy(rel.rowptr), torch.from_numpy(rel.col),
                                   torch.from_numpy(rel.mult.astype(np.int32)), (rel.n_rows, rel.n_cols), DEV)


@functools.lru_cache(maxsize=None)
def _dev_rel():
    rel = RD.relation()
    S = DevRel(rel)
    gt = S.wrapped.rg.graph_t                                            # the wrapper's transposed structure is the host's
    assert np.array_equal(gt.rowptr.cpu().numpy(), rel.rowptr_t) and np.array_equal(gt.col.cpu().numpy(), rel.col_t)
    assert np.array_equal(S.wrapped.rg.perm.cpu().numpy(), rel.perm)
    return S


@functools.lru_cache(maxsize=None)
def _edge_fwd_ref(K, case):
    """the forward reference, once per (K, case)"""
    rel = RD.relation()
    sL, sR, r, _ = RD.edge_inputs(K, case)
    return RD.edge_softmax_fwd(rel.rowptr, rel.col, rel.mult, sL, sR, r)


def _edge_fwd(S, K, sL, sR, r, n_rows, nnz):
    alpha = _guarded(nnz)
    rc = _lib.load().tagrec_dh_edge_softmax_fwd_f32(S.rowptr, S.col, S.mult, n_rows, sL, sR, r, K, alpha, _stream())
    return rc, alpha


def _edge_bwd(S, K, sL, sR, r, alpha, dalpha, n_rows, n_cols, shape):
    """shape: (nnz, rows, cols) of the guarded outputs -> rc, (g, dr, dsL, dsR)"""
    out = (_guarded(shape[0]), _guarded(shape[1], K), _guarded(shape[1], K), _guarded(shape[2], K))
    rc = _lib.load().tagrec_dh_edge_softmax_bwd_f32(S.rowptr, S.col, S.mult, n_rows, S.rowptr_t, S.col_t, S.perm, n_cols, sL, sR, r,
                                                    K, alpha, dalpha, *out, _stream())
    return rc, out


@pytest.mark.parametrize("case", ["plain", "big"])
@pytest.mark.parametrize("K", [1, 2, 4, 8])
def test_edge_softmax_fwd_bwd(K, case):
    rel, S = RD.relation(), _dev_rel()
    sL, sR, r, dalpha = RD.edge_inputs(K, case)
    sLg, sRg, rg, dag = sL.to(DEV), sR.to(DEV), r.to(DEV), dalpha.to(DEV)
    nnz, n_rows, n_cols, rp = rel.nnz, rel.n_rows, rel.n_cols, rel.rowptr
    chk = Chk(f"edge softmax K={K} {case}")
    (a_ref, a_mag, a_extra), (logit, _) = _edge_fwd_ref(K, case)
    if case == "big":
        assert logit.min() < -80 and logit.max() > 80

    def fwd():
        rc, alpha = _edge_fwd(S, K, sLg, sRg, rg, n_rows, nnz)
        _lib.check(rc, "dh_edge_softmax_fwd")
        return (alpha,)
    alpha = _split(chk, "alpha", twice(fwd)[0], nnz)
    t_e = RD.tree(rel.deg)[rel.rows_of]                                  # per entry: the sum tree of its row
    # expf of the numerator 8, the row sum of terms carrying expf's 8 through tree(deg), the divide: tree(deg) + 17; extra: the
    # logit's absolute error (K + 2 roundings), the row maximum's, and the rounding of logit - max, through the slope
    chk.close("alpha", alpha, a_ref, a_mag, t_e + 17, a_extra)
    ah = alpha.cpu().numpy()
    closed = dict(RD.CLOSED_ROWS)
    if K == 1:
        closed[RD.ZERO_ROWS[0]] = len(RD.ZERO_COLS)                     # its only factor is the exact-zero one
    for i, d in closed.items():
        chk.exact.append((f"row {i}: every gate closed, alpha == fl(1 / {d})",
                          bool((ah[rp[i]:rp[i + 1]] == np.float32(1.0) / np.float32(d)).all())))
    chk.exact.append(("single-entry rows: alpha == 1", bool((ah[rp[:-1][rel.deg == 1]] == 1.0).all())))
    chk.exact.append(("wrapper == direct call (forward)", same_bits(DH.edge_softmax(sLg, sRg, rg, S.wrapped), alpha)))

    def bwd():
        rc, out = _edge_bwd(S, K, sLg, sRg, rg, alpha, dag, n_rows, n_cols, (nnz, n_rows, n_cols))
        _lib.check(rc, "dh_edge_softmax_bwd")
        return out
    out = twice(bwd)
    g, dr, dsL, dsR = (_split(chk, what, t, n) for what, t, n in zip(("g", "dr", "dsL", "dsR"), out, (nnz, n_rows, n_rows, n_cols)))
    # fed the kernel's own alpha; the three sums from the g the row pass stored
    (g_ref, g_mag), dr_ref, dsL_ref, dsR_ref = RD.edge_softmax_bwd(rp, rel.col, rel.mult, n_cols, sL, sR, r, alpha, dalpha, g=g)
    t_r, t_c = RD.tree(rel.deg)[:, None], RD.tree(rel.cdeg)[:, None]
    chk.close("g", g, g_ref, g_mag, t_e + 3)                             # the dot's tree, the subtraction, two products
    chk.close("dr", dr, *dr_ref, t_r + 1)                                # sL + sR, fmas through the row's tree
    chk.close("dsL", dsL, *dsL_ref, t_r)                                 # fmas through the row's tree
    chk.close("dsR", dsR, *dsR_ref, t_c)                                 # fmas through the transposed row's tree
    drh, dsLh, dsRh = dr.cpu().numpy(), dsL.cpu().numpy(), dsR.cpu().numpy()
    chk.exact.append(("empty rows: dr == dsL == 0", bool((drh[rel.deg == 0] == 0).all() and (dsLh[rel.deg == 0] == 0).all())))
    chk.exact.append(("empty columns: dsR == 0", bool((rel.cdeg == 0).sum() == 2 and (dsRh[rel.cdeg == 0] == 0).all())))
    chk.exact.append(("closed rows: dr == dsL == 0", bool((drh[list(closed)] == 0).all() and (dsLh[list(closed)] == 0).all())))
    # sL + sR == 0 exactly is a closed gate: row 30 and column 10 hold only such entries in factor 0
    z0, c0 = RD.ZERO_ROWS[0], RD.ZERO_COLS[0]
    chk.exact.append(("sL + sR == 0 contributes nothing", bool(drh[z0, 0] == 0 and dsLh[z0, 0] == 0 and dsRh[c0, 0] == 0)))
    wl, wr, wrr = DH.edge_softmax_bwd(S.wrapped, sLg, sRg, rg, alpha.contiguous(), dag)
    chk.exact.append(("wrapper == direct call (backward)", same_bits(wl, dsL) and same_bits(wr, dsR) and same_bits(wrr, dr)))
    _done(chk)


def test_edge_passes_sizes_and_refusals():
    """n_rows = 0 / n_cols = 0 write nothing; a prefix of the rows writes that prefix's entries alone; K = 3, K = 16, a negative
    size and a null required pointer return their error code and write nothing."""
    rel, S, K = RD.relation(), _dev_rel(), 4
    sL, sR, r, dalpha = (t.to(DEV) for t in RD.edge_inputs(K, "plain"))
    nnz, n_rows, n_cols = rel.nnz, rel.n_rows, rel.n_cols
    shape = (nnz, n_rows, n_cols)
    rc, full = _edge_fwd(S, K, sL, sR, r, n_rows, nnz)
    assert rc == OK
    rc, out = _edge_fwd(S, K, sL, sR, r, 0, nnz)
    assert rc == OK and _untouched(out)
    n7 = 7                                                               # rows 0 ... 6: the second block holds three
    cut = int(rel.rowptr[n7])
    rc, out = _edge_fwd(S, K, sL, sR, r, n7, nnz)
    assert rc == OK and same_bits(out[:cut], full[:cut]) and _untouched(out[cut:]) and 0 < cut < nnz
    alpha = full[:nnz]
    rc, bfull = _edge_bwd(S, K, sL, sR, r, alpha, dalpha, n_rows, n_cols, shape)
    assert rc == OK
    rc, out = _edge_bwd(S, K, sL, sR, r, alpha, dalpha, 0, 0, shape)
    assert rc == OK and all(_untouched(t) for t in out)
    rc, out = _edge_bwd(S, K, sL, sR, r, alpha, dalpha, n_rows, 0, shape)             # the row pass alone
    assert rc == OK and all(same_bits(a, b) for a, b in zip(out[:3], bfull[:3])) and _untouched(out[3])
    rc, out = _edge_bwd(S, K, sL, sR, r, alpha, dalpha, n7, 0, shape)
    assert rc == OK and same_bits(out[0][:cut], bfull[0][:cut]) and _untouched(out[0][cut:])
    assert all(same_bits(out[k][:n7], bfull[k][:n7]) and _untouched(out[k][n7:]) for k in (1, 2))
    # refusals
    for bad_k in (3, 16):
        rc, out = _edge_fwd(S, bad_k, sL, sR, r, n_rows, nnz)
        assert rc == E_UNSUPPORTED and _untouched(out)
        rc, out = _edge_bwd(S, bad_k, sL, sR, r, alpha, dalpha, n_rows, n_cols, shape)
        assert rc == E_UNSUPPORTED and all(_untouched(t) for t in out)
    rc, out = _edge_fwd(S, K, sL, sR, r, -1, nnz)
    assert rc == E_INVALID and _untouched(out)
    rc, out = _edge_fwd(S, K, None, sR, r, n_rows, nnz)
    assert rc == E_INVALID and _untouched(out)
    for nr, nc in ((-1, n_cols), (n_rows, -1)):
        rc, out = _edge_bwd(S, K, sL, sR, r, alpha, dalpha, nr, nc, shape)
        assert rc == E_INVALID and all(_untouched(t) for t in out)
    rc, out = _edge_bwd(S, K, sL, sR, r, None, dalpha, n_rows, n_cols, shape)
    assert rc == E_INVALID and all(_untouched(t) for t in out)
    rc, out = _edge_bwd(S, K, sL, None, r, alpha, dalpha, n_rows, n_cols, shape)
    assert rc == E_INVALID and all(_untouched(t) for t in out)
    with pytest.raises(_lib.TagrecError, match="K must be 1, 2, 4 or 8"):
        _lib.check(_edge_fwd(S, 3, sL, sR, r, n_rows, nnz)[0], "dh_edge_softmax_fwd")


# ============================================================================================================= row passes
def _rows_call(name, ins, n, D, K, widths):
    """ROW_ENTRY[name](*ins, n, D, K, *outs, stream) into guarded outputs of the given widths -> rc, outs"""
    outs = tuple(_guarded(max(n, 0), w) for w in widths)
    rc = getattr(_lib.load(), ROW_ENTRY[name])(*ins, n, D, K, *outs, _stream())
    return rc, outs


def _rows_twice(chk, name, ins, n, D, K, widths):
    def run():
        rc, outs = _rows_call(name, ins, n, D, K, widths)
        _lib.check(rc, "dh_" + name)
        return outs
    return tuple(_split(chk, f"{name}[{k}] n={n}", t, n) for k, t in enumerate(twice(run)))


def _epilogue(chk, n, D, K, seed, case, forms=(("both", True, True),)):
    """rel_epi_fwd, then rel_epi_bwd fed the forward's own Yl, Z, r, in each of `forms` (name, with dZ, with dr)
    -> Yl, Z, r, {form: (dY, dZt, dsT)}"""
    dk, tag = D // K, f"n={n} {case}"
    Y, W, q, dZ, dr = RD.epilogue_inputs(n, D, K, seed, case)
    Yg, Wg, qg, dZg, drg = (t.to(DEV) for t in (Y, W, q, dZ, dr))
    Yl, Z, r = _rows_twice(chk, "rel_epi_fwd", (Yg, Wg, qg), n, D, K, (D, D, K))
    (yl_ref, yl_mag), (z_ref, z_mag), (r_ref, r_mag, r_extra) = RD.rel_epi_fwd(Y, W, q, K)
    chk.close(f"Yl {tag}", Yl, yl_ref, yl_mag, 2)                        # the product with the slope, the float 0.2f
    chk.close(f"Z {tag}", Z, z_ref, z_mag, dk + 2)                       # dk fmas of Yl
    # s - max (extra), expf 8, the sum of K such terms 8 + K - 1, the divide; extra: the score's absolute error (Z's through
    # tanh's slope, tanhf, the product with q, the in-order slice sum) and the subtraction's, through the softmax's slope
    chk.close(f"r {tag}", r, r_ref, r_mag, K + 16, r_extra)
    yh, ylh = Y.numpy(), Yl.cpu().numpy()
    chk.exact.append((f"Yl {tag}: +-0.0 in, the same zero out", bool((ylh[yh == 0] == 0).all()
                                                                    and np.array_equal(np.signbit(ylh[yh == 0]), np.signbit(yh[yh == 0])))))
    zero_rows = (yh == 0).all(1)
    chk.exact.append((f"{tag}: an all-zero row gives Z == 0 and r == 1 / K",
                      bool((Z.cpu().numpy()[zero_rows] == 0).all() and (r.cpu().numpy()[zero_rows] == np.float32(1.0 / K)).all())))
    got = {}
    for name, with_dz, with_dr in forms:
        gz, gr = (dZ if with_dz else None), (dr if with_dr else None)
        ins = (Yl, Z, r, dZg if with_dz else None, drg if with_dr else None, Wg, qg)
        dY, dZt, dsT = got[name] = _rows_twice(chk, "rel_epi_bwd", ins, n, D, K, (D, D, D))
        ref = RD.rel_epi_bwd(Yl, Z, r, gz, gr, W, q, K, dZt=dZt)           # dY from the dZt the kernel stored
        chk.close(f"dY {tag} {name}", dY, *ref[0], dk + 2)               # dk fmas, the slope, the float 0.2f
        chk.close(f"dZt {tag} {name}", dZt, *ref[1], K + 19)             # ds_k K + 2, 1 - th^2 14, two products, the addition
        chk.close(f"dsT {tag} {name}", dsT, *ref[2], K + 2 * RD.TANH_ULP + 3)      # ds_k K + 2, tanhf, the product
        if not with_dr:
            chk.exact.append((f"{tag} {name}: dZt == dZ, dsT == 0", bool(torch.equal(dZt, dZg if with_dz else torch.zeros_like(dZt))
                                                                         and (dsT == 0).all())))
        if not with_dz and not with_dr:
            chk.exact.append((f"{tag} neither: dY == 0", bool((dY == 0).all())))
    return (Y, W, q, dZ, dr), (Yl, Z, r), got


def _combine(chk, n, D, K, seed):
    """combine_fwd, then combine_bwd fed the forward's own x and inv"""
    dk, tag = D // K, f"n={n}"
    host = RD.combine_inputs(n, D, K, seed)
    ego, Z1, r1, Z2, r2, dy = host
    eg, Z1g, r1g, Z2g, r2g, dyg = (t.to(DEV) for t in host)
    x, y, inv = _rows_twice(chk, "combine_fwd", (eg, Z1g, r1g, Z2g, r2g), n, D, K, (D, D, K))
    (x_ref, x_mag), _, _, _ = RD.combine_fwd(ego, Z1, r1, Z2, r2, K)
    chk.close(f"x {tag}", x, x_ref, x_mag, 3)                            # a term passes a product and two additions
    _, (y_ref, y_mag), (inv_ref, inv_mag), clamped = RD.combine_fwd(ego, Z1, r1, Z2, r2, K, x=x)      # from the stored x
    c_norm = dk / 2 + 3                                                  # sum of squares halved, sqrtf, the float eps, the divide
    chk.close(f"y {tag}", y, y_ref, y_mag, c_norm)
    chk.close(f"inv {tag}", inv, inv_ref, inv_mag, c_norm)
    xs = f64(x).reshape(n * K, dk)
    zero = (xs == 0).all(1)
    chk.exact.append((f"{tag}: inv == 1e12 on every clamped slice", bool((inv.cpu().numpy()[clamped] == R.INV_CLAMPED).all())))
    chk.exact.append((f"{tag}: y == 0 on every zero slice", bool((f64(y).reshape(n * K, dk)[zero] == 0).all())))
    if n * K >= 8:
        assert zero.any() and (clamped.reshape(-1) & ~zero).any() and not clamped.all()
    dx, dZ1, dZ2, dr1, dr2 = _rows_twice(chk, "combine_bwd", (x, inv, dyg, Z1g, r1g, Z2g, r2g), n, D, K, (D, D, D, K, K))
    ref = RD.combine_bwd(x, inv, dy, Z1, r1, Z2, r2, K, dx=dx)            # dZ_e and dr_e from the dx the kernel stored
    chk.close(f"dx {tag}", dx, *ref[0], dk + 6)                          # z, the dot dk, z dot, the subtraction, inv, 1 spare
    chk.close(f"dZ1 {tag}", dZ1, *ref[1], 1)                             # one product
    chk.close(f"dZ2 {tag}", dZ2, *ref[2], 1)
    chk.close(f"dr1 {tag}", dr1, *ref[3], dk + 1)                        # the product and the in-order slice sum
    chk.close(f"dr2 {tag}", dr2, *ref[4], dk + 1)
    cl = np.repeat(clamped, dk, axis=1)                                  # the dot is dropped: dx = inv dy, one product
    chk.exact.append((f"{tag}: dx == fl(1e12 dy) on every clamped slice",
                      bool(np.array_equal(dx.cpu().numpy()[cl], (R.INV_CLAMPED * dy.numpy())[cl]))))
    return host, (x, y, inv), (dx, dZ1, dZ2, dr1, dr2)


@pytest.mark.parametrize("shape", SHAPES, ids=_id)
def test_row_passes_every_shape(shape):
    D, K = shape
    chk = Chk(f"row passes D={D} K={K}")
    for n in RD.row_sizes(D):
        _epilogue(chk, n, D, K, seed=D + K + n, case="plain")
        _combine(chk, n, D, K, seed=D + K + n)
    n = RD.row_sizes(D)[2]
    _, (_, Z, _), _ = _epilogue(chk, n, D, K, seed=D + K + n, case="sat")
    assert (Z.abs() > 9.0).float().mean() > 0.2                             # tanhf(Z) is +-1 there
    # the wrappers reach the same path: the same bits
    (ego, Z1, r1, Z2, r2, dy), (x, y, inv), grads = _combine(chk, n, D, K, seed=D + K + n)
    leaves = [t.to(DEV).requires_grad_() for t in (ego, Z1, r1, Z2, r2)]
    yw = DH.combine(*leaves, K)
    yw.backward(dy.to(DEV))
    dx, dZ1, dZ2, dr1, dr2 = grads
    chk.exact.append(("combine wrapper == direct calls", same_bits(yw.detach(), y) and all(
        same_bits(a.grad, b) for a, b in zip(leaves, (dx, dZ1, dr1, dZ2, dr2)))))
    _done(chk)


@pytest.mark.parametrize("shape", SECOND_TRIP, ids=_id)
def test_row_passes_second_trip(shape):
    """n = 4096 RB + RB + 1: 4098 groups on a grid of 4096 blocks, the last group of one row."""
    D, K = shape
    n, rb = RD.second_trip_n(D), 256 // D
    assert n > 4096 * (256 // D) and -(-n // rb) == RD.MAX_GROUPS + 2 == 4098
    chk = Chk(f"second trip D={D} K={K} n={n}")
    _epilogue(chk, n, D, K, seed=D + K, case="plain")
    _combine(chk, n, D, K, seed=D + K)
    _done(chk)


@pytest.mark.parametrize("shape", SHAPES, ids=_id)
def test_rel_epi_bwd_forms(shape):
    """The backward of the epilogue with dZ only, dr only, both and neither (NULL = 0), and the wrapper's host-side dW, dq."""
    D, K = shape
    dk, n = D // K, RD.row_sizes(D)[1] + 8
    chk = Chk(f"rel_epi_bwd forms D={D} K={K}")
    # (name, dZ given, dr given): "dZ" passes dr = NULL, "dr" passes dZ = NULL, "neither" passes both as NULL
    forms = (("dZ", True, False), ("dr", False, True), ("both", True, True), ("neither", False, False))
    (Y, W, q, dZ, dr), (Yl, Z, r), got = _epilogue(chk, n, D, K, seed=3 * D + K, case="plain", forms=forms)
    dY, dZt, dsT = got["both"]
    leaves = [t.to(DEV).requires_grad_() for t in (Y, W, q)]
    Zw, rw = DH.rel_epilogue(*leaves, K)
    torch.autograd.backward([Zw, rw], [dZ.to(DEV), dr.to(DEV)])
    chk.exact.append(("epilogue wrapper == direct calls", same_bits(Zw.detach(), Z) and same_bits(rw.detach(), r)
                      and same_bits(leaves[0].grad, dY)))
    ref = RD.rel_epi_bwd(Yl, Z, r, dZ, dr, W, q, K, dZt=dZt)
    # host-side sums over the n K slices in the BLAS's order: a term passes at most n K rounded operations; dq sums the
    # stored dsT, which carries its own K + 2 TANH_ULP + 3
    chk.close("dW", leaves[1].grad, *ref[3], n * K)
    chk.close("dq", leaves[2].grad, *ref[4], n * K + K + 2 * RD.TANH_ULP + 3)
    _done(chk)


def _buf(fill=0.5):
    return torch.full((2048,), fill, device=DEV)


_ROW_ARITY = {"rel_epi_fwd": (3, 3), "rel_epi_bwd": (7, 3), "combine_fwd": (5, 3), "combine_bwd": (7, 5)}      # inputs, outputs


@pytest.mark.parametrize("name", list(_ROW_ARITY))
def test_row_passes_refuse_and_write_nothing(name):
    """D = 48, K = 3, K = 16, a negative n and a null required pointer return the documented code; n = 0 returns OK; the
    outputs keep their poison in every case."""
    n_in, n_out = _ROW_ARITY[name]
    fn = getattr(_lib.load(), ROW_ENTRY[name])

    def call(n, D, K, null_in=None, null_out=None):
        ins = [None if k == null_in else _buf() for k in range(n_in)]
        outs = [None if k == null_out else nan_like(2048) for k in range(n_out)]
        rc = fn(*ins, n, D, K, *outs, _stream())
        torch.cuda.synchronize()
        return rc, all(_untouched(t) for t in outs if t is not None)

    assert call(4, 48, 4) == (E_UNSUPPORTED, True)
    assert call(4, 48, 3) == (E_UNSUPPORTED, True)
    assert call(4, 64, 3) == (E_UNSUPPORTED, True)
    assert call(4, 64, 16) == (E_UNSUPPORTED, True)
    assert call(4, 8, 1) == (E_UNSUPPORTED, True) and call(4, 512, 8) == (E_UNSUPPORTED, True)
    assert call(-1, 64, 4) == (E_INVALID, True)
    assert call(0, 64, 4) == (OK, True)
    required = [k for k in range(n_in) if not (name == "rel_epi_bwd" and k in (3, 4))]        # dZ and dr may be NULL
    for k in required:
        assert call(4, 64, 4, null_in=k) == (E_INVALID, True), f"input {k}"
    for k in range(n_out):
        assert call(4, 64, 4, null_out=k) == (E_INVALID, True), f"output {k}"
    rc, _ = call(4, 48, 4)
    with pytest.raises(_lib.TagrecError, match="needs D in"):
        _lib.check(rc, name)
