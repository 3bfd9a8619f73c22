"""GPU: the sparse products of csrc/spmm.hip -- every row epilogue, row class, flagged / masked / listed / edge-dropout form --
each against the plain fp64 restatement of its own operation in tests/spmm_ref.py (held to torch autograd by
test_spmm_ref_host.py).

Tolerance: the convention of test_gpu_rowops.py (spmm_ref.Chk): |got - ref64| <= c * 2^-24 * mag + 1e-30.  For a product row
c = its stored entries + its 512-entry chunks when it is long (`Ladder.c`: every term passes at most that many rounded
additions whatever the lane / chunk tree, an fma rounding once), + 1 where each weight is divided by 1 - p (edge dropout), + the
rounded operations of the epilogue, written beside each check.  Flags, counts, masks and "row untouched" are exact.  Every
test prints its worst err / bound (`-s`); DESIGN section 2 carries the table.

The ladder graph (`build_ladder`): 2301 x 2999 (and a 2301 x 2301 sibling), signed values, ~1e5 stored entries.  Rows
3 + 5 i (moved by one off a multiple of 32) hold the degree ladder 0, 1, 2, 3, 31, 32, 33, 63, 64, 65, 511, 512, 513, 1023,
1024 (the last short row), 1025, 1536, 2047, 2048, 2049 and a hub of 97 * 512 + 1 (column ids of the long rows repeat), then the
rows built around the 40 flagged columns `F` (below); the other rows have <= 80 distinct columns, column 2 among them in three
rows of four, so that the transpose has a long row too.  A lane group of the grouped
kernel (2 - 32 consecutive rows) therefore mixes long, short and empty rows.  Operand rows follow spmm_ref.norm_rows by index mod
8 (1: zero, 3: norm 1e-13); ordinary rows 9 mod 16 gather zero rows only (an exactly-zero product row) and rows 13 mod 16
at most four rows of norm 1e-13 (a clamped, non-zero product row)."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import tagrec_amd as T
from tagrec_amd import _lib
from tagrec_amd.dist import HipOps
from tagrec_amd.rowops import VEC_WIDTHS

import spmm_ref as R
from spmm_ref import Chk as _Chk, f64, same_bits

DEV = torch.device("cuda:0")
OPS = HipOps()
SCALAR_WIDTHS = (4, 10, 100, 260, 512)
S = float(np.float32(1.0 / 3.0))       # a scale that is exact as the float the ABI takes
NAN = float("nan")
HUB = 97 * 512 + 1
LADDER = (0, 1, 2, 3, 31, 32, 33, 63, 64, 65, 511, 512, 513, 1023, 1024, 1025, 1536, 2047, 2048, 2049, HUB)
K_LONG, K_CHUNK = 1024, 512            # kLongRow, kChunk of csrc/graph.h
LONG_COL = 2                           # the column three quarters of the ordinary rows store: a long row of the transpose


def Chk(name):
    return _Chk(name, tag="spmm")


def dev(a, dtype=None):
    t = a if isinstance(a, torch.Tensor) else torch.from_numpy(np.ascontiguousarray(a))
    return t.to(DEV) if dtype is None else t.to(DEV, dtype)


def nan_like(*shape):
    return torch.full(shape, NAN, device=DEV)


def twice(run):
    """Run a product twice from fresh buffers: every output of the two runs must have the same bits.  -> the outputs."""
    a, b = run(), run()
    assert all(same_bits(s, t) for s, t in zip(a, b)), "two runs of one product differ"
    return a


# ============================================================================================================ the ladder
def _lane_patterns(rng, F, U):
    """5 batches of 64 entries whose flagged (F) entries are: none, all, lane 0 only, lane 63 only, a scattered handful."""
    out = []
    for lanes in ((), range(64), (0,), (63,), (3, 17, 18, 40, 62)):
        b = rng.choice(U, 64)
        b[list(lanes)] = rng.choice(F, len(list(lanes)))
        out.append(b)
    return np.concatenate(out)


class Ladder:
    def __init__(self, name, rowptr, col, val, n_cols, graph=None, special=None, F=None):
        self.name, self.rowptr, self.col, self.val = name, np.asarray(rowptr, np.int64), np.asarray(col, np.int64), np.asarray(val, np.float32)
        self.n_rows, self.n_cols = len(rowptr) - 1, n_cols
        self.deg = np.diff(self.rowptr)
        self.long = self.deg > K_LONG
        self.chunks = np.where(self.long, -(-self.deg // K_CHUNK), 0)
        self.c = (self.deg + self.chunks).astype(np.float64)[:, None]      # rounded operations of a product row
        self.rows_of = np.repeat(np.arange(self.n_rows), self.deg)
        self.special, self.F = special or {}, F
        self.g = graph if graph is not None else T.Graph(dev(self.rowptr), dev(self.col, torch.int32), dev(self.val), (self.n_rows, n_cols))
        self._t, self._prod = None, {}

    @property
    def t(self):
        """The transposed graph (`Graph.transpose()`: duplicates summed) with its CSR read back to the host and held to the
        host transpose of this CSR: the same structure, columns ascending, each value the sum of its duplicates (summed in
        fp32 in no fixed order: k duplicates within k - 1 roundings of the sum of their magnitudes)."""
        if self._t is None:
            gt = self.g.transpose()
            t = Ladder(self.name + "^T", gt.rowptr.cpu().numpy(), gt.col.cpu().numpy(), gt.val.cpu().numpy(), self.n_rows, gt)
            rp, c, v = R.transpose_csr(self.rowptr, self.col, self.val, self.n_cols)
            key = np.repeat(np.arange(self.n_cols), np.diff(rp)) * self.n_rows + c
            ukey, first, k = np.unique(key, return_index=True, return_counts=True)
            assert np.array_equal(ukey, t.rows_of * self.n_rows + t.col) and (k > 1).any()
            want, mag = np.add.reduceat(f64(v), first), np.add.reduceat(np.abs(f64(v)), first)
            assert (np.abs(f64(t.val) - want) <= (k - 1) * R.U32 * mag).all()
            assert np.array_equal(t.val[k == 1], v[first][k == 1])
            self._t = t
        return self._t

    def product(self, key, X, val=None):
        """fp64 (A X, magnitude), computed once per operand key."""
        if key not in self._prod:
            if len(self._prod) > 6:
                self._prod.clear()
            self._prod[key] = R.product(self.rowptr, self.col, self.val if val is None else val, X)[:2]
        return self._prod[key]


def build_ladder(name, n_rows, n_cols, seed):
    rng = np.random.default_rng(seed)
    cols = np.arange(n_cols)
    F = cols[(cols % 8 != 1) & (cols % 8 != 3)][5::37][:40]               # 40 ordinary operand rows
    assert len(F) == 40
    U = np.setdiff1d(cols, F)
    designed = {d: None for d in LADDER}
    pat = _lane_patterns(rng, F, U)
    designed["pat"] = pat                                                # a short row: 5 designed batches
    for k in range(4):                                                   # k flagged entries at the head of a 70-entry row
        designed[f"g{k}"] = np.concatenate([rng.choice(F, k, replace=False), rng.choice(U, 70 - k, replace=False)])
    designed["g40"] = np.concatenate([rng.permutation(F), rng.choice(U, 30, replace=False)])      # every batch of <= 32 all flagged
    designed["gmid"] = np.concatenate([rng.choice(U, 33, replace=False), rng.choice(F, 3, replace=False), rng.choice(U, 34, replace=False)])
    special, pos = {}, 3
    for key in designed:
        if pos % 32 == 0:
            pos += 1
        special[key] = pos
        pos += 5
    at = {r: key for key, r in special.items()}
    rowptr, col = [0], []
    zeros, tiny = cols[cols % 8 == 1], cols[cols % 8 == 3]
    for r in range(n_rows):
        key = at.get(r)
        if key is None:
            if r % 16 == 9:
                c = rng.choice(zeros, int(rng.integers(1, 30)), replace=False)
            elif r % 16 == 13:
                c = rng.choice(tiny, int(rng.integers(1, 5)), replace=False)
            else:
                c = rng.choice(n_cols, int(rng.integers(0, 37)) if r % 3 else int(rng.integers(0, 80)), replace=False)
                if r % 4 != 1 and LONG_COL not in c:
                    c = np.append(c, LONG_COL)                           # a column with > kLongRow entries: a long row of A^T
        elif designed[key] is not None:
            c = designed[key]
        elif key > K_LONG:
            c = rng.integers(0, n_cols, key)                             # long rows: column ids repeat
            if key == 1536:
                c[:320] = pat                                            # the designed batches inside a chunk of a long row
        else:
            c = rng.choice(n_cols, key, replace=False)
        col += list(c)
        rowptr.append(len(col))
    col = np.array(col, np.int64)
    val = rng.uniform(0.05, 1.0, len(col)) * rng.choice([-1.0, 1.0], len(col))
    lad = Ladder(name, np.array(rowptr), col, val.astype(np.float32), n_cols, special=special, F=F)
    for d in LADDER:
        assert lad.deg[special[d]] == d and special[d] % 32 != 0
    assert n_rows % 128 != 0 and 8e4 < len(col) < 1.3e5
    return lad


@pytest.fixture(scope="module")
def rect():
    return build_ladder("rect", 2301, 2999, 1)


@pytest.fixture(scope="module")
def square():
    return build_ladder("square", 2301, 2301, 2)


def test_ladder_long_row_list(rect, square):
    for lad in (rect, square):
        info = lad.g.info()
        assert info["n_long_rows"] == int(lad.long.sum()) == 6
        assert info["n_chunks"] == int(lad.chunks.sum()) == 3 + 3 + 4 + 4 + 5 + 98
        assert (info["n_rows"], info["n_cols"], info["nnz"]) == (lad.n_rows, lad.n_cols, len(lad.col))
    t = rect.t
    info = t.g.info()
    assert t.deg[LONG_COL] > K_LONG and info["n_long_rows"] == int(t.long.sum()) and info["n_chunks"] == int(t.chunks.sum())


# ============================================================================================================ operands
class Ops:
    """Operands of one (graph, width): X / G gathered [n_cols, D]; x_raw, dz, acc0, b [n_rows, D]; inv of x_raw as the float32 a
    forward pass would have stored (1e12 exactly on its clamped rows); a supplied row dot."""

    def __init__(self, lad, D, seed):
        self.X, _, _ = R.norm_rows(lad.n_cols, D, seed)
        self.G, _, _ = R.norm_rows(lad.n_cols, D, seed + 10)
        self.xr, self.dz, self.clamped = R.norm_rows(lad.n_rows, D, seed + 20)
        self.inv = torch.from_numpy(R.inv_norm(self.xr)[0].astype(np.float32))
        assert (self.inv[torch.from_numpy(self.clamped)] == float(R.INV_CLAMPED)).all() and self.clamped.any()
        assert (self.inv[torch.from_numpy(~self.clamped)] < 1e6).all()
        self.acc0, self.b, self.dot = R.randn(lad.n_rows, D, seed=seed + 30), R.randn(lad.n_rows, D, seed=seed + 31), R.randn(lad.n_rows, seed=seed + 32)
        for k in ("X", "G", "xr", "dz", "inv", "acc0", "b", "dot"):
            setattr(self, k + "g", getattr(self, k).to(DEV))


def _check_norm_acc(chk, what, lad, D, y, m, acc0, got_y, got_inv, got_acc, rows=slice(None), c_extra=0):
    """NORM_ACC outputs on `rows` against the epilogue reference of the fp64 product (y, m)."""
    (_, _), (iv, ivm), acc, _ = R.epi_norm_acc(y, m, acc0, S)
    c = lad.c + c_extra
    chk.close(what + " y", f64(got_y)[rows], y[rows], m[rows], c[rows])
    # inv: D fmas of the sum of squares (halved by the square root), sqrtf, the float eps, the divide: + D + 3
    chk.close(what + " inv", f64(got_inv)[rows], iv[rows], ivm[rows], (c[:, 0] + D + 3)[rows])
    nrm = np.linalg.norm(y, axis=1)
    sure = np.zeros(len(nrm), bool)
    sure[rows] = True
    sure &= nrm < 0.999e-12                                             # clamped beyond fp32's doubt: exactly 1e12
    assert (got_inv.cpu().numpy()[sure] == R.INV_CLAMPED).all()
    if got_acc is not None:
        # acc: the quotient by the rounded norm (+ D + 3), s * (.) and the addition as one fma, + 2 spare: + D + 6
        chk.close(what + " acc", f64(got_acc)[rows], acc[0][rows], acc[1][rows], (c + D + 6)[rows])
    return sure


# ====================================================================================== every epilogue, all rows, twice
def _all_epilogues(chk, lad, D, Xg=None, o=None):
    g, n = lad.g, lad.n_rows
    o = o or Ops(lad, D, seed=D)
    Xg = o.Xg if Xg is None else Xg                                      # (the unaligned test passes its own view of X)
    Gg = o.Gg
    y, m = lad.product(("X", D), o.X)
    pg, pm = lad.product(("G", D), o.G)
    c = lad.c

    (out,) = twice(lambda: (g.spmm(Xg, nan_like(n, D)),))
    chk.close("spmm", out, y, m, c)                                      # c = entries + chunks

    def norm_acc():
        yg, ig, ag = nan_like(n, D), nan_like(n), o.acc0g.clone()
        g.spmm_norm_acc(Xg, yg, ig, ag, S)
        return yg, ig, ag
    yg, ig, ag = twice(norm_acc)
    sure = _check_norm_acc(chk, "norm_acc", lad, D, y, m, o.acc0, yg, ig, ag)
    if lad.name == "rect":
        assert sure.any() and (y == 0).all(1).any() and (sure & (y != 0).any(1)).any()      # zero and tiny product rows exist
    if D in VEC_WIDTHS and Xg is o.Xg:                                   # acc = None: the layer mean is not accumulated
        y2, i2 = nan_like(n, D), nan_like(n)
        g.spmm_norm_acc_rows(Xg, y2, i2, None, S, None)
        assert same_bits(y2, yg) and same_bits(i2, ig)

    def normbwd():
        og = nan_like(n, D)
        g.spmm_normbwd(Gg, o.xrg, o.invg, o.dzg, S, og)
        return (og,)
    ref, mag = R.epi_normbwd(pg, pm, o.xr, o.inv, o.dz, S, o.clamped)
    # + D + 7: the D + 6 of the normalize-backward row (test_gpu_rowops.py) and its addition to the product
    chk.close("normbwd", twice(normbwd)[0], ref, mag, c + D + 7)

    def axpy():
        og = nan_like(n, D)
        g.spmm_axpy(Gg, o.bg, S, og)
        return (og,)
    ref, mag = R.epi_axpy(pg, pm, o.b, S)
    chk.close("axpy", twice(axpy)[0], ref, mag, c + 1)                   # + 1: one fma

    def ss():
        og, sg = nan_like(n, D), nan_like(n)
        OPS.spmm_ss(g, Xg, og, sg)
        return og, sg
    og, sg = twice(ss)
    ref, mag = R.epi_ss(y, m)
    chk.close("ss y", og, y, m, c)
    chk.close("ss", sg, ref, mag, c[:, 0] + D)                           # + D fmas

    def nbdot():
        og = nan_like(n, D)
        OPS.spmm_normbwd_dot(g, Gg, o.xrg, o.invg, o.dzg, o.dotg, S, og)
        return (og,)
    ref, mag = R.epi_normbwd_dot(pg, pm, o.xr, o.inv, o.dz, o.dot, S)
    # + 6: s dz, x inv, (.) dot, the subtraction, the product with inv, the addition to the product
    chk.close("normbwd_dot", twice(nbdot)[0], ref, mag, c + 6)


@pytest.mark.parametrize("transposed", [False, True])
@pytest.mark.parametrize("D", VEC_WIDTHS + SCALAR_WIDTHS)
def test_every_epilogue_all_rows(rect, D, transposed):
    lad = rect.t if transposed else rect
    chk = Chk(f"epilogues {lad.name} D={D}")
    _all_epilogues(chk, lad, D)
    chk.done()


def test_unaligned_operand_takes_the_scalar_kernel_or_is_refused(rect, square):
    """D = 64 with the gathered operand a contiguous view 4 bytes into its storage: not 16-byte aligned, so the scalar kernel
    serves the six plain forms (same bounds); the forms that only the vector kernels implement refuse the operand."""
    D = 64
    chk = Chk("unaligned operand D=64")
    o = Ops(rect, D, seed=D)
    buf = torch.zeros(rect.n_cols * D + 1, device=DEV)
    Xv = buf[1:].view(rect.n_cols, D)
    Xv.copy_(o.Xg)
    assert Xv.is_contiguous() and Xv.data_ptr() % 16 == 4
    o.Gg = torch.zeros(rect.n_cols * D + 1, device=DEV)[1:].view(rect.n_cols, D).copy_(o.Gg)
    assert o.Gg.data_ptr() % 16 == 4
    _all_epilogues(chk, rect, D, Xg=Xv, o=o)
    chk.done()
    g, n = rect.g, rect.n_rows
    mask = torch.ones(n, dtype=torch.uint8, device=DEV)
    fl = torch.ones(rect.n_cols, dtype=torch.uint8, device=DEV)
    cnt = torch.zeros(1, dtype=torch.int32, device=DEV)
    refused = {
        "row_mask": lambda: g.spmm_rows(Xv, nan_like(n, D), mask),
        "flags": lambda: g.spmm_flags(Xv, fl, None, nan_like(n, D), torch.zeros(n, dtype=torch.uint8, device=DEV), cnt),
        "dropout": lambda: g.spmm_norm_acc(Xv, nan_like(n, D), nan_like(n), o.acc0g.clone(), S, drop_p=0.5, seed=1),
        "acc=None": lambda: g.spmm_norm_acc_rows(Xv, nan_like(n, D), nan_like(n), None, S, None),
    }
    for what, call in refused.items():
        with pytest.raises(_lib.TagrecError):
            call()
    so = Ops(square, D, seed=D)
    Gv = torch.zeros(square.n_cols * D + 1, device=DEV)[1:].view(square.n_cols, D).copy_(so.Gg)
    p, mm, vv = so.acc0g.clone(), torch.zeros_like(so.acc0g), torch.zeros_like(so.acc0g)
    with pytest.raises(_lib.TagrecError):
        square.g.spmm_axpy_adam(Gv, None, None, so.bg, S, None, p, mm, vv, 0.01, (0.9, 0.999), 1e-8, 1)
    torch.cuda.synchronize()
    assert same_bits(p, so.acc0g) and float(mm.abs().max()) == 0.0


# ============================================================================================== flags of an output
def _mixed_flags(n, inside):
    """Pre-fill of an out_flags array: 9 on the rows the product computes, and 0 / 9 alternating on the others (the caller
    zeroes them; whatever is there stays and is counted)."""
    f = torch.full((n,), 9, dtype=torch.uint8)
    outside = torch.from_numpy(~inside)
    f[outside] = (torch.arange(n)[outside] % 2 * 9).to(torch.uint8)
    return f


def _check_out_flags(got, ref, mag, flags, count, inside, pre):
    """flags[r] == 'got row has a non-zero' on the computed rows, == the reference's answer where its magnitude is non-zero;
    untouched elsewhere; count == non-zero bytes of the whole array."""
    fl, g = flags.cpu().numpy(), got.cpu().numpy()
    assert np.array_equal(fl[inside], (g[inside] != 0).any(1).astype(np.uint8))
    live = inside & (mag != 0).any(1)
    assert np.array_equal(fl[live], (ref[live] != 0).any(1).astype(np.uint8))
    assert not fl[inside & ~(mag != 0).any(1)].any()
    assert np.array_equal(fl[~inside], pre.numpy()[~inside])
    if count is not None:
        assert int(count.item()) == int(np.count_nonzero(fl))


def _untouched(t, pre, inside):
    out = torch.from_numpy(~inside).to(DEV)
    return same_bits(t[out], pre.to(DEV)[out])


# ============================================================================================================ row masks
def _masks(lad):
    rng = np.random.default_rng(7)
    return {"random": rng.random(lad.n_rows) < 0.5, "long": lad.long.copy(), "short": ~lad.long,
            "none": np.zeros(lad.n_rows, bool)}


@pytest.mark.parametrize("kind", ["random", "long", "short", "none"])
@pytest.mark.parametrize("D", VEC_WIDTHS)
def test_row_masks(square, D, kind):
    lad = square
    chk = Chk(f"row masks D={D} mask={kind}")
    g, n = lad.g, lad.n_rows
    inside = _masks(lad)[kind]
    mask = dev(inside.astype(np.uint8))
    o = Ops(lad, D, seed=D)
    y, m = lad.product(("X", D), o.X)
    o.G[1::2] = 0                                                        # under 4/5 of the rows flagged: the flags are consulted
    o.Gg = o.G.to(DEV)
    pg, pm = lad.product(("G/2", D), o.G)
    c = lad.c
    pre2, pre1 = torch.full((n, D), NAN), torch.full((n,), -7.0)
    in_flags = dev(R.row_flags(o.G))
    in_count = in_flags.sum(dtype=torch.int32).reshape(1)
    assert 0 < int(in_count) < 0.8 * n

    def both(run, outs=1):
        a, b = run(), run()
        for s, t in zip(a[:outs], b[:outs]):
            assert same_bits(s, t), "two runs of one masked product differ"
        return a

    (out,) = both(lambda: (g.spmm_rows(o.Xg, pre2.clone().to(DEV), mask),))
    chk.close("spmm_rows", f64(out)[inside], y[inside], m[inside], c[inside])
    assert _untouched(out, pre2, inside)

    def norm_acc():
        yg, ig, ag = pre2.clone().to(DEV), pre1.clone().to(DEV), o.acc0g.clone()
        g.spmm_norm_acc_rows(o.Xg, yg, ig, ag, S, mask)
        return yg, ig, ag
    yg, ig, ag = both(norm_acc, 3)
    _check_norm_acc(chk, "norm_acc_rows", lad, D, y, m, o.acc0, yg, ig, ag, rows=inside)
    assert _untouched(yg, pre2, inside) and _untouched(ig, pre1, inside) and _untouched(ag, o.acc0, inside)

    def ss_rows():
        yg, sg = pre2.clone().to(DEV), pre1.clone().to(DEV)
        OPS.spmm_ss_rows(g, o.Xg, yg, sg, mask)
        return yg, sg
    yg, sg = both(ss_rows, 2)
    ref, mag = R.epi_ss(y, m)
    chk.close("ss_rows y", f64(yg)[inside], y[inside], m[inside], c[inside])
    chk.close("ss_rows", f64(sg)[inside], ref[inside], mag[inside], (c[:, 0] + D)[inside])
    assert _untouched(yg, pre2, inside) and _untouched(sg, pre1, inside)

    fpre = _mixed_flags(n, inside)

    def normbwd():
        og, fo, cnt = pre2.clone().to(DEV), fpre.clone().to(DEV), torch.full((1,), 77, dtype=torch.int32, device=DEV)
        g.spmm_normbwd_sparse(o.Gg, in_flags, in_count, o.xrg, o.invg, o.dzg, S, og, fo, cnt, row_mask=mask)
        return og, fo, cnt
    og, fo, cnt = both(normbwd, 2)
    ref, mag = R.epi_normbwd(pg, pm, o.xr, o.inv, o.dz, S, o.clamped)
    chk.close("normbwd_sparse", f64(og)[inside], ref[inside], mag[inside], (c + D + 7)[inside])
    assert _untouched(og, pre2, inside)
    _check_out_flags(og, ref, mag, fo, cnt, inside, fpre)

    def axpy():
        og = pre2.clone().to(DEV)
        g.spmm_axpy_sparse(o.Gg, in_flags, in_count, o.bg, S, og, row_mask=mask)
        return (og,)
    (og,) = both(axpy)
    ref, mag = R.epi_axpy(pg, pm, o.b, S)
    chk.close("axpy_sparse", f64(og)[inside], ref[inside], mag[inside], (c + 1)[inside])
    assert _untouched(og, pre2, inside)

    def flags():
        og, fo, cnt = pre2.clone().to(DEV), fpre.clone().to(DEV), torch.full((1,), 77, dtype=torch.int32, device=DEV)
        g.spmm_flags(o.Gg, in_flags, in_count, og, fo, cnt, mask)
        return og, fo, cnt
    og, fo, cnt = both(flags, 2)
    chk.close("spmm_flags", f64(og)[inside], pg[inside], pm[inside], c[inside])
    assert _untouched(og, pre2, inside)
    _check_out_flags(og, pg, pm, fo, cnt, inside, fpre)

    # (the wrapper zero-fills the output and the flags outside the mask itself)
    def nbdot():
        og = pre2.clone().to(DEV)
        fo, cnt = OPS.spmm_normbwd_dot_sparse(g, o.Gg, (in_flags, in_count), o.xrg, o.invg, o.dzg, o.dotg, S, og, row_mask=mask)
        return og, fo, cnt
    og, fo, cnt = both(nbdot, 2)
    ref, mag = R.epi_normbwd_dot(pg, pm, o.xr, o.inv, o.dz, o.dot, S)
    chk.close("normbwd_dot_sparse", f64(og)[inside], ref[inside], mag[inside], (c + 6)[inside])
    assert float(og[dev(~inside)].abs().max() if (~inside).any() else 0.0) == 0.0
    _check_out_flags(og, ref, mag, fo, cnt, inside, torch.zeros(n, dtype=torch.uint8))
    chk.done()


# ===================================================================================================== flagged operands
def _flagged(lad, k, seed=3):
    """The first k columns of a fixed order that starts with the 40 designed columns F."""
    rng = np.random.default_rng(seed)
    rest = rng.permutation(np.setdiff1d(np.arange(lad.n_cols), lad.F))
    fl = np.zeros(lad.n_cols, np.uint8)
    fl[np.concatenate([lad.F, rest])[:k]] = 1
    return fl


def _flag_counts(n_cols):
    sw = int(0.8 * n_cols)
    return (0, 1, 3, 40, sw - 1, sw + 1, n_cols)


@pytest.mark.parametrize("ki", range(7))
@pytest.mark.parametrize("D", VEC_WIDTHS)
def test_flagged_operands(rect, D, ki):
    """in_flags on k operand rows (the others exactly zero): the un-masked kernels, on both sides of the 4/5 switch of the
    device counter, and with in_count None (flags always consulted) at the sparse counts.  k = 40 flags exactly F: the row `pat`
    and the head of the 1536-entry row hold batches with none / all / lane 0 / lane 63 / a handful of flagged entries."""
    lad = rect
    k = _flag_counts(lad.n_cols)[ki]
    chk = Chk(f"flagged operands D={D} k={k}")
    g, n = lad.g, lad.n_rows
    fl = _flagged(lad, k)
    assert 5 * (int(0.8 * lad.n_cols) - 1) < 4 * lad.n_cols <= 5 * (int(0.8 * lad.n_cols) + 1)      # the counts straddle the switch
    o = Ops(lad, D, seed=D)
    G = o.G.clone()
    G[torch.from_numpy(fl == 0)] = 0
    Gg = G.to(DEV)
    pg, pm = R.product(lad.rowptr, lad.col, lad.val, G)[:2]
    c = lad.c
    flg = dev(fl)
    everything = np.ones(n, bool)
    counters = [torch.full((1,), k, dtype=torch.int32, device=DEV)] + ([None] if k <= 40 else [])
    for cnt_in in counters:
        tag = "count" if cnt_in is not None else "always"
        def outs():
            return nan_like(n, D), torch.full((n,), 9, dtype=torch.uint8, device=DEV), torch.full((1,), 77, dtype=torch.int32, device=DEV)

        def flags():
            og, fo, cnt = outs()
            g.spmm_flags(Gg, flg, cnt_in, og, fo, cnt)
            return og, fo, cnt
        og, fo, cnt = twice(flags)
        chk.close(f"spmm_flags[{tag}]", og, pg, pm, c)
        if cnt_in is not None and 5 * k < 4 * lad.n_cols:
            # this side of the switch consults the flags: an unflagged row is not read, whatever it holds
            Gp = G.clone()
            Gp[torch.from_numpy(fl == 0)] = NAN
            op = nan_like(n, D)
            g.spmm_flags(Gp.to(DEV), flg, cnt_in, op, None, None)
            assert same_bits(op, og), "flags not consulted below 4/5"
        _check_out_flags(og, pg, pm, fo, cnt, everything, torch.zeros(n, dtype=torch.uint8))
        def normbwd():
            og, fo, cnt = outs()
            g.spmm_normbwd_sparse(Gg, flg, cnt_in, o.xrg, o.invg, o.dzg, S, og, fo, cnt)
            return og, fo, cnt
        og, fo, cnt = twice(normbwd)
        ref, mag = R.epi_normbwd(pg, pm, o.xr, o.inv, o.dz, S, o.clamped)
        chk.close(f"normbwd_sparse[{tag}]", og, ref, mag, c + D + 7)
        _check_out_flags(og, ref, mag, fo, cnt, everything, torch.zeros(n, dtype=torch.uint8))
        def axpy():
            og = nan_like(n, D)
            g.spmm_axpy_sparse(Gg, flg, cnt_in, o.bg, S, og)
            return (og,)
        (og,) = twice(axpy)
        ref, mag = R.epi_axpy(pg, pm, o.b, S)
        chk.close(f"axpy_sparse[{tag}]", og, ref, mag, c + 1)
    if k == 40:                                                          # the designed batches really are what the docstring says
        for row in (lad.special["pat"], lad.special[1536]):
            b = fl[lad.col[lad.rowptr[row]:lad.rowptr[row] + 320]].reshape(5, 64)
            assert b.sum(1).tolist() == [0, 64, 1, 1, 5] and b[2, 0] and b[3, 63]
    chk.done()


# ================================================================================================== the lane-grouped hop
@pytest.mark.parametrize("epi_flags", [False, True])
@pytest.mark.parametrize("which", ["F", "third"])
@pytest.mark.parametrize("D", VEC_WIDTHS)
def test_lane_grouped_hop(rect, D, which, epi_flags):
    """row_mask + in_flags + in_count None: D <= 128 runs spmm_rows_grouped_kernel (one row per lane group), D = 256 the masked
    one-wave-per-row kernel.  Flag sets: F (rows g0 .. g3 hold 0 - 3 flagged entries at their head -- the odd count is the
    t += 2 tail -- gmid three past the first 32, g40 forty in a row: more than any D / 4-entry batch holds) and a random third of
    the columns.  With dz_flags / b_flags the rows whose byte is 0 hold NaN in dz / x_raw / b: they are not read."""
    lad = rect
    chk = Chk(f"grouped hop D={D} flags={which} epi_flags={epi_flags}")
    g, n = lad.g, lad.n_rows
    fl = _flagged(lad, 40 if which == "F" else lad.n_cols // 3)
    rng = np.random.default_rng(11)
    inside = rng.random(n) < 0.7
    for key in ("g0", "g1", "g2", "g3", "g40", "gmid", "pat", 1025, 1536, HUB, 0, 1, 64):
        inside[lad.special[key]] = True
    inside[[lad.special[2049], lad.special[65]]] = False               # a long and a short row outside the mask
    mask = dev(inside.astype(np.uint8))
    o = Ops(lad, D, seed=D)
    G = o.G.clone()
    G[torch.from_numpy(fl == 0)] = NAN                                   # in_count None: unflagged rows may hold anything
    Gg = G.to(DEV)
    G0 = o.G.clone()
    G0[torch.from_numpy(fl == 0)] = 0
    pg, pm = R.product(lad.rowptr, lad.col, lad.val, G0)[:2]
    c = lad.c
    flg = dev(fl)
    pre2 = torch.full((n, D), NAN)
    ef = None
    xrg, dzg, bg = o.xrg, o.dzg, o.bg
    if epi_flags:
        ef = (rng.random(n) < 0.5).astype(np.uint8)
        off = dev(ef == 0)
        xrg, dzg, bg = o.xrg.clone(), o.dzg.clone(), o.bg.clone()
        xrg[off], dzg[off], bg[off] = NAN, NAN, NAN
    efg = dev(ef) if ef is not None else None
    fpre = _mixed_flags(n, inside)
    def hops():
        og, fo, cnt = pre2.clone().to(DEV), fpre.clone().to(DEV), torch.full((1,), 77, dtype=torch.int32, device=DEV)
        g.spmm_normbwd_sparse(Gg, flg, None, xrg, o.invg, dzg, S, og, fo, cnt, row_mask=mask, dz_flags=efg)
        ag = pre2.clone().to(DEV)
        g.spmm_axpy_sparse(Gg, flg, None, bg, S, ag, row_mask=mask, b_flags=efg)
        return og, fo, cnt, ag
    og, fo, cnt, ag = twice(hops)
    ref, mag = R.epi_normbwd(pg, pm, o.xr, o.inv, o.dz, S, o.clamped, b_flags=ef)
    chk.close("normbwd_sparse", f64(og)[inside], ref[inside], mag[inside], (c + D + 7)[inside])
    assert _untouched(og, pre2, inside)
    _check_out_flags(og, ref, mag, fo, cnt, inside, fpre)
    ref, mag = R.epi_axpy(pg, pm, o.b, S, b_flags=ef)
    chk.close("axpy_sparse", f64(ag)[inside], ref[inside], mag[inside], (c + 1)[inside])
    assert _untouched(ag, pre2, inside)
    if which == "F":
        heads = [int(fl[lad.col[lad.rowptr[lad.special[f"g{j}"]]:][:70]].sum()) for j in range(4)]
        assert heads == [0, 1, 2, 3] and fl[lad.col[lad.rowptr[lad.special["g40"]]:][:40]].all()
    chk.done()


# ======================================================================================= message dropout in the epilogue
def _check_drop_pattern(got, ref, kept, rows):
    """The zero pattern of a dropped output on `rows`: dropped elements are 0, kept ones are non-zero wherever the reference is."""
    g = got.cpu().numpy()[rows]
    assert (g[~kept[rows]] == 0).all()
    live = kept[rows] & (ref[rows] != 0)
    assert (g[live] != 0).all() and live.any()


@pytest.mark.parametrize("seed", [1, (2020 << 24) + 5])
@pytest.mark.parametrize("p", [0.1, 0.5, 0.999])
@pytest.mark.parametrize("D", VEC_WIDTHS)
def test_message_dropout_in_the_epilogue(square, D, p, seed):
    lad = square
    chk = Chk(f"epilogue dropout D={D} p={p} seed={seed}")
    g, n = lad.g, lad.n_rows
    o = Ops(lad, D, seed=D)
    y, m = lad.product(("X", D), o.X)
    pg, pm = lad.product(("G", D), o.G)
    kept, scale = R.drop_keep(n, D, p, seed)
    inside = _masks(lad)["random"]
    inside[lad.long] = True
    mask = dev(inside.astype(np.uint8))
    yd, md = y * kept * scale, m * kept * scale
    pre2, pre1 = torch.full((n, D), NAN), torch.full((n,), -7.0)
    for masked in (False, True):
        rows = inside if masked else np.ones(n, bool)
        def norm_acc():
            yg, ig, ag = pre2.clone().to(DEV), pre1.clone().to(DEV), o.acc0g.clone()
            if masked:
                g.spmm_norm_acc_rows(o.Xg, yg, ig, ag, S, mask, p, seed)
            else:
                g.spmm_norm_acc(o.Xg, yg, ig, ag, S, p, seed)
            return yg, ig, ag
        yg, ig, ag = twice(norm_acc)
        _check_drop_pattern(yg, y, kept, rows)                          # the zero pattern, exactly
        # + 1: the product with 1 / (1 - p)
        _check_norm_acc(chk, f"norm_acc[masked={masked}]", lad, D, yd, md, o.acc0, yg, ig, ag, rows=rows, c_extra=1)
        assert _untouched(yg, pre2, rows) and _untouched(ig, pre1, rows) and _untouched(ag, o.acc0, rows)
        def normbwd():
            og = pre2.clone().to(DEV)
            if masked:
                g.spmm_normbwd_sparse(o.Gg, None, None, o.xrg, o.invg, o.dzg, S, og, None, None, p, seed, row_mask=mask)
            else:
                g.spmm_normbwd(o.Gg, o.xrg, o.invg, o.dzg, S, og, p, seed)
            return (og,)
        (og,) = twice(normbwd)
        ref, mag = R.epi_normbwd(pg, pm, o.xr, o.inv, o.dz, S, o.clamped)
        _check_drop_pattern(og, ref, kept, rows)
        chk.close(f"normbwd[masked={masked}]", f64(og)[rows], (ref * kept * scale)[rows], (mag * kept * scale)[rows], (lad.c + D + 8)[rows])
        assert _untouched(og, pre2, rows)
    # masked + flagged + in_count None: the lane-grouped kernel up to D = 128, which applies the mask in its own epilogue
    fl = _flagged(lad, lad.n_cols // 3)
    G0 = o.G.clone()
    G0[torch.from_numpy(fl == 0)] = 0
    ref, mag = R.epi_normbwd(*R.product(lad.rowptr, lad.col, lad.val, G0)[:2], o.xr, o.inv, o.dz, S, o.clamped)
    def grouped():
        og, fo, cnt = pre2.clone().to(DEV), _mixed_flags(n, inside).to(DEV), torch.full((1,), 77, dtype=torch.int32, device=DEV)
        g.spmm_normbwd_sparse(G0.to(DEV), dev(fl), None, o.xrg, o.invg, o.dzg, S, og, fo, cnt, p, seed, row_mask=mask)
        return og, fo, cnt
    og, fo, cnt = twice(grouped)
    _check_drop_pattern(og, ref, kept, inside)
    chk.close("normbwd[grouped]", f64(og)[inside], (ref * kept * scale)[inside], (mag * kept * scale)[inside], (lad.c + D + 8)[inside])
    assert _untouched(og, pre2, inside)
    _check_out_flags(og, ref * kept, mag * kept, fo, cnt, inside, _mixed_flags(n, inside))
    chk.done()


# ========================================================================================== Adam folded into the last hop
def _adam_rowops(p, grad, m, v, lr, betas, eps, step):
    _lib.check(_lib.load().tagrec_adam_f32(_lib.ptr(p), _lib.ptr(grad), _lib.ptr(m), _lib.ptr(v), p.numel(), lr, betas[0], betas[1],
                                           eps, step, _lib.stream_ptr()), "adam")


@pytest.mark.parametrize("form", ["host", "device"])
@pytest.mark.parametrize("step", [1, 7])
@pytest.mark.parametrize("flagged", [False, True])
@pytest.mark.parametrize("D", VEC_WIDTHS)
def test_adam_folded_into_the_last_hop(square, D, flagged, step, form):
    """p, m, v of spmm_axpy_adam are the bits of spmm_axpy_sparse into a gradient buffer followed by the Adam kernel of rowops
    at the same step (the pinned roundings of csrc/common.h).  Both halves have their own fp64 parity: the product above,
    Adam in test_gpu_rowops.py."""
    lad = square
    g, n = lad.g, lad.n_rows
    lr, betas, eps = 0.01, (0.9, 0.999), 1e-8
    o = Ops(lad, D, seed=D)
    fl = bfl = None
    Gg, bg = o.Gg, o.bg
    if flagged:
        o.G[1::2] = 0                                                    # under 4/5 of the rows flagged: the flags are consulted
        Gg = o.G.to(DEV)
        fl = dev(R.row_flags(o.G))
        bf = (np.arange(n) % 3 != 0).astype(np.uint8)
        bfl = dev(bf)
        bg = o.bg.clone()
        bg[dev(bf == 0)] = NAN                                           # promised zero, never read
    cnt = fl.sum(dtype=torch.int32).reshape(1) if flagged else None
    p0 = R.randn(n, D, seed=D + 50).to(DEV)
    if step == 1:
        m0, v0 = torch.zeros_like(p0), torch.zeros_like(p0)
    else:
        m0, v0 = R.randn(n, D, seed=D + 51, scale=0.01).to(DEV), R.randn(n, D, seed=D + 52, scale=0.01).abs().to(DEV)
    grad = nan_like(n, D)
    g.spmm_axpy_sparse(Gg, fl, cnt, bg, S, grad, b_flags=bfl)
    pr, mr, vr = p0.clone(), m0.clone(), v0.clone()
    _adam_rowops(pr, grad, mr, vr, lr, betas, eps, step)
    pf, mf, vf = p0.clone(), m0.clone(), v0.clone()
    dev_state = None
    if form == "device":                                                 # as train.Adam(capturable=True) keeps it: the steps done so far
        dev_state = (torch.full((1,), step - 1, dtype=torch.int64, device=DEV), torch.zeros(2, dtype=torch.float32, device=DEV))
    g.spmm_axpy_adam(Gg, fl, cnt, bg, S, bfl, pf, mf, vf, lr, betas, eps, step, dev_state)
    torch.cuda.synchronize()
    if dev_state is not None:
        assert int(dev_state[0]) == step
    assert same_bits(mf, mr) and same_bits(vf, vr) and same_bits(pf, pr)
    assert not same_bits(pf, p0)
    print(f"[spmm] adam hop D={D} flagged={flagged} step={step} {form}: bit-identical to product + rowops Adam")


def test_a_refused_adam_hop_leaves_the_device_step_counter_alone():
    """The capturable form advances the device step counter only after every host-side check of the product has passed: a
    null graph handle (8 rows, D = 8, everything else valid) is refused as an invalid argument, the counter still reads 5
    and the factors, the parameters and the moments are untouched.  No product kernel is launched."""
    n, D = 8, 8
    Gg, bg = R.randn(n, D, seed=1).to(DEV), R.randn(n, D, seed=2).to(DEV)
    p0, m0, v0 = R.randn(n, D, seed=3).to(DEV), R.randn(n, D, seed=4, scale=0.01).to(DEV), R.randn(n, D, seed=5, scale=0.01).abs().to(DEV)
    p, m, v = p0.clone(), m0.clone(), v0.clone()
    step_dev = torch.full((1,), 5, dtype=torch.int64, device=DEV)
    coef0 = torch.tensor([0.25, 0.75], dtype=torch.float32, device=DEV)
    coef = coef0.clone()
    rc = _lib.load().tagrec_spmm_axpy_adam_graph_f32(None, Gg, None, None, bg, S, None, p, m, v, 0.01, 0.9, 0.999, 1e-8, step_dev, coef,
                                                     D, _lib.stream_ptr())
    torch.cuda.synchronize()
    assert rc == -1                                                      # TAGREC_E_INVALID
    assert "null graph handle" in _lib.load().tagrec_last_error().decode()
    assert int(step_dev) == 5 and same_bits(coef, coef0)
    assert same_bits(p, p0) and same_bits(m, m0) and same_bits(v, v0)


# ========================================================================================================== listed rows
def _listed_rows(lad, keys):
    rows = list(range(lad.n_rows)) + [lad.special[k] for k in keys]
    return np.random.default_rng(5).permutation(np.array(rows, np.int64))


@pytest.mark.parametrize("D", VEC_WIDTHS)
def test_listed_rows(rect, D):
    """Every row once, the hub three times more, the empty row and degrees 1, 2047, 2048, 2049 again (around the 32 x 64-entry
    split where per_split goes from 64 to 128), shuffled."""
    lad = rect
    chk = Chk(f"listed rows D={D}")
    rows = _listed_rows(lad, (HUB, HUB, HUB, 0, 1, 2047, 2048, 2049))
    o = Ops(lad, D, seed=D)
    y, m = lad.product(("X", D), o.X)
    rg = dev(rows)
    out = lad.g.spmm_listed(rg, o.Xg, nan_like(len(rows), D))
    assert same_bits(out, lad.g.spmm_listed(rg, o.Xg))
    # c = entries + the 4 waves of a range + the 32 ranges
    chk.close("spmm_listed", out, y[rows], m[rows], lad.deg[rows][:, None] + 36.0)
    empty = lad.g.spmm_listed(rg[:0], o.Xg)
    assert empty.shape == (0, D)
    chk.done()


# ================================================================================================ mark_rows / mark_cols
def test_mark_rows_and_mark_cols(rect, square):
    for lad, fn, self_too, n_flags in ((square, lambda r, f: square.g.mark_rows(r, f), True, square.n_rows),
                                       (rect, lambda r, f: OPS.mark_cols(rect.g, r, f), False, rect.n_cols)):
        for keys in ((), (0,), (31, 32, 33), (HUB, 0, 31, 32, 33, 33, HUB, 1, 513)):
            rows = np.array([lad.special[k] for k in keys], np.int64)
            pre = (np.arange(n_flags) % 5 == 0).astype(np.uint8) * 3      # bytes outside the expected set keep their value
            want = R.mark_rows(lad.rowptr, lad.col, rows, pre, self_too)
            got = torch.from_numpy(pre.copy()).to(DEV)
            fn(dev(rows), got)
            assert np.array_equal(got.cpu().numpy(), want), (lad.name, keys)
            assert (want != pre).any() == (len(keys) > 1 or (self_too and len(keys) == 1))      # the empty row marks itself at most
        # short ordinary rows, most of the graph's columns left alone
        rows = np.arange(200, 240, dtype=np.int64)
        pre = np.zeros(n_flags, np.uint8)
        got = torch.from_numpy(pre.copy()).to(DEV)
        fn(dev(rows), got)
        want = R.mark_rows(lad.rowptr, lad.col, rows, pre, self_too)
        assert np.array_equal(got.cpu().numpy(), want) and 0 < want.sum() < n_flags
    print("[spmm] mark_rows / mark_cols: exact")


# =================================================================================================== edge-dropout copies
@pytest.mark.parametrize("transposed", [False, True])
@pytest.mark.parametrize("p", [0.2, 0.9])
@pytest.mark.parametrize("D", [16, 64, 256])
def test_edge_dropout_copies(rect, D, p, transposed):
    """The edge-drop kernels against fp64 on the matrix masked by the numpy edge_kept and scaled by 1 / (1 - p), 1 - p taken
    in float32 as the kernels take it.  Every weight is divided once: c + 1."""
    seed = (2020 << 20) + 17
    lad = rect.t if transposed else rect
    chk = Chk(f"edge dropout {lad.name} D={D} p={p}")
    view = rect.g.edge_drop(p, seed)
    if transposed:
        view = view.transpose()
    assert view.shape == (lad.n_rows, lad.n_cols) and view.transposed == transposed
    keep = R.edge_kept(lad.rows_of, lad.col, p, seed, transposed)
    val = np.where(keep, f64(lad.val) / float(np.float32(1.0) - np.float32(p)), 0.0)
    assert 0 < keep.sum() < len(keep)
    n = lad.n_rows
    o = Ops(lad, D, seed=D)
    y, m = R.product(lad.rowptr, lad.col, val, o.X)[:2]
    c = lad.c + 1
    out = view.spmm(o.Xg, nan_like(n, D))
    assert same_bits(out, view.spmm(o.Xg))
    chk.close("spmm", out, y, m, c)
    inside = _masks(lad)["random"]
    inside[lad.long] = True
    mask = dev(inside.astype(np.uint8))
    pre2, pre1 = torch.full((n, D), NAN), torch.full((n,), -7.0)
    def norm_acc():
        yg, ig, ag = pre2.clone().to(DEV), pre1.clone().to(DEV), o.acc0g.clone()
        view.spmm_norm_acc_rows(o.Xg, yg, ig, ag, S, mask)
        return yg, ig, ag
    yg, ig, ag = twice(norm_acc)
    _check_norm_acc(chk, "norm_acc_rows", lad, D, y, m, o.acc0, yg, ig, ag, rows=inside, c_extra=1)
    assert _untouched(yg, pre2, inside) and _untouched(ig, pre1, inside) and _untouched(ag, o.acc0, inside)
    # backward hops: plain; masked with flags always consulted (the grouped edge-drop kernel up to D = 128)
    fl = _flagged(lad, lad.n_cols // 3) if lad.F is not None else (np.random.default_rng(3).random(lad.n_cols) < 0.33).astype(np.uint8)
    G0 = o.G.clone()
    G0[torch.from_numpy(fl == 0)] = 0
    pg0, pm0 = R.product(lad.rowptr, lad.col, val, G0)[:2]
    pg, pm = R.product(lad.rowptr, lad.col, val, o.G)[:2]
    for grouped in (False, True):
        rows = inside if grouped else np.ones(n, bool)
        a, am = (pg0, pm0) if grouped else (pg, pm)
        kw = dict(row_mask=mask) if grouped else {}
        Gg, flg = (G0.to(DEV), dev(fl)) if grouped else (o.Gg, None)
        def normbwd(drop_p=0.0, drop_seed=0):
            og, fo, cnt = pre2.clone().to(DEV), _mixed_flags(n, rows).to(DEV), torch.full((1,), 77, dtype=torch.int32, device=DEV)
            view.spmm_normbwd_sparse(Gg, flg, None, o.xrg, o.invg, o.dzg, S, og, fo, cnt, drop_p, drop_seed, **kw)
            return og, fo, cnt
        og, fo, cnt = twice(normbwd)
        ref, mag = R.epi_normbwd(a, am, o.xr, o.inv, o.dz, S, o.clamped)
        chk.close(f"normbwd_sparse[grouped={grouped}]", f64(og)[rows], ref[rows], mag[rows], (c + D + 7)[rows])
        _check_out_flags(og, ref, mag, fo, cnt, rows, _mixed_flags(n, rows))
        # message dropout of the gradient on top of the edge mask (the grouped edge-drop kernel applies it itself): + 1
        kept, scale = R.drop_keep(n, D, 0.5, seed + 1)
        dg, _, _ = twice(lambda: normbwd(0.5, seed + 1))
        _check_drop_pattern(dg, ref, kept, rows)
        chk.close(f"normbwd_sparse[grouped={grouped}, dropout]", f64(dg)[rows], (ref * kept * scale)[rows], (mag * kept * scale)[rows],
                  (c + D + 8)[rows])

        def axpy():
            ag2 = pre2.clone().to(DEV)
            view.spmm_axpy_sparse(Gg, flg, None, o.bg, S, ag2, **kw)
            return (ag2,)
        (ag2,) = twice(axpy)
        ref, mag = R.epi_axpy(a, am, o.b, S)
        chk.close(f"axpy_sparse[grouped={grouped}]", f64(ag2)[rows], ref[rows], mag[rows], (c + 1)[rows])
        assert _untouched(og, pre2, rows) and _untouched(ag2, pre2, rows) and _untouched(dg, pre2, rows)
    keys = (HUB, HUB, 0, 1, 2047, 2048, 2049) if not transposed else ()
    rows = np.concatenate([np.arange(n), np.array([rect.special[k] for k in keys], np.int64)])
    out = view.spmm_listed(dev(rows), o.Xg)
    assert same_bits(out, view.spmm_listed(dev(rows), o.Xg))
    chk.close("spmm_listed", out, y[rows], m[rows], lad.deg[rows][:, None] + 37.0)      # entries + 4 + 32, + 1 for the divide
    chk.done()


# ==================================================================================================== wrapper validation
def test_wrappers_refuse_bad_tensors(rect, square):
    """Every wrapper refuses, before any launch, a tensor of the wrong device, dtype, rank, row count, width or length."""
    D = 16
    g, n, nc = rect.g, rect.n_rows, rect.n_cols
    f32 = lambda *s: torch.zeros(*s, device=DEV)
    u8 = lambda k: torch.zeros(k, dtype=torch.uint8, device=DEV)
    i32 = lambda: torch.zeros(1, dtype=torch.int32, device=DEV)
    X, Y, inv, mask, fin = f32(nc, D), f32(n, D), f32(n), u8(n), u8(nc)
    rows = torch.zeros(4, dtype=torch.int64, device=DEV)
    bad2 = {"rows": f32(n - 1, D), "width": f32(n, D + 4), "dtype": torch.zeros(n, D, dtype=torch.float64, device=DEV), "rank": f32(n * D),
            "device": torch.zeros(n, D), "strided": f32(n, 2 * D)[:, :D]}
    bad_mask = {"length": u8(n + 1), "dtype": torch.zeros(n, dtype=torch.bool, device=DEV), "device": torch.zeros(n, dtype=torch.uint8),
                "rank": torch.zeros(n, 1, dtype=torch.uint8, device=DEV)}
    bad_fin = {"length": u8(nc - 1), "dtype": torch.zeros(nc, dtype=torch.int32, device=DEV)}
    bad_inv = {"length": f32(n + 3), "dtype": torch.zeros(n, dtype=torch.float64, device=DEV)}
    bad_cnt = {"dtype": torch.zeros(1, dtype=torch.int64, device=DEV), "empty": torch.zeros(0, dtype=torch.int32, device=DEV)}
    calls = []

    def both_forms(view):
        nonlocal calls
        for b in bad2.values():
            calls += [lambda b=b: view.spmm_norm_acc_rows(X, b, inv, Y, S, mask), lambda b=b: view.spmm_norm_acc_rows(X, Y, inv, b, S, mask),
                      lambda b=b: view.spmm_listed(rows, X, b),
                      lambda b=b: view.spmm_normbwd_sparse(X, fin, i32(), b, inv, Y, S, Y, None, None),
                      lambda b=b: view.spmm_normbwd_sparse(X, fin, i32(), Y, inv, b, S, Y, None, None),
                      lambda b=b: view.spmm_normbwd_sparse(X, fin, i32(), Y, inv, Y, S, b, None, None),
                      lambda b=b: view.spmm_axpy_sparse(X, fin, i32(), b, S, Y), lambda b=b: view.spmm_axpy_sparse(X, fin, i32(), Y, S, b)]
        for b in bad_mask.values():
            calls += [lambda b=b: view.spmm_norm_acc_rows(X, Y, inv, Y, S, b),
                      lambda b=b: view.spmm_normbwd_sparse(X, fin, i32(), Y, inv, Y, S, Y, None, None, row_mask=b),
                      lambda b=b: view.spmm_normbwd_sparse(X, fin, i32(), Y, inv, Y, S, Y, None, None, dz_flags=b),
                      lambda b=b: view.spmm_normbwd_sparse(X, fin, i32(), Y, inv, Y, S, Y, b, i32()),
                      lambda b=b: view.spmm_axpy_sparse(X, fin, i32(), Y, S, Y, row_mask=b),
                      lambda b=b: view.spmm_axpy_sparse(X, fin, i32(), Y, S, Y, b_flags=b)]
        for b in bad_fin.values():
            calls += [lambda b=b: view.spmm_normbwd_sparse(X, b, i32(), Y, inv, Y, S, Y, None, None),
                      lambda b=b: view.spmm_axpy_sparse(X, b, i32(), Y, S, Y)]
        for b in bad_inv.values():
            calls += [lambda b=b: view.spmm_norm_acc_rows(X, Y, b, Y, S, mask),
                      lambda b=b: view.spmm_normbwd_sparse(X, fin, i32(), Y, b, Y, S, Y, None, None)]
        for b in bad_cnt.values():
            calls += [lambda b=b: view.spmm_normbwd_sparse(X, fin, b, Y, inv, Y, S, Y, None, None),
                      lambda b=b: view.spmm_normbwd_sparse(X, fin, i32(), Y, inv, Y, S, Y, u8(n), b),
                      lambda b=b: view.spmm_axpy_sparse(X, fin, b, Y, S, Y)]
        calls += [lambda: view.spmm_listed(rows.int(), X), lambda: view.spmm_listed(rows.reshape(2, 2), X),
                  lambda: view.spmm_listed(rows, f32(nc - 1, D)), lambda: view.spmm_listed(rows.cpu(), X)]

    both_forms(g)
    both_forms(g.edge_drop(0.5, 3))
    for b in bad2.values():
        calls += [lambda b=b: g.spmm_rows(X, b, mask), lambda b=b: g.spmm_flags(X, fin, i32(), b, None)]
    for b in bad_mask.values():
        calls += [lambda b=b: g.spmm_rows(X, Y, b), lambda b=b: g.spmm_flags(X, fin, i32(), Y, b, i32()),
                  lambda b=b: g.spmm_flags(X, fin, i32(), Y, None, None, b)]
    for b in bad_fin.values():
        calls.append(lambda b=b: g.spmm_flags(X, b, i32(), Y, None))
    for b in bad_cnt.values():
        calls += [lambda b=b: g.spmm_flags(X, fin, b, Y, None), lambda b=b: g.spmm_flags(X, fin, i32(), Y, u8(n), b)]
    sq = square.g
    ns = square.n_rows
    for b in bad2.values():
        calls += [lambda b=b: g.spmm(X, b), lambda b=b: g.edge_drop(0.5, 3).spmm(X, b)]
    Xs, Ps = f32(ns, D), [f32(ns, D) for _ in range(4)]
    adam = lambda fl, cnt, bfl: sq.spmm_axpy_adam(Xs, fl, cnt, Ps[0], S, bfl, Ps[1], Ps[2], Ps[3], 0.01, (0.9, 0.999), 1e-8, 1)
    calls += [lambda: adam(u8(ns + 1), None, None), lambda: adam(torch.zeros(ns, dtype=torch.bool, device=DEV), None, None),
              lambda: adam(u8(ns), bad_cnt["dtype"], None), lambda: adam(None, None, u8(ns - 1)),
              lambda: adam(None, None, torch.zeros(ns, dtype=torch.int32, device=DEV))]
    calls += [lambda: sq.mark_rows(rows, u8(ns - 1)), lambda: sq.mark_rows(rows, torch.zeros(ns, dtype=torch.int32, device=DEV)),
              lambda: sq.mark_rows(rows.int(), u8(ns)), lambda: sq.mark_rows(rows, torch.zeros(ns, dtype=torch.uint8)),
              lambda: sq.mark_rows(rows.reshape(2, 2), u8(ns)), lambda: g.mark_rows(rows, u8(n)),
              lambda: sq.edge_drop(0.5, 3).mark_rows(rows, u8(ns + 1))]
    for call in calls:
        with pytest.raises(_lib.TagrecError):
            call()
    # and the well-formed calls go through
    g.spmm_rows(X, Y, mask)
    g.spmm_norm_acc_rows(X, Y, inv, None, S, None)
    g.spmm_flags(X, fin, i32(), Y, u8(n), i32(), mask)
    sq.mark_rows(rows, u8(ns))
    torch.cuda.synchronize()
    print(f"[spmm] wrapper refusals: {len(calls)} calls refused before launch")
