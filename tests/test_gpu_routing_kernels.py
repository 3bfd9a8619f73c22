"""GPU: every entry point of csrc/routing.hip -- the routed product with each epilogue, output selection, row class, row mask
and flagged-operand form, the score pass, the two softmaxes, the row sums, the permutation and the slice operations, at all
19 (D, K) instantiations -- each against the plain fp64 restatement of its own operation in tests/routing_ref.py (held to torch
autograd and the oracle by test_routing_ref_host.py).

Tolerance: the convention of test_gpu_spmm.py (spmm_ref.Chk): |got - ref64| <= c * 2^-24 * mag + extra + 1e-30, the counts `c`
those of the header of routing_ref.py, written beside each check (a long product row is held to two: stored entries + chunks,
and the depth of its lane tree, under which a lost partial sum of the hub cannot hide).  Permutations, "row untouched", the exact softmax cases and the
clamped 1e12 are exact; no element is left out of any comparison.  Every test prints its worst err / bound (`-s`); DESIGN section
2 carries the table.

Graphs: the rectangular ladder of test_gpu_spmm.py (2301 x 2999: degrees 0 ... 1024 | 1025 ... 2049 and a hub of 97 * 512 + 1 at
rows that are no multiple of 32, repeated column ids in the long rows), its RoutingGraph transpose (duplicates kept as separate
entries; column 2 is a long row) and a small symmetric graph with a hub of 1100 (the `symmetric` branch: only the permutation
is kept).  The weights of the products are signed with exact 0.0 and -0.0 entries; operand rows follow spmm_ref.norm_rows, so
exactly-zero and clamped (norm ~1e-13) product slices occur, and no slice norm lies near 1e-12 (asserted)."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import tagrec_amd as T
from tagrec_amd import _lib, rowops
from tagrec_amd import routing as RT

import routing_ref as RR
import spmm_ref as R
from spmm_ref import Chk as _Chk, U32, f64, same_bits
from test_gpu_routing import _random_symmetric_graph
from test_gpu_spmm import DEV, Ladder, _flag_counts, _flagged, build_ladder, dev, nan_like, twice

SHAPES = RR.SHAPES                                                       # all 19 ROUTE_CASE instantiations
SOME = tuple((D, K) for D in (16, 64, 256) for K in (1, 4, 8) if (D // 4) % K == 0)
assert len(SOME) == 8
B_SCALE = 0.25
INV_CLAMPED = float(R.INV_CLAMPED)


def Chk(name):
    chk = _Chk(name, tag="routing")
    chk.exact = []                                                       # (what, holds) of exact properties: asserted by _done
    return chk


def _done(chk):
    """Print and assert the worst err / bound first, then the exact properties collected on the way."""
    chk.done()
    for what, holds in chk.exact:
        assert holds, f"{chk.name}: {what}"


def _id(s):
    return f"D{s[0]}K{s[1]}"


# ============================================================================================================== graphs
class Routed:
    """A Ladder (host CSR + Graph), its RoutingGraph, the Ladder of the transposed structure and cached operands."""

    def __init__(self, lad):
        self.lad, self.rg = lad, RT.RoutingGraph(lad.g)
        self.perm = RR.host_perm(lad.rowptr, lad.col)
        rp, c, _ = R.transpose_csr(lad.rowptr, lad.col, lad.val, lad.n_cols)
        gt = self.rg.graph_t
        assert np.array_equal(gt.rowptr.cpu().numpy(), rp) and np.array_equal(gt.col.cpu().numpy(), c)
        self.t = Ladder(lad.name + "^T(dup)", rp, c, lad.val[self.perm], lad.n_rows, gt)
        self._w, self._x, self._ref = {}, {}, {}

    def w(self, K):
        """signed float32 weights [nnz, K] with exact 0.0 and -0.0 entries"""
        if K not in self._w:
            rng = np.random.default_rng(100 + K)
            w = (rng.uniform(0.05, 1.0, (len(self.lad.col), K)) * rng.choice([-1.0, 1.0], (len(self.lad.col), K))).astype(np.float32)
            w.reshape(-1)[7::23] = 0.0
            w.reshape(-1)[11::29] = -0.0
            w[5::97] = 0.0                                                 # whole entries too
            self._w[K] = (w, dev(w))
        return self._w[K]

    def x(self, n, D):
        """operand rows [n, D] after spmm_ref.norm_rows (1 mod 8: zero, 3 mod 8: norm 1e-13)"""
        if (n, D) not in self._x:
            x = R.norm_rows(n, D, seed=D)[0]
            self._x[n, D] = (x, x.to(DEV))
        return self._x[n, D]

    def epi(self, D, K):
        """post [n, K] (signed, 0.5 ... 1.5), self and B [n, D] ordinary, for the rows of the un-transposed graph"""
        n = self.lad.n_rows
        rng = np.random.default_rng(200 + K)
        post = torch.from_numpy((rng.uniform(0.5, 1.5, (n, K)) * rng.choice([-1.0, 1.0], (n, K))).astype(np.float32))
        return post, R.randn(n, D, seed=D + 1), R.randn(n, D, seed=D + 2)

    def product(self, D, K, transposed=False):
        """fp64 (A(w) x, magnitude) without epilogue, computed once per (D, K, side)."""
        key = (D, K, transposed)
        if key not in self._ref:
            lad = self.lad
            if transposed:
                y, m, _ = RR.transposed_product(lad.rowptr, lad.col, self.w(K)[0], self.x(lad.n_rows, D)[0], lad.n_cols)
            else:
                y, m = RR.routed_product(lad.rowptr, lad.col, self.w(K)[0], self.x(lad.n_cols, D)[0])
            self._ref[key] = (y, m)
        return self._ref[key]


@pytest.fixture(scope="module")
def rect():
    ro = Routed(build_ladder("rect", 2301, 2999, 1))
    assert not ro.rg.symmetric and ro.t.deg[2] > RR.K_LONG and ro.t.long.any()
    key = ro.t.rows_of * ro.lad.n_rows + ro.t.col
    assert len(np.unique(key)) < len(key)                                   # the transpose keeps duplicate entries
    return ro


@pytest.fixture(scope="module")
def sym():
    g, _, _ = _random_symmetric_graph(1500, 8, seed=5, hub=1100)
    lad = Ladder("sym", g.rowptr.cpu().numpy(), g.col.cpu().numpy(), g.val.cpu().numpy(), 1500, g)
    ro = Routed(lad)
    assert ro.rg.symmetric and ro.rg.graph_t is g and lad.long.any()
    return ro


# ======================================================================================================== direct calls
def _spmm(g, w, x, post=None, self_add=None, b=None, b_scale=0.0, raw=True, normed=False, row_mask=None, in_flags=None,
          in_count=None):
    """tagrec_route_spmm_ex_f32 into NaN-filled outputs -> (Y, Yn, inv)"""
    K, D, n = w.shape[1], x.shape[1], g.shape[0]
    y = nan_like(n, D) if raw else None
    yn = nan_like(n, D) if normed else None
    inv = nan_like(n, K) if normed else None
    _lib.check(_lib.load().tagrec_route_spmm_ex_f32(g.handle, _lib.ptr(w), K, _lib.ptr(x), _lib.ptr(post), _lib.ptr(self_add),
                                                    _lib.ptr(b), float(b_scale), _lib.ptr(y), _lib.ptr(yn), _lib.ptr(inv),
                                                    _lib.ptr(row_mask), _lib.ptr(in_flags), _lib.ptr(in_count), D,
                                                    _lib.stream_ptr()), "route_spmm")
    return y, yn, inv


def _score(g, H, Tt, logits, accumulate, row_mask=None):
    _lib.check(_lib.load().tagrec_route_score_rows_f32(g.handle, _lib.ptr(H), _lib.ptr(Tt), _lib.ptr(logits), logits.shape[1],
                                                       int(accumulate), _lib.ptr(row_mask), H.shape[1], _lib.stream_ptr()),
               "route_score")


def _present(outs):
    return tuple(t for t in outs if t is not None)


def _norm_ref(y, m, K):
    """slice normalisation of a product reference; every slice norm is zero, clamped well below 1e-12, or ordinary"""
    out = RR.slice_normalise(y, m, K)
    nrm = np.linalg.norm(RR._slices(y, K), axis=1)
    assert ((nrm < 0.7e-12) | (nrm > 1e-9)).all(), "a slice norm near the clamp"
    return out


def _check_product(chk, what, lad, K, got, y, m, c_epi, norm=None, rows=slice(None)):
    """(Y, Yn, inv) on `rows` against the product reference (y, m) with `c_epi` epilogue operations."""
    Y, Yn, inv = got
    c = lad.c + c_epi                                                    # stored entries + chunks + epilogue
    if Y is not None:
        chk.close(what + " y", f64(Y)[rows], y[rows], m[rows], c[rows])
        long = np.zeros(lad.n_rows, bool)
        long[rows] = True
        long &= lad.long
        if long.any():                                                   # the long rows, also to the depth of their lane tree
            ct = RR.tree_count(lad.deg, y.shape[1]) + c_epi
            chk.close(what + " y (long rows, tree depth)", f64(Y)[long], y[long], m[long], ct[long])
    if Yn is not None:
        (yn, ynm), (iv, ivm), clamped = norm if norm is not None else _norm_ref(y, m, K)
        dk = y.shape[1] // K
        # + D/K + 3: the slice's sum of squares, sqrtf, the float 1e-12, the divide
        chk.close(what + " yn", f64(Yn)[rows], yn[rows], ynm[rows], (c + dk + 3)[rows])
        chk.close(what + " inv", f64(inv)[rows], iv[rows], ivm[rows], (c + dk + 3)[rows])
        at_clamp = inv.cpu().numpy()[rows][clamped[rows]]
        chk.exact.append((what + ": inv == 1e12 on every clamped slice", bool((at_clamp == R.INV_CLAMPED).all())))
        return clamped
    return None


# ===================================================================================== the product: every shape and form
@pytest.mark.parametrize("shape", SHAPES, ids=_id)
def test_routed_product_every_shape(rect, shape):
    D, K = shape
    lad, g = rect.lad, rect.lad.g
    chk = Chk(f"routed product D={D} K={K}")
    # the hub row makes every lane group of route_spmm_finish_kernel take the 4-way unrolled loop (k + 3 NPI < nc for
    # k = 0 ... NPI - 1) and the single-step tail after it
    npi, nc = 256 // D, int(lad.chunks.max())
    assert nc >= 4 * npi and nc % (4 * npi) != 0
    (w, wg), (x, xg) = rect.w(K), rect.x(lad.n_cols, D)
    assert (w == 0).any() and np.signbit(w[w == 0]).any() and (w < 0).any()
    post, self_add, b = rect.epi(D, K)
    y0, m0 = rect.product(D, K)
    forms = {"none": {}, "post": {"post": post}, "full": {"post": post, "self_add": self_add, "b": b, "b_scale": B_SCALE}}
    for name, epi in forms.items():
        y, m = RR.epilogue(y0, m0, K, **epi)
        norm = _norm_ref(y, m, K)
        c_epi = RR.epilogue_count(epi.get("post"), epi.get("self_add"), epi.get("b"))
        on_dev = {k: (v.to(DEV) if isinstance(v, torch.Tensor) else v) for k, v in epi.items()}
        for raw, normed in ((True, False), (False, True), (True, True)):
            got = twice(lambda: _present(_spmm(g, wg, xg, raw=raw, normed=normed, **on_dev)))
            got = (got[0] if raw else None,) + (tuple(got[-2:]) if normed else (None, None))
            clamped = _check_product(chk, f"{name}[raw={raw}, normed={normed}]", lad, K, got, y, m, c_epi, norm)
        if name != "full":                                               # exactly-zero and clamped non-zero slices exist
            nrm = np.linalg.norm(RR._slices(y, K), axis=1).reshape(-1, K)
            assert (nrm == 0).any() and (clamped & (nrm > 0)).any() and not clamped.all()
        # the wrapper allocates its own outputs: the same bits
        wy, wyn, winv = rect.rg.spmm(wg, xg, raw=True, normed=True, **on_dev)
        assert same_bits(wy, got[0]) and same_bits(wyn, got[1]) and same_bits(winv, got[2])
    _done(chk)


# ============================================================================================== the transposed product
@pytest.mark.parametrize("which", ["rect", "sym"])
@pytest.mark.parametrize("shape", SOME, ids=_id)
def test_routed_product_transposed(rect, sym, shape, which):
    D, K = shape
    ro = rect if which == "rect" else sym
    lad, lt, rg = ro.lad, ro.t, ro.rg
    chk = Chk(f"transposed product {lad.name} D={D} K={K}")
    (w, wg), (x, xg) = ro.w(K), ro.x(lad.n_rows, D)
    assert same_bits(rg.perm.cpu(), torch.from_numpy(ro.perm.astype(np.int32)))
    wt = rg.permute(wg)
    assert same_bits(wt.cpu(), torch.from_numpy(w[ro.perm]))
    if which == "sym":                                                   # the transposed structure IS the structure
        assert np.array_equal(lt.rowptr, lad.rowptr) and np.array_equal(lt.col, lad.col)
    y, m = ro.product(D, K, transposed=True)
    got = twice(lambda: _present(_spmm(rg.graph_t, wt, xg, raw=True, normed=True)))
    _check_product(chk, "A(w)^T x", lt, K, got, y, m, 0)
    wy, wyn, winv = rg.spmm(wg, xg, raw=True, normed=True, transposed=True)
    assert same_bits(wy, got[0]) and same_bits(wyn, got[1]) and same_bits(winv, got[2])
    # with `post` on the transposed side's rows
    rng = np.random.default_rng(300 + K)
    post = torch.from_numpy((rng.uniform(0.5, 1.5, (lt.n_rows, K)) * rng.choice([-1.0, 1.0], (lt.n_rows, K))).astype(np.float32))
    yp, mp = RR.epilogue(y, m, K, post=post)
    (gy,) = twice(lambda: _present(_spmm(rg.graph_t, wt, xg, post=post.to(DEV))))
    _check_product(chk, "post * A(w)^T x", lt, K, (gy, None, None), yp, mp, 1)
    wy, _, _ = rg.spmm(wg, xg, post=post.to(DEV), transposed=True)
    assert same_bits(wy, gy)
    _done(chk)


# =========================================================================================================== row masks
def _row_masks(lad):
    third = (np.arange(lad.n_rows) % 3 == 0) | lad.long
    return {"all": np.ones(lad.n_rows, bool), "none": np.zeros(lad.n_rows, bool), "third+long": third, "short": ~lad.long}


@pytest.mark.parametrize("kind", ["all", "none", "third+long", "short"])
@pytest.mark.parametrize("shape", SOME, ids=_id)
def test_row_mask_leaves_other_rows_untouched(rect, shape, kind):
    D, K = shape
    lad, g = rect.lad, rect.lad.g
    chk = Chk(f"row mask D={D} K={K} mask={kind}")
    inside = _row_masks(lad)[kind]
    outside = torch.from_numpy(~inside).to(DEV)
    mask = dev(inside.astype(np.uint8))
    (w, wg), (x, xg) = rect.w(K), rect.x(lad.n_cols, D)
    post, self_add, b = rect.epi(D, K)
    y, m = RR.epilogue(*rect.product(D, K), K, post=post, self_add=self_add, b=b, b_scale=B_SCALE)
    got = twice(lambda: _spmm(g, wg, xg, post=post.to(DEV), self_add=self_add.to(DEV), b=b.to(DEV), b_scale=B_SCALE, raw=True,
                              normed=True, row_mask=mask))
    if inside.any():
        _check_product(chk, "masked product", lad, K, got, y, m, 3, rows=inside)
    for t in got:                                                        # NaN pre-fill: the rows outside keep its bits
        assert same_bits(t[outside], torch.full_like(t, float("nan"))[outside])
    # the score pass under the same mask: the entries of masked-out rows (long rows' chunks included) keep their bits
    H, Tt = R.randn(lad.n_rows, D, seed=D + 3), R.randn(lad.n_cols, D, seed=D + 4)
    Hg, Tg = H.to(DEV), Tt.to(DEV)
    ein = inside[lad.rows_of]
    eout = torch.from_numpy(~ein).to(DEV)
    sref, smag = RR.score(lad.rowptr, lad.col, H, Tt, K)

    def write():
        lg = nan_like(len(lad.col), K)
        _score(g, Hg, Tg, lg, False, mask)
        return (lg,)
    (lg,) = twice(write)
    if ein.any():
        chk.close("masked score", f64(lg)[ein], sref[ein], smag[ein], D // K)
    assert same_bits(lg[eout], torch.full_like(lg, float("nan"))[eout])
    prior = lg.clone()
    _score(g, Hg, Tg, lg, True, mask)
    if ein.any():
        chk.close("masked score +=", f64(lg)[ein], sref[ein] + f64(prior)[ein], smag[ein] + np.abs(f64(prior)[ein]), D // K + 1)
    assert same_bits(lg[eout], prior[eout])
    if kind == "short":
        assert (~ein).sum() == lad.deg[lad.long].sum() > 0
    _done(chk)


# ================================================================================================ flagged operand rows
@pytest.mark.parametrize("ki", range(7))
@pytest.mark.parametrize("shape", SOME, ids=_id)
def test_flagged_operand_rows(rect, shape, ki):
    """x with k non-zero rows, k on both sides of the 5 count < 4 n_cols switch: the wrapper's sparse_x and direct calls with
    the flags of rowops.row_flags, all to one fp64 reference; below the switch the unflagged rows are not read."""
    D, K = shape
    lad, g = rect.lad, rect.lad.g
    k = _flag_counts(lad.n_cols)[ki]
    sw = int(0.8 * lad.n_cols)
    assert 5 * (sw - 1) < 4 * lad.n_cols <= 5 * (sw + 1)                     # the counts straddle the switch
    chk = Chk(f"flagged operand rows D={D} K={K} k={k}")
    fl = _flagged(lad, k)
    x = R.randn(lad.n_cols, D, seed=D + 5)
    x[torch.from_numpy(fl == 0)] = 0
    xg = x.to(DEV)
    w, wg = rect.w(K)
    flags, count = rowops.row_flags(xg)
    assert np.array_equal(flags.cpu().numpy(), fl) and int(count.item()) == k
    y, m = RR.routed_product(lad.rowptr, lad.col, w, x)
    norm = _norm_ref(y, m, K)
    got = twice(lambda: _spmm(g, wg, xg, raw=True, normed=True, in_flags=flags, in_count=count))
    _check_product(chk, "flags + count", lad, K, got, y, m, 0, norm)
    plain = _spmm(g, wg, xg, raw=True, normed=True)
    _check_product(chk, "no flags", lad, K, plain, y, m, 0, norm)
    wy, wyn, winv = rect.rg.spmm(wg, xg, raw=True, normed=True, sparse_x=True)
    assert same_bits(wy, got[0]) and same_bits(wyn, got[1]) and same_bits(winv, got[2])
    if 5 * k < 4 * lad.n_cols:                                           # flags consulted: an unflagged row is not read
        xp = x.clone()
        xp[torch.from_numpy(fl == 0)] = float("nan")
        poisoned = _spmm(g, wg, xp.to(DEV), raw=True, normed=True, in_flags=flags, in_count=count)
        assert all(same_bits(s, t) for s, t in zip(poisoned, got)), "flags not consulted below 4/5"
    if ki == 0:
        with pytest.raises(_lib.TagrecError, match="go together"):
            _spmm(g, wg, xg, in_flags=flags)
        with pytest.raises(_lib.TagrecError, match="go together"):
            _spmm(g, wg, xg, in_count=count)
    _done(chk)


# ============================================================================================================== scores
@pytest.mark.parametrize("shape", SHAPES, ids=_id)
def test_scores_every_shape(rect, shape):
    D, K = shape
    lad, rg = rect.lad, rect.rg
    chk = Chk(f"scores D={D} K={K}")
    H, Tt = R.randn(lad.n_rows, D, seed=D + 3), R.randn(lad.n_cols, D, seed=D + 4)       # H != T, and of different heights
    Hg, Tg = H.to(DEV), Tt.to(DEV)
    sref, smag = RR.score(lad.rowptr, lad.col, H, Tt, K)

    def write():
        lg = nan_like(len(lad.col), K)
        rg.score(Hg, Tg, lg, accumulate=False)
        return (lg,)
    (lg,) = twice(write)
    chk.close("write", lg, sref, smag, D // K)                           # the slice dot: D/K (finite: every entry overwritten)
    prior = lg.clone()
    rg.score(Hg, Tg, lg, accumulate=True)
    # + 1: the addition to what was there; the prior value joins the magnitude
    chk.close("accumulate", lg, sref + f64(prior), smag + np.abs(f64(prior)), D // K + 1)
    _done(chk)


# =================================================================================== factor softmax, row sums, permutation
@pytest.mark.parametrize("K", [1, 2, 4, 8])
def test_factor_softmax_rowsum_permute(rect, K):
    lad, rg = rect.lad, rect.rg
    nnz = len(lad.col)
    assert nnz % 256 != 0
    chk = Chk(f"factor softmax / rowsum K={K}")
    rng = np.random.default_rng(400 + K)
    spread = np.array([0.5, 5.0, 80.0])[np.arange(nnz) % 3][:, None]
    logits = (rng.uniform(-1.0, 1.0, (nnz, K)) * spread).astype(np.float32)
    logits[0] = -80.0
    logits[0, K - 1] = 80.0                                              # the others underflow: exactly 1 and 0
    logits[nnz - 1] = 3.25                                               # all equal: exactly 1 / K
    got = nan_like(nnz, K)
    _lib.check(_lib.load().tagrec_route_softmax_f32(_lib.ptr(dev(logits)), _lib.ptr(got), nnz, K, _lib.stream_ptr()), "route_softmax")
    ref, mag, extra = RR.route_softmax(logits)
    chk.close("route_softmax", got, ref, mag, K + 16, extra)             # l - max in extra; expf 8, the sum 8 + K - 1, the divide
    gh = got.cpu().numpy()
    assert gh[0, K - 1] == 1.0 and (np.delete(gh[0], K - 1) == 0).all() and (gh[nnz - 1] == 1.0 / K).all()
    if K == 1:
        assert (gh == 1.0).all()
    assert same_bits(rg.softmax(dev(logits)), got)

    # row sums: positive weights, an empty row and a row whose weights are all exactly 0 -> exactly 0
    w = rng.uniform(0.05, 1.0, (nnz, K)).astype(np.float32)
    zero_row, empty_row = lad.special[31], lad.special[0]
    w[lad.rowptr[zero_row]:lad.rowptr[zero_row + 1]] = 0.0
    d = nan_like(lad.n_rows, K)
    _lib.check(_lib.load().tagrec_route_rowsum_rsqrt_f32(lad.g.handle, _lib.ptr(dev(w)), K, _lib.ptr(d), _lib.stream_ptr()), "rowsum")
    ref, mag = RR.rowsum_rsqrt(lad.rowptr, w)
    chk.close("rowsum_rsqrt", d, ref, mag, RR.rowsum_count(lad.deg))
    dh = d.cpu().numpy()
    assert lad.deg[empty_row] == 0 and (dh[lad.deg == 0] == 0).all() and (dh[zero_row] == 0).all()
    assert all(lad.deg[lad.special[k]] == k for k in (1025, 2049)) and lad.deg.max() == 97 * 512 + 1
    assert same_bits(rg.rowsum_rsqrt(dev(w)), d)

    # the permutation is a copy
    assert same_bits(rg.permute(dev(w)).cpu(), torch.from_numpy(w[rect.perm]))
    _done(chk)


# ========================================================================================================== row softmax
@pytest.mark.parametrize("spread", [2.0, 80.0])
def test_row_softmax_fwd_bwd(rect, spread):
    lad, rg = rect.lad, rect.rg
    nnz = len(lad.col)
    chk = Chk(f"row softmax spread={spread}")
    rng = np.random.default_rng(500)
    logits = rng.uniform(-spread, spread, nnz).astype(np.float32)
    lg = dev(logits)
    a = nan_like(nnz)
    _lib.check(_lib.load().tagrec_row_softmax_fwd_f32(lad.g.handle, _lib.ptr(lg), _lib.ptr(a), _lib.stream_ptr()), "row_softmax_fwd")
    ref, mag, extra = RR.row_softmax(lad.rowptr, logits)
    c_fwd, c_bwd = RR.row_softmax_count(lad.deg)
    chk.close("forward", a, ref, mag, c_fwd, extra)                      # the row's sum tree + 17
    single = lad.rowptr[lad.special[1]]
    assert lad.deg[lad.special[1]] == 1 and float(a[single]) == 1.0 and (lad.deg == 0).any()
    assert same_bits(rg.row_softmax(lg), a)
    da = rng.standard_normal(nnz).astype(np.float32)
    dl = nan_like(nnz)
    _lib.check(_lib.load().tagrec_row_softmax_bwd_f32(lad.g.handle, _lib.ptr(a), _lib.ptr(dev(da)), _lib.ptr(dl), _lib.stream_ptr()),
               "row_softmax_bwd")
    ref, mag = RR.row_softmax_bwd(lad.rowptr, a, da)                      # fed the kernel's own a
    chk.close("backward", dl, ref, mag, c_bwd)                           # the row's dot tree + 2
    assert float(dl[single]) == 0.0
    assert same_bits(rg.row_softmax_bwd(a, dev(da)), dl)
    _done(chk)


# ============================================================================================================ slice ops
def _slice_call(fn, *args):
    _lib.check(fn(*args, _lib.stream_ptr()), "slice op")


@pytest.mark.parametrize("shape", SHAPES, ids=_id)
def test_slice_ops_every_shape(shape):
    D, K = shape
    dk = D // K
    lib = _lib.load()
    chk = Chk(f"slice ops D={D} K={K}")
    worst_tanh = 0.0
    for n in (1, 63, 777):
        assert (n * D // 4) % 256 != 0
        xs, dzs, clamped = R.norm_rows(n * K, dk, seed=D + K + n)           # by SLICE: zero, 1e-13, zero dz, -0.0 dz
        x, dz, clamped = xs.reshape(n, D), dzs.reshape(n, D), clamped.reshape(n, K)
        xg, dzg = x.to(DEV), dz.to(DEV)
        p = R.randn(n, K, seed=D + n)
        y = nan_like(n, D)
        _slice_call(lib.tagrec_slice_scale_f32, _lib.ptr(xg), _lib.ptr(p.to(DEV)), _lib.ptr(y), n, D, K)
        chk.close(f"scale n={n}", y, *RR.slice_scale(x, p), 1)           # one product
        assert same_bits(RT.slice_scale(xg, p.to(DEV)), y)

        c_norm = dk / 2 + 3                                              # sum of squares halved, sqrtf, the float eps, the divide
        outs = {}
        for tanh in (False, True):
            (ref, mag, slope), (iref, imag) = RR.slice_norm_fwd(x, K, tanh=tanh)
            for want_inv in (True, False):
                y, inv = nan_like(n, D), (nan_like(n, K) if want_inv else None)
                _slice_call(lib.tagrec_slice_norm_fwd_f32, _lib.ptr(xg), _lib.ptr(y), _lib.ptr(inv), n, D, K, int(tanh))
                outs[tanh, want_inv] = y
                if tanh:                                                 # tanhf's own TANH_ULP ulp; the norm's count through the slope
                    chk.close(f"norm+tanh n={n}", y, ref, mag, 2 * RR.TANH_ULP, c_norm * U32 * slope)
                else:
                    chk.close(f"norm n={n}", y, ref, mag, c_norm)
                if want_inv:
                    chk.close(f"inv n={n}", inv, iref, imag, c_norm)
                    assert (inv.cpu().numpy()[clamped] == R.INV_CLAMPED).all()
            assert same_bits(outs[tanh, True], outs[tanh, False])
        wy, winv = RT.slice_norm_fwd(xg, K, tanh=True)
        assert same_bits(wy, outs[True, True])
        # tanhf alone: the kernel's tanh output against fp64 tanh of the kernel's own normalised float, in ulps of the result
        z32, t32 = f64(outs[False, True]), f64(outs[True, True])
        t64 = np.tanh(z32)
        ulp = np.abs(t32 - t64) / np.spacing(np.abs(t64).astype(np.float32)).astype(np.float64)
        worst_tanh = max(worst_tanh, float(ulp.max()))

        inv32 = torch.from_numpy(R.inv_norm(xs)[0].astype(np.float32).reshape(n, K))
        assert (inv32.numpy()[clamped] == R.INV_CLAMPED).all() and (inv32.numpy()[~clamped] < 1e6).all()
        dx = nan_like(n, D)
        _slice_call(lib.tagrec_slice_norm_bwd_f32, _lib.ptr(xg), _lib.ptr(inv32.to(DEV)), _lib.ptr(dzg), _lib.ptr(dx), n, D, K)
        chk.close(f"norm_bwd n={n}", dx, *RR.slice_norm_bwd(x, inv32, dz, K), dk + 6)
        assert same_bits(RT.slice_norm_bwd(xg, inv32.to(DEV), dzg), dx)
        if n * K >= 8:
            tiny = clamped & (np.linalg.norm(f64(xs), axis=1).reshape(n, K) > 0)
            assert tiny.any() and (clamped & ~tiny).any() and not clamped.all()
    print(f"[routing] tanhf D={D} K={K}: worst error {worst_tanh:.3f} ulp (allowed {RR.TANH_ULP})")
    _done(chk)


# ================================================================================================= one slab, many widths
def test_slab_regrows_across_widths(rect):
    """One fresh handle: row sums at width 1, the D = 256 product, row sums at width 8, the D = 16 product -- the long rows'
    partial sums of every width go through the same slab."""
    lad = rect.lad
    chk = Chk("slab across widths")
    g = T.Graph(dev(lad.rowptr), dev(lad.col, torch.int32), dev(lad.val), (lad.n_rows, lad.n_cols))
    fresh = Ladder("rect(fresh)", lad.rowptr, lad.col, lad.val, lad.n_cols, g)
    rng = np.random.default_rng(600)

    def rowsum(K):
        w = rng.uniform(0.05, 1.0, (len(lad.col), K)).astype(np.float32)
        d = nan_like(lad.n_rows, K)
        _lib.check(_lib.load().tagrec_route_rowsum_rsqrt_f32(g.handle, _lib.ptr(dev(w)), K, _lib.ptr(d), _lib.stream_ptr()), "rowsum")
        chk.close(f"rowsum K={K}", d, *RR.rowsum_rsqrt(lad.rowptr, w), RR.rowsum_count(lad.deg))

    def product(D, K):
        got = _spmm(g, rect.w(K)[1], rect.x(lad.n_cols, D)[1], raw=True, normed=True)
        _check_product(chk, f"product D={D} K={K}", fresh, K, got, *rect.product(D, K), 0)

    rowsum(1)
    product(256, 8)
    rowsum(8)
    product(16, 4)
    _done(chk)
