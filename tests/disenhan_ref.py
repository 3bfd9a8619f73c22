"""Plain fp64 restatements of the DisenHAN kernels of csrc/disenhan.hip and the hand-placed inputs they are tried on, shared
by test_gpu_disenhan_kernels.py and test_disenhan_ref_host.py (which holds them to fp64 torch autograd of
tests/disenhan_torch.py and asserts that the inputs hold the edges named below).  numpy / torch on the CPU; no project code.

Layout as in the kernels: embeddings [n, D] with factor k in columns [k dk, (k + 1) dk), dk = D / K; per-node per-factor
[n, K]; per-entry [nnz] in CSR entry order.  Every reference takes the kernel's OWN inputs -- for a backward pass the fp32
alpha, Yl, Z, r, x, inv the kernel was given -- and returns (ref, mag) pairs for the rule of spmm_ref.py,

    |got - ref64| <= c * 2^-24 * mag + extra + 1e-30,

mag the sum of the absolute values of the terms that are added.  Where a kernel forms an output from a value it has just
stored (g, dZt, x, dx: the register it goes on with is the float it wrote), the reference of what follows may be given that
stored float (`g=`, `dZt=`, `x=`, `dx=`): the stored value is held to its own reference, and what is formed from it to the
short count of its own operations, under which a lost term cannot hide behind the error of the value it came from.  Left
out (the host test), everything follows from the inputs in fp64.

The counts `c`, read off the kernels (u = 2^-24; an fma rounds once; tree(len) = ceil(len / 64) + 6: a lane adds its entries
j, j + 64, ... in turn, then the 6-step butterfly of the wavefront):

  edge_softmax_fwd
    logit          sL + sR (1), K fmas, the product with mult: K + 2 on lmag = mult sum_k |r_k| relu(sL + sR).  fl(a + b) has
                   the sign of a + b, so the gates agree with fp64 exactly.  The logits are not an output (they pass through
                   `alpha`); their absolute error e = (K + 2) u lmag enters alpha's `extra`.
    alpha          expf of the numerator (4 ulp = 8), the row sum of terms carrying expf's 8 through tree(deg), the divide:
                   tree(deg) + 17 on mag = alpha itself.  extra = alpha_j (da_j + sum_row alpha da), da_j = e_j + e_max(row)
                   + u |logit_j - max|: the logit's own error, the row maximum's, and the rounding of the subtraction.
  edge_softmax_bwd
    g              the dot alpha . dalpha by fmas in the same tree (tree(deg)), the subtraction, two products: tree(deg) + 3 on
                   mult |alpha| (|dalpha| + sum_row |alpha dalpha|).
    dr             from the stored g: sL + sR (1), fmas through the row's tree: tree(deg) + 1 on sum_j |g_j| relu(sL + sR).
    dsL            from the stored g: fmas through the row's tree: tree(deg) on sum_j |g_j r_k| over the open gates.
    dsR            the column pass reads g from memory: fmas through the tree of the transposed row: tree(cdeg).
  rel_epi_fwd
    Yl             the product with the slope and the float 0.2f (0.25 u off 0.2): 2.
    Z              dk fmas of Yl (2): dk + 2 on sum_d |Yl_d W_dc|.
    r              the factor softmax: s - max (1, through the slope: extra), expf 8, the sum of K such terms (8 + K - 1), the
                   divide: K + 16 on r itself.  extra = r_k (da_k + sum_i r_i da_i), da_k = ds_k + u |s_k - max| with the
                   absolute error of the score s_k = sum_c tanh(Z_c) q_c:
                   ds_k = u [ (dk + 2) sum_c |q_c| (1 - tanh^2) Zmag_c  +  (2 TANH_ULP + 1 + dk) sum_c |tanh(Z_c) q_c| ]
                   -- Z's error through tanh's slope; tanhf (routing_ref.TANH_ULP ulp), the product, the in-order slice sum.
  rel_epi_bwd      (inputs Yl, Z, r as stored by the forward)
    ds_k           sum r dr by K fmas, the subtraction, the product: K + 2 on |r_k| (|dr_k| + sum |r dr|).
    dZt            1 - th^2: th carries tanhf's 2 TANH_ULP twice and the square (13 on th^2), the subtraction: 14 on 1 + th^2 --
                   where tanh saturates the difference cancels and the bound does not shrink with it; ds_k (K + 2), two
                   products, the addition to dZ: K + 19 on |dZ| + dsmag |q| (1 + th^2).  dr NULL: dZt = dZ, exact.
    dsT            ds_k (K + 2), tanhf (2 TANH_ULP), the product: K + 2 TANH_ULP + 3.
    dY             from the stored dZt: dk fmas, the product with the slope and the float 0.2f: dk + 2.
    dW, dq         host-side sums over the n K slices in an order the BLAS chooses: a term passes at most n K rounded
                   operations whatever the order: n K on |Yl|^T |dZt| and on the column sums of |dsT|.
  combine_fwd
    x              the two products and the two additions; a term passes at most 3: 3.
    y, inv         from the stored x: dk squares and their in-order sum halved by the square root (dk / 2 + 1/2), sqrtf, the
                   float 1e-12f, the divide: dk / 2 + 3 (the count of routing_ref's slice_norm_fwd).
  combine_bwd      (inputs x, inv as stored by the forward)
    dx             z = x inv (1), the dot (dk), z dot (1), the subtraction, the product with inv, 1 spare: dk + 6 (the count
                   of routing_ref's slice_norm_bwd); the dot is dropped where inv >= 1e12f.
    dZ_e           from the stored dx: one product: 1.
    dr_e           from the stored dx: the product and the in-order slice sum: dk + 1."""
import functools

import numpy as np
import torch

import routing_ref as RR
import spmm_ref as R
from spmm_ref import U32, f64

TANH_ULP = RR.TANH_ULP
SLOPE = 0.2
SHAPES = tuple((D, K) for D in (16, 32, 64, 128, 256) for K in (1, 2, 4, 8))     # every pair dh_row_shape_ok accepts
MAX_GROUPS = 4096                      # dh_row_blocks: the grid of a row pass is capped at this many groups of 256 / D rows


def tree(deg):
    """rounded additions a term passes in a wavefront's sum over `deg` entries"""
    return -(-np.asarray(deg, np.int64) // 64) + 6


def _rows_of(rowptr):
    return RR._rows_of(rowptr)


def _row_sum(rows, n, v):
    out = np.zeros((n,) + v.shape[1:])
    np.add.at(out, rows, v)
    return out


# ===================================================================================================== edge softmax
def edge_softmax_fwd(rowptr, col, mult, sL, sR, r):
    """-> (alpha, mag, extra), (logit, lmag)"""
    rowptr, col = np.asarray(rowptr, np.int64), np.asarray(col, np.int64)
    mult, sL, sR, r = f64(mult), f64(sL), f64(sR), f64(r)
    rows, n, K = _rows_of(rowptr), len(rowptr) - 1, sL.shape[1]
    t = r[rows] * np.maximum(sL[rows] + sR[col], 0.0)
    logit, lmag = mult * t.sum(1), mult * np.abs(t).sum(1)
    e = (K + 2) * U32 * lmag
    mx, emax = np.full(n, -np.inf), np.zeros(n)
    np.maximum.at(mx, rows, logit)
    np.maximum.at(emax, rows, e)
    x = logit - mx[rows]
    ex = np.exp(x)
    a = ex / _row_sum(rows, n, ex)[rows]
    da = e + emax[rows] + U32 * np.abs(x)
    return (a, a, a * (da + _row_sum(rows, n, a * da)[rows])), (logit, lmag)


def edge_softmax_bwd(rowptr, col, mult, n_cols, sL, sR, r, alpha, dalpha, g=None):
    """-> (g, mag), (dr, mag), (dsL, mag), (dsR, mag); the three sums from the stored `g` when it is given."""
    rowptr, col = np.asarray(rowptr, np.int64), np.asarray(col, np.int64)
    mult, sL, sR, r, a, da = f64(mult), f64(sL), f64(sR), f64(r), f64(alpha), f64(dalpha)
    rows, n = _rows_of(rowptr), len(rowptr) - 1
    dot, dmag = _row_sum(rows, n, a * da), _row_sum(rows, n, np.abs(a * da))
    gref, gmag = mult * a * (da - dot[rows]), mult * np.abs(a) * (np.abs(da) + dmag[rows])
    gu, ga = (gref, gmag) if g is None else (f64(g), np.abs(f64(g)))        # without a stored g the sums' mag is that of g's terms
    pre = sL[rows] + sR[col]
    gate = pre > 0.0
    t_r, t_l = gu[:, None] * np.where(gate, pre, 0.0), gu[:, None] * np.where(gate, r[rows], 0.0)
    m_r, m_l = ga[:, None] * np.where(gate, pre, 0.0), ga[:, None] * np.where(gate, np.abs(r[rows]), 0.0)
    # the column pass walks the transposed structure: entry t of it is entry perm[t] here
    perm = RR.host_perm(rowptr, col)
    rp_t, rows_t, _ = R.transpose_csr(rowptr, col, mult, n_cols)
    assert np.array_equal(rows_t, rows[perm])
    cols_t = np.repeat(np.arange(n_cols), np.diff(rp_t))
    return ((gref, gmag), (_row_sum(rows, n, t_r), _row_sum(rows, n, m_r)), (_row_sum(rows, n, t_l), _row_sum(rows, n, m_l)),
            (_row_sum(cols_t, n_cols, t_l[perm]), _row_sum(cols_t, n_cols, m_l[perm])))


# ================================================================================================ relation epilogue
def _leaky(y):
    return np.where(y > 0.0, y, SLOPE * y)


def rel_epi_fwd(Y, W, q, K):
    """-> (Yl, mag), (Z, mag), (r, mag, extra)"""
    Y, W, q = f64(Y), f64(W), f64(q)
    n, D = Y.shape
    dk = D // K
    yl = _leaky(Y)
    z, zmag = yl.reshape(n, K, dk) @ W, np.abs(yl).reshape(n, K, dk) @ np.abs(W)
    t = np.tanh(z)
    s = (t * q).sum(2)
    ds = U32 * ((dk + 2) * (np.abs(q) * (1.0 - t * t) * zmag).sum(2) + (2 * TANH_ULP + 1 + dk) * np.abs(t * q).sum(2))
    x = s - s.max(1, keepdims=True)
    ex = np.exp(x)
    r = ex / ex.sum(1, keepdims=True)
    da = ds + U32 * np.abs(x)
    return (yl, np.abs(yl)), (z.reshape(n, D), zmag.reshape(n, D)), (r, r, r * (da + (r * da).sum(1, keepdims=True)))


def rel_epi_bwd(Yl, Z, r, dZ, dr, W, q, K, dZt=None):
    """dZ / dr: None = 0, as the ABI's NULL.  -> (dY, mag), (dZt, mag), (dsT, mag), (dW, mag), (dq, mag); dY and dW from the
    stored `dZt` when it is given."""
    Yl, Z, r, W, q = f64(Yl), f64(Z), f64(r), f64(W), f64(q)
    n, D = Yl.shape
    dk = D // K
    th = np.tanh(Z).reshape(n, K, dk)
    if dr is None:
        dsk, dsmag = np.zeros((n, K, 1)), np.zeros((n, K, 1))
    else:
        dr = f64(dr)
        rd, rdmag = (r * dr).sum(1, keepdims=True), np.abs(r * dr).sum(1, keepdims=True)
        dsk, dsmag = (r * (dr - rd))[:, :, None], (np.abs(r) * (np.abs(dr) + rdmag))[:, :, None]
    dz = np.zeros((n, K, dk)) if dZ is None else f64(dZ).reshape(n, K, dk)
    dzt, dztmag = dz + dsk * q * (1.0 - th * th), np.abs(dz) + dsmag * np.abs(q) * (1.0 + th * th)
    dst, dstmag = dsk * th, dsmag * np.abs(th)
    du = dzt if dZt is None else f64(dZt).reshape(n, K, dk)
    dua = dztmag if dZt is None else np.abs(du)                             # without a stored dZt: the mag of dZt's terms
    slope = np.where(Yl > 0.0, 1.0, SLOPE)
    dy, dymag = (du @ W.T).reshape(n, D) * slope, (dua @ np.abs(W).T).reshape(n, D) * slope
    yl2, du2, dua2 = Yl.reshape(n * K, dk), du.reshape(n * K, dk), dua.reshape(n * K, dk)
    return ((dy, dymag), (dzt.reshape(n, D), dztmag.reshape(n, D)), (dst.reshape(n, D), dstmag.reshape(n, D)),
            (yl2.T @ du2, np.abs(yl2).T @ dua2), (dst.reshape(n * K, dk).sum(0), dstmag.reshape(n * K, dk).sum(0)))


# ========================================================================================================== combine
def _per_slice(p, dk):
    return np.repeat(f64(p), dk, axis=1)


def combine_fwd(ego, Z1, r1, Z2, r2, K, x=None):
    """-> (x, mag), (y, mag), (inv, mag), clamped [n, K]; y and inv from the stored `x` when it is given."""
    ego, Z1, Z2 = f64(ego), f64(Z1), f64(Z2)
    n, D = ego.shape
    dk = D // K
    t1, t2 = Z1 * _per_slice(r1, dk), Z2 * _per_slice(r2, dk)
    xref, xmag = ego + t1 + t2, np.abs(ego) + np.abs(t1) + np.abs(t2)
    xu = xref if x is None else f64(x)
    inv, clamped = R.inv_norm(RR._slices(xu, K))
    y = (RR._slices(xu, K) * inv[:, None]).reshape(n, D)
    inv = inv.reshape(n, K)
    return (xref, xmag), (y, np.abs(y)), (inv, inv), clamped.reshape(n, K)


def combine_bwd(x, inv, dy, Z1, r1, Z2, r2, K, dx=None):
    """-> (dx, mag), (dZ1, mag), (dZ2, mag), (dr1, mag), (dr2, mag); the dot of dx is dropped on the slices whose inv is the
    clamped 1e12; dZ_e and dr_e from the stored `dx` when it is given."""
    n, D = f64(x).shape
    dk = D // K
    dxref, dxmag = RR.slice_norm_bwd(x, inv, dy, K)
    du, dua = (dxref, dxmag) if dx is None else (f64(dx), np.abs(f64(dx)))   # without a stored dx: the mag of dx's terms
    out = [(dxref, dxmag)]
    for p in (r1, r2):
        out.append((_per_slice(p, dk) * du, np.abs(_per_slice(p, dk)) * dua))
    for Z in (Z1, Z2):
        out.append(((f64(Z) * du).reshape(n, K, dk).sum(2), (np.abs(f64(Z)) * dua).reshape(n, K, dk).sum(2)))
    return tuple(out)


# ================================================================================================ hand-placed inputs
N_ROWS, N_COLS = 303, 201              # neither a multiple of the 4 wavefronts of an edge-pass block
ROW_DEG = {0: 0, 1: 1, 2: 2, 3: 63, 5: 64, 6: 65, 9: 128, 10: 129, 301: 0, 302: 190}      # row -> degree, placed on purpose
CLOSED_ROWS = {20: 3, 21: 70, 22: 130}                                                     # rows whose every gate is closed
ZERO_ROWS, ZERO_COLS = tuple(range(30, 36)), tuple(range(10, 16))      # sL[row, 0] + sR[col, 0] == 0 exactly on this block
COL_HUB, COL_63, COL_64, COL_65, COL_1, COL_EMPTY = 0, 1, 2, 3, 4, (5, 200)


class Rel:
    """host CSR (rowptr int64, col int32, mult float32), its degrees, the transposed structure and the permutation"""

    def __init__(self, rowptr, col, mult):
        self.rowptr, self.col, self.mult = rowptr, col, mult
        self.n_rows, self.n_cols, self.nnz = len(rowptr) - 1, N_COLS, len(col)
        self.deg, self.rows_of = np.diff(rowptr), _rows_of(rowptr)
        self.perm = RR.host_perm(rowptr, col)
        self.rowptr_t, self.col_t, _ = R.transpose_csr(rowptr, col, mult, N_COLS)
        self.cdeg = np.diff(self.rowptr_t)


@functools.lru_cache(maxsize=None)
def relation():
    """One merged relation, 303 x 201, multiplicities 1 ... 4.  Row degrees 0, 1, 2, 63, 64, 65, 128, 129, 190 at ROW_DEG (the
    190 in the last row, which sits in a block of three); column degrees 0 (twice, the last column among them), 1, 63, 64,
    65 and a hub above 128; closed rows of 3, 70 and 130 entries; the block ZERO_ROWS x ZERO_COLS fully stored, row 30
    holding nothing else and column 10 nothing else."""
    rng = np.random.default_rng(20)
    deg = rng.integers(5, 13, N_ROWS)
    for table in (ROW_DEG, CLOSED_ROWS):
        for i, d in table.items():
            deg[i] = d
    deg[list(ZERO_ROWS)] = 14                                              # room for the block, the hub and the three columns
    deg[ZERO_ROWS[0]] = len(ZERO_COLS)
    M =np.zeros((N_ROWS, N_COLS), bool)
    M[np.ix_(ZERO_ROWS, ZERO_COLS)] = True
    fixed = set(ROW_DEG) | {ZERO_ROWS[0]}
    M[3, COL_1] = True
    roomy = np.array([i for i in range(N_ROWS) if deg[i] >= 5 and i not in fixed or i in (3, 5, 6, 9, 10, 302)])
    for c, d in ((COL_63, 63), (COL_64, 64), (COL_65, 65)):
        M[rng.permutation(roomy)[:d], c] = True
    M[roomy, COL_HUB] = True
    free = np.array([c for c in range(6, N_COLS - 1) if c != ZERO_COLS[0]])
    for i in range(N_ROWS):
        need = deg[i] - M[i].sum()
        assert need >= 0, i
        cand = free[~M[i, free]]
        M[i, rng.choice(cand, need, replace=False)] = True
    rows, cols = np.nonzero(M)
    rowptr = np.zeros(N_ROWS + 1, np.int64)
    np.cumsum(M.sum(1), out=rowptr[1:])
    mult = rng.integers(1, 5, len(cols)).astype(np.float32)
    return Rel(rowptr, cols.astype(np.int32), mult)


@functools.lru_cache(maxsize=None)
def edge_inputs(K, case):
    """float32 sL [303, K], sR [201, K], r [303, K], dalpha [nnz] for the relation.  `plain`: ordinary scores, r a softmax.
    `big`: the scores times 12 and r signed, so the logits span beyond +-80.  In both, factor 0 of ZERO_ROWS / ZERO_COLS is
    +-0.5 times the scale (the sum is exactly 0), and sL of CLOSED_ROWS is so negative that every gate is closed."""
    rel = relation()
    scale = {"plain": 1.0, "big": 12.0}[case]
    sL, sR = R.randn(N_ROWS, K, seed=31 + K, scale=1.0), R.randn(N_COLS, K, seed=32 + K, scale=1.0)
    sL[list(ZERO_ROWS), 0], sR[list(ZERO_COLS), 0] = 0.5, -0.5
    sL[list(CLOSED_ROWS)] = -64.0
    sL, sR = sL * scale, sR * scale
    r = torch.softmax(R.randn(N_ROWS, K, seed=33 + K, scale=1.0), 1)
    if case == "big":
        sign = torch.from_numpy(np.random.default_rng(34 + K).choice([-1.0, 1.0], (N_ROWS, K)).astype(np.float32))
        r = r * sign
    dalpha = R.randn(rel.nnz, seed=35 + K, scale=1.0)
    dalpha[5::17] = 0.0
    return sL.contiguous(), sR.contiguous(), r.contiguous(), dalpha


def _slice_pattern(n, D, K, seed):
    """spmm_ref.norm_rows by SLICE: x, dz [n, D] whose slices are, by slice index mod 8: 1 all-zero x, 3 x of norm ~1e-13, 5
    all-zero dz, 6 dz zero but for one -0.0.  -> x, dz, kind [n, K] (0 ordinary, 1 zero, 3 tiny)"""
    dk = D // K
    xs, dzs, _ = R.norm_rows(n * K, dk, seed=seed)
    idx = (torch.arange(n * K) % 8).reshape(n, K).numpy()
    kind = np.where(idx == 1, 1, np.where(idx == 3, 3, 0))
    return xs.reshape(n, D), dzs.reshape(n, D), kind


def combine_inputs(n, D, K, seed):
    """ego, Z1, r1, Z2, r2, dy: x = ego + r1 Z1 + r2 Z2 has all-zero slices, slices of norm ~1e-13 (Z1 = Z2 = 0 there, so x
    is ego exactly) and ordinary ones; dy has all-zero slices and slices that are zero but for one -0.0."""
    ego, dy, kind = _slice_pattern(n, D, K, seed)
    keep = torch.from_numpy(np.repeat(kind == 0, D // K, axis=1))
    Z1, Z2 = R.randn(n, D, seed=seed + 2) * keep, R.randn(n, D, seed=seed + 3) * keep
    r1, r2 = torch.softmax(R.randn(n, K, seed=seed + 4, scale=1.0), 1), torch.softmax(R.randn(n, K, seed=seed + 5, scale=1.0), 1)
    return ego, Z1, r1, Z2, r2, dy


def epilogue_inputs(n, D, K, seed, case="plain"):
    """Y, W, q, dZ, dr.  Y holds exact 0.0, -0.0 and negative values, and all-zero rows (row index 1 mod 8: Z = 0 and
    r = 1 / K exactly); dZ follows the slice pattern (zero and -0.0 upstream slices).  `sat`: Y times 32, so that tanh(Z)
    saturates (|Z| of order 20)."""
    dk = D // K
    Y = R.randn(n, D, seed=seed, scale=1.0)
    Y.reshape(-1)[3::7] = 0.0
    Y.reshape(-1)[5::11] = -0.0
    Y[torch.arange(n) % 8 == 1] = 0.0
    if case == "sat":
        Y = Y * 32.0
    W = R.randn(dk, dk, seed=seed + 1, scale=1.0 / np.sqrt(dk))
    q = R.randn(dk, seed=seed + 2, scale=1.0)
    _, dZ, _ = _slice_pattern(n, D, K, seed + 3)
    dr = R.randn(n, K, seed=seed + 5, scale=1.0)
    return Y, W, q, dZ, dr


def row_sizes(D):
    """n of the every-shape test: one row, one row more than a block's group, one row short of five groups"""
    rb = 256 // D
    return 1, rb + 1, 5 * rb - 1


def second_trip_n(D):
    """more groups than the grid's cap, the last of them ragged: blocks 0 and 1 take a second trip of the grid-stride loop"""
    rb = 256 // D
    return MAX_GROUPS * rb + rb + 1
