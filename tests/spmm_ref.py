"""Plain fp64 restatements of the sparse products of csrc/spmm.hip and their row epilogues, the tolerance helper and the
counter-based masks shared by test_gpu_spmm.py, test_gpu_rowops.py, test_gpu_edge_drop.py and test_spmm_ref_host.py.
numpy / torch on the CPU; no project code.

Tolerance.  A float result is accepted iff

    |got - ref64| <= c * 2^-24 * mag + extra + 1e-30

`mag` is the fp64 sum of the absolute values of the terms that form the output and `c` the number of rounded fp32 operations on
the longest path to it, read off the kernel and written beside each check.  Every reference here returns (ref, mag).  Where a
result depends on a rounded product through a norm (NORM_ACC, SS), `mag` carries the first-order propagation of the product's
error: with y the product, m its magnitude and k = sum |y| m / sum y^2 >= 1 the condition of the row norm, an error of c u m
in y is an error of c u k in the relative norm."""
import numpy as np
import torch

U32 = 2.0 ** -24                       # unit roundoff of fp32
U64 = np.uint64
EPS = 1e-12                            # F.normalize's clamp
INV_CLAMPED = np.float32(1e12)         # what 1.0f / 1e-12f rounds to: the kernels test inv >= 1e12f


def f64(t):
    return t.detach().cpu().double().numpy() if isinstance(t, torch.Tensor) else np.asarray(t, dtype=np.float64)


class Chk:
    """Collects err / bound of every comparison of one test; `done()` prints the worst and asserts it is <= 1."""

    def __init__(self, name, tag="rowops"):
        self.name, self.tag, self.worst, self.where = name, tag, 0.0, "-"

    def close(self, what, got, ref, mag, c, extra=0.0):
        got, ref = f64(got), f64(ref)
        assert got.shape == ref.shape, f"{what}: shape {got.shape} vs {ref.shape}"
        assert np.isfinite(got).all() and np.isfinite(ref).all(), f"{what}: non-finite value"
        bound = np.broadcast_to(c * U32 * f64(mag) + extra + 1e-30, ref.shape)
        ratio = np.abs(got - ref) / bound
        if ratio.size and ratio.max() > self.worst:
            i = np.unravel_index(int(ratio.argmax()), ratio.shape)
            self.worst = float(ratio.max())
            self.where = f"{what}{list(map(int, i))}: got {got[i]!r} ref {ref[i]!r} bound {bound[i]:.3e}"

    def done(self):
        print(f"[{self.tag}] {self.name}: worst err/bound = {self.worst:.3f}  ({self.where})")
        assert self.worst <= 1.0, f"{self.name}: err / bound = {self.worst:.3f} at {self.where}"


def randn(*shape, seed, scale=0.1):
    return torch.randn(*shape, generator=torch.Generator().manual_seed(seed)) * scale


def same_bits(a, b):
    if a.dtype != torch.float32:                                     # flags, counters: equal values are equal bits
        return a.dtype == b.dtype and torch.equal(a, b)
    return torch.equal(a.contiguous().view(torch.int32), b.contiguous().view(torch.int32))


# ====================================================================================================== row normalise
def norm_rows(n, D, seed):
    """x, dz [n, D] with, by row index mod 8: 1 an all-zero x row, 3 an x row of norm ~1e-13 (clamped, non-zero), 5 an all-zero
    dz row, 6 a dz row that is zero but for one -0.0; the others ordinary.  -> x, dz, clamped (fp64 norm below eps)."""
    x, dz = randn(n, D, seed=seed), randn(n, D, seed=seed + 1)
    r = torch.arange(n) % 8
    x[r == 1] = 0
    tiny = r == 3
    x[tiny] = x[tiny] / x[tiny].double().norm(dim=1, keepdim=True).float() * 1e-13
    dz[r == 5] = 0
    dz[r == 6] = 0
    dz[r == 6, D // 2] = -0.0
    clamped = (x.double().norm(dim=1) < EPS).numpy()
    return x, dz, clamped


def inv_norm(x):
    """fp64 1 / max(||x[r]||, eps) and which rows are clamped."""
    nrm = np.linalg.norm(f64(x), axis=1)
    return 1.0 / np.maximum(nrm, EPS), nrm < EPS


def ref_norm_bwd(x, inv, dz, s, clamped):
    """fp64 normalize-backward from the kernel's own inputs (x, inv, dz): inv (s dz - z (z . s dz)), z = x inv, and the dot
    dropped where the norm was clamped to eps (the denominator is then a constant).  -> ref, mag, dot, dot_mag."""
    x, inv, sdz = f64(x), f64(inv)[:, None], s * f64(dz)
    z = x * inv
    dot, dmag = (z * sdz).sum(1, keepdims=True), np.abs(z * sdz).sum(1, keepdims=True)
    dot[clamped], dmag[clamped] = 0.0, 0.0
    return inv * (sdz - z * dot), np.abs(inv) * (np.abs(sdz) + np.abs(z) * dmag), dot[:, 0], dmag[:, 0]


# ============================================================================================================ products
def product(rowptr, col, val, X):
    """(A X, sum_j |val_j| |X[col_j]|, row degrees) in fp64, the CSR taken as given (duplicate column ids are further terms:
    they add up in the dense fp64 copy of A, and their absolute values in the copy of |A|)."""
    rowptr, col = np.asarray(rowptr, np.int64), np.asarray(col, np.int64)
    val, X = f64(val), f64(X)
    n, deg = len(rowptr) - 1, np.diff(rowptr)
    rows = np.repeat(np.arange(n), deg)
    A, Aabs = np.zeros((n, X.shape[0])), np.zeros((n, X.shape[0]))
    np.add.at(A, (rows, col), val)
    np.add.at(Aabs, (rows, col), np.abs(val))
    return A @ X, Aabs @ np.abs(X), deg


def transpose_csr(rowptr, col, val, n_cols):
    """CSR of the transpose, entries of a row in ascending source row, duplicates kept as separate entries."""
    rowptr, col = np.asarray(rowptr, np.int64), np.asarray(col, np.int64)
    rows = np.repeat(np.arange(len(rowptr) - 1), np.diff(rowptr))
    order = np.argsort(col, kind="stable")
    rp = np.zeros(n_cols + 1, np.int64)
    np.cumsum(np.bincount(col, minlength=n_cols), out=rp[1:])
    return rp, rows[order], np.asarray(val)[order]


def _norm_condition(y, m):
    ss = (y * y).sum(1)
    with np.errstate(divide="ignore", invalid="ignore"):
        k = np.where(ss > 0, (np.abs(y) * m).sum(1) / ss, 1.0)
    return ss, k


def epi_norm_acc(y, m, acc0, s):
    """NORM_ACC on the fp64 product (y, m): -> (y, m), (inv, inv_mag), (acc, acc_mag), clamped.
    inv = 1 / max(||y||, 1e-12); acc = acc0 + s y inv (acc0 None: no accumulator, acc is None)."""
    ss, k = _norm_condition(y, m)
    nrm = np.sqrt(ss)
    inv = 1.0 / np.maximum(nrm, EPS)
    out = None
    if acc0 is not None:
        a0 = f64(acc0)
        out = (a0 + s * y * inv[:, None], np.abs(a0) + abs(s) * inv[:, None] * (m + np.abs(y) * k[:, None]))
    return (y, m), (inv, inv * k), out, nrm < EPS


def epi_normbwd(y, m, x_raw, inv, dz, s, clamped, b_flags=None):
    """NORMBWD: A g + inv (s dz - z (z . s dz)); rows with b_flags == 0 have no second term (their dz is promised zero)."""
    nb, nbm, _, _ = ref_norm_bwd(x_raw, inv, dz, s, clamped)
    if b_flags is not None:
        off = np.asarray(b_flags) == 0
        nb, nbm = nb.copy(), nbm.copy()
        nb[off], nbm[off] = 0.0, 0.0
    return y + nb, m + nbm


def epi_axpy(y, m, b, s, b_flags=None):
    t = s * f64(b)
    if b_flags is not None:
        t = t.copy()
        t[np.asarray(b_flags) == 0] = 0.0
    return y + t, m + np.abs(t)


def epi_ss(y, m):
    """SS: the shard's sum of squares per row -> ref, mag (the error of y enters twice through y^2)."""
    return (y * y).sum(1), 2.0 * (np.abs(y) * m).sum(1)


def row_dot(x_raw, inv, dz, s):
    """z . (s dz) per row over the given columns (what the caller of NORMBWD_DOT sums over the column shards)."""
    return (f64(x_raw) * f64(inv)[:, None] * s * f64(dz)).sum(1)


def epi_normbwd_dot(y, m, x_raw, inv, dz, dot, s):
    """NORMBWD_DOT: A g + inv (s dz - x inv dot) with the row dot supplied; the dot is dropped where inv is the clamped 1e12."""
    x, iv, sdz = f64(x_raw), f64(inv)[:, None], s * f64(dz)
    dt = np.where(f64(inv) >= float(INV_CLAMPED), 0.0, f64(dot))[:, None]
    return y + iv * (sdz - x * iv * dt), m + np.abs(iv) * (np.abs(sdz) + np.abs(x * iv * dt))


# ================================================================================================= counter-based masks
def mix64(z):
    with np.errstate(over="ignore"):
        z = z + U64(0x9E3779B97F4A7C15)
        z = (z ^ (z >> U64(30))) * U64(0xBF58476D1CE4E5B9)
        z = (z ^ (z >> U64(27))) * U64(0x94D049BB133111EB)
        return z ^ (z >> U64(31))


def np_drop(x, idx4, p, seed):
    """numpy restatement of drop4: x [..., 4] float32, idx4 the float4 index of each group of four."""
    p32 = np.float32(p)
    h = mix64(U64(seed) ^ mix64(idx4.astype(U64)))
    thr = U64(int(p32 * np.float32(65536.0)))
    keep = np.float32(1.0) / (np.float32(1.0) - p32)
    draws = np.stack([(h >> U64(s)) & U64(0xFFFF) for s in (0, 16, 32, 48)], -1)
    return np.where(draws >= thr, x * keep, np.float32(0.0)).astype(np.float32)


def drop_keep(n, D, p, seed):
    """(keep mask [n, D] of the epilogue's message dropout, the float32 scale 1 / (1 - p)): element index r D / 4 + c."""
    idx4 = np.arange(n * (D // 4))
    kept = np_drop(np.ones((n * (D // 4), 4), np.float32), idx4, p, seed) != 0
    return kept.reshape(n, D), float(np.float32(1.0) / (np.float32(1.0) - np.float32(p)))


def edge_kept(rows, cols, p, seed, transposed=False):
    """numpy restatement of edge_kept (csrc/common.h): the stored entry (row, col) survives the mask of (p, seed)."""
    i, j = (cols, rows) if transposed else (rows, cols)
    key = (np.asarray(i).astype(U64) << U64(32)) | (np.asarray(j).astype(U64) & U64(0xFFFFFFFF))
    h = mix64(U64(seed) ^ mix64(key))
    thr = U64(int(np.float32(p) * np.float32(16777216.0)))
    return (h >> U64(40)) >= thr


# ================================================================================================ flags and row marks
def row_flags(a):
    """uint8 [n]: row r of `a` holds a non-zero (-0.0 is zero)."""
    return (f64(a) != 0).any(1).astype(np.uint8)


def mark_rows(rowptr, col, rows, flags, self_too=True):
    """Set walk of mark_rows (self_too) / mark_cols: flags[c] = 1 for every column stored in the listed rows (and the rows)."""
    out = np.array(flags, copy=True)
    hit = set()
    for r in map(int, rows):
        if self_too:
            hit.add(r)
        hit.update(int(c) for c in col[rowptr[r]:rowptr[r + 1]])
    for c in hit:
        out[c] = 1
    return out
