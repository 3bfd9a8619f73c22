"""Plain fp64 restatements of the routed-propagation kernels of csrc/routing.hip, shared by test_gpu_routing_kernels.py and
test_routing_ref_host.py (which holds them to torch autograd in fp64).  numpy / torch on the CPU; no project code.

Layout as in the kernels: embeddings [N, D] with factor k in columns [k D/K, (k+1) D/K); per-node scalars [N, K]; per-entry
scalars [nnz, K] in CSR entry order.  Every reference returns (ref, mag) for the rule of spmm_ref.py,

    |got - ref64| <= c * 2^-24 * mag + extra + 1e-30,

the two softmaxes (ref, mag, extra).  The counts `c`, read off the kernels (u = 2^-24; an fma rounds once):

  product row         stored entries + 512-entry chunks of a long row (`Ladder.c`: whatever the lane / chunk tree, a term passes
                      at most that many rounded additions), + 1 for each of `post` (a product), `self` (an addition) and
                      `b_scale * B` (an fma): epilogue_count().  mag = |post| sum |w| |x| + |self| + |b_scale B|.
     long rows, also  the depth of the lane tree, far below the count above on a hub: a wavefront's NPI = 256 / D lane groups
                      each add every NPI-th entry of a chunk by fmas in turn (512 / NPI), a butterfly joins them (log2 NPI);
                      the finish kernel adds every NPI-th chunk in turn (ceil(chunks / NPI)) and joins again (log2 NPI):
                      tree_count().  A dropped or doubled partial sum of a 98-chunk row hides under the first count.
  slice dot           r4_dot (a product and three fmas) and log2(SL) butterfly additions: <= D/K.
  Yn, inv of a        the D/K-term sum of squares (halved by the square root), sqrtf, the float 1e-12 and the divide: + D/K + 3 on
  product             the product's count; mag carries the first-order propagation of the product's error through the slice
                      norm (spmm_ref.epi_norm_acc on the [N K, D/K] view).
  score               the slice dot: D/K.  Accumulate form: + 1, and mag adds |prior|.
  route_softmax       l - max (1, through the slope: extra), expf (4 ulp = 8), the sum of K such terms (8 + K - 1), the divide:
                      K + 16.  extra = w_k (da_k + sum_i w_i da_i), da = u |l - max|, as test_gpu_rank_loss.py treats it.
  rowsum_rsqrt        a lane adds its entries j, j + 64, ... in turn, then a 6-step butterfly: ceil(len / 64) + 6 per row or
                      chunk (len <= 512 for a chunk), + the chunks of a long row added in turn.  The weights are positive, so
                      this is the sum's relative error; the square root halves it, sqrtf and the divide add 2: rowsum_count().
  row_softmax         the sum as above (ceil(deg / 64) + 6) of terms carrying expf's 8, the numerator's 8, the divide:
                      ceil(deg / 64) + 23, and the slope's extra as for route_softmax.
  row_softmax_bwd     the dot a . da by fmas in the same tree (ceil(deg / 64) + 6), the subtraction and the product: + 2.
  slice_scale         one product: 1.
  slice_norm_fwd      D/K-term sum of squares halved by sqrtf (D/2K), sqrtf, the float 1e-12, the divide: D/2K + 3 for y and inv.
     with tanh        the above through the slope 1 - tanh^2 as extra, + tanhf: TANH_ULP ulp = 2 TANH_ULP u on |tanh|.
  slice_norm_bwd      z = x inv (1), the dot (D/K), z dot (1), the subtraction, the product with inv, 1 spare: D/K + 6 (the count
                      of the row kernel in test_gpu_rowops.py, per slice).

tanhf: the project's rule (expf, logf: 4 ulp) does not cover it and the ROCm installation carries no accuracy table for the
device library, so it is measured: over the inputs of test_slice_ops_every_shape (all 19 shapes, |z| <= 1) the worst error of
the kernel's tanhf against fp64 tanh of the same float argument on an MI355X was 1.350 ulp (TANH_ULP_MEASURED; D = 64, K = 8);
the count allowed is twice that, rounded up: TANH_ULP = 3."""
import numpy as np

import spmm_ref as R
from spmm_ref import U32, f64

TANH_ULP_MEASURED = 1.350              # worst over the 19 shapes (D = 64, K = 8), printed by test_slice_ops_every_shape
TANH_ULP = 3                           # twice the measured worst, rounded up
K_LONG, K_CHUNK = 1024, 512            # kLongRow, kChunk of csrc/graph.h
# the 19 instantiations of ROUTE_CASE: D in {16, 32, 64, 128, 256}, K in {1, 2, 4, 8}, D / 4 a multiple of K
SHAPES = tuple((D, K) for D in (16, 32, 64, 128, 256) for K in (1, 2, 4, 8) if (D // 4) % K == 0)
assert len(SHAPES) == 19


def _rows_of(rowptr):
    rowptr = np.asarray(rowptr, np.int64)
    return np.repeat(np.arange(len(rowptr) - 1), np.diff(rowptr))


def _slices(a, K):
    """[N, D] -> [N K, D / K]: one row per factor slice."""
    a = f64(a)
    return a.reshape(a.shape[0] * K, a.shape[1] // K)


# ===================================================================================================== per-entry weights
def route_softmax(logits):
    """softmax over the K logits of every entry -> w, mag, extra."""
    a = f64(logits)
    a = a - a.max(1, keepdims=True)
    e = np.exp(a)
    w = e / e.sum(1, keepdims=True)
    da = U32 * np.abs(a)
    return w, w, w * (da + (w * da).sum(1, keepdims=True))


def rowsum_rsqrt(rowptr, w):
    """d[r, k] = 1 / sqrt(sum of w[j, k] over row r), inf -> 0."""
    w = f64(w)
    s = np.zeros((len(rowptr) - 1, w.shape[1]))
    np.add.at(s, _rows_of(rowptr), w)
    with np.errstate(divide="ignore"):
        d = np.where(s > 0, 1.0 / np.sqrt(s), 0.0)
    return d, np.abs(d)


def rowsum_count(deg):
    """[n, 1] rounded operations of rowsum_rsqrt per row of `deg` entries (header)."""
    deg = np.asarray(deg, np.int64)
    long = deg > K_LONG
    s = np.where(long, K_CHUNK // 64 + 6 + -(-deg // K_CHUNK), -(-deg // 64) + 6)
    return (0.5 * s + 2.0)[:, None]


def host_perm(rowptr, col):
    """Entry j of the transposed CSR (rows ascending inside a transposed row, duplicates kept) is entry perm[j] of this one."""
    return np.argsort(np.asarray(col, np.int64), kind="stable")


def permute(w, perm):
    out = f64(w)[np.asarray(perm, np.int64)]
    return out, np.abs(out)


# ============================================================================================================== products
def routed_product(rowptr, col, w, x, post=None, self_add=None, b=None, b_scale=0.0):
    """y = post * (A(w) x) + self + b_scale B per factor slice: K products of spmm_ref.product on column slices, val = w[:, k]."""
    w, x = f64(w), f64(x)
    K, D = w.shape[1], x.shape[1]
    dk = D // K
    n = len(rowptr) - 1
    y, m = np.empty((n, D)), np.empty((n, D))
    for k in range(K):
        sl = slice(k * dk, (k + 1) * dk)
        y[:, sl], m[:, sl], _ = R.product(rowptr, col, w[:, k], x[:, sl])
    return epilogue(y, m, K, post, self_add, b, b_scale)


def epilogue(y, m, K, post=None, self_add=None, b=None, b_scale=0.0):
    """(post * y + self + b_scale B, its magnitude) of a plain routed product (y, m); b_scale is the float the ABI takes."""
    if post is not None:
        p = np.repeat(f64(post), y.shape[1] // K, axis=1)
        y, m = p * y, np.abs(p) * m
    for t, s in ((self_add, 1.0), (b, float(np.float32(b_scale)))):
        if t is not None:
            y, m = y + s * f64(t), m + np.abs(s * f64(t))
    return y, m


def epilogue_count(post=None, self_add=None, b=None):
    return sum(t is not None for t in (post, self_add, b))


def tree_count(deg, D):
    """[n, 1] depth of the product's lane tree (header): the second, tighter count the long rows are also held to."""
    deg = np.asarray(deg, np.int64)
    npi = 256 // D                                                       # lane groups of a wavefront: 64 / (D / 4)
    lg = int(np.log2(npi))
    chunks = -(-deg // K_CHUNK)
    long = deg > K_LONG
    return np.where(long, K_CHUNK // npi + -(-chunks // npi) + 2 * lg, -(-deg // npi) + lg).astype(np.float64)[:, None]


def transposed_product(rowptr, col, w, x, n_cols, **epi):
    """A(w)^T x (+ epilogue) on the transpose with duplicates kept as separate entries -> y, mag, (rowptr_t, col_t)."""
    rp, c, wt = R.transpose_csr(rowptr, col, f64(w), n_cols)
    return routed_product(rp, c, wt, x, **epi) + ((rp, c),)


def slice_normalise(y, m, K):
    """The product's per-slice normalisation of (y, m): -> (Yn, Yn_mag), (inv [N, K], inv_mag), clamped [N, K].
    Yn = y / max(||y_slice||, 1e-12), inv = 1 / max(.); the mags carry the slice norm's condition (spmm_ref.epi_norm_acc)."""
    n, D = y.shape
    ys, ms = _slices(y, K), _slices(m, K)
    _, (inv, inv_mag), (yn, yn_mag), clamped = R.epi_norm_acc(ys, ms, np.zeros_like(ys), 1.0)
    return (yn.reshape(n, D), yn_mag.reshape(n, D)), (inv.reshape(n, K), inv_mag.reshape(n, K)), clamped.reshape(n, K)


def score(rowptr, col, H, T, K, prior=None, block=1 << 14):
    """logits[j, k] = <H[row_j, slice k], T[col_j, slice k]> (+ prior[j, k]: the accumulate form)."""
    H, T, col = f64(H), f64(T), np.asarray(col, np.int64)
    rows, dk = _rows_of(rowptr), H.shape[1] // K
    ref, mag = np.empty((len(col), K)), np.empty((len(col), K))
    for s in range(0, len(col), block):
        t = (H[rows[s:s + block]] * T[col[s:s + block]]).reshape(-1, K, dk)
        ref[s:s + block], mag[s:s + block] = t.sum(2), np.abs(t).sum(2)
    if prior is not None:
        ref, mag = ref + f64(prior), mag + np.abs(f64(prior))
    return ref, mag


# =========================================================================================================== row softmax
def row_softmax(rowptr, logits):
    """softmax over the stored entries of every CSR row -> a, mag, extra."""
    l, rows, n = f64(logits), _rows_of(rowptr), len(rowptr) - 1
    mx = np.full(n, -np.inf)
    np.maximum.at(mx, rows, l)
    x = l - mx[rows]
    e = np.exp(x)
    s = np.zeros(n)
    np.add.at(s, rows, e)
    a = e / s[rows]
    da = U32 * np.abs(x)
    pda = np.zeros(n)
    np.add.at(pda, rows, a * da)
    return a, a, a * (da + pda[rows])


def row_softmax_count(deg):
    """per-ENTRY counts (sum tree of the entry's row) -> (forward, backward)"""
    deg = np.asarray(deg, np.int64)
    tree = np.repeat(-(-deg // 64) + 6, deg).astype(np.float64)
    return tree + 17, tree + 2


def row_softmax_bwd(rowptr, a, da):
    """dlogit = a (da - sum_row a da)."""
    a, da, rows, n = f64(a), f64(da), _rows_of(rowptr), len(rowptr) - 1
    dot, dmag = np.zeros(n), np.zeros(n)
    np.add.at(dot, rows, a * da)
    np.add.at(dmag, rows, np.abs(a * da))
    return a * (da - dot[rows]), np.abs(a) * (np.abs(da) + dmag[rows])


# ============================================================================================================= slice ops
def slice_scale(x, p):
    x, p = f64(x), f64(p)
    n, D = x.shape
    y = (x.reshape(n, p.shape[1], -1) * p[:, :, None]).reshape(n, D)
    return y, np.abs(y)


def slice_norm_fwd(x, K, tanh=False):
    """y = x / max(||x_slice||, 1e-12) (tanh of it), inv = 1 / max(.)  -> (y, y_mag, y_extra_slope), (inv, inv_mag).
    y_extra_slope is |z| (1 - tanh^2 z), what an error of the normalised z costs after tanh (0 without tanh)."""
    x = f64(x)
    n, D = x.shape
    inv, _ = R.inv_norm(_slices(x, K))
    z = (_slices(x, K) * inv[:, None]).reshape(n, D)
    inv = inv.reshape(n, K)
    if not tanh:
        return (z, np.abs(z), np.zeros_like(z)), (inv, inv)
    t = np.tanh(z)
    return (t, np.abs(t), np.abs(z) * (1.0 - t * t)), (inv, inv)


def slice_norm_bwd(x, inv, dz, K):
    """dX = inv (dZ - z (z . dZ)) per slice, z = x inv, from the kernel's own inputs; the dot is dropped on the slices whose inv
    is the clamped 1e12 (the denominator is then a constant)."""
    n, D = f64(x).shape
    iv = f64(inv).reshape(n * K)
    ref, mag, _, _ = R.ref_norm_bwd(_slices(x, K), iv, _slices(dz, K), 1.0, iv >= float(R.INV_CLAMPED))
    return ref.reshape(n, D), mag.reshape(n, D)
