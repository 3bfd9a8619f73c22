"""Plain fp64 restatements of the TGCN neighbour-attention kernels (csrc/tgcn.hip and the two destination-centric pulls of
csrc/spmm.hip), shared by test_gpu_tgcn_attn_kernels.py and test_tgcn_attn_ref_host.py (which holds them to torch autograd in
fp64 and to the oracle).  numpy on the CPU; no project code.  What is restated is the kernels' CONTRACT (include/tagrec.h):

    h[v, n, :] = P[v] + WT[widx[v, n]] + (idx[v, n] ? Q[idx[v, n] - 1] : 0)        WT[0] is a row like any other
    s = relu(h) . v;   a = softmax_k(s) (a pad slot takes part);   out[v] = sum_n a (idx ? Ej[idx - 1] : 0)
    da = dOut . Ej[idx - 1] (0 at a pad);  ds = a (da - sum a da);  dh = ds v [h > 0]  (0 at h == 0)
    dP = sum_n dh;  dWT[w] = sum_{widx = w} dh;  dv = sum ds h [h > 0];  dQ[j] = sum_{idx - 1 = j} dh;  dEj[j] = sum a dOut
    comp = (ds, the A bits [h > 0]);   dQ[j] = v (.) sum_p ds[p] bits[p] (+ B)   (attn_pull_dq, attn_seg_dq)

Every reference returns (ref, mag) -- the forward weights and `out` also `extra` -- for the rule of spmm_ref.py,

    |got - ref64| <= c * 2^-24 * mag + extra + 1e-30,

`mag` the fp64 sum of the absolute values of the terms.  The counts `c`, read off the kernels (u = 2^-24; an fma rounds once; a
butterfly over lanes of which only the first m hold a non-zero term rounds at most ceil(log2 m) times on any path, adding 0 is
exact).  The tests draw P, Q, WT on the grid 2^-8 Z, so h is exact and neither it nor [h > 0] carries an error:

  score s           A products relu(h) v (1) and their xor tree (log2 A): c_score = 1 + log2 A.  mag = sum |relu(h) v|.
  weight a          expf of the numerator (4 ulp = 8 u), the k-term wave sum of terms carrying expf's 8 (8 + ceil(log2 k)), the
                    divide: c_attn = 17 + ceil(log2 k), mag = a.  The rounded s - max (u |s - max|) and the error of s itself
                    (c_score u mag_s) enter through the softmax's slope: extra = a_n (e_n + sum_i a_i e_i), e = the two summed
                    (as routing_ref.route_softmax).
  out               lane group g of RPI = 256 / D adds neighbours g, g + RPI, ... by fmas, four per pass of the unrolled loop,
                    the padded ones adding 0: 4 ceil(k / 4 RPI) steps, then the log2 RPI tree: c_out.  mag = sum a |Ej|; the
                    error of a propagates as extra = sum_n (c_attn u a_n + extra_n) |Ej[n]|.
  da                a lane's 4 columns (a product and three fmas: 4), the tree over the D / 4 lanes: c_da = 4 + log2(D / 4), in
                    attn_bwd as in attn_pull_da.  mag = sum |dOut| |Ej|.
  ds                the products a da (1), their k-term wave sum (ceil(log2 k)), the subtraction (1), the product with a (1):
                    c_ds = 3 + ceil(log2 k) on mag = a_n (|da_n| + sum_i a_i |da_i|); where da is formed in the same kernel
                    (attn_bwd) its c_da rides along on the same shape with |da| replaced by da's magnitude: c_da + c_ds.
  dh                one more product: c_ds + 1, mag = mag_ds |v|.
  dP                a lane adds neighbours grp, grp + npi, ... (npi = 64 / A) in turn: ceil(k / npi), then the log2 npi tree
                    over lane groups: c_dh + ceil(k / npi) + log2 npi.  mag = sum_n mag_dh.
  dWT, dv           LDS float atomics per block, then the fold.  A term passes at most: the additions of its block into the
                    same address -- for dWT[w] the block's pairs with widx = w (count_entries, maximum over blocks); for dv the
                    lane's fma chain over its nodes (ceil(n / (4 blocks)) ceil(k / npi)), the log2 npi tree and the block's 4
                    waves -- plus, for dWT of attn_bwd_ds, its 4 * 64 / A partial sums (the private LDS copies folded in turn, or,
                    with one shared copy, the w_major registers of every wave and lane group added to it) and 1 (the register
                    partial entering its private copy), plus the fold: every 16th
                    block in turn (ceil(blocks / 16)) and the 16 of the combine.  On top of c_dh (dWT) or c_ds + 1 (dv, the fma).
  scatter dQ, dEj   float atomics into the destination: its multiplicity m_j, on top of c_dh (dQ) or the product a dOut (1).
  pulls (dEj of     the destination's pairs plus its 512-entry chunks (whatever the lane / chunk tree, a term passes at most
  attn_pull_da,     that many additions), + 1 for the product with v (pull_dq), + 1 for B.  A destination of more than 1024
  dQ of pull_dq)    pairs is ALSO held to the depth of its lane tree: G lane groups (256 / D for pull_da, 64 / A for pull_dq)
                    each add every G-th entry of a chunk in turn (512 / G), a butterfly joins them (log2 G); the finish kernel
                    adds every F-th chunk in turn (ceil(chunks / F), F = 256 / D resp. 256 / A) and joins again (log2 F).
  seg_dq            a wave adds the entries of a destination inside its 256-entry segment in turn, multiplies by v (1) and adds
                    the segment to dQ atomically: pairs + segments spanned + 1.  mag includes |dQ before|.
"""
import numpy as np

from spmm_ref import U32, f64

K_LONG, K_CHUNK, SEG = 1024, 512, 256       # kLongRow, kChunk (csrc/graph.h), kSegEntries (csrc/tgcn.hip)
ATTN_BLOCKS, ATTN_WAVES = 2048, 4           # kAttnBlocks, kAttnWaves
EXPF_U = 8                                  # the project's 4-ulp expf, in units of u
DS = (16, 32, 64, 128, 256)
AS = (4, 8, 16, 32, 64)
KS = (1, 2, 3, 9, 25, 63, 64)


def _lg(x):
    return int(np.ceil(np.log2(x))) if x > 1 else 0


def _cdiv(a, b):
    return -(-a // b)


# ================================================================================================================ counts
def c_score(A):
    return 1 + _lg(A)


def c_attn(k):
    return 2 * EXPF_U + _lg(k) + 1


def c_out(k, D):
    rpi = 256 // D
    return 4 * _cdiv(k, 4 * rpi) + _lg(rpi)


def c_da(D):
    return 4 + _lg(D // 4)


def c_ds(k):
    return 3 + _lg(k)


def c_dp(k, A):
    npi = 64 // A
    return _cdiv(k, npi) + _lg(npi)


def attn_blocks(n):
    return min(max(_cdiv(n, ATTN_WAVES), 1), ATTN_BLOCKS)


def block_of(n):
    """block that walks node v: v = block * 4 + wave + i * (4 blocks)"""
    return (np.arange(n) % (ATTN_WAVES * attn_blocks(n))) // ATTN_WAVES


def c_fold(n):
    return _cdiv(attn_blocks(n), 16) + 16


def count_entries(widx, n_wt):
    """[n_wt, 1]: the most pairs with widx = w inside one block"""
    n, k = widx.shape
    cnt = np.zeros((attn_blocks(n), n_wt), np.int64)
    np.add.at(cnt, (np.repeat(block_of(n), k), np.asarray(widx, np.int64).reshape(-1)), 1)
    return cnt.max(0).astype(np.float64)[:, None]


def c_dwt(widx, n_wt, A, ds_form):
    """on top of c_dh"""
    return count_entries(widx, n_wt) + (ATTN_WAVES * (64 // A) + 1 if ds_form else 0) + c_fold(widx.shape[0])


def c_dv(n, k, A):
    """on top of c_ds + 1"""
    npi = 64 // A
    return _cdiv(n, ATTN_WAVES * attn_blocks(n)) * _cdiv(k, npi) + _lg(npi) + ATTN_WAVES + c_fold(n)


def pull_counts(deg, G, F):
    """([n_dst, 1] pairs + chunks, [n_dst, 1] depth of the lane tree (meant for deg > K_LONG)) of a destination-centric pull with
    G lane groups in the gather and F in the finish (header)."""
    deg = np.asarray(deg, np.int64)
    chunks = _cdiv(deg, K_CHUNK)
    flat = (deg + chunks).astype(np.float64)[:, None]
    tree = (K_CHUNK // G + _lg(G) + _cdiv(chunks, F) + _lg(F)).astype(np.float64)[:, None]
    return flat, tree


def seg_spans(rowptr):
    """[n_dst] number of 256-entry segments the sorted entries of a destination touch (0 for an empty one)"""
    rp = np.asarray(rowptr, np.int64)
    lo, hi = rp[:-1], rp[1:]
    return np.where(hi > lo, (hi - 1) // SEG - lo // SEG + 1, 0)


# =============================================================================================================== forward
def pre_activation(P, Q, WT, idx, widx):
    """h [n, k, A]"""
    P, Q, WT = f64(P), f64(Q), f64(WT)
    idx, widx = np.asarray(idx, np.int64), np.asarray(widx, np.int64)
    q = np.where((idx > 0)[:, :, None], Q[np.maximum(idx - 1, 0)], 0.0)
    return P[:, None, :] + WT[widx] + q


def neighbour_rows(Ej, idx):
    """[n, k, D]: Ej[idx - 1], a zero row at a pad"""
    Ej, idx = f64(Ej), np.asarray(idx, np.int64)
    return np.where((idx > 0)[:, :, None], Ej[np.maximum(idx - 1, 0)], 0.0)


def attn_fwd(P, Q, WT, v, Ej, idx, widx):
    """-> dict: s (ref, mag), attn (ref, mag, extra), out (ref, mag, extra), h"""
    v = f64(v)
    n, k = np.asarray(idx).shape
    A, D = v.shape[0], f64(Ej).shape[1]
    h = pre_activation(P, Q, WT, idx, widx)
    t = np.maximum(h, 0.0) * v
    s, s_mag = t.sum(2), np.abs(t).sum(2)
    x = s - s.max(1, keepdims=True)
    e = np.exp(x)
    a = e / e.sum(1, keepdims=True)
    err = U32 * np.abs(x) + c_score(A) * U32 * s_mag
    a_extra = a * (err + (a * err).sum(1, keepdims=True))
    E = neighbour_rows(Ej, idx)
    out = (a[:, :, None] * E).sum(1)
    out_mag = (a[:, :, None] * np.abs(E)).sum(1)
    out_extra = ((c_attn(k) * U32 * a + a_extra)[:, :, None] * np.abs(E)).sum(1)
    return {"h": h, "s": (s, s_mag), "attn": (a, a, a_extra), "out": (out, out_mag, out_extra)}


# ============================================================================================================== backward
def dot_da(Ej, idx, dOut):
    """da[v, n] = dOut[v] . Ej[idx - 1], exactly 0 at a pad -> (da, mag)"""
    E, g = neighbour_rows(Ej, idx), f64(dOut)[:, None, :]
    return (g * E).sum(2), (np.abs(g) * np.abs(E)).sum(2)


def softmax_bwd(attn, da, da_mag=None):
    """ds = a (da - sum a da) -> (ds, mag); da_mag: the magnitude of a da formed in the same kernel (default |da|)"""
    a, da = f64(attn), f64(da)
    m = np.abs(da) if da_mag is None else da_mag
    ds = a * (da - (a * da).sum(1, keepdims=True))
    return ds, np.abs(a) * (m + (np.abs(a) * m).sum(1, keepdims=True))


def relu_bits(h):
    """[n, k] int64: bit c set iff h[v, n, c] > 0"""
    A = h.shape[2]
    return ((h > 0).astype(np.int64) << np.arange(A, dtype=np.int64)).sum(2)


def bits_of(word, A):
    """[..., A] 0 / 1 from the integer words"""
    return (np.asarray(word, np.int64)[..., None] >> np.arange(A, dtype=np.int64)) & 1


def source_side(P, Q, WT, v, idx, widx, ds, ds_mag):
    """The source-centric half from ds: dict of dh, dP, dWT, dv as (ref, mag), bits, h."""
    v, widx = f64(v), np.asarray(widx, np.int64)
    h = pre_activation(P, Q, WT, idx, widx)
    pos = h > 0
    dh = ds[:, :, None] * v * pos
    dh_mag = ds_mag[:, :, None] * np.abs(v) * pos
    n_wt, A = f64(WT).shape
    dWT, dWT_mag = np.zeros((n_wt, A)), np.zeros((n_wt, A))
    np.add.at(dWT, widx.reshape(-1), dh.reshape(-1, A))
    np.add.at(dWT_mag, widx.reshape(-1), dh_mag.reshape(-1, A))
    dv = (ds[:, :, None] * h * pos).sum((0, 1))
    dv_mag = (ds_mag[:, :, None] * np.abs(h) * pos).sum((0, 1))
    return {"h": h, "bits": relu_bits(h), "dh": (dh, dh_mag), "dP": (dh.sum(1), dh_mag.sum(1)), "dWT": (dWT, dWT_mag),
            "dv": (dv, dv_mag)}


def scatter_rows(idx, x, x_mag, n_dst):
    """sum of x[v, n, :] into row idx - 1 of every non-pad pair -> (ref, mag)"""
    idx = np.asarray(idx, np.int64).reshape(-1)
    keep = idx > 0
    W = x.shape[-1]
    y, m = np.zeros((n_dst, W)), np.zeros((n_dst, W))
    np.add.at(y, idx[keep] - 1, x.reshape(-1, W)[keep])
    np.add.at(m, idx[keep] - 1, x_mag.reshape(-1, W)[keep])
    return y, m


def multiplicity(idx, n_dst):
    idx = np.asarray(idx, np.int64).reshape(-1)
    return np.bincount(idx[idx > 0] - 1, minlength=n_dst)


def attn_bwd(P, Q, WT, v, Ej, idx, widx, attn, dOut):
    """attn_bwd, both forms, from the kernel's own inputs (attn as stored) -> dict of (ref, mag): da, ds, dh, dP, dWT, dv, dQ,
    dEj; bits, h."""
    n_dst = f64(Ej).shape[0]
    da, da_mag = dot_da(Ej, idx, dOut)
    ds, ds_mag = softmax_bwd(attn, da, da_mag)
    r = source_side(P, Q, WT, v, idx, widx, ds, ds_mag)
    r["da"], r["ds"] = (da, da_mag), (ds, ds_mag)
    r["dQ"] = scatter_rows(idx, r["dh"][0], r["dh"][1], n_dst)
    t = f64(attn)[:, :, None] * f64(dOut)[:, None, :]
    r["dEj"] = scatter_rows(idx, t, np.abs(t), n_dst)
    return r


def attn_pull_da(Ej, idx, attn, dOut, B=None):
    """dEj (+ B) and da of every pair (0 at the pads, which the kernel does not write) -> dEj (ref, mag), da (ref, mag)"""
    t = f64(attn)[:, :, None] * f64(dOut)[:, None, :]
    y, m = scatter_rows(idx, t, np.abs(t), f64(Ej).shape[0])
    if B is not None:
        y, m = y + f64(B), m + np.abs(f64(B))
    return (y, m), dot_da(Ej, idx, dOut)


def attn_bwd_ds(P, Q, WT, v, idx, widx, attn, da):
    """from da as stored (whatever a pad slot holds counts as 0): dict of ds, dP, dWT, dv as (ref, mag), bits"""
    da = np.where(np.asarray(idx) > 0, f64(da), 0.0)
    ds, ds_mag = softmax_bwd(attn, da)
    r = source_side(P, Q, WT, v, idx, widx, ds, ds_mag)
    r["ds"] = (ds, ds_mag)
    return r


def dq_from_list(dest, pair, ds, bits, v, n_dst, B=None):
    """dQ[j] = v (.) sum over the listed entries with dest = j < n_dst of ds[pair] bits[pair] (+ B) -> (ref, mag); B is also
    what attn_seg_dq finds in dQ"""
    v, dest, pair = f64(v), np.asarray(dest, np.int64).reshape(-1), np.asarray(pair, np.int64).reshape(-1)
    keep = dest < n_dst
    p = pair[keep]
    x = f64(ds).reshape(-1)[p][:, None] * bits_of(np.asarray(bits).reshape(-1)[p], v.shape[0])
    y, m = np.zeros((n_dst, v.shape[0])), np.zeros((n_dst, v.shape[0]))
    np.add.at(y, dest[keep], x)
    np.add.at(m, dest[keep], np.abs(x))
    y, m = y * v, m * np.abs(v)
    if B is not None:
        y, m = y + f64(B), m + np.abs(f64(B))
    return y, m


def attn_dq_from_comp(idx, ds, bits, v, n_dst, B=None):
    """attn_pull_dq / attn_seg_dq on a table: every non-pad pair (v, n) is listed at destination idx - 1"""
    idx = np.asarray(idx, np.int64).reshape(-1)
    return dq_from_list(np.where(idx > 0, idx - 1, n_dst), np.arange(idx.size), ds, bits, v, n_dst, B)


# ======================================================================================================= integer kernels
def attn_keys(idx, n_dst):
    idx = np.asarray(idx, np.int64).reshape(-1)
    return np.where(idx > 0, idx - 1, n_dst).astype(np.int32)


def invert(idx, n_dst):
    """The inversion the step does around the kernels: stable sort of the keys -> (skey, order int64, rowptr [n_dst + 1])"""
    key = attn_keys(idx, n_dst)
    order = np.argsort(key, kind="stable").astype(np.int64)
    skey = key[order]
    return skey, order, np.searchsorted(skey, np.arange(n_dst + 1), side="left").astype(np.int64)


def attn_invert_fill(order, attn, k):
    order = np.asarray(order, np.int64)
    return order.astype(np.int32), (order // k).astype(np.int32), np.asarray(attn, np.float32).reshape(-1)[order]


def nbr_gather(idx, widx, rows, pos=None):
    rows = np.asarray(rows, np.int64)
    j = np.asarray(idx, np.int32)[rows]
    return (j if pos is None else np.asarray(pos, np.int32)[j]), np.asarray(widx, np.int32)[rows]


def inv_filter(perm, dest, k, pos_src, pos_dst, attn, n_dst, capacity):
    """-> skey [capacity] (n_dst behind the listed entries), pair, src, val [total], total"""
    perm, dest, pos_src = np.asarray(perm, np.int64), np.asarray(dest, np.int64), np.asarray(pos_src, np.int64)
    row_c = pos_src[perm // k + 1] - 1
    keep = row_c >= 0
    pair = row_c[keep] * k + perm[keep] % k
    d = dest[keep]
    total = int(keep.sum())
    skey = np.full(capacity, n_dst, np.int32)
    skey[:total] = d if pos_dst is None else np.asarray(pos_dst, np.int64)[d + 1] - 1
    return skey, pair.astype(np.int32), row_c[keep].astype(np.int32), np.asarray(attn, np.float32).reshape(-1)[pair], total


# ================================================================================================================ inputs
GRID = 2.0 ** -8                            # P, Q, WT are integer multiples of it, |P| <= 4, |Q|, |WT| <= 2: h is exact in fp32
N_MIN, N_LONG = 70, 1117                    # rows 0 ... 69 carry the planted cases; the long destinations need 10 + 1100 rows
LONG_A, LONG_B = 6, 8                       # destinations of 1100 (3 chunks) and 2 * 512 + 1 pairs in a `long` case


def make_case(n, n_dst, k, D, A, n_wt, seed, spread=False, long=False):
    """Inputs of one attention case as float32 / int32 numpy arrays (dict), with everything the tests look for planted:
      idx   pads in every slot position (row 6 + s, slot s) and at random; row 3 all pads; row 4 lists destination 4 twice;
            row 5 lists destination 5 k times with one weight id (equal logits); destination n_dst - 1 is listed by nobody;
            long: destination LONG_A is listed by 1100 rows (slot 0) and LONG_B by 1025 (slot 1), by nobody else
      widx  any id in [0, n_wt) at any slot, pads included; WT[0] is an ordinary row
      P, Q, WT on the grid (GRID); h == 0 exactly on the whole of pair (8, 0), of the pad pair (9, 3) when k > 3, and in one
            column of the pairs (20 ... 29, 0)
      v, Ej, dOut ordinary signed floats; spread: v scaled so that the logits reach about +-80."""
    assert n >= N_MIN and n_dst >= 12 and (not long or (n >= N_LONG and k >= 2))
    rng = np.random.default_rng(seed)
    idx = rng.integers(0, n_dst, (n, k))
    idx[rng.random((n, k)) < 0.15] = 0
    widx = rng.integers(0, n_wt, (n, k))
    if long:
        idx[(idx == LONG_A + 1) | (idx == LONG_B + 1)] = 1
        idx[10:10 + 1100, 0] = LONG_A + 1
        idx[10:10 + 2 * K_CHUNK + 1, 1] = LONG_B + 1
    idx[3] = 0
    idx[4, 0] = idx[4, min(1, k - 1)] = 5
    idx[5], widx[5] = 6, widx[5, 0]
    for s in range(k):
        idx[6 + s, s] = 0
    if k > 3:
        assert idx[9, 3] == 0
    idx[8, 0] = 3
    idx[20:30, 0] = np.where(idx[20:30, 0] == 0, 2, idx[20:30, 0])

    def grid(shape, lim):
        return (rng.integers(-int(lim / GRID), int(lim / GRID) + 1, shape) * GRID).astype(np.float32)
    P, Q, WT = grid((n, A), 4.0), grid((n_dst, A), 2.0), grid((n_wt, A), 2.0)
    P[8] = -(WT[widx[8, 0]] + Q[idx[8, 0] - 1])
    if k > 3:
        P[9] = -WT[widx[9, 3]]
    for r in range(20, 30):
        c = r % A
        P[r, c] = -(WT[widx[r, 0], c] + Q[idx[r, 0] - 1, c])
    v = (rng.standard_normal(A) * (0.5 / np.sqrt(A)) * (60.0 if spread else 1.0)).astype(np.float32)
    Ej = (rng.standard_normal((n_dst, D)) * 0.5).astype(np.float32)
    dOut = (rng.standard_normal((n, D)) * 0.5).astype(np.float32)
    return {"P": P, "Q": Q, "WT": WT, "v": v, "Ej": Ej, "dOut": dOut, "idx": idx.astype(np.int32), "widx": widx.astype(np.int32),
            "n": n, "n_dst": n_dst, "k": k, "D": D, "A": A, "n_wt": n_wt}
