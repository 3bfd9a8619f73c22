"""Plain fp64 restatement of the fused TGCN dense block of csrc/tgcn_fuse.hip -- one function per entry point (fwd, bwd, wf), each
from that kernel's OWN inputs -- shared by test_gpu_tgcn_fuse_kernels.py and test_tgcn_fuse_ref_host.py (which holds it to torch
autograd of tgcn._dense_block in fp64 and to the oracle).  torch, device-agnostic (the tensors decide), rows in chunks of CHUNK so
that y [n, 32 D + 48] never exists for more than a chunk; no project code.  The operation (A = C = 32, V = 8):

    S_j  = t_j U + q;  s_j = relu(S_j) . p;  bw = softmax_j(s);  e_j = bw_j t_j                     j = 0..2
    y    = [ relu(sum_j wb[c][j] e_j[d]) | relu(W[f] . e) ],  W [48, 3, D] the vector-level filters in the kernel's vec_feature
           order: conv_1 [c][h] (f = 3 c + h: w1[c] on e_h), conv_2 [c][h] (f = 24 + 2 c + h: taps w2[c][0], w2[c][1] on e_h, e_h+1),
           conv_3 [c] (f = 40 + c: w3[c][j] on e_j)
    out  = relu(y Wf + bf)
    bwd  : g = dOut [out > 0] with the `out` GIVEN (the kernel's own forward output: no ambiguity enters there); dy = g Wf^T;
           dfeat = dy_vec [vec > 0]; de_j = sum_c wb[c][j] dy_bit[c] [bit > 0] + sum_f W[f][j] dfeat[f]; db_j = de_j . t_j;
           ds_j = bw_j (db_j - sum_i bw_i db_i); dS_j = ds_j p [S_j > 0]; dt_j = bw_j de_j + U dS_j; yvec = relu(vec);
           small = dwb[c][j] = sum dy_bit[c] [bit > 0] . e_j | dq = sum dS_j | dp = sum ds_j relu(S_j)
    wf   : from T, bw, yvec, wb, out, dOut, dfeat, dS AS GIVEN: dWf = y^T g with y re-formed from T, the given bw and the given yvec
           (only ReLU VALUES enter, no mask: no kink), G[f][j] = sum dfeat[f] e_j, dU = sum_j t_j^T dS_j
    fold : G -> dw1, dw2, dw3 (what _FusedDense._backward_rows does with G)

Every output comes as Out(ref, mag, c, extra) for the rule of spmm_ref.py, |got - ref| <= c 2^-24 mag + extra + 1e-30: `mag` the
fp64 sum of the absolute values of the terms, `c` the rounded fp32 operations on the longest path to the output, `extra` the
first-order propagation of the bounds of the kernel-internal quantities it is formed from (all kernels recompute bw, e, S from T).
A ReLU is 1-Lipschitz: a VALUE behind it carries the error of its argument wherever the argument could be positive, whatever the
kernel's mask was.  A MASK is only compared where it is decided (`undecided`).  The counts, from the operation (u = 2^-24; an fma
rounds once; an MFMA 16x16x4 accumulator that takes K products in K / 4 steps is a sum of K + 1 terms: at most K roundings):

  S            D products through the MFMAs, + q: C_S = D + 1.                                mag = |t| |U| + |q|
  s            a lane's A / 4 = 8 fmas, the 2 levels over the 4 lanes of a node: C_SCORE = 10.       mag = relu(S) . |p|
               extra: |p| . err_S over the elements that can be positive.
               EXACT SUMS.  make_case draws T, U, q, p on grids of powers of two (GRID_T, GRID_U, GRID_P; q on GRID_T GRID_U).
               A sum whose terms are all multiples of g and whose magnitude (the sum of their absolute values) is below 2^24 g
               is exact in fp32 in any order: every partial sum is a multiple of g below 2^24 g.  Where that holds -- checked per
               element, on the grids the restatement FINDS in its inputs (`grid_of`), so inputs off any grid get the counts above
               -- S, s and s - max carry no error, [S > 0] is decided even at S == 0, and bw is left with C_BW alone.  Without
               this the worst-case C_S, C_SCORE leave bw with 1e-3 at D = 128 and more than half of the nodes undecided (one of
               their 4096 bit-level pre-activations within 1e-3 of 0); with it the share stays below UNDECIDED_CAP.
  bw           expf of the numerator (EXPF_U = 8 u, the project's 4-ulp figure), the 3-term denominator of such terms (8 + 2), the
               reciprocal (1 ulp = 2 u), the product (1): C_BW = 21, mag = bw.  The error E_i = err_s_i + u |s_i - max| of the
               exponents (the common shift by the maximum cancels) enters through the slope, d bw_n = bw_n sum_i bw_i (dx_n - dx_i):
               extra = bw_n sum_{i != n} bw_i (E_n + E_i) exp(2 max E)  (the factor: the remainder of exp beyond first order).
               UNDERFLOW.  expf(x) is exactly 0 in fp32 for x < -104, flushed or not, and the restatement sets such a weight to
               0 as well: the kernel's e_j is then 0, its pre-activations w . e_j are 0 and masked, and a restatement that kept
               1e-70 there would see [w . e_j > 0] by the sign of w . t_j -- a different dfeat.  make_case's spread node is
               beyond -110 on two weights.  Between -104 and -86 the result is denormal (kept or flushed): extra + 2^-125.
               (`underflow=False` restates the real-number operation instead: what fp64 autograd computes.)
  e            one product: u |e| + |t| err_bw.
  bit          fma(c0, e0, fma(c1, e1, c2 e2)): C_BIT = 3, mag = sum |wb| |e|; extra |wb| err_e.
  vec          taps D products through the MFMAs: C = D, 2 D, 3 D by group; extra |W| err_e.  This is yvec's bound too.
  out          32 D + 48 products through the MFMAs, + bf: C = 32 D + 49; extra err_y |Wf|.
  dy, dfeat    Dout products through the MFMAs (two accumulators of Dout / 2 and their sum): C_DY = Dout.
  de           32 fmas (bit level), <= 4 taps x 8 filters through the MFMAs (vector level), their sum: C_DE = 65; extra |wb| err_dy
               + |W| err_dfeat on the live elements.
  db           D / 4 fmas of a lane (two halves and their sum in the D = 128 kernel: + 1), 2 levels over the lanes: D / 4 + 3;
               extra err_de . |t|.
  ds           3 products and 2 additions of the mix, the subtraction, the product: on bw_j (|db_j| + sum bw_i |db_i|) C_DS = 5;
               extra from err_db and err_bw.      dS: one more product (1) on |dS|; extra |p| err_ds.
  dt           A products through the MFMAs and the fma: C_DT = A + 1 on bw |de| + |U| |dS|; extra err_bw |de| + bw err_de + |U| err_dS.
  small        LDS float atomics, then the fold over the blocks in turn -- held to the bound only.  With tiles = ceil(n / 16),
               blocks = min(ceil(tiles / 4), 512), it = ceil(tiles / 4 blocks) tiles per wave: a term of dq / dp passes the lane's
               chain (3 it), the 16-lane tree (4), the block's 4 waves into one address (4) and the fold (blocks): c_small =
               3 it + 8 + blocks on top of its own rounding (dS's; dp's fma 1); a term of dwb the lane's chain (D / 4 fmas), the
               tree (6, or 4 and the 4 slots of the D = 128 kernel: 2 more), the additions of the block's waves and tiles into
               one address (4 it, twice in the D = 128 kernel: 8 it) and the fold: c_dwb = D / 4 + 8 + 8 it + blocks.
  wf           rows sit on the MFMA k axis: a node group of `per` rows is one chain (per), the groups are folded in turn (groups),
               `wf_groups` restates the split.  dWf: per + groups, extra err_y^T |g| with err_y = 4 u mag_bit (e's product and the
               3 of bit) where y can be positive; G: + 1 (e's product); dU: three MFMAs per k-step, 3 per + groups.  The vector
               rows, G and dU of an unstaged shape run over their own, finer groups (per_small, small_groups).
  fold         sums of 3 (dw1) or 2 (dw2) entries of G: the same sum of G's bounds, + 2 u resp. 1 u on the absolute values.
"""
import math
from collections import namedtuple

import torch

U32 = 2.0 ** -24
A_, C_, V_ = 32, 32, 8
NF = 6 * V_
EXPF_U = 8
EXP_ZERO, EXP_TINY = -104.0, -86.0       # expf(x) is 0 in fp32 below the first (half the smallest denormal), denormal below ~-87.3
C_SCORE, C_BW, C_BIT, C_DE, C_DS = 10, 2 * EXPF_U + 2 + 2 + 1, 3, 65, 5
CHUNK = 1024
SIZES = (16, 32, 64, 128)
SHAPES = [(D, Dout) for D in SIZES for Dout in SIZES]
WF_GROUPS, WF_SMALL_GROUPS, WF_MERGED_GROUPS = 23, 36, 32           # kWfGroups, kWfSmallGroups, kWfMergedGroups
BWD_BLOCKS = 512                                                    # kFuseBwdBlocks
GRID_T, GRID_U, GRID_P = 2.0 ** -5, 2.0 ** -6, 2.0 ** -4             # make_case: S on 2^-11, s on 2^-15
PARAMS = ("U", "q", "p", "wb", "w1", "w2", "w3", "Wf", "bf")

Out = namedtuple("Out", "ref mag c extra")


def _cdiv(a, b):
    return -(-a // b)


def bound(o):
    return o.c * U32 * o.mag + o.extra


def merged(D, Dout):
    return D in (64, 128) and Dout in (64, 128)


def wf_groups(n, D, Dout):
    """(per, groups, per_small, small_groups) of launch_fuse_wf: rows per node group (a multiple of 8) and the groups that hold a
    row, for the heavy products and for the light ones (a merged shape carries them in the heavy groups)."""
    def split(want):
        groups = max(min(_cdiv(n, 256), want), 1)
        per = _cdiv(_cdiv(n, groups), 8) * 8
        return per, _cdiv(n, per)
    if merged(D, Dout):
        per, groups = split(WF_MERGED_GROUPS)
        return per, groups, per, groups
    return (*split(WF_GROUPS), *split(WF_SMALL_GROUPS))


def c_small(n, D):
    """(c of dq and dp, c of dwb) on top of the terms' own rounding (header)"""
    tiles = _cdiv(n, 16)
    blocks = min(_cdiv(tiles, 4), BWD_BLOCKS)
    it = _cdiv(tiles, 4 * blocks)
    return 3 * it + 8 + blocks, D // 4 + 8 + 8 * it + blocks


def grid_of(*xs):
    """the largest 2^-k, k <= 40, that every element of every tensor is a multiple of; 0.0 if there is none"""
    for k in range(41):
        g = 2.0 ** -k
        if all(bool((x.detach().double() / g == (x.detach().double() / g).round()).all()) for x in xs):
            return g
    return 0.0


def vec_weight(w1, w2, w3):
    """W [48, 3, D]: the weight of vector feature f on e_j, and taps [48] (rows of e a feature spans)"""
    D = w1.reshape(V_, -1).shape[1]
    w1, w2, w3 = w1.reshape(V_, D), w2.reshape(V_, 2, D), w3.reshape(V_, 3, D)
    W = w1.new_zeros(NF, 3, D)
    taps = w1.new_zeros(NF)
    for c in range(V_):
        for h in range(3):
            W[3 * c + h, h] = w1[c]
            taps[3 * c + h] = 1
        for h in range(2):
            W[3 * V_ + 2 * c + h, h] = w2[c, 0]
            W[3 * V_ + 2 * c + h, h + 1] = w2[c, 1]
            taps[3 * V_ + 2 * c + h] = 2
        W[5 * V_ + c] = w3[c]
        taps[5 * V_ + c] = 3
    return W, taps


def fold(G):
    """G [48, 3, D] -> dw1 [V, D], dw2 [V, 2 D], dw3 [V, 3 D]: feature (c, h) of conv_k reads its tap a from e_{h + a}"""
    D = G.shape[2]
    dw1, dw2, dw3 = G.new_zeros(V_, D), G.new_zeros(V_, 2, D), G.new_zeros(V_, 3, D)
    for c in range(V_):
        for h in range(3):
            dw1[c] += G[3 * c + h, h]
        for h in range(2):
            for a in range(2):
                dw2[c, a] += G[3 * V_ + 2 * c + h, h + a]
        for a in range(3):
            dw3[c, a] = G[5 * V_ + c, a]
    return dw1, dw2.reshape(V_, 2 * D), dw3.reshape(V_, 3 * D)


def fold_out(G):
    """fold of an Out -> (dw1, dw2, dw3) as Outs: the bound of a sum is the sum of the bounds, + its own additions"""
    refs, mags, bnds = fold(G.ref), fold(G.ref.abs()), fold(bound(G) + 0 * G.ref)
    return tuple(Out(r, m, c, b) for r, m, c, b in zip(refs, mags, (2, 1, 0), bnds))


# ================================================================================================================ rows
def _prm(P):
    """the nine parameters in fp64, in the kernels' layouts, + the vector-level filter table"""
    d = {k: P[k].detach().double() for k in PARAMS}
    d["q"], d["p"], d["bf"], d["wb"] = d["q"].reshape(-1), d["p"].reshape(-1), d["bf"].reshape(-1), d["wb"].reshape(C_, 3)
    d["W"], d["taps"] = vec_weight(d["w1"], d["w2"], d["w3"])
    d["gU"], d["gq"], d["gp"] = grid_of(d["U"]), grid_of(d["q"]), grid_of(d["p"])
    return d


def _stack(T0, T1, T2, lo, hi):
    return torch.stack([T0[lo:hi].detach().double(), T1[lo:hi].detach().double(), T2[lo:hi].detach().double()], dim=1)


def _features(t, d, gT, underflow=True):
    """everything up to y of the rows t [m, 3, D]: values, magnitudes and error bounds of what the kernels recompute; gT: the
    grid of T (grid_of)"""
    D = t.shape[2]
    r = {}
    gS = min(gT * d["gU"], d["gq"])                                  # S = t U + q is a sum of multiples of gS
    gs = gS * d["gp"]                                                # s = relu(S) . p of multiples of gs, where S is exact
    S = t @ d["U"] + d["q"]
    S_mag = t.abs() @ d["U"].abs() + d["q"].abs()
    S_exact = S_mag < 2.0 ** 24 * gS
    S_err = torch.where(S_exact, 0 * S_mag, (D + 1) * U32 * S_mag)
    rS = torch.relu(S)
    s, s_mag = rS @ d["p"], rS @ d["p"].abs()
    s_exact = S_exact.all(2) & (s_mag < 2.0 ** 24 * gs)
    s_err = torch.where(s_exact, 0 * s_mag, C_SCORE * U32 * s_mag + (S_err * (S + S_err > 0)) @ d["p"].abs())
    x = s - s.max(1, keepdim=True).values
    ex = torch.where(x < (EXP_ZERO if underflow else -math.inf), 0 * x, torch.exp(x))      # fp32's expf: exactly 0 (header)
    bw = ex / ex.sum(1, keepdim=True)
    E = s_err + torch.where(s_exact.all(1, keepdim=True), 0 * x, U32 * x.abs())
    tot = (bw * E).sum(1, keepdim=True)
    bw_extra = bw * ((1 - bw) * E + tot - bw * E) * torch.exp(2 * E.max(1, keepdim=True).values)
    bw_extra = bw_extra + ((x >= EXP_ZERO) & (x < EXP_TINY)) * (2.0 ** -125 if underflow else 0.0)
    bw_err = C_BW * U32 * bw + bw_extra
    e = bw[:, :, None] * t
    e_err = U32 * e.abs() + t.abs() * bw_err[:, :, None]
    wb, W = d["wb"], d["W"]
    bit = torch.einsum("cj,njd->ncd", wb, e)
    bit_mag = torch.einsum("cj,njd->ncd", wb.abs(), e.abs())
    bit_err = C_BIT * U32 * bit_mag + torch.einsum("cj,njd->ncd", wb.abs(), e_err)
    vec = torch.einsum("fjd,njd->nf", W, e)
    vec_mag = torch.einsum("fjd,njd->nf", W.abs(), e.abs())
    vec_extra = torch.einsum("fjd,njd->nf", W.abs(), e_err)
    vec_err = d["taps"] * D * U32 * vec_mag + vec_extra
    r.update(S=S, S_mag=S_mag, S_err=S_err, s=s, bw=bw, bw_extra=bw_extra, bw_err=bw_err, e=e, e_err=e_err, bit=bit, bit_mag=bit_mag,
             bit_err=bit_err, vec=vec, vec_mag=vec_mag, vec_extra=vec_extra, vec_err=vec_err)
    return r


def _undecided_rows(r):
    """a mask of the backward pass is open: a recomputed pre-activation within its bound of 0.  An exact 0 of zero magnitude (an
    all-zero input row) has bound 0 and is decided: both sides give gradient 0."""
    und = torch.zeros(r["S"].shape[0], dtype=torch.bool, device=r["S"].device)
    for v, err in ((r["S"], r["S_err"]), (r["bit"], r["bit_err"]), (r["vec"], r["vec_err"])):          # (an exact S: err 0)
        und |= ((v.abs() <= err) & (err > 0)).flatten(1).any(1)
    return und


def _cat(parts):
    """list of dicts of Out-like tuples (ref, mag, c, extra) per chunk -> dict of Outs over all rows (c is chunk-independent)"""
    out = {}
    for k in parts[0]:
        ref, mag, c, extra = zip(*[p[k] for p in parts])
        out[k] = Out(torch.cat(ref), torch.cat(mag), c[0], torch.cat(extra))
    return out


# ============================================================================================================= forward
def fwd(T0, T1, T2, P, chunk=CHUNK, underflow=True):
    """-> dict of Outs: bw [n, 3], out [n, Dout], the pre-activations S [n, 3, A], bit [n, 32, D] (only for n <= chunk: it is the
    size of y), vec [n, 48], pre_out [n, Dout]; and `undecided` bool [n]"""
    d = _prm(P)
    n, D = T0.shape
    K = C_ * D
    parts, und = [], []
    gT = grid_of(T0, T1, T2)
    for lo in range(0, n, chunk):
        t = _stack(T0, T1, T2, lo, min(lo + chunk, n))
        r = _features(t, d, gT, underflow)
        m = t.shape[0]
        yb, yv = torch.relu(r["bit"]).reshape(m, K), torch.relu(r["vec"])
        yb_err = (r["bit_err"] * (r["bit"] + r["bit_err"] > 0)).reshape(m, K)
        yv_err = r["vec_err"] * (r["vec"] + r["vec_err"] > 0)
        Wf, Wa = d["Wf"], d["Wf"].abs()
        pre = yb @ Wf[:K] + yv @ Wf[K:] + d["bf"]
        pre_mag = yb @ Wa[:K] + yv @ Wa[K:] + d["bf"].abs()
        pre_extra = yb_err @ Wa[:K] + yv_err @ Wa[K:]
        c_out = K + NF + 1
        p = {"bw": (r["bw"], r["bw"], C_BW, r["bw_extra"]),
             "S": (r["S"], r["S_mag"], D + 1, 0 * r["S"]),
             "vec": (r["vec"], r["vec_mag"], d["taps"] * D, r["vec_extra"]),
             "pre_out": (pre, pre_mag, c_out, pre_extra),
             "out": (torch.relu(pre), pre_mag, c_out, pre_extra)}
        if n <= chunk:
            p["bit"] = (r["bit"], r["bit_mag"], C_BIT, r["bit_err"] - C_BIT * U32 * r["bit_mag"])
        parts.append(p)
        und.append(_undecided_rows(r))
    res = _cat(parts)
    res["undecided"] = torch.cat(und)
    return res


def undecided(T0, T1, T2, P, chunk=CHUNK):
    """bool [n]: the nodes with an open mask (see _undecided_rows); the tests give them dOut = 0"""
    d, gT = _prm(P), grid_of(T0, T1, T2)
    return torch.cat([_undecided_rows(_features(_stack(T0, T1, T2, lo, min(lo + chunk, T0.shape[0])), d, gT))
                      for lo in range(0, T0.shape[0], chunk)])


# ============================================================================================================ backward
def bwd(T0, T1, T2, P, out, dOut, chunk=CHUNK, underflow=True):
    """-> dict of Outs: dT0, dT1, dT2 [n, D], yvec, dfeat [n, 48], dS [n, 3 A], ds [n, 3] (kernel-internal), dwb [32, 3], dq, dp [A]"""
    d = _prm(P)
    n, D = T0.shape
    Dout = d["Wf"].shape[1]
    K = C_ * D
    c_qp, c_wb = c_small(n, D)
    parts = []
    acc = {k: 0.0 for k in ("dwb", "dwb_mag", "dwb_x", "dq", "dq_mag", "dq_x", "dp", "dp_mag", "dp_x")}
    Wf, Wa, U, W, wb, p = d["Wf"], d["Wf"].abs(), d["U"], d["W"], d["wb"], d["p"]
    gT = grid_of(T0, T1, T2)
    for lo in range(0, n, chunk):
        hi = min(lo + chunk, n)
        t = _stack(T0, T1, T2, lo, hi)
        m = hi - lo
        r = _features(t, d, gT, underflow)
        bw, bw_err, e = r["bw"], r["bw_err"], r["e"]
        g = dOut[lo:hi].detach().double() * (out[lo:hi] > 0)
        dy, dy_mag = g @ Wf.t(), g.abs() @ Wa.t()
        dy_err = Dout * U32 * dy_mag
        bpos, vpos = r["bit"] > 0, r["vec"] > 0
        dbit, dbit_mag, dbit_err = (x[:, :K].reshape(m, C_, D) * bpos for x in (dy, dy_mag, dy_err))
        dfeat, dfeat_mag, dfeat_err = (x[:, K:] * vpos for x in (dy, dy_mag, dy_err))
        de = torch.einsum("cj,ncd->njd", wb, dbit) + torch.einsum("fjd,nf->njd", W, dfeat)
        de_mag = torch.einsum("cj,ncd->njd", wb.abs(), dbit.abs()) + torch.einsum("fjd,nf->njd", W.abs(), dfeat.abs())
        de_err = C_DE * U32 * de_mag + torch.einsum("cj,ncd->njd", wb.abs(), dbit_err) + torch.einsum("fjd,nf->njd", W.abs(), dfeat_err)
        db, db_mag = (de * t).sum(2), (de.abs() * t.abs()).sum(2)
        db_err = (D // 4 + 3) * U32 * db_mag + (de_err * t.abs()).sum(2)
        mix = (bw * db).sum(1, keepdim=True)
        ds = bw * (db - mix)
        ds_mag = bw * (db.abs() + (bw * db.abs()).sum(1, keepdim=True))
        ds_extra = (bw * (db_err + (bw * db_err).sum(1, keepdim=True)) + bw_err * (db - mix).abs()
                    + bw * (bw_err * db.abs()).sum(1, keepdim=True))
        ds_err = C_DS * U32 * ds_mag + ds_extra
        spos = r["S"] > 0
        dS = spos * ds[:, :, None] * p
        dS_extra = spos * p.abs() * ds_err[:, :, None]
        dS_err = U32 * dS.abs() + dS_extra
        dt = bw[:, :, None] * de + dS @ U.t()
        dt_mag = bw[:, :, None] * de.abs() + dS.abs() @ U.abs().t()
        dt_extra = bw_err[:, :, None] * de.abs() + bw[:, :, None] * de_err + dS_err @ U.abs().t()
        yv_err = r["vec_extra"] * (r["vec"] + r["vec_err"] > 0)
        pt = {f"dT{j}": (dt[:, j], dt_mag[:, j], A_ + 1, dt_extra[:, j]) for j in range(3)}
        pt.update(yvec=(torch.relu(r["vec"]), r["vec_mag"], d["taps"] * D, yv_err), dfeat=(dfeat, dfeat_mag, Dout, 0 * dfeat),
                  dS=(dS.reshape(m, 3 * A_), dS.abs().reshape(m, 3 * A_), 1, dS_extra.reshape(m, 3 * A_)), ds=(ds, ds_mag, C_DS, ds_extra))
        parts.append(pt)
        rS = torch.relu(r["S"])
        acc["dq"] += dS.sum((0, 1)); acc["dq_mag"] += dS.abs().sum((0, 1)); acc["dq_x"] += dS_err.sum((0, 1))
        acc["dp"] += (ds[:, :, None] * rS).sum((0, 1)); acc["dp_mag"] += (ds.abs()[:, :, None] * rS).sum((0, 1))
        acc["dp_x"] += (ds_err[:, :, None] * rS + ds.abs()[:, :, None] * r["S_err"] * (r["S"] + r["S_err"] > 0)).sum((0, 1))
        acc["dwb"] += torch.einsum("ncd,njd->cj", dbit, e); acc["dwb_mag"] += torch.einsum("ncd,njd->cj", dbit.abs(), e.abs())
        acc["dwb_x"] += torch.einsum("ncd,njd->cj", dbit_err, e.abs()) + torch.einsum("ncd,njd->cj", dbit.abs(), r["e_err"])
    res = _cat(parts)
    res["dq"] = Out(acc["dq"], acc["dq_mag"], c_qp, acc["dq_x"])
    res["dp"] = Out(acc["dp"], acc["dp_mag"], c_qp + 1, acc["dp_x"])
    res["dwb"] = Out(acc["dwb"], acc["dwb_mag"], c_wb + 1, acc["dwb_x"])
    return res


# ==================================================================================================== weight gradients
def wf(T0, T1, T2, bw, yvec, wb, out, dOut, dfeat, dS, chunk=CHUNK):
    """-> dict of Outs: dWf [32 D + 48, Dout], G [48, 3, D], dU [D, A], every input as given"""
    n, D = T0.shape
    Dout = out.shape[1]
    K = C_ * D
    wb = wb.detach().double().reshape(C_, 3)
    per, groups, per_s, groups_s = wf_groups(n, D, Dout)
    z = lambda *s: torch.zeros(*s, dtype=torch.float64, device=T0.device)
    dWf, dWf_mag, dWf_x = z(K + NF, Dout), z(K + NF, Dout), z(K + NF, Dout)
    G, G_mag, dU, dU_mag = z(NF, 3, D), z(NF, 3, D), z(D, A_), z(D, A_)
    for lo in range(0, n, chunk):
        hi = min(lo + chunk, n)
        t = _stack(T0, T1, T2, lo, hi)
        m = hi - lo
        e = bw[lo:hi].detach().double()[:, :, None] * t
        bit = torch.einsum("cj,njd->ncd", wb, e)
        bit_err = (1 + C_BIT) * U32 * torch.einsum("cj,njd->ncd", wb.abs(), e.abs())
        y = torch.cat([torch.relu(bit).reshape(m, K), yvec[lo:hi].detach().double()], dim=1)
        y_err = (bit_err * (bit + bit_err > 0)).reshape(m, K)
        g = dOut[lo:hi].detach().double() * (out[lo:hi] > 0)
        dWf += y.t() @ g
        dWf_mag += y.abs().t() @ g.abs()
        dWf_x[:K] += y_err.t() @ g.abs()
        df, s3 = dfeat[lo:hi].detach().double(), dS[lo:hi].detach().double().reshape(m, 3, A_)
        G += torch.einsum("nf,njd->fjd", df, e)
        G_mag += torch.einsum("nf,njd->fjd", df.abs(), e.abs())
        dU += torch.einsum("njd,nja->da", t, s3)
        dU_mag += torch.einsum("njd,nja->da", t.abs(), s3.abs())
    c_wf = torch.full((K + NF, 1), float(per + groups), dtype=torch.float64, device=T0.device)
    c_wf[K:] = per_s + groups_s
    return {"dWf": Out(dWf, dWf_mag, c_wf, dWf_x), "G": Out(G, G_mag, per_s + groups_s + 1, 0 * G),
            "dU": Out(dU, dU_mag, 3 * per_s + groups_s, 0 * dU)}


def masked_colsum(out, dOut):
    """dbf = column sums of dOut [out > 0]: whatever the order, a term passes at most n - 1 additions"""
    g = dOut.detach().double() * (out > 0)
    return Out(g.sum(0), g.abs().sum(0), max(out.shape[0] - 1, 0), 0 * g.sum(0))


# ============================================================================================================== inputs
def make_case(n, D, Dout, seed, spread=True, device="cpu"):
    """Inputs of one case, float32 (the scales of test_gpu_tgcn.py::test_fused_dense_block_vs_operator_form): dict of T0, T1, T2
    [n, D], the nine parameters in the kernels' layouts, dOut [n, Dout], and `plant` (what was planted where).  T, U, q, p are
    rounded to their grids (header: exact sums); everything else is an ordinary float.  As n allows:
      node n - 1   all three vectors zero (S = q, every convolution exactly 0 with zero magnitude)
      node n - 2   exactly one of its three vectors zero (the item-side one)
      node 0 ...   spread: the node among the first 64 whose scores are best separated has its rows scaled by a power of two
                   until they spread by more than 110: two soft-max weights underflow in fp32.  Its dOut row is scaled back by
                   the same factor, so that it does not own the sums over nodes.
      dOut         rows 5, 16, 27, ... all zero; dense otherwise, so every exactly-zero entry of `out` (a ReLU output: about
                   half of them) is met by a non-zero dOut."""
    g = torch.Generator().manual_seed(seed)
    rn = lambda *s, sc=1.0, grid=0.0: torch.randn(*s, generator=g) * sc if not grid else torch.round(torch.randn(*s, generator=g) * sc / grid) * grid
    c = {"T0": rn(n, D, sc=0.5, grid=GRID_T), "T1": rn(n, D, sc=0.5, grid=GRID_T), "T2": rn(n, D, sc=0.5, grid=GRID_T),
         "U": rn(D, A_, sc=0.2, grid=GRID_U), "q": rn(A_, sc=0.1, grid=GRID_T * GRID_U), "p": rn(A_, grid=GRID_P), "wb": rn(C_, 3, sc=0.5), "w1": rn(V_, D, sc=0.2),
         "w2": rn(V_, 2 * D, sc=0.2), "w3": rn(V_, 3 * D, sc=0.2), "Wf": rn(C_ * D + NF, Dout, sc=0.05), "bf": rn(Dout, sc=0.1),
         "dOut": rn(n, Dout)}
    plant = {}
    if n >= 2:
        for k in ("T0", "T1", "T2"):
            c[k][n - 1] = 0
        plant["zero"] = n - 1
    if n >= 3:
        c["T1"][n - 2] = 0
        plant["one_zero"] = n - 2
    if spread and n >= 4:
        m = min(n - 2, 64)
        s = torch.relu(_stack(c["T0"], c["T1"], c["T2"], 0, m) @ c["U"].double() + c["q"].double()) @ c["p"].double()
        top = s.topk(2, dim=1).values
        i = int(((top[:, 0] - top[:, 1]) / (top[:, 0].abs() + 1e-30)).argmax())
        f = 64.0
        while True:
            s = torch.relu(torch.stack([c[k][i].double() * f for k in ("T0", "T1", "T2")]) @ c["U"].double() + c["q"].double()) @ c["p"].double()
            top = s.topk(2).values
            if top[0] - top[1] > 110 or f >= 2.0 ** 20:
                break
            f *= 2
        for k in ("T0", "T1", "T2"):
            c[k][i] *= f
        c["dOut"][i] /= f
        plant["spread"], plant["spread_gap"] = i, float(top[0] - top[1])
    c["dOut"][5::11] = 0
    c = {k: v.to(device) for k, v in c.items()}
    c.update(n=n, D=D, Dout=Dout, plant=plant)
    return c


def decided_case(n, D, Dout, seed, device="cpu", tries=20):
    """make_case with the first seed of seed, seed + 1000, ... at which no node is undecided (for the cases of fewer than 64 nodes)"""
    for k in range(tries):
        c = make_case(n, D, Dout, seed + 1000 * k, device=device)
        if not bool(undecided(c["T0"], c["T1"], c["T2"], c).any()):
            return c
    raise AssertionError(f"no seed without an undecided node: n={n} D={D} Dout={Dout}")


# ===================================================================================== the cases of the GPU file, in one place
LADDER = (1, 15, 16, 17, 63, 64, 65, 129, 257)
LOOP2_FWD = [(16, 16, 65536 + 33), (64, 16, 32768 + 17), (64, 64, 32768 + 17)]      # NS = 2, NS = 1, the LDS-staged kernel
LOOP2_BWD = [(16, 16, 32768 + 17), (64, 64, 32768 + 17), (128, 64, 32768 + 17)]     # LDSW = false, LDSW = true, bwd2
WF_EDGE_SHAPES = [(32, 16), (64, 64), (128, 128)]                                   # unstaged, merged, merged with NH = 2
DROP_SHAPES = [(16, 16), (64, 16), (64, 64)]                                        # one per forward variant
DROP_N, FOLD_N = 203, 77
UNDECIDED_CAP = 0.05


def wf_edge_ns(D, Dout):
    caps = (WF_MERGED_GROUPS,) if merged(D, Dout) else (WF_GROUPS, WF_SMALL_GROUPS)
    return (1, 7, 9, 257) + tuple(cap * 256 + 1 for cap in caps)


def gpu_case(n, D, Dout, device="cpu"):
    """the inputs of case (n, D, Dout) of test_gpu_tgcn_fuse_kernels.py; below 64 nodes the seed is moved until none is undecided"""
    seed = 7 + 131 * D + 17 * Dout + n
    return decided_case(n, D, Dout, seed, device=device) if n < 64 else make_case(n, D, Dout, seed, device=device)


def gpu_cases():
    """every (n, D, Dout) the GPU file draws"""
    cases = {(n, D, Dout) for D, Dout in SHAPES for n in LADDER + (FOLD_N,)}
    cases |= {(n, D, Dout) for D, Dout, n in LOOP2_FWD + LOOP2_BWD}
    cases |= {(n, D, Dout) for D, Dout in WF_EDGE_SHAPES for n in wf_edge_ns(D, Dout)}
    cases |= {(DROP_N, D, Dout) for D, Dout in DROP_SHAPES}
    return sorted(cases)
