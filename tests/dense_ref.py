"""Plain fp64 restatements of the exact-fp32 MFMA dense kernels -- csrc/ngcf.hip (the dense half of an NGCF layer: fwd, bwd plain
and with the normalize-backward folded in, wgrad) and csrc/proj.hip (tall_mm, tall_mm_adam, tall_wgrad, small_mm, masked_colsum)
-- one function per entry point, each from that kernel's OWN inputs; shared by test_gpu_ngcf_kernels.py, test_gpu_proj_kernels.py
and test_dense_ref_host.py (which holds them to torch autograd in fp64, to the oracle and to torch.optim.Adam, and their bounds to
planted defects).  torch, device-agnostic (the tensors decide), rows in chunks of CHUNK; no project code.  The operations:

    fwd   : P1 = (N + X) W1p, P2 = (N * X) W2p;  Xp = lrelu(P1) + lrelu(P2), slope 0.2 (slope at exactly 0: 0.2);
            inv = 1 / max(||Xp||, 1e-12);  Z = Xp / max(||Xp||, 1e-12)
    bwd   : g = G (may be None) [+ inv (dZ - z (z . dZ)), z = Xp inv, with Xp, inv, dZ AS GIVEN; the dot dropped where inv >= 1e12f,
            the whole term dropped where dz_flags is 0];  dP1 = g lrelu'(P1), dP2 = g lrelu'(P2) with P recomputed from N, X;
            dA1 = dP1 W1p^T, dA2 = dP2 W2p^T;  dN = dA1 + dA2 * X, dXd = dA1 + dA2 * N.  Rows outside row_mask: nothing read.
    wgrad : dW1p = (N + X)^T dP1, dW2p = (N * X)^T dP2 over the rows inside row_mask, dP AS GIVEN
    tall_mm : Y = [X1 | X2][sel] W + [b1 | b2] (+ what Y held);  tall_mm_adam: torch.optim.Adam's step on the gradient G_in + X W
    tall_wgrad : dW = X^T [dY1 | dY2] (+ dW), db = column sums of [dY1 | dY2] (+ db)
    small_mm : C = A B (+ C);   masked_colsum : column sums of dOut [out > 0]

Every output comes as Out(ref, mag, c, extra) for the rule of spmm_ref.Chk, |got - ref| <= c 2^-24 mag + extra + 1e-30: `mag` the
fp64 sum of the absolute values of the terms, `c` the rounded fp32 operations on the longest path to the output, `extra` the
first-order propagation of the bounds of the kernel-internal quantities it is formed from.  LeakyReLU is 1-Lipschitz: a VALUE
behind it carries the error of its argument and needs no mask.  Its SLOPE in the backward is only compared where it is decided
(`undecided`).  The counts (u = 2^-24; an fma rounds once; an MFMA 16x16x4 accumulator that takes K products is a sum of K terms
onto its initial value: at most K roundings):

  P1, P2     N + X resp. N * X (1), Din products through the MFMAs: C_P = Din + 1.          mag = |N + X| |W1p|, |N * X| |W2p|
             (N = -X: the operand is exactly 0 in fp32 as well, P1 = 0 with magnitude 0; N = 0 likewise for P2)
  Xp         C_P, the product by the slope (1) and that the float 0.2f is not 0.2 (1), the sum (1): Din + 4.   mag = mag P1 + mag P2
  inv        ss: a lane's Dout / 4 fmas and the 2 xor levels, halved by sqrtf; sqrtf, the divide (the float 1e-12f on a clamped
             row is within them): ceil((Dout / 4 + 2) / 2) + 2 on mag = inv; extra inv k C_Xp u, k = sum |Xp| mag_Xp / sum Xp^2
             the condition of the row norm (spmm_ref._norm_condition)
  Z          the same count (ss, sqrtf, the divide) on |Z|; extra inv err_Xp + |Z| k C_Xp u
  g (NORM)   z = Xp inv (1), the dot's Dout / 4 fmas and 2 xor levels, z dot (1), the subtraction (1), the product by inv (1), the
             addition to G (1): C_G = Dout / 4 + 7 on |G| + inv (|dZ| + |z| sum |z dZ|)  (spmm_ref.ref_norm_bwd).  Plain: g = G, 0.
  dP         g times the slope (1) and the float 0.2f (1): C_G + 2 on mag_g slope
  dN, dXd    Dout products through the MFMAs, dA2 * X (1), the sum (1): Dout + 2 on |dP1| |W1p|^T + (|dP2| |W2p|^T) |X|;
             extra err_dP1 |W1p|^T + (err_dP2 |W2p|^T) |X|.  (128 -> 128 forms the same sum through memory: same count.)
  dW1p, dW2p rows sit on the MFMA k axis; `wgrad_split` restates launch_wgrad: a wave's chain of 4 per rows (4 per), the 16-way
             strided fold over the waves (ceil(waves / 16)), the 16 partial sums (16), the operand's own rounding (1)
  tall_mm    K products onto the bias (K), the addition of what Y held (1): K + 1 on |X| |W| + |b| + |old|
  tall_mm_adam  the convention of test_gpu_rowops.py -- p: 12 (m 2 + the float 1 - b1; v 3 + the float 1 - b2, halved by sqrtf, the
             float sqrt(bc2), the divide, + eps; m / denom; the float step size; the last fma) on |p| + max(lr, step_size mag_m /
             denom); m: 3 on mag_m = |m| + (1 - b1)(|g| + |m|); v: 4 on v -- and the gradient's own bound e_g propagated: extra =
             the larger move of the fp64 update evaluated at g + e_g and g - e_g
  tall_wgrad `tall_wgrad_split` restates wgrad_waves: 4 spw + ceil(waves / 16) + 16 (+ 1 when added to what dW / db held); db rides
             along as one more MFMA row block (the same count)
  small_mm   K fmas (+ 1 when accumulated);   masked_colsum: a thread's ceil(n / (blocks rpp)) additions, the block's rpp rows
             (rpp), proj_fold's ceil(blocks / 16) + 16
"""
import math
from collections import namedtuple

import torch

U32 = 2.0 ** -24
CHUNK = 1024
SLOPE = 0.2
EPS = 1e-12
INV_CLAMPED = float(torch.tensor(1e12, dtype=torch.float32))      # what 1.0f / 1e-12f rounds to: the kernels test inv >= 1e12f
SIZES = (16, 32, 64, 128)
SHAPES = [(a, b) for a in SIZES for b in SIZES]
WGRAD_WAVES, TALL_WAVES = 2048, 2048          # kWgradWaves (ngcf.hip), kWgradWaveCap (proj.hip)
COLSUM_BLOCKS = 1024                          # kColsumBlocks
UNDECIDED_CAP = 0.05

Out = namedtuple("Out", "ref mag c extra")


def _cdiv(a, b):
    return -(-a // b)


def bound(o):
    return o.c * U32 * o.mag + o.extra


def _d(t):
    return t.detach().double()


def _keep(mask, n, device):
    return torch.ones(n, dtype=torch.bool, device=device) if mask is None else mask.to(device) != 0


def _rows(t, lo, hi, keep):
    """rows [lo, hi) in fp64, the rows outside `keep` as zeros (they may hold NaN: the kernels do not read them)"""
    x = _d(t[lo:hi])
    k = keep[lo:hi]
    return torch.where(k.reshape(-1, *([1] * (x.dim() - 1))), x, torch.zeros_like(x))


def lrelu(x, slope=SLOPE):
    return torch.where(x > 0, x, slope * x)


def _pre(nn, x, W1, W2):
    a1, a2 = nn + x, nn * x
    return a1 @ W1, a1.abs() @ W1.abs(), a2 @ W2, a2.abs() @ W2.abs()


def _cat(parts):
    out = {}
    for k in parts[0]:
        ref, mag, c, extra = zip(*[p[k] for p in parts])
        out[k] = Out(torch.cat(ref), torch.cat(mag), c[0], torch.cat(extra))
    return out


# ============================================================================================================ NGCF layer
def ngcf_fwd(N, X, W1p, W2p, row_mask=None, chunk=CHUNK, slope=SLOPE):
    """-> dict of Outs: Xp [n, Dout], inv [n], Z [n, Dout], the pre-activations P1, P2 [n, Dout]; and `undecided` bool [n].
    Rows outside row_mask are computed from zeros (the kernel leaves their slots alone: the caller compares the rest)."""
    W1, W2 = _d(W1p), _d(W2p)
    Din, Dout = W1.shape
    n = N.shape[0]
    keep = _keep(row_mask, n, N.device)
    c_p, c_xp = Din + 1, Din + 4
    c_inv = _cdiv(Dout // 4 + 2, 2) + 2
    parts, und = [], []
    for lo in range(0, max(n, 1), chunk):
        hi = min(lo + chunk, n)
        nn, x = _rows(N, lo, hi, keep), _rows(X, lo, hi, keep)
        P1, m1, P2, m2 = _pre(nn, x, W1, W2)
        xp, xm = lrelu(P1, slope) + lrelu(P2, slope), m1 + m2
        xe = c_xp * U32 * xm
        ss = (xp * xp).sum(1)
        k = torch.where(ss > 0, (xp.abs() * xm).sum(1) / ss.clamp_min(1e-300), torch.ones_like(ss))
        inv = 1.0 / ss.sqrt().clamp_min(EPS)
        z = xp * inv[:, None]
        rel = k * c_xp * U32
        parts.append({"Xp": (xp, xm, c_xp, 0 * xp), "inv": (inv, inv, c_inv, inv * rel),
                      "Z": (z, z.abs(), c_inv, inv[:, None] * xe + z.abs() * rel[:, None]),
                      "P1": (P1, m1, c_p, 0 * P1), "P2": (P2, m2, c_p, 0 * P2)})
        und.append(_undecided_rows(P1, m1, P2, m2, c_p))
    res = _cat(parts)
    res["undecided"] = torch.cat(und)
    return res


def _undecided_rows(P1, m1, P2, m2, c_p):
    """a slope of the backward pass is open: a recomputed pre-activation within its bound of 0, the bound not 0.  An exact 0 of
    zero magnitude is decided: the kernel and torch both give the slope 0.2 there."""
    e1, e2 = c_p * U32 * m1, c_p * U32 * m2
    return (((P1.abs() <= e1) & (e1 > 0)) | ((P2.abs() <= e2) & (e2 > 0))).any(1)


def undecided(N, X, W1p, W2p, row_mask=None, chunk=CHUNK):
    """bool [n]: the rows with an open slope; the tests give them G = 0 and dZ = 0 (rows outside row_mask are never open)"""
    W1, W2 = _d(W1p), _d(W2p)
    n = N.shape[0]
    keep = _keep(row_mask, n, N.device)
    und = [_undecided_rows(*_pre(_rows(N, lo, min(lo + chunk, n), keep), _rows(X, lo, min(lo + chunk, n), keep), W1, W2), W1.shape[0] + 1)
           for lo in range(0, max(n, 1), chunk)]
    return torch.cat(und)


def ngcf_bwd(G, Xp, inv, dZ, dz_flags, N, X, W1p, W2p, row_mask=None, chunk=CHUNK, slope=SLOPE):
    """-> dict of Outs dP1, dP2 [n, Dout], dN, dXd [n, Din], every input as given.  Xp None: the plain form (g = G, which is then
    required); otherwise the normalize-backward of (Xp, inv, dZ) is added to G (None: no such term) on the rows whose dz_flags
    byte is not 0 (dz_flags None: all).  dZ: the [n, Dout] view of the slot."""
    W1, W2 = _d(W1p), _d(W2p)
    Din, Dout = W1.shape
    n = N.shape[0]
    keep = _keep(row_mask, n, N.device)
    norm = Xp is not None
    c_g = Dout // 4 + 7 if norm else 0
    c_dp = c_g + 2
    parts = []
    for lo in range(0, max(n, 1), chunk):
        hi = min(lo + chunk, n)
        nn, x = _rows(N, lo, hi, keep), _rows(X, lo, hi, keep)
        P1, _, P2, _ = _pre(nn, x, W1, W2)
        g = _rows(G, lo, hi, keep) if G is not None else torch.zeros_like(P1)
        gm = g.abs()
        if norm:
            nz = keep & _keep(dz_flags, n, N.device)
            xp, dz, iv = _rows(Xp, lo, hi, nz), _rows(dZ, lo, hi, nz), _rows(inv, lo, hi, nz)[:, None]
            z = xp * iv
            dot, dmag = (z * dz).sum(1, keepdim=True), (z * dz).abs().sum(1, keepdim=True)
            clamped = iv >= INV_CLAMPED
            dot, dmag = torch.where(clamped, 0 * dot, dot), torch.where(clamped, 0 * dmag, dmag)
            g = g + iv * (dz - z * dot)
            gm = gm + iv.abs() * (dz.abs() + z.abs() * dmag)
        s1 = torch.where(P1 > 0, torch.ones_like(P1), torch.full_like(P1, slope))
        s2 = torch.where(P2 > 0, torch.ones_like(P2), torch.full_like(P2, slope))
        dP1, dP2, m1, m2 = g * s1, g * s2, gm * s1, gm * s2
        e1, e2 = c_dp * U32 * m1, c_dp * U32 * m2
        Wa1, Wa2 = W1.abs().t(), W2.abs().t()
        dA1, dA2 = dP1 @ W1.t(), dP2 @ W2.t()
        A1m, A2m, A1x, A2x = m1 @ Wa1, m2 @ Wa2, e1 @ Wa1, e2 @ Wa2
        parts.append({"dP1": (dP1, m1, c_dp, 0 * dP1), "dP2": (dP2, m2, c_dp, 0 * dP2),
                      "dN": (dA1 + dA2 * x, A1m + A2m * x.abs(), Dout + 2, A1x + A2x * x.abs()),
                      "dXd": (dA1 + dA2 * nn, A1m + A2m * nn.abs(), Dout + 2, A1x + A2x * nn.abs())})
    return _cat(parts)


def wgrad_split(n):
    """(per, waves) of launch_wgrad (ngcf.hip): MFMA steps of 4 rows per wave, and the waves the fold walks (whole blocks of 4)"""
    steps = _cdiv(n, 4)
    per = max(8, _cdiv(steps, WGRAD_WAVES))
    waves = _cdiv(steps, per) if steps > 0 else 1
    return per, _cdiv(waves, 4) * 4


def ngcf_wgrad(N, X, dP1, dP2, row_mask=None, chunk=CHUNK):
    """-> dict of Outs dW1p, dW2p [Din, Dout]; rows outside row_mask count as zero"""
    n, Din = N.shape
    Dout = dP1.shape[1]
    keep = _keep(row_mask, n, N.device)
    per, waves = wgrad_split(n)
    c = 4 * per + _cdiv(waves, 16) + 16 + 1
    z = lambda: torch.zeros(Din, Dout, dtype=torch.float64, device=N.device)
    d1, d2, m1, m2 = z(), z(), z(), z()
    for lo in range(0, n, chunk):
        hi = min(lo + chunk, n)
        nn, x = _rows(N, lo, hi, keep), _rows(X, lo, hi, keep)
        p1, p2 = _rows(dP1, lo, hi, keep), _rows(dP2, lo, hi, keep)
        a1, a2 = nn + x, nn * x
        d1 += a1.t() @ p1; m1 += a1.abs().t() @ p1.abs()
        d2 += a2.t() @ p2; m2 += a2.abs().t() @ p2.abs()
    return {"dW1p": Out(d1, m1, c, 0 * d1), "dW2p": Out(d2, m2, c, 0 * d2)}


# ========================================================================================================= tall products
def _small(W1, W2, w_split):
    """the small matrix [K, NO] in fp64 from its one or two logical views (the strides are the views')"""
    if w_split == 0:
        return _d(W1)
    return torch.cat([_d(W1), _d(W2)], dim=0 if w_split == 1 else 1)


def tall_mm(X1, W1, X2=None, sel=None, n=None, W2=None, w_split=0, b1=None, b2=None, old=None, chunk=CHUNK):
    """-> Out Y [n, NO] = [X1 | X2][sel[:n]] W + [b1 | b2] (+ old).  W1 / W2: logical [k, c] views (a transposed or row-sliced
    store is the caller's view); w_split 1: W2 holds the rows k >= K / 2, 2: the columns c >= NO / 2; old [n, NO]: what the
    destination(s) held, None without `accumulate`"""
    W = _small(W1, W2, w_split)
    K, NO = W.shape
    if n is None:
        n = sel.shape[0] if sel is not None else X1.shape[0]
    b = torch.zeros(NO, dtype=torch.float64, device=W.device)
    if b1 is not None:
        b = torch.cat([_d(b1).reshape(-1)] + ([_d(b2).reshape(-1)] if b2 is not None else []))
    ref, mag = [], []
    for lo in range(0, n, chunk):
        hi = min(lo + chunk, n)
        idx = sel[lo:hi] if sel is not None else slice(lo, hi)
        x = _d(X1[idx]) if X2 is None else torch.cat([_d(X1[idx]), _d(X2[idx])], dim=1)
        y, m = x @ W + b, x.abs() @ W.abs() + b.abs()
        if old is not None:
            y, m = y + _d(old[lo:hi]), m + _d(old[lo:hi]).abs()
        ref.append(y); mag.append(m)
    ref, mag = torch.cat(ref), torch.cat(mag)
    return Out(ref, mag, K + 1, 0 * ref)


def adam_fp64(p, m, v, g, lr, b1, b2, eps, step):
    """torch.optim.Adam's update (_single_tensor_adam) in fp64 -> p, m, v, denom"""
    m = m + (1.0 - b1) * (g - m)
    v = b2 * v + (1.0 - b2) * g * g
    denom = v.sqrt() / math.sqrt(1.0 - b2 ** step) + eps
    return p - lr / (1.0 - b1 ** step) * m / denom, m, v, denom


def f32(x):
    """the double value of the float the ABI takes"""
    return float(torch.tensor(x, dtype=torch.float32))


def tall_mm_adam(X, W, G_in, p, m, v, lr, b1, b2, eps, step, chunk=CHUNK):
    """-> dict of Outs p, m, v [n, NO] after the step on g = G_in + X W, and g.  lr, b1, b2, eps: the floats handed to the kernel"""
    g = tall_mm(X, W, old=G_in, chunk=chunk)
    lr, b1, b2, eps = f32(lr), f32(b1), f32(b2), f32(eps)
    p0, m0, v0 = _d(p), _d(m), _d(v)
    pr, mr, vr, den = adam_fp64(p0, m0, v0, g.ref, lr, b1, b2, eps, step)
    e = bound(g)
    hi, lo = adam_fp64(p0, m0, v0, g.ref + e, lr, b1, b2, eps, step), adam_fp64(p0, m0, v0, g.ref - e, lr, b1, b2, eps, step)
    move = lambda i, r: torch.maximum((hi[i] - r).abs(), (lo[i] - r).abs())
    m_mag = m0.abs() + (1.0 - b1) * (g.ref.abs() + m0.abs())
    step_size = lr / (1.0 - b1 ** step)
    return {"p": Out(pr, pr.abs() + torch.clamp(step_size * m_mag / den, min=lr), 12, move(0, pr)),
            "m": Out(mr, m_mag, 3, move(1, mr)), "v": Out(vr, vr, 4, move(2, vr)), "g": g}


def tall_wgrad_split(n):
    """(spw, waves) of wgrad_waves (proj.hip)"""
    steps = _cdiv(n, 4)
    spw = max(16, _cdiv(steps, TALL_WAVES))
    return spw, _cdiv(_cdiv(steps, spw), 4) * 4


def tall_wgrad(X, dY1, dY2=None, old_W=None, old_b=None, chunk=CHUNK):
    """-> dict of Outs dW [KI, NO], db [NO] over [dY1 | dY2]; old_W / old_b: what the destinations held (acc_w / acc_b)"""
    n, KI = X.shape
    NO = dY1.shape[1] * (2 if dY2 is not None else 1)
    spw, waves = tall_wgrad_split(n)
    c = 4 * spw + _cdiv(waves, 16) + 16
    z = lambda *s: torch.zeros(*s, dtype=torch.float64, device=X.device)
    dW, Wm, db, bm = z(KI, NO), z(KI, NO), z(NO), z(NO)
    for lo in range(0, n, chunk):
        hi = min(lo + chunk, n)
        x = _d(X[lo:hi])
        y = _d(dY1[lo:hi]) if dY2 is None else torch.cat([_d(dY1[lo:hi]), _d(dY2[lo:hi])], dim=1)
        dW += x.t() @ y; Wm += x.abs().t() @ y.abs()
        db += y.sum(0); bm += y.abs().sum(0)
    cw = cb = c
    if old_W is not None:
        dW, Wm, cw = dW + _d(old_W), Wm + _d(old_W).abs(), c + 1
    if old_b is not None:
        db, bm, cb = db + _d(old_b).reshape(-1), bm + _d(old_b).reshape(-1).abs(), c + 1
    return {"dW": Out(dW, Wm, cw, 0 * dW), "db": Out(db, bm, cb, 0 * db)}


def small_mm(A, B, old=None):
    """-> Out C = A B (+ old), A [M, K] and B [K, N] logical views"""
    a, b = _d(A), _d(B)
    ref, mag = a @ b, a.abs() @ b.abs()
    c = A.shape[1]
    if old is not None:
        ref, mag, c = ref + _d(old), mag + _d(old).abs(), c + 1
    return Out(ref, mag, c, 0 * ref)


def masked_colsum(dOut, out):
    """-> Out [D]: column sums of dOut [out > 0] (-0.0 and 0.0 are not > 0)"""
    n, D = dOut.shape
    g = _d(dOut) * (out > 0)
    rpp = 256 // (D // 4)
    blocks = min(_cdiv(n, rpp), COLSUM_BLOCKS)
    c = _cdiv(n, max(blocks, 1) * rpp) + rpp + _cdiv(blocks, 16) + 16
    return Out(g.sum(0), g.abs().sum(0), c, 0 * g.sum(0))


# ============================================================================================================== inputs
def make_case(n, Din, Dout, seed, device="cpu"):
    """Inputs of one NGCF case, float32 (+-0.1-scale tables, 0.3-scale weights): dict of N, X [n, Din], W1p, W2p [Din, Dout],
    G, dZ [n, Dout] and the backward's GIVEN Xp [n, Dout], inv [n].  Planted by row index mod 8 (spmm_ref.norm_rows):
      1  N and X all zero: forward Xp = 0, inv = 1e12, Z = 0; the given Xp row is zero too
      2  N = -X: P1 is exactly 0 with magnitude 0            4  N = 0: P2 is exactly 0
      3  the given Xp row has norm ~1e-13 (clamped, non-zero)
      5  an all-zero dZ row                                   6  a dZ row that is zero but for one -0.0
    The given Xp is the fp64 forward rounded to float (row 3 scaled down), the given inv the float of 1 / max(||Xp||, 1e-12)."""
    g = torch.Generator().manual_seed(seed)
    rn = lambda *s, sc: torch.randn(*s, generator=g) * sc
    c = {"N": rn(n, Din, sc=0.1), "X": rn(n, Din, sc=0.1), "W1p": rn(Din, Dout, sc=0.3), "W2p": rn(Din, Dout, sc=0.3),
         "G": rn(n, Dout, sc=1.0), "dZ": rn(n, Dout, sc=1.0)}
    r = torch.arange(n) % 8
    c["N"][r == 1] = 0
    c["X"][r == 1] = 0
    c["N"][r == 2] = -c["X"][r == 2]
    c["N"][r == 4] = 0
    xp = ngcf_fwd(c["N"], c["X"], c["W1p"], c["W2p"])["Xp"].ref.float()
    tiny = r == 3
    xp[tiny] = (xp[tiny].double() / xp[tiny].double().norm(dim=1, keepdim=True) * 1e-13).float()
    c["Xp"] = xp
    c["inv"] = (1.0 / xp.double().norm(dim=1).clamp_min(EPS)).float()
    c["dZ"][r == 5] = 0
    c["dZ"][r == 6] = 0
    c["dZ"][r == 6, Dout // 2] = -0.0
    c = {k: v.to(device) for k, v in c.items()}
    c.update(n=n, Din=Din, Dout=Dout, r=r.to(device))
    return c


def decided_case(n, Din, Dout, seed, device="cpu", tries=50):
    """make_case with the first seed of seed, seed + 1000, ... at which no row is undecided (the cases of fewer than 64 rows)"""
    for k in range(tries):
        c = make_case(n, Din, Dout, seed + 1000 * k, device=device)
        if not bool(undecided(c["N"], c["X"], c["W1p"], c["W2p"]).any()):
            return c
    raise AssertionError(f"no seed without an undecided row: n={n} Din={Din} Dout={Dout}")


def make_masks(n, seed, device="cpu"):
    """row_mask, dz_flags (uint8 [n], dz_flags a subset): a whole 16-row wave empty (16..31), a 4-row wgrad step empty (40..43), a
    whole 64-row tile empty (128..191, where n reaches past it), and of the last tile only the last row set"""
    g = torch.Generator().manual_seed(seed)
    mask = torch.rand(n, generator=g) < 0.5
    mask[16:32] = False
    mask[40:44] = False
    if n > 192:
        mask[128:192] = False
    mask[(n - 1) // 64 * 64:] = False
    mask[n - 1] = True
    flags = mask & (torch.rand(n, generator=g) < 0.5)
    flags[n - 1] = True
    return mask.to(torch.uint8).to(device), flags.to(torch.uint8).to(device)


# ================================================================================= the cases of the GPU files, in one place
LADDER = (1, 15, 16, 17, 63, 64, 65, 129, 257)
LOOP2_N, LOOP2_ONE_N = 65569, 16417            # past 1024 x 64 rows with per = 9; past 256 x 64 rows (the one-matrix backward)
LOOP2_SHAPES = [(16, 16), (64, 64)]
MASK_SHAPES, MASK_NS = [(64, 64), (32, 64), (128, 128)], (777, 65)
PLANT_SHAPES, PLANT_N = [(16, 16), (128, 64)], 203
REFUSAL_CASE = (40, 16, 16)


def gpu_case(n, Din, Dout, device="cpu"):
    """the inputs of case (n, Din, Dout) of test_gpu_ngcf_kernels.py; below 64 rows the seed is moved until none is undecided"""
    seed = 11 + 131 * Din + 17 * Dout + n
    return decided_case(n, Din, Dout, seed, device=device) if n < 64 else make_case(n, Din, Dout, seed, device=device)


def gpu_cases():
    """every (n, Din, Dout) the GPU file draws"""
    cases = {(n, a, b) for a, b in SHAPES for n in LADDER}
    cases |= {(LOOP2_N, a, b) for a, b in LOOP2_SHAPES} | {(LOOP2_ONE_N, 128, 128), (LOOP2_N, 128, 128)}
    cases |= {(n, a, b) for a, b in MASK_SHAPES for n in MASK_NS} | {(PLANT_N, a, b) for a, b in PLANT_SHAPES}
    return sorted(cases | {REFUSAL_CASE})


# ---- proj.hip
TALL_LADDER = (1, 15, 16, 17, 63, 64, 65)
TALL_FORMS = ("plain", "bias_acc", "transposed", "row_sliced", "x2", "y2_b2", "w_split1", "w_split2", "sel")
TALL_LOOP2_N = 81937                           # past 1280 blocks x 4 waves x 16 rows
ADAM_SHAPES, ADAM_NS = [(128, 32), (32, 128), (16, 16)], (1, 17, 65, 4099)
TWG_SHAPES, TWG_NS, TWG_SPW17_N = [(16, 16), (64, 32), (128, 128)], (1, 3, 5, 63, 65, 257), 4 * (16 * 2048 + 1)


def form_applies(form, K, NO):
    return not ((form == "x2" and K < 32) or (form == "y2_b2" and NO < 32))


def tall_case(form, n, K, NO, seed, device="cpu"):
    """One tall_mm call: dict of X1, X2, sel, n, W1, W2 (logical [k, c] views, one stride pair), w_split, b1, b2, old1, old2 (what
    the destinations hold when `accumulate`; None otherwise) and `split_out`.  0.1-scale tables, 0.3-scale weights.
      plain | bias_acc: bias and accumulate together | transposed: W stored [NO, K] | row_sliced: rows 5 .. 5 + K of a taller W
      x2: the k axis over two tables (K >= 32) | y2_b2: two outputs, two biases (NO >= 32)
      w_split1: W's rows k >= K / 2 in W2, stored transposed, accumulated (with X2 where K >= 32: dXs += [dP1 | dP2] [Wa^T; Wb^T])
      w_split2: W's columns c >= NO / 2 in W2, row slices of two taller matrices (with Y2 and b2 where NO >= 32)
      sel: gathered rows with repeated ids, the explicit n smaller than the list and the table"""
    g = torch.Generator().manual_seed(seed)
    rn = lambda *s, sc: (torch.randn(*s, generator=g) * sc).to(device)
    c = dict(form=form, n=n, K=K, NO=NO, X2=None, sel=None, W2=None, w_split=0, b1=None, b2=None, old1=None, old2=None, split_out=False)
    c["X1"] = rn(n, K, sc=0.1)
    c["W1"] = rn(K, NO, sc=0.3)
    if form == "bias_acc":
        c["b1"], c["old1"] = rn(NO, sc=0.3), rn(n, NO, sc=0.1)
    elif form == "transposed":
        c["W1"] = rn(NO, K, sc=0.3).t()
    elif form == "row_sliced":
        c["W1"] = rn(K + 10, NO, sc=0.3)[5:5 + K]
    elif form == "x2":
        c["X1"], c["X2"] = rn(n, K // 2, sc=0.1), rn(n, K // 2, sc=0.1)
    elif form == "y2_b2":
        c["split_out"], c["b1"], c["b2"] = True, rn(NO // 2, sc=0.3), rn(NO // 2, sc=0.3)
    elif form == "w_split1":
        c["w_split"], c["W1"], c["W2"] = 1, rn(NO, K // 2, sc=0.3).t(), rn(NO, K // 2, sc=0.3).t()
        c["old1"] = rn(n, NO, sc=0.1)
        if K >= 32:
            c["X1"], c["X2"] = rn(n, K // 2, sc=0.1), rn(n, K // 2, sc=0.1)
    elif form == "w_split2":
        c["w_split"], c["W1"], c["W2"] = 2, rn(K + 10, NO // 2, sc=0.3)[:K], rn(K + 10, NO // 2, sc=0.3)[:K]
        if NO >= 32:
            c["split_out"], c["b1"], c["b2"] = True, rn(NO // 2, sc=0.3), rn(NO // 2, sc=0.3)
    elif form == "sel":
        c["X1"] = rn(n + 7, K, sc=0.1)
        sel = torch.randint(0, n + 7, (n + 3,), generator=g)
        sel[n // 2] = sel[0]
        c["sel"] = sel.to(device)
    elif form == "sel_y2":                             # (the second-loop case: a gather from a table half as long, two outputs)
        c["X1"] = rn(n // 2 + 7, K, sc=0.1)
        c["sel"] = torch.randint(0, n // 2 + 7, (n,), generator=g).to(device)
        c["split_out"], c["b1"], c["b2"] = True, rn(NO // 2, sc=0.3), rn(NO // 2, sc=0.3)
    else:
        assert form == "plain", form
    return c


def tall_ref(c):
    """the restatement of a tall_case -> Out [n, NO]"""
    old = c["old1"] if c["old2"] is None else torch.cat([c["old1"], c["old2"]], dim=1)
    return tall_mm(c["X1"], c["W1"], X2=c["X2"], sel=c["sel"], n=c["n"], W2=c["W2"], w_split=c["w_split"], b1=c["b1"], b2=c["b2"], old=old)
