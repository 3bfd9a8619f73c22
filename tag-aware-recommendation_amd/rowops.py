"""Host side of the row kernels of csrc/rowops.hip: row normalise and its backward forms, row flags, the BPR loss.

One function per C entry point, on tensors.  Row strides (`ld`, `ldz`, `lddz`, `ldreg`) are the tensors' `stride(0)`, so a
slot view such as `out[:, off:]` is passed as it is; `D`, `n_rows` and `B` come from the shapes.  Every tensor argument
stays referenced until the launch has been enqueued.
"""
import torch

from . import _lib
from ._lib import check, load, stream_ptr

VEC_WIDTHS = (8, 16, 32, 64, 128, 256)      # row widths the vector (row-sparse / row-masked) kernels are built for


def rownorm_fwd(x, z=None, inv=None):
    """z = F.normalize(x) (z may be a strided slot view), inv[r] = 1 / max(||x[r]||, 1e-12) -> (z, inv)."""
    n, D = x.shape
    if z is None:
        z = torch.empty(n, D, dtype=torch.float32, device=x.device)
    if inv is None:
        inv = torch.empty(n, dtype=torch.float32, device=x.device)
    check(load().tagrec_rownorm_fwd_f32(x, z, z.stride(0), inv, n, D, stream_ptr()), "rownorm_fwd")
    return z, inv


def _node_ids(what, node_ids, T, device):
    if node_ids is not None and (node_ids.dtype != torch.int64 or node_ids.shape != (T,) or not node_ids.is_contiguous()
                                 or node_ids.device != device):
        raise _lib.TagrecError(f"{what}: node_ids must be a contiguous int64 tensor of shape [{T}] on {device}")


def noise_rownorm_fwd(y, node_ids, eps, seed, view, layer, z=None, inv=None):
    """The compact top layer of a SimGCL view: row t of y (the product at node node_ids[t]; None: node t) is perturbed IN
    PLACE, y + eps sign(y) n(node), and normalised in the same pass -> (z, inv).  n: `noise_dir`.  D in VEC_WIDTHS."""
    _lib.require_gpu_tensor(y, torch.float32, "noise_rownorm_fwd: y")
    T, D = y.shape
    _node_ids("noise_rownorm_fwd", node_ids, T, y.device)
    if z is None:
        z = torch.empty(T, D, dtype=torch.float32, device=y.device)
    if inv is None:
        inv = torch.empty(T, dtype=torch.float32, device=y.device)
    check(load().tagrec_noise_rownorm_fwd_f32(y, node_ids, T, float(eps), int(seed), int(view), int(layer), z,
                                              z.stride(0) if T > 1 else D, inv, D, stream_ptr()), "noise_rownorm_fwd")
    return z, inv


def noise_dir(node_ids, D, seed, view, layer, device=None):
    """n(r) [T, D] of the SimGCL perturbation for the nodes `node_ids` (int64 [T]; an int T: nodes 0 .. T - 1): the unit
    direction the layer kernels draw on the fly from (seed, view, layer, node id) -- for tests and microbenchmarks."""
    if isinstance(node_ids, int):
        T, ids = node_ids, None
        if device is None:
            raise _lib.TagrecError("noise_dir: a row count needs a device")
    else:
        T, ids, device = node_ids.numel(), node_ids, node_ids.device
        _node_ids("noise_dir", ids, T, device)
    out = torch.empty(T, D, dtype=torch.float32, device=device)
    check(load().tagrec_noise_dir_f32(out, ids, T, int(seed), int(view), int(layer), D, stream_ptr()), "noise_dir")
    return out


def rownorm_bwd(x_raw, inv, dz, s, out, accumulate=False):
    """out (+)= normalize-backward(x_raw, inv, s * dz); dz may be a strided slot view."""
    n, D = x_raw.shape
    check(load().tagrec_rownorm_bwd_f32(x_raw, inv, dz, dz.stride(0), s, out, int(accumulate), n, D, stream_ptr()), "rownorm_bwd")
    return out


def layer_mean_rows(x0, rows, raws, invs, z_top, s, want_ego=True):
    """The layer mean of a restricted step on its batch rows, in one launch -> (out_b, ego_b or None), both [T, D]:
    out_b = s x0[rows] + sum_l s raws[l][rows] invs[l][rows, None] + s z_top, ego_b = x0[rows] -- the bits of the torch
    sequence index_select / `* s` / addcmul_(value=s) per layer / add_(alpha=s).  rows int64 [T] (may repeat); D % 4 == 0."""
    T, D = z_top.shape
    for t, nm in [(x0, "x0"), (z_top, "z_top")] + [(y, "raws") for y in raws] + [(v, "invs") for v in invs]:
        _lib.require_gpu_tensor(t, torch.float32, "layer_mean_rows: " + nm)
    _lib.require_gpu_tensor(rows, torch.int64, "layer_mean_rows: rows")
    n = x0.shape[0]
    if (rows.shape != (T,) or x0.shape[1] != D or len(raws) != len(invs) or len(raws) > 8 or D % 4
            or any(y.shape != x0.shape for y in raws) or any(v.shape != (n,) for v in invs)):
        raise _lib.TagrecError("layer_mean_rows: x0 / raws [n, D], invs [n], z_top [T, D], rows [T], D % 4 == 0, <= 8 layers expected")
    out_b = torch.empty(T, D, dtype=torch.float32, device=x0.device)
    ego_b = torch.empty(T, D, dtype=torch.float32, device=x0.device) if want_ego else None
    ys = (_lib.c_void_p * max(len(raws), 1))(*[y.data_ptr() for y in raws])
    vs = (_lib.c_void_p * max(len(invs), 1))(*[v.data_ptr() for v in invs])
    check(load().tagrec_layer_mean_rows_f32(x0, rows, T, n, ys, vs, len(raws), z_top, float(s), out_b, ego_b, D, stream_ptr()),
          "layer_mean_rows")
    return out_b, ego_b


def _flags_count(n, device, flags, count):
    if flags is None:
        flags = torch.empty(n, dtype=torch.uint8, device=device)
    if count is None:
        count = torch.zeros(1, dtype=torch.int32, device=device)
    return flags, count


def rownorm_bwd_flags(x_raw, inv, dz, s, out, flags=None, count=None):
    """`rownorm_bwd` that also writes which rows of `out` hold a non-zero and how many -> (flags, count)."""
    n, D = x_raw.shape
    flags, count = _flags_count(n, out.device, flags, count)
    check(load().tagrec_rownorm_bwd_flags_f32(x_raw, inv, dz, dz.stride(0), s, out, 0, n, D, flags, count, stream_ptr()),
          "rownorm_bwd_flags")
    return flags, count


def row_flags(x, flags=None, count=None):
    """flags[r] = row r of x holds a non-zero, count = number of such rows -> (flags, count)."""
    n, D = x.shape
    flags, count = _flags_count(n, x.device, flags, count)
    check(load().tagrec_row_flags_f32(x, n, D, flags, count, stream_ptr()), "row_flags")
    return flags, count


def _pair_ld(what, names, A, B, grads=()):
    """Row stride and width that the kernels index BOTH tables of a pair (U / I, Ureg / Ireg) and their gradient buffers
    with; raises before any launch if they do not share them.  A one-row tensor fits any row stride."""
    if A is None and B is None:
        return 0, 0
    if A is None or B is None:
        raise _lib.TagrecError(f"{what}: {names[0]} / {names[1]} must both be given or both None")
    if A.dim() != 2 or B.dim() != 2 or B.shape[1] != A.shape[1]:
        raise _lib.TagrecError(f"{what}: {names[0]} {tuple(A.shape)} and {names[1]} {tuple(B.shape)} must be 2-d of one width")
    ld = None
    for nm, t in zip(names + tuple("d" + n for n in names), (A, B) + tuple(grads)):
        if t is None:
            continue
        if t.dim() != 2 or t.shape[1] != A.shape[1]:
            raise _lib.TagrecError(f"{what}: {nm} {tuple(t.shape)} must be 2-d of width {A.shape[1]}")
        if t.shape[1] > 1 and t.stride(1) != 1:
            raise _lib.TagrecError(f"{what}: {nm} must have unit inner stride, got {t.stride(1)}")
        if t.shape[0] > 1:
            if ld is not None and t.stride(0) != ld:
                raise _lib.TagrecError(f"{what}: {nm} has row stride {t.stride(0)}, but the kernel indexes {names[0]}, {names[1]} "
                                       f"and their gradient buffers with one row stride ({ld})")
            ld = t.stride(0)
    return (A.shape[1] if ld is None else ld), A.shape[1]


def bpr_fwd(U, I, Ureg, Ireg, trip, loss_kind):
    """-> (res = [mul_loss, l2reg_loss (unweighted)], coef [B] for `bpr_bwd`).  Ureg / Ireg None: no L2 term."""
    B = trip.shape[0]
    coef = torch.empty(B, dtype=torch.float32, device=U.device)
    partials = torch.empty(2 * ((B + 3) // 4), dtype=torch.float32, device=U.device)     # two floats per launched block
    res = torch.empty(2, dtype=torch.float32, device=U.device)
    ld, D = _pair_ld("bpr_fwd", ("U", "I"), U, I)
    ldreg, dreg = _pair_ld("bpr_fwd", ("Ureg", "Ireg"), Ureg, Ireg)
    check(load().tagrec_bpr_fwd_f32(U, I, ld, D, Ureg, Ireg, ldreg, dreg, trip, B, loss_kind, coef, partials, res, stream_ptr()),
          "bpr_fwd")
    return res, coef


def bpr_bwd(U, I, Ureg, Ireg, trip, coef, g, dU, dI, dUreg, dIreg, what="bpr_bwd"):
    """Scatter-adds the gradients of `bpr_fwd`'s two loss parts (g = their upstream gradients, two floats) into the
    caller-zeroed dU / dI and dUreg / dIreg.  dU = dI = None: the L2 part only; Ureg = Ireg = None: no L2 part; g = None: both
    upstream gradients are 1."""
    g = None if g is None else g.contiguous()
    ld, D = _pair_ld(what, ("U", "I"), U, I, (dU, dI))
    ldreg, dreg = _pair_ld(what, ("Ureg", "Ireg"), Ureg, Ireg, (dUreg, dIreg))
    check(load().tagrec_bpr_bwd_f32(U, I, ld, D, Ureg, Ireg, ldreg, dreg, trip, trip.shape[0], coef, g, 1.0, dU, dI, dUreg, dIreg,
                                    stream_ptr()), what)


def bpr_dots(U, I, Ureg, Ireg, trip):
    """dots[b] = (u.p, u.n, 0.5 (|u|^2 + |p|^2 + |n|^2)) over the local columns of a column-sharded table -> [B, 3]."""
    B = trip.shape[0]
    dots = torch.empty(B, 3, dtype=torch.float32, device=U.device)
    ld, D = _pair_ld("bpr_dots", ("U", "I"), U, I)
    ldreg, dreg = _pair_ld("bpr_dots", ("Ureg", "Ireg"), Ureg, Ireg)
    check(load().tagrec_bpr_dots_f32(U, I, ld, D, Ureg, Ireg, ldreg, dreg, trip, B, dots, stream_ptr()), "bpr_dots")
    return dots


def compact_triplets(B, device):
    """Triplets of a loss on already gathered rows [users | pos items | neg items]: items are rows b and B + b of I = rows[B:]."""
    ar = torch.arange(B, device=device)
    return torch.stack([ar, ar, ar + B], dim=1).contiguous()


def batch_rows(trip, n_user):
    """Node ids [3 B] of a triplet batch in the [user | item] table: users, then positive and negative items."""
    return torch.cat([trip[:, 0], n_user + trip[:, 1], n_user + trip[:, 2]])


# ---- multi-negative ranking losses on compact rows (sampled softmax, K-negative BPR) ----

def tuple_rows(tuples, n_user):
    """Node ids [(2 + K) B] of a tuple batch [B, 2 + K] = (user, positive, K negatives) in the [user | item] table, in the
    slot order of `rank_fwd`: the B users, then item j of tuple b at slot B + j B + b.  K = 1: `batch_rows`."""
    return torch.cat([tuples[:, 0], (n_user + tuples[:, 1:]).t().reshape(-1)])


def _rank_shape(what, Ub, Ib):
    """(B, K) of a compact operand pair Ub [B, D] / Ib [(1 + K) B, D]."""
    if Ub is None or Ib is None or Ub.dim() != 2 or Ib.dim() != 2:
        raise _lib.TagrecError(f"{what}: Ub and Ib must be 2-d tensors")
    B = Ub.shape[0]
    K = Ib.shape[0] // B - 1 if B >= 1 else 0
    if B < 1 or Ib.shape[0] != (1 + K) * B or not 1 <= K <= 63:
        raise _lib.TagrecError(f"{what}: Ub {tuple(Ub.shape)} / Ib {tuple(Ib.shape)} must be [B, D] / [(1 + K) B, D] with K in 1 .. 63")
    return B, K


def _rank_reg_rows(what, Ureg, Ireg, B, K):
    if Ureg is not None and Ireg is not None and (Ureg.shape[0] != B or Ireg.shape[0] != (1 + K) * B):
        raise _lib.TagrecError(f"{what}: Ureg {tuple(Ureg.shape)} / Ireg {tuple(Ireg.shape)} must have {B} / {(1 + K) * B} rows")


def rank_fwd(Ub, Ib, Ureg, Ireg, loss_kind, temperature=1.0):
    """Ranking loss of B tuples on gathered rows: Ub [B, D] users, Ib [(1 + K) B, D] items (item j of tuple b at row j B + b,
    j = 0 the positive); Ureg / Ireg: the L2 rows in the same slot order (None: no L2 term).
    -> (res = [mul_loss, l2reg_loss (unweighted)], coef [B, K + 1] for `rank_bwd`)."""
    B, K = _rank_shape("rank_fwd", Ub, Ib)
    ld, D = _pair_ld("rank_fwd", ("Ub", "Ib"), Ub, Ib)
    ldreg, dreg = _pair_ld("rank_fwd", ("Ureg", "Ireg"), Ureg, Ireg)
    _rank_reg_rows("rank_fwd", Ureg, Ireg, B, K)
    coef = torch.empty(B, K + 1, dtype=torch.float32, device=Ub.device)
    partials = torch.empty(2 * ((B + 3) // 4), dtype=torch.float32, device=Ub.device)     # two floats per launched block
    res = torch.empty(2, dtype=torch.float32, device=Ub.device)
    check(load().tagrec_rank_fwd_f32(Ub, Ib, ld, D, Ureg, Ireg, ldreg, dreg, B, K, loss_kind, float(temperature), coef, partials,
                                     res, stream_ptr()), "rank_fwd")
    return res, coef


def rank_bwd(Ub, Ib, Ureg, Ireg, coef, g, dUb, dIb, dUreg, dIreg, what="rank_bwd"):
    """STORES the gradients of `rank_fwd`'s two loss parts (g = their upstream gradients, two floats; None: both 1) into every
    row of dUb / dIb and dUreg / dIreg -- no atomics, the old contents are not read.  dUb = dIb = None: the L2 part only;
    Ureg = Ireg = None: no L2 part; dUreg is dUb and dIreg is dIb (with Ureg is Ub, Ireg is Ib): one buffer takes the sum."""
    B, K = _rank_shape(what, Ub, Ib)
    g = None if g is None else g.contiguous()
    ld, D = _pair_ld(what, ("Ub", "Ib"), Ub, Ib, (dUb, dIb))
    ldreg, dreg = _pair_ld(what, ("Ureg", "Ireg"), Ureg, Ireg, (dUreg, dIreg))
    _rank_reg_rows(what, Ureg, Ireg, B, K)
    if coef.shape != (B, K + 1) or not coef.is_contiguous():
        raise _lib.TagrecError(f"{what}: coef {tuple(coef.shape)} must be a contiguous [{B}, {K + 1}] tensor")
    for nm, t, n in (("dUb", dUb, B), ("dIb", dIb, (1 + K) * B), ("dUreg", dUreg, B), ("dIreg", dIreg, (1 + K) * B)):
        if t is not None and t.shape[0] != n:
            raise _lib.TagrecError(f"{what}: {nm} {tuple(t.shape)} must have {n} rows")
    check(load().tagrec_rank_bwd_f32(Ub, Ib, ld, D, Ureg, Ireg, ldreg, dreg, B, K, coef, g, dUb, dIb, dUreg, dIreg, stream_ptr()),
          what)


# ---- weighted pointwise binary cross-entropy on compact rows (UltraGCN) ----

WBCE_MAX_SLOTS = 4096    # S = 1 + K + M: the kernels loop over the slots, the bound keeps a tuple's work in one wave sane


def _wbce_shape(what, Ub, Ib, K, M):
    """(B, S) of a compact operand pair Ub [B, D] / Ib [S B, D], S = 1 + K + M."""
    if Ub is None or Ib is None or Ub.dim() != 2 or Ib.dim() != 2:
        raise _lib.TagrecError(f"{what}: Ub and Ib must be 2-d tensors")
    if isinstance(K, bool) or isinstance(M, bool) or not isinstance(K, int) or not isinstance(M, int) or K < 1 or M < 0 \
            or 1 + K + M > WBCE_MAX_SLOTS:
        raise _lib.TagrecError(f"{what}: K={K!r} / M={M!r} must be integers with K >= 1, M >= 0 and 1 + K + M <= {WBCE_MAX_SLOTS}")
    B, S = Ub.shape[0], 1 + K + M
    if B < 1 or Ib.shape[0] != S * B:
        raise _lib.TagrecError(f"{what}: Ub {tuple(Ub.shape)} / Ib {tuple(Ib.shape)} must be [B, D] / [(1 + K + M) B, D] "
                               f"with K={K}, M={M}")
    return B, S


def _wbce_reg_rows(what, Ureg, Ireg, B, S):
    if Ureg is not None and Ireg is not None and (Ureg.shape[0] != B or Ireg.shape[0] != S * B):
        raise _lib.TagrecError(f"{what}: Ureg {tuple(Ureg.shape)} / Ireg {tuple(Ireg.shape)} must have {B} / {S * B} rows")


def wbce_fwd(Ub, Ib, Ureg, Ireg, weight, K, M=0):
    """Weighted pointwise BCE of B tuples on gathered rows: Ub [B, D] users, Ib [S B, D] items, S = 1 + K + M (slot j of tuple
    b at row j B + b; j = 0 the positive, 1 .. K the negatives, K + 1 .. K + M the positive's neighbours); labels +1 / -1 /
    +1; weight [B, S] float32 >= 0.  mul_loss = (1 / B) sum w softplus(-t s); the L2 part reads Ureg and slots 0 .. K of Ireg
    (None: no L2 term).  -> (res = [mul_loss, l2reg_loss (unweighted)], coef [B, S] for `wbce_bwd`, 1 / B folded in)."""
    B, S = _wbce_shape("wbce_fwd", Ub, Ib, K, M)
    ld, D = _pair_ld("wbce_fwd", ("Ub", "Ib"), Ub, Ib)
    ldreg, dreg = _pair_ld("wbce_fwd", ("Ureg", "Ireg"), Ureg, Ireg)
    _wbce_reg_rows("wbce_fwd", Ureg, Ireg, B, S)
    if not isinstance(weight, torch.Tensor) or weight.shape != (B, S) or not weight.is_contiguous():
        raise _lib.TagrecError(f"wbce_fwd: weight must be a contiguous [{B}, {S}] tensor")
    coef = torch.empty(B, S, dtype=torch.float32, device=Ub.device)
    partials = torch.empty(2 * ((B + 3) // 4), dtype=torch.float32, device=Ub.device)     # two floats per launched block
    res = torch.empty(2, dtype=torch.float32, device=Ub.device)
    check(load().tagrec_wbce_fwd_f32(Ub, Ib, ld, D, Ureg, Ireg, ldreg, dreg, B, K, M, weight, coef, partials, res, stream_ptr()),
          "wbce_fwd")
    return res, coef


def wbce_bwd(Ub, Ib, Ureg, Ireg, coef, g, dUb, dIb, dUreg, dIreg, K, M=0, what="wbce_bwd"):
    """STORES the gradients of `wbce_fwd`'s two loss parts into every row of dUb / dIb and dUreg / dIreg (zeros in the L2 rows
    of the neighbour slots) -- no atomics, the old contents are not read.  The None forms and the one-buffer form are
    `rank_bwd`'s: dUb = dIb = None: the L2 part only; Ureg = Ireg = None: no L2 part; dUreg is dUb and dIreg is dIb (with Ureg
    is Ub, Ireg is Ib): one buffer takes the sum."""
    B, S = _wbce_shape(what, Ub, Ib, K, M)
    g = None if g is None else g.contiguous()
    ld, D = _pair_ld(what, ("Ub", "Ib"), Ub, Ib, (dUb, dIb))
    ldreg, dreg = _pair_ld(what, ("Ureg", "Ireg"), Ureg, Ireg, (dUreg, dIreg))
    _wbce_reg_rows(what, Ureg, Ireg, B, S)
    if coef.shape != (B, S) or not coef.is_contiguous():
        raise _lib.TagrecError(f"{what}: coef {tuple(coef.shape)} must be a contiguous [{B}, {S}] tensor")
    for nm, t, n in (("dUb", dUb, B), ("dIb", dIb, S * B), ("dUreg", dUreg, B), ("dIreg", dIreg, S * B)):
        if t is not None and t.shape[0] != n:
            raise _lib.TagrecError(f"{what}: {nm} {tuple(t.shape)} must have {n} rows")
    check(load().tagrec_wbce_bwd_f32(Ub, Ib, ld, D, Ureg, Ireg, ldreg, dreg, B, K, M, coef, g, dUb, dIb, dUreg, dIreg, stream_ptr()),
          what)


# ---- in-batch sampled softmax on compact rows: the fused B x B loss (csrc/inbatch.hip) ----

INBATCH_TILE = 64        # rows per block of the in-batch kernels: `partials` holds two floats per block


def _inbatch_args(what, Ub, Ib, Ureg, Ireg, uid, iid, col_bias):
    """B of the operand pair Ub [B, D] / Ib [B, D] after the shape checks the two kernels share."""
    if Ub is None or Ib is None or Ub.dim() != 2 or Ib.dim() != 2 or Ub.shape[0] != Ib.shape[0]:
        raise _lib.TagrecError(f"{what}: Ub and Ib must be 2-d tensors with one row count (row b of Ib is the positive of row b of Ub)")
    B = Ub.shape[0]
    if B < 1:
        raise _lib.TagrecError(f"{what}: an empty batch (B = 0) has no loss")
    if (uid is None) != (iid is None):
        raise _lib.TagrecError(f"{what}: uid / iid must both be given or both None")
    for nm, t, dt in (("uid", uid, torch.int64), ("iid", iid, torch.int64), ("col_bias", col_bias, torch.float32)):
        if t is not None and (t.dtype != dt or t.shape != (B,) or not t.is_contiguous() or t.device != Ub.device):
            raise _lib.TagrecError(f"{what}: {nm} must be a contiguous {dt} tensor of shape [{B}] on {Ub.device}")
    if Ureg is not None and Ireg is not None and (Ureg.shape[0] != B or Ireg.shape[0] != B):
        raise _lib.TagrecError(f"{what}: Ureg {tuple(Ureg.shape)} / Ireg {tuple(Ireg.shape)} must have {B} rows")
    return B


def inbatch_fwd(Ub, Ib, Ureg, Ireg, temperature, uid=None, iid=None, col_bias=None):
    """In-batch softmax loss of B (row, positive) pairs on gathered rows: every other row of Ib is a negative of row b of Ub,
    except those whose iid equals iid[b] or whose uid equals uid[b] (masked).  Ureg / Ireg: the L2 rows (None: no L2 term).
    -> (res = [mul_loss, l2reg_loss (unweighted)], lse [B] for `inbatch_bwd`).  The B x B scores are never stored."""
    B = _inbatch_args("inbatch_fwd", Ub, Ib, Ureg, Ireg, uid, iid, col_bias)
    ld, D = _pair_ld("inbatch_fwd", ("Ub", "Ib"), Ub, Ib)
    ldreg, dreg = _pair_ld("inbatch_fwd", ("Ureg", "Ireg"), Ureg, Ireg)
    lse = torch.empty(B, dtype=torch.float32, device=Ub.device)
    partials = torch.empty(2 * max(1, (B + INBATCH_TILE - 1) // INBATCH_TILE), dtype=torch.float32, device=Ub.device)
    res = torch.empty(2, dtype=torch.float32, device=Ub.device)
    check(load().tagrec_inbatch_fwd_f32(Ub, Ib, ld, D, uid, iid, col_bias, Ureg, Ireg, ldreg, dreg, B, float(temperature), lse,
                                        partials, res, stream_ptr()), "inbatch_fwd")
    return res, lse


def inbatch_bwd(Ub, Ib, Ureg, Ireg, temperature, lse, g, dUb, dIb, dUreg, dIreg, uid=None, iid=None, col_bias=None,
                what="inbatch_bwd"):
    """STORES the gradients of `inbatch_fwd`'s two loss parts (g = their upstream gradients, two floats; None: both 1) into
    every row of dUb / dIb and dUreg / dIreg -- no atomics, the old contents are not read.  dUreg = dIreg = None: the L2
    gradient is not written; dUreg is dUb and dIreg is dIb (with Ureg is Ub, Ireg is Ib): one buffer takes the sum."""
    B = _inbatch_args(what, Ub, Ib, Ureg, Ireg, uid, iid, col_bias)
    g = None if g is None else g.contiguous()
    ld, D = _pair_ld(what, ("Ub", "Ib"), Ub, Ib, (dUb, dIb))
    ldreg, dreg = _pair_ld(what, ("Ureg", "Ireg"), Ureg, Ireg, (dUreg, dIreg))
    if lse.shape != (B,) or not lse.is_contiguous() or lse.dtype != torch.float32:
        raise _lib.TagrecError(f"{what}: lse {tuple(lse.shape)} must be a contiguous float32 [{B}] tensor")
    for nm, t in (("dUb", dUb), ("dIb", dIb), ("dUreg", dUreg), ("dIreg", dIreg)):
        if t is not None and t.shape[0] != B:
            raise _lib.TagrecError(f"{what}: {nm} {tuple(t.shape)} must have {B} rows")
    check(load().tagrec_inbatch_bwd_f32(Ub, Ib, ld, D, uid, iid, col_bias, Ureg, Ireg, ldreg, dreg, B, float(temperature), lse, g,
                                        dUb, dIb, dUreg, dIreg, stream_ptr()), what)


# ---- catalogue softmax: the fused rectangular B x N softmax cross-entropy (csrc/catsoftmax.hip) ----

def catsoftmax_splits(B, N, D):
    """The library's default number of column ranges for a [B, N] problem of width D (a pure function, >= 1)."""
    n = load().tagrec_catsoftmax_splits(B, N, D)
    if n < 1:
        check(n, "catsoftmax_splits")
    return n


def catsoftmax_workspace(B, N, D, n_split=0):
    """Bytes of the workspace of `catsoftmax_fwd` / `catsoftmax_bwd` (n_split = 0: the default split)."""
    nbytes = load().tagrec_catsoftmax_workspace(B, N, D, n_split)
    if nbytes <= 0:
        check(-1, "catsoftmax_workspace")
    return nbytes


def _row_ld(t):
    return t.stride(0) if t.shape[0] > 1 else t.shape[1]


def _catsoftmax_args(what, Q, T, target, qrow, Qreg, Treg, n_split, workspace):
    """(B, N, D, ldreg, Dreg, workspace) of a catalogue-softmax call after the checks the two kernels share.  The VALUES of
    target (in [0, N)) and qrow (rows of Q / Qreg) are not checked: that would take a host read."""
    for nm, t in (("Q", Q), ("T", T), ("Qreg", Qreg), ("Treg", Treg)):
        if t is None and nm in ("Qreg", "Treg"):
            continue
        if not isinstance(t, torch.Tensor) or not t.is_cuda or t.dtype != torch.float32 or t.dim() != 2:
            raise _lib.TagrecError(f"{what}: {nm} must be a 2-d float32 GPU tensor")
        if t.shape[1] > 1 and t.stride(1) != 1:
            raise _lib.TagrecError(f"{what}: {nm} must have unit inner stride, got {t.stride(1)}")
    if Q.shape[1] != T.shape[1]:
        raise _lib.TagrecError(f"{what}: Q {tuple(Q.shape)} and T {tuple(T.shape)} must be of one width")
    if not isinstance(target, torch.Tensor) or target.dtype != torch.int64 or target.dim() != 1 or not target.is_contiguous() \
            or target.device != Q.device:
        raise _lib.TagrecError(f"{what}: target must be a contiguous int64 tensor of shape [B] on {Q.device}")
    B, N, D = target.shape[0], T.shape[0], Q.shape[1]
    if B < 1:
        raise _lib.TagrecError(f"{what}: an empty batch (B = 0) has no loss")
    if N < 1:
        raise _lib.TagrecError(f"{what}: an empty column table (N = 0) has no softmax")
    if qrow is None:
        if Q.shape[0] != B:
            raise _lib.TagrecError(f"{what}: without qrow, Q {tuple(Q.shape)} must have one row per target ({B})")
    elif qrow.dtype != torch.int64 or qrow.shape != (B,) or not qrow.is_contiguous() or qrow.device != Q.device:
        raise _lib.TagrecError(f"{what}: qrow must be a contiguous int64 tensor of shape [{B}] on {Q.device}")
    if (Qreg is None) != (Treg is None):
        raise _lib.TagrecError(f"{what}: Qreg / Treg must both be given or both None")
    ldreg = dreg = 0
    if Qreg is not None:
        if Qreg.shape[1] != Treg.shape[1] or Qreg.shape[0] != Q.shape[0] or Treg.shape[0] != N:
            raise _lib.TagrecError(f"{what}: Qreg {tuple(Qreg.shape)} / Treg {tuple(Treg.shape)} must have the rows of Q "
                                   f"({Q.shape[0]}) / T ({N}) and one width")
        dreg = Qreg.shape[1]
        lds = {_row_ld(t) for t in (Qreg, Treg) if t.shape[0] > 1}
        if len(lds) > 1:
            raise _lib.TagrecError(f"{what}: Qreg and Treg are indexed with one row stride, got {sorted(lds)}")
        ldreg = lds.pop() if lds else dreg
    if isinstance(n_split, bool) or not isinstance(n_split, int) or not 0 <= n_split <= 65535:
        raise _lib.TagrecError(f"{what}: n_split must be an integer in 0 .. 65535 (0: the library's default), got {n_split!r}")
    need = catsoftmax_workspace(B, N, D, n_split)
    if workspace is None:
        workspace = torch.empty(need, dtype=torch.uint8, device=Q.device)
    elif workspace.dtype != torch.uint8 or workspace.numel() < need or workspace.device != Q.device or not workspace.is_contiguous():
        raise _lib.TagrecError(f"{what}: the workspace must be a contiguous uint8 tensor of >= {need} bytes on {Q.device}")
    return B, N, D, ldreg, dreg, workspace


_NO_COLS = {}        # device -> the one int32 that stands for the ids of an all-empty CSR (never read: every row is empty)


def _catsoftmax_mask(what, mask, Q, N):
    """The (ptr, cols) pair of the masked form after the checks that need no host read: ptr int64 [rows of Q + 1], cols int32,
    both contiguous and on Q's device.  Sortedness and the ids are NOT checked (that would take a host read): an unsorted list
    gives an unspecified mask, but the kernels read nothing outside [ptr[r], ptr[r + 1]) of cols."""
    if not isinstance(mask, (tuple, list)) or len(mask) != 2 or not all(isinstance(t, torch.Tensor) for t in mask):
        raise _lib.TagrecError(f"{what}: mask must be a pair of tensors (ptr, cols), got {type(mask).__name__}")
    ptr, cols = mask
    if ptr.dtype != torch.int64 or ptr.dim() != 1 or not ptr.is_contiguous() or ptr.device != Q.device \
            or ptr.numel() != Q.shape[0] + 1:
        raise _lib.TagrecError(f"{what}: mask ptr must be a contiguous int64 tensor of shape [{Q.shape[0] + 1}] (the rows of Q "
                               f"+ 1) on {Q.device}, got {ptr.dtype} {tuple(ptr.shape)} on {ptr.device}")
    if cols.dtype != torch.int32 or cols.dim() != 1 or not cols.is_contiguous() or cols.device != Q.device:
        raise _lib.TagrecError(f"{what}: mask cols must be a contiguous 1-d int32 tensor on {Q.device}, got {cols.dtype} "
                               f"{tuple(cols.shape)} on {cols.device}")
    if N > 2 ** 31 - 1:
        raise _lib.TagrecError(f"{what}: the masked form takes N <= 2^31 - 1 columns (int32 ids), got {N}")
    if cols.numel() == 0:                        # an empty tensor has no address: the library wants a pointer all the same
        cols = _NO_COLS.get(Q.device)
        if cols is None:                         # one per device, kept: nothing is allocated inside a later graph capture
            cols = _NO_COLS[Q.device] = torch.zeros(1, dtype=torch.int32, device=Q.device)
    return ptr, cols


def catsoftmax_fwd(Q, T, target, temperature, qrow=None, Qreg=None, Treg=None, n_split=0, workspace=None, mask=None):
    """Softmax cross-entropy of B rows against EVERY row of T: z_bn = Q[qrow[b]] . T[n] / temperature (qrow None: row b),
    loss_b = logsumexp_n z_bn - z_{b, target[b]}; Qreg / Treg (read at qrow / target; None: no L2 term) the L2 rows.
    -> (res = [mean_b loss_b, l2reg_loss (unweighted)], lse [B] for `catsoftmax_bwd`, zt [B] the target logits).
    The B x N logits are never stored.  n_split: column ranges the walk is cut into (0: `catsoftmax_splits`).  target must lie
    in [0, N) and qrow in the rows of Q: neither is checked (the kernels keep their reads inside the operands regardless).
    mask = (ptr int64 [rows of Q + 1], cols int32): a CSR over the rows of Q, ascending and unique within a row; row b leaves
    the columns of row qrow[b] (b without qrow) out of its softmax, all but target[b] itself (`_catsoftmax_mask` for what is
    checked).  None: the unmasked kernels, untouched."""
    what = "catsoftmax_fwd"
    B, N, D, ldreg, dreg, workspace = _catsoftmax_args(what, Q, T, target, qrow, Qreg, Treg, n_split, workspace)
    small = torch.empty(2 * B + 2, dtype=torch.float32, device=Q.device)         # lse | zt | res
    lse, zt, res = small[:B], small[B:2 * B], small[2 * B:]
    args = (Q, _row_ld(Q), qrow, T, _row_ld(T), N, D, target, Qreg, Treg, ldreg, dreg, B, float(temperature), n_split, workspace,
            workspace.numel(), lse, zt, res, stream_ptr())
    if mask is None:
        check(load().tagrec_catsoftmax_fwd_f32(*args), what)
    else:
        check(load().tagrec_catsoftmax_masked_fwd_f32(*args, *_catsoftmax_mask(what, mask, Q, N)), what)
    return res, lse, zt


def catsoftmax_bwd(Q, T, target, temperature, lse, g, dT, dQ=None, qrow=None, Qreg=None, Treg=None, dQreg=None, dTreg=None,
                   n_split=0, workspace=None, what="catsoftmax_bwd", mask=None):
    """STORES the gradients of `catsoftmax_fwd`'s two loss parts (g = their upstream gradients, two floats; None: both 1):
    every row of the dense dT [N, D] (may be a strided view) and of the compact dQ [B, D] (None: allocated) -- no atomics, the
    old contents are not read, the same bits for one (B, N, D, n_split).  dQreg / dTreg [B, Dreg] (both None: not written):
    the compact L2 gradients of the rows Qreg[qrow] / Treg[target]; dT = dQ = None: they alone.  Folding repeated qrow ids / targets is the caller's.
    mask: the forward's (`catsoftmax_fwd`); an excluded column's coefficient is exactly 0.
    -> dQ."""
    B, N, D, ldreg, dreg, workspace = _catsoftmax_args(what, Q, T, target, qrow, Qreg, Treg, n_split, workspace)
    g = None if g is None else g.contiguous()
    if lse.shape != (B,) or not lse.is_contiguous() or lse.dtype != torch.float32:
        raise _lib.TagrecError(f"{what}: lse {tuple(lse.shape)} must be a contiguous float32 [{B}] tensor")
    if dT is None:                           # the L2 part only
        if dQ is not None or dQreg is None:
            raise _lib.TagrecError(f"{what}: without dT, dQ must be None too and dQreg / dTreg are what is written")
    elif dQ is None:
        dQ = torch.empty(B, D, dtype=torch.float32, device=Q.device)
    if dT is None:
        pass
    elif dT.dim() != 2 or dT.shape != (N, D) or dT.dtype != torch.float32 or not dT.is_cuda or dT.stride(1) != 1:
        raise _lib.TagrecError(f"{what}: dT {tuple(dT.shape)} must be a float32 GPU tensor [{N}, {D}] with unit inner stride")
    if dQ is not None and (dQ.shape != (B, D) or dQ.dtype != torch.float32 or not dQ.is_contiguous()):
        raise _lib.TagrecError(f"{what}: dQ {tuple(dQ.shape)} must be a contiguous float32 [{B}, {D}] tensor")
    if (dQreg is None) != (dTreg is None) or (dQreg is not None and Qreg is None):
        raise _lib.TagrecError(f"{what}: dQreg / dTreg must both be given (with Qreg / Treg) or both None")
    for nm, t in (("dQreg", dQreg), ("dTreg", dTreg)):
        if t is not None and (t.shape != (B, dreg) or t.dtype != torch.float32 or not t.is_contiguous()):
            raise _lib.TagrecError(f"{what}: {nm} {tuple(t.shape)} must be a contiguous float32 [{B}, {dreg}] tensor")
    args = (Q, _row_ld(Q), qrow, T, _row_ld(T), N, D, target, Qreg, Treg, ldreg, dreg, B, float(temperature), n_split, workspace,
            workspace.numel(), lse, g, dT, 0 if dT is None else _row_ld(dT), dQ, dQreg, dTreg, stream_ptr())
    if mask is None:
        check(load().tagrec_catsoftmax_bwd_f32(*args), what)
    else:
        check(load().tagrec_catsoftmax_masked_bwd_f32(*args, *_catsoftmax_mask(what, mask, Q, N)), what)
    return dQ


# ---- nearest-centroid assignment: the fused n x K search of k-means (csrc/kmeans.hip) ----

def _kmeans_args(what, X, C, assign, best):
    """(n, K, D, assign, best) of an assignment call after the checks that need no host read."""
    for nm, t in (("X", X), ("C", C)):
        if not isinstance(t, torch.Tensor) or not t.is_cuda or t.dtype != torch.float32 or t.dim() != 2:
            raise _lib.TagrecError(f"{what}: {nm} must be a 2-d float32 GPU tensor")
        if t.shape[1] > 1 and t.stride(1) != 1:
            raise _lib.TagrecError(f"{what}: {nm} must have unit inner stride, got {t.stride(1)}")
    if X.shape[1] != C.shape[1] or X.device != C.device:
        raise _lib.TagrecError(f"{what}: X {tuple(X.shape)} and C {tuple(C.shape)} must be of one width and on one device")
    n, K, D = X.shape[0], C.shape[0], X.shape[1]
    if n < 1:
        raise _lib.TagrecError(f"{what}: no rows to assign (n = 0)")
    if K < 1:
        raise _lib.TagrecError(f"{what}: an empty centroid table (K = 0) has no nearest row")
    if D < 8 or D > 256 or D % 4 != 0:
        raise _lib.TagrecError(f"{what}: the width must be a multiple of 4 in 8 .. 256, got {D}")
    if assign is None:
        assign = torch.empty(n, dtype=torch.int64, device=X.device)
    elif not isinstance(assign, torch.Tensor) or assign.dtype != torch.int64 or assign.shape != (n,) or not assign.is_contiguous() \
            or assign.device != X.device:
        raise _lib.TagrecError(f"{what}: assign must be a contiguous int64 tensor of shape [{n}] on {X.device}")
    if best is None:
        best = torch.empty(n, dtype=torch.float32, device=X.device)
    elif not isinstance(best, torch.Tensor) or best.dtype != torch.float32 or best.shape != (n,) or not best.is_contiguous() \
            or best.device != X.device:
        raise _lib.TagrecError(f"{what}: best must be a contiguous float32 tensor of shape [{n}] on {X.device}")
    return n, K, D, assign, best


def kmeans_assign(X, C, assign=None, best=None, half_norm=None):
    """The nearest row of C [K, D] for every row of X [n, D] (both may be strided row views): s_ij = x_i . c_j - 0.5 |c_j|^2,
    assign[i] = argmax_j s_ij -- the Euclidean nearest centroid, ties to the LOWER id -- and best[i] = the winning score
    (the inertia is sum_i |x_i|^2 - 2 best_i).  -> (assign int64 [n], best float32 [n]); both are allocated when None.
    The n x K scores are never stored.  half_norm: float32 [K] scratch for the centroids' half norms (None: allocated)."""
    what = "kmeans_assign"
    n, K, D, assign, best = _kmeans_args(what, X, C, assign, best)
    if half_norm is None:
        half_norm = torch.empty(K, dtype=torch.float32, device=X.device)
    elif half_norm.dtype != torch.float32 or half_norm.numel() < K or not half_norm.is_contiguous() or half_norm.device != X.device:
        raise _lib.TagrecError(f"{what}: half_norm must be a contiguous float32 tensor of >= {K} elements on {X.device}")
    check(load().tagrec_kmeans_assign_f32(X, _row_ld(X), n, C, _row_ld(C), K, D, half_norm, assign, best, stream_ptr()), what)
    return assign, best


# ---- DirectAU on compact rows: alignment + uniformity on the unit sphere, fused B x B kernels (csrc/directau.hip) ----

AU_PREP_ROWS = 4         # batch positions per block of the prep kernel: `partials` holds two floats per block of it ...
AU_TILE = 64             # ... and one per side and block of the uniformity kernel


class AuState:
    """What `directau_fwd` keeps for `directau_bwd`: t, gamma, inv [2 B] (inverse row norms of Ub, then Ib), ls [2] = log S;
    parts = the forward's [align, unif_u, unif_i] (not read by the backward)."""
    __slots__ = ("t", "gamma", "inv", "ls", "parts")

    def __init__(self, t, gamma, inv, ls, parts):
        self.t, self.gamma, self.inv, self.ls, self.parts = t, gamma, inv, ls, parts


def _au_args(what, Ub, Ib, Ureg, Ireg):
    B = _inbatch_args(what, Ub, Ib, Ureg, Ireg, None, None, None)
    if B < 2:
        raise _lib.TagrecError(f"{what}: a batch of one pair (B = 1) has no other pair to be uniform against")
    return B


def directau_fwd(Ub, Ib, Ureg, Ireg, t, gamma):
    """DirectAU loss of B (user, positive) pairs on gathered rows: align + gamma (unif(Ub) + unif(Ib)) / 2 on the row-normalised
    operands (include/tagrec.h has the formulas); Ureg / Ireg: the L2 rows (None: no L2 term).
    -> (res = [mul_loss, l2reg_loss (unweighted)], parts = [align, unif_u, unif_i], state for `directau_bwd`).
    The B x B Gaussian potentials are never stored."""
    B = _au_args("directau_fwd", Ub, Ib, Ureg, Ireg)
    ld, D = _pair_ld("directau_fwd", ("Ub", "Ib"), Ub, Ib)
    ldreg, dreg = _pair_ld("directau_fwd", ("Ureg", "Ireg"), Ureg, Ireg)
    dev = Ub.device
    inv = torch.empty(2 * B, dtype=torch.float32, device=dev)
    small = torch.empty(7, dtype=torch.float32, device=dev)              # ls [2] | parts [3] | res [2]
    ls, parts, res = small[0:2], small[2:5], small[5:7]
    partials = torch.empty(2 * ((B + AU_PREP_ROWS - 1) // AU_PREP_ROWS) + 2 * ((B + AU_TILE - 1) // AU_TILE), dtype=torch.float32,
                           device=dev)
    check(load().tagrec_directau_fwd_f32(Ub, Ib, ld, D, Ureg, Ireg, ldreg, dreg, B, float(t), float(gamma), inv, ls, partials,
                                         parts, res, stream_ptr()), "directau_fwd")
    return res, parts, AuState(float(t), float(gamma), inv, ls, parts)


def directau_bwd(Ub, Ib, Ureg, Ireg, state, g, dUb, dIb, dUreg, dIreg, what="directau_bwd"):
    """STORES the gradients of `directau_fwd`'s two loss parts with respect to the RAW rows (g = their upstream gradients, two
    floats; None: both 1) into every row of dUb / dIb and dUreg / dIreg -- no atomics, the old contents are not read.
    dUreg = dIreg = None: the L2 gradient is not written; dUreg is dUb and dIreg is dIb (with Ureg is Ub, Ireg is Ib): one
    buffer takes the sum."""
    B = _au_args(what, Ub, Ib, Ureg, Ireg)
    g = None if g is None else g.contiguous()
    ld, D = _pair_ld(what, ("Ub", "Ib"), Ub, Ib, (dUb, dIb))
    ldreg, dreg = _pair_ld(what, ("Ureg", "Ireg"), Ureg, Ireg, (dUreg, dIreg))
    inv, ls = state.inv, state.ls
    if inv.shape != (2 * B,) or not inv.is_contiguous() or inv.dtype != torch.float32 or ls.shape != (2,) or ls.dtype != torch.float32:
        raise _lib.TagrecError(f"{what}: the state must hold a contiguous float32 inv [{2 * B}] and ls [2]")
    for nm, t in (("dUb", dUb), ("dIb", dIb), ("dUreg", dUreg), ("dIreg", dIreg)):
        if t is not None and t.shape[0] != B:
            raise _lib.TagrecError(f"{what}: {nm} {tuple(t.shape)} must have {B} rows")
    check(load().tagrec_directau_bwd_f32(Ub, Ib, ld, D, Ureg, Ireg, ldreg, dreg, B, state.t, state.gamma, inv, ls, g, dUb, dIb,
                                         dUreg, dIreg, stream_ptr()), what)


def fold_rows(dst, rows, src, plan=None, accumulate=True):
    """dst[rows[j]] (+)= src[j]: through `plan` (the `row_list_plan` of rows) in a fixed order, else by `index_add_` (float
    atomics where the list names a row twice).  Without `accumulate` the listed rows of dst are overwritten with their sums."""
    if plan is not None:
        return scatter_rows_ordered(dst, plan, src, accumulate)
    if not accumulate:
        dst.index_fill_(0, rows, 0.0)
    return dst.index_add_(0, rows, src)


# ---- fixed-order scatter of compact rows (csrc/rowscatter.hip): the `deterministic` mode of LightGCN / NGCF ----

class RowListPlan:
    """A row list (int64 node ids [T], may repeat) sorted into segments, one per distinct id, built on the device without a
    host read.  `order` (int32 [T]): the slots stably sorted by row id; `seg_row` / `seg_ptr` (int32 [T] / [T + 1]): the
    distinct rows ascending and where their slots start in `order`, valid up to the device-side segment count; `counts`
    (int32 [4]): segments, valid slots, ids outside [0, n).  All are views of `workspace`, which also holds the scatter's
    chunk sums: a plan serves one stream at a time and lives until its workspace is planned again."""
    __slots__ = ("rows", "n", "width", "workspace", "order", "seg_row", "seg_ptr", "counts")

    def segments(self):
        """(seg_row [S], seg_ptr [S + 1]) -- reads the segment count back to the host."""
        S = int(self.counts[0])
        return self.seg_row[:S], self.seg_ptr[:S + 1]

    def dropped(self):
        """Number of ids outside [0, n) that the plan left out -- reads the device counter back to the host."""
        return int(self.counts[2])


def row_list_workspace(n_listed, width):
    """Bytes of the workspace of a plan over n_listed rows whose scatters are at most `width` floats wide."""
    nbytes = load().tagrec_rowlist_workspace(n_listed, width)
    if nbytes <= 0:
        check(-1, "rowlist_workspace")
    return nbytes


def row_list_plan(rows, n, workspace=None, width=256):
    """-> RowListPlan of `rows` (int64 [T] ids into a table of n rows).  workspace: uint8 tensor of at least
    `row_list_workspace(T, width)` bytes (None: allocated here); width: the widest row the plan will scatter."""
    rows = _lib.require_gpu_tensor(rows, torch.int64, "row_list_plan: rows")
    T = rows.numel()
    need = row_list_workspace(T, width)
    if workspace is None:
        workspace = torch.empty(need, dtype=torch.uint8, device=rows.device)
    elif workspace.dtype != torch.uint8 or workspace.numel() < need or workspace.device != rows.device or not workspace.is_contiguous():
        raise _lib.TagrecError(f"row_list_plan: the workspace must be a contiguous uint8 tensor of >= {need} bytes on {rows.device}")
    lib = load()
    check(lib.tagrec_rowlist_plan_i64(rows, T, n, width, workspace, workspace.numel(), stream_ptr()), "rowlist_plan")
    p = RowListPlan()
    p.rows, p.n, p.width, p.workspace = rows, n, width, workspace
    at = [lib.tagrec_rowlist_plan_result(T, width, k) for k in range(4)]
    p.order = workspace[at[0]:at[0] + 4 * T].view(torch.int32)
    p.seg_row = workspace[at[1]:at[1] + 4 * T].view(torch.int32)
    p.seg_ptr = workspace[at[2]:at[2] + 4 * (T + 1)].view(torch.int32)
    p.counts = workspace[at[3]:at[3] + 16].view(torch.int32)
    return p


def scatter_rows_ordered(dst, plan, src, accumulate):
    """dst[r] (=|+=) sum of src[j] over plan.rows[j] == r, in ascending j (chunks of 1024: see include/tagrec.h); rows of dst
    the list does not name are not touched.  No float atomics: the same bits on every run.  src [T, D], dst [>= plan.n, D];
    both may have a row stride larger than D."""
    T = plan.rows.numel()
    if src.dim() != 2 or dst.dim() != 2 or src.shape[0] != T or src.shape[1] != dst.shape[1] or dst.shape[0] < plan.n:
        raise _lib.TagrecError(f"scatter_rows_ordered: src {tuple(src.shape)} must be [{T}, D] and dst {tuple(dst.shape)} "
                               f"[>= {plan.n}, D]")
    for nm, t in (("src", src), ("dst", dst)):
        if not t.is_cuda or t.dtype != torch.float32 or (t.shape[1] > 1 and t.stride(1) != 1):
            raise _lib.TagrecError(f"scatter_rows_ordered: {nm} must be a float32 GPU tensor with unit inner stride")
    D = src.shape[1]
    check(load().tagrec_row_scatter_ordered_f32(plan.workspace, plan.workspace.numel(), T, plan.width, src,
                                                src.stride(0) if T > 1 else D, dst, dst.stride(0) if dst.shape[0] > 1 else D,
                                                dst.shape[0], D, int(bool(accumulate)), stream_ptr()), "row_scatter_ordered")
    return dst


def bpr_bwd_ordered(out, ego, trip, coef, g, d_out, d_ego, plan, accumulate=False, what="bpr_bwd_ordered"):
    """`bpr_bwd` for triplets that index the real [user | item] tables, without float atomics on repeated rows: the 3 B operand
    rows are gathered, `bpr_bwd` runs on `compact_triplets` (every slot its own row: nothing collides) and the compact
    gradients are folded with `scatter_rows_ordered`.  out / ego: the tables of the main and the L2 part (ego None: no L2
    part); d_out / d_ego: where their gradients land (d_out None: the L2 part only; d_ego may be d_out); plan: the
    `row_list_plan` of `batch_rows(trip, n_user)`."""
    B = trip.shape[0]
    rows = plan.rows
    ctrip = compact_triplets(B, out.device)
    out_b = out.index_select(0, rows)
    d_b = None if d_out is None else torch.zeros_like(out_b)
    dU, dI = (None, None) if d_b is None else (d_b[:B], d_b[B:])
    Ue = Ie = dUe = dIe = d_e = None
    if ego is not None:
        ego_b = out_b if ego is out else ego.index_select(0, rows)
        d_e = d_b if (d_ego is d_out and d_b is not None) else torch.zeros_like(ego_b)
        Ue, Ie, dUe, dIe = ego_b[:B], ego_b[B:], d_e[:B], d_e[B:]
    bpr_bwd(out_b[:B], out_b[B:], Ue, Ie, ctrip, coef, g, dU, dI, dUe, dIe, what)
    if d_b is not None:
        scatter_rows_ordered(d_out, plan, d_b, accumulate)
    if d_e is not None and d_e is not d_b:
        scatter_rows_ordered(d_ego, plan, d_e, accumulate)


# ---- row-sparse Adam (csrc/rowadam.hip): the kernels behind train.RowAdam ----

ADAM_MAX_WINDOW = 4096   # steps one replay can span (the kernels stage that window of the ring in LDS)


def adam_coef(lr, b1, b2, t0, n):
    """The ring's pairs of steps t0 .. t0 + n - 1 as a CPU float32 tensor [n, 2] = (lr / (1 - b1^t), sqrt(1 - b2^t)): host
    arithmetic only (`tagrec_adam_coef`), no stream.  lr / b1 / b2 are taken as doubles; `tagrec_adam_f32` widens floats,
    so a caller that wants its bits passes the float-rounded values."""
    if t0 < 1 or n < 0:
        raise _lib.TagrecError(f"adam_coef: t0={t0} / n={n}: steps are counted from 1")
    buf = (_lib.ctypes.c_float * (2 * n))()
    check(load().tagrec_adam_coef(float(lr), float(b1), float(b2), int(t0), int(n), buf), "adam_coef")
    if n == 0:
        return torch.empty(0, 2, dtype=torch.float32)
    return torch.frombuffer(buf, dtype=torch.float32).view(n, 2)


def _row_adam_args(what, p, m, v, last, ring):
    """The table side of the three row-Adam kernels -> (row stride, n_rows, D, ring capacity)."""
    if not isinstance(p, torch.Tensor) or p.dim() != 2 or not p.is_cuda or p.dtype != torch.float32:
        raise _lib.TagrecError(f"{what}: p must be a 2-d float32 GPU tensor")
    n, D = p.shape
    ld = p.stride(0) if n > 1 else D
    for nm, t in (("p", p), ("m", m), ("v", v)):
        if not isinstance(t, torch.Tensor) or t.shape != p.shape or t.dtype != torch.float32 or t.device != p.device:
            raise _lib.TagrecError(f"{what}: {nm} must be a float32 tensor {tuple(p.shape)} on {p.device}")
        if (D > 1 and t.stride(1) != 1) or (n > 1 and t.stride(0) != ld) or ld < D:
            raise _lib.TagrecError(f"{what}: {nm} must have unit inner stride and the row stride of p ({ld})")
    if not isinstance(last, torch.Tensor) or last.shape != (n,) or last.dtype != torch.int32 or last.device != p.device \
            or not last.is_contiguous():
        raise _lib.TagrecError(f"{what}: last must be a contiguous int32 tensor [{n}] on {p.device}")
    if not isinstance(ring, torch.Tensor) or ring.dim() != 2 or ring.shape[1] != 2 or ring.shape[0] < 1 or ring.dtype != torch.float32 \
            or ring.device != p.device or not ring.is_contiguous():
        raise _lib.TagrecError(f"{what}: ring must be a contiguous float32 tensor [capacity, 2] on {p.device}")
    return ld, n, D, ring.shape[0]


def _row_adam_window(what, cap, t_floor, t_done):
    if not 0 <= t_floor <= t_done or t_done - t_floor > min(cap, ADAM_MAX_WINDOW):
        raise _lib.TagrecError(f"{what}: t_floor={t_floor} / t_done={t_done}: needs 0 <= t_floor <= t_done and at most "
                               f"min(the ring's {cap}, {ADAM_MAX_WINDOW}) steps between them")


def _row_adam_plan(what, plan, n, D, p):
    if not isinstance(plan, RowListPlan) or plan.n > n or plan.width < D or plan.workspace.device != p.device:
        raise _lib.TagrecError(f"{what}: plan must be a row_list_plan over at most {n} rows, of width >= {D}, on {p.device}")


def adam_catch_up(plan, p, m, v, last, ring, t_floor, t_done, betas=(0.9, 0.999), eps=1e-8):
    """Every distinct row r of `plan` takes Adam's zero-gradient update of steps last[r] + 1 .. t_done, in order (what dense
    Adam did to it while it was left alone); last[r] = t_done.  Rows the plan does not name are not touched.  p / m / v
    [n, D] (a shared row stride), last int32 [n], ring float32 [capacity, 2] (`adam_coef`'s pair of step t at t mod
    capacity), t_floor: a lower bound of `last` over the listed rows (rowops.ADAM_MAX_WINDOW bounds t_done - t_floor)."""
    what = "adam_catch_up"
    ld, n, D, cap = _row_adam_args(what, p, m, v, last, ring)
    _row_adam_plan(what, plan, n, D, p)
    _row_adam_window(what, cap, t_floor, t_done)
    check(load().tagrec_rowadam_catchup_f32(plan.workspace, plan.workspace.numel(), plan.rows.numel(), plan.width, p, m, v, ld, n, D,
                                            last, ring, cap, int(t_floor), int(t_done), float(betas[0]), float(betas[1]), float(eps),
                                            stream_ptr()), what)


def adam_apply_rows(plan, src, p, m, v, last, ring, t, betas=(0.9, 0.999), eps=1e-8):
    """One Adam step, number t, of the distinct rows of `plan`: a row's gradient is the sum of src[j] over plan.rows[j] == r
    in `scatter_rows_ordered`'s order (the same device code); last[r] = t.  src [T, D] (a row stride allowed).  The rows
    must be at step t - 1 (`adam_catch_up`); that is not checked.  Rows the plan does not name are not touched."""
    what = "adam_apply_rows"
    ld, n, D, cap = _row_adam_args(what, p, m, v, last, ring)
    _row_adam_plan(what, plan, n, D, p)
    T = plan.rows.numel()
    if not isinstance(src, torch.Tensor) or src.shape != (T, D) or src.dtype != torch.float32 or src.device != p.device \
            or (D > 1 and src.stride(1) != 1):
        raise _lib.TagrecError(f"{what}: src must be a float32 tensor [{T}, {D}] with unit inner stride on {p.device}")
    if t < 1:
        raise _lib.TagrecError(f"{what}: t={t}: steps are counted from 1")
    check(load().tagrec_rowadam_apply_f32(plan.workspace, plan.workspace.numel(), T, plan.width, src, src.stride(0) if T > 1 else D,
                                          p, m, v, ld, n, D, last, ring, cap, int(t), float(betas[0]), float(betas[1]), float(eps),
                                          stream_ptr()), what)


def adam_flush(p, m, v, last, ring, t_floor, t_done, betas=(0.9, 0.999), eps=1e-8):
    """Every row of the table with last[r] < t_done is replayed to t_done (`adam_catch_up` without a plan); a row that is
    current costs the read of its `last`.  t_floor: a lower bound of `last` over the whole table."""
    what = "adam_flush"
    ld, n, D, cap = _row_adam_args(what, p, m, v, last, ring)
    _row_adam_window(what, cap, t_floor, t_done)
    check(load().tagrec_rowadam_flush_f32(p, m, v, ld, n, D, last, ring, cap, int(t_floor), int(t_done), float(betas[0]),
                                          float(betas[1]), float(eps), stream_ptr()), what)
