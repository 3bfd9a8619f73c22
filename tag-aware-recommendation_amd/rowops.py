"""Host side of the row kernels of csrc/rowops.hip: row normalise and its backward forms, row flags, the BPR loss.

One function per C entry point, on tensors.  Row strides (`ld`, `ldz`, `lddz`, `ldreg`) are the tensors' `stride(0)`, so a
slot view such as `out[:, off:]` is passed as it is; `D`, `n_rows` and `B` come from the shapes.  Every tensor argument
stays referenced until the launch has been enqueued.
"""
import torch

from . import _lib
from ._lib import check, load, ptr, stream_ptr

VEC_WIDTHS = (8, 16, 32, 64, 128, 256)      # row widths the vector (row-sparse / row-masked) kernels are built for


def rownorm_fwd(x, z=None, inv=None):
    """z = F.normalize(x) (z may be a strided slot view), inv[r] = 1 / max(||x[r]||, 1e-12) -> (z, inv)."""
    n, D = x.shape
    if z is None:
        z = torch.empty(n, D, dtype=torch.float32, device=x.device)
    if inv is None:
        inv = torch.empty(n, dtype=torch.float32, device=x.device)
    check(load().tagrec_rownorm_fwd_f32(ptr(x), ptr(z), z.stride(0), ptr(inv), n, D, stream_ptr()), "rownorm_fwd")
    return z, inv


def rownorm_bwd(x_raw, inv, dz, s, out, accumulate=False):
    """out (+)= normalize-backward(x_raw, inv, s * dz); dz may be a strided slot view."""
    n, D = x_raw.shape
    check(load().tagrec_rownorm_bwd_f32(ptr(x_raw), ptr(inv), ptr(dz), dz.stride(0), s, ptr(out), int(accumulate), n, D,
                                        stream_ptr()), "rownorm_bwd")
    return out


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
    check(load().tagrec_rownorm_bwd_flags_f32(ptr(x_raw), ptr(inv), ptr(dz), dz.stride(0), s, ptr(out), 0, n, D, ptr(flags),
                                              ptr(count), stream_ptr()), "rownorm_bwd_flags")
    return flags, count


def row_flags(x, flags=None, count=None):
    """flags[r] = row r of x holds a non-zero, count = number of such rows -> (flags, count)."""
    n, D = x.shape
    flags, count = _flags_count(n, x.device, flags, count)
    check(load().tagrec_row_flags_f32(ptr(x), n, D, ptr(flags), ptr(count), stream_ptr()), "row_flags")
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
    check(load().tagrec_bpr_fwd_f32(ptr(U), ptr(I), ld, D, ptr(Ureg), ptr(Ireg), ldreg, dreg, ptr(trip), B,
                                    loss_kind, ptr(coef), ptr(partials), ptr(res), stream_ptr()), "bpr_fwd")
    return res, coef


def bpr_bwd(U, I, Ureg, Ireg, trip, coef, g, dU, dI, dUreg, dIreg, what="bpr_bwd"):
    """Scatter-adds the gradients of `bpr_fwd`'s two loss parts (g = their upstream gradients, two floats) into the
    caller-zeroed dU / dI and dUreg / dIreg.  dU = dI = None: the L2 part only; Ureg = Ireg = None: no L2 part; g = None: both
    upstream gradients are 1."""
    g = None if g is None else g.contiguous()
    ld, D = _pair_ld(what, ("U", "I"), U, I, (dU, dI))
    ldreg, dreg = _pair_ld(what, ("Ureg", "Ireg"), Ureg, Ireg, (dUreg, dIreg))
    check(load().tagrec_bpr_bwd_f32(ptr(U), ptr(I), ld, D, ptr(Ureg), ptr(Ireg), ldreg, dreg, ptr(trip),
                                    trip.shape[0], ptr(coef), ptr(g), 1.0, ptr(dU), ptr(dI), ptr(dUreg), ptr(dIreg),
                                    stream_ptr()), what)


def bpr_dots(U, I, Ureg, Ireg, trip):
    """dots[b] = (u.p, u.n, 0.5 (|u|^2 + |p|^2 + |n|^2)) over the local columns of a column-sharded table -> [B, 3]."""
    B = trip.shape[0]
    dots = torch.empty(B, 3, dtype=torch.float32, device=U.device)
    ld, D = _pair_ld("bpr_dots", ("U", "I"), U, I)
    ldreg, dreg = _pair_ld("bpr_dots", ("Ureg", "Ireg"), Ureg, Ireg)
    check(load().tagrec_bpr_dots_f32(ptr(U), ptr(I), ld, D, ptr(Ureg), ptr(Ireg), ldreg, dreg, ptr(trip), B,
                                     ptr(dots), stream_ptr()), "bpr_dots")
    return dots


def compact_triplets(B, device):
    """Triplets of a loss on already gathered rows [users | pos items | neg items]: items are rows b and B + b of I = rows[B:]."""
    ar = torch.arange(B, device=device)
    return torch.stack([ar, ar, ar + B], dim=1).contiguous()


def batch_rows(trip, n_user):
    """Node ids [3 B] of a triplet batch in the [user | item] table: users, then positive and negative items."""
    return torch.cat([trip[:, 0], n_user + trip[:, 1], n_user + trip[:, 2]])
