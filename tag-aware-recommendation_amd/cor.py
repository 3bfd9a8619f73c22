"""Host side of the distance-correlation kernels of csrc/cor.hip: the penalty between the factor slices of an embedding
sample (/root/reference/model/help/loss.py:53-80), the term that makes DGCF / DisenGCN / DisenHAN disentangled.

One function per C entry point, on tensors, and the `autograd.Function` over them.  X is [n, D] fp32 with unit column
stride; its row stride is passed as it is, so a column window of a wider tensor needs no copy.  Nothing is read back to the
host: the loss, the saved sums and the backward coefficients stay on the device, and the upstream gradient enters the
backward kernel as a device scalar.
"""
import torch

from ._lib import TagrecError, check, load, stream_ptr
from .rowops import VEC_WIDTHS


def _check(x, K, what):
    if not isinstance(x, torch.Tensor) or not x.is_cuda or x.dtype != torch.float32 or x.dim() != 2:
        raise TagrecError(f"{what}: expected a 2-d fp32 GPU tensor (tagrec_amd has no CPU path)")
    n, D = x.shape
    if x.stride(1) != 1 or x.stride(0) < D:
        raise TagrecError(f"{what}: rows must be contiguous (unit column stride)")
    if D not in VEC_WIDTHS or K < 2 or D % K or D // K < 2:
        raise TagrecError(f"{what}: need D in {VEC_WIDTHS}, 2 <= factor_k, factor_k | D and D / factor_k >= 2; got D={D}, factor_k={K}")
    if n < 2:
        raise TagrecError(f"{what}: need at least two rows, got {n}")


def cor_fwd(x, K):
    """-> (loss 0-d, saved = (rowsum [n, K] f64, gsum [K] f64, coef [K, 3]) for `cor_bwd`).  Workspace is O(n K)."""
    _check(x, K, "cor_fwd")
    n, D = x.shape
    dev = x.device
    rowsum = torch.empty(n, K, dtype=torch.float64, device=dev)
    gsum = torch.empty(K, dtype=torch.float64, device=dev)
    part = torch.empty(n, 2 * K, dtype=torch.float64, device=dev)
    sums = torch.empty(2 * K, dtype=torch.float64, device=dev)
    loss = torch.empty((), dtype=torch.float32, device=dev)
    coef = torch.empty(K, 3, dtype=torch.float32, device=dev)
    check(load().tagrec_cor_fwd_f32(x, x.stride(0), n, D, K, rowsum, gsum, part, sums, loss, coef, stream_ptr()), "cor_fwd")
    return loss, (rowsum, gsum, coef)


def cor_bwd(x, K, saved, g, dx=None):
    """dx [n, D] = g * d loss / dx; g is a device scalar.  Every row is written once."""
    _check(x, K, "cor_bwd")
    n, D = x.shape
    rowsum, gsum, coef = saved
    if dx is None:
        dx = torch.empty(n, D, dtype=torch.float32, device=x.device)
    check(load().tagrec_cor_bwd_f32(x, x.stride(0), n, D, K, rowsum, gsum, coef, g, dx, dx.stride(0), stream_ptr()), "cor_bwd")
    return dx


class _CorLoss(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, K):
        x = x.detach()
        if x.dim() == 2 and x.stride(1) == 1 and (x.stride(0) % 4 or x.data_ptr() % 16):
            x = x.contiguous()                       # the kernels load rows as 16-byte vectors
        loss, saved = cor_fwd(x, K)
        ctx.K = K
        ctx.save_for_backward(x, *saved)
        return loss

    @staticmethod
    def backward(ctx, g):
        x, rowsum, gsum, coef = ctx.saved_tensors
        g = g.to(torch.float32).contiguous()
        return cor_bwd(x, ctx.K, (rowsum, gsum, coef), g), None


def _as_one_tensor(parts):
    """The [n, K dk] tensor whose column slices `parts` are, without a copy when they are side-by-side views of one
    row-major tensor (what torch.split / torch.chunk along dim 1 return); otherwise their concatenation."""
    first = parts[0]
    base = first._base if first._base is not None else None
    n, dk = first.shape
    if base is not None and base.dim() == 2 and base.stride(1) == 1 and base.stride(0) >= 1:
        ok = all(p._base is base and tuple(p.shape) == (n, dk) and p.stride() == (base.stride(0), 1)
                 and p.storage_offset() == first.storage_offset() + k * dk for k, p in enumerate(parts))
        off = first.storage_offset() - base.storage_offset()
        r0, c0 = divmod(off, base.stride(0))
        if ok and off >= 0 and r0 + n <= base.shape[0] and c0 + len(parts) * dk <= base.shape[1]:
            return base[r0:r0 + n, c0:c0 + len(parts) * dk]
    return torch.cat(list(parts), dim=1)


def cor_loss(factor_emb, factor_k):
    """The reference's `cor_loss(factor_emb, factor_k)`: factor_emb is a sequence of factor_k [n, dk] tensors or one
    [n, factor_k dk] tensor -> 0-d loss (zero for factor_k = 1: there is no pair of slices)."""
    K = int(factor_k)
    if isinstance(factor_emb, torch.Tensor):
        x = factor_emb
    else:
        parts = list(factor_emb)[:K]
        if len(parts) != K:
            raise TagrecError(f"cor_loss: {len(parts)} factor slices for factor_k={K}")
        x = parts[0] if K == 1 else _as_one_tensor(parts)
    if not x.is_cuda:
        raise TagrecError("cor_loss: expected GPU tensors (tagrec_amd has no CPU path)")
    if K == 1:
        return x.sum() * 0.0
    return _CorLoss.apply(x, K)
