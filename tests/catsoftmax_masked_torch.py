"""fp64 restatement of the MASKED catalogue softmax loss (rowops.catsoftmax_fwd / catsoftmax_bwd with mask=, and
help.catalogue_softmax_loss with positives=) in plain torch: logits from a matmul, the excluded entries set by
masked_fill(-inf), F.cross_entropy(reduction="mean") and autograd -- what the tests compare against.  It is deliberately not
the form the kernels evaluate (no cursor, no running pair, no select on a coefficient): the CSR becomes a dense boolean matrix.
Nothing is read from the library.

Operands as in tests/catsoftmax_torch.py, plus the CSR (ptr int64 [rows of Q + 1], cols int32) over the rows of Q:
    E_b  = cols[ptr[qrow_b] : ptr[qrow_b + 1]] \\ {target_b}
    loss = mean_b [ -log softmax_{n not in E_b}(z_b)[target_b] ]
"""
import torch
import torch.nn.functional as F

from catsoftmax_torch import logits64


def dense_mask(ptr, cols, target, N, qrow=None):
    """bool [B, N]: True where column n is excluded for batch row b (the row's own target never is)."""
    ptr, cols = ptr.cpu().tolist(), cols.cpu().long()
    B = target.shape[0]
    ex = torch.zeros(B, N, dtype=torch.bool)
    for b in range(B):
        r = b if qrow is None else int(qrow[b])
        ex[b, cols[ptr[r]:ptr[r + 1]]] = True
    ex[torch.arange(B), target.cpu()] = False
    return ex


def masked_catalogue_loss64(Q, T, target, Qreg, Treg, ptr, cols, tau=1.0, qrow=None):
    """(mul_loss, l2reg_loss) in fp64; differentiable w.r.t. whatever requires grad."""
    ex = dense_mask(ptr, cols, target, T.shape[0], qrow)
    z = logits64(Q, T, tau, qrow).masked_fill(ex, float("-inf"))
    loss = F.cross_entropy(z, target, reduction="mean")
    if Qreg is None:
        return loss, torch.zeros((), dtype=torch.float64)
    B = target.shape[0]
    qr = Qreg.double() if qrow is None else Qreg.double()[qrow]
    return loss, 0.5 * (qr.pow(2).sum() + Treg.double()[target].pow(2).sum()) / B


def masked_catalogue_tables64(U, I, Ureg, Ireg, pairs, ptr, cols, tau=1.0):
    """The same on user / item tables and a [B, 2] (user, positive) batch; the CSR runs over the users."""
    return masked_catalogue_loss64(U, I, pairs[:, 1], Ureg, Ireg, ptr, cols, tau, pairs[:, 0])
