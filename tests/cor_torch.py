"""Torch restatement of the distance-correlation loss between factor slices (helper of test_cor_host.py and
test_gpu_cor.py, not a test file).  Float-generic: it computes in the dtype of X.

Direct two-pass form: |x_i - x_j|^2 as sum (x_i - x_j)^2, centred with the means of a first pass before anything is
multiplied.  `cor_loss_and_grad` also returns the analytic gradient (no autograd): centring is a projection, so
d sum(A^f A^g) / d d^f = A^g, and the loss depends on the 2K - 1 covariance sums through a few scalars."""
import torch


def _centred(X, K):
    n, D = X.shape
    Xs = X.reshape(n, K, D // K).permute(1, 0, 2)                       # [K, n, dk]
    diff = Xs[:, :, None, :] - Xs[:, None, :, :]
    d = torch.sqrt((diff * diff).sum(-1) + 1e-8)                        # [K, n, n]; the diagonal is 1e-4
    rm = d.mean(2, keepdim=True)
    A = d - rm - rm.transpose(1, 2) + d.mean((1, 2), keepdim=True)
    return diff, d, A


def _dcov(s, n):
    return torch.sqrt(torch.clamp(s / float(n * n), min=0) + 1e-8)


def cor_loss(X, K):
    """loss (0-d, dtype of X) of X [n, D] split into K column slices; K = 1 -> 0."""
    n = X.shape[0]
    if K == 1:
        return X.new_zeros(())
    _, _, A = _centred(X, K)
    loss = X.new_zeros(())
    for f in range(K - 1):                                              # adjacent pairs only
        xy, xx, yy = _dcov((A[f] * A[f + 1]).sum(), n), _dcov((A[f] * A[f]).sum(), n), _dcov((A[f + 1] * A[f + 1]).sum(), n)
        loss = loss + xy / (torch.sqrt(torch.clamp(xx * yy, min=0)) + 1e-10)
    return loss / ((K + 1.0) * K / 2)


def cor_loss_and_grad(X, K):
    """(loss, d loss / dX) by the analytic gradient."""
    n = X.shape[0]
    if K == 1:
        return X.new_zeros(()), torch.zeros_like(X)
    diff, d, A = _centred(X, K)
    n2, Z = float(n * n), (K + 1.0) * K / 2
    sff = (A * A).sum((1, 2))
    sfg = (A[:-1] * A[1:]).sum((1, 2))
    vff, vfg = _dcov(sff, n), _dcov(sfg, n)
    root = torch.sqrt(torch.clamp(vff[:-1] * vff[1:], min=0))
    den = root + 1e-10
    loss = (vfg / den).sum() / Z
    step = lambda s: (s > 0).to(X.dtype) + 0.5 * (s == 0).to(X.dtype)   # d max(s, 0) / ds, a tie split as torch.maximum does
    g_fg = step(sfg) / (den * Z) / (2 * vfg * n2)
    d_den = -vfg / (den * den * Z)
    g_xx = d_den * vff[1:] / (2 * root) * step(sff[:-1]) / (2 * vff[:-1] * n2)
    g_yy = d_den * vff[:-1] / (2 * root) * step(sff[1:]) / (2 * vff[1:] * n2)
    g_ff = torch.zeros_like(sff)
    g_ff[:-1] += g_xx
    g_ff[1:] += g_yy
    G = 2 * g_ff[:, None, None] * A                                     # d loss / d d^f
    G[:-1] += g_fg[:, None, None] * A[1:]
    G[1:] += g_fg[:, None, None] * A[:-1]
    gx = 2 * ((G / d)[..., None] * diff).sum(2)                         # [K, n, dk]
    return loss, gx.permute(1, 0, 2).reshape(X.shape)
