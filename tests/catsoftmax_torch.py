"""fp64 restatement of the catalogue softmax loss (rowops.catsoftmax_fwd / help.catalogue_softmax_loss) in plain torch:
logits from a matmul, F.cross_entropy(reduction="mean") and autograd -- what the tests compare against.  It is deliberately
not the logsumexp form the kernels evaluate.  Nothing is read from the library.

Operands Q [nq, D] (row b of the problem is Q[qrow[b]]; qrow None: row b), T [N, D], target [B] in [0, N):
    z_bn = Q[qrow_b] . T[n] / tau
    loss = mean_b [ -log softmax_n(z_b)[target_b] ]
    l2   = 0.5 (sum_b |Qreg[qrow_b]|^2 + sum_b |Treg[target_b]|^2) / B
"""
import torch
import torch.nn.functional as F


def logits64(Q, T, tau=1.0, qrow=None):
    q = Q.double() if qrow is None else Q.double()[qrow]
    return q @ T.double().t() / tau


def catalogue_loss64(Q, T, target, Qreg, Treg, tau=1.0, qrow=None):
    """(mul_loss, l2reg_loss) in fp64; differentiable w.r.t. whatever requires grad."""
    loss = F.cross_entropy(logits64(Q, T, tau, qrow), target, reduction="mean")
    if Qreg is None:
        return loss, torch.zeros((), dtype=torch.float64)
    B = target.shape[0]
    qr = Qreg.double() if qrow is None else Qreg.double()[qrow]
    return loss, 0.5 * (qr.pow(2).sum() + Treg.double()[target].pow(2).sum()) / B


def catalogue_tables64(U, I, Ureg, Ireg, pairs, tau=1.0):
    """The same on user / item tables and a [B, 2] (user, positive) batch: the users' rows are gathered, every item is a column."""
    return catalogue_loss64(U, I, pairs[:, 1], Ureg, Ireg, tau, pairs[:, 0])
