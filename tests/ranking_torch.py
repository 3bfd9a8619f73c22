"""fp64 restatement of the multi-negative ranking losses (rowops.rank_fwd / help.ranking_loss) in plain torch: the
definitions written out with torch.logsumexp, F.softplus, F.logsigmoid and autograd -- what the GPU tests compare against.

A batch is int64 [B, 2 + K] = (u, p, n_1 .. n_K); scores s_0 = u . p, s_k = u . n_k.
    "softmax"     mean_b [ logsumexp(s_0 / tau, .., s_K / tau) - s_0 / tau ]
    "softplus"    mean over the B K pairs of softplus(s_k - s_0)        (F.softplus: identity, slope 1, past 20)
    "logsigmoid"  mean over the B K pairs of -logsigmoid(s_0 - s_k)
    l2            0.5 (|u|^2 + |p|^2 + sum_k |n_k|^2) / B on the rows of the L2 tables
"""
import torch
import torch.nn.functional as F

LOSSES = ("softplus", "logsigmoid", "softmax")


def scores64(U, I, tuples):
    """[B, 1 + K] fp64 scores of a tuple batch against tables U [nu, D], I [ni, D]."""
    u = U.double()[tuples[:, 0]]
    it = I.double()[tuples[:, 1:]]                       # [B, 1 + K, D]
    return (u[:, None, :] * it).sum(-1)


def mul_loss64(s, loss_func, tau=1.0):
    """The ranking part from fp64 scores s [B, 1 + K] (column 0 the positive)."""
    if loss_func == "softmax":
        z = s / tau
        return (torch.logsumexp(z, dim=1) - z[:, 0]).mean()
    if loss_func == "softplus":
        return F.softplus(s[:, 1:] - s[:, :1]).mean()
    if loss_func == "logsigmoid":
        return (-F.logsigmoid(s[:, :1] - s[:, 1:])).mean()
    raise ValueError(loss_func)


def l2_64(Ureg, Ireg, tuples):
    B = tuples.shape[0]
    return 0.5 * (Ureg.double()[tuples[:, 0]].pow(2).sum() + Ireg.double()[tuples[:, 1:]].pow(2).sum()) / B


def ranking_loss64(U, I, Ureg, Ireg, tuples, loss_func, tau=1.0):
    """(mul_loss, l2reg_loss) in fp64; differentiable w.r.t. whatever of U / I / Ureg / Ireg requires grad."""
    loss = mul_loss64(scores64(U, I, tuples), loss_func, tau)
    reg = l2_64(Ureg, Ireg, tuples) if Ureg is not None else torch.zeros((), dtype=torch.float64)
    return loss, reg


def compact_tuples(B, K):
    """The tuple batch of compact operands Ub [B, D] / Ib [(1 + K) B, D]: item j of tuple b is row j B + b."""
    b = torch.arange(B)
    return torch.cat([b[:, None], b[:, None] + B * torch.arange(1 + K)[None, :]], dim=1)


def pair_loss64(x, loss_func):
    """The per-pair expression at gap x = s_k - s_0 (fp64 tensor): F.softplus(x) or -F.logsigmoid(-x)."""
    return F.softplus(x) if loss_func == "softplus" else -F.logsigmoid(-x)


def coef64(s, loss_func, tau=1.0):
    """d loss_b / d s_j [B, 1 + K] by autograd (loss_b = the tuple's term of the batch mean, times B)."""
    s = s.detach().clone().requires_grad_()
    (mul_loss64(s, loss_func, tau) * s.shape[0]).backward()
    return s.grad
