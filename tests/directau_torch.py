"""fp64 restatement of the DirectAU loss (rowops.directau_fwd / help.align_uniform_loss) in plain torch: F.normalize, explicit
pair differences over torch.triu_indices, exp, mean, log and autograd -- what the tests compare against.  Nothing is read
from the library.

Compact operands Ub [B, D], Ib [B, D]: row b of Ib is the positive of row b of Ub; repeated rows are kept.
    x^      = x / max(|x|, 1e-12)
    align   = mean_b |u^_b - i^_b|^2
    unif(X) = log mean_{i < j} exp(-t |x^_i - x^_j|^2)
    loss    = align + gamma (unif(U) + unif(I)) / 2
    l2      = 0.5 (sum |Ureg rows|^2 + sum |Ireg rows|^2) / B
"""
import torch
import torch.nn.functional as F


def normalize64(x):
    return F.normalize(x.double(), p=2, dim=1, eps=1e-12)


def align64(Ub, Ib):
    return (normalize64(Ub) - normalize64(Ib)).pow(2).sum(1).mean()


def pair_terms64(X, t):
    """exp(-t |x^_i - x^_j|^2) of every pair i < j, in the order of torch.triu_indices -> [B (B - 1) / 2]."""
    xh = normalize64(X)
    i, j = torch.triu_indices(X.shape[0], X.shape[0], offset=1)
    return torch.exp(-t * (xh[i] - xh[j]).pow(2).sum(1))


def uniform64(X, t):
    return pair_terms64(X, t).mean().log()


def directau_loss64(Ub, Ib, Ureg, Ireg, t=2.0, gamma=1.0):
    """(mul_loss, l2reg_loss, [align, unif_u, unif_i]) in fp64 on compact rows; differentiable w.r.t. whatever requires grad."""
    a, uu, ui = align64(Ub, Ib), uniform64(Ub, t), uniform64(Ib, t)
    B = Ub.shape[0]
    reg = 0.5 * (Ureg.double().pow(2).sum() + Ireg.double().pow(2).sum()) / B if Ureg is not None else torch.zeros((), dtype=torch.float64)
    return a + gamma * (uu + ui) / 2, reg, torch.stack([a, uu, ui])


def directau_tables64(U, I, Ureg, Ireg, pairs, t=2.0, gamma=1.0):
    """The same on tables and a [B, 2] (user, positive) batch: the rows are gathered, repeats kept."""
    u, i = pairs[:, 0], pairs[:, 1]
    return directau_loss64(U[u], I[i], None if Ureg is None else Ureg[u], None if Ireg is None else Ireg[i], t, gamma)
