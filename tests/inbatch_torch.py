"""fp64 restatement of the in-batch softmax loss (rowops.inbatch_fwd / help.in_batch_loss) in plain torch: logits from a
matmul, masked_fill(-inf), torch.logsumexp and autograd -- what the tests compare against.  Nothing is read from the library.

Compact operands Ub [B, D], Ib [B, D]: row b of Ib is the positive of row b of Ub, every other row a negative.
    z_bj   = Ub[b] . Ib[j] / tau - col_bias[j]
    masked   (b, j), j != b, with iid[j] == iid[b] or uid[j] == uid[b]
    loss   = mean_b [ logsumexp_{j unmasked} z_bj - z_bb ]
    l2     = 0.5 (sum |Ureg rows|^2 + sum |Ireg rows|^2) / B
"""
import torch


def mask(uid, iid):
    """[B, B] bool: the entries left out of the softmax (never the diagonal)."""
    same = (iid[None, :] == iid[:, None]) | (uid[None, :] == uid[:, None])
    return same & ~torch.eye(uid.shape[0], dtype=torch.bool)


def logits64(Ub, Ib, tau=1.0, col_bias=None):
    z = Ub.double() @ Ib.double().t() / tau
    return z if col_bias is None else z - col_bias.double()[None, :]


def lse64(z, m=None):
    """Row log-sum-exp over the unmasked entries of fp64 logits z [B, B]."""
    return torch.logsumexp(z if m is None else z.masked_fill(m, float("-inf")), dim=1)


def in_batch_loss64(Ub, Ib, Ureg, Ireg, tau=1.0, uid=None, iid=None, col_bias=None):
    """(mul_loss, l2reg_loss) in fp64 on compact rows; differentiable w.r.t. whatever requires grad."""
    z = logits64(Ub, Ib, tau, col_bias)
    m = None if uid is None else mask(uid, iid)
    loss = (lse64(z, m) - torch.diagonal(z)).mean()
    B = Ub.shape[0]
    reg = 0.5 * (Ureg.double().pow(2).sum() + Ireg.double().pow(2).sum()) / B if Ureg is not None else torch.zeros((), dtype=torch.float64)
    return loss, reg


def in_batch_tables64(U, I, Ureg, Ireg, pairs, tau=1.0, item_logq=None):
    """The same on tables and a [B, 2] (user, positive) batch: the rows are gathered, the mask ids are the two columns and
    col_bias = item_logq[pairs[:, 1]]."""
    u, i = pairs[:, 0], pairs[:, 1]
    bias = None if item_logq is None else item_logq[i]
    return in_batch_loss64(U[u], I[i], None if Ureg is None else Ureg[u], None if Ireg is None else Ireg[i], tau, u, i, bias)


def sampled_form(z):
    """[B, B] logits -> [B, 1 + (B - 1)]: column 0 the diagonal, then the other columns in ascending order -- in-batch softmax
    is sampled softmax with K = B - 1 whose negatives are the other positives."""
    B = z.shape[0]
    off = z[~torch.eye(B, dtype=torch.bool)].reshape(B, B - 1)
    return torch.cat([torch.diagonal(z)[:, None], off], dim=1)
