"""fp64 torch restatement of UltraGCN's loss as this repository states it (help.ultragcn_loss, include/tagrec.h):

    slots of tuple b: j = 0 the positive (t = +1), 1 .. K the negatives (t = -1), K + 1 .. K + M the positive's co-occurrence
    neighbours (t = +1);  s_bj = u_b . i_bj
    mul_loss = (1 / B) sum_b sum_j w_bj softplus(-t_j s_bj),   softplus(x) = max(x, 0) + log1p(exp(-|x|))
    coef[b, j] = -t_j w_bj sigmoid(-t_j s_bj) / B
    l2reg    = 0.5 (|u|^2 + sum_{j <= K} |i_j|^2) / B                      (the neighbour slots carry none)
    weights: positive w1 + w2 b_u b_i;  negative (w3 + w4 b_u b_j) negative_weight / K;  neighbour lambda omega
             b_u = sqrt(d_u + 1) / d_u (0 at d_u = 0), b_i = 1 / sqrt(d_i + 1)
"""
import numpy as np
import torch


def softplus64(x):
    return torch.clamp(x, min=0) + torch.log1p(torch.exp(-x.abs()))


def labels(K, M):
    t = torch.ones(1 + K + M, dtype=torch.float64)
    t[1:1 + K] = -1
    return t


def wbce64(Ub, Ib, weight, K, M, Ureg=None, Ireg=None):
    """Compact operands (any float dtype, taken to fp64) -> (mul_loss, l2reg, coef [B, S], scores [B, S])."""
    B, D = Ub.shape
    S = 1 + K + M
    u, it, w = Ub.double(), Ib.double().reshape(S, B, D), weight.double()
    s = (u[None] * it).sum(-1).T                             # [B, S]
    x = -labels(K, M)[None] * s
    mul = (w * softplus64(x)).sum() / B
    coef = -labels(K, M)[None] * w * torch.sigmoid(x) / B
    l2 = torch.zeros((), dtype=torch.float64)
    if Ureg is not None:
        Dr = Ureg.shape[1]
        l2 = 0.5 * ((Ureg.double() ** 2).sum() + (Ireg.double().reshape(S, B, Dr)[:1 + K] ** 2).sum()) / B
    return mul, l2, coef, s


def betas64(edges, n_user, n_item):
    e = np.unique(np.asarray(edges, dtype=np.int64).reshape(-1, 2), axis=0)
    du = np.bincount(e[:, 0], minlength=n_user).astype(np.float64)
    di = np.bincount(e[:, 1], minlength=n_item).astype(np.float64)
    bu = np.where(du > 0, np.sqrt(du + 1) / np.maximum(du, 1), 0.0)
    return torch.from_numpy(bu), torch.from_numpy(1.0 / np.sqrt(di + 1))


def slots(batch, nbr_id):
    """(item ids [B, S] with pads replaced by the positive, pad mask [B, M]) of a [B, 2 + K] batch; nbr_id int [n_item, M] or None."""
    items = batch[:, 1:]
    if nbr_id is None or nbr_id.shape[1] == 0:
        return items, None
    nb = torch.as_tensor(nbr_id).long()[batch[:, 1]]
    pad = nb < 0
    return torch.cat([items, torch.where(pad, batch[:, 1:2], nb)], 1), pad


def weights64(batch, beta_u, beta_i, nbr_id, nbr_w, w, negative_weight, lam):
    K = batch.shape[1] - 2
    bu = beta_u[batch[:, 0]][:, None]
    parts = [w[0] + w[1] * bu * beta_i[batch[:, 1]][:, None], (w[2] + w[3] * bu * beta_i[batch[:, 2:]]) * (negative_weight / K)]
    if nbr_id is not None and nbr_id.shape[1]:
        parts.append(lam * torch.as_tensor(nbr_w).double()[batch[:, 1]])
    return torch.cat(parts, 1)


def ultragcn_loss64(U, I, batch, beta_u, beta_i, nbr_id, nbr_w, w=(1e-6, 1.0, 1e-6, 1.0), negative_weight=10.0, lam=1.0):
    """(mul_loss, l2reg) of fp64 tables U / I (autograd flows into them) and a [B, 2 + K] int64 batch."""
    B, K = batch.shape[0], batch.shape[1] - 2
    ids, _ = slots(batch, nbr_id)
    M = ids.shape[1] - 1 - K
    wt = weights64(batch, beta_u.double(), beta_i.double(), nbr_id, nbr_w, w, negative_weight, lam)
    u, it = U[batch[:, 0]], I[ids]                           # [B, D], [B, S, D]
    s = (u[:, None] * it).sum(-1)
    mul = (wt * softplus64(-labels(K, M)[None] * s)).sum() / B
    l2 = 0.5 * ((u ** 2).sum() + (it[:, :1 + K] ** 2).sum()) / B
    return mul, l2
