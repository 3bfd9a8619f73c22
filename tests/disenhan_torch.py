"""Plain-torch restatement of DisenHAN (the reference's model/disenhan.py) on the merged relation structures: the
yardstick of the CPU parity tests, the GPU kernel tests (in fp64) and tools/disenhan_step.py (the GPU baseline).

The reference's per-entry attention `relu(<[new_a[i]_k, ego_b[j]_k], at[e,k]>)` is split into a row half and a column
half, sL[i,k] = <new_a[i]_k, at[e,k,:dk]> and sR[j,k] = <ego_b[j]_k, at[e,k,dk:]>; a merged entry of multiplicity m has
the logit m * sum_k r[i,k] relu(sL[i,k] + sR[j,k]) (torch.sparse.softmax coalesces duplicates by summing).  Any dtype
and device; autograd gives the gradients."""
import torch
import torch.nn.functional as F

# relation e: (row type, column type) -- ui iu ut tu it ti (disenhan.py:79); node types user 0, item 1, tag 2
INDEX = ((0, 1), (1, 0), (0, 2), (2, 0), (1, 2), (2, 1))
# the relations added into each node type's new factors (disenhan.py:91-93)
COMBINE = ((0, 2), (1, 4), (3, 5))


def coo(rel, device=None):
    """(rows, cols, mult, shape) of a merged relation (rowptr, col, mult, shape) as int64 / float tensors."""
    rowptr, col, mult, shape = rel
    rows = torch.repeat_interleave(torch.arange(shape[0]), rowptr[1:] - rowptr[:-1])
    return rows.to(device), col.long().to(device), mult.to(device), shape


def edge_softmax(sL, sR, r, rows, cols, mult, n_rows):
    """alpha over each row's merged entries."""
    logit = mult.to(sL.dtype) * (r[rows] * torch.relu(sL[rows] + sR[cols])).sum(1)
    mx = torch.full((n_rows,), -float("inf"), dtype=logit.dtype, device=logit.device)
    mx = mx.scatter_reduce(0, rows, logit.detach(), "amax")
    ex = torch.exp(logit - mx[rows])
    den = torch.zeros(n_rows, dtype=logit.dtype, device=logit.device).index_add(0, rows, ex)
    return ex / den[rows]


def rel_epilogue(Y, W, q, K):
    """(Z, r): Z = leaky_0.2(Y) W per factor slice, r = softmax_k <tanh(Z_k), q> (disenhan.py:51-59)."""
    n, D = Y.shape
    Z = F.leaky_relu(Y, 0.2).view(n, K, D // K) @ W
    r = torch.softmax((torch.tanh(Z) * q).sum(-1), dim=1)
    return Z.reshape(n, D), r


def combine(ego, terms, K):
    """slice_normalize(ego + sum r_e * Z_e) (disenhan.py:62-66)."""
    n, D = ego.shape
    x = ego.view(n, K, D // K)
    for Z, r in terms:
        x = x + Z.view(n, K, D // K) * r.unsqueeze(2)
    return F.normalize(x, p=2, dim=2).reshape(n, D)


def layer(embs, Wtk, at, W, q_rela, rels, K, iterate=2):
    """One Layer.forward; embs / result: [user, item, tag] [n, D]; rels: six coo() tuples."""
    D = embs[0].shape[1]
    dk = D // K
    ego = []
    for t in range(3):
        f = F.leaky_relu(torch.einsum("nd,kde->nke", embs[t], Wtk[t]), 0.2)
        ego.append(F.normalize(f, p=2, dim=2).reshape(-1, D))
    new = ego
    r = [torch.full((rels[e][3][0], K), 1.0 / K, dtype=embs[0].dtype, device=embs[0].device) for e in range(6)]
    for _ in range(iterate):
        outs = []
        for e, (a, b) in enumerate(INDEX):
            rows, cols, mult, shape = rels[e]
            sL = (new[a].view(-1, K, dk) * at[e, :, :dk]).sum(-1)
            sR = (ego[b].view(-1, K, dk) * at[e, :, dk:]).sum(-1)
            alpha = edge_softmax(sL, sR, r[e], rows, cols, mult, shape[0])
            Y = torch.zeros(shape[0], D, dtype=alpha.dtype, device=alpha.device).index_add(0, rows, alpha[:, None] * ego[b][cols])
            outs.append(rel_epilogue(Y, W, q_rela[e], K))
        new = [combine(ego[t], [outs[e] for e in COMBINE[t]], K) for t in range(3)]
        r = [o[1] for o in outs]
    return new


def forward(embs, layers, rels, K, iterate=2):
    """layers: list of (Wtk, at, W, q_rela)."""
    x = list(embs)
    for Wtk, at, W, q in layers:
        x = layer(x, Wtk, at, W, q, rels, K, iterate)
    return x


def loss(out, batch, reg, loss_func="softplus"):
    """(mul_loss, reg * l2reg_loss) on the propagated rows (disenhan.py:184-214)."""
    users, pos, neg = batch.long().T
    u, p, n = out[0][users], out[1][pos], out[1][neg]
    ps, ns = (u * p).sum(1), (u * n).sum(1)
    if loss_func == "logsigmoid":
        main = -F.logsigmoid(ps - ns).mean()
    else:
        main = F.softplus(ns - ps).mean()
    l2 = 0.5 * (u.norm(2).pow(2) + p.norm(2).pow(2) + n.norm(2).pow(2)) / float(u.shape[0])
    return main, reg * l2


def params_from_state(sd, n_layer, dtype=torch.float64, device=None):
    """(tables, layers) from a state dict keyed like the reference's (embed.0-2, layer.{i}.Wtk/at/W/q_rela)."""
    cv = lambda v: torch.as_tensor(v).to(dtype=dtype, device=device).clone().requires_grad_()
    tables = [cv(sd[f"embed.{t}"]) for t in range(3)]
    layers = [tuple(cv(sd[f"layer.{i}.{n}"]) for n in ("Wtk", "at", "W", "q_rela")) for i in range(n_layer)]
    return tables, layers
