"""Plain fp64 restatements of what the NCL pull request adds (kmeans.py, the two contrast terms of help.py), on the CPU; no
project code.  test_ncl_host.py pins each to explicit Python loops at tiny sizes, the GPU tests compare the kernels to them.

    seeded_init(x, k, seed)            x[randperm(n, CPU generator seeded with seed)[:k]]
    scores(x, c)                       s_ij = x_i . c_j - 0.5 |c_j|^2           (argmax_j = the Euclidean nearest centroid)
    assign(x, c)                       argmax_j s_ij, ties to the lower id
    lloyd(x, k, n_iter, init)          Lloyd's algorithm: n_iter x (assign, per-cluster mean; a cluster without members keeps
                                       its previous centroid), then one final assignment
                                       -> (centroids [k, D], assign int64 [n], counts int64 [k], best [n])
    struct_loss(x0, A, nu, ni, batch, tau, alpha)      the structure term on a dense adjacency A
    proto_loss(x0, nu, ni, batch, cu, ci, clu, cli, tau, alpha)    the prototype term on given unit centroids and cluster ids
Both terms are MEANS over the batch (F.cross_entropy(reduction="mean")) and differentiable by autograd."""
import torch
import torch.nn.functional as F


def seeded_init(x, k, seed):
    gen = torch.Generator(device="cpu")
    gen.manual_seed(int(seed))
    return x[torch.randperm(x.shape[0], generator=gen)[:k]]


def scores(x, c):
    x, c = x.double(), c.double()
    return x @ c.T - 0.5 * (c * c).sum(1)[None, :]


def assign(x, c):
    """(assign, best): torch.max returns the FIRST maximal index on the CPU only by convention, so the tie rule is spelled out:
    the lowest id among the columns that equal the row maximum."""
    s = scores(x, c)
    best = s.max(1).values
    ids = torch.arange(s.shape[1])[None, :].expand_as(s)
    first = torch.where(s == best[:, None], ids, torch.full_like(ids, s.shape[1])).min(1).values
    return first, best


def lloyd(x, k, n_iter, init):
    x = x.double()
    c = init.double().clone()
    assert c.shape == (k, x.shape[1])
    for _ in range(n_iter):
        a, _ = assign(x, c)
        sums = torch.zeros_like(c).index_add_(0, a, x)
        counts = torch.zeros(k, dtype=torch.int64).index_add_(0, a, torch.ones_like(a))
        c = torch.where((counts > 0)[:, None], sums / counts.clamp(min=1)[:, None].double(), c)
    a, best = assign(x, c)
    counts = torch.zeros(k, dtype=torch.int64).index_add_(0, a, torch.ones_like(a))
    return c, a, counts, best


def _contrast(q, t, target, tau):
    return F.cross_entropy(q @ t.T / tau, target, reduction="mean")


def struct_loss(x0, A, n_user, n_item, batch, tau, alpha):
    """x0 [n, D] fp64 (requires_grad for the gradient), A [n, n] dense fp64, batch int64 [B, >= 2]."""
    ub, ib = batch[:, 0], batch[:, 1]
    y2 = A @ (A @ x0)
    U0, I0 = x0[:n_user], x0[n_user:n_user + n_item]
    l_u = _contrast(F.normalize(y2[ub], dim=1), F.normalize(U0, dim=1), ub, tau)
    l_i = _contrast(F.normalize(y2[n_user + ib], dim=1), F.normalize(I0, dim=1), ib, tau)
    return l_u + alpha * l_i


def proto_loss(x0, n_user, n_item, batch, cent_u, cent_i, cluster_u, cluster_i, tau, alpha):
    """cent_* [K, D]: unit rows, constants; cluster_* int64 ids of every user / item."""
    ub, ib = batch[:, 0], batch[:, 1]
    U0, I0 = x0[:n_user], x0[n_user:n_user + n_item]
    l_u = _contrast(F.normalize(U0[ub], dim=1), cent_u.detach(), cluster_u[ub], tau)
    l_i = _contrast(F.normalize(I0[ib], dim=1), cent_i.detach(), cluster_i[ib], tau)
    return l_u + alpha * l_i


def blobs(n_blob=7, per=40, D=16, spread=10.0, sigma=0.1, seed=5):
    """Separated blobs: centres on a scaled axis grid (pairwise distance >= spread), `per` rows each at N(centre, sigma^2).
    -> (x float32 [n_blob per, D] in a shuffled order, labels int64, centres float32 [n_blob, D])."""
    g = torch.Generator().manual_seed(seed)
    centres = torch.zeros(n_blob, D)
    for b in range(n_blob):
        centres[b, b % D] = spread * (1 + b // D)
        centres[b, (b + 3) % D] -= spread * 0.5
    labels = torch.arange(n_blob).repeat_interleave(per)
    x = centres[labels] + sigma * torch.randn(n_blob * per, D, generator=g)
    perm = torch.randperm(x.shape[0], generator=g)
    return x[perm].float().contiguous(), labels[perm].contiguous(), centres.float()
