"""Host: the fp64 restatement of tests/ncl_torch.py against explicit Python loops at tiny sizes, the seeded init, the blobs
the GPU tests cluster, and the "ncl" configuration (no GPU)."""
import math

import pytest
import torch

import tagrec_amd as T
from tagrec_amd.kmeans import seeded_rows       # the draw the restatement's init is pinned to

import ncl_torch as NT


def _rand(*shape, seed):
    return torch.randn(*shape, generator=torch.Generator().manual_seed(seed), dtype=torch.float64)


def _loop_assign(x, c):
    out, best = [], []
    for i in range(x.shape[0]):
        bi, bs = -1, -math.inf
        for j in range(c.shape[0]):
            s = sum(float(x[i, d]) * float(c[j, d]) for d in range(x.shape[1])) - 0.5 * sum(float(c[j, d]) ** 2 for d in range(x.shape[1]))
            if s > bs:                                   # strict: a tie keeps the lower id
                bi, bs = j, s
        out.append(bi)
        best.append(bs)
    return out, best


def _loop_lloyd(x, init, n_iter):
    c = [[float(v) for v in row] for row in init]
    n, D, k = x.shape[0], x.shape[1], len(c)
    for _ in range(n_iter):
        a, _ = _loop_assign(x, torch.tensor(c, dtype=torch.float64))
        for j in range(k):
            members = [i for i in range(n) if a[i] == j]
            if members:                                  # an empty cluster keeps its row
                c[j] = [sum(float(x[i, d]) for i in members) / len(members) for d in range(D)]
    a, best = _loop_assign(x, torch.tensor(c, dtype=torch.float64))
    return c, a, [a.count(j) for j in range(k)], best


def test_assign_and_lloyd_against_loops():
    x = _rand(23, 5, seed=1)
    init = x[[3, 7, 11, 19]].clone()
    far = torch.full((1, 5), 50.0, dtype=torch.float64)                  # a centroid no row is nearest to: stays empty
    init = torch.cat([init, far])
    for n_iter in (0, 1, 3):
        c, a, counts, best = NT.lloyd(x, 5, n_iter, init)
        lc, la, lcounts, lbest = _loop_lloyd(x, init, n_iter)
        assert a.tolist() == la and counts.tolist() == lcounts
        assert torch.allclose(c, torch.tensor(lc, dtype=torch.float64), rtol=1e-12, atol=1e-12)
        assert torch.allclose(best, torch.tensor(lbest, dtype=torch.float64), rtol=1e-12, atol=1e-12)
        assert counts[4] == 0 and torch.equal(c[4], far[0])              # the empty-cluster rule
        assert int(counts.sum()) == 23


def test_ties_go_to_the_lower_id():
    x = _rand(9, 4, seed=2)
    c = _rand(6, 4, seed=3)
    c[4] = c[1]                                                          # identical rows score identically
    a, _ = NT.assign(x, c)
    assert 4 not in a.tolist()
    assert a.tolist() == _loop_assign(x, c)[0]


def test_euclidean_nearest():
    x, c = _rand(31, 6, seed=4), _rand(7, 6, seed=5)
    a, best = NT.assign(x, c)
    d2 = ((x[:, None, :] - c[None, :, :]) ** 2).sum(2)
    assert torch.equal(a, d2.argmin(1))
    assert torch.allclose((x * x).sum(1) - 2 * best, d2.min(1).values, rtol=1e-12, atol=1e-12)      # the inertia from best


def test_seeded_init():
    x = _rand(50, 4, seed=6)
    for seed in (0, 7, 2020 << 24):
        g = torch.Generator(device="cpu")
        g.manual_seed(seed)
        perm = torch.randperm(50, generator=g)
        assert torch.equal(NT.seeded_init(x, 9, seed), x[perm[:9]])
        assert len(set(perm[:9].tolist())) == 9                          # k distinct rows
    g = torch.Generator(device="cpu")
    g.manual_seed(11)
    assert torch.equal(seeded_rows(50, 9, 11), torch.randperm(50, generator=g)[:9])      # the package draws the same rows


def test_blobs_are_recovered_in_three_iterations():
    x, labels, centres = NT.blobs()
    assert x.shape == (280, 16)
    d = torch.cdist(centres.double(), centres.double()) + torch.eye(7) * 1e9
    assert d.min() >= 10.0
    init = torch.stack([x[(labels == b).nonzero()[0, 0]] for b in range(7)])          # one data row per blob
    for n_iter in (1, 2, 3):
        c, a, counts, _ = NT.lloyd(x, 7, n_iter, init)
        assert torch.equal(a, labels) and counts.tolist() == [40] * 7
        means = torch.stack([x[labels == b].double().mean(0) for b in range(7)])
        assert torch.allclose(c, means, rtol=1e-12, atol=1e-12)


def _loop_contrast(q, t, target, tau):
    tot = 0.0
    for b in range(len(q)):
        qn = math.sqrt(sum(v * v for v in q[b]))
        z = [sum((q[b][d] / qn) * t[n][d] for d in range(len(q[b]))) / tau for n in range(len(t))]
        m = max(z)
        tot += m + math.log(sum(math.exp(v - m) for v in z)) - z[target[b]]
    return tot / len(q)


def _unit(rows):
    out = []
    for r in rows:
        nr = math.sqrt(sum(v * v for v in r))
        out.append([v / nr for v in r])
    return out


def test_terms_against_loops():
    nu, ni, D, tau, alpha = 5, 4, 3, 0.3, 0.7
    n = nu + ni
    x0 = _rand(n, D, seed=8)
    A = torch.zeros(n, n, dtype=torch.float64)
    A[:nu, nu:] = _rand(nu, ni, seed=9).abs()
    A[nu:, :nu] = A[:nu, nu:].T
    batch = torch.tensor([[0, 1, 2], [3, 1, 0], [0, 2, 3], [4, 3, 1]])            # user 0 and item 1 repeat
    got = float(NT.struct_loss(x0, A, nu, ni, batch, tau, alpha))
    y2 = (A @ (A @ x0)).tolist()
    xl = x0.tolist()
    ub, ib = batch[:, 0].tolist(), batch[:, 1].tolist()
    want = _loop_contrast([y2[u] for u in ub], _unit(xl[:nu]), ub, tau) \
        + alpha * _loop_contrast([y2[nu + i] for i in ib], _unit(xl[nu:]), ib, tau)
    assert abs(got - want) <= 1e-12 * max(1.0, abs(want))

    cu, ci = _unit(_rand(3, D, seed=10).tolist()), _unit(_rand(2, D, seed=11).tolist())
    clu, cli = [0, 2, 1, 1, 0], [1, 0, 0, 1]
    got = float(NT.proto_loss(x0, nu, ni, batch, torch.tensor(cu, dtype=torch.float64), torch.tensor(ci, dtype=torch.float64),
                              torch.tensor(clu), torch.tensor(cli), tau, alpha))
    want = _loop_contrast([xl[u] for u in ub], cu, [clu[u] for u in ub], tau) \
        + alpha * _loop_contrast([xl[nu + i] for i in ib], ci, [cli[i] for i in ib], tau)
    assert abs(got - want) <= 1e-12 * max(1.0, abs(want))

    # autograd reaches the table through both operands of the structure term, through the batch rows only of the prototype term
    x = x0.clone().requires_grad_()
    NT.struct_loss(x, A, nu, ni, batch, tau, alpha).backward()
    assert (x.grad.abs().sum(1) > 0).all()
    x = x0.clone().requires_grad_()
    NT.proto_loss(x, nu, ni, batch, torch.tensor(cu, dtype=torch.float64), torch.tensor(ci, dtype=torch.float64),
                  torch.tensor(clu), torch.tensor(cli), tau, alpha).backward()
    touched = set(ub) | {nu + i for i in ib}
    assert {r for r in range(n) if float(x.grad[r].abs().sum()) > 0} == touched


DEFAULTS = {"ncl_struct_rate": 5e-4, "ncl_proto_rate": 3e-4, "ncl_alpha": 1.0, "ncl_temperature": 0.1, "ncl_clusters": 1000,
            "ncl_kmeans_iters": 20, "ncl_warm_up": 20}


def test_config_defaults():
    cfg = T.get_config("ncl")
    for k, v in DEFAULTS.items():
        assert cfg[k] == v and type(cfg[k]) is type(v), k
    assert cfg["use_tag"] is False and cfg["model"] == "ncl" and cfg["mul_loss_func"] == "softplus" and cfg["norm_type"] == "bi_norm"
    assert T.config.check_ncl(cfg) == (5e-4, 3e-4, 1.0, 0.1, 1000, 20, 20)
    assert "ncl_clusters" not in T.get_config("lightgcn")


NAN, INF = float("nan"), float("inf")
BAD = {"ncl_struct_rate": (-1e-3, NAN, INF, True, "0.1", None),
       "ncl_proto_rate": (-1e-3, NAN, INF, False, "0.1", None),
       "ncl_alpha": (-1.0, NAN, INF, True, "1", None),
       "ncl_temperature": (0, 0.0, -0.1, NAN, INF, True, "0.1", None),
       "ncl_clusters": (0, -3, 2.0, 1.5, True, "10", None),
       "ncl_kmeans_iters": (0, -1, 20.0, False, "20", None),
       "ncl_warm_up": (-1, 1.0, 0.5, True, "0", None)}


@pytest.mark.parametrize("key", sorted(BAD))
def test_config_refusals(key):
    for bad in BAD[key]:
        with pytest.raises(T.TagrecError, match=key):
            T.get_config("ncl", **{key: bad})
    good = {"ncl_struct_rate": 0, "ncl_proto_rate": 0.0, "ncl_alpha": 0, "ncl_temperature": 1e-3, "ncl_clusters": 1,
            "ncl_kmeans_iters": 1, "ncl_warm_up": 0}
    assert T.get_config("ncl", **{key: good[key]})[key] == good[key]
