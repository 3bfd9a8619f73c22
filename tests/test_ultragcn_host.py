"""CPU: the fp64 restatement of UltraGCN's loss (tests/ultragcn_torch.py) against torch's own operators and autograd."""
import numpy as np
import torch
import torch.nn.functional as F

import ultragcn_torch as UT


def _ops(B, K, M, D, seed):
    g = torch.Generator().manual_seed(seed)
    S = 1 + K + M
    return (torch.randn(B, D, generator=g, dtype=torch.float64), torch.randn(S * B, D, generator=g, dtype=torch.float64),
            torch.rand(B, S, generator=g, dtype=torch.float64))


def test_wbce_is_weighted_bce_with_logits():
    B, K, M, D = 5, 3, 2, 8
    Ub, Ib, w = _ops(B, K, M, D, 0)
    mul, l2, coef, s = UT.wbce64(Ub, Ib, w, K, M, Ub, Ib)
    target = (UT.labels(K, M) > 0).double()[None].expand(B, -1)
    want = F.binary_cross_entropy_with_logits(s, target, weight=w, reduction="sum") / B
    assert abs(float(mul - want)) <= 1e-13 * abs(float(want))
    it = Ib.reshape(1 + K + M, B, D)
    assert abs(float(l2) - 0.5 * float((Ub ** 2).sum() + (it[:1 + K] ** 2).sum()) / B) < 1e-12


def test_coef_is_the_gradient_of_the_loss_in_the_scores():
    B, K, M, D = 4, 2, 3, 6
    Ub, Ib, w = _ops(B, K, M, D, 1)
    s = ((Ub[None] * Ib.reshape(1 + K + M, B, D)).sum(-1).T).clone().requires_grad_()
    mul = (w * UT.softplus64(-UT.labels(K, M)[None] * s)).sum() / B
    mul.backward()
    coef = UT.wbce64(Ub, Ib, w, K, M)[2]
    assert torch.allclose(coef, s.grad, rtol=1e-12, atol=1e-15)


def test_softplus_is_stable_and_matches_torch():
    x = torch.tensor([-800.0, -60.0, -1.0, 0.0, 1.0, 60.0, 800.0], dtype=torch.float64)
    got = UT.softplus64(x)
    assert torch.isfinite(got).all() and got[-1] == 800.0 and got[0] == 0.0
    assert torch.allclose(got[1:-1], F.softplus(x[1:-1], threshold=1e9), rtol=1e-14, atol=0)


def test_model_loss_pads_weigh_nothing_and_repeat_nothing():
    nu, ni, D = 6, 7, 4
    g = torch.Generator().manual_seed(2)
    U = torch.randn(nu, D, generator=g, dtype=torch.float64, requires_grad=True)
    I = torch.randn(ni, D, generator=g, dtype=torch.float64, requires_grad=True)
    edges = [(0, 0), (0, 1), (1, 1), (2, 2), (3, 3), (4, 4), (5, 5), (5, 6)]
    bu, bi = UT.betas64(edges, nu, ni)
    assert float(bu[0]) == np.sqrt(3.0) / 2 and float(bi[1]) == 1 / np.sqrt(3.0)
    nbr_id = torch.tensor([[1, -1], [0, -1], [-1, -1], [-1, -1], [-1, -1], [6, -1], [5, -1]])
    nbr_w = torch.tensor([[0.5, 0], [0.25, 0], [0, 0], [0, 0], [0, 0], [0.75, 0], [0.125, 0]], dtype=torch.float64)
    batch = torch.tensor([[0, 0, 3, 4], [2, 2, 0, 1], [0, 1, 5, 6]])
    ids, pad = UT.slots(batch, nbr_id)
    assert ids.tolist() == [[0, 3, 4, 1, 0], [2, 0, 1, 2, 2], [1, 5, 6, 0, 1]] and pad.tolist() == [[False, True]] * 1 + [[True, True]] + [[False, True]]
    mul, l2 = UT.ultragcn_loss64(U, I, batch, bu, bi, nbr_id, nbr_w)
    mul0, _ = UT.ultragcn_loss64(U, I, batch, bu, bi, None, None)
    # the neighbour term by hand: lam * omega * softplus(-u . i_nbr) over the real neighbours
    want = mul0 + (0.5 * UT.softplus64(-(U[0] * I[1]).sum()) + 0.25 * UT.softplus64(-(U[0] * I[0]).sum())) / 3
    assert abs(float(mul - want)) < 1e-14
    (gI,) = torch.autograd.grad(mul - mul0, I)
    assert (gI[2:] == 0).all()                                # pads (replaced by the positive) carry an exact zero
    assert abs(float(l2) - 0.5 * float((U[[0, 2, 0]] ** 2).sum() + (I[batch[:, 1:]] ** 2).sum()) / 3) < 1e-13
