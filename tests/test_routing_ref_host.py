"""CPU-only: the fp64 references of tests/routing_ref.py against torch autograd in fp64 and the oracle's DGCF routing step --
what makes them independent of the kernels they judge in test_gpu_routing_kernels.py."""
import numpy as np
import torch
import torch.nn.functional as F

import routing_ref as RR
import spmm_ref as R
from oracle import models as om
from test_spmm_ref_host import _small_csr

RTOL = 1e-12


def _t(a):
    return torch.from_numpy(np.ascontiguousarray(a, dtype=np.float64))


def _close(got, want, atol=0.0):
    np.testing.assert_allclose(got, want.detach().numpy() if isinstance(want, torch.Tensor) else want, rtol=RTOL, atol=atol)


def _covers(ref, mag):
    assert (np.asarray(mag) >= np.abs(ref)).all()


def _rect_csr(n, n_cols, seed):
    """n x n_cols CSR: duplicate column ids, empty rows, signed weights [nnz, K] with exact 0.0 and -0.0 entries."""
    rng = np.random.default_rng(seed)
    rowptr, col = [0], []
    for r in range(n):
        d = 0 if r % 8 == 7 else int(rng.integers(1, 9))
        c = rng.integers(0, n_cols, d)
        if d >= 2:
            c[1] = c[0]
        col += list(c)
        rowptr.append(len(col))
    return np.array(rowptr), np.array(col)


def _weights(nnz, K, seed):
    w = np.random.default_rng(seed).uniform(-1, 1, (nnz, K))
    w[3::11] = 0.0
    w[5::13] = -0.0
    return w


def _torch_product(rows, cols, w, x, n, K, post=None, self_add=None, b=None, b_scale=0.0):
    """y = post * (A(w) x) + self + b_scale B by index_add on [nnz, K, D / K] (duplicates are further terms)."""
    D = x.shape[1]
    msg = w[:, :, None] * x.view(-1, K, D // K)[cols]
    y = torch.zeros(n, K, D // K, dtype=torch.float64).index_add(0, rows, msg)
    if post is not None:
        y = post[:, :, None] * y
    y = y.reshape(n, D)
    if self_add is not None:
        y = y + self_add
    if b is not None:
        y = y + b_scale * b
    return y


def test_routed_product_transpose_and_score_are_autograd_of_each_other():
    n, nc, D, K = 48, 37, 16, 4
    rowptr, col = _rect_csr(n, nc, 1)
    w = _weights(len(col), K, 2)
    rows, cols = torch.from_numpy(RR._rows_of(rowptr)), torch.from_numpy(col)
    x = R.randn(nc, D, seed=3).double().requires_grad_()
    wt = _t(w).requires_grad_()
    post, self_add, b = R.randn(n, K, seed=4).double(), R.randn(n, D, seed=5).double(), R.randn(n, D, seed=6).double()
    gy = R.randn(n, D, seed=7).double()

    y = _torch_product(rows, cols, wt, x, n, K, post, self_add, b, 0.25)
    ref, mag = RR.routed_product(rowptr, col, w, x, post=post, self_add=self_add, b=b, b_scale=0.25)
    _close(ref, y, atol=1e-15)
    _covers(ref, mag)
    assert RR.epilogue_count(post, self_add, b) == 3 and RR.epilogue_count() == 0

    # plain product: d / dx is the transposed routed product, d / dw the score pass (the identity _ValuedSpMM relies on)
    y0 = _torch_product(rows, cols, wt, x, n, K)
    ref0, mag0 = RR.routed_product(rowptr, col, w, x)
    _close(ref0, y0, atol=1e-15)
    _covers(ref0, mag0)
    assert (np.diff(rowptr) == 0).any() and (ref0[np.diff(rowptr) == 0] == 0).all()
    y0.backward(gy)
    tref, tmag, (rp, c) = RR.transposed_product(rowptr, col, w, gy, nc)
    _close(tref, x.grad, atol=1e-15)
    _covers(tref, tmag)
    assert len(rp) == nc + 1 and len(c) == len(col)                       # duplicates kept as separate entries
    sref, smag = RR.score(rowptr, col, gy, x.detach(), K, block=64)
    _close(sref, wt.grad, atol=1e-15)
    _covers(sref, smag)
    prior = R.randn(len(col), K, seed=8)
    aref, amag = RR.score(rowptr, col, gy, x.detach(), K, prior=prior)
    _close(aref, wt.grad + prior.double(), atol=1e-15)
    assert (amag >= smag).all() and (amag >= np.abs(aref)).all()

    # the permutation: entry j of the transpose is entry perm[j] here
    perm = RR.host_perm(rowptr, col)
    rp2, c2, v2 = R.transpose_csr(rowptr, col, w, nc)
    assert np.array_equal(v2, RR.permute(w, perm)[0]) and np.array_equal(c2, RR._rows_of(rowptr)[perm])
    _covers(*RR.permute(w, perm))
    # the lane-tree depth of a product row: short rows ceil(deg / NPI) + log2 NPI, long rows 512 / NPI + ceil(chunks / NPI) + 2 log2 NPI
    assert RR.tree_count([0, 1, 1024, 1025, 2049, 97 * 512 + 1], 16)[:, 0].tolist() == [4, 5, 68, 41, 41, 47]
    assert RR.tree_count([0, 1, 1024, 1025, 2049, 97 * 512 + 1], 256)[:, 0].tolist() == [0, 1, 1024, 515, 517, 610]


def test_slice_normalise_of_a_product_is_f_normalize():
    n, D, K = 64, 16, 4
    rowptr, col, _ = _small_csr(n, 3)
    w = _weights(len(col), K, 4)
    x, _, _ = R.norm_rows(n, D, seed=5)
    y, m = RR.routed_product(rowptr, col, w, x)
    (yn, ynm), (inv, invm), clamped = RR.slice_normalise(y, m, K)
    yt = _t(y).view(n, K, D // K)
    _close(yn, F.normalize(yt, dim=2).reshape(n, D))
    _close(inv, 1.0 / yt.norm(dim=2).clamp_min(1e-12))
    _covers(yn, ynm)
    _covers(inv, invm)
    nrm = yt.norm(dim=2).numpy()
    assert np.array_equal(clamped, nrm < 1e-12) and (nrm == 0).any() and ((nrm > 0) & clamped).any() and not clamped.all()
    assert (inv[clamped] == 1e12).all()


def test_slice_ops_are_autograd_of_f_normalize():
    n, D, K = 40, 32, 4
    xs, dzs, clamped = R.norm_rows(n * K, D // K, seed=9)                  # zero and 1e-13 SLICES, zero and -0.0 dz slices
    x, dz = xs.reshape(n, D), dzs.reshape(n, D)
    xr = x.double().requires_grad_()
    z = F.normalize(xr.view(n, K, D // K), dim=2).reshape(n, D)
    (y, ym, slope), (inv, invm) = RR.slice_norm_fwd(x, K)
    _close(y, z)
    _close(inv, 1.0 / xr.detach().view(n, K, -1).norm(dim=2).clamp_min(1e-12))
    assert (slope == 0).all() and (ym >= np.abs(y)).all() and (invm >= inv).all()
    (t, tm, slope), _ = RR.slice_norm_fwd(x, K, tanh=True)
    _close(t, torch.tanh(z))
    zz = z.detach().clone().requires_grad_()
    torch.tanh(zz).sum().backward()
    _close(slope, zz.grad * z.detach().abs(), atol=1e-300)
    _covers(t, tm)
    z.backward(dz.double())
    inv32 = inv.astype(np.float32)                                          # what a forward pass stores: 1e12 exactly when clamped
    assert (inv32.reshape(-1)[clamped] == R.INV_CLAMPED).all() and clamped.any() and not clamped.all()
    ref, mag = RR.slice_norm_bwd(x, inv, dz, K)
    _close(ref, xr.grad)
    _covers(ref, mag)
    ref32, _ = RR.slice_norm_bwd(x, inv32, dz, K)                           # the clamp is recognised on the stored float too
    cl = np.repeat(clamped.reshape(n, K), D // K, axis=1)
    np.testing.assert_allclose(ref32[cl], xr.grad.numpy()[cl], rtol=1e-8)    # float32(1e12) is 4e-9 off 1e12
    p = R.randn(n, K, seed=11)
    sref, smag = RR.slice_scale(x, p)
    _close(sref, (x.double().view(n, K, -1) * p.double()[:, :, None]).reshape(n, D))
    _covers(sref, smag)


def test_softmaxes_are_torch_softmax_and_its_autograd():
    n = 64
    rowptr, col, _ = _small_csr(n, 6)
    nnz, rows = len(col), torch.from_numpy(RR._rows_of(rowptr))
    rng = np.random.default_rng(7)
    for K in (1, 2, 4, 8):
        logits = rng.uniform(-80, 80, (nnz, K))
        logits[0] = -80.0
        logits[0, K - 1] = 80.0
        w, mag, extra = RR.route_softmax(logits)
        _close(w, torch.softmax(_t(logits), 1))
        assert (mag >= w).all() and (extra >= 0).all() and (extra <= 2 * 160 * R.U32 * w + 1e-300).all()
        assert w[0, K - 1] == 1.0 and (K == 1 or w[0, 0] < 1e-60)
    l = _t(rng.uniform(-80, 80, nnz)).requires_grad_()
    a = torch.cat([torch.softmax(l[rowptr[r]:rowptr[r + 1]], 0) for r in range(n)])
    ref, mag, extra = RR.row_softmax(rowptr, l.detach().numpy())
    _close(ref, a)
    assert (mag >= ref).all() and (extra >= 0).all()
    da = _t(rng.standard_normal(nnz))
    a.backward(da)
    bref, bmag = RR.row_softmax_bwd(rowptr, a.detach().numpy(), da.numpy())
    _close(bref, l.grad, atol=1e-18)
    _covers(bref, bmag)
    fwd_c, bwd_c = RR.row_softmax_count(np.diff(rowptr))
    assert fwd_c.shape == (nnz,) and (fwd_c == 7 + 17).all() and (bwd_c == 7 + 2).all()
    assert RR.rowsum_count([0, 64, 65, 1024, 1025, 2049])[:, 0].tolist() == [5.0, 5.5, 6.0, 13.0, 10.5, 11.5]


def test_references_are_the_oracles_dgcf_routing_step():
    """One routing iteration of DGCF as the oracle states it (softmax over factors, D^-1/2 A_k D^-1/2, the edge score of the
    normalised result against tanh of the normalised input), per factor, against the references chained as the model chains
    the kernels: route_softmax, rowsum_rsqrt, slice_scale, the product with `post`, slice_norm_fwd (plain / tanh), score."""
    n, D, K = 64, 16, 4
    rowptr, col, _ = _small_csr(n, 8)                                       # has empty rows: d = 0 there
    rows, cols = torch.from_numpy(RR._rows_of(rowptr)), torch.from_numpy(col)
    a_values = _t(np.random.default_rng(9).standard_normal((K, len(col))))
    ego = R.randn(n, D, seed=10).double()
    a_factor = torch.softmax(a_values, dim=0)
    w, _, _ = RR.route_softmax(a_values.T.numpy())
    _close(w, a_factor.T)
    d, dmag = RR.rowsum_rsqrt(rowptr, w)
    assert (d[np.diff(rowptr) == 0] == 0).all() and (dmag >= d).all()
    f, _ = RR.routed_product(rowptr, col, w, RR.slice_scale(ego, d)[0], post=d)
    (h, _, _), _ = RR.slice_norm_fwd(f, K)
    (t, _, _), _ = RR.slice_norm_fwd(ego, K, tanh=True)
    sc, _ = RR.score(rowptr, col, h, t, K)
    for k, split in enumerate(torch.split(ego, D // K, dim=1)):
        _, fk, sk = om.dgcf_factor_update(rows, cols, a_factor[k], split, n)
        _close(d[:, k], om._diag_inv_sqrt_rowsum(rows, a_factor[k], n))
        _close(f[:, k * (D // K):(k + 1) * (D // K)], fk, atol=1e-16)
        _close(sc[:, k], sk, atol=1e-15)
    wz = np.zeros((len(col), 2))
    wz[:, 1] = 1.0
    assert (RR.rowsum_rsqrt(rowptr, wz)[0][:, 0] == 0).all()                  # weights all exactly 0: inf -> 0
