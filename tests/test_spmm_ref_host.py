"""CPU-only: the fp64 references of tests/spmm_ref.py against torch autograd in fp64 -- what makes them independent of the
kernels they judge in test_gpu_spmm.py."""
import numpy as np
import torch

import spmm_ref as R


def _small_csr(n, seed):
    """Square CSR taken as given: signed values, duplicate column ids inside a row, empty rows; rows 2 mod 8 gather only
    operand rows 1 mod 8 (all-zero: an exactly-zero product row), rows 4 mod 8 only operand rows 3 mod 8 (norm 1e-13: a
    clamped, non-zero product row)."""
    rng = np.random.default_rng(seed)
    rowptr, col = [0], []
    for r in range(n):
        d = 0 if r % 8 == 7 else int(rng.integers(1, 9))
        if r % 8 == 2:
            c = rng.choice(np.arange(1, n, 8), d)
        elif r % 8 == 4:
            c = rng.choice(np.arange(3, n, 8), d)
        else:
            c = rng.integers(0, n, d)
        if d >= 2:
            c[1] = c[0]                                            # a duplicate column id
        col += list(c)
        rowptr.append(len(col))
    val = rng.uniform(-1, 1, len(col))
    return np.array(rowptr), np.array(col), val


def _dense(rowptr, col, val, n):
    A = torch.zeros(n, n, dtype=torch.float64)
    rows = np.repeat(np.arange(n), np.diff(rowptr))
    A.index_put_((torch.from_numpy(rows), torch.from_numpy(col)), torch.from_numpy(val), accumulate=True)
    return A


def test_product_takes_duplicates_and_empty_rows():
    n, D = 64, 12
    rowptr, col, val = _small_csr(n, 1)
    X = R.randn(n, D, seed=2).double()
    ref, mag, deg = R.product(rowptr, col, val, X)
    np.testing.assert_allclose(ref, (_dense(rowptr, col, val, n) @ X).numpy(), rtol=1e-12, atol=1e-15)
    np.testing.assert_allclose(mag, (_dense(rowptr, col, np.abs(val), n) @ X.abs()).numpy(), rtol=1e-12, atol=1e-15)
    assert np.array_equal(deg, np.diff(rowptr)) and (deg == 0).any() and (ref[deg == 0] == 0).all()
    rp, c, v = R.transpose_csr(rowptr, col, val, n)
    np.testing.assert_allclose(R.product(rp, c, v, X)[0], (_dense(rowptr, col, val, n).T @ X).numpy(), rtol=1e-12, atol=1e-15)


def test_references_are_torch_autograd_in_fp64():
    """LightGCN's chain (x_{k+1} = A x_k, acc = s sum_k normalize(x_k)) under a loss linear in acc: d loss / d x_0 is the
    NORMBWD reference over A^T, fed by the plain normalize-backward at the top and closed by AXPY at the bottom."""
    n, D, s = 64, 12, 1.0 / 3.0
    rowptr, col, val = _small_csr(n, 3)
    A = _dense(rowptr, col, val, n)
    x0, _, _ = R.norm_rows(n, D, seed=5)
    acc0, W = R.randn(n, D, seed=7).double(), R.randn(n, D, seed=8).double()
    xr = x0.double().requires_grad_()
    x1 = A @ xr
    x2 = A @ x1
    acc = acc0 + s * xr + s * torch.nn.functional.normalize(x1, dim=1) + s * torch.nn.functional.normalize(x2, dim=1)
    (acc * W).sum().backward()

    # forward through the references: the accumulator, the inverse norms and the clamped rows
    y1, m1, _ = R.product(rowptr, col, val, x0)
    _, (inv1, _), (a1, _), cl1 = R.epi_norm_acc(y1, m1, acc0 + s * x0.double(), s)
    y2, m2, _ = R.product(rowptr, col, val, y1)
    _, (inv2, _), (a2, _), cl2 = R.epi_norm_acc(y2, m2, a1, s)
    np.testing.assert_allclose(a2, acc.detach().numpy(), rtol=1e-12, atol=0)
    assert cl1.any() and (y1 == 0).all(1).any() and ((np.linalg.norm(y1, axis=1) > 0) & cl1).any()

    rp, c, v = R.transpose_csr(rowptr, col, val, n)
    g2 = R.ref_norm_bwd(y2, inv2, W, s, cl2)[0]
    g1 = R.epi_normbwd(*R.product(rp, c, v, g2)[:2], y1, inv1, W, s, cl1)[0]
    g0 = R.epi_axpy(*R.product(rp, c, v, g1)[:2], W, s)[0]
    np.testing.assert_allclose(g0, xr.grad.numpy(), rtol=1e-12, atol=0)


def test_ss_and_normbwd_dot_over_two_column_shards_compose_to_normbwd():
    n, D, s, h = 64, 12, 1.0 / 3.0, 7
    rowptr, col, val = _small_csr(n, 4)
    x0, dz, _ = R.norm_rows(n, D, seed=9)
    g = R.randn(n, D, seed=11).double().numpy()
    y, m, _ = R.product(rowptr, col, val, x0)
    shards = [(0, h), (h, D)]
    ss = sum(R.epi_ss(y[:, a:b], m[:, a:b])[0] for a, b in shards)
    inv = 1.0 / np.maximum(np.sqrt(ss), R.EPS)
    inv_full, clamped = R.inv_norm(y)
    np.testing.assert_allclose(inv, inv_full, rtol=1e-12, atol=0)
    # a clamped row carries exactly the constant the kernels test for
    inv[clamped] = float(R.INV_CLAMPED)
    inv_full[clamped] = float(R.INV_CLAMPED)
    dot = sum(R.row_dot(y[:, a:b], inv, dz[:, a:b], s) for a, b in shards)
    rp, c, v = R.transpose_csr(rowptr, col, val, n)
    pg, pm, _ = R.product(rp, c, v, g)
    parts = [R.epi_normbwd_dot(pg[:, a:b], pm[:, a:b], y[:, a:b], inv, dz[:, a:b], dot, s)[0] for a, b in shards]
    whole = R.epi_normbwd(pg, pm, y, inv_full, dz, s, clamped)[0]
    np.testing.assert_allclose(np.concatenate(parts, 1), whole, rtol=1e-12, atol=1e-18)
    assert clamped.any() and not clamped.all()


def test_masks_and_marks():
    # drop_keep is drop4's pattern on a [n, D] table; edge_kept swaps its arguments under `transposed`
    kept, scale = R.drop_keep(50, 16, 0.5, 3)
    assert kept.shape == (50, 16) and 0.4 < kept.mean() < 0.6 and scale == 2.0
    x = np.ones((50 * 4, 4), np.float32)
    assert np.array_equal(R.np_drop(x, np.arange(200), 0.5, 3).reshape(50, 16) != 0, kept)
    r, c = np.arange(100), np.arange(100)[::-1].copy()
    assert np.array_equal(R.edge_kept(r, c, 0.3, 5, transposed=True), R.edge_kept(c, r, 0.3, 5))
    assert R.edge_kept(r, c, 0.0, 5).all()
    rowptr, col = np.array([0, 2, 2, 3]), np.array([2, 2, 0])
    assert R.mark_rows(rowptr, col, [0, 1], np.zeros(3, np.uint8)).tolist() == [1, 1, 1]
    assert R.mark_rows(rowptr, col, [0, 1], np.full(3, 7, np.uint8), self_too=False).tolist() == [7, 7, 1]
    assert R.row_flags(np.array([[0.0, -0.0], [0.0, 1e-30]])).tolist() == [0, 1]
