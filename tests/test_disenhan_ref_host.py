"""CPU-only: the fp64 references of tests/disenhan_ref.py against fp64 torch autograd of tests/disenhan_torch.py (the
restatement test_disenhan_host.py holds to the reference's fixtures) -- what makes them independent of the kernels they judge in
test_gpu_disenhan_kernels.py -- on the hand-placed inputs that test uses, and the assertions that those inputs hold the edges
they are meant to hold."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

import disenhan_ref as RD
import disenhan_torch as DT
import spmm_ref as R
from spmm_ref import f64

RTOL = 1e-12


def _t(a, grad=False):
    t = torch.from_numpy(np.ascontiguousarray(f64(a)))
    return t.requires_grad_() if grad else t


def _close(what, pair, want):
    """|ref - autograd| <= 1e-12 mag: relative to the sum of the absolute terms, which a cancelling sum is not held below"""
    ref, mag = pair[0], pair[1]
    want = want.detach().numpy() if isinstance(want, torch.Tensor) else want
    assert ref.shape == want.shape, what
    assert (np.asarray(mag) >= np.abs(ref) * (1 - 1e-12)).all(), f"{what}: mag below |ref|"
    bad = np.abs(ref - want) > RTOL * np.asarray(mag) + 1e-300
    assert not bad.any(), f"{what}: {int(bad.sum())} elements off, worst {np.abs(ref - want).max():.3e}"


# ==================================================================================================== the relation
def test_relation_holds_the_placed_degrees():
    rel = RD.relation()
    assert (rel.n_rows, rel.n_cols) == (303, 201) and rel.n_rows % 4 and rel.n_cols % 4
    for table in (RD.ROW_DEG, RD.CLOSED_ROWS):
        for i, d in table.items():
            assert rel.deg[i] == d, (i, d)
    assert {0, 1, 2, 63, 64, 65, 128, 129, 190} <= set(rel.deg.tolist())
    assert rel.deg[rel.n_rows - 1] == 190 and (rel.n_rows - 1) % 4 == 2          # the long row in the block of three
    cd = rel.cdeg
    assert cd[RD.COL_63] == 63 and cd[RD.COL_64] == 64 and cd[RD.COL_65] == 65 and cd[RD.COL_1] == 1
    assert cd[RD.COL_HUB] > 128 and all(cd[c] == 0 for c in RD.COL_EMPTY) and RD.COL_EMPTY[1] == rel.n_cols - 1
    assert set(np.unique(rel.mult).tolist()) == {1.0, 2.0, 3.0, 4.0}
    # CSR: ascending unique columns inside a row; the transposed structure and the permutation agree
    for i in range(rel.n_rows):
        c = rel.col[rel.rowptr[i]:rel.rowptr[i + 1]]
        assert (np.diff(c) > 0).all()
    assert np.array_equal(rel.col_t, rel.rows_of[rel.perm]) and np.array_equal(np.sort(rel.perm), np.arange(rel.nnz))
    # the block of exact zeros: row 30 holds nothing else, column 10 nothing else
    z0, c0 = RD.ZERO_ROWS[0], RD.ZERO_COLS[0]
    assert rel.col[rel.rowptr[z0]:rel.rowptr[z0 + 1]].tolist() == list(RD.ZERO_COLS)
    assert rel.col_t[rel.rowptr_t[c0]:rel.rowptr_t[c0 + 1]].tolist() == list(RD.ZERO_ROWS)
    assert RD.tree([0, 1, 64, 65, 128, 129, 190]).tolist() == [6, 7, 7, 8, 8, 9, 9]


@pytest.mark.parametrize("case", ["plain", "big"])
@pytest.mark.parametrize("K", [1, 2, 4, 8])
def test_edge_softmax_is_autograd_of_the_restatement(K, case):
    rel = RD.relation()
    sL, sR, r, dalpha = RD.edge_inputs(K, case)
    rows, cols = torch.from_numpy(rel.rows_of), torch.from_numpy(rel.col.astype(np.int64))
    # the inputs hold the edges: exact zeros of sL + sR, closed rows, and in `big` logits beyond +-80
    pre = f64(sL)[rel.rows_of] + f64(sR)[rel.col]
    block = np.isin(rel.rows_of, RD.ZERO_ROWS) & np.isin(rel.col, RD.ZERO_COLS)
    assert block.sum() == 36 and (pre[block, 0] == 0.0).all()
    assert (sL.numpy()[rel.rows_of[block], 0] + sR.numpy()[rel.col[block], 0] == 0.0).all()     # in float32 too
    closed = np.isin(rel.rows_of, list(RD.CLOSED_ROWS))
    assert closed.sum() == 203 and (pre[closed] < 0).all()
    (a, amag, extra), (logit, lmag) = RD.edge_softmax_fwd(rel.rowptr, rel.col, rel.mult, sL, sR, r)
    assert (logit[closed] == 0).all() and (extra >= 0).all() and (lmag >= np.abs(logit)).all()
    for i, d in RD.CLOSED_ROWS.items():
        assert (a[rel.rowptr[i]:rel.rowptr[i + 1]] == 1.0 / d).all()
    if case == "big":
        assert logit.min() < -80 and logit.max() > 80
    else:
        assert logit.min() == 0 and 1 < logit.max() < 80
    tin = [_t(x, True) for x in (sL, sR, r)]
    alpha = DT.edge_softmax(*tin, rows, cols, _t(rel.mult), rel.n_rows)
    _close("alpha", (a, amag), alpha)
    (alpha * _t(dalpha)).sum().backward()
    (g, gmag), dr, dsL, dsR = RD.edge_softmax_bwd(rel.rowptr, rel.col, rel.mult, rel.n_cols, sL, sR, r, a, dalpha)
    assert (gmag >= np.abs(g)).all()
    _close("dsL", dsL, tin[0].grad)
    _close("dsR", dsR, tin[1].grad)
    _close("dr", dr, tin[2].grad)
    # empty rows / columns: exact zeros; the exact-zero gates contribute nothing (row 30 and column 10 see no other in k = 0)
    assert (dr[0][rel.deg == 0] == 0).all() and (dsL[0][rel.deg == 0] == 0).all() and (dsR[0][rel.cdeg == 0] == 0).all()
    assert dsL[0][RD.ZERO_ROWS[0], 0] == 0 and dr[0][RD.ZERO_ROWS[0], 0] == 0 and dsR[0][RD.ZERO_COLS[0], 0] == 0
    assert (dsL[0][list(RD.CLOSED_ROWS)] == 0).all() and (dr[0][list(RD.CLOSED_ROWS)] == 0).all()
    assert np.abs(g[block]).min() > 0 or K == 1 or case == "big"             # they would contribute under a `>=` gate
    # given the float32 g a kernel stores, the sums follow that g
    g32 = g.astype(np.float32)
    _, dr2, dsL2, dsR2 = RD.edge_softmax_bwd(rel.rowptr, rel.col, rel.mult, rel.n_cols, sL, sR, r, a, dalpha, g=g32)
    np.testing.assert_allclose(dsR2[0], dsR[0], rtol=0, atol=1e-6 * max(1.0, np.abs(dsR[0]).max()))
    np.testing.assert_allclose(dsL2[0], dsL[0], rtol=0, atol=1e-6 * max(1.0, np.abs(dsL[0]).max()))


# ================================================================================================ relation epilogue
def _epi_cases():
    """(n, D, K, case) of the GPU test that the host test walks: every shape at its largest small size, two saturated cases"""
    out = [(RD.row_sizes(D)[2], D, K, "plain") for D, K in RD.SHAPES]
    return out + [(19, 64, 4, "sat"), (79, 16, 8, "sat")]


@pytest.mark.parametrize("n,D,K,case", _epi_cases())
def test_rel_epilogue_is_autograd_of_the_restatement(n, D, K, case):
    Y, W, q, dZ, dr = RD.epilogue_inputs(n, D, K, seed=D + K + n, case=case)
    yh = Y.numpy()
    assert (yh == 0).any() and np.signbit(yh[yh == 0]).any() and (~np.signbit(yh[yh == 0])).any() and (yh < 0).any()
    (yl, ylmag), (z, zmag), (r, rmag, rextra) = RD.rel_epi_fwd(Y, W, q, K)
    tin = [_t(x, True) for x in (Y, W, q)]
    Z_t, r_t = DT.rel_epilogue(*tin, K)
    _close("Yl", (yl, ylmag), F.leaky_relu(_t(Y), 0.2))
    _close("Z", (z, zmag), Z_t)
    _close("r", (r, rmag), r_t)
    assert (rextra >= 0).all() and np.isfinite(rextra).all()
    zero_rows = (yh == 0).all(1)
    if n >= 2:
        assert zero_rows.any() and (z[zero_rows] == 0).all() and (r[zero_rows] == 1.0 / K).all()
    if case == "sat":
        assert (np.abs(np.tanh(z).astype(np.float32)) == 1.0).mean() > 0.2    # a good share of tanh(Z) is +-1 as a float
    else:
        assert np.abs(z).max() < 9.0
    dzh = dZ.numpy().reshape(n * K, -1)
    if n * K >= 8:
        assert (dzh == 0).all(1).any() and np.signbit(dzh).any()
    # the four forms of the backward: dZ only, dr only, both, neither
    for name, gz, gr in (("dZ", dZ, None), ("dr", None, dr), ("both", dZ, dr), ("neither", None, None)):
        dY, dZt, dsT, dW, dq = RD.rel_epi_bwd(yl, z, r, gz, gr, W, q, K)
        if name == "neither":
            assert all((p[0] == 0).all() and (p[1] == 0).all() for p in (dY, dZt, dsT, dW, dq))
            continue
        for x in tin:
            x.grad = None
        Z_t, r_t = DT.rel_epilogue(*tin, K)
        loss = (Z_t * _t(gz)).sum() if gz is not None else 0.0
        loss = loss + ((r_t * _t(gr)).sum() if gr is not None else 0.0)
        loss.backward()
        _close(f"{name}: dY", dY, tin[0].grad)
        _close(f"{name}: dW", dW, tin[1].grad)
        _close(f"{name}: dq", dq, tin[2].grad if tin[2].grad is not None else torch.zeros(D // K, dtype=torch.float64))
        if gr is None:
            assert np.array_equal(dZt[0], f64(gz)) and (dsT[0] == 0).all()     # dr NULL: dZt is dZ
        # given the float32 dZt a kernel stores, dY and dW follow it
        dY2, _, _, dW2, _ = RD.rel_epi_bwd(yl, z, r, gz, gr, W, q, K, dZt=dZt[0].astype(np.float32))
        np.testing.assert_allclose(dY2[0], dY[0], rtol=0, atol=1e-5 * max(1.0, np.abs(dY[0]).max()))
        np.testing.assert_allclose(dW2[0], dW[0], rtol=0, atol=1e-5 * max(1.0, np.abs(dW[0]).max()))


# ========================================================================================================== combine
def _combine_cases():
    return [(RD.row_sizes(D)[2], D, K) for D, K in RD.SHAPES] + [(1, 256, 1), (2, 256, 2)]


@pytest.mark.parametrize("n,D,K", _combine_cases())
def test_combine_is_autograd_of_f_normalize(n, D, K):
    dk = D // K
    ego, Z1, r1, Z2, r2, dy = RD.combine_inputs(n, D, K, seed=D + K + n)
    (x, xmag), (y, ymag), (inv, invmag), clamped = RD.combine_fwd(ego, Z1, r1, Z2, r2, K)
    # the inputs hold the edges: zero slices, slices of norm ~1e-13, none within a factor of 10 of the clamp
    nrm = np.linalg.norm(x.reshape(n * K, dk), axis=1).reshape(n, K)
    # (the tiny slices sit AT the factor: 1e-13 up to the rounding of the float32 scaling that makes them)
    assert ((nrm == 0) | ((nrm > 0.999e-13) & (nrm < 1.001e-13)) | (nrm > 1e-3)).all()
    assert not ((nrm > 1.001e-13) & (nrm < 1e-11)).any()
    assert np.array_equal(clamped, nrm < 1e-12)
    if n * K >= 8:
        assert (nrm == 0).any() and ((nrm > 0) & clamped).any() and not clamped.all()
        dyh = dy.numpy().reshape(n * K, dk)
        assert (dyh == 0).all(1).any() and np.signbit(dyh[(dyh == 0).all(1)]).any()
    assert (inv[clamped] == 1e12).all() and (inv.astype(np.float32)[clamped] == R.INV_CLAMPED).all()
    assert (y[np.repeat(nrm == 0, dk, axis=1)] == 0).all()
    tin = [_t(t, True) for t in (ego, Z1, r1, Z2, r2)]
    y_t = DT.combine(tin[0], [(tin[1], tin[2]), (tin[3], tin[4])], K)
    _close("y", (y, ymag), y_t)
    xt = _t(x).view(n, K, dk)
    _close("inv", (inv, invmag), 1.0 / xt.norm(dim=2).clamp_min(1e-12))
    y_t.backward(_t(dy))
    # the clamped-slice convention: F.normalize's gradient on a clamped slice is dy / eps -- the dot is dropped
    for inv_given in (inv, inv.astype(np.float32)):                          # the stored float 1e12 is recognised too
        dx, dZ1, dZ2, dr1, dr2 = RD.combine_bwd(x, inv_given, dy, Z1, r1, Z2, r2, K)
        if inv_given.dtype == np.float32:
            cl = np.repeat(clamped, dk, axis=1)
            np.testing.assert_allclose(dx[0][cl], tin[0].grad.numpy()[cl], rtol=1e-8)       # float32(1e12) is 4e-9 off 1e12
            continue
        _close("dx", dx, tin[0].grad)
        _close("dZ1", dZ1, tin[1].grad)
        _close("dr1", dr1, tin[2].grad)
        _close("dZ2", dZ2, tin[3].grad)
        _close("dr2", dr2, tin[4].grad)
        cl = np.repeat(clamped, dk, axis=1)
        assert np.array_equal(dx[0][cl], (f64(dy) * 1e12)[cl])
    # given the float32 x / dx a kernel stores, what follows is formed from them
    (_, _), (y2, _), (inv2, _), cl2 = RD.combine_fwd(ego, Z1, r1, Z2, r2, K, x=x.astype(np.float32))
    assert np.array_equal(cl2, clamped)
    np.testing.assert_allclose(y2, y, rtol=0, atol=1e-5)


def test_second_trip_sizes_pass_the_grid_cap():
    for D in (16, 64, 256):
        rb = 256 // D
        n = RD.second_trip_n(D)
        groups = -(-n // rb)
        assert n > RD.MAX_GROUPS * rb and groups == RD.MAX_GROUPS + 2 and n - (groups - 1) * rb == 1
    assert RD.second_trip_n(256) == 4098 and RD.second_trip_n(16) == 65553
    assert len(RD.SHAPES) == 20
