"""CPU: the fp64 restatements of tests/tgcn_attn_ref.py (what test_gpu_tgcn_attn_kernels.py holds the HIP kernels to) against
torch autograd in fp64 on the operator form (gather, relu, softmax, weighted sum), against the oracle's `Attention1` split the
way test_gpu_tgcn.py::test_attention_kernels_vs_oracle splits it, the pull form (da -> ds / bits -> dQ) against the direct form,
the integer restatements against torch.sort(stable=True) / searchsorted, and the inputs the GPU tests draw: on the 2^-8 grid the
fp32 pre-activation equals the fp64 one for every (v, n, c), so the kernels' [h > 0] is the reference's.

`close`: |got - ref| <= 1e-12 * (sum of the absolute values of the terms), the rtol = 1e-12 of a sum."""
import numpy as np
import pytest
import torch

import tgcn_attn_ref as AR
from oracle import models as om
from spmm_ref import f64

RTOL = 1e-12
CASES = [(70, 40, 1, 16, 4, 1), (70, 23, 3, 32, 8, 7), (90, 31, 9, 256, 64, 7), (1117, 50, 25, 64, 32, 5), (75, 12, 64, 16, 16, 3)]


def close(what, got, ref, mag):
    got, ref = f64(got), f64(ref)
    assert got.shape == ref.shape, what
    err = np.abs(got - ref)
    assert (err <= RTOL * f64(mag) + 1e-300).all(), f"{what}: {err.max():.3e}"


def _case(n, n_dst, k, D, A, n_wt, **kw):
    return AR.make_case(n, n_dst, k, D, A, n_wt, seed=n + k + A, long=n >= AR.N_LONG, **kw)


def _autograd(c, dOut):
    """operator form in fp64 -> attn, out, grads of P, Q, WT, v, Ej"""
    t = {kk: torch.from_numpy(c[kk]).double().requires_grad_() for kk in ("P", "Q", "WT", "v", "Ej")}
    idx, widx = torch.from_numpy(c["idx"]).long(), torch.from_numpy(c["widx"]).long()
    Qp = torch.cat([t["Q"].new_zeros(1, c["A"]), t["Q"]])
    Ep = torch.cat([t["Ej"].new_zeros(1, c["D"]), t["Ej"]])
    h = t["P"][:, None, :] + t["WT"][widx] + Qp[idx]
    a = torch.softmax(torch.relu(h) @ t["v"], dim=1)
    out = (a[:, :, None] * Ep[idx]).sum(1)
    (out * torch.from_numpy(dOut).double()).sum().backward()
    return a.detach().numpy(), out.detach().numpy(), {kk: x.grad.numpy() for kk, x in t.items()}


@pytest.mark.parametrize("shape", CASES, ids=str)
@pytest.mark.parametrize("spread", [False, True])
def test_restatements_vs_autograd_fp64(shape, spread):
    c = _case(*shape, spread=spread)
    a, out, g = _autograd(c, c["dOut"])
    f = AR.attn_fwd(c["P"], c["Q"], c["WT"], c["v"], c["Ej"], c["idx"], c["widx"])
    close("attn", f["attn"][0], a, np.ones_like(a))
    close("out", f["out"][0], out, f["out"][1])
    b = AR.attn_bwd(c["P"], c["Q"], c["WT"], c["v"], c["Ej"], c["idx"], c["widx"], f["attn"][0], c["dOut"])
    for name, key in (("dP", "P"), ("dQ", "Q"), ("dWT", "WT"), ("dv", "v"), ("dEj", "Ej")):
        close(name, b[name][0], g[key], b[name][1])
    # the planted cases are there: exact zeros of h (gradient 0 there), pads, an all-pad row, ties
    assert (f["h"][8, 0] == 0).all() and (b["dh"][0][8, 0] == 0).all() and (f["h"] == 0).sum() >= c["A"] + 10
    assert (out[3] == 0).all() and (c["idx"][3] == 0).all() and (b["da"][0][c["idx"] == 0] == 0).all()
    assert np.ptp(f["s"][0][5]) == 0 and AR.multiplicity(c["idx"], c["n_dst"])[-1] == 0
    assert (b["dQ"][0][-1] == 0).all() and (b["dEj"][0][-1] == 0).all()
    if spread:
        assert np.abs(f["s"][0]).max() > 60 and (a.astype(np.float32) == 1).any()
        assert c["k"] < 9 or (a.astype(np.float32) == 0).any()        # (few slots: no logit 104 below the maximum)


@pytest.mark.parametrize("shape", CASES[:4], ids=str)
def test_restatements_vs_oracle_attention1(shape):
    """`Attention1` of the oracle, P = ev W1[:D] + b, Q = ej W2, WT = cat(0, ew) W1[D:]: every gradient of the model's tensors
    from the restatement's dP, dQ, dWT, dv, dEj by the chain rule of the three GEMMs."""
    n, n_dst, k, D, A, n_wt = shape
    c = _case(*shape)
    gen = torch.Generator().manual_seed(k)
    dw = 10
    rnd = lambda *s: torch.randn(*s, generator=gen, dtype=torch.float64) * 0.3
    ev, ej, ew = rnd(n, D), rnd(n_dst, D), rnd(n_wt - 1, dw)                 # (n_wt = 1: the pad row alone)
    prm = {"W_1": rnd(D + dw, A), "W_2": rnd(D, A), "b": rnd(1, A), "v": rnd(1, A)}
    leaves = {kk: x.clone().requires_grad_() for kk, x in {**prm, "ev": ev, "ej": ej, "ew": ew}.items()}
    idx, widx = torch.from_numpy(c["idx"]).long(), torch.from_numpy(c["widx"]).long()
    up = torch.from_numpy(c["dOut"]).double()
    want = om.tgcn_attention1(leaves, "", leaves["ev"], leaves["ej"], leaves["ew"], idx, widx)
    (want * up).sum().backward()
    ewp = torch.cat([ew.new_zeros(1, dw), ew])
    P, Q, WT, v = ev @ prm["W_1"][:D] + prm["b"], ej @ prm["W_2"], ewp @ prm["W_1"][D:], prm["v"].reshape(-1)
    f = AR.attn_fwd(P, Q, WT, v, ej, c["idx"], c["widx"])
    b = AR.attn_bwd(P, Q, WT, v, ej, c["idx"], c["widx"], f["attn"][0], up)
    dP, dQ, dWT, dEj = (b[kk][0] for kk in ("dP", "dQ", "dWT", "dEj"))
    W1, W2 = prm["W_1"].numpy(), prm["W_2"].numpy()
    got = {"ev": dP @ W1[:D].T, "ej": dEj + dQ @ W2.T, "ew": (dWT @ W1[D:].T)[1:], "W_2": ej.numpy().T @ dQ,
           "W_1": np.concatenate([ev.numpy().T @ dP, ewp.numpy().T @ dWT]), "b": dP.sum(0, keepdims=True), "v": b["dv"][0][None]}
    scale = lambda x: np.abs(x).max(initial=0.0) + 1e-30                     # relative to the tensor (sums with cancellation)
    np.testing.assert_allclose(f["out"][0], want.detach().numpy(), rtol=0, atol=RTOL * scale(f["out"][1]))
    for kk, x in got.items():
        np.testing.assert_allclose(x, leaves[kk].grad.numpy(), rtol=0, atol=RTOL * scale(x), err_msg=kk)


@pytest.mark.parametrize("shape", CASES, ids=str)
def test_pull_form_equals_direct_form(shape):
    n, n_dst, k, D, A, n_wt = shape
    c = _case(*shape)
    rng = np.random.default_rng(1)
    B, BQ = rng.standard_normal((n_dst, D)), rng.standard_normal((n_dst, A))
    a = AR.attn_fwd(c["P"], c["Q"], c["WT"], c["v"], c["Ej"], c["idx"], c["widx"])["attn"][0]
    d = AR.attn_bwd(c["P"], c["Q"], c["WT"], c["v"], c["Ej"], c["idx"], c["widx"], a, c["dOut"])
    (dEj, dEj_mag), (da, _) = AR.attn_pull_da(c["Ej"], c["idx"], a, c["dOut"], B)
    close("dEj + B", dEj, d["dEj"][0] + B, dEj_mag)
    assert (da[c["idx"] == 0] == 0).all()
    poisoned = np.where(c["idx"] > 0, da, np.nan)
    s = AR.attn_bwd_ds(c["P"], c["Q"], c["WT"], c["v"], c["idx"], c["widx"], a, poisoned)
    for kk in ("ds", "dP", "dWT", "dv"):
        close(kk, s[kk][0], d[kk][0], d[kk][1])
    assert np.array_equal(s["bits"], d["bits"]) and np.array_equal(AR.bits_of(s["bits"], A), (d["h"] > 0).astype(np.int64))
    dQ, dQ_mag = AR.attn_dq_from_comp(c["idx"], s["ds"][0], s["bits"], c["v"], n_dst, BQ)
    close("dQ + B", dQ, d["dQ"][0] + BQ, dQ_mag)
    close("dh from comp", s["ds"][0][:, :, None] * AR.bits_of(s["bits"], A) * f64(c["v"]), d["dh"][0], d["dh"][1])


@pytest.mark.parametrize("shape", CASES, ids=str)
def test_integer_restatements_vs_torch_sort(shape):
    n, n_dst, k, D, A, n_wt = shape
    c = _case(*shape)
    idx = torch.from_numpy(c["idx"]).long()
    key = torch.where(idx > 0, idx - 1, torch.full_like(idx, n_dst)).reshape(-1).int()
    assert np.array_equal(AR.attn_keys(c["idx"], n_dst), key.numpy())
    skey_t, order_t = torch.sort(key, stable=True)
    skey, order, rowptr = AR.invert(c["idx"], n_dst)
    assert np.array_equal(skey, skey_t.numpy()) and np.array_equal(order, order_t.numpy())
    assert np.array_equal(rowptr, torch.searchsorted(skey_t, torch.arange(n_dst + 1, dtype=torch.int32)).numpy())
    assert np.array_equal(np.diff(rowptr), AR.multiplicity(c["idx"], n_dst))
    attn = np.random.default_rng(2).random((n, k)).astype(np.float32)
    pair, src, val = AR.attn_invert_fill(order, attn, k)
    total = int(rowptr[-1])
    assert (c["idx"].reshape(-1)[pair[:total]] - 1 == skey[:total]).all() and (c["idx"].reshape(-1)[pair[total:]] == 0).all()
    assert np.array_equal(src, pair // k) and np.array_equal(val, attn.reshape(-1)[pair])
    # a row subset: gathered tables, and the filtered static list = the inversion of the gathered table
    rng = np.random.default_rng(3)
    for rows in (np.sort(rng.permutation(n)[:n // 2]), np.arange(0), np.arange(n)):
        pos_src = np.zeros(n + 1, np.int32)
        pos_src[rows + 1] = np.arange(1, len(rows) + 1)
        sub_idx, sub_w = AR.nbr_gather(c["idx"], c["widx"], rows)
        assert np.array_equal(sub_idx, idx[torch.from_numpy(rows)].int().numpy()) and np.array_equal(sub_w, c["widx"][rows])
        sub_attn = attn[rows]
        fk, fp, fs, fv, tot = AR.inv_filter(order[:total], skey[:total], k, pos_src, None, sub_attn, n_dst, len(rows) * k)
        sk2, or2, rp2 = AR.invert(sub_idx, n_dst)
        p2, s2, v2 = AR.attn_invert_fill(or2, sub_attn, k)
        assert tot == rp2[-1] and np.array_equal(fk, sk2)
        assert np.array_equal(fp, p2[:tot]) and np.array_equal(fs, s2[:tot]) and np.array_equal(fv, v2[:tot])
    pos = rng.permutation(n_dst + 1).astype(np.int32)
    pos[0] = 0
    assert np.array_equal(AR.nbr_gather(c["idx"], c["widx"], rows, pos)[0], pos[c["idx"][rows]])


@pytest.mark.parametrize("shape", CASES, ids=str)
def test_grid_inputs_are_exact_in_fp32(shape):
    """P + WT + Q in fp32, in the kernels' order, equals the fp64 sum for every (v, n, c): [h > 0] and h == 0 are the same sets."""
    c = _case(*shape)
    for kk in ("P", "Q", "WT"):
        assert np.array_equal(c[kk] / AR.GRID, np.round(c[kk] / AR.GRID)) and np.abs(c[kk]).max() <= 4
    idx = c["idx"].astype(np.int64)
    q32 = np.where((idx > 0)[:, :, None], c["Q"][np.maximum(idx - 1, 0)], np.float32(0))
    h32 = (c["P"][:, None, :] + c["WT"][c["widx"]]) + q32
    assert h32.dtype == np.float32
    h64 = AR.pre_activation(c["P"], c["Q"], c["WT"], c["idx"], c["widx"])
    assert np.array_equal(h32.astype(np.float64), h64)
    assert c["WT"][0].any() and (c["widx"][c["idx"] == 0] != 0).any() == (c["n_wt"] > 1)
    assert all((c["idx"][:, s] == 0).any() for s in range(c["k"]))
    deg = AR.multiplicity(c["idx"], c["n_dst"])
    if c["n"] >= AR.N_LONG:
        assert deg[AR.LONG_A] == 1100 and deg[AR.LONG_B] == 2 * AR.K_CHUNK + 1
