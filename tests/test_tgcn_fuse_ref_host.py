"""CPU: the fp64 restatement of tests/tgcn_fuse_ref.py (what test_gpu_tgcn_fuse_kernels.py holds csrc/tgcn_fuse.hip to) against
torch autograd of tgcn._dense_block in fp64 (the output and all 12 gradients), against the oracle's `_atten2` + `_conv` + fusion
layer, `fold` against autograd's dw1 .. dw3 -- and the BOUNDS it hands out: not too tight (the operator form evaluated in fp32 on
the CPU, run through the protocol of the GPU file, stays inside every one of them), not too loose (eight planted defects, evaluated
in fp64, each break at least one), and the share of undecided nodes of every case the GPU file draws.

fp64 evaluations are held to the restatement with `underflow=False` (a soft-max weight of 1e-70 is not 0 there; see its header).

`close`: |got - ref| <= 1e-12 * (sum of the absolute values of the terms), the rtol = 1e-12 of a sum."""
import pytest
import torch

import tgcn_fuse_ref as FR
from oracle import models as om
from tagrec_amd import tgcn as TG

RTOL = 1e-12
A, C, V, NF = FR.A_, FR.C_, FR.V_, FR.NF
CASES = [(16, 16, 300), (32, 64, 257), (64, 32, 333), (128, 128, 257), (16, 128, 65)]
T3 = ("T0", "T1", "T2")


def close(what, got, ref, mag):
    assert got.shape == ref.shape, f"{what}: {tuple(got.shape)} vs {tuple(ref.shape)}"
    err = (got.double() - ref.double()).abs()
    assert bool((err <= RTOL * mag + 1e-300).all()), f"{what}: {float(err.max()):.3e}"


def ratio(got, o):
    """worst |got - ref| / bound of one output"""
    assert got.shape == o.ref.shape, f"{tuple(got.shape)} vs {tuple(o.ref.shape)}"
    return float(((got.double() - o.ref).abs() / (FR.bound(o) + 1e-30)).max())


def opform(c, dtype, g_of=None, defect=None):
    """The block operator by operator in `dtype`, with everything the three kernels hand on, run the way the GPU file runs them:
    out and bw; then, with g = dOut [out > 0] (g_of: another mask), the gradients and the intermediates yvec, dfeat (the gradient
    of the vector-level pre-activations), dS (of S), G.  defect: one of the planted ones."""
    n, D = c["n"], c["D"]
    T = [c[k].to(dtype).clone().requires_grad_() for k in T3]
    P = {k: c[k].to(dtype).clone().requires_grad_() for k in FR.PARAMS}
    t = torch.stack(T, dim=1)
    S = t @ P["U"] + P["q"]
    S.retain_grad()
    bw = torch.softmax(torch.relu(S) @ P["p"], dim=1)
    be = bw[:, [0, 2, 2]] if defect == "bw2_for_j1" else bw
    e = be[:, :, None] * t
    bit = torch.einsum("cj,njd->ncd", P["wb"], e)
    w2 = P["w2"].reshape(V, 2, D)
    if defect == "w2_taps_swapped":
        w2 = w2.flip(1)
    hi = e[:, 0:2] if defect == "e_h_for_e_h1" else e[:, 1:3]
    v1 = torch.einsum("nhd,cd->nch", e, P["w1"])
    v2 = torch.einsum("nhd,cd->nch", e[:, 0:2], w2[:, 0]) + torch.einsum("nhd,cd->nch", hi, w2[:, 1])
    v3 = torch.einsum("njd,cjd->nc", e, P["w3"].reshape(V, 3, D))
    vec = torch.cat([v1.reshape(n, -1), v2.reshape(n, -1), v3], dim=1)
    vec.retain_grad()
    yv = torch.relu(vec)
    if defect == "feature_dropped":
        keep = torch.ones(NF, dtype=dtype)
        keep[17] = 0
        yv = yv * keep
    pre = torch.cat([torch.relu(bit).reshape(n, -1), yv], dim=1) @ P["Wf"] + P["bf"]
    out = torch.relu(pre).detach()
    g = c["dOut"].to(dtype) * (out > 0) if g_of is None else g_of(out)
    (pre * g).sum().backward()
    r = {"bw": bw.detach(), "out": out, "yvec": torch.relu(vec).detach(), "dfeat": vec.grad, "dS": S.grad.reshape(n, 3 * A),
         "dwb": P["wb"].grad, "dq": P["q"].grad, "dp": P["p"].grad, "dWf": P["Wf"].grad, "dU": P["U"].grad, "dbf": P["bf"].grad,
         "dw1": P["w1"].grad, "dw2": P["w2"].grad, "dw3": P["w3"].grad, "e": e.detach()}
    r.update({f"dT{j}": T[j].grad for j in range(3)})
    r["G"] = torch.einsum("nf,njd->fjd", r["dfeat"], r["e"])
    return r


def protocol(c, r, underflow=True):
    """{output: worst err / bound} of a result `r` of opform, each kernel's outputs against the restatement from ITS inputs"""
    ts = [c[k] for k in T3]
    f = FR.fwd(*ts, c, underflow=underflow)
    b = FR.bwd(*ts, c, r["out"], c["dOut"], underflow=underflow)
    w = FR.wf(*ts, r["bw"], r["yvec"], c["wb"], r["out"], c["dOut"], r["dfeat"], r["dS"])
    res = {k: ratio(r[k], f[k]) for k in ("bw", "out")}
    res.update({k: ratio(r[k], b[k]) for k in ("dT0", "dT1", "dT2", "yvec", "dfeat", "dS", "dwb", "dq", "dp")})
    res.update({k: ratio(r[k], w[k]) for k in ("dWf", "G", "dU")})
    return res


def zero_undecided(c):
    und = FR.undecided(c["T0"], c["T1"], c["T2"], c)
    c["dOut"][und] = 0
    return und


# ============================================================================================================ exactness
@pytest.mark.parametrize("D,Dout,n", CASES)
def test_restatement_vs_autograd_fp64(D, Dout, n):
    c = FR.make_case(n, D, Dout, seed=D + Dout + n)
    ts = [c[k].double().requires_grad_() for k in T3]
    ps = [c[k].double().requires_grad_() for k in FR.PARAMS]
    U, q, p, wb, w1, w2, w3, Wf, bf = ps
    want = TG._dense_block(torch.stack(ts, dim=1), U, q, p, wb.reshape(C, 1, 3, 1), w1.reshape(V, 1, 1, D), w2.reshape(V, 1, 2, D),
                           w3.reshape(V, 1, 3, D), Wf, bf)
    (want * c["dOut"].double()).sum().backward()
    raw = [c[k] for k in T3]
    f = FR.fwd(*raw, c, underflow=False)
    close("out", f["out"].ref, want.detach(), f["out"].mag)
    out = f["out"].ref
    b = FR.bwd(*raw, c, out, c["dOut"], underflow=False)
    for j in range(3):
        close(f"dT{j}", b[f"dT{j}"].ref, ts[j].grad, b[f"dT{j}"].mag)
    w = FR.wf(*raw, f["bw"].ref, b["yvec"].ref, c["wb"], out, c["dOut"], b["dfeat"].ref, b["dS"].ref)
    dw = FR.fold_out(w["G"])
    dbf = FR.masked_colsum(out, c["dOut"])
    for name, o, x in (("dU", w["dU"], U), ("dq", b["dq"], q), ("dp", b["dp"], p), ("dwb", b["dwb"], wb), ("dw1", dw[0], w1),
                       ("dw2", dw[1], w2), ("dw3", dw[2], w3), ("dWf", w["dWf"], Wf), ("dbf", dbf, bf)):
        close(name, o.ref, x.grad, o.mag)
    # what make_case plants is there
    pl = c["plant"]
    assert bool((f["bit"].ref[pl["zero"]] == 0).all()) and bool((f["bit"].mag[pl["zero"]] == 0).all())
    assert not bool(f["undecided"][pl["zero"]]) and bool((b["dT0"].ref[pl["zero"]] == 0).all())
    assert bool((c["T1"][pl["one_zero"]] == 0).all()) and bool((c["T0"][pl["one_zero"]] != 0).any())
    assert pl["spread_gap"] > 100 and int((f["bw"].ref[pl["spread"]].float() == 0).sum()) == 2
    # fp32's underflow restated: the two weights are exactly 0, and nothing else moves
    f32 = FR.fwd(*raw, c)
    assert int((f32["bw"].ref[pl["spread"]] == 0).sum()) == 2 and int((f32["bw"].ref == 0).sum()) == 2
    rest = torch.arange(n) != pl["spread"]
    assert torch.equal(f32["out"].ref[rest], out[rest]) and not bool(f32["undecided"][pl["spread"]])
    assert bool((c["dOut"][5] == 0).all()) and int(((out == 0) & (c["dOut"] != 0)).sum()) > n


def test_fold_is_autograds_dw():
    """`fold` alone: G formed from autograd's own intermediates folds into autograd's dw1, dw2, dw3"""
    c = FR.make_case(65, 16, 32, seed=3)
    r = opform(c, torch.float64)
    for got, name in zip(FR.fold(r["G"]), ("dw1", "dw2", "dw3")):
        close(name, got, r[name], got.abs() + 1e-300)
    assert float(r["dw2"].abs().min()) > 0


def test_restatement_vs_oracle():
    """`BasicLayer._atten2`, `_conv` and the fusion layer as the oracle states them (toy size)"""
    n, D, Dout = 23, 16, 32
    c = FR.make_case(n, D, Dout, seed=11)
    prm = {"U": c["U"], "q": c["q"].reshape(1, A), "p": c["p"].reshape(1, A), "conv.bit_level.weight": c["wb"].reshape(C, 1, 3, 1),
           "conv.vec_level.conv_1.weight": c["w1"].reshape(V, 1, 1, D), "conv.vec_level.conv_2.weight": c["w2"].reshape(V, 1, 2, D),
           "conv.vec_level.conv_3.weight": c["w3"].reshape(V, 1, 3, D), "Wf": c["Wf"], "bf": c["bf"].reshape(1, Dout)}
    prm = {k: v.double() for k, v in prm.items()}
    e3 = om.tgcn_atten2(prm, "", *[c[k].double() for k in T3])
    y = om.tgcn_conv(prm, "", e3)
    want = torch.relu(y @ prm["Wf"] + prm["bf"])
    f = FR.fwd(c["T0"], c["T1"], c["T2"], c, underflow=False)
    close("out", f["out"].ref, want, f["out"].mag)
    close("yvec", torch.relu(f["vec"].ref), y[:, C * D:], f["vec"].mag)
    close("bit", torch.relu(f["bit"].ref).reshape(n, -1), y[:, :C * D], f["bit"].mag.reshape(n, -1))


# =============================================================================================================== bounds
@pytest.mark.parametrize("D,Dout,n", CASES)
def test_bounds_hold_the_fp32_operator_form(D, Dout, n):
    """not too tight: fp32 on the CPU through the GPU file's protocol (undecided nodes get dOut = 0, then row-locality)"""
    c = FR.make_case(n, D, Dout, seed=2 * D + Dout + n)
    und = zero_undecided(c)
    r = opform(c, torch.float32)
    res = protocol(c, r)
    print(f"[tgcn_fuse host] fp32 operator form D={D} Dout={Dout} n={n}: " + " ".join(f"{k}={v:.3f}" for k, v in res.items()))
    assert max(res.values()) <= 1.0, res
    for k in ("dT0", "dT1", "dT2", "dfeat", "dS"):
        assert bool((r[k][und] == 0).all()), k
    dw = FR.fold_out(FR.wf(*[c[k] for k in T3], r["bw"], r["yvec"], c["wb"], r["out"], c["dOut"], r["dfeat"], r["dS"])["G"])
    assert max(ratio(r[k], o) for k, o in zip(("dw1", "dw2", "dw3"), dw)) <= 1.0
    assert ratio(r["dbf"], FR.masked_colsum(r["out"], c["dOut"])) <= 1.0


def test_bounds_hold_off_the_grid():
    """inputs on no grid take the worst-case counts of S and s: still inside, with far more undecided nodes"""
    c = FR.make_case(300, 32, 32, seed=5)
    g = torch.Generator().manual_seed(1)
    for k in T3 + ("U", "q", "p"):
        c[k] = c[k] * (1 + 1e-3 * torch.rand(c[k].shape, generator=g))
    assert FR.grid_of(c["T0"]) < 2.0 ** -20
    zero_undecided(c)
    assert max(protocol(c, opform(c, torch.float32)).values()) <= 1.0


DEFECTS = ("w2_taps_swapped", "e_h_for_e_h1", "feature_dropped", "bw2_for_j1", "mask_out_ge_0", "last_wf_group_left_out",
           "rows_past_hi_counted_twice", "dq_without_relu_mask")


@pytest.mark.parametrize("defect", DEFECTS)
@pytest.mark.parametrize("D,Dout,n", [(16, 32, 300), (64, 64, 300)])
def test_bounds_catch_planted_defects(defect, D, Dout, n):
    """not too loose: each defect, evaluated in fp64, leaves at least one output outside its bound -- and the same code without
    a defect leaves none"""
    c = FR.make_case(n, D, Dout, seed=D + n)
    zero_undecided(c)
    ts = [c[k] for k in T3]
    good = opform(c, torch.float64)
    assert max(protocol(c, good, underflow=False).values()) <= 1e-3
    if defect == "mask_out_ge_0":
        res = protocol(c, opform(c, torch.float64, g_of=lambda out: c["dOut"].double() * (out >= 0)), underflow=False)
    elif defect in ("last_wf_group_left_out", "rows_past_hi_counted_twice"):
        per, groups, _, _ = FR.wf_groups(n, D, Dout)
        assert groups >= 2
        w = FR.wf(*ts, good["bw"], good["yvec"], c["wb"], good["out"], c["dOut"], good["dfeat"], good["dS"])
        x = {k: good[k].clone() for k in ("bw", "yvec", "out", "dfeat", "dS")}
        x.update({k: c[k].double().clone() for k in T3 + ("dOut",)})
        if defect == "last_wf_group_left_out":
            for k in ("dOut", "dfeat", "dS"):
                x[k][(groups - 1) * per:] = 0
        else:
            x = {k: torch.cat([v, v[per:per + 8]]) for k, v in x.items()}
        bad = FR.wf(x["T0"], x["T1"], x["T2"], x["bw"], x["yvec"], c["wb"], x["out"], x["dOut"], x["dfeat"], x["dS"])
        res = {k: ratio(bad[k].ref, w[k]) for k in ("dWf", "G", "dU")}
        assert min(res.values()) > 1.0, res                   # every product of the launch shows it
    elif defect == "dq_without_relu_mask":
        b = FR.bwd(*ts, c, good["out"], c["dOut"], underflow=False)
        res = {"dq": ratio((b["ds"].ref[:, :, None] * c["p"].double()).sum((0, 1)), b["dq"])}
    else:
        res = protocol(c, opform(c, torch.float64, defect=defect), underflow=False)
    print(f"[tgcn_fuse host] {defect} D={D} Dout={Dout}: " + " ".join(f"{k}={v:.3g}" for k, v in res.items() if v > 1))
    assert max(res.values()) > 1.0, res


def test_undecided_share_of_every_gpu_case():
    """the cap of the GPU file, on the restatement alone: at most 5 % of a case's nodes, none below 64 nodes"""
    worst = {}
    for n, D, Dout in FR.gpu_cases():
        c = FR.gpu_case(n, D, Dout)
        share = float(FR.undecided(c["T0"], c["T1"], c["T2"], c).double().mean())
        assert share <= FR.UNDECIDED_CAP and (n >= 64 or share == 0), (n, D, Dout, share)
        worst[D] = max(worst.get(D, 0.0), share)
    print("[tgcn_fuse host] largest share of undecided nodes by D: " + " ".join(f"{D}: {100 * s:.2f} %" for D, s in sorted(worst.items())))
