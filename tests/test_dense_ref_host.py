"""CPU: the fp64 restatements of tests/dense_ref.py (what test_gpu_ngcf_kernels.py and test_gpu_proj_kernels.py hold csrc/ngcf.hip
and csrc/proj.hip to) against torch autograd in fp64 of the operator form of ngcf.NGCF._propagate (the output and all four
gradients), against the oracle's ngcf_propagate on the ngcf_toy fixture, against plain fp64 `@` and torch.optim.Adam -- and the
BOUNDS they hand out: not too tight (the same operations in fp32 on the CPU, run through the protocol of the GPU files, stay inside
every one of them), not too loose (twelve planted defects, evaluated in fp64, each break at least one), and the share of
undecided rows of every case the GPU file draws.

`close`: |got - ref| <= 1e-12 * (sum of the absolute values of the terms), the rtol = 1e-12 of a sum."""
import pytest
import torch
import torch.nn.functional as F

import dense_ref as DR
from conftest import blocks_from_fixture
from oracle import adj as oadj
from oracle import models as om

torch.set_num_threads(4)
RTOL = 1e-12
ROW_OUT = ("dP1", "dP2", "dN", "dXd")
LR, B1, B2, EPS_ADAM = 0.01, 0.9, 0.999, 1e-8


def close(what, got, ref, mag):
    assert got.shape == ref.shape, f"{what}: {tuple(got.shape)} vs {tuple(ref.shape)}"
    err = (got.double() - ref.double()).abs()
    assert bool((err <= RTOL * mag + 1e-300).all()), f"{what}: {float(err.max()):.3e}"


def ratio(got, o, rows=None):
    """worst |got - ref| / bound of one output (over `rows` only, a bool mask)"""
    assert got.shape == o.ref.shape, f"{tuple(got.shape)} vs {tuple(o.ref.shape)}"
    assert bool(torch.isfinite(got if rows is None else got[rows]).all())
    r = (got.double() - o.ref).abs() / (DR.bound(o) + 1e-30)
    r = r if rows is None else r[rows]
    return float(r.max()) if r.numel() else 0.0


# ========================================================================================================= operator forms
def ngcf_opform(c, dtype, G=True, mask=None, flags=None, defect=None):
    """The layer operation by operation in `dtype`, run the way the GPU file runs the kernels: fwd; bwd plain from G and bwd NORM
    from the GIVEN Xp, inv, dZ (+ G); wgrad from the plain bwd's dP.  Rows outside `mask` are computed from zeros (their outputs are
    not compared).  defect: one of the planted ones."""
    keep = torch.ones(c["n"], dtype=torch.bool) if mask is None else mask.bool()
    nz = keep if flags is None else keep & flags.bool()
    if defect == "dz_flags_0_row_read":
        nz = keep
    z0 = lambda t, k: torch.where(k.reshape(-1, *([1] * (t.dim() - 1))), t, torch.zeros_like(t)).to(dtype)
    N, X, Gr = z0(c["N"], keep), z0(c["X"], keep), z0(c["G"], keep)
    W1, W2 = c["W1p"].to(dtype), c["W2p"].to(dtype)
    if defect == "w_swapped":
        W1, W2 = W2, W1
    slope = 0.02 if defect == "slope_002" else 0.2
    a1, a2 = N + X, N * X
    P1, P2 = a1 @ W1, a2 @ W2
    Xp = F.leaky_relu(P1, slope) + F.leaky_relu(P2, slope)
    den = Xp.norm(dim=1).clamp_min(1e-12)
    r = {"Xp": Xp, "inv": 1.0 / den, "Z": Xp / den[:, None]}
    s1 = torch.where(P1 > 0, torch.ones_like(P1), torch.full_like(P1, slope))
    s2 = torch.where(P2 > 0, torch.ones_like(P2), torch.full_like(P2, slope))

    def back(g):
        dP1, dP2 = g * s1, g * s2
        dA1, dA2 = dP1 @ W1.t(), dP2 @ W2.t()
        return {"dP1": dP1, "dP2": dP2, "dN": dA1 + dA2 * X, "dXd": dA1 + dA2 * (X if defect == "dXd_with_X" else N)}

    r["plain"] = back(Gr)
    xp, dz, iv = z0(c["Xp"], nz), z0(c["dZ"], nz), z0(c["inv"], nz)[:, None]
    z = xp * iv
    dot = (z * dz).sum(1, keepdim=True)
    if defect != "dot_on_clamped_row":
        dot = torch.where(iv >= DR.INV_CLAMPED, torch.zeros_like(dot), dot)
    term = iv * (dz - z * dot)
    r["norm"] = back(term + Gr if G else term)
    # wgrad from the plain backward's dP
    p1, p2 = r["plain"]["dP1"], r["plain"]["dP2"]
    if defect in ("last_wave_left_out", "first_wave_tail_twice", "masked_row_counted"):
        per, waves = DR.wgrad_split(c["n"])
        last = (DR._cdiv(DR._cdiv(c["n"], 4), per) - 1) * 4 * per
        w = torch.ones(c["n"], 1, dtype=dtype)
        if defect == "last_wave_left_out":
            assert last > 0
            w[last:] = 0
        elif defect == "first_wave_tail_twice":
            w[4 * per:4 * per + 4] = 2
        else:                                              # the first row outside the mask, with ordinary operands
            i = int((~keep).nonzero()[0])
            a1, a2, p1, p2 = a1.clone(), a2.clone(), p1.clone(), p2.clone()
            a1[i], a2[i] = (c["N"][i] + c["X"][i]).to(dtype), (c["N"][i] * c["X"][i]).to(dtype)
            p1[i], p2[i] = c["G"][i].to(dtype), c["G"][i].to(dtype)
        p1, p2 = p1 * w, p2 * w
    r["dW1p"], r["dW2p"] = a1.t() @ p1, a2.t() @ p2
    return r


def ngcf_protocol(c, r, G=True, mask=None, flags=None):
    """{output: worst err / bound} of a result of ngcf_opform, each kernel's outputs against the restatement from ITS inputs"""
    keep = None if mask is None else mask.bool()
    f = DR.ngcf_fwd(c["N"], c["X"], c["W1p"], c["W2p"], row_mask=mask)
    res = {k: ratio(r[k], f[k], keep) for k in ("Xp", "inv", "Z")}
    bp = DR.ngcf_bwd(c["G"], None, None, None, None, c["N"], c["X"], c["W1p"], c["W2p"], row_mask=mask)
    bn = DR.ngcf_bwd(c["G"] if G else None, c["Xp"], c["inv"], c["dZ"], flags, c["N"], c["X"], c["W1p"], c["W2p"], row_mask=mask)
    res.update({f"plain.{k}": ratio(r["plain"][k], bp[k], keep) for k in ROW_OUT})
    res.update({f"norm.{k}": ratio(r["norm"][k], bn[k], keep) for k in ROW_OUT})
    w = DR.ngcf_wgrad(c["N"], c["X"], r["plain"]["dP1"], r["plain"]["dP2"], row_mask=mask)
    res.update({k: ratio(r[k], w[k]) for k in ("dW1p", "dW2p")})
    return res


def zero_undecided(c, mask=None):
    und = DR.undecided(c["N"], c["X"], c["W1p"], c["W2p"], row_mask=mask)
    c["G"][und] = 0
    c["dZ"][und] = 0
    return und


def poisoned(c, mask, flags):
    """the case as the GPU file hands it to the *_rows_* forms: NaN outside the mask, Xp / dZ NaN where dz_flags is 0"""
    p = dict(c)
    keep, nz = mask.bool(), flags.bool()
    for k in ("N", "X", "G"):
        p[k] = c[k].clone()
        p[k][~keep] = float("nan")
    for k in ("Xp", "dZ", "inv"):
        p[k] = c[k].clone()
        p[k][~nz] = float("nan")
    return p


# ============================================================================================================ exactness
@pytest.mark.parametrize("Din,Dout", DR.SHAPES, ids=lambda v: str(v))
def test_restatement_vs_autograd_fp64(Din, Dout):
    """fwd + bwd NORM + wgrad = fp64 autograd of leaky_relu(matmul(nei + x, W1 + b1)) + leaky_relu(matmul(nei * x, W2 + b2)) and
    normalize (the operator form of NGCF._propagate): with and without G, with row_mask / dz_flags (G = 0 outside the mask, dZ = 0
    where the flag is 0, which is what they promise); row 3 mod 8 is scaled until its output row is clamped and non-zero."""
    n = 67
    c = DR.make_case(n, Din, Dout, seed=3 * Din + Dout)
    tiny = c["r"] == 3
    c["N"][tiny] *= 1e-14
    c["X"][tiny] *= 1e-14
    mask, flags = DR.make_masks(n, seed=Din + Dout)
    g = torch.Generator().manual_seed(1)
    b1, b2 = torch.randn(1, Dout, generator=g).double() * 0.1, torch.randn(1, Dout, generator=g).double() * 0.1
    for with_g, masked in ((True, False), (False, False), (True, True)):
        keep = mask.bool() if masked else torch.ones(n, dtype=torch.bool)
        nz = flags.bool() if masked else keep
        nei, x, W1, W2 = (c[k].double().requires_grad_() for k in ("N", "X", "W1p", "W2p"))
        s = F.leaky_relu(torch.matmul(nei + x, W1 + b1), 0.2)
        b = F.leaky_relu(torch.matmul(nei * x, W2 + b2), 0.2)
        xp = s + b
        z = F.normalize(xp, p=2, dim=1)
        G = c["G"].double() * keep[:, None] * (1.0 if with_g else 0.0)
        dZ = c["dZ"].double() * nz[:, None]
        ((xp * G).sum() + (z * dZ).sum()).backward()
        W1p, W2p = (W1 + b1).detach(), (W2 + b2).detach()
        f = DR.ngcf_fwd(c["N"], c["X"], W1p, W2p)
        close("Xp", f["Xp"].ref, xp.detach(), f["Xp"].mag)
        close("Z", f["Z"].ref, z.detach(), f["Z"].ref.abs() + 1e-300)
        assert bool((f["inv"].ref[tiny] == 1e12).all()) and bool((f["Xp"].ref[tiny] != 0).any())
        bw = DR.ngcf_bwd(c["G"] if with_g else None, f["Xp"].ref, f["inv"].ref, c["dZ"], flags if masked else None, c["N"], c["X"],
                         W1p, W2p, row_mask=mask if masked else None)
        close("dN", bw["dN"].ref[keep], nei.grad[keep], bw["dN"].mag[keep])
        close("dXd + dN", (bw["dN"].ref + bw["dXd"].ref)[keep], (nei.grad + x.grad)[keep], (bw["dN"].mag + bw["dXd"].mag)[keep])
        assert bool((nei.grad[~keep] == 0).all())
        w = DR.ngcf_wgrad(c["N"], c["X"], bw["dP1"].ref, bw["dP2"].ref, row_mask=mask if masked else None)
        close("dW1p", w["dW1p"].ref, W1.grad, w["dW1p"].mag)
        close("dW2p", w["dW2p"].ref, W2.grad, w["dW2p"].mag)


def test_autograd_splits_dx_as_the_kernel_does():
    """dN and dXd separately: autograd with the neighbour sum and the table row as two leaves gives the two halves"""
    c = DR.make_case(40, 32, 16, seed=9)
    nei, x = c["N"].double().requires_grad_(), c["X"].double().requires_grad_()
    xp = F.leaky_relu((nei + x) @ c["W1p"].double(), 0.2) + F.leaky_relu((nei * x) @ c["W2p"].double(), 0.2)
    (xp * c["G"].double()).sum().backward()
    b = DR.ngcf_bwd(c["G"], None, None, None, None, c["N"], c["X"], c["W1p"], c["W2p"])
    close("dN", b["dN"].ref, nei.grad, b["dN"].mag)
    close("dXd", b["dXd"].ref, x.grad, b["dXd"].mag)
    # what make_case plants is there
    f = DR.ngcf_fwd(c["N"], c["X"], c["W1p"], c["W2p"])
    r = c["r"]
    assert bool((f["Xp"].ref[r == 1] == 0).all()) and bool((f["inv"].ref[r == 1] == 1e12).all()) and bool((f["Z"].ref[r == 1] == 0).all())
    assert bool((f["P1"].ref[r == 2] == 0).all()) and bool((f["P1"].mag[r == 2] == 0).all()) and bool((f["P2"].ref[r == 2] != 0).all())
    assert bool((f["P2"].ref[r == 4] == 0).all()) and bool((f["P2"].mag[r == 4] == 0).all())
    assert not bool(f["undecided"][(r == 1) | (r == 2) | (r == 4)].any())
    assert bool((c["Xp"][r == 1] == 0).all()) and bool((c["inv"][(r == 1) | (r == 3)] == DR.INV_CLAMPED).all())
    nrm = c["Xp"][r == 3].double().norm(dim=1)
    assert bool(((nrm > 0.5e-13) & (nrm < 2e-13)).all())
    assert bool((c["dZ"][r == 5] == 0).all()) and bool((c["dZ"][r == 6] == 0).all())
    assert bool(torch.signbit(c["dZ"][r == 6]).any(1).all())


def test_restatement_vs_oracle(golden):
    """one layer of `NGCF.bi_inter_embed` as the oracle states it, on the ngcf_toy fixture"""
    fx = golden("ngcf_toy")
    csr = oadj.normalise(oadj.block_adjacency(*blocks_from_fixture(fx, int(fx["use_tag"]))), str(fx["norm_type"]))
    A = om.csr_to_torch(csr).double()
    x0 = torch.cat([torch.from_numpy(fx[k].copy()) for k in sorted(k for k in fx if k.startswith("init.embed."))]).double()
    mats = {k[9:]: torch.from_numpy(fx[k].copy()).double() for k in fx if k.startswith("init.mat.")}
    trace = []
    om.ngcf_propagate(x0, mats, A, 1, trace)
    nei, xp, z = trace[0]
    f = DR.ngcf_fwd(nei, x0, mats["W1_0"] + mats["b1_0"], mats["W2_0"] + mats["b2_0"])
    close("Xp", f["Xp"].ref, xp, f["Xp"].mag)
    close("Z", f["Z"].ref, z, f["Z"].ref.abs() + 1e-300)
    assert float(f["Xp"].ref.abs().max()) > 0


def _adam_state(n, NO, step, seed):
    g = torch.Generator().manual_seed(seed)
    p = torch.randn(n, NO, generator=g) * 0.1
    if step == 1:
        return p, torch.zeros(n, NO), torch.zeros(n, NO)
    return p, torch.randn(n, NO, generator=g) * 0.01, (torch.randn(n, NO, generator=g) * 0.01).abs()


def test_proj_restatements_vs_matmul_and_adam_fp64():
    for i, form in enumerate(DR.TALL_FORMS):
        c = DR.tall_case(form, 37, 32, 64, seed=i)
        X = c["X1"] if c["X2"] is None else torch.cat([c["X1"], c["X2"]], dim=1)
        X = X.double() if c["sel"] is None else X.double()[c["sel"][:37]]
        W = c["W1"].double() if c["W2"] is None else torch.cat([c["W1"].double(), c["W2"].double()], dim=0 if c["w_split"] == 1 else 1)
        want = X @ W
        if c["b1"] is not None:
            want = want + (c["b1"] if c["b2"] is None else torch.cat([c["b1"], c["b2"]])).double()
        if c["old1"] is not None:
            want = want + c["old1"].double()
        o = DR.tall_ref(c)
        close(form, o.ref, want, o.mag)
    g = torch.Generator().manual_seed(5)
    X, dY, oldW, oldb = (torch.randn(*s, generator=g) for s in ((300, 32), (300, 64), (32, 64), (64,)))
    w = DR.tall_wgrad(X, dY[:, :32], dY[:, 32:], old_W=oldW, old_b=oldb)
    close("dW", w["dW"].ref, oldW.double() + X.double().t() @ dY.double(), w["dW"].mag)
    close("db", w["db"].ref, oldb.double() + dY.double().sum(0), w["db"].mag)
    sm = DR.small_mm(X[:18, :10].t(), dY[:18, :32], old=oldW[:10, :32])
    close("small_mm", sm.ref, oldW[:10, :32].double() + X[:18, :10].double().t() @ dY[:18, :32].double(), sm.mag)
    out = dY.clone()
    out[0, :4] = torch.tensor([0.0, -0.0, 1.0, -1.0])
    mc = DR.masked_colsum(X @ torch.randn(32, 64, generator=g), out)
    assert mc.ref.shape == (64,) and float(mc.ref.abs().max()) > 0
    # Adam: torch.optim.Adam in fp64 with the double values of the floats the kernel is handed
    for step in (1, 7):
        p0, m0, v0 = _adam_state(65, 32, step, seed=step)
        Xa, Wa, Gin = torch.randn(65, 16, generator=g) * 0.1, torch.randn(16, 32, generator=g) * 0.3, torch.randn(65, 32, generator=g) * 0.1
        r = DR.tall_mm_adam(Xa, Wa, Gin, p0, m0, v0, LR, B1, B2, EPS_ADAM, step)
        p = p0.double().clone().requires_grad_()
        opt = torch.optim.Adam([p], lr=DR.f32(LR), betas=(DR.f32(B1), DR.f32(B2)), eps=DR.f32(EPS_ADAM))
        p.grad = Gin.double() + Xa.double() @ Wa.double()
        opt.state[p] = {"step": torch.tensor(float(step - 1)), "exp_avg": m0.double().clone(), "exp_avg_sq": v0.double().clone()}
        opt.step()
        close("adam p", r["p"].ref, p.detach(), r["p"].ref.abs() + LR)
        close("adam m", r["m"].ref, opt.state[p]["exp_avg"], r["m"].mag)
        close("adam v", r["v"].ref, opt.state[p]["exp_avg_sq"], r["v"].mag)
    assert DR.wgrad_split(65569) == (9, 1824) and DR.wgrad_split(1) == (8, 4) and DR.wgrad_split(0) == (8, 4)
    assert DR.tall_wgrad_split(DR.TWG_SPW17_N) == (17, 1928) and DR.tall_wgrad_split(65) == (16, 4)


# =============================================================================================================== bounds
HOST_CASES = [(16, 16, 300), (32, 64, 257), (64, 32, 333), (128, 128, 257), (16, 128, 65), (128, 16, 100)]


@pytest.mark.parametrize("Din,Dout,n", HOST_CASES)
def test_bounds_hold_the_fp32_operator_form(Din, Dout, n):
    """not too tight: fp32 on the CPU through the GPU file's protocol (undecided rows get G = 0 and dZ = 0, then row-locality),
    unmasked and with row_mask / dz_flags on poisoned inputs"""
    c = DR.make_case(n, Din, Dout, seed=2 * Din + Dout + n)
    und = zero_undecided(c)
    for G in (True, False):
        r = ngcf_opform(c, torch.float32, G=G)
        res = ngcf_protocol(c, r, G=G)
        print(f"[dense host] fp32 operator form {Din}->{Dout} n={n} G={G}: " + " ".join(f"{k}={v:.3f}" for k, v in res.items()))
        assert max(res.values()) <= 1.0, res
        for k in ROW_OUT:
            assert bool((r["norm"][k][und] == 0).all()) and bool((r["plain"][k][und] == 0).all()), k
    mask, flags = DR.make_masks(n, seed=n)
    p = poisoned(c, mask, flags)
    res = ngcf_protocol(p, ngcf_opform(p, torch.float32, mask=mask, flags=flags), mask=mask, flags=flags)
    assert max(res.values()) <= 1.0, res


def _proj_fp32(dtype=torch.float32, defect=None):
    """{output: err / bound} of the proj operations evaluated in `dtype` in plain torch"""
    res = {}
    for i, form in enumerate(DR.TALL_FORMS):
        for K, NO, n in ((32, 32, 65), (128, 64, 17), (16, 128, 63)):
            if not DR.form_applies(form, K, NO):
                continue
            c = DR.tall_case(form, n, K, NO, seed=7 * i + K)
            X = c["X1"] if c["X2"] is None else torch.cat([c["X1"], c["X2"]], dim=1)
            X = X.to(dtype) if c["sel"] is None else X.to(dtype)[c["sel"][:n]]
            W1, W2 = c["W1"].to(dtype), None if c["W2"] is None else c["W2"].to(dtype)
            if defect == "w1_for_upper_rows" and c["w_split"] == 1:
                W2 = W1
            W = W1 if W2 is None else torch.cat([W1, W2], dim=0 if c["w_split"] == 1 else 1)
            y = X @ W
            if c["b1"] is not None:
                b2 = c["b1"] if defect == "b1_for_second_output" and c["b2"] is not None else c["b2"]
                y = y + (c["b1"] if b2 is None else torch.cat([c["b1"], b2])).to(dtype)
            if c["old1"] is not None:
                y = y + c["old1"].to(dtype)
            res[f"tall_mm.{form}.{K}.{NO}"] = ratio(y, DR.tall_ref(c))
    g = torch.Generator().manual_seed(3)
    for KI, NO, n in ((16, 32, 300), (64, 32, 65)):
        X, d1, d2 = (torch.randn(n, s, generator=g) * sc for s, sc in ((KI, 0.1), (NO // 2, 1.0), (NO // 2, 1.0)))
        w = DR.tall_wgrad(X, d1, d2)
        dY = torch.cat([d1, d2], dim=1).to(dtype)
        db = dY.sum(0)
        if defect == "db2_over_dY1":
            db = torch.cat([d1.to(dtype).sum(0)] * 2)
        res[f"tall_wgrad.dW.{KI}.{NO}"] = ratio(X.to(dtype).t() @ dY, w["dW"])
        res[f"tall_wgrad.db.{KI}.{NO}"] = ratio(db, w["db"])
    for step in (1, 7):
        p0, m0, v0 = _adam_state(65, 32, step, seed=step)
        Xa, Wa, Gin = torch.randn(65, 16, generator=g) * 0.1, torch.randn(16, 32, generator=g) * 0.3, torch.randn(65, 32, generator=g) * 0.1
        r = DR.tall_mm_adam(Xa, Wa, Gin, p0, m0, v0, LR, B1, B2, EPS_ADAM, step)
        t = lambda x: torch.tensor(DR.f32(x), dtype=dtype)
        st = step - 1 if defect == "adam_step_minus_1" and step > 1 else step
        gr = Gin.to(dtype) + Xa.to(dtype) @ Wa.to(dtype)
        got = DR.adam_fp64(p0.to(dtype), m0.to(dtype), v0.to(dtype), gr, t(LR), t(B1), t(B2), t(EPS_ADAM), st)
        for k, x in zip(("p", "m", "v"), got):
            res[f"adam.{k}.step{step}"] = ratio(x, r[k])
    sm = DR.small_mm(Xa.t(), Gin)
    res["small_mm"] = ratio(Xa.to(dtype).t() @ Gin.to(dtype), sm)
    out = torch.randn(300, 64, generator=g)
    d = torch.randn(300, 64, generator=g)
    res["masked_colsum"] = ratio((d.to(dtype) * (out > 0)).sum(0), DR.masked_colsum(d, out))
    return res


def test_proj_bounds_hold_the_fp32_operator_form():
    res = _proj_fp32()
    print("[dense host] fp32 proj: worst " + " ".join(f"{k}={v:.3f}" for k, v in sorted(res.items(), key=lambda kv: -kv[1])[:6]))
    assert max(res.values()) <= 1.0, res


NGCF_DEFECTS = ("w_swapped", "dXd_with_X", "dot_on_clamped_row", "dz_flags_0_row_read", "slope_002", "last_wave_left_out",
                "first_wave_tail_twice", "masked_row_counted")
PROJ_DEFECTS = ("w1_for_upper_rows", "b1_for_second_output", "db2_over_dY1", "adam_step_minus_1")


@pytest.mark.parametrize("defect", NGCF_DEFECTS)
@pytest.mark.parametrize("Din,Dout,n", [(16, 32, 300), (64, 64, 300)])
def test_bounds_catch_planted_ngcf_defects(defect, Din, Dout, n):
    """not too loose: each defect, evaluated in fp64, leaves at least one output outside its bound -- and the same code without
    a defect leaves none"""
    c = DR.make_case(n, Din, Dout, seed=Din + n)
    zero_undecided(c)
    mask, flags = DR.make_masks(n, seed=n)
    kw = dict(mask=mask, flags=flags) if defect in ("dz_flags_0_row_read", "masked_row_counted") else {}
    good = ngcf_protocol(c, ngcf_opform(c, torch.float64, **kw), **kw)
    assert max(good.values()) <= 1e-3, good
    res = ngcf_protocol(c, ngcf_opform(c, torch.float64, defect=defect, **kw), **kw)
    print(f"[dense host] {defect} {Din}->{Dout}: " + " ".join(f"{k}={v:.3g}" for k, v in res.items() if v > 1))
    assert max(res.values()) > 1.0, res


@pytest.mark.parametrize("defect", PROJ_DEFECTS)
def test_bounds_catch_planted_proj_defects(defect):
    good = _proj_fp32(torch.float64)
    assert max(good.values()) <= 1e-3, good
    res = _proj_fp32(torch.float64, defect=defect)
    print(f"[dense host] {defect}: " + " ".join(f"{k}={v:.3g}" for k, v in res.items() if v > 1))
    assert max(res.values()) > 1.0, res


def test_undecided_share_of_every_gpu_case():
    """the cap of the GPU file, on the restatement alone: at most 5 % of a case's rows, none below 64 rows"""
    worst = {}
    for n, Din, Dout in DR.gpu_cases():
        c = DR.gpu_case(n, Din, Dout)
        share = float(DR.undecided(c["N"], c["X"], c["W1p"], c["W2p"]).double().mean())
        assert share <= DR.UNDECIDED_CAP and (n >= 64 or share == 0), (n, Din, Dout, share)
        worst[Din] = max(worst.get(Din, 0.0), share)
    print("[dense host] largest share of undecided rows by Din: " + " ".join(f"{D}: {100 * s:.2f} %" for D, s in sorted(worst.items())))
