"""DisenHAN on the GPU (csrc/disenhan.hip, tagrec_amd/disenhan.py) against the reference's fixtures
(tests/golden/disenhan_*.npz, tools/make_golden_disenhan.py) and against the fp64 plain-torch restatement
(tests/disenhan_torch.py)."""
import json
import math
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import disenhan_torch as DT
import tagrec_amd as T
from conftest import ROOT
from tagrec_amd import disenhan as DH
from test_disenhan_host import dataset_from_fixture

DEV = torch.device("cuda:0")
PARAMS = ("Wtk", "at", "W", "q_rela")


def _model(fx):
    cfg = T.disenhan_config(dim_latent=int(fx["D"]), dim_layer_list=[int(fx["D"])] * int(fx["n_layer"]), device=DEV,
                            reg=float(fx["reg"]), factor_k=int(fx["factor_k"]))
    m = T.DisenHAN(dataset_from_fixture(fx), config=cfg)
    m.load_state_dict({k[5:]: torch.from_numpy(fx[k]) for k in fx if k.startswith("init.")})
    return m


def _grad_check(got, want, rtol=1e-3):
    scale = np.abs(want).max()
    np.testing.assert_allclose(got, want, rtol=rtol, atol=2e-5 * scale)


@pytest.mark.parametrize("name", ["disenhan_toy", "disenhan_med"])
def test_disenhan_golden(golden, name):
    fx = golden(name)
    m = _model(fx)
    m.train()
    assert list(m.state_dict().keys()) == [k[5:] for k in fx if k.startswith("init.")]
    with torch.no_grad():
        for t, o in enumerate(m.forward()):
            np.testing.assert_allclose(o.cpu().numpy(), fx[f"out.{t}"], rtol=1e-4, atol=1e-6)
    cor = torch.zeros(2, 4, dtype=torch.long)
    lossx = m.loss((torch.from_numpy(fx["batches"][0]).to(DEV), cor))
    np.testing.assert_allclose([float(v.detach()) for v in lossx], fx["loss_parts"], rtol=1e-5, atol=1e-8)
    sum(lossx).backward()
    _grad_check(m.table.grad.cpu().numpy(), np.concatenate([fx[f"grad.embed.{t}"] for t in range(3)]))
    for k in range(int(fx["n_layer"])):
        for p in PARAMS:
            _grad_check(getattr(m.layer[k], p).grad.cpu().numpy(), fx[f"grad.layer.{k}.{p}"])
    for n_steps in (1, 3):
        m = _model(fx)
        m.train()
        opt = T.Adam(m.parameters(), lr=float(fx["lr"]))
        prod = T.Fixed_training_data([np.concatenate(fx["batches"][:n_steps])], fx["batches"].shape[1], DEV)
        prod.mini_batch = lambda: iter([(torch.from_numpy(b).to(DEV), cor) for b in fx["batches"][:n_steps]])
        losses = T.epoch_training(prod, m.loss, opt, verbose=False)
        np.testing.assert_allclose(losses, fx[f"step{n_steps}.losses"], rtol=5e-5)
        sd = m.state_dict()
        for key in sd:
            got, want = sd[key].cpu().numpy(), fx[f"step{n_steps}.{key}"]
            # as test_disengcn_golden: Adam turns a ~1e-8 gradient into a visible step on a last-bit difference
            assert np.mean(np.abs(got - want) <= 2e-5) >= 0.99, key
            assert np.abs(got - want).max() <= 1e-3, key
    m = _model(fx)
    m.eval()
    rating = m.predict_rating(torch.from_numpy(fx["predict.users"]))
    np.testing.assert_allclose(rating.cpu().numpy(), fx["predict.rating"], rtol=1e-4, atol=1e-6)


# ---- kernels against the fp64 restatement ---------------------------------------------------------------------------
def _relation(n_a, n_b, seed):
    """Merged relation with duplicates (multiplicities up to 4), empty rows, one row longer than a wavefront (150
    entries) and one hub column (in a third of the rows)."""
    rng = np.random.RandomState(seed)
    m = n_a * 3
    a, b = rng.randint(0, n_a, m), rng.randint(0, n_b, m)
    a = np.where(a % 7 == 3, (a + 1) % n_a, a)                       # rows = 3 mod 7 stay empty
    a = np.concatenate([a, np.full(150, 1), np.arange(0, n_a, 3)])
    b = np.concatenate([b, rng.randint(0, n_b, 150), np.zeros(len(range(0, n_a, 3)), np.int64)])
    keep = a % 7 != 3
    a, b = a[keep], b[keep]
    a, b = np.concatenate([a, a[:40]]), np.concatenate([b, b[:40]])  # explicit duplicates
    key, cnt = np.unique(a.astype(np.int64) * n_b + b, return_counts=True)
    rows, cols = key // n_b, key % n_b
    rowptr = np.zeros(n_a + 1, np.int64)
    np.cumsum(np.bincount(rows, minlength=n_a), out=rowptr[1:])
    rel = (torch.from_numpy(rowptr), torch.from_numpy(cols.astype(np.int32)), torch.from_numpy(cnt.astype(np.int32)), (n_a, n_b))
    assert cnt.max() > 1 and np.diff(rowptr).max() > 64 and (np.diff(rowptr) == 0).any()
    return rel


def _close(got, want, tol=2e-5):
    want = want.detach().cpu().double()
    scale = max(float(want.abs().max()), 1e-30)
    np.testing.assert_allclose(got.detach().cpu().double().numpy(), want.numpy(), rtol=tol, atol=tol * scale)


@pytest.mark.parametrize("D", [32, 64, 128])
@pytest.mark.parametrize("K", [1, 2, 4, 8])
def test_kernels_vs_fp64(K, D):
    n_a, n_b = 300, 200
    rel_h = _relation(n_a, n_b, seed=K * 1000 + D)
    rel = DH.Relation(*rel_h, device=DEV)
    rows, cols, mult, _ = DT.coo(rel_h, DEV)
    g = torch.Generator().manual_seed(K + D)
    rnd = lambda *s: torch.randn(*s, generator=g).double().to(DEV)          # fp32-representable inputs
    sL, sR = rnd(n_a, K), rnd(n_b, K)
    r = torch.softmax(rnd(n_a, K), dim=1)
    X = rnd(n_b, D)
    # edge softmax + product, forward and backward
    ref_in = [t.clone().requires_grad_() for t in (sL, sR, r, X)]
    alpha_ref = DT.edge_softmax(*ref_in[:3], rows, cols, mult, n_a)
    Y_ref = torch.zeros(n_a, D, dtype=torch.float64, device=DEV).index_add(0, rows, alpha_ref[:, None] * ref_in[3][cols])
    gY = rnd(n_a, D)
    (Y_ref * gY).sum().backward()
    got_in = [t.float().clone().requires_grad_() for t in (sL, sR, r, X)]
    alpha = DH.edge_softmax(*got_in[:3], rel)
    _close(alpha, alpha_ref)
    Y = T.routing.valued_spmm(alpha, got_in[3], rel.rg)
    _close(Y, Y_ref)
    (Y * gY.float()).sum().backward()
    for a, b in zip(got_in, ref_in):
        _close(a.grad, b.grad, 1e-4)
    # the relation epilogue (Y of the empty rows is exactly 0: Z = 0, r = 1/K)
    W, q = rnd(D // K, D // K) * 0.3, rnd(D // K)
    ref_in = [t.clone().requires_grad_() for t in (Y_ref.detach(), W, q)]
    Z_ref, r_ref = DT.rel_epilogue(*ref_in, K)
    gZ, gr = rnd(n_a, D), rnd(n_a, K)
    ((Z_ref * gZ).sum() + (r_ref * gr).sum()).backward()
    got_in = [t.float().clone().requires_grad_() for t in (Y_ref.detach(), W, q)]
    Z, r2 = DH.rel_epilogue(*got_in, K)
    _close(Z, Z_ref)
    _close(r2, r_ref)
    empty = (rel_h[0][1:] == rel_h[0][:-1]).to(DEV)
    assert empty.any()
    assert torch.all(Z[empty] == 0) and torch.all(r2[empty] == 1.0 / K)
    ((Z * gZ.float()).sum() + (r2 * gr.float()).sum()).backward()
    for a, b in zip(got_in, ref_in):
        _close(a.grad, b.grad, 1e-4)
    # combine + slice normalisation
    ego, Z1, Z2 = rnd(n_a, D), rnd(n_a, D), rnd(n_a, D)
    r1, r3 = torch.softmax(rnd(n_a, K), 1), torch.softmax(rnd(n_a, K), 1)
    ref_in = [t.clone().requires_grad_() for t in (ego, Z1, r1, Z2, r3)]
    y_ref = DT.combine(ref_in[0], [(ref_in[1], ref_in[2]), (ref_in[3], ref_in[4])], K)
    gy = rnd(n_a, D)
    (y_ref * gy).sum().backward()
    got_in = [t.float().clone().requires_grad_() for t in (ego, Z1, r1, Z2, r3)]
    y = DH.combine(*got_in, K)
    _close(y, y_ref)
    (y * gy.float()).sum().backward()
    for a, b in zip(got_in, ref_in):
        _close(a.grad, b.grad, 1e-4)


def test_edge_softmax_backward_bit_identical():
    n_a, n_b, K = 2000, 500, 4
    rel_h = _relation(n_a, n_b, seed=5)
    rel = DH.Relation(*rel_h, device=DEV)
    g = torch.Generator(device=DEV).manual_seed(3)
    sL, sR = torch.randn(n_a, K, device=DEV, generator=g), torch.randn(n_b, K, device=DEV, generator=g)
    r = torch.softmax(torch.randn(n_a, K, device=DEV, generator=g), 1)
    alpha = DH.edge_softmax(sL, sR, r, rel)
    da = torch.randn(rel.nnz, device=DEV, generator=g)
    first = DH.edge_softmax_bwd(rel, sL, sR, r, alpha, da)
    second = DH.edge_softmax_bwd(rel, sL, sR, r, alpha, da)
    for a, b in zip(first, second):
        assert torch.equal(a, b)


def test_larger_graph_vs_fp64():
    """About 10^4 nodes, 2 layers, K = 4: the model's forward and every gradient against the fp64 restatement."""
    ds = T.synth.make_cf_dataset(4000, 5000, 60000, seed=9, n_tag=1000, n_assign=40000)
    cfg = T.disenhan_config(dim_latent=64, dim_layer_list=[64, 64], device=DEV, reg=1e-3)
    torch.manual_seed(1)
    m = T.DisenHAN(ds, config=cfg)
    m.train()
    batch = torch.from_numpy(T.synth.sample_bpr_epoch(ds, 4)[:512]).to(DEV)
    out = m.forward()
    parts = m.loss(batch)
    sum(parts).backward()
    rels = [DT.coo(r, DEV) for r in DH.merged_relations(ds)]
    tables, layers = DT.params_from_state({k: v.detach() for k, v in m.state_dict().items()}, 2, device=DEV)
    ref = DT.forward(tables, layers, rels, 4)
    for a, b in zip(out, ref):
        _close(a, b, 1e-4)
    ref_parts = DT.loss(ref, batch, 1e-3)
    np.testing.assert_allclose([float(p) for p in parts], [float(p.detach()) for p in ref_parts], rtol=1e-5)
    sum(ref_parts).backward()
    _close(m.table.grad, torch.cat([t.grad for t in tables]), 2e-3)
    for k in range(2):
        for p, want in zip(PARAMS, layers[k]):
            _close(getattr(m.layer[k], p).grad, want.grad, 2e-3)


def test_graph_capture_matches_eager():
    """Three steps through epoch_training(graphs={}) (the third is a captured HIP graph): no capture errors, and the
    same losses and parameters as three eager steps."""
    fx_ds = T.synth.make_cf_dataset(200, 300, 5000, seed=2, n_tag=50, n_assign=3000)
    cfg = T.disenhan_config(dim_latent=32, dim_layer_list=[32], device=DEV, reg=1e-3, factor_k=2)
    tri = T.synth.sample_bpr_epoch(fx_ds, 6)
    batches = [torch.from_numpy(tri[k * 128:(k + 1) * 128]).to(DEV) for k in range(3)]
    results = []
    for graphs in (None, {}):
        torch.manual_seed(0)
        m = T.DisenHAN(fx_ds, config=cfg)
        m.train()
        opt = T.Adam(m.parameters(), lr=0.01, capturable=graphs is not None)
        prod = T.Fixed_training_data([np.concatenate(tri[:384])], 128, DEV)
        prod.mini_batch = lambda: iter(batches)
        losses = T.epoch_training(prod, m.loss, opt, verbose=False, graphs=graphs)
        if graphs is not None:
            assert not graphs.get("errors"), graphs.get("errors")
            assert any(isinstance(v, T.GraphedStep) for v in graphs.values())
        results.append((losses, {k: v.detach().cpu().numpy() for k, v in m.state_dict().items()}))
    np.testing.assert_allclose(results[1][0], results[0][0], rtol=1e-5)
    for k in results[0][1]:
        np.testing.assert_allclose(results[1][1][k], results[0][1][k], rtol=1e-4, atol=1e-6, err_msg=k)


def test_c4_shaped_step_runs():
    """tools/disenhan_step.py's C4 leg at --scale 0.1: the step runs and its loss is finite."""
    cmd = [sys.executable, os.path.join(ROOT, "tools", "disenhan_step.py"), "--skip-c1", "--scale", "0.1", "--c4-steps", "1"]
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=900)
    assert r.returncode == 0, r.stderr[-2000:]
    res = json.loads([ln for ln in r.stdout.splitlines() if ln.startswith("{")][-1])
    assert res["leg"] == "C4" and res["finite"] and math.isfinite(res["loss"])
