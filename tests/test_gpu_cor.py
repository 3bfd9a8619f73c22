"""GPU: the distance-correlation kernels (csrc/cor.hip) behind `help.cor_loss`, and the `cor_loss` switch of DGCF,
DisenGCN and DisenHAN.

The yardstick is the reference's own function in float64 (tests/golden/cor_loss.npz, tools/make_cor_golden.py); the
bar is the reference's own fp32 error recorded next to it.  Off the fixture the yardstick is tests/cor_torch.py in
float64, which test_cor_host.py ties to the reference to 1e-10."""
import functools

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import cor_torch as C
import tagrec_amd as T
from tagrec_amd import help as H
from test_disenhan_host import dataset_from_fixture

DEV = torch.device("cuda:0")


def _run(x_view, K, upstream=1.0):
    """(loss, gradient) of help.cor_loss on x_view (a leaf is made of it as it is, strides kept)."""
    x = x_view.detach().requires_grad_(True)
    loss = H.cor_loss(x, K)
    (loss * upstream).backward()
    return loss.detach(), x.grad


# ------------------------------------------------------------------ kernels
@pytest.mark.parametrize("c", ["A", "B", "C", "D"])
def test_kernel_within_the_reference_fp32_error(golden, c):
    """|loss - ref64| <= |ref32 - ref64| and max|grad - ref64| <= max|ref32 grad - ref64|: the kernels are at least
    as close to the reference evaluated in float64 as the reference is to itself in float32."""
    fx = golden("cor_loss")
    X, K = torch.from_numpy(fx[f"{c}.X"]).to(DEV), int(fx[f"{c}.K"])
    loss, grad = _run(X, K)
    assert loss.dim() == 0 and grad.shape == X.shape
    # the sequence-of-slices form of the reference's signature gives the same bits
    x2 = X.clone().requires_grad_(True)
    loss2 = H.cor_loss(torch.split(x2, X.shape[1] // K, dim=1), K)
    loss2.backward()
    assert torch.equal(loss2.detach(), loss) and torch.equal(x2.grad, grad)
    l64, g64 = float(fx[f"{c}.loss64"]), fx[f"{c}.grad64"]
    dl, dl_ref = abs(float(loss) - l64), abs(float(fx[f"{c}.loss32"]) - l64)
    dg = np.abs(grad.double().cpu().numpy() - g64).max()
    dg_ref = np.abs(fx[f"{c}.grad32"].astype(np.float64) - g64).max()
    print(f"case {c}: loss error {dl:.3e} (bar {dl_ref:.3e}), gradient error {dg:.3e} (bar {dg_ref:.3e})")
    assert dl <= dl_ref
    assert dg <= dg_ref


@functools.lru_cache(maxsize=None)
def _off_tile_case(n, D, K):
    """Input (inside a wider tensor), float64 yardstick and the fp32 restatement's distance from it, computed once."""
    g = torch.Generator().manual_seed(1000 * n + D + K)
    big = 0.3 * torch.randn(n, 64 + D + 32, generator=g)
    X = big[:, 64:64 + D]
    up = 0.37
    l64, g64 = C.cor_loss_and_grad(X.double(), K)
    l32, g32 = C.cor_loss_and_grad(X.contiguous(), K)
    return big, up, float(l64), up * g64, abs(float(l32) - float(l64)), float((up * g32.double() - up * g64).abs().max())


@pytest.mark.parametrize("D,K", [(8, 2), (64, 4), (256, 8)])
@pytest.mark.parametrize("n", [2, 63, 65, 129])
def test_shapes_off_the_tile_strided_input_and_upstream_gradient(n, D, K):
    """n below, across and off the 64-lane and tile sizes; the input is a column window of a wider tensor
    (`big[:, 64:64 + D]`), the upstream gradient is 0.37.  Bar: 16 x the distance of the fp32 restatement from the
    float64 one on the same input.  Why 16: that distance is ONE draw of fp32 rounding noise (a few hundred to a few
    thousand roundings that mostly cancel), and the kernels draw another -- they add the same terms in another order
    (tiles of j-rows, a butterfly across lanes) -- so the two differ by the spread of such a draw, not by its typical
    size: a draw falls below a quarter of its standard deviation one time in five, and three standard deviations above
    are not rare over 24 comparisons; 3 / 0.25 = 12, rounded up to a power of two.  A kernel on the matmul form of the
    distances misses this bar by two to four orders of magnitude."""
    big, up, l64, g64, dl_bar, dg_bar = _off_tile_case(n, D, K)
    loss, grad = _run(big.to(DEV)[:, 64:64 + D], K, upstream=up)
    dl = abs(float(loss) - l64)
    dg = float((grad.double().cpu() - g64).abs().max())
    print(f"n={n} D={D} K={K}: loss error {dl:.3e} (bar {16 * dl_bar:.3e}), gradient error {dg:.3e} (bar {16 * dg_bar:.3e})")
    assert dl <= 16 * dl_bar
    assert dg <= 16 * dg_bar


def test_degenerate_inputs_stay_finite():
    g = torch.Generator().manual_seed(3)
    X = torch.randn(40, 32, generator=g)
    X[7] = X[3]                      # two identical rows: their distance is the 1e-4 floor in every slice
    X[:, 8:16] = 0.0                 # an all-zero slice: every distance of it is the floor, its centred matrix vanishes
    loss, grad = _run(X.to(DEV), 4)
    assert torch.isfinite(loss) and torch.isfinite(grad).all()
    assert float(loss) >= 0.0 and float(grad[:, 8:16].abs().max()) == 0.0


def test_two_runs_are_bit_identical():
    X = (0.2 * torch.randn(1500, 64, generator=torch.Generator().manual_seed(4))).to(DEV)
    l0, g0 = _run(X, 4)
    l1, g1 = _run(X, 4)
    assert torch.equal(l0, l1) and torch.equal(g0, g1)


def test_one_factor_gives_zero_and_bad_shapes_raise():
    X = torch.randn(10, 16, device=DEV, requires_grad=True)
    loss = H.cor_loss(X, 1)
    assert loss.dim() == 0 and float(loss.detach()) == 0.0
    loss.backward()
    assert not X.grad.any()
    for bad, K in ((torch.randn(10, 24, device=DEV), 4), (torch.randn(10, 16, device=DEV), 16), (torch.randn(1, 16, device=DEV), 2),
                   (torch.randn(10, 16, device=DEV), 3)):
        with pytest.raises(T.TagrecError):
            H.cor_loss(bad, K)
    with pytest.raises(T.TagrecError):
        H.cor_loss(torch.randn(10, 16), 2)


def test_memory_stays_far_below_one_n_by_n_matrix():
    n, D, K = 4096, 64, 4
    X = (0.1 * torch.randn(n, D, generator=torch.Generator().manual_seed(5))).to(DEV)
    _run(X[:64], K)                                  # code objects loaded, library handle created
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats()
    before = torch.cuda.memory_allocated()
    loss, grad = _run(X, K)
    torch.cuda.synchronize()
    rise = torch.cuda.max_memory_allocated() - before
    print(f"n={n}: peak rise {rise / 2**20:.2f} MiB, one n x n fp32 matrix {n * n * 4 / 2**20:.0f} MiB")
    assert rise < n * n * 4 // 4
    assert torch.isfinite(loss) and torch.isfinite(grad).all()


def test_no_host_sync_in_forward_and_backward():
    """Forward + backward under torch.cuda.set_sync_debug_mode("error").  Whether this torch build honours the mode is
    probed with an `.item()`; if it does not, the run below asserts nothing about syncs."""
    X = (0.1 * torch.randn(300, 64, generator=torch.Generator().manual_seed(6))).to(DEV)
    _run(X, 4)
    up = torch.full((), 0.5, device=DEV)
    torch.cuda.synchronize()
    torch.cuda.set_sync_debug_mode("error")
    try:
        x = X.detach().requires_grad_(True)
        loss = H.cor_loss(torch.split(x, 16, dim=1), 4)
        (loss * up).backward()
        try:
            torch.ones(1, device=DEV).item()
            honoured = False
        except RuntimeError:
            honoured = True
    finally:
        torch.cuda.set_sync_debug_mode("default")
    print("sync debug mode honoured:", honoured)
    assert torch.isfinite(x.grad).all()


# ------------------------------------------------------------------ models
def _dgcf(**kw):
    ds = T.synth.make_cf_dataset(300, 200, 4000, seed=12, n_tag=40, n_assign=600)
    cfg = T.get_config("dgcf", device=DEV, train_batch=128, use_tag=True, dim_layer_list=[64], reg=1e-3, **kw)
    torch.manual_seed(8)
    return ds, cfg, T.DGCF(ds, config=cfg)


def _toy(name, golden, **kw):
    fx = golden(name + "_toy")
    common = dict(dim_latent=int(fx["D"]), dim_layer_list=[int(fx["D"])] * int(fx["n_layer"]), device=DEV, reg=float(fx["reg"]),
                  factor_k=int(fx["factor_k"]), **kw)
    if name == "disenhan":
        m = T.DisenHAN(dataset_from_fixture(fx), config=T.disenhan_config(**common))
    else:
        m = T.DisenGCN(dataset_from_fixture(fx), config=T.get_config("disengcn", use_tag=True, iterate_k=int(fx["iterate_k"]), **common))
    m.load_state_dict({k[5:]: torch.from_numpy(fx[k]) for k in fx if k.startswith("init.")})
    return m, torch.from_numpy(fx["batches"][0][:6]).to(DEV)


def _model_and_batch(name, golden, **kw):
    """(model, triplets [6, 3], cor [3, 4]).  The batch is small so that DGCF's restricted forward is in force on the
    540-node graph (a restriction is applied while 16 x rows <= nodes: 18 + 12 rows here)."""
    if name == "dgcf":
        ds, _, m = _dgcf(**kw)
        trip = torch.from_numpy(T.synth.sample_bpr_epoch(ds, 1)[:6]).to(DEV)
        cor = torch.tensor([[290, 291, 292, 293], [190, 191, 192, 193], [30, 31, 32, 33]], device=DEV)
        rows = torch.cat([trip[:, 0], trip[:, 1] + 300, trip[:, 2] + 300, m._cor_rows(list(cor))])
        assert m.routing.loss_row_mask(rows) is not None
    else:
        m, trip = _toy(name, golden, **kw)
        cor = torch.tensor([[3, 5, 7, 11], [2, 4, 6, 8], [0, 1, 9, 10]], device=DEV)
    m.train()
    return m, trip, cor


def _step(m, batch):
    m.zero_grad()
    parts = m.loss(batch)
    sum(parts).backward()
    return [p.detach().clone() for p in parts], {k: p.grad.clone() for k, p in m.named_parameters()}


@pytest.mark.parametrize("name", ["dgcf", "disengcn", "disenhan"])
def test_switch_off_ignores_the_cor_half_bit_for_bit(name, golden):
    m, trip, cor = _model_and_batch(name, golden, cor_reg=1e-2)          # cor_reg != 0 stays unused while cor_loss is off
    p0, g0 = _step(m, trip)
    p1, g1 = _step(m, (trip, cor))
    assert len(p0) == len(p1) == 2
    assert all(torch.equal(a, b) for a, b in zip(p0, p1))
    assert all(torch.equal(g0[k], g1[k]) for k in g0)


@pytest.mark.parametrize("name", ["dgcf", "disengcn", "disenhan"])
def test_switch_on_adds_the_cor_term(name, golden):
    """Three loss parts; the third is cor_reg * cor_loss of the propagated cor rows; restricted and full forward agree
    (this is what fails when the cor rows are missing from the rows the restricted forward computes).  Tolerances: those
    of test_gpu_routing.test_restricted_top_layer_equals_full_step."""
    m, trip, cor = _model_and_batch(name, golden, cor_loss=True, cor_reg=1e-2)
    res = {}
    for restrict in ((False, True) if hasattr(m, "restrict_forward") else (None,)):
        if restrict is not None:
            m.restrict_forward = restrict
        res[restrict] = _step(m, (trip, cor))
        parts = res[restrict][0]
        assert len(parts) == 3
        with torch.no_grad():
            outs = m.forward()
            want = 1e-2 * H.cor_loss(torch.cat([outs[t][cor[t]] for t in range(3)], dim=0), m.factor_k)
        assert float(parts[2]) > 0
        np.testing.assert_allclose(float(parts[2]), float(want), rtol=1e-6)
    if None not in res:
        (l0, g0), (l1, g1) = res[False], res[True]
        np.testing.assert_allclose([float(v) for v in l1], [float(v) for v in l0], rtol=1e-6)
        top = max(float(v.double().norm()) for v in g0.values())
        for k in g0:
            a, b = g0[k].double(), g1[k].double()
            assert float((a - b).norm()) <= 1e-3 * float(a.norm()) + 1e-6 * top, k
    with pytest.raises(T.TagrecError):
        m.loss(trip)
    with pytest.raises(T.TagrecError):
        m.loss((trip,))


def test_dgcf_epoch_with_the_cor_term():
    ds, cfg, m = _dgcf(cor_loss=True, cor_reg=1e-2)
    prod = T.DGCF_training_data(ds, config=cfg, seed=4)
    losses = T.epoch_training(prod, m.loss, T.Adam(m.parameters(), lr=0.01), verbose=False)
    assert len(losses) == len(ds.edge_index["train"]) // 128 + 1
    assert np.isfinite(losses).all() and losses[-1] < losses[0]
