"""CPU-only: the torch restatement of the distance-correlation loss (tests/cor_torch.py) against the reference's own
function, recorded in tests/golden/cor_loss.npz by tools/make_cor_golden.py; the `cor_loss` config key."""
import numpy as np
import pytest
import torch

import cor_torch as C
import tagrec_amd as T

CASES = ("A", "B", "C", "D")


def _case(fx, c):
    return torch.from_numpy(fx[f"{c}.X"]), int(fx[f"{c}.K"])


@pytest.mark.parametrize("c", CASES)
def test_restatement_float64_equals_reference_float64(golden, c):
    """Pins the math and the quirks: adjacent pairs only, the (K + 1) K / 2 divisor, the 1e-8 under both roots."""
    fx = golden("cor_loss")
    X, K = _case(fx, c)
    loss, grad = C.cor_loss_and_grad(X.double(), K)
    np.testing.assert_allclose(float(loss), float(fx[f"{c}.loss64"]), rtol=1e-10, atol=0)
    np.testing.assert_allclose(float(C.cor_loss(X.double(), K)), float(fx[f"{c}.loss64"]), rtol=1e-10, atol=0)
    g64 = fx[f"{c}.grad64"]
    assert np.abs(grad.numpy() - g64).max() <= 1e-10 * np.abs(g64).max()
    # the analytic gradient is the autograd gradient of the restatement
    x = X.double().clone().requires_grad_(True)
    C.cor_loss(x, K).backward()
    assert (x.grad - grad).abs().max() <= 1e-10 * grad.abs().max()


def test_one_factor_gives_zero():
    X = torch.randn(9, 8, generator=torch.Generator().manual_seed(0))
    loss, grad = C.cor_loss_and_grad(X, 1)
    assert float(loss) == 0.0 and float(C.cor_loss(X, 1)) == 0.0 and not grad.any()


@pytest.mark.parametrize("c", CASES)
def test_restatement_float32_is_no_further_from_float64_than_the_reference_float32(golden, c):
    """The direct two-pass form in fp32 against the reference's fp32 matmul form, both measured from the reference's
    float64 values: the loss and the largest gradient error."""
    fx = golden("cor_loss")
    X, K = _case(fx, c)
    loss, grad = C.cor_loss_and_grad(X, K)
    l64, g64 = float(fx[f"{c}.loss64"]), fx[f"{c}.grad64"]
    dl, dl_ref = abs(float(loss) - l64), abs(float(fx[f"{c}.loss32"]) - l64)
    dg = np.abs(grad.double().numpy() - g64).max()
    dg_ref = np.abs(fx[f"{c}.grad32"].astype(np.float64) - g64).max()
    print(f"case {c}: loss error {dl:.3e} (reference fp32 {dl_ref:.3e}), gradient error {dg:.3e} (reference fp32 {dg_ref:.3e})")
    assert dl <= dl_ref and dg <= dg_ref


def test_cor_loss_key_defaults_to_off():
    from tagrec_amd.disenhan import disenhan_config
    assert T.get_config("dgcf")["cor_loss"] is False
    assert T.get_config("disengcn")["cor_loss"] is False
    assert disenhan_config()["cor_loss"] is False
    assert T.get_config("dgcf", cor_loss=True)["cor_loss"] is True
    assert "cor_loss" not in T.get_config("kgat") and "cor_loss" not in T.get_config("lightgcn")
