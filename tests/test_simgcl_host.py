"""CPU-only: the fp64 restatement of SimGCL (tests/simgcl_torch.py) against hand-computed values, its InfoNCE against
F.cross_entropy, the Python-int noise generator's invariants, and the host side of the feature (config keys, refusals)."""
import math

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import tagrec_amd as T
from tagrec_amd.config import check_contrastive

import simgcl_torch as S
import spmm_ref as R


def test_views_on_a_three_node_graph_by_hand():
    """L = 1, D = 2, eps = 0.5, n = (0.6, 0.8) on every row.  Row 0 gathers (3, -4): x' = (3.3, -4.4), z = (0.6, -0.8);
    row 1 gathers (1, 0): the zero element keeps sign 0, x' = (1.3, 0), z = (1, 0); row 2 is empty and stays zero."""
    A = torch.tensor([[0, 1, 0], [0.5, 0, 0.5], [0, 0, 0]], dtype=torch.float64)
    table = torch.tensor([[1, 0], [3, -4], [1, 0]], dtype=torch.float64)
    n = torch.tensor([[0.6, 0.8]] * 3, dtype=torch.float64)
    x1 = S.perturb(A @ table, n, 0.5)
    assert torch.allclose(x1, torch.tensor([[3.3, -4.4], [1.3, 0.0], [0.0, 0.0]], dtype=torch.float64), rtol=0, atol=1e-15)
    (e,), (ys,) = S.views(A, table, [[n]], 0.5)
    assert torch.equal(ys[0], A @ table)
    want = torch.tensor([[0.8, -0.4], [2.0, -2.0], [0.5, 0.0]], dtype=torch.float64)
    assert torch.allclose(e, want, rtol=0, atol=1e-15)
    # eps = 0: the plain LightGCN mean, whatever the noise
    (e0,), _ = S.views(A, table, [[n * 7]], 0.0)
    assert torch.allclose(e0, (table + S.rownorm(A @ table)) / 2, rtol=0, atol=1e-15)
    # a perturbed row moved by exactly eps (n is a unit vector and no element of the row is zero)
    assert abs(float((x1[0] - (A @ table)[0]).norm()) - 0.5) < 1e-15


def test_info_nce_by_hand_and_against_cross_entropy():
    eye = torch.eye(2, dtype=torch.float64)
    assert abs(float(S.info_nce(eye, eye, 1.0)) - (math.log(math.e + 1.0) - 1.0)) < 1e-15
    g = torch.Generator().manual_seed(5)
    for B, D, tau in ((1, 8, 0.2), (5, 16, 0.2), (33, 64, 1.0)):
        a = S.rownorm(torch.randn(B, D, generator=g, dtype=torch.float64))
        b = S.rownorm(torch.randn(B, D, generator=g, dtype=torch.float64))
        want = F.cross_entropy(a @ b.t() / tau, torch.arange(B))
        assert abs(float(S.info_nce(a, b, tau)) - float(want)) <= 1e-13 * max(1.0, abs(float(want)))


def test_three_part_loss_has_autograd_and_reduces_to_lightgcn():
    g = torch.Generator().manual_seed(3)
    N, nu, D, L = 9, 5, 8, 2
    A = torch.rand(N, N, generator=g, dtype=torch.float64) * (torch.rand(N, N, generator=g) < 0.4)
    table = torch.randn(N, D, generator=g, dtype=torch.float64, requires_grad=True)
    trip = torch.tensor([[0, 1, 2], [4, 3, 0], [0, 3, 1]])
    noise = [[S.rownorm(torch.rand(N, D, generator=g, dtype=torch.float64)) for _ in range(L)] for _ in range(2)]
    parts = S.simgcl_loss(A, table, L, nu, trip, 1e-3, noise, 0.1, 0.2, 0.5)
    sum(parts).backward()
    parts = [p.detach() for p in parts]
    assert len(parts) == 3 and torch.isfinite(table.grad).all() and float(parts[2]) > 0
    table = table.detach()
    base = S.lightgcn_parts(A, table, L, nu, trip, 1e-3)
    assert float(parts[0]) == float(base[0]) and float(parts[1]) == float(base[1])
    # two identical views at eps = 0: a = b, the loss K18 gives on one operand
    e, _ = S.views(A, table, noise, 0.0)
    assert torch.equal(e[0], e[1])
    assert float(S.simgcl_loss(A, table, L, nu, trip, 1e-3, noise, 0.1, 0.2, 0.0)[2]) == 0.0


def test_generator_restatement():
    # the Python-int mix64 is the numpy one of spmm_ref (the dropout masks' generator)
    zs = [0, 1, 2020 << 24, (1 << 64) - 1, 0x9E3779B97F4A7C15]
    assert [S.mix64(z) for z in zs] == [int(v) for v in R.mix64(np.array(zs, dtype=np.uint64))]
    for D in (8, 64, 256):
        nodes = [0, 1, 5, 1599, (1 << 40) + 3]
        n, u = S.noise_dir(2020, 1, 2, nodes, D)
        assert u.shape == (len(nodes), D) and (u > 0).all() and (u <= 1).all()
        assert np.array_equal(u * 65536.0, np.round(u * 65536.0))               # (h16 + 1) 2^-16: 16-bit fractions
        assert np.array_equal(u.astype(np.float32).astype(np.float64), u)       # exact in fp32
        assert np.abs(np.sqrt((n * n).sum(1)) - 1.0).max() <= 4 * 2.0 ** -53
    # every part of the key matters, and the key does not depend on where a row is listed
    base = S.noise_u(7, 0, 1, [3, 4], 16)
    assert np.array_equal(S.noise_u(7, 0, 1, [4, 3], 16), base[::-1])
    for other in (S.noise_u(8, 0, 1, [3, 4], 16), S.noise_u(7, 1, 1, [3, 4], 16), S.noise_u(7, 0, 2, [3, 4], 16)):
        assert (other != base).any(axis=1).all()
    assert 0.45 < S.noise_u(1, 0, 1, range(64), 64).mean() < 0.55


def test_simgcl_config_defaults():
    cfg = T.get_config("simgcl")
    assert (cfg["cl_rate"], cfg["cl_eps"], cfg["cl_temperature"], cfg["use_tag"]) == (0.5, 0.1, 0.2, False)
    light = T.get_config("lightgcn")
    for k in ("mul_loss_func", "norm_type", "cor_batch", "dim_latent", "dim_layer_list", "reg", "message_drop_list", "node_drop"):
        assert cfg[k] == light[k]
    assert cfg["model"] == "simgcl"
    assert not any(k.startswith("cl_") for k in light) and not any(k.startswith("cl_") for k in T.get_config("ngcf"))
    assert check_contrastive(cfg) == (0.5, 0.1, 0.2)
    assert check_contrastive({}) == (0.5, 0.1, 0.2)
    assert T.get_config("simgcl", cl_rate=0, cl_eps=0)["cl_rate"] == 0


@pytest.mark.parametrize("key, bad", [("cl_rate", -0.1), ("cl_rate", float("nan")), ("cl_rate", float("inf")), ("cl_rate", "0.5"),
                                      ("cl_rate", True), ("cl_eps", -1e-9), ("cl_eps", float("inf")), ("cl_eps", None),
                                      ("cl_temperature", 0), ("cl_temperature", -0.2), ("cl_temperature", float("nan")),
                                      ("cl_temperature", float("inf")), ("cl_temperature", False)])
def test_check_contrastive_refuses(key, bad):
    with pytest.raises(T.TagrecError, match=key):
        T.get_config("simgcl", **{key: bad})
    with pytest.raises(T.TagrecError, match=key):
        check_contrastive({key: bad})


def test_simgcl_is_exported_and_needs_a_gpu():
    assert issubclass(T.SimGCL, T.LightGCN)
    ds = T.synth.make_cf_dataset(20, 15, 80, seed=0)
    with pytest.raises(T.TagrecError):                     # no CPU path, with or without a GPU in the machine
        T.SimGCL(ds, config=T.get_config("simgcl", device="cpu"))
