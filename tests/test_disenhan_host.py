"""CPU-only: DisenHAN's host side against the reference's fixtures (tests/golden/disenhan_*.npz,
tools/make_golden_disenhan.py): the configuration, the merged relation structures, the parameter layout and initial
values, and the plain-torch restatement (tests/disenhan_torch.py) against the reference's forward, loss and gradients."""
import numpy as np
import pytest
import torch

import disenhan_torch as DT
import tagrec_amd as T
from tagrec_amd import disenhan as DH
from tagrec_amd.synth import Coo

FIXTURES = ["disenhan_toy", "disenhan_med"]


def dataset_from_fixture(fx):
    ds = T.synth.Dataset()
    nu, ni, nt = int(fx["n_user"]), int(fx["n_item"]), int(fx["n_tag"])
    ds.num = {"user": nu, "item": ni, "tag": nt}
    one = lambda r: np.ones(len(r), np.float32)
    ds.ui_adj = Coo(fx["ui_row"], fx["ui_col"], one(fx["ui_row"]), (nu, ni))
    ds.ut_adj = Coo(fx["ut_row"], fx["ut_col"], one(fx["ut_row"]), (nu, nt))
    ds.it_adj = Coo(fx["it_row"], fx["it_col"], one(fx["it_row"]), (ni, nt))
    return ds


def test_surface_and_config_defaults():
    assert T.DisenHAN is DH.DisenHAN
    cfg = T.disenhan_config()
    assert cfg["model"] == "disenhan"
    assert (cfg["mul_loss_func"], cfg["norm_type"], cfg["factor_k"], cfg["iterate_k"], cfg["cor_batch"]) == \
        ("softplus", "plain", 4, 2, 100)
    base = T.get_config("lightgcn")
    for k in ("dim_latent", "dim_layer_list", "lr", "reg", "train_batch", "message_drop_list", "use_tag"):
        assert cfg[k] == base[k], k
    assert T.disenhan_config(factor_k=2, reg=1e-3)["factor_k"] == 2
    for m in ("forward", "loss", "predict_rating"):
        assert callable(getattr(T.DisenHAN, m))
    with pytest.raises(KeyError):                   # get_config's scope list is unchanged
        T.get_config("disenhan")


@pytest.mark.parametrize("name", FIXTURES)
def test_merged_relations_match_coalesced_indices(golden, name):
    fx = golden(name)
    rels = DH.merged_relations(dataset_from_fixture(fx))
    assert len(rels) == 6
    for e, (rowptr, col, mult, shape) in zip(DH.RELATIONS, rels):
        assert tuple(shape) == tuple(fx[f"rel.{e}.shape"])
        assert rowptr.dtype == torch.int64 and col.dtype == torch.int32 and mult.dtype == torch.int32
        rows = torch.repeat_interleave(torch.arange(shape[0]), rowptr[1:] - rowptr[:-1])
        np.testing.assert_array_equal(torch.stack([rows, col.long()]).numpy(), fx[f"rel.{e}.idx"])
        np.testing.assert_array_equal(mult.numpy(), fx[f"rel.{e}.mult"])
    # the tag relations really hold duplicates (the multiplicity is exercised), the user-item ones do not
    assert max(int(fx[f"rel.{e}.mult"].max()) for e in ("ut", "it")) > 1
    assert int(fx["rel.ui.mult"].max()) == 1


def test_merged_relations_sum_coo_counts():
    """A COO value is a count: one entry of value 3 is the same merged entry as three entries of value 1."""
    ds = T.synth.Dataset()
    ds.num = {"user": 2, "item": 2, "tag": 3}
    ds.ui_adj = Coo(np.array([0, 1]), np.array([1, 0]), np.ones(2, np.float32), (2, 2))
    ds.ut_adj = Coo(np.array([1, 0, 1]), np.array([2, 0, 2]), np.array([3.0, 1.0, 1.0], np.float32), (2, 3))
    ds.it_adj = Coo(np.array([0]), np.array([1]), np.ones(1, np.float32), (2, 3))
    rels = dict(zip(DH.RELATIONS, DH.merged_relations(ds)))
    rowptr, col, mult, shape = rels["ut"]
    assert rowptr.tolist() == [0, 1, 2] and col.tolist() == [0, 2] and mult.tolist() == [1, 4] and shape == (2, 3)
    rowptr, col, mult, shape = rels["tu"]
    assert rowptr.tolist() == [0, 1, 1, 2] and col.tolist() == [0, 1] and mult.tolist() == [1, 4] and shape == (3, 2)
    rowptr, col, mult, shape = rels["ti"]          # tag 0 has no item: an empty row
    assert rowptr.tolist() == [0, 0, 1, 1] and col.tolist() == [0] and shape == (3, 2)


@pytest.mark.parametrize("name", FIXTURES)
def test_parameter_layout_and_init_order(golden, name):
    """The reference's state-dict keys, order and shapes; xavier_uniform_ in the reference's order from torch's seeded
    CPU generator reproduces its initial values (the draws DisenHAN.__init__ makes)."""
    fx = golden(name)
    K, D, L = int(fx["factor_k"]), int(fx["D"]), int(fx["n_layer"])
    want = [k[5:] for k in fx if k.startswith("init.")]
    num = [int(fx["n_user"]), int(fx["n_item"]), int(fx["n_tag"])]
    keys = [f"embed.{t}" for t in range(3)]
    shapes = [(n, D) for n in num]
    torch.manual_seed(2020)
    values = list(T.base.xavier_tables(num, D, "cpu").split(num))
    for i in range(L):
        lyr = DH.Layer(K, D, D)
        for n, p in lyr.named_parameters():
            torch.nn.init.xavier_uniform_(p)
            keys.append(f"layer.{i}.{n}")
            shapes.append(tuple(p.shape))
            values.append(p.detach())
    assert keys == want
    for k, s, v in zip(keys, shapes, values):
        assert tuple(fx["init." + k].shape) == s, k
        np.testing.assert_array_equal(v.numpy(), fx["init." + k], err_msg=k)


@pytest.mark.parametrize("name", FIXTURES)
def test_torch_restatement_matches_reference(golden, name):
    fx = golden(name)
    K, L = int(fx["factor_k"]), int(fx["n_layer"])
    rels = [DT.coo(r) for r in DH.merged_relations(dataset_from_fixture(fx))]
    tables, layers = DT.params_from_state({k[5:]: fx[k] for k in fx if k.startswith("init.")}, L)
    out = DT.forward(tables, layers, rels, K)
    for t in range(3):
        np.testing.assert_allclose(out[t].detach().numpy(), fx[f"out.{t}"], rtol=1e-5, atol=1e-6)
    parts = DT.loss(out, torch.from_numpy(fx["batches"][0]), float(fx["reg"]), str(fx["loss_kind"]))
    np.testing.assert_allclose([float(p.detach()) for p in parts], fx["loss_parts"], rtol=1e-5, atol=1e-8)
    sum(parts).backward()
    grads = [t.grad for t in tables] + [p.grad for lyr in layers for p in lyr]
    names = [f"embed.{t}" for t in range(3)] + [f"layer.{i}.{n}" for i in range(L) for n in ("Wtk", "at", "W", "q_rela")]
    for n, g in zip(names, grads):
        want = fx["grad." + n]
        np.testing.assert_allclose(g.numpy(), want, rtol=1e-4, atol=1e-6 * np.abs(want).max(), err_msg=n)


def test_torch_restatement_edge_softmax_matches_trace(golden):
    """The first relation's edge softmax of the first iteration against the values the reference computed."""
    fx = golden("disenhan_toy")
    K = int(fx["factor_k"])
    rels = [DT.coo(r) for r in DH.merged_relations(dataset_from_fixture(fx))]
    tables, layers = DT.params_from_state({k[5:]: fx[k] for k in fx if k.startswith("init.")}, int(fx["n_layer"]))
    Wtk, at, _, _ = layers[0]
    D = tables[0].shape[1]
    dk = D // K
    ego = [torch.nn.functional.normalize(torch.nn.functional.leaky_relu(torch.einsum("nd,kde->nke", tables[t], Wtk[t]), 0.2),
                                         dim=2).reshape(-1, D) for t in range(3)]
    for e, (a, b) in enumerate(DT.INDEX):
        rows, cols, mult, shape = rels[e]
        sL = (ego[a].view(-1, K, dk) * at[e, :, :dk]).sum(-1)
        sR = (ego[b].view(-1, K, dk) * at[e, :, dk:]).sum(-1)
        r = torch.full((shape[0], K), 1.0 / K, dtype=torch.float64)
        alpha = DT.edge_softmax(sL, sR, r, rows, cols, mult, shape[0])
        np.testing.assert_allclose(alpha.detach().numpy(), fx[f"trace.alpha.0.0.{DH.RELATIONS[e]}"], rtol=1e-5, atol=1e-7)
