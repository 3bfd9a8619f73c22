"""Host side of the masked catalogue softmax (no GPU): the fp64 restatement the GPU tests compare against
(tests/catsoftmax_masked_torch.py) pinned against explicit loops, help.user_positives_csr, the catalogue_mask key and its
refusals, and the two new entry points in the header and the library."""
import math
import os

import numpy as np
import pytest
import torch

import tagrec_amd as T
from tagrec_amd import config as C, help as H, loss_stage as S

import catsoftmax_masked_torch as CM
import catsoftmax_torch as CS

CAT = dict(softmax_over="catalogue", mul_loss_func="softmax")


def _csr(lists):
    ptr = torch.tensor([0] + list(np.cumsum([len(l) for l in lists])), dtype=torch.int64)
    return ptr, torch.tensor([c for l in lists for c in l], dtype=torch.int32)


def test_restatement_against_a_brute_force_loop():
    """5 x 9: an empty list, a list holding the row's target (which stays live), a list without it, a row whose only live
    column is its target (loss 0), and two batch rows of one user with different targets that exclude each other's."""
    B, N, D, tau = 5, 9, 6, 0.5
    g = torch.Generator().manual_seed(59)
    Q, Tt = torch.randn(4, D, generator=g, dtype=torch.float64), torch.randn(N, D, generator=g, dtype=torch.float64)
    lists = [[], [1, 4, 8], [0, 2, 3], [n for n in range(N) if n != 5]]
    qrow, target = torch.tensor([0, 1, 2, 3, 1]), torch.tensor([3, 4, 7, 5, 8])
    ptr, cols = _csr(lists)
    got, reg = CM.masked_catalogue_loss64(Q, Tt, target, Q, Tt, ptr, cols, tau, qrow)
    rows = []
    for b in range(B):
        ex = set(lists[int(qrow[b])]) - {int(target[b])}
        zs = {n: sum(float(x) * float(y) for x, y in zip(Q[qrow[b]], Tt[n])) / tau for n in range(N) if n not in ex}
        m = max(zs.values())
        rows.append(m + math.log(sum(math.exp(z - m) for z in zs.values())) - zs[int(target[b])])
    assert abs(float(got) - sum(rows) / B) <= 1e-12
    assert rows[3] == 0.0
    assert float(reg) == float(CS.catalogue_loss64(Q, Tt, target, Q, Tt, tau, qrow)[1])          # the L2 part knows no mask
    ex = CM.dense_mask(ptr, cols, target, N, qrow)
    assert ex[1].tolist() == [n in (1, 8) for n in range(N)] and ex[4].tolist() == [n in (1, 4) for n in range(N)]
    assert not ex[0].any() and int(ex[3].sum()) == N - 1
    # every list empty: the unmasked restatement
    e_ptr, e_cols = _csr([[], [], [], []])
    a = CM.masked_catalogue_loss64(Q, Tt, target, None, None, e_ptr, e_cols, tau, qrow)[0]
    assert float(a) == float(CS.catalogue_loss64(Q, Tt, target, None, None, tau, qrow)[0])
    assert float(got) < float(a)                                                 # columns left: every row's sum shrinks
    # the gradient of an excluded column's row of T receives nothing from that batch row
    Tg = Tt.clone().requires_grad_()
    CM.masked_catalogue_loss64(Q, Tg, target[3:4], None, None, ptr, cols, tau, qrow[3:4])[0].backward()
    assert float(Tg.grad.abs().max()) == 0.0


@pytest.mark.parametrize("as_tensor", [False, True])
def test_user_positives_csr(as_tensor):
    """Unsorted input with duplicate edges, a user without edges in the middle and at the end."""
    edges = np.array([[3, 5], [0, 2], [3, 1], [0, 2], [0, 0], [3, 5], [1, 6], [3, 4], [0, 6]], dtype=np.int64)
    ptr, items = H.user_positives_csr(torch.from_numpy(edges) if as_tensor else edges, 5, 7, "cpu")
    assert ptr.dtype == torch.int64 and items.dtype == torch.int32 and ptr.shape == (6,)
    assert ptr.tolist() == [0, 3, 4, 4, 7, 7]
    assert items.tolist() == [0, 2, 6, 6, 1, 4, 5]
    # no edges at all; an id outside the tables is refused
    ptr, items = H.user_positives_csr(np.zeros((0, 2), dtype=np.int64), 3, 4, "cpu")
    assert ptr.tolist() == [0, 0, 0, 0] and items.numel() == 0 and items.dtype == torch.int32
    for bad in ([[5, 0]], [[0, 7]], [[-1, 0]]):
        with pytest.raises(T.TagrecError):
            H.user_positives_csr(np.array(bad), 5, 7, "cpu")
    # a larger random list against python sets
    rng = np.random.default_rng(3)
    e = np.stack([rng.integers(0, 40, 500), rng.integers(0, 30, 500)], 1)
    ptr, items = H.user_positives_csr(e, 40, 30, "cpu")
    for u in range(40):
        assert items[ptr[u]:ptr[u + 1]].tolist() == sorted({int(i) for uu, i in e if uu == u})


def test_check_catalogue_mask():
    assert C.CATALOGUE_MASKS == ("none", "train_positives")
    for model in ("lightgcn", "ngcf", "tgcn", "dgcf", "disengcn", "kgat", "simgcl", "directau"):
        cfg = T.get_config(model)
        assert cfg["catalogue_mask"] == "none" and C.check_catalogue_mask(cfg) is False
    assert T.disenhan_config()["catalogue_mask"] == "none"
    assert C.check_catalogue_mask({}) is False
    for model in ("lightgcn", "ngcf", "simgcl"):
        assert C.check_catalogue_mask(T.get_config(model, catalogue_mask="train_positives", **CAT)) is True
    assert C.check_catalogue_mask(T.get_config("lightgcn", catalogue_mask="none", **CAT)) is False
    for bad in (dict(catalogue_mask="train"), dict(catalogue_mask=None), dict(catalogue_mask=True),
                dict(catalogue_mask="train_positives"),                                             # no softmax_over="catalogue"
                dict(catalogue_mask="train_positives", mul_loss_func="softmax", n_negatives=4),
                dict(catalogue_mask="train_positives", negatives="in_batch", mul_loss_func="softmax")):
        with pytest.raises(T.TagrecError):
            T.get_config("lightgcn", **bad)
        with pytest.raises(T.TagrecError):
            C.check_catalogue_mask(bad)
    assert T._lib.ABI_VERSION == 2


def test_route_and_stage_carry_the_pair():
    pair = (torch.zeros(4, dtype=torch.int64), torch.zeros(0, dtype=torch.int32))
    batch = torch.zeros(8, 2, dtype=torch.int64)
    r = H.catalogue_route("m", batch, 2, pair)
    assert r.temperature == 2.0 and r.positives is pair
    st = H.stage_for(r, H.loss_kind_id("softmax"))
    assert isinstance(st, S.Catalogue) and st.positives is pair and st.temperature == 2.0
    assert H.catalogue_route("m", batch, 2).positives is None and S.Catalogue(1.0).positives is None


REFUSING = [(T.TGCN, lambda **kw: T.get_config("tgcn", **kw)), (T.DGCF, lambda **kw: T.get_config("dgcf", **kw)),
            (T.KGAT, lambda **kw: T.get_config("kgat", **kw)), (T.DisenHAN, T.disenhan_config)]


@pytest.mark.parametrize("cls,make", REFUSING, ids=[c.__name__ for c, _ in REFUSING])
def test_models_without_the_loss_refuse_a_stray_key(cls, make):
    cfg = make()
    cfg["catalogue_mask"] = "train_positives"              # a hand-edited config: softmax_over is still "negatives"
    with pytest.raises(T.TagrecError, match="catalogue_mask"):
        cls(None, config=cfg)


def test_the_two_entry_points_are_declared_and_exported():
    names = ("tagrec_catsoftmax_masked_fwd_f32", "tagrec_catsoftmax_masked_bwd_f32")
    text = open(T._lib.HEADER_PATH).read()
    protos = T._lib.parse_header(text)
    lib = T._lib.load()
    for name, base in zip(names, ("tagrec_catsoftmax_fwd_f32", "tagrec_catsoftmax_bwd_f32")):
        assert name in T._lib.exported_symbols() and hasattr(lib, name)
        restype, argtypes = protos[name]
        # the existing argument list, then the CSR
        assert argtypes == protos[base][1] + [T._lib.I64Ptr, T._lib.I32Ptr] and restype is protos[base][0]
        assert getattr(lib, name).argtypes == argtypes
    assert os.path.basename(T._lib.HEADER_PATH) == "tagrec.h" and lib.tagrec_abi_version() == 2
