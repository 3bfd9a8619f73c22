"""Host side of the multi-negative ranking losses (no GPU): the config keys, the fp64 restatement the GPU tests compare
against (tests/ranking_torch.py), and the loud refusals of everything that consumes (user, positive, one negative) triplets."""
import pytest
import torch
import torch.nn.functional as F

import tagrec_amd as T
from tagrec_amd import _lib, config as C, dist, help as H, rowops

import ranking_torch as R


def test_defaults_and_accepted_values():
    for model in ("lightgcn", "ngcf", "tgcn", "dgcf", "disengcn", "kgat"):
        cfg = T.get_config(model)
        assert cfg["n_negatives"] == 1 and cfg["loss_temperature"] == 1.0
    assert T.disenhan_config()["n_negatives"] == 1
    cfg = T.get_config("lightgcn", n_negatives=63, mul_loss_func="softmax", loss_temperature=0.05)
    assert C.check_ranking(cfg) == (63, "softmax", 0.05)
    assert C.check_ranking({}) == (1, "softplus", 1.0)               # a hand-built config without the keys: the defaults
    assert C.check_ranking(T.get_config("ngcf", n_negatives=4)) == (4, "logsigmoid", 1.0)
    assert C.MAX_NEGATIVES == 63 and C.MUL_LOSS_FUNCS == ("softplus", "logsigmoid", "softmax")
    assert (_lib.LOSS_SOFTPLUS, _lib.LOSS_LOGSIGMOID, _lib.LOSS_SOFTMAX) == (0, 1, 2)
    assert [H.loss_kind_id(n) for n in C.MUL_LOSS_FUNCS] == [0, 1, 2]


@pytest.mark.parametrize("bad", [dict(n_negatives=0), dict(n_negatives=64), dict(n_negatives=-1), dict(n_negatives=2.0),
                                 dict(n_negatives=True), dict(loss_temperature=0), dict(loss_temperature=0.0),
                                 dict(loss_temperature=float("inf")), dict(loss_temperature=float("nan")),
                                 dict(loss_temperature=-1.0), dict(loss_temperature="1"), dict(mul_loss_func="hinge"),
                                 dict(mul_loss_func=None)])
def test_bad_values_are_refused(bad):
    with pytest.raises(T.TagrecError):
        T.get_config("lightgcn", **bad)
    with pytest.raises(T.TagrecError):
        C.check_ranking(bad)


def test_softmax_of_one_negative_is_the_reference_loss():
    """K = 1, tau = 1: logsumexp(s_p, s_n) - s_p = softplus(s_n - s_p), the reference's mul_loss."""
    g = torch.Generator().manual_seed(5)
    s = torch.randn(257, 2, generator=g, dtype=torch.float64) * 6
    got = R.mul_loss64(s, "softmax", 1.0)
    x = s[:, 1] - s[:, 0]
    assert float(x.max()) > 20.0                                     # the batch reaches past F.softplus's threshold
    exact = F.softplus(x, threshold=700.0).mean()                    # log(1 + e^x) itself
    assert abs(float(got) - float(exact)) <= 1e-14 * float(exact)
    # F.softplus (threshold 20, what the reference calls) returns x past the threshold: it drops log1p(e^-x) < e^-20 there
    want = F.softplus(x).mean()
    assert 0.0 <= float(got) - float(want) <= 2.0612e-9
    assert abs(float(R.mul_loss64(s, "softplus")) - float(want)) == 0.0
    # and its derivative: the positive's entry is minus the negative's, a sigmoid of the gap
    c = R.coef64(s, "softmax", 1.0)
    torch.testing.assert_close(c[:, 1], torch.sigmoid(s[:, 1] - s[:, 0]), rtol=0, atol=1e-14)
    torch.testing.assert_close(c[:, 0], -c[:, 1], rtol=0, atol=1e-14)


def test_restatement_on_tables_and_compact_tuples():
    """The two ways the tests address rows agree: tuples into tables, and `compact_tuples` into gathered rows (slot order of
    rowops.tuple_rows: users, then item j of tuple b at row j B + b)."""
    g = torch.Generator().manual_seed(9)
    nu, ni, D, B, K = 11, 13, 6, 5, 3
    U, I = torch.randn(nu, D, generator=g), torch.randn(ni, D, generator=g)
    tup = torch.cat([torch.randint(0, nu, (B, 1), generator=g), torch.randint(0, ni, (B, 1 + K), generator=g)], 1)
    rows = rowops.tuple_rows(tup, nu)
    assert rows.shape == (B * (2 + K),)
    assert torch.equal(rows[:B], tup[:, 0])
    for j in range(1 + K):
        assert torch.equal(rows[B + j * B:B + (j + 1) * B], nu + tup[:, 1 + j])
    assert torch.equal(rowops.tuple_rows(tup[:, :3], nu), rowops.batch_rows(tup[:, :3], nu))
    tab = torch.cat([U, I])
    ct = R.compact_tuples(B, K)
    Ub, Ib = tab[rows[:B]], tab[rows[B:]]
    for name in R.LOSSES:
        a = R.ranking_loss64(U, I, U, I, tup, name, 0.5)
        b = R.ranking_loss64(Ub, Ib, Ub, Ib, ct, name, 0.5)
        assert float(a[0]) == float(b[0]) and float(a[1]) == float(b[1])
    # the pairwise kinds at K > 1 are the mean over the B K pairs
    s = R.scores64(U, I, tup)
    want = torch.stack([F.softplus(s[:, k] - s[:, 0]) for k in range(1, 1 + K)]).mean()
    assert abs(float(R.mul_loss64(s, "softplus")) - float(want)) <= 1e-15


def test_rank_route():
    b3, b6 = torch.zeros(8, 3, dtype=torch.int64), torch.zeros(8, 6, dtype=torch.int64)
    assert H.rank_route("m", b3, 1, "softplus", 1.0) is None and H.rank_route("m", b3, 1, "logsigmoid", 1.0) is None
    assert H.rank_route("m", b3, 1, "softmax", 0.5) == (1, 0.5)
    assert H.rank_route("m", b6, 4, "softplus", 1.0) == (4, 1.0)
    for batch, k in ((b3, 4), (b6, 1), (b6, 3), (b3[:, 0], 1)):
        with pytest.raises(T.TagrecError):
            H.rank_route("m", batch, k, "softmax", 1.0)


REFUSING = [(T.TGCN, lambda **kw: T.get_config("tgcn", **kw)), (T.DGCF, lambda **kw: T.get_config("dgcf", **kw)),
            (T.DisenGCN, lambda **kw: T.get_config("disengcn", **kw)), (T.KGAT, lambda **kw: T.get_config("kgat", **kw)),
            (T.DisenHAN, T.disenhan_config), (T.DGCF_training_data, lambda **kw: T.get_config("dgcf", **kw))]


@pytest.mark.parametrize("bad", [dict(n_negatives=2), dict(mul_loss_func="softmax")])
@pytest.mark.parametrize("cls,make", REFUSING, ids=[c.__name__ for c, _ in REFUSING])
def test_models_without_the_loss_refuse_at_construction(cls, make, bad):
    with pytest.raises(T.TagrecError, match="not covered"):
        cls(None, config=make(**bad))


@pytest.mark.parametrize("bad", [dict(n_negatives=2), dict(mul_loss_func="softmax")])
@pytest.mark.parametrize("cls", [dist.ShardedLightGCN, dist.ShardedNGCF, dist.FeatureShardedLightGCN])
def test_sharded_models_refuse_at_construction(cls, bad):
    with pytest.raises(T.TagrecError, match="not covered"):
        cls(None, T.get_config("lightgcn", **bad), None, None, None, 0)
