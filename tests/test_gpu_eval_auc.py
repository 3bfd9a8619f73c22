"""GPU: top-K + per-user AUC in one pass over the item table (csrc/eval.hip, tagrec_eval_topk_auc_f32) and the
grouped / AUC-reporting evaluation built on it (Basic_test.run(..., group_k=k), the default above 50 000 items).

Most kernel cases use embeddings on a coarse grid (entries in {-1, 0, 1} times a power of two), so every dot product
is exact in fp32 whatever the summation order; the host then knows which scores are equal and which differ, and the
pair count must match exactly.  `test_auc_ties_need_bit_identical_scores` uses off-grid values instead, so that it
fails unless positives and the item stream are scored with the same arithmetic."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import tagrec_amd as T
from tagrec_amd import evaluate as EV

DEV = torch.device("cuda:0")


def _csr(lists, n_user):
    ptr = np.zeros(n_user + 1, np.int64)
    ptr[1:] = np.cumsum([len(lists.get(u, [])) for u in range(n_user)])
    items = np.array([i for u in range(n_user) for i in sorted(lists.get(u, []))], np.int32)
    return torch.from_numpy(ptr).to(DEV), torch.from_numpy(items).to(DEV)


def _grid(rng, n, D):
    scale = 2.0 ** -(int(np.ceil(np.log2(np.sqrt(D)))) + 1)
    return rng.randint(-1, 2, size=(n, D)).astype(np.float64) * scale


def _host_pairs(z, train, test, n_item):
    """(auc_num2, n_pos, n_neg) of one user from exact dot products z [n_item] (fp32 sigmoid on the host: distinct z
    here are far enough apart that their fp32 sigmoids differ unless both saturate to 1)."""
    s = (1.0 / (1.0 + np.exp(-z))).astype(np.float32)
    valid = np.ones(n_item, bool)
    valid[np.asarray(train, np.int64)] = False
    pos = np.zeros(n_item, bool)
    pos[np.asarray(test, np.int64)] = True
    pos &= valid
    sp, sn = s[pos], np.sort(s[valid & ~pos])
    lt = np.searchsorted(sn, sp, side="left")
    le = np.searchsorted(sn, sp, side="right")
    return int((2 * lt + (le - lt)).sum()), int(pos.sum()), int(len(sn))


def _run(U, I, users, train, test, K=20):
    n_user = U.shape[0]
    tp, ti = _csr(train, n_user)
    sp, si = _csr(test, n_user)
    Ud = torch.from_numpy(U).float().to(DEV)
    Id = torch.from_numpy(I).float().to(DEV)
    ud = torch.as_tensor(users, dtype=torch.int64, device=DEV)
    return EV.fused_topk_auc(Ud, Id, ud, tp, ti, sp, si, K), (Ud, Id, ud, tp, ti)


def _check(U, I, users, train, test, K=20):
    (top, val, num2, npos, nneg), _ = _run(U, I, users, train, test, K)
    z = U @ I.T                                                     # exact: grid entries, float64
    for row, u in enumerate(users):
        want = _host_pairs(z[u], train.get(u, []), test.get(u, []), I.shape[0])
        got = (int(num2[row]), int(npos[row]), int(nneg[row]))
        assert got == want, (u, got, want)
    return num2, npos, nneg


def _lists(rng, n_user, n_item):
    train = {u: rng.choice(n_item, rng.randint(1, max(2, n_item // 6)), replace=False).tolist() for u in range(n_user)}
    test = {u: rng.choice(n_item, rng.randint(1, 12), replace=False).tolist() for u in range(n_user)}
    train[0] = []                                                    # no train items
    train[1] = list(range(n_item - 5))                               # everything masked but five items
    test[1] = [n_item - 1, n_item - 3, 2]
    train[2] = train[2] + train[2][:3]                               # duplicate ids in both lists
    test[2] = test[2] + test[2][:2] + [train[2][0]]                  # ... and a test id that is a train id
    test[3] = train[3][:2]                                           # no valid positive
    return train, test


@pytest.mark.parametrize("D,n_user,n_item", [(16, 70, 333), (64, 130, 1000), (192, 64, 517), (512, 40, 200)])
def test_auc_pair_count_exact(D, n_user, n_item):
    rng = np.random.RandomState(D + n_item)
    U, I = _grid(rng, n_user, D), _grid(rng, n_item, D)
    train, test = _lists(rng, n_user, n_item)
    users = rng.permutation(n_user)[: n_user - 2]
    users = np.concatenate([[0, 1, 2, 3], users[~np.isin(users, [0, 1, 2, 3])]])
    num2, npos, nneg = _check(U, I, users, train, test)
    assert int(npos[3]) == 0 and int(num2[3]) == 0


def test_auc_exact_ties_and_saturation():
    """Items drawn from six distinct rows whose dot product with every user is one of -2, -0.5, 0, 1, 24, 40: the
    last two both saturate the fp32 sigmoid to 1.0, so ties are everywhere.  auc_num2 must equal the pair count."""
    rng = np.random.RandomState(7)
    D, n_user, n_item = 64, 100, 777
    U = np.zeros((n_user, D))
    U[:, 0] = 1.0
    U[:, 1:] = _grid(rng, n_user, D - 1)
    rows = np.zeros((6, D))
    rows[:, 0] = [-2.0, -0.5, 0.0, 1.0, 24.0, 40.0]
    I = rows[rng.randint(0, 6, n_item)]
    train, test = _lists(rng, n_user, n_item)
    _check(U, I, np.arange(n_user), train, test)


def test_auc_ties_need_bit_identical_scores():
    """Items drawn from six distinct rows of ordinary (off-grid) fp32 values, users likewise: each row's score is
    rounded differently by every summation order, so two items share a score exactly when they share a row -- but only
    if the positives are scored with the same arithmetic as the item stream.  Scores sit near -11, -8, -5.5, -3 (where
    the fp32 sigmoid keeps the dot product's rounding) and near 25, 40 (both saturate to 1.0).  The host ranks items by
    their row (tied within a row and across the two saturated rows); auc_num2 must equal that pair count."""
    rng = np.random.RandomState(17)
    D, n_user, n_item = 64, 130, 1111
    e = rng.randn(D)
    e /= np.linalg.norm(e)
    U = (e[None, :] + 0.01 * rng.randn(n_user, D)).astype(np.float32).astype(np.float64)
    level = np.array([-11.0, -8.0, -5.5, -3.0, 25.0, 40.0])
    rows = (level[:, None] * e[None, :] + 0.01 * rng.randn(6, D)).astype(np.float32).astype(np.float64)
    z = U @ rows.T                                                   # float64: only to check the spacing
    assert (np.abs(z[:, :4] - level[:4]) < 0.5).all() and (z[:, 4:] > 20.0).all()
    cls = rng.randint(0, 6, n_item)
    I = rows[cls]
    rank = np.minimum(cls, 4)                                        # rows 4 and 5 tie at sigmoid = 1.0
    train, test = _lists(rng, n_user, n_item)
    (_, _, num2, npos, nneg), _ = _run(U, I, np.arange(n_user), train, test)
    tied = 0
    for u in range(n_user):
        valid = np.ones(n_item, bool)
        valid[np.asarray(train[u], np.int64)] = False
        pos = np.zeros(n_item, bool)
        pos[np.asarray(test[u], np.int64)] = True
        pos &= valid
        rp, rn = rank[pos], np.sort(rank[valid & ~pos])
        lt = np.searchsorted(rn, rp, side="left")
        le = np.searchsorted(rn, rp, side="right")
        tied += int((le - lt).sum())
        want = (int((2 * lt + (le - lt)).sum()), int(pos.sum()), int(len(rn)))
        assert (int(num2[u]), int(npos[u]), int(nneg[u])) == want, (u, want)
    assert tied > 1000                                               # the check rests on many exact ties


def test_auc_user_above_lds_cap():
    """Users with more valid positives than one pass holds (127) share a block with small users: exact."""
    rng = np.random.RandomState(3)
    D, n_user, n_item = 64, 150, 2100
    U, I = _grid(rng, n_user, D), _grid(rng, n_item, D)
    train, test = _lists(rng, n_user, n_item)
    for u, n in ((10, 700), (70, 129), (71, 128), (149, 300)):
        free = np.setdiff1d(np.arange(n_item), train[u])
        test[u] = rng.choice(free, n, replace=False).tolist() + test[u][:3]
    _, npos, _ = _check(U, I, np.arange(n_user), train, test)
    assert int(npos[10]) >= 700 and int(npos[149]) >= 300


@pytest.mark.parametrize("D,n_user,n_item,K", [(64, 300, 1000, 20), (256, 130, 515, 20), (16, 70, 33, 10), (384, 64, 200, 64)])
def test_topk_bitwise_equal_to_topk_entry(D, n_user, n_item, K):
    gen = torch.Generator(device=DEV).manual_seed(D + n_item)
    rng = np.random.RandomState(D)
    U = (torch.randn(n_user, D, device=DEV, generator=gen) * 0.3).double().cpu().numpy()
    I = (torch.randn(n_item, D, device=DEV, generator=gen) * 0.3).double().cpu().numpy()
    train, test = _lists(rng, n_user, n_item)
    users = rng.permutation(n_user)[: n_user - 3]
    (top, val, *_), (Ud, Id, ud, tp, ti) = _run(U, I, users, train, test, K)
    top0, val0 = EV.fused_topk(Ud, Id, ud, tp, ti, K)
    assert torch.equal(top, top0)
    assert torch.equal(val.view(torch.int32), val0.view(torch.int32))


def test_bad_arguments_raise():
    rng = np.random.RandomState(0)
    train, test = _lists(rng, 20, 50)
    with pytest.raises(T.TagrecError):
        _run(_grid(rng, 20, 48), _grid(rng, 50, 48), np.arange(20), train, test)
    with pytest.raises(T.TagrecError):
        _run(_grid(rng, 20, 64), _grid(rng, 50, 64), np.arange(20), train, test, K=65)


class _FixedScores(torch.nn.Module):
    def __init__(self, rating):
        super().__init__()
        self.r = rating

    def predict_rating(self, users):
        return self.r[users].clone()


@pytest.mark.parametrize("k", [2, 3, 4])
def test_grouped_run_matches_reference(golden, k):
    """Basic_test.run(..., group_k=k) on fixed scores (batched path) against the reference's grouped output."""
    fx = golden("eval_groups")
    nu, ni = fx["rating"].shape
    ds = T.synth.Dataset()
    ds.num = {"user": nu, "item": ni}
    ds.user_items = {"train": fx["bt.train"], "test": fx["bt.test"]}
    cfg = T.get_config("lightgcn", device=DEV, test_batch=7, topks=fx["topks"].tolist(), has_val=False)
    res = T.Basic_test(ds, config=cfg).run(_FixedScores(torch.from_numpy(fx["rating"]).to(DEV)), istest=True, group_k=k)
    keys = fx[f"bt.k{k}.keys"].tolist()
    assert list(res.keys()) == keys
    for g, key in enumerate(keys):
        for m in ("recall", "precision", "hr", "ndcg", "auc"):
            np.testing.assert_allclose(res[key][m], fx[f"bt.k{k}.{g}.{m}"], rtol=1e-6, err_msg=f"{key} {m}")


def _close(a, b, atol):
    assert list(a.keys()) == list(b.keys())
    for m in a:
        np.testing.assert_allclose(a[m], b[m], rtol=0, atol=atol, err_msg=m)


class _Frozen(torch.nn.Module):
    """The model's propagated tables, taken once, so that repeated evaluations see bit-identical scores."""
    def __init__(self, model):
        super().__init__()
        with torch.no_grad():
            self.u, self.i = (t.detach().clone() for t in model.forward()[:2])

    def forward(self):
        return self.u, self.i

    def predict_rating(self, users):
        return torch.sigmoid(self.u[users] @ self.i.t())


def test_default_eval_reports_auc_above_threshold():
    """60 000 items: the default Basic_test takes the fused pass and now reports a real AUC, equal to the batched
    path's within 1e-6, ungrouped and per group; every group equals the same evaluation restricted to its users."""
    ds = T.synth.make_cf_dataset(400, 60_000, 260_000)
    assert max(len(v) for v in ds.user_items["test"].values()) > 128      # some users above the per-pass cap
    cfg = T.get_config("lightgcn", use_tag=False, dim_layer_list=[64, 64], device=DEV, test_batch=128)
    torch.manual_seed(3)
    model = T.LightGCN(ds, config=cfg)
    opt = T.Adam(model.parameters(), lr=0.01)
    model.train()
    T.epoch_training(T.BPR_training_data(ds, config=cfg, seed=1), model.loss, opt, verbose=False)
    fused = T.Basic_test(ds, config=cfg)
    batched = T.Basic_test(ds, config=cfg, with_auc=True)
    assert fused.fused_auc and not batched.fused_auc
    res = fused.run(model)
    assert np.isfinite(res["auc"][0]) and 0.0 < res["auc"][0] < 1.0
    ref = batched.run(model)
    assert abs(res["auc"][0] - ref["auc"][0]) <= 1e-6, (res["auc"], ref["auc"])
    for m in ("recall", "precision", "hr", "ndcg"):                      # MFMA vs GEMM scores: near-ties may swap
        np.testing.assert_allclose(res[m], ref[m], rtol=0, atol=1e-3, err_msg=m)

    frozen = _Frozen(model)
    res = fused.run(frozen)
    flat = T.Basic_test(ds, config=cfg, with_auc=False).run(frozen)      # the top-K-only pass: same metrics, no AUC
    assert np.isnan(flat["auc"][0])
    for m in ("recall", "precision", "hr", "ndcg"):
        assert flat[m] == res[m], m
    grouped, grouped_ref = fused.run(frozen, group_k=4), batched.run(frozen, group_k=4)
    groups = T.user_group_split(ds.user_items["test"], ds.user_items["train"], 4)
    assert list(grouped.keys()) == [f"inter<{n}-{len(u)}" for n, u in groups.items()]
    assert list(grouped_ref.keys()) == list(grouped.keys())
    for (n, users), key in zip(groups.items(), grouped):
        g = grouped[key]
        assert np.isfinite(g["auc"][0])
        assert abs(g["auc"][0] - grouped_ref[key]["auc"][0]) <= 1e-6, key
        _close(g, fused.run(frozen, all_users=users), 1e-12)
