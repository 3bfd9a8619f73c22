"""GPU: the extended negative sampler (csrc/sampler.hip, tagrec_sample_negative_ex_i64) and the producers that use it.

Candidate ids, and the choice among them on integer tables, are compared exactly with Python-int restatements
(test_neg_sampler_host.py, and py_sample of test_gpu_rowops.py for the old stream).  Float scores are compared with
the float64 dot under the standard bound for a D-term fp32 dot in any order, with or without FMAs:

    |s32 - s64| <= gamma_D * sum_k |u_k i_k|,   gamma_D = D 2^-24 / (1 - D 2^-24).
"""
import functools
import types

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import tagrec_amd as T
from tagrec_amd import _lib, train_data

from test_gpu_rowops import _positives, py_sample
from test_neg_sampler_host import implied_p, py_candidates

DEV = torch.device("cuda:0")
SEED = (2020 << 20) + 3
N_RIGHT = 48
# rows: empty, {0, n_right - 1}, all but id 17, a few ids, empty (the case of test_sampler_equals_python_restatement)
ROWS = [set(), {0, 47}, set(range(48)) - {17}, {3, 4, 5, 30}, set()]
LEFT = torch.randint(0, 5, (1000,), generator=torch.Generator().manual_seed(1))
WIDTHS = (8, 64, 176, 512)        # 2 lanes per entry; 4 entries per wave; 44 of 64 lanes live; two passes


@functools.lru_cache(maxsize=None)
def _pos():
    return _positives(ROWS, N_RIGHT)


@functools.lru_cache(maxsize=None)
def _alias_host():
    # zero weight on the multiples of 7 (id 17, the only negative of row 2, keeps a weight)
    return train_data.alias_table((np.arange(N_RIGHT) % 7).astype(np.float64) ** 0.75)


@functools.lru_cache(maxsize=None)
def _alias_dev():
    prob, idx = _alias_host()
    return torch.from_numpy(prob).to(DEV), torch.from_numpy(idx).to(DEV)


@functools.lru_cache(maxsize=None)
def _restated(n_cand, alias=False, n=1000):
    """Restated candidates [n, n_cand] of the shared case; computed once per (n_cand, proposal)."""
    return np.array(py_candidates(LEFT[:n].tolist(), ROWS, N_RIGHT, SEED, n_cand, _alias_host() if alias else None), dtype=np.int64)


@functools.lru_cache(maxsize=None)
def _tables(D, kind):
    g = torch.Generator().manual_seed(100 + D)
    if kind == "int":             # integers in [-3, 3]: every partial sum of a dot is exact in fp32 whatever the order;
        U = torch.randint(-3, 4, (len(ROWS), D), generator=g).float()
        I = torch.randint(-3, 4, (12, D), generator=g).float().repeat(4, 1)     # item rows repeat with period 12: ties
    else:
        U, I = torch.randn(len(ROWS), D, generator=g), torch.randn(N_RIGHT, D, generator=g)
    return U.to(DEV), I.to(DEV)


def _first_argmax(scores):
    return np.argmax(scores, axis=1)          # numpy: the first of equal maxima


def _gamma(D):
    return D * 2.0 ** -24 / (1 - D * 2.0 ** -24)


# ------------------------------------------------------------------------------------------------------ 1. old stream
@pytest.mark.parametrize("n_rows", [0, 1, 3, 1000])
def test_one_uniform_candidate_is_the_old_stream(n_rows):
    left = LEFT[:n_rows].to(DEV)
    old = _pos().sample(left, SEED)
    neg, cand, score = _pos().sample(left, SEED, return_candidates=True)
    assert torch.equal(neg, old) and torch.equal(cand, neg[:, None]) and score is None
    assert neg.cpu().tolist() == py_sample(LEFT[:n_rows].tolist(), ROWS, N_RIGHT, SEED)


def test_one_candidate_past_32_bits():
    n_right, rows, left = 2 ** 40 + 7, [set(), {0}, set()], torch.tensor([0, 2, 2, 0, 0, 2] * 50)
    neg, cand, _ = _positives(rows, n_right).sample(left.to(DEV), SEED, return_candidates=True)
    assert neg.cpu().tolist() == py_sample(left.tolist(), rows, n_right, SEED) and torch.equal(cand[:, 0], neg)
    assert int(neg.max()) > 2 ** 32


# ------------------------------------------------------------------------------------------------------ 2. candidates
@pytest.mark.parametrize("D", WIDTHS)
@pytest.mark.parametrize("M", [2, 5, 16])
def test_candidates_equal_restatement(M, D):
    U, I = _tables(D, "float")
    neg, cand, score = _pos().sample(LEFT.to(DEV), SEED, n_cand=M, user_table=U, item_table=I, return_candidates=True)
    cand = cand.cpu().numpy()
    assert np.array_equal(cand, _restated(M))
    assert np.array_equal(cand[:, 0], _restated(1)[:, 0])            # candidate 0 is the old negative
    left = LEFT.numpy()
    assert not any(c in ROWS[l] for l, row in zip(left, cand) for c in row)
    assert np.all(cand[left == 2] == 17)
    assert score.shape == (1000, M) and neg.shape == (1000,)


# ---------------------------------------------------------------------------------------------------- 3. exact choice
@pytest.mark.parametrize("D", WIDTHS)
@pytest.mark.parametrize("M", [2, 16])
def test_choice_is_first_argmax_on_integer_tables(M, D):
    U, I = _tables(D, "int")
    neg, cand, score = _pos().sample(LEFT.to(DEV), SEED, n_cand=M, user_table=U, item_table=I, return_candidates=True)
    want_c = _restated(M)
    Ui, Ii = U.cpu().numpy().astype(np.int64), I.cpu().numpy().astype(np.int64)
    exact = np.einsum("ek,eck->ec", Ui[LEFT.numpy()], Ii[want_c])
    assert np.array_equal(cand.cpu().numpy(), want_c)
    assert np.array_equal(score.cpu().numpy().astype(np.float64), exact.astype(np.float64))
    pick = _first_argmax(exact)
    ties = int(np.sum((exact == exact.max(1, keepdims=True)).sum(1) > 1))
    assert ties > 50, ties                                           # the period-12 item rows do produce ties
    assert np.array_equal(neg.cpu().numpy(), want_c[np.arange(1000), pick])


# ---------------------------------------------------------------------------------------------------- 4. float tables
@pytest.mark.parametrize("D", WIDTHS)
@pytest.mark.parametrize("M", [2, 16])
def test_float_scores_within_dot_bound_and_choice_follows_them(M, D):
    U, I = _tables(D, "float")
    neg, cand, score = _pos().sample(LEFT.to(DEV), SEED, n_cand=M, user_table=U, item_table=I, return_candidates=True)
    cand, score = cand.cpu().numpy(), score.cpu().numpy()
    u64 = U.cpu().double().numpy()[LEFT.numpy()][:, None, :]
    i64 = I.cpu().double().numpy()[cand]
    ref, mag = (u64 * i64).sum(-1), np.abs(u64 * i64).sum(-1)
    err = np.abs(score.astype(np.float64) - ref)
    print(f"D={D} M={M}: worst err / bound = {np.max(err / (_gamma(D) * mag)):.3f}")
    assert np.all(err <= _gamma(D) * mag)
    assert np.array_equal(neg.cpu().numpy(), cand[np.arange(1000), _first_argmax(score)])


# --------------------------------------------------------------------------------------------- 5. constant item table
def test_constant_item_table_keeps_candidate_zero():
    U, _ = _tables(64, "float")
    I = torch.full((N_RIGHT, 64), 0.37, device=DEV)
    neg = _pos().sample(LEFT.to(DEV), SEED, n_cand=8, user_table=U, item_table=I)
    assert torch.equal(neg, _pos().sample(LEFT.to(DEV), SEED))


# ---------------------------------------------------------------------------------------------------------- 6. strides
def test_row_views_of_wider_tensors_and_refusals():
    g = torch.Generator().manual_seed(9)
    Uw, Iw = torch.randn(len(ROWS), 128, generator=g).to(DEV), torch.randn(N_RIGHT, 128, generator=g).to(DEV)
    left = LEFT.to(DEV)
    a = _pos().sample(left, SEED, n_cand=4, user_table=Uw[:, :64], item_table=Iw[:, :64], return_candidates=True)
    b = _pos().sample(left, SEED, n_cand=4, user_table=Uw[:, :64].contiguous(), item_table=Iw[:, :64].contiguous(),
                      return_candidates=True)
    assert not Uw[:, :64].is_contiguous()
    assert all(torch.equal(x, y) for x, y in zip(a, b))
    U, I = _tables(64, "float")
    with pytest.raises(T.TagrecError):                               # rows start 4 bytes off a 16-byte boundary
        _pos().sample(left, SEED, n_cand=4, user_table=Uw[:, 1:65], item_table=Iw[:, 1:65])
    with pytest.raises(T.TagrecError):                               # D = 6
        _pos().sample(left, SEED, n_cand=4, user_table=U[:, :6].contiguous(), item_table=I[:, :6].contiguous())
    with pytest.raises(T.TagrecError):
        _pos().sample(left, SEED, n_cand=17, user_table=U, item_table=I)
    with pytest.raises(T.TagrecError):                               # one item row short
        _pos().sample(left, SEED, n_cand=4, user_table=U, item_table=I[:47])
    with pytest.raises(T.TagrecError):                               # a table on the host
        _pos().sample(left, SEED, n_cand=4, user_table=U.cpu(), item_table=I)
    with pytest.raises(T.TagrecError):                               # no tables at all
        _pos().sample(left, SEED, n_cand=4)


# ------------------------------------------------------------------------------------------------------- 7. popularity
@pytest.mark.parametrize("M", [1, 4])
def test_popularity_equals_alias_restatement(M):
    U, I = _tables(64, "int")
    kw = dict(n_cand=M, user_table=U, item_table=I) if M > 1 else {}
    neg, cand, score = _pos().sample(LEFT.to(DEV), SEED, alias=_alias_dev(), return_candidates=True, **kw)
    want_c = _restated(M, alias=True)
    assert np.array_equal(cand.cpu().numpy(), want_c)
    assert not any(c in ROWS[l] for l, row in zip(LEFT.numpy(), want_c) for c in row)
    assert not np.any(want_c % 7 == 0)                               # zero-weight ids never appear
    if M == 1:
        assert score is None and torch.equal(neg, cand[:, 0])
        assert torch.equal(neg, _pos().sample(LEFT.to(DEV), SEED, alias=_alias_dev()))
    else:
        exact = np.einsum("ek,eck->ec", U.cpu().numpy().astype(np.int64)[LEFT.numpy()], I.cpu().numpy().astype(np.int64)[want_c])
        assert np.array_equal(neg.cpu().numpy(), want_c[np.arange(1000), _first_argmax(exact)])


def test_popularity_chi_square_of_an_empty_row_user():
    """200 000 entries of user 0 (no positives: nothing is rejected) against the distribution the stored table implies;
    every live cell expects at least 200 000 * 1 / sum(w) > 1 900 draws.  Bound: chi2 < dof + 6 sqrt(2 dof)."""
    n = 200_000
    neg = _pos().sample(torch.zeros(n, dtype=torch.int64, device=DEV), SEED, alias=_alias_dev())
    p = implied_p(*_alias_host())
    cnt = np.bincount(neg.cpu().numpy(), minlength=N_RIGHT).astype(np.float64)
    live = p > 0
    assert np.all(cnt[~live] == 0) and np.all(n * p[live] >= 5)
    exp = n * p[live]
    chi2, dof = ((cnt[live] - exp) ** 2 / exp).sum(), int(live.sum()) - 1
    print(f"chi2 {chi2:.2f} dof {dof} bound {dof + 6 * np.sqrt(2 * dof):.2f}")
    assert chi2 < dof + 6 * np.sqrt(2 * dof), (chi2, dof)


def test_popularity_refuses_a_user_who_holds_the_whole_support():
    # items 3 and 4 have no train user: the support is {0, 1, 2}, all held by user 0
    ds = types.SimpleNamespace(num={"user": 2, "item": 5}, edge_index={"train": np.array([[0, 0], [0, 1], [0, 2], [1, 1]])})
    cfg = T.get_config("lightgcn", use_tag=False, device=DEV)
    assert T.BPR_training_data(ds, config=cfg, seed=1).all_train_data.shape == (4, 3)       # uniform: items 3, 4 are free
    with pytest.raises(T.TagrecError):
        T.BPR_training_data(ds, config=dict(cfg, neg_sampling="popularity"), seed=1)
    with pytest.raises(T.TagrecError):
        T.BPR_training_data(ds, config=dict(cfg, neg_sampling="by_rank"), seed=1)


# ------------------------------------------------------------------------------------------------------ 8. two launches
@pytest.mark.parametrize("alias", [False, True])
@pytest.mark.parametrize("M,D", [(1, 0), (4, 64), (16, 176), (3, 512)])
def test_two_launches_give_identical_bits(M, D, alias):
    kw = dict(alias=_alias_dev() if alias else None, return_candidates=True)
    if M > 1:
        U, I = _tables(D, "float")
        kw.update(n_cand=M, user_table=U, item_table=I)
    a = _pos().sample(LEFT.to(DEV), SEED, **kw)
    b = _pos().sample(LEFT.to(DEV), SEED, **kw)
    assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1])
    assert (a[2] is None and b[2] is None) or torch.equal(a[2].view(torch.int32), b[2].view(torch.int32))


# ---------------------------------------------------------------------------------------------------------- 9. producer
@pytest.fixture(scope="module")
def toy():
    ds = T.synth.make_cf_dataset(300, 200, 6000, seed=5)
    cfg = T.get_config("lightgcn", use_tag=False, dim_latent=64, dim_layer_list=[64, 64], device=DEV, train_batch=512, epochs=2,
                       test_interval=100)
    tr = torch.as_tensor(np.asarray(ds.edge_index["train"])).to(DEV, torch.int64)
    return ds, cfg, tr


def _old_entry_epoch(tr, seed, epoch=0):
    """The epoch array before the shuffle, straight from the old C entry."""
    pos = train_data._Positives(tr[:, 0], tr[:, 1], 300, 200)
    u, neg = tr[:, 0].contiguous(), torch.empty(tr.shape[0], dtype=torch.int64, device=DEV)
    _lib.check(_lib.load().tagrec_sample_negative_i64(_lib.ptr(u), u.numel(), _lib.ptr(pos.rowptr), _lib.ptr(pos.cols), 300, 200,
                                                      (seed << 20) + epoch, _lib.ptr(neg), _lib.stream_ptr()), "old entry")
    return torch.stack([u, tr[:, 1], neg], dim=1)


def _perm(n, seed):
    gen = torch.Generator(device=DEV)
    gen.manual_seed(seed)
    return torch.randperm(n, device=DEV, generator=gen)


def test_producer_default_keys_give_the_old_epoch_arrays(toy):
    ds, cfg, tr = toy
    assert (cfg["neg_sampling"], cfg["neg_candidates"]) == ("uniform", 1)
    prod = T.BPR_training_data(ds, config=cfg, seed=11)
    want = _old_entry_epoch(tr, 11)[_perm(tr.shape[0], 11)]
    assert torch.equal(prod.all_train_data, want)
    assert prod.tot_inter == tr.shape[0] // 512


def test_producer_hard_negatives(toy):
    """Per edge the kernel keeps the candidate with the highest fp32 score, candidate 0 among them, so
    s32(chosen) >= s32(cand 0); each fp32 score is within gamma_D * mag of its float64 value, hence
    s64(chosen) >= s64(cand 0) - gamma_D * (mag(chosen) + mag(cand 0))."""
    ds, cfg, tr = toy
    cfg4 = dict(cfg, neg_candidates=4)
    torch.manual_seed(4)
    m = T.LightGCN(ds, config=cfg)
    m.train()
    prod = T.BPR_training_data(ds, config=cfg4, seed=11, model=m)
    assert m.training and all(p.grad is None for p in m.parameters())
    data = prod.all_train_data
    perm = _perm(tr.shape[0], 11)
    base = _old_entry_epoch(tr, 11)[perm]                            # same edges in the same order; column 2 = candidate 0
    assert torch.equal(data[:, :2], base[:, :2])
    key = lambda a, b: a * 200 + b
    assert torch.equal(torch.sort(key(data[:, 0], data[:, 1])).values, torch.sort(key(tr[:, 0], tr[:, 1])).values)
    assert not torch.isin(key(data[:, 0], data[:, 2]), key(tr[:, 0], tr[:, 1])).any()
    m.eval()
    with torch.no_grad():
        ut, it = (t.double() for t in m.forward()[:2])
    m.train()
    s = lambda items: ((ut[data[:, 0]] * it[items]).sum(1), (ut[data[:, 0]] * it[items]).abs().sum(1))
    (s_ch, mag_ch), (s_0, mag_0) = s(data[:, 2]), s(base[:, 2])
    assert torch.all(s_ch >= s_0 - _gamma(64) * (mag_ch + mag_0))
    assert int((data[:, 2] != base[:, 2]).sum()) > tr.shape[0] // 4     # the choice does move off candidate 0
    prod.reset()
    assert prod.all_train_data.shape == data.shape and not torch.equal(prod.all_train_data, data)
    assert m.training and all(p.grad is None for p in m.parameters())
    # attach_model: the first epoch waits for the model, then is the same array
    late = T.BPR_training_data(ds, config=cfg4, seed=11)
    assert late.all_train_data is None
    late.attach_model(m).reset()
    assert torch.equal(late.all_train_data, data)
    m.eval()
    late.reset()
    assert not m.training


def test_producer_hard_negatives_need_a_full_table_model(toy):
    ds, cfg, _ = toy
    cfg4 = dict(cfg, neg_candidates=4)
    with pytest.raises(T.TagrecError, match="attach_model"):
        T.BPR_training_data(ds, config=cfg4, seed=11).reset()
    half = types.SimpleNamespace(training=True, eval=lambda: None, train=lambda mode=True: None,
                                 forward=lambda: (torch.zeros(150, 64, device=DEV), torch.zeros(200, 64, device=DEV)))
    with pytest.raises(T.TagrecError, match="attach_model"):
        T.BPR_training_data(ds, config=cfg4, seed=11, model=half)


def test_dgcf_producer_popularity_and_refusal(toy):
    ds, _, tr = toy
    cfg = T.get_config("dgcf", use_tag=False, device=DEV, train_batch=128)
    with pytest.raises(T.TagrecError):
        T.DGCF_training_data(ds, config=dict(cfg, neg_candidates=2), seed=3)
    prod = T.DGCF_training_data(ds, config=dict(cfg, neg_sampling="popularity"), seed=3)
    train_keys = tr[:, 0] * 200 + tr[:, 1]
    held = torch.bincount(tr[:, 1], minlength=200) > 0
    for _, (batch, cor) in zip(range(2), prod.mini_batch()):
        assert batch.shape == (128, 3) and batch.dtype == torch.int64
        assert torch.isin(batch[:, 0] * 200 + batch[:, 1], train_keys).all()
        assert not torch.isin(batch[:, 0] * 200 + batch[:, 2], train_keys).any()
        assert held[batch[:, 2]].all()                               # only items of non-zero weight are proposed


def test_basic_train_runs_with_hard_negatives(toy):
    """Wiring only: two epochs with neg_candidates = 4 run to finite losses (no claim about accuracy)."""
    ds, cfg, _ = toy
    cfg4 = dict(cfg, neg_candidates=4)
    torch.manual_seed(4)
    m = T.LightGCN(ds, config=cfg4)
    train = T.Basic_train([T.BPR_training_data(ds, config=cfg4, seed=3, model=m)], [m.loss], [T.Adam(m.parameters(), lr=0.01)],
                          None, None, config=cfg4)
    hist = train.run(m, verbose=False)
    assert len(hist) == 2 and all(len(h[2]) > 0 and np.isfinite(h[2]).all() for h in hist)
