"""GPU: train.RowAdam -- the row-sparse Adam of UltraGCN whose lazy rows are caught up exactly (csrc/rowadam.hip).

The yardstick throughout is the dense `T.Adam` on a deterministic=True UltraGCN, from the same seed and the same batches.
Every comparison is `torch.equal` on p, m and v viewed as int32, after `flush()`: the optimizer claims the dense
optimizer's BITS, so there is no tolerance anywhere but in the comparison with torch.optim.Adam at the end, whose atol
2e-4 at lr 0.01 is the one of tests/test_gpu_ultragcn.py for the same comparison."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import tagrec_amd as T
from tagrec_amd import loss_stage as S, rowops

import cooc_ref as R
import ultragcn_torch as UT

DEV = torch.device("cuda:0")
NU, NI, K, B, LR = 300, 200, 4, 64, 0.01
QUIET = 250                    # users QUIET .. NU - 1 are in no batch: rows that are never named
_DS = {}


def _data():
    if "ds" not in _DS:
        ds = T.synth.make_cf_dataset(NU, NI, 3000, seed=5)
        _DS["ds"] = (ds, np.asarray(ds.edge_index["train"], dtype=np.int64))
    return _DS["ds"]


def _model(D, deterministic=True, seed=7):
    ds, _ = _data()
    cfg = T.get_config("ultragcn", device=DEV, dim_latent=D, reg=1e-3, ug_neighbors=3, n_negatives=K, deterministic=deterministic)
    torch.manual_seed(seed)
    return T.UltraGCN(ds, config=cfg)


def _batches(n, seed=11):
    """n batches [B, 2 + K] on the device.  User 0 opens batch 1 and is kept out of batches 2 .. 12; users >= QUIET are in none."""
    if ("b", n, seed) not in _DS:
        _, edges = _data()
        rng = np.random.RandomState(seed)
        loud = edges[edges[:, 0] < QUIET]
        rest = loud[loud[:, 0] != 0]
        out = []
        for step in range(1, n + 1):
            pool = rest if 2 <= step <= 12 else loud
            e = pool[rng.choice(len(pool), size=B, replace=False)].copy()
            if step == 1:
                e[0] = loud[loud[:, 0] == 0][0]
            e[2] = e[1]                                   # a repeated (user, positive): segments longer than one slot
            out.append(torch.from_numpy(np.concatenate([e, rng.randint(0, NI, size=(B, K))], 1).astype(np.int64)).to(DEV))
        _DS[("b", n, seed)] = out
    return _DS[("b", n, seed)]


def _named(model, batch):
    """The table rows a step on `batch` names (users, positives, negatives, the positives' neighbours), on the host."""
    return set(S.Ultra(model.tables).rows(batch, NU).cpu().tolist())


def _step(model, opt, batch, train=True):
    model.train(train)
    opt.zero_grad()
    sum(model.loss(batch)).backward()
    opt.step()
    model.train()


def _dense(D, **kw):
    m = _model(D, True)
    return m, T.Adam(m.parameters(), lr=LR, **kw)


def _lazy(D, max_lag, deterministic=True):
    m = _model(D, deterministic)
    return m, T.RowAdam(m.parameters(), lr=LR, max_lag=max_lag).attach(m)


def _bits(model, opt):
    st = opt.state[id(model.table)]
    return [t.detach().view(torch.int32) for t in (model.table.data, st["m"], st["v"])]


def _assert_same(md, od, ml, ol, what=""):
    for o in (od, ol):
        if isinstance(o, T.RowAdam):
            o.flush()
    for name, a, b in zip("pmv", _bits(md, od), _bits(ml, ol)):
        assert torch.equal(a, b), f"{what}: {name} differs in {int((a != b).sum())} elements"


_DENSE40 = {}


def _dense40(D):
    """The dense run of 40 steps, once per width: (model, optimizer, the table after step 13)."""
    if D not in _DENSE40:
        md, od = _dense(D)
        at13 = None
        for i, b in enumerate(_batches(40), 1):
            _step(md, od, b)
            if i == 13:
                at13 = torch.cat(md.forward()).detach().clone()
        _DENSE40[D] = (md, od, at13)
    return _DENSE40[D]


@pytest.mark.parametrize("D", (8, 64, 20))
def test_forty_steps_with_periodic_flushes_are_the_dense_bits(D):
    batches = _batches(40)
    md, od, at13 = _dense40(D)
    named = [_named(md, b) for b in batches]
    # from the batches: a row named at step 1 and then not for more than 7 steps, and a row that is never named
    gaps = [r for r in named[0] if not any(r in s for s in named[1:9])]
    assert gaps, "no row rests for more than max_lag steps after step 1"
    never = set(range(NU + NI)) - set().union(*named)
    assert never, "every row is named at some step"
    ml, ol = _lazy(D, max_lag=7)
    lagged = 0
    for i, b in enumerate(batches, 1):
        _step(ml, ol, b)
        assert ml.table.grad is None
        lagged = max(lagged, ol.lagging_rows(ml.table))
        assert i - int(ol.row_state(ml.table)[2].min()) < 7     # the periodic flush: after a step nobody is max_lag behind
        if i == 7:
            assert ol.lagging_rows(ml.table) == 0
        if i == 13:                                        # a mid-run read flushes; training goes on from the same state
            got = torch.cat(ml.forward()).detach()
            assert torch.equal(got.view(torch.int32), at13.view(torch.int32))
    assert lagged > 0
    sd, sl = md.state_dict(), ml.state_dict()              # state_dict() flushes by itself
    assert list(sd) == list(sl)
    for k in sd:
        assert torch.equal(sd[k].view(torch.int32), sl[k].view(torch.int32)), k
    _assert_same(md, od, ml, ol, f"D={D}")
    r = next(iter(never))
    assert int(ol.row_state(ml.table)[2][r]) == 40 and not bool(ol.row_state(ml.table)[0][r].any())


def test_laziness_is_real():
    D = 64
    batches = _batches(40)[:5]
    md, od = _dense(D)
    ml, ol = _lazy(D, max_lag=1000)
    for b in batches:
        _step(md, od, b)
        _step(ml, ol, b)
    assert ml.table.grad is None and md.table.grad is not None
    m, v, last, t = ol.row_state(ml.table)
    assert t == 5 and ol.lagging_rows(ml.table) > 0
    behind = (last < 5) & (m != 0).any(1)
    assert bool(behind.any()), "no lagging row with a non-zero first moment"
    r = int(behind.nonzero()[0])
    assert not torch.equal(ml.table.data[r], md.table.data[r])       # dense Adam moved it along the old m; the lazy row rests
    ol.flush()
    assert torch.equal(ml.table.data[r].view(torch.int32), md.table.data[r].view(torch.int32))
    assert ol.lagging_rows(ml.table) == 0
    ol.flush()                                                        # idempotent
    _assert_same(md, od, ml, ol)


@pytest.mark.parametrize("D", (64, 20))
def test_a_segment_longer_than_a_chunk(D):
    rng = np.random.RandomState(3)
    long = np.concatenate([np.full((1100, 1), 17), rng.randint(0, NI, size=(1100, 1 + K))], 1).astype(np.int64)
    seq = [torch.from_numpy(long).to(DEV)] + _batches(40)[:2]
    md, od = _dense(D)
    ml, ol = _lazy(D, max_lag=7)
    for b in seq:
        _step(md, od, b)
        _step(ml, ol, b)
    _assert_same(md, od, ml, ol, f"D={D}")


def test_deterministic_key_does_not_matter():
    ma, oa = _lazy(64, 7, deterministic=False)
    mb, ob = _lazy(64, 7, deterministic=True)
    for b in _batches(40)[:10]:
        _step(ma, oa, b)
        _step(mb, ob, b)
    _assert_same(ma, oa, mb, ob)


def test_dense_gradient_on_an_attached_table():
    md, od = _dense(64)
    ml, ol = _lazy(64, max_lag=7)
    for i, b in enumerate(_batches(40)[:9], 1):
        eval_mode = i in (4, 5)                                       # an eval-mode loss takes the dense path: p.grad arrives
        _step(md, od, b, not eval_mode)
        _step(ml, ol, b, not eval_mode)
        if eval_mode:
            assert ml.table.grad is not None and ol.lagging_rows(ml.table) == 0
    _assert_same(md, od, ml, ol)


# ---- the kernels directly ----

def _table(n, D, seed, stride=None):
    g = torch.Generator().manual_seed(seed)
    stride = stride or D
    mk = lambda scale, pos: ((torch.rand(n, stride, generator=g) - (0 if pos else 0.5)) * scale).to(DEV)[:, :D]
    return mk(0.2, False), mk(0.02, False), mk(1e-4, True)


def _ring(lr, b1, b2, upto, cap):
    """The ring as it stands after step `upto`: the last `cap` steps, step t at entry t mod cap."""
    ring = torch.zeros(cap, 2, dtype=torch.float32, device=DEV)
    t = torch.arange(max(1, upto - cap + 1), upto + 1)
    ring[(t % cap).to(DEV)] = rowops.adam_coef(np.float32(lr), np.float32(b1), np.float32(b2), 1, upto)[t - 1].to(DEV)
    return ring


@pytest.mark.parametrize("D,stride", ((64, 64), (8, 8), (20, 20), (16, 24), (64, 66)))
def test_catch_up_of_a_listed_subset(D, stride):
    n, t_done, lr, (b1, b2), eps = 97, 320, 0.01, (0.9, 0.999), 1e-8
    lib = T._lib.load()
    lags = [0, 1, 2, 7, 300]
    p, m, v = _table(n, D, 1, stride)
    m[5] = 0                                              # a listed row that was never named: zero moments
    v[5] = 0
    ref = [t.contiguous().clone() for t in (p, m, v)]
    rows = torch.tensor([3, 5, 9, 9, 40, 41, 96, 3, 64, 0], dtype=torch.int64, device=DEV)
    lag_of = {r: lags[k % len(lags)] for k, r in enumerate(sorted(set(rows.tolist())))}
    assert set(lag_of.values()) == set(lags)
    last = torch.full((n,), t_done, dtype=torch.int32, device=DEV)
    zero = torch.zeros(D, dtype=torch.float32, device=DEV)
    for r, lag in lag_of.items():
        last[r] = t_done - lag
        rp, rm, rv = (x[r].clone() for x in ref)
        for t in range(t_done - lag + 1, t_done + 1):     # the yardstick: the dense kernel, that many times, zero gradient
            T._lib.check(lib.tagrec_adam_f32(rp, zero, rm, rv, D, lr, b1, b2, eps, t, T._lib.stream_ptr()))
        ref[0][r], ref[1][r], ref[2][r] = rp, rm, rv
    listed = torch.zeros(n, dtype=torch.bool, device=DEV)
    listed[rows] = True
    for x in (p, m, v):
        x[~listed] = float("nan")
    plan = rowops.row_list_plan(rows, n, None, D)
    ring = _ring(lr, b1, b2, t_done, 310)                 # shorter than t_done: the ring has wrapped
    rowops.adam_catch_up(plan, p, m, v, last, ring, t_done - 300, t_done, (b1, b2), eps)
    for name, got, want in zip("pmv", (p, m, v), ref):
        assert bool(torch.isnan(got[~listed]).all()), f"{name}: a row outside the list was written"
        assert torch.equal(got[listed].contiguous().view(torch.int32), want[listed].view(torch.int32)), name
    assert bool((last == t_done).all())


@pytest.mark.parametrize("D,stride", ((64, 64), (8, 8), (20, 20), (32, 40)))
def test_apply_is_the_ordered_scatter_followed_by_adam(D, stride):
    n, t, lr, (b1, b2), eps = 97, 12, 0.01, (0.9, 0.999), 1e-8
    lib = T._lib.load()
    g = torch.Generator().manual_seed(2)
    rows = torch.cat([torch.randint(0, 30, (1500,), generator=g), torch.full((1300,), 50), torch.tensor([96, 0, 96])]).to(DEV)
    src = ((torch.rand(rows.numel(), stride, generator=g) - 0.5) * 0.1).to(DEV)[:, :D]
    p, m, v = _table(n, D, 4, stride)
    plan = rowops.row_list_plan(rows, n, None, D)
    grad = rowops.scatter_rows_ordered(torch.zeros(n, D, device=DEV), plan, src, True)
    ref = [x.contiguous().clone() for x in (p, m, v)]
    T._lib.check(lib.tagrec_adam_f32(ref[0], grad, ref[1], ref[2], n * D, lr, b1, b2, eps, t, T._lib.stream_ptr()))
    listed = torch.zeros(n, dtype=torch.bool, device=DEV)
    listed[rows] = True
    assert int(listed.sum()) < n
    for x in (p, m, v):
        x[~listed] = float("nan")
    last = torch.full((n,), t - 1, dtype=torch.int32, device=DEV)
    rowops.adam_apply_rows(plan, src, p, m, v, last, _ring(lr, b1, b2, t, 16), t, (b1, b2), eps)
    for name, got, want in zip("pmv", (p, m, v), ref):
        assert bool(torch.isnan(got[~listed]).all()), f"{name}: a row outside the list was written"
        assert torch.equal(got[listed].contiguous().view(torch.int32), want[listed].view(torch.int32)), name
    assert torch.equal(last == t, listed)


def test_flush_replays_the_lagging_rows_and_reads_no_others():
    n, D, t_done, lr, (b1, b2), eps = 70, 64, 9, 0.01, (0.9, 0.999), 1e-8
    lib = T._lib.load()
    p, m, v = _table(n, D, 6)
    last = (torch.arange(n, dtype=torch.int32) % 10).to(DEV)              # lags 9 .. 0
    m[7] = 0
    v[7] = 0
    ref = [x.clone() for x in (p, m, v)]
    zero = torch.zeros(D, dtype=torch.float32, device=DEV)
    for r in range(n):
        for t in range(int(last[r]) + 1, t_done + 1):
            T._lib.check(lib.tagrec_adam_f32(ref[0][r], zero, ref[1][r], ref[2][r], D, lr, b1, b2, eps, t, T._lib.stream_ptr()))
    current = last == t_done
    for x in (p, m, v):
        x[current] = float("nan")                                         # a current row costs its `last` only
    rowops.adam_flush(p, m, v, last, _ring(lr, b1, b2, t_done, 16), 0, t_done, (b1, b2), eps)
    for name, got, want in zip("pmv", (p, m, v), ref):
        assert bool(torch.isnan(got[current]).all()), name
        assert torch.equal(got[~current].view(torch.int32), want[~current].view(torch.int32)), name
    assert bool((last == t_done).all())


def test_wrappers_name_the_argument_they_refuse():
    p, m, v = _table(10, 8, 1)
    last = torch.zeros(10, dtype=torch.int32, device=DEV)
    ring = torch.zeros(16, 2, dtype=torch.float32, device=DEV)
    plan = rowops.row_list_plan(torch.tensor([1, 2], device=DEV), 10, None, 8)
    with pytest.raises(T.TagrecError, match="last"):
        rowops.adam_flush(p, m, v, last.long(), ring, 0, 1)
    with pytest.raises(T.TagrecError, match="ring"):
        rowops.adam_flush(p, m, v, last, ring[:, :1], 0, 1)
    with pytest.raises(T.TagrecError, match=" m "):
        rowops.adam_flush(p, m[:5], v, last, ring, 0, 1)
    with pytest.raises(T.TagrecError, match="t_floor"):
        rowops.adam_catch_up(plan, p, m, v, last, ring, 0, 17)
    with pytest.raises(T.TagrecError, match="src"):
        rowops.adam_apply_rows(plan, torch.zeros(3, 8, device=DEV), p, m, v, last, ring, 1)
    with pytest.raises(T.TagrecError, match="plan"):
        rowops.adam_catch_up(rowops.row_list_plan(torch.tensor([1], device=DEV), 11, None, 8), p, m, v, last, ring, 0, 1)


# ---- the step allocates nothing of the table's size ----

def test_no_table_sized_allocation_in_a_step():
    nu, ni, D, Bm = 120_000, 80_000, 64, 512
    ds = T.synth.make_bipartite_device(nu, ni, 600_000, 1, DEV)
    cfg = T.get_config("ultragcn", device=DEV, dim_latent=D, reg=1e-3, ug_neighbors=3, n_negatives=K)
    torch.manual_seed(1)
    model = T.UltraGCN(ds, config=cfg)
    opt = T.RowAdam(model.parameters(), lr=LR).attach(model)
    edges = ds.edge_index["train"]
    gen = torch.Generator(device=DEV).manual_seed(2)

    def batch():
        e = edges[torch.randint(0, edges.shape[0], (Bm,), device=DEV, generator=gen)]
        return torch.cat([e, torch.randint(0, ni, (Bm, K), device=DEV, generator=gen)], 1)

    model.train()
    for _ in range(3):
        _step(model, opt, batch())
    b = batch()
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats()
    before = torch.cuda.memory_allocated()
    _step(model, opt, b)
    torch.cuda.synchronize()
    table_bytes = model.table.numel() * 4
    extra = torch.cuda.max_memory_allocated() - before
    print(f"[row_adam] peak above the standing allocation: {extra / 2 ** 20:.2f} MiB (table {table_bytes / 2 ** 20:.1f} MiB)")
    assert table_bytes == 200_000 * 64 * 4 and extra < table_bytes / 4
    assert model.table.grad is None


# ---- against torch.optim.Adam on the fp64 restatement ----

def test_three_steps_track_torch_adam_on_the_fp64_restatement():
    nu, ni, K16 = 60, 50, 16
    ds = T.synth.make_cf_dataset(nu, ni, 600, seed=3)
    edges = np.asarray(ds.edge_index["train"], dtype=np.int64)
    nid, nw, _ = R.topk(edges, nu, ni, 10, False)
    nid, nw = torch.from_numpy(nid.astype(np.int64)), torch.from_numpy(nw)
    bu, bi = UT.betas64(edges, nu, ni)
    torch.manual_seed(7)
    m = T.UltraGCN(ds, config=T.get_config("ultragcn", device=DEV, dim_latent=64, reg=1e-3, n_negatives=K16))
    tab = m.table.detach().cpu().double()
    U, I = tab[:nu].clone().requires_grad_(), tab[nu:].clone().requires_grad_()
    opt, ropt = T.RowAdam(m.parameters(), lr=LR).attach(m), torch.optim.Adam([U, I], lr=LR)
    m.train()
    rng = np.random.RandomState(10)
    for _ in range(3):
        e = edges[rng.choice(len(edges), size=32, replace=False)]
        batch = torch.from_numpy(np.concatenate([e, rng.randint(0, ni, size=(32, K16))], 1).astype(np.int64))
        _step(m, opt, batch.to(DEV))
        ropt.zero_grad()
        rmul, rl2 = UT.ultragcn_loss64(U, I, batch, bu, bi, nid, nw)
        (rmul + 1e-3 * rl2).backward()
        ropt.step()
    got, want = torch.cat(m.forward()).detach().cpu().double(), torch.cat([U, I]).detach()
    print(f"[row_adam] three steps: max |dp| = {float((got - want).abs().max()):.2e}")
    np.testing.assert_allclose(got.numpy(), want.numpy(), atol=2e-4, rtol=0)
    assert float((got - tab).abs().max()) > 5e-3              # the steps moved the table


# ---- refusals ----

def test_refusals():
    ds, _ = _data()
    lcfg = T.get_config("lightgcn", device=DEV, use_tag=False, dim_layer_list=[64, 64])
    torch.manual_seed(1)
    lg = T.LightGCN(ds, config=lcfg)
    with pytest.raises(T.TagrecError, match="dense"):
        T.RowAdam(lg.parameters(), lr=LR).attach(lg)
    m = _model(64)
    with pytest.raises(T.TagrecError, match="capturable"):
        T.RowAdam(m.parameters(), lr=LR, capturable=True)
    with pytest.raises(T.TagrecError, match="max_lag"):
        T.RowAdam(m.parameters(), lr=LR, max_lag=0)
    with pytest.raises(T.TagrecError, match="fuse_into"):        # Adam.fuse_into(UltraGCN) raises as it always did
        T.Adam(m.parameters(), lr=LR).fuse_into(m)
    opt = T.RowAdam(m.parameters(), lr=LR).attach(m)
    for name, value in (("lr", 0.1), ("betas", (0.5, 0.9)), ("eps", 1e-6)):
        with pytest.raises(T.TagrecError, match=name):
            setattr(opt, name, value)
    assert opt.lr == LR
    b = _batches(40)[0]
    m.train()
    opt.zero_grad()
    sum(m.loss(b)).backward()
    with pytest.raises(T.TagrecError, match="second backward"):
        sum(m.loss(b)).backward()
    opt.step()
    with pytest.raises(T.TagrecError, match="capturable"):
        T.GraphedStep(m.loss, opt, b)
    # a newer optimizer over the table revokes the attachment: the model hands out dense gradients again
    opt2 = T.Adam(m.parameters(), lr=LR)
    _step(m, opt2, b)
    assert m.table.grad is not None
