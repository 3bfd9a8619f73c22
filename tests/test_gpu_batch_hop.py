"""The list-driven masked backward hop (csrc/batch_hop.hip: Graph.batch_hop_plan / Graph.batch_hop_normbwd) against the masked
row kernel it replaces in `lightgcn.restricted_backward` (Graph.spmm_normbwd_sparse with a row mask), and the restricted
training step built on it.

Bounds: rows of at most 1024 stored entries must come out bit for bit (the same fused multiply-adds in the same order).
Longer rows are summed in a different (fixed) order than the masked kernel's chunk partials; both are sums of at most T
terms, so the new path's error against an fp64 sum may exceed the masked kernel's by the factor two that a change of
order can cost, and no more.  (Measured on 73 rows of 5 k .. 100 k entries, D = 64: masked kernel 6.9e-9; a plain fp32
chain in ascending order 2.2e-8, which missed the bound -- the hop accumulates those rows in fp64 instead.)"""
import faulthandler

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import tagrec_amd as T
from tagrec_amd import lightgcn as LG
from tagrec_amd import rowops

DEV = torch.device("cuda:0")
NAN = float("nan")


@pytest.fixture(autouse=True)
def _per_test_timeout():
    """A hung kernel must end the run, not sit on the GPU: the process exits if one test takes longer than this."""
    faulthandler.dump_traceback_later(600, exit=True)
    yield
    faulthandler.cancel_dump_traceback_later()


def _hop_both(g, rows, D, seed, zero_dz=False):
    """The masked hop of A = g.transpose() on the batch list `rows`, by the masked row kernel and from the inverted list.
    Operand rows nobody may read hold NaN.  Returns (mid, tflag, old (out, flags), new (out, flags), new out on a NaN
    background, operands)."""
    n = g.shape[0]
    gt = g.transpose()
    gen = torch.Generator(device=DEV).manual_seed(seed)
    mid = g.mark_rows(rows, torch.zeros(n, dtype=torch.uint8, device=DEV))
    tflag = torch.zeros(n, dtype=torch.uint8, device=DEV)
    tflag.index_fill_(0, rows, 1)
    on = tflag.bool()
    g_in = torch.full((n, D), NAN, device=DEV)
    g_in[on] = torch.randn(int(on.sum()), D, device=DEV, generator=gen)
    x_raw = torch.full((n, D), NAN, device=DEV)
    x_raw[on] = torch.randn(int(on.sum()), D, device=DEV, generator=gen)
    inv = torch.full((n,), NAN, device=DEV)
    inv[on] = 1.0 / x_raw[on].norm(dim=1).clamp_min(1e-12)
    dz = torch.full((n, D), NAN, device=DEV)
    dz[on] = 0.0 if zero_dz else torch.randn(int(on.sum()), D, device=DEV, generator=gen)
    s = 0.25
    out_old, fo_old = torch.zeros(n, D, device=DEV), torch.zeros(n, dtype=torch.uint8, device=DEV)
    cnt = torch.zeros(1, dtype=torch.int32, device=DEV)
    gt.spmm_normbwd_sparse(g_in, tflag, None, x_raw, inv, dz, s, out_old, fo_old, cnt, row_mask=mid, dz_flags=tflag)
    src = gt.transpose()
    cap = src.batch_hop_capacity(rows.numel())
    buf = torch.full((src.batch_hop_workspace(rows.numel(), cap),), 0xFF, dtype=torch.uint8, device=DEV)   # poisoned scratch
    plan = src.batch_hop_plan(rows, cap, buf)
    out_new, fo_new = torch.zeros(n, D, device=DEV), torch.zeros(n, dtype=torch.uint8, device=DEV)
    gt.batch_hop_normbwd(plan, g_in, x_raw, inv, dz, s, out_new, fo_new, mid, tflag)
    out_nan = torch.full((n, D), NAN, device=DEV)
    gt.batch_hop_normbwd(plan, g_in, x_raw, inv, dz, s, out_nan, torch.zeros_like(fo_new), mid, tflag)
    src.batch_hop_check()
    return mid, tflag, (out_old, fo_old), (out_new, fo_new), out_nan, (g_in, gt)


@pytest.mark.parametrize("D", [8, 16, 32, 64, 128, 256])
def test_list_hop_is_bit_identical_on_short_rows(D):
    """Random square (non-symmetric) graph, no row or column above 1024 entries; the batch list repeats nodes and holds a
    node without any entry and a node whose single neighbour has no other entry."""
    n = 6000
    gen = torch.Generator(device=DEV).manual_seed(11 + D)
    r = torch.randint(0, n, (200_000,), device=DEV, generator=gen)
    c = torch.randint(0, n, (200_000,), device=DEV, generator=gen)
    z, p, q = 17, 23, 29                                   # z: isolated; p: one entry (p, q); q: nothing but that entry
    keep = torch.ones_like(r, dtype=torch.bool)
    for v in (z, p, q):
        keep &= (r != v) & (c != v)
    r = torch.cat([r[keep], torch.tensor([p], device=DEV)])
    c = torch.cat([c[keep], torch.tensor([q], device=DEV)])
    v = torch.rand(r.numel(), device=DEV, generator=gen) + 0.1
    rp, col, val = T.graph.coalesce_device(r, c, v, n, n)
    g = T.Graph(rp, col, val, (n, n))
    gt = g.transpose()
    assert int((rp[1:] - rp[:-1]).max()) <= 1024 and int((gt.rowptr[1:] - gt.rowptr[:-1]).max()) <= 1024
    some = torch.randint(0, n, (150,), device=DEV, generator=gen)
    rows = torch.cat([some, some[:60], torch.tensor([z, p, z], device=DEV)])          # repeats, the isolated node twice
    mid, tflag, (o0, f0), (o1, f1), o_nan, _ = _hop_both(g, rows, D, seed=D)
    assert int(mid.sum()) > 1000 and bool(mid[q]) and bool(f1[q])
    assert torch.equal(f1, f0)
    m = mid.bool()
    assert torch.equal(o1[m], o0[m])                       # (rows without a record or a dz term: zero in both, as the caller left them)
    wrote = f1.bool() | tflag.bool()
    assert torch.equal(o_nan[wrote], o0[wrote]) and bool(torch.isnan(o_nan[~wrote]).all())
    assert bool((o1[~m] == 0).all())


def test_list_hop_long_rows_against_fp64():
    """Rows of 5 k .. 100 k entries inside the mask (popular items next to a batch user): the masked kernel sums them through
    chunk partials, the list hop in ascending source order.  Both against the fp64 sum of the same terms."""
    ds = T.synth.make_bipartite_device(60_000, 3_000, 3_000_000, seed=5, device=DEV)
    e = ds.edge_index["train"]
    rp, col, val, n = T.graph.bipartite_norm_device(e[:, 0], e[:, 1], 60_000, 3_000, "bi_norm")
    g = T.Graph(rp, col, val, (n, n), symmetric=True)
    cfg = T.get_config("lightgcn", use_tag=False, device=DEV, train_batch=512)
    batch = T.BPR_training_data(ds, config=cfg, seed=2).all_train_data[:512].to(DEV)
    rows = rowops.batch_rows(batch, 60_000)
    D = 64
    mid, tflag, (o0, f0), (o1, f1), _, (g_in, gt) = _hop_both(g, rows, D, seed=3, zero_dz=True)
    deg = rp[1:] - rp[:-1]
    long_rows = torch.nonzero((deg >= 5000) & mid.bool()).flatten().tolist()
    assert len(long_rows) >= 3
    err_old = err_new = 0.0
    for j in long_rows:
        cols = col[rp[j]:rp[j + 1]].long()
        sel = tflag[cols].bool()
        ref = (val[rp[j]:rp[j + 1]][sel].double()[:, None] * g_in[cols[sel]].double()).sum(0)
        err_old = max(err_old, float((o0[j].double() - ref).abs().max()))
        err_new = max(err_new, float((o1[j].double() - ref).abs().max()))
    print(f"long rows: {len(long_rows)}, max error vs fp64: masked kernel {err_old:.3e}, list hop {err_new:.3e}")
    assert err_new <= 2.0 * err_old, f"max error vs fp64 on {len(long_rows)} long rows: masked kernel {err_old:.3e}, list hop {err_new:.3e}"
    assert torch.equal(f1, f0)
    short = mid.bool() & (deg <= 1024)
    assert torch.equal(o1[short], o0[short])


def _step_setup(seed=7):
    ds = T.synth.make_bipartite_device(50_000, 100_000, 1_500_000, seed=seed, device=DEV)
    e = ds.edge_index["train"]
    rp, col, val, n = T.graph.bipartite_norm_device(e[:, 0], e[:, 1], 50_000, 100_000, "bi_norm")
    g = T.Graph(rp, col, val, (n, n), symmetric=True)
    cfg = T.get_config("lightgcn", use_tag=False, dim_latent=64, dim_layer_list=[64, 64, 64], device=DEV, train_batch=128)
    data = T.BPR_training_data(ds, config=cfg, seed=1).all_train_data.to(DEV)
    return ds, g, cfg, data


def _model(ds, g, cfg, fuse, capturable=False):
    torch.manual_seed(3)
    m = T.LightGCN(ds, config=cfg, graph=g)
    m.train()
    opt = T.Adam(m.parameters(), lr=0.01, capturable=capturable)
    if fuse:
        opt.fuse_into(m)
    return m, opt


def _one_step(m, opt, batch):
    lossx = m.loss(batch)
    opt.zero_grad()
    sum(lossx).backward()
    opt.step()
    return torch.stack([v.detach() for v in lossx])


def _adam_state(m, opt):
    return [opt.state[id(p)][k].clone() for p in m.parameters() for k in ("m", "v")]


def _distinct_triples(data, k):
    """k triplets that share no user and no item (host-side pick from the head of the epoch)."""
    seen_u, seen_i, keep = set(), set(), []
    for idx, (u, p, q) in enumerate(data[:20_000].tolist()):
        if u in seen_u or p in seen_i or q in seen_i or p == q:
            continue
        seen_u.add(u); seen_i.update((p, q)); keep.append(idx)
        if len(keep) == k:
            break
    assert len(keep) == k
    return data[torch.tensor(keep, device=data.device)]


@pytest.mark.parametrize("fuse", [True, False])
def test_restricted_step_is_deterministic_with_repeated_batch_nodes(fuse):
    """Every batch node is listed exactly twice.  (The step scatters the batch rows' gradients with torch's index_add_, whose
    float atomics commute for two addends; a node listed three times or more gets an unordered fp32 sum there, before and
    after this hop -- that is not what this test is about.)"""
    ds, g, cfg, data = _step_setup()
    half = _distinct_triples(data, 64)
    batch = torch.cat([half, half])
    second = _distinct_triples(data[30_000:], 128)
    res = []
    for _ in range(2):
        m, opt = _model(ds, g, cfg, fuse)
        losses = [_one_step(m, opt, batch), _one_step(m, opt, second)]
        assert "hop_plan" in m.step_ws._buf, "the step did not take the list-driven hop"
        res.append((torch.stack(losses), m.table.detach().clone(), _adam_state(m, opt)))
        g.batch_hop_check()
    (l0, t0, a0), (l1, t1, a1) = res
    assert torch.equal(l0, l1) and torch.equal(t0, t1)
    for x, y in zip(a0, a1):
        assert torch.equal(x, y)
    # and against the masked row kernel: same loss, a table within the spread of a changed summation order on long rows
    LG.BATCH_HOP_LIST = False
    try:
        m, opt = _model(ds, g, cfg, fuse)
        l2 = torch.stack([_one_step(m, opt, batch), _one_step(m, opt, second)])
    finally:
        LG.BATCH_HOP_LIST = True
    np.testing.assert_allclose(l2.cpu().numpy(), l0.cpu().numpy(), rtol=1e-6)
    diff = (m.table.detach() - t0).abs()
    assert float((diff <= 2e-4).float().mean()) >= 0.999       # (Adam turns a last-bit difference of a near-zero gradient into lr)


def test_poisoned_workspace_changes_nothing():
    """Every buffer of the step workspace -- the hop plan included -- is filled with NaN (0xFF bytes for the integer ones)
    before the step: rows a kernel leaves unwritten are never read, so loss and table equal the clean run's."""
    ds, g, cfg, data = _step_setup()
    out = []
    for poison in (False, True):
        m, opt = _model(ds, g, cfg, True)
        _one_step(m, opt, _distinct_triples(data, 128))    # creates the buffers (repeat-free batches: see the test above)
        assert "hop_plan" in m.step_ws._buf
        if poison:
            for t in m.step_ws._buf.values():
                t.fill_(NAN) if t.is_floating_point() else t.view(torch.uint8).fill_(0xFF)
        loss = _one_step(m, opt, _distinct_triples(data[30_000:], 128))
        g.batch_hop_check()
        out.append((loss, m.table.detach().clone()))
    assert bool(torch.isfinite(out[1][0]).all()) and bool(torch.isfinite(out[1][1]).all())
    assert torch.equal(out[1][0], out[0][0]) and torch.equal(out[1][1], out[0][1])


def test_graphed_step_equals_eager_steps():
    ds, g, cfg, data = _step_setup()
    batches = [_distinct_triples(data[k * 30_000:], 128) for k in range(5)]     # (repeat-free: see the determinism test)
    m0, opt0 = _model(ds, g, cfg, True, capturable=True)
    eager = [_one_step(m0, opt0, b) for b in batches]
    m1, opt1 = _model(ds, g, cfg, True, capturable=True)
    for b in batches[:2]:
        _one_step(m1, opt1, b)
    gstep = T.GraphedStep(m1.loss, opt1, batches[2])
    got = [gstep(b) for b in batches[2:]]
    torch.cuda.synchronize()
    assert "hop_plan" in m1.step_ws._buf
    g.batch_hop_check()
    for a, b in zip(got, eager[2:]):
        assert torch.equal(a, b)
    assert torch.equal(m1.table.detach(), m0.table.detach())
