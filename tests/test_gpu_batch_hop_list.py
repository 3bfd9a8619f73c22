"""The list-driven hop's own plan (csrc/batch_hop.hip): the destination list the hop strides over, the balanced walk that
builds the records, the capacity bounds, and plan + hop under HIP-graph replay.  The yardstick throughout is the masked row
kernel (`Graph.spmm_normbwd_sparse` with a row mask), which the hop must reproduce bit for bit on rows of at most 1024
stored entries (`tests/test_gpu_batch_hop.py` holds the long-row bound)."""
import faulthandler

import pytest
import torch

pytestmark = pytest.mark.gpu

import tagrec_amd as T

DEV = torch.device("cuda:0")
NAN = float("nan")
LONG_ROW = 1024          # kLongRow of csrc/graph.h


@pytest.fixture(autouse=True)
def _per_test_timeout():
    """A hung kernel must end the run, not sit on the GPU: the process exits if one test takes longer than this."""
    faulthandler.dump_traceback_later(600, exit=True)
    yield
    faulthandler.cancel_dump_traceback_later()


def _operands(n, rows, D, seed):
    """Operands of the hop for the batch list `rows`: NaN wherever nobody may read."""
    gen = torch.Generator(device=DEV).manual_seed(seed)
    tflag = torch.zeros(n, dtype=torch.uint8, device=DEV)
    tflag.index_fill_(0, rows, 1)
    on = tflag.bool()
    k = int(on.sum())
    g_in, x_raw, dz = (torch.full((n, D), NAN, device=DEV) for _ in range(3))
    g_in[on] = torch.randn(k, D, device=DEV, generator=gen)
    x_raw[on] = torch.randn(k, D, device=DEV, generator=gen)
    dz[on] = torch.randn(k, D, device=DEV, generator=gen)
    inv = torch.full((n,), NAN, device=DEV)
    inv[on] = 1.0 / x_raw[on].norm(dim=1).clamp_min(1e-12)
    return tflag, g_in, x_raw, inv, dz


def _masked(gt, mid, ops, s=0.25):
    """The parent algorithm: the masked row kernel on a zero background.  Returns (out, flags)."""
    tflag, g_in, x_raw, inv, dz = ops
    n, D = g_in.shape
    out, fo = torch.zeros(n, D, device=DEV), torch.zeros(n, dtype=torch.uint8, device=DEV)
    cnt = torch.zeros(1, dtype=torch.int32, device=DEV)
    gt.spmm_normbwd_sparse(g_in, tflag, None, x_raw, inv, dz, s, out, fo, cnt, row_mask=mid, dz_flags=tflag)
    return out, fo


def _listed(g, gt, rows, mid, ops, s=0.25):
    """Plan (in a poisoned buffer) + hop on a NaN background.  Returns (out, flags, the plan's row list)."""
    tflag, g_in, x_raw, inv, dz = ops
    n, D = g_in.shape
    cap = g.batch_hop_capacity(rows.numel())
    buf = torch.full((g.batch_hop_workspace(rows.numel(), cap),), 0xFF, dtype=torch.uint8, device=DEV)
    plan = g.batch_hop_plan(rows, cap, buf)
    out, fo = torch.full((n, D), NAN, device=DEV), torch.zeros(n, dtype=torch.uint8, device=DEV)
    gt.batch_hop_normbwd(plan, g_in, x_raw, inv, dz, s, out, fo, mid, tflag)
    g.batch_hop_check()
    return out, fo, g.batch_hop_rows(plan).long()


def _random_graph(n, nnz, seed, special=()):
    """Random square non-symmetric graph; `special` = (z, p, q): z isolated, p's only entry is (p, q), q has nothing else."""
    gen = torch.Generator(device=DEV).manual_seed(seed)
    r = torch.randint(0, n, (nnz,), device=DEV, generator=gen)
    c = torch.randint(0, n, (nnz,), device=DEV, generator=gen)
    if special:
        z, p, q = special
        keep = torch.ones_like(r, dtype=torch.bool)
        for v in special:
            keep &= (r != v) & (c != v)
        r = torch.cat([r[keep], torch.tensor([p], device=DEV)])
        c = torch.cat([c[keep], torch.tensor([q], device=DEV)])
    v = torch.rand(r.numel(), device=DEV, generator=gen) + 0.1
    rp, col, val = T.graph.coalesce_device(r, c, v, n, n)
    return T.Graph(rp, col, val, (n, n)), gen


@pytest.fixture(scope="module")
def small():
    z, p, q = 17, 23, 29
    g, gen = _random_graph(6000, 200_000, 41, (z, p, q))
    some = torch.randint(0, 6000, (150,), device=DEV, generator=gen)
    return g, g.transpose(), some, (z, p, q)


def _check_destinations(g, gt, rows, D, seed):
    n = g.shape[0]
    mid = g.mark_rows(rows, torch.zeros(n, dtype=torch.uint8, device=DEV))
    ops = _operands(n, rows, D, seed)
    o_old, f_old = _masked(gt, mid, ops)
    o_new, f_new, dest = _listed(g, gt, rows, mid, ops)
    want = f_old.bool() | ops[0].bool()                    # the rows the masked kernel writes: a record or a batch row
    seen = torch.bincount(dest, minlength=n)
    assert int(seen.max()) == 1, "a row is listed twice"
    assert torch.equal(seen.bool(), want), "the list is not the set of rows the masked kernel writes"
    assert bool(torch.isnan(o_new[~want]).all()) and not bool(torch.isnan(o_new[want]).any())
    deg = gt.rowptr[1:] - gt.rowptr[:-1]
    short = want & (deg <= LONG_ROW)
    assert torch.equal(o_new[short], o_old[short]) and torch.equal(f_new, f_old)
    return dest


@pytest.mark.parametrize("case", ["one", "repeated", "isolated", "lonely_neighbour", "mixed"])
def test_destination_list_is_the_set_the_masked_kernel_writes(small, case):
    g, gt, some, (z, p, q) = small
    rows = {"one": some[:1],
            "repeated": torch.cat([some, some]),
            "isolated": torch.tensor([z], device=DEV),
            "lonely_neighbour": torch.tensor([p], device=DEV),
            "mixed": torch.cat([some, some[:60], torch.tensor([z, p, z], device=DEV)])}[case]
    dest = _check_destinations(g, gt, rows, 64, seed=3)
    if case == "isolated":
        assert dest.tolist() == [z]                        # no record, but the batch row's epilogue term
    if case == "lonely_neighbour":
        assert sorted(dest.tolist()) == [p, q]


@pytest.mark.parametrize("D", [16, 64])
def test_destination_list_longer_than_one_pass_of_the_grid(D):
    """16 384 listed rows of a 300 000-node graph: more destinations than the hop's grid takes in one pass."""
    n = 300_000
    g, gen = _random_graph(n, 3_000_000, 43)
    rows = torch.randint(0, n, (16_384,), device=DEV, generator=gen)
    per_pass = T.Graph.batch_hop_grid_rows(D)
    assert per_pass > 0
    dest = _check_destinations(g, g.transpose(), rows, D, seed=5)
    assert dest.numel() > per_pass, f"{dest.numel()} destinations do not outnumber one pass of {per_pass}"


@pytest.fixture(scope="module")
def skewed():
    """The bipartite graph of the long-row test (60 000 x 3 000, 3 M edges) and a list of 400 nodes whose row lengths run
    from 1 to the longest row of the graph (43 k entries: the items' degrees stop there), so the walk's fixed-size blocks
    cut inside rows and span many rows."""
    ds = T.synth.make_bipartite_device(60_000, 3_000, 3_000_000, seed=5, device=DEV)
    e = ds.edge_index["train"]
    rp, col, val, n = T.graph.bipartite_norm_device(e[:, 0], e[:, 1], 60_000, 3_000, "bi_norm")
    g = T.Graph(rp, col, val, (n, n), symmetric=True)
    deg = rp[1:] - rp[:-1]
    order = torch.argsort(deg)
    order = order[deg[order] > 0]
    pick = torch.linspace(0, order.numel() - 1, 300, device=DEV).long()
    rows = torch.cat([order[pick], order[-100:], order[:1]])            # a spread, the 100 longest rows, the shortest again
    dl = deg[rows]
    assert int(dl.min()) == 1 and int(dl.max()) >= 40_000 and int(dl.max()) == int(deg.max())
    return g, rows[torch.randperm(rows.numel(), device=DEV, generator=torch.Generator(device=DEV).manual_seed(1))]


@pytest.mark.parametrize("D", [16, 64])
def test_plan_contract_on_skewed_row_lengths(skewed, D):
    g, rows = skewed
    n = g.shape[0]
    gt = g.transpose()
    mid = g.mark_rows(rows, torch.zeros(n, dtype=torch.uint8, device=DEV))
    ops = _operands(n, rows, D, seed=7 + D)
    o_old, f_old = _masked(gt, mid, ops)
    o_new, f_new, dest = _listed(g, gt, rows, mid, ops)
    assert torch.equal(f_new, f_old)
    deg = gt.rowptr[1:] - gt.rowptr[:-1]
    wrote = f_old.bool() | ops[0].bool()
    short = wrote & (deg <= LONG_ROW)
    assert int(short.sum()) > 10_000 and int((wrote & ~short).sum()) >= 3
    assert torch.equal(o_new[short], o_old[short])
    assert bool(torch.isnan(o_new[~wrote]).all()) and not bool(torch.isnan(o_new[wrote]).any())
    assert int(torch.bincount(dest, minlength=n).max()) == 1


def test_overflow_is_reported_and_stays_inside_the_workspace(small):
    g, gt, some, _ = small
    rows = torch.cat([some, some[:40]])
    deg = g.rowptr[1:] - g.rowptr[:-1]
    records = int(deg[torch.unique(rows)].sum())
    GUARD = 4096
    for cap, overflows in ((records, False), (records - 1, True)):
        declared = g.batch_hop_workspace(rows.numel(), cap)
        buf = torch.full((declared + GUARD,), 0xFF, dtype=torch.uint8, device=DEV)
        buf[declared:] = 0xA5
        # (the wrapper hands the library the buffer from its first 256-byte boundary on; `declared` includes that slack)
        plan = g.batch_hop_plan(rows, cap, buf[:declared])
        torch.cuda.synchronize()
        assert bool((buf[declared:] == 0xA5).all()), "the plan wrote past its workspace"
        if overflows:
            with pytest.raises(T.TagrecError, match="record capacity exceeded"):
                g.batch_hop_check()
        else:
            g.batch_hop_check()
            assert g.batch_hop_rows(plan).numel() > 0
    g.batch_hop_check()                                    # (the check cleared the error)
    cap = g.batch_hop_capacity(3)
    buf = torch.full((g.batch_hop_workspace(3, cap),), 0xFF, dtype=torch.uint8, device=DEV)
    for bad in (g.shape[0], -1):
        g.batch_hop_plan(torch.tensor([5, bad, 7], device=DEV), cap, buf)
        with pytest.raises(T.TagrecError, match="row id outside the matrix"):
            g.batch_hop_check()


def test_captured_plan_and_hop_replay_with_other_lists(small):
    """Plan + hop captured once as a HIP graph, replayed with three other batch lists of the same length: the list's length
    and the hop's trip count live in device memory, so every replay equals the eager run of its own list."""
    g, gt, _, _ = small
    n, D, T_ = g.shape[0], 64, 200
    gen = torch.Generator(device=DEV).manual_seed(9)
    lists = [torch.randint(0, n, (T_,), device=DEV, generator=gen) for _ in range(4)]
    lists[2] = torch.cat([lists[2][:100], lists[2][:100]])                # one list names every node twice
    cap = g.batch_hop_capacity(T_)
    buf = torch.full((g.batch_hop_workspace(T_, cap),), 0xFF, dtype=torch.uint8, device=DEV)
    rows_s = lists[0].clone()
    mid_s = torch.zeros(n, dtype=torch.uint8, device=DEV)
    ops_s = [t.clone() for t in _operands(n, lists[0], D, 0)]
    out_s, fo_s = torch.full((n, D), NAN, device=DEV), torch.zeros(n, dtype=torch.uint8, device=DEV)

    def run():
        tflag, g_in, x_raw, inv, dz = ops_s
        out_s.fill_(NAN)
        fo_s.zero_()
        plan = g.batch_hop_plan(rows_s, cap, buf)
        gt.batch_hop_normbwd(plan, g_in, x_raw, inv, dz, 0.25, out_s, fo_s, mid_s, tflag)

    def load(k):
        rows_s.copy_(lists[k])
        mid_s.copy_(g.mark_rows(lists[k], torch.zeros(n, dtype=torch.uint8, device=DEV)))
        for dst, src in zip(ops_s, _operands(n, lists[k], D, k)):
            dst.copy_(src)

    load(0)
    run()                                                  # eager once: creates the error word and the capacity cache
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        run()
    for k in (1, 2, 3):
        load(k)
        graph.replay()
        got = (out_s.clone(), fo_s.clone())
        run()
        torch.cuda.synchronize()
        assert torch.equal(got[1], fo_s)
        assert torch.equal(got[0].view(torch.int32), out_s.view(torch.int32))      # bits, NaN background included
        o_old, f_old = _masked(gt, mid_s, ops_s)
        wrote = f_old.bool() | ops_s[0].bool()
        assert torch.equal(got[0][wrote], o_old[wrote]) and bool(torch.isnan(got[0][~wrote]).all())
    g.batch_hop_check()


@pytest.mark.parametrize("D", T.rowops.VEC_WIDTHS)
def test_layer_mean_rows_has_the_bits_of_the_torch_sequence(D):
    """`rowops.layer_mean_rows` (one launch) against what `restricted_forward` ran before it: index_select, `* s`, addcmul_ per
    stored layer, add_(alpha) and the ego gather -- bit for bit, NaN background where no row is read.  s = 1 / (L + 1)
    covers a power of two and 1/3 (where a differently contracted multiply-add would show)."""
    n = 5000
    gen = torch.Generator(device=DEV).manual_seed(100 + D)
    for n_rows in (1, 3, 1537):
        rows = torch.randint(0, n, (n_rows,), device=DEV, generator=gen)
        rows[0] = n - 1
        if n_rows > 1:
            rows[1] = 0
            rows[-1] = rows[0]                             # a repeated node
        on = torch.zeros(n, dtype=torch.bool, device=DEV)
        on[rows] = True
        for L in (1, 2, 3):
            s = 1.0 / (L + 1)
            x0 = torch.randn(n, D, device=DEV, generator=gen)
            raws, invs = [], []
            for _ in range(L - 1):
                y = torch.full((n, D), NAN, device=DEV)
                y[on] = torch.randn(int(on.sum()), D, device=DEV, generator=gen)
                inv = torch.full((n,), NAN, device=DEV)
                inv[on] = 1.0 / y[on].norm(dim=1).clamp_min(1e-12)
                raws.append(y)
                invs.append(inv)
            z_top = torch.randn(n_rows, D, device=DEV, generator=gen)
            want = x0.index_select(0, rows) * s
            for y, inv in zip(raws, invs):
                want.addcmul_(y.index_select(0, rows), inv.index_select(0, rows)[:, None], value=s)
            want.add_(z_top, alpha=s)
            out_b, ego_b = T.rowops.layer_mean_rows(x0, rows, raws, invs, z_top, s)
            assert torch.equal(out_b, want), (n_rows, L)
            assert torch.equal(ego_b, x0.index_select(0, rows))
            assert T.rowops.layer_mean_rows(x0, rows, raws, invs, z_top, s, want_ego=False)[1] is None
