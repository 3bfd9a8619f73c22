"""The row-list plan and the ordered scatter of csrc/rowscatter.hip, bit for bit against the numpy restatement of their order
contract (rowscatter_ref.py): `array_equal`, no tolerance.

The values are randn * 10^U(-3, 3), so an fp32 sum taken in another order differs in its last bits; before a case touches the
GPU it asserts on the CPU that the reference evaluated in DESCENDING slot order differs from the contract's order (for the
cases that name a row three times or more: two addends commute)."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import tagrec_amd as T
from tagrec_amd import rowops
from rowscatter_ref import make_values, scatter_ref, segments, zipf_rows

DEV = torch.device("cuda:0")
NAN = float("nan")


def _repeat(k, n=16, hot=7):
    """Row `hot` named k times, rows 0 and n - 1 named three times each in between."""
    rows = np.full(k + 6, hot, dtype=np.int64)
    rows[[0, k // 2, k + 5]] = 0
    rows[[1, k // 3, k + 4]] = n - 1
    return rows, n


def _small(T_, n=16, seed=0):
    rng = np.random.default_rng(100 + T_ + seed)
    rows = rng.integers(0, n, T_).astype(np.int64)
    rows[0] = n - 1
    if T_ > 1:
        rows[-1] = 0
    return rows, n


CASES = {
    "t1": lambda: _small(1),
    "t63": lambda: _small(63),
    "t64": lambda: _small(64),
    "t65": lambda: _small(65),
    "zipf1536": lambda: (zipf_rows(np.random.default_rng(5), 1536, 300), 300),
    "distinct": lambda: (np.random.default_rng(6).permutation(128)[:100].astype(np.int64), 128),
    "rep1023": lambda: _repeat(1023),
    "rep1024": lambda: _repeat(1024),
    "rep1025": lambda: _repeat(1025),
    "rep2049": lambda: _repeat(2049),
}


@pytest.fixture(scope="module")
def plans():
    """One device plan per case, shared by the tests (built with the widest tested row)."""
    cache = {}

    def get(name):
        if name not in cache:
            rows, n = CASES[name]()
            cache[name] = (rows, n, rowops.row_list_plan(torch.from_numpy(rows).to(DEV), n, width=264))
        return cache[name]
    return get


@pytest.mark.parametrize("D", [8, 64, 256, 20])
@pytest.mark.parametrize("case", list(CASES))
def test_scatter_equals_the_order_contract(plans, case, D):
    rows, n, plan = plans(case)
    T_ = len(rows)
    rng = np.random.default_rng(D * 1000 + T_)
    src = make_values(rng, T_, D)
    base = make_values(rng, n, D)
    named = np.zeros(n, dtype=bool)
    named[rows] = True
    want = {acc: scatter_ref(rows, n, src, base, acc) for acc in (False, True)}
    if max(len(s) for _, s in segments(rows, n)) >= 3:        # the test is not blind: another order gives other bits
        assert not np.array_equal(scatter_ref(rows, n, src, base, False, descending=True), want[False])
    for pad_s, pad_d in ((0, 0), (4, 8), (1, 3)):             # (1, 3): rows off 16-byte alignment -> the one-lane-per-column form
        for acc in (False, True):
            s_buf = torch.full((T_, D + pad_s), NAN, device=DEV)
            s_buf[:, :D] = torch.from_numpy(src).to(DEV)
            d_buf = torch.full((n, D + pad_d), NAN, device=DEV)
            d_buf[:, :D] = torch.from_numpy(base).to(DEV)
            d_buf[torch.from_numpy(~named).to(DEV)] = NAN      # rows the list does not name: poisoned, must stay NaN
            out = rowops.scatter_rows_ordered(d_buf[:, :D], plan, s_buf[:, :D], acc)
            got = out.cpu().numpy()
            what = f"{case} D={D} pad=({pad_s},{pad_d}) accumulate={acc}"
            assert np.array_equal(got[named], want[acc][named]), what
            assert np.isnan(got[~named]).all(), what
            assert np.isnan(d_buf[:, D:].cpu().numpy()).all(), what       # nothing written past a row's D columns


@pytest.mark.parametrize("case", list(CASES))
def test_plan_is_the_stable_sort(plans, case):
    rows, n, plan = plans(case)
    r = torch.from_numpy(rows).to(DEV)
    srt, idx = torch.sort(r, stable=True)
    assert plan.order.dtype == torch.int32 and torch.equal(plan.order.long(), idx)
    uniq, counts = torch.unique_consecutive(srt, return_counts=True)
    seg_row, seg_ptr = plan.segments()
    assert torch.equal(seg_row.long(), uniq)
    assert torch.equal(seg_ptr.long(), torch.cat([torch.zeros(1, dtype=torch.int64, device=DEV), counts.cumsum(0)]))
    assert plan.counts.tolist()[:3] == [len(uniq), len(rows), 0] and plan.dropped() == 0


def test_out_of_range_ids_are_counted_and_dropped():
    n, D = 16, 64
    rng = np.random.default_rng(9)
    rows = rng.integers(0, n, 70).astype(np.int64)
    rows[[3, 40, 69]] = [-1, n, 1 << 40]
    plan = rowops.row_list_plan(torch.from_numpy(rows).to(DEV), n, width=D)
    assert plan.dropped() == 3 and plan.counts.tolist()[1] == 67
    seg_row, _ = plan.segments()
    assert seg_row.tolist() == sorted(set(rows[(rows >= 0) & (rows < n)].tolist()))
    src, base = make_values(rng, 70, D), make_values(rng, n, D)
    for acc in (False, True):
        out = rowops.scatter_rows_ordered(torch.from_numpy(base).to(DEV), plan, torch.from_numpy(src).to(DEV), acc)
        assert np.array_equal(out.cpu().numpy(), scatter_ref(rows, n, src, base, acc))
    # nothing valid at all: no segment, nothing written
    plan = rowops.row_list_plan(torch.full((5,), n, dtype=torch.int64, device=DEV), n, width=D)
    assert plan.counts.tolist()[:3] == [0, 0, 5]
    dst = torch.full((n, D), NAN, device=DEV)
    rowops.scatter_rows_ordered(dst, plan, torch.ones(5, D, device=DEV), False)
    assert bool(torch.isnan(dst).all())


def test_workspace_reuse_and_argument_checks():
    n, D = 40, 32
    rows = torch.from_numpy(zipf_rows(np.random.default_rng(1), 90, n)).to(DEV)
    ws = torch.empty(rowops.row_list_workspace(90, D), dtype=torch.uint8, device=DEV)
    plan = rowops.row_list_plan(rows, n, ws, D)
    assert plan.workspace is ws and plan.order.data_ptr() >= ws.data_ptr()
    src = torch.randn(90, D, device=DEV)
    a = rowops.scatter_rows_ordered(torch.zeros(n, D, device=DEV), plan, src, False)
    ws.fill_(0xFF)                                            # a re-planned workspace carries nothing over
    plan = rowops.row_list_plan(rows, n, ws, D)
    assert torch.equal(rowops.scatter_rows_ordered(torch.zeros(n, D, device=DEV), plan, src, False), a)
    with pytest.raises(T.TagrecError):
        rowops.row_list_plan(rows, n, ws[:64], D)                                        # workspace too small
    with pytest.raises(T.TagrecError):
        rowops.scatter_rows_ordered(torch.zeros(n, 64, device=DEV), plan, torch.randn(90, 64, device=DEV), False)   # wider than planned
    with pytest.raises(T.TagrecError):
        rowops.scatter_rows_ordered(torch.zeros(n - 1, D, device=DEV), plan, src, False)  # fewer rows than the plan's table
    with pytest.raises(T.TagrecError):
        rowops.scatter_rows_ordered(torch.zeros(n, D, device=DEV), plan, src[:50], False)  # not one row per slot
    both = torch.zeros(n + 90, D, device=DEV)
    with pytest.raises(T.TagrecError):
        rowops.scatter_rows_ordered(both[:n + 10], plan, both[n:], False)                 # src and dst overlap
