"""CPU-only: the restatement of the batch hop in tests/batch_hop_ref.py against a dense fp64 product, torch autograd in fp64,
spmm_ref.mark_rows and exact rationals -- what makes it independent of the kernels it judges in
test_gpu_batch_hop_kernels.py -- and the conditions of the hop-ladder fixture, as facts about the inputs."""
from fractions import Fraction

import numpy as np
import pytest
import torch

import batch_hop_ref as H
import spmm_ref as R

WIDTHS = (8, 16, 32, 64, 128, 256)         # rowops.VEC_WIDTHS (the GPU test takes them from the package)
WALK_BLOCKS = 256                          # kWalkBlocks of csrc/batch_hop.hip


def test_the_ladder_is_what_the_gpu_test_relies_on():
    lad, n = H.ladder(), H.N
    assert n == 4 * H.BUCKET + 301 and 0.9e5 < len(lad.col) < 1.4e5
    rows_of = np.repeat(np.arange(n), lad.deg)
    assert len(np.unique(rows_of * n + lad.col)) == len(lad.col)                       # no duplicate column ids
    assert (np.diff(lad.col)[np.diff(rows_of) == 0] > 0).all()                         # ascending inside a row
    assert (lad.val != 0).all() and (lad.val < 0).any() and (lad.val > 0).any()
    plan = H.plan_of("core")
    in_core = np.isin(lad.col, plan.leaders)
    for name, r in lad.special.items():
        # (the hub stores every id that any row stores but 38: the 1102 core ids among them)
        deg, rec = name[1:].split("_")[0].split("r") if name != "hub" else (n - 50, 1102)
        assert lad.deg[r] == int(deg), name
        assert plan.nrec[r] == (lad.deg[r] if rec == "all" else int(rec)) == in_core[rows_of == r].sum(), name
    assert {2047, 2048, 4095, 4096, 8191, 8192, n - 1} <= set(lad.special.values())
    rec_counts = {int(plan.nrec[r]) for r in lad.special.values()}
    assert {0, 1, 3, 4, 5, 8, 65, 1024, 1025} <= rec_counts
    assert {int(lad.deg[r]) for r in lad.special.values()} == {0, 1, 2, 3, 4, 5, 63, 64, 65, 1023, 1024, 1025, 2049, n - 50}
    one, big = lad.special["d2049r1"], lad.special["d1025rall"]
    assert plan.long[one] and plan.nrec[one] == 1                                      # a long row with exactly one record
    assert plan.long[big] and plan.nrec[big] == 1025 and plan.long[n - 1] and plan.nrec[n - 1] >= 1025
    lone = lad.special["d1r0"]
    assert plan.nrec[lone] == 0 and not plan.is_leader[lone] and lone not in plan.dest  # masked in `full`, must stay untouched
    # bucket 2 holds neither a leader nor a record, bucket 3 only leaders without a record
    b2, b3 = slice(2 * H.BUCKET, 3 * H.BUCKET), slice(3 * H.BUCKET, 4 * H.BUCKET)
    assert not plan.has_record[b2].any() and not plan.is_leader[b2].any()
    assert not plan.has_record[b3].any() and plan.is_leader[b3].sum() == 3
    assert plan.has_record[4 * H.BUCKET:].sum() > 100                                  # the partial bucket has segments
    # the never-stored ids, the counted columns, the hub column
    rpT, colT, _ = lad.transposed()
    lenT = np.diff(rpT)
    assert (lenT[list(H.NEVER_COL)] == 0).all()
    assert (lenT[H.COL_1], lenT[H.COL_2], lenT[H.COL_255]) == (1, 2, 255)
    totals = {k: int(len(H.plan_of(k).records[0])) for k in H.LIST_NAMES}
    assert [totals[k] for k in ("rec1", "rec3", "rec255", "rec257", "zero_only")] == [1, 3, 255, 257, 0]
    assert lenT[H.HUB_COL] > 5000 and lenT[H.HUB_COL] > 100 * (totals["hubcol"] // WALK_BLOCKS + 1)    # shares cut inside it
    assert totals["n16384"] == len(lad.col) and len(H.plan_of("n16384").leaders) == n
    assert len(H.plan_of("n16384").dest) == n > 8192                                   # more than one pass of the grid at D = 256
    assert [len(lad.lists[k]) for k in ("one", "n1024", "n1025", "n16384", "x300")] == [1, 1024, 1025, 16384, 300]
    assert len(np.unique(lad.lists["x300"])) == 1 and len(lad.lists["core"]) > len(plan.leaders)       # repeats
    assert set(H.LIST_NAMES) == set(lad.lists)
    # the lone leader is an ordinary operand row (norm_rows: 0 mod 8), so its epilogue term is not zero
    assert lad.lists["one"][0] % 8 == 0 and lad.lists["x300"][0] == lad.lists["one"][0] and lenT[lad.lists["one"][0]] > 0
    # zero-degree leaders first, last and adjacent in sorted order: ties in the prefix of the leaders' row lengths
    for k, where in (("zero_first", [0]), ("zero_last", [-1]), ("zero_adjacent", [1, 2]), ("core", [0, 1, -1])):
        assert (lenT[H.plan_of(k).leaders[where]] == 0).all(), k
    assert lenT[H.plan_of("zero_adjacent").leaders[[0, 3]]].min() > 0
    # operand rows that make exactly-zero and clamped products: rows gathering only all-zero G rows have a record
    zero_rows = np.flatnonzero((np.arange(n) % 16 == 9) & plan.has_record & ~plan.is_leader)
    assert len(zero_rows) > 50
    # the quantised sibling: the same structure, 12 significant bits in [2^-5, 2^2)
    m, e = np.frexp(np.abs(lad.val_q.astype(np.float64)))
    assert (m * 2 ** 12 == np.round(m * 2 ** 12)).all() and (np.abs(lad.val_q) >= 2.0 ** -5).all() and (np.abs(lad.val_q) < 4).all()


def _dense_rows(lad, r0, r1):
    Ad = np.zeros((r1 - r0, lad.n))
    s = slice(lad.rowptr[r0], lad.rowptr[r1])
    Ad[np.repeat(np.arange(r0, r1), lad.deg[r0:r1]) - r0, lad.col[s]] = lad.val[s].astype(np.float64)
    return Ad


@pytest.mark.parametrize("name", ["core", "n1025", "hubcol", "rec257", "zero_only", "n16384"])
def test_ref_is_the_dense_product_plus_autograd_of_normalize(name):
    lad, D = H.ladder(), 8
    plan, (G, X, inv32, dZ), row_mask, dz_flags = H.list_case(name, D)
    inv64 = np.full(plan.n, np.nan)
    inv64[plan.leaders] = R.inv_norm(X[plan.leaders])[0]                # fp64 norms: what autograd differentiates
    res = plan.hop(G, X, inv64, dZ, H.S, row_mask, dz_flags)
    assert np.array_equal(np.flatnonzero(res.visited), plan.dest) and np.array_equal(np.flatnonzero(res.epi), plan.leaders)
    Gl = G[plan.leaders].double().numpy()
    want = np.concatenate([_dense_rows(lad, r, min(r + 1024, lad.n))[:, plan.leaders] @ Gl for r in range(0, lad.n, 1024)])
    x = X[plan.leaders].double().requires_grad_()
    (torch.nn.functional.normalize(x, dim=1) * (H.S * dZ[plan.leaders].double())).sum().backward()
    want[plan.leaders] += x.grad.numpy()
    np.testing.assert_allclose(res.ref, want, rtol=1e-12, atol=1e-18)
    assert (res.ref[~res.visited] == 0).all() and (want[~res.visited] == 0).all()
    assert np.array_equal(res.out_flags, (want != 0).any(1).astype(np.uint8))
    # the counts: records on a short row, 1 + records 2^-29 on a long one with a record, + D + 7 under the epilogue
    c = res.c[:, 0] - np.where(res.epi, D + 7, 0)
    short = lad.deg <= H.K_LONG
    assert np.array_equal(c[short], plan.nrec[short])
    assert np.array_equal(c[~short], np.where(plan.nrec[~short] > 0, 1 + plan.nrec[~short] * 2.0 ** -29, 0.0))
    if name == "core":
        assert (res.mag[res.visited] == 0).all(1).any() and (R.f64(inv32)[plan.leaders] == float(R.INV_CLAMPED)).any()


def test_visited_rows_under_masks_and_flags():
    for mask, dz in H.MASK_CASES:
        plan, _, row_mask, dz_flags = H.mask_case(mask, dz, 8)
        vis, epi = plan.visited(row_mask, dz_flags)
        want_vis, want_epi = np.zeros(plan.n, bool), np.zeros(plan.n, bool)
        for j in plan.dest:                                               # the sentence of the kernel's contract, row by row
            flagged = dz_flags is None or bool(dz_flags[j])
            want_vis[j] = bool(row_mask[j]) and (len(plan.segment(j)[0]) > 0 or flagged)
            want_epi[j] = want_vis[j] and flagged
        assert np.array_equal(vis, want_vis) and np.array_equal(epi, want_epi)
        lad = H.ladder()
        assert not vis[lad.special["d1r0"]]                               # masked or not: no record, no leader
        if mask == "cleared":
            gone = plan.has_record & (row_mask == 0)
            assert gone.sum() > 100 and gone[lad.special["d1025rall"]] and (plan.is_leader & (row_mask == 0)).sum() >= 2
        if dz == "subset":
            sub = np.flatnonzero(dz_flags)
            assert 0 < len(sub) < len(plan.leaders) and np.isin(sub, plan.leaders).all()
            assert (plan.is_leader & ~plan.has_record & (dz_flags == 0) & ~vis).sum() >= 1     # a bare leader is skipped
        else:
            assert (vis & ~plan.has_record).any() and np.array_equal(epi, vis)


@pytest.mark.parametrize("name", H.LIST_NAMES)
def test_dest_is_mark_rows_of_the_transpose(name):
    lad = H.ladder()
    plan = H.plan_of(name)
    rpT, colT, _ = lad.transposed()
    with_record = R.mark_rows(rpT, colT, plan.leaders, np.zeros(lad.n, np.uint8), self_too=False)
    assert np.array_equal(with_record.astype(bool), plan.has_record)
    both = R.mark_rows(rpT, colT, lad.lists[name], np.zeros(lad.n, np.uint8))
    assert np.array_equal(np.flatnonzero(both), plan.dest) and len(np.unique(plan.dest)) == len(plan.dest)
    assert np.array_equal(plan.leaders, np.unique(lad.lists[name]))
    j, b, w = plan.records                                               # the records are the stored entries of the leaders
    assert np.isin(b, plan.leaders).all() and len(j) == int(np.diff(rpT)[plan.leaders].sum())
    if name == "core":                                                   # each one the entry (j, b) of A itself, value and all
        entry = {(int(r), int(c)): v for r, c, v in zip(np.repeat(np.arange(lad.n), lad.deg), lad.col, lad.val)}
        assert all(entry[(int(jj), int(bb))] == ww for jj, bb, ww in zip(j, b, w))
        assert len(j) == int(np.isin(lad.col, plan.leaders).sum())
    for r in plan.dest[:: max(1, len(plan.dest) // 50)]:
        bs, _ = plan.segment(r)
        assert (np.diff(bs) > 0).all() and len(bs) == plan.nrec[r]


def _frac(a):
    return [Fraction(float(v)) for v in np.asarray(a, np.float64).ravel()]


def test_chain32_steps_are_exact_rationals():
    """Every fp64 step of chain32 on the quantised operands is the exact rational sum, so its rounding to float32 is an fmaf.
    The whole core list at D = 8; the 1024-record chain and a sample of the n16384 list."""
    for name, pick in (("core", None), ("n16384", 40)):
        plan, G, short, long_rows = H.order_case(name, 8)
        lad = H.ladder()
        rows = short if pick is None else np.unique(np.concatenate([short[:: len(short) // pick], [lad.special["d1024rall"]]]))
        trace = []
        got = plan.chain32(G, rows, trace=trace)
        assert len(trace) == plan.nrec[rows].max() == 1024
        for acc, w, x, s64 in trace:
            want = [a + ww * xx for a, ww, xx in zip(_frac(acc), _frac(np.broadcast_to(w, x.shape)), _frac(x))]
            assert want == _frac(s64)
        one = plan.chain32(G, int(rows[-1]))
        assert one.shape == (8,) and np.array_equal(one.view(np.int32), got[-1].view(np.int32))
        # the long rows: the fp64 sum of the quantised terms is exact as well, in any order
        for j in long_rows[:3] if pick is None else [lad.special["d1025rall"]]:
            b, w = plan.segment(j)
            exact = [sum(Fraction(float(ww)) * Fraction(float(xx)) for ww, xx in zip(w, G[b][:, d])) for d in range(8)]
            assert exact == _frac(plan.product(G)[0][j])


@pytest.mark.parametrize("D", [8, 32, 256])
@pytest.mark.parametrize("name", ["core", "n16384"])
def test_a_descending_chain_has_other_bits(name, D):
    plan, G, short, long_rows = H.order_case(name, D)
    up, down = plan.chain32(G, short), plan.chain32(G, short, descending=True)
    differ = (up.view(np.int32) != down.view(np.int32)).any(1)
    assert differ.sum() >= 100, f"{differ.sum()} of {len(short)} checked rows tell the order"
    assert len(long_rows) >= 3 and plan.nrec[long_rows].max() >= 1025
    assert plan.nrec[long_rows].min() == (1 if name == "core" else 1025)
    ref, mag = plan.product(G)
    assert (np.abs(up - ref[short]) <= plan.nrec[short, None] * R.U32 * mag[short]).all()


@pytest.mark.parametrize("D", WIDTHS)
def test_no_out_flag_is_left_undecided(D):
    """Every visited row of every case of the GPU test either has only exactly-zero terms or an element beyond its bound."""
    for name in H.LIST_NAMES:
        plan, ops, row_mask, dz_flags = H.list_case(name, D)
        res = plan.hop(*ops, H.S, row_mask, dz_flags)
        assert res.undecided.sum() == 0, (name, np.flatnonzero(res.undecided)[:5])
        assert res.visited.sum() == len(plan.dest)
    if D in (8, 64, 256):
        for mask, dz in H.MASK_CASES:
            plan, ops, row_mask, dz_flags = H.mask_case(mask, dz, D)
            res = plan.hop(*ops, H.S, row_mask, dz_flags)
            assert res.undecided.sum() == 0, (mask, dz)
            assert (res.out_flags[res.visited] == 0).any() and (res.out_flags[res.visited] == 1).any()
