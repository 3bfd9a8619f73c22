"""GPU: the list-driven batch hop of csrc/batch_hop.hip -- the plan (leader sort, balanced walk, buckets, segment order) and
batch_hop_kernel at every vector width -- against the plain restatement of tests/batch_hop_ref.py (held to a dense fp64
product, torch autograd, spmm_ref.mark_rows and exact rationals by test_batch_hop_ref_host.py).  No other kernel of the project
is the yardstick here; test_gpu_batch_hop.py and test_gpu_batch_hop_list.py compare the hop with the masked row kernel.

Tolerance: spmm_ref.Chk, |got - ref64| <= c * 2^-24 * mag + 1e-30, with c per row from batch_hop_ref.Plan.count: the row's
RECORDS (one fmaf each) when A's row has at most 1024 stored entries, 1 + records * 2^-29 when it is longer (an fp64 chain
rounded once), + D + 7 where the row takes the normalize-backward term.  The destination set, segment lengths, out_flags,
untouched rows (NaN / sentinel pre-fill), the fmaf chain in ascending source order on 12-bit operands and the long rows'
once-rounded sum are exact.  Every test prints its worst err / bound (`-s`); DESIGN section 2 carries the table.

The hop ladder (batch_hop_ref.HopLadder): 8493 = 4 * 2048 + 301 rows (five plan buckets, the last partial), ~1.2e5 signed
entries, rows of degree 0 .. 5, 63 .. 65, 1023 .. 1025, 2049 and a hub of 8443 at rows that include 2047, 2048, 4095, 4096,
8191, 8192 and 8492, with 0, 1, 3, 4, 5, 8 or all of their columns in the core list; 15 lists (1, 1024, 1025 and 16384 ids,
repeats, record totals 1, 3, 255, 257 and 0, a transposed row of ~6000, zero-degree leaders first, last and adjacent)."""
import faulthandler

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import tagrec_amd as T
from tagrec_amd import _lib
from tagrec_amd.rowops import VEC_WIDTHS

import batch_hop_ref as H
from spmm_ref import Chk as _Chk, same_bits

DEV = torch.device("cuda:0")
NAN = float("nan")
SENTINEL = 7                               # pre-fill of out_flags: a row the hop does not visit keeps it


@pytest.fixture(autouse=True)
def _per_test_timeout():
    """A hung kernel must end the run, not sit on the GPU: the process exits if one test takes longer than this."""
    faulthandler.dump_traceback_later(120, exit=True)
    yield
    faulthandler.cancel_dump_traceback_later()


def Chk(name):
    return _Chk(name, tag="batch_hop")


def dev(a, dtype=None):
    t = a if isinstance(a, torch.Tensor) else torch.from_numpy(np.ascontiguousarray(a))
    return t.to(DEV) if dtype is None else t.to(DEV, dtype)


def _bits(t):
    return t.cpu().numpy().view(np.int32)


# ============================================================================================================ the graphs
@pytest.fixture(scope="module")
def graphs():
    """(A, A^T) on the device for the ladder's values and for its 12-bit sibling.  The hop takes `is_long` from A's row
    pointer and the weights from the plan's graph, so the two must be exact transposes: A^T carries bit copies of the values
    in the host transpose's order, and the transpose of a fresh graph over A^T's arrays is A again."""
    lad, out = H.ladder(), []
    for q in (False, True):
        rp, col, val = lad.csr(q)
        A = T.Graph(dev(rp), dev(col, torch.int32), dev(val), (lad.n, lad.n))
        At = A.transpose()
        rpT, colT, valT = lad.transposed(q)
        assert np.array_equal(At.rowptr.cpu().numpy(), rpT) and np.array_equal(At.col.cpu().numpy(), colT)
        assert np.array_equal(_bits(At.val), np.asarray(valT, np.float32).view(np.int32))
        back = T.Graph(At.rowptr.clone(), At.col.clone(), At.val.clone(), (lad.n, lad.n)).transpose()
        assert np.array_equal(back.rowptr.cpu().numpy(), rp) and np.array_equal(back.col.cpu().numpy(), col)
        assert np.array_equal(_bits(back.val), val.view(np.int32))
        out.append((A, At))
    return lad, out[0], out[1]


def _plan(At, rows, cap=None):
    """The plan of `rows` in a buffer pre-filled with 0xFF."""
    cap = At.batch_hop_capacity(rows.numel()) if cap is None else cap
    buf = torch.full((At.batch_hop_workspace(rows.numel(), cap),), 0xFF, dtype=torch.uint8, device=DEV)
    return At.batch_hop_plan(rows, cap, buf)


def _dest_entries(At, plan):
    """The plan's (row, segment start, segment length) entries, read back as batch_hop_rows reads the rows."""
    buf, ptr, _, n_listed, capacity = plan
    at = [int(_lib.load().tagrec_batch_hop_list_result(At.shape[1], n_listed, capacity, k)) for k in range(3)]
    assert min(at) >= 0
    base = ptr - buf.data_ptr()
    k = int(buf[base + at[0]:base + at[0] + 4].view(torch.int32).item())
    assert 0 <= k <= at[2]
    return buf[base + at[1]:base + at[1] + 16 * k].view(torch.int32).view(-1, 4)[:, :3].cpu().numpy()


def _run(A, At, rows, ops, row_mask, dz_flags):
    """Plan + hop from fresh buffers, NaN background, out_flags pre-filled with a sentinel.  -> out, out_flags."""
    G, X, inv, dZ = ops
    plan = _plan(At, rows)
    out = torch.full((A.shape[0], G.shape[1]), NAN, device=DEV)
    fo = torch.full((A.shape[0],), SENTINEL, dtype=torch.uint8, device=DEV)
    A.batch_hop_normbwd(plan, G, X, inv, dZ, H.S, out, fo, row_mask, dz_flags)
    At.batch_hop_check()
    return out, fo


def _twice(run):
    a, b = run(), run()
    assert all(same_bits(s, t) for s, t in zip(a, b)), "two runs of one hop differ"
    return a


def _check(chk, what, res, out, fo):
    """Visited rows against (ref, mag, c); every other row bit-untouched; out_flags exact where the reference decides them
    (everywhere: the share of undecided rows must be zero).  A NaN read from an operand row outside the listed set would
    show as a non-finite value in a visited row."""
    vis = res.visited
    got = out.cpu().numpy()
    chk.close(what, got[vis], res.ref[vis], res.mag[vis], res.c[vis])
    untouched = np.float32(NAN).view(np.int32)
    assert (got.view(np.int32)[~vis] == untouched).all(), f"{what}: a row outside the visited set was written"
    flags = fo.cpu().numpy()
    assert (flags[~vis] == SENTINEL).all(), f"{what}: an out_flags byte outside the visited set was written"
    assert res.undecided.sum() == 0, f"{what}: {res.undecided.sum()} rows whose flag the reference cannot decide"
    assert np.array_equal(flags[vis], res.out_flags[vis]), f"{what}: out_flags"


# ============================================================================================================== the plan
@pytest.mark.parametrize("name", H.LIST_NAMES)
def test_plan_destinations_exact(graphs, name):
    lad, (A, At), _ = graphs
    ref = H.plan_of(name)
    rows = dev(lad.lists[name])
    cap = At.batch_hop_capacity(rows.numel())
    records = len(ref.records[0])
    assert cap >= records
    for capacity in (cap, max(1, records)):                              # the caller's bound, then the tight one
        plan = _plan(At, rows, capacity)
        At.batch_hop_check()
        dest = At.batch_hop_rows(plan).cpu().numpy()
        assert len(np.unique(dest)) == len(dest), "a row is listed twice"
        assert np.array_equal(np.sort(dest), ref.dest), "the list is not the set of destinations and leaders"
        ent = _dest_entries(At, plan)
        assert np.array_equal(ent[:, 0], dest) and np.array_equal(ent[:, 2], ref.nrec[dest]), "segment lengths"
        seg = ent[ent[:, 2] > 0]
        seg = seg[np.argsort(seg[:, 1])]                                 # the segments tile [0, records)
        assert np.array_equal(seg[:, 1], np.concatenate([[0], np.cumsum(seg[:, 2])])[:-1]) and seg[:, 2].sum() == records
    print(f"[batch_hop] plan {name}: {len(ref.leaders)} leaders, {records} records, {len(ref.dest)} destinations exact")


# =============================================================================================================== the hop
@pytest.mark.parametrize("D", VEC_WIDTHS)
@pytest.mark.parametrize("name", H.LIST_NAMES)
def test_hop_against_fp64(graphs, name, D):
    lad, (A, At), _ = graphs
    ref, ops, row_mask, dz_flags = H.list_case(name, D)
    rows = dev(lad.lists[name])
    mid = At.mark_rows(rows, torch.zeros(lad.n, dtype=torch.uint8, device=DEV))
    assert np.array_equal(mid.cpu().numpy(), row_mask)
    tflag = dev(dz_flags)
    ops_d = tuple(dev(t) for t in ops)
    if name == "n16384" and D == 256:                                    # the hop's loop and its prefetch run more than once
        assert len(ref.dest) > T.Graph.batch_hop_grid_rows(D) > 0
    out, fo = _twice(lambda: _run(A, At, rows, ops_d, mid, tflag))
    chk = Chk(f"hop {name} D={D}")
    # c = records | 1 + records 2^-29 on a long row, + D + 7 on the listed rows (batch_hop_ref.Plan.count)
    _check(chk, "hop", ref.hop(*ops, H.S, row_mask, dz_flags), out, fo)
    chk.done()


@pytest.mark.parametrize("D", [8, 64, 256])
def test_hop_masks_and_flags(graphs, D):
    lad, (A, At), _ = graphs
    rows = dev(lad.lists["core"])
    chk = Chk(f"masks and flags D={D}")
    for mask, dz in H.MASK_CASES:
        ref, ops, row_mask, dz_flags = H.mask_case(mask, dz, D)
        ops_d = tuple(dev(t) for t in ops)
        mask_d, dz_d = dev(row_mask), None if dz_flags is None else dev(dz_flags)
        out, fo = _twice(lambda: _run(A, At, rows, ops_d, mask_d, dz_d))
        res = ref.hop(*ops, H.S, row_mask, dz_flags)
        assert 0 < res.visited.sum() < len(ref.dest) or mask == "full" and dz == "none"
        # c as above; + D + 7 on every visited row when dz_flags is None, on the flagged subset of the leaders otherwise
        _check(chk, f"{mask}/{dz}", res, out, fo)
    chk.done()


@pytest.mark.parametrize("D", [8, 32, 256])
@pytest.mark.parametrize("name", ["core", "n16384"])
def test_segment_order_is_ascending_bits(graphs, name, D):
    """12-bit weights and operands: every step of the fp32 chain is exact in fp64, so the emulated chain is the kernel's fmaf
    chain bit for bit -- in ascending source order and in no other (test_batch_hop_ref_host.py: >= 100 of the checked rows
    change bits when summed in descending order); the long rows' fp64 sum is exact, so they equal its float32."""
    lad, _, (A, At) = graphs
    ref, G, short, long_rows = H.order_case(name, D)
    rows = dev(lad.lists[name])
    mid = At.mark_rows(rows, torch.zeros(lad.n, dtype=torch.uint8, device=DEV))
    off = torch.zeros(lad.n, dtype=torch.uint8, device=DEV)              # no row takes the epilogue term: its operands are NaN
    nan2, nan1 = torch.full((lad.n, D), NAN, device=DEV), torch.full((lad.n,), NAN, device=DEV)
    out, fo = _twice(lambda: _run(A, At, rows, (dev(G), nan2, nan1, nan2), mid, off))
    got = out.cpu().numpy()
    want = ref.chain32(G, short)
    bad = (got[short].view(np.int32) != want.view(np.int32)).any(1)
    assert not bad.any(), f"{bad.sum()} of {len(short)} short rows differ from the ascending fmaf chain, first {short[bad][:5]}"
    exact = ref.product(G)[0][long_rows].astype(np.float32)
    assert len(long_rows) >= 3 and np.array_equal(got[long_rows].view(np.int32), exact.view(np.int32)), "long rows"
    vis = ref.has_record
    assert (got.view(np.int32)[~vis] == np.float32(NAN).view(np.int32)).all()
    flags = fo.cpu().numpy()
    assert (flags[~vis] == SENTINEL).all() and np.array_equal(flags[vis], (got[vis] != 0).any(1).astype(np.uint8))
    chk = Chk(f"order {name} D={D} ({len(short)} short, {len(long_rows)} long rows)")
    chk.close("short", got[short], want, np.abs(want), 0)               # c = 0: nothing but the bits of the chain
    chk.close("long", got[long_rows], exact, np.abs(exact), 0)          # c = 0: the exact sum rounded once
    chk.done()


# ========================================================================================================== the wrappers
def test_wrapper_equals_direct_call(graphs):
    lad, (A, At), _ = graphs
    lib, n, D = _lib.load(), lad.n, 64
    ref, ops, row_mask, dz_flags = H.list_case("core", D)
    rows, mid, tflag = dev(lad.lists["core"]), dev(row_mask), dev(dz_flags)
    G, X, inv, dZ = (dev(t) for t in ops)
    out_w, fo_w = _run(A, At, rows, (G, X, inv, dZ), mid, tflag)

    cap = At.batch_hop_capacity(rows.numel())
    buf = torch.full((At.batch_hop_workspace(rows.numel(), cap),), 0xFF, dtype=torch.uint8, device=DEV)
    err = torch.zeros(1, dtype=torch.int32, device=DEV)
    shift = (-buf.data_ptr()) % 256
    ptr, nbytes = buf.data_ptr() + shift, buf.numel() - shift
    _lib.check(lib.tagrec_batch_hop_plan(At.handle, rows, rows.numel(), cap, _lib.c_void_p(ptr), nbytes, err, _lib.stream_ptr()),
               "batch_hop_plan")
    out_d = torch.full((n, D), NAN, device=DEV)
    fo_d = torch.full((n,), SENTINEL, dtype=torch.uint8, device=DEV)
    _lib.check(lib.tagrec_batch_hop_normbwd_f32(A.handle, _lib.c_void_p(ptr), nbytes, rows.numel(), cap, G, X, inv, dZ, H.S, out_d,
                                                fo_d, mid, tflag, D, _lib.stream_ptr()), "batch_hop_normbwd")
    assert int(err.item()) == 0 and same_bits(out_d, out_w) and same_bits(fo_d, fo_w)
    chk = Chk("wrapper = direct call")
    vis = torch.from_numpy(ref.visited(row_mask, dz_flags)[0])
    chk.close("hop", out_d.cpu()[vis], out_w.cpu()[vis], out_w.cpu()[vis].abs(), 0)        # c = 0: the same bits
    chk.done()

    # every id outside the matrix: no leader, so every later kernel of the plan and the hop are no-ops; the host is told
    outside = torch.tensor([n, n + 7, -1, 1 << 40], dtype=torch.int64, device=DEV)
    plan = _plan(At, outside)
    ones = torch.ones(n, dtype=torch.uint8, device=DEV)
    out = torch.full((n, D), NAN, device=DEV)
    fo = torch.full((n,), SENTINEL, dtype=torch.uint8, device=DEV)
    A.batch_hop_normbwd(plan, G, X, inv, dZ, H.S, out, fo, ones, None)
    with pytest.raises(T.TagrecError, match="row id outside the matrix"):
        At.batch_hop_check()
    At.batch_hop_check()                                                 # (the check cleared the error)
    assert At.batch_hop_rows(plan).numel() == 0
    assert same_bits(out, torch.full((n, D), NAN, device=DEV)) and bool((fo == SENTINEL).all())
