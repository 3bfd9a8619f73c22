"""numpy restatement of the order contract of `rowops.scatter_rows_ordered` (include/tagrec.h, row_scatter_ordered), shared by
test_gpu_rowscatter.py and test_rowscatter_host.py.  Every add is an explicit fp32 add of two fp32 arrays.

    dst[r] (=|+=) sum of src[j] over rows[j] == r
      * a row's slots in ascending slot id;
      * <= 1024 slots: one left-to-right chain that starts from the first term;
      * more: consecutive chunks of 1024 slots, each such a chain, and the chunk sums added left to right;
      * dst touched once per row: assign, or one add of the finished sum.
"""
import numpy as np

CHUNK = 1024


def make_values(rng, T, D):
    """randn * 10^U(-3, 3): magnitudes six decades apart, so the order of an fp32 sum shows in its last bits."""
    return (rng.standard_normal((T, D)) * 10.0 ** rng.uniform(-3, 3, (T, D))).astype(np.float32)


def segments(rows, n):
    """[(row, [slots ascending])] for the distinct in-range rows, ascending."""
    rows = np.asarray(rows)
    out = []
    for r in np.unique(rows[(rows >= 0) & (rows < n)]):
        out.append((int(r), np.flatnonzero(rows == r).tolist()))
    return out


def chain(src, slots):
    acc = src[slots[0]].astype(np.float32).copy()
    for j in slots[1:]:
        acc = acc + src[j]
        assert acc.dtype == np.float32
    return acc


def segment_sum(src, slots):
    parts = [chain(src, slots[k:k + CHUNK]) for k in range(0, len(slots), CHUNK)]
    tot = parts[0]
    for p in parts[1:]:
        tot = tot + p
    return tot


def scatter_ref(rows, n, src, dst, accumulate, descending=False):
    """-> a copy of dst after the scatter.  descending: the slots of every row taken in DESCENDING slot id (the same scheme
    otherwise) -- not the contract; what a test compares against to show that its values tell the orders apart."""
    out = dst.copy()
    for r, slots in segments(rows, n):
        s = segment_sum(src, slots[::-1] if descending else slots)
        out[r] = (out[r] + s) if accumulate else s
    return out


def zipf_rows(rng, T, n):
    """T ids in [0, n) with a Zipf-like head: a few ids hold most slots (the popular items of a BPR batch)."""
    return np.minimum(rng.zipf(1.3, T) - 1, n - 1).astype(np.int64)
