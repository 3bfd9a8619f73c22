"""Plain restatement of the list-driven batch hop of csrc/batch_hop.hip (plan and hop) and the "hop ladder" fixture shared
by test_gpu_batch_hop_kernels.py and test_batch_hop_ref_host.py.  numpy on the CPU; no project code.

The hop multiplies by a square matrix A.  Its plan is built from the TRANSPOSE of A and a list of row ids: the distinct listed
ids that are rows of the matrix are the LEADERS; every stored entry (b, j, w) of row b of the transpose, b a leader, is a RECORD
(j, b, w): destination j gathers w * G_in[b].  The hop visits every destination with a record and every leader (it may have
no record and still take the normalize-backward term), under a row mask and optional dz flags:

    out[j] = sum over the records of j, ascending b, of w * G_in[b]   (+ inv (s dz - z (z . s dz)) where the row takes the term)

Tolerance (spmm_ref.Chk): |got - ref64| <= c * 2^-24 * mag + 1e-30 with c, read off batch_hop_kernel:
  * a row of A with at most 1024 stored entries: its number of RECORDS, one fmaf each (not its stored entries: the bound is
    the handful of entries that point at a listed row, so a wrong or lost record cannot hide under the row's degree);
  * a longer row with a record: 1 + records * 2^-29 -- an fp64 fma chain (records * 2^-53 of the magnitude) rounded once;
    its reference is summed in extended precision so that the count pays for the kernel's chain alone;
  * + D + 7 where the row takes the epilogue term (the count test_gpu_spmm.py uses for NORMBWD)."""
import numpy as np

import spmm_ref as R

K_LONG = 1024                              # kLongRow of csrc/graph.h: rows of A with more stored entries take the fp64 chain
BUCKET = 2048                              # kBucketRows of csrc/batch_hop.hip
S = float(np.float32(1.0 / 3.0))           # a scale that is exact as the float the ABI takes


# ============================================================================================================= the plan
class Plan:
    """What tagrec_batch_hop_plan must produce for (A, A^T, listed), as sets and sorted arrays."""

    def __init__(self, A, At, listed):
        rpA, _, _ = A
        rpT, colT, valT = At
        self.n = n = len(rpA) - 1
        assert len(rpT) - 1 == n, "square matrix expected"
        ids = np.asarray(listed, np.int64)
        self.leaders = np.unique(ids[(ids >= 0) & (ids < n)])
        rpT = np.asarray(rpT, np.int64)
        lens = rpT[self.leaders + 1] - rpT[self.leaders]
        lpre = np.concatenate([[0], np.cumsum(lens)])
        at = np.arange(lpre[-1]) - np.repeat(lpre[:-1], lens) + np.repeat(rpT[self.leaders], lens)
        j, b, w = np.asarray(colT, np.int64)[at], np.repeat(self.leaders, lens), np.asarray(valT, np.float32)[at]
        self.records = (j, b, w)                                         # in the stored order of the transposed rows
        order = np.lexsort((b, j))                                       # by destination, ascending source inside one
        self.seg_j, self.seg_b, self.seg_w = j[order], b[order], w[order]
        self.nrec = np.bincount(j, minlength=n).astype(np.int64)
        self.seg_start = np.concatenate([[0], np.cumsum(self.nrec)])[:-1]
        self.has_record = self.nrec > 0
        self.is_leader = np.zeros(n, bool)
        self.is_leader[self.leaders] = True
        self.dest = np.flatnonzero(self.has_record | self.is_leader)
        self.deg = np.diff(np.asarray(rpA, np.int64))
        self.long = (self.deg > K_LONG) & self.has_record                # (a long row without a record sums nothing)

    def segment(self, j):
        """(b, w) of row j's records in ascending b."""
        s = slice(self.seg_start[j], self.seg_start[j] + self.nrec[j])
        return self.seg_b[s], self.seg_w[s]

    def visited(self, row_mask, dz_flags=None):
        """-> (rows the hop writes, rows among them that take the epilogue term), bool [n]."""
        on = np.zeros(self.n, bool)
        on[self.dest] = True
        flagged = np.ones(self.n, bool) if dz_flags is None else np.asarray(dz_flags) != 0
        vis = on & (np.asarray(row_mask) != 0) & (self.has_record | flagged)
        return vis, vis & flagged

    def count(self, D, epi):
        """c [n, 1]: rounded fp32 operations per row (module docstring)."""
        c = np.where(self.long, 1.0 + self.nrec * 2.0 ** -29, self.nrec.astype(np.float64))
        return (c + np.where(epi, D + 7.0, 0.0))[:, None]

    def product(self, G_in):
        """fp64 (sum w G_in[b], sum |w| |G_in[b]|) [n, D] over the records; rows without one are zero.  Only leader rows of
        G_in are read.  Long rows are summed in extended precision (every product of two floats is exact in fp64)."""
        G = np.asarray(G_in.detach().cpu().numpy() if hasattr(G_in, "detach") else G_in, np.float32)
        D = G.shape[1]
        ref, mag = np.zeros((self.n, D)), np.zeros((self.n, D))
        rows = np.flatnonzero(self.has_record)
        if len(rows) == 0:
            return ref, mag
        w = self.seg_w.astype(np.float64)[:, None]
        for c0 in range(0, D, 64):
            p = w * G[:, c0:c0 + 64].astype(np.float64)[self.seg_b]
            assert np.isfinite(p).all(), "a record gathers a row that holds no operand"
            ref[rows, c0:c0 + 64] = np.add.reduceat(p, self.seg_start[rows], axis=0)
            mag[rows, c0:c0 + 64] = np.add.reduceat(np.abs(p), self.seg_start[rows], axis=0)
        for j in np.flatnonzero(self.long):
            b, wj = self.segment(j)
            p = wj.astype(np.longdouble)[:, None] * G[b].astype(np.longdouble)
            ref[j] = p.sum(0).astype(np.float64)
        return ref, mag

    def hop(self, G_in, X_raw, inv_norm, dZ, s, row_mask, dz_flags=None):
        """The hop in fp64 from the kernel's own operands.  -> Result."""
        vis, epi = self.visited(row_mask, dz_flags)
        ref, mag = self.product(G_in)
        ref[~vis], mag[~vis] = 0.0, 0.0
        D = ref.shape[1]
        if epi.any():
            x, iv, dz = (R.f64(t)[epi] for t in (X_raw, inv_norm, dZ))
            assert np.isfinite(x).all() and np.isfinite(iv).all() and np.isfinite(dz).all(), "an epilogue row holds no operand"
            clamped = iv >= float(R.INV_CLAMPED)                         # the kernel's test: inv >= 1e12f drops the dot
            ref[epi], mag[epi] = R.epi_normbwd(ref[epi], mag[epi], x, iv, dz, s, clamped)
        c = self.count(D, epi)
        bound = c * R.U32 * mag + 1e-30
        zero_sure = (mag == 0).all(1)                                    # every term exactly zero
        nz_sure = (np.abs(ref) > bound).any(1)                           # some element cannot round to zero
        return Result(vis, epi, ref, mag, c, R.row_flags(ref), vis & ~zero_sure & ~nz_sure)

    def chain32(self, G_in, rows, descending=False, trace=None):
        """The fp32 fmaf chain from zero over each row's segment in ascending (descending) source order, emulated as
        float32(float64(acc) + float64(w) * float64(x)): an exact fmaf whenever the fp64 step is exact (the product of two
        floats always is).  -> float32 [len(rows), D].  trace: a list that receives (acc, w, x, sum64) of every step."""
        G = np.asarray(G_in.detach().cpu().numpy() if hasattr(G_in, "detach") else G_in, np.float32)
        one = np.ndim(rows) == 0
        rows = np.atleast_1d(np.asarray(rows, np.int64))
        by_len = np.argsort(-self.nrec[rows], kind="stable")             # the active rows of step t are a prefix
        L, start = self.nrec[rows][by_len], self.seg_start[rows][by_len]
        acc = np.zeros((len(rows), G.shape[1]), np.float32)
        for t in range(int(L.max()) if len(rows) else 0):
            k = int(np.searchsorted(-L, -t, side="left"))                # rows with L > t
            p = start[:k] + (L[:k] - 1 - t if descending else t)
            w, x = self.seg_w[p].astype(np.float64)[:, None], G[self.seg_b[p]].astype(np.float64)
            s64 = acc[:k].astype(np.float64) + w * x
            if trace is not None:
                trace.append((acc[:k].copy(), w, x, s64))
            acc[:k] = s64.astype(np.float32)
        out = np.empty_like(acc)
        out[by_len] = acc
        return out[0] if one else out


class Result:
    def __init__(self, visited, epi, ref, mag, c, out_flags, undecided):
        self.visited, self.epi, self.ref, self.mag, self.c = visited, epi, ref, mag, c
        self.out_flags, self.undecided = out_flags, undecided


# =========================================================================================================== the fixture
N = 4 * BUCKET + 301                       # five buckets, the last one partial (W = 301)
NEVER_COL = (7, 8, 9, 3000, 3500, 8191, 8490, 8491)       # ids no row of A stores: zero-degree rows of the transpose
HUB_COL = 5000                             # the column three quarters of the ordinary rows store: a transposed row of ~6000
COL_1, COL_2, COL_255 = 4100, 4101, 6200   # columns stored by exactly 1, 2 and 255 rows
LADDER_ROWS = (13, 18, 23, 28, 33, 38, 43, 48, 2047, 2048, 2053, 2058, 4095, 4096, 8191, 8192, N - 1)


class HopLadder:
    """Square CSR of N = 8493 rows without duplicate column ids (columns ascending inside a row), ~1.2e5 signed entries.

    The CORE list: ~1100 ids of buckets 0, 1 and 4 (rows 0 .. 4095, 8192 ..), three ids of bucket 3 and none of bucket 2; it
    holds the never-stored ids 7, 8 (first and adjacent in sorted order), 8191 and 8491 (last).  Rows of buckets 2 and 3 store
    no core column, so under the core list bucket 2 (rows 4096 .. 6143) holds neither a leader nor a record and bucket 3
    (6144 .. 8191) only leaders without a record.  `special` maps a name to its row:
      d{deg}r{records}: a row of that degree with that many core columns ("all" = every column is core).
    Ordinary rows of buckets 0, 1, 4 draw <= 24 columns from every id that may be stored; rows 9 mod 16 there draw core ids
    1 mod 8 only (operand rows that are all zero: an exactly-zero product) and rows 13 mod 16 at most four core ids 3 mod 8
    (operand rows of norm 1e-13)."""

    def __init__(self, seed=11):
        rng = np.random.default_rng(seed)
        n = self.n = N
        ids = np.arange(n)
        reserved = set(NEVER_COL) | {HUB_COL, COL_1, COL_2, COL_255}
        free = np.array([i for i in ids if i not in reserved])
        core_zone = free[((free > 9) & (free < 2 * BUCKET)) | ((free >= 4 * BUCKET) & (free < 8490))]   # 7, 8 first, 8491 last
        core_zone = np.setdiff1d(core_zone, LADDER_ROWS)                 # (a ladder row is a leader only where its name says so)
        core_big = np.sort(rng.choice(core_zone, 1100, replace=False))
        self.core = np.unique(np.concatenate([core_big, [7, 8, 6144, 7000, 8191, 8491]]))
        non_core = np.setdiff1d(free, self.core)
        zero_core, tiny_core = core_big[core_big % 8 == 1], core_big[core_big % 8 == 3]
        assert len(zero_core) > 60 and len(tiny_core) > 60

        def mixed(deg, rec):                                             # `rec` core columns, the rest not core
            return np.concatenate([rng.choice(core_big, rec, replace=False), rng.choice(non_core, deg - rec, replace=False)])

        designed = {
            "d0r0": (13, mixed(0, 0)), "d0r0_lead": (8191, mixed(0, 0)), "d1r0": (18, mixed(1, 0)), "d1r1": (23, mixed(1, 1)),
            "d2r1": (28, mixed(2, 1)), "d3r3": (33, mixed(3, 3)), "d4r4": (38, mixed(4, 4)), "d5r5": (43, mixed(5, 5)),
            "d5r0": (4096, mixed(5, 0)), "d63r8": (48, mixed(63, 8)), "d64r3": (2053, mixed(64, 3)), "d65r65": (8192, mixed(65, 65)),
            "d1023r5": (2058, mixed(1023, 5)), "d1024rall": (2047, mixed(1024, 1024)), "d1025rall": (2048, mixed(1025, 1025)),
            "d2049r1": (4095, mixed(2049, 1)),
            "hub": (n - 1, np.setdiff1d(free, rng.choice(non_core, 38, replace=False))),
        }
        self.special = {k: r for k, (r, _) in designed.items()}
        at = {r: c for r, c in designed.values()}
        assert sorted(at) == sorted(LADDER_ROWS)
        # the rows that store the counted columns: any bucket, ordinary rows only
        ordinary = np.array([r for r in ids if r not in at])
        extra = {}
        for c, k in ((COL_1, 1), (COL_2, 2), (COL_255, 255)):
            for r in rng.choice(ordinary, k, replace=False):
                extra.setdefault(int(r), []).append(c)
        rowptr, col = [0], []
        for r in range(n):
            if r in at:
                c = at[r]
            else:
                core_free = r < 2 * BUCKET or r >= 4 * BUCKET
                if core_free and r % 16 == 9:
                    c = rng.choice(zero_core, int(rng.integers(1, 12)), replace=False)
                elif core_free and r % 16 == 13:
                    c = rng.choice(tiny_core, int(rng.integers(1, 5)), replace=False)
                else:
                    c = rng.choice(free if core_free else non_core, int(rng.integers(0, 25)), replace=False)
                    if r % 4 != 1:
                        c = np.append(c, HUB_COL)
                c = np.concatenate([c, extra.get(r, [])]).astype(np.int64)
            assert len(np.unique(c)) == len(c)
            col += sorted(int(v) for v in c)
            rowptr.append(len(col))
        self.rowptr, self.col = np.array(rowptr, np.int64), np.array(col, np.int64)
        nnz = len(col)
        self.val = (rng.uniform(0.05, 1.0, nnz) * rng.choice([-1.0, 1.0], nnz)).astype(np.float32)
        self.val_q = quantised(rng, nnz)                                 # the same structure with 12-bit weights
        self.deg = np.diff(self.rowptr)
        self.lists = self._lists(rng)

    def csr(self, quantised_values=False):
        return self.rowptr, self.col, self.val_q if quantised_values else self.val

    def transposed(self, quantised_values=False):
        return R.transpose_csr(*self.csr(quantised_values), self.n)

    def _lists(self, rng):
        n, core = self.n, self.core
        every = np.concatenate([rng.permutation(n), rng.integers(0, n, 16384 - n)])
        a_leader = int(core[(core > 100) & (core % 8 == 0)][0])          # an ordinary operand row: its dZ is not zero
        return {
            "core": rng.permutation(np.concatenate([core, rng.choice(core, 300)])),     # shuffled, with repeats
            "one": np.array([a_leader]),
            "n1024": rng.integers(0, n, 1024),                           # the sort pads to 1024: one key per thread
            "n1025": rng.integers(0, n, 1025),                           # ... to 2048: two keys per thread
            "n16384": rng.permutation(every),                            # 16 keys per thread, every row a leader, records = nnz
            "x300": np.full(300, a_leader),                              # one id listed 300 times
            "rec1": np.array([COL_1]), "rec3": np.array([COL_2, COL_1]),
            "rec255": np.array([COL_255]), "rec257": np.array([COL_255, COL_2, COL_255]),
            "hubcol": np.array([COL_1, HUB_COL, 7]),                     # a transposed row far longer than a walk share
            "zero_first": np.array([2100, 7, 4200]), "zero_last": np.array([2100, 8491, 4200]),
            "zero_adjacent": np.array([4200, 3500, 2100, 3000]),         # sorted: 2100, 3000, 3500, 4200
            "zero_only": np.array([9, 7, 8, 8191]),                      # no record at all: every walk share is empty
        }


LIST_NAMES = ("core", "one", "n1024", "n1025", "n16384", "x300", "rec1", "rec3", "rec255", "rec257", "hubcol", "zero_first",
              "zero_last", "zero_adjacent", "zero_only")


def quantised(rng, shape):
    """float32 with 12 significant bits, magnitude in [2^-5, 2^2), random sign."""
    m, e = rng.integers(2 ** 11, 2 ** 12, shape), rng.integers(-16, -9, shape)
    return (rng.choice([-1.0, 1.0], shape) * m * 2.0 ** e).astype(np.float32)


def operands(n, D, seed, g_rows, e_rows):
    """G_in, X_raw, inv_norm, dZ (torch, CPU) after spmm_ref.norm_rows (by row index mod 8: zero rows, rows of norm 1e-13, zero
    dZ, a lone -0.0), inv_norm the float32 a forward pass stores (1e12 exactly on a clamped row).  NaN wherever the hop may
    not read: G_in outside g_rows (the leaders), the epilogue's three outside e_rows."""
    import torch
    G, _, _ = R.norm_rows(n, D, seed)
    X, dZ, clamped = R.norm_rows(n, D, seed + 20)
    inv = torch.from_numpy(R.inv_norm(X)[0].astype(np.float32))
    assert (inv[torch.from_numpy(clamped)] == float(R.INV_CLAMPED)).all() and (inv[torch.from_numpy(~clamped)] < 1e6).all()
    off_g, off_e = torch.ones(n, dtype=torch.bool), torch.ones(n, dtype=torch.bool)
    off_g[torch.as_tensor(np.asarray(g_rows, np.int64))] = False
    off_e[torch.as_tensor(np.asarray(e_rows, np.int64))] = False
    G[off_g], X[off_e], dZ[off_e], inv[off_e] = float("nan"), float("nan"), float("nan"), float("nan")
    return G, X, inv, dZ


def flags_of(n, rows):
    f = np.zeros(n, np.uint8)
    rows = np.asarray(rows, np.int64)
    f[rows[(rows >= 0) & (rows < n)]] = 1
    return f


# ============================================================================================== the cases of the two tests
_CACHE = {}


def ladder():
    if "lad" not in _CACHE:
        _CACHE["lad"] = HopLadder()
    return _CACHE["lad"]


def plan_of(name, quantised_values=False):
    """The reference plan of one named list of the ladder, built once."""
    key = (name, quantised_values)
    if key not in _CACHE:
        lad = ladder()
        _CACHE[key] = Plan(lad.csr(quantised_values), lad.transposed(quantised_values), lad.lists[name])
    return _CACHE[key]


def _seed(name, D):
    return 1000 * LIST_NAMES.index(name) + D


def list_case(name, D):
    """test_hop_against_fp64: row_mask = the marked rows (every destination), dz_flags = the listed rows; operands exist on
    the listed rows only.  -> plan, (G_in, X_raw, inv_norm, dZ), row_mask, dz_flags."""
    plan = plan_of(name)
    ops = operands(plan.n, D, _seed(name, D), plan.leaders, plan.leaders)
    return plan, ops, flags_of(plan.n, plan.dest), flags_of(plan.n, plan.leaders)


MASK_CASES = tuple((m, z) for m in ("full", "cleared") for z in ("none", "subset"))


def mask_case(mask, dz, D):
    """test_hop_masks_and_flags on the core list.  mask "full": every row of the matrix (rows that are no destination stay
    untouched all the same); "cleared": the destinations but every third one with a record, the leader 8191, the first
    listed leader and the long row 2048.  dz "none": dz_flags = None, every visited row takes the term, so the epilogue's
    operands exist on every destination; "subset": every second leader (the others are visited only with a record)."""
    plan, lad = plan_of("core"), ladder()
    if mask == "full":
        row_mask = np.ones(plan.n, np.uint8)
    else:
        row_mask = flags_of(plan.n, plan.dest)
        row_mask[np.flatnonzero(plan.has_record)[::3]] = 0
        row_mask[[lad.special["d0r0_lead"], int(plan.leaders[0]), lad.special["d1025rall"]]] = 0
    sub = plan.leaders[1::2]
    dz_flags = None if dz == "none" else flags_of(plan.n, sub)
    ops = operands(plan.n, D, 7000 + 10 * MASK_CASES.index((mask, dz)) + D, plan.leaders, plan.dest if dz == "none" else sub)
    return plan, ops, row_mask, dz_flags


def order_case(name, D):
    """test_segment_order_is_ascending_bits: the ladder with 12-bit weights, a 12-bit G_in on the leaders, no epilogue term
    anywhere (dz_flags all zero; X_raw, inv_norm and dZ are NaN throughout).  -> plan, G_in (numpy float32, NaN off the
    leaders), short rows to check, long rows to check."""
    plan = plan_of(name, quantised_values=True)
    G = np.full((plan.n, D), np.nan, np.float32)
    G[plan.leaders] = quantised(np.random.default_rng(_seed(name, D) + 5), (len(plan.leaders), D))
    return plan, G, np.flatnonzero(plan.has_record & ~plan.long), np.flatnonzero(plan.long)
