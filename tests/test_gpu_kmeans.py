"""GPU: the nearest-centroid assignment kernel (csrc/kmeans.hip) through rowops.kmeans_assign, and tagrec_amd.kmeans
(kmeans.py), against the fp64 restatement of tests/ncl_torch.py.

Tolerance: this repository's rule: |got - ref64| <= c * 2^-24 * mag, `c` counted off the kernels as built.

  score s_ij      x_i . c_j is a D-term MFMA chain (fmaf, ascending feature blocks; padded columns add exact zeros): D roundings
                  on sum_d |x_id c_jd|.  h_j = 0.5 |c_j|^2 is a D-term fmaf chain (D roundings on its own value; the product
                  with 0.5 is exact).  s = dot - h is one subtraction, on at most mag.  c = D + 1, and one more for the
                  second-order terms of the two chains:  c = D + 2  on  mag = sum_d |x_id c_jd| + 0.5 sum_d c_jd^2.
  assign          equality of indices with the fp64 argmax is the wrong test: on near ties the fp32 scores order differently.
                  Asserted for EVERY row: s64(i, assign_i) >= max_j s64(i, j) - (bound(i, assign_i) + bound(i, j*)).
  best            |best_i - s64(i, assign_i)| <= bound(i, assign_i).
  centroid        one M-step from the kernel's own assignment: a cluster of m rows is summed by the fixed-order scatter, whose
                  contract (include/tagrec.h) is chains of <= 1024 slots added left to right: min(m, 1024) - 1 adds in a
                  chain, ceil(m / 1024) - 1 adds of chunk sums, and the divide: c = min(m, 1024) + ceil(m / 1024) - 1 on
                  sum |x_id| / m.  The count is exact (m < 2^24 converts exactly).
Each test prints its worst err / bound (`-s`)."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import tagrec_amd as T
from tagrec_amd import rowops

import ncl_torch as NT
from spmm_ref import U32, Chk, f64, randn, same_bits

DEV = torch.device("cuda:0")
NS = (1, 63, 64, 65, 130, 1000)         # both sides of the row tile; 130: three blocks; 1000: 16 blocks, the last ragged
KS = (1, 2, 63, 64, 65, 130, 1000)      # both sides of the walked tile
DS = (8, 64, 100, 256)                  # 1, 4, 8, 16 accumulator tiles; 100 is ragged (Dp = 112)


def _c(D):
    return D + 2


def _ref(X, C):
    x, c = f64(X), f64(C)
    h = 0.5 * (c * c).sum(1)
    return x @ c.T - h[None, :], np.abs(x) @ np.abs(c).T + h[None, :]


def _check(chk, what, X, C, assign, best, chk_assign=None):
    """The criterion of the header for every row (its ratio goes to `chk_assign` when given, so that the two figures can be
    told apart); -> number of rows whose id differs from the fp64 argmax."""
    n, D = X.shape
    K = C.shape[0]
    s, mag = _ref(X, C)
    a = assign.cpu().numpy()
    assert a.dtype == np.int64 and ((a >= 0) & (a < K)).all(), f"{what}: an id outside [0, {K})"
    i = np.arange(n)
    js = s.argmax(1)
    bound = _c(D) * U32 * mag
    # gap <= slack, as a Chk ratio: got = s64 at the kernel's id, ref = the fp64 maximum
    (chk_assign or chk).close(what + " assign", s[i, a], s[i, js], 1.0, 0, bound[i, a] + bound[i, js])
    chk.close(what + " best", best, s[i, a], mag[i, a], _c(D))
    return int((a != js).sum())


def _operands(n, K, D, scale, near, seed):
    X = randn(n, D, seed=seed, scale=scale)
    if near:                            # centroids = data rows + 1e-3 (relative) noise: near ties all over
        C = X[torch.arange(K) % n] + randn(K, D, seed=seed + 1, scale=1e-3 * scale)
    else:
        C = randn(K, D, seed=seed + 1, scale=scale)
    return X.contiguous(), C.contiguous()


@pytest.mark.parametrize("near", (False, True), ids=("random", "near_tie"))
@pytest.mark.parametrize("D", DS)
def test_assign_against_fp64(D, near):
    chk = Chk(f"kmeans_assign best D={D} {'near-tie' if near else 'random'}", "kmeans")
    chk_a = Chk(f"kmeans_assign gap / allowance D={D} {'near-tie' if near else 'random'}", "kmeans")
    flips = rows = 0
    for scale in (1.0, 0.01):
        for n in NS:
            for K in KS:
                X, C = _operands(n, K, D, scale, near, seed=1000 * n + K)
                a, b = rowops.kmeans_assign(X.to(DEV), C.to(DEV))
                flips += _check(chk, f"n={n} K={K} s={scale}", X, C, a, b, chk_a)
                rows += n
    print(f"[kmeans] D={D}: {flips} of {rows} ids differ from the fp64 argmax")
    chk_a.done()
    chk.done()


# duplicated centroid rows (a, b), a < b: the same lane and tile (1, 2), (1, 17); the same tile, another q lane (3, 40);
# another tile, the same lane (5, 69); another tile and lane (5, 70), (5, 130); the last column of a ragged tile (0, 129)
PAIRS = ((1, 2), (1, 17), (3, 40), (5, 69), (5, 70), (5, 130), (0, 129))


@pytest.mark.parametrize("D", (8, 64, 100))
def test_ties_go_to_the_lower_id(D):
    for a, b in PAIRS:
        K, n = 131 if b > 129 else 130, 200
        C = randn(K, D, seed=7 * a + b, scale=1.0)
        C[b] = C[a]
        X = randn(n, D, seed=b, scale=1.0)
        X[::2] = C[a] + randn(n // 2, D, seed=a, scale=0.05)         # half of the rows sit on the duplicated centroid
        ids, _ = rowops.kmeans_assign(X.to(DEV), C.to(DEV))
        ids = ids.cpu()
        assert not (ids == b).any(), f"({a}, {b}): a row took the higher of two identical centroids"
        assert (ids[::2] == a).all(), f"({a}, {b})"


@pytest.mark.parametrize("K", (1, 63, 65))
def test_padded_columns_never_win(K):
    """Every true score negative (|c| >> |x|): a padded column's 0 - 0 = 0 would beat them all."""
    chk = Chk(f"kmeans_assign all-negative K={K}", "kmeans")
    for D in (8, 100):
        for n in (1, 65):
            X = randn(n, D, seed=K + n, scale=0.01)
            C = randn(K, D, seed=K + n + 1, scale=1.0)
            s, _ = _ref(X, C)
            assert (s < 0).all()
            a, b = rowops.kmeans_assign(X.to(DEV), C.to(DEV))
            assert (b < 0).all()
            _check(chk, f"n={n} D={D}", X, C, a, b)
    chk.done()


def _slot(t, pad, offset=0):
    """t as a slot of a NaN-filled wider buffer on the GPU: row stride D + pad, the first element `offset` floats in."""
    n, D = t.shape
    buf = torch.full((n * (D + pad) + offset + 8,), float("nan"))
    view = buf[offset:offset + n * (D + pad)].view(n, D + pad)
    view[:, :D] = t
    g = buf.to(DEV)
    return g[offset:offset + n * (D + pad)].view(n, D + pad)[:, :D]


@pytest.mark.parametrize("pad,offset", ((4, 0), (8, 4), (1, 0), (4, 1), (3, 2)),
                         ids=("vec", "vec_offset", "odd_stride", "unaligned_base", "both"))
def test_strided_operands_with_nan_between_the_rows(pad, offset):
    chk = Chk(f"kmeans_assign strided pad={pad} offset={offset}", "kmeans")
    for D in (8, 100):
        for n, K in ((65, 63), (130, 65)):
            X, C = _operands(n, K, D, 1.0, False, seed=n + K + pad)
            Xg, Cg = _slot(X, pad, offset), _slot(C, pad, offset)
            vec = Xg.data_ptr() % 16 == 0 and Xg.stride(0) % 4 == 0
            assert vec == (pad % 4 == 0 and offset % 4 == 0)         # the case is on the staging path its id says
            a, b = rowops.kmeans_assign(Xg, Cg)
            _check(chk, f"n={n} K={K} D={D}", X, C, a, b)
            a2, b2 = rowops.kmeans_assign(X.to(DEV), C.to(DEV))      # the staging path does not change a bit
            assert torch.equal(a, a2) and same_bits(b, b2)
    chk.done()


def test_nothing_past_row_n_is_written_and_two_launches_agree():
    n, K, D, extra = 130, 65, 64, 70
    X, C = _operands(n, K, D, 1.0, True, seed=3)
    Xg, Cg = X.to(DEV), C.to(DEV)
    big_a = torch.full((n + extra,), -7, dtype=torch.int64, device=DEV)
    big_b = torch.full((n + extra,), 123.5, dtype=torch.float32, device=DEV)
    half = torch.full((K + extra,), 321.0, dtype=torch.float32, device=DEV)
    a, b = rowops.kmeans_assign(Xg, Cg, big_a[:n], big_b[:n], half)
    assert a.data_ptr() == big_a.data_ptr() and b.data_ptr() == big_b.data_ptr()
    assert (big_a[n:] == -7).all() and (big_b[n:] == 123.5).all() and (half[K:] == 321.0).all()
    chk = Chk("kmeans_assign prefilled", "kmeans")
    _check(chk, "prefilled", X, C, a, b)
    chk.close("half_norm", half[:K], 0.5 * (f64(C) ** 2).sum(1), 0.5 * (f64(C) ** 2).sum(1), D)
    chk.done()
    a2, b2 = rowops.kmeans_assign(Xg, Cg)
    assert torch.equal(a, a2) and same_bits(b, b2)


def test_multi_block():
    n, K, D = 20000, 130, 64
    X, C = _operands(n, K, D, 1.0, False, seed=11)
    Xg, Cg = X.to(DEV), C.to(DEV)
    a, b = rowops.kmeans_assign(Xg, Cg)
    chk = Chk("kmeans_assign 20000 x 130 x 64", "kmeans")
    _check(chk, "multi-block", X, C, a, b)
    chk.done()
    a2, b2 = rowops.kmeans_assign(Xg, Cg)
    assert torch.equal(a, a2) and same_bits(b, b2)


def _mstep_check(chk, what, X, assign, cents, prev):
    """The centroids of one M-step against the fp64 means of `assign` (the kernel's own), counts included."""
    x, a = f64(X), assign.cpu().numpy()
    k = cents.shape[0]
    counts = np.bincount(a, minlength=k)
    ref, mag, c = f64(prev).copy(), np.abs(f64(prev)), np.zeros((k, 1))
    for j in np.nonzero(counts)[0]:
        m = counts[j]
        ref[j], mag[j] = x[a == j].mean(0), np.abs(x[a == j]).sum(0) / m
        c[j] = min(m, 1024) + -(-m // 1024) - 1
    chk.close(what, cents, ref, mag, c)
    return counts


@pytest.mark.parametrize("n,k,D", ((300, 7, 16), (5000, 3, 64), (1000, 130, 100)))
def test_one_lloyd_step(n, k, D):
    """n_iter = 1 from given centroids; (5000, 3): clusters longer than one 1024-slot chain."""
    X = randn(n, D, seed=n + k, scale=1.0)
    init = X[torch.arange(k) * (n // k)].clone()
    Xg = X.to(DEV)
    a0, _ = rowops.kmeans_assign(Xg, init.to(DEV))                    # what the step's E-step sees
    cents, assign, counts, best = T.kmeans(Xg, k, n_iter=1, centroids=init.to(DEV))
    chk = Chk(f"kmeans one step n={n} k={k} D={D}", "kmeans")
    want = _mstep_check(chk, "centroid", X, a0, cents, init)
    if k == 3:
        assert want.max() > 1024
    # the returned assignment, counts and best belong to the returned centroids
    _check(chk, "final assign", X, cents.cpu(), assign, best)
    assert counts.dtype == torch.int64 and counts.cpu().tolist() == np.bincount(assign.cpu().numpy(), minlength=k).tolist()
    assert int(counts.sum()) == n
    chk.done()


def test_an_empty_cluster_keeps_its_centroid():
    n, k, D = 200, 5, 16
    X = randn(n, D, seed=21, scale=1.0)
    init = X[:k].clone()
    init[3] = 1000.0                                                  # no row is nearest to it
    cents, assign, counts, _ = T.kmeans(X.to(DEV), k, n_iter=3, centroids=init.to(DEV))
    assert int(counts[3]) == 0 and not (assign == 3).any()
    assert same_bits(cents[3].cpu(), init[3])
    assert int(counts.sum()) == n and (counts.cpu()[[0, 1, 2, 4]] > 0).all()
    assert torch.isfinite(cents).all()


def test_kmeans_recovers_the_blobs():
    X, labels, _ = NT.blobs()
    init = torch.stack([X[(labels == b).nonzero()[0, 0]] for b in range(7)])
    cents, assign, counts, best = T.kmeans(X.to(DEV), 7, n_iter=3, centroids=init.to(DEV))
    assert torch.equal(assign.cpu(), labels) and counts.cpu().tolist() == [40] * 7
    chk = Chk("kmeans blobs", "kmeans")
    _mstep_check(chk, "centroid", X, assign, cents, init)             # the blob means: 40 rows, one chain
    _, a64, _, _ = NT.lloyd(X, 7, 3, init)                        # the restatement lands on the same clustering
    assert torch.equal(a64, labels)
    _check(chk, "final", X, cents.cpu(), assign, best)
    chk.done()


def test_seeded_init_and_reproducibility():
    n, k, D = 500, 9, 16
    X = randn(n, D, seed=31, scale=1.0)
    Xg = X.to(DEV)
    g = torch.Generator(device="cpu")
    g.manual_seed(77)
    perm = torch.randperm(n, generator=g)
    cents, assign, counts, best = T.kmeans(Xg, k, n_iter=0, seed=77)
    assert same_bits(cents.cpu(), X[perm[:k]]) and same_bits(cents.cpu(), NT.seeded_init(X, k, 77))
    assert int(counts.sum()) == n
    runs = [T.kmeans(Xg, k, n_iter=4, seed=5) for _ in range(2)]
    for t0, t1 in zip(*runs):
        assert same_bits(t0, t1)
    other = T.kmeans(Xg, k, n_iter=0, seed=6)[0]
    assert not same_bits(other, T.kmeans(Xg, k, n_iter=0, seed=5)[0])


def test_refusals(monkeypatch):
    calls = []
    real = rowops.kmeans_assign
    monkeypatch.setattr(rowops, "kmeans_assign", lambda *a, **kw: (calls.append(1), real(*a, **kw))[1])
    X = torch.zeros(20, 16, device=DEV)
    for bad in (dict(x=X, k=21), dict(x=X, k=0), dict(x=X, k=True), dict(x=torch.zeros(20, 6, device=DEV), k=2),
                dict(x=torch.zeros(20, 260, device=DEV), k=2), dict(x=X.double(), k=2), dict(x=X.cpu(), k=2),
                dict(x=X, k=2, n_iter=-1), dict(x=X, k=2, centroids=torch.zeros(3, 16, device=DEV))):
        with pytest.raises(T.TagrecError):
            T.kmeans(**bad)
    assert not calls                                                  # nothing was launched
    monkeypatch.undo()
    for Xb, Cb in ((torch.zeros(4, 6, device=DEV), torch.zeros(2, 6, device=DEV)),
                   (torch.zeros(4, 260, device=DEV), torch.zeros(2, 260, device=DEV)),
                   (X, torch.zeros(2, 8, device=DEV)), (X.double(), torch.zeros(2, 16, device=DEV).double()),
                   (X, torch.zeros(0, 16, device=DEV)), (X.cpu(), torch.zeros(2, 16))):
        with pytest.raises(T.TagrecError):
            rowops.kmeans_assign(Xb, Cb)
    # the library's own checks (the wrapper's come first): raw calls
    lib = T._lib.load()
    a = torch.empty(20, dtype=torch.int64, device=DEV)
    h = torch.empty(4, dtype=torch.float32, device=DEV)
    s = T._lib.stream_ptr()
    assert lib.tagrec_kmeans_assign_f32(X, 16, 20, X, 16, 4, 6, h, a, None, s) == -3
    assert lib.tagrec_kmeans_assign_f32(X, 16, 20, X, 16, 4, 260, h, a, None, s) == -3
    assert lib.tagrec_kmeans_assign_f32(X, 16, 0, X, 16, 4, 16, h, a, None, s) == -3
    assert lib.tagrec_kmeans_assign_f32(X, 16, 20, X, 16, 0, 16, h, a, None, s) == -3
    assert lib.tagrec_kmeans_assign_f32(X, 16, 20, X, 16, 2 ** 31, 16, h, a, None, s) == -3
    assert lib.tagrec_kmeans_assign_f32(X, 8, 20, X, 16, 4, 16, h, a, None, s) == -1
    a.fill_(-5)
    assert lib.tagrec_kmeans_assign_f32(X, 16, 20, X, 16, 4, 16, h, a, None, s) == 0      # best = NULL is allowed
    assert ((a >= 0) & (a < 4)).all()
