"""k-means (Lloyd's algorithm) on the device: the clustering step of prototype contrast (ncl.py).

    kmeans(x, k, n_iter=20, seed=0, centroids=None) -> (centroids [k, D] fp32, assign int64 [n], counts int64 [k], best [n])

Nothing is read back to the host after the initial draw, so a call is n_iter + 1 assignment launches and n_iter M-steps
enqueued on the current stream.

  init          `centroids` if given, else x[perm[:k]] with perm = torch.randperm(n, generator = a CPU generator seeded with
                `seed`): k distinct rows.
  E-step        `rowops.kmeans_assign` (csrc/kmeans.hip): the Euclidean nearest centroid, ties to the lower id.
  M-step        per-cluster sums through the fixed-order scatter (`rowops.row_list_plan` of the assignment +
                `rowops.scatter_rows_ordered`, 1024-slot chains added left to right: the same bits on every run), exact
                integer counts by an int64 `index_add_`, c_j = sums_j / count_j as one fp32 divide.
  empty cluster A cluster with no member KEEPS ITS PREVIOUS CENTROID (faiss splits a large cluster instead; this rule is
                simpler, needs no host read and leaves the result a pure function of the inputs).  Its count is 0.
  final pass    After the last update one more assignment runs, so that `assign`, `counts` and `best` belong to the returned
                centroids.  best[i] = x_i . c - 0.5 |c|^2 of the winner; the inertia is sum_i |x_i|^2 - 2 best_i.
"""
import torch

from . import _lib, rowops


def seeded_rows(n, k, seed):
    """The k distinct row ids of the seeded init: torch.randperm(n) under a CPU generator seeded with `seed`, cut at k."""
    gen = torch.Generator(device="cpu")
    gen.manual_seed(int(seed))
    return torch.randperm(n, generator=gen)[:k]


def _count(assign, counts, ones):
    counts.zero_()
    return counts.index_add_(0, assign, ones)           # integer atomics: exact, whatever the order


def kmeans(x, k, n_iter=20, seed=0, centroids=None):
    what = "kmeans"
    if not isinstance(x, torch.Tensor) or not x.is_cuda or x.dtype != torch.float32 or x.dim() != 2:
        raise _lib.TagrecError(f"{what}: x must be a 2-d float32 GPU tensor (tagrec_amd has no CPU path)")
    if x.shape[1] > 1 and x.stride(1) != 1:
        raise _lib.TagrecError(f"{what}: x must have unit inner stride, got {x.stride(1)}")
    n, D = x.shape
    if isinstance(k, bool) or not isinstance(k, int) or k < 1:
        raise _lib.TagrecError(f"{what}: k must be an integer >= 1, got {k!r}")
    if k > n:
        raise _lib.TagrecError(f"{what}: k = {k} clusters need at least as many rows, got n = {n}")
    if D < 8 or D > 256 or D % 4 != 0:
        raise _lib.TagrecError(f"{what}: the width must be a multiple of 4 in 8 .. 256, got {D}")
    if isinstance(n_iter, bool) or not isinstance(n_iter, int) or n_iter < 0:
        raise _lib.TagrecError(f"{what}: n_iter must be an integer >= 0, got {n_iter!r}")
    dev = x.device
    if centroids is None:
        c = x.index_select(0, seeded_rows(n, k, seed).to(dev))
    else:
        if not isinstance(centroids, torch.Tensor) or not centroids.is_cuda or centroids.dtype != torch.float32 \
                or centroids.shape != (k, D) or centroids.device != dev:
            raise _lib.TagrecError(f"{what}: centroids must be a float32 tensor of shape [{k}, {D}] on {dev}")
        c = centroids.detach().clone().contiguous()
    assign = torch.empty(n, dtype=torch.int64, device=dev)
    best = torch.empty(n, dtype=torch.float32, device=dev)
    half = torch.empty(k, dtype=torch.float32, device=dev)
    counts = torch.empty(k, dtype=torch.int64, device=dev)
    ones = torch.ones(n, dtype=torch.int64, device=dev)
    if n_iter > 0:
        plan_ws = torch.empty(rowops.row_list_workspace(n, D), dtype=torch.uint8, device=dev)      # once per call
        sums = torch.empty(k, D, dtype=torch.float32, device=dev)
    for _ in range(n_iter):
        rowops.kmeans_assign(x, c, assign, best, half)
        plan = rowops.row_list_plan(assign, k, plan_ws, D)
        sums.zero_()                                    # the scatter leaves a cluster without members untouched
        rowops.scatter_rows_ordered(sums, plan, x, accumulate=False)
        _count(assign, counts, ones)
        # one fp32 divide; a cluster without members keeps its previous row
        c = torch.where((counts > 0)[:, None], sums / counts.clamp(min=1).to(torch.float32)[:, None], c)
    rowops.kmeans_assign(x, c, assign, best, half)
    _count(assign, counts, ones)
    return c, assign, counts, best
