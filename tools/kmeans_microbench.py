"""Time the nearest-centroid assignment kernel (tagrec_kmeans_assign_f32, csrc/kmeans.hip), the M-step and a whole k-means.

Usage: python tools/kmeans_microbench.py [--rounds 9] [--scale 1.0]      (needs a GPU)
  assign      rowops.kmeans_assign at (n, K, D) = (1 M, 1000, 64) and (65 536, 1024, 64); TFLOP/s from 2 n K D.
  catsoftmax  rowops.catsoftmax_fwd at (B, N, D) = (65 536, 1024, 64), the yardstick: the same tile core with an expf where
              the assignment does a compare-select (it launches a combine and a reduce kernel besides, and splits its columns).
  mstep       one M-step of kmeans.py at n = 1 M, K = 1000: the row-list plan of the assignment, the fixed-order scatter, the
              integer counts and the divide.
  kmeans      T.kmeans(x [1 M, 64], 1000, n_iter = 20): 21 assignments and 20 M-steps.
  All variants interleaved in one process: rounds of every variant once, device events around each call, warm-up first;
  median, minimum and maximum.  Prints one JSON line per measurement."""
import argparse
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch

import tagrec_amd as T
from tagrec_amd import rowops

dev = torch.device("cuda:0")
D = 64


def event_ms(fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b)


def interleaved(variants, rounds, warmup):
    """{name: fn} -> {name: (median, min, max)} over `rounds` rounds, each running every variant once."""
    for _ in range(warmup):
        for fn in variants.values():
            fn()
    torch.cuda.synchronize()
    ms = {k: [] for k in variants}
    for _ in range(rounds):
        for k, fn in variants.items():
            ms[k].append(event_ms(fn))
    return {k: (sorted(v)[len(v) // 2], min(v), max(v)) for k, v in ms.items()}


def randn(n, d, seed):
    return torch.randn(n, d, device=dev, generator=torch.Generator(device=dev).manual_seed(seed)) * 0.1


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=9)
    ap.add_argument("--scale", type=float, default=1.0, help="shrink the row counts")
    ap.add_argument("--iters", type=int, default=20)
    a = ap.parse_args()
    n_big, n_small, K_big, K_small = max(int(1_000_000 * a.scale), 1000), max(int(65_536 * a.scale), 64), 1000, 1024
    print(json.dumps(dict(D=D, device=torch.cuda.get_device_name(0), rounds=a.rounds, scale=a.scale)), flush=True)

    Xb, Cb = randn(n_big, D, 1), randn(K_big, D, 2)
    Xs, Cs = randn(n_small, D, 3), randn(K_small, D, 4)
    ab, bb, hb = torch.empty(n_big, dtype=torch.int64, device=dev), torch.empty(n_big, device=dev), torch.empty(K_big, device=dev)
    as_, bs, hs = torch.empty(n_small, dtype=torch.int64, device=dev), torch.empty(n_small, device=dev), torch.empty(K_small, device=dev)
    tgt = torch.randint(0, K_small, (n_small,), device=dev)
    ws = torch.empty(rowops.catsoftmax_workspace(n_small, K_small, D), dtype=torch.uint8, device=dev)
    rowops.kmeans_assign(Xb, Cb, ab, bb, hb)
    plan_ws = torch.empty(rowops.row_list_workspace(n_big, D), dtype=torch.uint8, device=dev)
    sums = torch.empty(K_big, D, device=dev)
    counts, ones = torch.empty(K_big, dtype=torch.int64, device=dev), torch.ones(n_big, dtype=torch.int64, device=dev)

    def mstep():
        plan = rowops.row_list_plan(ab, K_big, plan_ws, D)
        sums.zero_()
        rowops.scatter_rows_ordered(sums, plan, Xb, accumulate=False)
        counts.zero_()
        counts.index_add_(0, ab, ones)
        return torch.where((counts > 0)[:, None], sums / counts.clamp(min=1).to(torch.float32)[:, None], Cb)

    variants = {
        "assign_1m_1000": lambda: rowops.kmeans_assign(Xb, Cb, ab, bb, hb),
        "assign_64k_1024": lambda: rowops.kmeans_assign(Xs, Cs, as_, bs, hs),
        "catsoftmax_fwd_64k_1024": lambda: rowops.catsoftmax_fwd(Xs, Cs, tgt, 1.0, workspace=ws),
        "mstep_1m_1000": mstep,
    }
    flops = {"assign_1m_1000": 2.0 * n_big * K_big * D, "assign_64k_1024": 2.0 * n_small * K_small * D,
             "catsoftmax_fwd_64k_1024": 2.0 * n_small * K_small * D}
    res = interleaved(variants, a.rounds, 3)
    for k, (med, lo, hi) in res.items():
        row = {"leg": "kernel", "variant": k, "median_ms": round(med, 4), "min_ms": round(lo, 4), "max_ms": round(hi, 4)}
        if k in flops:
            row["tflops_median"] = round(flops[k] / (med * 1e-3) / 1e12, 3)
        if k == "assign_64k_1024":
            row["ratio_to_catsoftmax_fwd"] = round(med / res["catsoftmax_fwd_64k_1024"][0], 4)
        print(json.dumps(row), flush=True)
    res = interleaved({"kmeans": lambda: T.kmeans(Xb, K_big, n_iter=a.iters, seed=1)}, max(3, a.rounds // 3), 1)
    med, lo, hi = res["kmeans"]
    print(json.dumps({"leg": "kmeans", "n": n_big, "k": K_big, "n_iter": a.iters, "median_ms": round(med, 3), "min_ms": round(lo, 3),
                      "max_ms": round(hi, 3)}), flush=True)
