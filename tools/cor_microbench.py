"""Time forward + backward of `help.cor_loss` (csrc/cor.hip) against the operator form that materialises the K n x n
distance matrices (torch ops on the GPU, autograd), and one DGCF step with the term off and on.

Usage: python tools/cor_microbench.py [--sizes 300,3000,30000] [--skip-dgcf]      (needs a GPU)
Per size (D = 64, K = 4): median ms over the timed repetitions after warm-up, device events around forward + backward,
the loss of both forms, and the rate of pair evaluations (3 passes x n^2 x K) / time of the kernels.  The DGCF legs time whole steps (loss, backward,
Adam) on a synthetic graph at cor_batch 100 and 4096.  Prints one JSON line per measurement."""
import argparse
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch

import tagrec_amd as T
from tagrec_amd import help as H

dev = torch.device("cuda:0")


def operator_form(X, K):
    """The same loss on torch operators: squared distances from one matmul per slice, K centred n x n matrices."""
    n = X.shape[0]
    A = []
    for x in torch.split(X, X.shape[1] // K, dim=1):
        r = (x * x).sum(1, keepdim=True)
        d = torch.sqrt(torch.clamp(r - 2 * x @ x.t() + r.t(), min=0) + 1e-8)
        A.append(d - d.mean(0, keepdim=True) - d.mean(1, keepdim=True) + d.mean())
    cov = lambda a, b: torch.sqrt(torch.clamp((a * b).sum() / (n * n), min=0) + 1e-8)
    loss = 0
    for f in range(K - 1):
        loss = loss + cov(A[f], A[f + 1]) / (torch.sqrt(torch.clamp(cov(A[f], A[f]) * cov(A[f + 1], A[f + 1]), min=0)) + 1e-10)
    return loss / ((K + 1.0) * K / 2)


def timed(fn, reps, warmup):
    for _ in range(warmup):
        out = fn()
    torch.cuda.synchronize()
    ms = []
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        out = fn()
        b.record()
        torch.cuda.synchronize()
        ms.append(a.elapsed_time(b))
    return sorted(ms)[len(ms) // 2], out


def fwd_bwd(loss_fn, X, K):
    def run():
        x = X.detach().requires_grad_(True)
        loss = loss_fn(x, K)
        loss.backward()
        return loss.detach()
    return run


def bench_sizes(sizes, D=64, K=4):
    for n in sizes:
        X = torch.nn.functional.normalize(torch.randn(n, D, device=dev, generator=torch.Generator(device=dev).manual_seed(n)), dim=1) * 0.5
        reps, warmup = (20, 3) if n <= 3000 else (5, 1)
        res = {"n": n, "D": D, "K": K}
        ms, loss = timed(fwd_bwd(H.cor_loss, X, K), reps, warmup)
        res.update(kernel_ms=round(ms, 4), kernel_loss=float(loss), kernel_gpairs_per_s=round(3 * n * n * K / ms / 1e6, 2))
        try:
            ms_op, loss_op = timed(fwd_bwd(operator_form, X, K), reps, warmup)
            res.update(operator_ms=round(ms_op, 4), operator_loss=float(loss_op), speedup=round(ms_op / ms, 2))
        except torch.OutOfMemoryError:
            res.update(operator_ms=None, operator_note="out of memory")
        torch.cuda.empty_cache()
        print(json.dumps(res), flush=True)


def bench_dgcf():
    ds = T.synth.make_cf_dataset(30000, 20000, 600_000, seed=3, n_tag=5000, n_assign=100_000)
    for cor_batch in (100, 4096):
        for on in (False, True):
            cfg = T.get_config("dgcf", device=dev, train_batch=1024, use_tag=True, dim_layer_list=[64, 64], reg=1e-3,
                               cor_batch=cor_batch, cor_loss=on, cor_reg=1e-2)
            torch.manual_seed(1)
            m = T.DGCF(ds, config=cfg)
            m.train()
            opt = T.Adam(m.parameters(), lr=0.01)
            prod = T.DGCF_training_data(ds, config=cfg, seed=4)
            batch = prod.mini_sample()

            def step():
                opt.zero_grad()
                parts = m.loss(batch)
                sum(parts).backward()
                opt.step()
                return parts
            ms, parts = timed(step, 10, 3)
            print(json.dumps({"dgcf_step_ms": round(ms, 3), "cor_loss": on, "cor_batch": cor_batch, "cor_rows": int(batch[1].numel()),
                              "parts": [float(p.detach()) for p in parts]}), flush=True)


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", default="300,3000,30000")
    ap.add_argument("--skip-dgcf", action="store_true")
    a = ap.parse_args()
    bench_sizes([int(s) for s in a.sizes.split(",") if s])
    if not a.skip_dgcf:
        bench_dgcf()
