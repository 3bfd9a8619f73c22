"""Time the multi-negative ranking kernels (tagrec_rank_fwd_f32 / tagrec_rank_bwd_f32, csrc/rowops.hip) and the LightGCN step
that uses them, at the C2 shape.

Usage: python tools/rank_loss_microbench.py [--scale 1.0] [--rounds 9] [--steps 20]      (needs a GPU)
  Kernels: B = 512 tuples, D = 64, K = 1, 4, 16, 63 negatives, each loss kind, on compact rows with distinct L2 rows (the
  LightGCN form); forward = rank kernel + the fixed-order reduce, backward = both parts.  All variants interleaved in one
  process: rounds of every variant once, device events around each call, warm-up first; median, minimum and maximum.
  Algorithmic bytes: forward reads (2 + K) B rows of the score and of the L2 operands, backward reads them again and
  writes as many: fwd 2 (2 + K) B D 4, bwd 4 (2 + K) B D 4.  At these sizes (<= 34 MB) everything sits in cache and the
  launches dominate, so the rate is reported for scale only.
  Step: one C2 LightGCN step (1 M x 1 M nodes, 50 M edges, 3 layers, D = 64, batch 512, Adam fused into the last hop) with
  mul_loss_func = "softmax" and K = 1, 4, 16, next to the default triplet step (K = 1, softplus), in the same process on
  the same graph: `--steps` steps between synchronisations per measurement, the variants interleaved over the rounds.
Prints one JSON line per measurement."""
import argparse
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch

import tagrec_amd as T
from tagrec_amd import _lib, rowops

dev = torch.device("cuda:0")
D, B = 64, 512


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


def kernel_variants():
    g = torch.Generator(device=dev).manual_seed(1)
    out = {}
    for K in (1, 4, 16, 63):
        Ub, Ib = torch.randn(B, D, device=dev, generator=g) * 0.3, torch.randn((1 + K) * B, D, device=dev, generator=g) * 0.3
        Ur, Ir = torch.randn(B, D, device=dev, generator=g) * 0.1, torch.randn((1 + K) * B, D, device=dev, generator=g) * 0.1
        dU, dI, dUr, dIr = (torch.empty_like(t) for t in (Ub, Ib, Ur, Ir))
        up = torch.tensor([1.0, 1e-3], device=dev)
        for name, kind in (("softmax", _lib.LOSS_SOFTMAX), ("softplus", _lib.LOSS_SOFTPLUS), ("logsigmoid", _lib.LOSS_LOGSIGMOID)):
            _, coef = rowops.rank_fwd(Ub, Ib, Ur, Ir, kind, 0.5)
            out[f"fwd_{name}_K{K}"] = (lambda Ub=Ub, Ib=Ib, Ur=Ur, Ir=Ir, kind=kind: rowops.rank_fwd(Ub, Ib, Ur, Ir, kind, 0.5))
            if name == "softmax":       # the backward does not depend on the kind
                out[f"bwd_K{K}"] = (lambda Ub=Ub, Ib=Ib, Ur=Ur, Ir=Ir, coef=coef, dU=dU, dI=dI, dUr=dUr, dIr=dIr:
                                    rowops.rank_bwd(Ub, Ib, Ur, Ir, coef, up, dU, dI, dUr, dIr))
    return out


def step_variants(scale, steps):
    nu = ni = max(int(1_000_000 * scale), 2000)
    ne = max(int(50_000_000 * scale), 40000)
    ds = T.synth.make_bipartite_device(nu, ni, ne, seed=1, device=dev)
    e = ds.edge_index["train"]
    rp, col, val, n = T.graph.bipartite_norm_device(e[:, 0], e[:, 1], nu, ni, "bi_norm")
    G = T.Graph(rp, col, val, (n, n), symmetric=True)
    G.transpose()
    out, info = {}, {"users": nu, "items": ni, "edges": int(e.shape[0]), "nnz": int(rp[-1])}
    for name, kw in [("triplet_softplus_K1", {})] + [(f"softmax_K{K}", dict(mul_loss_func="softmax", n_negatives=K,
                                                                           loss_temperature=0.5)) for K in (1, 4, 16)]:
        cfg = T.get_config("lightgcn", use_tag=False, dim_latent=D, dim_layer_list=[D] * 3, device=dev, train_batch=B, **kw)
        torch.manual_seed(cfg["seed"])
        model = T.LightGCN(ds, config=cfg, graph=G).train()
        opt = T.Adam(model.parameters(), lr=cfg["lr"])
        opt.fuse_into(model)
        epoch = T.BPR_training_data(ds, config=cfg, seed=2020).all_train_data
        batches = [epoch[k * B:(k + 1) * B] for k in range(steps)]
        assert batches[0].shape == (B, 2 + cfg["n_negatives"]) and batches[0].numel() * 16 <= n       # the compact path

        def run(model=model, opt=opt, batches=batches):
            for b in batches:
                lossx = model.loss(b)
                opt.zero_grad()
                sum(lossx).backward()
                opt.step()
        out[name] = run
    return out, info


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--scale", type=float, default=1.0, help="shrink the C2 graph (nodes and edges)")
    ap.add_argument("--rounds", type=int, default=9)
    ap.add_argument("--steps", type=int, default=20, help="steps per measurement of the step leg")
    ap.add_argument("--no-step", action="store_true", help="kernels only")
    a = ap.parse_args()
    print(json.dumps({"B": B, "D": D, "device": torch.cuda.get_device_name(0), "rounds": a.rounds}), flush=True)
    for k, (med, lo, hi) in interleaved(kernel_variants(), a.rounds, 3).items():
        K = int(k.rsplit("K", 1)[1])
        nbytes = (2 if k.startswith("fwd") else 4) * (2 + K) * B * D * 4
        print(json.dumps({"leg": "kernel", "variant": k, "K": K, "median_us": round(med * 1e3, 2), "min_us": round(lo * 1e3, 2),
                          "max_us": round(hi * 1e3, 2), "algorithmic_MB": round(nbytes / 1e6, 3),
                          "algorithmic_GBps": round(nbytes / (med * 1e-3) / 1e9, 1)}), flush=True)
    if not a.no_step:
        variants, info = step_variants(a.scale, a.steps)
        print(json.dumps(dict(shape="C2", scale=a.scale, steps_per_measurement=a.steps, **info)), flush=True)
        res = interleaved(variants, a.rounds, 1)
        base = res["triplet_softplus_K1"][0]
        for k, (med, lo, hi) in res.items():
            print(json.dumps({"leg": "lightgcn_step", "variant": k, "median_ms_per_step": round(med / a.steps, 4),
                              "min_ms_per_step": round(lo / a.steps, 4), "max_ms_per_step": round(hi / a.steps, 4),
                              "ratio_to_triplet": round(med / base, 4)}), flush=True)
