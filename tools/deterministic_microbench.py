"""Time what config["deterministic"] = True costs a LightGCN training step at the C2 shape.

Usage: python tools/deterministic_microbench.py [--scale 1.0] [--rounds 21] [--batch 512]      (needs a GPU)
  One LightGCN step (3 layers, D = 64, fused Adam where the path has it) in default and in deterministic mode, with reg = 0
  and reg > 0, on the same graph and the same batch; rounds of all variants interleaved in one process, device events around
  each step, warm-up first; median and minimum per variant.  Also the plan and one ordered scatter on their own, next to the
  `index_add_` they replace.  Prints one JSON line per measurement."""
import argparse
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch

import tagrec_amd as T
from tagrec_amd import rowops

dev = torch.device("cuda:0")


def event_ms(fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b)


def interleaved(variants, rounds, warmup):
    """{name: fn} -> {name: (median, min)} over `rounds` rounds, each running every variant once."""
    for _ in range(warmup):
        for fn in variants.values():
            fn()
    torch.cuda.synchronize()
    ms = {k: [] for k in variants}
    for _ in range(rounds):
        for k, fn in variants.items():
            ms[k].append(event_ms(fn))
    return {k: (sorted(v)[len(v) // 2], min(v)) for k, v in ms.items()}


def step_legs(ds, G, D, L, B, rounds):
    steps = {}
    for reg in (0.0, 1e-3):
        for det in (False, True):
            cfg = T.get_config("lightgcn", use_tag=False, dim_latent=D, dim_layer_list=[D] * L, device=dev, train_batch=B, reg=reg,
                               deterministic=det)
            torch.manual_seed(cfg["seed"])
            model = T.LightGCN(ds, config=cfg, graph=G)
            model.train()
            opt = T.Adam(model.parameters(), lr=cfg["lr"])
            opt.fuse_into(model)
            batch = T.BPR_training_data(ds, config=cfg, seed=2020).all_train_data[:B].contiguous()

            def step(model=model, opt=opt, batch=batch):
                lossx = model.loss(batch)
                opt.zero_grad()
                sum(lossx).backward()
                opt.step()
            steps[f"reg{reg:g}_{'deterministic' if det else 'default'}"] = step
    res = interleaved(steps, rounds, 3)
    for k, (med, lo) in res.items():
        base = res[k.split("_")[0] + "_default"][0]
        print(json.dumps({"leg": "lightgcn_step", "variant": k, "D": D, "layers": L, "batch": B, "median_ms": round(med, 3),
                          "min_ms": round(lo, 3), "ratio_to_default": round(med / base, 4)}), flush=True)


def fold_legs(n, D, B, rounds):
    g = torch.Generator(device=dev).manual_seed(1)
    rows = torch.randint(0, n, (3 * B,), device=dev, generator=g)
    rows[: B // 2] = rows[0]                                   # a popular row
    src = torch.randn(3 * B, D, device=dev, generator=g)
    dst = torch.zeros(n, D, device=dev)
    ws = torch.empty(rowops.row_list_workspace(3 * B, D), dtype=torch.uint8, device=dev)
    plan = rowops.row_list_plan(rows, n, ws, D)
    res = interleaved({"row_list_plan": lambda: rowops.row_list_plan(rows, n, ws, D),
                       "scatter_rows_ordered": lambda: rowops.scatter_rows_ordered(dst, plan, src, True),
                       "index_add_": lambda: dst.index_add_(0, rows, src)}, rounds, 3)
    for k, (med, lo) in res.items():
        print(json.dumps({"leg": "fold", "variant": k, "rows": 3 * B, "D": D, "median_ms": round(med, 4), "min_ms": round(lo, 4)}),
              flush=True)


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--scale", type=float, default=1.0, help="shrink the C2 graph (nodes and edges)")
    ap.add_argument("--rounds", type=int, default=21)
    ap.add_argument("--batch", type=int, default=512)
    a = ap.parse_args()
    nu = ni = max(int(1_000_000 * a.scale), 2000)
    ne = max(int(50_000_000 * a.scale), 40000)
    ds = T.synth.make_bipartite_device(nu, ni, ne, seed=1, device=dev)
    e = ds.edge_index["train"]
    rp, col, val, n = T.graph.bipartite_norm_device(e[:, 0], e[:, 1], nu, ni, "bi_norm")
    G = T.Graph(rp, col, val, (n, n), symmetric=True)
    print(json.dumps({"shape": "C2", "scale": a.scale, "n": n, "nnz": G.nnz, "device": torch.cuda.get_device_name(0)}), flush=True)
    fold_legs(n, 64, a.batch, a.rounds)
    step_legs(ds, G, 64, 3, a.batch, a.rounds)
