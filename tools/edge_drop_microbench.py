"""Time edge dropout inside the products (`node_drop_mode="kernel"`, Graph.edge_drop) at the C2 shape.

Usage: python tools/edge_drop_microbench.py [--scale 1.0] [--skip-step] [--skip-rebuild]      (needs a GPU)
  layer legs : the all-rows fused layer (SpMM + normalise + layer mean, D = 64) on the plain graph and on the edge-drop view
               at p = 0 / 0.1 / 0.3 -- rounds of all variants interleaved in one process, median and minimum per variant;
  step legs  : one LightGCN training step (3 layers, D = 64, batch 512, fused Adam where the path has it) with node_drop = 0,
               node_drop = 0.1 in kernel mode and node_drop = 0.1 in rebuild mode (the CSR and its transpose rebuilt per step).
Device events around each repetition, warm-up first.  Prints one JSON line per measurement."""
import argparse
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch

import tagrec_amd as T

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


def layer_legs(G, n, D, rounds):
    x = torch.randn(n, D, device=dev, generator=torch.Generator(device=dev).manual_seed(1)) * 0.1
    y, inv, acc = torch.empty_like(x), torch.empty(n, device=dev), torch.zeros_like(x)
    variants = {"plain": lambda: G.spmm_norm_acc(x, y, inv, acc, 0.25)}
    for p in (0.0, 0.1, 0.3):
        view = G.edge_drop(p, 7)
        variants[f"kernel_p{p}"] = (lambda v: lambda: v.spmm_norm_acc(x, y, inv, acc, 0.25))(view)
    res = interleaved(variants, rounds, 3)
    base = res["plain"][0]
    for k, (med, lo) in res.items():
        print(json.dumps({"leg": "all_rows_layer", "variant": k, "D": D, "nnz": G.nnz, "median_ms": round(med, 4),
                          "min_ms": round(lo, 4), "ratio_to_plain": round(med / base, 4)}), flush=True)


def step_legs(ds, G, D, L, B, rounds, rebuild):
    modes = [("node_drop_0", dict(node_drop=0.0)), ("kernel_p0.1", dict(node_drop=0.1, node_drop_mode="kernel"))]
    if rebuild:
        modes.append(("rebuild_p0.1", dict(node_drop=0.1, node_drop_mode="rebuild")))
    steps = {}
    for name, kw in modes:
        cfg = T.get_config("lightgcn", use_tag=False, dim_latent=D, dim_layer_list=[D] * L, device=dev, train_batch=B, **kw)
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
        steps[name] = step
    slow = {k: v for k, v in steps.items() if k.startswith("rebuild")}
    fast = {k: v for k, v in steps.items() if k not in slow}
    res = interleaved(fast, rounds, 3)
    if slow:
        res.update(interleaved(slow, 3, 1))
    base = res["node_drop_0"][0]
    for k, (med, lo) in res.items():
        print(json.dumps({"leg": "lightgcn_step", "variant": k, "D": D, "layers": L, "batch": B, "median_ms": round(med, 3),
                          "min_ms": round(lo, 3), "ratio_to_node_drop_0": round(med / base, 4)}), flush=True)
    if slow:
        print(json.dumps({"leg": "lightgcn_step", "kernel_over_rebuild": round(res["kernel_p0.1"][0] / res["rebuild_p0.1"][0], 4)}),
              flush=True)


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--scale", type=float, default=1.0, help="shrink the C2 graph (nodes and edges)")
    ap.add_argument("--rounds", type=int, default=11)
    ap.add_argument("--skip-step", action="store_true")
    ap.add_argument("--skip-rebuild", action="store_true")
    a = ap.parse_args()
    nu = ni = max(int(1_000_000 * a.scale), 2000)
    ne = max(int(50_000_000 * a.scale), 40000)
    ds = T.synth.make_bipartite_device(nu, ni, ne, seed=1, device=dev)
    e = ds.edge_index["train"]
    rp, col, val, n = T.graph.bipartite_norm_device(e[:, 0], e[:, 1], nu, ni, "bi_norm")
    G = T.Graph(rp, col, val, (n, n), symmetric=True)
    print(json.dumps({"shape": "C2", "scale": a.scale, "n": n, "nnz": G.nnz, "device": torch.cuda.get_device_name(0)}), flush=True)
    layer_legs(G, n, 64, a.rounds)
    if not a.skip_step:
        step_legs(ds, G, 64, 3, 512, a.rounds, not a.skip_rebuild)
