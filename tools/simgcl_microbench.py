"""Time the noise form of the fused LightGCN layer (tagrec_spmm_norm_acc_noise_f32, csrc/spmm.hip) and the SimGCL step at the
C2 shape.

Usage: python tools/simgcl_microbench.py [--scale 1.0] [--rounds 9] [--steps 10]      (needs a GPU)
  Layer (1 M x 1 M nodes, 50 M edges, D = 64; every variant writes the raw rows and the inverse norms of all rows):
    plain     Graph.spmm_norm_acc_rows(acc = None, no mask): the launch the LightGCN step makes for a lower layer
    noise     Graph.spmm_norm_acc_noise(acc = None, no mask): the same with the perturbation in the epilogue
    unfused   the alternative without the fused form: plain product (Graph.spmm), then a separate elementwise pass --
              rowops.noise_dir materialises the [N, D] directions, torch adds eps sign(y) n in place -- then rowops.rownorm_fwd
  All variants interleaved in one process: rounds of every variant once, device events around each call, warm-up first;
  median, minimum and maximum.
  Step: one SimGCL step (3 layers, batch 512, Adam as a separate launch: the fused update is refused) next to the LightGCN
  step on the same graph with the same optimizer form, and with Adam fused into the last hop (the default benchmark's form);
  `--steps` steps between synchronisations per measurement, the variants interleaved over the rounds.
Prints one JSON line per measurement."""
import argparse
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch

import tagrec_amd as T
from tagrec_amd import rowops

dev = torch.device("cuda:0")
D, EPS, SEED = 64, 0.1, (2020 << 24) + 1


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


def make_graph(scale):
    nu = ni = max(int(1_000_000 * scale), 2000)
    ne = max(int(50_000_000 * scale), 40000)
    ds = T.synth.make_bipartite_device(nu, ni, ne, seed=1, device=dev)
    e = ds.edge_index["train"]
    rp, col, val, n = T.graph.bipartite_norm_device(e[:, 0], e[:, 1], nu, ni, "bi_norm")
    G = T.Graph(rp, col, val, (n, n), symmetric=True)
    G.transpose()
    return ds, G, {"users": nu, "items": ni, "edges": int(e.shape[0]), "nnz": int(rp[-1])}


def layer_variants(G):
    n = G.shape[0]
    X = torch.randn(n, D, device=dev, generator=torch.Generator(device=dev).manual_seed(1)) * 0.1
    Y, inv, Z = torch.empty_like(X), torch.empty(n, device=dev), torch.empty_like(X)

    def plain():
        G.spmm_norm_acc_rows(X, Y, inv, None, 0.0, None)

    def noise():
        G.spmm_norm_acc_noise(X, Y, inv, None, 0.0, None, EPS, SEED, 0, 1)

    def unfused():
        G.spmm(X, Y)
        nd = rowops.noise_dir(n, D, SEED, 0, 1, dev)
        Y.addcmul_(torch.sign(Y), nd, value=EPS)
        rowops.rownorm_fwd(Y, Z, inv)
    return {"plain": plain, "noise": noise, "unfused": unfused}


def step_variants(ds, G, steps, B=512):
    out = {}
    for name, model_name, cls, fuse in (("lightgcn_fused_adam", "lightgcn", T.LightGCN, True), ("lightgcn", "lightgcn", T.LightGCN, False),
                                        ("simgcl", "simgcl", T.SimGCL, False)):
        cfg = T.get_config(model_name, use_tag=False, dim_latent=D, dim_layer_list=[D] * 3, device=dev, train_batch=B)
        torch.manual_seed(cfg["seed"])
        model = cls(ds, config=cfg, graph=G).train()
        opt = T.Adam(model.parameters(), lr=cfg["lr"])
        if fuse:
            opt.fuse_into(model)
        epoch = T.BPR_training_data(ds, config=cfg, seed=2020).all_train_data
        batches = [epoch[k * B:(k + 1) * B] for k in range(steps)]
        assert batches[0].shape == (B, 3) and batches[0].numel() * 16 <= G.shape[0]       # the compact path

        def run(model=model, opt=opt, batches=batches):
            for b in batches:
                lossx = model.loss(b)
                opt.zero_grad()
                sum(lossx).backward()
                opt.step()
        out[name] = run
    return out


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--scale", type=float, default=1.0, help="shrink the C2 graph (nodes and edges)")
    ap.add_argument("--rounds", type=int, default=9)
    ap.add_argument("--steps", type=int, default=10, help="steps per measurement of the step leg")
    ap.add_argument("--no-step", action="store_true", help="the layer only")
    a = ap.parse_args()
    ds, G, info = make_graph(a.scale)
    print(json.dumps(dict(D=D, eps=EPS, device=torch.cuda.get_device_name(0), rounds=a.rounds, shape="C2", scale=a.scale, **info)),
          flush=True)
    res = interleaved(layer_variants(G), a.rounds, 3)
    for k, (med, lo, hi) in res.items():
        print(json.dumps({"leg": "layer", "variant": k, "median_ms": round(med, 4), "min_ms": round(lo, 4), "max_ms": round(hi, 4),
                          "ratio_to_plain": round(med / res["plain"][0], 4), "ratio_to_unfused": round(med / res["unfused"][0], 4)}),
              flush=True)
    torch.cuda.empty_cache()
    if not a.no_step:
        res = interleaved(step_variants(ds, G, a.steps), a.rounds, 1)
        for k, (med, lo, hi) in res.items():
            print(json.dumps({"leg": "step", "variant": k, "steps_per_measurement": a.steps,
                              "median_ms_per_step": round(med / a.steps, 4), "min_ms_per_step": round(lo / a.steps, 4),
                              "max_ms_per_step": round(hi / a.steps, 4),
                              "ratio_to_lightgcn": round(med / res["lightgcn"][0], 4)}), flush=True)
