"""Time one NCL training step against one LightGCN step of the same commit on the C2-shaped synthetic graph, the pieces of
the NCL step, and one e_step.

Usage: python tools/ncl_microbench.py [--scale 1.0] [--rounds 7] [--steps 5]      (needs a GPU)
  step        NCL (3 layers, batch 512, D = 64, Adam as a separate launch: the fused update is refused; after one e_step, so
              both terms run) next to LightGCN with the same optimizer form; `--steps` steps between synchronisations.
  pieces      of one NCL step, each forward + backward to the table gradient, on one batch: the ranking step (LightGCN.loss),
              the two-hop view alone (two products forward, two transposed products backward), the two structure softmaxes
              (on a detached view: gather, normalise, K21 forward and backward, fold) and the two prototype softmaxes.
  e_step      both k-means (users and items, ncl_clusters = 1000, ncl_kmeans_iters = 20).
  All variants interleaved over the rounds, device events around each call, warm-up first; median, minimum and maximum.
Prints one JSON line per measurement."""
import argparse
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch

import tagrec_amd as T
from tagrec_amd import help as H

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


def build(ds, G, name, cls, **kw):
    cfg = T.get_config(name, use_tag=False, dim_latent=D, dim_layer_list=[D] * 3, device=dev, train_batch=B, **kw)
    torch.manual_seed(cfg["seed"])
    model = cls(ds, config=cfg, graph=G).train()
    return cfg, model, T.Adam(model.parameters(), lr=cfg["lr"])


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--scale", type=float, default=1.0, help="shrink the C2 graph (nodes and edges)")
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--steps", type=int, default=5, help="steps per measurement of the step leg")
    ap.add_argument("--clusters", type=int, default=1000)
    a = ap.parse_args()
    ds, G, info = make_graph(a.scale)
    print(json.dumps(dict(D=D, B=B, device=torch.cuda.get_device_name(0), rounds=a.rounds, shape="C2", scale=a.scale,
                          clusters=a.clusters, **info)), flush=True)
    cfg, ncl, ncl_opt = build(ds, G, "ncl", T.NCL, ncl_clusters=a.clusters)
    _, light, light_opt = build(ds, G, "lightgcn", T.LightGCN)
    epoch = T.BPR_training_data(ds, config=cfg, seed=2020).all_train_data
    batches = [epoch[k * B:(k + 1) * B] for k in range(a.steps)]
    nu, ni = ncl.num_list[0], ncl.num_list[1]

    res = interleaved({"e_step": ncl.e_step}, 3, 1)
    med, lo, hi = res["e_step"]
    print(json.dumps({"leg": "e_step", "clusters": a.clusters, "kmeans_iters": ncl.ncl_kmeans_iters, "median_ms": round(med, 3),
                      "min_ms": round(lo, 3), "max_ms": round(hi, 3)}), flush=True)

    def steps(model, opt):
        def run():
            for b in batches:
                lossx = model.loss(b)
                opt.zero_grad()
                sum(lossx).backward()
                opt.step()
        return run

    res = interleaved({"lightgcn": steps(light, light_opt), "ncl": steps(ncl, ncl_opt)}, a.rounds, 1)
    for k, (med, lo, hi) in res.items():
        print(json.dumps({"leg": "step", "variant": k, "steps_per_measurement": a.steps, "median_ms_per_step": round(med / a.steps, 4),
                          "min_ms_per_step": round(lo / a.steps, 4), "max_ms_per_step": round(hi / a.steps, 4),
                          "ratio_to_lightgcn": round(med / res["lightgcn"][0], 4)}), flush=True)

    b0 = batches[0].to(dev, torch.int64).contiguous()
    ub, ib = b0[:, 0].contiguous(), b0[:, 1].contiguous()
    tau, alpha, table = ncl.ncl_temperature, ncl.ncl_alpha, ncl.table
    y2_const = H.split_mm(G, H.split_mm(G, table.detach()))
    d_y2 = torch.randn_like(y2_const) * 1e-3

    def ranking():
        light.table.grad = None
        sum(light.loss(b0)).backward()

    def two_hop():
        table.grad = None
        H.split_mm(G, H.split_mm(G, table)).backward(d_y2)

    def struct_softmaxes():
        table.grad = None
        y2 = y2_const.detach().requires_grad_()
        l = H._NodeContrast.apply(y2, table[:nu], ub, ub, tau, False, None) \
            + alpha * H._NodeContrast.apply(y2, table[nu:nu + ni], ib + nu, ib, tau, False, None)
        l.backward()

    def proto_softmaxes():
        table.grad = None
        ncl.proto_loss(b0).backward()

    res = interleaved({"ranking_step": ranking, "two_hop_view_fwd_bwd": two_hop, "structure_softmaxes": struct_softmaxes,
                       "prototype_softmaxes": proto_softmaxes}, a.rounds, 2)
    for k, (med, lo, hi) in res.items():
        print(json.dumps({"leg": "piece", "variant": k, "median_ms": round(med, 4), "min_ms": round(lo, 4), "max_ms": round(hi, 4)}),
              flush=True)
