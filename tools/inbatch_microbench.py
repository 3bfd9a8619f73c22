"""Time the in-batch softmax kernels (tagrec_inbatch_fwd_f32 / tagrec_inbatch_bwd_f32, csrc/inbatch.hip) against the
materialised torch form, and the LightGCN step that uses them, at the C2 shape.

Usage: python tools/inbatch_microbench.py [--scale 1.0] [--rounds 9] [--steps 20]      (needs a GPU)
  Kernels: D = 64, B = 512, 2 048, 8 192, 16 384 pairs with distinct ids (nothing masked, the mask is still evaluated), L2 on
  the score rows.  "fused" = rowops.inbatch_fwd + inbatch_bwd (forward, fixed-order reduce, one backward launch for both
  operands).  "torch" = the materialised form on the same GPU: U @ I.T / tau, masked_fill with the same mask (built once,
  outside the timed call), F.cross_entropy against the diagonal, autograd -- it stores the B x B logits and their gradient
  (about 3 GB at B = 16 384; skipped with a note if the device has less free memory).  All variants interleaved in one process: rounds of every variant once,
  device events around each call, warm-up first; median, minimum and maximum.
  Arithmetic: the forward is 2 B^2 D flops, the backward recomputes the scores for both operands and forms both products:
  8 B^2 D; the rate of the fused pair is reported against 10 B^2 D.
  Step: one C2 LightGCN step (1 M x 1 M nodes, 50 M edges, 3 layers, D = 64, batch 512, Adam fused into the last hop) with
  negatives = "in_batch" next to the default triplet step and to mul_loss_func = "softmax" with K = 16, in the same process on
  the same graph: `--steps` steps between synchronisations per measurement, the variants interleaved over the rounds.
Prints one JSON line per measurement."""
import argparse
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch
import torch.nn.functional as F

import tagrec_amd as T
from tagrec_amd import rowops

dev = torch.device("cuda:0")
D, TAU = 64, 0.5
BS = (512, 2048, 8192, 16384)


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
    out, notes = {}, []
    for B in BS:
        Ub, Ib = torch.randn(B, D, device=dev, generator=g) * 0.3, torch.randn(B, D, device=dev, generator=g) * 0.3
        ids = torch.arange(B, device=dev)
        dU, dI = torch.empty_like(Ub), torch.empty_like(Ib)
        up = torch.tensor([1.0, 1e-3], device=dev)

        def fused(Ub=Ub, Ib=Ib, ids=ids, dU=dU, dI=dI, up=up):
            _, lse = rowops.inbatch_fwd(Ub, Ib, Ub, Ib, TAU, ids, ids)
            rowops.inbatch_bwd(Ub, Ib, Ub, Ib, TAU, lse, up, dU, dI, dU, dI, ids, ids)
        out[f"fused_B{B}"] = fused
        need = 3.2 * B * B * 4 + (1 << 28)                     # logits, masked copy, gradient, and the bool mask; headroom
        free = torch.cuda.mem_get_info()[0]
        if need > free:
            notes.append({"leg": "kernel", "variant": f"torch_B{B}", "skipped": f"needs {need / 1e9:.1f} GB, {free / 1e9:.1f} GB free"})
            continue
        Ut, It = Ub.clone().requires_grad_(), Ib.clone().requires_grad_()
        # the mask is built once, outside the timed call (the fused kernels evaluate theirs inside it)
        m = ((ids[None, :] == ids[:, None]) | (ids[None, :] == ids[:, None])) & ~torch.eye(B, dtype=torch.bool, device=dev)

        def torch_form(Ut=Ut, It=It, ids=ids, B=B, m=m):
            Ut.grad = It.grad = None
            z = Ut @ It.t() / TAU
            loss = F.cross_entropy(z.masked_fill(m, float("-inf")), ids) + 1e-3 * 0.5 * (Ut.pow(2).sum() + It.pow(2).sum()) / B
            loss.backward()
        out[f"torch_B{B}"] = torch_form
    return out, notes


def step_variants(scale, steps, B=512):
    nu = ni = max(int(1_000_000 * scale), 2000)
    ne = max(int(50_000_000 * scale), 40000)
    ds = T.synth.make_bipartite_device(nu, ni, ne, seed=1, device=dev)
    e = ds.edge_index["train"]
    rp, col, val, n = T.graph.bipartite_norm_device(e[:, 0], e[:, 1], nu, ni, "bi_norm")
    G = T.Graph(rp, col, val, (n, n), symmetric=True)
    G.transpose()
    out, info = {}, {"users": nu, "items": ni, "edges": int(e.shape[0]), "nnz": int(rp[-1])}
    for name, kw in (("triplet_softplus_K1", {}),
                     ("in_batch", dict(negatives="in_batch", mul_loss_func="softmax", loss_temperature=TAU)),
                     ("softmax_K16", dict(mul_loss_func="softmax", n_negatives=16, loss_temperature=TAU))):
        cfg = T.get_config("lightgcn", use_tag=False, dim_latent=D, dim_layer_list=[D] * 3, device=dev, train_batch=B, **kw)
        torch.manual_seed(cfg["seed"])
        model = T.LightGCN(ds, config=cfg, graph=G).train()
        opt = T.Adam(model.parameters(), lr=cfg["lr"])
        opt.fuse_into(model)
        epoch = T.BPR_training_data(ds, config=cfg, seed=2020).all_train_data
        batches = [epoch[k * B:(k + 1) * B] for k in range(steps)]
        width = 2 if name == "in_batch" else 2 + cfg["n_negatives"]
        assert batches[0].shape == (B, width) and batches[0].numel() * 16 <= n       # the compact path

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
    print(json.dumps({"D": D, "tau": TAU, "device": torch.cuda.get_device_name(0), "rounds": a.rounds}), flush=True)
    variants, notes = kernel_variants()
    for nline in notes:
        print(json.dumps(nline), flush=True)
    res = interleaved(variants, a.rounds, 3)
    for k, (med, lo, hi) in res.items():
        B = int(k.rsplit("B", 1)[1])
        line = {"leg": "kernel", "variant": k, "B": B, "median_us": round(med * 1e3, 2), "min_us": round(lo * 1e3, 2),
                "max_us": round(hi * 1e3, 2)}
        if k.startswith("fused"):
            line["TFLOPs_of_10_B2_D"] = round(10.0 * B * B * D / (med * 1e-3) / 1e12, 2)
            if f"torch_B{B}" in res:
                line["torch_over_fused"] = round(res[f"torch_B{B}"][0] / med, 3)
        print(json.dumps(line), flush=True)
    del variants
    torch.cuda.empty_cache()
    if not a.no_step:
        variants, info = step_variants(a.scale, a.steps)
        print(json.dumps(dict(shape="C2", scale=a.scale, steps_per_measurement=a.steps, **info)), flush=True)
        res = interleaved(variants, a.rounds, 1)
        base = res["triplet_softplus_K1"][0]
        for k, (med, lo, hi) in res.items():
            print(json.dumps({"leg": "lightgcn_step", "variant": k, "median_ms_per_step": round(med / a.steps, 4),
                              "min_ms_per_step": round(lo / a.steps, 4), "max_ms_per_step": round(hi / a.steps, 4),
                              "ratio_to_triplet": round(med / base, 4)}), flush=True)
