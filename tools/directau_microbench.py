"""Time the DirectAU kernels (tagrec_directau_fwd_f32 / tagrec_directau_bwd_f32, csrc/directau.hip) against the torch
composition of the same loss, and the DirectAU step next to the in-batch step at the C2 shape.

Usage: python tools/directau_microbench.py [--scale 1.0] [--rounds 20] [--steps 20] [--no-step]      (needs a GPU)
  Kernels: B = 512, 2 048, 8 192, 32 768 pairs x D = 64, 128, 256, t = 2, gamma = 1, L2 on the score rows.
  "fused" = rowops.directau_fwd + directau_bwd (prep, triangular forward, fixed-order reduce, one backward launch for both
  sides).  "torch" = the composition on the same GPU in the same process: F.normalize, the Gram matmul of each side with
  itself, exp(2 t (s - 1)), the strict upper triangle's sum through a mask built once outside the timed call, log, autograd --
  it stores two B x B matrices per side and their gradients (skipped with a note if the device has less free memory).
  "fused_fwd" / "inbatch_fwd": the two forwards alone at every shape (B = 512: 8 blocks per side against the in-batch
  forward's 8 blocks).  All variants interleaved in one process: rounds of every variant once, device events around each call,
  warm-up first; median, minimum and maximum.
  Arithmetic: the forward computes half of two B x B x D products: 2 B^2 D flops; the backward recomputes both in full and
  forms both second products: 8 B^2 D; the rate of the fused pair is reported against 10 B^2 D.
  Step: one C2 LightGCN-family step (1 M x 1 M nodes, 50 M edges, 3 layers, D = 64, batch 512, Adam fused into the last hop)
  of T.DirectAU next to T.LightGCN with negatives = "in_batch" and to the default triplet step, in the same process on the same
  graph: `--steps` steps between synchronisations per measurement, the variants interleaved over the rounds.
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
AU_T, GAMMA, TAU = 2.0, 1.0, 0.5
BS = (512, 2048, 8192, 32768)
DS = (64, 128, 256)


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


def kernel_variants(B, D):
    g = torch.Generator(device=dev).manual_seed(1)
    out, notes = {}, []
    Ub, Ib = torch.randn(B, D, device=dev, generator=g) * 0.3, torch.randn(B, D, device=dev, generator=g) * 0.3
    dU, dI = torch.empty_like(Ub), torch.empty_like(Ib)
    up = torch.tensor([1.0, 1e-3], device=dev)

    def fused():
        _, _, state = rowops.directau_fwd(Ub, Ib, Ub, Ib, AU_T, GAMMA)
        rowops.directau_bwd(Ub, Ib, Ub, Ib, state, up, dU, dI, dU, dI)
    out["fused"] = fused
    out["fused_fwd"] = lambda: rowops.directau_fwd(Ub, Ib, Ub, Ib, AU_T, GAMMA)
    out["inbatch_fwd"] = lambda: rowops.inbatch_fwd(Ub, Ib, Ub, Ib, TAU)
    need = 5.0 * B * B * 4 + B * B + (1 << 28)               # per side: Gram, exp, masked copy and two gradients; the mask; headroom
    free = torch.cuda.mem_get_info()[0]
    if need > free:
        notes.append({"leg": "kernel", "variant": "torch", "B": B, "D": D, "skipped": f"needs {need / 1e9:.1f} GB, {free / 1e9:.1f} GB free"})
        return out, notes
    Ut, It = Ub.clone().requires_grad_(), Ib.clone().requires_grad_()
    upper = torch.ones(B, B, dtype=torch.bool, device=dev).triu_(1)          # built once, outside the timed call
    n_pairs = B * (B - 1) / 2

    def torch_form():
        Ut.grad = It.grad = None
        x, y = F.normalize(Ut, dim=1), F.normalize(It, dim=1)
        align = (x - y).pow(2).sum(1).mean()

        def unif(z):
            return (torch.exp(2 * AU_T * (z @ z.t() - 1.0)).masked_fill(~upper, 0.0).sum() / n_pairs).log()
        loss = align + GAMMA * (unif(x) + unif(y)) / 2 + 1e-3 * 0.5 * (Ut.pow(2).sum() + It.pow(2).sum()) / B
        loss.backward()
    out["torch"] = torch_form
    return out, notes


def step_variants(scale, steps, D=64, B=512):
    nu = ni = max(int(1_000_000 * scale), 2000)
    ne = max(int(50_000_000 * scale), 40000)
    ds = T.synth.make_bipartite_device(nu, ni, ne, seed=1, device=dev)
    e = ds.edge_index["train"]
    rp, col, val, n = T.graph.bipartite_norm_device(e[:, 0], e[:, 1], nu, ni, "bi_norm")
    G = T.Graph(rp, col, val, (n, n), symmetric=True)
    G.transpose()
    out, info = {}, {"users": nu, "items": ni, "edges": int(e.shape[0]), "nnz": int(rp[-1])}
    for name, cls, model_name, kw in (("triplet_softplus_K1", T.LightGCN, "lightgcn", {}),
                                      ("in_batch", T.LightGCN, "lightgcn", dict(negatives="in_batch", mul_loss_func="softmax", loss_temperature=TAU)),
                                      ("directau", T.DirectAU, "directau", dict(au_t=AU_T, au_gamma=GAMMA))):
        cfg = T.get_config(model_name, use_tag=False, dim_latent=D, dim_layer_list=[D] * 3, device=dev, train_batch=B, **kw)
        torch.manual_seed(cfg["seed"])
        model = cls(ds, config=cfg, graph=G).train()
        opt = T.Adam(model.parameters(), lr=cfg["lr"])
        opt.fuse_into(model)
        epoch = T.BPR_training_data(ds, config=cfg, seed=2020).all_train_data
        batches = [epoch[k * B:(k + 1) * B] for k in range(steps)]
        assert batches[0].shape == (B, 3 if name.startswith("triplet") else 2) and batches[0].numel() * 16 <= n     # the compact path

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
    ap.add_argument("--rounds", type=int, default=20)
    ap.add_argument("--steps", type=int, default=20, help="steps per measurement of the step leg")
    ap.add_argument("--step-rounds", type=int, default=9)
    ap.add_argument("--no-step", action="store_true", help="kernels only")
    a = ap.parse_args()
    print(json.dumps({"t": AU_T, "gamma": GAMMA, "device": torch.cuda.get_device_name(0), "rounds": a.rounds}), flush=True)
    for D in DS:
        for B in BS:
            variants, notes = kernel_variants(B, D)
            for nline in notes:
                print(json.dumps(nline), flush=True)
            res = interleaved(variants, a.rounds, 3)
            for k, (med, lo, hi) in res.items():
                line = {"leg": "kernel", "variant": k, "B": B, "D": D, "median_us": round(med * 1e3, 2), "min_us": round(lo * 1e3, 2),
                        "max_us": round(hi * 1e3, 2)}
                if k == "fused":
                    line["TFLOPs_of_10_B2_D"] = round(10.0 * B * B * D / (med * 1e-3) / 1e12, 2)
                    if "torch" in res:
                        line["torch_over_fused"] = round(res["torch"][0] / med, 3)
                if k == "fused_fwd":
                    line["over_inbatch_fwd"] = round(med / res["inbatch_fwd"][0], 3)
                print(json.dumps(line), flush=True)
            del variants
            torch.cuda.empty_cache()
    if not a.no_step:
        variants, info = step_variants(a.scale, a.steps)
        print(json.dumps(dict(shape="C2", scale=a.scale, steps_per_measurement=a.steps, **info)), flush=True)
        res = interleaved(variants, a.step_rounds, 1)
        base = res["in_batch"][0]
        for k, (med, lo, hi) in res.items():
            print(json.dumps({"leg": "lightgcn_step", "variant": k, "median_ms_per_step": round(med / a.steps, 4),
                              "min_ms_per_step": round(lo / a.steps, 4), "max_ms_per_step": round(hi / a.steps, 4),
                              "ratio_to_in_batch": round(med / base, 4)}), flush=True)
