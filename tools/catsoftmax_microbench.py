"""Time the catalogue softmax kernels (tagrec_catsoftmax_fwd_f32 / tagrec_catsoftmax_bwd_f32, csrc/catsoftmax.hip) against
the materialised torch form and the eval kernel on the same table, and the LightGCN step that uses them, at the C2 shape.

Usage: python tools/catsoftmax_microbench.py [--scale 1.0] [--rounds 9] [--steps 10] [--mask-len L [--mask-only]]   (needs a GPU)
  Kernels: D = 64, N = 1 M items (times --scale), B = 512 and 2 048 users read through qrow from a 1 M-row table, L2 on the
  score tables.  "fused" = rowops.catsoftmax_fwd + catsoftmax_bwd (forward, combine, the dense dT, the split dQ and its sum),
  "fwd" the forward alone.  "torch" = the materialised form on the same GPU: U[u] @ I.T / tau, F.cross_entropy, autograd --
  it stores the B x N logits and their gradient (4 B N bytes each; skipped with a note if the device has less free memory).
  "eval_topk" = evaluate.fused_topk on the same users and table, k = 20: the nearest measured thing in the tree (one product).
  All variants interleaved in one process: rounds of every variant once, device events around each call, warm-up first;
  median, minimum and maximum.
  Arithmetic, the products counted as built: the forward is one product (2 B N D flops), the backward recomputes the scores
  for both operands and forms both gradients (four): the fused pair is reported against 10 B N D, the forward and the eval
  kernel against 2 B N D.
  Step: one C2 LightGCN step (1 M x 1 M nodes, 50 M edges, 3 layers, D = 64, batch 512, Adam fused into the last hop) with
  softmax_over = "catalogue" next to the default triplet step and to the same triplet step with restrict_forward = False (the
  catalogue step is an all-rows step plus the loss stage), in the same process on the same graph: `--steps` steps between
  synchronisations per measurement, the variants interleaved over the rounds.
  Mask (--mask-len L > 0): the masked entry points (mask=(ptr, cols)) next to the unmasked ones at B = 512, the forward and
  the backward (dT, dQ, its sum, the L2 rows) each as one call, interleaved as above.  Every row of the 1 M-row user table
  gets a list of exactly L columns, ascending and unique by construction: column j of a row is drawn uniformly from the
  j-th of L equal strata of [0, N) (L = 50 is the C2 mean: 50 M train edges over 1 M users).  --mask-only: this leg alone.
  The split of the backward into dT and dQ is not visible to device events around one call: take it from a kernel trace of
  `--mask-only` (the kernels are cat_dt_kernel / cat_dt_masked_kernel, cat_dq_kernel / cat_dq_masked_kernel).
Prints one JSON line per measurement."""
import argparse
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch
import torch.nn.functional as F

import tagrec_amd as T
from tagrec_amd import evaluate, rowops

dev = torch.device("cuda:0")
D, TAU = 64, 0.5
BS = (512, 2048)


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


def kernel_variants(N):
    g = torch.Generator(device=dev).manual_seed(1)
    U, I = torch.randn(N, D, device=dev, generator=g) * 0.3, torch.randn(N, D, device=dev, generator=g) * 0.3
    dI = torch.empty_like(I)
    up = torch.tensor([1.0, 1e-3], device=dev)
    out, notes = {}, []
    for B in BS:
        urow = torch.randint(0, N, (B,), device=dev, generator=g)
        target = torch.randint(0, N, (B,), device=dev, generator=g)
        ws = torch.empty(rowops.catsoftmax_workspace(B, N, D), dtype=torch.uint8, device=dev)
        dQ, dQr, dTr = (torch.empty(B, D, device=dev) for _ in range(3))
        notes.append({"leg": "kernel", "B": B, "N": N, "n_split": rowops.catsoftmax_splits(B, N, D), "workspace_MB": round(ws.numel() / 1e6, 1)})

        def fwd(urow=urow, target=target, ws=ws):
            return rowops.catsoftmax_fwd(U, I, target, TAU, urow, U, I, 0, ws)

        def fused(urow=urow, target=target, ws=ws, dQ=dQ, dQr=dQr, dTr=dTr):
            _, lse, _ = rowops.catsoftmax_fwd(U, I, target, TAU, urow, U, I, 0, ws)
            rowops.catsoftmax_bwd(U, I, target, TAU, lse, up, dI, dQ, urow, U, I, dQr, dTr, 0, ws)
        out[f"fwd_B{B}"], out[f"fused_B{B}"] = fwd, fused
        empty_ptr = torch.zeros(N + 1, dtype=torch.int64, device=dev)            # no train positives: nothing is masked
        empty_col = torch.zeros(1, dtype=torch.int32, device=dev)

        def eval_topk(urow=urow, empty_ptr=empty_ptr, empty_col=empty_col):
            evaluate.fused_topk(U, I, urow, empty_ptr, empty_col, 20)
        out[f"eval_topk_B{B}"] = eval_topk
        need = 3.2 * B * N * 4 + (1 << 28)                     # logits, softmax, gradient; headroom
        free = torch.cuda.mem_get_info()[0]
        if need > free:
            notes.append({"leg": "kernel", "variant": f"torch_B{B}", "skipped": f"needs {need / 1e9:.1f} GB, {free / 1e9:.1f} GB free"})
            continue
        Ut, It = U.clone().requires_grad_(), I.clone().requires_grad_()

        def torch_form(Ut=Ut, It=It, urow=urow, target=target, B=B):
            Ut.grad = It.grad = None
            u = Ut[urow]
            z = u @ It.t() / TAU
            loss = F.cross_entropy(z, target) + 1e-3 * 0.5 * (u.pow(2).sum() + It[target].pow(2).sum()) / B
            loss.backward()
        out[f"torch_B{B}"] = torch_form
    return out, notes


def stratified_lists(rows, N, L, g):
    """(ptr int64 [rows + 1], cols int32 [rows L]): L columns per row, ascending and unique: one uniform draw per stratum."""
    width = N // L
    assert width >= 1, "more list entries than columns"
    cols = torch.arange(L, device=dev, dtype=torch.int64)[None, :] * width + torch.randint(0, width, (rows, L), device=dev, generator=g)
    return torch.arange(rows + 1, device=dev, dtype=torch.int64) * L, cols.to(torch.int32).reshape(-1)


def mask_variants(N, L, B=512):
    g = torch.Generator(device=dev).manual_seed(1)
    U, I = torch.randn(N, D, device=dev, generator=g) * 0.3, torch.randn(N, D, device=dev, generator=g) * 0.3
    dI = torch.empty_like(I)
    up = torch.tensor([1.0, 1e-3], device=dev)
    urow = torch.randint(0, N, (B,), device=dev, generator=g)
    mask = stratified_lists(N, N, L, g)
    # a train pair: the target is one of the user's own listed items (it stays live)
    pick = torch.randint(0, L, (B,), device=dev, generator=g)
    target = mask[1][urow * L + pick].to(torch.int64)
    ws = torch.empty(rowops.catsoftmax_workspace(B, N, D), dtype=torch.uint8, device=dev)
    dQ, dQr, dTr = (torch.empty(B, D, device=dev) for _ in range(3))
    out = {}
    for name, m in (("unmasked", None), ("masked", mask)):
        _, lse, _ = rowops.catsoftmax_fwd(U, I, target, TAU, urow, U, I, 0, ws, mask=m)

        def fwd(m=m):
            return rowops.catsoftmax_fwd(U, I, target, TAU, urow, U, I, 0, ws, mask=m)

        def bwd(m=m, lse=lse):
            rowops.catsoftmax_bwd(U, I, target, TAU, lse, up, dI, dQ, urow, U, I, dQr, dTr, 0, ws, mask=m)
        out[f"fwd_{name}_B{B}"], out[f"bwd_{name}_B{B}"] = fwd, bwd
    note = {"leg": "mask", "B": B, "N": N, "list_len": L, "lists": "one uniform draw from each of L equal strata of [0, N), every "
            "row of the user table; the target is one of the row's listed items", "n_split": rowops.catsoftmax_splits(B, N, D),
            "list_MB": round(mask[1].numel() * 4 / 1e6, 1)}
    return out, note


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
                     ("triplet_all_rows", dict(restrict_forward=False)),
                     ("catalogue", dict(softmax_over="catalogue", mul_loss_func="softmax", loss_temperature=TAU))):
        cfg = T.get_config("lightgcn", use_tag=False, dim_latent=D, dim_layer_list=[D] * 3, device=dev, train_batch=B, **kw)
        torch.manual_seed(cfg["seed"])
        model = T.LightGCN(ds, config=cfg, graph=G).train()
        opt = T.Adam(model.parameters(), lr=cfg["lr"])
        opt.fuse_into(model)
        epoch = T.BPR_training_data(ds, config=cfg, seed=2020).all_train_data
        batches = [epoch[k * B:(k + 1) * B] for k in range(steps)]
        assert batches[0].shape == (B, 2 if name == "catalogue" else 3)

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
    ap.add_argument("--scale", type=float, default=1.0, help="shrink the item table and the C2 graph (nodes and edges)")
    ap.add_argument("--rounds", type=int, default=9)
    ap.add_argument("--steps", type=int, default=10, help="steps per measurement of the step leg")
    ap.add_argument("--no-step", action="store_true", help="kernels only")
    ap.add_argument("--mask-len", type=int, default=0, help="> 0: time the masked entry points with lists of this length per row")
    ap.add_argument("--mask-only", action="store_true", help="the mask leg alone (needs --mask-len)")
    a = ap.parse_args()
    N = max(int((1 << 20) * a.scale), 2048)
    print(json.dumps({"D": D, "tau": TAU, "N": N, "device": torch.cuda.get_device_name(0), "rounds": a.rounds}), flush=True)
    if a.mask_only and a.mask_len <= 0:
        ap.error("--mask-only needs --mask-len")
    if a.mask_len > 0:
        variants, note = mask_variants(N, a.mask_len)
        print(json.dumps(note), flush=True)
        res = interleaved(variants, a.rounds, 2)
        for k, (med, lo, hi) in res.items():
            line = {"leg": "mask", "variant": k, "median_ms": round(med, 4), "min_ms": round(lo, 4), "max_ms": round(hi, 4)}
            if "_masked_" in k:
                line["masked_over_unmasked"] = round(med / res[k.replace("_masked_", "_unmasked_")][0], 4)
            print(json.dumps(line), flush=True)
        del variants
        torch.cuda.empty_cache()
        if a.mask_only:
            sys.exit(0)
    variants, notes = kernel_variants(N)
    for nline in notes:
        print(json.dumps(nline), flush=True)
    res = interleaved(variants, a.rounds, 2)
    for k, (med, lo, hi) in res.items():
        B = int(k.rsplit("B", 1)[1])
        line = {"leg": "kernel", "variant": k, "B": B, "median_ms": round(med, 4), "min_ms": round(lo, 4), "max_ms": round(hi, 4)}
        products = 5 if k.startswith("fused") else (1 if k.startswith(("fwd", "eval")) else None)
        if products:
            line[f"TFLOPs_of_{2 * products}_B_N_D"] = round(2.0 * products * B * N * D / (med * 1e-3) / 1e12, 2)
        if k.startswith("fused") and f"torch_B{B}" in res:
            line["torch_over_fused"] = round(res[f"torch_B{B}"][0] / med, 3)
        print(json.dumps(line), flush=True)
    del variants
    torch.cuda.empty_cache()
    if not a.no_step:
        variants, info = step_variants(a.scale, a.steps)
        print(json.dumps(dict(shape="C2", scale=a.scale, steps_per_measurement=a.steps, **info)), flush=True)
        res = interleaved(variants, a.rounds, 1)
        base, allrows = res["triplet_softplus_K1"][0], res["triplet_all_rows"][0]
        for k, (med, lo, hi) in res.items():
            print(json.dumps({"leg": "lightgcn_step", "variant": k, "median_ms_per_step": round(med / a.steps, 4),
                              "min_ms_per_step": round(lo / a.steps, 4), "max_ms_per_step": round(hi / a.steps, 4),
                              "ratio_to_triplet": round(med / base, 4), "ms_over_all_rows": round((med - allrows) / a.steps, 4)}),
                  flush=True)
