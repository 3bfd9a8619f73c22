"""DisenHAN training-step time (needs a GPU).

    python tools/disenhan_step.py [--scale S] [--steps N] [--skip-c1] [--skip-c4] [--layers L] [--dim D]

C1: the tagged ml-100k-sized graph of tools/small_scale_step.py, eager and HIP-graph replay (epoch_training with
graphs={}), next to the plain-torch restatement (tests/disenhan_torch.py) on the GPU as the baseline.
C4: a tripartite graph of make_tripartite_device (1 M users, 1 M items, 2 M tags, 100 M assignments at --scale 1).
Also prints the algorithmic bytes of the edge-softmax passes and the products per step (sum over layers, iterations and
relations), so that a `rocprofv3 --kernel-trace --stats` run turns them into a share of 8 TB/s.  One JSON line per leg."""
import argparse
import json
import math
import os
import sys
import time
import types

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import torch  # noqa: E402

import tagrec_amd as T  # noqa: E402
from tagrec_amd import disenhan as DH  # noqa: E402


def algorithmic_bytes(model):
    """Bytes one training step moves in the edge passes and the products (fp32 / int32 entries, int64 row pointers)."""
    K, D, L = model.factor_k, model.dim_latent, model.num_layer
    out = {"edge_softmax_fwd": 0, "edge_softmax_bwd": 0, "spmm_fwd": 0, "spmm_bwd": 0, "score_bwd": 0}
    for rel in model.rels:
        nnz, (na, nb) = rel.nnz, rel.shape
        out["edge_softmax_fwd"] += nnz * (4 + 4 + 4 * K + 16) + na * (8 + 8 * K)
        out["edge_softmax_bwd"] += nnz * (8 + 8 + 4 + 4 + 4 * K + 4) + na * (8 + 16 * K) \
            + nnz * (4 + 4 + 4 + 8 * K) + nb * (8 + 8 * K)
        out["spmm_fwd"] += nnz * (4 + 4 + 4 * D) + na * (8 + 4 * D)
        out["spmm_bwd"] += nnz * (4 + 4 + 4 + 4 * D) + nb * (8 + 4 * D)           # permute + transposed product
        out["score_bwd"] += nnz * (4 + 4 + 4 * D) + na * (8 + 4 * D)
    return {k: v * L * DH.ITERATE for k, v in out.items()}


def _producer(batches):
    return types.SimpleNamespace(reset=lambda: None, mini_batch=lambda: iter(batches))


def time_model(model, batches, graphs, warm):
    opt = T.Adam(model.parameters(), lr=0.01, capturable=graphs is not None)
    model.train()
    T.epoch_training(_producer(batches[:warm]), model.loss, opt, verbose=False, graphs=graphs)
    torch.cuda.synchronize()
    t = time.perf_counter()
    losses = T.epoch_training(_producer(batches[warm:]), model.loss, opt, verbose=False, graphs=graphs)
    torch.cuda.synchronize()
    return (time.perf_counter() - t) / len(losses) * 1e3, losses[-1]


def time_torch_baseline(model, batches, warm):
    """The restatement in fp32 on the GPU, torch.optim.Adam: the plain-torch cost of the same step."""
    import disenhan_torch as DT
    rels = [DT.coo(tuple(t.cpu() if torch.is_tensor(t) else t for t in r), model.device)
            for r in DH.merged_relations(model._data)]
    sd = {k: v.detach().clone() for k, v in model.state_dict().items()}
    tables, layers = DT.params_from_state(sd, model.num_layer, dtype=torch.float32, device=model.device)
    params = tables + [p for lyr in layers for p in lyr]
    opt = torch.optim.Adam(params, lr=0.01)

    def step(b):
        parts = DT.loss(DT.forward(tables, layers, rels, model.factor_k), b, model.reg)
        opt.zero_grad()
        sum(parts).backward()
        opt.step()
        return parts
    for b in batches[:warm]:
        step(b)
    torch.cuda.synchronize()
    t = time.perf_counter()
    for b in batches[warm:]:
        parts = step(b)
    torch.cuda.synchronize()
    return (time.perf_counter() - t) / (len(batches) - warm) * 1e3, float(sum(parts).detach())


def bpr_batches(pos, n_item, B, n, seed, device):
    """n batches of (user, positive item, uniform random item) rows drawn from the [E, 2] positive pairs."""
    g = torch.Generator(device=device)
    g.manual_seed(seed)
    out = []
    for _ in range(n):
        pick = torch.randint(0, pos.shape[0], (B,), device=device, generator=g)
        neg = torch.randint(0, n_item, (B,), device=device, generator=g)
        out.append(torch.stack([pos[pick, 0], pos[pick, 1], neg], dim=1).contiguous())
    return out


def c1(args, dev):
    ds = T.synth.make_cf_dataset(943, 1682, 100000, seed=0, n_tag=400, n_assign=30000)
    cfg = T.disenhan_config(dim_latent=args.dim, dim_layer_list=[args.dim] * args.layers, device=dev, reg=1e-3)
    pos = torch.from_numpy(ds.edge_index["train"]).to(dev)
    batches = bpr_batches(pos, ds.num["item"], 512, args.steps + 3, 1, dev)
    res = {"leg": "C1", "users": 943, "items": 1682, "tags": 400, "layers": args.layers, "D": args.dim, "K": cfg["factor_k"]}
    for mode, graphs in (("eager", None), ("hip_graph", {})):
        torch.manual_seed(0)
        model = T.DisenHAN(ds, config=cfg)
        ms, loss = time_model(model, batches, graphs, 3)
        res[f"{mode}_ms"], res[f"{mode}_loss"] = round(ms, 3), loss
        if graphs is not None:
            res["graph_errors"] = graphs.get("errors", [])
    model._data = ds
    res["torch_ms"], res["torch_loss"] = time_torch_baseline(model, batches, 3)
    res["torch_ms"] = round(res["torch_ms"], 3)
    res["nnz"] = {e: r.nnz for e, r in zip(DH.RELATIONS, model.rels)}
    res["bytes"] = algorithmic_bytes(model)
    print(json.dumps(res), flush=True)


def c4(args, dev):
    s = args.scale
    nu, ni, nt, na = int(1_000_000 * s), int(1_000_000 * s), int(2_000_000 * s), int(100_000_000 * s)
    t0 = time.perf_counter()
    ds = T.synth.make_tripartite_device(nu, ni, nt, na, 7, dev)
    cfg = T.disenhan_config(dim_latent=args.dim, dim_layer_list=[args.dim] * args.layers, device=dev, reg=1e-3)
    torch.manual_seed(0)
    model = T.DisenHAN(ds, config=cfg)
    torch.cuda.synchronize()
    build_s = time.perf_counter() - t0
    batches = bpr_batches(ds.edge_index["train"], ni, 2048, args.c4_steps + 1, 2, dev)
    ms, loss = time_model(model, batches, None, 1)
    res = {"leg": "C4", "scale": s, "users": nu, "items": ni, "tags": nt, "assignments": int(ds.uit_data.shape[0]),
           "layers": args.layers, "D": args.dim, "K": cfg["factor_k"], "eager_ms": round(ms, 3), "loss": loss,
           "finite": bool(math.isfinite(loss)), "build_s": round(build_s, 2),
           "nnz": {e: r.nnz for e, r in zip(DH.RELATIONS, model.rels)}, "bytes": algorithmic_bytes(model),
           "peak_gib": round(torch.cuda.max_memory_allocated(dev) / 2**30, 2)}
    print(json.dumps(res), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--scale", type=float, default=1.0, help="C4 graph size relative to 1M / 1M / 2M nodes, 100M assignments")
    ap.add_argument("--steps", type=int, default=20, help="timed C1 steps")
    ap.add_argument("--c4-steps", type=int, default=3, help="timed C4 steps")
    ap.add_argument("--layers", type=int, default=2)
    ap.add_argument("--dim", type=int, default=64)
    ap.add_argument("--skip-c1", action="store_true")
    ap.add_argument("--skip-c4", action="store_true")
    args = ap.parse_args()
    dev = torch.device("cuda:0")
    if not args.skip_c1:
        c1(args, dev)
    if not args.skip_c4:
        c4(args, dev)


if __name__ == "__main__":
    main()
