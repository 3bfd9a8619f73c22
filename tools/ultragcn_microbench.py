"""Time one UltraGCN training step and its two loss kernels at the C2 shape.

Usage: python tools/ultragcn_microbench.py [--rounds 20] [--scale 1.0]      (needs a GPU)
  build    T.UltraGCN on synth.make_bipartite_device(1 M users, 1 M items, 50 M edges), D = 64, ug_neighbors = 10: the
           construction time (CSRs, degrees, the co-occurrence top-k).
  step     zero_grad / loss / backward / Adam.step on B = 512 tuples with K = 16 and K = 63 negatives (M = 10 neighbours), device
           events around each step, median / min / max over `rounds` after a warm-up.  For orientation only, beside the LightGCN
           step of `python bench.py` (profiles/ultragcn_bench_parent_vs_branch.log): the two models do different work.
  kernels  CALL times of rowops.wbce_fwd / wbce_bwd alone on gathered rows of the same shapes (device events around the Python
           wrapper: allocations, argument checks and, for the forward, two launches -- for kernel times run this script under
           `rocprofv3 --kernel-trace --stats` in a run of its own), with their algorithmic bytes -- forward: the
           (1 + S) B rows of D floats it reads, the weights it reads and the coefficients it writes; backward: the same rows
           read, as many written, the coefficients read (the L2 rows are the score rows: one shared buffer) -- and the achieved
           rate against the measured gather ceiling of bench.py's probes (random 256-byte rows from a 512 MB table, the C2
           table's size; the compact operands here are contiguous, so the ceiling is an orientation, not a roof).
  Prints one JSON line per measurement."""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch

import tagrec_amd as T
from tagrec_amd import rowops

dev = torch.device("cuda:0")
D, B, M = 64, 512, 10


def event_ms(fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b)


def stats(fn, rounds, warmup=5):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    v = sorted(event_ms(fn) for _ in range(rounds))
    return {"median_ms": round(v[len(v) // 2], 4), "min_ms": round(v[0], 4), "max_ms": round(v[-1], 4)}


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=20)
    ap.add_argument("--scale", type=float, default=1.0, help="shrink the graph")
    ap.add_argument("--no-probes", action="store_true")
    a = ap.parse_args()
    nu = ni = max(int(1_000_000 * a.scale), 1000)
    ne = max(int(50_000_000 * a.scale), 20000)
    print(json.dumps(dict(device=torch.cuda.get_device_name(0), n_user=nu, n_item=ni, edges=ne, D=D, B=B, M=M, rounds=a.rounds)), flush=True)
    ceiling = None
    if not a.no_probes:
        from bench import probe_ceilings
        ceiling = probe_ceilings(dev)["gather_256B_rows_from_512MB"]
        print(json.dumps(dict(leg="ceiling", gather_256B_rows_from_512MB_gbs=ceiling)), flush=True)
    ds = T.synth.make_bipartite_device(nu, ni, ne, 7, dev)
    gen = torch.Generator(device=dev).manual_seed(1)
    edges = ds.edge_index["train"]
    for K in (16, 63):
        cfg = T.get_config("ultragcn", device=dev, dim_latent=D, n_negatives=K, reg=1e-4, ug_neighbors=M)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        model = T.UltraGCN(ds, config=cfg)
        torch.cuda.synchronize()
        print(json.dumps(dict(leg="build", K=K, seconds=round(time.perf_counter() - t0, 3))), flush=True)
        opt = T.Adam(model.parameters(), lr=0.01)
        model.train()
        pick = edges[torch.randint(0, edges.shape[0], (B,), device=dev, generator=gen)]
        batch = torch.cat([pick, torch.randint(0, ni, (B, K), device=dev, generator=gen)], 1).contiguous()

        def step():
            opt.zero_grad()
            sum(model.loss(batch)).backward()
            opt.step()
        print(json.dumps(dict(leg="step", K=K, **stats(step, a.rounds))), flush=True)

        S = 1 + K + M
        stage = T.loss_stage.Ultra(model.tables)
        uid, iid = stage.ids(batch)
        U, I = model.embed
        Ub, Ib = U.detach().index_select(0, uid), I.detach().index_select(0, iid)
        w = stage.weights(batch)
        res, coef = rowops.wbce_fwd(Ub, Ib, Ub, Ib, w, K, M)
        dUb, dIb = torch.empty_like(Ub), torch.empty_like(Ib)
        g = torch.ones(2, device=dev)
        rows_bytes = (1 + S) * B * D * 4
        for name, fn, nbytes in (("wbce_fwd", lambda: rowops.wbce_fwd(Ub, Ib, Ub, Ib, w, K, M), rows_bytes + 2 * B * S * 4),
                                 ("wbce_bwd", lambda: rowops.wbce_bwd(Ub, Ib, Ub, Ib, coef, g, dUb, dIb, dUb, dIb, K, M),
                                  2 * rows_bytes + B * S * 4)):
            st = stats(fn, a.rounds)
            row = dict(leg="call", variant=name, K=K, S=S, algorithmic_bytes=nbytes, **st,
                       gbs_median=round(nbytes / (st["median_ms"] * 1e-3) / 1e9, 1))
            if ceiling:
                row["frac_of_gather_ceiling"] = round(row["gbs_median"] / ceiling, 4)
            print(json.dumps(row), flush=True)
        del model, opt
        torch.cuda.empty_cache()
