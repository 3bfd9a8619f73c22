"""Time UltraGCN's training step under the dense `T.Adam` and under the row-sparse `T.RowAdam`, in one process.

Usage: python tools/row_adam_microbench.py [--max-lag 1024] [--blocks 2] [--scale 1.0]      (needs a GPU)
  The shape of tools/ultragcn_microbench.py: synth.make_bipartite_device(1 M users, 1 M items, 50 M edges), D = 64, B = 512,
  K = 16 and 63 negatives, M = 10 neighbours.  Two models from the same seed, one per optimizer; fresh batches every step,
  the same ones for both legs.
  window   device events around whole windows of 2 * max_lag steps, so that RowAdam's periodic flushes (two per window) are
           inside the figure; the legs alternate (dense, lazy, dense, lazy, ...), `blocks` windows each.  ms_per_step = window
           time / steps.  The dense leg is the baseline; its own spread over the windows is what a difference must exceed.
  lag      just before a flush that is max_lag - 1 steps due: the share of the table's rows it has to replay (behind AND with a
           non-zero moment) and their mean lag; then that flush alone.
  kernels  the catch-up call (`opt.catch_up` on the step's plan) and `opt.step()` (the apply kernels, no flush due) alone.
  Prints one JSON line per measurement."""
import argparse
import copy
import json
import os
import sys

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


def med(v):
    v = sorted(v)
    return {"median_ms": round(v[len(v) // 2], 4), "min_ms": round(v[0], 4), "max_ms": round(v[-1], 4)}


def step(model, opt, batch):
    opt.zero_grad()
    sum(model.loss(batch)).backward()
    opt.step()


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--max-lag", type=int, default=1024)
    ap.add_argument("--blocks", type=int, default=2, help="windows per leg and K")
    ap.add_argument("--scale", type=float, default=1.0, help="shrink the graph")
    ap.add_argument("--rounds", type=int, default=20, help="samples of the kernels-alone legs")
    a = ap.parse_args()
    nu = ni = max(int(1_000_000 * a.scale), 1000)
    ne = max(int(50_000_000 * a.scale), 20000)
    steps = 2 * a.max_lag
    print(json.dumps(dict(device=torch.cuda.get_device_name(0), n_user=nu, n_item=ni, edges=ne, D=D, B=B, M=M, max_lag=a.max_lag,
                          window_steps=steps, blocks=a.blocks)), flush=True)
    ds = T.synth.make_bipartite_device(nu, ni, ne, 7, dev)
    edges = ds.edge_index["train"]
    gen = torch.Generator(device=dev).manual_seed(1)
    cfg = T.get_config("ultragcn", device=dev, dim_latent=D, n_negatives=16, reg=1e-4, ug_neighbors=M, deterministic=True)
    torch.manual_seed(3)
    dense = T.UltraGCN(ds, config=cfg)
    lazy = copy.deepcopy(dense)                     # the same table and constants: built once
    opt_d = T.Adam(dense.parameters(), lr=0.01)
    opt_l = T.RowAdam(lazy.parameters(), lr=0.01, max_lag=a.max_lag).attach(lazy)
    dense.train()
    lazy.train()

    def batches(n, K):
        pick = edges[torch.randint(0, edges.shape[0], (n * B,), device=dev, generator=gen)]
        return torch.cat([pick, torch.randint(0, ni, (n * B, K), device=dev, generator=gen)], 1).view(n, B, 2 + K)

    def window(model, opt, bs):
        def run():
            for i in range(bs.shape[0]):
                step(model, opt, bs[i])
        return event_ms(run)

    for K in (16, 63):
        dense.n_negatives = lazy.n_negatives = K
        warm = batches(8, K)
        for i in range(8):
            step(dense, opt_d, warm[i])
            step(lazy, opt_l, warm[i])
        per = {"dense": [], "lazy": []}
        for blk in range(a.blocks):
            bs = batches(steps, K)
            for leg, model, opt in (("dense", dense, opt_d), ("lazy", lazy, opt_l)):
                ms = window(model, opt, bs) / steps
                per[leg].append(ms)
                print(json.dumps(dict(leg="window", optimizer=leg, K=K, block=blk, steps=steps, ms_per_step=round(ms, 4))), flush=True)
        d, l = per["dense"], per["lazy"]
        print(json.dumps(dict(leg="summary", K=K, dense_ms_per_step=[round(x, 4) for x in d], lazy_ms_per_step=[round(x, 4) for x in l],
                              dense_spread_ms=round(max(d) - min(d), 4), dense_minus_lazy_ms=round(sum(d) / len(d) - sum(l) / len(l), 4))),
              flush=True)
        # lag statistics and the flush alone: max_lag - 1 steps after a flush
        opt_l.flush()
        bs = batches(a.max_lag - 1, K)
        for i in range(bs.shape[0]):
            step(lazy, opt_l, bs[i])
        m, v, last, t = opt_l.row_state(lazy.table)
        behind = last < t
        live = behind & ((m != 0).any(1) | (v != 0).any(1))
        n_live = int(live.sum())
        lag = float((t - last[live]).double().mean()) if n_live else 0.0
        flush_ms = event_ms(opt_l.flush)
        print(json.dumps(dict(leg="flush", K=K, steps_since_flush=a.max_lag - 1, rows=int(last.numel()), rows_behind=int(behind.sum()),
                              rows_replayed=n_live, share_replayed=round(n_live / last.numel(), 4), mean_lag=round(lag, 1),
                              flush_ms=round(flush_ms, 4), ns_per_element_step=round(flush_ms * 1e6 / max(n_live * D * lag, 1), 4),
                              flush_ms_per_step_amortised=round(flush_ms / a.max_lag, 4))), flush=True)
        # the catch-up call and the apply (opt.step) alone, mid-window
        bs = batches(a.max_lag // 2 + a.rounds, K)
        for i in range(a.max_lag // 2):
            step(lazy, opt_l, bs[i])
        cu, ap_ = [], []
        for i in range(a.max_lag // 2, bs.shape[0]):
            rows = T.loss_stage.Ultra(lazy.tables).rows(bs[i], nu)
            plan = rowops.row_list_plan(rows, lazy.table.shape[0], None, D)
            cu.append(event_ms(lambda: opt_l.catch_up(lazy.table, plan)))
            opt_l.zero_grad()
            sum(lazy.loss(bs[i])).backward()
            ap_.append(event_ms(opt_l.step))
        print(json.dumps(dict(leg="call", variant="catch_up", K=K, rows_listed=int(rows.numel()), **med(cu))), flush=True)
        print(json.dumps(dict(leg="call", variant="apply (opt.step)", K=K, **med(ap_))), flush=True)
