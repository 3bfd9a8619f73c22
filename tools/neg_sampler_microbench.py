"""Time one epoch's negative sampling (tagrec_sample_negative_ex_i64, csrc/sampler.hip) at the C2 shape.

Usage: python tools/neg_sampler_microbench.py [--scale 1.0] [--rounds 9]      (needs a GPU)
  One sample of all train edges (1 M x 1 M, 50 M edges, D = 64 tables) per measurement, for the proposals uniform and
  popularity (degree ** 0.75 through an alias table) and M = 1, 2, 4, 8, 16 candidates per edge, next to the old uniform
  kernel (tagrec_sample_negative_i64).  All variants are interleaved in one process: rounds of every variant once, device
  events around each call, warm-up first; median, minimum and maximum per variant.
  Algorithmic bytes of a variant = n_rows * (1 + M) * D * 4 (the user row and M candidate rows per edge; for M = 1 no
  row is read and no rate is given).  The ceiling they are judged against is measured in the same run: random 256-byte
  rows gathered from a table of the item table's size by tagrec_probe_gather_rows_f32.
Prints one JSON line per measurement."""
import argparse
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch

import tagrec_amd as T
from tagrec_amd import _lib, train_data

dev = torch.device("cuda:0")
D = 64


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


def gather_rate(n_rows, rounds):
    """GB/s of row bytes: 2^26 random 256-byte rows out of a [n_rows, 64] table."""
    lib = _lib.load()
    n_idx = 1 << 26
    table = torch.empty(n_rows, D, device=dev).normal_()
    idx = torch.randint(0, n_rows, (n_idx,), device=dev, dtype=torch.int32)
    sink = torch.empty(lib.tagrec_probe_gather_out_floats(), device=dev)
    res = interleaved({"g": lambda: _lib.check(lib.tagrec_probe_gather_rows_f32(_lib.ptr(table), n_rows, D, _lib.ptr(idx), n_idx,
                                                                                 _lib.ptr(sink), _lib.stream_ptr()), "gather")},
                      rounds, 2)["g"]
    return n_idx * 4.0 * D / (res[0] * 1e-3) / 1e9, res


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--scale", type=float, default=1.0, help="shrink the C2 graph (nodes and edges)")
    ap.add_argument("--rounds", type=int, default=9)
    a = ap.parse_args()
    nu = ni = max(int(1_000_000 * a.scale), 2000)
    ne = max(int(50_000_000 * a.scale), 40000)
    ds = T.synth.make_bipartite_device(nu, ni, ne, seed=1, device=dev)
    e = ds.edge_index["train"]
    pos = train_data._Positives(e[:, 0], e[:, 1], nu, ni)
    left = e[:, 0].contiguous()
    n_rows = left.numel()
    alias = pos.popularity_alias(0.75)
    g = torch.Generator(device=dev).manual_seed(1)
    U = torch.randn(nu, D, device=dev, generator=g) * 0.1
    I = torch.randn(ni, D, device=dev, generator=g) * 0.1
    print(json.dumps({"shape": "C2", "scale": a.scale, "users": nu, "items": ni, "edges": n_rows, "D": D,
                      "device": torch.cuda.get_device_name(0)}), flush=True)

    rate, gres = gather_rate(ni, a.rounds)
    print(json.dumps({"leg": "gather_256B_rows", "table_rows": ni, "median_ms": round(gres[0], 4), "min_ms": round(gres[1], 4),
                      "max_ms": round(gres[2], 4), "row_GBps": round(rate, 1)}), flush=True)

    seed = (2020 << 20) + 1
    lib = _lib.load()
    neg = torch.empty_like(left)

    def old_entry():
        _lib.check(lib.tagrec_sample_negative_i64(_lib.ptr(left), n_rows, _lib.ptr(pos.rowptr), _lib.ptr(pos.cols), nu, ni, seed,
                                                  _lib.ptr(neg), _lib.stream_ptr()), "old entry")

    def new_entry(table, M):
        prob, idx = table if table is not None else (None, None)
        tabs = (_lib.ptr(U), D, _lib.ptr(I), D, D) if M > 1 else (None, 0, None, 0, 0)

        def run():
            _lib.check(lib.tagrec_sample_negative_ex_i64(_lib.ptr(left), n_rows, _lib.ptr(pos.rowptr), _lib.ptr(pos.cols), nu, ni,
                                                         seed, M, _lib.ptr(prob), _lib.ptr(idx), *tabs, _lib.ptr(neg), None, None,
                                                         _lib.stream_ptr()), "new entry")
        return run

    variants = {"old_uniform_M1": old_entry}
    for prop, table in (("uniform", None), ("popularity", alias)):
        for M in (1, 2, 4, 8, 16):
            variants[f"{prop}_M{M}"] = new_entry(table, M)
    res = interleaved(variants, a.rounds, 2)
    old = res["old_uniform_M1"]
    for k, (med, lo, hi) in res.items():
        M = int(k.rsplit("M", 1)[1])
        line = {"leg": "epoch_sample", "variant": k, "median_ms": round(med, 4), "min_ms": round(lo, 4), "max_ms": round(hi, 4),
                "ratio_to_old": round(med / old[0], 4)}
        if M > 1:
            gbps = n_rows * (1.0 + M) * D * 4 / (med * 1e-3) / 1e9
            line.update(algorithmic_GB=round(n_rows * (1.0 + M) * D * 4 / 1e9, 2), algorithmic_GBps=round(gbps, 1),
                        fraction_of_gather_rate=round(gbps / rate, 4))
        print(json.dumps(line), flush=True)
