"""Time the item co-occurrence top-k (tagrec_amd.item_cooccurrence_topk, csrc/cooc.hip) per tier, beside what a user does
without it: torch.sparse.mm(A^T, A) and a per-row top-k of the product.

Usage: python tools/cooc_microbench.py [--shapes small,c2] [--rounds 3] [--k 10] [--workspace-gib 1.0]      (needs a GPU)
  small   synth.make_bipartite_device(100 k users, 100 k items, 5 M edges)
  c2      the C2 shape: 1 M users, 1 M items, 50 M edges
  For each shape: the CSR build, the D kernel, then `rounds` timed runs of the light tier (LDS hash table, D_i <= the kernel's
  limit), the hub launches (dense-path items above 2^18 visits, cut into parts) and the rest of the dense path (counter rows in
  a workspace of --workspace-gib), host-synchronised wall clock around each tier's launches (a tier is milliseconds or more, the
  clock's resolution does not matter) -- once with the hubs cut (the default) and once with every dense-path item on one block;
  the item counts, the largest D_i, the counter rows the budget gave; then the largest item ALONE on one block, the time the
  unsplit tier cannot go below.  Then the yardstick on the same graph, once: torch.sparse.mm(A^T, A) on coalesced COO operands and a
  top-k over row blocks of the product; its time, or the error that stopped it.  On the shapes outside --yardstick-shapes it is
  not attempted and the size of its partial products is recorded instead.
  Prints one JSON line per measurement."""
import argparse
import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch

import tagrec_amd as T
from tagrec_amd import cooc

dev = torch.device("cuda:0")
SHAPES = {"small": (100_000, 100_000, 5_000_000), "c2": (1_000_000, 1_000_000, 50_000_000)}


def wall(fn):
    torch.cuda.synchronize()
    t = time.perf_counter()
    out = fn()
    torch.cuda.synchronize()
    return time.perf_counter() - t, out


def yardstick(edges, nu, ni, k, D):
    """torch.sparse.mm(A^T, A), then per block of rows: densify, key = c^2 / (D_j + 1), torch.topk."""
    ones = torch.ones(edges.shape[0], device=dev)
    A = torch.sparse_coo_tensor(edges.t(), ones, (nu, ni)).coalesce()
    At = torch.sparse_coo_tensor(edges.t().flip(0), ones, (ni, nu)).coalesce()
    t_mm, C = wall(lambda: torch.sparse.mm(At, A).coalesce())
    inv = 1.0 / (D.double() + 1)

    def rows_topk():
        out = torch.empty(ni, k, dtype=torch.int64, device=dev)
        step = max(1, (1 << 28) // ni)                        # a dense block of at most 2^28 doubles
        for r0 in range(0, ni, step):
            r1 = min(ni, r0 + step)
            block = torch.index_select(C, 0, torch.arange(r0, r1, device=dev)).to_dense().double()
            out[r0:r1] = torch.topk(block * block * inv[None], min(k, ni), dim=1).indices
        return out
    t_topk, _ = wall(rows_topk)
    return {"sparse_mm_s": round(t_mm, 4), "product_nnz": int(C._nnz()), "row_topk_s": round(t_topk, 4), "total_s": round(t_mm + t_topk, 4)}


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--shapes", default="small,c2")
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--k", type=int, default=10)
    ap.add_argument("--workspace-gib", type=float, default=1.0)
    ap.add_argument("--yardstick-shapes", default="small", help="shapes on which torch.sparse.mm is attempted")
    a = ap.parse_args()
    budget = int(a.workspace_gib * (1 << 30))
    print(json.dumps(dict(device=torch.cuda.get_device_name(0), k=a.k, rounds=a.rounds, workspace_bytes=budget,
                          lds_limit=cooc.lds_limit_max())), flush=True)
    for name in a.shapes.split(","):
        nu, ni, ne = SHAPES[name]
        t_gen, ds = wall(lambda: T.synth.make_bipartite_device(nu, ni, ne, 7, dev))
        edges = ds.edge_index["train"]
        t_csr, csrs = wall(lambda: cooc.cooc_csrs(edges, nu, ni, dev))
        print(json.dumps(dict(shape=name, n_user=nu, n_item=ni, edges=int(edges.shape[0]), generate_s=round(t_gen, 3),
                              csr_build_s=round(t_csr, 3))), flush=True)
        top = cooc.lds_limit_max()
        res = {}
        for label, kw in (("hubs_split", {}), ("hubs_whole", {"split_hubs": False})):
            light, hub, heavy, total = [], [], [], []
            for r in range(a.rounds + 1):                     # the first run warms up
                st = {"time": True}
                t_all, out = wall(lambda: T.item_cooccurrence_topk(None, nu, ni, a.k, csrs=csrs, workspace_bytes=budget, stats=st, **kw))
                if r:
                    light.append(st["light_s"]), hub.append(st["hub_s"]), heavy.append(st["heavy_s"]), total.append(t_all)
            res[label] = out
            med = lambda v: round(sorted(v)[len(v) // 2], 4)
            D = out[2]
            print(json.dumps(dict(shape=name, leg="kernels", variant=label, n_light=st["n_light"], n_heavy=st["n_heavy"],
                                  n_hub=st["n_hub"], n_part=st["n_part"], max_D=st["max_D"], counter_rows=st["rows"],
                                  light_s=med(light), hub_s=med(hub), heavy_s=med(heavy), total_s=med(total),
                                  total_min_s=round(min(total), 4), total_max_s=round(max(total), 4),
                                  visits_light=int(D[D <= top].sum()), visits_heavy=int(D[D > top].sum()),
                                  visits_hub=int(D[D > cooc.DEFAULT_HUB_LIMIT].sum()), pads=int((out[0] < 0).sum()))), flush=True)
        same = all(torch.equal(x, y) for x, y in zip(res["hubs_split"], res["hubs_whole"]))
        # the largest item ALONE on one block (the dense-path entry point listed with that item only): what the tier cannot beat
        # without cutting it
        big = torch.argmax(D).to(torch.int32).reshape(1)
        row = torch.zeros(1, ni, dtype=torch.int32, device=dev)
        sink_id, sink_w = torch.empty(ni, a.k, dtype=torch.int32, device=dev), torch.empty(ni, a.k, device=dev)
        lib = T._lib.load()

        def alone():
            T._lib.check(lib.tagrec_cooc_topk_heavy_f32(csrs.iu_ptr, csrs.iu_idx, csrs.ui_ptr, csrs.ui_idx, D, big, 1, ni, a.k, 0, row,
                                                        1, sink_id, sink_w, T._lib.stream_ptr()), "heavy")
        alone()
        t_big = sorted(wall(alone)[0] for _ in range(a.rounds))
        print(json.dumps(dict(shape=name, leg="largest item alone on one block", item=int(big), D=int(D[big.long()]),
                              median_s=round(t_big[len(t_big) // 2], 4), split_equals_whole_bits=same)), flush=True)
        out = res["hubs_split"]
        if name not in a.yardstick_shapes.split(","):
            # not attempted: the product's partial products alone (one per visit, an int64 pair and a float each before they are
            # coalesced) are sum_i D_i * 20 bytes
            pairs = int(D.sum())
            print(json.dumps(dict(shape=name, leg="yardstick torch.sparse.mm + row top-k", not_run=True, partial_products=pairs,
                                  partial_product_bytes=pairs * 20)), flush=True)
            continue
        try:
            row = yardstick(edges, nu, ni, a.k, D)
        except (RuntimeError, torch.OutOfMemoryError) as e:     # the dense-ish product does not fit, or the backend refuses it
            row = {"error": type(e).__name__, "message": " ".join(str(e).split())[:200]}
            torch.cuda.empty_cache()
        print(json.dumps(dict(shape=name, leg="yardstick torch.sparse.mm + row top-k", **row)), flush=True)
        del ds, edges, csrs, out, D, res
        torch.cuda.empty_cache()
