"""Generate tests/golden/eval_groups.npz by running the REFERENCE's grouped evaluation on the CPU.

    python tools/make_golden_eval_groups.py

The reference is imported unmodified through oracle/make_golden.py's `import_reference` (which this script leaves
untouched); the fixture holds inputs and the reference's outputs only.

  * `training.basic_test.Basic_test(data, args).run(stub, istest=True, group_k=k)` for k in 2, 3, 4 on a fixed random
    rating matrix (`rating`, train / test edges `bt.train` / `bt.test`).  The stub's predict_rating returns rows of
    that matrix, args.pool.map is the builtin map (no process pool).  Per k: `bt.k{k}.keys` (the result keys in order)
    and `bt.k{k}.{g}.{metric}`.
  * `training.utils.user_group_split` for all four methods on three interaction distributions (`split.{d}.train` /
    `.test`: [E, 2] edges in dict insertion order; one with a heavy tail so that one n crosses several thresholds,
    one so small that some splits raise).  Per (d, method, k): `.keys` (the n's in order), `.sizes` and `.users` (the
    groups' users concatenated, in the reference's order), or `.error` (the exception's class name)."""
import os
import sys
import types

import numpy as np

sys.dont_write_bytecode = True
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
OUT = os.path.join(ROOT, "tests", "golden")
METHODS = ("interaction", "user", "interval", "item")
SPLIT_KS = (2, 3, 4, 7)


def _dict(edges):
    d = {}
    for u, i in edges.tolist():
        d.setdefault(u, []).append(i)
    return d


def main():
    import torch
    sys.path.insert(0, ROOT)
    from oracle.make_golden import import_reference
    R = import_reference()
    CFG = R["CFG"]
    CFG.update(device=torch.device("cpu"), has_val=False, topks=[10, 20], test_batch=1000)  # no empty trailing batch
    fx = {}

    # ---- Basic_test.run(..., group_k=k) on fixed scores
    rng = np.random.RandomState(11)
    nu, ni = 48, 90
    rating = rng.rand(nu, ni).astype(np.float32)
    rating[:, 5] = rating[:, 6]                                          # a few exact ties across items
    train, test = [], []
    for u in range(nu):
        n_tr = int(min(ni - 30, 1 + rng.zipf(1.6)))                      # heavy-tailed train degrees
        n_te = int(rng.randint(1, 12))
        its = rng.choice(ni, n_tr + n_te, replace=False)
        train += [(u, int(i)) for i in its[:n_tr]]
        test += [(u, int(i)) for i in its[n_tr:]]
    train, test = np.array(train, np.int64), np.array(test, np.int64)
    fx.update({"rating": rating, "topks": np.array(CFG["topks"]), "bt.train": train, "bt.test": test})

    class Stub(torch.nn.Module):
        def __init__(self, r):
            super().__init__()
            self.r = torch.from_numpy(r)

        def predict_rating(self, users):
            return self.r[users].clone()

    data = types.SimpleNamespace(user_items={"train": _dict(train), "test": _dict(test)})
    args = types.SimpleNamespace(pool=types.SimpleNamespace(map=map))
    tester = R["basic_test"].Basic_test(data, args)
    for k in (2, 3, 4):
        res = tester.run(Stub(rating), istest=True, group_k=k)
        fx[f"bt.k{k}.keys"] = np.array(list(res.keys()))
        for g, r in enumerate(res.values()):
            for m, v in r.items():
                fx[f"bt.k{k}.{g}.{m}"] = np.array(v, dtype=np.float64)
        print("group_k", k, list(res.keys()))

    # ---- user_group_split on three distributions
    rng = np.random.RandomState(5)
    dists = {}
    e_tr, e_te = [], []                                                  # moderate spread, a few duplicate ids
    for u in rng.permutation(200):
        e_tr += [(u, int(i)) for i in rng.randint(0, 500, rng.randint(1, 30))]
        e_te += [(u, int(i)) for i in rng.randint(0, 500, rng.randint(1, 8))]
    dists["mid"] = (e_tr, e_te)
    e_tr, e_te = [], []                                                  # heavy tail: a few users hold most edges
    for u in rng.permutation(150):
        n = int(min(3000, rng.zipf(1.3)))
        e_tr += [(u, int(i)) for i in rng.randint(0, 5000, n)]
        e_te += [(u, int(i)) for i in rng.randint(0, 5000, 1 + n // 5)]
    e_tr += [(900, i) for i in range(4000)]                              # one user with 4000 + 900 interactions
    e_te += [(900, i) for i in range(900)]
    e_te += [(901, 1)]                                                   # a test user with no train edges
    dists["tail"] = (e_tr, e_te)
    dists["tiny"] = ([(0, 1), (1, 2), (1, 3), (2, 4)], [(0, 5), (1, 6), (2, 7), (2, 8)])
    for d, (e_tr, e_te) in dists.items():
        e_tr, e_te = np.array(e_tr, np.int64), np.array(e_te, np.int64)
        fx[f"split.{d}.train"], fx[f"split.{d}.test"] = e_tr, e_te
        for method in METHODS:
            for k in SPLIT_KS:
                p = f"split.{d}.{method}.{k}"
                try:
                    groups = R["tr_utils"].user_group_split(_dict(e_te), _dict(e_tr), k, method)
                except Exception as exc:                                 # recorded: ours must raise too
                    fx[p + ".error"] = np.array(type(exc).__name__)
                    print(p, "raises", type(exc).__name__)
                    continue
                fx[p + ".keys"] = np.array(list(groups.keys()), np.int64)
                fx[p + ".sizes"] = np.array([len(v) for v in groups.values()], np.int64)
                fx[p + ".users"] = np.array([u for v in groups.values() for u in v], np.int64)
    path = os.path.join(OUT, "eval_groups.npz")
    np.savez_compressed(path, **fx)
    print("wrote", path, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
