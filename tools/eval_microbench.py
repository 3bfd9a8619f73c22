"""Time the fused evaluation pass with and without AUC (csrc/eval.hip): `fused_topk` against `fused_topk_auc` on random
tables, ~20 train items and ~10 test positives per user.
Usage: python tools/eval_microbench.py [n_user] [n_item] [D] [K] [n_test]     (needs a GPU; default 1 M x 1 M, 64, 20, 10)
Prints one JSON line: median ms of each pass over `reps` timed runs after one warm-up, and their ratio."""
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch

from tagrec_amd import evaluate as EV

n_user = int(sys.argv[1]) if len(sys.argv) > 1 else 1_000_000
n_item = int(sys.argv[2]) if len(sys.argv) > 2 else 1_000_000
D = int(sys.argv[3]) if len(sys.argv) > 3 else 64
K = int(sys.argv[4]) if len(sys.argv) > 4 else 20
n_test = int(sys.argv[5]) if len(sys.argv) > 5 else 10
reps = 3
dev = torch.device("cuda:0")
g = torch.Generator(device=dev).manual_seed(0)
U = torch.randn(n_user, D, device=dev, generator=g) * 0.1
I = torch.randn(n_item, D, device=dev, generator=g) * 0.1


def csr(per_user):
    """Per-user sorted, de-duplicated random item lists as (ptr int64 [n_user + 1], items int32)."""
    u = torch.arange(n_user, device=dev).repeat_interleave(per_user)
    key = torch.unique(u * n_item + torch.randint(0, n_item, (u.numel(),), device=dev, generator=g))
    ptr = torch.zeros(n_user + 1, dtype=torch.int64, device=dev)
    torch.cumsum(torch.bincount(key // n_item, minlength=n_user), 0, out=ptr[1:])
    return ptr, (key % n_item).to(torch.int32).contiguous()


train_ptr, train_items = csr(20)
test_ptr, test_items = csr(n_test)
users = torch.arange(n_user, device=dev)
passes = {
    "topk": lambda: EV.fused_topk(U, I, users, train_ptr, train_items, K),
    "topk_auc": lambda: EV.fused_topk_auc(U, I, users, train_ptr, train_items, test_ptr, test_items, K),
}
res = {"n_user": n_user, "n_item": n_item, "D": D, "K": K, "n_test": n_test}
outs = {}
for name, fn in passes.items():
    outs[name] = fn()
    torch.cuda.synchronize()
    ms = []
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        torch.cuda.synchronize()
        ms.append(a.elapsed_time(b))
    res[name + "_ms"] = sorted(ms)[reps // 2]
    print(name, [round(m, 1) for m in ms], flush=True)
res["ratio"] = res["topk_auc_ms"] / res["topk_ms"]
res["top_equal"] = bool(torch.equal(outs["topk"][0], outs["topk_auc"][0]))
num2, n_pos, n_neg = outs["topk_auc"][2:]
res["mean_auc"] = float((num2.double() / (2.0 * n_pos.double() * n_neg.double())).mean())
print(json.dumps(res))
