"""Evaluation with the reference's protocol and result layout
(/root/reference/training/basic_test.py:30-111, training/utils.py:7-54):

    Basic_test(data).run(model) -> {"recall": [@k...], "precision": [...], "hr": [...],
                                    "ndcg": [...], "auc": [x]}          means over the test users

Per 512-user batch: `model.predict_rating` -> train positives masked with -1024
(basic_test.py:47) -> torch.topk(max(topks)) -> hit labels.  The reference ships
the top-k to a multiprocessing pool and runs sklearn's AUC per user on the host;
here labels, recall/precision/hr/ndcg and a rank-based AUC are computed on the
device from sorted (user, item) keys, one host read at the end.

    run(model, group_k=k) -> {f"inter<{n}-{len(users)}": result, ...}   (basic_test.py:94-111)

one result per sparsity group of `user_group_split` (training/utils.py:58-109),
from one set of per-user metrics reduced per group on the device.
"""
import numpy as np
import torch

from . import _lib
from .config import CFG as _GLOBAL_CFG

FUSED_WIDTHS = (16, 32, 64, 128, 192, 256, 384, 512)


def fused_topk(user_table, item_table, users, train_ptr, train_items, k):
    """Top-k item ids per user by sigmoid(u . i), train positives excluded -- one fused HIP pass over the item
    table (csrc/eval.hip) instead of a [users, n_item] rating matrix + mask + torch.topk."""
    U = _lib.require_gpu_tensor(user_table.contiguous(), torch.float32, "eval user table")
    I = _lib.require_gpu_tensor(item_table.contiguous(), torch.float32, "eval item table")
    users = users.to(U.device, torch.int64).contiguous()
    top = torch.empty(users.numel(), k, dtype=torch.int64, device=U.device)
    val = torch.empty(users.numel(), k, dtype=torch.float32, device=U.device)
    _lib.check(_lib.load().tagrec_eval_topk_f32(U, I, I.shape[0], U.shape[1], users, users.numel(), train_ptr, train_items, k,
                                                top, val, _lib.stream_ptr()), "eval_topk")
    return top, val


def fused_topk_auc(user_table, item_table, users, train_ptr, train_items, test_ptr, test_items, k):
    """`fused_topk` plus each user's AUC pair count in the same pass over the item table (csrc/eval.hip):
    returns (top, val, auc_num2, n_pos, n_neg), AUC = auc_num2 / (2 n_pos n_neg).  test_ptr / test_items: each
    user's test items as a CSR of sorted int32 ids (duplicates and train ids allowed; they are not positives)."""
    U = _lib.require_gpu_tensor(user_table.contiguous(), torch.float32, "eval user table")
    I = _lib.require_gpu_tensor(item_table.contiguous(), torch.float32, "eval item table")
    users = users.to(U.device, torch.int64).contiguous()
    top = torch.empty(users.numel(), k, dtype=torch.int64, device=U.device)
    val = torch.empty(users.numel(), k, dtype=torch.float32, device=U.device)
    num2, n_pos, n_neg = (torch.empty(users.numel(), dtype=torch.int64, device=U.device) for _ in range(3))
    _lib.check(_lib.load().tagrec_eval_topk_auc_f32(U, I, I.shape[0], U.shape[1], users, users.numel(), train_ptr, train_items,
                                                    test_ptr, test_items, k, top, val, num2, n_pos, n_neg, _lib.stream_ptr()),
               "eval_topk_auc")
    return top, val, num2, n_pos, n_neg


def _user_counts(user_items):
    """(users, per-user edge counts) of a user -> items dict (key order) or an [E, 2] array / tensor (ascending ids)."""
    if isinstance(user_items, dict):
        users = np.fromiter(user_items.keys(), dtype=np.int64, count=len(user_items))
        return users, np.fromiter((len(v) for v in user_items.values()), dtype=np.int64, count=len(user_items))
    if isinstance(user_items, torch.Tensor):
        cnt = torch.bincount(user_items[:, 0].to(torch.int64)).cpu().numpy()
    else:
        arr = np.asarray(user_items)
        cnt = np.bincount(arr[:, 0].astype(np.int64)) if len(arr) else np.zeros(0, np.int64)
    users = np.flatnonzero(cnt)
    return users, cnt[users]


def user_group_split_counts(n_inter, k, method="interaction"):
    """Core of `user_group_split` on per-user interaction counts: [(n, positions into n_inter), ...] in the
    reference's order.  Users of one n keep their order; a group is all users whose n lies in (previous n, n]."""
    n_inter = np.asarray(n_inter, dtype=np.int64)
    order = np.argsort(n_inter, kind="stable")
    ns, first, per_n = np.unique(n_inter[order], return_index=True, return_counts=True)
    if method == "interaction":
        tot, f = int(n_inter.sum()), 0
    elif method == "user":
        tot, f = len(n_inter), 1
    elif method == "interval":
        tot, f = (int(ns[-1]) if len(ns) else 0), 2
    else:
        tot, f = len(ns), 3
    if k == 0 or tot // k == 0:
        raise ValueError(f"user_group_split: cannot split a total of {tot} into {k} groups")
    step = tot // k
    end = list(range(step, tot + 1, step))
    if not end:
        raise ValueError(f"user_group_split: cannot split a total of {tot} into {k} groups")
    end[-1] = tot
    groups, count, i, lo = [], 0, 0, 0
    for j, n in enumerate(ns.tolist()):
        if f == 0:
            count += n * int(per_n[j])
        elif f == 1:
            count += int(per_n[j])
        elif f == 2:
            count = n
        else:
            count += 1
        if i >= len(end):
            raise ValueError("user_group_split: more groups than thresholds")
        if count >= end[i]:             # one n may cross several thresholds and still closes one group
            hi = int(first[j] + per_n[j])
            groups.append((n, order[lo:hi]))
            lo, i = hi, i + 1
    return groups


def user_group_split(test_ui, train_ui, k, method="interaction"):
    """training/utils.py:58-109: the test users grouped by interaction count (test + train edges) into about k
    groups, {n: users with count in (previous n, n]}, keys ascending.  method: "interaction" (equal shares of all
    interactions), "user" (of users), "interval" (of [0, max n]) or anything else (of the distinct counts).  Takes
    user -> items dicts (groups are lists, in key order) or [E, 2] arrays / tensors (groups are int64 arrays,
    ascending).  Raises ValueError where the reference raises (e.g. a total below k)."""
    users, n_test = _user_counts(test_ui)
    t_users, n_train = _user_counts(train_ui)
    n_inter = n_test.copy()
    if len(t_users) and len(users):
        if isinstance(train_ui, dict):
            lookup = dict(zip(t_users.tolist(), n_train.tolist()))
            n_inter += np.fromiter((lookup.get(u, 0) for u in users.tolist()), dtype=np.int64, count=len(users))
        else:
            dense = np.zeros(max(int(t_users[-1]), int(users.max())) + 1, dtype=np.int64)
            dense[t_users] = n_train
            n_inter += dense[users]
    out = {}
    for n, pos in user_group_split_counts(n_inter, k, method):
        out[n] = users[pos].tolist() if isinstance(test_ui, dict) else users[pos]
    return out


def _edge_keys(user_items, n_item, device):
    if isinstance(user_items, dict):
        us = np.fromiter((u for u, its in user_items.items() for _ in its), dtype=np.int64)
        its = np.fromiter((i for its in user_items.values() for i in its), dtype=np.int64)
    elif isinstance(user_items, torch.Tensor):       # [E,2] tensor, possibly already on the device
        u = user_items[:, 0].to(device, torch.int64)
        i = user_items[:, 1].to(device, torch.int64)
        return u, i, torch.sort(u * n_item + i).values
    else:                                   # [E,2] array
        arr = np.asarray(user_items)
        us, its = arr[:, 0].astype(np.int64), arr[:, 1].astype(np.int64)
    u = torch.from_numpy(us).to(device)
    i = torch.from_numpy(its).to(device)
    key = torch.sort(u * n_item + i).values
    return u, i, key


def _member(keys_sorted, k):
    if keys_sorted.numel() == 0:
        return torch.zeros_like(k, dtype=torch.bool)
    pos = torch.searchsorted(keys_sorted, k).clamp_(max=keys_sorted.numel() - 1)
    return keys_sorted[pos] == k


def minibatch(data, batch_size):
    """training/utils.py:48-54 (a trailing empty slice is produced when len % batch == 0)."""
    step = len(data) // batch_size + 1
    for i in range(step):
        yield data[i * batch_size:(i + 1) * batch_size]


class Basic_test:
    def __init__(self, data, args=None, config=None, with_auc=None):
        self.cfg = config if config is not None else _GLOBAL_CFG
        self.device = torch.device(self.cfg["device"])
        self.n_item = data.num["item"]
        self.n_user = data.num["user"]
        self.train_u, self.train_i, _ = _edge_keys(data.user_items["train"], self.n_item, self.device)
        self.sets = {}
        self.test_csr = {}
        names = ["test"] + (["val"] if self.cfg.get("has_val") else [])
        for name in names:
            u, i, key = _edge_keys(data.user_items[name], self.n_item, self.device)
            cnt = torch.bincount(u, minlength=self.n_user)
            self.sets[name] = (key, cnt)
            # per-user sorted, de-duplicated test items for the fused AUC pass
            ukey = torch.unique_consecutive(key)
            ptr = torch.zeros(self.n_user + 1, dtype=torch.int64, device=self.device)
            torch.cumsum(torch.bincount(ukey // self.n_item, minlength=self.n_user), 0, out=ptr[1:])
            self.test_csr[name] = (ptr, (ukey % self.n_item).to(torch.int32).contiguous())
        order = torch.argsort(self.train_u, stable=True)
        self.train_u, self.train_i = self.train_u[order], self.train_i[order]
        self.train_ptr = torch.zeros(self.n_user + 1, dtype=torch.int64, device=self.device)
        torch.cumsum(torch.bincount(self.train_u, minlength=self.n_user), 0, out=self.train_ptr[1:])
        self.with_auc = (self.n_item <= 50_000) if with_auc is None else with_auc
        # above 50 000 items the default takes AUC from the fused pass (where that pass applies)
        self.fused_auc = with_auc is None and not self.with_auc
        # per-user SORTED train items for the fused kernel's mask look-up
        skey = torch.sort(self.train_u * self.n_item + self.train_i).values
        self.train_items_sorted = (skey % self.n_item).to(torch.int32).contiguous()
        self.fused = bool(self.cfg.get("eval_fused", True))

    @torch.no_grad()
    def run(self, model, istest=False, group_k=0, all_users=None):
        model.eval()
        name = "val" if (not istest and self.cfg.get("has_val")) else "test"
        key, cnt = self.sets[name]
        if all_users is None:
            all_users = torch.nonzero(cnt > 0).flatten()
        else:
            all_users = torch.as_tensor(all_users, dtype=torch.int64, device=self.device)
        topks = list(self.cfg["topks"])
        kmax = max(topks)
        disc = 1.0 / torch.log2(torch.arange(2, kmax + 2, device=self.device, dtype=torch.float64))
        sums = {m: torch.zeros(len(topks), dtype=torch.float64, device=self.device)
                for m in ("recall", "precision", "hr", "ndcg")}
        auc_sum = torch.zeros((), dtype=torch.float64, device=self.device)
        # group_k > 1: metrics per user ([n, 4, len(topks)]: recall, precision, hr, ndcg; AUC), reduced per group below
        rows = auc_rows = None
        if group_k > 1:
            rows = torch.zeros(all_users.numel(), 4, len(topks), dtype=torch.float64, device=self.device)
            auc_rows = torch.full((all_users.numel(),), float("nan"), dtype=torch.float64, device=self.device)

        def score(users, top, at=0):
            label = _member(key, users[:, None] * self.n_item + top.clamp_min(0))            # get_label
            # the fused kernel pads a list with id -1 when a user has fewer than k un-masked items: never a hit
            label = (label & (top >= 0)).to(torch.float64)
            n_true = cnt[users].to(torch.float64)
            for j, k in enumerate(topks):
                right = label[:, :k].sum(1)
                ideal = torch.cumsum(disc[:k], 0)[(torch.clamp(n_true, max=k) - 1).long()]
                ndcg = (label[:, :k] * disc[:k]).sum(1) / ideal
                if rows is not None:
                    r = rows[at:at + users.numel(), :, j]
                    r[:, 0], r[:, 1], r[:, 2], r[:, 3] = right / n_true, right / k, right > 0, ndcg
                    continue
                sums["recall"][j] += (right / n_true).sum()
                sums["precision"][j] += right.sum() / k
                sums["hr"][j] += (right > 0).sum()
                sums["ndcg"][j] += ndcg.sum()

        with_auc = self.with_auc
        tables = model.forward()[:2] if (self.fused and not self.with_auc and hasattr(model, "forward")) else None
        if tables is not None and tables[0].shape[1] in FUSED_WIDTHS and tables[0].is_cuda and kmax <= 64:
            # one propagation, one fused score/mask/top-k (+ AUC) pass; metrics in user chunks to bound temporaries
            if self.fused_auc:
                ptr, items = self.test_csr[name]
                top, _, num2, n_pos, n_neg = fused_topk_auc(tables[0], tables[1], all_users, self.train_ptr,
                                                            self.train_items_sorted, ptr, items, kmax)
                auc_u = num2.double() / (2.0 * n_pos.double() * n_neg.double())
                with_auc = True
            else:
                top, _ = fused_topk(tables[0], tables[1], all_users, self.train_ptr, self.train_items_sorted, kmax)
            for lo in range(0, all_users.numel(), 1 << 18):
                score(all_users[lo:lo + (1 << 18)], top[lo:lo + (1 << 18)], lo)
            if with_auc:
                if auc_rows is not None:
                    auc_rows = auc_u
                else:
                    auc_sum = auc_u.sum()
        else:
            at = 0
            for users in minibatch(all_users, self.cfg["test_batch"]):
                if users.numel() == 0:
                    continue
                rating = model.predict_rating(users)
                # mask the users' train items (basic_test.py:42-47)
                lo, hi = self.train_ptr[users], self.train_ptr[users + 1]
                deg = hi - lo
                row = torch.repeat_interleave(torch.arange(users.numel(), device=self.device), deg)
                start = torch.repeat_interleave(lo - torch.cumsum(deg, 0) + deg, deg)
                col = self.train_i[start + torch.arange(row.numel(), device=self.device)]
                rating[row, col] = -(1 << 10)
                _, top = torch.topk(rating, k=kmax)
                score(users, top, at)
                if self.with_auc:
                    auc = self._auc(rating, users, key)
                    if auc_rows is not None:
                        auc_rows[at:at + users.numel()] = auc
                    else:
                        auc_sum += auc.sum()
                at += users.numel()
        if rows is not None:
            return self._group_results(name, all_users, group_k, rows, auc_rows if with_auc else None)
        n = float(all_users.numel())
        out = {m: (v / n).cpu().tolist() for m, v in sums.items()}
        out["auc"] = [float(auc_sum.cpu()) / n] if with_auc else [float("nan")]
        return out

    def _group_results(self, name, all_users, group_k, rows, auc_rows):
        """basic_test.py:94-108: the users split by `user_group_split`; each group's metrics are means over its
        users of the per-user rows, summed per group on the device, one host read."""
        _, cnt = self.sets[name]
        n_inter = cnt[all_users] + self.train_ptr[all_users + 1] - self.train_ptr[all_users]
        groups = user_group_split_counts(n_inter.cpu().numpy(), group_k)
        gid = np.full(all_users.numel(), len(groups), dtype=np.int64)      # users past the last group: dropped
        for g, (_, pos) in enumerate(groups):
            gid[pos] = g
        gid = torch.from_numpy(gid).to(self.device)
        tot = torch.zeros(len(groups) + 1, *rows.shape[1:], dtype=torch.float64, device=self.device)
        tot.index_add_(0, gid, rows)
        auc = torch.zeros(len(groups) + 1, dtype=torch.float64, device=self.device)
        if auc_rows is not None:
            auc.index_add_(0, gid, auc_rows)
        tot, auc = tot.cpu().numpy(), auc.cpu().numpy()
        out = {}
        for g, (n, pos) in enumerate(groups):
            size = float(len(pos))
            res = {m: (tot[g, j] / size).tolist() for j, m in enumerate(("recall", "precision", "hr", "ndcg"))}
            res["auc"] = [float(auc[g]) / size] if auc_rows is not None else [float("nan")]
            out[f"inter<{n}-{len(pos)}"] = res
        return out

    def _auc(self, rating, users, key):
        """Per-user ROC AUC over the un-masked items (training/utils.py:37-45), as the
        Mann-Whitney statistic with average ranks for ties (what sklearn computes)."""
        n_item = rating.shape[1]
        items = torch.arange(n_item, device=self.device)
        pos = _member(key, users[:, None] * self.n_item + items[None, :])
        valid = rating >= 0
        r = rating.double().masked_fill(~valid, -1.0)
        srt, idx = torch.sort(r, dim=1)
        # average rank of ties: (first index + last index)/2 + 1 over equal values
        first = torch.searchsorted(srt, srt, right=False)
        last = torch.searchsorted(srt, srt, right=True)
        avg_rank_sorted = (first + last + 1).double() / 2.0
        ranks = torch.empty_like(avg_rank_sorted).scatter_(1, idx, avg_rank_sorted)
        n_invalid = (~valid).sum(1, keepdim=True).double()
        ranks = ranks - n_invalid                       # ranks among valid items only
        posv = pos & valid
        n_pos = posv.sum(1).double()
        n_neg = valid.sum(1).double() - n_pos
        u_stat = (ranks * posv).sum(1) - n_pos * (n_pos + 1) / 2.0
        return u_stat / (n_pos * n_neg)
