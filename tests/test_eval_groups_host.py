"""CPU-only: tagrec_amd.user_group_split (training/utils.py:58-109) against the reference's own groups
(tests/golden/eval_groups.npz, tools/make_golden_eval_groups.py): same keys in the same order, same users per group,
for every method, k and distribution, from user -> items dicts, [E, 2] arrays and tensors alike; ValueError where the
reference raises."""
import numpy as np
import pytest
import torch

import tagrec_amd as T

DISTS = ("mid", "tail", "tiny")
METHODS = ("interaction", "user", "interval", "item")
KS = (2, 3, 4, 7)


def _dict(edges):
    d = {}
    for u, i in edges.tolist():
        d.setdefault(u, []).append(i)
    return d


def _inputs(fx, d, form):
    tr, te = fx[f"split.{d}.train"], fx[f"split.{d}.test"]
    if form == "dict":
        return _dict(te), _dict(tr)
    if form == "array":
        return te, tr
    return torch.from_numpy(te), torch.from_numpy(tr)


@pytest.mark.parametrize("form", ["dict", "array", "tensor"])
@pytest.mark.parametrize("d", DISTS)
def test_user_group_split_matches_reference(golden, d, form):
    fx = golden("eval_groups")
    test_ui, train_ui = _inputs(fx, d, form)
    checked = 0
    for method in METHODS:
        for k in KS:
            p = f"split.{d}.{method}.{k}"
            if p + ".error" in fx:
                with pytest.raises(ValueError):
                    T.user_group_split(test_ui, train_ui, k, method)
                continue
            got = T.user_group_split(test_ui, train_ui, k, method)
            assert list(got.keys()) == fx[p + ".keys"].tolist(), p
            want = np.split(fx[p + ".users"], np.cumsum(fx[p + ".sizes"])[:-1])
            for (n, users), ref in zip(got.items(), want):
                if form == "dict":                  # dict input: the reference's lists, in its order
                    assert isinstance(users, list) and users == ref.tolist(), (p, n)
                else:
                    assert sorted(np.asarray(users).tolist()) == sorted(ref.tolist()), (p, n)
            checked += 1
    assert checked >= 8


def test_user_group_split_quirks(golden):
    """The heavy-tailed distribution has a count that crosses several thresholds: still one group per n, and the
    threshold list is longer than k.  A split of a total below k raises."""
    fx = golden("eval_groups")
    test_ui, train_ui = _inputs(fx, "tail", "dict")
    got = T.user_group_split(test_ui, train_ui, 7, "interaction")
    assert len(got) < 7
    with pytest.raises(ValueError):
        T.user_group_split({0: [1]}, {}, 4, "user")


def test_user_group_split_counts_core():
    from tagrec_amd.evaluate import user_group_split_counts
    n = np.random.RandomState(0).randint(1, 50, size=1_000_000)
    groups = user_group_split_counts(n, 4)
    sizes = [len(p) for _, p in groups]
    assert sum(sizes) <= n.size and len(groups) >= 1
    bounds = [g for g, _ in groups]
    assert bounds == sorted(bounds)
    lo = 0
    for g, pos in groups:
        assert ((n[pos] > lo) & (n[pos] <= g)).all()
        lo = g
