"""CPU-only: the host side of the extended negative sampler -- Vose's alias table, the three config keys, and the
Python-int restatement of the kernel's alias draw (the one tests/test_gpu_neg_sampler.py compares the kernel with)."""
import numpy as np
import pytest

import tagrec_amd as T
from tagrec_amd import train_data

M64 = (1 << 64) - 1


def py_mix64(z):
    z = (z + 0x9E3779B97F4A7C15) & M64
    z = ((z ^ (z >> 30)) * 0xBF58476D1CE4E5B9) & M64
    z = ((z ^ (z >> 27)) * 0x94D049BB133111EB) & M64
    return z ^ (z >> 31)


def py_cand_base(seed, e, c):
    base0 = py_mix64(seed ^ py_mix64(e))
    return base0 if c == 0 else py_mix64((base0 + (c << 32)) & M64)


def py_alias_try(base, t, prob, alias):
    """Try t of the stream `base`: column j, a 24-bit uniform u (u * 2^-24 is exact in fp32, and so is the comparison with
    the stored fp32 prob when both are taken as doubles)."""
    n = len(prob)
    j = (py_mix64((base + 2 * t) & M64) * n) >> 64
    u = (py_mix64((base + 2 * t + 1) & M64) >> 40) * 2.0 ** -24
    return j if u < float(prob[j]) else int(alias[j])


def py_candidates(left, rows, n_right, seed, n_cand, table=None):
    """[entries][n_cand] candidate ids: the rejection loop (at most 4096 tries, the last kept) on each candidate's stream."""
    out = []
    for e, l in enumerate(left):
        cands = []
        for c in range(n_cand):
            base = py_cand_base(seed, e, c)
            for t in range(4096):
                if table is None:
                    draw = (py_mix64((base + t) & M64) * n_right) >> 64
                else:
                    draw = py_alias_try(base, t, table[0], table[1])
                if draw not in rows[l]:
                    break
            cands.append(draw)
        out.append(cands)
    return out


def implied_p(prob, alias):
    """The distribution the stored fp32 table draws from: p_i = (prob[i] + sum_{j: alias[j] = i} (1 - prob[j])) / n."""
    prob = prob.astype(np.float64)
    p = prob.copy()
    np.add.at(p, alias.astype(np.int64), 1.0 - prob)
    return p / len(prob)


def power_law_degrees(n=200):
    return np.maximum(1, (300.0 / np.arange(1, n + 1) ** 0.9).astype(np.int64))


WEIGHT_CASES = {"hand": np.array([0, 1, 2, 0, 5, 1e-3, 7, 7], dtype=np.float64),
                "power_law_200": power_law_degrees().astype(np.float64) ** 0.75}


@pytest.mark.parametrize("name", sorted(WEIGHT_CASES))
def test_alias_table_implies_the_weights(name):
    w = WEIGHT_CASES[name]
    prob, alias = train_data.alias_table(w)
    assert prob.dtype == np.float32 and alias.dtype == np.int32 and prob.shape == alias.shape == w.shape
    assert np.all(prob >= 0) and np.all(prob <= 1) and np.all(alias >= 0) and np.all(alias < len(w))
    p = implied_p(prob, alias)
    assert np.max(np.abs(p - w / w.sum())) < 1e-6
    assert np.all(p[w == 0] == 0.0)
    again = train_data.alias_table(w.copy())
    assert np.array_equal(again[0], prob) and np.array_equal(again[1], alias)


@pytest.mark.parametrize("bad", [[1.0, float("nan")], [1.0, float("inf")], [1.0, -0.5], [0.0, 0.0, 0.0]])
def test_alias_table_refuses_bad_weights(bad):
    with pytest.raises(T.TagrecError):
        train_data.alias_table(bad)


def test_config_keys_and_refusals():
    cfg = T.get_config("lightgcn")
    assert (cfg["neg_sampling"], cfg["neg_pop_alpha"], cfg["neg_candidates"]) == ("uniform", 0.75, 1)
    assert T.get_config("ngcf", neg_sampling="popularity", neg_candidates=16)["neg_candidates"] == 16
    with pytest.raises(T.TagrecError):
        T.get_config("lightgcn", neg_sampling="hardest")
    for bad in (0, 17, 2.0):
        with pytest.raises(T.TagrecError):
            T.get_config("lightgcn", neg_candidates=bad)


def test_alias_draw_restatement_reproduces_the_distribution():
    """Inputs: the hand weights with the 1e-3 cell dropped (it would expect 0.009 draws), i.e. w = [0, 1, 2, 0, 5, 0, 7, 7]:
    200 000 draws expect at least 200 000 / 22 = 9 090 in every non-zero cell.  Seed 77, entry e = counter, candidate 0,
    try 0.  Bound: the project's chi2 < dof + 6 sqrt(2 dof) (tests/test_gpu_e2e.py)."""
    w = np.array([0, 1, 2, 0, 5, 0, 7, 7], dtype=np.float64)
    prob, alias = train_data.alias_table(w)
    p = implied_p(prob, alias)
    n = 200_000
    assert np.all(n * p[p > 0] >= 5)
    cnt = np.zeros(len(w))
    for e in range(n):
        cnt[py_alias_try(py_cand_base(77, e, 0), 0, prob, alias)] += 1
    assert np.all(cnt[p == 0] == 0)
    live = p > 0
    exp = n * p[live]
    chi2 = ((cnt[live] - exp) ** 2 / exp).sum()
    dof = int(live.sum()) - 1
    print(f"chi2 {chi2:.2f} dof {dof} bound {dof + 6 * np.sqrt(2 * dof):.2f}")
    assert chi2 < dof + 6 * np.sqrt(2 * dof), (chi2, dof)
