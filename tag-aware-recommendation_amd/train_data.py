"""Triplet producers with the reference's protocol (/root/reference/train_data):

    Abstract_training_data.reset() / .mini_batch()      abstract.py:4-23
    BPR_training_data(data)                              bpr_training_data.py:12-45
    TransTag_training_data(data)                         transe_training_data.py:42-70

The reference samples negatives in a forked `multiprocessing.Pool` with a Python
rejection loop per edge (train_data/utils.py:19-28) and copies the epoch's
[E,3] array to the device.  Here the epoch is sampled ON the device by a HIP
kernel (csrc/rowops.hip `sample_negative_kernel`): per edge, counter-based
uniform draws, membership test by binary search in the user's sorted positive
list, re-draw until a non-positive comes up; then a device-side shuffle.
Same distribution (one uniform non-train item per train edge); the reference's
own stream is not reproducible from its seed, so parity runs use
`Fixed_training_data` with arrays shared by both sides.

Beyond the reference (config keys `neg_sampling`, `neg_pop_alpha`, `neg_candidates`; csrc/sampler.hip): a
popularity-weighted proposal through an alias table, and dynamic hard negatives -- several candidates per edge, of
which the one the current model scores highest is kept.  The defaults give the uniform stream above bit for bit.
"""
import numpy as np
import torch

from . import _lib
from .config import CFG as _GLOBAL_CFG, check_neg_sampling, check_negatives, check_ranking, check_softmax_over


def alias_table(weights):
    """Vose's alias method on the host in float64: weights [n] -> (prob float32 [n], alias int32 [n]).  Column j is drawn
    uniformly and kept with probability prob[j], else alias[j] is taken, so id i comes up with probability
    (prob[i] + sum over j with alias[j] == i of (1 - prob[j])) / n = w_i / sum(w).  Deterministic, O(n); a zero weight gets
    prob 0 and is nobody's alias, so it is never drawn."""
    w = np.asarray(weights, dtype=np.float64).reshape(-1)
    if w.size == 0 or not np.all(np.isfinite(w)) or np.any(w < 0) or not w.sum() > 0:
        raise _lib.TagrecError("alias_table: weights must be finite, non-negative and not all zero")
    n = w.size
    p = w * (n / w.sum())
    prob = np.ones(n, dtype=np.float64)
    alias = np.arange(n, dtype=np.int64)
    # two stacks; the zero weights are popped first, while columns with mass to give are certain to be left
    small = [int(i) for i in np.flatnonzero((p < 1.0) & (w > 0))] + [int(i) for i in np.flatnonzero(w == 0)]
    large = [int(i) for i in np.flatnonzero(p >= 1.0)]
    p = p.tolist()
    while small and large:
        s, l = small.pop(), large.pop()
        prob[s], alias[s] = p[s], l
        p[l] = (p[l] + p[s]) - 1.0
        (small if p[l] < 1.0 else large).append(l)
    # what is left on either stack is 1 up to rounding: the column keeps itself
    return prob.astype(np.float32), alias.astype(np.int32)


class Abstract_training_data:
    def __init__(self, args=None, config=None):
        cfg = config if config is not None else _GLOBAL_CFG
        self.device = torch.device(cfg["device"])
        self.cpu_core = cfg["cpu_core"]
        self.all_train_data = None
        self.batch_size = cfg["train_batch"]

    def get_all_training_data(self):
        raise NotImplementedError

    def reset(self):
        self.all_train_data = self.get_all_training_data()

    def mini_batch(self):
        """abstract.py:17-23, the loop as written: once fewer than 2*batch rows remain the slice
        runs to the end -- and the loop still advances, so a short final slice repeats the tail."""
        n = self.all_train_data.shape[0]
        for i in range(0, n, self.batch_size):
            if i + 2 * self.batch_size > n:
                yield self.all_train_data[i:]
            else:
                yield self.all_train_data[i:i + self.batch_size]


class _Positives:
    """Sorted positive lists per left id as a device CSR (rowptr int64, cols int32), built once."""

    def __init__(self, left, right, n_left, n_right):
        key = torch.unique(left * n_right + right)
        l = torch.div(key, n_right, rounding_mode="floor")
        self.rowptr = torch.zeros(n_left + 1, dtype=torch.int64, device=left.device)
        torch.cumsum(torch.bincount(l, minlength=n_left), 0, out=self.rowptr[1:])
        self.cols = (key - l * n_right).to(torch.int32).contiguous()
        self.n_left, self.n_right = int(n_left), int(n_right)

    def sample(self, left, seed, n_cand=1, alias=None, user_table=None, item_table=None, return_candidates=False):
        """One non-positive draw per entry of `left` (HIP kernel, counter-based generator).  Defaults: the uniform draw.
        alias = (prob float32 [n_right], alias int32 [n_right]) on the device: draws follow that alias table instead.
        n_cand > 1: that many candidates per entry, the one with the highest user_table[left] . item_table[candidate]
        is returned (first arg-max; float32 tables [n_left, D] / [n_right, D], row views of wider tensors allowed).
        return_candidates: -> (neg, candidates int64 [n, n_cand], scores float32 [n, n_cand] or None when n_cand == 1)."""
        left = left.contiguous()
        neg = torch.empty_like(left)
        if left.numel() == 0:                     # (an empty tensor has no device pointer to hand over)
            n_cand = int(n_cand)
            return (neg, neg.new_empty((0, n_cand)), None if n_cand == 1 else neg.new_empty((0, n_cand), dtype=torch.float32)) \
                if return_candidates else neg
        if n_cand == 1 and alias is None and not return_candidates:
            _lib.check(_lib.load().tagrec_sample_negative_i64(left, left.numel(), self.rowptr, self.cols, self.n_left,
                                                              self.n_right, int(seed), neg, _lib.stream_ptr()), "sample_negative")
            return neg
        prob = idx = None
        if alias is not None:
            prob = _lib.require_gpu_tensor(alias[0], torch.float32, "sample: alias prob")
            idx = _lib.require_gpu_tensor(alias[1], torch.int32, "sample: alias ids")
            if prob.shape != (self.n_right,) or idx.shape != (self.n_right,):
                raise _lib.TagrecError(f"sample: the alias table must hold {self.n_right} columns")
        U = I = None
        ld_u = ld_i = D = 0
        if n_cand != 1:
            U, ld_u = self._table(user_table, self.n_left, "user_table")
            I, ld_i = self._table(item_table, self.n_right, "item_table")
            D = U.shape[1]
            if I.shape[1] != D:
                raise _lib.TagrecError(f"sample: user_table has {D} columns, item_table {I.shape[1]}")
        cand = torch.empty((left.numel(), n_cand), dtype=torch.int64, device=left.device) if return_candidates else None
        score = torch.empty((left.numel(), n_cand), dtype=torch.float32, device=left.device) \
            if return_candidates and n_cand != 1 else None
        _lib.check(_lib.load().tagrec_sample_negative_ex_i64(
            left, left.numel(), self.rowptr, self.cols, self.n_left, self.n_right, int(seed), int(n_cand), prob, idx, U, ld_u, I, ld_i,
            D, neg, cand, score, _lib.stream_ptr()), "sample_negative_ex")
        return (neg, cand, score) if return_candidates else neg

    @staticmethod
    def _table(t, n_rows, name):
        """A scoring table for the kernel -> (tensor, row stride in floats): a float32 GPU matrix with unit column stride
        and exactly n_rows rows; the kernel itself checks width, stride and alignment."""
        if t is None:
            raise _lib.TagrecError(f"sample: n_cand > 1 needs {name}")
        if isinstance(t, torch.Tensor) and t.dim() == 2 and t.shape[0] >= 1 and t.stride(1) == 1:
            _lib.require_gpu_tensor(t[0], torch.float32, f"sample: {name}")      # (a row view is itself not contiguous)
        else:
            t = _lib.require_gpu_tensor(t, torch.float32, f"sample: {name}")
        if t.dim() != 2 or t.shape[0] != n_rows:
            raise _lib.TagrecError(f"sample: {name} must be [{n_rows}, D], got {list(t.shape)}")
        return t, (t.stride(0) if t.shape[0] > 1 else t.shape[1])

    def popularity_alias(self, alpha):
        """Alias table (device tensors) of the proposal w_i = deg_i ** alpha, deg_i = distinct left ids of right id i.
        Ids nobody holds get weight 0.  A left id whose positives are the whole support could never be given a
        negative: refused."""
        deg = torch.bincount(self.cols.long(), minlength=self.n_right).cpu().numpy().astype(np.float64)
        w = np.where(deg > 0, np.power(np.maximum(deg, 1.0), float(alpha)), 0.0)
        prob, idx = alias_table(w)
        support = int(np.count_nonzero(w > 0))
        longest = int((self.rowptr[1:] - self.rowptr[:-1]).max()) if self.n_left else 0
        if longest >= support:
            raise _lib.TagrecError(f"neg_sampling='popularity': a left id holds all {support} ids of non-zero weight, "
                                   "no negative can be drawn for it")
        dev = self.cols.device
        return torch.from_numpy(prob).to(dev), torch.from_numpy(idx).to(dev)


def _sampler_keys(cfg, pos):
    """(alias table or None, number of candidates) of a producer, from the config's sampler keys."""
    mode, alpha, n_cand = check_neg_sampling(cfg)
    return (pos.popularity_alias(alpha) if mode == "popularity" else None), n_cand


class BPR_training_data(Abstract_training_data):
    """config["n_negatives"] = K negatives per train edge (default one: [E, 3] triplets; else [E, 2 + K] tuples), re-drawn
    and shuffled every epoch; config["negatives"] = "in_batch", config["softmax_over"] = "catalogue" or
    config["pair_batches"] = True: [E, 2] pairs, nothing is drawn, the shuffle is the same.
    With config["neg_candidates"] > 1 the epoch's
    negatives are scored by `model` (given here or through `attach_model`): one eval-mode, no-grad `model.forward()` per
    epoch supplies the user and item tables `predict_rating` scores with."""

    def __init__(self, data, args=None, config=None, seed=None, model=None):
        super().__init__(args, config)
        cfg = config if config is not None else _GLOBAL_CFG
        self.num = data.num["item"]
        self.num_user = data.num["user"]
        pos = data.edge_index["train"]
        self.pos_inter = (pos if isinstance(pos, torch.Tensor) else torch.from_numpy(np.asarray(pos))).to(
            self.device, torch.int64)
        self._pos = _Positives(self.pos_inter[:, 0], self.pos_inter[:, 1], self.num_user, self.num)
        self._alias, self._n_cand = _sampler_keys(cfg, self._pos)
        self._n_neg = check_ranking(cfg)[0]          # K negatives per edge: the epoch array is [E, 2 + K]
        # negatives="in_batch": the epoch array is [E, 2], the sampler is not launched (so no model is needed either)
        # pair_batches=True (DirectAU: an objective without negatives) takes the same branch
        pair = cfg.get("pair_batches", False)
        if not isinstance(pair, bool):
            raise _lib.TagrecError(f"pair_batches must be True or False, got {pair!r}")
        # softmax_over="catalogue" (every item is a column: nothing to draw) takes it too
        self._in_batch = check_negatives(cfg)[0] or pair or check_softmax_over(cfg)
        self._model = model
        self._seed = int(cfg["seed"] if seed is None else seed)
        self._epoch = 0
        self._gen = torch.Generator(device=self.device)
        self._gen.manual_seed(self._seed)
        self.tot_inter = self.pos_inter.shape[0] // self.batch_size
        # hard negatives need the model: without one the first epoch waits for attach_model() + reset()
        if self._n_cand == 1 or model is not None or self._in_batch:
            self.all_train_data = self.get_all_training_data()

    def attach_model(self, model):
        """The model whose tables score the candidates (neg_candidates > 1); takes effect at the next reset()."""
        self._model = model
        return self

    def _score_tables(self):
        """The propagated (user, item) tables of the attached model: eval mode, no gradient, training flag restored."""
        m = self._model
        if m is None:
            raise _lib.TagrecError("BPR_training_data: neg_candidates > 1 scores candidates with the model -- pass model= "
                                   "or call attach_model(model) before reset()")
        was_training = m.training
        m.eval()
        try:
            with torch.no_grad():
                out = m.forward()
        finally:
            m.train(was_training)
        tabs = out[:2] if isinstance(out, (tuple, list)) else ()
        if len(tabs) != 2 or not all(isinstance(t, torch.Tensor) and t.dim() == 2 for t in tabs) \
                or tabs[0].shape[0] != self.num_user or tabs[1].shape[0] != self.num or tabs[0].shape[1] != tabs[1].shape[1]:
            raise _lib.TagrecError(f"BPR_training_data: neg_candidates > 1 needs a model whose forward() returns the full "
                                   f"[{self.num_user}, D] and [{self.num}, D] tables ({type(m).__name__} does not; sharded "
                                   "models are not covered) -- see model= / attach_model")
        return tabs

    def negatives(self, epoch):
        """The epoch's negatives [E, K] in edge order (before the shuffle), a pure function of (seed, epoch) and, with
        neg_candidates > 1, of the attached model.  Column j is an independent rejection-tested draw per edge on its own
        counter stream derived from (epoch seed, j); column 0 is the stream of n_negatives = 1."""
        u = self.pos_inter[:, 0].contiguous()
        seed = (self._seed << 20) + int(epoch)                           # a fresh stream every epoch
        ut, it = self._score_tables() if self._n_cand != 1 else (None, None)
        cols = []
        for j in range(self._n_neg):
            sj = (seed + j * 0x9E3779B97F4A7C15) & 0xFFFFFFFFFFFFFFFF    # j = 0: the epoch seed itself
            if self._n_cand == 1:
                cols.append(self._pos.sample(u, sj, alias=self._alias))
            else:
                cols.append(self._pos.sample(u, sj, n_cand=self._n_cand, alias=self._alias, user_table=ut, item_table=it))
        return torch.stack(cols, dim=1)

    def get_all_training_data(self):
        if self._in_batch:                               # the shuffle draws from the same generator as the sampled producer
            data = self.pos_inter[:, :2]
        else:
            data = torch.cat([self.pos_inter[:, :2], self.negatives(self._epoch)], dim=1)
        self._epoch += 1
        perm = torch.randperm(data.shape[0], device=self.device, generator=self._gen)
        return data[perm].contiguous()


class DGCF_training_data(Abstract_training_data):
    """The per-batch sampler DGCF / DisenGCN train with (train_data/bpr_training_data.py:47-83, utils.py:58-80):
    every mini-batch draws `train_batch` users (without replacement when there are more users than that), one of
    the user's train items and one rejected-negative item, plus `cor_batch` random ids per node type (the unused
    `cor` half).  E // B + 1 batches per epoch; `reset()` does nothing.  Drawn on the device; statistical parity
    only (the reference draws from Python's and numpy's global generators)."""

    def __init__(self, data, args=None, config=None, seed=None):
        super().__init__(args, config)
        cfg = config if config is not None else _GLOBAL_CFG
        _lib.refuse_multi_negative(cfg, "DGCF_training_data")
        self.cor_batch = cfg.get("cor_batch", 100)
        self.use_tag = cfg["use_tag"]
        self.num_item, self.num_user, self.num_tag = data.num["item"], data.num["user"], data.num.get("tag", 0)
        pos = data.edge_index["train"]
        pos = (pos if isinstance(pos, torch.Tensor) else torch.from_numpy(np.asarray(pos))).to(self.device, torch.int64)
        self._pos = _Positives(pos[:, 0], pos[:, 1], self.num_user, self.num_item)
        self._alias, n_cand = _sampler_keys(cfg, self._pos)
        if n_cand != 1:
            raise _lib.TagrecError("DGCF_training_data: neg_candidates > 1 is not covered (it would cost a propagation per "
                                   "mini-batch); the per-epoch producer BPR_training_data has it")
        deg = self._pos.rowptr[1:] - self._pos.rowptr[:-1]
        self._users = torch.nonzero(deg > 0).flatten()                 # keys of user_items['train']
        self.tot_inter = pos.shape[0] // self.batch_size + 1
        self._seed = int(cfg["seed"] if seed is None else seed)
        self._draws = 0
        self._gen = torch.Generator(device=self.device)
        self._gen.manual_seed(self._seed)

    def mini_sample(self):
        B, nu = self.batch_size, self._users.numel()
        if nu > B:
            pick = torch.randperm(nu, device=self.device, generator=self._gen)[:B]
        else:
            pick = torch.randint(0, nu, (B,), device=self.device, generator=self._gen)
        u = self._users[pick]
        lo, hi = self._pos.rowptr[u], self._pos.rowptr[u + 1]
        r = torch.rand(B, device=self.device, generator=self._gen)
        at = torch.minimum(lo + (r * (hi - lo)).long(), hi - 1)
        pos_i = self._pos.cols[at].long()
        neg_i = self._pos.sample(u, (self._seed << 20) + self._draws, alias=self._alias)
        self._draws += 1
        cor = [torch.randperm(n, device=self.device, generator=self._gen)[:self.cor_batch]
               for n in ([self.num_user, self.num_item] + ([self.num_tag] if self.use_tag else []))]
        k = min(c.numel() for c in cor)
        return torch.stack([u, pos_i, neg_i], dim=1), torch.stack([c[:k] for c in cor])

    def reset(self):
        pass

    def mini_batch(self):
        for _ in range(self.tot_inter):
            yield self.mini_sample()


class KGAT_training_data(Abstract_training_data):
    """TransE-phase producer of KGAT (train_data/transe_training_data.py:12-41): all (head, relation, tail) triplets of
    `data.create_edge()` in relation order; batch i is the window `all_triplet[i : i + transe_batch]` -- consecutive
    windows overlap in all but one row, as the reference's loop is written (:37-38) -- with one uniform negative
    tail per row, rejected while (head, relation, tail) is a known triplet.  `reset()` does nothing."""

    def __init__(self, data, args=None, config=None, seed=None):
        super().__init__(args, config)
        cfg = config if config is not None else _GLOBAL_CFG
        self.batch_size = cfg["transe_batch"]
        self.num = data.num["user"] + data.num["item"] + data.num["tag"]
        parts = []
        for k, e in data.create_edge().items():
            e = torch.as_tensor(np.asarray(e), dtype=torch.int64)      # [2, E] (TGCN_load.create_edge); rows: head, tail
            parts.append(torch.stack([e[0], torch.full_like(e[0], int(k)), e[1]], dim=1))
        self.all_triplet = torch.cat(parts).to(self.device)
        n_rel = int(self.all_triplet[:, 1].max()) + 1 if self.all_triplet.numel() else 1
        self._n_rel = n_rel
        self._pos = _Positives(self.all_triplet[:, 0] * n_rel + self.all_triplet[:, 1], self.all_triplet[:, 2], self.num * n_rel,
                               self.num)
        self.tot_inter = self.all_triplet.shape[0] // self.batch_size
        self._seed = int(cfg["seed"] if seed is None else seed) + 2
        self._draws = 0

    def reset(self):
        pass

    def mini_batch(self):
        for i in range(self.tot_inter):
            batch = self.all_triplet[i:i + self.batch_size]
            left = (batch[:, 0] * self._n_rel + batch[:, 1]).contiguous()
            neg = self._pos.sample(left, (self._seed << 20) + self._draws)
            self._draws += 1
            yield torch.cat([batch, neg[:, None]], dim=1)


class Fixed_training_data(Abstract_training_data):
    """Replays given per-epoch triplet arrays (parity runs against the CPU oracle)."""

    def __init__(self, epochs, batch_size, device):
        self.device = torch.device(device)
        self.batch_size = batch_size
        self._epochs = [torch.as_tensor(e, dtype=torch.int64).to(self.device) for e in epochs]
        self._next = 0
        self.all_train_data = self._epochs[0]

    def get_all_training_data(self):
        out = self._epochs[self._next % len(self._epochs)]
        self._next += 1
        return out


class TransTag_training_data(Abstract_training_data):
    """(user, tag, pos_item, neg_item) rows: one negative item per (u, i, t) assignment, rejected
    while (u, t, item) is an assignment (transe_training_data.py:42-70, utils.py:31-40).  Not
    shuffled, re-sampled on every reset() (the reference inherits `reset`)."""

    def __init__(self, data, args=None, config=None, seed=None):
        super().__init__(args, config)
        cfg = config if config is not None else _GLOBAL_CFG
        self.batch_size = cfg["transtag_batch"]
        self.num = data.num["item"]
        n_tag = data.num["tag"]
        uit = data.uit_data if isinstance(data.uit_data, torch.Tensor) else torch.from_numpy(np.asarray(data.uit_data))
        uit = uit.to(self.device, torch.int64)
        self.uti = uit[:, [0, 2, 1]].contiguous()
        # positives of a (user, tag) pair = the items it was assigned to; pair ids are compacted so the CSR stays small
        pair = self.uti[:, 0] * n_tag + self.uti[:, 1]
        upair, self._left = torch.unique(pair, return_inverse=True)
        self._pos = _Positives(self._left, self.uti[:, 2], upair.numel(), self.num)
        self._seed = int(cfg["seed"] if seed is None else seed) + 1
        self._epoch = 0
        self.all_train_data = self.get_all_training_data()
        self.tot_inter = self.all_train_data.shape[0] // self.batch_size

    def get_all_training_data(self):
        neg = self._pos.sample(self._left, (self._seed << 20) + self._epoch)
        self._epoch += 1
        return torch.cat([self.uti, neg[:, None]], dim=1).contiguous()
