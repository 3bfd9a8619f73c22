"""The training step surface of /root/reference/training/basic_train.py, plus the
fused Adam that replaces `torch.optim.Adam` (com.py:14,25,69).

    epoch_training(training_data, loss_func, opt) -> list[float]      basic_train.py:10-30
    GraphedStep / epoch_training(..., graphs={})                       the same step replayed as one HIP graph
    Basic_train(train_data, loss_func, opt, test, args).run(model)    basic_train.py:50-85
    Early_stop                                                         training/early_stop.py:8-41
    Adam(params, lr)   zero_grad()/step()                              torch.optim.Adam defaults
"""
import gc
import os
import time

import numpy as np
import torch

from . import _lib
from .config import CFG as _GLOBAL_CFG


class Adam:
    """torch.optim.Adam (betas (0.9, 0.999), eps 1e-8, no weight decay, no amsgrad) as one fused
    HIP pass per parameter tensor.  Same zero_grad()/step() protocol, so it drops into
    `epoch_training` where the reference passes a torch optimizer."""

    MULTI_MAX_NUMEL = 1 << 22         # tensors up to this size share one launch (tagrec_adam_multi_f32); 0: one launch each

    def __init__(self, params, lr=1e-3, betas=(0.9, 0.999), eps=1e-8, capturable=False):
        """capturable=True keeps every parameter's step counter in device memory and advances it inside the
        update (tagrec_adam_graph_f32), so `step()` can be captured in a HIP graph and replayed (`GraphedStep`)."""
        self.params = [p for p in params]
        if not self.params:
            raise ValueError("Adam: empty parameter list")
        self.lr, self.betas, self.eps = float(lr), (float(betas[0]), float(betas[1])), float(eps)
        self.state = {}
        self.step_count = 0
        self.capturable = bool(capturable)
        self._fused_done = set()          # parameters whose update of the current step was applied inside backward()
        for p in self.params:             # the newest optimizer built over a parameter owns it: a fusion set up by an
            p._tagrec_owner = self        # earlier one is revoked (`fused_optimizer`), the model hands out gradients again

    def fuse_into(self, model):
        """Let `model` apply this optimizer's update of its embedding table inside the last kernel of its backward pass
        (the gradient row is consumed where it is formed: no gradient tensor, no separate Adam launch over the table).
        LightGCN / NGCF: `model.table`, in the epilogue of the last backward product; TGCN: the three node tables
        (`model.fused_tables()`), in the epilogue of the bottom layer's dQ W_2^T product of the BPR phase -- the TransTag
        phase and every other path hand out gradients as usual.
        The zero_grad() / backward() / step() protocol of basic_train.py:19-25 is unchanged: step() then only counts
        the step for that parameter.  One backward() per step().  With capturable=True (models that declare
        `fused_capturable`: LightGCN, NGCF) the step counter and the step-dependent factors live in device memory and
        are advanced inside the fused launch, so the whole step can be captured as a HIP graph (`GraphedStep`).  Models
        without the hook ignore the call.

        CONTRACT: with the fusion on, a training-mode backward() of `model.loss` CHANGES the table (and exp_avg /
        exp_avg_sq) -- also one that is not followed by step() (gradient inspection, clipping); a second such
        backward() before step() raises.  Use an un-fused optimizer for anything but the plain loop."""
        if self.capturable and not getattr(model, "fused_capturable", False):
            raise _lib.TagrecError("Adam.fuse_into: this model's fused update keeps its step counter on the host (capturable=False)")
        if hasattr(model, "set_fused_optimizer"):
            for table in _fused_tables(model):
                if not any(q is table for q in self.params):
                    raise _lib.TagrecError("Adam.fuse_into: the model's table is not one of this optimizer's parameters")
            for table in _fused_tables(model):
                table._tagrec_owner = self
            model.set_fused_optimizer(self)
        return self

    def fused_state(self, p):
        """(m, v, step number of the update about to be applied) for a parameter updated inside backward().  The caller
        launches the update and then calls `fused_commit(p)`: a launch that fails leaves no sticky mark."""
        if id(p) in self._fused_done:
            raise _lib.TagrecError("Adam: a second backward() before step() with a fused update")
        st = self.state.get(id(p))
        if st is None:
            st = self.state[id(p)] = {"m": torch.zeros_like(p.data), "v": torch.zeros_like(p.data), "t": 0}
            if self.capturable:
                st["t_dev"] = torch.zeros(1, dtype=torch.int64, device=p.device)
                st["coef"] = torch.zeros(2, dtype=torch.float32, device=p.device)
        return st["m"], st["v"], st["t"] + 1

    def fused_dev(self, p):
        """(device step counter, device factors) of a capturable optimizer's parameter, else None."""
        st = self.state.get(id(p))
        return (st["t_dev"], st["coef"]) if (self.capturable and st is not None) else None

    def fused_commit(self, p):
        """The fused update of `p` has been launched: step() only counts the step for it."""
        self._fused_done.add(id(p))

    def zero_grad(self, set_to_none=True):
        for p in self.params:
            if p.grad is not None:
                if set_to_none:
                    p.grad = None
                else:
                    p.grad.zero_()

    @torch.no_grad()
    def step(self):
        lib = _lib.load()
        self.step_count += 1
        small = {}                                        # step count -> [(p, g, m, v)] of the tensors updated in one launch
        for p in self.params:
            if id(p) in self._fused_done:             # updated inside backward(): only the step counter moves here
                self._fused_done.discard(id(p))
                self.state[id(p)]["t"] += 1
                if p.grad is None:
                    continue
                raise _lib.TagrecError("Adam: parameter with a fused update also received a gradient tensor")
            if p.grad is None:
                continue
            _lib.require_gpu_tensor(p.data, torch.float32, "Adam parameter")
            g = p.grad if p.grad.is_contiguous() else p.grad.contiguous()
            st = self.state.get(id(p))
            if st is None:
                st = self.state[id(p)] = {"m": torch.zeros_like(p.data), "v": torch.zeros_like(p.data), "t": 0}
                if self.capturable:
                    st["t_dev"] = torch.zeros(1, dtype=torch.int64, device=p.device)
                    st["coef"] = torch.zeros(2, dtype=torch.float32, device=p.device)
            st["t"] += 1
            if not self.capturable and p.numel() <= self.MULTI_MAX_NUMEL:
                small.setdefault(st["t"], []).append((p.data, g, st["m"], st["v"]))       # one launch for all of them, below
                continue
            if self.capturable:
                _lib.check(lib.tagrec_adam_graph_f32(p.data, g, st["m"], st["v"], p.numel(), self.lr, self.betas[0], self.betas[1],
                                                     self.eps, st["t_dev"], st["coef"], _lib.stream_ptr()), "adam_graph")
            else:
                _lib.check(lib.tagrec_adam_f32(p.data, g, st["m"], st["v"], p.numel(), self.lr, self.betas[0], self.betas[1],
                                               self.eps, st["t"], _lib.stream_ptr()), "adam")
        # the small tensors (a TGCN layer has 21): launches of up to 64 tensors each instead of a burst of tiny launches, during
        # which the GPU caught up with the host at the end of every step
        for t, group in small.items():
            k = len(group)
            if k < 3:                                     # a model with one or two tensors: the plain launch is cheaper to set up
                for pd, g_, m_, v_ in group:
                    _lib.check(lib.tagrec_adam_f32(pd, g_, m_, v_, pd.numel(), self.lr, self.betas[0], self.betas[1], self.eps, t,
                                                   _lib.stream_ptr()), "adam")
                continue
            arr = [(_lib.ctypes.c_void_p * k)(*[x[i].data_ptr() for x in group]) for i in range(4)]
            n = (_lib.ctypes.c_int64 * k)(*[x[0].numel() for x in group])
            _lib.check(lib.tagrec_adam_multi_f32(k, arr[0], arr[1], arr[2], arr[3], n, self.lr, self.betas[0], self.betas[1], self.eps,
                                                 t, _lib.stream_ptr()), "adam_multi")

    def prepare_state(self):
        """Allocate every parameter's state now (graph capture must not meet a first-use allocation whose zero fill
        would be replayed)."""
        for p in self.params:
            if id(p) not in self.state:
                st = self.state[id(p)] = {"m": torch.zeros_like(p.data), "v": torch.zeros_like(p.data), "t": 0}
                if self.capturable:
                    st["t_dev"] = torch.zeros(1, dtype=torch.int64, device=p.device)
                    st["coef"] = torch.zeros(2, dtype=torch.float32, device=p.device)


class RowAdam(Adam):
    """`Adam` whose step on an attached embedding table touches only the rows the batch names -- and still computes what
    `Adam` computes, bit for bit.  (`torch.optim.SparseAdam` skips the rows without a gradient; dense Adam does not: their
    m and v decay and p moves along the old m.)  That move is a function of the row's own state and of two per-step
    scalars, so an unnamed row is left alone and the steps it missed are replayed, in order, the next time something reads
    it (csrc/rowadam.hip).  No table-sized gradient exists and no pass over the table runs, except the flush below.

        opt = T.RowAdam(model.parameters(), lr=1e-3).attach(model)      # UltraGCN: the one model whose gradient is row-sparse
        zero_grad() / loss.backward() / step()                          # as before

    A training-mode `model.loss()` catches the batch's rows up, its backward hands (plan, compact gradient) to this
    optimizer and leaves `table.grad` None, `step()` applies them.  No row is ever more than `max_lag` steps behind: every
    max_lag steps `step()` runs `flush()`, which brings the whole table to the current step.  The model flushes before
    anything else reads the table (forward, predict_rating, get_ego_embed, state_dict, eval()).  A caller who reads
    `model.table.data` directly between steps sees LAGGING rows: call `opt.flush()` first.

    A dense `p.grad` on an attached table (an eval-mode loss, any other graph onto it) is served as `Adam` serves it, after
    a flush.  Parameters that are not attached behave as in `Adam`.  lr, betas and eps are fixed at construction (the
    per-step factors are filled ahead); the step number lives on the host, so capturable=True -- and with it
    `GraphedStep` -- is refused."""

    FILL = 1024                       # steps of the coefficient ring filled per host call, ahead of their use

    def __init__(self, params, lr=1e-3, betas=(0.9, 0.999), eps=1e-8, max_lag=1024, capturable=False):
        if capturable:
            raise _lib.TagrecError("RowAdam: capturable=True is not covered -- the step number of the lazy rows lives on the host")
        from . import rowops
        if not 1 <= int(max_lag) <= rowops.ADAM_MAX_WINDOW:
            raise _lib.TagrecError(f"RowAdam: max_lag={max_lag!r} must be 1 .. {rowops.ADAM_MAX_WINDOW}")
        super().__init__(params, lr, betas, eps, False)
        self.max_lag = int(max_lag)
        self._rows = {}                   # id(p) -> the lazy state of an attached table
        self._frozen = True

    def __setattr__(self, name, value):
        if name in ("lr", "betas", "eps", "max_lag") and getattr(self, "_frozen", False):
            raise _lib.TagrecError(f"RowAdam: {name} is fixed after construction (the ring of per-step factors is filled ahead); "
                                   "build a new optimizer")
        super().__setattr__(name, value)

    # tagrec_adam_f32 takes lr / b1 / b2 as floats and widens them: the ring is computed from the same values
    def _f32(self, x):
        return _lib.ctypes.c_float(x).value

    def attach(self, model):
        """Make `model`'s training step row-sparse under this optimizer (`model.set_row_optimizer`).  Only a model whose
        step names the rows it changes has the hook: UltraGCN."""
        if not hasattr(model, "set_row_optimizer"):
            raise _lib.TagrecError(f"RowAdam.attach: {type(model).__name__} is not covered -- its gradients are dense (propagation "
                                   "spreads every batch row's gradient over the table); only UltraGCN's step names its rows")
        table = model.table
        if not any(q is table for q in self.params):
            raise _lib.TagrecError("RowAdam.attach: the model's table is not one of this optimizer's parameters")
        _lib.require_gpu_tensor(table.data, torch.float32, "RowAdam.attach: the table")
        if id(table) not in self._rows:
            st = self.state.get(id(table))
            if st is None:
                st = self.state[id(table)] = {"m": torch.zeros_like(table.data), "v": torch.zeros_like(table.data), "t": 0}
            cap = self.FILL * ((self.max_lag + 1 + 2 * self.FILL - 1) // self.FILL)        # >= max_lag + 1 + one block ahead
            self._rows[id(table)] = {"p": table, "last": torch.full((table.shape[0],), st["t"], dtype=torch.int32, device=table.device),
                                     "ring": torch.zeros(cap, 2, dtype=torch.float32, device=table.device), "filled": st["t"],
                                     "flushed": st["t"], "pending": None}
            self._fill(self._rows[id(table)], st["t"] + 1)
        table._tagrec_owner = self
        model.set_row_optimizer(self)
        return self

    def _fill(self, rs, t):
        """The ring holds the factors of every step up to t: filled a block ahead, FILL-aligned so that a block never wraps.
        One host-to-device copy per block, none per step."""
        from . import rowops
        cap = rs["ring"].shape[0]
        while rs["filled"] < t:
            t0 = rs["filled"] + 1
            n = self.FILL - t0 % self.FILL                      # up to the next multiple of FILL (exclusive)
            coef = rowops.adam_coef(self._f32(self.lr), self._f32(self.betas[0]), self._f32(self.betas[1]), t0, n)
            rs["ring"][t0 % cap:t0 % cap + n].copy_(coef)
            rs["filled"] = t0 + n - 1

    def lagging_rows(self, p):
        """Number of rows of the attached table `p` that are behind the optimizer's step -- reads the device (tests, tools)."""
        rs = self._rows[id(p)]
        return int((rs["last"] < self.state[id(p)]["t"]).sum())

    def row_state(self, p):
        """(m, v, last, step) of an attached table."""
        st = self.state[id(p)]
        return st["m"], st["v"], self._rows[id(p)]["last"], st["t"]

    def catch_up(self, p, plan):
        """Bring the rows of `plan` to the steps done so far (the forward pass of the model's loss, before it gathers them)."""
        from . import rowops
        rs, st = self._rows[id(p)], self.state[id(p)]
        rowops.adam_catch_up(plan, p.data, st["m"], st["v"], rs["last"], rs["ring"], rs["flushed"], st["t"], self.betas, self.eps)

    def row_grad(self, p, plan, grad):
        """The model's backward: the compact gradient of `plan`'s rows, applied by the next step()."""
        rs = self._rows[id(p)]
        if rs["pending"] is not None:
            raise _lib.TagrecError("RowAdam: a second backward() before step() on a row-sparse step")
        rs["pending"] = (plan, grad)

    def zero_grad(self, set_to_none=True):
        super().zero_grad(set_to_none)
        for rs in self._rows.values():       # a gradient that was never stepped on is dropped, as p.grad would be
            rs["pending"] = None

    @torch.no_grad()
    def flush(self):
        """Bring every row of every attached table to the optimizer's step.  Idempotent; one pass over `last`, and over
        the rows that lag."""
        from . import rowops
        for rs in self._rows.values():
            st = self.state[id(rs["p"])]
            if rs["flushed"] < st["t"]:
                rowops.adam_flush(rs["p"].data, st["m"], st["v"], rs["last"], rs["ring"], rs["flushed"], st["t"], self.betas, self.eps)
                rs["flushed"] = st["t"]

    @torch.no_grad()
    def step(self):
        from . import rowops
        dense, lazy = [], []
        for rs in self._rows.values():
            p, st = rs["p"], self.state[id(rs["p"])]
            if rs["pending"] is not None:
                if p.grad is not None:
                    raise _lib.TagrecError("RowAdam: the table received a row-sparse gradient and a gradient tensor in one step")
                lazy.append((rs, st))
            elif p.grad is not None:             # a dense gradient: Adam's own pass over a table that is current
                dense.append((rs, st))
        if dense:
            self.flush()
        for rs, st in lazy:
            plan, grad = rs["pending"]
            self._fill(rs, st["t"] + 1)
            rowops.adam_apply_rows(plan, grad, rs["p"].data, st["m"], st["v"], rs["last"], rs["ring"], st["t"] + 1, self.betas, self.eps)
            rs["pending"] = None
            st["t"] += 1
        super().step()                           # every parameter with a gradient tensor, the dense tables among them
        for rs, st in dense:
            rs["last"].fill_(st["t"])
            rs["flushed"] = st["t"]
            self._fill(rs, st["t"] + 1)
        for rs, st in lazy:
            if st["t"] - rs["flushed"] >= self.max_lag:
                self.flush()
            self._fill(rs, st["t"] + 1)


def row_optimizer(model):
    """The `RowAdam` attached to `model` (`RowAdam.attach`), or None.  Live only while it is still the newest optimizer built
    over the table: one created later revokes it -- the table is flushed first, so that the new owner starts from the dense
    optimizer's state."""
    opt = getattr(model, "_row_opt", None)
    if opt is None:
        return None
    if getattr(model.table, "_tagrec_owner", None) is not opt:
        opt.flush()
        model._row_opt = None
        return None
    return opt


def _fused_tables(model):
    """The parameters a model can update inside its own backward pass: `model.fused_tables()` (TGCN: the three node
    tables) or the single `model.table`."""
    if hasattr(model, "fused_tables"):
        return list(model.fused_tables())
    table = getattr(model, "table", None)
    return [] if table is None else [table]


def fused_optimizer(model):
    """The optimizer whose update of `model.table` runs inside the model's backward pass (`Adam.fuse_into`), or None:
    the fusion is live only while that optimizer is still the newest one built over the table -- a second optimizer
    created for the same model (new run, new lr) revokes it instead of leaving the old one updating behind its back."""
    opt = getattr(model, "_fused_opt", None)
    if opt is None:
        return None
    tables = _fused_tables(model)
    if not tables or any(getattr(t, "_tagrec_owner", None) is not opt for t in tables):
        model._fused_opt = None
        return None
    return opt


def _step(loss_func, opt, data):
    lossx = loss_func(data)
    parts = torch.stack([x.detach() for x in lossx])
    loss = sum(lossx)
    if isinstance(opt, list):
        [op.zero_grad() for op in opt]
        loss.backward()
        [op.step() for op in opt]
    else:
        opt.zero_grad()
        loss.backward()
        opt.step()
    return parts


class GraphedStep:
    """One training step -- loss parts, backward, optimizer -- captured once as a HIP graph and replayed per batch.
    At the reference's dataset sizes (HetRec / ml-100k: ~1e5 edges) a step is a few dozen to a few hundred small
    launches and the GPU idles between them; replaying the captured graph removes the per-launch host cost.
    The optimizer must advance its step counter on the device (`Adam(capturable=True)`), the batch shape is fixed,
    and the step must not synchronise with the host (the fused model paths do not)."""

    def __init__(self, loss_func, opt, batch):
        opts = opt if isinstance(opt, list) else [opt]
        for op in opts:
            if not getattr(op, "capturable", False):
                raise _lib.TagrecError("GraphedStep: the optimizer must be Adam(capturable=True)")
            op.prepare_state()
        self.static_batch = batch.clone()
        self.graph = torch.cuda.CUDAGraph()
        self._opts = opts
        before = [op.step_count for op in opts]
        [op.zero_grad() for op in opts]
        # No destructor may free device memory inside the capture (`Graph.__del__` ends in hipFree, which invalidates it), and
        # torch no longer collects before one: collect what is dead now and keep the cycle collector off until the capture ends.
        gc.collect()
        gc_was_on = gc.isenabled()
        gc.disable()
        try:
            with torch.cuda.graph(self.graph):
                self.static_parts = _step(loss_func, opt, self.static_batch)
        finally:
            if gc_was_on:
                gc.enable()
        for op, b in zip(opts, before):          # capturing executed nothing: the host-side counters follow the replays
            op.step_count = b

    def __call__(self, batch):
        self.static_batch.copy_(batch)
        self.graph.replay()
        for op in self._opts:
            op.step_count += 1
        return self.static_parts.clone()


def _graph_key(loss_func, data):
    owner = getattr(loss_func, "__self__", None)
    return (id(owner), getattr(loss_func, "__name__", id(loss_func)), tuple(data.shape), data.dtype)


def epoch_training(training_data, loss_func, opt, verbose=True, graphs=None):
    """One pass over `training_data.mini_batch()` (basic_train.py:10-30): per batch the loss parts,
    their sum, zero_grad / backward / step.  Returns the per-batch totals as floats.
    The reference synchronises twice per step to read the losses (:16,27); here the parts stay on
    the device and are read back once at the end of the epoch -- same numbers, one sync.

    graphs: a dict kept by the caller across epochs.  When given, the first two batches of every (loss function,
    batch shape) run as usual -- they also grow every lazily sized buffer -- the third is captured as a HIP graph
    (`GraphedStep`) and from then on batches of that shape are graph replays; other shapes (the merged tail
    batch) and batches that are not plain tensors run as usual.  If a step cannot be captured it keeps running
    eagerly and the reason is recorded under graphs["errors"]."""
    parts_dev = []
    training_data.reset()
    for data in training_data.mini_batch():
        if graphs is not None and isinstance(data, torch.Tensor) and data.is_cuda:
            key = _graph_key(loss_func, data)
            entry = graphs.get(key, 0)
            if isinstance(entry, GraphedStep):
                parts_dev.append(entry(data))
                continue
            if entry == 2:
                try:
                    graphs[key] = GraphedStep(loss_func, opt, data)
                    parts_dev.append(graphs[key](data))
                    continue
                except Exception as exc:                 # not capturable: stay eager for this key
                    graphs[key] = -1
                    graphs.setdefault("errors", []).append(f"{key}: {type(exc).__name__}: {exc}")
                    torch.cuda.synchronize()
            elif entry >= 0:
                graphs[key] = entry + 1
        parts_dev.append(_step(loss_func, opt, data))
    if not parts_dev:
        return []
    parts = torch.stack(parts_dev).cpu().numpy()
    if verbose:
        print(f"[avg_loss of each part]:{list(parts.sum(0))}")
    # float32 sum of the parts, as `sum(lossx)` computes it on the device
    return [float(np.float32(sum(np.float32(v) for v in row))) for row in parts]


class Early_stop:
    """training/early_stop.py:8-41: track the best `key` metric (first entry of a list metric),
    save `state_dict` on improvement, stop after `patient_epoch` non-improving evaluations."""

    def __init__(self, args=None, config=None):
        cfg = config if config is not None else _GLOBAL_CFG
        self.best_value = None
        self.count_step = 0
        self.best_result = None
        self.best_epoch = 0
        self.patient_step = cfg["patient_epoch"]
        out_dir = getattr(args, "out_dir", None)
        self.save_path = f"{out_dir}/model.pth.tar" if out_dir else None
        self.key = cfg["early_stop_key"]
        self.higher = self.key in ("precision", "recall", "ndcg")

    def __call__(self, model, cur_results, epoch):
        cur = cur_results[self.key]
        cur = cur[0] if isinstance(cur, (list, tuple, np.ndarray)) else cur
        better = self.best_value is None or (cur > self.best_value if self.higher else cur < self.best_value)
        if better:
            self.best_value, self.count_step = cur, 0
            if self.save_path:
                os.makedirs(os.path.dirname(self.save_path), exist_ok=True)
                torch.save(model.state_dict(), self.save_path)
            self.best_result, self.best_epoch = cur_results, epoch
        else:
            self.count_step += 1
        return self.count_step > self.patient_step


class Basic_train:
    """basic_train.py:50-85: epochs x phases (phase i = train_data[i], loss_func[i], opt[i]),
    evaluation every `test_interval` epochs, early stop."""

    def __init__(self, train_data, loss_func, opt, test, args=None, config=None):
        self.cfg = config if config is not None else _GLOBAL_CFG
        self.train_sphase = len(train_data)
        self.train_data, self.loss_func, self.opt, self.test, self.args = train_data, loss_func, opt, test, args
        self.early_stop = Early_stop(args, self.cfg)
        # config["hip_graph"]: replay each phase's step as a captured HIP graph (needs Adam(capturable=True))
        self.graphs = {} if self.cfg.get("hip_graph", False) else None

    def run(self, model, verbose=True):
        history = []
        for ep in range(self.cfg["epochs"]):
            model.train()
            if hasattr(model, "begin_epoch"):      # per-epoch work outside the steps (NCL re-clusters its node tables)
                model.begin_epoch(ep)
            for i in range(self.train_sphase):
                start = time.time()
                loss_list = epoch_training(self.train_data[i], self.loss_func[i], self.opt[i], verbose=verbose, graphs=self.graphs)
                if verbose:
                    print(f"[Epoch:{ep}][Time:{(time.time() - start) / 60:.2}]:"
                          f"avg_loss_{i} :{sum(loss_list) / len(loss_list):.5}")
                history.append((ep, i, loss_list))
            if self.test is not None and ep % self.cfg["test_interval"] == 0:
                results = self.test.run(model)
                if verbose:
                    print(f"[Epoch {ep}] results: {results}")
                if self.early_stop(model, results, ep):
                    if verbose:
                        print(f"early stop trigger at epoch {ep}")
                    break
        return history
