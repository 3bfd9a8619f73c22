"""The loss stage of a LightGCN / NGCF step and of help.py's table losses: the one thing that varies between the objectives.

A stage is made per step (`help.stage_for(route, loss_kind)`, or directly by help.py's loss functions), runs one kernel pair of
rowops.py on GATHERED rows -- Ub [B, D] the batch's users, Ib [T - B, D] its items in slot order -- and keeps what its backward
needs (coef / lse / AuState) on itself:

    stage.rows(batch, n_user)              -> int64 node ids [T] of the [user | item] table, in the slot order of the kernels
    stage.ids(batch)                       -> (user ids [B], item ids [T - B]) of the same slots, for separate tables
    stage.check(name, batch)               refuses a batch of another shape in `name`'s words (the table losses)
    stage.fwd(batch, Ub, Ib, Ureg, Ireg)   -> res = [mul_loss, l2reg_loss (unweighted)]; Ureg / Ireg: the L2 rows, or None
    stage.bwd(Ub, Ib, Ureg, Ireg, g, dUb, dIb, dUreg, dIreg, what=None)
                                           the gradient rows of both parts (g = their upstream gradients); dUb = dIb = None: the
                                           L2 part only, Ureg = Ireg = None: no L2 part, dUreg is dUb: one buffer takes the sum
    stage.grads_zeroed                     True: the backward scatter-adds into caller-ZEROED rows; False: it STORES every row
    stage.reg_apart                        True: a step whose L2 rows are not its loss rows launches the backward once per part
    stage.extra                            None, or a device tensor the forward leaves to be appended to `res` (no gradient)

    stage.on_tables                        True: the stage has the second form below, and an all-rows step takes it
    stage.dense                            True: the stage reads EVERY item row, so it has the second form only -- its step is
                                           never compact and nothing of its forward pass may be row-masked

`Triplet` has a second form, `fwd_on_tables` / `bwd_on_tables`, for the all-rows step: its kernels take the real triplets and
gather from the full tables themselves, so that step has no gathered rows at all.  `Catalogue` has that form alone.
"""
import torch


from . import _lib, rowops


class _Stage:
    name = batch_word = None                 # the table loss of this stage in help.py and what it calls its batch
    grads_zeroed = reg_apart = on_tables = dense = False
    extra = None
    _ids = None

    def rows(self, batch, n_user):
        return rowops.tuple_rows(batch, n_user)

    def ids(self, batch):
        if self._ids is None:                # item j of tuple b at slot j B + b
            self._ids = (batch[:, 0].contiguous(), batch[:, 1:].t().contiguous().view(-1))
        return self._ids

    @staticmethod
    def _what(kernel, what):
        return () if what is None else (f"{kernel}({what})",)


class Triplet(_Stage):
    """[B, 3] = (user, positive, negative): `rowops.bpr_fwd` / `bpr_bwd` on `compact_triplets` of the gathered rows."""
    grads_zeroed = on_tables = True

    def __init__(self, loss_kind):
        self.loss_kind = loss_kind

    def rows(self, batch, n_user):
        return rowops.batch_rows(batch, n_user)

    def fwd(self, batch, Ub, Ib, Ureg, Ireg):
        self.trip = rowops.compact_triplets(batch.shape[0], batch.device)
        res, self.coef = rowops.bpr_fwd(Ub, Ib, Ureg, Ireg, self.trip, self.loss_kind)
        return res

    def bwd(self, Ub, Ib, Ureg, Ireg, g, dUb, dIb, dUreg, dIreg, what=None):
        rowops.bpr_bwd(Ub, Ib, Ureg, Ireg, self.trip, self.coef, g, dUb, dIb, dUreg, dIreg, *self._what("bpr_bwd", what))

    def fwd_on_tables(self, batch, out, ego, n_user, n_item):
        """The stage on the full [user | item] tables `out` (and `ego`: the L2 part's): the gather is the kernel's."""
        self.trip = batch
        self._cut = lambda t: (None, None) if t is None else (t[:n_user], t[n_user:n_user + n_item])
        res, self.coef = rowops.bpr_fwd(*self._cut(out), *self._cut(ego), batch, self.loss_kind)
        return res

    def bwd_on_tables(self, out, ego, g, d_out, d_ego, plan=None, what=None):
        """Scatter-adds into d_out / d_ego (ego None: no L2 part; d_out None: the L2 part only, added to what d_ego holds).
        plan (the `row_list_plan` of `rows`): `rowops.bpr_bwd_ordered`, no float atomics on repeated ids."""
        if plan is not None:
            rowops.bpr_bwd_ordered(out, ego, self.trip, self.coef, g, d_out, d_ego, plan, d_out is None,
                                   *self._what("bpr_bwd", what))
        else:
            rowops.bpr_bwd(*self._cut(out), *self._cut(ego), self.trip, self.coef, g, *self._cut(d_out), *self._cut(d_ego),
                           *self._what("bpr_bwd", what))


class Rank(_Stage):
    """[B, 2 + K] = (user, positive, K negatives): the multi-negative kernels `rowops.rank_fwd` / `rank_bwd`."""
    name, batch_word = "ranking_loss", "tuples"
    reg_apart = True         # (one launch that stores both parts would do; the steps have always launched two)

    def __init__(self, loss_kind, temperature):
        self.loss_kind, self.temperature = loss_kind, temperature

    def check(self, name, batch):
        if batch.dim() != 2 or batch.shape[1] < 3:
            raise _lib.TagrecError(f"{name}: tuples {tuple(batch.shape)} must be [B, 2 + K]")

    def fwd(self, batch, Ub, Ib, Ureg, Ireg):
        res, self.coef = rowops.rank_fwd(Ub, Ib, Ureg, Ireg, self.loss_kind, self.temperature)
        return res

    def bwd(self, Ub, Ib, Ureg, Ireg, g, dUb, dIb, dUreg, dIreg, what=None):
        rowops.rank_bwd(Ub, Ib, Ureg, Ireg, self.coef, g, dUb, dIb, dUreg, dIreg, *self._what("rank_bwd", what))


class Ultra(_Stage):
    """[B, 2 + K] = (user, positive, K negatives) under UltraGCN's weighted pointwise BCE (`rowops.wbce_fwd` / `wbce_bwd`):
    the M co-occurrence neighbours of the positive (`tables.nbr_id[positive]`) follow the negatives as slots K + 1 .. K + M.
    A pad (-1) is replaced by the positive's own id and weighs 0, so its gradient is an exact zero.  tables:
    `help.UltraTables`.  The [B, 1 + K + M] weights are gathered on the stream; nothing reads the host."""
    name, batch_word = "ultragcn_loss", "tuples"

    def __init__(self, tables):
        self.tables = tables
        self.M = 0 if tables.nbr_id is None else tables.nbr_id.shape[1]

    def check(self, name, batch):
        if batch.dim() != 2 or batch.shape[1] < 3 or batch.shape[0] < 1:
            raise _lib.TagrecError(f"{name}: tuples {tuple(batch.shape)} must be [B, 2 + K] = (user, positive, K >= 1 negatives)")
        if 1 + (batch.shape[1] - 2) + self.M > rowops.WBCE_MAX_SLOTS:
            raise _lib.TagrecError(f"{name}: {batch.shape[1] - 2} negatives and {self.M} neighbours exceed the "
                                   f"{rowops.WBCE_MAX_SLOTS} slots of a tuple")

    def rows(self, batch, n_user):
        uid, iid = self.ids(batch)
        return torch.cat([uid, n_user + iid])

    def ids(self, batch):
        if self._ids is None:
            t = self.tables
            uid, pos = batch[:, 0].contiguous(), batch[:, 1]
            items = batch[:, 1:]
            if self.M:
                nb = t.nbr_id.index_select(0, pos)                                   # [B, M] int64, -1 = pad
                items = torch.cat([items, torch.where(nb < 0, pos.unsqueeze(1), nb)], dim=1)
            self._ids = (uid, items.t().contiguous().view(-1))
        return self._ids

    def weights(self, batch):
        """[B, 1 + K + M]: positive w1 + w2 b_u b_i; negative (w3 + w4 b_u b_j) negative_weight / K; neighbour lambda omega."""
        t = self.tables
        uid, pos, neg = batch[:, 0], batch[:, 1], batch[:, 2:]
        w1, w2, w3, w4 = t.w
        bu = t.beta_u.index_select(0, uid).unsqueeze(1)
        parts = [w1 + w2 * bu * t.beta_i.index_select(0, pos).unsqueeze(1),
                 (w3 + w4 * bu * t.beta_i[neg]) * (t.negative_weight / neg.shape[1])]
        if self.M:
            parts.append(t.lam * t.nbr_w.index_select(0, pos))
        return torch.cat(parts, dim=1).contiguous()

    def fwd(self, batch, Ub, Ib, Ureg, Ireg):
        self.K = batch.shape[1] - 2
        res, self.coef = rowops.wbce_fwd(Ub, Ib, Ureg, Ireg, self.weights(batch), self.K, self.M)
        return res

    def bwd(self, Ub, Ib, Ureg, Ireg, g, dUb, dIb, dUreg, dIreg, what=None):
        rowops.wbce_bwd(Ub, Ib, Ureg, Ireg, self.coef, g, dUb, dIb, dUreg, dIreg, self.K, self.M, *self._what("wbce_bwd", what))


class InBatch(_Stage):
    """[B, 2] = (user, positive), the other positives are the negatives: the fused B x B kernels `rowops.inbatch_fwd` /
    `inbatch_bwd` with the batch's ids as masks and item_logq ([n_item], or None) as the column bias."""
    name, batch_word = "in_batch_loss", "pairs"

    def __init__(self, temperature, item_logq=None):
        self.temperature, self.item_logq = temperature, item_logq

    def check(self, name, batch):
        if batch.dim() != 2 or batch.shape[1] != 2:
            raise _lib.TagrecError(f"{name}: pairs {tuple(batch.shape)} must be [B, 2] = (user, positive)")

    def fwd(self, batch, Ub, Ib, Ureg, Ireg):
        uid, iid = self.ids(batch)
        self.bias = None if self.item_logq is None else self.item_logq.index_select(0, iid)
        res, self.lse = rowops.inbatch_fwd(Ub, Ib, Ureg, Ireg, self.temperature, uid, iid, self.bias)
        return res

    def bwd(self, Ub, Ib, Ureg, Ireg, g, dUb, dIb, dUreg, dIreg, what=None):
        rowops.inbatch_bwd(Ub, Ib, Ureg, Ireg, self.temperature, self.lse, g, dUb, dIb, dUreg, dIreg, *self._ids, self.bias,
                           *self._what("inbatch_bwd", what))


class Au(_Stage):
    """[B, 2] = (user, positive) under the alignment / uniformity loss: `rowops.directau_fwd` / `directau_bwd`.
    extra = [align, unif_u, unif_i] of the forward."""
    name, batch_word = "align_uniform_loss", "pairs"

    def __init__(self, t, gamma):
        self.t, self.gamma = t, gamma

    def check(self, name, batch):
        if batch.dim() != 2 or batch.shape[1] != 2:
            raise _lib.TagrecError(f"{name}: a batch of shape {tuple(batch.shape)} does not fit the alignment / uniformity loss "
                                   "(expected [B, 2] = user, positive; nothing is sampled)")
        if batch.shape[0] < 2:
            raise _lib.TagrecError(f"{name}: a batch of one pair (B = 1) has no other pair to be uniform against")

    def fwd(self, batch, Ub, Ib, Ureg, Ireg):
        res, self.extra, self.state = rowops.directau_fwd(Ub, Ib, Ureg, Ireg, self.t, self.gamma)
        return res

    def bwd(self, Ub, Ib, Ureg, Ireg, g, dUb, dIb, dUreg, dIreg, what=None):
        rowops.directau_bwd(Ub, Ib, Ureg, Ireg, self.state, g[:2], dUb, dIb, dUreg, dIreg, *self._what("directau_bwd", what))


class Catalogue(_Stage):
    """[B, 2] = (user, positive) under the full softmax: every item of the catalogue is a column of the user's softmax
    (`rowops.catsoftmax_fwd` / `catsoftmax_bwd`; the B x n_item logits are never stored).  Nothing is sampled.
    positives (`help.user_positives_csr`'s pair, or None: no mask): the user's other train items leave the row's softmax."""
    name, batch_word = "catalogue_softmax_loss", "pairs"
    grads_zeroed = on_tables = dense = True      # the dense store covers the item block only: the rest of d_out arrives zeroed

    def __init__(self, temperature, positives=None):
        self.temperature, self.positives = temperature, positives

    def check(self, name, batch):
        if batch.dim() != 2 or batch.shape[1] != 2:
            raise _lib.TagrecError(f"{name}: pairs {tuple(batch.shape)} must be [B, 2] = (user, positive)")

    def fwd_on_tables(self, batch, out, ego, n_user, n_item):
        """The stage on the full [user | item] tables `out` (and `ego`: the L2 part's, or None): the users' rows are read
        at batch[:, 0] by the kernel, the item block is the column table."""
        self._cut = lambda t: (None, None) if t is None else (t[:n_user], t[n_user:n_user + n_item])
        self.n_user = n_user
        self.urow, self.target = self.ids(batch)
        res, self.lse, _ = rowops.catsoftmax_fwd(*self._cut(out), self.target, self.temperature, self.urow, *self._cut(ego),
                                                 mask=self.positives)
        return res

    def bwd_on_tables(self, out, ego, g, d_out, d_ego, plan=None, what=None):
        """d_out (zeroed outside its item block by the caller): the item block is STORED by the kernel, then the compact user
        gradients are folded onto the user rows; ego / d_ego (None: no L2 part): the compact L2 rows are folded onto d_ego
        last -- d_ego may be d_out.  d_out None: the L2 part only, added to what d_ego holds.
        plan (the `row_list_plan` of `rows`, users then items): both folds run in a fixed order, no float atomics."""
        B, D = self.urow.shape[0], out.shape[1]
        kw = {"mask": self.positives}
        if what is not None:
            kw["what"] = f"catsoftmax_bwd({what})"
        d_e = dQr = dTr = None
        if ego is not None and d_ego is not None:
            d_e = torch.empty(2 * B, ego.shape[1], dtype=torch.float32, device=out.device)
            dQr, dTr = d_e[:B], d_e[B:]
        Ue, Ie = self._cut(ego if d_e is not None else None)
        if d_out is not None:
            # through a plan the user gradients travel as the first B of the plan's 2 B slots; the item slots add zero
            d_q = torch.zeros(2 * B, D, dtype=torch.float32, device=out.device) if plan is not None else \
                torch.empty(B, D, dtype=torch.float32, device=out.device)
            rowops.catsoftmax_bwd(*self._cut(out), self.target, self.temperature, self.lse, g, self._cut(d_out)[1], d_q[:B],
                                  self.urow, Ue, Ie, dQr, dTr, **kw)
            if plan is not None:
                rowops.scatter_rows_ordered(d_out, plan, d_q, True)
            else:
                d_out[:self.n_user].index_add_(0, self.urow, d_q)
        elif d_e is not None:
            rowops.catsoftmax_bwd(*self._cut(out), self.target, self.temperature, self.lse, g, None, None, self.urow, Ue, Ie,
                                  dQr, dTr, **kw)
        if d_e is not None:
            rowops.fold_rows(d_ego, plan.rows if plan is not None else self.rows_of(), d_e, plan)

    def rows_of(self):
        return torch.cat([self.urow, self.n_user + self.target])
