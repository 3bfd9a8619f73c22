"""Operator surface of /root/reference/model/help (adj.py, loss.py), same names and
argument meaning, backed by the HIP library through `torch.autograd.Function`s.

    split_mm(norm_adj, all_embed)            adj.py:158-167
    node_drop(graph, keep_prob, training)    adj.py:170-191
    mul_loss(u, p, n, loss_func)             loss.py:4-12
    l2reg_loss(*embs)                        loss.py:27-32
    transtag_loss / transe_loss              loss.py:35-50
    cor_loss(factor_emb, factor_k)           loss.py:53-80   (kernels: csrc/cor.hip, host side: cor.py)
    ncl_structure_loss / ncl_prototype_loss  --              (NCL's two contrast terms on the catalogue-softmax kernels; model: ncl.py)
    creat_adj(...)                           adj.py:38-46   (re-exported from graph.py)

Inputs must be GPU tensors; there is no CPU path.
"""
from typing import NamedTuple, Optional

import torch

from . import _lib, loss_stage as S, rowops
from .cor import cor_loss  # noqa: F401  (the distance-correlation penalty between factor slices)
from .graph import Graph, coalesce_device, creat_adj  # noqa: F401  (creat_adj re-exported)


def _new_like_rows(g, D, ref):
    return torch.empty(g.shape[0], D, dtype=torch.float32, device=ref.device)


class _SpMM(torch.autograd.Function):
    """Y = A @ X; backward dX = A^T @ dY (A carries no gradient, as in the reference
    where norm_adj is a constant sparse tensor)."""

    @staticmethod
    def forward(ctx, X, graph):
        ctx.graph = graph
        return graph.spmm(X.contiguous())

    @staticmethod
    def backward(ctx, dY):
        return ctx.graph.transpose().spmm(dY.contiguous()), None


def split_mm(norm_adj, all_embed):
    """One `Graph`, or a list of row-fold Graphs whose products are concatenated
    along dim 0 -- the reference's `split_adj_k` memory workaround."""
    if isinstance(norm_adj, (list, tuple)):
        return torch.cat([_SpMM.apply(all_embed, g) for g in norm_adj], dim=0)
    return _SpMM.apply(all_embed, norm_adj)


class _RowNormalize(torch.autograd.Function):
    """F.normalize(x, p=2, dim=1) (eps 1e-12) with its analytic backward."""

    @staticmethod
    def forward(ctx, X):
        X = _lib.require_gpu_tensor(X.contiguous(), torch.float32, "normalize_rows input")
        Z, inv = rowops.rownorm_fwd(X)
        ctx.save_for_backward(X, inv)
        return Z

    @staticmethod
    def backward(ctx, dZ):
        X, inv = ctx.saved_tensors
        return rowops.rownorm_bwd(X, inv, dZ.contiguous(), 1.0, torch.empty_like(X))


def normalize_rows(x):
    return _RowNormalize.apply(x)


class _TripletLoss(torch.autograd.Function):
    """BPR loss on tables + triplet indices (the gather is part of the kernel).
    Returns a 2-vector: [mul_loss, l2reg_loss (unweighted)]."""

    @staticmethod
    def forward(ctx, U, I, Ureg, Ireg, trip, loss_kind):
        for t, nm in ((U, "U"), (I, "I"), (Ureg, "Ureg"), (Ireg, "Ireg")):
            if t is not None:
                _lib.require_gpu_tensor(t, torch.float32, "bpr " + nm)
        trip = _lib.require_gpu_tensor(trip.contiguous(), torch.int64, "bpr triplets")
        has_reg = Ureg is not None
        out, coef = rowops.bpr_fwd(U, I, Ureg, Ireg, trip, loss_kind)
        ctx.save_for_backward(U, I, Ureg if has_reg else U.new_empty(0), Ireg if has_reg else U.new_empty(0), trip, coef)
        ctx.has_reg = has_reg
        ctx.same = has_reg and Ureg.data_ptr() == U.data_ptr() and Ireg.data_ptr() == I.data_ptr()
        return out

    @staticmethod
    def backward(ctx, g):
        U, I, Ureg, Ireg, trip, coef = ctx.saved_tensors
        dU, dI = torch.zeros_like(U), torch.zeros_like(I)
        if ctx.has_reg and not ctx.same:
            dUr, dIr = torch.zeros_like(Ureg), torch.zeros_like(Ireg)
        elif ctx.has_reg:
            dUr, dIr = dU, dI
        else:
            dUr = dIr = Ureg = Ireg = None
        rowops.bpr_bwd(U, I, Ureg, Ireg, trip, coef, g, dU, dI, dUr, dIr)
        if ctx.has_reg and ctx.same:
            return dU, dI, None, None, None, None
        return dU, dI, (dUr if ctx.has_reg else None), (dIr if ctx.has_reg else None), None, None


def loss_kind_id(loss_func):
    if loss_func == "softmax":
        return _lib.LOSS_SOFTMAX
    return _lib.LOSS_LOGSIGMOID if loss_func == "logsigmoid" else _lib.LOSS_SOFTPLUS


class _GatheredRowsLoss(torch.autograd.Function):
    """A loss stage (loss_stage.py) on tables + an id batch: the batch's rows are gathered, the stage's compact kernels run on
    them and the compact gradients are folded back onto the tables.
    Returns [mul_loss, l2reg_loss (unweighted), *stage.extra]; only the first two carry a gradient."""

    @staticmethod
    def forward(ctx, U, I, Ureg, Ireg, batch, stage, plans):
        name = stage.name
        for t, nm in ((U, "U"), (I, "I"), (Ureg, "Ureg"), (Ireg, "Ireg")):
            if t is not None and (not t.is_cuda or t.dtype != torch.float32 or t.dim() != 2):
                raise _lib.TagrecError(f"{name}: {nm} must be a 2-d float32 GPU tensor")
        batch = _lib.require_gpu_tensor(batch.contiguous(), torch.int64, f"{name} {stage.batch_word}")
        stage.check(name, batch)
        urows, irows = stage.ids(batch)
        Ub, Ib = U.index_select(0, urows), I.index_select(0, irows)
        has_reg = Ureg is not None
        same = has_reg and Ureg.data_ptr() == U.data_ptr() and Ireg.data_ptr() == I.data_ptr() and Ureg.shape == U.shape
        Urb, Irb = (Ub, Ib) if same else ((Ureg.index_select(0, urows), Ireg.index_select(0, irows)) if has_reg else (None, None))
        res = stage.fwd(batch, Ub, Ib, Urb, Irb)
        ctx.save_for_backward(Ub, Ib, Urb if has_reg else U.new_empty(0), Irb if has_reg else U.new_empty(0), urows, irows)
        ctx.stage, ctx.has_reg, ctx.same, ctx.plans = stage, has_reg, same, plans
        ctx.shapes = (U.shape, I.shape, Ureg.shape if has_reg else None, Ireg.shape if has_reg else None)
        return res if stage.extra is None else torch.cat([res, stage.extra])

    @staticmethod
    def backward(ctx, g):
        Ub, Ib, Urb, Irb, urows, irows = ctx.saved_tensors
        pu, pi = ctx.plans if ctx.plans is not None else (None, None)
        dUb, dIb = torch.empty_like(Ub), torch.empty_like(Ib)
        if ctx.has_reg and ctx.same:
            Urb, Irb, dUrb, dIrb = Ub, Ib, dUb, dIb        # reg on the same rows: one gradient buffer
        elif ctx.has_reg:
            dUrb, dIrb = torch.empty_like(Urb), torch.empty_like(Irb)
        else:
            Urb = Irb = dUrb = dIrb = None
        ctx.stage.bwd(Ub, Ib, Urb, Irb, g, dUb, dIb, dUrb, dIrb)

        def fold(shape, rows, src, plan):
            return rowops.fold_rows(torch.zeros(shape, dtype=torch.float32, device=src.device), rows, src, plan)

        dU, dI = fold(ctx.shapes[0], urows, dUb, pu), fold(ctx.shapes[1], irows, dIb, pi)
        if ctx.has_reg and not ctx.same:
            return dU, dI, fold(ctx.shapes[2], urows, dUrb, pu), fold(ctx.shapes[3], irows, dIrb, pi), None, None, None
        return dU, dI, None, None, None, None, None


class _RowSparseLoss(torch.autograd.Function):
    """`_GatheredRowsLoss` on ONE [user | item] table under a row optimizer (`train.RowAdam`), the L2 part on the same rows:
    one plan over the stage's rows, which are caught up to the optimizer's step before they are gathered; the backward
    hands (plan, compact gradient) to the optimizer and returns NO gradient for the table -- `table.grad` stays None and
    nothing table-sized is allocated.  Returns [mul_loss, l2reg_loss (unweighted)]."""

    @staticmethod
    def forward(ctx, table, batch, stage, n_user, opt, owner):
        # owner[0]: the parameter itself, the optimizer's key for the table (`table` may be autograd's alias of it)
        name = stage.name
        if not table.is_cuda or table.dtype != torch.float32 or table.dim() != 2:
            raise _lib.TagrecError(f"{name}: the table must be a 2-d float32 GPU tensor")
        batch = _lib.require_gpu_tensor(batch.contiguous(), torch.int64, f"{name} {stage.batch_word}")
        stage.check(name, batch)
        rows = stage.rows(batch, n_user)                 # the user slots, then the item slots shifted by n_user
        plan = rowops.row_list_plan(rows, table.shape[0], None, table.shape[1])
        opt.catch_up(owner[0], plan)
        B = batch.shape[0]
        Tb = table.detach().index_select(0, rows)
        Ub, Ib = Tb[:B], Tb[B:]
        res = stage.fwd(batch, Ub, Ib, Ub, Ib)
        ctx.saved = (owner[0], Tb, plan, B)
        ctx.stage, ctx.opt = stage, opt
        return res

    @staticmethod
    def backward(ctx, g):
        param, Tb, plan, B = ctx.saved
        d = torch.empty_like(Tb)
        Ub, Ib, dUb, dIb = Tb[:B], Tb[B:], d[:B], d[B:]
        ctx.stage.bwd(Ub, Ib, Ub, Ib, g, dUb, dIb, dUb, dIb)       # reg on the same rows: one gradient buffer
        ctx.opt.row_grad(param, plan, d)
        return None, None, None, None, None, None


def ultragcn_row_loss(table, n_user, tuples, tables, opt, stage=None):
    """`ultragcn_loss` of the [user | item] `table` (both parts on the same rows) for a training step under the row
    optimizer `opt` (`train.RowAdam`, attached): the same values, but the gradient goes to the optimizer as (plan, compact
    rows) and the table receives none.  The fold order is `ultragcn_plans`' -- a row's slots ascending, the user slots
    before the item slots -- whatever `deterministic` says."""
    out = _RowSparseLoss.apply(table, tuples, stage if stage is not None else S.Ultra(tables), n_user, opt, (table,))
    return out[0], out[1]


def stage_loss(stage, U, I, Ureg, Ireg, batch, plans=None):
    """[mul_loss, l2reg_loss (unweighted), *stage.extra] of `batch` against user / item tables under a loss stage: what the
    fused steps' autograd nodes return, operator by operator.  The triplet stage gathers inside its kernels (`_TripletLoss`)."""
    if isinstance(stage, S.Triplet):
        if Ureg is not None and Ureg.data_ptr() == U.data_ptr() and Ireg.data_ptr() == I.data_ptr():
            Ureg, Ireg = U, I          # reg on the same rows: one gradient buffer
        return _TripletLoss.apply(U, I, Ureg, Ireg, batch, stage.loss_kind)
    if stage.dense:                    # every row of I is an operand: nothing to gather
        return _CatalogueLoss.apply(U, I, Ureg, Ireg, batch, stage, plans)
    return _GatheredRowsLoss.apply(U, I, Ureg, Ireg, batch, stage, plans)


def rank_route(model, batch, n_negatives, loss_func, temperature):
    """Which loss stage a model's step takes for `batch` [B, 2 + K]: None = the triplet kernels (K = 1 with softplus /
    logsigmoid, exactly as before), else (K, temperature) for the multi-negative kernels.  A batch whose width disagrees with
    the model's n_negatives is refused."""
    if batch.dim() != 2 or batch.shape[1] != 2 + n_negatives:
        raise _lib.TagrecError(f"{model}: a batch of shape {tuple(batch.shape)} does not fit n_negatives={n_negatives} "
                               f"(expected [B, {2 + n_negatives}] = user, positive, {n_negatives} negative(s))")
    return (n_negatives, float(temperature)) if (n_negatives > 1 or loss_func == "softmax") else None


def ranking_plans(tuples, n_user, n_item, width=256):
    """(plan of the user slots, plan of the item slots) of a [B, 2 + K] tuple batch for `ranking_loss(plans=...)`: the
    `rowops.row_list_plan`s of its B user ids over n_user rows and of its (1 + K) B item ids (slot order) over n_item rows."""
    return (rowops.row_list_plan(tuples[:, 0].contiguous(), n_user, None, width),
            rowops.row_list_plan(tuples[:, 1:].t().reshape(-1), n_item, None, width))


def ranking_loss(U, I, Ureg, Ireg, tuples, loss_func, temperature=1.0, plans=None):
    """(mul_loss, l2reg_loss) of a [B, 2 + K] batch (user, positive, K negatives; K in 1 .. 63) against user / item tables:
    the multi-negative sibling of `triplet_loss`.  loss_func "softmax": mean_b [logsumexp_j(s_j / temperature) - s_0 /
    temperature]; "softplus" / "logsigmoid": the mean over the B K (positive, negative) pairs of `mul_loss`'s expression.
    l2reg_loss = 0.5 (|u|^2 + |p|^2 + sum_k |n_k|^2) / B on the rows of Ureg / Ireg (None: 0).
    plans (`ranking_plans`): the compact gradients are folded onto the tables in a fixed order (the same bits every run)
    instead of by `index_add_`."""
    out = stage_loss(S.Rank(loss_kind_id(loss_func), float(temperature)), U, I, Ureg, Ireg, tuples, plans)
    return out[0], out[1]


class UltraTables(NamedTuple):
    """The constants of UltraGCN's loss (Mao et al., CIKM 2021), built once from the train edges (`ultragcn_tables`)."""
    beta_u: torch.Tensor                   # [n_user] float32: sqrt(d_u + 1) / d_u, 0 at d_u = 0
    beta_i: torch.Tensor                   # [n_item] float32: 1 / sqrt(d_i + 1)
    nbr_id: Optional[torch.Tensor]         # [n_item, M] int64 co-occurrence neighbours, -1 = pad; None: no neighbour term
    nbr_w: Optional[torch.Tensor]          # [n_item, M] float32 omega, 0 at the pads
    w: tuple = (1e-6, 1.0, 1e-6, 1.0)      # w1 .. w4
    negative_weight: float = 10.0
    lam: float = 1.0                       # lambda of the neighbour term


def ultragcn_tables(edge_index, n_user, n_item, device, neighbors=10, zero_diagonal=False, w=(1e-6, 1.0, 1e-6, 1.0),
                    negative_weight=10.0, lam=1.0, **cooc_args):
    """`UltraTables` of the train edges [E, 2] = (user, item): the degree weights (fp64 on the host side of the edge list,
    rounded once) and, with neighbors > 0, every item's `neighbors` heaviest co-occurrence neighbours
    (`cooc.item_cooccurrence_topk`; cooc_args: its lds_limit / workspace_bytes)."""
    from .cooc import cooc_csrs, item_cooccurrence_topk
    csrs = cooc_csrs(edge_index, n_user, n_item, device)
    du = (csrs.ui_ptr[1:] - csrs.ui_ptr[:-1]).to(torch.float64)
    di = (csrs.iu_ptr[1:] - csrs.iu_ptr[:-1]).to(torch.float64)
    beta_u = torch.where(du > 0, torch.sqrt(du + 1) / du.clamp(min=1), torch.zeros_like(du)).to(torch.float32)
    beta_i = (1.0 / torch.sqrt(di + 1)).to(torch.float32)
    nbr_id = nbr_w = None
    if neighbors:
        nbr_id, nbr_w, _ = item_cooccurrence_topk(None, n_user, n_item, int(neighbors), zero_diagonal, csrs=csrs, **cooc_args)
        nbr_id = nbr_id.to(torch.int64)
    return UltraTables(beta_u, beta_i, nbr_id, nbr_w, tuple(float(x) for x in w), float(negative_weight), float(lam))


def ultragcn_plans(tuples, tables, n_user, n_item, width=256, stage=None):
    """(plan of the user slots, plan of the item slots) of a [B, 2 + K] tuple batch for `ultragcn_loss(plans=...)`: the item
    slots are the positive, the K negatives and the positive's neighbours, in the stage's slot order.  stage (an
    `loss_stage.Ultra` of `tables`, made for THIS batch): its slot ids are built here and reused by `ultragcn_loss(stage=...)`,
    so the neighbour gather runs once per step."""
    uid, iid = (stage if stage is not None else S.Ultra(tables)).ids(tuples)
    return rowops.row_list_plan(uid, n_user, None, width), rowops.row_list_plan(iid, n_item, None, width)


def ultragcn_loss(U, I, Ureg, Ireg, tuples, tables, plans=None, stage=None):
    """(mul_loss, l2reg_loss) of a [B, 2 + K] batch (user, positive, K >= 1 negatives) under UltraGCN's objective as a MEAN
    over the batch (the paper's code sums): with s = u . i, b_u = sqrt(d_u + 1) / d_u and b_i = 1 / sqrt(d_i + 1),
        mul_loss = (1 / B) sum_b [ (w1 + w2 b_u b_p) softplus(-s_p) + (negative_weight / K) sum_k (w3 + w4 b_u b_nk) softplus(s_nk)
                                   + lam sum_{j in top-M co-occurrence neighbours of p} omega_pj softplus(-s_j) ]
    l2reg_loss = 0.5 (|u|^2 + |p|^2 + sum_k |n_k|^2) / B on the rows of Ureg / Ireg (None: 0; the neighbour rows carry none).
    tables: `ultragcn_tables`.  plans (`ultragcn_plans`): the compact gradients are folded onto the tables in a fixed order (the
    same bits every run) instead of by `index_add_`.  stage: the `loss_stage.Ultra` that `ultragcn_plans` was handed for this
    batch (None: a new one)."""
    out = stage_loss(stage if stage is not None else S.Ultra(tables), U, I, Ureg, Ireg, tuples, plans)
    return out[0], out[1]


class InBatchRoute(NamedTuple):
    """What a fused step is handed in place of `rank_route`'s (K, temperature) when the model has negatives="in_batch"."""
    temperature: float
    item_logq: Optional[torch.Tensor]      # [n_item] logQ table, or None: no column bias


def in_batch_route(model, batch, temperature, item_logq=None):
    """A model with negatives="in_batch" takes [B, 2] = (user, positive) batches; any other width is refused.
    -> the `InBatchRoute` its step takes."""
    if batch.dim() != 2 or batch.shape[1] != 2:
        raise _lib.TagrecError(f"{model}: a batch of shape {tuple(batch.shape)} does not fit negatives=\"in_batch\" "
                               "(expected [B, 2] = user, positive; the negatives are the other positives of the batch)")
    return InBatchRoute(float(temperature), item_logq)


def in_batch_plans(pairs, n_user, n_item, width=256):
    """(plan of the user rows, plan of the item rows) of a [B, 2] pair batch for `in_batch_loss(plans=...)`."""
    return (rowops.row_list_plan(pairs[:, 0].contiguous(), n_user, None, width),
            rowops.row_list_plan(pairs[:, 1].contiguous(), n_item, None, width))


def item_logq_table(edge_index, n_item, device):
    """log(train degree of the item / number of train edges) [n_item] float32, computed in float64: the logQ correction of
    in-batch negatives (an item appears as an in-batch negative in proportion to its degree).  Degree 0 gives 0: such an
    item never enters a batch."""
    import numpy as np
    edges = edge_index.cpu().numpy() if torch.is_tensor(edge_index) else np.asarray(edge_index)      # [E, 2] = (user, item)
    items = edges[:, 1].astype(np.int64)
    deg = np.bincount(items, minlength=n_item).astype(np.float64)
    out = np.zeros(n_item, dtype=np.float64)
    nz = deg > 0
    out[nz] = np.log(deg[nz] / float(items.shape[0]))
    return torch.from_numpy(out.astype(np.float32)).to(device)


def in_batch_loss(U, I, Ureg, Ireg, pairs, temperature=1.0, item_logq=None, plans=None):
    """(mul_loss, l2reg_loss) of a [B, 2] batch (user, positive) with in-batch negatives: the other B - 1 positives of the
    batch are every user's negatives, except the entries that name the same item or the same user (masked).
    mul_loss = mean_b [logsumexp_{j unmasked}(z_bj) - z_bb], z_bj = u_b . i_j / temperature - item_logq[item_j] (None: no
    correction); l2reg_loss = 0.5 (|u|^2 + |p|^2) / B on the rows of Ureg / Ireg (None: 0).  The B x B scores are never stored.
    plans (`in_batch_plans`): the compact gradients are folded onto the tables in a fixed order (the same bits every run)
    instead of by `index_add_`."""
    out = stage_loss(S.InBatch(float(temperature), item_logq), U, I, Ureg, Ireg, pairs, plans)
    return out[0], out[1]


def user_positives_csr(edge_index, n_user, n_item, device):
    """The train items of every user as a CSR for the masked catalogue softmax (catalogue_mask="train_positives"):
    -> (ptr int64 [n_user + 1], items int32), a user's items ascending and unique (duplicate edges fold, the order of the
    edges does not matter), a user without edges has an empty row.  edge_index: [E, 2] = (user, item), a tensor or an array;
    built once on the host (numpy), as `item_logq_table` is, then moved to `device`."""
    import numpy as np
    edges = edge_index.cpu().numpy() if torch.is_tensor(edge_index) else np.asarray(edge_index)
    edges = edges.reshape(-1, 2).astype(np.int64)
    if n_item > 2 ** 31 - 1:
        raise _lib.TagrecError(f"user_positives_csr: the item ids are kept as int32, n_item={n_item} does not fit")
    users, items = edges[:, 0], edges[:, 1]
    if edges.shape[0] and (users.min() < 0 or users.max() >= n_user or items.min() < 0 or items.max() >= n_item):
        raise _lib.TagrecError(f"user_positives_csr: an edge lies outside [0, {n_user}) x [0, {n_item})")
    keys = np.unique(users * np.int64(n_item) + items)                      # sorted by (user, item), duplicates gone
    ptr = np.zeros(n_user + 1, dtype=np.int64)
    np.cumsum(np.bincount(keys // n_item, minlength=n_user), out=ptr[1:])
    return torch.from_numpy(ptr).to(device), torch.from_numpy((keys % n_item).astype(np.int32)).to(device)


class CatalogueRoute(NamedTuple):
    """What a fused step is handed in place of `rank_route`'s (K, temperature) when the model has softmax_over="catalogue"."""
    temperature: float
    positives: Optional[tuple] = None      # `user_positives_csr`'s pair (catalogue_mask="train_positives"), or None: no mask


def catalogue_route(model, batch, temperature, positives=None):
    """A model with softmax_over="catalogue" takes [B, 2] = (user, positive) batches; any other width is refused.
    -> the `CatalogueRoute` its step takes."""
    if batch.dim() != 2 or batch.shape[1] != 2:
        raise _lib.TagrecError(f"{model}: a batch of shape {tuple(batch.shape)} does not fit softmax_over=\"catalogue\" "
                               "(expected [B, 2] = user, positive; every item of the catalogue is a column of the softmax)")
    return CatalogueRoute(float(temperature), positives)


class _CatalogueLoss(torch.autograd.Function):
    """The catalogue stage (loss_stage.Catalogue) on tables + a pair batch: the kernels read the user rows at the batch's ids
    and walk the whole item table, the item gradient is stored dense and the compact user / L2 gradients are folded onto
    their tables.  Returns [mul_loss, l2reg_loss (unweighted)]."""

    @staticmethod
    def forward(ctx, U, I, Ureg, Ireg, pairs, stage, plans):
        name = stage.name
        for t, nm in ((U, "U"), (I, "I"), (Ureg, "Ureg"), (Ireg, "Ireg")):
            if t is not None and (not t.is_cuda or t.dtype != torch.float32 or t.dim() != 2):
                raise _lib.TagrecError(f"{name}: {nm} must be a 2-d float32 GPU tensor")
        pairs = _lib.require_gpu_tensor(pairs.contiguous(), torch.int64, f"{name} {stage.batch_word}")
        stage.check(name, pairs)
        urow, target = stage.ids(pairs)
        has_reg = Ureg is not None
        same = has_reg and Ureg.data_ptr() == U.data_ptr() and Ireg.data_ptr() == I.data_ptr() and Ureg.shape == U.shape
        res, lse, _ = rowops.catsoftmax_fwd(U, I, target, stage.temperature, urow, Ureg, Ireg, mask=stage.positives)
        ctx.save_for_backward(U, I, Ureg if has_reg else U.new_empty(0), Ireg if has_reg else U.new_empty(0), urow, target, lse)
        ctx.tau, ctx.has_reg, ctx.same, ctx.plans, ctx.mask = stage.temperature, has_reg, same, plans, stage.positives
        return res

    @staticmethod
    def backward(ctx, g):
        U, I, Ureg, Ireg, urow, target, lse = ctx.saved_tensors
        pu, pi = ctx.plans if ctx.plans is not None else (None, None)
        B = urow.shape[0]
        dI = torch.empty(I.shape, dtype=torch.float32, device=I.device)
        dUr = dIr = None
        if ctx.has_reg:
            dUr, dIr = torch.empty(2, B, Ureg.shape[1], dtype=torch.float32, device=U.device)
        else:
            Ureg = Ireg = None
        dQ = rowops.catsoftmax_bwd(U, I, target, ctx.tau, lse, g, dI, None, urow, Ureg, Ireg, dUr, dIr, mask=ctx.mask)
        dU = rowops.fold_rows(torch.zeros(U.shape, dtype=torch.float32, device=U.device), urow, dQ, pu)
        if not ctx.has_reg:
            return dU, dI, None, None, None, None, None
        if ctx.same:                           # reg on the same rows: the L2 rows join the two gradients
            rowops.fold_rows(dU, urow, dUr, pu)
            rowops.fold_rows(dI, target, dIr, pi)
            return dU, dI, None, None, None, None, None
        dUreg = rowops.fold_rows(torch.zeros(Ureg.shape, dtype=torch.float32, device=U.device), urow, dUr, pu)
        dIreg = rowops.fold_rows(torch.zeros(Ireg.shape, dtype=torch.float32, device=U.device), target, dIr, pi)
        return dU, dI, dUreg, dIreg, None, None, None


def catalogue_softmax_loss(U, I, Ureg, Ireg, pairs, temperature=1.0, plans=None, positives=None):
    """(mul_loss, l2reg_loss) of a [B, 2] batch (user, positive) under the full softmax: EVERY row of I is a column,
    mul_loss = mean_b [logsumexp_n(u_b . i_n / temperature) - u_b . i_{p_b} / temperature]; nothing is sampled or corrected,
    and nothing is masked unless `positives` is given.  l2reg_loss = 0.5 (|u|^2 + |p|^2) / B on the rows of Ureg / Ireg (None: 0).  The B x n_item logits are never
    stored; the gradient of I is dense.  The ids must lie inside the tables (not checked: that would take a host read).
    plans (`in_batch_plans`): the compact user and L2 gradients are folded onto the tables in a fixed order (the same bits
    every run) instead of by `index_add_`.
    positives (`user_positives_csr`'s pair over the rows of U; None: no mask): a pair (u, p) leaves u's OTHER listed items out
    of its softmax -- they are not negatives -- and their gradient coefficient is exactly 0; p itself stays a column whether
    or not it is listed."""
    out = stage_loss(S.Catalogue(float(temperature), positives), U, I, Ureg, Ireg, pairs, plans)
    return out[0], out[1]


class _NodeContrast(torch.autograd.Function):
    """One softmax of the NCL terms: the mean over b of logsumexp_n(z_bn) - z_{b, target_b}, z_bn = nrm(Y[qrows_b]) . t_n /
    temperature, through the catalogue-softmax kernels (`rowops.catsoftmax_*`, no L2 rows).  Repeated qrows are kept.
      t_const False   T = raw rows, t_n = nrm(T[n]); the gradient flows into BOTH operands: dQ -> rownorm_bwd -> a fold of
                      the repeated rows into dY; the dense dT -> rownorm_bwd -> dT.
      t_const True    T = unit rows taken as they are (a centroid table), a constant: only dY is returned; the dT the backward
                      kernel stores all the same lands in a scratch buffer and is dropped.
    plan: the `rowops.row_list_plan` of qrows over the rows of Y (the fold then runs in a fixed order), or None."""

    @staticmethod
    def forward(ctx, Y, T, qrows, target, temperature, t_const, plan):
        what = "ncl contrast"
        for t, nm in ((Y, "Y"), (T, "T")):
            if not isinstance(t, torch.Tensor) or not t.is_cuda or t.dtype != torch.float32 or t.dim() != 2:
                raise _lib.TagrecError(f"{what}: {nm} must be a 2-d float32 GPU tensor")
        qrows = _lib.require_gpu_tensor(qrows, torch.int64, f"{what} qrows")
        target = _lib.require_gpu_tensor(target, torch.int64, f"{what} target")
        q_raw = Y.index_select(0, qrows)
        Q, inv_q = rowops.rownorm_fwd(q_raw)
        if t_const:
            t_raw, inv_t, Tn = None, None, T.contiguous()
        else:
            t_raw = T.contiguous()
            Tn, inv_t = rowops.rownorm_fwd(t_raw)
        res, lse, _ = rowops.catsoftmax_fwd(Q, Tn, target, temperature)
        ctx.saved = (q_raw, Q, inv_q, t_raw, Tn, inv_t, qrows, target, lse)
        ctx.tau, ctx.plan, ctx.y_shape = float(temperature), plan, Y.shape
        return res[0].clone()

    @staticmethod
    def backward(ctx, g):
        q_raw, Q, inv_q, t_raw, Tn, inv_t, qrows, target, lse = ctx.saved
        ctx.saved = None
        g2 = torch.zeros(2, dtype=torch.float32, device=Q.device)
        g2[0] = g
        dT = torch.empty_like(Tn)                  # t_const: scratch, dropped
        dQ = rowops.catsoftmax_bwd(Q, Tn, target, ctx.tau, lse, g2, dT)
        dq_raw = rowops.rownorm_bwd(q_raw, inv_q, dQ, 1.0, torch.empty_like(q_raw))
        dY = rowops.fold_rows(torch.zeros(ctx.y_shape, dtype=torch.float32, device=Q.device), qrows, dq_raw, ctx.plan)
        dT_raw = None if t_raw is None else rowops.rownorm_bwd(t_raw, inv_t, dT, 1.0, torch.empty_like(t_raw))
        return dY, dT_raw, None, None, None, None, None


def _ncl_batch(what, batch):
    """(u_b, i_b): a batch's first two columns, each contiguous."""
    if batch.dim() != 2 or batch.shape[1] < 2 or batch.shape[0] < 1:
        raise _lib.TagrecError(f"{what}: a batch of shape {tuple(batch.shape)} has no (user, item) columns")
    return batch[:, 0].contiguous(), batch[:, 1].contiguous()


def ncl_structure_loss(x0, norm_adj, n_user, n_item, batch, temperature, alpha=1.0, deterministic=False):
    """NCL's structure term (Lin et al., WWW 2022, hyper_layers = 1) as a MEAN over the batch (the paper's code sums):
    y2 = A (A x0) is the raw two-hop product (two `split_mm`), (u_b, i_b) the batch's columns 0 and 1, repeats kept;
        L_su = mean_b [logsumexp_n(nrm(y2[u_b]) . nrm(U0[n]) / t) - nrm(y2[u_b]) . nrm(U0[u_b]) / t],   U0 = x0[:n_user]
        L_si   likewise with y2[n_user + i_b], I0 = x0[n_user : n_user + n_item] and i_b
    -> L_su + alpha * L_si.  The gradient flows into x0 through both operands of each softmax.  deterministic: the repeated
    rows' gradients are folded in a fixed order (`rowops.row_list_plan`), the same bits on every run."""
    what = "ncl_structure_loss"
    batch = _lib.require_gpu_tensor(batch.contiguous(), torch.int64, f"{what} batch")
    ub, ib = _ncl_batch(what, batch)
    n, D = x0.shape
    y2 = split_mm(norm_adj, split_mm(norm_adj, x0))
    qi = ib + n_user
    pu = rowops.row_list_plan(ub, n, None, D) if deterministic else None
    pi = rowops.row_list_plan(qi, n, None, D) if deterministic else None
    l_u = _NodeContrast.apply(y2, x0[:n_user], ub, ub, temperature, False, pu)
    l_i = _NodeContrast.apply(y2, x0[n_user:n_user + n_item], qi, ib, temperature, False, pi)
    return l_u + alpha * l_i


def ncl_prototype_loss(x0, n_user, n_item, batch, cent_u, cent_i, cluster_u, cluster_i, temperature, alpha=1.0,
                       deterministic=False):
    """NCL's prototype term as a MEAN over the batch: a node's ego row against the centroid table of its side,
        L_pu = mean_b [logsumexp_k(nrm(U0[u_b]) . Cu[k] / t) - nrm(U0[u_b]) . Cu[cluster_u[u_b]] / t]      and L_pi likewise
    -> L_pu + alpha * L_pi.  cent_u / cent_i [K, D]: the ROW-NORMALISED centroids; cluster_u [n_user] / cluster_i [n_item]:
    int64 cluster ids.  All four are constants: the gradient flows into x0 through the batch rows only."""
    what = "ncl_prototype_loss"
    batch = _lib.require_gpu_tensor(batch.contiguous(), torch.int64, f"{what} batch")
    ub, ib = _ncl_batch(what, batch)
    n, D = x0.shape
    for nm, c, cl, cnt in (("user", cent_u, cluster_u, n_user), ("item", cent_i, cluster_i, n_item)):
        if c.dim() != 2 or c.shape[1] != D or c.dtype != torch.float32 or not c.is_cuda:
            raise _lib.TagrecError(f"{what}: the {nm} centroids must be a float32 GPU tensor [K, {D}], got {tuple(c.shape)}")
        if cl.shape != (cnt,) or cl.dtype != torch.int64 or not cl.is_cuda:
            raise _lib.TagrecError(f"{what}: the {nm} cluster ids must be an int64 GPU tensor [{cnt}]")
    qi = ib + n_user
    pu = rowops.row_list_plan(ub, n, None, D) if deterministic else None
    pi = rowops.row_list_plan(qi, n, None, D) if deterministic else None
    l_u = _NodeContrast.apply(x0, cent_u.detach(), ub, cluster_u.index_select(0, ub), temperature, True, pu)
    l_i = _NodeContrast.apply(x0, cent_i.detach(), qi, cluster_i.index_select(0, ib), temperature, True, pi)
    return l_u + alpha * l_i


class AuRoute(NamedTuple):
    """What a fused step is handed in place of `rank_route`'s value by a DirectAU model: the alignment / uniformity loss."""
    t: float                               # the Gaussian potential exp(-t |x - y|^2) of the uniformity term
    gamma: float                           # its weight


def au_route(model, batch, t=2.0, gamma=1.0):
    """A DirectAU model takes [B, 2] = (user, positive) batches; any other width is refused.  -> the `AuRoute` of its step."""
    route = AuRoute(float(t), float(gamma))
    S.Au(*route).check(model, batch)
    return route


def stage_for(route, loss_kind):
    """The loss stage (loss_stage.py) of a step that was handed `route` -- the one place that tells the route values apart."""
    if route is None:
        return S.Triplet(loss_kind)
    if isinstance(route, InBatchRoute):
        return S.InBatch(*route)
    if isinstance(route, AuRoute):
        return S.Au(*route)
    if isinstance(route, CatalogueRoute):
        return S.Catalogue(*route)
    return S.Rank(loss_kind, route[1])


def align_uniform_loss(U, I, Ureg, Ireg, pairs, t=2.0, gamma=1.0, plans=None, parts_out=None):
    """(mul_loss, l2reg_loss) of a [B, 2] batch (user, positive) under DirectAU (Wang et al., KDD 2022): with x^ the
    row-normalised rows of the batch (repeated ids kept), mul_loss = mean_b |u^_b - i^_b|^2 + gamma (unif(U) + unif(I)) / 2,
    unif(X) = log mean_{i < j} exp(-t |x^_i - x^_j|^2); l2reg_loss = 0.5 (|u|^2 + |p|^2) / B on the rows of Ureg / Ireg
    (None: 0).  The B x B potentials are never stored.  0 < t <= 20, B >= 2.
    plans (`in_batch_plans`): the compact gradients are folded onto the tables in a fixed order (the same bits every run)
    instead of by `index_add_`.  parts_out (a list): receives the detached device tensor [align, unif_u, unif_i]."""
    out = stage_loss(S.Au(float(t), float(gamma)), U, I, Ureg, Ireg, pairs, plans)
    if parts_out is not None:
        parts_out.append(out[2:].detach())
    return out[0], out[1]


def triplet_loss(U, I, Ureg, Ireg, trip, loss_func):
    """(mul_loss, l2reg_loss) of a [B,3] triplet batch against user/item tables."""
    out = stage_loss(S.Triplet(loss_kind_id(loss_func)), U, I, Ureg, Ireg, trip)
    return out[0], out[1]


def mul_loss(users_emb, pos_emb, neg_emb, loss_func):
    """`mul_loss` on already gathered rows (loss.py:4-12)."""
    trip = rowops.compact_triplets(users_emb.shape[0], users_emb.device)
    items = torch.cat([pos_emb, neg_emb], dim=0)
    return _TripletLoss.apply(users_emb.contiguous(), items, None, None, trip, loss_kind_id(loss_func))[0]


def l2reg_loss(*embs):
    """0.5 * sum ||e||_F^2 / rows(first)  (loss.py:27-32); torch reductions on the GPU."""
    for e in embs:
        if not e.is_cuda:
            raise _lib.TagrecError("l2reg_loss: expected GPU tensors")
    tot = 0
    for e in embs:
        tot = tot + e.norm(2).pow(2)
    return 0.5 * tot / float(embs[0].shape[0])


class _TransTagLoss(torch.autograd.Function):
    """TransTag margin loss + L2 on table rows selected by a [B,4] (user, tag, pos_item, neg_item) batch;
    the gathers are part of the kernel.  Returns [loss, l2reg_loss (unweighted)]."""

    @staticmethod
    def forward(ctx, Eu, Ei, Et, quad, margin):
        for t, nm in ((Eu, "Eu"), (Ei, "Ei"), (Et, "Et")):
            _lib.require_gpu_tensor(t, torch.float32, "transtag " + nm)
        quad = _lib.require_gpu_tensor(quad.contiguous(), torch.int64, "transtag batch")
        B, D = quad.shape[0], Eu.shape[1]
        dist = torch.empty(B, 2, dtype=torch.float32, device=Eu.device)
        partials = torch.empty(2 * ((B + 3) // 4), dtype=torch.float32, device=Eu.device)
        out = torch.empty(2, dtype=torch.float32, device=Eu.device)
        _lib.check(_lib.load().tagrec_transtag_fwd_f32(Eu, Ei, Et, Eu.stride(0), D, quad, B, float(margin), dist, partials, out,
                                                       _lib.stream_ptr()), "transtag_fwd")
        ctx.save_for_backward(Eu, Ei, Et, quad, dist)
        ctx.margin = float(margin)
        return out

    @staticmethod
    def backward(ctx, g):
        Eu, Ei, Et, quad, dist = ctx.saved_tensors
        g = g.contiguous()
        dEu, dEi, dEt = torch.zeros_like(Eu), torch.zeros_like(Ei), torch.zeros_like(Et)
        _lib.check(_lib.load().tagrec_transtag_bwd_f32(Eu, Ei, Et, Eu.stride(0), Eu.shape[1], quad, quad.shape[0], ctx.margin,
                                                       dist, g, dEu, dEi, dEt, _lib.stream_ptr()), "transtag_bwd")
        return dEu, dEi, dEt, None, None


def transtag_batch_loss(Eu, Ei, Et, quad, margin):
    """(transtag_loss, l2reg_loss) of a [B,4] batch against the user / item / tag tables (tgcn.py:251-261)."""
    if not (Eu.stride(0) == Ei.stride(0) == Et.stride(0) and Eu.shape[1] == Ei.shape[1] == Et.shape[1]):
        raise _lib.TagrecError("transtag_batch_loss: tables must share width and row stride")
    out = _TransTagLoss.apply(Eu, Ei, Et, quad, margin)
    return out[0], out[1]


def transtag_loss(head_e, rela_e, pos_tail_e, neg_tail_e, margin=0):
    """mean relu(margin + ||h+r-t+|| - ||h+r-t-||)  (loss.py:35-41)."""
    if not head_e.is_cuda:
        raise _lib.TagrecError("transtag_loss: expected GPU tensors")
    ps = torch.norm(head_e + rela_e - pos_tail_e, p=2, dim=1)
    ns = torch.norm(head_e + rela_e - neg_tail_e, p=2, dim=1)
    return torch.relu(margin + ps - ns).mean()


def transe_loss(head_e, rela_e, pos_tail_e, neg_tail_e):
    """mean softplus(||h+r-t+|| - ||h+r-t-||)  (loss.py:44-50)."""
    ps = torch.norm(head_e + rela_e - pos_tail_e, p=2, dim=1)
    ns = torch.norm(head_e + rela_e - neg_tail_e, p=2, dim=1)
    return torch.nn.functional.softplus(ps - ns).mean()


def message_drop(x, p, seed, out=None, rows=None):
    """mask(seed) * x / (1 - p) with the library's counter-based mask (the one the fused layer kernels apply);
    p = 0 returns x.  rows (int64 [T], x is [T, d]): x holds rows `rows` of a full [N, d] tensor and element (j, c) takes
    the draw of element (rows[j], c) of that tensor -- repeated ids get the same mask."""
    if p <= 0:
        return x
    x = x.contiguous()
    out = torch.empty_like(x) if out is None else out
    if rows is not None:
        _lib.check(_lib.load().tagrec_dropout_rows_f32(x, out, rows, x.shape[0], x.shape[1], float(p), int(seed),
                                                       _lib.stream_ptr()), "dropout_rows")
        return out
    _lib.check(_lib.load().tagrec_dropout_f32(x, out, x.numel(), float(p), int(seed), _lib.stream_ptr()), "dropout")
    return out


class _MessageDrop(torch.autograd.Function):
    """`message_drop` with its backward (the same mask on the gradient)."""

    @staticmethod
    def forward(ctx, x, p, seed):
        ctx.p, ctx.seed = p, seed
        return message_drop(x, p, seed)

    @staticmethod
    def backward(ctx, g):
        return message_drop(g.contiguous(), ctx.p, ctx.seed), None, None


def message_dropout(x, p, seed):
    """F.dropout(x, p, training=True) with the library's counter-based mask (a function of seed and element index) instead
    of torch's generator: differentiable, and reproducible by every other path that is handed the same seed."""
    return x if p <= 0 else _MessageDrop.apply(x, float(p), int(seed))


NODE_DROP_MODES = ("rebuild", "kernel")


def node_drop(graph, keep_prob, training=False, mode="rebuild", seed=None):
    """Edge dropout (adj.py:170-191).  As in the reference the argument called
    `keep_prob` is the DROP rate: an edge survives iff int(rand + (1-drop)) != 0
    and survivors are divided by (1-drop).  The mask is drawn on the GPU (the
    reference draws it on the CPU), so parity is statistical.

    mode="rebuild": a torch.rand mask and a new CSR (and, for the backward pass, its transpose) per call.
    mode="kernel":  `Graph.edge_drop(keep_prob, seed)` -- a view of the same CSR whose products evaluate a counter-based
                    mask of (seed, row, column) as they go; nothing is rebuilt or sorted.  One Graph only (no row folds),
                    vector-kernel widths only; `seed` is required (one per training forward pass)."""
    if mode not in NODE_DROP_MODES:
        raise _lib.TagrecError(f"node_drop: unknown mode {mode!r} (have {NODE_DROP_MODES})")
    assert 0 <= keep_prob < 1
    if keep_prob == 0 or not training:
        return graph
    if mode == "kernel":
        if isinstance(graph, (list, tuple)):
            raise _lib.TagrecError("node_drop(mode='kernel'): row folds (split_adj_k > 1) are not covered; use mode='rebuild'")
        if seed is None:
            raise _lib.TagrecError("node_drop(mode='kernel'): a seed is required")
        return graph.edge_drop(keep_prob, seed)
    keep = 1.0 - keep_prob

    def drop(g):
        mask = (torch.rand(g.nnz, device=g.device) + keep).to(torch.int32).bool()
        deg = g.rowptr[1:] - g.rowptr[:-1]
        rows = torch.repeat_interleave(torch.arange(g.shape[0], device=g.device), deg)[mask]
        rp, c, v = coalesce_device(rows, g.col.long()[mask], g.val[mask] / keep, g.shape[0], g.shape[1])
        return Graph(rp, c, v, g.shape)          # the mask breaks symmetry: transpose is rebuilt

    if isinstance(graph, (list, tuple)):
        return [drop(g) for g in graph]
    return drop(graph)
