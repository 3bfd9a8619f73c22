"""LightGCN behind the reference's model surface (/root/reference/model/lightgcn.py).

    LightGCN(data)            ctor reads data.num / data.ui_adj[/ut_adj/it_adj] and the config   (:11-35)
    .forward()                -> tuple(user_emb, item_emb[, tag_emb])                              (:49-63)
    .loss(batch[B,3])         -> (mul_loss, reg * l2reg_loss on EGO rows), both differentiable     (:68-82)
    .predict_rating(users)    -> sigmoid(U_b I^T), [b, n_item]                                     (:84-89)
    .state_dict()             keys embed.0 / embed.1 [/ embed.2], as the reference's ParameterList

Differences in mechanism, not in results:
  * the per-type tables are row slices of ONE contiguous N x D parameter (`table`), so the
    `torch.cat` / `torch.split` copies of :52,62 disappear and Adam is one launch;
  * each layer is one fused HIP kernel (SpMM + L2-normalise + running layer mean), and the whole
    backward is hand-derived: BPR scatter, then one fused SpMM + normalise-backward per layer.
"""
import torch

from . import _lib, help as H, rowops
from .base import FusedStepModel, StepWorkspace, _Token, fused_last_hop, step_buffer, xavier_tables  # noqa: F401  (xavier_tables re-exported)
from .base import layer_seed as _layer_seed
from .config import CFG as _GLOBAL_CFG, check_catalogue_mask, check_negatives, check_ranking, check_softmax_over
from .graph import EdgeDropView, Graph, creat_adj
from .rowops import VEC_WIDTHS
from .train import fused_optimizer


def propagate_forward(graph, x0, n_layer, drops=None, seed=0, loss_rows=None, masks_out=None):
    """x0 -> (out, raws, invs): out = mean(x0, z1..zL), raws[k] = dropout(A raws[k-1]) (un-normalised),
    invs[k][r] = 1/max(||raws[k][r]||, 1e-12).  One fused kernel per layer.  drops[k] > 0 = message dropout of
    layer k's product (lightgcn.py:56), drawn inside the kernel from (seed, layer, element).

    loss_rows (int64 node ids): `out` will be read at these rows only (the batch rows of the BPR loss).  Then the last
    layer is computed on them alone and the layer below it on their neighbours (anything further down reaches nearly
    every node through the popular items, so it runs in full); the rows left out stay zero in raws / invs and are
    never read with a non-zero gradient in the backward pass.  Needs a square graph and a vector-kernel width.
    masks_out (dict): receives {layer: row mask} of the restricted layers, for `propagate_backward`."""
    s = 1.0 / (n_layer + 1)
    out = x0 * s
    raws, invs = [], []
    x = x0
    masks = {}
    if (loss_rows is not None and n_layer >= 1 and graph.shape[0] == graph.shape[1] and x0.shape[1] in VEC_WIDTHS
            and loss_rows.numel() * 16 <= x0.shape[0]):              # a batch that touches most rows gains nothing
        top = torch.zeros(x0.shape[0], dtype=torch.uint8, device=x0.device)
        top.index_fill_(0, loss_rows, 1)
        masks[n_layer - 1] = top
        if n_layer >= 2:
            masks[n_layer - 2] = graph.mark_rows(loss_rows, torch.zeros_like(top))
    if masks_out is not None:
        masks_out.update(masks)
    for k in range(n_layer):
        if k in masks:
            y = torch.zeros_like(x0)
            inv = torch.zeros(x0.shape[0], dtype=torch.float32, device=x0.device)
            graph.spmm_norm_acc_rows(x, y, inv, out, s, masks[k], drops[k] if drops else 0.0, _layer_seed(seed, k))
            raws.append(y)
            invs.append(inv)
            x = y
            continue
        y = torch.empty_like(x0)
        inv = torch.empty(x0.shape[0], dtype=torch.float32, device=x0.device)
        graph.spmm_norm_acc(x, y, inv, out, s, drops[k] if drops else 0.0, _layer_seed(seed, k))
        raws.append(y)
        invs.append(inv)
        x = y
    return out, raws, invs


def propagate_backward(graph_t, d_out, raws, invs, drops=None, seed=0, masks=None, fused=None):
    """Gradient of `propagate_forward` w.r.t. x0 given d_out (dense [N,D]).
    G^L = nb(X^L);  G^k = A^T G^(k+1) + nb(X^k);  G^0 = A^T G^1 + s*d_out,  nb = normalise-backward of s*d_out.
    With dropout each G^k (k >= 1) is multiplied by layer k's mask / (1 - p) before it travels on (it is the gradient
    w.r.t. the product the mask was applied to).
    masks = the row masks of a restricted forward (`propagate_forward(masks_out=...)`): a layer that was computed on
    masks[k] only has raws[k] = invs[k] = 0 elsewhere, and the gradient arriving from the layer above lives on rows
    whose neighbours all lie inside masks[k] -- so G^k is exactly zero outside masks[k] and those rows are not visited."""
    L = len(raws)
    s = 1.0 / (L + 1)
    if L == 0:
        return d_out.clone()
    n, D = d_out.shape
    g = torch.empty_like(d_out)
    # The gradient is non-zero on the batch rows only at the head of the chain and spreads by one hop per layer:
    # every product is told which rows of its operand hold a non-zero and leaves the others unfetched (bit-identical
    # result; the kernel ignores the flags once they cover 4/5 of the rows, without a host round trip).
    sparse = D in VEC_WIDTHS
    if sparse:
        flags = [torch.empty(n, dtype=torch.uint8, device=d_out.device) for _ in range(2)]
        counts = torch.zeros(2, dtype=torch.int32, device=d_out.device)
        rowops.rownorm_bwd_flags(raws[L - 1], invs[L - 1], d_out, s, g, flags[0], counts[0:1])
    else:
        rowops.rownorm_bwd(raws[L - 1], invs[L - 1], d_out, s, g)
    if drops and drops[L - 1] > 0:
        H.message_drop(g, drops[L - 1], _layer_seed(seed, L - 1), out=g)     # flags stay a superset of the non-zero rows
    cur = 0
    for k in range(L - 2, -1, -1):
        mask = masks.get(k) if (masks and sparse and (k + 1) in masks) else None
        gn = torch.empty_like(d_out) if mask is None else torch.zeros_like(d_out)
        if sparse:
            if mask is not None:
                flags[1 - cur].zero_()
            graph_t.spmm_normbwd_sparse(g, flags[cur], counts[cur:cur + 1], raws[k], invs[k], d_out, s, gn, flags[1 - cur],
                                        counts[1 - cur:2 - cur], drops[k] if drops else 0.0, _layer_seed(seed, k), mask)
            cur = 1 - cur
        else:
            graph_t.spmm_normbwd(g, raws[k], invs[k], d_out, s, gn, drops[k] if drops else 0.0, _layer_seed(seed, k))
        g = gn
    if isinstance(graph_t, EdgeDropView):
        fused = None                      # the Adam-in-epilogue hop has no edge-drop form: the optimizer gets a gradient tensor
    if fused is not None and sparse:      # (table, optimizer): Adam in the epilogue of the last hop, no gradient tensor
        fused_last_hop(graph_t, fused, g, flags[cur], counts[cur:cur + 1], d_out, s, None)
        return None
    g0 = torch.empty_like(d_out)
    if sparse:
        graph_t.spmm_axpy_sparse(g, flags[cur], counts[cur:cur + 1], d_out, s, g0)
    else:
        graph_t.spmm_axpy(g, d_out, s, g0)
    return g0


def spmm_listed(graph, rows, x, out=None):
    """(A x)[rows] as a compact [len(rows), D] tensor (rows int64, may repeat)."""
    return graph.spmm_listed(rows, x, out)


def restricted_forward(graph, x0, n_layer, rows, ws=None, want_ego=False):
    """The forward pass of a training step whose loss reads the layer mean at `rows` (int64 node ids [T], may repeat)
    only -- the BPR batch rows (lightgcn.py:71-75).  Layers below L-1 run on all rows (through the popular items every
    row is within two hops of the batch), layer L-1 on the batch rows and their neighbours (row-masked kernel), layer L
    in compact form on the batch rows alone (`spmm_listed`); no layer accumulates the mean, which is formed at the end
    on the T rows by one row kernel (`rowops.layer_mean_rows`), which also gathers the ego rows x0[rows] when want_ego.
    Returns (out_b [T, D], state for `restricted_backward`[, ego_b [T, D]]).  Rows a layer did not compute are left
    UNWRITTEN in its output; every later reader is told which rows are valid."""
    L, s = n_layer, 1.0 / (n_layer + 1)
    n, D = x0.shape
    dev = x0.device
    mid = graph.mark_rows(rows, step_buffer(ws, "mid", (n,), torch.uint8, dev).zero_()) if L >= 2 else None
    raws, invs = [], []
    x = x0
    for k in range(L - 1):
        y = step_buffer(ws, f"y{k}", (n, D), torch.float32, dev)
        inv = step_buffer(ws, f"inv{k}", (n,), torch.float32, dev)
        graph.spmm_norm_acc_rows(x, y, inv, None, 0.0, mid if k == L - 2 else None)
        raws.append(y)
        invs.append(inv)
        x = y
    y_top = spmm_listed(graph, rows, x)
    z_top, inv_top = rowops.rownorm_fwd(y_top)
    out_b, ego_b = rowops.layer_mean_rows(x0, rows, raws, invs, z_top, s, want_ego)
    state = (raws, invs, mid, y_top, inv_top)
    return (out_b, state, ego_b) if want_ego else (out_b, state)


# The masked hop of `restricted_backward` from an inverted list of the batch rows' entries (Graph.batch_hop_plan) instead of a
# walk over every masked row.  False: always the masked row kernel (same values; the same bits on rows of <= 1024 entries).
BATCH_HOP_LIST = True


def batch_hop_plan(graph_t, rows, ws=None):
    """The per-step plan of the list-driven masked hop of A = graph_t, or None where the masked row kernel serves better:
    a list or a matrix larger than the plan kernels take, or a record bound -- the sum of the len(rows) largest row degrees, cached on
    the graph -- above a quarter of the stored entries (the plan's buffers would rival the matrix)."""
    if isinstance(graph_t, EdgeDropView):     # edge dropout: the list-driven hop has no edge-drop form; the masked row kernel has
        return None
    src = graph_t.transpose()                 # its batch rows store exactly the entries of A that point at a batch row
    T = rows.numel()
    if (not BATCH_HOP_LIST or T < 1 or T > Graph.BATCH_HOP_MAX_LISTED or src.shape[0] != src.shape[1]
            or src.shape[0] > Graph.BATCH_HOP_MAX_ROWS):
        return None
    cap = src.batch_hop_capacity(T)
    if cap < 1 or cap > src.nnz // 4:
        return None
    buf = step_buffer(ws, "hop_plan", (src.batch_hop_workspace(T, cap),), torch.uint8, rows.device)
    return src.batch_hop_plan(rows, cap, buf)


def row_plan(rows, n, D, ws=None):
    """The step's `rowops.row_list_plan` of the batch rows (deterministic mode): one plan, kept in the step workspace, serves
    every fold of the step's compact [3 B, D] gradients into [n, D] tables."""
    buf = step_buffer(ws, "row_plan", (rowops.row_list_workspace(rows.numel(), D),), torch.uint8, rows.device)
    return rowops.row_list_plan(rows, n, buf, D)


def restricted_backward(graph_t, rows, d_out_b, state, shape, fused=None, ws=None, plan=None):
    """Gradient w.r.t. x0 of `restricted_forward` given d_out_b [T, D] = d loss / d out_b.  The chain starts on the batch
    rows (compact), lands on their neighbours (row-masked hop: G is non-zero there only) and spreads from there; every
    operand travels with one flag byte per row and zero rows are not gathered; the normalize-backward / mean terms exist
    on the batch rows only (dz_flags), so no other row's epilogue reads X_raw or dZ.
    plan (`row_plan` of rows): the compact gradients are folded onto the batch rows in a fixed order instead of by
    `index_add_` (float atomics where a batch names a node twice)."""
    raws, invs, mid, y_top, inv_top = state
    n, D = shape
    L = len(raws) + 1
    s = 1.0 / (L + 1)
    T = rows.numel()
    dev = d_out_b.device
    tflag = step_buffer(ws, "tflag", (n,), torch.uint8, dev).zero_()
    tflag.index_fill_(0, rows, 1)
    dz = step_buffer(ws, "dz", (n, D), torch.float32, dev)              # d loss / d out, valid on the batch rows only
    if plan is not None:
        rowops.scatter_rows_ordered(dz, plan, d_out_b, False)
    else:
        dz.index_fill_(0, rows, 0.0)
        dz.index_add_(0, rows, d_out_b)
    g_top = torch.empty(T, D, dtype=torch.float32, device=dev)
    rowops.rownorm_bwd(y_top, inv_top, d_out_b, s, g_top)
    g = step_buffer(ws, "g_top", (n, D), torch.float32, dev)             # G^L: valid on the batch rows only (flags = tflag)
    if plan is not None:
        rowops.scatter_rows_ordered(g, plan, g_top, False)
    else:
        g.index_fill_(0, rows, 0.0)
        g.index_add_(0, rows, g_top)
    flags, count = tflag, None                                           # count None: the flags are always consulted
    hop = batch_hop_plan(graph_t, rows, ws) if L >= 2 else None
    for k in range(L - 2, -1, -1):
        masked = k == L - 2
        gn = step_buffer(ws, f"g{k & 1}", (n, D), torch.float32, dev)
        fo = step_buffer(ws, f"fo{k & 1}", (n,), torch.uint8, dev)
        if masked:
            fo.zero_()
        cnt = step_buffer(ws, f"cnt{k & 1}", (1,), torch.int32, dev).zero_()
        if masked and hop is not None:    # rows of `mid` without a record or a dz term stay unwritten, their flag zero
            graph_t.batch_hop_normbwd(hop, g, raws[k], invs[k], dz, s, gn, fo, mid, tflag)
        else:
            graph_t.spmm_normbwd_sparse(g, flags, count, raws[k], invs[k], dz, s, gn, fo, cnt, row_mask=mid if masked else None,
                                        dz_flags=tflag)
        raws[k] = invs[k] = None          # last use: the 4 N D bytes go back to the allocator before the next hop allocates
        # a masked hop wrote the rows of `mid` only: its flags must always be honoured; a full hop wrote every row
        g, flags, count = gn, fo, (None if masked else cnt)
    if isinstance(graph_t, EdgeDropView):
        fused = None                  # the Adam-in-epilogue hop has no edge-drop form: the optimizer gets a gradient tensor
    if fused is not None:             # (table, optimizer): the last hop applies Adam to the table, no gradient is written
        fused_last_hop(graph_t, fused, g, flags, count, dz, s, tflag)
        return None
    g0 = torch.empty(n, D, dtype=torch.float32, device=dev)              # (handed to the optimizer: not a workspace buffer)
    graph_t.spmm_axpy_sparse(g, flags, count, dz, s, g0, b_flags=tflag)
    return g0


class _Propagate(torch.autograd.Function):
    @staticmethod
    def forward(ctx, table, graph, n_layer, drops=None, seed=0):
        out, raws, invs = propagate_forward(graph, table.detach(), n_layer, drops, seed)
        ctx.graph, ctx.raws, ctx.invs, ctx.drops, ctx.seed = graph, raws, invs, drops, seed
        return out

    @staticmethod
    def backward(ctx, d_out):
        g0 = propagate_backward(ctx.graph.transpose(), d_out.contiguous(), ctx.raws, ctx.invs, ctx.drops, ctx.seed)
        ctx.raws = ctx.invs = None
        return g0, None, None, None, None


class _PropagateBprLoss(torch.autograd.Function):
    """table -> [mul_loss, l2reg_loss(ego rows), *stage.extra] in one autograd node; stage: the loss stage (loss_stage.py)."""

    @staticmethod
    def forward(ctx, table, graph, n_layer, n_user, n_item, batch, stage, reg_active, drops=None, seed=0, restrict=True,
                fused_opt=None, ws=None, deterministic=False):
        x0 = table.detach()
        n, D = x0.shape
        ctx.ws, ctx.token = None, _Token()
        if ws is not None and ws.acquire(ctx.token):
            ctx.ws = ws
        # compact: the loss reads `out` at the batch rows only, and the top layers run on them alone (a batch that touches
        # most rows gains nothing); on_tables: the triplet kernels gather from the full tables themselves
        # a dense stage (every item row is a loss row) is never compact and nothing of its forward pass is row-masked
        restrict = restrict and not stage.dense
        compact = bool(restrict and drops is None and n_layer >= 1 and graph.shape[0] == graph.shape[1] and D in VEC_WIDTHS
                       and batch.numel() * 16 <= n)
        on_tables = not compact and stage.on_tables
        if stage.dense and not on_tables:
            raise _lib.TagrecError(f"{stage.name}: a dense stage has the on-tables form only")
        rows = stage.rows(batch, n_user) if (restrict or deterministic or not on_tables) else None
        # deterministic: one sorted plan of the batch rows per step; every fold of compact gradients goes through it
        plan = row_plan(rows, n, D, ctx.ws) if deterministic else None
        B = batch.shape[0]
        if compact:
            out_b, ctx.state, ego_b = restricted_forward(graph, x0, n_layer, rows, ctx.ws, want_ego=True)
        else:
            ctx.masks = {}
            out, ctx.raws, ctx.invs = propagate_forward(graph, x0, n_layer, drops, seed, rows if restrict else None, ctx.masks)
            ctx.drops, ctx.seed = drops, seed
        if on_tables:
            res = stage.fwd_on_tables(batch, out, x0, n_user, n_item)
            ctx.saved = (out, x0)
        else:
            if not compact:                  # the kernels take gathered rows only
                out_b, ego_b = out.index_select(0, rows), x0.index_select(0, rows)
            res = stage.fwd(batch, out_b[:B], out_b[B:], ego_b[:B], ego_b[B:])
            ctx.saved = (out_b, ego_b)
        # (table, optimizer): Adam in the epilogue of the backward pass's last hop -- which the L2 term would arrive too late for
        ctx.fused = (table, fused_opt) if (fused_opt is not None and not reg_active and n_layer >= 1) else None
        ctx.graph, ctx.stage, ctx.rows, ctx.plan, ctx.B, ctx.shape = graph, stage, rows, plan, B, x0.shape
        ctx.compact, ctx.on_tables, ctx.reg_active = compact, on_tables, reg_active
        return res if stage.extra is None else torch.cat([res, stage.extra])      # the extra entries carry no gradient

    @staticmethod
    def backward(ctx, g):
        stage, rows, plan, B, reg = ctx.stage, ctx.rows, ctx.plan, ctx.B, ctx.reg_active
        graph_t = ctx.graph.transpose()
        if ctx.on_tables:
            out, x0 = ctx.saved
            d_out = torch.zeros_like(out)
            stage.bwd_on_tables(out, None, g, d_out, None, plan)
        else:
            out_b, ego_b = ctx.saved
            # d / d out_b, d / d ego_b
            d_b, d_e = (torch.zeros if stage.grads_zeroed else torch.empty)(2, *out_b.shape, dtype=torch.float32, device=out_b.device)
            U, I, dU, dI = out_b[:B], out_b[B:], d_b[:B], d_b[B:]
            Ue, Ie, dUe, dIe = (ego_b[:B], ego_b[B:], d_e[:B], d_e[B:]) if reg else (None,) * 4
            if reg and stage.reg_apart:      # the L2 rows get a launch of their own, below
                stage.bwd(U, I, None, None, g, dU, dI, None, None)
            else:
                stage.bwd(U, I, Ue, Ie, g, dU, dI, dUe, dIe)
        if ctx.compact:
            g0 = restricted_backward(graph_t, rows, d_b, ctx.state, ctx.shape, ctx.fused, ctx.ws, plan)
        else:
            if not ctx.on_tables:
                d_out = rowops.fold_rows(torch.zeros(ctx.shape, dtype=torch.float32, device=d_b.device), rows, d_b, plan)
            g0 = propagate_backward(graph_t, d_out, ctx.raws, ctx.invs, ctx.drops, ctx.seed, ctx.masks, ctx.fused)
        # L2 term on the ego rows: added after the propagation hop has written g0
        if reg and ctx.on_tables:
            stage.bwd_on_tables(out, x0, g, None, g0, plan, "reg")
        elif reg:
            if stage.reg_apart:
                stage.bwd(U, I, Ue, Ie, g, None, None, dUe, dIe, "reg")
            rowops.fold_rows(g0, rows, d_e, plan)
        ctx.state = ctx.raws = ctx.invs = ctx.saved = None
        if ctx.ws is not None:
            ctx.ws.release(ctx.token)
        return (g0,) + (None,) * 13


class LightGCN(FusedStepModel):
    def __init__(self, data, args=None, config=None, graph=None):
        super().__init__()
        self._config(config if config is not None else _GLOBAL_CFG)
        self._init_table(data, self.use_tag, self.dim_latent, self.device)
        self.norm_adj = graph if graph is not None else creat_adj(data, self.use_tag, self.norm_type,
                                                                  self.split_adj_k, self.device)
        # the logQ correction of in-batch negatives: log(train degree / train edges) per item, fixed at construction
        self.item_logq = H.item_logq_table(data.edge_index["train"], self.num_list[1], self.device) if self.in_batch_logq else None
        # catalogue_mask="train_positives": every user's train items as a CSR, fixed at construction (rowops.catsoftmax_* mask)
        self.positives = H.user_positives_csr(data.edge_index["train"], self.num_list[0], self.num_list[1], self.device) \
            if self.mask_positives else None

    def _config(self, config):
        self.dim_latent = config["dim_latent"]
        self.num_layer = len(config["dim_layer_list"])   # only the LENGTH matters (lightgcn.py:27)
        self.device = torch.device(config["device"])
        self.norm_type = config["norm_type"]
        self.split_adj_k = config["split_adj_k"]
        self.reg = config["reg"]
        # K negatives per positive: batches are [B, 2 + K]; K > 1 or "softmax" takes the multi-negative loss kernels
        _lib.refuse_ultragcn(config, type(self).__name__)       # the ug_* keys are UltraGCN's: refused, not ignored
        self.n_negatives, self.loss_func, self.loss_temperature = check_ranking(config)
        # negatives="in_batch": [B, 2] batches, the other positives of the batch are the negatives (rowops.inbatch_*)
        self.in_batch, self.in_batch_logq = check_negatives(config)
        # softmax_over="catalogue": [B, 2] batches, every item is a column of the user's softmax (rowops.catsoftmax_*)
        self.over_catalogue = check_softmax_over(config)
        # catalogue_mask="train_positives": the user's other train items leave the row's softmax (help.user_positives_csr)
        self.mask_positives = check_catalogue_mask(config)
        self.use_tag = config["use_tag"]
        self.message_drop_list = config["message_drop_list"]
        self.node_drop = config["node_drop"]
        # "kernel": edge dropout evaluated inside the products (Graph.edge_drop) instead of a CSR rebuilt per forward pass
        self.node_drop_mode = config.get("node_drop_mode", "rebuild")
        if self.node_drop_mode not in H.NODE_DROP_MODES:
            raise _lib.TagrecError(f"LightGCN: unknown node_drop_mode {self.node_drop_mode!r} (have {H.NODE_DROP_MODES})")
        self.drop_seed = config.get("seed", 2020)
        # loss(): compute the top two layers only on the rows the batch's loss depends on (propagate_forward)
        self.restrict_forward = bool(config.get("restrict_forward", True))
        # persistent buffers of the restricted training step (base.StepWorkspace); config["step_workspace"] = False: allocate per step
        self.step_ws = StepWorkspace() if config.get("step_workspace", True) else None
        # one step = a pure function of its inputs: batch gradients are folded in a fixed order (rowops.scatter_rows_ordered)
        self.deterministic = bool(config.get("deterministic", False))

    def _fused_ok(self):
        return isinstance(self.norm_adj, Graph)

    def train(self, mode=True):
        if isinstance(getattr(self, "norm_adj", None), Graph):     # the host-side check of the steps' device-built hop plans
            self.norm_adj.batch_hop_check()
        return super().train(mode)

    def _check_drop_width(self):
        if self.dim_latent not in VEC_WIDTHS:
            raise _lib.TagrecError("LightGCN: fused message dropout needs dim_latent in {8,16,...,256}")

    def _graph(self):
        """The adjacency of this forward pass.  Kernel-mode edge dropout draws one seed per training-mode call, advanced like
        the message-dropout seed (`_drops`): every layer of the pass and its backward see the same dropped graph."""
        if self.node_drop_mode != "kernel" or not self.training or self.node_drop == 0:
            return H.node_drop(self.norm_adj, self.node_drop, self.training)
        if not isinstance(self.norm_adj, Graph):
            raise _lib.TagrecError("LightGCN: node_drop_mode='kernel' does not cover row folds (split_adj_k > 1)")
        if self.dim_latent not in VEC_WIDTHS:
            raise _lib.TagrecError("LightGCN: node_drop_mode='kernel' needs dim_latent in {8,16,...,256}")
        if torch.cuda.is_current_stream_capturing():
            raise _lib.TagrecError("LightGCN: kernel-mode node_drop draws a new seed on the host every step and cannot be "
                                   "captured in a HIP graph")
        self._node_drop_calls = getattr(self, "_node_drop_calls", 0) + 1
        return H.node_drop(self.norm_adj, self.node_drop, True, "kernel", (int(self.drop_seed) << 24) + self._node_drop_calls)

    def _propagate(self):
        graph = self._graph()
        if self._fused_ok():
            drops, seed = self._drops()
            return _Propagate.apply(self.table, graph, self.num_layer, drops, seed)
        # operator-by-operator path (row folds / message dropout), same order as lightgcn.py:52-60
        x = self.table
        layers = [x]
        for k in range(self.num_layer):
            x = H.split_mm(graph, x)
            x = torch.nn.functional.dropout(x, p=self.message_drop_list[k], training=self.training)
            layers.append(H.normalize_rows(x))
        return torch.mean(torch.stack(layers, dim=1), dim=1)

    def forward(self):
        return self._split(self._propagate())

    def _route(self, batch_data):
        """The loss stage of this model's step for `batch_data` (a subclass with another objective overrides it)."""
        if self.in_batch:
            return H.in_batch_route(type(self).__name__, batch_data, self.loss_temperature, self.item_logq)
        if self.over_catalogue:
            return H.catalogue_route(type(self).__name__, batch_data, self.loss_temperature, self.positives)
        return H.rank_route(type(self).__name__, batch_data, self.n_negatives, self.loss_func, self.loss_temperature)

    def loss(self, batch_data):
        batch_data = batch_data.to(self.device, torch.int64).contiguous()
        nu, ni = self.num_list[0], self.num_list[1]
        stage = H.stage_for(self._route(batch_data), H.loss_kind_id(self.loss_func))
        if self._fused_ok():
            graph = self._graph()                       # (first: kernel-mode edge dropout refuses a capture before any launch)
            drops, seed = self._drops()
            fused = fused_optimizer(self) if (self.training and torch.is_grad_enabled()) else None
            res = _PropagateBprLoss.apply(self.table, graph, self.num_layer, nu, ni, batch_data, stage, self.reg != 0, drops, seed,
                                          self.restrict_forward, fused,
                                          self.step_ws if (self.training and torch.is_grad_enabled()) else None, self.deterministic)
        elif self.deterministic:
            raise _lib.TagrecError("LightGCN: deterministic=True covers the fused step only (no row folds: split_adj_k == 1)")
        else:
            all_users, all_items = self.forward()[:2]
            res = H.stage_loss(stage, all_users, all_items, *self.embed[:2], batch_data)
        if stage.extra is not None:
            self.last_au_parts = res[2:].detach()
        return res[0], self.reg * res[1]
