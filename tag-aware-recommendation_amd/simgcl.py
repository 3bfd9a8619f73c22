"""SimGCL: LightGCN plus an InfoNCE term between two noise-perturbed views of the batch's nodes (Yu et al., "Are Graph
Augmentations Necessary?", SIGIR 2022).  Not in the reference; the surface is LightGCN's.

    SimGCL(data)            LightGCN's constructor; config keys cl_rate, cl_eps, cl_temperature (config.check_contrastive)
    .forward() / .predict_rating() / .state_dict()     inherited, unperturbed
    .loss(batch)            -> (mul_loss, reg * l2reg, cl_rate * cl_loss); the first two ARE LightGCN.loss(batch)

The contrastive part.  S_u / S_i = the sorted unique users / items of the batch (columns 0 and 1), rows = cat(S_u, n_user + S_i).
A view v in {0, 1} is the model's own propagation with every layer k = 1 .. L perturbed:
    y_k = A x'_{k-1} (x'_0 = table),   x'_k = y_k + cl_eps sign(y_k) n_{v,k}(r),   z_k = x'_k / max(||x'_k||, 1e-12),
    e^v = mean(x_0, z_1 .. z_L)
n_{v,k}(r) is a unit vector drawn INSIDE the layer kernels from (step seed, view, layer, node id r) -- include/tagrec.h has the
key -- so nothing is stored and the all-rows product, the row-masked product and the compact top layer perturb a node the same
way.  cl_loss = sum over S in {S_u, S_i} of mean_i [logsumexp_j(a_i . b_j / tau) - a_i . b_i / tau], a / b = the row-normalised
e^0[S] / e^1[S]: `rowops.inbatch_fwd` without ids, bias or L2 rows.

Backward: inbatch_bwd -> rownorm_bwd -> the view's propagation backward.  The perturbation has derivative 1 almost everywhere
(d y_k = d x'_k), so the backward kernels of LightGCN run unchanged on the stored perturbed raws; no backward kernel
re-creates the noise.  Each view is its own autograd node on the table; autograd adds the three table gradients.

Two execution paths per view, as in the parent: the compact restricted step (lower layers on all rows, layer L - 1 row-masked,
layer L = spmm_listed + noise_rownorm_fwd on the T listed rows; `restricted_backward`) when the graph is square, D is a
vector-kernel width, 16 T <= n and L >= 1 -- else an all-rows pass that accumulates the mean (`propagate_backward`)."""
import torch

from . import _lib, rowops
from .base import StepWorkspace, _Token, step_buffer
from .config import check_contrastive
from .graph import Graph
from .lightgcn import LightGCN, propagate_backward, restricted_backward, row_plan, spmm_listed
from .rowops import VEC_WIDTHS


def noisy_propagate_forward(graph, x0, n_layer, eps, seed, view):
    """`lightgcn.propagate_forward` of one view on all rows: x0 -> (out, raws, invs), raws[k] the PERTURBED product of layer
    k + 1 (what the next layer gathers and what `propagate_backward` reads)."""
    s = 1.0 / (n_layer + 1)
    out = x0 * s
    raws, invs = [], []
    x = x0
    for k in range(n_layer):
        y = torch.empty_like(x0)
        inv = torch.empty(x0.shape[0], dtype=torch.float32, device=x0.device)
        graph.spmm_norm_acc_noise(x, y, inv, out, s, None, eps, seed, view, k + 1)
        raws.append(y)
        invs.append(inv)
        x = y
    return out, raws, invs


def noisy_restricted_forward(graph, x0, n_layer, rows, eps, seed, view, ws=None):
    """`lightgcn.restricted_forward` of one view: the same layer schedule and the same state for `restricted_backward`, every
    layer through the noise form of its kernel.  rows: int64 node ids [T]; they key the top layer's noise."""
    L, s = n_layer, 1.0 / (n_layer + 1)
    n, D = x0.shape
    dev = x0.device
    mid = graph.mark_rows(rows, step_buffer(ws, "mid", (n,), torch.uint8, dev).zero_()) if L >= 2 else None
    raws, invs = [], []
    x = x0
    for k in range(L - 1):
        y = step_buffer(ws, f"y{k}", (n, D), torch.float32, dev)
        inv = step_buffer(ws, f"inv{k}", (n,), torch.float32, dev)
        graph.spmm_norm_acc_noise(x, y, inv, None, 0.0, mid if k == L - 2 else None, eps, seed, view, k + 1)
        raws.append(y)
        invs.append(inv)
        x = y
    y_top = spmm_listed(graph, rows, x)
    z_top, inv_top = rowops.noise_rownorm_fwd(y_top, rows, eps, seed, view, L)       # y_top now holds the perturbed rows
    out_b = x0.index_select(0, rows) * s
    for y, inv in zip(raws, invs):
        out_b.addcmul_(y.index_select(0, rows), inv.index_select(0, rows)[:, None], value=s)
    out_b.add_(z_top, alpha=s)
    return out_b, (raws, invs, mid, y_top, inv_top)


class _View(torch.autograd.Function):
    """table -> e^v[rows] ([T, D]) of one perturbed view, in one autograd node."""

    @staticmethod
    def forward(ctx, table, graph, n_layer, rows, eps, seed, view, compact, ws, deterministic):
        x0 = table.detach()
        n, D = x0.shape
        ctx.ws, ctx.token = None, _Token()
        if ws is not None and ws.acquire(ctx.token):
            ctx.ws = ws
        ctx.graph, ctx.rows, ctx.shape, ctx.compact = graph, rows, x0.shape, compact
        # the rows are unique, so no fold collides; the plan is passed anyway so that deterministic mode runs the tested path
        ctx.plan = row_plan(rows, n, D, ctx.ws) if deterministic else None
        if compact:
            out_b, ctx.state = noisy_restricted_forward(graph, x0, n_layer, rows, eps, seed, view, ctx.ws)
            return out_b
        out, ctx.raws, ctx.invs = noisy_propagate_forward(graph, x0, n_layer, eps, seed, view)
        return out.index_select(0, rows)

    @staticmethod
    def backward(ctx, d_b):
        d_b = d_b.contiguous()
        if ctx.compact:
            g0 = restricted_backward(ctx.graph.transpose(), ctx.rows, d_b, ctx.state, ctx.shape, None, ctx.ws, ctx.plan)
            ctx.state = None
        else:
            d_out = rowops.fold_rows(torch.zeros(ctx.shape, dtype=torch.float32, device=d_b.device), ctx.rows, d_b, ctx.plan)
            g0 = propagate_backward(ctx.graph.transpose(), d_out, ctx.raws, ctx.invs)
            ctx.raws = ctx.invs = None
        if ctx.ws is not None:
            ctx.ws.release(ctx.token)
        return (g0,) + (None,) * 9


class _InfoNCE(torch.autograd.Function):
    """(e0, e1 [T, D], split) -> l(rows [:split]) + l(rows [split:]), l = the in-batch softmax of the row-normalised views."""

    @staticmethod
    def forward(ctx, e0, e1, split, tau):
        e0, e1 = e0.contiguous(), e1.contiguous()
        a, inv_a = rowops.rownorm_fwd(e0)
        b, inv_b = rowops.rownorm_fwd(e1)
        total, lses = None, []
        for sl in (slice(0, split), slice(split, e0.shape[0])):
            res, lse = rowops.inbatch_fwd(a[sl], b[sl], None, None, tau)
            total = res[0] if total is None else total + res[0]
            lses.append(lse)
        ctx.saved = (e0, e1, a, b, inv_a, inv_b, lses)
        ctx.split, ctx.tau = split, tau
        return total

    @staticmethod
    def backward(ctx, g):
        e0, e1, a, b, inv_a, inv_b, lses = ctx.saved
        ctx.saved = None
        g2 = torch.zeros(2, dtype=torch.float32, device=a.device)
        g2[0] = g
        da, db = torch.empty_like(a), torch.empty_like(b)
        for sl, lse in zip((slice(0, ctx.split), slice(ctx.split, a.shape[0])), lses):
            rowops.inbatch_bwd(a[sl], b[sl], None, None, ctx.tau, lse, g2, da[sl], db[sl], None, None)
        d0 = rowops.rownorm_bwd(e0, inv_a, da, 1.0, torch.empty_like(e0))
        d1 = rowops.rownorm_bwd(e1, inv_b, db, 1.0, torch.empty_like(e1))
        return d0, d1, None, None


class SimGCL(LightGCN):
    def __init__(self, data, args=None, config=None, graph=None):
        super().__init__(data, args, config, graph)
        name = type(self).__name__
        if self.split_adj_k > 1 or not isinstance(self.norm_adj, Graph):
            raise _lib.TagrecError(f"{name}: the views run inside the fused products, which do not cover row folds (split_adj_k > 1)")
        if self.dim_latent not in VEC_WIDTHS:
            raise _lib.TagrecError(f"{name}: the noise kernels need dim_latent in {{8,16,...,256}}, got {self.dim_latent}")
        if any(float(p) != 0 for p in self.message_drop_list) or float(self.node_drop) != 0:
            raise _lib.TagrecError(f"{name}: message_drop_list / node_drop must be zero (the views are the model's only augmentation)")
        # one workspace per view: the two views of a step are alive at the same time
        self.view_ws = [StepWorkspace(), StepWorkspace()] if self.step_ws is not None else [None, None]
        self._cl_calls = 0
        self.last_cl_seed = None          # seed of the views of the latest training-mode loss() (tests re-create its noise)

    def _config(self, config):
        super()._config(config)
        self.cl_rate, self.cl_eps, self.cl_temperature = check_contrastive(config)

    def set_fused_optimizer(self, opt):
        if opt is not None:
            raise _lib.TagrecError("SimGCL: Adam.fuse_into is not covered -- the table receives three gradients (the ranking "
                                   "loss and two views), and the update in the epilogue would apply the first one alone")
        super().set_fused_optimizer(None)

    def _cl_seed(self):
        """Seed of this step's views; it advances with every training-mode loss(), like the message-dropout seed."""
        if torch.cuda.is_current_stream_capturing():
            raise _lib.TagrecError("SimGCL: the contrastive views draw a new seed on the host every step and cannot be "
                                   "captured in a HIP graph")
        self._cl_calls += 1
        self.last_cl_seed = (int(self.drop_seed) << 24) + self._cl_calls
        return self.last_cl_seed

    def view_rows(self, batch_data):
        """(rows = cat(S_u, n_user + S_i), |S_u|): the sorted unique users and items of the batch's first two columns."""
        s_u = torch.unique(batch_data[:, 0])
        s_i = torch.unique(batch_data[:, 1]) + self.num_list[0]
        return torch.cat([s_u, s_i]), int(s_u.numel())

    def views(self, rows, seed):
        """(e^0[rows], e^1[rows]), each an autograd node on the table."""
        n, D = self.table.shape
        g = self.norm_adj
        compact = bool(self.restrict_forward and self.num_layer >= 1 and g.shape[0] == g.shape[1] and D in VEC_WIDTHS
                       and rows.numel() * 16 <= n)
        live = self.training and torch.is_grad_enabled()
        return tuple(_View.apply(self.table, g, self.num_layer, rows, self.cl_eps, seed, v, compact,
                                 self.view_ws[v] if live else None, self.deterministic) for v in (0, 1))

    def cl_loss(self, batch_data, seed):
        rows, split = self.view_rows(batch_data)
        e0, e1 = self.views(rows, seed)
        return _InfoNCE.apply(e0, e1, split, self.cl_temperature)

    def loss(self, batch_data):
        batch_data = batch_data.to(self.device, torch.int64).contiguous()
        if self.training and self.cl_rate != 0:
            seed = self._cl_seed()                     # (first: a capture is refused before any launch)
        parts = super().loss(batch_data)
        if not (self.training and self.cl_rate != 0):
            return parts[0], parts[1], torch.zeros((), dtype=torch.float32, device=self.table.device)
        return parts[0], parts[1], self.cl_rate * self.cl_loss(batch_data, seed)
