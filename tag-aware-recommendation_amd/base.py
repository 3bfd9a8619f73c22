"""Shared plumbing of the table-based models (LightGCN, NGCF): one contiguous [N, D] parameter whose
row slices are the reference's per-type tables, the `embed.k` state-dict layout, and the cached
`predict_rating` (/root/reference/model/lightgcn.py:37-47,84-89; model/ngcf.py:39-44,107-112)."""
import torch
import torch.nn as nn

from . import _lib, rowops
from .cor import cor_loss


def layer_seed(seed, k):
    """Seed of layer k's dropout mask within the forward pass seeded `seed`."""
    return (int(seed) * 64 + k) & 0xFFFFFFFFFFFFFFFF


def scatter_rows(n, rows, compact, plan=None):
    """[n, D] tensor that holds sum of compact[j] over rows[j] == r at the listed rows and is UNWRITTEN elsewhere.
    plan (`rowops.row_list_plan` of rows): summed in the plan's fixed order, without float atomics."""
    t = torch.empty(n, compact.shape[1], dtype=torch.float32, device=compact.device)
    if plan is not None:
        return rowops.scatter_rows_ordered(t, plan, compact, False)
    t.index_fill_(0, rows, 0.0)
    return t.index_add_(0, rows, compact)


def fused_last_hop(graph_t, fused, g, flags, count, addend, s, b_flags):
    """The backward product that lands on the table, A^T g + s * addend, with Adam applied in its epilogue: fused =
    (table, optimizer); no gradient tensor is written.  The step is committed after the launch, so a launch that fails
    leaves no mark on the optimizer."""
    table, opt = fused
    m, v, step = opt.fused_state(table)
    graph_t.spmm_axpy_adam(g, flags, count, addend, s, b_flags, table.data, m, v, opt.lr, opt.betas, opt.eps, step,
                           opt.fused_dev(table))
    opt.fused_commit(table)


def xavier_tables(num_list, dim, device):
    """xavier_uniform_ per table, in order, drawn from torch's CPU generator so a seeded run
    reproduces the reference's initial values (lightgcn.py:37-47)."""
    parts = []
    for n in num_list:
        t = torch.empty(n, dim)
        nn.init.xavier_uniform_(t)
        parts.append(t)
    return torch.cat(parts, dim=0).to(device)


class StepWorkspace:
    """The [N, D]-sized buffers of a model's restricted training step, owned by the model and reused from step to step: no
    allocator traffic inside the step (at the C5 shape the caching allocator held 298 GB reserved against a 180 GB peak),
    and fixed addresses for a captured HIP graph.  One step at a time: `acquire(token)` hands the buffers to a forward pass;
    they are free again when its backward pass has run (`release`) or its autograd context has been dropped (the token
    died).  A forward pass that finds them taken -- two losses alive at once -- allocates its own buffers as before."""

    def __init__(self):
        self._buf = {}
        self._owner = None

    def acquire(self, token):
        if self._owner is not None and self._owner() is not None:
            return False
        import weakref
        self._owner = weakref.ref(token)
        return True

    def release(self, token):
        if self._owner is not None and self._owner() is token:
            self._owner = None

    def get(self, name, shape, dtype, device):
        t = self._buf.get(name)
        if t is None or tuple(t.shape) != tuple(shape) or t.dtype != dtype or t.device != device:
            t = self._buf[name] = torch.empty(shape, dtype=dtype, device=device)
        return t

    def nbytes(self):
        return sum(t.numel() * t.element_size() for t in self._buf.values())

    def clear(self):
        """Give the buffers back to the allocator (they are re-created by the next restricted step): before a phase that
        needs the memory for something else -- an all-rows pass at the C5 shape holds six more [N, D] tensors.  Refused
        while a forward pass still owns them."""
        if self._owner is not None and self._owner() is not None:
            return False
        self._buf = {}
        return True


class _Token:
    pass


def step_buffer(ws, name, shape, dtype, device):
    """A workspace buffer when a workspace is in use, otherwise a fresh torch.empty."""
    return torch.empty(shape, dtype=dtype, device=device) if ws is None else ws.get(name, shape, dtype, device)


class TableModel(nn.Module):
    def _init_table(self, data, use_tag, dim, device):
        if torch.device(device).type != "cuda":
            raise _lib.TagrecError(f"{type(self).__name__}: tagrec_amd needs a GPU device (no CPU path)")
        _lib.load()
        self.num_list = [data.num["user"], data.num["item"]] + ([data.num["tag"]] if use_tag else [])
        self.table = nn.Parameter(xavier_tables(self.num_list, dim, device))
        self._offsets = [0]
        for n in self.num_list:
            self._offsets.append(self._offsets[-1] + n)
        self._eval_cache = None
        self._register_state_dict_hook(_split_table_hook)
        self._register_load_state_dict_pre_hook(_merge_table_hook, with_module=True)

    @property
    def embed(self):
        return [self.table[a:b] for a, b in zip(self._offsets[:-1], self._offsets[1:])]

    def get_ego_embed(self):
        return self.embed

    get_ego_emb = get_ego_embed          # ngcf.py:92 spells it without the final 'ed'

    def _split(self, out):
        return tuple(out[a:b] for a, b in zip(self._offsets[:-1], self._offsets[1:]))

    # -- the distance-correlation term of the disentangled models (DGCF, DisenGCN, DisenHAN; config key `cor_loss`)
    use_cor_loss = False

    def _loss_batch(self, batch_data):
        """`loss`'s argument, (triplets [B, 3], cor) or the triplets alone -> (triplets int64 on the device, cor).  cor
        ([node types, c] ids per node type, what DGCF_training_data draws) is None unless the model's `cor_loss` is on:
        with the term off that half of the batch is ignored, as in the reference."""
        pair = isinstance(batch_data, (tuple, list))
        data = (batch_data[0] if pair else batch_data).to(self.device, torch.int64).contiguous()
        if not self.use_cor_loss:
            return data, None
        cor = batch_data[1] if pair and len(batch_data) > 1 else None
        n_type = 3 if self.use_tag else 2
        if cor is None or len(cor) < n_type:
            raise _lib.TagrecError(f"{type(self).__name__}: cor_loss=True needs a (triplets, cor) batch with ids for "
                                   f"{n_type} node types (DGCF_training_data yields it)")
        return data, [cor[t].to(self.device, torch.int64) for t in range(n_type)]

    def _cor_rows(self, cor):
        """Node ids (with the type offsets) of the cor sample: rows a restricted forward pass must get right too."""
        return torch.cat([c + self._offsets[t] for t, c in enumerate(cor)])

    def _cor_term(self, all_embs, cor):
        """cor_reg * cor_loss of the propagated rows cor[0] of the users, cor[1] of the items (and cor[2] of the tags),
        stacked along dim 0 and split into factor_k column slices (the reference's commented-out block, dgcf.py:131-143)."""
        sample = torch.cat([all_embs[t][c] for t, c in enumerate(cor)], dim=0)
        return self.cor_reg * cor_loss(sample, self.factor_k)

    def train(self, mode=True):
        self._eval_cache = None          # parameters may change once training resumes
        return super().train(mode)

    def predict_rating(self, users):
        """sigmoid(U_b I^T).  The reference re-runs forward() for every 512-user batch
        (lightgcn.py:85).  In eval mode the propagated tables are computed once and reused until
        `train()` is called again (same values, fewer propagations); in training mode every call
        propagates, as the reference does."""
        if self.training or self._eval_cache is None:
            with torch.no_grad():
                all_users, all_items = self.forward()[:2]
            if not self.training:
                self._eval_cache = (all_users, all_items)
        else:
            all_users, all_items = self._eval_cache
        users = users.to(self.table.device)
        return torch.sigmoid(torch.matmul(all_users[users], all_items.t()))


class FusedStepModel(TableModel):
    """What LightGCN and NGCF share beyond the table: the hook `Adam.fuse_into(model)` looks for, and the per-step seed of
    the library's counter-based message dropout."""

    fused_capturable = True        # Adam(capturable=True).fuse_into(model): the fused update advances its counter on the device
    _drop_rates = list             # the container the rates are handed over in

    def set_fused_optimizer(self, opt):
        """`Adam.fuse_into(model)`: the compact restricted step applies the table's Adam update in the epilogue of the
        product that lands on it; every other path hands the optimizer a gradient as usual.  None switches it off."""
        self._fused_opt = opt

    def _check_drop_width(self):
        """Raise if the fused dropout kernels cannot serve this model's width."""

    def _drops(self):
        """(per-layer drop rates, seed of this forward pass) when message dropout is active, else (None, 0).  The
        seed advances with every training-mode forward pass; masks are functions of (seed, layer, element)."""
        drops = [float(p) for p in self.message_drop_list[:self.num_layer]]
        if not (self.training and any(p > 0 for p in drops)):
            return None, 0
        self._check_drop_width()
        if torch.cuda.is_current_stream_capturing():
            raise _lib.TagrecError(f"{type(self).__name__}: message dropout draws a new seed on the host every step and "
                                   "cannot be captured in a HIP graph")
        self._drop_calls = getattr(self, "_drop_calls", 0) + 1
        return (self._drop_rates(drops + [0.0] * (self.num_layer - len(drops))),
                (int(self.drop_seed) << 24) + self._drop_calls)


def _split_table_hook(module, state_dict, prefix, local_metadata):
    table = state_dict.pop(prefix + "table")
    for k, (a, b) in enumerate(zip(module._offsets[:-1], module._offsets[1:])):
        state_dict[f"{prefix}embed.{k}"] = table[a:b]
    # keep the reference's key order: embed.* first
    for key in [k for k in state_dict if k.startswith(prefix) and not k.startswith(prefix + "embed.")]:
        state_dict.move_to_end(key)
    return state_dict


def _merge_table_hook(module, state_dict, prefix, local_metadata, strict, missing_keys, unexpected_keys, error_msgs):
    keys = [f"{prefix}embed.{k}" for k in range(len(module.num_list))]
    module._eval_cache = None
    if all(k in state_dict for k in keys):
        state_dict[prefix + "table"] = torch.cat([state_dict.pop(k) for k in keys], dim=0)
