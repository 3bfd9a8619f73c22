"""UltraGCN: collaborative filtering without message passing (Mao et al., "UltraGCN: Ultra Simplification of Graph
Convolutional Networks for Recommendation", CIKM 2021).  Not in the reference.

    UltraGCN(data)          config keys ug_w, ug_negative_weight, ug_lambda, ug_neighbors, ug_zero_diagonal (config.check_ultragcn)
    .forward()              -> (user table, item table): the ego tables, there is no propagation
    .loss(batch[B, 2 + K])  -> (mul_loss, reg * l2reg_loss); batch = (user, positive, K = n_negatives negatives)
    .predict_rating(users) / .state_dict()     TableModel's, so Basic_test's fused evaluation works as for every table model

The objective is `help.ultragcn_loss` (its docstring has the formula): a degree-weighted binary cross-entropy that scores the
positive, the K sampled negatives and -- the item-item constraint -- the ug_neighbors items that co-occur most with the
positive, every slot on its own (`rowops.wbce_fwd` / `wbce_bwd` through the `Ultra` stage of loss_stage.py).  The degrees, the
beta weights and the neighbour tables (`cooc.item_cooccurrence_topk`: the sparse A^T A row by row, exact) are built once at
construction from the train edges.  The terms are MEANS over the batch where the paper's code sums, and the L2 term is on the
batch's rows (user, positive, negatives), not on the whole tables.  ug_neighbors = 0 turns the neighbour term off.

Nothing in loss() reads the host.  deterministic=True folds the compact gradients through `help.ultragcn_plans` (the same bits
every run).  `Adam.fuse_into` is refused: there is no backward product whose epilogue could take the update.

`RowAdam.attach(model)` (train.py) makes the step row-sparse: a training-mode loss() catches the batch's rows up to the
optimizer's step and its backward hands the optimizer (plan, compact gradient) instead of a table-sized gradient.  Rows a
batch did not name then LAG behind the dense optimizer until they are next read; forward(), predict_rating(), get_ego_embed(),
state_dict() and eval() flush them first.  `model.table.data` read directly between steps is not flushed."""
import numpy as np
import torch

from . import _lib, help as H, loss_stage as S
from .base import TableModel
from .config import CFG as _GLOBAL_CFG, check_ranking, check_ultragcn


class UltraGCN(TableModel):
    def __init__(self, data, args=None, config=None):
        super().__init__()
        self._config(config if config is not None else _GLOBAL_CFG)
        self._init_table(data, False, self.dim_latent, self.device)
        nu, ni = self.num_list
        ui = data.user_items.get("train")
        if ui:
            edges = np.array([(u, i) for u, items in ui.items() for i in items], dtype=np.int64).reshape(-1, 2)
        else:                             # a device-generated dataset (synth.make_bipartite_device) keeps the edge list only
            edges = data.edge_index["train"]
        self.tables = H.ultragcn_tables(edges, nu, ni, self.device, self.ug_neighbors, self.ug_zero_diagonal, self.ug_w,
                                        self.ug_negative_weight, self.ug_lambda)

    def _config(self, config):
        name = type(self).__name__
        if config.get("model") != "ultragcn":
            raise _lib.TagrecError(f"{name}: needs get_config(\"ultragcn\"), got the {config.get('model')!r} configuration")
        self.ug_w, self.ug_negative_weight, self.ug_lambda, self.ug_neighbors, self.ug_zero_diagonal = check_ultragcn(config)
        self.n_negatives = check_ranking(config)[0]
        if config.get("use_tag", False):
            raise _lib.TagrecError(f"{name}: use_tag=True is not covered (user and item tables only)")
        if config.get("split_adj_k", 1) != 1:
            raise _lib.TagrecError(f"{name}: row folds (split_adj_k > 1) are not covered: there is no adjacency to fold")
        if config.get("catalogue_mask", "none") != "none":
            raise _lib.TagrecError(f"{name}: catalogue_mask masks a softmax over the catalogue; this loss has none")
        self.dim_latent = config["dim_latent"]
        self.device = torch.device(config["device"])
        self.reg = config["reg"]
        self.use_tag = False
        self.deterministic = bool(config.get("deterministic", False))

    def set_fused_optimizer(self, opt):
        if opt is not None:
            raise _lib.TagrecError("UltraGCN: Adam.fuse_into is not covered -- the step has no backward product whose epilogue "
                                   "could apply the update")

    def set_row_optimizer(self, opt):
        """`RowAdam.attach(model)`: a training-mode loss() catches the batch's rows up to the optimizer's step, and its
        backward hands the optimizer (plan, compact gradient) in place of a table-sized gradient.  Between steps the rows a
        batch did not name LAG behind the dense optimizer; every reader below flushes them first.  None switches it off."""
        old = getattr(self, "_row_opt", None)
        if old is not None and old is not opt:
            old.flush()
        self._row_opt = opt

    def _row_optimizer(self):
        from .train import row_optimizer
        return row_optimizer(self)

    def _flush_rows(self):
        opt = self._row_optimizer()
        if opt is not None:
            opt.flush()
        return opt

    def forward(self):
        self._flush_rows()
        return tuple(self.embed)

    def get_ego_embed(self):
        self._flush_rows()
        return self.embed

    get_ego_emb = get_ego_embed

    def predict_rating(self, users):
        self._flush_rows()
        return super().predict_rating(users)

    def state_dict(self, *args, **kwargs):
        self._flush_rows()
        return super().state_dict(*args, **kwargs)

    def train(self, mode=True):
        if not mode:
            self._flush_rows()
        return super().train(mode)

    def loss(self, batch_data):
        batch = batch_data.to(self.device, torch.int64).contiguous()
        name = type(self).__name__
        if batch.dim() != 2 or batch.shape[1] != 2 + self.n_negatives:
            raise _lib.TagrecError(f"{name}: a batch of shape {tuple(batch.shape)} does not fit n_negatives={self.n_negatives} "
                                   f"(expected [B, {2 + self.n_negatives}] = user, positive, {self.n_negatives} negative(s))")
        nu, ni = self.num_list
        stage = S.Ultra(self.tables)         # one per step: the plans and the loss share its slot ids
        opt = self._flush_rows() if not self.training else self._row_optimizer()
        if opt is not None and self.training:            # row-sparse step: ONE plan over the stage's rows, no table gradient
            mul, l2 = H.ultragcn_row_loss(self.table, nu, batch, self.tables, opt, stage)
            return mul, self.reg * l2
        U, I = self.embed
        plans = H.ultragcn_plans(batch, self.tables, nu, ni, self.dim_latent, stage) if self.deterministic else None
        mul, l2 = H.ultragcn_loss(U, I, U, I, batch, self.tables, plans, stage)
        return mul, self.reg * l2
