"""DirectAU: LightGCN trained by alignment and uniformity on the unit sphere (Wang et al., "Towards Representation Alignment
and Uniformity in Collaborative Filtering", KDD 2022).  Not in the reference; the surface is LightGCN's.

    DirectAU(data)          LightGCN's constructor; config keys au_gamma, au_t (config.check_alignment)
    .forward() / .predict_rating() / .state_dict()     inherited
    .loss(batch[B, 2])      -> (mul_loss, reg * l2reg_loss on EGO rows); batch = (user, positive), nothing is sampled
    .last_au_parts          device tensor [align, unif_u, unif_i] of the latest loss() (no host read)

With U / I the propagated rows of the batch's users / positives (repeated ids kept, as in the paper's code) and
x^ = x / max(|x|, 1e-12):

    align    = (1 / B) sum_b |U^_b - I^_b|^2
    unif(X)  = log( 2 / (B (B - 1)) sum_{i < j} exp(-au_t |x^_i - x^_j|^2) )
    mul_loss = align + au_gamma (unif(U) + unif(I)) / 2

The loss stage is `rowops.directau_fwd` / `directau_bwd` (csrc/directau.hip: the B x B potentials are never stored, no float
atomics), wrapped as the `Au` stage of loss_stage.py: `_route` returns an `help.AuRoute`, `help.stage_for` turns it into the
stage, and LightGCN's own autograd node (`lightgcn._PropagateBprLoss`) runs its one forward and backward around it as around
any other stage.  So everything around the loss is LightGCN's: the compact restricted step and the
all-rows path, deterministic=True, Adam.fuse_into, GraphedStep replay, the step workspace, message dropout and both
edge-dropout modes.  Batches come from `BPR_training_data` with config["pair_batches"] = True (the "directau" default)."""
from . import _lib, help as H
from .config import check_alignment
from .lightgcn import LightGCN


class DirectAU(LightGCN):
    def __init__(self, data, args=None, config=None, graph=None):
        super().__init__(data, args, config, graph)
        self.last_au_parts = None

    def _config(self, config):
        super()._config(config)
        name = type(self).__name__
        if self.n_negatives != 1:
            raise _lib.TagrecError(f"{name}: the alignment / uniformity loss takes no negatives: it needs n_negatives=1 (the "
                                   f"default, unused), got {self.n_negatives!r}")
        if self.in_batch:
            raise _lib.TagrecError(f"{name}: the alignment / uniformity loss takes no negatives: it needs negatives=\"sampled\" "
                                   "(the default, unused), got \"in_batch\"")
        if self.over_catalogue:
            raise _lib.TagrecError(f"{name}: the alignment / uniformity loss is its own objective: it needs softmax_over=\"negatives\" "
                                   "(the default, unused), got \"catalogue\"")
        self.au_gamma, self.au_t = check_alignment(config)

    def _route(self, batch_data):
        return H.au_route(type(self).__name__, batch_data, self.au_t, self.au_gamma)
