"""NCL: LightGCN plus two neighbourhood contrasts (Lin et al., "Improving Graph Collaborative Filtering with
Neighborhood-enriched Contrastive Learning", WWW 2022).  Not in the reference; the surface is LightGCN's.

    NCL(data)               LightGCN's constructor; config keys ncl_struct_rate, ncl_proto_rate, ncl_alpha, ncl_temperature,
                            ncl_clusters, ncl_kmeans_iters, ncl_warm_up (config.check_ncl)
    .forward() / .predict_rating() / .state_dict()     inherited
    .loss(batch)            -> (mul_loss, reg * l2reg, ncl_struct_rate * L_struct, ncl_proto_rate * L_proto); the first two
                            ARE LightGCN.loss(batch), for every batch form
    .e_step()               re-cluster the user and the item ego tables (kmeans.py) into the model's centroid / cluster buffers
    .begin_epoch(ep)        what Basic_train.run calls before an epoch's phases: e_step() from epoch ncl_warm_up on

The two terms read columns 0 and 1 of the batch, (u_b, i_b), repeats kept, and are MEANS over the batch (`help.
ncl_structure_loss`, `help.ncl_prototype_loss` have the formulas); the paper's code sums, so its weights are ours divided by
B.  The structure term contrasts a node's raw two-hop product A (A x0) with the ego rows of its own side (hyper_layers = 1);
the prototype term contrasts a node's ego row with the k-means centroids of its side, and is an exact 0 until the first
e_step().  In eval mode, or with a zero rate, a term launches nothing and is an exact 0.

The centroids are constants of a step (the M-step of the paper's EM view): e_step() runs under no-grad on the detached raw
ego rows, with a seed derived from (config seed, e-step counter, side), and copies the ROW-NORMALISED centroids and the int64
cluster ids into buffers that keep their identity.  The buffers are plain attributes, not part of state_dict(): a restored
model re-clusters at its next epoch.

Each term is its own autograd node on the table and autograd adds the gradients, so `Adam.fuse_into` is refused (as for
SimGCL), and so is a stream capture of loss(): the prototype term switches on mid-run.  deterministic=True is supported:
every fold of repeated rows then runs through a `rowops.row_list_plan`."""
import torch

from . import _lib, help as H
from .config import check_ncl
from .graph import Graph
from .kmeans import kmeans
from .lightgcn import LightGCN
from .rowops import rownorm_fwd


class NCL(LightGCN):
    def __init__(self, data, args=None, config=None, graph=None):
        super().__init__(data, args, config, graph)
        name = type(self).__name__
        if self.split_adj_k > 1 or not isinstance(self.norm_adj, Graph):
            raise _lib.TagrecError(f"{name}: the two-hop view runs on one Graph, not on row folds (split_adj_k > 1)")
        if self.num_layer < 2:
            raise _lib.TagrecError(f"{name}: the structure term contrasts a node with its two-hop view: it needs at least 2 "
                                   f"layers (dim_layer_list), got {self.num_layer}")
        D = self.dim_latent
        if D < 8 or D > 256 or D % 4 != 0:
            raise _lib.TagrecError(f"{name}: the softmax and assignment kernels need dim_latent a multiple of 4 in 8 .. 256, got {D}")
        if any(float(p) != 0 for p in self.message_drop_list) or float(self.node_drop) != 0:
            raise _lib.TagrecError(f"{name}: message_drop_list / node_drop must be zero (the two-hop view is the model's graph as it is)")
        nu, ni = self.num_list[0], self.num_list[1]
        if self.ncl_clusters > min(nu, ni):
            raise _lib.TagrecError(f"{name}: ncl_clusters = {self.ncl_clusters} exceeds the smaller node table "
                                   f"(n_user = {nu}, n_item = {ni})")
        dev, K = self.table.device, self.ncl_clusters
        # what e_step() fills, in place: unit centroid rows and cluster ids per side
        self.cent_u = torch.zeros(K, D, dtype=torch.float32, device=dev)
        self.cent_i = torch.zeros(K, D, dtype=torch.float32, device=dev)
        self.cluster_u = torch.zeros(nu, dtype=torch.int64, device=dev)
        self.cluster_i = torch.zeros(ni, dtype=torch.int64, device=dev)
        self.e_steps = 0                  # finished e_step() calls; the prototype term is off at 0

    def _config(self, config):
        super()._config(config)
        (self.ncl_struct_rate, self.ncl_proto_rate, self.ncl_alpha, self.ncl_temperature, self.ncl_clusters,
         self.ncl_kmeans_iters, self.ncl_warm_up) = check_ncl(config)

    def set_fused_optimizer(self, opt):
        if opt is not None:
            raise _lib.TagrecError("NCL: Adam.fuse_into is not covered -- the table receives several gradients (the ranking "
                                   "loss and the contrast terms), and the update in the epilogue would apply the first one alone")
        super().set_fused_optimizer(None)

    def kmeans_seed(self, side):
        """Seed of the coming e-step's k-means of one side (0 users, 1 items): a function of (config seed, e-step counter, side)."""
        return ((int(self.drop_seed) << 24) + 2 * self.e_steps + side) & ((1 << 62) - 1)

    @torch.no_grad()
    def e_step(self):
        nu, ni = self.num_list[0], self.num_list[1]
        x0 = self.table.detach()
        for side, (rows, cent, cluster) in enumerate(((x0[:nu], self.cent_u, self.cluster_u),
                                                      (x0[nu:nu + ni], self.cent_i, self.cluster_i))):
            c, assign, _, _ = kmeans(rows, self.ncl_clusters, self.ncl_kmeans_iters, self.kmeans_seed(side))
            rownorm_fwd(c, cent)
            cluster.copy_(assign)
        self.e_steps += 1

    def begin_epoch(self, ep):
        if ep >= self.ncl_warm_up and (self.ncl_struct_rate > 0 or self.ncl_proto_rate > 0):
            self.e_step()

    def struct_loss(self, batch_data):
        nu, ni = self.num_list[0], self.num_list[1]
        return H.ncl_structure_loss(self.table, self.norm_adj, nu, ni, batch_data, self.ncl_temperature, self.ncl_alpha,
                                    self.deterministic)

    def proto_loss(self, batch_data):
        nu, ni = self.num_list[0], self.num_list[1]
        return H.ncl_prototype_loss(self.table, nu, ni, batch_data, self.cent_u, self.cent_i, self.cluster_u, self.cluster_i,
                                    self.ncl_temperature, self.ncl_alpha, self.deterministic)

    def loss(self, batch_data):
        batch_data = batch_data.to(self.device, torch.int64).contiguous()
        want_s = self.training and self.ncl_struct_rate != 0
        want_p = self.training and self.ncl_proto_rate != 0
        if (want_s or want_p) and torch.cuda.is_current_stream_capturing():      # (first: refused before any launch)
            raise _lib.TagrecError("NCL: loss() cannot be captured in a HIP graph -- the prototype term switches on at the "
                                   "first e_step(), so one captured step does not stand for the run")
        parts = super().loss(batch_data)
        zero = torch.zeros((), dtype=torch.float32, device=self.table.device)
        l_s = self.ncl_struct_rate * self.struct_loss(batch_data) if want_s else zero
        l_p = self.ncl_proto_rate * self.proto_loss(batch_data) if (want_p and self.e_steps > 0) else zero
        return parts[0], parts[1], l_s, l_p
