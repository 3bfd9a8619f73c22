"""DisenHAN behind the reference's model surface (/root/reference/model/disenhan.py).

    DisenHAN(data)            three tables (user, item, tag) + per layer Wtk [3, K, D, dk], at [6, K, 2 dk], W [dk, dk],
                              q_rela [6, dk]                                                              (:21-26, :146-157)
    .forward()                -> (user_emb, item_emb, tag_emb): the LAST layer's output                   (:159-179)
    .loss((batch[B,3], cor))  -> (mul_loss, reg * l2reg_loss on the PROPAGATED rows)                      (:181-214)
                              config cor_loss=True: + cor_reg * cor_loss of the propagated cor rows (:200-212, commented
                              out in the reference); off (the default) the cor half is ignored
    .predict_rating(users)    -> sigmoid(U_b I^T)                                                         (:216-222)

Layer (:28-97): ego_t = slice_normalize(leaky_0.2(emb_t Wtk[t])) -- one [D, D] GEMM per node type; then two routing
iterations (hard-coded: `iterate_k` is read but not used) over the six relations ui iu ut tu it ti.  Per relation the
attention splits into a row half and a column half (sL / sR, [n, K] on torch.matmul), the edge softmax, its product
A(alpha) ego_b (route_spmm, one weight per entry), the relation epilogue (Z, r) and the per-type combine run on the
kernels of csrc/disenhan.hip; nothing is detached, so gradients reach every parameter through both iterations and r.

The reference's user-tag / item-tag COO matrices hold one entry per (u, i, t) assignment; torch.sparse.softmax
coalesces them, so a merged entry of multiplicity m has m times the logit and appears once in the product
(`merged_relations`)."""
import numpy as np
import torch
import torch.nn as nn

from . import _lib, help as H
from . import routing as R
from .base import TableModel
from .config import _BASE
from .graph import Graph

RELATIONS = ("ui", "iu", "ut", "tu", "it", "ti")
INDEX = ((0, 1), (1, 0), (0, 2), (2, 0), (1, 2), (2, 1))      # (row type, column type) of each relation (:79)
COMBINE = ((0, 2), (1, 4), (3, 5))                              # relations added into user / item / tag (:91-93)
ITERATE = 2                                                     # Layer(K, D, D, 6, 2) (:157)

# utility/config.py:32-39
_DISENHAN = {"mul_loss_func": "softplus", "norm_type": "plain", "factor_k": 4, "iterate_k": 2, "cor_batch": 100,
             "cor_loss": False}


def disenhan_config(**overrides):
    """The reference's base configuration + its `_disenhan` dict (DisenHAN stays outside `get_config`'s scope list)."""
    cfg = dict(_BASE)
    cfg["model"] = "disenhan"
    cfg.update(_DISENHAN)
    cfg["device"] = torch.device("cuda" if torch.cuda.is_available() else "cpu")
    cfg.update(overrides)
    return cfg


def merged_relations(data):
    """The six relations ui iu ut tu it ti as merged CSR: (rowptr int64 [n_a + 1], col int32, mult int32, (n_a, n_b)),
    entries in row-major order (torch's coalesced order).  mult = how many entries of the reference's COO matrix hold
    the pair (a COO value carries a count: the blocks of the reference's loader hold ones).  Host tensors from the COO
    blocks of `data`; a dataset of the device generator (`data.rel`) is already merged and is only reordered."""
    nu, ni, nt = int(data.num["user"]), int(data.num["item"]), int(data.num["tag"])
    if getattr(data, "rel", None) is not None:
        size = {"u": nu, "i": ni, "t": nt}
        return [tuple(data.rel[e]) + ((size[e[0]], size[e[1]]),) for e in RELATIONS]
    out = []
    for c, na, nb in ((data.ui_adj, nu, ni), (data.ut_adj, nu, nt), (data.it_adj, ni, nt)):
        row = torch.from_numpy(np.asarray(c.row).astype(np.int64))
        col = torch.from_numpy(np.asarray(c.col).astype(np.int64))
        cnt = torch.from_numpy(np.rint(np.asarray(c.data)).astype(np.int64))
        for a, b, n_a, n_b in ((row, col, na, nb), (col, row, nb, na)):
            key, inv = torch.unique(a * n_b + b, return_inverse=True)
            mult = torch.zeros(key.numel(), dtype=torch.int64).index_add_(0, inv, cnt)
            r = torch.div(key, n_b, rounding_mode="floor")
            rowptr = torch.zeros(n_a + 1, dtype=torch.int64)
            torch.cumsum(torch.bincount(r, minlength=n_a), 0, out=rowptr[1:])
            out.append((rowptr, (key - r * n_b).to(torch.int32), mult.to(torch.int32), (n_a, n_b)))
    return out


class Relation:
    """One merged relation on the device: the routing structure (route_spmm / route_score, its transposed structure
    and permutation) + the entry multiplicities as fp32."""

    def __init__(self, rowptr, col, mult, shape, device):
        self.shape = (int(shape[0]), int(shape[1]))
        self.mult = mult.to(device=device, dtype=torch.float32).contiguous()
        g = Graph(rowptr.to(device=device, dtype=torch.int64).contiguous(), col.to(device=device, dtype=torch.int32).contiguous(),
                  self.mult, self.shape)
        self.rg = R.RoutingGraph(g)
        self.nnz = self.rg.nnz


class _EdgeSoftmax(torch.autograd.Function):
    """alpha = row softmax of mult * sum_k r relu(sL[row] + sR[col]) (disenhan.py:37-49)."""

    @staticmethod
    def forward(ctx, sL, sR, r, rel):
        sL, sR, r = sL.contiguous(), sR.contiguous(), r.contiguous()
        g = rel.rg.graph
        alpha = torch.empty(rel.nnz, dtype=torch.float32, device=sL.device)
        _lib.check(_lib.load().tagrec_dh_edge_softmax_fwd_f32(g.rowptr, g.col, rel.mult, rel.shape[0], sL, sR, r, sL.shape[1],
                                                              alpha, _lib.stream_ptr()), "dh_edge_softmax_fwd")
        ctx.rel = rel
        ctx.save_for_backward(sL, sR, r, alpha)
        return alpha

    @staticmethod
    def backward(ctx, dalpha):
        sL, sR, r, alpha = ctx.saved_tensors
        rel = ctx.rel
        return (*edge_softmax_bwd(rel, sL, sR, r, alpha, dalpha.contiguous()), None)


def edge_softmax_bwd(rel, sL, sR, r, alpha, dalpha):
    """(dsL, dsR, dr) of the edge softmax: a row pass and a column pass over the transposed structure."""
    g, gt = rel.rg.graph, rel.rg.graph_t
    K = sL.shape[1]
    scratch = torch.empty(rel.nnz, dtype=torch.float32, device=sL.device)
    dsL, dr = torch.empty_like(sL), torch.empty_like(r)
    dsR = torch.empty_like(sR)
    _lib.check(_lib.load().tagrec_dh_edge_softmax_bwd_f32(g.rowptr, g.col, rel.mult, rel.shape[0], gt.rowptr, gt.col, rel.rg.perm,
                                                          rel.shape[1], sL, sR, r, K, alpha, dalpha, scratch, dr, dsL, dsR,
                                                          _lib.stream_ptr()), "dh_edge_softmax_bwd")
    return dsL, dsR, dr


class _RelEpilogue(torch.autograd.Function):
    """(Z, r): Z = leaky_0.2(Y) W per factor slice, r = softmax_k <tanh(Z_k), q> (disenhan.py:51-59)."""

    @staticmethod
    def forward(ctx, Y, W, q, K):
        Y, W, q = Y.contiguous(), W.detach().contiguous(), q.detach().contiguous()
        n, D = Y.shape
        Yl, Z = torch.empty_like(Y), torch.empty_like(Y)
        r = torch.empty(n, K, dtype=torch.float32, device=Y.device)
        _lib.check(_lib.load().tagrec_dh_rel_epi_fwd_f32(Y, W, q, n, D, K, Yl, Z, r, _lib.stream_ptr()), "dh_rel_epi_fwd")
        ctx.K = K
        ctx.save_for_backward(Yl, Z, r, W, q)
        return Z, r

    @staticmethod
    def backward(ctx, dZ, dr):
        Yl, Z, r, W, q = ctx.saved_tensors
        n, D = Yl.shape
        K = ctx.K
        dk = D // K
        dZ = None if dZ is None else dZ.contiguous()
        dr = None if dr is None else dr.contiguous()
        dY, dZt, dsT = torch.empty_like(Yl), torch.empty_like(Yl), torch.empty_like(Yl)
        _lib.check(_lib.load().tagrec_dh_rel_epi_bwd_f32(Yl, Z, r, dZ, dr, W, q, n, D, K, dY, dZt, dsT, _lib.stream_ptr()),
                   "dh_rel_epi_bwd")
        dW = torch.matmul(Yl.view(-1, dk).t(), dZt.view(-1, dk))
        dq = dsT.view(-1, dk).sum(0)
        return dY, dW, dq, None


class _Combine(torch.autograd.Function):
    """slice_normalize(ego + r1 (.) Z1 + r2 (.) Z2) (disenhan.py:62-66)."""

    @staticmethod
    def forward(ctx, ego, Z1, r1, Z2, r2, K):
        ego, Z1, r1, Z2, r2 = (t.contiguous() for t in (ego, Z1, r1, Z2, r2))
        n, D = ego.shape
        x, y = torch.empty_like(ego), torch.empty_like(ego)
        inv = torch.empty(n, K, dtype=torch.float32, device=ego.device)
        _lib.check(_lib.load().tagrec_dh_combine_fwd_f32(ego, Z1, r1, Z2, r2, n, D, K, x, y, inv, _lib.stream_ptr()),
                   "dh_combine_fwd")
        ctx.K = K
        ctx.save_for_backward(x, inv, Z1, r1, Z2, r2)
        return y

    @staticmethod
    def backward(ctx, dy):
        x, inv, Z1, r1, Z2, r2 = ctx.saved_tensors
        n, D = x.shape
        dy = dy.contiguous()
        dx, dZ1, dZ2 = torch.empty_like(x), torch.empty_like(x), torch.empty_like(x)
        dr1, dr2 = torch.empty_like(r1), torch.empty_like(r2)
        _lib.check(_lib.load().tagrec_dh_combine_bwd_f32(x, inv, dy, Z1, r1, Z2, r2, n, D, ctx.K, dx, dZ1, dZ2, dr1, dr2,
                                                         _lib.stream_ptr()), "dh_combine_bwd")
        return dx, dZ1, dr1, dZ2, dr2, None


def edge_softmax(sL, sR, r, rel):
    return _EdgeSoftmax.apply(sL, sR, r, rel)


def rel_epilogue(Y, W, q, K):
    return _RelEpilogue.apply(Y, W, q, K)


def combine(ego, Z1, r1, Z2, r2, K):
    return _Combine.apply(ego, Z1, r1, Z2, r2, K)


def _half_scores(x, a, K):
    """[n, K] scores <x[i]_k, a[k]> for a [K, dk]: x times the block-diagonal [D, K] matrix of a's rows."""
    return torch.matmul(x, torch.block_diag(*a.unsqueeze(-1)))


class Layer(nn.Module):
    def __init__(self, factor_k, dim_in, dim_out):
        super().__init__()
        self.factor_k, self.dim_in, self.dim_out = factor_k, dim_in, dim_out
        dim_k = dim_out // factor_k
        self.Wtk = nn.Parameter(torch.empty(3, factor_k, dim_in, dim_k))
        self.at = nn.Parameter(torch.empty(6, factor_k, 2 * dim_k))
        self.W = nn.Parameter(torch.empty(dim_k, dim_k))
        self.q_rela = nn.Parameter(torch.empty(6, dim_k))

    def forward(self, rels, embs):
        K, D = self.factor_k, self.dim_out
        dk = D // K
        ego = []
        for t in range(3):                                                      # fac (:29-34)
            w = self.Wtk[t].permute(1, 0, 2).reshape(self.dim_in, D)
            ego.append(R.slice_normalize(torch.nn.functional.leaky_relu(torch.matmul(embs[t], w), 0.2), K))
        sR = [_half_scores(ego[b], self.at[e, :, dk:], K) for e, (_, b) in enumerate(INDEX)]
        r = [torch.full((rels[e].shape[0], K), 1.0 / K, dtype=torch.float32, device=ego[0].device) for e in range(6)]
        new = ego
        for _ in range(ITERATE):
            outs = []
            for e, (a, b) in enumerate(INDEX):
                alpha = edge_softmax(_half_scores(new[a], self.at[e, :, :dk], K), sR[e], r[e], rels[e])
                Y = R.valued_spmm(alpha, ego[b], rels[e].rg)
                outs.append(rel_epilogue(Y, self.W, self.q_rela[e], K))
            new = [combine(ego[t], *outs[COMBINE[t][0]], *outs[COMBINE[t][1]], K) for t in range(3)]
            r = [o[1] for o in outs]
        return new


class DisenHAN(TableModel):
    def __init__(self, data, args=None, config=None):
        super().__init__()
        self._config(config if config is not None else disenhan_config())
        self._init_table(data, True, self.dim_latent, self.device)         # embed.0-2, xavier in order (:146-155)
        self.rels = [Relation(*rel, device=self.device) for rel in merged_relations(data)]
        self.layer = nn.ModuleList(Layer(self.factor_k, self.dim_latent, self.dim_latent) for _ in range(self.num_layer))
        for lyr in self.layer:
            for p in lyr.parameters():                                          # Wtk, at, W, q_rela per layer, in order
                nn.init.xavier_uniform_(p)
        self.layer.to(self.device)

    def _config(self, config):
        _lib.refuse_deterministic(config, "DisenHAN", "the backward of its torch gathers sums repeated batch rows with float atomics")
        _lib.refuse_multi_negative(config, "DisenHAN")
        _lib.refuse_ultragcn(config, "DisenHAN")
        self.dim_latent = config["dim_latent"]
        self.num_layer = len(config["dim_layer_list"])
        self.device = torch.device(config["device"])
        self.norm_type = config["norm_type"]
        self.factor_k = config["factor_k"]
        self.iterate_k = config["iterate_k"]                                   # read but not used, as in the reference
        self.dim_k = self.dim_latent // self.factor_k
        self.reg = config["reg"]
        self.cor_reg = config["cor_reg"]
        self.use_cor_loss = bool(config.get("cor_loss", False))
        self.loss_func = config["mul_loss_func"]
        self.use_tag = config["use_tag"]
        self.message_drop_list = config["message_drop_list"]

    def forward(self):
        x = list(self._split(self.table))
        for lyr in self.layer:
            x = lyr(self.rels, x)
        return tuple(x)

    def loss(self, batch_data):
        data, cor = self._loss_batch(batch_data)
        all_embs = self.forward()
        all_users, all_items = all_embs[:2]
        loss, reg_loss = H.triplet_loss(all_users, all_items, all_users, all_items, data, self.loss_func)
        if cor is None:
            return loss, self.reg * reg_loss
        return loss, self.reg * reg_loss, self._cor_term(all_embs, cor)
