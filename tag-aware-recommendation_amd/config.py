"""Run configuration with the reference's defaults.

The reference parses sys.argv at import time into a module-global dict
(/root/reference/utility/word.py:7, utility/utils.py:18-62) and merges a per-model
dict (utility/config.py:1-81).  Here `get_config(model, **overrides)` builds the
same dict explicitly; `CFG` is the process-wide default the models read when no
config is passed, exactly as the reference's models read `utility.word.CFG`.
"""
import torch

_BASE = {
    "model": "lightgcn", "dataset": "synthetic",
    "train_batch": 512, "test_batch": 512, "has_val": False, "use_tag": True,
    "patient_epoch": 10, "test_interval": 5, "early_stop_key": "ndcg",
    "topks": [10, 20], "lr": 0.01, "reg": 0.0, "cor_reg": 0.0,
    "epochs": 1000, "dim_latent": 64, "dim_layer_list": [64, 32, 16],
    "message_drop_list": [0.0, 0.0, 0.0], "node_drop": 0.0,
    "node_drop_mode": "rebuild",   # "kernel": edge dropout evaluated inside the products (help.node_drop), no CSR rebuilt per step
    "seed": 2020, "cpu_core": 4, "split_adj_k": 1,
    "hip_graph": False,       # Basic_train: replay each phase's step as one captured HIP graph (train.GraphedStep)
    "deterministic": False,   # LightGCN / NGCF: fold batch gradients in a fixed order (rowops.scatter_rows_ordered), no float atomics
    "all_gather": "collective",   # row-sharded models (dist.py): "direct" = one grouped send / receive pair per peer
    # negative sampler of the BPR producers (train_data.py; the reference has the uniform proposal and one draw only)
    "neg_sampling": "uniform",    # "popularity": proposal proportional to (distinct train users of the item) ** neg_pop_alpha
    "neg_pop_alpha": 0.75,
    "neg_candidates": 1,          # > 1: draw that many candidates, keep the one the current model scores highest
    # multi-negative ranking losses (rowops.rank_fwd / rank_bwd; LightGCN, NGCF and BPR_training_data; the reference has K = 1)
    "n_negatives": 1,             # K negatives per positive: batches are [B, 2 + K]
    "loss_temperature": 1.0,      # tau of mul_loss_func = "softmax" (not read by the other kinds)
    # where a positive's negatives come from (LightGCN, NGCF and BPR_training_data)
    "negatives": "sampled",       # "in_batch": the other positives of the batch (rowops.inbatch_*); batches are [B, 2], nothing is sampled
    "in_batch_logq": False,       # in-batch: subtract log(train degree of the item / train edges) from every column's logit
    # what the "softmax" loss normalises over (LightGCN, NGCF and BPR_training_data)
    "softmax_over": "negatives",  # "catalogue": every item (rowops.catsoftmax_*); batches are [B, 2], nothing is sampled
    # softmax_over="catalogue" only: which columns leave a row's softmax (LightGCN, NGCF; SimGCL's ranking part)
    "catalogue_mask": "none",     # "train_positives": the user's OTHER train items (help.user_positives_csr), as at evaluation
    # BPR_training_data: produce [E, 2] = (user, positive) epoch arrays without launching the sampler (the in-batch branch)
    # for objectives that take no negatives (DirectAU); the other producers do not read it
    "pair_batches": False,
}
NEG_SAMPLING_MODES = ("uniform", "popularity")
MAX_NEG_CANDIDATES = 16
MUL_LOSS_FUNCS = ("softplus", "logsigmoid", "softmax")
NEGATIVES_MODES = ("sampled", "in_batch")
SOFTMAX_OVER = ("negatives", "catalogue")
CATALOGUE_MASKS = ("none", "train_positives")
MAX_NEGATIVES = 63                # the kernel keeps the K + 1 scores of a tuple one per lane of a 64-lane wavefront

# utility/config.py:1-12, 41-52
_PER_MODEL = {
    "ngcf": {"norm_type": "ngcf", "agg_type": "bi_agg", "mul_loss_func": "logsigmoid"},
    "lightgcn": {"mul_loss_func": "softplus", "norm_type": "bi_norm", "cor_batch": 100},
    "tgcn": {"dim_weight": 10, "dim_atten": 32, "num_bit_conv": 32, "num_vec_conv": 8, "margin": 1,
             "transtag_batch": 512, "neighbor_k": 25, "transtag_reg": 0.0001, "mul_loss_func": "logsigmoid"},
    # utility/config.py:14-30
    # cor_loss (not in the reference, whose models leave the term commented out): add cor_reg * help.cor_loss on the batch's cor rows
    "dgcf": {"mul_loss_func": "softplus", "norm_type": "plain", "factor_k": 4, "iterate_k": 2, "cor_batch": 100, "cor_loss": False},
    "disengcn": {"mul_loss_func": "softplus", "norm_type": "plain", "factor_k": 4, "iterate_k": 2, "cor_batch": 100,
                 "cor_loss": False},
    # utility/config.py:54-61 -- note the default agg_type "bi_agg" switches KGAT's propagation off (kgat.py:100)
    "kgat": {"dim_relation": 64, "transe_reg": 0.0001, "transe_batch": 1024, "agg_type": "bi_agg", "mul_loss_func": "softplus"},
    # SimGCL (not in the reference): LightGCN plus an InfoNCE term between two noise-perturbed views of the batch's nodes
    # (simgcl.py); cl_rate weighs the term, cl_eps is the length of the per-layer perturbation, cl_temperature its tau
    "simgcl": {"mul_loss_func": "softplus", "norm_type": "bi_norm", "cor_batch": 100,
               "cl_rate": 0.5, "cl_eps": 0.1, "cl_temperature": 0.2, "use_tag": False},
    # DirectAU (not in the reference; Wang et al., KDD 2022): LightGCN trained by alignment of the positive pairs plus au_gamma
    # times the uniformity of the batch's users and items on the unit sphere, Gaussian potential exp(-au_t |x - y|^2)
    # (directau.py, rowops.directau_*); batches are [B, 2], nothing is sampled
    "directau": {"mul_loss_func": "softplus", "norm_type": "bi_norm", "cor_batch": 100,
                 "au_gamma": 1.0, "au_t": 2.0, "use_tag": False, "pair_batches": True},
    # NCL (not in the reference; Lin et al., WWW 2022): LightGCN plus a structure contrast (a node against its two-hop view)
    # and a prototype contrast (a node against the k-means centroid of its cluster, re-clustered every epoch from
    # ncl_warm_up on) (ncl.py, kmeans.py, rowops.kmeans_assign / catsoftmax_*).  The terms are MEANS over the batch; the
    # defaults are untuned and no accuracy run exists
    "ncl": {"mul_loss_func": "softplus", "norm_type": "bi_norm", "cor_batch": 100, "use_tag": False,
            "ncl_struct_rate": 5e-4, "ncl_proto_rate": 3e-4, "ncl_alpha": 1.0, "ncl_temperature": 0.1,
            "ncl_clusters": 1000, "ncl_kmeans_iters": 20, "ncl_warm_up": 20},
    # UltraGCN (not in the reference; Mao et al., CIKM 2021): no propagation -- plain user / item tables under a degree-weighted
    # pointwise BCE plus a constraint that pulls a user towards the ug_neighbors items that co-occur most with the positive
    # (ultragcn.py, cooc.py, rowops.wbce_*).  The terms are MEANS over the batch; the defaults are untuned and no accuracy run exists
    "ultragcn": {"mul_loss_func": "softplus", "use_tag": False, "n_negatives": 16,
                 "ug_w": (1e-6, 1.0, 1e-6, 1.0), "ug_negative_weight": 10.0, "ug_lambda": 1.0, "ug_neighbors": 10,
                 "ug_zero_diagonal": False},
}
MAX_AU_T = 20.0                   # a term of the uniformity sum is >= e^(-4 au_t): e^-80 is still a normal fp32 number
MAX_UG_NEIGHBORS = 64             # cooc.item_cooccurrence_topk keeps at most 64 neighbours per item


def get_config(model="lightgcn", **overrides):
    if model not in _PER_MODEL:
        raise KeyError(f"model {model!r} is outside the hot-path scope (have {sorted(_PER_MODEL)})")
    cfg = dict(_BASE)
    cfg["model"] = model
    cfg.update(_PER_MODEL[model])
    cfg["device"] = torch.device("cuda" if torch.cuda.is_available() else "cpu")
    cfg.update(overrides)
    check_neg_sampling(cfg)
    check_ranking(cfg)
    check_negatives(cfg)
    check_softmax_over(cfg)
    check_catalogue_mask(cfg)
    if model == "simgcl":
        check_contrastive(cfg)
    if model == "directau":
        check_alignment(cfg)
    if model == "ncl":
        check_ncl(cfg)
    if model == "ultragcn":
        check_ultragcn(cfg)
    else:
        from ._lib import refuse_ultragcn
        refuse_ultragcn(cfg, f"get_config({model!r})")
    return cfg


def check_neg_sampling(cfg):
    """The three sampler keys of a config -> (mode, alpha, candidates); an unknown value is refused."""
    from ._lib import TagrecError
    mode, alpha, cand = cfg.get("neg_sampling", "uniform"), cfg.get("neg_pop_alpha", 0.75), cfg.get("neg_candidates", 1)
    if mode not in NEG_SAMPLING_MODES:
        raise TagrecError(f"unknown neg_sampling {mode!r} (have {NEG_SAMPLING_MODES})")
    if isinstance(cand, bool) or not isinstance(cand, int) or not 1 <= cand <= MAX_NEG_CANDIDATES:
        raise TagrecError(f"neg_candidates must be an integer in 1 .. {MAX_NEG_CANDIDATES}, got {cand!r}")
    if isinstance(alpha, bool) or not isinstance(alpha, (int, float)) or not alpha == alpha or abs(alpha) == float("inf"):
        raise TagrecError(f"neg_pop_alpha must be a finite number, got {alpha!r}")
    return mode, float(alpha), cand


def check_ranking(cfg):
    """The three loss keys of a config -> (n_negatives, mul_loss_func, loss_temperature); a bad value is refused."""
    from ._lib import TagrecError
    k, loss, tau = cfg.get("n_negatives", 1), cfg.get("mul_loss_func", "softplus"), cfg.get("loss_temperature", 1.0)
    if isinstance(k, bool) or not isinstance(k, int) or not 1 <= k <= MAX_NEGATIVES:
        raise TagrecError(f"n_negatives must be an integer in 1 .. {MAX_NEGATIVES}, got {k!r}")
    if loss not in MUL_LOSS_FUNCS:
        raise TagrecError(f"unknown mul_loss_func {loss!r} (have {MUL_LOSS_FUNCS})")
    if isinstance(tau, bool) or not isinstance(tau, (int, float)) or not 0 < tau < float("inf"):
        raise TagrecError(f"loss_temperature must be a finite number > 0, got {tau!r}")
    return k, loss, float(tau)


def check_negatives(cfg):
    """The two in-batch keys of a config -> (in_batch, in_batch_logq); an unknown value, and negatives="in_batch" with anything
    but mul_loss_func="softmax" and n_negatives=1 (in-batch and sampled negatives are not mixed), is refused."""
    from ._lib import TagrecError
    neg, logq = cfg.get("negatives", "sampled"), cfg.get("in_batch_logq", False)
    if neg not in NEGATIVES_MODES:
        raise TagrecError(f"unknown negatives {neg!r} (have {NEGATIVES_MODES})")
    if not isinstance(logq, bool):
        raise TagrecError(f"in_batch_logq must be True or False, got {logq!r}")
    if neg == "in_batch":
        k, loss = cfg.get("n_negatives", 1), cfg.get("mul_loss_func", "softplus")
        if loss != "softmax":
            raise TagrecError(f"negatives=\"in_batch\" is a softmax over the batch: it needs mul_loss_func=\"softmax\", got {loss!r}")
        if k != 1:
            raise TagrecError(f"negatives=\"in_batch\" samples nothing: it needs n_negatives=1, got {k!r}")
    elif logq:
        raise TagrecError("in_batch_logq=True corrects in-batch negatives: it needs negatives=\"in_batch\"")
    return neg == "in_batch", logq


def check_softmax_over(cfg):
    """The softmax_over key of a config -> whether the softmax runs over the whole catalogue; an unknown value, and "catalogue"
    with anything but mul_loss_func="softmax", n_negatives=1 and negatives="sampled" (it samples nothing and is not mixed with
    in-batch negatives), is refused."""
    from ._lib import TagrecError
    over = cfg.get("softmax_over", "negatives")
    if over not in SOFTMAX_OVER:
        raise TagrecError(f"unknown softmax_over {over!r} (have {SOFTMAX_OVER})")
    if over == "catalogue":
        k, loss, neg = cfg.get("n_negatives", 1), cfg.get("mul_loss_func", "softplus"), cfg.get("negatives", "sampled")
        if loss != "softmax":
            raise TagrecError(f"softmax_over=\"catalogue\" is a softmax over every item: it needs mul_loss_func=\"softmax\", got {loss!r}")
        if k != 1:
            raise TagrecError(f"softmax_over=\"catalogue\" samples nothing: it needs n_negatives=1, got {k!r}")
        if neg != "sampled":
            raise TagrecError(f"softmax_over=\"catalogue\" is not mixed with negatives={neg!r}: it needs negatives=\"sampled\"")
    return over == "catalogue"


def check_catalogue_mask(cfg):
    """The catalogue_mask key of a config -> whether a user's other train positives leave the catalogue softmax; an unknown
    value, and "train_positives" without softmax_over="catalogue" (there is no catalogue to mask), is refused."""
    from ._lib import TagrecError
    mask = cfg.get("catalogue_mask", "none")
    if mask not in CATALOGUE_MASKS:
        raise TagrecError(f"unknown catalogue_mask {mask!r} (have {CATALOGUE_MASKS})")
    if mask != "none" and cfg.get("softmax_over", "negatives") != "catalogue":
        raise TagrecError(f"catalogue_mask={mask!r} masks columns of the softmax over the catalogue: it needs "
                          f"softmax_over=\"catalogue\", got {cfg.get('softmax_over', 'negatives')!r}")
    return mask == "train_positives"


def check_contrastive(cfg):
    """The three contrastive keys of a SimGCL config -> (cl_rate, cl_eps, cl_temperature); a bad value is refused."""
    from ._lib import TagrecError
    rate, eps, tau = cfg.get("cl_rate", 0.5), cfg.get("cl_eps", 0.1), cfg.get("cl_temperature", 0.2)
    for name, v in (("cl_rate", rate), ("cl_eps", eps)):
        if isinstance(v, bool) or not isinstance(v, (int, float)) or not 0 <= v < float("inf"):
            raise TagrecError(f"{name} must be a finite number >= 0, got {v!r}")
    if isinstance(tau, bool) or not isinstance(tau, (int, float)) or not 0 < tau < float("inf"):
        raise TagrecError(f"cl_temperature must be a finite number > 0, got {tau!r}")
    return float(rate), float(eps), float(tau)


def check_alignment(cfg):
    """The two DirectAU keys of a config -> (au_gamma, au_t); a bad value is refused: au_gamma finite and >= 0, au_t in
    (0, 20] (the uniformity kernels sum exp(-au_t |x - y|^2) <= e^(-4 au_t) without a running maximum)."""
    from ._lib import TagrecError
    gamma, t = cfg.get("au_gamma", 1.0), cfg.get("au_t", 2.0)
    if isinstance(gamma, bool) or not isinstance(gamma, (int, float)) or not 0 <= gamma < float("inf"):
        raise TagrecError(f"au_gamma must be a finite number >= 0, got {gamma!r}")
    if isinstance(t, bool) or not isinstance(t, (int, float)) or not 0 < t <= MAX_AU_T:
        raise TagrecError(f"au_t must be a number in (0, {MAX_AU_T:g}], got {t!r}")
    return float(gamma), float(t)


def check_ncl(cfg):
    """The seven NCL keys of a config -> (struct_rate, proto_rate, alpha, temperature, clusters, kmeans_iters, warm_up); a bad
    value is refused: the rates and alpha finite and >= 0, the temperature finite and > 0, clusters and iterations integers
    >= 1, warm-up an integer >= 0."""
    from ._lib import TagrecError
    d = _PER_MODEL["ncl"]
    vals = {k: cfg.get(k, d[k]) for k in ("ncl_struct_rate", "ncl_proto_rate", "ncl_alpha", "ncl_temperature", "ncl_clusters",
                                          "ncl_kmeans_iters", "ncl_warm_up")}
    for name in ("ncl_struct_rate", "ncl_proto_rate", "ncl_alpha"):
        v = vals[name]
        if isinstance(v, bool) or not isinstance(v, (int, float)) or not 0 <= v < float("inf"):
            raise TagrecError(f"{name} must be a finite number >= 0, got {v!r}")
    tau = vals["ncl_temperature"]
    if isinstance(tau, bool) or not isinstance(tau, (int, float)) or not 0 < tau < float("inf"):
        raise TagrecError(f"ncl_temperature must be a finite number > 0, got {tau!r}")
    for name, low in (("ncl_clusters", 1), ("ncl_kmeans_iters", 1), ("ncl_warm_up", 0)):
        v = vals[name]
        if isinstance(v, bool) or not isinstance(v, int) or v < low:
            raise TagrecError(f"{name} must be an integer >= {low}, got {v!r}")
    return (float(vals["ncl_struct_rate"]), float(vals["ncl_proto_rate"]), float(vals["ncl_alpha"]), float(tau),
            vals["ncl_clusters"], vals["ncl_kmeans_iters"], vals["ncl_warm_up"])


def check_ultragcn(cfg):
    """The five UltraGCN keys of a config -> (w1 .. w4, negative_weight, lambda, neighbors, zero_diagonal); a bad value is
    refused: the weights finite and >= 0, ug_neighbors an integer in 0 .. 64 (0: no neighbour term), ug_zero_diagonal a bool.
    The objective is its own: negatives="in_batch", softmax_over="catalogue" and mul_loss_func="softmax" are refused."""
    from ._lib import TagrecError
    d = _PER_MODEL["ultragcn"]
    w = cfg.get("ug_w", d["ug_w"])
    if not isinstance(w, (tuple, list)) or len(w) != 4:
        raise TagrecError(f"ug_w must be four numbers (w1, w2, w3, w4), got {w!r}")
    nums = [(f"ug_w[{i}]", v) for i, v in enumerate(w)] + [(k, cfg.get(k, d[k])) for k in ("ug_negative_weight", "ug_lambda")]
    for name, v in nums:
        if isinstance(v, bool) or not isinstance(v, (int, float)) or not 0 <= v < float("inf"):
            raise TagrecError(f"{name} must be a finite number >= 0, got {v!r}")
    m, zd = cfg.get("ug_neighbors", d["ug_neighbors"]), cfg.get("ug_zero_diagonal", d["ug_zero_diagonal"])
    if isinstance(m, bool) or not isinstance(m, int) or not 0 <= m <= MAX_UG_NEIGHBORS:
        raise TagrecError(f"ug_neighbors must be an integer in 0 .. {MAX_UG_NEIGHBORS}, got {m!r}")
    if not isinstance(zd, bool):
        raise TagrecError(f"ug_zero_diagonal must be True or False, got {zd!r}")
    if cfg.get("negatives", "sampled") != "sampled":
        raise TagrecError(f"ultragcn scores sampled negatives one by one: it needs negatives=\"sampled\", got {cfg.get('negatives')!r}")
    if cfg.get("softmax_over", "negatives") != "negatives":
        raise TagrecError("ultragcn is a pointwise loss, there is no softmax: it needs softmax_over=\"negatives\" (the default, "
                          f"unused), got {cfg.get('softmax_over')!r}")
    if cfg.get("mul_loss_func", "softplus") == "softmax":
        raise TagrecError("ultragcn is a pointwise loss: mul_loss_func=\"softmax\" is not covered")
    return tuple(float(v) for v in w), float(nums[4][1]), float(nums[5][1]), m, zd


CFG =get_config("lightgcn")


def init_seed(seed):
    """utility/utils.py:10-15."""
    import random
    import numpy as np
    random.seed(seed)
    np.random.seed(seed)
    torch.manual_seed(seed)
    if torch.cuda.is_available():
        torch.cuda.manual_seed_all(seed)
