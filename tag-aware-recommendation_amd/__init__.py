"""tagrec_amd -- MI355X-native hot path for tag-aware graph recommenders.

Python host code (this package) mirrors the reference's operator / model / step
surface and calls a C-ABI HIP library
(`csrc/` -> `libtagrec_hip.so`, declared in `include/tagrec.h`) through ctypes.
There is no CPU fallback: every op raises if the library or a GPU is missing.

Reference name                      here
  model.help.split_mm / mul_loss ...  tagrec_amd.help
  model.LightGCN / NGCF / TGCN        tagrec_amd.LightGCN / NGCF / TGCN
  model.DGCF / DisenGCN / KGAT        tagrec_amd.DGCF / DisenGCN / KGAT
  model.DisenHAN                      tagrec_amd.DisenHAN (disenhan_config(**kw))
  -- (not in the reference)           tagrec_amd.SimGCL: LightGCN + contrastive noise views (get_config("simgcl"))
  -- (not in the reference)           tagrec_amd.DirectAU: LightGCN under the alignment / uniformity loss (get_config("directau"))
  -- (not in the reference)           tagrec_amd.NCL: LightGCN + structure / prototype contrast (get_config("ncl"))
  -- (not in the reference)           tagrec_amd.UltraGCN: plain tables under a weighted pointwise BCE (get_config("ultragcn"))
  -- (not in the reference)           tagrec_amd.item_cooccurrence_topk: top-k of the sparse item-item product (cooc.py)
  -- (not in the reference)           tagrec_amd.kmeans: Lloyd's algorithm on the device (kmeans.py)
  train_data.BPR_training_data        tagrec_amd.BPR_training_data
  training.Basic_train / Basic_test   tagrec_amd.Basic_train / Basic_test
  training.utils.user_group_split     tagrec_amd.user_group_split
  training.basic_train.epoch_training tagrec_amd.epoch_training
  utility.word.CFG                    tagrec_amd.CFG (get_config(model, **kw))
"""
from . import synth  # noqa: F401
from . import _lib, config, data, graph, help  # noqa: F401
from ._lib import TagrecError  # noqa: F401
from .config import CFG, get_config, init_seed  # noqa: F401
from .evaluate import Basic_test, user_group_split  # noqa: F401
from .graph import Graph, creat_adj  # noqa: F401
from .lightgcn import LightGCN  # noqa: F401
from .simgcl import SimGCL  # noqa: F401
from .directau import DirectAU  # noqa: F401
from .kmeans import kmeans  # noqa: F401
from .ncl import NCL  # noqa: F401
from .cooc import item_cooccurrence_topk  # noqa: F401
from .ultragcn import UltraGCN  # noqa: F401
from .ngcf import NGCF  # noqa: F401
from .tgcn import TGCN  # noqa: F401
from .dgcf import DGCF  # noqa: F401
from .disengcn import DisenGCN  # noqa: F401
from .kgat import KGAT  # noqa: F401
from .disenhan import DisenHAN, disenhan_config  # noqa: F401
from .train import Adam, Basic_train, Early_stop, GraphedStep, RowAdam, epoch_training  # noqa: F401
from .train_data import (Abstract_training_data, BPR_training_data, DGCF_training_data,  # noqa: F401
                         Fixed_training_data, KGAT_training_data, TransTag_training_data)
