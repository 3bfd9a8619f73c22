"""CPU-only: the host surface of kernel-mode edge dropout (`node_drop_mode`) -- defaults, refusals, ABI additions."""
import pytest

import tagrec_amd as T
from tagrec_amd import help as H


def test_node_drop_mode_defaults_to_rebuild():
    assert T.get_config("lightgcn")["node_drop_mode"] == "rebuild"
    assert T.get_config("ngcf")["node_drop_mode"] == "rebuild"
    assert H.NODE_DROP_MODES == ("rebuild", "kernel")


def test_unknown_mode_raises():
    with pytest.raises(T.TagrecError):
        H.node_drop(None, 0.1, True, mode="in_place")
    with pytest.raises(T.TagrecError):
        H.node_drop(None, 0.0, False, mode="")


def test_kernel_mode_refuses_fold_lists_and_needs_a_seed():
    with pytest.raises(T.TagrecError):
        H.node_drop([object(), object()], 0.1, True, mode="kernel", seed=1)
    with pytest.raises(T.TagrecError):
        H.node_drop(object(), 0.1, True, mode="kernel")
    g = object()
    assert H.node_drop(g, 0.0, True, mode="kernel", seed=1) is g and H.node_drop(g, 0.3, False, mode="kernel") is g
    with pytest.raises(T.TagrecError):
        T.graph.EdgeDropView(object(), 0.1, 1, False)


def test_edge_drop_entry_points_are_exported():
    lib = T._lib.load()
    names = [n for n in T._lib.exported_symbols() if "edrop" in n or "edge_drop" in n]
    assert sorted(names) == ["tagrec_edge_drop_mask_u8", "tagrec_spmm_axpy_sparse_edrop_f32", "tagrec_spmm_edrop_f32",
                             "tagrec_spmm_listed_edrop_f32", "tagrec_spmm_norm_acc_rows_edrop_f32",
                             "tagrec_spmm_normbwd_sparse_edrop_f32"]
    assert all(hasattr(lib, n) for n in names) and lib.tagrec_abi_version() == 2
    # argument checks that need no device: a null handle, p outside [0, 1), a width without a vector kernel
    assert lib.tagrec_edge_drop_mask_u8(None, 0.5, 1, 0, None, None) != 0
    assert lib.tagrec_spmm_edrop_f32(None, None, None, 1.0, 1, 0, 64, None) != 0
    assert lib.tagrec_spmm_edrop_f32(None, None, None, 0.5, 1, 0, 20, None) != 0
    assert b"edge dropout" in lib.tagrec_last_error()

