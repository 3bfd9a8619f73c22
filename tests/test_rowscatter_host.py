"""CPU-only checks of the deterministic mode: the config key, the numpy order reference that the GPU tests compare against
(rowscatter_ref.py) against a float64 sum, and the new entry points in the built library."""
import numpy as np

import tagrec_amd as T
from rowscatter_ref import make_values, scatter_ref, segments, zipf_rows


def test_config_carries_the_key_switched_off():
    for model in ("lightgcn", "ngcf", "tgcn", "dgcf", "disengcn", "kgat"):
        assert T.get_config(model)["deterministic"] is False
    assert T.get_config("lightgcn", deterministic=True)["deterministic"] is True


def test_order_reference_agrees_with_float64():
    """Per row and element: |fp32 chain - float64 sum| <= T * 2^-24 * sum |terms| for a row named T times (every one of the
    T - 1 adds, and the adds of the chunk sums, rounds a partial sum of magnitude <= sum |terms| by at most 2^-24 of it)."""
    rng = np.random.default_rng(0)
    for rows, n in ((zipf_rows(rng, 1536, 300), 300), (np.full(2049, 3, dtype=np.int64), 16)):
        src = make_values(rng, len(rows), 20)
        got = scatter_ref(rows, n, src, np.zeros((n, 20), np.float32), False)
        assert got.dtype == np.float32
        for r, slots in segments(rows, n):
            terms = src[slots].astype(np.float64)
            bound = len(slots) * 2.0 ** -24 * np.abs(terms).sum(0)
            assert np.all(np.abs(got[r].astype(np.float64) - terms.sum(0)) <= bound), r
        # and the order matters at these values, or the GPU tests would be blind
        assert not np.array_equal(scatter_ref(rows, n, src, np.zeros((n, 20), np.float32), False, descending=True), got)


def test_new_entry_points_are_exported():
    lib = T._lib.load()
    for name in ("tagrec_rowlist_workspace", "tagrec_rowlist_plan_result", "tagrec_rowlist_plan_i64", "tagrec_row_scatter_ordered_f32"):
        assert name in T._lib.exported_symbols() and hasattr(lib, name)
    # argument checks come before anything touches a device
    assert lib.tagrec_rowlist_workspace(0, 64) == 0 and lib.tagrec_rowlist_workspace(16, 0) == 0
    assert lib.tagrec_rowlist_plan_i64(None, 4, 16, 64, None, 0, None) != 0
    assert b"null pointer" in lib.tagrec_last_error()
