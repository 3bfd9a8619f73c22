"""Host: `tagrec_adam_coef`, the per-step factors of the row-sparse Adam's ring (csrc/rowadam.hip).  No GPU: the library
loads without one and the function is host arithmetic only.

The factors are the double-precision expressions of `tagrec_adam_f32` -- lr / (1 - b1^t) and sqrt(1 - b2^t), each rounded to
float once -- so they must equal the same expressions in Python floats (doubles, the same libm) EXACTLY."""
import math

import numpy as np
import pytest

import tagrec_amd as T

CASES = ((1e-3, 0.9, 0.999), (0.01, 0.8, 0.99))


def _expected(lr, b1, b2, t0, n):
    return np.array([[np.float32(lr / (1 - b1 ** t)), np.float32(math.sqrt(1 - b2 ** t))] for t in range(t0, t0 + n)], dtype=np.float32)


def test_library_loads_without_a_gpu_and_exports_the_row_adam_entry_points():
    lib = T._lib.load()
    for name in ("tagrec_adam_coef", "tagrec_rowadam_catchup_f32", "tagrec_rowadam_apply_f32", "tagrec_rowadam_flush_f32"):
        assert name in T._lib.exported_symbols() and hasattr(lib, name)
    assert lib.tagrec_abi_version() == 2


@pytest.mark.parametrize("lr,b1,b2", CASES)
def test_coef_equals_the_double_expressions_exactly(lr, b1, b2):
    got = T.rowops.adam_coef(lr, b1, b2, 1, 5000).numpy()
    want = _expected(lr, b1, b2, 1, 5000)
    assert got.shape == (5000, 2) and got.dtype == np.float32
    assert np.array_equal(got.view(np.int32), want.view(np.int32))


@pytest.mark.parametrize("lr,b1,b2", CASES)
def test_a_block_that_starts_later_equals_the_same_entries(lr, b1, b2):
    whole = T.rowops.adam_coef(lr, b1, b2, 1, 5000).numpy()
    block = T.rowops.adam_coef(lr, b1, b2, 4097, 600).numpy()
    assert np.array_equal(block.view(np.int32), whole[4096:4696].view(np.int32))


def test_coef_refuses_step_zero_and_takes_an_empty_block():
    with pytest.raises(T.TagrecError, match="counted from 1"):
        T.rowops.adam_coef(1e-3, 0.9, 0.999, 0, 4)
    assert tuple(T.rowops.adam_coef(1e-3, 0.9, 0.999, 7, 0).shape) == (0, 2)
