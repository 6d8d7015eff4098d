"""lig_shard_rows_set_linear_values / lig_shard_rows_diagnose_attached without a GPU: the symbols are exported and bound, the wrappers
have the stated signatures, and the argument checks that come before any shard or device is looked at give the codes the one-GPU calls
give (the checks on a real shard: tests/test_gpu_shard_values.py, tests/test_gpu_shard_diagnose_attached.py)."""
import ctypes as C
import inspect

import pytest

import hip_lib


@pytest.fixture(scope="module")
def amd():
    return hip_lib.load()


def test_symbols_are_exported_and_bound(amd):
    L = amd.load_library()
    for name in ("lig_shard_rows_set_linear_values", "lig_shard_rows_diagnose_attached"):
        assert name in amd.EXPORTS and hasattr(L, name), name
    assert len(L.lig_shard_rows_set_linear_values.argtypes) == len(L.lig_rows_set_linear_values.argtypes) == 3
    assert list(L.lig_shard_rows_set_linear_values.argtypes) == list(L.lig_rows_set_linear_values.argtypes)
    assert len(L.lig_shard_rows_diagnose_attached.argtypes) == len(L.lig_rows_diagnose_attached.argtypes) == 6
    assert list(L.lig_shard_rows_diagnose_attached.argtypes) == list(L.lig_rows_diagnose_attached.argtypes)


def test_wrapper_signatures(amd):
    sig = inspect.signature(amd.Context.shard_rows_set_linear_values)
    assert list(sig.parameters) == ["self", "shard", "coefs"]
    assert list(inspect.signature(amd.Context.rows_set_linear_values).parameters) == ["self", "trace", "coefs"]
    sig = inspect.signature(amd.Context.shard_rows_diagnose_attached)
    assert list(sig.parameters) == ["self", "shard", "lin_cap", "quad_cap"]
    assert [sig.parameters[p].default for p in ("lin_cap", "quad_cap")] == [1024, 1024]
    one = inspect.signature(amd.Context.rows_diagnose_attached)
    assert [one.parameters[p].default for p in ("lin_cap", "quad_cap")] == [1024, 1024]


def test_null_shard_gives_the_code_of_rows_set_linear_values(amd):
    L = amd.load_library()
    tab = (C.c_uint8 * 32)()
    for args in ((None, None, 0), (None, tab, 1)):
        assert L.lig_shard_rows_set_linear_values(*args) == L.lig_rows_set_linear_values(*args) == -1


def test_null_shard_null_info_and_short_info_give_the_codes_of_rows_diagnose_attached(amd):
    L = amd.load_library()
    info = amd.DiagInfo()
    info.struct_bytes = C.sizeof(amd.DiagInfo)
    short = amd.DiagInfo()
    short.struct_bytes = C.sizeof(amd.DiagInfo) - 8
    for args in ((None, None, 0, None, 0, C.byref(info)), (None, None, 0, None, 0, None), (None, None, 0, None, 0, C.byref(short))):
        assert L.lig_shard_rows_diagnose_attached(*args) == L.lig_rows_diagnose_attached(*args) == -1
