"""lig_shard_rows_diagnose without a GPU: the symbol is exported and bound, and the argument checks that come before any shard or device
is looked at give the codes lig_rows_diagnose gives (the checks on a real shard: tests/test_gpu_shard_diagnose.py)."""
import ctypes as C
import inspect

import pytest

import hip_lib


@pytest.fixture(scope="module")
def amd():
    return hip_lib.load()


def test_symbol_is_exported_and_bound(amd):
    L = amd.load_library()
    assert "lig_shard_rows_diagnose" in amd.EXPORTS and hasattr(L, "lig_shard_rows_diagnose")
    assert len(L.lig_shard_rows_diagnose.argtypes) == len(L.lig_rows_diagnose.argtypes) == 7
    sig = inspect.signature(amd.Context.shard_rows_diagnose)
    assert list(sig.parameters) == ["self", "shard", "system", "lin_cap", "quad_cap"]
    assert [sig.parameters[p].default for p in ("system", "lin_cap", "quad_cap")] == [None, 1024, 1024]


def test_null_shard_null_info_and_short_info_give_the_codes_of_rows_diagnose(amd):
    L = amd.load_library()
    info = amd.DiagInfo()
    info.struct_bytes = C.sizeof(amd.DiagInfo)
    short = amd.DiagInfo()
    short.struct_bytes = C.sizeof(amd.DiagInfo) - 8
    for args in ((None, None, None, 0, None, 0, C.byref(info)), (None, None, None, 0, None, 0, None), (None, None, None, 0, None, 0, C.byref(short))):
        assert L.lig_shard_rows_diagnose(*args) == L.lig_rows_diagnose(*args) == -1
