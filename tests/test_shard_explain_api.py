"""lig_shard_rows_explain / lig_shard_rows_read_slots without a GPU: the header declares both entries with the parameters of the one-GPU
calls (a shard in place of the trace), the library exports them, the Python EXPORTS list and the Context methods are in step, the
argument checks that come before any shard or device is looked at give the codes of lig_rows_explain / lig_rows_read_slots, and the
four notes that said the sharded entry was not covered are gone (the checks on a real shard: tests/test_gpu_shard_explain.py)."""
import ctypes as C
import inspect
import os
import re

import numpy as np
import pytest

import hip_lib

ROOT = hip_lib.ROOT
E_ARG = -1


@pytest.fixture(scope="module")
def amd():
    return hip_lib.load()


def header():
    hdr = open(os.path.join(ROOT, "include", "lig_hip.h")).read()
    return re.sub(r"/\*.*?\*/", "", hdr, flags=re.S)


def declaration(name):
    """the parameter list of `name` in include/lig_hip.h -> [(type, parameter name)], comments removed"""
    m = re.search(r"\bint\s+%s\s*\(([^)]*)\)\s*;" % name, header())
    assert m, "%s is not declared" % name
    out = []
    for p in m.group(1).split(","):
        ty, pname = re.match(r"\s*(.*?)\s*(\w+)\s*$", p, flags=re.S).groups()
        out.append((re.sub(r"\s+", " ", ty).replace(" *", "*"), pname))
    return out


def test_header_declares_the_one_gpu_parameters_with_a_shard_in_front():
    for shard, one in (("lig_shard_rows_explain", "lig_rows_explain"), ("lig_shard_rows_read_slots", "lig_rows_read_slots")):
        assert declaration(shard) == [("lig_shard*", "shard")] + declaration(one)[1:]


def test_symbols_are_exported_and_bound(amd):
    L = amd.load_library()
    for shard, one in (("lig_shard_rows_explain", "lig_rows_explain"), ("lig_shard_rows_read_slots", "lig_rows_read_slots")):
        assert shard in amd.EXPORTS and hasattr(L, shard)
        assert getattr(L, shard).argtypes == getattr(L, one).argtypes and len(getattr(L, shard).argtypes) == len(declaration(shard))
    sig = inspect.signature(amd.Context.shard_rows_explain)
    assert list(sig.parameters) == ["self", "shard", "system", "constraints", "term_cap"] and sig.parameters["term_cap"].default == 4096
    assert list(inspect.signature(amd.Context.shard_rows_read_slots).parameters) == ["self", "shard", "slots"]


def test_null_shard_null_info_and_short_info_give_the_codes_of_the_one_gpu_calls(amd):
    L = amd.load_library()
    info = amd.ExplainInfo()
    info.struct_bytes = C.sizeof(amd.ExplainInfo)
    short = amd.ExplainInfo()
    short.struct_bytes = C.sizeof(amd.ExplainInfo) - 8
    for args in ((None, None, None, 0, None, None, 0, C.byref(info)), (None, None, None, 0, None, None, 0, None), (None, None, None, 0, None, None, 0, C.byref(short))):
        assert L.lig_shard_rows_explain(*args) == L.lig_rows_explain(*args) == E_ARG
    slots, values = np.zeros(2, dtype=np.uint32), np.zeros((2, 8), dtype=np.uint32)
    for args in ((None, None, 0, None), (None, amd._hptr(slots), 2, amd._hptr(values))):
        assert L.lig_shard_rows_read_slots(*args) == L.lig_rows_read_slots(*args) == E_ARG


def test_the_notes_that_the_sharded_entry_is_not_covered_are_gone():
    def flat(rel):
        return re.sub(r"[\s/*]+", " ", open(os.path.join(ROOT, rel)).read())
    assert "Not covered: the sharded entry" not in flat("include/lig_hip.h")
    assert "explain_batcher_prog.cpp`). Not on the sharded entry" not in flat("INTEGRATION.md")
    batcher = flat("include/lig_hip_row_batcher.hpp")
    assert "hip_row_batcher::explain: not on a sharded batcher" not in batcher and "hip_row_batcher::read_slots: not on a sharded batcher" not in batcher
    assert "lig_shard_rows_explain" in flat("DESIGN.md") and "lig_shard_rows_explain" in flat("README.md") and "lig_shard_rows_explain" in flat("INTEGRATION.md")
