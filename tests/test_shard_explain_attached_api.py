"""lig_shard_rows_explain_attached without a GPU: the header declares the entry with the parameters of lig_rows_explain_attached (a shard
in place of the trace), the library exports it, the Python EXPORTS list and the Context method are in step, the argument checks that come
before any shard or device is looked at give the codes of the one-GPU call, and the notes that said a shard has no attached explain are
reworded (the checks on a real shard: tests/test_gpu_shard_explain_attached.py)."""
import ctypes as C
import inspect
import os
import re

import pytest

import hip_lib
from test_shard_explain_api import declaration

ROOT = hip_lib.ROOT
E_ARG = -1
NEW, ONE_GPU = "lig_shard_rows_explain_attached", "lig_rows_explain_attached"


@pytest.fixture(scope="module")
def amd():
    return hip_lib.load()


def test_header_declares_the_one_gpu_parameters_with_a_shard_in_front():
    assert declaration(NEW) == [("lig_shard*", "shard")] + declaration(ONE_GPU)[1:]


def test_symbol_is_exported_and_bound(amd):
    L = amd.load_library()
    assert NEW in amd.EXPORTS and hasattr(L, NEW)
    assert getattr(L, NEW).argtypes == getattr(L, ONE_GPU).argtypes and len(getattr(L, NEW).argtypes) == len(declaration(NEW))
    sig = inspect.signature(amd.Context.shard_rows_explain_attached)
    assert list(sig.parameters) == ["self", "shard", "constraints", "term_cap"] and sig.parameters["term_cap"].default == 4096


def test_null_shard_null_info_and_short_info_give_the_codes_of_the_one_gpu_call(amd):
    L = amd.load_library()
    info = amd.ExplainInfo()
    info.struct_bytes = C.sizeof(amd.ExplainInfo)
    short = amd.ExplainInfo()
    short.struct_bytes = C.sizeof(amd.ExplainInfo) - 8
    for args in ((None, None, 0, None, None, 0, C.byref(info)), (None, None, 0, None, None, 0, None), (None, None, 0, None, None, 0, C.byref(short))):
        assert L.lig_shard_rows_explain_attached(*args) == L.lig_rows_explain_attached(*args) == E_ARG


def test_the_notes_that_a_shard_has_no_attached_explain_are_reworded():
    def flat(rel):
        return re.sub(r"[\s/*]+", " ", open(os.path.join(ROOT, rel)).read())
    for rel in ("include/lig_hip.h", "DESIGN.md", "README.md", "INTEGRATION.md"):
        assert "an attached explain on a shard" not in flat(rel), rel
        assert NEW in flat(rel), rel
    assert "There is no attached variant" not in flat("INTEGRATION.md")
