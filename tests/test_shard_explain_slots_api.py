"""lig_shard_rows_explain_slots* / lig_shard_rows_untouched_slots* without a GPU: the header declares the four entries with the parameters of
the one-GPU calls (a shard in place of the trace), the library exports them, the Python EXPORTS list and the Context methods are in step,
no struct of the ABI changed, the argument checks that come before any shard or device is looked at give the codes of the one-GPU calls,
the header documents the contract, and the notes that called the sharded entry the next step are reworded (the checks on a real shard:
tests/test_gpu_shard_explain_slots.py)."""
import ctypes as C
import inspect
import os
import re

import numpy as np
import pytest

import hip_lib
from test_explain_api import declaration, header

ROOT = hip_lib.ROOT
E_ARG = -1
PAIRS = {"lig_shard_rows_explain_slots": "lig_rows_explain_slots", "lig_shard_rows_explain_slots_attached": "lig_rows_explain_slots_attached",
         "lig_shard_rows_untouched_slots": "lig_rows_untouched_slots", "lig_shard_rows_untouched_slots_attached": "lig_rows_untouched_slots_attached"}


@pytest.fixture(scope="module")
def amd():
    return hip_lib.load()


def info_of(cls, short=0):
    info = cls()
    info.struct_bytes = C.sizeof(cls) - short
    return info


def test_header_declares_the_one_gpu_parameters_with_a_shard_in_front():
    for new, one_gpu in PAIRS.items():
        assert declaration(new) == [("lig_shard*", "shard")] + declaration(one_gpu)[1:], new
    assert declaration("lig_shard_rows_explain_slots")[1] == declaration("lig_shard_rows_untouched_slots")[1] == ("const lig_linear_system*", "sys")


def test_symbols_are_exported_and_bound(amd):
    L = amd.load_library()
    assert len(set(amd.EXPORTS)) == len(amd.EXPORTS)
    for new, one_gpu in PAIRS.items():
        assert new in amd.EXPORTS and hasattr(L, new), new
        fn = getattr(L, new)
        assert list(fn.argtypes) == list(getattr(L, one_gpu).argtypes) and len(fn.argtypes) == len(declaration(new)), new
        assert fn.restype is C.c_int


def test_python_methods(amd):
    sig = inspect.signature(amd.Context.shard_rows_explain_slots)
    att = inspect.signature(amd.Context.shard_rows_explain_slots_attached)
    assert list(sig.parameters) == ["self", "shard", "system", "slots", "term_cap"] and list(att.parameters) == ["self", "shard", "slots", "term_cap"]
    assert sig.parameters["term_cap"].default == att.parameters["term_cap"].default == inspect.signature(amd.Context.rows_explain_slots).parameters["term_cap"].default
    sig = inspect.signature(amd.Context.shard_rows_untouched_slots)
    att = inspect.signature(amd.Context.shard_rows_untouched_slots_attached)
    assert list(sig.parameters) == ["self", "shard", "system", "nonzero_only", "cap"] and list(att.parameters) == ["self", "shard", "nonzero_only", "cap"]
    assert sig.parameters["cap"].default == att.parameters["cap"].default == inspect.signature(amd.Context.rows_untouched_slots).parameters["cap"].default
    assert sig.parameters["nonzero_only"].default is False and att.parameters["nonzero_only"].default is False


def test_no_new_abi_struct(amd):
    L = amd.load_library()
    sizes = (C.c_uint32 * 6)()
    L.lig_abi_sizes(sizes)
    assert list(sizes) == [32, 192, 184, 56, 168, 64]
    assert re.search(r"LIG_ABI_STRUCTS\s*=\s*6\b", header())
    assert (amd.SLOT_RECORD.itemsize, amd.SLOT_TERM.itemsize, C.sizeof(amd.SlotInfo), amd.SLOT_VALUE.itemsize, C.sizeof(amd.UntouchedInfo)) == (56, 80, 40, 40, 40)


def test_argument_errors_before_any_shard_is_looked_at(amd):
    L = amd.load_library()
    asked = np.zeros(1, dtype=np.uint32)
    rec, terms, vals = np.zeros(1, dtype=amd.SLOT_RECORD), np.zeros(4, dtype=amd.SLOT_TERM), np.zeros(4, dtype=amd.SLOT_VALUE)
    p = lambda a: a.ctypes.data_as(C.c_void_p)
    si, ui = lambda short=0: C.byref(info_of(amd.SlotInfo, short)), lambda short=0: C.byref(info_of(amd.UntouchedInfo, short))
    # a NULL shard: the codes of the one-GPU calls for a NULL trace
    for args in ((None, p(asked), 1, p(rec), p(terms), 4, si()), (None, None, 0, None, None, 0, si())):
        assert L.lig_shard_rows_explain_slots_attached(*args) == L.lig_rows_explain_slots_attached(*args) == E_ARG
    assert L.lig_shard_rows_explain_slots(None, None, p(asked), 1, p(rec), p(terms), 4, si()) == E_ARG
    assert L.lig_shard_rows_untouched_slots_attached(None, 0, p(vals), 4, ui()) == L.lig_rows_untouched_slots_attached(None, 0, p(vals), 4, ui()) == E_ARG
    assert L.lig_shard_rows_untouched_slots(None, None, 1, None, 0, ui()) == E_ARG
    # a NULL or short info, a NULL array with a count or cap: decided before the shard is dereferenced (the "shard" is zeroed memory)
    fake = np.zeros(1 << 16, dtype=np.uint8)
    for call, head in ((L.lig_shard_rows_explain_slots_attached, (p(fake),)), (L.lig_shard_rows_explain_slots, (p(fake), None))):
        assert call(*head, p(asked), 1, p(rec), p(terms), 4, None) == E_ARG
        assert call(*head, p(asked), 1, p(rec), p(terms), 4, si(short=8)) == E_ARG
        assert call(*head, p(asked), 1, None, p(terms), 4, si()) == E_ARG
        assert call(*head, None, 1, p(rec), p(terms), 4, si()) == E_ARG
        assert call(*head, p(asked), 1, p(rec), None, 4, si()) == E_ARG
    for call, head in ((L.lig_shard_rows_untouched_slots_attached, (p(fake),)), (L.lig_shard_rows_untouched_slots, (p(fake), None))):
        assert call(*head, 0, p(vals), 4, None) == E_ARG
        assert call(*head, 0, p(vals), 4, ui(short=8)) == E_ARG
        assert call(*head, 1, None, 4, ui()) == E_ARG
    # (the range, order and state errors on a REAL shard: tests/test_gpu_shard_explain_slots.py)


def flat(rel):
    return re.sub(r"[\s/*]+", " ", open(os.path.join(ROOT, rel)).read())


def test_header_documents_the_contract():
    h = flat("include/lig_hip.h")
    at = h.index("lig_rows_explain_slots lig_rows_untouched_slots on a rows shard")
    doc = h[at:h.index("int lig_shard_rows_explain_slots_attached(", at)]
    for phrase in ("SLOTS ARE GLOBAL", "COLLECTIVE", "EVERY RANK RECEIVES THE SAME BYTES", "WINDOW, FAILURE, POISONING", "REFUSALS", "LIG_E_ARG", "LIG_E_STATE",
                   "n_asked == 0: LIG_OK, no launch, no collective", "exactly one holder", "16 + 48 n_asked", "16 P bytes", "40 P bytes", "term_cap = 0",
                   "world == 1 without LIG_SHARD_FORCE_EXCHANGE", "SCRATCH", "lig_comm.forget"):
        assert phrase in doc, phrase
    assert "Not covered here: the sharded entry" not in h and "lig_shard_rows_explain_slots lig_shard_rows_untouched_slots below" in h


def test_the_notes_that_called_the_sharded_entry_the_next_step_are_reworded():
    for rel in ("DESIGN.md", "README.md", "INTEGRATION.md", "tools/README.md"):
        assert "lig_shard_rows_explain_slots" in flat(rel), rel
    for rel in ("DESIGN.md", "README.md", "INTEGRATION.md"):
        assert "lig_shard_rows_untouched_slots" in flat(rel), rel
    assert "the sharded entry is the next step" not in flat("README.md")
    assert "Not done: the sharded entry (the next change)" not in flat("DESIGN.md")
    shim = flat("include/lig_hip_row_batcher.hpp")
    for member in ("shard_explain_slots(", "shard_explain_slots_attached(", "shard_untouched_slots(", "shard_untouched_slots_attached("):
        assert "void " + member in shim, member
