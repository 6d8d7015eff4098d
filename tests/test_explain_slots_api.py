"""lig_rows_explain_slots* / lig_rows_untouched_slots* without a GPU: the four entries are declared, exported and bound with the header's
signatures, the Python methods have the documented parameters, the new structs have their stated sizes, no struct of the ABI changed size,
the argument checks that come before any trace or device is looked at answer, and the reference of the GPU tests (tests/slots_ref.py)
is consistent with the reference of lig_rows_explain (tests/explain_ref.py)."""
import ctypes as C
import inspect
import re

import numpy as np
import pytest

import explain_ref as er
import hip_lib
import linear_ref as lr
import oracle_lib as ol
import slots_ref as sr
from test_explain_api import declaration, header, small_case

P = ol.P
E_ARG = -1
NEW = ["lig_rows_explain_slots", "lig_rows_explain_slots_attached", "lig_rows_untouched_slots", "lig_rows_untouched_slots_attached"]


@pytest.fixture(scope="module")
def amd():
    return hip_lib.load()


def info_of(cls, short=0):
    info = cls()
    info.struct_bytes = C.sizeof(cls) - short
    return info


def test_declared_exported_and_bound(amd):
    L = amd.load_library()
    declared = set(re.findall(r"\b(lig_\w+)\s*\(", header()))
    assert set(NEW) <= declared and all(name in amd.EXPORTS for name in NEW) and len(set(amd.EXPORTS)) == len(amd.EXPORTS)
    attached = declaration("lig_rows_explain_slots_attached")
    assert attached == [("lig_trace*", "trace"), ("const uint32_t*", "slots"), ("uint64_t", "n_asked"), ("lig_slot_record*", "slot_out"),
                        ("lig_slot_term*", "terms_out"), ("uint64_t", "term_cap"), ("lig_slot_info*", "info")]
    assert attached == [p for p in declaration("lig_rows_explain_slots") if p[1] != "sys"]
    assert declaration("lig_rows_explain_slots")[1] == ("const lig_linear_system*", "sys")
    untouched = declaration("lig_rows_untouched_slots_attached")
    assert untouched == [("lig_trace*", "trace"), ("int", "nonzero_only"), ("lig_slot_value*", "out"), ("uint64_t", "cap"), ("lig_untouched_info*", "info")]
    assert untouched == [p for p in declaration("lig_rows_untouched_slots") if p[1] != "sys"]
    assert declaration("lig_rows_untouched_slots")[1] == ("const lig_linear_system*", "sys")
    ctype = {"lig_trace*": C.c_void_p, "const uint32_t*": C.c_void_p, "lig_slot_record*": C.c_void_p, "lig_slot_term*": C.c_void_p,
             "lig_slot_value*": C.c_void_p, "uint64_t": C.c_uint64, "int": C.c_int, "lig_slot_info*": C.POINTER(amd.SlotInfo),
             "lig_untouched_info*": C.POINTER(amd.UntouchedInfo), "const lig_linear_system*": C.POINTER(amd.LinearSystem)}
    for name in NEW:
        fn = getattr(L, name)                                     # resolves in the library
        assert list(fn.argtypes) == [ctype[ty] for ty, _ in declaration(name)], name
        assert fn.restype is C.c_int


def test_python_methods(amd):
    sig = inspect.signature(amd.Context.rows_explain_slots)
    att = inspect.signature(amd.Context.rows_explain_slots_attached)
    assert list(sig.parameters) == ["self", "trace", "system", "slots", "term_cap"] and list(att.parameters) == ["self", "trace", "slots", "term_cap"]
    assert sig.parameters["term_cap"].default == att.parameters["term_cap"].default == 4096
    sig = inspect.signature(amd.Context.rows_untouched_slots)
    att = inspect.signature(amd.Context.rows_untouched_slots_attached)
    assert list(sig.parameters) == ["self", "trace", "system", "nonzero_only", "cap"] and list(att.parameters) == ["self", "trace", "nonzero_only", "cap"]
    assert sig.parameters["cap"].default == att.parameters["cap"].default == 1024
    assert sig.parameters["nonzero_only"].default is False and att.parameters["nonzero_only"].default is False


def test_struct_sizes_are_the_headers_and_the_abi_is_unchanged(amd):
    L = amd.load_library()
    stated = {name: int(n) for name, n in re.findall(r"\}\s*(lig_slot_\w+|lig_untouched_info)\s*;\s*/\*\s*(\d+) bytes", open(hip_lib.ROOT + "/include/lig_hip.h").read())}
    assert stated == {"lig_slot_record": 56, "lig_slot_term": 80, "lig_slot_info": 40, "lig_slot_value": 40, "lig_untouched_info": 40}
    assert (amd.SLOT_RECORD.itemsize, amd.SLOT_TERM.itemsize, C.sizeof(amd.SlotInfo), amd.SLOT_VALUE.itemsize, C.sizeof(amd.UntouchedInfo)) == (56, 80, 40, 40, 40)
    assert [amd.SLOT_RECORD.fields[f][1] for f in ("slot", "row_kind", "n_terms", "first_term", "value")] == [0, 4, 8, 16, 24]
    assert [amd.SLOT_TERM.fields[f][1] for f in ("slot", "constraint", "coef_index", "constraint_terms", "coef", "residual")] == [0, 4, 8, 12, 16, 48]
    assert [amd.SLOT_VALUE.fields[f][1] for f in ("slot", "row_kind", "value")] == [0, 4, 8]
    assert [getattr(amd.SlotInfo, f).offset for f in ("struct_bytes", "n_terms_total", "n_terms_reported", "n_constraints_distinct", "ms_total")] == [0, 8, 16, 24, 32]
    assert [getattr(amd.UntouchedInfo, f).offset for f in ("struct_bytes", "n_untouched", "n_untouched_nonzero", "n_reported", "ms_total")] == [0, 8, 16, 24, 32]
    sizes = (C.c_uint32 * 6)()
    L.lig_abi_sizes(sizes)
    assert list(sizes) == [32, 192, 184, 56, 168, 64]
    assert re.search(r"LIG_ABI_STRUCTS\s*=\s*6\b", header())


def test_argument_errors_before_any_trace_is_looked_at(amd):
    L = amd.load_library()
    asked = np.zeros(1, dtype=np.uint32)
    rec, terms, vals = np.zeros(1, dtype=amd.SLOT_RECORD), np.zeros(4, dtype=amd.SLOT_TERM), np.zeros(4, dtype=amd.SLOT_VALUE)
    p = lambda a: a.ctypes.data_as(C.c_void_p)
    si, ui = lambda short=0: C.byref(info_of(amd.SlotInfo, short)), lambda short=0: C.byref(info_of(amd.UntouchedInfo, short))
    # a NULL trace: no context is needed to say so
    assert L.lig_rows_explain_slots_attached(None, p(asked), 1, p(rec), p(terms), 4, si()) == E_ARG
    assert L.lig_rows_explain_slots(None, None, p(asked), 1, p(rec), p(terms), 4, si()) == E_ARG
    assert L.lig_rows_explain_slots_attached(None, None, 0, None, None, 0, si()) == E_ARG
    assert L.lig_rows_untouched_slots_attached(None, 0, p(vals), 4, ui()) == E_ARG
    assert L.lig_rows_untouched_slots(None, None, 1, None, 0, ui()) == E_ARG
    # a NULL or short info, a NULL array with a count or cap: decided before the trace is dereferenced (the "trace" is zeroed memory)
    fake = np.zeros(1 << 16, dtype=np.uint8)
    for call, head in ((L.lig_rows_explain_slots_attached, (p(fake),)), (L.lig_rows_explain_slots, (p(fake), None))):
        assert call(*head, p(asked), 1, p(rec), p(terms), 4, None) == E_ARG
        assert call(*head, p(asked), 1, p(rec), p(terms), 4, si(short=8)) == E_ARG
        assert call(*head, p(asked), 1, None, p(terms), 4, si()) == E_ARG
        assert call(*head, None, 1, p(rec), p(terms), 4, si()) == E_ARG
        assert call(*head, p(asked), 1, p(rec), None, 4, si()) == E_ARG
    for call, head in ((L.lig_rows_untouched_slots_attached, (p(fake),)), (L.lig_rows_untouched_slots, (p(fake), None))):
        assert call(*head, 0, p(vals), 4, None) == E_ARG
        assert call(*head, 0, p(vals), 4, ui(short=8)) == E_ARG
        assert call(*head, 1, None, 4, ui()) == E_ARG
    # (the range, order and state errors on a REAL trace: tests/test_gpu_explain_slots.py)


def test_reference_is_the_explain_reference_seen_from_the_slots():
    system, rows, l, w = small_case()
    kinds = [0, 1, 2, 3]
    total, rep, distinct, recs, terms = sr.explain_slots(system, kinds, rows, l, range(4 * l), 100)
    assert (total, rep, distinct) == (11, 11, 4)                  # every term once; the empty constraint is on no slot
    assert [(r[0], r[2], r[3]) for r in recs if r[2]] == [(1, 1, 0), (2, 1, 1), (3, 2, 2), (5, 1, 4), (6, 3, 5), (9, 1, 8), (30, 1, 9), (31, 1, 10)]
    assert [r[1] for r in recs] == [k for k in kinds for _ in range(l)] and all(r[4] == er.le32(w[r[0]]) for r in recs)
    # slot 6: constraint 1 three times -- index 2 twice, then the special; slot 3: w - w, the specials in unsigned order
    assert [t[:4] for t in terms[5:8]] == [(6, 1, 2, 4), (6, 1, 2, 4), (6, 1, lr.ONE, 4)] and terms[5] == terms[6]
    assert [t[:4] for t in terms[2:4]] == [(3, 3, lr.NEG_ONE, 2), (3, 3, lr.ONE, 2)]
    assert all(t[5] == bytes(32) for t in terms) and terms[5][4] == er.le32(P - 3)
    # the same multiset of (constraint, slot, coef_index) as explain_ref over all constraints
    _, _, _, eterms = er.explain(system, rows, l, range(5), 100)
    assert sorted((t[1], t[0], t[2]) for t in terms) == sorted((t[0], t[1], t[2]) for t in eterms)
    # a changed witness: every constraint through the slot carries explain_ref's residual, the others zero
    bad = rows.copy()
    bad[0, 6] = ol.to_limbs([(w[6] + 5) % P])[0]
    res = er.residuals(system, bad, l, range(5))
    _, _, _, recs2, terms2 = sr.explain_slots(system, kinds, bad, l, [1, 5, 6], 100)
    assert [(t[0], t[1], int.from_bytes(t[5], "little")) for t in terms2] == [(1, 1, res[1]), (5, 0, 0), (6, 1, res[1]), (6, 1, res[1]), (6, 1, res[1])]
    assert res[1] != 0 and recs2[2][4] == er.le32((w[6] + 5) % P)
    # a cap inside a slot: the slot records stay complete
    total, rep, distinct, recs3, terms3 = sr.explain_slots(system, kinds, bad, l, [5, 6, 30], 2)
    assert (total, rep, distinct, len(terms3)) == (5, 2, 3, 2) and [(r[2], r[3]) for r in recs3] == [(1, 0), (3, 1), (1, 4)]
    # untouched: 32 slots, 8 distinct ones touched; a zeroed untouched slot drops out of nonzero_only alone
    touched = sorted(set(system.slots))
    assert len(touched) == 8
    n, nz, rep, out = sr.untouched(system, kinds, rows, l, False, 100)
    assert (n, nz, rep) == (24, 24, 24) and [o[0] for o in out] == [s for s in range(32) if s not in touched]
    z = rows.copy()
    z[0, 0] = 0
    z[0, 1] = 0                                                   # (slot 1 is touched: not counted either way)
    assert sr.untouched(system, kinds, z, l, False, 3)[:3] == (24, 23, 3) and sr.untouched(system, kinds, z, l, True, 100)[:3] == (24, 23, 23)
    assert sr.untouched(system, kinds, z, l, True, 100)[3][0][0] == 4 and sr.untouched(system, kinds, z, l, False, 1)[3] == [(0, 0, bytes(32))]
    assert sr.untouched(system, [0, 4, 2, 5], rows, l, False, 100)[0] == 16 - 5      # batch-kind rows are not covered
    empty = lr.System([0], [], [], [], [], [], 0)
    assert sr.untouched(empty, kinds, rows, l, False, 0)[:3] == (32, 32, 0)
