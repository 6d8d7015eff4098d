"""lig_rows_explain / lig_rows_explain_attached / lig_rows_read_slots without a GPU: the entries are exported and their ctypes signatures
are the header's declarations, the Python methods have the documented parameters, the argument checks that come before any trace or
device is looked at answer, no struct of the ABI changed size, and the reference of the GPU tests (tests/explain_ref.py) agrees with the
reference of lig_rows_diagnose (tests/diagnose_ref.py) on the residuals."""
import ctypes as C
import inspect
import os
import re

import numpy as np
import pytest

import diagnose_ref as dr
import explain_ref as er
import hip_lib
import linear_ref as lr
import oracle_lib as ol

ROOT = hip_lib.ROOT
P = ol.P
E_ARG = -1
NEW = ["lig_rows_explain", "lig_rows_explain_attached", "lig_rows_read_slots"]


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


def explain_info(amd, short=0):
    info = amd.ExplainInfo()
    info.struct_bytes = C.sizeof(amd.ExplainInfo) - short
    return info


def test_signatures_match_the_header(amd):
    L = amd.load_library()
    attached = declaration("lig_rows_explain_attached")
    assert attached == [("lig_trace*", "trace"), ("const uint32_t*", "constraints"), ("uint64_t", "n_asked"), ("lig_explain_constraint*", "con_out"),
                        ("lig_explain_term*", "terms_out"), ("uint64_t", "term_cap"), ("lig_explain_info*", "info")]
    # lig_rows_explain without its system: the same parameters in the same order
    assert attached == [p for p in declaration("lig_rows_explain") if p[1] != "sys"]
    assert declaration("lig_rows_explain")[1] == ("const lig_linear_system*", "sys")
    assert declaration("lig_rows_read_slots") == [("lig_trace*", "trace"), ("const uint32_t*", "slots"), ("uint64_t", "n_slots"), ("uint8_t*", "values")]
    ctype = {"lig_trace*": C.c_void_p, "const uint32_t*": C.c_void_p, "uint8_t*": C.c_void_p, "lig_explain_constraint*": C.c_void_p,
             "lig_explain_term*": C.c_void_p, "uint64_t": C.c_uint64, "lig_explain_info*": C.POINTER(amd.ExplainInfo),
             "const lig_linear_system*": C.POINTER(amd.LinearSystem)}
    for name in NEW:
        fn = getattr(L, name)
        assert list(fn.argtypes) == [ctype[ty] for ty, _ in declaration(name)], name
        assert fn.restype is C.c_int


def test_exports_are_in_sync(amd):
    assert all(name in amd.EXPORTS for name in NEW) and len(set(amd.EXPORTS)) == len(amd.EXPORTS)
    declared = set(re.findall(r"\b(lig_\w+)\s*\(", header()))
    assert set(NEW) <= declared
    L = amd.load_library()
    for name in amd.EXPORTS:                                      # every name of the list resolves in the library
        getattr(L, name)


def test_python_methods(amd):
    sig = inspect.signature(amd.Context.rows_explain)
    assert list(sig.parameters) == ["self", "trace", "system", "constraints", "term_cap"]
    att = inspect.signature(amd.Context.rows_explain_attached)
    assert list(att.parameters) == ["self", "trace", "constraints", "term_cap"]
    assert sig.parameters["term_cap"].default == att.parameters["term_cap"].default == 4096
    assert [p for p in sig.parameters if p != "system"] == list(att.parameters)
    assert list(inspect.signature(amd.Context.rows_read_slots).parameters) == ["self", "trace", "slots"]


def test_argument_errors_before_any_trace_is_looked_at(amd):
    L = amd.load_library()
    asked = np.zeros(1, dtype=np.uint32)
    con, terms = np.zeros(1, dtype=amd.EXPLAIN_CONSTRAINT), np.zeros(4, dtype=amd.EXPLAIN_TERM)
    vals = np.zeros((1, 8), dtype=np.uint32)
    p = lambda a: a.ctypes.data_as(C.c_void_p)
    # a NULL trace
    assert L.lig_rows_explain_attached(None, p(asked), 1, p(con), p(terms), 4, C.byref(explain_info(amd))) == E_ARG
    assert L.lig_rows_explain(None, None, p(asked), 1, p(con), p(terms), 4, C.byref(explain_info(amd))) == E_ARG
    assert L.lig_rows_read_slots(None, p(asked), 1, p(vals)) == E_ARG
    assert L.lig_rows_read_slots(None, None, 0, None) == E_ARG
    # a NULL or short info, a NULL array with a count > 0: decided before the trace is dereferenced (the "trace" is zeroed memory)
    fake = np.zeros(1 << 16, dtype=np.uint8)
    for call, head in ((L.lig_rows_explain_attached, (p(fake),)), (L.lig_rows_explain, (p(fake), None))):
        assert call(*head, p(asked), 1, p(con), p(terms), 4, None) == E_ARG
        assert call(*head, p(asked), 1, p(con), p(terms), 4, C.byref(explain_info(amd, short=8))) == E_ARG
        assert call(*head, p(asked), 1, None, p(terms), 4, C.byref(explain_info(amd))) == E_ARG
        assert call(*head, None, 1, p(con), p(terms), 4, C.byref(explain_info(amd))) == E_ARG
        assert call(*head, p(asked), 1, p(con), None, 4, C.byref(explain_info(amd))) == E_ARG
    assert L.lig_rows_read_slots(p(fake), None, 1, p(vals)) == E_ARG
    assert L.lig_rows_read_slots(p(fake), p(asked), 1, None) == E_ARG
    # (the range and state errors on a REAL trace: tests/test_gpu_explain.py)


def test_abi_sizes_are_unchanged(amd):
    L = amd.load_library()
    sizes = (C.c_uint32 * 6)()
    L.lig_abi_sizes(sizes)
    # lig_batch_op, lig_synth_job, lig_proof_info, lig_verify_info, lig_rows_job, lig_comm
    assert list(sizes) == [32, 192, 184, 56, 168, 64]
    assert re.search(r"LIG_ABI_STRUCTS\s*=\s*6\b", header())
    assert amd.EXPLAIN_TERM.itemsize == 80 and amd.EXPLAIN_CONSTRAINT.itemsize == 88 and C.sizeof(amd.ExplainInfo) == 32
    assert C.sizeof(amd.DiagInfo) == 48 and amd.DIAG_LINEAR.itemsize == 40 and amd.DIAG_QUAD.itemsize == 48
    assert [amd.EXPLAIN_TERM.fields[f][1] for f in ("constraint", "slot", "coef_index", "reserved", "coef", "value")] == [0, 4, 8, 12, 16, 48]
    assert [amd.EXPLAIN_CONSTRAINT.fields[f][1] for f in ("constraint", "reserved", "n_terms", "first_term", "rhs", "residual")] == [0, 4, 8, 16, 24, 56]


def small_case():
    """4 rows x 8 slots of seeded elements (k = 12); constraints: table and special coefficients with a right-hand side, a slot named three
    times (twice with one index), an empty one, one without a right-hand side"""
    l, k = 8, 12
    rng = np.random.default_rng(5)
    rows = np.zeros((4, k, 8), dtype=np.uint32)
    rows[:, :l] = ol.rand_field(rng, 4 * l).reshape(4, l, 8)
    w = lr.witness(rows, l)
    tab = [7, (1 << 250) + 9, P - 3]
    cons = [[(5, 0), (2, lr.ONE), (31, 1), (9, lr.NEG_ONE)], [(6, 2), (6, lr.ONE), (6, 2), (1, 0)], [], [(3, lr.ONE), (3, lr.NEG_ONE)], [(30, 1)]]
    val = lambda ci: 1 if ci == lr.ONE else P - 1 if ci == lr.NEG_ONE else tab[ci]
    term_begin, slots, cidx, rhs_c, rhs_b, coefs = [0], [], [], [], [], list(tab)
    for cn, terms in enumerate(cons):
        slots += [s for s, _ in terms]
        cidx += [ci for _, ci in terms]
        term_begin.append(len(slots))
        b = sum(val(ci) * w[s] for s, ci in terms) % P
        if b:
            rhs_c.append(cn)
            rhs_b.append(len(coefs))
            coefs.append(b)
    return lr.System(term_begin, slots, cidx, rhs_c, rhs_b, coefs, 0), rows, l, w


def test_reference_agrees_with_the_diagnose_reference():
    system, rows, l, w = small_case()
    assert dr.linear_violations(system, rows, l) == []
    total, rep, cons, terms = er.explain(system, rows, l, range(5), 100)
    assert (total, rep) == (11, 11) and [c[1] for c in cons] == [4, 4, 0, 2, 1] and [c[2] for c in cons] == [0, 4, 8, 8, 10]
    assert all(c[4] == bytes(32) for c in cons)                   # satisfied: zero residuals
    assert cons[2][3] == bytes(32) and cons[3][3] == bytes(32)    # the empty constraint and w - w: no right-hand side
    # the order: slot, then index as an unsigned number (the specials last); the repeated term twice
    assert [(t[1], t[2]) for t in terms[:8]] == [(2, lr.ONE), (5, 0), (9, lr.NEG_ONE), (31, 1), (1, 0), (6, 2), (6, 2), (6, lr.ONE)]
    assert terms[5] == terms[6] and terms[3][3] == er.le32((1 << 250) + 9) and terms[3][4] == er.le32(w[31])
    assert terms[2][3] == er.le32(P - 1) and terms[0][3] == er.le32(1)
    # a changed witness: the residual of diagnose_ref on the violated constraints, zero on the others
    bad = rows.copy()
    bad[0, 6] = ol.to_limbs([(w[6] + 5) % P])[0]                  # slot 6: constraint 1, coefficients (P - 3) twice and 1
    bad[3, 6] = ol.to_limbs([(w[30] + P - 1) % P])[0]             # slot 30: constraint 4, coefficient 2^250 + 9
    viol = dict(dr.linear_violations(system, bad, l))
    assert sorted(viol) == [1, 4] and viol[1] == 5 * (2 * (P - 3) + 1) % P
    assert er.residuals(system, bad, l, range(5)) == {c: viol.get(c, 0) for c in range(5)}
    assert er.residuals(system, bad, l, [1, 4]) == viol
    # a cap inside a constraint: the constraint records stay complete
    total, rep, cons2, terms2 = er.explain(system, bad, l, [0, 1, 4], 6)
    assert (total, rep, len(terms2)) == (9, 6, 6) and [c[1:3] for c in cons2] == [(4, 0), (4, 4), (1, 8)]
    assert terms2[5][4] == er.le32((w[6] + 5) % P)
    assert (er.slot_values(bad, l, [30, 6, 30]) == bad[[3, 0, 3], [6, 6, 6]]).all()
