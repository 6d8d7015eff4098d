"""ligero-prover_amd -- ctypes binding of liblig_hip.so (the MI355X-native Ligero prover backend).

This is a thin loader for tests and bench.py; the product is the C-ABI library (include/lig_hip.h) and the
C++ `hip_context` mirror of the reference's `webgpu_context` (include/lig_hip_context.hpp).  There is NO CPU
fallback: if the HIP library is missing or no GPU is visible, construction raises.

The directory name contains a hyphen, so import it by path:
    spec = importlib.util.spec_from_file_location("ligero_prover_amd", ".../ligero-prover_amd/__init__.py")
(tests/hip_lib.py and bench.py do exactly that).
"""
import ctypes as C
import os

import numpy as np

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.environ.get("LIG_HIP_LIB") or os.path.join(_HERE, "liblig_hip.so")      # LIG_HIP_LIB: A/B builds of experiments

OPS = dict(ADD=0, SUB=1, ADD_ASSIGN=2, ADD_CONST=3, SUB_CONST=4, CONST_SUB=5, MUL=6, MUL_CONST=7,
           MONTMUL_CONST=8, FMA=9, FMA_CONST=10, DIV=11, BIT_DECOMPOSE=12)
SIZE_K, SIZE_2K, SIZE_N = 0, 1, 2

EXPORTS = [
    "lig_ctx_create", "lig_ctx_destroy", "lig_sync", "lig_last_error", "lig_version", "lig_message_size",
    "lig_padding_size", "lig_encoding_size", "lig_stream", "lig_malloc", "lig_free", "lig_write", "lig_write_clear",
    "lig_clear", "lig_copy", "lig_read", "lig_encode", "lig_encode_2k", "lig_decode", "lig_ntt", "lig_eltwise",
    "lig_powmod", "lig_sha_state_bytes", "lig_sha_init", "lig_sha_update", "lig_sha_final", "lig_sample_init",
    "lig_sample_gather", "lig_encode_rows", "lig_sha_update_rows", "lig_merkle_nodes", "lig_merkle_build",
    "lig_rlc_rows", "lig_gather_rows", "lig_rng_fill", "lig_profile_enable", "lig_profile_read",
    "lig_synth_prepare", "lig_synth_prove", "lig_trace_rows", "lig_trace_destroy",
    "lig_shard_prepare", "lig_shard_prove", "lig_shard_destroy", "lig_synth_verify", "lig_verify_release",
    "lig_proof_gzip_bound", "lig_proof_gzip", "lig_proof_gunzip_size", "lig_proof_gunzip",
    "lig_rows_begin", "lig_rows_commit", "lig_rows_prove", "lig_rows_restart", "lig_rng_fill_rows",
    "lig_rows_verify_begin", "lig_rows_verify_finish", "lig_vtrace_destroy",
    "lig_public_arg_bytes", "lig_instance_hash", "lig_sample_columns",
    "lig_rccl_unique_id", "lig_rccl_comm_create", "lig_rccl_comm_destroy", "lig_rccl_available", "lig_rccl_comm_count",
    "lig_shard_plan", "lig_ipc_comm_create", "lig_ipc_comm_destroy",
    "lig_device_pci_bus_id", "lig_device_peer_access", "lig_host_alloc", "lig_host_free", "lig_write_async", "lig_fence_record", "lig_fence_wait", "lig_fence_destroy", "lig_rows_push_rands", "lig_rows_push_rands_sparse",
    "lig_abi_sizes", "lig_shard_rows_plan", "lig_shard_rows_begin", "lig_shard_rows_restart", "lig_shard_rows_commit", "lig_shard_rows_prove",
    "lig_upload_health", "lig_profile_read_launches",
    "lig_linear_check", "lig_linear_form", "lig_rows_set_linear", "lig_rows_verify_set_linear",
    "lig_shard_rows_set_linear", "lig_shard_rows_linear_stats", "lig_linear_shard_count", "lig_shard_rows_diagnose",
    "lig_linear_prepare", "lig_linear_program_release", "lig_linear_program_bytes", "lig_rows_attach_linear", "lig_rows_verify_attach_linear",
    "lig_rows_set_linear_values", "lig_rows_verify_set_linear_values", "lig_linear_program_form",
    "lig_rows_diagnose", "lig_rows_diagnose_attached",
    "lig_rows_explain", "lig_rows_explain_attached", "lig_rows_read_slots",
    "lig_rows_explain_slots", "lig_rows_explain_slots_attached", "lig_rows_untouched_slots", "lig_rows_untouched_slots_attached",
    "lig_shard_rows_explain", "lig_shard_rows_read_slots", "lig_shard_rows_explain_attached",
    "lig_shard_rows_set_linear_values", "lig_shard_rows_diagnose_attached",
    "lig_shard_rows_explain_slots", "lig_shard_rows_explain_slots_attached", "lig_shard_rows_untouched_slots", "lig_shard_rows_untouched_slots_attached",
    "lig_derived_check", "lig_rows_set_derived",
    "lig_derived_shard_count", "lig_shard_rows_set_derived",
]

ROW_KINDS = dict(LINEAR=0, QX=1, QY=2, QZ=3, INIT=4, BIT=5, EQX=6, EQY=7, BQX=8, BQY=9, BQZ=10)
ROW_DRAW_PAD = 0x80
ELEM_BIT = 0x81            # lig_rows_job.elem_bytes: the row's data slots are bits (LIG_ELEM_BIT)
ELEM_PRODUCT = 0x82        # ... the QZ row of a triple is not shipped: the library forms x * y mod p on the device (LIG_ELEM_PRODUCT)
ROWS_JOB_WIDE = 1          # lig_rows_job.reserved: the struct has wide_per_row (LIG_ROWS_JOB_WIDE)
WIDE_RECORD_BYTES = 36     # lig_rows_job.wide_per_row: a record of a mixed row, uint32 column + 8 uint32 limbs (LIG_WIDE_RECORD_BYTES)
ARG_I64, ARG_STR, ARG_HEX = 0, 1, 2
COEF_ONE, COEF_NEG_ONE = 0xFFFFFFFF, 0xFFFFFFFE      # lig_lin_term.coef values that need no table entry (LIG_COEF_ONE / LIG_COEF_NEG_ONE)
DERIVE_MAX_WAVES = 16      # lig_rows_set_derived: a derived slot may read derived slots of at most this many earlier waves (LIG_DERIVE_MAX_WAVES)
DERIVED_PRODUCT = 0xFFFFFFFF      # the `constraint` of a product entry (slot, DERIVED_PRODUCT): slot = column i of an ELEM_PRODUCT row, re-formed as x_i * y_i from the matrix in wave order (LIG_DERIVED_PRODUCT)


class VerifyInfo(C.Structure):
    _fields_ = [(n, C.c_int32) for n in ("parsed", "indices_match", "valid_merkle", "valid_code", "valid_linear", "valid_quad",
                                          "code_equal", "linear_equal", "quad_equal", "accept", "reserved")] + [("ms_total", C.c_double)]

A2A_FN = C.CFUNCTYPE(C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_size_t)


A2A_ON_FN = C.CFUNCTYPE(C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_size_t, C.c_void_p)


class Comm(C.Structure):
    """lig_comm: host-synchronous callbacks (tests over gloo) and, when made by lig_rccl_comm_create, the stream-ordered RCCL forms"""
    _fields_ = [("user", C.c_void_p), ("all_to_all", A2A_FN), ("all_gather", A2A_FN),
                ("all_to_all_on", A2A_ON_FN), ("all_gather_on", A2A_ON_FN), ("forget", C.CFUNCTYPE(None, C.c_void_p)),
                ("failed", C.CFUNCTYPE(C.c_int, C.c_void_p)), ("abort", C.CFUNCTYPE(None, C.c_void_p))]


class SynthJob(C.Structure):
    _fields_ = [("n_linear", C.c_uint64), ("n_quad", C.c_uint64), ("encoding_seed", C.c_uint8 * 32),
                ("witness_key", C.c_uint8 * 32), ("program_hash", C.c_uint8 * 32), ("generated_at", C.c_int64),
                ("version", C.c_char * 16),
                ("batch_ops", C.c_void_p), ("n_batch_ops", C.c_uint64), ("batch_data", C.c_void_p), ("batch_data_bytes", C.c_uint64),
                ("public_args", C.c_void_p), ("public_arg_lens", C.c_void_p), ("n_public_args", C.c_uint64)]

    def set_public_args(self, args):
        """args: list of byte strings in input_args form (see public_arg_bytes); kept alive on the job object"""
        _attach_public_args(self, args)


class RowsJob(C.Structure):
    _fields_ = [("rows", C.c_uint64), ("kinds", C.c_void_p), ("msgs", C.c_void_p), ("msgs_on_device", C.c_int32),
                ("reserved", C.c_int32), ("encoding_seed", C.c_uint8 * 32), ("program_hash", C.c_uint8 * 32),
                ("generated_at", C.c_int64), ("version", C.c_char * 16),
                ("public_args", C.c_void_p), ("public_arg_lens", C.c_void_p), ("n_public_args", C.c_uint64),
                ("dense_rands_per_row", C.c_void_p), ("elem_bytes", C.c_void_p), ("wide_per_row", C.c_void_p)]

    def set_public_args(self, args):
        _attach_public_args(self, args)


def _attach_public_args(job, args):
    args = [bytes(a) for a in (args or [])]
    blob = np.frombuffer(b"".join(args) or b"\0", dtype=np.uint8).copy()
    lens = np.array([len(a) for a in args] or [0], dtype=np.uint64)
    job._pub_keep = (blob, lens)
    job.public_args = blob.ctypes.data if args else None
    job.public_arg_lens = lens.ctypes.data if args else None
    job.n_public_args = len(args)


class LinearSystem(C.Structure):
    """lig_linear_system: linear constraints sum_j a_cj * w[slot_cj] = b_c as a sparse term list of integers (include/lig_hip.h).
    Build it with LinearSystem.make(...): the arrays are kept alive on the object."""
    _fields_ = [("struct_bytes", C.c_uint32), ("reserved", C.c_uint32), ("n_constraints", C.c_uint64), ("n_terms", C.c_uint64),
                ("term_begin", C.c_void_p), ("terms", C.c_void_p), ("rhs_constraint", C.c_void_p), ("rhs_coef", C.c_void_p),
                ("n_rhs", C.c_uint64), ("coefs", C.c_void_p), ("n_coefs", C.c_uint64), ("first_random", C.c_uint64)]

    @classmethod
    def make(cls, term_begin, slots, coef_idx, rhs_constraint=(), rhs_coef=(), coefs=(), first_random=0):
        """term_begin: n_constraints + 1 offsets into the terms; slots / coef_idx: one entry per term (slot = row * l + column;
        coefficient = index into `coefs`, COEF_ONE or COEF_NEG_ONE); rhs_constraint / rhs_coef: the constraints with b_c != 0,
        ascending, and the coefficient index of b_c; coefs: the table, Python integers in [0, p) or an (n, 8) uint32 array"""
        sys_ = cls()
        tb = np.ascontiguousarray(term_begin, dtype=np.uint32)
        slots, coef_idx = np.asarray(slots, dtype=np.uint32), np.asarray(coef_idx, dtype=np.uint32)
        assert slots.shape == coef_idx.shape and slots.ndim == 1 and tb.ndim == 1 and len(tb) >= 1
        terms = np.empty((len(slots), 2), dtype=np.uint32)
        terms[:, 0], terms[:, 1] = slots, coef_idx
        rc, rb = np.ascontiguousarray(rhs_constraint, dtype=np.uint32), np.ascontiguousarray(rhs_coef, dtype=np.uint32)
        assert rc.shape == rb.shape and rc.ndim == 1
        if isinstance(coefs, np.ndarray):
            tab = np.ascontiguousarray(coefs, dtype=np.uint32).reshape(-1, 8)
        else:
            tab = np.frombuffer(b"".join(int(v).to_bytes(32, "little") for v in coefs), dtype=np.uint32).reshape(-1, 8).copy()
        sys_._keep = (tb, terms, rc, rb, tab)
        sys_.struct_bytes = C.sizeof(cls)
        sys_.n_constraints, sys_.n_terms, sys_.n_rhs, sys_.n_coefs = len(tb) - 1, len(terms), len(rc), len(tab)
        sys_.term_begin = tb.ctypes.data
        sys_.terms = terms.ctypes.data if len(terms) else None
        sys_.rhs_constraint = rc.ctypes.data if len(rc) else None
        sys_.rhs_coef = rb.ctypes.data if len(rb) else None
        sys_.coefs = tab.ctypes.data if len(tab) else None
        sys_.first_random = first_random
        return sys_


def linear_check(system, kinds, l):
    """lig_linear_check (host only) -> the return code: 0, or LIG_E_ARG (-1) for a system that breaks a rule of the format"""
    kinds = np.ascontiguousarray(kinds, dtype=np.uint8)
    return load_library().lig_linear_check(C.byref(system), kinds.ctypes.data if len(kinds) else None, len(kinds), l)


class DerivedInfo(C.Structure):
    """lig_derived_info: n_slots = the listed slots, n_terms = the other terms of all defining constraints + 2 per product entry, n_waves"""
    _fields_ = [("struct_bytes", C.c_uint32), ("reserved", C.c_uint32), ("n_slots", C.c_uint64), ("n_terms", C.c_uint64),
                ("n_waves", C.c_uint32), ("reserved2", C.c_uint32)]


def _derived_pairs(pairs):
    """(slot, defining constraint) pairs -> the (n, 2) uint32 array of lig_derived_slot"""
    d = np.ascontiguousarray(pairs, dtype=np.uint32).reshape(-1, 2)
    return d


def derived_check(system, kinds, l, pairs, elem_bytes=None):
    """lig_derived_check (host only): pairs = (slot, defining constraint) of every derived slot and (slot, DERIVED_PRODUCT) of every product
    entry, any order; elem_bytes: the widths of the
    rows job or None -> the wave of every pair (uint32 array, 1 = reads no derived slot); LigError(-1) for a list the rules refuse"""
    kinds = np.ascontiguousarray(kinds, dtype=np.uint8)
    d = _derived_pairs(pairs)
    eb = np.ascontiguousarray(elem_bytes, dtype=np.uint8) if elem_bytes is not None else None
    if eb is not None and len(eb) != len(kinds):
        raise ValueError("derived_check: %d widths for %d rows" % (len(eb), len(kinds)))
    waves = np.zeros(len(d), dtype=np.uint32)
    rc = load_library().lig_derived_check(C.byref(system), kinds.ctypes.data if len(kinds) else None, len(kinds), l,
                                          eb.ctypes.data if eb is not None and len(eb) else None, d.ctypes.data if len(d) else None, len(d),
                                          waves.ctypes.data if len(d) else None, None)
    if rc != 0:
        raise LigError("lig_derived_check failed (%d)" % rc)
    return waves


class DerivedShardInfo(C.Structure):
    """lig_derived_shard_info: n_slots, n_terms, n_waves of the whole list, n_exchanges = its waves with an all-gather; of this rank:
    local_targets, local_terms + imported_terms (the other terms of its targets), imports = distinct foreign slots read, exports = slots
    sent, exchange_bytes = what it receives per commit"""
    _fields_ = [("struct_bytes", C.c_uint32), ("reserved", C.c_uint32), ("n_slots", C.c_uint64), ("n_terms", C.c_uint64),
                ("n_waves", C.c_uint32), ("n_exchanges", C.c_uint32), ("local_targets", C.c_uint64), ("local_terms", C.c_uint64),
                ("imported_terms", C.c_uint64), ("imports", C.c_uint64), ("exports", C.c_uint64), ("exchange_bytes", C.c_uint64)]

    def as_dict(self):
        return {name: int(getattr(self, name)) for name, _ in self._fields_ if not name.startswith("reserved") and name != "struct_bytes"}


def derived_shard_count(system, kinds, l, pairs, elem_bytes, rank, world):
    """lig_derived_shard_count (host only): what lig_shard_rows_set_derived reports on `rank` of `world` for the list `pairs` under the deal
    of shard_rows_plan -> DerivedShardInfo; LigError(-1) for rank >= world, world == 0 or a list lig_derived_check refuses"""
    kinds = np.ascontiguousarray(kinds, dtype=np.uint8)
    d = _derived_pairs(pairs)
    eb = np.ascontiguousarray(elem_bytes, dtype=np.uint8) if elem_bytes is not None else None
    if eb is not None and len(eb) != len(kinds):
        raise ValueError("derived_shard_count: %d widths for %d rows" % (len(eb), len(kinds)))
    info = DerivedShardInfo()
    info.struct_bytes = C.sizeof(DerivedShardInfo)
    rc = load_library().lig_derived_shard_count(C.byref(system), kinds.ctypes.data if len(kinds) else None, len(kinds), l,
                                                eb.ctypes.data if eb is not None and len(eb) else None, d.ctypes.data if len(d) else None, len(d),
                                                rank, world, C.byref(info))
    if rc != 0:
        raise LigError("lig_derived_shard_count failed (%d)" % rc)
    return info


def linear_shard_count(system, kinds, l, rank, world):
    """lig_linear_shard_count (host only) -> (local_terms, needed_constraints): the terms of `system` that `rank` of `world` keeps under
    the deal of shard_rows_plan, and the distinct stream elements it samples per proof; LigError(-1) for rank >= world, world == 0 or a
    system lig_linear_check rejects"""
    kinds = np.ascontiguousarray(kinds, dtype=np.uint8)
    lt, nc = C.c_uint64(), C.c_uint64()
    rc = load_library().lig_linear_shard_count(C.byref(system), kinds.ctypes.data if len(kinds) else None, len(kinds), l, rank, world, C.byref(lt), C.byref(nc))
    if rc != 0:
        raise LigError("lig_linear_shard_count failed (%d)" % rc)
    return int(lt.value), int(nc.value)


def coef_table(coefs):
    """a coefficient table as the (n, 8) uint32 array the library reads: Python integers in [0, 2^256) or an array of limbs"""
    if isinstance(coefs, np.ndarray):
        return np.ascontiguousarray(coefs, dtype=np.uint32).reshape(-1, 8)
    return np.frombuffer(b"".join(int(v).to_bytes(32, "little") for v in coefs), dtype=np.uint32).reshape(-1, 8).copy()


class LinearProgram:
    """lig_linear_program: a prepared linear system (Context.linear_prepare) -- immutable, reference counted by the library, bound to a
    device and (l, k).  This object is the CALLER's reference: release() (or leaving a `with` block) drops it exactly once; traces it
    was attached to keep the structure alive for as long as they need it."""

    def __init__(self, lib, handle):
        self._lib, self.h = lib, handle

    def release(self):
        h, self.h = self.h, None
        if h:
            self._lib.lig_linear_program_release(h)

    def bytes(self):
        """-> (device bytes the program holds, device bytes every attachment adds)"""
        pb, ab = C.c_uint64(), C.c_uint64()
        if self._lib.lig_linear_program_bytes(self._handle(), C.byref(pb), C.byref(ab)) != 0:
            raise LigError("lig_linear_program_bytes failed")
        return int(pb.value), int(ab.value)

    def _handle(self):
        if not self.h:
            raise LigError("the linear program has been released")
        return self.h

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.release()

    def __del__(self):
        try:
            self.release()
        except Exception:
            pass


class DiagInfo(C.Structure):
    """lig_diag_info: the counts cover every violation, the *_reported ones what fitted the caps"""
    _fields_ = [("struct_bytes", C.c_uint32), ("reserved", C.c_uint32), ("n_linear_bad", C.c_uint64), ("n_quad_bad", C.c_uint64),
                ("n_linear_reported", C.c_uint64), ("n_quad_reported", C.c_uint64), ("ms_total", C.c_double)]


# lig_diag_linear (40 bytes) / lig_diag_quad (48 bytes) as numpy records; residual = 32 little-endian bytes, canonical
DIAG_LINEAR = np.dtype([("constraint", "<u4"), ("reserved", "<u4"), ("residual", "u1", (32,))])
DIAG_QUAD = np.dtype([("row_x", "<u4"), ("row_y", "<u4"), ("row_z", "<u4"), ("column", "<u4"), ("residual", "u1", (32,))])


class ExplainInfo(C.Structure):
    """lig_explain_info: n_terms_total covers every term of the asked constraints, n_terms_reported what fitted term_cap"""
    _fields_ = [("struct_bytes", C.c_uint32), ("reserved", C.c_uint32), ("n_terms_total", C.c_uint64), ("n_terms_reported", C.c_uint64),
                ("ms_total", C.c_double)]


# lig_explain_term (80 bytes) / lig_explain_constraint (88 bytes) as numpy records; coef, value, rhs, residual = 32 little-endian bytes, canonical
EXPLAIN_TERM = np.dtype([("constraint", "<u4"), ("slot", "<u4"), ("coef_index", "<u4"), ("reserved", "<u4"), ("coef", "u1", (32,)),
                         ("value", "u1", (32,))])
EXPLAIN_CONSTRAINT = np.dtype([("constraint", "<u4"), ("reserved", "<u4"), ("n_terms", "<u8"), ("first_term", "<u8"), ("rhs", "u1", (32,)),
                               ("residual", "u1", (32,))])


class SlotInfo(C.Structure):
    """lig_slot_info: n_terms_total covers every term on the asked slots, n_terms_reported what fitted term_cap, n_constraints_distinct the
    distinct constraints over all asked slots"""
    _fields_ = [("struct_bytes", C.c_uint32), ("reserved", C.c_uint32), ("n_terms_total", C.c_uint64), ("n_terms_reported", C.c_uint64),
                ("n_constraints_distinct", C.c_uint64), ("ms_total", C.c_double)]


class UntouchedInfo(C.Structure):
    """lig_untouched_info: n_untouched / n_untouched_nonzero count every LINEAR .. QZ slot no term touches (with a nonzero committed value),
    n_reported what fitted cap"""
    _fields_ = [("struct_bytes", C.c_uint32), ("reserved", C.c_uint32), ("n_untouched", C.c_uint64), ("n_untouched_nonzero", C.c_uint64),
                ("n_reported", C.c_uint64), ("ms_total", C.c_double)]


# lig_slot_record (56 bytes) / lig_slot_term (80 bytes) / lig_slot_value (40 bytes) as numpy records; value, coef, residual = 32 little-endian
# bytes, canonical
SLOT_RECORD = np.dtype([("slot", "<u4"), ("row_kind", "<u4"), ("n_terms", "<u8"), ("first_term", "<u8"), ("value", "u1", (32,))])
SLOT_TERM = np.dtype([("slot", "<u4"), ("constraint", "<u4"), ("coef_index", "<u4"), ("constraint_terms", "<u4"), ("coef", "u1", (32,)),
                      ("residual", "u1", (32,))])
SLOT_VALUE = np.dtype([("slot", "<u4"), ("row_kind", "<u4"), ("value", "u1", (32,))])


class ProofInfo(C.Structure):
    _fields_ = [("root", C.c_uint8 * 32), ("stage1_seed", C.c_uint8 * 32), ("stage2_seed", C.c_uint8 * 32),
                ("const_sum", C.c_uint8 * 32), ("rows", C.c_uint64), ("valid_code", C.c_int32),
                ("valid_linear", C.c_int32), ("valid_quad", C.c_int32), ("reserved", C.c_int32),
                ("ms_stage1", C.c_double), ("ms_stage2", C.c_double), ("ms_stage3", C.c_double), ("ms_total", C.c_double)]


def build(force=False):
    """compile the HIP extension in-tree for gfx950 (hipcc cross-compiles without a GPU)"""
    import subprocess
    csrc = os.path.join(_HERE, "csrc")
    if force:
        subprocess.check_call(["make", "-C", csrc, "clean"], stdout=subprocess.DEVNULL)
    subprocess.check_call(["make", "-C", csrc, "-j8"], stdout=subprocess.DEVNULL)
    return LIB_PATH


def load_library():
    if not os.path.exists(LIB_PATH):
        raise RuntimeError("liblig_hip.so is missing (%s): run `python -c 'import __graft_entry__ as g; g.build()'` "
                           "-- there is no CPU fallback for the HIP path" % LIB_PATH)
    L = C.CDLL(LIB_PATH)
    vp, sz, u32, u64 = C.c_void_p, C.c_size_t, C.c_uint32, C.c_uint64
    # struct layouts of this binding against the library's own sizeof (include/lig_hip.h: lig_abi_sizes): a stale binding would hand the
    # library structs it reads past the end of
    sizes = (u32 * 6)()
    L.lig_abi_sizes.argtypes = [C.POINTER(u32)]
    L.lig_abi_sizes.restype = None
    L.lig_abi_sizes(sizes)
    for idx, (name, cls) in {1: ("lig_synth_job", SynthJob), 2: ("lig_proof_info", ProofInfo), 3: ("lig_verify_info", VerifyInfo),
                             4: ("lig_rows_job", RowsJob), 5: ("lig_comm", Comm)}.items():
        if C.sizeof(cls) != sizes[idx]:
            raise RuntimeError("binding out of date: sizeof(%s) is %d in %s, %d in this module" % (name, sizes[idx], LIB_PATH, C.sizeof(cls)))
    L.lig_ctx_create.argtypes = [C.POINTER(vp), C.c_int, u32, u32, u32]
    L.lig_ctx_destroy.argtypes = [vp]
    L.lig_ctx_destroy.restype = None
    L.lig_sync.argtypes = [vp]
    L.lig_last_error.argtypes = [vp]
    L.lig_last_error.restype = C.c_char_p
    L.lig_version.restype = C.c_char_p
    for f in ("lig_message_size", "lig_padding_size", "lig_encoding_size"):
        getattr(L, f).argtypes = [vp]
        getattr(L, f).restype = u32
    L.lig_stream.argtypes = [vp]
    L.lig_stream.restype = vp
    L.lig_malloc.argtypes = [vp, sz, C.POINTER(vp)]
    L.lig_free.argtypes = [vp, vp]
    L.lig_write.argtypes = [vp, vp, vp, sz]
    L.lig_write_clear.argtypes = [vp, vp, sz, vp, sz]
    L.lig_clear.argtypes = [vp, vp, sz]
    L.lig_copy.argtypes = [vp, vp, vp, sz]
    L.lig_read.argtypes = [vp, vp, vp, sz]
    for f in ("lig_encode", "lig_encode_2k", "lig_decode"):
        getattr(L, f).argtypes = [vp, vp]
    L.lig_ntt.argtypes = [vp, vp, C.c_int, C.c_int]
    L.lig_eltwise.argtypes = [vp, C.c_int, vp, vp, vp, sz, vp, u32]
    L.lig_powmod.argtypes = [vp, vp, vp, vp, vp, sz, C.c_int]
    L.lig_sha_state_bytes.argtypes = [sz]
    L.lig_sha_state_bytes.restype = sz
    L.lig_sha_init.argtypes = [vp, vp, sz]
    L.lig_sha_update.argtypes = [vp, vp, vp]
    L.lig_sha_final.argtypes = [vp, vp, vp]
    L.lig_sample_init.argtypes = [vp, vp, sz]
    L.lig_sample_gather.argtypes = [vp, vp, vp, sz]
    L.lig_encode_rows.argtypes = [vp, vp, vp, sz]
    L.lig_sha_update_rows.argtypes = [vp, vp, vp, sz]
    L.lig_merkle_nodes.argtypes = [sz]
    L.lig_merkle_nodes.restype = sz
    L.lig_merkle_build.argtypes = [vp, vp, sz, vp]
    L.lig_rlc_rows.argtypes = [vp, vp, vp, sz, vp, vp, vp, vp, vp, sz, vp]
    L.lig_gather_rows.argtypes = [vp, vp, sz, vp]
    L.lig_rng_fill.argtypes = [vp, vp, u64, vp, sz]
    L.lig_synth_prepare.argtypes = [vp, C.POINTER(SynthJob), C.POINTER(vp)]
    L.lig_synth_prove.argtypes = [vp, C.POINTER(C.POINTER(C.c_uint8)), C.POINTER(sz), C.POINTER(ProofInfo)]
    L.lig_trace_rows.argtypes = [vp]
    L.lig_trace_rows.restype = u64
    L.lig_trace_destroy.argtypes = [vp]
    L.lig_trace_destroy.restype = None
    L.lig_proof_gzip_bound.restype = sz
    L.lig_proof_gzip_bound.argtypes = [sz]
    L.lig_proof_gzip.argtypes = [vp, sz, vp, sz, C.POINTER(sz)]
    L.lig_proof_gunzip_size.restype = sz
    L.lig_proof_gunzip_size.argtypes = [vp, sz]
    L.lig_proof_gunzip.argtypes = [vp, sz, vp, sz, C.POINTER(sz)]
    L.lig_synth_verify.argtypes = [vp, C.POINTER(SynthJob), vp, vp, sz, C.POINTER(VerifyInfo)]
    L.lig_verify_release.argtypes = [vp]
    L.lig_shard_prepare.argtypes = [vp, C.POINTER(SynthJob), u32, u32, C.POINTER(Comm), C.POINTER(vp)]
    L.lig_shard_prove.argtypes = [vp, C.POINTER(C.POINTER(C.c_uint8)), C.POINTER(sz), C.POINTER(ProofInfo)]
    L.lig_shard_destroy.argtypes = [vp]
    L.lig_shard_destroy.restype = None
    L.lig_rows_begin.argtypes = [vp, C.POINTER(RowsJob), C.POINTER(vp)]
    L.lig_rows_commit.argtypes = [vp, vp, vp]
    L.lig_rows_restart.argtypes = [vp, vp, C.c_int]
    L.lig_rows_verify_begin.argtypes = [vp, C.POINTER(RowsJob), vp, sz, C.POINTER(vp), vp, C.POINTER(VerifyInfo)]
    L.lig_rows_verify_finish.argtypes = [vp, vp, C.c_int, vp, C.POINTER(VerifyInfo)]
    L.lig_vtrace_destroy.argtypes = [vp]
    L.lig_vtrace_destroy.restype = None
    L.lig_rows_prove.argtypes = [vp, vp, C.c_int, vp, C.POINTER(C.POINTER(C.c_uint8)), C.POINTER(sz), C.POINTER(ProofInfo)]
    L.lig_rng_fill_rows.argtypes = [vp, vp, u64, vp, sz, vp]
    L.lig_public_arg_bytes.argtypes = [C.c_int, C.c_char_p, vp, sz, C.POINTER(sz)]
    L.lig_instance_hash.argtypes = [vp, vp, sz, vp]
    L.lig_sample_columns.argtypes = [vp, u32, u32, vp]
    L.lig_rccl_unique_id.argtypes = [vp]
    L.lig_rccl_comm_create.argtypes = [vp, vp, u32, u32, C.POINTER(Comm)]
    L.lig_rccl_comm_destroy.argtypes = [C.POINTER(Comm)]
    L.lig_rccl_comm_destroy.restype = None
    L.lig_shard_rows_plan.argtypes = [vp, sz, u32, C.POINTER(u64), vp, sz]
    L.lig_shard_rows_begin.argtypes = [vp, C.POINTER(RowsJob), u32, u32, C.POINTER(Comm), C.POINTER(vp)]
    L.lig_shard_rows_restart.argtypes = [vp, vp, C.c_int]
    L.lig_shard_rows_commit.argtypes = [vp, vp, vp]
    L.lig_shard_rows_prove.argtypes = [vp, vp, C.c_int, vp, C.POINTER(C.POINTER(C.c_uint8)), C.POINTER(sz), C.POINTER(ProofInfo)]
    L.lig_ipc_comm_create.argtypes = [vp, C.c_char_p, u32, u32, C.POINTER(Comm)]
    L.lig_ipc_comm_destroy.argtypes = [C.POINTER(Comm)]
    L.lig_ipc_comm_destroy.restype = None
    L.lig_rccl_available.argtypes = [C.c_char_p, sz, C.POINTER(C.c_int)]
    L.lig_rccl_comm_count.argtypes = [C.POINTER(Comm), C.POINTER(u32)]
    L.lig_device_pci_bus_id.argtypes = [C.c_int, C.c_char_p, sz]
    L.lig_device_peer_access.argtypes = [C.c_int, C.c_int, C.POINTER(C.c_int)]
    L.lig_host_alloc.argtypes = [vp, sz, C.POINTER(vp)]
    L.lig_host_free.argtypes = [vp, vp]
    L.lig_write_async.argtypes = [vp, vp, vp, sz]
    L.lig_fence_record.argtypes = [vp, C.POINTER(vp)]
    L.lig_fence_wait.argtypes = [vp, vp]
    L.lig_fence_destroy.argtypes = [vp, vp]
    L.lig_fence_destroy.restype = None
    L.lig_rows_push_rands.argtypes = [vp, u64, u64, vp]
    L.lig_upload_health.argtypes = [vp, C.POINTER(u32), C.POINTER(u32)]
    L.lig_rows_push_rands_sparse.argtypes = [vp, u64, u64, vp, vp]
    L.lig_profile_enable.argtypes = [vp, C.c_int]
    L.lig_profile_read.argtypes = [vp, C.POINTER(u64), C.POINTER(u64), C.POINTER(C.c_double)]
    L.lig_profile_read_launches.argtypes = [vp, u32, C.POINTER(u64), C.POINTER(C.c_double)]
    L.lig_linear_check.argtypes = [C.POINTER(LinearSystem), vp, u64, u32]
    L.lig_linear_form.argtypes = [vp, C.POINTER(LinearSystem), vp, u64, vp, vp, vp]
    L.lig_derived_check.argtypes = [C.POINTER(LinearSystem), vp, u64, u32, vp, vp, u64, vp, C.POINTER(DerivedInfo)]
    L.lig_rows_set_derived.argtypes = [vp, C.POINTER(LinearSystem), vp, u64, C.POINTER(DerivedInfo)]
    L.lig_rows_set_linear.argtypes = [vp, C.POINTER(LinearSystem)]
    L.lig_rows_verify_set_linear.argtypes = [vp, C.POINTER(LinearSystem)]
    L.lig_shard_rows_set_linear.argtypes = [vp, C.POINTER(LinearSystem)]
    L.lig_shard_rows_linear_stats.argtypes = [vp, C.POINTER(u64), C.POINTER(u64)]
    L.lig_derived_shard_count.argtypes = [C.POINTER(LinearSystem), vp, u64, u32, vp, vp, u64, u32, u32, C.POINTER(DerivedShardInfo)]
    L.lig_shard_rows_set_derived.argtypes = [vp, C.POINTER(LinearSystem), vp, u64, C.POINTER(DerivedShardInfo)]
    L.lig_linear_shard_count.argtypes = [C.POINTER(LinearSystem), vp, u64, u32, u32, u32, C.POINTER(u64), C.POINTER(u64)]
    L.lig_linear_prepare.argtypes = [vp, C.POINTER(LinearSystem), vp, u64, C.POINTER(vp)]
    L.lig_linear_program_release.argtypes = [vp]
    L.lig_linear_program_release.restype = None
    L.lig_linear_program_bytes.argtypes = [vp, C.POINTER(u64), C.POINTER(u64)]
    L.lig_rows_attach_linear.argtypes = [vp, vp]
    L.lig_rows_verify_attach_linear.argtypes = [vp, vp]
    L.lig_rows_set_linear_values.argtypes = [vp, vp, u64]
    L.lig_rows_verify_set_linear_values.argtypes = [vp, vp, u64]
    L.lig_linear_program_form.argtypes = [vp, vp, vp, vp, u64, vp, vp]
    L.lig_rows_diagnose.argtypes = [vp, C.POINTER(LinearSystem), vp, u64, vp, u64, C.POINTER(DiagInfo)]
    L.lig_shard_rows_diagnose.argtypes = [vp, C.POINTER(LinearSystem), vp, u64, vp, u64, C.POINTER(DiagInfo)]
    L.lig_rows_diagnose_attached.argtypes = [vp, vp, u64, vp, u64, C.POINTER(DiagInfo)]
    L.lig_shard_rows_set_linear_values.argtypes = [vp, vp, u64]
    L.lig_shard_rows_diagnose_attached.argtypes = [vp, vp, u64, vp, u64, C.POINTER(DiagInfo)]
    L.lig_rows_explain.argtypes = [vp, C.POINTER(LinearSystem), vp, u64, vp, vp, u64, C.POINTER(ExplainInfo)]
    L.lig_rows_explain_attached.argtypes = [vp, vp, u64, vp, vp, u64, C.POINTER(ExplainInfo)]
    L.lig_rows_read_slots.argtypes = [vp, vp, u64, vp]
    L.lig_rows_explain_slots.argtypes = [vp, C.POINTER(LinearSystem), vp, u64, vp, vp, u64, C.POINTER(SlotInfo)]
    L.lig_rows_explain_slots_attached.argtypes = [vp, vp, u64, vp, vp, u64, C.POINTER(SlotInfo)]
    L.lig_rows_untouched_slots.argtypes = [vp, C.POINTER(LinearSystem), C.c_int, vp, u64, C.POINTER(UntouchedInfo)]
    L.lig_rows_untouched_slots_attached.argtypes = [vp, C.c_int, vp, u64, C.POINTER(UntouchedInfo)]
    L.lig_shard_rows_explain.argtypes = [vp, C.POINTER(LinearSystem), vp, u64, vp, vp, u64, C.POINTER(ExplainInfo)]
    L.lig_shard_rows_read_slots.argtypes = [vp, vp, u64, vp]
    L.lig_shard_rows_explain_attached.argtypes = [vp, vp, u64, vp, vp, u64, C.POINTER(ExplainInfo)]
    L.lig_shard_rows_explain_slots.argtypes = [vp, C.POINTER(LinearSystem), vp, u64, vp, vp, u64, C.POINTER(SlotInfo)]
    L.lig_shard_rows_explain_slots_attached.argtypes = [vp, vp, u64, vp, vp, u64, C.POINTER(SlotInfo)]
    L.lig_shard_rows_untouched_slots.argtypes = [vp, C.POINTER(LinearSystem), C.c_int, vp, u64, C.POINTER(UntouchedInfo)]
    L.lig_shard_rows_untouched_slots_attached.argtypes = [vp, C.c_int, vp, u64, C.POINTER(UntouchedInfo)]
    return L


class LigError(RuntimeError):
    pass


# ---- host-only transcript helpers (no GPU needed)
def public_arg_bytes(kind, text):
    """one JSON "args" entry ({"i64": ..} / {"str": ..} / {"hex": ..}) -> the bytes the reference hashes"""
    L = load_library()
    kind = {"i64": ARG_I64, "str": ARG_STR, "hex": ARG_HEX}.get(kind, kind)
    ln = C.c_size_t()
    txt = str(text).encode()
    L.lig_public_arg_bytes(kind, txt, None, 0, C.byref(ln))
    buf = (C.c_uint8 * max(1, ln.value))()
    if L.lig_public_arg_bytes(kind, txt, buf, ln.value, C.byref(ln)) != 0:
        raise LigError("malformed public argument %r" % (text,))
    return bytes(buf[:ln.value])


def instance_hash(args):
    L = load_library()
    args = [bytes(a) for a in args]
    blob = np.frombuffer(b"".join(args) or b"\0", dtype=np.uint8).copy()
    lens = np.array([len(a) for a in args] or [0], dtype=np.uint64)
    out = np.zeros(32, dtype=np.uint8)
    if L.lig_instance_hash(_hptr(blob), _hptr(lens), len(args), _hptr(out)) != 0:
        raise LigError("lig_instance_hash failed")
    return out.tobytes()


def rccl_available():
    """-> (ok, path of the librccl the library resolved or the reason it could not, ncclGetVersion code)"""
    L = load_library()
    buf, ver = C.create_string_buffer(512), C.c_int()
    rc = L.lig_rccl_available(buf, 512, C.byref(ver))
    return rc == 0, buf.value.decode(), ver.value


def device_pci_bus_id(device):
    """-> "0000:c1:00.0" of a HIP device ordinal (None if the runtime cannot say)"""
    L = load_library()
    buf = C.create_string_buffer(64)
    return buf.value.decode() if L.lig_device_pci_bus_id(device, buf, 64) == 0 else None


def device_peer_access(device, peer):
    L = load_library()
    can = C.c_int()
    return bool(can.value) if L.lig_device_peer_access(device, peer, C.byref(can)) == 0 else None


def shard_plan(job, l, world):
    """-> (rounds, boundaries): the block-cyclic deal of the job's rows over `world` ranks (host only)"""
    L = load_library()
    L.lig_shard_plan.argtypes = [C.POINTER(SynthJob), C.c_uint32, C.c_uint32, C.POINTER(C.c_uint64), C.c_void_p, C.c_size_t]
    rounds = C.c_uint64()
    cap = 1 << 16
    b = np.zeros(cap, dtype=np.uint64)
    if L.lig_shard_plan(C.byref(job), l, world, C.byref(rounds), _hptr(b), cap) != 0:
        raise LigError("lig_shard_plan failed")
    return int(rounds.value), [int(x) for x in b[:rounds.value * world + 1]]


def pack_rows(rows, widths, l):
    """rows (R, k, 8) uint32 + per-row width (1 / 2 / 4 / 8 / 32 / ELEM_BIT / ELEM_PRODUCT) -> the packed byte array of the narrow
    row format (lig_rows_job.elem_bytes): a narrow row contributes its l data slots as little-endian integers of that width
    (ELEM_BIT: bit i % 8 of byte i / 8, LSB first), zero-padded to a multiple of 4 bytes; a row of width 0 / 32 all of its k
    slots; an ELEM_PRODUCT row (a derived QZ row: rows[r] is not looked at) nothing"""
    parts = []
    for r, w in enumerate(widths):
        w = int(w)
        if w == ELEM_PRODUCT:
            continue
        if w in (0, 32):
            parts.append(np.ascontiguousarray(rows[r], dtype=np.uint32).tobytes())
            continue
        if w == ELEM_BIT:
            assert not rows[r, :l, 1:].any() and not (rows[r, :l, 0] > 1).any(), "row %d is not a bit row" % r
            b = np.packbits(rows[r, :l, 0].astype(np.uint8), bitorder="little").tobytes()
        elif w in (1, 2):
            assert not rows[r, :l, 1:].any() and not (rows[r, :l, 0] >> (8 * w)).any(), "row %d does not fit %d-byte elements" % (r, w)
            b = rows[r, :l, 0].astype("<u%d" % w).tobytes()
        elif w in (4, 8):
            assert not rows[r, :l, w // 4:].any(), "row %d does not fit %d-byte elements" % (r, w)
            b = np.ascontiguousarray(rows[r, :l, :w // 4], dtype=np.uint32).tobytes()
        else:
            raise ValueError("row %d: no such width %d" % (r, w))
        parts.append(b + bytes(-len(b) % 4))
    return np.frombuffer(b"".join(parts), dtype=np.uint8).copy()


def narrowest_widths(rows, kinds, l, derive_products=False):
    """-> uint8 widths for pack_rows / elem_bytes: the smallest width each LINEAR / QX / QY / QZ row of rows (R, k, 8) fits into
    (ELEM_BIT if every data slot is 0 or 1, else 1, 2, 4, 8 bytes, else 32); every other row kind is 32.
    derive_products: every QZ row is ELEM_PRODUCT instead (not shipped; the row must then be flagged ROW_DRAW_PAD)"""
    rows = np.asarray(rows)
    kinds = np.asarray(kinds, dtype=np.uint8) & 0x7F
    out = np.full(len(kinds), 32, dtype=np.uint8)
    for r in range(len(kinds)):
        if kinds[r] > 3:
            continue
        if derive_products and kinds[r] == 3:
            out[r] = ELEM_PRODUCT
            continue
        d = rows[r, :l]
        if d[:, 2:].any():
            continue
        hi = int(d[:, 1].max()) if l else 0
        lo = int(d[:, 0].max()) if l else 0
        if hi:
            out[r] = 8
        elif lo <= 1:
            out[r] = ELEM_BIT
        elif lo <= 0xFF:
            out[r] = 1
        elif lo <= 0xFFFF:
            out[r] = 2
        else:
            out[r] = 4
    return out


def narrow_row_bytes(w, l, k):
    """packed bytes of one row of width w without records: 0 / 32 all k slots; ELEM_BIT, 1, 2, 4, 8 the l data slots rounded up to a
    multiple of 4; ELEM_PRODUCT nothing"""
    w = int(w)
    if w in (0, 32):
        return 32 * k
    if w == ELEM_PRODUCT:
        return 0
    if w == ELEM_BIT:
        return (l + 31) // 32 * 4
    if w in (1, 2, 4, 8):
        return (l * w + 3) // 4 * 4
    raise ValueError("no such width %d" % w)


_MIXED_BASES = ((ELEM_BIT, 1), (1, 8), (2, 16), (4, 32), (8, 64))       # base width, bits a slot may have to fit it


def _slot_bits(d):
    """(l, 8) uint32 -> the bit length of every slot"""
    d = np.asarray(d, dtype=np.uint32)
    top = np.zeros(len(d), dtype=np.int64)
    for j in range(8):                           # the highest non-zero limb decides
        nz = d[:, j] != 0
        top[nz] = 32 * j + np.floor(np.log2(d[nz, j].astype(np.float64))).astype(np.int64) + 1
    return top


def mixed_widths(rows, kinds, l, derive_products=False):
    """-> (widths, wide_per_row) for pack_rows_mixed / elem_bytes + wide_per_row: every LINEAR / QX / QY / QZ row of rows (R, k, 8) as
    the cheapest MIXED row -- a base width b of ELEM_BIT, 1, 2, 4, 8 costs narrow_row_bytes(b) + 36 bytes per data slot that does
    not fit b; on a tie the narrower base -- or at full width (32) where that is not more bytes than the cheapest mixed form; every
    other row kind is 32 with no records.  derive_products: every QZ row is ELEM_PRODUCT instead, as narrowest_widths does"""
    rows = np.asarray(rows)
    kinds = np.asarray(kinds, dtype=np.uint8) & 0x7F
    k = rows.shape[1] if len(kinds) else 0
    widths = np.full(len(kinds), 32, dtype=np.uint8)
    wide = np.zeros(len(kinds), dtype=np.uint32)
    for r in range(len(kinds)):
        if kinds[r] > 3:
            continue
        if derive_products and kinds[r] == 3:
            widths[r] = ELEM_PRODUCT
            continue
        bits = _slot_bits(rows[r, :l])
        best = None
        for b, fit in _MIXED_BASES:
            c = int((bits > fit).sum())
            cost = narrow_row_bytes(b, l, k) + WIDE_RECORD_BYTES * c
            if best is None or cost < best[0]:
                best = (cost, b, c)
        if 32 * k <= best[0]:
            continue
        widths[r], wide[r] = best[1], best[2]
    return widths, wide


def pack_rows_mixed(rows, widths, wide_per_row, l):
    """pack_rows for MIXED rows (lig_rows_job.wide_per_row): row r with wide_per_row[r] = c > 0 is its narrow row of width widths[r] with
    0 in the slots that do not fit, followed by c records -- uint32 column, 8 uint32 limbs -- of exactly those slots, ascending; the
    row must have exactly c such data slots.  With all counts 0 this is pack_rows"""
    rows = np.asarray(rows)
    parts = []
    for r, w in enumerate(widths):
        w, c = int(w), int(wide_per_row[r])
        if not c:
            parts.append(pack_rows(rows[r:r + 1], [w], l).tobytes())
            continue
        fit = dict(_MIXED_BASES).get(w)
        if fit is None:
            raise ValueError("row %d: records on a row of width %d" % (r, w))
        cols = np.nonzero(_slot_bits(rows[r, :l]) > fit)[0]
        if len(cols) != c:
            raise ValueError("row %d: %d slots do not fit its width, wide_per_row says %d" % (r, len(cols), c))
        base = np.array(rows[r:r + 1], dtype=np.uint32)
        base[0, cols] = 0
        rec = np.zeros((c, 9), dtype=np.uint32)
        rec[:, 0] = cols
        rec[:, 1:] = rows[r, cols]
        parts.append(pack_rows(base, [w], l).tobytes() + rec.tobytes())
    return np.frombuffer(b"".join(parts), dtype=np.uint8).copy()


def shard_rows_plan(kinds, world):
    """-> (rounds, boundaries): the block-cyclic deal of a rows job's committed rows over `world` ranks (host only):
    global chunk g = rows [b[g], b[g+1]) belongs to rank g mod world"""
    L = load_library()
    kinds = np.ascontiguousarray(kinds, dtype=np.uint8)
    rounds = C.c_uint64()
    cap = 1 << 16
    b = np.zeros(cap, dtype=np.uint64)
    if L.lig_shard_rows_plan(_hptr(kinds) if len(kinds) else None, len(kinds), world, C.byref(rounds), _hptr(b), cap) != 0:
        raise LigError("lig_shard_rows_plan failed")
    return int(rounds.value), [int(x) for x in b[:rounds.value * world + 1]]


def local_rows_of(boundaries, rank, world):
    """global row indices of `rank`'s chunks, in commit order"""
    out = []
    for g in range(rank, len(boundaries) - 1, world):
        out.extend(range(boundaries[g], boundaries[g + 1]))
    return out


def sample_columns(seed, n, t=192):
    L = load_library()
    s = np.frombuffer(bytes(seed), dtype=np.uint8).copy()
    out = np.zeros(min(t, n), dtype=np.uint32)
    if L.lig_sample_columns(_hptr(s), n, t, _hptr(out)) != 0:
        raise LigError("lig_sample_columns failed")
    return out


def _hptr(a):
    return a.ctypes.data_as(C.c_void_p) if a is not None else None


class Context:
    """owns a lig_ctx; device buffers are plain integer device pointers"""

    def __init__(self, l, k, n, device=0):
        self.L = load_library()
        self.l, self.k, self.n = l, k, n
        h = C.c_void_p()
        rc = self.L.lig_ctx_create(C.byref(h), device, l, k, n)
        self.h = h
        if rc != 0:
            msg = self.L.lig_last_error(h).decode() if h else "invalid arguments"
            if h:
                self.L.lig_ctx_destroy(h)
            self.h = None
            raise LigError("lig_ctx_create failed (%d): %s" % (rc, msg))
        self._bufs = []

    def close(self):
        if getattr(self, "h", None):
            for p in self._bufs:
                self.L.lig_free(self.h, p)
            self._bufs = []
            self.L.lig_ctx_destroy(self.h)
            self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def check(self, rc):
        if rc != 0:
            raise LigError("lig call failed (%d): %s" % (rc, self.L.lig_last_error(self.h).decode()))

    # ---- buffers
    def malloc(self, nbytes):
        p = C.c_void_p()
        self.check(self.L.lig_malloc(self.h, nbytes, C.byref(p)))
        self._bufs.append(p)
        return p

    def free(self, p):
        self._bufs = [q for q in self._bufs if q.value != p.value]
        self.check(self.L.lig_free(self.h, p))

    def upload(self, arr):
        arr = np.ascontiguousarray(arr)
        p = self.malloc(arr.nbytes)
        self.check(self.L.lig_write(self.h, p, _hptr(arr), arr.nbytes))
        return p

    def write(self, p, arr, offset=0):
        arr = np.ascontiguousarray(arr)
        self.check(self.L.lig_write(self.h, C.c_void_p(p.value + offset), _hptr(arr), arr.nbytes))

    def download(self, p, shape, dtype=np.uint32, offset=0):
        out = np.zeros(shape, dtype=dtype)
        self.check(self.L.lig_read(self.h, _hptr(out), C.c_void_p(p.value + offset), out.nbytes))
        return out

    def sync(self):
        self.check(self.L.lig_sync(self.h))

    # ---- ops (thin)
    def encode(self, p): self.check(self.L.lig_encode(self.h, p))
    def encode_2k(self, p): self.check(self.L.lig_encode_2k(self.h, p))
    def decode(self, p): self.check(self.L.lig_decode(self.h, p))
    def ntt(self, p, which, inverse): self.check(self.L.lig_ntt(self.h, p, which, int(inverse)))
    def encode_rows(self, msgs, cws, rows): self.check(self.L.lig_encode_rows(self.h, msgs, cws, rows))

    def eltwise(self, op, x, y, out, count, scalar=None, bit=0):
        sc = None
        if scalar is not None:
            sc = np.frombuffer(int(scalar).to_bytes(32, "little"), dtype=np.uint8).copy()
        self.check(self.L.lig_eltwise(self.h, OPS[op] if isinstance(op, str) else op, x, y, out, count, _hptr(sc), bit))

    def powmod(self, base, exp_p, coeff_p, out_p, count, add=False):
        b = np.frombuffer(int(base).to_bytes(32, "little"), dtype=np.uint8).copy()
        self.check(self.L.lig_powmod(self.h, _hptr(b), exp_p, coeff_p, out_p, count, int(add)))

    def sha_state(self, n_inst):
        p = self.malloc(self.L.lig_sha_state_bytes(n_inst))
        self.check(self.L.lig_sha_init(self.h, p, n_inst))
        return p

    def sha_update_rows(self, st, cws, rows): self.check(self.L.lig_sha_update_rows(self.h, st, cws, rows))
    def sha_final(self, st, digests): self.check(self.L.lig_sha_final(self.h, st, digests))

    def merkle_build(self, leaves, n_leaves):
        nodes = self.malloc(32 * self.L.lig_merkle_nodes(n_leaves))
        self.check(self.L.lig_merkle_build(self.h, leaves, n_leaves, nodes))
        return nodes

    def sample_init(self, idx):
        idx = np.ascontiguousarray(idx, dtype=np.uint32)
        self.check(self.L.lig_sample_init(self.h, _hptr(idx), len(idx)))

    def gather_rows(self, cws, rows, out): self.check(self.L.lig_gather_rows(self.h, cws, rows, out))

    def rlc_rows(self, U, Rn, rows, rc, code, lin, triples=None, rq=None, quad=None):
        def sc(vals):
            return np.frombuffer(b"".join(int(v).to_bytes(32, "little") for v in vals), dtype=np.uint8).copy()
        rcb = sc(rc) if rc is not None else None
        nt = 0 if triples is None else len(triples)
        tri = np.ascontiguousarray(np.array(triples, dtype=np.uint32).reshape(-1)) if nt else None
        rqb = sc(rq) if nt else None
        self.check(self.L.lig_rlc_rows(self.h, U, Rn, rows, _hptr(rcb), code, lin, _hptr(tri), _hptr(rqb), nt, quad))

    # ---- batched prover over a synthetic trace
    @staticmethod
    def make_job(n_linear, n_quad=0, synth_seed=1, generated_at=0, encoding_seed=None, public_args=None):
        import hashlib
        job = SynthJob()
        job.set_public_args(public_args)
        job.n_linear, job.n_quad, job.generated_at = n_linear, n_quad, generated_at
        es = bytes(range(32)) if encoding_seed is None else bytes(encoding_seed)
        wk = hashlib.sha256(b"lig-synth" + int(synth_seed).to_bytes(8, "little")).digest()
        for i in range(32):
            job.encoding_seed[i] = es[i]
            job.witness_key[i] = wk[i]
            job.program_hash[i] = 0
        job.version = b"1.5.0"
        return job

    # ---- RCCL communicator of the sharded prover (csrc/comm_rccl.hip)
    def rccl_unique_id(self):
        out = np.zeros(128, dtype=np.uint8)
        self.check(self.L.lig_rccl_unique_id(_hptr(out)))
        return out.tobytes()

    def rccl_comm(self, unique_id, rank, world):
        comm = Comm()
        uid = np.frombuffer(bytes(unique_id), dtype=np.uint8).copy()
        self.check(self.L.lig_rccl_comm_create(self.h, _hptr(uid), rank, world, C.byref(comm)))
        return comm

    def rccl_comm_destroy(self, comm):
        self.L.lig_rccl_comm_destroy(C.byref(comm))

    def ipc_comm(self, shm_name, rank, world):
        """the process-to-process communicator (csrc/comm_ipc.hip): same fresh "/name" on every rank"""
        comm = Comm()
        self.check(self.L.lig_ipc_comm_create(self.h, shm_name.encode(), rank, world, C.byref(comm)))
        return comm

    def ipc_comm_destroy(self, comm):
        self.L.lig_ipc_comm_destroy(C.byref(comm))

    def rccl_comm_count(self, comm):
        n = C.c_uint32()
        self.check(self.L.lig_rccl_comm_count(C.byref(comm), C.byref(n)))
        return n.value

    # ---- one trace sharded over ranks (comm: a Comm built by dist.Group.make_comm)
    def shard_prepare(self, job, rank, world, comm):
        t = C.c_void_p()
        self.check(self.L.lig_shard_prepare(self.h, C.byref(job), rank, world, C.byref(comm), C.byref(t)))
        return t

    def shard_prove(self, shard, copy=True):
        proof, ln, info = C.POINTER(C.c_uint8)(), C.c_size_t(), ProofInfo()
        self.check(self.L.lig_shard_prove(shard, C.byref(proof), C.byref(ln), C.byref(info)))
        if not copy:
            return (C.addressof(proof.contents), ln.value), info
        return C.string_at(proof, ln.value), info

    def shard_destroy(self, shard):
        self.L.lig_shard_destroy(shard)
        getattr(self, "_shard_keep", {}).pop(shard.value, None)

    # ---- one trace sharded over ranks, rows supplied by the caller (lig_shard_rows_*)
    def shard_rows_begin(self, kinds_all, local_msgs, rank, world, comm, on_device=False, encoding_seed=None, generated_at=0,
                         public_args=None, dense_rands_per_row=None, elem_bytes=None, wide_per_row=None):
        """kinds_all: the kinds of ALL committed rows; local_msgs: this rank's rows (lig_shard_rows_plan), (rows_local, k, 8) uint32;
        with elem_bytes (one width per row of the WHOLE trace): this rank's rows packed back to back (pack_rows of the local rows)"""
        kinds = np.ascontiguousarray(kinds_all, dtype=np.uint8)
        job = RowsJob()
        job.rows = len(kinds)
        job.kinds = kinds.ctypes.data if len(kinds) else None
        keep = (kinds,)
        if elem_bytes is not None:
            eb = np.ascontiguousarray(elem_bytes, dtype=np.uint8)
            job.elem_bytes = eb.ctypes.data if len(eb) else None
            keep += (eb,)
        if wide_per_row is not None:              # mixed rows: one record count per row of the WHOLE trace
            wp = np.ascontiguousarray(wide_per_row, dtype=np.uint32)
            job.wide_per_row = wp.ctypes.data if len(wp) else None
            job.reserved = ROWS_JOB_WIDE                 # this struct has the member
            keep += (wp,)
        if on_device:
            job.msgs = local_msgs.value if hasattr(local_msgs, "value") else int(local_msgs)
        elif elem_bytes is not None:              # narrow format: the packed byte string
            local_msgs = np.frombuffer(bytes(local_msgs), dtype=np.uint8).copy() if not isinstance(local_msgs, np.ndarray) else np.ascontiguousarray(local_msgs, dtype=np.uint8)
            job.msgs = local_msgs.ctypes.data if local_msgs.size else None
            keep += (local_msgs,)
        else:
            local_msgs = np.ascontiguousarray(local_msgs, dtype=np.uint32)
            job.msgs = local_msgs.ctypes.data if local_msgs.size else None
            keep += (local_msgs,)
        job.msgs_on_device = int(bool(on_device))
        es = bytes(range(32)) if encoding_seed is None else bytes(encoding_seed)
        for i in range(32):
            job.encoding_seed[i] = es[i]
            job.program_hash[i] = 0
        job.generated_at = generated_at
        job.version = b"1.5.0"
        job.set_public_args(public_args)
        if dense_rands_per_row is not None:
            dr = np.ascontiguousarray(dense_rands_per_row, dtype=np.uint32)
            job.dense_rands_per_row = dr.ctypes.data if len(dr) else None
            keep += (dr,)
        t = C.c_void_p()
        self.check(self.L.lig_shard_rows_begin(self.h, C.byref(job), rank, world, C.byref(comm), C.byref(t)))
        # host rows are read asynchronously (uploader thread) until lig_shard_rows_commit returns: the arrays live as long as the shard
        if not hasattr(self, "_shard_keep"):
            self._shard_keep = {}
        self._shard_keep[t.value] = keep
        return t

    def shard_rows_restart(self, shard, local_msgs, on_device=False):
        """the next trace of the same shape (after shard_rows_prove of the previous one); a narrow shard takes the packed bytes"""
        if on_device:
            ptr, keep = (local_msgs if hasattr(local_msgs, "value") else C.c_void_p(int(local_msgs))), ()
        else:
            local_msgs = np.ascontiguousarray(local_msgs, dtype=local_msgs.dtype if isinstance(local_msgs, np.ndarray) and local_msgs.dtype == np.uint8 else np.uint32)
            ptr, keep = C.c_void_p(local_msgs.ctypes.data if local_msgs.size else None), (local_msgs,)
        if hasattr(self, "_shard_keep"):
            self._shard_keep[shard.value] = keep
        self.check(self.L.lig_shard_rows_restart(shard, ptr, int(bool(on_device))))

    def shard_rows_commit(self, shard):
        root, seed = np.zeros(32, dtype=np.uint8), np.zeros(32, dtype=np.uint8)
        self.check(self.L.lig_shard_rows_commit(shard, _hptr(root), _hptr(seed)))
        return root.tobytes(), seed.tobytes()

    def shard_rows_set_linear(self, shard, system):
        """lig_shard_rows_set_linear: `system` describes the WHOLE trace and is the same on every rank; shard_rows_prove(shard, None, None)
        then forms this rank's randomness rows and the constant itself; None removes it"""
        self.check(self.L.lig_shard_rows_set_linear(shard, C.byref(system) if system is not None else None))

    def shard_rows_set_derived(self, shard, system, pairs):
        """lig_shard_rows_set_derived: pairs = (global slot, defining constraint of `system`) of the slots of the WHOLE trace the ranks form
        themselves from the next shard_rows_commit on, product entries (slot, DERIVED_PRODUCT) included; the same on every rank; None or an
        empty list removes the list -> DerivedShardInfo"""
        info = DerivedShardInfo()
        info.struct_bytes = C.sizeof(DerivedShardInfo)
        d = _derived_pairs(pairs) if pairs is not None else np.zeros((0, 2), dtype=np.uint32)
        self.check(self.L.lig_shard_rows_set_derived(shard, C.byref(system) if system is not None else None, d.ctypes.data if len(d) else None, len(d),
                                                     C.byref(info)))
        return info

    def shard_rows_linear_stats(self, shard):
        """-> (local_terms, sampled_constraints) of the system set last on this rank"""
        lt, sc = C.c_uint64(), C.c_uint64()
        self.check(self.L.lig_shard_rows_linear_stats(shard, C.byref(lt), C.byref(sc)))
        return int(lt.value), int(sc.value)

    def shard_rows_prove(self, shard, local_rands=None, const_sum=None, on_device=False):
        """local_rands = None: the rows come from dense_rands_per_row or from the system of shard_rows_set_linear"""
        proof, ln, info = C.POINTER(C.c_uint8)(), C.c_size_t(), ProofInfo()
        cs = np.frombuffer(bytes(const_sum), dtype=np.uint8).copy() if const_sum is not None else None
        if local_rands is None:
            rp = None
        elif on_device:
            rp = local_rands
        else:
            local_rands = np.ascontiguousarray(local_rands, dtype=np.uint32)
            rp = C.c_void_p(local_rands.ctypes.data if local_rands.size else None)
        self.check(self.L.lig_shard_rows_prove(shard, rp, int(bool(on_device)), _hptr(cs), C.byref(proof), C.byref(ln), C.byref(info)))
        return C.string_at(proof, ln.value), info

    def synth_prepare(self, n_linear, n_quad=0, synth_seed=1, generated_at=0, encoding_seed=None):
        import hashlib
        job = SynthJob()
        job.n_linear, job.n_quad, job.generated_at = n_linear, n_quad, generated_at
        es = bytes(range(32)) if encoding_seed is None else bytes(encoding_seed)
        wk = hashlib.sha256(b"lig-synth" + int(synth_seed).to_bytes(8, "little")).digest()
        for i in range(32):
            job.encoding_seed[i] = es[i]
            job.witness_key[i] = wk[i]
            job.program_hash[i] = 0
        job.version = b"1.5.0"
        return self.synth_prepare_job(job)

    def synth_prepare_job(self, job):
        """prepare from a SynthJob built by make_job (e.g. with a batch program attached, tests/batch_prog.py)"""
        t = C.c_void_p()
        self.check(self.L.lig_synth_prepare(self.h, C.byref(job), C.byref(t)))
        return t

    def synth_prove(self, trace, copy=True):
        """-> (proof bytes, ProofInfo); copy=False returns (address, length) of the trace-owned pinned buffer"""
        proof, ln, info = C.POINTER(C.c_uint8)(), C.c_size_t(), ProofInfo()
        self.check(self.L.lig_synth_prove(trace, C.byref(proof), C.byref(ln), C.byref(info)))
        if not copy:
            return (C.addressof(proof.contents), ln.value), info
        return C.string_at(proof, ln.value), info

    def synth_verify(self, job, const_sum, proof):
        """-> VerifyInfo (accept = 1 iff the reference's seven verifier predicates hold).  const_sum=None: the verifier
        derives the constant of the linear test from the public statement (the sound mode)"""
        info = VerifyInfo()
        cs = np.frombuffer(bytes(const_sum), dtype=np.uint8).copy() if const_sum is not None else None
        pb = np.frombuffer(bytes(proof), dtype=np.uint8).copy()
        self.check(self.L.lig_synth_verify(self.h, C.byref(job), _hptr(cs), _hptr(pb), len(pb), C.byref(info)))
        return info

    def verify_release(self):
        self.check(self.L.lig_verify_release(self.h))

    # ---- the same prover over rows supplied by the caller (lig_rows_*)
    def rows_begin(self, kinds, msgs, on_device=False, encoding_seed=None, generated_at=0, public_args=None, program_hash=None,
                   dense_rands_per_row=None, elem_bytes=None, wide_per_row=None):
        """kinds: uint8 array (ROW_KINDS | ROW_DRAW_PAD); msgs: device pointer (on_device) or a (rows, k, 8) uint32 host array.
        -> (trace, keepalive); keep `keepalive` referenced until rows_commit has returned"""
        kinds = np.ascontiguousarray(kinds, dtype=np.uint8)
        job = RowsJob()
        job.rows = len(kinds)
        job.kinds = kinds.ctypes.data if len(kinds) else None
        if on_device:
            job.msgs, keep = (msgs.value if hasattr(msgs, "value") else int(msgs)), (kinds,)
        elif elem_bytes is not None:              # narrow format: msgs is the packed byte string (pack_rows)
            msgs = np.frombuffer(bytes(msgs), dtype=np.uint8).copy() if not isinstance(msgs, np.ndarray) else np.ascontiguousarray(msgs, dtype=np.uint8)
            job.msgs, keep = (msgs.ctypes.data if msgs.size else None), (kinds, msgs)
        else:
            msgs = np.ascontiguousarray(msgs, dtype=np.uint32)
            job.msgs, keep = (msgs.ctypes.data if msgs.size else None), (kinds, msgs)
        if elem_bytes is not None:
            eb = np.ascontiguousarray(elem_bytes, dtype=np.uint8)
            job.elem_bytes = eb.ctypes.data if len(eb) else None
            keep = keep + (eb,)
        if wide_per_row is not None:              # mixed rows (pack_rows_mixed): one record count per row
            wp = np.ascontiguousarray(wide_per_row, dtype=np.uint32)
            job.wide_per_row = wp.ctypes.data if len(wp) else None
            job.reserved = ROWS_JOB_WIDE                 # this struct has the member
            keep = keep + (wp,)
        job.msgs_on_device = int(bool(on_device))
        es = bytes(range(32)) if encoding_seed is None else bytes(encoding_seed)
        ph = bytes(32) if program_hash is None else bytes(program_hash)
        for i in range(32):
            job.encoding_seed[i] = es[i]
            job.program_hash[i] = ph[i]
        job.generated_at = generated_at
        job.version = b"1.5.0"
        job.set_public_args(public_args)
        if dense_rands_per_row is not None:
            dr = np.ascontiguousarray(dense_rands_per_row, dtype=np.uint32)
            job.dense_rands_per_row = dr.ctypes.data if len(dr) else None
            keep = keep + (dr,)
        t = C.c_void_p()
        self.check(self.L.lig_rows_begin(self.h, C.byref(job), C.byref(t)))
        return t, keep + (job,)

    def rows_restart(self, trace, msgs, on_device=False):
        p = msgs if on_device else C.c_void_p(msgs if isinstance(msgs, int) else msgs.ctypes.data)
        self.check(self.L.lig_rows_restart(trace, p, int(bool(on_device))))

    def rows_commit(self, trace):
        root, seed = np.zeros(32, dtype=np.uint8), np.zeros(32, dtype=np.uint8)
        self.check(self.L.lig_rows_commit(trace, _hptr(root), _hptr(seed)))
        return root.tobytes(), seed.tobytes()

    def rows_prove(self, trace, rands, const_sum, on_device=False, copy=True):
        proof, ln, info = C.POINTER(C.c_uint8)(), C.c_size_t(), ProofInfo()
        cs = np.frombuffer(bytes(const_sum), dtype=np.uint8).copy() if const_sum is not None else None
        if rands is None:
            rp = None
        elif on_device:
            rp = rands
        elif isinstance(rands, int):              # a raw host address (e.g. a pinned torch tensor's data_ptr()): no copy, no conversion
            rp = C.c_void_p(rands)
        else:
            rands = np.ascontiguousarray(rands, dtype=np.uint32)
            rp = C.c_void_p(rands.ctypes.data if rands.size else None)
        self.check(self.L.lig_rows_prove(trace, rp, int(bool(on_device)), _hptr(cs), C.byref(proof), C.byref(ln), C.byref(info)))
        if not copy:
            return (C.addressof(proof.contents), ln.value), info
        return C.string_at(proof, ln.value), info

    def host_alloc(self, nbytes):
        """page-locked host memory (lig_host_alloc) as a uint8 numpy view; keep the returned (array, ptr) until host_free(ptr)"""
        p = C.c_void_p()
        self.check(self.L.lig_host_alloc(self.h, nbytes, C.byref(p)))
        arr = np.ctypeslib.as_array(C.cast(p, C.POINTER(C.c_uint8)), shape=(max(1, nbytes),))[:nbytes]
        return arr, p

    def host_free(self, p):
        self.check(self.L.lig_host_free(self.h, p))

    def upload_health(self):
        """lig_upload_health -> (retries, unsettled): calls that re-made a timed-out upload / abandoned transfers still pending"""
        r, u = C.c_uint32(0), C.c_uint32(0)
        self.check(self.L.lig_upload_health(self.h, C.byref(r), C.byref(u)))
        return r.value, u.value

    def rows_push_rands(self, trace, first_row, n_rows, host_ptr):
        """lig_rows_push_rands: randomness rows [first_row, first_row + n_rows), host memory valid until rows_prove returns"""
        self.check(self.L.lig_rows_push_rands(trace, first_row, n_rows, C.c_void_p(host_ptr)))

    def rows_push_rands_sparse(self, trace, first_row, present, host_ptr):
        """lig_rows_push_rands_sparse: `present` (uint8 per row) says which of the rows have a randomness row at host_ptr (packed)"""
        present = np.ascontiguousarray(present, dtype=np.uint8)
        self.check(self.L.lig_rows_push_rands_sparse(trace, first_row, len(present), _hptr(present), C.c_void_p(host_ptr)))

    def rows_verify_begin(self, kinds, proof, public_args=None):
        """-> (vtrace or None, stage1_seed bytes, VerifyInfo): the verifier's first half for a rows job (kinds + public data)"""
        kinds = np.ascontiguousarray(kinds, dtype=np.uint8)
        job = RowsJob()
        job.rows = len(kinds)
        job.kinds = kinds.ctypes.data if len(kinds) else None
        job.set_public_args(public_args)
        pb = np.frombuffer(bytes(proof), dtype=np.uint8).copy()
        vt, seed, info = C.c_void_p(), np.zeros(32, dtype=np.uint8), VerifyInfo()
        self.check(self.L.lig_rows_verify_begin(self.h, C.byref(job), _hptr(pb), len(pb), C.byref(vt), _hptr(seed), C.byref(info)))
        return (vt if vt.value else None), seed.tobytes(), info

    def rows_verify_finish(self, vtrace, rands, const_sum, on_device=False):
        """rands=None / const_sum=None: formed from the linear system set with rows_verify_set_linear"""
        info = VerifyInfo()
        cs = np.frombuffer(bytes(const_sum), dtype=np.uint8).copy() if const_sum is not None else None
        if rands is None:
            rp = None
        elif on_device:
            rp = rands
        else:
            rands = np.ascontiguousarray(rands, dtype=np.uint32)
            rp = C.c_void_p(rands.ctypes.data if rands.size else None)
        self.check(self.L.lig_rows_verify_finish(vtrace, rp, int(bool(on_device)), _hptr(cs), C.byref(info)))
        return info

    # ---- sparse linear constraints: the linear-test randomness formed on the GPU (LinearSystem)
    def linear_check(self, system, kinds):
        return linear_check(system, kinds, self.l)

    def rows_set_linear(self, trace, system):
        """lig_rows_set_linear: rows_prove(trace, None, None) then forms randomness matrix and constant itself; None removes it"""
        self.check(self.L.lig_rows_set_linear(trace, C.byref(system) if system is not None else None))

    def rows_set_derived(self, trace, system, pairs):
        """lig_rows_set_derived: pairs = (slot, defining constraint of `system`) of the slots the library forms itself from the next
        rows_commit on (whatever the rows carry there is ignored), and (slot, DERIVED_PRODUCT) of the columns of ELEM_PRODUCT rows to re-form
        from the committed operands in wave order; None or an empty list removes the list -> DerivedInfo"""
        info = DerivedInfo()
        info.struct_bytes = C.sizeof(DerivedInfo)
        d = _derived_pairs(pairs) if pairs is not None else np.zeros((0, 2), dtype=np.uint32)
        self.check(self.L.lig_rows_set_derived(trace, C.byref(system) if system is not None else None, d.ctypes.data if len(d) else None, len(d),
                                               C.byref(info)))
        return info

    def rows_verify_set_linear(self, vtrace, system):
        self.check(self.L.lig_rows_verify_set_linear(vtrace, C.byref(system) if system is not None else None))

    def linear_form(self, system, kinds, key, out):
        """lig_linear_form: out (device, len(kinds) x k x 32 bytes) <- the randomness matrix for the stream keyed by `key`;
        -> the constant (32 bytes)"""
        kinds = np.ascontiguousarray(kinds, dtype=np.uint8)
        kb = np.frombuffer(bytes(key), dtype=np.uint8).copy()
        cs = np.zeros(32, dtype=np.uint8)
        self.check(self.L.lig_linear_form(self.h, C.byref(system), kinds.ctypes.data if len(kinds) else None, len(kinds), _hptr(kb), out, _hptr(cs)))
        return cs.tobytes()

    # ---- prepared linear systems: one LinearProgram for many proofs, verifications and contexts
    def linear_prepare(self, system, kinds, rows=None):
        """lig_linear_prepare -> LinearProgram (the caller's reference: release() it, or use it in a `with` block)"""
        kinds = np.ascontiguousarray(kinds, dtype=np.uint8)
        rows = len(kinds) if rows is None else int(rows)
        if rows > len(kinds):
            raise ValueError("linear_prepare: %d rows but %d kinds" % (rows, len(kinds)))
        h = C.c_void_p()
        self.check(self.L.lig_linear_prepare(self.h, C.byref(system), kinds.ctypes.data if len(kinds) else None, rows, C.byref(h)))
        return LinearProgram(self.L, h)

    def rows_attach_linear(self, trace, program):
        """lig_rows_attach_linear: rows_set_linear with a prepared LinearProgram; None detaches"""
        self.check(self.L.lig_rows_attach_linear(trace, program._handle() if program is not None else None))

    def rows_verify_attach_linear(self, vtrace, program):
        self.check(self.L.lig_rows_verify_attach_linear(vtrace, program._handle() if program is not None else None))

    def rows_set_linear_values(self, trace, coefs):
        """lig_rows_set_linear_values: this trace's values of the coefficient table (integers or (n, 8) uint32); None: the program's own"""
        tab = coef_table(coefs) if coefs is not None else None
        self.check(self.L.lig_rows_set_linear_values(trace, _hptr(tab) if tab is not None and len(tab) else None, len(tab) if tab is not None else 0))

    def rows_verify_set_linear_values(self, vtrace, coefs):
        tab = coef_table(coefs) if coefs is not None else None
        self.check(self.L.lig_rows_verify_set_linear_values(vtrace, _hptr(tab) if tab is not None and len(tab) else None, len(tab) if tab is not None else 0))

    def linear_program_form(self, program, key, out, coefs=None):
        """lig_linear_program_form: linear_form without the prepare; coefs: a table of values for this call (None: the program's)
        -> the constant (32 bytes)"""
        kb = np.frombuffer(bytes(key), dtype=np.uint8).copy()
        cs = np.zeros(32, dtype=np.uint8)
        tab = coef_table(coefs) if coefs is not None else None
        self.check(self.L.lig_linear_program_form(self.h, program._handle(), _hptr(kb), _hptr(tab) if tab is not None and len(tab) else None,
                                                  len(tab) if tab is not None else 0, out, _hptr(cs)))
        return cs.tobytes()

    def rows_diagnose(self, trace, system=None, lin_cap=1024, quad_cap=1024):
        """lig_rows_diagnose: which constraints of `system` (None: the quadratic part only) and which quadratic terms does the committed
        witness violate -> (DiagInfo, linear records, quadratic records): numpy record arrays (DIAG_LINEAR, DIAG_QUAD) of the first
        lin_cap / quad_cap violations in ascending order; the counts in DiagInfo cover all of them"""
        info = DiagInfo()
        info.struct_bytes = C.sizeof(DiagInfo)
        lin, quad = np.zeros(lin_cap, dtype=DIAG_LINEAR), np.zeros(quad_cap, dtype=DIAG_QUAD)
        self.check(self.L.lig_rows_diagnose(trace, C.byref(system) if system is not None else None, _hptr(lin) if lin_cap else None, lin_cap,
                                            _hptr(quad) if quad_cap else None, quad_cap, C.byref(info)))
        return info, lin[:info.n_linear_reported], quad[:info.n_quad_reported]

    def rows_diagnose_attached(self, trace, lin_cap=1024, quad_cap=1024):
        """lig_rows_diagnose_attached: rows_diagnose against the statement attached to the trace (rows_set_linear / rows_attach_linear, with
        the values of rows_set_linear_values in force): no term list is passed -> the same triple as rows_diagnose"""
        info = DiagInfo()
        info.struct_bytes = C.sizeof(DiagInfo)
        lin, quad = np.zeros(lin_cap, dtype=DIAG_LINEAR), np.zeros(quad_cap, dtype=DIAG_QUAD)
        self.check(self.L.lig_rows_diagnose_attached(trace, _hptr(lin) if lin_cap else None, lin_cap, _hptr(quad) if quad_cap else None, quad_cap,
                                                     C.byref(info)))
        return info, lin[:info.n_linear_reported], quad[:info.n_quad_reported]

    def _rows_explain(self, call, head, constraints, term_cap):
        info = ExplainInfo()
        info.struct_bytes = C.sizeof(ExplainInfo)
        asked = np.ascontiguousarray(constraints, dtype=np.uint32)
        con, terms = np.zeros(len(asked), dtype=EXPLAIN_CONSTRAINT), np.zeros(term_cap, dtype=EXPLAIN_TERM)
        self.check(call(*head, _hptr(asked) if len(asked) else None, len(asked), _hptr(con) if len(asked) else None,
                        _hptr(terms) if term_cap else None, term_cap, C.byref(info)))
        return info, con, terms[:info.n_terms_reported]

    def rows_explain(self, trace, system, constraints, term_cap=4096):
        """lig_rows_explain: the constraints `constraints` (numbers, strictly ascending) of `system` as the library holds them ->
        (ExplainInfo, constraint records, term records): numpy record arrays (EXPLAIN_CONSTRAINT: n_terms, first_term, rhs, residual;
        EXPLAIN_TERM: slot, coef_index, coefficient value, committed witness value), the first term_cap terms in ascending (constraint,
        slot, coef_index) order; the counts cover all terms"""
        return self._rows_explain(self.L.lig_rows_explain, (trace, C.byref(system) if system is not None else None), constraints, term_cap)

    def rows_explain_attached(self, trace, constraints, term_cap=4096):
        """lig_rows_explain_attached: rows_explain against the statement attached to the trace (rows_set_linear / rows_attach_linear, with
        the values of rows_set_linear_values in force): no term list is passed -> the same triple as rows_explain"""
        return self._rows_explain(self.L.lig_rows_explain_attached, (trace,), constraints, term_cap)

    def rows_read_slots(self, trace, slots):
        """lig_rows_read_slots: the committed witness elements of `slots` (row * l + column over the committed rows of any kind; any order,
        repeats allowed) -> (n, 8) uint32 limbs, canonical"""
        sl = np.ascontiguousarray(slots, dtype=np.uint32)
        out = np.zeros((len(sl), 8), dtype=np.uint32)
        self.check(self.L.lig_rows_read_slots(trace, _hptr(sl) if len(sl) else None, len(sl), _hptr(out) if len(sl) else None))
        return out

    def _rows_explain_slots(self, call, head, slots, term_cap):
        info = SlotInfo()
        info.struct_bytes = C.sizeof(SlotInfo)
        asked = np.ascontiguousarray(slots, dtype=np.uint32)
        rec, terms = np.zeros(len(asked), dtype=SLOT_RECORD), np.zeros(term_cap, dtype=SLOT_TERM)
        self.check(call(*head, _hptr(asked) if len(asked) else None, len(asked), _hptr(rec) if len(asked) else None,
                        _hptr(terms) if term_cap else None, term_cap, C.byref(info)))
        return info, rec, terms[:info.n_terms_reported]

    def rows_explain_slots(self, trace, system, slots, term_cap=4096):
        """lig_rows_explain_slots: the constraints of `system` through the slots `slots` (row * l + column, strictly ascending) ->
        (SlotInfo, slot records, term records): numpy record arrays (SLOT_RECORD: row_kind, n_terms, first_term, committed value;
        SLOT_TERM: constraint, coef_index, the constraint's term count, coefficient value, the constraint's residual), the first term_cap
        terms in ascending (slot, constraint, coef_index) order; the counts cover all terms"""
        return self._rows_explain_slots(self.L.lig_rows_explain_slots, (trace, C.byref(system) if system is not None else None), slots, term_cap)

    def rows_explain_slots_attached(self, trace, slots, term_cap=4096):
        """lig_rows_explain_slots_attached: rows_explain_slots against the statement attached to the trace (rows_set_linear /
        rows_attach_linear, with the values of rows_set_linear_values in force): no term list is passed -> the same triple"""
        return self._rows_explain_slots(self.L.lig_rows_explain_slots_attached, (trace,), slots, term_cap)

    def _rows_untouched_slots(self, call, head, nonzero_only, cap):
        info = UntouchedInfo()
        info.struct_bytes = C.sizeof(UntouchedInfo)
        out = np.zeros(cap, dtype=SLOT_VALUE)
        self.check(call(*head, 1 if nonzero_only else 0, _hptr(out) if cap else None, cap, C.byref(info)))
        return info, out[:info.n_reported]

    def rows_untouched_slots(self, trace, system, nonzero_only=False, cap=1024):
        """lig_rows_untouched_slots: the slots of the LINEAR / QX / QY / QZ rows that no term of `system` touches -> (UntouchedInfo, numpy
        SLOT_VALUE records of the first `cap` of them in ascending order, each with its row kind and committed value); nonzero_only: only
        those whose committed value is not zero.  The two counts in UntouchedInfo always cover all of them"""
        return self._rows_untouched_slots(self.L.lig_rows_untouched_slots, (trace, C.byref(system) if system is not None else None), nonzero_only, cap)

    def rows_untouched_slots_attached(self, trace, nonzero_only=False, cap=1024):
        """lig_rows_untouched_slots_attached: rows_untouched_slots against the statement attached to the trace -> the same pair"""
        return self._rows_untouched_slots(self.L.lig_rows_untouched_slots_attached, (trace,), nonzero_only, cap)

    def shard_rows_diagnose(self, shard, system=None, lin_cap=1024, quad_cap=1024):
        """lig_shard_rows_diagnose: rows_diagnose on a rows shard.  Collective: every rank passes the same `system` (of the WHOLE trace) and
        the same caps, and every rank gets what rows_diagnose gives for the whole trace on one GPU (global row numbers)"""
        info = DiagInfo()
        info.struct_bytes = C.sizeof(DiagInfo)
        lin, quad = np.zeros(lin_cap, dtype=DIAG_LINEAR), np.zeros(quad_cap, dtype=DIAG_QUAD)
        self.check(self.L.lig_shard_rows_diagnose(shard, C.byref(system) if system is not None else None, _hptr(lin) if lin_cap else None, lin_cap,
                                                  _hptr(quad) if quad_cap else None, quad_cap, C.byref(info)))
        return info, lin[:info.n_linear_reported], quad[:info.n_quad_reported]

    def shard_rows_set_linear_values(self, shard, coefs):
        """lig_shard_rows_set_linear_values: rows_set_linear_values on a rows shard -- this rank's values of the coefficient table of the
        system of shard_rows_set_linear (integers or (n, 8) uint32); None: the system's own.  Every rank passes the same table; no collective"""
        tab = coef_table(coefs) if coefs is not None else None
        self.check(self.L.lig_shard_rows_set_linear_values(shard, _hptr(tab) if tab is not None and len(tab) else None, len(tab) if tab is not None else 0))

    def shard_rows_diagnose_attached(self, shard, lin_cap=1024, quad_cap=1024):
        """lig_shard_rows_diagnose_attached: shard_rows_diagnose against the system attached to the shard (shard_rows_set_linear, with the
        values of shard_rows_set_linear_values in force): no term list is passed.  Collective: every rank passes the same caps and gets
        the same triple as shard_rows_diagnose"""
        info = DiagInfo()
        info.struct_bytes = C.sizeof(DiagInfo)
        lin, quad = np.zeros(lin_cap, dtype=DIAG_LINEAR), np.zeros(quad_cap, dtype=DIAG_QUAD)
        self.check(self.L.lig_shard_rows_diagnose_attached(shard, _hptr(lin) if lin_cap else None, lin_cap, _hptr(quad) if quad_cap else None, quad_cap,
                                                           C.byref(info)))
        return info, lin[:info.n_linear_reported], quad[:info.n_quad_reported]

    def shard_rows_explain(self, shard, system, constraints, term_cap=4096):
        """lig_shard_rows_explain: rows_explain on a rows shard.  Collective: every rank passes the same `system` (of the WHOLE trace, global
        slots), the same constraints and the same term_cap, and every rank gets the triple rows_explain gives for the whole trace on one GPU"""
        return self._rows_explain(self.L.lig_shard_rows_explain, (shard, C.byref(system) if system is not None else None), constraints, term_cap)

    def shard_rows_explain_attached(self, shard, constraints, term_cap=4096):
        """lig_shard_rows_explain_attached: shard_rows_explain against the system attached to the shard (shard_rows_set_linear, with the
        values of shard_rows_set_linear_values in force): no term list is passed.  Collective: every rank passes the same constraints and
        the same term_cap and gets the same triple as shard_rows_explain"""
        return self._rows_explain(self.L.lig_shard_rows_explain_attached, (shard,), constraints, term_cap)

    def shard_rows_explain_slots(self, shard, system, slots, term_cap=4096):
        """lig_shard_rows_explain_slots: rows_explain_slots on a rows shard.  Collective: every rank passes the same `system` (of the WHOLE
        trace), the same GLOBAL slots (row * l + column over the rows of the whole trace, strictly ascending) and the same term_cap, and
        every rank gets the triple rows_explain_slots gives for the whole trace on one GPU"""
        return self._rows_explain_slots(self.L.lig_shard_rows_explain_slots, (shard, C.byref(system) if system is not None else None), slots, term_cap)

    def shard_rows_explain_slots_attached(self, shard, slots, term_cap=4096):
        """lig_shard_rows_explain_slots_attached: shard_rows_explain_slots against the system attached to the shard (shard_rows_set_linear,
        with the values of shard_rows_set_linear_values in force): no term list is passed.  Collective -> the same triple on every rank"""
        return self._rows_explain_slots(self.L.lig_shard_rows_explain_slots_attached, (shard,), slots, term_cap)

    def shard_rows_untouched_slots(self, shard, system, nonzero_only=False, cap=1024):
        """lig_shard_rows_untouched_slots: rows_untouched_slots on a rows shard.  Collective: every rank passes the same `system` (of the
        WHOLE trace), nonzero_only and cap, and every rank gets the pair rows_untouched_slots gives for the whole trace on one GPU (global
        slots; the counts cover all ranks)"""
        return self._rows_untouched_slots(self.L.lig_shard_rows_untouched_slots, (shard, C.byref(system) if system is not None else None), nonzero_only, cap)

    def shard_rows_untouched_slots_attached(self, shard, nonzero_only=False, cap=1024):
        """lig_shard_rows_untouched_slots_attached: shard_rows_untouched_slots against the system attached to the shard.  Collective -> the
        same pair on every rank"""
        return self._rows_untouched_slots(self.L.lig_shard_rows_untouched_slots_attached, (shard,), nonzero_only, cap)

    def shard_rows_read_slots(self, shard, slots):
        """lig_shard_rows_read_slots: rows_read_slots on a rows shard.  Collective: every rank passes the same global slots (row * l + column
        over the rows of the WHOLE trace) and gets the same (n, 8) uint32 limbs, whichever rank holds the rows"""
        sl = np.ascontiguousarray(slots, dtype=np.uint32)
        out = np.zeros((len(sl), 8), dtype=np.uint32)
        self.check(self.L.lig_shard_rows_read_slots(shard, _hptr(sl) if len(sl) else None, len(sl), _hptr(out) if len(sl) else None))
        return out

    def vtrace_destroy(self, vtrace):
        """give up a verification between begin and finish (finish frees the trace itself)"""
        self.L.lig_vtrace_destroy(vtrace)

    def rng_fill_rows(self, key, first_elem, per_row, out):
        k = np.frombuffer(bytes(key), dtype=np.uint8).copy()
        pr = np.ascontiguousarray(per_row, dtype=np.uint32)
        self.check(self.L.lig_rng_fill_rows(self.h, _hptr(k), first_elem, _hptr(pr), len(pr), out))

    def trace_destroy(self, trace):
        self.L.lig_trace_destroy(trace)

    def profile_enable(self, on=True):
        self.check(self.L.lig_profile_enable(self.h, int(on)))

    def profile_read(self):
        a, b, ms = C.c_uint64(), C.c_uint64(), C.c_double()
        self.check(self.L.lig_profile_read(self.h, C.byref(a), C.byref(b), C.byref(ms)))
        return a.value, b.value, ms.value

    def profile_read_launches(self, rows_in_launch):
        """lig_profile_read_launches -> (launches of exactly that many rows, their summed ms)"""
        a, ms = C.c_uint64(), C.c_double()
        self.check(self.L.lig_profile_read_launches(self.h, rows_in_launch, C.byref(a), C.byref(ms)))
        return a.value, ms.value

    def rng_fill(self, key, first_elem, out, count):
        k = np.frombuffer(bytes(key), dtype=np.uint8).copy()
        self.check(self.L.lig_rng_fill(self.h, _hptr(k), first_elem, out, count))
