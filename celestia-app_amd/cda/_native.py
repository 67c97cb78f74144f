"""ctypes binding of libcda.so (include/cda.h).

The product path: every compute call goes through the HIP library.  There is
no CPU fallback — if libcda.so is missing or no GPU is visible the calls raise.
"""
import ctypes
import os
import threading

import numpy as np

_HERE = os.path.dirname(os.path.abspath(__file__))
# CDA_LIB: another build of the library (A/B measurements of kernel variants on one box)
LIB_PATH = os.environ.get("CDA_LIB") or os.path.join(_HERE, "libcda.so")
# the test-hooks build of the same sources (-DCDA_TEST_HOOKS=1, `make hooks`): failure injection through
# CDA_FAULT_INJECT, which a release libcda.so ignores.  Only the fault tests load it, beside the release library.
HOOKS_LIB_PATH = os.path.join(_HERE, "libcda_hooks.so")

SHARE_SIZE = 512
NAMESPACE_SIZE = 29
NODE_SIZE = 90
HASH_SIZE = 32
REC_BYTES = 96

OK = 0
E_NOT_POW2 = -1
E_NOT_SQUARE = -2
E_SHARD_SIZE = -3
E_NS_SHORT = -4
E_NS_ORDER = -5
E_TOO_FEW = -6
E_UNREPAIRABLE = -7
E_BYZANTINE = -8
E_ARG = -9
E_DEVICE = -10
E_PUSH_PAST = -11
E_UNSUPPORTED = -12
E_SHARE_VERSION = -13
E_BLOB_SIZE = -14
E_NOMEM = -15
E_INTERNAL = -16

AXIS_ROW = 0
AXIS_COL = 1

# Every symbol declared in include/cda.h (checked by tests/test_abi.py).
EXPORTS = [
    "cda_init", "cda_free", "cda_strerror", "cda_last_device_error", "cda_build_info",
    "cda_rs_encode", "cda_rs_decode", "cda_rs_max_chunks", "cda_rs_name", "cda_rs_validate_chunk_size",
    "cda_extend_commit", "cda_extend_commit_batch", "cda_extend_commit_device", "cda_commit_eds", "cda_extend_commit_eds",
    "cda_dah_hash", "cda_nmt_axis_root", "cda_repair", "cda_repair_device",
    "cda_rs_encode_device", "cda_nmt_roots_device", "cda_nmt_fold_device", "cda_dah_device",
    "cda_profile_enable", "cda_profile_read", "cda_profile_reset",
    "cda_blob_commitments", "cda_merkle_roots", "cda_extend_commit_nodes", "cda_share_inclusion_proof",
    "cda_host_alloc", "cda_host_free", "cda_multi_init", "cda_multi_free", "cda_multi_device_count",
    "cda_multi_context", "cda_multi_device", "cda_multi_extend_commit_batch", "cda_build_ods_device",
    "cda_construct_extend_commit", "cda_multi_extend_commit_split", "cda_multi_extend_commit_split_device",
    "cda_multi_init_replicas", "cda_set_option", "cda_host_register", "cda_host_unregister",
    "cda_square_open", "cda_square_close", "cda_square_prove", "cda_nmt_verify", "cda_nmt_verify_device",
    "cda_square_share_proofs", "cda_share_proofs_validate", "cda_share_proofs_validate_device",
    "cda_square_prove_namespace", "cda_nmt_verify_namespace", "cda_nmt_verify_namespace_device",
    "cda_square_open_eds", "cda_befp_validate", "cda_befp_validate_device",
    "cda_samples_assemble_device", "cda_square_open_eds_device", "cda_square_rebuild",
    "cda_commitment_proof_sizes", "cda_square_commitment_proofs", "cda_commitment_proofs_verify",
    "cda_commitment_proofs_verify_device", "cda_square_index", "cda_square_read",
    "cda_square_axis_halves", "cda_axis_halves_verify", "cda_axis_halves_verify_device",
    "cda_axis_halves_assemble_device", "cda_square_rebuild_axes",
    "cda_extend_commit_mixed", "cda_extend_commit_mixed_device",
]

OPT_HUGE_PAGES = 1
OPT_MIXED_SMALL_MAX = 2


class ErrInfo(ctypes.Structure):
    _fields_ = [("code", ctypes.c_int32), ("axis", ctypes.c_int32), ("index", ctypes.c_int32),
                ("leaf", ctypes.c_int32), ("block", ctypes.c_int32)]


class ShareSegment(ctypes.Structure):
    """cda_share_segment (include/cda.h): one run of shares of a square plan."""
    _fields_ = [("kind", ctypes.c_uint32), ("first_share", ctypes.c_uint32), ("nshares", ctypes.c_uint32),
                ("share_version", ctypes.c_uint32), ("data_off", ctypes.c_uint64), ("data_len", ctypes.c_uint64),
                ("reserved_off", ctypes.c_uint32), ("ns", ctypes.c_uint8 * 29), ("pad_", ctypes.c_uint8 * 3)]


class ShareProofInfo(ctypes.Structure):
    _fields_ = [("start_row", ctypes.c_uint32), ("end_row", ctypes.c_uint32), ("nrows", ctypes.c_uint32),
                ("total", ctypes.c_uint32), ("naunts", ctypes.c_uint32), ("max_nodes", ctypes.c_uint32)]


class RangeQuery(ctypes.Structure):
    """cda_range_query: tree (axis, index).ProveRange(start, end)."""
    _fields_ = [("axis", ctypes.c_uint32), ("index", ctypes.c_uint32), ("start", ctypes.c_uint32),
                ("end", ctypes.c_uint32)]


class NmtProofDesc(ctypes.Structure):
    """cda_nmt_proof_desc: one proof of a cda_nmt_verify batch."""
    _fields_ = [("start", ctypes.c_uint32), ("end", ctypes.c_uint32), ("node_off", ctypes.c_uint32),
                ("nnodes", ctypes.c_uint32), ("leaf_off", ctypes.c_uint32), ("root", ctypes.c_uint32)]


class ShareRange(ctypes.Structure):
    """cda_share_range: ODS shares [start, end), row-major."""
    _fields_ = [("start", ctypes.c_uint32), ("end", ctypes.c_uint32)]


class ShareRow(ctypes.Structure):
    """cda_share_row: one row of a ShareProof (its NMTProof and the merkle Proof of its row root)."""
    _fields_ = [("nmt_start", ctypes.c_int32), ("nmt_end", ctypes.c_int32), ("node_off", ctypes.c_uint32),
                ("nnodes", ctypes.c_uint32), ("total", ctypes.c_int64), ("index", ctypes.c_int64),
                ("aunt_off", ctypes.c_uint32), ("naunts", ctypes.c_uint32), ("row", ctypes.c_uint32),
                ("pad_", ctypes.c_uint32)]


class ShareProofDesc(ctypes.Structure):
    """cda_share_proof_desc: one ShareProof of a cda_share_proofs_validate batch."""
    _fields_ = [("row_off", ctypes.c_uint32), ("nshare_proofs", ctypes.c_uint32), ("nrow_roots", ctypes.c_uint32),
                ("nrow_proofs", ctypes.c_uint32), ("leaf_off", ctypes.c_uint32), ("nleaves", ctypes.c_uint32),
                ("start_row", ctypes.c_uint32), ("end_row", ctypes.c_uint32), ("data_root", ctypes.c_uint32),
                ("ns", ctypes.c_uint8 * 29), ("pad_", ctypes.c_uint8 * 3)]


class BlobRange(ctypes.Structure):
    """cda_blob_range: ODS shares [start, start + len), row-major."""
    _fields_ = [("start", ctypes.c_uint32), ("len", ctypes.c_uint32)]


class CommitmentRow(ctypes.Structure):
    """cda_commitment_row: one row of a commitment proof (its subtree roots, its NMTProof nodes, its row proof)."""
    _fields_ = [("nmt_start", ctypes.c_int32), ("nmt_end", ctypes.c_int32), ("node_off", ctypes.c_uint32),
                ("nnodes", ctypes.c_uint32), ("root_off", ctypes.c_uint32), ("nroots", ctypes.c_uint32),
                ("total", ctypes.c_int64), ("index", ctypes.c_int64), ("aunt_off", ctypes.c_uint32),
                ("naunts", ctypes.c_uint32), ("row", ctypes.c_uint32), ("pad_", ctypes.c_uint32)]


class CommitmentProofDesc(ctypes.Structure):
    """cda_commitment_proof_desc: one proof of a cda_commitment_proofs_verify batch."""
    _fields_ = [("row_off", ctypes.c_uint32), ("nrows", ctypes.c_uint32), ("start_row", ctypes.c_uint32),
                ("end_row", ctypes.c_uint32), ("data_root", ctypes.c_uint32), ("commitment", ctypes.c_uint32),
                ("subtree_root_threshold", ctypes.c_uint32), ("ns", ctypes.c_uint8 * 29), ("pad_", ctypes.c_uint8 * 3)]


class Sequence(ctypes.Structure):
    """cda_sequence: one sequence of a retained square (cda_square_index)."""
    _fields_ = [("start", ctypes.c_uint32), ("nshares", ctypes.c_uint32), ("seq_len", ctypes.c_uint32),
                ("kind", ctypes.c_uint8), ("share_version", ctypes.c_uint8), ("status", ctypes.c_uint8),
                ("pad_", ctypes.c_uint8), ("ns", ctypes.c_uint8 * 29), ("pad2_", ctypes.c_uint8 * 3)]


class SquareSummary(ctypes.Structure):
    """cda_square_summary: what cda_square_index counted."""
    _fields_ = [("k", ctypes.c_uint32), ("nseq", ctypes.c_uint32), ("npadding", ctypes.c_uint32),
                ("norphans", ctypes.c_uint32), ("first_orphan", ctypes.c_uint32)]


class SequenceRange(ctypes.Structure):
    """cda_sequence_range: one query of cda_square_read."""
    _fields_ = [("start", ctypes.c_uint32), ("nshares", ctypes.c_uint32), ("seq_len", ctypes.c_uint32),
                ("compact", ctypes.c_uint32)]


class NamespaceQuery(ctypes.Structure):
    """cda_namespace_query: tree (axis, index).ProveNamespace(ns)."""
    _fields_ = [("axis", ctypes.c_uint32), ("index", ctypes.c_uint32), ("ns", ctypes.c_uint8 * 29),
                ("pad_", ctypes.c_uint8 * 3)]


class NamespaceResult(ctypes.Structure):
    """cda_namespace_result: what cda_square_prove_namespace found for one query."""
    _fields_ = [("kind", ctypes.c_uint32), ("start", ctypes.c_uint32), ("end", ctypes.c_uint32),
                ("nnodes", ctypes.c_uint32), ("share_off", ctypes.c_uint32), ("nshares", ctypes.c_uint32)]


class NmtNsProofDesc(ctypes.Structure):
    """cda_nmt_ns_proof_desc: one proof of a cda_nmt_verify_namespace batch."""
    _fields_ = [("start", ctypes.c_uint32), ("end", ctypes.c_uint32), ("node_off", ctypes.c_uint32),
                ("nnodes", ctypes.c_uint32), ("leaf_off", ctypes.c_uint32), ("nleaves", ctypes.c_uint32),
                ("root", ctypes.c_uint32), ("leaf_hash", ctypes.c_uint32)]


class BefpDesc(ctypes.Structure):
    """cda_befp_desc: one bad-encoding fraud proof of a cda_befp_validate batch."""
    _fields_ = [("axis", ctypes.c_uint32), ("index", ctypes.c_uint32), ("entry_off", ctypes.c_uint32),
                ("nshares", ctypes.c_uint32), ("root_off", ctypes.c_uint32)]


class BefpEntry(ctypes.Structure):
    """cda_befp_entry: one share of a bad-encoding fraud proof and where its NMT proof's nodes lie."""
    _fields_ = [("pos", ctypes.c_uint32), ("node_off", ctypes.c_uint32), ("nnodes", ctypes.c_uint32)]


# cda_befp_validate's verdicts (include/cda.h CDA_BEFP_*)
BEFP_FRAUD, BEFP_NO_FRAUD, BEFP_MALFORMED, BEFP_TOO_FEW, BEFP_BAD_SHARE = 1, 0, -1, -2, -3


class SampleDesc(ctypes.Structure):
    """cda_sample_desc: one proved cell of a cda_square_rebuild / cda_samples_assemble_device batch."""
    _fields_ = [("axis", ctypes.c_uint32), ("index", ctypes.c_uint32), ("pos", ctypes.c_uint32),
                ("node_off", ctypes.c_uint32), ("nnodes", ctypes.c_uint32)]


# the per-sample statuses of an assembled square (include/cda.h CDA_SAMPLE_*)
SAMPLE_PLACED, SAMPLE_DUPLICATE, SAMPLE_CONFLICT, SAMPLE_REJECTED, SAMPLE_MALFORMED = range(5)


class AxisHalfDesc(ctypes.Structure):
    """cda_axis_half_desc: k consecutive cells of a row or a column, cells [side k, side k + k)."""
    _fields_ = [("axis", ctypes.c_uint32), ("index", ctypes.c_uint32), ("side", ctypes.c_uint32),
                ("root_off", ctypes.c_uint32)]


# which half of the axis (include/cda.h CDA_SIDE_*), and the per-half statuses (CDA_HALF_*)
SIDE_FIRST, SIDE_SECOND = 0, 1
HALF_PLACED, HALF_DUPLICATE, HALF_CONFLICT, HALF_BAD_ROOT, HALF_MALFORMED = range(5)

# cda_namespace_result.kind (include/cda.h CDA_NSP_*), and "no leaf hash" of a cda_nmt_ns_proof_desc
NSP_EMPTY, NSP_INCLUSION, NSP_ABSENCE = range(3)
NO_LEAF_HASH = 0xFFFFFFFF

# ShareProof.Validate's checks in its order (include/cda.h CDA_SP_*)
SP_VALID, SP_PROOF_COUNT, SP_DATA_COUNT, SP_NEG_START, SP_EMPTY_RANGE, SP_ROW_COUNT, SP_ROW_PROOFS, SP_ROW_PROOF, \
    SP_SHARE_PROOF, SP_MALFORMED = range(10)

# cda_commitment_proofs_verify's verdicts: 0, or the first of rules C0-C8 that fails (include/cda.h CDA_CP_*)
CP_VALID, CP_MALFORMED, CP_ROW_COUNT, CP_RANGE, CP_ALIGNMENT, CP_ROOT_COUNT, CP_NAMESPACE, CP_ROW_PROOF, \
    CP_SUBTREE_ROOTS, CP_COMMITMENT = range(10)

# the same records as numpy rows (whole batches are built as arrays)
# cda_sequence's kind and status bits (include/cda.h CDA_SEQ_*)
SEQ_KIND_TX, SEQ_KIND_PFB, SEQ_KIND_BLOB = 0, 1, 2
SEQ_TRUNCATED, SEQ_BROKEN, SEQ_VERSION, SEQ_RESERVED_NS, SEQ_UNALIGNED = 1, 2, 4, 8, 16
NO_SHARE = 0xFFFFFFFF
SEQUENCE_DTYPE = np.dtype([("start", "<u4"), ("nshares", "<u4"), ("seq_len", "<u4"), ("kind", "u1"),
                           ("share_version", "u1"), ("status", "u1"), ("pad_", "u1"), ("ns", "u1", (29,)),
                           ("pad2_", "u1", (3,))])
SEQUENCE_RANGE_DTYPE = np.dtype([("start", "<u4"), ("nshares", "<u4"), ("seq_len", "<u4"), ("compact", "<u4")])
BLOB_RANGE_DTYPE = np.dtype([("start", "<u4"), ("len", "<u4")])
COMMITMENT_ROW_DTYPE = np.dtype([("nmt_start", "<i4"), ("nmt_end", "<i4"), ("node_off", "<u4"), ("nnodes", "<u4"),
                                 ("root_off", "<u4"), ("nroots", "<u4"), ("total", "<i8"), ("index", "<i8"),
                                 ("aunt_off", "<u4"), ("naunts", "<u4"), ("row", "<u4"), ("pad_", "<u4")])
COMMITMENT_PROOF_DESC_DTYPE = np.dtype([("row_off", "<u4"), ("nrows", "<u4"), ("start_row", "<u4"), ("end_row", "<u4"),
                                        ("data_root", "<u4"), ("commitment", "<u4"),
                                        ("subtree_root_threshold", "<u4"), ("ns", "u1", (29,)), ("pad_", "u1", (3,))])
SHARE_RANGE_DTYPE = np.dtype([("start", "<u4"), ("end", "<u4")])
SHARE_ROW_DTYPE = np.dtype([("nmt_start", "<i4"), ("nmt_end", "<i4"), ("node_off", "<u4"), ("nnodes", "<u4"),
                            ("total", "<i8"), ("index", "<i8"), ("aunt_off", "<u4"), ("naunts", "<u4"),
                            ("row", "<u4"), ("pad_", "<u4")])
SHARE_PROOF_DESC_DTYPE = np.dtype([("row_off", "<u4"), ("nshare_proofs", "<u4"), ("nrow_roots", "<u4"),
                                   ("nrow_proofs", "<u4"), ("leaf_off", "<u4"), ("nleaves", "<u4"),
                                   ("start_row", "<u4"), ("end_row", "<u4"), ("data_root", "<u4"),
                                   ("ns", "u1", (29,)), ("pad_", "u1", (3,))])
NAMESPACE_QUERY_DTYPE = np.dtype([("axis", "<u4"), ("index", "<u4"), ("ns", "u1", (29,)), ("pad_", "u1", (3,))])
NAMESPACE_RESULT_DTYPE = np.dtype([("kind", "<u4"), ("start", "<u4"), ("end", "<u4"), ("nnodes", "<u4"),
                                   ("share_off", "<u4"), ("nshares", "<u4")])
NMT_NS_PROOF_DESC_DTYPE = np.dtype([("start", "<u4"), ("end", "<u4"), ("node_off", "<u4"), ("nnodes", "<u4"),
                                    ("leaf_off", "<u4"), ("nleaves", "<u4"), ("root", "<u4"), ("leaf_hash", "<u4")])
BEFP_DESC_DTYPE = np.dtype([("axis", "<u4"), ("index", "<u4"), ("entry_off", "<u4"), ("nshares", "<u4"),
                            ("root_off", "<u4")])
BEFP_ENTRY_DTYPE = np.dtype([("pos", "<u4"), ("node_off", "<u4"), ("nnodes", "<u4")])
SAMPLE_DESC_DTYPE = np.dtype([("axis", "<u4"), ("index", "<u4"), ("pos", "<u4"), ("node_off", "<u4"),
                              ("nnodes", "<u4")])
AXIS_HALF_DESC_DTYPE = np.dtype([("axis", "<u4"), ("index", "<u4"), ("side", "<u4"), ("root_off", "<u4")])
RANGE_QUERY_DTYPE = np.dtype([("axis", "<u4"), ("index", "<u4"), ("start", "<u4"), ("end", "<u4")])
NMT_PROOF_DESC_DTYPE = np.dtype([("start", "<u4"), ("end", "<u4"), ("node_off", "<u4"), ("nnodes", "<u4"),
                                 ("leaf_off", "<u4"), ("root", "<u4")])


class CdaError(Exception):
    """Error returned by libcda; `code` is a CDA_E_* value."""

    def __init__(self, code, msg="", axis=-1, index=-1, leaf=-1, block=-1):
        self.code, self.axis, self.index, self.leaf, self.block = code, axis, index, leaf, block
        super().__init__(f"{msg or strerror(code)} (code {code}, axis {axis}, index {index}, leaf {leaf})")


_libs = {}
_lib_lock = threading.Lock()


def lib(path=None, older=False):
    """Load libcda.so, or the build at `path` (raises if it was not built: no silent fallback).  older: `path` is a
    build of an earlier commit (an A/B probe's other side): the calls it lacks are left unbound instead of refused;
    a Context(lib_path=path) made afterwards uses it."""
    path = path or LIB_PATH
    with _lib_lock:
        if path not in _libs:
            if not os.path.exists(path):
                raise RuntimeError(f"libcda not built at {path}; run __graft_entry__.build()")
            L = ctypes.CDLL(path)
            P, U32, I32, U64, I64, SZ = (ctypes.c_void_p, ctypes.c_uint32, ctypes.c_int, ctypes.c_uint64,
                                          ctypes.c_int64, ctypes.c_size_t)
            sig = {
                "cda_init": (I32, [I32, ctypes.POINTER(P)]),
                "cda_free": (None, [P]),
                "cda_strerror": (ctypes.c_char_p, [I32]),
                "cda_last_device_error": (ctypes.c_char_p, [P]),
                "cda_build_info": (ctypes.c_char_p, []),
                "cda_rs_encode": (I32, [P, U32, U32, P, P]),
                "cda_rs_decode": (I32, [P, U32, U32, P, P]),
                "cda_rs_max_chunks": (I64, []),
                "cda_rs_name": (ctypes.c_char_p, []),
                "cda_rs_validate_chunk_size": (I32, [I64]),
                "cda_extend_commit": (I32, [P, U32, U32, P, P, P, P, P, P]),
                "cda_extend_commit_batch": (I32, [P, U32, U32, P, P, P, P, P, P]),
                "cda_extend_commit_device": (I32, [P, U32, U32, P, P, P, P, P, P]),
                "cda_commit_eds": (I32, [P, U32, P, P, P, P, P]),
                "cda_extend_commit_eds": (I32, [P, U32, P, P, P, P, P]),
                "cda_dah_hash": (I32, [P, U32, P, P, P]),
                "cda_nmt_axis_root": (I32, [P, U64, U64, U32, U32, P, P, P]),
                "cda_repair": (I32, [P, U32, P, P, P, P, P]),
                "cda_repair_device": (I32, [P, U32, P, P, P, P, P, P]),
                "cda_rs_encode_device": (I32, [P, U32, U32, U32, P, I64, I64, P, I64, I64, P]),
                "cda_nmt_roots_device": (I32, [P, U32, P, U32, U32, U32, U32, U32, P, P, P]),
                "cda_nmt_fold_device": (I32, [P, U32, U32, P, P, P]),
                "cda_dah_device": (I32, [P, U32, P, P, P]),
                "cda_profile_enable": (I32, [P, I32]),
                "cda_profile_read": (I32, [P, P, SZ, P, P, I32]),
                "cda_profile_reset": (I32, [P]),
                "cda_blob_commitments": (I32, [P, U32, P, P, P, P, U32, P, P]),
                "cda_merkle_roots": (I32, [P, U32, P, P, U32, P]),
                "cda_extend_commit_nodes": (I32, [P, U32, U32, P, P, P, P, P, P, P, P, P]),
                "cda_share_inclusion_proof": (I32, [P, U32, U32, P, U32, U32, P, P, P, P, P, P, P, P, P,
                                                      P]),
                "cda_host_alloc": (I32, [P, SZ, ctypes.POINTER(P)]),
                "cda_host_free": (I32, [P, P]),
                "cda_multi_init": (I32, [U32, ctypes.POINTER(P)]),
                "cda_multi_free": (None, [P]),
                "cda_multi_device_count": (I32, [P]),
                "cda_multi_context": (P, [P, I32]),
                "cda_multi_device": (I32, [P, I32]),
                "cda_multi_extend_commit_batch": (I32, [P, U32, U32, P, P, P, P, P, P]),
                "cda_multi_extend_commit_split": (I32, [P, U32, P, P, P, P, P, P]),
                "cda_multi_extend_commit_split_device": (I32, [P, U32, P, P, P, P, P]),
                "cda_multi_init_replicas": (I32, [I32, U32, ctypes.POINTER(P)]),
                "cda_build_ods_device": (I32, [P, U32, U32, P, P, U64, P, U32, P, P]),
                "cda_construct_extend_commit": (I32, [P, U32, U32, P, P, U64, P, U32, P, P, P, P, P, P]),
                "cda_set_option": (I32, [P, I32, I64]),
                "cda_host_register": (I32, [P, P, SZ]),
                "cda_host_unregister": (I32, [P, P]),
                "cda_square_open": (I32, [P, U32, U32, P, ctypes.POINTER(P), P, P, P, P]),
                "cda_square_close": (None, [P]),
                "cda_square_prove": (I32, [P, U32, P, U32, P, P, P, U64]),
                "cda_nmt_verify": (I32, [P, U32, P, P, P, U32, P, U32, P, U32, P]),
                "cda_nmt_verify_device": (I32, [P, U32, P, P, P, U32, P, U32, P, U32, P, P]),
                "cda_square_share_proofs": (I32, [P, U32, P, U32, U32, P, P, P, P, P, P, P, U64, P]),
                "cda_share_proofs_validate": (I32, [P, U32, P, P, P, P, U32, P, U32, P, U32, P, U32, P, U32, P]),
                "cda_share_proofs_validate_device": (I32, [P, U32, P, P, P, P, U32, P, U32, P, U32, P, U32, P, U32, P,
                                                             P]),
                "cda_square_prove_namespace": (I32, [P, U32, P, U32, P, P, P, P, U64, P]),
                "cda_nmt_verify_namespace": (I32, [P, U32, P, P, P, U32, P, U32, P, U32, P, U32, P]),
                "cda_nmt_verify_namespace_device": (I32, [P, U32, P, P, P, U32, P, U32, P, U32, P, U32, P, P]),
                "cda_square_open_eds": (I32, [P, U32, P, ctypes.POINTER(P), P, P, P, P]),
                "cda_befp_validate": (I32, [P, U32, U32, P, P, U32, P, P, U32, P, U32, P]),
                "cda_befp_validate_device": (I32, [P, U32, U32, P, P, U32, P, P, U32, P, U32, P, P]),
                "cda_samples_assemble_device": (I32, [P, U32, U32, P, P, P, U32, P, P, P, P, P]),
                "cda_square_open_eds_device": (I32, [P, U32, P, ctypes.POINTER(P), P, P, P, P, P]),
                "cda_square_rebuild": (I32, [P, U32, U32, P, P, P, U32, P, P, ctypes.POINTER(P), P, P, P, P, P]),
                "cda_commitment_proof_sizes": (I32, [U32, U32, U32, P, P, P]),
                "cda_square_commitment_proofs": (I32, [P, U32, P, U32, U32, U32, U32, P, P, P, P, P, P, P, P, P]),
                "cda_commitment_proofs_verify": (I32, [P, U32, P, P, P, P, U32, P, U32, P, U32, P, U32, P, U32, P, U32,
                                                         P]),
                "cda_commitment_proofs_verify_device": (I32, [P, U32, P, P, P, P, U32, P, U32, P, U32, P, U32, P, U32,
                                                                P, U32, P, P]),
                "cda_square_index": (I32, [P, U32, U32, P, P, P]),
                "cda_square_read": (I32, [P, U32, P, P, U64, P]),
                "cda_square_axis_halves": (I32, [P, U32, P, P, U64]),
                "cda_axis_halves_verify": (I32, [P, U32, U32, P, P, P, U32, P, P]),
                "cda_axis_halves_verify_device": (I32, [P, U32, U32, P, P, P, U32, P, P, P]),
                "cda_axis_halves_assemble_device": (I32, [P, U32, U32, P, P, P, P, P, P, P]),
                "cda_square_rebuild_axes": (I32, [P, U32, U32, P, P, P, P, ctypes.POINTER(P), P, P, P, P, P]),
                "cda_extend_commit_mixed": (I32, [P, U32, P, P, P, P, P, P, P]),
                "cda_extend_commit_mixed_device": (I32, [P, U32, P, P, P, P, P, P, P]),
            }
            for name, (res, args) in sig.items():
                if older and not hasattr(L, name):
                    continue
                f = getattr(L, name)
                f.restype = res
                f.argtypes = args
            _libs[path] = L
    return _libs[path]


def build_info(path=None):
    """cda_build_info(): "release gfx950", or "diagnostic gfx950 <tags>" for a diagnostic or test-hooks build."""
    return lib(path).cda_build_info().decode()


def strerror(code):
    return lib().cda_strerror(code).decode()


def _p(a):
    return None if a is None else a.ctypes.data_as(ctypes.c_void_p)


def mixed_offsets(ks):
    """Where block b of a mixed-size call (cda_extend_commit_mixed) starts in each packed buffer, as int64 arrays of
    len(ks) + 1 entries (the last is the total): "ods" and "eds" in bytes; "roots" in nodes of the host form's
    row_roots / col_roots (2k per block); "recs" in 96-B records of the device form's d_roots (4k per block: the row
    roots, then the column roots)."""
    k = np.asarray(ks, np.int64)
    cum = lambda v: np.concatenate([[0], np.cumsum(v)]).astype(np.int64)  # noqa: E731
    return {"ods": cum(k * k * SHARE_SIZE), "eds": cum(4 * k * k * SHARE_SIZE), "roots": cum(2 * k), "recs": cum(4 * k)}


def _check(rc, err=None, ctx=None):
    if rc == OK:
        return
    if rc in (E_DEVICE, E_NOMEM, E_INTERNAL) and ctx is not None:
        raise CdaError(rc, strerror(rc) + ": " + ctx._L.cda_last_device_error(ctx._h).decode())
    if err is not None:
        raise CdaError(rc, axis=err.axis, index=err.index, leaf=err.leaf, block=err.block)
    raise CdaError(rc)


class Context:
    """One cda_ctx bound to one HIP device (one process per GPU)."""

    def pinned(self, shape, dtype=np.uint8):
        """Pinned host buffer (cda_host_alloc) for the host-buffer batch path."""
        return PinnedBuffer(self, shape, dtype)

    def __init__(self, device=0, lib_path=None):
        """lib_path: another build of libcda to bind this context to (the test-hooks library); default libcda.so."""
        self._L = lib(lib_path)
        h = ctypes.c_void_p()
        rc = self._L.cda_init(device, ctypes.byref(h))
        if rc != OK:
            raise CdaError(rc, "cda_init failed (no GPU visible?)")
        self._h = h
        self.device = device

    def close(self):
        if getattr(self, "_h", None) and not getattr(self, "_borrowed", False):  # a MultiContext's view: not ours
            self._L.cda_free(self._h)
        self._h = None

    def set_option(self, option, value):
        """cda_set_option (include/cda.h), e.g. OPT_HUGE_PAGES."""
        _check(self._L.cda_set_option(self._h, option, int(value)), ctx=self)

    def host_register(self, array):
        """Page-lock a C-contiguous numpy array's memory for reuse as share / EDS buffers (cda_host_register)."""
        _check(self._L.cda_host_register(self._h, array.ctypes.data_as(ctypes.c_void_p), array.nbytes), ctx=self)

    def host_unregister(self, array):
        _check(self._L.cda_host_unregister(self._h, array.ctypes.data_as(ctypes.c_void_p)), ctx=self)

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    # ---- codec ----
    def rs_encode(self, data):
        data = np.ascontiguousarray(data, np.uint8)
        k, L = data.shape
        parity = np.empty_like(data)
        _check(self._L.cda_rs_encode(self._h, k, L, _p(data), _p(parity)), ctx=self)
        return parity

    def rs_decode(self, shards, present):
        sh = np.ascontiguousarray(shards, np.uint8).copy()
        pres = np.ascontiguousarray(present, np.uint8)
        n, L = sh.shape
        _check(self._L.cda_rs_decode(self._h, n // 2, L, _p(sh), _p(pres)), ctx=self)
        return sh

    # ---- block path ----
    def extend_commit(self, shares, want_eds=True):
        shares = np.ascontiguousarray(shares, np.uint8)
        count, L = shares.shape
        k = max(1, int(round(count ** 0.5)))
        eds = np.empty((4 * k * k, L), np.uint8) if want_eds else None
        rr = np.empty((2 * k, NODE_SIZE), np.uint8)
        cr = np.empty((2 * k, NODE_SIZE), np.uint8)
        dah = np.empty(32, np.uint8)
        err = ErrInfo()
        rc = self._L.cda_extend_commit(self._h, count, L, _p(shares), _p(eds), _p(rr), _p(cr), _p(dah),
                                     ctypes.byref(err))
        _check(rc, err, self)
        return eds, rr, cr, dah.tobytes()

    def extend_commit_batch(self, ods, want_eds=True, eds_out=None):
        """ods: (nblocks, k*k, 512); eds_out: optional preallocated (nblocks, 4k^2, 512) uint8 output."""
        ods, k, eds, rr, cr, dah = _batch_outputs(ods, want_eds, eds_out)
        nb = len(ods)
        err = ErrInfo()
        rc = self._L.cda_extend_commit_batch(self._h, k, nb, _p(ods), _p(eds), _p(rr), _p(cr), _p(dah),
                                           ctypes.byref(err))
        _check(rc, err, self)
        return eds, rr, cr, dah

    def construct_extend_commit(self, k, segs, want_ods=False, want_eds=True, prepared=None):
        """square.Construct + ExtendShares + NewDataAvailabilityHeader from a square plan (cda.square.plan):
        the shares are assembled on the device (cda_construct_extend_commit).  -> (ods, eds, rr, cr, dah).
        prepared: cda.square.device_plan(segs) computed beforehand (the C-ABI records)."""
        from .square import device_plan
        recs, data, reserved = prepared if prepared is not None else device_plan(segs)
        w = 2 * k
        ods = np.empty((k * k, SHARE_SIZE), np.uint8) if want_ods else None
        eds = np.empty((w * w, SHARE_SIZE), np.uint8) if want_eds else None
        rr = np.empty((w, NODE_SIZE), np.uint8)
        cr = np.empty((w, NODE_SIZE), np.uint8)
        dah = np.empty(32, np.uint8)
        err = ErrInfo()
        rc = self._L.cda_construct_extend_commit(self._h, k, len(recs), ctypes.cast(recs, ctypes.c_void_p), _p(data),
                                               sum(r.data_len for r in recs), _p(reserved), len(reserved), _p(ods),
                                               _p(eds), _p(rr), _p(cr), _p(dah), ctypes.byref(err))
        _check(rc, err, self)
        return ods, eds, rr, cr, dah.tobytes()

    def extend_commit_device(self, k, nblocks, d_ods, d_eds, d_roots, d_dah, d_status, stream=None):
        rc = self._L.cda_extend_commit_device(self._h, k, nblocks, ctypes.c_void_p(d_ods), ctypes.c_void_p(d_eds),
                                            ctypes.c_void_p(d_roots), ctypes.c_void_p(d_dah),
                                            ctypes.c_void_p(d_status), ctypes.c_void_p(stream or 0))
        _check(rc, ctx=self)

    # ---- blocks of different sizes in one call ----
    def extend_commit_mixed(self, ods_list, want_eds=True):
        """ods_list: (k*k, 512) arrays, any mix of sizes -> per-block lists (eds or None, row roots, column roots, dah),
        each block as extend_commit returns it (cda_extend_commit_mixed)."""
        blocks = [np.ascontiguousarray(o, np.uint8).reshape(-1, SHARE_SIZE) for o in ods_list]
        ks = np.array([max(1, int(round(len(b) ** 0.5))) for b in blocks], np.uint32)
        if any(int(k) * int(k) != len(b) for k, b in zip(ks, blocks)):
            raise CdaError(E_NOT_SQUARE)
        off = mixed_offsets(ks)
        ods = np.concatenate(blocks) if blocks else np.empty((0, SHARE_SIZE), np.uint8)
        eds = np.empty((off["eds"][-1] // SHARE_SIZE, SHARE_SIZE), np.uint8) if want_eds else None
        rr = np.empty((off["roots"][-1], NODE_SIZE), np.uint8)
        cr = np.empty((off["roots"][-1], NODE_SIZE), np.uint8)
        dah = np.empty((len(blocks), 32), np.uint8)
        err = ErrInfo()
        rc = self._L.cda_extend_commit_mixed(self._h, len(blocks), _p(ks), _p(ods), _p(eds), _p(rr), _p(cr), _p(dah),
                                           ctypes.byref(err))
        _check(rc, err, self)
        cells, roots = off["eds"] // SHARE_SIZE, off["roots"]
        n = len(blocks)
        return ([eds[cells[b]:cells[b + 1]] for b in range(n)] if want_eds else [None] * n,
                [rr[roots[b]:roots[b + 1]] for b in range(n)], [cr[roots[b]:roots[b + 1]] for b in range(n)],
                [dah[b].tobytes() for b in range(n)])

    def extend_commit_mixed_device(self, ks, d_ods, d_eds, d_roots, d_dah, d_status, stream=None):
        """cda_extend_commit_mixed_device: device addresses of buffers packed as mixed_offsets(ks) says; asynchronous
        on `stream` (ks is read before the call returns)."""
        ks = np.ascontiguousarray(ks, np.uint32)
        rc = self._L.cda_extend_commit_mixed_device(self._h, len(ks), _p(ks), ctypes.c_void_p(d_ods),
                                                  ctypes.c_void_p(d_eds), ctypes.c_void_p(d_roots),
                                                  ctypes.c_void_p(d_dah), ctypes.c_void_p(d_status),
                                                  ctypes.c_void_p(stream or 0))
        _check(rc, ctx=self)

    # ---- device-resident building blocks (pointers are device addresses) ----
    def rs_encode_device(self, k, shard_len, ncw, d_src, src_cw, src_sh, d_dst, dst_cw, dst_sh, stream=None):
        rc = self._L.cda_rs_encode_device(self._h, k, shard_len, ncw, ctypes.c_void_p(d_src), src_cw, src_sh,
                                        ctypes.c_void_p(d_dst), dst_cw, dst_sh, ctypes.c_void_p(stream or 0))
        _check(rc, ctx=self)

    def nmt_roots_device(self, k, d_eds, axis, first_index, naxes, leaf_off, nleaves, d_roots, d_status,
                         stream=None):
        rc = self._L.cda_nmt_roots_device(self._h, k, ctypes.c_void_p(d_eds), axis, first_index, naxes, leaf_off,
                                        nleaves, ctypes.c_void_p(d_roots), ctypes.c_void_p(d_status),
                                        ctypes.c_void_p(stream or 0))
        _check(rc, ctx=self)

    def nmt_fold_device(self, ntrees, n, d_nodes, d_roots, stream=None):
        rc = self._L.cda_nmt_fold_device(self._h, ntrees, n, ctypes.c_void_p(d_nodes), ctypes.c_void_p(d_roots),
                                       ctypes.c_void_p(stream or 0))
        _check(rc, ctx=self)

    def dah_device(self, n_total, d_roots, d_dah, stream=None):
        rc = self._L.cda_dah_device(self._h, n_total, ctypes.c_void_p(d_roots), ctypes.c_void_p(d_dah),
                                  ctypes.c_void_p(stream or 0))
        _check(rc, ctx=self)

    def extend_commit_eds(self, eds):
        """In place (cda_extend_commit_eds): eds (4k^2, 512) uint8, C-contiguous, with the ODS in its top-left quadrant
        (row r of the ODS = eds[r * 2k : r * 2k + k]); Q1..Q3 are written around it.  -> (row_roots, col_roots, dah)."""
        if not (isinstance(eds, np.ndarray) and eds.dtype == np.uint8 and eds.flags.c_contiguous and eds.ndim == 2
                and eds.shape[1] == SHARE_SIZE):
            raise ValueError("eds must be a C-contiguous (4k^2, 512) uint8 array")
        w = int(round(eds.shape[0] ** 0.5))
        if w * w != eds.shape[0] or w % 2:
            raise ValueError(f"eds holds {eds.shape[0]} shares, not a (2k)^2 square")
        rr = np.empty((w, NODE_SIZE), np.uint8)
        cr = np.empty((w, NODE_SIZE), np.uint8)
        dah = np.empty(32, np.uint8)
        err = ErrInfo()
        _check(self._L.cda_extend_commit_eds(self._h, w // 2, _p(eds), _p(rr), _p(cr), _p(dah), ctypes.byref(err)),
               err, self)
        return rr, cr, dah.tobytes()

    def commit_eds(self, eds):
        eds = np.ascontiguousarray(eds, np.uint8)
        w = int(round(eds.shape[0] ** 0.5))
        rr = np.empty((w, NODE_SIZE), np.uint8)
        cr = np.empty((w, NODE_SIZE), np.uint8)
        dah = np.empty(32, np.uint8)
        err = ErrInfo()
        _check(self._L.cda_commit_eds(self._h, w // 2, _p(eds), _p(rr), _p(cr), _p(dah), ctypes.byref(err)), err, self)
        return rr, cr, dah.tobytes()

    def dah_hash(self, row_roots, col_roots):
        n = 0 if row_roots is None else len(row_roots)
        rr = np.ascontiguousarray(np.asarray(row_roots, np.uint8).reshape(n, NODE_SIZE)) if n else None
        cr = np.ascontiguousarray(np.asarray(col_roots, np.uint8).reshape(n, NODE_SIZE)) if n else None
        out = np.empty(32, np.uint8)
        _check(self._L.cda_dah_hash(self._h, n, _p(rr), _p(cr), _p(out)), ctx=self)
        return out.tobytes()

    def nmt_axis_root(self, square_size, axis_index, leaves):
        n = len(leaves)
        if n:
            lens = {len(x) for x in leaves}
            leaf_len = min(lens)
            if len(lens) != 1:
                raise CdaError(E_SHARD_SIZE, "leaves of unequal length")
            buf = np.frombuffer(b"".join(bytes(x) for x in leaves), np.uint8).copy()
        else:
            leaf_len, buf = 0, None
        root = np.empty(NODE_SIZE, np.uint8)
        err = ErrInfo()
        rc = self._L.cda_nmt_axis_root(self._h, square_size, axis_index, n, leaf_len, _p(buf), _p(root),
                                     ctypes.byref(err))
        _check(rc, err, self)
        return root.tobytes()

    def repair(self, eds, present, row_roots, col_roots, inplace=False):
        rc, eds, pres, err = self.repair_status(eds, present, row_roots, col_roots, inplace)
        _check(rc, err, self)
        return eds, pres

    def repair_status(self, eds, present, row_roots, col_roots, inplace=False):
        """cda_repair without raising: (rc, eds, present, err) where eds/present hold the square as far as
        it was repaired (rsmt2d leaves the square 'most repaired prior to the Byzantine axis').  inplace=True
        repairs the caller's C-contiguous uint8 arrays themselves (as the C ABI does) instead of copies."""
        if inplace:
            if not (isinstance(eds, np.ndarray) and eds.dtype == np.uint8 and eds.flags.c_contiguous
                    and isinstance(present, np.ndarray) and present.dtype == np.uint8 and present.flags.c_contiguous):
                raise CdaError(E_ARG, "inplace repair needs C-contiguous uint8 arrays")
            pres = present
        else:
            eds = np.ascontiguousarray(eds, np.uint8).copy()
            pres = np.ascontiguousarray(present, np.uint8).copy()
        w = len(row_roots)
        if eds.shape[0] != w * w or eds.size != w * w * SHARE_SIZE or pres.size != w * w:
            raise CdaError(E_ARG, "eds must be (2k)^2 x 512 bytes and present (2k)^2 flags")
        err = ErrInfo()
        rc = self._L.cda_repair(self._h, w // 2, _p(eds), _p(pres), _p(np.ascontiguousarray(row_roots, np.uint8)),
                              _p(np.ascontiguousarray(col_roots, np.uint8)), ctypes.byref(err))
        return rc, eds, pres, err

    def repair_device(self, k, d_eds, present, row_roots, col_roots, stream=None):
        """cda_repair_device: repairs the square at device address d_eds (4k^2 x 512 B) in place.
        -> (rc, present, err); present is a repaired copy of the caller's flags."""
        pres = np.ascontiguousarray(present, np.uint8).copy()
        w = 2 * k
        if pres.size != w * w or len(row_roots) != w or len(col_roots) != w:
            raise CdaError(E_ARG, "present must hold (2k)^2 flags and the roots 2k entries each")
        err = ErrInfo()
        rc = self._L.cda_repair_device(self._h, k, ctypes.c_void_p(d_eds), _p(pres),
                                     _p(np.ascontiguousarray(row_roots, np.uint8)),
                                     _p(np.ascontiguousarray(col_roots, np.uint8)), ctypes.byref(err),
                                     ctypes.c_void_p(stream or 0))
        return rc, pres, err

    # ---- blob share commitments, node export, proofs ----
    def blob_commitments(self, namespaces, datas, share_versions=None, subtree_root_threshold=64):
        """inclusion.CreateCommitments over many blobs in one call -> list of 32-byte commitments."""
        nb = len(datas)
        if nb == 0:
            return []
        ns = np.frombuffer(b"".join(bytes(n) for n in namespaces), np.uint8).copy()
        if ns.size != nb * NAMESPACE_SIZE:
            raise CdaError(E_ARG, "namespaces must be 29 bytes each")
        flat = b"".join(bytes(d) for d in datas)
        data = np.frombuffer(flat, np.uint8).copy() if flat else np.zeros(1, np.uint8)
        offs = np.zeros(nb + 1, np.uint64)
        offs[1:] = np.cumsum([len(d) for d in datas])
        sv = None if share_versions is None else np.ascontiguousarray(share_versions, np.uint8)
        return [bytes(o) for o in self.blob_commitments_packed(ns, data, offs, sv, subtree_root_threshold)]

    def blob_commitments_packed(self, namespaces, data, offsets, share_versions=None, subtree_root_threshold=64):
        """cda_blob_commitments on pre-packed arrays: namespaces (n*29,) uint8, data uint8, offsets (n+1,) uint64."""
        nb = len(offsets) - 1
        out = np.empty((nb, 32), np.uint8)
        err = ErrInfo()
        rc = self._L.cda_blob_commitments(self._h, nb, _p(namespaces), _p(data), _p(offsets), _p(share_versions),
                                        subtree_root_threshold, _p(out), ctypes.byref(err))
        _check(rc, err, self)
        return out

    def merkle_roots(self, sets):
        """merkle.HashFromByteSlices of each list of 90-byte NMT nodes."""
        offs = np.zeros(len(sets) + 1, np.uint32)
        offs[1:] = np.cumsum([len(x) for x in sets])
        flat = b"".join(bytes(x) for st in sets for x in st)
        items = np.frombuffer(flat, np.uint8).copy() if flat else None
        out = np.empty((len(sets), 32), np.uint8)
        _check(self._L.cda_merkle_roots(self._h, len(sets), _p(offs), _p(items), NODE_SIZE, _p(out)), ctx=self)
        return [bytes(o) for o in out]

    def extend_commit_nodes(self, shares, want_eds=False, rows=True, cols=True, dah_tree=True):
        """extend_commit plus every node of the row / column NMTs and of the DAH tree."""
        shares = np.ascontiguousarray(shares, np.uint8)
        count, L = shares.shape
        w = 2 * max(1, int(round(count ** 0.5)))
        eds = np.empty((w * w, L), np.uint8) if want_eds else None
        rr, cr = np.empty((w, NODE_SIZE), np.uint8), np.empty((w, NODE_SIZE), np.uint8)
        dah = np.empty(32, np.uint8)
        rn = np.empty((w, 2 * w - 1, NODE_SIZE), np.uint8) if rows else None
        cn = np.empty((w, 2 * w - 1, NODE_SIZE), np.uint8) if cols else None
        dn = np.empty((4 * w - 1, 32), np.uint8) if dah_tree else None
        err = ErrInfo()
        rc = self._L.cda_extend_commit_nodes(self._h, count, L, _p(shares), _p(eds), _p(rr), _p(cr), _p(dah), _p(rn),
                                           _p(cn), _p(dn), ctypes.byref(err))
        _check(rc, err, self)
        return {"eds": eds, "row_roots": rr, "col_roots": cr, "dah": dah.tobytes(), "row_nodes": rn,
                "col_nodes": cn, "dah_nodes": dn}

    def share_inclusion_proof(self, shares, start, end):
        """pkg/proof NewShareInclusionProof for ODS shares [start, end) (raw proof parts)."""
        shares = np.ascontiguousarray(shares, np.uint8)
        count, L = shares.shape
        k = max(1, int(round(count ** 0.5)))
        lg = (2 * k).bit_length() - 1
        info = ShareProofInfo()
        rr, lh = np.empty((k, NODE_SIZE), np.uint8), np.empty((k, 32), np.uint8)
        au = np.empty((k, lg + 1, 32), np.uint8)
        ns, ne, nc = np.empty(k, np.int32), np.empty(k, np.int32), np.empty(k, np.int32)
        nodes = np.empty((k, 2 * lg, NODE_SIZE), np.uint8)
        root = np.empty(32, np.uint8)
        err = ErrInfo()
        rc = self._L.cda_share_inclusion_proof(self._h, count, L, _p(shares), start, end, ctypes.byref(info), _p(rr),
                                             _p(lh), _p(au), _p(ns), _p(ne), _p(nc), _p(nodes), _p(root),
                                             ctypes.byref(err))
        _check(rc, err, self)
        rows = [{"row_root": rr[i].tobytes(), "leaf_hash": lh[i].tobytes(),
                 "aunts": [au[i, j].tobytes() for j in range(info.naunts)], "start": int(ns[i]), "end": int(ne[i]),
                 "nodes": [nodes[i, j].tobytes() for j in range(nc[i])]} for i in range(info.nrows)]
        return {"start_row": info.start_row, "end_row": info.end_row, "total": info.total, "rows": rows,
                "data_root": root.tobytes()}

    # ---- sample proofs: a retained square that proves its cells, batched proof verification ----
    def open_square(self, shares):
        """cda_square_open: extend and commit `shares` once and keep the EDS and every tree node on the device.
        -> Square (row_roots, col_roots, dah as attributes); use as a context manager or call close()."""
        return Square(self, shares)

    def open_square_eds(self, eds):
        """cda_square_open_eds: retain the extended square `eds` ((2k)^2, 512) as it was committed -- nothing is
        extended and the encoding is not checked.  -> Square, as open_square."""
        return Square(self, eds, extended=True)

    def nmt_verify(self, descs, namespaces, roots, nodes, leaves):
        """cda_nmt_verify: nmt Proof.VerifyInclusion of a batch.  descs: NMT_PROOF_DESC_DTYPE rows; namespaces
        (nproofs, 29); roots (nroots, 90); nodes (nnodes, 90); leaves (nleaves, 512), all uint8.  -> verdicts (nproofs,)
        uint8, 1 = verifies."""
        descs = np.ascontiguousarray(descs, NMT_PROOF_DESC_DTYPE)
        n = len(descs)
        namespaces = np.ascontiguousarray(namespaces, np.uint8).reshape(n, NAMESPACE_SIZE)
        roots = np.ascontiguousarray(roots, np.uint8).reshape(-1, NODE_SIZE)
        nodes = np.ascontiguousarray(nodes, np.uint8).reshape(-1, NODE_SIZE)
        leaves = np.ascontiguousarray(leaves, np.uint8).reshape(-1, SHARE_SIZE)
        ok = np.zeros(n, np.uint8)
        rc = self._L.cda_nmt_verify(self._h, n, _p(descs), _p(namespaces), _p(roots) if len(roots) else None,
                                    len(roots), _p(nodes) if len(nodes) else None, len(nodes),
                                    _p(leaves) if len(leaves) else None, len(leaves), _p(ok))
        _check(rc, ctx=self)
        return ok

    def nmt_verify_device(self, nproofs, d_descs, d_namespaces, d_roots, nroots, d_nodes, nnodes, d_leaves, nleaves,
                          d_ok, stream=None):
        """cda_nmt_verify_device: the same with device addresses, asynchronous on `stream`."""
        rc = self._L.cda_nmt_verify_device(self._h, nproofs, ctypes.c_void_p(d_descs), ctypes.c_void_p(d_namespaces),
                                           ctypes.c_void_p(d_roots), nroots, ctypes.c_void_p(d_nodes), nnodes,
                                           ctypes.c_void_p(d_leaves), nleaves, ctypes.c_void_p(d_ok),
                                           ctypes.c_void_p(stream or 0))
        _check(rc, ctx=self)

    def share_proofs_validate(self, descs, rows, row_roots, leaf_hashes, nodes, aunts, leaves, data_roots):
        """cda_share_proofs_validate: ShareProof.Validate of a batch.  descs: SHARE_PROOF_DESC_DTYPE rows; rows:
        SHARE_ROW_DTYPE rows with row_roots (nrows, 90) and leaf_hashes (nrows, 32); nodes (n, 90); aunts (n, 32);
        leaves (n, 512); data_roots (n, 32), all uint8.  -> verdicts (nproofs,) int32, SP_* codes."""
        descs = np.ascontiguousarray(descs, SHARE_PROOF_DESC_DTYPE)
        rows = np.ascontiguousarray(rows, SHARE_ROW_DTYPE)
        nrows = len(rows)
        row_roots = np.ascontiguousarray(row_roots, np.uint8).reshape(nrows, NODE_SIZE)
        leaf_hashes = np.ascontiguousarray(leaf_hashes, np.uint8).reshape(nrows, 32)
        nodes = np.ascontiguousarray(nodes, np.uint8).reshape(-1, NODE_SIZE)
        aunts = np.ascontiguousarray(aunts, np.uint8).reshape(-1, 32)
        leaves = np.ascontiguousarray(leaves, np.uint8).reshape(-1, SHARE_SIZE)
        data_roots = np.ascontiguousarray(data_roots, np.uint8).reshape(-1, 32)
        verdicts = np.full(len(descs), -1, np.int32)

        def p(a):
            return _p(a) if len(a) else None
        rc = self._L.cda_share_proofs_validate(self._h, len(descs), p(descs), p(rows), p(row_roots), p(leaf_hashes),
                                               nrows, p(nodes), len(nodes), p(aunts), len(aunts), p(leaves),
                                               len(leaves), p(data_roots), len(data_roots), _p(verdicts))
        _check(rc, ctx=self)
        return verdicts

    def share_proofs_validate_device(self, nproofs, d_descs, d_rows, d_row_roots, d_leaf_hashes, nrows, d_nodes, nnodes,
                                     d_aunts, naunts, d_leaves, nleaves, d_data_roots, nroots, d_verdicts, stream=None):
        """cda_share_proofs_validate_device: the same with device addresses, asynchronous on `stream`."""
        V = ctypes.c_void_p
        rc = self._L.cda_share_proofs_validate_device(self._h, nproofs, V(d_descs), V(d_rows), V(d_row_roots),
                                                      V(d_leaf_hashes), nrows, V(d_nodes), nnodes, V(d_aunts), naunts,
                                                      V(d_leaves), nleaves, V(d_data_roots), nroots, V(d_verdicts),
                                                      V(stream or 0))
        _check(rc, ctx=self)

    def commitment_proofs_verify(self, descs, rows, row_roots, leaf_hashes, nodes, subtree_roots, aunts, data_roots,
                                 commitments):
        """cda_commitment_proofs_verify: rules C0-C8 of a batch.  descs: COMMITMENT_PROOF_DESC_DTYPE rows; rows:
        COMMITMENT_ROW_DTYPE rows with row_roots (nrows, 90) and leaf_hashes (nrows, 32); nodes and subtree_roots
        (n, 90); aunts, data_roots and commitments (n, 32), all uint8.  -> verdicts (nproofs,) int32, CP_* codes."""
        descs = np.ascontiguousarray(descs, COMMITMENT_PROOF_DESC_DTYPE)
        rows = np.ascontiguousarray(rows, COMMITMENT_ROW_DTYPE)
        nrows = len(rows)
        row_roots = np.ascontiguousarray(row_roots, np.uint8).reshape(nrows, NODE_SIZE)
        leaf_hashes = np.ascontiguousarray(leaf_hashes, np.uint8).reshape(nrows, 32)
        nodes = np.ascontiguousarray(nodes, np.uint8).reshape(-1, NODE_SIZE)
        subtree_roots = np.ascontiguousarray(subtree_roots, np.uint8).reshape(-1, NODE_SIZE)
        aunts = np.ascontiguousarray(aunts, np.uint8).reshape(-1, 32)
        data_roots = np.ascontiguousarray(data_roots, np.uint8).reshape(-1, 32)
        commitments = np.ascontiguousarray(commitments, np.uint8).reshape(-1, 32)
        verdicts = np.full(len(descs), -1, np.int32)

        def p(a):
            return _p(a) if len(a) else None
        rc = self._L.cda_commitment_proofs_verify(self._h, len(descs), p(descs), p(rows), p(row_roots), p(leaf_hashes),
                                                  nrows, p(nodes), len(nodes), p(subtree_roots), len(subtree_roots),
                                                  p(aunts), len(aunts), p(data_roots), len(data_roots), p(commitments),
                                                  len(commitments), _p(verdicts))
        _check(rc, ctx=self)
        return verdicts

    def commitment_proofs_verify_device(self, nproofs, d_descs, d_rows, d_row_roots, d_leaf_hashes, nrows, d_nodes,
                                        nnodes, d_subtree_roots, nsubtree_roots, d_aunts, naunts, d_data_roots, nroots,
                                        d_commitments, ncommitments, d_verdicts, stream=None):
        """cda_commitment_proofs_verify_device: the same with device addresses, asynchronous on `stream`."""
        V = ctypes.c_void_p
        rc = self._L.cda_commitment_proofs_verify_device(self._h, nproofs, V(d_descs), V(d_rows), V(d_row_roots),
                                                         V(d_leaf_hashes), nrows, V(d_nodes), nnodes,
                                                         V(d_subtree_roots), nsubtree_roots, V(d_aunts), naunts,
                                                         V(d_data_roots), nroots, V(d_commitments), ncommitments,
                                                         V(d_verdicts), V(stream or 0))
        _check(rc, ctx=self)

    def nmt_verify_namespace(self, descs, namespaces, roots, nodes, leaf_hashes, leaves):
        """cda_nmt_verify_namespace: nmt Proof.VerifyNamespace of a batch.  descs: NMT_NS_PROOF_DESC_DTYPE rows;
        namespaces (nproofs, 29); roots (nroots, 90); nodes (nnodes, 90); leaf_hashes (n, 90); leaves (nleaves, 512), all
        uint8.  -> verdicts (nproofs,) uint8, 1 = verifies."""
        descs = np.ascontiguousarray(descs, NMT_NS_PROOF_DESC_DTYPE)
        n = len(descs)
        namespaces = np.ascontiguousarray(namespaces, np.uint8).reshape(n, NAMESPACE_SIZE)
        roots = np.ascontiguousarray(roots, np.uint8).reshape(-1, NODE_SIZE)
        nodes = np.ascontiguousarray(nodes, np.uint8).reshape(-1, NODE_SIZE)
        leaf_hashes = np.ascontiguousarray(leaf_hashes, np.uint8).reshape(-1, NODE_SIZE)
        leaves = np.ascontiguousarray(leaves, np.uint8).reshape(-1, SHARE_SIZE)
        ok = np.zeros(n, np.uint8)

        def p(a):
            return _p(a) if len(a) else None
        rc = self._L.cda_nmt_verify_namespace(self._h, n, _p(descs), _p(namespaces), p(roots), len(roots), p(nodes),
                                              len(nodes), p(leaf_hashes), len(leaf_hashes), p(leaves), len(leaves),
                                              _p(ok))
        _check(rc, ctx=self)
        return ok

    def nmt_verify_namespace_device(self, nproofs, d_descs, d_namespaces, d_roots, nroots, d_nodes, nnodes,
                                    d_leaf_hashes, nleaf_hashes, d_leaves, nleaves, d_ok, stream=None):
        """cda_nmt_verify_namespace_device: the same with device addresses, asynchronous on `stream`."""
        V = ctypes.c_void_p
        rc = self._L.cda_nmt_verify_namespace_device(self._h, nproofs, V(d_descs), V(d_namespaces), V(d_roots), nroots,
                                                     V(d_nodes), nnodes, V(d_leaf_hashes), nleaf_hashes, V(d_leaves),
                                                     nleaves, V(d_ok), V(stream or 0))
        _check(rc, ctx=self)

    def befp_validate(self, k, descs, entries, shares, nodes, roots):
        """cda_befp_validate: Validate of a batch of bad-encoding fraud proofs of 2k x 2k squares.  descs:
        BEFP_DESC_DTYPE rows; entries: BEFP_ENTRY_DTYPE rows with shares (nentries, 512); nodes (n, 90); roots (n, 90),
        per block the 2k row roots then the 2k column roots, all uint8.  -> verdicts (nproofs,) int32, BEFP_* codes."""
        descs = np.ascontiguousarray(descs, BEFP_DESC_DTYPE)
        entries = np.ascontiguousarray(entries, BEFP_ENTRY_DTYPE)
        shares = np.ascontiguousarray(shares, np.uint8).reshape(len(entries), SHARE_SIZE)
        nodes = np.ascontiguousarray(nodes, np.uint8).reshape(-1, NODE_SIZE)
        roots = np.ascontiguousarray(roots, np.uint8).reshape(-1, NODE_SIZE)
        verdicts = np.full(len(descs), BEFP_MALFORMED, np.int32)

        def p(a):
            return _p(a) if len(a) else None
        rc = self._L.cda_befp_validate(self._h, k, len(descs), p(descs), p(entries), len(entries), p(shares), p(nodes),
                                       len(nodes), p(roots), len(roots), _p(verdicts))
        _check(rc, ctx=self)
        return verdicts

    def befp_validate_device(self, k, nproofs, d_descs, d_entries, nentries, d_shares, d_nodes, nnodes, d_roots, nroots,
                             d_verdicts, stream=None):
        """cda_befp_validate_device: the same with device addresses, asynchronous on `stream`."""
        V = ctypes.c_void_p
        rc = self._L.cda_befp_validate_device(self._h, k, nproofs, V(d_descs), V(d_entries), nentries, V(d_shares),
                                              V(d_nodes), nnodes, V(d_roots), nroots, V(d_verdicts), V(stream or 0))
        _check(rc, ctx=self)

    # ---- a square rebuilt from proved samples ----
    def samples_assemble_device(self, k, nsamples, d_descs, d_shares, d_nodes, nnodes, d_roots, d_eds, d_present,
                                d_statuses, stream=None):
        """cda_samples_assemble_device: verify the samples and place the accepted cells, every argument a device
        address, asynchronous on `stream`.  d_eds ((2k)^2 x 512 B), d_present ((2k)^2) and d_statuses (nsamples,
        SAMPLE_* codes) are the outputs."""
        V = ctypes.c_void_p
        rc = self._L.cda_samples_assemble_device(self._h, k, nsamples, V(d_descs), V(d_shares), V(d_nodes), nnodes,
                                                 V(d_roots), V(d_eds), V(d_present), V(d_statuses), V(stream or 0))
        _check(rc, ctx=self)

    def open_square_eds_device(self, k, d_eds, stream=None):
        """cda_square_open_eds_device: retain the extended square at device address d_eds ((2k)^2 x 512 B) as
        open_square_eds retains one from host memory.  -> Square."""
        w = 2 * k
        row_roots, col_roots = np.empty((w, NODE_SIZE), np.uint8), np.empty((w, NODE_SIZE), np.uint8)
        dah = np.empty(32, np.uint8)
        h, err = ctypes.c_void_p(), ErrInfo()
        rc = self._L.cda_square_open_eds_device(self._h, k, ctypes.c_void_p(d_eds), ctypes.byref(h), _p(row_roots),
                                                _p(col_roots), _p(dah), ctypes.byref(err),
                                                ctypes.c_void_p(stream or 0))
        _check(rc, err, self)
        return Square._adopt(self, k, h, row_roots, col_roots, dah)

    def rebuild_square_status(self, descs, shares, nodes, row_roots, col_roots, want_eds=False):
        """cda_square_rebuild without raising on the two repair errors: (rc, square or None, statuses, present, eds or
        None, err).  On CDA_E_UNREPAIRABLE / CDA_E_BYZANTINE present and eds hold the square where rsmt2d stops."""
        descs = np.ascontiguousarray(descs, SAMPLE_DESC_DTYPE)
        n = len(descs)
        shares = np.ascontiguousarray(shares, np.uint8).reshape(n, SHARE_SIZE)
        nodes = np.ascontiguousarray(nodes, np.uint8).reshape(-1, NODE_SIZE)
        row_roots = np.ascontiguousarray(row_roots, np.uint8).reshape(-1, NODE_SIZE)
        col_roots = np.ascontiguousarray(col_roots, np.uint8).reshape(-1, NODE_SIZE)
        w = len(row_roots)
        if len(col_roots) != w or w % 2:
            raise CdaError(E_ARG, "the roots are 2k row roots and 2k column roots")
        statuses = np.full(n, SAMPLE_MALFORMED, np.uint8)
        present = np.zeros(w * w, np.uint8)
        eds = np.zeros((w * w, SHARE_SIZE), np.uint8) if want_eds else None
        dah = np.empty(32, np.uint8)
        h, err = ctypes.c_void_p(), ErrInfo()

        def p(a):
            return _p(a) if len(a) else None
        rc = self._L.cda_square_rebuild(self._h, w // 2, n, p(descs), p(shares), p(nodes), len(nodes), _p(row_roots),
                                        _p(col_roots), ctypes.byref(h), p(statuses), _p(present), _p(eds), _p(dah),
                                        ctypes.byref(err))
        if rc not in (OK, E_UNREPAIRABLE, E_BYZANTINE):
            _check(rc, err, self)
        sq = Square._adopt(self, w // 2, h, row_roots.copy(), col_roots.copy(), dah) if rc == OK else None
        return rc, sq, statuses, present, eds, err

    def rebuild_square(self, descs, shares, nodes, row_roots, col_roots):
        """cda_square_rebuild: the samples (SAMPLE_DESC_DTYPE rows, shares (n, 512), nodes (m, 90)) verified, placed,
        repaired against the roots and retained.  -> Square; CdaError (axis, index) when rsmt2d's Repair fails."""
        rc, sq, _, _, _, err = self.rebuild_square_status(descs, shares, nodes, row_roots, col_roots)
        _check(rc, err, self)
        return sq

    # ---- halves of rows and columns ----
    def axis_halves_verify(self, k, descs, shares, roots, want_axes=False):
        """cda_axis_halves_verify: batched Row.Verify of halves of 2k x 2k squares.  descs: AXIS_HALF_DESC_DTYPE rows;
        shares (nhalves, k, 512); roots (n, 90), per block the 2k row roots then the 2k column roots, all uint8.
        -> statuses (nhalves,) uint8, HALF_* codes[, axes (nhalves, 2k, 512)]."""
        descs = np.ascontiguousarray(descs, AXIS_HALF_DESC_DTYPE)
        n = len(descs)
        shares = np.ascontiguousarray(shares, np.uint8).reshape(n, k, SHARE_SIZE)
        roots = np.ascontiguousarray(roots, np.uint8).reshape(-1, NODE_SIZE)
        statuses = np.full(n, HALF_MALFORMED, np.uint8)
        axes = np.zeros((n, 2 * k, SHARE_SIZE), np.uint8) if want_axes else None

        def p(a):
            return _p(a) if a is not None and len(a) else None
        rc = self._L.cda_axis_halves_verify(self._h, k, n, p(descs), p(shares), p(roots), len(roots), p(statuses),
                                            p(axes))
        _check(rc, ctx=self)
        return (statuses, axes) if want_axes else statuses

    def axis_halves_verify_device(self, k, nhalves, d_descs, d_shares, d_roots, nroots, d_statuses, d_axes=0,
                                  stream=None):
        """cda_axis_halves_verify_device: the same with device addresses, asynchronous on `stream`."""
        V = ctypes.c_void_p
        rc = self._L.cda_axis_halves_verify_device(self._h, k, nhalves, V(d_descs), V(d_shares), V(d_roots), nroots,
                                                   V(d_statuses), V(d_axes or None), V(stream or 0))
        _check(rc, ctx=self)

    def axis_halves_assemble_device(self, k, nhalves, d_descs, d_shares, d_roots, d_eds, d_present, d_statuses,
                                    stream=None):
        """cda_axis_halves_assemble_device: verify the halves of one square and place the completed axes, every
        argument a device address, asynchronous on `stream`.  d_eds ((2k)^2 x 512 B), d_present ((2k)^2) and
        d_statuses (nhalves, HALF_* codes) are the outputs."""
        V = ctypes.c_void_p
        rc = self._L.cda_axis_halves_assemble_device(self._h, k, nhalves, V(d_descs), V(d_shares), V(d_roots),
                                                     V(d_eds), V(d_present), V(d_statuses), V(stream or 0))
        _check(rc, ctx=self)

    def square_rebuild_axes(self, descs, shares, row_roots, col_roots, want_eds=False):
        """cda_square_rebuild_axes without raising on the two repair errors: (rc, square or None, statuses, present,
        eds or None, err).  On CDA_E_UNREPAIRABLE / CDA_E_BYZANTINE present and eds hold the square where rsmt2d
        stops."""
        descs = np.ascontiguousarray(descs, AXIS_HALF_DESC_DTYPE)
        n = len(descs)
        row_roots = np.ascontiguousarray(row_roots, np.uint8).reshape(-1, NODE_SIZE)
        col_roots = np.ascontiguousarray(col_roots, np.uint8).reshape(-1, NODE_SIZE)
        w = len(row_roots)
        if len(col_roots) != w or w % 2:
            raise CdaError(E_ARG, "the roots are 2k row roots and 2k column roots")
        shares = np.ascontiguousarray(shares, np.uint8).reshape(n, w // 2, SHARE_SIZE)
        statuses = np.full(n, HALF_MALFORMED, np.uint8)
        present = np.zeros(w * w, np.uint8)
        eds = np.zeros((w * w, SHARE_SIZE), np.uint8) if want_eds else None
        dah = np.empty(32, np.uint8)
        h, err = ctypes.c_void_p(), ErrInfo()

        def p(a):
            return _p(a) if len(a) else None
        rc = self._L.cda_square_rebuild_axes(self._h, w // 2, n, p(descs), p(shares), _p(row_roots), _p(col_roots),
                                             ctypes.byref(h), p(statuses), _p(present), _p(eds), _p(dah),
                                             ctypes.byref(err))
        if rc not in (OK, E_UNREPAIRABLE, E_BYZANTINE):
            _check(rc, err, self)
        sq = Square._adopt(self, w // 2, h, row_roots.copy(), col_roots.copy(), dah) if rc == OK else None
        return rc, sq, statuses, present, eds, err

    # ---- profiling ----
    def profile_enable(self, on=True):
        _check(self._L.cda_profile_enable(self._h, 1 if on else 0), ctx=self)

    def profile_reset(self):
        _check(self._L.cda_profile_reset(self._h), ctx=self)

    def profile_read(self):
        cap = 64
        names = ctypes.create_string_buffer(4096)
        ms = np.zeros(cap, np.float64)
        cnt = np.zeros(cap, np.int64)
        n = self._L.cda_profile_read(self._h, names, 4096, _p(ms), _p(cnt), cap)
        out, parts = {}, names.raw.split(b"\0")
        for i in range(n):
            out[parts[i].decode()] = (float(ms[i]), int(cnt[i]))
        return out


class Square:
    """cda_square: one extended block retained on the device (Context.open_square: the k x k shares are extended;
    Context.open_square_eds: `shares` is the (2k)^2 extended square, retained as given)."""

    def __init__(self, ctx, shares, extended=False):
        shares = np.ascontiguousarray(shares, np.uint8)
        count, L = shares.shape
        self.k = max(1, int(round(count ** 0.5)))
        if extended:
            self.k //= 2
            if L != SHARE_SIZE or count != 4 * self.k * self.k or self.k == 0:
                raise ValueError("open_square_eds takes the (2k)^2 cells of an extended square, 512 bytes each")
        w = 2 * self.k
        self.row_roots = np.empty((w, NODE_SIZE), np.uint8)
        self.col_roots = np.empty((w, NODE_SIZE), np.uint8)
        dah = np.empty(32, np.uint8)
        self._ctx, self._h = ctx, None
        h = ctypes.c_void_p()
        err = ErrInfo()
        if extended:
            rc = ctx._L.cda_square_open_eds(ctx._h, self.k, _p(shares), ctypes.byref(h), _p(self.row_roots),
                                            _p(self.col_roots), _p(dah), ctypes.byref(err))
        else:
            rc = ctx._L.cda_square_open(ctx._h, count, L, _p(shares), ctypes.byref(h), _p(self.row_roots),
                                        _p(self.col_roots), _p(dah), ctypes.byref(err))
        _check(rc, err, ctx)
        self._h = h
        self.dah = dah.tobytes()
        self.max_nodes = 2 * (w.bit_length() - 1)

    @classmethod
    def _adopt(cls, ctx, k, handle, row_roots, col_roots, dah):
        """The Square of a handle the library has already built (open_square_eds_device, rebuild_square)."""
        self = object.__new__(cls)
        self._ctx, self._h, self.k = ctx, handle, k
        self.row_roots, self.col_roots, self.dah = row_roots, col_roots, dah.tobytes()
        self.max_nodes = 2 * ((2 * k).bit_length() - 1)
        return self

    def prove(self, queries, want_shares=True):
        """cda_square_prove.  queries: (axis, index, start, end) tuples or RANGE_QUERY_DTYPE rows.
        -> (counts (nq,) int32, nodes (nq, max_nodes, 90) uint8, shares (sum(end - start), 512) uint8 or None): query
        q's proof is nodes[q, :counts[q]], its cells follow those of the queries before it."""
        q = queries if isinstance(queries, np.ndarray) and queries.dtype == RANGE_QUERY_DTYPE else \
            np.array([tuple(x) for x in queries], RANGE_QUERY_DTYPE)
        q = np.ascontiguousarray(q)
        nq = len(q)
        mn = max(1, self.max_nodes)
        counts = np.zeros(nq, np.int32)
        nodes = np.zeros((nq, mn, NODE_SIZE), np.uint8)
        ncells = int((q["end"].astype(np.int64) - q["start"].astype(np.int64)).clip(min=0).sum())
        shares = np.zeros((ncells, SHARE_SIZE), np.uint8) if want_shares else None
        rc = self._ctx._L.cda_square_prove(self._h, nq, _p(q), mn, _p(counts), _p(nodes), _p(shares),
                                           shares.nbytes if want_shares else 0)
        _check(rc, ctx=self._ctx)
        return counts, nodes, shares

    def prove_device(self, queries, max_nodes, d_counts, d_nodes, d_shares=0, shares_cap=0):
        """cda_square_prove with the outputs at device addresses (queries stay host records)."""
        q = np.ascontiguousarray(queries, RANGE_QUERY_DTYPE)
        rc = self._ctx._L.cda_square_prove(self._h, len(q), _p(q), max_nodes, ctypes.c_void_p(d_counts),
                                           ctypes.c_void_p(d_nodes), ctypes.c_void_p(d_shares or None), shares_cap)
        _check(rc, ctx=self._ctx)

    def axis_halves(self, queries, d_shares=0, shares_cap=0):
        """cda_square_axis_halves.  queries: (axis, index, side) tuples or AXIS_HALF_DESC_DTYPE rows.
        -> shares (nq, k, 512) uint8, query q's k cells in cell order; with d_shares (a device address of shares_cap
        bytes) the halves are written there instead and nothing is returned."""
        q = queries if isinstance(queries, np.ndarray) and queries.dtype == AXIS_HALF_DESC_DTYPE else \
            np.array([tuple(x)[:3] + (0,) for x in queries], AXIS_HALF_DESC_DTYPE)
        q = np.ascontiguousarray(q)
        if d_shares:
            rc = self._ctx._L.cda_square_axis_halves(self._h, len(q), _p(q), ctypes.c_void_p(d_shares), shares_cap)
            _check(rc, ctx=self._ctx)
            return None
        shares = np.zeros((len(q), self.k, SHARE_SIZE), np.uint8)
        rc = self._ctx._L.cda_square_axis_halves(self._h, len(q), _p(q), _p(shares), shares.nbytes)
        _check(rc, ctx=self._ctx)
        return shares

    @staticmethod
    def share_proof_sizes(k, ranges):
        """(row records, shares) the proofs of `ranges` ((start, end) ODS share ranges) of a k x k square take."""
        nrows = sum((int(e) - 1) // k - int(s) // k + 1 for s, e in ranges)
        return nrows, sum(int(e) - int(s) for s, e in ranges)

    def share_proofs_raw(self, ranges, want_shares=True):
        """cda_square_share_proofs: pkg/proof NewShareInclusionProof of every (start, end) ODS share range, one
        launch.  -> dict of the flat arrays the call writes: row_off (nq + 1,), rows (SHARE_ROW_DTYPE), nodes
        (nrows, max_nodes, 90), row_roots (nrows, 90), leaf_hashes (nrows, 32), aunts (nrows, log2(4k), 32), shares
        (n, 512) or None, data_root bytes.  Query q's records are rows[row_off[q]:row_off[q + 1]]."""
        q = np.array([(int(s), int(e)) for s, e in ranges], SHARE_RANGE_DTYPE).reshape(-1)
        nq, mn, na = len(q), max(1, self.max_nodes), (4 * self.k).bit_length() - 1
        # sized on the host from ranges that may be bad: the library checks them (clip keeps the sizes sane)
        nrows, nshares = self.share_proof_sizes(self.k, [(s, max(s + 1, min(e, self.k * self.k))) for s, e in
                                                         ((int(x["start"]), int(x["end"])) for x in q)])
        out = {"row_off": np.zeros(nq + 1, np.uint32), "rows": np.zeros(nrows, SHARE_ROW_DTYPE),
               "nodes": np.zeros((nrows, mn, NODE_SIZE), np.uint8), "row_roots": np.zeros((nrows, NODE_SIZE), np.uint8),
               "leaf_hashes": np.zeros((nrows, 32), np.uint8), "aunts": np.zeros((nrows, na, 32), np.uint8),
               "shares": np.zeros((nshares, SHARE_SIZE), np.uint8) if want_shares else None}
        root = np.zeros(32, np.uint8)
        rc = self._ctx._L.cda_square_share_proofs(self._h, nq, _p(q), mn, nrows, _p(out["row_off"]), _p(out["rows"]),
                                                  _p(out["nodes"]), _p(out["row_roots"]), _p(out["leaf_hashes"]),
                                                  _p(out["aunts"]), _p(out["shares"]) if want_shares else None,
                                                  out["shares"].nbytes if want_shares else 0, _p(root))
        _check(rc, ctx=self._ctx)
        out["data_root"] = root.tobytes()
        return out

    def share_proofs_device(self, ranges, max_nodes, rows_cap, d_row_off, d_rows, d_nodes, d_row_roots, d_leaf_hashes,
                            d_aunts, d_shares, shares_cap, d_data_root):
        """cda_square_share_proofs with the outputs at device addresses (the ranges stay host records)."""
        q = np.array([(int(s), int(e)) for s, e in ranges], SHARE_RANGE_DTYPE).reshape(-1)
        V = ctypes.c_void_p
        rc = self._ctx._L.cda_square_share_proofs(self._h, len(q), _p(q), max_nodes, rows_cap, V(d_row_off), V(d_rows),
                                                  V(d_nodes), V(d_row_roots), V(d_leaf_hashes), V(d_aunts),
                                                  V(d_shares or None), shares_cap, V(d_data_root))
        _check(rc, ctx=self._ctx)

    def share_proofs(self, ranges, namespaces=None):
        """pkg/proof NewShareInclusionProof for every (start, end) ODS share range, one launch -> list of
        cda.proof.ShareProof.  namespaces: the 29-byte namespace of each range (ParseNamespace's result); default:
        the namespace of the range's first share."""
        from . import proof as P
        ranges = [(int(s), int(e)) for s, e in ranges]
        raw = self.share_proofs_raw(ranges)
        rows, out, cursor = raw["rows"], [], 0
        for i, (s, e) in enumerate(ranges):
            lo, hi = int(raw["row_off"][i]), int(raw["row_off"][i + 1])
            data = [raw["shares"][cursor + j].tobytes() for j in range(e - s)]
            cursor += e - s
            ns = bytes(namespaces[i]) if namespaces is not None else data[0][:NAMESPACE_SIZE]
            nmt = [P.NMTProof(int(rows[r]["nmt_start"]), int(rows[r]["nmt_end"]),
                              [raw["nodes"][r, j].tobytes() for j in range(int(rows[r]["nnodes"]))])
                   for r in range(lo, hi)]
            row_proof = P.RowProof([raw["row_roots"][r].tobytes() for r in range(lo, hi)],
                                   [P.Proof(int(rows[r]["total"]), int(rows[r]["index"]),
                                            raw["leaf_hashes"][r].tobytes(),
                                            [raw["aunts"][r, j].tobytes() for j in range(int(rows[r]["naunts"]))])
                                    for r in range(lo, hi)], int(rows[lo]["row"]), int(rows[hi - 1]["row"]))
            out.append(P.ShareProof(data, nmt, ns[1:], row_proof, ns[0], raw["data_root"]))
        return out

    @staticmethod
    def blob_ranges(ranges):
        """(start, len) tuples -> BLOB_RANGE_DTYPE rows."""
        return np.array([(int(s), int(n)) for s, n in ranges], BLOB_RANGE_DTYPE).reshape(-1)

    def commitment_proof_sizes(self, ranges, threshold=64):
        """cda_commitment_proof_sizes: (row records, subtree roots) the commitment proofs of `ranges` ((start, len) ODS
        share ranges) take under `threshold`; CdaError(E_ARG) for a range the prover rejects."""
        q = self.blob_ranges(ranges)
        nrows, nroots = ctypes.c_uint64(), ctypes.c_uint64()
        _check(self._ctx._L.cda_commitment_proof_sizes(self.k, threshold, len(q), _p(q), ctypes.byref(nrows),
                                                       ctypes.byref(nroots)))
        return nrows.value, nroots.value

    def commitments(self, ranges, threshold=64):
        """GetCommitment (pkg/inclusion/get_commit.go) of every (start, len) blob of the retained square in one call:
        cda_square_commitment_proofs with the commitments alone -> list of 32-byte commitments."""
        q = self.blob_ranges(ranges)
        out = np.zeros((len(q), 32), np.uint8)
        rc = self._ctx._L.cda_square_commitment_proofs(self._h, len(q), _p(q), threshold, 0, 0, 0, None, None, None, None,
                                                       None, None, None, _p(out), None)
        _check(rc, ctx=self._ctx)
        return [x.tobytes() for x in out]

    def commitment_proofs_raw(self, ranges, threshold=64, rows_cap=None, roots_cap=None):
        """cda_square_commitment_proofs -> dict of the flat arrays the call writes: row_off (nq + 1,), rows
        (COMMITMENT_ROW_DTYPE), nodes (nrows, max_nodes, 90), subtree_roots (nroots, 90), row_roots (nrows, 90),
        leaf_hashes (nrows, 32), aunts (nrows, log2(4k), 32), commitments (nq, 32), data_root bytes.  Blob q's records
        are rows[row_off[q]:row_off[q + 1]].  rows_cap / roots_cap: the capacities handed to the call (default: what
        cda_commitment_proof_sizes says)."""
        q = self.blob_ranges(ranges)
        nq, mn, na = len(q), max(1, self.max_nodes), (4 * self.k).bit_length() - 1
        nrows, nroots = self.commitment_proof_sizes(ranges, threshold)
        nrows = nrows if rows_cap is None else rows_cap
        nroots = nroots if roots_cap is None else roots_cap
        out = {"row_off": np.zeros(nq + 1, np.uint32), "rows": np.zeros(nrows, COMMITMENT_ROW_DTYPE),
               "nodes": np.zeros((nrows, mn, NODE_SIZE), np.uint8), "subtree_roots": np.zeros((nroots, NODE_SIZE), np.uint8),
               "row_roots": np.zeros((nrows, NODE_SIZE), np.uint8), "leaf_hashes": np.zeros((nrows, 32), np.uint8),
               "aunts": np.zeros((nrows, na, 32), np.uint8), "commitments": np.zeros((nq, 32), np.uint8)}
        root = np.zeros(32, np.uint8)
        rc = self._ctx._L.cda_square_commitment_proofs(self._h, nq, _p(q), threshold, mn, nrows, nroots,
                                                       _p(out["row_off"]), _p(out["rows"]), _p(out["nodes"]),
                                                       _p(out["subtree_roots"]), _p(out["row_roots"]),
                                                       _p(out["leaf_hashes"]), _p(out["aunts"]), _p(out["commitments"]),
                                                       _p(root))
        _check(rc, ctx=self._ctx)
        out["data_root"] = root.tobytes()
        return out

    def commitment_proofs_device(self, ranges, threshold, max_nodes, rows_cap, roots_cap, d_row_off, d_rows, d_nodes,
                                 d_subtree_roots, d_row_roots, d_leaf_hashes, d_aunts, d_commitments, d_data_root):
        """cda_square_commitment_proofs with the outputs at device addresses (the ranges stay host records)."""
        q = self.blob_ranges(ranges)
        V = ctypes.c_void_p
        rc = self._ctx._L.cda_square_commitment_proofs(self._h, len(q), _p(q), threshold, max_nodes, rows_cap, roots_cap,
                                                       V(d_row_off), V(d_rows), V(d_nodes), V(d_subtree_roots),
                                                       V(d_row_roots), V(d_leaf_hashes), V(d_aunts), V(d_commitments),
                                                       V(d_data_root))
        _check(rc, ctx=self._ctx)

    def commitment_proofs(self, ranges, namespaces, threshold=64):
        """ADR-011's blob inclusion proof for every (start, len) blob of the retained square, one call -> list of
        cda.commitment.CommitmentProof; namespaces: the 29-byte namespace of each blob."""
        from . import commitment as C
        return C.proofs_from_raw(self.commitment_proofs_raw(ranges, threshold), namespaces)

    def index(self, threshold=64, commitments=True, cap=None):
        """cda_square_index: every sequence of the square (the two compact ones and the blobs) in ascending order
        -> (SEQUENCE_DTYPE rows, (nseq, 32) uint8 share commitments or None, summary dict).  A blob whose status is
        not 0 has a commitment of zeros.  cap: records offered at first; if the square has more, one more call."""
        cap = 256 if cap is None else int(cap)
        while True:
            seqs = np.zeros(cap, SEQUENCE_DTYPE)
            com = np.zeros((cap, 32), np.uint8) if commitments else None
            summary = SquareSummary()
            rc = self._ctx._L.cda_square_index(self._h, threshold, cap, _p(seqs), _p(com), ctypes.byref(summary))
            _check(rc, ctx=self._ctx)
            if summary.nseq <= cap:
                break
            cap = summary.nseq
        n = summary.nseq
        info = {name: int(getattr(summary, name)) for name, _ in SquareSummary._fields_}
        return seqs[:n], (com[:n] if commitments else None), info

    @staticmethod
    def sequence_ranges(seqs):
        """SEQUENCE_DTYPE rows, or (start, nshares, seq_len, compact) tuples -> SEQUENCE_RANGE_DTYPE rows."""
        if isinstance(seqs, np.ndarray) and seqs.dtype == SEQUENCE_RANGE_DTYPE:
            return np.ascontiguousarray(seqs)
        if isinstance(seqs, np.ndarray) and seqs.dtype == SEQUENCE_DTYPE:
            q = np.zeros(len(seqs), SEQUENCE_RANGE_DTYPE)
            for name in ("start", "nshares", "seq_len"):
                q[name] = seqs[name]
            q["compact"] = seqs["kind"] != SEQ_KIND_BLOB
            return q
        return np.array([tuple(int(v) for v in x) for x in seqs], SEQUENCE_RANGE_DTYPE).reshape(-1)

    def read(self, seqs):
        """cda_square_read: the payload of every sequence, share headers stripped -> list of bytes."""
        q = self.sequence_ranges(seqs)
        lens = q["seq_len"].astype(np.uint64)
        off = np.zeros(len(q) + 1, np.uint64)
        np.cumsum(lens, out=off[1:])
        data = np.zeros(max(1, int(off[-1])), np.uint8)
        rc = self._ctx._L.cda_square_read(self._h, len(q), _p(q), _p(off), int(off[-1]), _p(data))
        _check(rc, ctx=self._ctx)
        return [data[int(off[i]):int(off[i + 1])].tobytes() for i in range(len(q))]

    def read_device(self, seqs, data_off, data_cap, d_data):
        """cda_square_read with the payloads at the device address d_data: query q at [data_off[q], + seq_len)."""
        q = self.sequence_ranges(seqs)
        off = np.ascontiguousarray(data_off, np.uint64)
        if len(off) < len(q):
            raise ValueError("one offset per sequence")
        rc = self._ctx._L.cda_square_read(self._h, len(q), _p(q), _p(off), int(data_cap), ctypes.c_void_p(d_data))
        _check(rc, ctx=self._ctx)

    @staticmethod
    def namespace_queries(queries):
        """(axis, index, namespace) tuples -> NAMESPACE_QUERY_DTYPE rows (rows of that dtype pass through)."""
        if isinstance(queries, np.ndarray) and queries.dtype == NAMESPACE_QUERY_DTYPE:
            return np.ascontiguousarray(queries)
        q = np.zeros(len(queries), NAMESPACE_QUERY_DTYPE)
        for i, (axis, index, ns) in enumerate(queries):
            ns = bytes(ns)
            if len(ns) != NAMESPACE_SIZE:
                raise ValueError(f"namespace of {len(ns)} bytes: cda_square_prove_namespace takes {NAMESPACE_SIZE}")
            q[i] = (axis, index, np.frombuffer(ns, np.uint8), 0)
        return q

    def prove_namespace(self, queries, want_shares=True, shares_cap=None):
        """cda_square_prove_namespace: nmt ProveNamespace of many (axis, index, namespace) queries, one call.
        -> (results (nq,) NAMESPACE_RESULT_DTYPE, nodes (nq, max_nodes, 90), leaf_hashes (nq, 90), shares (n, 512) or
        None): query q's proof is nodes[q, :results[q]["nnodes"]], its shares are
        shares[share_off : share_off + nshares].  shares_cap: bytes of the share buffer to offer (default: the bound
        nq * 2k * 512 that always suffices, trimmed to the total afterwards)."""
        q = self.namespace_queries(queries)
        nq, mn, w = len(q), max(1, self.max_nodes), 2 * self.k
        results = np.zeros(nq, NAMESPACE_RESULT_DTYPE)
        nodes = np.zeros((nq, mn, NODE_SIZE), np.uint8)
        leaf_hashes = np.zeros((nq, NODE_SIZE), np.uint8)
        cap = nq * w * SHARE_SIZE if shares_cap is None else int(shares_cap)
        shares = np.zeros((max(1, cap // SHARE_SIZE), SHARE_SIZE), np.uint8) if want_shares else None
        total = ctypes.c_uint64(0)
        rc = self._ctx._L.cda_square_prove_namespace(self._h, nq, _p(q), mn, _p(results), _p(nodes), _p(leaf_hashes),
                                                     _p(shares), cap if want_shares else 0, ctypes.byref(total))
        self.nshares_total = int(total.value)
        _check(rc, ctx=self._ctx)
        return results, nodes, leaf_hashes, (shares[:self.nshares_total] if want_shares else None)

    def prove_namespace_device(self, queries, max_nodes, d_results, d_nodes, d_leaf_hashes, d_shares=0, shares_cap=0):
        """cda_square_prove_namespace with the outputs at device addresses (queries stay host records).  -> the
        number of shares of all results (also when the call fails for a shares_cap too small: CdaError E_ARG, the
        total then in self.nshares_total)."""
        q = self.namespace_queries(queries)
        V = ctypes.c_void_p
        total = ctypes.c_uint64(0)
        rc = self._ctx._L.cda_square_prove_namespace(self._h, len(q), _p(q), max_nodes, V(d_results), V(d_nodes),
                                                     V(d_leaf_hashes), V(d_shares or None), shares_cap,
                                                     ctypes.byref(total))
        self.nshares_total = int(total.value)
        _check(rc, ctx=self._ctx)
        return self.nshares_total

    def close(self):
        if getattr(self, "_h", None):
            self._ctx._L.cda_square_close(self._h)
        self._h = None

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


_default = None
_default_lock = threading.Lock()


def _batch_outputs(ods, want_eds, eds_out):
    """Shape checks shared by the batch entry points; returns (ods, k, eds, rr, cr, dah)."""
    ods = np.ascontiguousarray(ods, np.uint8)
    if ods.ndim != 3:
        raise CdaError(E_ARG, "ods must be (nblocks, k*k, 512)")
    nb, kk, L = ods.shape
    k = int(round(kk ** 0.5))
    if k * k != kk or L != SHARE_SIZE or nb == 0:
        raise CdaError(E_ARG, "ods must be (nblocks, k*k, 512) with nblocks > 0")
    if eds_out is not None:
        # the library writes nblocks * 4k^2 * 512 bytes through this pointer: it must be exactly that array
        if (not isinstance(eds_out, np.ndarray) or eds_out.dtype != np.uint8 or not eds_out.flags.c_contiguous
                or not eds_out.flags.writeable or eds_out.shape != (nb, 4 * k * k, L)):
            raise CdaError(E_ARG, f"eds_out must be a writeable C-contiguous uint8 array of shape {(nb, 4 * k * k, L)}")
    eds = eds_out if eds_out is not None else (np.empty((nb, 4 * k * k, L), np.uint8) if want_eds else None)
    rr = np.empty((nb, 2 * k, NODE_SIZE), np.uint8)
    cr = np.empty((nb, 2 * k, NODE_SIZE), np.uint8)
    dah = np.empty((nb, 32), np.uint8)
    return ods, k, eds, rr, cr, dah


class PinnedBuffer:
    """Pinned host memory from cda_host_alloc, viewed as a numpy array (freed with the object)."""

    def __init__(self, ctx, shape, dtype=np.uint8):
        nbytes = int(np.prod(shape)) * np.dtype(dtype).itemsize
        ptr = ctypes.c_void_p()
        _check(ctx._L.cda_host_alloc(ctx._h, nbytes, ctypes.byref(ptr)), ctx=ctx)
        self._ctx, self._ptr = ctx, ptr
        buf = (ctypes.c_uint8 * max(1, nbytes)).from_address(ptr.value)
        self.array = np.frombuffer(buf, np.uint8, count=nbytes).view(dtype).reshape(shape)

    def free(self):
        if self._ptr is not None and self._ctx._h:
            self._ctx._L.cda_host_free(self._ctx._h, self._ptr)
        self._ptr = None

    def __del__(self):
        try:
            self.free()
        except Exception:
            pass


class MultiContext:
    """cda_multi: one handle over several GPUs of this process (device mask; 0 = all visible).
    MultiContext.replicas(device, n): n contexts on one device whose split exchanges are device copies."""

    def __init__(self, device_mask=0, _handle=None):
        if _handle is not None:
            self._h = _handle
            return
        h = ctypes.c_void_p()
        rc = lib().cda_multi_init(device_mask, ctypes.byref(h))
        if rc != OK:
            raise CdaError(rc, "cda_multi_init failed")
        self._h = h

    @classmethod
    def replicas(cls, device, count):
        h = ctypes.c_void_p()
        rc = lib().cda_multi_init_replicas(device, count, ctypes.byref(h))
        if rc != OK:
            raise CdaError(rc, "cda_multi_init_replicas failed")
        return cls(_handle=h)

    def context(self, i):
        """Context view of device i's cda_ctx (owned by this handle)."""
        c = Context.__new__(Context)
        c._L = lib()
        c._h = ctypes.c_void_p(lib().cda_multi_context(self._h, i))
        c.device = lib().cda_multi_device(self._h, i)
        c._borrowed = True
        return c

    def extend_commit_split(self, ods, want_eds=True):
        """ONE k x k square (ods: (k*k, 512) uint8) split over the handle's devices (cda_multi_extend_commit_split).
        Returns (eds or None, row_roots, col_roots, dah bytes)."""
        ods = np.ascontiguousarray(ods, np.uint8)
        count = ods.shape[0]
        k = int(round(count ** 0.5))
        if k * k != count or ods.shape[1] != SHARE_SIZE:
            raise CdaError(E_ARG, "ods must be (k*k, 512)")
        eds = np.empty((4 * k * k, SHARE_SIZE), np.uint8) if want_eds else None
        rr = np.zeros((2 * k, NODE_SIZE), np.uint8)
        cr = np.zeros((2 * k, NODE_SIZE), np.uint8)
        dah = np.zeros(32, np.uint8)
        err = ErrInfo()
        rc = lib().cda_multi_extend_commit_split(self._h, k, _p(ods), _p(eds), _p(rr), _p(cr), _p(dah),
                                                 ctypes.byref(err))
        _check(rc, err, self.context(0))
        return eds, rr, cr, dah.tobytes()

    def extend_commit_split_device(self, k, slab_ptrs):
        """The split with device g's ODS rows already at device pointer slab_ptrs[g]; returns (rr, cr, dah)."""
        arr = (ctypes.c_void_p * len(slab_ptrs))(*slab_ptrs)
        rr = np.zeros((2 * k, NODE_SIZE), np.uint8)
        cr = np.zeros((2 * k, NODE_SIZE), np.uint8)
        dah = np.zeros(32, np.uint8)
        err = ErrInfo()
        rc = lib().cda_multi_extend_commit_split_device(self._h, k, arr, _p(rr), _p(cr), _p(dah), ctypes.byref(err))
        _check(rc, err, self.context(0))
        return rr, cr, dah.tobytes()

    @property
    def device_count(self):
        return lib().cda_multi_device_count(self._h)

    def extend_commit_batch(self, ods, want_eds=True, eds_out=None):
        ods, k, eds, rr, cr, dah = _batch_outputs(ods, want_eds, eds_out)
        err = ErrInfo()
        rc = lib().cda_multi_extend_commit_batch(self._h, k, len(ods), _p(ods), _p(eds), _p(rr), _p(cr), _p(dah),
                                                 ctypes.byref(err))
        _check(rc, err)
        return eds, rr, cr, dah

    def close(self):
        if getattr(self, "_h", None):
            lib().cda_multi_free(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


def default_context():
    global _default
    with _default_lock:
        if _default is None:
            _default = Context(int(os.environ.get("LOCAL_RANK", "0")) if os.environ.get("CDA_USE_LOCAL_RANK") else 0)
    return _default
