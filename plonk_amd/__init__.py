"""plonk_amd — MI355X (gfx950) backend for dusk-plonk's prover hot path.

Host-side mirror of the reference's two crate-private seams, over the C-ABI of
libplonk_hip.so (include/plonk_hip.h):

  Context.ntt(...)   EvaluationDomain::{fft, ifft, coset_fft, coset_ifft}
                     (reference src/fft/domain.rs:166-232)
  Context.srs_load   CommitKey { powers_of_g } (src/commitment_scheme/kzg10/key.rs:37-41)
  Context.msm / commit   CommitKey::commit -> msm_variable_base (key.rs:376-388)
  Context.kzg_open / kzg_flatten, KzgKey.batch_check   compute_aggregate_witness + commit, AggregateProof::flatten,
                     OpeningKey::batch_check (key.rs:394-417, 661-707; proof.rs:69-109)
  KzgDomain.open     the n witnesses, n evaluations and the commitment of a polynomial over a whole evaluation domain
                     (open_single at every root of unity, by group FFTs)

There is NO CPU fallback: if the HIP library or a GPU is missing every call
raises.  Nothing in this package imports `oracle/`.
"""
from __future__ import annotations

import ctypes
import os
import weakref
from typing import Iterable, Sequence

# dmabuf IPC: RCCL between processes needs it on this platform's driver, and it must be in the environment before the
# first HIP call of the process — the host program's job (include/plonk_hip.h, "Multi-GPU"); this binding is that host
os.environ.setdefault("HSA_ENABLE_IPC_MODE_LEGACY", "0")

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.environ.get("PLONK_HIP_LIB") or os.path.join(_HERE, "lib", "libplonk_hip.so")   # override: A/B builds

# field constants needed to marshal Python ints <-> Montgomery limbs at the ABI
Q = 0x73EDA753299D7D483339D80809A1D80553BDA402FFFE5BFEFFFFFFFF00000001
P = 0x1A0111EA397FE69A4B1BA7B6434BACD764774B84F38512BF6730D2A0F6B0F6241EABFFFEB153FFFFB9FEFFFFFFFFAAAB
_FR_R = (1 << 256) % Q
_FR_RINV = pow(_FR_R, -1, Q)
_FP_R = (1 << 384) % P
_FP_RINV = pow(_FP_R, -1, P)

PLONK_OK = 0
ERRORS = {
    -1: "PLONK_ERR_ARG", -2: "PLONK_ERR_HIP", -3: "PLONK_ERR_DEGREE (PolynomialDegreeTooLarge)",
    -4: "PLONK_ERR_NO_SRS", -5: "PLONK_ERR_NO_GPU", -6: "PLONK_ERR_UNSAT (CircuitUnsatisfied)",
    -7: "PLONK_ERR_STATE", -8: "PLONK_ERR_BYTES (NotEnoughBytes)", -9: "PLONK_ERR_DATA (InvalidData)",
    -10: "PLONK_ERR_POINT (PointMalformed)", -11: "PLONK_ERR_NOMEM (host allocation failed inside the library)",
    -12: "PLONK_ERR_VERIFY (ProofVerificationError)",
}

# every symbol include/plonk_hip.h declares (checked by tests/test_capi_symbols.py)
EXPORTS = [
    "plonk_ctx_create", "plonk_ctx_destroy", "plonk_last_error", "plonk_ntt", "plonk_ntt_batch",
    "plonk_srs_load", "plonk_msm", "plonk_msm_batch", "plonk_ntt_dev", "plonk_msm_dev",
    "plonk_srs_load_dev", "plonk_srs_generate_dev", "plonk_dev_alloc", "plonk_dev_free",
    "plonk_dev_h2d", "plonk_dev_d2h", "plonk_dev_sync", "plonk_ctx_stream", "plonk_ctx_table_rows",
    "plonk_profile_enable", "plonk_profile_read", "plonk_profile_reset",
    "plonk_prover_create", "plonk_prover_destroy", "plonk_prover_vk", "plonk_prover_size",
    "plonk_prover_prove", "plonk_prover_prove_dev", "plonk_prover_peek",
    "plonk_prover_blob_check", "plonk_prover_from_bytes", "plonk_srs_validate",
    "plonk_comm_unique_id", "plonk_comm_init", "plonk_comm_info", "plonk_comm_selftest", "plonk_comm_destroy",
    "plonk_comm_measure_loopback", "plonk_comm_warning", "plonk_prover_set_version", "plonk_comm_set_library", "plonk_comm_library",
    "plonk_ctx_create_ex", "plonk_ctx_get_config", "plonk_ctx_set_config", "plonk_ctx_describe_msm", "plonk_ctx_last_msm",
    "plonk_ctx_table_bytes", "plonk_prover_describe",
    "plonk_host_alloc", "plonk_host_free", "plonk_lagrange_key",
    "plonk_compile", "plonk_prover_prove_witnesses", "plonk_prover_to_bytes", "plonk_verifier_to_bytes",
    "plonk_public_parameters_check", "plonk_srs_load_public_parameters",
    "plonk_verifier_from_bytes", "plonk_verifier_destroy", "plonk_verifier_set_version", "plonk_verify", "plonk_verifier_last",
    "plonk_verify_mixed",
    "plonk_prover_diagnose", "plonk_prover_diagnose_dev", "plonk_prover_diagnose_witnesses",
    "plonk_kzg_open", "plonk_kzg_open_dev", "plonk_kzg_flatten", "plonk_kzg_key_create", "plonk_kzg_key_destroy",
    "plonk_kzg_batch_check", "plonk_srs_check",
    "plonk_composer_create", "plonk_composer_destroy", "plonk_composer_witness", "plonk_composer_gate", "plonk_composer_gadget",
    "plonk_composer_info", "plonk_composer_layout", "plonk_compile_composer",
    "plonk_prover_fill_inputs", "plonk_prover_prove_inputs", "plonk_prover_diagnose_inputs",
    "plonk_msm_points", "plonk_msm_points_dev", "plonk_ctx_last_msm_points",
    "plonk_kzg_pairing_check_each", "plonk_kzg_check_each", "plonk_verify_each",
    "plonk_kzg_domain_create", "plonk_kzg_domain_destroy", "plonk_kzg_domain_points", "plonk_kzg_open_domain",
    "plonk_kzg_open_domain_dev", "plonk_kzg_domain_last",
    "plonk_kzg_commit_evals", "plonk_kzg_commit_evals_dev", "plonk_kzg_open_evals", "plonk_kzg_open_evals_dev",
    "plonk_kzg_evals_last",
    "plonk_kzg_evals_tables_build", "plonk_kzg_evals_tables_drop", "plonk_kzg_evals_tables_last",
    "plonk_kzg_many_tables_build", "plonk_kzg_many_tables_drop", "plonk_kzg_commit_many", "plonk_kzg_commit_many_dev",
    "plonk_kzg_update_many", "plonk_kzg_many_last",
    "plonk_kzg_tree_create", "plonk_kzg_tree_destroy", "plonk_kzg_tree_build", "plonk_kzg_tree_build_dev", "plonk_kzg_tree_root",
    "plonk_kzg_tree_nodes", "plonk_kzg_tree_update", "plonk_kzg_tree_proof_nodes", "plonk_kzg_tree_prove", "plonk_kzg_tree_check",
    "plonk_kzg_tree_last",
    "plonk_kzg_open_cells", "plonk_kzg_open_cells_dev", "plonk_kzg_cell_points", "plonk_kzg_cells_last",
    "plonk_kzg_cell_verifier_create", "plonk_kzg_cell_verifier_destroy", "plonk_kzg_verify_cells", "plonk_kzg_verify_cells_each",
    "plonk_kzg_cell_verifier_last",
    "plonk_kzg_recover_cells", "plonk_kzg_recover_cells_dev", "plonk_kzg_recover_last",
    "plonk_kzg_multiproof_open", "plonk_kzg_multiproof_open_dev", "plonk_kzg_multiproof_last", "plonk_kzg_multiproof_check",
]

# what bit f of plonk_unsat_row.families / slot f of plonk_unsat_info.family_rows stands for (include/plonk_hip.h); the
# 18th names the copy-constraint slot
IDENTITY_FAMILIES = [
    "arithmetic gate",
    "range: quad c - 4d", "range: quad b - 4c", "range: quad a - 4b", "range: quad next d - 4a",
    "logic: left quad", "logic: right quad", "logic: output quad", "logic: product of the input quads", "logic: xor/and relation",
    "fixed-base: scalar bit", "fixed-base: xy of the bit", "fixed-base: x accumulator", "fixed-base: y accumulator",
    "curve addition: x1 y2", "curve addition: x3", "curve addition: y3",
    "copy constraint",
]

POLY_ORDER = ["q_m", "q_l", "q_r", "q_o", "q_f", "q_c", "q_arith", "q_range", "q_logic",
              "q_fixed_group_add", "q_variable_group_add", "s_sigma_1", "s_sigma_2", "s_sigma_3", "s_sigma_4"]


TABLE_AUTO, TABLE_WINDOW, TABLE_HALFPOS, TABLE_BITPOS = 0, 16, 128, 256
TABLE_QUARTERPOS = 64
PLAN_TAIL_SERIAL, PLAN_BUCKET_SUM_LANE, PLAN_ACCUMULATE_LDS, PLAN_SORT13 = 1, 2, 4, 8


class GpuConfig(ctypes.Structure):
    """plonk_gpu_config (include/plonk_hip.h): zero = default for every field; struct_size is filled in by the binding."""
    _fields_ = [("struct_size", ctypes.c_uint32), ("reserved", ctypes.c_uint32), ("table_budget_bytes", ctypes.c_uint64),
                ("table_mode", ctypes.c_int32), ("msm_bucket_bits", ctypes.c_int32), ("quotient_domain", ctypes.c_int32),
                ("wire_commit", ctypes.c_int32), ("shard_quotient", ctypes.c_int32), ("shard_grand_product", ctypes.c_int32),
                ("shard_side_stream", ctypes.c_int32), ("ntt_elements_log2", ctypes.c_int32), ("comm_timeout_ms", ctypes.c_int32),
                ("side_stream_cus", ctypes.c_int32)]

    def __init__(self, **kw):
        super().__init__(**kw)
        self.struct_size = ctypes.sizeof(GpuConfig)

    def as_dict(self) -> dict:
        return {k: getattr(self, k) for k, _ in self._fields_ if k not in ("struct_size", "reserved")}


class _MsmPlan(ctypes.Structure):
    _fields_ = [("table_rows", ctypes.c_uint32), ("bucket_bits", ctypes.c_uint32), ("digit_width", ctypes.c_uint32),
                ("slice_entries", ctypes.c_uint32), ("ordered_lanes", ctypes.c_uint32), ("wide_words", ctypes.c_uint32),
                ("flags", ctypes.c_uint32), ("reserved", ctypes.c_uint32), ("terms", ctypes.c_uint64), ("accumulate_kernel", ctypes.c_char * 64)]

    def as_dict(self) -> dict:
        d = {k: getattr(self, k) for k, _ in self._fields_}
        d["accumulate_kernel"] = d["accumulate_kernel"].decode()
        return d


POINTS_COMPRESSED, POINTS_CHECK = 1, 2


class _MsmPointsOpts(ctypes.Structure):
    """plonk_msm_points_opts (include/plonk_hip.h): zero = automatic; struct_size is filled in by the binding."""
    _fields_ = [("struct_size", ctypes.c_uint32), ("flags", ctypes.c_uint32), ("window_bits", ctypes.c_uint32),
                ("slice_entries", ctypes.c_uint32), ("min_bucket_terms", ctypes.c_uint32), ("reserved", ctypes.c_uint32)]

    def __init__(self, **kw):
        super().__init__(**kw)
        self.struct_size = ctypes.sizeof(_MsmPointsOpts)


class _MsmPointsInfo(ctypes.Structure):
    _fields_ = [("path", ctypes.c_uint32), ("window_bits", ctypes.c_uint32), ("windows", ctypes.c_uint32),
                ("slice_entries", ctypes.c_uint32), ("terms", ctypes.c_uint64), ("nonzero_digits", ctypes.c_uint64),
                ("slices", ctypes.c_uint64), ("longest_bucket", ctypes.c_uint64)]


class _KzgDomainInfo(ctypes.Structure):
    """plonk_kzg_domain_info (include/plonk_hip.h)"""
    _fields_ = [("log_n", ctypes.c_uint32), ("chunks", ctypes.c_uint32), ("count", ctypes.c_uint64),
                ("device_bytes", ctypes.c_uint64), ("workspace_cap_bytes", ctypes.c_uint64), ("chunk_polys", ctypes.c_uint64),
                ("stage_launches", ctypes.c_uint64), ("scalar_muls", ctypes.c_uint64)]


class _KzgEvalsInfo(ctypes.Structure):
    """plonk_kzg_evals_info (include/plonk_hip.h)"""
    _fields_ = [("log_n", ctypes.c_uint32), ("built_points", ctypes.c_uint32), ("count", ctypes.c_uint64),
                ("in_domain_index", ctypes.c_uint64), ("msm_launches", ctypes.c_uint64), ("msm_terms", ctypes.c_uint64),
                ("lagrange_bytes", ctypes.c_uint64)]


class _KzgEvalsTablesInfo(ctypes.Structure):
    """plonk_kzg_evals_tables_info (include/plonk_hip.h)"""
    _fields_ = [("log_n", ctypes.c_uint32), ("table_rows", ctypes.c_uint32), ("table_bytes", ctypes.c_uint64),
                ("built", ctypes.c_uint32), ("bucket_bits", ctypes.c_uint32), ("msms", ctypes.c_uint64),
                ("group_launches", ctypes.c_uint64), ("device_finished", ctypes.c_uint32), ("reserved", ctypes.c_uint32)]


class _KzgManyInfo(ctypes.Structure):
    """plonk_kzg_many_info (include/plonk_hip.h)"""
    _fields_ = [("log_n", ctypes.c_uint32), ("window_bits", ctypes.c_uint32), ("windows", ctypes.c_uint32), ("built", ctypes.c_uint32),
                ("table_bytes", ctypes.c_uint64), ("count", ctypes.c_uint64), ("terms", ctypes.c_uint64), ("chunks", ctypes.c_uint64),
                ("chunk_vectors", ctypes.c_uint64), ("slices", ctypes.c_uint32), ("reserved", ctypes.c_uint32),
                ("additions", ctypes.c_uint64)]


class _KzgTreeInfo(ctypes.Structure):
    _fields_ = [("log_n", ctypes.c_uint32), ("depth", ctypes.c_uint32), ("built", ctypes.c_uint32), ("kind", ctypes.c_uint32),
                ("leaves", ctypes.c_uint64), ("device_bytes", ctypes.c_uint64), ("touched_nodes", ctypes.c_uint64),
                ("sparse_terms", ctypes.c_uint64), ("chunks", ctypes.c_uint64), ("items", ctypes.c_uint64), ("vectors", ctypes.c_uint64)]


class _KzgCellsInfo(ctypes.Structure):
    """plonk_kzg_cells_info (include/plonk_hip.h)"""
    _fields_ = [("log_n", ctypes.c_uint32), ("log_cell", ctypes.c_uint32), ("chunks", ctypes.c_uint32), ("built_table", ctypes.c_uint32),
                ("count", ctypes.c_uint64), ("slices", ctypes.c_uint64), ("chunk_polys", ctypes.c_uint64),
                ("workspace_bytes", ctypes.c_uint64), ("table_bytes", ctypes.c_uint64), ("stage_launches", ctypes.c_uint64),
                ("scalar_muls", ctypes.c_uint64)]


class _KzgRecoverInfo(ctypes.Structure):
    """plonk_kzg_recover_info (include/plonk_hip.h)"""
    _fields_ = [("log_n", ctypes.c_uint32), ("log_cell", ctypes.c_uint32), ("chunks", ctypes.c_uint32), ("built_table", ctypes.c_uint32),
                ("count", ctypes.c_uint64), ("available", ctypes.c_uint64), ("missing", ctypes.c_uint64), ("max_len", ctypes.c_uint64),
                ("chunk_polys", ctypes.c_uint64), ("transforms", ctypes.c_uint64), ("vanish_muls", ctypes.c_uint64),
                ("workspace_bytes", ctypes.c_uint64), ("inconsistent", ctypes.c_uint64)]


class _KzgMultiproofInfo(ctypes.Structure):
    """plonk_kzg_multiproof_info (include/plonk_hip.h)"""
    _fields_ = [("log_n", ctypes.c_uint32), ("built_points", ctypes.c_uint32), ("items", ctypes.c_uint64), ("vectors", ctypes.c_uint64),
                ("point_groups", ctypes.c_uint64), ("commitments_computed", ctypes.c_uint64), ("msm_launches", ctypes.c_uint64),
                ("msm_terms", ctypes.c_uint64), ("products", ctypes.c_uint64), ("device_bytes", ctypes.c_uint64)]


class _KzgCellVerifyInfo(ctypes.Structure):
    """plonk_kzg_cell_verify_info (include/plonk_hip.h)"""
    _fields_ = [("log_n", ctypes.c_uint32), ("log_cell", ctypes.c_uint32), ("key_checked", ctypes.c_uint32), ("path_each", ctypes.c_uint32),
                ("items", ctypes.c_uint64), ("commitments", ctypes.c_uint64), ("transforms", ctypes.c_uint64),
                ("msm_terms_left", ctypes.c_uint64), ("msm_terms_right", ctypes.c_uint64),
                ("msm_path_left", ctypes.c_uint32), ("msm_path_right", ctypes.c_uint32),
                ("scalar_muls", ctypes.c_uint64), ("device_bytes", ctypes.c_uint64)]


class _ProverInfo(ctypes.Structure):
    _fields_ = [("size", ctypes.c_uint64), ("quotient_domain", ctypes.c_uint32), ("wire_commit_values", ctypes.c_uint32),
                ("lagrange_table_rows", ctypes.c_uint32), ("shard_world", ctypes.c_uint32), ("shard_rank", ctypes.c_uint32),
                ("sharded_quotient", ctypes.c_uint32), ("quotient_classes", ctypes.c_uint32), ("wire_group_launches", ctypes.c_uint32),
                ("lagrange_points", ctypes.c_uint64)]


class _ProverDesc(ctypes.Structure):
    _fields_ = [("constraints", ctypes.c_uint64), ("label", ctypes.c_char_p), ("label_len", ctypes.c_uint64),
                ("polys", ctypes.c_void_p * 15), ("poly_len", ctypes.c_uint64 * 15),
                ("vk_commitments", ctypes.c_char_p), ("shard_rank", ctypes.c_int), ("shard_world", ctypes.c_int),
                ("srs_total", ctypes.c_uint64), ("allgather", ctypes.c_void_p), ("allgather_user", ctypes.c_void_p),
                ("lagrange_xy96", ctypes.c_char_p), ("lagrange_count", ctypes.c_uint64)]


class _CircuitDesc(ctypes.Structure):
    _fields_ = [("constraints", ctypes.c_uint64), ("label", ctypes.c_char_p), ("label_len", ctypes.c_uint64),
                ("selectors", ctypes.c_void_p * 11), ("wires", ctypes.c_void_p * 4), ("witnesses", ctypes.c_uint64),
                ("shard_rank", ctypes.c_int), ("shard_world", ctypes.c_int),
                ("srs_total", ctypes.c_uint64), ("allgather", ctypes.c_void_p), ("allgather_user", ctypes.c_void_p),
                ("lagrange_xy96", ctypes.c_char_p), ("lagrange_count", ctypes.c_uint64)]


class _UnsatRow(ctypes.Structure):
    _fields_ = [("row", ctypes.c_uint64), ("families", ctypes.c_uint32), ("copy_wires", ctypes.c_uint32)]


class _UnsatInfo(ctypes.Structure):
    _fields_ = [("rows_checked", ctypes.c_uint64), ("rows_failing", ctypes.c_uint64), ("family_rows", ctypes.c_uint64 * 18),
                ("first_row", ctypes.c_uint64), ("first_family", ctypes.c_uint32), ("reserved", ctypes.c_uint32),
                ("ms", ctypes.c_double)]


class Diagnosis:
    """What plonk_prover_diagnose* reports: ok, rows = [(row, families, copy_wires)] ascending (at most `cap` of them),
    and the plonk_unsat_info fields as attributes (info: the same as a dict, without the timing)."""

    def __init__(self, rc: int, rows, info: "_UnsatInfo"):
        self.ok = rc == PLONK_OK
        self.rows = rows
        self.rows_checked, self.rows_failing = info.rows_checked, info.rows_failing
        self.family_rows = list(info.family_rows)
        self.first_row, self.first_family = info.first_row, info.first_family   # 2^64 - 1 / 0 when no row fails
        self.ms = info.ms

    @property
    def info(self) -> dict:
        return dict(rows_checked=self.rows_checked, rows_failing=self.rows_failing, family_rows=self.family_rows,
                    first_row=self.first_row, first_family=self.first_family)

    def __repr__(self):
        if self.ok:
            return f"Diagnosis(ok, {self.rows_checked} rows)"
        return (f"Diagnosis({self.rows_failing} of {self.rows_checked} rows fail; first: row {self.first_row}, "
                f"{IDENTITY_FAMILIES[self.first_family]})")


class _ComposerSummary(ctypes.Structure):
    _fields_ = [("constraints", ctypes.c_uint64), ("witnesses", ctypes.c_uint64), ("inputs", ctypes.c_uint64),
                ("public_rows", ctypes.c_uint64), ("records", ctypes.c_uint64), ("levels", ctypes.c_uint64),
                ("widest_level", ctypes.c_uint64)]


class _BlobInfo(ctypes.Structure):
    _fields_ = [("size", ctypes.c_uint64), ("constraints", ctypes.c_uint64), ("label_off", ctypes.c_uint64),
                ("label_len", ctypes.c_uint64), ("poly_off", ctypes.c_uint64 * 15), ("poly_len", ctypes.c_uint64 * 15),
                ("srs_off", ctypes.c_uint64), ("srs_points", ctypes.c_uint64), ("vk_off", ctypes.c_uint64)]


class _VerifyInfo(ctypes.Structure):
    _fields_ = [("proofs", ctypes.c_uint64), ("msm_terms", ctypes.c_uint64), ("pairing_checks", ctypes.c_uint32),
                ("rejected", ctypes.c_uint32), ("ms_decode", ctypes.c_double), ("ms_scalars", ctypes.c_double),
                ("ms_msm", ctypes.c_double), ("ms_pairing", ctypes.c_double)]


class KzgProof(ctypes.Structure):
    """plonk_kzg_proof = kzg10::Proof (reference proof.rs:15-23): commitment to the polynomial (48-byte compressed), the
    evaluation (Fr, Montgomery limbs), commitment to the witness.  `KzgProof.make(commitment, evaluation, witness)` takes the
    evaluation as an int; `.value` gives it back."""
    _fields_ = [("commitment", ctypes.c_uint8 * 48), ("evaluation", ctypes.c_uint64 * 4), ("witness", ctypes.c_uint8 * 48)]

    @classmethod
    def make(cls, commitment: bytes, evaluation: int, witness: bytes) -> "KzgProof":
        p = cls()
        ctypes.memmove(p.commitment, bytes(commitment), 48)
        ctypes.memmove(p.evaluation, fr_to_bytes_mont([evaluation]), 32)
        ctypes.memmove(p.witness, bytes(witness), 48)
        return p

    @property
    def value(self) -> int:
        return fr_from_bytes_mont(bytes(self.evaluation))[0]


class _PublicParametersInfo(ctypes.Structure):
    _fields_ = [("opening_key_off", ctypes.c_uint64), ("points_off", ctypes.c_uint64), ("point_stride", ctypes.c_uint64),
                ("points_total", ctypes.c_uint64), ("points_kept", ctypes.c_uint64)]


PP_RAW_UNCHECKED, PP_RAW, PP_COMPRESSED = 0, 1, 2   # plonk_hip.h PLONK_PP_*


ALLGATHER_FN = ctypes.CFUNCTYPE(ctypes.c_int, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_uint64)


def shard_range(total: int, rank: int, world: int) -> tuple[int, int]:
    """Contiguous SRS point range owned by `rank` (same rule as prover.hip)."""
    per = (total + world - 1) // world
    lo = min(per * rank, total)
    return lo, min(lo + per, total)


class CircuitUnsatisfied(Exception):
    """Mirrors Error::CircuitUnsatisfied (reference quotient_poly.rs:132)."""


class PlonkError(RuntimeError):
    def __init__(self, code: int, detail: str = ""):
        self.code = code
        super().__init__(f"{ERRORS.get(code, code)} {detail}".strip())


class NotEnoughBytes(PlonkError):
    """Mirrors Error::NotEnoughBytes (reference prover.rs:274,310; widget.rs:484; key.rs:265,281)."""


class InvalidData(PlonkError):
    """Mirrors dusk_bytes::Error::InvalidData as the reference's decoders raise it."""


class PointMalformed(PlonkError):
    """Mirrors Error::PointMalformed (reference key.rs:292)."""


_DECODE_ERRORS = {-8: NotEnoughBytes, -9: InvalidData, -10: PointMalformed}


class ProofVerificationError(PlonkError):
    """Mirrors Error::ProofVerificationError (reference proof.rs:502-512): plonk_verify's PLONK_ERR_VERIFY."""


class PolynomialDegreeTooLarge(PlonkError):
    """Mirrors Error::PolynomialDegreeTooLarge (reference key.rs:362-370)."""


_lib = None


def load_library() -> ctypes.CDLL:
    """dlopen libplonk_hip.so (built in-tree by __graft_entry__.build()).  Fails loudly."""
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(LIB_PATH):
        raise FileNotFoundError(
            f"{LIB_PATH} not built — run `python __graft_entry__.py` (hipcc --offload-arch=gfx950)")
    lib = ctypes.CDLL(LIB_PATH)
    vp, u64, u32, ci = ctypes.c_void_p, ctypes.c_uint64, ctypes.c_uint32, ctypes.c_int
    lib.plonk_last_error.restype = ctypes.c_char_p
    lib.plonk_ctx_create.argtypes = [ctypes.POINTER(vp), ctypes.POINTER(ci), ci]
    lib.plonk_ctx_destroy.argtypes = [vp]
    lib.plonk_ctx_destroy.restype = None
    lib.plonk_ntt.argtypes = [vp, vp, u32, ci, ci, u64]
    lib.plonk_ntt_batch.argtypes = [vp, ctypes.POINTER(vp), ci, u32, ci, ci, ctypes.POINTER(u64)]
    lib.plonk_srs_load.argtypes = [vp, vp, u64]
    lib.plonk_msm.argtypes = [vp, vp, u64, vp]
    lib.plonk_msm_batch.argtypes = [vp, ctypes.POINTER(vp), ctypes.POINTER(u64), ci, vp]
    lib.plonk_ntt_dev.argtypes = [vp, vp, vp, vp, u32, ci, ci, u64]
    lib.plonk_msm_dev.argtypes = [vp, vp, u64, vp]
    lib.plonk_srs_load_dev.argtypes = [vp, vp, u64]
    lib.plonk_srs_generate_dev.argtypes = [vp, vp, vp, u64, vp]
    lib.plonk_dev_alloc.argtypes = [vp, u64, ctypes.POINTER(vp)]
    lib.plonk_dev_free.argtypes = [vp, vp]
    lib.plonk_dev_h2d.argtypes = [vp, vp, vp, u64]
    lib.plonk_dev_d2h.argtypes = [vp, vp, vp, u64]
    lib.plonk_dev_sync.argtypes = [vp]
    lib.plonk_ctx_stream.argtypes = [vp]
    lib.plonk_ctx_table_rows.argtypes = [vp]
    lib.plonk_ctx_stream.restype = vp
    lib.plonk_profile_enable.argtypes = [vp, ci]
    lib.plonk_profile_read.argtypes = [vp, ci, ctypes.POINTER(ctypes.c_double), ctypes.POINTER(u64)]
    lib.plonk_profile_reset.argtypes = [vp]
    lib.plonk_prover_create.argtypes = [vp, ctypes.POINTER(_ProverDesc), ctypes.POINTER(vp)]
    lib.plonk_prover_destroy.argtypes = [vp]
    lib.plonk_prover_destroy.restype = None
    lib.plonk_prover_vk.argtypes = [vp, vp]
    lib.plonk_prover_size.argtypes = [vp]
    lib.plonk_prover_size.restype = u64
    lib.plonk_prover_peek.argtypes = [vp, ci, u64, u64, vp]
    lib.plonk_prover_prove.argtypes = [vp, ctypes.POINTER(vp), vp, vp, u64, vp, vp]
    lib.plonk_prover_prove_dev.argtypes = [vp, vp, vp, vp, u64, vp, vp]
    lib.plonk_prover_blob_check.argtypes = [vp, u64, ctypes.POINTER(_BlobInfo)]
    lib.plonk_prover_from_bytes.argtypes = [vp, vp, u64, ctypes.POINTER(vp)]
    lib.plonk_srs_validate.argtypes = [vp, vp, u64]
    lib.plonk_public_parameters_check.argtypes = [vp, u64, u64, ci, ctypes.POINTER(_PublicParametersInfo)]
    lib.plonk_srs_load_public_parameters.argtypes = [vp, vp, u64, u64, ci, vp, ctypes.POINTER(u64)]
    lib.plonk_lagrange_key.argtypes = [vp, u32, vp]
    lib.plonk_compile.argtypes = [vp, ctypes.POINTER(_CircuitDesc), ctypes.POINTER(vp)]
    lib.plonk_prover_prove_witnesses.argtypes = [vp, vp, u64, vp, vp, u64, vp, vp]
    lib.plonk_prover_to_bytes.argtypes = [vp, vp, u64, ctypes.POINTER(u64)]
    lib.plonk_verifier_to_bytes.argtypes = [vp, vp, u64, vp, u64, vp, u64, ctypes.POINTER(u64)]
    lib.plonk_verifier_from_bytes.argtypes = [vp, vp, u64, ctypes.POINTER(vp)]
    lib.plonk_verifier_destroy.argtypes = [vp]
    lib.plonk_verifier_destroy.restype = None
    lib.plonk_verifier_set_version.argtypes = [vp, ci]
    lib.plonk_verify.argtypes = [vp, vp, vp, u64, u64, vp]
    lib.plonk_verifier_last.argtypes = [vp, vp]
    lib.plonk_test_verify_msm.argtypes = [vp, vp, vp, u64, vp]   # test hook of verify.hip, not in the header
    lib.plonk_verify_mixed.argtypes = [vp, u32, vp, vp, vp, u64, u64, vp, vp]
    lib.plonk_test_verify_replay.argtypes = [vp, u32, vp, vp, vp, u64, u64, vp, vp, vp]   # test hook of verify.hip
    lib.plonk_host_alloc.argtypes = [u64, ctypes.POINTER(vp)]
    lib.plonk_host_free.argtypes = [vp]
    lib.plonk_comm_unique_id.argtypes = [vp]
    lib.plonk_comm_init.argtypes = [vp, vp, ci, ci]
    lib.plonk_comm_selftest.argtypes = [vp]
    lib.plonk_comm_info.argtypes = [vp, ctypes.POINTER(ci), ctypes.POINTER(ci)]
    lib.plonk_comm_destroy.argtypes = [vp]
    lib.plonk_comm_warning.argtypes = [vp, vp, u64]
    lib.plonk_comm_measure_loopback.argtypes = [vp, ci]
    lib.plonk_ctx_create_ex.argtypes = [ctypes.POINTER(vp), ci, ctypes.POINTER(GpuConfig)]
    lib.plonk_ctx_get_config.argtypes = [vp, ctypes.POINTER(GpuConfig)]
    lib.plonk_ctx_set_config.argtypes = [vp, ctypes.POINTER(GpuConfig)]
    lib.plonk_ctx_describe_msm.argtypes = [vp, u64, ci, ci, u32, u64, ctypes.POINTER(_MsmPlan)]
    lib.plonk_ctx_last_msm.argtypes = [vp, ctypes.POINTER(_MsmPlan)]
    lib.plonk_ctx_table_bytes.argtypes = [vp, ctypes.POINTER(u64), ctypes.POINTER(u64)]
    lib.plonk_prover_describe.argtypes = [vp, ctypes.POINTER(_ProverInfo)]
    lib.plonk_comm_set_library.argtypes = [ctypes.c_char_p]
    lib.plonk_comm_library.argtypes = [vp, u64]
    lib.plonk_prover_set_version.argtypes = [vp, ci]
    lib.plonk_prover_diagnose.argtypes = [vp, ctypes.POINTER(vp), vp, vp, u64, vp, u64, vp]
    lib.plonk_prover_diagnose_dev.argtypes = [vp, vp, vp, vp, u64, vp, u64, vp]
    lib.plonk_prover_diagnose_witnesses.argtypes = [vp, vp, u64, vp, vp, u64, vp, u64, vp]
    lib.plonk_kzg_open.argtypes = [vp, ctypes.POINTER(vp), ctypes.POINTER(u64), u64, vp, vp, vp, vp, vp]
    lib.plonk_kzg_open_dev.argtypes = [vp, ctypes.POINTER(vp), ctypes.POINTER(u64), u64, vp, vp, vp, vp, vp]
    lib.plonk_kzg_flatten.argtypes = [vp, vp, vp, u64, vp, vp, ctypes.POINTER(KzgProof)]
    lib.plonk_kzg_key_create.argtypes = [vp, vp, ctypes.POINTER(vp)]
    lib.plonk_kzg_key_destroy.argtypes = [vp]
    lib.plonk_kzg_key_destroy.restype = None
    lib.plonk_kzg_batch_check.argtypes = [vp, vp, vp, u64, vp, u64, vp, vp]
    lib.plonk_srs_check.argtypes = [vp, vp]
    lib.plonk_test_kzg_last.argtypes = [vp, vp, vp]   # test hook of kzg.hip, not in the header
    lib.plonk_kzg_pairing_check_each.argtypes = [vp, vp, vp, u64, vp, vp]
    lib.plonk_kzg_check_each.argtypes = [vp, vp, vp, u64, vp, vp]
    lib.plonk_verify_each.argtypes = [vp, u32, vp, vp, vp, u64, u64, vp, vp]
    lib.plonk_test_pairing_each.argtypes = [vp, vp, vp, u64, vp]   # test hook of kzg.hip, not in the header
    lib.plonk_composer_create.argtypes = [ctypes.POINTER(vp)]
    lib.plonk_composer_destroy.argtypes = [vp]
    lib.plonk_composer_destroy.restype = None
    lib.plonk_composer_witness.argtypes = [vp, ctypes.POINTER(u32)]
    lib.plonk_composer_gate.argtypes = [vp, vp, vp, u32, ctypes.POINTER(u32)]
    lib.plonk_composer_gadget.argtypes = [vp, ci, u32, vp, u32, vp, u32, vp, u32, ctypes.POINTER(u32)]
    lib.plonk_composer_info.argtypes = [vp, ctypes.POINTER(_ComposerSummary)]
    lib.plonk_composer_layout.argtypes = [vp, vp, vp, vp, vp]
    lib.plonk_compile_composer.argtypes = [vp, vp, vp, u64, ctypes.POINTER(vp)]
    lib.plonk_prover_fill_inputs.argtypes = [vp, vp, u64, vp, vp]
    lib.plonk_prover_prove_inputs.argtypes = [vp, vp, u64, vp, vp, vp]
    lib.plonk_prover_diagnose_inputs.argtypes = [vp, vp, u64, vp, u64, vp]
    lib.plonk_msm_points.argtypes = [vp, vp, vp, u64, ctypes.POINTER(_MsmPointsOpts), vp]
    lib.plonk_msm_points_dev.argtypes = [vp, vp, vp, u64, ctypes.POINTER(_MsmPointsOpts), vp]
    lib.plonk_ctx_last_msm_points.argtypes = [vp, ctypes.POINTER(_MsmPointsInfo)]
    lib.plonk_kzg_domain_create.argtypes = [vp, u32, ctypes.POINTER(vp)]
    lib.plonk_kzg_domain_destroy.argtypes = [vp]
    lib.plonk_kzg_domain_destroy.restype = None
    lib.plonk_kzg_domain_points.argtypes = [vp, vp]
    lib.plonk_kzg_open_domain.argtypes = [vp, ctypes.POINTER(vp), ctypes.POINTER(u64), u64, vp, vp, vp]
    lib.plonk_kzg_open_domain_dev.argtypes = [vp, ctypes.POINTER(vp), ctypes.POINTER(u64), u64, vp, vp, vp]
    lib.plonk_kzg_domain_last.argtypes = [vp, ctypes.POINTER(_KzgDomainInfo)]
    lib.plonk_test_kzg_domain_set_cap.argtypes = [vp, u64]   # test hook of kzg_domain.hip, not in the header
    lib.plonk_kzg_commit_evals.argtypes = [vp, ctypes.POINTER(vp), u64, vp]
    lib.plonk_kzg_commit_evals_dev.argtypes = [vp, ctypes.POINTER(vp), u64, vp]
    lib.plonk_kzg_open_evals.argtypes = [vp, ctypes.POINTER(vp), u64, vp, vp, vp, vp, vp]
    lib.plonk_kzg_open_evals_dev.argtypes = [vp, ctypes.POINTER(vp), u64, vp, vp, vp, vp, vp]
    lib.plonk_kzg_evals_last.argtypes = [vp, ctypes.POINTER(_KzgEvalsInfo)]
    lib.plonk_kzg_evals_tables_build.argtypes = [vp]
    lib.plonk_kzg_evals_tables_drop.argtypes = [vp]
    lib.plonk_kzg_evals_tables_last.argtypes = [vp, ctypes.POINTER(_KzgEvalsTablesInfo)]
    lib.plonk_kzg_many_tables_build.argtypes = [vp, u32]
    lib.plonk_kzg_many_tables_drop.argtypes = [vp]
    lib.plonk_kzg_commit_many.argtypes = [vp, vp, u64, vp]
    lib.plonk_kzg_commit_many_dev.argtypes = [vp, vp, u64, vp]
    lib.plonk_kzg_update_many.argtypes = [vp, vp, vp, vp, vp, u64, vp]
    lib.plonk_kzg_many_last.argtypes = [vp, ctypes.POINTER(_KzgManyInfo)]
    lib.plonk_kzg_tree_create.argtypes = [vp, u32, ctypes.POINTER(vp)]
    lib.plonk_kzg_tree_destroy.argtypes = [vp]
    lib.plonk_kzg_tree_destroy.restype = None
    lib.plonk_kzg_tree_build.argtypes = [vp, vp]
    lib.plonk_kzg_tree_build_dev.argtypes = [vp, vp]
    lib.plonk_kzg_tree_root.argtypes = [vp, vp]
    lib.plonk_kzg_tree_nodes.argtypes = [vp, u32, u64, u64, vp]
    lib.plonk_kzg_tree_update.argtypes = [vp, vp, vp, u64]
    lib.plonk_kzg_tree_proof_nodes.argtypes = [u32, u32, vp, u64, ctypes.POINTER(u64)]
    lib.plonk_kzg_tree_prove.argtypes = [vp, vp, u64, vp, u64, vp, vp, vp, vp]
    lib.plonk_kzg_tree_check.argtypes = [vp, u32, u32, vp, vp, vp, u64, vp, u64, vp, vp, u64, vp, vp]
    lib.plonk_kzg_tree_last.argtypes = [vp, ctypes.POINTER(_KzgTreeInfo)]
    lib.plonk_kzg_open_cells.argtypes = [vp, u32, ctypes.POINTER(vp), ctypes.POINTER(u64), u64, vp, vp, vp]
    lib.plonk_kzg_open_cells_dev.argtypes = [vp, u32, ctypes.POINTER(vp), ctypes.POINTER(u64), u64, vp, vp, vp]
    lib.plonk_kzg_cell_points.argtypes = [vp, u32, vp, vp]
    lib.plonk_kzg_cells_last.argtypes = [vp, ctypes.POINTER(_KzgCellsInfo)]
    lib.plonk_kzg_recover_cells.argtypes = [vp, u32, vp, u64, ctypes.POINTER(vp), u64, u64, vp, vp, vp, vp, vp]
    lib.plonk_kzg_recover_cells_dev.argtypes = [vp, u32, vp, u64, ctypes.POINTER(vp), u64, u64, vp, vp, vp, vp, vp]
    lib.plonk_kzg_recover_last.argtypes = [vp, ctypes.POINTER(_KzgRecoverInfo)]
    lib.plonk_kzg_cell_verifier_create.argtypes = [vp, u32, u32, ctypes.POINTER(vp)]
    lib.plonk_kzg_cell_verifier_destroy.argtypes = [vp]
    lib.plonk_kzg_cell_verifier_destroy.restype = None
    lib.plonk_kzg_verify_cells.argtypes = [vp, vp, u64, vp, vp, vp, vp, u64, vp, u64, vp, vp]
    lib.plonk_kzg_verify_cells_each.argtypes = [vp, vp, u64, vp, vp, vp, vp, u64, vp, vp]
    lib.plonk_kzg_cell_verifier_last.argtypes = [vp, ctypes.POINTER(_KzgCellVerifyInfo)]
    lib.plonk_test_kzg_cell_verify_last_rho.argtypes = [vp, vp]   # test hooks of kzg_cell_verify.hip, not in the header
    lib.plonk_test_kzg_cell_verify_force_paths.argtypes = [vp, u32, u32]
    lib.plonk_kzg_multiproof_open.argtypes = [vp, ctypes.POINTER(vp), u64, vp, vp, vp, u64, vp, u64, vp, vp, vp, vp]
    lib.plonk_kzg_multiproof_open_dev.argtypes = [vp, ctypes.POINTER(vp), u64, vp, vp, vp, u64, vp, u64, vp, vp, vp, vp]
    lib.plonk_kzg_multiproof_last.argtypes = [vp, ctypes.POINTER(_KzgMultiproofInfo)]
    lib.plonk_kzg_multiproof_check.argtypes = [vp, u32, vp, u64, vp, vp, vp, u64, vp, vp, u64, vp, vp]
    lib.plonk_test_kzg_multiproof_last_challenges.argtypes = [vp, vp]   # test hook of kzg_multiproof.hip, not in the header
    _lib = lib
    return lib


def prover_blob_check(blob: bytes) -> dict:
    """Host-only decode + validation of a reference Prover::to_bytes() blob (no GPU needed):
    returns the layout (offsets into `blob`) or raises NotEnoughBytes / InvalidData / PointMalformed."""
    lib = load_library()
    info = _BlobInfo()
    rc = lib.plonk_prover_blob_check(blob, len(blob), ctypes.byref(info))
    if rc in _DECODE_ERRORS:
        raise _DECODE_ERRORS[rc](rc, (lib.plonk_last_error() or b"").decode())
    if rc != PLONK_OK:
        raise PlonkError(rc, (lib.plonk_last_error() or b"").decode())
    return {"size": info.size, "constraints": info.constraints,
            "label": blob[info.label_off:info.label_off + info.label_len],
            "polys": {name: (info.poly_off[k], info.poly_len[k]) for k, name in enumerate(POLY_ORDER)},
            "srs": (info.srs_off, info.srs_points), "vk_off": info.vk_off}


def _pp_mode(validate: bool, compressed: bool) -> int:
    return PP_COMPRESSED if compressed else (PP_RAW if validate else PP_RAW_UNCHECKED)


def public_parameters_check(data: bytes, truncated_degree: int = 0, validate: bool = True, compressed: bool = False) -> dict:
    """Host-only decode of a PublicParameters file (reference srs.rs:103-178, key.rs:215-326; no GPU needed) — the raw form
    (`to_raw_var_bytes`, checked or unchecked) or the compressed form (`to_var_bytes`): the opening-key bytes and the layout of
    the (trimmed) commit key, or NotEnoughBytes / InvalidData / PointMalformed / PlonkError(-3) for a trim beyond the key
    (Error::TruncatedDegreeTooLarge)."""
    lib = load_library()
    info = _PublicParametersInfo()
    rc = lib.plonk_public_parameters_check(data, len(data), truncated_degree, _pp_mode(validate, compressed), ctypes.byref(info))
    if rc in _DECODE_ERRORS:
        raise _DECODE_ERRORS[rc](rc, (lib.plonk_last_error() or b"").decode())
    if rc != PLONK_OK:
        raise PlonkError(rc, (lib.plonk_last_error() or b"").decode())
    return {"opening_key": data[info.opening_key_off:info.opening_key_off + 240], "points_off": info.points_off,
            "point_stride": info.point_stride, "points_total": info.points_total, "points_kept": info.points_kept}


# ---- marshalling -----------------------------------------------------------------
def fr_to_bytes_mont(vals: Iterable[int]) -> bytes:
    return b"".join(((v % Q) * _FR_R % Q).to_bytes(32, "little") for v in vals)


def fr_from_bytes_mont(buf: bytes) -> list[int]:
    return [int.from_bytes(buf[i:i + 32], "little") * _FR_RINV % Q for i in range(0, len(buf), 32)]


def g1_to_raw96(pt) -> bytes:
    x, y = pt
    return (x * _FP_R % P).to_bytes(48, "little") + (y * _FP_R % P).to_bytes(48, "little")


def g1_from_raw97(buf: bytes):
    if buf[96]:
        return None
    return (int.from_bytes(buf[:48], "little") * _FP_RINV % P,
            int.from_bytes(buf[48:96], "little") * _FP_RINV % P)


def g1_compress(pt) -> bytes:
    """Commitment::to_bytes — 48-byte compressed G1 (reference commitment.rs:46-57)."""
    if pt is None:
        return bytes([0xC0]) + bytes(47)
    x, y = pt
    b = bytearray(x.to_bytes(48, "big"))
    b[0] |= 0x80
    if y > (P - y) % P:
        b[0] |= 0x20
    return bytes(b)


class DeviceBuffer:
    def __init__(self, ctx: "Context", nbytes: int):
        self.ctx, self.nbytes = ctx, nbytes
        p = ctypes.c_void_p()
        ctx._check(ctx.lib.plonk_dev_alloc(ctx.handle, nbytes, ctypes.byref(p)))
        self.ptr = p.value

    def upload(self, data: bytes, offset: int = 0):
        assert offset + len(data) <= self.nbytes
        self.ctx._check(self.ctx.lib.plonk_dev_h2d(self.ctx.handle, self.ptr + offset, data, len(data)))

    def download(self, nbytes: int | None = None, offset: int = 0) -> bytes:
        nbytes = self.nbytes - offset if nbytes is None else nbytes
        out = ctypes.create_string_buffer(nbytes)
        self.ctx._check(self.ctx.lib.plonk_dev_d2h(self.ctx.handle, out, self.ptr + offset, nbytes))
        return out.raw

    def free(self):
        if self.ptr:
            self.ctx.lib.plonk_dev_free(self.ctx.handle, self.ptr)
            self.ptr = None


class PinnedBuffer:
    """Pinned host memory (plonk_host_alloc): uploads from it are asynchronous, which is what lets
    plonk_srs_load overlap the streamed key with the table build."""

    def __init__(self, nbytes: int):
        self.lib = load_library()
        p = ctypes.c_void_p()
        rc = self.lib.plonk_host_alloc(nbytes, ctypes.byref(p))
        if rc != PLONK_OK:
            raise PlonkError(rc, (self.lib.plonk_last_error() or b"").decode())
        self.ptr, self.nbytes = p.value, nbytes

    def write(self, data: bytes, offset: int = 0):
        assert offset + len(data) <= self.nbytes
        ctypes.memmove(self.ptr + offset, data, len(data))

    def free(self):
        if self.ptr:
            self.lib.plonk_host_free(self.ptr)
            self.ptr = None


class Context:
    """One GPU, one stream (plonk_ctx).  One process per GPU in multi-GPU runs."""

    def __init__(self, device: int = 0, config: "GpuConfig | None" = None):
        self.lib = load_library()
        h = ctypes.c_void_p()
        if config is None:
            dev = (ctypes.c_int * 1)(device)
            rc = self.lib.plonk_ctx_create(ctypes.byref(h), dev, 1)
        else:
            rc = self.lib.plonk_ctx_create_ex(ctypes.byref(h), device, ctypes.byref(config))
        if rc != PLONK_OK:
            raise PlonkError(rc, (self.lib.plonk_last_error() or b"").decode())
        self.handle = h
        self.srs_points = 0
        self._provers = weakref.WeakSet()   # provers hold a pointer to the native context: close() destroys them first (plonk_hip.h)

    def close(self):
        if getattr(self, "handle", None):
            for p in list(getattr(self, "_provers", ())):
                p.close()
            self.lib.plonk_ctx_destroy(self.handle)
            self.handle = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def _check(self, rc: int):
        if rc == -3:
            raise PolynomialDegreeTooLarge(rc)
        if rc == -6:
            raise CircuitUnsatisfied()
        if rc in _DECODE_ERRORS:
            raise _DECODE_ERRORS[rc](rc, (self.lib.plonk_last_error() or b"").decode())
        if rc != PLONK_OK:
            raise PlonkError(rc, (self.lib.plonk_last_error() or b"").decode())

    # ---- EvaluationDomain seam ------------------------------------------------------
    def ntt_bytes(self, data: bytes, log_n: int, inverse: bool, coset: bool, in_len: int) -> bytes:
        n = 1 << log_n
        buf = ctypes.create_string_buffer(32 * n)
        ctypes.memmove(buf, data, min(len(data), 32 * n))
        self._check(self.lib.plonk_ntt(self.handle, buf, log_n, int(inverse), int(coset), in_len))
        return buf.raw

    def ntt_batch_bytes(self, datas, log_n: int, inverse: bool, coset: bool, in_lens=None) -> list[bytes]:
        """compute_coset_evaluations' fan-out (quotient_poly.rs:139-157) as one plonk_ntt_batch call."""
        n = 1 << log_n
        bufs = []
        for d in datas:
            b = ctypes.create_string_buffer(32 * n)
            ctypes.memmove(b, d, min(len(d), 32 * n))
            bufs.append(b)
        arr = (ctypes.c_void_p * max(len(bufs), 1))(*[ctypes.cast(b, ctypes.c_void_p) for b in bufs])
        lens = None
        if in_lens is not None:
            lens = (ctypes.c_uint64 * max(len(bufs), 1))(*in_lens)
        self._check(self.lib.plonk_ntt_batch(self.handle, arr, len(bufs), log_n, int(inverse), int(coset), lens))
        return [b.raw for b in bufs]

    def msm_batch_bytes(self, scalar_sets) -> list[bytes]:
        """commit_polynomials' fan-out (prover.rs:187-210) as one plonk_msm_batch call: list of
        Montgomery scalar byte strings -> list of 97-byte raw results."""
        keep = [ctypes.create_string_buffer(bytes(s), max(len(s), 1)) for s in scalar_sets]
        arr = (ctypes.c_void_p * max(len(keep), 1))(*[ctypes.cast(b, ctypes.c_void_p) for b in keep])
        ms = (ctypes.c_uint64 * max(len(keep), 1))(*[len(s) // 32 for s in scalar_sets])
        out = ctypes.create_string_buffer(97 * max(len(keep), 1))
        self._check(self.lib.plonk_msm_batch(self.handle, arr, ms, len(keep), out))
        return [out.raw[97 * i:97 * i + 97] for i in range(len(keep))]

    def ntt(self, values: Sequence[int], log_n: int, inverse: bool = False, coset: bool = False) -> list[int]:
        """fft / ifft / coset_fft / coset_ifft on Python ints: zero-pads or truncates to
        2^log_n exactly like Vec::resize at reference domain.rs:174."""
        n = 1 << log_n
        vals = list(values[:n])
        return fr_from_bytes_mont(self.ntt_bytes(fr_to_bytes_mont(vals), log_n, inverse, coset,
                                                 len(vals) if not inverse else n))

    # ---- CommitKey seam ------------------------------------------------------------
    def srs_load(self, points) -> None:
        raw = b"".join(g1_to_raw96(p) for p in points)
        self.srs_load_bytes(raw, len(points))

    def srs_load_bytes(self, raw: bytes, npoints: int) -> None:
        self._check(self.lib.plonk_srs_load(self.handle, raw, npoints))
        self.srs_points = npoints

    def srs_load_public_parameters(self, data: bytes, truncated_degree: int = 0, validate: bool = True,
                                   compressed: bool = False) -> bytes:
        """PublicParameters::from_slice_unchecked / CommitKey::from_raw_var_bytes / PublicParameters::from_slice (compressed)
        + trim(truncated_degree) straight into the context's window tables (plonk_srs_load_public_parameters); returns the
        240 opening-key bytes."""
        ok = ctypes.create_string_buffer(240)
        n = ctypes.c_uint64(0)
        self._check(self.lib.plonk_srs_load_public_parameters(self.handle, data, len(data), truncated_degree,
                                                              _pp_mode(validate, compressed), ok, ctypes.byref(n)))
        self.srs_points = n.value
        return ok.raw

    def srs_load_host_ptr(self, ptr: int, npoints: int) -> None:
        """plonk_srs_load from a raw host address (e.g. inside a PinnedBuffer): streamed in chunks."""
        self._check(self.lib.plonk_srs_load(self.handle, ctypes.c_void_p(ptr), npoints))
        self.srs_points = npoints

    def d2h_into(self, host_ptr: int, dev_ptr: int, nbytes: int) -> None:
        self._check(self.lib.plonk_dev_d2h(self.handle, ctypes.c_void_p(host_ptr), dev_ptr, nbytes))

    def h2d_from(self, dev_ptr: int, host_ptr: int, nbytes: int) -> None:
        """plonk_dev_h2d from a raw host address (e.g. PinnedBuffer.ptr); queued on the context's stream"""
        self._check(self.lib.plonk_dev_h2d(self.handle, dev_ptr, ctypes.c_void_p(host_ptr), nbytes))

    def msm_bytes(self, scalars_mont: bytes, m: int) -> bytes:
        out = ctypes.create_string_buffer(97)
        self._check(self.lib.plonk_msm(self.handle, scalars_mont, m, out))
        return out.raw

    def msm(self, scalars: Sequence[int]):
        """msm_variable_base(&powers_of_g, scalars) -> affine point or None (identity)."""
        return g1_from_raw97(self.msm_bytes(fr_to_bytes_mont(scalars), len(scalars)))

    @staticmethod
    def _msm_points_opts(compressed, check, window_bits, slice_entries, min_bucket_terms) -> "_MsmPointsOpts":
        return _MsmPointsOpts(flags=(POINTS_COMPRESSED if compressed else 0) | (POINTS_CHECK if check else 0),
                              window_bits=window_bits, slice_entries=slice_entries, min_bucket_terms=min_bucket_terms)

    def msm_points_bytes(self, points: bytes, scalars_mont: bytes, m: int, compressed: bool = False, check: bool = False,
                         window_bits: int = 0, slice_entries: int = 0, min_bucket_terms: int = 0) -> bytes:
        """plonk_msm_points on marshalled input: m x 96 (or m x 48 compressed) point bytes, m x 32 Montgomery scalar bytes ->
        the 97 result bytes"""
        opts = self._msm_points_opts(compressed, check, window_bits, slice_entries, min_bucket_terms)
        out = ctypes.create_string_buffer(97)
        self._check(self.lib.plonk_msm_points(self.handle, points, scalars_mont, m, ctypes.byref(opts), out))
        return out.raw

    def msm_points(self, points, scalars: Sequence[int], compressed: bool = False, check: bool = False, window_bits: int = 0,
                   slice_entries: int = 0, min_bucket_terms: int = 0):
        """msm_variable_base(points, scalars) over the CALLER's points -> affine point or None (identity), as msm().  points:
        affine pairs (None = the identity), or the marshalled bytes (m x 96 raw, m x 48 with compressed=True).  check=True
        tests every finite point for the curve and the subgroup (PointMalformed).  window_bits / slice_entries /
        min_bucket_terms force the plan (0 = automatic); last_msm_points() tells what ran."""
        m = len(scalars)
        if not isinstance(points, (bytes, bytearray)):
            assert len(points) == m
            if compressed:
                points = b"".join(g1_compress(p) for p in points)
            else:
                points = b"".join(bytes(96) if p is None else g1_to_raw96(p) for p in points)
        assert len(points) == (48 if compressed else 96) * m
        return g1_from_raw97(self.msm_points_bytes(bytes(points), fr_to_bytes_mont(scalars), m, compressed, check, window_bits,
                                                   slice_entries, min_bucket_terms))

    def msm_points_dev(self, points: int, scalars: int, m: int, out97: int, compressed: bool = False, check: bool = False,
                       window_bits: int = 0, slice_entries: int = 0, min_bucket_terms: int = 0):
        """plonk_msm_points_dev: device pointers to the points, the Montgomery scalars and the 97 output bytes"""
        opts = self._msm_points_opts(compressed, check, window_bits, slice_entries, min_bucket_terms)
        self._check(self.lib.plonk_msm_points_dev(self.handle, points, scalars, m, ctypes.byref(opts), out97))

    def last_msm_points(self) -> dict:
        """what the last msm_points / msm_points_dev call on this context ran as (plonk_msm_points_info)"""
        info = _MsmPointsInfo()
        self._check(self.lib.plonk_ctx_last_msm_points(self.handle, ctypes.byref(info)))
        return {k: getattr(info, k) for k, _ in info._fields_}

    def commit(self, coeffs: Sequence[int]):
        """CommitKey::commit (key.rs:376-388): trailing zeros trimmed like
        Polynomial::from_coefficients_vec; degree check before the MSM."""
        c = list(coeffs)
        while c and c[-1] % Q == 0:
            c.pop()
        if len(c) > self.srs_points:
            raise PolynomialDegreeTooLarge(-3)
        return self.msm(c)

    # ---- device-resident API ----------------------------------------------------
    def _kzg_open(self, fn, ptrs, lens, point, v, commitments):
        count = len(lens)
        parr = (ctypes.c_void_p * max(count, 1))(*ptrs)
        larr = (ctypes.c_uint64 * max(count, 1))(*lens)
        evals = ctypes.create_string_buffer(32 * max(count, 1))
        comms = ctypes.create_string_buffer(48 * max(count, 1)) if commitments else None
        wit = ctypes.create_string_buffer(48)
        vb = fr_to_bytes_mont([v]) if v is not None else None
        self._check(fn(self.handle, parr, larr, count, fr_to_bytes_mont([point]), vb, evals, comms, wit))
        return (fr_from_bytes_mont(evals.raw[:32 * count]),
                [comms.raw[48 * i:48 * i + 48] for i in range(count)] if commitments else None, wit.raw)

    def kzg_open(self, polys, point: int, v: "int | None" = None, commitments: bool = True):
        """plonk_kzg_open: open the polynomials (coefficient lists of ints, or Montgomery bytes) at `point` ->
        (evaluations, commitments or None, witness): p_i(point), the 48-byte commit(p_i), and the 48-byte commitment of
        (sum_i v^i p_i) / (X - point) — CommitKey::compute_aggregate_witness + commit (reference key.rs:394-417).  One
        polynomial is open_single (v may be None)."""
        bufs = [p if isinstance(p, (bytes, bytearray)) else fr_to_bytes_mont(p) for p in polys]
        keep = [ctypes.create_string_buffer(bytes(b), len(b)) if b else None for b in bufs]
        ptrs = [ctypes.cast(k, ctypes.c_void_p).value if k is not None else None for k in keep]
        return self._kzg_open(self.lib.plonk_kzg_open, ptrs, [len(b) // 32 for b in bufs], point, v, commitments)

    def kzg_open_dev(self, ptrs, lens, point: int, v: "int | None" = None, commitments: bool = True):
        """plonk_kzg_open_dev: the same for polynomials resident in HBM (device pointers, coefficients each)."""
        return self._kzg_open(self.lib.plonk_kzg_open_dev, list(ptrs), list(lens), point, v, commitments)

    def kzg_flatten(self, commitments, evaluations, v: int, witness: bytes) -> "KzgProof":
        """plonk_kzg_flatten = AggregateProof::flatten (reference proof.rs:69-109)."""
        out = KzgProof()
        self._check(self.lib.plonk_kzg_flatten(self.handle, b"".join(bytes(c) for c in commitments), fr_to_bytes_mont(evaluations),
                                               len(commitments), fr_to_bytes_mont([v]), bytes(witness), ctypes.byref(out)))
        return out

    def _verify_msm(self, points, scalars):
        """TEST HOOK: the device MSM of plonk_verify (verify.hip) on affine points (None = identity) and integer scalars;
        returns the affine sum.  Not part of the C API."""
        assert len(points) == len(scalars) and points
        comp = b"".join(g1_compress(p) for p in points)
        sc = b"".join((s % Q).to_bytes(32, "little") for s in scalars)
        out = ctypes.create_string_buffer(97)
        self._check(self.lib.plonk_test_verify_msm(self.handle, comp, sc, len(points), out))
        return g1_from_raw97(out.raw)

    def _verify_replay(self, items):
        """TEST HOOK: the device replay of plonk_verify_mixed (verify.hip) on items [(Verifier, proof, public_inputs)];
        returns per proof (status, 28 scalars as Montgomery bytes, 32-byte digest).  Not part of the C API."""
        args = _mixed_args(items)
        count = len(items)
        status = (ctypes.c_int32 * count)()
        scalars = ctypes.create_string_buffer(28 * 32 * count)
        digests = ctypes.create_string_buffer(32 * count)
        self._check(self.lib.plonk_test_verify_replay(*args, status, scalars, digests))
        raw = scalars.raw
        return [(int(status[k]), [raw[896 * k + 32 * j:896 * k + 32 * j + 32] for j in range(28)],
                 digests.raw[32 * k:32 * k + 32]) for k in range(count)]

    def alloc(self, nbytes: int) -> DeviceBuffer:
        return DeviceBuffer(self, nbytes)

    # ---- configuration / introspection ----------------------------------------------------
    def get_config(self) -> "GpuConfig":
        """the EFFECTIVE configuration (defaults and environment overrides resolved)"""
        g = GpuConfig()
        self._check(self.lib.plonk_ctx_get_config(self.handle, ctypes.byref(g)))
        return g

    def set_config(self, config: "GpuConfig"):
        self._check(self.lib.plonk_ctx_set_config(self.handle, ctypes.byref(config)))

    def describe_msm(self, m: int, count: int = 1, bit_sum_tail: bool = True, table_rows: int = 0, table_points: int = 0) -> dict:
        """what an MSM of `count` sets of <= m terms would run as (table_rows = 0: over the context's commit key)"""
        p = _MsmPlan()
        self._check(self.lib.plonk_ctx_describe_msm(self.handle, m, count, int(bit_sum_tail), table_rows, table_points, ctypes.byref(p)))
        return p.as_dict()

    def last_msm(self) -> dict:
        """what the last MSM group on this context did run as"""
        p = _MsmPlan()
        self._check(self.lib.plonk_ctx_last_msm(self.handle, ctypes.byref(p)))
        return p.as_dict()

    def table_bytes(self) -> tuple[int, int]:
        """(bytes of point tables the context holds, its budget)"""
        a, b = ctypes.c_uint64(0), ctypes.c_uint64(0)
        self._check(self.lib.plonk_ctx_table_bytes(self.handle, ctypes.byref(a), ctypes.byref(b)))
        return a.value, b.value

    def table_rows(self) -> int:
        """256: one table row per bit position (width-17 NAF digits), 128 / 64: a row for every second / fourth position, 16: window rows, 0: no key"""
        return int(self.lib.plonk_ctx_table_rows(self.handle))

    def ntt_dev(self, src: int, dst: int, tmp: int, log_n: int, inverse=False, coset=False, in_len=None):
        in_len = (1 << log_n) if in_len is None else in_len
        self._check(self.lib.plonk_ntt_dev(self.handle, src, dst, tmp, log_n, int(inverse), int(coset), in_len))

    def msm_dev(self, scalars: int, m: int, out97: int):
        self._check(self.lib.plonk_msm_dev(self.handle, scalars, m, out97))

    def srs_load_dev(self, ptr: int, npoints: int):
        self._check(self.lib.plonk_srs_load_dev(self.handle, ptr, npoints))
        self.srs_points = npoints

    def srs_generate_dev(self, tau: int, g_scalar: int, npoints: int, out_ptr: int):
        self._check(self.lib.plonk_srs_generate_dev(self.handle, fr_to_bytes_mont([tau]),
                                                    fr_to_bytes_mont([g_scalar]), npoints, out_ptr))

    def lagrange_key(self, log_n: int) -> bytes:
        """(n + 2) x 96 B: [L_i(tau)] G and the two blinding points, from the context's commit key (plonk_lagrange_key)."""
        out = ctypes.create_string_buffer(96 * ((1 << log_n) + 2))
        self._check(self.lib.plonk_lagrange_key(self.handle, log_n, out))
        return out.raw

    def sync(self):
        self._check(self.lib.plonk_dev_sync(self.handle))

    # ---- multi-GPU (RCCL inside the library) -----------------------------------------------
    @staticmethod
    def comm_unique_id() -> bytes:
        """ncclGetUniqueId on rank 0; hand the 128 bytes to the other ranks out of band."""
        lib = load_library()
        out = ctypes.create_string_buffer(128)
        rc = lib.plonk_comm_unique_id(out)
        if rc != PLONK_OK:
            raise PlonkError(rc, (lib.plonk_last_error() or b"").decode())
        return out.raw

    @staticmethod
    def comm_set_library(path: str):
        """Name the transport library (default: librccl) before the first communicator call of the process."""
        lib = load_library()
        rc = lib.plonk_comm_set_library(os.fsencode(path))
        if rc != PLONK_OK:
            raise PlonkError(rc, (lib.plonk_last_error() or b"").decode())

    @staticmethod
    def comm_library() -> str:
        """Path of the transport library that was actually loaded (dladdr of its ncclAllGather)."""
        lib = load_library()
        out = ctypes.create_string_buffer(1024)
        rc = lib.plonk_comm_library(out, 1024)
        if rc != PLONK_OK:
            raise PlonkError(rc, (lib.plonk_last_error() or b"").decode())
        return out.value.decode()

    def comm_init(self, unique_id: bytes, rank: int, world: int):
        assert len(unique_id) == 128
        self._check(self.lib.plonk_comm_init(self.handle, unique_id, rank, world))

    def comm_info(self) -> tuple[int, int]:
        """(rank, size) as the RCCL communicator reports them"""
        r, w = ctypes.c_int(-1), ctypes.c_int(-1)
        self._check(self.lib.plonk_comm_info(self.handle, ctypes.byref(r), ctypes.byref(w)))
        return r.value, w.value

    def comm_warning(self) -> str:
        """The note plonk_comm_init left on this context ("" = none); a successful call never writes the last-error text."""
        out = ctypes.create_string_buffer(512)
        self._check(self.lib.plonk_comm_warning(self.handle, out, 512))
        return out.value.decode()

    def comm_selftest(self):
        self._check(self.lib.plonk_comm_selftest(self.handle))

    def comm_destroy(self):
        self._check(self.lib.plonk_comm_destroy(self.handle))

    def comm_measure_loopback(self, on: bool = True):
        """MEASUREMENT ONLY (tools/rank_alone.py): collectives of this context return the rank's own contribution."""
        self._check(self.lib.plonk_comm_measure_loopback(self.handle, int(on)))

    def profile(self, on: bool):
        self._check(self.lib.plonk_profile_enable(self.handle, int(on)))

    def profile_reset(self):
        self._check(self.lib.plonk_profile_reset(self.handle))

    def profile_read(self, slot: int):
        ms, n = ctypes.c_double(), ctypes.c_uint64()
        self._check(self.lib.plonk_profile_read(self.handle, slot, ctypes.byref(ms), ctypes.byref(n)))
        return ms.value, n.value


# kinds of plonk_composer_gadget (enum plonk_gadget of include/plonk_hip.h, in its order)
GADGETS = ["CONSTANT", "PUBLIC", "ASSERT_EQUAL", "ASSERT_EQUAL_CONSTANT", "BOOLEAN", "SELECT", "SELECT_ONE", "SELECT_ZERO",
           "DECOMPOSITION", "RANGE_BITS", "RANGE", "TRUNCATE", "BIND_TRUNCATION_SPLIT", "CANONICAL_TRUNCATION", "LOGIC_AND",
           "LOGIC_XOR", "POINT", "CONSTANT_POINT", "PUBLIC_POINT", "ASSERT_EQUAL_POINT", "ASSERT_EQUAL_PUBLIC_POINT", "NEG_POINT",
           "SUB_POINT", "ADD_POINT", "SELECT_IDENTITY", "SELECT_POINT", "TORSION_FREE", "CANONICAL_JUBJUB_SCALAR", "MUL_GENERATOR",
           "MUL_POINT"]
G = {name: k for k, name in enumerate(GADGETS)}


class Composer:
    """Records a circuit from gadgets (plonk_composer_*): one method per gadget of the reference's Composer, returning
    witness indices — pairs (x, y) for points.  ZERO / ONE / IDENTITY are the constants of Composer::initialized.
    Values are not given here: append_witness allocates an INPUT, and Prover.fill_inputs / prove_inputs take the input
    values of one proof in allocation order."""
    ZERO, ONE = 0, 1
    IDENTITY = (0, 1)

    def __init__(self):
        self.lib = load_library()
        h = ctypes.c_void_p()
        self._check(self.lib.plonk_composer_create(ctypes.byref(h)))
        self.handle = h

    def _check(self, rc):
        if rc == -10:
            raise PointMalformed(rc, (self.lib.plonk_last_error() or b"").decode())
        if rc != PLONK_OK:
            raise PlonkError(rc, (self.lib.plonk_last_error() or b"").decode())

    def close(self):
        if getattr(self, "handle", None):
            self.lib.plonk_composer_destroy(self.handle)
            self.handle = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    # ---- the three recording calls
    def append_witness(self) -> int:
        out = ctypes.c_uint32()
        self._check(self.lib.plonk_composer_witness(self.handle, ctypes.byref(out)))
        return out.value

    def append_gate(self, a=0, b=0, c=0, d=0, q_m=0, q_l=0, q_r=0, q_o=0, q_f=0, q_c=0, public=False, evaluate=False):
        """one arithmetic gate; evaluate: solve it for c, allocate c and return its index (append_evaluated_output)"""
        sel = fr_to_bytes_mont([q_m, q_l, q_r, q_o, q_f, q_c])
        wires = (ctypes.c_uint32 * 4)(a, b, c, d)
        out = ctypes.c_uint32()
        self._check(self.lib.plonk_composer_gate(self.handle, sel, wires, (1 if public else 0) | (2 if evaluate else 0), ctypes.byref(out)))
        return out.value if evaluate and out.value != 0xFFFFFFFF else None

    def gadget(self, kind: str, ins=(), width: int = 0, consts=(), nout: int = 0):
        arr = (ctypes.c_uint32 * max(len(ins), 1))(*ins)
        cst = fr_to_bytes_mont(consts)
        out = (ctypes.c_uint32 * max(nout, 1))()
        got = ctypes.c_uint32()
        self._check(self.lib.plonk_composer_gadget(self.handle, G[kind], width, arr, len(ins), cst, len(consts), out, nout, ctypes.byref(got)))
        assert got.value == nout, (kind, got.value, nout)
        return list(out[:nout])

    # ---- composer basics
    def append_evaluated_output(self, **kw):
        return self.append_gate(evaluate=True, **kw)

    def gate_add(self, a, b, d=0, q_l=1, q_r=1, q_f=0, q_c=0):
        return self.append_gate(a=a, b=b, d=d, q_l=q_l, q_r=q_r, q_f=q_f, q_c=q_c, q_o=Q - 1, evaluate=True)

    def gate_mul(self, a, b, d=0, q_m=1, q_f=0, q_c=0):
        return self.append_gate(a=a, b=b, d=d, q_m=q_m, q_f=q_f, q_c=q_c, q_o=Q - 1, evaluate=True)

    def append_constant(self, value: int) -> int:
        return self.gadget("CONSTANT", consts=[value], nout=1)[0]

    def append_public(self) -> int:
        return self.gadget("PUBLIC", nout=1)[0]

    def assert_equal(self, a, b):
        self.gadget("ASSERT_EQUAL", [a, b])

    def assert_equal_constant(self, a, constant: int, public: bool = False):
        self.gadget("ASSERT_EQUAL_CONSTANT", [a], width=1 if public else 0, consts=[constant])

    # ---- bits and selection
    def component_boolean(self, a):
        self.gadget("BOOLEAN", [a])

    def component_select(self, bit, a, b) -> int:
        return self.gadget("SELECT", [bit, a, b], nout=1)[0]

    def component_select_one(self, bit, value) -> int:
        return self.gadget("SELECT_ONE", [bit, value], nout=1)[0]

    def component_select_zero(self, bit, value) -> int:
        return self.gadget("SELECT_ZERO", [bit, value], nout=1)[0]

    def component_decomposition(self, scalar, n: int) -> list:
        return self.gadget("DECOMPOSITION", [scalar], width=n, nout=n)

    # ---- range and truncation
    def component_range_bits(self, w, bits: int):
        self.gadget("RANGE_BITS", [w], width=bits)

    def component_range(self, w, bit_pairs: int):
        self.gadget("RANGE", [w], width=bit_pairs)

    def component_truncate(self, w, n: int) -> int:
        return self.gadget("TRUNCATE", [w], width=n, nout=1)[0]

    def bind_truncation_split(self, input_w, low, num_bits: int):
        self.gadget("BIND_TRUNCATION_SPLIT", [input_w, low], width=num_bits)

    def assert_canonical_truncation(self, high, low, num_bits: int):
        self.gadget("CANONICAL_TRUNCATION", [high, low], width=num_bits)

    # ---- logic
    def append_logic_and(self, a, b, bit_pairs: int) -> int:
        return self.gadget("LOGIC_AND", [a, b], width=bit_pairs, nout=1)[0]

    def append_logic_xor(self, a, b, bit_pairs: int) -> int:
        return self.gadget("LOGIC_XOR", [a, b], width=bit_pairs, nout=1)[0]

    # ---- points
    def append_point(self):
        return tuple(self.gadget("POINT", nout=2))

    def append_constant_point(self, point):
        return tuple(self.gadget("CONSTANT_POINT", consts=list(point), nout=2))

    def append_public_point(self):
        return tuple(self.gadget("PUBLIC_POINT", nout=2))

    def assert_equal_point(self, a, b):
        self.gadget("ASSERT_EQUAL_POINT", [*a, *b])

    def assert_equal_public_point(self, point):
        self.gadget("ASSERT_EQUAL_PUBLIC_POINT", list(point))

    def component_neg_point(self, p):
        return tuple(self.gadget("NEG_POINT", list(p), nout=2))

    def component_sub_point(self, a, b):
        return tuple(self.gadget("SUB_POINT", [*a, *b], nout=2))

    def component_add_point(self, a, b):
        return tuple(self.gadget("ADD_POINT", [*a, *b], nout=2))

    def component_select_identity(self, bit, a):
        return tuple(self.gadget("SELECT_IDENTITY", [bit, *a], nout=2))

    def component_select_point(self, bit, a, b):
        return tuple(self.gadget("SELECT_POINT", [bit, *a, *b], nout=2))

    def assert_torsion_free_point(self, p):
        self.gadget("TORSION_FREE", list(p))
        return tuple(p)

    # ---- scalar multiplication
    def assert_canonical_jubjub_scalar(self, s):
        self.gadget("CANONICAL_JUBJUB_SCALAR", [s])

    def component_mul_generator(self, s, generator):
        return tuple(self.gadget("MUL_GENERATOR", [s], consts=list(generator), nout=2))

    def component_mul_point(self, s, p):
        return tuple(self.gadget("MUL_POINT", [s, *p], nout=2))

    # ---- inspection
    def info(self) -> dict:
        out = _ComposerSummary()
        self._check(self.lib.plonk_composer_info(self.handle, ctypes.byref(out)))
        return {k: getattr(out, k) for k, _ in out._fields_}

    def layout(self) -> dict:
        """what plonk_compile would be given: selectors {name: Montgomery bytes}, wires (4 lists), witnesses, plus the witness
        slot of every input and the public-input rows"""
        info = self.info()
        n = info["constraints"]
        sels = [ctypes.create_string_buffer(max(32 * n, 1)) for _ in range(11)]
        wires = [(ctypes.c_uint32 * max(n, 1))() for _ in range(4)]
        sp = (ctypes.c_void_p * 11)(*[ctypes.cast(b, ctypes.c_void_p) for b in sels])
        wp = (ctypes.c_void_p * 4)(*[ctypes.cast(b, ctypes.c_void_p) for b in wires])
        slots = (ctypes.c_uint32 * max(info["inputs"], 1))()
        rows = (ctypes.c_uint64 * max(info["public_rows"], 1))()
        self._check(self.lib.plonk_composer_layout(self.handle, sp, wp, slots, rows))
        return {"selectors": {name: sels[k].raw[:32 * n] for k, name in enumerate(POLY_ORDER[:11])},
                "wires": [list(w[:n]) for w in wires], "witnesses": info["witnesses"],
                "input_slots": list(slots[:info["inputs"]]), "pi_rows": list(rows[:info["public_rows"]])}


class Prover:
    """Device-resident mirror of the reference `Prover` (src/compiler/prover.rs:27-42):
    built from the 15 ProverKey polynomials + label + constraint count; `prove` takes the
    padded wire columns, sparse public inputs and the 14 blinders drawn by the caller's RNG
    (prover.rs:154-161,133-135,553-555) and returns Proof::to_bytes (1008 bytes)."""

    def __init__(self, ctx: Context, constraints: int, label: bytes, polys: dict, vk_commitments: bytes | None = None,
                 rank: int = 0, world: int = 1, srs_total: int = 0, allgather=None, lagrange_slice: bytes | None = None):
        """allgather(send: bytes) -> bytes (rank-major concatenation) when world > 1 and the context has no RCCL
        communicator; lagrange_slice: this rank's points of Context.lagrange_key (multi-GPU)."""
        self.ctx = ctx
        desc = _ProverDesc()
        self._shard(desc, rank, world, srs_total, allgather, lagrange_slice)
        desc.constraints = constraints
        desc.label = label
        desc.label_len = len(label)
        self._keep = []
        for k, name in enumerate(POLY_ORDER):
            coeffs = polys.get(name, [])
            raw = coeffs if isinstance(coeffs, (bytes, bytearray)) else fr_to_bytes_mont(coeffs)
            buf = ctypes.create_string_buffer(bytes(raw), max(len(raw), 1))
            self._keep.append(buf)
            desc.polys[k] = ctypes.cast(buf, ctypes.c_void_p)
            desc.poly_len[k] = len(raw) // 32
        desc.vk_commitments = vk_commitments
        h = ctypes.c_void_p()
        ctx._check(ctx.lib.plonk_prover_create(ctx.handle, ctypes.byref(desc), ctypes.byref(h)))
        self.handle = h
        ctx._provers.add(self)
        self.size = ctx.lib.plonk_prover_size(h)
        self._keep = None

    def describe(self) -> dict:
        """what the prover was built as (plonk_prover_describe): quotient domain, wire-commitment mode, sharding"""
        info = _ProverInfo()
        self.ctx._check(self.ctx.lib.plonk_prover_describe(self.handle, ctypes.byref(info)))
        return {k: getattr(info, k) for k, _ in info._fields_ if k != "reserved"}

    @classmethod
    def from_bytes(cls, ctx: Context, blob: bytes) -> "Prover":
        """Prover::try_from_bytes (reference prover.rs:266-345) on the output of the reference's
        Prover::to_bytes(): validates the blob, loads its commit key into `ctx` and builds the device
        prover.  Raises NotEnoughBytes / InvalidData / PointMalformed like the reference."""
        self = cls.__new__(cls)
        self.ctx, self._cb, self._keep = ctx, None, None
        h = ctypes.c_void_p()
        ctx._check(ctx.lib.plonk_prover_from_bytes(ctx.handle, blob, len(blob), ctypes.byref(h)))
        self.handle = h
        ctx._provers.add(self)
        self.size = ctx.lib.plonk_prover_size(h)
        return self

    def _shard(self, desc, rank, world, srs_total, allgather, lagrange_slice):
        self._cb = None
        if world > 1:
            desc.shard_rank, desc.shard_world, desc.srs_total = rank, world, srs_total
        if world > 1 and allgather is not None:
            def _cb(user, send, recv, nbytes):
                try:
                    out = allgather(ctypes.string_at(send, nbytes))
                    assert len(out) == nbytes * world
                    ctypes.memmove(recv, out, len(out))
                    return 0
                except Exception:   # never unwind through the C frame
                    import traceback
                    traceback.print_exc()
                    return 1
            self._cb = ALLGATHER_FN(_cb)
            desc.allgather = ctypes.cast(self._cb, ctypes.c_void_p)
        if lagrange_slice is not None:   # an empty slice still selects the mode (every rank must take the same one)
            desc.lagrange_xy96 = lagrange_slice if lagrange_slice else b"\0"
            desc.lagrange_count = len(lagrange_slice) // 96

    @classmethod
    def compile(cls, ctx: Context, label: bytes, selectors: dict, wires, witnesses: int, rank: int = 0, world: int = 1,
                srs_total: int = 0, allgather=None, lagrange_slice: bytes | None = None) -> "Prover":
        """Compiler::preprocess (reference src/compiler.rs:132-461) on the device.  selectors: {name: per-gate values},
        names from POLY_ORDER[:11], values as ints or Montgomery bytes, missing = zero; wires: four sequences of witness
        indices (one per gate); witnesses: how many witnesses the composer allocated."""
        self = cls.__new__(cls)
        self.ctx, self._keep = ctx, []
        desc = _CircuitDesc()
        self._shard(desc, rank, world, srs_total, allgather, lagrange_slice)
        def u32_bytes(w):   # list of ints, raw little-endian uint32 bytes, or anything with tobytes() (a uint32 array)
            if isinstance(w, (bytes, bytearray)):
                return bytes(w)
            if hasattr(w, "tobytes"):
                assert getattr(w, "itemsize", 4) == 4
                return w.tobytes()
            return bytes((ctypes.c_uint32 * len(w))(*w))
        wire_raw = [u32_bytes(w) for w in wires]
        constraints = len(wire_raw[0]) // 4
        desc.constraints, desc.label, desc.label_len, desc.witnesses = constraints, label, len(label), witnesses
        for k, name in enumerate(POLY_ORDER[:11]):
            col = selectors.get(name)
            if col is None or len(col) == 0:
                continue
            raw = bytes(col) if isinstance(col, (bytes, bytearray)) else fr_to_bytes_mont(col)
            assert len(raw) == 32 * constraints, name
            self._keep.append(raw)   # the library reads the bytes object in place
            desc.selectors[k] = ctypes.cast(ctypes.c_char_p(raw), ctypes.c_void_p)
        for w in range(4):
            assert len(wire_raw[w]) == 4 * constraints
            desc.wires[w] = ctypes.cast(ctypes.c_char_p(wire_raw[w]), ctypes.c_void_p)
        h = ctypes.c_void_p()
        ctx._check(ctx.lib.plonk_compile(ctx.handle, ctypes.byref(desc), ctypes.byref(h)))
        self.handle = h
        ctx._provers.add(self)
        self.size = ctx.lib.plonk_prover_size(h)
        self._keep = None
        return self

    def prove_witnesses(self, witnesses, public_inputs, blinders) -> bytes:
        """Proof from the witness values (ints or Montgomery bytes) on a compiled prover (prover.rs:446-460 on the device)."""
        raw = bytes(witnesses) if isinstance(witnesses, (bytes, bytearray)) else fr_to_bytes_mont(witnesses)
        bl = bytes(blinders) if isinstance(blinders, (bytes, bytearray)) else fr_to_bytes_mont(blinders)
        assert len(bl) == 14 * 32
        idx, val, cnt = self._pi(public_inputs)
        proof = ctypes.create_string_buffer(1008)
        self.ctx._check(self.ctx.lib.plonk_prover_prove_witnesses(self.handle, raw, len(raw) // 32, idx, val, cnt, bl, proof))
        return proof.raw

    def prove_witnesses_ptr(self, values_ptr: int, count: int, public_inputs, blinders_mont: bytes) -> bytes:
        """prove_witnesses on a raw host address (e.g. PinnedBuffer.ptr) holding count x 32 bytes."""
        idx, val, cnt = self._pi(public_inputs)
        proof = ctypes.create_string_buffer(1008)
        self.ctx._check(self.ctx.lib.plonk_prover_prove_witnesses(self.handle, values_ptr, count, idx, val, cnt, blinders_mont, proof))
        return proof.raw

    def to_bytes(self) -> bytes:
        """Prover::to_bytes() (reference prover.rs:238-263) of this prover and its context's commit key."""
        n = ctypes.c_uint64()
        self.ctx._check(self.ctx.lib.plonk_prover_to_bytes(self.handle, None, 0, ctypes.byref(n)))
        buf = ctypes.create_string_buffer(n.value)
        self.ctx._check(self.ctx.lib.plonk_prover_to_bytes(self.handle, buf, n.value, ctypes.byref(n)))
        return buf.raw

    def verifier_to_bytes(self, opening_key: bytes, public_input_indexes) -> bytes:
        """Verifier::to_bytes() (reference verifier.rs:88-117); opening_key = OpeningKey::to_bytes() of the caller's parameters."""
        idx = list(public_input_indexes)
        arr = (ctypes.c_uint64 * max(len(idx), 1))(*idx)
        n = ctypes.c_uint64()
        self.ctx._check(self.ctx.lib.plonk_verifier_to_bytes(self.handle, opening_key, len(opening_key), arr, len(idx), None, 0, ctypes.byref(n)))
        buf = ctypes.create_string_buffer(n.value)
        self.ctx._check(self.ctx.lib.plonk_verifier_to_bytes(self.handle, opening_key, len(opening_key), arr, len(idx), buf, n.value, ctypes.byref(n)))
        return buf.raw

    def vk_commitments(self) -> bytes:
        out = ctypes.create_string_buffer(15 * 48)
        self.ctx._check(self.ctx.lib.plonk_prover_vk(self.handle, out))
        return out.raw

    @staticmethod
    def _pi(public_inputs):
        items = sorted(public_inputs.items()) if isinstance(public_inputs, dict) else list(public_inputs or [])
        idx = (ctypes.c_uint64 * max(len(items), 1))(*[i for i, _ in items])
        val = fr_to_bytes_mont([v for _, v in items])
        return idx, val, len(items)

    def prove(self, wires, public_inputs, blinders) -> bytes:
        """wires: 4 sequences of ints (length <= size, zero padded); blinders: 14 ints."""
        assert len(blinders) == 14
        n = self.size
        bufs = []
        for w in wires:
            raw = w if isinstance(w, (bytes, bytearray)) else fr_to_bytes_mont(list(w) + [0] * (n - len(w)))
            assert len(raw) == 32 * n
            bufs.append(ctypes.create_string_buffer(bytes(raw), len(raw)))
        arr = (ctypes.c_void_p * 4)(*[ctypes.cast(b, ctypes.c_void_p) for b in bufs])
        idx, val, cnt = self._pi(public_inputs)
        proof = ctypes.create_string_buffer(1008)
        self.ctx._check(self.ctx.lib.plonk_prover_prove(self.handle, arr, idx, val, cnt,
                                                        fr_to_bytes_mont(blinders), proof))
        return proof.raw

    def prove_host_bytes(self, wires, public_inputs, blinders_mont: bytes) -> bytes:
        """plonk_prover_prove on four byte strings of size x 32 B (pageable host memory), blinders as Montgomery bytes"""
        n = self.size
        assert all(len(w) == 32 * n for w in wires)
        bufs = [ctypes.create_string_buffer(bytes(w), 32 * n) for w in wires]
        return self.prove_host_ptrs([ctypes.addressof(b) for b in bufs], public_inputs, blinders_mont)

    def prove_host_ptrs(self, wire_ptrs, public_inputs, blinders_mont: bytes) -> bytes:
        """plonk_prover_prove on four raw host addresses (e.g. PinnedBuffer.ptr): the columns are uploaded on the copy
        stream while round 1 already transforms the ones that have arrived."""
        arr = (ctypes.c_void_p * 4)(*[ctypes.c_void_p(p) for p in wire_ptrs])
        idx, val, cnt = self._pi(public_inputs)
        proof = ctypes.create_string_buffer(1008)
        self.ctx._check(self.ctx.lib.plonk_prover_prove(self.handle, arr, idx, val, cnt, blinders_mont, proof))
        return proof.raw

    def set_version(self, version: int):
        """Prover::prove_with_version (prover.rs:365-413): 3 (default) or the legacy 2 (transcript seeding only)."""
        self.ctx._check(self.ctx.lib.plonk_prover_set_version(self.handle, version))

    def prove_dev(self, wires_ptr: int, public_inputs, blinders_mont: bytes) -> bytes:
        idx, val, cnt = self._pi(public_inputs)
        proof = ctypes.create_string_buffer(1008)
        self.ctx._check(self.ctx.lib.plonk_prover_prove_dev(self.handle, wires_ptr, idx, val, cnt,
                                                            blinders_mont, proof))
        return proof.raw

    # ---- witness diagnosis (plonk_prover_diagnose*): which rows fail which identity family / copy constraint
    def _diagnose(self, call, cap: int) -> Diagnosis:
        out = (_UnsatRow * cap)() if cap else None
        info = _UnsatInfo()
        rc = call(out, cap, ctypes.byref(info))
        if rc not in (PLONK_OK, -6):
            self.ctx._check(rc)
        got = min(cap, info.rows_failing)
        return Diagnosis(rc, [(out[i].row, out[i].families, out[i].copy_wires) for i in range(got)], info)

    def diagnose(self, wires, public_inputs=None, cap: int = 64) -> Diagnosis:
        """wires: 4 sequences of ints (length <= size, zero padded) or of size x 32 Montgomery bytes."""
        n = self.size
        bufs = []
        for w in wires:
            raw = w if isinstance(w, (bytes, bytearray)) else fr_to_bytes_mont(list(w) + [0] * (n - len(w)))
            assert len(raw) == 32 * n
            bufs.append(ctypes.create_string_buffer(bytes(raw), len(raw)))
        arr = (ctypes.c_void_p * 4)(*[ctypes.cast(b, ctypes.c_void_p) for b in bufs])
        idx, val, cnt = self._pi(public_inputs)
        return self._diagnose(lambda out, c, info: self.ctx.lib.plonk_prover_diagnose(self.handle, arr, idx, val, cnt, out, c, info), cap)

    def diagnose_dev(self, wires_ptr: int, public_inputs=None, cap: int = 64) -> Diagnosis:
        """the 4 x size wire columns already resident in HBM (contiguous a|b|c|d), as prove_dev takes them"""
        idx, val, cnt = self._pi(public_inputs)
        return self._diagnose(lambda out, c, info: self.ctx.lib.plonk_prover_diagnose_dev(self.handle, wires_ptr, idx, val, cnt, out, c, info), cap)

    def diagnose_witnesses(self, values, public_inputs=None, cap: int = 64) -> Diagnosis:
        """from the witness values (ints or Montgomery bytes) on a compiled prover, as prove_witnesses takes them"""
        raw = bytes(values) if isinstance(values, (bytes, bytearray)) else fr_to_bytes_mont(values)
        idx, val, cnt = self._pi(public_inputs)
        return self._diagnose(lambda out, c, info: self.ctx.lib.plonk_prover_diagnose_witnesses(self.handle, raw, len(raw) // 32, idx, val, cnt, out, c, info), cap)

    # ---- circuits from gadgets (plonk_compile_composer, plonk_prover_*_inputs): the witness table is filled on the device
    @classmethod
    def compile_composer(cls, ctx: Context, label: bytes, composer: "Composer") -> "Prover":
        """plonk_compile on the composer's layout with its witness program attached; the composer may be closed afterwards"""
        self = cls.__new__(cls)
        self.ctx, self._keep, self._cb = ctx, None, None
        h = ctypes.c_void_p()
        ctx._check(ctx.lib.plonk_compile_composer(ctx.handle, composer.handle, label, len(label), ctypes.byref(h)))
        self.handle = h
        ctx._provers.add(self)
        self.size = ctx.lib.plonk_prover_size(h)
        info = composer.info()
        self.composer_counts = (info["witnesses"], info["public_rows"])
        return self

    def fill_inputs(self, inputs, want_witnesses: bool = True):
        """runs the witness program: (witness table as Montgomery bytes or None, public-input values as ints)"""
        raw = bytes(inputs) if isinstance(inputs, (bytes, bytearray)) else fr_to_bytes_mont(inputs)
        nw, npi = self.composer_counts
        wit = ctypes.create_string_buffer(max(32 * nw, 1)) if want_witnesses else None
        pi = ctypes.create_string_buffer(max(32 * npi, 1))
        self.ctx._check(self.ctx.lib.plonk_prover_fill_inputs(self.handle, raw, len(raw) // 32, wit, pi))
        return (wit.raw[:32 * nw] if want_witnesses else None), fr_from_bytes_mont(pi.raw[:32 * npi])

    def prove_inputs(self, inputs, blinders):
        """(proof bytes, public-input values) from the circuit's input values"""
        raw = bytes(inputs) if isinstance(inputs, (bytes, bytearray)) else fr_to_bytes_mont(inputs)
        bl = bytes(blinders) if isinstance(blinders, (bytes, bytearray)) else fr_to_bytes_mont(blinders)
        assert len(bl) == 14 * 32
        npi = self.composer_counts[1]
        pi = ctypes.create_string_buffer(max(32 * npi, 1))
        proof = ctypes.create_string_buffer(1008)
        self.ctx._check(self.ctx.lib.plonk_prover_prove_inputs(self.handle, raw, len(raw) // 32, bl, proof, pi))
        return proof.raw, fr_from_bytes_mont(pi.raw[:32 * npi])

    def diagnose_inputs(self, inputs, cap: int = 64) -> Diagnosis:
        raw = bytes(inputs) if isinstance(inputs, (bytes, bytearray)) else fr_to_bytes_mont(inputs)
        return self._diagnose(lambda out, c, info: self.ctx.lib.plonk_prover_diagnose_inputs(self.handle, raw, len(raw) // 32, out, c, info), cap)

    def peek(self, which: int, offset: int, count: int) -> list[int]:
        out = ctypes.create_string_buffer(32 * count)
        self.ctx._check(self.ctx.lib.plonk_prover_peek(self.handle, which, offset, count, out))
        return fr_from_bytes_mont(out.raw)

    def close(self):
        if getattr(self, "handle", None):
            if getattr(self.ctx, "handle", None):          # a closed context already destroyed its provers
                self.ctx.lib.plonk_prover_destroy(self.handle)
            self.handle = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


class Verifier:
    """The reference's `Verifier` (src/compiler/verifier.rs): built from Verifier::to_bytes() (plonk_verifier_from_bytes;
    raises NotEnoughBytes / InvalidData like try_from_bytes).  `verify` checks one proof, `verify_batch` a batch of proofs
    of this circuit in one aggregated pairing check (plonk_verify).  Destroyed before its context, like a prover."""

    def __init__(self, ctx: Context, blob: bytes):
        self.ctx = ctx
        h = ctypes.c_void_p()
        ctx._check(ctx.lib.plonk_verifier_from_bytes(ctx.handle, blob, len(blob), ctypes.byref(h)))
        self.handle = h
        ctx._provers.add(self)

    def set_version(self, version: int):
        """3 (default, PlonkVersion::V3) or the legacy 2 transcript seeding."""
        self.ctx._check(self.ctx.lib.plonk_verifier_set_version(self.handle, version))

    def _call(self, proofs, pis):
        proofs = list(proofs)
        pis = [list(p) for p in pis]
        if len(proofs) != len(pis):
            raise ValueError("one public-input list per proof")
        count = len(proofs)
        npi = len(pis[0]) if pis else 0
        if any(len(p) != npi for p in pis):
            raise ValueError("every proof needs the same number of public inputs")
        blob = b"".join(bytes(p) for p in proofs)
        if any(len(p) != 1008 for p in proofs):
            raise ValueError("a proof is 1008 bytes")
        pi = fr_to_bytes_mont([v for p in pis for v in p])
        verdicts = (ctypes.c_int32 * max(count, 1))()
        rc = self.ctx.lib.plonk_verify(self.handle, blob, pi if npi else None, npi, count, verdicts)
        return rc, [int(v) for v in verdicts[:count]]

    def verify(self, proof: bytes, public_inputs) -> bool:
        """Verifier::verify: True for a valid proof, False for PLONK_ERR_VERIFY / _DATA / _POINT; public_inputs in the
        verifier's index order.  Raises on argument errors (e.g. PLONK_ERR_ARG for the wrong number of inputs)."""
        rc, verdicts = self._call([proof], [public_inputs])
        if rc not in (PLONK_OK, -12):
            self.ctx._check(rc)
        return rc == PLONK_OK

    def verify_batch(self, proofs, public_inputs) -> list:
        """per-proof verdict codes (0 = valid, -12 PLONK_ERR_VERIFY, -9 PLONK_ERR_DATA, -10 PLONK_ERR_POINT)"""
        if not proofs:
            raise ValueError("empty batch")
        rc, verdicts = self._call(proofs, public_inputs)
        if rc not in (PLONK_OK, -12):
            self.ctx._check(rc)
        return verdicts

    def verify_each(self, proofs, public_inputs) -> list:
        """plonk_verify_each with circuit == NULL: every proof of this circuit checked on its own, one pairing per proof
        on the device; per-proof verdict codes as verify_batch, at a cost that does not depend on how many are bad."""
        proofs, pis = [bytes(p) for p in proofs], [list(p) for p in public_inputs]
        if not proofs or len(proofs) != len(pis):
            raise ValueError("a non-empty batch with one public-input list per proof")
        if any(len(p) != 1008 for p in proofs):
            raise ValueError("a proof is 1008 bytes")
        flat = [v for p in pis for v in p]
        handles = (ctypes.c_void_p * 1)(self.handle)
        verdicts = (ctypes.c_int32 * len(proofs))()
        rc = self.ctx.lib.plonk_verify_each(handles, 1, None, b"".join(proofs), fr_to_bytes_mont(flat) if flat else None, len(flat),
                                            len(proofs), verdicts, None)
        if rc not in (PLONK_OK, -12):
            self.ctx._check(rc)
        return [int(v) for v in verdicts]

    def last(self) -> dict:
        """plonk_verifier_last: what the last verification ran (proofs, msm_terms, pairing_checks, rejected, phase times)"""
        info = _VerifyInfo()
        self.ctx._check(self.ctx.lib.plonk_verifier_last(self.handle, ctypes.byref(info)))
        return {k: getattr(info, k) for k, _ in info._fields_}

    def close(self):
        if getattr(self, "handle", None):
            if getattr(self.ctx, "handle", None):
                self.ctx.lib.plonk_verifier_destroy(self.handle)
            self.handle = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


def kzg_flatten(ctx: Context, commitments, evaluations, v: int, witness: bytes) -> KzgProof:
    """AggregateProof::flatten on `ctx` (Context.kzg_flatten)."""
    return ctx.kzg_flatten(commitments, evaluations, v, witness)


def _multi_challenges(challenges):
    """(r, t) ints -> the 8 Montgomery limbs of challenges_override; bytes pass through; None stays None"""
    if challenges is None or isinstance(challenges, (bytes, bytearray)):
        return bytes(challenges) if challenges is not None else None
    r, t = challenges
    return fr_to_bytes_mont([r, t])


class KzgKey:
    """An OpeningKey (240 bytes g || h || x_h, OpeningKey::to_bytes) bound to a context: plonk_kzg_key_create validates it like
    OpeningKey::from_bytes (raises InvalidData).  `batch_check` is OpeningKey::batch_check (reference key.rs:661-707),
    `srs_check` tests the context's commit key against this key.  Destroyed before its context, like a Prover."""

    def __init__(self, ctx: Context, opening_key: bytes):
        if len(opening_key) != 240:
            raise ValueError("an opening key is 240 bytes")
        self.ctx = ctx
        h = ctypes.c_void_p()
        ctx._check(ctx.lib.plonk_kzg_key_create(ctx.handle, bytes(opening_key), ctypes.byref(h)))
        self.handle = h
        ctx._provers.add(self)

    def batch_check_code(self, points, proofs, label: bytes = b"", u: "int | None" = None):
        """(return code of plonk_kzg_batch_check, plonk_verify_info as a dict)"""
        points, proofs = list(points), list(proofs)
        if len(points) != len(proofs):
            raise ValueError("one point per proof")
        arr = (KzgProof * max(len(proofs), 1))(*proofs)
        info = _VerifyInfo()
        rc = self.ctx.lib.plonk_kzg_batch_check(self.handle, fr_to_bytes_mont(points), arr, len(proofs), label, len(label),
                                                fr_to_bytes_mont([u]) if u is not None else None, ctypes.byref(info))
        return rc, {k: getattr(info, k) for k, _ in info._fields_}

    def batch_check(self, points, proofs, label: bytes = b"", u: "int | None" = None) -> bool:
        """True when every opening proofs[k] at points[k] holds, False when the batch does not verify (PLONK_ERR_VERIFY, an
        empty batch included).  Malformed input raises like every other error: a commitment that is no compressed G1 point
        (PLONK_ERR_POINT), a non-canonical scalar (PLONK_ERR_DATA) — `batch_check_code` returns the bare code instead.  `u`
        replaces the challenge the library derives from a fresh transcript over `label` — for a caller whose own transcript
        already has state; a predictable u voids the check."""
        rc, _ = self.batch_check_code(points, proofs, label, u)
        if rc not in (PLONK_OK, -12):
            self.ctx._check(rc)
        return rc == PLONK_OK

    def srs_check(self, seed: bytes) -> bool:
        """plonk_srs_check: is the context's commit key the powers of this opening key's tau?  seed: 32 fresh random bytes
        chosen after the key file was fixed."""
        if len(seed) != 32:
            raise ValueError("seed is 32 bytes")
        rc = self.ctx.lib.plonk_srs_check(self.handle, bytes(seed))
        if rc not in (PLONK_OK, -12):
            self.ctx._check(rc)
        return rc == PLONK_OK

    def pairing_check_each_info(self, a, b):
        """(verdict codes, plonk_verify_info as a dict) of plonk_kzg_pairing_check_each: verdict k is 0 iff
        e(a[k], x_h) == e(b[k], h); a, b: 48-byte compressed G1 points.  -10 (PLONK_ERR_POINT) for an item with a point that
        does not decode or is outside the subgroup; the compressed identity is legal."""
        a, b = [bytes(x) for x in a], [bytes(x) for x in b]
        if len(a) != len(b) or not a or any(len(x) != 48 for x in a + b):
            raise ValueError("two non-empty lists of 48-byte points, one pair per check")
        verdicts = (ctypes.c_int32 * len(a))()
        info = _VerifyInfo()
        rc = self.ctx.lib.plonk_kzg_pairing_check_each(self.handle, b"".join(a), b"".join(b), len(a), verdicts, ctypes.byref(info))
        if rc not in (PLONK_OK, -12):
            self.ctx._check(rc)
        return [int(v) for v in verdicts], {k: getattr(info, k) for k, _ in info._fields_}

    def pairing_check_each(self, a, b) -> list:
        return self.pairing_check_each_info(a, b)[0]

    def check_each_info(self, points, proofs):
        """(verdict codes, plonk_verify_info as a dict) of plonk_kzg_check_each: OpeningKey::check of every opening on its
        own (0 valid, -12 PLONK_ERR_VERIFY, -10 PLONK_ERR_POINT, -9 PLONK_ERR_DATA).  `points` may hold Montgomery bytes
        (32 each) in place of ints, for the non-canonical cases."""
        points, proofs = list(points), list(proofs)
        if len(points) != len(proofs) or not proofs:
            raise ValueError("a non-empty batch with one point per proof")
        arr = (KzgProof * len(proofs))(*proofs)
        pts = b"".join(p if isinstance(p, (bytes, bytearray)) else fr_to_bytes_mont([p]) for p in points)
        verdicts = (ctypes.c_int32 * len(proofs))()
        info = _VerifyInfo()
        rc = self.ctx.lib.plonk_kzg_check_each(self.handle, pts, arr, len(proofs), verdicts, ctypes.byref(info))
        if rc not in (PLONK_OK, -12):
            self.ctx._check(rc)
        return [int(v) for v in verdicts], {k: getattr(info, k) for k, _ in info._fields_}

    def check_each(self, points, proofs) -> list:
        return self.check_each_info(points, proofs)[0]

    def check_multi_code(self, log_n: int, commitments, items, values, proof: bytes, label: bytes = b"", challenges=None):
        """(return code of plonk_kzg_multiproof_check, plonk_verify_info as a dict).  items: (vector index, point index) pairs;
        values: one int per item, or 32 Montgomery bytes (for the non-canonical cases); challenges: (r, t) ints, or 64 Montgomery
        bytes."""
        commitments, items, values = [bytes(c) for c in commitments], list(items), list(values)
        if any(len(c) != 48 for c in commitments) or len(bytes(proof)) != 96:
            raise ValueError("commitments are 48-byte compressed G1 points, a multiproof is 96 bytes")
        if len(values) != len(items):
            raise ValueError("one value per item")
        n = max(len(items), 1)
        vidx = (ctypes.c_uint32 * n)(*[it[0] for it in items])
        midx = (ctypes.c_uint32 * n)(*[it[1] for it in items])
        vals = b"".join(bytes(v) if isinstance(v, (bytes, bytearray)) else fr_to_bytes_mont([v]) for v in values) or b"\0"
        info = _VerifyInfo()
        rc = self.ctx.lib.plonk_kzg_multiproof_check(self.handle, log_n, b"".join(commitments) or None, len(commitments), vidx, midx, vals,
                                                     len(items), bytes(proof), label, len(label), _multi_challenges(challenges),
                                                     ctypes.byref(info))
        return rc, {k: getattr(info, k) for k, _ in info._fields_}

    def check_multi(self, log_n: int, commitments, items, values, proof: bytes, label: bytes = b"", challenges=None) -> bool:
        """plonk_kzg_multiproof_check: True when the multiproof of KzgDomain.open_multi verifies, False when it does not
        (PLONK_ERR_VERIFY); malformed input raises.  `challenges` = (r, t) replaces both challenges the library derives from a
        fresh transcript over `label` and every input; a predictable r or t voids the check."""
        rc, _ = self.check_multi_code(log_n, commitments, items, values, proof, label, challenges)
        if rc not in (PLONK_OK, -12):
            self.ctx._check(rc)
        return rc == PLONK_OK

    def check_tree_code(self, log_n: int, depth: int, root: bytes, leaf_index, values, path, proof: bytes, label: bytes = b"",
                        challenges=None, nodes: "int | None" = None):
        """(return code of plonk_kzg_tree_check, plonk_verify_info as a dict).  values: one int per leaf index, or 32 Montgomery
        bytes; path: the 48-byte path commitments KzgTree.prove returned; nodes: their count as told to the library (default:
        len(path))"""
        leaf_index, values, path = list(leaf_index), list(values), [bytes(c) for c in path]
        if len(bytes(root)) != 48 or any(len(c) != 48 for c in path) or len(bytes(proof)) != 96:
            raise ValueError("commitments are 48-byte compressed G1 points, a multiproof is 96 bytes")
        if len(values) != len(leaf_index):
            raise ValueError("one value per leaf index")
        idx = (ctypes.c_uint64 * max(len(leaf_index), 1))(*leaf_index)
        vals = b"".join(bytes(v) if isinstance(v, (bytes, bytearray)) else fr_to_bytes_mont([v]) for v in values) or b"\0"
        info = _VerifyInfo()
        rc = self.ctx.lib.plonk_kzg_tree_check(self.handle, log_n, depth, bytes(root), idx, vals, len(leaf_index), b"".join(path) or None,
                                               len(path) if nodes is None else nodes, bytes(proof), label, len(label),
                                               _multi_challenges(challenges), ctypes.byref(info))
        return rc, {k: getattr(info, k) for k, _ in info._fields_}

    def check_tree(self, log_n: int, depth: int, root: bytes, leaf_index, values, path, proof: bytes, label: bytes = b"",
                   challenges=None) -> bool:
        """plonk_kzg_tree_check: True when the proof of KzgTree.prove shows these leaves under `root`, False when it does not
        (PLONK_ERR_VERIFY); malformed input raises.  Needs no tree and no domain."""
        rc, _ = self.check_tree_code(log_n, depth, root, leaf_index, values, path, proof, label, challenges)
        if rc not in (PLONK_OK, -12):
            self.ctx._check(rc)
        return rc == PLONK_OK

    def _pairing_each_values(self, a, b):
        """TEST HOOK: per check the final-exponentiated Fp12 value of e(-a, x_h) e(b, h) as 12 integers (tower order), from
        the device pairing kernel.  Not part of the C API."""
        a, b = [bytes(x) for x in a], [bytes(x) for x in b]
        out = (ctypes.c_uint64 * (72 * len(a)))()
        self.ctx._check(self.ctx.lib.plonk_test_pairing_each(self.handle, b"".join(a), b"".join(b), len(a), out))
        return [[sum(int(out[72 * k + 6 * i + j]) << (64 * j) for j in range(6)) for i in range(12)] for k in range(len(a))]

    def _last_challenges(self):
        u, r = ctypes.create_string_buffer(32), ctypes.create_string_buffer(32)
        self.ctx._check(self.ctx.lib.plonk_test_kzg_last(self.handle, u, r))
        return fr_from_bytes_mont(u.raw)[0], fr_from_bytes_mont(r.raw)[0]

    def close(self):
        if getattr(self, "handle", None):
            for v in list(getattr(self, "_cell_verifiers", ())):   # they hold a pointer to the native key
                v.close()
            if getattr(self.ctx, "handle", None):
                self.ctx.lib.plonk_kzg_key_destroy(self.handle)
            self.handle = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


class KzgCellVerifier:
    """plonk_kzg_cell_verifier: checks the cells and proofs of KzgDomain.open_cells on the device (include/plonk_hip.h).
    `key` is a KzgKey whose third element is [tau^l] h.  The handle copies the first l points of the context's commit key;
    reloading that key afterwards does not affect it.  `items` is a list of (commitment_index, cell_index, values, proof48);
    values: l ints, or 32 l Montgomery bytes (for the non-canonical cases).  Destroyed before its key."""

    def __init__(self, key: KzgKey, log_n: int, log_cell: int):
        self.key, self.ctx, self.log_n, self.log_cell = key, key.ctx, log_n, log_cell
        h = ctypes.c_void_p()
        self.ctx._check(self.ctx.lib.plonk_kzg_cell_verifier_create(key.handle, log_n, log_cell, ctypes.byref(h)))
        self.handle = h
        if not hasattr(key, "_cell_verifiers"):
            key._cell_verifiers = weakref.WeakSet()
        key._cell_verifiers.add(self)

    def _args(self, commitments, items):
        commitments, items = [bytes(c) for c in commitments], list(items)
        l = 1 << self.log_cell
        if any(len(c) != 48 for c in commitments) or any(len(bytes(it[3])) != 48 for it in items):
            raise ValueError("commitments and proofs are 48-byte compressed G1 points")
        vals = []
        for it in items:
            v = bytes(it[2]) if isinstance(it[2], (bytes, bytearray)) else fr_to_bytes_mont(it[2])
            if len(v) != 32 * l:
                raise ValueError("a cell has 2^log_cell values")
            vals.append(v)
        n = max(len(items), 1)
        cidx = (ctypes.c_uint32 * n)(*[it[0] for it in items])
        kidx = (ctypes.c_uint32 * n)(*[it[1] for it in items])
        return (self.handle, b"".join(commitments) or None, len(commitments), cidx, kidx, b"".join(vals) or b"\0",
                b"".join(bytes(it[3]) for it in items) or b"\0", len(items))

    def verify_code(self, commitments, items, label: bytes = b"", rho: "int | None" = None):
        """(return code of plonk_kzg_verify_cells, plonk_verify_info as a dict)"""
        info = _VerifyInfo()
        rc = self.ctx.lib.plonk_kzg_verify_cells(*self._args(commitments, items), label, len(label),
                                                 fr_to_bytes_mont([rho]) if rho is not None else None, ctypes.byref(info))
        return rc, {k: getattr(info, k) for k, _ in info._fields_}

    def verify(self, commitments, items, label: bytes = b"", rho: "int | None" = None) -> bool:
        """The folded check: True when the whole batch verifies, False when it does not (PLONK_ERR_VERIFY, an empty batch
        included); malformed input raises.  `rho` replaces the challenge the library derives from a fresh transcript over
        `label` and every input; a rho the prover could predict voids the check."""
        rc, _ = self.verify_code(commitments, items, label, rho)
        if rc not in (PLONK_OK, -12):
            self.ctx._check(rc)
        return rc == PLONK_OK

    def verify_each_info(self, commitments, items):
        """(verdict codes, plonk_verify_info as a dict) of plonk_kzg_verify_cells_each: 0 valid, -12 PLONK_ERR_VERIFY, -10
        PLONK_ERR_POINT, -9 PLONK_ERR_DATA per item"""
        args = self._args(commitments, items)
        verdicts = (ctypes.c_int32 * max(args[-1], 1))()
        info = _VerifyInfo()
        rc = self.ctx.lib.plonk_kzg_verify_cells_each(*args, verdicts, ctypes.byref(info))
        if rc not in (PLONK_OK, -12):
            self.ctx._check(rc)
        return [int(v) for v in verdicts][:args[-1]], {k: getattr(info, k) for k, _ in info._fields_}

    def verify_each(self, commitments, items) -> list:
        return self.verify_each_info(commitments, items)[0]

    def last(self) -> dict:
        info = _KzgCellVerifyInfo()
        self.ctx._check(self.ctx.lib.plonk_kzg_cell_verifier_last(self.handle, ctypes.byref(info)))
        return {k: getattr(info, k) for k, _ in info._fields_}

    def _last_rho(self) -> int:
        """TEST HOOK: the challenge of the last folded call.  Not part of the C API."""
        out = ctypes.create_string_buffer(32)
        self.ctx._check(self.ctx.lib.plonk_test_kzg_cell_verify_last_rho(self.handle, out))
        return fr_from_bytes_mont(out.raw)[0]

    def _force_paths(self, min_left: int = 0, min_right: int = 0):
        """TEST HOOK: plonk_msm_points' min_bucket_terms for the left / right sum of the next folded calls (1 forces the
        buckets, a value above the term count the per-term kernel, 0 restores the rule).  Not part of the C API."""
        self.ctx._check(self.ctx.lib.plonk_test_kzg_cell_verify_force_paths(self.handle, min_left, min_right))

    def close(self):
        if getattr(self, "handle", None):
            if getattr(self.key, "handle", None) and getattr(self.ctx, "handle", None):
                self.ctx.lib.plonk_kzg_cell_verifier_destroy(self.handle)
            self.handle = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


class KzgDomain:
    """plonk_kzg_domain: the commit key of `ctx` prepared for openings at EVERY point of the size-2^log_n domain (group FFTs,
    include/plonk_hip.h).  `open` returns per polynomial its n evaluations and n witnesses; witness i and evaluation i belong
    to `points()[i]`.  Destroyed before its context, like a KzgKey."""

    def __init__(self, ctx: Context, log_n: int):
        self.ctx, self.log_n, self.n = ctx, log_n, 1 << max(log_n, 0)
        h = ctypes.c_void_p()
        ctx._check(ctx.lib.plonk_kzg_domain_create(ctx.handle, log_n, ctypes.byref(h)))
        self.handle = h
        ctx._provers.add(self)

    def points(self) -> list:
        out = ctypes.create_string_buffer(32 * self.n)
        self.ctx._check(self.ctx.lib.plonk_kzg_domain_points(self.handle, out))
        return fr_from_bytes_mont(out.raw)

    def open_bytes(self, polys_bytes, commitments: bool = True):
        """plonk_kzg_open_domain on Montgomery bytes (32 per coefficient) -> (evaluation bytes, witness bytes, commitment
        bytes or None), each the concatenation over the polynomials"""
        bufs = [bytes(b) for b in polys_bytes]
        count = len(bufs)
        keep = [ctypes.create_string_buffer(b, len(b)) if b else None for b in bufs]
        parr = (ctypes.c_void_p * max(count, 1))(*[ctypes.cast(k, ctypes.c_void_p).value if k is not None else None for k in keep])
        larr = (ctypes.c_uint64 * max(count, 1))(*[len(b) // 32 for b in bufs])
        ev = ctypes.create_string_buffer(max(32 * self.n * count, 1))
        wit = ctypes.create_string_buffer(max(48 * self.n * count, 1))
        cm = ctypes.create_string_buffer(max(48 * count, 1)) if commitments else None
        self.ctx._check(self.ctx.lib.plonk_kzg_open_domain(self.handle, parr, larr, count, ev, wit, cm))
        return ev.raw[:32 * self.n * count], wit.raw[:48 * self.n * count], cm.raw[:48 * count] if commitments else None

    def open(self, polys, commitments: bool = True):
        """polys: coefficient lists of ints, or Montgomery bytes -> (evaluations[j][i], witnesses[j][i] (48 bytes each),
        commitments[j] or None)"""
        bufs = [p if isinstance(p, (bytes, bytearray)) else fr_to_bytes_mont(p) for p in polys]
        ev, wit, cm = self.open_bytes(bufs, commitments)
        n, count = self.n, len(bufs)
        evs = fr_from_bytes_mont(ev)
        return ([evs[j * n:(j + 1) * n] for j in range(count)],
                [[wit[48 * (j * n + i):48 * (j * n + i + 1)] for i in range(n)] for j in range(count)],
                [cm[48 * j:48 * j + 48] for j in range(count)] if commitments else None)

    def open_dev(self, ptrs, lens, evaluations: int, witnesses: int, commitments: "int | None" = None):
        """plonk_kzg_open_domain_dev: polynomials resident in HBM (device pointers, coefficients each); the outputs are device
        pointers (count x n x 32, count x n x 48, count x 48 bytes or None)"""
        ptrs, lens = list(ptrs), list(lens)
        count = len(lens)
        parr = (ctypes.c_void_p * max(count, 1))(*ptrs)
        larr = (ctypes.c_uint64 * max(count, 1))(*lens)
        self.ctx._check(self.ctx.lib.plonk_kzg_open_domain_dev(self.handle, parr, larr, count, evaluations, witnesses, commitments))

    def last(self) -> dict:
        info = _KzgDomainInfo()
        self.ctx._check(self.ctx.lib.plonk_kzg_domain_last(self.handle, ctypes.byref(info)))
        return {k: getattr(info, k) for k, _ in info._fields_}

    # ---- evaluation form: vectors of exactly n values on the domain ----
    def _host_vectors(self, vectors):
        bufs = [bytes(p) if isinstance(p, (bytes, bytearray)) else fr_to_bytes_mont(p) for p in vectors]
        for b in bufs:
            if len(b) != 32 * self.n:
                raise ValueError("a vector of values must hold exactly n field elements")
        keep = [ctypes.create_string_buffer(b, len(b)) for b in bufs]
        return keep, [ctypes.cast(k, ctypes.c_void_p).value for k in keep]

    def _commit_evals(self, fn, ptrs):
        count = len(ptrs)
        parr = (ctypes.c_void_p * max(count, 1))(*ptrs)
        cm = ctypes.create_string_buffer(48 * max(count, 1))
        self.ctx._check(fn(self.handle, parr, count, cm))
        return [cm.raw[48 * j:48 * j + 48] for j in range(count)]

    def commit_evals(self, vectors) -> list:
        """plonk_kzg_commit_evals: vectors of n values (lists of ints, or Montgomery bytes) -> 48-byte commitments"""
        keep, ptrs = self._host_vectors(vectors)
        return self._commit_evals(self.ctx.lib.plonk_kzg_commit_evals, ptrs)

    def commit_evals_dev(self, ptrs) -> list:
        """plonk_kzg_commit_evals_dev: the same for vectors resident in HBM (device pointers, n values each)"""
        return self._commit_evals(self.ctx.lib.plonk_kzg_commit_evals_dev, list(ptrs))

    def _open_evals(self, fn, ptrs, point, v, commitments, witness):
        count = len(ptrs)
        parr = (ctypes.c_void_p * max(count, 1))(*ptrs)
        ev = ctypes.create_string_buffer(32 * max(count, 1))
        cm = ctypes.create_string_buffer(48 * max(count, 1)) if commitments else None
        wit = ctypes.create_string_buffer(48) if witness else None
        vb = fr_to_bytes_mont([v]) if v is not None else None
        self.ctx._check(fn(self.handle, parr, count, fr_to_bytes_mont([point]), vb, ev, cm, wit))
        return (fr_from_bytes_mont(ev.raw[:32 * count]),
                [cm.raw[48 * j:48 * j + 48] for j in range(count)] if commitments else None, wit.raw if witness else None)

    def open_evals(self, vectors, point: int, v: "int | None" = None, commitments: bool = True, witness: bool = True):
        """plonk_kzg_open_evals: vectors of n values opened at `point` (any field element, a domain point included) ->
        (evaluations, commitments or None, witness or None), the tuple Context.kzg_open returns for the coefficient forms"""
        keep, ptrs = self._host_vectors(vectors)
        return self._open_evals(self.ctx.lib.plonk_kzg_open_evals, ptrs, point, v, commitments, witness)

    def open_evals_dev(self, ptrs, point: int, v: "int | None" = None, commitments: bool = True, witness: bool = True):
        """plonk_kzg_open_evals_dev: the same for vectors resident in HBM (device pointers, n values each)"""
        return self._open_evals(self.ctx.lib.plonk_kzg_open_evals_dev, list(ptrs), point, v, commitments, witness)

    def evals_last(self) -> dict:
        info = _KzgEvalsInfo()
        self.ctx._check(self.ctx.lib.plonk_kzg_evals_last(self.handle, ctypes.byref(info)))
        return {k: getattr(info, k) for k, _ in info._fields_}

    # ---- opt-in Lagrange-basis tables: the MSMs of the evaluation-form calls and multiproofs as grouped table launches ----
    def tables_last(self) -> dict:
        info = _KzgEvalsTablesInfo()
        self.ctx._check(self.ctx.lib.plonk_kzg_evals_tables_last(self.handle, ctypes.byref(info)))
        return {k: getattr(info, k) for k, _ in info._fields_ if k != "reserved"}

    def build_tables(self) -> dict:
        """plonk_kzg_evals_tables_build: rows x n x 128 bytes of the context's table budget until drop_tables / close"""
        self.ctx._check(self.ctx.lib.plonk_kzg_evals_tables_build(self.handle))
        return self.tables_last()

    def drop_tables(self):
        self.ctx._check(self.ctx.lib.plonk_kzg_evals_tables_drop(self.handle))

    # ---- opt-in window tables: commitments of MANY SHORT vectors, one wave per vector ----
    def many_last(self) -> dict:
        info = _KzgManyInfo()
        self.ctx._check(self.ctx.lib.plonk_kzg_many_last(self.handle, ctypes.byref(info)))
        return {k: getattr(info, k) for k, _ in info._fields_ if k != "reserved"}

    def build_many_tables(self, window_bits: int = 0) -> dict:
        """plonk_kzg_many_tables_build: n x W x 2^(c-1) x 128 bytes of the context's table budget until drop_many_tables /
        close; window_bits 0 picks the widest width that fits"""
        self.ctx._check(self.ctx.lib.plonk_kzg_many_tables_build(self.handle, window_bits))
        return self.many_last()

    def drop_many_tables(self):
        self.ctx._check(self.ctx.lib.plonk_kzg_many_tables_drop(self.handle))

    def commit_many(self, vectors) -> list:
        """plonk_kzg_commit_many: vectors of n values (lists of ints, or ONE bytes object of count x n x 32 Montgomery bytes)
        -> 48-byte commitments"""
        if isinstance(vectors, (bytes, bytearray)):
            raw = bytes(vectors)
        else:
            raw = b"".join(bytes(p) if isinstance(p, (bytes, bytearray)) else fr_to_bytes_mont(p) for p in vectors)
        if len(raw) % (32 * self.n):
            raise ValueError("a vector of values must hold exactly n field elements")
        count = len(raw) // (32 * self.n)
        cm = ctypes.create_string_buffer(48 * max(count, 1))
        self.ctx._check(self.ctx.lib.plonk_kzg_commit_many(self.handle, raw, count, cm))
        return [cm.raw[48 * j:48 * j + 48] for j in range(count)]

    def commit_many_dev(self, ptr: int, count: int, out_ptr: int):
        """plonk_kzg_commit_many_dev: count x n values resident at `ptr`; the count x 48 bytes are written to the device
        pointer `out_ptr`"""
        self.ctx._check(self.ctx.lib.plonk_kzg_commit_many_dev(self.handle, ptr, count, out_ptr))

    def update_many(self, updates, base=None) -> list:
        """plonk_kzg_update_many: updates[j] = [(index, delta), ...]; base: one 48-byte commitment per segment, or None for
        the identity -> base_j + sum delta L_index as 48 bytes each"""
        updates = [list(u) for u in updates]
        count = len(updates)
        offs, idx, deltas = [0], [], []
        for u in updates:
            idx.extend(i for i, _ in u)
            deltas.extend(x for _, x in u)
            offs.append(len(idx))
        bin_ = None
        if base is not None:
            bin_ = b"".join(bytes(b) for b in base)
            if len(bin_) != 48 * count:
                raise ValueError("one 48-byte base per segment")
        oarr = (ctypes.c_uint64 * (count + 1))(*offs)
        iarr = (ctypes.c_uint32 * max(len(idx), 1))(*idx)
        cm = ctypes.create_string_buffer(48 * max(count, 1))
        self.ctx._check(self.ctx.lib.plonk_kzg_update_many(self.handle, bin_, oarr, iarr, fr_to_bytes_mont(deltas) if deltas else b"\0" * 32,
                                                            count, cm))
        return [cm.raw[48 * j:48 * j + 48] for j in range(count)]

    # ---- multiproofs: many (vector, domain point) openings, one 96-byte proof ----
    def _open_multi(self, fn, ptrs, items, label, commitments, challenges):
        items = list(items)
        M, K = len(ptrs), len(items)
        parr = (ctypes.c_void_p * max(M, 1))(*ptrs)
        vidx = (ctypes.c_uint32 * max(K, 1))(*[it[0] for it in items])
        midx = (ctypes.c_uint32 * max(K, 1))(*[it[1] for it in items])
        cin = None
        if commitments is not None:
            cin = b"".join(bytes(c) for c in commitments)
            if len(cin) != 48 * M:
                raise ValueError("one 48-byte commitment per vector")
        vals = ctypes.create_string_buffer(32 * max(K, 1))
        cout = ctypes.create_string_buffer(48 * max(M, 1))
        proof = ctypes.create_string_buffer(96)
        self.ctx._check(fn(self.handle, parr, M, cin, vidx, midx, K, label, len(label), _multi_challenges(challenges), vals, cout, proof))
        return fr_from_bytes_mont(vals.raw[:32 * K]), [cout.raw[48 * j:48 * j + 48] for j in range(M)], proof.raw

    def open_multi(self, vectors, items, label: bytes = b"", commitments=None, challenges=None):
        """plonk_kzg_multiproof_open: vectors of n values (lists of ints, or Montgomery bytes); items: (vector index, point index)
        pairs -> (values, commitments, proof): the value of every item, the commitments the proof is bound to (those given, or
        computed when `commitments` is None) and the 96-byte proof D || pi.  `challenges` = (r, t) replaces both transcript
        challenges; a predictable r or t voids the check."""
        keep, ptrs = self._host_vectors(vectors)
        return self._open_multi(self.ctx.lib.plonk_kzg_multiproof_open, ptrs, items, label, commitments, challenges)

    def open_multi_dev(self, ptrs, items, label: bytes = b"", commitments=None, challenges=None):
        """plonk_kzg_multiproof_open_dev: the same for vectors resident in HBM (device pointers, n values each)"""
        return self._open_multi(self.ctx.lib.plonk_kzg_multiproof_open_dev, list(ptrs), items, label, commitments, challenges)

    def multi_last(self) -> dict:
        info = _KzgMultiproofInfo()
        self.ctx._check(self.ctx.lib.plonk_kzg_multiproof_last(self.handle, ctypes.byref(info)))
        return {k: getattr(info, k) for k, _ in info._fields_}

    def _multi_last_challenges(self):
        """TEST HOOK: (r, t) of the last open_multi / open_multi_dev.  Not part of the C API."""
        out = ctypes.create_string_buffer(64)
        self.ctx._check(self.ctx.lib.plonk_test_kzg_multiproof_last_challenges(self.handle, out))
        return tuple(fr_from_bytes_mont(out.raw))

    # ---- cell proofs: one proof per coset of l = 2^log_cell values ----
    def open_cells_bytes(self, polys_bytes, log_cell: int, commitments: bool = True):
        """plonk_kzg_open_cells on Montgomery bytes (32 per coefficient) -> (cell-value bytes, proof bytes, commitment bytes or
        None), each the concatenation over the polynomials"""
        bufs = [bytes(b) for b in polys_bytes]
        count = len(bufs)
        r = self.n >> log_cell if 0 <= log_cell < 64 else 0
        keep = [ctypes.create_string_buffer(b, len(b)) if b else None for b in bufs]
        parr = (ctypes.c_void_p * max(count, 1))(*[ctypes.cast(k, ctypes.c_void_p).value if k is not None else None for k in keep])
        larr = (ctypes.c_uint64 * max(count, 1))(*[len(b) // 32 for b in bufs])
        cells = ctypes.create_string_buffer(max(32 * self.n * count, 1))
        proofs = ctypes.create_string_buffer(max(48 * r * count, 1))
        cm = ctypes.create_string_buffer(max(48 * count, 1)) if commitments else None
        self.ctx._check(self.ctx.lib.plonk_kzg_open_cells(self.handle, log_cell, parr, larr, count, cells, proofs, cm))
        return cells.raw[:32 * self.n * count], proofs.raw[:48 * r * count], cm.raw[:48 * count] if commitments else None

    def open_cells(self, polys, log_cell: int, commitments: bool = True):
        """polys: coefficient lists of ints, or Montgomery bytes -> (cells[j][k] (the l values of cell k: f(w^(k + r i)), i < l),
        proofs[j][k] (48 bytes each), commitments[j] or None); cell k and proof k belong to cell_points(log_cell)[0][k]"""
        bufs = [p if isinstance(p, (bytes, bytearray)) else fr_to_bytes_mont(p) for p in polys]
        cells, proofs, cm = self.open_cells_bytes(bufs, log_cell, commitments)
        n, count, l = self.n, len(bufs), 1 << log_cell
        r = n >> log_cell
        vals = fr_from_bytes_mont(cells)
        return ([[vals[j * n + k * l:j * n + (k + 1) * l] for k in range(r)] for j in range(count)],
                [[proofs[48 * (j * r + k):48 * (j * r + k + 1)] for k in range(r)] for j in range(count)],
                [cm[48 * j:48 * j + 48] for j in range(count)] if commitments else None)

    def open_cells_dev(self, ptrs, lens, log_cell: int, cells: int, proofs: int, commitments: "int | None" = None):
        """plonk_kzg_open_cells_dev: polynomials resident in HBM (device pointers, coefficients each); the outputs are device
        pointers (count x n x 32, count x r x 48, count x 48 bytes or None)"""
        ptrs, lens = list(ptrs), list(lens)
        count = len(lens)
        parr = (ctypes.c_void_p * max(count, 1))(*ptrs)
        larr = (ctypes.c_uint64 * max(count, 1))(*lens)
        self.ctx._check(self.ctx.lib.plonk_kzg_open_cells_dev(self.handle, log_cell, parr, larr, count, cells, proofs, commitments))

    def cell_points(self, log_cell: int):
        """plonk_kzg_cell_points -> (x, shift): x[k] = w^(l k), the constant of cell k's vanishing polynomial X^l - x[k], and
        shift[k] = w^k, the coset's representative"""
        r = max(self.n >> log_cell, 1) if 0 <= log_cell < 64 else 1
        x, sh = ctypes.create_string_buffer(32 * r), ctypes.create_string_buffer(32 * r)
        self.ctx._check(self.ctx.lib.plonk_kzg_cell_points(self.handle, log_cell, x, sh))
        return fr_from_bytes_mont(x.raw), fr_from_bytes_mont(sh.raw)

    def cells_last(self) -> dict:
        info = _KzgCellsInfo()
        self.ctx._check(self.ctx.lib.plonk_kzg_cells_last(self.handle, ctypes.byref(info)))
        return {k: getattr(info, k) for k, _ in info._fields_}

    # ---- cell recovery: the polynomial, all of its cells and their proofs from a subset of the cells ----
    def _recover_check(self, rc: int, status, count: int):
        if rc == -12:
            err = ProofVerificationError(rc, (self.ctx.lib.plonk_last_error() or b"").decode())
            err.status = list(status[:count])
            raise err
        self.ctx._check(rc)

    def recover_cells_bytes(self, cell_ids, values_bytes, log_cell: int, max_len: int, proofs: bool = True, commitments: bool = True,
                            coeffs: bool = False, cells: bool = True):
        """plonk_kzg_recover_cells on Montgomery bytes: values_bytes[j] = the cells cell_ids of polynomial j, l x 32 bytes each, in
        the order of cell_ids -> (cell-value bytes, proof bytes, commitment bytes, coefficient bytes), each the concatenation
        over the polynomials, or None where not asked for.  Raises ProofVerificationError (with .status, one code per
        polynomial) when a polynomial's values fit no polynomial of max_len coefficients; nothing is returned then."""
        ids = list(cell_ids)
        bufs = [bytes(b) for b in values_bytes]
        count, a = len(bufs), len(ids)
        r = self.n >> log_cell if 0 <= log_cell < 64 else 0
        for b in bufs:
            if len(b) != 32 * (a << log_cell if 0 <= log_cell < 64 else 0):
                raise ValueError("a polynomial's values must hold exactly len(cell_ids) cells of l field elements")
        keep = [ctypes.create_string_buffer(b, len(b)) for b in bufs]
        parr = (ctypes.c_void_p * max(count, 1))(*[ctypes.cast(k, ctypes.c_void_p).value for k in keep])
        iarr = (ctypes.c_uint32 * max(a, 1))(*ids)
        out_cells = ctypes.create_string_buffer(max(32 * self.n * count, 1)) if cells else None
        out_proofs = ctypes.create_string_buffer(max(48 * r * count, 1)) if proofs else None
        out_cm = ctypes.create_string_buffer(max(48 * count, 1)) if commitments else None
        out_coeffs = ctypes.create_string_buffer(max(32 * self.n * count, 1)) if coeffs else None
        status = (ctypes.c_int32 * max(count, 1))()
        rc = self.ctx.lib.plonk_kzg_recover_cells(self.handle, log_cell, iarr, a, parr, count, max_len, out_coeffs, out_cells, out_proofs,
                                                  out_cm, status)
        self._recover_check(rc, status, count)
        return (out_cells.raw[:32 * self.n * count] if cells else None, out_proofs.raw[:48 * r * count] if proofs else None,
                out_cm.raw[:48 * count] if commitments else None, out_coeffs.raw[:32 * self.n * count] if coeffs else None)

    def recover_cells(self, cell_ids, values, log_cell: int, max_len: int, proofs: bool = True, commitments: bool = True,
                      coeffs: bool = False):
        """values[j][i]: the l values (ints) of cell cell_ids[i] of polynomial j — what open_cells returned as cells[j][cell_ids[i]]
        — or per polynomial the same as Montgomery bytes.  All polynomials share the cell set; each has at most max_len
        coefficients, max_len <= len(cell_ids) * l.  -> (cells[j][k], proofs[j][k] or None, commitments[j] or None, coefficients[j]
        (n ints) or None): the first three are what open_cells returns for the recovered polynomials."""
        bufs = [v if isinstance(v, (bytes, bytearray)) else fr_to_bytes_mont([x for cell in v for x in cell]) for v in values]
        cl, pr, cm, co = self.recover_cells_bytes(cell_ids, bufs, log_cell, max_len, proofs, commitments, coeffs)
        n, count, l = self.n, len(bufs), 1 << log_cell
        r = n >> log_cell
        vals = fr_from_bytes_mont(cl)
        cof = fr_from_bytes_mont(co) if coeffs else None
        return ([[vals[j * n + k * l:j * n + (k + 1) * l] for k in range(r)] for j in range(count)],
                [[pr[48 * (j * r + k):48 * (j * r + k + 1)] for k in range(r)] for j in range(count)] if proofs else None,
                [cm[48 * j:48 * j + 48] for j in range(count)] if commitments else None,
                [cof[j * n:(j + 1) * n] for j in range(count)] if coeffs else None)

    def recover_cells_dev(self, cell_ids, ptrs, log_cell: int, max_len: int, coeffs: "int | None" = None, cells: "int | None" = None,
                          proofs: "int | None" = None, commitments: "int | None" = None):
        """plonk_kzg_recover_cells_dev: values resident in HBM (device pointers, len(cell_ids) x l values each); the outputs are
        device pointers (count x n x 32, count x n x 32, count x r x 48, count x 48 bytes) or None.  Returns the status list."""
        ids, ptrs = list(cell_ids), list(ptrs)
        count = len(ptrs)
        parr = (ctypes.c_void_p * max(count, 1))(*ptrs)
        iarr = (ctypes.c_uint32 * max(len(ids), 1))(*ids)
        status = (ctypes.c_int32 * max(count, 1))()
        rc = self.ctx.lib.plonk_kzg_recover_cells_dev(self.handle, log_cell, iarr, len(ids), parr, count, max_len, coeffs, cells, proofs,
                                                      commitments, status)
        self._recover_check(rc, status, count)
        return list(status[:count])

    def recover_last(self) -> dict:
        info = _KzgRecoverInfo()
        self.ctx._check(self.ctx.lib.plonk_kzg_recover_last(self.handle, ctypes.byref(info)))
        return {k: getattr(info, k) for k, _ in info._fields_}

    def _set_workspace_cap(self, nbytes: int):
        """TEST HOOK: the cap on the point workspace (0 = default), to force several chunks.  Not part of the C API."""
        self.ctx._check(self.ctx.lib.plonk_test_kzg_domain_set_cap(self.handle, nbytes))

    def close(self):
        if getattr(self, "handle", None):
            for t in list(getattr(self, "_trees", ())):   # they hold a pointer to the native handle
                t.close()
            if getattr(self.ctx, "handle", None):
                self.ctx.lib.plonk_kzg_evals_tables_drop(self.handle)   # the table budget first, then the handle
                self.ctx.lib.plonk_kzg_many_tables_drop(self.handle)
                self.ctx.lib.plonk_kzg_domain_destroy(self.handle)
            self.handle = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


class KzgTree:
    """plonk_kzg_tree: a dense n-ary KZG vector-commitment tree of `depth` levels over `domain` (n = 2^log_n values per node,
    N = n^depth leaves), every level resident on the device (include/plonk_hip.h).  The domain must hold many-vector tables
    (KzgDomain.build_many_tables) for `build` and `update`.  Closed before its domain: KzgDomain.close does it."""

    def __init__(self, domain: "KzgDomain", depth: int):
        self.domain, self.ctx, self.depth, self.log_n = domain, domain.ctx, depth, domain.log_n
        self.leaves = 1 << (domain.log_n * max(depth, 0)) if 0 <= domain.log_n * max(depth, 0) <= 26 else 0
        h = ctypes.c_void_p()
        self.ctx._check(self.ctx.lib.plonk_kzg_tree_create(domain.handle, depth, ctypes.byref(h)))
        self.handle = h
        if not hasattr(domain, "_trees"):
            domain._trees = weakref.WeakSet()
        domain._trees.add(self)

    def build(self, leaves):
        """plonk_kzg_tree_build: the N leaves as ints, or N x 32 Montgomery bytes"""
        raw = bytes(leaves) if isinstance(leaves, (bytes, bytearray)) else fr_to_bytes_mont(leaves)
        if len(raw) != 32 * self.leaves:
            raise ValueError("a tree is built from exactly n^depth leaves")
        self.ctx._check(self.ctx.lib.plonk_kzg_tree_build(self.handle, raw))

    def build_dev(self, ptr: int):
        """plonk_kzg_tree_build_dev: the N leaves resident at the device pointer `ptr`"""
        self.ctx._check(self.ctx.lib.plonk_kzg_tree_build_dev(self.handle, ptr))

    def root(self) -> bytes:
        out = ctypes.create_string_buffer(48)
        self.ctx._check(self.ctx.lib.plonk_kzg_tree_root(self.handle, out))
        return out.raw

    def nodes(self, level: int, first: int = 0, count: "int | None" = None) -> list:
        """plonk_kzg_tree_nodes: the 48-byte commitments of `count` nodes of `level` from `first` on (default: the rest)"""
        if count is None:
            count = (1 << (self.log_n * level)) - first
        out = ctypes.create_string_buffer(48 * max(count, 1))
        self.ctx._check(self.ctx.lib.plonk_kzg_tree_nodes(self.handle, level, first, count, out))
        return [out.raw[48 * j:48 * j + 48] for j in range(count)]

    def update(self, leaf_index, values):
        """plonk_kzg_tree_update: leaf leaf_index[k] becomes values[k] (ints, or 32 Montgomery bytes each)"""
        leaf_index, values = list(leaf_index), list(values)
        if len(leaf_index) != len(values):
            raise ValueError("one value per leaf index")
        idx = (ctypes.c_uint64 * max(len(leaf_index), 1))(*leaf_index)
        vals = b"".join(bytes(v) if isinstance(v, (bytes, bytearray)) else fr_to_bytes_mont([v]) for v in values) or b"\0" * 32
        self.ctx._check(self.ctx.lib.plonk_kzg_tree_update(self.handle, idx, vals, len(leaf_index)))

    def proof_nodes(self, leaf_index) -> int:
        leaf_index = list(leaf_index)
        idx = (ctypes.c_uint64 * max(len(leaf_index), 1))(*leaf_index)
        out = ctypes.c_uint64()
        self.ctx._check(self.ctx.lib.plonk_kzg_tree_proof_nodes(self.log_n, self.depth, idx, len(leaf_index), ctypes.byref(out)))
        return out.value

    def prove(self, leaf_index, label: bytes = b"", challenges=None):
        """plonk_kzg_tree_prove -> (values, path, proof): the leaves in the order of leaf_index, the path commitments (48 bytes
        each, levels 1 .. depth-1, ascending within a level) and the 96-byte multiproof"""
        leaf_index = list(leaf_index)
        count = len(leaf_index)
        idx = (ctypes.c_uint64 * max(count, 1))(*leaf_index)
        nodes = ctypes.c_uint64()
        self.ctx._check(self.ctx.lib.plonk_kzg_tree_proof_nodes(self.log_n, self.depth, idx, count, ctypes.byref(nodes)))
        vals = ctypes.create_string_buffer(32 * max(count, 1))
        path = ctypes.create_string_buffer(48 * max(nodes.value, 1))
        proof = ctypes.create_string_buffer(96)
        self.ctx._check(self.ctx.lib.plonk_kzg_tree_prove(self.handle, idx, count, label, len(label), _multi_challenges(challenges), vals, path,
                                                          proof))
        return (fr_from_bytes_mont(vals.raw[:32 * count]), [path.raw[48 * j:48 * j + 48] for j in range(nodes.value)], proof.raw)

    def last(self) -> dict:
        info = _KzgTreeInfo()
        self.ctx._check(self.ctx.lib.plonk_kzg_tree_last(self.handle, ctypes.byref(info)))
        return {k: getattr(info, k) for k, _ in info._fields_}

    def close(self):
        if getattr(self, "handle", None):
            if getattr(self.domain, "handle", None) and getattr(self.ctx, "handle", None):
                self.ctx.lib.plonk_kzg_tree_destroy(self.handle)
            self.handle = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


def _mixed_args(items):
    """(verifiers array, nverifiers, circuit, proofs, pi, pi_total, count) of plonk_verify_mixed: one slot per distinct
    Verifier object, in the order of first appearance"""
    items = list(items)
    if not items:
        raise ValueError("empty batch")
    slots, pos = [], {}
    circuit, proofs, pis = [], [], []
    for v, proof, public_inputs in items:
        if id(v) not in pos:
            pos[id(v)] = len(slots)
            slots.append(v)
        if len(proof) != 1008:
            raise ValueError("a proof is 1008 bytes")
        circuit.append(pos[id(v)])
        proofs.append(bytes(proof))
        pis.extend(public_inputs)
    handles = (ctypes.c_void_p * len(slots))(*[v.handle for v in slots])
    circ = (ctypes.c_uint32 * len(circuit))(*circuit)
    pi = fr_to_bytes_mont(pis) if pis else None
    return handles, len(slots), circ, b"".join(proofs), pi, len(pis), len(items)


def verify_mixed(items):
    """plonk_verify_mixed: proofs of several circuits that share one opening key, in one aggregated pairing check.
    items: [(Verifier, proof_bytes, public_inputs)], public_inputs in that verifier's index order.  Returns (verdicts,
    info): per-proof codes as Verifier.verify_batch (0 = valid, -12 PLONK_ERR_VERIFY, -9 PLONK_ERR_DATA, -10
    PLONK_ERR_POINT) and the plonk_verify_info of the call as a dict.  Raises on argument errors (PLONK_ERR_ARG)."""
    items = list(items)
    args = _mixed_args(items)
    ctx = items[0][0].ctx
    verdicts = (ctypes.c_int32 * len(items))()
    info = _VerifyInfo()
    rc = ctx.lib.plonk_verify_mixed(*args, verdicts, ctypes.byref(info))
    if rc not in (PLONK_OK, -12):
        ctx._check(rc)
    return [int(x) for x in verdicts], {k: getattr(info, k) for k, _ in info._fields_}


def verify_each_info(items):
    """plonk_verify_each: every proof checked on its own, one pairing per proof on the device — no batch challenge and no
    bisection, so the cost does not depend on how many proofs are bad.  items as verify_mixed takes them; returns
    (verdicts, info) in the same form.  Raises on argument errors (PLONK_ERR_ARG), never for a bad item."""
    items = list(items)
    args = _mixed_args(items)
    ctx = items[0][0].ctx
    verdicts = (ctypes.c_int32 * len(items))()
    info = _VerifyInfo()
    rc = ctx.lib.plonk_verify_each(*args, verdicts, ctypes.byref(info))
    if rc not in (PLONK_OK, -12):
        ctx._check(rc)
    return [int(x) for x in verdicts], {k: getattr(info, k) for k, _ in info._fields_}


def verify_each(items) -> list:
    """the verdict codes of verify_each_info"""
    return verify_each_info(items)[0]
