"""ctypes binding of ``libprysm_hip.so`` (include/prysm_hip.h).

Loading fails loudly: if the in-tree library is missing, importing a compute entry point
raises ``PzError`` — there is no CPU fallback anywhere in ``prysm_amd``.
"""
import ctypes
import os

import numpy as np

# One HIP runtime per process.  PyTorch-ROCm ships its own libamdhip64 and loads it into the
# global symbol scope at import; when torch is present we import it BEFORE loading our
# library so that libprysm_hip.so binds to that same runtime (device pointers, streams and
# events are then interchangeable with torch's).  Without torch (e.g. a cgo host) the
# library binds to /opt/rocm's runtime.  Initialising two different HIP runtimes in one
# process fails ("No HIP GPUs are available"), so this order is load-bearing.
try:  # pragma: no cover - import side effect only
    import torch  # noqa: F401
    HAVE_TORCH = True
except ImportError:  # pragma: no cover
    HAVE_TORCH = False

HERE = os.path.dirname(os.path.abspath(__file__))
library_path = os.path.join(HERE, "libprysm_hip.so")

PZ_OK = 0
PZ_ENIL = -1
PZ_EINDEX = -2
PZ_ETOOMANY = -3
PZ_EDEVICE = -4
PZ_ENOTFOUND = -5
PZ_EINVAL = -6
PZ_ERANGE = -7

_NAMES = {PZ_ENIL: "ENIL", PZ_EINDEX: "EINDEX", PZ_ETOOMANY: "ETOOMANY", PZ_EDEVICE: "EDEVICE",
          PZ_ENOTFOUND: "ENOTFOUND", PZ_EINVAL: "EINVAL", PZ_ERANGE: "ERANGE"}


class PzError(RuntimeError):
    def __init__(self, code, msg):
        super().__init__("%s (%d): %s" % (_NAMES.get(code, "?"), code, msg))
        self.code = code


c_u8p = ctypes.POINTER(ctypes.c_uint8)
c_u32p = ctypes.POINTER(ctypes.c_uint32)
c_u64p = ctypes.POINTER(ctypes.c_uint64)
c_intp = ctypes.POINTER(ctypes.c_int)
u64 = ctypes.c_uint64
u32 = ctypes.c_uint32
vp = ctypes.c_void_p

# name -> argtypes (all return int status unless listed in _RESTYPES)
SIGNATURES = {
    "pz_init": [ctypes.c_int],
    "pz_device_count": [c_intp],
    "pz_last_error": [],
    "pz_version": [],
    "pz_blake2b512_batch": [vp, vp, u64, vp, u32],
    "pz_set_serial_threshold": [u64],
    "pz_set_host_threads": [u32],
    "pz_chain_set_options": [vp, vp],
    "pz_set_small_batch_threshold": [u64],
    "pz_dev_blake2b512_batch": [vp, vp, u64, vp, u32, vp],
    "pz_dev_blake2b512_spans": [vp, vp, vp, u64, vp, u32, vp],
    "pz_dev_blake2b512_fixed": [vp, u64, u64, u64, vp, u32, vp],
    "pz_validator_indices": [vp, vp, u64, u64, ctypes.c_int, vp, c_u64p],
    "pz_attesters_total_deposit": [vp, u64, c_u64p],
    "pz_calculate_rewards": [vp, vp, vp, u64, u64, u64, vp, vp, u64, c_intp],
    "pz_crosslink_tally": [vp, vp, u64, vp, vp, vp, u64, vp, u64, vp, vp],
    "pz_process_crosslinks": [vp, vp, u64, vp, vp, vp, vp, u64, vp, u64, vp, u64, u64, vp, vp, vp],
    "pz_shuffle_indices": [vp, vp, u64],
    "pz_dev_epoch_count": [vp, vp],
    "pz_dev_epoch_finish": [vp, vp],
    "pz_dev_epoch_gather_compact": [vp, vp, u32, u64, vp, vp],
    "pz_chain_new": [u64, ctypes.c_int, vp],
    "pz_chain_new_comm": [u64, vp, vp],
    "pz_chain_new_from_state": [vp, u64, vp, u64, ctypes.c_int, vp],
    "pz_chain_free": [vp],
    "pz_count_attestations": [vp, vp, u64, c_u64p],
    "pz_chain_process_blocks": [vp, vp, vp, u64, vp, vp, u64],
    "pz_chain_roots": [vp, vp, c_intp],
    "pz_chain_state_bytes": [vp, ctypes.c_int, vp, u64, c_u64p],
    "pz_chain_vote_totals": [vp, vp, vp, u64, c_u64p],
    "pz_chain_phase_times": [vp, vp, ctypes.c_int],
    "pz_dev_vote_tally": [vp, vp],
    "pz_vote_tally": [vp, vp, u64, vp, vp, vp, u64, vp, vp, u64, vp, u64, vp, u64, u64, vp],
    "pz_comm_vote_tally": [vp, vp, vp, u64, vp, vp, vp, u64, vp, vp, u64, vp, u64, vp, u64, u64, vp],
    "pz_wire_validators_bound": [u64, u64],
    "pz_wire_scratch_bytes": [u64],
    "pz_wire_validators": [vp, u64, u32, vp, u64, vp, c_u64p],
    "pz_dev_wire_validators": [vp, u64, u32, vp, vp, vp, vp, vp],
    "pz_check_attestations": [vp],
    "pz_rotate_validator_set": [vp, vp, vp, u64, u64],
    "pz_shuffle_validators_to_committees": [vp, vp, vp, u64, u64, u64, vp, vp, vp, vp, u64, c_u64p],
    "pz_wire_attestations_bound": [u64, u64, u64, u64],
    "pz_wire_attestations_scratch_bytes": [u64],
    "pz_wire_attestations": [vp, u64, u32, vp, u64, vp, c_u64p],
    "pz_dev_wire_attestations": [vp, u64, u32, vp, vp, vp, vp],
    "pz_unwire_attestations_scratch_bytes": [u64],
    "pz_dev_unwire_attestations": [vp, vp, vp, u64, u32, vp, vp, vp, vp],
    "pz_unwire_attestations": [vp, vp, u64, u32, vp, vp, vp],
    "pz_unwire_blocks_scratch_bytes": [u64],
    "pz_dev_unwire_blocks": [vp, vp, u64, u64, vp, vp, vp, vp],
    "pz_unwire_blocks": [vp, vp, u64, u64, vp, c_u64p],
    "pz_dev_check_attestations": [vp, vp],
    "pz_dev_attestation_keys": [vp, u64, vp, vp, u32, vp],
    "pz_attestation_keys": [vp, u64, vp, u32],
    "pz_dev_attestation_messages": [vp, vp],
    "pz_attestation_messages": [vp],
    "pz_vote_cache_new": [u64, u32, ctypes.c_int, vp],
    "pz_vote_cache_free": [vp],
    "pz_vote_cache_scratch_bytes": [u64, u64, u64],
    "pz_dev_vote_cache_tally": [vp, vp, vp, vp],
    "pz_vote_cache_tally": [vp, vp],
    "pz_vote_cache_read": [vp, vp, vp, u64, c_u64p],
    "pz_vote_cache_voters": [vp, vp, vp, c_intp],
    "pz_dev_vote_cache_lookup": [vp, vp, u64, vp, vp, vp],
    "pz_vote_cache_lookup": [vp, vp, u64, vp, vp],
    "pz_vote_cache_capacity": [vp, c_u32p],
    "pz_dev_vote_cache_reserve": [vp, u32, vp],
    "pz_vote_cache_reserve": [vp, u32],
    "pz_vote_cache_retain_scratch_bytes": [u32, u64],
    "pz_dev_vote_cache_retain": [vp, vp, u64, vp, vp],
    "pz_vote_cache_retain": [vp, vp, u64],
    "pz_dev_block_gate": [vp, vp],
    "pz_block_gate": [vp],
    "pz_recent_hashes_new": [vp, vp, u64, ctypes.c_int, vp],
    "pz_recent_hashes_free": [vp],
    "pz_recent_hashes_view": [vp, vp, vp],
    "pz_recent_hashes_read": [vp, vp, vp],
    "pz_dev_recent_hashes_append": [vp, vp, vp, u64, vp],
    "pz_recent_hashes_append": [vp, vp, vp, u64],
    "pz_block_walk_scratch_bytes": [u64, u64],
    "pz_dev_block_walk": [vp, vp, vp],
    "pz_block_walk": [vp, vp],
    "pz_block_cycle_scratch_bytes": [u64, u64],
    "pz_dev_block_cycle": [vp, vp, vp],
    "pz_block_cycle": [vp, vp],
    "pz_block_set_new": [vp, u64, u64, ctypes.c_int, vp],
    "pz_block_set_free": [vp],
    "pz_block_set_count": [vp, vp],
    "pz_block_set_read": [vp, vp, u64, vp],
    "pz_dev_block_set_contains": [vp, vp, u64, vp, vp],
    "pz_block_set_contains": [vp, vp, u64, vp],
    "pz_dev_block_set_insert": [vp, vp, vp, u64, vp],
    "pz_block_set_insert": [vp, vp, vp, u64],
    "pz_dev_block_set_reserve": [vp, u64, vp],
    "pz_block_set_reserve": [vp, u64],
    "pz_block_parents_scratch_bytes": [u64],
    "pz_dev_block_parents": [vp, vp, vp, vp],
    "pz_block_parents": [vp, vp],
    "pz_dev_block_set_insert_walked": [vp, vp, vp, vp, u64, vp, vp],
    "pz_block_store_scratch_bytes": [u64, u64],
    "pz_dev_block_store_select": [vp, vp, vp],
    "pz_dev_block_store_digests": [vp, vp, u64, vp],
    "pz_block_store_select": [vp],
    "pz_block_store_digests": [vp, vp, u64],
    "pz_att_pool_new": [vp, ctypes.c_int, vp],
    "pz_att_pool_free": [vp],
    "pz_att_pool_scratch_bytes": [u64],
    "pz_dev_att_pool_append": [vp, vp, u64, vp, vp, vp, vp, vp],
    "pz_att_pool_append": [vp, vp, u64, vp, vp, vp],
    "pz_dev_att_pool_prune": [vp, u64, vp],
    "pz_att_pool_counts": [vp, vp],
    "pz_att_pool_view": [vp, vp, vp, vp],
    "pz_att_pool_read": [vp, vp, vp, vp],
    "pz_att_pool_shard_block_hashes": [vp, vp, u64, vp, u64, vp],
    "pz_att_pool_capacity": [vp, vp],
    "pz_dev_att_pool_reserve": [vp, vp, vp],
    "pz_att_pool_reserve": [vp, vp],
    "pz_att_pool_need_scratch_bytes": [u64],
    "pz_dev_att_pool_need": [vp, u64, vp, vp, vp, vp, vp, vp],
    "pz_att_pool_need": [vp, u64, vp, vp, vp, vp],
    "pz_recalc_state_new": [u32, u32, vp, vp, vp, vp, vp, ctypes.c_int, vp],
    "pz_recalc_state_free": [vp],
    "pz_recalc_state_read": [vp, vp, vp, vp, vp, vp, vp],
    "pz_state_recalc_scratch_bytes": [u64, u64, u32],
    "pz_dev_state_recalc": [vp, vp, vp, vp, vp, vp],
    "pz_wire_committees_bound": [u64, u64, u64],
    "pz_wire_committees_scratch_bytes": [u64, u64, u64],
    "pz_dev_wire_committees": [vp, u64, u64, u32, vp, vp, vp, vp],
    "pz_wire_committees": [vp, u64, u32, vp, u64, c_u64p],
    "pz_crystallized_state_bound": [u32, u32, u64, u64, u64],
    "pz_crystallized_state_scratch_bytes": [u64],
    "pz_dev_crystallized_state_bytes": [vp, vp, vp, u64, vp, u64, vp, vp, vp, vp],
    "pz_crystallized_state_read": [vp, vp, vp, u64, vp, u64, vp, u64, c_u64p, vp],
    "pz_cstate_head": [vp, u64, vp, vp, vp, vp, vp, vp, u64, c_u64p, c_u64p],
    "pz_cstate_scratch_bytes": [u64],
    "pz_dev_cstate_frame": [vp, u64, u64, vp, vp, vp],
    "pz_dev_cstate_decode": [vp, u64, vp, vp, vp, vp, vp],
    "pz_active_state_bound": [vp, u64],
    "pz_dev_active_state_bytes": [vp, vp, vp, u64, vp, u64, vp, vp],
    "pz_active_state_read": [vp, vp, vp, u64, vp, u64, c_u64p, vp],
    "pz_shutdown": [],
    "pz_state_new": [u64, ctypes.c_int, vp],
    "pz_state_upload": [vp, vp, vp, vp],
    "pz_state_download": [vp, vp, vp, vp],
    "pz_state_validator_indices": [vp, u64, ctypes.c_int, vp, c_u64p],
    "pz_state_calculate_rewards": [vp, u64, u64, vp, vp, u64, c_intp],
    "pz_state_active_balance": [vp, u64, c_u64p],
    "pz_state_free": [vp],
    "pz_comm_unique_id": [vp],
    "pz_comm_init_rank": [vp, ctypes.c_int, ctypes.c_int, ctypes.c_int, vp],
    "pz_init_devices": [ctypes.c_int, vp, vp],
    "pz_comm_init_loopback": [ctypes.c_int, ctypes.c_int, vp],
    "pz_comm_init_shm": [ctypes.c_char_p, ctypes.c_int, ctypes.c_int, ctypes.c_int, u32, vp],
    "pz_comm_set_timing": [vp, ctypes.c_int],
    "pz_comm_collective_time": [vp, vp, vp],
    "pz_comm_size": [vp, c_intp, c_intp, c_intp],
    "pz_comm_device": [vp, ctypes.c_int, c_intp],
    "pz_comm_free": [vp],
    "pz_comm_blake2b512_batch": [vp, vp, vp, u64, vp, u32],
    "pz_epoch_state_new": [vp, ctypes.c_int, vp, vp],
    "pz_epoch_state_new_opts": [vp, ctypes.c_int, vp, vp, vp],
    "pz_epoch_state_step": [vp],
    "pz_epoch_state_sync": [vp],
    "pz_epoch_state_shard": [vp, ctypes.c_int, c_u64p, c_u64p, c_intp, vp],
    "pz_epoch_state_bind_stream": [vp, ctypes.c_int, vp],
    "pz_epoch_state_results": [vp, ctypes.c_int, vp, vp, vp, vp, vp],
    "pz_epoch_state_free": [vp],
    "pz_epoch_state_validators": [vp, ctypes.c_int, vp],
    "pz_epoch_state_layout": [vp, c_intp],
    "pz_epoch_state_columns": [vp, vp, vp],
    "pz_epoch_state_tallies": [vp],
    "pz_epoch_plan": [vp, ctypes.c_int, ctypes.c_int, c_u64p, c_u64p, c_intp],
}


class EpochBatch(ctypes.Structure):
    """Mirror of ``pz_epoch_batch`` (include/prysm_hip.h)."""
    _fields_ = [
        ("ninst", ctypes.c_uint32), ("nval", u64), ("val_offset", u64), ("nval_global", u64),
        ("kind", ctypes.c_int), ("balance", vp), ("start", vp), ("end", vp), ("dynasty", vp),
        ("total_deposit", vp), ("natt", ctypes.c_uint32), ("bits", vp), ("boffs", vp),
        ("max_inst_bytes", u64), ("pop_rank", ctypes.c_uint32), ("pop_world", ctypes.c_uint32),
        ("committee", vp), ("coffs", vp), ("att_comm", vp), ("att_shard", vp),
        ("nrec", ctypes.c_uint32), ("rec_dynasty", vp), ("winner", vp), ("vote", vp), ("total", vp),
        ("scal", vp), ("act_mask", vp), ("blk_cnt", vp), ("act_list", vp), ("scal_next", vp),
        ("cpos", vp), ("co_index", vp),
    ]


class EpochHost(ctypes.Structure):
    """Mirror of ``pz_epoch_host`` (include/prysm_hip.h)."""
    _fields_ = [
        ("ninst", ctypes.c_uint32), ("nval", u64), ("balance", vp), ("start", vp), ("end", vp),
        ("dynasty", vp), ("total_deposit", vp), ("natt", ctypes.c_uint32), ("bits", vp), ("boffs", vp),
        ("committee", vp), ("coffs", vp), ("ncomm", u64), ("att_comm", vp), ("att_shard", vp),
        ("nrec", ctypes.c_uint32), ("rec_dynasty", vp), ("layout", ctypes.c_uint32),
    ]


class ChainOptions(ctypes.Structure):
    """Mirror of ``pz_chain_options`` (include/prysm_hip.h)."""
    _fields_ = [("msg_batch", u64), ("tally_forms", u32)]


TALLY_PER_ATTESTATION, TALLY_BITS_ROWS, TALLY_ID_ROWS = 1, 2, 4  # pz_chain_options.tally_forms


class EpochOptions(ctypes.Structure):
    """Mirror of ``pz_epoch_options`` (include/prysm_hip.h)."""
    _fields_ = [("rebase_period", u64), ("window_only", ctypes.c_int)]


class VoteBatch(ctypes.Structure):
    """Mirror of ``pz_vote_batch`` (include/prysm_hip.h)."""
    _fields_ = [
        ("committee", vp), ("coffs", vp), ("att_comm", vp), ("bits", vp), ("boffs", vp),
        ("item_att", vp), ("item_slot", vp), ("nitems", u64), ("balance", vp), ("nval", u64),
        ("bitmaps", vp), ("words_per_slot", u64), ("totals", vp), ("err", vp),
        ("val_offset", u64), ("nval_global", u64),
    ]


class ValidatorCols(ctypes.Structure):
    """Mirror of ``pz_validator_cols`` (include/prysm_hip.h)."""
    _fields_ = [
        ("public_key", vp), ("withdrawal_shard", vp), ("withdrawal_address", vp),
        ("withdrawal_address_offs", vp), ("randao_commitment", vp), ("randao_commitment_offs", vp),
        ("balance", vp), ("start_dynasty", vp), ("end_dynasty", vp),
    ]


class AttestationCols(ctypes.Structure):
    """Mirror of ``pz_attestation_cols`` (include/prysm_hip.h)."""
    _fields_ = [
        ("slot", vp), ("shard_id", vp), ("justified_slot", vp), ("justified_block_hash", vp),
        ("justified_block_hash_offs", vp), ("shard_block_hash", vp), ("shard_block_hash_offs", vp),
        ("attester_bitfield", vp), ("attester_bitfield_offs", vp), ("oblique_parent_hashes", vp),
        ("oblique_offs", vp), ("oblique_first", vp), ("aggregate_sig", vp), ("aggregate_sig_first", vp),
    ]


class AttestationColsOut(ctypes.Structure):
    """Mirror of ``pz_attestation_cols_out`` (include/prysm_hip.h)."""
    _fields_ = AttestationCols._fields_ + [("n_oblique", vp), ("last_byte", vp), ("status", vp)]


class BlockColsOut(ctypes.Structure):
    """Mirror of ``pz_block_cols_out`` (include/prysm_hip.h)."""
    _fields_ = [
        ("slot_number", vp), ("ts_seconds", vp), ("ts_nanos", vp), ("has_timestamp", vp), ("bytes_beg", vp),
        ("bytes_len", vp), ("att_first", vp), ("att_beg", vp), ("att_end", vp), ("att_block_slot", vp),
        ("att_block", vp), ("status", vp),
    ]


class AttCheckBatch(ctypes.Structure):
    """Mirror of ``pz_att_check_batch`` (include/prysm_hip.h)."""
    _fields_ = [
        ("natt", u64), ("slot", vp), ("justified_slot", vp), ("shard_id", vp), ("n_oblique", vp),
        ("bits", vp), ("boffs", vp), ("block_slot", vp), ("last_justified_slot", u64),
        ("last_state_recalc", u64), ("n_recent", u64), ("narr", u64), ("arr_offs", vp), ("arr_shard", vp),
        ("arr_comm", vp), ("coffs", vp), ("status", vp), ("committee", vp), ("parents_start", vp),
        ("last_byte", vp),
    ]


class AttMsgBatch(ctypes.Structure):
    """Mirror of ``pz_att_msg_batch`` (include/prysm_hip.h)."""
    _fields_ = [
        ("natt", u64), ("slot", vp), ("shard_id", vp), ("shard_block_hash", vp), ("shard_block_hash_offs", vp),
        ("oblique_parent_hashes", vp), ("oblique_offs", vp), ("oblique_first", vp), ("status", vp),
        ("parents_start", vp), ("recent", vp), ("n_recent", u64), ("out", vp), ("msg_len", vp),
    ]


class VoteColsBatch(ctypes.Structure):
    """Mirror of ``pz_vote_cols_batch`` (include/prysm_hip.h)."""
    _fields_ = [
        ("natt", u64), ("n_oblique", vp), ("oblique_parent_hashes", vp), ("oblique_offs", vp), ("oblique_first", vp),
        ("n_oblique_total", u64), ("bits", vp), ("boffs", vp), ("status", vp), ("committee", vp),
        ("parents_start", vp), ("take", vp), ("recent", vp), ("n_recent", u64), ("members", vp), ("coffs", vp),
        ("ncomm", u64), ("balance", vp),
    ]


class BlockGateBatch(ctypes.Structure):
    """Mirror of ``pz_block_gate_batch`` (include/prysm_hip.h)."""
    _fields_ = [
        ("nblocks", u64), ("att_first", vp), ("block_status", vp), ("rec_status", vp), ("candidate", vp),
        ("chk", AttCheckBatch), ("report", vp), ("vote_status", vp), ("pend_take", vp), ("flags", vp),
    ]


class BlockWalkBatch(ctypes.Structure):
    """Mirror of ``pz_block_walk_batch`` (include/prysm_hip.h)."""
    _fields_ = [
        ("nblocks", u64), ("slot_number", vp), ("report", vp), ("block_hash", vp), ("has_candidate", u64),
        ("candidate_slot", u64), ("last_state_recalc", u64), ("lag", u64), ("natt", u64), ("att_block", vp),
        ("vote_status", vp), ("pend_take", vp), ("parents_start", vp), ("walk", vp), ("base", vp), ("result", vp),
        ("log", vp), ("flags", vp),
    ]


class BlockCycleBatch(ctypes.Structure):
    """Mirror of ``pz_block_cycle_batch`` (include/prysm_hip.h)."""
    _fields_ = [
        ("nblocks", u64), ("slot_number", vp), ("report", vp), ("block_hash", vp), ("has_candidate", u64),
        ("candidate_slot", u64), ("last_state_recalc", u64), ("lag", u64), ("natt", u64), ("att_block", vp),
        ("vote_status", vp), ("pend_take", vp), ("parents_start", vp), ("vote0", vp), ("vote1", vp), ("take0", vp),
        ("take1", vp), ("walk", vp), ("base", vp), ("result", vp), ("log", vp), ("flags", vp),
    ]


class BlockParentsBatch(ctypes.Structure):
    """Mirror of ``pz_block_parents_batch`` (include/prysm_hip.h)."""
    _fields_ = [
        ("nblocks", u64), ("bytes", vp), ("nbytes", u64), ("bytes_beg", vp), ("bytes_len", vp), ("slot_number", vp),
        ("block_hash", vp), ("att_first", vp), ("block_status", vp), ("rec_status", vp), ("att_status", vp), ("natt", u64),
        ("parent_ok", vp), ("saved0", vp), ("block_status_out", vp),
    ]


class BlockStoreBatch(ctypes.Structure):
    """Mirror of ``pz_block_store_batch`` (include/prysm_hip.h)."""
    _fields_ = [
        ("nblocks", u64), ("att_first", vp), ("block_status", vp), ("parent_ok", vp), ("stop", vp), ("natt", u64),
        ("att_block", vp), ("att_status", vp), ("rec_status", vp), ("att_beg", vp), ("att_end", vp), ("rows", vp), ("span", vp),
        ("first", vp), ("count", vp), ("bytes", vp), ("nbytes", u64), ("key", vp), ("hash", vp), ("lists", vp),
    ]


class RecalcBatch(ctypes.Structure):
    """Mirror of ``pz_recalc_batch`` (include/prysm_hip.h)."""
    _fields_ = [
        ("nval", u64), ("balance", vp), ("start", vp), ("end", vp), ("members", vp), ("coffs", vp), ("recent", vp),
        ("n_recent", u64), ("block_slot", u64),
    ]


class CommitteeTable(ctypes.Structure):
    """Mirror of ``pz_committee_table`` (include/prysm_hip.h)."""
    _fields_ = [("narr", u64), ("arr_offs", vp), ("arr_shard", vp), ("arr_comm", vp), ("ncomm", u64), ("coffs", vp),
                ("members", vp)]


class ValidatorColsOut(ctypes.Structure):
    """Mirror of ``pz_validator_cols_out`` (include/prysm_hip.h)."""
    _fields_ = ValidatorCols._fields_


class CommitteeTableOut(ctypes.Structure):
    """Mirror of ``pz_committee_table_out`` (include/prysm_hip.h)."""
    _fields_ = CommitteeTable._fields_


class CstateRest(ctypes.Structure):
    """Mirror of ``pz_cstate_rest`` (include/prysm_hip.h)."""
    _fields_ = [("crosslinking_start_shard", u64), ("dynasty_seed", ctypes.c_uint8 * 64), ("dynasty_seed_len", u32),
                ("dynasty_seed_last_reset", u64)]


RS_LAST_STATE_RECALC, RS_JUSTIFIED_STREAK, RS_LAST_JUSTIFIED_SLOT, RS_LAST_FINALIZED_SLOT, RS_CURRENT_DYNASTY, \
    RS_TOTAL_DEPOSITS = range(6)  # pz_recalc_state's scalars
RS_COUNT = 8
CSF_STATUS, CSF_OFFSET, CSF_NVAL, CSF_ADDRESS_BYTES, CSF_COMMITMENT_BYTES, CSF_NARR, CSF_NENTRIES, CSF_NMEMBERS, CSF_VAL_END, \
    CSF_F12_END = range(10)  # pz_dev_cstate_frame's result record
CSF_COUNT = 12
CSTATE_RECORD_LIMIT, CSTATE_TILE_BYTES, CSTATE_GROUP_TILES = 510, 4096, 64  # PZ_CSTATE_*
SCAL_POP, SCAL_NACT, SCAL_ERR_XL, SCAL_ERR_RWD, SCAL_APPLIED, SCAL_NEXT_BAL, SCAL_MAXIDX1, SCAL_NOMATCH = range(8)
SCAL_COUNT = 8
KIND_ACTIVE, KIND_EXITED, KIND_QUEUED = 0, 1, 2
_RESTYPES = {"pz_last_error": ctypes.c_char_p, "pz_chain_free": None, "pz_set_serial_threshold": u64, "pz_set_host_threads": u32,
             "pz_shutdown": None, "pz_state_free": None, "pz_set_small_batch_threshold": u64, "pz_comm_free": None, "pz_epoch_state_free": None,
             "pz_wire_validators_bound": u64, "pz_wire_scratch_bytes": u64,
             "pz_wire_attestations_bound": u64, "pz_wire_attestations_scratch_bytes": u64,
             "pz_unwire_attestations_scratch_bytes": u64, "pz_unwire_blocks_scratch_bytes": u64,
             "pz_vote_cache_free": None, "pz_vote_cache_scratch_bytes": u64, "pz_vote_cache_retain_scratch_bytes": u64,
             "pz_att_pool_free": None, "pz_att_pool_scratch_bytes": u64, "pz_att_pool_need_scratch_bytes": u64,
             "pz_recent_hashes_free": None, "pz_block_walk_scratch_bytes": u64,
             "pz_block_cycle_scratch_bytes": u64,
             "pz_block_set_free": None, "pz_block_parents_scratch_bytes": u64, "pz_block_store_scratch_bytes": u64,
             "pz_recalc_state_free": None, "pz_state_recalc_scratch_bytes": u64,
             "pz_wire_committees_bound": u64, "pz_wire_committees_scratch_bytes": u64,
             "pz_crystallized_state_bound": u64, "pz_crystallized_state_scratch_bytes": u64, "pz_active_state_bound": u64,
             "pz_cstate_scratch_bytes": u64}
SERIAL_DEFAULT = 65536        # the library's default serial threshold (bytes)
SERIAL_ON_GPU = (1 << 64) - 1  # pz_set_serial_threshold value that keeps every message on the GPU


class _Lib:
    def __init__(self):
        self._dll = None

    def _load(self):
        if self._dll is None:
            # the in-tree product build; no environment switch selects another one (tests marked
            # `ab` and tools/ point library_path at the A/B library before the first call)
            path = library_path
            if not os.path.exists(path):
                raise PzError(PZ_EDEVICE, "HIP library not built: %s (run __graft_entry__.build())" % path)
            dll = ctypes.CDLL(path)
            for name, args in SIGNATURES.items():
                fn = getattr(dll, name)
                fn.argtypes = args
                fn.restype = _RESTYPES.get(name, ctypes.c_int)
            self._dll = dll
        return self._dll

    @property
    def dll(self):
        return self._load()

    def call(self, name, *args):
        rc = getattr(self._load(), name)(*args)
        if rc != PZ_OK:
            raise PzError(rc, self._load().pz_last_error().decode())
        return rc


lib = _Lib()


def ptr(a):
    """Host pointer of a C-contiguous numpy array (None for empty)."""
    if a is None:
        return None
    assert a.flags["C_CONTIGUOUS"]
    return a.ctypes.data if a.size else None


def dptr(t):
    """Device address of a torch tensor (None for None and for an empty one)."""
    return t.data_ptr() if t is not None and t.numel() else None


def stream_ptr(device):
    """The current torch stream of ``device`` (an index or a ``torch.device``) as the ABI's ``void*``."""
    import torch

    dev = torch.device("cuda", device) if isinstance(device, int) else device
    return ctypes.c_void_p(torch.cuda.current_stream(dev).cuda_stream)


ATT_COLS = tuple(k for k, _ in AttestationCols._fields_)
_ATT_DATA = ("justified_block_hash", "shard_block_hash", "attester_bitfield", "oblique_parent_hashes", "aggregate_sig")


def att_cols(cols, keys=ATT_COLS):
    """``AttestationCols`` over the columns of ``cols`` named by ``keys``: numpy arrays (host
    addresses) or torch tensors (device addresses).  A missing, None or empty column is NULL, with
    one exception: a data column with no entry still needs an address, since the entry points refuse
    offsets without their data column, so it gets a one-entry placeholder.  The struct keeps what
    its addresses point into alive (``_keep``)."""
    c = AttestationCols()
    c._keep = []
    for k in keys:
        v = cols.get(k)
        if v is None:
            continue
        host = not hasattr(v, "data_ptr")
        v = np.ascontiguousarray(v) if host else v
        if k in _ATT_DATA and not (v.size if host else v.numel()):
            v = np.zeros(1, dtype=v.dtype) if host else v.new_zeros(1)
        if v.size if host else v.numel():
            setattr(c, k, v.ctypes.data if host else v.data_ptr())
            c._keep.append(v)
    return c


class Handle:
    """A resident handle of the library: the ``void*`` ``_new`` fills, freed by the entry point
    named ``_FREE`` when the object goes.  ``_STICKY``: the codes of the handle's sticky errors."""
    _FREE = None
    _STICKY = ()

    def _new(self, name, *args):
        self._h = ctypes.c_void_p()
        lib.call(name, *args, ctypes.byref(self._h))

    def __del__(self):
        h = getattr(self, "_h", None)
        if h is not None and h.value:
            getattr(lib.dll, self._FREE)(h)
            self._h = None

    def _rc(self, rc, strict=True, sticky_codes=None):
        """Raises unless ``rc`` is PZ_OK, or a sticky code while ``strict`` is off."""
        if rc != PZ_OK and (strict or rc not in (self._STICKY if sticky_codes is None else sticky_codes)):
            raise PzError(rc, lib.dll.pz_last_error().decode())


def as_u8(buf):
    return np.frombuffer(bytes(buf), dtype=np.uint8) if not isinstance(buf, np.ndarray) else buf


def blake2b512_batch(messages, out_bytes=32):
    """Hash a list of byte strings on the GPU; returns a list of ``out_bytes``-byte digests."""
    n = len(messages)
    if n == 0:
        return []
    offsets = np.zeros(n + 1, dtype=np.uint64)
    offsets[1:] = np.cumsum([len(m) for m in messages], dtype=np.uint64)
    data = np.frombuffer(b"".join(bytes(m) for m in messages) + b"\0" * 16, dtype=np.uint8)
    out = np.empty(n * out_bytes, dtype=np.uint8)
    lib.call("pz_blake2b512_batch", ptr(data), ptr(offsets), n, ptr(out), out_bytes)
    raw = out.tobytes()
    return [raw[i * out_bytes:(i + 1) * out_bytes] for i in range(n)]


def blake2b512_csr(data, offsets, out_bytes=32):
    """Hash CSR messages (numpy uint8 data, uint64 offsets[n+1]); returns (n, out_bytes) uint8."""
    n = len(offsets) - 1
    out = np.empty((max(n, 0), out_bytes), dtype=np.uint8)
    if n > 0:
        data = np.ascontiguousarray(data, dtype=np.uint8)
        offsets = np.ascontiguousarray(offsets, dtype=np.uint64)
        lib.call("pz_blake2b512_batch", ptr(data), ptr(offsets), n, ptr(out), out_bytes)
    return out


def set_serial_threshold(nbytes):
    """Messages of at least ``nbytes`` bytes are hashed on host threads by the batch entry
    points (serial chains); ``SERIAL_ON_GPU`` keeps all of them on the GPU.
    Returns the previous threshold."""
    return int(lib.dll.pz_set_serial_threshold(nbytes))


def serial_threshold_default():
    return SERIAL_DEFAULT


SMALL_BATCH_DEFAULT = 256  # compressions (serial_hash.h PZ_SMALL_BATCH_DEFAULT)


class small_batch_threshold:
    """Context manager: batches of at most ``compressions`` compressions are hashed on the
    calling thread (0: every batch on the GPU)."""

    def __init__(self, compressions):
        self.c = compressions

    def __enter__(self):
        self.old = int(lib.dll.pz_set_small_batch_threshold(self.c))
        return self

    def __exit__(self, *exc):
        lib.dll.pz_set_small_batch_threshold(self.old)


class serial_threshold:
    """Context manager form of :func:`set_serial_threshold`."""

    def __init__(self, nbytes):
        self.nbytes = nbytes

    def __enter__(self):
        self.old = set_serial_threshold(self.nbytes)
        return self

    def __exit__(self, *exc):
        set_serial_threshold(self.old)
