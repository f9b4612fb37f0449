/*
 * prysm_hip.h — C ABI of the MI355X-native state-transition hot path.
 *
 * This is the drop-in boundary: the entry points a cgo shim inside the reference's Go
 * packages would bind.  Every function is `extern "C"`, takes plain
 * pointers and sizes, never retains a caller pointer after it returns, and is thread-safe
 * (per-device mutex; one library-owned HIP stream per device for the host-pointer API).
 *
 * Two flavours:
 *   pz_*      host pointers, synchronous (the Go-API drop-in; data is copied H2D/D2H);
 *   pz_dev_*  device pointers, enqueued on the caller's hipStream_t (passed as void*),
 *             asynchronous; used by the device-resident mirror and the benchmark.
 *
 * Paths below are relative to the reference tree (/root/reference).  All arithmetic is
 * integer and bit-exact with the Go reference (uint64 wrap-around, MSB-first bitfields).
 *
 * The library fails loudly: if no gfx950 device is usable every compute entry point
 * returns PZ_EDEVICE; there is no CPU fallback.
 */
#ifndef PRYSM_HIP_H
#define PRYSM_HIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* ---- status codes ------------------------------------------------------------------ */
#define PZ_OK         0
#define PZ_ENIL      -1  /* nil message: Go returns a proto.ErrNil-wrapped error (types/block_test.go:37-43) */
#define PZ_EINDEX    -2  /* Go index-out-of-range panic (CheckBit / committee / record index) */
#define PZ_ETOOMANY  -3  /* > params.MaxValidators (utils/shuffle.go:15-17) */
#define PZ_EDEVICE   -4  /* HIP failure or no usable gfx950 device */
#define PZ_ENOTFOUND -5  /* committee lookup failed: Go error (blockchain/core.go:373) */
#define PZ_EINVAL    -6  /* malformed arguments (null pointer with n > 0, bad sizes) */
#define PZ_ERANGE    -7  /* slice bounds out of range (Go panic, blockchain/core.go:353) */

/* params/config.go:4-26 */
#define PZ_ATTESTER_REWARD      1ULL
#define PZ_CYCLE_LENGTH         64
#define PZ_SHARD_COUNT          1024
#define PZ_DEFAULT_BALANCE      32ULL
#define PZ_MAX_VALIDATORS       4194304ULL
#define PZ_MIN_COMMITTEE_SIZE   128
#define PZ_DEFAULT_END_DYNASTY  9999999999999999999ULL

/* ---- runtime ------------------------------------------------------------------------ */
int         pz_init(int device);          /* select/initialise a device for this thread */
int         pz_device_count(int* count);
const char* pz_last_error(void);          /* thread-local message for the last failure */
int         pz_version(void);             /* ABI version: 1 */
/* Releases every device context the library created (streams, staging buffers).  Call it
 * last, from one thread, after every pz_chain / pz_epoch_state / pz_comm has been freed;
 * afterwards any entry point re-initialises lazily.  (The reference has no teardown: the Go
 * process exits; a long-lived cgo host calls this on node shutdown, node/node.go:124-132.) */
void        pz_shutdown(void);

/* ---- H: BLAKE2b-512 of serialized messages ------------------------------------------
 * Replaces `h := blake2b.Sum512(data); copy(hash[:], h[:32])` at
 *   types/block.go:73-76          (*Block).Hash
 *   types/attestation.go:55-58    (*Attestation).Hash
 *   types/attestation.go:74-76    (*Attestation).Key
 *   types/state.go:145-148        (*ActiveState).Hash
 *   types/state.go:244-247        (*CrystallizedState).Hash
 *   blockchain/core.go:290        processAttestation message hash (keeps all 64 bytes)
 *   utils/shuffle.go:19           ShuffleIndices seed stream (keeps all 64 bytes)
 * Messages are CSR: message i is msgs[offsets[i] .. offsets[i+1]); offsets has n+1 entries.
 * out receives n * out_bytes bytes (out_bytes = 32: the hot path's truncated digest; 64: full).
 */
int pz_blake2b512_batch(const uint8_t* msgs, const uint64_t* offsets, uint64_t n,
                        uint8_t* out, uint32_t out_bytes);

/* Long single messages (a state root is one serial chain of up to 221,844 compressions at
 * 1M validators) cannot use more than one lane: the batch entry points above hash every
 * message of at least `bytes` bytes on host threads (AVX2), concurrently with the GPU launch
 * for the rest of the batch.  Default 65,536; UINT64_MAX keeps everything on
 * the GPU.  Returns the previous value.  The pz_dev_* forms never leave the device. */
uint64_t pz_set_serial_threshold(uint64_t bytes);
/* Host threads the library uses beside the GPU (the serial hashes of long messages, the chain
 * engine's parse and result copies): 0 (the default) min(16, the process's CPU affinity), else n
 * (at most 256).  Returns the previous setting.  A placement control, not a reference API. */
uint32_t pz_set_host_threads(uint32_t n);

/* A batch of at most `compressions` BLAKE2b compressions in all (a drop-in Hash() call: one
 * 100-600 B message is 1-5) is hashed on the calling thread: the GPU route's launch, PCIe
 * copies and stream sync cost tens of microseconds against ~1 us of host work (DESIGN.md §3,
 * the measured crossover).  0 sends every batch to the GPU.  Returns the previous value.
 * The library still refuses to run without a gfx950 device. */
uint64_t pz_set_small_batch_threshold(uint64_t compressions);

/* Device-resident forms (device pointers; caller's stream).  The CSR form requires 4
 * readable bytes past msgs[offsets[n]-1] (the library's own buffers are padded). */
int pz_dev_blake2b512_batch(const uint8_t* d_msgs, const uint64_t* d_offsets, uint64_t n,
                            uint8_t* d_out, uint32_t out_bytes, void* stream);
/* Messages where they lie: message i is d_msgs[d_begs[i] .. d_ends[i]); spans may overlap or
 * leave gaps (the CSR form is d_offsets, d_offsets + 1), with the same 4 readable bytes past
 * the last one.  Over pz_block_cols_out's att_beg / att_end this is types/attestation.go:55-58
 * (*Attestation).Hash of every attestation of a batch of received blocks, in one launch. */
int pz_dev_blake2b512_spans(const uint8_t* d_msgs, const uint64_t* d_begs, const uint64_t* d_ends, uint64_t n,
                            uint8_t* d_out, uint32_t out_bytes, void* stream);
/* Fixed-length records: message i is d_msgs[i*stride .. i*stride+len); stride % 16 == 0,
 * d_msgs 16-byte aligned, stride >= len.  This is the batched-record fast path.  The kernels
 * load whole aligned chunks, so the buffer must be readable up to the end of the last
 * record's chunk: (n-1)*stride + 128*ceil(len/128) bytes when stride >= 128*ceil(len/128)
 * (the LDS-staged path), (n-1)*stride + 16*ceil(len/16) otherwise; a buffer of n*stride
 * bytes with stride a multiple of 128 always suffices; with len == 0 nothing is read.  Bytes
 * past len never affect a digest. */
int pz_dev_blake2b512_fixed(const uint8_t* d_msgs, uint64_t stride, uint64_t len, uint64_t n,
                            uint8_t* d_out, uint32_t out_bytes, void* stream);

/* ---- a2 / §8f: proto3 encoding of ValidatorRecords on the device -------------------
 * Replaces the validators span of gogo proto.Marshal(CrystallizedState) at
 * types/state.go:141 (Marshal) and :240 (Hash); record layout messages.pb.go:803-809.
 * Columns are SoA; a NULL scalar column means 0 in every record (omitted, as proto3 omits
 * zero scalars); a bytes column is CSR (data + offsets[n+1]), NULL offsets = all empty.
 * field_num > 0 frames every record as that length-delimited field (11 = the
 * CrystallizedState's `validators`); 0 writes bare records (then offsets delimit them).
 * offsets (optional, n+1) receive each record's start in out; offsets[n] = total length. */
typedef struct pz_validator_cols {
  const uint64_t* public_key;              /* field 1 */
  const uint64_t* withdrawal_shard;        /* field 2 */
  const uint8_t*  withdrawal_address;      /* field 3 (bytes) */
  const uint64_t* withdrawal_address_offs;
  const uint8_t*  randao_commitment;       /* field 4 (bytes) */
  const uint64_t* randao_commitment_offs;
  const uint64_t* balance;                 /* field 5 */
  const uint64_t* start_dynasty;           /* field 6 */
  const uint64_t* end_dynasty;             /* field 7 */
} pz_validator_cols;
/* Upper bound of the encoded length (bytes_total = both bytes columns' total length). */
uint64_t pz_wire_validators_bound(uint64_t n, uint64_t bytes_total);
/* Device scratch the pz_dev_ form needs for n records. */
uint64_t pz_wire_scratch_bytes(uint64_t n);
/* Host pointers, synchronous.  PZ_ERANGE (nothing written) when the encoding exceeds cap;
 * *len always receives the encoded length. */
int pz_wire_validators(const pz_validator_cols* v, uint64_t n, uint32_t field_num, uint8_t* out,
                       uint64_t cap, uint64_t* offsets, uint64_t* len);
/* Device pointers (columns included), caller's stream.  d_out must hold
 * pz_wire_validators_bound(...) bytes; *d_total (device) receives the length.  Nothing outside
 * d_out[0, *d_total) is written: not the rest of the bound, not a byte before d_out, whatever
 * d_out's alignment; with n == 0 d_out is not touched and may be NULL.  d_scratch need not be
 * cleared: every call resets what it uses. */
int pz_dev_wire_validators(const pz_validator_cols* v, uint64_t n, uint32_t field_num, uint8_t* d_out,
                           uint64_t* d_offsets, void* d_scratch, uint64_t* d_total, void* stream);

/* ---- a2 / §8f: proto3 encoding of AttestationRecords on the device -------------------
 * Replaces golang/protobuf proto.Marshal(AttestationRecord) at types/attestation.go:51,56
 * (and the records inside BeaconBlock field 8, block.go:69, and ActiveState field 1,
 * state.go:141); record layout messages.pb.go:889-896.  Scalars: NULL = 0 everywhere.
 * Bytes fields: CSR (data + offsets[n+1]; NULL offsets = empty).  oblique_parent_hashes: an
 * element CSR (data + oblique_offs[m+1]) and the element range of record i,
 * oblique_first[i] .. oblique_first[i+1] (NULL = none).  aggregate_sig: values and the range
 * of record i, aggregate_sig_first[i] .. [i+1] (NULL = none).  field_num frames each record
 * (8: BeaconBlock.attestations, 1: ActiveState.pending_attestations; 0: bare records, the
 * bytes Attestation.Hash() hashes).  offsets[i] = start of record i, offsets[n] = length. */
typedef struct pz_attestation_cols {
  const uint64_t* slot;                    /* field 1 */
  const uint64_t* shard_id;                /* field 2 */
  const uint64_t* justified_slot;          /* field 3 */
  const uint8_t*  justified_block_hash;    /* field 4 */
  const uint64_t* justified_block_hash_offs;
  const uint8_t*  shard_block_hash;        /* field 5 */
  const uint64_t* shard_block_hash_offs;
  const uint8_t*  attester_bitfield;       /* field 6 */
  const uint64_t* attester_bitfield_offs;
  const uint8_t*  oblique_parent_hashes;   /* field 7 */
  const uint64_t* oblique_offs;
  const uint64_t* oblique_first;
  const uint64_t* aggregate_sig;           /* field 8 */
  const uint64_t* aggregate_sig_first;
} pz_attestation_cols;
uint64_t pz_wire_attestations_bound(uint64_t n, uint64_t bytes_total, uint64_t n_oblique, uint64_t n_sig);
uint64_t pz_wire_attestations_scratch_bytes(uint64_t n);
/* Host pointers, synchronous; ranges must start at 0.  PZ_ERANGE when the encoding exceeds
 * cap (*len still receives its length). */
int pz_wire_attestations(const pz_attestation_cols* a, uint64_t n, uint32_t field_num, uint8_t* out,
                         uint64_t cap, uint64_t* offsets, uint64_t* len);
/* Device pointers, caller's stream; d_out holds pz_wire_attestations_bound(...) bytes,
 * d_offsets n+1 entries (required).  Nothing outside d_out[0, d_offsets[n]) is written: not the
 * rest of the bound, not a byte before d_out, whatever d_out's alignment.  Ranges need not start
 * at 0 here; d_scratch need not be cleared: every call resets what it uses. */
int pz_dev_wire_attestations(const pz_attestation_cols* a, uint64_t n, uint32_t field_num, uint8_t* d_out,
                             uint64_t* d_offsets, void* d_scratch, void* stream);

/* ---- §8f: proto3 decoding of AttestationRecords on the device -------------------------
 * The inverse of pz_wire_attestations.  Replaces golang/protobuf proto.Unmarshal of the
 * AttestationRecords (messages.pb.go:889-896) of a received BeaconBlock (sync/service.go:147-164)
 * and of a stored ActiveState (types/state.go:141's inverse), under the engine's rule that an
 * input is accepted only if it is the canonical encoding of its own decoding (types/block.go:69
 * hashes Marshal of the DECODED message): minimal varints for keys, values and lengths (a
 * 10-byte varint ends in 0x01, nothing is longer), fields 1-8 with their wire types only,
 * ascending, only field 7 repeating and only in a run, zero scalars and empty singular bytes
 * absent, empty field-7 elements allowed, field 8 packed, non-empty, every varint in it whole
 * and minimal, no length reaching past the record.
 * Record i is bytes[begs[i] .. ends[i]) (a CSR batch passes offsets and offsets + 1).
 * field_num == 0: a bare record; field_num > 0: the span starts with that field's key and a
 * minimal length that covers exactly the rest of the span (what pz_wire_attestations emits).
 * A record that fails gets status[i] = PZ_EINVAL, scalars 0 and empty ranges in every offsets
 * column, so the other records' columns are what they would be without it; the call returns
 * PZ_OK.  totals[7]: justified_block_hash bytes, shard_block_hash bytes, bitfield bytes,
 * elements, element bytes, sig values, bad records.
 * Output bounds, with B the batch's byte count (the sum of the spans): every bytes column
 * (the elements' included) holds B bytes, oblique_offs B/2 + 1 entries (an element takes two
 * bytes at least), aggregate_sig B values (a value takes one), every other offsets column n+1.
 * The kernels read no byte outside the spans (the contract allows up to 16 bytes after the last
 * byte of the buffer, as the hash kernels' pad; this form reads none) and write only inside the
 * ranges their scans assign. */
typedef struct pz_attestation_cols_out {
  uint64_t* slot;                          /* n */
  uint64_t* shard_id;
  uint64_t* justified_slot;
  uint8_t*  justified_block_hash;
  uint64_t* justified_block_hash_offs;     /* n+1 */
  uint8_t*  shard_block_hash;
  uint64_t* shard_block_hash_offs;
  uint8_t*  attester_bitfield;
  uint64_t* attester_bitfield_offs;
  uint8_t*  oblique_parent_hashes;
  uint64_t* oblique_offs;                  /* m+1, m = oblique_first[n] */
  uint64_t* oblique_first;                 /* n+1 */
  uint64_t* aggregate_sig;
  uint64_t* aggregate_sig_first;           /* n+1 */
  uint64_t* n_oblique;                     /* optional, n: pz_att_check_batch.n_oblique */
  uint8_t*  last_byte;                     /* optional, n: pz_att_check_batch.last_byte (0 when the
                                              bitfield is empty) */
  int32_t*  status;                        /* n: PZ_OK, or PZ_EINVAL for a record that is not canonical */
} pz_attestation_cols_out;
uint64_t pz_unwire_attestations_scratch_bytes(uint64_t n);
/* Device pointers, caller's stream; d_totals (device) receives the seven totals. */
int pz_dev_unwire_attestations(const uint8_t* d_bytes, const uint64_t* d_begs, const uint64_t* d_ends,
                               uint64_t n, uint32_t field_num, const pz_attestation_cols_out* out,
                               uint64_t* d_totals, void* d_scratch, void* stream);
/* Host pointers, synchronous; offsets[n+1].  caps: the capacities of justified_block_hash,
 * shard_block_hash, attester_bitfield (bytes), oblique_offs (elements; it holds one entry
 * more), oblique_parent_hashes (bytes) and aggregate_sig (values).  PZ_ERANGE, nothing
 * written, when a total exceeds its capacity; totals is filled either way. */
int pz_unwire_attestations(const uint8_t* bytes, const uint64_t* offsets, uint64_t n, uint32_t field_num,
                           const pz_attestation_cols_out* out, const uint64_t caps[6], uint64_t totals[7]);

/* ---- §8f: the top level of serialized BeaconBlocks on the device ------------------------
 * Replaces proto.Unmarshal(BeaconBlock) at sync/service.go:147-164 (messages.pb.go:224-232)
 * down to the attestations' spans, which pz_dev_unwire_attestations decodes where they lie
 * (field_num 0 over att_beg / att_end).  Block i is blocks[offsets[i] .. offsets[i+1]).  The
 * rules are the ones above for fields 1-8 of the block (1, 3-6 bytes, 2 varint, 7 Timestamp,
 * 8 repeated records) and for the Timestamp (seconds 1, nanos 2: an int32, so its varint is
 * the sign extension of its low 32 bits); a bytes field of 4 GiB or more does not fit
 * bytes_len and fails too.  A block that fails has status PZ_EINVAL, zero fields and no
 * attestations.  The records' bodies are not judged here: a block is acceptable to the engine
 * when its status and every one of its attestations' statuses are PZ_OK.
 * Attestation rows past att_cap are not written; *natt receives their true number. */
typedef struct pz_block_cols_out {
  uint64_t* slot_number;                   /* n */
  int64_t*  ts_seconds;                    /* n */
  int64_t*  ts_nanos;                      /* n */
  uint8_t*  has_timestamp;                 /* n: field 7 present (it may be present and empty) */
  uint64_t* bytes_beg;                     /* n*5: fields 1, 3, 4, 5, 6 of block i at [5i .. 5i+5) */
  uint32_t* bytes_len;                     /* n*5: spans into blocks (len 0 = absent) */
  uint64_t* att_first;                     /* n+1: block i's attestations are rows att_first[i] .. [i+1] */
  uint64_t* att_beg;                       /* per attestation: its bare record inside blocks */
  uint64_t* att_end;
  uint64_t* att_block_slot;                /* per attestation: pz_att_check_batch.block_slot */
  uint32_t* att_block;                     /* per attestation: its block's index */
  int32_t*  status;                        /* n: PZ_OK / PZ_EINVAL */
} pz_block_cols_out;
uint64_t pz_unwire_blocks_scratch_bytes(uint64_t n);
/* Device pointers, caller's stream; *d_natt (device) receives the number of attestations. */
int pz_dev_unwire_blocks(const uint8_t* d_blocks, const uint64_t* d_offsets, uint64_t n, uint64_t att_cap,
                         const pz_block_cols_out* out, uint64_t* d_natt, void* d_scratch, void* stream);
/* Host pointers, synchronous, same results.  PZ_ERANGE (nothing written, *natt filled) when
 * att_cap is short. */
int pz_unwire_blocks(const uint8_t* blocks, const uint64_t* offsets, uint64_t n, uint64_t att_cap,
                     const pz_block_cols_out* out, uint64_t* natt);

/* ---- T/R: validator-set filters (casper/validator.go) ------------------------------- */
#define PZ_KIND_ACTIVE 0  /* start <= dyn < end        casper/validator.go:45-53 */
#define PZ_KIND_EXITED 1  /* start <  dyn && end <= dyn casper/validator.go:57-65 */
#define PZ_KIND_QUEUED 2  /* start >  dyn               casper/validator.go:69-77 */
/* out (capacity n) receives the ascending indices; *count their number (0 == Go nil). */
int pz_validator_indices(const uint64_t* start_dynasty, const uint64_t* end_dynasty, uint64_t n,
                         uint64_t dynasty, int kind, uint32_t* out, uint64_t* count);

/* casper/validator.go:93-102 GetAttestersTotalDeposit: popcount of every pending
 * attestation's bitfield bytes (concatenated) x DefaultBalance. */
int pz_attesters_total_deposit(const uint8_t* bits, uint64_t nbytes, uint64_t* out);

/* casper/incentives.go:14-32 CalculateRewards, in place on balance[n].
 * Pending attestations are CSR bitfields (bits, boffs[natt+1]); the reward bit for rank i
 * is CheckBit(last bitfield, active[i]) and the target is balance[i] (rank, not index).
 * Returns PZ_EINDEX (balances untouched) where Go would panic. *applied = 1 when the
 * 2/3 threshold held. */
int pz_calculate_rewards(uint64_t* balance, const uint64_t* start_dynasty,
                         const uint64_t* end_dynasty, uint64_t n, uint64_t dynasty,
                         uint64_t total_deposit, const uint8_t* bits, const uint64_t* boffs,
                         uint64_t natt, int* applied);

/* blockchain/core.go:515-545 processCrosslinks tallies: for attestation a with committee
 * c = att_committee[a] (members committee[coffs[c] .. coffs[c+1])):
 *   total[a] = sum balance[member], vote[a] = sum balance[member] * CheckBit(bits_a, pos). */
int pz_crosslink_tally(const uint32_t* committee, const uint64_t* coffs, uint64_t ncomm,
                       const uint32_t* att_committee, const uint8_t* bits, const uint64_t* boffs,
                       uint64_t natt, const uint64_t* balance, uint64_t nval,
                       uint64_t* vote_out, uint64_t* total_out);

/* blockchain/core.go:502-558 processCrosslinks, complete: tallies as above, then the in-order
 * winner rule — for each shard the FIRST attestation with 3*vote >= 2*total (uint64 wrap)
 * and dynasty > rec_dynasty[shard] wins.  winner[s] (capacity nrec) receives the winning
 * attestation index or UINT32_MAX; the caller rewrites records[s] = {dynasty, that
 * attestation's ShardBlockHash, slot}.  PZ_EINDEX where Go would panic. */
int pz_process_crosslinks(const uint32_t* committee, const uint64_t* coffs, uint64_t ncomm,
                          const uint32_t* att_committee, const uint32_t* att_shard,
                          const uint8_t* bits, const uint64_t* boffs, uint64_t natt,
                          const uint64_t* balance, uint64_t nval, const uint64_t* rec_dynasty,
                          uint64_t nrec, uint64_t dynasty, uint32_t* winner,
                          uint64_t* vote_out, uint64_t* total_out);

/* utils/shuffle.go:14-33 ShuffleIndices, in place.  Host-resident by design (a sequential
 * swap chain, north_star); the 64-byte seed stream blake2b.Sum512(seed) goes through the batch
 * hash API (one compression: the small-batch route).  While n - i > 255 every swap target is
 * i + a fixed byte offset, so the chain runs division-free in a 256-entry window. */
int pz_shuffle_indices(const uint8_t seed[32], uint32_t* list, uint64_t n);

/* casper/validator.go:17-41 RotateValidatorSet, in place on start/end: active validators
 * below DefaultBalance/2 exit (end = dynasty); then the first min(len(active)/30 + 1,
 * len(queued)) queued validators, by ascending index, start (start = dynasty).  The active
 * count, the exits and the queued list run on the device filter kernels. */
int pz_rotate_validator_set(const uint64_t* balance, uint64_t* start, uint64_t* end, uint64_t n,
                            uint64_t dynasty);

/* casper/sharding.go:11-53 ShuffleValidatorsToCommittees: active indices (device filter),
 * ShuffleIndices (host swap chain), then splitBySlotShard into CSR: slot s (0..63) holds
 * committees slot_offs[s] .. slot_offs[s+1]; committee c has shard shard_id[c] and members
 * members[coffs[c] .. coffs[c+1]].  members needs room for n, coffs for cap_comm+1 and shard_id
 * for cap_comm entries, slot_offs for 65; PZ_ERANGE (with *ncomm = the count needed) when
 * cap_comm is short, PZ_ETOOMANY above MaxValidators (utils/shuffle.go:15-17). */
int pz_shuffle_validators_to_committees(const uint8_t seed[32], const uint64_t* start, const uint64_t* end,
                                        uint64_t n, uint64_t dynasty, uint64_t crosslink_start_shard,
                                        uint32_t* members, uint64_t* coffs, uint64_t* shard_id,
                                        uint64_t* slot_offs, uint64_t cap_comm, uint64_t* ncomm);

/* ---- a device-resident mirror of the validator set (SURVEY.md §8b "Ownership") ----------
 * The Go APIs take []*pb.ValidatorRecord, so every host-pointer casper call above re-packs and
 * re-copies the whole set.  A pz_state keeps one CrystallizedState's validators (SoA balance /
 * start / end) in HBM, owned by the library; the shim syncs it explicitly (upload after the
 * set changes, download when Go needs the balances) and the casper drop-ins run on it:
 * only the attestation bitfields cross PCIe per call.  NULL columns in upload / download are
 * skipped.  Same results and error codes as the host-pointer forms. */
typedef struct pz_state pz_state;
int  pz_state_new(uint64_t n, int device, pz_state** out);
int  pz_state_upload(pz_state* st, const uint64_t* balance, const uint64_t* start_dynasty,
                     const uint64_t* end_dynasty);
int  pz_state_download(pz_state* st, uint64_t* balance, uint64_t* start_dynasty, uint64_t* end_dynasty);
/* casper/validator.go:45-77 (pz_validator_indices on the mirror) */
int  pz_state_validator_indices(pz_state* st, uint64_t dynasty, int kind, uint32_t* out, uint64_t* count);
/* casper/incentives.go:14-32 (pz_calculate_rewards on the mirror's balances, in place) */
int  pz_state_calculate_rewards(pz_state* st, uint64_t dynasty, uint64_t total_deposit, const uint8_t* bits,
                                const uint64_t* boffs, uint64_t natt, int* applied);
/* blockchain/core.go:459-464: sum of the active validators' balances (TotalDeposits) */
int  pz_state_active_balance(pz_state* st, uint64_t dynasty, uint64_t* total);
void pz_state_free(pz_state* st);

/* ---- device-resident batched epoch transition (throughput mode, multi-GPU shards) -----
 * B independent instances of the data-parallel part of stateRecalc (blockchain/core.go:
 * 433-464): crosslink tallies + winners, attester popcount, CalculateRewards and the
 * next-cycle total balance.  All pointers are device pointers.  Validators are
 * instance-major [B][nval]; this rank holds global indices [val_offset, val_offset+nval)
 * of nval_global.  `scal` must be zero before pass 1 (allocate it zeroed, then ping-pong
 * with `scal_next`, which the finish pass zeroes); pass 1 initialises `winner` itself.
 * Single GPU: pz_dev_epoch_count -> pz_dev_epoch_finish.  Multi-GPU: count ->
 * all-reduce(sum) over the contiguous block {scal, vote, total} -> [when not every
 * validator is active: all-gather act_mask -> pz_dev_epoch_gather_compact] -> finish ->
 * all-reduce(sum) of scal[.][PZ_SCAL_NEXT_BAL].  After a multi-rank all-reduce,
 * PZ_SCAL_MAXIDX1 holds the sum of the per-rank values (single rank: the value). */
#define PZ_SCAL_POP       0  /* attester bit count (deposit = 32 * this)               */
#define PZ_SCAL_NACT      1  /* validators matching `kind` (written by the finish pass)  */
#define PZ_SCAL_ERR_XL    2  /* != 0: processCrosslinks would panic                     */
#define PZ_SCAL_ERR_RWD   3  /* != 0: CalculateRewards would panic (if threshold holds)  */
#define PZ_SCAL_APPLIED   4  /* 1: threshold held, balances updated                     */
#define PZ_SCAL_NEXT_BAL  5  /* sum of post-reward balances of active validators         */
#define PZ_SCAL_MAXIDX1   6  /* 1 + max matching global index (0: none)                 */
#define PZ_SCAL_NOMATCH   7  /* pass 1: validators in range NOT matching `kind` (all-reduced
                                with the rest); pass 2 sets PZ_SCAL_NACT = nval_global - this */
#define PZ_SCAL_COUNT     8
/* PZ_SCAL_ERR_XL is the sum, over every (attestation, rank) that found one, of the
 * PZ_XLERR_* values below: != 0 is the panic; the bits name the cause when one raiser did. */
#define PZ_XLERR_MEMBER   1ULL
#define PZ_XLERR_BITFIELD 2ULL
#define PZ_XLERR_SHARD    4ULL
#define PZ_XLERR_LAYOUT   8ULL  /* committee-order layout used with a non-matching validator */

typedef struct pz_epoch_batch {
  uint32_t ninst;                 /* B */
  uint64_t nval;                  /* validators per instance on this rank */
  uint64_t val_offset;            /* global index of local validator 0 */
  uint64_t nval_global;           /* validators per instance over all ranks */
  int kind;                       /* PZ_KIND_* (epoch transition: PZ_KIND_ACTIVE) */
  uint64_t* balance;              /* [B][nval] in/out */
  const uint64_t* start;          /* [B][nval] */
  const uint64_t* end;            /* [B][nval] */
  const uint64_t* dynasty;        /* [B] CurrentDynasty */
  const uint64_t* total_deposit;  /* [B] TotalDeposits */
  uint32_t natt;                  /* pending attestations per instance */
  const uint8_t* bits;            /* CSR bitfield bytes over B*natt attestations */
  const uint64_t* boffs;          /* [B*natt + 1] */
  uint64_t max_inst_bytes;        /* max bitfield bytes of one instance */
  uint32_t pop_rank, pop_world;   /* popcount chunks split over ranks (0, 1 single GPU) */
  const uint32_t* committee;      /* committee members (global validator indices) */
  const uint64_t* coffs;          /* [ncomm + 1] */
  const uint32_t* att_comm;       /* [B*natt] committee id of each attestation */
  const uint32_t* att_shard;      /* [B*natt] shard id of each attestation */
  uint32_t nrec;                  /* crosslink records per instance */
  const uint64_t* rec_dynasty;    /* [B][nrec] */
  uint32_t* winner;               /* [B][nrec] out */
  uint64_t* vote;                 /* [B*natt] out */
  uint64_t* total;                /* [B*natt] out */
  uint64_t* scal;                 /* [B][PZ_SCAL_COUNT] out */
  uint64_t* act_mask;             /* [B][ceil(nval/64)] scratch (general rank path) */
  uint32_t* blk_cnt;              /* [B][ceil(nval/2048)] scratch */
  uint32_t* act_list;             /* [B][nval_global] scratch (general rank path) */
  uint64_t* scal_next;            /* optional [B][PZ_SCAL_COUNT]: zeroed by the finish pass so
                                     the NEXT step can accumulate into it (ping-pong; saves a
                                     memset launch per step) */
  const uint32_t* cpos;           /* optional, multi-rank: `committee`/`coffs` list only this
                                     rank's members (global indices in [val_offset,
                                     val_offset + nval), plus, on rank 0, any member >=
                                     nval_global so that its panic is raised) and cpos[k] is
                                     member k's position in its full committee (the bitfield
                                     bit); NULL: full committees, position = index in the row */
  const uint32_t* co_index;       /* optional "committee order": the validator arrays of every
                                     instance are stored in committee order -- committee c
                                     occupies storage positions [coffs[c], coffs[c+1]) of
                                     [0, nval_global), which the committees partition -- and
                                     co_index[p - val_offset] is the validator index stored at
                                     position p.  The crosslink tallies then stream contiguous
                                     balances (no member gathers; `committee`/`cpos` unused) and
                                     CalculateRewards reads bit co_index[p] of the last bitfield.
                                     Requires every validator to match `kind` (else
                                     PZ_XLERR_LAYOUT in scal[PZ_SCAL_ERR_XL]). */
} pz_epoch_batch;

/* ---- T: block vote-cache tally (blockchain/core.go:300-345 calculateBlockVoteCache) ----
 * Each signed parent hash h has a dense slot id (host-assigned; the host keeps the 32-byte
 * hash -> slot map exactly like the Go map key).  A work item (attestation a, slot s) adds
 * every committee member of a whose bit is set and who is not yet in s's voter set:
 * totals[s] += balance[v].  Slots own an nval-bit dedup bitmap (words_per_slot u32 words).
 * Items of many blocks may share a launch as long as no balance changes between them
 * (balances change only in stateRecalc).  *err != 0 where Go would panic. */
typedef struct pz_vote_batch {
  const uint32_t* committee;   /* committee members (validator indices) */
  const uint64_t* coffs;       /* [ncomm + 1] */
  const uint32_t* att_comm;    /* [natt] committee id of each attestation */
  const uint8_t* bits;         /* CSR bitfields of the attestations */
  const uint64_t* boffs;       /* [natt + 1] */
  const uint32_t* item_att;    /* [nitems] */
  const uint32_t* item_slot;   /* [nitems] */
  uint64_t nitems;
  const uint64_t* balance;     /* [nval] */
  uint64_t nval;
  uint32_t* bitmaps;           /* [nslots][words_per_slot] in/out */
  uint64_t words_per_slot;     /* >= ceil(nval / 32) */
  uint64_t* totals;            /* [nslots] in/out (VoteTotalDeposit) */
  uint64_t* err;               /* [1] in/out */
  uint64_t val_offset;         /* validator-range shard: this rank holds
                                  validators [val_offset, val_offset + nval) of nval_global;
                                  balance and the bitmaps index v - val_offset and the members
                                  outside the range are skipped (another rank adds them) */
  uint64_t nval_global;        /* 0: no shard (nval_global = nval, val_offset = 0) */
} pz_vote_batch;

int pz_dev_vote_tally(const pz_vote_batch* b, void* stream);

/* Host-pointer form: same inputs; bitmaps/totals are read and written back in place. */
int pz_vote_tally(const uint32_t* committee, const uint64_t* coffs, uint64_t ncomm,
                  const uint32_t* att_comm, const uint8_t* bits, const uint64_t* boffs,
                  uint64_t natt, const uint32_t* item_att, const uint32_t* item_slot,
                  uint64_t nitems, const uint64_t* balance, uint64_t nval, uint32_t* bitmaps,
                  uint64_t nslots, uint64_t words_per_slot, uint64_t* totals);

typedef struct pz_comm pz_comm;  /* the ranks of a multi-GPU partition ("multi-GPU" below) */
/* The same tally sharded by validator range over the ranks of `comm`:
 * every local rank tallies the items' committee members in its 64-aligned validator range
 * [lo, hi) into its slice of the bitmaps (words [lo/32, hi/32) of every slot), and one RCCL
 * all-reduce (u64 sum) of the per-slot partial totals gives every rank the totals
 * (stateRecalc reads them, core.go:413-418).  Dedup stays exact: a voter's bit lives on the
 * one rank that owns it.  Host arrays as in pz_vote_tally; `totals` receives the global
 * totals; only the bitmap words of this process's local ranks are written back (one process
 * per GPU: each process holds its own slice). */
int pz_comm_vote_tally(const pz_comm* comm, const uint32_t* committee, const uint64_t* coffs, uint64_t ncomm,
                       const uint32_t* att_comm, const uint8_t* bits, const uint64_t* boffs, uint64_t natt,
                       const uint32_t* item_att, const uint32_t* item_slot, uint64_t nitems,
                       const uint64_t* balance, uint64_t nval, uint32_t* bitmaps, uint64_t nslots,
                       uint64_t words_per_slot, uint64_t* totals);

/* Pass 1 (pre-reward balances): classify/count, attester popcount, crosslink tallies. */
int pz_dev_epoch_count(const pz_epoch_batch* b, void* stream);
/* Pass 2 (after any cross-rank all-reduce): winners, active-list compaction when needed,
 * rewards in place and the post-reward total. */
int pz_dev_epoch_finish(const pz_epoch_batch* b, void* stream);

/* Multi-rank general rank path (not every validator active): between count and finish,
 * all-gather every rank's act_mask into gathered_mask[world][B][shard_words] (rank r owns the
 * global validators [r*64*shard_words, (r+1)*64*shard_words)), then call this to rebuild the
 * global compacted active list act_list[B][nval_global] on every rank; CalculateRewards
 * (casper/incentives.go:22-28) reads it by global rank position.  gblk is scratch
 * [B][ceil(nval_global/2048)] u32.  Instances with every validator active are skipped. */
int pz_dev_epoch_gather_compact(const pz_epoch_batch* b, const uint64_t* gathered_mask, uint32_t world,
                                uint64_t shard_words, uint32_t* gblk, void* stream);

/* ---- multi-GPU: communicators (RCCL over xGMI) ------------------------------------------
 * The reference is one Go process (ChainService.blockProcessing is one goroutine,
 * blockchain/service.go:229); nothing in it is distributed.  North_star shards the epoch by
 * validator range over the GPUs of one node and combines the participation and total-balance
 * sums with RCCL all-reduce.  A pz_comm names the ranks of that partition:
 *   pz_init_devices       one process drives ndev GPUs (ncclCommInitAll): the Go node's shape;
 *   pz_comm_init_rank     one process per GPU (ncclCommInitRank), the id from rank 0's
 *                         pz_comm_unique_id passed to every rank by the launcher;
 *   pz_comm_init_loopback `world` ranks in this process on ONE device, collectives by device
 *                         copies and a sum kernel (no RCCL): the sharded code path on a
 *                         one-GPU machine (tests);
 *   pz_comm_init_shm      one process per rank, ranks free to share a device: collectives
 *                         staged through host memory and a POSIX shared-memory group named
 *                         `name` (rank 0 creates it, O_EXCL; unlinked once every rank attached),
 *                         synchronous.  The one-process-per-GPU call sequence on a one-GPU
 *                         machine (tests, the bench's gloo rehearsal).  Every collective checks
 *                         that all ranks issued the same one (kind and sizes): a divergence fails
 *                         with PZ_EINVAL naming both calls, a rank missing for timeout_ms (0:
 *                         60 s) with PZ_EDEVICE -- where RCCL would hang.
 * librccl is resolved at run time (the copy already mapped into the process, else /opt/rocm's). */
#define PZ_COMM_ID_BYTES 128
typedef struct pz_comm pz_comm;
int  pz_comm_unique_id(uint8_t id[PZ_COMM_ID_BYTES]);
int  pz_comm_init_rank(const uint8_t id[PZ_COMM_ID_BYTES], int world, int rank, int device, pz_comm** out);
int  pz_init_devices(int ndev, const int* devices /* NULL: 0..ndev-1 */, pz_comm** out);
int  pz_comm_init_loopback(int world, int device, pz_comm** out);
int  pz_comm_init_shm(const char* name, int world, int rank, int device, uint32_t timeout_ms, pz_comm** out);
/* Collective timing: with timing on, every collective is bracketed by a HIP event pair on the
 * communicator's stream of each local rank (after its wait for the compute stream: the
 * collective's own time, exposed or overlapped).  pz_comm_collective_time returns the sum over
 * the collectives since the last call (the max over local ranks for each) and their count, and
 * restarts the sum; it waits for the pending collectives.  Each timed collective holds two
 * events per local rank until it is collected: a caller that leaves timing on collects
 * regularly (the bench collects once per timed run). */
int  pz_comm_set_timing(pz_comm* comm, int on);
int  pz_comm_collective_time(pz_comm* comm, double* ms, uint64_t* count);
/* world = ranks in the partition, nlocal = ranks this process drives (global ranks
 * first_rank .. first_rank+nlocal-1). */
int  pz_comm_size(const pz_comm* comm, int* world, int* nlocal, int* first_rank);
int  pz_comm_device(const pz_comm* comm, int local, int* device);
void pz_comm_free(pz_comm* comm);

/* H over the communicator: message batches shard with no collective.  Local rank i hashes
 * messages [n*r/world, n*(r+1)/world) of the batch (r = first_rank + i), on its own device,
 * all local ranks concurrently; out receives those digests (out_bytes each, at the message's
 * index).  A single-process communicator (pz_init_devices) covers the whole batch, which is
 * the multi-GPU form of pz_blake2b512_batch. */
int pz_comm_blake2b512_batch(const pz_comm* comm, const uint8_t* msgs, const uint64_t* offsets, uint64_t n,
                             uint8_t* out, uint32_t out_bytes);

/* ---- multi-GPU: the device-resident, validator-range-sharded epoch ----------------------
 * B independent epoch instances (the data-parallel part of stateRecalc, blockchain/core.go:
 * 433-464), described by host arrays over ALL validators; each local rank of `comm` uploads
 * its 64-aligned validator range [lo, hi) of every instance into its GPU's HBM (SoA,
 * instance-major) and the committee members inside it.  comm == NULL: one device, world 1.
 * When every validator is active and the committees partition the set, the validators are
 * stored in committee order (pz_epoch_batch.co_index): the crosslink tallies stream contiguous
 * balances and each rank holds a range of committee positions.  A step enqueues (no host sync):
 *   count -> RCCL all-reduce {scal, vote, total} -> [some validator inactive: all-gather of
 *   the active masks -> global compaction] -> finish -> all-reduce of the next-cycle totals,
 * the instances split in two parts so one part's collectives overlap the other's kernels.
 * In committee order, unless some attestation names a shard >= nrec (that panic depends on
 * the tallies), the step is one pass over the validators instead:
 *   bit count -> one stream (classify, crosslink tallies on the pre-reward balances, reward,
 *   next-cycle sum) -> winners -> one grouped RCCL collective (u64 sum of scal, u32 minimum
 *   of the winners)
 * (32 B per validator-epoch instead of 40).  Its ranks hold committee-aligned ranges, so the
 * vote/total of an attestation are complete on the rank holding its committee;
 * pz_epoch_state_tallies completes them everywhere.
 * Results are those of pz_dev_epoch_count/finish (bit-exact with the reference; panics
 * reported in scal[PZ_SCAL_ERR_*] with the balances untouched). */
typedef struct pz_epoch_host {
  uint32_t ninst;                  /* B */
  uint64_t nval;                   /* N validators per instance */
  const uint64_t* balance;         /* [B][N] */
  const uint64_t* start;           /* [B][N] */
  const uint64_t* end;             /* [B][N] */
  const uint64_t* dynasty;         /* [B] */
  const uint64_t* total_deposit;   /* [B] */
  uint32_t natt;                   /* pending attestations per instance */
  const uint8_t* bits;             /* CSR bitfields over B*natt attestations */
  const uint64_t* boffs;           /* [B*natt + 1], boffs[0] == 0 */
  const uint32_t* committee;       /* committee members (global validator indices) */
  const uint64_t* coffs;           /* [ncomm + 1], coffs[0] == 0 */
  uint64_t ncomm;
  const uint32_t* att_comm;        /* [B*natt] */
  const uint32_t* att_shard;       /* [B*natt] */
  uint32_t nrec;                   /* crosslink records per instance */
  const uint64_t* rec_dynasty;     /* [B][nrec].  dynasty, rec_dynasty, the committees and the
                                      attestations are copied by pz_epoch_state_new and fixed for
                                      the state's lifetime (no call updates them; the one-pass
                                      step's plan tables are built from them once).  A caller
                                      whose records or dynasty change makes a new state. */
  uint32_t layout;                 /* PZ_LAYOUT_AUTO: committee order when every validator is
                                      active and the committees partition the set, else index
                                      order; PZ_LAYOUT_INDEX: always index order;
                                      PZ_LAYOUT_TWOPASS: AUTO's layout, two-pass step */
} pz_epoch_host;
#define PZ_LAYOUT_AUTO    0
#define PZ_LAYOUT_INDEX   1
#define PZ_LAYOUT_TWOPASS 2  /* committee order as AUTO, but the two-pass step (A/B, tests) */
typedef struct pz_epoch_state pz_epoch_state;
int  pz_epoch_state_new(pz_comm* comm, int device, const pz_epoch_host* h, pz_epoch_state** out);
/* The state's options (no reference counterpart: placement and test controls of this library;
 * NULL or pz_epoch_state_new: every field 0).  There are no environment switches. */
typedef struct pz_epoch_options {
  uint64_t rebase_period;  /* u32-offset balances: steps between re-bases of the offsets (0: 2^29,
                              the product; larger values are clamped to it) */
  int window_only;         /* 1: one instance on one rank also takes the window pass (the
                              multi-instance one-pass kernel) instead of pz_epoch_one_kernel */
} pz_epoch_options;
int  pz_epoch_state_new_opts(pz_comm* comm, int device, const pz_epoch_host* h, const pz_epoch_options* opts,
                             pz_epoch_state** out);
int  pz_epoch_state_step(pz_epoch_state* st);
int  pz_epoch_state_sync(pz_epoch_state* st);
/* Local rank `local`'s validator range, device and compute stream (for event timing). */
int  pz_epoch_state_shard(const pz_epoch_state* st, int local, uint64_t* lo, uint64_t* hi, int* device,
                          void** stream);
/* From now on local rank `local` enqueues its steps on the caller's hipStream_t `stream` (of
 * that rank's device; NULL: back to the state's own stream).  Work already enqueued is waited
 * for first.  Several states bound to one stream step in issue order (e.g. a caller rotating
 * over state sets larger than the caches, or ordering the step after its own kernels). */
int  pz_epoch_state_bind_stream(pz_epoch_state* st, int local, void* stream);
/* After a step (synchronises): the balances of the hi-lo validators local rank `local` holds
 * ([B][hi-lo], in its storage order: pz_epoch_state_validators names them), and the reduced
 * scal [B][PZ_SCAL_COUNT], vote / total [B][natt] and winners [B][nrec] (any may be NULL). */
int  pz_epoch_state_results(pz_epoch_state* st, int local, uint64_t* balance, uint64_t* scal, uint64_t* vote,
                            uint64_t* total, uint32_t* winner);
/* The validator index held at each of local rank `local`'s hi-lo storage positions: lo.. in
 * index order; the members of the committees, in committee order, in the committee-order
 * layout (pz_epoch_batch.co_index), which *committee_order reports. */
int  pz_epoch_state_validators(const pz_epoch_state* st, int local, uint32_t* index);
/* The sharded one-pass step leaves each attestation's vote/total complete only on the rank
 * holding its committee (its winners are exact everywhere: proposed by that rank, combined by
 * a minimum all-reduce); this collective (every rank calls it) completes them on every rank
 * for pz_epoch_state_results.  A no-op for the other steps, and for a step whose tallies it
 * has already completed (calling it twice never sums complete tallies again). */
int  pz_epoch_state_tallies(pz_epoch_state* st);
/* *committee_order: 0 index order, 1 committee order (two-pass step), 2 committee order with
 * the one-pass step. */
int  pz_epoch_state_layout(const pz_epoch_state* st, int* committee_order);
/* The widths the one-pass stream reads per validator-epoch (the roofline's bytes; no reference
 * counterpart -- the Go state holds *pb.ValidatorRecord, types/state.go, messages.pb.go:803-809):
 * *balance_bytes 4 when the balances are held as u32 offsets from a per-instance u64 base
 * (every instance's balances within 2^30 of each other; results are the u64 values, exact mod
 * 2^64; the state re-bases the offsets every 2^29 steps), else 8; *dynasty_bytes 4, 8 or 16 for
 * the {start, end} column (16-, 32-bit saturated, or the u64 columns).  The widest part wins. */
int  pz_epoch_state_columns(const pz_epoch_state* st, uint32_t* balance_bytes, uint32_t* dynasty_bytes);
void pz_epoch_state_free(pz_epoch_state* st);
/* Host only (no device call): the layout a pz_epoch_state would choose for h (as
 * pz_epoch_state_layout) and global rank `rank`'s storage positions [lo, hi) in a world of
 * `world` ranks.  Lets a launcher size each rank's memory before any device is opened. */
int  pz_epoch_plan(const pz_epoch_host* h, int world, int rank, uint64_t* lo, uint64_t* hi, int* committee_order);

/* ---- block pipeline: sync replay of serialized blocks ---------------------------------
 * A chain object runs blocks through the reference's ChainService.blockProcessing
 * (blockchain/service.go:229-363) and updateHead (:170-227) over BeaconChain (core.go),
 * starting from the genesis states of `nval` validators (types/state.go:44-112).  Blocks are
 * canonical proto3 BeaconBlock encodings (messages.proto:37-46), CSR (offsets[n+1]), as they
 * arrive from the sync service (sync/service.go:147-164); a block that is not the canonical
 * encoding of its own decoding is PZ_EINVAL (the reference hashes proto.Marshal of the decoded
 * block).  Results per block and per attestation are what the reference stores or logs:
 * block digest (Block.Hash), attestation Key/Hash (saveAttestation, Attestation.Hash) and the
 * 64-byte processAttestation message digest (core.go:277-290).  Where the reference panics
 * the call returns PZ_EINDEX and the chain is unusable afterwards.  Thread-safe per chain. */
#define PZ_BLOCK_PROCESSED            0  /* became the candidate (and maybe a cycle transition) */
#define PZ_BLOCK_NO_PARENT            1  /* parent never saved, slot > 1 (service.go:261-269)   */
#define PZ_BLOCK_ATTS_REJECTED        2  /* last attestation failed / none (service.go:304-306)  */
#define PZ_BLOCK_SAVED_NOT_CANDIDATE  3  /* saved, a candidate was already chosen (:331-333)     */
#define PZ_ATT_PROCESSED              0
#define PZ_ATT_NOT_PROCESSED          1  /* its block was dropped before processAttestation       */
#define PZ_ATT_SLOT_HIGH              2  /* core.go:244-248 */
#define PZ_ATT_SLOT_LOW               3  /* core.go:249-253 */
#define PZ_ATT_JUSTIFIED              4  /* core.go:255-259 */
#define PZ_ATT_NO_COMMITTEE           5  /* core.go:373     */
#define PZ_ATT_BITFIELD_LEN           6  /* core.go:379-382 */
#define PZ_ATT_TRAILING_BITS          7  /* core.go:385-392 */

/* ---- §8f: processAttestation's checks for a batch, one GPU lane per attestation --------
 * blockchain/core.go:240-297 with getSignedParentHashes (:348-360), getAttesterIndices
 * (:363-374) and validateAttesterBitfields (:377-394), in Go's order.  Attestation i was
 * carried by a block of slot block_slot[i]; the chain state is the one processAttestation
 * reads (CrystallizedState.LastJustifiedSlot / LastStateRecalc / ShardAndCommitteesForSlots,
 * len(ActiveState.RecentBlockHashes)).  status[i] receives PZ_ATT_PROCESSED or the first
 * check that failed (PZ_ATT_*), or PZ_ERANGE / PZ_EINDEX where Go panics (the slice bounds
 * of :353, the committee index of :367).  committee[i] (optional) receives the committee id
 * (UINT32_MAX if not reached) and parents_start[i] (optional) the first RecentBlockHashes
 * index the signed parent hashes start at.
 * What tests/test_attcheck_dev_gpu.py pins, for both entry points and every kernel form:
 *  - a row that does not reach the committee walk (PZ_ATT_SLOT_HIGH, _SLOT_LOW, _JUSTIFIED,
 *    PZ_ERANGE, PZ_EINDEX) gets committee UINT32_MAX and parents_start 0; PZ_ATT_NO_COMMITTEE
 *    gets UINT32_MAX and block_slot - slot; every later status the committee id and
 *    block_slot - slot (the block gate completes these two columns in place);
 *  - last_byte, when given, is the only source of the trailing-bits byte: bits is not read;
 *  - nothing is written outside entries [0, natt) of the three outputs, and nothing at all
 *    when natt is 0 or the call returns PZ_EINVAL;
 *  - with narr == 0 the four table pointers may be NULL (every row that gets that far is
 *    PZ_EINDEX).
 * The slot window keeps Go's int: int(block_slot) - CycleLength wraps for block_slot in
 * [2^63, 2^63 + 63], where every slot not above block_slot is PZ_ATT_SLOT_LOW. */
typedef struct pz_att_check_batch {
  uint64_t natt;
  const uint64_t* slot;            /* AttestationRecord.Slot */
  const uint64_t* justified_slot;  /* .JustifiedSlot */
  const uint64_t* shard_id;        /* .ShardId */
  const uint64_t* n_oblique;       /* len(.ObliqueParentHashes) */
  const uint8_t*  bits;            /* .AttesterBitfield, CSR */
  const uint64_t* boffs;           /* natt+1 */
  const uint64_t* block_slot;      /* SlotNumber of the carrying block */
  uint64_t last_justified_slot, last_state_recalc, n_recent;
  uint64_t narr;                   /* len(ShardAndCommitteesForSlots) */
  const uint64_t* arr_offs;        /* narr+1: array a = entries arr_offs[a] .. arr_offs[a+1] */
  const uint64_t* arr_shard;       /* entry -> ShardId */
  const uint32_t* arr_comm;        /* entry -> committee id */
  const uint64_t* coffs;           /* committee c has coffs[c+1] - coffs[c] members */
  int32_t*  status;
  uint32_t* committee;
  uint64_t* parents_start;
  const uint8_t* last_byte;        /* optional (NULL: read from bits): natt bytes, the last byte of
                                      each bitfield (bits[boffs[i+1]-1]; any value when empty), a
                                      caller-side column so the trailing-bits check streams 1 B per
                                      attestation instead of touching every bitfield line */
} pz_att_check_batch;
int pz_check_attestations(const pz_att_check_batch* b);                  /* host pointers */
int pz_dev_check_attestations(const pz_att_check_batch* b, void* stream); /* device pointers */

/* ---- H: Attestation.Key and the processAttestation message digest from device columns ----
 * The two digests of blockProcessing whose messages are not a span of the received bytes;
 * neither message is materialised: one GPU lane per attestation assembles it block by block
 * from the columns pz_dev_unwire_attestations leaves on the device.  Memory contract: 4
 * readable bytes past the last byte of every bytes column (the CSR hash form's).
 *
 * pz_dev_attestation_keys replaces (*Attestation).Key, types/attestation.go:61-77 (the DB key
 * of saveAttestation): blake2b.Sum512 of
 *   key[0:10] (PutUvarint(Slot) at 0, then PutUvarint(ShardId) at 0 over it)
 *   | ShardBlockHash (its full length) | copy into [32]byte of each ObliqueParentHashes element
 * truncated to out_bytes (32: what Key returns; 64: the whole Sum512).  Of `a` it reads slot,
 * shard_id, shard_block_hash(+_offs) and the three oblique columns, with pz_attestation_cols'
 * NULL rules (a NULL scalar is 0 everywhere, NULL offsets are empty ranges).  A row with
 * d_rec_status[i] != PZ_OK (optional: pz_attestation_cols_out.status) gets a zero key.
 * PZ_EINVAL, before any launch: out_bytes other than 32 or 64; with n > 0 a NULL a or d_out,
 * offsets without their data column, d_out not 16-byte aligned.  n == 0 launches nothing. */
int pz_dev_attestation_keys(const pz_attestation_cols* a, uint64_t n, const int32_t* d_rec_status /* optional */,
                            uint8_t* d_out, uint32_t out_bytes /* 32 | 64 */, void* stream);
int pz_attestation_keys(const pz_attestation_cols* a, uint64_t n, uint8_t* out, uint32_t out_bytes);  /* host, sync */

/* pz_dev_attestation_messages replaces the message assembly and hash of processAttestation,
 * blockchain/core.go:277-290, with getSignedParentHashes' result (:348-360) taken as
 * parents_start: for every row whose status is PZ_ATT_PROCESSED, out[64 i ..] = blake2b.Sum512 of
 *   msg[0:10] (PutUvarint(Slot % 64) at 0, then PutUvarint(ShardId) at 0 over it)
 *   | for r < 64: parent_r | ' ' | ShardBlockHash
 * where parent_r = recent[parents_start[i] + r] for r < 64 - m and the record's m oblique
 * elements under common.BytesToHash after them; msg_len[i] = 2122 + len(ShardBlockHash).  A row
 * with any other status gets a zero digest and msg_len 0, and nothing is read through its
 * parents_start; so does a PROCESSED row whose m > 64 or whose parents would leave recent
 * (pz_dev_check_attestations never reports one).
 * PZ_EINVAL, before any launch: with natt > 0 a NULL status, parents_start or out, offsets
 * without their data column, n_recent < 64 (or a NULL recent) while a row is PROCESSED.  The
 * device form cannot see the statuses before it launches, so it applies that last rule to every
 * non-empty batch, and wants out 16-byte aligned.  natt == 0 launches nothing. */
typedef struct pz_att_msg_batch {   /* every member a pointer or a uint64_t */
  uint64_t natt;
  const uint64_t *slot, *shard_id;
  const uint8_t* shard_block_hash;      const uint64_t* shard_block_hash_offs;
  const uint8_t* oblique_parent_hashes; const uint64_t *oblique_offs, *oblique_first;
  const int32_t*  status;               /* pz_att_check_batch.status */
  const uint64_t* parents_start;        /* pz_att_check_batch.parents_start */
  const uint8_t*  recent; uint64_t n_recent;   /* RecentBlockHashes(), n_recent x 32 B, already BytesToHash-normalised */
  uint8_t* out;  /* natt x 64 */   uint32_t* msg_len;  /* optional */
} pz_att_msg_batch;
int pz_dev_attestation_messages(const pz_att_msg_batch* b, void* stream);
int pz_attestation_messages(const pz_att_msg_batch* b);   /* host pointers, sync */

/* ---- T: a device-resident block vote cache fed from decoded attestation columns -----------
 * calculateBlockVoteCache (blockchain/core.go:300-345; the loop of blockchain/service.go:313-318)
 * for a batch of attestations held as device columns: the handle owns the Go map
 * map[[32]byte]*VoteCache (types/state.go:27-31) -- the hash -> slot table, the 32-byte keys,
 * and per slot the voter bitmap and VoteTotalDeposit in pz_vote_batch's layout -- so the caller
 * builds no work list and keeps no hash map (pz_vote_tally needs both).
 *
 * For row i (carried by a block of slot bs), with m = its number of oblique elements, the 64
 * signed parents (getSignedParentHashes, core.go:348-360) are recent[parents_start[i] + r] for
 * r < 64 - m, then common.BytesToHash of each oblique element (the last 32 bytes of a longer
 * one, a shorter one right-aligned behind zeros).  A parent is skipped iff some RAW oblique
 * element of the row is exactly 32 bytes long and equals it (core.go:318-320).  Every parent
 * that is not skipped gets a map entry if it has none (core.go:322-326) and, for every committee
 * member v whose bit is set (MSB first) and who is not yet a voter of that hash, v joins the
 * voters and balance[v] is added to the total, mod 2^64 (core.go:328-341).
 *
 * Scope: the rows tallied are those with status[i] == PZ_ATT_PROCESSED and, when take is given,
 * take[i] != 0.  The reference also tallies the FAILED attestations of a block whose last
 * attestation passed (service.go:304-318 looks only at the last error), re-deriving their parents
 * and committee.  That decision is the block gate's (pz_dev_block_gate below): its vote_status
 * column reads PZ_ATT_PROCESSED on exactly the rows the reference tallies, with committee and
 * parents_start completed for the re-derived ones, and is passed here as `status`; a caller that
 * passes the checks' status instead tallies the passed rows only
 * (prysm_amd.blockchain.tally_serialized_blocks, tally_mixed).  A row also
 * contributes nothing, and nothing is read through its offsets, when m > 64, when
 * parents_start[i] + 64 - m > n_recent (the checks never report either as PROCESSED), when the
 * n_oblique column disagrees with oblique_first, or when committee[i] >= ncomm, which sets the
 * panic error besides.
 *
 * The table: open addressing over u32 cells, cells = the smallest power of two >= 2 * slot_cap
 * (at least 2); the home cell of a hash is le32(hash[0..4]) & (cells - 1); linear probing with
 * wraparound.  A cell is 0xFFFFFFFF (empty), a slot id, or, inside a call, 0x80000000 | the
 * smallest source index of a new hash (source s < n_recent is recent[s], source n_recent + e is
 * oblique element e).  New slots are numbered in ascending order of that index: slot ids are
 * deterministic.  A call that needs more slots than remain (or finds no cell) changes nothing
 * and sets the sticky capacity error: it lands whole or not at all.
 *
 * One tally is a memset and four dependent launches on the caller's stream (mark, intern,
 * commit, tally: DESIGN.md §3); no workgroup waits for another.  Balances must not change
 * between the calls of one cache (they change only in stateRecalc).
 * PZ_EINVAL, before any launch: with natt > 0 a NULL bits, boffs, status, committee,
 * parents_start, members, coffs or balance; oblique offsets without oblique_parent_hashes,
 * oblique_first without oblique_offs; n_oblique_total > 0 without the three oblique columns
 * (with n_oblique_total == 0 they may be NULL); n_recent > 0 with a NULL recent;
 * n_recent + n_oblique_total >= 2^31; natt >= 2^27; d_scratch NULL or not 16-byte aligned.
 * natt == 0 launches nothing.  n_oblique and take are optional.  Thread-safe per handle. */
typedef struct pz_vote_cache pz_vote_cache;
int      pz_vote_cache_new(uint64_t nval, uint32_t slot_cap, int device, pz_vote_cache** out);
void     pz_vote_cache_free(pz_vote_cache* cache);
uint64_t pz_vote_cache_scratch_bytes(uint64_t natt, uint64_t n_recent, uint64_t n_oblique_total);
typedef struct pz_vote_cols_batch {   /* every member a pointer or a uint64_t */
  uint64_t natt;
  const uint64_t* n_oblique;            /* optional: pz_att_check_batch.n_oblique */
  const uint8_t* oblique_parent_hashes; const uint64_t *oblique_offs, *oblique_first; uint64_t n_oblique_total;
  const uint8_t* bits; const uint64_t* boffs;   /* attester_bitfield, attester_bitfield_offs */
  const int32_t* status; const uint32_t* committee; const uint64_t* parents_start;  /* pz_att_check_batch outputs */
  const uint8_t* take;                  /* optional, natt: 0 leaves the row out */
  const uint8_t* recent; uint64_t n_recent;     /* RecentBlockHashes(), already BytesToHash-normalised, as pz_att_msg_batch */
  const uint32_t* members; const uint64_t* coffs; uint64_t ncomm;   /* the committees, CSR (pz_vote_batch.committee / coffs) */
  const uint64_t* balance;              /* nval */
} pz_vote_cols_batch;
/* Device pointers, caller's stream, asynchronous; d_scratch holds pz_vote_cache_scratch_bytes(...). */
int pz_dev_vote_cache_tally(pz_vote_cache* cache, const pz_vote_cols_batch* b, void* d_scratch, void* stream);
/* Host pointers (ranges start at 0), synchronous; waits for the stream of the cache's last call
 * first.  Only the elements the rows name are staged: n_oblique_total is a bound here.  Errors the
 * kernels find are sticky and reported by the two calls below, not here. */
int pz_vote_cache_tally(pz_vote_cache* cache, const pz_vote_cols_batch* b);
/* The map's entries in slot order (the deterministic order above): *count of them; hashes[32 i]
 * and totals[i] (VoteTotalDeposit) are filled when cap >= *count.  Waits for the stream of the
 * last tally.  The sticky error comes first: PZ_EINDEX where Go panics (core.go:328-329, :367),
 * else PZ_ERANGE when a call was dropped for capacity; the outputs are filled all the same (they
 * hold every call that landed).  After a pz_[dev_]vote_cache_retain the entries are the kept ones
 * only, in their new slot order. */
int pz_vote_cache_read(pz_vote_cache* cache, uint8_t* hashes, uint64_t* totals, uint64_t cap, uint64_t* count);
/* VoterIndices of one hash as a bitmap (ceil(nval / 32) u32 words, bit v & 31 of word v >> 5;
 * zeros when absent) and *present = the map has the entry.  Same waiting and errors as read.  After
 * a pz_[dev_]vote_cache_retain it speaks of the kept entries only: a dropped hash is absent. */
int pz_vote_cache_voters(pz_vote_cache* cache, const uint8_t hash[32], uint32_t* words, int* present);
/* `if _, ok := blockVoteCache[blockHash]` and .VoteTotalDeposit, core.go:414-418, for n hashes
 * (BytesToHash-normalised, n x 32 bytes) on the device: d_totals[q] is the entry's VoteTotalDeposit,
 * 0 when the map has none; d_slots[q] (optional) its slot id, 0xFFFFFFFF when absent.  One launch
 * on the caller's stream, a lane per query walking the table above with plain loads: the caller
 * orders it after the cache's earlier calls (one stream, or its own events) and no call of the
 * cache may run beside it.  Reports no sticky error (read and voters do).  n == 0 launches nothing.
 * PZ_EINVAL, before any launch: a NULL cache; with n > 0 a NULL d_hashes or d_totals, or a
 * d_hashes that is not 16-byte aligned. */
int pz_dev_vote_cache_lookup(pz_vote_cache* cache, const uint8_t* d_hashes, uint64_t n, uint64_t* d_totals,
                             uint32_t* d_slots /* optional */, void* stream);
/* The same lookup (core.go:414-418) over host pointers (any alignment), synchronous; waits for the
 * stream of the cache's last call first. */
int pz_vote_cache_lookup(pz_vote_cache* cache, const uint8_t* hashes, uint64_t n, uint64_t* totals,
                         uint32_t* slots /* optional */);
/* Growth and retirement, for a chain of any length.  The reference's map (types/state.go:27-31)
 * only grows: every candidate block's hash and every oblique parent hash becomes an entry
 * (core.go:300-345).  A cache is created with slot_cap slots; a tally that needs more lands
 * nothing and sets the sticky PZ_ERANGE.  Both calls below move the entries into the cache's second
 * buffer set (allocated at the first of them, not at creation) on the device and then swap the
 * sets; both carry the sticky error word over unchanged, are ordered on their stream like every
 * other call on the handle, and leave lookup, read, voters, tally and pz_dev_state_recalc working
 * on the new set.  Slots at or past the count read zero voters and a zero total, as after
 * pz_vote_cache_new.  (votecache_dev.h holds the rules and the argument)
 *
 * The slots the cache holds now (no reference counterpart: a Go map has no capacity).  Host only,
 * no device call. */
int pz_vote_cache_capacity(pz_vote_cache* cache, uint32_t* slot_cap);
/* Room for min_slots entries: the Go map's own growth (runtime map growth; types/state.go:27-31 has
 * no bound).  With min_slots <= the capacity nothing happens and nothing is launched.  Otherwise
 * the cache gets exactly min_slots slots and the cells of a cache created with as many; every entry
 * keeps its slot id, key, total and voters.  A memset and two launches (move, rehash) on the
 * caller's stream.  The host decides from the capacity it keeps: nothing is read back.  PZ_EINVAL,
 * before any launch: a NULL cache, min_slots above 2^30.  An allocation failure returns PZ_EDEVICE
 * and leaves the cache as it was. */
int pz_dev_vote_cache_reserve(pz_vote_cache* cache, uint32_t min_slots, void* stream);
/* The same reserve (the map's own growth, types/state.go:27-31), synchronous; waits for the stream
 * of the cache's last call first. */
int pz_vote_cache_reserve(pz_vote_cache* cache, uint32_t min_slots);
/* Retirement (no reference counterpart: the Go map never deletes).  The cache keeps exactly the
 * entries whose key is among the n hashes (n x 32 bytes, BytesToHash-normalised; a hash given twice
 * or one the map lacks is harmless) and drops the others; a kept entry's new slot id is its rank
 * among the kept ones in ascending old id, so ids stay deterministic; key, total and voters go
 * with it.  n == 0 empties the cache.  The capacity stays.  What may be dropped is the caller's
 * judgement: stateRecalc's justification loop (core.go:411-431) reads the map only at
 * RecentBlockHashes()[0..63] of the ActiveState being promoted, and a hash that has left the ring
 * never enters it again (service.go:320-333), so the ring's entries and the candidates of the run
 * in hand cover every later read -- except the votes an oblique parent hash collected before the
 * block it names became a candidate (votecache_dev.h).
 * Two memsets and four launches (keep, renumber, move, rehash) on the caller's stream; d_scratch
 * holds pz_vote_cache_retain_scratch_bytes(the cache's capacity, n).  PZ_EINVAL, before any launch:
 * a NULL cache; n > 0 with a NULL d_hashes or one that is not 16-byte aligned; n >= 2^31; a NULL or
 * misaligned d_scratch.  An allocation failure as for reserve. */
uint64_t pz_vote_cache_retain_scratch_bytes(uint32_t slot_cap, uint64_t n);
int pz_dev_vote_cache_retain(pz_vote_cache* cache, const uint8_t* d_hashes, uint64_t n, void* d_scratch, void* stream);
/* The same retain (no reference counterpart) over host pointers (any alignment), synchronous;
 * waits for the stream of the cache's last call first. */
int pz_vote_cache_retain(pz_vote_cache* cache, const uint8_t* hashes, uint64_t n);

/* ---- T/R: the block gate: which blocks go on, which rows reach the cache and the pool -----------
 * blockProcessing looks only at the LAST attestation's error (blockchain/service.go:281-306), then
 * runs calculateBlockVoteCache over EVERY attestation of the block (service.go:313-318, core.go:
 * 300-345), the ones processAttestation refused included, and appends the ones that passed to
 * processedAttestations (service.go:299).  For a batch of decoded blocks (block b's rows are
 * att_first[b] .. att_first[b+1] of the attestation columns, n_rows of them):
 *
 * block b is ACCEPTED iff block_status[b] == PZ_OK and rec_status (when given) is PZ_OK on every
 * one of its rows; it is OPEN iff it is accepted, n_rows > 0 and its last row's check status is
 * PZ_ATT_PROCESSED.  report[b] = 0 not open, 1 open with every row PROCESSED, 2 open with some row
 * not PROCESSED.  A block whose att_first pair is inverted or runs past chk.natt is rejected, and
 * nothing is read or written through it.
 *
 * vote_status[i] is PZ_ATT_PROCESSED exactly where the reference tallies row i.  In an open block,
 * by the row's check status:
 *   PROCESSED, BITFIELD_LEN, TRAILING_BITS  tallied with the checks' committee / parents_start
 *                   (CheckBit ignores the bits past the committee and panics past the bitfield,
 *                   core.go:328-331: the tally raises that panic when a parent is not skipped);
 *   NO_COMMITTEE    getAttesterIndices returns an error (core.go:373): keeps its status;
 *   SLOT_HIGH, SLOT_LOW, JUSTIFIED  re-derived, in u64 arithmetic that wraps: start = bs - slot,
 *                   end = start - m + 64; start > end or end > n_recent: Go panics (core.go:353);
 *                   idx = slot - last_state_recalc >= narr: Go panics (core.go:367); else array
 *                   idx is walked for the shard: found, committee[i] and parents_start[i] = start
 *                   are written over the checks' and the row is tallied; not found, it keeps its
 *                   status (core.go:373);
 *   PZ_ERANGE, PZ_EINDEX  processAttestation itself panicked: the panic bit, in any accepted block,
 *                   open or not.
 * In a block that is not open nothing is tallied: a PROCESSED row reads PZ_ATT_NOT_PROCESSED,
 * every other row keeps its check status.  pend_take[i] = 1 iff row i is PROCESSED, its block is
 * open and candidate[b] != 0 (when given: the walk's decision that block b reaches
 * computeNewActiveState, service.go:261-269, :331-333).  flags: one word the caller zeroes, ORed:
 * bit 0 = the reference panics on some row (the other outputs are filled all the same).
 *
 * One launch, one wave per block; no scratch.  Of chk it reads natt, status, slot,
 * block_slot, n_oblique, shard_id, last_state_recalc, n_recent and the table (narr, arr_offs,
 * arr_shard, arr_comm), and writes committee and parents_start.
 * PZ_EINVAL, before any launch: a NULL batch; nblocks >= 2^31; with nblocks > 0 a NULL att_first,
 * block_status, report, vote_status, flags, chk.committee or chk.parents_start, with chk.natt > 0
 * a NULL column of those read, with chk.narr > 0 a NULL table.  nblocks == 0 launches nothing. */
typedef struct pz_block_gate_batch {   /* every member a pointer, a uint64_t or the embedded batch */
  uint64_t nblocks;
  const uint64_t* att_first;     /* nblocks + 1 (pz_unwire_blocks) */
  const int32_t*  block_status;  /* nblocks: the decoder's top-level status */
  const int32_t*  rec_status;    /* optional, chk.natt: pz_attestation_cols_out.status */
  const uint8_t*  candidate;     /* optional, nblocks */
  pz_att_check_batch chk;        /* the columns and state the checks read, and their three outputs,
                                    already filled by pz_[dev_]check_attestations; committee and
                                    parents_start are completed in place for re-derived rows */
  uint8_t*  report;              /* nblocks: 0 / 1 / 2 */
  int32_t*  vote_status;         /* chk.natt: feed it to pz_vote_cols_batch.status */
  uint8_t*  pend_take;           /* optional, chk.natt: feed it to pz_dev_att_pool_append */
  uint32_t* flags;               /* one word, ORed: bit 0 = the reference panics */
} pz_block_gate_batch;
/* service.go:281-318 over device pointers, on the caller's stream, asynchronous. */
int pz_dev_block_gate(const pz_block_gate_batch* b, void* stream);
/* service.go:281-318 over host pointers, synchronous; returns PZ_EINDEX when bit 0 of *flags is
 * set, the outputs filled all the same.  A row no block names comes back as it was. */
int pz_block_gate(const pz_block_gate_batch* b);

/* ---- R: ActiveState.RecentBlockHashes resident on the device --------------------------------------
 * The ring of the last 128 block hashes (types/state.go:45-49, 189-195) that computeNewActiveState
 * rolls by one for every candidate block (blockchain/core.go:223-237), in place on the object
 * c.chain.ActiveState() returns (service.go:346).  The handle owns 129 entries of 32 bytes
 * (common.BytesToHash-normalised) with a stored length each (u8; a genesis entry has length 0: what
 * pz_dev_active_state_bytes' d_recent_len wants): entry 0 is one hash of history, entries 1..128 are
 * the window.  The history entry is there because the block after a transition block is still
 * checked and tallied against the ring as it was before the transition block's hash went in
 * (updateHead, service.go:320-321, runs after :281-318).  Two buffer sets ping-pong, as the pool's
 * do: every append and every walk writes the other set and swaps.  Calls on one ring are ordered by
 * the caller (one stream, or its own events).  Thread-safe per handle.
 *
 * pz_recent_hashes_new: types.NewGenesisStates' ring (types/state.go:45-49) or a later one, n == 128
 * hashes with their stored lengths (lens NULL: all 32; a length above 32 counts as 32); the history
 * entry starts as zeros.  A chain from genesis always holds 128 (core.go:230-232): any other n is
 * PZ_EINVAL, and a shorter ring stays with the one-state functions. */
typedef struct pz_recent_hashes pz_recent_hashes;
int  pz_recent_hashes_new(const uint8_t* hashes, const uint8_t* lens, uint64_t n, int device, pz_recent_hashes** out);
void pz_recent_hashes_free(pz_recent_hashes* ring);
/* RecentBlockHashes() (types/state.go:189-195) as device pointers to the live set's window (128 x 32
 * bytes, 16-byte aligned) and its 128 lengths, valid until the ring's next append or walk: pass them
 * as they are to pz_dev_state_recalc (recent), pz_dev_active_state_bytes (d_recent, d_recent_len),
 * pz_vote_cols_batch.recent and pz_att_msg_batch.recent.  Either output may be NULL.  No device call. */
int  pz_recent_hashes_view(pz_recent_hashes* ring, const uint8_t** d_hashes, const uint8_t** d_lens);
/* Host download of all 129 entries (RecentBlockHashes(), types/state.go:189-195, behind the history
 * entry) and their lengths; either may be NULL.  Waits for the stream of the ring's last call. */
int  pz_recent_hashes_read(pz_recent_hashes* ring, uint8_t* hashes /* 129 x 32 */, uint8_t* lens /* 129 */);
/* computeNewActiveState's append (core.go:230-237) for a caller that decides for itself (the
 * transition block's path, one-block callers): of n hashes (n x 32 bytes, 16-byte aligned), those
 * with d_take[j] != 0 (NULL: all) are appended in order, and the last 129 entries are kept.  When
 * any hash is taken EVERY entry's stored length becomes 32: the reference appends to
 * RecentBlockHashes(), the [32]byte form of every entry (types/state.go:189-195), and stores that
 * list back whole (core.go:230-236); only a ring nothing was appended to keeps its lengths.  One launch of one workgroup on the caller's stream, no scratch.  PZ_EINVAL, before any
 * launch: a NULL ring; with n > 0 a NULL or misaligned d_hashes; n >= 2^31.  n == 0 launches nothing. */
int  pz_dev_recent_hashes_append(pz_recent_hashes* ring, const uint8_t* d_hashes, const uint8_t* d_take /* optional */,
                                 uint64_t n, void* stream);
/* The same append (core.go:230-237) over host pointers (any alignment), synchronous. */
int  pz_recent_hashes_append(pz_recent_hashes* ring, const uint8_t* hashes, const uint8_t* take /* optional */, uint64_t n);

/* ---- T/R: the block walk: a run of blocks, each against its own RecentBlockHashes -----------------
 * The sequential decisions blockProcessing takes over the blocks that go on -- updateHead and the
 * candidate rule (blockchain/service.go:320-333), IsCycleTransition (core.go:181-183) -- as scans
 * over a run of nblocks received blocks, and the window of RecentBlockHashes each of them reads
 * (getSignedParentHashes, core.go:348-360): the reference appends each candidate's hash in place
 * (core.go:223-237 on the pointer of service.go:346), so block j reads a window shifted by the
 * number of candidates before it.
 *
 * go_j = report[j] != 0 (the block gate's report).  Eligibility stays the caller's: the parent is
 * saved (service.go:261-269) and CanProcessBlock holds (:272, :308); the caller applies it by handing
 * the gate a block_status other than PZ_OK for an ineligible block.  In block order, "pending" being
 * has_candidate or an earlier block of the run that went on:
 *   cand_j = go_j and (not pending, or slot_j > 1 and slot_j > the largest slot of the carried
 *            candidate and of the earlier candidates of the run)                  (service.go:320-333)
 *   stop   = the smallest of: the index of the first candidate with slot >= last_state_recalc + 64
 *            (core.go:181-183; that block excluded), with lag > 0 one past the first candidate (from
 *            the next block on the CrystallizedState differs too), and nblocks.
 *   walk[j] = 0 not going on, 1 saved but not the candidate (:331-333), 2 candidate, 3 deferred
 *            (j >= stop: no tally, no pool row, no hash; the caller submits it again).
 *   base[j] = 1 - lag + (the candidates before j), 0 for a deferred block.
 * The log is the ring's 129 entries followed by the run's candidate hashes in order, the rest of
 * its 129 + nblocks entries zeroed; block j's window is log[base[j], base[j] + 128).  Per row i of
 * block b = att_block[i]: parents_start[i] += base[b]; pend_take[i] &= (walk[b] == 2); where b is
 * deferred a PZ_ATT_PROCESSED vote_status[i] becomes PZ_ATT_NOT_PROCESSED.  With the checks run at
 * n_recent = 128 no row names a log position at or past 129 + the candidates before its block
 * (blockwalk_dev.h has the proof), so `log` with n_recent = 129 + nblocks goes to
 * pz_dev_vote_cache_tally and pz_dev_attestation_messages as `recent`.  Last the ring becomes the
 * last 129 entries of the log's used part (core.go:230-232), every stored length 32 when the run
 * had a candidate (as pz_dev_recent_hashes_append) -- unless
 * flags is given and its bit 0 is set (the reference panics somewhere in the batch, and the caller
 * will land none of it): then the ring's content stays as it was.
 * result[4]: stop, the number of candidates before stop, and has_candidate / candidate_slot as
 * they are after block stop - 1 (to carry into the next call).
 *
 * Three dependent launches on the caller's stream (scan, rows, roll: DESIGN.md §3); no workgroup
 * waits for another, the host reads nothing.  PZ_EINVAL, before any launch: a NULL ring or batch;
 * nblocks >= 2^31; lag > 1; with nblocks > 0 a NULL slot_number, report, block_hash, walk, base,
 * result or (device form) log, a block_hash or log that is not 16-byte aligned; with natt > 0 a
 * NULL att_block, vote_status or parents_start.  nblocks == 0 launches nothing and leaves the ring
 * as it is.  pend_take is optional. */
typedef struct pz_block_walk_batch {   /* every member a pointer or a uint64_t */
  uint64_t nblocks;
  const uint64_t* slot_number;   /* nblocks: pz_block_cols_out.slot_number */
  const uint8_t*  report;        /* nblocks: pz_block_gate_batch.report */
  const uint8_t*  block_hash;    /* nblocks x 32: Block.Hash(), pz_dev_blake2b512_spans over the blocks */
  uint64_t has_candidate, candidate_slot;   /* carried in: candidateBlock != nilBlock, its SlotNumber */
  uint64_t last_state_recalc;    /* CrystallizedState.LastStateRecalc as IsCycleTransition reads it, after
                                    updateHead (service.go:320-321, :345): with lag, the new state's */
  uint64_t lag;                  /* 1: the run starts right after a transition block (see the ring) */
  uint64_t natt;
  const uint32_t* att_block;     /* natt: pz_block_cols_out.att_block */
  int32_t*  vote_status;         /* natt: pz_block_gate_batch.vote_status, narrowed in place */
  uint8_t*  pend_take;           /* optional, natt: pz_block_gate_batch.pend_take, narrowed in place */
  uint64_t* parents_start;       /* natt: pz_att_check_batch.parents_start, made absolute in place */
  uint8_t*  walk;                /* nblocks */
  uint64_t* base;                /* nblocks */
  uint64_t* result;              /* 4 */
  uint8_t*  log;                 /* pz_block_walk_scratch_bytes(nblocks, natt) bytes: (129 + nblocks) x 32 */
  const uint32_t* flags;         /* optional: pz_block_gate_batch.flags; with bit 0 set the ring stays as it is */
} pz_block_walk_batch;
/* The bytes of `log` (no reference counterpart). */
uint64_t pz_block_walk_scratch_bytes(uint64_t nblocks, uint64_t natt);
/* service.go:320-333 over a run, device pointers, on the caller's stream, asynchronous. */
int pz_dev_block_walk(pz_recent_hashes* ring, const pz_block_walk_batch* b, void* stream);
/* service.go:320-333 over a run, host pointers (any alignment), synchronous; waits for the stream
 * of the ring's last call first.  log is optional here. */
int pz_block_walk(pz_recent_hashes* ring, const pz_block_walk_batch* b);

/* ---- T/R: a run of blocks through a cycle transition ----------------------------------------------
 * pz_block_walk for a run that holds the transition block itself: the candidate rule and updateHead
 * (blockchain/service.go:320-333) unchanged, and IsCycleTransition (core.go:181-183) deciding where
 * stateRecalc (core.go:398-497, from service.go:345-353) stands in the run, not where the run ends.
 * stateRecalc builds the CANDIDATE's states; the chain keeps its own until the next block with a
 * larger slot promotes them (updateHead, service.go:170-227), and every block is checked and tallied
 * against the chain's (service.go:281-318 run before :320).  CalculateRewards writes the balances in
 * place (casper/incentives.go:22-28) on the slice stateRecalc hands on (core.go:468) and the vote
 * cache is one shared map (core.go:494-496), so the two pairs of states differ in two host scalars,
 * the ring's history entry, and the side of stateRecalc a tally or a pool append falls on.
 *
 * go, pending, cand_j, rank_j (the candidates before j) and the log as pz_block_walk_batch defines
 * them; last_state_recalc is the value IsCycleTransition reads for the first candidate, as there.
 *   T = with lag == 0 the first candidate with slot >= last_state_recalc + 64; it is INCLUDED.
 *   L = with lag == 0 the first candidate after T, tested against last_state_recalc + 128 (the sums
 *       wrap as Go's uint64); with lag == 1 the first candidate, tested against last_state_recalc.
 *   lag == 0: L no transition: stop = L + 1, lag_out = 0; L a transition (a slot jump of a cycle or
 *       more): stop = L (deferred: one stateRecalc a call), lag_out = 1; the run ends before an L:
 *       stop = nblocks, lag_out = 1; no T: stop = nblocks, lag_out = 0.
 *   lag == 1: L no transition: stop = L + 1, lag_out = 0; L a transition: it is taken as T, stop =
 *       L + 1, lag_out = 1; no L: stop = nblocks, lag_out = 1.
 *   walk[j] as pz_block_walk_batch.walk (the same four codes: pz_dev_block_set_insert_walked takes
 *       them unchanged); base[j] = 1 - lagged_j + rank_j with lagged_j = lag or j > T, 0 for a
 *       deferred block: a lagged block reads the ring as it was before T's hash went in.
 * Per row i of block b = att_block[i]: parents_start[i] += base[b];
 *   vote0[i] = vote_status[i] where b <= T (no T: every b) and b < stop -- the rows calculateBlockVoteCache
 *              tallies BEFORE stateRecalc, T's own included (service.go:313-318 precede :345);
 *   vote1[i] = vote_status[i] where T < b < stop -- the rows tallied after it, against the balances
 *              CalculateRewards left; elsewhere a PZ_ATT_PROCESSED becomes PZ_ATT_NOT_PROCESSED;
 *   take0[i] = pend_take[i] (NULL: 1) and walk[b] == 2 and b < T (no T: every b): what the chain's
 *              PendingAttestations holds when stateRecalc reads and prunes it;
 *   take1[i] = pend_take[i] and walk[b] == 2 and b >= T: what computeNewActiveState appends to the
 *              new ActiveState (core.go:223-237), T's own rows first.
 * No row names a log position at or past 129 + rank_b (blockcycle_dev.h has the proof), so `log`
 * with n_recent = 129 + nblocks is `recent` for both tallies and the message digests.  The promoted
 * ActiveState's RecentBlockHashes -- stateRecalc's `recent` (core.go:413), 128 entries -- starts at log
 * entry 1 + t_rank.  The ring rolls as in pz_block_walk (flags likewise).
 * result[8]: stop, the candidates before stop (T and L included), has_candidate / candidate_slot
 * after block stop - 1, t_index (all ones: no T), t_rank, t_slot (0 without a T), lag_out.
 *
 * Three dependent launches on the caller's stream (scan, rows, and the walk's roll: DESIGN.md §3); no
 * workgroup waits for another, the host reads nothing.  PZ_EINVAL, before any launch: a NULL ring or
 * batch; nblocks >= 2^31; lag > 1; with nblocks > 0 a NULL slot_number, report, block_hash, walk,
 * base, result or (device form) log, a block_hash or log that is not 16-byte aligned; with natt > 0
 * a NULL att_block, vote_status, parents_start, vote0, vote1, take0 or take1.  nblocks == 0 launches
 * nothing and leaves the ring as it is. */
typedef struct pz_block_cycle_batch {   /* every member a pointer or a uint64_t */
  uint64_t nblocks;
  const uint64_t* slot_number;   /* nblocks: pz_block_cols_out.slot_number */
  const uint8_t*  report;        /* nblocks: pz_block_gate_batch.report */
  const uint8_t*  block_hash;    /* nblocks x 32: Block.Hash(), pz_dev_blake2b512_spans over the blocks */
  uint64_t has_candidate, candidate_slot;   /* carried in: candidateBlock != nilBlock, its SlotNumber */
  uint64_t last_state_recalc;    /* as pz_block_walk_batch.last_state_recalc: with lag, the new state's */
  uint64_t lag;                  /* 1: the last call's lag_out: a transition block's states are not promoted yet */
  uint64_t natt;
  const uint32_t* att_block;     /* natt: pz_block_cols_out.att_block */
  const int32_t*  vote_status;   /* natt: pz_block_gate_batch.vote_status */
  const uint8_t*  pend_take;     /* optional, natt: pz_block_gate_batch.pend_take */
  uint64_t* parents_start;       /* natt: pz_att_check_batch.parents_start, made absolute in place */
  int32_t*  vote0;               /* natt: the tally's status before stateRecalc */
  int32_t*  vote1;               /* natt: the tally's status after it */
  uint8_t*  take0;               /* natt: the pool's take before stateRecalc */
  uint8_t*  take1;               /* natt: the pool's take after it */
  uint8_t*  walk;                /* nblocks */
  uint64_t* base;                /* nblocks */
  uint64_t* result;              /* 8 */
  uint8_t*  log;                 /* pz_block_cycle_scratch_bytes(nblocks, natt) bytes: (129 + nblocks) x 32 */
  const uint32_t* flags;         /* optional: pz_block_gate_batch.flags; with bit 0 set the ring stays as it is */
} pz_block_cycle_batch;
/* The bytes of `log` (no reference counterpart). */
uint64_t pz_block_cycle_scratch_bytes(uint64_t nblocks, uint64_t natt);
/* service.go:320-361 over a run with its transition block, device pointers, on the caller's stream,
 * asynchronous. */
int pz_dev_block_cycle(pz_recent_hashes* ring, const pz_block_cycle_batch* b, void* stream);
/* service.go:320-361 over a run with its transition block, host pointers (any alignment),
 * synchronous; waits for the stream of the ring's last call first.  log is optional here. */
int pz_block_cycle(pz_recent_hashes* ring, const pz_block_cycle_batch* b);

/* ---- R: the saved-block set resident on the device, and the parent check over a run ---------------
 * hasBlock (blockchain/core.go:560-562) answers blockProcessing's first question about a received
 * block, `hasBlock(block.ParentHash())` (service.go:261-269), from the blocks saveBlock stored
 * (service.go:324, core.go:565-577).  The handle owns that set of 32-byte block hashes on one device:
 * an open-addressing table with a power-of-two number of cells (at least 8), linear probing from the
 * cell the hash's first little-endian word names, a state word per cell beside its 32 key bytes (the
 * all-zero hash is an ordinary key), a device-side count of distinct keys and a sticky error word.
 * Probes take at most `cells` steps; a key that finds no cell sets the capacity bit (the keys that
 * found one stay), reported as PZ_ERANGE by pz_block_set_count / _read.  Two buffer sets: a reserve
 * that grows rehashes into the other one on the device.  Calls on one set are ordered by the caller
 * (one stream, or its own events).  Thread-safe per handle.
 *
 * pz_block_set_new: the set a chain resumes with (NewBeaconChain over a stored DB, core.go:59-95):
 * n hashes (n x 32 bytes, host, any alignment; duplicates count once) in a table of the smallest
 * power of two >= 2 * max(n, min_keys) cells.  PZ_EINVAL: out NULL, n > 0 with hashes NULL, n or
 * min_keys above 2^30. */
typedef struct pz_block_set pz_block_set;
int  pz_block_set_new(const uint8_t* hashes, uint64_t n, uint64_t min_keys, int device, pz_block_set** out);
void pz_block_set_free(pz_block_set* set);
/* The number of distinct keys (no reference counterpart: the DB is not counted); waits for the stream
 * of the set's last call.  *count is filled also when the sticky PZ_ERANGE is returned. */
int  pz_block_set_count(pz_block_set* set, uint64_t* count);
/* Every key, in any order (no reference counterpart: the DB is not iterated): *count receives their
 * number, and when cap >= *count hashes receives them (cap x 32 bytes).  Waits as _count does. */
int  pz_block_set_read(pz_block_set* set, uint8_t* hashes, uint64_t cap, uint64_t* count);
/* hasBlock (core.go:560-562) for n hashes (n x 32 bytes, 16-byte aligned device memory): d_out[q] = 1
 * iff hash q is a key.  One launch, a lane per query, plain loads, on the caller's stream.
 * PZ_EINVAL, before any launch: a NULL set; with n > 0 a NULL or misaligned d_hashes or a NULL d_out;
 * n >= 2^31.  n == 0 launches nothing. */
int  pz_dev_block_set_contains(pz_block_set* set, const uint8_t* d_hashes, uint64_t n, uint8_t* d_out, void* stream);
/* hasBlock (core.go:560-562) over host pointers (any alignment), synchronous. */
int  pz_block_set_contains(pz_block_set* set, const uint8_t* hashes, uint64_t n, uint8_t* out);
/* saveBlock's key (core.go:565-577; service.go:324) for the caller that decides for itself -- the
 * transition block's path, one-block callers: of n hashes (n x 32 bytes, 16-byte aligned device
 * memory) those with d_take[j] != 0 (NULL: all) become keys; a hash that is already a key, or that
 * the call holds twice, counts once.  One launch of one workgroup on the caller's stream, no scratch:
 * per tile of 1,024 hashes a lane claims the first empty cell of its probe with a tentative claim
 * that carries its index, a lane that reads a claim compares against that input hash, and after a
 * barrier the lane whose claim stands writes the key.  PZ_EINVAL as _contains (d_out apart).  The
 * caller reserves first: with fewer than n free cells the capacity bit may be set. */
int  pz_dev_block_set_insert(pz_block_set* set, const uint8_t* d_hashes, const uint8_t* d_take /* optional */, uint64_t n,
                             void* stream);
/* saveBlock's key (core.go:565-577) over host pointers (any alignment), synchronous; reserves for
 * the n hashes itself. */
int  pz_block_set_insert(pz_block_set* set, const uint8_t* hashes, const uint8_t* take /* optional */, uint64_t n);
/* Room for min_keys keys (no reference counterpart: the DB grows by itself): when 2 * min_keys exceeds
 * the cells, every key is rehashed on the device, on the caller's stream, into a table of the
 * smallest power of two that holds them; otherwise nothing happens.  The host decides from the cell
 * count it keeps: nothing is read back.  PZ_EINVAL: a NULL set, min_keys above 2^30. */
int  pz_dev_block_set_reserve(pz_block_set* set, uint64_t min_keys, void* stream);
/* The same reserve (no reference counterpart), synchronous. */
int  pz_block_set_reserve(pz_block_set* set, uint64_t min_keys);

/* The parent check (service.go:261-269) for a RUN of nblocks decoded blocks, in block order, with the
 * blocks of the run saving each other as the reference's loop would (service.go:324):
 *   parent_j = BytesToHash of field 1: bytes[bytes_beg[5j] .. + bytes_len[5j]) (absent: the zero hash;
 *              a span that leaves [0, nbytes) refuses the block);
 *   free_j   = slot_number[j] <= 1 (service.go:267);
 *   open0_j  = block_status[j] == PZ_OK and the block gate's report over the same att_first,
 *              rec_status and att_status is not 0: the gate would open block j if its parent is saved;
 *   link_j   = the largest i < j with block_hash[i] == parent_j and open0_i, or none;
 *   parent_ok[j] = free_j or parent_j is in the set or (link_j exists and saved0[link_j]);
 *   saved0[j]    = open0_j and parent_ok[j];
 *   block_status_out[j] = block_status[j] where parent_ok[j], else PZ_ENOTFOUND.
 * The largest open copy suffices (blockparents_dev.h has the proof).  Hand block_status_out to
 * pz_dev_block_gate: its report is then non-zero exactly where saved0 holds.  CanProcessBlock
 * (service.go:272, :308) stays the caller's, folded into block_status.  The set is only read.
 *
 * A memset and three dependent launches on the caller's stream, whatever nblocks; no workgroup waits
 * for another, the host reads nothing: (1) a lane per block takes open0 and enters the open blocks
 * into a run table in scratch, keyed by block_hash; (2) a lane per block probes the set and the run
 * table for parent_j; (3) one workgroup resolves the chains by ceil(log2 nblocks) double-buffered
 * pointer-jumping rounds and writes the three outputs.
 * PZ_EINVAL, before any launch: a NULL set or batch; nblocks >= 2^31; with nblocks > 0 a NULL
 * bytes_beg, bytes_len, slot_number, block_hash, att_first, block_status, parent_ok, saved0 or
 * block_status_out, nbytes > 0 with bytes NULL, natt > 0 with att_status NULL, (device form) a NULL or
 * misaligned d_scratch, a block_hash that is not 16-byte aligned.  nblocks == 0 launches nothing. */
typedef struct pz_block_parents_batch {   /* every member a pointer or a uint64_t */
  uint64_t nblocks;
  const uint8_t*  bytes;            /* nbytes: the received blocks (what pz_unwire_blocks split) */
  uint64_t nbytes;
  const uint64_t* bytes_beg;        /* nblocks*5: pz_block_cols_out.bytes_beg (entry 5j is read) */
  const uint32_t* bytes_len;        /* nblocks*5: pz_block_cols_out.bytes_len */
  const uint64_t* slot_number;      /* nblocks: pz_block_cols_out.slot_number */
  const uint8_t*  block_hash;       /* nblocks x 32: Block.Hash(), pz_dev_blake2b512_spans over the blocks */
  const uint64_t* att_first;        /* nblocks + 1: pz_block_gate_batch.att_first */
  const int32_t*  block_status;     /* nblocks: what pz_block_gate_batch.block_status would have been */
  const int32_t*  rec_status;       /* optional, natt: pz_block_gate_batch.rec_status */
  const int32_t*  att_status;       /* natt: pz_block_gate_batch.chk.status */
  uint64_t natt;                    /* pz_block_gate_batch.chk.natt */
  uint8_t*  parent_ok;              /* nblocks */
  uint8_t*  saved0;                 /* nblocks */
  int32_t*  block_status_out;       /* nblocks: feed it to pz_block_gate_batch.block_status */
} pz_block_parents_batch;
/* The bytes of d_scratch (no reference counterpart). */
uint64_t pz_block_parents_scratch_bytes(uint64_t nblocks);
/* service.go:261-269 over a run, device pointers, on the caller's stream, asynchronous. */
int pz_dev_block_parents(pz_block_set* set, const pz_block_parents_batch* b, void* d_scratch, void* stream);
/* service.go:261-269 over a run, host pointers (any alignment), synchronous. */
int pz_block_parents(pz_block_set* set, const pz_block_parents_batch* b);
/* saveBlock (service.go:324) for the run the walk has decided: block_hash[j] becomes a key for every j
 * with walk[j] saved or candidate (1 or 2: pz_block_walk_batch.walk); deferred blocks, at or past the
 * walk's stop, and blocks that did not go on are untouched.  With d_flags given (pz_block_gate_batch
 * .flags) and its bit 0 set -- the reference panics in the run -- nothing is inserted.  d_count_out
 * (optional, one u64, 8-byte aligned) receives the set's count after the insert.  One launch of one
 * workgroup, as pz_dev_block_set_insert.  PZ_EINVAL, before any launch: a NULL set; nblocks >= 2^31;
 * with nblocks > 0 a NULL or misaligned d_block_hash or a NULL d_walk.  nblocks == 0 launches
 * nothing. */
int pz_dev_block_set_insert_walked(pz_block_set* set, const uint8_t* d_block_hash, const uint8_t* d_walk,
                                   const uint32_t* d_flags /* optional */, uint64_t nblocks, uint64_t* d_count_out /* optional */,
                                   void* stream);

/* ---- H: the attestation store batch of a run of blocks --------------------------------------------
 * What blockProcessing writes to the database for every attestation it accepts (blockchain/
 * service.go:281-301): saveAttestation stores the record under Attestation.Key() (core.go:650-658,
 * types/attestation.go:61-77) and saveAttestationHash appends Attestation.Hash() (types/attestation.go:
 * 50-59) to the block's AttestationHashes list (core.go:745-760).  The batch of a run is selected,
 * hashed and encoded on the device from the columns the run's other entry points left there.
 *
 * Row r of block j = att_block[r] is SAVED when j < *stop (NULL: nblocks; a deferred block is written
 * by the call that processes it), block_status[j] == PZ_OK (the decoder's status with every record's
 * folded in: a block with a non-canonical block or record is refused whole), parent_ok[j] != 0
 * (service.go:261-269), att_status[r] == PZ_ATT_PROCESSED and rec_status[r] == PZ_OK (NULL: all).  The
 * rule does not read CanProcessBlock (tested at service.go:308, after the saves at :288-297) nor the
 * outcome of the block's last attestation (:304): blockstore_dev.h states it once.
 *
 * select, with m the number of saved rows: rows[i] (i < m) = the i-th saved row in ascending order,
 * span[2 i], span[2 i + 1] = its att_beg, att_end -- the bytes saveAttestation writes, since only
 * canonical records get here -- first[j] (j <= nblocks) = the number of saved rows before row
 * att_first[j], so that block j's are [first[j], first[j + 1]), and *count = m.  Entries of rows and
 * span past m are not written.
 * digests, over the m rows select left: hash[32 i ..] = Attestation.Hash() = blake2b.Sum512 of
 * bytes[span[2 i], span[2 i + 1]) truncated to 32 bytes (4 readable bytes past `bytes`, the span
 * hash's contract); key[32 i ..] = Attestation.Key() of row rows[i] of the natt rows of `a`, as
 * pz_dev_attestation_keys makes it (a rows[i] >= natt gets a zero key); lists[34 i ..] = 0a 20 |
 * hash[i], the proto3 encoding of one AttestationHashes.attestation_hash element (messages.proto:
 * 128-130): block j's appended bytes are lists[34 first[j] .. 34 first[j + 1]).  Exactly 34 m bytes of
 * lists are written.
 *
 * select is four dependent launches on the caller's stream (size, scan, write, first: the
 * reduce-then-scan of DESIGN.md §3), digests three independent ones (the span hash, the key kernel
 * through the row list, the entries as whole dwords); no workgroup waits for another, the host reads
 * nothing.  PZ_EINVAL, before any launch -- select: a NULL batch; nblocks >= 2^31; natt >= 2^32; with
 * nblocks > 0 and natt > 0 a NULL att_first, block_status, parent_ok, att_block, att_status, att_beg,
 * att_end, rows, span, first or count; (device form) a NULL or misaligned d_scratch, a span that is
 * not 16-byte aligned, any other pointer that is not aligned to its element.  digests: a NULL batch;
 * m > natt; natt >= 2^32; with m > 0 a NULL bytes, rows, span, key, hash, lists or `a`, offsets of `a`
 * without their data column; (device form) a span, key or hash that is not 16-byte aligned, rows or
 * lists not 4-byte aligned; (host form) a rows[i] >= natt, a span that is inverted or leaves
 * [0, nbytes), offsets of `a` that are not monotone.  nblocks == 0 or natt == 0 (select) and m == 0
 * (digests) launch nothing; the host form of select then sets *count and first[0 .. nblocks] to 0. */
typedef struct pz_block_store_batch {   /* every member a pointer or a uint64_t */
  uint64_t nblocks;
  const uint64_t* att_first;     /* nblocks + 1: pz_block_cols_out.att_first */
  const int32_t*  block_status;  /* nblocks: pz_block_cols_out.status with the records' statuses folded in */
  const uint8_t*  parent_ok;     /* nblocks: pz_block_parents_batch.parent_ok */
  const uint64_t* stop;          /* optional, one word: pz_block_cycle_batch.result (word 0), read on the device */
  uint64_t natt;
  const uint32_t* att_block;     /* natt: pz_block_cols_out.att_block */
  const int32_t*  att_status;    /* natt: pz_att_check_batch.status */
  const int32_t*  rec_status;    /* optional, natt: pz_attestation_cols_out.status */
  const uint64_t* att_beg;       /* natt: pz_block_cols_out.att_beg */
  const uint64_t* att_end;       /* natt: pz_block_cols_out.att_end */
  uint32_t* rows;                /* room for natt; m written by select, read by digests */
  uint64_t* span;                /* room for natt x 2; m x 2 written by select, read by digests */
  uint64_t* first;               /* nblocks + 1, select */
  uint64_t* count;               /* one word, select: m */
  const uint8_t* bytes;          /* digests: the received blocks' bytes the spans point into */
  uint64_t nbytes;               /* the host form uploads this many */
  uint8_t* key;                  /* digests: m x 32 */
  uint8_t* hash;                 /* digests: m x 32 */
  uint8_t* lists;                /* digests: 34 m */
} pz_block_store_batch;
/* The bytes of select's d_scratch (no reference counterpart). */
uint64_t pz_block_store_scratch_bytes(uint64_t nblocks, uint64_t natt);
/* Which rows service.go:281-301 saves, device pointers, on the caller's stream, asynchronous. */
int pz_dev_block_store_select(const pz_block_store_batch* b, void* d_scratch, void* stream);
/* Key, Hash and the list entries of the saved rows (core.go:650-658, :745-760), device pointers (`a`
 * holds device pointers too), on the caller's stream, asynchronous. */
int pz_dev_block_store_digests(const pz_block_store_batch* b, const pz_attestation_cols* a, uint64_t m, void* stream);
/* Which rows service.go:281-301 saves, host pointers (any alignment), synchronous. */
int pz_block_store_select(const pz_block_store_batch* b);
/* Key, Hash and the list entries of the saved rows (core.go:650-658, :745-760), host pointers (any
 * alignment), synchronous. */
int pz_block_store_digests(const pz_block_store_batch* b, const pz_attestation_cols* a, uint64_t m);

/* ---- R: ActiveState.PendingAttestations resident on the device --------------------------------
 * The attestations a block contributes (processedAttestations, blockchain/service.go:280-301)
 * become ActiveState.PendingAttestations (computeNewActiveState, core.go:223-237) and feed the
 * cycle transition: processCrosslinks, CalculateRewards and the Slot > lastStateRecalc filter
 * (core.go:433-457).  The handle owns that list on one device as the full pz_attestation_cols
 * column set (three scalars, three bytes CSRs, the element CSR of field 7 with oblique_first,
 * aggregate_sig with aggregate_sig_first) plus two columns: `committee` (u32, the checks'
 * committee id) and `shard32` (u32, shard_id saturated to UINT32_MAX: a shard of 2^32 or more
 * still raises the epoch's PZ_XLERR_SHARD).  It is appended to from the decoder's columns and the
 * checks' outputs, pruned by slot, and read in place: as the epoch kernels' attestation inputs
 * (pz_epoch_batch.bits / boffs = attester_bitfield(+_offs), att_comm = committee, att_shard =
 * shard32), as pz_attestation_cols for pz_dev_wire_attestations(field_num = 1) (the stored
 * ActiveState's field 1, types/state.go:141), and as the crosslink winners' ShardBlockHash.
 *
 * caps[7], in the order of the decoder's totals with "rows" first: rows, justified_block_hash
 * bytes, shard_block_hash bytes, bitfield bytes, elements, element bytes, sig values.  They are
 * what the pool starts with: pz_[dev_]att_pool_reserve raises them on the device, as append grows
 * the Go slice (core.go:223-237), and pz_[dev_]att_pool_need tells what an append would add.
 * Seven running counts live on the device.  Two buffer sets ping-pong for the prune and the
 * reserve; every bytes column has the 4 readable bytes of slack the digest kernels' contract asks
 * for.
 *
 * Append and prune are the same four dependent launches on the caller's stream (size, scan,
 * commit, write: DESIGN.md §3); no workgroup waits for another.  A call that would exceed any of
 * the seven capacities changes nothing and sets the sticky capacity error: it lands whole or not
 * at all.  Calls on one pool are ordered by the caller (one stream, or its own events).
 * Thread-safe per handle. */
typedef struct pz_att_pool pz_att_pool;
/* types.NewActiveState's pending list (types/state.go:39), empty.  PZ_EINVAL: a zero row capacity. */
int      pz_att_pool_new(const uint64_t caps[7], int device, pz_att_pool** out);
void     pz_att_pool_free(pz_att_pool* pool);
/* The scratch an append of n rows needs (no reference counterpart). */
uint64_t pz_att_pool_scratch_bytes(uint64_t n);
/* processedAttestations = append(processedAttestations, attestation) (service.go:300) followed by
 * NewPendingAttestation / append(PendingAttestations, ...) (core.go:223-237): appends, in row
 * order, every row of `a` with status[i] == PZ_ATT_PROCESSED and, when take is given, take[i] != 0.
 * pz_attestation_cols' NULL rules hold (a NULL scalar is 0, NULL offsets are empty ranges).
 * Offsets must be non-decreasing, as the decoder's are; a kept row with an inverted range lands
 * with zero scalars, six empty ranges and committee UINT32_MAX, and sets a sticky PZ_EINVAL bit.
 * PZ_EINVAL, before any launch: with n > 0 a NULL a, status or committee, offsets without their
 * data column (oblique_first also wants oblique_offs), d_scratch NULL or not 16-byte aligned.
 * n == 0 launches nothing.  Device pointers, caller's stream, asynchronous. */
int pz_dev_att_pool_append(pz_att_pool* pool, const pz_attestation_cols* a, uint64_t n, const int32_t* status,
                           const uint32_t* committee, const uint8_t* take /* optional */, void* d_scratch, void* stream);
/* The same append (service.go:300, core.go:223-237) over host pointers (ranges start at 0),
 * synchronous; waits for the stream of the pool's last call first.  Errors the kernels find are
 * sticky and reported by pz_att_pool_counts / pz_att_pool_read, not here. */
int pz_att_pool_append(pz_att_pool* pool, const pz_attestation_cols* a, uint64_t n, const int32_t* status,
                       const uint32_t* committee, const uint8_t* take /* optional */);
/* stateRecalc's filter, core.go:444-450: keeps, in order, the rows with slot > last_state_recalc.
 * Writes into the other buffer set, then the sets swap.  Caller's stream, asynchronous. */
int pz_dev_att_pool_prune(pz_att_pool* pool, uint64_t last_state_recalc, void* stream);
/* len(PendingAttestations()) (types/state.go:164) and the six other counts, in caps' order.  Waits for the last call's
 * stream.  The sticky error comes first (PZ_EINVAL for an inverted range, else PZ_ERANGE when a
 * call was dropped for capacity); the counts are filled all the same. */
int pz_att_pool_counts(pz_att_pool* pool, uint64_t counts[7]);
/* PendingAttestations() (types/state.go:164) as device pointers into the live buffer set,
 * valid until the next prune, reserve or free; any of the three outputs may be NULL.  No device call. */
int pz_att_pool_view(pz_att_pool* pool, pz_attestation_cols* cols, const uint32_t** committee, const uint32_t** shard32);
/* Host download of PendingAttestations() (types/state.go:164; tests, persistence): the fourteen columns of out (its
 * n_oblique, last_byte and status are not touched; a NULL column is skipped) and committee
 * (optional).  caps: as pz_unwire_attestations' (the rows are sized from pz_att_pool_counts);
 * PZ_ERANGE, nothing written, when a count exceeds its capacity.  Same waiting and sticky error as
 * pz_att_pool_counts, the outputs filled all the same. */
int pz_att_pool_read(pz_att_pool* pool, const pz_attestation_cols_out* out, uint32_t* committee, const uint64_t caps[6]);
/* Host, synchronous: field 5 (ShardBlockHash) of the named rows, out[offs[k] .. offs[k+1]) for
 * rows[k]; offs holds nrows + 1 entries: what a crosslink winner writes into its record,
 * core.go:550-554.  PZ_EINDEX for a row the pool does not hold, PZ_ERANGE (offs filled) when the
 * bytes exceed cap. */
int pz_att_pool_shard_block_hashes(pz_att_pool* pool, const uint32_t* rows, uint64_t nrows, uint8_t* out, uint64_t cap,
                                   uint64_t* offs);
/* The seven capacities now (no reference counterpart: a Go slice's cap is not observable here).
 * Host only, no device call. */
int pz_att_pool_capacity(pz_att_pool* pool, uint64_t caps[7]);
/* append's own growth of PendingAttestations (core.go:223-237; types/state.go:169): the capacities
 * become max(cap, min_caps) column by column, exactly.  Where every min_caps[c] <= cap[c] nothing
 * happens and nothing is launched.  Otherwise ONE launch on the caller's stream
 * (pz_att_pool_move_kernel) copies the live prefix of every column into the other buffer set,
 * grown first, and the sets swap; the host decides from the capacities it keeps and reads nothing
 * back.  The seven counts, the rows and their order, every column's contents, committee, shard32
 * and the sticky error word (both bits) are unchanged, and every entry point of the handle works
 * on the grown pool.  The set left behind stays allocated, so a kernel already queued over
 * pz_att_pool_view still reads valid memory, and grows when a prune or a reserve next writes into
 * it; the pool's own prune scratch follows caps[0].  pz_att_pool_view's pointers are valid until
 * the next prune, free or reserve.  PZ_EINVAL, before any launch: a NULL pool or min_caps, a
 * min_caps[c] of 2^40 or more (what pz_att_pool_new refuses).  PZ_EDEVICE: an allocation failed;
 * the pool is as it was.  Caller's stream, asynchronous, ordered there like every call on the
 * handle. */
int pz_dev_att_pool_reserve(pz_att_pool* pool, const uint64_t min_caps[7], void* stream);
/* The same growth (core.go:223-237; types/state.go:169), synchronous; waits for the stream of the
 * pool's last call first. */
int pz_att_pool_reserve(pz_att_pool* pool, const uint64_t min_caps[7]);
/* The scratch pz_dev_att_pool_need over n rows needs (no reference counterpart). */
uint64_t pz_att_pool_need_scratch_bytes(uint64_t n);
/* What pz_[dev_]att_pool_append of these rows would add to the seven counts (the rows
 * processedAttestations keeps, service.go:299-300), per take column: d_need[k][c] is the sum over
 * the rows with status[i] == PZ_ATT_PROCESSED and take_k[i] != 0 (a NULL take: every PROCESSED
 * row; with both NULL the two rows of the output are equal) of the row's seven sizes, an inverted
 * row counting as the empty row it lands as.  The append's own size and scan launches without a
 * commit; no pool is touched and no sticky bit is set.  pz_attestation_cols' NULL rules hold.
 * n == 0 launches nothing and queues a memset: the output is zeros.  PZ_EINVAL, before any launch:
 * with n > 0 a NULL a or status, offsets without their data column; d_need NULL or not 8-byte
 * aligned, d_scratch NULL or not 16-byte aligned.  Device pointers, caller's stream, asynchronous. */
int pz_dev_att_pool_need(const pz_attestation_cols* a, uint64_t n, const int32_t* status,
                         const uint8_t* take0 /* optional */, const uint8_t* take1 /* optional */,
                         uint64_t* d_need /* [2][7] */, void* d_scratch, void* stream);
/* The same sums (service.go:299-300) over host pointers (ranges start at 0), synchronous, on the
 * current device. */
int pz_att_pool_need(const pz_attestation_cols* a, uint64_t n, const int32_t* status,
                     const uint8_t* take0 /* optional */, const uint8_t* take1 /* optional */, uint64_t need[2][7]);

/* ---- R: stateRecalc over the resident pool and vote cache -----------------------------------------
 * The cycle transition (stateRecalc, blockchain/core.go:398-497) as one call: the justification
 * loop over the vote cache (core.go:411-431), processCrosslinks, CalculateRewards and the
 * next-cycle balance over the pending-attestation pool (core.go:433-464), the new crosslink
 * records (core.go:549-555), the new CrystallizedState's scalars (core.go:467-478) and the pool's
 * prune (core.go:444-450).  pz_recalc_state owns, on one device, the CrystallizedState's side:
 * scalars[PZ_RS_COUNT] (u64, the indices below, the rest zero), the crosslink records as columns
 * (rec_dynasty, rec_slot u64; rec_hash at hash_stride bytes a record with rec_hash_len u32), the
 * last call's winners and a sticky error word.  hash_stride is fixed at creation, a multiple of 16
 * in [32, 256].  The validators (balance, start, end) and the committee CSR stay the caller's
 * device arrays.  Single device: the epoch runs with pop_world = 1 and no co_index.
 *
 * One call is, on the caller's stream (no workgroup waits for another):
 *   1 a fit check over the pool's rows and the call's ONE wait, for the pool's seven counts, the
 *     handle's lastStateRecalc and the check's flag (pz_epoch_batch.natt, max_inst_bytes and the
 *     prune's bound are host values).  A pending ShardBlockHash longer than hash_stride -- on any
 *     row: any could win -- is PZ_ERANGE and nothing changes.  The check can only refuse.
 *   2 the justification: one wave, lane i looks RecentBlockHashes()[i] up in the cache (0 with a
 *     NULL cache), 3 * total >= 2 * TotalDeposits mod 2^64, and the loop of core.go:411-431 runs
 *     over the ballot, slot = lastStateRecalc - 64 + i and slot - 64 wrapping as Go's do.
 *   3 pz_dev_epoch_count then pz_dev_epoch_finish, one instance over pz_att_pool_view; dynasty,
 *     total_deposit and rec_dynasty are the handle's own memory.
 *   4 the commit.  Where the reference panics -- scal[PZ_SCAL_ERR_XL] != 0, or pop * 32 * 3 >=
 *     2 * TotalDeposits mod 2^64 with PZ_SCAL_NACT > 0 and PZ_SCAL_ERR_RWD != 0 -- the sticky
 *     PZ_EINDEX bit is set, nothing of the handle is written, the balances are untouched (the
 *     epoch kernels' contract) and the pool's contents are unspecified.  Otherwise every record
 *     with a winner becomes {CurrentDynasty, block_slot, the winning row's ShardBlockHash}, and
 *     the scalars become lastStateRecalc + 64, the loop's three values, TotalDeposits =
 *     scal[PZ_SCAL_NEXT_BAL] and CurrentDynasty = 0 (the reference's new state leaves it unset).
 *   5 pz_dev_att_pool_prune(pool, lastStateRecalc).
 * Calls on the three objects are ordered by the caller (one stream, or its own events).
 * Thread-safe per handle. */
#define PZ_RS_LAST_STATE_RECALC   0
#define PZ_RS_JUSTIFIED_STREAK    1
#define PZ_RS_LAST_JUSTIFIED_SLOT 2
#define PZ_RS_LAST_FINALIZED_SLOT 3
#define PZ_RS_CURRENT_DYNASTY     4
#define PZ_RS_TOTAL_DEPOSITS      5
#define PZ_RS_COUNT               8
typedef struct pz_recalc_state pz_recalc_state;
/* NewCrystallizedState (types/state.go:34): its scalars and CrosslinkRecords from host pointers;
 * the records' hashes are CSR (rec_hash_offs holds nrec + 1 entries).  nrec may be 0.  PZ_EINVAL: a
 * bad hash_stride, NULL scalars, NULL columns with nrec > 0; PZ_ERANGE: a record's hash is longer
 * than hash_stride. */
int  pz_recalc_state_new(uint32_t nrec, uint32_t hash_stride, const uint64_t scalars[PZ_RS_COUNT],
                         const uint64_t* rec_dynasty, const uint64_t* rec_slot, const uint8_t* rec_hash,
                         const uint64_t* rec_hash_offs, int device, pz_recalc_state** out);
void pz_recalc_state_free(pz_recalc_state* st);
/* Host download of the scalars, the records (rec_hash: nrec x hash_stride bytes, zero behind each
 * record's rec_hash_len) and the last call's winner[nrec] (one pool row per record before the
 * prune, 0xFFFFFFFF: none; core.go:549-555); any output may be NULL.  Waits for the last call's
 * stream.  The sticky error comes first (PZ_EINDEX where stateRecalc panics); the outputs are
 * filled all the same and hold the state before the panicking call. */
int  pz_recalc_state_read(pz_recalc_state* st, uint64_t scalars[PZ_RS_COUNT], uint64_t* rec_dynasty, uint64_t* rec_slot,
                          uint8_t* rec_hash, uint32_t* rec_hash_len, uint32_t* winner);
typedef struct pz_recalc_batch {           /* device pointers */
  uint64_t nval; uint64_t* balance; const uint64_t *start, *end;
  const uint32_t* members; const uint64_t* coffs;   /* committees, CSR, full */
  const uint8_t* recent; uint64_t n_recent;         /* RecentBlockHashes(), BytesToHash-normalised, 16-B aligned */
  uint64_t block_slot;                              /* the transition block's SlotNumber */
} pz_recalc_batch;
/* The scratch one call needs (no reference counterpart); rows_cap: the pool's row capacity. */
uint64_t pz_state_recalc_scratch_bytes(uint64_t nval, uint64_t rows_cap, uint32_t nrec);
/* stateRecalc, core.go:398-497, as above.  cache may be NULL (no entry: every total 0).
 * PZ_EINDEX before any launch, nothing changed, when n_recent < 64 (the panic of core.go:413).
 * PZ_EINVAL, before any launch: a NULL state, pool, batch, scratch or batch member; recent or
 * d_scratch not 16-byte aligned; nval different from the cache's; objects on different devices.
 * PZ_ERANGE from the fit check, nothing changed.  A panic the kernels find is sticky and reported
 * by pz_recalc_state_read, not here. */
int pz_dev_state_recalc(pz_recalc_state* st, pz_att_pool* pool, pz_vote_cache* cache /* NULL: no entry */,
                        const pz_recalc_batch* b, void* d_scratch, void* stream);

/* ---- a2 / R: the two states' proto3 bytes and roots from the resident objects -----------------------
 * What PersistActiveState / PersistCrystallizedState store (blockchain/core.go:161-177, proto.Marshal
 * at types/state.go:141, 240) and what ActiveState.Hash() / CrystallizedState.Hash() hash
 * (types/state.go:138-149, 237-248), from pz_att_pool, pz_recalc_state and the caller's validator
 * columns where they lie.  In the kernels these entry points add (wire_state.hip) no workgroup waits
 * for another; pz_dev_wire_validators and pz_dev_wire_attestations run inside them as they are.
 *
 * ShardAndCommitteesForSlots (CrystallizedState field 12, messages.proto:72, 75-77, 87-90; replaces
 * that span of proto.Marshal at types/state.go:240) from the committee table in pz_att_check_batch's
 * form plus the committees' members (pz_recalc_batch's CSR): array a holds entries arr_offs[a] ..
 * arr_offs[a+1]; entry e has shard arr_shard[e] and the members of committee arr_comm[e] (entries
 * may share a committee).  Per array: the key of field_num, the length, then per entry 0a, length,
 * shard_id (field 1, absent when 0) and committee (packed field 2, absent when empty).  field_num
 * follows pz_wire_validators' rule (0: the arrays' bare bodies). */
typedef struct pz_committee_table {
  uint64_t narr;                   /* len(ShardAndCommitteesForSlots) */
  const uint64_t* arr_offs;        /* narr+1, arr_offs[0] == 0 */
  const uint64_t* arr_shard;       /* entry -> ShardId */
  const uint32_t* arr_comm;        /* entry -> committee id */
  uint64_t ncomm;
  const uint64_t* coffs;           /* ncomm+1 */
  const uint32_t* members;         /* committee c = members[coffs[c] .. coffs[c+1]) */
} pz_committee_table;
/* Upper bound of the encoded length (types/state.go:240's span; sizes d_out). */
uint64_t pz_wire_committees_bound(uint64_t narr, uint64_t nentries, uint64_t members_cap);
/* Device scratch the pz_dev_ form needs (no reference counterpart). */
uint64_t pz_wire_committees_scratch_bytes(uint64_t narr, uint64_t nentries, uint64_t members_cap);
/* Device pointers, caller's stream, four dependent launches (plan, size, scan, write: DESIGN.md §3).
 * nentries and members_cap (an upper bound of the sum of the entries' committee sizes) are host
 * values that size the launches and the scratch; the true sums are read on the device.
 * d_result[0] receives the length and d_result[1] the status: PZ_ERANGE when arr_offs[0] != 0,
 * arr_offs decreases, arr_offs[narr] != nentries, a committee's range is inverted or the member sum
 * exceeds members_cap; PZ_EINDEX when an arr_comm[e] >= ncomm.  With a status nothing of d_out is
 * written, the length is 0 and the call still returns PZ_OK.  Nothing outside d_out[0, length) is
 * written, whatever d_out's alignment; narr == 0 gives length 0 and d_out may be NULL.  d_scratch
 * need not be cleared.  PZ_EINVAL, before any launch: a NULL t, d_result, or (narr > 0) d_out,
 * arr_offs, (nentries > 0) entry columns or coffs, (members_cap > 0) members; d_scratch NULL or not
 * 16-byte aligned; 2^31 arrays or entries, 2^40 members, or field_num >= 2^29; a table the write
 * launch's grid cannot cover: members_cap / 256 + nentries + ceil((nentries + narr) / 256) must stay
 * below 2^31.  The plan and scan launches are one workgroup each, serial over the entries in steps
 * of 1,024. */
int pz_dev_wire_committees(const pz_committee_table* t, uint64_t nentries, uint64_t members_cap, uint32_t field_num,
                           uint8_t* d_out, uint64_t* d_result /* [2]: length, status */, void* d_scratch, void* stream);
/* Host pointers, synchronous (types/state.go:240's span).  The table's status is the return value;
 * PZ_ERANGE also when the encoding exceeds cap (*len still receives its length, nothing written). */
int pz_wire_committees(const pz_committee_table* t, uint64_t nentries, uint32_t field_num, uint8_t* out, uint64_t cap,
                       uint64_t* len);

/* The stored CrystallizedState (messages.proto:59-72; proto.Marshal at types/state.go:240) from a
 * pz_recalc_state: fields 1-5 and 7 are the handle's scalars, field 10 its crosslink records
 * (messages.proto:122-126; zero scalars and an empty hash absent, so a record of three zero fields
 * is 52 00), field 11 pz_dev_wire_validators over v, field 12 the caller's already encoded span
 * (pz_dev_wire_committees; the table changes only at a dynasty transition, core.go:470), and the
 * fields the handle does not hold come by value: */
typedef struct pz_cstate_rest {
  uint64_t crosslinking_start_shard;       /* field 6 */
  uint8_t  dynasty_seed[64];               /* field 8 */
  uint32_t dynasty_seed_len;               /* PZ_EINVAL above 64 */
  uint64_t dynasty_seed_last_reset;        /* field 9 */
} pz_cstate_rest;
/* Bytes d_out must hold (val_bytes_total: both bytes columns' total length); types/state.go:240. */
uint64_t pz_crystallized_state_bound(uint32_t nrec, uint32_t hash_stride, uint64_t nval, uint64_t val_bytes_total,
                                     uint64_t field12_len);
/* Device scratch of the pz_dev_ form (no reference counterpart). */
uint64_t pz_crystallized_state_scratch_bytes(uint64_t nval);
/* proto.Marshal(CrystallizedState), types/state.go:240, on the caller's stream with no wait: the
 * head (fields 1-10) is written right-aligned so that it ends at the host-known head bound H, the
 * validators start at d_out + H, and a tail launch that reads their length on the device copies
 * d_field12 behind them.  The message is d_out[d_span[0], d_span[0] + d_span[1]); nothing outside
 * it is written.  v and d_field12 are device pointers.  PZ_EINVAL, before any launch: a NULL st,
 * rest, v, d_out or d_span, field12_len > 0 with a NULL d_field12, a seed above 64 bytes, d_scratch
 * NULL or not 16-byte aligned. */
int pz_dev_crystallized_state_bytes(pz_recalc_state* st, const pz_cstate_rest* rest, const pz_validator_cols* v, uint64_t nval,
                                    const uint8_t* d_field12, uint64_t field12_len, uint8_t* d_out,
                                    uint64_t* d_span /* [2]: begin, length */, void* d_scratch, void* stream);
/* PersistCrystallizedState's bytes (core.go:170-177) and, with root, CrystallizedState.Hash()
 * (types/state.go:237-248): allocates what it needs, waits for the handle's last call and for its
 * own, copies the message to out (host) and hashes it on the host route of long messages.
 * PZ_ERANGE, *len set, out untouched, when the message exceeds cap.  The handle's sticky PZ_EINDEX
 * comes as pz_recalc_state_read reports it: the outputs are filled all the same and hold the state
 * before the panicking call.  The call runs on the library's own stream and orders itself against
 * st's earlier calls only: what produces v's columns and d_field12 (pz_dev_wire_committees makes no
 * wait) must have completed before it, the caller synchronising those streams first. */
int pz_crystallized_state_read(pz_recalc_state* st, const pz_cstate_rest* rest, const pz_validator_cols* v /* device */,
                               uint64_t nval, const uint8_t* d_field12, uint64_t field12_len, uint8_t* out /* host */,
                               uint64_t cap, uint64_t* len, uint8_t root[32] /* optional */);

/* ---- a2 / R: the stored CrystallizedState read back into the resident objects' columns ---------------
 * NewBeaconChain over a database that holds a state (blockchain/core.go:86-95) for the resident path:
 * replaces proto.Unmarshal of messages.pb.go's CrystallizedState (one heap object per validator) and
 * the repacking into columns.  The inverse of pz_crystallized_state_read: the bytes it emits load back
 * into the same columns.  Exactly the canonical encoding is accepted -- what proto.Marshal emits and
 * PersistCrystallizedState stores (core.go:170-177): field order, minimal varints, zero scalars and
 * empty bytes absent, packed members, no unknown field, no trailing byte.  Anything else is PZ_EINVAL
 * with the offset of the key byte of the first field that breaks the rule (for a run of records that
 * ends where no header stands: that position); pz_chain_new_from_state's host reader stays the lenient
 * path for such input.  prysm_amd/csrc/unwire_state_dev.h states the rules; DESIGN.md §3 the launches.
 *
 * pz_cstate_head: host only, no device (as pz_count_attestations).  Fields 1-10 of cstate[0, len): the
 * PZ_RS_* scalars and the crosslink records as pz_recalc_state_new takes them (rec_hash_offs: nrec + 1
 * entries; rec_hash must hold the hashes' total, below len), *rest the fields the handle does not hold,
 * *body_beg the offset of the first byte behind field 10.  PZ_ERANGE with *nrec set when rec_cap is too
 * small (call again); PZ_EINVAL with *body_beg = the violation's offset when the head is not canonical
 * (a dynasty_seed above 64 bytes included). */
int pz_cstate_head(const uint8_t* cstate, uint64_t len, uint64_t scalars[PZ_RS_COUNT], pz_cstate_rest* rest,
                   uint64_t* rec_dynasty, uint64_t* rec_slot, uint8_t* rec_hash, uint64_t* rec_hash_offs, uint64_t rec_cap,
                   uint64_t* nrec, uint64_t* body_beg);
/* pz_dev_cstate_frame's result record, u64 words: */
#define PZ_CSF_STATUS           0  /* PZ_OK, PZ_EINVAL or PZ_ERANGE (as int64); with a status every other word but OFFSET is 0 */
#define PZ_CSF_OFFSET           1  /* the violation's offset */
#define PZ_CSF_NVAL             2  /* ValidatorRecords (field 11) */
#define PZ_CSF_ADDRESS_BYTES    3  /* the withdrawal_address column's total */
#define PZ_CSF_COMMITMENT_BYTES 4  /* the randao_commitment column's total */
#define PZ_CSF_NARR             5  /* ShardAndCommitteeArrays (field 12) */
#define PZ_CSF_NENTRIES         6  /* ShardAndCommittee entries in all of them */
#define PZ_CSF_NMEMBERS         7  /* committee members in all of them */
#define PZ_CSF_VAL_END          8  /* where field 11's run ends: field 12 is d_bytes[VAL_END, F12_END) */
#define PZ_CSF_F12_END          9  /* == len */
#define PZ_CSF_COUNT            12
/* One ValidatorRecord (key, length, body) may take at most 512 bytes -- the offsets at which the framing
 * lets a chain enter a tile: a body of PZ_CSTATE_RECORD_LIMIT bytes or more is PZ_ERANGE in the result
 * record (the largest canonical record with a 20-byte address and a 32-byte commitment has 111).  The
 * framing's units, for callers that size test inputs: a tile of 4,096 bytes, a group of 64 tiles. */
#define PZ_CSTATE_RECORD_LIMIT 510
#define PZ_CSTATE_TILE_BYTES   4096
#define PZ_CSTATE_GROUP_TILES  64
/* Device scratch of frame and decode for a message of len bytes (no reference counterpart): 2,076 bytes
 * per tile of 4,096 (the tile tables take 2,048 of them) plus 8,204 per group of 64 tiles: below
 * 0.54 * len + 24 KiB.  It need not be cleared. */
uint64_t pz_cstate_scratch_bytes(uint64_t len);
/* Frames field 11 and field 12 of d_bytes[body_beg, len) on the caller's stream, asynchronously, and
 * sizes what decode writes: d_result[PZ_CSF_COUNT] (device).  The caller reads it back -- the load's
 * one wait -- allocates exact-size outputs and calls pz_dev_cstate_decode with the same scratch.  A
 * violation in a record's or an array's headers and fields is reported here; a committee member's in
 * decode.  A message of 4 GiB or more is PZ_ERANGE in the record.  With body_beg == len (no field 11,
 * no field 12; len == 0 included) only the record is written: zeros, both ends len.  PZ_EINVAL, before
 * any launch: d_bytes NULL with len > 0, d_result NULL, d_scratch NULL or not 16-byte aligned,
 * body_beg > len. */
int pz_dev_cstate_frame(const uint8_t* d_bytes, uint64_t len, uint64_t body_beg, void* d_scratch, uint64_t* d_result,
                        void* stream);
/* The outputs: pz_validator_cols and pz_committee_table with pointers the decoder writes through. */
typedef struct pz_validator_cols_out {
  uint64_t* public_key;
  uint64_t* withdrawal_shard;
  uint8_t*  withdrawal_address;            /* ADDRESS_BYTES */
  uint64_t* withdrawal_address_offs;       /* nval + 1 */
  uint8_t*  randao_commitment;             /* COMMITMENT_BYTES */
  uint64_t* randao_commitment_offs;        /* nval + 1 */
  uint64_t* balance;
  uint64_t* start_dynasty;
  uint64_t* end_dynasty;
} pz_validator_cols_out;
typedef struct pz_committee_table_out {
  uint64_t narr;                   /* the frame's NARR */
  uint64_t* arr_offs;              /* narr + 1 */
  uint64_t* arr_shard;             /* nentries */
  uint32_t* arr_comm;              /* nentries: the identity, one committee per entry */
  uint64_t ncomm;                  /* the frame's NENTRIES */
  uint64_t* coffs;                 /* nentries + 1 */
  uint32_t* members;               /* NMEMBERS */
} pz_committee_table_out;
/* Decodes what the frame found, with its scratch, on the caller's stream: every ValidatorRecord into
 * the seven columns (a lane per record) and field 12 into the committee table (members in parallel: an
 * element ends at each byte with a clear top bit).  d_status[2] (device): PZ_OK, or PZ_EINVAL and the
 * offset of the first committee member that is not a minimal varint of a u32; a frame that reported a
 * status is repeated here and nothing is written; sizes in t that are not the frame's are PZ_EINVAL at
 * offset 0.  On error the outputs' contents are unspecified; every write lies inside the sizes the
 * frame reported.  Every output pointer must be an address, also of an empty column.  With len == 0
 * nothing is launched.  PZ_EINVAL, before any launch: a NULL argument or output, d_scratch not
 * 16-byte aligned. */
int pz_dev_cstate_decode(const uint8_t* d_bytes, uint64_t len, void* d_scratch, const pz_validator_cols_out* v,
                         const pz_committee_table_out* t, uint64_t* d_status, void* stream);

/* The stored ActiveState (messages.proto:94-97; proto.Marshal at types/state.go:141) from a
 * pz_att_pool: field 1 is pz_dev_wire_attestations over pz_att_pool_view, field 2
 * (recent_block_hashes) one lane per hash, written at the device-known end of field 1: entry i is
 * 12, its length and the LAST recent_len[i] bytes of row i (common.BytesToHash right-aligns; the
 * genesis state's 128 empty entries, types/state.go:46-57, are 12 00 each).
 * The bound for the pool's seven counts (types/state.go:141; sizes d_out): */
uint64_t pz_active_state_bound(const uint64_t counts[7], uint64_t n_recent);
/* proto.Marshal(ActiveState), types/state.go:141, on the caller's stream.  The call makes ONE wait,
 * for the pool's seven counts (pz_dev_wire_attestations takes its row count from the host), as
 * pz_dev_state_recalc does.  *d_total (device) receives the length; nothing outside
 * d_out[0, *d_total) is written.  PZ_ERANGE, nothing written, when cap is below
 * pz_active_state_bound of those counts.  The pool's sticky error is returned as
 * pz_att_pool_counts returns it, the output written all the same.  d_recent: n_recent x 32 bytes,
 * BytesToHash-normalised; d_recent_len optional (NULL: all 32; values above 32 count as 32). */
int pz_dev_active_state_bytes(pz_att_pool* pool, const uint8_t* d_recent, const uint8_t* d_recent_len, uint64_t n_recent,
                              uint8_t* d_out, uint64_t cap, uint64_t* d_total, void* stream);
/* PersistActiveState's bytes (core.go:161-168) and, with root, ActiveState.Hash()
 * (types/state.go:138-149), over host recent / recent_len; waits for the pool's last call.
 * PZ_ERANGE, *len set, out untouched, when the message exceeds cap. */
int pz_active_state_read(pz_att_pool* pool, const uint8_t* recent, const uint8_t* recent_len, uint64_t n_recent,
                         uint8_t* out, uint64_t cap, uint64_t* len, uint8_t root[32] /* optional */);

typedef struct pz_block_result {
  uint8_t hash[32];      /* Block.Hash() */
  int32_t status;        /* PZ_BLOCK_* */
  int32_t transition;    /* 1: stateRecalc ran for this block */
  uint32_t first_att;    /* index of its first attestation in att_out */
  uint32_t natt;
} pz_block_result;

typedef struct pz_att_result {
  int32_t status;        /* PZ_ATT_* */
  uint32_t msg_len;      /* processAttestation message length */
  uint8_t key[32];       /* Attestation.Key()  (types/attestation.go:61-77) */
  uint8_t hash[32];      /* Attestation.Hash() (types/attestation.go:49-59) */
  uint8_t msg_digest[64];/* blake2b.Sum512(msg) (core.go:290) */
} pz_att_result;

typedef struct pz_chain pz_chain;
int  pz_chain_new(uint64_t nval, int device, pz_chain** out);
/* NewBeaconChain over a database that holds a CrystallizedState (blockchain/core.go:86-95):
 * the chain resumes from the stored encoding `cstate` (the bytes pz_chain_state_bytes returns
 * for the chain's CrystallizedState, which updateHead persists, core.go:170-177) with the
 * genesis ActiveState, exactly as the reference reloads; `saved_hashes` (32 bytes each) are
 * the block hashes the database holds (hasBlock, core.go:591-601), so their children are
 * processed.  PZ_EINVAL when the bytes do not decode (proto.Unmarshal's error). */
int  pz_chain_new_from_state(const uint8_t* cstate, uint64_t len, const uint8_t* saved_hashes, uint64_t nsaved,
                             int device, pz_chain** out);
/* One chain over the ranks of `comm` (blockchain/core.go:300-345,
 * 398-497): each local rank holds the 64-aligned validator range [lo, hi) of the balances, its
 * columns of every vote-cache voter bitmap (so a voter's dedup bit lives on one rank) and its
 * partial VoteTotalDeposit sums; a stateRecalc all-reduces the 64 totals the justification
 * loop reads (65 words with the tally panic flag) and runs the epoch sharded like
 * pz_epoch_state (partial crosslink tallies, bit counts and next-cycle balances all-reduced,
 * rewards on each range).  The block walk, digests and messages run on local rank 0 of every
 * process (one process per GPU replays the same blocks; the device work is split).  Genesis
 * only: every validator stays active, so rank == index.  `comm` must outlive the chain. */
int  pz_chain_new_comm(uint64_t nval, pz_comm* comm, pz_chain** out);
void pz_chain_free(pz_chain* chain);
/* The engine's options (no reference counterpart: placement and test controls; every field 0
 * is the product's choice).  Set them before the chain's first pz_chain_process_blocks call:
 * afterwards a change of tally_forms fails with PZ_EINVAL (msg_batch may change at any time). */
typedef struct pz_chain_options {
  uint64_t msg_batch;    /* processAttestation messages digested in batches of at least this many,
                            sent while the walk goes on (0: one batch at the end of the call) */
  uint32_t tally_forms;  /* tests: the vote-cache tally's general forms forced (PZ_TALLY_*) */
} pz_chain_options;
#define PZ_TALLY_PER_ATTESTATION 1u  /* the per-attestation tally instead of the committee-grouped one */
#define PZ_TALLY_BITS_ROWS       2u  /* every bitfield in the row array, none inline in its record */
#define PZ_TALLY_ID_ROWS         4u  /* every attestation's parent ids as an explicit row, no run */
int  pz_chain_set_options(pz_chain* chain, const pz_chain_options* opts);
/* Number of attestations in a batch of serialized blocks (host only; sizes att_out). */
int  pz_count_attestations(const uint8_t* blocks, const uint64_t* offsets, uint64_t n, uint64_t* count);
/* att_out: capacity att_cap >= the total number of attestations in the batch.
 * A reference panic returns PZ_EINDEX and poisons the chain.  A stateRecalc's device epoch
 * (processCrosslinks, CalculateRewards) is collected at the next transition or at the end of
 * the call, so its panic is reported up to 63 blocks later: the message names the transition's
 * block index and slot, and the result rows of the blocks after that block are undefined (the
 * reference stops at it, blockchain/service.go:345-354). */
int  pz_chain_process_blocks(pz_chain* chain, const uint8_t* blocks, const uint64_t* offsets, uint64_t n,
                             pz_block_result* block_out, pz_att_result* att_out, uint64_t att_cap);
/* State roots (types/state.go:138-149, 237-248): out[0..31] chain ActiveState, [32..63] chain
 * CrystallizedState, [64..127] the candidate's (zero when *has_candidate == 0). */
int  pz_chain_roots(pz_chain* chain, uint8_t out[4 * 32], int* has_candidate);
/* Persistence format: the proto3 encoding the reference stores under activeStateLookupKey /
 * crystallizedStateLookupKey (PersistActiveState / PersistCrystallizedState,
 * blockchain/core.go:161-177, schema.go:17-27) — the bytes the state roots hash.
 * which: 0 chain ActiveState, 1 chain CrystallizedState, 2 / 3 the candidate's (PZ_EINVAL
 * when there is no candidate).  *len receives the size; bytes are written when cap >= *len. */
int  pz_chain_state_bytes(pz_chain* chain, int which, uint8_t* out, uint64_t cap, uint64_t* len);
/* The block vote cache: *count entries (0 when the map is nil); fills hashes[32*i] and
 * totals[i] (VoteTotalDeposit) when cap >= *count. */
int  pz_chain_vote_totals(pz_chain* chain, uint8_t* hashes, uint64_t* totals, uint64_t cap, uint64_t* count);
/* Observability (no reference counterpart; the Go node's pprof wall profile of the same
 * phases): the engine's cumulative wall seconds per phase of pz_chain_process_blocks since the
 * chain was created, out[0..n): parse, digest batch, attestation checks, vote queueing, tally
 * flushes, stateRecalc, message digests, the walk, the whole call, attestation counting, arena
 * waits, message sends / hash log / waits, the tally totals' wait, then two counts (tally-total
 * polls that fell back to the event wait; queued attestations with an explicit parent-id row).
 * The checks and vote queueing are clocked only by the A/B library (they read 0 here).
 * Returns the number of slots the library keeps. */
int  pz_chain_phase_times(pz_chain* chain, double* out, int n);

#ifdef __cplusplus
}
#endif
#endif /* PRYSM_HIP_H */
