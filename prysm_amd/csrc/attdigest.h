// What attdigest.hip shows the attestation store (blockstore.hip): Attestation.Key through a row
// list, by the key kernel's own device code.  Not part of the C ABI.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/prysm_hip.h"

namespace pz {

// out[32 i ..] = Key (types/attestation.go:61-77) of source row list[i] of the nsrc rows of `a`, for
// i < n (n > 0); a list entry >= nsrc gets a zero key.  The memory contract is
// pz_dev_attestation_keys'.
hipError_t launch_att_keys_rows(const pz_attestation_cols& a, uint64_t nsrc, const uint32_t* list, uint64_t n, uint8_t* out,
                                hipStream_t s);

// What pz_[dev_]attestation_keys refuse about the columns Key reads: offsets without their data
// column, and (host form, where the offsets can be read) offsets that are not monotone over n rows.
int check_att_key_cols(const pz_attestation_cols* a, uint64_t n, bool host_form);

}  // namespace pz
