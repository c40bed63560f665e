// srd_append.h -- the arithmetic of srd_batch_append_device: how a source
// range is judged, where every entry of the batch lands, and which outcomes
// refuse the batch.  Plain integer code shared by the layout / finish kernels
// (srd_append.hip), the host glue (srd_ops.hip) and a CPU check
// (tests/sanitize_append/append_check.cpp): outside HIP the qualifiers are
// empty.  The work units are the gather's chunks (srd_gather.h); the unit
// table and the CRC combine are every caller's (srd_segments.h, UnitArgs).
//
// Layout (batch_write_with_key_hashes, data_store.rs:847-939, for payloads
// that are no tombstones): with base = roundup64(tail), entry i has its
// payload at P_i = base + pre[i], pre = the exclusive sum of append_slot(len)
// = roundup64(len + 20) -- DESIGN.md 4.7's argument with a base other than 0 --
// its metadata at m_i = P_i + len_i, prev_offset = m_(i-1) + 20 (entry 0: the
// tail), and the store ends at m_(n-1) + 20.
#pragma once
#include <stdint.h>

#include "srd_gather.h"

namespace srd {

// what a source range decides on its own (the order of the reference's tests,
// data_store.rs:864-905; a range outside the blob has no counterpart there)
constexpr uint32_t APPEND_OK = 0;
constexpr uint32_t APPEND_EMPTY = 1;      // "Payload cannot be empty."
constexpr uint32_t APPEND_NULL_BYTE = 2;  // "NULL-byte payloads cannot be written directly." (the layout kernel's one byte read)
constexpr uint32_t APPEND_BAD_RANGE = 3;  // not inside [0, payloads_len)
constexpr uint32_t APPEND_TOO_LONG = 4;   // the entry alone passes the 48-bit offset space

constexpr uint64_t APPEND_TAIL_LIMIT = 1ull << 48;  // KeyIndexer::pack: 48-bit offsets
constexpr uint32_t APPEND_COARSE_SHIFT = 20;

// The range [off, off + len) against a blob of blob_len bytes, by arithmetic
// that cannot wrap (gather_range_status' rule); a refused range is never
// dereferenced.  len == 1 still needs the byte itself (APPEND_NULL_BYTE).
SRD_GA_HD uint32_t append_range_status(uint64_t off, uint64_t len, uint64_t blob_len) {
  if (len == 0) return APPEND_EMPTY;
  if (off > blob_len || len > blob_len - off) return APPEND_BAD_RANGE;
  if (len >= APPEND_TAIL_LIMIT) return APPEND_TOO_LONG;
  return APPEND_OK;
}
SRD_GA_HD uint64_t append_base(uint64_t tail) { return gather_pad64(tail); }
// payload + metadata up to the next entry's payload (len < 2^48: no wrap)
SRD_GA_HD uint64_t append_slot(uint64_t len) { return gather_pad64(len + 20); }
SRD_GA_HD uint64_t append_payload(uint64_t base, uint64_t pre) { return base + pre; }
SRD_GA_HD uint64_t append_meta(uint64_t base, uint64_t pre, uint64_t len) { return base + pre + len; }

// The first refused entry decides the message, as the reference's loop does:
// the error word is the minimum of these over the batch (~0: none)
SRD_GA_HD uint64_t append_err_word(uint64_t i, uint32_t status) { return (i << 8) | status; }
SRD_GA_HD uint32_t append_err_status(uint64_t word) { return (uint32_t)(word & 0xFF); }

// The exclusive sum of n < 2^31 slots of up to 2^48 bytes could wrap; the sum
// of the slots' coarse parts (slot >> 20, each < 2^29) cannot.  With coarse <=
// 2^28 the exact sum is below (2^28 + 1 + n) * 2^20 < 2^52 and can be trusted;
// otherwise it is at least 2^48 + 2^20 and the new tail (the sum less the last
// slot's padding, < 64 bytes) lies beyond 2^48: the batch is refused.
SRD_GA_HD uint64_t append_coarse(uint64_t slot) { return slot >> APPEND_COARSE_SHIFT; }
SRD_GA_HD bool append_sum_exact(uint64_t coarse_sum) {
  return coarse_sum <= (APPEND_TAIL_LIMIT >> APPEND_COARSE_SHIFT);
}
// the new tail from the last entry's prefix and length; false: 2^48 or more
SRD_GA_HD bool append_new_tail(uint64_t tail, uint64_t coarse_sum, uint64_t pre_last, uint64_t len_last,
                               uint64_t* new_tail) {
  if (tail >= APPEND_TAIL_LIMIT || !append_sum_exact(coarse_sum)) return false;
  const uint64_t nt = append_meta(append_base(tail), pre_last, len_last) + 20;  // < 2^48 + 64 + 2^52 + 2^48
  if (nt >= APPEND_TAIL_LIMIT) return false;
  *new_tail = nt;
  return true;
}

}  // namespace srd
