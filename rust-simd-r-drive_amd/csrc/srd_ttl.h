// srd_ttl.h -- the TTL cache's rule, once: how an indexed entry becomes a TTL
// verdict (ttl_judge, on top of the read's range rule entry_range), how an
// expiry is made, and which queries of a batch an eviction writes a tombstone
// for.  Plain integer code shared by the kernels (srd_ttl.hip, srd_index.hip),
// the host glue (srd_ops.hip) and a CPU check (tests/sanitize_ttl/
// ttl_check.cpp): outside HIP the qualifiers are empty and the two unaligned
// loads are defined here (inside HIP they are srd_kernels.hip's).
//
// Reference being replaced (jzombie/rust-simd-r-drive v0.16.3-alpha):
//   StorageCacheExt::write_with_ttl / read_with_ttl  extensions/src/storage_cache_ext.rs:23-107
//   NamespaceHasher::namespace                        src/utils/namespace_hasher.rs:33-65
//   TTL_PREFIX                                        extensions/src/constants.rs:20-42
// A TTL entry's payload is le64(expiry) || value, stored under
// compute_hash(le64(xxh3_64(prefix)) || le64(xxh3_64(key))); a read at `now`
// gives the value while now < expiry, deletes the entry otherwise, and calls a
// payload below 8 bytes InvalidData.
#pragma once
#include <stdint.h>

#include "srd_amd.h"
#include "srd_fin.h"

#if defined(__HIPCC__) || defined(__CUDACC__)
#define SRD_TTL_FN __device__ __forceinline__
#else
#define SRD_TTL_FN inline
#endif

namespace srd {

#if !(defined(__HIPCC__) || defined(__CUDACC__))
inline uint64_t ld_u64_unaligned(const uint8_t* f, uint64_t o) {
  uint64_t v = 0;
  for (int k = 0; k < 8; k++) v |= (uint64_t)f[o + k] << (8 * k);
  return v;
}
#endif

// The payload range of the entry whose metadata is at `off`, with the
// reference's bounds, prepad and tombstone rules (read_entry_with_context
// :524-553, par_iter_entries :322-353, EntryIterator::next
// entry_iterator.rs:85-118); false for None (out of range / tombstone).
SRD_TTL_FN bool entry_range(const uint8_t* file, uint64_t flen, uint64_t off, uint64_t* start,
                            uint64_t* end) {
  if (off + 20 > flen) return false;
  const uint64_t prev = ld_u64_unaligned(file, off + 8);  // EntryMetadata.prev_offset
  uint64_t s = prev + prepad64(prev);
  if (off > prev && off - prev == 1 && file[prev] == 0) s = prev;  // tombstone: no prepad
  if (s >= off) return false;
  if (off - s == 1 && file[s] == 0) return false;  // tombstone -> None
  *start = s;
  *end = off;
  return true;
}

constexpr uint32_t TTL_NOT_FOUND = SRD_TTL_NOT_FOUND, TTL_LIVE = SRD_TTL_LIVE, TTL_EXPIRED = SRD_TTL_EXPIRED,
                   TTL_TOO_SHORT = SRD_TTL_TOO_SHORT;
constexpr uint64_t TTL_HEADER = 8;  // le64(expiry) in front of the value

// write_with_ttl's expiry (storage_cache_ext.rs:36-41): now.saturating_add(ttl)
SRD_TTL_FN uint64_t ttl_expiry(uint64_t now, uint64_t ttl) { return now + ttl < now ? ~0ull : now + ttl; }

// read_with_ttl's decision (storage_cache_ext.rs:72-104) for the entry whose
// metadata is at `off`.  [start, end) is the whole payload, header included,
// for LIVE and (0, 0) otherwise; expiry is 0 unless the payload holds one (LIVE,
// EXPIRED).  Reads what entry_range reads and, only when the payload has them,
// its first 8 bytes: nothing outside [0, flen).
struct TtlVerdict {
  uint32_t status;
  uint64_t start, end, expiry;
};
SRD_TTL_FN TtlVerdict ttl_judge(const uint8_t* file, uint64_t flen, uint64_t off, uint64_t now) {
  TtlVerdict v{TTL_NOT_FOUND, 0, 0, 0};
  uint64_t s = 0, e = 0;
  if (!entry_range(file, flen, off, &s, &e)) return v;
  if (e - s < TTL_HEADER) {  // "Data too short to contain TTL"
    v.status = TTL_TOO_SHORT;
    return v;
  }
  v.expiry = ld_u64_unaligned(file, s);
  if (now >= v.expiry) {
    v.status = TTL_EXPIRED;
    return v;
  }
  v.status = TTL_LIVE;
  v.start = s;
  v.end = e;
  return v;
}

// Eviction's choice among a batch: the queries judged EXPIRED are the
// candidates, in batch order; among the candidates of one key the last one
// gets the key's tombstone.  word = the key's slot of live_dedupe_kernel's
// scratch table run over the candidates: 1 + the last candidate position of
// the key.  The kept candidates, in ascending position, are the tombstones.
SRD_TTL_FN bool ttl_evict_candidate(uint32_t status) { return status == TTL_EXPIRED; }
SRD_TTL_FN bool ttl_evict_keeps(uint32_t word, uint64_t j) { return word == (uint32_t)j + 1; }

}  // namespace srd
