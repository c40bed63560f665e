// srd_table.h -- the device KeyIndexer table's rule, once: slot states, probe,
// claim and size arithmetic, for the table's kernels (srd_index.hip,
// srd_index_live.hip), the host entries (srd_ops.hip) and a CPU check
// (tests/sanitize/table_check.cpp): outside HIP the qualifiers are empty.
//
// Open addressing, linear probing over 2^log2cap slots: keys[] then packed[]
// in one allocation of 16 << log2cap bytes.  A slot's state is its packed word:
//   TBL_EMPTY    never used: a probe ends here
//   live         tag16 << 48 | offset48, offset < file_len (never all ones)
//   TBL_DELETED  the slot keeps its key, the key is absent: a probe goes on
//                past it, an insert of the key revives it (no packed value
//                either: tag 0xFFFF with offset 2^48 - 2)
// A slot never returns to TBL_EMPTY, so no probe chain breaks; at most half of
// the slots are not empty (table_admits), so every probe ends.
#pragma once
#include <stdint.h>

#if defined(__HIPCC__) || defined(__CUDACC__)
#define SRD_TBL_HD __host__ __device__ __forceinline__
#else
#define SRD_TBL_HD inline
#endif

namespace srd {

constexpr uint64_t TBL_EMPTY = ~0ull;
constexpr uint64_t TBL_DELETED = ~0ull - 1;
constexpr uint64_t TBL_MIN_CAP = 64;

SRD_TBL_HD uint64_t idx_slot(uint64_t k, uint32_t log2cap) {
  k ^= k >> 29;  // key hashes are XXH3 outputs already; one mix keeps clustered inputs spread
  return (k * 0x9E3779B97F4A7C15ull) >> (64 - log2cap);
}

struct Table {
  uint64_t* keys;
  uint64_t* packed;
  uint32_t log2cap;
};

// The probe for k: the word of k's slot (live or TBL_DELETED) with *slot = that
// slot, or TBL_EMPTY with *slot = the empty slot that ended the probe.
SRD_TBL_HD uint64_t table_find(const Table& t, uint64_t k, uint64_t* slot) {
  const uint64_t mask = (1ull << t.log2cap) - 1;
  uint64_t s = idx_slot(k, t.log2cap);
  for (;;) {  // terminates: at most cap/2 slots are not empty
    const uint64_t p = t.packed[s];
    if (p == TBL_EMPTY || t.keys[s] == k) {
      *slot = s;
      return p;
    }
    s = (s + 1) & mask;
  }
}

// KeyIndexer::get_packed: a deleted key reads as absent (TBL_EMPTY)
SRD_TBL_HD uint64_t table_get(const Table& t, uint64_t k) {
  uint64_t s;
  const uint64_t p = table_find(t, k, &s);
  return p == TBL_DELETED ? TBL_EMPTY : p;
}

// an empty slot's packed word taken for `value` (device: claims run concurrently)
SRD_TBL_HD bool slot_take(uint64_t* word, uint64_t value) {
#if defined(__HIP_DEVICE_COMPILE__)
  return atomicCAS((unsigned long long*)word, (unsigned long long)TBL_EMPTY, (unsigned long long)value) == TBL_EMPTY;
#else
  if (*word != TBL_EMPTY) return false;
  *word = value;
  return true;
#endif
}
// Claim the first empty slot of k's probe chain for (k, value) and return it:
// for a key known to have no slot (no key word is compared) and admitted by
// table_admits.  The key word follows the packed word; no lane of the launch reads it.
SRD_TBL_HD uint64_t table_claim(const Table& t, uint64_t k, uint64_t value) {
  const uint64_t mask = (1ull << t.log2cap) - 1;
  uint64_t s = idx_slot(k, t.log2cap);
  while (!slot_take(t.packed + s, value)) s = (s + 1) & mask;
  t.keys[s] = k;
  return s;
}

// load <= 1/2: `fresh` new slots on top of `used` non-empty ones
SRD_TBL_HD bool table_admits(uint64_t used, uint64_t fresh, uint32_t log2cap) {
  return used + fresh <= (1ull << log2cap) / 2;
}

// the table of n keys: the power of two >= max(TBL_MIN_CAP, 2 n) slots
SRD_TBL_HD uint64_t table_capacity(uint64_t n) {
  uint64_t cap = TBL_MIN_CAP;
  while (cap < 2 * n) cap <<= 1;
  return cap;
}
SRD_TBL_HD uint64_t table_bytes_for(uint64_t n) { return 16 * table_capacity(n); }
// a buffer of table_bytes holds the largest power-of-two table that fits
SRD_TBL_HD uint32_t table_log2cap(uint64_t table_bytes) {
  uint32_t l = 0;
  while (l < 62 && (16ull << (l + 1)) <= table_bytes) l++;
  return l;
}
SRD_TBL_HD bool table_ok(const void* d_table, uint64_t table_bytes) { return d_table && table_bytes >= 16 * TBL_MIN_CAP; }
SRD_TBL_HD Table table_view(const void* d_table, uint64_t table_bytes) {
  const uint32_t l = table_log2cap(table_bytes);
  return Table{(uint64_t*)d_table, (uint64_t*)d_table + (1ull << l), l};
}

}  // namespace srd
