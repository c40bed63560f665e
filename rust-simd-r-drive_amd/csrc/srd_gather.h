// srd_gather.h -- the arithmetic of srd_payload_gather_device: how a query's
// range is judged, how hits are cut into work units (chunks), how a unit finds
// its hit again, and the powers of x a CRC-32 is put together with (a hit's is
// combined from its chunks' raw CRCs as every entry's is: srd_segments.h,
// seg_unit_term).  Plain integer code shared by the layout kernel
// (srd_gather.hip), the unit kernels (srd_units.hip) and a CPU check
// (tests/sanitize_gather/gather_check.cpp): outside HIP the qualifiers are
// empty.
//
// A hit of len bytes has ceil(len / SRD_GATHER_CHUNK) chunks; chunk j covers
// its bytes [j C, min(len, (j + 1) C)).  The units of a batch are the chunks of
// its hits in query order: unit u belongs to the hit i with cpre[i] <= u <
// cpre[i + 1], cpre = the exclusive sum of the chunk counts (cpre[n] = the
// unit count), and is chunk u - cpre[i] of it.
//
// pow8[k] = x^(8 * 2^k) (CrcTables::pow8, DevTables::pow8) behind any pointer
// type.
#pragma once
#include <stdint.h>

#include "srd_amd.h"
#include "srd_crc.h"

#if defined(__HIPCC__) || defined(__CUDACC__)
#define SRD_GA_HD __host__ __device__ __forceinline__
#else
#define SRD_GA_HD inline
#endif

namespace srd {

constexpr uint64_t GATHER_CHUNK = SRD_GATHER_CHUNK;
static_assert(GATHER_CHUNK >= 4096 && GATHER_CHUNK % 4096 == 0, "a unit is a whole number of 4 KiB blocks");

// What the range alone decides: NONE, BAD_RANGE, or a hit (reported as OK
// here; the checksum turns it into OK or BAD_CRC).  A hit lies inside the
// file with its 20-byte metadata: start < end and end + 20 <= file_len, tested
// without an addition that could wrap.
SRD_GA_HD uint32_t gather_range_status(uint64_t start, uint64_t end, uint64_t file_len) {
  if (start == end) return SRD_GATHER_NONE;
  if (start > end || end > file_len || file_len - end < 20) return SRD_GATHER_BAD_RANGE;
  return SRD_GATHER_OK;
}
SRD_GA_HD uint64_t gather_pad64(uint64_t len) { return (len + 63) & ~63ull; }
SRD_GA_HD uint64_t gather_chunks(uint64_t len) { return (len + GATHER_CHUNK - 1) / GATHER_CHUNK; }
SRD_GA_HD uint64_t gather_chunk_len(uint64_t len, uint64_t j) {
  const uint64_t o = j * GATHER_CHUNK;
  return len - o < GATHER_CHUNK ? len - o : GATHER_CHUNK;
}

// the hit of unit u (u < cpre[n]): the last i with cpre[i] <= u -- a query
// without chunks (cpre[i] == cpre[i + 1]) is never the answer
template <class P>
SRD_GA_HD uint64_t gather_unit_hit(P cpre, uint64_t n, uint64_t u) {
  uint64_t lo = 0, hi = n;  // cpre[lo] <= u < cpre[hi]
  while (hi - lo > 1) {
    const uint64_t mid = lo + (hi - lo) / 2;
    if (cpre[mid] <= u) lo = mid;
    else hi = mid;
  }
  return lo;
}

// x^(8 n)
template <class P>
SRD_GA_HD uint32_t gather_xpow8(P pow8, uint64_t n) {
  uint32_t r = kX0;
  for (int k = 0; n; k++, n >>= 1)
    if (n & 1) r = mulp(pow8[k], r);
  return r;
}

// CRC32 from crc_raw: crc32fast's init and xorout 0xFFFFFFFF depend on the
// length alone (srd_crc.h: CRC32(D) = crc_raw(D) ^ CRC32(0^|D|)), the fix the
// batch writer applies
template <class P>
SRD_GA_HD uint32_t gather_final(uint32_t raw, uint64_t len, P pow8) {
  return raw ^ ~mulp(gather_xpow8(pow8, len), 0xFFFFFFFFu);
}

}  // namespace srd
