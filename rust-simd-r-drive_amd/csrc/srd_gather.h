// srd_gather.h -- the arithmetic of srd_payload_gather_device: how a query's
// range is judged, how hits are cut into work units (chunks), how a unit finds
// its hit again, and how a hit's CRC-32 is put together from its chunks' raw
// CRCs.  Plain integer code shared by the layout / unit-table / combine
// kernels (srd_gather.hip) and a CPU check (tests/sanitize_gather/
// gather_check.cpp): outside HIP the qualifiers are empty.
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
constexpr int GATHER_LANES = 64;  // the combine's split of a hit's chunks over one wave

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

// crc_raw of the hit's bytes [j0 C, min(len, j1 C)) from the chunks' raw CRCs
// raw[j0 .. j1): one Horner step per chunk, by x^(8 C) for a whole chunk and
// by the last chunk's own length (j0 < j1 <= the hit's chunk count)
template <class R, class P>
SRD_GA_HD uint32_t gather_fold(R raw, uint64_t j0, uint64_t j1, uint64_t len, P pow8) {
  const uint32_t xc = gather_xpow8(pow8, GATHER_CHUNK);
  uint32_t acc = 0;
  for (uint64_t j = j0; j < j1; j++) {
    const uint64_t cl = gather_chunk_len(len, j);
    acc = mulp(cl == GATHER_CHUNK ? xc : gather_xpow8(pow8, cl), acc) ^ raw[j];
  }
  return acc;
}
// the segment of lane l when k chunks are split over GATHER_LANES lanes:
// chunks [l s, min(k, (l + 1) s)), s = ceil(k / GATHER_LANES)
SRD_GA_HD void gather_lane_chunks(uint64_t k, uint32_t l, uint64_t* j0, uint64_t* j1) {
  const uint64_t s = (k + GATHER_LANES - 1) / GATHER_LANES;
  const uint64_t a = s * l, b = a + s;
  *j0 = a < k ? a : k;
  *j1 = b < k ? b : k;
}
// a lane's term of the hit's raw CRC: its segment's value moved up by the
// bytes that follow the segment (the XOR over the lanes is crc_raw(hit))
template <class R, class P>
SRD_GA_HD uint32_t gather_lane_term(R raw, uint64_t k, uint32_t l, uint64_t len, P pow8) {
  uint64_t j0, j1;
  gather_lane_chunks(k, l, &j0, &j1);
  if (j0 >= j1) return 0;
  const uint64_t seg_end = j1 * GATHER_CHUNK < len ? j1 * GATHER_CHUNK : len;
  return mulp(gather_xpow8(pow8, len - seg_end), gather_fold(raw, j0, j1, len, pow8));
}
// CRC32 from crc_raw: crc32fast's init and xorout 0xFFFFFFFF depend on the
// length alone (srd_crc.h: CRC32(D) = crc_raw(D) ^ CRC32(0^|D|)), the fix the
// batch writer applies
template <class P>
SRD_GA_HD uint32_t gather_final(uint32_t raw, uint64_t len, P pow8) {
  return raw ^ ~mulp(gather_xpow8(pow8, len), 0xFFFFFFFFu);
}
// a hit's CRC32 from its k chunks' raw CRCs, serially
template <class R, class P>
SRD_GA_HD uint32_t gather_combine(R raw, uint64_t k, uint64_t len, P pow8) {
  return gather_final(gather_fold(raw, 0, k, len, pow8), len, pow8);
}

}  // namespace srd
