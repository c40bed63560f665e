// srd_scatter.h -- the arithmetic of srd_payload_scatter_device: how a query's
// segments are judged against the destination table, where each of them takes
// its bytes inside the payload, how many work units it is cut into, and whether
// the segments' lengths add up to the payload's.  Plain integer code shared by
// the layout kernel (srd_scatter.hip), the host glue (srd_ops.hip) and a CPU
// check (tests/sanitize_scatter/scatter_check.cpp): outside HIP the qualifiers
// are empty.  The range rule is the gather's (srd_gather.h), the table rule,
// the unit cut, the unit descriptor and the view the units are read through
// (ScatterView) are srd_segments.h's.
//
// The counterpart of seg_entry_layout with the roles swapped: a segment names
// DESTINATION bytes, table[src].address + off, and the unit cut is aligned to
// the destination -- here an address, known only with the table, where the
// segment append's is the segment's offset inside its entry.  A segment's
// source is the payload from soff[s] on, the sum of the lengths before it.
#pragma once
#include <stdint.h>

#include "srd_segments.h"

namespace srd {

constexpr uint32_t SCATTER_BAD_LENGTH = SRD_SCATTER_BAD_LENGTH;
// A segment's unit count as the prefix sum sees it: capped, so that the sum
// over fewer than 2^31 segments cannot wrap, and a capped count alone takes the
// total to the 2^32 units at which the call is refused
constexpr uint64_t SCATTER_UNITS_CAP = 1ull << 32;

// the interleaved destination table [2 n_dst]: address, length
struct ScatterTable {
  const uint64_t* t;
  SRD_GA_HD uint64_t addr(uint64_t k) const { return t[2 * k]; }
  SRD_GA_HD uint64_t operator[](uint64_t k) const { return t[2 * k + 1]; }  // (seg_ok's lengths)
};

// Query i's segments [s0, s1) (seg_first_ok) against its range's status (the
// gather's: NONE, BAD_RANGE, or OK for a hit of want = end - start bytes).
//   bad     a malformed segment (seg_ok): it refuses the call whatever the
//           status, and is never used for anything else;
//   status  the range's, or for a hit whose segments' lengths do not sum to
//           want -- judged without a sum that could wrap -- SCATTER_BAD_LENGTH;
//   units   the query's work units: none unless status is OK.
// sent[s] = i for every segment; soff[s] and sun[s] (the capped unit count) are
// meaningful for status OK, and sun[s] = 0 for every segment otherwise.
struct ScatterEntry {
  uint32_t status;
  bool bad;
  uint64_t units;
};
template <class SegP, class OffP, class UnP, class EntP>
SRD_GA_HD ScatterEntry scatter_entry_layout(SegP segs, uint64_t s0, uint64_t s1, ScatterTable tab, uint64_t n_dst,
                                            uint32_t range_status, uint64_t want, uint32_t i, OffP soff, UnP sun,
                                            EntP sent) {
  ScatterEntry e{range_status, false, 0};
  const bool hit = range_status == SRD_GATHER_OK;
  uint64_t sum = 0;
  bool over = false;
  for (uint64_t s = s0; s < s1; s++) {
    const srd_segment g = segs[s];
    uint64_t k = 0;
    if (!seg_ok(g, tab, n_dst)) e.bad = true;
    else if (!hit || over || g.len > want - sum) over = true;  // (sum <= want)
    else {
      // (a length from the cap's on has that many units at least, and seg_unit_count's sum could wrap)
      k = g.len >= SCATTER_UNITS_CAP * GATHER_CHUNK ? SCATTER_UNITS_CAP : seg_unit_count((tab.addr(g.src) + g.off) & 15, g.len);
      soff[s] = sum;
      sum += g.len;
      e.units += k;
    }
    sun[s] = k;
    sent[s] = i;
  }
  if (hit && (over || sum != want)) e.status = SCATTER_BAD_LENGTH;
  if (e.status != SRD_GATHER_OK || e.bad) {
    e.units = 0;
    for (uint64_t s = s0; s < s1; s++) sun[s] = 0;
  }
  return e;
}

}  // namespace srd
