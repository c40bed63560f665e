// srd_part.h -- the scan's partition arithmetic (ScanPart): which resident spans
// each scan block and each of its waves takes, and the inverse the link step
// needs.  Plain integer code shared by the kernels (srd_kernels.hip), the host
// (srd_scan_host.hip, srd_ctx.hip) and a stand-alone CPU check
// (tests/sanitize/part_check.cpp): outside HIP the qualifiers are empty.
#pragma once
#include <stdint.h>

#if defined(__HIPCC__) || defined(__CUDACC__)
#define SRD_PART_HD __host__ __device__ __forceinline__
#else
#define SRD_PART_HD inline
#endif

namespace srd {

// The scan's wave partition (both passes; link_record inverts it).  Block b of g
// takes the resident spans [st(b), st(b+1)), st(b) = b*ns/g; inside a block
// wave v takes the share [cw(v), cw(v+1)) (units of 1/65536) of the block's
// spans.  Waves of one SIMD do not progress equally: the SIMD issues for
// its oldest waves first, so with an even split waves 0-3 (the oldest on
// each SIMD) finished ~15% before waves 12-15 (tools/wave_stamps.py); the
// per-slot shares wq[v] (scan_weights: fitted to the wave stamps) even out
// the finish times.  The optimistic pass replaces st(b) by a device table
// (XPart, XCD-aware block shares) once a context has scanned a store of the
// same span count and grid.
struct ScanPart {
  uint64_t s_lo;   // first resident span
  uint64_t ns;     // resident spans
  uint32_t g;      // scan blocks
  uint32_t nw;     // waves per scan block (<= 16; the launch's variant sets it, scan_geom)
  uint32_t wq[16];  // share of wave slot v of each block; wq[0] + .. + wq[nw-1] == 65536
  uint32_t cw[17];  // cumulative: cw[v] = wq[0] + .. + wq[v-1] (part_fill_cw)
  const uint64_t* bs;  // device: st(0..g) (XPart::bs of this call), nullptr: st(b) = b*ns/g
};

// The domain of a block-start table st(0..g) over ns resident spans (what
// xpart_update writes and srd_ctx_set_scan_blocks accepts): 1 <= g <=
// XP_MAX_BLOCKS, st(0) = 0, st(g) = ns, non-decreasing (empty blocks anywhere
// are fine: part_span_wave skips them, their waves take empty ranges), and no
// block above part_table_block_bound -- the size part_max_wave_spans assumes
// when the host sizes each wave's record region.
constexpr uint32_t XP_MAX_BLOCKS = 1024;
SRD_PART_HD uint64_t part_table_block_bound(uint64_t ns, uint64_t g) { return (ns * 5 + 4 * g - 1) / (4 * g) + 1; }
SRD_PART_HD bool part_table_ok(const uint64_t* st, uint64_t g, uint64_t ns) {
  if (!st || g < 1 || g > XP_MAX_BLOCKS || st[0] != 0 || st[g] != ns) return false;
  const uint64_t bound = part_table_block_bound(ns, g);
  for (uint64_t b = 0; b < g; b++)
    if (st[b + 1] < st[b] || st[b + 1] - st[b] > bound) return false;
  return true;
}

SRD_PART_HD void part_fill_cw(ScanPart& p) {
  p.cw[0] = 0;
  for (uint32_t v = 0; v < 16; v++) p.cw[v + 1] = p.cw[v] + (v < p.nw ? p.wq[v] : 0u);
}
// cumulative share of the waves below v (v <= 16)
SRD_PART_HD uint64_t part_cw(const ScanPart& p, uint32_t v) { return p.cw[v]; }
SRD_PART_HD uint64_t part_block_start(const ScanPart& p, uint64_t b) {
  if (p.bs) return p.bs[b];  // (device pointer: host code sizes with the even split, bs unset)
  return b * p.ns / p.g;
}
// wave v of block b: resident-relative spans [*r0, *r1)
SRD_PART_HD void part_wave_range(const ScanPart& p, uint64_t b, uint32_t v, uint64_t* r0, uint64_t* r1) {
  const uint64_t bs = part_block_start(p, b), nb = part_block_start(p, b + 1) - bs;
  *r0 = bs + ((nb * part_cw(p, v)) >> 16);
  *r1 = bs + ((nb * part_cw(p, v + 1)) >> 16);
}
// the scan wave (b * nw + v) holding resident-relative span rel < ns
SRD_PART_HD uint64_t part_span_wave(const ScanPart& p, uint64_t rel) {
  uint64_t b;
  if (p.bs) {  // the last block whose start is <= rel (empty blocks are skipped over)
    uint64_t lo = 0, hi = p.g - 1;
    while (lo < hi) {
      const uint64_t mid = (lo + hi + 1) >> 1;
      if (p.bs[mid] <= rel) lo = mid; else hi = mid - 1;
    }
    b = lo;
  } else {
    b = rel * p.g / p.ns;
    while (b + 1 < p.g && part_block_start(p, b + 1) <= rel) b++;
  }
  const uint64_t bs = part_block_start(p, b), nb = part_block_start(p, b + 1) - bs, o = rel - bs;
  uint32_t v = 0;
#pragma unroll
  for (uint32_t j = 1; j < 16; j++) v += j < p.nw && o >= ((nb * part_cw(p, j)) >> 16) ? 1u : 0u;
  return b * p.nw + v;
}
// an upper bound on the spans of one wave; xpart: with XCD-aware block
// shares, a block holds at most (1 + XP_CLAMP) / (1 - XP_CLAMP) < 1.25 of
// the even share + 1 span (xpart_update, part_table_block_bound)
SRD_PART_HD uint64_t part_max_wave_spans(const ScanPart& p, bool xpart = false) {
  if (!p.g) return 1;
  uint32_t wmax = 0;
  for (uint32_t v = 0; v < p.nw; v++) wmax = p.wq[v] > wmax ? p.wq[v] : wmax;
  const uint64_t nb = xpart ? part_table_block_bound(p.ns, p.g) : (p.ns + p.g - 1) / p.g;
  return (nb * wmax + 65535) / 65536 + 1;
}

}  // namespace srd
