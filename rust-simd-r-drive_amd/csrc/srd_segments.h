// srd_segments.h -- the arithmetic of srd_batch_append_segments_device, and
// the one entry model of everything that streams payload bytes: how a segment
// table is judged, how an entry's segments are cut into work units, what a
// unit's descriptor holds (SegUnit), what describes a batch of entries cut into
// units (UnitArgs, read through a view: a segment table, or ranges, each its
// own entry of one segment -- the gather's hits, the append's and the live
// compaction's payloads -- or, for the scatter read, ranges delivered into a
// segment table of destinations), and how an entry's CRC-32 is put together
// from its units' raw CRCs.  Plain integer code shared by the layout kernels
// (srd_segments.hip, srd_scatter.hip), the unit / terms / combine kernels
// (srd_units.hip), the streaming kernel (srd_stream.hip), the host glue
// (srd_ops.hip) and CPU checks (tests/sanitize_segments/segments_check.cpp,
// tests/sanitize_scatter/scatter_check.cpp): outside HIP the
// qualifiers are empty.  The entry layout (slots, base, the new tail, the error
// word) is the append's (srd_append.h) as it is.
//
// Entry i's payload is the concatenation of segments first[i] .. first[i + 1);
// segment s of it starts at offset seg_off[s] inside the entry, i.e. at file
// offset D = P_i + seg_off[s], and P_i is a multiple of 64: D mod 16 =
// seg_off[s] mod 16 is known before the layout's exclusive sum.
//
// The cut: with A = D mod 16, the A bytes below D down to the 16-byte boundary
// and the segment's L bytes form a virtual stream of A + L bytes that is cut
// every SRD_GATHER_CHUNK bytes.  Unit k holds the segment's bytes
//   [k C - A, min(L, (k + 1) C - A))       (unit 0 from byte 0)
// so a segment has ceil((A + L) / C) units (none for L == 0), each of at most
// C bytes, unit 0 carries the head of fewer than 16 bytes that brings the
// destination to a 16-byte boundary, and every later unit starts at one.  A
// segment that starts 16-aligned in the store (A == 0) is cut exactly like a
// payload of the append.
#pragma once
#include <stdint.h>

#include "srd_append.h"

namespace srd {

// what an entry's part of the tables decides (on top of APPEND_OK / _EMPTY / _TOO_LONG)
constexpr uint32_t SEG_BAD_SEGMENT = 5;  // src >= n_src, reserved != 0, or a range not inside its source
constexpr uint32_t SEG_BAD_FIRST = 6;    // d_seg_first: first[0] != 0, a decreasing pair, first[n] != n_segs

// d_seg_first around entry i (f0 = first[i], f1 = first[i + 1]): true when the
// entry's segments [f0, f1) may be looked at
SRD_GA_HD bool seg_first_ok(uint64_t f0, uint64_t f1, uint64_t i, uint64_t n, uint64_t n_segs) {
  if (i == 0 && f0 != 0) return false;
  if (i == n - 1 && f1 != n_segs) return false;
  return f0 <= f1 && f1 <= n_segs;
}

// one segment against the source table, by arithmetic that cannot wrap
// (append_range_status' rule; a zero length is no fault here)
template <class LenP>
SRD_GA_HD bool seg_ok(const srd_segment& g, LenP src_lens, uint64_t n_src) {
  if (g.src >= n_src || g.reserved != 0) return false;
  const uint64_t sl = src_lens[g.src];
  return g.off <= sl && g.len <= sl - g.off;
}

SRD_GA_HD uint64_t seg_unit_count(uint64_t a, uint64_t len) {  // a = D mod 16
  return len ? (a + len + GATHER_CHUNK - 1) / GATHER_CHUNK : 0;
}
// unit k of the segment: its bytes [*b0, *b1) of the segment (k < seg_unit_count)
SRD_GA_HD void seg_unit_range(uint64_t a, uint64_t len, uint64_t k, uint64_t* b0, uint64_t* b1) {
  const uint64_t e = (k + 1) * GATHER_CHUNK - a;
  *b0 = k ? k * GATHER_CHUNK - a : 0;
  *b1 = e < len ? e : len;
}

// An entry's segments [s0, s1) (seg_first_ok): its status, its length and its
// unit count; seg_off[s] / seg_units[s] for each of them (meaningful for an
// accepted entry).  A malformed segment decides whatever the total length; a
// malformed segment is never used for anything else.
struct SegEntry {
  uint32_t status;
  uint64_t len, units;
};
template <class SegP, class LenP, class OffP, class UnP>
SRD_GA_HD SegEntry seg_entry_layout(SegP segs, uint64_t s0, uint64_t s1, LenP src_lens, uint64_t n_src, OffP seg_off,
                                    UnP seg_units) {
  SegEntry e{APPEND_OK, 0, 0};
  bool bad = false, too_long = false;
  for (uint64_t s = s0; s < s1; s++) {
    const srd_segment g = segs[s];
    uint64_t k = 0;
    if (!seg_ok(g, src_lens, n_src)) bad = true;
    else if (too_long || g.len >= APPEND_TAIL_LIMIT || e.len + g.len >= APPEND_TAIL_LIMIT) too_long = true;
    else {
      k = seg_unit_count(e.len & 15, g.len);
      seg_off[s] = e.len;
      e.len += g.len;
      e.units += k;
    }
    seg_units[s] = k;
  }
  e.status = bad ? SEG_BAD_SEGMENT : too_long ? APPEND_TOO_LONG : e.len == 0 ? APPEND_EMPTY : APPEND_OK;
  return e;
}

// A work unit: a piece of one segment.
struct SegUnit {
  uint64_t src;  // address of its first source byte
  uint64_t dst;  // offset of its first byte from the streaming kernel's out (the appends: its file offset in the store)
  uint64_t end;  // offset of its end inside its entry (the combine's weight; a single unit: the entry's length)
  uint32_t ent;  // its entry
  uint32_t lf;   // seg_unit_lf
};
static_assert(sizeof(SegUnit) == 32, "read as eight scalar words");
// lf: bits 0-16 the length (1 .. C), bits 20-24 / 25-29 how many bytes of the
// SEGMENT lie below the unit's first / behind its last byte (capped at 16: all
// an aligned 16-byte load can reach), bit 30: the unit owns the zero bytes from
// its end up to the next 64-byte boundary of the output (SEG_LF_PAD), bit 31:
// the entry's only unit
static_assert(GATHER_CHUNK <= (1u << 16), "a unit's length takes 17 bits of SegUnit::lf");
constexpr uint32_t SEG_LF_PAD = 1u << 30;
SRD_GA_HD uint32_t seg_unit_lf(uint64_t len, uint64_t below, uint64_t behind, bool single) {
  return (uint32_t)len | (uint32_t)(below < 16 ? below : 16) << 20 | (uint32_t)(behind < 16 ? behind : 16) << 25 |
         (single ? 1u << 31 : 0u);
}
SRD_GA_HD uint32_t seg_lf_len(uint32_t lf) { return lf & 0x1FFFFu; }
SRD_GA_HD uint32_t seg_lf_below(uint32_t lf) { return (lf >> 20) & 31u; }
SRD_GA_HD uint32_t seg_lf_behind(uint32_t lf) { return (lf >> 25) & 31u; }
SRD_GA_HD bool seg_lf_single(uint32_t lf) { return lf >> 31; }

// unit k of a segment of len bytes at src_addr whose first byte lies at file
// offset dst and at offset off inside an entry of ent_units units
SRD_GA_HD SegUnit seg_unit(uint64_t src_addr, uint64_t dst, uint64_t off, uint64_t len, uint64_t k, uint32_t ent,
                           uint64_t ent_units) {
  uint64_t b0, b1;
  seg_unit_range(dst & 15, len, k, &b0, &b1);
  return SegUnit{src_addr + b0, dst + b0, off + b1, ent, seg_unit_lf(b1 - b0, b0, len - b1, ent_units == 1)};
}
// how many zero bytes a unit owns behind its end (output offsets of hits are multiples of 64)
SRD_GA_HD uint32_t seg_unit_pad(uint64_t dst, uint32_t lf) {
  return lf & SEG_LF_PAD ? (uint32_t)(0 - (dst + seg_lf_len(lf))) & 63u : 0u;
}

// The streaming kernel's frame of a unit, aligned to the DESTINATION: with a =
// dst mod 16 the frame starts a bytes below the unit's first byte, at a 16-byte
// boundary of the store, and the unit's bytes are [a, vlen) of it.  r = (source
// address - destination address) mod 16 (the store's base is 16-byte aligned).
// Piece o (a multiple of 16) is the frame's bytes [o, o + 16): one aligned
// vector of the store, and in the source, for r == 0, the aligned vector [o, o
// + 16), for r != 0 the bytes r .. r + 15 of the aligned pair [o - r, o - r +
// 32).  The segment is [a - below, vlen + behind) of the frame.
struct SegFrame {
  uint32_t a, vlen, r;
  uint32_t lo, hi;  // r != 0: the first piece whose pair starts inside the segment; pairs must end by hi - r
};
SRD_GA_HD SegFrame seg_frame(uint64_t src, uint64_t dst, uint32_t lf) {
  SegFrame f;
  f.a = (uint32_t)dst & 15u;
  f.vlen = f.a + seg_lf_len(lf);
  f.r = (uint32_t)(src - dst) & 15u;
  f.lo = f.a + f.r > seg_lf_below(lf) ? f.a + f.r - seg_lf_below(lf) : 0u;
  f.hi = f.vlen + seg_lf_behind(lf) + f.r;
  return f;
}
// piece o holds 16 bytes of the unit and every aligned source vector it takes
// lies inside the segment: it moves as vectors; any other piece byte by byte
SRD_GA_HD bool seg_piece_vec(const SegFrame& f, uint32_t o) {
  const bool whole = o >= f.a && o + 16 <= f.vlen;
  return f.r ? whole && o >= f.lo && o + 32 <= f.hi : whole;
}

// A unit's term of its entry's raw CRC: the unit's raw CRC moved up by the
// entry's bytes behind the unit; the XOR over the entry's units is
// crc_raw(entry), and gather_final makes it the CRC-32.
template <class P>
SRD_GA_HD uint32_t seg_unit_term(uint32_t raw, uint64_t ent_len, uint64_t end, P pow8) {
  return mulp(gather_xpow8(pow8, ent_len - end), raw);
}

// A batch of entries cut into units: what the unit table and the combine need
// of it, whoever laid it out.  An entry is a run of segments; a view (below)
// says where a segment's values are.
struct UnitArgs {
  uint64_t n;       // entries
  uint64_t n_segs;  // segments (ranges: n)
  uint64_t* eun;    // [n] an entry's unit count
  uint64_t* off;    // [n] where its bytes go, less dst0: a multiple of 64
  uint64_t* upre;   // [n_segs] exclusive sum of the segments' unit counts
  // ranges: segment s is entry s, the bytes [start[s], end[s]) of file
  const uint8_t* file;
  const uint64_t *start, *end;
  // a table: entry i is the segments first[i] .. first[i + 1)
  const uint64_t* srcs;  // [2 n_src] the source table on the device: address, length (the scatter: of destinations)
  const srd_segment* segs;
  const uint64_t* first;  // [n + 1]
  uint64_t* len;          // [n] the entries' lengths
  uint64_t* soff;         // [n_segs] a segment's offset inside its entry
  uint64_t* sun;          // [n_segs] its unit count (upre's addends)
  uint32_t* sent;         // [n_segs] its entry
  uint64_t dst0;   // a multiple of 64 (the scatter: the address that out stands for, a multiple of 16)
  bool pad;        // an entry's last unit zeroes up to the next 64-byte boundary of the output
  SegUnit* unit;   // [n_units] the unit table
  uint64_t n_units;
  uint32_t* raw;   // [n_units] a multi-unit entry's units: crc_raw, then the unit's term
  uint32_t* crc;   // [n] an entry's CRC32
  // the unit kernels' device-count forms (srd_read_rows_device): the unit count
  // and the count of multi-unit entries are words in device memory, n_units
  // above only bounds the grids
  const uint64_t* d_n_units;
  const unsigned long long* d_n_multi;
};
// (nothing is materialised for ranges: their unit count is eun[s], their unit
// prefix upre[s], and the entry's first unit upre[i]); dst is where a
// segment's first byte goes, as an offset from the streaming kernel's out
struct RangeView {
  static SRD_GA_HD uint64_t addr(const UnitArgs& a, uint64_t s) { return (uint64_t)(uintptr_t)a.file + a.start[s]; }
  static SRD_GA_HD uint64_t len(const UnitArgs& a, uint64_t s) { return a.end[s] - a.start[s]; }
  static SRD_GA_HD uint64_t soff(const UnitArgs&, uint64_t) { return 0; }
  static SRD_GA_HD uint64_t ent(const UnitArgs&, uint64_t s) { return s; }
  static SRD_GA_HD uint64_t first(const UnitArgs&, uint64_t i) { return i; }
  static SRD_GA_HD uint64_t ent_len(const UnitArgs& a, uint64_t i) { return a.end[i] - a.start[i]; }
  static SRD_GA_HD uint64_t dst(const UnitArgs& a, uint64_t s) { return a.dst0 + a.off[s]; }
};
struct TableView {
  static SRD_GA_HD uint64_t addr(const UnitArgs& a, uint64_t s) { return a.srcs[2 * a.segs[s].src] + a.segs[s].off; }
  static SRD_GA_HD uint64_t len(const UnitArgs& a, uint64_t s) { return a.segs[s].len; }
  static SRD_GA_HD uint64_t soff(const UnitArgs& a, uint64_t s) { return a.soff[s]; }
  static SRD_GA_HD uint64_t ent(const UnitArgs& a, uint64_t s) { return a.sent[s]; }
  static SRD_GA_HD uint64_t first(const UnitArgs& a, uint64_t i) { return a.first[i]; }
  static SRD_GA_HD uint64_t ent_len(const UnitArgs& a, uint64_t i) { return a.len[i]; }
  static SRD_GA_HD uint64_t dst(const UnitArgs& a, uint64_t s) { return a.dst0 + a.off[a.sent[s]] + a.soff[s]; }
};
// The scatter read (srd_scatter.h): entry i is the range [start[i], end[i]) of
// file, delivered in order into the segments first[i] .. first[i + 1) of a
// table of DESTINATIONS -- segment s takes the entry's bytes from soff[s] on
// and puts them at its table address + off, an offset from dst0, the 16-byte
// boundary at or below the lowest table address.  A unit's below / behind
// counts are the segment's, so its loads stay inside the payload.
struct ScatterView {
  static SRD_GA_HD uint64_t addr(const UnitArgs& a, uint64_t s) {
    return (uint64_t)(uintptr_t)a.file + a.start[a.sent[s]] + a.soff[s];
  }
  static SRD_GA_HD uint64_t len(const UnitArgs& a, uint64_t s) { return a.segs[s].len; }
  static SRD_GA_HD uint64_t soff(const UnitArgs& a, uint64_t s) { return a.soff[s]; }
  static SRD_GA_HD uint64_t ent(const UnitArgs& a, uint64_t s) { return a.sent[s]; }
  static SRD_GA_HD uint64_t first(const UnitArgs& a, uint64_t i) { return a.first[i]; }
  static SRD_GA_HD uint64_t ent_len(const UnitArgs& a, uint64_t i) { return a.end[i] - a.start[i]; }
  static SRD_GA_HD uint64_t dst(const UnitArgs& a, uint64_t s) { return a.srcs[2 * a.segs[s].src] + a.segs[s].off - a.dst0; }
};
// an entry's first unit (an entry with units has a segment)
template <class View>
SRD_GA_HD uint64_t unit_first(const UnitArgs& a, uint64_t i) {
  return a.upre[View::first(a, i)];
}
// unit u (u < n_units): piece u - upre[s] of the segment s with upre[s] <= u <
// upre[s + 1]; of a range, that is chunk u - upre[i] of range i (srd_gather.h:
// the destination is 64-aligned, so the cut is the chunk cut, the below /
// behind counts are taken against the range itself, and end is the chunk's end
// inside it).  The destination is the view's: the appends' and the gather's at
// dst0 + off[ent] + soff, the scatter's wherever its segment points.
template <class View>
SRD_GA_HD SegUnit unit_of(const UnitArgs& a, uint64_t u) {
  const uint64_t s = gather_unit_hit(a.upre, a.n_segs, u), off = View::soff(a, s), ent = View::ent(a, s), k = a.eun[ent];
  SegUnit x = seg_unit(View::addr(a, s), View::dst(a, s), off, View::len(a, s), u - a.upre[s], (uint32_t)ent, k);
  if (a.pad && u + 1 == unit_first<View>(a, ent) + k) x.lf |= SEG_LF_PAD;
  return x;
}

}  // namespace srd
