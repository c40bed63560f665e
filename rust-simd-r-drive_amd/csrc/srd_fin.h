// srd_fin.h -- the finalize rule: how a chain entry's CRC-32 is put together
// from what the scan recorded (candidate record flags, per-tile values) and
// when it cannot be (the slow list).  Plain integer code shared by both passes
// (finalize_in / finalize_core in srd_kernels.hip, chain_finalize_kernel's
// entry pass in srd_glue.hip), the slow path, the batch writer and the host
// (srd_selftest_host, tests/sanitize/fin_check.cpp): outside HIP the
// qualifiers are empty.
//
// Tables: every function takes a `t` with the members it reads, each a pointer
// to or an array of words -- tab (4 x 256, slice-by-4), m16k (4 x 256: v -> v *
// x^16384), winit, zero_crc, invpow, x32768 (a word), and for the grouped
// combine m32k (v -> v * x^32768) and mtk (3 x 4 x 256: v -> v * x^(32768 (j +
// 2))).  FinLds and SlowLds (the LDS copies) are such types as they stand;
// FinTabs is the view over flat tables elsewhere (g_tabs, the host's CrcTables).
//
// Tile values: tv[0], tv[1] = the half-tile partials of lines 0 and 1, tv[2] =
// SX_32 (scan_kernel's tile_sx()); any type with operator[].
#pragma once
#include <stdint.h>

#include "srd_crc.h"

#if defined(__HIPCC__) || defined(__CUDACC__)
#define SRD_FIN_HD __host__ __device__ __forceinline__
#else
#define SRD_FIN_HD inline
#endif
#if defined(__clang__)
#define SRD_UNROLL _Pragma("unroll")
#else
#define SRD_UNROLL
#endif

namespace srd {

constexpr int TILE = 4096;

// flags of a candidate record
constexpr uint32_t F_TOMB = 1u, F_TAIL = 2u, F_SXM = 4u;
constexpr int F_SUF_SHIFT = 3;        // 2 bits: 0 value, 1 next-tile T, 2 next-tile SX1, 3 missing
// the recorded sxm / suf value is a lower-half partial (line < 32): true value =
// v * x^16384 ^ SX_32 of the tile holding m (sxm) or the entry start (suf kind 0) -- see lower_half()
constexpr uint32_t F_SXM_LO = 32u, F_SUF_LO = 64u;
constexpr uint32_t F_NO_PARENT = 3u << F_SUF_SHIFT;  // the parent flags of an entry without a parent record

// whole tiles a finalize thread combines serially (longer entries go to the
// slow list, a wave each).  C3 glue (tools/lib_ab.py, contexts interleaved):
// 4 -> 1.66 ms, 8 -> 1.61, 16 -> 1.57, 32 -> 1.57; C2 (entries of 2 tiles)
// unchanged
#ifndef SRD_LONG_TILES
#define SRD_LONG_TILES 16
#endif
constexpr uint64_t LONG_TILES = SRD_LONG_TILES;

constexpr uint32_t TOMB_CRC = 0xD202EF8Du;  // CRC32(b"\0"): the tombstone byte is 0 by the rule

struct FinTabs {
  const uint32_t *tab, *m16k, *m32k, *mtk, *winit, *zero_crc, *invpow;
  uint32_t x32768;
};
inline FinTabs fin_tabs_host(const CrcTables& c) {
  return {&c.tab[0][0], &c.m16k[0][0], &c.m32k[0][0], &c.mtk[0][0][0], c.winit, c.zero_crc, c.invpow, c.x32768};
}

// v * (the table's fixed multiplier) by four byte-table lookups; m = 4 x 256
// words behind any pointer type (LDS, global, the writer's scalar-load pointer)
template <class P>
SRD_FIN_HD uint32_t mulfix(uint32_t v, P m) {
  return m[v & 0xff] ^ m[256 + ((v >> 8) & 0xff)] ^ m[512 + ((v >> 16) & 0xff)] ^ m[768 + (v >> 24)];
}

SRD_FIN_HD uint64_t prepad64(uint64_t o) { return (64 - (o & 63)) & 63; }
SRD_FIN_HD uint64_t fin_start(uint32_t fl, uint64_t p) { return (fl & F_TOMB) ? p : p + prepad64(p); }
SRD_FIN_HD uint32_t line_of(uint64_t o) { return (uint32_t)((o % TILE) / 64); }

// a lower-half partial v (line < 32) as the true suffix value, sx32 = the tile's SX_32
template <class T>
SRD_FIN_HD uint32_t lower_half(uint32_t v, uint32_t sx32, const T& t) { return mulfix(v, t.m16k) ^ sx32; }
// the suffix value SX_j of line j = 0, 1 or 32 from the tile's values
template <class V, class T>
SRD_FIN_HD uint32_t tile_suffix(const V& tv, uint32_t j, const T& t) {
  return j == 32 ? tv[2] : lower_half(j == 0 ? tv[0] : tv[1], tv[2], t);
}
// ... when line j is one of those three
template <class V, class T>
SRD_FIN_HD bool tile_line(const V& tv, uint32_t j, const T& t, uint32_t* out) {
  if (j == 0) *out = tile_suffix(tv, 0, t);
  else if (j == 1) *out = tile_suffix(tv, 1, t);
  else if (j == 32) *out = tv[2];
  else return false;
  return true;
}

// The pieces of one entry's CRC.  suf = the suffix value of the entry's start
// line (bit 0 of pieces), sxm = that of its metadata line (bit 1), bit 2 = the
// partial last line's CRC is 0 (F_TAIL: m is 64-aligned).  Inputs: the record's
// flags fl and sxm word sxv, its parent record's flags pfl and suf word psuf
// (F_NO_PARENT: no parent record -- the root entry, a root-linked entry, a
// shard's first entry), the values t0 / t1 of the tiles holding start and mo.
// A piece no record holds comes from the per-tile values when its line is 0, 1
// or 32 of the tile (C1/C2/C5: root metadata at 4096, the child's start at
// 4160); else the slow path recomputes it.
struct FinPieces {
  uint32_t suf, sxm, pieces;
};
template <class V, class T>
SRD_FIN_HD FinPieces fin_pieces(uint32_t fl, uint32_t sxv, uint32_t pfl, uint32_t psuf, const V& t0, const V& t1,
                                uint64_t start, uint64_t mo, const T& t) {
  FinPieces r = {0, 0, 0};
  if (fl & F_SXM) {
    r.sxm = (fl & F_SXM_LO) ? lower_half(sxv, t1[2], t) : sxv;
    r.pieces |= 2;
  } else if (tile_line(t1, line_of(mo), t, &r.sxm)) {
    r.pieces |= 2;
  }
  if (fl & F_TAIL) r.pieces |= 4;
  const uint32_t kind = (pfl >> F_SUF_SHIFT) & 3;
  if (kind == 0) {  // the parent recorded it (its own tile: t0)
    r.suf = (pfl & F_SUF_LO) ? lower_half(psuf, t0[2], t) : psuf;
    r.pieces |= 1;
  } else if (kind == 1) {  // line 0 of the next tile
    r.suf = tile_suffix(t0, 0, t);
    r.pieces |= 1;
  } else if (kind == 2) {  // line 1
    r.suf = tile_suffix(t0, 1, t);
    r.pieces |= 1;
  } else if (tile_line(t0, line_of(start), t, &r.suf)) {
    r.pieces |= 1;
  }
  return r;
}

// what computes a live entry's CRC: the thread itself (FIN_SHORT: len < 64, the
// tail alone; FIN_INLINE: crc_from_pieces) or a wave of the slow path
// (FIN_SLOW: a piece is missing, or more than LONG_TILES whole tiles lie
// between the start tile k0 and the metadata tile k1)
enum FinRoute { FIN_SHORT, FIN_INLINE, FIN_SLOW };
SRD_FIN_HD FinRoute fin_route(uint64_t len, uint64_t k0, uint64_t k1, uint32_t pieces) {
  if (len < 64) return FIN_SHORT;
  return (pieces & 3) == 3 && k1 <= k0 + 1 + LONG_TILES ? FIN_INLINE : FIN_SLOW;
}

// CRC32 of bytes [s, m) from the pieces and the per-tile values t4[k] (tail =
// crc_raw of the partial last line), the whole tiles one Horner step each
template <class V, class T>
SRD_FIN_HD uint32_t crc_from_pieces(uint64_t s, uint64_t m, uint32_t suf, uint32_t sxm, uint32_t tail, const V* t4,
                                    const T& t) {
  const uint64_t len = m - s;
  if (len < 64) return tail ^ t.zero_crc[len];
  const uint64_t k0 = s / TILE, k1 = m / TILE;
  uint32_t acc = suf ^ t.winit[line_of(s)];
  uint32_t y;
  if (k0 == k1) {
    y = acc ^ sxm;
  } else {
    for (uint64_t k = k0 + 1; k < k1; k++) acc = mulp(t.x32768, acc) ^ tile_suffix(t4[k], 0, t);
    y = mulp(t.x32768, acc) ^ tile_suffix(t4[k1], 0, t) ^ sxm;
  }
  return ~(mulp(t.invpow[(k1 + 1) * TILE - m], y) ^ tail);
}

// The same with the whole tiles 4 at a time (their values loaded together): acc
// = acc * X^r ^ sx_0 X^(r-1) ^ ... ^ sx_(r-1) for the group's r <= 4 tiles (X =
// x^32768, sx = the tile's line-0 suffix), so the dependent chain is one table
// multiply per 4 tiles, not per tile (the same 32 lookups per 4 tiles; C3's
// 2-16-tile entries).  t1 = t4[k1], already loaded.
template <class V, class T>
SRD_FIN_HD uint32_t crc_from_pieces4(uint64_t s, uint64_t m, uint32_t suf, uint32_t sxm, uint32_t tail, const V* t4,
                                     const V& t1, const T& t) {
  const uint64_t len = m - s;
  if (len < 64) return tail ^ t.zero_crc[len];
  const uint64_t k0 = s / TILE, k1 = m / TILE;
  uint32_t acc = suf ^ t.winit[line_of(s)];
  uint32_t y;
  if (k0 == k1) {
    y = acc ^ sxm;
  } else {
    for (uint64_t kb = k0 + 1; kb < k1; kb += 4) {
      V tv[4];
      SRD_UNROLL
      for (int q = 0; q < 4; q++) tv[q] = t4[kb + q < k1 ? kb + q : k1];
      const uint32_t r = (uint32_t)(k1 - kb < 4 ? k1 - kb : 4);
      uint32_t sx[4];  // the tiles' line-0 suffix values
      SRD_UNROLL
      for (int q = 0; q < 4; q++) sx[q] = tile_suffix(tv[q], 0, t);
      // X^j tables: j = 1 m32k, j = 2..4 mtk[j - 2]
      uint32_t v = mulfix(acc, r == 1 ? t.m32k : t.mtk + 1024 * (r - 2)) ^ sx[r - 1];
      if (r >= 2) v ^= mulfix(sx[r - 2], t.m32k);
      if (r >= 3) v ^= mulfix(sx[r - 3], t.mtk);
      if (r >= 4) v ^= mulfix(sx[0], t.mtk + 1024);
      acc = v;
    }
    y = mulfix(acc, t.m32k) ^ tile_suffix(t1, 0, t) ^ sxm;
  }
  return ~(mulp(t.invpow[(k1 + 1) * TILE - m], y) ^ tail);
}

// crc_raw of bytes [floor64(m), m) (<= 63 bytes) in one round trip: the
// 64-byte line at floor64(m) by four independent 16-byte loads (the store is
// readable to srd_padded_size, so the whole line is), then <= 15 slice-by-4
// word steps and <= 3 byte steps from registers.  (A word load per step made
// every step wait for its own HBM round trip: up to 18 dependent loads per
// entry, which set C3's finalize pass time.)  V = a 16-byte vector of 4 words.
template <class V, class T>
SRD_FIN_HD uint32_t tail_crc_line(const uint8_t* file, uint64_t m, const T& t) {
  const uint64_t L = m & ~63ull;
  const uint32_t r = (uint32_t)(m - L);
  if (r == 0) return 0;
  const V* lp = (const V*)(file + L);
  const V q0 = lp[0], q1 = lp[1], q2 = lp[2], q3 = lp[3];
  const uint32_t w[16] = {q0[0], q0[1], q0[2], q0[3], q1[0], q1[1], q1[2], q1[3],
                          q2[0], q2[1], q2[2], q2[3], q3[0], q3[1], q3[2], q3[3]};
  uint32_t s = 0;
  SRD_UNROLL
  for (int i = 0; i < 15; i++) {
    if (4u * i + 4u <= r) {
      s ^= w[i];
      s = t.tab[768 + (s & 0xff)] ^ t.tab[512 + ((s >> 8) & 0xff)] ^ t.tab[256 + ((s >> 16) & 0xff)] ^ t.tab[s >> 24];
    }
  }
  uint32_t pw = 0;  // the partial word w[r / 4] (selects: no indexed register access)
  SRD_UNROLL
  for (int i = 0; i < 16; i++) pw = (uint32_t)i == (r >> 2) ? w[i] : pw;
  for (uint32_t b = 0; b < (r & 3u); b++) s = t.tab[(s ^ (pw >> (8 * b))) & 0xff] ^ (s >> 8);
  return s;
}

}  // namespace srd
