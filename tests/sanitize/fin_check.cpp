// ASan/UBSan check of the finalize rule (TEST INFRASTRUCTURE):
// rust-simd-r-drive_amd/csrc/srd_fin.h compiled for the host, the very code
// finalize_core, finalize_in and the slow path run, against a CRC-32 computed
// byte by byte (its own table) over a pseudo-random buffer of 26 tiles:
//   - sweep: every start-line class (0, 1, 32, other) x metadata-line class x
//     0..22 whole tiles between them (and the same-tile case): the serial and
//     the grouped crc_from_pieces equal the byte-wise CRC, tail_crc_line the
//     byte-wise tail, tile_suffix the byte-wise suffix of lines 0, 1 and 32;
//   - short entries: len 0, 1, 63, 64, 65;
//   - every fin_pieces branch (parent kinds 0 with and without F_SUF_LO, 1, 2,
//     no parent record; F_SXM with and without F_SXM_LO, none; F_TAIL; the
//     tombstone): a piece whose bit is set equals the suffix recomputed from
//     the bytes, the bit is set exactly when the piece is known, and fin_route
//     sends to the slow list exactly the entries of >= 64 bytes with a missing
//     piece or more than LONG_TILES whole tiles.
// Exit status 0 = no sanitizer report and every check held.
#include <stdint.h>
#include <stdio.h>

#include <initializer_list>

#include "check.h"
#include "srd_crc.h"
#include "srd_fin.h"

using namespace srd;

static uint64_t g_cases = 0;

constexpr uint64_t NT = 26;  // tiles
alignas(64) static uint8_t buf[NT * TILE];
struct Tile {  // one tile's values, as the scan stores them (16 bytes)
  uint32_t v[4];
  uint32_t operator[](int i) const { return v[i]; }
};
static Tile tiles[NT];
static uint32_t btab[256];  // the byte-wise reference's own table

// crc_raw / CRC32 of bytes [a, b), byte by byte
static uint32_t raw(uint64_t a, uint64_t b, uint32_t s = 0) {
  for (uint64_t i = a; i < b; i++) s = btab[(s ^ buf[i]) & 0xff] ^ (s >> 8);
  return s;
}
static uint32_t crc32(uint64_t a, uint64_t b) { return ~raw(a, b, ~0u); }
// crc_raw(o's line .. the end of its tile): the suffix value of o's line
static uint32_t suffix_at(uint64_t o) { return raw(o & ~63ull, (o | (TILE - 1)) + 1); }
// the lower-half partial of o's line (line < 32): crc_raw(o's line .. line 31)
static uint32_t partial_at(uint64_t o) { return raw(o & ~63ull, (o & ~(uint64_t)(TILE - 1)) + TILE / 2); }

static CrcTables ct;
static FinTabs ft;

// both combines and the tail against the bytes
static void check_crc(uint64_t s, uint64_t m) {
  g_cases++;
  const uint32_t want = crc32(s, m), tail = tail_crc_line<Tile>(buf, m, ft);
  EXPECT(tail == raw(m & ~63ull, m));
  const uint32_t a = crc_from_pieces(s, m, suffix_at(s), suffix_at(m), tail, tiles, ft);
  const uint32_t b = crc_from_pieces4(s, m, suffix_at(s), suffix_at(m), tail, tiles, tiles[m / TILE], ft);
  EXPECT(a == want);
  EXPECT(b == want);
}

// one entry through fin_pieces / fin_route / the combine.  start = the entry's
// start, mo its metadata offset; know_suf / know_sxm: the rule must resolve the piece
static void check_entry(uint32_t fl, uint32_t sxv, uint32_t pfl, uint32_t psuf, uint64_t start, uint64_t mo,
                        bool know_suf, bool know_sxm) {
  g_cases++;
  const uint64_t k0 = start / TILE, k1 = mo / TILE, len = mo - start;
  const FinPieces pc = fin_pieces(fl, sxv, pfl, psuf, tiles[k0], tiles[k1], start, mo, ft);
  EXPECT(((pc.pieces & 1) != 0) == know_suf);
  EXPECT(((pc.pieces & 2) != 0) == know_sxm);
  EXPECT(((pc.pieces & 4) != 0) == ((fl & F_TAIL) != 0));
  if (pc.pieces & 1) EXPECT(pc.suf == suffix_at(start));
  if (pc.pieces & 2) EXPECT(pc.sxm == suffix_at(mo));
  const FinRoute rt = fin_route(len, k0, k1, pc.pieces);
  const bool slow = len >= 64 && (!know_suf || !know_sxm || k1 - k0 - (k1 > k0) > LONG_TILES);
  EXPECT((rt == FIN_SLOW) == slow);
  EXPECT((rt == FIN_SHORT) == (len < 64));
  if (rt == FIN_SLOW) return;
  const uint32_t tail = (pc.pieces & 4) ? 0u : tail_crc_line<Tile>(buf, mo, ft);
  EXPECT(crc_from_pieces(start, mo, pc.suf, pc.sxm, tail, tiles, ft) == crc32(start, mo));
  EXPECT(crc_from_pieces4(start, mo, pc.suf, pc.sxm, tail, tiles, tiles[k1], ft) == crc32(start, mo));
}

int main() {
  for (uint32_t i = 0; i < 256; i++) {
    uint32_t c = i;
    for (int k = 0; k < 8; k++) c = (c >> 1) ^ ((c & 1) ? 0xEDB88320u : 0u);
    btab[i] = c;
  }
  uint64_t z = 0x5EED0F1Dull;
  for (auto& b : buf) {
    z = z * 6364136223846793005ull + 1442695040888963407ull;
    b = (uint8_t)(z >> 56);
  }
  build_crc_tables(ct);
  ft = fin_tabs_host(ct);
  for (uint64_t k = 0; k < NT; k++)  // what the scan records per tile: lines 0..31, 1..31, 32..63
    tiles[k] = {{partial_at(k * TILE), partial_at(k * TILE + 64), suffix_at(k * TILE + TILE / 2), 0}};

  // the per-tile values give the suffix of lines 0, 1 and 32, and of no other line
  for (uint64_t k = 0; k < NT; k++)
    for (uint32_t j = 0; j < 64; j++) {
      uint32_t v = 0;
      const bool kept = tile_line(tiles[k], j, ft, &v);
      EXPECT(kept == (j == 0 || j == 1 || j == 32));
      if (kept) EXPECT(v == suffix_at(k * TILE + 64 * j) && v == tile_suffix(tiles[k], j, ft));
    }

  // sweep: line classes x whole tiles between (n = -1: the same tile)
  const uint32_t lines[] = {0, 1, 32, 7, 45};  // 0, 1, 32, other (a lower and an upper one)
  const uint32_t offs[] = {0, 17, 63};         // m's offset in its line (0: no partial last line)
  for (uint32_t sj : lines)
    for (uint32_t mj : lines)
      for (int n = -1; n <= 22; n++)
        for (uint32_t off : offs) {
          const uint64_t k0 = 1, k1 = k0 + 1 + n;
          const uint64_t s = k0 * TILE + 64 * sj, m = k1 * TILE + 64 * mj + off;
          if (m < s) continue;
          check_crc(s, m);
        }
  // short entries (and their neighbours): the tail alone below 64 bytes
  for (uint64_t len : {0, 1, 63, 64, 65})
    for (uint64_t s : {0ull, 64ull * 63, 1ull * TILE + 64 * 31, 3ull * TILE + 64 * 62}) {
      check_crc(s, s + len);
      EXPECT(fin_route(len, s / TILE, (s + len) / TILE, 7) == (len < 64 ? FIN_SHORT : FIN_INLINE));
      EXPECT(fin_route(len, s / TILE, (s + len) / TILE, 0) == (len < 64 ? FIN_SHORT : FIN_SLOW));
    }

  // every fin_pieces branch.  The start's source: {parent flags, start line}
  struct Suf {
    uint32_t pfl, line;
    bool lo, known;  // lo: the parent recorded a lower-half partial
  };
  const Suf sufs[] = {
      {0, 40, false, true},                                   // kind 0: the parent's value
      {F_SUF_LO, 7, true, true},                              // kind 0, a lower-half partial
      {1u << F_SUF_SHIFT, 0, false, true},                    // kind 1: line 0 of the next tile
      {2u << F_SUF_SHIFT, 1, false, true},                    // kind 2: line 1
      {F_NO_PARENT, 0, false, true},  {F_NO_PARENT, 1, false, true},  // no parent record: by the start line
      {F_NO_PARENT, 32, false, true}, {F_NO_PARENT, 7, false, false}, {F_NO_PARENT, 45, false, false},
  };
  struct Sxm {
    uint32_t fl, line;
    bool known;
  };
  const Sxm sxms[] = {
      {F_SXM, 40, true}, {F_SXM | F_SXM_LO, 7, true},                          // recorded: value, lower-half partial
      {0, 0, true},      {0, 1, true},      {0, 32, true}, {0, 7, false}, {0, 45, false},  // by the metadata line
  };
  for (const Suf& sf : sufs)
    for (const Sxm& sx : sxms)
      for (int n : {-1, 0, 3, (int)LONG_TILES, (int)LONG_TILES + 1, 22})
        for (uint32_t off : {0u, 29u}) {
          const uint64_t k0 = 2, k1 = k0 + 1 + n;
          const uint64_t start = k0 * TILE + 64 * sf.line, mo = k1 * TILE + 64 * sx.line + off;
          if (mo < start) continue;
          const uint32_t psuf = sf.lo ? partial_at(start) : ((sf.pfl >> F_SUF_SHIFT) & 3) == 0 ? suffix_at(start) : 0xDEADBEEFu;
          const uint32_t sxv = !(sx.fl & F_SXM) ? 0xDEADBEEFu : (sx.fl & F_SXM_LO) ? partial_at(mo) : suffix_at(mo);
          check_entry(sx.fl | (off ? 0u : F_TAIL), sxv, sf.pfl, psuf, start, mo, sf.known, sx.known);
        }
  // the root entry: no record, no parent, start 0 (finalize_core synthesises these inputs)
  check_entry(0, 0, F_NO_PARENT, 0, 0, 1 * TILE, true, true);
  check_entry(0, 0, F_NO_PARENT, 0, 0, 2 * TILE + 64 * 9 + 5, true, false);
  // the tombstone: one zero byte at p, start == p (no pre-pad), a constant CRC
  {
    const uint64_t p = 5 * TILE + 777;
    EXPECT(fin_start(F_TOMB, p) == p && fin_start(0, p) == ((p + 63) & ~63ull) && fin_start(0, 128) == 128);
    const uint8_t keep = buf[p];
    buf[p] = 0;
    EXPECT(TOMB_CRC == crc32(p, p + 1));
    buf[p] = keep;
  }

  return check_done("fin_check", "%llu cases", (unsigned long long)g_cases);
}
