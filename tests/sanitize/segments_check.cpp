// ASan/UBSan check of the segment append's arithmetic (TEST INFRASTRUCTURE):
// rust-simd-r-drive_amd/csrc/srd_segments.h compiled for the host, the very
// code the layout / unit / combine kernels and the host glue of
// srd_batch_append_segments_device run, over srd_append.h and the tables of
// srd_crc.h.  Over seeded random segment tables:
//   - the units tile every entry's bytes exactly once and in order, every unit
//     lies inside one segment, is at most SRD_GATHER_CHUNK long, and ends where
//     the next unit's destination begins; every unit but a segment's first
//     starts at a 16-byte boundary of the store;
//   - a unit's descriptor never lets an aligned 16-byte load leave its segment,
//     and the funnel of the loaded vectors gives the unit's bytes;
//   - the same for the chunk units of the gather and the append (a whole range
//     as one segment: the range view) at every start residue, with the pad
//     count of a last unit;
//   - over seeded range batches, the range view and an explicit table of one
//     segment per entry give the same descriptor for every unit;
//   - the XOR of the units' terms (bitwise host CRC per unit) is the CRC-32 of
//     the concatenation (check value 0xCBF43926 included);
//   - the entry layout equals srd_batch_layout's for the concatenated lengths
//     at every tail residue 0..63;
//   - every refusal the arithmetic decides is taken, the first entry deciding,
//     with wrap-around values near 2^64.
// Exit status 0 = no sanitizer report and every invariant held.
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <random>
#include <vector>

#include "check.h"
#include "srd_segments.h"
#include "srd_host.h"

using namespace srd;

static const uint64_t C = GATHER_CHUNK;
static const uint64_t M = ~0ull;

// what the device computes for a batch: per entry status / length / units, the
// error word, the exclusive sums, the coarse sum, the new tail
struct Batch {
  std::vector<uint64_t> len, slot, eun, pre, soff, sun, upre;
  std::vector<uint32_t> sent;
  uint64_t err = M, coarse = 0, new_tail = 0, units = 0;
  bool tail_ok = false;
};
static Batch device_layout(uint64_t tail, const std::vector<srd_segment>& segs, const std::vector<uint64_t>& first,
                           const std::vector<uint64_t>& src_lens) {
  const uint64_t n = first.size() - 1, ns = segs.size();
  Batch b;
  b.len.assign(n, 0);
  b.slot.assign(n, 0);
  b.eun.assign(n, 0);
  b.pre.assign(n + 1, 0);
  b.soff.assign(ns, 0);
  b.sun.assign(ns, 0);
  b.upre.assign(ns + 1, 0);
  b.sent.assign(ns, 0);
  uint64_t len_last = 0;
  for (uint64_t i = n; i-- > 0;) {  // (any order: the minimum decides)
    SegEntry e{SEG_BAD_FIRST, 0, 0};
    if (seg_first_ok(first[i], first[i + 1], i, n, ns)) {
      e = seg_entry_layout(segs.data(), first[i], first[i + 1], src_lens.data(), src_lens.size(), b.soff.data(), b.sun.data());
      for (uint64_t s = first[i]; s < first[i + 1]; s++) b.sent[s] = (uint32_t)i;
    }
    if (i == n - 1) len_last = e.len;
    if (e.status != APPEND_OK) {
      const uint64_t w = append_err_word(i, e.status);
      if (w < b.err) b.err = w;
      continue;
    }
    b.len[i] = e.len;
    b.slot[i] = append_slot(e.len);
    b.eun[i] = e.units;
    b.coarse += append_coarse(b.slot[i]);
  }
  for (uint64_t i = 0; i < n; i++) b.pre[i + 1] = b.pre[i] + b.slot[i];
  for (uint64_t s = 0; s < ns; s++) b.upre[s + 1] = b.upre[s] + b.sun[s];
  b.units = b.upre[ns];
  if (n) b.tail_ok = append_new_tail(tail, b.coarse, b.pre[n - 1], len_last, &b.new_tail);
  return b;
}

// The streaming kernel's walk over a unit's frame, piece by piece (seg_frame,
// seg_piece_vec): a piece that moves as vectors reads aligned source vectors
// that lie inside the segment [seg, seg + seg_len) and writes 16 bytes of the
// unit; the funnel of the pair gives the unit's bytes (`want`); only the first
// and last partial piece, and for r != 0 at most one whole piece at either end
// of a SEGMENT, go byte by byte.
static uint64_t g_vec = 0, g_bytewise = 0;
static void check_frame(const SegUnit& x, uint64_t seg, uint64_t seg_len, const uint8_t* want) {
  const SegFrame f = seg_frame(x.src, x.dst, x.lf);
  const uint64_t fs = x.src - f.a;  // the frame's first byte in the source
  EXPECT(f.a == (x.dst & 15) && f.vlen == f.a + seg_lf_len(x.lf) && f.vlen <= C);
  uint32_t slow_whole = 0;
  for (uint32_t o = 0; o < f.vlen; o += 16) {
    if (!seg_piece_vec(f, o)) {
      const bool whole = o >= f.a && o + 16 <= f.vlen;
      EXPECT(whole ? f.r != 0 : (o == 0 || o + 16 > f.vlen));
      if (whole) {
        slow_whole++;
        // ... only where the pair would leave the segment
        EXPECT(fs + o - f.r < seg || fs + o - f.r + 32 > seg + seg_len);
      }
      g_bytewise++;
      continue;
    }
    g_vec++;
    const uint64_t q = fs + o - f.r, nq = f.r ? 32 : 16;
    EXPECT(q % 16 == 0 && q >= seg && q + nq <= seg + seg_len);
    if (!(q >= seg && q + nq <= seg + seg_len)) continue;
    uint32_t w[8] = {0}, d[4];
    memcpy(w, (const void*)(uintptr_t)q, nq);
    for (int k = 0; k < 4; k++) {  // v_alignbyte_b32(hi, lo, sh) = ({hi, lo} >> 8 sh), low 32 bits
      const uint32_t lo = w[(f.r >> 2) + k], hi = w[(f.r >> 2) + k + 1 < 8 ? (f.r >> 2) + k + 1 : 7], sh = f.r & 3;
      d[k] = f.r ? (uint32_t)((((uint64_t)hi << 32) | lo) >> (8 * sh)) : w[k];
    }
    EXPECT(memcmp(d, want + (o - f.a), 16) == 0);
  }
  EXPECT(slow_whole <= 2);
}

static uint64_t g_entries = 0, g_segs = 0, g_units = 0;
static void check_tables(const CrcTables& t, std::mt19937_64& rng, uint64_t tail, const std::vector<std::vector<uint8_t>>& src) {
  const uint64_t n = 1 + rng() % 12;
  std::vector<uint64_t> src_lens;
  for (auto& s : src) src_lens.push_back(s.size());
  std::vector<srd_segment> segs;
  std::vector<uint64_t> first = {0};
  std::vector<std::vector<uint8_t>> cat(n);
  for (uint64_t i = 0; i < n; i++) {
    const uint64_t k = 1 + rng() % 5;
    for (uint64_t j = 0; j < k; j++) {
      srd_segment g{};
      g.src = (uint32_t)(rng() % src.size());
      g.len = pick_len(rng, C);
      if (j == k - 1 && cat[i].empty() && !g.len) g.len = 1 + rng() % 100;  // (no empty entry here)
      if (g.len > src_lens[g.src]) g.len = src_lens[g.src];
      g.off = rng() % (src_lens[g.src] - g.len + 1);
      segs.push_back(g);
      cat[i].insert(cat[i].end(), src[g.src].begin() + g.off, src[g.src].begin() + g.off + g.len);
    }
    first.push_back(segs.size());
  }
  const Batch b = device_layout(tail, segs, first, src_lens);
  EXPECT(b.err == M && b.tail_ok);
  if (b.err != M) return;
  // the entry layout against srd_batch_layout over the concatenated lengths
  std::vector<uint64_t> len(n), zero(n, 0);
  for (uint64_t i = 0; i < n; i++) len[i] = cat[i].size();
  std::vector<srd_write_entry> E(n);
  uint64_t want_tail = 0;
  const char* why = "";
  EXPECT(srd_host::batch_layout(tail, nullptr, zero.data(), zero.data(), zero.data(), len.data(), n, 0, E.data(),
                                &want_tail, &why) == 0);
  const uint64_t base = append_base(tail);
  for (uint64_t i = 0; i < n; i++) {
    EXPECT(b.len[i] == len[i]);
    const uint64_t P = append_payload(base, b.pre[i]), m = append_meta(base, b.pre[i], len[i]);
    const uint64_t prev = i ? append_meta(base, b.pre[i - 1], len[i - 1]) + 20 : tail;
    EXPECT(prev == E[i].tail);
    EXPECT(P == E[i].tail + ((64 - E[i].tail % 64) & 63));
    EXPECT(P % 64 == 0 && m == P + len[i]);
    if (i + 1 < n) EXPECT(append_payload(base, b.pre[i + 1]) == gather_pad64(m + 20));
  }
  EXPECT(b.new_tail == want_tail);
  // the units: in unit order they walk every entry's bytes once, front to back
  std::vector<uint64_t> covered(n, 0), seen(n, 0);
  std::vector<uint32_t> term(n, 0);
  uint64_t next_dst = 0, prev_ent = M, prev_seg = M;
  for (uint64_t u = 0; u < b.units; u++) {
    const uint64_t s = gather_unit_hit(b.upre.data(), segs.size(), u);
    EXPECT(s < segs.size() && b.upre[s] <= u && u < b.upre[s + 1]);
    const srd_segment g = segs[s];
    const uint32_t i = b.sent[s];
    EXPECT(first[i] <= s && s < first[i + 1]);
    const uint64_t dst0 = base + b.pre[i] + b.soff[s], k = u - b.upre[s];
    const uint8_t* sp = src[g.src].data();
    const SegUnit x = seg_unit((uint64_t)(uintptr_t)sp + g.off, dst0, b.soff[s], g.len, k, i, b.eun[i]);
    const uint64_t ul = seg_lf_len(x.lf);
    EXPECT(x.ent == i && ul >= 1 && ul <= C);
    // inside its segment, in the source and in the store
    const uint64_t b0 = x.src - ((uint64_t)(uintptr_t)sp + g.off);
    EXPECT(b0 < g.len && b0 + ul <= g.len && x.dst == dst0 + b0);
    EXPECT(k == 0 ? b0 == 0 : x.dst % 16 == 0);
    EXPECT((x.dst & 15) + ul <= C);  // the destination-aligned frame fits a unit's blocks
    EXPECT(seg_lf_below(x.lf) == (b0 < 16 ? b0 : 16) && seg_lf_behind(x.lf) == (g.len - b0 - ul < 16 ? g.len - b0 - ul : 16));
    EXPECT(seg_lf_single(x.lf) == (b.eun[i] == 1));
    // in order: the entry's next byte, the store's next byte
    EXPECT(x.dst == base + b.pre[i] + covered[i] && x.end == covered[i] + ul);
    if (prev_ent == i) EXPECT(x.dst == next_dst);
    else EXPECT(covered[i] == 0 && (prev_ent == M || i > prev_ent));
    if (prev_seg != M) EXPECT(s >= prev_seg);
    EXPECT(memcmp(sp + g.off + b0, cat[i].data() + covered[i], ul) == 0);
    check_frame(x, (uint64_t)(uintptr_t)sp + g.off, g.len, cat[i].data() + covered[i]);
    next_dst = x.dst + ul;
    prev_ent = i;
    prev_seg = s;
    covered[i] += ul;
    seen[i]++;
    term[i] ^= seg_unit_term(host_crc_raw_bytes(t, 0, sp + g.off + b0, ul), len[i], x.end, t.pow8);
  }
  for (uint64_t i = 0; i < n; i++) {
    EXPECT(seen[i] == b.eun[i] && covered[i] == len[i]);
    EXPECT(gather_final(term[i], len[i], t.pow8) == (uint32_t)~host_crc_raw_bytes(t, 0xFFFFFFFFu, cat[i].data(), len[i]));
  }
  g_entries += n;
  g_segs += segs.size();
  g_units += b.units;
}

static void check_cut() {
  for (uint64_t a = 0; a < 16; a++) {
    EXPECT(seg_unit_count(a, 0) == 0);
    EXPECT(seg_unit_count(a, 1) == 1);
    EXPECT(seg_unit_count(a, C - a) == 1);
    EXPECT(seg_unit_count(a, C - a + 1) == 2);
    EXPECT(seg_unit_count(a, 2 * C - a) == 2);
    uint64_t b0, b1;
    seg_unit_range(a, 3 * C, 0, &b0, &b1);
    EXPECT(b0 == 0 && b1 == C - a);
    seg_unit_range(a, 3 * C, 1, &b0, &b1);
    EXPECT(b0 == C - a && b1 == 2 * C - a);
    seg_unit_range(a, 3 * C, seg_unit_count(a, 3 * C) - 1, &b0, &b1);
    EXPECT(b1 == 3 * C && b1 - b0 == (a ? a : C));
  }
  // a segment that starts 16-aligned in the store is cut like a payload of the append
  for (uint64_t len : std::vector<uint64_t>{1, C - 1, C, C + 1, 3 * C + 4097}) {
    EXPECT(seg_unit_count(0, len) == gather_chunks(len));
    for (uint64_t k = 0; k < gather_chunks(len); k++) {
      uint64_t b0, b1;
      seg_unit_range(0, len, k, &b0, &b1);
      EXPECT(b0 == k * C && b1 - b0 == gather_chunk_len(len, k));
    }
  }
}

// Chunk units as the gather and the append build them (unit_of<RangeView>): a
// whole range [start, end) taken as one segment whose destination starts at a
// 64-byte boundary (here: range 7 of 8, the others without units).  At every start residue, for lengths around 16, 4096, C and 2 C:
// the units are the range's chunks, every aligned source vector the streaming
// kernel's walk admits lies inside [start, end) (check_frame; the range ends at
// its allocation's end, so the sanitizer sees a read past it), and a range's
// last unit owns the zero bytes up to the next 64-byte boundary when asked to.
static uint64_t g_chunk_units = 0;
static void check_chunk_units(std::mt19937_64& rng) {
  const uint64_t lens[] = {1, 15, 16, 17, 31, 32, 33, 47, 48, 49, 4095, 4096, 4097, 4111, 4112, 4113, C - 17, C - 16,
                           C - 1, C, C + 1, C + 15, C + 16, C + 17, 2 * C - 1, 2 * C, 2 * C + 1, 2 * C + 17};
  for (uint64_t res = 0; res < 16; res++) {
    for (uint64_t len : lens) {
      uint8_t* exact = (uint8_t*)malloc(16 + res + len);  // (malloc aligns to 16: the range ends where the block ends)
      EXPECT(exact && ((uintptr_t)exact & 15) == 0);
      if (!exact || ((uintptr_t)exact & 15)) continue;
      for (uint64_t j = 0; j < 16 + res + len; j++) exact[j] = (uint8_t)(rng() >> 56);
      const uint64_t start = (uint64_t)(uintptr_t)exact + 16 + res;
      const std::vector<uint8_t> copy(exact + 16 + res, exact + 16 + res + len);
      const uint64_t chunks = gather_chunks(len), dst = 64 * (1 + rng() % 1000);
      uint64_t r_st[8] = {0}, r_en[8] = {0}, r_un[8] = {0}, r_off[8] = {0}, r_pre[8] = {0};
      r_st[7] = start;
      r_en[7] = start + len;
      r_un[7] = chunks;
      r_off[7] = dst;
      UnitArgs ra{};
      ra.n = ra.n_segs = 8;
      ra.start = r_st;
      ra.end = r_en;
      ra.eun = r_un;
      ra.off = r_off;
      ra.upre = r_pre;
      for (int pad = 0; pad < 2; pad++) {
        ra.pad = pad;
        for (uint64_t k = 0; k < chunks; k++) {
          const SegUnit x = unit_of<RangeView>(ra, k);
          const uint64_t cl = gather_chunk_len(len, k);
          EXPECT(x.src == start + k * C && x.dst == dst + k * C && seg_lf_len(x.lf) == cl && x.end == k * C + cl);
          EXPECT(x.ent == 7 && seg_lf_single(x.lf) == (chunks == 1) && (x.dst & 15) == 0);
          EXPECT(seg_lf_below(x.lf) == (k ? 16 : 0));
          EXPECT(seg_lf_behind(x.lf) == (len - x.end < 16 ? len - x.end : 16));
          EXPECT(seg_frame(x.src, x.dst, x.lf).r == (res & 15));
          EXPECT(seg_unit_pad(x.dst, x.lf) == (pad && k + 1 == chunks ? gather_pad64(len) - len : 0));
          check_frame(x, start, len, copy.data() + k * C);
          g_chunk_units++;
        }
      }
      free(exact);
    }
  }
}

// Range batches (the generator of gather_check.cpp's check_batch: hits of 1
// byte .. 5 chunks, None reads, bad ranges, duplicates) as the gather lays them
// out, with a 64-aligned dst0, with and without pad: the range view and an
// explicit table of one segment per entry (a range without units: an empty
// segment) give the same descriptor for every unit.  Nothing is dereferenced.
static uint64_t g_view_units = 0;
static void check_views(std::mt19937_64& rng) {
  const uint64_t F = 40 * C;
  const uint64_t n = 1 + rng() % 200;
  std::vector<uint64_t> st(n), en(n), len(n), chk(n), off(n + 1), cpre(n + 1), zero(n, 0), first(n + 1);
  std::vector<uint32_t> sent(n);
  std::vector<srd_segment> segs(n);
  static const uint8_t file[64] = {0};  // (the ranges' base address only)
  uint64_t so = 0, sc = 0;
  for (uint64_t i = 0; i < n; i++) {
    const uint32_t kind = rng() % 10;
    uint64_t l;
    switch (rng() % 5) {
      case 0: l = 1 + rng() % 200; break;
      case 1: l = 1 + rng() % (5 * C); break;
      case 2: l = C * (1 + rng() % 5); break;
      case 3: l = C * (1 + rng() % 4) + (rng() % 2 ? 1 : C - 1); break;
      default: l = 1 + rng() % 9000; break;
    }
    st[i] = (rng() % (F - 20 - l)) & (rng() % 4 ? ~63ull : ~0ull);
    en[i] = st[i] + l;
    if (kind == 0) en[i] = st[i];                       // a None read
    if (kind == 1) std::swap(st[i], en[i]);             // start > end
    if (kind == 2) en[i] = F - rng() % 20;              // metadata past the end
    if (kind == 3 && i) { st[i] = st[i - 1]; en[i] = en[i - 1]; }  // a duplicate
    len[i] = gather_range_status(st[i], en[i], F) == SRD_GATHER_OK ? en[i] - st[i] : 0;
    chk[i] = gather_chunks(len[i]);
    off[i] = so;
    cpre[i] = sc;
    so += gather_pad64(len[i]);
    sc += chk[i];
    segs[i] = srd_segment{};
    segs[i].off = len[i] ? st[i] : 0;
    segs[i].len = len[i];
    sent[i] = (uint32_t)i;
    first[i] = i;
  }
  off[n] = so;
  cpre[n] = sc;
  first[n] = n;
  const uint64_t srcs[2] = {(uint64_t)(uintptr_t)file, F};
  for (int pad = 0; pad < 2; pad++) {
    UnitArgs r{};
    r.n = r.n_segs = n;
    r.eun = chk.data();
    r.off = off.data();
    r.upre = cpre.data();
    r.dst0 = 64 * (rng() % 100000);
    r.pad = pad;
    r.n_units = sc;
    UnitArgs tb = r;
    r.file = file;
    r.start = st.data();
    r.end = en.data();
    tb.srcs = srcs;
    tb.segs = segs.data();
    tb.first = first.data();
    tb.len = len.data();
    tb.soff = zero.data();
    tb.sun = chk.data();
    tb.sent = sent.data();
    for (uint64_t u = 0; u < sc; u++) {
      const SegUnit x = unit_of<RangeView>(r, u), y = unit_of<TableView>(tb, u);
      EXPECT(x.src == y.src && x.dst == y.dst && x.end == y.end && x.ent == y.ent && x.lf == y.lf);
      EXPECT(x.ent < n && RangeView::ent_len(r, x.ent) == TableView::ent_len(tb, x.ent));
      EXPECT(unit_first<RangeView>(r, x.ent) == unit_first<TableView>(tb, x.ent));
      const uint64_t k = u - cpre[x.ent];  // the bits of a chunk unit
      EXPECT(x.src == (uint64_t)(uintptr_t)file + st[x.ent] + k * C && x.dst == r.dst0 + off[x.ent] + k * C);
      EXPECT(seg_lf_len(x.lf) == gather_chunk_len(len[x.ent], k) && !(x.lf & SEG_LF_PAD) == !(pad && k + 1 == chk[x.ent]));
    }
    g_view_units += sc;
  }
}

static void check_crc_value(const CrcTables& t) {
  // "123456789" in three pieces behind a 5-byte piece of another source: CRC-32 0xCBF43926
  const uint8_t s[] = "123456789";
  const uint64_t cut[4] = {0, 2, 2, 9};  // (one piece is empty)
  uint32_t x = 0;
  for (int j = 0; j < 3; j++) x ^= seg_unit_term(host_crc_raw_bytes(t, 0, s + cut[j], cut[j + 1] - cut[j]), 9, cut[j + 1], t.pow8);
  EXPECT(gather_final(x, 9, t.pow8) == 0xCBF43926u);
}

static srd_segment seg(uint32_t src, uint64_t off, uint64_t len, uint32_t reserved = 0) {
  srd_segment g{};
  g.src = src;
  g.reserved = reserved;
  g.off = off;
  g.len = len;
  return g;
}

static void check_refusals() {
  const std::vector<uint64_t> sl = {1000, 0, M};
  auto st = [&](const std::vector<srd_segment>& segs, const std::vector<uint64_t>& first) {
    return device_layout(100, segs, first, sl).err;
  };
  const srd_segment ok = seg(0, 10, 20);
  EXPECT(st({ok}, {0, 1}) == M);
  EXPECT(st({seg(0, 0, 1000)}, {0, 1}) == M);
  EXPECT(st({seg(0, 1000, 0), ok}, {0, 2}) == M);  // an empty range at the source's end is a range
  // the empty entry: no segments, only zero-length ones
  EXPECT(st({ok}, {0, 0, 1}) == append_err_word(0, APPEND_EMPTY));
  EXPECT(st({ok, seg(0, 5, 0), seg(1, 0, 0)}, {0, 1, 3}) == append_err_word(1, APPEND_EMPTY));
  // malformed segments
  EXPECT(st({seg(3, 0, 1)}, {0, 1}) == append_err_word(0, SEG_BAD_SEGMENT));           // src >= n_src
  EXPECT(st({seg(0xFFFFFFFFu, 0, 1)}, {0, 1}) == append_err_word(0, SEG_BAD_SEGMENT));
  EXPECT(st({seg(0, 10, 20, 1)}, {0, 1}) == append_err_word(0, SEG_BAD_SEGMENT));      // reserved
  EXPECT(st({seg(0, 999, 2)}, {0, 1}) == append_err_word(0, SEG_BAD_SEGMENT));         // one byte past the source
  EXPECT(st({seg(0, 1001, 0)}, {0, 1}) == append_err_word(0, SEG_BAD_SEGMENT));
  EXPECT(st({seg(1, 0, 1)}, {0, 1}) == append_err_word(0, SEG_BAD_SEGMENT));           // an empty source
  EXPECT(st({seg(0, M, 1)}, {0, 1}) == append_err_word(0, SEG_BAD_SEGMENT));           // off + len wraps to 0
  EXPECT(st({seg(0, M - 7, 108)}, {0, 1}) == append_err_word(0, SEG_BAD_SEGMENT));     // wraps into the source
  EXPECT(st({seg(0, 8, M - 7)}, {0, 1}) == append_err_word(0, SEG_BAD_SEGMENT));       // wraps to 0
  EXPECT(st({seg(0, 100, M)}, {0, 1}) == append_err_word(0, SEG_BAD_SEGMENT));
  EXPECT(st({seg(0, 1ull << 63, 1ull << 63)}, {0, 1}) == append_err_word(0, SEG_BAD_SEGMENT));
  // ... decide whatever the entry's length: among empty segments, behind a too long one
  EXPECT(st({seg(0, 0, 0), seg(0, 2000, 0)}, {0, 2}) == append_err_word(0, SEG_BAD_SEGMENT));
  EXPECT(st({seg(2, 0, APPEND_TAIL_LIMIT), seg(0, 999, 2)}, {0, 2}) == append_err_word(0, SEG_BAD_SEGMENT));
  // an entry of 2^48 bytes or more: one segment, several, a sum that would wrap 2^64
  const uint64_t L = APPEND_TAIL_LIMIT;
  EXPECT(st({seg(2, 0, L - 1)}, {0, 1}) == M);
  EXPECT(st({seg(2, 0, L)}, {0, 1}) == append_err_word(0, APPEND_TOO_LONG));
  EXPECT(st({seg(2, 0, L - 1), seg(0, 0, 1)}, {0, 2}) == append_err_word(0, APPEND_TOO_LONG));
  EXPECT(st({seg(2, 0, L - 2), seg(0, 0, 1)}, {0, 2}) == M);
  EXPECT(st({seg(2, 5, M - 5), seg(2, 0, 6)}, {0, 2}) == append_err_word(0, APPEND_TOO_LONG));  // the sum wraps to 0
  EXPECT(st({seg(2, 1, M - 1), seg(2, 1, M - 1), seg(2, 0, 3)}, {0, 3}) == append_err_word(0, APPEND_TOO_LONG));
  // d_seg_first
  EXPECT(st({ok, ok}, {1, 2}) == append_err_word(0, SEG_BAD_FIRST));        // first[0] != 0
  EXPECT(st({ok, ok}, {0, 2, 1, 2}) == append_err_word(1, SEG_BAD_FIRST));  // a decreasing pair
  EXPECT(st({ok, ok}, {0, 1}) == append_err_word(0, SEG_BAD_FIRST));        // first[n] != n_segs
  EXPECT(st({ok, ok}, {0, 1, 3}) == append_err_word(1, SEG_BAD_FIRST));
  EXPECT(st({ok, ok}, {0, M, 2}) == append_err_word(0, SEG_BAD_FIRST));     // (never used as an index)
  EXPECT(st({ok, ok}, {0, 1, M}) == append_err_word(1, SEG_BAD_FIRST));
  // the first refused entry decides, whatever the others are
  EXPECT(st({ok, seg(0, 0, 0), seg(5, 0, 1), ok}, {0, 1, 2, 3, 4}) == append_err_word(1, APPEND_EMPTY));
  EXPECT(st({ok, seg(5, 0, 1), seg(0, 0, 0), ok}, {0, 1, 2, 3, 4}) == append_err_word(1, SEG_BAD_SEGMENT));
  EXPECT(append_err_status(append_err_word(7, SEG_BAD_FIRST)) == SEG_BAD_FIRST);
  // the 2^48 bound on the new tail: nt = base + len + 20, the length in two segments
  for (uint64_t tail : {0ull, 1ull, 63ull, 64ull, 4097ull}) {
    const uint64_t base = append_base(tail);
    const Batch yes = device_layout(tail, {seg(2, 0, 7), seg(2, 9, L - 1 - 20 - base - 7)}, {0, 2}, sl);
    EXPECT(yes.err == M && yes.tail_ok && yes.new_tail == L - 1);
    const Batch no = device_layout(tail, {seg(2, 0, 7), seg(2, 9, L - 20 - base - 7)}, {0, 2}, sl);
    EXPECT(no.err == M && !no.tail_ok);
  }
  {  // the exact sum of the slots wraps 2^64: the coarse sum refuses
    const uint64_t n = 1ull << 17;
    std::vector<srd_segment> segs(n, seg(2, 0, (1ull << 47) - 20));
    std::vector<uint64_t> first(n + 1);
    for (uint64_t i = 0; i <= n; i++) first[i] = i;
    const Batch wrap = device_layout(0, segs, first, sl);
    EXPECT(wrap.err == M && wrap.pre[n] == 0 && !append_sum_exact(wrap.coarse) && !wrap.tail_ok);
  }
}

int main() {
  static CrcTables t;
  build_crc_tables(t);
  check_cut();
  check_crc_value(t);
  std::mt19937_64 rng(0x5EED5E65ull);
  std::vector<std::vector<uint8_t>> src(3);
  src[0].resize(3 * C + 100);
  src[1].resize(20);
  src[2].resize(C + 33);
  for (auto& s : src)
    for (auto& v : s) v = (uint8_t)(rng() >> 56);
  for (uint64_t res = 0; res < 64; res++)
    for (int it = 0; it < 3; it++) check_tables(t, rng, (rng() % 5000) * 64 + res, src);
  for (uint64_t res = 0; res < 64; res++) check_tables(t, rng, res, src);  // (a store of less than one line)
  check_chunk_units(rng);
  for (int it = 0; it < 100; it++) check_views(rng);
  check_refusals();
  return check_done("segments_check", "chunk %llu, %llu entries, %llu segments, %llu units, %llu chunk units, %llu units under both views",
                    (unsigned long long)C, (unsigned long long)g_entries, (unsigned long long)g_segs, (unsigned long long)g_units,
                    (unsigned long long)g_chunk_units, (unsigned long long)g_view_units);
}
