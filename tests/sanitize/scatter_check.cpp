// ASan/UBSan check of the scatter read's arithmetic (TEST INFRASTRUCTURE):
// rust-simd-r-drive_amd/csrc/srd_scatter.h and the scatter view of
// srd_segments.h compiled for the host, the very code the layout / unit /
// combine kernels and the host glue of srd_payload_scatter_device run.  A
// batch here is what the device sees: a 16-byte-aligned "file" of payloads at
// arbitrary start residues with guard bytes around them, destination arenas
// filled with 0xA5 whose segments lie at arbitrary residues with guard bytes
// between them, a destination table (ranges that overlap, an empty one with a
// NULL pointer), segments and first.  Over seeded random batches and a sweep of
// all 256 (destination residue, source residue) pairs:
//   - the units tile each OK entry's payload exactly once and in order, each
//     inside one destination segment and at most SRD_GATHER_CHUNK long, with a
//     frame of at most SRD_GATHER_CHUNK bytes;
//   - the layout's unit counts (seg_unit_count at the destination ADDRESS'
//     residue) equal the units' at every destination residue;
//   - walking seg_frame / seg_piece_vec piece by piece as the streaming kernel
//     does, no vector load leaves [start, end), no store leaves its segment,
//     the funnel gives the unit's bytes, and afterwards every arena equals the
//     expected image WHOLE (guard bytes, the segments of queries that are not
//     OK, and the other bytes of a vector that holds a head or a tail intact);
//   - the XOR of the units' terms is a bitwise CRC-32 of the payload;
//   - every refusal the arithmetic decides is taken, the first query deciding,
//     with values near 2^64; the range decides before the length does;
//   - SCATTER_BAD_LENGTH for sums one short and one over, and sums that would
//     wrap 2^64; a count that the prefix sum could not hold is capped so that
//     the total refuses the call.
// Exit status 0 = no sanitizer report and every invariant held.
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <random>
#include <vector>

#include "check.h"
#include "srd_scatter.h"

using namespace srd;

static const uint64_t C = GATHER_CHUNK;
static const uint64_t M = ~0ull;
static const uint8_t FILL = 0xA5, GUARD = 0xEE;

// what scatter_layout_kernel and the host compute for a batch
struct Layout {
  std::vector<uint8_t> st;
  std::vector<uint64_t> eun, soff, sun, upre;
  std::vector<uint32_t> sent;
  uint64_t err = M, units = 0, n_multi = 0;
};
static Layout device_layout(uint64_t flen, const std::vector<uint64_t>& start, const std::vector<uint64_t>& end,
                            const std::vector<srd_segment>& segs, const std::vector<uint64_t>& first,
                            const std::vector<uint64_t>& tab) {
  const uint64_t n = start.size(), ns = segs.size();
  Layout b;
  b.st.assign(n, 0xFF);
  b.eun.assign(n, 0);
  b.soff.assign(ns, 0);
  b.sun.assign(ns, 0);
  b.upre.assign(ns + 1, 0);
  b.sent.assign(ns, 0);
  for (uint64_t i = n; i-- > 0;) {  // (any order: the minimum decides)
    uint32_t st = gather_range_status(start[i], end[i], flen);
    uint64_t k = 0;
    if (!seg_first_ok(first[i], first[i + 1], i, n, ns)) {
      const uint64_t w = append_err_word(i, SEG_BAD_FIRST);
      if (w < b.err) b.err = w;
    } else {
      const ScatterEntry x = scatter_entry_layout(segs.data(), first[i], first[i + 1], ScatterTable{tab.data()}, tab.size() / 2,
                                                  st, end[i] - start[i], (uint32_t)i, b.soff.data(), b.sun.data(), b.sent.data());
      if (x.bad) {
        const uint64_t w = append_err_word(i, SEG_BAD_SEGMENT);
        if (w < b.err) b.err = w;
      }
      st = x.status;
      k = x.units;
    }
    b.st[i] = (uint8_t)st;
    b.eun[i] = k;
    b.n_multi += k > 1;
  }
  for (uint64_t s = 0; s < ns; s++) b.upre[s + 1] = b.upre[s] + b.sun[s];
  b.units = b.upre[ns];
  return b;
}

// A batch in host memory.  Query kinds: what the caller asks for.
enum Kind { K_OK, K_NONE, K_BAD_RANGE, K_SHORT, K_OVER };
struct SegSpec {
  uint64_t len;
  int res;  // destination residue 0..15, or -1: whatever the gap gives
};
struct QuerySpec {
  Kind kind;
  uint64_t len;  // payload bytes (>= 1)
  int res;       // start residue 0..15, or -1: random
  std::vector<SegSpec> segs;  // lengths summing to len (K_SHORT / K_OVER: the last one is changed by one)
};

struct Arena {
  uint8_t* p = nullptr;
  uint64_t size = 0;
  std::vector<uint8_t> want;  // the expected image
};

static uint64_t g_queries = 0, g_segs = 0, g_units = 0, g_vec = 0, g_bytewise = 0;

static void run_batch(const CrcTables& t, std::mt19937_64& rng, const std::vector<QuerySpec>& spec) {
  const uint64_t n = spec.size();
  // the file: guard, payload at its residue, 20 metadata bytes, guard, ...
  std::vector<uint64_t> start(n), end(n);
  uint64_t pos = 64;
  for (uint64_t i = 0; i < n; i++) {
    const uint64_t res = spec[i].res < 0 ? rng() % 16 : (uint64_t)spec[i].res;
    pos = ((pos + 32 + 15) & ~15ull) + res;
    start[i] = pos;
    end[i] = pos + spec[i].len;
    pos = end[i] + 20;
  }
  const uint64_t flen = pos;
  uint8_t* file = nullptr;
  EXPECT(posix_memalign((void**)&file, 64, flen + 64) == 0 && file);
  if (!file) return;
  memset(file, GUARD, flen + 64);
  for (uint64_t i = 0; i < n; i++)
    for (uint64_t j = start[i]; j < end[i]; j++) file[j] = (uint8_t)(rng() >> 56);
  std::vector<uint64_t> qs = start, qe = end;
  for (uint64_t i = 0; i < n; i++) {
    if (spec[i].kind == K_NONE) qe[i] = qs[i] = rng() % 2 ? start[i] : M - 3;
    if (spec[i].kind == K_BAD_RANGE) {
      switch (rng() % 3) {
        case 0: std::swap(qs[i], qe[i]); break;  // start > end
        case 1: qe[i] = flen - rng() % 20; break;  // metadata past the end
        default: qe[i] = M - rng() % 5; break;
      }
    }
  }
  // the segments: each in one of three arenas, behind a gap that gives it its residue
  Arena ar[3];
  uint64_t cur[3] = {32, 32, 32};
  struct Placed { int arena; uint64_t off, len; uint64_t q; };
  std::vector<Placed> placed;
  std::vector<uint64_t> first = {0};
  for (uint64_t i = 0; i < n; i++) {
    std::vector<SegSpec> sg = spec[i].segs;
    if (spec[i].kind == K_SHORT) {
      uint64_t j = sg.size();
      while (j-- > 0)
        if (sg[j].len) { sg[j].len--; break; }
    }
    if (spec[i].kind == K_OVER) sg.back().len++;
    for (const SegSpec& g : sg) {
      const int a = (int)(rng() % 3);
      uint64_t off = cur[a] + 1 + rng() % 40;
      if (g.res >= 0) off = ((off + 15) & ~15ull) + (uint64_t)g.res;
      placed.push_back(Placed{a, off, g.len, i});
      cur[a] = off + g.len;
    }
    first.push_back(placed.size());
  }
  for (int a = 0; a < 3; a++) {
    ar[a].size = cur[a] + 33 + rng() % 16;
    EXPECT(posix_memalign((void**)&ar[a].p, 16, ar[a].size) == 0 && ar[a].p);
    if (!ar[a].p) return;
    memset(ar[a].p, FILL, ar[a].size);
    ar[a].want.assign(ar[a].size, FILL);
  }
  // the table: per arena a range that leaves lead bytes out at either side, for
  // arena 0 a second range that overlaps the first, and an empty range at NULL
  uint64_t lead[4] = {rng() % 16, rng() % 16, rng() % 16, 16 + rng() % 16};
  std::vector<uint64_t> tab;
  for (int a = 0; a < 3; a++) {
    tab.push_back((uint64_t)(uintptr_t)ar[a].p + lead[a]);
    tab.push_back(ar[a].size - 2 * lead[a]);
  }
  tab.push_back((uint64_t)(uintptr_t)ar[0].p + lead[3]);
  tab.push_back(ar[0].size - lead[3] - 7);
  tab.push_back(0);
  tab.push_back(0);
  uint64_t base = M;
  for (uint64_t k = 0; k < tab.size() / 2; k++)
    if (tab[2 * k + 1] && tab[2 * k] < base) base = tab[2 * k];
  base &= ~15ull;
  std::vector<srd_segment> segs;
  for (const Placed& p : placed) {
    srd_segment g{};
    int k = p.arena == 0 && rng() % 2 ? 3 : p.arena;
    if (k == 3 && p.off + p.len > ar[0].size - 7) k = 0;
    g.src = (uint32_t)k;
    g.off = p.off - lead[k];
    g.len = p.len;
    if (!p.len && rng() % 4 == 0) { g.src = 4; g.off = 0; }  // an empty segment in the empty range
    segs.push_back(g);
  }
  const Layout b = device_layout(flen, qs, qe, segs, first, tab);
  EXPECT(b.err == M);
  // statuses, and the expected image
  for (uint64_t i = 0; i < n; i++) {
    const uint32_t want_st = spec[i].kind == K_OK ? SRD_GATHER_OK : spec[i].kind == K_NONE ? SRD_GATHER_NONE
                             : spec[i].kind == K_BAD_RANGE ? SRD_GATHER_BAD_RANGE : SCATTER_BAD_LENGTH;
    EXPECT(b.st[i] == want_st);
    uint64_t so = 0, un = 0;
    for (uint64_t s = first[i]; s < first[i + 1]; s++) {
      EXPECT(b.sent[s] == i);
      if (want_st != SRD_GATHER_OK) { EXPECT(b.sun[s] == 0); continue; }
      const Placed& p = placed[s];
      EXPECT(b.soff[s] == so);
      // the layout's count at the destination ADDRESS' residue
      EXPECT(b.sun[s] == seg_unit_count(((uint64_t)(uintptr_t)ar[p.arena].p + p.off) & 15, p.len));
      memcpy(ar[p.arena].want.data() + p.off, file + start[i] + so, p.len);
      so += p.len;
      un += b.sun[s];
    }
    EXPECT(b.eun[i] == un && (want_st != SRD_GATHER_OK || (so == spec[i].len && un >= 1)));
  }
  EXPECT(b.units < (1ull << 32));
  // the units through the scatter view, as units_kernel builds them
  UnitArgs a{};
  a.n = n;
  a.n_segs = segs.size();
  a.eun = const_cast<uint64_t*>(b.eun.data());
  a.upre = const_cast<uint64_t*>(b.upre.data());
  a.file = file;
  a.start = qs.data();
  a.end = qe.data();
  a.srcs = tab.data();
  a.segs = segs.data();
  a.first = first.data();
  a.soff = const_cast<uint64_t*>(b.soff.data());
  a.sun = const_cast<uint64_t*>(b.sun.data());
  a.sent = const_cast<uint32_t*>(b.sent.data());
  a.dst0 = base;
  a.n_units = b.units;
  std::vector<uint64_t> covered(n, 0), seen(n, 0), seg_seen(segs.size(), 0);
  std::vector<uint32_t> term(n, 0);
  uint64_t prev_ent = M, prev_seg = M;
  for (uint64_t u = 0; u < b.units; u++) {
    const SegUnit x = unit_of<ScatterView>(a, u);
    const uint64_t s = gather_unit_hit(b.upre.data(), segs.size(), u);
    EXPECT(s < segs.size() && b.upre[s] <= u && u < b.upre[s + 1]);
    const Placed& p = placed[s];
    const uint64_t i = x.ent, ul = seg_lf_len(x.lf);
    EXPECT(i == p.q && i < n && b.st[i] == SRD_GATHER_OK);
    if (i >= n) return;
    EXPECT(ul >= 1 && ul <= C && !(x.lf & SEG_LF_PAD) && seg_unit_pad(x.dst, x.lf) == 0);
    EXPECT(seg_lf_single(x.lf) == (b.eun[i] == 1));
    // in order: the payload's next byte; inside its one destination segment
    const uint64_t pay = (uint64_t)(uintptr_t)file + start[i];
    EXPECT(x.src == pay + covered[i] && x.end == covered[i] + ul && x.end <= spec[i].len);
    if (prev_ent != i) EXPECT(covered[i] == 0 && (prev_ent == M || i > prev_ent));
    if (prev_seg != M) EXPECT(s >= prev_seg);
    const uint64_t sd = (uint64_t)(uintptr_t)ar[p.arena].p + p.off;  // the segment's destination
    const uint64_t ud = base + x.dst, b0 = ud - sd;
    EXPECT(ud >= sd && b0 + ul <= p.len && b0 == covered[i] - b.soff[s]);
    EXPECT(u == b.upre[s] ? b0 == 0 : ud % 16 == 0);
    EXPECT(seg_lf_below(x.lf) == (b0 < 16 ? b0 : 16) && seg_lf_behind(x.lf) == (p.len - b0 - ul < 16 ? p.len - b0 - ul : 16));
    // the streaming kernel's walk over the unit's frame
    const SegFrame f = seg_frame(x.src, x.dst, x.lf);
    EXPECT(f.a == (ud & 15) && f.vlen == f.a + ul && f.vlen <= C && f.r == ((x.src - ud) & 15));
    const uint64_t fs = x.src - f.a, fd = ud - f.a;  // the frame's first byte in the source / the destination
    const uint8_t* want = file + start[i] + covered[i];
    uint32_t slow_whole = 0;
    for (uint32_t o = 0; o < f.vlen; o += 16) {
      if (seg_piece_vec(f, o)) {
        g_vec++;
        const uint64_t q = fs + o - f.r, nq = f.r ? 32 : 16;
        const bool in = q % 16 == 0 && q >= pay && q + nq <= pay + spec[i].len;  // no vector load leaves [start, end)
        EXPECT(in && q >= pay + b.soff[s] && q + nq <= pay + b.soff[s] + p.len);
        const uint64_t d0 = fd + o;
        const bool out = d0 % 16 == 0 && d0 >= sd && d0 + 16 <= sd + p.len;  // no store leaves its segment
        EXPECT(out);
        if (!in || !out) continue;
        uint32_t w[8] = {0}, d[4];
        memcpy(w, (const void*)(uintptr_t)q, nq);
        for (int k = 0; k < 4; k++) {  // v_alignbyte_b32(hi, lo, sh) = ({hi, lo} >> 8 sh), low 32 bits
          const uint32_t lo = w[(f.r >> 2) + k], hi = w[(f.r >> 2) + k + 1 < 8 ? (f.r >> 2) + k + 1 : 7], sh = f.r & 3;
          d[k] = f.r ? (uint32_t)((((uint64_t)hi << 32) | lo) >> (8 * sh)) : w[k];
        }
        EXPECT(memcmp(d, want + (o - f.a), 16) == 0);
        memcpy((void*)(uintptr_t)d0, d, 16);
      } else {
        g_bytewise++;
        const bool whole = o >= f.a && o + 16 <= f.vlen;
        EXPECT(whole ? f.r != 0 : (o == 0 || o + 16 > f.vlen));
        slow_whole += whole;
        for (uint32_t pb = o; pb < o + 16; pb++) {
          if (pb < f.a || pb >= f.vlen) continue;
          const uint64_t q = fs + pb, d0 = fd + pb;
          const bool ok = q >= pay + b.soff[s] && q < pay + b.soff[s] + p.len && d0 >= sd && d0 < sd + p.len;
          EXPECT(ok);
          if (ok) *(uint8_t*)(uintptr_t)d0 = *(const uint8_t*)(uintptr_t)q;
        }
      }
    }
    EXPECT(slow_whole <= 2);
    term[i] ^= seg_unit_term(host_crc_raw_bytes(t, 0, want, ul), ScatterView::ent_len(a, i), x.end, t.pow8);
    covered[i] += ul;
    seen[i]++;
    seg_seen[s]++;
    prev_ent = i;
    prev_seg = s;
  }
  for (uint64_t s = 0; s < segs.size(); s++) EXPECT(seg_seen[s] == b.sun[s]);
  for (uint64_t i = 0; i < n; i++) {
    EXPECT(seen[i] == b.eun[i]);
    if (b.st[i] != SRD_GATHER_OK) { EXPECT(covered[i] == 0); continue; }
    EXPECT(covered[i] == spec[i].len && unit_first<ScatterView>(a, i) + b.eun[i] <= b.units);
    EXPECT(gather_final(term[i], spec[i].len, t.pow8) == crc32_bitwise(file + start[i], spec[i].len));
  }
  for (int k = 0; k < 3; k++) EXPECT(memcmp(ar[k].p, ar[k].want.data(), ar[k].size) == 0);
  for (uint64_t j = 0; j < 64; j++) EXPECT(file[j] == GUARD && file[flen + j] == GUARD);
  g_queries += n;
  g_segs += segs.size();
  g_units += b.units;
  for (int k = 0; k < 3; k++) free(ar[k].p);
  free(file);
}

static void check_random(const CrcTables& t, std::mt19937_64& rng) {
  std::vector<QuerySpec> spec;
  const uint64_t n = 1 + rng() % 10;
  for (uint64_t i = 0; i < n; i++) {
    QuerySpec q;
    const uint32_t kd = rng() % 10;
    q.kind = kd == 0 ? K_NONE : kd == 1 ? K_BAD_RANGE : kd == 2 ? K_SHORT : kd == 3 ? K_OVER : K_OK;
    q.res = -1;
    q.len = 0;
    const uint64_t k = 1 + rng() % 5;
    for (uint64_t j = 0; j < k; j++) {
      q.segs.push_back(SegSpec{pick_len(rng, C), -1});
      q.len += q.segs.back().len;
    }
    if (!q.len) { q.segs.back().len = 1 + rng() % 100; q.len = q.segs.back().len; }
    spec.push_back(q);
  }
  run_batch(t, rng, spec);
}

// all 256 (destination residue, source residue) pairs: one segment, and three
// whose boundaries fall around a unit boundary
static void check_residues(const CrcTables& t, std::mt19937_64& rng) {
  const uint64_t lens[] = {1, 15, 16, 17, 31, 32, 33, 200, 4095, 4096, 4097, C - 1, C, C + 1, C + 200};
  for (int dr = 0; dr < 16; dr++) {
    for (int sr = 0; sr < 16; sr++) {
      std::vector<QuerySpec> spec;
      for (uint64_t len : lens) spec.push_back(QuerySpec{K_OK, len, sr, {SegSpec{len, dr}}});
      // (the first segment ends one below / at / one behind the unit boundary of a destination at residue dr)
      for (int d = -1; d <= 1; d++) {
        const uint64_t l0 = C - dr + d;
        spec.push_back(QuerySpec{K_OK, l0 + C + 77, sr, {SegSpec{l0, dr}, SegSpec{0, -1}, SegSpec{C, (dr + 5) & 15}, SegSpec{77, -1}}});
      }
      run_batch(t, rng, spec);
    }
  }
}

static srd_segment seg(uint32_t src, uint64_t off, uint64_t len, uint32_t reserved = 0) {
  srd_segment g{};
  g.src = src;
  g.reserved = reserved;
  g.off = off;
  g.len = len;
  return g;
}

static const uint64_t F = 1ull << 40;  // check_refusals' file length
static void check_refusals() {
  // a table of three ranges (addresses are never dereferenced here): 1000 bytes, empty, everything
  const std::vector<uint64_t> tab = {0x10000, 1000, 0, 0, 0, M};
  struct Q { uint64_t s, e; };
  auto lay = [&](const std::vector<Q>& q, const std::vector<srd_segment>& segs, const std::vector<uint64_t>& first,
                 uint64_t flen = F) {
    std::vector<uint64_t> st, en;
    for (const Q& x : q) { st.push_back(x.s); en.push_back(x.e); }
    return device_layout(flen, st, en, segs, first, tab);
  };
  const Q hit{64, 84};  // 20 bytes
  const srd_segment ok = seg(0, 10, 20);
  EXPECT(lay({hit}, {ok}, {0, 1}).err == M && lay({hit}, {ok}, {0, 1}).st[0] == SRD_GATHER_OK);
  EXPECT(lay({hit}, {seg(0, 1000, 0), ok}, {0, 2}).st[0] == SRD_GATHER_OK);  // an empty range at the table range's end
  EXPECT(lay({hit}, {seg(0, 980, 20)}, {0, 1}).st[0] == SRD_GATHER_OK);
  // malformed segments
  auto bad = [&](const srd_segment& g) { return lay({hit}, {g}, {0, 1}).err == append_err_word(0, SEG_BAD_SEGMENT); };
  EXPECT(bad(seg(3, 0, 20)));                      // src >= n_dst
  EXPECT(bad(seg(0xFFFFFFFFu, 0, 20)));
  EXPECT(bad(seg(0, 10, 20, 1)));                  // reserved
  EXPECT(bad(seg(0, 981, 20)));                    // one byte past the table range
  EXPECT(bad(seg(0, 1001, 0)));
  EXPECT(bad(seg(1, 0, 1)));                       // an empty table range
  EXPECT(bad(seg(0, M, 1)));                       // off + len wraps to 0
  EXPECT(bad(seg(0, M - 7, 28)));                  // wraps into the range
  EXPECT(bad(seg(0, 8, M - 7)));                   // wraps to 0
  EXPECT(bad(seg(0, 100, M)));
  EXPECT(bad(seg(0, 1ull << 63, 1ull << 63)));
  EXPECT(bad(seg(2, 1, M)));                       // one past everything
  EXPECT(lay({hit}, {seg(2, M - 20, 20)}, {0, 1}).err == M);  // (the top of the address space is a range)
  // ... decide whatever the query's status would be: None, bad range, bad length
  EXPECT(lay({Q{5, 5}}, {seg(3, 0, 0)}, {0, 1}).err == append_err_word(0, SEG_BAD_SEGMENT));
  EXPECT(lay({Q{9, 5}}, {seg(0, 999, 2)}, {0, 1}).err == append_err_word(0, SEG_BAD_SEGMENT));
  EXPECT(lay({hit}, {seg(0, 0, 500), seg(0, 999, 2)}, {0, 2}).err == append_err_word(0, SEG_BAD_SEGMENT));
  {  // a refused query gets no units
    const Layout b = lay({hit, hit}, {seg(0, 0, 20), seg(0, 0, 10), seg(0, 999, 2), seg(0, 20, 10)}, {0, 1, 4});
    EXPECT(b.err == append_err_word(1, SEG_BAD_SEGMENT) && b.eun[1] == 0 && b.sun[1] == 0 && b.sun[3] == 0);
  }
  // d_seg_first
  EXPECT(lay({hit, hit}, {ok, ok}, {1, 2, 2}).err == append_err_word(0, SEG_BAD_FIRST));  // first[0] != 0
  EXPECT(lay({hit, hit, hit}, {ok, ok}, {0, 2, 1, 2}).err == append_err_word(1, SEG_BAD_FIRST));  // a decreasing pair
  EXPECT(lay({hit}, {ok, ok}, {0, 1}).err == append_err_word(0, SEG_BAD_FIRST));  // first[n] != n_segs
  EXPECT(lay({hit, hit}, {ok, ok}, {0, 1, 3}).err == append_err_word(1, SEG_BAD_FIRST));
  EXPECT(lay({hit, hit}, {ok, ok}, {0, M, 2}).err == append_err_word(0, SEG_BAD_FIRST));  // (never used as an index)
  EXPECT(lay({hit, hit}, {ok, ok}, {0, 1, M}).err == append_err_word(1, SEG_BAD_FIRST));
  // the first refused query decides, whatever the others are
  EXPECT(lay({hit, hit, hit, hit}, {ok, seg(5, 0, 1), seg(0, 0, 20, 7), ok}, {0, 1, 2, 3, 4}).err == append_err_word(1, SEG_BAD_SEGMENT));
  EXPECT(lay({hit, hit, hit}, {ok, ok, seg(5, 0, 1)}, {0, 1, 1, 3}).err == append_err_word(2, SEG_BAD_SEGMENT));
  EXPECT(lay({hit, hit, hit}, {ok, ok, seg(5, 0, 1)}, {0, 2, 1, 3}).err == append_err_word(1, SEG_BAD_FIRST));
  // the length: one short, one over, no segments, only empty ones; the range decides first
  auto st0 = [&](const Q& q, const std::vector<srd_segment>& segs, uint64_t flen = F) {
    const Layout b = lay({q}, segs, {0, segs.size()}, flen);
    EXPECT(b.err == M);
    if (b.st[0] != SRD_GATHER_OK) {
      EXPECT(b.eun[0] == 0 && b.units == 0);
      for (uint64_t v : b.sun) EXPECT(v == 0);
    }
    return (uint32_t)b.st[0];
  };
  EXPECT(st0(hit, {seg(0, 0, 19)}) == SCATTER_BAD_LENGTH);
  EXPECT(st0(hit, {seg(0, 0, 21)}) == SCATTER_BAD_LENGTH);
  EXPECT(st0(hit, {seg(0, 0, 10), seg(0, 10, 9)}) == SCATTER_BAD_LENGTH);
  EXPECT(st0(hit, {seg(0, 0, 10), seg(0, 10, 11)}) == SCATTER_BAD_LENGTH);
  EXPECT(st0(hit, {seg(0, 0, 10), seg(0, 10, 10)}) == SRD_GATHER_OK);
  EXPECT(st0(hit, {seg(0, 0, 10), seg(0, 10, 10), seg(0, 30, 1)}) == SCATTER_BAD_LENGTH);
  EXPECT(st0(hit, {seg(0, 0, 20), seg(0, 30, 0), seg(1, 0, 0)}) == SRD_GATHER_OK);
  EXPECT(st0(hit, {}) == SCATTER_BAD_LENGTH);
  EXPECT(st0(hit, {seg(0, 0, 0), seg(1, 0, 0)}) == SCATTER_BAD_LENGTH);
  EXPECT(st0(Q{7, 7}, {}) == SRD_GATHER_NONE);
  EXPECT(st0(Q{7, 7}, {seg(0, 0, 33)}) == SRD_GATHER_NONE);
  EXPECT(st0(Q{M, M}, {seg(0, 0, 33)}) == SRD_GATHER_NONE);
  EXPECT(st0(Q{9, 7}, {seg(0, 0, 33)}) == SRD_GATHER_BAD_RANGE);
  EXPECT(st0(Q{9, 7}, {seg(2, 0, M - 1)}) == SRD_GATHER_BAD_RANGE);  // (end - start wraps to M - 1: never a length)
  EXPECT(st0(Q{64, F - 19}, {seg(0, 0, 20)}) == SRD_GATHER_BAD_RANGE);
  EXPECT(st0(Q{64, M}, {seg(0, 0, 20)}) == SRD_GATHER_BAD_RANGE);
  EXPECT(st0(Q{F - 40, F - 20}, {seg(0, 0, 20)}) == SRD_GATHER_OK);
  // sums that would wrap 2^64
  EXPECT(st0(hit, {seg(2, 0, M), seg(2, 0, 21)}) == SCATTER_BAD_LENGTH);      // wraps to 20
  EXPECT(st0(hit, {seg(2, 5, M - 5), seg(2, 0, 26)}) == SCATTER_BAD_LENGTH);
  EXPECT(st0(hit, {seg(0, 0, 10), seg(2, 1, M - 1), seg(2, 0, 12)}) == SCATTER_BAD_LENGTH);
  EXPECT(st0(hit, {seg(2, 1, M - 1), seg(2, 1, M - 1), seg(2, 0, 24)}) == SCATTER_BAD_LENGTH);
  {  // a payload whose unit count the sum of 2^31 segments could not hold: capped, and the total refuses the call
    const uint64_t big = M - 100;
    const Layout b = lay({Q{0, big}}, {seg(2, 3, big)}, {0, 1}, M - 20);
    EXPECT(b.err == M && b.st[0] == SRD_GATHER_OK && b.sun[0] == SCATTER_UNITS_CAP && b.units >= (1ull << 32));
    // (fewer than 2^31 segments of at most 2^32 units each: the prefix sum stays below 2^63)
    const Layout c = lay({Q{0, (1ull << 32) * C - 3}}, {seg(2, 3, (1ull << 32) * C - 3)}, {0, 1}, M - 20);
    EXPECT(c.st[0] == SRD_GATHER_OK && c.units == (1ull << 32));  // (3 + len = 2^32 C: exactly the bound)
    const Layout d = lay({Q{0, ((1ull << 32) - 1) * C - 3}}, {seg(2, 3, ((1ull << 32) - 1) * C - 3)}, {0, 1}, M - 20);
    EXPECT(d.st[0] == SRD_GATHER_OK && d.units == (1ull << 32) - 1);  // (one below it)
    const Layout e = lay({Q{0, (1ull << 32) * C}}, {seg(2, 0, (1ull << 32) * C)}, {0, 1}, M - 20);
    EXPECT(e.st[0] == SRD_GATHER_OK && e.sun[0] == SCATTER_UNITS_CAP);
  }
  EXPECT(SCATTER_BAD_LENGTH == 4 && SRD_SCATTER_BAD_LENGTH == 4u);
}

int main() {
  static CrcTables t;
  build_crc_tables(t);
  EXPECT(crc32_bitwise((const uint8_t*)"123456789", 9) == 0xCBF43926u);
  std::mt19937_64 rng(0x5EED5CA7ull);
  for (int it = 0; it < 150; it++) check_random(t, rng);
  check_residues(t, rng);
  check_refusals();
  return check_done("scatter_check", "chunk %llu, %llu queries, %llu segments, %llu units, %llu vector pieces, %llu pieces byte by byte",
                    (unsigned long long)C, (unsigned long long)g_queries, (unsigned long long)g_segs, (unsigned long long)g_units,
                    (unsigned long long)g_vec, (unsigned long long)g_bytewise);
}
