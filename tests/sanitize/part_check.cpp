// ASan/UBSan check of the scan's partition arithmetic (TEST INFRASTRUCTURE):
// rust-simd-r-drive_amd/csrc/srd_part.h compiled for the host, the very code
// the scan kernel, link2 and the host's workspace sizing run.  For seeded
// random (resident spans, grid, wave shares, block-start table):
//   - the wave ranges [r0, r1) in (block, wave) order tile [0, ns) exactly;
//   - part_span_wave(rel) is, for every rel < ns, the one wave holding rel;
//   - no wave holds more spans than part_max_wave_spans allows;
//   - part_table_ok accepts every table of the documented domain (drawn here
//     from all of it: empty blocks at 0 and g - 1, runs of empty blocks,
//     one-span blocks, blocks exactly at the bound) and refuses its borders.
// The wave shares are every share set of test_scan_wave_shares; the bound is
// the one the workspace is sized by; the tables' domain is the one
// srd_ctx_set_scan_blocks documents.
// Every valid table of the stores of up to 40 spans is enumerated.
// Exit status 0 = no sanitizer report and every invariant held.
#include <stdint.h>
#include <stdio.h>

#include <algorithm>
#include <cmath>
#include <random>
#include <vector>

#include "check.h"
#include "srd_part.h"

using namespace srd;

static uint64_t g_cases = 0, g_spans = 0;

// the library's grid for ns resident spans of a 16-wave variant on 256 CUs (scan_grid)
static uint32_t grid_of(uint64_t ns) { return (uint32_t)std::min<uint64_t>((ns + 15) / 16, 256); }

// relative weights -> shares of 65536 (weights_to_shares, srd_ctx.hip)
static void shares(const double (&f)[16], uint32_t (&wq)[16]) {
  double sum = 0;
  for (double x : f) sum += x;
  uint32_t used = 0;
  for (int v = 0; v < 15; v++) used += wq[v] = (uint32_t)(65536.0 * f[v] / sum);
  wq[15] = 65536 - used;
}
static std::vector<std::vector<uint32_t>> share_sets() {
  std::vector<std::vector<uint32_t>> out;
  auto add = [&](const double (&f)[16]) {
    uint32_t wq[16];
    shares(f, wq);
    out.emplace_back(wq, wq + 16);
  };
  const double dflt[16] = {1.0000, 0.9787, 0.9796, 0.9788, 0.9081, 0.9072, 0.9074, 0.8915,
                           0.8432, 0.8324, 0.8337, 0.8314, 0.7726, 0.7701, 0.7712, 0.7590};
  add(dflt);
  double f[16];
  for (int v = 0; v < 16; v++) f[v] = 1;
  add(f);  // "1,1,1,1"
  const double g4[4] = {3, 0.3, 1, 2};
  for (int v = 0; v < 16; v++) f[v] = g4[v / 4];
  add(f);
  std::mt19937_64 rng(7);
  std::uniform_real_distribution<double> u(0.3, 3.0);
  for (int v = 0; v < 16; v++) f[v] = u(rng);
  add(f);
  for (int v = 0; v < 16; v++) f[v] = v == 15 ? 8 : 1;
  add(f);
  return out;
}

static ScanPart make_part(uint64_t ns, uint32_t g, const std::vector<uint32_t>& wq, const uint64_t* bs) {
  ScanPart p{};
  p.s_lo = 3;  // (the arithmetic is resident-relative: unused)
  p.ns = ns;
  p.g = g;
  p.nw = 16;
  for (int v = 0; v < 16; v++) p.wq[v] = wq[v];
  part_fill_cw(p);
  p.bs = bs;
  return p;
}

static void check_part(uint64_t ns, uint32_t g, const std::vector<uint32_t>& wq, const std::vector<uint64_t>* table) {
  // a heap copy of exactly g + 1 starts so ASan sees a read past either end
  std::vector<uint64_t> bs;
  if (table) {
    bs.assign(table->begin(), table->end());
    bs.shrink_to_fit();
    EXPECT(bs.size() == (size_t)g + 1);
    EXPECT(part_table_ok(bs.data(), g, ns));
  }
  const ScanPart p = make_part(ns, g, wq, table ? bs.data() : nullptr);
  const uint64_t spw = part_max_wave_spans(p, table != nullptr);
  std::vector<uint32_t> owner(ns, ~0u);
  uint64_t at = 0;
  for (uint32_t b = 0; b < g; b++)
    for (uint32_t v = 0; v < 16; v++) {
      uint64_t r0 = 0, r1 = 0;
      part_wave_range(p, b, v, &r0, &r1);
      EXPECT(r0 == at);  // no gap, no overlap
      EXPECT(r1 >= r0 && r1 <= ns);
      EXPECT(r1 - r0 <= spw);
      for (uint64_t r = r0; r < r1 && r < ns; r++) owner[r] = b * 16 + v;
      at = r1;
    }
  EXPECT(at == ns);
  for (uint64_t rel = 0; rel < ns; rel++) {
    const uint64_t w = part_span_wave(p, rel);
    if (w != owner[rel]) {
      EXPECT(w == owner[rel]);
      if (g_fail <= 20) fprintf(stderr,"  ns %llu g %u table %d: span %llu -> wave %llu, its range is wave %u's\n",
              (unsigned long long)ns, g, table ? 1 : 0, (unsigned long long)rel, (unsigned long long)w, owner[rel]);
      break;
    }
  }
  g_cases++;
  g_spans += ns;
}

// block sizes -> starts, after moving every size into [0, bound] and the sum
// to ns (blocks visited in a seeded random order, so the features the caller
// placed mostly survive)
static std::vector<uint64_t> table_from_sizes(std::vector<uint64_t> sz, uint64_t ns, std::mt19937_64& rng) {
  const uint64_t g = sz.size(), bound = part_table_block_bound(ns, g);
  uint64_t sum = 0;
  for (auto& s : sz) { s = std::min(s, bound); sum += s; }
  std::vector<uint32_t> order(g);
  for (uint32_t b = 0; b < g; b++) order[b] = b;
  std::shuffle(order.begin(), order.end(), rng);
  for (int pass = 0; pass < 2 && sum != ns; pass++)  // pass 0 spares the empty and the full blocks
    for (uint32_t b : order) {
      if (sum == ns) break;
      if (!pass && (sz[b] == 0 || sz[b] == bound)) continue;
      if (sum < ns) { const uint64_t d = std::min(ns - sum, bound - sz[b]); sz[b] += d; sum += d; }
      else { const uint64_t d = std::min(sum - ns, sz[b]); sz[b] -= d; sum -= d; }
    }
  std::vector<uint64_t> st(g + 1, 0);
  for (uint64_t b = 0; b < g; b++) st[b + 1] = st[b] + sz[b];
  return st;
}

struct Seen { bool empty0, empty_last, empty_pair, one_span, at_bound; } g_seen{};
static void note(const std::vector<uint64_t>& st, uint64_t ns) {
  const uint64_t g = st.size() - 1, bound = part_table_block_bound(ns, g);
  for (uint64_t b = 0; b < g; b++) {
    const uint64_t n = st[b + 1] - st[b];
    if (!n && b == 0) g_seen.empty0 = true;
    if (!n && b == g - 1) g_seen.empty_last = true;
    if (!n && b + 1 < g && st[b + 2] == st[b + 1]) g_seen.empty_pair = true;
    if (n == 1) g_seen.one_span = true;
    if (n == bound) g_seen.at_bound = true;
  }
}

static std::vector<std::vector<uint64_t>> tables_for(uint64_t ns, uint32_t g, std::mt19937_64& rng) {
  std::vector<std::vector<uint64_t>> out;
  const uint64_t bound = part_table_block_bound(ns, g);
  std::vector<uint64_t> sz(g);
  {  // the even split as a table
    std::vector<uint64_t> st(g + 1);
    for (uint32_t b = 0; b <= g; b++) st[b] = (uint64_t)b * ns / g;
    out.push_back(st);
  }
  // the clamp extremes alternating with the XCD (b mod 8: odd / even), and their inverse
  for (int inv = 0; inv < 2; inv++) {
    for (uint32_t b = 0; b < g; b++) sz[b] = (uint64_t)((double)ns / g * (((b & 7 & 1) != (uint32_t)inv) ? 0.9 : 1.1));
    out.push_back(table_from_sizes(sz, ns, rng));
  }
  // full blocks from the left, the rest empty; and mirrored
  for (int mir = 0; mir < 2; mir++) {
    uint64_t left = ns;
    for (uint32_t i = 0; i < g; i++) {
      const uint64_t n = std::min(left, bound);
      sz[mir ? g - 1 - i : i] = n;
      left -= n;
    }
    out.push_back(table_from_sizes(sz, ns, rng));
  }
  // a sawtooth: empty, empty, bound, 1, bound, bound, 1, 0, ... with block 0 and g - 1 empty
  {
    const uint64_t pat[8] = {0, 0, bound, 1, bound, bound, 1, 0};
    for (uint32_t b = 0; b < g; b++) sz[b] = pat[b & 7];
    sz[g - 1] = 0;
    out.push_back(table_from_sizes(sz, ns, rng));
  }
  // random tables: sizes uniform in [0, bound], and sparse ones (mostly empty or full)
  for (int k = 0; k < 4; k++) {
    for (uint32_t b = 0; b < g; b++) {
      const uint64_t r = rng();
      sz[b] = k < 2 ? r % (bound + 1) : (r & 3) == 0 ? 0 : (r & 3) == 1 ? bound : (r & 3) == 2 ? 1 : (r >> 8) % (bound + 1);
    }
    out.push_back(table_from_sizes(sz, ns, rng));
  }
  return out;
}

// every valid table of g blocks over ns spans
static void enumerate(uint64_t ns, uint32_t g, const std::vector<std::vector<uint32_t>>& ws) {
  const uint64_t bound = part_table_block_bound(ns, g);
  std::vector<uint64_t> st(g + 1, 0);
  uint64_t n = 0;
  std::vector<uint32_t> stack;
  // depth-first over the block sizes
  struct Rec {
    static void go(uint32_t b, uint64_t ns, uint32_t g, uint64_t bound, std::vector<uint64_t>& st,
                   const std::vector<std::vector<uint32_t>>& ws, uint64_t& n) {
      if (b == g) {
        if (st[g] != ns) return;
        note(st, ns);
        check_part(ns, g, ws[n % ws.size()], &st);
        n++;
        return;
      }
      const uint64_t left = ns - st[b], after = (uint64_t)(g - b - 1) * bound;
      for (uint64_t s = left > after ? left - after : 0; s <= std::min(left, bound); s++) {
        st[b + 1] = st[b] + s;
        go(b + 1, ns, g, bound, st, ws, n);
      }
    }
  };
  Rec::go(0, ns, g, bound, st, ws, n);
  EXPECT(n >= 1);
}

static void check_domain_borders() {
  const uint64_t ns = 100;
  const uint32_t g = 7;
  const uint64_t bound = part_table_block_bound(ns, g);  // (500 + 27) / 28 + 1 = 19
  EXPECT(bound == 19);
  std::vector<uint64_t> ok = {0, 19, 19, 38, 39, 58, 81, 100};
  EXPECT(!part_table_ok(ok.data(), g, ns));  // 58 -> 81: 23 spans, above the bound
  ok = {0, 19, 19, 38, 57, 62, 81, 100};
  EXPECT(part_table_ok(ok.data(), g, ns));
  auto bad = ok;
  bad[0] = 1;
  EXPECT(!part_table_ok(bad.data(), g, ns));
  bad = ok;
  bad[g] = 99;
  EXPECT(!part_table_ok(bad.data(), g, ns));
  EXPECT(!part_table_ok(ok.data(), g, ns + 1));
  bad = ok;
  bad[4] = 37;  // decreasing
  EXPECT(!part_table_ok(bad.data(), g, ns));
  bad = ok;
  bad[5] = 57 + 20;  // one block one span above the bound
  EXPECT(!part_table_ok(bad.data(), g, ns));
  EXPECT(!part_table_ok(ok.data(), 0, ns));
  EXPECT(!part_table_ok(nullptr, g, ns));
  std::vector<uint64_t> big(XP_MAX_BLOCKS + 2, 0);
  big[XP_MAX_BLOCKS + 1] = 1;
  EXPECT(!part_table_ok(big.data(), XP_MAX_BLOCKS + 1, 1));
  big[XP_MAX_BLOCKS] = 1;
  EXPECT(part_table_ok(big.data(), XP_MAX_BLOCKS, 1));
}

int main() {
  const auto ws = share_sets();
  for (const auto& w : ws) {
    uint32_t s = 0;
    for (uint32_t x : w) s += x;
    EXPECT(s == 65536);
  }
  check_domain_borders();
  // every valid table of the smallest stores (1 to 3 blocks)
  for (uint64_t ns = 1; ns <= 40; ns++) enumerate(ns, grid_of(ns), ws);
  // seeded random stores, 1 .. ~20,000 spans: the sizes around the grid's steps and its cap, then a log-uniform draw
  std::mt19937_64 rng(0x5EED0005);
  std::vector<uint64_t> sizes = {1, 2, 15, 16, 17, 31, 32, 33, 255, 256, 257, 4079, 4080, 4081, 4095, 4096, 4097,
                                 4999, 12643, 19997, 20000};
  for (int k = 0; k < 60; k++) {
    const double e = std::uniform_real_distribution<double>(0.0, 1.0)(rng);
    sizes.push_back((uint64_t)std::max(1.0, std::exp(e * std::log(20000.0))));
  }
  uint64_t k = 0;
  for (uint64_t ns : sizes) {
    const uint32_t g = grid_of(ns);
    // no table: every share set
    for (const auto& w : ws) check_part(ns, g, w, nullptr);
    for (const auto& st : tables_for(ns, g, rng)) {
      note(st, ns);
      check_part(ns, g, ws[k++ % ws.size()], &st);
    }
  }
  EXPECT(g_seen.empty0 && g_seen.empty_last && g_seen.empty_pair && g_seen.one_span && g_seen.at_bound);
  return check_done("part_check", "%llu partitions, %llu spans inverted", (unsigned long long)g_cases,
                    (unsigned long long)g_spans);
}
