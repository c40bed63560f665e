// ASan/UBSan check of the payload gather's arithmetic (TEST INFRASTRUCTURE):
// rust-simd-r-drive_amd/csrc/srd_gather.h (and srd_segments.h' unit cut and
// CRC term) compiled for the host, the very code the layout, unit-table and
// combine kernels run, over the tables of srd_crc.h.
//   - gather_range_status: the borders of NONE / BAD_RANGE / hit, without wrap;
//   - for seeded random batches (hits of 1 byte .. 5 chunks, None reads, bad
//     ranges, duplicates): the units tile every hit's bytes exactly once, every
//     unit finds its hit again (gather_unit_hit inverts the chunk prefix), and
//     the offsets -- the exclusive sum of the padded lengths -- give every
//     payload its own 64-aligned place;
//   - for the lengths of the GPU tests' set L and seeded random lengths up to
//     5 chunks, cut as a range is (chunks) and as a segment at destination
//     residue 5 is (unit 0 shorter than a chunk): the CRC combined from the
//     per-unit raw CRCs as the combine does it -- every unit's term
//     (seg_unit_term), XORed per lane over the units l, l + 64, ... and over
//     the lanes, then gather_final -- equals a byte-wise CRC-32, and the
//     lanes' shares partition the units.
// Exit status 0 = no sanitizer report and every invariant held.
#include <stdint.h>
#include <stdio.h>

#include <random>
#include <vector>

#include "check.h"
#include "srd_gather.h"
#include "srd_segments.h"

using namespace srd;

static const uint64_t C = GATHER_CHUNK;

static void check_status() {
  const uint64_t F = 100000;
  EXPECT(gather_range_status(0, 0, F) == SRD_GATHER_NONE);
  EXPECT(gather_range_status(777, 777, F) == SRD_GATHER_NONE);
  EXPECT(gather_range_status(~0ull, ~0ull, F) == SRD_GATHER_NONE);
  EXPECT(gather_range_status(64, 65, F) == SRD_GATHER_OK);
  EXPECT(gather_range_status(0, F - 20, F) == SRD_GATHER_OK);          // end + 20 == file_len
  EXPECT(gather_range_status(0, F - 19, F) == SRD_GATHER_BAD_RANGE);   // end + 20 == file_len + 1
  EXPECT(gather_range_status(65, 64, F) == SRD_GATHER_BAD_RANGE);      // start > end
  EXPECT(gather_range_status(0, F, F) == SRD_GATHER_BAD_RANGE);
  EXPECT(gather_range_status(0, 1ull << 63, F) == SRD_GATHER_BAD_RANGE);
  EXPECT(gather_range_status(0, ~0ull, F) == SRD_GATHER_BAD_RANGE);    // end + 20 would wrap
  EXPECT(gather_range_status(0, ~0ull - 19, F) == SRD_GATHER_BAD_RANGE);
  EXPECT(gather_range_status(0, 1, 20) == SRD_GATHER_BAD_RANGE);
  EXPECT(gather_range_status(0, 1, 21) == SRD_GATHER_OK);
  EXPECT(gather_range_status(0, 1, 0) == SRD_GATHER_BAD_RANGE);
}

static uint64_t g_units = 0, g_hits = 0;
static void check_batch(std::mt19937_64& rng) {
  const uint64_t F = 40 * C;
  const uint64_t n = 1 + rng() % 200;
  std::vector<uint64_t> st(n), en(n), plen(n + 1, 0), chk(n + 1, 0), off(n + 1), cpre(n + 1);
  std::vector<uint32_t> status(n);
  for (uint64_t i = 0; i < n; i++) {
    const uint32_t kind = rng() % 10;
    uint64_t len;
    switch (rng() % 5) {
      case 0: len = 1 + rng() % 200; break;
      case 1: len = 1 + rng() % (5 * C); break;
      case 2: len = C * (1 + rng() % 5); break;
      case 3: len = C * (1 + rng() % 4) + (rng() % 2 ? 1 : C - 1); break;
      default: len = 1 + rng() % 9000; break;
    }
    st[i] = (rng() % (F - 20 - len)) & (rng() % 4 ? ~63ull : ~0ull);
    en[i] = st[i] + len;
    if (kind == 0) en[i] = st[i];                       // a None read
    if (kind == 1) std::swap(st[i], en[i]);             // start > end
    if (kind == 2) en[i] = F - rng() % 20;              // metadata past the end
    if (kind == 3 && i) { st[i] = st[i - 1]; en[i] = en[i - 1]; }  // a duplicate
    status[i] = gather_range_status(st[i], en[i], F);
    const uint64_t l = status[i] == SRD_GATHER_OK ? en[i] - st[i] : 0;
    plen[i] = gather_pad64(l);
    chk[i] = gather_chunks(l);
    EXPECT(plen[i] % 64 == 0 && plen[i] >= l && plen[i] < l + 64);
    EXPECT((chk[i] == 0) == (l == 0) && (chk[i] ? (chk[i] - 1) * C < l && l <= chk[i] * C : true));
  }
  uint64_t so = 0, sc = 0;
  for (uint64_t i = 0; i <= n; i++) {  // what the two exclusive sums give
    off[i] = so;
    cpre[i] = sc;
    so += plen[i];
    sc += chk[i];
  }
  // every payload its own 64-aligned place below the total
  for (uint64_t i = 0; i < n; i++) {
    EXPECT(off[i] % 64 == 0 && off[i + 1] - off[i] == plen[i] && off[i] + plen[i] <= off[n]);
  }
  // the units tile every hit once; unit -> hit inverts the prefix
  const uint64_t U = cpre[n];
  std::vector<uint64_t> covered(n, 0), seen(n, 0);
  for (uint64_t u = 0; u < U; u++) {
    const uint64_t i = gather_unit_hit(cpre.data(), n, u);
    EXPECT(i < n && cpre[i] <= u && u < cpre[i + 1]);
    if (!(i < n)) continue;
    EXPECT(status[i] == SRD_GATHER_OK);
    const uint64_t c = u - cpre[i], l = en[i] - st[i];
    EXPECT(c == seen[i]);  // a hit's chunks are consecutive units in order
    seen[i]++;
    const uint64_t cl = gather_chunk_len(l, c);
    EXPECT(cl >= 1 && cl <= C && c * C + cl <= l && c * C == covered[i]);
    EXPECT((cl < C) ? c * C + cl == l : true);
    covered[i] += cl;
  }
  for (uint64_t i = 0; i < n; i++) {
    EXPECT(seen[i] == chk[i]);
    EXPECT(covered[i] == (status[i] == SRD_GATHER_OK ? en[i] - st[i] : 0));
    g_hits += status[i] == SRD_GATHER_OK;
  }
  g_units += U;
}

// the entry buf[s, s + len) at destination residue a (seg_unit_range's cut; a
// == 0: the chunk cut of a range), combined as unit_terms_kernel and
// unit_combine_kernel do it
static uint64_t g_crcs = 0;
static void check_crc(const CrcTables& t, const std::vector<uint8_t>& buf, uint64_t s, uint64_t len, uint64_t a = 0) {
  const uint8_t* p = buf.data() + s;
  const uint32_t want = ~host_crc_raw_bytes(t, 0xFFFFFFFFu, p, len);
  const uint64_t k = seg_unit_count(a, len);
  if (!a) EXPECT(k == gather_chunks(len));
  std::vector<uint32_t> term(k);
  uint64_t at = 0;
  for (uint64_t j = 0; j < k; j++) {
    uint64_t b0, b1;
    seg_unit_range(a, len, j, &b0, &b1);
    EXPECT(b0 == at && b1 > b0 && b1 - b0 <= C && b1 == (len < (j + 1) * C - a ? len : (j + 1) * C - a));
    if (!a) EXPECT(b0 == j * C && b1 - b0 == gather_chunk_len(len, j));
    at = b1;
    term[j] = seg_unit_term(host_crc_raw_bytes(t, 0, p + b0, b1 - b0), len, b1, t.pow8);
  }
  EXPECT(at == len);
  uint32_t x = 0;
  std::vector<uint8_t> taken(k, 0);
  for (uint64_t l = 0; l < 64; l++) {  // lane l: the units l, l + 64, ...
    uint32_t tl = 0;
    for (uint64_t j = l; j < k; j += 64) {
      tl ^= term[j];
      taken[j]++;
    }
    x ^= tl;
  }
  for (uint64_t j = 0; j < k; j++) EXPECT(taken[j] == 1);  // the lanes' shares partition 0 .. k
  EXPECT(gather_final(x, len, t.pow8) == want);
  g_crcs++;
}
// ... on both cuts
static void check_crc2(const CrcTables& t, const std::vector<uint8_t>& buf, uint64_t s, uint64_t len) {
  check_crc(t, buf, s, len);
  check_crc(t, buf, s, len, 5);
}

int main() {
  static CrcTables t;
  build_crc_tables(t);
  check_status();
  std::mt19937_64 rng(0x5EED6A7Eull);
  for (int it = 0; it < 300; it++) check_batch(rng);
  // the GPU tests' length set L
  const uint64_t L[] = {1, 2, 15, 16, 17, 63, 64, 65, 1023, 1024, 1025, 1040, 4095, 4096, 4097, 8191, 8192, 8193, 12289,
                        C - 1, C, C + 1, 2 * C, 2 * C + 17, 3 * C + 4097};
  std::vector<uint8_t> buf(5 * C + 4096);
  for (auto& b : buf) b = (uint8_t)rng();
  for (uint64_t len : L) check_crc2(t, buf, 0, len);
  for (int it = 0; it < 40; it++) {
    const uint64_t len = 1 + rng() % (5 * C);
    check_crc2(t, buf, rng() % (buf.size() - len + 1), len);
  }
  // many units: lanes with one, two and three units
  {
    std::vector<uint8_t> big(131 * C + 77);
    for (auto& b : big) b = (uint8_t)rng();
    check_crc2(t, big, 0, big.size());
    check_crc2(t, big, 0, 64 * C);
    check_crc2(t, big, 0, 65 * C + 1);
  }
  return check_done("gather_check", "chunk %llu, %llu hits, %llu units, %llu CRCs", (unsigned long long)C,
                    (unsigned long long)g_hits, (unsigned long long)g_units, (unsigned long long)g_crcs);
}
