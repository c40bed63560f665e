// ASan/UBSan check of the device append's arithmetic (TEST INFRASTRUCTURE):
// rust-simd-r-drive_amd/csrc/srd_append.h compiled for the host, the very code
// the layout / finish kernels and the host glue of srd_batch_append_device run,
// with srd_gather.h's unit arithmetic under it.
//   - append_range_status: zero lengths, ranges outside the blob (wrap-around
//     values near 2^64 included), the borders of a blob, a length of 2^48;
//   - for seeded random length vectors and every start tail residue 0..63: the
//     layout by one exclusive sum (payload starts, metadata offsets,
//     prev_offsets, the new tail) equals srd_batch_layout's (srd_host.cpp);
//   - the first refused entry decides (the error word's minimum);
//   - the 2^48 bound: the last tail below it is accepted, the first at it is
//     refused, and a batch whose exact sum wraps 2^64 is refused by its coarse sum;
//   - the units tile every entry exactly once, every unit finds its entry
//     again, and every unit's destination is 64-aligned inside its payload.
// Exit status 0 = no sanitizer report and every invariant held.
#include <stdint.h>
#include <stdio.h>

#include <random>
#include <vector>

#include "check.h"
#include "srd_append.h"
#include "srd_host.h"

using namespace srd;

static const uint64_t C = GATHER_CHUNK;
static const uint64_t M = ~0ull;

static void check_status() {
  const uint64_t B = 100000;
  EXPECT(append_range_status(0, 0, B) == APPEND_EMPTY);
  EXPECT(append_range_status(B + 5, 0, B) == APPEND_EMPTY);  // (the reference tests the length first)
  EXPECT(append_range_status(M, 0, B) == APPEND_EMPTY);
  EXPECT(append_range_status(0, 1, B) == APPEND_OK);
  EXPECT(append_range_status(0, B, B) == APPEND_OK);
  EXPECT(append_range_status(B - 1, 1, B) == APPEND_OK);
  EXPECT(append_range_status(B - 1, 2, B) == APPEND_BAD_RANGE);  // ends one byte past the blob
  EXPECT(append_range_status(0, B + 1, B) == APPEND_BAD_RANGE);
  EXPECT(append_range_status(B, 1, B) == APPEND_BAD_RANGE);
  EXPECT(append_range_status(B + 1, 1, B) == APPEND_BAD_RANGE);
  EXPECT(append_range_status(M, 1, B) == APPEND_BAD_RANGE);       // off + len wraps to 0
  EXPECT(append_range_status(M - 7, 8, B) == APPEND_BAD_RANGE);   // wraps to 0
  EXPECT(append_range_status(M - 7, 108, B) == APPEND_BAD_RANGE); // wraps into the blob
  EXPECT(append_range_status(8, M - 7, B) == APPEND_BAD_RANGE);   // wraps to 0
  EXPECT(append_range_status(100, M, B) == APPEND_BAD_RANGE);     // wraps to 99
  EXPECT(append_range_status(M, M, B) == APPEND_BAD_RANGE);
  EXPECT(append_range_status(1ull << 63, 1ull << 63, B) == APPEND_BAD_RANGE);
  EXPECT(append_range_status(0, 1, 0) == APPEND_BAD_RANGE);
  EXPECT(append_range_status(0, 0, 0) == APPEND_EMPTY);
  // an entry that alone passes the 48-bit offset space (a blob that large is arithmetic only)
  EXPECT(append_range_status(0, APPEND_TAIL_LIMIT - 1, M) == APPEND_OK);
  EXPECT(append_range_status(0, APPEND_TAIL_LIMIT, M) == APPEND_TOO_LONG);
  EXPECT(append_range_status(5, M - 5, M) == APPEND_TOO_LONG);
  EXPECT(append_range_status(5, M - 4, M) == APPEND_BAD_RANGE);
}

// what the device computes for a batch: statuses, the error word, the two
// exclusive sums, the coarse sum, the new tail
struct Batch {
  std::vector<uint64_t> slot, chk, pre, cpre;
  uint64_t err = M, coarse = 0, new_tail = 0;
  bool tail_ok = false;
};
static Batch device_layout(uint64_t tail, const std::vector<uint64_t>& off, const std::vector<uint64_t>& len,
                           uint64_t blob_len) {
  const uint64_t n = len.size();
  Batch b;
  b.slot.assign(n, 0);
  b.chk.assign(n, 0);
  b.pre.assign(n + 1, 0);
  b.cpre.assign(n + 1, 0);
  for (uint64_t i = n; i-- > 0;) {  // (any order: the minimum decides)
    const uint32_t st = append_range_status(off[i], len[i], blob_len);
    if (st != APPEND_OK) {
      const uint64_t w = append_err_word(i, st);
      if (w < b.err) b.err = w;
      continue;
    }
    b.slot[i] = append_slot(len[i]);
    b.chk[i] = gather_chunks(len[i]);
    b.coarse += append_coarse(b.slot[i]);
  }
  for (uint64_t i = 0; i < n; i++) {
    b.pre[i + 1] = b.pre[i] + b.slot[i];  // (may wrap: unsigned, as on the device)
    b.cpre[i + 1] = b.cpre[i] + b.chk[i];
  }
  if (n) b.tail_ok = append_new_tail(tail, b.coarse, b.pre[n - 1], len[n - 1], &b.new_tail);
  return b;
}

static uint64_t g_entries = 0, g_units = 0;
static void check_layout(std::mt19937_64& rng, uint64_t tail) {
  const uint64_t n = 1 + rng() % 60;
  std::vector<uint64_t> off(n), len(n), zero(n, 0);
  const uint64_t blob = 8 * C;
  for (uint64_t i = 0; i < n; i++) {
    switch (rng() % 6) {
      case 0: len[i] = 1 + rng() % 130; break;
      case 1: len[i] = 44 + 64 * (rng() % 4); break;  // len + 20 a multiple of 64
      case 2: len[i] = 43 + 64 * (rng() % 4) + 2 * (rng() % 2); break;
      case 3: len[i] = C * (1 + rng() % 3) + (rng() % 3) - 1; break;
      case 4: len[i] = 1 + rng() % (4 * C); break;
      default: len[i] = 1 + rng() % 9000; break;
    }
    off[i] = rng() % (blob - len[i] + 1);
  }
  const Batch b = device_layout(tail, off, len, blob);
  EXPECT(b.err == M && b.tail_ok);
  std::vector<srd_write_entry> E(n);
  uint64_t want_tail = 0;
  const char* why = "";
  EXPECT(srd_host::batch_layout(tail, nullptr, zero.data(), zero.data(), off.data(), len.data(), n, 0, E.data(),
                                &want_tail, &why) == 0);
  const uint64_t base = append_base(tail);
  EXPECT(base % 64 == 0 && base >= tail && base - tail < 64);
  for (uint64_t i = 0; i < n; i++) {
    const uint64_t P = append_payload(base, b.pre[i]), m = append_meta(base, b.pre[i], len[i]);
    const uint64_t prev = i ? append_meta(base, b.pre[i - 1], len[i - 1]) + 20 : tail;
    EXPECT(prev == E[i].tail);                                   // prev_offset
    EXPECT(P == E[i].tail + ((64 - E[i].tail % 64) & 63));        // the payload behind its prepad
    EXPECT(P % 64 == 0 && m == P + len[i]);
    if (i + 1 < n) EXPECT(append_payload(base, b.pre[i + 1]) == gather_pad64(m + 20));
  }
  EXPECT(b.new_tail == want_tail);
  // the units tile every entry once; unit -> entry inverts the prefix; destinations 64-aligned
  const uint64_t U = b.cpre[n];
  std::vector<uint64_t> covered(n, 0), seen(n, 0);
  for (uint64_t u = 0; u < U; u++) {
    const uint64_t i = gather_unit_hit(b.cpre.data(), n, u);
    EXPECT(i < n && b.cpre[i] <= u && u < b.cpre[i + 1]);
    if (!(i < n)) continue;
    const uint64_t c = u - b.cpre[i];
    EXPECT(c == seen[i]);
    seen[i]++;
    const uint64_t cl = gather_chunk_len(len[i], c);
    const uint64_t dst = append_payload(base, b.pre[i]) + c * C;
    EXPECT(dst % 64 == 0 && cl >= 1 && cl <= C && c * C == covered[i]);
    EXPECT(dst + cl <= append_meta(base, b.pre[i], len[i]));
    EXPECT((cl < C) ? c * C + cl == len[i] : true);
    covered[i] += cl;
  }
  for (uint64_t i = 0; i < n; i++) EXPECT(seen[i] == b.chk[i] && covered[i] == len[i]);
  g_entries += n;
  g_units += U;
}

static void check_refusals() {
  const uint64_t blob = 1000;
  {  // the first refused entry decides, whatever the others are
    const std::vector<uint64_t> off = {0, 10, 990, M - 3, 0}, len = {5, 0, 11, 8, 0};
    const Batch b = device_layout(100, off, len, blob);
    EXPECT(b.err == append_err_word(1, APPEND_EMPTY) && append_err_status(b.err) == APPEND_EMPTY);
    const std::vector<uint64_t> off2 = {0, 990, 10, 0}, len2 = {5, 11, 0, 7};
    const Batch b2 = device_layout(100, off2, len2, blob);
    EXPECT((b2.err >> 8) == 1 && append_err_status(b2.err) == APPEND_BAD_RANGE);
  }
  {  // the 2^48 bound on the new tail: nt = base + len + 20
    const uint64_t L = APPEND_TAIL_LIMIT;
    for (uint64_t tail : {0ull, 1ull, 63ull, 64ull, 4097ull}) {
      const uint64_t base = append_base(tail);
      const std::vector<uint64_t> off = {0};
      const Batch ok = device_layout(tail, off, {L - 1 - 20 - base}, M);
      EXPECT(ok.err == M && ok.tail_ok && ok.new_tail == L - 1);
      const Batch no = device_layout(tail, off, {L - 20 - base}, M);
      EXPECT(no.err == M && !no.tail_ok);
    }
    // a tail that is itself at the bound
    EXPECT(!device_layout(L, {0}, {1}, M).tail_ok);
    EXPECT(device_layout(L - 22, {0}, {1}, M).tail_ok == (append_base(L - 22) + 21 < L));
    // two entries crossing it together
    const Batch two = device_layout(0, {0, 0}, {L / 2, L / 2}, M);
    EXPECT(two.err == M && !two.tail_ok);
    // the exact sum wraps 2^64 (2^17 slots of 2^47 bytes): the coarse sum refuses
    const uint64_t n = 1ull << 17;
    std::vector<uint64_t> off(n, 0), len(n, (1ull << 47) - 20);
    const Batch wrap = device_layout(0, off, len, M);
    EXPECT(wrap.err == M && wrap.pre[n] == 0 && !append_sum_exact(wrap.coarse) && !wrap.tail_ok);
    // ... and with one entry more the wrapped sum looks small: still refused
    off.push_back(0);
    len.push_back(100);
    EXPECT(!device_layout(0, off, len, M).tail_ok);
  }
}

int main() {
  check_status();
  std::mt19937_64 rng(0x5EEDA99Eull);
  for (uint64_t res = 0; res < 64; res++)
    for (int it = 0; it < 6; it++) check_layout(rng, (rng() % 5000) * 64 + res);
  for (uint64_t res = 0; res < 64; res++) check_layout(rng, res);  // (a store of less than one line)
  check_refusals();
  return check_done("append_check", "chunk %llu, %llu entries, %llu units", (unsigned long long)C,
                    (unsigned long long)g_entries, (unsigned long long)g_units);
}
