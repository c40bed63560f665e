// What the stand-alone ASan/UBSan programs of this directory share (TEST
// INFRASTRUCTURE): the check macro and the common tail of main, a seeded
// generator, a model of the reference's append, the exact-size heap copy that
// turns a read past file_len into a sanitizer report, a bitwise CRC-32 and the
// segment length draw.  Nothing here knows the code under test.
#pragma once
#include <stdarg.h>
#include <stdint.h>
#include <stdio.h>
#include <string.h>

#include <memory>
#include <vector>

static uint64_t g_fail = 0, g_checks = 0;  // EXPECTs that failed / that were evaluated
#define EXPECT(c)                                                                              \
  do {                                                                                         \
    g_checks++;                                                                                \
    if (!(c)) {                                                                                \
      if (g_fail < 20) fprintf(stderr, "%s:%d: check failed: %s\n", __FILE__, __LINE__, #c);   \
      g_fail++;                                                                                \
    }                                                                                          \
  } while (0)

// The tail of every main: main's return value.  "NAME ok: M checks[, detail]"
// on stdout, or "NAME: N of M checks failed" on stderr.
__attribute__((format(printf, 2, 3))) static int check_done(const char* name, const char* detail_fmt, ...) {
  if (g_fail) {
    fprintf(stderr, "%s: %llu of %llu checks failed\n", name, (unsigned long long)g_fail, (unsigned long long)g_checks);
    return 1;
  }
  printf("%s ok: %llu checks", name, (unsigned long long)g_checks);
  if (detail_fmt) {
    va_list ap;
    va_start(ap, detail_fmt);
    printf(", ");
    vprintf(detail_fmt, ap);
    va_end(ap);
  }
  printf("\n");
  return 0;
}

struct SplitMix64 {
  uint64_t state;
  uint64_t operator()() {
    uint64_t z = (state += 0x9E3779B97F4A7C15ull);
    z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
    z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
    return z ^ (z >> 31);
  }
};

static inline void put64(std::vector<uint8_t>& f, uint64_t v) {
  for (int k = 0; k < 8; k++) f.push_back((uint8_t)(v >> (8 * k)));
}

// what the model knows about an entry it wrote
struct Ent {
  uint64_t kh, meta, start;  // key hash, metadata offset, payload start
  bool tomb;
};
// the reference's append (data_store.rs:864-914): prepad to 64 (none for a
// tombstone), payload, {key_hash, prev_offset = the tail before, crc}
struct Store {
  SplitMix64& rng;  // the program's generator
  std::vector<uint8_t> f;
  std::vector<Ent> ents;
  explicit Store(SplitMix64& r) : rng(r) {}
  void append(const std::vector<uint8_t>& payload, uint64_t kh, bool tomb) {
    const uint64_t tail = f.size();
    if (!tomb) f.resize(tail + ((64 - (tail & 63)) & 63), 0);
    const uint64_t st = f.size();
    f.insert(f.end(), payload.begin(), payload.end());
    const uint64_t meta = f.size();
    put64(f, kh);
    put64(f, tail);
    for (int k = 0; k < 4; k++) f.push_back((uint8_t)rng());  // (the rules read no checksum)
    ents.push_back(Ent{kh, meta, st, tomb});
  }
  void plain(uint64_t len, uint64_t kh) {  // len bytes, none of them zero
    std::vector<uint8_t> p;
    for (uint64_t i = 0; i < len; i++) p.push_back((uint8_t)(rng() | 1));
    append(p, kh, false);
  }
  void tombstone(uint64_t kh) { append({0}, kh, true); }
};

// fn(p) with p an exact-size heap copy of f[0 .. flen), nullptr for flen == 0:
// a read at flen or beyond, or below the buffer, is a heap overflow report
template <class Fn>
static auto with_exact_copy(const uint8_t* f, uint64_t flen, Fn&& fn) {
  std::unique_ptr<uint8_t[]> buf(new uint8_t[flen ? flen : 1]);
  if (flen) memcpy(buf.get(), f, flen);
  return fn(flen ? (const uint8_t*)buf.get() : nullptr);
}

// CRC-32 (IEEE, reflected) bit by bit; its user checks "123456789" -> 0xCBF43926
static inline uint32_t crc32_bitwise(const uint8_t* p, uint64_t n) {
  uint32_t c = 0xFFFFFFFFu;
  for (uint64_t i = 0; i < n; i++) {
    c ^= p[i];
    for (int k = 0; k < 8; k++) c = (c >> 1) ^ (0xEDB88320u & (0u - (c & 1)));
  }
  return ~c;
}

// a segment's length: empty, below and around 16 bytes, around one chunk C and
// around 4096, one or two chunks and a little, anything up to 9000
template <class Rng>
static uint64_t pick_len(Rng& rng, uint64_t C) {
  switch (rng() % 8) {
    case 0: return 0;
    case 1: return 1 + rng() % 17;
    case 2: return 15 + rng() % 3;
    case 3: return C - 16 + rng() % 33;
    case 4: return C * (1 + rng() % 2) + rng() % 40;
    case 5: return 4080 + rng() % 40;
    default: return 1 + rng() % 9000;
  }
}
