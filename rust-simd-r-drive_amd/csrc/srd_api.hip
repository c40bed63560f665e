// srd_api.hip -- the library's one translation unit: C ABI of include/srd_amd.h.
//
// A unity build (the device globals live in this TU); the Makefile,
// tools/isa_check.sh and `make variant` compile this file only.  File map:
//
//   device code
//     srd_crc.h, srd_xxh3.h   CRC algebra / tables, XXH3-64
//     srd_part.h              the scan's block / wave partition and its inverse (host code and a CPU check use it too)
//     srd_kernels.hip         scan, link, full-pass glue, finalize, batch digests, synth
//     srd_glue.hip            sync-free glue of the optimistic pass, bucketed index, owner partition
//     srd_writer.hip          batch writer
//     srd_index.hip           lookup table, batched reads, iterator, compaction
//     srd_index_live.hip      the table kept live: apply, export, batched delete
//     srd_probe.hip           stream probe
//   host code (in include order: each file uses only the ones above it)
//     srd_host.cpp / .h       no-HIP parsers (shard cuts, batch layout)
//     srd_ctx.hip             errors, context + workspace, table upload, knobs, create / destroy, timing
//     srd_scan_host.hip       scan geometry, workspace and launch, load-pattern trial
//     srd_index_build.hip     bucketed / global index build, owner partition, their entries
//     srd_validate.hip        optimistic pass, full pass, finish; the two validate entries
//     srd_host_input.hip      staging, pinned host results, host-pointer entries
//     srd_multi.hip           multi-GPU open
//     srd_ops.hip             probe, batch digests, synth, writer, table / reads / maintenance, iterator,
//                             compaction
//   this file               error / build-info entries, stamps read-outs, host self-test
//
// Glue scans/compactions use hipCUB (library primitives, like calling
// rocBLAS for a plain GEMM); every byte-touching hot kernel is hand-written.
#include <hip/hip_ext.h>
#include <hip/hip_runtime.h>
#include <hipcub/hipcub.hpp>

#include <algorithm>
#include <atomic>
#include <chrono>
#include <cmath>
#include <condition_variable>
#include <cstdio>
#include <functional>
#include <cstdlib>
#include <cstring>
#include <mutex>
#include <string>
#include <thread>
#include <vector>

#include "srd_amd.h"
#include "srd_host.cpp"
#include "srd_kernels.hip"
#include "srd_glue.hip"
#include "srd_writer.hip"
#include "srd_index.hip"
#include "srd_index_live.hip"
#include "srd_probe.hip"

using namespace srd;

#include "srd_ctx.hip"
#include "srd_scan_host.hip"
#include "srd_index_build.hip"
#include "srd_validate.hip"
#include "srd_host_input.hip"
#include "srd_multi.hip"
#include "srd_ops.hip"

extern "C" const char* srd_last_error(void) { return g_err.c_str(); }
#ifndef SRD_SOURCE_HASH
#define SRD_SOURCE_HASH "unknown"  // (built without the Makefile)
#endif
extern "C" const char* srd_build_info(void) { return SRD_SOURCE_HASH; }

#ifdef SRD_GLUE_STAMPS
// timing-only build: the last fused chain_finalize's per-block phase stamps
extern "C" int srd_debug_glue_stamps(uint64_t* out) {
  HIPCHK(hipDeviceSynchronize());
  HIPCHK(hipMemcpyFromSymbol(out, HIP_SYMBOL(g_glue_stamp), sizeof(uint64_t) * CHAIN_BLOCKS * 8));
  return 0;
}
#endif
#ifdef SRD_WAVE_STAMPS
// timing-only build: the last scan's per-wave end stamps and per-block start
// stamps (s_memrealtime, 100 MHz)
extern "C" int srd_debug_wave_stamps(uint64_t* out) {
  HIPCHK(hipDeviceSynchronize());
  HIPCHK(hipMemcpyFromSymbol(out, HIP_SYMBOL(g_wave_stamp), sizeof(uint64_t) * (8192 + 1024)));
  return 0;
}
// and the shader-clock counter (s_memtime) at the same wave ends / block starts
extern "C" int srd_debug_wave_clk(uint64_t* out) {
  HIPCHK(hipDeviceSynchronize());
  HIPCHK(hipMemcpyFromSymbol(out, HIP_SYMBOL(g_wave_clk), sizeof(uint64_t) * (4096 + 256)));
  return 0;
}
#endif

// host self-test of the CRC algebra (no GPU): checks the tables against a
// byte-wise CRC on pseudo-random data with the same combine the kernels use.
extern "C" int srd_selftest_host(void) {
  const CrcTables& t = host_tabs();
  static uint8_t buf[5 * 4096];
  memset(buf, 0, sizeof buf);
  uint64_t z = 12345;
  for (int i = 0; i < 3 * 4096 + 200; i++) { auto& b = buf[i]; z = z * 6364136223846793005ull + 1442695040888963407ull; b = (uint8_t)(z >> 56); }
  // x^-8 * x^8 == 1
  if (mulp(t.invpow[1], t.pow8[0]) != kX0) return 1;
  // check crc_from_pieces-style assembly for several (s, m)
  auto raw = [&](uint64_t a, uint64_t b) { return host_crc_raw_bytes(t, 0, buf + a, b - a); };
  auto crc32 = [&](uint64_t a, uint64_t b) { return ~host_crc_raw_bytes(t, ~0u, buf + a, b - a); };
  auto sx = [&](uint64_t k, uint32_t j) {  // crc_raw(lines j..63 of tile k)
    return raw(k * 4096 + 64 * j, k * 4096 + 4096);
  };
  const uint64_t cases[][2] = {{0, 100}, {64, 4096}, {128, 5000}, {4096, 8192 + 77}, {192, 12288 + 3}, {0, 63}};
  for (auto& cs : cases) {
    uint64_t s = cs[0], m = cs[1];
    uint64_t len = m - s;
    uint32_t want = crc32(s, m);
    uint32_t tail = raw(m & ~63ull, m);
    uint32_t got;
    if (len < 64) {
      got = tail ^ t.zero_crc[len];
    } else {
      uint64_t k0 = s / 4096, k1 = m / 4096;
      uint32_t acc = sx(k0, (uint32_t)((s % 4096) / 64)) ^ t.winit[(s % 4096) / 64];
      uint32_t sxm = sx(k1, (uint32_t)((m % 4096) / 64));
      uint32_t y;
      if (k0 == k1) y = acc ^ sxm;
      else {
        for (uint64_t k = k0 + 1; k < k1; k++) acc = mulp(t.x32768, acc) ^ sx(k, 0);
        y = mulp(t.x32768, acc) ^ sx(k1, 0) ^ sxm;
      }
      got = ~(mulp(t.invpow[(k1 + 1) * 4096 - m], y) ^ tail);
    }
    if (got != want) return 2;
  }
  return 0;
}
