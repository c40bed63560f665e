// srd_api.hip -- the library's one translation unit: C ABI of include/srd_amd.h.
//
// A unity build (the device globals live in this TU); the Makefile,
// tools/isa_check.sh and `make variant` compile this file only.  File map:
//
//   device code
//     srd_crc.h, srd_xxh3.h   CRC algebra / tables, XXH3-64
//     srd_part.h              the scan's block / wave partition and its inverse (host code and a CPU check use it too)
//     srd_fin.h               the finalize rule: an entry's CRC from the scan's pieces, the byte-table multiply
//                             (both passes, the slow path, the writer, the host self-test and a CPU check)
//     srd_kernels.hip         scan, link, full-pass glue, finalize (one entry: finalize_in), slow path, batch digests, synth
//     srd_glue.hip            sync-free glue of the optimistic pass (shape test, entry pass), bucketed index, owner partition
//     srd_writer.hip          batch writer
//     srd_gather.h            the payload gather's range rule, chunk arithmetic, unit search and the powers of x a
//                             CRC is combined with (a CPU check uses it too)
//     srd_append.h            the device append's range rule, layout and refusals (a CPU check uses it too)
//     srd_segments.h          the segment append's table rule and unit cut; for every caller the unit descriptor, the
//                             batch cut into units (UnitArgs) under its three views, a unit's CRC term and the frame
//                             of the streaming kernel (a CPU check uses it too)
//     srd_scatter.h           the scatter read's entry walk: segments against the destination table, the length
//                             comparison, unit counts at the destination's residue (a CPU check uses it too)
//     srd_stream.hip          the streaming copy + CRC kernel, one wave per unit descriptor, for any source /
//                             destination alignment: the gather's, both appends' and the live compaction's
//                             (uses the writer's helpers)
//     srd_units.hip           the unit table and the CRC combine (terms, XOR) around the streaming kernel, for the
//                             same callers
//     srd_gather.hip          verified payloads: layout and finish around the unit kernels
//     srd_append.hip          payloads in HBM appended to a store: layout (its second half shared with the segment
//                             append's) and finish around the unit kernels
//     srd_segments.hip        entries made of device segments appended to a store: layout (around the unit kernels
//                             and the append's finish)
//     srd_scatter.hip         verified payloads read into device segments: layout and finish around the unit kernels
//     srd_table.h             the lookup table's rule: slot states, probe, claim, size arithmetic (the host entries
//                             and a CPU check use it too)
//     srd_ttl.h               the TTL cache's rule: the read's range rule (entry_range), the verdict on an indexed
//                             entry (ttl_judge), the expiry, eviction's choice among a batch (a CPU check uses it too)
//     srd_index.hip           lookup table build and reads, iterator, compaction
//     srd_index_live.hip      the table kept live: apply, export, batched delete; the live compaction's two steps
//     srd_ttl.hip             the TTL cache: namespaced key hash, the batched read's decision, the sweep
//     srd_rows.h              the rows read's rule: a looked-up entry's status, length and unit count (rows_judge),
//                             the unit bound that sizes grids and workspace, the host's refusals (a CPU check uses
//                             it too)
//     srd_rows.hip            keyed reads into fixed-size rows with no host wait: layout (look-up included) and
//                             finish around the unit kernels' device-count forms
//     srd_probe.hip           stream probe
//   host code (in include order: each file uses only the ones above it)
//     srd_host.cpp / .h       no-HIP parsers (shard cuts, batch layout)
//     srd_ctx.hip             errors, the launch check (LAUNCHED), context + workspace, table upload, the pinned
//                             read-back of small results (read_small), the hipCUB wrappers and their scratch,
//                             knobs, create / destroy, timing
//     srd_scan_host.hip       scan geometry, workspace and launch, load-pattern trial
//     srd_index_build.hip     bucketed / global index build, owner partition, their entries
//     srd_validate.hip        optimistic pass, full pass, finish; the two validate entries
//     srd_host_input.hip      staging, pinned host results, host-pointer entries
//     srd_multi.hip           multi-GPU open
//     srd_ops.hip             probe, batch digests, synth, writer, table / reads / maintenance, iterator,
//                             compaction, payload gather and scatter, device append, segment append, live
//                             compaction, TTL cache, rows read
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
#include "srd_gather.h"
#include "srd_append.h"
#include "srd_segments.h"
#include "srd_scatter.h"
#include "srd_stream.hip"
#include "srd_units.hip"
#include "srd_gather.hip"
#include "srd_append.hip"
#include "srd_segments.hip"
#include "srd_scatter.hip"
#include "srd_table.h"
#include "srd_ttl.h"
#include "srd_index.hip"
#include "srd_index_live.hip"
#include "srd_ttl.hip"
#include "srd_rows.h"
#include "srd_rows.hip"
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

// host self-test of the CRC algebra (no GPU): the tables and the combine the
// kernels run (srd_fin.h), against a byte-wise CRC on pseudo-random data.
// (tests/sanitize/fin_check.cpp sweeps the rule's every branch.)
extern "C" int srd_selftest_host(void) {
  const CrcTables& t = host_tabs();
  const FinTabs ft = fin_tabs_host(t);
  static uint8_t buf[5 * 4096];
  memset(buf, 0, sizeof buf);
  uint64_t z = 12345;
  for (int i = 0; i < 3 * 4096 + 200; i++) { auto& b = buf[i]; z = z * 6364136223846793005ull + 1442695040888963407ull; b = (uint8_t)(z >> 56); }
  // x^-8 * x^8 == 1
  if (mulp(t.invpow[1], t.pow8[0]) != kX0) return 1;
  auto raw = [&](uint64_t a, uint64_t b) { return host_crc_raw_bytes(t, 0, buf + a, b - a); };
  struct { uint32_t v[4]; uint32_t operator[](int i) const { return v[i]; } } tile[5];
  for (uint64_t k = 0; k < 5; k++)  // what the scan records per tile: lines 0..31, 1..31, 32..63
    tile[k] = {{raw(k * 4096, k * 4096 + 2048), raw(k * 4096 + 64, k * 4096 + 2048), raw(k * 4096 + 2048, k * 4096 + 4096), 0}};
  auto sx = [&](uint64_t o) { return raw(o & ~63ull, (o | 4095) + 1); };  // crc_raw(o's line .. its tile's end)
  const uint64_t cases[][2] = {{0, 100}, {64, 4096}, {128, 5000}, {4096, 8192 + 77}, {192, 12288 + 3}, {0, 63}};
  for (auto& cs : cases) {
    const uint64_t s = cs[0], m = cs[1];
    const uint32_t want = ~host_crc_raw_bytes(t, ~0u, buf + s, m - s), tail = raw(m & ~63ull, m);
    if (crc_from_pieces(s, m, sx(s), sx(m), tail, tile, ft) != want) return 2;
    if (crc_from_pieces4(s, m, sx(s), sx(m), tail, tile, tile[m / 4096], ft) != want) return 3;
  }
  return 0;
}
