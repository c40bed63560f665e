// srd_gather.hip -- verified payloads: the batched gather with checksum check
// (srd_payload_gather_device; host glue in srd_ops.hip).
//
// Reference being replaced (jzombie/rust-simd-r-drive v0.16.3-alpha): what a
// reader does with the handles of a batch read --
//   EntryHandle::as_slice / is_valid_checksum
//                       simd-r-drive-entry-handle/src/entry_handle.rs:260-275
//   compute_checksum    src/storage_engine/digest/compute_checksum.rs:15-20
//
// The read-side mirror of write_kernel: the payloads of a batch of ranges are
// copied out of the store into one packed buffer (each at a 64-byte boundary)
// while their CRC-32 is computed from the same registers and compared with the
// checksum stored in the entry's metadata.  The writer gives a whole entry to
// one wave; a read batch is often a few large payloads, so here the unit of
// work is one CHUNK of one hit (SRD_GATHER_CHUNK bytes, the last chunk of a
// hit shorter; srd_gather.h) and the rate does not depend on how the bytes are
// distributed over the hits.  Steps, all on the caller's stream:
//   payload_layout_kernel   per query: status by arithmetic, padded length,
//                           chunk count (then two hipCUB exclusive sums)
//   payload_units_kernel    the unit table: per chunk its descriptor (SegUnit)
//   stream_copy_crc_kernel  one wave per unit: copy + raw CRC of the chunk (a
//                           single-unit hit's CRC is finished here; srd_stream.hip)
//   payload_combine_kernel  one wave per multi-unit hit: folds its chunks' CRCs
//   payload_finish_kernel   per query: stored checksum, status, the caller's arrays
// srd_batch_append_device (srd_append.hip) cuts its payloads into the same
// units (PayloadRanges) and folds them with the same combine.

namespace srd {

// A batch of ranges cut into chunk units: what the unit table and the combine
// need of it, whoever laid it out (the gather's hits, the append's payloads)
struct PayloadRanges {
  const uint8_t* file;          // the bytes the ranges index
  const uint64_t *start, *end;  // the ranges [n]
  uint64_t n;
  uint64_t* chk;   // [n] chunk count
  uint64_t* off;   // [n] the output offsets less dst0, multiples of 64
  uint64_t* cpre;  // [n] exclusive sum of chk
  uint64_t dst0;   // a multiple of 64
  bool pad;        // a range's last unit zeroes up to the next 64-byte boundary of the output
  SegUnit* unit;   // [n_units] the unit table
  uint64_t n_units;
  uint32_t* raw;   // [n_units] a multi-unit range's chunks: crc_raw
  uint32_t* crc;   // [n] a range's CRC32
};

struct PayloadGatherArgs : PayloadRanges {  // (off = the exclusive sum of plen)
  uint64_t flen;
  uint8_t* st;     // [n] gather_range_status
  uint64_t* plen;  // [n] padded length (0 for no hit)
  uint64_t total;  // off[n - 1] + plen[n - 1] (known after the host's wait)
  unsigned long long* cnt;  // [0] the hits of more than one chunk
  // the caller's arrays (payload_finish_kernel)
  uint64_t* o_off;
  uint8_t* o_status;
  uint32_t* o_crc;
  uint32_t layout_only;
};

__global__ __launch_bounds__(256) void payload_layout_kernel(PayloadGatherArgs a) {
  for (uint64_t i = blockIdx.x * 256ull + threadIdx.x; i < a.n; i += gridDim.x * 256ull) {
    const uint64_t s = a.start[i], e = a.end[i];
    const uint32_t st = gather_range_status(s, e, a.flen);
    const uint64_t len = st == SRD_GATHER_OK ? e - s : 0;
    a.st[i] = (uint8_t)st;
    const uint64_t k = gather_chunks(len);
    a.plen[i] = gather_pad64(len);
    a.chk[i] = k;
    const uint64_t m = __ballot(k > 1);
    if (m && (threadIdx.x & 63) == (uint32_t)__builtin_ctzll(m)) atomicAdd(a.cnt, (unsigned long long)__builtin_popcountll(m));
  }
}

// unit u: chunk u - cpre[i] of the range i with cpre[i] <= u < cpre[i + 1]
__global__ __launch_bounds__(256) void payload_units_kernel(PayloadRanges a) {
  for (uint64_t u = blockIdx.x * 256ull + threadIdx.x; u < a.n_units; u += gridDim.x * 256ull) {
    const uint64_t i = gather_unit_hit(a.cpre, a.n, u), s = a.start[i];
    a.unit[u] = seg_chunk_unit((uint64_t)(uintptr_t)a.file + s, a.dst0 + a.off[i], a.end[i] - s, u - a.cpre[i], (uint32_t)i,
                               a.chk[i], a.pad);
  }
}

// One wave per hit of more than one chunk: lane l folds the raw CRCs of its
// share of the chunks (gather_lane_term: Horner by x^(8 chunk), moved up by
// the bytes behind the share), the XOR over the lanes is crc_raw(hit), and the
// length-dependent init / xorout fix makes it the CRC32.
__global__ __launch_bounds__(256) void payload_combine_kernel(PayloadRanges a) {
  const uint32_t lane = threadIdx.x & 63;
  const uint64_t W = gridDim.x * 4ull;
  for (uint64_t i = blockIdx.x * 4ull + (threadIdx.x >> 6); i < a.n; i += W) {
    const uint64_t k = a.chk[i];
    if (k < 2) continue;  // (uniform per wave)
    const uint64_t len = a.end[i] - a.start[i];
    const uint32_t t = wave_xor(gather_lane_term(a.raw + a.cpre[i], k, lane, len, g_tabs.pow8));
    if (lane == 0) a.crc[i] = gather_final(t, len, g_tabs.pow8);
  }
}

// Per query: the output offset, and (unless layout only) the stored checksum
// -- the little-endian u32 at end + 16, inside the file by gather_range_status
// -- against the computed one: status and CRC into the caller's arrays.
__global__ __launch_bounds__(256) void payload_finish_kernel(PayloadGatherArgs a) {
  for (uint64_t i = blockIdx.x * 256ull + threadIdx.x; i <= a.n; i += gridDim.x * 256ull) {
    a.o_off[i] = i < a.n ? a.off[i] : a.total;
    if (i == a.n) continue;
    uint32_t st = a.st[i], crc = 0;
    if (st == SRD_GATHER_OK) {
      if (a.layout_only) continue;
      crc = a.crc[i];
      if (crc != ld_u32_unaligned(a.file, a.end[i] + 16)) st = SRD_GATHER_BAD_CRC;
    }
    a.o_status[i] = (uint8_t)st;
    if (a.o_crc && !a.layout_only) a.o_crc[i] = crc;
  }
}

}  // namespace srd
