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
//   units_kernel .. unit_combine_kernel   the unit table, the streaming kernel
//                           and the combine (srd_units.hip), the hits as ranges
//   payload_finish_kernel   per query: stored checksum, status, the caller's arrays

namespace srd {

// (the hits as UnitArgs' ranges: eun = the chunk counts, off = the exclusive
// sum of plen, upre = the exclusive sum of the chunk counts)
struct PayloadGatherArgs : UnitArgs {
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
    a.eun[i] = k;
    const uint64_t m = __ballot(k > 1);
    if (m && (threadIdx.x & 63) == (uint32_t)__builtin_ctzll(m)) atomicAdd(a.cnt, (unsigned long long)__builtin_popcountll(m));
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
