// srd_scatter.hip -- verified payloads read into a sequence of device segments
// (srd_payload_scatter_device; host glue in srd_ops.hip).
//
// Reference being replaced (jzombie/rust-simd-r-drive v0.16.3-alpha): a reader
// that fills its own buffers from an entry piece by piece, and checks it --
//   EntryStream (Read over an EntryHandle)   src/storage_engine/entry_stream.rs:44-92
//   EntryHandle::is_valid_checksum           simd-r-drive-entry-handle/src/entry_handle.rs:260-275
//
// The read-side mirror of the segment append (srd_segments.hip), and the
// gather (srd_gather.hip) without its packed buffer: the ranges are the
// gather's, the segment table is the segment append's with the roles swapped --
// a segment names the bytes that RECEIVE the next len bytes of the payload.
// The work units are pieces of segments cut at the destination's 16-byte
// boundaries (srd_scatter.h), which the streaming kernel (srd_stream.hip) takes
// as they are: a unit's destination is an offset from the 16-byte boundary
// below the lowest destination of the call.  Steps, all on the caller's stream:
//   scatter_layout_kernel   per query: status by arithmetic, the segments
//                           judged, per segment its offset inside the payload,
//                           its unit count and its query (then one hipCUB
//                           exclusive sum: units per segment)
//   units_kernel .. unit_combine_kernel   the unit table, the streaming kernel
//                           and the combine (srd_units.hip), the scatter view
//   scatter_finish_kernel   per query: stored checksum, status, the caller's arrays

namespace srd {

// (the queries as UnitArgs' ranges and table: eun = the queries' unit counts,
// sun / upre = the segments' and their exclusive sum)
struct ScatterArgs : UnitArgs {
  uint64_t flen;
  uint64_t n_dst;
  uint8_t* st;  // [n] the range's status, or SCATTER_BAD_LENGTH
  // [0] the queries of more than one unit, [1] the error word (append_err_word: atomicMin)
  unsigned long long* cnt;
  // the caller's arrays (scatter_finish_kernel)
  uint8_t* o_status;
  uint32_t* o_crc;
};

__global__ __launch_bounds__(256) void scatter_layout_kernel(ScatterArgs a) {
  uint64_t err = ~0ull;
  for (uint64_t i = blockIdx.x * 256ull + threadIdx.x; i < a.n; i += gridDim.x * 256ull) {
    const uint64_t s = a.start[i], e = a.end[i], f0 = a.first[i], f1 = a.first[i + 1];
    uint32_t st = gather_range_status(s, e, a.flen);
    uint64_t k = 0;
    if (!seg_first_ok(f0, f1, i, a.n, a.n_segs)) err = min<uint64_t>(err, append_err_word(i, SEG_BAD_FIRST));
    else {
      const ScatterEntry x = scatter_entry_layout(a.segs, f0, f1, ScatterTable{a.srcs}, a.n_dst, st, e - s, (uint32_t)i,
                                                  a.soff, a.sun, a.sent);
      if (x.bad) err = min<uint64_t>(err, append_err_word(i, SEG_BAD_SEGMENT));
      st = x.status;
      k = x.units;
    }
    a.st[i] = (uint8_t)st;
    a.eun[i] = k;
    const uint64_t m = __ballot(k > 1);
    if (m && (threadIdx.x & 63) == (uint32_t)__builtin_ctzll(m)) atomicAdd(a.cnt, (unsigned long long)__builtin_popcountll(m));
  }
  if (err != ~0ull) atomicMin(a.cnt + 1, (unsigned long long)err);  // (a refused call only)
}

// Per query: the stored checksum -- the little-endian u32 at end + 16, inside
// the file by gather_range_status -- against the computed one: status and CRC
// into the caller's arrays.
__global__ __launch_bounds__(256) void scatter_finish_kernel(ScatterArgs a) {
  for (uint64_t i = blockIdx.x * 256ull + threadIdx.x; i < a.n; i += gridDim.x * 256ull) {
    uint32_t st = a.st[i], crc = 0;
    if (st == SRD_GATHER_OK) {
      crc = a.crc[i];
      if (crc != ld_u32_unaligned(a.file, a.end[i] + 16)) st = SRD_GATHER_BAD_CRC;
    }
    a.o_status[i] = (uint8_t)st;
    if (a.o_crc) a.o_crc[i] = crc;
  }
}

}  // namespace srd
