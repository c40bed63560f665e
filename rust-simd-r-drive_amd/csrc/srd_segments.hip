// srd_segments.hip -- entries whose payload is a sequence of device segments
// appended to a store (srd_batch_append_segments_device; host glue in
// srd_ops.hip).
//
// Reference being replaced (jzombie/rust-simd-r-drive v0.16.3-alpha):
//   write_stream_with_key_hash   src/storage_engine/data_store.rs:758-825
//   (the checksum runs over the pieces in order, :775,788)
//
// The append (srd_append.hip) with a payload that arrives in pieces: the entry
// layout, the finish step and the stream rule are the append's as they are;
// new are the table's judgement, the work units -- pieces of SEGMENTS
// (srd_segments.h), so a unit's destination is wherever the previous piece
// ended, which the streaming kernel (srd_stream.hip) takes at any source and
// destination alignment -- and a combine for units of arbitrary lengths.
// Steps, all on the caller's stream:
//   segments_layout_kernel   per entry: d_seg_first and the segments judged by
//                            arithmetic, the entry's length, slot and unit
//                            count, per segment its offset inside the entry,
//                            its unit count and its entry (then two hipCUB
//                            exclusive sums: slots, units per segment)
//   segments_units_kernel    per unit: its descriptor (SegUnit)
//   stream_copy_crc_kernel   one wave per unit: copy + raw CRC (a single-unit
//                            entry's CRC is finished here), marks the entries
//                            that are not all 0 (srd_stream.hip, <true>)
//   segments_terms_kernel    per unit of a multi-unit entry: its term of the
//                            entry's raw CRC
//   segments_combine_kernel  one wave per multi-unit entry: the XOR of its
//                            units' terms
//   append_finish_kernel     the append's, over the entries' total lengths

namespace srd {

struct SegArgs {
  const uint64_t* srcs;  // [2 n_src] the source table on the device: address, length
  uint64_t n_src;
  const srd_segment* segs;
  uint64_t n_segs;
  const uint64_t* first;  // [n + 1]
  uint64_t n, base;       // base = append_base(tail)
  uint64_t* len;          // [n] the entries' lengths
  uint64_t* slot;         // [n] append_slot(len)
  uint64_t* eun;          // [n] the entries' unit counts
  const uint64_t* pre;    // [n] exclusive sum of slot
  uint64_t* soff;         // [n_segs] a segment's offset inside its entry
  uint64_t* sun;          // [n_segs] its unit count
  const uint64_t* upre;   // [n_segs] exclusive sum of sun
  uint32_t* sent;         // [n_segs] its entry
  unsigned long long* cnt;  // AppendArgs::cnt's words
  SegUnit* unit;          // [n_units]
  uint64_t n_units;
  uint32_t* raw;  // [n_units] a multi-unit entry's units: crc_raw
  uint32_t* crc;  // [n] the entries' CRC32
  uint32_t* nz;   // [n] the entry has a byte that is not 0
};

struct SegSrcLens {  // the lengths of the interleaved source table
  const uint64_t* t;
  __device__ uint64_t operator[](uint64_t k) const { return t[2 * k + 1]; }
};

__global__ __launch_bounds__(256) void segments_layout_kernel(SegArgs a) {
  uint64_t coarse = 0, err = ~0ull;
  // (whole waves in every round: the ballot and the reductions see 64 lanes)
  const uint64_t rounds = (a.n + gridDim.x * 256ull - 1) / (gridDim.x * 256ull);
  for (uint64_t r = 0; r < rounds; r++) {
    const uint64_t i = (r * gridDim.x + blockIdx.x) * 256ull + threadIdx.x;
    uint64_t k = 0;
    if (i < a.n) {
      const uint64_t f0 = a.first[i], f1 = a.first[i + 1];
      SegEntry e{SEG_BAD_FIRST, 0, 0};
      if (seg_first_ok(f0, f1, i, a.n, a.n_segs)) {
        e = seg_entry_layout(a.segs, f0, f1, SegSrcLens{a.srcs}, a.n_src, a.soff, a.sun);
        for (uint64_t s = f0; s < f1; s++) a.sent[s] = (uint32_t)i;
      }
      const bool ok = e.status == APPEND_OK;
      const uint64_t slot = ok ? append_slot(e.len) : 0;
      k = ok ? e.units : 0;
      a.len[i] = ok ? e.len : 0;
      a.slot[i] = slot;
      a.eun[i] = k;
      coarse += append_coarse(slot);
      if (!ok) err = min<uint64_t>(err, append_err_word(i, e.status));
      if (i == a.n - 1) a.cnt[3] = e.len;
    }
    const uint64_t m = __ballot(k > 1);
    if (m && (threadIdx.x & 63) == (uint32_t)__builtin_ctzll(m)) atomicAdd(a.cnt, (unsigned long long)__builtin_popcountll(m));
  }
  if (err != ~0ull) atomicMin(a.cnt + 1, (unsigned long long)err);  // (a refused batch only)
  coarse = wave_sum_u64(coarse);
  if ((threadIdx.x & 63) == 0 && coarse) atomicAdd(a.cnt + 2, (unsigned long long)coarse);
}

// unit u: piece u - upre[s] of the segment s with upre[s] <= u < upre[s + 1]
__global__ __launch_bounds__(256) void segments_units_kernel(SegArgs a) {
  for (uint64_t u = blockIdx.x * 256ull + threadIdx.x; u < a.n_units; u += gridDim.x * 256ull) {
    const uint64_t s = gather_unit_hit(a.upre, a.n_segs, u);
    const srd_segment g = a.segs[s];
    const uint32_t ent = a.sent[s];
    const uint64_t off = a.soff[s];
    a.unit[u] = seg_unit(a.srcs[2 * g.src] + g.off, a.base + a.pre[ent] + off, off, g.len, u - a.upre[s], ent, a.eun[ent]);
  }
}

// The combine, in two steps (units of one entry have arbitrary lengths, so
// there is no common Horner step): per unit of a multi-unit entry, its term --
// the unit's raw CRC moved up by the entry's bytes behind the unit
// (seg_unit_term: one x^(8 k) by square-and-multiply per unit, so one thread
// per unit, not one wave per entry) -- in place of its raw CRC ...
__global__ __launch_bounds__(256) void segments_terms_kernel(SegArgs a) {
  for (uint64_t u = blockIdx.x * 256ull + threadIdx.x; u < a.n_units; u += gridDim.x * 256ull) {
    const SegUnit x = a.unit[u];
    if (!seg_lf_single(x.lf)) a.raw[u] = seg_unit_term(a.raw[u], a.len[x.ent], x.end, g_tabs.pow8);
  }
}
// ... then one wave per entry of more than one unit, the lanes striding over
// the entry's units: the XOR of the terms is crc_raw(entry), and the
// length-dependent init / xorout fix makes it the CRC32.
__global__ __launch_bounds__(256) void segments_combine_kernel(SegArgs a) {
  const uint32_t lane = threadIdx.x & 63;
  const uint64_t W = gridDim.x * 4ull;
  for (uint64_t i = blockIdx.x * 4ull + (threadIdx.x >> 6); i < a.n; i += W) {
    const uint64_t k = a.eun[i];
    if (k < 2) continue;  // (uniform per wave)
    const uint64_t u0 = a.upre[a.first[i]];  // (an entry with units has a segment)
    uint32_t t = 0;
    for (uint64_t j = lane; j < k; j += 64) t ^= a.raw[u0 + j];
    t = wave_xor(t);
    if (lane == 0) a.crc[i] = gather_final(t, a.len[i], g_tabs.pow8);
  }
}

}  // namespace srd
