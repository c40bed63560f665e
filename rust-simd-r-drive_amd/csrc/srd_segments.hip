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
// destination alignment.  The combine is every caller's (srd_units.hip): it
// takes units of arbitrary lengths.
// Steps, all on the caller's stream:
//   segments_layout_kernel   per entry: d_seg_first and the segments judged by
//                            arithmetic, the entry's length, slot and unit
//                            count, per segment its offset inside the entry,
//                            its unit count and its entry (then two hipCUB
//                            exclusive sums: slots, units per segment)
//   units_kernel .. unit_combine_kernel   the unit table, the streaming kernel
//                            (<true>: marks the entries that are not all 0) and
//                            the combine (srd_units.hip), the table view
//   append_finish_kernel     the append's, over the entries' total lengths

namespace srd {

struct SegSrcLens {  // the lengths of the interleaved source table
  const uint64_t* t;
  __device__ uint64_t operator[](uint64_t k) const { return t[2 * k + 1]; }
};

// (a: the entry layout's arrays and counter words; g: the table and what the
// unit kernels read of it)
__global__ __launch_bounds__(256) void segments_layout_kernel(AppendArgs a, UnitArgs g, uint64_t n_src) {
  LayoutSums sums;
  // (whole waves in every round: the ballot and the reductions see 64 lanes)
  const uint64_t rounds = (a.n + gridDim.x * 256ull - 1) / (gridDim.x * 256ull);
  for (uint64_t r = 0; r < rounds; r++) {
    const uint64_t i = (r * gridDim.x + blockIdx.x) * 256ull + threadIdx.x;
    SegEntry e{SEG_BAD_FIRST, 0, 0};
    if (i < a.n) {
      const uint64_t f0 = g.first[i], f1 = g.first[i + 1];
      if (seg_first_ok(f0, f1, i, a.n, g.n_segs)) {
        e = seg_entry_layout(g.segs, f0, f1, SegSrcLens{g.srcs}, n_src, g.soff, g.sun);
        for (uint64_t s = f0; s < f1; s++) g.sent[s] = (uint32_t)i;
      }
      g.len[i] = e.status == APPEND_OK ? e.len : 0;
    }
    append_layout_entry(a, i, e.status, e.len, e.units, sums);
  }
  append_layout_close(a, sums);
}

}  // namespace srd
