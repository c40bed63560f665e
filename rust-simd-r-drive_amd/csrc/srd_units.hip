// srd_units.hip -- the unit table and the CRC combine around the streaming
// kernel (srd_stream.hip), for every caller: the gather (srd_gather.hip), the
// device append and the live compaction (srd_append.hip) under the range view,
// the segment append (srd_segments.hip) under the table view (UnitArgs and the
// views: srd_segments.h).  Steps, all on the caller's stream (stream_units,
// srd_ops.hip):
//   units_kernel            per unit: its descriptor (SegUnit)
//   stream_copy_crc_kernel  one wave per unit: copy + raw CRC (a single-unit
//                           entry's CRC is finished here)
//   unit_terms_kernel       per unit of a multi-unit entry: its term of the
//                           entry's raw CRC
//   unit_combine_kernel     one wave per multi-unit entry: the XOR of its
//                           units' terms
// (the last two only when the batch has a multi-unit entry)
// DEV: the device-count forms (srd_read_rows_device, whose host never learns
// the counts): the unit count is the word *a.d_n_units, the grids are sized
// from a bound, and the last two leave at once when *a.d_n_multi is 0.

namespace srd {

template <class View, bool DEV = false>
__global__ __launch_bounds__(256) void units_kernel(UnitArgs a) {
  const uint64_t n_units = DEV ? *a.d_n_units : a.n_units;
  for (uint64_t u = blockIdx.x * 256ull + threadIdx.x; u < n_units; u += gridDim.x * 256ull) a.unit[u] = unit_of<View>(a, u);
}

// The combine, in two steps (units of one entry have arbitrary lengths, so
// there is no common Horner step): per unit of a multi-unit entry, its term --
// the unit's raw CRC moved up by the entry's bytes behind the unit
// (seg_unit_term: one x^(8 k) by square-and-multiply per unit, so one thread
// per unit, not one wave per entry) -- in place of its raw CRC ...
template <class View, bool DEV = false>
__global__ __launch_bounds__(256) void unit_terms_kernel(UnitArgs a) {
  if (DEV && !*a.d_n_multi) return;
  const uint64_t n_units = DEV ? *a.d_n_units : a.n_units;
  for (uint64_t u = blockIdx.x * 256ull + threadIdx.x; u < n_units; u += gridDim.x * 256ull) {
    const SegUnit x = a.unit[u];
    if (!seg_lf_single(x.lf)) a.raw[u] = seg_unit_term(a.raw[u], View::ent_len(a, x.ent), x.end, g_tabs.pow8);
  }
}
// ... then one wave per entry of more than one unit, the lanes striding over
// the entry's units: the XOR of the terms is crc_raw(entry), and the
// length-dependent init / xorout fix makes it the CRC32.
template <class View, bool DEV = false>
__global__ __launch_bounds__(256) void unit_combine_kernel(UnitArgs a) {
  if (DEV && !*a.d_n_multi) return;
  const uint32_t lane = threadIdx.x & 63;
  const uint64_t W = gridDim.x * 4ull;
  for (uint64_t i = blockIdx.x * 4ull + (threadIdx.x >> 6); i < a.n; i += W) {
    const uint64_t k = a.eun[i];
    if (k < 2) continue;  // (uniform per wave)
    const uint64_t u0 = unit_first<View>(a, i);
    uint32_t t = 0;
    for (uint64_t j = lane; j < k; j += 64) t ^= a.raw[u0 + j];
    t = wave_xor(t);
    if (lane == 0) a.crc[i] = gather_final(t, View::ent_len(a, i), g_tabs.pow8);
  }
}

}  // namespace srd
