// srd_append.hip -- payloads already in HBM appended to a store
// (srd_batch_append_device; host glue in srd_ops.hip).
//
// Reference being replaced (jzombie/rust-simd-r-drive v0.16.3-alpha):
//   batch_write_with_key_hashes(.., false)  src/storage_engine/data_store.rs:847-939
//   write_stream_with_key_hash              src/storage_engine/data_store.rs:758-825
//   (copy / transfer / rename go through it: :941-984, copy_handle :587-590)
//
// The write-side mirror of the gather: the layout is one exclusive sum on the
// device (srd_append.h), the payload bytes move in the gather's work units
// (UnitArgs' ranges: the payloads inside the caller's blob, the output offsets
// the layout's prefix from roundup64(tail) on) through the streaming kernel,
// and only what an append has on top of a copy is new.
// Steps, all on the caller's stream:
//   append_layout_kernel     per entry: status by arithmetic (one byte read
//                            for a 1-byte payload), slot size, chunk count, the
//                            source range's end (then two hipCUB exclusive sums)
//   units_kernel .. unit_combine_kernel   the unit table, the streaming kernel
//                            (<true> under the stream rule: marks the entries
//                            that are not all 0) and the combine (srd_units.hip),
//                            the payloads as ranges
//   append_finish_kernel     per entry: the 20 metadata bytes, the zero prepad
//                            up to the next payload, the metadata offset

namespace srd {

struct AppendArgs {
  const uint8_t* pay;   // the caller's blob
  uint64_t pay_len;
  const uint64_t *src, *len, *kh;  // the caller's arrays [n]
  uint64_t n;
  uint64_t tail, base;  // base = append_base(tail)
  uint64_t* end;        // [n] src + len (the gather kernels' range end; 0 for a refused range)
  uint64_t* slot;       // [n] append_slot(len)
  uint64_t* chk;        // [n] unit count (UnitArgs::eun)
  const uint64_t* pre;  // [n] exclusive sum of slot
  // [0] entries of more than one chunk, [1] the error word (append_err_word:
  // atomicMin), [2] the sum of append_coarse(slot), [3] the last entry's
  // length, [4] null_only (the stream rule's outcome)
  unsigned long long* cnt;
  const uint32_t* crc;  // [n] the entries' CRC32 (gather kernels)
  const uint32_t* nz;   // [n] stream rule: the entry has a byte that is not 0 (nullptr: no rule)
  uint8_t* file;        // the store, file[j] = file byte j
  uint64_t* mo;         // [n] the caller's metadata offsets
};

__device__ __forceinline__ uint64_t wave_sum_u64(uint64_t v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o);
  return v;
}
__device__ __forceinline__ uint64_t lane_u64(uint64_t v, int l) {
  return ((uint64_t)(uint32_t)__builtin_amdgcn_readlane((uint32_t)(v >> 32), l) << 32) |
         (uint64_t)(uint32_t)__builtin_amdgcn_readlane((uint32_t)v, l);
}

// What both layout kernels (the segment append's: srd_segments.hip) do with an
// entry once it is judged -- status st, len bytes, `units` units; every lane of
// a wave comes here, the lanes past the batch (i >= n) too: the ballot sees 64
// lanes -- its slot and unit count (none for a refused entry), the sums, the
// last entry's length, and the count of the entries of more than one unit ...
struct LayoutSums { uint64_t coarse = 0, err = ~0ull; };
__device__ __forceinline__ void append_layout_entry(const AppendArgs& a, uint64_t i, uint32_t st, uint64_t len, uint64_t units,
                                                    LayoutSums& t) {
  uint64_t k = 0;
  if (i < a.n) {
    const bool ok = st == APPEND_OK;
    const uint64_t slot = ok ? append_slot(len) : 0;
    k = ok ? units : 0;
    a.slot[i] = slot;
    a.chk[i] = k;
    t.coarse += append_coarse(slot);
    if (!ok) t.err = min<uint64_t>(t.err, append_err_word(i, st));
    if (i == a.n - 1) a.cnt[3] = len;
  }
  const uint64_t m = __ballot(k > 1);
  if (m && (threadIdx.x & 63) == (uint32_t)__builtin_ctzll(m)) atomicAdd(a.cnt, (unsigned long long)__builtin_popcountll(m));
}
// ... and, behind the last round, the error word and the coarse sum
__device__ __forceinline__ void append_layout_close(const AppendArgs& a, LayoutSums t) {
  if (t.err != ~0ull) atomicMin(a.cnt + 1, (unsigned long long)t.err);  // (a refused batch only)
  t.coarse = wave_sum_u64(t.coarse);
  if ((threadIdx.x & 63) == 0 && t.coarse) atomicAdd(a.cnt + 2, (unsigned long long)t.coarse);
}

__global__ __launch_bounds__(256) void append_layout_kernel(AppendArgs a) {
  LayoutSums sums;
  // (whole waves in every round: the ballot and the reductions see 64 lanes)
  const uint64_t rounds = (a.n + gridDim.x * 256ull - 1) / (gridDim.x * 256ull);
  for (uint64_t r = 0; r < rounds; r++) {
    const uint64_t i = (r * gridDim.x + blockIdx.x) * 256ull + threadIdx.x;
    uint64_t len = 0;
    uint32_t st = APPEND_EMPTY;
    if (i < a.n) {
      const uint64_t s = a.src[i];
      len = a.len[i];
      st = append_range_status(s, len, a.pay_len);
      if (st == APPEND_OK && len == 1 && a.pay[s] == 0) st = APPEND_NULL_BYTE;
      a.end[i] = st == APPEND_OK ? s + len : 0;
    }
    append_layout_entry(a, i, st, len, gather_chunks(len), sums);
  }
  append_layout_close(a, sums);
}

// One wave per 64 consecutive entries: lane j loads entry i0 + j's layout (its
// own and its predecessor's prefix and length), then the wave writes the
// entries one after another -- EntryMetadata::serialize (key_hash LE,
// prev_offset LE, checksum LE: bytes 0-19, one per lane) and the zero bytes up
// to the next entry's payload (data_store.rs:907-914; none behind the batch's
// last entry), by byte stores: the first line of the batch is shared with the
// bytes below the tail, which stay as they are.  Entry 0's wave also zeroes
// the batch's own prepad [tail, base).
__global__ __launch_bounds__(256) void append_finish_kernel(AppendArgs a) {
  const int lane = threadIdx.x & 63;
  const uint64_t W = gridDim.x * 4ull;
  for (uint64_t g = blockIdx.x * 4ull + (threadIdx.x >> 6); g * 64 < a.n; g += W) {
    const uint64_t i = g * 64 + lane;
    uint64_t m = 0, prev = 0, kh = 0;
    uint32_t crc = 0, nb = 0;
    if (i < a.n) {
      m = append_meta(a.base, a.pre[i], a.len[i]);
      prev = i ? append_meta(a.base, a.pre[i - 1], a.len[i - 1]) + 20 : a.tail;
      kh = a.kh[i];
      crc = a.crc[i];
      nb = i + 1 < a.n ? (uint32_t)(gather_pad64(m + 20) - m) : 20u;  // 20 .. 83
      a.mo[i] = m;
      if (a.nz && !a.nz[i]) atomicOr((unsigned int*)(a.cnt + 4), 1u);
    }
    const int cnt = (int)min<uint64_t>(64, a.n - g * 64);
    for (int j = 0; j < cnt; j++) {
      const uint64_t mj = lane_u64(m, j), pj = lane_u64(prev, j), kj = lane_u64(kh, j);
      const uint32_t cj = (uint32_t)__builtin_amdgcn_readlane(crc, j), nj = (uint32_t)__builtin_amdgcn_readlane(nb, j);
      const uint64_t v = lane < 8 ? kj : lane < 16 ? pj : (uint64_t)cj;
      uint8_t* q = a.file + mj;
      if ((uint32_t)lane < nj) q[lane] = lane < 20 ? (uint8_t)(v >> (8 * (lane & 7))) : (uint8_t)0;
      if (64u + lane < nj) q[64 + lane] = 0;
    }
    if (g == 0 && a.tail + lane < a.base) a.file[a.tail + lane] = 0;
  }
}

}  // namespace srd
