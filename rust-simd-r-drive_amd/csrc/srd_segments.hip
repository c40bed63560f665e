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
// ended -- and a streaming kernel that stores whole 16-byte destination vectors
// at any source and destination alignment.  Steps, all on the caller's stream:
//   segments_layout_kernel   per entry: d_seg_first and the segments judged by
//                            arithmetic, the entry's length, slot and unit
//                            count, per segment its offset inside the entry,
//                            its unit count and its entry (then two hipCUB
//                            exclusive sums: slots, units per segment)
//   segments_units_kernel    per unit: its descriptor (SegUnit)
//   segments_stream_kernel   one wave per unit: copy + raw CRC (a single-unit
//                            entry's CRC is finished here), marks the entries
//                            that are not all 0
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
  uint8_t* file;  // the store, file[j] = file byte j
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

// four destination words from two adjacent aligned source vectors w[0..8): the
// bytes [4 Q + sh, 4 Q + sh + 16) of the pair
template <int Q>
__device__ __forceinline__ void seg_funnel(uint32_t (&d)[16], const uint32_t (&e)[16], uint32_t sh) {
#pragma unroll
  for (int j = 0; j < 4; j++) {
    const uint32_t w[8] = {d[4 * j], d[4 * j + 1], d[4 * j + 2], d[4 * j + 3], e[4 * j], e[4 * j + 1], e[4 * j + 2], e[4 * j + 3]};
#pragma unroll
    for (int k = 0; k < 4; k++) d[4 * j + k] = __builtin_amdgcn_alignbyte(w[Q + k + 1], w[Q + k], sh);
  }
}

// One wave per unit, units w, w + W, ... of the batch (W waves in the grid):
// payload_gather_kernel's structure -- the 4 KiB blocks of the wave's units as
// one sequence, the 2-deep register ring, per block the raw CRC from the
// registers that are stored (crc_line4_wide, lane_weight_or, half_suffix_xor),
// the blocks folded Horner-style, the last block's zero padding divided out --
// in a frame that is aligned to the DESTINATION: with A = dst mod 16 the unit
// is the A + len bytes from the 16-byte boundary below its first byte, the A
// leading ones taken as 0 (leading zero bytes leave a raw CRC as it is).  Lane
// l's piece j of block b is the 16 bytes at 4096 b + 1024 j + 16 l of that
// frame, a whole aligned vector of the store; where the piece holds 16 bytes of
// the unit it is stored as one.  With r = (source - destination) mod 16, the
// same for the whole unit:
//   r == 0  the piece is one aligned source vector;
//   r != 0  it is assembled from the two aligned source vectors that hold its
//           bytes by a byte-funnel shift (v_alignbyte_b32; r is uniform, the
//           shift amount scalar) -- the second vector rides the ring too.
// An aligned source vector is loaded only where all of it lies inside the
// unit's SEGMENT (SegUnit::lf); a piece that would need another one, and the
// pieces that hold the unit's first and last fewer-than-16 bytes, go byte by
// byte.  Nothing outside the unit's own destination bytes is written.
__global__ __launch_bounds__(SCAN_WAVES_V2 * 64, 1) void segments_stream_kernel(SegArgs a) {
  __shared__ ScanLds lds;
  load_crc_lds<true>(lds);
  const int lane = threadIdx.x & 63;
  const int wv = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  uint32_t R[4];
  crc_lane_bases(R, lane);
  const uint32_t nib_lane = lds_off(lds.nib) + 4u * (lane & 31);
  const uint64_t W = (uint64_t)gridDim.x * SCAN_WAVES_V2;
  const uint64_t w = (uint64_t)blockIdx.x * SCAN_WAVES_V2 + wv;
  if (w >= a.n_units) return;
  uint64_t last_len = ~0ull;  // cache of ~(x^(8 len) * 0xFFFFFFFF) for runs of equal lengths
  uint32_t last_fix = 0;

  struct Unit {
    const uint8_t* src;  // the frame's first byte in the source (never dereferenced below src + f.a)
    uint64_t dst;        // ... and its file offset, a multiple of 16
    uint64_t end;
    uint32_t ent;
    SegFrame f;          // (srd_segments.h)
    bool single;
  };
  // unit u's descriptor by SCALAR loads (the table is read-only here): as
  // vector loads they would join the ring's vmcnt queue
  auto unit_s = [&](uint64_t u) {
    typedef const __attribute__((address_space(4))) uint64_t* q64_t;
    const q64_t q = (q64_t)(a.unit + u);
    const uint64_t src = q[0], dst = q[1], el = q[3];
    const uint32_t lf = (uint32_t)(el >> 32);
    Unit x;
    x.end = q[2];
    x.ent = (uint32_t)el;
    x.f = seg_frame(src, dst, lf);
    x.src = (const uint8_t*)(uintptr_t)(src - x.f.a);
    x.dst = dst - x.f.a;
    x.single = seg_lf_single(lf);
    return x;
  };
  // piece j of the lane holds 16 bytes of the unit, and its source vectors may be loaded
  auto vec_piece = [&](const Unit& x, uint32_t b, int j) -> bool {
    return seg_piece_vec(x.f, b * (uint32_t)TILE + 1024u * j + 16u * lane);
  };
  auto load_blk = [&](const Unit& x, uint32_t b, uint32_t (&o0)[16], uint32_t (&o1)[16]) {
    const u32x4* q[4];
#pragma unroll
    for (int j = 0; j < 4; j++) {
      q[j] = vec_piece(x, b, j) ? (const u32x4*)(x.src + b * (uint32_t)TILE + 1024u * j + 16u * lane - x.f.r) : &g_wdummy[j];
      const u32x4 v = q[j][0];
      o0[4 * j] = v[0]; o0[4 * j + 1] = v[1]; o0[4 * j + 2] = v[2]; o0[4 * j + 3] = v[3];
    }
    if (x.f.r) {  // (uniform)
#pragma unroll
      for (int j = 0; j < 4; j++) {
        const u32x4 v = vec_piece(x, b, j) ? q[j][1] : g_wdummy[j];
        o1[4 * j] = v[0]; o1[4 * j + 1] = v[1]; o1[4 * j + 2] = v[2]; o1[4 * j + 3] = v[3];
      }
    }
  };

  uint64_t u = w;
  uint32_t b = 0;
  Unit x = unit_s(u);
  uint32_t acc = 0, any = 0;
  auto step = [&](uint32_t (&d)[16], uint32_t (&e)[16], uint32_t (&nd)[16], uint32_t (&ne)[16]) -> bool {
    const uint32_t nb = (x.f.vlen + (uint32_t)TILE - 1) / (uint32_t)TILE;
    // the block after (u, b); past the wave's last unit: block 0 of this unit again (harmless)
    uint64_t u2 = u;
    uint32_t b2 = b + 1;
    Unit x2 = x;
    if (b2 >= nb) {
      u2 = u + W;
      b2 = 0;
      if (u2 < a.n_units) x2 = unit_s(u2);
    }
    load_blk(x2, b2, nd, ne);
    bool vp[4];
#pragma unroll
    for (int j = 0; j < 4; j++) vp[j] = vec_piece(x, b, j);
    if (x.f.r) {  // (uniform) the destination vectors from the source pairs
      const uint32_t sh = x.f.r & 3u;
      switch (x.f.r >> 2) {
        case 0: seg_funnel<0>(d, e, sh); break;
        case 1: seg_funnel<1>(d, e, sh); break;
        case 2: seg_funnel<2>(d, e, sh); break;
        default: seg_funnel<3>(d, e, sh); break;
      }
    }
    // any other piece: byte by byte, zero outside the unit (extra memory ops on
    // this path only: the ring's waits stay right)
    {
      uint8_t* dst = a.file + x.dst;
#pragma unroll
      for (int j = 0; j < 4; j++) {
        if (!vp[j]) {
          const uint32_t oj = b * (uint32_t)TILE + 1024u * j + 16u * lane;
#pragma unroll
          for (int k = 0; k < 4; k++) {
            uint32_t wd = 0;
#pragma unroll
            for (int kb = 0; kb < 4; kb++) {
              const uint32_t p = oj + 4u * k + kb;
              if (p >= x.f.a && p < x.f.vlen) {
                const uint8_t v = x.src[p];
                dst[p] = v;
                wd |= (uint32_t)v << (8 * kb);
              }
            }
            d[4 * j + k] = wd;
          }
        }
      }
    }
    {
      const __amdgpu_buffer_rsrc_t rb = out_rsrc(a.file + x.dst + (uint64_t)b * TILE, TILE);
#pragma unroll
      for (int j = 0; j < 4; j++)
        __builtin_amdgcn_raw_buffer_store_b128(u32x4{d[4 * j], d[4 * j + 1], d[4 * j + 2], d[4 * j + 3]}, rb,
                                               vp[j] ? 16u * lane + 1024u * j : OOB_OFF, 0, 0);
    }
    if (b == 0) any = 0;
#pragma unroll
    for (int j = 0; j < 16; j++) any |= d[j];
    // raw CRC of this 4 KiB block of the frame (zero below and behind the unit)
    const uint32_t hx = half_suffix_xor(lane_weight_or(crc_line4_wide(d, lds, R), nib_lane), lane);
    const uint32_t lo = __builtin_amdgcn_readlane(hx, 0), hi = __builtin_amdgcn_readlane(hx, 32);
    const uint32_t raw = mulfix(lo, utab(g_tabs.m4096)) ^ hi;
    acc = b ? mul_tile_u(acc) ^ raw : raw;
    const bool done = b + 1 == nb;
    uint32_t val = acc;
    if (done) {
      const uint32_t z = nb * (uint32_t)TILE - x.f.vlen;  // trailing zero padding of the last block, < 4096
      if (z) val = mulp(tab_u(&g_tabs.invpow[z]), acc);
      if (x.single) {  // (the entry's length is the unit's end)
        if (x.end != last_len) {
          last_len = x.end;
          last_fix = ~mulp(xpow8_u(x.end), 0xFFFFFFFFu);
        }
        val ^= last_fix;  // crc32fast: init and xorout 0xFFFFFFFF
      }
    }
    // the unit's result: a single-unit entry's CRC32, else the unit's raw CRC
    __builtin_amdgcn_raw_buffer_store_b32(val, out_rsrc(a.crc + x.ent, done && x.single ? 4u : 0u), 4u * lane, 0, 0);
    __builtin_amdgcn_raw_buffer_store_b32(val, out_rsrc(a.raw + u, done && !x.single ? 4u : 0u), 4u * lane, 0, 0);
    // (every unit of an entry that stores here stores the same word)
    __builtin_amdgcn_raw_buffer_store_b32(1u, out_rsrc(a.nz + x.ent, done && __ballot(any != 0) ? 4u : 0u), 4u * lane, 0, 0);
    u = u2;
    b = b2;
    x = x2;
    return u < a.n_units;
  };
  uint32_t c0[16], c1[16], n0[16], n1[16];
  load_blk(x, 0, c0, c1);
  // the ring: two register blocks, the roles swapped every block
  while (step(c0, c1, n0, n1) && step(n0, n1, c0, c1)) {
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
