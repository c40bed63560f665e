// srd_stream.hip -- the streaming copy + CRC-32 kernel of the payload gather
// (srd_gather.hip), the device append and the live compaction (srd_append.hip)
// and the segment append (srd_segments.hip): one wave per work unit over a
// table of unit descriptors (SegUnit, srd_segments.h), whoever built it.

namespace srd {

struct StreamArgs {
  const SegUnit* unit;  // [n_units]; SegUnit::dst is an offset from out, ent an index of crc / nz
  uint64_t n_units;
  uint8_t* out;   // 16-byte aligned; nullptr: nothing is written but the results (verify only)
  uint32_t* raw;  // [n_units] a unit of a multi-unit entry: crc_raw
  uint32_t* crc;  // [entries] a single-unit entry's CRC32
  uint32_t* nz;   // [entries] NZ: set for an entry with a byte that is not 0
  const uint64_t* d_n_units;  // DEV: the unit count, a word in device memory (n_units only bounds the grid)
};

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

// One wave per unit, units w, w + W, ... of the batch (W waves in the grid).
// The 4 KiB blocks of the wave's units form one sequence; a 2-deep register
// ring keeps the next block's loads in flight while the current one is stored
// and checksummed.  Per block, as in write_kernel: lane l moves its four
// 16-byte pieces (1024 j + 16 l, j < 4) and computes their raw CRCs from the
// same registers (crc_line4_wide), weighted by lane (lane_weight_or with
// nib_c) and XOR-reduced per half-wave: raw CRC of the block = (lo * x^4096) ^
// hi; the blocks of a unit are folded Horner-style with x^32768 and the last
// block's zero padding is divided out (invpow).  The unit descriptors come by
// scalar loads; every store of the ring is an unconditional buffer store whose
// unused lanes are out of range (verify only: all of them).
// The blocks lie in a frame that is aligned to the DESTINATION: with A = dst
// mod 16 the unit is the A + len bytes from the 16-byte boundary below its
// first byte, the A leading ones taken as 0 (leading zero bytes leave a raw CRC
// as it is).  Lane l's piece j of block b is the 16 bytes at 4096 b + 1024 j +
// 16 l of that frame, a whole aligned vector of the output; where the piece
// holds 16 bytes of the unit it is stored as one.  With r = (source -
// destination) mod 16, the same for the whole unit:
//   r == 0  the piece is one aligned source vector;
//   r != 0  it is assembled from the two aligned source vectors that hold its
//           bytes by a byte-funnel shift (v_alignbyte_b32; r is uniform, the
//           shift amount scalar) -- the second vector rides the ring too.
// An aligned source vector is loaded only where all of it lies inside the
// unit's SEGMENT (SegUnit::lf; for a chunk unit: its hit or payload); a piece
// that would need another one, and the pieces that hold the unit's first and
// last fewer-than-16 bytes, go byte by byte.  Nothing outside the segment is
// read, and nothing outside the unit's own destination bytes is written but
// the zero bytes a unit owns behind it (seg_unit_pad).
// NZ (the stream rule): the unit also ORs its words, as write_kernel does for
// its null_only word, and a unit with a byte that is not 0 marks its entry in
// a.nz.
// DEV (srd_read_rows_device): the unit count comes from device memory and the
// grid from a bound, so whole blocks may have nothing to do: a block none of
// whose waves has a unit leaves before the LDS fill (158 KiB per block; the
// fill is a step of the whole block, so the decision is the block's).
template <bool NZ, bool DEV = false>
__global__ __launch_bounds__(SCAN_WAVES_V2 * 64, 1) void stream_copy_crc_kernel(StreamArgs a) {
  __shared__ ScanLds lds;
  const uint64_t n_units = DEV ? *a.d_n_units : a.n_units;
  if (DEV && (uint64_t)blockIdx.x * SCAN_WAVES_V2 >= n_units) return;
  load_crc_lds<true>(lds);
  const int lane = threadIdx.x & 63;
  const int wv = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  uint32_t R[4];
  crc_lane_bases(R, lane);
  const uint32_t nib_lane = lds_off(lds.nib) + 4u * (lane & 31);
  const uint64_t W = (uint64_t)gridDim.x * SCAN_WAVES_V2;
  const uint64_t w = (uint64_t)blockIdx.x * SCAN_WAVES_V2 + wv;
  if (w >= n_units) return;
  const bool copy = a.out != nullptr;
  uint64_t last_len = ~0ull;  // cache of ~(x^(8 len) * 0xFFFFFFFF) for runs of equal lengths
  uint32_t last_fix = 0;

  struct Unit {
    const uint8_t* src;  // the frame's first byte in the source (never dereferenced below src + f.a)
    uint64_t dst;        // ... and its offset in out, a multiple of 16
    uint64_t end;
    uint32_t ent;
    SegFrame f;          // (srd_segments.h)
    uint32_t pad;        // seg_unit_pad
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
    x.pad = seg_unit_pad(dst, lf);
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
      if (u2 < n_units) x2 = unit_s(u2);
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
    // this path only: the ring's waits stay right); its stores go through a
    // resource over the frame, empty for verify only
    {
      const __amdgpu_buffer_rsrc_t rf = out_rsrc(a.out + x.dst, copy ? x.f.vlen : 0u);
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
                __builtin_amdgcn_raw_buffer_store_b8(v, rf, p, 0, 0);
                wd |= (uint32_t)v << (8 * kb);
              }
            }
            d[4 * j + k] = wd;
          }
        }
      }
    }
    {
      const __amdgpu_buffer_rsrc_t rb = out_rsrc(a.out + x.dst + (uint64_t)b * TILE, copy ? TILE : 0u);
#pragma unroll
      for (int j = 0; j < 4; j++)
        __builtin_amdgcn_raw_buffer_store_b128(u32x4{d[4 * j], d[4 * j + 1], d[4 * j + 2], d[4 * j + 3]}, rb,
                                               vp[j] && copy ? 16u * lane + 1024u * j : OOB_OFF, 0, 0);
    }
    if constexpr (NZ) {
      if (b == 0) any = 0;
#pragma unroll
      for (int j = 0; j < 16; j++) any |= d[j];
    }
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
    // the unit's result -- a single-unit entry's CRC32, else the unit's raw CRC
    // -- and the zero bytes the unit owns behind it
    __builtin_amdgcn_raw_buffer_store_b32(val, out_rsrc(a.crc + x.ent, done && x.single ? 4u : 0u), 4u * lane, 0, 0);
    __builtin_amdgcn_raw_buffer_store_b32(val, out_rsrc(a.raw + u, done && !x.single ? 4u : 0u), 4u * lane, 0, 0);
    if constexpr (NZ)  // (every unit of an entry that stores here stores the same word)
      __builtin_amdgcn_raw_buffer_store_b32(1u, out_rsrc(a.nz + x.ent, done && __ballot(any != 0) ? 4u : 0u), 4u * lane, 0,
                                            0);
    __builtin_amdgcn_raw_buffer_store_b8((uint8_t)0, out_rsrc(a.out + x.dst + x.f.vlen, done && copy ? x.pad : 0u),
                                         (uint32_t)lane, 0, 0);
    u = u2;
    b = b2;
    x = x2;
    return u < n_units;
  };
  uint32_t c0[16], c1[16], n0[16], n1[16];
  load_blk(x, 0, c0, c1);
  // the ring: two register blocks, the roles swapped every block
  while (step(c0, c1, n0, n1) && step(n0, n1, c0, c1)) {
  }
}

}  // namespace srd
