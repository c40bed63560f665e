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
//   payload_units_kernel    the expanded unit table: unit -> hit
//   payload_gather_kernel   one wave per unit: copy + raw CRC of the chunk (a
//                           single-unit hit's CRC is finished here)
//   payload_combine_kernel  one wave per multi-unit hit: folds its chunks' CRCs
//   payload_finish_kernel   per query: stored checksum, status, the caller's arrays
// srd_batch_append_device (srd_append.hip) runs the units, gather and combine
// kernels as they are, with the caller's blob as the file and the store as the
// output.

namespace srd {

struct PayloadGatherArgs {
  const uint8_t* file;
  uint64_t flen;
  const uint64_t *start, *end;  // the caller's ranges [n]
  uint64_t n;
  uint8_t* st;     // [n] gather_range_status
  uint64_t* plen;  // [n] padded length (0 for no hit)
  uint64_t* chk;   // [n] chunk count
  uint64_t* off;   // [n] exclusive sum of plen: the output offsets
  uint64_t* cpre;  // [n] exclusive sum of chk
  uint64_t total;  // off[n - 1] + plen[n - 1] (known after the host's wait)
  unsigned long long* cnt;  // [0] the hits of more than one chunk
  uint32_t* unit_hit;       // [units] the expanded unit table
  uint64_t n_units;
  uint32_t* raw;   // [units] a multi-unit hit's chunks: crc_raw
  uint32_t* crc;   // [n] a hit's CRC32
  uint8_t* out;    // nullptr: nothing is copied (verify only)
  // the caller's arrays (payload_finish_kernel)
  uint64_t* o_off;
  uint8_t* o_status;
  uint32_t* o_crc;
  uint32_t layout_only;
  uint32_t* nz;    // [n] payload_gather_kernel<true>: set for a hit with a byte that is not 0
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

__global__ __launch_bounds__(256) void payload_units_kernel(PayloadGatherArgs a) {
  for (uint64_t u = blockIdx.x * 256ull + threadIdx.x; u < a.n_units; u += gridDim.x * 256ull)
    a.unit_hit[u] = (uint32_t)gather_unit_hit(a.cpre, a.n, u);
}

// One wave per unit, units w, w + W, ... of the batch (W waves in the grid).
// The 4 KiB blocks of the wave's units form one sequence; a 2-deep register
// ring keeps the next block's loads in flight while the current one is
// stored and checksummed.  Per block, as in write_kernel: lane l moves its
// four 16-byte pieces (1024 j + 16 l, j < 4) and computes their raw CRCs from
// the same registers (crc_line4_wide), weighted by lane (lane_weight_or with
// nib_c) and XOR-reduced per half-wave: raw CRC of the block = (lo * x^4096) ^
// hi; the blocks of a unit are folded Horner-style with x^32768 and the last
// block's zero padding is divided out (invpow).  The unit descriptors come by
// scalar loads; every store of the ring is an unconditional buffer store whose
// unused lanes are out of range (verify only: all of them); a partial or
// unaligned piece takes the byte path.  Nothing outside the unit's own
// payload bytes is read: whole pieces lie inside the chunk, the byte path
// stops at its end.
// NZ (srd_batch_append_device's stream rule; the gather runs NZ = false): the
// unit also ORs its words, as write_kernel does for its null_only word, and a
// unit with a byte that is not 0 marks its hit in a.nz.
template <bool NZ = false>
__global__ __launch_bounds__(SCAN_WAVES_V2 * 64, 1) void payload_gather_kernel(PayloadGatherArgs a) {
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
  const bool copy = a.out != nullptr;
  uint64_t last_len = ~0ull;  // cache of ~(x^(8 len) * 0xFFFFFFFF) for runs of equal lengths
  uint32_t last_fix = 0;

  struct Unit {
    uint64_t src;    // file offset of the chunk
    uint64_t dst;    // its offset in out
    uint64_t clen;   // its length
    uint64_t hlen;   // the hit's length
    uint32_t hit;
    bool single, last;  // the hit's only / last chunk
    bool al;            // the chunk's address is 16-byte aligned
  };
  // unit u's descriptor by SCALAR loads (the tables are read-only here): as
  // vector loads they would join the ring's vmcnt queue
  auto unit_s = [&](uint64_t u) {
    typedef const __attribute__((address_space(4))) uint64_t* q64_t;
    Unit x;
    x.hit = ((const __attribute__((address_space(4))) uint32_t*)a.unit_hit)[u];
    const uint64_t s = ((q64_t)a.start)[x.hit], e = ((q64_t)a.end)[x.hit];
    const uint64_t c = u - ((q64_t)a.cpre)[x.hit];
    x.hlen = e - s;
    x.src = s + c * GATHER_CHUNK;
    x.dst = ((q64_t)a.off)[x.hit] + c * GATHER_CHUNK;
    x.clen = gather_chunk_len(x.hlen, c);
    x.last = c * GATHER_CHUNK + x.clen == x.hlen;
    x.single = x.last && c == 0;
    x.al = (((uintptr_t)a.file + x.src) & 15) == 0;
    return x;
  };
  // piece j of the lane is a whole 16-byte vector inside the chunk
  auto vec_piece = [&](const Unit& x, uint64_t b, int j) -> bool {
    return x.al && b * TILE + 1024ull * j + 16ull * lane + 16 <= x.clen;
  };
  auto load_blk = [&](const Unit& x, uint64_t b, uint32_t (&o)[16]) {
#pragma unroll
    for (int j = 0; j < 4; j++) {
      const u32x4* q =
          vec_piece(x, b, j) ? (const u32x4*)(a.file + x.src + b * TILE + 1024ull * j + 16ull * lane) : &g_wdummy[j];
      const u32x4 v = *q;
      o[4 * j] = v[0]; o[4 * j + 1] = v[1]; o[4 * j + 2] = v[2]; o[4 * j + 3] = v[3];
    }
  };

  uint64_t u = w, b = 0;
  Unit x = unit_s(u);
  uint32_t acc = 0, any = 0;
  auto step = [&](uint32_t (&d)[16], uint32_t (&nx)[16]) -> bool {
    const uint64_t nb = (x.clen + TILE - 1) / TILE;
    // the block after (u, b); past the wave's last unit: block 0 of this unit again (harmless)
    uint64_t u2 = u, b2 = b + 1;
    Unit x2 = x;
    if (b2 >= nb) {
      u2 = u + W;
      b2 = 0;
      if (u2 < a.n_units) x2 = unit_s(u2);
    }
    load_blk(x2, b2, nx);
    bool vp[4];
#pragma unroll
    for (int j = 0; j < 4; j++) vp[j] = vec_piece(x, b, j);
    // a partial (or unaligned) piece: byte by byte, zero past the chunk
    // (extra memory ops on this path only: the ring's waits stay right)
    {
      const uint8_t* src = a.file + x.src;
      uint8_t* dst = a.out + x.dst;
#pragma unroll
      for (int j = 0; j < 4; j++) {
        if (!vp[j]) {
          const uint64_t oj = b * TILE + 1024ull * j + 16ull * lane;
          const uint32_t nl = oj < x.clen ? (uint32_t)min<uint64_t>(16, x.clen - oj) : 0u;
#pragma unroll
          for (int k = 0; k < 4; k++) {
            uint32_t wd = 0;
#pragma unroll
            for (int kb = 0; kb < 4; kb++) {
              const uint32_t q = 4u * k + kb;
              if (q < nl) {
                const uint8_t v = src[oj + q];
                if (copy) dst[oj + q] = v;
                wd |= (uint32_t)v << (8 * kb);
              }
            }
            d[4 * j + k] = wd;
          }
        }
      }
    }
    {
      const __amdgpu_buffer_rsrc_t rb = out_rsrc(a.out + x.dst + b * TILE, copy ? TILE : 0u);
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
    // raw CRC of this 4 KiB block (zero-padded past the chunk)
    const uint32_t hx = half_suffix_xor(lane_weight_or(crc_line4_wide(d, lds, R), nib_lane), lane);
    const uint32_t lo = __builtin_amdgcn_readlane(hx, 0), hi = __builtin_amdgcn_readlane(hx, 32);
    const uint32_t raw = mulfix(lo, utab(g_tabs.m4096)) ^ hi;
    acc = b ? mul_tile_u(acc) ^ raw : raw;
    const bool done = b + 1 == nb;
    uint32_t val = acc;
    if (done) {
      const uint64_t z = nb * TILE - x.clen;  // trailing zero padding of the last block, < 4096
      if (z) val = mulp(tab_u(&g_tabs.invpow[z]), acc);
      if (x.single) {
        if (x.hlen != last_len) {
          last_len = x.hlen;
          last_fix = ~mulp(xpow8_u(x.hlen), 0xFFFFFFFFu);
        }
        val ^= last_fix;  // crc32fast: init and xorout 0xFFFFFFFF
      }
    }
    // the unit's result -- a single-unit hit's CRC32, else the chunk's raw CRC
    // -- and, behind a hit's last chunk, the zero bytes up to the 64-byte boundary
    __builtin_amdgcn_raw_buffer_store_b32(val, out_rsrc(a.crc + x.hit, done && x.single ? 4u : 0u), 4u * lane, 0, 0);
    __builtin_amdgcn_raw_buffer_store_b32(val, out_rsrc(a.raw + u, done && !x.single ? 4u : 0u), 4u * lane, 0, 0);
    if constexpr (NZ)  // (every unit of a hit that stores here stores the same word)
      __builtin_amdgcn_raw_buffer_store_b32(1u, out_rsrc(a.nz + x.hit, done && __ballot(any != 0) ? 4u : 0u), 4u * lane, 0,
                                            0);
    const uint32_t nz = done && x.last && copy ? (uint32_t)(gather_pad64(x.hlen) - x.hlen) : 0u;
    __builtin_amdgcn_raw_buffer_store_b8((uint8_t)0, out_rsrc(a.out + x.dst + x.clen, nz), (uint32_t)lane, 0, 0);
    u = u2;
    b = b2;
    x = x2;
    return u < a.n_units;
  };
  uint32_t cur[16], nxt[16];
  load_blk(x, 0, cur);
  // the ring: two register blocks, the roles swapped every block
  while (step(cur, nxt) && step(nxt, cur)) {
  }
}

// One wave per hit of more than one chunk: lane l folds the raw CRCs of its
// share of the chunks (gather_lane_term: Horner by x^(8 chunk), moved up by
// the bytes behind the share), the XOR over the lanes is crc_raw(hit), and the
// length-dependent init / xorout fix makes it the CRC32.
__global__ __launch_bounds__(256) void payload_combine_kernel(PayloadGatherArgs a) {
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
