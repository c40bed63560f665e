// srd_ttl.hip -- the TTL cache on the device: the
// namespaced key hash, the batched read's decision, and the sweep over the
// live index.  The rule is srd_ttl.h's (ttl_judge), the table's probe is
// srd_table.h's, the hash is srd_xxh3.h's.
//
// Reference being replaced (jzombie/rust-simd-r-drive v0.16.3-alpha):
//   StorageCacheExt::read_with_ttl  extensions/src/storage_cache_ext.rs:72-107
//   NamespaceHasher::namespace      src/utils/namespace_hasher.rs:33-65
//
// Every kernel here only reads the store and the table.  What an eviction
// writes goes through the delete's path: live_dedupe_kernel over the expired
// queries, live_tomb_entries_kernel, the writer and the apply (srd_ops.hip).

namespace srd {

// the keys of a batch as raw bytes: key i = keys[offs[i] .. offs[i] + lens[i])
struct NsKeys {
  const uint8_t* keys;
  const uint64_t* offs;
  const uint64_t* lens;
  uint64_t prefix_hash;  // xxh3_64(prefix)
};

// xxh3_64 of the 16 bytes le64(a) || le64(b): the 9-to-16-byte path of
// srd_xxh3.h's xxh3_64 with both words already in registers
__device__ __forceinline__ uint64_t xxh3_64_u64x2(uint64_t a, uint64_t b) {
  const uint64_t lo = a ^ (x_sec64(24) ^ x_sec64(32));
  const uint64_t hi = b ^ (x_sec64(40) ^ x_sec64(48));
  return x_av3(16 + __builtin_bswap64(lo) + hi + x_fold(lo, hi));
}

// NamespaceHasher::namespace (namespace_hasher.rs:52-64) and compute_hash of
// its result for key i; *key_hash = xxh3_64(key i), the namespaced key's second word
__device__ __forceinline__ uint64_t ns_hash(const NsKeys& k, uint64_t i, uint64_t* key_hash) {
  *key_hash = xxh3_64(k.keys + k.offs[i], k.lens[i]);
  return xxh3_64_u64x2(k.prefix_hash, *key_hash);
}

// one lane per key; ns (nullable, 8-byte aligned): the 16 namespaced bytes of each key
__global__ __launch_bounds__(256) void ns_hash_kernel(NsKeys k, uint64_t n, uint64_t* ns, uint64_t* out) {
  const uint64_t i = blockIdx.x * 256ull + threadIdx.x;
  if (i >= n) return;
  uint64_t kh;
  out[i] = ns_hash(k, i, &kh);
  if (ns) {
    ns[2 * i] = k.prefix_hash;
    ns[2 * i + 1] = kh;
  }
}

struct TtlResolveArgs {
  Table t;
  const uint8_t* file;
  uint64_t flen;
  const uint64_t* q;  // [n] key hashes (the hashed form)
  NsKeys k;           // the keys (the fused form)
  uint64_t* q_out;    // [n] the fused form's hashes
  uint64_t n, now;
  uint64_t *start, *end;    // [n]
  uint64_t* expiry;         // [n] nullable
  uint8_t* status;          // [n]
  unsigned long long* cnt;  // [4] nullable: queries per status, added to
};

// read_with_ttl's decision per query (storage_cache_ext.rs:72-104), nothing
// written to the store: the probe (KeyIndexer::get_packed), the metadata, the
// payload's first 8 bytes.  KEYS: the query is a raw key, hashed here first.
// The read's tag check (data_store.rs:513-521) compares the stored tag with
// the tag of the hash the entry was looked up by: it cannot fire.
template <bool KEYS>
__global__ __launch_bounds__(256) void ttl_resolve_kernel(TtlResolveArgs a) {
  unsigned long long c[4] = {0, 0, 0, 0};
  for (uint64_t i = blockIdx.x * 256ull + threadIdx.x; i < a.n; i += gridDim.x * 256ull) {
    uint64_t h;
    if (KEYS) {
      uint64_t kh;
      h = ns_hash(a.k, i, &kh);
      a.q_out[i] = h;
    } else {
      h = a.q[i];
    }
    const uint64_t p = table_get(a.t, h);
    TtlVerdict v{TTL_NOT_FOUND, 0, 0, 0};
    if (p != TBL_EMPTY) v = ttl_judge(a.file, a.flen, p & 0xFFFFFFFFFFFFull, a.now);
    a.start[i] = v.start;
    a.end[i] = v.end;
    if (a.expiry) a.expiry[i] = v.expiry;
    a.status[i] = (uint8_t)v.status;
#pragma unroll
    for (uint32_t s = 0; s < 4; s++) c[s] += v.status == s;
  }
  if (!a.cnt) return;
  // a wave reduction, the block's four waves through LDS, one atomic per block
  // and status that occurred (iter_flag_kernel's shape).  One atomic per WAVE
  // and status over a grid of n / 256 blocks put 2^15 of them on one line for
  // 2^20 queries and took three quarters of the kernel's time (section 18).
  __shared__ unsigned long long part[4][4];
#pragma unroll
  for (int s = 0; s < 4; s++) {
    for (int o = 32; o > 0; o >>= 1) c[s] += __shfl_xor(c[s], o);
    if ((threadIdx.x & 63) == 0) part[threadIdx.x >> 6][s] = c[s];
  }
  __syncthreads();
  if (threadIdx.x < 4) {
    const unsigned long long sum = part[0][threadIdx.x] + part[1][threadIdx.x] + part[2][threadIdx.x] + part[3][threadIdx.x];
    if (sum) atomicAdd(a.cnt + threadIdx.x, sum);
  }
}

// The expired queries' hashes, packed in batch order (pos = the exclusive sum
// of flag), for live_dedupe_kernel ...
__global__ void ttl_candidates_kernel(const uint8_t* status, uint64_t n, uint32_t* flag) {
  for (uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (uint64_t)gridDim.x * blockDim.x)
    flag[i] = ttl_evict_candidate(status[i]);
}
__global__ void ttl_pack_kernel(const uint64_t* q, const uint32_t* flag, const uint32_t* pos, uint64_t n, uint64_t* xq) {
  for (uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (uint64_t)gridDim.x * blockDim.x)
    if (flag[i]) xq[pos[i]] = q[i];
}
// ... and behind it the candidates that get their key's tombstone
__global__ void ttl_keep_kernel(const uint32_t* dslot, const uint32_t* lslot, uint64_t m, uint32_t* flag) {
  for (uint64_t j = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; j < m; j += (uint64_t)gridDim.x * blockDim.x)
    flag[j] = ttl_evict_keeps(dslot[lslot[j]], j);
}

// The sweep: ttl_judge over the table's live pairs in ascending metadata
// offset (the export's order).  flag[i] = pair i is expired; cnt[0] expired,
// cnt[1] too short, cnt[2] the smallest expiry among the LIVE ones (preset ~0).
__global__ __launch_bounds__(256) void ttl_sweep_kernel(const uint8_t* file, uint64_t flen, const uint64_t* packed,
                                                        uint64_t n, uint64_t now, uint32_t* flag,
                                                        unsigned long long* cnt) {
  unsigned long long ne = 0, ns = 0, next = ~0ull;
  for (uint64_t i = blockIdx.x * 256ull + threadIdx.x; i < n; i += gridDim.x * 256ull) {
    const TtlVerdict v = ttl_judge(file, flen, packed[i] & 0xFFFFFFFFFFFFull, now);
    flag[i] = v.status == TTL_EXPIRED;
    ne += v.status == TTL_EXPIRED;
    ns += v.status == TTL_TOO_SHORT;
    if (v.status == TTL_LIVE) next = min(next, (unsigned long long)v.expiry);
  }
  for (int o = 32; o > 0; o >>= 1) {
    ne += __shfl_xor(ne, o);
    ns += __shfl_xor(ns, o);
    next = min(next, (unsigned long long)__shfl_xor(next, o));
  }
  __shared__ unsigned long long part[4][3];
  if ((threadIdx.x & 63) == 0) {
    part[threadIdx.x >> 6][0] = ne;
    part[threadIdx.x >> 6][1] = ns;
    part[threadIdx.x >> 6][2] = next;
  }
  __syncthreads();
  if (threadIdx.x == 0) {  // one set of atomics per block
    ne = part[0][0] + part[1][0] + part[2][0] + part[3][0];
    ns = part[0][1] + part[1][1] + part[2][1] + part[3][1];
    next = min(min(part[0][2], part[1][2]), min(part[2][2], part[3][2]));
    if (ne) atomicAdd(cnt + 0, ne);
    if (ns) atomicAdd(cnt + 1, ns);
    if (next != ~0ull) atomicMin(cnt + 2, next);
  }
}

}  // namespace srd
