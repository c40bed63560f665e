// srd_index_live.hip -- in-place maintenance of the device KeyIndexer table of
// srd_index.hip: apply a batch of (key_hash, metadata offset, tombstone) pairs,
// export the live pairs, lay out a batch of tombstones;
// and the two steps srd_compact_live_device has around the append's path
// (section 13).
//
// Reference being replaced (jzombie/rust-simd-r-drive v0.16.3-alpha):
//   DataStore::reindex          src/storage_engine/data_store.rs:224-259
//   KeyIndexer::insert / remove src/storage_engine/key_indexer.rs:135-160, :174-178
//   batch_delete_key_hashes     src/storage_engine/data_store.rs:995-1024
//
// The slot states and the probe / claim loops are srd_table.h.
//
// An apply is three launches, each race-free by what it may touch:
//   1 live_dedupe_kernel  batch -> scratch table of batch positions (table untouched)
//   2 live_lookup_kernel  one lane per distinct key reads the table (nobody writes it)
//   -- the host reads the counts: a batch that would overfill the table ends here --
//   3 live_commit_kernel  stores into found slots (one lane per slot) and
//                         claims of empty slots for keys known absent and unique
// No lane ever waits for another one.

namespace srd {

constexpr uint64_t LIVE_OP_NONE = ~0ull;       // LiveArgs::op_slot: nothing to do for this pair
constexpr uint64_t LIVE_OP_CLAIM = ~0ull - 1;  // a new key: claim an empty slot

struct LiveArgs {
  const uint64_t* kh;   // [n] key hashes of the batch
  const uint64_t* mo;   // [n] metadata offsets
  const uint8_t* tomb;  // [n] nullable: 1 = the pair is a tombstone
  uint64_t n;
  uint32_t* dslot;      // [2^log2dc] scratch table: 0 = empty, else 1 + the last batch position of the slot's key
  uint32_t* dtomb;      // [2^log2dc / 32] bit s: a pair of slot s's key is a tombstone (deleted_keys, data_store.rs:861,896)
  uint32_t log2dc;
  uint32_t* lslot;      // [n] the scratch slot of pair i's key
  Table t;              // the table
  uint64_t* op_slot;    // [n] table slot to store op_val into / LIVE_OP_CLAIM / LIVE_OP_NONE
  uint64_t* op_val;     // [n]
  unsigned long long* cnt;  // [4] inserted, updated, removed (per distinct key), new slots needed
};

// KeyIndexer::pack(tag_from_hash(key_hash), offset) (key_indexer.rs:64-82)
__device__ __forceinline__ uint64_t live_pack(uint64_t key_hash, uint64_t meta_off) {
  return (key_hash >> 48 << 48) | (meta_off & 0xFFFFFFFFFFFFull);
}

// Latest-wins dedupe of the batch.  A scratch slot holds a batch position, so
// its key is kh[position]: read from the input, never from a word another
// lane may still be writing (key hashes 0 and 2^64-1 are legal, no key value
// could mark "not yet written").  Two lanes with the same new key: one wins
// the CAS on the empty slot, the other sees the winner's position in the CAS
// result, finds its own key there and raises the slot to the later position
// (atomicMax).  A slot that is not empty only ever changes to another
// position of the same key, so a stale read of it still names the right key.
// Terminates: 2^log2dc >= 2 n slots.
__global__ void live_dedupe_kernel(LiveArgs a) {
  const uint32_t mask = (1u << a.log2dc) - 1;
  for (uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; i < a.n; i += (uint64_t)gridDim.x * blockDim.x) {
    const uint64_t k = a.kh[i];
    const uint32_t me = (uint32_t)i + 1;
    uint32_t s = (uint32_t)idx_slot(k, a.log2dc);
    for (;;) {
      uint32_t v = __hip_atomic_load(a.dslot + s, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
      if (v == 0) {
        v = atomicCAS(a.dslot + s, 0u, me);
        if (v == 0) break;  // claimed for k
      }
      if (a.kh[v - 1] == k) {
        atomicMax(a.dslot + s, me);
        break;
      }
      s = (s + 1) & mask;
    }
    a.lslot[i] = s;
    if (a.tomb && a.tomb[i]) atomicOr(a.dtomb + (s >> 5), 1u << (s & 31));
  }
}

// One lane per distinct key (the pair whose position the scratch slot ended
// with: the key's last pair in batch order) looks the key up in the table,
// which no lane writes during this launch, and records what the commit has
// to do.  The reference's loop per key (reindex, data_store.rs:238-253):
//   key in deleted_keys -> KeyIndexer::remove; otherwise KeyIndexer::insert
//   of the last pair's offset.
// KeyIndexer::insert's tag check (key_indexer.rs:135-160) compares the stored
// packed value's tag with the new one's; both are key_hash >> 48 of the same
// key_hash, so it can never fire here and there is no error path for it.
__global__ void live_lookup_kernel(LiveArgs a) {
  unsigned long long ins = 0, upd = 0, rem = 0, fresh = 0;
  for (uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; i < a.n; i += (uint64_t)gridDim.x * blockDim.x) {
    uint64_t op = LIVE_OP_NONE, val = 0;
    const uint32_t ds = a.lslot[i];
    if (a.dslot[ds] == (uint32_t)i + 1) {
      const uint64_t k = a.kh[i];
      const bool del = (a.dtomb[ds >> 5] >> (ds & 31)) & 1;
      const uint64_t np = live_pack(k, a.mo[i]);
      uint64_t s;
      const uint64_t p = table_find(a.t, k, &s);
      const bool found = p != TBL_EMPTY;
      const bool present = found && p != TBL_DELETED;
      if (del) {
        if (present) { op = s; val = TBL_DELETED; rem++; }
      } else {
        val = np;
        if (found) {
          op = s;  // update, or revival of the key's own deleted slot
          if (present) upd++; else ins++;
        } else {
          op = LIVE_OP_CLAIM;
          ins++;
          fresh++;
        }
      }
    }
    a.op_slot[i] = op;
    a.op_val[i] = val;
  }
  for (int o = 32; o > 0; o >>= 1) {
    ins += __shfl_xor(ins, o);
    upd += __shfl_xor(upd, o);
    rem += __shfl_xor(rem, o);
    fresh += __shfl_xor(fresh, o);
  }
  if ((threadIdx.x & 63) == 0) {
    if (ins) atomicAdd(a.cnt + 0, ins);
    if (upd) atomicAdd(a.cnt + 1, upd);
    if (rem) atomicAdd(a.cnt + 2, rem);
    if (fresh) atomicAdd(a.cnt + 3, fresh);
  }
}

// Commit.  Stores: each found slot belongs to one distinct key, so one lane
// writes it, and its value is never TBL_EMPTY before or after.  Claims: the
// keys are distinct and known absent, so a claim compares no key words -- it
// takes the first slot of its probe chain whose packed word it can CAS from
// TBL_EMPTY (the build's claim, idx_table_insert_kernel) and then writes the
// key word, which no lane of this launch reads.  A store and a claim never
// contend for a slot: the CAS only succeeds on TBL_EMPTY.  Readers come in a
// later launch and see both words.
__global__ void live_commit_kernel(LiveArgs a) {
  const uint64_t mask = (1ull << a.t.log2cap) - 1;
  for (uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; i < a.n; i += (uint64_t)gridDim.x * blockDim.x) {
    const uint64_t op = a.op_slot[i];
    if (op == LIVE_OP_NONE) continue;
    const uint64_t val = a.op_val[i];
    if (op != LIVE_OP_CLAIM) {
      a.t.packed[op & mask] = val;
      continue;
    }
    table_claim(a.t, a.kh[i], val);  // terminates: the host admitted the batch (table_admits)
  }
}

// live = neither empty nor deleted
__global__ void live_count_kernel(const uint64_t* tpacked, uint64_t cap, unsigned long long* cnt) {
  unsigned long long mine = 0;
  for (uint64_t s = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; s < cap; s += (uint64_t)gridDim.x * blockDim.x)
    mine += tpacked[s] < TBL_DELETED;
  for (int o = 32; o > 0; o >>= 1) mine += __shfl_xor(mine, o);
  if ((threadIdx.x & 63) == 0 && mine) atomicAdd(cnt, mine);
}

// the live pairs in any order (the sort by offset that follows fixes it); the
// caller sized the outputs by live_count_kernel's count
__global__ void live_gather_kernel(const uint64_t* tkeys, const uint64_t* tpacked, uint64_t cap, unsigned long long* cnt,
                                   uint64_t* okeys, uint64_t* opacked, uint64_t out_cap) {
  for (uint64_t s = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; s < cap; s += (uint64_t)gridDim.x * blockDim.x) {
    const uint64_t p = tpacked[s];
    if (p >= TBL_DELETED) continue;
    const uint64_t j = atomicAdd(cnt, 1ull);
    if (j < out_cap) {
      okeys[j] = tkeys[s];
      opacked[j] = p;
    }
  }
}

// batch_delete_key_hashes keeps the hashes the index holds (data_store.rs:
// 1004-1008), in input order, duplicates included
__global__ void live_present_kernel(Table t, const uint64_t* q, uint64_t n, uint32_t* flag) {
  for (uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (uint64_t)gridDim.x * blockDim.x)
    flag[i] = table_get(t, q[i]) != TBL_EMPTY;
}

// ... and appends one tombstone per kept hash from `tail`: a NULL byte and
// the metadata, 21 bytes, no prepad (data_store.rs:864-897)
__global__ void live_tomb_entries_kernel(const uint64_t* q, const uint32_t* flag, const uint32_t* pos, uint64_t n,
                                         uint64_t tail, srd_write_entry* ent) {
  for (uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (uint64_t)gridDim.x * blockDim.x)
    if (flag[i]) ent[pos[i]] = srd_write_entry{0, 1, q[i], tail + 21ull * pos[i], 0u, SRD_ENTRY_TOMB | SRD_ENTRY_HASHED};
}

// ---------------------------------------------------------------------------
// srd_compact_live_device: the two steps around the
// append's path.  The iterator's ranges [start, end) as the append's lengths --
// its starts and key hashes are the append's src_off and key_hash arrays as
// they are.
__global__ __launch_bounds__(256) void compact_lens_kernel(const uint64_t* st, const uint64_t* en, uint64_t n,
                                                           uint64_t* len) {
  for (uint64_t i = blockIdx.x * 256ull + threadIdx.x; i < n; i += gridDim.x * 256ull) len[i] = en[i] - st[i];
}

// Behind the append's finish, per written entry: the recomputed CRC (the
// gather kernels') against the checksum stored in the source, the
// little-endian u32 at end + 16 (inside the file by entry_range) -- cnt[0]
// counts the entries that differ, cnt[1] is the lowest output position among
// them (preset to ~0) -- and the pair's value for the new table,
// pack(key_hash >> 48, new metadata offset).
__global__ __launch_bounds__(256) void compact_finish_kernel(const uint8_t* file, const uint64_t* en, const uint64_t* kh,
                                                             const uint32_t* crc, const uint64_t* mo, uint64_t n,
                                                             uint64_t* packed, unsigned long long* cnt) {
  unsigned long long first = ~0ull;
  // (whole waves in every round: the ballot sees 64 lanes)
  const uint64_t rounds = (n + gridDim.x * 256ull - 1) / (gridDim.x * 256ull);
  for (uint64_t r = 0; r < rounds; r++) {
    const uint64_t i = (r * gridDim.x + blockIdx.x) * 256ull + threadIdx.x;
    bool bad = false;
    if (i < n) {
      bad = crc[i] != ld_u32_unaligned(file, en[i] + 16);
      packed[i] = live_pack(kh[i], mo[i]);
      if (bad) first = min(first, (unsigned long long)i);
    }
    const uint64_t m = __ballot(bad);
    if (m && (threadIdx.x & 63) == (uint32_t)__builtin_ctzll(m)) atomicAdd(cnt, (unsigned long long)__builtin_popcountll(m));
  }
  if (first != ~0ull) atomicMin(cnt + 1, first);  // (a corrupt store only)
}

}  // namespace srd
