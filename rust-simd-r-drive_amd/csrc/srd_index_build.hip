// srd_index_build.hip -- KeyIndexer::build on the device, host side (included
// by srd_api.hip): the bucketed build and its global-table fallback, the
// owner partition, and their C entries.

// global-table KeyIndexer::build workspace (full pass / skewed-bucket fallback)
static int alloc_hash(Ctx* c, uint64_t n) {
  const uint64_t hc = table_capacity(n);
  TRY(ensure(c, B_HKEYS, hc * 8));
  TRY(ensure(c, B_HVALS, hc * 8));
  TRY(ensure(c, B_LATEST, (n + 1) * 4));
  TRY(ensure(c, B_IPOS, (n + 1) * 4));
  TRY(ensure_cub(c, n + 1));
  return 0;
}

// KeyIndexer::build over n (key_hash, meta_off) pairs in file order with one
// global open-addressing table (device-wide atomics); syncs for the count.
// Default pairs: the chain in B_O_KH / B_O_MO -> B_IKEY / B_IPACKED.
static int index_global(Ctx* c, uint64_t n, uint64_t* n_index, const uint64_t* kh = nullptr,
                        const uint64_t* mo = nullptr, uint64_t* okey = nullptr, uint64_t* opacked = nullptr) {
  if (!kh) { kh = P<uint64_t>(c, B_O_KH); mo = P<uint64_t>(c, B_O_MO); }
  TRY(alloc_hash(c, n));
  if (!okey) { okey = P<uint64_t>(c, B_IKEY); opacked = P<uint64_t>(c, B_IPACKED); }
  uint64_t* cnt = P<uint64_t>(c, B_COUNTERS);
  const uint64_t hc = table_capacity(n);
  HIPCHK(hipMemsetAsync(P<void>(c, B_HKEYS), 0xff, hc * 8, c->stream));
  HIPCHK(hipMemsetAsync(P<void>(c, B_HVALS), 0, hc * 8, c->stream));
  HIPCHK(hipMemsetAsync(cnt + 7, 0, 8, c->stream));
  HIPCHK(hipMemsetAsync(P<uint32_t>(c, B_LATEST) + n, 0, 4, c->stream));
  if (n) {
    index_insert_kernel<<<blocks(n, 256), 256, 0, c->stream>>>(
        kh, mo, n, P<uint64_t>(c, B_HKEYS), P<unsigned long long>(c, B_HVALS), hc - 1, (unsigned long long*)(cnt + 7));
    LAUNCHED(c->stream, "index_insert_kernel");
    index_latest_kernel<<<blocks(n, 256), 256, 0, c->stream>>>(
        kh, mo, n, P<uint64_t>(c, B_HKEYS), P<unsigned long long>(c, B_HVALS), hc - 1, (unsigned long long*)(cnt + 7),
        P<uint32_t>(c, B_LATEST));
    LAUNCHED(c->stream, "index_latest_kernel");
  }
  TRY(scan_sum(c, P<uint32_t>(c, B_LATEST), P<uint32_t>(c, B_IPOS), n + 1));
  if (n) {
    index_emit_kernel<<<blocks(n, 256), 256, 0, c->stream>>>(kh, mo, P<uint32_t>(c, B_LATEST), P<uint32_t>(c, B_IPOS),
                                                             n, okey, opacked);
    LAUNCHED(c->stream, "index_emit_kernel");
  }
  uint32_t nidx = 0;
  TRY(read_small(c, c->stream, {rd(P<uint32_t>(c, B_IPOS) + n, &nidx)}));
  *n_index = nidx;
  return 0;
}

// KeyIndexer::build (key_indexer.rs:98-124) as a bucketed build over the
// pairs (kh[i], mo[i]), i < *n_dev, in file order (latest = last position);
// *status != 0 disables it.  Scratch (alloc_index): B_HOFF = the bucket fills [nbk] (zero
// before the claims) followed by the chunk counts [GLUE_BLOCKS], B_SKEY = nbk
// buckets of IDX_TCAP records, B_LATEST8.  pl->n_index / pl->idx_overflow are
// written.
static int alloc_index(Ctx* c, uint64_t n_cap, uint32_t log2_nbk) {
  const uint64_t nbk = (uint64_t)1 << log2_nbk;
  TRY(ensure(c, B_HOFF, (nbk + GLUE_BLOCKS) * 4));
  TRY(ensure(c, B_SKEY, nbk * IDX_TCAP * 8));
  TRY(ensure_z(c, B_LATEST8, n_cap + 1));  // zero on (re)allocation: no entry carries a live generation
  return 0;
}
// a fresh generation of the non-latest marks for each index build (the
// array is cleared once every 255 builds)
static int next_lgen(Ctx* c) {
  if (++c->lgen == 0) {
    HIPCHK(hipMemsetAsync(P<void>(c, B_LATEST8), 0, c->bufs[B_LATEST8].n, c->stream));
    c->lgen = 1;
  }
  return 0;
}
// the words every index build needs zeroed: the bucket fills and, after them,
// the per-chunk non-latest counts (IdxArgs::ccount)
static uint32_t* index_zero_words(Ctx* c, uint32_t log2_nbk, uint32_t* n) {
  *n = (1u << log2_nbk) + GLUE_BLOCKS;
  return P<uint32_t>(c, B_HOFF);
}
static uint32_t index_log2_buckets(uint64_t n_est) {
  uint32_t log2_nbk = 1;  // >= 1: the bucket is the hash's top log2_nbk bits
  while (log2_nbk < 14 && ((uint64_t)IDX_BUCKET_AVG << log2_nbk) < n_est) log2_nbk++;
  return log2_nbk;
}
static IdxArgs index_args(Ctx* c, uint32_t log2_nbk) {
  IdxArgs ia{};
  ia.log2_nbk = log2_nbk;
  ia.bfill = P<uint32_t>(c, B_HOFF);
  ia.ccount = ia.bfill + ((size_t)1 << log2_nbk);
  ia.srec = P<uint64_t>(c, B_SKEY);
  ia.latest = P<uint8_t>(c, B_LATEST8);
  ia.lgen = c->lgen;
  return ia;
}
// fused: chain_finalize_kernel already claimed the bucket ranges and wrote
// the records (child2_kernel zeroed the fills); otherwise the fills are
// zeroed here, and idx_hist_scatter_kernel claims the ranges and fills them
static int launch_index_bucketed(Ctx* c, const uint64_t* kh, const uint64_t* mo, const uint64_t* n_dev,
                                 const uint32_t* status, uint32_t log2_nbk, uint64_t* okey, uint64_t* opacked,
                                 Plan* pl, bool fused = false, const FinArgs* slow = nullptr, bool zeroed = false,
                                 const uint64_t* scan_ticks = nullptr) {
  TRY(next_lgen(c));
  IdxArgs ia = index_args(c, log2_nbk);
  ia.alias = fused ? 1u : 0u;
  if (fused) {
    ia.pub = c->h_pub;
    ia.pub_seq = ++c->pub_seq;
    ia.scan_ticks = scan_ticks;  // (the optimistic scan's device time, XPart)
  }
  ia.kh = kh;
  ia.mo = mo;
  ia.n_dev = n_dev;
  ia.status = status;
  ia.okey = okey;
  ia.opacked = opacked;
  ia.plan = pl;
  const uint32_t nbk = 1u << log2_nbk;
  if (!fused) {
    uint32_t nz = 0;
    uint32_t* zw = index_zero_words(c, log2_nbk, &nz);
    if (!zeroed) HIPCHK(hipMemsetAsync(zw, 0, (size_t)nz * 4, c->stream));
    idx_hist_scatter_kernel<<<IDX_HBLOCKS, 256, nbk * 4, c->stream>>>(ia);
    LAUNCHED(c->stream, "idx_hist_scatter_kernel");
  }
  FinArgs fs{};  // n_slow == nullptr: no slow list
  if (slow) fs = *slow;
  idx_dedup_kernel<<<nbk, 512, 0, c->stream>>>(ia, fs);
  LAUNCHED(c->stream, "idx_dedup_kernel");
  idx_emit_kernel<<<GLUE_BLOCKS, GLUE_THREADS, 0, c->stream>>>(ia);
  LAUNCHED(c->stream, "idx_emit_kernel");
  return 0;
}

// stable partition of n (key, value) device pairs by owner rank; interleaved
// output at out (out_v == nullptr) or keys at out / values at out_v.  counts
// (host, [world]) receives the group sizes.  Synchronises.
// counts (host, nullable): the per-owner pair counts, read back with one
// host round trip; d_counts (nullable): their device address instead, no
// sync (the multi-GPU exchange's owners read them over xGMI)
static int partition_impl(Ctx* c, const uint64_t* keys, const uint64_t* vals, uint64_t n, uint32_t world,
                          uint64_t* out, uint64_t* out_v, uint64_t* counts, const uint64_t** d_counts = nullptr) {
  const uint64_t nc = (uint64_t)world * GLUE_BLOCKS + 1;
  TRY(ensure(c, B_PCNT, nc * 4));
  TRY(ensure(c, B_POFF, nc * 4 + 8 * PART_MAX_WORLD));
  TRY(ensure_cub(c, nc));
  PartArgs a{};
  a.keys = keys;
  a.vals = vals;
  a.n = n;
  a.world = world;
  a.cnt = P<uint32_t>(c, B_PCNT);
  a.off = P<uint32_t>(c, B_POFF);
  a.out = out;
  a.out_v = out_v;
  a.counts = (uint64_t*)(P<uint32_t>(c, B_POFF) + ((nc + 1) & ~1ull));
  part_count_kernel<<<GLUE_BLOCKS, 256, 0, c->stream>>>(a);
  LAUNCHED(c->stream, "part_count_kernel");
  TRY(scan_sum(c, a.cnt, a.off, nc));
  part_scatter_kernel<<<GLUE_BLOCKS, 256, 0, c->stream>>>(a);
  LAUNCHED(c->stream, "part_scatter_kernel");
  part_counts_kernel<<<1, 64, 0, c->stream>>>(a);
  LAUNCHED(c->stream, "part_counts_kernel");
  if (d_counts) *d_counts = a.counts;
  if (counts) {
    HIPCHK(hipMemcpyAsync(counts, a.counts, world * 8, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(spin_sync(c->stream));
  }
  return 0;
}

extern "C" int srd_index_partition_device(srd_ctx* c, const uint64_t* d_keys, const uint64_t* d_vals, uint64_t n,
                                          uint32_t world, uint64_t* d_out_pairs, uint64_t* counts) {
  if (!c || !counts || world == 0 || world > PART_MAX_WORLD || (n && (!d_keys || !d_vals || !d_out_pairs))) {
    set_err("bad argument");
    return SRD_ERR_ARG;
  }
  HIPCHK(hipSetDevice(c->device));
  return partition_impl(c, d_keys, d_vals, n, world, d_out_pairs, nullptr, counts);
}

// KeyIndexer::build over (key_hash, meta_off or packed) device pairs given as
// two arrays, in file order (latest position wins); output in chain order of
// each key's latest entry.  The pair count is n; or, with d_n, it is on the
// device (*d_n <= n) and the buckets are sized for n_est expected pairs: the
// multi-GPU owners' build right behind their gather, no host round trip for
// the count.  Synchronises once.
static int index_build_sep(Ctx* c, const uint64_t* keys, const uint64_t* vals, uint64_t n, uint64_t* okeys,
                           uint64_t* opacked, uint64_t* n_index, const uint64_t* d_n = nullptr,
                           uint64_t n_est = 0) {
  *n_index = 0;
  if (!n) return 0;
  TRY(ensure(c, B_MPLAN, sizeof(Plan)));
  const uint32_t log2_nbk = index_log2_buckets(d_n ? std::max<uint64_t>(n_est, 1) : n);
  TRY(alloc_index(c, n, log2_nbk));
  Plan* pl = P<Plan>(c, B_MPLAN);
  // one launch zeroes the plan, sets its n_chain to the pair count and zeroes
  // the bucket fills
  uint32_t nz = 0;
  uint32_t* zw = index_zero_words(c, log2_nbk, &nz);
  if (d_n) {
    index_prep_dev_kernel<<<(std::max<uint32_t>(nz, 64) + 255) / 256, 256, 0, c->stream>>>(pl, d_n, zw, nz);
    LAUNCHED(c->stream, "index_prep_dev_kernel");
  } else {
    index_prep_kernel<<<(nz + 255) / 256, 256, 0, c->stream>>>(pl, n, zw, nz);
    LAUNCHED(c->stream, "index_prep_kernel");
  }
  TRY(launch_index_bucketed(c, keys, vals, &pl->n_chain, &pl->status, log2_nbk, okeys, opacked, pl, false, nullptr,
                            true));
  HIPCHK(hipMemcpyAsync(c->h_plan, pl, sizeof(Plan), hipMemcpyDeviceToHost, c->stream));
  HIPCHK(spin_sync(c->stream));
  if (c->h_plan->idx_overflow) return index_global(c, c->h_plan->n_chain, n_index, keys, vals, okeys, opacked);
  *n_index = c->h_plan->n_index;
  return 0;
}

extern "C" int srd_index_build_device(srd_ctx* c, const uint64_t* d_pairs, uint64_t n, uint64_t* d_out_keys,
                                      uint64_t* d_out_packed, uint64_t* n_index) {
  if (!c || !n_index || (n && (!d_pairs || !d_out_keys || !d_out_packed))) { set_err("bad argument"); return SRD_ERR_ARG; }
  if (n >= (1ull << 31)) { set_err("too many pairs"); return SRD_ERR_ARG; }
  HIPCHK(hipSetDevice(c->device));
  *n_index = 0;
  if (!n) return 0;
  TRY(ensure(c, B_MKEY, n * 8));
  TRY(ensure(c, B_MVAL, n * 8));
  deinterleave_kernel<<<blocks(std::min<uint64_t>(n, 1 << 20), 256), 256, 0, c->stream>>>(
      d_pairs, n, P<uint64_t>(c, B_MKEY), P<uint64_t>(c, B_MVAL));
  LAUNCHED(c->stream, "deinterleave_kernel");
  return index_build_sep(c, P<uint64_t>(c, B_MKEY), P<uint64_t>(c, B_MVAL), n, d_out_keys, d_out_packed, n_index);
}

extern "C" int srd_index_hash_device(srd_ctx* c, const uint64_t* d_keys, uint64_t n, uint64_t* d_out, void* stream) {
  if (!c || (n && (!d_keys || !d_out))) { set_err("bad argument"); return SRD_ERR_ARG; }
  if (!n) return 0;
  HIPCHK(hipSetDevice(c->device));
  hipStream_t s = stream_of(c, stream);
  index_hash_kernel<<<(unsigned)std::min<uint64_t>((n + 255) / 256, 8192), 256, 0, s>>>(d_keys, n, d_out);
  LAUNCHED(s, "index_hash_kernel");
  return 0;
}
