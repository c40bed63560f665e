// srd_validate.hip -- the validate path (included by srd_api.hip): the
// optimistic pass, the full pass, finalize + index, and the two device
// entries srd_validate_index_device / srd_validate_span_device.

// Spin until idx_emit's published words (IdxArgs::pub) all carry this
// call's seq; if the stream completes without them (an error), fail.
static int wait_publish(Ctx* c, uint64_t* w) {
  const uint32_t seq = c->pub_seq;
  volatile const uint64_t* pub = c->h_pub;
  const auto read = [&] {
    bool ok = true;
    for (int i = 0; i < PUB_WORDS; i++) {
      w[i] = pub[i];
      ok = ok && (uint32_t)(w[i] >> 32) == seq;
    }
    return ok;
  };
  for (uint64_t it = 0;; it++) {
    if (read()) return 0;
    if ((it & 1023) == 1023) {
      const hipError_t e = hipStreamQuery(c->stream);
      if (e == hipSuccess) {  // finished: re-read once, the words may have landed meanwhile
        if (read()) return 0;
        set_err("internal: the glue finished without publishing its outcome");
        return SRD_ERR_INTERNAL;
      }
      if (e != hipErrorNotReady) HIPCHK(e);
    }
  }
}

// Core runs over n nodes with parents par: core[g] = something links to g
// (B_CORE); launch_key writes every node's run key into B_DHEAD, and two
// max-scans leave 1 + the head of each core node's run in B_RUNHEAD.
// alloc_dense sized B_CORE, B_DHEAD / B_RUNHEAD and the hipCUB scratch for n.
template <class KeyLaunch>
static int core_runs(Ctx* c, const int64_t* par, uint64_t n, const char* key_name, KeyLaunch launch_key) {
  const unsigned nb = blocks(n, 256);
  uint8_t* core = P<uint8_t>(c, B_CORE);
  uint32_t* key = P<uint32_t>(c, B_DHEAD);
  uint32_t* chead = P<uint32_t>(c, B_RUNHEAD);
  HIPCHK(hipMemsetAsync(core, 0, n, c->stream));
  child_kernel<<<nb, 256, 0, c->stream>>>(par, n, core);
  LAUNCHED(c->stream, "child_kernel");
  launch_key(nb, core, key);
  LAUNCHED(c->stream, key_name);
  TRY(scan_max(c, key, chead, n));
  head_key_kernel<<<nb, 256, 0, c->stream>>>(core, par, chead, n, key);
  LAUNCHED(c->stream, "head_key_kernel");
  return scan_max(c, key, chead, n);
}

// walk state (start) must already be on the device
static int walk_and_mark(Ctx* c, const int64_t* par, const uint64_t* slot, uint64_t n, const uint64_t* map,
                         WalkState* hws) {
  WalkState* ws = P<WalkState>(c, B_WALK);
  uint8_t* core = P<uint8_t>(c, B_CORE);
  TRY(core_runs(c, par, n, "core_key_kernel", [&](unsigned nb, uint8_t* co, uint32_t* key) {
    core_key_kernel<<<nb, 256, 0, c->stream>>>(co, ws, n, key);
  }));
  walk_kernel<<<1, 64, 0, c->stream>>>(par, P<uint32_t>(c, B_RUNHEAD), slot, P<u32x4>(c, B_CREC),
                                       P<uint64_t>(c, B_INTS), ws, n);
  LAUNCHED(c->stream, "walk_kernel");
  TRY(read_small(c, c->stream, {rd(ws, hws)}));
  if (hws->status != 1) return 0;
  mark_kernel<<<blocks(n, 256), 256, 0, c->stream>>>(P<uint64_t>(c, B_INTS), ws, n, core,
                                                     P<uint32_t>(c, B_ONPATH));
  LAUNCHED(c->stream, "mark_kernel");
  HIPCHK(hipMemsetAsync(P<uint32_t>(c, B_ONPATH) + n, 0, 4, c->stream));
  TRY(scan_sum(c, P<uint32_t>(c, B_ONPATH), P<uint32_t>(c, B_CPOS), n + 1));
  scatter_chain_kernel<<<blocks(n, 256), 256, 0, c->stream>>>(P<uint32_t>(c, B_ONPATH), P<uint32_t>(c, B_CPOS), n,
                                                              map, P<uint64_t>(c, B_CHAIN_G));
  LAUNCHED(c->stream, "scatter_chain_kernel");
  uint32_t on_path = 0;
  TRY(read_small(c, c->stream, {rd(P<uint32_t>(c, B_CPOS) + n, &on_path)}));
  hws->chain_len = 1 + (uint64_t)on_path;
  return 0;
}

static int alloc_dense(Ctx* c, uint64_t K) {
  TRY(ensure(c, B_DM, K * 8));
  TRY(ensure(c, B_DPAR, K * 8));
  TRY(ensure(c, B_DSLOT, K * 8));
  TRY(ensure(c, B_DHEAD, K * 4));    // run keys / heads: g + 1 in 32 bits (K < 2^32 - 1: run_scan)
  TRY(ensure(c, B_RUNHEAD, K * 4));
  TRY(ensure(c, B_INTS, K * 16 + 16));
  TRY(ensure(c, B_ONPATH, (K + 1) * 4));
  TRY(ensure(c, B_CPOS, (K + 1) * 4));
  TRY(ensure(c, B_CHAIN_G, (K + 1) * 8));
  TRY(ensure(c, B_CORE, K + 1));
  TRY(ensure_cub(c, K + 1));
  return 0;
}

static int alloc_out(Ctx* c, uint64_t n) {
  TRY(ensure(c, B_O_MO, n * 8));
  TRY(ensure(c, B_O_KH, n * 8));
  TRY(ensure(c, B_O_PREV, n * 8));
  TRY(ensure(c, B_O_START, n * 8));
  TRY(ensure(c, B_O_LEN, n * 8));
  TRY(ensure(c, B_O_CRCST, n * 4));
  TRY(ensure(c, B_O_CRC, n * 4));
  TRY(ensure(c, B_O_OK, n));
  TRY(ensure(c, B_O_PIECES, n * 4));
  TRY(ensure(c, B_O_SUF, n * 4));
  TRY(ensure(c, B_O_SXM, n * 4));
  TRY(ensure(c, B_O_TAIL, n * 4));
  TRY(ensure(c, B_SLOW, n * 8));
  TRY(ensure(c, B_IKEY, n * 8));
  TRY(ensure(c, B_IPACKED, n * 8));
  TRY(ensure(c, B_O_PACKED, n * 8));
  return 0;
}

static void set_out_ptrs(Ctx* c, srd_device_result* out) {
  out->meta_off = P<uint64_t>(c, B_O_MO);
  out->key_hash = P<uint64_t>(c, B_O_KH);
  out->prev_offset = P<uint64_t>(c, B_O_PREV);
  out->payload_start = P<uint64_t>(c, B_O_START);
  out->payload_len = P<uint64_t>(c, B_O_LEN);
  out->crc_stored = P<uint32_t>(c, B_O_CRCST);
  out->crc_computed = P<uint32_t>(c, B_O_CRC);
  out->crc_ok = P<uint8_t>(c, B_O_OK);
  out->index_key_hash = P<uint64_t>(c, B_IKEY);
  out->index_packed = P<uint64_t>(c, B_IPACKED);
}

// The FinArgs fields finish and the optimistic pass set the same way: the
// store, the candidate records and every per-entry output array of alloc_out.
// The callers add the chain, the tile array (the optimistic pass shifts its
// base), coff and where n_bad / n_slow are counted.
static FinArgs fin_args(Ctx* c, const uint8_t* d_file, uint64_t flen, uint32_t flags) {
  FinArgs f{};
  f.file = d_file;
  f.flen = flen;
  f.c_m = P<uint64_t>(c, B_CM);
  f.c_rec = P<u32x4>(c, B_CREC);
  f.c_rec1 = crec1(c);
  f.no_crc = (flags & SRD_FLAG_NO_CRC) ? 1 : 0;
  f.o_mo = P<uint64_t>(c, B_O_MO);
  f.o_kh = P<uint64_t>(c, B_O_KH);
  f.o_prev = P<uint64_t>(c, B_O_PREV);
  f.o_start = P<uint64_t>(c, B_O_START);
  f.o_len = P<uint64_t>(c, B_O_LEN);
  f.o_crc_st = P<uint32_t>(c, B_O_CRCST);
  f.o_crc = P<uint32_t>(c, B_O_CRC);
  f.o_pieces = P<uint32_t>(c, B_O_PIECES);
  f.o_suf = P<uint32_t>(c, B_O_SUF);
  f.o_sxm = P<uint32_t>(c, B_O_SXM);
  f.o_tail = P<uint32_t>(c, B_O_TAIL);
  f.o_ok = P<uint8_t>(c, B_O_OK);
  f.slow_list = P<uint64_t>(c, B_SLOW);
  return f;
}

// finalize + index for a chain of n entries whose chain_g / walk state are set
static int finish(Ctx* c, const uint8_t* d_file, uint64_t flen, uint64_t n, uint32_t flags,
                  srd_device_result* out) {
  TRY(alloc_out(c, n));
  uint64_t* cnt = P<uint64_t>(c, B_COUNTERS);
  HIPCHK(hipMemsetAsync(cnt + 5, 0, 16, c->stream));  // n_slow, n_bad
  FinArgs f = fin_args(c, d_file, flen, flags);
  f.n_chain = n;
  f.chain_g = P<uint64_t>(c, B_CHAIN_G);
  f.slot = P<uint64_t>(c, B_DSLOT);
  f.par = P<int64_t>(c, B_DPAR);
  f.ws = P<WalkState>(c, B_WALK);
  f.tile = P<uint32_t>(c, B_TILE);
  f.coff = 1;
  f.n_slow = (unsigned long long*)(cnt + 5);
  f.n_bad = (unsigned long long*)(cnt + 6);
  if (n) {
    finalize_kernel<<<blocks(n, 256), 256, 0, c->stream>>>(f);
    LAUNCHED(c->stream, "finalize_kernel");
    if (!f.no_crc) {
      slow_kernel<<<2048 / SLOW_WAVES, SLOW_WAVES * 64, 0, c->stream>>>(f);
      LAUNCHED(c->stream, "slow_kernel");
    }
  }
  // ---- KeyIndexer::build (bucketed; the global table if a bucket overflows) ----
  // the counters (n_bad: final after finalize / slow) ride on the build's wait
  TRY(enqueue_counters(c));
  uint64_t nidx = 0;
  TRY(index_build_sep(c, P<uint64_t>(c, B_O_KH), P<uint64_t>(c, B_O_MO), n, P<uint64_t>(c, B_IKEY),
                      P<uint64_t>(c, B_IPACKED), &nidx));
  if (!n) HIPCHK(spin_sync(c->stream));  // index_build_sep waited only for n > 0
  uint64_t h[8];
  counters_landed(c, h);
  out->n_index = nidx;
  out->n_crc_bad = h[6];
  out->n_chain = n;
  set_out_ptrs(c, out);
  return 0;
}

// the full pass's scan (every candidate) and link
static int run_scan(Ctx* c, const uint8_t* d_file, uint64_t flen, uint64_t* K, uint64_t* h) {
  const uint64_t n_tiles = (flen + TILE - 1) / TILE;
  const uint64_t n_spans = (n_tiles + SPAN_TILES - 1) / SPAN_TILES;
  fit_cap(c->cfull, flen);
  while (true) {
    TRY(alloc_scan(c, n_tiles, n_spans, c->cfull.cap));
    TRY(ensure_cub(c, n_spans + 1));
    uint64_t* cnt = P<uint64_t>(c, B_COUNTERS);
    HIPCHK(hipMemsetAsync(cnt, 0, 64, c->stream));
    // the scan writes every span's count; only the scan sentinel needs a zero
    HIPCHK(hipMemsetAsync(P<uint32_t>(c, B_SPAN_COUNT) + n_spans, 0, 4, c->stream));
    ScanArgs a;
    TRY(scan_args(c, d_file, flen, scan_variant_for(c), c->cfull.cap, &a));
    a.tile = P<uint32_t>(c, B_TILE);
    a.span_count = P<uint32_t>(c, B_SPAN_COUNT);
    TRY(ensure(c, B_SPAN_FIRST, (n_spans + 1) * 4));
    a.span_first = P<uint32_t>(c, B_SPAN_FIRST);
    a.wcap = 0;  // the full pass stores records at span * cap + slot
    if (n_spans) {
      uint32_t nw;
      const unsigned g = scan_grid(c, a.variant, n_spans, &nw);
      a.part = scan_part(c, 0, n_spans, g, nw);
      hipEvent_t e0, e1;
      TRY(next_scan_events(c, &e0, &e1));
      launch_scan<true>(g, a, c->stream, e0, e1);
      LAUNCHED(c->stream, "scan_kernel");
    }
    TRY(scan_sum(c, P<uint32_t>(c, B_SPAN_COUNT), P<uint64_t>(c, B_SPAN_BASE), n_spans + 1));
    TRY(read_counters(c, h, P<uint64_t>(c, B_SPAN_BASE) + n_spans, K));
    if (*K >= 0xFFFFFFFFull) { set_err("more than 2^32 - 2 chain-node candidates (full pass)"); return SRD_ERR_ALLOC; }
    if ((uint32_t)h[2] == 0) break;
    if (c->cfull.cap >= SPAN_BYTES) { set_err("candidate overflow"); return SRD_ERR_INTERNAL; }
    grow_cap(c->cfull, flen);
  }
  if (*K) {
    TRY(alloc_dense(c, *K));
    LinkArgs l{};
    l.file = d_file;
    l.flen = flen;
    l.n_spans = n_spans;
    l.cap = c->cfull.cap;
    l.span_count = P<uint32_t>(c, B_SPAN_COUNT);
    l.span_base = P<uint64_t>(c, B_SPAN_BASE);
    l.c_m = P<uint64_t>(c, B_CM);
    l.c_rec = P<u32x4>(c, B_CREC);
    l.d_m = P<uint64_t>(c, B_DM);
    l.d_par = P<int64_t>(c, B_DPAR);
    l.d_slot = P<uint64_t>(c, B_DSLOT);
    link_kernel<<<blocks(n_spans, 256 / LINK_LANES), 256, 0, c->stream>>>(l);
    LAUNCHED(c->stream, "link_kernel");
  } else {
    TRY(alloc_dense(c, 1));
  }
  return 0;
}

static int set_single_root(Ctx* c, uint64_t t) {
  WalkState w{};
  w.status = 1;
  w.chain_len = 1;
  w.root_t = t;
  w.final_len = t;
  HIPCHK(hipMemcpyAsync(P<WalkState>(c, B_WALK), &w, sizeof w, hipMemcpyHostToDevice, c->stream));
  return 0;
}

// ---------------------------------------------------------------------------
// Optimistic pass, sync-free: scan (strong candidates only) -> link -> shape
// check -> chain scatter -> finalize -> bucketed index, all counts on the
// device; one host sync at the end.  *done=false sends the call to the full
// pass (the check could not prove the chain from file_len).
static int alloc_fast(Ctx* c, uint64_t capK, uint32_t log2_nbk) {
  TRY(ensure(c, B_DPAR, capK * 4));
  TRY(ensure_z(c, B_HASCHILD, capK * 4));
  TRY(ensure_z(c, B_HASCHILD2, capK * 4));
  TRY(ensure_z(c, B_CHILDOF, capK * 8));
  TRY(ensure(c, B_FLAG, capK));
  TRY(ensure(c, B_PART, GLUE_BLOCKS * 4));
  TRY(ensure(c, B_PARTEX, CHAIN_BLOCKS * CHAIN_WAVES * 4));
  TRY(ensure_z(c, B_LOOKB, CHAIN_BLOCKS * 8));  // look-back granules: zero = no call's tag
  TRY(ensure(c, B_PLAN, sizeof(Plan)));
  TRY(alloc_out(c, capK + 1));
  TRY(alloc_index(c, capK, log2_nbk));
  return 0;
}

// What the phases of one attempt of the optimistic pass share
struct OptAttempt {
  const uint8_t* d_file;  // absolute file offsets index it (only [span_off, ..) is read)
  uint64_t flen;
  uint32_t flags;
  uint32_t coff;
  uint32_t log2_nbk;     // index buckets: ~IDX_BUCKET_AVG chain entries per bucket
  uint32_t var;          // the scan's load pattern
  uint64_t total_waves;  // scan waves; each one's records are dense in its region of ...
  uint64_t wcap;         // ... wcap = (spans per wave) * cap slots
  uint64_t capK;         // the slot space: total_waves * wcap
  uint32_t wpb;          // scan waves per chain block
  XPart* xp;             // XCD-aware block shares (nullptr: off)
  ScanArgs a;            // the scan's arguments (opt_scan); link2 and the glue read them
};

// The scan of one attempt.  It writes every span's count and (its last block)
// the counters, the wave bases and K; block 0 zeroes the plan.  The per-tile /
// per-span arrays hold the resident range only: their base pointers are
// shifted so kernels index them by absolute tile / span.
static int opt_scan(Ctx* c, OptAttempt& o, const ScanPart& part, unsigned g, uint64_t lo, uint64_t k_lo,
                    uint64_t s_lo) {
  ScanArgs& a = o.a;
  TRY(scan_args(c, o.d_file, o.flen, o.var, c->copt.cap, &a));
  a.part = part;
  a.xp = o.xp;
  a.xp_next = c->xp_par ^ 1u;
  a.tile = P<uint32_t>(c, B_TILE) - 4 * k_lo;
  a.span_count = P<uint32_t>(c, B_SPAN_COUNT) - s_lo;
  a.span_first = P<uint32_t>(c, B_SPAN_FIRST) - s_lo;
  a.wcap = o.wcap;  // c_m / c_rec are wave regions, indexed by the wave of this launch
  a.k_lo = k_lo;
  a.m_lo = lo;
  a.zero_words = P<uint32_t>(c, B_PLAN);
  a.n_zero_words = (uint32_t)(sizeof(Plan) / 4);
  // the link phase (every node claims its parent) and the index bucket fills
  // chain_finalize claims (zeroed by block 0)
  a.d_par = P<int32_t>(c, B_DPAR);
  a.childof = P<unsigned long long>(c, B_CHILDOF);
  a.gen = c->gen;
  a.span_lo = lo;
  a.zero2 = index_zero_words(c, o.log2_nbk, &a.n_zero2);
  hipEvent_t e0, e1;
  TRY(next_scan_events(c, &e0, &e1));
  launch_scan<false>(g, a, c->stream, e0, e1);
  LAUNCHED(c->stream, "scan_kernel");
  return 0;
}

// the glue's shape arguments of one attempt (the rounds set has_child / gen)
static ShapeArgs shape_args(Ctx* c, const OptAttempt& o) {
  ShapeArgs sa{};
  sa.file = o.d_file;
  sa.flen = o.flen;
  sa.Kp = o.a.k_total;
  sa.wave_total = o.a.wave_total;
  sa.wcap = o.wcap;
  sa.n_waves = (uint32_t)o.total_waves;
  sa.wpb = o.wpb;
  sa.n_slots = o.capK;
  sa.coff = o.coff;
  sa.c_m = o.a.c_m;
  sa.d_par = o.a.d_par;
  sa.c_rec = o.a.c_rec;
  sa.childof = P<uint64_t>(c, B_CHILDOF);
  sa.flag = P<uint8_t>(c, B_FLAG);
  sa.part = P<uint32_t>(c, B_PART);
  sa.wpart = P<uint32_t>(c, B_PARTEX);
  sa.counters = P<const unsigned long long>(c, B_COUNTERS);
  sa.plan = P<Plan>(c, B_PLAN);
  sa.zero = index_zero_words(c, o.log2_nbk, &sa.n_zero);  // child2 zeroes the index's bucket fills
  sa.lb_fail = c->lb_fail;
  return sa;
}

// The outcome of one glue round into *hp.  idx_emit publishes it to pinned
// memory when it starts; a proven chain whose index aliases the chain arrays
// needs nothing else (no plan copy is enqueued: the next call's scan would
// queue behind it); anything else copies the whole plan and waits for the
// stream.
static int opt_outcome(Ctx* c, const OptAttempt& o, Plan* hp) {
  if (!(c->timing >= SRD_TIMING_CALL)) {
    uint64_t w[PUB_WORDS];
    TRY(wait_publish(c, w));
    const uint32_t fl = (uint32_t)w[0];
    if ((fl & 0x3ffu) == 0x100u) {  // status 0, aliased index, no bucket overflow
      scan_tune_feedback(c, o.var, (uint32_t)w[6]);
      *hp = Plan{};
      hp->n_chain = (uint32_t)w[1];
      hp->n_index = (uint32_t)w[2];
      hp->n_bad = (uint32_t)w[3];
      hp->K = (uint32_t)w[4];
      hp->top_gap = (uint32_t)w[5];
      hp->idx_alias = 1;
      return 0;
    }
  }
  HIPCHK(hipMemcpyAsync(c->h_plan, P<Plan>(c, B_PLAN), sizeof(Plan), hipMemcpyDeviceToHost, c->stream));
  HIPCHK(spin_sync(c->stream));
  *hp = *c->h_plan;
  return 0;
}

// Shape check, chain, finalize and index of one attempt, behind its scan and
// link2; retried on the device with more prune rounds when false candidates
// chained onto each other.  *hp: the last round's plan.
static int opt_glue(Ctx* c, const OptAttempt& o, Plan* hp) {
  Plan* pl = P<Plan>(c, B_PLAN);
  uint32_t* marks = P<uint32_t>(c, B_HASCHILD);
  uint32_t* marks2 = P<uint32_t>(c, B_HASCHILD2);
  uint32_t mgen = c->gen;
  const uint32_t log2_nbk = o.log2_nbk;
  for (int rounds = 0;; rounds += 2) {
    if (rounds) HIPCHK(hipMemsetAsync(pl, 0, sizeof(Plan), c->stream));  // round 0: zeroed by the scan
    ShapeArgs sa = shape_args(c, o);
    if (rounds == 0) {
      // round 0: the link phase's claims (every node claims its parent) are the
      // core flags and the branch test; no marks
      sa.has_child = nullptr;
      sa.gen = mgen;
    } else {
      if (rounds == 2) {  // the retry's first marks: the nodes the link claims were made on
        sa.gen = mgen;
        marks_from_claims_kernel<<<GLUE_BLOCKS, GLUE_THREADS, 0, c->stream>>>(sa, marks);
        LAUNCHED(c->stream, "marks_from_claims_kernel");
      }
      for (int r = 0; r < 2; r++) {  // two more prune rounds per retry
        sa.has_child = marks;
        sa.gen = mgen;
        const uint32_t g2 = ++c->gen;
        prune_kernel<<<GLUE_BLOCKS, GLUE_THREADS, 0, c->stream>>>(sa, marks2, g2);
        LAUNCHED(c->stream, "prune_kernel");
        std::swap(marks, marks2);
        mgen = g2;
      }
      sa.has_child = marks;
      sa.gen = mgen;
      child2_kernel<<<GLUE_BLOCKS, GLUE_THREADS, 0, c->stream>>>(sa);  // core-only claims
      LAUNCHED(c->stream, "child2_kernel");
    }
    const bool fused = rounds == 0 && c->glue_fused;
    if (!fused) {
      check_kernel<<<CHAIN_BLOCKS, CHAIN_THREADS, 0, c->stream>>>(sa);
      LAUNCHED(c->stream, "check_kernel");
    }
    // ---- plan + chain ranks + per-entry outputs / CRC + index histogram ----
    FinArgs f = fin_args(c, o.d_file, o.flen, o.flags);
    f.tile = o.a.tile;
    f.coff = o.coff;
    f.n_bad = (unsigned long long*)&pl->n_bad;
    f.n_slow = (unsigned long long*)&pl->n_slow;  // zeroed with the plan; idx_dedup runs the slow list
    f.o_packed = P<uint64_t>(c, B_O_PACKED);
    unsigned long long* lb = P<unsigned long long>(c, B_LOOKB);
    if (fused)
      chain_finalize_kernel<true><<<CHAIN_BLOCKS, CHAIN_THREADS, (1u << log2_nbk) * 4, c->stream>>>(
          sa, f, index_args(c, log2_nbk), log2_nbk, lb);
    else
      chain_finalize_kernel<false><<<CHAIN_BLOCKS, CHAIN_THREADS, (1u << log2_nbk) * 4, c->stream>>>(
          sa, f, index_args(c, log2_nbk), log2_nbk, lb);
    LAUNCHED(c->stream, "chain_finalize_kernel");
    // ---- KeyIndexer::build, bucketed ----
    TRY(launch_index_bucketed(c, f.o_kh, f.o_mo, &pl->n_chain, &pl->status, log2_nbk, P<uint64_t>(c, B_IKEY),
                              P<uint64_t>(c, B_IPACKED), pl, true, &f, false, o.xp ? &o.xp->scan_ticks : nullptr));
    if (c->timing >= SRD_TIMING_CALL) {
      HIPCHK(hipEventRecord(c->ev[3], c->stream));  // end of the device work (srd_ctx_timings)
      c->ev3_recorded = true;
    }
    TRY(opt_outcome(c, o, hp));
    if (debug_env()) {
      fprintf(stderr, "plan K=%lu n_chain=%lu root_t=%lu start=%lu n_index=%lu bad=%lu slow=%lu st=%u nroot=%u "
              "troot=%u idxov=%u log2nbk=%u capK=%lu rounds=%d\n",
              (unsigned long)hp->K, (unsigned long)hp->n_chain, (unsigned long)hp->root_t, (unsigned long)hp->start,
              (unsigned long)hp->n_index, (unsigned long)hp->n_bad, (unsigned long)hp->n_slow, hp->status, hp->nroot,
              hp->troot, hp->idx_overflow, log2_nbk, (unsigned long)o.capK, rounds);
    }
    // only a shape / root-count failure can be a false chain; at most 6 extra rounds
    const uint32_t retry_bits = ST_SHAPE | ST_ROOTS;
    if (!(hp->status & retry_bits) || (hp->status & ~retry_bits) || rounds >= 6) return 0;
  }
}

// ---------------------------------------------------------------------------
// Span mode (lo > 0): d_span holds file bytes [span_off, flen) (span_off a
// multiple of SPAN_BYTES, <= lo); the chain must run from flen down to an
// entry whose prev == lo.  Whole file: span_off = lo = 0.
static int optimistic_pass(Ctx* c, const uint8_t* d_span, uint64_t span_off, uint64_t lo, uint64_t flen,
                           uint32_t flags, srd_device_result* out, bool* done) {
  *done = false;
  const uint64_t n_tiles = (flen + TILE - 1) / TILE;
  const uint64_t n_spans = (n_tiles + SPAN_TILES - 1) / SPAN_TILES;
  const uint64_t k_lo = span_off / TILE, s_lo = k_lo / SPAN_TILES;
  const uint64_t nt_rel = n_tiles - k_lo, ns_rel = n_spans - s_lo;
  OptAttempt o{};
  o.d_file = d_span - span_off;
  o.flen = flen;
  o.flags = flags;
  o.coff = lo ? 0u : 1u;
  fit_cap(c->copt, flen - span_off);
  for (int attempt = 0; attempt < 6; attempt++) {
    const uint64_t n_est = std::max<uint64_t>(std::max<uint64_t>(c->last_n, (flen - span_off) / 4096), 1);
    o.log2_nbk = index_log2_buckets(n_est);
    // the scan's partition (ScanPart): total_waves waves of at most spw
    // spans; each wave's records are dense in its region of wcap = spw * cap slots
    // (the variant once: its geometry sizes the partition and the launch;
    // every variant has the same grid)
    uint32_t nw;
    const unsigned g = scan_grid(c, 0, ns_rel, &nw);
    o.var = scan_variant_tune(c, ns_rel, g);
    c->last_loads = o.var == SCAN_LINES ? 1 : o.var == 0 ? 0 : -1;
    ScanPart part = scan_part(c, s_lo, ns_rel, g, nw);
    const bool xpart = c->xpart_on && g <= XP_MAX_BLOCKS;
    o.xp = nullptr;
    if (xpart) {
      TRY(ensure_z(c, B_XPART, sizeof(XPart)));
      o.xp = P<XPart>(c, B_XPART);
      // the table the previous scan's link2 wrote, if it was made for this span count and grid
      if (c->xp_valid && c->xp_ns == ns_rel && c->xp_g == g) part.bs = &o.xp->bs[c->xp_par][0];
    }
    {  // what this scan runs with (srd_ctx_scan_blocks)
      Ctx::LastPart& l = c->xp_last;
      l.any = true;
      l.ns = ns_rel;
      l.g = g;
      l.par = c->xp_par;
      l.src = !part.bs ? SRD_SCAN_BLOCKS_EVEN : c->xp_installed ? SRD_SCAN_BLOCKS_INSTALLED : SRD_SCAN_BLOCKS_MEASURED;
      l.attempts = attempt + 1;
      if (!attempt) l.first_src = l.src;
    }
    o.total_waves = (uint64_t)g * nw;
    const uint64_t spw = part_max_wave_spans(part, xpart);
    o.wcap = spw * c->copt.cap;
    // the glue works in slot space (slot = wave * wcap + record): its parent
    // words are 31-bit; stores above ~1 TiB (or a denser cap) take the full pass
    o.capK = o.total_waves * o.wcap;
    if (o.capK >= c->slot_limit) { out->full_reason = SRD_FULL_SLOT_SPACE; return 0; }
    o.wpb = (uint32_t)((o.total_waves + CHAIN_BLOCKS - 1) / CHAIN_BLOCKS);
    if (o.wpb > BW_MAX) { out->full_reason = SRD_FULL_WAVES; return 0; }
    TRY(alloc_scan(c, nt_rel, std::max<uint64_t>(ns_rel, o.total_waves * spw), c->copt.cap));
    TRY(ensure(c, B_SPAN_FIRST, (ns_rel + 1) * 4));
    TRY(alloc_fast(c, o.capK, o.log2_nbk));
    if (c->gen >= 0xFFFFFFF0u || c->gen == 0) {  // tag wrap: clear the marks once
      c->gen = 0;
      HIPCHK(hipMemsetAsync(P<void>(c, B_HASCHILD), 0, c->bufs[B_HASCHILD].n, c->stream));
      HIPCHK(hipMemsetAsync(P<void>(c, B_HASCHILD2), 0, c->bufs[B_HASCHILD2].n, c->stream));
      HIPCHK(hipMemsetAsync(P<void>(c, B_CHILDOF), 0, c->bufs[B_CHILDOF].n, c->stream));
    }
    ++c->gen;
    TRY(opt_scan(c, o, part, g, lo, k_lo, s_lo));
#ifdef SRD_DEBUG_API
    if (flags & kDbgScanOnly) {  // timing-only ablations: the scan alone, no result
      HIPCHK(hipStreamSynchronize(c->stream));
      *done = true;
      return 0;
    }
#endif
    // every record's node test, parent and claim (slot space), one block per scan wave
    link2_kernel<<<(unsigned)((o.total_waves + LINK_WPB - 1) / LINK_WPB), 256 * LINK_WPB, 0, c->stream>>>(
        o.a, (uint32_t)o.total_waves);
    LAUNCHED(c->stream, "link2_kernel");
    if (o.xp) {  // link2 wrote the next call's block starts into the other half
      c->xp_par ^= 1u;
      c->xp_valid = true;
      c->xp_installed = false;
      c->xp_ns = ns_rel;
      c->xp_g = g;
    }
    Plan hp{};
    TRY(opt_glue(c, o, &hp));
    out->n_candidates = hp.K;
    if (hp.status & ST_OVERFLOW) {
      // (cannot happen: <= one candidate per byte) not provable here
      if (c->copt.cap >= SPAN_BYTES) { out->full_reason = SRD_FULL_CAP; return 0; }
      grow_cap(c->copt, flen - span_off);
      out->full_reason = SRD_FULL_CAP;  // (if the attempts run out)
      continue;
    }
    if (hp.status) {  // not provable here -> full pass (whole file) / unproven (span)
      out->full_reason = (hp.status & ST_LOOKBACK) ? SRD_FULL_LOOKBACK
                         : (hp.status & ST_NOSTART) ? SRD_FULL_NO_START
                                                    : SRD_FULL_UNPROVEN;
      return 0;
    }
    out->full_reason = SRD_FULL_NONE;
    out->final_len = flen - hp.top_gap;  // find_top's start tail (a torn tail within TOP_WINDOW bytes: below flen)
    out->n_chain = hp.n_chain;
    out->n_crc_bad = hp.n_bad;
    out->n_index = hp.n_index;
    c->last_n = hp.n_chain;
    if (hp.idx_overflow) {  // a skewed bucket: the global table
      c->ev3_recorded = false;
      TRY(index_global(c, hp.n_chain, &out->n_index));
      hp.idx_alias = 0;
    }
    set_out_ptrs(c, out);
    if (hp.idx_alias) {  // every entry its key's latest: the index is the chain's own arrays
      out->index_key_hash = P<uint64_t>(c, B_O_KH);
      out->index_packed = P<uint64_t>(c, B_O_PACKED);
    }
    *done = true;
    return 0;
  }
  return 0;
}

// ---------------------------------------------------------------------------
// Full pass: every candidate, the valid status of every node by pointer
// jumping over the core runs, the walk from the best valid node.
static int full_pass(Ctx* c, const uint8_t* d_file, uint64_t flen, uint32_t flags, srd_device_result* out) {
  uint64_t K = 0, h[8];
  out->mode = 1;
  TRY(run_scan(c, d_file, flen, &K, h));
  out->n_candidates = K;
  if (debug_env()) fprintf(stderr, "full pass: K=%lu candidates (reason %lu)\n", (unsigned long)K,
                           (unsigned long)out->full_reason);
  const uint64_t max_root = h[0];
  uint64_t best_g1 = 0, tlin = 0;
  if (K) {
    TRY(ensure(c, B_ST, K));
    TRY(ensure(c, B_JMP, K * 8));
    TRY(ensure(c, B_VFLAG, K * 4));
    const unsigned kb = blocks(K, 256);
    const int64_t* par = P<int64_t>(c, B_DPAR);
    uint8_t* core = P<uint8_t>(c, B_CORE);
    uint32_t* chead = P<uint32_t>(c, B_RUNHEAD);
    uint8_t* st = P<uint8_t>(c, B_ST);
    int64_t* jmp = P<int64_t>(c, B_JMP);
    TRY(core_runs(c, par, K, "core_flag_key_kernel", [&](unsigned nb, uint8_t* co, uint32_t* key) {
      core_flag_key_kernel<<<nb, 256, 0, c->stream>>>(co, K, key);
    }));
    status_init_kernel<<<kb, 256, 0, c->stream>>>(par, core, chead, K, st, jmp);
    LAUNCHED(c->stream, "status_init_kernel");
    uint64_t* cnt = P<uint64_t>(c, B_COUNTERS);
    // pointer jumping over the core run heads: every round doubles how far
    // each unresolved head looks along its chain of runs, so ceil(log2 K) + 1
    // rounds resolve every head.  Rounds run back to back (a round after
    // convergence exits at once) and one more round, with the change flag
    // cleared before it, proves convergence with one host wait: first 12
    // rounds (C2's chain of runs converges in ~10), then 8, 16, ... more
    int rounds = 1;
    while ((1ull << rounds) < K) rounds++;
    TRY(ensure(c, B_RFLAG, 4 * 72));
    unsigned int* rflag = P<unsigned int>(c, B_RFLAG);
    int done_rounds = 0;
    for (int pass = 0; pass < 8; pass++) {
      const int nr = std::max(1, std::min(pass ? 4 << pass : 12, rounds + 1 - done_rounds));
      done_rounds += nr;
      HIPCHK(hipMemsetAsync(rflag, 0, 4 * 72, c->stream));
      for (int r = 0; r < std::min(nr, 70); r++) {
        // a fixed grid (grid-stride): a round after convergence exits at once
        status_round_kernel<<<std::min(kb, 1024u), 256, 0, c->stream>>>(K, core, chead, st, jmp, rflag + r,
                                                                       r ? rflag + r - 1 : nullptr);
        LAUNCHED(c->stream, "status_round_kernel");
      }
      HIPCHK(hipMemsetAsync(cnt + 4, 0, 8, c->stream));
      status_round_kernel<<<std::min(kb, 1024u), 256, 0, c->stream>>>(K, core, chead, st, jmp, (unsigned int*)(cnt + 4),
                                                                     nullptr);
      LAUNCHED(c->stream, "status_round_kernel");
      TRY(read_counters(c, h));
      if (!h[4]) break;
      if (pass == 7) { set_err("internal: pointer jumping did not converge"); return SRD_ERR_INTERNAL; }
    }
    status_spread_core_kernel<<<kb, 256, 0, c->stream>>>(K, core, chead, st);
    LAUNCHED(c->stream, "status_spread_core_kernel");
    status_spread_leaf_kernel<<<kb, 256, 0, c->stream>>>(K, par, core, st);
    LAUNCHED(c->stream, "status_spread_leaf_kernel");
    const unsigned vb = blocks(K, 256);
    TRY(ensure(c, B_JMP, std::max<uint64_t>(K, vb) * 8));  // per-block maxima (the jump pointers are dead now)
    valid_max_kernel<<<vb, 256, 0, c->stream>>>(P<uint8_t>(c, B_ST), K, P<uint64_t>(c, B_JMP), P<uint32_t>(c, B_VFLAG));
    LAUNCHED(c->stream, "valid_max_kernel");
    max_reduce_kernel<<<1, 1024, 0, c->stream>>>(P<uint64_t>(c, B_JMP), vb, (unsigned long long*)(cnt + 3),
                                                 P<uint64_t>(c, B_DM), (unsigned long long*)(cnt + 7));
    LAUNCHED(c->stream, "max_reduce_kernel");
    TRY(read_counters(c, h));
    best_g1 = h[3];
    if (best_g1) tlin = h[7] + 20;  // d_m[best_g1 - 1] + 20
  }
  const uint64_t final_len = std::max(tlin, max_root);
  out->final_len = final_len;
  if (final_len == 0) return finish(c, d_file, flen, 0, flags, out);
  if (final_len == max_root && max_root > tlin) {
    TRY(set_single_root(c, final_len));
    return finish(c, d_file, flen, 1, flags, out);
  }
  // compact the valid nodes, walk from the best one
  TRY(ensure(c, B_VLIST, K * 8));
  TRY(ensure(c, B_NV, 8));
  TRY(ensure(c, B_VPOS, K * 8));
  TRY(ensure(c, B_VPAR, K * 8));
  TRY(ensure(c, B_VSLOT, K * 8));
  // valid nodes in dense order: an exclusive scan of the flags, then one
  // scatter writes vlist[pos] = g, vpos[g] = pos and nv (no host wait before
  // the remap: its grid covers K and stops at nv on the device)
  TRY(ensure(c, B_VSCAN, K * 4));
  TRY(scan_sum(c, P<uint32_t>(c, B_VFLAG), P<uint32_t>(c, B_VSCAN), K));
  compact_valid_kernel<<<blocks(K, 256), 256, 0, c->stream>>>(P<uint32_t>(c, B_VFLAG), P<uint32_t>(c, B_VSCAN), K,
                                                              P<uint64_t>(c, B_VLIST), P<uint64_t>(c, B_VPOS),
                                                              P<uint64_t>(c, B_NV));
  LAUNCHED(c->stream, "compact_valid_kernel");
  remap_kernel<<<blocks(K, 256), 256, 0, c->stream>>>(P<uint64_t>(c, B_VLIST), P<uint64_t>(c, B_NV),
                                                      P<int64_t>(c, B_DPAR), P<uint64_t>(c, B_VPOS),
                                                      P<int64_t>(c, B_VPAR), P<uint64_t>(c, B_VSLOT),
                                                      P<uint64_t>(c, B_DSLOT));
  LAUNCHED(c->stream, "remap_kernel");
  // the walk starts at the best node's compacted position
  walk_start_kernel<<<1, 64, 0, c->stream>>>(P<WalkState>(c, B_WALK), P<uint64_t>(c, B_VPOS), best_g1 - 1);
  LAUNCHED(c->stream, "walk_start_kernel");
  uint64_t nv = 0;
  TRY(read_small(c, c->stream, {rd(P<uint64_t>(c, B_NV), &nv)}));
  WalkState hw{};
  TRY(walk_and_mark(c, P<int64_t>(c, B_VPAR), P<uint64_t>(c, B_VSLOT), nv, P<uint64_t>(c, B_VLIST), &hw));
  if (hw.status != 1) { set_err("internal: valid walk did not reach a root"); return SRD_ERR_INTERNAL; }
  return finish(c, d_file, flen, hw.chain_len, flags, out);
}

// argument checks, the store too short for any entry, then the optimistic
// pass and, where it cannot prove the chain, the full pass
static int validate_device_impl(srd_ctx* c, const uint8_t* d_file, uint64_t flen, uint32_t flags,
                                srd_device_result* out) {
  if (!c || !out || (!d_file && flen)) { set_err("bad argument"); return SRD_ERR_ARG; }
  if (flen > kMaxFile) { set_err("stores above 2^48 bytes cannot be indexed (48-bit packed offsets)"); return SRD_ERR_ARG; }
  HIPCHK(hipSetDevice(c->device));
  memset(out, 0, sizeof *out);
  out->file_len = flen;
  if (flen < 21) {  // no tail can be valid (recover_valid_chain :384-386, t>=21)
    TRY(alloc_dense(c, 1));
    TRY(alloc_scan(c, 1, 1, c->copt.cap));
    return finish(c, d_file, flen, 0, flags, out);
  }
  if (flags & SRD_FLAG_FORCE_FULL) {
    out->full_reason = SRD_FULL_FORCED;
  } else {
    // optimistic pass: strong candidates only; valid iff the chain from
    // file_len is proven through recorded nodes
    bool done = false;
    TRY(optimistic_pass(c, d_file, 0, 0, flen, flags, out, &done));
    if (done) return 0;
  }
  return full_pass(c, d_file, flen, flags, out);
}

// The call bracket of the two validate entries.  call_begin: the device, the
// call-timing state and ev[2] (a wait for the caller's input would go here).
// call_end: ev[3] and the wait for the stream -- not when the pass has waited
// for its outcome already (synced) -- and the elapsed time.
static int call_begin(Ctx* c) {
  HIPCHK(hipSetDevice(c->device));
  c->total_ms = 0;
  c->ev3_recorded = false;
  if (c->timing >= SRD_TIMING_CALL) HIPCHK(hipEventRecord(c->ev[2], c->stream));
  return 0;
}
static int call_end(Ctx* c, bool synced) {
  const bool tcall = c->timing >= SRD_TIMING_CALL;
  if (!synced) {
    if (tcall) {
      HIPCHK(hipEventRecord(c->ev[3], c->stream));
      HIPCHK(hipEventSynchronize(c->ev[3]));
    } else {
      HIPCHK(spin_sync(c->stream));
    }
  }
  if (tcall) {
    float ms = 0;
    HIPCHK(hipEventElapsedTime(&ms, c->ev[2], c->ev[3]));
    c->total_ms = ms;
  }
  return 0;
}

extern "C" int srd_validate_index_device(srd_ctx* c, const uint8_t* d_file, uint64_t flen, uint32_t flags,
                                         srd_device_result* out) {
  if (!c) { set_err("bad argument"); return SRD_ERR_ARG; }
  TRY(call_begin(c));
  const int r = validate_device_impl(c, d_file, flen, flags, out);
  // the optimistic pass returns with its outcome read: nothing to wait for,
  // unless the call is timed and the pass did not record ev[3] itself
  const bool synced =
      r == 0 && out->mode == SRD_MODE_OPTIMISTIC && (c->ev3_recorded || c->timing < SRD_TIMING_CALL);
  TRY(call_end(c, synced));
  return r;
}

extern "C" int srd_validate_span_device(srd_ctx* c, const uint8_t* d_span, uint64_t span_off, uint64_t lo,
                                        uint64_t hi, uint32_t flags, srd_device_result* out) {
  if (!c || !out || !d_span) { set_err("bad argument"); return SRD_ERR_ARG; }
  if (lo == 0) {
    if (span_off) { set_err("bad argument: a span starting at tail 0 is the whole file (span_off must be 0)"); return SRD_ERR_ARG; }
    return srd_validate_index_device(c, d_span, hi, flags, out);
  }
  if (span_off % SPAN_BYTES || span_off > lo || hi < lo + 21 || hi > kMaxFile) {
    set_err("bad span: need span_off % 16384 == 0, span_off <= lo, lo + 21 <= hi <= 2^48");
    return SRD_ERR_ARG;
  }
  TRY(call_begin(c));
  memset(out, 0, sizeof *out);
  out->file_len = hi;
  bool done = false;
  const int r = optimistic_pass(c, d_span, span_off, lo, hi, flags, out, &done);
  if (!r && !done) {
    out->mode = SRD_MODE_SPAN_UNPROVEN;
    out->final_len = 0;
    out->n_chain = 0;
    out->n_index = 0;
    out->n_crc_bad = 0;
  }
  TRY(call_end(c, false));
  return r;
}
