// srd_scan_host.hip -- host side of the scan kernel (included by srd_api.hip).
//
// Candidate caps, the scan grid and its partition, the scan's workspace and
// launch, and the per-store load-pattern trial.  Used by both passes of
// srd_validate.hip.

// stores above 2^40 bytes take the WIDE scan (48-bit prev offsets)
constexpr uint64_t kWide = 1ull << 40;
constexpr uint64_t kMaxFile = 1ull << 48;  // packed offsets are 48-bit (key_indexer.rs:12-15, 79-85)
#ifdef SRD_DEBUG_API
constexpr uint32_t kDbgScanOnly = 1u << 30;  // SRD_DEBUG_API timing builds: the optimistic scan alone
#endif
// With timing events, the scan is launched by hipExtLaunchKernel, which
// stamps the events with the kernel's own start and stop (the dispatch
// packet's, as rocprofv3 sees them) instead of marker packets around it: a
// marker recorded on an idle stream before the launch runs while the host is
// still submitting the kernel (+30 us on the bracket), and one after it
// delays the next kernel (~6 us per call).
template <bool FULL>
static void launch_scan(unsigned g, const ScanArgs& a, hipStream_t s, hipEvent_t e0 = nullptr,
                        hipEvent_t e1 = nullptr) {
  const dim3 grid(g), block(scan_nw((int)a.variant) * 64);
  if (a.variant == SCAN_LINES) {  // line-per-lane tile loads (large stores: scan_variant_for)
    if (a.flen > kWide) hipExtLaunchKernelGGL(scan_kernel<FULL, true, SCAN_LINES>, grid, block, 0, s, e0, e1, 0, a);
    else hipExtLaunchKernelGGL(scan_kernel<FULL, false, SCAN_LINES>, grid, block, 0, s, e0, e1, 0, a);
#ifdef SRD_DEBUG_API
  } else if (a.variant == 7) {  // timing-only ablations (scan_kernel's V) inside one context
    hipExtLaunchKernelGGL(scan_kernel<FULL, false, 7>, grid, block, 0, s, e0, e1, 0, a);
  } else if (a.variant == 8) {
    hipExtLaunchKernelGGL(scan_kernel<FULL, false, 8>, grid, block, 0, s, e0, e1, 0, a);
#endif
  } else if (e0) {
    if (a.flen > kWide)
      hipExtLaunchKernelGGL(scan_kernel<FULL, true>, grid, block, 0, s, e0, e1, 0, a);
    else
      hipExtLaunchKernelGGL(scan_kernel<FULL, false>, grid, block, 0, s, e0, e1, 0, a);
  } else if (a.flen > kWide) {
    scan_kernel<FULL, true><<<grid, block, 0, s>>>(a);
  } else {
    scan_kernel<FULL, false><<<grid, block, 0, s>>>(a);
  }
}

// A store of another size starts at the default again; a store within 2x of
// the size whose overflow grew the cap keeps that cap (a dense store would
// otherwise overflow -- and rescan -- on every call).
static void fit_cap(CandCap& k, uint64_t bytes) {
  const bool similar = k.grown_bytes && bytes <= 2 * k.grown_bytes && 2 * bytes >= k.grown_bytes;
  k.cap = similar ? std::max(k.grown_cap, k.floor) : k.floor;
}
static void grow_cap(CandCap& k, uint64_t bytes) {
  k.cap = (uint32_t)std::min<uint64_t>((uint64_t)k.cap * 4, SPAN_BYTES);
  k.grown_cap = k.cap;
  k.grown_bytes = bytes;
}

// the scan grid of `variant` over ns resident spans: blocks (<= blocks per
// CU x CUs) and waves per block (scan_nw / scan_bpc)
static unsigned scan_grid(const Ctx* c, uint32_t variant, uint64_t ns, uint32_t* nw) {
  *nw = (uint32_t)scan_nw((int)variant);
  return (unsigned)std::min<uint64_t>((ns + *nw - 1) / *nw, (uint64_t)c->scan_blocks);
}
static ScanPart scan_part(const Ctx* c, uint64_t s_lo, uint64_t ns, unsigned g, uint32_t nw) {
  ScanPart p{};
  p.s_lo = s_lo;
  p.ns = ns;
  p.g = g;
  p.nw = nw;
  if (nw == 16) {
    for (int q = 0; q < 16; q++) p.wq[q] = c->scan_wq[q];
  } else {  // (the fitted shares are the 16-wave block's) an even split
    for (uint32_t q = 0; q < nw; q++) p.wq[q] = 65536u / nw;
    p.wq[nw - 1] += 65536u - nw * (65536u / nw);
  }
  part_fill_cw(p);
  return p;
}
// (part_max_wave_spans, the bound on the spans of one wave: srd_part.h)

static int alloc_scan(Ctx* c, uint64_t n_tiles, uint64_t n_spans, uint32_t cap) {
  const uint64_t slots = n_spans * cap;
  TRY(ensure(c, B_TILE, n_tiles * 16));
  TRY(ensure(c, B_SPAN_COUNT, (n_spans + 1) * 4));
  TRY(ensure(c, B_SPAN_BASE, (n_spans + 1) * 8));
  TRY(ensure(c, B_CM, slots * 8));
  TRY(ensure(c, B_CREC, slots * 32));
  TRY(ensure(c, B_COUNTERS, 8 * 8));
  TRY(ensure(c, B_WALK, sizeof(WalkState)));
  return 0;
}

// the second half of every candidate record (ScanArgs::c_rec1): B_CREC's
// upper half (its lower half is c_rec), fixed while the buffer is
static u32x4* crec1(Ctx* c) { return P<u32x4>(c, B_CREC) + c->bufs[B_CREC].n / 32; }

// The ScanArgs fields both passes set the same way, after alloc_scan: the
// store, the candidate buffers and counters, and the scan's per-wave results
// and last-block reduction.  The callers add the per-tile / per-span arrays
// (the optimistic pass shifts their bases), wcap, the partition and the
// fields only they use.
static int scan_args(Ctx* c, const uint8_t* d_file, uint64_t flen, uint32_t variant, uint32_t cap, ScanArgs* a) {
  *a = ScanArgs{};
  a->variant = variant;
  a->file = d_file;
  a->flen = flen;
  a->n_tiles = (flen + TILE - 1) / TILE;
  a->n_spans = (a->n_tiles + SPAN_TILES - 1) / SPAN_TILES;
  a->cap = cap;
  a->c_m = P<uint64_t>(c, B_CM);
  a->c_rec = P<u32x4>(c, B_CREC);
  a->c_rec1 = crec1(c);
  a->counters = P<unsigned long long>(c, B_COUNTERS);
  a->filt_hb = (uint32_t)((flen ? flen - 1 : 0) >> 32);
  const uint64_t W = (uint64_t)c->scan_blocks * 32;  // up to 32 waves per CU (scan_grid)
  TRY(ensure(c, B_WTOT, W * 8));
  TRY(ensure(c, B_WROOT, W * 8));
  TRY(ensure(c, B_KTOT, 64));
  TRY(ensure_z(c, B_DONE, 64));  // zero once; the scan's last block resets it
  a->wave_total = P<uint64_t>(c, B_WTOT);
  a->wave_root = P<uint64_t>(c, B_WROOT);
  a->k_total = P<uint64_t>(c, B_KTOT);
  a->done = P<uint32_t>(c, B_DONE);
  return 0;
}

// The scan's tile loads (scan_kernel): coalesced nontemporal loads + an
// in-register transpose (V 0) or round 4's line-per-lane loads (SCAN_LINES).
// Which one streams faster depends on the store and on the box: in round 5's
// same-context A/Bs (profiles/r05/variant_ab_coal_*.txt) the coalesced loads
// were 7.5 % faster on C2, 4.8 % slower on C3 (72.5 GB), and on round 6's
// boxes the line-per-lane loads were also faster on C2 in 2 of 3 contexts
// (profiles/r06/variant_ab_body_stream_c2.txt).  So the optimistic pass
// measures: for each store (span count, grid) its first scan runs coalesced
// and is not counted, the next ones alternate the patterns, each timed on the
// device (the scan's first block start to its last block end, XPart::
// scan_ticks, published with the outcome: no host wait, no event), and the
// pattern with the faster best time is kept for the store: from the fourth
// measured call on as soon as the bests differ by more than TUNE_MARGIN, at
// the eighth in any case (a close call costs little either way); measured
// again every 4096 calls.  srd_ctx_scan_trial reports the two best times.
// SRD_SCAN_LOADS pins a pattern; the debug build's srd_debug_set_scan_variant
// overrides both; the full pass takes the current choice (coalesced before one).
constexpr uint32_t TUNE_WARM = 1, TUNE_TRIAL = 4, TUNE_TRIAL_MAX = 8, TUNE_EVERY = 4096;
constexpr double TUNE_MARGIN = 0.02;
static uint32_t scan_variant_for(const Ctx* c) {
  if (c->scan_variant) return c->scan_variant;
  if (c->loads_pin >= 0) return (uint32_t)c->loads_pin;
  return c->tune.choice == 1 ? (uint32_t)SCAN_LINES : 0u;
}
static uint32_t scan_variant_tune(Ctx* c, uint64_t ns, uint32_t g) {
  if (c->scan_variant) return c->scan_variant;
  if (c->loads_pin >= 0) return (uint32_t)c->loads_pin;
  Ctx::LoadTune& t = c->tune;
  if (t.ns != ns || t.g != g || (t.choice >= 0 && t.calls >= TUNE_WARM + TUNE_TRIAL_MAX + TUNE_EVERY)) {
    t = Ctx::LoadTune{};
    t.ns = ns;
    t.g = g;
  }
  if (t.choice >= 0) return t.choice ? (uint32_t)SCAN_LINES : 0u;
  const uint32_t i = t.calls;  // the trial's order: coalesced (warm-up), then coalesced, lines, coalesced, ...
  return i >= TUNE_WARM && ((i - TUNE_WARM) & 1) ? (uint32_t)SCAN_LINES : 0u;
}
// one optimistic scan of the tuned store done: its pattern and device ticks
// (0: not measured -- XCD-aware shares off)
static void scan_tune_feedback(Ctx* c, uint32_t var, uint64_t ticks) {
  Ctx::LoadTune& t = c->tune;
  const uint32_t i = t.calls++;
  if (t.choice >= 0 || i < TUNE_WARM || !ticks || c->scan_variant || c->loads_pin >= 0) return;
  const int k = var == SCAN_LINES ? 1 : 0;
  if (!t.n[k] || ticks < t.best[k]) t.best[k] = ticks;
  t.n[k]++;
  const uint32_t m = t.n[0] + t.n[1];
  if (m < TUNE_TRIAL || !t.n[0] || !t.n[1]) return;
  const double b0 = (double)t.best[0], b1 = (double)t.best[1];
  if (m >= TUNE_TRIAL_MAX || fabs(b0 - b1) > TUNE_MARGIN * fmin(b0, b1)) t.choice = b1 < b0 ? 1 : 0;
}
