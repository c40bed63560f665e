// srd_ctx.hip -- the context and its workspace (included by srd_api.hip).
//
// Error reporting (g_err, HIPCHK / TRY, the launch check LAUNCHED), the
// context struct and its buffer table, the CRC table upload, the small helpers
// every host file uses (spin_sync, stream_of, the pinned read-back read_small
// and the validate counters, the hipCUB wrappers: the only users of h_small
// and B_CUB_TMP), the environment knobs, srd_ctx_create / destroy / getters
// and the timing entries.
static thread_local std::string g_err;
static void set_err(const std::string& s) { g_err = s; }

#define HIPCHK(x)                                                                         \
  do {                                                                                    \
    hipError_t e_ = (x);                                                                  \
    if (e_ != hipSuccess) {                                                               \
      set_err(std::string(#x) + ": " + hipGetErrorString(e_));                            \
      return SRD_ERR_HIP;                                                                 \
    }                                                                                     \
  } while (0)

namespace {

#define TRY(x)                 \
  do {                         \
    int r_ = (x);              \
    if (r_) return r_;         \
  } while (0)

// The check behind every kernel launch and hipCUB call on stream s: the launch
// error, always; with SRD_SYNC_DEBUG=1 (a debugging aid, read once per
// process) also a wait for s -- the stream the kernel went to -- and the name
// of the kernel that failed.
static int launched(hipStream_t s, const char* name) {
  static const bool sync = [] { const char* e = getenv("SRD_SYNC_DEBUG"); return e && *e && *e != '0'; }();
  HIPCHK(hipGetLastError());
  if (!sync) return 0;
  hipError_t e = hipStreamSynchronize(s);
  if (e == hipSuccess) e = hipGetLastError();
  if (e == hipSuccess) return 0;
  set_err(std::string("kernel ") + name + ": " + hipGetErrorString(e));
  fprintf(stderr, "srd: kernel %s failed: %s\n", name, hipGetErrorString(e));
  return SRD_ERR_HIP;
}
#define LAUNCHED(s, name) TRY(launched(s, name))

struct Buf {
  void* p = nullptr;
  size_t n = 0;
};

// Candidate record slots per span; grow x4 on overflow and are remembered by
// the context for stores of a similar size.  The optimistic pass starts at 8
// (a C2 span holds ~4 records): its 4096 scan waves write their records into
// regions of spans x cap slots, and with 64 slots the regions were 135 KiB
// apart (a 604 MB record buffer for C2) -- on the first-allocated workspace of
// a process that cost 6-8 % of the scan (same-box A/B, profiles/r03/
// scan_record_regions_ab.txt); at 8 the regions are 17 KiB apart and every
// placement runs at the fast rate.
struct CandCap {
  uint32_t cap;          // slots per span
  uint32_t grown_cap;    // the cap the last overflow needed ...
  uint64_t grown_bytes;  // ... for a store (span) of this many bytes
  uint32_t floor;        // the default (a store of another size starts here again)
};

// A context's persistent host thread (the multi-GPU open runs each shard's
// work on its context's worker: no thread spawn / join per phase).  One job
// at a time; post() then wait().
struct Worker {
  std::thread th;
  std::mutex mu;
  std::condition_variable cv;
  std::function<void()> job;
  bool has = false, stop = false;
  Worker() {
    th = std::thread([this] {
      std::unique_lock<std::mutex> lk(mu);
      for (;;) {
        cv.wait(lk, [this] { return has || stop; });
        if (!has) return;  // stop
        lk.unlock();
        job();
        lk.lock();
        has = false;
        job = nullptr;
        cv.notify_all();
      }
    });
  }
  ~Worker() {
    {
      std::lock_guard<std::mutex> lk(mu);
      stop = true;
    }
    cv.notify_all();
    th.join();
  }
  void post(std::function<void()> f) {
    std::lock_guard<std::mutex> lk(mu);
    job = std::move(f);
    has = true;
    cv.notify_all();
  }
  void wait() {
    std::unique_lock<std::mutex> lk(mu);
    cv.wait(lk, [this] { return !has; });
  }
};

struct Ctx {
  int device = 0;
  hipStream_t stream = nullptr;
  std::vector<Buf> bufs;  // indexed by the enum below
  // candidate slots per span (4 tiles) of the optimistic pass's scan and of
  // the full pass's (CandCap): each scan wave's records are dense in a region
  // of (its spans x cap) slots, so the cap sets how far apart the waves'
  // record stores land -- see CandCap
  CandCap copt{8, 8, 0, 8};
  CandCap cfull{32, 32, 0, 32};
  unsigned scan_blocks = 256;  // persistent scan grid (one 16-wave block per CU)
  unsigned scan_cus = 256;
  uint32_t scan_wq[16] = {};  // ScanPart::wq (scan_weights())
  uint32_t scan_variant = 0;  // ScanArgs::variant (srd_debug_set_scan_variant)
  // the optimistic pass's slot-space bound (the glue's parent words are 31-bit):
  // 2^31; SRD_SLOT_LIMIT_LOG2 (10..31, read at srd_ctx_create) lowers it so the
  // SRD_FULL_SLOT_SPACE fallback can be tested on a small store
  uint64_t slot_limit = 1ull << 31;
  // the scan's tile loads: SRD_SCAN_LOADS pins one pattern (0 coalesced +
  // transpose, SCAN_LINES line per lane); -1 = chosen per store by measuring
  // both (LoadTune, scan_variant_tune)
  int loads_pin = -1;
  int last_loads = -1;  // srd_ctx_scan_loads: the last optimistic scan's pattern
  struct LoadTune {
    uint64_t ns = ~0ull;       // the store (resident spans, grid) the state is for
    uint32_t g = 0;
    uint32_t calls = 0;        // optimistic scans of this store so far
    uint64_t best[2] = {0, 0};  // the fastest scan of each pattern, ticks (0 coalesced, 1 line per lane)
    uint32_t n[2] = {0, 0};
    int choice = -1;           // -1: still measuring
  } tune;
  // round 0 of the optimistic pass runs the shape check inside
  // chain_finalize_kernel<true> (look-back ranks) instead of check_kernel +
  // chain_finalize_kernel<false>; srd_debug_set_glue_fused A/Bs the two
  bool glue_fused = true;
  // test knobs read at srd_ctx_create: SRD_GLUE_FUSED=0 (round 0 through
  // check_kernel + chain_finalize_kernel<false>, the retry rounds' shape) and
  // SRD_LB_FAIL_BLOCK=b (chain block b's look-back treated as timed out)
  uint32_t lb_fail = ~0u;
  // XCD-aware block shares of the optimistic scan (XPart, B_XPART; SRD_XPART=0
  // at srd_ctx_create turns them off): the parity of the table the next scan
  // reads, and the span count / grid the table was made for
  bool xpart_on = true, xp_valid = false;
  uint32_t xp_par = 0, xp_g = 0;
  uint64_t xp_ns = 0;
  // diagnostics (srd_ctx_set_scan_blocks / srd_ctx_scan_blocks): the table
  // the next scan reads was installed by the caller; and what the last
  // optimistic scan ran with -- its resident spans and grid, where its block
  // starts came from (SRD_SCAN_BLOCKS_*) and the half of XPart::bs it read
  bool xp_installed = false;
  struct LastPart {
    bool any = false;
    uint64_t ns = 0;
    uint32_t g = 0, src = 0, par = 0;
    uint32_t attempts = 0, first_src = 0;  // of the call that scan belonged to: its scans, the first one's source
  } xp_last;
  srd_device_result res{};
  // host-input staging
  Buf file;
  // timing (HIP events on `stream`)
  hipEvent_t ev[4] = {nullptr, nullptr, nullptr, nullptr};
  // srd_ctx_set_timing: 0 none (default), 1 scan kernel (a ring of start /
  // stop pairs stamped by the scan dispatches), 2 + whole call (ev[2],
  // ev[3]).  The scan pairs are read out when srd_ctx_timings asks (or when
  // the ring wraps), not inside the calls: hipEventElapsedTime per call was
  // host time on every call's critical path
  int timing = SRD_TIMING_NONE;
  static constexpr uint32_t kScanRing = 64;
  hipEvent_t sev[2 * kScanRing] = {};
  uint32_t sev_next = 0, sev_pending = 0;  // next pair, pairs not yet read out
  double scan_ms = 0, total_ms = 0;  // scan_ms / scan_launches: since the last srd_ctx_timings
  int scan_launches = 0;
  uint32_t timing_every = 1, timing_seq = 0;  // srd_ctx_set_timing_every
  // the individual scan durations behind scan_ms (scan_list), and those of
  // the last srd_ctx_timings read (scan_last: srd_ctx_scan_list)
  std::vector<float> scan_list, scan_last;
  // sync-free optimistic pass
  uint32_t gen = 0;     // generation tag of has_child / childof
  uint64_t last_n = 0;  // chain length of the previous call (index bucket sizing)
  Plan* h_plan = nullptr;  // pinned host copy
  uint64_t* h_pub = nullptr;  // pinned: idx_emit's published outcome (IdxArgs::pub)
  uint64_t* h_small = nullptr;  // pinned: small device reads (counters, K, ...): async copies, one wait
  uint32_t pub_seq = 0;
  // batch writer (srd_batch_write): side copy stream, double-buffer events,
  // pinned entry tables and pinned bounce buffers (non-contiguous inputs)
  hipStream_t cstream = nullptr;
  hipEvent_t wev_copied[2] = {nullptr, nullptr}, wev_done[2] = {nullptr, nullptr};
  void* pin_ent[2] = {nullptr, nullptr};
  // host-input staging (stage_host): bounce buffers, one stream per worker
  int stage_workers = 8;
  int stage_mode = -1;  // last call: 0 pinned input, 1 registered, 2 bounce buffers, 3 pageable
  double stage_ms = 0;  // host wall time of the last staging
  bool ev3_recorded = false;  // the optimistic pass recorded ev[3] before its final sync
  std::vector<void*> stage_pin;
  std::vector<hipStream_t> stage_streams;
  std::vector<hipEvent_t> stage_ev;
  srd_multi_summary last_multi{};  // the last multi-GPU open with this context as ctxs[0]
  std::vector<double> last_shard_ms;  // its per-shard validate times (srd_ctx_multi_shard_ms)
  void* h_out = nullptr;  // pinned host result arrays (srd_validate_index / _multi)
  uint64_t h_out_n = 0;
  uint8_t lgen = 0;  // generation of the index build's non-latest marks (B_LATEST8)
  // multi-GPU open: the context's persistent host worker (created on first
  // use) and the event every cross-context copy out of this context's memory
  // waits on (recorded on `stream` once the data it reads is enqueued)
  Worker* worker = nullptr;
  hipEvent_t ev_ready = nullptr;
  bool ready_recorded = false;
};

enum BufId {
  B_TILE, B_SPAN_COUNT, B_SPAN_BASE,
  B_CM, B_CREC,
  B_COUNTERS,  // [0]=max_root [1]=start tail (find_top) [2]=overflow [3]=best_g1 [4]=changed [5]=n_slow [6]=n_bad [7]=special
  B_DM, B_DPAR, B_DSLOT, B_DHEAD, B_RUNHEAD, B_INTS, B_WALK,
  B_ST, B_JMP, B_VFLAG, B_VLIST, B_NV, B_VPOS, B_VPAR, B_VHEAD, B_VSLOT,
  B_ONPATH, B_CPOS, B_CHAIN_G, B_CORE,
  B_O_MO, B_O_KH, B_O_PREV, B_O_START, B_O_LEN, B_O_CRCST, B_O_CRC, B_O_OK,
  B_O_PIECES, B_O_SUF, B_O_SXM, B_O_TAIL, B_SLOW,
  B_HKEYS, B_HVALS, B_LATEST, B_IPOS, B_IKEY, B_IPACKED,
  B_CUB_TMP,
  B_PLAN, B_HASCHILD, B_CHILDOF, B_FLAG, B_PART, B_PARTEX, B_HOFF, B_SKEY, B_SIDX, B_LATEST8, B_XPART,
  B_MPLAN, B_MKEY, B_MVAL, B_PCNT, B_POFF, B_HASCHILD2,
  B_WPAY0, B_WPAY1, B_WKEY0, B_WKEY1, B_WENT0, B_WENT1, B_WKH, B_WMO,
  B_IT_FLAG, B_IT_POS, B_IT_ST, B_IT_EN, B_IT_KEPT, B_IT_OST, B_IT_OEN, B_IT_OKH, B_IT_ENT, B_IT_RLEN, B_IT_PST,
  B_GKEY, B_GVAL, B_GOKEY, B_GOPACKED,
  B_WTOT, B_WROOT, B_KTOT, B_DONE, B_SPAN_FIRST,
  B_XKEY, B_XVAL, B_GATHER, B_RFLAG, B_O_PACKED, B_VSCAN, B_LOOKB, B_PROBE, B_XTOT,
  B_LV_DSLOT, B_LV_DTOMB, B_LV_LSLOT, B_LV_OPS, B_LV_OPV, B_LV_CNT,  // live table: apply
  B_LV_XK, B_LV_XP, B_LV_FLAG, B_LV_POS, B_LV_ENT, B_LV_TOMB,        // export, batched delete
  B_GA_ST, B_GA_PLEN, B_GA_CHK, B_GA_OFF, B_GA_CPRE, B_GA_CNT, B_GA_RAW, B_GA_CRC,  // payload gather
  B_ST_UNIT,  // the streaming kernel's unit descriptors, whoever builds them
  B_AP_END, B_AP_NZ,  // device append (on top of the gather's)
  B_CL_XK, B_CL_XP, B_CL_LEN, B_CL_MO, B_CL_PACKED, B_CL_CNT,  // live compaction (on top of the export's, the iterator's and the append's)
  B_SG_SRC, B_SG_LEN, B_SG_OFF, B_SG_UN, B_SG_UPRE, B_SG_ENT,  // segment append (on top of the append's)
  B_TT_CNT, B_TT_XQ, B_TT_FLAG, B_TT_POS,  // TTL eviction and sweep (on top of the delete's, the apply's and the export's)
  // rows read (srd_read_rows_device): its own buffers, the scan's scratch included, which no other entry
  // grows or moves -- a captured read holds their addresses
  B_RW_START, B_RW_END, B_RW_EUN, B_RW_OFF, B_RW_UPRE, B_RW_CRC, B_RW_ST, B_RW_CNT, B_RW_UNIT, B_RW_RAW, B_RW_TMP,
  B_COUNT_
};

int ensure(Ctx* c, BufId id, size_t bytes) {
  Buf& b = c->bufs[id];
  if (b.n >= bytes && b.p) return 0;
  if (b.p) HIPCHK(hipFree(b.p));
  b.p = nullptr;
  b.n = 0;
  size_t want = std::max<size_t>(bytes, 256);
  if (hipMalloc(&b.p, want) != hipSuccess) {
    set_err("hipMalloc failed for " + std::to_string(want) + " bytes");
    b.p = nullptr;
    return SRD_ERR_ALLOC;
  }
  b.n = want;
  return 0;
}
template <class T>
T* P(Ctx* c, BufId id) { return (T*)c->bufs[id].p; }

// ensure + zero-fill whenever the buffer is (re)allocated
int ensure_z(Ctx* c, BufId id, size_t bytes) {
  void* before = c->bufs[id].p;
  size_t nb = c->bufs[id].n;
  int r = ensure(c, id, bytes);
  if (r) return r;
  if (c->bufs[id].p != before || c->bufs[id].n != nb) HIPCHK(hipMemsetAsync(c->bufs[id].p, 0, c->bufs[id].n, c->stream));
  return 0;
}

// the host CRC tables, built on first use
const CrcTables& host_tabs() {
  static CrcTables t;
  static const bool built = (build_crc_tables(t), true);
  (void)built;
  return t;
}

int upload_tables() {
  static std::mutex mu;
  std::lock_guard<std::mutex> lk(mu);
  const CrcTables& ht = host_tabs();
  // per device upload
  int dev = 0;
  HIPCHK(hipGetDevice(&dev));
  static uint64_t uploaded = 0;
  if (uploaded & (1ull << dev)) return 0;
  DevTables t;
  memcpy(t.tab, ht.tab, sizeof t.tab);
  memcpy(t.lw, ht.lw, sizeof t.lw);
  memcpy(t.winit, ht.winit, sizeof t.winit);
  memcpy(t.zero_crc, ht.zero_crc, sizeof t.zero_crc);
  t.x32768 = ht.x32768;
  t.xtile[0] = kX0;
  for (int e = 1; e <= 64; e++) t.xtile[e] = mulp(ht.x32768, t.xtile[e - 1]);
  t.xt64[0] = kX0;
  for (int q = 1; q <= 64; q++) t.xt64[q] = mulp(t.xtile[64], t.xt64[q - 1]);
  for (int tb = 0; tb < 4; tb++)
    for (int b = 0; b < 256; b++) t.mx64[tb][b] = mulp(t.xtile[64], (uint32_t)b << (8 * tb));
  memcpy(t.pow8, ht.pow8, sizeof t.pow8);
  memcpy(t.invpow, ht.invpow, sizeof t.invpow);
  memcpy(t.m16k, ht.m16k, sizeof t.m16k);
  memcpy(t.m32k, ht.m32k, sizeof t.m32k);
  memcpy(t.mtk, ht.mtk, sizeof t.mtk);
  for (int pos = 0; pos < 8; pos++)
    for (int nb = 0; nb < 16; nb++)
      for (int l = 0; l < 32; l++)  // x^(512*(31-l)) = lw[l + 32]
        t.nib[((pos * 16 + nb) << 5) + l] = mulp(ht.lw[l + 32], (uint32_t)nb << (4 * pos));
  {
    for (int tb = 0; tb < 4; tb++)
      for (int b = 0; b < 256; b++) {
        for (int q = 0; q < 3; q++) {
          t.last[q][tb][b] = mulp(host_xpow8(ht, 4 + 16 * (3 - q)), (uint32_t)b << (8 * tb));
          t.last_c[q][tb][b] = mulp(host_xpow8(ht, 4 + 1024 * (3 - q)), (uint32_t)b << (8 * tb));
        }
        t.m4096[tb][b] = mulp(host_xpow8(ht, 512), (uint32_t)b << (8 * tb));
      }
    for (int pos = 0; pos < 8; pos++)
      for (int nb = 0; nb < 16; nb++)
        for (int l = 0; l < 32; l++)
          t.nib_c[((pos * 16 + nb) << 5) + l] = mulp(host_xpow8(ht, 16 * (31 - l)), (uint32_t)nb << (4 * pos));
  }
  HIPCHK(hipMemcpyToSymbol(HIP_SYMBOL(g_tabs), &t, sizeof t));
  uploaded |= 1ull << dev;
  return 0;
}

inline unsigned blocks(uint64_t n, unsigned t) { return (unsigned)((n + t - 1) / t); }

// hipCUB temp size for all glue ops up to n elements
int ensure_cub(Ctx* c, uint64_t n) {
  size_t t1 = 0, t2 = 0, t3 = 0, t4 = 0, t5 = 0;
  int nn = (int)std::min<uint64_t>(n + 1, 0x7fffffff);
  hipcub::DeviceScan::ExclusiveSum(nullptr, t1, (uint32_t*)nullptr, (uint64_t*)nullptr, nn);
  hipcub::DeviceScan::InclusiveScan(nullptr, t2, (uint32_t*)nullptr, (uint32_t*)nullptr, hipcub::Max(), nn);
  hipcub::DeviceScan::ExclusiveSum(nullptr, t3, (uint32_t*)nullptr, (uint32_t*)nullptr, nn);
  hipcub::DeviceSelect::Flagged(nullptr, t4, hipcub::CountingInputIterator<uint64_t>(0), (uint32_t*)nullptr,
                                (uint64_t*)nullptr, (uint64_t*)nullptr, nn);
  t5 = std::max(std::max(t1, t2), std::max(t3, t4));
  return ensure(c, B_CUB_TMP, t5 + 256);
}
static bool debug_env() {
  static const bool v = [] { const char* e = getenv("SRD_DEBUG"); return e && *e && *e != '0'; }();
  return v;
}

// Wait for the stream by polling (the call's result is on the host's
// critical path: a blocking wait's wake-up adds tens of us per call)
static hipError_t spin_sync(hipStream_t s) {
  hipError_t e;
  while ((e = hipStreamQuery(s)) == hipErrorNotReady) {
  }
  return e;
}
// the stream of an entry that takes one (nullptr = the context's)
static hipStream_t stream_of(Ctx* c, void* stream) { return stream ? (hipStream_t)stream : c->stream; }

// Small device reads go through the pinned h_small (a copy into pageable
// memory would wait by itself): words [0, 8) are the validate counters',
// words [8, 32) serve one read_small at a time, which enqueues its reads on
// s, waits once and hands the values to their destinations -- nothing is left
// in the pinned area, so a caller may hold values across another such read.
struct SmallRead {
  const void* src;  // device
  void* dst;        // host
  size_t bytes;     // 0: skipped
};
template <class T>
static SmallRead rd(const T* src, T* dst) { return SmallRead{src, dst, sizeof(T)}; }
static int read_small(Ctx* c, hipStream_t s, std::initializer_list<SmallRead> reads) {
  uint64_t* w = c->h_small + 8;  // each read takes whole words
  for (const SmallRead& r : reads) {
    if (w + (r.bytes + 7) / 8 > c->h_small + 32) { set_err("internal: read_small over its pinned area"); return SRD_ERR_INTERNAL; }
    if (r.bytes) HIPCHK(hipMemcpyAsync(w, r.src, r.bytes, hipMemcpyDeviceToHost, s));
    w += (r.bytes + 7) / 8;
  }
  HIPCHK(spin_sync(s));
  w = c->h_small + 8;
  for (const SmallRead& r : reads) {
    if (r.bytes) memcpy(r.dst, w, r.bytes);
    w += (r.bytes + 7) / 8;
  }
  return 0;
}
// The 8 validate counters into h_small[0, 8).  Two phases where the copy rides
// on somebody else's wait (finish: the index build's); read_counters = both
// with a wait of its own, which one more u64 (extra_src, nullable) shares.
static int enqueue_counters(Ctx* c) {
  HIPCHK(hipMemcpyAsync(c->h_small, P<uint64_t>(c, B_COUNTERS), 8 * 8, hipMemcpyDeviceToHost, c->stream));
  return 0;
}
static void counters_landed(Ctx* c, uint64_t* h) { memcpy(h, c->h_small, 64); }
int read_counters(Ctx* c, uint64_t* h, const uint64_t* extra_src = nullptr, uint64_t* extra = nullptr) {
  TRY(enqueue_counters(c));
  if (extra_src) TRY(read_small(c, c->stream, {rd(extra_src, extra)}));
  else HIPCHK(spin_sync(c->stream));
  counters_landed(c, h);
  return 0;
}

// hipCUB on stream s (nullptr = the context's) with the scratch in B_CUB_TMP,
// which the caller sized before: ensure_cub (the validate passes) or
// ensure_scan (one exclusive sum of these types); sort_pairs48 sizes it itself.
template <class In, class Out>
static int ensure_scan(Ctx* c, In in, Out out, uint64_t n) {
  size_t tb = 0;
  HIPCHK(hipcub::DeviceScan::ExclusiveSum(nullptr, tb, in, out, (int)n));
  return ensure(c, B_CUB_TMP, tb + 256);
}
template <class In, class Out>
static int scan_max(Ctx* c, In in, Out out, uint64_t n) {
  size_t tb = c->bufs[B_CUB_TMP].n;
  HIPCHK(hipcub::DeviceScan::InclusiveScan(P<void>(c, B_CUB_TMP), tb, in, out, hipcub::Max(), (int)n, c->stream));
  LAUNCHED(c->stream, "hipcub");
  return 0;
}
template <class In, class Out>
static int scan_sum(Ctx* c, In in, Out out, uint64_t n, hipStream_t s = nullptr) {
  if (!s) s = c->stream;
  size_t tb = c->bufs[B_CUB_TMP].n;
  HIPCHK(hipcub::DeviceScan::ExclusiveSum(P<void>(c, B_CUB_TMP), tb, in, out, (int)n, s));
  LAUNCHED(s, "hipcub");
  return 0;
}
// ... and its total (the last prefix + the last term, n >= 1) read back with
// one wait, which up to three more reads share
template <class T, class U>
static int scan_sum_total(Ctx* c, T* in, U* out, uint64_t n, hipStream_t s, uint64_t* total, SmallRead r1 = {},
                          SmallRead r2 = {}, SmallRead r3 = {}) {
  if (!s) s = c->stream;
  TRY(scan_sum(c, in, out, n, s));
  U prefix{};
  typename std::remove_const<T>::type term{};
  TRY(read_small(c, s, {rd(out + n - 1, &prefix), rd(in + n - 1, &term), r1, r2, r3}));
  *total = (uint64_t)prefix + term;
  return 0;
}
// pairs sorted by the low 48 bits of their keys
static int sort_pairs48(Ctx* c, const uint64_t* kin, uint64_t* kout, const uint64_t* vin, uint64_t* vout, uint64_t n) {
  size_t tb = 0;
  HIPCHK(hipcub::DeviceRadixSort::SortPairs(nullptr, tb, kin, kout, vin, vout, (int)n, 0, 48, c->stream));
  TRY(ensure(c, B_CUB_TMP, tb + 256));
  tb = c->bufs[B_CUB_TMP].n;
  HIPCHK(hipcub::DeviceRadixSort::SortPairs(P<void>(c, B_CUB_TMP), tb, kin, kout, vin, vout, (int)n, 0, 48, c->stream));
  LAUNCHED(c->stream, "hipcub");
  return 0;
}

}  // namespace

struct srd_ctx : Ctx {};

// read out the oldest n pending scan event pairs (their launches completed
// before the call that made them returned)
static int drain_scan_events(Ctx* c, uint32_t n) {
  for (; n && c->sev_pending; n--) {
    const uint32_t i = (c->sev_next - c->sev_pending) % Ctx::kScanRing;
    float ms = 0;
    HIPCHK(hipEventElapsedTime(&ms, c->sev[2 * i], c->sev[2 * i + 1]));
    c->scan_ms += ms;
    c->scan_launches++;
    if (c->scan_list.size() < (1u << 16)) c->scan_list.push_back(ms);
    c->sev_pending--;
  }
  return 0;
}
// the event pair for the next scan launch (none below SRD_TIMING_SCAN)
static int next_scan_events(Ctx* c, hipEvent_t* e0, hipEvent_t* e1) {
  *e0 = *e1 = nullptr;
  if (c->timing < SRD_TIMING_SCAN) return 0;
  if (c->timing_seq++ % c->timing_every) return 0;  // srd_ctx_set_timing_every: a sampled launch only
  if (c->sev_pending == Ctx::kScanRing) TRY(drain_scan_events(c, 1));
  const uint32_t i = c->sev_next++ % Ctx::kScanRing;
  c->sev_pending++;
  *e0 = c->sev[2 * i];
  *e1 = c->sev[2 * i + 1];
  return 0;
}

// relative weights of a block's 16 wave slots -> their shares of 65536
static void weights_to_shares(const double (&f)[16], uint32_t (&wq)[16]) {
  double sum = 0;
  for (double x : f) sum += x;
  uint32_t used = 0;
  for (int v = 0; v < 15; v++) used += wq[v] = (uint32_t)(65536.0 * f[v] / sum);
  wq[15] = 65536 - used;
}

// ScanPart::wq, the share of each wave slot of a block.  The SIMD's issue
// arbitration favours its older waves (slots 0-3 are the oldest on each
// SIMD, 12-15 the youngest), so an even split ended the slots at 1 : 1.069 :
// 1.125 : 1.179 by age group (tools/wave_stamps.py).  Default: per-slot
// shares from the wave stamps of per-age-group shares (1 : 1/1.069 : 1/1.125
// : 1/1.179), each slot's share scaled by (mean end / its end)^1.5: -1.3 to
// -1.6 % scan against the age-group shares, -0.8 % at power 1, -0.6 % at 2
// (tools/weights_ab.py: every set inside the same contexts).
// SRD_SCAN_WEIGHTS sets relative shares: 4 values (one per age group;
// "1,1,1,1" is the even split) or 16 (one per slot).
static void scan_weights(uint32_t (&wq)[16]) {
  double f[16] = {1.0000, 0.9787, 0.9796, 0.9788, 0.9081, 0.9072, 0.9074, 0.8915,
                  0.8432, 0.8324, 0.8337, 0.8314, 0.7726, 0.7701, 0.7712, 0.7590};
  if (const char* e = getenv("SRD_SCAN_WEIGHTS")) {
    // 4 or 16 finite positive values whose sum is finite; anything else
    // (unparsable, 'inf', 'nan', an overflowing sum) keeps the defaults
    double g[16], gs = 0;
    int n = 0;
    for (const char* q = e; n < 16 && *q;) {
      char* end = nullptr;
      const double x = strtod(q, &end);
      if (end == q || !(x > 0) || !std::isfinite(x)) { n = 0; break; }
      g[n++] = x;
      gs += x;
      q = *end == ',' ? end + 1 : end;
      if (*end && *end != ',') { n = 0; break; }
    }
    if (!std::isfinite(gs)) n = 0;
    if (n == 4)
      for (int v = 0; v < 16; v++) f[v] = g[v / 4];
    else if (n == 16)
      for (int v = 0; v < 16; v++) f[v] = g[v];
  }
  weights_to_shares(f, wq);
}
#ifdef SRD_DEBUG_API  // timing builds: A/B of scan variants inside one context (one workspace)
extern "C" int srd_debug_set_scan_variant(srd_ctx* c, int v) {
  if (!c || !(v == 0 || v == 7 || v == 8 || v == SCAN_LINES)) return SRD_ERR_ARG;
  c->scan_variant = (uint32_t)v;
  return 0;
}
extern "C" int srd_debug_set_scan_bpc(srd_ctx* c, int bpc) {  // scan blocks per CU (1 or 2; one resident at a time)
  if (!c || bpc < 1 || bpc > 2) return SRD_ERR_ARG;
  c->scan_blocks = c->scan_cus * (unsigned)bpc;
  return 0;
}
extern "C" int srd_debug_set_xpart(srd_ctx* c, int on) {  // XCD-aware scan block shares on / off
  if (!c) return SRD_ERR_ARG;
  c->xpart_on = on != 0;
  return 0;
}
extern "C" int srd_debug_set_glue_fused(srd_ctx* c, int fused) {
  if (!c) return SRD_ERR_ARG;
  c->glue_fused = fused != 0;
  return 0;
}
extern "C" int srd_debug_set_scan_weights(srd_ctx* c, const double* w, int n) {
  if (!c || !w || (n != 4 && n != 16)) return SRD_ERR_ARG;
  double f[16], sum = 0;
  for (int v = 0; v < 16; v++) {
    sum += f[v] = n == 4 ? w[v / 4] : w[v];
    if (!(f[v] > 0) || !std::isfinite(f[v])) return SRD_ERR_ARG;
  }
  if (!std::isfinite(sum)) return SRD_ERR_ARG;
  weights_to_shares(f, c->scan_wq);
  return 0;
}
#endif
// srd_ctx_create's work on the new context; on a failure the caller destroys
// it (srd_ctx_destroy frees whatever was made so far)
static int ctx_init(srd_ctx* c, int device) {
  c->device = device;
  c->bufs.resize(B_COUNT_);
  if (hipStreamCreateWithFlags(&c->stream, hipStreamNonBlocking) != hipSuccess) {
    set_err("hipStreamCreate failed");
    return SRD_ERR_HIP;
  }
  TRY(upload_tables());
  // timing events (srd_ctx_timings) with a device-scope release: a default
  // event's system-scope release (an L2 write-back) put ~5 us into the
  // timeline at each record (four per call)
  for (auto& e : c->ev) HIPCHK(hipEventCreateWithFlags(&e, hipEventReleaseToDevice));
  HIPCHK(hipEventCreateWithFlags(&c->ev_ready, hipEventDisableTiming));
  HIPCHK(hipHostMalloc((void**)&c->h_plan, sizeof(Plan), hipHostMallocDefault));
  HIPCHK(hipHostMalloc((void**)&c->h_pub, 64, hipHostMallocCoherent));  // fine-grained: the device's system-scope stores land here
  memset(c->h_pub, 0, 64);
  HIPCHK(hipHostMalloc((void**)&c->h_small, 256, hipHostMallocDefault));
  c->stage_workers = (int)std::max(1u, std::min(8u, std::thread::hardware_concurrency()));
  int ncu = 0;
  if (hipDeviceGetAttribute(&ncu, hipDeviceAttributeMultiprocessorCount, device) == hipSuccess && ncu > 0)
    c->scan_cus = c->scan_blocks = (unsigned)ncu;
  scan_weights(c->scan_wq);
  if (const char* e = getenv("SRD_SLOT_LIMIT_LOG2")) {
    const long v = strtol(e, nullptr, 10);
    if (v >= 10 && v <= 31) c->slot_limit = 1ull << v;
  }
  // the scan's tile loads for every store size: "lines" (line-per-lane) or
  // "coal" (coalesced + transpose); unset = by size (scan_variant_for).  The
  // results are identical either way (tests/test_gpu_parity.py runs both)
  if (const char* e = getenv("SRD_SCAN_LOADS")) {
    if (!strcmp(e, "lines")) c->loads_pin = SCAN_LINES;
    else if (!strcmp(e, "coal")) c->loads_pin = 0;
  }
  if (const char* e = getenv("SRD_GLUE_FUSED")) c->glue_fused = strcmp(e, "0") != 0;
  if (const char* e = getenv("SRD_XPART")) c->xpart_on = strcmp(e, "0") != 0;
  if (const char* e = getenv("SRD_LB_FAIL_BLOCK")) {
    char* end = nullptr;
    const unsigned long v = strtoul(e, &end, 10);
    if (end != e && v < CHAIN_BLOCKS) c->lb_fail = (uint32_t)v;
  }
  return 0;
}

extern "C" int srd_ctx_create(int device, srd_ctx** out) {
  if (!out) { set_err("null out"); return SRD_ERR_ARG; }
  int n = 0;
  HIPCHK(hipGetDeviceCount(&n));
  if (device < 0 || device >= n) { set_err("bad device index"); return SRD_ERR_ARG; }
  HIPCHK(hipSetDevice(device));
  auto* c = new srd_ctx();
  const int r = ctx_init(c, device);
  if (r) {
    srd_ctx_destroy(c);
    return r;
  }
  *out = c;
  return 0;
}

extern "C" void srd_ctx_destroy(srd_ctx* c) {
  if (!c) return;
  delete c->worker;  // idle between calls: joins at once
  hipSetDevice(c->device);
  if (c->ev_ready) hipEventDestroy(c->ev_ready);
  for (auto& b : c->bufs)
    if (b.p) hipFree(b.p);
  if (c->file.p) hipFree(c->file.p);
  for (auto& e : c->ev)
    if (e) hipEventDestroy(e);
  for (auto& e : c->sev)
    if (e) hipEventDestroy(e);
  if (c->h_plan) hipHostFree(c->h_plan);
  if (c->h_pub) hipHostFree(c->h_pub);
  if (c->h_small) hipHostFree(c->h_small);
  if (c->h_out) hipHostFree(c->h_out);
  for (int i = 0; i < 2; i++) {
    if (c->pin_ent[i]) hipHostFree(c->pin_ent[i]);
    if (c->wev_copied[i]) hipEventDestroy(c->wev_copied[i]);
    if (c->wev_done[i]) hipEventDestroy(c->wev_done[i]);
  }
  if (c->cstream) hipStreamDestroy(c->cstream);
  for (auto p : c->stage_pin)
    if (p) hipHostFree(p);
  for (auto e : c->stage_ev)
    if (e) hipEventDestroy(e);
  for (auto st : c->stage_streams)
    if (st) hipStreamDestroy(st);
  if (c->stream) hipStreamDestroy(c->stream);
  delete c;
}

extern "C" void* srd_ctx_stream(srd_ctx* c) { return c ? (void*)c->stream : nullptr; }
extern "C" int srd_ctx_scan_loads(srd_ctx* c) { return c ? c->last_loads : -1; }
extern "C" int srd_ctx_scan_trial(srd_ctx* c, double* ms) {
  if (!c) return -1;
  if (ms)
    for (int k = 0; k < 2; k++) ms[k] = c->tune.n[k] ? (double)c->tune.best[k] * 1e-5 : 0.0;  // 10 ns ticks
  return c->tune.choice;
}
// The block-start table of the optimistic scan, installed and read back
// (diagnostics: tests pin the partition a call runs on instead of taking
// whatever the box's timing history produced).  The copies go through the
// context's stream, behind the previous call's link2 and in front of the next
// call's scan, and are waited for.
extern "C" int srd_ctx_set_scan_blocks(srd_ctx* c, const uint64_t* starts, uint32_t n_blocks, uint64_t n_spans) {
  if (!c || !starts) { set_err("bad argument"); return SRD_ERR_ARG; }
  if (!c->xpart_on) { set_err("XCD-aware block shares are off on this context (SRD_XPART=0)"); return SRD_ERR_ARG; }
  if (!part_table_ok(starts, n_blocks, n_spans)) {
    set_err("bad argument: not a block-start table of n_blocks blocks over n_spans spans (srd_ctx_set_scan_blocks)");
    return SRD_ERR_ARG;
  }
  HIPCHK(hipSetDevice(c->device));
  TRY(ensure_z(c, B_XPART, sizeof(XPart)));
  HIPCHK(hipMemcpyAsync(&P<XPart>(c, B_XPART)->bs[c->xp_par][0], starts, ((size_t)n_blocks + 1) * 8,
                        hipMemcpyHostToDevice, c->stream));
  HIPCHK(hipStreamSynchronize(c->stream));
  c->xp_valid = true;
  c->xp_installed = true;
  c->xp_ns = n_spans;
  c->xp_g = n_blocks;
  return 0;
}
extern "C" int srd_ctx_scan_blocks(srd_ctx* c, int which, uint64_t* starts, uint32_t cap,
                                   srd_scan_blocks_info* info) {
  if (!c || !info || (cap && !starts) || (which != SRD_SCAN_BLOCKS_LAST && which != SRD_SCAN_BLOCKS_NEXT)) {
    set_err("bad argument");
    return SRD_ERR_ARG;
  }
  *info = srd_scan_blocks_info{};
  const Ctx::LastPart& l = c->xp_last;
  uint32_t par = 0;
  if (which == SRD_SCAN_BLOCKS_LAST) {
    if (!l.any) return 0;
    info->n_spans = l.ns;
    info->n_blocks = l.g;
    info->source = l.src;
    info->attempts = l.attempts;
    info->first_source = l.first_src;
    par = l.par;
  } else {
    if (!c->xp_valid) return 0;
    info->n_spans = c->xp_ns;
    info->n_blocks = c->xp_g;
    info->source = c->xp_installed ? SRD_SCAN_BLOCKS_INSTALLED : SRD_SCAN_BLOCKS_MEASURED;
    par = c->xp_par;
  }
  const size_t n = std::min<size_t>(cap, (size_t)info->n_blocks + 1);
  if (!n) return 0;
  if (info->source == SRD_SCAN_BLOCKS_EVEN) {
    for (size_t b = 0; b < n; b++) starts[b] = b * info->n_spans / info->n_blocks;
    return 0;
  }
  HIPCHK(hipSetDevice(c->device));
  HIPCHK(hipMemcpyAsync(starts, &P<XPart>(c, B_XPART)->bs[par][0], n * 8, hipMemcpyDeviceToHost, c->stream));
  HIPCHK(hipStreamSynchronize(c->stream));
  return 0;
}
extern "C" uint64_t srd_ctx_device_bytes(srd_ctx* c) {
  if (!c) return 0;
  uint64_t n = c->file.n;
  for (const Buf& b : c->bufs) n += b.n;
  return n;
}

extern "C" int srd_ctx_set_timing(srd_ctx* c, int level) {
  if (!c || level < SRD_TIMING_NONE || level > SRD_TIMING_CALL) { set_err("bad argument"); return SRD_ERR_ARG; }
  if (level >= SRD_TIMING_SCAN && !c->sev[0]) {
    HIPCHK(hipSetDevice(c->device));
    for (auto& e : c->sev) HIPCHK(hipEventCreateWithFlags(&e, hipEventReleaseToDevice));
  }
  c->timing = level;
  return 0;
}

extern "C" int srd_ctx_set_timing_every(srd_ctx* c, int n) {
  if (!c || n < 1) { set_err("bad argument"); return SRD_ERR_ARG; }
  c->timing_every = (uint32_t)n;
  c->timing_seq = 0;
  return 0;
}

extern "C" int srd_ctx_timings(srd_ctx* c, double* scan_ms, int* scan_launches, double* total_ms) {
  if (!c) { set_err("bad argument"); return SRD_ERR_ARG; }
  HIPCHK(hipSetDevice(c->device));
  TRY(drain_scan_events(c, c->sev_pending));
  if (scan_ms) *scan_ms = c->scan_ms;
  if (scan_launches) *scan_launches = c->scan_launches;
  if (total_ms) *total_ms = c->total_ms;
  c->scan_ms = 0;
  c->scan_launches = 0;
  c->scan_last.swap(c->scan_list);
  c->scan_list.clear();
  return 0;
}

extern "C" int srd_ctx_scan_list(srd_ctx* c, float* out, int cap) {
  if (!c || (cap > 0 && !out)) { set_err("bad argument"); return SRD_ERR_ARG; }
  const int n = (int)std::min<size_t>(c->scan_last.size(), (size_t)std::max(cap, 0));
  for (int i = 0; i < n; i++) out[i] = c->scan_last[i];
  return (int)c->scan_last.size();
}
