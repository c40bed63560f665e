// srd_multi.hip -- DataStore::open on n GPUs in one process, no RCCL
// (SURVEY.md 8(e)); included by srd_api.hip.
//
// srd_validate_index_multi_device: every context holds its entry-range shard
// in its own HBM.  One host thread per context validates its span
// (srd_validate_span_device) and, for the by-owner index, partitions its
// shard-local index by owner; the host composes the shards; each owner then
// pulls its runs from every shard in shard (= file) order over xGMI
// (hipMemcpyPeerAsync; no collective library) and builds its part of the
// latest-wins index.  With SRD_FLAG_MERGE_INDEX ctxs[0] pulls the whole
// shard indexes instead and builds the one merged index.
// srd_validate_index_multi (host input) stages the spans and calls the same
// implementation with the merged index, then copies the result to the host.
//
// Peer access of device dev0 to dev's memory, enabled once per pair and
// process.  Returns false when it cannot be enabled (no xGMI path, or the
// runtime refused): hipMemcpyPeerAsync still works then, staged through host
// memory, and the call counts the pair in srd_multi_summary::peer_errors.
static bool enable_peer(int dev0, int dev) {
  static std::mutex mu;
  static uint8_t state[64][64] = {};  // 0 not tried, 1 enabled, 2 failed
  if (dev0 == dev) return true;
  if (dev0 < 0 || dev < 0 || dev0 >= 64 || dev >= 64) return false;
  std::lock_guard<std::mutex> lk(mu);
  if (!state[dev0][dev]) {
    int can = 0, cur = 0;
    bool ok = hipDeviceCanAccessPeer(&can, dev0, dev) == hipSuccess && can;
    if (ok && hipGetDevice(&cur) == hipSuccess && hipSetDevice(dev0) == hipSuccess) {
      const hipError_t e = hipDeviceEnablePeerAccess(dev, 0);
      ok = e == hipSuccess || e == hipErrorPeerAccessAlreadyEnabled;
      (void)hipSetDevice(cur);
    } else {
      ok = false;
    }
    (void)hipGetLastError();
    state[dev0][dev] = ok ? 1 : 2;
  }
  return state[dev0][dev] == 1;
}

// the same context twice would be driven by two host threads at once (its
// stream, workspace and staging buffers are not shareable)
static int check_ctxs(srd_ctx* const* ctxs, uint32_t nc) {
  if (nc > PART_MAX_WORLD) { set_err("bad argument: at most 64 contexts"); return SRD_ERR_ARG; }
  for (uint32_t i = 0; i < nc; i++) {
    if (!ctxs[i]) { set_err("bad argument: null context"); return SRD_ERR_ARG; }
    for (uint32_t j = 0; j < i; j++)
      if (ctxs[j] == ctxs[i]) { set_err("bad argument: each entry of ctxs must be a distinct context"); return SRD_ERR_ARG; }
  }
  return 0;
}

// Task i of n runs on the persistent worker of context on(i) (task 0 on the
// calling thread); the contexts of one call are distinct (check_ctxs), so no
// worker gets two tasks.  Replaces a std::thread per task per phase.
template <class On, class F>
static void parallel_for(uint32_t n, On&& on, F&& f) {
  for (uint32_t i = 1; i < n; i++) {
    Ctx* c = on(i);
    if (!c->worker) c->worker = new Worker();
    c->worker->post([&f, i] { f(i); });
  }
  if (n) f(0);
  for (uint32_t i = 1; i < n; i++) on(i)->worker->wait();
}

// Record, on the context's stream, that the device data a later cross-
// context copy will read is enqueued (the copy's stream waits on it)
static hipError_t mark_ready(Ctx* c) {
  const hipError_t e = hipEventRecord(c->ev_ready, c->stream);
  c->ready_recorded = e == hipSuccess;
  return e;
}

// device copy into dst's memory on dst's stream (peer copy over xGMI when the
// source lives on another GPU), ordered after the source context's last
// mark_ready by an explicit event wait on dst's stream; *peer_fail counts the
// copies between devices without peer access (staged by the runtime)
static hipError_t copy_to(Ctx* dst, void* d, const Ctx* src, const void* s, uint64_t bytes,
                          std::atomic<uint32_t>* peer_fail) {
  if (!bytes) return hipSuccess;
  if (src != dst && src->ready_recorded) {
    const hipError_t e = hipStreamWaitEvent(dst->stream, src->ev_ready, 0);
    if (e != hipSuccess) return e;
  }
  if (src->device == dst->device) return hipMemcpyAsync(d, s, bytes, hipMemcpyDeviceToDevice, dst->stream);
  if (!enable_peer(dst->device, src->device) && peer_fail) peer_fail->fetch_add(1);
  return hipMemcpyPeerAsync(d, dst->device, s, src->device, bytes, dst->stream);
}

using Clock = std::chrono::steady_clock;
static double ms_since(Clock::time_point t0) {
  return std::chrono::duration<double, std::milli>(Clock::now() - t0).count();
}

struct MultiIn {
  srd_ctx* const* ctxs;
  uint32_t nc;
  const uint8_t* const* span;  // span[i] = file byte soff[i] on ctxs[i]'s device
  const uint64_t* soff;
  const uint64_t* cuts;        // [nc + 1]: shard i holds [soff[i], cuts[i + 1]) when cuts[i] < cuts[i + 1]
  uint64_t flen;
  std::atomic<uint32_t>* peer_fail;  // copies between devices without peer access
};

// file bytes [x, y) assembled in dst's B_GATHER buffer from the shards whose
// resident range covers them (the re-validation of a run of unproven shards
// with its lower neighbour, and the whole-file path)
static int gather_range(Ctx* dst, const MultiIn& in, uint64_t x, uint64_t y, const uint8_t** out) {
  TRY(ensure(dst, B_GATHER, srd_padded_size(y - x)));
  uint8_t* d = P<uint8_t>(dst, B_GATHER);
  for (uint64_t pos = x; pos < y;) {
    int best = -1;
    uint64_t reach = pos;
    for (uint32_t j = 0; j < in.nc; j++)
      if (in.cuts[j] < in.cuts[j + 1] && in.soff[j] <= pos && in.cuts[j + 1] > reach) {
        reach = in.cuts[j + 1];
        best = (int)j;
      }
    if (best < 0) { set_err("internal: no shard holds file byte " + std::to_string(pos)); return SRD_ERR_INTERNAL; }
    const uint64_t e = std::min(y, reach);
    HIPCHK(copy_to(dst, d + (pos - x), in.ctxs[best], in.span[best] + (pos - in.soff[best]), e - pos, in.peer_fail));
    pos = e;
  }
  *out = d;
  return 0;
}

static void release_gather(Ctx* c) {
  Buf& b = c->bufs[B_GATHER];
  if (b.p) {
    (void)hipStreamSynchronize(c->stream);
    (void)hipFree(b.p);
  }
  b.p = nullptr;
  b.n = 0;
}

// The outcome of a task that ran on a context's worker: g_err is per thread,
// so the message travels with the code.
struct TaskErr {
  int rc = 0;
  std::string err;
  void fail(int r, const char* why) { rc = r; err = why; }
  void note(int r) { rc = r; if (r) err = g_err; }  // r from a call on this thread (its message is in g_err)
};
// the first failed task's error, as the calling thread's
static int first_error(const std::vector<TaskErr>& tasks) {
  for (const TaskErr& t : tasks)
    if (t.rc) { set_err(t.err); return t.rc; }
  return 0;
}

struct MShard : TaskErr {
  srd_device_result r{};
  bool proven = false;
  bool parted = false;
  uint64_t cnt[PART_MAX_WORLD] = {};  // owner run lengths of the partitioned shard index (host counts)
  const uint64_t* d_cnt = nullptr;     // or their device address (dev_counts: no host round trip)
};

// the state of one multi-GPU open
struct MultiRun {
  const MultiIn& in;
  bool merged;      // SRD_FLAG_MERGE_INDEX: one index on ctxs[0] instead of one per owner
  uint32_t vflags;  // the shards' validate flags
  // every owner can read every source's HBM (peer access, or one device):
  // the partition counts stay on the devices and the owners' gather reads
  // them (no host round trip per shard); otherwise host counts and copies
  bool dev_counts;
  std::vector<uint64_t> cuts;
  std::vector<MShard> sh;
  std::vector<double> vms;  // per-shard validate time
  uint32_t path = SRD_MULTI_COMPOSED, n_err = 0;
  std::string first_err;
  Ctx* ctx(uint32_t i) const { return in.ctxs[i]; }
};

// the index the exchange leaves: one per owner (ni pairs in each context's
// B_GOKEY / B_GOPACKED) or the merged one
struct MultiIndex {
  std::vector<uint64_t> ni;
  uint64_t merged_n = 0;
  uint64_t *mkey = nullptr, *mpacked = nullptr;
};

// owner partition of shard i's index (by-owner layout, nc > 1)
static int part_shard(MultiRun& m, uint32_t i) {
  MShard& s = m.sh[i];
  const uint32_t nc = m.in.nc;
  if (m.merged || nc == 1 || s.parted) return 0;
  Ctx* c = m.ctx(i);
  const uint64_t n = s.r.n_index;
  TRY(ensure(c, B_XKEY, std::max<uint64_t>(n, 1) * 8));
  TRY(ensure(c, B_XVAL, std::max<uint64_t>(n, 1) * 8));
  if (m.dev_counts)  // (n == 0 too: the owners read its zero counts)
    TRY(partition_impl(c, s.r.index_key_hash, s.r.index_packed, n, nc, P<uint64_t>(c, B_XKEY), P<uint64_t>(c, B_XVAL),
                       nullptr, &s.d_cnt));
  else if (n)
    TRY(partition_impl(c, s.r.index_key_hash, s.r.index_packed, n, nc, P<uint64_t>(c, B_XKEY), P<uint64_t>(c, B_XVAL), s.cnt));
  s.parted = true;
  HIPCHK(mark_ready(c));  // the owners' pulls wait on it
  return 0;
}

// shard i as the span [lo, hi) whose bytes from soff on lie at d on its context
static void validate_shard(MultiRun& m, uint32_t i, const uint8_t* d, uint64_t soff, uint64_t lo, uint64_t hi) {
  const auto t0 = Clock::now();
  MShard& s = m.sh[i];
  s = MShard{};
  if (lo == hi) { s.proven = true; return; }  // an empty shard composes trivially
  srd_ctx* c = m.in.ctxs[i];
  s.rc = srd_validate_span_device(c, d, soff, lo, hi, m.vflags, &s.r);
  if (!s.rc) {
    s.proven = s.r.final_len == hi && s.r.mode != SRD_MODE_SPAN_UNPROVEN;
    if (s.proven) s.rc = part_shard(m, i);
    // the merged gather reads the shard's result arrays from another stream
    if (!s.rc && mark_ready(c) != hipSuccess) { set_err("hipEventRecord"); s.rc = SRD_ERR_HIP; }
  }
  if (s.rc) s.err = g_err;
  m.vms[i] += ms_since(t0);
}

// every shard proven and no error; the failed shards are counted
static bool composes(MultiRun& m) {
  bool ok = true;
  for (auto& x : m.sh) {
    ok = ok && !x.rc && x.proven;
    if (x.rc) {
      m.n_err++;
      if (m.first_err.empty()) m.first_err = x.err;
    }
  }
  return ok;
}

// A cut that is no chain tail (a forged metadata record in a payload) leaves
// the shard above it unproven (no node has prev == the cut).  Each run [a, b]
// of unproven shards is re-validated once together with its lower neighbour,
// as the span [cuts[a], cuts[b+1]) whose ends are tails the neighbours proved
// -- its bytes gathered onto ctxs[a]'s GPU: 2/nc of the store instead of all
// of it.  Still unproven (a torn tail, corruption): the whole-file path decides.
static void repair_neighbours(MultiRun& m) {
  const MultiIn& in = m.in;
  const uint32_t nc = in.nc;
  std::vector<uint64_t>& cuts = m.cuts;
  std::vector<MShard>& sh = m.sh;
  m.path = SRD_MULTI_NEIGHBOUR;
  std::vector<std::pair<uint32_t, uint32_t>> runs;
  uint32_t floor = 0;  // the first shard the next run may take
  for (uint32_t i = 0; i < nc; i++) {
    if (sh[i].proven) continue;
    uint32_t b = i;
    while (b + 1 < nc && !sh[b + 1].proven) b++;
    // the lower neighbour: the first non-empty shard below (an empty shard
    // "proves" nothing; its cut may be the forged one)
    uint32_t a = i ? i - 1 : 0;
    while (a > floor && cuts[a] == cuts[a + 1]) a--;
    if (!runs.empty() && a <= floor && cuts[a] == cuts[a + 1]) {
      // the walk reached the previous run through empty shards only: no
      // shard between proves a tail, so this run joins the previous one
      // (two runs would both start or end at the suspect cut)
      runs.back().second = b;
    } else {
      runs.emplace_back(std::max(a, floor), b);
    }
    floor = b + 1;
    i = b;
  }
  for (auto [a, b] : runs)
    for (uint32_t i = a + 1; i <= b; i++) {
      cuts[i] = cuts[b + 1];  // shards a+1..b become empty; shard a spans the run
      sh[i] = MShard{};
      sh[i].proven = true;
    }
  parallel_for((uint32_t)runs.size(), [&](uint32_t k) { return m.ctx(runs[k].first); }, [&](uint32_t k) {
    const uint32_t a = runs[k].first;
    const uint64_t lo = cuts[a], hi = cuts[a + 1], x = lo - lo % SPAN_BYTES;
    const uint8_t* d = nullptr;
    Ctx* c = m.ctx(a);
    int r = hipSetDevice(c->device) == hipSuccess ? 0 : SRD_ERR_HIP;
    if (!r && lo < hi) r = gather_range(c, in, x, hi, &d);
    if (r) {
      sh[a] = MShard{};
      sh[a].note(r);
      return;
    }
    validate_shard(m, a, d, x, lo, hi);
  });
}

// A torn tail, corruption, or a shard that failed (capacity, allocation):
// recover_valid_chain's byte-wise search is global, so the whole-file path
// decides, on ctxs[0] with the store gathered there.
static int repair_whole_file(MultiRun& m) {
  const MultiIn& in = m.in;
  m.path = SRD_MULTI_WHOLE_FILE;
  for (uint32_t i = 1; i < in.nc; i++) {
    m.sh[i] = MShard{};
    m.cuts[i] = in.flen;
  }
  srd_ctx* c0 = in.ctxs[0];
  const auto t0 = Clock::now();
  m.sh[0] = MShard{};
  const uint8_t* d = nullptr;
  int r = hipSetDevice(c0->device) == hipSuccess ? 0 : SRD_ERR_HIP;
  if (!r) r = gather_range(c0, in, 0, in.flen, &d);
  if (!r) r = srd_validate_index_device(c0, d, in.flen, m.vflags, &m.sh[0].r);
  if (!r) r = part_shard(m, 0);
  m.vms[0] += ms_since(t0);
  if (r) {
    if (!m.first_err.empty()) set_err(g_err + " (after a shard error: " + m.first_err + ")");
    release_gather(c0);
  }
  return r;
}

// the gather and build buffers of an index of n pairs on context c
static int ensure_gather(Ctx* c, uint64_t n) {
  const uint64_t bytes = std::max<uint64_t>(n, 1) * 8;
  TRY(ensure(c, B_GKEY, bytes));
  TRY(ensure(c, B_GVAL, bytes));
  TRY(ensure(c, B_GOKEY, bytes));
  TRY(ensure(c, B_GOPACKED, bytes));
  return 0;
}

// c's stream waits for what every other context marked ready (mark_ready)
static int wait_sources(const MultiIn& in, Ctx* c) {
  for (uint32_t s = 0; s < in.nc; s++) {
    Ctx* cs = in.ctxs[s];
    if (cs != c && cs->ready_recorded && hipStreamWaitEvent(c->stream, cs->ev_ready, 0) != hipSuccess) {
      set_err("index exchange: event wait failed");
      return SRD_ERR_HIP;
    }
  }
  return 0;
}

// one block column per source, sized for runs of about run_pairs pairs
static int launch_gather_runs(Ctx* c, const GatherArgs& ga, uint32_t nsrc, uint64_t run_pairs) {
  const dim3 grid((unsigned)std::min<uint64_t>(std::max<uint64_t>((run_pairs + 255) / 256, 1), 128), nsrc);
  gather_runs_kernel<<<grid, 256, 0, c->stream>>>(ga);
  if (hipGetLastError() != hipSuccess) { set_err("index exchange: gather launch failed"); return SRD_ERR_HIP; }
  return 0;
}

// Merged layout: ctxs[0] pulls the whole shard indexes in shard (= file)
// order and builds the one latest-wins index.
static int exchange_merged(MultiRun& m, MultiIndex* x) {
  const MultiIn& in = m.in;
  Ctx* c0 = m.ctx(0);
  if (hipSetDevice(c0->device) != hipSuccess) return SRD_ERR_HIP;
  uint64_t NI = 0;
  for (auto& s : m.sh) NI += s.r.n_index;
  TRY(ensure_gather(c0, NI));
  uint64_t acc = 0;
  for (uint32_t s = 0; s < in.nc; s++) {
    const uint64_t n = m.sh[s].r.n_index;
    if (copy_to(c0, P<uint64_t>(c0, B_GKEY) + acc, in.ctxs[s], m.sh[s].r.index_key_hash, n * 8, in.peer_fail) != hipSuccess ||
        copy_to(c0, P<uint64_t>(c0, B_GVAL) + acc, in.ctxs[s], m.sh[s].r.index_packed, n * 8, in.peer_fail) != hipSuccess) {
      set_err("index gather: peer copy failed");
      return SRD_ERR_HIP;
    }
    acc += n;
  }
  x->mkey = P<uint64_t>(c0, B_GOKEY);
  x->mpacked = P<uint64_t>(c0, B_GOPACKED);
  return index_build_sep(c0, P<uint64_t>(c0, B_GKEY), P<uint64_t>(c0, B_GVAL), NI, x->mkey, x->mpacked, &x->merged_n);
}

// By owner, device counts: owner p's runs, their lengths and offsets from the
// sources' partition counts in their HBM (gather_runs_kernel), the build's n
// on the device; sized by the bound ni_all (the pairs of every shard),
// buckets for ni_all / nc pairs (owner = the key hash's top bits: an even
// split).  ni_max: the largest shard's pairs.
static int owner_build_dev(MultiRun& m, uint32_t p, uint64_t ni_all, uint64_t ni_max, uint64_t* n_index) {
  const MultiIn& in = m.in;
  const uint32_t nc = in.nc;
  Ctx* c = m.ctx(p);
  TRY(ensure_gather(c, ni_all));
  TRY(ensure(c, B_XTOT, 64));
  GatherArgs ga{};
  for (uint32_t s = 0; s < nc; s++) {
    ga.src_k[s] = P<uint64_t>(m.ctx(s), B_XKEY);
    ga.src_v[s] = P<uint64_t>(m.ctx(s), B_XVAL);
    ga.src_cnt[s] = m.sh[s].d_cnt;
  }
  ga.dst_k = P<uint64_t>(c, B_GKEY);
  ga.dst_v = P<uint64_t>(c, B_GVAL);
  ga.d_total = P<uint64_t>(c, B_XTOT);
  ga.owner = p;
  ga.nsrc = nc;
  TRY(wait_sources(in, c));
  TRY(launch_gather_runs(c, ga, nc, 2 * (ni_max / nc + 1)));  // ~ twice a source's run for one owner
  return index_build_sep(c, ga.dst_k, ga.dst_v, ni_all, P<uint64_t>(c, B_GOKEY), P<uint64_t>(c, B_GOPACKED), n_index,
                         ga.d_total, ni_all / nc + 1);
}

// By owner, host counts: owner p pulls its run of every source in shard
// order -- one gather launch reading the peers' HBM when every source GPU is
// peer-accessible, else one copy per run -- and builds its index.
static int owner_build_host(MultiRun& m, uint32_t p, uint64_t* n_index) {
  const MultiIn& in = m.in;
  const uint32_t nc = in.nc;
  Ctx* c = m.ctx(p);
  uint64_t NI = 0;
  for (auto& x : m.sh) NI += x.cnt[p];
  TRY(ensure_gather(c, NI));
  GatherArgs ga{};
  bool direct = true;
  uint64_t acc = 0, nmax = 0;
  for (uint32_t s = 0; s < nc; s++) {
    uint64_t off = 0;
    for (uint32_t q = 0; q < p; q++) off += m.sh[s].cnt[q];
    Ctx* cs = m.ctx(s);
    ga.src_k[s] = P<uint64_t>(cs, B_XKEY) + off;
    ga.src_v[s] = P<uint64_t>(cs, B_XVAL) + off;
    ga.dst_off[s] = acc;
    acc += m.sh[s].cnt[p];
    nmax = std::max<uint64_t>(nmax, m.sh[s].cnt[p]);
    if (cs->device != c->device && !enable_peer(c->device, cs->device)) direct = false;
  }
  ga.dst_off[nc] = acc;
  ga.dst_k = P<uint64_t>(c, B_GKEY);
  ga.dst_v = P<uint64_t>(c, B_GVAL);
  if (direct && nmax) {
    TRY(wait_sources(in, c));
    TRY(launch_gather_runs(c, ga, nc, nmax));
  } else {
    for (uint32_t s = 0; s < nc; s++) {
      const uint64_t n = m.sh[s].cnt[p];
      if (copy_to(c, ga.dst_k + ga.dst_off[s], m.ctx(s), ga.src_k[s], n * 8, in.peer_fail) != hipSuccess ||
          copy_to(c, ga.dst_v + ga.dst_off[s], m.ctx(s), ga.src_v[s], n * 8, in.peer_fail) != hipSuccess) {
        set_err("index exchange: peer copy failed");
        return SRD_ERR_HIP;
      }
    }
  }
  return index_build_sep(c, ga.dst_k, ga.dst_v, NI, P<uint64_t>(c, B_GOKEY), P<uint64_t>(c, B_GOPACKED), n_index);
}

// By-owner layouts: the shards re-validated by a repair partition now; then
// every owner gathers its runs and builds its part of the latest-wins index.
static int exchange_by_owner(MultiRun& m, MultiIndex* x) {
  const uint32_t nc = m.in.nc;
  const auto on = [&](uint32_t i) { return m.ctx(i); };
  std::vector<TaskErr> te(nc);
  parallel_for(nc, on, [&](uint32_t i) {
    if (hipSetDevice(m.ctx(i)->device) != hipSuccess) { te[i].fail(SRD_ERR_HIP, "hipSetDevice"); return; }
    te[i].note(part_shard(m, i));
  });
  TRY(first_error(te));
  uint64_t ni_all = 0, ni_max = 0;
  for (auto& s : m.sh) {
    ni_all += s.r.n_index;
    ni_max = std::max<uint64_t>(ni_max, s.r.n_index);
  }
  parallel_for(nc, on, [&](uint32_t p) {
    if (hipSetDevice(m.ctx(p)->device) != hipSuccess) { te[p].fail(SRD_ERR_HIP, "hipSetDevice"); return; }
    te[p].note(m.dev_counts ? owner_build_dev(m, p, ni_all, ni_max, &x->ni[p]) : owner_build_host(m, p, &x->ni[p]));
  });
  return first_error(te);
}

static srd_multi_summary summarise(const MultiRun& m, const MultiIndex& x, srd_device_result* shards) {
  const uint32_t nc = m.in.nc;
  const bool one_index = m.merged || nc == 1;
  srd_multi_summary S{};
  S.file_len = m.in.flen;
  S.final_len = m.path == SRD_MULTI_WHOLE_FILE ? m.sh[0].r.final_len : m.in.flen;
  S.mode = SRD_MODE_OPTIMISTIC;
  for (uint32_t i = 0; i < nc; i++) {
    srd_device_result o = m.sh[i].r;
    if (m.cuts[i] == m.cuts[i + 1] && m.path != SRD_MULTI_WHOLE_FILE) memset(&o, 0, sizeof o);
    if (m.path == SRD_MULTI_WHOLE_FILE && i) memset(&o, 0, sizeof o);
    S.n_chain += o.n_chain;
    S.n_crc_bad += o.n_crc_bad;
    S.n_candidates += o.n_candidates;
    if ((o.n_chain || i == 0) && o.mode != SRD_MODE_OPTIMISTIC) S.mode = SRD_MODE_FULL;
    if (one_index) {
      if (nc > 1) {
        o.n_index = 0;
        o.index_key_hash = o.index_packed = nullptr;
      }
    } else {
      o.n_index = x.ni[i];
      o.index_key_hash = P<uint64_t>(m.ctx(i), B_GOKEY);
      o.index_packed = P<uint64_t>(m.ctx(i), B_GOPACKED);
      S.n_index += x.ni[i];
    }
    shards[i] = o;
  }
  if (one_index) {
    S.n_index = x.merged_n;
    S.index_key_hash = x.mkey;
    S.index_packed = x.mpacked;
  }
  S.path = m.path;
  S.n_shards = nc;
  S.merged = one_index ? 1u : 0u;
  S.shard_errors = m.n_err;
  S.peer_errors = m.in.peer_fail ? m.in.peer_fail->load() : 0u;
  for (double v : m.vms) S.validate_ms = std::max(S.validate_ms, v);
  return S;
}

// validate every shard -> repair what does not compose -> exchange the index -> summarise
static int multi_device_impl(const MultiIn& in, uint32_t flags, srd_device_result* shards, srd_multi_summary* sum) {
  const auto t_call = Clock::now();
  const uint32_t nc = in.nc;
  const bool merged = flags & SRD_FLAG_MERGE_INDEX;
  MultiRun m{in, merged, flags & ~(kStageFlags | SRD_FLAG_MERGE_INDEX), !merged && nc > 1};
  m.cuts.assign(in.cuts, in.cuts + nc + 1);
  m.sh.resize(nc);
  m.vms.assign(nc, 0.0);
  for (uint32_t p = 0; p < nc && m.dev_counts; p++)
    for (uint32_t q = 0; q < nc && m.dev_counts; q++)
      if (m.ctx(p)->device != m.ctx(q)->device && !enable_peer(m.ctx(p)->device, m.ctx(q)->device))
        m.dev_counts = false;

  parallel_for(nc, [&](uint32_t i) { return m.ctx(i); }, [&](uint32_t i) {
    if (hipSetDevice(m.ctx(i)->device) != hipSuccess) { m.sh[i] = MShard{}; m.sh[i].fail(SRD_ERR_HIP, "hipSetDevice"); return; }
    validate_shard(m, i, in.span[i], in.soff[i], m.cuts[i], m.cuts[i + 1]);
  });
  bool composed = composes(m);
  // shard 0 over the whole store IS the whole-file path (lo = 0)
  const bool whole_already = m.cuts[1] == in.flen;
  if (!composed && !m.n_err && !whole_already) {
    repair_neighbours(m);
    composed = composes(m);
  }
  if (!composed && !whole_already) {
    TRY(repair_whole_file(m));
  } else if (!composed) {
    m.path = SRD_MULTI_WHOLE_FILE;  // shard 0 was the whole store: its answer is final
    if (m.sh[0].rc) {
      set_err(m.sh[0].err);
      return m.sh[0].rc;
    }
  }
  for (uint32_t i = 0; i < nc; i++) release_gather(m.ctx(i));

  const auto t_ex = Clock::now();
  MultiIndex x;
  x.ni.assign(nc, 0);
  if (nc == 1) {
    x.ni[0] = x.merged_n = m.sh[0].r.n_index;
    x.mkey = m.sh[0].r.index_key_hash;
    x.mpacked = m.sh[0].r.index_packed;
  } else if (merged) {
    TRY(exchange_merged(m, &x));
  } else {
    TRY(exchange_by_owner(m, &x));
  }
  const double ex_ms = ms_since(t_ex);

  srd_multi_summary S = summarise(m, x, shards);
  S.exchange_ms = ex_ms;
  S.total_ms = ms_since(t_call);
  if (sum) *sum = S;
  in.ctxs[0]->last_multi = S;
  in.ctxs[0]->last_shard_ms = m.vms;
  return 0;
}

extern "C" int srd_validate_index_multi_device(srd_ctx* const* ctxs, uint32_t nc, const uint8_t* const* d_spans,
                                               const uint64_t* span_offs, const uint64_t* cuts, uint32_t flags,
                                               srd_device_result* shards, srd_multi_summary* summary) {
  if (!ctxs || !nc || !d_spans || !span_offs || !cuts || !shards) { set_err("bad argument"); return SRD_ERR_ARG; }
  TRY(check_ctxs(ctxs, nc));
  const uint64_t flen = cuts[nc];
  if (cuts[0] != 0 || flen > kMaxFile) { set_err("bad argument: cuts[0] must be 0 and file_len <= 2^48"); return SRD_ERR_ARG; }
  for (uint32_t i = 0; i < nc; i++) {
    if (cuts[i] > cuts[i + 1]) { set_err("bad argument: cuts must be non-decreasing"); return SRD_ERR_ARG; }
    if (cuts[i] == cuts[i + 1]) continue;
    if (!d_spans[i] || span_offs[i] % SPAN_BYTES || span_offs[i] > cuts[i] || (cuts[i] == 0 && span_offs[i])) {
      set_err("bad argument: shard " + std::to_string(i) +
              " needs a span starting at a multiple of 16 KiB at or below its lower tail");
      return SRD_ERR_ARG;
    }
  }
  std::atomic<uint32_t> peer_fail{0};
  MultiIn in{ctxs, nc, d_spans, span_offs, cuts, flen, &peer_fail};
  return multi_device_impl(in, flags, shards, summary);
}

extern "C" int srd_ctx_multi_shard_ms(srd_ctx* c, double* out, int cap) {
  if (!c || cap < 0 || (cap && !out)) { set_err("bad argument"); return SRD_ERR_ARG; }
  const int n = (int)c->last_shard_ms.size();
  for (int i = 0; i < std::min(n, cap); i++) out[i] = c->last_shard_ms[i];
  return n;
}

extern "C" int srd_ctx_multi_summary(srd_ctx* c, srd_multi_summary* out) {
  if (!c || !out) { set_err("bad argument"); return SRD_ERR_ARG; }
  *out = c->last_multi;
  return 0;
}

extern "C" int srd_validate_index_multi(srd_ctx* const* ctxs, uint32_t nc, const uint8_t* file, uint64_t flen,
                                        uint32_t flags, srd_result* out) {
  if (!ctxs || !nc || !out || (!file && flen)) { set_err("bad argument"); return SRD_ERR_ARG; }
  TRY(check_ctxs(ctxs, nc));
  if (nc == 1) return srd_validate_index(ctxs[0], file, flen, flags, out);
  std::vector<uint64_t> cuts(nc + 1), soff(nc, 0);
  {
    const char* why = "";
    const int r = srd_host::shard_cuts(file, flen, nc, cuts.data(), &why);
    if (r) { set_err(why); return r; }
  }
  // pinned input: each shard copies its span directly.  SRD_FLAG_STAGE_REGISTER:
  // the mapping is registered once for all shards (their spans overlap by
  // up to 16 KiB).  Otherwise each shard's bounce workers (the host threads
  // split over the shards) stage its span.
  uintptr_t reg_a = 0, reg_e = 0;
  bool pinned = false;
  if (flen && !(flags & SRD_FLAG_STAGE_PAGEABLE)) {
    if (host_is_pinned(file)) {
      pinned = true;
    } else if (flags & SRD_FLAG_STAGE_REGISTER) {
      HIPCHK(hipSetDevice(ctxs[0]->device));
      reg_a = (uintptr_t)file & ~(uintptr_t)4095;
      reg_e = ((uintptr_t)file + flen + 4095) & ~(uintptr_t)4095;
      pinned = hipHostRegister((void*)reg_a, reg_e - reg_a, hipHostRegisterReadOnly | hipHostRegisterPortable) ==
               hipSuccess;
      (void)hipGetLastError();
      if (!pinned) reg_a = reg_e = 0;
    }
  }
  std::vector<const uint8_t*> span(nc, nullptr);
  std::vector<TaskErr> te(nc);
  const auto on = [&](uint32_t i) -> Ctx* { return ctxs[i]; };
  parallel_for(nc, on, [&](uint32_t i) {
    srd_ctx* c = ctxs[i];
    const uint64_t lo = cuts[i], hi = cuts[i + 1];
    if (lo == hi) return;
    soff[i] = lo - lo % SPAN_BYTES;
    if (hipSetDevice(c->device) != hipSuccess) { te[i].fail(SRD_ERR_HIP, "hipSetDevice"); return; }
    te[i].note(stage_host(c, file + soff[i], hi - soff[i], flags, &span[i], pinned,
                          std::max(1, ctxs[0]->stage_workers / (int)nc)));
  });
  if (reg_a) {
    (void)hipSetDevice(ctxs[0]->device);
    (void)hipHostUnregister((void*)reg_a);
  }
  TRY(first_error(te));
  std::vector<srd_device_result> sr(nc);
  srd_multi_summary sum{};
  std::atomic<uint32_t> peer_fail{0};
  MultiIn in{ctxs, nc, span.data(), soff.data(), cuts.data(), flen, &peer_fail};
  TRY(multi_device_impl(in, (flags & ~kStageFlags) | SRD_FLAG_MERGE_INDEX, sr.data(), &sum));

  memset(out, 0, sizeof *out);
  const uint64_t N = sum.n_chain;
  TRY(host_result_arrays(ctxs[0], N, sum.n_index, out));
  // chain segments D2H on each shard's stream (file order); the merged
  // index from ctxs[0]
  std::vector<uint64_t> cb(nc, 0);
  for (uint32_t i = 1; i < nc; i++) cb[i] = cb[i - 1] + sr[i - 1].n_chain;
  parallel_for(nc, on, [&](uint32_t i) {
    srd_ctx* c = ctxs[i];
    const uint64_t nk = i == 0 ? sum.n_index : 0;
    if (!sr[i].n_chain && !nk) return;
    if (hipSetDevice(c->device) != hipSuccess) { te[i].fail(SRD_ERR_HIP, "result copy failed"); return; }
    hipError_t e = copy_chain_d2h(c->stream, sr[i], sr[i].n_chain, out, cb[i]);
    if (e == hipSuccess && nk)
      e = hipMemcpyAsync(out->index_key_hash, sum.index_key_hash, nk * 8, hipMemcpyDeviceToHost, c->stream);
    if (e == hipSuccess && nk)
      e = hipMemcpyAsync(out->index_packed, sum.index_packed, nk * 8, hipMemcpyDeviceToHost, c->stream);
    if (e == hipSuccess) e = hipStreamSynchronize(c->stream);
    if (e != hipSuccess) te[i].fail(SRD_ERR_HIP, "result copy failed");
  });
  if (const int r = first_error(te)) {
    srd_result_free(out);
    return r;
  }
  out->file_len = flen;
  out->final_len = sum.final_len;
  out->n_chain = N;
  out->n_index = sum.n_index;
  out->n_crc_bad = sum.n_crc_bad;
  out->n_candidates = sum.n_candidates;
  out->mode = sum.mode;
  return 0;
}
