// srd_host_input.hip -- host input and host results (included by srd_api.hip):
// staging of a store in host memory, the pinned result arrays, and the C
// entries that take host pointers.
extern "C" uint64_t srd_padded_size(uint64_t flen) { return ((flen + TILE - 1) / TILE) * TILE + 2 * TILE; }

// ---------------------------------------------------------- shard boundaries
// Host pre-pass for the entry-range shards of an arbitrary store (SURVEY.md
// 8(e)); the parser lives in srd_host.cpp (no HIP, sanitizer-tested).
extern "C" int srd_shard_cuts(const uint8_t* file, uint64_t flen, uint32_t world, uint64_t* cuts) {
  const char* why = "";
  const int r = srd_host::shard_cuts(file, flen, world, cuts, &why);
  if (r) set_err(why);
  return r;
}

// ---------------------------------------------------------------- host input
// The path starts in host memory: the mmap'd single-file store
// (data_store.rs:172-174 init_mmap, called from open :84-117).  Staging modes:
//  - already pinned host memory: one DMA copy;
//  - default: host threads copy 16 MiB chunks into double-buffered pinned
//    bounce buffers, each worker DMA-ing its previous chunk on its own stream
//    meanwhile (the memcpy also takes the mapping's page faults on several
//    cores): the pinned-buffer rate from a page-cache-warm mmap (C2: 87 ms,
//    vs 114 ms registered and 133 ms pageable);
//  - SRD_FLAG_STAGE_REGISTER: hipHostRegister (read-only) of the mapped
//    range, one DMA copy, unregister (bounce buffers if refused);
//  - SRD_FLAG_STAGE_PAGEABLE: one pageable hipMemcpy (the runtime's own
//    staging; measurement baseline).
constexpr uint32_t kStageFlags = SRD_FLAG_STAGE_PAGEABLE | SRD_FLAG_STAGE_REGISTER;
constexpr uint64_t kBounceBytes = 16ull << 20;

static int ensure_file_buf(Ctx* c, uint64_t flen, uint8_t** d) {
  const uint64_t need = srd_padded_size(flen);
  if (c->file.n < need) {
    if (c->file.p) HIPCHK(hipFree(c->file.p));
    c->file.p = nullptr;
    c->file.n = 0;
    if (hipMalloc(&c->file.p, need) != hipSuccess) { set_err("hipMalloc(file)"); return SRD_ERR_ALLOC; }
    c->file.n = need;
  }
  *d = (uint8_t*)c->file.p;
  return 0;
}

static int stage_bounce(Ctx* c, const uint8_t* src, uint64_t len, uint8_t* dst, int workers) {
  const uint64_t nch = (len + kBounceBytes - 1) / kBounceBytes;
  // T workers, each with two pinned bounce buffers and a stream: allocated
  // when a call first needs them (the multi-GPU open gives each shard fewer)
  const int T = (int)std::min<uint64_t>((uint64_t)std::max(1, std::min(workers, c->stage_workers)), nch);
  for (int w = (int)c->stage_streams.size(); w < T; w++) {
    void* pin[2] = {nullptr, nullptr};
    hipEvent_t ev[2] = {nullptr, nullptr};
    hipStream_t st = nullptr;
    for (int k = 0; k < 2; k++) {
      HIPCHK(hipHostMalloc(&pin[k], kBounceBytes, hipHostMallocDefault));
      HIPCHK(hipEventCreateWithFlags(&ev[k], hipEventDisableTiming));
    }
    HIPCHK(hipStreamCreateWithFlags(&st, hipStreamNonBlocking));
    c->stage_pin.insert(c->stage_pin.end(), pin, pin + 2);
    c->stage_ev.insert(c->stage_ev.end(), ev, ev + 2);
    c->stage_streams.push_back(st);
  }
  std::vector<int> rc(T, 0);
  auto work = [&](int w) {
    if (hipSetDevice(c->device) != hipSuccess) { rc[w] = SRD_ERR_HIP; return; }
    uint64_t j = 0;
    for (uint64_t ch = w; ch < nch; ch += T, j++) {
      const int b = 2 * w + (int)(j & 1);
      if (j >= 2 && hipEventSynchronize(c->stage_ev[b]) != hipSuccess) { rc[w] = SRD_ERR_HIP; return; }
      const uint64_t off = ch * kBounceBytes, n = std::min(kBounceBytes, len - off);
      memcpy(c->stage_pin[b], src + off, n);
      if (hipMemcpyAsync(dst + off, c->stage_pin[b], n, hipMemcpyHostToDevice, c->stage_streams[w]) != hipSuccess ||
          hipEventRecord(c->stage_ev[b], c->stage_streams[w]) != hipSuccess) {
        rc[w] = SRD_ERR_HIP;
        return;
      }
    }
    if (hipStreamSynchronize(c->stage_streams[w]) != hipSuccess) rc[w] = SRD_ERR_HIP;
  };
  std::vector<std::thread> th;
  for (int w = 1; w < T; w++) th.emplace_back(work, w);
  if (T) work(0);
  for (auto& t : th) t.join();
  for (int w = 0; w < T; w++)
    if (rc[w]) { set_err("bounce-buffer staging failed"); return rc[w]; }
  c->stage_mode = 2;
  return 0;
}

// pinned or registered host memory? (a pointer the runtime does not know is
// not an error here)
static bool host_is_pinned(const void* p) {
  hipPointerAttribute_t at{};
  const bool r = hipPointerGetAttributes(&at, p) == hipSuccess && at.type == hipMemoryTypeHost;
  (void)hipGetLastError();
  return r;
}

// one DMA copy of a range the runtime can read directly (or stages itself)
static int stage_copy(Ctx* c, uint8_t* d, const uint8_t* src, uint64_t len, int mode) {
  HIPCHK(hipMemcpyAsync(d, src, len, hipMemcpyHostToDevice, c->stream));
  HIPCHK(hipStreamSynchronize(c->stream));
  c->stage_mode = mode;
  return 0;
}
static int stage_host_impl(Ctx* c, const uint8_t* src, uint64_t len, uint32_t flags, const uint8_t** d_out,
                           bool pinned, int workers) {
  uint8_t* d = nullptr;
  TRY(ensure_file_buf(c, len, &d));
  *d_out = d;
  if (!len) return 0;
  if (pinned) return stage_copy(c, d, src, len, 1);
  if (flags & SRD_FLAG_STAGE_PAGEABLE) return stage_copy(c, d, src, len, 3);
  if (host_is_pinned(src)) return stage_copy(c, d, src, len, 0);  // already pinned
  if (flags & SRD_FLAG_STAGE_REGISTER) {
    const uintptr_t a = (uintptr_t)src & ~(uintptr_t)4095, e = ((uintptr_t)src + len + 4095) & ~(uintptr_t)4095;
    if (hipHostRegister((void*)a, e - a, hipHostRegisterReadOnly) == hipSuccess) {
      const int r = stage_copy(c, d, src, len, 1);
      hipHostUnregister((void*)a);
      return r;
    }
    (void)hipGetLastError();
  }
  return stage_bounce(c, src, len, d, workers);
}
// stage host bytes [src, src + len) into the context's device file buffer;
// pinned = the caller knows the range is pinned / registered; workers:
// bounce-buffer threads (the multi-GPU open splits them over its shards)
static int stage_host(Ctx* c, const uint8_t* src, uint64_t len, uint32_t flags, const uint8_t** d_out,
                      bool pinned = false, int workers = 1 << 20) {
  const auto t0 = std::chrono::steady_clock::now();
  const int r = stage_host_impl(c, src, len, flags, d_out, pinned, workers);
  c->stage_ms = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
  return r;
}

// Host results live in one pinned buffer the context owns (valid until the
// next host-input call on it): the device arrays are DMA'd straight into it
// -- no malloc'd pageable destinations (the runtime's own staging and their
// first-touch page faults cost ~10 ms of a C2 open) -- and srd_result_free
// only clears the struct (SRD_RESULT_CTX_OWNED in `reserved`).
constexpr uint32_t SRD_RESULT_CTX_OWNED = 1u;
static int host_result_arrays(Ctx* c, uint64_t n, uint64_t ni, srd_result* out) {
  const uint64_t n1 = std::max<uint64_t>(n, 1), k1 = std::max<uint64_t>(ni, 1);
  const uint64_t need = n1 * (5 * 8 + 2 * 4 + 1) + k1 * 16 + 64;
  if (c->h_out_n < need) {
    if (c->h_out) HIPCHK(hipHostFree(c->h_out));
    c->h_out = nullptr;
    c->h_out_n = 0;
    if (hipHostMalloc(&c->h_out, need, hipHostMallocDefault) != hipSuccess) {
      set_err("hipHostMalloc(results) failed");
      return SRD_ERR_ALLOC;
    }
    c->h_out_n = need;
  }
  uint8_t* b = (uint8_t*)c->h_out;
  auto take = [&](uint64_t bytes) { uint8_t* p = b; b += (bytes + 7) & ~7ull; return p; };
  out->meta_off = (uint64_t*)take(n1 * 8);
  out->key_hash = (uint64_t*)take(n1 * 8);
  out->prev_offset = (uint64_t*)take(n1 * 8);
  out->payload_start = (uint64_t*)take(n1 * 8);
  out->payload_len = (uint64_t*)take(n1 * 8);
  out->index_key_hash = (uint64_t*)take(k1 * 8);
  out->index_packed = (uint64_t*)take(k1 * 8);
  out->crc_stored = (uint32_t*)take(n1 * 4);
  out->crc_computed = (uint32_t*)take(n1 * 4);
  out->crc_ok = (uint8_t*)take(n1);
  out->reserved = SRD_RESULT_CTX_OWNED;
  return 0;
}

// chain entries [0, n) of a device result into host result entries [b, b + n)
static hipError_t copy_chain_d2h(hipStream_t st, const srd_device_result& r, uint64_t n, srd_result* out,
                                 uint64_t b) {
  hipError_t e = hipSuccess;
  auto cp = [&](void* dst, const void* src, uint64_t bytes) {
    if (e == hipSuccess && bytes) e = hipMemcpyAsync(dst, src, bytes, hipMemcpyDeviceToHost, st);
  };
  cp(out->meta_off + b, r.meta_off, n * 8);
  cp(out->key_hash + b, r.key_hash, n * 8);
  cp(out->prev_offset + b, r.prev_offset, n * 8);
  cp(out->payload_start + b, r.payload_start, n * 8);
  cp(out->payload_len + b, r.payload_len, n * 8);
  cp(out->crc_stored + b, r.crc_stored, n * 4);
  cp(out->crc_computed + b, r.crc_computed, n * 4);
  cp(out->crc_ok + b, r.crc_ok, n);
  return e;
}

extern "C" int srd_validate_index(srd_ctx* c, const uint8_t* file, uint64_t flen, uint32_t flags, srd_result* out) {
  if (!c || !out || (!file && flen)) { set_err("bad argument"); return SRD_ERR_ARG; }
  HIPCHK(hipSetDevice(c->device));
  const uint8_t* d = nullptr;
  TRY(stage_host(c, file, flen, flags, &d));
  srd_device_result r;
  TRY(srd_validate_index_device(c, d, flen, flags & ~kStageFlags, &r));
  *out = r;
  TRY(host_result_arrays(c, r.n_chain, r.n_index, out));
  HIPCHK(copy_chain_d2h(c->stream, r, r.n_chain, out, 0));
  if (r.n_index) {
    HIPCHK(hipMemcpyAsync(out->index_key_hash, r.index_key_hash, r.n_index * 8, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(hipMemcpyAsync(out->index_packed, r.index_packed, r.n_index * 8, hipMemcpyDeviceToHost, c->stream));
  }
  HIPCHK(spin_sync(c->stream));
  return 0;
}

extern "C" void srd_result_free(srd_result* r) {
  if (!r) return;
  if (!(r->reserved & SRD_RESULT_CTX_OWNED)) {
    free(r->meta_off); free(r->key_hash); free(r->prev_offset); free(r->payload_start); free(r->payload_len);
    free(r->crc_stored); free(r->crc_computed); free(r->crc_ok); free(r->index_key_hash); free(r->index_packed);
  }
  memset(r, 0, sizeof *r);
}

extern "C" int srd_ctx_stage_info(srd_ctx* c, int* mode, double* stage_ms) {
  if (!c) { set_err("bad argument"); return SRD_ERR_ARG; }
  if (mode) *mode = c->stage_mode;
  if (stage_ms) *stage_ms = c->stage_ms;
  return 0;
}

extern "C" int srd_recover_valid_chain(srd_ctx* c, const uint8_t* file, uint64_t flen, uint64_t* final_len) {
  if (!final_len) { set_err("bad argument"); return SRD_ERR_ARG; }
  if (!c) { set_err("bad argument"); return SRD_ERR_ARG; }
  HIPCHK(hipSetDevice(c->device));
  const uint8_t* d = nullptr;
  TRY(stage_host(c, file, flen, 0, &d));
  srd_device_result r;
  TRY(srd_validate_index_device(c, d, flen, SRD_FLAG_NO_CRC, &r));
  *final_len = r.final_len;
  return 0;
}

extern "C" int srd_key_indexer_build(srd_ctx* c, const uint8_t* file, uint64_t tail, uint64_t* keys,
                                     uint64_t* packed, uint64_t cap, uint64_t* n_out) {
  if (!n_out) { set_err("bad argument"); return SRD_ERR_ARG; }
  if (!c) { set_err("bad argument"); return SRD_ERR_ARG; }
  HIPCHK(hipSetDevice(c->device));
  const uint8_t* d = nullptr;
  TRY(stage_host(c, file, tail, 0, &d));
  srd_device_result r;
  TRY(srd_validate_index_device(c, d, tail, SRD_FLAG_NO_CRC, &r));
  if (r.final_len != tail) {
    set_err("tail is not a valid chain tail (KeyIndexer::build expects the recovered tail)");
    return SRD_ERR_ARG;
  }
  *n_out = r.n_index;
  uint64_t k = std::min(cap, r.n_index);
  if (k) {
    HIPCHK(hipMemcpyAsync(keys, r.index_key_hash, k * 8, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(hipMemcpyAsync(packed, r.index_packed, k * 8, hipMemcpyDeviceToHost, c->stream));
  }
  HIPCHK(spin_sync(c->stream));
  return 0;
}
