// srd_ops.hip -- host launch code of the remaining kernel families (included
// by srd_api.hip): stream probe, batch digests, synth, batch writer, device
// lookup table, batched reads and the table's maintenance, iterator and
// compaction, payload gather and scatter, device append, segment append, live
// compaction.

// A device allocation / an event that lasts for one call, released on every return path
// (no workspace buffer: as large as the caller's input, the context would keep and report it)
struct DevTmp {
  void* p = nullptr;
  DevTmp() = default;
  DevTmp(const DevTmp&) = delete;
  ~DevTmp() { if (p) hipFree(p); }
  hipError_t alloc(size_t bytes) { return hipMalloc(&p, bytes); }
};
struct EventTmp {
  hipEvent_t e = nullptr;
  EventTmp() = default;
  EventTmp(const EventTmp&) = delete;
  ~EventTmp() { if (e) hipEventDestroy(e); }
};

extern "C" int srd_stream_probe_device(srd_ctx* c, const uint8_t* d_buf, uint64_t bytes, int reps, double* best_ms,
                                       double* median_ms) {
  if (!c || !d_buf || bytes < TILE || reps < 1 || !best_ms) { set_err("bad argument"); return SRD_ERR_ARG; }
  HIPCHK(hipSetDevice(c->device));
  const uint64_t ntiles = bytes / TILE;
  TRY(ensure(c, B_PROBE, (uint64_t)c->scan_blocks * 16 * 4));
  EventTmp e[2];
  for (auto& x : e) HIPCHK(hipEventCreateWithFlags(&x.e, hipEventReleaseToDevice));
  std::vector<float> ms;
  for (int r = 0; r < reps + 1; r++) {  // (the first run warms the code and the TLB)
    hipExtLaunchKernelGGL(stream_probe_kernel, dim3(c->scan_blocks), dim3(1024), 0, c->stream, e[0].e, e[1].e, 0,
                          d_buf, ntiles, P<uint32_t>(c, B_PROBE));
    float t = 0;
    if (hipGetLastError() != hipSuccess || hipEventSynchronize(e[1].e) != hipSuccess ||
        hipEventElapsedTime(&t, e[0].e, e[1].e) != hipSuccess) {
      set_err("stream probe launch failed");
      return SRD_ERR_HIP;
    }
    if (r) ms.push_back(t);
  }
  std::sort(ms.begin(), ms.end());
  *best_ms = ms[0];
  if (median_ms) *median_ms = ms[ms.size() / 2];
  return 0;
}

extern "C" int srd_crc32_batch_device(srd_ctx* c, const uint8_t* d_buf, const uint64_t* d_offs,
                                      const uint64_t* d_lens, uint64_t n, uint32_t* d_out, void* stream) {
  if (!c) { set_err("bad argument"); return SRD_ERR_ARG; }
  hipStream_t s = stream_of(c, stream);
  if (!n) return 0;
  crc_batch_kernel<<<(unsigned)std::min<uint64_t>(n, 8192), 64, 0, s>>>(d_buf, d_offs, d_lens, n, d_out);
  LAUNCHED(s, "crc_batch_kernel");
  return 0;
}

extern "C" int srd_xxh3_64_batch_device(srd_ctx* c, const uint8_t* d_keys, const uint64_t* d_offs,
                                        const uint64_t* d_lens, uint64_t n, uint64_t* d_out, void* stream) {
  if (!c) { set_err("bad argument"); return SRD_ERR_ARG; }
  hipStream_t s = stream_of(c, stream);
  if (!n) return 0;
  xxh3_batch_kernel<<<blocks(n, 256), 256, 0, s>>>(d_keys, d_offs, d_lens, n, d_out);
  LAUNCHED(s, "xxh3_batch_kernel");
  return 0;
}

template <class OUT, class F>
static int batch_host(srd_ctx* c, const uint8_t* buf, uint64_t blen, const uint64_t* offs, const uint64_t* lens,
                      uint64_t n, OUT* out, F launch) {
  HIPCHK(hipSetDevice(c->device));
  for (uint64_t i = 0; i < n; i++)
    if (offs[i] > blen || lens[i] > blen - offs[i]) { set_err("range out of bounds"); return SRD_ERR_ARG; }
  DevTmp db, dof, dl, dout;
  HIPCHK(db.alloc(blen + 1));
  HIPCHK(dof.alloc(n * 8 + 8));
  HIPCHK(dl.alloc(n * 8 + 8));
  HIPCHK(dout.alloc(n * sizeof(OUT) + 8));
  if (blen) HIPCHK(hipMemcpyAsync(db.p, buf, blen, hipMemcpyHostToDevice, c->stream));
  if (n) {
    HIPCHK(hipMemcpyAsync(dof.p, offs, n * 8, hipMemcpyHostToDevice, c->stream));
    HIPCHK(hipMemcpyAsync(dl.p, lens, n * 8, hipMemcpyHostToDevice, c->stream));
  }
  int r = launch((const uint8_t*)db.p, (const uint64_t*)dof.p, (const uint64_t*)dl.p, (OUT*)dout.p);
  if (!r && n) HIPCHK(hipMemcpyAsync(out, dout.p, n * sizeof(OUT), hipMemcpyDeviceToHost, c->stream));
  HIPCHK(spin_sync(c->stream));
  return r;
}

extern "C" int srd_crc32_batch(srd_ctx* c, const uint8_t* buf, uint64_t blen, const uint64_t* offs,
                               const uint64_t* lens, uint64_t n, uint32_t* out) {
  if (!c || (n && (!offs || !lens || !out))) { set_err("bad argument"); return SRD_ERR_ARG; }
  return batch_host<uint32_t>(c, buf, blen, offs, lens, n, out, [&](auto db, auto dof, auto dl, auto dout) {
    return srd_crc32_batch_device(c, db, dof, dl, n, dout, nullptr);
  });
}

extern "C" int srd_xxh3_64_batch(srd_ctx* c, const uint8_t* keys, uint64_t klen, const uint64_t* offs,
                                 const uint64_t* lens, uint64_t n, uint64_t* out) {
  if (!c || (n && (!offs || !lens || !out))) { set_err("bad argument"); return SRD_ERR_ARG; }
  return batch_host<uint64_t>(c, keys, klen, offs, lens, n, out, [&](auto db, auto dof, auto dl, auto dout) {
    return srd_xxh3_64_batch_device(c, db, dof, dl, n, dout, nullptr);
  });
}

// entry tails: lens (if given) holds the lengths of entries 0 .. first+n-1
static int synth_offsets(uint64_t first, uint64_t n, uint64_t fixed_len, const uint64_t* lens, uint64_t span_off,
                         std::vector<uint64_t>* off, uint64_t* e0, uint64_t* lo, uint64_t* hi) {
  uint64_t tail = 0;
  *lo = 0;
  *e0 = first;
  bool have_e0 = false;
  if (off) off->clear();
  for (uint64_t i = 0; i < first + n; i++) {
    const uint64_t L = lens ? lens[i] : fixed_len;
    if (L == 0) { set_err("empty payload"); return SRD_ERR_ARG; }
    if (i == first) *lo = tail;
    const uint64_t end = tail + ((64 - tail % 64) & 63) + L + 20;
    if (!have_e0 && (end > span_off || i == first)) { *e0 = i; have_e0 = true; }
    if (have_e0 && off) off->push_back(tail);
    tail = end;
  }
  *hi = tail;
  return 0;
}

static int synth_launch(Ctx* c, uint8_t* d_abs, const std::vector<uint64_t>& off, uint64_t e0, uint64_t fixed_len,
                        const uint64_t* lens, uint64_t seed, uint64_t clip_lo) {
  const uint64_t n = off.size();
  if (!n) return 0;
  HIPCHK(hipSetDevice(c->device));
  DevTmp doff, dl;
  HIPCHK(doff.alloc(n * 8));
  HIPCHK(hipMemcpyAsync(doff.p, off.data(), n * 8, hipMemcpyHostToDevice, c->stream));
  if (lens) {
    HIPCHK(dl.alloc(n * 8));
    HIPCHK(hipMemcpyAsync(dl.p, lens + e0, n * 8, hipMemcpyHostToDevice, c->stream));
  }
  synth_kernel<<<(unsigned)std::min<uint64_t>(n, 65536), 64, 0, c->stream>>>(
      d_abs, (const uint64_t*)doff.p, (const uint64_t*)dl.p, fixed_len, n, seed, e0, clip_lo);
  LAUNCHED(c->stream, "synth_kernel");
  HIPCHK(spin_sync(c->stream));
  return 0;
}

extern "C" int srd_synth_store_device(srd_ctx* c, uint8_t* d_out, uint64_t n, uint64_t fixed_len,
                                      const uint64_t* lens, uint64_t seed, uint64_t* len_out) {
  if (!len_out) { set_err("bad argument"); return SRD_ERR_ARG; }
  std::vector<uint64_t> off;
  uint64_t e0, lo, hi;
  TRY(synth_offsets(0, n, fixed_len, lens, 0, d_out ? &off : nullptr, &e0, &lo, &hi));
  *len_out = hi;
  if (!d_out || !n) return 0;
  if (!c) { set_err("bad argument"); return SRD_ERR_ARG; }
  return synth_launch(c, d_out, off, 0, fixed_len, lens, seed, 0);
}

extern "C" int srd_synth_span_device(srd_ctx* c, uint8_t* d_span, uint64_t span_off, uint64_t first,
                                     uint64_t n, uint64_t fixed_len, const uint64_t* lens, uint64_t seed,
                                     uint64_t* lo_out, uint64_t* hi_out) {
  if (!lo_out || !hi_out || (span_off % SPAN_BYTES)) { set_err("bad argument"); return SRD_ERR_ARG; }
  std::vector<uint64_t> off;
  uint64_t e0, lo, hi;
  TRY(synth_offsets(first, n, fixed_len, lens, span_off, d_span ? &off : nullptr, &e0, &lo, &hi));
  *lo_out = lo;
  *hi_out = hi;
  if (!d_span || !n) return 0;
  if (!c || span_off > lo) { set_err("bad argument: span_off must be <= the shard's lower tail"); return SRD_ERR_ARG; }
  return synth_launch(c, d_span - span_off, off, e0, fixed_len, lens, seed, span_off);
}

// ---------------------------------------------------------------------------
// Checksum-on-append batch writer (C5): layout on the host (prepad_len chains
// every start to all earlier lengths), serialization + CRC + key hash on the
// device (write_kernel), chunked H2D of the inputs on a side stream.
extern "C" int srd_batch_layout(uint64_t tail, const uint8_t* payloads, const uint64_t* key_offs,
                                const uint64_t* key_lens, const uint64_t* pay_offs, const uint64_t* pay_lens,
                                uint64_t n, uint32_t flags, srd_write_entry* out, uint64_t* new_tail) {
  const char* why = "";
  const int r = srd_host::batch_layout(tail, payloads, key_offs, key_lens, pay_offs, pay_lens, n, flags, out, new_tail,
                                       &why);
  if (r) set_err(why);
  return r;
}

static int launch_write(Ctx* c, hipStream_t s, const uint8_t* pay, const uint8_t* keys, const srd_write_entry* ent,
                        uint64_t n, uint8_t* out, uint64_t base, uint64_t* kh, uint64_t* mo,
                        unsigned int* null_only = nullptr) {
  if (!n) return 0;
  WriteArgs w{pay, keys, ent, n, out, base, kh, mo, null_only};
  const unsigned g = (unsigned)std::min<uint64_t>((n + SCAN_WAVES_V2 - 1) / SCAN_WAVES_V2, c->scan_blocks);
#ifdef SRD_DEBUG_API
  if (c->scan_variant == 21)
    write_kernel<1><<<g, SCAN_WAVES_V2 * 64, 0, s>>>(w);
  else if (c->scan_variant == 22)
    write_kernel<2><<<g, SCAN_WAVES_V2 * 64, 0, s>>>(w);
  else if (c->scan_variant == 29)
    write_kernel<9><<<g, SCAN_WAVES_V2 * 64, 0, s>>>(w);
  else
#endif
    write_kernel<<<g, SCAN_WAVES_V2 * 64, 0, s>>>(w);
  LAUNCHED(s, "write_kernel");
  return 0;
}

extern "C" int srd_batch_write_device(srd_ctx* c, const uint8_t* d_keys, const uint8_t* d_payloads,
                                      const srd_write_entry* d_entries, uint64_t n, uint8_t* d_out,
                                      uint64_t out_base, uint64_t* d_kh_out, uint64_t* d_mo_out, void* stream) {
  if (!c || (out_base & 63) ||
      (n && (!d_keys || !d_payloads || !d_entries || !d_out || !d_kh_out || !d_mo_out))) {
    set_err("bad argument");
    return SRD_ERR_ARG;
  }
  HIPCHK(hipSetDevice(c->device));
  return launch_write(c, stream_of(c, stream), d_payloads, d_keys, d_entries, n, d_out, out_base, d_kh_out, d_mo_out);
}

extern "C" int srd_batch_write(srd_ctx* c, uint64_t tail, const uint8_t* keys, const uint64_t* key_offs,
                               const uint64_t* key_lens, const uint8_t* payloads, const uint64_t* pay_offs,
                               const uint64_t* pay_lens, uint64_t n, uint32_t flags, uint8_t* d_out, uint64_t out_cap,
                               uint64_t* new_tail, uint64_t* kh_out, uint64_t* mo_out) {
  if (!c || !new_tail || (n && (!payloads || !keys))) { set_err("bad argument"); return SRD_ERR_ARG; }
  std::vector<srd_write_entry> E(n);
  uint64_t nt = 0;
  TRY(srd_batch_layout(tail, payloads, key_offs, key_lens, pay_offs, pay_lens, n, flags, E.data(), &nt));
  *new_tail = nt;
  if (!d_out || !n) return 0;
  const uint64_t base = tail & ~63ull;
  if (nt - base > out_cap) { set_err("out_cap too small for the batch"); return SRD_ERR_ARG; }
  HIPCHK(hipSetDevice(c->device));
  constexpr uint64_t CH = 64ull << 20;  // payload bytes per chunk (double-buffered in HBM)
  constexpr uint64_t KCH = 8ull << 20;  // key bytes per chunk
  constexpr uint64_t ENT_MAX = 1u << 16;
  if (!c->cstream) {
    HIPCHK(hipStreamCreateWithFlags(&c->cstream, hipStreamNonBlocking));
    for (int i = 0; i < 2; i++) {
      HIPCHK(hipEventCreateWithFlags(&c->wev_copied[i], hipEventDisableTiming));
      HIPCHK(hipEventCreateWithFlags(&c->wev_done[i], hipEventDisableTiming));
      HIPCHK(hipHostMalloc(&c->pin_ent[i], ENT_MAX * sizeof(srd_write_entry), hipHostMallocDefault));
    }
  }
  TRY(ensure(c, B_WKH, n * 8));
  TRY(ensure(c, B_WMO, n * 8));
  uint64_t* kh_dev = P<uint64_t>(c, B_WKH);
  uint64_t* mo_dev = P<uint64_t>(c, B_WMO);
  uint64_t e0 = 0;
  for (int ci = 0; e0 < n; ci++) {
    // a chunk: consecutive entries whose payload and key source ranges stay
    // within CH / KCH (one entry at least); the ranges are copied as they lie
    uint64_t plo = E[e0].src, phi = E[e0].src + E[e0].len;
    uint64_t klo = E[e0].key_src, khi = klo + E[e0].key_len;
    uint64_t e1 = e0 + 1;
    while (e1 < n && e1 - e0 < ENT_MAX) {
      const uint64_t pl2 = std::min(plo, E[e1].src), ph2 = std::max(phi, E[e1].src + E[e1].len);
      const uint64_t kl2 = std::min(klo, E[e1].key_src), kh2 = std::max(khi, E[e1].key_src + E[e1].key_len);
      if (ph2 - (pl2 & ~15ull) > CH || kh2 - kl2 > KCH) break;
      plo = pl2; phi = ph2; klo = kl2; khi = kh2;
      e1++;
    }
    const uint64_t pa = plo & ~15ull;  // keeps every source's 16-byte alignment in the staging buffer
    const int slot = ci & 1;
    if (ci >= 2) HIPCHK(hipEventSynchronize(c->wev_done[slot]));  // chunk ci-2's kernel has released the slot
    TRY(ensure(c, (BufId)(B_WPAY0 + slot), phi - pa));
    TRY(ensure(c, (BufId)(B_WKEY0 + slot), std::max<uint64_t>(khi - klo, 1)));
    TRY(ensure(c, (BufId)(B_WENT0 + slot), ENT_MAX * sizeof(srd_write_entry)));
    srd_write_entry* pe = (srd_write_entry*)c->pin_ent[slot];
    for (uint64_t i = e0; i < e1; i++) {
      pe[i - e0] = E[i];
      pe[i - e0].src -= pa;
      pe[i - e0].key_src -= klo;
    }
    HIPCHK(hipMemcpyAsync(P<void>(c, (BufId)(B_WPAY0 + slot)), payloads + pa, phi - pa, hipMemcpyHostToDevice,
                          c->cstream));
    if (khi > klo)
      HIPCHK(hipMemcpyAsync(P<void>(c, (BufId)(B_WKEY0 + slot)), keys + klo, khi - klo, hipMemcpyHostToDevice,
                            c->cstream));
    HIPCHK(hipMemcpyAsync(P<void>(c, (BufId)(B_WENT0 + slot)), pe, (e1 - e0) * sizeof(srd_write_entry),
                          hipMemcpyHostToDevice, c->cstream));
    HIPCHK(hipEventRecord(c->wev_copied[slot], c->cstream));
    HIPCHK(hipStreamWaitEvent(c->stream, c->wev_copied[slot], 0));
    TRY(launch_write(c, c->stream, P<uint8_t>(c, (BufId)(B_WPAY0 + slot)), P<uint8_t>(c, (BufId)(B_WKEY0 + slot)),
                     P<srd_write_entry>(c, (BufId)(B_WENT0 + slot)), e1 - e0, d_out, base, kh_dev + e0, mo_dev + e0));
    HIPCHK(hipEventRecord(c->wev_done[slot], c->stream));
    e0 = e1;
  }
  if (kh_out) HIPCHK(hipMemcpyAsync(kh_out, kh_dev, n * 8, hipMemcpyDeviceToHost, c->stream));
  if (mo_out) HIPCHK(hipMemcpyAsync(mo_out, mo_dev, n * 8, hipMemcpyDeviceToHost, c->stream));
  HIPCHK(spin_sync(c->stream));
  return 0;
}

// ---------------------------------------------------------------------------
// Device KeyIndexer table + batched keyed reads (srd_table.h, srd_index.hip)
extern "C" uint64_t srd_index_table_bytes(uint64_t n) { return table_bytes_for(n); }
static unsigned grid_for(uint64_t n) { return (unsigned)std::max<uint64_t>(1, std::min<uint64_t>((n + 255) / 256, 8192)); }

// the build enqueued on the context stream: every slot empty, then one claim per pair
static int table_build_run(Ctx* c, const uint64_t* d_keys, const uint64_t* d_packed, uint64_t n, void* d_table,
                           uint64_t table_bytes) {
  const Table t = table_view(d_table, table_bytes);
  HIPCHK(hipMemsetAsync(t.packed, 0xFF, (1ull << t.log2cap) * 8, c->stream));
  if (n) idx_table_insert_kernel<<<grid_for(n), 256, 0, c->stream>>>(d_keys, d_packed, n, t);
  LAUNCHED(c->stream, "idx_table_insert_kernel");
  return 0;
}

extern "C" int srd_index_table_build_device(srd_ctx* c, const uint64_t* d_keys, const uint64_t* d_packed, uint64_t n,
                                            void* d_table, uint64_t table_bytes) {
  if (!c || !d_table || (n && (!d_keys || !d_packed)) || table_bytes < srd_index_table_bytes(n)) {
    set_err("bad argument (table_bytes < srd_index_table_bytes(n)?)");
    return SRD_ERR_ARG;
  }
  HIPCHK(hipSetDevice(c->device));
  TRY(table_build_run(c, d_keys, d_packed, n, d_table, table_bytes));
  HIPCHK(spin_sync(c->stream));
  return 0;
}

extern "C" int srd_index_get_packed_device(srd_ctx* c, const void* d_table, uint64_t table_bytes,
                                           const uint64_t* d_hashes, uint64_t n, uint64_t* d_packed_out,
                                           void* stream) {
  if (!c || !table_ok(d_table, table_bytes) || (n && (!d_hashes || !d_packed_out))) {
    set_err("bad argument");
    return SRD_ERR_ARG;
  }
  if (!n) return 0;
  HIPCHK(hipSetDevice(c->device));
  hipStream_t s = stream_of(c, stream);
  idx_get_packed_kernel<<<grid_for(n), 256, 0, s>>>(table_view(d_table, table_bytes), d_hashes, n, d_packed_out);
  LAUNCHED(s, "idx_get_packed_kernel");
  return 0;
}

extern "C" int srd_batch_read_hashed_device(srd_ctx* c, const void* d_table, uint64_t table_bytes,
                                            const uint8_t* d_file, uint64_t flen, const uint64_t* d_hashes,
                                            const uint64_t* d_verify, uint64_t n, uint64_t* d_start, uint64_t* d_end,
                                            void* stream) {
  if (!c || !table_ok(d_table, table_bytes) || (n && (!d_hashes || !d_start || !d_end || (flen && !d_file)))) {
    set_err("bad argument");
    return SRD_ERR_ARG;
  }
  if (!n) return 0;
  HIPCHK(hipSetDevice(c->device));
  hipStream_t s = stream_of(c, stream);
  batch_read_kernel<<<grid_for(n), 256, 0, s>>>(table_view(d_table, table_bytes), d_file, flen, d_hashes, d_verify, n,
                                                d_start, d_end);
  LAUNCHED(s, "batch_read_kernel");
  return 0;
}

extern "C" int srd_batch_read(srd_ctx* c, const void* d_table, uint64_t table_bytes, const uint8_t* d_file,
                              uint64_t flen, const uint8_t* keys, const uint64_t* key_offs, const uint64_t* key_lens,
                              uint64_t n, uint64_t* start_out, uint64_t* end_out) {
  if (!c || (n && (!keys || !key_offs || !key_lens || !start_out || !end_out))) {
    set_err("bad argument");
    return SRD_ERR_ARG;
  }
  if (!n) return 0;
  HIPCHK(hipSetDevice(c->device));
  uint64_t klen = 0;
  for (uint64_t i = 0; i < n; i++) klen = std::max(klen, key_offs[i] + key_lens[i]);
  DevTmp dk, dof, dl, dh, ds, de;
  if (dk.alloc(klen + 1) || dof.alloc(n * 8) || dl.alloc(n * 8) || dh.alloc(n * 8) || ds.alloc(n * 8) ||
      de.alloc(n * 8)) {
    set_err("hipMalloc failed");
    return SRD_ERR_ALLOC;
  }
  if (klen) HIPCHK(hipMemcpyAsync(dk.p, keys, klen, hipMemcpyHostToDevice, c->stream));
  HIPCHK(hipMemcpyAsync(dof.p, key_offs, n * 8, hipMemcpyHostToDevice, c->stream));
  HIPCHK(hipMemcpyAsync(dl.p, key_lens, n * 8, hipMemcpyHostToDevice, c->stream));
  int r = srd_xxh3_64_batch_device(c, (const uint8_t*)dk.p, (const uint64_t*)dof.p, (const uint64_t*)dl.p, n,
                                   (uint64_t*)dh.p, nullptr);  // compute_hash_batch (data_store.rs:1112)
  // batch_read verifies every key by its own tag (Some(keys), :1113)
  if (!r) r = srd_batch_read_hashed_device(c, d_table, table_bytes, d_file, flen, (const uint64_t*)dh.p,
                                           (const uint64_t*)dh.p, n, (uint64_t*)ds.p, (uint64_t*)de.p, nullptr);
  if (!r) {
    HIPCHK(hipMemcpyAsync(start_out, ds.p, n * 8, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(hipMemcpyAsync(end_out, de.p, n * 8, hipMemcpyDeviceToHost, c->stream));
  }
  HIPCHK(spin_sync(c->stream));
  return r;
}

// ---------------------------------------------------------------------------
// The table kept live (srd_index_live.hip): reindex, export, batched delete

// reindex (data_store.rs:224-259) of n pairs on stream s: dedupe and look up
// (the table is only read), one host wait for the counts, then the commit.
// SRD_ERR_FULL leaves the table as it was: nothing has written it yet.
static int apply_impl(Ctx* c, void* d_table, uint64_t table_bytes, uint64_t* used, const uint64_t* kh,
                      const uint64_t* mo, const uint8_t* tomb, uint64_t n, srd_index_apply_stats* stats,
                      hipStream_t s) {
  if (stats) *stats = srd_index_apply_stats{0, 0, 0};
  if (!n) return 0;
  HIPCHK(hipSetDevice(c->device));
  uint32_t log2dc = 6;
  while ((1ull << log2dc) < 2 * n) log2dc++;
  const uint64_t dc = 1ull << log2dc;
  TRY(ensure(c, B_LV_DSLOT, dc * 4));
  TRY(ensure(c, B_LV_DTOMB, dc / 32 * 4));
  TRY(ensure(c, B_LV_LSLOT, n * 4));
  TRY(ensure(c, B_LV_OPS, n * 8));
  TRY(ensure(c, B_LV_OPV, n * 8));
  TRY(ensure(c, B_LV_CNT, 64));
  LiveArgs a{};
  a.kh = kh;
  a.mo = mo;
  a.tomb = tomb;
  a.n = n;
  a.dslot = P<uint32_t>(c, B_LV_DSLOT);
  a.dtomb = P<uint32_t>(c, B_LV_DTOMB);
  a.log2dc = log2dc;
  a.lslot = P<uint32_t>(c, B_LV_LSLOT);
  a.t = table_view(d_table, table_bytes);
  a.op_slot = P<uint64_t>(c, B_LV_OPS);
  a.op_val = P<uint64_t>(c, B_LV_OPV);
  a.cnt = P<unsigned long long>(c, B_LV_CNT);
  HIPCHK(hipMemsetAsync(a.dslot, 0, dc * 4, s));
  HIPCHK(hipMemsetAsync(a.dtomb, 0, dc / 32 * 4, s));
  HIPCHK(hipMemsetAsync(a.cnt, 0, 32, s));
  live_dedupe_kernel<<<grid_for(n), 256, 0, s>>>(a);
  LAUNCHED(s, "live_dedupe_kernel");
  live_lookup_kernel<<<grid_for(n), 256, 0, s>>>(a);
  LAUNCHED(s, "live_lookup_kernel");
  struct { unsigned long long ins, upd, rem, fresh; } h;
  TRY(read_small(c, s, {SmallRead{a.cnt, &h, sizeof h}}));
  if (!table_admits(*used, h.fresh, a.t.log2cap)) {
    set_err("index table full: " + std::to_string(*used) + " used slots + " + std::to_string(h.fresh) +
            " new keys exceed half of " + std::to_string(1ull << a.t.log2cap));
    return SRD_ERR_FULL;
  }
  if (h.ins + h.upd + h.rem) live_commit_kernel<<<grid_for(n), 256, 0, s>>>(a);
  LAUNCHED(s, "live_commit_kernel");
  *used += h.fresh;
  if (stats) *stats = srd_index_apply_stats{h.ins, h.upd, h.rem};
  return 0;
}

extern "C" int srd_index_table_apply_device(srd_ctx* c, void* d_table, uint64_t table_bytes, uint64_t* used,
                                            const uint64_t* d_key_hashes, const uint64_t* d_meta_offs,
                                            const uint8_t* d_tomb, uint64_t n, srd_index_apply_stats* stats,
                                            void* stream) {
  if (!c || !table_ok(d_table, table_bytes) || !used || n >= (1ull << 31) || (n && (!d_key_hashes || !d_meta_offs))) {
    set_err("bad argument");
    return SRD_ERR_ARG;
  }
  return apply_impl(c, d_table, table_bytes, used, d_key_hashes, d_meta_offs, d_tomb, n, stats, stream_of(c, stream));
}

// The export enqueued on the context stream: the count (one wait), the gather
// of the live pairs and their sort.  *keys_out / *packed_out are the caller's
// arrays of cap_out elements (both null: the count only); with ws they are
// context workspace sized by the count and handed back (srd_compact_live_device).
static int export_run(Ctx* c, const void* d_table, uint64_t table_bytes, uint64_t** keys_out, uint64_t** packed_out,
                      uint64_t cap_out, bool ws, uint64_t* n_live) {
  const Table t = table_view(d_table, table_bytes);
  const uint64_t cap = 1ull << t.log2cap;
  TRY(ensure(c, B_LV_CNT, 64));
  unsigned long long* cnt = P<unsigned long long>(c, B_LV_CNT) + 4;
  HIPCHK(hipMemsetAsync(cnt, 0, 8, c->stream));
  live_count_kernel<<<grid_for(cap), 256, 0, c->stream>>>(t.packed, cap, cnt);
  LAUNCHED(c->stream, "live_count_kernel");
  unsigned long long nl = 0;
  TRY(read_small(c, c->stream, {rd(cnt, &nl)}));
  *n_live = nl;
  if (!(ws || *keys_out) || !nl) return 0;
  if (ws) {
    TRY(ensure(c, B_CL_XK, nl * 8));
    TRY(ensure(c, B_CL_XP, nl * 8));
    *keys_out = P<uint64_t>(c, B_CL_XK);
    *packed_out = P<uint64_t>(c, B_CL_XP);
    cap_out = nl;
  }
  if (nl > cap_out) { set_err("cap_out too small for the live pairs"); return SRD_ERR_ARG; }
  if (nl >= (1ull << 31)) { set_err("too many pairs"); return SRD_ERR_ARG; }
  // file order = ascending metadata offset: the offsets are distinct, so a
  // radix sort over the 48 offset bits of the packed words fixes the order
  // whatever order the gather's atomic counter handed out
  TRY(ensure(c, B_LV_XK, nl * 8));
  TRY(ensure(c, B_LV_XP, nl * 8));
  HIPCHK(hipMemsetAsync(cnt, 0, 8, c->stream));
  live_gather_kernel<<<grid_for(cap), 256, 0, c->stream>>>(t.keys, t.packed, cap, cnt, P<uint64_t>(c, B_LV_XK),
                                                          P<uint64_t>(c, B_LV_XP), nl);
  LAUNCHED(c->stream, "live_gather_kernel");
  TRY(sort_pairs48(c, P<uint64_t>(c, B_LV_XP), *packed_out, P<uint64_t>(c, B_LV_XK), *keys_out, nl));
  return 0;
}

extern "C" int srd_index_table_export_device(srd_ctx* c, const void* d_table, uint64_t table_bytes,
                                             uint64_t* d_keys_out, uint64_t* d_packed_out, uint64_t cap_out,
                                             uint64_t* n_live) {
  if (!c || !table_ok(d_table, table_bytes) || !n_live || (!d_keys_out != !d_packed_out)) {
    set_err("bad argument");
    return SRD_ERR_ARG;
  }
  HIPCHK(hipSetDevice(c->device));
  TRY(export_run(c, d_table, table_bytes, &d_keys_out, &d_packed_out, cap_out, false, n_live));
  HIPCHK(spin_sync(c->stream));
  return 0;
}

// nk tombstones at `tail` on the context stream, one per flagged hash of q[n]
// in the order pos gives (the exclusive sum of flag; nk >= 1 its total), and
// the keys removed from the table: the delete's second half, and what a TTL
// eviction ends in.  Refused with nothing written when the tombstones do not
// fit file_cap; waits for the stream at the end.
static int tombs_commit(Ctx* c, void* d_table, uint64_t table_bytes, uint64_t* used, const uint64_t* q,
                        const uint32_t* flag, const uint32_t* pos, uint64_t n, uint64_t nk, uint64_t tail,
                        uint8_t* d_file, uint64_t file_cap, uint64_t* new_tail) {
  const uint64_t nt = tail + 21 * nk;
  if (srd_padded_size(nt) > file_cap) { set_err("file_cap too small for the tombstones"); return SRD_ERR_ARG; }
  TRY(ensure(c, B_LV_ENT, nk * sizeof(srd_write_entry)));
  TRY(ensure(c, B_LV_TOMB, nk));
  TRY(ensure(c, B_WKH, nk * 8));
  TRY(ensure(c, B_WMO, nk * 8));
  live_tomb_entries_kernel<<<grid_for(n), 256, 0, c->stream>>>(q, flag, pos, n, tail, P<srd_write_entry>(c, B_LV_ENT));
  LAUNCHED(c->stream, "live_tomb_entries_kernel");
  HIPCHK(hipMemsetAsync(P<void>(c, B_LV_TOMB), 1, nk, c->stream));
  // (a tombstone reads no payload or key bytes: d_file only stands for the payload base)
  TRY(launch_write(c, c->stream, d_file, nullptr, P<srd_write_entry>(c, B_LV_ENT), nk, d_file, 0,
                   P<uint64_t>(c, B_WKH), P<uint64_t>(c, B_WMO)));
  // every kept key was present and every pair is a tombstone: the apply
  // removes them all and needs no new slot, so it cannot be refused
  TRY(apply_impl(c, d_table, table_bytes, used, P<uint64_t>(c, B_WKH), P<uint64_t>(c, B_WMO), P<uint8_t>(c, B_LV_TOMB),
                 nk, nullptr, c->stream));
  HIPCHK(spin_sync(c->stream));
  *new_tail = nt;
  return 0;
}

extern "C" int srd_batch_delete_hashed_device(srd_ctx* c, void* d_table, uint64_t table_bytes, uint64_t* used,
                                              const uint64_t* d_hashes, uint64_t n, uint64_t tail, uint8_t* d_file,
                                              uint64_t file_cap, uint64_t* new_tail, uint64_t* n_deleted) {
  if (!c || !table_ok(d_table, table_bytes) || !used || !new_tail || n >= (1ull << 31) ||
      (n && (!d_hashes || !d_file))) {
    set_err("bad argument");
    return SRD_ERR_ARG;
  }
  *new_tail = tail;
  if (n_deleted) *n_deleted = 0;
  if (!n) return 0;
  HIPCHK(hipSetDevice(c->device));
  TRY(ensure(c, B_LV_FLAG, n * 4));
  TRY(ensure(c, B_LV_POS, n * 4));
  uint32_t* flag = P<uint32_t>(c, B_LV_FLAG);
  uint32_t* pos = P<uint32_t>(c, B_LV_POS);
  TRY(ensure_scan(c, flag, pos, n));
  live_present_kernel<<<grid_for(n), 256, 0, c->stream>>>(table_view(d_table, table_bytes), d_hashes, n, flag);
  LAUNCHED(c->stream, "live_present_kernel");
  uint64_t nk = 0;
  TRY(scan_sum_total(c, flag, pos, n, c->stream, &nk));
  if (!nk) return 0;  // (the reference returns the unchanged tail: data_store.rs:1011-1014)
  TRY(tombs_commit(c, d_table, table_bytes, used, d_hashes, flag, pos, n, nk, tail, d_file, file_cap, new_tail));
  if (n_deleted) *n_deleted = nk;
  return 0;
}

// ---------------------------------------------------------------------------
// par_iter_entries / EntryIterator, estimate_compaction_savings and compact
// over the device index (srd_index.hip iter_* kernels + the writer)
static int iter_run(Ctx* c, const uint8_t* d_file, uint64_t flen, const uint64_t* d_packed, uint64_t n,
                    uint64_t* d_start, uint64_t* d_end, uint64_t* d_meta, uint64_t* d_kh, uint64_t* n_out,
                    uint64_t* kept_bytes) {
  *n_out = 0;
  if (kept_bytes) *kept_bytes = 0;
  if (!n) return 0;
  HIPCHK(hipSetDevice(c->device));
  TRY(ensure(c, B_IT_FLAG, n * 4));
  TRY(ensure(c, B_IT_POS, n * 4));
  TRY(ensure(c, B_IT_ST, n * 8));
  TRY(ensure(c, B_IT_EN, n * 8));
  TRY(ensure(c, B_IT_KEPT, 64));
  uint32_t* flag = P<uint32_t>(c, B_IT_FLAG);
  uint32_t* pos = P<uint32_t>(c, B_IT_POS);
  TRY(ensure_scan(c, flag, pos, n));
  unsigned long long* kept = P<unsigned long long>(c, B_IT_KEPT);
  HIPCHK(hipMemsetAsync(kept, 0, 8, c->stream));
  iter_flag_kernel<<<grid_for(n), 256, 0, c->stream>>>(d_file, flen, d_packed, n, flag, P<uint64_t>(c, B_IT_ST),
                                                       P<uint64_t>(c, B_IT_EN), kept);
  LAUNCHED(c->stream, "iter_flag_kernel");
  uint64_t nv = 0;
  unsigned long long hk = 0;
  TRY(scan_sum_total(c, flag, pos, n, c->stream, &nv, rd(kept, &hk)));
  if (d_start && nv) {
    iter_emit_kernel<<<grid_for(n), 256, 0, c->stream>>>(d_file, d_packed, flag, pos, n, nv, P<uint64_t>(c, B_IT_ST),
                                                         P<uint64_t>(c, B_IT_EN), d_start, d_end, d_meta, d_kh);
    LAUNCHED(c->stream, "iter_emit_kernel");
    HIPCHK(spin_sync(c->stream));
  }
  *n_out = nv;
  if (kept_bytes) *kept_bytes = hk;
  return 0;
}

extern "C" int srd_iter_entries_device(srd_ctx* c, const uint8_t* d_file, uint64_t flen, const uint64_t* d_packed,
                                       uint64_t n_index, uint64_t* d_start, uint64_t* d_end, uint64_t* d_meta_off,
                                       uint64_t* d_key_hash, uint64_t* n_out) {
  if (!c || !n_out || (n_index && (!d_file || !d_packed || !d_start || !d_end))) {
    set_err("bad argument");
    return SRD_ERR_ARG;
  }
  return iter_run(c, d_file, flen, d_packed, n_index, d_start, d_end, d_meta_off, d_key_hash, n_out, nullptr);
}

extern "C" int srd_estimate_compaction_savings_device(srd_ctx* c, const uint8_t* d_file, uint64_t flen,
                                                      const uint64_t* d_packed, uint64_t n_index, uint64_t* savings) {
  if (!c || !savings || (n_index && (!d_file || !d_packed))) { set_err("bad argument"); return SRD_ERR_ARG; }
  uint64_t nv = 0, kept = 0;
  TRY(iter_run(c, d_file, flen, d_packed, n_index, nullptr, nullptr, nullptr, nullptr, &nv, &kept));
  *savings = flen > kept ? flen - kept : 0;  // total_size.saturating_sub(unique_entry_size)
  return 0;
}

extern "C" int srd_compact_device(srd_ctx* c, const uint8_t* d_file, uint64_t flen, const uint64_t* d_packed,
                                  uint64_t n_index, uint8_t* d_out, uint64_t out_cap, uint64_t* new_len,
                                  uint64_t* d_key_hash_out, uint64_t* d_meta_off_out) {
  if (!c || !new_len || (n_index && (!d_file || !d_packed))) { set_err("bad argument"); return SRD_ERR_ARG; }
  *new_len = 0;
  if (!n_index) return 0;
  TRY(ensure(c, B_IT_OST, n_index * 8));
  TRY(ensure(c, B_IT_OEN, n_index * 8));
  TRY(ensure(c, B_IT_OKH, n_index * 8));
  uint64_t nv = 0;
  TRY(iter_run(c, d_file, flen, d_packed, n_index, P<uint64_t>(c, B_IT_OST), P<uint64_t>(c, B_IT_OEN), nullptr,
               P<uint64_t>(c, B_IT_OKH), &nv, nullptr));
  // layout of the compacted file on the device: write_stream_with_key_hash
  // per entry in iter_entries order (data_store.rs:706-719, 758-825), tail
  // from 0 -- a prefix sum (compact_sizes_kernel), then the write entries
  if (!nv) return 0;
  const uint64_t* st = P<uint64_t>(c, B_IT_OST);
  const uint64_t* en = P<uint64_t>(c, B_IT_OEN);
  TRY(ensure(c, B_IT_RLEN, nv * 8));
  TRY(ensure(c, B_IT_PST, nv * 8));
  TRY(ensure(c, B_IT_ENT, nv * sizeof(srd_write_entry)));
  TRY(ensure(c, B_IT_KEPT, 64));
  TRY(ensure_scan(c, P<uint64_t>(c, B_IT_RLEN), P<uint64_t>(c, B_IT_PST), nv));
  compact_sizes_kernel<<<grid_for(nv), 256, 0, c->stream>>>(st, en, nv, P<uint64_t>(c, B_IT_RLEN));
  LAUNCHED(c->stream, "compact_sizes_kernel");
  TRY(scan_sum(c, P<uint64_t>(c, B_IT_RLEN), P<uint64_t>(c, B_IT_PST), nv));
  uint64_t* d_new_len = P<uint64_t>(c, B_IT_KEPT) + 2;
  compact_entries_kernel<<<grid_for(nv), 256, 0, c->stream>>>(st, en, P<uint64_t>(c, B_IT_OKH), P<uint64_t>(c, B_IT_PST),
                                                             nv, P<srd_write_entry>(c, B_IT_ENT), d_new_len);
  LAUNCHED(c->stream, "compact_entries_kernel");
  uint64_t tail = 0;
  TRY(read_small(c, c->stream, {rd(d_new_len, &tail)}));
  *new_len = tail;
  if (!d_out) return 0;
  if (tail > out_cap) { set_err("out_cap too small for the compacted store"); return SRD_ERR_ARG; }
  TRY(ensure(c, B_WKH, nv * 8));
  TRY(ensure(c, B_WMO, nv * 8));
  unsigned int* nullf = (unsigned int*)(P<uint8_t>(c, B_IT_KEPT) + 8);
  HIPCHK(hipMemsetAsync(nullf, 0, 4, c->stream));
  TRY(launch_write(c, c->stream, d_file, nullptr, P<srd_write_entry>(c, B_IT_ENT), nv, d_out, 0,
                   d_key_hash_out ? d_key_hash_out : P<uint64_t>(c, B_WKH),
                   d_meta_off_out ? d_meta_off_out : P<uint64_t>(c, B_WMO), nullf));
  unsigned int hn = 0;
  TRY(read_small(c, c->stream, {rd(nullf, &hn)}));
  if (hn) {  // write_stream rejects NULL-only payloads (data_store.rs:792-797); compact() fails with it
    set_err("NULL-byte-only streams cannot be written directly.");
    return SRD_ERR_ARG;
  }
  return 0;
}

// ---------------------------------------------------------------------------
// The streaming kernel (srd_stream.hip) over a unit table: one wave per unit up
// to the scan's grid, with the stream rule's OR where there is an nz array
static int launch_stream(Ctx* c, hipStream_t s, const StreamArgs& a) {
  const unsigned g = (unsigned)std::min<uint64_t>((a.n_units + SCAN_WAVES_V2 - 1) / SCAN_WAVES_V2, c->scan_blocks);
  if (a.nz) stream_copy_crc_kernel<true><<<g, SCAN_WAVES_V2 * 64, 0, s>>>(a);
  else stream_copy_crc_kernel<false><<<g, SCAN_WAVES_V2 * 64, 0, s>>>(a);
  LAUNCHED(s, "stream_copy_crc_kernel");
  return 0;
}

// A batch of entries moved in units (srd_units.hip): the unit table, the
// streaming kernel into out (nullptr: verify only) and the combine for the
// n_multi entries of more than one unit (units < 2^32: the caller's check)
template <class View>
static int stream_units_as(Ctx* c, hipStream_t s, UnitArgs a, uint64_t units, uint64_t n_multi, uint8_t* out, uint32_t* nz) {
  TRY(ensure(c, B_ST_UNIT, units * sizeof(SegUnit)));
  TRY(ensure(c, B_GA_RAW, units * 4));
  a.unit = P<SegUnit>(c, B_ST_UNIT);
  a.n_units = units;
  a.raw = P<uint32_t>(c, B_GA_RAW);
  units_kernel<View><<<grid_for(units), 256, 0, s>>>(a);
  LAUNCHED(s, "units_kernel");
  TRY(launch_stream(c, s, StreamArgs{a.unit, units, out, a.raw, a.crc, nz}));
  if (n_multi) {
    unit_terms_kernel<View><<<grid_for(units), 256, 0, s>>>(a);
    LAUNCHED(s, "unit_terms_kernel");
    unit_combine_kernel<View><<<(unsigned)std::min<uint64_t>((a.n + 3) / 4, 4096), 256, 0, s>>>(a);
    LAUNCHED(s, "unit_combine_kernel");
  }
  return 0;
}
// (a batch with a segment table is read through it -- ranges of a file
// delivered into a table: the scatter -- any other as ranges)
static int stream_units(Ctx* c, hipStream_t s, const UnitArgs& a, uint64_t units, uint64_t n_multi, uint8_t* out,
                        uint32_t* nz) {
  return a.segs ? a.start ? stream_units_as<ScatterView>(c, s, a, units, n_multi, out, nz)
                          : stream_units_as<TableView>(c, s, a, units, n_multi, out, nz)
                : stream_units_as<RangeView>(c, s, a, units, n_multi, out, nz);
}

// Verified payloads (srd_gather.hip): layout, one wait for the totals, then the
// unit table, the streaming kernel, the combine and the finish enqueued on the
// stream
extern "C" int srd_payload_gather_device(srd_ctx* c, const uint8_t* d_file, uint64_t flen, const uint64_t* d_start,
                                         const uint64_t* d_end, uint64_t n, uint32_t flags, uint8_t* d_out,
                                         uint64_t out_cap, uint64_t* d_out_off, uint8_t* d_status,
                                         uint32_t* d_crc_computed, uint64_t* total, void* stream) {
  const bool verify = flags & SRD_GATHER_VERIFY_ONLY;
  if (verify) d_out = nullptr;
  if (!c || !total || !d_out_off || n >= (1ull << 31) || (flags & ~SRD_GATHER_VERIFY_ONLY) ||
      (n && (!d_start || !d_end || !d_status || (flen && !d_file))) || ((uintptr_t)d_out & 15)) {
    set_err("bad argument");
    return SRD_ERR_ARG;
  }
  *total = 0;
  if (d_out) {  // the output may not lie in what the store's kernels read (srd_padded_size)
    const uintptr_t f0 = (uintptr_t)d_file, f1 = f0 + srd_padded_size(flen), o0 = (uintptr_t)d_out, o1 = o0 + out_cap;
    if (d_file && out_cap && o0 < f1 && f0 < o1) {
      set_err("d_out overlaps the store");
      return SRD_ERR_ARG;
    }
  }
  HIPCHK(hipSetDevice(c->device));
  hipStream_t s = stream_of(c, stream);
  if (!n) {
    HIPCHK(hipMemsetAsync(d_out_off, 0, 8, s));
    return 0;
  }
  TRY(ensure(c, B_GA_ST, n));
  TRY(ensure(c, B_GA_PLEN, n * 8));
  TRY(ensure(c, B_GA_CHK, n * 8));
  TRY(ensure(c, B_GA_OFF, n * 8));
  TRY(ensure(c, B_GA_CPRE, n * 8));
  TRY(ensure(c, B_GA_CRC, n * 4));
  TRY(ensure(c, B_GA_CNT, 64));
  TRY(ensure_scan(c, (const uint64_t*)nullptr, (uint64_t*)nullptr, n));  // both scans below
  PayloadGatherArgs a{};
  a.file = d_file;
  a.flen = flen;
  a.start = d_start;
  a.end = d_end;
  a.n = a.n_segs = n;
  a.st = P<uint8_t>(c, B_GA_ST);
  a.plen = P<uint64_t>(c, B_GA_PLEN);
  a.eun = P<uint64_t>(c, B_GA_CHK);
  a.off = P<uint64_t>(c, B_GA_OFF);
  a.upre = P<uint64_t>(c, B_GA_CPRE);
  a.pad = true;  // each hit's zero bytes up to the 64-byte boundary of the packed output
  a.cnt = P<unsigned long long>(c, B_GA_CNT);
  a.crc = P<uint32_t>(c, B_GA_CRC);
  a.o_off = d_out_off;
  a.o_status = d_status;
  a.o_crc = d_crc_computed;
  a.layout_only = !d_out && !verify;
  HIPCHK(hipMemsetAsync(a.cnt, 0, 8, s));
  payload_layout_kernel<<<grid_for(n), 256, 0, s>>>(a);
  LAUNCHED(s, "payload_layout_kernel");
  // both totals and the multi-chunk count on one wait (n < 2^31 fits hipCUB's int count)
  uint64_t off_last = 0, plen_last = 0, units = 0;
  unsigned long long n_multi = 0;
  TRY(scan_sum(c, (const uint64_t*)a.plen, a.off, n, s));
  TRY(scan_sum_total(c, (const uint64_t*)a.eun, a.upre, n, s, &units, rd(a.off + n - 1, &off_last),
                     rd(a.plen + n - 1, &plen_last), rd(a.cnt, &n_multi)));
  const uint64_t tot = off_last + plen_last;
  *total = tot;
  a.total = tot;
  if (d_out && tot > out_cap) {
    set_err("out_cap too small for the gathered payloads: " + std::to_string(tot) + " bytes");
    return SRD_ERR_ARG;
  }
  if (units >= (1ull << 32)) { set_err("too many work units in one batch"); return SRD_ERR_ARG; }
  if (!a.layout_only && units) TRY(stream_units(c, s, a, units, n_multi, d_out, nullptr));
  payload_finish_kernel<<<grid_for(n + 1), 256, 0, s>>>(a);
  LAUNCHED(s, "payload_finish_kernel");
  return 0;
}

// Verified payloads into the caller's segments (srd_scatter.hip): the gather's
// sequence with the segment append's table -- the table's upload, the layout,
// one wait for the error word, the unit total and the multi-unit count, then
// the unit table, the streaming kernel, the combine and the finish enqueued on
// the stream.  The streaming kernel's out is the 16-byte boundary at or below
// the lowest destination: every unit's destination is an offset from it.
extern "C" int srd_payload_scatter_device(srd_ctx* c, const uint8_t* d_file, uint64_t flen, const uint64_t* d_start,
                                          const uint64_t* d_end, uint64_t n, uint8_t* const* dst_ptrs,
                                          const uint64_t* dst_lens, uint64_t n_dst, const srd_segment* d_segs,
                                          uint64_t n_segs, const uint64_t* d_seg_first, uint32_t flags, uint8_t* d_status,
                                          uint32_t* d_crc_computed, void* stream) {
  if (!c || (n_dst && (!dst_ptrs || !dst_lens)) || (n_segs && !d_segs) ||
      (n && (!d_start || !d_end || !d_seg_first || !d_status || (flen && !d_file)))) {
    set_err("bad argument");
    return SRD_ERR_ARG;
  }
  if (flags) { set_err("bad argument: flags must be 0"); return SRD_ERR_ARG; }
  if (n >= (1ull << 31)) { set_err("too many queries in one batch"); return SRD_ERR_ARG; }
  if (n_segs >= (1ull << 31)) { set_err("too many segments in one batch"); return SRD_ERR_ARG; }
  if (n_dst >= (1ull << 32)) { set_err("too many destinations in one batch"); return SRD_ERR_ARG; }
  if (!n) return 0;
  std::vector<uint64_t> tab(2 * n_dst);
  uint64_t base = ~0ull;  // the lowest destination address
  const uintptr_t f0 = (uintptr_t)d_file, f1 = f0 + srd_padded_size(flen);
  for (uint64_t k = 0; k < n_dst; k++) {
    const uintptr_t p0 = (uintptr_t)dst_ptrs[k], len = (uintptr_t)dst_lens[k];
    if (len && !p0) { set_err("bad argument: destination " + std::to_string(k) + " is NULL"); return SRD_ERR_ARG; }
    // no destination may lie in what the store's kernels read (p0 + len may not be formed: it could wrap)
    if (len && d_file && p0 < f1 && (f0 <= p0 || f0 - p0 < len)) {
      set_err("destination " + std::to_string(k) + " overlaps the store");
      return SRD_ERR_ARG;
    }
    if (len) base = std::min<uint64_t>(base, p0);
    tab[2 * k] = p0;
    tab[2 * k + 1] = len;
  }
  base &= ~15ull;
  HIPCHK(hipSetDevice(c->device));
  hipStream_t s = stream_of(c, stream);
  TRY(ensure(c, B_GA_ST, n));
  TRY(ensure(c, B_GA_CHK, n * 8));
  TRY(ensure(c, B_GA_CRC, n * 4));
  TRY(ensure(c, B_GA_CNT, 64));
  TRY(ensure(c, B_SG_SRC, tab.size() * 8));
  TRY(ensure(c, B_SG_OFF, n_segs * 8));
  TRY(ensure(c, B_SG_UN, n_segs * 8));
  TRY(ensure(c, B_SG_UPRE, n_segs * 8));
  TRY(ensure(c, B_SG_ENT, n_segs * 4));
  TRY(ensure_scan(c, (const uint64_t*)nullptr, (uint64_t*)nullptr, std::max<uint64_t>(n_segs, 1)));
  ScatterArgs a{};
  a.n = n;
  a.n_segs = n_segs;
  a.eun = P<uint64_t>(c, B_GA_CHK);
  a.upre = P<uint64_t>(c, B_SG_UPRE);
  a.file = d_file;
  a.start = d_start;
  a.end = d_end;
  a.srcs = P<uint64_t>(c, B_SG_SRC);
  a.segs = d_segs;
  a.first = d_seg_first;
  a.soff = P<uint64_t>(c, B_SG_OFF);
  a.sun = P<uint64_t>(c, B_SG_UN);
  a.sent = P<uint32_t>(c, B_SG_ENT);
  a.dst0 = base;
  a.crc = P<uint32_t>(c, B_GA_CRC);
  a.flen = flen;
  a.n_dst = n_dst;
  a.st = P<uint8_t>(c, B_GA_ST);
  a.cnt = P<unsigned long long>(c, B_GA_CNT);
  a.o_status = d_status;
  a.o_crc = d_crc_computed;
  // (the table is the caller's for the call: the wait below comes before the return)
  if (!tab.empty()) HIPCHK(hipMemcpyAsync(P<void>(c, B_SG_SRC), tab.data(), tab.size() * 8, hipMemcpyHostToDevice, s));
  HIPCHK(hipMemsetAsync(a.cnt, 0, 8, s));
  HIPCHK(hipMemsetAsync(a.cnt + 1, 0xFF, 8, s));  // the error word: none
  if (n_segs) HIPCHK(hipMemsetAsync(a.sun, 0, n_segs * 8, s));  // (a malformed d_seg_first leaves segments unvisited)
  scatter_layout_kernel<<<grid_for(n), 256, 0, s>>>(a);
  LAUNCHED(s, "scatter_layout_kernel");
  // everything the host decides on, on one wait
  uint64_t units = 0;
  struct { unsigned long long n_multi, err; } h{};
  if (n_segs) TRY(scan_sum_total(c, (const uint64_t*)a.sun, a.upre, n_segs, s, &units, SmallRead{a.cnt, &h, sizeof h}));
  else TRY(read_small(c, s, {SmallRead{a.cnt, &h, sizeof h}}));  // (no query has a segment: NONE, BAD_RANGE or BAD_LENGTH)
  if (h.err != ~0ull) {
    const std::string i = std::to_string(h.err >> 8);
    set_err(append_err_status(h.err) == SEG_BAD_SEGMENT
                ? "query " + i + " has a malformed segment (src, reserved, or a range outside its destination)"
                : "d_seg_first is malformed at query " + i);
    return SRD_ERR_ARG;
  }
  if (units >= (1ull << 32)) { set_err("too many work units in one batch"); return SRD_ERR_ARG; }
  if (units) TRY(stream_units(c, s, a, units, h.n_multi, (uint8_t*)(uintptr_t)base, nullptr));
  scatter_finish_kernel<<<grid_for(n), 256, 0, s>>>(a);
  LAUNCHED(s, "scatter_finish_kernel");
  return 0;
}

// ---------------------------------------------------------------------------
// Entries appended to a store from bytes already in HBM: the device append
// (srd_append.hip; srd_compact_live_device runs it too) and the segment append
// (srd_segments.hip).  Two steps each: the plan runs the owner's layout kernel
// and exclusive sums and waits once for the error word, the new tail and the
// unit counts (nothing of the store is written); the commit enqueues the unit
// table, the streaming kernel, the combine and the finish.
struct AppendPlan {
  AppendArgs a;  // the layout's and the finish's arguments (file and mo: append_finish's)
  UnitArgs u;    // the batch cut into units: the append's ranges, the segment append's table
  uint64_t new_tail, units, n_multi;
};
struct PlanWords { unsigned long long n_multi, err, coarse, len_last; };  // a.cnt[0 .. 4) read back

// The workspace and arguments both layouts share, the counter words at their
// start values (n < 2^31: the caller's check; it fits hipCUB's int count)
static int plan_begin(Ctx* c, hipStream_t s, AppendPlan* p, uint64_t n, uint64_t tail, bool rule) {
  TRY(ensure(c, B_GA_PLEN, n * 8));
  TRY(ensure(c, B_GA_CHK, n * 8));
  TRY(ensure(c, B_GA_OFF, n * 8));
  TRY(ensure(c, B_GA_CRC, n * 4));
  TRY(ensure(c, B_GA_CNT, 64));
  if (rule) TRY(ensure(c, B_AP_NZ, n * 4));
  *p = AppendPlan{};
  AppendArgs& a = p->a;
  a.n = n;
  a.tail = tail;
  a.base = append_base(tail);
  a.slot = P<uint64_t>(c, B_GA_PLEN);
  a.chk = P<uint64_t>(c, B_GA_CHK);
  a.pre = P<uint64_t>(c, B_GA_OFF);
  a.cnt = P<unsigned long long>(c, B_GA_CNT);
  a.crc = P<uint32_t>(c, B_GA_CRC);
  a.nz = rule ? P<uint32_t>(c, B_AP_NZ) : nullptr;
  UnitArgs& u = p->u;  // (the layout's unit counts and prefix are what the unit kernels read)
  u.n = n;
  u.eun = a.chk;
  u.off = P<uint64_t>(c, B_GA_OFF);
  u.dst0 = a.base;
  u.crc = P<uint32_t>(c, B_GA_CRC);
  HIPCHK(hipMemsetAsync(a.cnt, 0, 40, s));
  HIPCHK(hipMemsetAsync(a.cnt + 1, 0xFF, 8, s));  // the error word: none
  if (rule) HIPCHK(hipMemsetAsync(P<void>(c, B_AP_NZ), 0, n * 4, s));
  return 0;
}
// ... and, once the owner has turned an error word into its message, what the
// host decides from the words read back: the new tail
static int plan_end(AppendPlan* p, const PlanWords& h, uint64_t pre_last) {
  if (!append_new_tail(p->a.tail, h.coarse, pre_last, h.len_last, &p->new_tail)) {
    set_err("the batch would end at 2^48 or beyond (the index packs 48-bit offsets)");
    return SRD_ERR_ARG;
  }
  p->n_multi = h.n_multi;
  return 0;
}
static int append_fits(uint64_t new_tail, uint64_t file_cap) {
  if (srd_padded_size(new_tail) <= file_cap) return 0;
  set_err("file_cap too small for the batch: it ends at " + std::to_string(new_tail));
  return SRD_ERR_ARG;
}
// per entry: the metadata, the prepad, the caller's metadata offsets, the stream rule's outcome
static int append_finish(hipStream_t s, AppendPlan* p, uint8_t* d_file, uint64_t* d_mo) {
  AppendArgs& a = p->a;
  a.file = d_file;
  a.mo = d_mo;
  append_finish_kernel<<<(unsigned)std::min<uint64_t>((a.n + 255) / 256, 4096), 256, 0, s>>>(a);
  LAUNCHED(s, "append_finish_kernel");
  return 0;
}
// write_stream's check comes after the bytes (data_store.rs:783-797)
static int append_null_only(unsigned long long null_only) {
  if (!null_only) return 0;
  set_err("NULL-byte-only streams cannot be written directly.");
  return SRD_ERR_ARG;
}
// the second wait: the rule's outcome is in a.cnt[4] once the stream has run
static int append_rule_wait(Ctx* c, hipStream_t s, const AppendPlan& p) {
  unsigned long long null_only = 0;
  TRY(read_small(c, s, {rd(p.a.cnt + 4, &null_only)}));
  return append_null_only(null_only);
}

// The append's plan: SRD_ERR_ARG with the refusal's message for what the
// entries themselves decide
static int append_plan(Ctx* c, hipStream_t s, const uint8_t* d_payloads, uint64_t payloads_len,
                       const uint64_t* d_src_off, const uint64_t* d_len, const uint64_t* d_key_hashes, uint64_t n,
                       bool rule, uint64_t tail, AppendPlan* p) {
  TRY(plan_begin(c, s, p, n, tail, rule));
  TRY(ensure(c, B_GA_CPRE, n * 8));
  TRY(ensure(c, B_AP_END, n * 8));
  TRY(ensure_scan(c, (const uint64_t*)nullptr, (uint64_t*)nullptr, n));  // both scans below
  AppendArgs& a = p->a;
  a.pay = d_payloads;
  a.pay_len = payloads_len;
  a.src = d_src_off;
  a.len = d_len;
  a.kh = d_key_hashes;
  a.end = P<uint64_t>(c, B_AP_END);
  UnitArgs& u = p->u;  // the payloads as ranges of the blob
  u.n_segs = n;
  u.upre = P<uint64_t>(c, B_GA_CPRE);
  u.file = d_payloads;
  u.start = d_src_off;
  u.end = a.end;
  append_layout_kernel<<<grid_for(n), 256, 0, s>>>(a);
  LAUNCHED(s, "append_layout_kernel");
  // everything the host decides on, on one wait
  uint64_t pre_last = 0;
  PlanWords h{};
  TRY(scan_sum(c, (const uint64_t*)a.slot, P<uint64_t>(c, B_GA_OFF), n, s));
  TRY(scan_sum_total(c, (const uint64_t*)a.chk, u.upre, n, s, &p->units, rd(a.pre + n - 1, &pre_last),
                     SmallRead{a.cnt, &h, sizeof h}));
  if (h.err != ~0ull) {
    const uint32_t st = append_err_status(h.err);
    set_err(st == APPEND_EMPTY       ? "Payload cannot be empty."
            : st == APPEND_NULL_BYTE ? "NULL-byte payloads cannot be written directly."
            : st == APPEND_BAD_RANGE ? "payload range " + std::to_string(h.err >> 8) + " does not lie inside d_payloads"
                                     : "the batch would end at 2^48 or beyond (the index packs 48-bit offsets)");
    return SRD_ERR_ARG;
  }
  return plan_end(p, h, pre_last);
}

// The planned batch written to d_file (file byte j at d_file[j], 16-byte
// aligned) and its metadata offsets to d_mo, enqueued on s; the one refusal
// left (too many units) comes before anything is written.
static int plan_commit(Ctx* c, hipStream_t s, AppendPlan* p, uint8_t* d_file, uint64_t* d_mo) {
  if (p->units >= (1ull << 32)) { set_err("too many work units in one batch"); return SRD_ERR_ARG; }
  TRY(stream_units(c, s, p->u, p->units, p->n_multi, d_file, const_cast<uint32_t*>(p->a.nz)));
  return append_finish(s, p, d_file, d_mo);
}

extern "C" int srd_batch_append_device(srd_ctx* c, const uint8_t* d_payloads, uint64_t payloads_len,
                                       const uint64_t* d_src_off, const uint64_t* d_len, const uint64_t* d_key_hashes,
                                       uint64_t n, uint32_t flags, uint64_t tail, uint8_t* d_file, uint64_t file_cap,
                                       uint64_t* new_tail, uint64_t* d_meta_off_out, void* stream) {
  if (!c || !new_tail || (flags & ~SRD_APPEND_STREAM_RULE) || ((uintptr_t)d_file & 15) ||
      (n && (!d_src_off || !d_len || !d_key_hashes || !d_file || !d_meta_off_out || (payloads_len && !d_payloads)))) {
    set_err("bad argument");
    return SRD_ERR_ARG;
  }
  *new_tail = tail;
  if (n >= (1ull << 31)) { set_err("too many entries in one batch"); return SRD_ERR_ARG; }
  if (!n) return 0;
  const bool rule = flags & SRD_APPEND_STREAM_RULE;
  HIPCHK(hipSetDevice(c->device));
  hipStream_t s = stream_of(c, stream);
  AppendPlan p{};
  TRY(append_plan(c, s, d_payloads, payloads_len, d_src_off, d_len, d_key_hashes, n, rule, tail, &p));
  const uint64_t nt = p.new_tail;
  TRY(append_fits(nt, file_cap));
  {  // the blob may not lie in what the call writes
    const uintptr_t p0 = (uintptr_t)d_payloads, p1 = p0 + payloads_len;
    const uintptr_t w0 = (uintptr_t)d_file + tail, w1 = (uintptr_t)d_file + gather_pad64(nt);
    if (payloads_len && p0 < w1 && w0 < p1) { set_err("d_payloads overlaps the bytes the batch writes"); return SRD_ERR_ARG; }
  }
  TRY(plan_commit(c, s, &p, d_file, d_meta_off_out));
  if (rule) TRY(append_rule_wait(c, s, p));
  *new_tail = nt;
  return 0;
}

// The segment append's plan: uploads the source table; the sums are the
// entries' slots and the segments' unit counts
static int segments_plan(Ctx* c, hipStream_t s, const std::vector<uint64_t>& srcs, const srd_segment* d_segs,
                         uint64_t n_segs, const uint64_t* d_seg_first, const uint64_t* d_key_hashes, uint64_t n,
                         uint64_t tail, AppendPlan* p) {
  TRY(plan_begin(c, s, p, n, tail, true));
  TRY(ensure(c, B_SG_SRC, srcs.size() * 8));
  TRY(ensure(c, B_SG_LEN, n * 8));
  TRY(ensure(c, B_SG_OFF, n_segs * 8));
  TRY(ensure(c, B_SG_UN, n_segs * 8));
  TRY(ensure(c, B_SG_UPRE, n_segs * 8));
  TRY(ensure(c, B_SG_ENT, n_segs * 4));
  TRY(ensure_scan(c, (const uint64_t*)nullptr, (uint64_t*)nullptr, std::max(n, n_segs)));  // both scans below
  AppendArgs& a = p->a;
  UnitArgs& u = p->u;
  u.n_segs = n_segs;
  u.upre = P<uint64_t>(c, B_SG_UPRE);
  u.srcs = P<uint64_t>(c, B_SG_SRC);
  u.segs = d_segs;
  u.first = d_seg_first;
  u.len = P<uint64_t>(c, B_SG_LEN);
  u.soff = P<uint64_t>(c, B_SG_OFF);
  u.sun = P<uint64_t>(c, B_SG_UN);
  u.sent = P<uint32_t>(c, B_SG_ENT);
  a.len = u.len;  // (the finish runs over the entries' total lengths)
  a.kh = d_key_hashes;
  // (the table is the caller's for the call: the wait below comes before the return)
  if (!srcs.empty()) HIPCHK(hipMemcpyAsync(P<void>(c, B_SG_SRC), srcs.data(), srcs.size() * 8, hipMemcpyHostToDevice, s));
  if (n_segs) HIPCHK(hipMemsetAsync(u.sun, 0, n_segs * 8, s));  // (a refused entry leaves its segments' counts alone)
  segments_layout_kernel<<<grid_for(n), 256, 0, s>>>(a, u, srcs.size() / 2);
  LAUNCHED(s, "segments_layout_kernel");
  // everything the host decides on, on one wait
  uint64_t pre_last = 0;
  PlanWords h{};
  if (n_segs) {
    TRY(scan_sum(c, (const uint64_t*)a.slot, P<uint64_t>(c, B_GA_OFF), n, s));
    TRY(scan_sum_total(c, (const uint64_t*)u.sun, u.upre, n_segs, s, &p->units,
                       rd(a.pre + n - 1, &pre_last), SmallRead{a.cnt, &h, sizeof h}));
  } else {
    TRY(read_small(c, s, {SmallRead{a.cnt, &h, sizeof h}}));  // (every entry is empty: refused below)
  }
  if (h.err != ~0ull) {
    const uint32_t st = append_err_status(h.err);
    const std::string i = std::to_string(h.err >> 8);
    set_err(st == APPEND_EMPTY      ? "Payload cannot be empty."
            : st == SEG_BAD_SEGMENT ? "entry " + i + " has a malformed segment (src, reserved, or a range outside its source)"
            : st == SEG_BAD_FIRST   ? "d_seg_first is malformed at entry " + i
                                    : "entry " + i + " is 2^48 bytes or longer (the index packs 48-bit offsets)");
    return SRD_ERR_ARG;
  }
  return plan_end(p, h, pre_last);
}

extern "C" int srd_batch_append_segments_device(srd_ctx* c, const uint8_t* const* src_ptrs, const uint64_t* src_lens,
                                                uint64_t n_src, const srd_segment* d_segs, uint64_t n_segs,
                                                const uint64_t* d_seg_first, const uint64_t* d_key_hashes, uint64_t n,
                                                uint32_t flags, uint64_t tail, uint8_t* d_file, uint64_t file_cap,
                                                uint64_t* new_tail, uint64_t* d_meta_off_out, void* stream) {
  if (!c || !new_tail || ((uintptr_t)d_file & 15) || (n_src && (!src_ptrs || !src_lens)) || (n_segs && !d_segs) ||
      (n && (!d_seg_first || !d_key_hashes || !d_file || !d_meta_off_out))) {
    set_err("bad argument");
    return SRD_ERR_ARG;
  }
  *new_tail = tail;
  if (flags) { set_err("bad argument: flags must be 0"); return SRD_ERR_ARG; }
  if (n >= (1ull << 31)) { set_err("too many entries in one batch"); return SRD_ERR_ARG; }
  if (n_segs >= (1ull << 31)) { set_err("too many segments in one batch"); return SRD_ERR_ARG; }
  if (n_src >= (1ull << 32)) { set_err("too many sources in one batch"); return SRD_ERR_ARG; }
  if (!n) return 0;
  std::vector<uint64_t> srcs(2 * n_src);
  for (uint64_t k = 0; k < n_src; k++) {
    if (src_lens[k] && !src_ptrs[k]) { set_err("bad argument: source " + std::to_string(k) + " is NULL"); return SRD_ERR_ARG; }
    srcs[2 * k] = (uint64_t)(uintptr_t)src_ptrs[k];
    srcs[2 * k + 1] = src_lens[k];
  }
  HIPCHK(hipSetDevice(c->device));
  hipStream_t s = stream_of(c, stream);
  AppendPlan p{};
  TRY(segments_plan(c, s, srcs, d_segs, n_segs, d_seg_first, d_key_hashes, n, tail, &p));
  const uint64_t nt = p.new_tail;
  TRY(append_fits(nt, file_cap));
  for (uint64_t k = 0; k < n_src; k++) {  // no source may lie in what the call writes
    const uintptr_t p0 = (uintptr_t)srcs[2 * k], len = (uintptr_t)srcs[2 * k + 1];
    const uintptr_t w0 = (uintptr_t)d_file + tail, w1 = (uintptr_t)d_file + gather_pad64(nt);
    if (len && p0 < w1 && (w0 < p0 || w0 - p0 < len)) {  // (p0 + len may not be formed: it could wrap)
      set_err("source " + std::to_string(k) + " overlaps the bytes the batch writes");
      return SRD_ERR_ARG;
    }
  }
  TRY(plan_commit(c, s, &p, d_file, d_meta_off_out));
  TRY(append_rule_wait(c, s, p));
  *new_tail = nt;
  return 0;
}

// ---------------------------------------------------------------------------
// A live session compacted (srd_index_live.hip's compact_* kernels around the
// append's path): the export's body and the iterator's
// into workspace, the append's plan (the new length), the refusals, then the
// append's commit, the CRC comparison with the pairs for the new table, the
// table build, and one wait for the outcome
static bool ranges_meet(const void* a, uint64_t an, const void* b, uint64_t bn) {
  const uintptr_t a0 = (uintptr_t)a, b0 = (uintptr_t)b;
  return a && b && an && bn && a0 < b0 + bn && b0 < a0 + an;
}

extern "C" int srd_compact_live_device(srd_ctx* c, const void* d_table, uint64_t table_bytes, const uint8_t* d_file,
                                       uint64_t file_len, uint8_t* d_out, uint64_t out_cap, void* d_new_table,
                                       uint64_t new_table_bytes, srd_compact_stats* stats) {
  if (stats) *stats = srd_compact_stats{0, 0, 0, 0, ~0ull};
  if (!c || !stats || !table_ok(d_table, table_bytes) || (file_len && !d_file) || (d_out && !d_new_table)) {
    set_err("bad argument");
    return SRD_ERR_ARG;
  }
  if (d_out) {  // what the arguments decide on their own, before anything runs
    if ((uintptr_t)d_out & 15) { set_err("d_out is not 16-byte aligned"); return SRD_ERR_ARG; }
    const uint64_t padded = srd_padded_size(file_len);
    if (ranges_meet(d_out, out_cap, d_file, padded) || ranges_meet(d_out, out_cap, d_table, table_bytes)) {
      set_err("d_out overlaps the store or its table");
      return SRD_ERR_ARG;
    }
    if (ranges_meet(d_new_table, new_table_bytes, d_file, padded) ||
        ranges_meet(d_new_table, new_table_bytes, d_table, table_bytes) ||
        ranges_meet(d_new_table, new_table_bytes, d_out, out_cap)) {
      set_err("d_new_table overlaps the store, its table or d_out");
      return SRD_ERR_ARG;
    }
  }
  HIPCHK(hipSetDevice(c->device));
  hipStream_t s = c->stream;
  // the live pairs in file order, then par_iter_entries' filter, newest first
  uint64_t nl = 0, nv = 0, kept = 0;
  uint64_t *xk = nullptr, *xp = nullptr;
  TRY(export_run(c, d_table, table_bytes, &xk, &xp, 0, true, &nl));
  if (nl) {
    TRY(ensure(c, B_IT_OST, nl * 8));
    TRY(ensure(c, B_IT_OEN, nl * 8));
    TRY(ensure(c, B_IT_OKH, nl * 8));
    TRY(iter_run(c, d_file, file_len, xp, nl, P<uint64_t>(c, B_IT_OST), P<uint64_t>(c, B_IT_OEN), nullptr,
                 P<uint64_t>(c, B_IT_OKH), &nv, &kept));
  }
  stats->n_entries = nv;
  stats->kept_bytes = kept;
  AppendPlan p{};
  const uint64_t* st = P<uint64_t>(c, B_IT_OST);
  const uint64_t* en = P<uint64_t>(c, B_IT_OEN);
  const uint64_t* kh = P<uint64_t>(c, B_IT_OKH);
  if (nv) {  // (nv <= nl < 2^31: the append's bound on n holds)
    TRY(ensure(c, B_CL_LEN, nv * 8));
    compact_lens_kernel<<<grid_for(nv), 256, 0, s>>>(st, en, nv, P<uint64_t>(c, B_CL_LEN));
    LAUNCHED(s, "compact_lens_kernel");
    TRY(append_plan(c, s, d_file, file_len, st, P<uint64_t>(c, B_CL_LEN), kh, nv, true, 0, &p));
    stats->new_len = p.new_tail;
  }
  if (!d_out) return 0;  // the planning call
  if (nv && srd_padded_size(stats->new_len) > out_cap) {
    set_err("out_cap too small for the compacted store: it ends at " + std::to_string(stats->new_len));
    return SRD_ERR_ARG;
  }
  if (new_table_bytes < srd_index_table_bytes(nv)) {
    set_err("new_table_bytes < srd_index_table_bytes(n_entries)");
    return SRD_ERR_ARG;
  }
  if (!nv) {  // no live entry: the empty table
    TRY(table_build_run(c, nullptr, nullptr, 0, d_new_table, new_table_bytes));
    HIPCHK(spin_sync(s));
    return 0;
  }
  TRY(ensure(c, B_CL_MO, nv * 8));
  TRY(ensure(c, B_CL_PACKED, nv * 8));
  TRY(ensure(c, B_CL_CNT, 64));
  unsigned long long* cnt = P<unsigned long long>(c, B_CL_CNT);
  TRY(plan_commit(c, s, &p, d_out, P<uint64_t>(c, B_CL_MO)));
  HIPCHK(hipMemsetAsync(cnt, 0, 8, s));
  HIPCHK(hipMemsetAsync(cnt + 1, 0xFF, 8, s));  // the first bad position: none
  compact_finish_kernel<<<grid_for(nv), 256, 0, s>>>(d_file, en, kh, p.a.crc, P<uint64_t>(c, B_CL_MO), nv,
                                                     P<uint64_t>(c, B_CL_PACKED), cnt);
  LAUNCHED(s, "compact_finish_kernel");
  TRY(table_build_run(c, kh, P<uint64_t>(c, B_CL_PACKED), nv, d_new_table, new_table_bytes));
  // the one wait behind the kernels: the stream rule's outcome and the CRC comparison's
  unsigned long long null_only = 0;
  struct { unsigned long long n_bad, first; } h{};
  TRY(read_small(c, s, {rd(p.a.cnt + 4, &null_only), SmallRead{cnt, &h, sizeof h}}));
  TRY(append_null_only(null_only));
  stats->n_crc_bad = h.n_bad;
  if (h.n_bad) TRY(read_small(c, s, {rd(en + h.first, &stats->first_bad)}));  // (a corrupt store only) its source metadata offset
  return 0;
}

// ---------------------------------------------------------------------------
// The TTL cache (srd_ttl.h, srd_ttl.hip): namespaced key
// hashes, the batched read's decision, eviction and the sweep
extern "C" int srd_namespace_hash_batch_device(srd_ctx* c, uint64_t prefix_hash, const uint8_t* d_keys,
                                               const uint64_t* d_offs, const uint64_t* d_lens, uint64_t n,
                                               uint8_t* d_ns_out, uint64_t* d_hash_out, void* stream) {
  if (!c || ((uintptr_t)d_ns_out & 7) || (n && (!d_keys || !d_offs || !d_lens || !d_hash_out))) {
    set_err("bad argument");
    return SRD_ERR_ARG;
  }
  if (!n) return 0;
  HIPCHK(hipSetDevice(c->device));
  hipStream_t s = stream_of(c, stream);
  ns_hash_kernel<<<blocks(n, 256), 256, 0, s>>>(NsKeys{d_keys, d_offs, d_lens, prefix_hash}, n, (uint64_t*)d_ns_out,
                                                d_hash_out);
  LAUNCHED(s, "ns_hash_kernel");
  return 0;
}

extern "C" int srd_namespace_hash_batch(srd_ctx* c, uint64_t prefix_hash, const uint8_t* keys, uint64_t klen,
                                        const uint64_t* offs, const uint64_t* lens, uint64_t n, uint8_t* ns_out,
                                        uint64_t* hash_out) {
  if (!c || (n && (!offs || !lens || !hash_out))) { set_err("bad argument"); return SRD_ERR_ARG; }
  DevTmp dns;  // (released behind batch_host's wait)
  if (ns_out && n && dns.alloc(16 * n) != hipSuccess) { set_err("hipMalloc failed"); return SRD_ERR_ALLOC; }
  return batch_host<uint64_t>(c, keys, klen, offs, lens, n, hash_out, [&](auto db, auto dof, auto dl, auto dout) {
    TRY(srd_namespace_hash_batch_device(c, prefix_hash, db, dof, dl, n, (uint8_t*)dns.p, dout, nullptr));
    if (dns.p) HIPCHK(hipMemcpyAsync(ns_out, dns.p, 16 * n, hipMemcpyDeviceToHost, c->stream));
    return 0;
  });
}

// One lane per query or pair, in strides over a grid that fills the machine
// exactly once -- the blocks of 256 the kernel's registers let a CU hold, asked
// of the runtime once per kernel -- so that no second, partial round of blocks
// trails the first and the counts cost one set of atomics per resident block
template <auto Kernel>
static unsigned ttl_grid(Ctx* c, uint64_t n) {
  static const int per_cu = [] {
    int b = 0;
    return hipOccupancyMaxActiveBlocksPerMultiprocessor(&b, Kernel, 256, 0) == hipSuccess && b > 0 ? b : 8;
  }();
  return std::min(grid_for(n), c->scan_cus * (unsigned)per_cu);
}

static int ttl_resolve_run(srd_ctx* c, const void* d_table, uint64_t table_bytes, const uint8_t* d_file, uint64_t flen,
                           const uint64_t* d_hashes, const NsKeys* keys, uint64_t* d_hashes_out, uint64_t n,
                           uint64_t now, uint64_t* d_start, uint64_t* d_end, uint64_t* d_expiry, uint8_t* d_status,
                           uint64_t* d_counts, void* stream) {
  const bool ins = keys ? keys->keys && keys->offs && keys->lens && d_hashes_out : d_hashes != nullptr;
  if (!c || !table_ok(d_table, table_bytes) || (n && (!ins || !d_start || !d_end || !d_status || (flen && !d_file)))) {
    set_err("bad argument");
    return SRD_ERR_ARG;
  }
  HIPCHK(hipSetDevice(c->device));
  hipStream_t s = stream_of(c, stream);
  if (d_counts) HIPCHK(hipMemsetAsync(d_counts, 0, 32, s));
  if (!n) return 0;
  TtlResolveArgs a{};
  a.t = table_view(d_table, table_bytes);
  a.file = d_file;
  a.flen = flen;
  a.q = d_hashes;
  if (keys) a.k = *keys;
  a.q_out = d_hashes_out;
  a.n = n;
  a.now = now;
  a.start = d_start;
  a.end = d_end;
  a.expiry = d_expiry;
  a.status = d_status;
  a.cnt = (unsigned long long*)d_counts;
  if (keys)
    ttl_resolve_kernel<true><<<ttl_grid<ttl_resolve_kernel<true>>(c, n), 256, 0, s>>>(a);
  else
    ttl_resolve_kernel<false><<<ttl_grid<ttl_resolve_kernel<false>>(c, n), 256, 0, s>>>(a);
  LAUNCHED(s, "ttl_resolve_kernel");
  return 0;
}

extern "C" int srd_ttl_resolve_device(srd_ctx* c, const void* d_table, uint64_t table_bytes, const uint8_t* d_file,
                                      uint64_t file_len, const uint64_t* d_hashes, uint64_t n, uint64_t now,
                                      uint64_t* d_start, uint64_t* d_end, uint64_t* d_expiry, uint8_t* d_status,
                                      uint64_t* d_counts, void* stream) {
  return ttl_resolve_run(c, d_table, table_bytes, d_file, file_len, d_hashes, nullptr, nullptr, n, now, d_start, d_end,
                         d_expiry, d_status, d_counts, stream);
}

extern "C" int srd_ttl_resolve_keys_device(srd_ctx* c, const void* d_table, uint64_t table_bytes, const uint8_t* d_file,
                                           uint64_t file_len, uint64_t prefix_hash, const uint8_t* d_keys,
                                           const uint64_t* d_offs, const uint64_t* d_lens, uint64_t n, uint64_t now,
                                           uint64_t* d_hashes_out, uint64_t* d_start, uint64_t* d_end,
                                           uint64_t* d_expiry, uint8_t* d_status, uint64_t* d_counts, void* stream) {
  const NsKeys k{d_keys, d_offs, d_lens, prefix_hash};
  return ttl_resolve_run(c, d_table, table_bytes, d_file, file_len, nullptr, &k, d_hashes_out, n, now, d_start, d_end,
                         d_expiry, d_status, d_counts, stream);
}

extern "C" int srd_ttl_evict_device(srd_ctx* c, void* d_table, uint64_t table_bytes, uint64_t* used,
                                    const uint64_t* d_hashes, const uint8_t* d_status, uint64_t n, uint64_t tail,
                                    uint8_t* d_file, uint64_t file_cap, uint64_t* new_tail, uint64_t* n_evicted) {
  if (!c || !table_ok(d_table, table_bytes) || !used || !new_tail || n >= (1ull << 31) ||
      (n && (!d_hashes || !d_status || !d_file))) {
    set_err("bad argument");
    return SRD_ERR_ARG;
  }
  *new_tail = tail;
  if (n_evicted) *n_evicted = 0;
  if (!n) return 0;
  HIPCHK(hipSetDevice(c->device));
  hipStream_t s = c->stream;
  // the expired queries' hashes, packed in batch order
  TRY(ensure(c, B_LV_FLAG, n * 4));
  TRY(ensure(c, B_LV_POS, n * 4));
  uint32_t* flag = P<uint32_t>(c, B_LV_FLAG);
  uint32_t* pos = P<uint32_t>(c, B_LV_POS);
  TRY(ensure_scan(c, flag, pos, n));
  ttl_candidates_kernel<<<grid_for(n), 256, 0, s>>>(d_status, n, flag);
  LAUNCHED(s, "ttl_candidates_kernel");
  uint64_t m = 0;
  TRY(scan_sum_total(c, flag, pos, n, s, &m));
  if (!m) return 0;
  TRY(ensure(c, B_TT_XQ, m * 8));
  uint64_t* xq = P<uint64_t>(c, B_TT_XQ);
  ttl_pack_kernel<<<grid_for(n), 256, 0, s>>>(d_hashes, flag, pos, n, xq);
  LAUNCHED(s, "ttl_pack_kernel");
  // one tombstone per distinct key among them, at the key's last occurrence:
  // the apply's dedupe over the packed hashes (the table is not touched)
  uint32_t log2dc = 6;
  while ((1ull << log2dc) < 2 * m) log2dc++;
  const uint64_t dc = 1ull << log2dc;
  TRY(ensure(c, B_LV_DSLOT, dc * 4));
  TRY(ensure(c, B_LV_LSLOT, m * 4));
  TRY(ensure(c, B_TT_FLAG, m * 4));
  TRY(ensure(c, B_TT_POS, m * 4));
  LiveArgs a{};
  a.kh = xq;
  a.n = m;
  a.dslot = P<uint32_t>(c, B_LV_DSLOT);
  a.log2dc = log2dc;
  a.lslot = P<uint32_t>(c, B_LV_LSLOT);
  uint32_t* keep = P<uint32_t>(c, B_TT_FLAG);
  uint32_t* kpos = P<uint32_t>(c, B_TT_POS);
  TRY(ensure_scan(c, keep, kpos, m));
  HIPCHK(hipMemsetAsync(a.dslot, 0, dc * 4, s));
  live_dedupe_kernel<<<grid_for(m), 256, 0, s>>>(a);
  LAUNCHED(s, "live_dedupe_kernel");
  ttl_keep_kernel<<<grid_for(m), 256, 0, s>>>(a.dslot, a.lslot, m, keep);
  LAUNCHED(s, "ttl_keep_kernel");
  uint64_t nk = 0;
  TRY(scan_sum_total(c, keep, kpos, m, s, &nk));
  TRY(tombs_commit(c, d_table, table_bytes, used, xq, keep, kpos, m, nk, tail, d_file, file_cap, new_tail));
  if (n_evicted) *n_evicted = nk;
  return 0;
}

extern "C" int srd_ttl_sweep_device(srd_ctx* c, void* d_table, uint64_t table_bytes, uint64_t* used, uint8_t* d_file,
                                    uint64_t tail, uint64_t file_cap, uint64_t now, uint32_t flags, uint64_t* new_tail,
                                    srd_ttl_sweep_stats* stats) {
  if (stats) *stats = srd_ttl_sweep_stats{0, 0, 0, ~0ull};
  if (!c || !table_ok(d_table, table_bytes) || !used || !new_tail || !stats || (flags & ~SRD_TTL_SWEEP_PLAN) ||
      (tail && !d_file)) {
    set_err("bad argument");
    return SRD_ERR_ARG;
  }
  *new_tail = tail;
  HIPCHK(hipSetDevice(c->device));
  hipStream_t s = c->stream;
  // the live pairs in ascending metadata offset (workspace)
  uint64_t nl = 0;
  uint64_t *xk = nullptr, *xp = nullptr;
  TRY(export_run(c, d_table, table_bytes, &xk, &xp, 0, true, &nl));
  stats->n_judged = nl;
  if (!nl) return 0;
  TRY(ensure(c, B_LV_FLAG, nl * 4));
  TRY(ensure(c, B_LV_POS, nl * 4));
  TRY(ensure(c, B_TT_CNT, 64));
  uint32_t* flag = P<uint32_t>(c, B_LV_FLAG);
  uint32_t* pos = P<uint32_t>(c, B_LV_POS);
  unsigned long long* cnt = P<unsigned long long>(c, B_TT_CNT);
  TRY(ensure_scan(c, flag, pos, nl));
  HIPCHK(hipMemsetAsync(cnt, 0, 16, s));
  HIPCHK(hipMemsetAsync(cnt + 2, 0xFF, 8, s));  // the smallest surviving expiry: none
  ttl_sweep_kernel<<<ttl_grid<ttl_sweep_kernel>(c, nl), 256, 0, s>>>(d_file, tail, xp, nl, now, flag, cnt);
  LAUNCHED(s, "ttl_sweep_kernel");
  struct { unsigned long long expired, too_short, next; } h{};
  uint64_t nk = 0;
  TRY(scan_sum_total(c, flag, pos, nl, s, &nk, SmallRead{cnt, &h, sizeof h}));
  if (nk != h.expired) { set_err("internal: the sweep's flags and its count differ"); return SRD_ERR_INTERNAL; }
  stats->n_expired = h.expired;
  stats->n_short = h.too_short;
  stats->next_expiry = h.next;
  if ((flags & SRD_TTL_SWEEP_PLAN) || !nk) return 0;
  // the flagged keys are distinct (a table's) and in ascending metadata offset already
  return tombs_commit(c, d_table, table_bytes, used, xk, flag, pos, nl, nk, tail, d_file, file_cap, new_tail);
}

// ---------------------------------------------------------------------------
// Keyed reads into fixed-size rows (srd_rows.hip): the
// look-up, the layout, the unit prefix, the unit kernels in their device-count
// forms and the finish enqueued on the stream -- no count comes back to the
// host.  Grids and workspace are sized from the bound on the units
// (srd_rows.h); the workspace is the entry's own (B_RW_*), so a captured call
// stays valid whatever the context's other entries grow.
struct RowsBuf {
  BufId id;
  uint64_t bytes;
};
struct RowsWork {
  uint64_t bound, per_row;
  size_t scan_tmp;
  RowsBuf need[11];
};
// (n < 2^31 and a bound below 2^32: rows_refusal's, or the reserve's own check)
static int rows_work(uint64_t n, uint64_t row_cap, RowsWork* w) {
  w->per_row = rows_units_per_row(row_cap);
  w->bound = n * w->per_row;
  w->scan_tmp = 0;
  HIPCHK(hipcub::DeviceScan::ExclusiveSum(nullptr, w->scan_tmp, (const uint64_t*)nullptr, (uint64_t*)nullptr, n + 1));
  const RowsBuf need[11] = {
      {B_RW_START, rows_ws_u64(n)}, {B_RW_END, rows_ws_u64(n)},  {B_RW_EUN, rows_ws_u64(n)},
      {B_RW_OFF, rows_ws_u64(n)},   {B_RW_UPRE, rows_ws_u64(n)}, {B_RW_CRC, rows_ws_u32(n)},
      {B_RW_ST, rows_ws_u8(n)},     {B_RW_CNT, 64},              {B_RW_UNIT, rows_ws_units(w->bound)},
      {B_RW_RAW, rows_ws_raw(w->bound)}, {B_RW_TMP, w->scan_tmp + 256}};
  for (int k = 0; k < 11; k++) w->need[k] = need[k];
  return 0;
}
static bool rows_work_ready(Ctx* c, const RowsWork& w) {
  for (const auto& x : w.need)
    if (!c->bufs[x.id].p || c->bufs[x.id].n < x.bytes) return false;
  return true;
}
static int rows_work_grow(Ctx* c, const RowsWork& w) {
  for (const auto& x : w.need) TRY(ensure(c, x.id, x.bytes));
  (void)ttl_grid<rows_layout_kernel>(c, 1);  // (the runtime's occupancy answers: asked once, outside any capture)
  (void)ttl_grid<rows_finish_kernel>(c, 1);
  return 0;
}

extern "C" int srd_ctx_reserve_rows(srd_ctx* c, uint64_t n, uint64_t row_cap) {
  uint64_t bound = 0;
  if (!c || n >= (1ull << 31) || !rows_units_bound(n, row_cap, &bound) || bound >= (1ull << 32)) {
    set_err("bad argument (n >= 2^31, or n * ceil(row_cap / SRD_GATHER_CHUNK) >= 2^32?)");
    return SRD_ERR_ARG;
  }
  HIPCHK(hipSetDevice(c->device));
  RowsWork w;
  TRY(rows_work(n, row_cap, &w));
  if (rows_work_ready(c, w)) return 0;
  // a buffer that is replaced may still be read by work on some stream
  HIPCHK(hipDeviceSynchronize());
  return rows_work_grow(c, w);
}

extern "C" int srd_read_rows_device(srd_ctx* c, const void* d_table, uint64_t table_bytes, const uint8_t* d_file,
                                    uint64_t file_len, const uint64_t* d_hashes, const uint64_t* d_verify_hashes,
                                    uint64_t n, uint8_t* d_out, uint64_t row_stride, uint64_t row_cap, uint64_t* d_len,
                                    uint8_t* d_status, uint32_t* d_crc_computed, uint64_t* d_counts, uint32_t flags,
                                    void* stream) {
  if (!c) { set_err("bad argument"); return SRD_ERR_ARG; }
  RowsCall rc{};
  rc.file = (uint64_t)(uintptr_t)d_file;
  rc.file_padded = d_file ? srd_padded_size(file_len) : 0;
  rc.out = (uint64_t)(uintptr_t)d_out;
  rc.n = n;
  rc.row_stride = row_stride;
  rc.row_cap = row_cap;
  rc.flags = flags;
  rc.ptrs = table_ok(d_table, table_bytes) && d_hashes && d_out && d_len && d_status && (d_file || !file_len);
  if (const char* why = rows_refusal(rc)) { set_err(why); return SRD_ERR_ARG; }
  if (!n) return 0;
  HIPCHK(hipSetDevice(c->device));
  hipStream_t s = stream_of(c, stream);
  RowsWork w;
  TRY(rows_work(n, row_cap, &w));
  if (!rows_work_ready(c, w)) {
    hipStreamCaptureStatus cap = hipStreamCaptureStatusNone;
    HIPCHK(hipStreamIsCapturing(s, &cap));
    if (cap != hipStreamCaptureStatusNone) {
      set_err("the workspace for (n, row_cap) = (" + std::to_string(n) + ", " + std::to_string(row_cap) +
              ") is not there and cannot grow while the stream is capturing: call srd_ctx_reserve_rows first");
      return SRD_ERR_ARG;
    }
    TRY(rows_work_grow(c, w));
  }
  RowsArgs a{};
  a.n = a.n_segs = n;
  a.eun = P<uint64_t>(c, B_RW_EUN);
  a.off = P<uint64_t>(c, B_RW_OFF);
  a.upre = P<uint64_t>(c, B_RW_UPRE);
  a.file = d_file;
  a.start = a.o_start = P<uint64_t>(c, B_RW_START);
  a.end = a.o_end = P<uint64_t>(c, B_RW_END);
  a.unit = P<SegUnit>(c, B_RW_UNIT);
  a.n_units = w.bound;
  a.raw = P<uint32_t>(c, B_RW_RAW);
  a.crc = P<uint32_t>(c, B_RW_CRC);
  a.d_n_units = a.upre + n;
  a.cnt = P<unsigned long long>(c, B_RW_CNT);
  a.d_n_multi = a.cnt;
  a.t = table_view(d_table, table_bytes);
  a.flen = file_len;
  a.q = d_hashes;
  a.verify = d_verify_hashes;
  a.row_stride = row_stride;
  a.row_cap = row_cap;
  a.st = P<uint8_t>(c, B_RW_ST);
  a.o_len = d_len;
  a.o_status = d_status;
  a.o_crc = d_crc_computed;
  a.o_counts = (unsigned long long*)d_counts;
  rows_begin_kernel<<<1, 64, 0, s>>>(a.cnt, a.o_counts);
  LAUNCHED(s, "rows_begin_kernel");
  rows_layout_kernel<<<ttl_grid<rows_layout_kernel>(c, n + 1), 256, 0, s>>>(a);
  LAUNCHED(s, "rows_layout_kernel");
  size_t tb = c->bufs[B_RW_TMP].n;
  HIPCHK(hipcub::DeviceScan::ExclusiveSum(P<void>(c, B_RW_TMP), tb, (const uint64_t*)a.eun, a.upre, n + 1, s));
  LAUNCHED(s, "hipcub");
  units_kernel<RangeView, true><<<grid_for(w.bound), 256, 0, s>>>(a);
  LAUNCHED(s, "units_kernel");
  const unsigned g = (unsigned)std::min<uint64_t>((w.bound + SCAN_WAVES_V2 - 1) / SCAN_WAVES_V2, c->scan_blocks);
  stream_copy_crc_kernel<false, true><<<g, SCAN_WAVES_V2 * 64, 0, s>>>(
      StreamArgs{a.unit, w.bound, d_out, a.raw, a.crc, nullptr, a.d_n_units});
  LAUNCHED(s, "stream_copy_crc_kernel");
  if (w.per_row > 1) {  // (a row of one chunk at most has no multi-unit entry: known by arithmetic)
    unit_terms_kernel<RangeView, true><<<grid_for(w.bound), 256, 0, s>>>(a);
    LAUNCHED(s, "unit_terms_kernel");
    unit_combine_kernel<RangeView, true><<<(unsigned)std::min<uint64_t>((n + 3) / 4, 4096), 256, 0, s>>>(a);
    LAUNCHED(s, "unit_combine_kernel");
  }
  rows_finish_kernel<<<ttl_grid<rows_finish_kernel>(c, n), 256, 0, s>>>(a);
  LAUNCHED(s, "rows_finish_kernel");
  return 0;
}
