/*
 * srd_amd.h -- C ABI of the MI355X-native open-time hot path of SIMD R Drive
 * (jzombie/rust-simd-r-drive v0.16.3-alpha): validation-chain recovery,
 * per-payload IEEE CRC-32 check, and the latest-wins key-index rebuild,
 * plus the batch digest entry points.
 *
 * Plain pointers and sizes only (no torch / HIP types).  `stream` arguments
 * are `hipStream_t` passed as `void*` (NULL = the context's own stream).
 *
 * Each entry point names the reference interface it replaces
 * (paths relative to the reference repo root):
 *
 *   srd_recover_valid_chain   <- DataStore::recover_valid_chain
 *                                src/storage_engine/data_store.rs:383-482
 *   srd_key_indexer_build     <- KeyIndexer::build
 *                                src/storage_engine/key_indexer.rs:98-124
 *   srd_validate_index(_device) <- the two calls inside DataStore::open
 *                                (data_store.rs:89 and :108) fused with
 *                                EntryHandle::is_valid_checksum
 *                                (simd-r-drive-entry-handle/src/entry_handle.rs:260-275)
 *                                over every chain entry
 *   srd_crc32_batch(_device)  <- compute_checksum
 *                                src/storage_engine/digest/compute_checksum.rs:15-20
 *   srd_xxh3_64_batch(_device) <- compute_hash_batch
 *                                src/storage_engine/digest/compute_hash.rs:64-77
 *   srd_xxh3_64               <- compute_hash  (compute_hash.rs:25-27)
 *   srd_compact_live_device   <- DataStore::compact
 *                                src/storage_engine/data_store.rs:706-749
 *                                over a live session's store and index
 *
 * Semantics (bit-exact with the reference):
 *   - final_len = largest tail t <= file_len whose backward chain is
 *     structurally valid down to offset 0 (0 if none), exactly as the
 *     reference's byte-wise outer loop finds it.
 *   - chain = entries of the chain ending at final_len, in file order.
 *   - crc_computed = IEEE CRC-32 (crc32fast) of each chain payload;
 *     crc_ok = (crc_computed == stored little-endian checksum).
 *   - index = key_hash -> pack(tag16 = key_hash >> 48, meta_off48), latest
 *     entry per key_hash wins, tombstones INCLUDED (as KeyIndexer::build).
 * Errors: 0 = ok; negative = HIP / allocation / argument error
 * (srd_last_error() has the message).  Invalid chains and bad CRCs are
 * data, never errors.  Arithmetic on offsets wraps like release-mode Rust.
 */
#ifndef SRD_AMD_H
#define SRD_AMD_H
#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define SRD_OK 0
#define SRD_ERR_HIP (-1)
#define SRD_ERR_ALLOC (-2)
#define SRD_ERR_ARG (-3)
#define SRD_ERR_INTERNAL (-4)

/* srd_device_result.mode */
#define SRD_MODE_OPTIMISTIC 0      /* the chain was proven through recorded nodes from the largest tail
                                      within 256 B of file_len that passes recover_valid_chain's first
                                      test (file_len for an intact store, below it for a short torn tail) */
#define SRD_MODE_FULL 1            /* full pass (torn tail / corrupt store / unusual structure) */
#define SRD_MODE_SPAN_UNPROVEN 3   /* span mode: the shard's chain was not proven; use the whole-file path */

/* srd_device_result.full_reason: why the optimistic pass left the call to
 * the full pass (mode SRD_MODE_FULL) or left a span unproven
 * (SRD_MODE_SPAN_UNPROVEN); SRD_FULL_NONE when it decided.  The full pass
 * costs ~1.8x the optimistic one, so a store that always lands here (e.g. one
 * above ~1 TiB: SRD_FULL_SLOT_SPACE) is visible instead of silently slower. */
#define SRD_FULL_NONE 0
#define SRD_FULL_FORCED 1     /* SRD_FLAG_FORCE_FULL */
#define SRD_FULL_SLOT_SPACE 2 /* scan waves x candidate slots per wave >= the glue's 31-bit slot space */
#define SRD_FULL_WAVES 3      /* more scan waves per chain block than the shape check's bound */
#define SRD_FULL_NO_START 4   /* no strong node or root at the start tail (find_top): torn / corrupt end */
#define SRD_FULL_UNPROVEN 5   /* the recorded nodes do not prove one chain (shape / root count) */
#define SRD_FULL_CAP 6        /* the candidate slots per span could not grow further */
#define SRD_FULL_LOOKBACK 7   /* the fused shape check's decoupled look-back timed out (a chain block
                                 waited too long for a lower one): nothing it computed is used */

/* option flags */
#define SRD_FLAG_FORCE_FULL 1u   /* skip the optimistic (strong-candidate) pass */
#define SRD_FLAG_NO_CRC 2u       /* structural recovery + index only */
/* host-input staging (srd_validate_index / _multi).  Default: pinned input is
 * copied directly; any other memory (the mmap) goes through double-buffered
 * pinned bounce buffers that host threads fill (taking the mapping's page
 * faults on several cores) while the previous chunks DMA -- measured at the
 * pinned-buffer rate on MI355X (end to end). */
#define SRD_FLAG_STAGE_PAGEABLE 4u /* one pageable hipMemcpy (measurement baseline) */
#define SRD_FLAG_STAGE_REGISTER 8u /* hipHostRegister the range (read-only) for one DMA copy;
                                      bounce buffers when registration is refused */

typedef struct srd_ctx srd_ctx; /* one device + stream + reusable workspace */

int srd_ctx_create(int device, srd_ctx **out);
void srd_ctx_destroy(srd_ctx *ctx);
/* The HIP stream the context launches on (hipStream_t as void*). */
void *srd_ctx_stream(srd_ctx *ctx);
/* Device bytes the context holds now: its workspace buffers (candidate
 * records, per-slot glue words, result arrays, index buckets, ...) plus its
 * staging copy of a host store, if any.  The optimistic pass sizes its
 * per-slot arrays by slot space (~S / 2048 slots of ~160 B for an S-byte
 * store at the default 8 slots per 16 KiB span: DESIGN.md section 3). */
uint64_t srd_ctx_device_bytes(srd_ctx *ctx);
/* The tile-load pattern of the context's last optimistic scan: 0 coalesced
 * loads + in-register transpose, 1 line per lane (the pass measures both on
 * each new store and keeps the faster: DESIGN.md section 4.1); -1 before any. */
int srd_ctx_scan_loads(srd_ctx *ctx);
/* The load-pattern trial of the current store: ms[0] / ms[1] = the fastest
 * device-timed optimistic scan with coalesced / line-per-lane loads so far (0
 * if not measured); returns the choice (0, 1) or -1 while still measuring
 * (or pinned by SRD_SCAN_LOADS, or with XCD-aware shares off). */
int srd_ctx_scan_trial(srd_ctx *ctx, double *ms);
/* Diagnostics: the optimistic scan's block partition, installed and read back.
 * The scan's block b of n_blocks takes the resident spans [starts[b],
 * starts[b + 1]) (16 KiB spans, relative to the first resident one).  Without
 * a table that is the even split b * n_spans / n_blocks; with XCD-aware block
 * shares (the default; SRD_XPART=0 at srd_ctx_create turns them off) every
 * call measures its blocks and prepares the table of the next call on a store
 * of the same resident span count and grid.
 *
 * srd_ctx_set_scan_blocks installs starts[0..n_blocks] as the table of the
 * next optimistic scan, for that scan only (the scan prepares its successor's
 * table as always); like a measured table it is ignored if that scan's
 * resident span count or grid differ.  A valid table has 1 <= n_blocks <=
 * 1024, starts[0] == 0, starts[n_blocks] == n_spans, non-decreasing starts
 * (empty blocks are allowed anywhere) and no block larger than
 * (5 n_spans + 4 n_blocks - 1) / (4 n_blocks) + 1 spans, the size the pass's
 * workspace is laid out for.  Anything else, or a context with the shares off:
 * SRD_ERR_ARG, nothing changed.
 *
 * srd_ctx_scan_blocks reads back SRD_SCAN_BLOCKS_LAST, the partition the
 * last optimistic scan ran with (of a call that retried: its last attempt's;
 * info->attempts counts that call's scans, info->first_source tells what the
 * first one ran with), or SRD_SCAN_BLOCKS_NEXT, the table prepared for the
 * next one.  info->source says where the starts come from; up to cap of the
 * n_blocks + 1 starts are copied to starts.  info->n_blocks == 0: none (no
 * scan yet / no table prepared).  Both entries wait for the context's stream. */
#define SRD_SCAN_BLOCKS_LAST 0
#define SRD_SCAN_BLOCKS_NEXT 1
#define SRD_SCAN_BLOCKS_EVEN 0      /* source: no table, the even split */
#define SRD_SCAN_BLOCKS_MEASURED 1  /* the table the previous scan's durations gave */
#define SRD_SCAN_BLOCKS_INSTALLED 2 /* srd_ctx_set_scan_blocks */
typedef struct {
  uint64_t n_spans;
  uint32_t n_blocks;
  uint32_t source;
  uint32_t attempts;
  uint32_t first_source;
} srd_scan_blocks_info;
int srd_ctx_set_scan_blocks(srd_ctx *ctx, const uint64_t *starts,
                            uint32_t n_blocks, uint64_t n_spans);
int srd_ctx_scan_blocks(srd_ctx *ctx, int which, uint64_t *starts,
                        uint32_t cap, srd_scan_blocks_info *info);
const char *srd_last_error(void);
/* The sha256 of the sources this library was compiled from (every .hip / .h /
 * .cpp file under csrc/ and include/srd_amd.h, as computed by
 * rust-simd-r-drive_amd/src_hash.py, which is not itself hashed), 64 hex digits;
 * the Python mirror refuses a library whose hash differs from the sources
 * beside it, and bench.py / smoke print it. */
const char *srd_build_info(void);
/* HIP-event timing of the validate calls on ctx: SRD_TIMING_NONE (the
 * default), SRD_TIMING_SCAN (the streaming scan's launches: events stamped by
 * the scan dispatch itself, hipExtLaunchKernel -- bench.py's roofline),
 * SRD_TIMING_CALL (+ marker events around the whole call, ~10 us each).  Not
 * part of the reference interface. */
#define SRD_TIMING_NONE 0
#define SRD_TIMING_SCAN 1
#define SRD_TIMING_CALL 2
int srd_ctx_set_timing(srd_ctx *ctx, int level);
/* With SRD_TIMING_SCAN: stamp only every n-th scan launch (n >= 1; 1 = every
 * launch, the default).  The event-stamped launch costs ~7 us more wall time
 * than a plain one; a systematic sample keeps that off most calls. */
int srd_ctx_set_timing_every(srd_ctx *ctx, int n);

/* HIP-event timings on the context stream: the summed duration (ms) and the
 * count of the streaming scan kernel launches of every validate call since the
 * previous srd_ctx_timings call (the scans' event pairs are read out here, not
 * inside the calls), and the device span of the last call (0 unless the
 * timing level includes them). */
int srd_ctx_timings(srd_ctx *ctx, double *scan_ms, int *scan_launches,
                    double *total_ms);
/* The individual scan durations (ms) summed by the last srd_ctx_timings
 * read, in launch order: copies up to cap of them to out and returns how
 * many there were (< 0: error). */
int srd_ctx_scan_list(srd_ctx *ctx, float *out, int cap);

/* Result of one validate+index pass whose arrays live in DEVICE memory owned
 * by the context (valid until the next call on the same ctx). */
typedef struct {
  uint64_t file_len;
  uint64_t final_len;      /* recover_valid_chain */
  uint64_t n_chain;        /* entries on the chain ending at final_len */
  uint64_t n_index;        /* KeyIndexer entries */
  uint64_t n_crc_bad;      /* chain entries whose CRC does not match */
  uint64_t n_candidates;   /* chain-node candidates recorded by the scan */
  uint64_t full_reason;    /* SRD_FULL_*: why the optimistic pass did not decide (0 when it did) */
  uint32_t mode;           /* 0 = optimistic pass sufficed, 1 = full pass */
  uint32_t reserved;       /* host results: 1 = arrays owned by the context */
  /* chain, file order; device pointers */
  uint64_t *meta_off, *key_hash, *prev_offset, *payload_start, *payload_len;
  uint32_t *crc_stored, *crc_computed;
  uint8_t *crc_ok;
  /* index (chain order of the latest entry per key); device pointers */
  uint64_t *index_key_hash, *index_packed;
} srd_device_result;

/* Bytes the device buffer handed to srd_validate_index_device must be
 * readable for: file_len rounded up to 4 KiB plus 8 KiB of slack (contents
 * past file_len are ignored).  The streaming kernel loads whole 4 KiB tiles
 * unconditionally so its prefetch ring never drains on a bounds branch. */
uint64_t srd_padded_size(uint64_t file_len);

/* Device-resident validate+index over `file_len` bytes at `d_file`
 * (device pointer, 16-byte aligned, readable to srd_padded_size(file_len);
 * the bytes are the mmap'd store).  The call launches on the context's own
 * non-blocking stream (srd_ctx_stream): the caller's writes to d_file must be
 * complete, or ordered on that stream, before the call. */
int srd_validate_index_device(srd_ctx *ctx, const uint8_t *d_file,
                              uint64_t file_len, uint32_t flags,
                              srd_device_result *out);

/* Entry-range shard of a store (multi-GPU, one process per GPU; no
 * collective inside).  `d_span` holds file bytes [span_off, hi) -- span_off a
 * multiple of 16 KiB and <= lo, readable to srd_padded_size(hi - span_off) --
 * where lo and hi are entry tails: lo = the previous shard's last tail, hi =
 * this shard's last tail (hi = file_len for the last shard).  Proves that the
 * backward chain from hi reaches an entry whose prev_offset == lo and returns
 * that chain segment (file order, absolute offsets), every payload's CRC and
 * the shard-local latest-wins index.  final_len = hi when proven; otherwise
 * mode = SRD_MODE_SPAN_UNPROVEN, final_len = 0 and the caller falls back to
 * the whole-file path (a torn tail, for example, can only be recovered there,
 * recover_valid_chain's byte-wise outer loop is global).  The shards' chains
 * compose to the whole file's chain when shard 0 has lo = 0 (whole-file rule)
 * and each shard's lo equals the previous shard's hi.  lo == 0 with
 * span_off == 0 is exactly srd_validate_index_device (the whole-file rule:
 * final_len may lie below hi in any mode); a shard is proven iff
 * final_len == hi and mode != SRD_MODE_SPAN_UNPROVEN. */
int srd_validate_span_device(srd_ctx *ctx, const uint8_t *d_span,
                             uint64_t span_off, uint64_t lo, uint64_t hi,
                             uint32_t flags, srd_device_result *out);

/* Shard boundaries of an arbitrary store (host pre-pass, no GPU): cuts[0] = 0,
 * cuts[world] = file_len, and cuts[r] (0 < r < world) the highest byte t at
 * or below r * file_len / world (searched down to 64 MiB below it) whose
 * backward walk passes recover_valid_chain's node test (data_store.rs:404-470)
 * for 8 hops without reaching offset 0.  Non-decreasing; a cut with no candidate repeats the previous
 * one (an empty shard).  The cuts are guesses that srd_validate_span_device
 * plus the composition check prove or refute: [cuts[r], cuts[r+1]) are rank
 * r's lo / hi. */
int srd_shard_cuts(const uint8_t *file, uint64_t file_len, uint32_t world,
                   uint64_t *cuts);

/* Index exchange between shards (KeyIndexer semantics, key_indexer.rs:98-124).
 * Partition n (key_hash, value) pairs (device arrays) by owner rank
 * owner = ((key_hash >> 32) * world) >> 32 into d_out_pairs ([2n] u64,
 * interleaved key,value; grouped by owner, input order kept inside a group);
 * counts[world] (host) receives the group sizes.  Synchronises. */
int srd_index_partition_device(srd_ctx *ctx, const uint64_t *d_keys,
                               const uint64_t *d_vals, uint64_t n,
                               uint32_t world, uint64_t *d_out_pairs,
                               uint64_t *counts);

/* KeyIndexer::build over n interleaved (key_hash, meta_off or packed) device
 * pairs in file order (the latest position of a key wins; tombstones are
 * entries like any other).  Writes the index (key_hash, pack(tag16,
 * offset48)) in file order of each key's latest entry to the caller's device
 * arrays (capacity n each); *n_index = its size.  Synchronises. */
int srd_index_build_device(srd_ctx *ctx, const uint64_t *d_pairs, uint64_t n,
                           uint64_t *d_out_keys, uint64_t *d_out_packed,
                           uint64_t *n_index);

/* Same result with host-memory arrays.  `file` is host memory (e.g. the
 * mmap); it is staged to HBM inside.  The arrays live in pinned host memory
 * owned by the context (ctxs[0] for the multi-GPU form), DMA'd there straight
 * from HBM: valid until the next srd_validate_index(_multi) call on that
 * context; srd_result_free releases nothing then, it only clears the struct
 * (reserved == 1 marks such a result). */
typedef srd_device_result srd_result;
int srd_validate_index(srd_ctx *ctx, const uint8_t *file, uint64_t file_len,
                       uint32_t flags, srd_result *out);
void srd_result_free(srd_result *res);

/* DataStore::open of one host store (the mmap) on n GPUs in ONE process,
 * without RCCL (data_store.rs:84-117).  ctxs[i] are distinct
 * contexts (one per GPU; the same device may repeat, the same context may
 * not: SRD_ERR_ARG).  The host pre-pass
 * srd_shard_cuts splits the store into n entry ranges; one host thread per
 * context stages its span [span_off, hi) and runs srd_validate_span_device.
 * The host composes the shards (every shard proven, each lo == the previous
 * hi); then the chain arrays are concatenated and the per-shard indexes are
 * gathered to ctxs[0]'s device (hipMemcpyPeer over xGMI) in shard order and
 * merged latest-wins there (KeyIndexer::build, key_indexer.rs:98-124).  A
 * store that does not compose (a torn tail, corruption, a wrong cut, a shard
 * error) is decided by the whole-file path on ctxs[0].  The result is
 * identical to srd_validate_index's. */
int srd_validate_index_multi(srd_ctx *const *ctxs, uint32_t n_ctx,
                             const uint8_t *file, uint64_t file_len,
                             uint32_t flags, srd_result *out);

/* ---- the same open over a store already resident in the GPUs' HBM ----
 *   srd_validate_index_multi_device <- DataStore::open (data_store.rs:84-117:
 *                                      recover_valid_chain :383-482 +
 *                                      KeyIndexer::build key_indexer.rs:98-124)
 *                                      with the file sharded by entry range over
 *                                      the GPUs of one node, no RCCL
 * Context i holds its shard in its own HBM: d_spans[i] = file bytes
 * [span_offs[i], cuts[i+1]) (span_offs[i] a multiple of 16 KiB, <= cuts[i];
 * span_offs[0] = 0; readable to srd_padded_size(cuts[i+1] - span_offs[i])).
 * cuts[0] = 0 <= cuts[1] <= .. <= cuts[n] = file_len are entry tails (e.g.
 * from the writer's layout or srd_shard_cuts); an empty shard (cuts[i] ==
 * cuts[i+1]) needs no span.  One host thread per context validates its shard;
 * the host composes them.  Index (latest wins over the whole chain):
 *   default: by owner -- shards[i].index_* (device arrays on ctxs[i]'s GPU)
 *            hold the keys with owner ((key_hash >> 32) * n) >> 32 == i, in
 *            file order of each key's latest entry; every owner pulls its runs
 *            from all shards over xGMI (hipMemcpyPeerAsync) in shard order;
 *   SRD_FLAG_MERGE_INDEX: the whole index on ctxs[0]'s GPU
 *            (summary->index_*, the order srd_validate_index_device gives).
 * shards[i] (array of n) = chain segment i (device arrays on ctxs[i]'s GPU,
 * owned by the context until its next call); the segments concatenated in
 * shard order are the chain in file order.  A shard left unproven by its cut
 * (a cut that is no chain tail) is re-validated together with its lower
 * neighbour, the bytes gathered onto that neighbour's GPU over xGMI; a store
 * that still does not compose (a torn tail, corruption, a shard error) is
 * decided by the whole-file path on ctxs[0] (the store gathered there; its
 * whole chain is then shards[0]).  summary (nullable) reports which path
 * decided, the totals and host timings.  Each entry of ctxs must be a
 * distinct context (the same device may repeat).  Synchronises. */
#define SRD_FLAG_MERGE_INDEX 16u
#define SRD_MULTI_COMPOSED 0u   /* every shard proven on its own */
#define SRD_MULTI_NEIGHBOUR 1u  /* a run of unproven shards proven with its lower neighbour */
#define SRD_MULTI_WHOLE_FILE 2u /* the whole-file path decided (torn tail / corruption / shard error) */
typedef struct {
  uint64_t file_len, final_len;  /* final_len: recover_valid_chain's answer */
  uint64_t n_chain, n_index, n_crc_bad, n_candidates;  /* totals */
  uint32_t mode;          /* SRD_MODE_OPTIMISTIC if every shard's pass was optimistic */
  uint32_t path;          /* SRD_MULTI_* */
  uint32_t n_shards;
  uint32_t merged;        /* 1: the index is summary->index_* on ctxs[0] */
  uint32_t shard_errors;  /* shards whose first validation failed with an error */
  uint32_t peer_errors;   /* cross-device copies between GPUs without peer access
                             (hipDeviceEnablePeerAccess refused: staged by the runtime) */
  double validate_ms;     /* host wall time of the slowest shard's validation(s) */
  double exchange_ms;     /* index exchange + builds */
  double total_ms;        /* the whole call */
  uint64_t *index_key_hash, *index_packed; /* merged: device arrays on ctxs[0] */
} srd_multi_summary;
int srd_validate_index_multi_device(srd_ctx *const *ctxs, uint32_t n_ctx,
                                    const uint8_t *const *d_spans,
                                    const uint64_t *span_offs,
                                    const uint64_t *cuts, uint32_t flags,
                                    srd_device_result *shards,
                                    srd_multi_summary *summary);
/* The summary of the last multi-GPU open (host or device input) that had ctx
 * as ctxs[0]: which path decided it, totals, timings. */
int srd_ctx_multi_summary(srd_ctx *ctx, srd_multi_summary *out);
/* Its per-shard validate times (host wall ms of each shard's own thread,
 * re-validations included): copies up to cap of them to out and returns the
 * shard count (< 0: error). */
int srd_ctx_multi_shard_ms(srd_ctx *ctx, double *out, int cap);
/* Staging of the last host-input call on ctx: *mode = 0 pinned input, 1
 * registered mapping, 2 bounce buffers, 3 pageable copy (-1 none yet);
 * *stage_ms = host wall time from the call's start until the store was in
 * HBM (registration / page faults / copies included).  Nullable outputs. */
int srd_ctx_stage_info(srd_ctx *ctx, int *mode, double *stage_ms);

/* The index bucket hash on the device: out[i] = xxh3_64(le8(keys[i])), the
 * Xxh3BuildHasher's Hasher::write (digest/xxh3_build_hasher.rs:11-13) the
 * KeyIndexer HashMap applies to every key_hash.  Asynchronous on `stream`. */
int srd_index_hash_device(srd_ctx *ctx, const uint64_t *d_keys, uint64_t n,
                          uint64_t *d_out, void *stream);

/* Measurement utility (bench.py's roofline.peak_measured; not part of the
 * reference interface): the streaming-read ceiling of the scan's geometry
 * -- one 16-wave block per CU, a contiguous tile range per wave, 64 B per
 * lane, a 3-deep register ring, no work on the bytes -- over the first
 * floor(bytes / 4096) tiles of d_buf, timed `reps` times (after one warm-up
 * run) with HIP events on the context stream.  *best_ms / *median_ms
 * (nullable) over the reps.  Synchronises. */
int srd_stream_probe_device(srd_ctx *ctx, const uint8_t *d_buf, uint64_t bytes,
                            int reps, double *best_ms, double *median_ms);

/* recover_valid_chain: final_len only (host input). */
int srd_recover_valid_chain(srd_ctx *ctx, const uint8_t *file,
                            uint64_t file_len, uint64_t *final_len);

/* KeyIndexer::build over the chain ending at `tail` (host input).  Writes up
 * to `cap` pairs; *n_out = number of index entries. */
int srd_key_indexer_build(srd_ctx *ctx, const uint8_t *file, uint64_t tail,
                          uint64_t *key_hash_out, uint64_t *packed_out,
                          uint64_t cap, uint64_t *n_out);

/* CRC-32 (crc32fast) of n byte ranges [offs[i], offs[i]+lens[i]) of buf. */
int srd_crc32_batch(srd_ctx *ctx, const uint8_t *buf, uint64_t buf_len,
                    const uint64_t *offs, const uint64_t *lens, uint64_t n,
                    uint32_t *out);
int srd_crc32_batch_device(srd_ctx *ctx, const uint8_t *d_buf,
                           const uint64_t *d_offs, const uint64_t *d_lens,
                           uint64_t n, uint32_t *d_out, void *stream);

/* XXH3-64 (seed 0, default secret) of n keys [offs[i], offs[i]+lens[i]). */
int srd_xxh3_64_batch(srd_ctx *ctx, const uint8_t *keys, uint64_t keys_len,
                      const uint64_t *offs, const uint64_t *lens, uint64_t n,
                      uint64_t *out);
int srd_xxh3_64_batch_device(srd_ctx *ctx, const uint8_t *d_keys,
                             const uint64_t *d_offs, const uint64_t *d_lens,
                             uint64_t n, uint64_t *d_out, void *stream);

/* ---- checksum-on-append batch writer (BASELINE config C5) ----
 *   srd_batch_write           <- DataStoreWriter::batch_write
 *                                src/storage_engine/data_store.rs:838-843
 *                                (compute_hash_batch + batch_write_with_key_hashes
 *                                 data_store.rs:847-939, allow_null_bytes = false)
 *   SRD_WRITE_ALLOW_NULL      <- batch_write_with_key_hashes(.., true), the
 *                                tombstone path used by deletes (:864-897)
 * The serialized bytes are exactly what the reference appends to the file:
 * per entry a zero prepad to the next 64-byte boundary (none for a
 * tombstone), the payload, and EntryMetadata{key_hash, prev_offset = the
 * previous tail, crc32(payload)} (entry_metadata.rs:75-93).  The returned
 * (key_hash, metadata offset) pairs are the reference's key_hash_offsets, in
 * entry order, for the caller's index (reindex, data_store.rs:936). */
#define SRD_WRITE_ALLOW_NULL 1u

typedef struct {
  uint64_t src;      /* payload offset in the payload buffer */
  uint64_t len;      /* payload length (1 for a tombstone) */
  uint64_t key_src;  /* key offset in the key buffer (SRD_ENTRY_HASHED: the key hash) */
  uint64_t tail;     /* file tail before this entry (its prev_offset) */
  uint32_t key_len;
  uint32_t flags;    /* SRD_ENTRY_TOMB | SRD_ENTRY_HASHED */
} srd_write_entry;
#define SRD_ENTRY_TOMB 1u   /* NULL-byte payload written as a tombstone */
#define SRD_ENTRY_HASHED 2u /* key_src holds the key hash (batch_write_with_key_hashes) */

/* Host-side layout of a batch appended at file offset `tail`: fills out[n]
 * and *new_tail.  `payloads` (host) is read only to recognise NULL-byte
 * payloads.  Errors (SRD_ERR_ARG, message as the reference's InvalidInput):
 * "Payload cannot be empty.", "NULL-byte payloads cannot be written
 * directly." (without SRD_WRITE_ALLOW_NULL). */
int srd_batch_layout(uint64_t tail, const uint8_t *payloads,
                     const uint64_t *key_offs, const uint64_t *key_lens,
                     const uint64_t *pay_offs, const uint64_t *pay_lens,
                     uint64_t n, uint32_t flags, srd_write_entry *out,
                     uint64_t *new_tail);

/* batch_write from HOST buffers (pin them for full PCIe rate): payload and
 * key bytes are copied to HBM in chunks on a side stream while the writer
 * kernel serializes the previous chunk on the context stream.  The output
 * goes to d_out (device), d_out[j] = file byte (tail & ~63) + j, capacity
 * out_cap bytes; d_out == NULL only computes *new_tail.  kh_out / mo_out
 * (host, nullable) receive the key hashes and metadata offsets. */
int srd_batch_write(srd_ctx *ctx, uint64_t tail, const uint8_t *keys,
                    const uint64_t *key_offs, const uint64_t *key_lens,
                    const uint8_t *payloads, const uint64_t *pay_offs,
                    const uint64_t *pay_lens, uint64_t n, uint32_t flags,
                    uint8_t *d_out, uint64_t out_cap, uint64_t *new_tail,
                    uint64_t *kh_out, uint64_t *mo_out);

/* The writer kernel alone on device-resident inputs (entries from
 * srd_batch_layout, copied to the device by the caller); out[j] = file byte
 * out_base + j (out_base 64-aligned).  Asynchronous on `stream`. */
int srd_batch_write_device(srd_ctx *ctx, const uint8_t *d_keys,
                           const uint8_t *d_payloads,
                           const srd_write_entry *d_entries, uint64_t n,
                           uint8_t *d_out, uint64_t out_base,
                           uint64_t *d_kh_out, uint64_t *d_mo_out,
                           void *stream);

/* ---- device KeyIndexer + batched keyed reads ----
 *   srd_index_table_build_device <- the KeyIndexer HashMap<u64, u64> that
 *                                   DataStore::open fills (key_indexer.rs:98-124),
 *                                   adopted on the GPU from the validate pass's
 *                                   index arrays instead of re-inserted on the host
 *   srd_index_get_packed_device  <- KeyIndexer::get_packed (key_indexer.rs:164-167)
 *   srd_batch_read_hashed_device <- DataStoreReader::batch_read_hashed_keys
 *                                   (data_store.rs:1117-1158) over
 *                                   read_entry_with_context (:502-565)
 *   srd_batch_read               <- DataStoreReader::batch_read (:1111-1115)
 * The table lives in caller-provided device memory of srd_index_table_bytes(n)
 * bytes (open addressing, load <= 1/2).  A read returns the entry's payload
 * range [start, end) in the file, or start == end == 0 for None: key absent,
 * tag mismatch against the verification hash (the reference's collision
 * check), metadata out of range, or a tombstone. */
#define SRD_INDEX_NONE (~(uint64_t)0) /* get_packed: key absent */

uint64_t srd_index_table_bytes(uint64_t n);
/* n unique (key_hash, packed) device pairs (e.g. srd_device_result's index). */
int srd_index_table_build_device(srd_ctx *ctx, const uint64_t *d_keys,
                                 const uint64_t *d_packed, uint64_t n,
                                 void *d_table, uint64_t table_bytes);
int srd_index_get_packed_device(srd_ctx *ctx, const void *d_table,
                                uint64_t table_bytes, const uint64_t *d_hashes,
                                uint64_t n, uint64_t *d_packed_out, void *stream);
/* d_verify_hashes (nullable): compute_hash of the non-hashed keys; the read is
 * None when its tag (hash >> 48) differs from the indexed entry's tag. */
int srd_batch_read_hashed_device(srd_ctx *ctx, const void *d_table,
                                 uint64_t table_bytes, const uint8_t *d_file,
                                 uint64_t file_len, const uint64_t *d_hashes,
                                 const uint64_t *d_verify_hashes, uint64_t n,
                                 uint64_t *d_start, uint64_t *d_end, void *stream);
/* Host keys in, host ranges out: keys hashed on the device (XXH3-64) and
 * verified by their own tags, as batch_read does.  Synchronises. */
int srd_batch_read(srd_ctx *ctx, const void *d_table, uint64_t table_bytes,
                   const uint8_t *d_file, uint64_t file_len, const uint8_t *keys,
                   const uint64_t *key_offs, const uint64_t *key_lens, uint64_t n,
                   uint64_t *start_out, uint64_t *end_out);

/* ---- the device KeyIndexer kept live: appends and deletes in place ----
 *   srd_index_table_apply_device   <- DataStore::reindex (data_store.rs:224-259)
 *                                     over KeyIndexer::insert (key_indexer.rs:135-160)
 *                                     and KeyIndexer::remove (:174-178), the
 *                                     step every write ends in (:936)
 *   srd_index_table_export_device  <- the live map's pairs in file order (what
 *                                     KeyIndexer::build would give without the
 *                                     removed keys), for the iterator /
 *                                     compaction calls below and for growth
 *   srd_batch_delete_hashed_device <- DataStoreWriter::batch_delete_key_hashes
 *                                     (data_store.rs:995-1024)
 * The table is the one srd_index_table_build_device fills.  A removed key's
 * slot keeps its key and holds the value ~0 - 1 ("deleted": no packed value,
 * its offset 2^48 - 2 lies above any file_len); every read reports such a key
 * as absent (SRD_INDEX_NONE / start == end == 0) and probes on past it, and a
 * later insert of the key revives the slot.  `used` counts the slots that
 * are not empty (live + deleted): n after a build; it only grows, and a table
 * holds at most capacity / 2 of them (capacity = the largest power of two
 * with 16 * capacity <= table_bytes).  To grow, or to drop the deleted slots:
 * export, then srd_index_table_build_device into a larger buffer.
 * A table that is built and never modified answers exactly as before. */
#define SRD_ERR_FULL (-5) /* the batch's new keys would push the used slots above capacity / 2; table unchanged */
typedef struct {
  uint64_t n_inserted; /* distinct keys absent before, present after */
  uint64_t n_updated;  /* present before and after */
  uint64_t n_removed;  /* present before, absent after */
} srd_index_apply_stats;
/* The reference's loop over n (key_hash, metadata offset) device pairs in
 * batch order -- d_kh_out / d_mo_out of srd_batch_write_device as they are;
 * d_tomb (nullable) marks the pairs that are tombstones.  Afterwards every
 * key with at least one tombstone pair in the batch is absent (deleted_keys,
 * data_store.rs:861,896: also when the batch wrote it, before or after), and
 * every other key maps to pack(key_hash >> 48, offset) of its last pair.
 * SRD_ERR_FULL: *used + the batch's distinct new keys > capacity / 2; nothing
 * was written (the look-up runs first, the commit second).
 * Ordered on `stream`; waits once, for the look-up's counts, and returns
 * with the commit enqueued: later work on `stream` sees the new table. */
int srd_index_table_apply_device(srd_ctx *ctx, void *d_table,
                                 uint64_t table_bytes, uint64_t *used,
                                 const uint64_t *d_key_hashes,
                                 const uint64_t *d_meta_offs,
                                 const uint8_t *d_tomb, uint64_t n,
                                 srd_index_apply_stats *stats, void *stream);
/* The live (key_hash, packed) pairs in ascending metadata offset (file order,
 * the order of srd_device_result's index arrays) into device arrays of
 * cap_out elements; *n_live = their number.  Both outputs NULL: the count
 * only.  On the context stream; synchronises. */
int srd_index_table_export_device(srd_ctx *ctx, const void *d_table,
                                  uint64_t table_bytes, uint64_t *d_keys_out,
                                  uint64_t *d_packed_out, uint64_t cap_out,
                                  uint64_t *n_live);
/* Keeps the hashes the index holds (input order, duplicates kept; a removed
 * key is absent, a key whose indexed entry is a tombstone on disk is held),
 * appends one tombstone entry per kept hash at `tail` of the store at d_file
 * (d_file[j] = file byte j, writable to file_cap bytes; 21 bytes each: a NULL
 * byte, no prepad, prev_offset = the previous tail, CRC 0xD202EF8D) and
 * removes the keys from the table.  *n_deleted (nullable) = tombstones
 * written.  Nothing kept: nothing written, *new_tail = tail.  SRD_ERR_ARG
 * when srd_padded_size(new tail) > file_cap (nothing written).  On the
 * context stream; synchronises. */
int srd_batch_delete_hashed_device(srd_ctx *ctx, void *d_table,
                                   uint64_t table_bytes, uint64_t *used,
                                   const uint64_t *d_hashes, uint64_t n,
                                   uint64_t tail, uint8_t *d_file,
                                   uint64_t file_cap, uint64_t *new_tail,
                                   uint64_t *n_deleted);

/* ---- iteration and compaction over the device index ----
 *   srd_iter_entries_device   <- EntryIterator (entry_iterator.rs:69-126) /
 *                                par_iter_entries (data_store.rs:297-361):
 *                                the latest non-tombstone entry per key, in
 *                                EntryIterator order (newest first)
 *   srd_estimate_compaction_savings_device
 *                             <- estimate_compaction_savings (:605-616)
 *   srd_compact_device        <- compact (:706-749): the latest entries
 *                                re-serialized by write_stream_with_key_hash
 *                                in iter_entries order from offset 0 (the
 *                                write_kernel with prehashed keys), into d_out
 * d_index_packed = srd_device_result.index_packed (n_index values). */
int srd_iter_entries_device(srd_ctx *ctx, const uint8_t *d_file,
                            uint64_t file_len, const uint64_t *d_index_packed,
                            uint64_t n_index, uint64_t *d_start, uint64_t *d_end,
                            uint64_t *d_meta_off, uint64_t *d_key_hash,
                            uint64_t *n_out);
int srd_estimate_compaction_savings_device(srd_ctx *ctx, const uint8_t *d_file,
                                           uint64_t file_len,
                                           const uint64_t *d_index_packed,
                                           uint64_t n_index, uint64_t *savings);
/* d_out == NULL only computes *new_len.  Fails (SRD_ERR_ARG) like the
 * reference when a kept payload is all NULL bytes ("NULL-byte-only streams
 * cannot be written directly."). */
int srd_compact_device(srd_ctx *ctx, const uint8_t *d_file, uint64_t file_len,
                       const uint64_t *d_index_packed, uint64_t n_index,
                       uint8_t *d_out, uint64_t out_cap, uint64_t *new_len,
                       uint64_t *d_key_hash_out, uint64_t *d_meta_off_out);

/* ---- verified payloads: batched gather with checksum check ----
 *   srd_payload_gather_device <- what a reader does with the handles a read
 *                                returns: EntryHandle::as_slice plus
 *                                EntryHandle::is_valid_checksum
 *                                (simd-r-drive-entry-handle/src/entry_handle.rs:260-275),
 *                                for a whole batch of ranges
 * d_start / d_end are n payload ranges [start, end) as the read and iterator
 * calls above write them (srd_device_result's payload_start / meta_off work as
 * they are): end is the entry's metadata offset, the stored checksum the
 * little-endian u32 at d_file[end + 16 .. end + 20).  The ranges are the
 * caller's: a range that does not lie inside the file with its metadata is
 * refused by arithmetic (SRD_GATHER_BAD_RANGE) and nothing of it is read; no
 * byte outside [0, file_len) is read because of any range.  Any start alignment
 * gives the right bytes and CRC; 64-aligned starts (every real entry) are the
 * fast path.
 * Output: d_out_off[i] = the exclusive sum of roundup64(end - start) over the
 * queries with status OK or BAD_CRC, d_out_off[n] = the total (also *total);
 * payload i lies at d_out[d_out_off[i] ..) and the bytes up to the next
 * 64-byte boundary are written as zero; no byte at or past the total is
 * touched.  d_out must be 16-byte aligned.  d_crc_computed[i] (nullable) =
 * crc32(payload i), 0 for NONE / BAD_RANGE.
 *   d_out == NULL without SRD_GATHER_VERIFY_ONLY: the layout only -- d_out_off,
 *     *total and the NONE / BAD_RANGE statuses (the statuses of the other
 *     queries and d_crc_computed are left as they are);
 *   SRD_GATHER_VERIFY_ONLY: d_out is ignored and never written; statuses and
 *     CRCs are complete (a batched is_valid_checksum).
 * SRD_ERR_ARG, nothing written but *total: the total exceeds out_cap; [d_out,
 * d_out + out_cap) overlaps the store's padded range; n >= 2^31; the
 * batch has 2^32 or more work units.
 * Ordered on `stream`; waits once, for the total, and returns with the copy
 * enqueued: later work on `stream` sees the outputs.  The workspace comes
 * from the context (srd_ctx_device_bytes counts it). */
#ifndef SRD_GATHER_CHUNK
#define SRD_GATHER_CHUNK 65536u   /* work-unit size in bytes, a multiple of 4096 (measured: DESIGN.md section 11) */
#endif
#define SRD_GATHER_VERIFY_ONLY 1u /* compute statuses and CRCs, copy nothing */
/* d_status values */
#define SRD_GATHER_NONE 0u       /* start == end (a read's None): nothing copied */
#define SRD_GATHER_OK 1u         /* copied, crc32(payload) == the stored checksum */
#define SRD_GATHER_BAD_CRC 2u    /* copied faithfully, checksum differs */
#define SRD_GATHER_BAD_RANGE 3u  /* start > end, or end + 20 > file_len: nothing read, nothing copied */
int srd_payload_gather_device(srd_ctx *ctx, const uint8_t *d_file, uint64_t file_len,
                              const uint64_t *d_start, const uint64_t *d_end, uint64_t n,
                              uint32_t flags, uint8_t *d_out, uint64_t out_cap,
                              uint64_t *d_out_off /* n + 1 */, uint8_t *d_status /* n */,
                              uint32_t *d_crc_computed /* n, nullable */,
                              uint64_t *total, void *stream);

/* ---- payloads already in HBM appended to a store ----
 *   srd_batch_append_device <- DataStoreWriter::batch_write_with_key_hashes(.., false)
 *                              (data_store.rs:847-939) for payloads that are
 *                              device ranges, = n write_stream_with_key_hash
 *                              calls (:758-825); what copy / transfer / rename
 *                              (:941-984) run on
 * d_src_off / d_len are n ranges [off, off + len) inside d_payloads[0 ..
 * payloads_len); d_file[j] = file byte j, writable to file_cap bytes, 16-byte
 * aligned.  With P_0 = roundup64(tail): entry i's payload lies at P_i, its
 * metadata {key_hash, prev_offset, crc32(payload)} at m_i = P_i + len_i,
 * prev_offset_0 = tail, prev_offset_i = m_(i-1) + 20, P_(i+1) = roundup64(m_i +
 * 20), *new_tail = m_(n-1) + 20; the bytes [tail, P_0) and [m_i + 20, P_(i+1))
 * are zero.  d_meta_off_out[i] = m_i: with d_key_hashes, the pairs
 * srd_index_table_apply_device takes as they are (the call itself does not
 * touch any index table).  No byte below tail changes, none at or above
 * roundup64(*new_tail) is touched, and [*new_tail, roundup64(*new_tail)) is
 * left alone or written as zero.  Any source alignment gives the right bytes;
 * 16-byte-aligned sources are the fast path.  No tombstones (deletes:
 * srd_batch_delete_hashed_device).  n == 0: *new_tail = tail, nothing runs.
 * SRD_ERR_ARG with the reference's message, nothing written to d_file or
 * d_meta_off_out, *new_tail = tail: a length of 0 ("Payload cannot be
 * empty."); a payload that is the single byte 0 ("NULL-byte payloads cannot be
 * written directly."; the only payload byte the layout reads); a range not
 * inside [0, payloads_len) (judged without wrap, never dereferenced); a new
 * tail of 2^48 or more; srd_padded_size(new tail) > file_cap (the message names
 * file_cap); d_payloads[0 .. payloads_len) overlapping d_file[tail ..
 * roundup64(new tail)); n >= 2^31; 2^32 or more work units (chunks of
 * SRD_GATHER_CHUNK bytes of one entry).  With several refused entries the
 * first in batch order decides the message.
 * SRD_APPEND_STREAM_RULE adds write_stream's check (data_store.rs:783-797): a
 * payload of any length whose bytes are all 0 fails the call with
 * "NULL-byte-only streams cannot be written directly." -- known only after
 * the bytes have been streamed, as in the reference: bytes at or above tail
 * and d_meta_off_out may have been written, *new_tail = tail, and the
 * caller's tail and index do not move.
 * Ordered on `stream`; waits once, for the error word, the new tail and the
 * unit counts, and returns with the copy enqueued: later work on `stream`
 * sees the store and d_meta_off_out.  With SRD_APPEND_STREAM_RULE the call
 * waits a second time, for the kernels, before it returns.  The workspace
 * comes from the context (srd_ctx_device_bytes counts it). */
#define SRD_APPEND_STREAM_RULE 1u
int srd_batch_append_device(srd_ctx *ctx, const uint8_t *d_payloads, uint64_t payloads_len,
                            const uint64_t *d_src_off, const uint64_t *d_len,
                            const uint64_t *d_key_hashes, uint64_t n, uint32_t flags,
                            uint64_t tail, uint8_t *d_file, uint64_t file_cap,
                            uint64_t *new_tail, uint64_t *d_meta_off_out /* n */,
                            void *stream);

/* ---- entries whose payload is a sequence of device segments ----
 *   srd_batch_append_segments_device <- n write_stream_with_key_hash calls
 *                              (data_store.rs:758-825): the payload arrives in
 *                              pieces, the checksum runs over the pieces in
 *                              order (:775,788), the entry is laid out like
 *                              any other
 * src_ptrs / src_lens are HOST arrays of n_src device ranges [src_ptrs[k],
 * src_ptrs[k] + src_lens[k]): the call's source table.  The sources are only
 * read; they may overlap each other and may be the store itself below tail.
 * d_segs (device) holds n_segs segments, each the bytes sources[src][off ..
 * off + len); one segment may name the same bytes as another, len may be 0.
 * d_seg_first (device, n + 1 values, first[0] = 0, non-decreasing, first[n] =
 * n_segs): entry i's payload is the concatenation of the segments d_segs[
 * first[i] .. first[i + 1]) in order, its length len_i the sum of theirs.
 * Everything else is srd_batch_append_device's contract: d_file[j] = file byte
 * j, writable to file_cap bytes, 16-byte aligned; with P_0 = roundup64(tail)
 * entry i's payload lies at P_i, its metadata {key_hash, prev_offset,
 * crc32(payload)} at m_i = P_i + len_i, prev_offset_0 = tail, prev_offset_i =
 * m_(i-1) + 20, P_(i+1) = roundup64(m_i + 20), *new_tail = m_(n-1) + 20; the
 * bytes [tail, P_0) and [m_i + 20, P_(i+1)) are zero; d_meta_off_out[i] = m_i;
 * the call touches no index table.  No byte below tail changes, none at or
 * above roundup64(*new_tail) is touched, and [*new_tail, roundup64(*new_tail))
 * is left alone or written as zero.  Whole 16-byte vectors of the store are
 * written at any source and destination alignment (a piece's destination is
 * wherever the previous piece ended).  n == 0: *new_tail = tail, nothing runs.
 * SRD_ERR_ARG, nothing written to d_file or d_meta_off_out, *new_tail = tail
 * (the first refused entry in batch order decides the message):
 *   an entry with no segments, or only zero-length ones ("Payload cannot be
 *     empty.", data_store.rs:799-804);
 *   a malformed segment -- src >= n_src, reserved != 0, a range not inside its
 *     source (judged without wrap), an entry length of 2^48 or more: such a
 *     segment is never dereferenced, the message names the entry, and the
 *     entry is refused for it whatever its total length;
 *   a malformed d_seg_first: first[0] != 0, a decreasing pair, first[n] !=
 *     n_segs;
 *   a new tail of 2^48 or more; srd_padded_size(new tail) > file_cap (the
 *     message names file_cap); n >= 2^31; n_segs >= 2^31; 2^32 or more work
 *     units (pieces of at most SRD_GATHER_CHUNK bytes of one segment);
 *     flags != 0;
 *   a source [src_ptrs[k], src_ptrs[k] + src_lens[k]) that meets d_file[tail ..
 *     roundup64(new tail)).
 * The stream rule is always on -- this is write_stream: a payload whose bytes
 * are all 0 (any length, over all its segments) fails the call with
 * "NULL-byte-only streams cannot be written directly." (:792-797), known only
 * after the bytes have been streamed, as documented for
 * SRD_APPEND_STREAM_RULE: bytes at or above tail and d_meta_off_out may have
 * been written, *new_tail = tail, the caller's tail and index do not move.
 * Ordered on `stream`; the call waits twice: once for the error word, the new
 * tail and the unit counts, and once more, for the kernels, before it returns
 * (later work on `stream` sees the store and d_meta_off_out).  The workspace
 * comes from the context (srd_ctx_device_bytes counts it). */
typedef struct {
  uint32_t src;       /* index into the call's source table (srd_payload_scatter_device: its DESTINATION table) */
  uint32_t reserved;  /* 0 */
  uint64_t off, len;  /* the bytes sources[src][off .. off + len); len may be 0 */
} srd_segment;        /* 24 bytes, no padding */
int srd_batch_append_segments_device(srd_ctx *ctx, const uint8_t *const *src_ptrs,
                                     const uint64_t *src_lens, uint64_t n_src,
                                     const srd_segment *d_segs, uint64_t n_segs,
                                     const uint64_t *d_seg_first /* n + 1 */,
                                     const uint64_t *d_key_hashes, uint64_t n, uint32_t flags /* 0 */,
                                     uint64_t tail, uint8_t *d_file, uint64_t file_cap,
                                     uint64_t *new_tail, uint64_t *d_meta_off_out /* n */,
                                     void *stream);

/* ---- verified payloads read into a sequence of device segments ----
 *   srd_payload_scatter_device <- EntryStream, a Read over an EntryHandle that
 *                                 fills the caller's buffers piece by piece
 *                                 (src/storage_engine/entry_stream.rs:44-92),
 *                                 with EntryHandle::is_valid_checksum
 *                                 (simd-r-drive-entry-handle/src/entry_handle.rs:260-275),
 *                                 for a whole batch of ranges
 * The read-side mirror of srd_batch_append_segments_device: no packed buffer,
 * every payload goes straight to where the caller wants its pieces.
 * d_start / d_end are srd_payload_gather_device's ranges, word for word: n
 * payload ranges [start, end), end the entry's metadata offset, the stored
 * checksum the little-endian u32 at d_file[end + 16 .. end + 20); any start
 * alignment is accepted; start == end is a read's None; a range that does not
 * lie inside the file with its metadata is SRD_GATHER_BAD_RANGE.
 * dst_ptrs / dst_lens are HOST arrays of n_dst writable device ranges
 * [dst_ptrs[k], dst_ptrs[k] + dst_lens[k]): the call's destination table, as
 * src_ptrs / src_lens are the segment append's source table.  It is uploaded
 * before the call's one wait: the host arrays are the caller's again on
 * return.  Table ranges may overlap each other.
 * d_segs / d_seg_first (device) are the segment append's arrays and the same
 * srd_segment, src being the index into the DESTINATION table: query i's
 * payload is delivered in order into the segments d_segs[first[i] .. first[i +
 * 1]), segment s receiving the payload bytes [soff_s, soff_s + len_s), soff_s
 * the sum of the lengths before it in the query.  A segment may be empty;
 * several segments may point into one table range (one arena).  Two segments
 * of one call that name the same destination byte are not detected: that byte
 * ends as one of the bytes written to it; statuses and CRCs are still right.
 * d_status[i]:
 *   SRD_GATHER_NONE       start == end: the query's segments are ignored,
 *                         nothing is written;
 *   SRD_GATHER_BAD_RANGE  as the gather: nothing read, nothing written;
 *   SRD_GATHER_OK         delivered, crc32(payload) == the stored checksum;
 *   SRD_GATHER_BAD_CRC    delivered faithfully, the checksum differs;
 *   SRD_SCATTER_BAD_LENGTH  the segments' lengths do not sum to end - start:
 *                         nothing of the entry is read, none of its
 *                         destinations is written.
 * The range decides before the length does.  d_crc_computed[i] (nullable) =
 * crc32(payload i), 0 for NONE / BAD_RANGE / BAD_LENGTH.
 * No byte outside the named destination bytes of OK / BAD_CRC queries is
 * written: no padding, no zero fill; the bytes between, below and behind
 * segments are left alone, the other 15 bytes of a 16-byte vector that holds a
 * segment's head or tail included (whole 16-byte vectors are stored wherever a
 * vector lies inside one segment, at any source and destination alignment).
 * Of a payload nothing outside [start, end) is read, plus its 4 checksum bytes.
 * SRD_ERR_ARG, nothing written to any destination, d_status or d_crc_computed
 * (the first refused query in batch order decides the message):
 *   a malformed segment -- src >= n_dst, reserved != 0, a range not inside its
 *     table range (judged without wrap): never dereferenced, and it decides
 *     whatever the query's status would be;
 *   a malformed d_seg_first: first[0] != 0, a decreasing pair, first[n] !=
 *     n_segs;
 *   flags != 0; n >= 2^31; n_segs >= 2^31; n_dst >= 2^32; 2^32 or more work
 *     units (pieces of at most SRD_GATHER_CHUNK bytes of one segment);
 *   a table range of length > 0 with a NULL pointer, or one that meets d_file[0
 *     .. srd_padded_size(file_len)) -- checked on the host before anything runs.
 * n == 0 runs nothing.
 * Ordered on `stream`; waits once, for the error word, the unit total and the
 * multi-unit count, and returns with the copy and the finish enqueued: later
 * work on `stream` sees the destinations and both output arrays; d_segs and
 * d_seg_first stay alive as for any stream work.  The workspace comes from the
 * context (srd_ctx_device_bytes counts it). */
#define SRD_SCATTER_BAD_LENGTH 4u /* d_status: the segments' lengths do not sum to end - start */
int srd_payload_scatter_device(srd_ctx *ctx, const uint8_t *d_file, uint64_t file_len,
                               const uint64_t *d_start, const uint64_t *d_end, uint64_t n,
                               uint8_t *const *dst_ptrs, const uint64_t *dst_lens, uint64_t n_dst,
                               const srd_segment *d_segs, uint64_t n_segs,
                               const uint64_t *d_seg_first /* n + 1 */, uint32_t flags /* 0 */,
                               uint8_t *d_status /* n */, uint32_t *d_crc_computed /* n, nullable */,
                               void *stream);

/* ---- a live session compacted on the device, its index carried over ----
 *   srd_compact_live_device <- DataStore::compact (data_store.rs:706-749) over
 *                              iter_entries (:276-280) / EntryIterator
 *                              (entry_iterator.rs:69-126), each entry written
 *                              by copy_handle (:587-590), which is
 *                              write_stream_with_key_hash (:758-825)
 * d_table is the live table of the store d_file[0 .. file_len) (as
 * srd_index_table_build_device / _apply_device / srd_batch_delete_hashed_device
 * leave it); both are only read.  The entries written are the table's live
 * pairs -- what srd_index_table_export_device gives, removed keys are absent --
 * that pass par_iter_entries' filter (a key whose indexed entry is a tombstone
 * on disk is dropped), newest first: the order of srd_iter_entries_device over
 * the export.  No trip through a validate pass, and the pairs never leave the
 * device.
 * d_out[0 .. new_len) is exactly what srd_batch_append_device(..,
 * SRD_APPEND_STREAM_RULE, tail = 0, ..) writes for those payload ranges in that
 * order (its comment above is the layout rule: P_0 = 0, P_(i+1) = roundup64(m_i
 * + 20), metadata {key_hash, prev_offset, crc32(payload)}, zero prepads; the
 * checksum is recomputed) -- byte for byte what srd_compact_device writes for
 * the same index.  No byte at or above roundup64(new_len) is touched, and
 * [new_len, roundup64(new_len)) is left alone or written as zero.  d_out must
 * be 16-byte aligned.
 * d_new_table (new_table_bytes >= srd_index_table_bytes(n_entries)) receives
 * the table srd_index_table_build_device would build from the n_entries pairs
 * (key_hash, pack(key_hash >> 48, new metadata offset)): its `used` count is
 * n_entries, no slot is deleted.
 * A written entry whose recomputed CRC-32 differs from the checksum stored in
 * the source (the little-endian u32 at d_file[end + 16 .. end + 20)) is copied
 * faithfully, as the reference would, gets the recomputed checksum, and counts
 * into n_crc_bad: a bad CRC is data, never an error -- the caller decides.
 * d_out == NULL is a planning call: n_entries, new_len and kept_bytes only,
 * nothing is written, d_new_table is ignored.
 * SRD_ERR_ARG, nothing written to d_out or d_new_table, n_entries / kept_bytes
 * / new_len still reported where they are known (the first three cases below:
 * nothing has run, they are 0):
 *   d_out not 16-byte aligned;
 *   [d_out, d_out + out_cap) or [d_new_table, d_new_table + new_table_bytes)
 *     overlapping the store's padded range (srd_padded_size(file_len)), the old
 *     table, or each other;
 *   a NULL stats, a table_bytes below the smallest table;
 *   srd_padded_size(new_len) > out_cap (the store the call leaves is one the
 *     validate and append calls can take as it is: they need that slack);
 *   new_table_bytes < srd_index_table_bytes(n_entries);
 *   the append's own bounds: 2^31 or more entries, 2^32 or more work units, a
 *     new length of 2^48 or more.
 * A kept payload whose bytes are all 0 fails the call with the reference's
 * "NULL-byte-only streams cannot be written directly." (as srd_compact_device
 * and the stream rule do): known only after the bytes have been streamed, so
 * d_out and d_new_table may have been written by then.
 * No live entry: n_entries = new_len = 0, an empty table is built, nothing
 * else runs.
 * On the context stream; synchronises (one wait behind the kernels, for the
 * stream rule's outcome and n_crc_bad), like srd_batch_delete_hashed_device:
 * the caller's writes to d_file and d_table must be complete, or ordered on
 * that stream, before the call.  The workspace comes from the context
 * (srd_ctx_device_bytes counts it). */
typedef struct {
  uint64_t n_entries;   /* entries written: the table's live keys whose indexed entry is not a tombstone */
  uint64_t new_len;     /* length of the compacted store */
  uint64_t kept_bytes;  /* sum of (payload length + 20) over them: estimate_compaction_savings' unique_entry_size */
  uint64_t n_crc_bad;   /* written entries whose recomputed CRC-32 differs from the checksum stored in the source */
  uint64_t first_bad;   /* source metadata offset of the first of them in output order; ~0 when there is none */
} srd_compact_stats;
int srd_compact_live_device(srd_ctx *ctx, const void *d_table, uint64_t table_bytes,
                            const uint8_t *d_file, uint64_t file_len,
                            uint8_t *d_out, uint64_t out_cap,
                            void *d_new_table, uint64_t new_table_bytes,
                            srd_compact_stats *stats);

/* ---- TTL entries: namespaced keys, expiry reads, eviction and the sweep ----
 *   srd_namespace_hash_batch[_device] <- NamespaceHasher::namespace
 *                                (src/utils/namespace_hasher.rs:33-65) followed
 *                                by compute_hash of the namespaced key
 *   srd_ttl_resolve[_keys]_device <- the decision of StorageCacheExt::
 *                                read_with_ttl (extensions/src/storage_cache_ext.rs:72-107)
 *                                for a batch, nothing written
 *   srd_ttl_evict_device      <- that read's delete(namespaced key) of an
 *                                expired entry (storage_cache_ext.rs:91-96),
 *                                for the batch's expired keys
 *   srd_ttl_sweep_device      <- no counterpart: the reference evicts an
 *                                expired entry only when somebody reads it
 * The contract (write_with_ttl, storage_cache_ext.rs:23-58; TTL_PREFIX = the 5
 * bytes F7 74 74 6C FD, extensions/src/constants.rs:20-42): the namespaced key
 * of `key` under `prefix` is the 16 bytes le64(xxh3_64(prefix)) ||
 * le64(xxh3_64(key)); the entry is stored under key_hash = xxh3_64(namespaced
 * key); its payload is le64(expiry) || value with expiry =
 * now_secs.saturating_add(ttl_secs).  Writing needs no call of its own: the
 * payload goes through any write or append call above under that key_hash.
 * A read at `now`: absent -> NotFound; payload below 8 bytes -> InvalidData
 * ("Data too short to contain TTL"); now >= expiry -> the entry is deleted,
 * None; otherwise the value.  The read's tag check compares the stored tag
 * with the tag of the hash the entry was found by, so it cannot fire. */
#define SRD_TTL_NOT_FOUND 0u  /* absent, removed, or the indexed entry is a tombstone / out of range */
#define SRD_TTL_LIVE      1u
#define SRD_TTL_EXPIRED   2u  /* now >= expiry */
#define SRD_TTL_TOO_SHORT 3u  /* payload < 8 bytes: the reference's InvalidData */

/* Key i = d_keys[d_offs[i] .. d_offs[i] + d_lens[i]) (device).  d_hash_out[i] =
 * xxh3_64 of key i's namespaced key under prefix_hash = xxh3_64(prefix);
 * d_ns_out (nullable; 16 n bytes, 8-byte aligned) receives the namespaced keys
 * themselves.  Reads the keys, writes the two outputs, nothing else.
 * Asynchronous on `stream` (NULL: the context's): returns with the kernel
 * enqueued.  SRD_ERR_ARG: a NULL context, a missing array with n > 0, d_ns_out
 * not 8-byte aligned. */
int srd_namespace_hash_batch_device(srd_ctx *ctx, uint64_t prefix_hash, const uint8_t *d_keys,
                                    const uint64_t *d_offs, const uint64_t *d_lens, uint64_t n,
                                    uint8_t *d_ns_out /* 16 n, nullable */, uint64_t *d_hash_out /* n */,
                                    void *stream);
/* The same for host arrays (keys[0 .. klen), every key inside it: SRD_ERR_ARG
 * otherwise), as srd_xxh3_64_batch: staged, hashed and copied back on the
 * context stream; synchronises.  ns_out is nullable. */
int srd_namespace_hash_batch(srd_ctx *ctx, uint64_t prefix_hash, const uint8_t *keys, uint64_t klen,
                             const uint64_t *offs, const uint64_t *lens, uint64_t n,
                             uint8_t *ns_out /* 16 n, nullable */, uint64_t *hash_out /* n */);

/* read_with_ttl's decision for n key hashes (of namespaced keys) against the
 * live table d_table of the store d_file[0 .. file_len), judged at `now`: per
 * query the probe (KeyIndexer::get_packed), the indexed entry's metadata with
 * srd_batch_read_hashed_device's bounds, prepad and tombstone rules, and -- only
 * when the payload holds them -- the 8 expiry bytes at its start.  No byte
 * outside [0, file_len) is read, and the call reads only: table and store are
 * left as they are.
 *   d_status[i]        SRD_TTL_*
 *   d_start / d_end    LIVE: the whole payload, its 8 expiry bytes included --
 *                      srd_payload_gather_device and srd_payload_scatter_device
 *                      take these ranges as they are, and the stored CRC covers
 *                      what they stream; every other status: (0, 0), the
 *                      gather's NONE
 *   d_expiry[i]        (nullable) the stored expiry for LIVE and EXPIRED, else 0
 *   d_counts           (nullable, 4 x u64) set to the number of queries per status
 * A batch is judged against the store as it is when the call runs: a key that
 * is expired and appears twice is EXPIRED twice (n sequential reference reads
 * would delete it at the first and say NotFound at the second).
 * Asynchronous on `stream` (NULL: the context's): returns with the work
 * enqueued, later work on `stream` sees the outputs.  SRD_ERR_ARG, nothing
 * written: a NULL context, a table_bytes below the smallest table, a missing
 * array with n > 0. */
int srd_ttl_resolve_device(srd_ctx *ctx, const void *d_table, uint64_t table_bytes,
                           const uint8_t *d_file, uint64_t file_len,
                           const uint64_t *d_hashes, uint64_t n, uint64_t now,
                           uint64_t *d_start, uint64_t *d_end, uint64_t *d_expiry /* nullable */,
                           uint8_t *d_status, uint64_t *d_counts /* 4, nullable */, void *stream);
/* The same from the raw keys (key i = d_keys[d_offs[i] .. + d_lens[i]), as
 * srd_namespace_hash_batch_device), hashed inside the same launch: a keyed
 * read's decision in one kernel, no intermediate arrays.  d_hashes_out[i] = the
 * key hash query i was looked up by (what srd_ttl_evict_device takes). */
int srd_ttl_resolve_keys_device(srd_ctx *ctx, const void *d_table, uint64_t table_bytes,
                                const uint8_t *d_file, uint64_t file_len, uint64_t prefix_hash,
                                const uint8_t *d_keys, const uint64_t *d_offs, const uint64_t *d_lens,
                                uint64_t n, uint64_t now, uint64_t *d_hashes_out,
                                uint64_t *d_start, uint64_t *d_end, uint64_t *d_expiry /* nullable */,
                                uint8_t *d_status, uint64_t *d_counts /* 4, nullable */, void *stream);

/* srd_batch_delete_hashed_device restricted to the queries with d_status[i] ==
 * SRD_TTL_EXPIRED (as a resolve call wrote them) and deduplicated: one
 * tombstone per distinct key among them, in batch order of each key's last
 * such query, appended at `tail` of the store at d_file (d_file[j] = file byte
 * j, writable to file_cap bytes; 21 bytes each: a NULL byte, no prepad,
 * prev_offset = the previous tail, CRC 0xD202EF8D), and the keys removed from
 * the table.  *n_evicted (nullable) = tombstones written.  Nothing expired:
 * nothing written, *new_tail = tail.  SRD_ERR_ARG when srd_padded_size(new
 * tail) > file_cap (nothing written, *new_tail = tail), for n >= 2^31 and for
 * missing arguments.  On the context stream; synchronises. */
int srd_ttl_evict_device(srd_ctx *ctx, void *d_table, uint64_t table_bytes, uint64_t *used,
                         const uint64_t *d_hashes, const uint8_t *d_status, uint64_t n,
                         uint64_t tail, uint8_t *d_file, uint64_t file_cap,
                         uint64_t *new_tail, uint64_t *n_evicted);

/* The sweep: every live pair of the table (what srd_index_table_export_device
 * gives, ascending metadata offset) judged at `now` by the resolve's rule, and
 * the expired ones evicted -- one tombstone each, in ascending metadata offset
 * of the entries they remove, written and applied as srd_ttl_evict_device
 * does.  KEYS ARE NOT STORED, so nothing tells a TTL entry from any other:
 * EVERY live entry is judged as a TTL entry, its first 8 payload bytes taken
 * as an expiry.  The call is for stores written only through the TTL writes.
 * Entries whose payload is below 8 bytes are left alone and counted (n_short).
 * SRD_TTL_SWEEP_PLAN computes the stats and writes nothing.  *new_tail = tail
 * when nothing is written.  SRD_ERR_ARG: srd_padded_size(new tail) > file_cap
 * (nothing written, the stats are reported), unknown flags, missing arguments,
 * 2^31 or more live pairs.  On the context stream; synchronises; the
 * workspace comes from the context (srd_ctx_device_bytes counts it). */
#define SRD_TTL_SWEEP_PLAN 1u
typedef struct {
  uint64_t n_judged;     /* live pairs of the table */
  uint64_t n_expired;    /* of them now >= expiry: the tombstones (to be) written */
  uint64_t n_short;      /* of them with a payload below 8 bytes: left alone */
  uint64_t next_expiry;  /* the smallest expiry among the survivors (LIVE); ~0 when there is none */
} srd_ttl_sweep_stats;
int srd_ttl_sweep_device(srd_ctx *ctx, void *d_table, uint64_t table_bytes, uint64_t *used,
                         uint8_t *d_file, uint64_t tail, uint64_t file_cap, uint64_t now,
                         uint32_t flags, uint64_t *new_tail, srd_ttl_sweep_stats *stats);

/* ---- keyed reads into fixed-size rows, no host wait, graph-replayable ----
 *   srd_read_rows_device <- batch_read_hashed_keys (data_store.rs:1111-1158)
 *                           over read_entry_with_context (:502-565), each
 *                           handle copied out (EntryHandle::as_slice) and
 *                           checked (EntryHandle::is_valid_checksum,
 *                           simd-r-drive-entry-handle/src/entry_handle.rs:260-275)
 * "Fetch these n keys into my [n, row_stride] buffer": the look-up of
 * srd_batch_read_hashed_device (d_hashes, the optional tag check against
 * d_verify_hashes, file_len the bound no read crosses: an indexed offset at or
 * above it is NONE) and the verified copy of srd_payload_gather_device in one
 * call whose destination is known by arithmetic: query i's payload goes to
 * d_out[i * row_stride ..).  d_status[i]:
 *   SRD_GATHER_NONE     no such key, removed, tag mismatch, out of range or a
 *                       tombstone: d_len[i] = 0, row i is not written;
 *   SRD_ROWS_TOO_LONG   the payload is longer than row_cap: d_len[i] = its
 *                       true length (the caller can fall back to a call with
 *                       larger rows or to srd_payload_scatter_device), nothing
 *                       of the entry is read but its metadata, row i is not
 *                       written;
 *   SRD_GATHER_OK       delivered, crc32(payload) == the stored checksum;
 *   SRD_GATHER_BAD_CRC  delivered faithfully, the checksum differs;
 * d_len[i] = the payload's length for the last two.  d_crc_computed[i]
 * (nullable) = crc32(payload i), 0 unless delivered.  d_counts (nullable, 6
 * words) is SET to the number of queries per status value 0 .. 5 (3 and 4
 * cannot arise here and stay 0).
 * No byte outside [d_out + i * row_stride, d_out + i * row_stride + d_len[i])
 * of a delivered row is written: no padding, no zero fill (the scatter's rule,
 * not the gather's).  Of a payload nothing outside [start, end) is read, plus
 * its metadata.
 * SRD_ERR_ARG, decided on the host by arithmetic with nothing enqueued: d_out
 * not 16-byte aligned; row_stride not a multiple of 16, or below row_cap;
 * row_cap == 0; n >= 2^31; n * ceil(row_cap / SRD_GATHER_CHUNK) >= 2^32 (the
 * bound on the work units); n * row_stride not fitting 64 bits; [d_out, d_out
 * + n * row_stride) meeting d_file[0 .. srd_padded_size(file_len)); flags != 0;
 * a NULL among the required pointers with n > 0.  n == 0 runs nothing.
 * Ordered on `stream`.  The call DOES NOT WAIT: it reads nothing back, waits
 * for nothing, allocates and frees nothing and makes no synchronous copy once
 * the workspace for (n, row_cap) is there -- after srd_ctx_reserve_rows(ctx, n,
 * row_cap) or any earlier call of at least that n and row_cap -- and returns
 * with everything enqueued: later work on `stream` sees d_out and the output
 * arrays.  So the call can be captured into a graph (hipStreamBeginCapture)
 * and replayed: a replay reads the table, the store and d_hashes as they are
 * then, and is valid while d_table, d_file, the caller's arrays and the
 * workspace are where they were.  If `stream` is capturing and the workspace
 * would have to grow, the call returns SRD_ERR_ARG with a message that names
 * srd_ctx_reserve_rows, before anything is enqueued; outside a capture it
 * grows the workspace as every other entry does (and may wait doing so).  The
 * workspace is this entry's own: no other entry moves it.  One call (or
 * replay) per context may be in flight at a time unless all of them are
 * ordered on one stream.
 *
 * srd_ctx_reserve_rows: the workspace for every later srd_read_rows_device of
 * at most n queries and at most row_cap bytes per row, so that those calls do
 * not wait and can be captured.  What the reserve is for is exactly that; it
 * may synchronise the device, and it moves the workspace when it grows it
 * (which ends the validity of graphs captured before).  SRD_ERR_ARG: n >=
 * 2^31 or a unit bound of 2^32 or more.  srd_ctx_device_bytes counts the
 * workspace. */
#define SRD_ROWS_TOO_LONG 5u /* d_status: the payload is longer than row_cap; d_len holds its length */
int srd_ctx_reserve_rows(srd_ctx *ctx, uint64_t n, uint64_t row_cap);
int srd_read_rows_device(srd_ctx *ctx, const void *d_table, uint64_t table_bytes,
                         const uint8_t *d_file, uint64_t file_len,
                         const uint64_t *d_hashes, const uint64_t *d_verify_hashes /* nullable */,
                         uint64_t n, uint8_t *d_out, uint64_t row_stride, uint64_t row_cap,
                         uint64_t *d_len /* n */, uint8_t *d_status /* n */,
                         uint32_t *d_crc_computed /* n, nullable */,
                         uint64_t *d_counts /* 6, by status value, nullable */,
                         uint32_t flags /* 0 */, void *stream);

/* Synthetic store of the BASELINE configs written on the device (the
 * checksum-on-append writer of data_store.rs:847-939 for keys
 * "bench-key-{i}" and counter-mode splitmix64 payloads).  lens==NULL ->
 * every payload is fixed_len bytes.  Returns the file length in *len_out;
 * d_out==NULL only computes the length. */
int srd_synth_store_device(srd_ctx *ctx, uint8_t *d_out, uint64_t n_entries,
                           uint64_t fixed_len, const uint64_t *lens,
                           uint64_t seed, uint64_t *len_out);

/* The shard [lo, hi) of that synthetic store holding entries
 * [first, first + n) (lens, if given, holds the lengths of entries
 * 0 .. first + n - 1), written into d_span = file bytes [span_off, hi)
 * (span_off a multiple of 16 KiB, <= lo; bytes of earlier entries at or past
 * span_off are written too).  d_span == NULL only computes lo / hi. */
int srd_synth_span_device(srd_ctx *ctx, uint8_t *d_span, uint64_t span_off,
                          uint64_t first, uint64_t n, uint64_t fixed_len,
                          const uint64_t *lens, uint64_t seed,
                          uint64_t *lo_out, uint64_t *hi_out);

/* Library self-test of the CRC algebra tables (host only, no GPU). */
int srd_selftest_host(void);

#ifdef __cplusplus
}
#endif
#endif
