"""Python binding of the MI355X-native validate+index path (include/srd_amd.h).

Mirrors the reference's interface for this path (jzombie/rust-simd-r-drive):

  recover_valid_chain(file)      data_store.rs:383-482  -> final_len
  KeyIndexer.build(file, tail)   key_indexer.rs:98-124   -> {key_hash: packed}
  KeyIndexer.tag_from_hash/pack/unpack                   key_indexer.rs:64-93
  compute_checksum(data)         compute_checksum.rs:15-20 -> 4 LE bytes
  compute_hash(key)              compute_hash.rs:25-27
  compute_hash_batch(keys)       compute_hash.rs:64-77
  DataStore.open(path)           data_store.rs:84-117 (mmap -> recover ->
                                 truncate + re-open -> index), with every chain
                                 payload's CRC verified on the GPU
  EntryHandle.is_valid_checksum  entry_handle.rs:260-275

All compute runs in libsrd_amd.so (HIP, gfx950).  There is no CPU fallback:
if the library or a GPU is missing, calls raise.
"""
from __future__ import annotations

import ctypes as C
import mmap as _mmap
import os
import subprocess
import time

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.environ.get("SRD_LIB_PATH") or os.path.join(HERE, "build", "libsrd_amd.so")  # override: timing tools only

SRD_FLAG_FORCE_FULL = 1
SRD_FLAG_NO_CRC = 2
SRD_FLAG_STAGE_PAGEABLE = 4  # host input: one pageable hipMemcpy (measurement baseline)
SRD_FLAG_STAGE_REGISTER = 8  # host input: hipHostRegister the range (default: pinned bounce buffers)
STAGE_MODES = {0: "pinned input", 1: "registered mapping", 2: "bounce buffers", 3: "pageable copy"}
TIMING_NONE, TIMING_SCAN, TIMING_CALL = 0, 1, 2  # srd_ctx_set_timing levels
SRD_MODE_OPTIMISTIC = 0
SRD_MODE_FULL = 1
SRD_MODE_SPAN_UNPROVEN = 3
# srd_device_result.full_reason (include/srd_amd.h)
SRD_FULL_NONE, SRD_FULL_FORCED, SRD_FULL_SLOT_SPACE, SRD_FULL_WAVES = 0, 1, 2, 3
SRD_FULL_NO_START, SRD_FULL_UNPROVEN, SRD_FULL_CAP, SRD_FULL_LOOKBACK = 4, 5, 6, 7
SRD_ERR_ARG, SRD_ERR_FULL = -3, -5
SCAN_BLOCKS_LAST, SCAN_BLOCKS_NEXT = 0, 1  # srd_ctx_scan_blocks: which partition
SCAN_BLOCKS_EVEN, SCAN_BLOCKS_MEASURED, SCAN_BLOCKS_INSTALLED = 0, 1, 2  # srd_scan_blocks_info.source
SRD_FLAG_MERGE_INDEX = 16  # multi-GPU open: the whole index on ctxs[0] (default: by owner)
SRD_MULTI_COMPOSED, SRD_MULTI_NEIGHBOUR, SRD_MULTI_WHOLE_FILE = 0, 1, 2  # srd_multi_summary.path
SPAN_ALIGN = 16384  # span_off granularity of srd_validate_span_device
METADATA_SIZE = 20
NULL_BYTE = b"\x00"
TAG_BITS = 16
OFFSET_MASK = (1 << 48) - 1

# symbols include/srd_amd.h declares
EXPORTS = [
    "srd_ctx_create", "srd_ctx_destroy", "srd_ctx_stream", "srd_ctx_device_bytes", "srd_ctx_scan_loads",
    "srd_ctx_scan_trial", "srd_ctx_set_scan_blocks", "srd_ctx_scan_blocks",
    "srd_last_error", "srd_build_info",
    "srd_ctx_timings",
    "srd_ctx_set_timing",
    "srd_validate_index_device", "srd_validate_index", "srd_result_free",
    "srd_recover_valid_chain", "srd_key_indexer_build", "srd_crc32_batch",
    "srd_crc32_batch_device", "srd_xxh3_64_batch", "srd_xxh3_64_batch_device",
    "srd_synth_store_device", "srd_selftest_host", "srd_padded_size",
    "srd_validate_span_device", "srd_index_partition_device", "srd_index_build_device",
    "srd_synth_span_device", "srd_batch_layout", "srd_batch_write", "srd_batch_write_device",
    "srd_index_table_bytes", "srd_index_table_build_device", "srd_index_get_packed_device",
    "srd_batch_read_hashed_device", "srd_batch_read",
    "srd_iter_entries_device", "srd_estimate_compaction_savings_device", "srd_compact_device",
    "srd_shard_cuts", "srd_validate_index_multi", "srd_ctx_stage_info", "srd_index_hash_device",
    "srd_validate_index_multi_device", "srd_ctx_multi_summary", "srd_ctx_scan_list", "srd_ctx_set_timing_every",
    "srd_stream_probe_device", "srd_ctx_multi_shard_ms",
    "srd_index_table_apply_device", "srd_index_table_export_device", "srd_batch_delete_hashed_device",
    "srd_payload_gather_device", "srd_batch_append_device", "srd_compact_live_device",
    "srd_batch_append_segments_device", "srd_payload_scatter_device",
    "srd_namespace_hash_batch_device", "srd_namespace_hash_batch", "srd_ttl_resolve_device",
    "srd_ttl_resolve_keys_device", "srd_ttl_evict_device", "srd_ttl_sweep_device",
    "srd_ctx_reserve_rows", "srd_read_rows_device",
]


class DeviceResult(C.Structure):
    _fields_ = [
        ("file_len", C.c_uint64), ("final_len", C.c_uint64), ("n_chain", C.c_uint64),
        ("n_index", C.c_uint64), ("n_crc_bad", C.c_uint64), ("n_candidates", C.c_uint64),
        ("full_reason", C.c_uint64), ("mode", C.c_uint32), ("reserved", C.c_uint32),
        ("meta_off", C.c_void_p), ("key_hash", C.c_void_p), ("prev_offset", C.c_void_p),
        ("payload_start", C.c_void_p), ("payload_len", C.c_void_p),
        ("crc_stored", C.c_void_p), ("crc_computed", C.c_void_p), ("crc_ok", C.c_void_p),
        ("index_key_hash", C.c_void_p), ("index_packed", C.c_void_p),
    ]


class ScanBlocksInfo(C.Structure):
    """srd_scan_blocks_info (include/srd_amd.h)"""
    _fields_ = [("n_spans", C.c_uint64), ("n_blocks", C.c_uint32), ("source", C.c_uint32),
                ("attempts", C.c_uint32), ("first_source", C.c_uint32)]


class MultiSummary(C.Structure):
    """srd_multi_summary (include/srd_amd.h)"""
    _fields_ = [
        ("file_len", C.c_uint64), ("final_len", C.c_uint64), ("n_chain", C.c_uint64),
        ("n_index", C.c_uint64), ("n_crc_bad", C.c_uint64), ("n_candidates", C.c_uint64),
        ("mode", C.c_uint32), ("path", C.c_uint32), ("n_shards", C.c_uint32), ("merged", C.c_uint32),
        ("shard_errors", C.c_uint32), ("peer_errors", C.c_uint32),
        ("validate_ms", C.c_double), ("exchange_ms", C.c_double), ("total_ms", C.c_double),
        ("index_key_hash", C.c_void_p), ("index_packed", C.c_void_p),
    ]


class ApplyStats(C.Structure):
    """srd_index_apply_stats (include/srd_amd.h): per distinct key of the batch"""
    _fields_ = [("n_inserted", C.c_uint64), ("n_updated", C.c_uint64), ("n_removed", C.c_uint64)]

    def as_tuple(self):
        return int(self.n_inserted), int(self.n_updated), int(self.n_removed)


class CompactStats(C.Structure):
    """srd_compact_stats (include/srd_amd.h)"""
    _fields_ = [("n_entries", C.c_uint64), ("new_len", C.c_uint64), ("kept_bytes", C.c_uint64),
                ("n_crc_bad", C.c_uint64), ("first_bad", C.c_uint64)]

    def __repr__(self):
        return "CompactStats(" + ", ".join(f"{n}={int(getattr(self, n))}" for n, _ in self._fields_) + ")"


class TtlSweepStats(C.Structure):
    """srd_ttl_sweep_stats (include/srd_amd.h)"""
    _fields_ = [("n_judged", C.c_uint64), ("n_expired", C.c_uint64), ("n_short", C.c_uint64),
                ("next_expiry", C.c_uint64)]

    def __repr__(self):
        return "TtlSweepStats(" + ", ".join(f"{n}={int(getattr(self, n))}" for n, _ in self._fields_) + ")"


class Segment(C.Structure):
    """srd_segment (include/srd_amd.h): the bytes sources[src][off : off + len]
    (srd_payload_scatter_device: of its destination table)"""
    _fields_ = [("src", C.c_uint32), ("reserved", C.c_uint32), ("off", C.c_uint64), ("len", C.c_uint64)]


def build_info() -> str:
    """srd_build_info(): the sha256 of the sources the loaded library was
    compiled from (equal to src_hash.source_hash(), or lib() refused it)."""
    return lib().srd_build_info().decode()


def build() -> str:
    """Compile the HIP library in-tree (hipcc --offload-arch=gfx950)."""
    subprocess.check_call(["make", "-s", "-C", HERE])
    return LIB_PATH


_lib = None


def lib():
    global _lib
    if _lib is None:
        if not os.path.exists(LIB_PATH):
            raise RuntimeError(f"{LIB_PATH} missing: run `make -C {HERE}` (no CPU fallback exists)")
        # One HIP runtime per process: if PyTorch is present, load it first so
        # that libsrd_amd.so binds to the libamdhip64.so.7 torch already mapped
        # (torch NEEDs "libamdhip64.so", we NEED the soname "libamdhip64.so.7";
        # loading us first would map a second runtime from /opt/rocm).
        try:
            import torch  # noqa: F401
        except Exception:
            pass
        L = C.CDLL(LIB_PATH)
        vp, u64, u32, i32 = C.c_void_p, C.c_uint64, C.c_uint32, C.c_int
        L.srd_build_info.restype = C.c_char_p
        L.srd_ctx_device_bytes.argtypes = [vp]
        L.srd_ctx_device_bytes.restype = u64
        L.srd_ctx_scan_loads.argtypes = [vp]
        L.srd_ctx_scan_trial.argtypes = [vp, C.POINTER(C.c_double)]
        L.srd_ctx_set_scan_blocks.argtypes = [vp, vp, u32, u64]
        L.srd_ctx_scan_blocks.argtypes = [vp, i32, vp, u32, C.POINTER(ScanBlocksInfo)]
        if not os.environ.get("SRD_LIB_PATH"):  # (timing tools load variant builds by path)
            import importlib.util
            spec = importlib.util.spec_from_file_location("srd_src_hash", os.path.join(HERE, "src_hash.py"))
            sh = importlib.util.module_from_spec(spec)
            spec.loader.exec_module(sh)
            want, got = sh.source_hash(), L.srd_build_info().decode()
            if got != want:
                raise RuntimeError(f"{LIB_PATH} was built from other sources (sha256 {got}, the sources here "
                                   f"{want}): run `make -C {HERE}`")
        L.srd_ctx_create.argtypes = [i32, C.POINTER(vp)]
        L.srd_ctx_destroy.argtypes = [vp]
        L.srd_ctx_stream.argtypes = [vp]
        L.srd_ctx_stream.restype = vp
        L.srd_last_error.restype = C.c_char_p
        L.srd_ctx_timings.argtypes = [vp, C.POINTER(C.c_double), C.POINTER(C.c_int), C.POINTER(C.c_double)]
        L.srd_ctx_set_timing.argtypes = [vp, C.c_int]
        L.srd_ctx_scan_list.argtypes = [vp, C.POINTER(C.c_float), C.c_int]
        L.srd_ctx_set_timing_every.argtypes = [vp, C.c_int]
        L.srd_validate_index_device.argtypes = [vp, vp, u64, u32, C.POINTER(DeviceResult)]
        L.srd_validate_index.argtypes = [vp, vp, u64, u32, C.POINTER(DeviceResult)]
        L.srd_result_free.argtypes = [C.POINTER(DeviceResult)]
        L.srd_recover_valid_chain.argtypes = [vp, vp, u64, C.POINTER(u64)]
        L.srd_key_indexer_build.argtypes = [vp, vp, u64, vp, vp, u64, C.POINTER(u64)]
        L.srd_crc32_batch.argtypes = [vp, vp, u64, vp, vp, u64, vp]
        L.srd_crc32_batch_device.argtypes = [vp, vp, vp, vp, u64, vp, vp]
        L.srd_xxh3_64_batch.argtypes = [vp, vp, u64, vp, vp, u64, vp]
        L.srd_xxh3_64_batch_device.argtypes = [vp, vp, vp, vp, u64, vp, vp]
        L.srd_padded_size.argtypes = [u64]
        L.srd_padded_size.restype = u64
        L.srd_synth_store_device.argtypes = [vp, vp, u64, u64, vp, u64, C.POINTER(u64)]
        L.srd_validate_span_device.argtypes = [vp, vp, u64, u64, u64, u32, C.POINTER(DeviceResult)]
        L.srd_shard_cuts.argtypes = [vp, u64, u32, vp]
        L.srd_index_partition_device.argtypes = [vp, vp, vp, u64, u32, vp, vp]
        L.srd_index_build_device.argtypes = [vp, vp, u64, vp, vp, C.POINTER(u64)]
        L.srd_synth_span_device.argtypes = [vp, vp, u64, u64, u64, u64, vp, u64, C.POINTER(u64), C.POINTER(u64)]
        L.srd_batch_layout.argtypes = [u64, vp, vp, vp, vp, vp, u64, u32, vp, C.POINTER(u64)]
        L.srd_batch_write.argtypes = [vp, u64, vp, vp, vp, vp, vp, vp, u64, u32, vp, u64, C.POINTER(u64), vp, vp]
        L.srd_batch_write_device.argtypes = [vp, vp, vp, vp, u64, vp, u64, vp, vp, vp]
        L.srd_index_table_bytes.argtypes = [u64]
        L.srd_index_table_bytes.restype = u64
        L.srd_index_table_build_device.argtypes = [vp, vp, vp, u64, vp, u64]
        L.srd_index_get_packed_device.argtypes = [vp, vp, u64, vp, u64, vp, vp]
        L.srd_batch_read_hashed_device.argtypes = [vp, vp, u64, vp, u64, vp, vp, u64, vp, vp, vp]
        L.srd_batch_read.argtypes = [vp, vp, u64, vp, u64, vp, vp, vp, u64, vp, vp]
        L.srd_index_table_apply_device.argtypes = [vp, vp, u64, C.POINTER(u64), vp, vp, vp, u64,
                                                   C.POINTER(ApplyStats), vp]
        L.srd_index_table_export_device.argtypes = [vp, vp, u64, vp, vp, u64, C.POINTER(u64)]
        L.srd_batch_delete_hashed_device.argtypes = [vp, vp, u64, C.POINTER(u64), vp, u64, u64, vp, u64,
                                                     C.POINTER(u64), C.POINTER(u64)]
        L.srd_payload_gather_device.argtypes = [vp, vp, u64, vp, vp, u64, u32, vp, u64, vp, vp, vp,
                                                C.POINTER(u64), vp]
        L.srd_batch_append_device.argtypes = [vp, vp, u64, vp, vp, vp, u64, u32, u64, vp, u64, C.POINTER(u64), vp, vp]
        L.srd_batch_append_segments_device.argtypes = [vp, C.POINTER(vp), C.POINTER(u64), u64, vp, u64, vp, vp, u64, u32,
                                                       u64, vp, u64, C.POINTER(u64), vp, vp]
        L.srd_payload_scatter_device.argtypes = [vp, vp, u64, vp, vp, u64, C.POINTER(vp), C.POINTER(u64), u64, vp, u64,
                                                 vp, u32, vp, vp, vp]
        L.srd_compact_live_device.argtypes = [vp, vp, u64, vp, u64, vp, u64, vp, u64, C.POINTER(CompactStats)]
        L.srd_namespace_hash_batch_device.argtypes = [vp, u64, vp, vp, vp, u64, vp, vp, vp]
        L.srd_namespace_hash_batch.argtypes = [vp, u64, vp, u64, vp, vp, u64, vp, vp]
        L.srd_ttl_resolve_device.argtypes = [vp, vp, u64, vp, u64, vp, u64, u64, vp, vp, vp, vp, vp, vp]
        L.srd_ttl_resolve_keys_device.argtypes = [vp, vp, u64, vp, u64, u64, vp, vp, vp, u64, u64, vp, vp, vp, vp, vp,
                                                  vp, vp]
        L.srd_ttl_evict_device.argtypes = [vp, vp, u64, C.POINTER(u64), vp, vp, u64, u64, vp, u64, C.POINTER(u64),
                                           C.POINTER(u64)]
        L.srd_ttl_sweep_device.argtypes = [vp, vp, u64, C.POINTER(u64), vp, u64, u64, u64, u32, C.POINTER(u64),
                                           C.POINTER(TtlSweepStats)]
        L.srd_ctx_reserve_rows.argtypes = [vp, u64, u64]
        L.srd_read_rows_device.argtypes = [vp, vp, u64, vp, u64, vp, vp, u64, vp, u64, u64, vp, vp, vp, vp, u32, vp]
        L.srd_iter_entries_device.argtypes = [vp, vp, u64, vp, u64, vp, vp, vp, vp, C.POINTER(u64)]
        L.srd_estimate_compaction_savings_device.argtypes = [vp, vp, u64, vp, u64, C.POINTER(u64)]
        L.srd_compact_device.argtypes = [vp, vp, u64, vp, u64, vp, u64, C.POINTER(u64), vp, vp]
        L.srd_validate_index_multi.argtypes = [C.POINTER(vp), u32, vp, u64, u32, C.POINTER(DeviceResult)]
        L.srd_ctx_stage_info.argtypes = [vp, C.POINTER(i32), C.POINTER(C.c_double)]
        L.srd_index_hash_device.argtypes = [vp, vp, u64, vp, vp]
        L.srd_validate_index_multi_device.argtypes = [C.POINTER(vp), u32, C.POINTER(vp), vp, vp, u32,
                                                      C.POINTER(DeviceResult), C.POINTER(MultiSummary)]
        L.srd_ctx_multi_summary.argtypes = [vp, C.POINTER(MultiSummary)]
        L.srd_ctx_multi_shard_ms.argtypes = [vp, C.POINTER(C.c_double), i32]
        L.srd_stream_probe_device.argtypes = [vp, vp, u64, i32, C.POINTER(C.c_double), C.POINTER(C.c_double)]
        for f in EXPORTS:
            if f not in ("srd_ctx_destroy", "srd_result_free", "srd_ctx_stream", "srd_ctx_device_bytes", "srd_last_error",
                         "srd_build_info",
                         "srd_padded_size", "srd_index_table_bytes"):
                getattr(L, f).restype = i32
        _lib = L
    return _lib


class WriteEntry(C.Structure):
    """srd_write_entry (include/srd_amd.h)"""
    _fields_ = [("src", C.c_uint64), ("len", C.c_uint64), ("key_src", C.c_uint64), ("tail", C.c_uint64),
                ("key_len", C.c_uint32), ("flags", C.c_uint32)]


WRITE_ALLOW_NULL = 1


class SrdError(RuntimeError):
    pass


def _check(rc):
    if rc != 0:
        raise SrdError(f"srd error {rc}: {lib().srd_last_error().decode()}")


class Context:
    """One GPU + stream + reusable HBM workspace (srd_ctx)."""

    def __init__(self, device: int = 0):
        self.device = device
        self.h = C.c_void_p()
        _check(lib().srd_ctx_create(device, C.byref(self.h)))

    def close(self):
        if self.h:
            lib().srd_ctx_destroy(self.h)
            self.h = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def set_timing(self, level: int):
        """HIP-event timing level: TIMING_NONE (default), TIMING_SCAN, TIMING_CALL."""
        _check(lib().srd_ctx_set_timing(self.h, level))

    def set_timing_every(self, n: int):
        """With TIMING_SCAN: stamp only every n-th scan launch (srd_ctx_set_timing_every)."""
        _check(lib().srd_ctx_set_timing_every(self.h, n))

    def reserve_rows(self, n: int, row_cap: int) -> None:
        """srd_ctx_reserve_rows: the workspace for every later rows read of at most
        n queries and row_cap bytes per row, so that those reads wait for nothing
        and can be captured into a graph.  May synchronise."""
        _check(lib().srd_ctx_reserve_rows(self.h, n, row_cap))

    def device_bytes(self) -> int:
        """srd_ctx_device_bytes: the context's device workspace (+ staging copy)."""
        return int(lib().srd_ctx_device_bytes(self.h))

    def scan_loads(self) -> int:
        """srd_ctx_scan_loads: 0 coalesced, 1 line per lane, -1 none yet."""
        return int(lib().srd_ctx_scan_loads(self.h))

    def scan_trial(self):
        """srd_ctx_scan_trial: (choice, best coalesced ms, best line-per-lane ms); choice -1 = still measuring."""
        ms = (C.c_double * 2)()
        ch = int(lib().srd_ctx_scan_trial(self.h, ms))
        return ch, float(ms[0]), float(ms[1])

    def set_scan_blocks(self, starts, n_spans: int):
        """srd_ctx_set_scan_blocks: install starts[0..n_blocks] as the block-start table of the next
        optimistic scan (diagnostics); SrdError (SRD_ERR_ARG) outside the table domain or with the shares off."""
        st = np.ascontiguousarray(starts, dtype=np.uint64)
        _check(lib().srd_ctx_set_scan_blocks(self.h, C.c_void_p(st.ctypes.data), max(st.size, 1) - 1, n_spans))

    def scan_blocks(self, which: int = SCAN_BLOCKS_LAST):
        """srd_ctx_scan_blocks: (starts [n_blocks + 1] u64, ScanBlocksInfo) of the partition the last optimistic
        scan ran with (SCAN_BLOCKS_LAST) or of the table prepared for the next one (SCAN_BLOCKS_NEXT);
        info.n_blocks == 0 and no starts: none."""
        info = ScanBlocksInfo()
        _check(lib().srd_ctx_scan_blocks(self.h, which, None, 0, C.byref(info)))
        st = np.zeros(info.n_blocks + 1 if info.n_blocks else 0, np.uint64)
        if st.size:
            _check(lib().srd_ctx_scan_blocks(self.h, which, C.c_void_p(st.ctypes.data), st.size, C.byref(info)))
        return st, info

    def timings(self):
        """(scan_ms, scan_launches) summed over the validate calls since the last
        read, and total_ms of the last call (HIP events; srd_ctx_timings)."""
        a, n, b = C.c_double(), C.c_int(), C.c_double()
        _check(lib().srd_ctx_timings(self.h, C.byref(a), C.byref(n), C.byref(b)))
        return a.value, n.value, b.value

    def scan_list(self) -> list[float]:
        """The individual scan durations (ms) behind the last timings() read."""
        n = lib().srd_ctx_scan_list(self.h, None, 0)
        if n < 0:
            _check(n)
        buf = (C.c_float * max(n, 1))()
        lib().srd_ctx_scan_list(self.h, buf, n)
        return list(buf[:n])

    @property
    def stream(self) -> int:
        return lib().srd_ctx_stream(self.h)

    def stage_info(self) -> tuple[str, float]:
        """(how the last host-input call staged the store (STAGE_MODES), its host wall ms)."""
        m, ms = C.c_int(), C.c_double()
        _check(lib().srd_ctx_stage_info(self.h, C.byref(m), C.byref(ms)))
        return STAGE_MODES.get(m.value, "none"), ms.value

    def stage_mode(self) -> str:
        return self.stage_info()[0]

    def multi_summary(self) -> MultiSummary:
        """srd_multi_summary of the last multi-GPU open with this context as ctxs[0]."""
        m = MultiSummary()
        _check(lib().srd_ctx_multi_summary(self.h, C.byref(m)))
        return m


_default_ctx = None


def default_ctx() -> Context:
    global _default_ctx
    if _default_ctx is None:
        _default_ctx = Context(int(os.environ.get("SRD_DEVICE", "0")))
    return _default_ctx


def _u8(file) -> np.ndarray:
    if isinstance(file, np.ndarray):
        return np.ascontiguousarray(file, dtype=np.uint8).reshape(-1)
    return np.frombuffer(memoryview(file), dtype=np.uint8)


def _ptr(a: np.ndarray):
    return C.c_void_p(a.ctypes.data) if a.size else C.c_void_p(0)


class Result:
    """Host copy of srd_result: the recovered tail, the chain and the index."""

    def __init__(self, r: DeviceResult):
        self.file_len = r.file_len
        self.final_len = r.final_len
        self.n_chain = r.n_chain
        self.n_index = r.n_index
        self.n_crc_bad = r.n_crc_bad
        self.n_candidates = r.n_candidates
        self.full_reason = r.full_reason
        self.mode = r.mode

        def arr(p, n, dt):
            if n == 0 or not p:
                return np.zeros(0, dt)
            return np.ctypeslib.as_array(C.cast(p, C.POINTER(np.ctypeslib.as_ctypes_type(dt))), (n,)).copy()

        n, ni = r.n_chain, r.n_index
        self.meta_off = arr(r.meta_off, n, np.uint64)
        self.key_hash = arr(r.key_hash, n, np.uint64)
        self.prev_offset = arr(r.prev_offset, n, np.uint64)
        self.payload_start = arr(r.payload_start, n, np.uint64)
        self.payload_len = arr(r.payload_len, n, np.uint64)
        self.crc_stored = arr(r.crc_stored, n, np.uint32)
        self.crc_computed = arr(r.crc_computed, n, np.uint32)
        self.crc_ok = arr(r.crc_ok, n, np.uint8)
        self.index_key_hash = arr(r.index_key_hash, ni, np.uint64)
        self.index_packed = arr(r.index_packed, ni, np.uint64)

    def index(self) -> dict[int, int]:
        return {int(k): int(v) for k, v in zip(self.index_key_hash, self.index_packed)}

    def chain(self) -> list[dict]:
        keys = ["meta_off", "key_hash", "prev_offset", "payload_start", "payload_len",
                "crc_stored", "crc_computed", "crc_ok"]
        return [{k: int(getattr(self, k)[i]) for k in keys} for i in range(self.n_chain)]


def validate_index(file, flags: int = 0, ctx: Context | None = None) -> Result:
    """The fused open-time pass: recover_valid_chain + KeyIndexer::build +
    is_valid_checksum over every chain entry, on the GPU."""
    ctx = ctx or default_ctx()
    a = _u8(file)
    r = DeviceResult()
    _check(lib().srd_validate_index(ctx.h, _ptr(a), a.size, flags, C.byref(r)))
    try:
        return Result(r)
    finally:
        lib().srd_result_free(C.byref(r))


def validate_index_call(file, flags: int = 0, ctx: Context | None = None) -> DeviceResult:
    """srd_validate_index alone: the result's arrays stay in the context-owned
    pinned host buffers (valid until the next call on ctx; `Result(r)` copies
    them into numpy).  The end-to-end timing of the library call."""
    ctx = ctx or default_ctx()
    a = _u8(file)
    r = DeviceResult()
    _check(lib().srd_validate_index(ctx.h, _ptr(a), a.size, flags, C.byref(r)))
    return r


def validate_index_multi(file, ctxs, flags: int = 0) -> Result:
    """DataStore::open's pass over one host store on len(ctxs) GPUs in one
    process (srd_validate_index_multi): entry-range shards, host composition,
    index merged latest-wins on ctxs[0]'s device; no RCCL.  Same result as
    validate_index."""
    a = _u8(file)
    hs = (C.c_void_p * len(ctxs))(*[c.h.value for c in ctxs])
    r = DeviceResult()
    _check(lib().srd_validate_index_multi(hs, len(ctxs), _ptr(a), a.size, flags, C.byref(r)))
    try:
        return Result(r)
    finally:
        lib().srd_result_free(C.byref(r))


def validate_index_multi_device(ctxs, spans, span_offs, cuts, flags: int = 0):
    """DataStore::open of a store resident in the HBM of len(ctxs) GPUs, one
    entry-range shard per context (srd_validate_index_multi_device; no RCCL):
    spans[i] = device pointer of file byte span_offs[i] .. cuts[i+1] on
    ctxs[i]'s GPU (0 for an empty shard).  Returns (shard results -- chain
    segment i and, by default, the index part owned by i, device arrays on
    ctxs[i]'s GPU --, MultiSummary)."""
    n = len(ctxs)
    hs = (C.c_void_p * n)(*[c.h.value for c in ctxs])
    sp = (C.c_void_p * n)(*[int(x or 0) for x in spans])
    so = np.ascontiguousarray(span_offs, np.uint64)
    cu = np.ascontiguousarray(cuts, np.uint64)
    assert so.size == n and cu.size == n + 1
    res = (DeviceResult * n)()
    summ = MultiSummary()
    _check(lib().srd_validate_index_multi_device(hs, n, sp, _ptr(so), _ptr(cu), flags, res, C.byref(summ)))
    return list(res), summ


def index_hash_device(d_keys: int, n: int, d_out: int, ctx: Context | None = None) -> None:
    """xxh3_64(le8(k)) per key on the device (the KeyIndexer's Xxh3BuildHasher)."""
    ctx = ctx or default_ctx()
    _check(lib().srd_index_hash_device(ctx.h, C.c_void_p(d_keys), n, C.c_void_p(d_out), C.c_void_p(ctx.stream)))


def validate_index_device(d_ptr: int, file_len: int, flags: int = 0, ctx: Context | None = None) -> DeviceResult:
    """Device-resident variant: d_ptr is a device pointer (e.g. a torch
    uint8 CUDA tensor's data_ptr()).  Result arrays stay in HBM."""
    ctx = ctx or default_ctx()
    r = DeviceResult()
    _check(lib().srd_validate_index_device(ctx.h, C.c_void_p(d_ptr), file_len, flags, C.byref(r)))
    return r


class _DevView:
    def __init__(self, ptr: int, n: int, typestr: str):
        self.__cuda_array_interface__ = {"shape": (n,), "typestr": typestr, "data": (ptr, False), "version": 3}


_TYPESTR = {np.uint64: "<i8", np.uint32: "<i4", np.uint8: "|u1"}


def device_view(ptr: int, n: int, dtype=np.uint64, device: int = 0):
    """Zero-copy torch view of n elements of a library-owned device array
    (result arrays of the *_device calls; int64/int32/uint8 bit patterns)."""
    import torch
    if n == 0 or not ptr:
        return torch.empty(0, dtype={np.uint64: torch.int64, np.uint32: torch.int32, np.uint8: torch.uint8}[dtype],
                           device=f"cuda:{device}")
    return torch.as_tensor(_DevView(ptr, n, _TYPESTR[dtype]), device=f"cuda:{device}")


def device_to_numpy(ptr: int, n: int, dtype=np.uint64) -> np.ndarray:
    return device_view(ptr, n, dtype).cpu().numpy().view(dtype).copy()


def validate_span_device(d_ptr: int, span_off: int, lo: int, hi: int, flags: int = 0,
                         ctx: Context | None = None) -> DeviceResult:
    """Entry-range shard [lo, hi) of a store, resident at d_ptr = file byte
    span_off (srd_validate_span_device).  mode == SRD_MODE_SPAN_UNPROVEN means
    the caller must use the whole-file path."""
    ctx = ctx or default_ctx()
    r = DeviceResult()
    _check(lib().srd_validate_span_device(ctx.h, C.c_void_p(d_ptr), span_off, lo, hi, flags, C.byref(r)))
    return r


def index_partition_device(d_keys: int, d_vals: int, n: int, world: int, d_out_pairs: int,
                           ctx: Context | None = None) -> list[int]:
    """Group n device (key_hash, value) pairs by owner rank into interleaved
    pairs at d_out_pairs; returns the per-owner counts."""
    ctx = ctx or default_ctx()
    counts = np.zeros(max(world, 1), np.uint64)
    _check(lib().srd_index_partition_device(ctx.h, C.c_void_p(d_keys), C.c_void_p(d_vals), n, world,
                                            C.c_void_p(d_out_pairs), _ptr(counts)))
    return [int(x) for x in counts[:world]]


def index_build_device(d_pairs: int, n: int, d_out_keys: int, d_out_packed: int,
                       ctx: Context | None = None) -> int:
    """KeyIndexer::build over n interleaved device (key_hash, offset) pairs in
    file order; returns the index size."""
    ctx = ctx or default_ctx()
    out = C.c_uint64()
    _check(lib().srd_index_build_device(ctx.h, C.c_void_p(d_pairs), n, C.c_void_p(d_out_keys),
                                        C.c_void_p(d_out_packed), C.byref(out)))
    return out.value


def synth_span(d_ptr: int | None, span_off: int, first: int, n: int, payload_len: int = 4096, lens=None,
               seed: int = 0x5EED0001, ctx: Context | None = None) -> tuple[int, int]:
    """Shard of the synthetic store holding entries [first, first+n): returns
    (lo, hi); writes file bytes [span_off, hi) at d_ptr when given."""
    lo, hi = C.c_uint64(), C.c_uint64()
    lp = None
    if lens is not None:
        lens = np.ascontiguousarray(lens, np.uint64)
        lp = _ptr(lens)
    h = (ctx or default_ctx()).h if d_ptr else C.c_void_p(0)
    _check(lib().srd_synth_span_device(h, C.c_void_p(d_ptr or 0), span_off, first, n, payload_len, lp, seed,
                                       C.byref(lo), C.byref(hi)))
    return lo.value, hi.value


def recover_valid_chain(file, ctx: Context | None = None) -> int:
    """data_store.rs:383-482: the largest valid tail <= file_len (0 if none)."""
    ctx = ctx or default_ctx()
    a = _u8(file)
    out = C.c_uint64()
    _check(lib().srd_recover_valid_chain(ctx.h, _ptr(a), a.size, C.byref(out)))
    return out.value


def compute_hash_batch(keys, ctx: Context | None = None) -> list[int]:
    """compute_hash.rs:64-77"""
    ctx = ctx or default_ctx()
    keys = [bytes(k) for k in keys]
    buf = np.frombuffer(b"".join(keys) or b"\x00", np.uint8)
    lens = np.array([len(k) for k in keys], np.uint64)
    offs = np.zeros(len(keys), np.uint64)
    if len(keys) > 1:
        offs[1:] = np.cumsum(lens)[:-1]
    out = np.zeros(max(len(keys), 1), np.uint64)
    _check(lib().srd_xxh3_64_batch(ctx.h, _ptr(buf), buf.size, _ptr(offs), _ptr(lens), len(keys), _ptr(out)))
    return [int(x) for x in out[: len(keys)]]


def compute_hash(key: bytes) -> int:
    """compute_hash.rs:25-27"""
    return compute_hash_batch([key])[0]


def crc32_batch(buf, offs, lens, ctx: Context | None = None) -> np.ndarray:
    ctx = ctx or default_ctx()
    a = _u8(buf)
    offs = np.ascontiguousarray(offs, np.uint64)
    lens = np.ascontiguousarray(lens, np.uint64)
    out = np.zeros(max(len(offs), 1), np.uint32)
    _check(lib().srd_crc32_batch(ctx.h, _ptr(a), a.size, _ptr(offs), _ptr(lens), len(offs), _ptr(out)))
    return out[: len(offs)]


def compute_checksum(data: bytes) -> bytes:
    """compute_checksum.rs:15-20: CRC-32 as 4 little-endian bytes."""
    d = bytes(data)
    v = int(crc32_batch(np.frombuffer(d or b"\x00", np.uint8), [0], [len(d)])[0])
    return v.to_bytes(4, "little")


# ---------------------------------------------------------------------------
# The TTL cache's keys (extensions/src/storage_cache_ext.rs:23-107 over
# src/utils/namespace_hasher.rs:33-65)

TTL_PREFIX = bytes([0xF7, 0x74, 0x74, 0x6C, 0xFD])  # extensions/src/constants.rs:20-42
TTL_NOT_FOUND, TTL_LIVE, TTL_EXPIRED, TTL_TOO_SHORT = 0, 1, 2, 3  # SRD_TTL_*
TTL_SWEEP_PLAN = 1  # SRD_TTL_SWEEP_PLAN
U64_MAX = (1 << 64) - 1


class NamespaceHasher:
    """NamespaceHasher (namespace_hasher.rs:33-65): `prefix` is hashed once; the
    namespaced key of `key` is the 16 bytes le64(xxh3_64(prefix)) ||
    le64(xxh3_64(key)).  Both hashes run on the device."""

    def __init__(self, prefix: bytes, ctx: Context | None = None):
        self.ctx = ctx or default_ctx()
        self.prefix = bytes(prefix)
        self.prefix_hash = compute_hash_batch([self.prefix], self.ctx)[0]

    def _batch(self, keys, want_ns: bool):
        buf, offs, lens = _blob(keys)
        n = len(lens)
        out = np.zeros(max(n, 1), np.uint64)
        ns = np.zeros(16 * max(n, 1), np.uint8) if want_ns else None
        _check(lib().srd_namespace_hash_batch(self.ctx.h, self.prefix_hash, _ptr(buf), buf.size if n else 0, _ptr(offs),
                                              _ptr(lens), n, _ptr(ns) if want_ns else None, _ptr(out)))
        return ns, out[:n]

    def namespace(self, key: bytes) -> bytes:
        """namespace_hasher.rs:52-64: the 16-byte namespaced key."""
        return self._batch([key], True)[0].tobytes()

    def hash_batch(self, keys) -> list[int]:
        """compute_hash_batch of the keys' namespaced keys: the hashes their entries are stored under."""
        return [int(x) for x in self._batch(keys, False)[1]]


class KeyIndexer:
    """key_indexer.rs: key_hash -> (tag16 << 48 | offset48).  Array-backed
    (the validate pass's index arrays, sorted by key_hash for lookups), so
    that adopting a million-key index costs a sort, not a Python dict."""

    def __init__(self, index: dict[int, int] | None = None, keys=None, packed=None):
        if index is not None:
            keys = np.fromiter(index.keys(), np.uint64, len(index))
            packed = np.fromiter(index.values(), np.uint64, len(index))
        keys = np.zeros(0, np.uint64) if keys is None else np.asarray(keys, np.uint64)
        packed = np.zeros(0, np.uint64) if packed is None else np.asarray(packed, np.uint64)
        o = np.argsort(keys, kind="stable")
        self._keys, self._packed = keys[o], packed[o]

    @classmethod
    def from_arrays(cls, keys: np.ndarray, packed: np.ndarray) -> "KeyIndexer":
        return cls(keys=keys, packed=packed)

    @property
    def index(self) -> dict[int, int]:
        return {int(k): int(v) for k, v in zip(self._keys, self._packed)}

    @staticmethod
    def tag_from_hash(key_hash: int) -> int:
        return key_hash >> (64 - TAG_BITS)

    @staticmethod
    def pack(tag: int, offset: int) -> int:
        return (tag << (64 - TAG_BITS)) | offset

    @staticmethod
    def unpack(packed: int) -> tuple[int, int]:
        return packed >> (64 - TAG_BITS), packed & OFFSET_MASK

    @classmethod
    def build(cls, file, tail: int, ctx: Context | None = None) -> "KeyIndexer":
        ctx = ctx or default_ctx()
        a = _u8(file)
        cap = max(1, tail // METADATA_SIZE + 1)
        k = np.zeros(cap, np.uint64)
        v = np.zeros(cap, np.uint64)
        n = C.c_uint64()
        _check(lib().srd_key_indexer_build(ctx.h, _ptr(a), tail, _ptr(k), _ptr(v), cap, C.byref(n)))
        return cls(keys=k[: n.value], packed=v[: n.value])

    def get_packed(self, key_hash: int):
        i = int(np.searchsorted(self._keys, np.uint64(key_hash)))
        if i < self._keys.size and int(self._keys[i]) == key_hash:
            return int(self._packed[i])
        return None

    def get_offset(self, key_hash: int):
        p = self.get_packed(key_hash)
        return None if p is None else p & OFFSET_MASK

    def __len__(self):
        return int(self._keys.size)


class EntryHandle:
    def __init__(self, store: "DataStore", i: int):
        self.store, self.i = store, i
        r = store.result
        self.metadata_offset = int(r.meta_off[i])
        self.start_offset = int(r.payload_start[i])
        self.end_offset = self.metadata_offset
        self.key_hash = int(r.key_hash[i])

    def as_slice(self) -> bytes:
        return bytes(self.store.mm[self.start_offset:self.end_offset])

    def checksum(self) -> int:
        return int(self.store.result.crc_stored[self.i])

    def is_valid_checksum(self) -> bool:
        """entry_handle.rs:260-275, computed on the GPU during open."""
        return bool(self.store.result.crc_ok[self.i])


class DataStore:
    """The part of DataStore::open (data_store.rs:84-117) this path replaces."""

    def __init__(self, path, mm, result: Result):
        self.path, self.mm, self.result = path, mm, result
        self.tail_offset = result.final_len
        self.key_indexer = KeyIndexer.from_arrays(result.index_key_hash, result.index_packed)

    @classmethod
    def open(cls, path, ctx: Context | None = None, ctxs=None, flags: int = 0) -> "DataStore":
        """ctxs: contexts of several GPUs (one process, srd_validate_index_multi);
        otherwise ctx (default: the default context).  The mapping is handed to
        the library as is; it stages it (registered mapping or bounce buffers)."""
        with open(path, "a+b"):
            pass
        size = os.path.getsize(path)
        with open(path, "r+b") as f:
            mm = _mmap.mmap(f.fileno(), 0, access=_mmap.ACCESS_READ) if size else b""
            view = np.frombuffer(mm, np.uint8) if size else b""
            if ctxs and len(ctxs) > 1:
                res = validate_index_multi(view, ctxs, flags)
            else:
                res = validate_index(view, flags, ctx=(ctxs[0] if ctxs else ctx))
            del view
        if res.final_len < size:
            # data_store.rs:91-104: warn, truncate to the valid tail, re-open
            import warnings
            warnings.warn(f"Truncating corrupted data in {path} from offset {res.final_len} to {size}.")
            if size and hasattr(mm, "close"):
                mm.close()
            with open(path, "r+b") as f:
                f.truncate(res.final_len)
                os.fsync(f.fileno())
            return cls.open(path, ctx, ctxs, flags)
        return cls(path, mm, res)

    def read_entry(self, key_hash: int):
        packed = self.key_indexer.get_packed(key_hash)
        if packed is None:
            return None
        tag, off = KeyIndexer.unpack(packed)
        if tag != KeyIndexer.tag_from_hash(key_hash):
            return None
        i = int(np.searchsorted(self.result.meta_off, np.uint64(off)))  # the chain is in file order
        if int(self.result.payload_len[i]) == 1 and self.mm[int(self.result.payload_start[i])] == 0:
            return None  # tombstone
        return EntryHandle(self, i)

    def read(self, key: bytes):
        return self.read_entry(compute_hash(key))

    def len(self) -> int:
        return len(self.key_indexer)


def shard_cuts(file: np.ndarray, world: int) -> list[int]:
    """Entry-tail cuts [0, c_1, .., file_len] splitting a host store into
    `world` byte-balanced entry ranges (host pre-pass, srd_shard_cuts)."""
    f = np.ascontiguousarray(file, dtype=np.uint8)
    cuts = np.zeros(world + 1, np.uint64)
    _check(lib().srd_shard_cuts(f.ctypes.data, f.size, world, cuts.ctypes.data))
    return [int(x) for x in cuts]


def padded_size(file_len: int) -> int:
    """Bytes a device buffer for validate_index_device must be readable for."""
    return int(lib().srd_padded_size(file_len))


def zipf_lens(n: int, seed: int = 0x5EED0003, s: float = 2.0) -> np.ndarray:
    """C3 payload sizes: 2^k bytes, k = 6..20, Zipf over
    rank k - 5 with exponent s; L = 2^k - j, j uniform in [0, 63], for k >= 7."""
    rng = np.random.default_rng(seed)
    r = np.arange(1, 16)
    p = 1.0 / r ** s
    p /= p.sum()
    k = rng.choice(np.arange(6, 21), size=n, p=p)
    j = rng.integers(0, 64, size=n)
    return ((1 << k) - np.where(k >= 7, j, 0)).astype(np.uint64)


def synth_store_len(n_entries: int, payload_len: int = 4096, lens=None) -> int:
    out = C.c_uint64()
    lp = None
    if lens is not None:
        lens = np.ascontiguousarray(lens, np.uint64)
        lp = _ptr(lens)
    _check(lib().srd_synth_store_device(C.c_void_p(0), None, n_entries, payload_len, lp, 0, C.byref(out)))
    return out.value


def synth_store_device(d_ptr: int, n_entries: int, payload_len: int = 4096, lens=None,
                       seed: int = 0x5EED0001, ctx: Context | None = None) -> int:
    ctx = ctx or default_ctx()
    out = C.c_uint64()
    lp = None
    if lens is not None:
        lens = np.ascontiguousarray(lens, np.uint64)
        lp = _ptr(lens)
    _check(lib().srd_synth_store_device(ctx.h, C.c_void_p(d_ptr), n_entries, payload_len, lp, seed, C.byref(out)))
    return out.value


# ---------------------------------------------------------------------------
# DataStoreWriter::batch_write (data_store.rs:838-939) -- the checksum-on-append
# writer (BASELINE config C5)

def _blob(parts):
    parts = [bytes(p) for p in parts]
    lens = np.array([len(p) for p in parts], np.uint64)
    offs = np.zeros(len(parts), np.uint64)
    if len(parts) > 1:
        offs[1:] = np.cumsum(lens)[:-1]
    buf = np.frombuffer(b"".join(parts) or b"\x00", np.uint8)
    return buf, offs, lens


def stream_probe_device(ptr: int, nbytes: int, reps: int = 8, ctx: Context | None = None):
    """srd_stream_probe_device: (best_ms, median_ms) of the scan-geometry
    streaming read of the first nbytes // 4096 tiles at device pointer ptr."""
    ctx = ctx or default_ctx()
    b, m = C.c_double(), C.c_double()
    _check(lib().srd_stream_probe_device(ctx.h, C.c_void_p(ptr), nbytes, reps, C.byref(b), C.byref(m)))
    return b.value, m.value


def batch_layout(tail: int, keys, payloads, allow_null: bool = False):
    """srd_batch_layout: (entries as a structured array, new tail); raises SrdError
    with the reference's InvalidInput messages (empty / NULL-byte payloads)."""
    kb, ko, kl = _blob(keys)
    pb, po, pl = _blob(payloads)
    n = len(payloads)
    out = (WriteEntry * max(n, 1))()
    nt = C.c_uint64()
    _check(lib().srd_batch_layout(tail, _ptr(pb), _ptr(ko), _ptr(kl), _ptr(po), _ptr(pl), n,
                                  WRITE_ALLOW_NULL if allow_null else 0, C.cast(out, C.c_void_p), C.byref(nt)))
    return out, int(nt.value)


def batch_write_raw(d_out: int, out_cap: int, tail: int, keys_ptr: int, key_offs: np.ndarray, key_lens: np.ndarray,
                    pay_ptr: int, pay_offs: np.ndarray, pay_lens: np.ndarray, flags: int = 0,
                    ctx: Context | None = None, want_index: bool = True):
    """srd_batch_write on caller buffers (host key / payload bytes at keys_ptr /
    pay_ptr, pinned for full PCIe rate; output in device memory d_out, which
    holds file bytes from tail & ~63).  Returns (new_tail, key_hashes, meta_offs)."""
    ctx = ctx or default_ctx()
    n = len(pay_lens)
    key_offs = np.ascontiguousarray(key_offs, np.uint64)
    key_lens = np.ascontiguousarray(key_lens, np.uint64)
    pay_offs = np.ascontiguousarray(pay_offs, np.uint64)
    pay_lens = np.ascontiguousarray(pay_lens, np.uint64)
    kh = np.zeros(max(n, 1), np.uint64) if want_index else None
    mo = np.zeros(max(n, 1), np.uint64) if want_index else None
    nt = C.c_uint64()
    _check(lib().srd_batch_write(ctx.h, tail, C.c_void_p(keys_ptr), _ptr(key_offs), _ptr(key_lens), C.c_void_p(pay_ptr),
                                 _ptr(pay_offs), _ptr(pay_lens), n, flags, C.c_void_p(d_out), out_cap, C.byref(nt),
                                 _ptr(kh) if want_index else None, _ptr(mo) if want_index else None))
    return int(nt.value), (kh[:n] if want_index else None), (mo[:n] if want_index else None)


def batch_write(keys, payloads, tail: int = 0, allow_null: bool = False, ctx: Context | None = None):
    """DataStoreWriter::batch_write on the GPU: keys hashed (compute_hash_batch),
    payloads CRC'd and serialized exactly as the reference appends them.
    Returns (new_tail, appended bytes [tail, new_tail), key_hashes, meta_offsets)."""
    import torch
    ctx = ctx or default_ctx()
    kb, ko, kl = _blob(keys)
    pb, po, pl = _blob(payloads)
    flags = WRITE_ALLOW_NULL if allow_null else 0
    nt = C.c_uint64()
    _check(lib().srd_batch_write(ctx.h, tail, _ptr(kb), _ptr(ko), _ptr(kl), _ptr(pb), _ptr(po), _ptr(pl),
                                 len(payloads), flags, None, 0, C.byref(nt), None, None))
    base = tail & ~63
    cap = max(int(nt.value) - base, 1)
    dev = torch.zeros(cap + 64, dtype=torch.uint8, device=f"cuda:{_ctx_device(ctx)}")
    _after_torch(ctx, dev.device)
    new_tail, kh, mo = batch_write_raw(dev.data_ptr(), cap, tail, kb.ctypes.data, ko, kl, pb.ctypes.data, po, pl,
                                       flags, ctx)
    _sync_ctx(ctx, dev.device)
    out = dev[tail - base: new_tail - base].cpu().numpy().tobytes()
    return new_tail, out, [int(x) for x in kh], [int(x) for x in mo]


def _ctx_device(ctx: Context) -> int:
    return int(os.environ.get("SRD_DEVICE", "0")) if ctx is None else getattr(ctx, "device", 0)


def _after_torch(ctx: Context, device):  # (DESIGN.md section 10's stream rule: this and _sync_ctx)
    """The context stream waits for torch's current stream (inputs torch wrote): an event, no host wait."""
    import torch
    torch.cuda.ExternalStream(ctx.stream, device=device).wait_stream(torch.cuda.current_stream(device))


def _sync_ctx(ctx: Context, device):
    """The host waits for the context stream (before torch reads what the library wrote)."""
    import torch
    torch.cuda.ExternalStream(ctx.stream, device=device).synchronize()


def _same_len(a, b, what: str):
    if len(a) != len(b):
        raise ValueError(f"Mismatched lengths for {what}.")


# ---------------------------------------------------------------------------
# Device KeyIndexer + batched keyed reads:
# KeyIndexer::get_packed (key_indexer.rs:164-167), batch_read /
# batch_read_hashed_keys (data_store.rs:1111-1158) over read_entry_with_context
# (:502-565)

INDEX_NONE = (1 << 64) - 1

# srd_payload_gather_device (include/srd_amd.h)
GATHER_CHUNK = 65536  # SRD_GATHER_CHUNK: the work-unit size in bytes
GATHER_VERIFY_ONLY = 1
GATHER_NONE, GATHER_OK, GATHER_BAD_CRC, GATHER_BAD_RANGE = 0, 1, 2, 3


class GatherResult:
    """What srd_payload_gather_device wrote for n queries: `data` (uint8 device
    tensor of the total: payload i at data[offs[i] : offs[i] + lens[i]], zero up
    to the next 64-byte boundary; None after a verify-only call), and the host
    arrays `offs` (n + 1), `lens`, `status` (GATHER_*) and `crc_computed`."""

    def __init__(self, data, offs, lens, status, crc_computed):
        self.data, self.offs, self.lens, self.status, self.crc_computed = data, offs, lens, status, crc_computed

    def __len__(self):
        return len(self.status)

    def payloads(self):
        """[payload bytes | None] in query order (None: no hit), by one copy to the host."""
        if self.data is None:
            raise ValueError("a verify-only gather holds no payload bytes")
        flat = self.data.cpu().numpy().tobytes() if self.data.numel() else b""
        return [flat[int(o): int(o) + int(n)] if s in (GATHER_OK, GATHER_BAD_CRC) else None
                for o, n, s in zip(self.offs, self.lens, self.status)]

    def is_valid_checksum(self):
        """EntryHandle::is_valid_checksum per query: [bool | None] (None: no hit)."""
        return [True if s == GATHER_OK else False if s == GATHER_BAD_CRC else None for s in self.status]


def payload_gather_device(d_file: int, file_len: int, d_start: int, d_end: int, n: int, flags: int = 0,
                          d_out: int | None = None, out_cap: int = 0, d_out_off: int | None = None,
                          d_status: int | None = None, d_crc_computed: int | None = None,
                          ctx: "Context | None" = None, stream: int | None = None) -> int:
    """srd_payload_gather_device as it is (device pointers in, the total out):
    ordered on `stream` (default: the context stream), returns with the copy
    enqueued.  SrdError carries SRD_ERR_ARG's message; `.total` is set on it when
    the capacity was the reason."""
    ctx = ctx or default_ctx()
    tot = C.c_uint64()
    rc = lib().srd_payload_gather_device(ctx.h, C.c_void_p(d_file), file_len, C.c_void_p(d_start), C.c_void_p(d_end), n,
                                         flags, C.c_void_p(d_out), out_cap, C.c_void_p(d_out_off),
                                         C.c_void_p(d_status), C.c_void_p(d_crc_computed), C.byref(tot),
                                         C.c_void_p(stream if stream is not None else ctx.stream))
    if rc != 0:
        e = SrdError(f"srd error {rc}: {lib().srd_last_error().decode()}")
        e.rc, e.total = rc, int(tot.value)
        raise e
    return int(tot.value)


def gather_ranges(d_file: int, file_len: int, st, en, flags: int = 0, ctx: "Context | None" = None) -> GatherResult:
    """The payloads of the ranges [st[i], en[i]) (device int64 tensors, as the
    read and iterator calls write them) gathered into one device buffer and
    checked against their stored checksums: the layout call sizes the buffer,
    the full call fills it.  §10's stream rule: the context stream waits for
    torch's current stream first, the host for the context stream at the end."""
    import torch
    ctx = ctx or default_ctx()
    dev, n = st.device, st.numel()
    offs = torch.empty(n + 1, dtype=torch.int64, device=dev)
    status = torch.empty(max(n, 1), dtype=torch.uint8, device=dev)
    crc = torch.empty(max(n, 1), dtype=torch.int32, device=dev)
    _after_torch(ctx, dev)
    args = (d_file, file_len, st.data_ptr(), en.data_ptr(), n)
    data = None
    if flags & GATHER_VERIFY_ONLY:
        payload_gather_device(*args, flags, None, 0, offs.data_ptr(), status.data_ptr(), crc.data_ptr(), ctx)
    else:
        total = payload_gather_device(*args, flags, None, 0, offs.data_ptr(), status.data_ptr(), None, ctx)
        data = torch.empty(total, dtype=torch.uint8, device=dev)
        _after_torch(ctx, dev)
        # (no hit at all: nothing to copy, the verify-only call completes statuses and CRCs)
        payload_gather_device(*args, flags if total else flags | GATHER_VERIFY_ONLY, data.data_ptr() if total else None,
                              total, offs.data_ptr(), status.data_ptr(), crc.data_ptr(), ctx)
    _sync_ctx(ctx, dev)
    o = offs.cpu().numpy().view(np.uint64)
    s = status[:n].cpu().numpy()
    ln = (en - st).cpu().numpy().view(np.uint64).copy()
    ln[(s != GATHER_OK) & (s != GATHER_BAD_CRC)] = 0
    return GatherResult(data, o, ln, s, crc[:n].cpu().numpy().view(np.uint32))


APPEND_STREAM_RULE = 1  # SRD_APPEND_STREAM_RULE: write_stream's refusal of NULL-byte-only payloads


def batch_append_device(d_payloads: int, payloads_len: int, d_src_off: int, d_len: int, d_key_hashes: int, n: int,
                        flags: int, tail: int, d_file: int, file_cap: int, d_meta_off_out: int,
                        ctx: "Context | None" = None, stream: int | None = None) -> int:
    """srd_batch_append_device as it is (device pointers in, the new tail out):
    ordered on `stream` (default: the context stream), returns with the copy
    enqueued.  SrdError carries the refusal's message and `.rc`."""
    ctx = ctx or default_ctx()
    nt = C.c_uint64()
    rc = lib().srd_batch_append_device(ctx.h, C.c_void_p(d_payloads), payloads_len, C.c_void_p(d_src_off),
                                       C.c_void_p(d_len), C.c_void_p(d_key_hashes), n, flags, tail, C.c_void_p(d_file),
                                       file_cap, C.byref(nt), C.c_void_p(d_meta_off_out),
                                       C.c_void_p(stream if stream is not None else ctx.stream))
    if rc != 0:
        e = SrdError(f"srd error {rc}: {lib().srd_last_error().decode()}")
        e.rc = rc
        raise e
    return int(nt.value)


def batch_append_segments_device(src_ptrs, src_lens, d_segs: int, n_segs: int, d_seg_first: int, d_key_hashes: int,
                                 n: int, tail: int, d_file: int, file_cap: int, d_meta_off_out: int,
                                 ctx: "Context | None" = None, stream: int | None = None, flags: int = 0) -> int:
    """srd_batch_append_segments_device as it is (the source table as host
    sequences of device addresses and lengths, device pointers for the rest, the
    new tail out): ordered on `stream` (default: the context stream), waits
    twice.  SrdError carries the refusal's message and `.rc`."""
    ctx = ctx or default_ctx()
    _same_len(src_ptrs, src_lens, "source pointers and source lengths")
    k = len(src_ptrs)
    ptrs = (C.c_void_p * max(k, 1))(*[int(p) for p in src_ptrs])
    lens = (C.c_uint64 * max(k, 1))(*[int(x) for x in src_lens])
    nt = C.c_uint64()
    rc = lib().srd_batch_append_segments_device(ctx.h, ptrs, lens, k, C.c_void_p(d_segs), n_segs, C.c_void_p(d_seg_first),
                                                C.c_void_p(d_key_hashes), n, flags, tail, C.c_void_p(d_file), file_cap,
                                                C.byref(nt), C.c_void_p(d_meta_off_out),
                                                C.c_void_p(stream if stream is not None else ctx.stream))
    if rc != 0:
        e = SrdError(f"srd error {rc}: {lib().srd_last_error().decode()}")
        e.rc = rc
        raise e
    return int(nt.value)


def _segment_table(entries, dev):
    """entries[i] as a sequence of contiguous tensors of any dtype on `dev`, taken
    as their bytes: the table {(data_ptr, nbytes): index} of the distinct tensors,
    the srd_segment tuples (whole tensors), the entries' first segments (n + 1)
    and the tensors (to keep them alive).  ValueError for anything else."""
    import torch
    table, keep = {}, []
    segs, first = [], [0]
    for ent in entries:
        if isinstance(ent, torch.Tensor) or isinstance(ent, (bytes, bytearray, str)):
            raise ValueError("an entry must be a sequence of tensors")
        for t in ent:
            if not isinstance(t, torch.Tensor) or t.device != dev or not t.is_contiguous():
                raise ValueError("a segment must be a contiguous tensor on the store's device")
            nb = t.numel() * t.element_size()
            k = table.setdefault((t.data_ptr(), nb), len(table))
            keep.append(t)
            segs.append((k, 0, 0, nb))
        first.append(len(segs))
    return table, segs, first, keep


def _header_segments(table, segs, first, hdr):
    """_segment_table's segments with 8 bytes of `hdr` (a device int64[n], added
    to the table) in front of each entry's: entry i starts with hdr[i]'s bytes
    -- a TTL entry's expiry header.  Returns the segments and the first segments."""
    k = table.setdefault((hdr.data_ptr(), 8 * hdr.numel()), len(table))
    out, ofirst = [], [0]
    for i in range(len(first) - 1):
        out.append((k, 0, 8 * i, 8))
        out.extend(segs[first[i]: first[i + 1]])
        ofirst.append(len(out))
    return out, ofirst


def _segments_to_device(segs, dev):
    import torch
    seg_arr = (Segment * max(len(segs), 1))(*segs)
    return torch.from_numpy(np.frombuffer(seg_arr, np.uint8).copy()).to(dev)


# srd_payload_scatter_device (include/srd_amd.h): d_status holds GATHER_* or
SCATTER_BAD_LENGTH = 4  # SRD_SCATTER_BAD_LENGTH: the segments' lengths do not sum to the payload's


class ScatterResult:
    """What srd_payload_scatter_device reported for n queries: the host arrays
    `status` (GATHER_NONE / _OK / _BAD_CRC / _BAD_RANGE, SCATTER_BAD_LENGTH) and
    `crc_computed` (0 where nothing was delivered).  The payloads themselves are
    in the caller's tensors."""

    def __init__(self, status, crc_computed):
        self.status, self.crc_computed = status, crc_computed

    def __len__(self):
        return len(self.status)

    def is_valid_checksum(self):
        """EntryHandle::is_valid_checksum per query, GatherResult's rule: [bool |
        None] (None: no hit -- a read's None or a BAD_RANGE).  ValueError if a
        query's tensors did not hold exactly its payload's bytes (BAD_LENGTH):
        nothing was delivered there, so there is no handle to judge."""
        bad = [i for i, s in enumerate(self.status) if s == SCATTER_BAD_LENGTH]
        if bad:
            raise ValueError(f"the segments of queries {bad[:8]} do not hold exactly their payloads' bytes")
        return [True if s == GATHER_OK else False if s == GATHER_BAD_CRC else None for s in self.status]


# srd_read_rows_device (include/srd_amd.h): d_status holds GATHER_NONE / _OK / _BAD_CRC or
ROWS_TOO_LONG = 5  # SRD_ROWS_TOO_LONG: the payload is longer than a row; lens holds its length


class RowsResult:
    """What srd_read_rows_device writes for n queries, as DEVICE tensors: `out`
    ([n, row_cap] uint8: payload i in out[i, :lens[i]] when delivered, the row
    left alone otherwise), `lens` (int64: the payload's length, also for a
    ROWS_TOO_LONG row; 0 for no entry), `status` (uint8: GATHER_NONE / _OK /
    _BAD_CRC, ROWS_TOO_LONG), `crc` (int32 bits of crc32(payload), 0 unless
    delivered) and `counts` (int64[6], queries per status value; None unless
    asked for).  Making one waits for nothing: the tensors are valid for work
    ordered behind the read on the stream it ran on (`stream`).  The host
    accessors below wait for that stream -- and torch's current one -- the first
    time one of them is called, copy `status` and `lens` once and keep them; a
    caller who replays a graph makes a new RowsResult of its tensors after each
    replay."""

    def __init__(self, out, lens, status, crc, counts=None, stream=None):
        self.out, self.lens, self.status, self.crc, self.counts, self.stream = out, lens, status, crc, counts, stream
        self._h = None

    def _host(self):
        if self._h is None:
            import torch
            if self.stream is not None:
                self.stream.synchronize()
            if self.status.is_cuda:
                torch.cuda.current_stream(self.status.device).synchronize()
            self._h = (self.status.cpu().numpy(), self.lens.cpu().numpy())
        return self._h

    def __len__(self):
        return int(self.status.shape[0])

    def is_valid_checksum(self):
        """EntryHandle::is_valid_checksum per query: [bool | None] (None: nothing
        was delivered -- no entry, or one too long for a row)."""
        return [True if s == GATHER_OK else False if s == GATHER_BAD_CRC else None for s in self._host()[0]]

    def too_long(self):
        """[(query, true length)] of the ROWS_TOO_LONG rows: what to read again
        with larger rows or through batch_read_into."""
        st, ln = self._host()
        return [(i, int(ln[i])) for i in np.flatnonzero(st == ROWS_TOO_LONG)]

    def payloads(self):
        """[payload bytes | None] in query order (None: nothing delivered), by one
        copy of `out` to the host."""
        st, ln = self._host()
        rows = self.out.cpu().numpy() if len(st) else None
        return [rows[i, : int(n)].tobytes() if s in (GATHER_OK, GATHER_BAD_CRC) else None
                for i, (n, s) in enumerate(zip(ln, st))]


class TtlReadResult:
    """What a batched read_with_ttl decided for n keys: the host arrays `status`
    (TTL_NOT_FOUND / _LIVE / _EXPIRED / _TOO_SHORT) and `expiry` (the stored
    expiry for LIVE and EXPIRED, else 0), `n_evicted` (tombstones the call wrote)
    and `gather`: the GatherResult of the live payloads, expiry header included
    (batch_read_with_ttl), or the ScatterResult (batch_read_with_ttl_into)."""

    def __init__(self, status, expiry, gather):
        self.status, self.expiry, self.gather, self.n_evicted = status, expiry, gather, 0

    def __len__(self):
        return len(self.status)

    def is_valid_checksum(self):
        """EntryHandle::is_valid_checksum per key: [bool | None] (None: not LIVE, nothing was read)."""
        return self.gather.is_valid_checksum()

    def values(self):
        """[value bytes | None] in key order (None: not LIVE): the gathered payloads without their 8 expiry bytes."""
        return [p[8:] if s == TTL_LIVE and p is not None else None for s, p in zip(self.status, self.gather.payloads())]


def payload_scatter_device(d_file: int, file_len: int, d_start: int, d_end: int, n: int, dst_ptrs, dst_lens,
                           d_segs: int, n_segs: int, d_seg_first: int, flags: int = 0, d_status: int | None = None,
                           d_crc_computed: int | None = None, ctx: "Context | None" = None,
                           stream: int | None = None) -> None:
    """srd_payload_scatter_device as it is (the destination table as host
    sequences of device addresses and lengths, device pointers for the rest):
    ordered on `stream` (default: the context stream), waits once and returns
    with the copy enqueued.  SrdError carries the refusal's message and `.rc`."""
    ctx = ctx or default_ctx()
    _same_len(dst_ptrs, dst_lens, "destination pointers and destination lengths")
    k = len(dst_ptrs)
    ptrs = (C.c_void_p * max(k, 1))(*[int(p) for p in dst_ptrs])
    lens = (C.c_uint64 * max(k, 1))(*[int(x) for x in dst_lens])
    rc = lib().srd_payload_scatter_device(ctx.h, C.c_void_p(d_file), file_len, C.c_void_p(d_start), C.c_void_p(d_end), n,
                                          ptrs, lens, k, C.c_void_p(d_segs), n_segs, C.c_void_p(d_seg_first), flags,
                                          C.c_void_p(d_status), C.c_void_p(d_crc_computed),
                                          C.c_void_p(stream if stream is not None else ctx.stream))
    if rc != 0:
        e = SrdError(f"srd error {rc}: {lib().srd_last_error().decode()}")
        e.rc = rc
        raise e


def _scatter_table(d_file: int, file_len: int, st, en, prep, ctx: Context) -> ScatterResult:
    """scatter_ranges behind _segment_table (prep)."""
    import torch
    table, segs, first, _keep = prep  # (the tensors live until the host has waited)
    dev, n = st.device, st.numel()
    if len(first) != n + 1:
        raise ValueError("Mismatched lengths for ranges and entries.")
    status = torch.empty(max(n, 1), dtype=torch.uint8, device=dev)
    crc = torch.empty(max(n, 1), dtype=torch.int32, device=dev)
    if n:
        d_segs = _segments_to_device(segs, dev)
        d_first = torch.from_numpy(np.array(first, np.int64)).to(dev)
        _after_torch(ctx, dev)
        try:
            payload_scatter_device(d_file, file_len, st.data_ptr(), en.data_ptr(), n, [p for p, _ in table],
                                   [nb for _, nb in table], d_segs.data_ptr(), len(segs), d_first.data_ptr(), 0,
                                   status.data_ptr(), crc.data_ptr(), ctx)
        finally:
            _sync_ctx(ctx, dev)  # (after a refusal too: the ranges may be temporaries still being written)
    return ScatterResult(status[:n].cpu().numpy(), crc[:n].cpu().numpy().view(np.uint32))


def scatter_ranges(d_file: int, file_len: int, st, en, entries, ctx: "Context | None" = None) -> ScatterResult:
    """The payloads of the ranges [st[i], en[i]) (device int64 tensors, as the
    read and iterator calls write them) delivered into entries[i], a sequence of
    contiguous tensors of any dtype on the ranges' device, taken as their bytes
    in order, and checked against their stored checksums
    (srd_payload_scatter_device; one destination per distinct (data_ptr,
    nbytes)).  §10's stream rule: the context stream waits for torch's current
    stream first, the host for the context stream at the end."""
    return _scatter_table(d_file, file_len, st, en, _segment_table(entries, st.device), ctx or default_ctx())


class DeviceIndex:
    """The KeyIndexer adopted on the GPU: an open-addressing table in HBM built
    from n unique (key_hash, packed) device pairs -- e.g. the index arrays of a
    validate pass (DeviceResult.index_key_hash / index_packed)."""

    def __init__(self, d_keys: int, d_packed: int, n: int, ctx: Context | None = None):
        import torch
        self.ctx = ctx or default_ctx()
        self.n = n
        self.nbytes = int(lib().srd_index_table_bytes(n))
        self.table = torch.empty(self.nbytes, dtype=torch.uint8, device=f"cuda:{self.ctx.device}")
        _check(lib().srd_index_table_build_device(self.ctx.h, C.c_void_p(d_keys), C.c_void_p(d_packed), n,
                                                  C.c_void_p(self.table.data_ptr()), self.nbytes))
        self._used = n      # slots that are not empty (live + deleted)
        self._live = n      # KeyIndexer::len; None = count on demand (after a delete through the C call)

    # -- kept live: reindex (data_store.rs:224-259) on the table in place -----------------

    def _lib_after_torch(self):
        _after_torch(self.ctx, self.table.device)

    def _sync_lib(self):
        _sync_ctx(self.ctx, self.table.device)

    def _as_dev(self, a, dtype=np.uint64):
        import torch
        if isinstance(a, torch.Tensor):
            return a.to(self.table.device).contiguous()
        h = np.ascontiguousarray(a, dtype)
        return torch.from_numpy(h.view(np.int64) if dtype == np.uint64 else h).to(self.table.device)

    @property
    def used(self) -> int:
        """Slots that are not empty: live keys plus removed ones (at most capacity / 2)."""
        return self._used

    @property
    def capacity(self) -> int:
        return 1 << ((self.nbytes // 16).bit_length() - 1)

    def __len__(self) -> int:
        """KeyIndexer::len: the live keys."""
        if self._live is None:
            n = C.c_uint64()
            self._lib_after_torch()
            _check(lib().srd_index_table_export_device(self.ctx.h, C.c_void_p(self.table.data_ptr()), self.nbytes,
                                                       None, None, 0, C.byref(n)))
            self._live = int(n.value)
        return self._live

    def export(self):
        """The live (key_hash, packed) pairs in file order (ascending metadata
        offset) as two device int64 tensors -- the index arrays the iterator and
        compaction calls take."""
        import torch
        n = len(self) if self._live is not None else self._used
        k = torch.empty(max(n, 1), dtype=torch.int64, device=self.table.device)
        p = torch.empty_like(k)
        got = C.c_uint64()
        self._lib_after_torch()
        _check(lib().srd_index_table_export_device(self.ctx.h, C.c_void_p(self.table.data_ptr()), self.nbytes,
                                                   C.c_void_p(k.data_ptr()), C.c_void_p(p.data_ptr()), k.numel(),
                                                   C.byref(got)))  # synchronises
        self._live = int(got.value)
        return k[: self._live], p[: self._live]

    def grow(self, n_keys: int):
        """A table for at least n_keys keys: export, then build into a larger
        buffer (which also drops the removed keys' slots)."""
        import torch
        k, p = self.export()
        n = k.numel()
        nbytes = int(lib().srd_index_table_bytes(max(n_keys, n)))
        table = torch.empty(nbytes, dtype=torch.uint8, device=self.table.device)
        self._lib_after_torch()
        _check(lib().srd_index_table_build_device(self.ctx.h, C.c_void_p(k.data_ptr()), C.c_void_p(p.data_ptr()), n,
                                                  C.c_void_p(table.data_ptr()), nbytes))  # synchronises
        self.table, self.nbytes, self.n, self._used, self._live = table, nbytes, n, n, n

    def apply(self, key_hashes, meta_offs, tomb=None) -> tuple[int, int, int]:
        """DataStore::reindex of a batch of (key_hash, metadata offset[, tombstone])
        pairs -- host arrays or device tensors, e.g. the writer's outputs.  Returns
        (inserted, updated, removed) per distinct key.  A batch the table has no
        room for grows it (export + rebuild at twice the need) and is applied then."""
        kh, mo = self._as_dev(key_hashes), self._as_dev(meta_offs)
        tb = self._as_dev(tomb, np.uint8) if tomb is not None else None
        n = kh.numel()
        if mo.numel() != n or (tb is not None and tb.numel() != n):
            raise ValueError("Mismatched lengths for key hashes, offsets and tombstone flags.")
        st = ApplyStats()
        for attempt in range(2):
            used = C.c_uint64(self._used)
            self._lib_after_torch()
            rc = lib().srd_index_table_apply_device(self.ctx.h, C.c_void_p(self.table.data_ptr()), self.nbytes,
                                                    C.byref(used), C.c_void_p(kh.data_ptr()), C.c_void_p(mo.data_ptr()),
                                                    C.c_void_p(tb.data_ptr()) if tb is not None else None, n,
                                                    C.byref(st), C.c_void_p(self.ctx.stream))
            if rc == SRD_ERR_FULL and attempt == 0:
                self.grow(2 * (self._used + n))  # room for every pair being a new key, at load <= 1/4
                continue
            _check(rc)
            break
        self._sync_lib()  # the inputs may be temporaries: the commit has read them before they are released
        self._used = int(used.value)
        if self._live is not None:
            self._live += int(st.n_inserted) - int(st.n_removed)
        return st.as_tuple()

    def remove(self, key_hashes) -> int:
        """KeyIndexer::remove for each hash; returns how many keys were present."""
        kh = self._as_dev(key_hashes)
        import torch
        ones = torch.ones(kh.numel(), dtype=torch.uint8, device=self.table.device)
        return self.apply(kh, torch.zeros_like(kh), ones)[2]

    def get_packed(self, hashes) -> np.ndarray:
        """KeyIndexer::get_packed for each hash (INDEX_NONE when absent)."""
        import torch
        q = self._as_dev(hashes)
        out = torch.empty_like(q)
        self._lib_after_torch()
        _check(lib().srd_index_get_packed_device(self.ctx.h, C.c_void_p(self.table.data_ptr()), self.nbytes,
                                                 C.c_void_p(q.data_ptr()), q.numel(), C.c_void_p(out.data_ptr()),
                                                 C.c_void_p(self.ctx.stream)))
        self._sync_lib()
        return out.cpu().numpy().view(np.uint64)

    def _ranges_device(self, d_file: int, file_len: int, hashes, verify=None):
        """srd_batch_read_hashed_device on the context stream: the ranges stay on
        the device (two int64 tensors), nothing waits."""
        import torch
        q = self._as_dev(hashes)
        v = self._as_dev(verify) if verify is not None else None
        st, en = torch.empty_like(q), torch.empty_like(q)
        self._lib_after_torch()
        _check(lib().srd_batch_read_hashed_device(self.ctx.h, C.c_void_p(self.table.data_ptr()), self.nbytes,
                                                  C.c_void_p(d_file), file_len, C.c_void_p(q.data_ptr()),
                                                  C.c_void_p(v.data_ptr()) if v is not None else None, q.numel(),
                                                  C.c_void_p(st.data_ptr()), C.c_void_p(en.data_ptr()),
                                                  C.c_void_p(self.ctx.stream)))
        return st, en, (q, v)  # (the inputs live until the caller has waited)

    def _ranges_host(self, d_file: int, file_len: int, hashes, verify=None):
        """... waited for and copied to the host: two uint64 arrays (start == end: None)."""
        st, en, _keep = self._ranges_device(d_file, file_len, hashes, verify)
        self._sync_lib()
        return st.cpu().numpy().view(np.uint64), en.cpu().numpy().view(np.uint64)

    def batch_read_hashed_keys(self, d_file: int, file_len: int, hashes, non_hashed_keys=None):
        """batch_read_hashed_keys: [(start, end) | None] in query order; with
        non_hashed_keys, each read is verified by tag_from_key (data_store.rs:513-521)."""
        if non_hashed_keys is not None:
            _same_len(non_hashed_keys, hashes, "hashed and non-hashed keys")
        v = compute_hash_batch(non_hashed_keys, self.ctx) if non_hashed_keys is not None else None
        s, e = self._ranges_host(d_file, file_len, hashes, v)
        return [None if a == b else (int(a), int(b)) for a, b in zip(s, e)]

    def batch_gather(self, d_file: int, file_len: int, hashes, non_hashed_keys=None, flags: int = 0) -> GatherResult:
        """batch_read_hashed_keys with the payloads: the look-up and the verified
        gather (srd_payload_gather_device) on the device, one GatherResult in query
        order -- a read's bytes plus EntryHandle::is_valid_checksum for each."""
        if non_hashed_keys is not None:
            _same_len(non_hashed_keys, hashes, "hashed and non-hashed keys")
        v = compute_hash_batch(non_hashed_keys, self.ctx) if non_hashed_keys is not None else None
        return self._gather(d_file, file_len, hashes, v, flags)

    def _gather(self, d_file: int, file_len: int, hashes, verify, flags: int) -> GatherResult:
        st, en, _keep = self._ranges_device(d_file, file_len, hashes, verify)  # (alive until the gather has waited)
        return gather_ranges(d_file, file_len, st, en, flags, self.ctx)

    def batch_scatter(self, d_file: int, file_len: int, hashes, entries, non_hashed_keys=None) -> ScatterResult:
        """batch_read_hashed_keys with every payload delivered into the caller's
        own tensors (entries[i]: scatter_ranges' rule) and checked: the look-up
        and srd_payload_scatter_device on the device -- an EntryStream read into
        the caller's buffers (entry_stream.rs:76-91) plus
        EntryHandle::is_valid_checksum for each query."""
        if non_hashed_keys is not None:
            _same_len(non_hashed_keys, hashes, "hashed and non-hashed keys")
        v = compute_hash_batch(non_hashed_keys, self.ctx) if non_hashed_keys is not None else None
        return self._scatter(d_file, file_len, hashes, v, entries)

    def _scatter(self, d_file: int, file_len: int, hashes, verify, entries) -> ScatterResult:
        _same_len(hashes, entries, "key hashes and entries")
        prep = _segment_table(entries, self.table.device)  # (the ValueErrors: before any call)
        st, en, _keep = self._ranges_device(d_file, file_len, hashes, verify)  # (alive until the scatter has waited)
        return _scatter_table(d_file, file_len, st, en, prep, self.ctx)

    def batch_read(self, d_file: int, file_len: int, keys):
        """batch_read (data_store.rs:1111-1115): host keys, hashed and verified on the device."""
        kb, ko, kl = _blob(keys)
        n = len(keys)
        st = np.zeros(max(n, 1), np.uint64)
        en = np.zeros(max(n, 1), np.uint64)
        _check(lib().srd_batch_read(self.ctx.h, C.c_void_p(self.table.data_ptr()), self.nbytes, C.c_void_p(d_file),
                                    file_len, _ptr(kb), _ptr(ko), _ptr(kl), n, _ptr(st), _ptr(en)))
        return [None if a == b else (int(a), int(b)) for a, b in zip(st[:n], en[:n])]

    def read_rows(self, d_file: int, file_len: int, hashes, out, non_hashed_keys=None, lens=None, status=None,
                  crc=None, counts=None) -> RowsResult:
        """batch_read_hashed_keys (data_store.rs:1111-1158) with payload i copied
        into row i of `out` and checked (srd_read_rows_device): the look-up, the
        copy and the checksum on the device, with NO host wait anywhere -- nothing
        of the layout goes through the host.  `out` is a 2-D uint8 tensor on the
        index's device whose rows are contiguous (out.stride(1) == 1): row_cap =
        out.shape[1], row_stride = out.stride(0), a multiple of 16, out.data_ptr()
        16-byte aligned.  `hashes` may be a contiguous device int64 tensor, which is
        used in place with no copy (a replayed graph reads it as it is then); a
        host sequence is copied to the device first.  `non_hashed_keys` (host keys,
        hashed here, which waits; or a device int64 tensor of their hashes, used in
        place) verifies each read by tag_from_key (:513-521).  `lens` (int64[n]),
        `status` (uint8[n]), `crc` (int32[n]) and `counts` (int64[6]) are the
        caller's own output tensors when given -- a caller who replays a graph
        passes them in; `counts` is only filled when given.  A row that is not
        delivered (GATHER_NONE, ROWS_TOO_LONG) is left exactly as it was.
        The stream rule: the call runs on torch's CURRENT stream.  Outside a
        capture that stream first waits in-stream (an event) for the context
        stream, so it sees what the library wrote before.  torch's default
        stream has the handle 0, which the library reads as "the context
        stream": the call then runs on the context stream between two events
        -- that stream waits for torch's, torch's waits for the read -- so work
        ordered behind the read on torch's stream, and a host wait for that
        stream, see the results all the same.  Under capture
        (torch.cuda.is_current_stream_capturing()) no cross-stream wait is issued:
        the caller has waited for the context stream (DeviceStore.sync) before
        capturing, and has called Context.reserve_rows(n, row_cap) -- a capture
        that would have to grow the workspace raises SrdError naming
        srd_ctx_reserve_rows."""
        import torch
        dev = self.table.device
        if not (isinstance(out, torch.Tensor) and out.dtype == torch.uint8 and out.dim() == 2 and out.device == dev and
                (out.shape[1] == 0 or out.stride(1) == 1)):
            raise ValueError("out must be a 2-D uint8 tensor on the index's device with contiguous rows")
        n = out.shape[0]
        q = hashes if isinstance(hashes, torch.Tensor) else self._as_dev(hashes)
        v = non_hashed_keys
        if v is not None and not isinstance(v, torch.Tensor):
            _same_len(v, q, "hashed and non-hashed keys")
            v = self._as_dev(compute_hash_batch(v, self.ctx))
        outs = {"hashes": (q, torch.int64, n), "non_hashed_keys": (v, torch.int64, n), "lens": (lens, torch.int64, n),
                "status": (status, torch.uint8, n), "crc": (crc, torch.int32, n), "counts": (counts, torch.int64, 6)}
        for name, (t, dt, m) in outs.items():
            if t is not None and not (isinstance(t, torch.Tensor) and t.dtype == dt and t.dim() == 1 and
                                      t.numel() == m and t.device == dev and t.is_contiguous()):
                raise ValueError(f"{name} must be a contiguous {dt} tensor of {m} elements on the index's device")
        lens = lens if lens is not None else torch.empty(n, dtype=torch.int64, device=dev)
        status = status if status is not None else torch.empty(n, dtype=torch.uint8, device=dev)
        crc = crc if crc is not None else torch.empty(n, dtype=torch.int32, device=dev)
        cur = torch.cuda.current_stream(dev)
        res = RowsResult(out, lens, status, crc, counts, cur)
        if not n:
            return res
        on_ctx = cur.cuda_stream == 0  # (the default stream cannot be named to the library: NULL is the context's)
        lib_stream = torch.cuda.ExternalStream(self.ctx.stream, device=dev)
        if on_ctx:
            lib_stream.wait_stream(cur)
        elif not torch.cuda.is_current_stream_capturing():
            cur.wait_stream(lib_stream)
        p = lambda t: C.c_void_p(t.data_ptr()) if t is not None else None
        _check(lib().srd_read_rows_device(self.ctx.h, p(self.table), self.nbytes, C.c_void_p(d_file), file_len, p(q), p(v),
                                          n, p(out), out.stride(0), out.shape[1], p(lens), p(status), p(crc), p(counts), 0,
                                          C.c_void_p(self.ctx.stream if on_ctx else cur.cuda_stream)))
        if on_ctx:
            cur.wait_stream(lib_stream)
        res._keep = (q, v)  # (temporaries of this call: torch's allocator reuses them in stream order)
        return res


# ---------------------------------------------------------------------------
# EntryIterator / par_iter_entries, estimate_compaction_savings and compact
# over the device index (data_store.rs:297-361, 605-749; entry_iterator.rs:69-126)

def _iter_entries(d_file: int, file_len: int, d_index_packed: int, n_index: int, ctx: Context):
    """srd_iter_entries_device (synchronises): device int64 tensors (start, end, meta_off, key_hash)."""
    import torch
    dev = torch.device(f"cuda:{ctx.device}")
    outs = [torch.empty(max(n_index, 1), dtype=torch.int64, device=dev) for _ in range(4)]
    n = C.c_uint64()
    _after_torch(ctx, dev)
    _check(lib().srd_iter_entries_device(ctx.h, C.c_void_p(d_file), file_len, C.c_void_p(d_index_packed), n_index,
                                         *[C.c_void_p(t.data_ptr()) for t in outs], C.byref(n)))
    return tuple(t[: int(n.value)] for t in outs)


def iter_entries_device(d_file: int, file_len: int, d_index_packed: int, n_index: int, ctx: Context | None = None):
    """The latest non-tombstone entry per key, newest first (EntryIterator
    order): numpy arrays (start, end, meta_off, key_hash)."""
    outs = _iter_entries(d_file, file_len, d_index_packed, n_index, ctx or default_ctx())
    return tuple(t.cpu().numpy().view(np.uint64) for t in outs)


def estimate_compaction_savings_device(d_file: int, file_len: int, d_index_packed: int, n_index: int,
                                       ctx: Context | None = None) -> int:
    ctx = ctx or default_ctx()
    s = C.c_uint64()
    _check(lib().srd_estimate_compaction_savings_device(ctx.h, C.c_void_p(d_file), file_len,
                                                        C.c_void_p(d_index_packed), n_index, C.byref(s)))
    return int(s.value)


def compact_device(d_file: int, file_len: int, d_index_packed: int, n_index: int, ctx: Context | None = None):
    """compact(): the compacted store's bytes as a device tensor."""
    import torch
    ctx = ctx or default_ctx()
    dev = torch.device(f"cuda:{ctx.device}")
    nl = C.c_uint64()
    _after_torch(ctx, dev)
    _check(lib().srd_compact_device(ctx.h, C.c_void_p(d_file), file_len, C.c_void_p(d_index_packed), n_index, None,
                                    0, C.byref(nl), None, None))
    out = torch.zeros(max(int(nl.value), 1) + 64, dtype=torch.uint8, device=dev)
    _after_torch(ctx, dev)
    _check(lib().srd_compact_device(ctx.h, C.c_void_p(d_file), file_len, C.c_void_p(d_index_packed), n_index,
                                    C.c_void_p(out.data_ptr()), out.numel(), C.byref(nl), None, None))
    _sync_ctx(ctx, dev)
    return out[: int(nl.value)]


def compact_live_device(d_table: int, table_bytes: int, d_file: int, file_len: int, d_out: int | None = None,
                        out_cap: int = 0, d_new_table: int | None = None, new_table_bytes: int = 0,
                        ctx: Context | None = None) -> CompactStats:
    """srd_compact_live_device as it is (device pointers in, the stats out): on
    the context stream, synchronises.  d_out None is the planning call.  SrdError
    carries the refusal's message, `.rc` and `.stats` (what was known by then)."""
    ctx = ctx or default_ctx()
    st = CompactStats()
    rc = lib().srd_compact_live_device(ctx.h, C.c_void_p(d_table), table_bytes, C.c_void_p(d_file), file_len,
                                       C.c_void_p(d_out), out_cap, C.c_void_p(d_new_table), new_table_bytes,
                                       C.byref(st))
    if rc != 0:
        e = SrdError(f"srd error {rc}: {lib().srd_last_error().decode()}")
        e.rc, e.stats = rc, st
        raise e
    return st


# ---------------------------------------------------------------------------
# A store resident in HBM with its index kept live: write -> reindex -> read
# (DataStoreWriter / DataStoreReader of data_store.rs over one device buffer)

class DeviceStore:
    """A store in a device byte buffer of fixed capacity, its tail, and the
    DeviceIndex of it, maintained in place by every write and delete -- the
    in-session loop of the reference (batch_write_with_key_hashes ends in
    reindex, data_store.rs:936).  Each method is named after the reference
    method it replaces.  All library work runs on the context stream, ordered
    after torch's current stream where it reads what torch wrote; the host
    waits for the context stream before torch reads what the library wrote."""

    def __init__(self, buf, tail: int, index: DeviceIndex, ctx: Context):
        self.buf, self._tail, self.index, self.ctx = buf, tail, index, ctx

    @classmethod
    def create(cls, capacity: int, ctx: Context | None = None) -> "DeviceStore":
        """An empty store that can grow to `capacity` bytes."""
        import torch
        ctx = ctx or default_ctx()
        buf = torch.zeros(padded_size(capacity), dtype=torch.uint8, device=f"cuda:{ctx.device}")
        return cls(buf, 0, DeviceIndex(0, 0, 0, ctx), ctx)

    @classmethod
    def open(cls, dev_tensor, file_len: int, ctx: Context | None = None) -> "DeviceStore":
        """DataStore::open (data_store.rs:84-117) of the store in dev_tensor[:file_len]
        (a uint8 device tensor of at least padded_size(file_len) bytes; its size is
        the capacity): validates it, adopts the index, and appends at the recovered tail."""
        import torch
        ctx = ctx or default_ctx()
        if dev_tensor.numel() < padded_size(file_len):
            raise ValueError("the store buffer must hold padded_size(file_len) bytes")
        _after_torch(ctx, dev_tensor.device)
        r = validate_index_device(dev_tensor.data_ptr(), file_len, 0, ctx)  # synchronises
        return cls(dev_tensor, int(r.final_len), DeviceIndex(r.index_key_hash, r.index_packed, int(r.n_index), ctx), ctx)

    @property
    def tail(self) -> int:
        return self._tail

    def len(self) -> int:
        """DataStoreReader::len (data_store.rs:1164): the index's live keys."""
        return len(self.index)

    __len__ = len

    def bytes(self) -> bytes:
        """The store's bytes [0, tail)."""
        self.index._sync_lib()
        return self.buf[: self._tail].cpu().numpy().tobytes()

    # -- writes ---------------------------------------------------------------------------

    def batch_write(self, keys, payloads) -> int:
        """DataStoreWriter::batch_write (data_store.rs:838-843): compute_hash_batch,
        then batch_write_with_key_hashes."""
        _same_len(keys, payloads, "keys and payloads")
        return self.batch_write_with_key_hashes(compute_hash_batch(keys, self.ctx), payloads, False)

    def batch_write_with_key_hashes(self, hashes, payloads, allow_null: bool = False) -> int:
        """data_store.rs:847-939: the entries serialized at the tail by the writer
        kernel, straight into the store buffer, then the reindex of their (key_hash,
        offset) pairs on the device.  Returns the new tail.  Empty / NULL-byte
        payloads fail as srd_batch_layout does; a batch that does not fit the
        capacity raises ValueError before anything is written."""
        import torch
        n = len(payloads)
        _same_len(hashes, payloads, "key hashes and payloads")
        if not n:
            return self._tail
        payloads = [bytes(p) for p in payloads]
        lens = np.array([len(p) for p in payloads], np.uint64)
        # every payload at a 16-byte boundary of the staging blob: the writer moves
        # whole 16-byte pieces of such sources
        offs = np.zeros(n, np.uint64)
        offs[1:] = np.cumsum((lens + np.uint64(15)) & ~np.uint64(15))[:-1]
        blob = np.zeros(int(offs[-1] + lens[-1]) or 1, np.uint8)
        for o, p in zip(offs, payloads):
            blob[int(o): int(o) + len(p)] = np.frombuffer(p, np.uint8)
        zero = np.zeros(n, np.uint64)
        ent = (WriteEntry * n)()
        nt = C.c_uint64()
        _check(lib().srd_batch_layout(self._tail, _ptr(blob), _ptr(zero), _ptr(zero), _ptr(offs), _ptr(lens), n,
                                      WRITE_ALLOW_NULL if allow_null else 0, C.cast(ent, C.c_void_p), C.byref(nt)))
        new_tail = int(nt.value)
        if padded_size(new_tail) > self.buf.numel():
            raise ValueError(f"the batch ends at {new_tail}: beyond the store's capacity")
        tomb = np.zeros(n, np.uint8)
        for i, h in enumerate(hashes):  # batch_write_with_key_hashes: the keys are prehashed
            ent[i].key_src = int(h)
            ent[i].key_len = 0
            tomb[i] = ent[i].flags & 1
            ent[i].flags |= 2  # SRD_ENTRY_HASHED
        dev = self.buf.device
        d_ent = torch.from_numpy(np.frombuffer(ent, np.uint8).copy()).to(dev)
        d_pay = torch.from_numpy(blob).to(dev)
        d_kh = torch.empty(n, dtype=torch.int64, device=dev)
        d_mo = torch.empty(n, dtype=torch.int64, device=dev)
        base = self._tail & ~63
        self.index._lib_after_torch()
        _check(lib().srd_batch_write_device(self.ctx.h, C.c_void_p(d_pay.data_ptr()), C.c_void_p(d_pay.data_ptr()),
                                            C.c_void_p(d_ent.data_ptr()), n, C.c_void_p(self.buf.data_ptr() + base),
                                            base, C.c_void_p(d_kh.data_ptr()), C.c_void_p(d_mo.data_ptr()),
                                            C.c_void_p(self.ctx.stream)))
        self.index.apply(d_kh, d_mo, tomb if tomb.any() else None)  # same stream: behind the writer; waits
        self._tail = new_tail
        return new_tail

    # -- writes of payloads that are already on the device ----------------------------------

    def _append_reindex(self, call, d_hashes, d_mo) -> int:
        """A library append call on the context stream (§10's stream rule; call()
        returns the new tail and fills d_mo), then the reindex of its (key_hash,
        offset) pairs, then the tail.  Any error leaves the tail and the index as
        they were."""
        self.index._lib_after_torch()
        try:
            new_tail = call()
        except SrdError as e:
            self.index._sync_lib()  # (the inputs may be temporaries of the caller)
            if e.rc == SRD_ERR_ARG and "file_cap" in str(e):
                raise ValueError("the batch ends beyond the store's capacity") from e
            raise
        self.index.apply(d_hashes, d_mo)  # same stream: behind the append; waits
        self._tail = new_tail
        return new_tail

    def _append_device(self, d_hashes, blob_ptr: int, blob_len: int, d_offs, d_lens, flags: int) -> int:
        """srd_batch_append_device, reindex, tail (_append_reindex)."""
        import torch
        n = d_hashes.numel()
        d_mo = torch.empty(n, dtype=torch.int64, device=self.buf.device)
        return self._append_reindex(
            lambda: batch_append_device(blob_ptr, blob_len, d_offs.data_ptr(), d_lens.data_ptr(), d_hashes.data_ptr(), n,
                                        flags, self._tail, self.buf.data_ptr(), self.buf.numel(), d_mo.data_ptr(),
                                        self.ctx), d_hashes, d_mo)

    def batch_write_device_with_key_hashes(self, hashes, blob, offs, lens, stream_rule: bool = False) -> int:
        """batch_write_with_key_hashes(.., false) (data_store.rs:847-939) for
        payloads that already lie in HBM: entry i is blob[offs[i] : offs[i] +
        lens[i]] (`blob`: a contiguous uint8 tensor on the store's device; hashes,
        offs, lens: host sequences or device int64 tensors).  The layout, the copy
        and the checksums run on the device (srd_batch_append_device), then the
        reindex.  Returns the new tail.  stream_rule adds write_stream's refusal of
        payloads that are all NULL bytes.  A batch beyond the capacity raises
        ValueError, the other refusals SrdError with the reference's message; the
        tail and the index are unchanged then."""
        import torch
        if not isinstance(blob, torch.Tensor) or blob.dtype != torch.uint8 or blob.device != self.buf.device or \
                not blob.is_contiguous():
            raise ValueError("blob must be a contiguous uint8 tensor on the store's device")
        _same_len(hashes, offs, "key hashes and payload offsets")
        _same_len(hashes, lens, "key hashes and payload lengths")
        if not len(hashes):
            return self._tail
        as_dev = self.index._as_dev
        return self._append_device(as_dev(hashes), blob.data_ptr(), blob.numel(), as_dev(offs), as_dev(lens),
                                   APPEND_STREAM_RULE if stream_rule else 0)

    def batch_write_device(self, keys, blob, offs, lens) -> int:
        """batch_write (data_store.rs:838-843) for payloads in HBM: compute_hash_batch,
        then batch_write_device_with_key_hashes."""
        _same_len(keys, offs, "keys and payloads")
        if not len(keys):
            return self._tail
        return self.batch_write_device_with_key_hashes(compute_hash_batch(keys, self.ctx), blob, offs, lens)

    # -- writes of payloads that arrive as a sequence of device segments ----------------------

    def batch_write_stream_with_key_hashes(self, hashes, entries) -> int:
        """n write_stream_with_key_hash calls (data_store.rs:758-825) for payloads
        that arrive in pieces in HBM: entries[i] is a sequence of contiguous
        tensors of any dtype on the store's device, taken as their bytes, in
        order (a tensor of no bytes adds nothing; a slice of the store's own
        buffer below the tail is allowed).  One source per distinct (data_ptr,
        nbytes); the layout, the copy and the checksums over the pieces run on
        the device (srd_batch_append_segments_device), then the reindex.  Returns
        the new tail.  Anything that is not such a tensor raises ValueError
        before any call, as does a batch beyond the capacity; the library's
        refusals (an empty payload, one that is all NULL bytes, ...) raise
        SrdError with the reference's message; the tail and the index are
        unchanged then."""
        import torch
        _same_len(hashes, entries, "key hashes and entries")
        n = len(entries)
        if not n:
            return self._tail
        srcs, segs, first, keep = _segment_table(entries, self.buf.device)
        return self._append_segments(hashes, srcs, segs, first, keep)

    def _append_segments(self, hashes, srcs, segs, first, _keep) -> int:
        """srd_batch_append_segments_device over a source table, its srd_segment
        tuples and the entries' first segments (_segment_table's), reindex, tail."""
        import torch
        dev, n = self.buf.device, len(first) - 1
        d_segs = _segments_to_device(segs, dev)
        d_first = self.index._as_dev(np.array(first, np.uint64))
        d_hashes = self.index._as_dev(hashes)
        d_mo = torch.empty(n, dtype=torch.int64, device=dev)
        return self._append_reindex(  # (_keep holds the segments until the call has returned)
            lambda: batch_append_segments_device([p for p, _ in srcs], [nb for _, nb in srcs], d_segs.data_ptr(),
                                                 len(segs), d_first.data_ptr(), d_hashes.data_ptr(), n, self._tail,
                                                 self.buf.data_ptr(), self.buf.numel(), d_mo.data_ptr(), self.ctx),
            d_hashes, d_mo)

    def batch_write_stream(self, keys, entries) -> int:
        """write_stream (data_store.rs:753-756) of every key: compute_hash_batch,
        then batch_write_stream_with_key_hashes."""
        _same_len(keys, entries, "keys and entries")
        if not len(keys):
            return self._tail
        return self.batch_write_stream_with_key_hashes(compute_hash_batch(keys, self.ctx), entries)

    def write_stream_with_key_hash(self, key_hash: int, segments) -> int:
        """write_stream_with_key_hash (data_store.rs:758-825): one entry from its segments."""
        return self.batch_write_stream_with_key_hashes([key_hash], [segments])

    def write_stream(self, key: bytes, segments) -> int:
        """write_stream (data_store.rs:753-756)."""
        return self.batch_write_stream([key], [segments])

    # -- copy / transfer / rename (data_store.rs:941-984): write_stream of the read entry ---

    def _entries_of(self, keys, missing: str):
        """The payload ranges of `keys` as device tensors (hashes, start, length)
        and the lengths on the host, every read verified by its key's own tag;
        KeyError for a key that reads as None."""
        keys = [bytes(k) for k in keys]
        if len(set(keys)) != len(keys):
            raise ValueError("Duplicate keys in one batch.")
        h = compute_hash_batch(keys, self.ctx)
        st, en, _keep = self.index._ranges_device(self.buf.data_ptr(), self._tail, h, h)
        self.index._sync_lib()
        hs, he = st.cpu().numpy(), en.cpu().numpy()
        for k, a, b in zip(keys, hs, he):
            if a == b:
                raise KeyError(f"{missing}: {k!r}")
        return _keep[0], st, en - st, he - hs

    def _append_from(self, src: "DeviceStore", d_hashes, st, lens) -> int:
        """write_stream_with_key_hash of src's entries at [st, st + lens) into this
        store (copy_handle, data_store.rs:587-590): the checksums are recomputed,
        NULL-byte-only payloads refused.  Runs on this store's context, after
        src's context stream."""
        import torch
        if src.buf.device != self.buf.device:
            raise ValueError("both stores must be on one device")
        dev = self.buf.device
        torch.cuda.ExternalStream(self.ctx.stream, device=dev).wait_stream(
            torch.cuda.ExternalStream(src.ctx.stream, device=dev))
        return self._append_device(d_hashes, src.buf.data_ptr(), src._tail, st, lens, APPEND_STREAM_RULE)

    def batch_copy(self, keys, target: "DeviceStore") -> int:
        """copy (data_store.rs:960-979) of every key: the entries appended to
        `target` under their key hashes.  Returns target's new tail."""
        if target is self or target.buf.data_ptr() == self.buf.data_ptr():
            raise ValueError("Cannot copy entry to the same storage. Use `rename` instead.")
        if not len(keys):
            return target._tail
        return target._append_from(self, *self._entries_of(keys, "Key not found")[:3])

    def batch_transfer(self, keys, target: "DeviceStore") -> int:
        """transfer (data_store.rs:981-984): copy, then delete here.  Returns this
        store's new tail.  The whole transfer or nothing: once the keys are
        resolved (copy's errors come first: the same storage, a duplicate, a
        missing key), tombstones that would end beyond this store's capacity
        raise ValueError before anything is copied."""
        if target is self or target.buf.data_ptr() == self.buf.data_ptr():
            raise ValueError("Cannot copy entry to the same storage. Use `rename` instead.")
        if not len(keys):
            return self._tail
        h, st, lens, _hl = self._entries_of(keys, "Key not found")
        if padded_size(self._tail + 21 * len(keys)) > self.buf.numel():
            raise ValueError("the tombstones end beyond the store's capacity")
        target._append_from(self, h, st, lens)
        return self.batch_delete(keys)

    def batch_rename(self, old_keys, new_keys) -> int:
        """rename (data_store.rs:941-958) of every pair: the old entries appended
        under the new keys' hashes, then the old keys deleted.  Returns the new
        tail.  The whole rename or nothing: entries whose tombstones would end
        beyond the capacity raise ValueError before anything is appended."""
        _same_len(old_keys, new_keys, "old and new keys")
        old_keys, new_keys = [bytes(k) for k in old_keys], [bytes(k) for k in new_keys]
        if any(a == b for a, b in zip(old_keys, new_keys)):
            raise ValueError("Cannot rename a key to itself")
        if len(set(new_keys)) != len(new_keys) or set(new_keys) & set(old_keys):
            raise ValueError("Duplicate keys in one batch.")
        if not old_keys:
            return self._tail
        _h, st, lens, hl = self._entries_of(old_keys, "Old key not found")
        tail = self._tail
        for n in hl:  # each payload at the next 64-byte boundary, then its 20 metadata bytes
            tail = ((tail + 63) & ~63) + int(n) + 20
        if padded_size(tail + 21 * len(old_keys)) > self.buf.numel():
            raise ValueError("the renamed entries and their tombstones end beyond the store's capacity")
        self._append_from(self, self.index._as_dev(compute_hash_batch(new_keys, self.ctx)), st, lens)
        return self.batch_delete(old_keys)

    def copy(self, key: bytes, target: "DeviceStore") -> int:
        return self.batch_copy([key], target)

    def transfer(self, key: bytes, target: "DeviceStore") -> int:
        return self.batch_transfer([key], target)

    def rename(self, old_key: bytes, new_key: bytes) -> int:
        return self.batch_rename([old_key], [new_key])

    def batch_delete(self, keys) -> int:
        """DataStoreWriter::batch_delete (data_store.rs:990-993)."""
        return self.batch_delete_key_hashes(compute_hash_batch(keys, self.ctx))

    def batch_delete_key_hashes(self, hashes) -> int:
        """data_store.rs:995-1024: one tombstone per listed hash the index holds,
        appended at the tail, and the keys removed from the index.  Returns the new tail."""
        idx = self.index
        q = idx._as_dev(hashes)
        used, nt, nd = C.c_uint64(idx._used), C.c_uint64(), C.c_uint64()
        idx._lib_after_torch()
        rc = lib().srd_batch_delete_hashed_device(self.ctx.h, C.c_void_p(idx.table.data_ptr()), idx.nbytes,
                                                  C.byref(used), C.c_void_p(q.data_ptr()), q.numel(), self._tail,
                                                  C.c_void_p(self.buf.data_ptr()), self.buf.numel(), C.byref(nt),
                                                  C.byref(nd))  # synchronises
        if rc == SRD_ERR_ARG and "file_cap" in lib().srd_last_error().decode():
            raise ValueError("the tombstones end beyond the store's capacity")
        _check(rc)
        idx._used = int(used.value)
        if nd.value:
            idx._live = None  # (duplicates in the list: the count of distinct keys is the table's)
        self._tail = int(nt.value)
        return self._tail

    # -- reads ----------------------------------------------------------------------------

    def _ranges(self, hashes, verify):
        return self.index._ranges_host(self.buf.data_ptr(), self._tail, hashes, verify)

    def _payloads(self, st, en):
        import torch
        hit = [(int(a), int(b)) for a, b in zip(st, en) if a != b]
        if not hit:
            return [None] * len(st)
        flat = torch.cat([self.buf[a:b] for a, b in hit]).cpu().numpy().tobytes()  # one copy to the host
        out, o = [], 0
        for a, b in zip(st, en):
            if a == b:
                out.append(None)
            else:
                out.append(flat[o: o + int(b - a)])
                o += int(b - a)
        return out

    def batch_read(self, keys):
        """DataStoreReader::batch_read (data_store.rs:1105-1109): [payload bytes | None];
        every read verified by its key's own tag."""
        if not len(keys):
            return []
        h = compute_hash_batch(keys, self.ctx)
        return self._payloads(*self._ranges(h, h))

    def batch_read_hashed_keys(self, hashes, non_hashed_keys=None):
        """data_store.rs:1111-1158: with non_hashed_keys each read is verified by
        tag_from_key (:513-521)."""
        if non_hashed_keys is not None:
            _same_len(non_hashed_keys, hashes, "hashed and non-hashed keys")
        if not len(hashes):
            return []
        v = compute_hash_batch(non_hashed_keys, self.ctx) if non_hashed_keys is not None else None
        return self._payloads(*self._ranges(hashes, v))

    def read(self, key: bytes):
        return self.batch_read([key])[0]

    def exists(self, key: bytes) -> bool:
        """DataStoreReader::exists (data_store.rs:1030-1032): read(key).is_some()."""
        return self.read(key) is not None

    # -- verified reads: the payloads gathered and checked on the device --------------------

    def batch_gather(self, keys, flags: int = 0) -> GatherResult:
        """batch_read with EntryHandle::is_valid_checksum on every handle: the
        payloads of `keys` gathered into one device buffer, each checked against
        its stored checksum (every read verified by its key's own tag)."""
        h = compute_hash_batch(keys, self.ctx) if len(keys) else []
        return self.index._gather(self.buf.data_ptr(), self._tail, h, h, flags)

    def batch_gather_hashed_keys(self, hashes, non_hashed_keys=None, flags: int = 0) -> GatherResult:
        """batch_read_hashed_keys (data_store.rs:1111-1158) with the payloads verified."""
        return self.index.batch_gather(self.buf.data_ptr(), self._tail, hashes, non_hashed_keys, flags)

    # -- verified reads into the caller's own tensors -----------------------------------------

    def batch_read_into_hashed_keys(self, hashes, entries, non_hashed_keys=None) -> ScatterResult:
        """batch_read_hashed_keys (data_store.rs:1111-1158) with every payload read
        into the caller's buffers piece by piece, as an EntryStream read does
        (entry_stream.rs:76-91), and checked (EntryHandle::is_valid_checksum):
        entries[i] is a sequence of contiguous tensors of any dtype on the store's
        device, taken as their bytes, in order -- batch_write_stream's rule, the
        tensors being the destinations (one per distinct (data_ptr, nbytes)).
        The look-up and srd_payload_scatter_device run on the device; no payload
        length goes through the host.  ScatterResult.status[i]: GATHER_OK /
        GATHER_BAD_CRC (delivered), GATHER_NONE (no such key: its tensors are left
        alone), SCATTER_BAD_LENGTH (its tensors do not hold exactly the payload's
        bytes: left alone).  Anything that is not such a tensor raises ValueError
        before any call; a tensor inside the store's own buffer raises SrdError."""
        if not len(entries) and not len(hashes):
            return ScatterResult(np.zeros(0, np.uint8), np.zeros(0, np.uint32))
        return self.index.batch_scatter(self.buf.data_ptr(), self._tail, hashes, entries, non_hashed_keys)

    def batch_read_into(self, keys, entries) -> ScatterResult:
        """batch_read (data_store.rs:1105-1109) into the caller's tensors, each entry
        an EntryStream read (entry_stream.rs:76-91): compute_hash_batch, then
        batch_read_into_hashed_keys with every read verified by its key's own tag."""
        _same_len(keys, entries, "keys and entries")
        if not len(keys):
            return ScatterResult(np.zeros(0, np.uint8), np.zeros(0, np.uint32))
        h = compute_hash_batch(keys, self.ctx)
        return self.index._scatter(self.buf.data_ptr(), self._tail, h, h, entries)

    def read_into(self, key: bytes, segments) -> int:
        """One entry read into `segments` (entry_stream.rs:76-91): its status."""
        return int(self.batch_read_into([key], [segments]).status[0])

    def verify(self, keys):
        """The batched is_valid_checksum of `keys` (no payload is copied):
        [True | False | None (no such key)] in query order."""
        return self.batch_gather(keys, GATHER_VERIFY_ONLY).is_valid_checksum()

    # -- verified reads into fixed-size rows: no host wait, graph-replayable -------------------

    def _rows_file_len(self) -> int:
        """The buffer's capacity bound: the largest L with padded_size(L) <= buf.numel()."""
        return max(self.buf.numel() // 4096 - 2, 0) * 4096

    def batch_read_rows_hashed_keys(self, hashes, out, non_hashed_keys=None, **outs) -> RowsResult:
        """batch_read_hashed_keys (data_store.rs:1111-1158) into the rows of `out`,
        each payload checked (EntryHandle::is_valid_checksum): DeviceIndex.read_rows
        over the session's buffer -- its contract, stream rule and keyword outputs
        (lens, status, crc, counts) word for word.  No host wait happens anywhere in
        the call when `hashes` (and `non_hashed_keys`, if given) are device tensors.
        What is passed as the read bound is the buffer's CAPACITY bound (the
        largest L with padded_size(L) <= buf.numel()), not the tail: the session's
        index only ever points below the tail and no read leaves the buffer either
        way, so the results are the same -- and a graph captured around this call
        (after sync() and reserve_rows()) sees, when replayed, the entries appended
        and deleted since.  A captured read is valid while rows_token() is
        unchanged: DeviceIndex.grow, a write that grows the table, compact and
        reserve move the table or the buffer (documented, not enforced)."""
        return self.index.read_rows(self.buf.data_ptr(), self._rows_file_len(), hashes, out, non_hashed_keys, **outs)

    def batch_read_rows(self, keys, out) -> RowsResult:
        """batch_read (data_store.rs:1105-1109) into the rows of `out`:
        compute_hash_batch of the host keys (which waits), then
        batch_read_rows_hashed_keys with every read verified by its key's own tag."""
        import torch
        if len(keys) != out.shape[0]:
            raise ValueError("Mismatched lengths for keys and rows.")
        h = self.index._as_dev(compute_hash_batch(keys, self.ctx)) if len(keys) else \
            torch.empty(0, dtype=torch.int64, device=self.buf.device)
        return self.batch_read_rows_hashed_keys(h, out, h)

    def reserve_rows(self, n: int, row_cap: int) -> None:
        """Context.reserve_rows: the workspace for rows reads of at most n keys into
        rows of at most row_cap bytes (what a capture needs beforehand)."""
        self.ctx.reserve_rows(n, row_cap)

    def sync(self) -> None:
        """The host waits for the context stream: everything the session's writes
        and deletes enqueued has landed (call it before capturing a rows read and
        before replaying one after a write)."""
        self.index._sync_lib()

    def rows_token(self):
        """(table ptr, table bytes, buffer ptr): a captured rows read is valid
        while this is unchanged."""
        return (self.index.table.data_ptr(), self.index.nbytes, self.buf.data_ptr())

    def iter_gather(self) -> GatherResult:
        """Every live payload in EntryIterator order (newest first), gathered and
        verified: the index's export, srd_iter_entries_device, then the gather of
        its ranges."""
        st, en, _mo, _kh = self._live_entries()
        return gather_ranges(self.buf.data_ptr(), self._tail, st, en, 0, self.ctx)

    def _live_entries(self):
        """The live index's export, then srd_iter_entries_device over it: device
        int64 tensors (start, end, meta_off, key_hash), newest first."""
        _k, p = self.index.export()  # synchronises
        return _iter_entries(self.buf.data_ptr(), self._tail, p.data_ptr(), p.numel(), self.ctx)

    def iter_entries(self):
        """iter_entries (data_store.rs:276-280) over the live index: numpy arrays
        (start, end, meta_off, key_hash), newest first (EntryIterator order)."""
        return tuple(t.cpu().numpy().view(np.uint64) for t in self._live_entries())

    # -- TTL entries (StorageCacheExt, extensions/src/storage_cache_ext.rs:23-107) ------------

    def _ttl_hasher(self) -> NamespaceHasher:
        if getattr(self, "_ttl_ns", None) is None:
            self._ttl_ns = NamespaceHasher(TTL_PREFIX, self.ctx)
        return self._ttl_ns

    @staticmethod
    def _ttl_expiries(n: int, ttl_secs, now) -> list[int]:
        """now_secs.saturating_add(ttl_secs) (storage_cache_ext.rs:36-41), ttl_secs one number or one per key."""
        now = int(time.time()) if now is None else int(now)
        ttl = [int(ttl_secs)] * n if isinstance(ttl_secs, (int, np.integer)) else [int(t) for t in ttl_secs]
        if len(ttl) != n:
            raise ValueError("Mismatched lengths for keys and ttl_secs.")
        if now < 0 or now > U64_MAX or any(t < 0 or t > U64_MAX for t in ttl):
            raise ValueError("now and ttl_secs must fit an unsigned 64-bit integer")
        return [min(now + t, U64_MAX) for t in ttl]

    def batch_write_with_ttl(self, keys, values, ttl_secs, now=None) -> int:
        """write_with_ttl (storage_cache_ext.rs:23-58) of every key: the payload
        le64(expiry) || value (host bytes) under the hash of the key's namespaced
        key, through batch_write_with_key_hashes.  Returns the new tail."""
        _same_len(keys, values, "keys and values")
        if not len(keys):
            return self._tail
        exp = self._ttl_expiries(len(keys), ttl_secs, now)
        return self.batch_write_with_key_hashes(self._ttl_hasher().hash_batch(keys),
                                                [e.to_bytes(8, "little") + bytes(v) for e, v in zip(exp, values)], False)

    def write_with_ttl(self, key: bytes, value: bytes, ttl_secs: int, now=None) -> int:
        return self.batch_write_with_ttl([key], [value], ttl_secs, now)

    def batch_write_stream_with_ttl(self, keys, entries, ttl_secs, now=None) -> int:
        """write_with_ttl for values that lie in HBM in pieces (entries[i]:
        batch_write_stream_with_key_hashes' rule): the expiries are one device
        uint64[n], entry i's first segment is its 8 bytes, the value's tensors
        follow -- the segment append as it is.  Returns the new tail."""
        import torch
        _same_len(keys, entries, "keys and entries")
        n = len(keys)
        if not n:
            return self._tail
        dev = self.buf.device
        exp = np.array(self._ttl_expiries(n, ttl_secs, now), np.uint64)
        srcs, segs, first, keep = _segment_table(entries, dev)
        d_exp = torch.from_numpy(exp.view(np.int64)).to(dev)
        with_hdr, hfirst = _header_segments(srcs, segs, first, d_exp)
        return self._append_segments(self._ttl_hasher().hash_batch(keys), srcs, with_hdr, hfirst, (keep, d_exp))

    def _ttl_resolve(self, keys, now):
        """srd_ttl_resolve_keys_device on the context stream: device tensors
        (hashes, start, end, expiry, status, counts) and what must outlive the
        caller's wait.  Nothing waits here."""
        import torch
        idx, dev = self.index, self.buf.device
        kb, ko, kl = _blob(keys)
        n = len(kl)
        d_k, d_o, d_l = torch.from_numpy(kb.copy()).to(dev), idx._as_dev(ko), idx._as_dev(kl)
        h, st, en, ex = (torch.empty(max(n, 1), dtype=torch.int64, device=dev) for _ in range(4))
        status = torch.empty(max(n, 1), dtype=torch.uint8, device=dev)
        counts = torch.empty(4, dtype=torch.int64, device=dev)
        idx._lib_after_torch()
        _check(lib().srd_ttl_resolve_keys_device(
            self.ctx.h, C.c_void_p(idx.table.data_ptr()), idx.nbytes, C.c_void_p(self.buf.data_ptr()), self._tail,
            self._ttl_hasher().prefix_hash, C.c_void_p(d_k.data_ptr()), C.c_void_p(d_o.data_ptr()),
            C.c_void_p(d_l.data_ptr()), n, now, C.c_void_p(h.data_ptr()), C.c_void_p(st.data_ptr()),
            C.c_void_p(en.data_ptr()), C.c_void_p(ex.data_ptr()), C.c_void_p(status.data_ptr()),
            C.c_void_p(counts.data_ptr()), C.c_void_p(self.ctx.stream)))
        return h[:n], st[:n], en[:n], ex[:n], status[:n], counts, (d_k, d_o, d_l)

    def _ttl_evict(self, d_hashes, d_status) -> int:
        """srd_ttl_evict_device: the tombstones of the batch's expired keys, the
        index and the tail.  Returns the number of keys evicted."""
        idx = self.index
        used, nt, nd = C.c_uint64(idx._used), C.c_uint64(), C.c_uint64()
        rc = lib().srd_ttl_evict_device(self.ctx.h, C.c_void_p(idx.table.data_ptr()), idx.nbytes, C.byref(used),
                                        C.c_void_p(d_hashes.data_ptr()), C.c_void_p(d_status.data_ptr()),
                                        d_hashes.numel(), self._tail, C.c_void_p(self.buf.data_ptr()), self.buf.numel(),
                                        C.byref(nt), C.byref(nd))  # synchronises
        if rc == SRD_ERR_ARG and "file_cap" in lib().srd_last_error().decode():
            raise ValueError("the tombstones end beyond the store's capacity")
        _check(rc)
        idx._used = int(used.value)
        if idx._live is not None:
            idx._live -= int(nd.value)  # (every evicted key was live: the resolve found it)
        self._tail = int(nt.value)
        return int(nd.value)

    def batch_read_with_ttl(self, keys, now=None, evict: bool = True) -> "TtlReadResult":
        """read_with_ttl (storage_cache_ext.rs:72-107) of every key at `now`: the
        decision in one launch from the raw keys (srd_ttl_resolve_keys_device),
        the live payloads gathered and checked (srd_payload_gather_device), and
        -- unless evict=False -- one tombstone per distinct expired key
        (srd_ttl_evict_device).  The batch is judged against the store as it is
        when the call starts: an expired key listed twice is EXPIRED twice."""
        now = int(time.time()) if now is None else int(now)
        if not len(keys):
            return TtlReadResult(np.zeros(0, np.uint8), np.zeros(0, np.uint64),
                                 GatherResult(None, np.zeros(1, np.uint64), np.zeros(0, np.uint64), np.zeros(0, np.uint8),
                                              np.zeros(0, np.uint32)))
        h, st, en, ex, status, counts, _keep = self._ttl_resolve(keys, now)
        g = gather_ranges(self.buf.data_ptr(), self._tail, st, en, 0, self.ctx)  # waits
        res = TtlReadResult(status.cpu().numpy(), ex.cpu().numpy().view(np.uint64), g)
        if evict and int(counts[TTL_EXPIRED]):
            res.n_evicted = self._ttl_evict(h, status)
        return res

    def read_with_ttl(self, key: bytes, now=None):
        """read_with_ttl (storage_cache_ext.rs:72-107): the value; None when expired (the entry is deleted);
        KeyError when absent; ValueError("Data too short to contain TTL")."""
        r = self.batch_read_with_ttl([key], now)
        s = int(r.status[0])
        if s == TTL_NOT_FOUND:
            raise KeyError(f"Key not found: {key!r}")
        if s == TTL_TOO_SHORT:
            raise ValueError("Data too short to contain TTL")
        return r.values()[0] if s == TTL_LIVE else None

    def batch_read_with_ttl_into(self, keys, entries, now=None, evict: bool = True) -> "TtlReadResult":
        """batch_read_with_ttl with every live value read into the caller's own
        tensors (entries[i]: batch_read_into's rule): the scatter with one internal
        8-byte destination in front of each query's segments, which takes the
        expiry header.  The result's gather is a ScatterResult."""
        import torch
        _same_len(keys, entries, "keys and entries")
        now = int(time.time()) if now is None else int(now)
        n, dev = len(keys), self.buf.device
        if not n:
            return TtlReadResult(np.zeros(0, np.uint8), np.zeros(0, np.uint64),
                                 ScatterResult(np.zeros(0, np.uint8), np.zeros(0, np.uint32)))
        srcs, segs, first, keep = _segment_table(entries, dev)
        hdr = torch.empty(n, dtype=torch.int64, device=dev)
        with_hdr, hfirst = _header_segments(srcs, segs, first, hdr)
        h, st, en, ex, status, counts, _keep = self._ttl_resolve(keys, now)
        sc = _scatter_table(self.buf.data_ptr(), self._tail, st, en, (srcs, with_hdr, hfirst, (keep, hdr)), self.ctx)
        res = TtlReadResult(status.cpu().numpy(), ex.cpu().numpy().view(np.uint64), sc)
        if evict and int(counts[TTL_EXPIRED]):
            res.n_evicted = self._ttl_evict(h, status)
        return res

    def sweep_expired(self, now=None, plan: bool = False) -> TtlSweepStats:
        """srd_ttl_sweep_device: every live entry judged as a TTL entry at `now`
        (keys are not stored: for stores written only through the TTL writes),
        the expired ones deleted -- tombstones in ascending offset of the entries
        they remove; plan=True reports the counts and writes nothing.  Entries too
        short to hold an expiry are left alone and counted.  `compact` then
        returns the bytes."""
        now = int(time.time()) if now is None else int(now)
        idx = self.index
        used, nt, st = C.c_uint64(idx._used), C.c_uint64(), TtlSweepStats()
        idx._lib_after_torch()
        rc = lib().srd_ttl_sweep_device(self.ctx.h, C.c_void_p(idx.table.data_ptr()), idx.nbytes, C.byref(used),
                                        C.c_void_p(self.buf.data_ptr()), self._tail, self.buf.numel(), now,
                                        TTL_SWEEP_PLAN if plan else 0, C.byref(nt), C.byref(st))  # synchronises
        if rc == SRD_ERR_ARG and "file_cap" in lib().srd_last_error().decode():
            raise ValueError("the tombstones end beyond the store's capacity")
        _check(rc)
        if not plan:
            idx._used = int(used.value)
            if int(nt.value) != self._tail:
                idx._live = int(st.n_judged) - int(st.n_expired)
            self._tail = int(nt.value)
        return st

    # -- compaction and growth --------------------------------------------------------------

    def _compact_plan(self) -> CompactStats:
        idx = self.index
        idx._lib_after_torch()
        return compact_live_device(idx.table.data_ptr(), idx.nbytes, self.buf.data_ptr(), self._tail, ctx=self.ctx)

    def estimate_compaction_savings(self) -> int:
        """estimate_compaction_savings (data_store.rs:605-616): the tail less the
        bytes the live entries need (payload + 20 each), saturating at 0."""
        return max(self._tail - int(self._compact_plan().kept_bytes), 0)

    def compact(self, capacity: int | None = None, allow_bad_crc: bool = False) -> CompactStats:
        """DataStore::compact (data_store.rs:706-749) of the session, on the device
        (srd_compact_live_device): every live entry, newest first, re-written from
        offset 0 into a new buffer of padded_size(capacity) bytes (default: the
        current buffer's size) with its checksum recomputed, and the index rebuilt
        for the new offsets; then buffer, tail and index table are replaced in one
        step.  Both buffers -- and both tables -- are held in HBM during the call.
        A key whose indexed entry is a tombstone on disk (such keys can only come
        from `open`) disappears from len(), as it would on re-opening the compacted
        file in the reference.  ValueError when the compacted store does not fit the
        capacity, and -- unless allow_bad_crc -- when a live payload's recomputed
        CRC differs from its stored checksum (the message names n_crc_bad and
        first_bad, the first such entry's metadata offset in the old store; the
        reference would silently give it a fresh, matching checksum); SrdError for
        the library's refusals (a live payload of NULL bytes only).  Any error
        leaves the session exactly as it was: same buffer, tail and table."""
        import torch
        idx = self.index
        plan = self._compact_plan()
        nbytes = padded_size(capacity) if capacity is not None else self.buf.numel()
        if padded_size(int(plan.new_len)) > nbytes:
            raise ValueError(f"the compacted store ends at {int(plan.new_len)}: beyond the capacity")
        dev = self.buf.device
        buf = torch.zeros(nbytes, dtype=torch.uint8, device=dev)
        tbytes = int(lib().srd_index_table_bytes(max(int(plan.n_entries), 1)))
        table = torch.empty(tbytes, dtype=torch.uint8, device=dev)
        idx._lib_after_torch()  # (behind torch's zero fill)
        st = compact_live_device(idx.table.data_ptr(), idx.nbytes, self.buf.data_ptr(), self._tail, buf.data_ptr(),
                                 nbytes, table.data_ptr(), tbytes, self.ctx)  # synchronises
        if st.n_crc_bad and not allow_bad_crc:
            raise ValueError(f"live payloads fail their stored checksum: n_crc_bad = {int(st.n_crc_bad)}, first_bad = "
                             f"{int(st.first_bad)} (its metadata offset); compact(allow_bad_crc=True) keeps them")
        n = int(st.n_entries)
        self.buf, self._tail = buf, int(st.new_len)
        idx.table, idx.nbytes, idx.n, idx._used, idx._live = table, tbytes, n, n, n
        return st

    def reserve(self, capacity: int) -> None:
        """A buffer that can grow to `capacity` bytes: a new zeroed tensor, the
        bytes [0, padded_size(tail)) copied on the device, then the swap.  For when
        the live data itself has outgrown the buffer (dead space: `compact`).
        ValueError when capacity is below the tail."""
        import torch
        if capacity < self._tail:
            raise ValueError(f"capacity {capacity} is below the tail {self._tail}")
        buf = torch.zeros(padded_size(capacity), dtype=torch.uint8, device=self.buf.device)
        n = min(padded_size(self._tail), self.buf.numel(), buf.numel())
        self.index._sync_lib()  # what the library wrote has landed before torch reads it
        buf[:n].copy_(self.buf[:n])
        self.buf = buf
