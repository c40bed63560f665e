"""What the incremental index path buys: on a C2 store
(2^20 keys x 4 KiB) resident in HBM, the time of DeviceIndex.apply's C call for
one 1024-pair batch (the reference bench's batch size: 512 overwrites of
existing keys + 512 new keys) against the only way to reach the same state
without it -- srd_validate_index_device + srd_index_table_build_device.

Both are timed with device events on the context stream around the library
calls (so an apply's one host wait for its counts is inside its window) and
with the host clock around the same calls ending in a synchronise; warm-ups
first, then the median / min / max over the repetitions.  One JSON line.

usage: python tools/live_apply_bench.py [--entries N] [--reps R] [--out FILE]"""
import argparse
import ctypes as C
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "rust-simd-r-drive_amd"))

import numpy as np  # noqa: E402
import torch  # noqa: E402

import srd_amd as S  # noqa: E402


def stats(x):
    return {"median": round(statistics.median(x), 4), "min": round(min(x), 4), "max": round(max(x), 4), "n": len(x)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--entries", type=int, default=1 << 20)
    ap.add_argument("--batch", type=int, default=1024)
    ap.add_argument("--reps", type=int, default=50)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    ctx = S.Context(0)
    L = S.lib()
    flen = S.synth_store_len(a.entries)
    dev = torch.zeros(S.padded_size(flen), dtype=torch.uint8, device="cuda")
    S.synth_store_device(dev.data_ptr(), a.entries, ctx=ctx)
    torch.cuda.synchronize()
    lib_stream = torch.cuda.ExternalStream(ctx.stream)

    def timed(fn):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        lib_stream.synchronize()
        t0 = time.perf_counter()
        e0.record(lib_stream)
        fn()
        e1.record(lib_stream)
        e1.synchronize()
        return e0.elapsed_time(e1), (time.perf_counter() - t0) * 1e3

    # the parent's way: open the store again and adopt the index
    table = torch.empty(int(L.srd_index_table_bytes(a.entries)), dtype=torch.uint8, device="cuda")
    res = {}

    def reopen():
        r = S.validate_index_device(dev.data_ptr(), flen, 0, ctx)
        S._check(L.srd_index_table_build_device(ctx.h, C.c_void_p(r.index_key_hash), C.c_void_p(r.index_packed),
                                                r.n_index, C.c_void_p(table.data_ptr()), table.numel()))
        res["n"] = r.n_index

    ro = [timed(reopen) for _ in range(a.warmup + 10)][a.warmup:]
    assert res["n"] == a.entries

    r = S.validate_index_device(dev.data_ptr(), flen, 0, ctx)
    idx = S.DeviceIndex(r.index_key_hash, r.index_packed, r.n_index, ctx)
    have = S.device_view(r.index_key_hash, r.n_index).clone()
    idx.grow(2 * a.entries)  # room for the new keys of every repetition
    rng = np.random.default_rng(7)
    half = a.batch // 2
    ap_t = []
    for rep in range(a.warmup + a.reps):
        pick = torch.from_numpy(rng.choice(a.entries, half, replace=False)).cuda()
        new = torch.from_numpy(rng.integers(0, 1 << 63, a.batch - half, dtype=np.int64)).cuda()
        kh = torch.cat([have[pick], new])[torch.randperm(a.batch, device="cuda")].contiguous()
        mo = (flen + 21 * (rep * a.batch + torch.arange(a.batch, device="cuda"))).contiguous()
        used, st = C.c_uint64(idx.used), S.ApplyStats()
        idx._lib_after_torch()

        def apply():
            S._check(L.srd_index_table_apply_device(ctx.h, C.c_void_p(idx.table.data_ptr()), idx.nbytes, C.byref(used),
                                                    C.c_void_p(kh.data_ptr()), C.c_void_p(mo.data_ptr()), None, a.batch,
                                                    C.byref(st), C.c_void_p(ctx.stream)))

        t = timed(apply)
        assert st.n_updated == half and st.n_inserted == a.batch - half, st.as_tuple()
        idx._used = int(used.value)
        if rep >= a.warmup:
            ap_t.append(t)
    line = json.dumps({
        "entries": a.entries, "file_len": flen, "batch": a.batch, "table_capacity": idx.capacity,
        "apply_event_ms": stats([t[0] for t in ap_t]), "apply_host_ms": stats([t[1] for t in ap_t]),
        "reopen_event_ms": stats([t[0] for t in ro]), "reopen_host_ms": stats([t[1] for t in ro]),
        "lib": S.build_info(),
    })
    print(line)
    if a.out:
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
