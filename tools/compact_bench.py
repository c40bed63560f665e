"""What compacting a live session costs: a store in HBM
with its live index table, compacted by srd_compact_live_device, and alongside,
interleaved in the same process, the route there was before it --
srd_index_table_export_device + srd_compact_device + the packing of its (key
hash, offset) outputs + srd_index_table_build_device -- and the runtime's
device-to-device copy of new_len bytes as the floor:

  a  1024 x 4 KiB, all live: the call's fixed cost;
  c  2^19 keys x 4 KiB, each written twice: half the store is dead, ~2.15 GB moves;
  d  8 live + 8 superseded payloads of 256 MiB: few and large entries, one wave
     per entry against chunk units (the old route runs --old-reps-d times only).

Every call is timed with device events on the context stream (the calls' host
waits are inside their windows); warm-ups first, then median [min, max].  Every
case first checks that both routes wrote identical bytes and built tables with
identical exports.  Each case runs in a process of its own; one JSON line each.

usage: python tools/compact_bench.py [--cases acd] [--reps R] [--warmup W] [--out FILE]"""
import argparse
import ctypes as C
import json
import os
import statistics
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "rust-simd-r-drive_amd"))

SHAPES = {"a": (1024, 4096, 1), "c": (1 << 19, 4096, 2), "d": (8, 256 << 20, 2)}  # keys, payload length, writes per key


def stats(x):
    return {"median": round(statistics.median(x), 4), "min": round(min(x), 4), "max": round(max(x), 4), "n": len(x)}


def run_case(case, reps, warmup, old_reps_d):
    import numpy as np
    import torch

    import srd_amd as S

    n, length, writes = SHAPES[case]
    ctx = S.Context(0)
    L = S.lib()
    stream = torch.cuda.ExternalStream(ctx.stream)
    vp = C.c_void_p

    # the session: every key written `writes` times from a blob of random bytes in HBM
    stride = (length + 15) & ~15
    slot = (length + 20 + 63) & ~63
    st = S.DeviceStore.create(writes * n * slot + 4096, ctx)
    hashes = (np.arange(n, dtype=np.uint64) + np.uint64(1)) * np.uint64(0x9E3779B97F4A7C15)
    offs = np.arange(n, dtype=np.uint64) * np.uint64(stride)
    lens = np.full(n, length, np.uint64)
    for _ in range(writes):
        blob = torch.randint(1, 256, (n * stride,), dtype=torch.uint8, device="cuda")
        st.batch_write_device_with_key_hashes(hashes, blob, offs, lens)
        del blob
    torch.cuda.empty_cache()
    idx = st.index
    assert st.len() == n

    plan = S.compact_live_device(idx.table.data_ptr(), idx.nbytes, st.buf.data_ptr(), st.tail, ctx=ctx)
    new_len = int(plan.new_len)
    assert int(plan.n_entries) == n and new_len == (n - 1) * slot + length + 20
    cap = S.padded_size(new_len)
    tbytes = int(L.srd_index_table_bytes(n))
    out_a = torch.zeros(cap, dtype=torch.uint8, device="cuda")
    out_b = torch.zeros(cap, dtype=torch.uint8, device="cuda")
    tab_a = torch.empty(tbytes, dtype=torch.uint8, device="cuda")
    tab_b = torch.empty(tbytes, dtype=torch.uint8, device="cuda")
    xk, xp = (torch.empty(n, dtype=torch.int64, device="cuda") for _ in range(2))
    kh_b, mo_b = (torch.empty(n, dtype=torch.int64, device="cuda") for _ in range(2))
    got, nl = C.c_uint64(), C.c_uint64()
    cs = S.CompactStats()

    def live_fn():
        S._check(L.srd_compact_live_device(ctx.h, vp(idx.table.data_ptr()), idx.nbytes, vp(st.buf.data_ptr()), st.tail,
                                           vp(out_a.data_ptr()), cap, vp(tab_a.data_ptr()), tbytes, C.byref(cs)))

    def old_fn():
        S._check(L.srd_index_table_export_device(ctx.h, vp(idx.table.data_ptr()), idx.nbytes, vp(xk.data_ptr()),
                                                 vp(xp.data_ptr()), n, C.byref(got)))
        S._check(L.srd_compact_device(ctx.h, vp(st.buf.data_ptr()), st.tail, vp(xp.data_ptr()), n, vp(out_b.data_ptr()),
                                      cap, C.byref(nl), vp(kh_b.data_ptr()), vp(mo_b.data_ptr())))
        with torch.cuda.stream(stream):  # KeyIndexer::pack of the writer's outputs, on the context stream
            packed = ((kh_b >> 48) << 48) | mo_b
        S._check(L.srd_index_table_build_device(ctx.h, vp(kh_b.data_ptr()), vp(packed.data_ptr()), n,
                                                vp(tab_b.data_ptr()), tbytes))

    def memcpy_fn():
        # torch's copy of a contiguous uint8 range on one device is the runtime's own
        # device-to-device hipMemcpyAsync, here on the context stream
        with torch.cuda.stream(stream):
            out_b[:new_len].copy_(st.buf[:new_len])

    def timed(fn):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        torch.cuda.synchronize()
        e0.record(stream)
        fn()
        e1.record(stream)
        e1.synchronize()
        return e0.elapsed_time(e1)

    def export(tab):
        k, p = torch.empty_like(xk), torch.empty_like(xp)
        S._check(L.srd_index_table_export_device(ctx.h, vp(tab.data_ptr()), tbytes, vp(k.data_ptr()), vp(p.data_ptr()), n,
                                                 C.byref(got)))
        assert int(got.value) == n
        return k, p

    # identical bytes and identical table exports from both routes, before anything is timed
    timed(memcpy_fn)
    timed(old_fn)
    timed(live_fn)
    assert int(cs.new_len) == int(nl.value) == new_len and int(cs.n_crc_bad) == 0
    assert torch.equal(out_a[:new_len], out_b[:new_len]), "live compaction != export + srd_compact_device"
    (ka, pa), (kb, pb) = export(tab_a), export(tab_b)
    assert torch.equal(ka, kb) and torch.equal(pa, pb), "the two routes' tables differ"
    old_reps = old_reps_d if case == "d" else reps
    tl, to, tm = [], [], []
    for r in range(warmup + reps):  # interleaved
        x, z = timed(live_fn), timed(memcpy_fn)
        y = timed(old_fn) if r < warmup + old_reps else None
        if r >= warmup:
            tl.append(x), tm.append(z)
            if y is not None:
                to.append(y)
    sl, so, sm = stats(tl), stats(to), stats(tm)
    return {"case": case, "keys": n, "payload_len": length, "writes_per_key": writes, "store_len": st.tail,
            "new_len": new_len, "chunk": S.GATHER_CHUNK, "lib": S.build_info(),
            "compact_live_event_ms": sl, "export_compact_pack_build_event_ms": so, "memcpy_dtod_event_ms": sm,
            "live_GBps_rw": round(2 * new_len / (sl["median"] * 1e6), 1),
            "live_over_memcpy": round(sl["median"] / sm["median"], 3),
            "old_over_memcpy": round(so["median"] / sm["median"], 3),
            "old_over_live": round(so["median"] / sl["median"], 3),
            "memcpy": "hipMemcpyAsync device-to-device (torch copy_ of a contiguous range)"}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--cases", default="acd")
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--old-reps-d", type=int, default=2)
    ap.add_argument("--out", default=None)
    ap.add_argument("--one", default=None, help=argparse.SUPPRESS)  # a child: this case, in this process
    a = ap.parse_args()
    if a.one:
        print(json.dumps(run_case(a.one, a.reps, a.warmup, a.old_reps_d)))
        return
    lines = []
    for case in a.cases:  # each case in a process of its own
        out = subprocess.check_output([sys.executable, os.path.abspath(__file__), "--one", case, "--reps", str(a.reps),
                                       "--warmup", str(a.warmup), "--old-reps-d", str(a.old_reps_d)], text=True)
        lines.append(out.strip().splitlines()[-1])
        print(lines[-1], flush=True)
    if a.out:
        with open(a.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
