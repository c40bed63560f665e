"""What the device append costs: payloads that lie in a
device blob appended to an empty store in HBM by srd_batch_append_device, and
alongside, interleaved in the same process, the paths next to it -- the same
call under SRD_APPEND_STREAM_RULE, srd_batch_write_device on the same entries
(its host layout and entry table made outside the timed window) and the
runtime's device-to-device copy of the same byte count:

  a  1024 x 4 KiB: the call's fixed cost;
  c  2^20 x 4 KiB: the C5 bytes from HBM;
  d  8 x 256 MiB: few and large payloads, one wave per entry against chunk units
     (the writer baseline runs --writer-reps-d times only: a quarter of a second each);
  e  2^20 x 8 B: the reference's storage_benchmark shape, one wave per tiny unit.

Library calls are timed with device events on the context stream (an append's
one host wait is inside its window) and with the host clock ending in a
synchronise; warm-ups first, then median [min, max].  Every case first checks
that the append and the writer produced the same store bytes.  One JSON line.

--src-residue K moves every payload K bytes up inside the blob (K = 1..15: no
source is 16-byte aligned to its destination slot).

usage: python tools/append_bench.py [--cases acde] [--reps R] [--warmup W] [--src-residue K] [--out FILE]"""
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

ENTRY = np.dtype([("src", "<u8"), ("len", "<u8"), ("key_src", "<u8"), ("tail", "<u8"), ("key_len", "<u4"), ("flags", "<u4")])


def stats(x):
    return {"median": round(statistics.median(x), 4), "min": round(min(x), 4), "max": round(max(x), 4), "n": len(x)}


def gbps(nbytes, st):
    return {k: round(2 * nbytes / (st[j] * 1e6), 1) for k, j in (("median", "median"), ("best", "min"), ("worst", "max"))}


class Bench:
    def __init__(self, ctx, residue=0):
        self.ctx, self.L, self.residue = ctx, S.lib(), residue
        self.stream = torch.cuda.ExternalStream(ctx.stream)

    def timed(self, fn):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        e0.record(self.stream)
        fn()
        e1.record(self.stream)
        e1.synchronize()
        return e0.elapsed_time(e1), (time.perf_counter() - t0) * 1e3

    def case(self, n, length, reps, warmup, writer_reps=None):
        """n payloads of `length` bytes, back to back at 16-byte boundaries (+ the residue) of one device blob."""
        stride = (length + 15) & ~15
        lens = np.full(n, length, np.uint64)
        offs = np.arange(n, dtype=np.uint64) * np.uint64(stride) + np.uint64(self.residue)
        hashes = (np.arange(n, dtype=np.uint64) + np.uint64(1)) * np.uint64(0x9E3779B97F4A7C15)
        blob = torch.randint(1, 256, (n * stride + 16,), dtype=torch.uint8, device="cuda")
        nbytes = n * length
        # the writer's host layout and entry table (outside every timed window)
        ent = np.zeros(n, ENTRY)
        zero = np.zeros(n, np.uint64)
        nt = C.c_uint64()
        S._check(self.L.srd_batch_layout(0, None, S._ptr(zero), S._ptr(zero), S._ptr(offs), S._ptr(lens), n, 0,
                                         C.c_void_p(ent.ctypes.data), C.byref(nt)))
        ent["key_src"], ent["key_len"], ent["flags"] = hashes, 0, 2  # SRD_ENTRY_HASHED
        new_tail = int(nt.value)
        cap = S.padded_size(new_tail)
        out_a = torch.zeros(cap, dtype=torch.uint8, device="cuda")
        out_w = torch.zeros(cap, dtype=torch.uint8, device="cuda")
        d_ent = torch.from_numpy(ent.view(np.uint8)).cuda()
        d_o, d_l, d_h = (torch.from_numpy(x.view(np.int64)).cuda() for x in (offs, lens, hashes))
        mo_a = torch.empty(n, dtype=torch.int64, device="cuda")
        kh_w, mo_w = torch.empty_like(mo_a), torch.empty_like(mo_a)
        got = C.c_uint64()

        def append_fn(flags):
            def fn():
                S._check(self.L.srd_batch_append_device(
                    self.ctx.h, C.c_void_p(blob.data_ptr()), blob.numel(), C.c_void_p(d_o.data_ptr()),
                    C.c_void_p(d_l.data_ptr()), C.c_void_p(d_h.data_ptr()), n, flags, 0, C.c_void_p(out_a.data_ptr()), cap,
                    C.byref(got), C.c_void_p(mo_a.data_ptr()), C.c_void_p(self.ctx.stream)))
            return fn

        def writer_fn():
            S._check(self.L.srd_batch_write_device(
                self.ctx.h, C.c_void_p(blob.data_ptr()), C.c_void_p(blob.data_ptr()), C.c_void_p(d_ent.data_ptr()), n,
                C.c_void_p(out_w.data_ptr()), 0, C.c_void_p(kh_w.data_ptr()), C.c_void_p(mo_w.data_ptr()),
                C.c_void_p(self.ctx.stream)))

        def memcpy_fn():
            # torch's copy of a contiguous uint8 range on one device is the runtime's own
            # device-to-device hipMemcpyAsync, here on the context stream
            with torch.cuda.stream(self.stream):
                out_w[:nbytes].copy_(blob[self.residue: self.residue + nbytes])

        plain, rule = append_fn(0), append_fn(S.APPEND_STREAM_RULE)
        # the same bytes and offsets from both paths, before anything is timed
        self.timed(memcpy_fn)
        self.timed(writer_fn)
        self.timed(plain)
        assert int(got.value) == new_tail
        assert torch.equal(out_a[:new_tail], out_w[:new_tail]) and torch.equal(mo_a, mo_w), "append != writer"
        wr = reps if writer_reps is None else writer_reps
        ta, tr, tw, tm = [], [], [], []
        for r in range(warmup + reps):  # interleaved
            x, y, z = self.timed(plain), self.timed(rule), self.timed(memcpy_fn)
            w = self.timed(writer_fn) if r < warmup + wr else None
            if r >= warmup:
                ta.append(x), tr.append(y), tm.append(z)
                if w:
                    tw.append(w)
        sa, sr, sw, sm = (stats([t[0] for t in x]) for x in (ta, tr, tw, tm))
        return {"entries": n, "payload_len": length, "payload_bytes": nbytes, "new_tail": new_tail,
                "append_event_ms": sa, "append_host_ms": stats([t[1] for t in ta]), "append_GBps_rw": gbps(nbytes, sa),
                "append_stream_rule_event_ms": sr, "writer_event_ms": sw, "writer_GBps_rw": gbps(nbytes, sw),
                "memcpy_dtod_event_ms": sm, "memcpy_GBps_rw": gbps(nbytes, sm),
                "append_over_memcpy": round(sa["median"] / sm["median"], 3),
                "append_over_writer": round(sa["median"] / sw["median"], 3),
                "writer_over_memcpy": round(sw["median"] / sm["median"], 3),
                "stream_rule_over_append": round(sr["median"] / sa["median"], 3)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--cases", default="acde")
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--writer-reps-d", type=int, default=2)
    ap.add_argument("--src-residue", type=int, default=0, choices=range(16))
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    ctx = S.Context(0)
    B = Bench(ctx, a.src_residue)
    res = {"chunk": S.GATHER_CHUNK, "lib": S.build_info(), "src_residue": a.src_residue,
           "memcpy": "hipMemcpyAsync device-to-device (torch copy_ of a contiguous range)"}
    shapes = {"a": (1024, 4096, None), "c": (1 << 20, 4096, None), "d": (8, 256 << 20, a.writer_reps_d),
              "e": (1 << 20, 8, None)}
    for case in a.cases:
        n, length, wr = shapes[case]
        res[case] = B.case(n, length, a.reps, a.warmup, wr)
        torch.cuda.empty_cache()
    line = json.dumps(res)
    print(line)
    if a.out:
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
