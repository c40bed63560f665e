"""What writing entries from device segments costs:
payloads that lie in HBM in pieces appended to an empty store by
srd_batch_append_segments_device, and alongside, interleaved in the same
process, the routes next to it:

  segments  the new call over the pieces where they lie;
  append    srd_batch_append_device under SRD_APPEND_STREAM_RULE over the same
            bytes laid contiguous beforehand (the floor for this machinery: the
            copy that makes them contiguous is outside its window);
  cat       the route there was before: torch.cat of the pieces into one blob,
            inside the window, then that append (per entry into a 16-aligned
            slot; cases a, b, f: one cat of all pieces, whose entries land
            16-aligned by their lengths);
  memcpy    the runtime's device-to-device copy of the same byte count.

  a  2^19 x 4 KiB, one segment each;
  b  2^19 x (64 B header + 4032 B body), both 16-aligned;
  c  8 x (64 B header + 256 MiB body);
  d  8 x (20 B header + 256 MiB body): the realigning path;
  e  8 x (64 B header + 256 MiB body at source residue 1): the realigning path;
  f  1024 entries x 64 pages of 16 KiB, scattered over a pool.

Every route is timed with device events on the context stream (the calls' host
waits are inside their windows); warm-ups first, then median [min, max].  Every
case first checks that the routes wrote identical store bytes.  One JSON line.

usage: python tools/segments_bench.py [--cases abcdef] [--reps R] [--warmup W] [--shift K] [--out FILE]
(--shift K divides the entry counts of a, b, f and the body size of c, d, e by 2^K: a quick look)"""
import argparse
import ctypes as C
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "rust-simd-r-drive_amd"))

import numpy as np  # noqa: E402
import torch  # noqa: E402

import srd_amd as S  # noqa: E402

SEG = np.dtype([("src", "<u4"), ("reserved", "<u4"), ("off", "<u8"), ("len", "<u8")])


def stats(x):
    return {"median": round(statistics.median(x), 4), "min": round(min(x), 4), "max": round(max(x), 4), "n": len(x)}


def dev_i64(a):
    return torch.from_numpy(np.ascontiguousarray(a, np.uint64).view(np.int64)).cuda()


def rand(n):
    return torch.randint(1, 256, (n,), dtype=torch.uint8, device="cuda")


def shapes(case, shift):
    """(sources, segment table, first, per-entry cat): the case's pieces in HBM."""
    if case in "ab":
        n = (1 << 19) >> shift
        if case == "a":
            srcs = [rand(n * 4096)]
            seg = np.zeros(n, SEG)
            seg["off"], seg["len"] = np.arange(n, dtype=np.uint64) * 4096, 4096
            return srcs, seg, np.arange(n + 1, dtype=np.uint64), False
        srcs = [rand(n * 64), rand(n * 4032)]
        seg = np.zeros(2 * n, SEG)
        seg["src"] = np.tile([0, 1], n)
        seg["len"] = np.tile([64, 4032], n)
        seg["off"][0::2], seg["off"][1::2] = np.arange(n, dtype=np.uint64) * 64, np.arange(n, dtype=np.uint64) * 4032
        return srcs, seg, np.arange(n + 1, dtype=np.uint64) * 2, False
    if case in "cde":
        n, body = 8, (256 << 20) >> shift
        head, res = (20, 0) if case == "d" else (64, 1 if case == "e" else 0)
        srcs = [rand(n * head)] + [rand(body + 16)[res: res + body] for _ in range(n)]
        seg = np.zeros(2 * n, SEG)
        seg["src"][1::2] = np.arange(1, n + 1)
        seg["off"][0::2] = np.arange(n, dtype=np.uint64) * head
        seg["len"] = np.tile([head, body], n)
        return srcs, seg, np.arange(n + 1, dtype=np.uint64) * 2, True
    n, pages, page = 1024 >> shift, 64, 16384
    srcs = [rand(n * pages * page)]
    seg = np.zeros(n * pages, SEG)
    seg["off"] = np.random.default_rng(0xF).permutation(n * pages).astype(np.uint64) * page
    seg["len"] = page
    return srcs, seg, np.arange(n + 1, dtype=np.uint64) * pages, False


class Bench:
    def __init__(self, ctx):
        self.ctx, self.L = ctx, S.lib()
        self.stream = torch.cuda.ExternalStream(ctx.stream)

    def timed(self, fn):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        torch.cuda.synchronize()
        e0.record(self.stream)
        fn()
        e1.record(self.stream)
        e1.synchronize()
        return e0.elapsed_time(e1)

    def case(self, name, shift, reps, warmup):
        srcs, seg, first, per_entry = shapes(name, shift)
        n = len(first) - 1
        lens = np.add.reduceat(seg["len"], first[:-1].astype(np.int64)).astype(np.uint64)
        nbytes = int(lens.sum())
        # the contiguous layout: every entry at a 16-byte boundary of one blob
        offs = np.zeros(n, np.uint64)
        offs[1:] = np.cumsum((lens + np.uint64(15)) & ~np.uint64(15))[:-1]
        blob_len = int(offs[-1] + lens[-1])
        assert per_entry or blob_len == nbytes
        parts = [srcs[int(s)][int(o): int(o) + int(ln)] for s, o, ln in zip(seg["src"], seg["off"], seg["len"])]
        hashes = (np.arange(n, dtype=np.uint64) + np.uint64(1)) * np.uint64(0x9E3779B97F4A7C15)
        d_seg = torch.from_numpy(seg.view(np.uint8).copy()).cuda()
        d_first, d_h, d_o, d_l = dev_i64(first), dev_i64(hashes), dev_i64(offs), dev_i64(lens)
        ptrs = (C.c_void_p * len(srcs))(*[t.data_ptr() for t in srcs])
        slens = (C.c_uint64 * len(srcs))(*[t.numel() for t in srcs])
        cap = S.padded_size(nbytes + 84 * n + 64)
        out_s, out_a, out_c = (torch.zeros(cap, dtype=torch.uint8, device="cuda") for _ in range(3))
        blob = torch.empty(blob_len, dtype=torch.uint8, device="cuda")   # the floor's, filled once below
        blob_c = torch.empty(blob_len, dtype=torch.uint8, device="cuda")  # the cat route's, filled in its window
        mo_s, mo_a = torch.empty(n, dtype=torch.int64, device="cuda"), torch.empty(n, dtype=torch.int64, device="cuda")
        got = C.c_uint64()

        def cat_into(b):
            with torch.cuda.stream(self.stream):
                if per_entry:
                    for i in range(n):
                        o, ln = int(offs[i]), int(lens[i])
                        torch.cat(parts[int(first[i]): int(first[i + 1])], out=b[o: o + ln])
                else:
                    torch.cat(parts, out=b)

        def append_of(b, out):
            S._check(self.L.srd_batch_append_device(
                self.ctx.h, C.c_void_p(b.data_ptr()), b.numel(), C.c_void_p(d_o.data_ptr()), C.c_void_p(d_l.data_ptr()),
                C.c_void_p(d_h.data_ptr()), n, S.APPEND_STREAM_RULE, 0, C.c_void_p(out.data_ptr()), cap, C.byref(got),
                C.c_void_p(mo_a.data_ptr()), C.c_void_p(self.ctx.stream)))

        def segments_fn():
            S._check(self.L.srd_batch_append_segments_device(
                self.ctx.h, ptrs, slens, len(srcs), C.c_void_p(d_seg.data_ptr()), len(seg), C.c_void_p(d_first.data_ptr()),
                C.c_void_p(d_h.data_ptr()), n, 0, 0, C.c_void_p(out_s.data_ptr()), cap, C.byref(got),
                C.c_void_p(mo_s.data_ptr()), C.c_void_p(self.ctx.stream)))

        def append_fn():
            append_of(blob, out_a)

        def cat_fn():
            cat_into(blob_c)
            append_of(blob_c, out_c)

        def memcpy_fn():
            with torch.cuda.stream(self.stream):
                out_c[:nbytes].copy_(blob[:nbytes] if blob_len >= nbytes else blob)

        # identical store bytes from every route, before anything is timed
        self.timed(lambda: cat_into(blob))
        self.timed(segments_fn)
        nt = int(got.value)
        self.timed(append_fn)
        assert int(got.value) == nt
        assert torch.equal(out_s[:nt], out_a[:nt]) and torch.equal(mo_s, mo_a), "segments != append"
        self.timed(cat_fn)
        assert torch.equal(out_c[:nt], out_a[:nt]), "cat route != append"
        t = {"segments": [], "append": [], "cat": [], "memcpy": []}
        for r in range(warmup + reps):  # interleaved
            row = {"segments": self.timed(segments_fn), "append": self.timed(append_fn), "cat": self.timed(cat_fn),
                   "memcpy": self.timed(memcpy_fn)}
            if r >= warmup:
                for k, v in row.items():
                    t[k].append(v)
        st = {k: stats(v) for k, v in t.items()}
        res = {"entries": n, "segments": len(seg), "payload_bytes": nbytes, "new_tail": nt}
        for k, v in st.items():
            res[k + "_event_ms"] = v
            res[k + "_GBps_rw"] = round(2 * nbytes / (v["median"] * 1e6), 1)
        res["segments_over_append"] = round(st["segments"]["median"] / st["append"]["median"], 3)
        res["segments_over_cat"] = round(st["segments"]["median"] / st["cat"]["median"], 3)
        res["segments_over_memcpy"] = round(st["segments"]["median"] / st["memcpy"]["median"], 3)
        return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--cases", default="abcdef")
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--shift", type=int, default=0)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    ctx = S.Context(0)
    B = Bench(ctx)
    res = {"chunk": S.GATHER_CHUNK, "lib": S.build_info(), "shift": a.shift,
           "memcpy": "hipMemcpyAsync device-to-device (torch copy_ of a contiguous range)"}
    for case in a.cases:
        res[case] = B.case(case, a.shift, a.reps, a.warmup)
        torch.cuda.empty_cache()
    for k in "de":
        if k in res and "c" in res:
            res[k + "_over_c"] = round(res[k]["segments_event_ms"]["median"] / res["c"]["segments_event_ms"]["median"], 3)
    line = json.dumps(res)
    print(line)
    if a.out:
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
