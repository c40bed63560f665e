"""What reading entries into device segments costs: the
payloads of a store in HBM delivered into the caller's own tensors by
srd_payload_scatter_device, and alongside, interleaved in the same process, the
routes next to it:

  scatter  the new call: every payload straight into its pieces;
  gather   srd_payload_gather_device over the same ranges into one packed
           buffer (the floor for this machinery: nothing is where the caller
           wants it yet);
  copy     the route there was before: that gather, then torch copy_ from the
           packed buffer into the pieces, inside the window (a: one copy_ of
           the whole buffer; b: one strided copy_ per destination tensor; c, d,
           e, f: one copy_ per piece).

The cases are section 14's, read back: tools/segments_bench.py's shapes are
written to a store by srd_batch_append_segments_device, and the destinations
are fresh tensors of the sources' shapes at the sources' address residues.

  a  2^19 x 4 KiB, one segment each;
  b  2^19 x (64 B header + 4032 B body), both 16-aligned;
  c  8 x (64 B header + 256 MiB body);
  d  8 x (20 B header + 256 MiB body): the realigning path;
  e  8 x (64 B header + 256 MiB body at destination residue 1): the realigning path;
  f  1024 entries x 64 pages of 16 KiB, scattered over a pool.

Every route is timed with device events on the context stream (the calls' host
waits are inside their windows); warm-ups first, then median [min, max].  Every
case first checks that the routes delivered identical bytes: the sources'.  One
JSON line.

usage: python tools/scatter_bench.py [--cases abcdef] [--reps R] [--warmup W] [--shift K] [--out FILE]
(--shift K divides the entry counts of a, b, f and the body size of c, d, e by 2^K: a quick look)"""
import argparse
import ctypes as C
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "rust-simd-r-drive_amd"))
sys.path.insert(0, os.path.join(ROOT, "tools"))

import numpy as np  # noqa: E402
import torch  # noqa: E402

import srd_amd as S  # noqa: E402
from segments_bench import dev_i64, shapes, stats  # noqa: E402


def like(t):
    """A zeroed tensor of t's length at t's address residue mod 16."""
    r = t.data_ptr() % 16
    return torch.zeros(t.numel() + 16, dtype=torch.uint8, device="cuda")[r: r + t.numel()]


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
        srcs, seg, first, _ = shapes(name, shift)
        n = len(first) - 1
        lens = np.add.reduceat(seg["len"], first[:-1].astype(np.int64)).astype(np.uint64)
        nbytes = int(lens.sum())
        # the store: the pieces written by the segment append
        d_seg = torch.from_numpy(seg.view(np.uint8).copy()).cuda()
        d_first = dev_i64(first)
        d_h = dev_i64((np.arange(n, dtype=np.uint64) + np.uint64(1)) * np.uint64(0x9E3779B97F4A7C15))
        cap = S.padded_size(nbytes + 84 * n + 64)
        store = torch.zeros(cap, dtype=torch.uint8, device="cuda")
        mo = torch.empty(n, dtype=torch.int64, device="cuda")
        ptrs = (C.c_void_p * len(srcs))(*[t.data_ptr() for t in srcs])
        slens = (C.c_uint64 * len(srcs))(*[t.numel() for t in srcs])
        got = C.c_uint64()
        torch.cuda.synchronize()
        S._check(self.L.srd_batch_append_segments_device(
            self.ctx.h, ptrs, slens, len(srcs), C.c_void_p(d_seg.data_ptr()), len(seg), C.c_void_p(d_first.data_ptr()),
            C.c_void_p(d_h.data_ptr()), n, 0, 0, C.c_void_p(store.data_ptr()), cap, C.byref(got), C.c_void_p(mo.data_ptr()),
            C.c_void_p(self.ctx.stream)))
        flen = int(got.value)
        d_en = mo
        d_st = mo - dev_i64(lens)
        torch.cuda.synchronize()
        # the destinations of both routes, the packed buffer, the outputs
        dst_s, dst_c = [like(t) for t in srcs], [like(t) for t in srcs]
        status = torch.empty(n, dtype=torch.uint8, device="cuda")
        crc = torch.empty(n, dtype=torch.int32, device="cuda")
        offs = torch.empty(n + 1, dtype=torch.int64, device="cuda")
        tot = C.c_uint64()
        dptrs = (C.c_void_p * len(dst_s))(*[t.data_ptr() for t in dst_s])

        def gather_into(d_out, out_cap):
            S._check(self.L.srd_payload_gather_device(
                self.ctx.h, C.c_void_p(store.data_ptr()), flen, C.c_void_p(d_st.data_ptr()), C.c_void_p(d_en.data_ptr()), n,
                0, C.c_void_p(d_out), out_cap, C.c_void_p(offs.data_ptr()), C.c_void_p(status.data_ptr()),
                C.c_void_p(crc.data_ptr()), C.byref(tot), C.c_void_p(self.ctx.stream)))

        gather_into(None, 0)  # the layout call sizes the packed buffer
        torch.cuda.synchronize()
        total = int(tot.value)
        packed = torch.empty(total, dtype=torch.uint8, device="cuda")
        poff = offs.cpu().numpy().view(np.uint64)
        # the copies of the old route, as (destination view, packed view) pairs made outside the window
        if name == "a":
            assert total == nbytes
            pairs = [(dst_c[0], packed)]
        elif name == "b":
            rows = packed.view(n, 4096)
            pairs = [(dst_c[0].view(n, 64), rows[:, :64]), (dst_c[1].view(n, 4032), rows[:, 64:])]
        else:
            pairs = []
            for i in range(n):
                o = int(poff[i])
                for s, so, ln in zip(*(seg[k][int(first[i]): int(first[i + 1])] for k in ("src", "off", "len"))):
                    pairs.append((dst_c[int(s)][int(so): int(so) + int(ln)], packed[o: o + int(ln)]))
                    o += int(ln)

        def scatter_fn():
            S._check(self.L.srd_payload_scatter_device(
                self.ctx.h, C.c_void_p(store.data_ptr()), flen, C.c_void_p(d_st.data_ptr()), C.c_void_p(d_en.data_ptr()), n,
                dptrs, slens, len(dst_s), C.c_void_p(d_seg.data_ptr()), len(seg), C.c_void_p(d_first.data_ptr()), 0,
                C.c_void_p(status.data_ptr()), C.c_void_p(crc.data_ptr()), C.c_void_p(self.ctx.stream)))

        def gather_fn():
            gather_into(packed.data_ptr(), total)

        def copy_fn():
            gather_fn()
            with torch.cuda.stream(self.stream):
                for d, p in pairs:
                    d.copy_(p)

        # identical bytes from both routes -- the sources' -- before anything is timed
        self.timed(scatter_fn)
        assert bool((status == S.GATHER_OK).all()), "scatter: a status is not OK"
        crc_s = crc.clone()
        self.timed(copy_fn)
        assert bool((status == S.GATHER_OK).all()) and torch.equal(crc, crc_s)
        for a, b, c in zip(srcs, dst_s, dst_c):
            assert torch.equal(a, b), "scatter != the sources"
            assert torch.equal(a, c), "gather + copy_ != the sources"
        t = {"scatter": [], "gather": [], "copy": []}
        for r in range(warmup + reps):  # interleaved
            row = {"scatter": self.timed(scatter_fn), "gather": self.timed(gather_fn), "copy": self.timed(copy_fn)}
            if r >= warmup:
                for k, v in row.items():
                    t[k].append(v)
        st = {k: stats(v) for k, v in t.items()}
        res = {"entries": n, "segments": len(seg), "copies": len(pairs), "payload_bytes": nbytes, "file_len": flen}
        for k, v in st.items():
            res[k + "_event_ms"] = v
            res[k + "_GBps_rw"] = round(2 * nbytes / (v["median"] * 1e6), 1)
        res["scatter_over_gather"] = round(st["scatter"]["median"] / st["gather"]["median"], 3)
        res["scatter_over_copy"] = round(st["scatter"]["median"] / st["copy"]["median"], 3)
        res["scatter_inside_gather_min_max"] = st["gather"]["min"] <= st["scatter"]["median"] <= st["gather"]["max"]
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
    res = {"chunk": S.GATHER_CHUNK, "lib": S.build_info(), "shift": a.shift}
    for case in a.cases:
        res[case] = B.case(case, a.shift, a.reps, a.warmup)
        torch.cuda.empty_cache()
    for k in "de":
        if k in res and "c" in res:
            res[k + "_over_c"] = round(res[k]["scatter_event_ms"]["median"] / res["c"]["scatter_event_ms"]["median"], 3)
    line = json.dumps(res)
    print(line)
    if a.out:
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
