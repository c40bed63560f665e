"""What the verified gather costs: on a C2 store (2^20
keys x 4 KiB) resident in HBM,

  a / b  a gather of 1024 / 65,536 random distinct keys -- the gather call
         alone (ranges given) and with the look-up (srd_batch_read_hashed_device)
         -- and alongside, interleaved in the same process, the path it replaces:
         torch.cat over the same slices (host clock: its cost is host-side
         slicing) plus srd_crc32_batch_device over the same ranges for the check
         the old path lacks;
  c      all 2^20 payloads (4.3 GB out): GB/s read + written against
         the runtime's device-to-device copy of the same byte count, and the verify-only call
         (the CRC without the copy);
  d      8 payloads of 256 MiB each: the same, few and large hits.

Library calls are timed with device events on the context stream (a gather's
one host wait is inside its window) and with the host clock ending in a
synchronise; warm-ups first, then median [min, max].  One JSON line.

usage: python tools/gather_bench.py [--cases abcd] [--reps R] [--chunk LABEL] [--out FILE]
(SRD_LIB_PATH=build/var/lib_X.so loads a `make variant` build, e.g. another
SRD_GATHER_CHUNK; --chunk records its value in the line)"""
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


def gbps(nbytes, st):
    return {k: round(2 * nbytes / (st[j] * 1e6), 1) for k, j in (("median", "median"), ("best", "min"), ("worst", "max"))}


class Bench:
    def __init__(self, ctx):
        self.ctx, self.L = ctx, S.lib()
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

    def gather_fn(self, d_file, flen, st, en, flags, out, offs, status, crc):
        n = st.numel()
        tot = C.c_uint64()

        def fn():
            S._check(self.L.srd_payload_gather_device(
                self.ctx.h, C.c_void_p(d_file), flen, C.c_void_p(st.data_ptr()), C.c_void_p(en.data_ptr()), n, flags,
                C.c_void_p(out.data_ptr()), out.numel(), C.c_void_p(offs.data_ptr()), C.c_void_p(status.data_ptr()),
                C.c_void_p(crc.data_ptr()), C.byref(tot), C.c_void_p(self.ctx.stream)))
        return fn

    def memcpy_fn(self, dst, src, nbytes):
        # torch's copy of a contiguous uint8 range on one device is the runtime's
        # own device-to-device hipMemcpyAsync, here on the context stream (one HIP
        # runtime per process: the library binds to the one torch loaded)
        def fn():
            with torch.cuda.stream(self.stream):
                dst[:nbytes].copy_(src[:nbytes])
        return fn

    def run(self, fn, reps, warmup):
        return [self.timed(fn) for _ in range(warmup + reps)][warmup:]

    def bulk(self, d_file_t, flen, st, en, reps, warmup):
        """cases c / d: the whole gather, the verify-only call and the runtime's copy of the same bytes."""
        n = st.numel()
        nbytes = int((en - st).sum().item())
        padded = int((((en - st) + 63) & ~63).sum().item())
        out = torch.empty(padded, dtype=torch.uint8, device="cuda")
        offs = torch.empty(n + 1, dtype=torch.int64, device="cuda")
        status = torch.empty(n, dtype=torch.uint8, device="cuda")
        crc = torch.empty(n, dtype=torch.int32, device="cuda")
        g = self.gather_fn(d_file_t.data_ptr(), flen, st, en, 0, out, offs, status, crc)
        v = self.gather_fn(d_file_t.data_ptr(), flen, st, en, S.GATHER_VERIFY_ONLY, out, offs, status, crc)
        m = self.memcpy_fn(out, d_file_t, nbytes)
        tg, tv, tm = [], [], []
        for r in range(warmup + reps):  # interleaved
            a, b, c = self.timed(g), self.timed(v), self.timed(m)
            if r >= warmup:
                tg.append(a), tv.append(b), tm.append(c)
        self.timed(g)
        assert bool((status == S.GATHER_OK).all()), "a synthetic payload failed its checksum"
        sg, sv, sm = (stats([t[0] for t in x]) for x in (tg, tv, tm))
        return {"hits": n, "payload_bytes": nbytes, "gather_event_ms": sg, "gather_host_ms": stats([t[1] for t in tg]),
                "gather_GBps_rw": gbps(nbytes, sg), "verify_only_event_ms": sv, "verify_only_GBps_read": {
                    k: round(x / 2, 1) for k, x in gbps(nbytes, sv).items()},
                "memcpy_dtod_event_ms": sm, "memcpy_GBps_rw": gbps(nbytes, sm),
                "gather_over_memcpy": round(sg["median"] / sm["median"], 3)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--cases", default="abcd")
    ap.add_argument("--entries", type=int, default=1 << 20)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--chunk", type=int, default=S.GATHER_CHUNK)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    ctx = S.Context(0)
    B = Bench(ctx)
    L = B.L
    res = {"chunk": a.chunk, "lib": S.build_info(), "memcpy": "hipMemcpyAsync device-to-device (torch copy_ of a contiguous range)"}
    if set(a.cases) & set("abc"):
        flen = S.synth_store_len(a.entries)
        dev = torch.zeros(S.padded_size(flen), dtype=torch.uint8, device="cuda")
        torch.cuda.synchronize()
        S.synth_store_device(dev.data_ptr(), a.entries, ctx=ctx)
        r = S.validate_index_device(dev.data_ptr(), flen, 0, ctx)
        assert r.n_index == a.entries and r.final_len == flen
        idx = S.DeviceIndex(r.index_key_hash, r.index_packed, r.n_index, ctx)
        have = S.device_view(r.index_key_hash, r.n_index).clone()
        all_st = S.device_view(r.payload_start, r.n_chain).clone()
        all_en = S.device_view(r.meta_off, r.n_chain).clone()
        torch.cuda.synchronize()
        res.update(entries=a.entries, file_len=flen)
        rng = np.random.default_rng(11)
        for case, k in (("a", 1024), ("b", 65536)):
            if case not in a.cases:
                continue
            k = min(k, a.entries)
            reps_old = a.reps if k <= 4096 else max(3, a.reps // 4)
            out = torch.empty(k * 4096, dtype=torch.uint8, device="cuda")
            offs = torch.empty(k + 1, dtype=torch.int64, device="cuda")
            status = torch.empty(k, dtype=torch.uint8, device="cuda")
            crc = torch.empty(k, dtype=torch.int32, device="cuda")
            crc_old = torch.empty(k, dtype=torch.int32, device="cuda")
            st, en = torch.empty(k, dtype=torch.int64, device="cuda"), torch.empty(k, dtype=torch.int64, device="cuda")
            t_g, t_gl, t_cat, t_crc = [], [], [], []
            for rep in range(a.warmup + a.reps):
                q = have[torch.from_numpy(rng.choice(a.entries, k, replace=False)).cuda()].contiguous()
                torch.cuda.synchronize()

                def lookup():
                    S._check(L.srd_batch_read_hashed_device(ctx.h, C.c_void_p(idx.table.data_ptr()), idx.nbytes,
                                                            C.c_void_p(dev.data_ptr()), flen, C.c_void_p(q.data_ptr()),
                                                            None, k, C.c_void_p(st.data_ptr()), C.c_void_p(en.data_ptr()),
                                                            C.c_void_p(ctx.stream)))

                gather = B.gather_fn(dev.data_ptr(), flen, st, en, 0, out, offs, status, crc)
                tl = B.timed(lambda: (lookup(), gather()))
                tg = B.timed(gather)
                assert bool((status == S.GATHER_OK).all())
                if rep >= a.warmup:
                    t_gl.append(tl), t_g.append(tg)
                if rep < a.warmup + reps_old:
                    # the path it replaces: DeviceStore._payloads' torch.cat, and the CRC batch for the check
                    hs, he = st.cpu().numpy(), en.cpu().numpy()
                    hit = [(int(x), int(y)) for x, y in zip(hs, he)]
                    ln = (en - st).contiguous()
                    torch.cuda.synchronize()
                    t0 = time.perf_counter()
                    flat = torch.cat([dev[x:y] for x, y in hit])
                    torch.cuda.synchronize()
                    tc = (time.perf_counter() - t0) * 1e3
                    tk = B.timed(lambda: S._check(L.srd_crc32_batch_device(
                        ctx.h, C.c_void_p(dev.data_ptr()), C.c_void_p(st.data_ptr()), C.c_void_p(ln.data_ptr()), k,
                        C.c_void_p(crc_old.data_ptr()), C.c_void_p(ctx.stream))))
                    assert bool((crc_old == crc).all()) and flat.numel() == k * 4096
                    if rep >= a.warmup:
                        t_cat.append(tc), t_crc.append(tk)
            old_sum = [c + e[1] for c, e in zip(t_cat, t_crc)]
            res[case] = {"keys": k, "gather_event_ms": stats([t[0] for t in t_g]),
                         "gather_host_ms": stats([t[1] for t in t_g]),
                         "lookup_gather_event_ms": stats([t[0] for t in t_gl]),
                         "lookup_gather_host_ms": stats([t[1] for t in t_gl]),
                         "old_cat_host_ms": stats(t_cat), "old_crc_event_ms": stats([t[0] for t in t_crc]),
                         "old_cat_plus_crc_host_ms": stats(old_sum)}
            del out
        if "c" in a.cases:
            res["c"] = B.bulk(dev, flen, all_st, all_en, max(5, a.reps // 2), a.warmup)
        del dev, idx, have, all_st, all_en
        torch.cuda.empty_cache()
    if "d" in a.cases:
        lens = np.full(8, 256 << 20, np.uint64)
        flen = S.synth_store_len(8, lens=lens)
        dev = torch.zeros(S.padded_size(flen), dtype=torch.uint8, device="cuda")
        torch.cuda.synchronize()
        S.synth_store_device(dev.data_ptr(), 8, lens=lens, ctx=ctx)
        st, tail = [], 0
        for ln in lens:  # the writer's layout: each payload at the next 64-byte boundary, 20 bytes of metadata after it
            st.append((tail + 63) & ~63)
            tail = st[-1] + int(ln) + 20
        assert tail == flen
        d_st = torch.tensor(st, dtype=torch.int64, device="cuda")
        d_en = d_st + (256 << 20)
        torch.cuda.synchronize()
        res["d"] = B.bulk(dev, flen, d_st, d_en, max(5, a.reps // 2), a.warmup)
    line = json.dumps(res)
    print(line)
    if a.out:
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
