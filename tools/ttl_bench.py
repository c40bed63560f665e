"""What a TTL read's decision and the sweep cost: on a
TTL store of N entries x 4 KiB payload (8 expiry bytes + value) resident in
HBM, a third of it expired, with N queries (every key once, shuffled),

  resolve        srd_ttl_resolve_device on the namespaced hashes
  resolve_nc     the same without d_counts (what the per-status counts cost)
  resolve_keys   srd_ttl_resolve_keys_device from the raw keys: one launch
  two_launch     srd_namespace_hash_batch_device, then the resolve
  three_launch   srd_xxh3_64_batch_device over the raw keys (what a keyed read
                 runs first today), srd_namespace_hash_batch_device, then the
                 resolve
  read_hashed    srd_batch_read_hashed_device on the same hashes: the yardstick
                 (the same probe and metadata line, without the payload head);
                 with --parent-lib also from that library (a build of the
                 parent commit), on a context of its own
  sweep_plan     srd_ttl_sweep_device(SRD_TTL_SWEEP_PLAN): export, sort, judge

interleaved in one process.  Library calls are timed with device events on
their context's stream and with the host clock ending in a synchronise;
warm-ups first, then median [min, max].  One JSON line.

usage: python tools/ttl_bench.py [--entries N] [--reps R] [--parent-lib FILE] [--out FILE]"""
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

NOW = 1_700_000_000


def stats(x):
    return {"median": round(statistics.median(x), 4), "min": round(min(x), 4), "max": round(max(x), 4), "n": len(x)}


def timed(stream, fn):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    e0.record(stream)
    fn()
    e1.record(stream)
    e1.synchronize()
    return e0.elapsed_time(e1), (time.perf_counter() - t0) * 1e3


def p(t):
    return C.c_void_p(t.data_ptr())


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--entries", type=int, default=1 << 20)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--parent-lib", default=None)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    n = a.entries
    ctx = S.Context(0)
    L = S.lib()
    stream = torch.cuda.ExternalStream(ctx.stream)
    ph = S.NamespaceHasher(S.TTL_PREFIX, ctx).prefix_hash

    # the keys, their namespaced hashes (on the device) and the store
    keys = [b"ttl-key-%d" % i for i in range(n)]
    kb, ko, kl = S._blob(keys)
    d_kb = torch.from_numpy(kb.copy()).cuda()
    d_ko, d_kl = (torch.from_numpy(x.view(np.int64).copy()).cuda() for x in (ko, kl))
    d_h = torch.empty(n, dtype=torch.int64, device="cuda")
    S._check(L.srd_namespace_hash_batch_device(ctx.h, ph, p(d_kb), p(d_ko), p(d_kl), n, None, p(d_h), None))
    S._sync_ctx(ctx, 0)
    blob = torch.randint(1, 255, (n * 4096,), dtype=torch.uint8, device="cuda")
    i = torch.arange(n, dtype=torch.int64, device="cuda")
    exp = torch.where(i % 3 == 0, NOW - 1 - i % 5, NOW + 1 + i)
    blob.view(torch.int64).view(n, 512)[:, 0] = exp
    st = S.DeviceStore.create(n * (4096 + 64) + 4096, ctx)
    st.batch_write_device_with_key_hashes(d_h, blob, i * 4096, torch.full_like(i, 4096))
    del blob
    torch.cuda.empty_cache()
    idx, flen = st.index, st.tail
    n_exp = int((exp <= NOW).sum().item())

    # the queries: every key once, shuffled
    perm = torch.from_numpy(np.random.default_rng(18).permutation(n)).cuda()
    q, qo, ql = d_h[perm].contiguous(), d_ko[perm].contiguous(), d_kl[perm].contiguous()
    o_st, o_en, o_ex, o_h, o_kh = (torch.empty(n, dtype=torch.int64, device="cuda") for _ in range(5))
    o_s = torch.empty(n, dtype=torch.uint8, device="cuda")
    o_c = torch.empty(4, dtype=torch.int64, device="cuda")
    tab = (p(idx.table), idx.nbytes, p(st.buf), flen)
    sv = C.c_void_p(ctx.stream)

    def resolve(hashes=q, counts=o_c):
        S._check(L.srd_ttl_resolve_device(ctx.h, *tab, p(hashes), n, NOW, p(o_st), p(o_en), p(o_ex), p(o_s),
                                          p(counts) if counts is not None else None, sv))

    def resolve_keys():
        S._check(L.srd_ttl_resolve_keys_device(ctx.h, *tab, ph, p(d_kb), p(qo), p(ql), n, NOW, p(o_h), p(o_st), p(o_en),
                                               p(o_ex), p(o_s), p(o_c), sv))

    def ns_hash():
        S._check(L.srd_namespace_hash_batch_device(ctx.h, ph, p(d_kb), p(qo), p(ql), n, None, p(o_h), sv))

    def two_launch():
        ns_hash()
        resolve(o_h)

    def three_launch():
        S._check(L.srd_xxh3_64_batch_device(ctx.h, p(d_kb), p(qo), p(ql), n, p(o_kh), sv))
        two_launch()

    def read_hashed():
        S._check(L.srd_batch_read_hashed_device(ctx.h, *tab, p(q), None, n, p(o_st), p(o_en), sv))

    def sweep_plan():
        used, nt, ss = C.c_uint64(idx.used), C.c_uint64(), S.TtlSweepStats()
        S._check(L.srd_ttl_sweep_device(ctx.h, p(idx.table), idx.nbytes, C.byref(used), p(st.buf), flen, st.buf.numel(),
                                        NOW, S.TTL_SWEEP_PLAN, C.byref(nt), C.byref(ss)))
        assert (ss.n_judged, ss.n_expired, ss.n_short) == (n, n_exp, 0), ss

    cases = {"resolve": (stream, resolve), "resolve_nc": (stream, lambda: resolve(q, None)),
             "resolve_keys": (stream, resolve_keys), "two_launch": (stream, two_launch),
             "three_launch": (stream, three_launch), "read_hashed": (stream, read_hashed),
             "sweep_plan": (stream, sweep_plan)}
    res = {"entries": n, "queries": n, "file_len": flen, "expired": n_exp, "lib": S.build_info(),
           "table_slots": idx.capacity}
    if a.parent_lib:
        P = C.CDLL(a.parent_lib)
        vp, u64 = C.c_void_p, C.c_uint64
        P.srd_ctx_create.argtypes = [C.c_int, C.POINTER(vp)]
        P.srd_ctx_stream.argtypes, P.srd_ctx_stream.restype = [vp], vp
        P.srd_build_info.restype = C.c_char_p
        P.srd_batch_read_hashed_device.argtypes = [vp, vp, u64, vp, u64, vp, vp, u64, vp, vp, vp]
        ph_ctx = vp()
        assert P.srd_ctx_create(0, C.byref(ph_ctx)) == 0
        pstream = P.srd_ctx_stream(ph_ctx)
        p_st, p_en = torch.empty_like(o_st), torch.empty_like(o_en)

        def read_hashed_parent():
            assert P.srd_batch_read_hashed_device(ph_ctx, *tab, p(q), None, n, p(p_st), p(p_en), vp(pstream)) == 0
        cases["read_hashed_parent"] = (torch.cuda.ExternalStream(pstream), read_hashed_parent)
        res["parent_lib"] = P.srd_build_info().decode()

    t = {k: [] for k in cases}
    for rep in range(a.warmup + a.reps):  # interleaved
        for k, (s, fn) in cases.items():
            x = timed(s, fn)
            if rep >= a.warmup:
                t[k].append(x)
    # the forms agree, and the counts are what the store holds
    resolve()
    S._sync_ctx(ctx, 0)
    want = (o_st.clone(), o_en.clone(), o_ex.clone(), o_s.clone(), o_c.clone())
    resolve_keys()
    S._sync_ctx(ctx, 0)
    assert all(torch.equal(x, y) for x, y in zip(want, (o_st, o_en, o_ex, o_s, o_c))) and torch.equal(o_h, q)
    assert o_c.tolist() == [0, n - n_exp, n_exp, 0], o_c.tolist()
    for k in cases:
        res[k] = {"event_ms": stats([x[0] for x in t[k]]), "host_ms": stats([x[1] for x in t[k]])}
    y = "read_hashed_parent" if a.parent_lib else "read_hashed"
    res["yardstick"] = y
    res["resolve_over_yardstick"] = round(res["resolve"]["event_ms"]["median"] / res[y]["event_ms"]["median"], 3)
    res["fused_over_three_launch"] = round(res["resolve_keys"]["event_ms"]["median"] /
                                           res["three_launch"]["event_ms"]["median"], 3)
    res["fused_over_two_launch"] = round(res["resolve_keys"]["event_ms"]["median"] /
                                         res["two_launch"]["event_ms"]["median"], 3)
    line = json.dumps(res)
    print(line)
    if a.out:
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
