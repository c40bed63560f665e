"""What a keyed read into fixed-size rows costs: on a
store of N entries x 4 KiB payload resident in HBM (section 18's store) plus 64
entries of 1 MiB, batches of n = 1, 64, 4096 and N keys read into rows of 4096
bytes, and the 64 long entries into rows of 1 MiB (many units per row),

  rows             srd_read_rows_device: one call, no host wait
  rows_replay      the same call captured into a graph once: one replay, timed on
                   the host from the launch to completion
  parent_a / _b    the yardstick, twice: srd_batch_read_hashed_device +
                   srd_payload_gather_device (one call with the output buffer
                   already there) from --parent-lib (a build of the parent commit;
                   default: this build), each on a context of its own

all cases and forms interleaved in one process.  Per form: the host wall time
from the call to its return (`return_ms`), the device time between events on
the call's stream (`event_ms`), the host wall time to completion
(`complete_ms`); warm-ups first, then median [min, max].  The bound of section
15 for the device time of `rows` at n = N: the larger parent median plus the
distance between the two parent medians.  Every form's bytes and statuses are
compared.  One JSON line.

usage: python tools/rows_bench.py [--entries N] [--reps R] [--parent-lib FILE] [--out FILE]"""
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

LONG_N, LONG_LEN = 64, 1 << 20


def stats(x):
    return {"median": round(statistics.median(x), 4), "min": round(min(x), 4), "max": round(max(x), 4), "n": len(x)}


def p(t):
    return C.c_void_p(t.data_ptr()) if t is not None else None


def timed(stream, fn):
    """(event_ms, return_ms, complete_ms) of fn, which enqueues on stream."""
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    e0.record(stream)
    fn()
    t1 = time.perf_counter()
    e1.record(stream)
    e1.synchronize()
    t2 = time.perf_counter()
    return e0.elapsed_time(e1), (t1 - t0) * 1e3, (t2 - t0) * 1e3


def bind_parent(path):
    P = C.CDLL(path)
    vp, u64, u32 = C.c_void_p, C.c_uint64, C.c_uint32
    P.srd_ctx_create.argtypes = [C.c_int, C.POINTER(vp)]
    P.srd_ctx_stream.argtypes, P.srd_ctx_stream.restype = [vp], vp
    P.srd_build_info.restype = C.c_char_p
    P.srd_last_error.restype = C.c_char_p
    P.srd_batch_read_hashed_device.argtypes = [vp, vp, u64, vp, u64, vp, vp, u64, vp, vp, vp]
    P.srd_payload_gather_device.argtypes = [vp, vp, u64, vp, vp, u64, u32, vp, u64, vp, vp, vp, C.POINTER(u64), vp]
    return P


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--entries", type=int, default=1 << 20)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--parent-lib", default=None)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    N = a.entries
    ctx = S.Context(0)
    L = S.lib()
    P = bind_parent(a.parent_lib or S.LIB_PATH)

    # the store: N x 4 KiB, then 64 x 1 MiB, under distinct random key hashes
    g = torch.Generator(device="cuda").manual_seed(19)
    d_h = torch.randint(1, 1 << 62, (N + LONG_N,), dtype=torch.int64, device="cuda", generator=g)
    assert torch.unique(d_h).numel() == N + LONG_N
    st = S.DeviceStore.create(N * (4096 + 64) + LONG_N * (LONG_LEN + 64) + 8192, ctx)
    for h, cnt, ln in ((d_h[:N], N, 4096), (d_h[N:], LONG_N, LONG_LEN)):
        blob = torch.randint(1, 255, (cnt * ln,), dtype=torch.uint8, device="cuda", generator=g)
        i = torch.arange(cnt, dtype=torch.int64, device="cuda")
        st.batch_write_device_with_key_hashes(h.contiguous(), blob, i * ln, torch.full_like(i, ln))
        del blob
    torch.cuda.empty_cache()
    idx, flen = st.index, st._rows_file_len()
    st.sync()

    perm = torch.from_numpy(np.random.default_rng(19).permutation(N)).cuda()
    shapes = [(n, 4096) for n in (1, 64, 4096, N) if n <= N] + [(LONG_N, LONG_LEN)]
    nmax = max(n for n, _ in shapes)
    out_bytes = max(n * cap for n, cap in shapes)
    out_new = torch.empty(out_bytes, dtype=torch.uint8, device="cuda")
    out_par = torch.empty(out_bytes, dtype=torch.uint8, device="cuda")
    o_len, o_st, o_en = (torch.empty(nmax + 1, dtype=torch.int64, device="cuda") for _ in range(3))
    o_off = torch.empty(nmax + 1, dtype=torch.int64, device="cuda")
    o_s, o_sp = (torch.empty(nmax, dtype=torch.uint8, device="cuda") for _ in range(2))
    o_crc, o_crcp = (torch.empty(nmax, dtype=torch.int32, device="cuda") for _ in range(2))
    ctx.reserve_rows(nmax, 4096)
    ctx.reserve_rows(LONG_N, LONG_LEN)
    tab = (p(idx.table), idx.nbytes, p(st.buf), flen)
    new_stream = torch.cuda.ExternalStream(ctx.stream)

    parents = []
    for _ in range(2):
        h = C.c_void_p()
        assert P.srd_ctx_create(0, C.byref(h)) == 0
        parents.append((h, P.srd_ctx_stream(h)))

    res = {"entries": N, "long_entries": LONG_N, "long_len": LONG_LEN, "file_len_bound": flen, "tail": st.tail,
           "lib": S.build_info(), "parent_lib": P.srd_build_info().decode(), "table_slots": idx.capacity,
           "reps": a.reps, "warmup": a.warmup, "cases": {}}
    cases = []
    for n, cap in shapes:
        q = (d_h[:N][perm[:n]] if cap == 4096 else d_h[N:]).contiguous()

        def rows(stream=ctx.stream, q=q, n=n, cap=cap):
            S._check(L.srd_read_rows_device(ctx.h, *tab, p(q), None, n, p(out_new), cap, cap, p(o_len), p(o_s), p(o_crc),
                                            None, 0, C.c_void_p(stream)))

        def parent(k, q=q, n=n):
            h, s = parents[k]
            tot = C.c_uint64()
            assert P.srd_batch_read_hashed_device(h, *tab, p(q), None, n, p(o_st), p(o_en), C.c_void_p(s)) == 0
            assert P.srd_payload_gather_device(h, p(st.buf), flen, p(o_st), p(o_en), n, 0, p(out_par), out_bytes, p(o_off),
                                               p(o_sp), p(o_crcp), C.byref(tot), C.c_void_p(s)) == 0, P.srd_last_error()

        graph = torch.cuda.CUDAGraph()
        torch.cuda.synchronize()
        with torch.cuda.graph(graph):
            rows(torch.cuda.current_stream().cuda_stream)

        def replay(graph=graph):
            graph.replay()

        name = f"n={n},row_cap={cap}"
        cases.append((name, n, cap, {"rows": (new_stream, rows), "rows_replay": (torch.cuda.current_stream(), replay),
                                     "parent_a": (torch.cuda.ExternalStream(parents[0][1]), lambda f=parent: f(0)),
                                     "parent_b": (torch.cuda.ExternalStream(parents[1][1]), lambda f=parent: f(1))}))
    t = {(name, k): [] for name, _, _, forms in cases for k in forms}
    for rep in range(a.warmup + a.reps):  # interleaved: every case and form in every round
        for name, _, _, forms in cases:
            for k, (s, fn) in forms.items():
                x = timed(s, fn)
                if rep >= a.warmup:
                    t[(name, k)].append(x)
    for name, n, cap, forms in cases:
        # the forms agree: bytes (row i = packed payload i: both lengths are multiples of 64), statuses, CRCs
        for k in ("rows", "rows_replay"):
            out_new.zero_()
            o_s.zero_()
            torch.cuda.synchronize()
            forms[k][1]()
            forms["parent_a"][1]()
            torch.cuda.synchronize()
            assert bool((o_s[:n] == S.GATHER_OK).all()) and torch.equal(o_s[:n], o_sp[:n]), (name, k)
            assert torch.equal(out_new[: n * cap], out_par[: n * cap]) and torch.equal(o_crc[:n], o_crcp[:n]), (name, k)
            assert bool((o_len[:n] == cap).all()), (name, k)
        r = {k: {"event_ms": stats([x[0] for x in t[(name, k)]]), "return_ms": stats([x[1] for x in t[(name, k)]]),
                 "complete_ms": stats([x[2] for x in t[(name, k)]])} for k in forms}
        pa, pb = r["parent_a"]["event_ms"]["median"], r["parent_b"]["event_ms"]["median"]
        r["bound_event_ms"] = round(max(pa, pb) + abs(pa - pb), 4)
        r["rows_inside_bound"] = r["rows"]["event_ms"]["median"] <= r["bound_event_ms"]
        r["payload_bytes"] = n * cap
        res["cases"][name] = r
    line = json.dumps(res)
    print(line)
    if a.out:
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
