"""Two or more builds of the library A/B'd on the verified gather's case c (all
2^20 payloads of a C2 store) in ONE process on the same
device-resident store (timing tool; tools/lib_ab.py's scheme for
srd_payload_gather_device): NCTX contexts per build, the builds' calls
interleaved round by round, each call timed with device events on its
context's stream.  Every call's statuses are checked.
usage: python tools/gather_ab.py A.so B.so [C.so ...]     env: NCTX (3), ROUNDS (8), OUT (a JSON file)"""
import ctypes as C
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "rust-simd-r-drive_amd"))
import torch  # noqa: E402
import srd_amd as S  # noqa: E402


def bind(path):
    L = C.CDLL(path)
    vp, u64, u32 = C.c_void_p, C.c_uint64, C.c_uint32
    L.srd_ctx_create.argtypes = [C.c_int, C.POINTER(vp)]
    L.srd_ctx_stream.argtypes = [vp]
    L.srd_ctx_stream.restype = vp
    L.srd_last_error.restype = C.c_char_p
    L.srd_payload_gather_device.argtypes = [vp, vp, u64, vp, vp, u64, u32, vp, u64, vp, vp, vp, C.POINTER(u64), vp]
    return L


libs = [bind(p) for p in sys.argv[1:]]
names = [os.path.basename(os.path.dirname(p)) + "/" + os.path.basename(p) for p in sys.argv[1:]]
nctx, rounds = int(os.environ.get("NCTX", 3)), int(os.environ.get("ROUNDS", 8))
n = 1 << 20
flen = S.synth_store_len(n)
dev = torch.zeros(S.padded_size(flen), dtype=torch.uint8, device="cuda")
torch.cuda.synchronize()
S.synth_store_device(dev.data_ptr(), n)
# the writer's layout: each 4 KiB payload at the next 64-byte boundary, 20 bytes of metadata behind it
st = torch.arange(n, dtype=torch.int64, device="cuda") * ((4096 + 20 + 63) & ~63)
en = st + 4096
out = torch.empty(n * 4096, dtype=torch.uint8, device="cuda")
offs = torch.empty(n + 1, dtype=torch.int64, device="cuda")
status = torch.empty(n, dtype=torch.uint8, device="cuda")
crc = torch.empty(n, dtype=torch.int32, device="cuda")
torch.cuda.synchronize()
ctxs = []
for _ in range(nctx):  # contexts created round-robin over the builds
    for b, L in enumerate(libs):
        h = C.c_void_p()
        assert L.srd_ctx_create(0, C.byref(h)) == 0
        ctxs.append((b, L, h, torch.cuda.ExternalStream(L.srd_ctx_stream(h))))
ms = {i: [] for i in range(len(ctxs))}
tot = C.c_uint64()
for rnd in range(rounds + 1):
    for i, (b, L, h, s) in enumerate(ctxs):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        status.zero_()
        torch.cuda.synchronize()
        e0.record(s)
        rc = L.srd_payload_gather_device(h, dev.data_ptr(), flen, st.data_ptr(), en.data_ptr(), n, 0, out.data_ptr(),
                                         out.numel(), offs.data_ptr(), status.data_ptr(), crc.data_ptr(), C.byref(tot),
                                         s.cuda_stream)
        e1.record(s)
        e1.synchronize()
        assert rc == 0, L.srd_last_error()
        assert int(tot.value) == n * 4096 and bool((status == S.GATHER_OK).all()), names[b]
        if rnd:  # (round 0 warms every context)
            ms[i].append(e0.elapsed_time(e1))
res = {"case": "gather c: 2^20 x 4 KiB", "builds": names, "nctx": nctx, "rounds": rounds, "per_ctx": []}
for i, (b, L, h, s) in enumerate(ctxs):
    res["per_ctx"].append({"build": names[b], "median_ms": round(statistics.median(ms[i]), 4),
                           "min_ms": round(min(ms[i]), 4), "max_ms": round(max(ms[i]), 4)})
for b in range(len(libs)):
    allms = [x for i, c in enumerate(ctxs) if c[0] == b for x in ms[i]]
    res[names[b]] = {"median_ms": round(statistics.median(allms), 4), "min_ms": round(min(allms), 4),
                     "max_ms": round(max(allms), 4), "n": len(allms)}
line = json.dumps(res)
print(line)
if os.environ.get("OUT"):
    with open(os.environ["OUT"], "w") as f:
        f.write(line + "\n")
