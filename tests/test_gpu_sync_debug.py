"""SRD_SYNC_DEBUG=1 (a wait and a named check behind every kernel launch, on
the stream the kernel went to) changes no result: one small DeviceStore session
-- writes with a duplicate key and a key written and deleted in one batch,
reads, verified gathers, a batched delete with a duplicate in its list, the
iterator gather, compaction, and a gather ordered on a torch side stream --
runs in this process without the knob and in a fresh child process with it
(the knob is read once per process), and everything either returns is compared.
The session without the knob is also held against a dict model of the store.
Run as a script, this file is the child: it prints the session as JSON."""
import hashlib
import json
import os
import random
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LENS = [1, 63, 64, 65, 4096, 70_000]  # 70 000 > one 64 KiB gather unit: the combine kernel runs
KEYS = [b"key-%02d" % i for i in range(48)]


def _sha(b):
    return None if b is None else hashlib.sha256(bytes(b)).hexdigest()


def _payloads():
    rng = random.Random(0x51DEB)
    first = {k: rng.randbytes(LENS[i % len(LENS)]) for i, k in enumerate(KEYS)}
    return first, rng.randbytes(777), rng.randbytes(65), rng.randbytes(300)


def session():
    import numpy as np
    import torch
    import srd_amd as S
    ctx = S.Context(0)
    first, again3, again41, tmp = _payloads()
    out = {}
    store = S.DeviceStore.create(2 << 20, ctx)
    out["tail1"] = store.batch_write(KEYS[:40], [first[k] for k in KEYS[:40]])
    # one batch: new keys, key-41 twice, key-03 overwritten, and a key written and then deleted
    k2 = KEYS[40:] + [KEYS[41], KEYS[3], b"tmp", b"tmp"]
    p2 = [first[k] for k in KEYS[40:]] + [again41, again3, tmp, b"\x00"]
    out["tail2"] = store.batch_write_with_key_hashes(S.compute_hash_batch(k2, ctx), p2, allow_null=True)
    out["len2"] = len(store)
    ask = KEYS + [b"absent", b"tmp"]
    out["read"] = [_sha(p) for p in store.batch_read(ask)]
    g = store.batch_gather(ask)
    out["gather"] = {"payloads": [_sha(p) for p in g.payloads()], "status": [int(s) for s in g.status],
                     "crc": [int(c) for c in g.crc_computed], "offs": [int(o) for o in g.offs]}
    out["verify"] = store.verify(ask)
    out["packed"] = [int(x) for x in store.index.get_packed(S.compute_hash_batch(ask, ctx))]
    out["tail3"] = store.batch_delete([KEYS[5], KEYS[6], KEYS[5], b"absent"])
    out["len3"] = len(store)
    out["read3"] = [_sha(p) for p in store.batch_read(ask)]
    it = store.iter_gather()
    out["iter"] = {"payloads": [_sha(p) for p in it.payloads()], "status": [int(s) for s in it.status],
                   "crc": [int(c) for c in it.crc_computed]}
    # a gather ordered on a torch side stream: the ranges, the outputs and both calls on it
    h = S.compute_hash_batch(ask, ctx)
    st, en = store._ranges(h, h)
    side = torch.cuda.Stream()
    with torch.cuda.stream(side):
        d_st = torch.from_numpy(st.view(np.int64).copy()).cuda()
        d_en = torch.from_numpy(en.view(np.int64).copy()).cuda()
        n = len(ask)
        offs = torch.empty(n + 1, dtype=torch.int64, device="cuda")
        status = torch.empty(n, dtype=torch.uint8, device="cuda")
        crc = torch.empty(n, dtype=torch.int32, device="cuda")
        args = (store.buf.data_ptr(), store.tail, d_st.data_ptr(), d_en.data_ptr(), n)
        total = S.payload_gather_device(*args, 0, None, 0, offs.data_ptr(), status.data_ptr(), None, ctx,
                                        stream=side.cuda_stream)
        data = torch.empty(total, dtype=torch.uint8, device="cuda")
        S.payload_gather_device(*args, 0, data.data_ptr(), total, offs.data_ptr(), status.data_ptr(), crc.data_ptr(),
                                ctx, stream=side.cuda_stream)
    side.synchronize()
    out["side"] = {"total": total, "data": _sha(data.cpu().numpy().tobytes()), "offs": [int(o) for o in offs.cpu()],
                   "status": [int(s) for s in status.cpu()], "crc": [int(c) & 0xFFFFFFFF for c in crc.cpu()]}
    _k, p = store.index.export()
    comp = S.compact_device(store.buf.data_ptr(), store.tail, p.data_ptr(), p.numel(), ctx)
    out["compact"] = {"len": int(comp.numel()), "sha": _sha(comp.cpu().numpy().tobytes())}
    out["crc32"] = [int(c) for c in S.crc32_batch(first[KEYS[4]], [0, 5], [4096, 100], ctx)]
    out["bytes"] = _sha(store.bytes())
    ctx.close()
    return out


@pytest.mark.gpu
def test_sync_debug_changes_no_result():
    import srd_amd as S
    plain = session()
    # the session against a model of the store
    first, again3, again41, _tmp = _payloads()
    model = dict(first)
    model[KEYS[3]], model[KEYS[41]] = again3, again41
    want = [_sha(model[k]) for k in KEYS] + [None, None]
    assert plain["read"] == want and plain["gather"]["payloads"] == want
    assert plain["verify"] == [True] * len(KEYS) + [None, None]
    assert plain["len2"] == len(KEYS)
    del model[KEYS[5]], model[KEYS[6]]
    # (batch_delete_key_hashes keeps a listed hash once per listing: key-05 gets two tombstones)
    assert plain["tail3"] == plain["tail2"] + 3 * 21 and plain["len3"] == len(KEYS) - 2
    assert plain["read3"] == [_sha(model.get(k)) for k in KEYS] + [None, None]
    assert sorted(plain["iter"]["payloads"]) == sorted(_sha(p) for p in model.values())
    assert set(plain["iter"]["status"]) == {S.GATHER_OK}
    assert plain["side"]["status"] == [S.GATHER_OK if k in model else S.GATHER_NONE for k in KEYS] + [S.GATHER_NONE] * 2
    assert plain["side"]["crc"][:5] == plain["gather"]["crc"][:5]
    assert plain["compact"]["len"] > 0
    # ... and the same session with a wait and a check behind every launch
    env = dict(os.environ, SRD_SYNC_DEBUG="1")
    p = subprocess.run([sys.executable, os.path.abspath(__file__)], capture_output=True, text=True, env=env, timeout=300)
    assert p.returncode == 0, p.stderr[-4000:]
    debug = json.loads(p.stdout.strip().splitlines()[-1])
    assert debug.pop("sync_debug") == "1"
    for k in plain:
        assert debug[k] == plain[k], k
    assert debug.keys() == plain.keys()


if __name__ == "__main__":
    for d in (ROOT, os.path.join(ROOT, "oracle"), os.path.join(ROOT, "rust-simd-r-drive_amd")):
        sys.path.insert(0, d)
    res = session()
    res["sync_debug"] = os.environ.get("SRD_SYNC_DEBUG", "")
    print(json.dumps(res))
