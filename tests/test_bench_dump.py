"""bench.py --dump-outputs: the sample is fixed and what dump_result writes is
the result the library returned (against the CPU oracle), exactly, with the
index in key order."""
import os
import sys

import numpy as np
import pytest

import oracle as O
import srd_amd as S

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)


def _u64(a):
    """(k, 2) float64 halves -> uint64"""
    assert a.dtype == np.float64 and a.ndim == 2 and a.shape[1] == 2
    return (a[:, 0].astype(np.uint64) << np.uint64(32)) | a[:, 1].astype(np.uint64)


def test_dump_sample_is_fixed():
    import bench
    assert list(bench.dump_sample(0)) == []
    assert list(bench.dump_sample(7)) == list(range(7))
    assert list(bench.dump_sample(bench.DUMP_SAMPLE)) == list(range(bench.DUMP_SAMPLE))
    for n in (bench.DUMP_SAMPLE + 1, 1 << 20):
        a, b = bench.dump_sample(n), bench.dump_sample(n)
        assert a.size == bench.DUMP_SAMPLE and np.array_equal(a, b)
        assert np.all(np.diff(a) > 0) and a[0] >= 0 and a[-1] < n
    # 10 result arrays per shard, u64 ones as two float64 columns: 8 shards stay under 64 MB
    assert 8 * 10 * bench.DUMP_SAMPLE * 16 <= 64 * 1000 * 1000


@pytest.mark.gpu
def test_dump_result_matches_oracle(tmp_path, monkeypatch):
    import torch

    import bench
    monkeypatch.setattr(bench, "DUMP_SAMPLE", 1000)  # 3001 entries: the sampled path
    n = 3001
    first = O.synth_store(n - 1, 1024)
    # a second write of the first key: the index (3000 keys) is shorter than the chain
    buf = bytearray(first.tobytes())
    O.write_entries(buf, first.size, [(O.chain(first, first.size, False)[0]["key_hash"], b"again")])
    host = np.frombuffer(bytes(buf), np.uint8)
    ctx = S.Context(0)
    try:
        store = torch.zeros(S.padded_size(host.size), dtype=torch.uint8, device="cuda:0")
        store[: host.size].copy_(torch.from_numpy(host.copy()))
        torch.cuda.synchronize()
        r = S.validate_index_device(store.data_ptr(), host.size, 0, ctx)
        bench.dump_result(str(tmp_path), r, 0)
    finally:
        ctx.close()
    want_len = O.recover_valid_chain(host)
    ch = O.chain(host, want_len)
    assert r.final_len == want_len == host.size and r.n_chain == len(ch) == n
    keep = bench.dump_sample(n)
    assert keep.size == 1000
    sums = np.load(tmp_path / "sums.npy")
    assert sums.dtype == np.float64 and sums.shape == (len(bench.RESULT_ARRAYS),)
    for i, (name, dt, cnt) in enumerate(bench.RESULT_ARRAYS[:8]):
        exp = np.array([e[name] for e in ch], np.uint64)
        got = np.load(tmp_path / f"{name}.npy")
        got = _u64(got) if dt is np.uint64 else got.astype(np.uint64)
        assert np.array_equal(got, exp[keep]), name
        assert int(sums[i]) == int(exp.sum(dtype=np.uint64)) & 0xFFFFFFFF, name
    index = O.key_indexer_build(host, want_len)
    assert r.n_index == len(index) == n - 1
    # key order as the dump sorts it: the hashes' bit patterns as signed 64-bit
    keys = np.sort(np.fromiter(index.keys(), np.uint64, len(index)).view(np.int64)).view(np.uint64)
    ikeep = bench.dump_sample(len(index))
    assert np.array_equal(_u64(np.load(tmp_path / "index_key_hash.npy")), keys[ikeep])
    assert np.array_equal(_u64(np.load(tmp_path / "index_packed.npy")),
                          np.array([index[int(k)] for k in keys[ikeep]], np.uint64))
