"""TTL entries on the device against the CPU oracle and
the contract of StorageCacheExt (extensions/src/storage_cache_ext.rs:23-107)
over NamespaceHasher (src/utils/namespace_hasher.rs:33-65): namespaced hashes at
XXH3's path boundaries, the two TTL writes byte for byte, the resolve in its
hashed and fused forms with every output array compared whole, packed and
scattered reads, eviction's tombstones and refusal, and the sweep.  `now` is
always passed; nothing sleeps."""
import ctypes as C

import numpy as np
import pytest

import oracle as O
import srd_amd as S

pytestmark = pytest.mark.gpu

M64 = (1 << 64) - 1
NOW = 1_700_000_000
CHUNK = S.GATHER_CHUNK


@pytest.fixture(scope="module")
def ctx():
    c = S.Context(0)
    yield c
    c.close()


def le64(x):
    return int(x).to_bytes(8, "little")


def ns_key(key, prefix=S.TTL_PREFIX):
    return le64(O.xxh3_64(prefix)) + le64(O.xxh3_64(key))


def ns_hash(key, prefix=S.TTL_PREFIX):
    return O.xxh3_64(ns_key(key, prefix))


def dev_u64(a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a, np.uint64).view(np.int64).copy()).cuda()


def keys_to_dev(keys):
    import torch
    buf, offs, lens = S._blob(keys)
    return torch.from_numpy(buf.copy()).cuda(), dev_u64(offs), dev_u64(lens)


def sync(ctx):
    S._sync_ctx(ctx, 0)


def ptr(t):
    return C.c_void_p(t.data_ptr()) if t is not None else None


# ---------------------------------------------------------------------------
# namespaced hashes

KEY_LENS = [0, 1, 3, 4, 8, 9, 16, 17, 128, 129, 240, 241, 1025]


def ns_device(ctx, prefix_hash, keys, want_ns=True):
    """srd_namespace_hash_batch_device into sentinel-filled arrays one element longer than needed."""
    import torch
    n = len(keys)
    kb, ko, kl = keys_to_dev(keys)
    out = torch.full((n + 1,), 0x5A5A5A5A5A5A5A5A, dtype=torch.int64, device="cuda")
    ns = torch.full((16 * (n + 1),), 0xA5, dtype=torch.uint8, device="cuda") if want_ns else None
    S._after_torch(ctx, out.device)
    S._check(S.lib().srd_namespace_hash_batch_device(ctx.h, prefix_hash, ptr(kb), ptr(ko), ptr(kl), n, ptr(ns), ptr(out),
                                                     C.c_void_p(ctx.stream)))
    sync(ctx)
    h = out.cpu().numpy().view(np.uint64)
    assert h[n] == 0x5A5A5A5A5A5A5A5A
    b = ns.cpu().numpy().tobytes() if want_ns else None
    if want_ns:
        assert b[16 * n:] == b"\xA5" * 16
    return [int(x) for x in h[:n]], b


@pytest.mark.parametrize("n", [0, 1, 64, 65, 257])
def test_namespace_hashes_match_the_oracle(ctx, n):
    rng = np.random.default_rng(0x7714 + n)
    keys = [rng.integers(0, 256, KEY_LENS[(i + n) % len(KEY_LENS)], dtype=np.uint8).tobytes() for i in range(n)]
    ph = O.xxh3_64(S.TTL_PREFIX)
    h, b = ns_device(ctx, ph, keys)
    assert h == [ns_hash(k) for k in keys]
    assert b[: 16 * n] == b"".join(ns_key(k) for k in keys)
    assert ns_device(ctx, ph, keys, want_ns=False)[0] == h
    # the host-pointer twin and the Python class on top of it
    hs = S.NamespaceHasher(S.TTL_PREFIX, ctx)
    assert hs.prefix_hash == ph and hs.hash_batch(keys) == h


def test_every_key_length_and_the_reference_goldens(ctx, ref_goldens):
    rng = np.random.default_rng(0x7715)
    keys = [rng.integers(0, 256, ln, dtype=np.uint8).tobytes() for ln in KEY_LENS]
    h, b = ns_device(ctx, O.xxh3_64(b"some prefix"), keys)
    assert h == [ns_hash(k, b"some prefix") for k in keys]
    assert b[: 16 * len(keys)] == b"".join(ns_key(k, b"some prefix") for k in keys)
    # tests/namespace_hasher_tests.rs' values, out of d_ns_out
    assert len(ref_goldens["namespace"]) == 2
    for g in ref_goldens["namespace"]:
        prefix, key = g["prefix"].encode(), g["key"].encode()
        _, b = ns_device(ctx, O.xxh3_64(prefix), [key])
        assert b[:16].hex() == g["out"]
        assert S.NamespaceHasher(prefix, ctx).namespace(key).hex() == g["out"]


# ---------------------------------------------------------------------------
# writes

def test_ttl_writes_match_the_oracle_and_the_prefix_is_applied(ctx):
    import torch
    rng = np.random.default_rng(0x7716)
    keys = [b"test_key"] + [b"k%d" % i for i in range(6)]
    vals = [b"hello"] + [rng.integers(0, 256, ln, dtype=np.uint8).tobytes() for ln in (0, 1, 55, 56, 57, 3000)]
    ttls = [60, 0, 1, M64, M64 - NOW, M64 - NOW + 1, 7]
    exps = [NOW + 60, NOW, NOW + 1, M64, M64, M64, NOW + 7]  # the add saturates
    buf, tail = bytearray(), 0
    tail = O.write_entries(buf, tail, [(ns_hash(k), le64(e) + v) for k, e, v in zip(keys, exps, vals)])
    want = bytes(buf[:tail])

    a = S.DeviceStore.create(1 << 16, ctx)
    assert a.batch_write_with_ttl(keys, vals, ttls, now=NOW) == tail
    assert a.bytes() == want
    # values as device segments: the header is a slice of one device uint64[n]
    b = S.DeviceStore.create(1 << 16, ctx)
    ents = []
    for v in vals:
        t = torch.from_numpy(np.frombuffer(v, np.uint8).copy()).cuda()
        cut = len(v) // 3
        ents.append([t[:cut].clone(), t[cut:].clone()] if len(v) > 1 else [t] if len(v) else [])
    assert b.batch_write_stream_with_ttl(keys, ents, ttls, now=NOW) == tail
    assert b.bytes() == want
    # one number for all keys, and the single-key form
    c = S.DeviceStore.create(1 << 12, ctx)
    c.write_with_ttl(b"test_key", b"hello", 60, now=NOW)
    assert c.bytes() == want[: c.tail]
    for st in (a, b):
        # test_ttl_prefix_is_applied: nothing under the raw key, header + value under the namespaced key
        assert st.read(b"test_key") is None
        assert st.read(ns_key(b"test_key")) == le64(NOW + 60) + b"hello"
        assert st.len() == len(keys)
    assert O.xxh3_64(ns_key(b"test_key")) == ns_hash(b"test_key") != O.xxh3_64(b"test_key")


# ---------------------------------------------------------------------------
# one store for resolve, reads and eviction

RNG = np.random.default_rng(0x7717)
V64 = RNG.integers(1, 256, 64, dtype=np.uint8).tobytes()
VBIG = RNG.integers(0, 256, CHUNK, dtype=np.uint8).tobytes()
# key -> (expiry, value) of a TTL entry / the raw payload of an entry too short to be one
TTL_ENTRIES = {
    b"len8": (NOW + 100, b""),        # an empty value
    b"len9": (NOW, b"z"),             # expires exactly now
    b"len72": (NOW - 1, V64),
    b"big": (NOW + 1, VBIG),          # GATHER_CHUNK + 8 bytes of payload
    b"forever": (M64, V64[::-1]),
    b"epoch": (0, b"\x01" + V64),
    b"deleted": (NOW + 5, b"gone in the session"),
    b"tombstoned": (NOW + 5, b"gone on disk"),
}
SHORT = {b"len1": b"\x07", b"len7": b"sevenby"}
QUERIES = [b"len1", b"len9", b"len7", b"len8", b"len72", b"big", b"forever", b"epoch", b"absent", b"deleted",
           b"tombstoned", b"plain", b"len9", b"big", b"epoch", b"len72", b"len9"]


def model_status(key):
    if key in SHORT:
        return S.TTL_TOO_SHORT
    if key not in TTL_ENTRIES or key in (b"deleted", b"tombstoned"):
        return S.TTL_NOT_FOUND
    return S.TTL_EXPIRED if NOW >= TTL_ENTRIES[key][0] else S.TTL_LIVE


def session_bytes():
    """The oracle's store: the TTL entries, the short ones, a plain write, and a
    tombstone as the newest entry of b"tombstoned"."""
    buf, tail = bytearray(), 0
    ents = [(ns_hash(k), le64(e) + v) for k, (e, v) in TTL_ENTRIES.items()]
    ents += [(ns_hash(k), p) for k, p in SHORT.items()]
    ents += [(O.xxh3_64(b"plain"), le64(NOW + 50) + b"written by a plain write")]
    tail = O.write_entries(buf, tail, ents)
    tail = O.write_entries(buf, tail, [(ns_hash(b"tombstoned"), b"\x00")], allow_null=True)
    return buf, tail


def open_session(ctx, extra=4096):  # (room for the tombstones)
    """... re-opened on the device, then b"deleted" deleted in the session.
    Returns the store, the oracle's bytes after the delete and its tail."""
    import torch
    buf, tail = session_bytes()
    dev = torch.zeros(S.padded_size(tail) + extra, dtype=torch.uint8, device="cuda")
    dev[:tail] = torch.from_numpy(np.frombuffer(bytes(buf[:tail]), np.uint8).copy()).cuda()
    st = S.DeviceStore.open(dev, tail, ctx)
    assert st.tail == tail
    st.batch_delete_key_hashes([ns_hash(b"deleted")])
    tail = O.write_entries(buf, tail, [(ns_hash(b"deleted"), b"\x00")], allow_null=True)
    assert st.bytes() == bytes(buf[:tail])
    return st, buf, tail


def ranges_of(buf, tail):
    """{key_hash: (payload_start, meta_off)} of each key's newest entry."""
    return {e["key_hash"]: (e["payload_start"], e["meta_off"]) for e in O.chain(bytes(buf[:tail]), tail, False)}


SENT = 0x7E7E7E7E7E7E7E7E


def resolve(ctx, st, queries, fused, with_optional=True):
    """The resolve call as it is, outputs sentinel-filled and one element longer than n."""
    import torch
    n = len(queries)
    outs = [torch.full((n + 1,), SENT, dtype=torch.int64, device="cuda") for _ in range(4)]  # start, end, expiry, hashes
    status = torch.full((n + 1,), 0x7E, dtype=torch.uint8, device="cuda")
    counts = torch.full((5,), SENT, dtype=torch.int64, device="cuda")
    idx = st.index
    ex = outs[2] if with_optional else None
    cn = counts if with_optional else None
    S._after_torch(ctx, status.device)
    if fused:
        kb, ko, kl = keys_to_dev(queries)
        S._check(S.lib().srd_ttl_resolve_keys_device(
            ctx.h, ptr(idx.table), idx.nbytes, ptr(st.buf), st.tail, O.xxh3_64(S.TTL_PREFIX), ptr(kb), ptr(ko), ptr(kl),
            n, NOW, ptr(outs[3]), ptr(outs[0]), ptr(outs[1]), ptr(ex), ptr(status), ptr(cn), C.c_void_p(ctx.stream)))
    else:
        q = dev_u64([ns_hash(k) for k in queries])
        S._check(S.lib().srd_ttl_resolve_device(
            ctx.h, ptr(idx.table), idx.nbytes, ptr(st.buf), st.tail, ptr(q), n, NOW, ptr(outs[0]), ptr(outs[1]),
            ptr(ex), ptr(status), ptr(cn), C.c_void_p(ctx.stream)))
    sync(ctx)
    return [o.cpu().numpy().view(np.uint64) for o in outs] + [status.cpu().numpy(), counts.cpu().numpy().view(np.uint64)]


def test_resolve_hashed_and_fused(ctx):
    st, buf, tail = open_session(ctx)
    before, n_keys = st.bytes(), st.len()
    rg = ranges_of(buf, tail)
    n = len(QUERIES)
    want_status = np.array([model_status(k) for k in QUERIES] + [0x7E], np.uint8)
    want_start, want_end, want_exp = (np.full(n + 1, SENT, np.uint64) for _ in range(3))
    for i, k in enumerate(QUERIES):
        s = want_status[i]
        want_start[i], want_end[i] = rg[ns_hash(k)] if s == S.TTL_LIVE else (0, 0)
        want_exp[i] = TTL_ENTRIES[k][0] if s in (S.TTL_LIVE, S.TTL_EXPIRED) else 0
    assert sorted(set(want_status[:n])) == [0, 1, 2, 3]  # every status occurs
    want_counts = np.array([int((want_status[:n] == s).sum()) for s in range(4)] + [SENT], np.uint64)
    for fused in (False, True):
        start, end, exp, hashes, status, counts = resolve(ctx, st, QUERIES, fused)
        assert np.array_equal(status, want_status), (fused, status)
        assert np.array_equal(start, want_start) and np.array_equal(end, want_end), fused
        assert np.array_equal(exp, want_exp), fused
        assert np.array_equal(counts, want_counts), (fused, counts)
        want_h = np.array([ns_hash(k) for k in QUERIES] + [SENT], np.uint64) if fused else np.full(n + 1, SENT, np.uint64)
        assert np.array_equal(hashes, want_h), fused
        # the nullable outputs left out: the same verdicts, nothing else written
        start2, end2, exp2, _h, status2, counts2 = resolve(ctx, st, QUERIES, fused, with_optional=False)
        assert np.array_equal(status2, want_status) and np.array_equal(start2, want_start)
        assert np.array_equal(end2, want_end) and (exp2 == SENT).all() and (counts2 == SENT).all()
        # n = 0: the counts are zeroed, nothing else is touched
        o = resolve(ctx, st, [], fused)
        assert all((a == SENT).all() for a in o[:4]) and o[4][0] == 0x7E and list(o[5]) == [0, 0, 0, 0, SENT]
    # a LIVE range is the whole payload: the header and the value
    i = QUERIES.index(b"big")
    assert want_end[i] - want_start[i] == CHUNK + 8
    st.index._live = None
    assert st.bytes() == before and st.len() == n_keys  # the call reads only


def test_reads_packed_and_scattered(ctx):
    import torch
    st, buf, tail = open_session(ctx)
    before, n_keys = st.bytes(), st.len()
    want_status = [model_status(k) for k in QUERIES]
    want_vals = [TTL_ENTRIES[k][1] if s == S.TTL_LIVE else None for k, s in zip(QUERIES, want_status)]
    r = st.batch_read_with_ttl(QUERIES, now=NOW, evict=False)
    assert list(r.status) == want_status and r.values() == want_vals and r.n_evicted == 0
    assert [int(x) for x in r.expiry] == [TTL_ENTRIES[k][0] if s in (S.TTL_LIVE, S.TTL_EXPIRED) else 0
                                          for k, s in zip(QUERIES, want_status)]
    assert r.is_valid_checksum() == [True if s == S.TTL_LIVE else None for s in want_status]
    # the gathered payloads carry their headers
    assert r.gather.payloads()[QUERIES.index(b"len8")] == le64(NOW + 100)

    # scattered: a LIVE value into two tensors of odd sizes, everything else into 3 bytes that stay as they were
    def dest(v):
        if v is None:
            return [torch.full((3,), 0xA5, dtype=torch.uint8, device="cuda")]
        if not v:
            return []  # an empty value: only the header is read
        cut = min(len(v), 4097) if len(v) > 4097 else len(v) // 2
        return [torch.full((cut,), 0xA5, dtype=torch.uint8, device="cuda"),
                torch.full((len(v) - cut,), 0xA5, dtype=torch.uint8, device="cuda")]
    ents = [dest(v) for v in want_vals]
    r2 = st.batch_read_with_ttl_into(QUERIES, ents, now=NOW, evict=False)
    assert list(r2.status) == want_status and r2.n_evicted == 0
    assert r2.is_valid_checksum() == [True if s == S.TTL_LIVE else None for s in want_status]
    for v, e in zip(want_vals, ents):
        got = b"".join(t.cpu().numpy().tobytes() for t in e)
        assert got == (v if v is not None else b"\xA5" * 3)
    assert st.bytes() == before and st.len() == n_keys and st.tail == tail  # evict=False: bytes and index untouched

    # one flipped value byte: LIVE, the checksum says so, the bytes are delivered as they are
    s0, _m = ranges_of(buf, tail)[ns_hash(b"big")]
    st.buf[s0 + 8 + 1000] ^= 0x40
    torch.cuda.synchronize()
    flipped = bytearray(VBIG)
    flipped[1000] ^= 0x40
    r3 = st.batch_read_with_ttl([b"big", b"forever"], now=NOW, evict=False)
    assert list(r3.status) == [S.TTL_LIVE, S.TTL_LIVE] and r3.is_valid_checksum() == [False, True]
    assert list(r3.gather.status) == [S.GATHER_BAD_CRC, S.GATHER_OK]
    assert r3.values() == [bytes(flipped), V64[::-1]]
    ents = [dest(bytes(flipped)), dest(V64[::-1])]
    r4 = st.batch_read_with_ttl_into([b"big", b"forever"], ents, now=NOW, evict=False)
    assert r4.is_valid_checksum() == [False, True]
    assert b"".join(t.cpu().numpy().tobytes() for t in ents[0]) == bytes(flipped)


def test_eviction_writes_the_reference_tombstones(ctx):
    st, buf, tail = open_session(ctx)
    n_keys = st.len()
    # the distinct expired keys in batch order of their last occurrence
    expired = [k for k in QUERIES if model_status(k) == S.TTL_EXPIRED]
    order = sorted(set(expired), key=lambda k: max(i for i, q in enumerate(QUERIES) if q == k))
    assert order == [b"epoch", b"len72", b"len9"] and len(expired) == 7
    r = st.batch_read_with_ttl(QUERIES, now=NOW)
    assert list(r.status) == [model_status(k) for k in QUERIES]  # judged as the store was: EXPIRED each time
    assert r.n_evicted == len(order)
    new_tail = O.write_entries(buf, tail, [(ns_hash(k), b"\x00") for k in order], allow_null=True)
    assert new_tail == tail + 21 * len(order) == st.tail
    assert st.bytes() == bytes(buf[:new_tail])
    assert st.len() == n_keys - len(order)
    st.index._live = None
    assert st.len() == n_keys - len(order)  # (counted from the table)
    r = st.batch_read_with_ttl(QUERIES, now=NOW)
    assert [s for k, s in zip(QUERIES, r.status) if k in order] == [S.TTL_NOT_FOUND] * len(expired)
    assert r.n_evicted == 0 and st.tail == new_tail  # nothing expired: nothing written
    # the single-key form
    assert st.read_with_ttl(b"forever", now=NOW) == V64[::-1]
    assert st.read_with_ttl(b"big", now=NOW + 1) is None and st.tail == new_tail + 21
    with pytest.raises(KeyError):
        st.read_with_ttl(b"big", now=NOW)
    with pytest.raises(KeyError):
        st.read_with_ttl(b"plain", now=NOW)
    with pytest.raises(ValueError, match="Data too short to contain TTL"):
        st.read_with_ttl(b"len7", now=NOW)


def test_eviction_refused_one_byte_short(ctx):
    import torch
    st, buf, tail = open_session(ctx)
    idx = st.index
    qs = [b"len9", b"forever", b"len72", b"len9"]
    _s, _e, _x, _h, status, _c = resolve(ctx, st, qs, False)
    d_h, d_s = dev_u64([ns_hash(k) for k in qs]), torch.from_numpy(status[:4].copy()).cuda()
    need = S.padded_size(tail + 21 * 2)
    whole = torch.zeros(need + 64, dtype=torch.uint8, device="cuda")
    whole[:need] = st.buf[:need]  # (zero above the tail)
    table_before, whole_before, n_keys = idx.table.clone(), whole.clone(), st.len()
    for cap, ok in ((need - 1, False), (need, True)):
        used, nt, nd = C.c_uint64(idx.used), C.c_uint64(77), C.c_uint64(77)
        S._after_torch(ctx, whole.device)
        rc = S.lib().srd_ttl_evict_device(ctx.h, ptr(idx.table), idx.nbytes, C.byref(used), ptr(d_h), ptr(d_s), 4, tail,
                                          ptr(whole), cap, C.byref(nt), C.byref(nd))
        if not ok:
            assert rc == S.SRD_ERR_ARG and "file_cap" in S.lib().srd_last_error().decode()
            assert nt.value == tail and nd.value == 0 and used.value == idx.used
            assert torch.equal(whole, whole_before) and torch.equal(idx.table, table_before)
            idx._live = None
            assert st.len() == n_keys
        else:
            assert rc == 0 and nt.value == tail + 42 and nd.value == 2
            want = O.write_entries(buf, tail, [(ns_hash(k), b"\x00") for k in (b"len72", b"len9")], allow_null=True)
            assert whole[:want].cpu().numpy().tobytes() == bytes(buf[:want])
            assert torch.equal(whole[S.padded_size(want):], whole_before[S.padded_size(want):])


# ---------------------------------------------------------------------------
# the sweep

def test_sweep_then_compact_leaves_the_survivors(ctx):
    n = 3000
    keys = [b"sweep-%d" % i for i in range(n)]
    vals = [bytes([1 + i % 255]) * (1 + i % 40) for i in range(n)]
    exps = [NOW - (i % 5) if i % 3 == 0 else NOW + 1 + ((i * 7919) % 100003) for i in range(n)]
    short = [b"short-%d" % i for i in range(5)]
    gone = [7, 8, 1500, 2998]  # deleted in the session: two expired or not, whatever they are
    st = S.DeviceStore.create(1 << 20, ctx)
    buf, tail = bytearray(), 0
    for lo in range(0, n, 1000):  # three batches, the short ones in between
        st.batch_write_with_ttl(keys[lo: lo + 1000], vals[lo: lo + 1000], [e - 1000 for e in exps[lo: lo + 1000]],
                                now=1000)
        tail = O.write_entries(buf, tail, [(ns_hash(k), le64(e) + v) for k, e, v in
                                           zip(keys[lo: lo + 1000], exps[lo: lo + 1000], vals[lo: lo + 1000])])
        if lo == 1000:
            st.batch_write_with_key_hashes([ns_hash(k) for k in short], [b"abc"] * 5)
            tail = O.write_entries(buf, tail, [(ns_hash(k), b"abc") for k in short])
    st.batch_delete_key_hashes([ns_hash(keys[i]) for i in gone])
    tail = O.write_entries(buf, tail, [(ns_hash(keys[i]), b"\x00") for i in gone], allow_null=True)
    assert st.bytes() == bytes(buf[:tail])
    assert st.index.capacity >= 8192  # several blocks of 256 slots
    live = [i for i in range(n) if i not in gone]
    expired = [i for i in live if NOW >= exps[i]]
    survivors = [i for i in live if NOW < exps[i]]
    assert len(expired) > 900 and len(survivors) > 1900

    plan = st.sweep_expired(now=NOW, plan=True)
    want = (len(live) + 5, len(expired), 5, min(exps[i] for i in survivors))
    assert (plan.n_judged, plan.n_expired, plan.n_short, plan.next_expiry) == want
    assert st.tail == tail and st.bytes() == bytes(buf[:tail]) and st.len() == len(live) + 5  # the plan writes nothing

    ws = ctx.device_bytes()
    got = st.sweep_expired(now=NOW)
    assert (got.n_judged, got.n_expired, got.n_short, got.next_expiry) == want
    assert ctx.device_bytes() >= ws > 0  # the workspace is the context's
    # one tombstone per expired key, in ascending offset of the entry it removes (= write order here)
    tail = O.write_entries(buf, tail, [(ns_hash(keys[i]), b"\x00") for i in expired], allow_null=True)
    assert st.tail == tail and st.bytes() == bytes(buf[:tail])
    assert st.len() == len(survivors) + 5
    st.index._live = None
    assert st.len() == len(survivors) + 5
    again = st.sweep_expired(now=NOW)
    assert (again.n_judged, again.n_expired, again.n_short, again.next_expiry) == (len(survivors) + 5, 0, 5, want[3])
    assert st.tail == tail

    cs = st.compact()
    assert int(cs.n_entries) == len(survivors) + 5 == st.len() and st.tail < tail
    r = st.batch_read_with_ttl(keys + short, now=NOW, evict=False)
    sv = set(survivors)
    assert list(r.status) == [S.TTL_LIVE if i in sv else S.TTL_NOT_FOUND for i in range(n)] + [S.TTL_TOO_SHORT] * 5
    assert r.values() == [vals[i] if i in sv else None for i in range(n)] + [None] * 5
    assert [int(x) for x in r.expiry[:n]] == [exps[i] if i in sv else 0 for i in range(n)]


def test_sweep_empty_store_and_smallest_table(ctx):
    st = S.DeviceStore.create(1 << 12, ctx)
    for plan in (True, False):
        s = st.sweep_expired(now=NOW, plan=plan)
        assert (s.n_judged, s.n_expired, s.n_short, s.next_expiry) == (0, 0, 0, M64) and st.tail == 0
    keys = [b"small-%d" % i for i in range(20)]
    exps = [NOW + 10 - i for i in range(20)]  # 10 live, 10 expired (the eleventh exactly now)
    st.batch_write_with_ttl(keys, [b"v%d" % i for i in range(20)], [e - 5 for e in exps], now=5)
    assert st.index.capacity == 64
    buf, tail = bytearray(st.bytes()), st.tail
    s = st.sweep_expired(now=NOW)
    assert (s.n_judged, s.n_expired, s.n_short, s.next_expiry) == (20, 10, 0, NOW + 1)
    tail = O.write_entries(buf, tail, [(ns_hash(k), b"\x00") for k in keys[10:]], allow_null=True)
    assert st.bytes() == bytes(buf[:tail]) and st.len() == 10 and st.index.capacity == 64
    # everything expires: no survivor has an expiry
    s = st.sweep_expired(now=M64)
    assert (s.n_judged, s.n_expired, s.n_short, s.next_expiry) == (10, 10, 0, M64) and st.len() == 0
    # the tombstones that do not fit: refused with the store as it was
    full = S.DeviceStore.create(4096, ctx)
    full.write_with_ttl(b"k", b"v" * 4062, 1, now=NOW)  # the entry ends at 4090: a tombstone would end in the next tile
    before = full.bytes()
    assert full.tail == 4090 and S.padded_size(4090 + 21) > full.buf.numel() == S.padded_size(4090)
    with pytest.raises(ValueError):
        full.sweep_expired(now=NOW + 1)
    assert full.bytes() == before and full.len() == 1 and full.tail == 4090
    s = full.sweep_expired(now=NOW + 1, plan=True)  # the plan still says what a sweep would do
    assert (s.n_judged, s.n_expired, s.n_short, s.next_expiry) == (1, 1, 0, M64)
