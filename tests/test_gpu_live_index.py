"""The device KeyIndexer kept live: DataStore::reindex (data_store.rs:224-259)
over KeyIndexer::insert / remove (key_indexer.rs:135-160, :174-178) applied to
the device table in place, batch_delete_key_hashes (data_store.rs:995-1024) and
the DeviceStore session (write -> reindex -> read) over a store in HBM.

The model of every table test is a Python dict driven by the reference loop:

    D = {kh for kh, mo, t in batch if t}
    for kh, mo, t in batch: index.pop(kh, None) if kh in D else index[kh] = pack(kh >> 48, mo)

All comparisons are bit-exact."""
import ctypes as C
import random

import numpy as np
import pytest

import oracle as O
import srd_amd as S

pytestmark = pytest.mark.gpu

M64 = (1 << 64) - 1


@pytest.fixture(scope="module")
def ctx():
    c = S.Context(0)
    yield c
    c.close()


def pack(kh, mo):
    return ((kh >> 48) << 48) | mo


def idx_slot(k, log2cap):
    """The table's home slot of a key hash (csrc/srd_index.hip), restated."""
    k ^= k >> 29
    return ((k * 0x9E3779B97F4A7C15) & M64) >> (64 - log2cap)


def model_apply(index, batch):
    """The reference loop; returns (inserted, updated, removed) per distinct key."""
    before = {kh: kh in index for kh, _, _ in batch}
    D = {kh for kh, _, t in batch if t}
    for kh, mo, t in batch:
        if kh in D:
            index.pop(kh, None)
        else:
            index[kh] = pack(kh, mo)
    ins = sum(1 for kh, was in before.items() if not was and kh in index)
    upd = sum(1 for kh, was in before.items() if was and kh in index)
    rem = sum(1 for kh, was in before.items() if was and kh not in index)
    return ins, upd, rem


def build_store(seed):
    """The store of tests/test_gpu_lookup.py: ~300 keys, overwrites, tombstones."""
    rng = random.Random(seed)
    buf = bytearray()
    tail = 0
    keys = [b"key-%d" % i for i in range(300)] + [b"a", b"b", b"c", b"d"]
    for rnd in range(4):
        batch = []
        for k in rng.sample(keys, 120):
            if rnd and rng.random() < 0.25:
                batch.append((k, b"\x00"))
            else:
                p = bytes(rng.getrandbits(8) for _ in range(rng.choice([1, 3, 7, 64, 100, 4096, 5000])))
                batch.append((k, b"\x01" if p == b"\x00" else p))
        tail = O.write_entries(buf, tail, [(O.xxh3_64(k), p) for k, p in batch], allow_null=True)
    return bytes(buf), keys


@pytest.fixture(scope="module")
def store1():
    f, keys = build_store(11)
    return f, keys, O.key_indexer_build(np.frombuffer(f, np.uint8), len(f))


def to_dev(f, extra=0):
    import torch
    dev = torch.zeros(S.padded_size(len(f) + extra), dtype=torch.uint8, device="cuda")
    dev[: len(f)] = torch.frombuffer(bytearray(f), dtype=torch.uint8).cuda()
    torch.cuda.synchronize()  # the library launches on its own stream, not ordered behind torch's
    return dev


def index_of(ctx, pairs):
    """A DeviceIndex built from host (key_hash, packed) pairs."""
    import torch
    k = torch.from_numpy(np.array([p[0] for p in pairs], np.uint64).view(np.int64)).cuda()
    v = torch.from_numpy(np.array([p[1] for p in pairs], np.uint64).view(np.int64)).cuda()
    torch.cuda.synchronize()
    return S.DeviceIndex(k.data_ptr(), v.data_ptr(), len(pairs), ctx)


def raw_apply(idx, batch):
    """srd_index_table_apply_device itself: (rc, used after, stats)."""
    import torch
    kh = idx._as_dev([b[0] for b in batch])
    mo = idx._as_dev([b[1] for b in batch])
    tb = idx._as_dev([int(b[2]) for b in batch], np.uint8)
    used, st = C.c_uint64(idx.used), S.ApplyStats()
    torch.cuda.synchronize()
    rc = S.lib().srd_index_table_apply_device(idx.ctx.h, C.c_void_p(idx.table.data_ptr()), idx.nbytes, C.byref(used),
                                              C.c_void_p(kh.data_ptr()), C.c_void_p(mo.data_ptr()),
                                              C.c_void_p(tb.data_ptr()), len(batch), C.byref(st),
                                              C.c_void_p(idx.ctx.stream))
    torch.cuda.synchronize()
    return rc, int(used.value), st.as_tuple()


def exported(idx):
    k, p = idx.export()
    return list(zip((int(x) for x in k.cpu().numpy().view(np.uint64)), (int(x) for x in p.cpu().numpy().view(np.uint64))))


def check_table(idx, model, probe):
    got = idx.get_packed(np.array(probe, np.uint64))
    for h, g in zip(probe, got):
        assert int(g) == model.get(h, S.INDEX_NONE), hex(h)
    assert exported(idx) == sorted(model.items(), key=lambda kv: kv[1] & S.OFFSET_MASK)
    assert len(idx) == len(model)


def merge_groups(rng, groups):
    """One batch out of per-key op lists: random interleaving, each list's order kept."""
    groups = [list(g) for g in groups if g]
    out = []
    while groups:
        g = rng.choice(groups)
        out.append(g.pop(0))
        if not g:
            groups.remove(g)
    return out


def test_apply_matches_reference_loop(ctx, store1):
    f, keys, on_disk = store1
    dev = to_dev(f)
    r = S.validate_index_device(dev.data_ptr(), len(f), 0, ctx)
    assert r.final_len == len(f)
    idx = S.DeviceIndex(r.index_key_hash, r.index_packed, r.n_index, ctx)
    model = dict(on_disk)
    slots = set(model)  # keys that ever took a slot: `used` grows by first-time keys only
    rng = random.Random(5)
    hashes = [O.xxh3_64(k) for k in keys]
    fresh = [O.xxh3_64(b"new-%d" % i) for i in range(400)]
    never = [O.xxh3_64(b"never-%d" % i) for i in range(20)] + [12345]
    seen = set(hashes) | {0, M64}
    next_off = [len(f) + 1]

    def off():
        next_off[0] += rng.choice([21, 64, 85, 4116])
        return next_off[0]

    # a key removed before the first round, so that round 0 has a revival too
    gone = [rng.choice(sorted(model))]
    assert idx.remove(gone) == 1
    model.pop(gone[0])
    check_table(idx, model, sorted(seen) + never)
    assert idx.used == len(slots)

    for rnd in range(6):
        live = sorted(model)
        rep, a, b = rng.sample(live, 3)
        special = {rep, a, b, gone[-1], 0, M64}
        groups = [
            [(rep, off(), False) for _ in range(3 + rnd % 2)],            # one key three or four times
            [(a, off(), False), (a, off(), True)],                        # written, then deleted
            [(b, off(), True), (b, off(), False)],                        # deleted, then written: absent too
            [(gone[-1], off(), False)],                                   # revival of a removed key
            [(0, off(), rnd == 3)],                                       # the legal key hashes 0 ...
            [(M64, off(), False)] + ([(M64, off(), True)] if rnd == 4 else []),  # ... and 2^64 - 1
        ]
        for kh in rng.sample([h for h in hashes if h not in special], 12) + [fresh.pop() for _ in range(14)]:
            groups.append([(kh, off(), rng.random() < 0.2)])
        extra = fresh.pop()  # a new key written twice, the two lanes racing for one slot
        groups.append([(extra, off(), False), (extra, off(), False)])
        batch = merge_groups(rng, groups)
        assert len(batch) <= 64
        seen |= {kh for kh, _, _ in batch}
        want = model_apply(model, batch)
        slots |= set(model)
        got = idx.apply([x[0] for x in batch], [x[1] for x in batch], [int(x[2]) for x in batch])
        assert got == want, rnd
        assert a not in model and b not in model and gone[-1] in model
        check_table(idx, model, sorted(seen) + never)
        assert idx.used == len(slots), rnd
        gone.append(a)


def test_duplicate_storm_claims_one_slot_per_key(ctx):
    # 4096 pairs (16 blocks) over 64 new keys and 8 deleted ones: every key's
    # lanes race for its slot, in the dedupe and nowhere else
    rng = random.Random(9)
    keys = [rng.getrandbits(64) for _ in range(72)]
    batch = [(rng.choice(keys[:64]), 100 + 21 * i, False) for i in range(4096)]
    for i in rng.sample(range(4096), 40):
        batch[i] = (rng.choice(keys[64:]), batch[i][1], rng.random() < 0.5)
    for k in keys[64:]:
        batch[rng.randrange(4096)] = (k, 0, True)
    for j, i in enumerate(rng.sample(range(4096), 64)):
        batch[i] = (keys[j], batch[i][1], False)  # (every one of the 64 occurs)
    idx = index_of(ctx, [(k, pack(k, 50 + i)) for i, k in enumerate(keys[60:68])])
    model = {k: pack(k, 50 + i) for i, k in enumerate(keys[60:68])}
    slots = set(model)
    want = model_apply(model, batch)
    slots |= set(model)
    assert idx.apply([x[0] for x in batch], [x[1] for x in batch], [int(x[2]) for x in batch]) == want
    check_table(idx, model, keys + [0, M64])
    assert idx.used == len(slots)


def wrap_keys():
    """Three key hashes whose home slot in a 64-slot table is 62 and three at 63:
    their probe chain covers slots 62, 63, 0, 1, 2, 3."""
    rng = random.Random(1)
    by_home = {62: [], 63: []}
    while min(len(v) for v in by_home.values()) < 3:
        k = rng.getrandbits(64)
        h = idx_slot(k, 6)
        if h in by_home and len(by_home[h]) < 3:
            by_home[h].append(k)
    return [by_home[62][0], by_home[63][0], by_home[62][1], by_home[63][1], by_home[62][2], by_home[63][2]]


def test_smallest_table_chain_across_the_wrap(ctx):
    ks = wrap_keys()
    # under the restated slot function the chain really wraps: linear probing
    # of six keys with homes 62 / 63 fills 62, 63 and then 0 .. 3 in any order
    occ = set()
    for k in ks:
        s = idx_slot(k, 6)
        assert s in (62, 63)
        while s in occ:
            s = (s + 1) & 63
        occ.add(s)
    assert occ == {62, 63, 0, 1, 2, 3} and len(ks) >= 5
    model = {k: pack(k, 1000 + 64 * i) for i, k in enumerate(ks[:3])}
    idx = index_of(ctx, list(model.items()))
    assert idx.nbytes == 16 * 64 == S.lib().srd_index_table_bytes(32)
    batch = [(k, 2000 + 64 * i, False) for i, k in enumerate(ks[3:])]
    assert idx.apply(*zip(*batch)) == model_apply(model, batch) == (3, 0, 0)
    probe = ks + [0, M64, 777]
    check_table(idx, model, probe)
    assert idx.used == 6
    # which key sits in the middle of the chain depends on who won each claim:
    # every key takes its turn, so the middle ones do
    off = 3000
    for k in ks:
        assert idx.apply([k], [0], [1]) == model_apply(model, [(k, 0, True)]) == (0, 0, 1)
        check_table(idx, model, probe)  # every other key of the chain is still found
        assert idx.used == 6
        off += 64
        assert idx.apply([k], [off]) == model_apply(model, [(k, off, False)]) == (1, 0, 0)
        check_table(idx, model, probe)
        assert idx.used == 6  # revived in its own slot


def test_full_table_is_refused_unchanged_then_grown(ctx):
    rng = random.Random(3)
    keys = [rng.getrandbits(64) for _ in range(35)]
    model = {k: pack(k, 500 + 32 * i) for i, k in enumerate(keys[:30])}
    idx = index_of(ctx, list(model.items()))
    assert idx.capacity == 64 and idx.used == 30
    before = exported(idx)
    upd = [(k, 9000 + 32 * i, False) for i, k in enumerate(keys[:3])]
    new = [(k, 9500 + 32 * i, False) for i, k in enumerate(keys[30:])]
    refused = new[:2] + upd[:1] + new[2:] + upd[1:]
    rc, used, _ = raw_apply(idx, refused)
    assert rc == S.SRD_ERR_FULL == -5 and used == 30
    assert exported(idx) == before == sorted(model.items(), key=lambda kv: kv[1] & S.OFFSET_MASK)
    ok = upd + new[:2]
    rc, used, st = raw_apply(idx, ok)
    assert rc == 0 and used == 32 and st == model_apply(model, ok) == (2, 3, 0)
    idx._used = used
    idx._live = None
    check_table(idx, model, keys)
    want = model_apply(model, refused)
    assert idx.apply(*[[x[i] for x in refused] for i in range(3)]) == want == (3, 5, 0)
    assert idx.capacity > 64 and idx.used == 35  # the rebuild kept the live keys only (none was deleted)
    check_table(idx, model, keys + [0, M64])


def test_batch_delete_writes_the_reference_tombstones(ctx, store1):
    f, keys, on_disk = store1
    dev = to_dev(f, extra=8192)
    st = S.DeviceStore.open(dev, len(f), ctx)
    assert st.tail == len(f) and st.len() == len(on_disk)
    model = dict(on_disk)
    buf, tail = bytearray(f), len(f)
    flen = len(f)

    def tombstoned(h):  # the key's indexed entry is a tombstone on disk
        mo = on_disk[h] & S.OFFSET_MASK
        prev = int.from_bytes(f[mo + 8:mo + 16], "little")
        return mo - prev == 1 and f[prev] == 0

    dead = [h for h in sorted(on_disk) if tombstoned(h)]
    alive = [h for h in sorted(on_disk) if not tombstoned(h)]
    assert dead and len(alive) > 10

    def delete(hashes):
        nonlocal tail
        kept = [h for h in hashes if h in model]
        new_tail = O.write_entries(buf, tail, [(h, b"\x00") for h in kept], allow_null=True) if kept else tail
        assert st.batch_delete_key_hashes(hashes) == new_tail == tail + 21 * len(kept)
        tail = new_tail
        for h in kept:
            model.pop(h, None)
        assert st.tail == tail and st.bytes() == bytes(buf)  # the whole store, the bytes below the old tail included
        assert st.len() == len(model)
        return kept

    assert delete([alive[0]]) == [alive[0]]  # a key removed earlier in the session
    assert flen % 64 and tail % 64  # (unaligned tails: the writer must leave the bytes below them alone)
    absent = [O.xxh3_64(b"never-1"), 0, M64]
    lst = [absent[0], alive[1], alive[0], dead[0], alive[2], alive[1], absent[1], absent[2], alive[3]]
    kept = delete(lst)
    assert kept == [alive[1], dead[0], alive[2], alive[1], alive[3]]  # input order, the duplicate kept
    assert st.batch_read_hashed_keys(kept) == [None] * len(kept)
    got = st.index.get_packed(np.array(lst, np.uint64))
    assert [int(g) for g in got] == [S.INDEX_NONE] * len(lst)
    assert delete(absent + [alive[0], alive[1]]) == []  # nothing to delete: tail and bytes unchanged
    assert delete([]) == []
    # what is left reads as before
    assert None not in st.batch_read_hashed_keys(alive[4:12])
    # and the store re-opens whole
    r = S.validate_index_device(dev.data_ptr(), tail, 0, ctx)
    assert r.final_len == tail and r.n_crc_bad == 0


def test_device_store_session(ctx):
    import torch
    rng = random.Random(21)
    st = S.DeviceStore.create(600_000, ctx)
    buf, tail = bytearray(), 0
    model, deleted = {}, set()
    keys = [b"k-%d" % i for i in range(40)]
    lens = [1, 3, 7, 64, 100, 4096, 5000]

    def payload(i):
        p = bytes(rng.getrandbits(8) for _ in range(lens[i % len(lens)]))
        return b"\x01" if p == b"\x00" else p

    def check():
        assert st.tail == tail
        probe = keys + [b"missing_key"]
        got = st.batch_read(probe)
        assert got == [model.get(k) for k in probe]
        assert st.len() == len(model) == len(st.index)
        for k in (keys[0], keys[7], keys[39], b"missing_key"):
            assert st.exists(k) == (k in model)

    def write(ks):
        nonlocal tail
        ps = [payload(i) for i in range(len(ks))]
        tail = O.write_entries(buf, tail, [(O.xxh3_64(k), p) for k, p in zip(ks, ps)])
        assert st.batch_write(ks, ps) == tail
        for k, p in zip(ks, ps):
            model[k] = p
            deleted.discard(k)
        check()

    def delete(ks):
        nonlocal tail
        kept = [k for k in ks if k in model]
        if kept:
            tail = O.write_entries(buf, tail, [(O.xxh3_64(k), b"\x00") for k in kept], allow_null=True)
        assert st.batch_delete(ks) == tail
        for k in kept:
            model.pop(k, None)
            deleted.add(k)
        check()

    check()
    write(keys[:20])
    write(keys[10:34])             # overwrites of 10 .. 19
    write(keys[5:12] + keys[30:38] + [keys[6]])  # more overwrites, one key twice in a batch
    delete([keys[3], keys[11], b"missing_key", keys[33], keys[3]])
    delete([keys[3]])              # already gone: nothing written
    write([keys[11], keys[38]])    # a write after a delete
    with pytest.raises(S.SrdError, match="Payload cannot be empty"):
        st.batch_write([b"x"], [b""])
    with pytest.raises(S.SrdError, match="NULL-byte payloads cannot be written directly"):
        st.batch_write([b"x"], [b"\x00"])
    check()

    assert st.bytes() == bytes(buf)
    # the existing read calls on the live table: a removed key is None in srd_batch_read too
    rd = st.index.batch_read(st.buf.data_ptr(), st.tail, [keys[3], keys[0], keys[33], keys[11]])
    assert rd[0] is None and rd[2] is None
    assert [bytes(buf[s:e]) for s, e in (rd[1], rd[3])] == [model[keys[0]], model[keys[11]]]
    r = S.validate_index_device(st.buf.data_ptr(), st.tail, 0, ctx)
    assert r.final_len == tail and r.n_crc_bad == 0
    rk = S.device_view(r.index_key_hash, r.n_index).clone()
    rp = S.device_view(r.index_packed, r.n_index).clone()
    torch.cuda.synchronize()
    reopened = dict(zip((int(x) for x in rk.cpu().numpy().view(np.uint64)),
                        (int(x) for x in rp.cpu().numpy().view(np.uint64))))
    assert reopened == O.key_indexer_build(np.frombuffer(bytes(buf), np.uint8), tail)
    live = dict(exported(st.index))
    assert set(live) == {O.xxh3_64(k) for k in model}
    for h, p in live.items():
        assert reopened[h] == p
    got = st.index.get_packed(np.array(sorted(live), np.uint64))
    assert [int(g) for g in got] == [live[h] for h in sorted(live)]
    assert set(reopened) - set(live) == {O.xxh3_64(k) for k in deleted} and deleted == {keys[3], keys[33]}
    ek, ep = st.index.export()
    a = S.iter_entries_device(st.buf.data_ptr(), tail, ep.data_ptr(), ep.numel(), ctx)
    b = S.iter_entries_device(st.buf.data_ptr(), tail, rp.data_ptr(), rp.numel(), ctx)
    assert len(a[0]) == len(model)
    for x, y in zip(a, b):
        assert np.array_equal(x, y)

    n_before = st.len()
    with pytest.raises(ValueError, match="capacity"):
        st.batch_write([b"big-%d" % i for i in range(200)], [b"\x07" * 4096] * 200)
    assert st.tail == tail and st.len() == n_before and st.bytes() == bytes(buf)
    check()
