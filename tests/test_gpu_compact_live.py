"""A live session compacted on the device: srd_compact_live_device (the live
table's export and the iterator's filter into workspace, the append's layout,
chunk units and checksums as they are, the CRC comparison with the source's
stored checksums, the new table built from pairs that never leave the device)
and the session methods over it: DeviceStore.compact / estimate_compaction_savings
/ iter_entries / reserve.

Expected bytes come from a host model: an EntryIterator restatement over the
session's bytes(), then O.write_entries(bytearray(), 0, [...]) -- compact()'s
write_stream_with_key_hash per iter_entries entry (data_store.rs:706-719).
Every comparison is bit-exact.  Output buffers are 0xA5 before a call and are
checked over the whole allocation: [0, new_len) is the model's store, [new_len,
roundup64(new_len)) is 0xA5 or 0, everything behind is still 0xA5.  The shapes
are the smallest at which the path can go wrong (tests/test_gpu_append.py's
length list, CH = GATHER_CHUNK; more than 256 entries for the finish step's
64-entry wave and 256-thread block)."""
import ctypes as C
import hashlib
import random

import numpy as np
import pytest

import oracle as O
import srd_amd as S

pytestmark = pytest.mark.gpu

CH = S.GATHER_CHUNK
# tests/test_gpu_append.py's LENGTHS
LENGTHS = [1, 2, 15, 16, 17, 63, 64, 65, 1023, 1024, 1025, 1040, 4095, 4096, 4097, 8191, 8192, 8193, 12289,
           CH - 1, CH, CH + 1, 2 * CH, 2 * CH + 17, 3 * CH + 4097]
FILL = 0xA5
SLACK = 8192
NONE = (1 << 64) - 1
MASK48 = (1 << 48) - 1


@pytest.fixture(scope="module")
def ctx():
    c = S.Context(0)
    yield c
    c.close()


def pad64(n):
    return (n + 63) & ~63


def kh(name):
    return O.xxh3_64(name)


def nonzero_bytes(rng, n):
    """n random bytes, the first of them not 0 (no payload is a tombstone or NULL-byte-only)."""
    return bytes([rng.randrange(1, 256)]) + rng.randbytes(n - 1)


def entry_iterator(f: bytes, tail: int):
    """EntryIterator::next (entry_iterator.rs:69-126): (start, end, meta_off, key_hash), newest first
    (tests/test_gpu_iter.py's restatement)."""
    out, seen, cursor = [], set(), tail
    while cursor >= 20:
        mo = cursor - 20
        k = int.from_bytes(f[mo:mo + 8], "little")
        prev = int.from_bytes(f[mo + 8:mo + 16], "little")
        start = prev + ((64 - prev % 64) & 63)
        if mo > prev and mo - prev == 1 and f[prev:mo] == b"\x00":
            start = prev
        if start >= mo or mo > len(f):
            break
        cursor = prev
        if k in seen:
            continue
        seen.add(k)
        if mo - start == 1 and f[start:mo] == b"\x00":
            continue
        out.append((start, mo, mo, k))
    return out


def model_compact(f: bytes, tail: int):
    """(the compacted store's bytes, the iterator's tuples): compact() on the host."""
    its = entry_iterator(f, tail)
    buf = bytearray()
    nt = O.write_entries(buf, 0, [(k, f[s:e]) for s, e, _, k in its])
    assert nt == len(buf)
    return bytes(buf), its


class Model:
    """The reference's operation sequence replayed with the oracle (tests/test_gpu_append.py's, plus compact)."""

    def __init__(self, buf=b"", live=None):
        self.buf, self.tail, self.live = bytearray(buf), len(buf), dict(live or {})

    def write(self, pairs):
        self.tail = O.write_entries(self.buf, self.tail, [(kh(k), p) for k, p in pairs])
        self.live.update(pairs)
        return self.tail

    def delete(self, keys):
        present = [k for k in keys if k in self.live]
        if present:
            self.tail = O.write_entries(self.buf, self.tail, [(kh(k), b"\x00") for k in present], allow_null=True)
        for k in present:
            del self.live[k]
        return self.tail

    def compact(self):
        out, its = model_compact(bytes(self.buf), self.tail)
        assert {k for _, _, _, k in its} == {kh(k) for k in self.live}
        self.buf, self.tail = bytearray(out), len(out)
        return self.tail


def open_store(ctx, f: bytes, room: int = 0):
    import torch
    dev = torch.zeros(S.padded_size(len(f) + room), dtype=torch.uint8, device="cuda")
    if f:
        dev[: len(f)] = torch.frombuffer(bytearray(f), dtype=torch.uint8).cuda()
    st = S.DeviceStore.open(dev, len(f), ctx)
    assert st.tail == len(f)
    return st


def sha(t):
    return hashlib.sha256(t.cpu().numpy().tobytes()).hexdigest()


def source_state(st):
    """(sha256 of the whole store buffer, sha256 of the whole table)."""
    st.index._sync_lib()
    return sha(st.buf), sha(st.index.table)


def first_diff(got, want):
    w = np.frombuffer(want, np.uint8)
    d = np.nonzero(got != w)[0]
    return "first difference at byte %d of %d (%d differ)" % (int(d[0]), len(w), len(d)) if len(d) else "equal"


class Raw:
    """One srd_compact_live_device call on a session's buffer and table, into 0xA5-filled outputs."""

    def __init__(self, ctx, st, n_entries, new_len, out_cap=None, table_bytes=None, d_out=None):
        import torch
        self.alloc = S.padded_size(new_len) + SLACK
        self.out = torch.full((self.alloc,), FILL, dtype=torch.uint8, device="cuda")
        self.tbytes = int(S.lib().srd_index_table_bytes(n_entries))
        self.table = torch.full((self.tbytes,), FILL, dtype=torch.uint8, device="cuda")
        self.stats = S.CompactStats()
        S._after_torch(ctx, self.out.device)  # section 10's stream rule: no host wait between torch's writes and the call
        self.rc = S.lib().srd_compact_live_device(
            ctx.h, C.c_void_p(st.index.table.data_ptr()), st.index.nbytes, C.c_void_p(st.buf.data_ptr()), st.tail,
            C.c_void_p(self.out.data_ptr() if d_out is None else d_out),
            S.padded_size(new_len) if out_cap is None else out_cap, C.c_void_p(self.table.data_ptr()),
            self.tbytes if table_bytes is None else table_bytes, C.byref(self.stats))
        self.msg = S.lib().srd_last_error().decode() if self.rc else ""
        torch.cuda.synchronize()

    def check_bytes(self, want: bytes):
        """The whole output allocation against the model's store."""
        got = self.out.cpu().numpy()
        nt = len(want)
        assert got[:nt].tobytes() == want, first_diff(got[:nt], want)
        gap = got[nt: pad64(nt)]
        assert bool(((gap == FILL) | (gap == 0)).all())
        assert bool((got[pad64(nt):] == FILL).all()), "a byte at or above roundup64(new_len) was touched"

    def untouched(self):
        return bool((self.out == FILL).all()) and bool((self.table == FILL).all())

    def export(self, ctx, n):
        """The new table's live pairs in file order, through a DeviceIndex over it."""
        idx = S.DeviceIndex(0, 0, 0, ctx)
        idx.table, idx.nbytes, idx.n, idx._used, idx._live = self.table, self.tbytes, n, n, None
        k, p = idx.export()
        return [int(x) for x in k.cpu().numpy().view(np.uint64)], [int(x) for x in p.cpu().numpy().view(np.uint64)]


def check_compacted(ctx, st, f: bytes):
    """The low-level call on session `st` (whose bytes are f) against the host model; returns (Raw, model bytes, its)."""
    want, its = model_compact(f, len(f))
    before = source_state(st)
    r = Raw(ctx, st, len(its), len(want))
    assert r.rc == 0, r.msg
    s = r.stats
    assert (int(s.n_entries), int(s.new_len), int(s.kept_bytes)) == (len(its), len(want), sum(e - a + 20 for a, e, _, _ in its))
    r.check_bytes(want)
    assert source_state(st) == before  # the source store and the old table are only read
    return r, want, its


def check_new_table(ctx, r, want: bytes, n):
    keys, packed = r.export(ctx, n)
    ok, op = O.key_indexer_arrays(np.frombuffer(want, np.uint8), len(want))
    pairs = sorted(zip((int(x) for x in ok), (int(x) for x in op)), key=lambda kp: kp[1] & MASK48)
    assert set(zip(keys, packed)) == set(pairs) and len(keys) == n
    assert list(zip(keys, packed)) == pairs  # ... and in file order


# -- 1. bytes, stats and table ------------------------------------------------------------

def build_store(seed, n_keys=300, rounds=4):
    """Round 0 writes every key, the later rounds overwrite or tombstone half of them."""
    rng = random.Random(seed)
    buf, tail, live = bytearray(), 0, {}
    keys = [b"k%d" % i for i in range(n_keys)]
    for rnd in range(rounds):
        batch = []
        for k in (keys if rnd == 0 else rng.sample(keys, n_keys // 2)):
            if rnd and rng.random() < 0.1:
                batch.append((kh(k), b"\x00"))
                live.pop(k, None)
            else:
                live[k] = nonzero_bytes(rng, rng.choice(LENGTHS))
                batch.append((kh(k), live[k]))
        tail = O.write_entries(buf, tail, batch, allow_null=True)
    return bytes(buf), live


@pytest.fixture(scope="module")
def big(ctx):
    """The oracle-built store opened as a session, then 20 overwrites, 10 deletes and 3 renames in session:
    (session, its bytes, the model)."""
    rng = random.Random(0xC0FFEE)
    f0, live = build_store(0xC0A1)
    st = open_store(ctx, f0, room=4 << 20)
    m = Model(f0, live)
    names = sorted(live)
    over = [(k, nonzero_bytes(rng, rng.choice(LENGTHS[:19]))) for k in names[:20]]
    assert st.batch_write([k for k, _ in over], [p for _, p in over]) == m.write(over)
    assert st.batch_delete(names[20:30]) == m.delete(names[20:30])
    olds, news = names[30:33], [b"renamed-%d" % i for i in range(3)]
    m.write([(n, m.live[o]) for o, n in zip(olds, news)])  # (batch_rename appends all three, then deletes all three)
    assert st.batch_rename(olds, news) == m.delete(olds)
    f = st.bytes()
    assert f == bytes(m.buf)
    return st, f, m


def test_bytes_stats_and_table(ctx, big):
    st, f, m = big
    r, want, its = check_compacted(ctx, st, f)
    assert len(its) == len(m.live) > 256  # crosses the finish step's wave and block
    assert int(r.stats.n_crc_bad) == 0 and int(r.stats.first_bad) == NONE
    # the one-shot compaction over the export writes the same bytes
    _k, p = st.index.export()
    one = S.compact_device(st.buf.data_ptr(), st.tail, p.data_ptr(), p.numel(), ctx).cpu().numpy().tobytes()
    assert one == want
    check_new_table(ctx, r, want, len(its))
    assert O.recover_valid_chain(np.frombuffer(want, np.uint8)) == len(want)


def test_savings_and_iter_entries(ctx, big):
    st, f, _m = big
    its = entry_iterator(f, len(f))
    assert st.estimate_compaction_savings() == len(f) - sum(e - s + 20 for s, e, _, _ in its) > 0
    got = st.iter_entries()
    assert [tuple(int(x) for x in t) for t in zip(*got)] == its


# -- 2. every length alone ------------------------------------------------------------------

@pytest.mark.parametrize("long_live", [True, False])
@pytest.mark.parametrize("n", LENGTHS)
def test_every_length_alone(ctx, n, long_live):
    """Two entries under one key, of length n and of length 7: only the later one is kept."""
    rng = random.Random(n)
    pays = [nonzero_bytes(rng, 7), nonzero_bytes(rng, n)]
    if not long_live:
        pays.reverse()
    buf = bytearray()
    O.write_entries(buf, 0, [(kh(b"key"), pays[0])])
    O.write_entries(buf, len(buf), [(kh(b"key"), pays[1])])
    st = open_store(ctx, bytes(buf))
    r, want, its = check_compacted(ctx, st, bytes(buf))
    assert len(its) == 1 and want[: len(pays[1])] == pays[1] and len(want) == len(pays[1]) + 20
    assert int(r.stats.n_crc_bad) == 0
    check_new_table(ctx, r, want, 1)


# -- 3. the session goes on ------------------------------------------------------------------

def small_session(ctx, seed, capacity=4 << 20):
    rng = random.Random(seed)
    st, m = S.DeviceStore.create(capacity, ctx), Model()
    keys = [b"s-%d" % i for i in range(24)]
    # (keys[0], the newest live entry once renamed, and keys[1], the oldest, pad alike: 1 and 65 bytes.  Compaction
    # writes newest first, so a second one reverses the order, and the length is the slots' sum less the LAST
    # slot's padding: the two lengths agree exactly when the first and the last entry pad alike.)
    lens = [1, 65, 4097, CH + 1, 2 * CH + 17] + [40 + 3 * i for i in range(19)]
    pairs = [(k, nonzero_bytes(rng, n)) for k, n in zip(keys, lens)]
    assert st.batch_write([k for k, _ in pairs], [p for _, p in pairs]) == m.write(pairs)
    over = [(k, nonzero_bytes(rng, 300)) for k in keys[3:9]]
    assert st.batch_write([k for k, _ in over], [p for _, p in over]) == m.write(over)
    assert st.batch_delete(keys[10:14]) == m.delete(keys[10:14])
    m.write([(b"moved", m.live[keys[0]])])
    assert st.rename(keys[0], b"moved") == m.delete([keys[0]])
    return st, m, keys, rng


def reads_match(st, m, probe):
    g = st.batch_gather(probe)
    assert g.payloads() == [m.live.get(k) for k in probe]
    assert g.is_valid_checksum() == [True if k in m.live else None for k in probe]


def test_session_goes_on(ctx):
    import torch
    st, m, keys, rng = small_session(ctx, 3)
    probe = keys + [b"moved", b"absent"]
    stats = st.compact()
    assert st.tail == int(stats.new_len) == m.compact() and st.len() == len(m.live) == int(stats.n_entries)
    assert st.bytes() == bytes(m.buf)
    reads_match(st, m, probe)  # deleted and renamed-away keys read None
    k, p = st.index.export()
    exp = dict(zip((int(x) for x in k.cpu().numpy().view(np.uint64)), (int(x) for x in p.cpu().numpy().view(np.uint64))))
    assert exp == O.key_indexer_build(np.frombuffer(bytes(m.buf), np.uint8), m.tail)
    assert st.index.used == len(m.live)  # no deleted slot came over
    # a second compaction right behind the first: the same length, the same live payloads
    again = st.compact()
    assert int(again.new_len) == m.compact() and st.bytes() == bytes(m.buf)
    assert int(again.new_len) == int(stats.new_len) and int(again.n_entries) == int(stats.n_entries)
    reads_match(st, m, probe)
    # ... and the session goes on: host write, device write, delete, rename
    new = [(b"n-%d" % i, nonzero_bytes(rng, 500 + i)) for i in range(3)] + [(keys[5], nonzero_bytes(rng, 9000))]
    assert st.batch_write([k for k, _ in new], [p for _, p in new]) == m.write(new)
    dpay = [nonzero_bytes(rng, CH + 5), nonzero_bytes(rng, 33)]
    blob = torch.frombuffer(bytearray(dpay[0] + bytes(11) + dpay[1]), dtype=torch.uint8).cuda()
    dkeys = [b"d-0", keys[6]]
    assert st.batch_write_device(dkeys, blob, [0, len(dpay[0]) + 11], [len(p) for p in dpay]) == m.write(list(zip(dkeys, dpay)))
    gone = [keys[7], b"n-1"]
    assert st.batch_delete(gone) == m.delete(gone)
    m.write([(b"moved-again", m.live[b"moved"])])
    assert st.rename(b"moved", b"moved-again") == m.delete([b"moved"])
    gone.append(b"moved")
    f = st.bytes()
    assert f == bytes(m.buf) and O.recover_valid_chain(np.frombuffer(f, np.uint8)) == st.tail == m.tail
    reads_match(st, m, probe + [k for k, _ in new] + dkeys + [b"moved-again"])
    # the index: KeyIndexer::build of the bytes, less the keys whose latest entry is a tombstone -- exactly the
    # keys deleted since the compaction (reindex removes them, data_store.rs:224-259)
    built = O.key_indexer_build(np.frombuffer(f, np.uint8), st.tail)
    tombs = {h for h, v in built.items() if f[(v & MASK48) - 1: v & MASK48] == b"\x00" and
             int.from_bytes(f[(v & MASK48) + 8: (v & MASK48) + 16], "little") == (v & MASK48) - 1}
    assert tombs == {kh(k) for k in gone}
    k, p = st.index.export()
    exp = dict(zip((int(x) for x in k.cpu().numpy().view(np.uint64)), (int(x) for x in p.cpu().numpy().view(np.uint64))))
    assert exp == {h: v for h, v in built.items() if h not in tombs} and st.len() == len(m.live)


# -- 4. room is made ----------------------------------------------------------------------------

def test_room_is_made(ctx):
    rng = random.Random(4)
    keys = [b"r-%d" % i for i in range(8)]
    batch_bytes = 8 * pad64(1000 + 20)
    cap = 3 * batch_bytes
    st, m = S.DeviceStore.create(cap, ctx), Model()
    for _ in range(3):
        pairs = [(k, nonzero_bytes(rng, 1000)) for k in keys]
        assert st.batch_write(keys, [p for _, p in pairs]) == m.write(pairs)
    pairs = [(k, nonzero_bytes(rng, 1000)) for k in keys]
    buf_before, tail = st.buf.data_ptr(), st.tail
    with pytest.raises(ValueError, match="beyond the store's capacity"):
        st.batch_write(keys, [p for _, p in pairs])
    assert (st.buf.data_ptr(), st.tail) == (buf_before, tail)
    assert st.estimate_compaction_savings() == tail - 8 * 1020
    stats = st.compact()
    assert int(stats.new_len) == m.compact() == st.tail and int(stats.n_entries) == 8
    assert st.buf.numel() == S.padded_size(cap)  # the capacity is kept
    assert st.batch_write(keys, [p for _, p in pairs]) == m.write(pairs)  # ... and the same call succeeds
    assert st.bytes() == bytes(m.buf)
    # the live data itself outgrows the buffer: reserve
    big = [(b"big-%d" % i, nonzero_bytes(rng, 4000)) for i in range(8)]
    with pytest.raises(ValueError, match="beyond the store's capacity"):
        st.batch_write([k for k, _ in big], [p for _, p in big])
    with pytest.raises(ValueError, match="below the tail"):
        st.reserve(st.tail - 1)
    before = st.bytes()
    st.reserve(2 * cap)
    assert st.buf.numel() == S.padded_size(2 * cap) and st.tail == m.tail and st.bytes() == before
    reads_match(st, m, keys + [b"absent"])
    assert st.batch_write([k for k, _ in big], [p for _, p in big]) == m.write(big)
    assert st.bytes() == bytes(m.buf)
    reads_match(st, m, keys + [k for k, _ in big])


# -- 5. corruption is reported, not blessed silently ----------------------------------------------

def flip_session(ctx):
    """Six keys, two of them overwritten: (session, model, its tuples newest first, a superseded payload's offset)."""
    rng = random.Random(5)
    st, m = S.DeviceStore.create(1 << 20, ctx), Model()
    keys = [b"c-%d" % i for i in range(6)]
    pairs = [(k, nonzero_bytes(rng, n)) for k, n in zip(keys, [100, CH + 9, 64, 4097, 33, 2 * CH + 1])]
    assert st.batch_write(keys, [p for _, p in pairs]) == m.write(pairs)
    over = [(keys[0], nonzero_bytes(rng, 77)), (keys[3], nonzero_bytes(rng, 5000))]
    assert st.batch_write([k for k, _ in over], [p for _, p in over]) == m.write(over)
    its = entry_iterator(bytes(m.buf), m.tail)
    assert len(its) == 6
    return st, m, its, 0  # (offset 0: the first, superseded, version of c-0)


def test_corruption_is_reported(ctx):
    st, m, its, dead_off = flip_session(ctx)
    probe = [b"c-%d" % i for i in range(6)]
    # one bit of a live multi-chunk payload, flipped by torch with no host wait: the stream rule orders it
    victim = next(t for t in its if t[1] - t[0] == CH + 9)
    st.buf[victim[0] + CH + 3] ^= 0x10
    flipped = bytearray(m.buf)
    flipped[victim[0] + CH + 3] ^= 0x10
    want, _ = model_compact(bytes(flipped), m.tail)  # (the checksum is recomputed: the model's bytes over the flipped store)
    r = Raw(ctx, st, 6, len(want))
    assert r.rc == 0, r.msg
    assert int(r.stats.n_crc_bad) == 1 and int(r.stats.first_bad) == victim[2]
    r.check_bytes(want)
    check_new_table(ctx, r, want, 6)
    # the session refuses, and is exactly as it was
    state = (st.buf.data_ptr(), st.tail, st.index.table.data_ptr(), source_state(st))
    with pytest.raises(ValueError, match=r"n_crc_bad = 1, first_bad = %d\b" % victim[2]):
        st.compact()
    assert (st.buf.data_ptr(), st.tail, st.index.table.data_ptr(), source_state(st)) == state
    assert st.len() == 6 and st.bytes() == bytes(flipped)
    g = st.batch_gather(probe)
    assert g.payloads() == [bytes(flipped[s:e]) for k in probe for s, e, _, h in its if h == kh(k)]
    assert g.is_valid_checksum().count(False) == 1
    # ... unless told to keep it: the entry is copied faithfully under a fresh checksum
    stats = st.compact(allow_bad_crc=True)
    assert int(stats.n_crc_bad) == 1 and st.bytes() == want and st.tail == len(want)
    assert st.verify(probe) == [True] * 6


def test_corruption_of_dead_and_of_two_live_entries(ctx):
    st, m, its, dead_off = flip_session(ctx)
    st.buf[dead_off + 5] ^= 1  # a superseded entry: not copied, not counted
    r = Raw(ctx, st, 6, len(model_compact(bytes(m.buf), m.tail)[0]))
    assert r.rc == 0 and int(r.stats.n_crc_bad) == 0 and int(r.stats.first_bad) == NONE
    r.check_bytes(model_compact(bytes(m.buf), m.tail)[0])
    # two live entries: first_bad is the newer one's offset, it comes first in output order
    a, b = its[1], its[4]
    flipped = bytearray(m.buf)
    for t in (a, b):
        st.buf[t[1] - 1] ^= 0x80
        flipped[t[1] - 1] ^= 0x80
    want, _ = model_compact(bytes(flipped), m.tail)
    r = Raw(ctx, st, 6, len(want))
    assert r.rc == 0 and int(r.stats.n_crc_bad) == 2 and int(r.stats.first_bad) == a[2] > b[2]
    r.check_bytes(want)


# -- 6. refusals ------------------------------------------------------------------------------------

REFUSALS = ["out_cap_one_short", "table_16_short", "d_out_inside_store", "d_out_misaligned"]


@pytest.mark.parametrize("case", REFUSALS)
def test_refusals_write_nothing(ctx, case):
    st, m, _keys, _rng = small_session(ctx, 6)
    want, its = model_compact(bytes(m.buf), m.tail)
    n, nl = len(its), len(want)
    before = source_state(st)
    import torch
    spare = torch.full((S.padded_size(nl) + 64,), FILL, dtype=torch.uint8, device="cuda")
    kw, known = {}, True
    if case == "out_cap_one_short":
        kw = {"out_cap": S.padded_size(nl) - 1}
    elif case == "table_16_short":
        kw = {"table_bytes": int(S.lib().srd_index_table_bytes(n)) - 16}
    elif case == "d_out_inside_store":  # the last 64 bytes of the store's padded range
        kw, known = {"d_out": st.buf.data_ptr() + S.padded_size(st.tail) - 64, "out_cap": 1 << 20}, False
    elif case == "d_out_misaligned":
        kw, known = {"d_out": spare.data_ptr() + 8}, False
    r = Raw(ctx, st, n, nl, **kw)
    assert r.rc == S.SRD_ERR_ARG and r.msg, (r.rc, r.msg)
    assert r.untouched() and bool((spare == FILL).all()) and source_state(st) == before
    # new_len and n_entries are reported where they are known: the argument checks come before anything runs
    assert (int(r.stats.new_len), int(r.stats.n_entries)) == ((nl, n) if known else (0, 0))
    assert int(r.stats.n_crc_bad) == 0 and int(r.stats.first_bad) == NONE
    if known:  # ... and with the missing bytes the call succeeds
        ok = Raw(ctx, st, n, nl)
        assert ok.rc == 0, ok.msg
        ok.check_bytes(want)


def test_null_only_payload_fails_the_session_call(ctx):
    st, m, keys, _rng = small_session(ctx, 7)
    pairs = [(b"zeros", b"\x00\x00\x00")]
    assert st.batch_write([b"zeros"], [b"\x00\x00\x00"]) == m.write(pairs)
    state = (st.buf.data_ptr(), st.tail, st.index.table.data_ptr(), source_state(st))
    with pytest.raises(S.SrdError, match="NULL-byte-only streams cannot be written directly."):
        st.compact()
    assert (st.buf.data_ptr(), st.tail, st.index.table.data_ptr(), source_state(st)) == state
    assert st.len() == len(m.live) and st.bytes() == bytes(m.buf)
    assert st.batch_read([b"zeros", keys[1]]) == [b"\x00\x00\x00", m.live[keys[1]]]


# -- 7. edges -------------------------------------------------------------------------------------------

def test_empty_and_all_deleted_sessions(ctx):
    st = S.DeviceStore.create(1 << 16, ctx)
    s = st.compact()
    assert (int(s.n_entries), int(s.new_len), int(s.kept_bytes), int(s.n_crc_bad)) == (0, 0, 0, 0)
    assert st.tail == 0 and st.len() == 0 and st.estimate_compaction_savings() == 0
    m = Model()
    pairs = [(b"a", b"alpha"), (b"b", b"beta" * 300)]
    assert st.batch_write([k for k, _ in pairs], [p for _, p in pairs]) == m.write(pairs)
    assert st.bytes() == bytes(m.buf) and st.batch_read([b"a", b"b"]) == [p for _, p in pairs]
    # every key deleted: the same
    assert st.batch_delete([b"a", b"b"]) == m.delete([b"a", b"b"])
    assert st.estimate_compaction_savings() == st.tail > 0
    s = st.compact()
    assert (int(s.n_entries), int(s.new_len), st.tail, st.len()) == (0, 0, 0, 0)
    assert st.iter_entries()[0].size == 0
    m = Model()
    assert st.batch_write([b"c"], [b"gamma"]) == m.write([(b"c", b"gamma")])
    assert st.bytes() == bytes(m.buf) and st.read(b"c") == b"gamma" and st.read(b"a") is None


def test_keys_indexed_at_a_tombstone_disappear(ctx):
    """A store whose latest entry for 5 keys is a tombstone: open's index holds them (KeyIndexer::build
    includes tombstones), the compacted store's does not."""
    rng = random.Random(8)
    keys = [b"t-%d" % i for i in range(12)]
    buf = bytearray()
    tail = O.write_entries(buf, 0, [(kh(k), nonzero_bytes(rng, 50 + i)) for i, k in enumerate(keys)])
    tail = O.write_entries(buf, tail, [(kh(k), b"\x00") for k in keys[:5]], allow_null=True)
    f = bytes(buf)
    st = open_store(ctx, f)
    assert st.len() == 12
    r, want, its = check_compacted(ctx, st, f)
    assert len(its) == 7
    check_new_table(ctx, r, want, 7)
    s = st.compact()
    assert int(s.n_entries) == 7 and st.len() == 7 and st.bytes() == want
    assert st.batch_read(keys) == [None] * 5 + [f[a:e] for a, e, _, _ in sorted(its, key=lambda t: t[0])]
