"""Random sessions over every DeviceStore operation against the host model of
tests/test_session_model.py: two sessions on two
contexts of device 0, each step run on the device and on the model, every
comparison bit-exact against the oracle, zlib.crc32 or the model.

A failing step names its seed, its number, the operation and its arguments;
replay(seed, upto) rebuilds both sessions (and the models) to that step:

    import test_gpu_session_fuzz as F
    s = F.replay(0x5E551, 57)      # the state before step 57
    s.step(57)                     # ... and the step itself, with every check
"""
import hashlib
import random
import zlib

import numpy as np
import pytest

import oracle as O
import srd_amd as S
import test_gpu_compact_live as L
import test_gpu_rows as R
import test_gpu_ttl as T
import test_session_model as M

pytestmark = pytest.mark.gpu

CH = S.GATHER_CHUNK
FILL = 0xA5
ROW_CAP = CH + 16  # the longest payload of the schedule (2 * CH + 17) does not fit a row


def dev_bytes(b: bytes):
    import torch
    if not b:
        return torch.empty(0, dtype=torch.uint8, device="cuda")
    return torch.from_numpy(np.frombuffer(b, np.uint8).copy()).cuda()


def dev_u64(a):
    import torch
    return torch.from_numpy(np.array(a, np.uint64).view(np.int64).copy()).cuda()


def sha(t):
    return hashlib.sha256(t.cpu().numpy().tobytes()).hexdigest()


def snapshot(st):
    """What a refusal must leave as it was: the buffer, the tail, the whole table and the bytes."""
    st.sync()
    return st.buf.data_ptr(), st.tail, st.index.table.data_ptr(), sha(st.index.table), st.bytes()


def table_state(st):
    return st.index.used, st.len(), st.index.capacity


def odd_pieces(n):
    """Destinations of n bytes in all: odd-sized pieces filled with 0xA5."""
    import torch
    sizes, left = [], n
    for s in (1, 7, 33, 4097):
        if left > s:
            sizes.append(s)
            left -= s
    sizes.append(left)
    return [torch.full((s,), FILL, dtype=torch.uint8, device="cuda") for s in sizes]


# -- one operation of a schedule on the device ------------------------------------------------------

def segments(st, pieces):
    return [st.buf[p[1]: p[2]] if p[0] == "s" else dev_bytes(p[1]) for p in pieces]


def host_bytes(pieces):
    """A payload for the paths that take host bytes (the schedule cuts only the stream paths' payloads)."""
    assert all(p[0] == "b" for p in pieces)
    return b"".join(p[1] for p in pieces)


def device_step(sts, op, a):
    """Operation (op, a) on the sessions: what the call returns, in the model's terms."""
    st = sts[a["store"]]
    if op == "write":
        keys = [M.read_key(k) for k in a["keys"]]
        hashes = [O.xxh3_64(k) for k in keys]
        path, dev = a["path"], a["dev"]
        if path.startswith("stream"):
            ents = [segments(st, p) for p in a["payloads"]]
            if path == "stream_keys":
                return st.batch_write_stream(keys, ents)
            return st.batch_write_stream_with_key_hashes(dev_u64(hashes) if dev else hashes, ents)
        pays = [host_bytes(p) for p in a["payloads"]]
        if path == "host_keys":
            return st.batch_write(keys, pays)
        if path == "host_hashes":
            return st.batch_write_with_key_hashes(hashes, pays)
        offs, blob = [], b"\xEE" * 5  # the payloads in one blob, 11 bytes between them
        for p in pays:
            offs.append(len(blob))
            blob += p + b"\xEE" * 11
        lens = [len(p) for p in pays]
        offs, lens = (dev_u64(offs), dev_u64(lens)) if dev else (offs, lens)
        if path == "dev_keys":
            return st.batch_write_device(keys, dev_bytes(blob), offs, lens)
        return st.batch_write_device_with_key_hashes(dev_u64(hashes) if dev else hashes, dev_bytes(blob), offs, lens)
    if op == "write_ttl":
        if a["path"] == "stream":
            return st.batch_write_stream_with_ttl(a["names"], [segments(st, p) for p in a["values"]], a["ttls"],
                                                  now=a["now"])
        vals = [host_bytes(p) for p in a["values"]]
        return st.batch_write_with_ttl(a["names"], vals, a["ttls"], now=a["now"])
    if op == "delete":
        keys = [M.read_key(k) for k in a["keys"]]
        if a["by"] == "keys":
            return st.batch_delete(keys)
        hashes = [O.xxh3_64(k) for k in keys]
        return st.batch_delete_key_hashes(dev_u64(hashes) if a["dev"] else hashes)
    if op == "rename":
        return st.batch_rename([M.read_key(k) for k in a["olds"]], [M.read_key(k) for k in a["news"]])
    if op == "copy":
        return st.batch_copy([M.read_key(k) for k in a["keys"]], sts[a["target"]])
    if op == "transfer":
        return st.batch_transfer([M.read_key(k) for k in a["keys"]], sts[a["target"]])
    if op == "read_ttl":
        r = st.batch_read_with_ttl(a["names"], now=a["now"], evict=a["evict"])
        assert r.is_valid_checksum() == [True if s == S.TTL_LIVE else None for s in r.status]
        return [int(s) for s in r.status], r.values(), [int(e) for e in r.expiry], r.n_evicted
    if op == "sweep":
        s = st.sweep_expired(now=a["now"], plan=a["plan"])
        return int(s.n_judged), int(s.n_expired), int(s.n_short), int(s.next_expiry)
    if op == "compact":
        s = st.compact(a["capacity"])
        assert int(s.n_crc_bad) == 0 and int(s.first_bad) == L.NONE
        return int(s.n_entries), int(s.new_len), int(s.kept_bytes)
    if op == "reserve":
        return st.reserve(a["capacity"])
    raise AssertionError(op)


# -- the read paths against a {hash: payload} picture of the store -------------------------------------

def check_reads(st, keys, live, bad=()):
    """Every read path over the probe `keys` against live = {hash: payload as the store holds it}; the hashes in
    `bad` hold bytes that fail their stored checksum: delivered as they are, reported BAD_CRC or False."""
    hashes = [O.xxh3_64(k) for k in keys]
    want = [live.get(h) for h in hashes]
    verdict = [None if p is None else h not in bad for h, p in zip(hashes, want)]
    status = [S.GATHER_NONE if v is None else S.GATHER_OK if v else S.GATHER_BAD_CRC for v in verdict]
    crcs = [zlib.crc32(p) if p is not None else 0 for p in want]
    assert st.batch_read(keys) == want
    g = st.batch_gather(keys)
    assert g.payloads() == want and [int(s) for s in g.status] == status and g.is_valid_checksum() == verdict
    assert [int(c) for c, p in zip(g.crc_computed, want) if p is not None] == [c for c, p in zip(crcs, want) if p is not None]
    # into the caller's tensors: odd-sized pieces for a hit, three bytes that stay as they were for a miss
    ents = [odd_pieces(len(p)) if p is not None else odd_pieces(3) for p in want]
    sc = st.batch_read_into(keys, ents)
    assert [int(s) for s in sc.status] == [s if p is not None else S.GATHER_NONE for s, p in zip(status, want)]
    assert [int(c) for c in sc.crc_computed] == crcs
    for p, e in zip(want, ents):
        assert b"".join(t.cpu().numpy().tobytes() for t in e) == (p if p is not None else bytes([FILL]) * 3)
    # into rows, every output sentinel-filled and checked whole
    rows = [R.want_of(p, ROW_CAP, bad=h in bad) for h, p in zip(hashes, want)]
    o = R.Outs(len(keys), ROW_CAP, ROW_CAP + 16)
    d_h = dev_u64(hashes)
    st.batch_read_rows_hashed_keys(d_h, o.out, d_h, **o.kw())
    o.check(rows)
    o2 = R.Outs(len(keys), ROW_CAP, ROW_CAP)
    r = st.batch_read_rows(keys, o2.out)
    assert r.payloads() == [w[3] for w in rows] and [int(s) for s in r.status.cpu().numpy()] == [w[0] for w in rows]
    assert [int(c) for c in r.crc.cpu().numpy().view(np.uint32)] == [w[2] for w in rows]
    img = np.full((len(keys), ROW_CAP), FILL, np.uint8)
    for i, w in enumerate(rows):
        if w[3] is not None:
            img[i, : w[1]] = np.frombuffer(w[3], np.uint8)
    assert np.array_equal(o2.base.cpu().numpy(), img)
    assert st.verify(keys) == verdict
    assert [st.exists(k) for k in keys] == [p is not None for p in want]


def check_iter_gather(st, f: bytes, tail: int, bad=()):
    its = L.entry_iterator(f, tail)
    g = st.iter_gather()
    assert g.payloads() == [f[s:e] for s, e, _, _ in its]
    assert [int(s) for s in g.status] == [S.GATHER_BAD_CRC if k in bad else S.GATHER_OK for _, _, _, k in its]
    assert [int(c) for c in g.crc_computed] == [zlib.crc32(f[s:e]) for s, e, _, _ in its]


def reopened(ctx, st, tail):
    """A clone of buf[:padded_size(tail)] validated and re-opened on another context: (n_crc_bad, the session)."""
    st.sync()
    clone = st.buf[: S.padded_size(tail)].clone()
    S._after_torch(ctx, clone.device)
    r = S.validate_index_device(clone.data_ptr(), tail, 0, ctx)
    assert int(r.final_len) == tail
    st3 = S.DeviceStore.open(clone, tail, ctx)
    assert st3.tail == tail
    return int(r.n_crc_bad), st3


class Session:
    """Two sessions on two contexts, their models, a third context for re-opening, and the key each hash reads by."""

    def __init__(self, seed, n_steps):
        self.seed, self.ops = seed, M.schedule(seed, n_steps)
        self.ctxs = [S.Context(0) for _ in range(3)]
        self.sts = [S.DeviceStore.create(c, x) for c, x in zip((M.CAP0, M.CAP1), self.ctxs)]
        self.ms = [M.SessionModel(M.CAP0), M.SessionModel(M.CAP1)]
        self.keys = {}  # hash -> the key it is read by
        self.table_changes = self.revivals = 0

    def close(self):
        self.sts = None
        for c in self.ctxs:
            c.close()

    def step(self, i, check=True):
        op, a = self.ops[i]
        try:
            self._step(i, op, a, check)
        except Exception as e:
            raise AssertionError(f"seed {self.seed:#x} step {i}: {M.describe(op, a)}: {type(e).__name__}: {e}") from e

    def _step(self, i, op, a, check):
        sts, ms = self.sts, self.ms
        for k in M.op_keys(op, a):
            self.keys[M.hash_of(k)] = M.read_key(k)
        touched = sorted({a["store"], a.get("target", a["store"])})
        table = table_state(sts[0]) if check else None  # (an unchecked step asks the device nothing of its own)
        want = M.outcome(lambda: M.model_step(ms, op, a))
        snaps = [snapshot(sts[j]) for j in touched] if want[0] == "err" and check else None
        got = M.outcome(lambda: device_step(sts, op, a))
        if want[0] == "err":
            assert got[0] == "err" and type(got[1]) is type(want[1]) and str(want[1]) in str(got[1]), (got, want)
            if check:  # a refusal leaves the session as it was
                assert [snapshot(sts[j]) for j in touched] == snaps
        else:
            assert got == want, (got, want)
        if not check:
            return
        after = table_state(sts[0])
        grown = after[2] != table[2]
        self.table_changes += grown
        self.revivals += op in ("write", "write_ttl") and a["store"] == 0 and M.is_revival(table, after)
        for st, m in zip(sts, ms):
            assert st.tail == m.tail
            assert st.len() == len(st.index) == len(m.live)
            assert st.bytes() == bytes(m.buf)
            assert st.index.used <= st.index.capacity // 2 and st.index.used >= st.len()
            assert (st.index.used, st.index.capacity) == (len(m.slots), m.tcap)  # srd_table.h's rules, restated
        full = op in ("compact", "reserve", "sweep") or (op == "read_ttl" and a["evict"]) or grown
        for j in range(2):
            if i % 8 == 7 or (full and j in touched):
                self.full_check(j, i)

    def probe(self, j, i):
        """Live keys (the long payloads among them), deleted keys, never-written keys and a duplicate."""
        m, rng = self.ms[j], random.Random(self.seed * 1000 + i)
        live = sorted(m.live)
        long_ones = [h for h in live if len(m.live[h]) > 4096][:3]
        hs = rng.sample(live, min(len(live), 10)) + long_ones + rng.sample(sorted(m.tombs), min(len(m.tombs), 3))
        keys = [self.keys[h] for h in hs] + [b"never-written-%d" % i, b""]
        keys.append(rng.choice(keys))
        rng.shuffle(keys)
        return keys

    def full_check(self, j, i):
        st, m = self.sts[j], self.ms[j]
        f = bytes(m.buf)
        check_reads(st, self.probe(j, i), m.live)
        check_iter_gather(st, f, m.tail)
        # the table: KeyIndexer::build of the bytes less the tombstoned hashes, in file order
        built = O.key_indexer_build(np.frombuffer(f, np.uint8), m.tail) if f else {}
        tombs = M.tomb_hashes(f, built)
        pairs = sorted(((h, v) for h, v in built.items() if h not in tombs), key=lambda kv: kv[1] & M.MASK48)
        k, p = st.index.export()
        assert list(zip((int(x) for x in k.cpu().numpy().view(np.uint64)),
                        (int(x) for x in p.cpu().numpy().view(np.uint64)))) == pairs
        q = [h for h, _ in pairs] + sorted(tombs)
        if q:
            assert [int(x) for x in st.index.get_packed(np.array(q, np.uint64))] == \
                [v for _, v in pairs] + [S.INDEX_NONE] * len(tombs)
        st.index._live = None
        assert st.len() == len(m.live)  # counted from the table
        if m.tail:
            n_bad, st3 = reopened(self.ctxs[2], st, m.tail)
            assert n_bad == 0
            assert {int(x) for x in st3.iter_entries()[3]} == set(m.live)


def replay(seed, upto, n_steps=M.N_STEPS):
    """Both sessions and their models as they are before step `upto` of seed's schedule."""
    s = Session(seed, max(n_steps, upto + 1))
    for i in range(upto):
        s.step(i, check=False)
    return s


# -- the tests ---------------------------------------------------------------------------------------

@pytest.mark.parametrize("seed", M.SEEDS)
def test_random_session(seed):
    s = Session(seed, M.N_STEPS)
    try:
        for i in range(M.N_STEPS):
            s.step(i)
        assert s.table_changes >= 2, f"seed {seed:#x}: {s.table_changes} table capacity changes"
        assert s.revivals >= 1, f"seed {seed:#x}: no write revived a deleted slot"
    finally:
        s.close()


@pytest.mark.parametrize("seed", M.SEEDS)
def test_random_session_checked_every_twelfth_step(seed):
    """The same sessions with eleven steps in a row left to themselves: between two checked steps the test adds
    no host read of its own (no bytes(), len() or snapshot), so the families' stream rules meet each other
    across operations as a caller's would; every return value is still compared, and what the unchecked steps
    left behind is judged whole at the next checked one and at the end."""
    s = Session(seed, M.N_STEPS)
    try:
        for i in range(M.N_STEPS):
            s.step(i, check=i % 12 == 11)
        for j in range(2):
            try:
                s.full_check(j, M.N_STEPS)
            except Exception as e:
                raise AssertionError(f"seed {seed:#x} after {M.N_STEPS} steps, store {j}: {type(e).__name__}: {e}") from e
    finally:
        s.close()


def test_corruption_in_a_random_session():
    seed, n = M.CORRUPTION_SEED, M.CORRUPTION_STEPS
    s = Session(seed, n)
    try:
        for i in range(n):
            s.step(i)
        st, m, ctx3 = s.sts[0], s.ms[0], s.ctxs[2]
        (start, mo, victim), dead = M.corruption_victims(m)
        keys = [s.keys[victim]] + s.probe(0, n)
        # one bit of a live payload of more than one unit, flipped by torch with no host wait
        st.buf[start + CH] ^= 0x10
        flipped = bytearray(m.buf)
        flipped[start + CH] ^= 0x10
        live = dict(m.live)
        live[victim] = bytes(flipped[start:mo])
        check_reads(st, keys, live, bad={victim})
        check_iter_gather(st, bytes(flipped), m.tail, bad={victim})
        snap = snapshot(st)
        with pytest.raises(ValueError, match=r"n_crc_bad = 1, first_bad = %d\b" % mo):
            st.compact()
        assert snapshot(st) == snap and st.len() == len(m.live) and st.bytes() == bytes(flipped)
        assert reopened(ctx3, st, m.tail)[0] == 1
        # the bit flipped back, one bit of a superseded entry flipped instead: no read path sees it
        st.buf[start + CH] ^= 0x10
        st.buf[dead + 5] ^= 0x01
        check_reads(st, keys, m.live)
        check_iter_gather(st, bytes(m.buf), m.tail)
        tail = m.tail
        st.sync()
        clone = st.buf[: S.padded_size(tail)].clone()
        assert device_step(s.sts, "compact", {"store": 0, "capacity": None}) == m.compact()
        assert st.bytes() == bytes(m.buf) and st.len() == len(m.live)
        check_reads(st, keys, m.live)
        S._after_torch(ctx3, clone.device)
        r = S.validate_index_device(clone.data_ptr(), tail, 0, ctx3)
        assert int(r.final_len) == tail and int(r.n_crc_bad) == 1
    finally:
        s.close()


def test_captured_rows_read_survives_other_entries():
    """One captured rows read replayed between operations that each grow the context's workspace: the rows entry's
    workspace is its own, so the graph stays valid while rows_token() is unchanged."""
    import torch
    rng = random.Random(0xCA97)
    ctx = S.Context(0)
    try:
        cap = 4 << 20  # large enough that nothing below moves the buffer
        st, m = S.DeviceStore.create(cap, ctx), M.SessionModel(cap)
        n, keys_of = 65, {}

        def write(names, lens):
            pays = [L.nonzero_bytes(rng, x) for x in lens]
            for k in names:
                keys_of[O.xxh3_64(k)] = k
            assert st.batch_write(names, pays) == m.write([(O.xxh3_64(k), p) for k, p in zip(names, pays)], host=True)

        def write_ttl(names, now):
            vals = [L.nonzero_bytes(rng, 1 + i % 40) for i in range(len(names))]
            ttls = [M.TICK * (i % 7) for i in range(len(names))]
            for k in names:
                keys_of[T.ns_hash(k)] = T.ns_key(k)
            assert st.batch_write_with_ttl(names, vals, ttls, now=now) == m.write_ttl(names, vals, ttls, now, host=True)

        plain = [b"g%d" % i for i in range(80)]
        write(plain, [1, 17, 64, 100, 4095, 4096, 4097, CH, CH + 1, 2 * CH + 17] + [50 + i for i in range(70)])
        st.reserve_rows(n, ROW_CAP)
        st.index.grow(8192)
        ttl = [b"t%d" % i for i in range(3000)]
        for lo in range(0, 3000, 250):
            write_ttl(ttl[lo: lo + 250], M.NOW0)
        d_h = torch.zeros(n, dtype=torch.int64, device="cuda")
        o = R.Outs(n, ROW_CAP, ROW_CAP + 16)

        def capture():
            st.sync()
            g = torch.cuda.CUDAGraph()
            with torch.cuda.graph(g):
                st.batch_read_rows_hashed_keys(d_h, o.out, **o.kw())
            return g, st.rows_token()

        def replay_and_check(g, token):
            """Other keys in the same tensor, the outputs refilled, the replay checked whole against the model."""
            pool = sorted(m.live) + sorted(m.tombs)[:40]
            hs = rng.sample(pool, n - 3) + [O.xxh3_64(b"missing"), O.xxh3_64(b"g9")]
            hs.append(hs[0])
            d_h.copy_(dev_u64(hs))
            st.sync()
            o.refill()
            g.replay()
            o.check([R.want_of(m.live.get(h), ROW_CAP) for h in hs])
            assert st.rows_token() == token
            assert (st.tail, st.len()) == (m.tail, len(m.live))

        g, token = capture()
        replay_and_check(g, token)
        now = M.NOW0 + 3 * M.TICK

        def grows(call, model=lambda: None):
            """(what the call returns, what the model returns) of an operation that must grow the workspace."""
            before = ctx.device_bytes()
            out, want = call(), model()
            assert ctx.device_bytes() > before, "the operation fitted the workspace the context had"
            replay_and_check(g, token)
            return out, want

        # a gather of the 2 * CH + 17 payload: the first gather of this context
        got, _ = grows(lambda: st.batch_gather([b"g9", b"g8"]))
        assert got.payloads() == [m.live[O.xxh3_64(b"g9")], m.live[O.xxh3_64(b"g8")]]
        # an evicting read of several hundred keys, some of them twice
        q = ttl[:600] + ttl[:30]
        r, want = grows(lambda: st.batch_read_with_ttl(q, now=now), lambda: m.read_ttl([T.ns_hash(k) for k in q], now, True))
        assert ([int(x) for x in r.status], r.values(), [int(e) for e in r.expiry], r.n_evicted) == want
        assert want[3] > 200
        # an export of a few thousand pairs
        (k, _p), _ = grows(lambda: st.index.export())
        assert k.numel() == len(m.live)
        # a sweep over several thousand TTL entries
        sw, want = grows(lambda: st.sweep_expired(now=now + M.TICK), lambda: m.sweep(now + M.TICK))
        assert (int(sw.n_judged), int(sw.n_expired), int(sw.n_short), int(sw.next_expiry)) == want
        assert int(sw.n_judged) > 2000 and int(sw.n_expired) > 500
        assert st.bytes() == bytes(m.buf)
        # compaction moves the buffer and the table: a new capture
        cs = st.compact()
        assert (int(cs.n_entries), int(cs.new_len), int(cs.kept_bytes)) == m.compact()
        assert st.rows_token() != token and st.bytes() == bytes(m.buf)
        g2, token2 = capture()
        replay_and_check(g2, token2)
    finally:
        ctx.close()


def test_sweep_order_when_offset_order_is_not_write_order():
    ctx = S.Context(0)
    try:
        cap = 1 << 20
        st, m = S.DeviceStore.create(cap, ctx), M.SessionModel(cap)
        now = M.NOW0
        keys = [b"o-%d" % i for i in range(300)]

        def write(names, lens, ttls, now):
            vals = [bytes([1 + (i + x) % 255]) * x for i, x in enumerate(lens)]
            assert st.batch_write_with_ttl(names, vals, ttls, now=now) == m.write_ttl(names, vals, ttls, now, host=True)

        def sweep(now):
            before = len(m.live)
            s = st.sweep_expired(now=now)
            want = m.sweep(now)
            assert (int(s.n_judged), int(s.n_expired), int(s.n_short), int(s.next_expiry)) == want
            assert st.tail == m.tail and st.bytes() == bytes(m.buf)
            assert st.len() == len(m.live) == before - want[1]
            st.index._live = None
            assert st.len() == len(m.live)
            return want

        write(keys, [1 + i % 40 for i in range(300)], [M.TICK * (i % 6) for i in range(300)], now)
        # every third key again, with a later expiry and another length: their entries now lie behind the others'
        again = keys[::3]
        write(again, [50 + i % 30 for i in range(100)], [M.TICK * (1 + i % 5) for i in range(100)], now + M.TICK)
        gone = [T.ns_hash(k) for k in (keys[4], keys[9], keys[150], keys[299])]
        assert st.batch_delete_key_hashes(gone) == m.delete(gone)
        want = sweep(now + 3 * M.TICK)
        assert 100 < want[1] < 200  # about half
        offs = m.last_sweep  # ascending offset of the entries removed: not key order, not write order of the keys
        names = {T.ns_hash(k): i for i, k in enumerate(keys)}
        removed = [names[int.from_bytes(bytes(m.buf[t + 1: t + 9]), "little")]
                   for t in range(m.tail - 21 * want[1], m.tail, 21)]
        assert removed != sorted(removed) and len(offs) == want[1]
        # compaction puts the newest first: offset order is now the reverse of write order
        cs = st.compact()
        assert (int(cs.n_entries), int(cs.new_len), int(cs.kept_bytes)) == m.compact()
        assert st.bytes() == bytes(m.buf)
        more = [b"late-%d" % i for i in range(40)]
        write(more, [8 + i for i in range(40)], [M.TICK * (i % 4) for i in range(40)], now + 4 * M.TICK)
        want = sweep(now + 5 * M.TICK)
        assert want[1] >= 20
        assert [q for _, q in m.last_sweep] != sorted(q for _, q in m.last_sweep)
    finally:
        ctx.close()


def test_rename_and_transfer_are_refused_as_a_whole():
    """The tombstones of a rename or a transfer that would end beyond the capacity: refused before anything is
    appended or copied (both used to append or copy first and fail at the delete)."""
    ctx, ctx2 = S.Context(0), S.Context(0)
    try:
        st, other = S.DeviceStore.create(4096, ctx), S.DeviceStore.create(1 << 16, ctx2)
        pay = L.nonzero_bytes(random.Random(1), 2008)
        assert st.batch_write([b"a"], [pay]) == 2028  # the copy ends at 4076, its tombstone at 4097: one byte too far
        snap, snap2 = snapshot(st), snapshot(other)
        with pytest.raises(ValueError, match="beyond the store's capacity"):
            st.rename(b"a", b"b")
        assert snapshot(st) == snap and st.batch_read([b"a", b"b"]) == [pay, None] and st.len() == 1
        st.reserve(8192)
        assert st.rename(b"a", b"b") == 4097 and st.batch_read([b"a", b"b"]) == [None, pay]
        full = S.DeviceStore.create(4096, ctx)
        assert full.batch_write([b"k"], [pay + pay + bytes(40)]) == 4076
        snap = snapshot(full)
        with pytest.raises(ValueError, match="tombstones end beyond the store's capacity"):
            full.transfer(b"k", other)
        with pytest.raises(KeyError):  # the keys are resolved first: a missing key is reported as such
            full.transfer(b"missing", other)
        assert snapshot(full) == snap and snapshot(other) == snap2 and other.len() == 0
        assert full.copy(b"k", other) == 4076 and other.read(b"k") == pay + pay + bytes(40)
    finally:
        ctx.close()
        ctx2.close()


def test_rows_result_waits_for_a_read_on_the_default_stream():
    """A rows read issued on torch's default stream (handle 0: the library's "the context stream") while the
    context stream is still busy: RowsResult's host accessors, and torch work behind the read, see its results.
    (They used to wait for torch's stream alone, which such a read never ran on: test_random_session found the
    accessors reading statuses the kernels had not written yet.)"""
    import torch
    ctx = S.Context(0)
    try:
        ents = [(b"w%d" % i, L.nonzero_bytes(random.Random(i), 40 + i)) for i in range(64)]
        st = R.make_store(ctx, ents)
        d_h = dev_u64([O.xxh3_64(k) for k, _ in ents])
        o = R.Outs(64, 128, 128)
        busy = torch.empty(1 << 29, dtype=torch.uint8, device="cuda")
        torch.cuda.synchronize()
        assert torch.cuda.current_stream().cuda_stream == 0
        with torch.cuda.stream(torch.cuda.ExternalStream(ctx.stream)):
            for _ in range(16):  # some milliseconds of fills in front of the read: the host gets there first
                busy.fill_(1)
        r = st.batch_read_rows_hashed_keys(d_h, o.out, **o.kw())
        seen = o.status.clone()  # torch work ordered behind the read
        assert r.is_valid_checksum() == [True] * 64 and r.payloads() == [p for _, p in ents]
        assert [int(x) for x in seen.cpu().numpy()] == [S.GATHER_OK] * 64
        o.check([R.want_of(p, 128) for _, p in ents])
    finally:
        ctx.close()
