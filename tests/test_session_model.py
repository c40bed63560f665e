"""A host model of a live DeviceStore session and a deterministic schedule of
random operations over it.  No GPU call is made here:
the model is plain Python over the CPU oracle and the restatements the suite
already has, and tests/test_gpu_session_fuzz.py runs the same schedules on the
device against it.

SessionModel replays the reference's operation sequence: every write is one
O.write_entries at the tail (data_store.rs:847-939), a delete is one tombstone
per listed hash the index holds, duplicates included, in list order
(data_store.rs:995-1024), rename is write-then-delete (:941-958), compaction is
test_gpu_compact_live.model_compact (EntryIterator order, newest first), the
TTL payload and key are test_gpu_ttl's le64 / ns_hash.  The capacity rule is
the product's documented one: a batch is refused when padded_size(new_tail)
exceeds the buffer.  A refused operation leaves every field as it was.

The model also restates csrc/srd_table.h's slot rules (a slot never returns to
TBL_EMPTY, at most half of the slots are not empty, a full table is rebuilt at
twice the need, compaction builds a table of the live keys), so that the
coverage conditions on deleted-slot churn, table growth and revival can be
asserted here, before any GPU time is spent.

schedule(seed, n_steps) is a pure function of its arguments: random.Random(seed)
and the model's own state, no wall clock."""
import collections
import random

import numpy as np
import pytest

import oracle as O
import srd_amd as S
import test_gpu_compact_live as L  # entry_iterator, model_compact, nonzero_bytes
import test_gpu_ttl as T  # KEY_LENS, le64, ns_key, ns_hash

CH = S.GATHER_CHUNK
M64 = (1 << 64) - 1
MASK48 = (1 << 48) - 1
SEEDS = [0x5E551, 0x5E553, 0x5E557]  # the committed seeds: each meets every coverage condition below
N_STEPS = 120
CORRUPTION_SEED, CORRUPTION_STEPS = 0x5E554, 40
NOW0, TICK = 1_700_000_000, 10
CAP0, CAP1 = 192 << 10, 1 << 20  # the first store is small: capacity refusals occur on their own
SMALL, MID, BIG = [1, 7, 8, 9, 15, 16, 17, 63, 64, 65], [4095, 4096, 4097], [CH - 1, CH, CH + 1, 2 * CH + 17]
WRITE_PATHS = ["host_keys", "host_hashes", "dev_keys", "dev_hashes", "stream_keys", "stream_hashes"]
KINDS = ["write", "write_ttl", "delete", "rename", "copy", "transfer", "read_ttl", "sweep", "compact", "reserve"]
NULL_ONLY = "NULL-byte-only streams cannot be written directly."


def pad64(n):
    return (n + 63) & ~63


def tail_after(tail, lens):
    """The tail after entries of these payload lengths: each payload starts at the next 64-byte boundary and is
    followed by its 20 metadata bytes (data_store.rs:864-897)."""
    for n in lens:
        tail = pad64(tail) + n + 20
    return tail


def table_capacity(n):
    """srd_table.h: the power of two >= max(64, 2 n) slots."""
    c = 64
    while c < 2 * n:
        c *= 2
    return c


def read_key(key):
    """The bytes whose xxh3 a (kind, name) key is stored under: the name itself for a plain key, the 16-byte
    namespaced key for a TTL key -- so every entry can be read through the keyed reads."""
    kind, name = key
    return name if kind == "p" else T.ns_key(name)


def hash_of(key):
    return O.xxh3_64(read_key(key))


def tomb_hashes(f: bytes, built: dict) -> set:
    """The hashes of KeyIndexer::build's result whose indexed entry is a tombstone (test_session_goes_on's rule)."""
    out = set()
    for h, v in built.items():
        mo = v & MASK48
        if f[mo - 1: mo] == b"\x00" and int.from_bytes(f[mo + 8: mo + 16], "little") == mo - 1:
            out.add(h)
    return out


class SessionModel:
    """The store's bytes, tail and capacity, {key_hash: payload} of the live entries, the tombstoned hashes, and
    the table's slot bookkeeping.  One method per operation: it returns what the device call must return, or
    raises the exception the device call must raise (same class; the model's message is part of the device's)."""

    def __init__(self, capacity: int):
        self.buf, self.tail, self.cap = bytearray(), 0, S.padded_size(capacity)
        self.live, self.tombs = {}, set()
        self.seq, self.n_writes = {}, 0  # write order of the live entries
        self.slots, self.tcap = set(), table_capacity(0)  # hashes that own a slot (live or deleted), the slots
        self.ever = set()
        self.peak_live = 0
        self.last_sweep = []  # (metadata offset, write order) of the entries the last sweep removed

    # -- helpers --------------------------------------------------------------------------------

    def _refuse(self, exc):
        exc.model = self
        raise exc

    def _fits(self, new_tail):
        return S.padded_size(new_tail) <= self.cap

    def _apply(self, hashes):
        """DeviceIndex.apply's slot rule for a batch of written hashes (before `live` is updated)."""
        used, fresh = len(self.slots), len(set(hashes) - self.slots)
        if used + fresh > self.tcap // 2:  # SRD_ERR_FULL: export the live keys, rebuild at twice the need
            self.tcap = table_capacity(max(2 * (used + len(hashes)), len(self.live)))
            self.slots = set(self.live)
        self.slots |= set(hashes)

    def _append(self, entries, allow_null=False):
        nt = O.write_entries(self.buf, self.tail, entries, allow_null=allow_null)
        assert nt == len(self.buf)
        self.tail = nt

    def _tombstones(self, hashes):
        """One tombstone per hash, in order; every hash is live."""
        nt = self.tail + 21 * len(hashes)
        if not self._fits(nt):
            self._refuse(ValueError("the tombstones end beyond the store's capacity"))
        self._append([(h, b"\x00") for h in hashes], allow_null=True)
        assert self.tail == nt
        for h in hashes:
            self.live.pop(h, None)
            self.seq.pop(h, None)
            self.tombs.add(h)

    def offsets(self):
        """{hash: metadata offset} of the live entries, from KeyIndexer::build of the bytes."""
        built = O.key_indexer_build(np.frombuffer(bytes(self.buf), np.uint8), self.tail) if self.tail else {}
        return {h: v & MASK48 for h, v in built.items() if h in self.live}

    # -- operations -----------------------------------------------------------------------------

    def write(self, entries, stream_rule=False, host=False):
        """batch_write[_with_key_hashes], batch_write_device[_with_key_hashes], batch_write_stream[_with_key_hashes]:
        entries = [(key_hash, payload)].  Returns the new tail."""
        nt = tail_after(self.tail, [len(p) for _, p in entries])
        if not self._fits(nt):
            self._refuse(ValueError(f"the batch ends at {nt}: beyond the store's capacity" if host else
                                    "beyond the store's capacity"))
        if stream_rule and any(not any(p) for _, p in entries):  # (the check comes after the capacity's)
            self._refuse(S.SrdError(NULL_ONLY))
        self._apply([h for h, _ in entries])
        self._append(entries)
        assert self.tail == nt
        for h, p in entries:
            self.live[h] = p
            self.seq[h] = self.n_writes
            self.n_writes += 1
            self.tombs.discard(h)
            self.ever.add(h)
        self.peak_live = max(self.peak_live, len(self.live))
        return self.tail

    def write_ttl(self, names, values, ttls, now, host=False):
        """batch_write_with_ttl / batch_write_stream_with_ttl: le64(min(now + ttl, 2^64 - 1)) || value under the
        namespaced hash."""
        return self.write([(T.ns_hash(k, S.TTL_PREFIX), T.le64(min(now + t, M64)) + v)
                           for k, v, t in zip(names, values, ttls)], host=host)

    def delete(self, hashes):
        present = [h for h in hashes if h in self.live]
        if present:
            self._tombstones(present)
        return self.tail

    def rename(self, olds, news):
        """All entries appended under the new hashes, then all the old ones deleted; refused as a whole."""
        entries = [(n, self.live[o]) for o, n in zip(olds, news)]
        nt = tail_after(self.tail, [len(p) for _, p in entries])
        if not self._fits(nt + 21 * len(olds)):
            self._refuse(ValueError("beyond the store's capacity"))
        self.write(entries, stream_rule=True)
        return self.delete(olds)

    def copy(self, hashes, target: "SessionModel"):
        return target.write([(h, self.live[h]) for h in hashes], stream_rule=True)

    def transfer(self, hashes, target: "SessionModel"):
        """copy, then delete here; refused as a whole."""
        entries = [(h, self.live[h]) for h in hashes]  # (a missing key is reported before the capacity)
        if not self._fits(self.tail + 21 * len(hashes)):
            self._refuse(ValueError("the tombstones end beyond the store's capacity"))
        target.write(entries, stream_rule=True)
        return self.delete(hashes)

    def read_ttl(self, hashes, now, evict):
        """(status, value | None, expiry) per query, judged against the store as it is when the call starts, and
        the number of keys evicted: one tombstone per distinct expired key, in the order of each key's last
        occurrence in the batch."""
        status, values, expiry = [], [], []
        for h in hashes:
            p = self.live.get(h)
            if p is None:
                s, v, e = S.TTL_NOT_FOUND, None, 0
            elif len(p) < 8:
                s, v, e = S.TTL_TOO_SHORT, None, 0
            else:
                e = int.from_bytes(p[:8], "little")
                s, v = (S.TTL_EXPIRED, None) if e <= now else (S.TTL_LIVE, p[8:])
            status.append(s)
            values.append(v)
            expiry.append(e)
        order = []
        if evict:
            last = {h: i for i, (h, s) in enumerate(zip(hashes, status)) if s == S.TTL_EXPIRED}
            order = sorted(last, key=last.get)
            if order:
                self._tombstones(order)
        return status, values, expiry, len(order)

    def sweep(self, now, plan=False):
        """(n_judged, n_expired, n_short, next_expiry): every live entry judged as a TTL entry, plain ones
        included; tombstones in ascending metadata offset of the entries they remove."""
        short = [h for h, p in self.live.items() if len(p) < 8]
        exp = {h: int.from_bytes(p[:8], "little") for h, p in self.live.items() if len(p) >= 8}
        expired = [h for h, e in exp.items() if e <= now]
        nxt = min([e for e in exp.values() if e > now], default=M64)
        stats = (len(self.live), len(expired), len(short), nxt)
        if plan or not expired:
            return stats
        off = self.offsets()
        expired.sort(key=off.get)
        removed = [(off[h], self.seq[h]) for h in expired]
        self._tombstones(expired)
        self.last_sweep = removed
        return stats

    def compact(self, capacity=None):
        """(n_entries, new_len, kept_bytes): model_compact, newest first."""
        f = bytes(self.buf)
        out, its = L.model_compact(f, self.tail)
        cap = S.padded_size(capacity) if capacity is not None else self.cap
        if out and S.padded_size(len(out)) > cap:
            self._refuse(ValueError("beyond the capacity"))
        if any(not any(f[s:e]) for s, e, _, _ in its):
            self._refuse(S.SrdError(NULL_ONLY))
        assert {k for _, _, _, k in its} == set(self.live)
        self.buf, self.tail, self.cap = bytearray(out), len(out), cap
        self.tombs = set()
        self.slots = set(self.live)
        self.tcap = table_capacity(max(len(its), 1))
        return len(its), len(out), sum(e - s + 20 for s, e, _, _ in its)

    def reserve(self, capacity):
        if capacity < self.tail:
            self._refuse(ValueError("below the tail"))
        self.cap = S.padded_size(capacity)

    def savings(self):
        return self.tail - sum(len(p) + 20 for p in self.live.values())


# -- running one operation of a schedule on the models ----------------------------------------------

def resolve(m: SessionModel, pieces):
    """A payload's pieces as bytes: ("b", bytes) as they are, ("s", a, b) the store's own bytes [a, b)."""
    return [bytes(m.buf[p[1]: p[2]]) if p[0] == "s" else p[1] for p in pieces]


def model_step(ms, op, a):
    """Operation (op, a) on the models ms: the value the device call must return (or the model's exception)."""
    m = ms[a["store"]]
    if op == "write":
        ents = [(hash_of(k), b"".join(resolve(m, p))) for k, p in zip(a["keys"], a["payloads"])]
        return m.write(ents, stream_rule=a["path"].startswith("stream"), host=a["path"].startswith("host"))
    if op == "write_ttl":
        return m.write_ttl(a["names"], [b"".join(resolve(m, p)) for p in a["values"]], a["ttls"], a["now"],
                           host=a["path"] == "host")
    if op == "delete":
        return m.delete([hash_of(k) for k in a["keys"]])
    if op == "rename":
        return m.rename([hash_of(k) for k in a["olds"]], [hash_of(k) for k in a["news"]])
    if op == "copy":
        return m.copy([hash_of(k) for k in a["keys"]], ms[a["target"]])
    if op == "transfer":
        return m.transfer([hash_of(k) for k in a["keys"]], ms[a["target"]])
    if op == "read_ttl":
        return m.read_ttl([T.ns_hash(n, S.TTL_PREFIX) for n in a["names"]], a["now"], a["evict"])
    if op == "sweep":
        return m.sweep(a["now"], a["plan"])
    if op == "compact":
        return m.compact(a["capacity"])
    if op == "reserve":
        return m.reserve(a["capacity"])
    raise AssertionError(op)


def outcome(call):
    """("ok", value) or ("err", exception) of one operation."""
    try:
        return "ok", call()
    except (ValueError, KeyError, S.SrdError) as e:
        return "err", e


def op_keys(op, a):
    """Every (kind, name) key an operation names."""
    if op in ("write", "delete", "copy", "transfer"):
        return list(a["keys"])
    if op == "rename":
        return list(a["olds"]) + list(a["news"])
    if op in ("write_ttl", "read_ttl"):
        return [("t", n) for n in a["names"]]
    return []


def describe(op, a):
    """An operation and its arguments for an assertion message, long payloads as their lengths."""
    def short(v):
        if isinstance(v, (bytes, bytearray)):
            return v if len(v) <= 24 else f"<{len(v)} bytes>"
        if isinstance(v, (list, tuple)):
            return type(v)(short(x) for x in v)
        return v
    return f"{op} " + ", ".join(f"{k}={short(v)!r}" for k, v in a.items())


# -- the schedule -----------------------------------------------------------------------------------

def draw_len(rng):
    r = rng.random()
    return rng.choice(BIG) if r < 0.02 else rng.choice(MID) if r < 0.12 else rng.choice(SMALL)


def cut(rng, payload: bytes):
    """The payload in 1 to 4 pieces at random byte offsets (zero-length pieces included)."""
    at = sorted(rng.randint(0, len(payload)) for _ in range(rng.randint(0, 3)))
    return [("b", payload[a:b]) for a, b in zip([0] + at, at + [len(payload)])]


class Generator:
    def __init__(self, seed):
        self.rng = rng = random.Random(seed)
        self.ms = [SessionModel(CAP0), SessionModel(CAP1)]
        self.ops, self.now, self.n_fresh = [], NOW0, 0
        names, i = [], 0
        while len(names) < 48:  # the pool: key lengths from test_gpu_ttl's KEY_LENS (one key of length 0)
            n = rng.randbytes(T.KEY_LENS[i % len(T.KEY_LENS)])
            i += 1
            if n not in names:
                names.append(n)
        self.pool = [("t" if i % 2 else "p", n) for i, n in enumerate(names)]
        self.extra = []  # keys renamed to
        self.due = []  # (step, fresh keys to delete then)
        self.copied = []  # keys copied or transferred to the second store

    # .. emitting, with a user's answer to a capacity refusal

    def emit(self, op, a):
        for _ in range(4):
            self.ops.append((op, a))
            kind, v = outcome(lambda: model_step(self.ms, op, a))
            if kind == "ok" or not isinstance(v, ValueError) or "capacity" not in str(v):
                return kind, v
            m = v.model
            s = self.ms.index(m)
            if op != "compact" and m.savings() > m.tail // 4:
                self.emit("compact", {"store": s, "capacity": None})
            else:
                need = sum(sum(len(x) for x in resolve(self.ms[a["store"]], p)) + 84
                           for f in ("payloads", "values") for p in a.get(f, []))
                self.emit("reserve", {"store": s, "capacity": 2 * (m.cap - 8192) + need})
            a = dict(a)  # the same call again (the store's own bytes may have moved: such pieces as plain bytes)
            for f in ("payloads", "values"):
                if f in a:
                    a[f] = [[("b", x) for x in resolve(self.ms[a["store"]], p)] for p in a[f]]
        raise AssertionError("a refused call was not admitted after three answers")

    def fresh_name(self, prefix=b"f"):
        self.n_fresh += 1
        n = prefix + b"%d" % self.n_fresh
        want = self.rng.choice([x for x in T.KEY_LENS if x])
        return n + b"." * max(want - len(n), 0)

    def payload(self, n=None):
        return L.nonzero_bytes(self.rng, draw_len(self.rng) if n is None else n)

    def pieces(self, m, payload, stream):
        rng = self.rng
        if not stream:
            return [("b", payload)]
        p = cut(rng, payload)
        if m.tail > 64 and rng.random() < 0.2:  # one piece is a slice of the store's own buffer below the tail
            a = rng.randrange(0, m.tail - 1)
            p.insert(rng.randint(0, len(p)), ("s", a, min(m.tail, a + rng.choice([1, 20, 64, 777, 5000]))))
        return p

    def live_keys(self, s, pred=lambda k: True):
        m = self.ms[s]
        return [k for k in self.pool + self.extra if pred(k) and hash_of(k) in m.live]

    # .. the operations

    def op_write(self, keys, store=0):
        rng, m = self.rng, self.ms[store]
        if len(keys) > 1 and rng.random() < 0.3:
            keys = keys + [rng.choice(keys)]  # a key twice in one batch: the later entry wins
        path = rng.choice(WRITE_PATHS)
        pays = [self.pieces(m, self.payload(), path.startswith("stream")) for _ in keys]
        return self.emit("write", {"store": store, "path": path, "keys": keys, "payloads": pays,
                                   "dev": rng.random() < 0.5})

    def op_fresh(self):
        rng = self.rng
        if self.due:  # one batch of fresh keys at a time
            return self.delete_due(0)
        keys = [("p", self.fresh_name()) for _ in range(rng.randint(1, 40))]
        self.op_write(keys)
        self.due.append((len(self.ops) + rng.randint(2, 4), keys))

    def delete_due(self, i):
        rng = self.rng
        _at, keys = self.due.pop(i)
        return self.emit("delete", {"store": 0, "keys": keys, "by": rng.choice(["keys", "hashes"]),
                                    "dev": rng.random() < 0.5})

    def op_pool(self):
        rng = self.rng
        plain = [k for k in self.pool + self.extra if k[0] == "p"]
        if rng.random() < 0.25:  # entries under namespaced hashes written by the plain writes: short ones among them
            keys = rng.sample([k for k in self.pool if k[0] == "t"], rng.randint(1, 4))
            pays = [[("b", self.payload(rng.choice([1, 7, 8, 9, 64])))] for _ in keys]
            return self.emit("write", {"store": 0, "path": rng.choice(["host_hashes", "dev_hashes", "stream_hashes"]),
                                       "keys": keys, "payloads": pays, "dev": rng.random() < 0.5})
        gone = [k for k in plain if hash_of(k) in self.ms[0].tombs]
        if gone and rng.random() < 0.4:  # only keys whose slot is deleted: a revival
            return self.op_write(rng.sample(gone, min(len(gone), rng.randint(1, 3))))
        return self.op_write(rng.sample(plain, min(len(plain), rng.choice([1, 2, 3, 5, 8, 13]))))

    def op_write_ttl(self):
        rng, m = self.rng, self.ms[0]
        names = [n for k, n in self.pool if k == "t"]
        names = rng.sample(names, rng.choice([1, 2, 4, 8, 12, 16, 24]))
        if len(names) > 1 and rng.random() < 0.3:
            names.append(rng.choice(names))
        stream = rng.random() < 0.5
        vals = [self.pieces(m, self.payload() if rng.random() < 0.9 else b"", stream) for _ in names]
        ttls = [rng.choice([0, 1, 1, 2, 2, 3, 5, 8, 1000]) * TICK for _ in names]
        return self.emit("write_ttl", {"store": 0, "path": "stream" if stream else "host", "names": names,
                                       "values": vals, "ttls": ttls, "now": self.now})

    def op_delete(self, store=0):
        rng, m = self.rng, self.ms[store]
        known = self.pool + self.extra if store == 0 else self.copied
        live = [k for k in known if hash_of(k) in m.live]
        keys = rng.sample(live, min(len(live), rng.randint(0, 5))) + [("p", b"never-%d" % rng.randrange(99))]
        keys += rng.sample(known, min(len(known), 2))
        if keys and rng.random() < 0.5:
            keys.append(rng.choice(keys))  # listed twice: two tombstones if it is live
        rng.shuffle(keys)
        return self.emit("delete", {"store": store, "keys": keys, "by": rng.choice(["keys", "hashes"]),
                                    "dev": rng.random() < 0.5})

    def op_rename(self):
        rng = self.rng
        live = self.live_keys(0)
        if not live:
            return self.op_pool()
        olds = rng.sample(live, min(len(live), rng.randint(1, 3)))
        news = [("p", self.fresh_name(b"ren-")) for _ in olds]
        kind, _ = self.emit("rename", {"store": 0, "olds": olds, "news": news})
        if kind == "ok":
            self.extra += news

    def op_move(self, op):
        rng = self.rng
        live = self.live_keys(0)
        if not live:
            return self.op_pool()
        keys = rng.sample(live, min(len(live), rng.randint(1, 4)))
        kind, _ = self.emit(op, {"store": 0, "target": 1, "keys": keys})
        if kind == "ok":
            self.copied += [k for k in keys if k not in self.copied]

    def op_read_ttl(self):
        rng, m = self.rng, self.ms[0]
        names = [n for k, n in self.pool if k == "t"]
        live = [n for n in names if T.ns_hash(n, S.TTL_PREFIX) in m.live]
        expired = [n for n in live if len(m.live[T.ns_hash(n, S.TTL_PREFIX)]) >= 8 and
                   int.from_bytes(m.live[T.ns_hash(n, S.TTL_PREFIX)][:8], "little") <= self.now]
        q = rng.sample(live, min(len(live), rng.randint(1, 10))) + rng.sample(names, 3)
        q += rng.sample(expired, min(len(expired), 3))
        q += [b"never-%d" % rng.randrange(99), rng.choice(expired or q)]  # a duplicate: an expired key if there is one
        rng.shuffle(q)
        return self.emit("read_ttl", {"store": 0, "names": q, "now": self.now, "evict": rng.random() < 0.75})

    def step(self):
        rng = self.rng
        if rng.random() < 0.5:
            self.now += TICK
        for i, (at, keys) in enumerate(self.due):
            if at <= len(self.ops):
                return self.delete_due(i)
        r = rng.random() * 100
        for w, f in [(26, self.op_fresh), (10, self.op_pool), (12, self.op_write_ttl), (7, self.op_delete),
                     (11, self.op_read_ttl), (6, lambda: self.emit("sweep", {"store": 0, "now": self.now,
                                                                             "plan": rng.random() < 0.2})),
                     (5, self.op_rename), (5, lambda: self.op_move("copy")), (5, lambda: self.op_move("transfer")),
                     (3, lambda: self.emit("compact", {"store": int(rng.random() < 0.2), "capacity": None})),
                     (4, lambda: self.emit("reserve", {"store": 0, "capacity": self.ms[0].cap - 8192 + (64 << 10)})),
                     (2, lambda: self.op_delete(1)), (4, self.op_null_only)]:
            if r < w:
                return f()
            r -= w

    def op_null_only(self):
        """A stream write one of whose payloads is NULL bytes only: refused, nothing written."""
        rng = self.rng
        keys = [("p", self.fresh_name(b"z")) for _ in range(rng.randint(1, 3))]
        pays = [cut(rng, self.payload(rng.choice(SMALL))) for _ in keys]
        pays[rng.randrange(len(keys))] = cut(rng, bytes(rng.choice([1, 3, 64, 65])))
        return self.emit("write", {"store": 0, "path": rng.choice(["stream_keys", "stream_hashes"]), "keys": keys,
                                   "payloads": pays, "dev": rng.random() < 0.5})


_SCHEDULES = {}


def schedule(seed, n_steps):
    """The first n_steps operations [(op, args)] of seed's session (a refused call's answer and repetition are
    steps of their own)."""
    if seed not in _SCHEDULES or len(_SCHEDULES[seed]) < n_steps:
        g = Generator(seed)
        while len(g.ops) < n_steps:
            g.step()
        _SCHEDULES[seed] = g.ops
    return _SCHEDULES[seed][:n_steps]


# -- CPU tests: the model's invariants and the seeds' coverage ----------------------------------------

def check_invariants(m: SessionModel, where):
    f = bytes(m.buf)
    assert len(f) == m.tail, where
    a = np.frombuffer(f, np.uint8)
    assert (O.recover_valid_chain(a) if f else 0) == m.tail, where
    built = O.key_indexer_build(a, m.tail) if f else {}
    tombs = tomb_hashes(f, built)
    assert set(built) - tombs == set(m.live), where
    assert tombs == m.tombs, where
    its = L.entry_iterator(f, m.tail)
    assert {k: f[s:e] for s, e, _, k in its} == m.live and len(its) == len(m.live), where
    assert len(m.slots) <= m.tcap // 2 and set(m.live) <= m.slots, where


def table_state(m: SessionModel):
    return len(m.slots), len(m.live), m.tcap


def is_revival(before, after):
    """A write of a key whose slot was deleted: `used` unchanged while `len` rose ((used, len, capacity) pairs)."""
    return after[0] == before[0] and after[1] > before[1] and after[2] == before[2]


def run_model(seed, n_steps, check=None):
    """The schedule on fresh models: the coverage counters (and check(models, step, op, args, outcome) per step)."""
    ms = [SessionModel(CAP0), SessionModel(CAP1)]
    c = collections.Counter()
    compacted, plain = 0, set()  # the tail the last compaction of the first store left: below it, newest first
    for i, (op, a) in enumerate(schedule(seed, n_steps)):
        m = ms[a["store"]]
        plain |= {hash_of(k) for k in op_keys(op, a) if k[0] == "p"}
        chain_before = len(O.chain(bytes(m.buf), m.tail, False)) if op == "compact" and m.tail else 0
        plain_long = any(len(p) >= 8 for h, p in m.live.items() if h in plain)
        table = table_state(ms[0])
        kind, v = outcome(lambda: model_step(ms, op, a))
        c[op] += 1
        c["table changes"] += table_state(ms[0])[2] != table[2]
        c["revivals"] += op in ("write", "write_ttl") and a["store"] == 0 and is_revival(table, table_state(ms[0]))
        if kind == "err":
            c["capacity refusals"] += isinstance(v, ValueError) and "capacity" in str(v)
            c["NULL-only refusals"] += isinstance(v, S.SrdError) and NULL_ONLY in str(v)
        elif op == "compact":
            c["compactions with dead entries"] += chain_before > v[0]
            if a["store"] == 0:
                compacted = v[1]
            if m.buf:  # after every compaction the new bytes are one valid chain
                assert O.recover_valid_chain(np.frombuffer(bytes(m.buf), np.uint8)) == len(m.buf)
        elif op == "sweep":
            c["sweeps with short and long plain entries"] += v[2] > 0 and plain_long
            if not a["plan"] and v[1]:
                offs = m.last_sweep  # in tombstone order: ascending offset; and the write order of the same entries
                assert [o for o, _ in offs] == sorted(o for o, _ in offs) and len(offs) == v[1]
                placed = [q for o, q in offs if o < compacted]  # entries that compaction itself placed
                c["sweeps after a compaction whose offset order is not the write order"] += \
                    len(placed) >= 2 and placed != sorted(placed)
        elif op == "read_ttl" and a["evict"]:
            twice = {n for n in a["names"] if a["names"].count(n) > 1}
            c["evicting reads that expire a key listed twice"] += any(
                q == S.TTL_EXPIRED and n in twice for n, q in zip(a["names"], v[0]))
        if check:
            check(ms, i, op, a, (kind, v))
    c["ever"], c["peak live"] = len(ms[0].ever), ms[0].peak_live
    return c, ms


@pytest.mark.parametrize("seed", SEEDS + [CORRUPTION_SEED])
def test_model_invariants_after_every_step(seed):
    n = CORRUPTION_STEPS if seed == CORRUPTION_SEED else N_STEPS

    def check(ms, i, op, a, out):
        where = f"seed {seed:#x} step {i}: {describe(op, a)}"
        before = states[0]
        if out[0] == "err":  # a refused operation leaves every field as it was
            assert [state(m) for m in ms] == before, where
        states[0] = [state(m) for m in ms]
        for m in ms:
            check_invariants(m, where)

    def state(m):
        return bytes(m.buf), m.tail, m.cap, dict(m.live), set(m.tombs), set(m.slots), m.tcap

    states = [[state(SessionModel(CAP0)), state(SessionModel(CAP1))]]
    run_model(seed, n, check)


@pytest.mark.parametrize("seed", SEEDS)
def test_seed_meets_the_coverage_conditions(seed):
    c, ms = run_model(seed, N_STEPS)
    for k in KINDS:
        assert c[k] >= 3, (k, dict(c))
    assert c["compactions with dead entries"] >= 2, dict(c)
    assert c["sweeps after a compaction whose offset order is not the write order"] >= 1, dict(c)
    assert c["capacity refusals"] >= 2, dict(c)
    assert c["NULL-only refusals"] >= 1, dict(c)
    assert c["evicting reads that expire a key listed twice"] >= 3, dict(c)
    assert c["sweeps with short and long plain entries"] >= 1, dict(c)
    assert c["ever"] >= 4 * c["peak live"], dict(c)  # deleted-slot churn
    assert c["table changes"] >= 2 and c["revivals"] >= 1, dict(c)  # what the device test must observe
    assert len(ms[0].buf) < 8 << 20  # the session's store stays within a few MiB


def test_corruption_seed_has_its_victims():
    """After its steps the corruption test's session holds a live payload of more than one unit and a superseded
    entry that is no tombstone."""
    _c, ms = run_model(CORRUPTION_SEED, CORRUPTION_STEPS)
    assert corruption_victims(ms[0]) is not None


def corruption_victims(m: SessionModel):
    """((payload start, metadata offset, key hash) of a live entry longer than a unit, the payload start of a
    superseded non-tombstone entry), or None."""
    f = bytes(m.buf)
    its = L.entry_iterator(f, m.tail)
    live = [(s, e, k) for s, e, _, k in its if e - s > CH]
    newest = {e for _, e, _, _ in its}
    dead = [c["payload_start"] for c in O.chain(f, m.tail, False)
            if c["meta_off"] not in newest and not c["is_tombstone"] and c["payload_len"] >= 8]
    return (live[0], dead[0]) if live and dead else None


def test_schedule_is_deterministic_and_a_prefix():
    a = schedule(SEEDS[0], N_STEPS)
    _SCHEDULES.clear()
    b = schedule(SEEDS[0], N_STEPS)
    assert a == b and schedule(SEEDS[0], 50) == b[:50]
    _SCHEDULES.clear()
    assert schedule(SEEDS[0], 50) == b[:50]


def test_model_rules_on_small_cases():
    """The rules the generator cannot be relied on to isolate, each on a store of a few entries."""
    m = SessionModel(1 << 16)
    h = [O.xxh3_64(b"k%d" % i) for i in range(4)]
    m.write([(h[0], b"a"), (h[1], b"bb"), (h[0], b"ccc")])  # a key twice: the later entry wins
    assert m.live == {h[0]: b"ccc", h[1]: b"bb"}
    t = m.tail
    assert m.delete([h[2]]) == t  # nothing live: nothing written
    assert m.delete([h[1], h[2], h[1]]) == t + 42 and h[1] in m.tombs  # listed twice: two tombstones, as the reference
    # the expiry tie counts as expired; eviction in the order of the last occurrences
    m.write_ttl([b"x", b"y", b"z"], [b"1", b"", b"3"], [10, 20, 30], now=100)
    hx, hy, hz = (T.ns_hash(k, S.TTL_PREFIX) for k in (b"x", b"y", b"z"))
    st, vals, exp, n = m.read_ttl([hy, hx, hz, hy, hx], now=120, evict=False)
    assert st == [S.TTL_EXPIRED, S.TTL_EXPIRED, S.TTL_LIVE, S.TTL_EXPIRED, S.TTL_EXPIRED] and n == 0
    assert vals[2] == b"3" and exp == [120, 110, 130, 120, 110]
    before = bytes(m.buf)
    assert m.read_ttl([hy, hx, hz, hy, hx], now=120, evict=True)[3] == 2
    want = bytearray(before)
    O.write_entries(want, len(before), [(hy, b"\x00"), (hx, b"\x00")], allow_null=True)
    assert bytes(m.buf) == bytes(want)
    # a refusal leaves everything as it was, whichever rule refuses
    small = SessionModel(4096)
    small.write([(h[0], b"v" * 4000)])
    snap = (bytes(small.buf), small.tail, dict(small.live))
    for call in (lambda: small.write([(h[1], b"w" * 5000)]), lambda: small.write([(h[1], b"\x00\x00")], stream_rule=True),
                 lambda: small.rename([h[0]], [h[1]]), lambda: small.compact(capacity=0)):
        with pytest.raises((ValueError, S.SrdError)):
            call()
        assert (bytes(small.buf), small.tail, dict(small.live)) == snap
