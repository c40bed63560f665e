"""The optimistic scan's block partition, pinned, and nothing surviving a call.

Which resident spans each scan block takes is chosen per box and per call from
timing history (XPart / xpart_update, srd_kernels.hip: each call's link2 turns
the blocks' measured durations into the next call's block-start table), and the
pass's device buffers -- tile values, candidate records, span_first, wave
totals -- persist from call to call.  A span that a partition failed to cover
would silently reuse the previous call's correct values on an unchanged store.

So here every call runs on a block-start table the test installs
(srd_ctx_set_scan_blocks; srd_ctx_scan_blocks proves the scan ran with it),
drawn from the whole documented domain -- empty blocks at 0 and g - 1 and in
runs, one-span blocks, blocks exactly at the bound -- and between consecutive
calls on one context every 2 KiB of the device-resident store gets a changed
payload byte, so every tile value and every entry's CRC must be computed anew.
Every call is bit-exact against the oracle run over a host copy that received
the same mutations: the counts, all eight per-entry arrays, the sorted index
pairs, and mode / full_reason (a bad CRC is data, not a status).

Every torch write to a store is followed by torch.cuda.synchronize() before
the library call: the library launches on its own non-blocking stream.
"""
import itertools
import os

import numpy as np
import pytest

import oracle as O
import srd_amd as S

pytestmark = pytest.mark.gpu

FIELDS = (("meta_off", np.uint64), ("key_hash", np.uint64), ("prev_offset", np.uint64),
          ("payload_start", np.uint64), ("payload_len", np.uint64), ("crc_stored", np.uint32),
          ("crc_computed", np.uint32), ("crc_ok", np.uint8))
SKEWED = "3,0.3,1,2"  # one of test_scan_wave_shares' sets


def _ctx_with_env(**env):
    """A context created under the given SRD_* knobs (read once at srd_ctx_create)."""
    env = {k: str(v) for k, v in env.items() if v is not None}
    old = {k: os.environ.get(k) for k in env}
    os.environ.update(env)
    try:
        return S.Context(0)
    finally:
        for k, v in old.items():
            if v is None:
                del os.environ[k]
            else:
                os.environ[k] = v


# ---- stores: device-resident, with a host copy that receives the same mutations ----

class Store:
    def __init__(self, dev, size, host):
        self.dev, self.size, self.host = dev, size, host
        ch = O.chain_arrays(host, size, compute_crc=False)
        self.pstart = ch["payload_start"].astype(np.int64)
        self.plen = ch["payload_len"].astype(np.int64)
        self.meta_off = ch["meta_off"].astype(np.int64)
        self.calls = 0

    @property
    def ptr(self):
        return self.dev.data_ptr()

    def mutate(self):
        """XOR payload bytes, on the device and in the host copy, so that every 2 KiB of the file holds a
        changed byte: per entry the payload offsets d, d + 900, d + 1800, ... below its length (d moves with
        the call number; d % length for a payload no longer than d).  Between the last one of an entry and
        the first of the next lie < 900 + 20 (metadata) + 63 (prepad) + 900 bytes.  No metadata or prepad
        byte changes."""
        import torch
        torch.cuda.synchronize()  # the previous call's kernels may still be reading the store
        self.calls += 1
        d = (self.calls * 37) % 900
        first = np.where(self.plen > d, d, d % np.maximum(self.plen, 1))
        cnt = np.where(self.plen > d, (self.plen - d + 899) // 900, 1)
        ent = np.repeat(np.arange(self.plen.size), cnt)
        j = np.arange(ent.size) - np.repeat(np.cumsum(cnt) - cnt, cnt)
        pos = self.pstart[ent] + first[ent] + 900 * j
        assert np.all(pos < self.pstart[ent] + self.plen[ent]) and np.all(pos >= self.pstart[ent])
        pos = np.unique(np.append(pos, self.pstart[-1] + self.plen[-1] - 1))  # and the store's last payload byte
        assert pos[0] < 2048 and int(np.diff(pos).max()) < 2048
        val = 1 << (self.calls % 8)
        self.host[pos] ^= np.uint8(val)
        idx = torch.from_numpy(pos).cuda()
        self.dev[idx] = self.dev[idx] ^ val
        torch.cuda.synchronize()  # the library's stream is not ordered behind torch's


_PRISTINE = {}


def _pristine(name):
    import torch
    if name not in _PRISTINE:
        n, plen, lens, seed = {
            "S16": (1000, 4096, None, 0x5EED0001),      # grid 16, ~16 spans per block, one span per wave
            "S256": (20_000, 4096, None, 0x5EED0001),   # 83 MB: the full 256-block grid, waves of 0-2 spans
            "S256b": (20_000, 4096, None, 0x5EED0B0B),  # other keys and payload bytes, the same span count
            "Z": (8000, 0, S.zipf_lens(8000), 0x5EED0001),  # ~70 MB, entries up to 1 MiB: CRCs assembled across blocks
            "D": (200_000, 8, None, 0x5EED0001),        # the bench_8b shape: overflows the 8-slot cap
            "T1": (3, 4096, None, 0x5EED0001), "T2": (6, 4096, None, 0x5EED0001),      # 1, 2 spans
            "T17": (66, 4096, None, 0x5EED0001), "T33": (129, 4096, None, 0x5EED0001),  # 17, 33 spans
        }[name]
        size = S.synth_store_len(n, plen, lens)
        t = torch.zeros(S.padded_size(size), dtype=torch.uint8, device="cuda")
        torch.cuda.synchronize()
        S.synth_store_device(t.data_ptr(), n, plen, lens, seed=seed)
        torch.cuda.synchronize()
        _PRISTINE[name] = (t, size, t[:size].cpu().numpy())
    return _PRISTINE[name]


def _store(name) -> Store:
    """A private copy of the named store (the cached original stays unchanged)."""
    import torch
    t, size, host = _pristine(name)
    dev = t.clone()
    torch.cuda.synchronize()
    return Store(dev, size, host.copy())


# ---- block-start tables ----

def _bound(g, ns):
    return (5 * ns + 4 * g - 1) // (4 * g) + 1


def _table_ok(st, g, ns):
    """The documented domain of srd_ctx_set_scan_blocks (include/srd_amd.h)."""
    st = np.asarray(st).astype(np.int64)
    sz = np.diff(st)
    return (1 <= g <= 1024 and st.size == g + 1 and st[0] == 0 and st[g] == ns and bool(np.all(sz >= 0))
            and bool(np.all(sz <= _bound(g, ns))))


def _fit(sz, ns, bound, rng):
    """Block sizes moved into [0, bound] and their sum to ns: blocks in a seeded random order, the empty
    and the full ones last."""
    sz = np.clip(np.asarray(sz, np.int64), 0, bound)
    order = rng.permutation(sz.size)
    for spare in (True, False):
        for b in order:
            diff = ns - int(sz.sum())
            if diff == 0:
                break
            if spare and sz[b] in (0, bound):
                continue
            sz[b] += min(diff, bound - sz[b]) if diff > 0 else -min(-diff, sz[b])
    st = np.concatenate([[0], np.cumsum(sz)]).astype(np.uint64)
    assert _table_ok(st, sz.size, ns), (sz, ns, bound)
    return st


def _even(g, ns):
    return (np.arange(g + 1, dtype=np.uint64) * np.uint64(ns)) // np.uint64(g)


def _clamp(g, ns, inv, rng):
    """The clamp extremes of xpart_update, alternating with the XCD (b mod 8: odd / even): 0.9 / 1.1 of even."""
    b = np.arange(g)
    f = np.where(((b % 8) & 1) == inv, 1.1, 0.9)
    return _fit(np.floor(ns / g * f), ns, _bound(g, ns), rng)


def _sawtooth(g, ns, rng):
    """Blocks at the bound between small ones: empty blocks 0 and g - 1, a one-span block, an adjacent empty
    pair (0, 1), then every 8th block empty and more one-span blocks -- as many of these, in this order, as the bound leaves
    room for (the others at the bound must still hold ns spans); the excess is taken off the last full
    blocks.  Returns (starts, features placed)."""
    B = _bound(g, ns)
    small = {}
    want = [(0, 0), (g - 1, 0), (4 % g, 1), (1, 0)] + [(b, 0) for b in range(8, g, 8)] + \
           [(b, 1) for b in range(12, g, 16)] + [(b, 0) for b in range(9, g, 64)]
    for b, s in want:
        if b in small or g < 2:
            continue
        if sum(small.values()) + s + (g - len(small) - 1) * B >= ns:
            small[b] = s
    sz = np.full(g, B, np.int64)
    for b, s in small.items():
        sz[b] = s
    excess = int(sz.sum()) - ns
    for b in range(g - 1, -1, -1):
        if excess <= 0:
            break
        if b in small:
            continue
        take = min(excess, B - 2)  # (stays >= 2: neither empty nor a one-span block)
        sz[b] -= take
        excess -= take
    assert excess == 0
    st = np.concatenate([[0], np.cumsum(sz)]).astype(np.uint64)
    assert _table_ok(st, g, ns)
    return st, sz


def _random_tables(g, ns, rng, n=5):
    B = _bound(g, ns)
    out = []
    for k in range(n):
        if k % 2 == 0:  # sizes uniform in [0, bound]
            sz = rng.integers(0, B + 1, g)
        else:  # mostly empty / one-span / full blocks
            kind = rng.integers(0, 4, g)
            sz = np.select([kind == 0, kind == 1, kind == 2], [0, B, 1], rng.integers(0, B + 1, g))
        out.append(_fit(sz, ns, B, rng))
    return out


def _tables(g, ns, seed, full_sawtooth=True):
    """The issue's set: the even split, the clamp extremes and their inverse, the sawtooth at the bound,
    five seeded random tables from the domain."""
    rng = np.random.default_rng(seed)
    saw, sz = _sawtooth(g, ns, rng)
    B = _bound(g, ns)
    assert sz[0] == 0 and sz[g - 1] == 0 and (sz == 1).any() and (sz == B).any()
    if full_sawtooth:  # (16 blocks: the bound leaves no room for a third empty block beside a one-span one)
        assert (sz == 0).sum() >= g // 8 and sz[1] == 0
    return [("even", _even(g, ns)), ("clamp", _clamp(g, ns, 0, rng)), ("clamp-inv", _clamp(g, ns, 1, rng)),
            ("sawtooth", saw)] + [(f"random{k}", t) for k, t in enumerate(_random_tables(g, ns, rng))]


# ---- one call, checked ----

def _arrays(r):
    out = {k: S.device_to_numpy(getattr(r, k), r.n_chain, dt) for k, dt in FIELDS}
    ik = S.device_to_numpy(r.index_key_hash, r.n_index, np.uint64)
    iv = S.device_to_numpy(r.index_packed, r.n_index, np.uint64)
    o = np.argsort(ik, kind="stable")
    out["index"] = (ik[o], iv[o])
    return out


def _check(r, store, name):
    """One result against the oracle over the store's host copy; returns the result's arrays."""
    host = store.host
    st = O.validate_index(host, 8)
    assert (r.final_len, r.n_chain, r.n_crc_bad, r.n_index) == (st.final_len, st.n_chain, st.n_crc_bad, st.n_index), \
        (name, (r.final_len, r.n_chain, r.n_crc_bad, r.n_index), (st.final_len, st.n_chain, st.n_crc_bad, st.n_index))
    assert (r.mode, r.full_reason) == (S.SRD_MODE_OPTIMISTIC, S.SRD_FULL_NONE), (name, r.mode, r.full_reason)
    ch = O.chain_arrays(host, st.final_len)
    got = _arrays(r)
    for k, _ in FIELDS:
        exp = ch[k].astype(np.uint64)
        bad = np.nonzero(got[k].astype(np.uint64) != exp)[0]
        assert bad.size == 0, (name, k, bad.size, bad[:5], got[k][bad[:5]], exp[bad[:5]])
    keys, packed = O.key_indexer_arrays(host, st.final_len)
    assert np.array_equal(got["index"][0], keys) and np.array_equal(got["index"][1], packed), name
    return got


def _learn(ctx, store):
    """(g, ns) of the store from a first, checked call (the partition the scan ran with)."""
    r = S.validate_index_device(store.ptr, store.size, 0, ctx)
    _check(r, store, "first call")
    st, info = ctx.scan_blocks(S.SCAN_BLOCKS_LAST)
    assert info.n_blocks >= 1 and info.n_spans >= 1 and st.size == info.n_blocks + 1
    assert _table_ok(st, info.n_blocks, info.n_spans)
    return int(info.n_blocks), int(info.n_spans)


def _check_next_table(ctx, g, ns, name):
    """What this call's link2 prepared for the next one (xpart_update's prefix arithmetic on real durations)."""
    st, info = ctx.scan_blocks(S.SCAN_BLOCKS_NEXT)
    assert (info.n_blocks, info.n_spans, info.source) == (g, ns, S.SCAN_BLOCKS_MEASURED), \
        (name, info.n_blocks, info.n_spans, info.source)
    assert _table_ok(st, g, ns), (name, st)


def _call_on(ctx, store, table, g, ns, name):
    """One call on an installed table: proven to have run on it, checked against the oracle.

    Each scan wave's records go, dense, into a region of (spans per wave at the table bound) x (candidate
    slots per span); a table that gives one wave more spans of a dense store than the even split did can
    fill that region.  The pass then grows the slots and retries inside the same call -- on the table its
    first attempt measured, so that result is checked but was not computed on the installed table.  The
    context keeps the grown slots: the same table installed again runs in one attempt."""
    for k in range(4):
        if k:
            store.mutate()
        ctx.set_scan_blocks(table, ns)
        nxt, info = ctx.scan_blocks(S.SCAN_BLOCKS_NEXT)
        assert info.source == S.SCAN_BLOCKS_INSTALLED and np.array_equal(nxt, table), name
        r = S.validate_index_device(store.ptr, store.size, 0, ctx)
        ran, info = ctx.scan_blocks(S.SCAN_BLOCKS_LAST)
        assert (info.first_source, info.n_blocks, info.n_spans) == (S.SCAN_BLOCKS_INSTALLED, g, ns), \
            (name, info.first_source, info.n_blocks, info.n_spans)
        got = _check(r, store, name)
        _check_next_table(ctx, g, ns, name)
        if info.attempts == 1:
            break
        assert info.source == S.SCAN_BLOCKS_MEASURED and _table_ok(ran, g, ns), (name, info.source)
    # a table silently ignored would prove nothing
    assert (info.attempts, info.source) == (1, S.SCAN_BLOCKS_INSTALLED) and np.array_equal(ran, table), \
        (name, info.attempts, info.source)
    return got


def _sequence(ctx, store, seed, full_sawtooth=True, off=None):
    """The table set over one store on one context, the store mutated before every call; with `off` (a
    context with the shares off) the even table's outputs must equal that context's bit for bit."""
    g, ns = _learn(ctx, store)
    for name, table in _tables(g, ns, seed, full_sawtooth):
        store.mutate()
        got = _call_on(ctx, store, table, g, ns, name)
        if off is not None and name == "even":
            r2 = S.validate_index_device(store.ptr, store.size, 0, off)
            st2, info2 = off.scan_blocks(S.SCAN_BLOCKS_LAST)
            assert info2.source == S.SCAN_BLOCKS_EVEN and np.array_equal(st2, table)
            got2 = _check(r2, store, "shares off")
            for k, _ in FIELDS:
                assert np.array_equal(got[k], got2[k]), k
            assert all(np.array_equal(a, b) for a, b in zip(got["index"], got2["index"]))
            assert off.scan_blocks(S.SCAN_BLOCKS_NEXT)[1].n_blocks == 0  # no table is ever prepared there
    return g, ns


# ---- the tests ----

def test_small_grid_tables_and_shares_off():
    """S16 (grid 16, one span per wave): the table set, the even table against a context with SRD_XPART=0."""
    ctx, off = S.Context(0), _ctx_with_env(SRD_XPART=0)
    try:
        g, ns = _sequence(ctx, _store("S16"), 16, full_sawtooth=False, off=off)
        assert g == 16
    finally:
        ctx.close()
        off.close()


@pytest.mark.parametrize("store", ["S256", "Z"])
@pytest.mark.parametrize("loads,weights,fused", [("coal", None, None), ("lines", None, None), ("coal", SKEWED, None),
                                                 ("lines", SKEWED, 0)])
def test_full_grid_tables_pinned_variants(store, loads, weights, fused):
    """S256 (the full 256-block grid, waves of 0-2 spans) and Z (entries up to 1 MiB: one entry's CRC is
    assembled from tile values several blocks wrote): the table set under each tile-load pattern, the
    default and a skewed wave-share set, and once through the unfused glue."""
    ctx = _ctx_with_env(SRD_SCAN_LOADS=loads, SRD_SCAN_WEIGHTS=weights, SRD_GLUE_FUSED=fused)
    off = _ctx_with_env(SRD_XPART=0, SRD_SCAN_LOADS=loads, SRD_SCAN_WEIGHTS=weights) if fused is None else None
    try:
        g, ns = _sequence(ctx, _store(store), 256 + len(store), off=off)
        assert g > 16 and ctx.scan_loads() == (1 if loads == "lines" else 0)
    finally:
        ctx.close()
        if off is not None:
            off.close()


def test_alternating_stores_on_one_context():
    """S256, Z and a seed-shifted S256 (other keys and payload bytes, the same span count) in turn on one
    context, a table installed before each call and each store mutated after its call: a stale candidate
    record, span_first entry or wave total of the previous store shows in the oracle comparison."""
    ctx = S.Context(0)
    try:
        stores = {n: _store(n) for n in ("S256", "Z", "S256b")}
        geo = {n: _learn(ctx, s) for n, s in stores.items()}
        assert geo["S256"] == geo["S256b"] != geo["Z"]
        rng = np.random.default_rng(99)
        tabs = {}
        for n, (g, ns) in geo.items():
            tabs[n] = itertools.cycle([_sawtooth(g, ns, rng)[0]] + _random_tables(g, ns, rng, 2)
                                      + [_clamp(g, ns, 0, rng)])
        for k, n in enumerate(["S256", "Z", "S256b", "S256", "S256b", "Z", "S256"]):
            g, ns = geo[n]
            _call_on(ctx, stores[n], next(tabs[n]), g, ns, f"alt{k}:{n}")
            stores[n].mutate()
    finally:
        ctx.close()


def test_dense_store_retries_on_its_own_table():
    """D (200,000 x 8-byte payloads) overflows the default 8 candidate slots per span, so one call makes
    several attempts: the first on the installed table, every retry on the table the attempt before it
    measured (its own link2 wrote it).  A fresh context each time: a context keeps the grown cap."""
    store = _store("D")
    c0 = S.Context(0)
    try:
        g, ns = _learn(c0, store)
        assert c0.scan_blocks(S.SCAN_BLOCKS_LAST)[1].attempts >= 2
    finally:
        c0.close()
    rng = np.random.default_rng(5)
    for name, table in [("sawtooth", _sawtooth(g, ns, rng)[0]), ("random", _random_tables(g, ns, rng, 1)[0])]:
        store.mutate()
        ctx = S.Context(0)
        try:
            ctx.set_scan_blocks(table, ns)
            r = S.validate_index_device(store.ptr, store.size, 0, ctx)
            ran, info = ctx.scan_blocks(S.SCAN_BLOCKS_LAST)
            assert info.attempts >= 2 and info.first_source == S.SCAN_BLOCKS_INSTALLED, (info.attempts, info.first_source)
            assert (info.source, info.n_blocks, info.n_spans) == (S.SCAN_BLOCKS_MEASURED, g, ns)
            assert _table_ok(ran, g, ns), ran
            _check(r, store, f"dense:{name}")
            _check_next_table(ctx, g, ns, name)
        finally:
            ctx.close()


def _all_tables(g, ns):
    B = _bound(g, ns)
    for sz in itertools.product(range(B + 1), repeat=g):
        if sum(sz) == ns:
            yield np.concatenate([[0], np.cumsum(sz)]).astype(np.uint64)


@pytest.mark.parametrize("name,spans", [("T1", 1), ("T2", 2), ("T17", 17), ("T33", 33)])
def test_tiny_stores_every_table(name, spans):
    """Stores of 1, 2, 17 and 33 spans (1 to 3 blocks): every valid table, enumerated."""
    ctx = S.Context(0)
    try:
        store = _store(name)
        g, ns = _learn(ctx, store)
        assert ns == spans and g <= 3
        n = 0
        for table in _all_tables(g, ns):
            store.mutate()
            _call_on(ctx, store, table, g, ns, f"{name}:{table.tolist()}")
            n += 1
        assert n >= 1
    finally:
        ctx.close()


def test_span_mode_shards_on_tables():
    """S256 cut into two entry-range shards, each through srd_validate_span_device on tables installed for
    its resident span count: the two segments concatenated are the oracle's chain."""
    ctx = S.Context(0)
    try:
        store = _store("S256")
        n = store.plen.size
        cut = int(store.meta_off[n // 2 - 1]) + 20  # the tail of entry n/2 - 1
        off1 = cut // S.SPAN_ALIGN * S.SPAN_ALIGN
        shards = [(store.ptr, 0, 0, cut), (store.ptr + off1, off1, cut, store.size)]
        geo = []
        for p, so, lo, hi in shards:
            r = S.validate_span_device(p, so, lo, hi, 0, ctx)
            assert r.mode == S.SRD_MODE_OPTIMISTIC and r.final_len == hi
            info = ctx.scan_blocks(S.SCAN_BLOCKS_LAST)[1]
            geo.append((int(info.n_blocks), int(info.n_spans)))
        rng = np.random.default_rng(21)
        for k in range(2):
            store.mutate()
            ch = O.chain_arrays(store.host, store.size)
            segs = []
            for (p, so, lo, hi), (g, ns) in zip(shards, geo):
                table = _sawtooth(g, ns, rng)[0] if k == 0 else _random_tables(g, ns, rng, 1)[0]
                ctx.set_scan_blocks(table, ns)
                r = S.validate_span_device(p, so, lo, hi, 0, ctx)
                ran, info = ctx.scan_blocks(S.SCAN_BLOCKS_LAST)
                assert info.source == S.SCAN_BLOCKS_INSTALLED and np.array_equal(ran, table), (k, lo)
                assert (r.mode, r.full_reason, r.final_len) == (S.SRD_MODE_OPTIMISTIC, S.SRD_FULL_NONE, hi)
                segs.append({f: S.device_to_numpy(getattr(r, f), r.n_chain, dt) for f, dt in FIELDS})
                _check_next_table(ctx, g, ns, f"span{k}")
            assert [s["meta_off"].size for s in segs] == [n // 2, n - n // 2]
            for f, _ in FIELDS:
                got = np.concatenate([s[f] for s in segs]).astype(np.uint64)
                assert np.array_equal(got, ch[f].astype(np.uint64)), (k, f)
    finally:
        ctx.close()


def test_install_rejects_and_ignores():
    """srd_ctx_set_scan_blocks refuses (SRD_ERR_ARG, nothing changed) whatever lies outside the documented
    domain, and any table on a context with the shares off; a table made for another span count or grid is
    ignored by the next scan, as a measured one is."""
    ctx, off = S.Context(0), _ctx_with_env(SRD_XPART=0)
    try:
        small, big = _store("S16"), _store("S256")
        g, ns = _learn(ctx, small)
        B = _bound(g, ns)
        good = _even(g, ns)
        before = ctx.scan_blocks(S.SCAN_BLOCKS_NEXT)
        bad = []
        t = good.copy(); t[0] = 1; bad.append((t, ns))
        bad.append((good, ns + 1))
        t = good.copy(); t[3] = t[2] - np.uint64(1); bad.append((t, ns))  # decreasing
        t = good.copy(); t[1] = B + 1; bad.append((t, ns))                # block 0 one span above the bound
        bad.append((np.zeros(1, np.uint64), 0))                           # no block
        bad.append((np.concatenate([np.zeros(1025, np.uint64), [1]]).astype(np.uint64), 1))  # 1025 blocks
        for t, n in bad:
            with pytest.raises(S.SrdError):
                ctx.set_scan_blocks(t, n)
        after = ctx.scan_blocks(S.SCAN_BLOCKS_NEXT)
        assert np.array_equal(before[0], after[0]) and after[1].source == before[1].source == S.SCAN_BLOCKS_MEASURED
        with pytest.raises(S.SrdError):
            off.set_scan_blocks(good, ns)
        # at the bound exactly: accepted (and run)
        t, _ = _sawtooth(g, ns, np.random.default_rng(1))
        assert int(np.diff(t.astype(np.int64)).max()) == B
        small.mutate()
        _call_on(ctx, small, t, g, ns, "at the bound")
        # a table for S16 does not apply to S256
        ctx.set_scan_blocks(t, ns)
        r = S.validate_index_device(big.ptr, big.size, 0, ctx)
        info = ctx.scan_blocks(S.SCAN_BLOCKS_LAST)[1]
        assert info.source == S.SCAN_BLOCKS_EVEN and (info.n_blocks, info.n_spans) != (g, ns)
        _check(r, big, "ignored table")
    finally:
        ctx.close()
        off.close()
