"""Keyed reads into fixed-size rows with no host wait: srd_read_rows_device (the
look-up of a batch read, the verified copy of the gather and a destination
known by arithmetic -- query i goes to row i of the caller's [n, row_stride]
buffer -- with the unit count kept on the device) and the Python layers over it
(DeviceIndex.read_rows, DeviceStore.batch_read_rows[_hashed_keys], reserve_rows,
sync, rows_token, RowsResult).

The discipline of test_gpu_scatter: stores are made by the existing writers;
expectations come from the host copy of the payloads and zlib.crc32 and are
cross-checked against batch_gather_hashed_keys; `out` is filled with 0xA5 and
compared WHOLE (its padding columns included); lens / status / crc / counts are
sentinel-filled and compared whole.  The shapes are the smallest at which this
code can go wrong, C = GATHER_CHUNK."""
import ctypes as C
import zlib

import numpy as np
import pytest

import srd_amd as S

pytestmark = pytest.mark.gpu

CH = S.GATHER_CHUNK
FILL = 0xA5
ST_SENT, CRC_SENT, LEN_SENT, CNT_SENT = 0xEE, 0x5A5A5A5A, 0x5B5B5B5B5B5B5B5B, 0x5C5C5C5C5C5C5C5C
WAVES_PER_BLOCK = 16  # the streaming kernel's launch line: one block of 16 waves per CU
OK, NONE, BAD_CRC, TOO_LONG = S.GATHER_OK, S.GATHER_NONE, S.GATHER_BAD_CRC, S.ROWS_TOO_LONG
ASSORTED = [1, 15, 16, 17, 63, 64, 65, 4095, 4096, 4097, CH - 1, CH, CH + 1, 2 * CH + 17]
UNITS = [63, 64, 65, 130]


@pytest.fixture(scope="module")
def ctx():
    c = S.Context(0)
    yield c
    c.close()


def rand_bytes(seed, n):
    """n random bytes, the first not 0."""
    b = bytearray(np.random.default_rng(seed).bytes(n))
    b[0] |= 1
    return bytes(b)


def make_store(ctx, ents, room=1 << 16):
    s = S.DeviceStore.create(sum(len(p) + 84 for _, p in ents) + room, ctx)
    s.batch_write([k for k, _ in ents], [p for _, p in ents])
    return s


@pytest.fixture(scope="module")
def store(ctx):
    """(session, {key: payload}) of the assorted lengths."""
    ents = [(b"len-%d" % n, rand_bytes(200 + i, n)) for i, n in enumerate(ASSORTED)]
    return make_store(ctx, ents), dict(ents)


def want_of(payload, row_cap, bad=False):
    """What the contract says of one query whose entry holds `payload` (None: no entry): (status, length, crc, bytes | None)."""
    if payload is None:
        return (NONE, 0, 0, None)
    if len(payload) > row_cap:
        return (TOO_LONG, len(payload), 0, None)
    return (BAD_CRC if bad else OK, len(payload), zlib.crc32(payload), payload)


class Outs:
    """The caller's tensors of one read, sentinel-filled: out is the first row_cap columns of a [n, stride] buffer."""

    def __init__(self, n, row_cap, stride):
        import torch
        self.base = torch.full((max(n, 1), stride), FILL, dtype=torch.uint8, device="cuda")[:n]
        self.out = self.base[:, :row_cap]
        self.lens = torch.full((n,), LEN_SENT, dtype=torch.int64, device="cuda")
        self.status = torch.full((n,), ST_SENT, dtype=torch.uint8, device="cuda")
        self.crc = torch.full((n,), CRC_SENT, dtype=torch.int32, device="cuda")
        self.counts = torch.full((6,), CNT_SENT, dtype=torch.int64, device="cuda")
        assert self.out.data_ptr() % 16 == 0 and (n < 2 or self.out.stride(0) == stride)

    def kw(self):
        return dict(lens=self.lens, status=self.status, crc=self.crc, counts=self.counts)

    def refill(self):
        self.base.fill_(FILL)
        self.lens.fill_(LEN_SENT)
        self.status.fill_(ST_SENT)
        self.crc.fill_(CRC_SENT)
        self.counts.fill_(CNT_SENT)

    def check(self, want):
        """Every output whole against want = [(status, length, crc, bytes | None)]."""
        import torch
        torch.cuda.synchronize()
        n = len(want)
        img = np.full(tuple(self.base.shape), FILL, np.uint8)
        for i, (_, _, _, p) in enumerate(want):
            if p is not None:
                img[i, : len(p)] = np.frombuffer(p, np.uint8)
        got = self.base.cpu().numpy()
        if not np.array_equal(got, img):
            bad = np.argwhere(got != img)
            raise AssertionError(f"out: {len(bad)} bytes differ, first at {tuple(bad[0])}, last at {tuple(bad[-1])}")
        assert [int(x) for x in self.status.cpu().numpy()] == [w[0] for w in want]
        assert [int(x) for x in self.lens.cpu().numpy()] == [w[1] for w in want]
        assert [int(x) for x in self.crc.cpu().numpy().view(np.uint32)] == [w[2] for w in want]
        hist = [sum(1 for w in want if w[0] == k) for k in range(6)]
        assert [int(x) for x in self.counts.cpu().numpy()] == hist and sum(hist) == n


def read_ok(s, hashes, want, row_cap, stride, non_hashed_keys=None):
    """One batch_read_rows_hashed_keys with fresh outputs, checked whole and against the gather."""
    o = Outs(len(hashes), row_cap, stride)
    r = s.batch_read_rows_hashed_keys(hashes, o.out, non_hashed_keys, **o.kw())
    o.check(want)
    g = s.batch_gather_hashed_keys(hashes, non_hashed_keys)
    gp = g.payloads()
    for i, w in enumerate(want):  # the gather delivers what does not fit a row too; everything else agrees
        if w[0] == TOO_LONG:
            assert int(g.status[i]) in (OK, BAD_CRC) and len(gp[i]) == w[1]
        else:
            assert (int(g.status[i]), int(g.crc_computed[i]), gp[i]) == (w[0], w[2], w[3])
    assert r.payloads() == [w[3] for w in want]
    assert r.is_valid_checksum() == [True if w[0] == OK else False if w[0] == BAD_CRC else None for w in want]
    assert r.too_long() == [(i, w[1]) for i, w in enumerate(want) if w[0] == TOO_LONG] and len(r) == len(want)
    return o


# -- 1. lengths against row capacities ------------------------------------------------------------

@pytest.mark.parametrize("extra", [0, 16])
@pytest.mark.parametrize("row_cap", [64, 4112, CH, CH + 16, 3 * CH + 48])
def test_lengths_by_the_rule(ctx, store, row_cap, extra):
    """Every row is delivered or TOO_LONG exactly by the rule; TOO_LONG rows report the true length and stay 0xA5."""
    s, pay = store
    keys = list(pay)
    h = S.compute_hash_batch(keys, ctx)
    want = [want_of(pay[k], row_cap) for k in keys]
    assert {w[0] for w in want} == ({OK, TOO_LONG} if row_cap < 2 * CH + 17 else {OK})
    read_ok(s, h, want, row_cap, row_cap + extra)


# -- 2. batch sizes, keys listed twice and three times --------------------------------------------

@pytest.mark.parametrize("n", [1, 63, 64, 65, 257])
def test_batch_sizes_with_repeated_keys(ctx, store, n):
    s, pay = store
    keys = [k for k in pay if len(pay[k]) <= 4097]
    q = [keys[(7 * i) % len(keys)] for i in range(n)]  # (n > len(keys): every key twice or more)
    want = [want_of(pay[k], 4112) for k in q]
    read_ok(s, S.compute_hash_batch(q, ctx), want, 4112, 4112 + 16 * (n & 1))


def test_more_units_than_waves(ctx):
    import torch
    W = WAVES_PER_BLOCK * torch.cuda.get_device_properties(0).multi_processor_count
    n = 2 * W + W // 2 + 3
    rng = np.random.default_rng(0x5CA8)
    ents = [(b"s%d" % i, rand_bytes(1000 + i, int(ln))) for i, ln in enumerate(rng.integers(1, 120, n))]
    s = make_store(ctx, ents)
    o = Outs(n, 112, 128)
    s.batch_read_rows_hashed_keys(S.compute_hash_batch([k for k, _ in ents], ctx), o.out, **o.kw())
    want = [want_of(p, 112) for _, p in ents]
    assert {w[0] for w in want} == {OK, TOO_LONG}
    o.check(want)


# -- 3. entries around the combine's lane stride ---------------------------------------------------

def test_rows_of_many_units(ctx):
    ents = [(b"u%d" % k, rand_bytes(100 + k, (k - 1) * CH + 777)) for k in UNITS]
    s = make_store(ctx, ents)
    keys = [k for k, _ in ents] + [b"u64", b"nobody"]
    pay = dict(ents)
    row_cap = 130 * CH
    want = [want_of(pay.get(k), row_cap) for k in keys]
    read_ok(s, S.compute_hash_batch(keys, ctx), want, row_cap, row_cap + 16)
    # ... and one unit short of the longest: that row alone is TOO_LONG
    row_cap = 129 * CH
    want = [want_of(pay.get(k), row_cap) for k in keys]
    assert [w[0] for w in want] == [OK, OK, OK, TOO_LONG, OK, NONE]
    read_ok(s, S.compute_hash_batch(keys, ctx), want, row_cap, row_cap)


# -- 4. mixed statuses in one batch ----------------------------------------------------------------

def test_mixed_statuses_and_counts(ctx):
    import torch
    ents = [(b"k%d" % i, rand_bytes(300 + i, ln)) for i, ln in enumerate([100, 5000, CH + 9, 64, 2000, 77, 31])]
    s0 = make_store(ctx, ents)
    s0.batch_delete([b"k3"])  # a tombstone on disk
    s = S.DeviceStore.open(s0.buf.clone(), s0.tail, ctx)  # re-opened: the index holds the tombstone's key
    s.batch_delete([b"k5"])  # deleted in the session: removed from the table
    pay = dict(ents)
    a = s._ranges(S.compute_hash_batch([b"k4"], ctx), None)[0]
    flip = int(a[0]) + 1234
    s.buf[flip] ^= 0x40  # a flipped payload byte: delivered, BAD_CRC
    bad = bytearray(pay[b"k4"])
    bad[1234] ^= 0x40
    keys = [b"k0", b"absent", b"k5", b"k3", b"k1", b"k4", b"k2", b"k6", b"k0"]
    other = [b"k0", b"absent", b"k5", b"k3", b"not-k1", b"k4", b"k2", b"k6", b"k0"]
    h, hv = S.compute_hash_batch(keys, ctx), S.compute_hash_batch(other, ctx)
    assert h[4] >> 48 != hv[4] >> 48  # (tag_from_key differs: the read is refused)
    row_cap = CH + 16
    want = [want_of(pay[b"k0"], row_cap), want_of(None, row_cap), want_of(None, row_cap), want_of(None, row_cap),
            want_of(None, row_cap), want_of(bytes(bad), row_cap, bad=True), want_of(pay[b"k2"], row_cap),
            want_of(pay[b"k6"], row_cap), want_of(pay[b"k0"], row_cap)]
    o = read_ok(s, h, want, row_cap, row_cap + 16, non_hashed_keys=other)
    assert [int(x) for x in o.counts.cpu().numpy()] == [4, 4, 1, 0, 0, 0]
    # without the verification the mismatched key is read; a smaller row makes two of them TOO_LONG
    want2 = [want_of(pay[b"k0"], 4096), want_of(None, 0), want_of(None, 0), want_of(None, 0), want_of(pay[b"k1"], 4096),
             want_of(bytes(bad), 4096, bad=True), want_of(pay[b"k2"], 4096), want_of(pay[b"k6"], 4096),
             want_of(pay[b"k0"], 4096)]
    o = read_ok(s, torch.from_numpy(np.array(h, np.uint64).view(np.int64)).cuda(), want2, 4096, 4096)
    assert [int(x) for x in o.counts.cpu().numpy()] == [3, 3, 1, 0, 0, 2]


# -- 5. the empty device count ----------------------------------------------------------------------

@pytest.mark.parametrize("row_cap", [64, CH + 16])
def test_nothing_to_deliver(ctx, store, row_cap):
    """Only absent keys, then only TOO_LONG rows: the unit total on the device is 0, every unit kernel leaves at
    once (a row_cap above C also launches terms and combine); nothing is written and all outputs are right."""
    s, pay = store
    absent = [b"none-%d" % i for i in range(70)]
    read_ok(s, S.compute_hash_batch(absent, ctx), [want_of(None, row_cap)] * 70, row_cap, row_cap + 16)
    long_keys = [k for k in pay if len(pay[k]) > row_cap] * 3
    want = [want_of(pay[k], row_cap) for k in long_keys]
    assert want and all(w[0] == TOO_LONG for w in want)
    read_ok(s, S.compute_hash_batch(long_keys, ctx), want, row_cap, row_cap)


# -- 6. refusals -----------------------------------------------------------------------------------

def test_refusals_by_message(ctx, store):
    import torch
    s, pay = store
    n = 4
    o = Outs(n, 64, 64)
    h = torch.zeros(n, dtype=torch.int64, device="cuda")
    flen = s._rows_file_len()
    torch.cuda.synchronize()

    def call(out=o.out.data_ptr(), n=n, stride=64, cap=64, flags=0, table=s.index.table.data_ptr(), hashes=h.data_ptr(),
             lens=o.lens.data_ptr(), status=o.status.data_ptr(), file=s.buf.data_ptr()):
        p = lambda x: C.c_void_p(x) if x else None
        rc = S.lib().srd_read_rows_device(ctx.h, p(table), s.index.nbytes, p(file), flen, p(hashes), None, n, p(out), stride,
                                          cap, p(lens), p(status), p(o.crc.data_ptr()), p(o.counts.data_ptr()), flags,
                                          C.c_void_p(ctx.stream))
        return rc, S.lib().srd_last_error().decode() if rc else ""

    ARG = -3
    for kw, msg in [(dict(out=o.out.data_ptr() + 8), "16-byte aligned"), (dict(stride=72), "multiple of 16"),
                    (dict(stride=48), "below row_cap"), (dict(cap=0), "row_cap"), (dict(n=1 << 31), "too many queries"),
                    (dict(n=1 << 20, stride=CH << 12, cap=CH << 12), "work units"),
                    (dict(n=1 << 30, stride=1 << 40, cap=16), "does not fit 64 bits"), (dict(flags=1), "flags"),
                    (dict(hashes=0), "NULL"), (dict(lens=0), "NULL"), (dict(status=0), "NULL"), (dict(out=0), "NULL"),
                    (dict(table=0), "NULL"), (dict(out=s.buf.data_ptr() + 4096), "overlaps the store"),
                    (dict(out=s.buf.data_ptr() + S.padded_size(flen) - 16), "overlaps the store"),
                    (dict(out=s.buf.data_ptr() - 64 * n + 16), "overlaps the store")]:
        rc, why = call(**kw)
        assert rc == ARG and msg in why, (kw, rc, why)
    assert call(n=0, flags=1)[0] == ARG  # (flags are judged whatever n is)
    assert call(n=0, out=0, hashes=0, lens=0, status=0, cap=0, stride=7) == (0, "")  # n == 0 runs nothing
    torch.cuda.synchronize()  # ... and no refused call has written anything
    assert int(o.status.cpu()[0]) == ST_SENT and int(o.counts.cpu()[0]) == CNT_SENT and bool((o.base == FILL).all())
    # through the session: rows inside the store's own buffer, tensors of the wrong kind, n == 0
    with pytest.raises(S.SrdError, match="overlaps the store"):
        s.batch_read_rows_hashed_keys(h, s.buf[4096: 4096 + 64 * n].view(n, 64))
    with pytest.raises(ValueError):
        s.batch_read_rows_hashed_keys(h, o.out.view(-1))
    with pytest.raises(ValueError):
        s.batch_read_rows_hashed_keys(h[:3], o.out)
    with pytest.raises(ValueError):
        s.batch_read_rows_hashed_keys(h, o.out, lens=o.status)
    r = s.batch_read_rows_hashed_keys([], torch.empty((0, 64), dtype=torch.uint8, device="cuda"))
    assert len(r) == 0 and r.payloads() == [] and s.batch_read_rows([], o.out[:0]).is_valid_checksum() == []


# -- 7. no host wait: the read captured into a graph and replayed -----------------------------------

def test_captured_read_replays_against_the_live_session(ctx):
    import torch
    lens0 = [1, 17, 64, 100, 4095, 4096, 4097, CH, CH + 1, 333] + [50 + i for i in range(70)]
    ents = [(b"g%d" % i, rand_bytes(500 + i, ln)) for i, ln in enumerate(lens0)]
    s = make_store(ctx, ents, room=1 << 20)
    s.index.grow(1024)  # room in the table for the writes below: rows_token() must not change
    pay = dict(ents)
    n, row_cap = 65, CH + 16
    keys = [b"g%d" % (i % 75) for i in range(n - 2)] + [b"missing", b"g8"]
    d_h = torch.from_numpy(np.array(S.compute_hash_batch(keys, ctx), np.uint64).view(np.int64)).cuda()
    o = Outs(n, row_cap, row_cap + 16)
    s.reserve_rows(n, row_cap)
    s.sync()
    token = s.rows_token()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):  # one stream, one chain
        s.batch_read_rows_hashed_keys(d_h, o.out, **o.kw())
    o.refill()
    g.replay()
    want = [want_of(pay.get(k), row_cap) for k in keys]
    o.check(want)
    fresh = s.batch_gather_hashed_keys(S.compute_hash_batch(keys, ctx))
    assert fresh.payloads() == [w[3] for w in want] and [int(x) for x in fresh.status] == [w[0] for w in want]
    # other keys in the same tensor, new entries, an overwrite and a delete: the same graph sees them
    new = [(b"new%d" % i, rand_bytes(900 + i, ln)) for i, ln in enumerate([5, 4096, CH + 7, 70000])] + \
          [(b"g3", rand_bytes(990, 4000))]
    s.batch_write([k for k, _ in new], [p for _, p in new])
    s.batch_delete([b"g5"])
    pay.update(new)
    pay[b"g5"] = None
    assert s.rows_token() == token
    keys2 = [b"new0", b"new1", b"new2", b"new3", b"g3", b"g5", b"g0"] + [b"g%d" % (79 - i) for i in range(n - 7)]
    d_h.copy_(torch.from_numpy(np.array(S.compute_hash_batch(keys2, ctx), np.uint64).view(np.int64)))
    s.sync()
    o.refill()
    g.replay()
    want2 = [want_of(pay.get(k), row_cap) for k in keys2]
    assert [w[0] for w in want2[:7]] == [OK, OK, OK, TOO_LONG, OK, NONE, OK]
    o.check(want2)
    r = S.RowsResult(o.out, o.lens, o.status, o.crc, o.counts)
    assert r.payloads() == [w[3] for w in want2] and r.too_long() == [(3, 70000)]


def test_capture_without_reserve_is_refused():
    import torch
    c2 = S.Context(0)
    try:
        ents = [(b"c%d" % i, rand_bytes(700 + i, 40 + i % 20)) for i in range(200)]
        s = make_store(c2, ents)
        d_h = torch.from_numpy(np.array(S.compute_hash_batch([k for k, _ in ents], c2), np.uint64).view(np.int64)).cuda()
        o = Outs(200, 64, 64)
        read = lambda: s.batch_read_rows_hashed_keys(d_h, o.out, **o.kw())
        want = [want_of(p, 64) for _, p in ents]
        s.reserve_rows(8, 64)  # smaller than the read: it would have to grow
        before = c2.device_bytes()
        s.sync()
        g = torch.cuda.CUDAGraph()
        with pytest.raises(S.SrdError, match="srd_ctx_reserve_rows"):
            with torch.cuda.graph(g):
                read()
        torch.cuda.synchronize()
        assert c2.device_bytes() == before
        assert bool((o.base == FILL).all()) and bool((o.status == ST_SENT).all()) and bool((o.counts == CNT_SENT).all())
        # outside a capture the same call grows the workspace; after that the capture goes through
        read()
        o.check(want)
        assert c2.device_bytes() > before
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g):
            read()
        o.refill()
        g.replay()
        o.check(want)
    finally:
        c2.close()


# -- 8. the session round trip ----------------------------------------------------------------------

def test_session_round_trip(ctx):
    row_cap = 4096
    model = {b"a": rand_bytes(1, 10), b"b": rand_bytes(2, 4096), b"c": rand_bytes(3, 4097), b"d": rand_bytes(4, 777)}
    s = make_store(ctx, list(model.items()))
    keys = [b"a", b"b", b"c", b"d", b"e", b"a"]

    def check():
        o = Outs(len(keys), row_cap, row_cap)
        r = s.batch_read_rows(keys, o.out)
        want = [want_of(model.get(k), row_cap) for k in keys]
        assert r.payloads() == [w[3] for w in want]
        assert [int(x) for x in r.status.cpu().numpy()] == [w[0] for w in want]
        assert [int(x) for x in r.lens.cpu().numpy()] == [w[1] for w in want]
        assert r.too_long() == [(i, w[1]) for i, w in enumerate(want) if w[0] == TOO_LONG]
        img = np.full((len(keys), row_cap), FILL, np.uint8)
        for i, w in enumerate(want):
            if w[3] is not None:
                img[i, : w[1]] = np.frombuffer(w[3], np.uint8)
        assert np.array_equal(o.base.cpu().numpy(), img)

    check()
    model[b"a"], model[b"e"] = rand_bytes(5, 3000), rand_bytes(6, 1)
    s.batch_write([b"a", b"e"], [model[b"a"], model[b"e"]])
    check()
    s.batch_delete([b"b"])
    model[b"b"] = None
    check()
    s.compact()
    check()
