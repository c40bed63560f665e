"""Verified payloads read into a sequence of device segments:
srd_payload_scatter_device (the gather's ranges delivered straight into the
caller's destination segments, in units that are pieces of segments cut at the
destination's 16-byte boundaries, each payload's CRC-32 computed on the way and
compared with its stored checksum -- an EntryStream read, entry_stream.rs:44-92,
plus EntryHandle::is_valid_checksum) and the Python layers over it
(scatter_ranges, DeviceIndex.batch_scatter, DeviceStore.batch_read_into[_hashed_keys]
/ read_into).

The discipline of test_gpu_append / test_gpu_segments: a store is made by the
existing writers (DeviceStore.batch_write / batch_write_stream); expected bytes
come from the host copy of the store and zlib.crc32; every destination
allocation is filled with 0xA5 before a call and compared WHOLE afterwards;
d_status / d_crc_computed are sentinel-filled.  The shapes are the smallest at
which this code can go wrong, C = GATHER_CHUNK."""
import ctypes as C
import zlib

import numpy as np
import pytest

import srd_amd as S

pytestmark = pytest.mark.gpu

CH = S.GATHER_CHUNK
FILL = 0xA5
ST_SENT, CRC_SENT = 0xEE, 0x5A5A5A5A
M64 = (1 << 64) - 1
WAVES_PER_BLOCK = 16  # the streaming kernel's launch line: one block of 16 waves per CU
OK, NONE, BAD_CRC, BAD_RANGE, BAD_LENGTH = S.GATHER_OK, S.GATHER_NONE, S.GATHER_BAD_CRC, S.GATHER_BAD_RANGE, 4
LENS = [0, 1, 15, 16, 17, 31, 32, 33, 4095, 4096, 4097, CH - 1, CH, CH + 1]
UNITS = [63, 64, 65, 127, 128, 130]
ASSORTED = [1, 15, 16, 17, 63, 64, 65, 4095, 4096, 4097, CH - 1, CH, CH + 1, 2 * CH + 17]


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


class Store:
    """A DeviceStore written by batch_write, its host copy, and {key: (start, end)} by the library's look-up."""

    def __init__(self, ctx, ents):
        cap = sum(len(p) + 84 for _, p in ents) + 16384  # (room behind the padded range: a destination of one test)
        self.s = S.DeviceStore.create(cap, ctx)
        self.s.batch_write([k for k, _ in ents], [p for _, p in ents])
        self.f = self.s.bytes()
        self.flen = len(self.f)
        h = S.compute_hash_batch([k for k, _ in ents], ctx)
        st, en = self.s._ranges(h, h)
        self.rg = {k: (int(a), int(b)) for (k, _), a, b in zip(ents, st, en)}
        for k, p in ents:
            a, b = self.rg[k]
            assert self.f[a:b] == p and a % 64 == 0
        self.ptr = self.s.buf.data_ptr()


@pytest.fixture(scope="module")
def store(ctx):
    ents = [(b"p200", rand_bytes(1, 200)), (b"pC200", rand_bytes(2, CH + 200)), (b"pool", rand_bytes(3, 3 * CH + 5000)),
            (b"lens", rand_bytes(4, sum(LENS))), (b"three", rand_bytes(5, 3 * CH))]
    ents += [(b"u%d" % k, rand_bytes(100 + k, (k - 1) * CH + 777)) for k in UNITS]
    ents += [(b"len-%d" % n, rand_bytes(200 + i, n)) for i, n in enumerate(ASSORTED)]
    return Store(ctx, ents)


class Arenas:
    """Destination allocations, all FILL, with their expected images."""

    def __init__(self, sizes=(), tensors=()):
        import torch
        self.t = [torch.full((s,), FILL, dtype=torch.uint8, device="cuda") for s in sizes] + list(tensors)
        self.want = [t.cpu().numpy().copy() for t in self.t]
        for t in self.t:
            assert t.data_ptr() % 16 == 0

    def ptr(self, a, off=0):
        return self.t[a].data_ptr() + off

    def check(self):
        for k, (t, w) in enumerate(zip(self.t, self.want)):
            got = t.cpu().numpy()
            if not np.array_equal(got, w):
                bad = np.flatnonzero(got != w)
                raise AssertionError(f"arena {k}: {bad.size} bytes differ, first at {int(bad[0])}, last at {int(bad[-1])}")


def dev_u64(a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a, np.uint64).view(np.int64)).cuda()


def raw(ctx, d_file, flen, st, en, table, segs, first, flags=0, n=None, n_segs=None, n_dst=None, with_crc=True):
    """One raw srd_payload_scatter_device call with sentinel-filled outputs.
    table: (address, length) pairs; segs: (k, off, len[, reserved]).  (rc, status, crc, message)."""
    import torch
    n = len(st) if n is None else n
    m = max(len(st), 1)
    arr = (S.Segment * max(len(segs), 1))(*[(s[0], s[3] if len(s) > 3 else 0, s[1], s[2]) for s in segs])
    d_segs = torch.from_numpy(np.frombuffer(arr, np.uint8).copy()).cuda()
    d_st, d_en, d_first = dev_u64(st if len(st) else [0]), dev_u64(en if len(en) else [0]), dev_u64(first)
    status = torch.full((m,), ST_SENT, dtype=torch.uint8, device="cuda")
    crc = torch.full((m,), CRC_SENT, dtype=torch.int32, device="cuda")
    k = len(table)
    ptrs = (C.c_void_p * max(k, 1))(*[int(p) for p, _ in table])
    lens = (C.c_uint64 * max(k, 1))(*[int(x) for _, x in table])
    torch.cuda.synchronize()  # the library launches on its own stream, not ordered behind torch's
    rc = S.lib().srd_payload_scatter_device(
        ctx.h, C.c_void_p(d_file), flen, C.c_void_p(d_st.data_ptr()), C.c_void_p(d_en.data_ptr()), n, ptrs, lens,
        k if n_dst is None else n_dst, C.c_void_p(d_segs.data_ptr()), len(segs) if n_segs is None else n_segs,
        C.c_void_p(d_first.data_ptr()), flags, C.c_void_p(status.data_ptr()),
        C.c_void_p(crc.data_ptr()) if with_crc else None, C.c_void_p(ctx.stream))
    msg = S.lib().srd_last_error().decode() if rc else ""
    torch.cuda.synchronize()
    return rc, status.cpu().numpy(), crc.cpu().numpy().view(np.uint32), msg


def expect(f, st, en, segs, first):
    """Per query what the contract says, from the host copy f: (status, crc, payload | None)."""
    out = []
    for i, (s, e) in enumerate(zip(st, en)):
        if s == e:
            out.append((NONE, 0, None))
        elif s > e or e > len(f) or len(f) - e < 20:
            out.append((BAD_RANGE, 0, None))
        elif sum(g[2] for g in segs[first[i]: first[i + 1]]) != e - s:
            out.append((BAD_LENGTH, 0, None))
        else:
            p = f[s:e]
            crc = zlib.crc32(p)
            out.append((OK if crc == int.from_bytes(f[e + 16: e + 20], "little") else BAD_CRC, crc, p))
    return out


def scatter_ok(ctx, d_file, f, st, en, A, tab, segs, first):
    """tab: (arena, offset, length) table ranges.  Calls, and checks statuses, CRCs and every arena whole."""
    want = expect(f, st, en, segs, first)
    for i, (_, _, p) in enumerate(want):
        so = 0
        for k, off, ln in segs[first[i]: first[i + 1]] if p is not None else []:
            a, t0, _ = tab[k]
            A.want[a][t0 + off: t0 + off + ln] = np.frombuffer(p[so: so + ln], np.uint8)
            so += ln
    rc, status, crc, msg = raw(ctx, d_file, len(f), st, en, [(A.ptr(a, o), ln) for a, o, ln in tab], segs, first)
    assert rc == 0, msg
    assert [int(x) for x in status[: len(st)]] == [w[0] for w in want]
    assert [int(x) for x in crc[: len(st)]] == [w[1] for w in want]
    A.check()
    return want


# -- 1. one 16-aligned segment per entry: the gather's own shapes ---------------------------------

def test_one_aligned_segment_per_entry_equals_the_gather(ctx, store):
    keys = [b"p200", b"pC200", b"lens", b"three"] + [b"len-%d" % n for n in ASSORTED]
    st, en = [store.rg[k][0] for k in keys], [store.rg[k][1] for k in keys]
    offs, o = [], 0
    for a, b in zip(st, en):
        offs.append(o)
        o += (b - a + 15) & ~15
    A = Arenas([o + 64])
    segs = [(0, off, b - a) for off, a, b in zip(offs, st, en)]
    want = scatter_ok(ctx, store.ptr, store.f, st, en, A, [(0, 0, o + 64)], segs, list(range(len(keys) + 1)))
    assert all(w[0] == OK for w in want)
    g = S.gather_ranges(store.ptr, store.flen, dev_u64(st), dev_u64(en), 0, ctx)
    assert [int(x) for x in g.status] == [w[0] for w in want] and [int(x) for x in g.crc_computed] == [w[1] for w in want]
    assert g.payloads() == [bytes(A.want[0][off: off + b - a]) for off, a, b in zip(offs, st, en)]


# -- 2. every (destination, source) residue pair --------------------------------------------------

@pytest.mark.parametrize("length", [200, CH + 200])
def test_all_residue_pairs(ctx, store, length):
    """A unit boundary falls on the realigning path for the longer payload; an
    unaligned start is the gather's contract (the range is a piece of an entry:
    the checksum behind it is whatever lies there)."""
    a0 = store.rg[b"pool"][0]
    st, en, segs, o = [], [], [], 0
    for dr in range(16):
        for sr in range(16):
            st.append(a0 + 64 * dr + sr)
            en.append(st[-1] + length)
            o = ((o + 15 + 7) & ~15) + dr  # (at least 7 bytes between neighbours)
            segs.append((0, o, length))
            o += length
    A = Arenas([o + 64])
    want = scatter_ok(ctx, store.ptr, store.f, st, en, A, [(0, 0, o + 64)], segs, list(range(257)))
    assert all(w[0] in (OK, BAD_CRC) for w in want)


# -- 3. segment lengths around 16, 4096 and the chunk; empty segments -----------------------------

def test_segment_lengths_at_two_residues(ctx, store):
    a, b = store.rg[b"lens"]
    tab, segs, first, o = [(0, 0, 0)], [], [0], 0
    for res in (3, 8):
        lens = [0] + LENS[1:8] + [0] + LENS[8:] + [0]  # empty segments first, in the middle and last
        for ln in lens:
            o = ((o + 15 + 16) & ~15) + res
            segs.append((0, o, ln))
            o += ln
        first.append(len(segs))
    A = Arenas([o + 64])
    tab[0] = (0, 0, o + 64)
    want = scatter_ok(ctx, store.ptr, store.f, [a, a], [b, b], A, tab, segs, first)
    assert [w[0] for w in want] == [OK, OK]


# -- 4. entries of 63 .. 130 units: the combine's lane stride -------------------------------------

def test_entries_around_the_combines_lane_stride(ctx, store):
    keys = [b"u%d" % k for k in UNITS]
    st, en = [store.rg[k][0] for k in keys], [store.rg[k][1] for k in keys]
    segs, o = [], 0
    for a, b in zip(st, en):
        segs.append((0, o, b - a))
        o += (b - a + 15) & ~15
    assert [(g[2] + CH - 1) // CH for g in segs] == UNITS
    A = Arenas([o + 64])
    want = scatter_ok(ctx, store.ptr, store.f, st, en, A, [(0, 0, o + 64)], segs, list(range(len(keys) + 1)))
    assert all(w[0] == OK for w in want)


# -- 5. three segments whose boundaries fall at a unit boundary +- 1 ------------------------------

@pytest.mark.parametrize("d", [-1, 1])
def test_three_segments_around_unit_boundaries(ctx, store, d):
    a, b = store.rg[b"three"]
    res = 5  # the first segment's destination residue: its first unit holds CH - res bytes
    l0 = CH - res + d
    l1 = CH + d  # (the second segment starts 16-aligned: its unit boundary is CH behind its start)
    lens = [l0, l1, 3 * CH - l0 - l1]
    segs = [(0, 16 + res, l0), (1, 32, l1), (0, 2 * CH + 9, lens[2])]
    A = Arenas([2 * CH + 9 + lens[2] + 40, 32 + l1 + 40])
    want = scatter_ok(ctx, store.ptr, store.f, [a], [b], A, [(0, 0, A.t[0].numel()), (1, 0, A.t[1].numel())], segs, [0, 3])
    assert want[0][0] == OK


# -- 6. more units than the grid has waves, with small entries ------------------------------------

def test_more_units_than_waves(ctx):
    import torch
    W = WAVES_PER_BLOCK * torch.cuda.get_device_properties(0).multi_processor_count
    n = 2 * W + W // 2 + 3
    rng = np.random.default_rng(0x5CA7)
    ents = [(b"s%d" % i, rand_bytes(1000 + i, int(ln))) for i, ln in enumerate(rng.integers(1, 120, n))]
    sm = Store(ctx, ents)
    st, en = [sm.rg[k][0] for k, _ in ents], [sm.rg[k][1] for k, _ in ents]
    segs, o = [], 5
    for a, b in zip(st, en):
        segs.append((0, o, b - a))
        o += b - a + 3
    A = Arenas([o + 64])
    want = scatter_ok(ctx, sm.ptr, sm.f, st, en, A, [(0, 0, o + 64)], segs, list(range(n + 1)))
    assert all(w[0] == OK for w in want)


# -- 7. the table: several ranges, one arena for many segments, overlaps, another store's buffer --

def test_table_ranges(ctx, store):
    other = S.DeviceStore.create(1 << 16, ctx)  # another store's buffer as a destination
    other.buf.fill_(FILL)
    A = Arenas([CH + 5000, 3000], [other.buf])
    # ranges 0 and 1 overlap inside arena 0; range 2 is arena 1 less its ends; range 3 is empty at NULL
    tab = [(0, 0, CH + 3000), (0, 1000, CH + 4000), (1, 7, 2900), (2, 64, 4096)]
    table = [(A.ptr(a, o), ln) for a, o, ln in tab] + [(0, 0)]
    keys = [b"pC200", b"p200", b"len-4097", b"len-17"]
    st, en = [store.rg[k][0] for k in keys], [store.rg[k][1] for k in keys]
    segs = [(0, 3, 1000), (1, 10, CH - 1000), (1, CH - 990 + 5, 200),  # pC200: arena 0 through both ranges
            (2, 0, 100), (4, 0, 0), (2, 2800, 100),                     # p200: the ends of range 2
            (3, 0, 4096), (1, CH + 3999, 1),                            # len-4097: the other store, range 1's last byte
            (2, 500, 17)]
    first = [0, 3, 6, 8, 9]
    want = expect(store.f, st, en, segs, first)
    for i, (_, _, p) in enumerate(want):
        so = 0
        for k, off, ln in segs[first[i]: first[i + 1]]:
            if ln:
                a, t0, _ = tab[k]
                A.want[a][t0 + off: t0 + off + ln] = np.frombuffer(p[so: so + ln], np.uint8)
            so += ln
    rc, status, crc, msg = raw(ctx, store.ptr, store.flen, st, en, table, segs, first)
    assert rc == 0, msg
    assert [int(x) for x in status] == [OK] * 4 and [int(x) for x in crc] == [w[1] for w in want]
    A.check()


# -- 8. one batch of every status ------------------------------------------------------------------

def test_mixed_statuses(ctx, store):
    import torch
    d = store.s.buf.clone()  # a copy with one flipped payload byte
    f = bytearray(store.f)
    a2, b2 = store.rg[b"len-4097"]
    f[a2 + 4000] ^= 0x40
    d[a2 + 4000] = f[a2 + 4000]
    f = bytes(f)
    torch.cuda.synchronize()
    rg = store.rg
    q = [rg[b"p200"], (77, 77), (rg[b"p200"][1], rg[b"p200"][0]), rg[b"len-17"], rg[b"len-65"], (a2, b2),
         (store.flen - 30, store.flen - 10), rg[b"pC200"], (M64, M64)]
    st, en = [x[0] for x in q], [x[1] for x in q]
    segs = [(0, 16, 150), (0, 200, 50),          # OK in two pieces
            (0, 300, 40),                        # NONE: ignored
            (0, 400, 200),                       # BAD_RANGE (start > end)
            (0, 700, 16),                        # BAD_LENGTH, one short
            (0, 800, 60), (0, 900, 6),           # BAD_LENGTH, one over
            (0, 1001, 4097),                     # BAD_CRC: delivered as the bytes lie
            (0, 6000, 10),                       # BAD_RANGE (metadata past the end)
            (0, 6100, CH), (0, 6100 + CH + 1, 200)]  # OK, two units
    first = [0, 2, 3, 4, 5, 7, 8, 9, 11, 11]
    A = Arenas([6100 + CH + 300])
    want = scatter_ok(ctx, d.data_ptr(), f, st, en, A, [(0, 0, A.t[0].numel())], segs, first)
    assert [w[0] for w in want] == [OK, NONE, BAD_RANGE, BAD_LENGTH, BAD_LENGTH, BAD_CRC, BAD_RANGE, OK, NONE]
    assert want[5][1] == zlib.crc32(f[a2:b2]) != int.from_bytes(f[b2 + 16: b2 + 20], "little")
    # without d_crc_computed: the same bytes and statuses
    A2 = Arenas([A.t[0].numel()])
    rc, status, crc, msg = raw(ctx, d.data_ptr(), len(f), st, en, [(A2.ptr(0), A2.t[0].numel())], segs, first, with_crc=False)
    assert rc == 0 and [int(x) for x in status] == [w[0] for w in want] and all(int(x) == CRC_SENT for x in crc)
    assert np.array_equal(A2.t[0].cpu().numpy(), A.want[0])


# -- 9. refusals: SRD_ERR_ARG, nothing written anywhere --------------------------------------------

def test_refusals(ctx, store):
    a, b = store.rg[b"p200"]
    A = Arenas([4096, 4096])
    table = [(A.ptr(0), 4096), (A.ptr(1), 1000), (0, 0)]
    ok = (0, 0, 200)

    def refused(needle, st, en, segs, first, table=table, **kw):
        rc, status, crc, msg = raw(ctx, kw.pop("d_file", store.ptr), kw.pop("flen", store.flen), st, en, table, segs, first, **kw)
        assert rc == S.SRD_ERR_ARG and needle in msg, (rc, msg)
        assert all(int(x) == ST_SENT for x in status) and all(int(x) == CRC_SENT for x in crc)
        A.check()

    def three(bad_seg, i=1):  # three queries, the i-th with the bad segment
        segs = [ok, ok, ok]
        segs[i] = bad_seg
        return [a] * 3, [b] * 3, segs, [0, 1, 2, 3]

    # malformed segments: never dereferenced, the message names the query
    for g in [(3, 0, 200), (0xFFFFFFFF, 0, 200), (0, 0, 200, 1), (1, 801, 200), (1, 1001, 0), (2, 0, 1), (0, M64, 1),
              (0, M64 - 7, 208), (0, 8, M64 - 7), (0, 100, M64), (0, 1 << 63, 1 << 63)]:
        refused("query 1 has a malformed segment", *three(g))
    # ... whatever the query's status would be: a None, a bad range, a wrong length
    refused("query 0 has a malformed segment", [5], [5], [(7, 0, 0)], [0, 1])
    refused("query 0 has a malformed segment", [9], [5], [(1, 999, 2)], [0, 1])
    refused("query 0 has a malformed segment", [a], [b], [(0, 0, 500), (1, 999, 2)], [0, 2])
    # the first refused query decides
    refused("query 1 has a malformed segment", [a] * 4, [b] * 4, [ok, (5, 0, 1), (0, 0, 200, 7), ok], [0, 1, 2, 3, 4])
    refused("d_seg_first is malformed at query 1", [a] * 3, [b] * 3, [ok, ok, (5, 0, 1)], [0, 2, 1, 3])
    # d_seg_first
    refused("d_seg_first is malformed at query 0", [a, a], [b, b], [ok, ok], [1, 2, 2])
    refused("d_seg_first is malformed at query 0", [a], [b], [ok, ok], [0, 1])
    refused("d_seg_first is malformed at query 1", [a, a], [b, b], [ok, ok], [0, 1, 3])
    refused("d_seg_first is malformed at query 0", [a, a], [b, b], [ok, ok], [0, M64, 2])
    # what the host decides before anything runs
    refused("flags must be 0", [a], [b], [ok], [0, 1], flags=1)
    refused("too many queries", [a], [b], [ok], [0, 1], n=1 << 31)
    refused("too many segments", [a], [b], [ok], [0, 1], n_segs=1 << 31)
    refused("too many destinations", [a], [b], [ok], [0, 1], n_dst=1 << 32)
    refused("destination 1 is NULL", [a], [b], [ok], [0, 1], table=[(A.ptr(0), 4096), (0, 8)])
    # 2^32 work units: a file and a table range of 2^48 bytes at addresses where nothing lies; the refusal comes
    # from the layout's counts alone, neither is ever touched
    big = 1 << 48
    refused("too many work units", [0], [big], [(0, 0, big)], [0, 1], table=[(1 << 52, big)], d_file=1 << 56, flen=big + 20)


def test_destination_inside_the_store_is_refused(ctx, store):
    a, b = store.rg[b"p200"]
    A = Arenas([4096])
    padded = S.padded_size(store.flen)
    assert store.s.buf.numel() > padded + 4096  # (room behind the padded range inside the same allocation)
    before = store.s.buf.cpu().numpy().copy()
    for p, ln in [(store.ptr, 4096), (store.ptr + padded - 1, 4096), (store.ptr + store.flen, 1),
                  (store.ptr - 64, 65), (store.ptr - 64, M64)]:
        rc, status, crc, msg = raw(ctx, store.ptr, store.flen, [a], [b], [(A.ptr(0), 4096), (p, ln)], [(0, 0, 200)], [0, 1])
        assert rc == S.SRD_ERR_ARG and "destination 1 overlaps the store" in msg, (rc, msg)
        assert int(status[0]) == ST_SENT and int(crc[0]) == CRC_SENT
    A.check()
    # directly behind the padded range the same allocation is a destination like any other
    rc, status, crc, msg = raw(ctx, store.ptr, store.flen, [a], [b], [(store.ptr + padded, 4096)], [(0, 3, 200)], [0, 1])
    assert rc == 0 and int(status[0]) == OK, msg
    after = store.s.buf.cpu().numpy()
    assert after[padded + 3: padded + 203].tobytes() == store.f[a:b]
    after[padded + 3: padded + 203] = before[padded + 3: padded + 203]
    assert np.array_equal(after, before)
    store.s.buf[padded: padded + 4096] = 0  # (as DeviceStore.create left it)


def test_no_queries_runs_nothing(ctx, store):
    A = Arenas([256])
    rc, status, crc, msg = raw(ctx, store.ptr, store.flen, [], [], [(A.ptr(0), 256)], [], [0])
    assert rc == 0 and int(status[0]) == ST_SENT and int(crc[0]) == CRC_SENT
    A.check()


# -- 10. a session: write in pieces, read back in pieces ------------------------------------------

def test_session_round_trip(ctx):
    import torch
    g = torch.Generator(device="cpu").manual_seed(0x5E55)

    def piece(shape, dtype, residue):
        """A tensor at an address = residue mod 16 (a slice of a byte allocation viewed as dtype)."""
        nb = int(np.prod(shape)) * torch.empty(0, dtype=dtype).element_size()
        raw_ = torch.full((nb + 64,), FILL, dtype=torch.uint8, device="cuda")
        t = raw_[residue: residue + nb].view(dtype).view(shape)
        assert (not nb or t.data_ptr() == raw_.data_ptr() + residue) and raw_.data_ptr() % 16 == 0 and t.is_contiguous()
        return raw_, t

    def fill(t):
        nb = t.numel() * t.element_size()
        t.view(torch.uint8).reshape(-1).copy_(torch.randint(1, 256, (nb,), dtype=torch.uint8, generator=g))

    shapes = [[((24,), torch.uint8, 1), ((33, 7), torch.float32, 4), ((0,), torch.float16, 2)],
              [((5,), torch.int64, 8), ((CH + 300,), torch.uint8, 3)],
              [((129, 3), torch.float16, 6)]]
    keys = [b"k0", b"k1", b"k2"]
    src = [[piece(*s) for s in ent] for ent in shapes]
    for ent in src:
        for _, t in ent:
            fill(t)
    s = S.DeviceStore.create(1 << 20, ctx)
    s.batch_write_stream(keys, [[t for _, t in ent] for ent in src])

    def read_back(store_, ks):
        dst = [[piece(*sh) for sh in ent] for ent in shapes]
        r = store_.batch_read_into(ks, [[t for _, t in ent] for ent in dst])
        return dst, r

    def same(dst):
        for e_src, e_dst in zip(src, dst):
            for (_, a), (rw, b) in zip(e_src, e_dst):
                assert a.dtype == b.dtype and a.shape == b.shape and torch.equal(a.view(torch.uint8), b.view(torch.uint8))
                w = np.full(rw.numel(), FILL, np.uint8)  # the allocation whole: nothing around the tensor is touched
                nb = b.numel() * b.element_size()
                if nb:
                    res = b.data_ptr() - rw.data_ptr()
                    w[res: res + nb] = a.view(torch.uint8).reshape(-1).cpu().numpy()
                assert np.array_equal(rw.cpu().numpy(), w)

    dst, r = read_back(s, keys)
    assert [int(x) for x in r.status] == [OK] * 3 and r.is_valid_checksum() == [True] * 3
    host = s.bytes()
    h = S.compute_hash_batch(keys, ctx)
    assert [int(x) for x in r.crc_computed] == [zlib.crc32(host[int(a):int(b)]) for a, b in zip(*s._ranges(h, h))]
    same(dst)
    # a missing key: NONE, its tensors intact; a wrong-size tensor: BAD_LENGTH, intact
    raw0, t0 = piece((40,), torch.uint8, 5)
    raw1, t1 = piece((23,), torch.uint8, 9)
    raw2, t2 = piece((129, 3), torch.float16, 6)
    r = s.batch_read_into([b"nope", b"k0", b"k2"], [[t0], [t1], [t2]])
    assert [int(x) for x in r.status] == [NONE, BAD_LENGTH, OK]
    assert bool((raw0 == FILL).all()) and bool((raw1 == FILL).all())
    assert torch.equal(t2.view(torch.uint8), src[2][0][1].view(torch.uint8))
    with pytest.raises(ValueError):
        r.is_valid_checksum()
    assert s.read_into(b"k2", [t2]) == OK and s.read_into(b"nope", [t0]) == NONE
    # the ValueErrors come before any call; a tensor inside the store is the library's refusal
    with pytest.raises(ValueError):
        s.batch_read_into([b"k0"], [t1])
    with pytest.raises(ValueError):
        s.batch_read_into([b"k0"], [[t1.cpu()]])
    with pytest.raises(ValueError):
        s.batch_read_into([b"k0", b"k1"], [[t1]])
    with pytest.raises(S.SrdError):
        s.batch_read_into([b"k0"], [[s.buf[64:88]]])
    # directly behind a torch write to the store on the null stream: the call sees it
    a0 = int(s._ranges(h[:1], h[:1])[0][0])
    s.buf[a0 + 2] ^= 0xFF
    raw3, t3 = piece((24,), torch.uint8, 1)
    rawf, tf = piece((33, 7), torch.float32, 4)
    r = s.batch_read_into([b"k0"], [[t3, tf, src[0][2][1]]])
    flipped = bytearray(host[a0: a0 + 24 + 33 * 7 * 4])
    flipped[2] ^= 0xFF
    assert int(r.status[0]) == BAD_CRC and int(r.crc_computed[0]) == zlib.crc32(bytes(flipped))
    assert bytes(t3.cpu().numpy()) == bytes(flipped[:24]) and r.is_valid_checksum() == [False]
    s.buf[a0 + 2] ^= 0xFF
    # the same after compact
    s.batch_write([b"k1"], [b"dead space"])
    s.batch_write_stream([b"k1"], [[t for _, t in src[1]]])
    s.compact()
    dst, r = read_back(s, keys)
    assert [int(x) for x in r.status] == [OK] * 3
    same(dst)
