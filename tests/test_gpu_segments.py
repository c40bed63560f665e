"""Entries whose payload is a sequence of device segments:
srd_batch_append_segments_device (the table judged and the entries laid out on
the device, the bytes moved in units that are pieces of segments with their
CRC-32 computed on the way, whole 16-byte vectors of the store at any source
and destination alignment) and the Python layers over it (DeviceStore.
batch_write_stream[_with_key_hashes], write_stream[_with_key_hash]).

test_gpu_append's discipline: expected bytes come from the oracle
(O.write_entries over the host concatenation of each entry's segments); every
comparison is bit-exact and covers the whole allocation: the buffer is 0xA5
beyond the tail before a call, and afterwards [0, new_tail) is the oracle's
store, [new_tail, roundup64(new_tail)) is 0xA5 or 0, and everything behind is
still 0xA5; d_meta_off_out is sentinel-filled.  The shapes are the smallest at
which this code can go wrong, C = GATHER_CHUNK."""
import ctypes as C
import random

import numpy as np
import pytest

import oracle as O
import srd_amd as S
import test_chunk_unit_batches as U
import test_gpu_append as A

pytestmark = pytest.mark.gpu

CH = S.GATHER_CHUNK
SENTINEL = A.SENTINEL
NULL_ONLY = "NULL-byte-only streams cannot be written directly."
EMPTY = "Payload cannot be empty."
M64 = (1 << 64) - 1
kh, pad64, Dev, nonzero_bytes = A.kh, A.pad64, A.Dev, A.nonzero_bytes


@pytest.fixture(scope="module")
def ctx():
    c = S.Context(0)
    yield c
    c.close()


@pytest.fixture(scope="module")
def W():
    """The waves of the streaming kernel's grid once a batch has a unit for each (as tests/test_gpu_chunk_units.py)."""
    import torch
    return U.WAVES_PER_BLOCK * torch.cuda.get_device_properties(0).multi_processor_count


def place(data: bytes, residue=0):
    """The bytes in an allocation of their own, at an address = residue mod 16."""
    import torch
    base = torch.full((len(data) + 32,), 0xEE, dtype=torch.uint8, device="cuda")
    t = base[residue: residue + len(data)]
    if data:
        t.copy_(torch.frombuffer(bytearray(data), dtype=torch.uint8))
    assert t.data_ptr() % 16 == residue
    return t


def rand_bytes(seed, n):
    """n random bytes, the first not 0."""
    b = bytearray(np.random.default_rng(seed).integers(0, 256, n, dtype=np.uint8).tobytes())
    b[0] |= 1
    return bytes(b)


def call(ctx, dev, sources, segs, first, hashes, flags=0, file_cap=None, tail=None, src_lens=None, n_segs=None, n=None):
    """One raw srd_batch_append_segments_device call with a sentinel-filled
    d_meta_off_out.  sources: device tensors; segs: (src, off, len[, reserved]);
    (rc, new_tail, meta offsets, message)."""
    import torch
    n = len(first) - 1 if n is None else n
    arr = (S.Segment * max(len(segs), 1))(*[(s[0], s[3] if len(s) > 3 else 0, s[1], s[2]) for s in segs])
    d_segs = torch.from_numpy(np.frombuffer(arr, np.uint8).copy()).cuda()
    d_first, d_h = A.dev_u64(first), A.dev_u64(hashes if len(hashes) else [0])
    mo = torch.from_numpy(np.full(max(n, 1), SENTINEL, np.uint64).view(np.int64)).cuda()
    k = len(sources)
    ptrs = (C.c_void_p * max(k, 1))(*[t.data_ptr() for t in sources])
    lens = (C.c_uint64 * max(k, 1))(*(src_lens if src_lens is not None else [t.numel() for t in sources]))
    nt = C.c_uint64(0xDEAD)
    torch.cuda.synchronize()  # the library launches on its own stream, not ordered behind torch's
    rc = S.lib().srd_batch_append_segments_device(
        ctx.h, ptrs, lens, k, C.c_void_p(d_segs.data_ptr()), len(segs) if n_segs is None else n_segs,
        C.c_void_p(d_first.data_ptr()), C.c_void_p(d_h.data_ptr()), n, flags, dev.tail if tail is None else tail,
        C.c_void_p(dev.t.data_ptr()), dev.cap if file_cap is None else file_cap, C.byref(nt), C.c_void_p(mo.data_ptr()),
        C.c_void_p(ctx.stream))
    msg = S.lib().srd_last_error().decode() if rc else ""
    torch.cuda.synchronize()
    return rc, int(nt.value), [int(x) for x in mo.cpu().numpy().view(np.uint64)[:n]], msg


def concat(host_sources, segs, first):
    """The entries' payloads: the host concatenation of each entry's segments."""
    return [b"".join(bytes(host_sources[s[0]][s[1]: s[1] + s[2]]) for s in segs[a:b]) for a, b in zip(first, first[1:])]


def segments_ok(ctx, dev, prefix, sources, host_sources, segs, first, hashes):
    """Appends through the device call and checks the whole buffer and the offsets; returns the oracle's store."""
    payloads = concat(host_sources, segs, first)
    want, want_mo = A.oracle_append(prefix, hashes, payloads)
    rc, nt, mo, msg = call(ctx, dev, sources, segs, first, hashes)
    assert rc == 0, msg
    assert nt == len(want)
    dev.check(want)
    assert mo == want_mo
    dev.tail = nt
    return want


def room(host_sources, segs):
    return sum(s[2] for s in segs) + 84 * len(segs) + 4096


# -- 1. one segment per entry, one source: the append's own shapes ---------------------------------

@pytest.mark.parametrize("residue", [0, 1, 8, 15])
def test_one_segment_per_entry_equals_the_append(ctx, residue):
    import torch
    ents = A.length_entries()
    hashes, payloads = [kh(k) for k, _ in ents], [p for _, p in ents]
    blob, offs = A.pack(payloads, residue, 32)
    blob_t = torch.from_numpy(blob).cuda()
    prefix = A.store_with_residue(44)
    segs, first = [(0, o, len(p)) for o, p in zip(offs, payloads)], list(range(len(payloads) + 1))
    dev = Dev(prefix, room([blob], segs))
    want = segments_ok(ctx, dev, prefix, [blob_t], [blob], segs, first, hashes)
    # the append under the stream rule on a second buffer: the same bytes, tail and offsets
    dev2 = Dev(prefix, room([blob], segs))
    rc, nt, mo, msg = A.append(ctx, dev2, blob_t, offs, [len(p) for p in payloads], hashes, flags=S.APPEND_STREAM_RULE)
    assert rc == 0, msg
    assert nt == len(want)
    dev2.check(want)  # (either call may leave [new_tail, roundup64(new_tail)) alone or write it as zero)
    assert dev2.host()[:nt].tobytes() == dev.host()[:nt].tobytes()
    assert mo == A.oracle_append(prefix, hashes, payloads)[1]
    if residue == 1:
        A.validate_matches_oracle(ctx, dev, want)


# -- 2. every (destination, source) residue pair -------------------------------------------------

def test_every_residue_pair(ctx):
    """256 entries [d bytes, 5000 bytes at source residue s], every (d mod 16, s) once; the same with a second
    segment of C + 4097 bytes (a unit boundary on the realigning path, both ring roles) for 12 pairs."""
    rng = random.Random(0x5E65)
    cases = [(d, s, 5000) for d in range(1, 17) for s in range(16)] + \
            [(d, s, CH + 4097) for d in (1, 4, 15, 16) for s in (0, 1, 15)]
    heads, bodies, segs, first, o = bytearray(), bytearray(16), [], [0], 16
    for d, s, n in cases:
        segs.append((0, len(heads), d))
        heads += nonzero_bytes(rng, d)
        o = ((o + 15) & ~15) + s
        bodies += bytes(o - len(bodies)) + rng.randbytes(n)
        segs.append((1, o, n))
        o += n
        first.append(len(segs))
    host = [bytes(heads), bytes(bodies)]
    srcs = [place(host[0]), place(host[1])]
    hashes = [kh(b"rp-%d" % i) for i in range(len(cases))]
    prefix = A.store_with_residue(1)
    dev = Dev(prefix, room(host, segs))
    want = segments_ok(ctx, dev, prefix, srcs, host, segs, first, hashes)
    A.validate_matches_oracle(ctx, dev, want)


# -- 3. segment lengths at every granule -----------------------------------------------------------

GRANULES = [1, 15, 16, 17, 63, 64, 65, 1023, 1024, 1025, 4095, 4096, 4097, CH - 1, CH, CH + 1, 2 * CH + 17]


def test_segment_lengths_at_every_granule(ctx):
    """Entries [a, b, a]: every value of GRANULES as a and as b, at random source offsets."""
    rng = random.Random(3)
    host = [rand_bytes(31, 3 * CH + 4096)]
    segs, first = [], [0]
    for k, a in enumerate(GRANULES):
        b = GRANULES[(k + 5) % len(GRANULES)]
        for n in (a, b, a):
            segs.append((0, rng.randrange(0, len(host[0]) - n + 1), n))
        first.append(len(segs))
    assert {s[2] for s in segs[0::3]} == {s[2] for s in segs[1::3]} == set(GRANULES)
    hashes = [kh(b"g-%d" % i) for i in range(len(GRANULES))]
    prefix = A.store_with_residue(63)
    dev = Dev(prefix, room(host, segs))
    segments_ok(ctx, dev, prefix, [place(host[0], 3)], host, segs, first, hashes)


# -- 4. zero-length segments --------------------------------------------------------------------

def test_zero_length_segments(ctx):
    host = [rand_bytes(41, 20000), b""]
    body = [(0, 5, 100), (0, 7001, 4097), (0, 300, 17)]
    z = [(0, 0, 0), (0, 20000, 0), (1, 0, 0)]  # empty ranges: at a source's start and end, of an empty source
    with_zeros = [z[0]] + body[:1] + [z[1], z[2]] + body[1:] + [z[0]] + [z[2]] + body[:2] + [z[1]]
    first_z = [0, 7, 11]
    without = body + body[:2]
    first_w = [0, 3, 5]
    srcs = [place(host[0], 9), place(b"")]
    prefix = A.store_with_residue(43)
    hashes = [kh(b"z-0"), kh(b"z-1")]
    assert concat(host, with_zeros, first_z) == concat(host, without, first_w)
    dev = Dev(prefix, 40000)
    segments_ok(ctx, dev, prefix, srcs, host, with_zeros, first_z, hashes)
    dev2 = Dev(prefix, 40000)
    segments_ok(ctx, dev2, prefix, srcs, host, without, first_w, hashes)
    assert bool((dev.host() == dev2.host()).all())


# -- 5. many units per entry: the combine's lane stride -----------------------------------------

def test_many_units_per_entry(ctx):
    """63, 64, 65, 129 and 200 segments of 16 bytes, 200 of 1 byte, 130 of C / 2 + 1 bytes: every segment is a
    unit; full, ragged and empty lanes of the combine, and more than one round."""
    rng = random.Random(5)
    host = [rand_bytes(51, 2 * CH)]
    segs, first = [], [0]
    for count, n in [(63, 16), (64, 16), (65, 16), (129, 16), (200, 16), (200, 1), (130, CH // 2 + 1)]:
        for _ in range(count):
            segs.append((0, rng.randrange(0, len(host[0]) - n + 1), n))
        first.append(len(segs))
    hashes = [kh(b"mu-%d" % i) for i in range(len(first) - 1)]
    prefix = A.store_with_residue(0)
    dev = Dev(prefix, room(host, segs))
    want = segments_ok(ctx, dev, prefix, [place(host[0])], host, segs, first, hashes)
    A.validate_matches_oracle(ctx, dev, want)


# -- 6. more units than the grid has waves ---------------------------------------------------------

def test_more_units_than_waves(ctx, W):
    """At least 2.5 W units of mixed 1-, 2- and 3-block segments in entries of 1 to 4 segments: every wave walks
    from unit to unit across entry ends, in both ring roles."""
    rng = random.Random(6)
    host = [rand_bytes(61, 1 << 20)]
    n_units = 5 * W // 2 + 7
    segs, first = [], [0]
    while len(segs) < n_units:
        for _ in range(rng.randrange(1, 5)):
            n = rng.randrange(1, 4097) + 4096 * rng.randrange(3)
            segs.append((0, rng.randrange(0, len(host[0]) - n + 1), n))
        first.append(len(segs))
    hashes = [rng.getrandbits(63) for _ in range(len(first) - 1)]
    prefix = A.store_with_residue(1)
    dev = Dev(prefix, room(host, segs))
    segments_ok(ctx, dev, prefix, [place(host[0], 5)], host, segs, first, hashes)


# -- 7. several sources ----------------------------------------------------------------------------

def test_three_sources_named_twice_and_overlapping(ctx):
    h0, h1, big = rand_bytes(71, 64), rand_bytes(72, 70001), rand_bytes(73, 12000)
    t_big = place(big, 4)
    # sources 2 and 3 overlap each other: two ranges of one allocation
    srcs = [place(h0), place(h1, 7), t_big[:8000], t_big[5000:]]
    host = [h0, h1, big[:8000], big[5000:]]
    segs = [(0, 0, 64), (1, 0, 70001),                     # header + tensor
            (0, 0, 64), (2, 100, 7900), (3, 0, 7000),      # the same header again; the overlapping sources
            (1, 69000, 1001), (1, 69000, 1001),            # one segment named twice in one entry
            (3, 6999, 1)]
    first = [0, 2, 5, 7, 8]
    hashes = [kh(b"ms-%d" % i) for i in range(4)]
    prefix = A.store_with_residue(44)
    dev = Dev(prefix, room(host, segs))
    want = segments_ok(ctx, dev, prefix, srcs, host, segs, first, hashes)
    A.validate_matches_oracle(ctx, dev, want)


# -- 8. sources inside the store --------------------------------------------------------------------

def oracle_store():
    rng = random.Random(8)
    pays = [nonzero_bytes(rng, n) for n in (300, 5000, CH + 77, 41)]
    buf = bytearray()
    tail = O.write_entries(buf, 0, [(kh(b"old-%d" % i), p) for i, p in enumerate(pays)])
    ranges, t = [], 0
    for p in pays:
        ranges.append((pad64(t), len(p)))
        t = pad64(t) + len(p) + 20
    assert t == tail == len(buf)
    return bytes(buf), ranges


def test_sources_inside_the_store(ctx):
    prefix, ranges = oracle_store()
    header = rand_bytes(81, 20)
    dev = Dev(prefix, 2 * CH)
    tail = dev.tail
    # a new entry: a header from another tensor, then the payloads of old-2 and old-1
    srcs, host = [place(header, 2), dev.t[:tail]], [header, prefix]
    segs, first = [(0, 0, 20), (1, ranges[2][0], ranges[2][1]), (1, ranges[1][0], ranges[1][1])], [0, 3]
    want = segments_ok(ctx, dev, prefix, srcs, host, segs, first, [kh(b"joined")])
    assert want[:tail] == prefix
    A.validate_matches_oracle(ctx, dev, want)  # n_crc_bad == 0, the chain and the index are the oracle's
    # a source that reaches into [tail, roundup64(new_tail)) is refused, nothing written
    before = dev.host().copy()
    last = pad64(dev.tail) + 63  # new_tail = roundup64(tail) + 41: the last byte below roundup64(new_tail)
    for reach in (dev.t[: dev.tail + 1], dev.t[last: last + 1]):
        rc, nt, mo, msg = call(ctx, dev, [srcs[0], reach], [(0, 0, 20), (1, 0, 1)], [0, 2], [kh(b"x")])
        assert rc == S.SRD_ERR_ARG and "overlaps" in msg, (rc, msg)
        assert nt == dev.tail and mo == [SENTINEL]
        assert bool((dev.host() == before).all())
    # ... the byte just below the tail and the line just behind the batch are legal sources
    behind = pad64(pad64(dev.tail) + 21 + 20)
    rc, nt, mo, msg = call(ctx, dev, [srcs[0], dev.t[: dev.tail], dev.t[behind: behind + 8]],
                           [(0, 0, 20), (1, dev.tail - 1, 1)], [0, 2], [kh(b"x")])
    assert rc == 0 and nt == pad64(dev.tail) + 21 + 20, msg


# -- 9. the stream rule -----------------------------------------------------------------------------

@pytest.mark.parametrize("last_byte", [0, 7])
def test_stream_rule_over_segments(ctx, last_byte):
    """An entry of three all-zero segments (1, 4096 and C + 5 bytes) is refused; with the last byte of the last
    segment not 0 it is accepted."""
    z = bytearray(CH + 5)
    z[-1] = last_byte
    host = [rand_bytes(91, 2 * CH + 8192), bytes(4096), bytes(z)]
    srcs = [place(host[0]), place(host[1], 3), place(host[2], 11)]
    segs, first = [(0, 0, 100), (1, 0, 1), (1, 0, 4096), (2, 0, CH + 5)], [0, 1, 4]
    prefix = A.store_with_residue(63)
    dev = Dev(prefix, 3 * CH)
    if last_byte:
        segments_ok(ctx, dev, prefix, srcs, host, segs, first, [kh(b"a"), kh(b"z")])
        return
    rc, nt, _mo, msg = call(ctx, dev, srcs, segs, first, [kh(b"a"), kh(b"z")])
    assert rc == S.SRD_ERR_ARG and NULL_ONLY in msg, (rc, msg)
    assert nt == dev.tail == len(prefix)
    got = dev.host()
    assert got[: len(prefix)].tobytes() == prefix  # nothing below the tail changed
    assert bool((got[pad64(pad64(len(prefix)) + 100 + 84 + CH + 4102 + 84):] == A.FILL).all())
    # ... and a valid batch at the same tail (longer than what the refused one wrote) gives the oracle's store
    want = segments_ok(ctx, dev, prefix, srcs, host, segs[:1] + [(0, 0, len(host[0]))], [0, 1, 2], [kh(b"a"), kh(b"b")])
    A.validate_matches_oracle(ctx, dev, want)


def test_zero_entry_behind_a_nonzero_unit(ctx, W):
    """An all-zero entry whose unit is its wave's second, behind a unit of two nonzero blocks, is refused."""
    host = [rand_bytes(92, 8192 + 64), bytes(5000)]
    srcs = [place(host[0]), place(host[1])]
    segs = [(0, 16 * (i % 4), 8192) for i in range(W)] + [(1, 0, 5000)]
    first = list(range(W + 2))
    dev = Dev(b"", room(host, segs))
    rc, nt, _mo, msg = call(ctx, dev, srcs, segs, first, list(range(1, W + 2)))
    assert rc == S.SRD_ERR_ARG and NULL_ONLY in msg and nt == 0, (rc, msg)
    # the same batch with one byte of that entry not 0
    host[1] = bytes(4999) + b"\x01"
    srcs[1] = place(host[1])
    segments_ok(ctx, dev, b"", srcs, host, segs, first, list(range(1, W + 2)))


# -- 10. plan-time refusals: nothing is written -------------------------------------------------------

REFUSALS = ["no_segments", "zero_length_only", "src_out_of_table", "reserved", "one_past_source", "off_wraps",
            "len_wraps", "first0", "first_decreasing", "first_n", "cap_one_short", "flags"]


def refusal_setup():
    host = [rand_bytes(101, 6000), rand_bytes(102, 64)]
    segs = [(1, 0, 64), (0, 0, 5000), (0, 100, 1), (1, 3, 20), (0, 5000, 1000)]
    return host, [place(host[0], 1), place(host[1])], segs, [0, 2, 3, 5]


@pytest.mark.parametrize("case", REFUSALS)
def test_refusals_write_nothing(ctx, case):
    host, srcs, segs, first = refusal_setup()
    hashes = [kh(b"r-%d" % i) for i in range(3)]
    prefix = A.store_with_residue(43)
    dev = Dev(prefix, 16384)
    before = dev.host().copy()
    want, _ = A.oracle_append(prefix, hashes, concat(host, segs, first))
    kw, match = {}, None
    if case == "no_segments":
        first, match = [0, 2, 2, 5], EMPTY
        segs = segs[:2] + segs[3:] + [(0, 0, 1)]
    elif case == "zero_length_only":
        segs[2], match = (0, 6000, 0), EMPTY
    elif case == "src_out_of_table":
        segs[3], match = (2, 0, 1), "entry 2 has a malformed segment"
    elif case == "reserved":
        segs[2], match = (0, 100, 1, 1), "entry 1 has a malformed segment"
    elif case == "one_past_source":
        segs[4], match = (0, 5000, 1001), "entry 2 has a malformed segment"
    elif case == "off_wraps":
        segs[1], match = (0, M64 - 99, 200), "entry 0 has a malformed segment"
    elif case == "len_wraps":
        segs[1], match = (0, 64, M64 - 31), "entry 0 has a malformed segment"
    elif case == "first0":
        first, match = [1, 2, 3, 5], "d_seg_first is malformed at entry 0"
    elif case == "first_decreasing":
        first, match = [0, 3, 2, 5], "d_seg_first is malformed at entry 1"
    elif case == "first_n":
        first, match = [0, 2, 3, 4], "d_seg_first is malformed at entry 2"
    elif case == "cap_one_short":
        kw, match = {"file_cap": S.padded_size(len(want)) - 1}, "file_cap"
    elif case == "flags":
        kw, match = {"flags": 1}, "flags"
    rc, nt, mo, msg = call(ctx, dev, srcs, segs, first, hashes, **kw)
    assert rc == S.SRD_ERR_ARG and match in msg, (rc, msg)
    assert nt == dev.tail  # the caller's tail does not move
    assert mo == [SENTINEL] * 3
    assert bool((dev.host() == before).all())
    if case == "cap_one_short":  # ... and with that one byte it fits
        rc, nt, mo, msg = call(ctx, dev, srcs, segs, first, hashes, file_cap=kw["file_cap"] + 1)
        assert rc == 0 and nt == len(want), msg
        dev.check(want)


def test_first_refused_entry_decides(ctx):
    host, srcs, segs, first = refusal_setup()
    dev = Dev(A.store_with_residue(43), 16384)
    before = dev.host().copy()
    bad, empty = (7, 0, 1), (0, 0, 0)
    rc, nt, mo, msg = call(ctx, dev, srcs, segs[:2] + [empty, segs[3], bad], first, [1, 2, 3])
    assert rc == S.SRD_ERR_ARG and EMPTY in msg and nt == dev.tail and mo == [SENTINEL] * 3
    rc, _nt, _mo, msg = call(ctx, dev, srcs, [bad] + segs[1:2] + [empty] + segs[3:], first, [1, 2, 3])
    assert rc == S.SRD_ERR_ARG and "entry 0 has a malformed segment" in msg
    # an entry with a malformed segment is refused for that, whatever its length (here: 0 otherwise)
    rc, _nt, _mo, msg = call(ctx, dev, srcs, segs[:2] + [(0, 6001, 0)] + segs[3:], first, [1, 2, 3])
    assert rc == S.SRD_ERR_ARG and "entry 1 has a malformed segment" in msg
    assert bool((dev.host() == before).all())


def test_empty_batch(ctx):
    dev = Dev(A.store_with_residue(44), 4096)
    before = dev.host().copy()
    rc, nt, _mo, msg = call(ctx, dev, [], [], [0], [])
    assert rc == 0 and nt == dev.tail, msg
    assert bool((dev.host() == before).all())


# -- 11. the session: DeviceStore ---------------------------------------------------------------------

def test_session_write_stream(ctx):
    import torch
    rng = random.Random(111)
    st = S.DeviceStore.create(4 << 20, ctx)
    model = bytearray()
    keys = [b"k-%d" % i for i in range(6)]
    bodies = [nonzero_bytes(rng, n) for n in (1, 64, 4097, CH + 1, 2 * CH + 17, 300)]
    headers = [nonzero_bytes(rng, n) for n in (64, 20, 1, 15, 16, 33)]
    # header + body entries: uint8 headers, bodies of several dtypes (taken as their bytes)
    body_t = [place(b, 1) for b in bodies[:3]] + [place(b + bytes(-len(b) % 4)) for b in bodies[3:]]
    body_t[5] = body_t[5].view(torch.float32)
    body_t[3] = body_t[3].view(torch.int16)[: (CH + 1) // 2 + 1]
    for i in (3, 4, 5):  # (padded to whole elements above)
        bodies[i] = body_t[i].cpu().numpy().tobytes()
    assert len(bodies[3]) == CH + 2 and len(bodies[4]) == 2 * CH + 20
    ents = [[place(h), b] for h, b in zip(headers, body_t)]
    pays = [h + b for h, b in zip(headers, bodies)]
    nt = st.batch_write_stream(keys, ents)
    assert nt == O.write_entries(model, 0, [(kh(k), p) for k, p in zip(keys, pays)]) == st.tail
    assert st.bytes() == bytes(model) and st.len() == 6
    assert st.batch_read(keys + [b"absent"]) == pays + [None]
    assert st.verify(keys + [b"absent"]) == [True] * 6 + [None]
    # write_stream of a key that exists: overwritten
    new = nonzero_bytes(rng, 777)
    nt2 = st.write_stream(keys[2], [place(new[:700], 5), place(new[700:])])
    assert nt2 == O.write_entries(model, nt, [(kh(keys[2]), new)]) == st.tail
    pays[2] = new
    assert st.len() == 6 and st.batch_read(keys) == pays
    # a stream made of slices of the store's own buffer: the payloads of two earlier entries, joined
    idx = O.key_indexer_build(np.frombuffer(bytes(model), np.uint8), len(model))

    def payload_range(k):
        mo = idx[kh(k)] & ((1 << 48) - 1)
        return mo - len(pays[keys.index(k)]), mo

    (a0, a1), (b0, b1) = payload_range(keys[4]), payload_range(keys[0])
    nt3 = st.write_stream_with_key_hash(kh(b"joined"), [st.buf[a0:a1], st.buf[b0:b1]])
    assert nt3 == O.write_entries(model, nt2, [(kh(b"joined"), pays[4] + pays[0])]) == st.tail
    assert st.bytes() == bytes(model) and st.len() == 7
    assert st.batch_read([b"joined"]) == [pays[4] + pays[0]]

    def index_is_the_oracles():
        got = st.bytes()
        k, p = st.index.export()
        exp = dict(zip((int(x) for x in k.cpu().numpy().view(np.uint64)), (int(x) for x in p.cpu().numpy().view(np.uint64))))
        assert exp == O.key_indexer_build(np.frombuffer(got, np.uint8), len(got)) and st.len() == len(exp)

    index_is_the_oracles()
    allk, allp = keys + [b"joined"], pays + [pays[4] + pays[0]]
    st.compact()
    assert st.batch_read(allk) == allp and st.verify(allk) == [True] * 7
    index_is_the_oracles()

    # errors leave the tail, len() and bytes() as they were
    tail, before = st.tail, st.bytes()

    def unchanged():
        assert st.tail == tail and st.bytes() == before and st.len() == 7
        assert st.batch_read(allk) == allp

    with pytest.raises(ValueError, match="capacity"):
        st.write_stream(b"big", [place(headers[0]), torch.ones(4 << 20, dtype=torch.uint8, device="cuda")])
    unchanged()
    with pytest.raises(S.SrdError, match="NULL-byte-only streams"):
        st.batch_write_stream([b"ok", b"nul"], [[place(headers[0])], [place(bytes(10)), place(bytes(5000), 3)]])
    unchanged()
    with pytest.raises(S.SrdError, match="Payload cannot be empty."):
        st.write_stream(b"none", [])
    unchanged()
    with pytest.raises(ValueError, match="tensor"):
        st.write_stream(b"host", [place(headers[0]), torch.ones(8, dtype=torch.uint8)])
    with pytest.raises(ValueError, match="tensor"):
        st.write_stream(b"strided", [torch.ones((8, 8), dtype=torch.uint8, device="cuda")[:, 0]])
    with pytest.raises(ValueError, match="tensor"):
        st.write_stream(b"bytes", [b"abc"])
    with pytest.raises(ValueError, match="Mismatched"):
        st.batch_write_stream([b"a", b"b"], [[place(headers[0])]])
    unchanged()
    assert st.batch_write_stream([], []) == tail
