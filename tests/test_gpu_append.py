"""Payloads already in HBM appended to a store: srd_batch_append_device (the
layout by one exclusive sum on the device, the payload bytes moved in the
gather's work units with their CRC-32 computed on the way, metadata and prepads
by the finish step) and the Python layers over it (DeviceStore.
batch_write_device[_with_key_hashes], batch_copy / batch_transfer /
batch_rename and their single-key forms).

Expected bytes come from the oracle (O.write_entries applied to a host copy of
the store); every comparison is bit-exact and covers the whole allocation: the
buffer is 0xA5 beyond the tail before a call, and afterwards [0, new_tail) is the
oracle's store, [new_tail, roundup64(new_tail)) is 0xA5 or 0, and everything
behind is still 0xA5.  The shapes are the smallest at which the kernels can go
wrong, C = GATHER_CHUNK: the 16-byte piece, the 64-byte line, the 1 KiB lane
row, the 4 KiB block in both ring roles, the chunk, every prepad length at the
start tail, and more units than the grid has waves."""
import ctypes as C
import random

import numpy as np
import pytest

import oracle as O
import srd_amd as S

pytestmark = pytest.mark.gpu

CH = S.GATHER_CHUNK
LENGTHS = [1, 2, 15, 16, 17, 63, 64, 65, 1023, 1024, 1025, 1040, 4095, 4096, 4097, 8191, 8192, 8193, 12289,
           CH - 1, CH, CH + 1, 2 * CH, 2 * CH + 17, 3 * CH + 4097]
FILL = 0xA5
SLACK = 8192
SENTINEL = 0x5A5A5A5A5A5A5A5A


@pytest.fixture(scope="module")
def ctx():
    c = S.Context(0)
    yield c
    c.close()


def pad64(n):
    return (n + 63) & ~63


def kh(name):
    return O.xxh3_64(name)


def dev_u64(a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a, np.uint64).view(np.int64)).cuda()


def nonzero_bytes(rng, n):
    """n random bytes, none of them 0 (a 1-byte payload must not be the NULL byte)."""
    return bytes(rng.randrange(1, 256) for _ in range(n)) if n < 64 else bytes([rng.randrange(1, 256)]) + rng.randbytes(n - 1)


def length_entries():
    """(key, payload) per length in LENGTHS (random bytes), one all-0xFF payload, one zero-heavy payload."""
    rng = random.Random(0xA99E)
    ents = [(b"len-%d" % n, nonzero_bytes(rng, n)) for n in LENGTHS]
    ents.append((b"all-ff", b"\xff" * 5000))
    zh = bytearray(9000)
    zh[0], zh[4096], zh[8999] = 1, 7, 9
    ents.append((b"zero-heavy", bytes(zh)))
    return ents


@pytest.fixture(scope="module")
def lents():
    return length_entries()


def pack(payloads, residue=0, lead=0):
    """The payloads in one host blob, each at an offset = residue mod 16 behind `lead` unused bytes."""
    offs, o = [], lead
    for p in payloads:
        o = ((o + 15) & ~15) + residue
        offs.append(o)
        o += len(p)
    blob = np.full(max(o, 1), 0xEE, np.uint8)
    for a, p in zip(offs, payloads):
        blob[a: a + len(p)] = np.frombuffer(p, np.uint8)
    return blob, offs


def oracle_append(prefix: bytes, hashes, payloads):
    """(the oracle's store after the batch, its metadata offsets)."""
    buf = bytearray(prefix)
    tail = O.write_entries(buf, len(prefix), list(zip(hashes, payloads)))
    assert tail == len(buf)
    # the batch's metadata offsets, by the reference's layout rule over the oracle's bytes
    mo, t = [], len(prefix)
    for p in payloads:
        m = pad64(t) + len(p)
        mo.append(m)
        t = m + 20
    assert t == tail
    for h, m in zip(hashes, mo):  # ... each is where the oracle put that key hash
        assert int.from_bytes(buf[m: m + 8], "little") == h
    return bytes(buf), mo


class Dev:
    """A store buffer on the device: `prefix` below the tail, FILL up to the end of the allocation."""

    def __init__(self, prefix: bytes, room: int):
        import torch
        self.cap = S.padded_size(len(prefix) + room) + SLACK
        self.t = torch.full((self.cap,), FILL, dtype=torch.uint8, device="cuda")
        if prefix:
            self.t[: len(prefix)] = torch.frombuffer(bytearray(prefix), dtype=torch.uint8).cuda()
        self.tail = len(prefix)
        torch.cuda.synchronize()

    def host(self):
        return self.t.cpu().numpy()

    def check(self, want: bytes):
        """The whole allocation against the oracle's store `want`."""
        got = self.host()
        nt = len(want)
        assert got[:nt].tobytes() == want, first_diff(got[:nt], want)
        gap = got[nt: pad64(nt)]
        assert bool(((gap == FILL) | (gap == 0)).all())
        assert bool((got[pad64(nt):] == FILL).all()), "a byte at or above roundup64(new_tail) was touched"


def first_diff(got, want):
    w = np.frombuffer(want, np.uint8)
    d = np.nonzero(got != w)[0]
    return "first difference at byte %d of %d (%d differ)" % (int(d[0]), len(w), len(d)) if len(d) else "equal"


def append(ctx, dev, blob_t, offs, lens, hashes, flags=0, file_cap=None, blob_len=None, tail=None):
    """One raw srd_batch_append_device call with a sentinel-filled d_meta_off_out:
    (rc, new_tail, meta offsets, message)."""
    import torch
    n = len(offs)
    d_o, d_l, d_h = dev_u64(offs), dev_u64(lens), dev_u64(hashes)
    mo = torch.from_numpy(np.full(max(n, 1), SENTINEL, np.uint64).view(np.int64)).cuda()
    nt = C.c_uint64(0xDEAD)
    torch.cuda.synchronize()  # the library launches on its own stream, not ordered behind torch's
    rc = S.lib().srd_batch_append_device(
        ctx.h, C.c_void_p(blob_t.data_ptr()), blob_t.numel() if blob_len is None else blob_len, C.c_void_p(d_o.data_ptr()),
        C.c_void_p(d_l.data_ptr()), C.c_void_p(d_h.data_ptr()), n, flags, dev.tail if tail is None else tail,
        C.c_void_p(dev.t.data_ptr()), dev.cap if file_cap is None else file_cap, C.byref(nt), C.c_void_p(mo.data_ptr()),
        C.c_void_p(ctx.stream))
    msg = S.lib().srd_last_error().decode() if rc else ""
    torch.cuda.synchronize()
    return rc, int(nt.value), [int(x) for x in mo.cpu().numpy().view(np.uint64)[:n]], msg


def append_ok(ctx, dev, prefix: bytes, hashes, payloads, residue=0, lead=0, base_shift=0, flags=0):
    """Appends through the device call and checks the whole buffer and the offsets; returns the oracle's store."""
    import torch
    blob, offs = pack(payloads, residue, lead + base_shift)
    blob_t = torch.from_numpy(blob).cuda()[base_shift:]  # (base_shift 1: a blob base that is not 16-aligned)
    offs = [o - base_shift for o in offs]
    want, want_mo = oracle_append(prefix, hashes, payloads)
    rc, nt, mo, msg = append(ctx, dev, blob_t, offs, [len(p) for p in payloads], hashes, flags)
    assert rc == 0, msg
    assert nt == len(want)
    dev.check(want)
    assert mo == want_mo
    dev.tail = nt
    return want


def validate_matches_oracle(ctx, dev, want: bytes):
    r = S.validate_index_device(dev.t.data_ptr(), len(want), 0, ctx)
    f = np.frombuffer(want, np.uint8)
    assert int(r.final_len) == O.recover_valid_chain(f) == len(want)
    ch = O.chain(f, len(want))
    assert int(r.n_chain) == len(ch) and int(r.n_crc_bad) == 0
    got_mo = sorted(int(x) for x in S.device_to_numpy(r.meta_off, int(r.n_chain)))
    assert got_mo == sorted(e["meta_off"] for e in ch)
    got_crc = dict(zip((int(x) for x in S.device_to_numpy(r.meta_off, int(r.n_chain))),
                       (int(x) for x in S.device_to_numpy(r.crc_computed, int(r.n_chain), np.uint32))))
    assert got_crc == {e["meta_off"]: e["crc_computed"] for e in ch}
    idx = dict(zip((int(x) for x in S.device_to_numpy(r.index_key_hash, int(r.n_index))),
                   (int(x) for x in S.device_to_numpy(r.index_packed, int(r.n_index)))))
    assert idx == O.key_indexer_build(f, len(want))


# -- lengths ----------------------------------------------------------------------------

def test_lengths_in_one_batch(ctx, lents):
    hashes, payloads = [kh(k) for k, _ in lents], [p for _, p in lents]
    dev = Dev(b"", sum(len(p) + 84 for p in payloads))
    want = append_ok(ctx, dev, b"", hashes, payloads)
    validate_matches_oracle(ctx, dev, want)
    # the same bytes as the host-input write of the same pairs
    st = S.DeviceStore.create(len(want) + 4096, ctx)
    assert st.batch_write_with_key_hashes(hashes, payloads) == len(want)
    assert st.bytes() == want


def test_lengths_one_call_per_entry(ctx, lents):
    """Every length as a wave's first and last unit; prev_offset chained across calls."""
    dev = Dev(b"", sum(len(p) + 84 for _, p in lents))
    cur = b""
    for k, p in lents:
        cur = append_ok(ctx, dev, cur, [kh(k)], [p])
    validate_matches_oracle(ctx, dev, cur)


# -- start tails: every prepad length, the first metadata line shared with old bytes ------

def store_with_residue(res):
    """An oracle-written store whose tail is `res` mod 64."""
    n = (res - 20) % 64 or 64
    buf = bytearray()
    tail = O.write_entries(buf, 0, [(kh(b"old-a"), b"\x11" * 200), (kh(b"old-b"), b"\x22" * n)])
    assert tail % 64 == res and tail == len(buf)
    return bytes(buf)


@pytest.mark.parametrize("res", [0, 1, 43, 44, 63])
def test_start_tail_residues(ctx, res):
    rng = random.Random(res)
    prefix = store_with_residue(res)
    payloads = [nonzero_bytes(rng, n) for n in (1, 44, 23, 4097, CH + 1, 107)]
    hashes = [kh(b"new-%d" % i) for i in range(len(payloads))]
    dev = Dev(prefix, sum(len(p) + 84 for p in payloads))
    want = append_ok(ctx, dev, prefix, hashes, payloads)
    assert want[: len(prefix)] == prefix
    validate_matches_oracle(ctx, dev, want)
    # and one entry alone behind it: a batch whose first entry is its last
    more = append_ok(ctx, dev, want, [kh(b"tail")], [nonzero_bytes(rng, 300)])
    validate_matches_oracle(ctx, dev, more)


# -- source alignment ---------------------------------------------------------------------

@pytest.mark.parametrize("base_shift", [0, 1])
@pytest.mark.parametrize("residue", range(16))
def test_source_alignment(ctx, residue, base_shift):
    """Every source residue mod 16 against the 64-aligned payload slots: the
    streaming kernel's one-vector path (residue + base_shift a multiple of 16)
    and each shift of its two-vector path."""
    rng = random.Random(16 * base_shift + residue)
    payloads = [nonzero_bytes(rng, n) for n in (17, 1040, 4097, 12289, CH + 1, 2 * CH + 17)]
    hashes = [kh(b"al-%d" % i) for i in range(len(payloads))]
    prefix = store_with_residue(44)
    dev = Dev(prefix, sum(len(p) + 84 for p in payloads))
    append_ok(ctx, dev, prefix, hashes, payloads, residue=residue, lead=32, base_shift=base_shift)


# -- many units per wave ------------------------------------------------------------------

def test_many_small_entries(ctx):
    """100,000 entries of 1..64 bytes in one call: every wave of the grid walks a long unit sequence."""
    import torch
    n = 100_000
    rng = np.random.default_rng(0xA99E)
    lens = rng.integers(1, 65, n).astype(np.uint64)
    offs = np.zeros(n, np.uint64)
    offs[1:] = np.cumsum(lens)[:-1]  # packed back to back: every source alignment
    blob = rng.integers(1, 256, int(lens.sum()), dtype=np.uint8)
    hashes = rng.integers(0, 1 << 63, n).astype(np.uint64)
    raw = blob.tobytes()
    payloads = [raw[int(o): int(o) + int(ln)] for o, ln in zip(offs, lens)]
    prefix = store_with_residue(1)
    want, want_mo = oracle_append(prefix, [int(h) for h in hashes], payloads)
    dev = Dev(prefix, len(want) - len(prefix))
    rc, nt, mo, msg = append(ctx, dev, torch.from_numpy(blob).cuda(), offs, lens, hashes)
    assert rc == 0, msg
    assert nt == len(want) and mo == want_mo
    dev.check(want)


# -- refusals: nothing is written -----------------------------------------------------------

def refusal_setup():
    import torch
    rng = random.Random(7)
    prefix = store_with_residue(43)
    payloads = [nonzero_bytes(rng, n) for n in (100, 5000, 1, 300)]
    blob, offs = pack(payloads + [b"\x00"])
    return prefix, payloads, torch.from_numpy(blob).cuda(), offs


REFUSALS = ["zero_len", "nul_byte", "one_past_blob", "src_off_wraps", "len_wraps", "cap_one_short", "overlap"]


@pytest.mark.parametrize("case", REFUSALS)
def test_refusals_write_nothing(ctx, case):
    prefix, payloads, blob_t, offs = refusal_setup()
    nul_off, offs = offs[-1], offs[:-1]
    lens = [len(p) for p in payloads]
    hashes = [kh(b"r-%d" % i) for i in range(len(payloads))]
    dev = Dev(prefix, 16384)
    before = dev.host().copy()
    kw, match = {}, None
    if case == "zero_len":
        lens[2], match = 0, "Payload cannot be empty."
    elif case == "nul_byte":
        offs[2], match = nul_off, "NULL-byte payloads cannot be written directly."
    elif case == "one_past_blob":
        offs[3], match = blob_t.numel() - lens[3] + 1, "does not lie inside d_payloads"
    elif case == "src_off_wraps":
        offs[1], match = (1 << 64) - 100, "does not lie inside d_payloads"
    elif case == "len_wraps":
        offs[1], lens[1], match = 64, (1 << 64) - 32, "does not lie inside d_payloads"
    elif case == "cap_one_short":
        want, _ = oracle_append(prefix, hashes, payloads)
        kw, match = {"file_cap": S.padded_size(len(want)) - 1}, "file_cap"
    elif case == "overlap":
        # the store itself as the blob, one byte longer than what lies below the tail
        blob_t, offs, lens, match = dev.t, [0, 64, 128, 192], [10, 10, 10, 10], "overlaps"
        kw = {"blob_len": dev.tail + 1}
    rc, nt, mo, msg = append(ctx, dev, blob_t, offs, lens, hashes, **kw)
    assert rc == S.SRD_ERR_ARG and match in msg, (rc, msg)
    assert nt == dev.tail  # the caller's tail does not move
    assert mo == [SENTINEL] * len(offs)
    assert bool((dev.host() == before).all())
    if case == "cap_one_short":  # ... and with that one byte it fits
        rc, nt, mo, msg = append(ctx, dev, blob_t, offs, lens, hashes, file_cap=kw["file_cap"] + 1)
        assert rc == 0 and nt == len(want), msg
        dev.check(want)
    if case == "overlap":  # ... and the store below its tail is a legal blob (rename's case)
        rc, nt, mo, msg = append(ctx, dev, blob_t, offs, lens, hashes, blob_len=dev.tail)
        want, want_mo = oracle_append(prefix, hashes, [prefix[o: o + 10] for o in offs])
        assert rc == 0 and nt == len(want) and mo == want_mo, msg
        dev.check(want)


def test_first_refused_entry_decides(ctx):
    prefix, payloads, blob_t, offs = refusal_setup()
    offs, lens = offs[:-1], [len(p) for p in payloads]
    dev = Dev(prefix, 16384)
    lens[1], offs[3] = 0, 1 << 63
    rc, _nt, _mo, msg = append(ctx, dev, blob_t, offs, lens, [1, 2, 3, 4])
    assert rc == S.SRD_ERR_ARG and "Payload cannot be empty." in msg
    lens[1], lens[3], offs[3], offs[0] = 7, 0, 0, 1 << 63
    rc, _nt, _mo, msg = append(ctx, dev, blob_t, offs, lens, [1, 2, 3, 4])
    assert rc == S.SRD_ERR_ARG and "does not lie inside d_payloads" in msg


def test_empty_batch(ctx):
    import torch
    prefix = store_with_residue(44)
    dev = Dev(prefix, 4096)
    before = dev.host().copy()
    rc, nt, _mo, msg = append(ctx, dev, torch.zeros(16, dtype=torch.uint8, device="cuda"), [], [], [])
    assert rc == 0 and nt == dev.tail, msg
    assert bool((dev.host() == before).all())


# -- the stream rule --------------------------------------------------------------------------

def test_stream_rule(ctx):
    import torch
    rng = random.Random(11)
    prefix = store_with_residue(63)
    zeros = bytes(5000)
    h = [kh(b"z")]
    # without the flag 5000 zero bytes are a payload like any other
    dev = Dev(prefix, 3 * CH)
    append_ok(ctx, dev, prefix, h, [zeros])
    # with it the call fails after streaming; the tail does not move ...
    dev = Dev(prefix, 3 * CH)
    blob, offs = pack([nonzero_bytes(rng, 100), zeros])
    rc, nt, _mo, msg = append(ctx, dev, torch.from_numpy(blob).cuda(), offs, [100, 5000], [kh(b"a"), kh(b"z")],
                              flags=S.APPEND_STREAM_RULE)
    assert rc == S.SRD_ERR_ARG and "NULL-byte-only streams cannot be written directly." in msg
    assert nt == dev.tail == len(prefix)
    got = dev.host()
    assert got[: len(prefix)].tobytes() == prefix  # nothing below the tail changed
    assert bool((got[pad64(len(prefix) + 64 + 100 + 84 + 5000 + 84):] == FILL).all())
    # ... and a valid append at the same tail (longer than what the refused one wrote) gives the oracle's store
    pay = [nonzero_bytes(rng, 100), nonzero_bytes(rng, 6000)]
    want = append_ok(ctx, dev, prefix, [kh(b"a"), kh(b"b")], pay, flags=S.APPEND_STREAM_RULE)
    validate_matches_oracle(ctx, dev, want)


@pytest.mark.parametrize("nonzero_at", [None, 0, CH, 2 * CH + 16])
def test_stream_rule_multi_chunk(ctx, nonzero_at):
    """A payload of three chunks: all 0 is refused; one byte that is not 0, in any chunk, is accepted."""
    import torch
    p = bytearray(2 * CH + 17)
    if nonzero_at is not None:
        p[nonzero_at] = 3
    dev = Dev(b"", 4 * CH)
    if nonzero_at is None:
        blob, offs = pack([bytes(p), b"\x05" * 70])
        rc, nt, _mo, msg = append(ctx, dev, torch.from_numpy(blob).cuda(), offs, [len(p), 70], [1, 2],
                                  flags=S.APPEND_STREAM_RULE)
        assert rc == S.SRD_ERR_ARG and "NULL-byte-only streams" in msg and nt == 0
    else:
        append_ok(ctx, dev, b"", [1, 2], [bytes(p), b"\x05" * 70], flags=S.APPEND_STREAM_RULE)


# -- the session: DeviceStore --------------------------------------------------------------------

def to_blob(payloads):
    import torch
    blob, offs = pack(payloads)
    return torch.from_numpy(blob).cuda(), offs, [len(p) for p in payloads]


def test_session_write_read_overwrite_grow(ctx):
    import torch
    rng = random.Random(21)
    st = S.DeviceStore.create(4 << 20, ctx)
    model = bytearray()
    keys = [b"k-%d" % i for i in range(20)]
    pay = [nonzero_bytes(rng, n) for n in [1, 64, 4097, CH + 1, 2 * CH + 17] + [50 + i for i in range(15)]]
    blob, offs, lens = to_blob(pay)
    nt = st.batch_write_device(keys, blob, offs, lens)
    assert nt == O.write_entries(model, 0, [(kh(k), p) for k, p in zip(keys, pay)]) == st.tail
    assert st.bytes() == bytes(model) and st.len() == 20
    assert st.batch_read(keys + [b"absent"]) == pay + [None]
    g = st.batch_gather(keys)
    assert g.payloads() == pay and g.is_valid_checksum() == [True] * 20
    assert st.verify(keys + [b"absent"]) == [True] * 20 + [None]
    # an overwrite through the device path: device tensors for hashes, offsets and lengths
    new = [nonzero_bytes(rng, 777), nonzero_bytes(rng, 5)]
    blob2, offs2, lens2 = to_blob(new)
    hashes = torch.from_numpy(np.array([kh(keys[3]), kh(keys[0])], np.uint64).view(np.int64)).cuda()
    nt2 = st.batch_write_device_with_key_hashes(hashes, blob2, torch.tensor(offs2, device="cuda"),
                                                torch.tensor(lens2, device="cuda"), stream_rule=True)
    assert nt2 == O.write_entries(model, nt, [(kh(keys[3]), new[0]), (kh(keys[0]), new[1])]) == st.tail
    assert st.bytes() == bytes(model) and st.len() == 20
    assert st.batch_read([keys[0], keys[3], keys[4]]) == [new[1], new[0], pay[4]]
    # growth of the index: more new keys than the table has room for
    cap0 = st.index.capacity
    many = [b"m-%d" % i for i in range(cap0)]
    mp = [nonzero_bytes(rng, 1 + i % 90) for i in range(cap0)]
    blob3, offs3, lens3 = to_blob(mp)
    nt3 = st.batch_write_device(many, blob3, offs3, lens3)
    assert nt3 == O.write_entries(model, nt2, [(kh(k), p) for k, p in zip(many, mp)])
    assert st.index.capacity > cap0 and st.len() == 20 + cap0
    assert st.bytes() == bytes(model)
    assert st.batch_read(many[::7] + [keys[3]]) == mp[::7] + [new[0]]
    assert st.verify(many[:5]) == [True] * 5


def test_session_refusals_leave_tail_and_index(ctx):
    rng = random.Random(22)
    st = S.DeviceStore.create(1 << 16, ctx)
    pay = [nonzero_bytes(rng, 100), nonzero_bytes(rng, 200)]
    blob, offs, lens = to_blob(pay)
    st.batch_write_device([b"a", b"b"], blob, offs, lens)
    tail, before = st.tail, st.bytes()

    def unchanged():
        assert st.tail == tail and st.bytes() == before and st.len() == 2
        assert st.batch_read([b"a", b"b", b"c"]) == pay + [None]

    with pytest.raises(S.SrdError, match="Payload cannot be empty."):
        st.batch_write_device([b"c", b"d"], blob, offs, [lens[0], 0])
    unchanged()
    with pytest.raises(S.SrdError, match="does not lie inside d_payloads"):
        st.batch_write_device([b"c"], blob, [blob.numel() - 5], [6])
    unchanged()
    zblob, zoffs, zlens = to_blob([bytes(300)])
    with pytest.raises(S.SrdError, match="NULL-byte-only streams"):
        st.batch_write_device_with_key_hashes([kh(b"c")], zblob, zoffs, zlens, stream_rule=True)
    unchanged()
    big, boffs, blens = to_blob([nonzero_bytes(rng, 1 << 16)])
    with pytest.raises(ValueError, match="capacity"):
        st.batch_write_device([b"c"], big, boffs, blens)
    unchanged()
    with pytest.raises(ValueError, match="blob"):
        st.batch_write_device([b"c"], blob.cpu(), offs[:1], lens[:1])
    with pytest.raises(ValueError, match="Mismatched"):
        st.batch_write_device([b"c"], blob, offs, lens)
    unchanged()
    assert st.batch_write_device([], blob, [], []) == tail


# -- copy / transfer / rename ------------------------------------------------------------------

class Model:
    """The reference's sequence replayed with the oracle: write_entries, and
    write_entries(.., allow_null=True) for the deletes of the keys that are present."""

    def __init__(self):
        self.buf, self.tail, self.live = bytearray(), 0, {}

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


def same(store, model, probe):
    assert store.tail == model.tail and store.bytes() == bytes(model.buf)
    assert store.len() == len(model.live)
    assert store.batch_read(probe) == [model.live.get(k) for k in probe]
    assert store.verify(probe) == [True if k in model.live else None for k in probe]


def two_stores(ctx):
    rng = random.Random(31)
    src_pairs = [(b"s-%d" % i, nonzero_bytes(rng, n)) for i, n in enumerate([1, 70, 4097, 2 * CH + 17, 300, 44])]
    dst_pairs = [(b"t-0", nonzero_bytes(rng, 90)), (b"s-1", nonzero_bytes(rng, 33))]  # s-1 exists there: overwritten
    out = []
    for pairs in (src_pairs, dst_pairs):
        st, m = S.DeviceStore.create(2 << 20, ctx), Model()
        assert st.batch_write([k for k, _ in pairs], [p for _, p in pairs]) == m.write(pairs)
        out.append((st, m))
    return out


PROBE = [b"s-%d" % i for i in range(6)] + [b"t-0", b"n-0", b"n-1", b"absent"]


def test_batch_copy_transfer(ctx):
    (a, ma), (b, mb) = two_stores(ctx)
    keys = [b"s-3", b"s-0", b"s-1"]  # the multi-chunk payload first
    assert a.batch_copy(keys, b) == mb.write([(k, ma.live[k]) for k in keys])
    same(a, ma, PROBE)
    same(b, mb, PROBE)
    assert a.copy(b"s-4", b) == mb.write([(b"s-4", ma.live[b"s-4"])])
    same(b, mb, PROBE)
    # transfer: copy, then delete at the source; returns the source's new tail
    keys = [b"s-2", b"s-5"]
    mb.write([(k, ma.live[k]) for k in keys])
    assert a.batch_transfer(keys, b) == ma.delete(keys)
    same(a, ma, PROBE)
    same(b, mb, PROBE)
    mb.write([(b"s-0", ma.live[b"s-0"])])
    assert a.transfer(b"s-0", b) == ma.delete([b"s-0"])
    same(a, ma, PROBE)
    same(b, mb, PROBE)


def test_batch_rename(ctx):
    (a, ma), _ = two_stores(ctx)
    olds, news = [b"s-3", b"s-1"], [b"n-0", b"n-1"]
    ma.write([(n, ma.live[o]) for o, n in zip(olds, news)])
    assert a.batch_rename(olds, news) == ma.delete(olds)
    same(a, ma, PROBE)
    # onto a key that exists: it is overwritten
    ma.write([(b"s-0", ma.live[b"n-0"])])
    assert a.rename(b"n-0", b"s-0") == ma.delete([b"n-0"])
    same(a, ma, PROBE)
    f = np.frombuffer(bytes(ma.buf), np.uint8)
    assert O.recover_valid_chain(f) == ma.tail


def test_copy_rename_errors_change_nothing(ctx):
    (a, ma), (b, mb) = two_stores(ctx)
    ma.delete([b"s-4"])
    assert a.batch_delete([b"s-4"]) == ma.tail  # a tombstoned key reads as None

    def unchanged():
        same(a, ma, PROBE)
        same(b, mb, PROBE)

    for bad in ([b"s-0", b"absent"], [b"s-4"], [b"s-0", b"s-4", b"s-1"]):
        with pytest.raises(KeyError):
            a.batch_copy(bad, b)
        with pytest.raises(KeyError):
            a.batch_transfer(bad, b)
        with pytest.raises(KeyError):
            a.batch_rename(bad, [b"x-%d" % i for i in range(len(bad))])
        unchanged()
    with pytest.raises(ValueError, match="Use `rename` instead"):
        a.batch_copy([b"s-0"], a)
    with pytest.raises(ValueError, match="Use `rename` instead"):
        a.copy(b"s-0", a)
    with pytest.raises(ValueError, match="Duplicate"):
        a.batch_copy([b"s-0", b"s-1", b"s-0"], b)
    with pytest.raises(ValueError, match="Duplicate"):
        a.batch_transfer([b"s-0", b"s-0"], b)
    with pytest.raises(ValueError, match="Cannot rename a key to itself"):
        a.batch_rename([b"s-0", b"s-1"], [b"n-0", b"s-1"])
    with pytest.raises(ValueError, match="Cannot rename a key to itself"):
        a.rename(b"s-0", b"s-0")
    with pytest.raises(ValueError, match="Duplicate"):
        a.batch_rename([b"s-0", b"s-1"], [b"n-0", b"n-0"])
    with pytest.raises(ValueError, match="Duplicate"):
        a.batch_rename([b"s-0", b"s-0"], [b"n-0", b"n-1"])
    with pytest.raises(ValueError, match="Duplicate"):  # a new key that is also an old key of the batch
        a.batch_rename([b"s-0", b"s-1"], [b"s-1", b"n-0"])
    with pytest.raises(ValueError, match="Mismatched"):
        a.batch_rename([b"s-0"], [b"n-0", b"n-1"])
    unchanged()
