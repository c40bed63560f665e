"""Verified payloads on the device: srd_payload_gather_device (a batch of
ranges copied into one packed buffer, each payload's CRC-32 computed on the way
and compared with the checksum stored in its metadata -- a read's bytes plus
EntryHandle::is_valid_checksum, entry_handle.rs:260-275) and the Python layers
over it (DeviceIndex.batch_gather, DeviceStore.batch_gather / verify /
iter_gather).

Expected values come from the oracle (O.write_entries, O.crc32,
O.crc32_ranges) over a host copy of the store; every comparison is bit-exact.
The shapes are the smallest at which the kernel can go wrong, C = GATHER_CHUNK:
the 16-byte piece, the 64-byte line, the 1 KiB lane row, the 4 KiB block in
both ring roles, and the chunk."""
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
SLACK = 4096


@pytest.fixture(scope="module")
def ctx():
    c = S.Context(0)
    yield c
    c.close()


def pad64(n):
    return (n + 63) & ~63


def kh(name):
    return O.xxh3_64(name)


def build_lengths_store():
    """One oracle-written entry per length in LENGTHS (random bytes), one
    all-0xFF payload, one zero-heavy payload, one tombstoned key."""
    rng = random.Random(0x6A7E)
    ents = [(b"len-%d" % n, rng.randbytes(n)) for n in LENGTHS]
    ents.append((b"all-ff", b"\xff" * 5000))
    zh = bytearray(9000)
    zh[0], zh[4096], zh[8999] = 1, 7, 9
    ents.append((b"zero-heavy", bytes(zh)))
    ents.append((b"gone", rng.randbytes(300)))
    buf = bytearray()
    tail = O.write_entries(buf, 0, [(kh(k), p) for k, p in ents])
    tail = O.write_entries(buf, tail, [(kh(b"gone"), b"\x00")], allow_null=True)
    assert tail == len(buf)
    return bytes(buf), ents


def host_ranges(f):
    """{key_hash: (start, end) | None} of the latest entries, from the oracle's chain."""
    out = {}
    for e in O.chain(np.frombuffer(f, np.uint8), len(f)):
        out[e["key_hash"]] = None if e["is_tombstone"] else (e["payload_start"], e["meta_off"])
    return out


@pytest.fixture(scope="module")
def lstore():
    f, ents = build_lengths_store()
    rg = host_ranges(f)
    assert rg[kh(b"gone")] is None
    for k, p in ents[:-1]:
        a, b = rg[kh(k)]
        assert f[a:b] == p and a % 64 == 0
    return f, ents, rg


def to_dev(f):
    import torch
    dev = torch.zeros(S.padded_size(len(f)), dtype=torch.uint8, device="cuda")
    dev[: len(f)] = torch.frombuffer(bytearray(f), dtype=torch.uint8).cuda()
    torch.cuda.synchronize()  # the library launches on its own stream, not ordered behind torch's
    return dev


def index_for(ctx, f):
    import torch
    idx = O.key_indexer_build(np.frombuffer(f, np.uint8), len(f))
    k = torch.from_numpy(np.array(list(idx.keys()), np.uint64).view(np.int64)).cuda()
    v = torch.from_numpy(np.array(list(idx.values()), np.uint64).view(np.int64)).cuda()
    torch.cuda.synchronize()
    return S.DeviceIndex(k.data_ptr(), v.data_ptr(), len(idx), ctx)


def dev_u64(a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a, np.uint64).view(np.int64)).cuda()


class Raw:
    """One raw srd_payload_gather_device call with sentinel-filled outputs."""

    def __init__(self, ctx, d_file, flen, st, en, flags=0, out="fit", cap=None):
        import torch
        n = len(st)
        self.n = n
        d_st, d_en = dev_u64(st), dev_u64(en)
        offs = torch.full((n + 1,), -1, dtype=torch.int64, device="cuda")
        status = torch.full((max(n, 1),), 0xEE, dtype=torch.uint8, device="cuda")
        crc = torch.full((max(n, 1),), 0x5A5A5A5A, dtype=torch.int32, device="cuda")
        tot = C.c_uint64(12345)
        call = S.lib().srd_payload_gather_device

        def run(fl, d_out, out_cap, d_crc):
            torch.cuda.synchronize()
            rc = call(ctx.h, C.c_void_p(d_file), flen, C.c_void_p(d_st.data_ptr()), C.c_void_p(d_en.data_ptr()), n, fl,
                      C.c_void_p(d_out), out_cap, C.c_void_p(offs.data_ptr()), C.c_void_p(status.data_ptr()),
                      C.c_void_p(d_crc), C.byref(tot), C.c_void_p(ctx.stream))
            torch.cuda.synchronize()
            return rc

        self.out = None
        if isinstance(out, str) and out == "layout":
            self.rc = run(flags, None, 0, None)
        elif isinstance(out, str):  # "fit": the layout call sizes d_out: the total + SLACK, all FILL
            self.rc = run(0, None, 0, None)
            assert self.rc == 0, S.lib().srd_last_error()
            self.layout_offs = offs.cpu().numpy().view(np.uint64).copy()
            total = int(tot.value)
            buf = torch.full((total + SLACK,), FILL, dtype=torch.uint8, device="cuda")
            self.rc = run(flags, buf.data_ptr(), total if cap is None else cap, crc.data_ptr())
            self.out = buf.cpu().numpy()
        else:  # a caller's buffer (tensor) of the given capacity
            self.rc = run(flags, out.data_ptr(), cap, crc.data_ptr())
            self.out = out.cpu().numpy()
        self.total = int(tot.value)
        self.offs = offs.cpu().numpy().view(np.uint64)
        self.status = status[:n].cpu().numpy()
        self.crc = crc[:n].cpu().numpy().view(np.uint32)


def check_packed(out, offs, total, want):
    """want[i] = payload bytes or None: offsets are the exclusive sum of the
    padded lengths, bytes right, padding zero, nothing at or past the total touched."""
    o = 0
    for i, p in enumerate(want):
        assert int(offs[i]) == o, i
        if p is not None:
            assert out[o: o + len(p)].tobytes() == p, (i, len(p))
            assert not out[o + len(p): o + pad64(len(p))].any(), (i, len(p))
            o += pad64(len(p))
    assert int(offs[len(want)]) == o == total
    assert (out[total:] == FILL).all() and out.size == total + SLACK


def queries(lstore, seed=1):
    """Every key, shuffled, with duplicates, the tombstoned key and two missing keys."""
    f, ents, rg = lstore
    rng = random.Random(seed)
    names = [k for k, _ in ents] + [b"missing-1", b"missing-2"]
    names += rng.sample(names, 9)
    rng.shuffle(names)
    pay = dict(ents)
    want = [pay[k] if rg.get(kh(k)) else None for k in names]
    return names, want


def expect_clean(want):
    st = [S.GATHER_OK if p is not None else S.GATHER_NONE for p in want]
    crc = [O.crc32(p) if p is not None else 0 for p in want]
    return st, crc


def test_lengths(ctx, lstore):
    f, ents, rg = lstore
    dev = to_dev(f)
    names, want = queries(lstore)
    st_want, crc_want = expect_clean(want)
    # through the index
    idx = index_for(ctx, f)
    r = idx.batch_gather(dev.data_ptr(), len(f), [kh(k) for k in names], names)
    assert r.payloads() == want
    assert list(r.status) == st_want and [int(x) for x in r.crc_computed] == crc_want
    assert [int(x) for x in r.lens] == [len(p) if p is not None else 0 for p in want]
    assert r.is_valid_checksum() == [None if p is None else True for p in want]
    assert r.data.numel() == int(r.offs[-1]) == sum(pad64(len(p)) for p in want if p is not None)
    # through raw ranges (a None read is start == end == 0)
    rr = [rg.get(kh(k)) or (0, 0) for k in names]
    g = Raw(ctx, dev.data_ptr(), len(f), [a for a, _ in rr], [b for _, b in rr])
    assert g.rc == 0
    check_packed(g.out, g.offs, g.total, want)
    assert list(g.status) == st_want and [int(x) for x in g.crc] == crc_want
    assert (g.layout_offs == g.offs).all()


def corrupt(lstore):
    """The flips of test 2 on a host mirror: {key: position} plus one metadata flip."""
    f, ents, rg = lstore
    pos = [0, 15, 16, 1023, 1024, 4095, 4096, CH - 1, CH]
    used, flips = set(), {}
    by_len = sorted((len(p), k) for k, p in ents[:len(LENGTHS)])
    for q in pos:
        n, k = next((n, k) for n, k in by_len if n > q and k not in used)
        used.add(k)
        flips[k] = q
    n, k = next((n, k) for n, k in reversed(by_len) if k not in used)
    used.add(k)
    flips[k] = n - 1  # a last byte
    meta_key = next(k for _, k in by_len if k not in used and _ > 100)
    g = bytearray(f)
    for k, q in flips.items():
        g[rg[kh(k)][0] + q] ^= 0xFF
    g[rg[kh(meta_key)][1] + 17] ^= 0x40  # a byte of the stored checksum
    return bytes(g), flips, meta_key


def flip_on_device(dev, f, g):
    import torch
    d = np.nonzero(np.frombuffer(f, np.uint8) != np.frombuffer(g, np.uint8))[0]
    dev[torch.from_numpy(d).cuda()] = torch.from_numpy(np.frombuffer(g, np.uint8)[d].copy()).cuda()
    torch.cuda.synchronize()


def test_corruption_is_reported_not_hidden(ctx, lstore):
    f, ents, rg = lstore
    g, flips, meta_key = corrupt(lstore)
    assert len(flips) == 10
    dev = to_dev(f)
    flip_on_device(dev, f, g)
    names, _ = queries(lstore, seed=2)
    want = [g[rg[kh(k)][0]: rg[kh(k)][1]] if rg.get(kh(k)) else None for k in names]
    bad = set(flips) | {meta_key}
    st_want = [S.GATHER_NONE if p is None else S.GATHER_BAD_CRC if k in bad else S.GATHER_OK for k, p in zip(names, want)]
    assert st_want.count(S.GATHER_BAD_CRC) >= 11
    rr = [rg.get(kh(k)) or (0, 0) for k in names]
    r = Raw(ctx, dev.data_ptr(), len(f), [a for a, _ in rr], [b for _, b in rr])
    assert r.rc == 0
    assert list(r.status) == st_want
    assert [int(x) for x in r.crc] == [O.crc32(p) if p is not None else 0 for p in want]
    check_packed(r.out, r.offs, r.total, want)  # the copied bytes are the flipped bytes


@pytest.mark.parametrize("flipped", [False, True])
def test_verify_only(ctx, lstore, flipped):
    import torch
    f, ents, rg = lstore
    g, flips, meta_key = corrupt(lstore) if flipped else (f, {}, None)
    dev = to_dev(f)
    if flipped:
        flip_on_device(dev, f, g)
    names, _ = queries(lstore, seed=3)
    want = [g[rg[kh(k)][0]: rg[kh(k)][1]] if rg.get(kh(k)) else None for k in names]
    bad = set(flips) | {meta_key}
    st_want = [S.GATHER_NONE if p is None else S.GATHER_BAD_CRC if k in bad else S.GATHER_OK for k, p in zip(names, want)]
    rr = [rg.get(kh(k)) or (0, 0) for k in names]
    sentinel = torch.full((1 << 20,), FILL, dtype=torch.uint8, device="cuda")
    r = Raw(ctx, dev.data_ptr(), len(f), [a for a, _ in rr], [b for _, b in rr], S.GATHER_VERIFY_ONLY, out=sentinel,
            cap=sentinel.numel())
    assert r.rc == 0
    assert list(r.status) == st_want
    assert [int(x) for x in r.crc] == [O.crc32(p) if p is not None else 0 for p in want]
    assert (r.out == FILL).all()
    # and through the index: the same answers, no data
    idx = index_for(ctx, f)
    v = idx.batch_gather(dev.data_ptr(), len(f), [kh(k) for k in names], None, S.GATHER_VERIFY_ONLY)
    assert v.data is None and list(v.status) == st_want
    assert v.is_valid_checksum() == [None if s == S.GATHER_NONE else s == S.GATHER_OK for s in st_want]


def test_caller_made_ranges(ctx, lstore):
    """Ranges no read call made: odd start alignments, a range ending inside a
    payload (its "stored checksum" is whatever bytes follow), and ranges that do
    not lie in the file -- refused by arithmetic before any access.  The store
    sits at the end of its allocation."""
    import torch
    f, ents, rg = lstore
    flen = len(f)
    big = torch.zeros(32 << 20, dtype=torch.uint8, device="cuda")
    at = big.numel() - pad64(flen)
    big[at: at + flen] = torch.frombuffer(bytearray(f), dtype=torch.uint8).cuda()
    torch.cuda.synchronize()
    d_file = big.data_ptr() + at
    a0, b0 = rg[kh(b"len-%d" % (3 * CH + 4097))]
    a1, b1 = rg[kh(b"len-8193")]
    a2, b2 = rg[kh(b"len-1040")]
    cases = [(a0 + 1, b0), (a0 + 5, b0 - 3 * CH), (a1 + 63, b1), (a2 + 1, a2 + 2), (a0 + 5, a0 + 5 + 2 * CH),
             (a0, a0 + CH + 100),  # ends inside a payload, aligned start
             (a1, b1),             # a real entry between them
             (b1, a1),             # start > end
             (a1, flen - 19),      # end + 20 == file_len + 1
             (0, 1 << 63), (5, (1 << 64) - 1), (flen, flen + 1),
             (0, 0), ((1 << 64) - 1, (1 << 64) - 1)]
    n_ok = 7
    want = [f[a:b] for a, b in cases[:n_ok]] + [None] * (len(cases) - n_ok)
    r = Raw(ctx, d_file, flen, [a for a, _ in cases], [b for _, b in cases])
    assert r.rc == 0
    check_packed(r.out, r.offs, r.total, want)
    st_want = []
    for a, b in cases[:n_ok]:
        stored = int.from_bytes(f[b + 16: b + 20], "little")
        st_want.append(S.GATHER_OK if stored == O.crc32(f[a:b]) else S.GATHER_BAD_CRC)
    assert st_want == [S.GATHER_BAD_CRC] * 6 + [S.GATHER_OK]
    st_want += [S.GATHER_BAD_RANGE] * 5 + [S.GATHER_NONE] * 2
    assert list(r.status) == st_want
    assert [int(x) for x in r.crc] == [O.crc32(p) if p is not None else 0 for p in want]


REALIGN_LENGTHS = [1, 15, 16, 17, 33, 4095, 4097, CH + 1, 2 * CH + 17]


@pytest.fixture(scope="module")
def realign_hits():
    """Hand-made hits at every start residue mod 16 and every length of
    REALIGN_LENGTHS: random payload bytes, 16 arbitrary bytes, the little-endian
    CRC-32 of the payload at end + 16.  (file bytes, [(start, end)], [payload])"""
    rng = random.Random(0xA116)
    buf, ranges, pays = bytearray(rng.randbytes(7)), [], []
    for res in range(16):
        for n in REALIGN_LENGTHS:
            buf += rng.randbytes(1 + (res - len(buf) - 1) % 16)  # (at least one byte between two hits)
            assert len(buf) % 16 == res
            p = rng.randbytes(n)
            ranges.append((len(buf), len(buf) + n))
            pays.append(p)
            buf += p + rng.randbytes(16) + O.crc32(p).to_bytes(4, "little")
    return bytes(buf), ranges, pays


def shifted_dev(f, shift):
    """The file on the device at an address that is `shift` mod 16."""
    import torch
    dev = torch.zeros(S.padded_size(len(f)) + 64, dtype=torch.uint8, device="cuda")
    assert dev.data_ptr() % 16 == 0
    dev[shift: shift + len(f)] = torch.frombuffer(bytearray(f), dtype=torch.uint8).cuda()
    torch.cuda.synchronize()
    return dev, dev.data_ptr() + shift


@pytest.mark.parametrize("shift", [0, 1])
def test_realigned_sources(ctx, realign_hits, shift):
    """Sources that are not 16-byte aligned to the packed output (every start
    residue, the file base aligned and not): the streaming kernel assembles each
    destination vector from two source vectors.  A copying and a verify-only
    call; bytes, padding, statuses and CRCs against the oracle."""
    import torch
    f, ranges, pays = realign_hits
    dev, d_file = shifted_dev(f, shift)
    st, en = [a for a, _ in ranges], [b for _, b in ranges]
    crc_want = [O.crc32(p) for p in pays]
    r = Raw(ctx, d_file, len(f), st, en)
    assert r.rc == 0
    assert list(r.status) == [S.GATHER_OK] * len(pays) and [int(x) for x in r.crc] == crc_want
    check_packed(r.out, r.offs, r.total, pays)
    sentinel = torch.full((r.total + SLACK,), FILL, dtype=torch.uint8, device="cuda")
    v = Raw(ctx, d_file, len(f), st, en, S.GATHER_VERIFY_ONLY, out=sentinel, cap=sentinel.numel())
    assert v.rc == 0
    assert list(v.status) == [S.GATHER_OK] * len(pays) and [int(x) for x in v.crc] == crc_want
    assert (v.out == FILL).all()


def test_realigned_flip_is_reported(ctx, realign_hits):
    """One flipped byte in the second chunk of a multi-chunk hit at start
    residue 5: that status, and only that one, is BAD_CRC."""
    f, ranges, pays = realign_hits
    i = 5 * len(REALIGN_LENGTHS) + REALIGN_LENGTHS.index(2 * CH + 17)
    assert ranges[i][0] % 16 == 5 and ranges[i][1] - ranges[i][0] == 2 * CH + 17
    g = bytearray(f)
    g[ranges[i][0] + CH + 100] ^= 0x10
    flipped = [bytes(g[a:b]) for a, b in ranges]
    dev, d_file = shifted_dev(bytes(g), 1)
    r = Raw(ctx, d_file, len(f), [a for a, _ in ranges], [b for _, b in ranges])
    assert r.rc == 0
    assert list(r.status) == [S.GATHER_BAD_CRC if j == i else S.GATHER_OK for j in range(len(pays))]
    assert [int(x) for x in r.crc] == [O.crc32(p) for p in flipped]
    check_packed(r.out, r.offs, r.total, flipped)


def test_many_units_per_wave(ctx):
    import torch
    n = 300_000
    lens = np.clip(S.zipf_lens(n), 1, 200)
    flen = S.synth_store_len(n, lens=lens)
    dev = torch.zeros(S.padded_size(flen), dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()
    assert S.synth_store_device(dev.data_ptr(), n, lens=lens, ctx=ctx) == flen
    res = S.validate_index_device(dev.data_ptr(), flen, 0, ctx)
    assert res.final_len == flen and res.n_chain == n
    offs = torch.empty(n + 1, dtype=torch.int64, device="cuda")
    status = torch.empty(n, dtype=torch.uint8, device="cuda")
    crc = torch.empty(n, dtype=torch.int32, device="cuda")
    torch.cuda.synchronize()
    args = (dev.data_ptr(), flen, res.payload_start, res.meta_off, n)
    total = S.payload_gather_device(*args, 0, None, 0, offs.data_ptr(), status.data_ptr(), None, ctx)
    out = torch.full((total + SLACK,), FILL, dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()
    assert S.payload_gather_device(*args, 0, out.data_ptr(), total, offs.data_ptr(), status.data_ptr(), crc.data_ptr(),
                                   ctx) == total
    torch.cuda.synchronize()
    st = S.device_to_numpy(res.payload_start, n)
    en = S.device_to_numpy(res.meta_off, n)
    host = dev[:flen].cpu().numpy()
    ln = (en - st).astype(np.int64)
    assert (ln == lens.astype(np.int64)).all()
    assert (status.cpu().numpy() == S.GATHER_OK).all()
    assert (crc.cpu().numpy().view(np.uint32) == O.crc32_ranges(host, st, ln.astype(np.uint64), threads=16)).all()
    pl = (ln + 63) & ~63
    o_want = np.concatenate([[0], np.cumsum(pl)]).astype(np.uint64)
    assert (offs.cpu().numpy().view(np.uint64) == o_want).all() and total == int(o_want[-1])
    # the output against a numpy gather: payload bytes in place, zero elsewhere below the total
    want = np.zeros(total + SLACK, np.uint8)
    want[total:] = FILL
    within = np.arange(int(ln.sum()), dtype=np.int64) - np.repeat(np.cumsum(ln) - ln, ln)
    want[np.repeat(o_want[:-1].astype(np.int64), ln) + within] = host[np.repeat(st.astype(np.int64), ln) + within]
    assert (out.cpu().numpy() == want).all()


def test_capacity_overlap_and_edges(ctx, lstore):
    import torch
    f, ents, rg = lstore
    dev = to_dev(f)
    names, want = queries(lstore, seed=4)
    rr = [rg.get(kh(k)) or (0, 0) for k in names]
    st, en = [a for a, _ in rr], [b for _, b in rr]
    full = Raw(ctx, dev.data_ptr(), len(f), st, en)
    assert full.rc == 0
    # out_cap = total - 1: refused, the total still reported, nothing written
    r = Raw(ctx, dev.data_ptr(), len(f), st, en, cap=full.total - 1)
    assert r.rc == S.SRD_ERR_ARG and r.total == full.total
    assert (r.out == FILL).all() and (r.crc == 0x5A5A5A5A).all()
    lay_status = [0xEE if p is not None else S.GATHER_NONE for p in want]  # (Raw's own layout call wrote the Nones)
    assert [int(x) for x in r.status] == lay_status
    # d_out inside the store
    inside = dev[4096:]
    r = Raw(ctx, dev.data_ptr(), len(f), st, en, out=inside, cap=inside.numel())
    assert r.rc == S.SRD_ERR_ARG and (r.status == 0xEE).all()
    assert r.out[: len(f) - 4096].tobytes() == f[4096:]
    # the layout-only call: the same offsets, None / bad-range statuses only
    lay = Raw(ctx, dev.data_ptr(), len(f), st + [7], en + [3], out="layout")
    assert lay.rc == 0 and lay.total == full.total
    assert (lay.offs[:-1] == full.offs).all() and int(lay.offs[-1]) == full.total
    assert [int(x) for x in lay.status] == lay_status + [S.GATHER_BAD_RANGE]
    # n = 0 and an all-None batch
    r = Raw(ctx, dev.data_ptr(), len(f), [], [])
    assert r.rc == 0 and r.total == 0 and list(r.offs) == [0] and (r.out == FILL).all()
    r = Raw(ctx, dev.data_ptr(), len(f), [0, 9, 64], [0, 9, 64])
    assert r.rc == 0 and r.total == 0 and list(r.offs) == [0, 0, 0, 0] and (r.out == FILL).all()
    assert list(r.status) == [S.GATHER_NONE] * 3 and list(r.crc) == [0, 0, 0]
    # n >= 2^31
    tot = C.c_uint64()
    assert S.lib().srd_payload_gather_device(ctx.h, C.c_void_p(dev.data_ptr()), len(f), C.c_void_p(dev.data_ptr()),
                                             C.c_void_p(dev.data_ptr()), 1 << 31, 0, None, 0,
                                             C.c_void_p(dev.data_ptr()), C.c_void_p(dev.data_ptr()), None, C.byref(tot),
                                             C.c_void_p(ctx.stream)) == S.SRD_ERR_ARG
    assert ctx.device_bytes() > 0  # the workspace is the context's


def test_session(ctx):
    """create -> batch_write -> batch_gather -> overwrite -> delete -> batch_gather:
    the gather agrees with batch_read at every step, validity all True."""
    import torch
    rng = random.Random(77)
    s = S.DeviceStore.create(16 << 20, ctx)
    keys = [b"k%d" % i for i in range(40)]
    pay = {k: rng.randbytes(rng.choice([1, 17, 64, 1000, 4096, 5000, CH + 3])) for k in keys}
    probe = keys + [b"nope"]

    def agree():
        rd = s.batch_read(probe)
        g = s.batch_gather(probe)
        assert g.payloads() == rd
        assert g.is_valid_checksum() == [None if p is None else True for p in rd]
        assert s.verify(probe) == g.is_valid_checksum()
        gh = s.batch_gather_hashed_keys([kh(k) for k in probe], probe)
        assert gh.payloads() == rd
        return rd

    s.batch_write(keys, [pay[k] for k in keys])
    assert agree() == [pay[k] for k in keys] + [None]
    for k in keys[:10]:
        pay[k] = rng.randbytes(rng.choice([3, 4097, 2 * CH]))
    s.batch_write(keys[:10], [pay[k] for k in keys[:10]])
    agree()
    s.batch_delete(keys[5:15])
    rd = agree()
    assert rd == [None if 5 <= i < 15 else pay[k] for i, k in enumerate(keys)] + [None]
    # iter_gather: EntryIterator order, the payloads of iter_entries_device's ranges
    _k, p = s.index.export()
    st, en, _mo, _kh = S.iter_entries_device(s.buf.data_ptr(), s.tail, p.data_ptr(), p.numel(), ctx)
    host = s.bytes()
    it = s.iter_gather()
    assert it.payloads() == [host[int(a): int(b)] for a, b in zip(st, en)] and len(it) == 30
    assert all(it.is_valid_checksum())
    # a byte poked into the buffer: verify reports exactly that key
    victim = keys[20]
    a, _b = s._ranges([kh(victim)], None)
    s.buf[int(a[0]) + len(pay[victim]) // 2] ^= 0x01
    torch.cuda.synchronize()
    assert s.verify(probe) == [None if (5 <= i < 15 or k == b"nope") else k != victim for i, k in enumerate(probe)]
