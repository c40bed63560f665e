"""Chunk units at many chunks per hit and many units per wave: the shapes of
units_kernel / stream_copy_crc_kernel / unit_terms_kernel + unit_combine_kernel that the
length lists of test_gpu_gather.py, test_gpu_append.py and
test_gpu_compact_live.py do not reach, through all three callers
(srd_payload_gather_device, srd_batch_append_device, DeviceStore.compact).

A. Hits of 63..130 chunks: the combine's lanes stride over a hit's units by
   64, in 1, 2 and 3 rounds, with an empty lane, full rounds and rounds that
   only the first lanes take.
B. Batches of at least 2.5 W units, W = the grid's waves: every wave walks
   from one unit to the next, over every ordered pair of block counts (1, 2,
   3, 5, 16), of source alignments, and across the end of a multi-chunk hit.
C. The stream rule when an all-zero payload's unit follows a nonzero unit in
   the same wave: refused, as the reference's write_stream refuses it.

The batches and the conditions they must meet are tests/test_chunk_unit_batches.py's
(checked there without a GPU for three grid sizes, asserted again here for the
device's own).  Expected values come from the oracle (O.crc32, O.crc32_ranges,
O.write_entries, model_compact); every comparison is bit-exact, output buffers
are 0xA5 before a call and checked over the whole allocation, result arrays are
sentinel-filled (the helpers of the three files named above)."""
import random

import numpy as np
import pytest

import oracle as O
import srd_amd as S
import test_chunk_unit_batches as U
import test_gpu_append as A
import test_gpu_compact_live as K
import test_gpu_gather as G

pytestmark = pytest.mark.gpu

CH = S.GATHER_CHUNK
FILL = 0xA5
NONE = (1 << 64) - 1
NULL_ONLY = "NULL-byte-only streams cannot be written directly."


@pytest.fixture(scope="module")
def ctx():
    c = S.Context(0)
    yield c
    c.close()


@pytest.fixture(scope="module")
def W():
    """The waves of stream_copy_crc_kernel's grid once a batch has a unit for each: SCAN_WAVES_V2 = 16 per block,
    one block per CU (U.WAVES_PER_BLOCK names the launch line)."""
    import torch
    return U.WAVES_PER_BLOCK * torch.cuda.get_device_properties(0).multi_processor_count


def pad64(n):
    return (n + 63) & ~63


def kh(name):
    return O.xxh3_64(name)


def random_payloads(lens, seed):
    """(one blob of random bytes holding the payloads back to back, their offsets, the payloads): the first byte
    of every payload is not 0."""
    offs = U.packed_offsets(lens)
    blob = np.random.default_rng(seed).integers(0, 256, int(sum(lens)), dtype=np.uint8)
    blob[offs] |= 1
    raw = blob.tobytes()
    return blob, offs, [raw[int(o): int(o) + n] for o, n in zip(offs, lens)]


def random_hashes(n, seed):
    h = [int(x) for x in np.random.default_rng(seed).integers(0, 1 << 63, n).astype(np.uint64)]
    assert len(set(h)) == n
    return h


def to_cuda(blob):
    import torch
    t = torch.from_numpy(blob).cuda()
    assert t.data_ptr() % 16 == 0  # U.unit_table's alignments are offsets from a 16-aligned base
    return t


def sentinel_out():
    import torch
    return torch.full((1 << 20,), FILL, dtype=torch.uint8, device="cuda")


def append_equals_oracle(ctx, prefix, blob_t, offs, lens, hashes, flags, want, want_mo):
    """One srd_batch_append_device call onto `prefix`: the whole allocation and the offsets against the oracle's."""
    dev = A.Dev(prefix, len(want) - len(prefix))
    rc, nt, mo, msg = A.append(ctx, dev, blob_t, offs, lens, hashes, flags)
    assert rc == 0, msg
    assert nt == len(want)
    dev.check(want)
    assert mo == want_mo
    return dev


# -- A. many chunks per hit: the combine's lane split ------------------------------------------------------

@pytest.fixture(scope="module")
def combine():
    """(keys, payloads, their CRC-32) of U.COMBINE_LENGTHS."""
    _blob, _offs, pays = random_payloads(U.COMBINE_LENGTHS, 0xA1)
    return [b"k-%d" % k for k in U.COMBINE_K], pays, [O.crc32(p) for p in pays]


@pytest.fixture(scope="module")
def combine_appended(combine):
    names, pays, _ = combine
    prefix = A.store_with_residue(1)
    hashes = [kh(k) for k in names]
    want, want_mo = A.oracle_append(prefix, hashes, pays)
    return prefix, hashes, want, want_mo


def test_combine_gather(ctx, combine):
    names, pays, crcs = combine
    seg65, seg129 = U.lane_split(65), U.lane_split(129)
    assert seg65[0] == [0, 64] and all(us == [l] for l, us in enumerate(seg65) if l)
    assert seg129[0] == [0, 64, 128] and all(us == [l, l + 64] for l, us in enumerate(seg129) if l)
    buf = bytearray()
    O.write_entries(buf, 0, [(kh(k), p) for k, p in zip(names, pays)])
    f = bytes(buf)
    rg = G.host_ranges(f)
    st, en = [rg[kh(k)][0] for k in names], [rg[kh(k)][1] for k in names]
    assert all(f[a:b] == p for a, b, p in zip(st, en, pays))
    dev = G.to_dev(f)
    n = len(names)
    g = G.Raw(ctx, dev.data_ptr(), len(f), st, en)
    assert g.rc == 0
    assert list(g.status) == [S.GATHER_OK] * n and [int(x) for x in g.crc] == crcs
    G.check_packed(g.out, g.offs, g.total, pays)
    assert (g.layout_offs == g.offs).all()
    out = sentinel_out()
    v = G.Raw(ctx, dev.data_ptr(), len(f), st, en, S.GATHER_VERIFY_ONLY, out=out, cap=out.numel())
    assert v.rc == 0 and (v.out == FILL).all()
    assert list(v.status) == [S.GATHER_OK] * n and [int(x) for x in v.crc] == crcs
    # one flipped byte per position in the k = 65 and the k = 129 hit: reported with the flipped bytes' CRC
    victims = [U.COMBINE_K.index(65), U.COMBINE_K.index(129)]
    pos = {i: U.combine_flip_positions(len(pays[i])) for i in victims}
    assert len(pos[victims[0]]) == len(pos[victims[1]]) == 5
    cur = f
    for q in range(5):
        g2 = bytearray(f)
        for i in victims:
            g2[st[i] + pos[i][q]] ^= 0xFF
        g2 = bytes(g2)
        G.flip_on_device(dev, cur, g2)
        cur = g2
        want = [g2[a:b] for a, b in zip(st, en)]
        assert [w != p for w, p in zip(want, pays)] == [i in victims for i in range(n)]
        r = G.Raw(ctx, dev.data_ptr(), len(f), st, en)
        assert r.rc == 0
        assert list(r.status) == [S.GATHER_BAD_CRC if i in victims else S.GATHER_OK for i in range(n)], q
        assert [int(x) for x in r.crc] == [O.crc32(w) for w in want], q
        G.check_packed(r.out, r.offs, r.total, want)  # the copied bytes are the flipped bytes


def test_combine_three_range_callers(ctx, combine):
    """The same seven ranges through the three range callers of the one combine: gathered, verified only, and
    copied into an empty store (batch_copy: the append under the stream rule).  Each reports the oracle's CRC-32
    per entry; the copied store is the oracle writer's."""
    names, pays, crcs = combine
    entries = [(kh(k), p) for k, p in zip(names, pays)]
    buf = bytearray()
    O.write_entries(buf, 0, entries)
    f = bytes(buf)
    rg = G.host_ranges(f)
    st, en = [rg[h][0] for h, _ in entries], [rg[h][1] for h, _ in entries]
    assert [b - a for a, b in zip(st, en)] == U.COMBINE_LENGTHS
    src = K.open_store(ctx, f)
    for flags in (0, S.GATHER_VERIFY_ONLY):
        out = sentinel_out() if flags else None
        g = G.Raw(ctx, src.buf.data_ptr(), len(f), st, en, flags, **({"out": out, "cap": out.numel()} if flags else {}))
        assert g.rc == 0 and list(g.status) == [S.GATHER_OK] * len(names), flags
        assert [int(x) for x in g.crc] == crcs, flags
    dst = S.DeviceStore.create(len(f) + 4096, ctx)
    assert src.batch_copy(names, dst) == len(f)
    got = dst.bytes()
    assert got == f  # (the oracle wrote the same entries to an empty store)
    # an entry's metadata follows its payload: key hash, prev offset, checksum
    assert [int.from_bytes(got[m + 16: m + 20], "little") for m in en] == crcs
    assert dst.batch_read(names) == pays


@pytest.mark.parametrize("flags", [0, S.APPEND_STREAM_RULE])
@pytest.mark.parametrize("residue", [0, 5])
def test_combine_append(ctx, combine, combine_appended, residue, flags):
    """Every source 16-aligned, and at residue 5: whole units on the byte path."""
    _names, pays, _ = combine
    prefix, hashes, want, want_mo = combine_appended
    assert len(prefix) % 64 == 1
    blob, offs = A.pack(pays, residue)
    assert all(o % 16 == residue for o in offs)
    dev = append_equals_oracle(ctx, prefix, to_cuda(blob), offs, [len(p) for p in pays], hashes, flags, want, want_mo)
    A.validate_matches_oracle(ctx, dev, want)


def combine_session(combine):
    """An oracle-written session: first versions of two of the keys and a second key holding the k = 64 payload,
    then the seven payloads (two of them overwrites), then that second key deleted."""
    names, pays, _ = combine
    rng = random.Random(0xA3)
    buf = bytearray()
    t = O.write_entries(buf, 0, [(kh(names[0]), K.nonzero_bytes(rng, 300)), (kh(names[3]), K.nonzero_bytes(rng, 5000)),
                                 (kh(b"gone"), pays[1])])
    t = O.write_entries(buf, t, [(kh(k), p) for k, p in zip(names, pays)])
    t = O.write_entries(buf, t, [(kh(b"gone"), b"\x00")], allow_null=True)
    assert t == len(buf)
    return bytes(buf)


def test_combine_compact(ctx, combine):
    names, pays, _ = combine
    f = combine_session(combine)
    want, its = K.model_compact(f, len(f))
    assert [k for _, _, _, k in its] == [kh(k) for k in reversed(names)]
    st = K.open_store(ctx, f)
    assert st.len() == 8  # (open's index holds the tombstoned key)
    s = st.compact()
    assert (int(s.n_entries), int(s.new_len), int(s.kept_bytes)) == (7, len(want), sum(len(p) + 20 for p in pays))
    assert int(s.n_crc_bad) == 0 and int(s.first_bad) == NONE
    assert st.tail == len(want) and st.len() == 7
    assert st.bytes() == want
    assert st.batch_read(names + [b"gone"]) == pays + [None]
    # one byte of the last lane's first unit of the k = 129 payload, flipped in the source of a fresh session
    st = K.open_store(ctx, f)
    a, _e, mo, _k = next(t for t in its if t[3] == kh(b"k-129"))
    lane = U.last_lane(129)
    q = a + U.lane_split(129)[lane][0] * CH + 7
    assert lane == 63 and q < mo
    st.buf[q] ^= 0x10
    flipped = bytearray(f)
    flipped[q] ^= 0x10
    state = (st.buf.data_ptr(), st.tail, st.index.table.data_ptr(), K.source_state(st))
    with pytest.raises(ValueError, match=r"n_crc_bad = 1, first_bad = %d\b" % mo):
        st.compact()
    assert (st.buf.data_ptr(), st.tail, st.index.table.data_ptr(), K.source_state(st)) == state
    s = st.compact(allow_bad_crc=True)
    assert int(s.n_crc_bad) == 1 and int(s.first_bad) == mo
    assert st.bytes() == K.model_compact(bytes(flipped), len(f))[0]


# -- B. more units than waves: the streaming kernel's walk from unit to unit --------------------------------

class Walk:
    """The batch of U.gen_lengths(W): payloads back to back in one blob (the append's source), their hashes and
    the unit table of that layout."""

    def __init__(self, W):
        self.W = W
        self.lens = U.gen_lengths(W)
        self.blob, self.offs, self.pays = random_payloads(self.lens, 0xB2)
        self.hashes = random_hashes(len(self.lens), 0xB3)
        self.tab = U.unit_table(self.lens, self.offs)
        self.prefix = A.store_with_residue(1)
        self._want = None

    def appended(self):
        """(the oracle's store after the batch, its metadata offsets), computed once."""
        if self._want is None:
            self._want = A.oracle_append(self.prefix, self.hashes, self.pays)
        return self._want


@pytest.fixture(scope="module")
def walk(W):
    return Walk(W)


def test_walk_gather(ctx, W, walk):
    lens, n = walk.lens, len(walk.lens)
    offs, flen = U.spaced_offsets(lens)
    U.check_coverage(U.unit_table(lens, offs), W)
    ends = offs + np.asarray(lens, np.int64)
    host = np.full(flen, 0xEE, np.uint8)
    for o, a, ln in zip(offs, walk.offs, lens):
        host[o: o + ln] = walk.blob[a: a + ln]
    crc = O.crc32_ranges(host, offs, lens, threads=16)
    planted = crc.copy()
    planted[1::2] ^= 0x80000001  # the correct checksum behind the even hits, a wrong one behind the odd hits
    for e, c in zip(ends, planted):
        host[e + 16: e + 20] = np.frombuffer(int(c).to_bytes(4, "little"), np.uint8)
    assert set(int(o) % 16 for o in offs) == set(range(16)) and int(ends[-1]) + 20 <= flen
    dev = G.to_dev(host.tobytes())
    assert dev.data_ptr() % 16 == 0
    st_want = [S.GATHER_BAD_CRC if i & 1 else S.GATHER_OK for i in range(n)]
    g = G.Raw(ctx, dev.data_ptr(), flen, offs, ends)
    assert g.rc == 0
    assert list(g.status) == st_want
    assert (g.crc == crc).all()
    G.check_packed(g.out, g.offs, g.total, walk.pays)  # per hit, by slices; padding 0; nothing above the total
    assert (g.layout_offs == g.offs).all()
    out = sentinel_out()
    v = G.Raw(ctx, dev.data_ptr(), flen, offs, ends, S.GATHER_VERIFY_ONLY, out=out, cap=out.numel())
    assert v.rc == 0 and (v.out == FILL).all()
    assert list(v.status) == st_want and (v.crc == crc).all()


@pytest.mark.parametrize("flags", [0, S.APPEND_STREAM_RULE])
def test_walk_append(ctx, W, walk, flags):
    U.check_coverage(walk.tab, W)
    want, want_mo = walk.appended()
    append_equals_oracle(ctx, walk.prefix, to_cuda(walk.blob), walk.offs, walk.lens, walk.hashes, flags, want, want_mo)


class Rounds:
    """U.compaction_plan(W) with bytes: the hashes, round 0's payloads in one blob, round 1's overwrites and
    deletes; `zero`: a key index whose round-0 payload is all 0."""

    def __init__(self, W, zero=None):
        self.r0, self.over, self.gone, self.live = U.compaction_plan(W)
        self.hashes = random_hashes(len(self.r0), 0xB4)
        self.blob, self.offs, self.p0 = random_payloads(self.r0, 0xB5)
        if zero is not None:
            a = int(self.offs[zero])
            self.blob[a: a + self.r0[zero]] = 0
            self.p0[zero] = bytes(self.r0[zero])
        _b, _o, self.p1 = random_payloads([n for _, n in self.over], 0xB6)
        self.live_lens = [n for _, n in self.live]
        self.tab = U.unit_table(self.live_lens)  # (every source is a payload start of the store: 64-aligned)

    def store(self, upto=None):
        """The oracle-written store: round 0 (its first `upto` entries only), then -- unless cut -- round 1."""
        buf = bytearray()
        t = O.write_entries(buf, 0, list(zip(self.hashes[:upto], self.p0[:upto])))
        if upto is None:
            t = O.write_entries(buf, t, [(self.hashes[i], p) for (i, _), p in zip(self.over, self.p1)])
            t = O.write_entries(buf, t, [(self.hashes[i], b"\x00") for i in self.gone], allow_null=True)
        assert t == len(buf)
        return bytes(buf)

    def reads(self):
        """What a read of every key returns."""
        rd = list(self.p0)
        for (i, _), p in zip(self.over, self.p1):
            rd[i] = p
        for i in self.gone:
            rd[i] = None
        return rd


def test_walk_compact(ctx, W):
    r = Rounds(W)
    U.check_coverage(r.tab, W, alignments=False)
    f = r.store()
    want, its = K.model_compact(f, len(f))
    # the compaction's hits are the plan's: the live entries newest first, each at a 64-byte boundary
    assert [(k, e - a) for a, e, _, k in its] == [(r.hashes[i], n) for i, n in r.live]
    assert all(a % 64 == 0 for a, _, _, _ in its)
    st = K.open_store(ctx, f)
    s = st.compact()
    assert (int(s.n_entries), int(s.new_len), int(s.kept_bytes)) == (len(its), len(want), sum(r.live_lens) + 20 * len(its))
    assert int(s.n_crc_bad) == 0 and int(s.first_bad) == NONE
    assert st.tail == len(want) and st.len() == len(its)
    assert st.bytes() == want
    rd = st.batch_read_hashed_keys(r.hashes)
    assert rd == r.reads()
    again = st.compact()  # (its hits are the same entries in the opposite order)
    assert int(again.n_entries) == len(its) and int(again.n_crc_bad) == 0
    assert st.batch_read_hashed_keys(r.hashes) == rd


# -- C. the stream rule when a zero payload is not its wave's first unit ----------------------------------------

def assert_placed(tab, W, lens, i, pays):
    """Every unit u of hit i is some wave's second or later unit, and that wave's previous unit u - W belongs to
    a payload with a byte that is not 0 and has 2 or more blocks."""
    first = int(tab["cpre"][i])
    for u in range(first, first + int(tab["k"][i])):
        assert u >= W and tab["hit"][u] == i
        prev = int(tab["hit"][u - W])
        assert prev != i and any(pays[prev]) and tab["blocks"][u - W] >= 2


@pytest.mark.parametrize("case", U.ZERO_CASES)
def test_zero_payload_behind_a_nonzero_unit(ctx, W, walk, case):
    lens, tab = walk.lens, walk.tab
    i = U.zero_placement(tab, W, lens, case)
    n, a = lens[i], int(walk.offs[i])
    pays = list(walk.pays)
    pays[i] = bytes(n)
    assert_placed(tab, W, lens, i, pays)
    assert {"three_blocks": 2 * 4096 < n <= 3 * 4096, "chunk_plus_one": n == CH + 1, "one_block_behind_16": n <= 4096}[case]
    if case == "chunk_plus_one":  # two units, in two different waves
        assert int(tab["k"][i]) == 2 and W > 1
    if case == "one_block_behind_16":
        assert tab["blocks"][int(tab["cpre"][i]) - W] == 16
    blob = walk.blob.copy()
    blob[a: a + n] = 0
    blob_t = to_cuda(blob)
    prefix = walk.prefix
    full = len(walk.appended()[0])  # (the lengths are the same: every variant ends here)
    # under the rule the call fails; the tail does not move, nothing below it changes
    dev = A.Dev(prefix, full - len(prefix))
    rc, nt, _mo, msg = A.append(ctx, dev, blob_t, walk.offs, lens, walk.hashes, flags=S.APPEND_STREAM_RULE)
    assert rc == S.SRD_ERR_ARG and NULL_ONLY in msg, (rc, msg)
    assert nt == dev.tail == len(prefix)
    got = dev.host()
    assert got[: len(prefix)].tobytes() == prefix
    assert bool((got[pad64(full):] == FILL).all())
    del got, dev
    # without the flag the same batch is the oracle's store
    want, want_mo = A.oracle_append(prefix, walk.hashes, pays)
    assert len(want) == full
    append_equals_oracle(ctx, prefix, blob_t, walk.offs, lens, walk.hashes, 0, want, want_mo)
    # with the rule and one byte that is not 0, the payload's last: accepted
    blob[a + n - 1] = 1
    pays[i] = bytes(n - 1) + b"\x01"
    want, want_mo = A.oracle_append(prefix, walk.hashes, pays)
    append_equals_oracle(ctx, prefix, to_cuda(blob), walk.offs, lens, walk.hashes, S.APPEND_STREAM_RULE, want, want_mo)


def test_zero_payload_fails_the_compaction(ctx, W):
    """test_walk_compact's session with a 3-block payload of zeros: written without the rule, refused by
    compact(), which leaves the session as it was (test_null_only_payload_fails_the_session_call's checks)."""
    _r0, over, _gone, live = U.compaction_plan(W)
    lens = [n for _, n in live]
    j = U.zero_placement(U.unit_table(lens), W, lens, "three_blocks", among=range(len(over), len(live)))
    z = live[j][0]  # a round-0 key that is live
    r = Rounds(W, zero=z)
    newer = dict(zip((i for i, _ in r.over), r.p1))
    live_pays = [newer.get(i, r.p0[i]) for i, _ in r.live]
    assert live_pays[j] == bytes(r.r0[z]) and [len(p) for p in live_pays] == r.live_lens
    assert_placed(r.tab, W, r.live_lens, j, live_pays)
    f = r.store()
    assert [(k, e - a) for a, e, _, k in K.entry_iterator(f, len(f))] == [(r.hashes[i], n) for i, n in r.live]
    # the session: the oracle's store up to the zero payload opened, the rest of round 0 -- the zero payload
    # first -- appended from a device blob with flags 0, then round 1 through the session
    head = r.store(upto=z)
    st = K.open_store(ctx, head, room=len(f) - len(head) + 4096)
    st.batch_write_device_with_key_hashes(r.hashes[z:], to_cuda(r.blob), r.offs[z:], r.r0[z:])
    st.batch_write_with_key_hashes([r.hashes[i] for i, _ in r.over], r.p1)
    assert st.batch_delete_key_hashes([r.hashes[i] for i in r.gone]) == len(f)
    assert st.bytes() == f
    state = (st.buf.data_ptr(), st.tail, st.index.table.data_ptr(), K.source_state(st))
    with pytest.raises(S.SrdError, match=NULL_ONLY):
        st.compact()
    assert (st.buf.data_ptr(), st.tail, st.index.table.data_ptr(), K.source_state(st)) == state
    assert st.len() == len(r.live) and st.bytes() == f
    assert st.batch_read_hashed_keys([r.hashes[z], r.hashes[r.live[0][0]]]) == [bytes(r.r0[z]), live_pays[0]]
