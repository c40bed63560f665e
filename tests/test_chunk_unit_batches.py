"""The batches tests/test_gpu_chunk_units.py runs, and what they must cover.

A host restatement of the chunk units of srd_gather.h / srd_units.hip -- how a
batch's hits are cut into units, which wave of stream_copy_crc_kernel's grid
walks which units, and how unit_combine_kernel splits a hit's units over its
64 lanes -- plus the seeded generators of the batches.  The tests here need
no GPU: they assert that the generated batches meet the coverage conditions
for every grid size the GPU test may meet (W = 16 waves x 64, 256 and 304
CUs), so that on the device those conditions are facts, not luck."""
import random

import numpy as np
import pytest

import srd_amd as S

CH = S.GATHER_CHUNK
TILE = 4096          # stream_copy_crc_kernel's block (srd_stream.hip)
COMBINE_LANES = 64   # unit_combine_kernel's wave (srd_units.hip)
# SCAN_WAVES_V2 (srd_kernels.hip): the waves of one stream_copy_crc_kernel block.  The grid is
# min(ceil(units / SCAN_WAVES_V2), c->scan_blocks) blocks, scan_blocks = the CU count (launch_stream,
# srd_ops.hip, for srd_payload_gather_device and plan_commit alike), so a batch of more than W = 16 x CUs units gives
# wave w the units w, w + W, w + 2 W, ...
WAVES_PER_BLOCK = 16
GRIDS = [WAVES_PER_BLOCK * cus for cus in (64, 256, 304)]

# -- part A: many chunks per hit ---------------------------------------------------------------

COMBINE_K = [63, 64, 65, 66, 128, 129, 130]
COMBINE_R = [1, 17, 4097, CH - 1, CH]
COMBINE_LENGTHS = [(k - 1) * CH + COMBINE_R[i % len(COMBINE_R)] for i, k in enumerate(COMBINE_K)]


def lane_split(k):
    """unit_combine_kernel's split of an entry's k units over the 64 lanes of its wave: lane l XORs the terms of
    the units l, l + 64, l + 128, ...  Returns the list of units per lane."""
    return [list(range(l, k, COMBINE_LANES)) for l in range(COMBINE_LANES)]


def last_lane(k):
    """The last lane that holds a unit."""
    return max(l for l, us in enumerate(lane_split(k)) if us)


def combine_flip_positions(n):
    """The byte positions test A1 flips in a hit of n bytes (more than 64 units): byte 0, the last byte, the first
    byte of unit 1 (lane 1), byte 7 of unit 63 (the last lane's first unit), byte 7 of unit 64 (lane 0's second
    round) and, for 129 units or more, byte 7 of unit 128 (lane 0's third round) -- unless that unit is shorter
    than 8 bytes: it is the hit's last unit then, and the last byte already lies in it."""
    k = (n + CH - 1) // CH
    split = lane_split(k)
    assert k > 64 and split[1][0] == 1 and split[last_lane(k)][0] == 63 and split[0][1] == 64
    pos = [0, n - 1, CH, 63 * CH + 7, 64 * CH + 7]
    if k >= 129:
        assert split[0][2] == 128
        if 128 * CH + 7 < n:
            pos.append(128 * CH + 7)
        assert any(p // CH == 128 for p in pos)
    assert len(set(pos)) == len(pos) and all(0 <= p < n for p in pos)
    return pos


def test_combine_lengths_change_the_split():
    assert [(n + CH - 1) // CH for n in COMBINE_LENGTHS] == COMBINE_K and sum(COMBINE_K) == 645
    assert set((n - 1) % CH + 1 for n in COMBINE_LENGTHS) == set(COMBINE_R)
    rounds = lambda k: sorted(set(len(us) for us in lane_split(k)))   # the lanes' unit counts
    used = lambda k: [l for l, us in enumerate(lane_split(k)) if us]
    assert rounds(63) == [0, 1] and used(63) == list(range(63)) and last_lane(63) == 62   # lane 63 empty
    assert rounds(64) == [1] and last_lane(64) == 63                        # the last k of one round
    assert rounds(65) == [1, 2] and lane_split(65)[0] == [0, 64]            # lane 0 alone has a second round
    assert all(us == [l] for l, us in enumerate(lane_split(65)) if l)
    assert rounds(66) == [1, 2] and [l for l, us in enumerate(lane_split(66)) if len(us) == 2] == [0, 1]
    assert rounds(128) == [2] and lane_split(128)[63] == [63, 127]          # the last k of two rounds
    assert rounds(129) == [2, 3] and lane_split(129)[0] == [0, 64, 128]     # lane 0 alone has a third round
    assert all(us == [l, l + 64] for l, us in enumerate(lane_split(129)) if l)
    assert rounds(130) == [2, 3] and lane_split(130)[1] == [1, 65, 129] and lane_split(130)[2] == [2, 66]
    for k in COMBINE_K:  # the lanes' shares are a partition of the units
        assert sorted(j for us in lane_split(k) for j in us) == list(range(k))
        assert all(j % COMBINE_LANES == l for l, us in enumerate(lane_split(k)) for j in us)
        assert used(k) == list(range(min(k, COMBINE_LANES)))
    # the flipped bytes of the k = 129 and the k = 65 hit: each in a unit of another lane or round (the k = 129
    # hit ends one byte into unit 128, so its last byte is the position in lane 0's third round)
    assert combine_flip_positions(COMBINE_LENGTHS[5]) == [0, 128 * CH, CH, 63 * CH + 7, 64 * CH + 7]
    assert combine_flip_positions(COMBINE_LENGTHS[2]) == [0, 64 * CH + 4096, CH, 63 * CH + 7, 64 * CH + 7]
    assert combine_flip_positions(COMBINE_LENGTHS[6]) == [0, 129 * CH + 16, CH, 63 * CH + 7, 64 * CH + 7, 128 * CH + 7]


# -- part B: more units than waves -----------------------------------------------------------------

TAIL_R = [1, 15, 16, 17, 1023, 1040, 4095, 4096]
BLOCKS, BLOCK_WEIGHTS = [1, 2, 3, 5, 16], [25, 25, 25, 15, 10]
MULTI = [CH + 1, 2 * CH + 17]   # a few hits of more than one chunk: 0.5 % each
SEED = 0xC4A9
ONLY, FIRST, MIDDLE, LAST = 0, 1, 2, 3   # a unit's role in its hit


def draw_length(rng):
    x = rng.random()
    if x < 0.01:
        return MULTI[x < 0.005]
    return (rng.choices(BLOCKS, BLOCK_WEIGHTS)[0] - 1) * TILE + rng.choice(TAIL_R)


def gen_lengths(W, factor=2.5, seed=SEED):
    """Payload lengths drawn until the batch has at least factor * W units."""
    rng = random.Random(seed)
    lens, units = [], 0
    while units < factor * W:
        lens.append(draw_length(rng))
        units += (lens[-1] + CH - 1) // CH
    return lens


def packed_offsets(lens):
    """Back to back: every source alignment occurs."""
    o = np.zeros(len(lens), np.int64)
    o[1:] = np.cumsum(np.asarray(lens, np.int64))[:-1]
    return o


def spaced_offsets(lens, seed=SEED):
    """Ranges with at least 20 spare bytes behind each (the planted checksum at end + 16), half of them
    16-aligned, the others at a residue 1..15.  Returns (offsets, the blob's length)."""
    rng = random.Random(seed ^ 0x5A)
    offs, o = [], 0
    for n in lens:
        o = ((o + 15) & ~15) + (0 if rng.random() < 0.5 else rng.randrange(1, 16))
        offs.append(o)
        o += n + 20 + rng.randrange(0, 9)
    return np.array(offs, np.int64), o


def unit_table(lens, srcs=None):
    """The units of a batch in query order, as stream_copy_crc_kernel's unit_s sees them: per unit its hit, its
    4 KiB block count, whether its source address is 16-byte aligned (srcs: byte offsets from a 16-aligned base),
    and its role in the hit."""
    lens = np.asarray(lens, np.int64)
    srcs = np.zeros(len(lens), np.int64) if srcs is None else np.asarray(srcs, np.int64)
    k = (lens + CH - 1) // CH
    cpre = np.cumsum(k) - k
    hit = np.repeat(np.arange(len(lens)), k)
    c = np.arange(int(k.sum())) - cpre[hit]
    clen = np.minimum(lens[hit] - c * CH, CH)
    role = np.where(k[hit] == 1, ONLY, np.where(c == 0, FIRST, np.where(c == k[hit] - 1, LAST, MIDDLE)))
    return {"hit": hit, "blocks": (clen + TILE - 1) // TILE, "al": (srcs[hit] + c * CH) % 16 == 0, "role": role,
            "cpre": cpre, "k": k, "n": int(k.sum())}


def wave_pairs(tab, W, what):
    """{(x[u], x[u + W])}: the ordered pairs a wave meets on its walk from one unit to the next."""
    x = tab[what]
    return set(zip(x[:-W].tolist(), x[W:].tolist())) if tab["n"] > W else set()


def check_coverage(tab, W, alignments=True):
    """The conditions under which a batch exercises the streaming kernel's unit-to-unit state."""
    assert tab["n"] >= 2.5 * W, (tab["n"], W)
    assert wave_pairs(tab, W, "blocks") == {(a, b) for a in BLOCKS for b in BLOCKS}
    if alignments:
        assert wave_pairs(tab, W, "al") == {(a, b) for a in (False, True) for b in (False, True)}
    roles = wave_pairs(tab, W, "role")
    assert (LAST, ONLY) in roles and (ONLY, LAST) in roles


# -- part C: an all-zero payload that is not its wave's first unit ------------------------------------

ZERO_CASES = ["three_blocks", "chunk_plus_one", "one_block_behind_16"]


def placement_ok(tab, W, lens, i, case):
    """Every unit u of hit i has u >= W, and the wave's previous unit u - W belongs to another payload and has
    2 or more blocks (16 for the one-block case: directly behind a 16-block unit)."""
    n = lens[i]
    want = {"three_blocks": 2 * TILE < n <= 3 * TILE, "chunk_plus_one": n == CH + 1,
            "one_block_behind_16": n <= TILE}[case]
    us = range(int(tab["cpre"][i]), int(tab["cpre"][i] + tab["k"][i]))
    need = 16 if case == "one_block_behind_16" else 2
    return want and all(u >= W and tab["blocks"][u - W] >= need and tab["hit"][u - W] != i for u in us)


def zero_placement(tab, W, lens, case, among=None):
    """The first hit (of `among`) that meets placement_ok."""
    for i in (range(len(lens)) if among is None else among):
        if placement_ok(tab, W, lens, i, case):
            return i
    raise AssertionError("no hit of the batch fits the %s placement at W = %d" % (case, W))


# -- the compaction's batch (B3): two oracle rounds, then the live entries newest first ------------------

def compaction_plan(W, seed=SEED):
    """Round 0 writes every length of gen_lengths(W, 2.8); round 1 overwrites 7 % of the keys with fresh lengths
    and deletes 3 %.  Returns (round-0 lengths, [(key index, new length)], deleted key indices, the live entries
    newest first -- the compaction's hits -- as [(key index, length)])."""
    lens = gen_lengths(W, 2.8, seed)
    rng = random.Random(seed ^ 0xC3)
    picked = rng.sample(range(len(lens)), len(lens) // 10)
    n_over = len(picked) * 7 // 10
    over = [(i, draw_length(rng)) for i in picked[:n_over]]
    gone = picked[n_over:]
    dead = set(picked)
    live = [(i, n) for i, n in reversed(over)] + [(i, lens[i]) for i in reversed(range(len(lens))) if i not in dead]
    return lens, over, gone, live


@pytest.mark.parametrize("W", GRIDS)
def test_generated_batches_cover_the_walk(W):
    lens = gen_lengths(W)
    assert gen_lengths(W) == lens  # seeded
    packed = unit_table(lens, packed_offsets(lens))   # B2 and C: the append's blob
    check_coverage(packed, W)
    check_coverage(unit_table(lens, spaced_offsets(lens)[0]), W)   # B1: the gather's ranges
    assert set(lens) >= set(MULTI)
    for case in ZERO_CASES:
        i = zero_placement(packed, W, lens, case)
        assert placement_ok(packed, W, lens, i, case)
    # B3: the compaction's hits are the live entries, newest first; their sources are 64-aligned
    r0, over, gone, live = compaction_plan(W)
    assert len(over) > 3 and len(gone) > 3 and len(live) == len(r0) - len(gone)
    ctab = unit_table([n for _, n in live])
    check_coverage(ctab, W, alignments=False)
    j = zero_placement(ctab, W, [n for _, n in live], "three_blocks", among=range(len(over), len(live)))
    assert live[j][0] not in {i for i, _ in over}  # a round-0 entry that is still live


def test_unit_table_restates_the_header():
    """unit_table against the definitions it restates, on a batch small enough to spell out."""
    lens = [1, CH, CH + 1, 2 * CH + 17, 4097]
    t = unit_table(lens, [0, 16, 5, 32, 7])
    assert t["hit"].tolist() == [0, 1, 2, 2, 3, 3, 3, 4] and t["n"] == 8
    assert t["blocks"].tolist() == [1, 16, 16, 1, 16, 16, 1, 2]
    assert t["al"].tolist() == [True, True, False, False, True, True, True, False]
    assert t["role"].tolist() == [ONLY, ONLY, FIRST, LAST, FIRST, MIDDLE, LAST, ONLY]
    assert wave_pairs(t, 3, "blocks") == {(1, 1), (16, 16), (16, 2)}
    assert wave_pairs(t, 3, "role") == {(ONLY, LAST), (ONLY, FIRST), (FIRST, MIDDLE), (LAST, LAST), (FIRST, ONLY)}
