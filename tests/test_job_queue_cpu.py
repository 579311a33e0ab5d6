"""The job queue's block decode and per-lane packing (csrc/rt_render.h: queue_block, queue_pack / queue_unpack), without a
GPU: the host build of the device functions' own text (native.queue_blocks_host, native.queue_pack_host).

A block is the 64 jobs of one wave-quarter of a tile for one chunk of samples.  Block ids must cover every (tile slot,
quarter, chunk) exactly once, in the order the static grid gives its workgroups -- the big chunks of every tile before
any small one -- and carry the chunk's sample range; chunk_range is restated here."""
import itertools

import numpy as np
import pytest

import _golden as G

rtr = G.rtr
blocks_host = rtr.native.queue_blocks_host
pack_host = rtr.native.queue_pack_host


def chunk_range(spp, chunks, guided, c):
    n_big, big, small = guided
    if small == 0:
        s0, s1 = c * spp // chunks, (c + 1) * spp // chunks
    elif c < n_big:
        s0, s1 = c * big, c * big + big
    else:
        s0 = n_big * big + (c - n_big) * small
        s1 = s0 + small
    s0, s1 = min(s0, spp), min(s1, spp)
    return s0, (spp if c == chunks - 1 else s1)


def guided_split(spp, chunks):
    """the split choose_chunks (csrc/rt_select.h) makes of `chunks` equal parts: (chunks, (n_big, big_spp, small_spp))"""
    n_big = max(1, chunks * 6 // 8)
    big = int((0.90 * spp + n_big - 1) / n_big)
    rem = spp - n_big * big
    small = max(1, big // 3)
    assert rem > 0
    return n_big + -(-rem // small), (n_big, big, small)


# (spp, chunks, (n_big, big_spp, small_spp)): equal parts, then guided splits, each with 1, 3 and 8 chunks
SPLITS = [(6, 1, (0, 0, 0)), (7, 3, (0, 0, 0)), (3, 3, (0, 0, 0)), (400, 8, (0, 0, 0))]
SPLITS += [(10, 1, (1, 9, 3)), (10, 3, (2, 4, 2)), (20, 3, (2, 9, 1))]
SPLITS += [(spp,) + guided_split(spp, chunks) for spp, chunks in ((400, 8), (64, 4))]


@pytest.mark.parametrize("n_tiles", [1, 5])
@pytest.mark.parametrize("spp,chunks,guided", SPLITS)
def test_block_decode(n_tiles, spp, chunks, guided):
    recs = blocks_host(n_tiles, spp, chunks, guided)
    assert len(recs) == n_tiles * chunks * 4
    keys = list(zip(recs["slot"].tolist(), recs["quarter"].tolist(), recs["chunk"].tolist()))
    assert sorted(keys) == list(itertools.product(range(n_tiles), range(4), range(chunks)))  # each exactly once
    # the four quarters of a (tile, chunk) are consecutive blocks: block b belongs to workgroup b >> 2 of the static grid
    for b in range(0, len(recs), 4):
        assert recs["quarter"][b:b + 4].tolist() == [0, 1, 2, 3]
        assert len(set(keys[b + q][::2] for q in range(4))) == 1
    n_big = guided[0] if guided[2] else chunks
    big = recs["chunk"] < n_big
    if (~big).any():
        assert np.flatnonzero(big).max() < np.flatnonzero(~big).min()  # every big-chunk block before every small one
    for r in recs:
        want = chunk_range(spp, chunks, guided, int(r["chunk"]))
        assert (int(r["s0"]), int(r["s1"])) == want == (int(r["ref_s0"]), int(r["ref_s1"]))
    # the chunks of a pixel tile its samples
    for slot in range(n_tiles):
        mine = recs[(recs["slot"] == slot) & (recs["quarter"] == 0)]
        mine = mine[np.argsort(mine["chunk"])]
        assert mine["s0"][0] == 0 and mine["s1"][-1] == spp
        assert np.array_equal(mine["s0"][1:], mine["s1"][:-1])


def test_guided_splits_are_guided():
    assert guided_split(400, 8) == (8, (6, 60, 20))  # the headline's split: six chunks of 60 samples, two of 20
    assert sorted(set(s[1] for s in SPLITS if s[2][2] > 0)) == [1, 3, 5, 8]
    assert sorted(set(s[1] for s in SPLITS if s[2][2] == 0)) == [1, 3, 8]


@pytest.mark.parametrize("i,j,s_end", list(itertools.product([0, 1, 65535], [0, 1, 65535], [0, 1, 2 ** 31 - 1])))
def test_packing_round_trips(i, j, s_end):
    (lo, hi), back = pack_host(i, j, s_end)
    assert back == (i, j, s_end)
    assert lo == (i | (j << 16)) and hi == s_end  # pixel in one half of the parked word, s_end in the other
