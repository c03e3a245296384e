"""The tile plan of the wave-specialised iteration kernel's tile queue (gnnkeras_amd/csrc/kernel_state_fused4.hpp: f4_tile_plan, the ONE
function both the launcher and every workgroup evaluate), through its C export - no GPU.  For every XCD of a launch the static blocks (the
first T1 WG-local tiles of each of its workgroups, t_begin + lb + L * blk) and the pool's chunks must cover the XCD's tile range exactly
once; only the last chunk may reach past the range's end; below the threshold the plan is the static assignment."""
import ctypes as C
import os

import numpy as np
import pytest

from gnnkeras_amd import _native as nat


@pytest.fixture(scope='module')
def lib():
    if not os.path.exists(nat.LIB_PATH):
        nat.build()
    return nat.lib()


def _consts(lib):
    q = lib.gnn_debug_f4_tile_queue_const
    return dict(CH=q(0, 0), AHEAD={sp: q(1, sp) for sp in (16, 32, 64)}, MIN_SHARE=q(2, 0), MAX_CHUNKS=q(3, 0), TAB=q(4, 0))


def _plans(lib, ntiles, nblk, ahead, out=None):
    """The plans of all 8 XCDs of one launch: [8, 7] = t_begin, t_end, workgroups, T1, pool_begin, pool_end, n_chunks."""
    out = np.empty((8, 7), dtype=np.int32) if out is None else out
    lib.gnn_debug_f4_tile_plan(ntiles, nblk, ahead, out.ctypes.data_as(C.POINTER(C.c_int32)))
    return out


def _check_identities(c, P, ntiles, nblk, ahead):
    """P [..., 8, 7] plans, ntiles / nblk [..., 1]: the identities that make the cover exact (see _check_one_by_one for the count itself)."""
    CH = c['CH']
    t_begin, t_end, blk, T1, pool_begin, pool_end, n_chunks = (P[..., i] for i in range(7))
    x = np.arange(8)
    tpx = (ntiles + 7) // 8
    assert (t_begin == np.minimum(ntiles, x * tpx)).all() and (t_end == np.minimum(ntiles, (x + 1) * tpx)).all()     # the XCD's range stays what it was
    assert (blk == nblk // 8).all() and (T1 >= 0).all()
    queued = n_chunks > 0
    assert (queued.all(axis=-1) | ~queued.any(axis=-1)).all()              # one decision per launch: host and every workgroup agree
    n = t_end - t_begin
    s = ~queued                                                              # static: every workgroup walks t_first + L * blk to the end of the range
    assert (pool_begin[s] == t_end[s]).all() and (pool_end[s] == t_end[s]).all() and (T1[s] == -(-n[s] // blk[s])).all()
    q = queued                                                               # queue: lb + L * blk, lb < blk, L < T1, is every number below T1 * blk once
    assert (T1[q] >= ahead).all() and (n[q] >= c['MIN_SHARE'] * blk[q]).all()
    assert (pool_begin[q] == t_begin[q] + T1[q] * blk[q]).all() and (t_begin[q] < pool_begin[q]).all() and (pool_begin[q] < pool_end[q]).all()
    assert (pool_end[q] == t_end[q]).all()
    assert (n_chunks[q] == -(-(pool_end[q] - pool_begin[q]) // CH)).all() and (n_chunks[q] <= c['MAX_CHUNKS']).all() and c['MAX_CHUNKS'] < c['TAB'] - ahead
    over = pool_begin[q] + n_chunks[q] * CH - t_end[q]
    assert (0 <= over).all() and (over < CH).all()                           # only the last chunk reaches past t_end, by less than a chunk
    return queued.all(axis=-1)


def _check_one_by_one(c, P, ntiles):
    CH = c['CH']
    cover = np.zeros(ntiles + CH, dtype=np.int32)
    for t_begin, t_end, blk, T1, pool_begin, pool_end, n_chunks in P.tolist():
        static_end = pool_begin if n_chunks else t_end
        t = (t_begin + np.arange(blk)[:, None] + blk * np.arange(T1)[None, :]).ravel()
        np.add.at(cover, t[t < static_end], 1)
        t = (pool_begin + CH * np.arange(n_chunks)[:, None] + np.arange(CH)[None, :])
        if n_chunks: assert t[:-1].max(initial=-1) < t_end                   # chunks past the end: the last one alone, wholly or partly
        np.add.at(cover, t[t < t_end], 1)                                    # (tiles at and past t_end are pad tiles: tile_of() maps them to -1)
    assert (cover[:ntiles] == 1).all() and (cover[ntiles:] == 0).all(), ntiles


def test_every_range_is_covered_exactly_once(lib):
    """ntiles 1 .. 3 000 x 8 .. 512 workgroups in steps of 8, every XCD."""
    c = _consts(lib)
    ahead = c['AHEAD'][64]
    nt, nb = np.arange(1, 3001), np.arange(8, 513, 8)
    P = np.empty((len(nt), len(nb), 8, 7), dtype=np.int32)
    for i, ntiles in enumerate(nt.tolist()):
        for j, nblk in enumerate(nb.tolist()):
            _plans(lib, ntiles, nblk, ahead, P[i, j])
    queued = _check_identities(c, P, nt[:, None, None], nb[None, :, None], ahead)
    assert queued.any() and not queued.all()                                 # (few workgroups over many tiles: both sides of the threshold are in the sweep)
    for i, j in [(2999, 0), (2999, 1), (2998, 2), (1500, 0), (1023, 0), (129, 0), (8, 0), (0, 0), (2999, 63)]:
        _check_one_by_one(c, P[i, j], int(nt[i]))


@pytest.mark.parametrize('ntiles,nblk', [(1, 8), (7, 8), (9, 8), (130, 8), (1023, 8), (1024, 8), (1025, 16), (2999, 16), (3000, 24), (3000, 512),
                                        (12_500, 512), (12_501, 512), (6_250, 512), (2_500, 512), (62_500, 512), (250_000, 512), (250_001, 504)])
def test_tiles_counted_one_by_one(lib, ntiles, nblk):
    """... and counted tile by tile, for shapes on both sides of the threshold, the C4 (62 500) and 4 M-node (250 000) tile counts."""
    c = _consts(lib)
    for sp in (64, 32, 16):
        P = _plans(lib, ntiles, nblk, c['AHEAD'][sp])
        _check_identities(c, P, np.array([ntiles]), np.array([nblk]), c['AHEAD'][sp])
        _check_one_by_one(c, P, ntiles)


def test_threshold(lib):
    """The 200 000-node shape (24 tiles per workgroup) takes the queue at padded widths 64 and 32, C3 (12) and everything smaller do not; a
    pool too large for a workgroup's table is cut to the table's size, not dropped."""
    c = _consts(lib)
    for sp in (64, 32):
        assert (_plans(lib, 12_500, 512, c['AHEAD'][sp])[:, 6] > 0).all() and (_plans(lib, 12_501, 512, c['AHEAD'][sp])[:, 6] > 0).all()
    for ntiles in (6_250, 2_500, 512, 1):
        assert (_plans(lib, ntiles, 512, c['AHEAD'][64])[:, 6] == 0).all()
    assert _plans(lib, 62_500, 512, c['AHEAD'][64])[0, 3] == 7 * 7813 // (8 * 64)      # C4: T1 = 7/8 of the equal share
    big = _plans(lib, 2_500_000, 512, c['AHEAD'][64])
    # T1 is rounded up to whole rows of workgroups, so the pool is the largest that fits the table: within one such row of its cap
    pool = big[:, 5] - big[:, 4]
    assert (pool <= c['MAX_CHUNKS'] * c['CH']).all() and (pool > c['MAX_CHUNKS'] * c['CH'] - big[:, 2]).all()
    assert (big[:, 6] > 0).all() and (big[:, 6] <= c['MAX_CHUNKS']).all()
    _check_identities(c, big, np.array([2_500_000]), np.array([512]), c['AHEAD'][64])
