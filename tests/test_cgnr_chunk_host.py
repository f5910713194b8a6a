"""CGNR's chunk mode (lsq_set_cg_chunks; cg_layout and cg_chunk_geometry in lsqr_cg.inc) on the host: the
layout rule restated, and the inputs of tests/test_gpu_cgnr_chunk.py under the rounding-boundary
condition of tests/test_cgnr_host.py.

With 20 to 64 epochs a tile of whole time columns, even one row with its ±2 halo rows, exceeds 64 KB of
LDS.  Chunk mode cuts the tiles along dim 2 as well: a tile is ty rows × 64 dim-1 positions × one chunk
of ≤ tc owned nodes with a halo of h nodes on either side, a node column of the image having the odd
stride tcpad ≥ tc + 2h.  Two caps: (h + (ty + 2h)·(64 + 2h)·tcpad + h)·8 ≤ 64 KB and ty·tc ≤ 64 items.
  1. (ty*, tc*) minimises the staged-to-owned ratio (ty + 2h)(tc + 2h) / (ty·tc); ties go to more items,
     then to the longer chunk.  h = 2: (5, 9), ahead of (9, 5) by the last tie-break only.
  2. nch = ceil(S2 / tc*) chunks of near-equal length: chunk k owns [k·S2/nch, (k + 1)·S2/nch), and
     tc = ceil(S2 / nch).
  3. ty = the most rows ≤ S0 that both caps admit at that tc."""
from fractions import Fraction

import numpy as np
import pytest

import conftest  # noqa: F401
import cgnr_host as H

CG_TX, CG_MAXI, CG_MAXT, CG_NCW, LDS_BYTES, H_DZ = 64, 16, 16, 16, 64 * 1024, 2
# (shape, epochs) of the GPU cases: formation / operator / iterates, the masked ones, the dense oracle's
CHUNK_SWEEP = [((7, 70), nt) for nt in (20, 23, 28, 41, 64)] + [((5, 200), nt) for nt in (20, 28, 41)]
CHUNK_MASKED = [((5, 200), 28), ((7, 70), 41)]
CHUNK_DENSE, CHUNK_DENSE_NT = (9, 11), (20, 28, 64)


def _pad(tc, h):
    return (tc + 2 * h) | 1


def _lds(ty, tc, h):
    """doubles of a tile's image with its front and back pads"""
    return h + (ty + 2 * h) * (CG_TX + 2 * h) * _pad(tc, h) + h


def _fits(ty, tc, h):
    return ty * tc <= 4 * CG_MAXI and _lds(ty, tc, h) * 8 <= LDS_BYTES


def best_pair(S2, h=H_DZ):
    """step 1: (ty*, tc*)"""
    cands = [(ty, tc) for ty in range(1, 4 * CG_MAXI + 1) for tc in range(1, min(S2, 4 * CG_MAXI // ty) + 1)
             if _fits(ty, tc, h)]
    return min(cands, key=lambda c: (Fraction((c[0] + 2 * h) * (c[1] + 2 * h), c[0] * c[1]), -c[0] * c[1], -c[1]))


def chunk_rule(S0, S2, h=H_DZ):
    """(ty, tc, chunks, tcpad) of a grid of S0 rows and S2 nodes along dim 2 in chunk mode"""
    by, bc = best_pair(S2, h)
    nch = -(-S2 // bc)
    tc = -(-S2 // nch)
    ty = min(by, S0)
    while ty < S0 and _fits(ty + 1, tc, h):
        ty += 1
    return ty, tc, nch, _pad(tc, h)


def chunk_ranges(S2, nch):
    return [(k * S2 // nch, (k + 1) * S2 // nch) for k in range(nch)]


def mode_rule(S0, S2, chunks, h=H_DZ):
    """cg_layout's mode of such a grid: 'column', 'tile', 'chunk' (with the flag), or the refusal ('lds',
    'nodes')"""
    if S2 > 4 * CG_MAXI:
        return 'nodes'
    tpad = S2 | 1
    if S2 <= CG_MAXT and (CG_TX + 2 * h) * tpad <= CG_NCW * 64:
        return 'column'
    ty = max(1, min(S0, 48 // S2, 4 * CG_MAXI // S2))
    if (h + (ty + 2 * h) * (CG_TX + 2 * h) * tpad + h) * 8 <= LDS_BYTES:
        return 'tile'
    return 'chunk' if chunks else 'lds'


def halo_ratio(S0, S2, h=H_DZ):
    """staged-to-owned ratio of the rule's tiles away from the grid's faces"""
    ty, tc, nch, _ = chunk_rule(S0, S2, h)
    staged = sum((ty + 2 * h) * (b - a + 2 * h) * (CG_TX + 2 * h) for a, b in chunk_ranges(S2, nch))
    return staged / (ty * S2 * CG_TX)


def test_the_derived_figures():
    """(5, 9): 9·68·13 = 7 956 doubles and 2.76; (4, 11): 8 160 doubles and 2.90; tile mode at 16 epochs 2.63"""
    assert best_pair(64) == best_pair(20) == (5, 9)
    assert 9 * 68 * 13 == 7956 and _lds(5, 9, 2) == 7960 and _fits(5, 9, 2) and not _fits(6, 9, 2)
    assert 8 * 68 * 15 == 8160 and _fits(4, 11, 2)
    ratio = lambda ty, tc: (ty + 4) * (tc + 4) * 68 / (ty * tc * 64)
    assert round(ratio(5, 9), 2) == 2.76 and round(ratio(4, 11), 2) == 2.90 and ratio(9, 5) == ratio(5, 9)
    assert round((3 + 4) * 68 * 17 / (3 * 16 * 64), 2) == 2.63
    # the rule's ratio with S0 rows to spare
    assert [round(halo_ratio(1000, nt), 2) for nt in (20, 28, 64)] == [2.83, 2.78, 2.87]
    assert [chunk_rule(1000, nt) for nt in (20, 28, 64)] == [(6, 7, 3, 11), (6, 7, 4, 11), (5, 8, 8, 13)]


@pytest.mark.parametrize('S2', range(20, 65))
def test_layout_rule_20_to_64_epochs(S2):
    # (a grid of one row still fits tile mode up to 23 epochs, 5·68·23 doubles, and stays there)
    assert (mode_rule(1, S2, False), mode_rule(1, S2, True)) == (('tile', 'tile') if S2 <= 23 else ('lds', 'chunk'))
    for S0 in (2, 5, 7, 9, 1000):
        assert mode_rule(S0, S2, True) == 'chunk' and mode_rule(S0, S2, False) == 'lds'
        ty, tc, nch, tcpad = chunk_rule(S0, S2)
        assert 1 <= ty <= S0 and tcpad & 1 and tcpad >= tc + 2 * H_DZ
        assert _lds(ty, tc, H_DZ) * 8 <= LDS_BYTES and ty * tc <= 4 * CG_MAXI       # the two caps
        assert S0 == ty or not _fits(ty + 1, tc, H_DZ)
        assert nch == -(-S2 // 9)
        r = chunk_ranges(S2, nch)
        assert r[0][0] == 0 and r[-1][1] == S2 and all(a[1] == b[0] for a, b in zip(r, r[1:]))   # no gap, no overlap
        lens = [b - a for a, b in r]
        assert max(lens) == tc and max(lens) - min(lens) <= 1 and min(lens) >= 1


def test_up_to_19_epochs_are_not_chunked():
    for chunks in (False, True):
        assert [mode_rule(9, nt, chunks) for nt in (2, 13, 15, 16, 17, 19)] == \
            ['column', 'column', 'column', 'tile', 'tile', 'tile']
        assert mode_rule(9, 65, chunks) == 'nodes'
    assert mode_rule(9, 1, True, h=2) == 'column' and mode_rule(9, 20, True) == 'chunk'


def _name(shape, nt, tag=''):
    return f'tile-{shape[0]}x{shape[1]}-{nt}' + (f'-{tag}' if tag else '')


CASES = [_name(s, nt) for s, nt in CHUNK_SWEEP] + [_name(CHUNK_DENSE, nt) for nt in CHUNK_DENSE_NT] + \
    [_name(s, nt, 'mask') for s, nt in CHUNK_MASKED]


@pytest.mark.parametrize('name', CASES)
def test_no_factor_entry_near_a_rounding_boundary(name):
    """test_cgnr_host.py's condition on the inputs of the chunk-mode GPU cases (node blocks of 16 + 4 up
    to 4 × 16 columns): the pivots hold and no factor entry lies within 1e-11 of a bf16 rounding boundary."""
    h, A, b, blocks = H.host_case(name)
    nt = int(name.split('-')[2])
    assert sorted({C.shape[1] for C in blocks}) == sorted({16, nt % 16} - {0})
    ent = H.factor_entries(H.block_factors(A, blocks, round=False))     # also asserts the pivots
    assert ent.size == sum(C.shape[0] * C.shape[1] * (C.shape[1] + 1) // 2 for C in blocks)
    assert H.at_risk_entries(ent) == 0
    assert H.at_risk_entries(ent, eps=1e-3) > 0 or ent.size < 1000     # the count does count
    assert np.isfinite(b).all()
