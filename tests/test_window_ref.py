"""The host expectations of tests/window_ref.py (extents and brute-force halo guard, used by the
GPU tests of the windowed lattice ABI) against the host restatements the sharded driver is tested
with (cbf_amd.shard.sub_extents / guard_ok): two independent statements of the same contract."""
import numpy as np
import pytest

from cbf_amd import scenarios
from cbf_amd.shard import guard_ok, sub_extents

from . import window_ref as wr

W, H = 24, 36


@pytest.mark.parametrize("spacing,seed", [(0.145, 1), (0.09, 2), (0.3, 3)])
def test_extents_match_shard_sub_extents(spacing, seed):
    pos = scenarios.lattice(W, H, seed=seed, spacing=spacing)
    for rb, re in [(0, 12), (12, 24), (24, 36), (20, 21), (0, 36)]:
        for guard in (0, 1, 3, re - rb, re - rb + 2):
            w0, w1 = max(0, rb - 4), min(H, re + 4)
            want = sub_extents(pos[w0 * W:w1 * W], W, w0, rb, re, rb, re, min(guard, re - rb))
            got = wr.expected_extents(pos, W, rb, re, guard)
            assert np.array_equal(got[:2], want[[4, 5]]), (rb, re, guard)
            assert np.array_equal(got[2:], want[2:4]), (rb, re, guard)
            y = pos[:, 1].reshape(H, W)[rb:re]
            assert got[0] == y.min() and got[1] == y.max()
    e = wr.expected_extents(pos, W, 12, 24, 12)
    assert e[2] == -np.inf and e[3] == np.inf


@pytest.mark.parametrize("spacing,seed", [(0.145, 1), (0.09, 2), (0.3, 3), (0.21, 4)])
def test_brute_guard_matches_shard_guard_ok(spacing, seed):
    """Three stripes of 12 rows: the guard over records, over the positions themselves, and
    shard.guard_ok agree for every halo and rank (both outcomes occur over the cases)."""
    pos = scenarios.lattice(W, H, seed=seed, spacing=spacing)
    stripes = [(0, 12), (12, 24), (24, 36)]
    seen = set()
    for halo in (1, 2, 3, 4):
        e = np.stack([wr.expected_extents(pos, W, rb, re, halo - 1) for rb, re in stripes])
        recs = np.concatenate([e, e[:, :2]], axis=1)  # computed rows = owned rows
        for rank, (rb, re) in enumerate(stripes):
            want = guard_ok(recs, rank, 0.2)
            assert wr.brute_guard_records(e, rank, 0.2) == want, (halo, rank)
            assert wr.brute_guard_positions(pos, W, H, rb, re, halo - 1, 0.2) == want, (halo, rank)
            seen.add(want)
    if spacing == 0.145:
        assert seen == {True, False}  # rows 3 apart are out of range, rows 2 apart are not


def test_brute_guard_edges():
    rm = wr.guard_radius(0.2)
    assert wr.brute_guard([1.0, 2.0], [], [], 0.2)
    assert not wr.brute_guard([rm], [0.0], [], 0.2)                     # a gap of exactly rm
    assert wr.brute_guard([np.nextafter(rm, np.inf)], [0.0], [], 0.2)
    assert not wr.brute_guard([0.0], [], [rm], 0.2)
    assert wr.brute_guard([0.0], [], [np.nextafter(rm, np.inf)], 0.2)
    assert not wr.brute_guard([1.0, np.nan], [0.0], [], 0.2)
    assert not wr.brute_guard([1.0], [], [np.nan], 0.2)
    assert wr.brute_guard([1.0], [-np.inf], [np.inf], 0.2)


def test_window_sufficient_and_candidate_rows():
    assert wr.candidate_rows(48, 0, 15) == (0, 14)
    assert wr.candidate_rows(48, 9, 18) == (10, 26)
    assert wr.candidate_rows(48, 33, 15) == (34, 48)
    assert wr.candidate_rows(48, 0, 48) == (0, 48)
    Wl, Hl = 40, 48
    pos = scenarios.lattice(Wl, Hl, seed=7, spacing=0.145)
    assert wr.window_sufficient(pos, Wl, Hl, 12, 24, 9, 18, 0.2)       # owned +- 3
    assert not wr.window_sufficient(pos, Wl, Hl, 12, 24, 10, 16, 0.2)  # owned +- 2
    assert wr.window_sufficient(pos, Wl, Hl, 0, 12, 0, 15, 0.2)
    assert not wr.window_sufficient(pos, Wl, Hl, 0, 12, 0, 14, 0.2)
    dense = scenarios.lattice(Wl, Hl, seed=3, spacing=0.09)
    assert wr.window_sufficient(dense, Wl, Hl, 12, 24, 8, 20, 0.2)      # owned +- 4
    assert not wr.window_sufficient(dense, Wl, Hl, 12, 24, 9, 18, 0.2)
