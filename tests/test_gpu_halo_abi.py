"""The halo exchange's four pack / unpack entry points through the public C ABI (include/cbf_amd.h:
cbf_halo_pack, cbf_halo_unpack and their _nbr forms), on tiny seeded buffers.  The collective is a
host-side copy (tests/halo_ref.py); every expectation is NumPy's restatement of the layout and
shard.guard_ok, never the library's, and everything is compared bit for bit."""
import itertools

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")
if not torch.cuda.is_available():
    pytest.skip("needs a ROCm GPU", allow_module_level=True)

from cbf_amd._lib import check, lib, ptr, stream_handle  # noqa: E402
from cbf_amd.shard import RADIUS_GUARD_EPS, guard_ok  # noqa: E402

from . import halo_ref as hr  # noqa: E402

DEV = torch.device("cuda")
RADIUS = 0.2
FILL = -7.25                              # what a buffer holds where nothing may be written
PAD = np.uint64(0x5A5A5A5A5A5A5A5A)       # the unused words of a key slot

# (W, halo, owned rows): n_own == 2 halo W, so the first and last slabs touch; rows well above that;
# 280 double2 per slab, more than one 256-thread block
GEOMS = [(5, 2, 4), (5, 2, 7), (70, 4, 9)]
# 5: more than the 4 waves of block 0, so its loop over sub-steps turns; 64: the most
NSUBS = [1, 5, 64]
# (world_size, rank): both ends and the middle; at 65 the record fan-out over destinations turns
NBR_RANKS = [(1, 0), (2, 0), (2, 1), (3, 0), (3, 1), (3, 2), (65, 0), (65, 32), (65, 64)]


def dev(a):
    return torch.as_tensor(np.ascontiguousarray(a).view(np.int64) if a.dtype == np.uint64 else a, device=DEV)


def host(t, dtype=np.float64):
    return t.cpu().numpy().view(dtype)


def same(a, b):
    return np.array_equal(hr.bits(a), hr.bits(b))


def seeded(seed, W, rows, nsub):
    """Owned positions (rows W, 2) and key values (nsub, slots, 6) of both signs, one distinct value
    per slot."""
    rng = np.random.default_rng(seed)
    return rng.normal(size=(rows * W, 2)), rng.normal(scale=3.0, size=(nsub, hr.EXT_SLOTS, hr.EXT_VALS))


def check_keys_reset(keys, nsub):
    k = host(keys, np.uint64).reshape(nsub, hr.EXT_SLOTS, hr.SLOT_WORDS)
    assert np.array_equal(k[:, :, :hr.EXT_VALS], np.broadcast_to(hr.dkey(hr.IDENTITY), k[:, :, :hr.EXT_VALS].shape))
    assert np.all(k[:, :, hr.EXT_VALS:] == PAD)


def test_reference_layout_matches_the_abi_formula():
    """tests/halo_ref.py's neighbour offsets (ShardedLattice.nbr_splits) against cbf_halo_nbr_elems'
    formula and the library's own value of it (a host function)."""
    for (W, halo, _), nsub, (ws, rank) in itertools.product(GEOMS, NSUBS, NBR_RANKS):
        off = hr.nbr_offsets(ws, rank, 2 * halo * W, nsub)
        assert off[-1] == hr.nbr_elems(W, halo, nsub, ws, rank) == lib.cbf_halo_nbr_elems(W, halo, nsub, ws, rank)
        assert np.all(np.diff(off) >= hr.REC * nsub)
    assert lib.cbf_halo_ext_bytes(3) == 3 * hr.EXT_SLOTS * hr.SLOT_WORDS * 8


@pytest.mark.parametrize("nsub", NSUBS)
@pytest.mark.parametrize("geom", GEOMS, ids=lambda g: "W%d-halo%d-rows%d" % g)
def test_pack_gathered(geom, nsub):
    W, halo, rows = geom
    own, vals = seeded(11, W, rows, nsub)
    keys, d_own = dev(hr.key_sets(vals, PAD)), dev(own)
    n_send = 4 * halo * W + hr.REC * nsub
    for want in (hr.records(vals), np.broadcast_to(hr.IDENTITY, (nsub, hr.EXT_VALS))):  # a second pack: identity
        send = dev(np.full(n_send + 4, FILL))
        check(lib.cbf_halo_pack(W, halo, rows * W, ptr(d_own), ptr(keys), nsub, ptr(send), stream_handle()),
              "cbf_halo_pack")
        got, exp = host(send), hr.send_gathered(own, W, halo, want, FILL)
        assert same(got[:4 * halo * W], exp[:4 * halo * W])
        assert same(got[4 * halo * W:n_send].reshape(nsub, hr.REC)[:, :hr.EXT_VALS], want)
        assert same(got[n_send:], np.full(4, FILL))
        check_keys_reset(keys, nsub)


@pytest.mark.parametrize("ws,rank", NBR_RANKS)
def test_pack_neighbour(ws, rank):
    for (W, halo, rows), nsub in itertools.product(GEOMS, NSUBS):
        own, vals = seeded(13, W, rows, nsub)
        keys, d_own = dev(hr.key_sets(vals, PAD)), dev(own)
        n_send = hr.nbr_elems(W, halo, nsub, ws, rank)
        off = hr.nbr_offsets(ws, rank, 2 * halo * W, nsub)
        for want in (hr.records(vals), np.broadcast_to(hr.IDENTITY, (nsub, hr.EXT_VALS))):
            send = dev(np.full(n_send + 4, FILL))
            check(lib.cbf_halo_pack_nbr(W, halo, rows * W, ptr(d_own), ptr(keys), nsub, ws, rank, ptr(send),
                                        stream_handle()), "cbf_halo_pack_nbr")
            got, exp = host(send), hr.send_nbr(own, W, halo, want, ws, rank, FILL)
            for q in range(ws):   # every destination chunk: its records, then its rows if it gets any
                r8 = hr.REC * nsub
                assert same(got[off[q]:off[q] + r8].reshape(nsub, hr.REC)[:, :hr.EXT_VALS], want), (W, nsub, q)
                assert same(got[off[q] + r8:off[q + 1]], exp[off[q] + r8:off[q + 1]]), (W, nsub, q)
            assert same(got[n_send:], np.full(4, FILL))
            check_keys_reset(keys, nsub)


def exchange(mode, owns, recs, W, halo, rank):
    """Rank's receive buffer after every rank q packed owns[q] and recs[q] (nsub, 6) and the
    collective ran, on the device; (buffer, stride or None)."""
    ws, nsub = len(owns), recs[0].shape[0]
    if mode == "gathered":
        stride = 4 * halo * W + hr.REC * nsub + 2    # (a slab larger than its contents)
        sends = [hr.send_gathered(owns[q], W, halo, recs[q], FILL) for q in range(ws)]
        return dev(hr.gather(sends, stride, FILL)), stride
    sends = [hr.send_nbr(owns[q], W, halo, recs[q], ws, q, FILL) for q in range(ws)]
    return dev(hr.all_to_all(sends, W, halo, nsub, rank)), None


def unpack(mode, recv, stride, W, halo, rows_lo, rows_hi, hi_row_offset, ws, rank, nsub, wpos, flag):
    if mode == "gathered":
        check(lib.cbf_halo_unpack(W, halo, rows_lo, rows_hi, hi_row_offset, ptr(recv), stride, ws, rank, RADIUS, nsub,
                                  ptr(wpos), ptr(flag), stream_handle()), "cbf_halo_unpack")
    else:
        check(lib.cbf_halo_unpack_nbr(W, halo, rows_lo, rows_hi, hi_row_offset, ptr(recv), ws, rank, RADIUS, nsub,
                                      ptr(wpos), ptr(flag), stream_handle()), "cbf_halo_unpack_nbr")


CLEAR = np.array([0.0, 0.0, -5.0, 5.0, 0.0, 0.0])   # a record whose owner's agents all sit at y = 0


def clear_records(ws, nsub):
    """recs[q] (nsub, 6) such that every rank's guard holds by a wide margin: rank q's agents at
    y = 10 q."""
    return [np.tile(CLEAR + 10.0 * q, (nsub, 1)) for q in range(ws)]


# (world_size, rank, rows_lo, rows_hi) at halo 2: full, partial and, at the edge ranks, none
ROW_CASES = [(1, 0, 0, 0), (3, 0, 0, 2), (3, 0, 0, 1), (3, 1, 2, 2), (3, 1, 1, 1), (3, 1, 2, 1), (3, 2, 2, 0),
             (3, 2, 1, 0)]


@pytest.mark.parametrize("mode", ["gathered", "neighbour"])
@pytest.mark.parametrize("W,halo", [(5, 2), (70, 4)])
def test_unpack_rows(mode, W, halo):
    """The ghost rows land where rows_lo, rows_hi and hi_row_offset say, nothing else is written,
    and a guard that holds leaves the flag as it was (0 and 1)."""
    own_rows, nsub = 2 * halo + 1, 2
    for (ws, rank, lo, hi), preset in itertools.product(ROW_CASES, (0, 1)):
        lo, hi = lo * halo // 2, hi * halo // 2
        owns = [seeded(17 + q, W, own_rows, 1)[0] for q in range(ws)]
        recv, stride = exchange(mode, owns, clear_records(ws, nsub), W, halo, rank)
        hi_off = lo + own_rows + 1     # (one row more than a window needs: the offset is the caller's)
        wpos0 = np.full(((hi_off + hi + 1) * W, 2), FILL)
        wpos, flag = dev(wpos0), dev(np.array([preset], dtype=np.int32))
        unpack(mode, recv, stride, W, halo, lo, hi, hi_off, ws, rank, nsub, wpos, flag)
        assert same(host(wpos).reshape(-1, 2), hr.window_after_unpack(wpos0, owns, W, rank, lo, hi, hi_off)), \
            (ws, rank, lo, hi)
        assert int(flag.cpu()[0]) == preset, (ws, rank, lo, hi)


def guard_margin():
    return RADIUS * (1.0 + RADIUS_GUARD_EPS[0]) + RADIUS_GUARD_EPS[1]


# the record field that bounds rank 2 of 5 from (rank q, field): the adjacent ranks' rows outside the
# candidate band (fields 2 / 3) and the far ranks' owned rows (fields 5 / 4)
GUARD_FIELDS = [(1, 2), (0, 5), (3, 3), (4, 4)]


@pytest.mark.parametrize("mode", ["gathered", "neighbour"])
def test_unpack_guard(mode):
    """The guard of rank 2 of 5, whose agents sit at y = 0.  Every field of another rank's record
    that the rule does not read is 0 too (reading it instead would flag a breach); the one it reads
    is far away, except in one sub-step of 5, where it is one ulp farther than the guard margin
    (holds) or one ulp nearer (breach)."""
    W, halo, ws, rank, nsub, bad_sub = 5, 2, 5, 2, 5, 3
    owns = [seeded(23 + q, W, 2 * halo, 1)[0] for q in range(ws)]
    rm = guard_margin()
    base = [np.zeros((nsub, hr.EXT_VALS)) for _ in range(ws)]
    for q, f in GUARD_FIELDS:
        base[q][:, f] = -5.0 if q < rank else 5.0
    for (q, f), (gap, holds), preset in itertools.product(
            GUARD_FIELDS, ((np.nextafter(rm, np.inf), True), (np.nextafter(rm, -np.inf), False)), (0, 1)):
        recs = [r.copy() for r in base]
        recs[q][bad_sub, f] = -gap if q < rank else gap
        by_sub = [guard_ok(np.stack([recs[p][s] for p in range(ws)]), rank, RADIUS) for s in range(nsub)]
        assert by_sub == [True] * bad_sub + [holds] + [True] * (nsub - bad_sub - 1)   # the cases straddle the margin
        recv, stride = exchange(mode, owns, recs, W, halo, rank)
        wpos, flag = dev(np.zeros((3 * halo * W, 2))), dev(np.array([preset], dtype=np.int32))
        unpack(mode, recv, stride, W, halo, halo, halo, 2 * halo, ws, rank, nsub, wpos, flag)
        assert int(flag.cpu()[0]) == (preset | (0 if holds else 1)), (q, f, holds, preset)


@pytest.mark.parametrize("mode", ["gathered", "neighbour"])
def test_unpack_guard_identity_own_record(mode):
    """A rank that recorded no computed agent (its own record is the identity) leaves the flag
    untouched, whatever the other ranks' records say."""
    W, halo, ws, rank, nsub = 5, 2, 3, 1, 2
    owns = [seeded(29 + q, W, 2 * halo, 1)[0] for q in range(ws)]
    recs = [np.zeros((nsub, hr.EXT_VALS)) for _ in range(ws)]     # everyone at y = 0: a breach ...
    assert not guard_ok(np.stack([r[0] for r in recs]), rank, RADIUS)
    recs[rank] = np.tile(hr.IDENTITY, (nsub, 1))                   # ... unless rank computed nothing
    assert guard_ok(np.stack([r[0] for r in recs]), rank, RADIUS)
    recv, stride = exchange(mode, owns, recs, W, halo, rank)
    wpos, flag = dev(np.zeros((3 * halo * W, 2))), dev(np.array([0], dtype=np.int32))
    unpack(mode, recv, stride, W, halo, halo, halo, 2 * halo, ws, rank, nsub, wpos, flag)
    assert int(flag.cpu()[0]) == 0
