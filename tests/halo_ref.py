"""NumPy restatement of the halo exchange's buffers (include/cbf_amd.h: cbf_halo_pack / _unpack and
their _nbr forms), for tests/test_gpu_halo_abi.py: the extent-key sets, the two send layouts, the
host-side "collective" that turns every rank's send buffer into one rank's receive buffer, and what
an unpack must find there.  Offsets of the neighbour layout come from ShardedLattice.nbr_splits."""
import numpy as np

from cbf_amd.shard import ShardedLattice

EXT_SLOTS, SLOT_WORDS, EXT_VALS = 64, 16, 6   # csrc/lattice_ego.hpp kExtSlots, kExtSlotWords, kExtVals
EXT_IS_MIN = np.array([True, False, False, True, True, False])
IDENTITY = np.where(EXT_IS_MIN, np.inf, -np.inf)   # the record of a set nothing was accumulated into
REC = 8                                            # doubles per record in a buffer (EXT_VALS used)


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


def dkey(v):
    """The order-preserving uint64 key of a double (csrc/cbf_device.hpp dkey)."""
    u = bits(v)
    return np.where(u >> np.uint64(63), ~u, u | np.uint64(1 << 63))


def key_sets(vals, pad):
    """The key words of nsub sets from vals (nsub, EXT_SLOTS, EXT_VALS); the unused words of every
    slot hold `pad`."""
    k = np.full(vals.shape[:2] + (SLOT_WORDS,), pad, dtype=np.uint64)
    k[:, :, :EXT_VALS] = dkey(vals)
    return k.reshape(-1)


def records(vals):
    """The nsub records (nsub, EXT_VALS) a pack reduces the sets to: min or max per field."""
    return np.where(EXT_IS_MIN, vals.min(axis=1), vals.max(axis=1))


def nbr_offsets(ws, rank, rows_elems, nsub):
    """Offsets (doubles) of the ws chunks of rank's neighbour-layout buffer, and its size."""
    return np.concatenate([[0], np.cumsum(ShardedLattice.nbr_splits(ws, rank, rows_elems, nsub))]).astype(np.int64)


def nbr_elems(W, halo, nsub, ws, rank):
    """cbf_halo_nbr_elems' formula."""
    return ws * REC * nsub + (2 * halo * W if rank > 0 else 0) + (2 * halo * W if rank + 1 < ws else 0)


def send_gathered(own, W, halo, recs, fill):
    """[first halo rows | last halo rows | nsub records]; record fields past EXT_VALS hold fill."""
    rs = halo * W
    r8 = np.full((recs.shape[0], REC), fill)
    r8[:, :EXT_VALS] = recs
    return np.concatenate([own[:rs].reshape(-1), own[own.shape[0] - rs:].reshape(-1), r8.reshape(-1)])


def send_nbr(own, W, halo, recs, ws, rank, fill):
    """Chunk q (to rank q) = [nsub records | first halo rows if q = rank - 1, last if q = rank + 1]."""
    rs, nsub = halo * W, recs.shape[0]
    off = nbr_offsets(ws, rank, 2 * rs, nsub)
    send = np.full(off[-1], fill)
    for q in range(ws):
        send[off[q]:off[q] + REC * nsub].reshape(nsub, REC)[:, :EXT_VALS] = recs
        if abs(q - rank) == 1:
            rows = own[:rs] if q < rank else own[own.shape[0] - rs:]
            send[off[q] + REC * nsub:off[q + 1]] = rows.reshape(-1)
    return send


def gather(sends, stride, fill):
    """The all-gather: slab q of the receive buffer (every rank's is the same) is rank q's send."""
    recv = np.full(stride * len(sends), fill)
    for q, s in enumerate(sends):
        recv[q * stride:q * stride + s.size] = s
    return recv


def all_to_all(sends, W, halo, nsub, rank):
    """The all-to-all: chunk q of rank's receive buffer is chunk `rank` of rank q's send."""
    ws = len(sends)
    mine = nbr_offsets(ws, rank, 2 * halo * W, nsub)
    recv = np.empty(mine[-1])
    for q, s in enumerate(sends):
        theirs = nbr_offsets(ws, q, 2 * halo * W, nsub)
        recv[mine[q]:mine[q + 1]] = s[theirs[rank]:theirs[rank + 1]]
    return recv


def window_after_unpack(wpos, owns, W, rank, rows_lo, rows_hi, hi_row_offset):
    """wpos (agents, 2) with rank - 1's last rows_lo rows at its start and rank + 1's first rows_hi
    rows from row hi_row_offset; nothing else changes."""
    out = wpos.copy()
    if rows_lo:
        out[:rows_lo * W] = owns[rank - 1][owns[rank - 1].shape[0] - rows_lo * W:]
    if rows_hi:
        out[hi_row_offset * W:(hi_row_offset + rows_hi) * W] = owns[rank + 1][:rows_hi * W]
    return out
