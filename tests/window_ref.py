"""Host-side expectations for the windowed lattice calls of the C ABI (include/cbf_amd.h:
cbf_lattice_step / _advance / _advance_hocbf with a halo window, their `extents`, cbf_halo_guard),
from positions alone (NumPy): nothing here calls the library.  Used by
tests/test_gpu_lattice_window_abi.py; checked against cbf_amd.shard's host restatements in
tests/test_window_ref.py."""
import numpy as np


def guard_radius(radius):
    """The guard's margin on the cull radius (cbf_amd.h: farther than `radius` in y, with the
    rounding slack of cbf_amd/shard.py RADIUS_GUARD_EPS)."""
    return radius * (1.0 + 1e-9) + 1e-12


def candidate_rows(H, w0, wrows):
    """Rows [lo, hi) of a window [w0, w0 + wrows) whose agents are cull candidates: all but the
    first and the last window row, unless that row is a lattice edge."""
    return (w0 + 1 if w0 > 0 else 0), (w0 + wrows - 1 if w0 + wrows < H else H)


def window_sufficient(pos, W, H, rb, re, w0, wrows, radius):
    """True iff every agent outside the window's candidate rows is farther than the guard radius,
    in y, below (rows under the candidates) or above (rows over them) every owned agent: the
    windowed step then equals the whole-lattice step on the owned rows."""
    y = np.asarray(pos)[:, 1].reshape(H, W)
    lo, hi = candidate_rows(H, w0, wrows)
    own = y[rb:re]
    rm = guard_radius(radius)
    below_ok = lo == 0 or own.min() - y[:lo].max() > rm
    above_ok = hi == H or y[hi:].min() - own.max() > rm
    return bool(below_ok and above_ok)


def expected_extents(new_pos, W, rb, re, guard):
    """`extents` of a step that owns rows [rb, re), from the whole lattice's new positions:
    {min y, max y over the owned rows, max y over owned rows < re - guard, min y over owned rows
    >= rb + guard} (-inf / +inf where no row qualifies)."""
    y = np.asarray(new_pos)[:, 1].reshape(-1, W)
    own = y[rb:re]
    low = y[rb:max(rb, re - guard)]
    high = y[min(re, rb + guard):re]
    return np.array([own.min(), own.max(), low.max() if low.size else -np.inf,
                     high.min() if high.size else np.inf], dtype=np.float64)


def brute_guard(own_y, below_y, above_y, radius):
    """The halo guard by definition: True (clear) iff every y of below_y lies more than the guard
    radius under every owned y and every y of above_y more than it over every owned y.  Every pair
    is compared; a NaN on either side makes its comparisons false, i.e. a breach."""
    rm = guard_radius(radius)
    own = np.asarray(own_y, dtype=np.float64).reshape(-1, 1)
    below = np.asarray(below_y, dtype=np.float64).reshape(1, -1)
    above = np.asarray(above_y, dtype=np.float64).reshape(1, -1)
    with np.errstate(invalid="ignore"):
        return bool(np.all(own - below > rm) and np.all(above - own > rm))


def brute_guard_records(recs, rank, radius):
    """brute_guard over the y-sets that extents records stand for: rank's owned agents span
    {e0, e1}; of rank - 1 only the rows outside the halo (topped by its e2) and of rank + 1 only
    those bottomed by its e3 lie outside rank's candidate rows; every other rank's agents all do
    (spanned by its {e0, e1}).  recs: (world_size, >= 4)."""
    recs = np.asarray(recs, dtype=np.float64)
    below, above = [], []
    for q in range(recs.shape[0]):
        if q < rank:
            below += [recs[q, 2]] if q == rank - 1 else [recs[q, 0], recs[q, 1]]
        elif q > rank:
            above += [recs[q, 3]] if q == rank + 1 else [recs[q, 0], recs[q, 1]]
    return brute_guard(recs[rank, :2], below, above, radius)


def brute_guard_positions(new_pos, W, H, rb, re, keep, radius):
    """brute_guard of the stripe [rb, re) over actual positions: its owned y against the y of every
    agent outside rows [rb - keep, re + keep) (keep = halo - 1: the neighbours' rows inside this
    stripe's candidate band)."""
    y = np.asarray(new_pos)[:, 1].reshape(H, W)
    return brute_guard(y[rb:re], y[:max(0, rb - keep)], y[min(H, re + keep):], radius)
