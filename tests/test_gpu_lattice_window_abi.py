"""Windowed lattice advances through the public C ABI (include/cbf_amd.h): a stripe of owned rows
[row_begin, row_end) advanced from a halo window [win_row0, win_row0 + win_rows), its `extents`
(the per-wave records behind the workspace, the queue blocks' records, k_extents_finalize) and
cbf_halo_guard -- the documented way to shard a lattice without cbf_amd/shard.py.  Both barriers
(reference: solves inline and queued, the fused cbf_lattice_step; Euclidean HOCBF: main, hard and
wide roles).  Every expectation comes from the whole-lattice oracle step and NumPy
(tests/window_ref.py), never from the library: outputs bit for bit, extents exactly."""
import ctypes as C
import functools

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")
if not torch.cuda.is_available():
    pytest.skip("needs a ROCm GPU", allow_module_level=True)

import cbf_amd  # noqa: E402
from cbf_amd import scenarios, swarm  # noqa: E402
from cbf_amd._lib import CbfHocbf, decode_stats, lib, ptr, stream_handle  # noqa: E402
from oracle import coracle, pyoracle as po  # noqa: E402

from . import window_ref as wr  # noqa: E402

DEV = torch.device("cuda")
W, H = 40, 48
T = 1 / 30
GAIN = scenarios.LATTICE_GAIN
RADIUS = 0.2        # FilterParams.safety_distance, the cull radius
FILTER_BLOCK = 256  # lanes of a filter block (csrc/cbf_device.hpp kBlock)

# lattice name -> (spacing, seed, halo): rows `halo` or more apart are out of y-range of each other
# (0.145: smallest such gap 0.2908; 0.09: 0.2705), rows halo - 1 apart are not
LATTICES = {"sparse": (0.145, 7, 3), "dense": (0.09, 3, 4)}

# config name -> (barrier, solve placement, alpha, lattice)
CONFIGS = {
    "ref-inline": ("reference", "inline", None, "sparse"),
    "ref-queued": ("reference", "queued", None, "sparse"),   # k_lattice_filter_hard and its block records
    "hocbf-1-1": ("euclidean_hocbf", "auto", (1.0, 1.0), "sparse"),
    "hocbf-2-0.5": ("euclidean_hocbf", "auto", (2.0, 0.5), "sparse"),
    "hocbf-dense": ("euclidean_hocbf", "auto", (1.0, 1.0), "dense"),  # 9..20 neighbours: the wide role
}


def _geometries(halo):
    """name -> (rb, re, w0, wrows): the smallest sufficient window of each stripe, one two rows wider
    than needed, and one of 32 rows (W * 32 agents: a whole number of filter blocks)."""
    g = {}
    for name, rb, re in [("bottom", 0, 12), ("interior", 12, 24), ("top", 36, 48), ("single-row", 20, 21),
                         ("whole", 0, 48)]:
        w0, w1 = max(0, rb - halo), min(H, re + halo)
        g[name] = (rb, re, w0, w1 - w0)
    g["wider"] = (12, 24, 12 - halo - 1, 12 + 2 * halo + 2)
    g["block-multiple"] = (12, 24, 2, 32)
    return g


GEOMETRY_NAMES = list(_geometries(3))


def _lattice(lat, shifted):
    spacing, seed, _ = LATTICES[lat]
    pos = scenarios.lattice(W, H, seed=seed, spacing=spacing)
    if shifted:  # every y < 0
        pos[:, 1] -= (H + 4) * spacing
    return pos


@functools.lru_cache(maxsize=None)
def _ref(lat, shifted, barrier, alpha, step=0):
    """Whole-lattice oracle timestep `step` (teacher-forced: its input is the oracle's output of the
    step before), computed once and shared read-only."""
    pos = _lattice(lat, shifted) if step == 0 else _ref(lat, shifted, barrier, alpha, step - 1)["new"]
    vel = coracle.consensus_lattice(W, H, 0, H, pos, GAIN)
    p = po.Params(15)
    if barrier == "reference":
        out = coracle.filter_swarm(p, pos, vel, 0)
    else:
        out = coracle.filter_swarm_hocbf(p, po.HocbfParams(*alpha), pos, vel, 0)
    ref = dict(pos=pos, vel=vel, u=out["u"], status=out["status"], cnt=out["cnt"],
               new=coracle.euler(pos, out["u"], T))
    assert ref["cnt"].max() <= 24  # (no HOCBF neighbour overflow: u would be u0 there)
    for a in ref.values():
        a.setflags(write=False)
    return ref


def _config_ref(config, shifted=False, step=0):
    barrier, _, alpha, lat = CONFIGS[config]
    return _ref(lat, shifted, barrier, alpha, step)


class _Stripe:
    """One stripe's buffers and calls: a zero-filled workspace of its own window geometry, the
    window's positions (not aliasing pos_out), owned-row-sized outputs and a device double[4]."""

    def __init__(self, barrier, pos_full, W, H, rb, re, w0, wrows, guard, params, alpha, want_extents=True,
                 want_stats=False):
        self.barrier, self.W, self.H, self.geom, self.guard = barrier, W, H, (rb, re, w0, wrows), guard
        self.cp = params.c()
        self.hp = CbfHocbf(*(alpha or (1.0, 1.0)))
        self.grid = swarm.grid_for_points(np.asarray(pos_full), params.safety_distance)  # the whole lattice
        self.ws_bytes = lib.cbf_lattice_workspace_size(W, wrows, C.byref(self.grid))
        assert self.ws_bytes > 0
        self.ws = torch.zeros(self.ws_bytes, dtype=torch.uint8, device=DEV)
        n_own = (re - rb) * W
        self.pos = torch.empty((wrows * W, 2), dtype=torch.float64, device=DEV)
        self.pos_out = torch.empty((n_own, 2), dtype=torch.float64, device=DEV)
        self.vel = torch.empty((n_own, 2), dtype=torch.float64, device=DEV)
        self.u = torch.empty((n_own, 2), dtype=torch.float64, device=DEV)
        self.status = torch.empty(n_own, dtype=torch.int32, device=DEV)
        self.cnt = torch.empty(n_own, dtype=torch.int32, device=DEV)
        self.ext = torch.empty(4, dtype=torch.float64, device=DEV) if want_extents else None
        self.stats = torch.zeros(1024, dtype=torch.int64, device=DEV) if want_stats else None
        self.set_pos(pos_full)
        self.poison()

    def set_pos(self, pos_full):
        _, _, w0, wrows = self.geom
        win = np.array(np.asarray(pos_full)[w0 * self.W:(w0 + wrows) * self.W])  # (a writable copy of the window)
        self.pos.copy_(torch.as_tensor(win))

    def poison(self, vel=True):
        """Outputs a kernel fails to write stay recognisable."""
        for t in (self.pos_out, self.u) + ((self.vel,) if vel else ()) + ((self.ext,) if self.ext is not None else ()):
            t.fill_(float("nan"))
        self.status.fill_(-1)
        self.cnt.fill_(-1)
        if self.stats is not None:
            self.stats.zero_()

    def _args(self):
        rb, re, w0, wrows = self.geom
        return (self.cp, C.byref(self.grid), self.W, self.H, rb, re, w0, wrows, ptr(self.pos))

    def _tail(self):
        return (ptr(self.u), ptr(self.status), ptr(self.cnt), self.guard, ptr(self.ext) if self.ext is not None
                else None, ptr(self.stats) if self.stats is not None else None, ptr(self.ws), self.ws_bytes,
                stream_handle())

    def build(self):
        assert lib.cbf_lattice_build(*self._args(), GAIN, ptr(self.vel), ptr(self.ws), self.ws_bytes,
                                     stream_handle()) == 0

    def advance(self):
        if self.barrier == "reference":
            assert lib.cbf_lattice_advance(*self._args(), T, ptr(self.pos_out), *self._tail()) == 0
        else:
            cp, g, *rest = self._args()
            assert lib.cbf_lattice_advance_hocbf(cp, C.byref(self.hp), g, *rest, T, ptr(self.pos_out),
                                                 *self._tail()) == 0

    def step_fused(self):
        assert self.barrier == "reference"
        assert lib.cbf_lattice_step(*self._args(), GAIN, T, ptr(self.pos_out), ptr(self.vel), *self._tail()) == 0

    def result(self):
        torch.cuda.synchronize()
        out = dict(pos=self.pos_out.cpu().numpy(), vel=self.vel.cpu().numpy(), u=self.u.cpu().numpy(),
                   status=self.status.cpu().numpy(), cnt=self.cnt.cpu().numpy(),
                   extents=None if self.ext is None else self.ext.cpu().numpy())
        if self.stats is not None:
            out["solves"] = decode_stats(self.stats.cpu().numpy())["solves"]
        return out


def _stripe(barrier, pos_full, W, H, rb, re, w0, wrows, guard, params, alpha, fused, **kw):
    """One stripe through the public ABI: cbf_lattice_build then cbf_lattice_advance /
    cbf_lattice_advance_hocbf, or the fused cbf_lattice_step (reference barrier)."""
    S = _Stripe(barrier, pos_full, W, H, rb, re, w0, wrows, guard, params, alpha, **kw)
    if fused:
        S.step_fused()
    else:
        S.build()
        S.advance()
    return S.result()


def _config_stripe(config, pos_full, geom, guard, fused=False, **kw):
    barrier, placement, alpha, _ = CONFIGS[config]
    return _stripe(barrier, pos_full, W, H, *geom, guard, swarm.FilterParams(solve_placement=placement), alpha,
                   fused, **kw)


def _bits(a):
    return a.view(np.int64) if a.dtype == np.float64 else a


def _check(out, ref, rb, re, guard, what=""):
    """The stripe's outputs against the owned rows of the whole-lattice oracle step, bit for bit,
    and its extents against the oracle's new owned y, exactly."""
    sl = slice(rb * W, re * W)
    for key, want in (("vel", ref["vel"]), ("cnt", ref["cnt"]), ("status", ref["status"]), ("u", ref["u"]),
                      ("pos", ref["new"])):
        got, want = out[key], np.ascontiguousarray(want[sl])
        bad = np.flatnonzero((_bits(got) != _bits(want)).reshape(got.shape[0], -1).any(axis=1))
        assert bad.size == 0, (what, key, bad[:8], got[bad[:4]], want[bad[:4]])
    if out["extents"] is not None:
        want = wr.expected_extents(ref["new"], W, rb, re, guard)
        assert np.array_equal(out["extents"], want), (what, "extents", guard, out["extents"], want)


# ---- 1. stripes x barriers ----

@pytest.mark.parametrize("geometry", GEOMETRY_NAMES)
@pytest.mark.parametrize("config", list(CONFIGS))
def test_stripe_vs_oracle(config, geometry):
    halo = LATTICES[CONFIGS[config][3]][2]
    rb, re, w0, wrows = geom = _geometries(halo)[geometry]
    ref = _config_ref(config)
    assert wr.window_sufficient(ref["pos"], W, H, rb, re, w0, wrows, RADIUS)
    assert (W * wrows % FILTER_BLOCK == 0) == (geometry == "block-multiple")
    own_cnt = ref["cnt"][rb * W:re * W]
    assert own_cnt.max() > 0
    if CONFIGS[config][3] == "dense":  # the wide role (more than 8 neighbours), none over the cap
        assert int((ref["cnt"] > 8).sum()) == 1832 and ref["cnt"].max() == 20
        if re - rb >= 12:
            assert (own_cnt > 8).any() and (own_cnt <= 8).any()
    for guard in (0, halo - 1, re - rb):
        out = _config_stripe(config, ref["pos"], geom, guard)
        _check(out, ref, rb, re, guard, (config, geometry))
        if guard == re - rb:
            assert out["extents"][2] == -np.inf and out["extents"][3] == np.inf


# ---- 2. the fused step, once per solve placement ----

@pytest.mark.parametrize("config", ["ref-inline", "ref-queued"])
def test_fused_step_stripe(config):
    geom = _geometries(3)["interior"]
    ref = _config_ref(config)
    assert wr.window_sufficient(ref["pos"], W, H, *geom, RADIUS)
    out = _config_stripe(config, ref["pos"], geom, 2, fused=True, want_stats=True)
    _check(out, ref, geom[0], geom[1], 2, (config, "fused"))
    assert out["solves"] == int((ref["cnt"][geom[0] * W:geom[1] * W] > 0).sum()) > 0  # counted over the owned rows


# ---- 3. sign of y ----

@pytest.mark.parametrize("config", ["ref-queued", "hocbf-1-1", "hocbf-dense"])
def test_stripe_negative_y(config):
    """The same lattice with every y < 0 (and the oracle run on it): a record of zeros left in the
    workspace would cap e1 and e2 from below here, as it caps e0 and e3 from above for y > 0."""
    halo = LATTICES[CONFIGS[config][3]][2]
    rb, re, w0, wrows = geom = _geometries(halo)["interior"]
    ref = _config_ref(config, shifted=True)
    assert ref["pos"][:, 1].max() < 0 and ref["new"][rb * W:re * W, 1].max() < 0
    assert _config_ref(config)["new"][rb * W:re * W, 1].min() > 0  # (the positive-y case is test_stripe_vs_oracle's)
    assert wr.window_sufficient(ref["pos"], W, H, rb, re, w0, wrows, RADIUS)
    for guard in (0, halo - 1):
        out = _config_stripe(config, ref["pos"], geom, guard)
        _check(out, ref, rb, re, guard, (config, "y < 0"))


# ---- 4. reuse of one workspace ----

@pytest.mark.parametrize("config", ["ref-queued", "hocbf-1-1", "hocbf-dense"])
def test_workspace_reuse_keeps_no_records(config):
    """One workspace: the advance twice on one build, then a teacher-forced second timestep, then
    another stripe of the same window shape -- each time the outputs, extents and solve count of a
    fresh call (no extents record, queue entry or count left from the call before)."""
    barrier, placement, alpha, lat = CONFIGS[config]
    halo = LATTICES[lat][2]
    rb, re, w0, wrows = _geometries(halo)["interior"]
    guard = halo - 1
    ref0, ref1 = _config_ref(config), _config_ref(config, step=1)
    for r in (ref0, ref1):
        assert wr.window_sufficient(r["pos"], W, H, rb, re, w0, wrows, RADIUS)
    S = _Stripe(barrier, ref0["pos"], W, H, rb, re, w0, wrows, guard, swarm.FilterParams(solve_placement=placement),
                alpha, want_stats=True)
    n_solves = int((ref0["cnt"][rb * W:re * W] > 0).sum())
    S.build()
    outs = []
    for _ in range(2):
        S.set_pos(ref0["pos"])
        S.poison(vel=False)  # (vel_out is the build's)
        S.advance()
        outs.append(S.result())
        _check(outs[-1], ref0, rb, re, guard, (config, "advance", len(outs)))
        assert outs[-1]["solves"] == n_solves > 0
    for k in outs[0]:
        assert np.array_equal(outs[0][k], outs[1][k]), k
    # second timestep from the oracle's positions after the first
    S.set_pos(ref1["pos"])
    S.poison()
    S.build()
    S.advance()
    _check(S.result(), ref1, rb, re, guard, (config, "timestep 2"))
    # the stripe above, same window shape (its y lie above every record the workspace has seen)
    up = re - rb
    assert wr.window_sufficient(ref0["pos"], W, H, rb + up, re + up, w0 + up, wrows, RADIUS)
    S.geom = (rb + up, re + up, w0 + up, wrows)
    S.set_pos(ref0["pos"])
    S.poison()
    S.build()
    S.advance()
    _check(S.result(), ref0, rb + up, re + up, guard, (config, "next stripe"))


# ---- 5. extents = NULL ----

@pytest.mark.parametrize("config", ["ref-inline", "ref-queued", "hocbf-1-1"])
def test_extents_null_changes_nothing_else(config):
    halo = LATTICES[CONFIGS[config][3]][2]
    rb, re, w0, wrows = geom = _geometries(halo)["interior"]
    ref = _config_ref(config)
    a = _config_stripe(config, ref["pos"], geom, halo - 1)
    b = _config_stripe(config, ref["pos"], geom, halo - 1, want_extents=False)
    assert a["extents"] is not None and b["extents"] is None
    for k in ("pos", "vel", "u", "status", "cnt"):
        assert np.array_equal(_bits(a[k]), _bits(b[k])), k
    _check(b, ref, rb, re, halo - 1, (config, "extents = NULL"))


# ---- 6. cbf_halo_guard on crafted records ----

def _guard_scenarios(ws, rank):
    """(name, records (ws, 4), clear?) for rank of ws: rank q's owned y span [100 (q - rank),
    100 (q - rank) + 50], its rows outside a neighbour's halo [.. + 10, .. + 40]."""
    rm = wr.guard_radius(RADIUS)
    base = np.array([[100.0 * (q - rank), 100.0 * (q - rank) + 50, 100.0 * (q - rank) + 40, 100.0 * (q - rank) + 10]
                     for q in range(ws)])
    yield "all clear", base, True

    def mod(*edits):
        r = base.copy()
        for q, k, v in edits:
            r[q, k] = v
        return r
    if rank > 0:
        yield "rank-1 e2 in range", mod((rank - 1, 2, -0.1), (rank - 1, 1, -0.1)), False
        yield "rank-1 e1 inside the halo", mod((rank - 1, 1, 5.0)), True
        yield "below: gap == rm", mod((rank, 0, rm), (rank - 1, 2, 0.0), (rank - 1, 1, 5.0)), False
        yield "below: gap just over rm", mod((rank, 0, np.nextafter(rm, np.inf)), (rank - 1, 2, 0.0),
                                             (rank - 1, 1, 5.0)), True
        yield "rank-1 NaN", mod(*[(rank - 1, k, np.nan) for k in range(4)]), False
    if rank < ws - 1:
        yield "rank+1 e3 in range", mod((rank + 1, 3, 50.1), (rank + 1, 0, 50.1)), False
        yield "rank+1 e0 inside the halo", mod((rank + 1, 0, 45.0)), True
        top = [(rank, 0, -50.0), (rank, 1, 0.0), (rank, 2, -10.0), (rank, 3, -40.0), (rank + 1, 0, -5.0)]
        yield "above: gap == rm", mod(*top, (rank + 1, 3, rm)), False
        yield "above: gap just over rm", mod(*top, (rank + 1, 3, np.nextafter(rm, np.inf))), True
        yield "rank+1 NaN", mod(*[(rank + 1, k, np.nan) for k in range(4)]), False
    if rank > 1:
        yield "rank-2 e1 in range", mod((rank - 2, 1, -0.1)), False
    if rank < ws - 2:
        yield "rank+2 e0 in range", mod((rank + 2, 0, 50.1)), False
    if ws > 1:
        yield "own record NaN", mod(*[(rank, k, np.nan) for k in range(4)]), False


@pytest.mark.parametrize("stride", [4, 8])
def test_halo_guard_records(stride):
    """k_halo_guard alone: the flag it ORs in against the brute-force guard over the y-sets the
    records stand for (tests/window_ref.py), each scenario also pinned to its intended outcome."""
    n = 0
    for ws in (1, 2, 3, 4):
        for rank in range(ws):
            for name, recs, clear in _guard_scenarios(ws, rank):
                want_clear = wr.brute_guard_records(recs, rank, RADIUS)
                assert want_clear == clear, (ws, rank, name)
                buf = np.full((ws, stride), np.nan)  # (padding of a wider record is never read)
                buf[:, :4] = recs
                E = torch.as_tensor(buf, device=DEV)
                for pre in (0, 1, 6):
                    flag = torch.tensor([pre, 77], dtype=torch.int32, device=DEV)
                    assert lib.cbf_halo_guard(ptr(E), stride, ws, rank, RADIUS, ptr(flag), stream_handle()) == 0
                    got = flag.cpu().numpy()
                    assert got[0] == (pre | (0 if want_clear else 1)) and got[1] == 77, (ws, rank, name, pre, got)
                    n += 1
    assert n == 3 * 85  # scenarios over the 10 (world size, rank) pairs


# ---- 7. composition: three stripes + the guard, as the header documents ----

@pytest.mark.parametrize("halo", [3, 2, 1])
@pytest.mark.parametrize("config", ["ref-queued", "hocbf-1-1"])
def test_three_stripes_compose(config, halo):
    """Stripes of 16 rows over windows of +- halo rows with guard_rows = halo - 1, their extents
    gathered and cbf_halo_guard run for every rank.  halo = 3 is wide enough at this spacing: no
    flag, and the concatenated outputs are the whole-lattice step.  halo = 2 and 1 are not: every
    rank must say so (a wrong-halo answer that is reported, not a fault)."""
    ref = _config_ref(config)
    stripes = [(0, 16), (16, 32), (32, 48)]
    ext_all = torch.full((3, 4), float("nan"), dtype=torch.float64, device=DEV)
    outs = []
    windows = [(max(0, rb - halo), min(H, re + halo) - max(0, rb - halo)) for rb, re in stripes]  # (w0, wrows)
    for q, ((rb, re), (w0, wrows)) in enumerate(zip(stripes, windows)):
        outs.append(_config_stripe(config, ref["pos"], (rb, re, w0, wrows), halo - 1))
        ext_all[q].copy_(torch.as_tensor(outs[-1]["extents"]))
    want = [0 if wr.brute_guard_positions(ref["new"], W, H, rb, re, halo - 1, RADIUS) else 1 for rb, re in stripes]
    assert want == ([0, 0, 0] if halo == 3 else [1, 1, 1])
    flags = torch.zeros(3, dtype=torch.int32, device=DEV)
    for q in range(3):
        assert lib.cbf_halo_guard(ptr(ext_all), 4, 3, q, RADIUS, ptr(flags[q:]), stream_handle()) == 0
    assert flags.cpu().numpy().tolist() == want, ext_all.cpu().numpy()
    if halo == 3:
        for out, (rb, re), (w0, wrows) in zip(outs, stripes, windows):
            assert wr.window_sufficient(ref["pos"], W, H, rb, re, w0, wrows, RADIUS)
            _check(out, ref, rb, re, halo - 1, (config, "compose", rb))
        assert np.array_equal(np.concatenate([o["pos"] for o in outs]), ref["new"])
        assert np.array_equal(np.concatenate([o["u"] for o in outs]), ref["u"])
        assert cbf_amd.STATUS_NBR_OVERFLOW not in set(np.concatenate([o["status"] for o in outs]) & 0xFF)
