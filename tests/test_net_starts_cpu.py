"""CPU: the upper bound from many starts.  The entry points gnnb_net_starts / gnnb_net_descend_starts (with its
workspace and tile functions) are declared, bound and exported, their kernels have one profile class each, they refuse a null handle and
every value outside its range with a message that names them and the value; the five drivers reject bad restart options before they touch
a device; and the Python restatement of gnnb_net_starts' generator, which tests/test_gpu_net_starts.py holds the device to bit for bit,
meets its known answers and its own properties.  (A handle needs a GPU to exist: the other refusals are in the GPU file.)"""
import struct
from fractions import Fraction

import numpy as np
import pytest

from gnn_branching_amd import _lib, frontier
from tests.test_frontier_cpu import NoDevice
from tests.test_frontier_jobs_cpu import job

NEW = ("gnnb_net_starts", "gnnb_net_descend_starts", "gnnb_net_descend_starts_workspace_bytes", "gnnb_net_descend_starts_tile")
NEW_CLASSES = ("k_net_starts", "k_net_descend_tile", "k_net_starts_pick")

# ---- the restatement of gnnb_net_starts (include/gnnb.h) -----------------------------------------------------------------------------
M64 = (1 << 64) - 1
G = 0x9E3779B97F4A7C15


def mix(z):
    """The splitmix64 finaliser, mod 2^64."""
    z &= M64
    z = ((z ^ (z >> 30)) * 0xBF58476D1CE4E5B9) & M64
    z = ((z ^ (z >> 27)) * 0x94D049BB133111EB) & M64
    return z ^ (z >> 31)


def bits32(x):
    return struct.unpack("<I", struct.pack("<f", x))[0] if not isinstance(x, np.float32) else int(np.array(x, dtype=np.float32).view(np.uint32))


def row_key(x0, seed, order=None):
    """seed + the sum over the row's coordinates, in ``order`` (None: ascending); x0: the row's fp32 values, flat."""
    bits = np.ascontiguousarray(x0, dtype=np.float32).view(np.uint32).tolist()
    k = seed
    for m in (range(len(bits)) if order is None else order):
        k = (k + mix(bits[m] + (m << 32))) & M64
    return k


def uniform(key, r, m, N0):
    """u(b, r, m): a multiple of 2^-53 in [0, 1), exact as a float."""
    return (mix(key + G * (r * N0 + m + 1)) >> 11) * 2.0 ** -53


def inside32(v, lo, hi):
    """The fp64 value v rounded to the nearest fp32 and moved to the neighbouring float inside [lo, hi] where rounding left it."""
    f = np.float32(v)
    if float(f) < lo:
        f = np.nextafter(f, np.float32(np.inf))
    elif float(f) > hi:
        f = np.nextafter(f, np.float32(-np.inf))
    return f


def fma_point(lo, hi, u):
    """fma(hi - lo, u, lo): the width rounded to fp64, then ONE correct rounding of the exact width * u + lo."""
    return float(Fraction(hi - lo) * Fraction(u) + Fraction(lo))


def two_rounding_point(lo, hi, u):
    return lo + (hi - lo) * u


def start_points(x0, x_lo, x_hi, R, seed):
    """Row b's (R + 1, N_0) fp32 start points: slot 0 is x0, slot r >= 1 the generator's.  x0: (N_0,) fp32; x_lo / x_hi: (N_0,) fp64."""
    x0 = np.ascontiguousarray(x0, dtype=np.float32).reshape(-1)
    lo, hi = np.asarray(x_lo, dtype=np.float64).reshape(-1).tolist(), np.asarray(x_hi, dtype=np.float64).reshape(-1).tolist()
    N0, key = x0.size, row_key(x0, seed)
    out = np.empty((R + 1, N0), dtype=np.float32)
    out[0] = x0
    for r in range(1, R + 1):
        for m in range(N0):
            out[r, m] = inside32(fma_point(lo[m], hi[m], uniform(key, r, m, N0)), lo[m], hi[m])
    return out


# ---- the library -----------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def lib():
    _lib.build_library()
    return _lib.load()


def starts(lib, h, B=2, R=3, seed=0):
    return lib.gnnb_net_starts(h, None, None, None, B, R, seed, None, None)


def descend_starts(lib, h, B=2, n_starts=3, n_steps=1, step=0.5):
    return lib.gnnb_net_descend_starts(h, None, n_starts, *([None] * 4), B, n_steps, step, *([None] * 5), None, 0, None)


def test_new_symbols_are_declared_bound_and_exported(lib):
    names = {s[0] for s in _lib.SYMBOLS}
    header = open(_lib.CSRC + "/../../include/gnnb.h").read()
    for n in NEW:
        assert n in names and hasattr(lib, n) and n + "(" in header, n
    assert lib.gnnb_abi_version() == 2 and "#define GNNB_ABI_VERSION 2" in header      # the additions are additive
    assert "gnnb_k_starts.h" in _lib.SOURCES and "gnnb_k_net.h" in _lib.SOURCES
    assert lib.gnnb_net_descend_starts_tile() >= 1
    from gnn_branching_amd.engine import ScorerEngine
    for m in ("net_starts", "net_descend_starts"):
        assert callable(getattr(ScorerEngine, m)), m


def test_every_new_kernel_has_one_profile_class_and_no_name_is_doubled(lib):
    classes = [lib.gnnb_profile_class_name(i).decode() for i in range(lib.gnnb_profile_classes())]
    for k in NEW_CLASSES + ("k_net_descend", "k_net_eval"):
        assert classes.count(k) == 1, k
    assert len(set(classes)) == len(classes) and "" not in classes


def test_null_handle_is_refused_with_a_message(lib):
    for name, call in (("gnnb_net_starts", lambda: starts(lib, None)), ("gnnb_net_descend_starts", lambda: descend_starts(lib, None))):
        assert call() == -1, name
        msg = lib.gnnb_last_error()
        assert name.encode() + b":" in msg and b"null handle" in msg, (name, msg)
    assert lib.gnnb_net_descend_starts_workspace_bytes(None, 4, 5) == 0


@pytest.mark.parametrize("kw,word", [({"B": 0}, "B = 0"), ({"B": -2}, "B = -2"), ({"R": -1}, "R = -1"), ({"R": 4097}, "R = 4097")])
def test_starts_refuses_values_outside_their_ranges_with_a_message(lib, kw, word):
    assert starts(lib, None, **kw) == -1
    msg = lib.gnnb_last_error()
    assert b"gnnb_net_starts:" in msg and word.encode() in msg and b"null handle" not in msg, msg


@pytest.mark.parametrize("kw,word", [({"B": 0}, "B = 0"), ({"B": -2}, "B = -2"), ({"n_starts": 0}, "n_starts = 0"), ({"n_starts": -1}, "n_starts = -1"),
                                     ({"n_starts": 4098}, "n_starts = 4098"), ({"n_steps": -1}, "n_steps = -1"), ({"step": 0.0}, "step = 0"),
                                     ({"step": -0.25}, "step = -0.25"), ({"step": 1.5}, "step = 1.5"), ({"step": float("nan")}, "step = nan"),
                                     ({"step": float("inf")}, "step = inf")])
def test_descend_starts_refuses_values_outside_their_ranges_with_a_message(lib, kw, word):
    assert descend_starts(lib, None, **kw) == -1
    msg = lib.gnnb_last_error()
    assert b"gnnb_net_descend_starts:" in msg and word.encode() in msg and b"null handle" not in msg, msg


# ---- the options of the five drivers ---------------------------------------------------------------------------------------------------
BAD = [{"pgd_steps": 4, "pgd_restarts": -1}, {"pgd_steps": 4, "pgd_restarts": True}, {"pgd_steps": 4, "pgd_restarts": False},
       {"pgd_steps": 4, "pgd_restarts": 2.0}, {"pgd_steps": 4, "pgd_restarts": "3"}, {"pgd_steps": 4, "pgd_restarts": 4097},
       {"pgd_restarts": 3}, {"pgd_restarts": 0},                                                                  # needs pgd_steps
       {"pgd_steps": 4, "pgd_restarts": 3, "pgd_seed": -1}, {"pgd_steps": 4, "pgd_restarts": 3, "pgd_seed": 2 ** 64},
       {"pgd_steps": 4, "pgd_restarts": 3, "pgd_seed": True}, {"pgd_steps": 4, "pgd_restarts": 3, "pgd_seed": 1.0},
       {"pgd_steps": 4, "pgd_restarts": 3, "pgd_seed": None}, {"pgd_seed": "7"}]


@pytest.mark.parametrize("kw", BAD)
def test_bad_options_are_rejected_before_a_device_is_touched(kw):
    with pytest.raises(ValueError):
        frontier.branch_and_bound_frontier(NoDevice(), NoDevice(), [], K=4, **kw)
    with pytest.raises(ValueError):
        frontier.branch_and_bound_frontier(NoDevice(), NoDevice(), [], K=4, branching_threshold=0.5, **kw)
    with pytest.raises(ValueError):
        frontier.FrontierRun(NoDevice(), NoDevice(), [], K=4, **kw)
    with pytest.raises(ValueError):
        frontier.verify_properties(NoDevice(), [], frontier.FrontierJobs([job()], **kw), K=4)
    with pytest.raises(ValueError):
        frontier.verify_properties_threshold(NoDevice(), [], frontier.FrontierJobs([job()], **kw), 0.5, K=4)


def test_good_options_pass_the_check():
    for kw in ({}, {"pgd_steps": 0, "pgd_restarts": 0}, {"pgd_steps": 0, "pgd_restarts": 64}, {"pgd_steps": 4, "pgd_restarts": 4096},
               {"pgd_steps": 4, "pgd_restarts": 3, "pgd_seed": 2 ** 64 - 1}, {"pgd_seed": 5}, {"pgd_steps": 4, "pgd_restarts": None}):
        frontier._check_restarts(kw.get("pgd_restarts"), kw.get("pgd_seed", 0), kw.get("pgd_steps"))


def test_the_jobs_loops_take_the_options_on_their_jobs_and_upper_of_is_unchanged():
    point = []
    jobs = frontier.FrontierJobs([job(), job()], witness=point, pgd_steps=4, pgd_step=0.25, pgd_restarts=3, pgd_seed=11)
    assert isinstance(jobs, list) and len(jobs) == 2
    assert frontier._options_of(jobs) == {"witness": point, "pgd_steps": 4, "pgd_step": 0.25, "pgd_restarts": 3, "pgd_seed": 11}
    assert frontier._options_of(jobs)["witness"] is point
    assert frontier._options_of(list(jobs)) == {}
    assert frontier._options_of(frontier.FrontierJobs([job()])) == {"witness": None, "pgd_steps": None, "pgd_step": 1.0 / 64, "pgd_restarts": None,
                                                                    "pgd_seed": 0}


# ---- the generator's restatement -------------------------------------------------------------------------------------------------------
def test_known_answers_of_the_finaliser():
    assert mix(G) == 0xE220A8397B1DCDAF
    assert mix(2 * G) == 0x6E789E6AA1B965F4


def row(seed, N0=37):
    rng = np.random.RandomState(seed)
    x0 = rng.uniform(-1, 1, N0).astype(np.float32)
    lo = x0.astype(np.float64) - rng.uniform(0.01, 0.3, N0)          # widths that are no powers of two
    hi = x0.astype(np.float64) + rng.uniform(0.01, 0.3, N0)
    return x0, lo, hi


def test_u_lies_in_the_unit_interval_and_is_exact():
    x0, _, _ = row(3)
    key = row_key(x0, 5)
    us = [uniform(key, r, m, x0.size) for r in range(1, 40) for m in range(x0.size)]
    assert min(us) >= 0.0 and max(us) < 1.0
    assert all(float(Fraction(u) * 2 ** 53).is_integer() for u in us)
    assert len(set(us)) == len(us) and 0.4 < sum(us) / len(us) < 0.6
    assert (M64 >> 11) * 2.0 ** -53 < 1.0                                # the largest value the hash can give


def test_the_key_does_not_depend_on_the_order_of_the_sum():
    x0, _, _ = row(4)
    want = row_key(x0, 99)
    rng = np.random.RandomState(0)
    for _ in range(4):
        assert row_key(x0, 99, order=rng.permutation(x0.size).tolist()) == want
    assert row_key(x0, 100) == (want + 1) & M64
    other = x0.copy()
    other[5] = np.nextafter(other[5], np.float32(2))
    assert row_key(other, 99) != want
    nan = x0.copy()
    nan[3] = np.float32("nan")                                           # a NaN hashes by its bits
    assert row_key(nan, 99) == row_key(nan.copy(), 99) != want


SEED = 7                            # the seed on which the fma and the two-rounding form differ on `row(SEED)` (asserted below)


def test_the_start_is_one_rounding_and_lies_inside_the_box():
    x0, lo, hi = row(SEED)
    pts = start_points(x0, lo, hi, 6, SEED)
    assert pts.dtype == np.float32 and np.array_equal(pts[0].view(np.uint32), x0.view(np.uint32))
    assert bool((pts.astype(np.float64) >= lo).all()) and bool((pts.astype(np.float64) <= hi).all())
    key, N0, differ = row_key(x0, SEED), x0.size, 0
    for r in range(1, 7):
        for m in range(N0):
            u = uniform(key, r, m, N0)
            differ += fma_point(float(lo[m]), float(hi[m]), u) != two_rounding_point(float(lo[m]), float(hi[m]), u)
    assert differ > 0, "choose another seed: the two forms agree at every coordinate"
    # a degenerate coordinate is that value, and a box of fp32 corners needs no move
    assert fma_point(0.25, 0.25, 0.7) == 0.25 and inside32(0.25, 0.25, 0.25) == np.float32(0.25)
    # rounding to fp32 can leave the box: the move brings the point back
    hi1 = float(np.nextafter(np.float64(np.float32(0.1)), -1.0))         # just below an fp32 value: hi1 rounds up and out
    assert float(np.float32(hi1)) > hi1 and hi1 - 0.05 <= float(inside32(hi1, hi1 - 0.05, hi1)) <= hi1


def test_two_seeds_and_two_rows_differ():
    x0, lo, hi = row(SEED)
    a, b = start_points(x0, lo, hi, 2, 1), start_points(x0, lo, hi, 2, 2)
    assert np.array_equal(a[0], b[0]) and not np.array_equal(a[1:], b[1:])
    y0 = x0.copy()
    y0[0] = np.nextafter(y0[0], np.float32(2))
    assert not np.array_equal(start_points(y0, lo, hi, 2, 1)[1:], a[1:])
