"""The cases of the evaluation sweeps (tests/test_eval_ksteps.py: every
compile-time k-step count of the D <= 60 evaluation on non-square grids;
tests/test_eval_phase_range.py: the branch points of its phase reduction).

Geometry, coefficient rows and references only -- numpy and the oracle, no
GPU -- so the CPU companion test can pin the same inputs the GPU tests run.
Everything returned from a cached function is shared: do not modify it.
"""

import functools

import numpy as np

from conftest import FIELD
from oracle import geometry as og
from oracle import kl as okl

# (ny, nx) of the k-step sweep: whole 64-pixel wave blocks with partial 256-,
# 512- and 1024-pixel runs; float4 stores with a partial wave block; odd
# (scalar stores, the register tile for everything)
GRIDS = ((40, 56), (18, 20), (19, 17))
# whole wave blocks (15 x 64), a partial 256-pixel block
WAVE_GRID = (24, 40)
S_SWEEP = 37      # two whole 16-slot groups and a 5-slot tail
NAN_ROW, INF_ROW = 9, 31
BIG_ROWS = slice(20, 30)


def ksteps(D):
    return (D + 3) // 4


@functools.lru_cache(maxsize=None)
def piercepoints(D):
    """[D, 3] piercepoints of D synthetic directions (and the field centre
    the grid coordinates are taken about)."""
    from ska_sdp_screen_fitting_amd.synthetic import make_solutions
    s = make_solutions(n_ant=2, n_time=2, n_freq=1, n_dir=D, seed=4)
    return og.piercepoints(s.dir_radec)


@functools.lru_cache(maxsize=None)
def grid(D, ny, nx):
    """(x [nx], y [ny]): the leading coordinates of the usual square test
    grid of max(ny, nx) cells -- different lengths and different values."""
    _, mra, mdec = piercepoints(D)
    n = max(ny, nx)
    cell = FIELD["width"] / (n - 0.5)
    x, y = og.grid_coords(FIELD["rad"], FIELD["dec"], FIELD["width"], cell,
                          mra, mdec)
    assert len(x) == n and len(y) == n
    x, y = np.ascontiguousarray(x[:nx]), np.ascontiguousarray(y[:ny])
    assert not np.array_equal(x[:min(nx, ny)], y[:min(nx, ny)])
    return x, y


@functools.lru_cache(maxsize=None)
def cpix(D, ny, nx, swap=False):
    """The oracle's pixel basis [ny * nx, D] (swap: x and y exchanged, i.e.
    the transposed grid [nx * ny, D])."""
    x, y = grid(D, ny, nx)
    if swap:
        x, y = y, x
    return okl.cpix_matrix(piercepoints(D)[0], x, y)


@functools.lru_cache(maxsize=None)
def sweep_rows(D):
    """[37, D] phase coefficients of the sweep: normal(0, 0.01), ten rows of
    many turns, one NaN and one Inf row."""
    rng = np.random.default_rng(1000 + D)
    coef = rng.normal(0, 0.01, size=(S_SWEEP, D))
    coef[BIG_ROWS] *= 300.0
    coef[NAN_ROW, D // 2] = np.nan
    coef[INF_ROW, 0] = np.inf
    return coef


def finite_rows(coef):
    return np.isfinite(coef).all(axis=1)


def planes_f64(coef, cp):
    """The fp64 oracle's Jones planes [S, 4, P] of finite rows."""
    return okl.eval_planes(okl.eval_phase_screens(coef, cp))


@functools.lru_cache(maxsize=None)
def gain_rows(D, ny, nx):
    """(phase, log10 A_XX, log10 A_YY) rows [37, D] scaled as
    test_gain.py::test_gain_eval_kernels_agree scales them: phases of many
    turns, |log2 A| up to 60, NaN / Inf in each of the three."""
    rng = np.random.default_rng(7 * D + nx)
    S = S_SWEEP
    ph = rng.normal(0, 0.01, (S, D))
    ph[BIG_ROWS] *= 300.0
    ax = rng.normal(0, 0.002, (S, D))
    ay = rng.normal(0, 0.002, (S, D))
    big = ax[32:36] @ cpix(D, ny, nx).T * np.log2(10.0)
    ax[32:36] *= 60.0 / np.abs(big).max()
    ph[NAN_ROW, D // 2] = np.nan
    ph[INF_ROW, 0] = np.inf
    ax[12, D - 1] = np.nan
    ay[17, 0] = np.inf
    return ph, ax, ay


# ------------------------------------------------------------ high precision

LD_OK = np.finfo(np.longdouble).nmant >= 63
TWO_PI_LD = np.longdouble("6.283185307179586476925286766559005768")


def rev_reference(coef, cp):
    """Phase in turns [S, P] in extended precision (fp64 when this platform's
    long double is no wider: see LD_OK), then the residual rev - rint(rev) in
    fp64 and max |rev|."""
    if LD_OK:
        rev = (np.asarray(coef, np.longdouble) @ np.asarray(cp, np.longdouble).T) / TWO_PI_LD
    else:
        rev = (np.asarray(coef, np.float64) @ cp.T) / (2.0 * np.pi)
    frac = (rev - np.rint(rev)).astype(np.float64)
    return frac, float(np.abs(rev).max())


def planes_from_frac(frac):
    a = 2.0 * np.pi * frac
    c, s = np.cos(a), np.sin(a)
    return np.stack([c, s, c, s], axis=-2)


def range_tolerance(D, rev_max):
    """2e-6 (the fast epilogue's own bound) + the contraction's accumulation:
    KS fp64 roundings at the magnitude of the accumulators, which start at
    kRevMagic = 1.5 * 2^20 up to 11 k-steps and at 0 above."""
    ks = ksteps(D)
    at = (1.5 * 2.0 ** 20 + rev_max) if ks <= 11 else rev_max
    return 2e-6 + 2.0 * np.pi * ks * float(np.spacing(at))


# ------------------------------------------------- fixed-point boundary rows

F_SAFE, F_EXACT, F_HUGE = 0.9, 1.2, 8.0
FIXED_D = (1, 7, 20, 40)     # D = 1 and the auto LDS16H / LDS16 / LDS4 ranges
# 16-slot groups of fixed_rows
G_SAFE, G_EXACT, G_HUGE, G_MIX_SAFE, G_MIX_SMALL, G_SMALL = range(6)


def rev_threshold(cp):
    """The library's rule (sf_set_grid): a 16-slot group takes the fixed-point
    epilogue when every lane's sum |coef| / 2 pi is below
    2^15 / (1.01 max |Cpix|)."""
    return 32768.0 / (1.01 * np.abs(cp).max())


def lane_sums(coef):
    """[S, 4] sum |coef| / 2 pi over the directions d % 4 = c of each of the
    four lane classes (a lane of the MFMA A fragment holds one class)."""
    t = np.abs(coef) / (2.0 * np.pi)
    return np.stack([t[:, c::4].sum(axis=1) for c in range(4)], axis=1)


def _lane_rows(rng, n, D, target):
    """n rows of positive coefficients whose lane sums are all `target`
    turns (the classes that hold a direction)."""
    w = rng.uniform(0.5, 1.0, size=(n, D))
    for c in range(min(4, D)):
        w[:, c::4] /= w[:, c::4].sum(axis=1, keepdims=True)
    return w * (2.0 * np.pi * target)


@functools.lru_cache(maxsize=None)
def fixed_rows(D, ny, nx):
    """[96, D] rows around the fixed-point bound of the grid, six 16-slot
    groups: safe (f = 0.9), exact (1.2), huge (8), 15 of the safe rows with
    one exact row, 15 small rows with one exact row, the small rows alone."""
    thr = rev_threshold(cpix(D, ny, nx))
    rng = np.random.default_rng(77 + D)
    safe = _lane_rows(rng, 16, D, F_SAFE * thr)
    exact = _lane_rows(rng, 16, D, F_EXACT * thr)
    huge = _lane_rows(rng, 16, D, F_HUGE * thr)
    small = rng.normal(0, 0.01, size=(16, D))
    mix_safe = np.concatenate([safe[:15], exact[3:4]])
    mix_small = np.concatenate([small[:15], exact[5:6]])
    return np.concatenate([safe, exact, huge, mix_safe, mix_small, small])


def group(g):
    return slice(16 * g, 16 * g + 16)


# ------------------------------------------------- integer-digit boundary rows

TAU = 44                                  # cq = rint(coef / 2 pi 2^44)
M6 = (256 ** 6 - 1) // 255                # 6 balanced base-256 digits of 1
K_POS = 127 * M6 / 2.0 ** TAU             # 7.969 turns
K_NEG = -128 * M6 / 2.0 ** TAU            # -8.031 turns
INV_2PI = 0.15915494309189535             # the kernels' prescale
INT_D = (45, 60)
N_INT = 16


def fixed_point_turns(coef):
    """rint(coef / 2 pi 2^44) as Python integers, as the digit prepass
    takes it (the fp64 product with the prescale, then ldexp and rint)."""
    y = np.ldexp(np.asarray(coef, np.float64) * INV_2PI, TAU)
    return [[int(v) for v in row] for row in np.rint(y)]


@functools.lru_cache(maxsize=None)
def int_rows(D):
    """(inside, outside) [16, D] each.  inside: every coefficient within
    0.07 turn of the digit range's ends, signs mixed -- the largest legal
    digits in every K position; outside: the same rows with one coefficient
    moved just past the end of its sign."""
    assert 7.968 < K_POS < 7.970 and -8.032 < K_NEG < -8.030
    rng = np.random.default_rng(500 + D)
    pos = rng.uniform(7.90, 7.968, size=(N_INT, D))
    neg = rng.uniform(-8.030, -7.90, size=(N_INT, D))
    turns = np.where(rng.random((N_INT, D)) < 0.5, pos, neg)
    out = turns.copy()
    for s in range(N_INT):
        d = (7 * s + 3) % D
        out[s, d] = 7.970 if s % 2 == 0 else -8.032
    return turns * (2.0 * np.pi), out * (2.0 * np.pi)
