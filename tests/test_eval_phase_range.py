"""The branch points of the evaluation's phase reduction, hit by finite data.

Fixed point (kl_eval_impl.h kRevMagic, up to 11 k-steps): a 16-slot group
takes the fixed-point epilogue when every lane's sum |coef| / 2 pi is below
rev_thr = 2^15 / (1.01 max |Cpix|) (sf_set_grid), else the exact reduction.
Rows of same-sign coefficients -- Cpix is negative everywhere, so they add
up -- put every lane at 0.9 x, 1.2 x and 8 x that bound: phases of 2^15 ..
2^19 turns, where the rest of the suite stays below a few tens on the safe
path and reaches the exact one only with NaN / Inf rows.  Mixed groups check
the claim that both reductions give the same float.

Integer digits (kl_eval_int.h, from 12 k-steps): a slot is carried when
every rint(coef / 2 pi 2^44) fits 6 balanced base-256 digits, -8.031 ..
7.969 turns.  Rows within 0.07 turn inside both ends (the largest legal
digits in every K position) and rows with one coefficient just outside.

The reference is the phase in turns in extended precision, reduced modulo 1
turn and then through fp64 cos / sin (eval_cases.rev_reference); where long
double is no wider than double the fp64 oracle stands in, and the test ids
say so.  The CPU test pins the inputs; the others need an MI355X (``gpu``).
"""

import numpy as np
import pytest

import eval_cases as ec

REF_ID = "" if ec.LD_OK else "-fp64ref"
RANGE_GRIDS = (ec.GRIDS[1], ec.WAVE_GRID)


def _gpu():
    torch = pytest.importorskip("torch")
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    from ska_sdp_screen_fitting_amd import get_context
    dev = torch.device("cuda", 0)
    ctx = get_context(0)
    ctx.set_stream(torch.cuda.current_stream(dev).cuda_stream)
    return torch, dev, ctx


def bits(a):
    return a.view(np.int32)


def rev_max_rows(coef, cp):
    """[S] max |rev| (turns) of each row, fp64."""
    return np.abs(coef @ cp.T).max(axis=1) / (2.0 * np.pi)


# ----------------------------------------------------------------- CPU: inputs

def test_phase_range_inputs():
    """The rows the GPU tests run are where they are meant to be: lane sums
    on the intended side of the fixed-point bound, phases of 2^14.5 .. 2^21
    turns, a reference that is not the limit, and integer rows whose digits
    fit (inside) or leave a remainder (outside)."""
    from test_int_digits import digits
    for D in ec.FIXED_D:
        live = min(4, D)           # lane classes that hold a direction
        for ny, nx in RANGE_GRIDS:
            what = (D, ny, nx)
            cp = ec.cpix(D, ny, nx)
            assert np.all(cp < 0.0), what
            thr = ec.rev_threshold(cp)
            rows = ec.fixed_rows(D, ny, nx)
            assert rows.shape == (96, D) and np.all(rows[:48] > 0.0)
            f = ec.lane_sums(rows)[:, :live] / thr
            np.testing.assert_allclose(f[ec.group(ec.G_SAFE)], ec.F_SAFE, rtol=1e-12)
            np.testing.assert_allclose(f[ec.group(ec.G_EXACT)], ec.F_EXACT, rtol=1e-12)
            np.testing.assert_allclose(f[ec.group(ec.G_HUGE)], ec.F_HUGE, rtol=1e-12)
            for g in (ec.G_MIX_SAFE, ec.G_MIX_SMALL):
                m = f[ec.group(g)]
                assert np.all(m[:15] < 0.95) and np.all(m[15] > 1.15), what
            assert np.all(f[ec.group(ec.G_SMALL)] < 0.01), what
            # the mixed groups repeat rows that also sit in a safe group
            assert np.array_equal(rows[ec.group(ec.G_MIX_SAFE)][:15],
                                  rows[ec.group(ec.G_SAFE)][:15])
            assert np.array_equal(rows[ec.group(ec.G_MIX_SMALL)][:15],
                                  rows[ec.group(ec.G_SMALL)][:15])
            rm = rev_max_rows(rows, cp)
            floor = 14.5 if D == 1 else 15.5
            assert np.all(rm[ec.group(ec.G_SAFE)] >= 2.0 ** floor), what
            assert np.all(rm[ec.group(ec.G_HUGE)] >= 2.0 ** 17.5), what
            # the fixed-point read-out (rev_fixed: the low dword of
            # kRevMagic + rev as 2^-32 turns) restated: right on the safe
            # rows; past 2^19 turns the accumulator leaves [2^20, 2^21), so a
            # huge group wrongly sent down that path would be visibly wrong
            rev = rows[:48] @ cp.T / (2.0 * np.pi)
            lo = (1572864.0 + rev).view(np.int64) & 0xFFFFFFFF
            fixed = (((lo + 2 ** 31) % 2 ** 32) - 2 ** 31) * 2.0 ** -32
            d = fixed - (rev - np.rint(rev))
            d = np.abs(d - np.rint(d))
            assert d[ec.group(ec.G_SAFE)].max() < 1e-9, what
            if D > 1:
                assert rm[ec.group(ec.G_HUGE)].max() > 2.0 ** 19, what
                assert d[ec.group(ec.G_HUGE)].max() > 0.01, what
            frac, rmax = ec.rev_reference(rows, cp)
            assert rmax <= 2.0 ** 21, what
            assert ec.range_tolerance(D, rmax) - 2e-6 < 1e-7, what
            if ec.LD_OK:
                d = np.abs(ec.planes_f64(rows, cp) - ec.planes_from_frac(frac)).max()
                assert d <= 1e-8, (what, d)
    # the digit range's ends, derived: 127 / -128 in all six digits
    assert digits(127 * ec.M6) == ([127] * 6, 0)
    assert digits(-128 * ec.M6) == ([-128] * 6, 0)
    assert digits(127 * ec.M6 + 1)[1] != 0 and digits(-128 * ec.M6 - 1)[1] != 0
    for D in ec.INT_D:
        inside, outside = ec.int_rows(D)
        assert (inside > 0).any(axis=1).all() and (inside < 0).any(axis=1).all()
        for row in ec.fixed_point_turns(inside):
            assert all(digits(v)[1] == 0 for v in row), D
        for row in ec.fixed_point_turns(outside):
            assert sum(digits(v)[1] != 0 for v in row) == 1, D
        for ny, nx in RANGE_GRIDS:
            cp = ec.cpix(D, ny, nx)
            # sf_set_grid's range check of the pixel digits (with its 1 %)
            assert 1.01 * np.abs(cp).max() < 1.86 * 2.0 ** 10
            both = np.concatenate([inside, outside])
            frac, rmax = ec.rev_reference(both, cp)
            assert rmax <= 2.0 ** 21
            if ec.LD_OK:
                d = np.abs(ec.planes_f64(both, cp) - ec.planes_from_frac(frac)).max()
                assert d <= 1e-8, (D, ny, nx, d)


# ------------------------------------------------------------------------ GPU

def run_kernels(torch, dev, ctx, coef, ny, nx, flags, wg8=False):
    """{kernel value (or '8 waves'): cube} for every SF_OPT_EVAL_KERNEL value
    and AUTO on the bound grid."""
    from ska_sdp_screen_fitting_amd._lib import (
        EVAL_KERNEL_NAMES, SF_EVAL_KERNEL_AUTO, SF_EVAL_KERNEL_TILE,
        SF_OPT_EVAL_KERNEL, SF_OPT_EVAL_WG_WAVES)
    S = coef.shape[0]
    c = torch.from_numpy(np.ascontiguousarray(coef, np.float64)).to(dev)

    def run():
        out = torch.full((S, 4, ny, nx), -7.0, dtype=torch.float32, device=dev)
        ctx.eval(c, S, out, S, flags)
        torch.cuda.synchronize()
        return out.cpu().numpy()

    outs = {}
    try:
        for kv in sorted(EVAL_KERNEL_NAMES) + [SF_EVAL_KERNEL_AUTO]:
            ctx.set_option(SF_OPT_EVAL_KERNEL, kv)
            outs[kv] = run()
        if wg8:
            ctx.set_option(SF_OPT_EVAL_KERNEL, SF_EVAL_KERNEL_TILE)
            ctx.set_option(SF_OPT_EVAL_WG_WAVES, 8)
            outs["8 waves"] = run()
    finally:
        ctx.set_option(SF_OPT_EVAL_KERNEL, SF_EVAL_KERNEL_AUTO)
        ctx.set_option(SF_OPT_EVAL_WG_WAVES, 0)
    return outs


@pytest.mark.gpu
@pytest.mark.parametrize("grid", RANGE_GRIDS, ids=lambda g: f"{g[0]}x{g[1]}")
@pytest.mark.parametrize("D", ec.FIXED_D, ids=lambda D: f"D{D}{REF_ID}")
def test_fixed_point_boundary(D, grid):
    """Groups at 0.9 x (fixed point, at its edge), 1.2 x and 8 x (exact
    reduction of finite data) the fixed-point bound, and mixed groups: every
    kernel writes the same bits, every row matches the reference within
    2e-6 + 2 pi KS ulp(1.5 2^20 + max |rev|), and the 15 safe rows of a
    group sent down the exact path by its 16th row are bit-equal to the same
    rows in a safe group."""
    from ska_sdp_screen_fitting_amd._lib import (
        EVAL_KERNEL_NAMES, SF_EVAL_FAST_SINCOS, SF_EVAL_KERNEL_LDS4,
        SF_EVAL_KERNEL_LDS16, SF_EVAL_KERNEL_LDS16H, SF_EVAL_KERNEL_TILE,
        SF_EVAL_NAN_SCRUB)
    torch, dev, ctx = _gpu()
    ny, nx = grid
    x, y = ec.grid(D, ny, nx)
    ctx.set_piercepoints(ec.piercepoints(D)[0])
    ctx.set_grid(x, y)
    flags = SF_EVAL_NAN_SCRUB | SF_EVAL_FAST_SINCOS
    auto = {1: SF_EVAL_KERNEL_LDS16H, 7: SF_EVAL_KERNEL_LDS16H,
            20: SF_EVAL_KERNEL_LDS16, 40: SF_EVAL_KERNEL_LDS4}[D]
    assert ctx.eval_kernel(flags) == EVAL_KERNEL_NAMES[auto]
    rows = ec.fixed_rows(D, ny, nx)
    cp = ec.cpix(D, ny, nx)
    outs = run_kernels(torch, dev, ctx, rows, ny, nx, flags)
    got = outs[SF_EVAL_KERNEL_TILE]
    for kv, o in outs.items():
        assert np.array_equal(bits(o), bits(got)), kv
    frac, rmax = ec.rev_reference(rows, cp)
    rm = rev_max_rows(rows, cp)
    floor = 14.5 if D == 1 else 15.5
    assert np.all(rm[ec.group(ec.G_SAFE)] >= 2.0 ** floor)
    assert np.all(rm[ec.group(ec.G_HUGE)] >= 2.0 ** 17.5)
    assert rmax <= 2.0 ** 21
    tol = ec.range_tolerance(D, rmax)
    assert tol < 2.1e-6
    want = ec.planes_from_frac(frac)
    err = np.abs(got.reshape(want.shape) - want).max(axis=(1, 2))
    print(f"D={D} grid={grid}: max|err| per group",
          [float(err[ec.group(g)].max()) for g in range(6)], "tol", tol)
    assert np.all(err <= tol), (np.argmax(err), err.max(), tol)
    for mixed, alone in ((ec.G_MIX_SAFE, ec.G_SAFE), (ec.G_MIX_SMALL, ec.G_SMALL)):
        a = got[ec.group(mixed)][:15]
        b = got[ec.group(alone)][:15]
        assert np.array_equal(bits(a), bits(b)), (mixed, alone)


@pytest.mark.gpu
@pytest.mark.parametrize("D", ec.INT_D, ids=lambda D: f"D{D}{REF_ID}")
def test_integer_digit_boundary(D):
    """Rows at the ends of the digit range on every kernel family that takes
    the integer contraction: inside rows within 2e-6 + 2 pi 7.06e-9 (the
    documented digit error bound) of the reference and within 3e-7 of the
    fp64 contraction; rows with one coefficient outside bit-equal to the
    SF_OPT_EVAL_INT = 0 run, also next to inside rows in one group."""
    from ska_sdp_screen_fitting_amd._lib import (
        SF_EVAL_FAST_SINCOS, SF_EVAL_KERNEL_AUTO, SF_EVAL_KERNEL_TILE,
        SF_EVAL_NAN_SCRUB, SF_OPT_EVAL_INT, SF_OPT_EVAL_KERNEL)
    torch, dev, ctx = _gpu()
    inside, outside = ec.int_rows(D)
    n = ec.N_INT
    mixed = np.where((np.arange(n) % 2 == 0)[:, None], inside, outside)
    rows = np.concatenate([inside, outside, mixed])
    carried = np.concatenate([np.ones(n, bool), np.zeros(n, bool), np.arange(n) % 2 == 0])
    flags = SF_EVAL_NAN_SCRUB | SF_EVAL_FAST_SINCOS
    for ny, nx in RANGE_GRIDS:
        what = (D, ny, nx)
        x, y = ec.grid(D, ny, nx)
        ctx.set_piercepoints(ec.piercepoints(D)[0])
        ctx.set_grid(x, y)
        assert ctx.eval_contraction(flags) == "i8-digits", what
        outs = run_kernels(torch, dev, ctx, rows, ny, nx, flags, wg8=True)
        got = outs[SF_EVAL_KERNEL_TILE]
        for kv, o in outs.items():
            assert np.array_equal(bits(o), bits(got)), (what, kv)
        try:
            ctx.set_option(SF_OPT_EVAL_INT, 0)
            ctx.set_option(SF_OPT_EVAL_KERNEL, SF_EVAL_KERNEL_TILE)
            assert ctx.eval_contraction(flags) == "f64", what
            fp64c = run_kernels(torch, dev, ctx, rows, ny, nx, flags)[SF_EVAL_KERNEL_TILE]
        finally:
            ctx.set_option(SF_OPT_EVAL_INT, -1)
            ctx.set_option(SF_OPT_EVAL_KERNEL, SF_EVAL_KERNEL_AUTO)
        assert np.array_equal(bits(got[~carried]), bits(fp64c[~carried])), what
        d = np.abs(got[carried] - fp64c[carried]).max()
        assert d <= 3e-7, (what, d)
        # the integer path really ran on the carried rows
        assert not np.array_equal(bits(got[carried]), bits(fp64c[carried])), what
        cp = ec.cpix(D, ny, nx)
        frac, rmax = ec.rev_reference(rows, cp)
        assert rmax <= 2.0 ** 21
        want = ec.planes_from_frac(frac)
        err = np.abs(got.reshape(want.shape) - want).max(axis=(1, 2))
        print(f"D={D} grid={(ny, nx)}: max|err| carried", float(err[carried].max()),
              "fp64 rows", float(err[~carried].max()))
        assert np.all(err[carried] <= 2e-6 + 2.0 * np.pi * 7.06e-9), (what, err[carried].max())
        assert np.all(err[~carried] <= ec.range_tolerance(D, rmax)), (what, err[~carried].max())
