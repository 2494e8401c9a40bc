"""Every compile-time k-step count of the D <= 60 evaluation (kl_eval_impl.h,
kl_eval_launch.h, kl_eval_ks*.hip) on non-square grids.

launch_eval switches on KS = ceil(D / 4) into 15 separately compiled
launch_eval_pick<KS>, each with its own register tiles (direct addressing up
to 11 k-steps), gain tile, TILE3, five LDS-staged shapes, SHB tile and, from
12 k-steps, the integer-digit variants; the group-count and auto-kernel rules
branch on KS as well.  One test per KS and screen kind, each at
D = 4 KS - 3 (one live direction in the last k-step; D = 1 included) and
D = 4 KS (a full last k-step), on the three (ny, nx) grids of
eval_cases.GRIDS: nx != ny everywhere, so a swapped extent in the pixel basis
(kl_cpix_kernel), the pixel digits (kl_cdig_kernel) or the cmax scan of
sf_set_grid cannot hide as it does on a square grid.

Geometry is bound with set_piercepoints (no eigen-basis: D = 1 is a pure
evaluation case).  The reference is the fp64 oracle (oracle/kl.py) with the
project's own tolerances: 1e-6 with fp64 sincos, 2e-6 with the fast epilogue.
Needs an MI355X: every test is marked ``gpu``.
"""

import numpy as np
import pytest

import eval_cases as ec

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

KS_ALL = range(1, 16)


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    return torch.device("cuda", 0)


@pytest.fixture(scope="module")
def ctx(dev):
    from ska_sdp_screen_fitting_amd import get_context
    c = get_context(0)
    c.set_stream(torch.cuda.current_stream(dev).cuda_stream)
    return c


def bits(a):
    return a.view(np.int32)


def upload(dev, a):
    return torch.from_numpy(np.ascontiguousarray(a, np.float64)).to(dev)


def bind(ctx, D, ny, nx, swap=False):
    """set_piercepoints + set_grid of a case -> (ny, nx) of the bound grid."""
    x, y = ec.grid(D, ny, nx)
    if swap:
        x, y = y, x
    ctx.set_piercepoints(ec.piercepoints(D)[0])
    ctx.set_grid(x, y)
    return len(y), len(x)


def auto_kernel(ks, float4):
    """pick_eval_kernel's rule for phase screens on the fast epilogue."""
    from ska_sdp_screen_fitting_amd import _lib
    if not float4 or ks >= 12:
        return _lib.SF_EVAL_KERNEL_TILE
    if ks <= 3:
        return _lib.SF_EVAL_KERNEL_LDS16H
    return _lib.SF_EVAL_KERNEL_LDS16 if ks <= 8 else _lib.SF_EVAL_KERNEL_LDS4


def check_phase(ctx, dev, D, ny, nx, swap=False):
    """The phase checks of one (D, grid); returns the register tile's cube."""
    from ska_sdp_screen_fitting_amd._lib import (
        EVAL_KERNEL_NAMES, SF_EVAL_FAST_SINCOS, SF_EVAL_KERNEL_AUTO,
        SF_EVAL_KERNEL_LDS4, SF_EVAL_KERNEL_TILE, SF_EVAL_KERNEL_TILE3,
        SF_EVAL_KERNEL_WIDE, SF_EVAL_NAN_SCRUB, SF_OPT_EVAL_INT,
        SF_OPT_EVAL_KERNEL, SF_OPT_EVAL_KS_PAD, SF_OPT_EVAL_WG_WAVES)
    what = f"D={D} grid={(ny, nx)}{' swapped' if swap else ''}"
    ks = ec.ksteps(D)
    gy, gx = bind(ctx, D, ny, nx, swap)
    float4 = (gy * gx) % 4 == 0
    coef = ec.sweep_rows(D)
    S = coef.shape[0]
    c = upload(dev, coef)
    fast = SF_EVAL_NAN_SCRUB | SF_EVAL_FAST_SINCOS

    def run(flags):
        out = torch.full((S, 4, gy, gx), -7.0, dtype=torch.float32, device=dev)
        ctx.eval(c, S, out, S, flags)
        torch.cuda.synchronize()
        return out.cpu().numpy()

    outs = {}
    try:
        for kv in sorted(EVAL_KERNEL_NAMES) + [SF_EVAL_KERNEL_AUTO]:
            ctx.set_option(SF_OPT_EVAL_KERNEL, kv)
            # the kernel the sweep means to run is the one that runs: every
            # forced shape on a float4 grid, the register tile on an odd one
            want = kv
            if kv in (SF_EVAL_KERNEL_AUTO, SF_EVAL_KERNEL_WIDE):
                want = auto_kernel(ks, float4)
            elif not float4 and kv != SF_EVAL_KERNEL_TILE3:
                want = SF_EVAL_KERNEL_TILE
            assert ctx.eval_kernel(fast) == EVAL_KERNEL_NAMES[want], (what, kv)
            if ks >= 12 and float4:
                assert ctx.eval_contraction(fast) == "i8-digits", (what, kv)
            outs[kv] = run(fast)
        ctx.set_option(SF_OPT_EVAL_KERNEL, SF_EVAL_KERNEL_TILE)
        if ks >= 12:
            # the integer register tile with 8-wave workgroups, and the fp64
            # contraction of the same D
            ctx.set_option(SF_OPT_EVAL_WG_WAVES, 8)
            outs["8 waves"] = run(fast)
            ctx.set_option(SF_OPT_EVAL_WG_WAVES, 0)
            ctx.set_option(SF_OPT_EVAL_INT, 0)
            assert ctx.eval_contraction(fast) == "f64", what
            fp64c = run(fast)
            ctx.set_option(SF_OPT_EVAL_INT, -1)
        if (ny, nx) == ec.GRIDS[0] and ks + 1 <= 15:
            # one zero k-step: launch_eval_pick<KS + 1> on the real KS
            ctx.set_option(SF_OPT_EVAL_KERNEL, SF_EVAL_KERNEL_LDS4)
            ctx.set_option(SF_OPT_EVAL_KS_PAD, 1)
            outs["pad"] = run(fast)
            ctx.set_option(SF_OPT_EVAL_KS_PAD, 0)
            ctx.set_option(SF_OPT_EVAL_KERNEL, SF_EVAL_KERNEL_TILE)
        # fp64 sincos: the BEM 2 register tile
        precise = run(SF_EVAL_NAN_SCRUB)
        raw_precise = run(0)
        ctx.set_option(SF_OPT_EVAL_KERNEL, SF_EVAL_KERNEL_AUTO)
        raw_fast = run(SF_EVAL_FAST_SINCOS)
    finally:
        ctx.set_option(SF_OPT_EVAL_KERNEL, SF_EVAL_KERNEL_AUTO)
        ctx.set_option(SF_OPT_EVAL_WG_WAVES, 0)
        ctx.set_option(SF_OPT_EVAL_INT, -1)
        ctx.set_option(SF_OPT_EVAL_KS_PAD, 0)
    ref = outs[SF_EVAL_KERNEL_TILE]
    for k, o in outs.items():
        assert np.array_equal(bits(o), bits(ref)), (what, k)
    if ks >= 12:
        err = np.abs(ref - fp64c).max()
        assert err <= 3e-7, (what, "int vs fp64 contraction", err)
    ok = ec.finite_rows(coef)
    want = ec.planes_f64(coef[ok], ec.cpix(D, ny, nx, swap))
    for name, o, tol in (("fast", ref, 2e-6), ("fp64 sincos", precise, 1e-6)):
        err = np.abs(o[ok].reshape(want.shape) - want).max()
        assert err <= tol, (what, name, err)
        # scrubbed NaN / Inf rows: exactly cos 1, sin 0
        for s in (ec.NAN_ROW, ec.INF_ROW):
            assert np.all(o[s, 0::2] == 1.0) and np.all(o[s, 1::2] == 0.0), (what, name, s)
        assert np.array_equal(bits(o[:, 2:4]), bits(o[:, 0:2])), (what, name, "planes")
    # unscrubbed: NaN in every plane of those rows, the rest unchanged
    for name, raw, o in (("fast", raw_fast, ref), ("fp64 sincos", raw_precise, precise)):
        assert np.isnan(raw[[ec.NAN_ROW, ec.INF_ROW]]).all(), (what, name)
        assert np.array_equal(bits(raw[ok]), bits(o[ok])), (what, name, "unscrubbed")
    return ref


@pytest.mark.parametrize("ks", KS_ALL, ids=lambda k: f"ks{k}")
def test_phase_ksteps(ctx, dev, ks):
    """Phase screens at D = 4 KS - 3 and 4 KS on the three grids: every
    SF_OPT_EVAL_KERNEL value (and AUTO) writes the register tile's bits; from
    12 k-steps so do 8-wave workgroups, and the fp64 contraction is within
    3e-7 (test_eval_int.py's bound); one zero k-step of padding on an
    LDS-staged shape changes nothing; the fast and the fp64-sincos cubes
    match the oracle; NaN / Inf rows are 1 / 0 scrubbed and NaN unscrubbed;
    planes 2 / 3 repeat planes 0 / 1."""
    for D in (4 * ks - 3, 4 * ks):
        for ny, nx in ec.GRIDS:
            check_phase(ctx, dev, D, ny, nx)


@pytest.mark.parametrize("ks", [5, 13], ids=lambda k: f"ks{k}")
def test_phase_transposed_grid(ctx, dev, ks):
    """The (40, 56) grid and its transpose (56, 40) with x and y exchanged
    both pass the phase checks, and the second cube is not the first one
    transposed: the two orientations really differ on this geometry, so a
    kernel that exchanged the extents would fail one of them."""
    ny, nx = ec.GRIDS[0]
    for D in (4 * ks - 3, 4 * ks):
        a = check_phase(ctx, dev, D, ny, nx)
        b = check_phase(ctx, dev, D, ny, nx, swap=True)
        assert b.shape == (ec.S_SWEEP, 4, nx, ny)
        ok = ec.finite_rows(ec.sweep_rows(D))
        assert np.abs(b[ok] - a[ok].transpose(0, 1, 3, 2)).max() > 0.1, D
        assert np.abs(b[ok].reshape(a[ok].shape) - a[ok]).max() > 0.1, D


@pytest.mark.parametrize("ks", KS_ALL, ids=lambda k: f"ks{k}")
def test_gain_ksteps(ctx, dev, ks):
    """Gain screens at D = 4 KS - 1 on (18, 20) and (40, 56): every
    SF_OPT_EVAL_KERNEL value writes the register tile's bits, and the tile
    is within 2e-6 + 1.2e-7 |log2 A| (relative to max(1, A)) of fp64 numpy,
    the tolerance of test_gain.py::test_gain_eval_kernels_agree."""
    from ska_sdp_screen_fitting_amd._lib import (
        EVAL_KERNEL_NAMES, SF_EVAL_FAST_SINCOS, SF_EVAL_KERNEL_AUTO,
        SF_EVAL_KERNEL_TILE, SF_EVAL_NAN_SCRUB, SF_OPT_EVAL_KERNEL)
    D = 4 * ks - 1
    flags = SF_EVAL_NAN_SCRUB | SF_EVAL_FAST_SINCOS
    for ny, nx in (ec.GRIDS[1], ec.GRIDS[0]):
        what = f"D={D} grid={(ny, nx)}"
        bind(ctx, D, ny, nx)
        ph, ax, ay = ec.gain_rows(D, ny, nx)
        S = ph.shape[0]
        up = [upload(dev, a) for a in (ph, ax, ay)]
        outs = {}
        try:
            for kv in sorted(EVAL_KERNEL_NAMES) + [SF_EVAL_KERNEL_AUTO]:
                ctx.set_option(SF_OPT_EVAL_KERNEL, kv)
                out = torch.full((S, 4, ny, nx), -7.0, dtype=torch.float32, device=dev)
                ctx.eval_gain(up[0], up[1], up[2], S, out, S, flags)
                torch.cuda.synchronize()
                outs[kv] = out.cpu().numpy()
        finally:
            ctx.set_option(SF_OPT_EVAL_KERNEL, SF_EVAL_KERNEL_AUTO)
        ref = outs[SF_EVAL_KERNEL_TILE]
        for kv, o in outs.items():
            assert np.array_equal(bits(o), bits(ref)), (what, kv)
        # scrubbed products: a NaN phase -> all four planes, NaN log A_XX ->
        # the XX planes
        for s in (ec.NAN_ROW, ec.INF_ROW):
            assert np.all(ref[s, 0::2] == 1.0) and np.all(ref[s, 1::2] == 0.0), (what, s)
        assert np.all(ref[12, 0] == 1.0) and np.all(ref[12, 1] == 0.0), what
        good = ec.finite_rows(ph) & ec.finite_rows(ax) & ec.finite_rows(ay)
        cp = ec.cpix(D, ny, nx)
        L = np.log2(10.0)
        phase = ph[good] @ cp.T
        lx, ly = ax[good] @ cp.T * L, ay[good] @ cp.T * L
        want = np.stack([2 ** lx * np.cos(phase), 2 ** lx * np.sin(phase),
                         2 ** ly * np.cos(phase), 2 ** ly * np.sin(phase)], 1)
        ampl = np.maximum(1.0, np.stack([2 ** lx, 2 ** lx, 2 ** ly, 2 ** ly], 1))
        lmax = np.maximum(np.abs(lx), np.abs(ly))[:, None, :]
        err = np.abs(ref[good].reshape(want.shape) - want) / ampl
        assert np.all(err <= 2e-6 + 1.2e-7 * lmax), (what, err.max())


@pytest.mark.parametrize("ks", KS_ALL, ids=lambda k: f"ks{k}")
def test_sums_ksteps(ctx, dev, ks):
    """sf_kl_eval_sums at D = 4 KS - 1 on (18, 20): each slot's checksum is
    the word sum mod 2^32 of the cube the same call wrote."""
    from ska_sdp_screen_fitting_amd._lib import (
        SF_EVAL_FAST_SINCOS, SF_EVAL_NAN_SCRUB, SF_EVAL_NT_STORES)
    from test_slot_sums import host_sums
    D = 4 * ks - 1
    ny, nx = ec.GRIDS[1]
    bind(ctx, D, ny, nx)
    coef = ec.sweep_rows(D)
    S = coef.shape[0]
    out = torch.full((S, 4, ny, nx), -7.0, dtype=torch.float32, device=dev)
    sums = torch.zeros(S, dtype=torch.int32, device=dev)
    ctx.eval_sums(upload(dev, coef), S, out, sums, S,
                  flags=SF_EVAL_NAN_SCRUB | SF_EVAL_FAST_SINCOS | SF_EVAL_NT_STORES)
    torch.cuda.synchronize()
    o = out.cpu().numpy()
    np.testing.assert_array_equal(sums.cpu().numpy().view(np.uint32), host_sums(o))
    # (the cube is a real one: the oracle's, as in test_phase_ksteps)
    ok = ec.finite_rows(coef)
    want = ec.planes_f64(coef[ok], ec.cpix(D, ny, nx))
    assert np.abs(o[ok].reshape(want.shape) - want).max() <= 2e-6
