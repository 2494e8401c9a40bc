"""sf_kl_eval_pol (csrc/kl_eval_pol.hip): KL screens with polarized phases --
planes 0 / 1 from the XX phase (and amplitude) coefficients, planes 2 / 3 from
the YY ones, one kernel for 1..128 directions.

Expected values are composed from the oracle (fp64 numpy restatement of
calculate_kl_screen, kl_screen.py:411-449 and :367-380): planes 0 / 1 of a call
with the XX inputs, planes 2 / 3 of a call with the YY inputs.  Tolerances are
the project's evaluation tolerances: 2e-6 with SF_EVAL_FAST_SINCOS, 1e-6
without (tests/test_tec_jones.py), times max(1, A) with amplitudes
(tests/test_wide_eval.py).  Needs an MI355X: every test is marked ``gpu``.
"""

import numpy as np
import pytest

from conftest import load_golden
from oracle import kl as okl
from test_wide_eval import BE, FAST, NT, SCRUB, grid_for, phase_coef, up

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

TOL = {FAST: 2e-6, 0: 1e-6}
GRIDS = [(17, 17), (20, 18), (64, 64)]


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


def bind(ctx, n_dir, nx, ny, seed=None):
    """Geometry of n_dir directions and an nx x ny grid (the leading
    coordinates of the square grid of side max(nx, ny)); returns Cpix."""
    pp, x, y = grid_for(n_dir, max(nx, ny), seed=n_dir if seed is None else seed)
    x, y = x[:nx], y[:ny]
    ctx.set_piercepoints(pp)
    ctx.set_grid(x, y)
    return okl.cpix_matrix(pp, x, y)


def coefs(rng, S, n_dir, cpix, amps=True):
    """Independent XX / YY phase coefficients (test_wide_eval.phase_coef: some
    rows x 300, so both pols span many turns) and log10 amplitudes scaled to
    |log10 A| <= 1."""
    out = [phase_coef(rng, S, n_dir), phase_coef(rng, S, n_dir)]
    for _ in range(2 if amps else 0):
        a = rng.normal(0, 1.0, (S, n_dir))
        out.append(a / np.abs(a @ cpix.T).max())
    return out


def want_planes(px, py, cpix, ax=None, ay=None):
    """[S, 4, P] float64 and the largest amplitude."""
    if ax is None:
        wx = okl.eval_planes(okl.eval_phase_screens(px, cpix))
        wy = okl.eval_planes(okl.eval_phase_screens(py, cpix))
        amax = 1.0
    else:
        a_x = 10 ** okl.eval_phase_screens(ax, cpix)
        a_y = 10 ** okl.eval_phase_screens(ay, cpix)
        wx = okl.eval_planes(okl.eval_phase_screens(px, cpix), a_x, a_y)
        wy = okl.eval_planes(okl.eval_phase_screens(py, cpix), a_x, a_y)
        amax = max(1.0, a_x.max(), a_y.max())
    return np.concatenate([wx[:, 0:2], wy[:, 2:4]], axis=1), amax


def run_pol(ctx, dev, px, py, nx, ny, flags, ax=None, ay=None, ring=None, S=None):
    S = px.shape[0] if S is None else S
    n = S if ring is None else min(S, ring)
    out = torch.full((n, 4, ny, nx), -7.0, dtype=torch.float32, device=dev)
    ctx.eval_pol(up(dev, px), up(dev, py), S, out, ring_slots=ring,
                 amp_xx=None if ax is None else up(dev, ax),
                 amp_yy=None if ay is None else up(dev, ay), flags=flags)
    torch.cuda.synchronize()
    return out.cpu().numpy()


def bits(a):
    return np.ascontiguousarray(a).view(np.int32)


# 1: a lone direction; 7: the fixture; 20: five full k-steps; 61: one live
# direction in the last k-step and a padded trip; 65: the K = 64 boundary;
# 128: SF_MAX_EVAL_DIR.  17 x 17: odd pixel count (scalar stores); 20 x 18:
# non-square, partial 64-pixel block; 64 x 64: float4 stores, 64 blocks.
@pytest.mark.parametrize("nx,ny", GRIDS)
@pytest.mark.parametrize("n_dir", [1, 7, 20, 61, 65, 128])
def test_pol_vs_oracle(ctx, dev, n_dir, nx, ny):
    cpix = bind(ctx, n_dir, nx, ny)
    px, py, ax, ay = coefs(np.random.default_rng(1000 * nx + n_dir), 33, n_dir, cpix)
    for amps in ((None, None), (ax, ay)):
        want, amax = want_planes(px, py, cpix, *amps)
        for sinc in (FAST, 0):
            for S in (1, 19, 33):  # ragged 16-slot groups
                a = [None if v is None else v[:S] for v in amps]
                got = run_pol(ctx, dev, px[:S], py[:S], nx, ny, SCRUB | NT | sinc, *a)
                err = np.abs(got.reshape(S, 4, -1) - want[:S]).max()
                print(f"D={n_dir} {nx}x{ny} S={S} fast={bool(sinc)} "
                      f"amps={a[0] is not None} max|d|={err:.3g} A={amax:.3g}")
                assert err <= TOL[sinc] * amax


@pytest.mark.parametrize("n_dir", [7, 20, 61, 128])
def test_pol_symmetry_bit_for_bit(ctx, dev, n_dir):
    nx, ny, S = 20, 18, 19
    cpix = bind(ctx, n_dir, nx, ny)
    rng = np.random.default_rng(n_dir)
    px, py, ax, ay = coefs(rng, S, n_dir, cpix)
    qy, _, by, _ = coefs(rng, S, n_dir, cpix)  # another YY set
    for sinc in (FAST, 0):
        fl = SCRUB | sinc
        for amps, other in (((None, None), (None, None)), ((ax, ay), (ax, by))):
            ref = run_pol(ctx, dev, px, py, nx, ny, fl, *amps)
            # swapping the (xx, yy) inputs swaps the plane pairs
            sw = run_pol(ctx, dev, py, px, nx, ny, fl, *amps[::-1])
            assert np.array_equal(bits(sw[:, 2:4]), bits(ref[:, 0:2]))
            assert np.array_equal(bits(sw[:, 0:2]), bits(ref[:, 2:4]))
            # planes 0 / 1 do not depend on the YY inputs
            ch = run_pol(ctx, dev, px, qy, nx, ny, fl, *other)
            assert np.array_equal(bits(ch[:, 0:2]), bits(ref[:, 0:2]))
            assert not np.array_equal(bits(ch[:, 2:4]), bits(ref[:, 2:4]))
            # equal pols: the two plane pairs agree (amplitudes: equal too)
            same = run_pol(ctx, dev, px, px, nx, ny, fl, amps[0], amps[0])
            assert np.array_equal(bits(same[:, 0:2]), bits(same[:, 2:4]))
            assert np.array_equal(bits(same[:, 0:2]), bits(ref[:, 0:2]))
            if n_dir <= 60:
                continue
            # D > 60: sf_kl_eval / sf_kl_eval_gain run the wide kernel, which
            # shares the contraction order and the epilogue: the same cube
            out = torch.full((S, 4, ny, nx), -7.0, dtype=torch.float32, device=dev)
            if amps[0] is None:
                assert ctx.eval_kernel(fl) == "kl_eval_wide_kernel"
                ctx.eval(up(dev, px), S, out, flags=fl)
                eq = run_pol(ctx, dev, px, px, nx, ny, fl)
            else:
                assert ctx.eval_kernel(fl, gain=True) == "kl_eval_wide_kernel"
                ctx.eval_gain(up(dev, px), up(dev, ax), up(dev, ay), S, out, flags=fl)
                eq = run_pol(ctx, dev, px, px, nx, ny, fl, ax, ay)
            torch.cuda.synchronize()
            assert np.array_equal(bits(eq), bits(out.cpu().numpy()))


@pytest.mark.parametrize("nx,ny", [(17, 17), (20, 18)])
def test_pol_nan_stays_in_its_slot_and_pair(ctx, dev, nx, ny):
    n_dir, S, k = 61, 19, 7
    cpix = bind(ctx, n_dir, nx, ny)
    clean = coefs(np.random.default_rng(nx), S, n_dir, cpix)
    others = [s for s in range(S) if s != k]
    for sinc in (FAST, 0):
        ref = run_pol(ctx, dev, clean[0], clean[1], nx, ny, SCRUB | sinc, *clean[2:])
        ref2 = run_pol(ctx, dev, clean[0], clean[1], nx, ny, SCRUB | sinc)
        for which in range(4):  # phase XX, phase YY, amplitude XX, amplitude YY
            c = [a.copy() for a in clean]
            c[which][k, 33 % n_dir] = np.nan
            pair = slice(0, 2) if which % 2 == 0 else slice(2, 4)
            keep = slice(2, 4) if which % 2 == 0 else slice(0, 2)
            cases = [(c, ref)] if which >= 2 else [(c, ref), (c[:2] + [None, None], ref2)]
            for (a, b, ax, ay), clean_run in cases:
                raw = run_pol(ctx, dev, a, b, nx, ny, sinc, ax, ay)
                scr = run_pol(ctx, dev, a, b, nx, ny, SCRUB | sinc, ax, ay)
                assert np.isnan(raw[k, pair]).all()
                assert np.all(scr[k, pair][0] == 1.0) and np.all(scr[k, pair][1] == 0.0)
                for got in (raw, scr):
                    assert np.array_equal(bits(got[k, keep]), bits(clean_run[k, keep]))
                    assert np.array_equal(bits(got[others]), bits(clean_run[others]))


@pytest.mark.parametrize("nx,ny", [(20, 18), (16, 16)])
def test_pol_store_paths_ring_and_walk(ctx, dev, nx, ny):
    from ska_sdp_screen_fitting_amd._lib import (SF_OPT_EVAL_BANDS, SF_OPT_EVAL_GROUPS,
                                                 SF_OPT_EVAL_MAX_BLOCKS,
                                                 SF_OPT_EVAL_XCD_MAP)
    n_dir, S = 65, 37
    cpix = bind(ctx, n_dir, nx, ny)
    px, py, ax, ay = coefs(np.random.default_rng(nx + 1), S, n_dir, cpix)
    for amps in ((None, None), (ax, ay)):
        for sinc in (FAST, 0):
            base = SCRUB | sinc
            ref = run_pol(ctx, dev, px, py, nx, ny, base, *amps)
            want, amax = want_planes(px, py, cpix, *amps)
            assert np.abs(ref.reshape(S, 4, -1) - want).max() <= TOL[sinc] * amax
            nt = run_pol(ctx, dev, px, py, nx, ny, base | NT, *amps)
            assert np.array_equal(bits(nt), bits(ref))
            be = run_pol(ctx, dev, px, py, nx, ny, base | BE | NT, *amps)
            assert np.array_equal(bits(be.byteswap()), bits(ref))
            # an output that is not 16-byte aligned
            buf = torch.full((S * 4 * ny * nx + 2,), -7.0, dtype=torch.float32, device=dev)
            off = buf[1:-1]
            assert off.data_ptr() % 16 == 4
            ctx.eval_pol(up(dev, px), up(dev, py), S, off,
                         amp_xx=None if amps[0] is None else up(dev, ax),
                         amp_yy=None if amps[1] is None else up(dev, ay), flags=base | NT)
            torch.cuda.synchronize()
            assert float(buf[0]) == -7.0 and float(buf[-1]) == -7.0
            assert np.array_equal(bits(off.cpu().numpy().reshape(ref.shape)), bits(ref))
            # ring of 5: every entry holds its last slot
            rg = run_pol(ctx, dev, px, py, nx, ny, base, *amps, ring=5)
            for e in range(5):
                last = max(s for s in range(S) if s % 5 == e)
                assert np.array_equal(bits(rg[e]), bits(ref[last])), e
            # a ring longer than the call changes nothing
            lg = run_pol(ctx, dev, px, py, nx, ny, base, *amps, ring=S + 3)
            assert np.array_equal(bits(lg), bits(ref))
            # the work-item walk: few workgroups, one group per item, bands, XCD maps
            for opts in (((SF_OPT_EVAL_MAX_BLOCKS, 1),), ((SF_OPT_EVAL_GROUPS, 1),),
                         ((SF_OPT_EVAL_MAX_BLOCKS, 3), (SF_OPT_EVAL_GROUPS, 2)),
                         ((SF_OPT_EVAL_BANDS, 2), (SF_OPT_EVAL_XCD_MAP, 1)),
                         ((SF_OPT_EVAL_XCD_MAP, 0),)):
                for o, v in opts:
                    ctx.set_option(o, v)
                try:
                    wk = run_pol(ctx, dev, px, py, nx, ny, base, *amps)
                finally:
                    for o, _ in opts:
                        ctx.set_option(o, -1 if o == SF_OPT_EVAL_XCD_MAP else 0)
                assert np.array_equal(bits(wk), bits(ref)), opts
    # S = 0 writes nothing
    out = torch.full((1, 4, ny, nx), -7.0, dtype=torch.float32, device=dev)
    ctx.eval_pol(up(dev, px), up(dev, py), 0, out)
    torch.cuda.synchronize()
    assert bool((out == -7.0).all())


def test_pol_walk_on_many_blocks(ctx, dev):
    """64 x 64: 64 wave blocks, so the XCD map and the bands take effect."""
    from ska_sdp_screen_fitting_amd._lib import (SF_OPT_EVAL_BANDS, SF_OPT_EVAL_GROUPS,
                                                 SF_OPT_EVAL_MAX_BLOCKS,
                                                 SF_OPT_EVAL_XCD_MAP)
    n_dir, S, n = 20, 37, 64
    cpix = bind(ctx, n_dir, n, n)
    px, py, ax, ay = coefs(np.random.default_rng(5), S, n_dir, cpix)
    fl = SCRUB | FAST | NT
    ref = run_pol(ctx, dev, px, py, n, n, fl, ax, ay)
    for opts in (((SF_OPT_EVAL_MAX_BLOCKS, 8),), ((SF_OPT_EVAL_BANDS, 4),),
                 ((SF_OPT_EVAL_XCD_MAP, 1), (SF_OPT_EVAL_GROUPS, 1)),
                 ((SF_OPT_EVAL_XCD_MAP, 0), (SF_OPT_EVAL_BANDS, 2),
                  (SF_OPT_EVAL_MAX_BLOCKS, 16))):
        for o, v in opts:
            ctx.set_option(o, v)
        try:
            wk = run_pol(ctx, dev, px, py, n, n, fl, ax, ay)
        finally:
            for o, _ in opts:
                ctx.set_option(o, -1 if o == SF_OPT_EVAL_XCD_MAP else 0)
        assert np.array_equal(bits(wk), bits(ref)), opts


def test_pol_interleaved_with_eval(ctx, dev):
    """Calls interleaved with sf_kl_eval on one context, no sync between."""
    n_dir, S, nx, ny = 20, 19, 20, 18
    cpix = bind(ctx, n_dir, nx, ny)
    px, py, ax, ay = coefs(np.random.default_rng(9), S, n_dir, cpix)
    fl = SCRUB | FAST
    ref_pol = run_pol(ctx, dev, px, py, nx, ny, fl, ax, ay)
    ref_ph = torch.full((S, 4, ny, nx), -7.0, dtype=torch.float32, device=dev)
    ctx.eval(up(dev, py), S, ref_ph, flags=fl)
    torch.cuda.synchronize()
    d = [up(dev, a) for a in (px, py, ax, ay)]
    outs = [torch.full((S, 4, ny, nx), -7.0, dtype=torch.float32, device=dev)
            for _ in range(6)]
    for i in range(0, 6, 2):
        ctx.eval_pol(d[0], d[1], S, outs[i], amp_xx=d[2], amp_yy=d[3], flags=fl)
        ctx.eval(d[1], S, outs[i + 1], flags=fl)
    torch.cuda.synchronize()
    for i in range(0, 6, 2):
        assert np.array_equal(bits(outs[i].cpu().numpy()), bits(ref_pol))
        assert torch.equal(outs[i + 1], ref_ph)


def test_pol_contract(dev):
    from ska_sdp_screen_fitting_amd._lib import Context, ScreenFitError
    n_dir, S, nx, ny = 12, 3, 17, 17
    pp, x, y = grid_for(n_dir, 17, seed=5)
    c = Context(0)
    try:
        c.set_stream(torch.cuda.current_stream(dev).cuda_stream)
        c.set_piercepoints(pp)
        cpix = okl.cpix_matrix(pp, x, y)
        px, py, ax, ay = (up(dev, a) for a in
                          coefs(np.random.default_rng(1), S, n_dir, cpix))
        out = torch.full((S, 4, ny, nx), -7.0, dtype=torch.float32, device=dev)
        with pytest.raises(ScreenFitError, match="sf_set_grid"):  # no grid
            c.eval_pol(px, py, S, out)
        c.set_grid(x, y)
        bad = [dict(phase_yy=None),                      # a missing phase_yy
               dict(phase_xx=None),
               dict(amp_xx=ax), dict(amp_yy=ay),         # one amplitude pointer
               dict(flags=1 << 11), dict(flags=SCRUB | (1 << 30)),  # unknown bits
               dict(ring_slots=0), dict(ring_slots=-2)]
        for kw in bad:
            a = dict(phase_xx=px, phase_yy=py, amp_xx=None, amp_yy=None,
                     flags=SCRUB | FAST, ring_slots=S)
            a.update(kw)
            rc = c.lib.sf_kl_eval_pol(
                c.h, *(None if a[k] is None else a[k].data_ptr()
                       for k in ("phase_xx", "phase_yy", "amp_xx", "amp_yy")),
                S, out.data_ptr(), a["ring_slots"], a["flags"])
            assert rc == -22, kw  # SF_EINVAL
            assert c.lib.sf_last_error().decode().startswith("sf_kl_eval_pol"), kw
        torch.cuda.synchronize()
        assert bool((out == -7.0).all())
        # the context is still usable
        c.eval_pol(px, py, S, out, amp_xx=ax, amp_yy=ay, flags=SCRUB | FAST)
        torch.cuda.synchronize()
        want, amax = want_planes(*(t.cpu().numpy() for t in (px, py)), cpix,
                                 ax.cpu().numpy(), ay.cpu().numpy())
        assert np.abs(out.cpu().numpy().reshape(S, 4, -1) - want).max() <= 2e-6 * amax
    finally:
        c.close()


def test_pol_vs_reference_golden(ctx, dev):
    """The reference's per-pol coefficients and calculate_kl_screen planes
    (tests/golden/make_golden_pol.py), XX in planes 0 / 1, YY in 2 / 3."""
    g = load_golden("pol12")
    ctx.set_piercepoints(g["piercepoints"], float(g["r_0"]), float(g["beta"]))
    ctx.set_grid(g["x17"], g["y17"])
    for sinc in (FAST, 0):
        for k, (f, a) in enumerate(g["pairs17"]):
            cx, cy = g["coef"][:, f, a, :, 0], g["coef"][:, f, a, :, 1]
            got = run_pol(ctx, dev, cx, cy, 17, 17, sinc)
            assert np.abs(got - g["pol17"][k]).max() <= TOL[sinc]
            assert np.abs(got[:, 0:2] - got[:, 2:4]).max() > 1e-3  # the pols differ
