"""KL evaluation with 61..128 directions: sf_set_piercepoints (the
evaluation-only geometry, SF_MAX_EVAL_DIR = 128) and the wide kernel of
csrc/kl_eval_wide.hip (run-time k-loop, Cpix of a 64-pixel block in LDS, fp64
MFMA contraction; kl_screen.py:411-449 contraction, :367-380 epilogue).

Checked against the oracle (fp64 numpy restatement of calculate_kl_screen) at
the tolerance of every evaluation test (atol 2e-6; gain: 2e-6 max(1, A)),
against the reference's own planes at D = 80 (tests/golden/wide80.npz), and
for D <= 60 bit for bit against the sf_set_basis route.
Needs an MI355X: every test is marked ``gpu``.
"""

import numpy as np
import pytest

from conftest import FIELD, load_golden
from oracle import kl as okl

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

FAST = 1 << 8   # SF_EVAL_FAST_SINCOS
SCRUB = 1       # SF_EVAL_NAN_SCRUB
NT = 1 << 9     # SF_EVAL_NT_STORES
BE = 1 << 10    # SF_EVAL_BIG_ENDIAN
WIDE = "kl_eval_wide_kernel"


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


def grid_for(n_dir, grid, seed):
    from ska_sdp_screen_fitting_amd import geometry
    from ska_sdp_screen_fitting_amd.synthetic import make_solutions
    s = make_solutions(n_ant=2, n_time=2, n_freq=1, n_dir=n_dir, seed=seed)
    pp, mra, mdec = geometry.piercepoints(s.dir_radec)
    cell = FIELD["width"] / (grid - 0.5)
    x, y = geometry.grid_coords(FIELD["rad"], FIELD["dec"], FIELD["width"],
                                cell, mra, mdec)
    assert len(x) == grid
    return pp, x, y


def up(dev, a):
    return torch.from_numpy(np.ascontiguousarray(a, np.float64)).to(dev)


def phase_coef(rng, S, n_dir):
    """As tests/test_eval_int.py: small coefficients, some rows x 300 so the
    phases span many turns (the exact reduction)."""
    coef = rng.normal(0, 0.01, size=(S, n_dir))
    coef[5:12] *= 300.0
    return coef


def run_phase(ctx, dev, coef, nx, ny, flags, ring=None, S=None):
    S = coef.shape[0] if S is None else S
    n = S if ring is None else min(S, ring)
    out = torch.full((n, 4, ny, nx), -7.0, dtype=torch.float32, device=dev)
    ctx.eval(up(dev, coef), S, out, ring_slots=ring, flags=flags)
    torch.cuda.synchronize()
    return out.cpu().numpy()


def run_gain(ctx, dev, ph, ax, ay, nx, ny, flags):
    S = ph.shape[0]
    out = torch.full((S, 4, ny, nx), -7.0, dtype=torch.float32, device=dev)
    ctx.eval_gain(up(dev, ph), up(dev, ax), up(dev, ay), S, out, flags=flags)
    torch.cuda.synchronize()
    return out.cpu().numpy()


def gain_coef(rng, S, n_dir, cpix):
    """Phase as phase_coef; log10 amplitudes scaled to |log10 A| <= 1."""
    ph = phase_coef(rng, S, n_dir)
    ax = rng.normal(0, 1.0, (S, n_dir))
    ay = rng.normal(0, 1.0, (S, n_dir))
    ax /= np.abs(ax @ cpix.T).max()
    ay /= np.abs(ay @ cpix.T).max()
    return ph, ax, ay


def gain_want(ph, ax, ay, cpix):
    phase = okl.eval_phase_screens(ph, cpix)
    a_x = 10 ** okl.eval_phase_screens(ax, cpix)
    a_y = 10 ** okl.eval_phase_screens(ay, cpix)
    return okl.eval_planes(phase, a_x, a_y), max(1.0, a_x.max(), a_y.max())


# 61 / 65: one live direction in the last k-step; 127: three; 64 | 65: the
# K = 64 boundary; 128: SF_MAX_EVAL_DIR.  17^2: odd pixel count (scalar
# stores); 64^2: float4 stores, 64 wave blocks.
@pytest.mark.parametrize("grid", [17, 64])
@pytest.mark.parametrize("n_dir", [61, 64, 65, 80, 127, 128])
def test_wide_phase_vs_oracle(ctx, dev, n_dir, grid):
    pp, x, y = grid_for(n_dir, grid, seed=n_dir)
    ctx.set_piercepoints(pp)
    ctx.set_grid(x, y)
    cpix = okl.cpix_matrix(pp, x, y)
    coef = phase_coef(np.random.default_rng(grid + n_dir), 33, n_dir)
    want = okl.eval_planes(okl.eval_phase_screens(coef, cpix))
    for flags in (SCRUB | FAST | NT, SCRUB | NT):
        assert ctx.eval_kernel(flags) == WIDE
        assert ctx.eval_contraction(flags) == "f64"
        for S in (1, 19, 33):  # ragged 16-slot groups
            got = run_phase(ctx, dev, coef[:S], grid, grid, flags)
            err = np.abs(got.reshape(S, 4, -1) - want[:S]).max()
            print(f"D={n_dir} grid={grid} S={S} flags={flags:#x} max|d|={err:.3g}")
            assert err <= 2e-6


def test_wide_phase_vs_reference_golden(ctx, dev):
    """The reference's own coefficients and KLScreen.make_matrix planes at
    D = 80 (tests/golden/make_golden_wide.py)."""
    g = load_golden("wide80")
    ctx.set_piercepoints(g["piercepoints"], float(g["r_0"]), float(g["beta"]))
    ctx.set_grid(g["x17"], g["y17"])
    for flags in (FAST, 0):
        assert ctx.eval_kernel(flags) == WIDE
        for k, (f, a) in enumerate(g["pairs17"]):
            coef = g["coef"][:, f, a, :]
            got = run_phase(ctx, dev, coef, 17, 17, flags)
            ref = g["kl17"][k]                    # [T][2][17][17]
            for p in range(4):
                assert np.abs(got[:, p] - ref[:, p % 2]).max() <= 2e-6


@pytest.mark.parametrize("grid", [17, 64])
@pytest.mark.parametrize("n_dir", [80, 128])
def test_wide_gain_vs_oracle(ctx, dev, n_dir, grid):
    pp, x, y = grid_for(n_dir, grid, seed=n_dir + 1)
    ctx.set_piercepoints(pp)
    ctx.set_grid(x, y)
    cpix = okl.cpix_matrix(pp, x, y)
    S = 19
    ph, ax, ay = gain_coef(np.random.default_rng(3 * grid + n_dir), S, n_dir, cpix)
    want, amax = gain_want(ph, ax, ay, cpix)
    for flags in (SCRUB | FAST | NT, SCRUB):
        assert ctx.eval_kernel(flags, gain=True) == WIDE
        assert ctx.eval_contraction(flags, gain=True) == "f64"
        got = run_gain(ctx, dev, ph, ax, ay, grid, grid, flags)
        err = np.abs(got.reshape(S, 4, -1) - want).max()
        print(f"gain D={n_dir} grid={grid} flags={flags:#x} max|d|={err:.3g} A={amax:.3g}")
        assert err <= 2e-6 * amax


@pytest.mark.parametrize("grid", [17, 64])
def test_wide_flags_and_rings(ctx, dev, grid):
    from ska_sdp_screen_fitting_amd._lib import SF_OPT_EVAL_MAX_BLOCKS
    n_dir, S = 80, 19
    pp, x, y = grid_for(n_dir, grid, seed=5)
    ctx.set_piercepoints(pp)
    ctx.set_grid(x, y)
    cpix = okl.cpix_matrix(pp, x, y)
    coef = phase_coef(np.random.default_rng(grid), S, n_dir)
    coef[7, 33] = np.nan
    ok = np.isfinite(coef).all(axis=1)
    want = okl.eval_planes(okl.eval_phase_screens(coef[ok], cpix))
    for sinc in (FAST, 0):
        base = sinc | SCRUB
        ref = run_phase(ctx, dev, coef, grid, grid, base)
        # NaN coefficient: scrubbed to (1, 0, 1, 0), or NaN without the scrub
        assert np.all(ref[7, 0::2] == 1.0) and np.all(ref[7, 1::2] == 0.0)
        raw = run_phase(ctx, dev, coef, grid, grid, sinc)
        assert np.isnan(raw[7]).all()
        assert np.array_equal(raw[ok].view(np.int32), ref[ok].view(np.int32))
        assert np.abs(ref[ok].reshape(want.shape) - want).max() <= 2e-6
        # big-endian output is the byte-swapped native output
        be = run_phase(ctx, dev, coef, grid, grid, base | BE)
        assert np.array_equal(be.byteswap().view(np.int32), ref.view(np.int32))
        # non-temporal stores
        nt = run_phase(ctx, dev, coef, grid, grid, base | NT)
        assert np.array_equal(nt.view(np.int32), ref.view(np.int32))
        # ring of 5: every entry holds its last writer
        rg = run_phase(ctx, dev, coef, grid, grid, base, ring=5)
        for e in range(5):
            last = max(s for s in range(S) if s % 5 == e)
            assert np.array_equal(rg[e].view(np.int32), ref[last].view(np.int32)), e
        # workgroups walking several work items
        ctx.set_option(SF_OPT_EVAL_MAX_BLOCKS, 1)
        try:
            wk = run_phase(ctx, dev, coef, grid, grid, base)
        finally:
            ctx.set_option(SF_OPT_EVAL_MAX_BLOCKS, 0)
        assert np.array_equal(wk.view(np.int32), ref.view(np.int32))
        # an output that is not 16-byte aligned
        buf = torch.full((S * 4 * grid * grid + 1,), -7.0, dtype=torch.float32,
                         device=dev)
        off = buf[1:]
        assert off.data_ptr() % 16 == 4
        ctx.eval(up(dev, coef), S, off, flags=base)
        torch.cuda.synchronize()
        assert float(buf[0]) == -7.0
        un = off.cpu().numpy().reshape(ref.shape)
        assert np.array_equal(un.view(np.int32), ref.view(np.int32))
    # S = 0 writes nothing
    out = torch.full((1, 4, grid, grid), -7.0, dtype=torch.float32, device=dev)
    ctx.eval(up(dev, coef), 0, out)
    torch.cuda.synchronize()
    assert bool((out == -7.0).all())


@pytest.mark.parametrize("grid", [17, 64])
def test_wide_eval_sums(ctx, dev, grid):
    n_dir, S = 80, 33
    pp, x, y = grid_for(n_dir, grid, seed=6)
    ctx.set_piercepoints(pp)
    ctx.set_grid(x, y)
    cpix = okl.cpix_matrix(pp, x, y)
    ph, ax, ay = gain_coef(np.random.default_rng(grid + 1), S, n_dir, cpix)
    flags = SCRUB | FAST | NT
    for gain in (False, True):
        if gain:
            ref = run_gain(ctx, dev, ph, ax, ay, grid, grid, flags)
        else:
            ref = run_phase(ctx, dev, ph, grid, grid, flags)
        want = ref.reshape(S, -1).view(np.uint32).astype(np.uint64).sum(1) % 2 ** 32
        out = torch.full((S, 4, grid, grid), -7.0, dtype=torch.float32, device=dev)
        cs = torch.zeros(S, dtype=torch.int32, device=dev)
        ctx.eval_sums(up(dev, ph), S, out, cs, S,
                      coef_xx=up(dev, ax) if gain else None,
                      coef_yy=up(dev, ay) if gain else None, flags=flags)
        torch.cuda.synchronize()
        assert np.array_equal(out.cpu().numpy().view(np.int32), ref.view(np.int32))
        assert np.array_equal(cs.cpu().numpy().view(np.uint32), want.astype(np.uint32))


@pytest.mark.parametrize("n_dir", [20, 50, 60])
def test_piercepoints_route_unchanged_below_limit(ctx, dev, n_dir):
    """D <= SF_MAX_DIR: set_piercepoints -> set_grid -> eval writes the bytes
    of the set_basis route, on the same kernel with the same contraction."""
    grid, S = 64, 19
    pp, x, y = grid_for(n_dir, grid, seed=n_dir)
    cpix = okl.cpix_matrix(pp, x, y)
    ph, ax, ay = gain_coef(np.random.default_rng(n_dir), S, n_dir, cpix)
    flags = SCRUB | FAST | NT
    res = []
    for setter in (ctx.set_basis, ctx.set_piercepoints):
        setter(pp)
        ctx.set_grid(x, y)
        res.append((ctx.eval_kernel(flags), ctx.eval_contraction(flags),
                    ctx.eval_kernel(flags, gain=True),
                    run_phase(ctx, dev, ph, grid, grid, flags),
                    run_phase(ctx, dev, ph, grid, grid, SCRUB),
                    run_gain(ctx, dev, ph, ax, ay, grid, grid, flags)))
    assert res[0][:3] == res[1][:3]
    assert res[0][0] != WIDE
    for a, b in zip(res[0][3:], res[1][3:]):
        assert np.array_equal(a.view(np.int32), b.view(np.int32))


def test_wide_boundaries(ctx, dev):
    from ska_sdp_screen_fitting_amd._lib import (SF_MAX_DIR, SF_MAX_EVAL_DIR,
                                                 ScreenFitError)
    from ska_sdp_screen_fitting_amd.synthetic import make_solutions
    from ska_sdp_screen_fitting_amd import geometry
    from ska_sdp_screen_fitting_amd.stationscreen import station_orders
    pp, x, y = grid_for(12, 17, seed=5)
    ctx.set_piercepoints(pp)
    ctx.set_grid(x, y)
    big = np.random.default_rng(0).normal(0, 50.0, (SF_MAX_EVAL_DIR + 1, 3))
    with pytest.raises(ScreenFitError):
        ctx.set_piercepoints(big)
    with pytest.raises(ScreenFitError):
        ctx.set_basis(big[:SF_MAX_DIR + 1])
    # the context is still usable
    ctx.set_piercepoints(pp)
    ctx.set_grid(x, y)
    coef = phase_coef(np.random.default_rng(1), 3, 12)
    want = okl.eval_planes(okl.eval_phase_screens(coef, okl.cpix_matrix(pp, x, y)))
    got = run_phase(ctx, dev, coef, 17, 17, SCRUB | FAST)
    assert np.abs(got.reshape(want.shape) - want).max() <= 2e-6
    # no eigen-basis on a piercepoints-only context
    sol = make_solutions(n_ant=3, n_time=2, n_freq=1, n_dir=12, seed=5)
    T, F, A, D = sol.val.shape
    pp12, _, _ = geometry.piercepoints(sol.dir_radec)
    ref = okl.reference_station(sol.weight)
    st = station_orders(sol.ant_pos, ref, 11)
    phd = torch.from_numpy(sol.val).to(dev)
    wtd = torch.from_numpy(sol.weight).to(dev)
    cfd = torch.empty_like(phd)
    ctx.set_piercepoints(pp12)
    with pytest.raises(ScreenFitError, match="sf_set_basis"):
        ctx.fit(phd, wtd, T, F, A, st, ref_ant=ref, coef=cfd)
    with pytest.raises(ScreenFitError, match="sf_set_basis"):
        ctx.get_basis()
    # sf_set_basis makes it a full context again
    ctx.set_basis(pp12)
    ctx.fit(phd, wtd, T, F, A, st, ref_ant=ref, coef=cfd)
    torch.cuda.synchronize()
    want_fit = okl.run_phase(sol.val, sol.weight, sol.ant_pos, pp12, ref, 11)
    assert np.abs(cfd.cpu().numpy() - want_fit["coef"]).max() < 1e-6
    ctx.get_basis()


def test_kl_evaluator_80_directions(dev):
    from ska_sdp_screen_fitting_amd.kl_screen import KLEvaluator
    pp, x, y = grid_for(80, 17, seed=80)
    ev = KLEvaluator(pp, 100.0, 5.0 / 3.0, x, y)
    coef = phase_coef(np.random.default_rng(80), 2 * 3 * 4, 80).reshape(2, 3, 4, 80)
    got = ev.eval_host(coef)
    assert got.shape == (2, 3, 4, 4, 17, 17)
    want = okl.eval_planes(okl.eval_phase_screens(coef.reshape(-1, 80),
                                                  okl.cpix_matrix(pp, x, y)))
    assert np.abs(got.reshape(want.shape) - want).max() <= 2e-6
    ev.ctx.close()
