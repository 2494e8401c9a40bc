"""Screen value cubes on the pixel grid (sf_kl_eval_values, csrc/kl_values.hip)
and the dTEC a-term products built on them (KLEvaluator.values_*,
KLTecScreen, make_tec_aterm_image).

Reference: fp64 numpy, ``oracle.kl.cpix_matrix`` + ``eval_phase_screens``.

Tolerance per element:  |out - v| <= 2^-24 |v| + C_SUM * sum_d |Cpix coef|.
The first term is the round-to-nearest of the one fp32 cast (Q12).  The second
covers the fp64 summation order of the MFMA contraction and the device pow in
Cpix.  C_SUM is measured, not guessed: M is the largest
|sf_kl_eval_point_values - numpy| / sum_d |Cpix coef| over the shapes of this
module (every D and grid of ``test_shapes``, the grid positions bound as
points) -- existing fp64 code, not the code under test -- and C_SUM = 8 M
rounded up to one digit.  Measured on an MI355X: M = 4.69e-16, 8 M = 3.76e-15,
so C_SUM = 4e-15; ``test_tolerance_constant`` repeats the measurement and
fails if 8 M outgrows C_SUM.  An fp32 accumulation would show at >= 6e-8, seven
decades above.  (On that run the value cube's error never left the cast term:
0 x sum |terms| beyond 2^-24 |v| in all 347 comparisons.)

Every output buffer is sentinel-filled and carries a guard row after it.
Needs an MI355X: every test is marked ``gpu``.
"""

import numpy as np
import pytest

from conftest import load_golden
from oracle import kl as okl

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

M_MEASURED = 4.69e-16
C_SUM = 4e-15

SCRUB = 1           # SF_EVAL_NAN_SCRUB
FAST = 1 << 8       # SF_EVAL_FAST_SINCOS: not a flag of sf_kl_eval_values
NT = 1 << 9         # SF_EVAL_NT_STORES
BE = 1 << 10        # SF_EVAL_BIG_ENDIAN
SENT = -7.0

DS = (1, 3, 4, 5, 20, 59, 60, 61, 64, 65, 128)
# (nx, ny): one full 256-pixel block on float4 stores; P = 289, scalar stores
# and a 33-pixel tail block; nx != ny both ways (Q8's orientation); 16 blocks
GRIDS = ((16, 16), (17, 17), (20, 12), (12, 20), (64, 64))
SLOTS = (1, 15, 16, 17, 33, 70)
S_MAX = max(SLOTS)


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


def up(dev, a):
    return torch.from_numpy(np.array(a, np.float64, order="C")).to(dev)


def values(ctx, dev, coef, flags=0, ring=None, offset=0):
    """sf_kl_eval_values into a sentinel-filled buffer with a guard row after
    it (and ``offset`` floats in front): host [min(S, ring)][ny][nx] float32."""
    nx, ny = ctx.grid
    S = coef.shape[0]
    R = S if ring is None else min(S, ring)
    n = R * nx * ny
    buf = torch.full((offset + n + nx * ny,), SENT, dtype=torch.float32, device=dev)
    ctx.eval_values(up(dev, coef), S, buf[offset:offset + n], ring, flags)
    torch.cuda.synchronize()
    h = buf.cpu().numpy()
    assert np.all(h[:offset] == SENT) and np.all(h[offset + n:] == SENT), "guard"
    got = h[offset:offset + n].reshape(R, ny, nx)
    if not flags & BE:
        assert not np.any(got == SENT), "an output element was not written"
    return got


def bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


def geometry(D, nx, ny):
    """D piercepoints over +-3000 piercepoint pixels (the goldens span ~4000)
    and an nx x ny grid over a slightly larger, off-centre field."""
    rng = np.random.default_rng(1000 * D + 37 * nx + ny)
    pp = np.zeros((D, 3))
    pp[:, :2] = rng.uniform(-3000.0, 3000.0, (D, 2))
    x = np.linspace(-3300.0, 3250.0, nx)
    y = np.linspace(-3100.0, 3500.0, ny)
    coef = rng.uniform(-1.0, 1.0, (S_MAX, D))
    return pp, x, y, coef


_REF = {}


def reference(D, nx, ny):
    """(pp, x, y, coef, v [S_MAX][P] fp64, sum |terms| [S_MAX][P]), computed
    once per shape and shared (read-only) by the tests."""
    key = (D, nx, ny)
    if key not in _REF:
        pp, x, y, coef = geometry(D, nx, ny)
        cpix = okl.cpix_matrix(pp, x, y)
        v = okl.eval_phase_screens(coef, cpix)
        a = np.abs(coef) @ np.abs(cpix).T
        for arr in (pp, x, y, coef, v, a):
            arr.setflags(write=False)
        _REF[key] = (pp, x, y, coef, v, a)
    return _REF[key]


def check(got, v, a, what):
    """The module's tolerance; prints the figures before it asserts."""
    got = got.reshape(v.shape).astype(np.float64)
    err = np.abs(got - v)
    tol = 2.0 ** -24 * np.abs(v) + C_SUM * a
    worst = float((err / np.maximum(tol, 1e-300)).max())
    resid = float((np.maximum(err - 2.0 ** -24 * np.abs(v), 0.0) /
                   np.maximum(a, 1e-300)).max())
    print(f"{what}: max err / tol = {worst:.3f}, beyond the cast: {resid:.3g} x sum|terms|")
    assert np.all(err <= tol), (what, worst)


def bind(ctx, pp, x, y):
    ctx.set_piercepoints(pp)
    ctx.set_grid(x, y)


def nan_slot(S):
    """A slot in the middle of a 16-slot group (of the last group for S > 16)."""
    return min(S - 1, 16 * ((S - 1) // 16) + 7)


# ------------------------------------------------------------------ tolerance

def measure_m(ctx, dev):
    """max |sf_kl_eval_point_values - numpy| / sum |terms| over the shapes."""
    m = 0.0
    for D in DS:
        for nx, ny in GRIDS:
            pp, x, y, coef, v, a = reference(D, nx, ny)
            ctx.set_piercepoints(pp)
            X, Y = np.meshgrid(x, y)
            ctx.set_points(np.stack([X.ravel(), Y.ravel()], axis=1))
            out = torch.full((S_MAX, nx * ny), SENT, dtype=torch.float64, device=dev)
            ctx.eval_point_values(up(dev, coef), S_MAX, out)
            torch.cuda.synchronize()
            r = float((np.abs(out.cpu().numpy() - v) / a).max())
            print(f"D={D} {nx}x{ny}: point values vs numpy {r:.3g} x sum|terms|")
            m = max(m, r)
    return m


def test_tolerance_constant(ctx, dev):
    m = measure_m(ctx, dev)
    print(f"M = {m:.3g}, 8 M = {8 * m:.3g}, C_SUM = {C_SUM:.3g}")
    assert 8 * m <= 1e-10
    assert 8 * m <= C_SUM


# --------------------------------------------------------------------- shapes

@pytest.mark.parametrize("D", DS)
def test_shapes(ctx, dev, D):
    """Every grid x slot count against numpy; each also with a NaN slot: raw
    (a NaN plane, the other slots bit-equal) and scrubbed (a 0.0f plane)."""
    for nx, ny in GRIDS:
        pp, x, y, coef, v, a = reference(D, nx, ny)
        bind(ctx, pp, x, y)
        for S in SLOTS:
            got = values(ctx, dev, coef[:S])
            assert got.shape == (S, ny, nx)
            check(got, v[:S], a[:S], f"D={D} {nx}x{ny} S={S}")
            bad = nan_slot(S)
            c2 = coef[:S].copy()
            c2[bad, D // 2] = np.nan
            keep = np.arange(S) != bad
            raw = values(ctx, dev, c2)
            assert np.all(np.isnan(raw[bad]))
            np.testing.assert_array_equal(bits(raw[keep]), bits(got[keep]))
            scr = values(ctx, dev, c2, SCRUB)
            assert np.all(bits(scr[bad]) == 0)      # +0.0f
            np.testing.assert_array_equal(bits(scr[keep]), bits(got[keep]))


@pytest.mark.parametrize("D", [20, 65])
@pytest.mark.parametrize("grid", [(16, 16), (17, 17)])
def test_ring(ctx, dev, D, grid):
    """ring_slots = 16, S = 40: an entry ends up holding its last slot --
    entries 0..7 slots 32..39, entries 8..15 slots 24..31."""
    pp, x, y, coef, v, a = reference(D, *grid)
    bind(ctx, pp, x, y)
    full = values(ctx, dev, coef[:40])
    got = values(ctx, dev, coef[:40], ring=16)
    assert got.shape[0] == 16
    np.testing.assert_array_equal(bits(got[0:8]), bits(full[32:40]))
    np.testing.assert_array_equal(bits(got[8:16]), bits(full[24:32]))
    # a ring longer than the call: every slot its own place
    np.testing.assert_array_equal(bits(values(ctx, dev, coef[:40], ring=64)), bits(full))


@pytest.mark.parametrize("grid", [(16, 16), (20, 12), (17, 17)])
def test_output_offset_by_one_float(ctx, dev, grid):
    """A pointer that is only 4-byte aligned takes the scalar stores on an
    even grid: the same bits."""
    pp, x, y, coef, v, a = reference(20, *grid)
    bind(ctx, pp, x, y)
    want = values(ctx, dev, coef[:33])
    for off in (1, 2, 3):
        got = values(ctx, dev, coef[:33], offset=off)
        np.testing.assert_array_equal(bits(got), bits(want))
        check(got, v[:33], a[:33], f"offset {off} {grid}")


@pytest.mark.parametrize("D,grid", [(20, (64, 64)), (65, (17, 17)), (128, (20, 12))])
def test_work_item_walk(ctx, dev, D, grid):
    """SF_OPT_EVAL_MAX_BLOCKS = 2 and SF_OPT_EVAL_GROUPS = 1: few workgroups
    walk many one-group items; bit-equal to the default launch."""
    from ska_sdp_screen_fitting_amd._lib import (SF_OPT_EVAL_GROUPS,
                                                 SF_OPT_EVAL_MAX_BLOCKS)
    pp, x, y, coef, v, a = reference(D, *grid)
    bind(ctx, pp, x, y)
    want = values(ctx, dev, coef)
    ring_want = values(ctx, dev, coef, ring=32)
    try:
        ctx.set_option(SF_OPT_EVAL_MAX_BLOCKS, 2)
        ctx.set_option(SF_OPT_EVAL_GROUPS, 1)
        got = values(ctx, dev, coef)
        ring_got = values(ctx, dev, coef, ring=32)
    finally:
        ctx.set_option(SF_OPT_EVAL_MAX_BLOCKS, 0)
        ctx.set_option(SF_OPT_EVAL_GROUPS, 0)
    np.testing.assert_array_equal(bits(got), bits(want))
    np.testing.assert_array_equal(bits(ring_got), bits(ring_want))
    check(got, v, a, f"walk D={D} {grid}")


@pytest.mark.parametrize("grid", [(16, 16), (17, 17), (64, 64)])
def test_big_endian_and_nt_stores(ctx, dev, grid):
    pp, x, y, coef, v, a = reference(59, *grid)
    bind(ctx, pp, x, y)
    c2 = coef[:33].copy()
    c2[23, 5] = np.nan
    for base in (0, SCRUB):
        le = values(ctx, dev, c2, base)
        be = values(ctx, dev, c2, base | BE)
        np.testing.assert_array_equal(bits(be).byteswap(), bits(le))
        np.testing.assert_array_equal(bits(values(ctx, dev, c2, base | NT)), bits(le))
        np.testing.assert_array_equal(bits(values(ctx, dev, c2, base | NT | BE)), bits(be))
        # NT asked for where it cannot be honoured (unaligned): plain stores
        np.testing.assert_array_equal(bits(values(ctx, dev, c2, base | NT, offset=1)),
                                      bits(le))


def test_contract(dev):
    from ska_sdp_screen_fitting_amd._lib import Context, ScreenFitError
    c = Context(0)
    try:
        c.set_stream(torch.cuda.current_stream(dev).cuda_stream)
        pp, x, y, coef, v, a = reference(20, 16, 16)
        cd = up(dev, coef[:4])
        out = torch.full((5, 16, 16), SENT, dtype=torch.float32, device=dev)
        c.set_piercepoints(pp)
        with pytest.raises(ScreenFitError, match=r"\(-22\).*sf_set_grid"):
            c.eval_values(cd, 4, out.data_ptr())     # no grid
        c.set_grid(x, y)
        for bad in (FAST, 1 << 1, 1 << 11, 1 << 30):
            with pytest.raises(ScreenFitError, match=r"\(-22\)"):
                c.eval_values(cd, 4, out, flags=bad)
        with pytest.raises(ValueError):
            c.eval_values(cd, 4, out[:3])            # the binding: short buffer
        torch.cuda.synchronize()
        assert torch.all(out == SENT)
        c.eval_values(cd, 0, out)                    # S = 0: nothing
        c.eval_values(cd, 4, out)
        torch.cuda.synchronize()
        assert torch.all(out[4] == SENT) and not torch.any(out[:4] == SENT)
        # a new geometry drops the grid
        c.set_piercepoints(pp)
        with pytest.raises(ScreenFitError, match=r"\(-22\)"):
            c.eval_values(cd, 4, out.data_ptr())
    finally:
        c.close()


# --------------------------------------------- the reference's own coefficients

def test_tec14_reference_coefficients(ctx, dev):
    """The reference's tec fit (tec14 ``ref_coef``) on the 17 x 17 fixture
    grid: within the tolerance; the reference station's slots, whose
    coefficients are zero, exactly 0.0f (so are those of the all-NaN input
    block, which the reference fits to zeros)."""
    g = load_golden("tec14")
    fx = load_golden("fixture_kl")
    pp, x, y = g["piercepoints"], fx["x17"], fx["y17"]
    bind(ctx, pp, x, y)
    T, F, A, D = g["ref_coef"].shape
    coef = g["ref_coef"].reshape(-1, D)
    cpix = okl.cpix_matrix(pp, x, y)
    assert np.isfinite(coef).all()
    got = values(ctx, dev, coef).reshape(len(coef), -1)
    v = okl.eval_phase_screens(coef, cpix)
    a = np.abs(coef) @ np.abs(cpix).T
    ratio = a.sum() / np.abs(v).sum()
    print(f"tec14 on 17^2: sum|terms| / |value| = {ratio:.1f} (mean)")
    check(got, v, a, "tec14 ref_coef")
    ref = int(g["ref_ref_ant"])
    zero = got.reshape(T, F, A, -1)[:, :, ref]
    assert np.all(g["ref_coef"][:, :, ref] == 0)
    assert np.all(zero == 0.0)
    assert np.all(got.reshape(T, F, A, -1)[:, 1, 3] == 0.0)
    assert np.any(got != 0.0)
    scr = values(ctx, dev, coef, SCRUB).reshape(len(coef), -1)
    np.testing.assert_array_equal(bits(scr), bits(got))


def test_cross_check_with_the_jones_cube(ctx, dev):
    """synth20 on 17 x 17 in one context: sf_kl_eval's planes 0 / 1 are
    cos / sin of the fp64 value (1e-6), the value cube is that value, and an
    interleaved sf_kl_eval_values call leaves sf_kl_eval's bytes alone."""
    g = load_golden("synth20")
    pp, x, y = g["piercepoints"], g["x17"], g["y17"]
    ctx.set_piercepoints(pp, float(g["r_0"]), float(g["beta"]))
    ctx.set_grid(x, y)
    D = g["coef"].shape[-1]
    coef = g["coef"].reshape(-1, D)
    coef = coef[np.isfinite(coef).all(axis=1)]
    S = len(coef)
    cpix = okl.cpix_matrix(pp, x, y, float(g["r_0"]), float(g["beta"]))
    v = okl.eval_phase_screens(coef, cpix)
    cd = up(dev, coef)
    for flags in (0, FAST):
        before = torch.full((S, 4, 17, 17), SENT, dtype=torch.float32, device=dev)
        ctx.eval(cd, S, before, flags=flags)
        vals = values(ctx, dev, coef)
        after = torch.full((S, 4, 17, 17), SENT, dtype=torch.float32, device=dev)
        ctx.eval(cd, S, after, flags=flags)
        torch.cuda.synchronize()
        assert torch.equal(before.view(torch.int32), after.view(torch.int32))
        pl = before.cpu().numpy().reshape(S, 4, -1)
        e_cos, e_sin = np.abs(pl[:, 0] - np.cos(v)).max(), np.abs(pl[:, 1] - np.sin(v)).max()
        print(f"flags={flags:#x}: planes vs cos / sin of the value {e_cos:.3g} / {e_sin:.3g}")
        assert e_cos <= 1e-6 and e_sin <= 1e-6
        check(vals, v, np.abs(coef) @ np.abs(cpix).T, "synth20 values")


def test_evaluator_values(dev):
    """KLEvaluator.values_device / values_host: shapes, dtype, the numbers."""
    from ska_sdp_screen_fitting_amd.kl_screen import KLEvaluator
    pp, x, y, coef, v, a = reference(20, 20, 12)
    ev = KLEvaluator(pp, 100.0, 5.0 / 3.0, x, y)
    h = ev.values_host(coef[:12].reshape(3, 4, 20).copy())
    assert h.shape == (3, 4, 12, 20) and h.dtype == np.float32
    check(h, v[:12], a[:12], "values_host")
    d = ev.values_device(up(dev, coef[:12]))
    assert d.shape == (12, 12, 20) and d.dtype == torch.float32 and d.is_cuda
    np.testing.assert_array_equal(bits(d.cpu().numpy().reshape(h.shape)), bits(h))


# ---------------------------------------------------------------- end to end

BOUNDS = dict(bounds_deg=[124.565, 66.165, 127.895, 62.835],
              bounds_mid_deg=[126.23, 64.50], padding_fraction=0, cellsize_deg=0.2)
# gain rendering: 120 / 150 / 180 MHz, k / nu = -70 / -56 / -47 rad per TECU; the
# fixture's dTEC screens stay below 1 TECU on the grid, so the phases stay
# below ~100 rad (printed below)
NU_HZ = [1.2e8, 1.5e8, 1.8e8]


@pytest.fixture(scope="module")
def tec_h5(tmp_path_factory):
    """tec14's values as a ``tec`` soltab in an H5parm written by the
    package's own writer (float32 weights: the tiny ones exactly)."""
    from ska_sdp_screen_fitting_amd.h5parm import Solset, Soltab, write_h5parm
    g = load_golden("tec14")
    ants = [str(s) for s in g["ant_names"]]
    dirs = [str(s) for s in g["dir_names"]]
    ss = Solset("sol000", ants, g["ant_pos"], dirs, g["dir_radec"])
    ss.soltabs["tec000"] = Soltab(
        "tec000", "tec", ["time", "freq", "ant", "dir"],
        [g["times"], g["freqs"], np.array(ants), np.array(dirs)],
        g["val"], g["weight"], solset=ss)
    path = str(tmp_path_factory.mktemp("tec") / "tec14.h5")
    write_h5parm(path, [ss], weight_dtype=np.float32)
    return path, g


@pytest.fixture(scope="module")
def tec_screen(dev, tec_h5):
    """The fitted screen object: its ``vals_ph`` are ``tec_screen000``."""
    from ska_sdp_screen_fitting_amd.kl_tec_screen import KLTecScreen
    path, g = tec_h5
    # the width make_tec_aterm_image derives from BOUNDS (padding_fraction 0)
    b = BOUNDS["bounds_deg"]
    pad = (b[3] - b[1]) * (0.0 - 1.0)
    width = (b[3] + pad) - (b[1] - pad)
    scr = KLTecScreen("tec", path, None, 126.23, 64.50, width, width,
                      tec_soltab_name="tec000")
    scr.process(ncpu=0)
    from ska_sdp_screen_fitting_amd import geometry as geo
    x, y = geo.grid_coords(scr.rad, scr.dec, scr.width_ra, 0.2, scr.mid_ra, scr.mid_dec)
    cpix = okl.cpix_matrix(scr.piercepoints, x, y, scr.r_0, scr.beta_val)
    return scr, cpix


def test_make_tec_aterm_image_tec(tmp_path, tec_h5, tec_screen):
    from ska_sdp_screen_fitting_amd import fits as sffits
    from ska_sdp_screen_fitting_amd import make_tec_aterm_image
    path, g = tec_h5
    scr, cpix = tec_screen
    outroot = str(tmp_path / "dtec")
    assert make_tec_aterm_image(path, soltabname="tec000", outroot=outroot,
                                aterm_type="tec", **BOUNDS) is None
    with open(outroot + ".txt", encoding="utf8") as fh:
        assert fh.read().split() == [outroot + "_0.fits"]
    hdr, cube = sffits.read_cube(outroot + "_0.fits")
    assert cube.shape == (10, 2, 6, 17, 17) and cube.dtype == np.dtype(">f4")
    want_hdr = sffits.tec_header(126.23, 64.50, 17, 17, 0.2, g["freqs"], g["times"], 6)
    assert list(hdr) == [k for k, _ in want_hdr]
    for k, v in want_hdr:
        if isinstance(v, float):
            assert hdr[k] == float(sffits.card(k, v)[10:30]), k
        else:
            assert hdr[k] == v, k
    coef = np.asarray(scr.vals_ph)
    T, F, A, D = coef.shape
    assert (T, F, A, D) == (10, 2, 6, 14)
    flat = coef.reshape(-1, D)
    fin = np.isfinite(flat).all(axis=1)
    # (the all-NaN input block is fitted to zero coefficients with zero
    # weights; any NaN coefficient would be scrubbed to 0 on the device)
    data = np.asarray(cube, np.float32).reshape(len(flat), -1)
    check(data[fin], okl.eval_phase_screens(flat[fin], cpix),
          np.abs(flat[fin]) @ np.abs(cpix).T, "dTEC cube vs the fitted coefficients")
    assert np.all(data[~fin] == 0.0)        # NaN-scrubbed on the device
    assert np.all(cube[:, :, scr.ref_ind] == 0.0)
    assert np.any(data[fin] != 0.0)
    # make_matrix: one (freq, station), raw (NaN kept), the cube's rounding
    m = scr.make_matrix(2, 7, 1, 4, 0.2)
    assert m.shape == (5, 17, 17) and m.dtype == np.float64
    np.testing.assert_array_equal(m, np.asarray(cube[2:7, 1, 4], np.float64))
    assert np.all(scr.make_matrix(0, 10, 1, 3, 0.2) == 0.0)   # the all-NaN block


def test_make_tec_aterm_image_gain(tmp_path, tec_h5, tec_screen):
    from ska_sdp_screen_fitting_amd import fits as sffits
    from ska_sdp_screen_fitting_amd import make_tec_aterm_image
    from ska_sdp_screen_fitting_amd.kl_tec_screen import TEC_TO_PHASE
    from ska_sdp_screen_fitting_amd.screen import nearest_index
    path, g = tec_h5
    scr, cpix = tec_screen
    outroot = str(tmp_path / "jones")
    make_tec_aterm_image(path, soltabname="tec000", outroot=outroot,
                         aterm_type="gain", freqs_hz=NU_HZ, **BOUNDS)
    hdr, cube = sffits.read_cube(outroot + "_0.fits")
    assert cube.shape == (10, 3, 6, 4, 17, 17)
    assert hdr["CTYPE3"] == "MATRIX" and hdr["CRVAL5"] == NU_HZ[0]
    coef = np.asarray(scr.vals_ph)
    T, F, A, D = coef.shape
    fidx = nearest_index(g["freqs"], NU_HZ)
    print("tec frequencies", g["freqs"], "-> index per output frequency", fidx)
    v = np.einsum("tfad,pd->tfap", coef[:, fidx], cpix)
    phase = (TEC_TO_PHASE / np.array(NU_HZ))[None, :, None, None] * v
    fin = np.isfinite(phase)
    print(f"largest |dTEC| {np.nanmax(np.abs(v)):.3g} TECU, |phase| "
          f"{np.nanmax(np.abs(phase)):.3g} rad")
    assert np.nanmax(np.abs(phase)) < 500.0
    data = np.asarray(cube, np.float64).reshape(T, 3, A, 4, -1)
    for q, fn in enumerate((np.cos, np.sin, np.cos, np.sin)):
        err = np.abs(data[:, :, :, q] - fn(phase))[fin].max()
        print(f"plane {q}: {err:.3g}")
        assert err <= 1e-6
        # a NaN coefficient is scrubbed to 1 / 0
        assert np.all(data[:, :, :, q][~fin] == (1.0 if q % 2 == 0 else 0.0))
        # zero coefficients (reference station, the all-NaN input block): 1 / 0
        assert np.all(data[:, :, scr.ref_ind, q] == (1.0 if q % 2 == 0 else 0.0))
    # another constant: the phases scale with it
    outroot2 = str(tmp_path / "jones2")
    make_tec_aterm_image(path, soltabname="tec000", outroot=outroot2,
                         aterm_type="gain", freqs_hz=NU_HZ, tec_to_phase=1.0e9, **BOUNDS)
    _, cube2 = sffits.read_cube(outroot2 + "_0.fits")
    ph2 = (1.0e9 / np.array(NU_HZ))[None, :, None, None] * v
    err = np.abs(np.asarray(cube2, np.float64).reshape(T, 3, A, 4, -1)[:, :, :, 1]
                 - np.sin(ph2))[fin].max()
    assert err <= 1e-6
