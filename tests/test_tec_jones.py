"""TEC screens to Jones cubes at many channels (sf_set_tec_freqs /
sf_kl_eval_tec, csrc/kl_tec.hip) and the product path built on them
(KLEvaluator.eval_tec_*, KLTecScreen(..., phase_soltab_name), fused=True).

Reference: fp64 numpy from ``oracle.kl.cpix_matrix`` and the contract

    out[t][f][a][.][p] = (cos, sin, cos, sin)(
        rad_per_tecu[f] * sum_d Cpix[p][d] tec[t][i_f][a][d]
                        + sum_d Cpix[p][d] ph[t][i_f][a][d] ),  i_f = tec_index[f].

Inputs are scaled so |phase| < 500 rad (asserted), where numpy's cos / sin are
good to ~1e-13.  Tolerance: the project's for every evaluation test
(tests/test_wide_eval.py, tests/test_points.py): 2e-6 with SF_EVAL_FAST_SINCOS,
1e-6 without.

Every output buffer is sentinel-filled with guard regions before and after it.
Needs an MI355X: every test is marked ``gpu``.
"""

import numpy as np
import pytest

from conftest import load_golden
from oracle import kl as okl

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

SCRUB = 1           # SF_EVAL_NAN_SCRUB
FAST = 1 << 8       # SF_EVAL_FAST_SINCOS
NT = 1 << 9         # SF_EVAL_NT_STORES
BE = 1 << 10        # SF_EVAL_BIG_ENDIAN
SENT = -7.0
GUARD = 64          # floats in front of the output: 256 B, keeps its alignment
TOL = {FAST: 2e-6, 0: 1e-6}

# rad per TECU at 120 / 150 / 180 MHz with the usual constant
K3 = -8.4479745e9 / np.array([1.2e8, 1.5e8, 1.8e8])
IDX3 = [0, 1, 1]
T0, A0 = 5, 6       # 30 slots: a ragged second group, groups straddle time rows


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


def bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


def tec_eval(ctx, dev, tec, k, idx=None, ph=None, flags=SCRUB | FAST, offset=0, bind=True):
    """sf_kl_eval_tec into a sentinel-filled buffer with GUARD floats in front
    (plus ``offset``) and a slot-sized guard after: host [T][F][A][4][ny][nx]."""
    nx, ny = ctx.grid
    T, F_tec, A, D = tec.shape
    F = len(k)
    if bind:
        ctx.set_tec_freqs(k, idx, F_tec)
    n = T * F * A * 4 * nx * ny
    lo = GUARD + offset
    buf = torch.full((lo + n + 4 * nx * ny,), SENT, dtype=torch.float32, device=dev)
    ctx.eval_tec(up(dev, tec), T, A, buf[lo:lo + n],
                 None if ph is None else up(dev, ph), flags)
    torch.cuda.synchronize()
    h = buf.cpu().numpy()
    assert np.all(h[:lo] == SENT) and np.all(h[lo + n:] == SENT), "guard"
    got = h[lo:lo + n].reshape(T, F, A, 4, ny, nx)
    if not flags & BE:
        assert not np.any(got == SENT), "an output element was not written"
    return got


def geometry(D, nx, ny):
    rng = np.random.default_rng(7000 * D + 37 * nx + ny)
    pp = np.zeros((D, 3))
    pp[:, :2] = rng.uniform(-3000.0, 3000.0, (D, 2))
    x = np.linspace(-3300.0, 3250.0, nx)
    y = np.linspace(-3100.0, 3500.0, ny)
    return rng, pp, x, y


_REF = {}


def reference(D, nx, ny, T=T0, A=A0, F_tec=2, k=K3, idx=IDX3):
    """(pp, x, y, tec, ph, phase_tec [T][F][A][P], phase_ph [T][F][A][P]): the
    fp64 phases of the TEC part and of the phase part, computed once per shape
    and shared read-only.  The coefficients are scaled so the TEC part stays
    below 300 rad and the phase part below 100 rad."""
    key = (D, nx, ny, T, A, F_tec, tuple(k), tuple(idx))
    if key not in _REF:
        rng, pp, x, y = geometry(D, nx, ny)
        cpix = okl.cpix_matrix(pp, x, y)
        tec = rng.uniform(-1.0, 1.0, (T, F_tec, A, D))
        ph = rng.uniform(-1.0, 1.0, (T, F_tec, A, D))
        k = np.asarray(k)
        v = np.einsum("tiad,pd->tiap", tec, cpix)[:, idx] * k[None, :, None, None]
        tec *= 300.0 / np.abs(v).max()
        w = np.einsum("tiad,pd->tiap", ph, cpix)
        ph *= 100.0 / np.abs(w).max()
        p_tec = np.einsum("tiad,pd->tiap", tec, cpix)[:, idx] * k[None, :, None, None]
        p_ph = np.einsum("tiad,pd->tiap", ph, cpix)[:, idx]
        assert np.abs(p_tec).max() + np.abs(p_ph).max() < 500.0
        for arr in (pp, x, y, tec, ph, p_tec, p_ph):
            arr.setflags(write=False)
        _REF[key] = (pp, x, y, tec, ph, p_tec, p_ph)
    return _REF[key]


def check(got, phase, flags, what):
    """Planes against cos / sin of the fp64 phase; prints before it asserts."""
    assert np.nanmax(np.abs(phase)) < 500.0
    g = got.reshape(phase.shape[:3] + (4, -1)).astype(np.float64)
    tol = TOL[flags & FAST]
    worst = 0.0
    for q, fn in enumerate((np.cos, np.sin, np.cos, np.sin)):
        worst = max(worst, float(np.abs(g[:, :, :, q] - fn(phase)).max()))
    print(f"{what}: max |plane - cos / sin| = {worst:.3g} (tol {tol:g})")
    assert worst <= tol, (what, worst)


def bind(ctx, pp, x, y):
    ctx.set_piercepoints(pp)
    ctx.set_grid(x, y)


# ------------------------------------------------------------------- 1. accuracy

@pytest.mark.parametrize("D", [1, 7, 20, 50, 61, 128])
def test_accuracy(ctx, dev, D):
    """17 x 17 (P = 289: scalar stores, a 33-pixel last block), 30 slots,
    F_tec = 2, F = 3 with index [0, 1, 1]; fast and fp64 sincos, the scrub on;
    with and without phase coefficients."""
    pp, x, y, tec, ph, p_tec, p_ph = reference(D, 17, 17)
    bind(ctx, pp, x, y)
    for flags in (SCRUB | FAST, SCRUB):
        got = tec_eval(ctx, dev, tec, K3, IDX3, None, flags)
        assert got.shape == (T0, 3, A0, 4, 17, 17) and not np.isnan(got).any()
        check(got, p_tec, flags, f"D={D} flags={flags:#x} tec")
        np.testing.assert_array_equal(bits(got[:, :, :, 0]), bits(got[:, :, :, 2]))
        np.testing.assert_array_equal(bits(got[:, :, :, 1]), bits(got[:, :, :, 3]))
        got = tec_eval(ctx, dev, tec, K3, IDX3, ph, flags)
        check(got, p_tec + p_ph, flags, f"D={D} flags={flags:#x} tec + phase")


# ---------------------------------------------------------------- 2. store paths

@pytest.mark.parametrize("grid", [(20, 18), (16, 16)])
@pytest.mark.parametrize("with_ph", [False, True])
def test_store_paths(ctx, dev, grid, with_ph):
    """P = 360 (float4 stores, a partial last block) and 256: NT and plain
    stores, a 4-byte offset (scalar stores) and the byte swap write the same
    values."""
    pp, x, y, tec, ph, p_tec, p_ph = reference(20, *grid)
    bind(ctx, pp, x, y)
    p = ph if with_ph else None
    for base in (SCRUB | FAST, SCRUB):
        le = tec_eval(ctx, dev, tec, K3, IDX3, p, base)
        check(le, p_tec + p_ph if with_ph else p_tec, base, f"{grid} flags={base:#x}")
        nt = tec_eval(ctx, dev, tec, K3, IDX3, p, base | NT)
        np.testing.assert_array_equal(bits(nt), bits(le))
        off = tec_eval(ctx, dev, tec, K3, IDX3, p, base | NT, offset=1)
        np.testing.assert_array_equal(bits(off), bits(le))
        be = tec_eval(ctx, dev, tec, K3, IDX3, p, base | BE)
        np.testing.assert_array_equal(bits(be).byteswap(), bits(le))
        be1 = tec_eval(ctx, dev, tec, K3, IDX3, p, base | BE | NT, offset=1)
        np.testing.assert_array_equal(bits(be1), bits(be))


# ----------------------------------------------------------------------- 3. NaN

@pytest.mark.parametrize("grid", [(17, 17), (20, 18)])
@pytest.mark.parametrize("F_tec", [1, 2])
def test_nan_stays_in_its_slot(ctx, dev, grid, F_tec):
    """One NaN in one slot's TEC row, one in another slot's phase row.  Raw:
    those (t, a) are NaN in every channel of their TEC frequency (all F
    channels for F_tec = 1) and every other output bit is untouched; scrubbed:
    exactly 1 / 0 there."""
    idx = [0, 0, 0] if F_tec == 1 else IDX3
    pp, x, y, tec, ph, p_tec, p_ph = reference(20, *grid, F_tec=F_tec, idx=idx)
    bind(ctx, pp, x, y)
    i_ph = F_tec - 1
    t2, p2 = tec.copy(), ph.copy()
    t2[1, 0, 2, 7] = np.nan       # slot s = 1 * 6 + 2 = 8
    p2[3, i_ph, 4, 19] = np.nan   # slot s = 22, the ragged second group
    bad = np.zeros((T0, 3, A0), bool)
    bad[1, [f for f in range(3) if idx[f] == 0], 2] = True
    bad[3, [f for f in range(3) if idx[f] == i_ph], 4] = True
    assert bad.sum() == (6 if F_tec == 1 else 3)
    for base in (FAST, 0):
        clean = tec_eval(ctx, dev, tec, K3, idx, ph, base)
        raw = tec_eval(ctx, dev, t2, K3, idx, p2, base)
        assert np.isnan(raw[bad]).all()
        np.testing.assert_array_equal(bits(raw[~bad]), bits(clean[~bad]))
        scr = tec_eval(ctx, dev, t2, K3, idx, p2, base | SCRUB)
        assert np.all(scr[bad][:, [0, 2]] == 1.0) and np.all(scr[bad][:, [1, 3]] == 0.0)
        np.testing.assert_array_equal(bits(scr[~bad]), bits(clean[~bad]))
        # a NaN in the TEC row alone, no phase coefficients
        raw = tec_eval(ctx, dev, t2, K3, idx, None, base)
        only = np.zeros_like(bad)
        only[1, [f for f in range(3) if idx[f] == 0], 2] = True
        assert np.isnan(raw[only]).all() and not np.isnan(raw[~only]).any()


# ---------------------------------------------------------------- 4. invariants

@pytest.mark.parametrize("D,grid", [(20, (17, 17)), (61, (20, 18))])
def test_channels_and_rows_are_independent(ctx, dev, D, grid):
    """Channel f of an F-channel call equals a one-channel call of that
    frequency; T rows at once equal the rows one by one.  Bit for bit."""
    pp, x, y, tec, ph, p_tec, p_ph = reference(D, *grid)
    bind(ctx, pp, x, y)
    for p in (None, ph):
        full = tec_eval(ctx, dev, tec, K3, IDX3, p)
        for f in range(3):
            one = tec_eval(ctx, dev, tec, K3[f:f + 1], IDX3[f:f + 1], p)
            np.testing.assert_array_equal(bits(one[:, 0]), bits(full[:, f]))
        ctx.set_tec_freqs(K3, IDX3, 2)
        for t in range(T0):
            row = tec_eval(ctx, dev, tec[t:t + 1], K3, IDX3,
                           None if p is None else p[t:t + 1], bind=False)
            np.testing.assert_array_equal(bits(row[0]), bits(full[t]))


def test_work_item_walk(ctx, dev):
    """1,000 slots at 8 x 8: SF_OPT_EVAL_MAX_BLOCKS = 1 and 2 and
    SF_OPT_EVAL_GROUPS = 1 (few workgroups walk many items) equal the default
    launch bit for bit."""
    from ska_sdp_screen_fitting_amd._lib import (SF_OPT_EVAL_GROUPS,
                                                 SF_OPT_EVAL_MAX_BLOCKS)
    k, idx = K3[:2], [0, 0]
    pp, x, y, tec, ph, p_tec, p_ph = reference(20, 8, 8, T=125, A=8, F_tec=1, k=k, idx=idx)
    bind(ctx, pp, x, y)
    want = tec_eval(ctx, dev, tec, k, idx, ph)
    check(want, p_tec + p_ph, SCRUB | FAST, "1,000 slots, default launch")
    try:
        for blocks, groups in ((1, 0), (2, 0), (0, 1), (2, 1)):
            ctx.set_option(SF_OPT_EVAL_MAX_BLOCKS, blocks)
            ctx.set_option(SF_OPT_EVAL_GROUPS, groups)
            got = tec_eval(ctx, dev, tec, k, idx, ph)
            np.testing.assert_array_equal(bits(got), bits(want))
    finally:
        ctx.set_option(SF_OPT_EVAL_MAX_BLOCKS, 0)
        ctx.set_option(SF_OPT_EVAL_GROUPS, 0)


def test_interleaved_with_sf_kl_eval(ctx, dev):
    """sf_kl_eval between two sf_kl_eval_tec calls: neither changes the
    other's output."""
    pp, x, y, tec, ph, p_tec, p_ph = reference(20, 17, 17)
    bind(ctx, pp, x, y)
    coef = up(dev, tec.reshape(-1, 20))
    S = coef.shape[0]
    first = tec_eval(ctx, dev, tec, K3, IDX3, ph)
    a = torch.full((S, 4, 17, 17), SENT, dtype=torch.float32, device=dev)
    ctx.eval(coef, S, a)
    again = tec_eval(ctx, dev, tec, K3, IDX3, ph, bind=False)
    b = torch.full((S, 4, 17, 17), SENT, dtype=torch.float32, device=dev)
    ctx.eval(coef, S, b)
    torch.cuda.synchronize()
    np.testing.assert_array_equal(bits(again), bits(first))
    assert torch.equal(a.view(torch.int32), b.view(torch.int32))
    assert not torch.any(a == SENT)


# ------------------------------------------------------ 5. an unused TEC frequency

@pytest.mark.parametrize("grid", [(17, 17), (16, 16)])
def test_unused_tec_frequency_is_never_read(ctx, dev, grid):
    """F_tec = 3, index [2, 0]: the middle frequency's coefficients are all
    NaN, and no scrub is asked for; the cube is correct and holds no NaN."""
    k, idx = K3[:2], [2, 0]
    pp, x, y, tec, ph, p_tec, p_ph = reference(20, *grid, F_tec=3, k=k, idx=idx)
    bind(ctx, pp, x, y)
    t2, p2 = tec.copy(), ph.copy()
    t2[:, 1] = np.nan
    p2[:, 1] = np.nan
    for flags in (FAST, 0):
        got = tec_eval(ctx, dev, t2, k, idx, p2, flags)
        assert not np.isnan(got).any()
        check(got, p_tec + p_ph, flags, f"unused frequency {grid} flags={flags:#x}")
        np.testing.assert_array_equal(bits(got), bits(tec_eval(ctx, dev, tec, k, idx, ph, flags)))


# -------------------------------------------------------------------- 6. errors

def test_contract(dev):
    from ska_sdp_screen_fitting_amd._lib import SF_MAX_TEC_FREQ, Context, ScreenFitError
    pp, x, y, tec, ph, p_tec, p_ph = reference(20, 17, 17)
    td = up(dev, tec)
    out = torch.full((T0 * 3 * A0 * 4 * 289 + 64,), SENT, dtype=torch.float32, device=dev)
    einval = r"\(-22\)"
    c = Context(0)
    try:
        c.set_stream(torch.cuda.current_stream(dev).cuda_stream)
        c.set_piercepoints(pp)
        c.set_tec_freqs(K3, IDX3, 2)
        with pytest.raises(ScreenFitError, match=einval + r".*sf_set_grid"):
            c.eval_tec(td, T0, A0, out)                  # channels but no grid
    finally:
        c.close()
    c = Context(0)
    try:
        c.set_stream(torch.cuda.current_stream(dev).cuda_stream)
        c.set_piercepoints(pp)
        c.set_grid(x, y)
        with pytest.raises(ScreenFitError, match=einval + r".*sf_set_tec_freqs"):
            c.eval_tec(td, T0, A0, out.data_ptr())       # a grid but no channels
        # sf_set_tec_freqs: every SF_EINVAL case
        for k, idx, n in ((np.zeros(0), None, 1),                      # F = 0
                          (np.ones(SF_MAX_TEC_FREQ + 1), None, 1),     # F too large
                          (K3, IDX3, 0),                               # F_tec < 1
                          (K3, [0, 2, 1], 2), (K3, [0, -1, 1], 2),     # index out of range
                          (np.array([1.0, np.nan]), None, 1),
                          (np.array([np.inf, 1.0]), None, 1)):
            with pytest.raises(ScreenFitError, match=einval + r".*sf_set_tec_freqs"):
                c.set_tec_freqs(k, idx, n)
        assert c.lib.sf_set_tec_freqs(c.h, None, None, 1, 1) == -22   # NULL scales
        with pytest.raises(ScreenFitError, match=einval + r".*sf_set_tec_freqs"):
            c.eval_tec(td, T0, A0, out.data_ptr())       # still no binding
        c.set_tec_freqs(np.ones(SF_MAX_TEC_FREQ), None, 1)             # the largest F
        c.set_tec_freqs(K3, IDX3, 2)
        n = T0 * 3 * A0 * 4 * 289
        c.eval_tec(td, T0, A0, out[:n])
        torch.cuda.synchronize()
        want = out[:n].clone()
        # a failed call keeps the previous binding
        with pytest.raises(ScreenFitError, match=einval):
            c.set_tec_freqs(K3, [0, 5, 1], 2)
        out.fill_(SENT)
        c.eval_tec(td, T0, A0, out[:n])
        torch.cuda.synchronize()
        assert torch.equal(out[:n].view(torch.int32), want.view(torch.int32))
        assert torch.all(out[n:] == SENT)
        # flags: any bit but the four is refused, and nothing is written
        out.fill_(SENT)
        for bad in (1 << 1, 1 << 7, 1 << 11, 1 << 27, 1 << 30, 1 << 31):
            with pytest.raises(ScreenFitError, match=einval + r".*sf_kl_eval_tec"):
                c.eval_tec(td, T0, A0, out, flags=FAST | bad)
        with pytest.raises(ScreenFitError, match=einval):
            c.eval_tec(td, T0, 0, out.data_ptr())        # A < 1
        with pytest.raises(ScreenFitError, match=einval):
            c.eval_tec(td, T0, A0, out.data_ptr() + 2)   # not 4-byte aligned
        with pytest.raises(ValueError):
            c.eval_tec(td, T0, A0, out[:n - 1])          # the binding: short buffer
        c.eval_tec(td, 0, A0, out)                       # T = 0: nothing
        torch.cuda.synchronize()
        assert torch.all(out == SENT)
        # a new geometry with another D drops the grid, not the channels
        pp7, x7, y7, tec7, ph7, pt7, pp7h = reference(7, 17, 17)
        c.set_basis(pp7)
        with pytest.raises(ScreenFitError, match=einval + r".*sf_set_grid"):
            c.eval_tec(up(dev, tec7), T0, A0, out.data_ptr())
        c.set_grid(x7, y7)
        c.eval_tec(up(dev, tec7), T0, A0, out[:n], flags=SCRUB | FAST)
        torch.cuda.synchronize()
        check(out[:n].cpu().numpy().reshape(T0, 3, A0, 4, 17, 17), pt7, FAST,
              "after sf_set_basis with D = 7, the old channel binding")
    finally:
        c.close()


# -------------------------------------------------------------- 7. product path

BOUNDS = dict(bounds_deg=[124.565, 66.165, 127.895, 62.835],
              bounds_mid_deg=[126.23, 64.50], padding_fraction=0, cellsize_deg=0.2)
NU_HZ = [1.2e8, 1.5e8, 1.8e8]


@pytest.fixture(scope="module")
def tec_h5(tmp_path_factory):
    """tec14's values as a ``tec`` soltab in an H5parm written by the
    package's own writer (the recipe of tests/test_values.py), plus a scalar
    ``phase`` soltab on the same times, stations and directions with ONE
    frequency: smooth per-direction phases of a few tenths of a radian."""
    from ska_sdp_screen_fitting_amd.h5parm import Solset, Soltab, write_h5parm
    g = load_golden("tec14")
    ants = [str(s) for s in g["ant_names"]]
    dirs = [str(s) for s in g["dir_names"]]
    ss = Solset("sol000", ants, g["ant_pos"], dirs, g["dir_radec"])
    ss.soltabs["tec000"] = Soltab(
        "tec000", "tec", ["time", "freq", "ant", "dir"],
        [g["times"], g["freqs"], np.array(ants), np.array(dirs)],
        g["val"], g["weight"], solset=ss)
    T, F, A, D = g["val"].shape
    rng = np.random.default_rng(14)
    radec = np.asarray(g["dir_radec"], np.float64)
    slope = rng.normal(0.0, 4.0, (T, 1, A, 2))
    phi = (slope[..., :1] * (radec[:, 0] - radec[:, 0].mean())
           + slope[..., 1:] * (radec[:, 1] - radec[:, 1].mean())
           + rng.normal(0.0, 0.02, (T, 1, A, D)))
    ss.soltabs["phase000"] = Soltab(
        "phase000", "phase", ["time", "freq", "ant", "dir"],
        [g["times"], g["freqs"][:1], np.array(ants), np.array(dirs)],
        phi, np.ones(phi.shape, np.float32), solset=ss)
    path = str(tmp_path_factory.mktemp("tecjones") / "tec14.h5")
    write_h5parm(path, [ss], weight_dtype=np.float32)
    return path, g


def fitted(path, phase_soltab_name):
    from ska_sdp_screen_fitting_amd import geometry as geo
    from ska_sdp_screen_fitting_amd.kl_tec_screen import KLTecScreen
    b = BOUNDS["bounds_deg"]
    pad = (b[3] - b[1]) * (0.0 - 1.0)
    width = (b[3] + pad) - (b[1] - pad)
    scr = KLTecScreen("tec", path, None, 126.23, 64.50, width, width,
                      tec_soltab_name="tec000", phase_soltab_name=phase_soltab_name)
    scr.process(ncpu=0)
    x, y = geo.grid_coords(scr.rad, scr.dec, scr.width_ra, 0.2, scr.mid_ra, scr.mid_dec)
    cpix = okl.cpix_matrix(scr.piercepoints, x, y, scr.r_0, scr.beta_val)
    return scr, cpix


def cube_of(tmp_path, path, name, **kw):
    from ska_sdp_screen_fitting_amd import fits as sffits
    from ska_sdp_screen_fitting_amd import make_tec_aterm_image
    outroot = str(tmp_path / name)
    make_tec_aterm_image(path, soltabname="tec000", outroot=outroot, aterm_type="gain",
                         freqs_hz=NU_HZ, **BOUNDS, **kw)
    hdr, cube = sffits.read_cube(outroot + "_0.fits")
    assert cube.shape == (10, 3, 6, 4, 17, 17)
    return np.asarray(cube, np.float64).reshape(10, 3, 6, 4, -1)


@pytest.mark.parametrize("phase_soltab_name", [None, "phase000"])
def test_make_tec_aterm_image_fused(dev, tmp_path, tec_h5, phase_soltab_name):
    """The gain cube through the fused evaluation against numpy (as
    tests/test_values.py checks the replicated one), and against the
    replicated path within twice the tolerance; with the phase soltab, the
    phase phi0 + k dTEC / nu, and 1 / 0 at the reference station."""
    from ska_sdp_screen_fitting_amd.kl_tec_screen import TEC_TO_PHASE
    from ska_sdp_screen_fitting_amd.screen import nearest_index
    path, g = tec_h5
    scr, cpix = fitted(path, phase_soltab_name)
    coef = np.asarray(scr.vals_ph)
    assert coef.shape == (10, 2, 6, 14)
    fidx = nearest_index(g["freqs"], NU_HZ)
    v = np.einsum("tfad,pd->tfap", coef[:, fidx], cpix)
    phase = (TEC_TO_PHASE / np.array(NU_HZ))[None, :, None, None] * v
    if phase_soltab_name is None:
        assert scr.vals_phi0 is None
    else:
        phi0 = np.asarray(scr.vals_phi0)
        assert phi0.shape == coef.shape          # the one frequency, broadcast
        np.testing.assert_array_equal(phi0[:, 0], phi0[:, 1])
        assert np.all(phi0[:, :, scr.ref_ind] == 0) and np.any(phi0 != 0)
        phase = phase + np.einsum("tfad,pd->tfap", phi0[:, fidx], cpix)
    fin = np.isfinite(phase)
    print(f"largest |phase| {np.nanmax(np.abs(phase)):.3g} rad")
    assert np.nanmax(np.abs(phase)) < 500.0
    kw = dict(phase_soltab_name=phase_soltab_name)
    fused = cube_of(tmp_path, path, "fused", fused=True, **kw)
    plain = cube_of(tmp_path, path, "plain", fused=False, **kw)
    for q, fn in enumerate((np.cos, np.sin, np.cos, np.sin)):
        one = 1.0 if q % 2 == 0 else 0.0
        for name, data in (("fused", fused), ("replicated", plain)):
            err = np.abs(data[:, :, :, q] - fn(phase))[fin].max()
            print(f"plane {q} {name}: {err:.3g}")
            assert err <= 2e-6
            assert np.all(data[:, :, :, q][~fin] == one)       # NaN scrubbed to 1 / 0
            assert np.all(data[:, :, scr.ref_ind, q] == one)   # zero coefficients
        d = np.abs(fused[:, :, :, q] - plain[:, :, :, q]).max()
        print(f"plane {q} fused - replicated: {d:.3g}")
        assert d <= 2 * 2e-6
    assert np.any(fused[:, :, :, 1] != 0.0)
    if phase_soltab_name is None:
        # fused=False is the path of the parent: "auto" may pick either, and
        # both are within the tolerance of numpy
        auto = cube_of(tmp_path, path, "auto")
        assert (np.array_equal(auto, fused) or np.array_equal(auto, plain))


def test_evaluator_eval_tec(dev):
    """KLEvaluator.eval_tec_host / eval_tec_device: shapes, dtype, and the
    numbers against eval_host of the replicated, pre-scaled coefficients
    (another order of the same arithmetic: twice the tolerance) and numpy."""
    from ska_sdp_screen_fitting_amd.kl_screen import DEFAULT_FLAGS, KLEvaluator
    pp, x, y, tec, ph, p_tec, p_ph = reference(20, 20, 18)
    tec, ph = tec.copy(), ph.copy()   # writable: torch.from_numpy wants that
    ev = KLEvaluator(pp, 100.0, 5.0 / 3.0, x, y)
    h = ev.eval_tec_host(tec, K3, IDX3)
    assert h.shape == (T0, 3, A0, 4, 18, 20) and h.dtype == np.float32
    check(h, p_tec, DEFAULT_FLAGS, "eval_tec_host")
    rep = tec[:, IDX3] * K3[None, :, None, None]
    want = ev.eval_host(rep)
    assert want.shape == h.shape
    d = float(np.abs(h.astype(np.float64) - want).max())
    print(f"eval_tec_host - eval_host of replicated coefficients: {d:.3g}")
    assert d <= 2 * 2e-6
    hp = ev.eval_tec_host(tec, K3, IDX3, ph)
    check(hp, p_tec + p_ph, DEFAULT_FLAGS, "eval_tec_host with phase")
    d = float(np.abs(hp.astype(np.float64) - ev.eval_host(rep + ph[:, IDX3])).max())
    assert d <= 2 * 2e-6
    o = ev.eval_tec_device(up(dev, tec), K3, IDX3, up(dev, ph))
    assert o.shape == hp.shape and o.dtype == torch.float32 and o.is_cuda
    np.testing.assert_array_equal(bits(o.cpu().numpy()), bits(hp))
    with pytest.raises(ValueError):
        ev.eval_tec_host(tec, K3)                # F_tec = 2 needs tec_index
    with pytest.raises(ValueError):
        ev.eval_tec_host(tec, K3, [0, 2, 1])
    with pytest.raises(ValueError):
        ev.eval_tec_host(tec, K3, IDX3, ph[:, :1])
