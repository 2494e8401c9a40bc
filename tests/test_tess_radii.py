"""Every fused smoothing radius of the tessellated fill (R = 1..24, R =
int(4 sigma + 0.5)) through every kernel that serves it: the interior-lookup
and wide-tile kernels with the compiled and the run-time radius, two and four
planes, the 65- and the 129-entry LDS tables -- bit for bit against the fused
16 x 16 tile kernel (SF_OPT_TESS_TILE), and one fill per radius against the
oracle (oracle/voronoi.py: scipy's gaussian_filter of the gather), which none
of the kernels shares code with.  R = 25 is the first radius of the split path
(gather, then sf_smooth).  Needs an MI355X: every test is marked ``gpu``.
"""

import functools

import numpy as np
import pytest

from oracle import voronoi as ov

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

SCRUB = 1       # SF_EVAL_NAN_SCRUB
BE = 1 << 10    # SF_EVAL_BIG_ENDIAN

S = 35  # a ragged last chunk for the 8-slot and the 32-slot work items
# (40, 12): float4 stores, a tile shorter than the halo (the reflection wraps
# more than once at R = 24); (21, 9): the scalar store tail
SHAPES = [(40, 12), (21, 9)]
DIRS = [11, 70]  # table capacities 65 and 129
# radii at the edges of the compiled sets (8 | 9, 11 | 12, 24) with every flag
ALL_FLAGS = (1, 8, 9, 11, 12, 24)


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


@functools.lru_cache(maxsize=None)
def inputs(nx, ny, D):
    """Noise labels (most pixels are cell boundaries) beside a constant
    quadrant (interior pixels), one NaN phase and one NaN amplitude."""
    rng = np.random.default_rng(nx * 7 + ny + 1000 * D)
    lab = rng.integers(1, D + 1, size=(ny, nx)).astype(np.int32)
    lab[: ny // 2, : nx // 2] = 3
    ph = rng.uniform(-9.0, 9.0, size=(S, D))
    ph[4, 3] = np.nan
    ax = 10.0 ** rng.normal(0.0, 0.3, size=(S, D))
    ax[S - 1, 2] = np.nan
    ay = 10.0 ** rng.normal(0.0, 0.3, size=(S, D))
    for a in (lab, ph, ax, ay):
        a.setflags(write=False)
    return lab, ph, ax, ay


@functools.lru_cache(maxsize=None)
def device_inputs(nx, ny, D):
    return tuple(torch.from_numpy(a.copy()).to("cuda:0") for a in inputs(nx, ny, D))


@functools.lru_cache(maxsize=None)
def gathered(nx, ny, D):
    """The oracle's unsmoothed four-plane cube, shared by the anchors."""
    lab, ph, ax, ay = inputs(nx, ny, D)
    want = ov.gather_planes(lab, ph, ax, ay)
    want.setflags(write=False)
    return want


def scrub(planes):
    out = planes.copy()
    for p in range(4):
        v = out[..., p, :, :]
        v[np.isnan(v)] = 0.0 if p % 2 else 1.0
    return out


def fill(ctx, nx, ny, D, yy, sigma, flags, tile=0, box=-1):
    from ska_sdp_screen_fitting_amd._lib import SF_OPT_TESS_BOX, SF_OPT_TESS_TILE
    lab, ph, ax, ay = device_inputs(nx, ny, D)
    out = torch.full((S, 4, ny, nx), -5.0, dtype=torch.float32, device=lab.device)
    ctx.set_option(SF_OPT_TESS_TILE, tile)
    ctx.set_option(SF_OPT_TESS_BOX, box)
    try:
        ctx.tess_fill(lab, nx, ny, ph, D, S, out, amp_xx=ax, amp_yy=ay if yy else None,
                      smooth_pix=sigma, flags=flags)
        torch.cuda.synchronize()
    finally:
        ctx.set_option(SF_OPT_TESS_TILE, 0)
        ctx.set_option(SF_OPT_TESS_BOX, -1)
    return out.cpu().numpy()


def check_oracle(ctx, nx, ny, D, sigma, got_scrubbed):
    """1e-6 x max(1, |A|) from scipy, and scipy's NaN pattern before the
    scrub."""
    want = ov.smooth(gathered(nx, ny, D), sigma)
    nan = np.isnan(want)
    assert nan.any() and not nan.all()
    raw = fill(ctx, nx, ny, D, True, sigma, 0)
    assert np.array_equal(np.isnan(raw), nan)
    want = scrub(want)
    err = np.abs(got_scrubbed - want) / np.maximum(1.0, np.abs(want))
    print(f"D={D} {nx}x{ny} sigma={sigma}: max scaled error {err.max():.3g}")
    assert err.max() <= 1e-6


@pytest.mark.parametrize("R", range(1, 25))
def test_every_fused_radius(ctx, dev, R):
    """Interior lookups (SF_OPT_TESS_BOX = 1) and the wide tile (0) write the
    bits of the 16 x 16 tile kernel, whichever instantiation the radius, the
    plane count and the table capacity select; the four-plane scrubbed fill
    also matches the oracle."""
    sigma = R / 4.0  # exact in binary: int(4 sigma + 0.5) == R
    assert int(4 * sigma + 0.5) == R
    flag_sets = (SCRUB, SCRUB | BE, 0) if R in ALL_FLAGS else (SCRUB,)
    for D, (nx, ny) in [(D, s) for D in DIRS for s in SHAPES]:
        for yy in (False, True):
            for flags in flag_sets:
                ref = fill(ctx, nx, ny, D, yy, sigma, flags, tile=1).view(np.uint32)
                assert not (ref == np.float32(-5.0).view(np.uint32)).any()
                for box in (0, 1):
                    got = fill(ctx, nx, ny, D, yy, sigma, flags, box=box).view(np.uint32)
                    assert np.array_equal(ref, got), (D, nx, ny, yy, flags, box,
                                                      int((ref != got).sum()))
                if yy and flags == SCRUB:
                    check_oracle(ctx, nx, ny, D, sigma, ref.view(np.float32))


def test_first_split_radius(ctx, dev):
    """R = 25 > the fused limit: gather, then the two passes of sf_smooth."""
    D, sigma = 70, 6.25
    assert int(4 * sigma + 0.5) == 25
    for nx, ny in SHAPES:
        check_oracle(ctx, nx, ny, D, sigma, fill(ctx, nx, ny, D, True, sigma, SCRUB))
