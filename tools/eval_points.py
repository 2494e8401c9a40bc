"""Timing of the point-sampling kernel (kl_points.hip: sf_kl_eval_points,
sf_kl_eval_point_values) on one GPU, beside sf_kl_eval of the 17^2 cube on the
same slots in the same process.

    python tools/eval_points.py [--reps 5] [--slots 1048576] [--out FILE]

Seeded coefficients (generated on the device), S slots per launch, shapes
(D, P) = (20, 20), (50, 50), (128, 128), (20, 289); per shape three modes:
Jones planes with the fast sincos, gain planes, values.  Each case is warmed
up once and then timed ``reps`` times with device events; for D = 20 the
17^2 grid (289 pixels) is evaluated with sf_kl_eval on the same slots,
alternating with the point kernel repetition by repetition, since the cube is
the only other way to the numbers at the patches.  Reported per case: median /
min / max ms per launch, the algorithmic bytes S (8 D n_coef + 16 P) (8 P for
values; n_coef = 3 for gain) and their share of 8 TB/s (HBM bandwidth is the
bound: the kernel reads each coefficient and writes each output once).  A
small batch of every case is first checked against fp64 numpy.
"""
import argparse
import os
import sys

import numpy as np
import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(REPO, "ska-sdp-screen-fitting_amd"))
from ska_sdp_screen_fitting_amd import get_context  # noqa: E402
from ska_sdp_screen_fitting_amd._lib import (  # noqa: E402
    SF_EVAL_FAST_SINCOS, SF_EVAL_NAN_SCRUB, SF_EVAL_NT_STORES, library_identity)

ap = argparse.ArgumentParser()
ap.add_argument("--reps", type=int, default=5)
ap.add_argument("--slots", type=int, default=1 << 20, help="slots per launch")
ap.add_argument("--out", default=None, help="also write the report here")
args = ap.parse_args()

if not torch.cuda.is_available():
    raise SystemExit("eval_points.py needs a GPU: nothing is estimated")
dev = torch.device("cuda", 0)
ctx = get_context(0)
stream = torch.cuda.current_stream(dev)
ctx.set_stream(stream.cuda_stream)
PT_FLAGS = SF_EVAL_NAN_SCRUB | SF_EVAL_FAST_SINCOS
CUBE_FLAGS = PT_FLAGS | SF_EVAL_NT_STORES
S = args.slots
SHAPES = ((20, 20), (50, 50), (128, 128), (20, 289))
MODES = ("planes", "gain", "values")
GRID = 17
lines = []


def say(s):
    print(s, flush=True)
    lines.append(s)


def geometry(D, P):
    rng = np.random.default_rng(D * 1000 + P)
    pp = np.stack([rng.uniform(-3000, 3000, D), rng.uniform(-3000, 3000, D),
                   np.zeros(D)], 1)
    if P == GRID * GRID:
        x = np.linspace(-2000, 2000, GRID)
        gx, gy = np.meshgrid(x, x)
        xy = np.stack([gx.ravel(), gy.ravel()], 1)
    else:
        xy = rng.uniform(-3000, 3000, (P, 2))
    return pp, xy


def coefficients(D):
    """Phase coefficients of ~0.01 rad and log10-amplitude coefficients of
    2e-5 (|Cpix| is ~2e3 here), seeded, made on the device."""
    gen = torch.Generator(device=dev).manual_seed(D)
    return [torch.randn((S, D), generator=gen, dtype=torch.float64, device=dev) * sc
            for sc in (0.01, 2e-5, 2e-5)]


def run(mode, c, out):
    if mode == "values":
        ctx.eval_point_values(c[0], S, out)
    elif mode == "gain":
        ctx.eval_points(c[0], S, out, c[1], c[2], PT_FLAGS)
    else:
        ctx.eval_points(c[0], S, out, flags=PT_FLAGS)


def timed(fn):
    e0 = torch.cuda.Event(enable_timing=True)
    e1 = torch.cuda.Event(enable_timing=True)
    e0.record(stream)
    fn()
    e1.record(stream)
    torch.cuda.synchronize()
    return e0.elapsed_time(e1)


def check(mode, pp, xy, c, out):
    n = 37
    d2 = ((pp[:, 0][None, :] - xy[:, 0:1]) ** 2 + (pp[:, 1][None, :] - xy[:, 1:2]) ** 2
          + pp[:, 2][None, :] ** 2)
    cpix = -((d2 / 100.0 ** 2) ** (5.0 / 6.0)) / 2.0
    h = [t[:n].cpu().numpy() for t in c]
    v = h[0] @ cpix.T
    got = out.reshape(S, -1)[:n].cpu().numpy()
    if mode == "values":
        err, tol = np.abs(got - v).max(), 1e-9 * max(1.0, np.abs(v).max())
    else:
        ax = 10 ** (h[1] @ cpix.T) if mode == "gain" else np.ones_like(v)
        ay = 10 ** (h[2] @ cpix.T) if mode == "gain" else ax
        want = np.stack([ax * np.cos(v), ax * np.sin(v), ay * np.cos(v), ay * np.sin(v)], 1)
        err = np.abs(got.reshape(want.shape) - want).max()
        tol = 2e-6 * max(1.0, ax.max(), ay.max())
    if not err <= tol:
        raise SystemExit(f"eval_points.py: output check failed ({mode}: {err} > {tol})")
    return err


say(f"library {library_identity()}  slots/launch {S}  reps {args.reps}  "
    f"flags: points NAN_SCRUB|FAST_SINCOS, cube +NT_STORES")
res, cube_ms = {}, {}
for D, P in SHAPES:
    pp, xy = geometry(D, P)
    c = coefficients(D)
    ctx.set_basis(pp) if D <= 60 else ctx.set_piercepoints(pp)
    ctx.set_points(xy)
    planes = torch.empty((S, 4, P), dtype=torch.float32, device=dev)
    values = torch.empty((S, P), dtype=torch.float64, device=dev)
    cube = None
    if D == 20:
        x = np.linspace(-2000, 2000, GRID)
        ctx.set_grid(x, x)
        cube = torch.empty((S, 4, GRID, GRID), dtype=torch.float32, device=dev)
        ctx.eval(c[0], S, cube, S, CUBE_FLAGS)  # warm-up
        torch.cuda.synchronize()
    for mode in MODES:
        out = values if mode == "values" else planes
        run(mode, c, out)  # warm-up
        torch.cuda.synchronize()
        err = check(mode, pp, xy, c, out)
        ms, cms = [], []
        for _ in range(args.reps):
            ms.append(timed(lambda: run(mode, c, out)))
            if cube is not None and mode == "planes":
                cms.append(timed(lambda: ctx.eval(c[0], S, cube, S, CUBE_FLAGS)))
        n_coef = 3 if mode == "gain" else 1
        nbytes = S * (8 * D * n_coef + (8 if mode == "values" else 16) * P)
        med = float(np.median(ms))
        res[(D, P, mode)] = med
        say(f"D={D:3d} P={P:3d} {mode:6s} median {med:8.3f} ms  min {min(ms):8.3f}  "
            f"max {max(ms):8.3f}  bytes {nbytes / 1e6:9.1f} MB  frac of 8 TB/s "
            f"{nbytes / (med * 1e-3) / 8e12:.3f}  check max|d| {err:.2g}")
        if cms:
            cmed = float(np.median(cms))
            cube_ms[(D, P)] = cmed
            cb = S * (8 * D + 16 * GRID * GRID)
            say(f"D={D:3d} sf_kl_eval 17^2 cube ({ctx.eval_kernel(CUBE_FLAGS)}) median "
                f"{cmed:8.3f} ms  min {min(cms):8.3f}  max {max(cms):8.3f}  bytes "
                f"{cb / 1e6:9.1f} MB  frac of 8 TB/s {cb / (cmed * 1e-3) / 8e12:.3f}")
    del planes, values, cube, c
    torch.cuda.empty_cache()
t_pt, t_cube = res[(20, 20, "planes")], cube_ms[(20, 20)]
say(f"D=20 P=20 planes vs the 17^2 cube of the same slots: {t_pt:.3f} ms vs "
    f"{t_cube:.3f} ms, ratio {t_cube / t_pt:.2f} (byte ratio 4784 : 480 = 9.97; "
    f"less than one third of the cube's time: {'yes' if 3 * t_pt < t_cube else 'NO'})")
if args.out:
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w", encoding="utf8") as fh:
        fh.write("\n".join(lines) + "\n")
