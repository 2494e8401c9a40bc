"""Timing of the wide evaluation kernel (kl_eval_wide.hip, D > 60) on one GPU,
beside the fp64 register tile at D = 60 in the same process.

    python tools/eval_wide.py [--reps 7] [--slots 51200] [--out FILE]

Per repetition every case runs once (interleaved, so drift hits all alike):
phase screens (DEFAULT_FLAGS) and gain screens at 256^2 with D = 80 and
D = 128 through sf_set_piercepoints, and D = 60 through sf_set_basis with
SF_OPT_EVAL_INT = 0 (the fp64 contraction on the register tile) as the
yardstick.  The output streams through a 16 GiB ring, far past the MALL.
Reported per case: median ms per launch, slots/s, bytes / time as a fraction
of 8 TB/s (bytes = S (16 N^2 + 8 D), gain S (16 N^2 + 24 D)), and the
contraction-bound expectation: the D = 60 fp64 fraction x 15 / k-steps.
A small batch is first checked against fp64 numpy (2e-6).
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
    SF_EVAL_FAST_SINCOS, SF_EVAL_NAN_SCRUB, SF_EVAL_NT_STORES, SF_MAX_DIR,
    SF_OPT_EVAL_INT, library_identity)

ap = argparse.ArgumentParser()
ap.add_argument("--reps", type=int, default=7)
ap.add_argument("--slots", type=int, default=51200, help="slots per launch")
ap.add_argument("--grid", type=int, default=256)
ap.add_argument("--out", default=None, help="also write the report here")
args = ap.parse_args()

if not torch.cuda.is_available():
    raise SystemExit("eval_wide.py needs a GPU: nothing is estimated")
dev = torch.device("cuda", 0)
ctx = get_context(0)
stream = torch.cuda.current_stream(dev)
ctx.set_stream(stream.cuda_stream)
FLAGS = SF_EVAL_NAN_SCRUB | SF_EVAL_FAST_SINCOS | SF_EVAL_NT_STORES
N, S = args.grid, args.slots
ring_bytes = 16 * 2 ** 30
ring = ring_bytes // (16 * N * N)
out = torch.empty(ring_bytes // 4, dtype=torch.float32,
                  device=dev)[: ring * 4 * N * N].view(ring, 4, N, N)
x = np.linspace(-2000, 2000, N)

cases = []  # (name, D, gain)
for D in (60, 80, 128):
    for gain in (False, True):
        cases.append((f"D={D} {'gain' if gain else 'phase'}", D, gain))
data = {}
for D in (60, 80, 128):
    rng = np.random.default_rng(D * 1000 + N)
    pp = np.stack([rng.uniform(-3000, 3000, D), rng.uniform(-3000, 3000, D),
                   np.zeros(D)], 1)
    # log10 amplitudes of a few tenths (|Cpix| is ~2e3 here)
    coef = [rng.normal(0, 0.01, (S, D)), rng.normal(0, 2e-5, (S, D)),
            rng.normal(0, 2e-5, (S, D))]
    data[D] = (pp, coef, [torch.from_numpy(c).to(dev) for c in coef])


def select(D):
    pp = data[D][0]
    if D > SF_MAX_DIR:
        ctx.set_piercepoints(pp)
    else:
        ctx.set_basis(pp)
    ctx.set_grid(x, x)


def run(D, gain, n, o, rg):
    c = data[D][2]
    if gain:
        ctx.eval_gain(c[0], c[1], c[2], n, o, rg, FLAGS)
    else:
        ctx.eval(c[0], n, o, rg, FLAGS)


lines = []


def say(s):
    print(s, flush=True)
    lines.append(s)


ctx.set_option(SF_OPT_EVAL_INT, 0)
try:
    say(f"library {library_identity()}  grid {N}^2  slots/launch {S}  "
        f"ring {ring} slots ({ring_bytes >> 30} GiB)  reps {args.reps}")
    kern = {}
    for name, D, gain in cases:
        select(D)
        kern[name] = f"{ctx.eval_kernel(FLAGS, gain)} / {ctx.eval_contraction(FLAGS, gain)}"
        # check a ragged batch against fp64 numpy
        Sc = 37
        o = torch.full((Sc, 4, N, N), -7.0, dtype=torch.float32, device=dev)
        run(D, gain, Sc, o, Sc)
        torch.cuda.synchronize()
        pp, coef, _ = data[D]
        gx, gy = np.meshgrid(x, x)
        d2 = ((pp[:, 0][None, :] - gx.reshape(-1, 1)) ** 2
              + (pp[:, 1][None, :] - gy.reshape(-1, 1)) ** 2 + pp[:, 2][None, :] ** 2)
        cpix = -((d2 / 100.0 ** 2) ** (5.0 / 6.0)) / 2.0
        ph = coef[0][:Sc] @ cpix.T
        ax = 10 ** (coef[1][:Sc] @ cpix.T) if gain else np.ones_like(ph)
        ay = 10 ** (coef[2][:Sc] @ cpix.T) if gain else ax
        want = np.stack([ax * np.cos(ph), ax * np.sin(ph), ay * np.cos(ph),
                         ay * np.sin(ph)], 1)
        err = np.abs(o.cpu().numpy().reshape(want.shape) - want).max()
        tol = 2e-6 * max(1.0, ax.max(), ay.max())
        say(f"check {name}: {kern[name]}  max|d| {err:.3g} (tol {tol:.3g})")
        if not err <= tol:
            raise SystemExit("eval_wide.py: output check failed")
    res = {}
    for rep in range(args.reps + 1):
        for name, D, gain in cases:
            select(D)
            run(D, gain, S, out, ring)  # untimed: re-warm after select()
            e0 = torch.cuda.Event(enable_timing=True)
            e1 = torch.cuda.Event(enable_timing=True)
            e0.record(stream)
            run(D, gain, S, out, ring)
            e1.record(stream)
            torch.cuda.synchronize()
            if rep:
                res.setdefault(name, []).append(e0.elapsed_time(e1))
finally:
    ctx.set_option(SF_OPT_EVAL_INT, -1)

frac = {}
for name, D, gain in cases:
    ms = float(np.median(res[name]))
    nbytes = S * (16 * N * N + (24 if gain else 8) * D)
    frac[name] = nbytes / (ms * 1e-3) / 8e12
for name, D, gain in cases:
    v = res[name]
    ms = float(np.median(v))
    ks = (D + 3) // 4
    base = frac[f"D=60 {'gain' if gain else 'phase'}"]
    say(f"{name:12s} {kern[name]:36s} median {ms:8.3f} ms  min {min(v):8.3f}  "
        f"max {max(v):8.3f}  {S / ms * 1e3:11.0f} slots/s  frac of 8 TB/s "
        f"{frac[name]:.3f}  contraction-bound expectation {base * 15 / ks:.3f}")
if args.out:
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w", encoding="utf8") as fh:
        fh.write("\n".join(lines) + "\n")
