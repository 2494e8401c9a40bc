"""Timing of the fused TEC -> Jones evaluation (sf_kl_eval_tec, kl_tec.hip) on
one GPU, beside the path it replaces for KLTecScreen.write(aterm_type="gain"):
tec_to_phase_coef (the TEC coefficients replicated and scaled per channel, a
torch broadcast) + sf_kl_eval over T x F x A slots.

    python tools/eval_tec.py [--reps 7] [--out FILE]

Shapes: 256^2, D = 20, 50, 61, 80, 128 (61: the first D the parent path runs on
the wide kernel), F = 1, 8, 32 output channels of F_tec = 1 TEC frequency.
Both paths write the same [T][F][A][4][256][256] float32 cube into the same
buffer: there is no ring, so the cube has to fit the device.  T x A is sized from a calibration launch so that a fused launch takes >= 50 ms,
capped so that the cube stays below --max-gib (default: half of the free
device memory, at most 128 GiB); where the cap binds the report says so.
Per repetition every case runs once, interleaved (drift hits both alike),
each timed launch after an untimed warm-up launch of its own:
  fused   sf_set_tec_freqs once, then sf_kl_eval_tec, DEFAULT_FLAGS
  parent  tec_to_phase_coef + sf_kl_eval, DEFAULT_FLAGS, default SF_OPT_EVAL_INT
Reported per shape and case: median / min / max ms, algorithmic TB/s with
bytes = output + coefficients read (8 D per slot the kernel contracts: T A for
fused, T F A for parent) + Cpix once (8 D N^2), and its fraction of 8 TB/s.
The fused kernel WINS a shape when its median is below the parent's median by
more than the parent's max - min spread.  A ragged batch (T = 3, A = 7, with
phase coefficients) of each shape is first checked against fp64 numpy with the
tolerance of tests/test_tec_jones.py (2e-6 on the fast sincos) on every 61st
pixel.  The last lines are the table for kl_tec_screen.FUSED_AUTO_WINS.
"""
import argparse
import os
import sys

import numpy as np
import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(REPO, "ska-sdp-screen-fitting_amd"))
from ska_sdp_screen_fitting_amd import get_context  # noqa: E402
from ska_sdp_screen_fitting_amd._lib import SF_MAX_DIR, library_identity  # noqa: E402
from ska_sdp_screen_fitting_amd.kl_screen import DEFAULT_FLAGS  # noqa: E402
from ska_sdp_screen_fitting_amd.kl_tec_screen import (  # noqa: E402
    TEC_TO_PHASE, tec_to_phase_coef)

ap = argparse.ArgumentParser()
ap.add_argument("--reps", type=int, default=7)
ap.add_argument("--target-ms", type=float, default=55.0,
                help="fused-launch time the slot count is sized for")
ap.add_argument("--max-gib", type=float, default=None, help="cap of the cube")
ap.add_argument("--out", default=None, help="also write the report here")
args = ap.parse_args()
if args.reps < 5:
    raise SystemExit("eval_tec.py: at least 5 timed launches")
if not torch.cuda.is_available():
    raise SystemExit("eval_tec.py needs a GPU: nothing is estimated")
dev = torch.device("cuda", 0)
ctx = get_context(0)
stream = torch.cuda.current_stream(dev)
ctx.set_stream(stream.cuda_stream)

HBM = 8e12
N = 256
P = N * N
DS = (20, 50, 61, 80, 128)
FS = (1, 8, 32)
A = 64
free = torch.cuda.mem_get_info(dev)[0]
cap = min(free // 2, 128 * 2 ** 30) if args.max_gib is None else int(args.max_gib * 2 ** 30)
buf = torch.empty(cap // 4, dtype=torch.float32, device=dev)
lines = []


def say(s):
    print(s, flush=True)
    lines.append(s)


def geometry(D):
    rng = np.random.default_rng(D * 1000 + N)
    pp = np.stack([rng.uniform(-3000, 3000, D), rng.uniform(-3000, 3000, D),
                   np.zeros(D)], 1)
    return pp, np.linspace(-2000, 2000, N), rng


def cpix_np(pp, x, pix):
    gx, gy = np.meshgrid(x, x)
    gx, gy = gx.reshape(-1)[pix], gy.reshape(-1)[pix]
    d2 = ((pp[:, 0][None, :] - gx[:, None]) ** 2
          + (pp[:, 1][None, :] - gy[:, None]) ** 2 + pp[:, 2][None, :] ** 2)
    return -((d2 / 100.0 ** 2) ** (5.0 / 6.0)) / 2.0


def timed(fn):
    e0 = torch.cuda.Event(enable_timing=True)
    e1 = torch.cuda.Event(enable_timing=True)
    e0.record(stream)
    fn()
    e1.record(stream)
    torch.cuda.synchronize()
    return e0.elapsed_time(e1)


def freqs(F):
    return np.linspace(1.2e8, 1.8e8, F) if F > 1 else np.array([1.5e8])


say(f"library {library_identity()}  cube cap {cap / 2 ** 30:.0f} GiB of "
    f"{free / 2 ** 30:.0f} GiB free  reps {args.reps}  HBM {HBM / 1e12:.0f} TB/s  "
    f"flags {DEFAULT_FLAGS:#x}")
wins = {}
for D in DS:
    pp, x, rng = geometry(D)
    if D > SF_MAX_DIR:
        ctx.set_piercepoints(pp)
    else:
        ctx.set_basis(pp)
    ctx.set_grid(x, x)
    # TEC coefficients that keep |phase| below ~300 rad at 120 MHz
    pix = np.arange(0, P, 61)
    cpix = cpix_np(pp, x, pix)
    scale = 300.0 / (abs(TEC_TO_PHASE) / 1.2e8) / np.abs(cpix).sum(axis=1).max()
    for F in FS:
        nu = freqs(F)
        k = TEC_TO_PHASE / nu
        ctx.set_tec_freqs(k, None, 1)
        # ---- check a ragged batch against fp64 numpy
        Tc, Ac = 3, 7
        tc = rng.uniform(-scale, scale, (Tc, 1, Ac, D))
        pc = rng.uniform(-1.0, 1.0, (Tc, 1, Ac, D)) * 50.0 / np.abs(cpix).sum(axis=1).max()
        o = buf[: Tc * F * Ac * 4 * P]
        o.fill_(-7.0)
        ctx.eval_tec(torch.from_numpy(tc).to(dev), Tc, Ac, o,
                     torch.from_numpy(pc).to(dev), DEFAULT_FLAGS)
        torch.cuda.synchronize()
        got = o.view(Tc, F, Ac, 4, P)[..., torch.from_numpy(pix).to(dev)].cpu().numpy()
        phase = (np.einsum("tiad,pd->tap", tc, cpix)[:, None] * k[None, :, None, None]
                 + np.einsum("tiad,pd->tap", pc, cpix)[:, None])
        assert np.abs(phase).max() < 500.0
        err = max(float(np.abs(got[:, :, :, q] - fn(phase)).max())
                  for q, fn in enumerate((np.cos, np.sin, np.cos, np.sin)))
        say(f"check D={D} F={F}: max |plane - cos / sin| {err:.3g} (tol 2e-6), "
            f"|phase| <= {np.abs(phase).max():.0f} rad")
        if not err <= 2e-6:
            raise SystemExit("eval_tec.py: output check failed")
        # ---- size T from a calibration launch, under the memory cap
        T_cap = cap // (16 * P * F * A)
        T0 = max(1, min(T_cap, 4096 // (F * A) or 1))
        c0 = torch.from_numpy(rng.uniform(-scale, scale, (T0, 1, A, D))).to(dev)
        ctx.eval_tec(c0, T0, A, buf, None, DEFAULT_FLAGS)
        t0 = min(timed(lambda: ctx.eval_tec(c0, T0, A, buf, None, DEFAULT_FLAGS))
                 for _ in range(3))
        T = int(min(T_cap, max(T0, np.ceil(args.target_ms / t0 * T0))))
        tec = torch.from_numpy(rng.uniform(-scale, scale, (T, 1, A, D))).to(dev)
        S = T * F * A
        out = buf[: S * 4 * P]

        def fused():
            ctx.eval_tec(tec, T, A, out, None, DEFAULT_FLAGS)

        def parent():
            coef = tec_to_phase_coef(tec, nu, TEC_TO_PHASE, None).view(S, D)
            ctx.eval(coef, S, out, S, DEFAULT_FLAGS)

        cases = {"fused": fused, "parent": parent}
        kern = f"{ctx.eval_kernel(DEFAULT_FLAGS)} / {ctx.eval_contraction(DEFAULT_FLAGS)}"
        res = {name: [] for name in cases}
        for rep in range(args.reps + 1):
            for name, fn in cases.items():
                fn()  # untimed warm-up
                t = timed(fn)
                if rep:
                    res[name].append(t)
        say(f"--- 256^2 D={D} F={F}  T={T} A={A}: {T * A} contractions, {S} output slots, "
            f"cube {S * 16 * P / 2 ** 30:.1f} GiB{' (memory cap)' if T == T_cap else ''}  "
            f"parent = tec_to_phase_coef + {kern}")
        med = {}
        for name in cases:
            t = res[name]
            med[name] = float(np.median(t))
            contracted = T * A if name == "fused" else S
            nbytes = S * 16 * P + contracted * 8 * D + 8 * D * P
            say(f"{name:7s} median {med[name]:8.3f} ms  min {min(t):8.3f}  max {max(t):8.3f}  "
                f"{nbytes / (med[name] * 1e-3) / 1e12:6.3f} TB/s "
                f"({nbytes / (med[name] * 1e-3) / HBM:.3f} of 8 TB/s)")
        spread = max(res["parent"]) - min(res["parent"])
        win = med["fused"] < med["parent"] - spread
        wins[(D, F)] = win
        say(f"D={D} F={F}: fused {med['fused']:.3f} ms vs parent {med['parent']:.3f} ms - "
            f"spread {spread:.3f} ms: {'WIN' if win else 'no win'}  "
            f"(x{med['parent'] / med['fused']:.3f})")
        del tec, c0
say(f"FUSED_AUTO_D = {DS}")
say(f"FUSED_AUTO_F = {FS}")
say("FUSED_AUTO_WINS = (" + ",\n                   ".join(
    "(" + ", ".join(str(wins[(D, F)]) for F in FS) + ")" for D in DS) + ")")
if args.out:
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w", encoding="utf8") as fh:
        fh.write("\n".join(lines) + "\n")
