"""Timing of the polarized-phase evaluation (sf_kl_eval_pol, kl_eval_pol.hip)
on one GPU, beside the only path to the same cube without it: sf_kl_eval (or
sf_kl_eval_gain) of the XX set into the final cube, the same of the YY set into
a scratch cube, and a device copy of planes 2 / 3 -- default options.

    python tools/eval_pol.py [--reps 7] [--out FILE]

Shapes: 256^2, D = 20, 50, 80, 128, phase-only (2 coefficient sets) and with
amplitudes (4 sets).  Every case writes the S slots through a ring of --ring
slots (default 16384: a 16 GiB cube, and as much scratch for the baseline); S
is a multiple of the ring, sized from a calibration launch so that a fused
launch takes >= 50 ms.  The baseline works ring by ring (evaluate XX, evaluate
YY, copy), so that it leaves the cube the fused call leaves: 3 S / ring
launches of a few ms each.  Per repetition every case runs once, interleaved
(drift hits all alike), each timed run after an untimed warm-up run of its own:
  fused     sf_kl_eval_pol, DEFAULT_FLAGS
  baseline  2 x sf_kl_eval[_gain] + plane copy per ring, DEFAULT_FLAGS
  gain      sf_kl_eval_gain alone at the same D and S (3 sets, one phase): the
            SIMD-budget reference, not a path to this cube
Reported per shape and case: median / min / max ms and the algorithmic TB/s
with bytes = output (16 N^2 per slot) + 8 D NSET per slot + Cpix once (8 D N^2)
-- the fused call's bytes for all three cases -- and its fraction of 8 TB/s.
The fused kernel WINS a shape when its median is below the baseline's median
by more than the baseline's max - min spread.  A ragged batch (S = 19) of each
shape is first checked against fp64 numpy on every 61st pixel at the tolerance
of tests/test_eval_pol.py (2e-6 max(1, A) on the fast sincos), and the
baseline's cube against the fused one (planes 0 / 1 and 2 / 3, same tolerance;
bit-equal above 60 directions).
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

ap = argparse.ArgumentParser()
ap.add_argument("--reps", type=int, default=7)
ap.add_argument("--target-ms", type=float, default=55.0,
                help="fused-launch time the slot count is sized for")
ap.add_argument("--ring", type=int, default=16384, help="ring slots (a multiple of 16)")
ap.add_argument("--dirs", default="20,50,80,128")
ap.add_argument("--out", default=None, help="also write the report here")
args = ap.parse_args()
if args.reps < 5:
    raise SystemExit("eval_pol.py: at least 5 timed launches")
if not torch.cuda.is_available():
    raise SystemExit("eval_pol.py needs a GPU: nothing is estimated")
dev = torch.device("cuda", 0)
ctx = get_context(0)
stream = torch.cuda.current_stream(dev)
ctx.set_stream(stream.cuda_stream)

HBM = 8e12
N = 256
P = N * N
DS = tuple(int(d) for d in args.dirs.split(","))
R = args.ring
cube = torch.empty((R, 4, P), dtype=torch.float32, device=dev)
scratch = torch.empty((R, 4, P), dtype=torch.float32, device=dev)
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


def dev_coef(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(dev)


def fused(px, py, ax, ay, S, out, ring):
    ctx.eval_pol(px, py, S, out, ring, ax, ay, DEFAULT_FLAGS)


def baseline(px, py, ax, ay, S, out, scr, ring):
    """What a user has without sf_kl_eval_pol, ring by ring."""
    for s0 in range(0, S, ring):
        n = min(ring, S - s0)
        sl = slice(s0, s0 + n)
        if ax is None:
            ctx.eval(px[sl], n, out, n, DEFAULT_FLAGS)
            ctx.eval(py[sl], n, scr, n, DEFAULT_FLAGS)
        else:
            ctx.eval_gain(px[sl], ax[sl], ay[sl], n, out, n, DEFAULT_FLAGS)
            ctx.eval_gain(py[sl], ax[sl], ay[sl], n, scr, n, DEFAULT_FLAGS)
        out[:n, 2:4].copy_(scr[:n, 2:4])


say(f"library {library_identity()}  ring {R} slots ({R * 16 * P / 2 ** 30:.0f} GiB, "
    f"as much scratch for the baseline)  reps {args.reps}  HBM {HBM / 1e12:.0f} TB/s  "
    f"flags {DEFAULT_FLAGS:#x}")
verdict = {}
for D in DS:
    pp, x, rng = geometry(D)
    if D > SF_MAX_DIR:
        ctx.set_piercepoints(pp)
    else:
        ctx.set_basis(pp)
    ctx.set_grid(x, x)
    pix = np.arange(0, P, 61)
    cpix = cpix_np(pp, x, pix)
    norm = np.abs(cpix).sum(axis=1).max()
    for gain in (False, True):
        nset = 4 if gain else 2
        tag = "phase + amplitudes" if gain else "phase-only"

        def draw(S):
            """Phases below ~300 rad, |log10 A| <= 0.3."""
            ph = [rng.uniform(-300.0 / norm, 300.0 / norm, (S, D)) for _ in range(2)]
            am = [rng.uniform(-0.3 / norm, 0.3 / norm, (S, D)) for _ in range(2)]
            return ph + (am if gain else [None, None])

        # ---- check a ragged batch against fp64 numpy, and the baseline against it
        Sc = 19
        h = draw(Sc)
        d = [None if a is None else dev_coef(a) for a in h]
        cube[:Sc].fill_(-7.0)
        fused(*d, Sc, cube, Sc)
        torch.cuda.synchronize()
        got_all = cube[:Sc].clone()
        got = got_all[..., torch.from_numpy(pix).to(dev)].cpu().numpy()
        phx, phy = h[0] @ cpix.T, h[1] @ cpix.T
        a_x = 10 ** (h[2] @ cpix.T) if gain else np.ones_like(phx)
        a_y = 10 ** (h[3] @ cpix.T) if gain else np.ones_like(phx)
        want = np.stack([a_x * np.cos(phx), a_x * np.sin(phx),
                         a_y * np.cos(phy), a_y * np.sin(phy)], axis=1)
        amax = max(1.0, a_x.max(), a_y.max())
        err = float(np.abs(got - want).max())
        baseline(*d, Sc, cube, scratch, Sc)
        torch.cuda.synchronize()
        dif = float((cube[:Sc] - got_all).abs().max())
        say(f"check D={D} {tag}: max |plane - numpy| {err:.3g}, |baseline - fused| "
            f"{dif:.3g} (tol {2e-6 * amax:.3g}), |phase| <= "
            f"{max(np.abs(phx).max(), np.abs(phy).max()):.0f} rad")
        if not (err <= 2e-6 * amax and dif <= 2e-6 * amax):
            raise SystemExit("eval_pol.py: output check failed")
        # ---- size S (a multiple of the ring) from a calibration launch
        d = [None if a is None else dev_coef(a) for a in draw(R)]
        fused(*d, R, cube, R)
        t0 = min(timed(lambda: fused(*d, R, cube, R)) for _ in range(3))
        laps = max(1, int(np.ceil(args.target_ms / t0)))
        S = laps * R
        d = [None if a is None else a.repeat(laps, 1) for a in d]
        kern = (f"{ctx.eval_kernel(DEFAULT_FLAGS, gain=gain)} / "
                f"{ctx.eval_contraction(DEFAULT_FLAGS, gain=gain)}")
        gd = d if gain else d[:2] + [dev_coef(a).repeat(laps, 1) for a in (
            rng.uniform(-0.3 / norm, 0.3 / norm, (R, D)),
            rng.uniform(-0.3 / norm, 0.3 / norm, (R, D)))]
        cases = {
            "fused": lambda: fused(*d, S, cube, R),
            "baseline": lambda: baseline(*d, S, cube, scratch, R),
            "gain": lambda: ctx.eval_gain(gd[0], gd[2], gd[3], S, cube, R, DEFAULT_FLAGS),
        }
        res = {name: [] for name in cases}
        for rep in range(args.reps + 1):
            for name, fn in cases.items():
                fn()  # untimed warm-up
                t = timed(fn)
                if rep:
                    res[name].append(t)
        say(f"--- 256^2 D={D} {tag} ({nset} sets)  S={S} slots through a ring of {R} "
            f"({S * 16 * P / 2 ** 30:.0f} GiB written)  baseline = 2 x {kern} + copy, "
            f"{3 * laps} launches")
        nbytes = S * 16 * P + S * 8 * D * nset + 8 * D * P
        med = {}
        for name in cases:
            t = res[name]
            med[name] = float(np.median(t))
            say(f"{name:8s} median {med[name]:8.3f} ms  min {min(t):8.3f}  max {max(t):8.3f}  "
                f"{nbytes / (med[name] * 1e-3) / 1e12:6.3f} TB/s "
                f"({nbytes / (med[name] * 1e-3) / HBM:.3f} of 8 TB/s)")
        spread = max(res["baseline"]) - min(res["baseline"])
        win = med["fused"] < med["baseline"] - spread
        verdict[(D, gain)] = win
        say(f"D={D} {tag}: fused {med['fused']:.3f} ms vs baseline {med['baseline']:.3f} ms "
            f"- spread {spread:.3f} ms: {'WIN' if win else 'no win'}  "
            f"(x{med['baseline'] / med['fused']:.3f}); fused / gain alone "
            f"x{med['fused'] / med['gain']:.3f}")
        del d, gd
say("fused beats the baseline by more than its spread at: " +
    (", ".join(f"D={D} {'gain' if g else 'phase'}" for (D, g), w in verdict.items() if w)
     or "no shape"))
say("it does not at: " +
    (", ".join(f"D={D} {'gain' if g else 'phase'}" for (D, g), w in verdict.items() if not w)
     or "no shape"))
if args.out:
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w", encoding="utf8") as fh:
        fh.write("\n".join(lines) + "\n")
