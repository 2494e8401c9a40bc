"""Timing of the tessellated value fill (sf_tess_fill_values, tess_values.hip)
on one GPU, beside the only other route to the same array: sf_tess_fill(phase =
0, amp_xx = values) into a four-plane scratch cube plus a device copy of plane
0 -- default options.

    python tools/tess_values.py [--reps 5] [--out FILE]

Shapes: 256^2, a Voronoi raster from tessellation_template on seeded
directions, D = 20 and 128, sigma = 0, 0.5, 2 and 6 px (fused) and 6.25 px
(split: gather, then the two passes).  Every case writes S slots ring by ring:
S / ring calls of --ring slots each (default 8192: a 2 GiB cube, 8 GiB of
scratch for the baseline), every call with ring_slots = its slot count, so
that every output byte of a call goes to a line of its own and the cube is
eight times the 256 MiB of MALL.  (One call of S slots through a shorter ring
rewrites each 4 KiB run S / ring times back to back from one wave, and the
caches absorb the overwrites: that measures no HBM write.)  S is a multiple of the ring, sized from a calibration run so that
a timed run of the new call takes >= 50 ms.  The baseline works the same way,
ring by ring (fill, copy), so that it leaves the cube the new call leaves.  Per
repetition every case runs once, interleaved (drift hits all alike), each timed
run after an untimed warm-up run of its own.  Reported per shape and case:
median / min / max ms and the algorithmic TB/s with bytes = 4 N^2 + 8 D per
slot -- the new call's bytes for both cases -- and its fraction of 8 TB/s.  The
new call WINS a shape when its median is below the baseline's median by more
than the baseline's max - min spread.  A ragged batch (S = 19) of each shape is
first checked: the new call against numpy (bit-equal unsmoothed) and against
plane 0 of the baseline (bit-equal where finite).

--sweep also times the unsmoothed fill for slots per work item x waves per
workgroup (SF_OPT_TESS_SLOTS x SF_OPT_TESS_WAVES), interleaved in the same way:
the source of the kernel's defaults.
"""
import argparse
import os
import sys

import numpy as np
import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(REPO, "ska-sdp-screen-fitting_amd"))
from ska_sdp_screen_fitting_amd import get_context  # noqa: E402
from ska_sdp_screen_fitting_amd._lib import (SF_EVAL_NAN_SCRUB, SF_EVAL_NT_STORES,  # noqa: E402
                                             SF_OPT_TESS_SLOTS, SF_OPT_TESS_WAVES,
                                             library_identity)
from ska_sdp_screen_fitting_amd.voronoi_screen import tessellation_template  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--reps", type=int, default=5)
ap.add_argument("--target-ms", type=float, default=55.0,
                help="launch time of the new call the slot count is sized for")
ap.add_argument("--ring", type=int, default=8192, help="ring slots")
ap.add_argument("--dirs", default="20,128")
ap.add_argument("--sigmas", default="0,0.5,2,6,6.25")
ap.add_argument("--sweep", action="store_true",
                help="also sweep slots per item x waves per workgroup (unsmoothed)")
ap.add_argument("--out", default=None, help="also write the report here")
args = ap.parse_args()
if args.reps < 5:
    raise SystemExit("tess_values.py: at least 5 timed launches")
if not torch.cuda.is_available():
    raise SystemExit("tess_values.py needs a GPU: nothing is estimated")
dev = torch.device("cuda", 0)
ctx = get_context(0)
stream = torch.cuda.current_stream(dev)
ctx.set_stream(stream.cuda_stream)

HBM = 8e12
N = 256
P = N * N
R = args.ring
FLAGS = SF_EVAL_NAN_SCRUB | SF_EVAL_NT_STORES
cube = torch.empty((R, P), dtype=torch.float32, device=dev)
scratch = torch.empty((R, 4, P), dtype=torch.float32, device=dev)
lines = []


def say(s):
    print(s, flush=True)
    lines.append(s)


def raster(D):
    """256^2 labels of D seeded directions in a 4 deg field."""
    rng = np.random.default_rng(D * 1000 + N)
    rad, dec, width = 126.0, 64.5, 4.0
    radec = np.stack([rad + rng.uniform(-1.8, 1.8, D) / np.cos(np.deg2rad(dec)),
                      dec + rng.uniform(-1.8, 1.8, D)], axis=1)
    lab = tessellation_template(radec, rad, dec, width, width / N)[0]
    assert lab.shape == (N, N) and lab.min() >= 1 and lab.max() <= D
    return lab, rng


def timed(fn):
    e0 = torch.cuda.Event(enable_timing=True)
    e1 = torch.cuda.Event(enable_timing=True)
    e0.record(stream)
    fn()
    e1.record(stream)
    torch.cuda.synchronize()
    return e0.elapsed_time(e1)


def new_call(lab, v, D, S, sigma):
    for s0 in range(0, S, R):  # ring by ring, ring_slots = the call's slots
        n = min(R, S - s0)
        ctx.tess_fill_values(lab, N, N, v[s0:s0 + n], D, n, cube, n, sigma, FLAGS)


def baseline(lab, v, zero, D, S, sigma):
    """What a user has without sf_tess_fill_values, ring by ring."""
    for s0 in range(0, S, R):
        n = min(R, S - s0)
        ctx.tess_fill(lab, N, N, zero[s0:s0 + n], D, n, scratch, n, amp_xx=v[s0:s0 + n],
                      smooth_pix=sigma, flags=SF_EVAL_NAN_SCRUB)
        cube[:n].copy_(scratch[:n, 0])


def report(name, t, nbytes):
    med = float(np.median(t))
    say(f"{name:24s} median {med:8.3f} ms  min {min(t):8.3f}  max {max(t):8.3f}  "
        f"{nbytes / (med * 1e-3) / 1e12:6.3f} TB/s ({nbytes / (med * 1e-3) / HBM:.3f} of 8 TB/s)")
    return med


say(f"library {library_identity()}  ring {R} slots ({R * 4 * P / 2 ** 30:.0f} GiB cube, "
    f"{R * 16 * P / 2 ** 30:.0f} GiB baseline scratch)  reps {args.reps}  "
    f"HBM {HBM / 1e12:.0f} TB/s  flags {FLAGS:#x}")
verdict = {}
for D in (int(d) for d in args.dirs.split(",")):
    lab_h, rng = raster(D)
    lab = torch.from_numpy(lab_h.astype(np.int32)).to(dev)
    # ---- check a ragged batch against numpy and against the baseline
    Sc = 19
    vh = rng.uniform(-40.0, 40.0, (Sc, D))
    vh[4, 3] = np.nan
    vc = torch.from_numpy(vh).to(dev)
    zc = torch.zeros_like(vc)
    want = vh[:, lab_h - 1].astype(np.float32)
    for sigma in (float(s) for s in args.sigmas.split(",")):
        cube[:Sc].fill_(-7.0)
        ctx.tess_fill_values(lab, N, N, vc, D, Sc, cube, Sc, sigma, 0)
        ctx.tess_fill(lab, N, N, zc, D, Sc, scratch, Sc, amp_xx=vc, smooth_pix=sigma, flags=0)
        torch.cuda.synchronize()
        got = cube[:Sc].cpu().numpy().reshape(Sc, N, N)
        base = scratch[:Sc, 0].cpu().numpy().reshape(Sc, N, N)
        fin = ~np.isnan(base)
        ok = (np.array_equal(np.isnan(got), ~fin)
              and np.array_equal(got.view(np.uint32)[fin], base.view(np.uint32)[fin]))
        if sigma == 0.0:
            ok = ok and np.array_equal(got.view(np.uint32)[fin], want.view(np.uint32)[fin])
        say(f"check D={D} sigma={sigma}: new call {'==' if ok else '!='} plane 0 of the baseline"
            f"{' == numpy' if sigma == 0.0 and ok else ''} ({int((~fin).sum())} NaN pixels)")
        if not ok:
            raise SystemExit("tess_values.py: output check failed")
    # ---- timings
    for sigma in (float(s) for s in args.sigmas.split(",")):
        split = int(4.0 * sigma + 0.5) > 24
        v = torch.from_numpy(rng.uniform(-40.0, 40.0, (R, D))).to(dev)
        new_call(lab, v, D, R, sigma)
        t0 = min(timed(lambda: new_call(lab, v, D, R, sigma)) for _ in range(3))
        laps = max(1, int(np.ceil(args.target_ms / t0)))
        S = laps * R
        v = v.repeat(laps, 1)
        zero = torch.zeros_like(v)
        cases = {"sf_tess_fill_values": lambda: new_call(lab, v, D, S, sigma),
                 "baseline": lambda: baseline(lab, v, zero, D, S, sigma)}
        if args.sweep and sigma == 0.0:
            def variant(slots, waves):
                def run():
                    ctx.set_option(SF_OPT_TESS_SLOTS, slots)
                    ctx.set_option(SF_OPT_TESS_WAVES, waves)
                    new_call(lab, v, D, S, sigma)
                    ctx.set_option(SF_OPT_TESS_SLOTS, 0)
                    ctx.set_option(SF_OPT_TESS_WAVES, 0)
                return run
            for slots in (8, 16, 32, 64):
                for waves in (4, 8, 16):
                    cases[f"  slots {slots:3d} waves {waves:2d}"] = variant(slots, waves)
        res = {name: [] for name in cases}
        for rep in range(args.reps + 1):
            for name, fn in cases.items():
                fn()  # untimed warm-up
                t = timed(fn)
                if rep:
                    res[name].append(t)
        say(f"--- 256^2 D={D} sigma={sigma} px (R={int(4.0 * sigma + 0.5)}"
            f"{', split path' if split else ''})  S={S} slots, {laps} call(s) of {R} per timed "
            f"run ({S * 4 * P / 2 ** 30:.0f} GiB written)")
        nbytes = S * (4 * P + 8 * D)
        med = {name: report(name, res[name], nbytes) for name in cases}
        spread = max(res["baseline"]) - min(res["baseline"])
        win = med["sf_tess_fill_values"] < med["baseline"] - spread
        verdict[(D, sigma)] = win
        say(f"D={D} sigma={sigma}: new {med['sf_tess_fill_values']:.3f} ms vs baseline "
            f"{med['baseline']:.3f} ms - spread {spread:.3f} ms: {'WIN' if win else 'no win'}  "
            f"(x{med['baseline'] / med['sf_tess_fill_values']:.3f})")
        del v, zero
say("sf_tess_fill_values beats the baseline by more than its spread at: " +
    (", ".join(f"D={D} sigma={s}" for (D, s), w in verdict.items() if w) or "no shape"))
say("it does not at: " +
    (", ".join(f"D={D} sigma={s}" for (D, s), w in verdict.items() if not w) or "no shape"))
if args.out:
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w", encoding="utf8") as fh:
        fh.write("\n".join(lines) + "\n")
