"""Timing of the wide KL fit (kl_fit_wide.hip, 61..128 directions) on one GPU,
beside the <= 60 direction fit of the same shape in the same process.

    python tools/fit_wide.py [--reps 5] [--ant 64] [--time 64] [--freq 4]
                             [--workloads random structured] [--out FILE]

Phase screens, order 20, niter 2, adjusted orders, as KLScreen.fit runs them:
64 stations x 64 times x 4 freqs (16384 slots) at D = 60 (sf_set_basis, the
mask-cached fit), D = 80 and D = 128 (sf_set_basis_wide, one workgroup per
slot), on two workloads:

  random      2 % flags drawn per (time, freq, station, direction), 0.5 %
              outliers (seeds 7000 + D);
  structured  every station has 1..3 directions flagged at all times and
              frequencies (one mask per fitted station: 63 masks), 0.5 %
              outliers.

Above 60 directions every case runs with the mask cache on and off
(SF_OPT_FIT_WIDE_CACHE; a library that does not know the option runs once,
marked "n/a").  Per case one warm-up call, then --reps timed sf_kl_fit calls:
wall time around the call and a stream synchronisation (sf_kl_fit returns
with the fit complete, so it is the call a user waits for; inputs stay on the
device).  Reported: median / min / max ms per call, slots/s, the share of
fitted slots that carry a flagged direction and sf_get_fit_stats' count
(wide: subset decompositions run over both passes -- pool entries built plus
the ones slots ran for themselves; D = 60: distinct masks decomposed).
"""
import argparse
import os
import sys
import time

import numpy as np
import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(REPO, "ska-sdp-screen-fitting_amd"))
sys.path.insert(0, REPO)
from oracle import kl as okl  # noqa: E402
from ska_sdp_screen_fitting_amd import geometry, get_context  # noqa: E402
from ska_sdp_screen_fitting_amd._lib import (SF_MAX_DIR, ScreenFitError,  # noqa: E402
                                             library_identity)
from ska_sdp_screen_fitting_amd.stationscreen import station_orders  # noqa: E402
from ska_sdp_screen_fitting_amd.synthetic import make_solutions  # noqa: E402

SF_OPT_FIT_WIDE_CACHE = 19

ap = argparse.ArgumentParser()
ap.add_argument("--reps", type=int, default=5)
ap.add_argument("--ant", type=int, default=64)
ap.add_argument("--time", type=int, default=64)
ap.add_argument("--freq", type=int, default=4)
ap.add_argument("--dirs", type=int, nargs="+", default=[60, 80, 128])
ap.add_argument("--workloads", nargs="+", default=["random", "structured"],
                choices=["random", "structured"])
ap.add_argument("--out", default=None, help="also write the report here")
args = ap.parse_args()

if not torch.cuda.is_available():
    raise SystemExit("fit_wide.py needs a GPU: nothing is estimated")
dev = torch.device("cuda", 0)
ctx = get_context(0)
stream = torch.cuda.current_stream(dev)
ctx.set_stream(stream.cuda_stream)
lines = []


def say(s):
    print(s, flush=True)
    lines.append(s)


def has_cache_option():
    try:
        ctx.set_option(SF_OPT_FIT_WIDE_CACHE, 1)
        return True
    except ScreenFitError:
        return False


def workload(name, D):
    if name == "random":
        return make_solutions(n_ant=args.ant, n_time=args.time, n_freq=args.freq,
                              n_dir=D, seed=7000 + D, flag_frac=0.02,
                              outlier_frac=0.005)
    s = make_solutions(n_ant=args.ant, n_time=args.time, n_freq=args.freq,
                       n_dir=D, seed=7000 + D, flag_frac=0.0, outlier_frac=0.005)
    rng = np.random.default_rng(8000 + D)
    for a in range(args.ant):
        s.weight[:, :, a, rng.choice(D, 1 + a % 3, replace=False)] = 0.0
    return s


CACHE_OPTION = has_cache_option()
say(f"library {library_identity()}  {args.ant} stations x {args.time} times x "
    f"{args.freq} freqs  reps {args.reps}  SF_OPT_FIT_WIDE_CACHE "
    f"{'known' if CACHE_OPTION else 'unknown to this library'}")
for wl in args.workloads:
    for D in args.dirs:
        s = workload(wl, D)
        T, F, A, _ = s.val.shape
        S = T * F * A
        pp, _, _ = geometry.piercepoints(s.dir_radec)
        ref = okl.reference_station(s.weight)
        st = station_orders(s.ant_pos, ref, 20)
        wide = D > SF_MAX_DIR
        if wide:
            ctx.set_basis_wide(pp)
        else:
            ctx.set_basis(pp)
        ph = torch.from_numpy(s.val).to(dev)
        wt = torch.from_numpy(s.weight).to(dev)
        coef, resid = torch.empty_like(ph), torch.empty_like(ph)
        w_out = torch.empty_like(wt)
        order = torch.empty((T, F, A), dtype=torch.int32, device=dev)

        def call():
            ctx.fit(ph, wt, T, F, A, st, ref_ant=ref, coef=coef, resid=resid,
                    w_out=w_out, order_out=order)
            stream.synchronize()

        # a sample of slots against the oracle (1e-8, orders and flags equal)
        pick = [(0, 0, a) for a in range(A) if a != ref][:3] + [(T - 1, F - 1, A - 1)]
        r = okl.run_phase(s.val, s.weight, s.ant_pos, pp, ref, 20,
                          slot_filter=lambda t, f, a: (t, f, a) in pick)
        fitted = S - args.time * args.freq  # the reference station is skipped
        keep = np.ones(A, bool)
        keep[ref] = False
        flagged = float(((s.weight[:, :, keep] <= 0).any(-1)).mean())
        first = None
        for cache in ([1, 0] if wide and CACHE_OPTION else [None]):
            if cache is not None:
                ctx.set_option(SF_OPT_FIT_WIDE_CACHE, cache)
            call()  # warm-up (scratch allocation, code load)
            got = coef.cpu().numpy()
            err = max(np.abs(got[p] - r["coef"][p]).max() for p in pick)
            ok = all(int(order[p]) == int(r["orders"][p]) for p in pick)
            if not (err <= 1e-8 * max(1.0, np.abs(r["coef"]).max()) and ok):
                raise SystemExit(f"fit_wide.py: output check failed ({wl} D={D} "
                                 f"cache {cache}: max|d coef| {err:.3g})")
            # cache on and off: the same bytes
            outs = [x.cpu().numpy().copy() for x in (coef, resid, w_out, order)]
            if first is None:
                first = outs
            elif not all(np.array_equal(a.view(np.uint8), b.view(np.uint8))
                         for a, b in zip(first, outs)):
                raise SystemExit(f"fit_wide.py: cache on / off differ ({wl} D={D})")
            ms = []
            for _ in range(args.reps):
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                call()
                ms.append((time.perf_counter() - t0) * 1e3)
            stats = ctx.fit_stats()
            med = float(np.median(ms))
            what = ("subset decompositions run (both passes)" if wide
                    else "distinct masks decomposed (mask cache)")
            tag = {None: "n/a", 1: "on ", 0: "off"}[cache] if wide else "-  "
            say(f"{wl:10s} D={D:3d} {'wide' if wide else 'lane-per-direction'} fit "
                f"cache {tag}: median {med:9.2f} ms  min {min(ms):9.2f}  "
                f"max {max(ms):9.2f}  {S / med * 1e3:9.0f} slots/s  check vs "
                f"oracle max|d coef| {err:.3g}  share of fitted slots with a "
                f"flagged direction {flagged:.3f}  {stats['n_masks']} {what} for "
                f"{fitted} fitted slots  general-path slots {stats['n_general']}")
        if wide and CACHE_OPTION:
            ctx.set_option(SF_OPT_FIT_WIDE_CACHE, 1)
if args.out:
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w", encoding="utf8") as fh:
        fh.write("\n".join(lines) + "\n")
