"""Timing of the wide KL fit (kl_fit_wide.hip, 61..128 directions) on one GPU,
beside the <= 60 direction fit of the same shape in the same process.

    python tools/fit_wide.py [--reps 5] [--ant 64] [--time 64] [--freq 4] [--out FILE]

Phase screens, order 20, niter 2, adjusted orders, as KLScreen.fit runs them:
64 stations x 64 times x 4 freqs (16384 slots), 2 % flags, 0.5 % outliers, at
D = 60 (sf_set_basis, the mask-cached fit), D = 80 and D = 128
(sf_set_basis_wide, one workgroup per slot, no mask cache).  Per case one
warm-up call, then --reps timed sf_kl_fit calls: wall time around the call
and a stream synchronisation (sf_kl_fit returns with the fit complete, so it
is the call a user waits for; inputs stay on the device).  Reported: median /
min / max ms per call, slots/s, the share of fitted slots that carry a flagged
direction (each decomposes its own subset covariance above 60 directions) and
sf_get_fit_stats' count (wide: decompositions run over both passes; D = 60:
distinct masks decomposed, shared by the slots that carry them).
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
from ska_sdp_screen_fitting_amd._lib import SF_MAX_DIR, library_identity  # noqa: E402
from ska_sdp_screen_fitting_amd.stationscreen import station_orders  # noqa: E402
from ska_sdp_screen_fitting_amd.synthetic import make_solutions  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--reps", type=int, default=5)
ap.add_argument("--ant", type=int, default=64)
ap.add_argument("--time", type=int, default=64)
ap.add_argument("--freq", type=int, default=4)
ap.add_argument("--dirs", type=int, nargs="+", default=[60, 80, 128])
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


say(f"library {library_identity()}  {args.ant} stations x {args.time} times x "
    f"{args.freq} freqs  reps {args.reps}")
for D in args.dirs:
    s = make_solutions(n_ant=args.ant, n_time=args.time, n_freq=args.freq,
                       n_dir=D, seed=7000 + D, flag_frac=0.02, outlier_frac=0.005)
    T, F, A, _ = s.val.shape
    S = T * F * A
    pp, _, _ = geometry.piercepoints(s.dir_radec)
    ref = okl.reference_station(s.weight)
    st = station_orders(s.ant_pos, ref, 20)
    if D > SF_MAX_DIR:
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

    call()  # warm-up (scratch allocation, code load)
    # a sample of slots against the oracle (1e-8, orders and flags equal)
    got = coef.cpu().numpy()
    pick = [(0, 0, a) for a in range(A) if a != ref][:3] + [(T - 1, F - 1, A - 1)]
    r = okl.run_phase(s.val, s.weight, s.ant_pos, pp, ref, 20,
                      slot_filter=lambda t, f, a: (t, f, a) in pick)
    err = max(np.abs(got[p] - r["coef"][p]).max() for p in pick)
    ok = all(int(order[p]) == int(r["orders"][p]) for p in pick)
    say(f"check D={D}: {len(pick)} slots vs oracle max|d coef| {err:.3g}, orders "
        f"{'equal' if ok else 'DIFFER'}")
    if not (err <= 1e-8 * max(1.0, np.abs(r["coef"]).max()) and ok):
        raise SystemExit("fit_wide.py: output check failed")
    ms = []
    for _ in range(args.reps):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        call()
        ms.append((time.perf_counter() - t0) * 1e3)
    stats = ctx.fit_stats()
    fitted = S - args.time * args.freq  # the reference station is skipped
    med = float(np.median(ms))
    keep = np.ones(A, bool)
    keep[ref] = False
    flagged = float(((s.weight[:, :, keep] <= 0).any(-1)).mean())
    what = ("subset decompositions run (both passes)" if D > SF_MAX_DIR
            else "distinct masks decomposed (mask cache)")
    say(f"D={D:3d} {'wide' if D > SF_MAX_DIR else 'lane-per-direction'} fit: "
        f"median {med:9.2f} ms  min {min(ms):9.2f}  max {max(ms):9.2f}  "
        f"{S / med * 1e3:9.0f} slots/s  share of fitted slots with a flagged "
        f"direction {flagged:.3f}  {stats['n_masks']} {what} for {fitted} "
        f"fitted slots  general-path slots {stats['n_general']}")
if args.out:
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w", encoding="utf8") as fh:
        fh.write("\n".join(lines) + "\n")
