"""A/B of the fit pass layouts (SF_OPT_FIT_LEAN) on a bench workload, one
GPU: the fit of all slots, timed with HIP events, repeated and interleaved;
outputs (coefficients, residuals, weights, orders) compared bit for bit.

    python tools/fit_ab.py [--workload config4] [--reps 5] [--weight-scale 400]

--weight-scale multiplies the weights: with the workloads' weights of 1 the
reduced chi^2 is ~ 0.003 and the order walk of adjust_order re-fits no slot;
x 400 (1 / sigma^2 of the 0.05 rad noise) makes it re-fit about half of
them, up to three times per pass.  The line reports how many slots moved.
"""
import argparse
import os
import sys

import numpy as np
import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(REPO, "ska-sdp-screen-fitting_amd"))
sys.path.insert(0, REPO)
from bench import WORKLOADS  # noqa: E402
from ska_sdp_screen_fitting_amd import get_context  # noqa: E402
from ska_sdp_screen_fitting_amd._lib import SF_OPT_FIT_LEAN  # noqa: E402
from ska_sdp_screen_fitting_amd.distributed import setup_shard  # noqa: E402
from ska_sdp_screen_fitting_amd.synthetic import (FIELD_DEC_DEG, FIELD_RA_DEG,  # noqa: E402
                                                  FIELD_WIDTH_DEG, make_solutions)

ap = argparse.ArgumentParser()
ap.add_argument("--workload", default="config4")
ap.add_argument("--reps", type=int, default=5)
ap.add_argument("--times", type=int, default=0, help="time slots (0: the workload's)")
ap.add_argument("--weights", default="01", help="01: the workload's 0/1 weights; "
                "random: uniform(0.5, 1) weights (the general layout)")
ap.add_argument("--weight-scale", type=float, default=1.0,
                help="multiply the weights (400: the order walk re-fits)")
args = ap.parse_args()

A, T, F, D, N, cell = WORKLOADS[args.workload]
if args.times:
    T = args.times
sol = make_solutions(n_ant=A, n_time=T, n_freq=F, n_dir=D, ant_offset=0, n_ant_total=A)
if args.weights == "random":
    rng = np.random.default_rng(7)
    w = sol.weight
    sol.weight[...] = np.where(w > 0, rng.uniform(0.5, 1.0, w.shape), 0).astype(w.dtype)
if args.weight_scale != 1.0:
    sol.weight[...] = sol.weight * np.float32(args.weight_scale)
setup = setup_shard(sol, 0, A, FIELD_RA_DEG, FIELD_DEC_DEG, FIELD_WIDTH_DEG, cell,
                    device="cpu")
dev = torch.device("cuda", 0)
ctx = get_context(0)
stream = torch.cuda.current_stream(dev)
ctx.set_stream(stream.cuda_stream)
ctx.set_basis(setup["piercepoints"], 100, 5.0 / 3.0)
phase = torch.from_numpy(sol.val).to(dev)
weight = torch.from_numpy(sol.weight).to(dev)
refph = setup["ref_phase"].to(dev).contiguous()
S = T * F * A


def run(lean):
    ctx.set_option(SF_OPT_FIT_LEAN, lean)
    out = dict(coef=torch.empty_like(phase), resid=torch.empty_like(phase),
               w_out=torch.empty_like(weight),
               order_out=torch.empty((T, F, A), dtype=torch.int32, device=dev))
    e0 = torch.cuda.Event(enable_timing=True)
    e1 = torch.cuda.Event(enable_timing=True)
    e0.record(stream)
    ctx.fit(phase, weight, T, F, A, setup["st_order"], niter=2, nsigma=5.0,
            adjust_order=True, ref_ant=setup["ref_ant"], ref_phase=refph,
            ant_offset=setup["ant_offset"], **out)
    e1.record(stream)
    torch.cuda.synchronize()
    return e0.elapsed_time(e1), out


ms = {0: [], 1: []}
ref = {}
for rep in range(args.reps + 1):
    for lean in (0, 1):
        t, out = run(lean)
        if rep:
            ms[lean].append(t)
        else:
            ref[lean] = {k: v.cpu().numpy() for k, v in out.items()}
ctx.set_option(SF_OPT_FIT_LEAN, 1)
same = all(np.array_equal(ref[0][k].view(np.uint8), ref[1][k].view(np.uint8))
           for k in ref[0])
n_unfl = (ref[1]["w_out"] > 0).sum(axis=-1)
start = np.minimum(np.asarray(setup["st_order"])[None, None, :], n_unfl - 1)
moved = int(((ref[1]["order_out"] != start) & (ref[1]["order_out"] > 0)).sum())
print(f"{args.workload} S={S} D={D} weights={args.weights} x {args.weight_scale:g} "
      f"({moved} slots left their starting order): general "
      f"{np.median(ms[0]):.2f} ms, lean {np.median(ms[1]):.2f} ms "
      f"(x{np.median(ms[0]) / np.median(ms[1]):.2f}); outputs bit-identical: {same}",
      flush=True)
if not same:
    for k in ref[0]:
        a, b = ref[0][k], ref[1][k]
        print(k, "differs" if not np.array_equal(a.view(np.uint8), b.view(np.uint8))
              else "same", float(np.nanmax(np.abs(a.astype(np.float64) - b))))
    sys.exit(1)
