"""What the constraint check costs the host stepper: lock-step rounds of idaens_stream on linear_dense (n = 512, a few hundred
systems) with the constraint vector unset (idahip_post_newton) and set to all zeros (idahip_post_newton_constr: the check runs in
every attempt and always passes, so both ensembles take the same steps), alternating in one process on one device. Also the two
vector kernels alone, by the kernel-class timer. One JSON object per line on stdout; --json also writes them to a file.

    python tools/constr_ab.py [--n 512] [--batch 256] [--rounds 100] [--runs 3] [--json profiles/constr_ab.json]
"""
import argparse
import json
import os
import socket
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "rust-ida_amd"))
import idahip  # noqa: E402
from idahip import problems  # noqa: E402

LINES = []


def emit(rec):
    LINES.append(rec)
    print(json.dumps(rec), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=512)
    ap.add_argument("--batch", type=int, default=256)
    ap.add_argument("--rounds", type=int, default=100)
    ap.add_argument("--runs", type=int, default=3)
    ap.add_argument("--json", default=None)
    a = ap.parse_args()
    p = problems.linear_dense(n=a.n, batch=a.batch)
    touts = p["touts"]
    side = {}
    for mode in ("unset", "zeros"):
        ctx = problems.make_ctx(p)
        if mode == "zeros":
            ctx.set_constraints(np.zeros(a.n))
        ens = idahip.Ensemble(ctx, p["yy0"], p["yp0"])
        ens.set_device_controller(0)
        assert ens.device_controller_active() == 0
        ens.stream(touts, 60, stagger_rounds=30)  # spin-up: the systems spread over the phases of an integration
        side[mode] = (ctx, ens)
    sec = {"unset": [], "zeros": []}
    vec_ms = {"unset": [], "zeros": []}
    for _ in range(a.runs):
        for mode in ("unset", "zeros"):
            ctx, ens = side[mode]
            ctx.H.idahip_sync(ctx.h)
            t0 = time.perf_counter()
            ens.stream(touts, a.rounds)
            ctx.H.idahip_sync(ctx.h)
            sec[mode].append((time.perf_counter() - t0) / a.rounds)
    # the two kernels alone on the state the streams left: device time of one call over the whole batch
    for mode in ("unset", "zeros"):
        ctx, ens = side[mode]
        cj, kk = np.full(a.batch, 100.0), np.full(a.batch, 2, dtype=np.int32)
        for r in range(a.runs + 1):
            ctx.timing(1)
            ctx.timing_reset()
            if mode == "zeros":
                ctx.post_newton_constr(cj, kk, 0.33, 1)
            else:
                ctx.post_newton(cj, kk)
            if r > 0:
                vec_ms[mode].append(ctx.timing_get()["vector"]["ms"])
            ctx.timing(0)
    same = all(np.array_equal(side["unset"][1].counter(k), side["zeros"][1].counter(k)) for k in ("nst", "nni", "n_attempts", "ncfn"))
    rec = {"case": "host_stepper_rounds", "kind": "linear_dense", "n": a.n, "batch": a.batch, "rounds": a.rounds, "runs": a.runs,
           "host": socket.gethostname(), "same_counters": bool(same)}
    for mode in ("unset", "zeros"):
        rec[mode + "_ms_per_round"] = [round(1e3 * v, 4) for v in sec[mode]]
        rec[mode + "_ms_per_round_median"] = round(1e3 * float(np.median(sec[mode])), 4)
        rec[mode + "_post_newton_kernel_ms"] = round(float(np.median(vec_ms[mode])), 4)
    rec["zeros_over_unset"] = round(rec["zeros_ms_per_round_median"] / rec["unset_ms_per_round_median"], 4)
    emit(rec)
    for ctx, ens in side.values():
        ens.close()
        ctx.close()
    if a.json:
        with open(a.json, "w") as f:
            json.dump(LINES, f, indent=1)


if __name__ == "__main__":
    main()
