"""Analytic against difference-quotient (DQ) Jacobians in one process, on one device: per-setup times of every problem kind
(idahip_nls_lsetup against idahip_nls_lsetup_dq on the same state, alternating), the linear-dense DQ kernel's fp64 rate, and the
heat band stream (config 4 on a band ctx, N = 4096, B = 256) in Newton iterations/s with each kind of Jacobian. One JSON object per
line on stdout; --json also writes them to a file.

    python tools/dq_ab.py [--reps 20] [--rounds 200] [--json profiles/dq_ab.json]

The rate counts 4 n^3 flops per system (n residuals of 2 n^2 multiply-adds each), as a plain evaluation of the definition would
execute them; the kernel itself executes fewer (dq_kernels.hpp: prefix chains and products shared exactly), so the figure is an
effective rate, quoted against DESIGN.md's 39.3 TFLOP/s fp64 ceiling without FMA."""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "rust-ida_amd"))
import idahip  # noqa: E402
from idahip import problems  # noqa: E402

F_YYPREDICT, F_YPPREDICT, F_EWT = 2, 3, 4
UNFUSED_CEILING = 39.3e12
LINES = []


def emit(rec):
    LINES.append(rec)
    print(json.dumps(rec), flush=True)


def problem(kind, n, B):
    if kind == "heat1d":
        return problems.heat1d(n=n, batch=B)
    if kind == "linear_dense":
        return problems.linear_dense(n=n, batch=B)
    if kind == "lorenz63":
        return problems.lorenz63(batch=B)
    p = problems.roberts()
    return dict(p, yy0=np.tile(p["yy0"], (B, 1)), yp0=np.tile(p["yp0"], (B, 1)))


def setups(kind, n, B, band, reps):
    """seconds per call of the two setup entry points, and of their Jacobian kernels alone (kernel-class timers)"""
    p = problem(kind, n, B)
    ctx = problems.make_ctx(p, band=band if band else False)
    ewt = 1.0 / (p["rtol"] * np.abs(p["yy0"]) + np.asarray(p["atol"])[None, :])
    ctx.upload(F_YYPREDICT, p["yy0"]); ctx.upload(F_YPPREDICT, p["yp0"]); ctx.upload(F_EWT, ewt)
    tn, cj, hh = np.zeros(B), np.full(B, 1.0e3), np.full(B, 1.0e-3)
    ctx.nls_sys(tn, cj, True)
    res = {"analytic": [], "dq": []}
    jac = {"analytic": 0.0, "dq": 0.0}
    for r in range(reps + 1):
        for mode in ("analytic", "dq"):
            ctx.set_jacobian_dq(mode == "dq")
            ctx.H.idahip_sync(ctx.h)
            ctx.timing(1); ctx.timing_reset()
            t0 = time.perf_counter()
            if mode == "dq":
                ctx.nls_lsetup_dq(tn, cj, hh)
            else:
                ctx.nls_lsetup(tn, cj)
            ctx.H.idahip_sync(ctx.h)
            dt = time.perf_counter() - t0
            t = ctx.timing_get()
            ctx.timing(0)
            if r > 0:  # (the first pair warms up)
                res[mode].append(dt)
                jac[mode] += t["jac"]["ms"] / 1e3
    ctx.close()
    out = {"case": "setup", "kind": kind, "n": n, "batch": B, "band": list(band) if band else None, "reps": reps}
    for mode in ("analytic", "dq"):
        out[mode + "_setup_ms"] = round(1e3 * float(np.median(res[mode])), 4)
        out[mode + "_jac_ms"] = round(1e3 * jac[mode] / reps, 4)
    if kind == "linear_dense":
        flops = 4.0 * n ** 3 * B
        rate = flops / (jac["dq"] / reps)
        out["dq_jac_tflops_4n3"] = round(rate / 1e12, 3)
        out["dq_jac_fraction_of_39.3T"] = round(rate / UNFUSED_CEILING, 4)
    emit(out)


def heat_band_stream(rounds, runs):
    p = problems.heat1d(n=4096, batch=256)
    rec = {"case": "heat_band_stream", "n": 4096, "batch": 256, "band": [1, 1], "rounds": rounds, "lu_period": 5}
    ens_ctx = {}
    for mode in ("analytic", "dq"):
        ctx = problems.make_ctx(p, band=True)
        ctx.set_lu_period(5)
        ctx.set_jacobian_dq(mode == "dq")
        ens = idahip.Ensemble(ctx, p["yy0"], p["yp0"])
        assert ens.device_controller_active() == 2
        ens.stream(p["touts"], 200, stagger_rounds=100)
        ens_ctx[mode] = (ctx, ens)
    rates = {"analytic": [], "dq": []}
    for _ in range(runs):
        for mode in ("analytic", "dq"):
            ctx, ens = ens_ctx[mode]
            ctx.H.idahip_sync(ctx.h)
            it0 = ens.total_newton_iters()
            t0 = time.perf_counter()
            ens.stream(p["touts"], rounds)
            ctx.H.idahip_sync(ctx.h)
            rates[mode].append((ens.total_newton_iters() - it0) / (time.perf_counter() - t0))
    for mode in ("analytic", "dq"):
        rec[mode + "_iters_per_s"] = [round(v, 1) for v in rates[mode]]
        rec[mode + "_median"] = round(float(np.median(rates[mode])), 1)
        ctx, ens = ens_ctx[mode]
        rec[mode + "_nre_dq_total"] = int(ens.counter("nre_dq").sum())
        ens.close()
        ctx.close()
    emit(rec)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--rounds", type=int, default=200)
    ap.add_argument("--runs", type=int, default=3)
    ap.add_argument("--json", default=None)
    a = ap.parse_args()
    for kind, n, B, band in (("roberts", 3, 1024, None), ("lorenz63", 3, 1024, None), ("heat1d", 4096, 256, (1, 1)),
                             ("heat1d", 4096, 32, None), ("linear_dense", 512, 512, None), ("linear_dense", 1024, 64, None)):
        setups(kind, n, B, band, a.reps)
    heat_band_stream(a.rounds, a.runs)
    if a.json:
        with open(a.json, "w") as f:
            json.dump(LINES, f, indent=1)


if __name__ == "__main__":
    main()
