"""Config 4 (1-D heat, N = 4096, B = 256, bench.py's outputs and lu_period 5) in throughput mode on a dense ctx and on a band ctx
(idahip_create_band, ml = mu = 1), alternating, plus the band ctx alone at larger batches and one wider band (ml = mu = 16, raw
setup / solve). One JSON object per line on stdout; --json also writes them to a file.

    python tools/band_ab.py [--rounds 300] [--runs 3] [--json profiles/band_ab_config4.json]
    python tools/band_ab.py --band-only --rounds 200    # the band config-4 stream alone (for rocprofv3 --kernel-trace --stats)
"""
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

LINES = []


def emit(rec):
    LINES.append(rec)
    print(json.dumps(rec), flush=True)


def stream_setup(p, band, lu_period=5, spin_up=200, stagger=100):
    ctx = problems.make_ctx(p, band=band)
    ctx.set_lu_period(lu_period)
    ens = idahip.Ensemble(ctx, p["yy0"], p["yp0"])
    assert ens.device_controller_active() == 2
    ens.stream(p["touts"], spin_up, stagger_rounds=stagger)
    return ctx, ens


def timed(ens, ctx, touts, rounds):
    ctx.H.idahip_sync(ctx.h)
    it0 = ens.total_newton_iters()
    t0 = time.perf_counter()
    ens.stream(touts, rounds)
    ctx.H.idahip_sync(ctx.h)
    dt = time.perf_counter() - t0
    return (ens.total_newton_iters() - it0) / dt, dt


def classes(ctx, ens, touts, rounds):
    ctx.timing(1)
    ctx.timing_reset()
    ens.stream(touts, rounds)
    t = ctx.timing_get()
    ctx.timing(0)
    return {k: round(v["ms"] / rounds, 4) for k, v in t.items() if v["launches"]}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=300)
    ap.add_argument("--runs", type=int, default=3)
    ap.add_argument("--band-only", action="store_true")
    ap.add_argument("--json", default=None)
    a = ap.parse_args()
    n = 4096
    p = problems.heat1d(n=n, batch=256)
    if a.band_only:
        ctx, ens = stream_setup(p, True)
        rate, dt = timed(ens, ctx, p["touts"], a.rounds)
        emit({"what": "band config 4 stream (profiled run)", "iters_per_s": rate, "rounds": a.rounds, "s": dt})
        return
    runs = {False: [], True: []}
    ctxs = {}
    for band in (False, True):
        ctxs[band] = stream_setup(p, band)
    for r in range(a.runs):
        for band in (False, True):
            ctx, ens = ctxs[band]
            rate, dt = timed(ens, ctx, p["touts"], a.rounds)
            runs[band].append(rate)
            emit({"what": "config 4 stream", "ctx": "band" if band else "dense", "run": r, "iters_per_s": rate, "rounds": a.rounds, "s": dt})
    states = {}
    for band in (False, True):
        ctx, ens = ctxs[band]
        emit({"what": "kernel ms per round (idahip_timing_get)", "ctx": "band" if band else "dense", "ms_per_round": classes(ctx, ens, p["touts"], 50)})
        states[band] = (ens.yy(), ens.yp(), ens.counters(), ens.real("hused"), ens.total_newton_iters())
    (y0, yp0, c0, h0, i0), (y1, yp1, c1, h1, i1) = states[False], states[True]
    emit({"what": "stream state dense vs band after the same rounds", "yy_equal_by_value": bool(np.array_equal(y0, y1)),
          "yp_equal_by_value": bool(np.array_equal(yp0, yp1)), "counters_equal": all(np.array_equal(c0[k], c1[k]) for k in c0),
          "hused_equal": bool(np.array_equal(h0, h1)), "newton_iters_equal": i0 == i1})
    md, mb = float(np.median(runs[False])), float(np.median(runs[True]))
    emit({"what": "config 4 summary", "dense_median": md, "band_median": mb, "speedup": mb / md})
    for ctx, ens in ctxs.values():
        ens.close()
        ctx.close()
    for B in (1024, 4096, 16384):
        q = problems.heat1d(n=n, batch=B)
        ctx, ens = stream_setup(q, True)
        rate, dt = timed(ens, ctx, q["touts"], a.rounds)
        emit({"what": "band stream, batch scaling", "B": B, "iters_per_s": rate, "rounds": a.rounds, "s": dt,
              "ms_per_round": classes(ctx, ens, q["touts"], 30)})
        ens.close()
        ctx.close()
        del q
    # one wider band through the raw calls: ml = mu = 16, N = 4096, B = 256
    ml = mu = 16
    B = 256
    rng = np.random.default_rng(16)
    ld = idahip.band_ldab(ml, mu)
    ab = rng.standard_normal((B, n, ld))
    ab[:, :, ml + mu] += 40.0
    ctx = idahip.Ctx("host_callback", n, B, band=(0, 0))
    dA, dP = ctx.dev_array(ab), ctx.dev_array(np.zeros((B, n), dtype=np.int64))
    dX = ctx.dev_array(rng.standard_normal((B, n)))
    ctx.ls_setup_band(ml, mu, dA, dP)
    for _ in range(3):
        ctx.H.idahip_memcpy_h2d(ctx.h, dA, ab.ctypes.data_as(idahip.C.c_void_p), ab.nbytes)
        ctx.ls_setup_band(ml, mu, dA, dP)
    ctx.H.idahip_sync(ctx.h)
    ctx.timing(1)
    ctx.timing_reset()
    ctx.H.idahip_memcpy_h2d(ctx.h, dA, ab.ctypes.data_as(idahip.C.c_void_p), ab.nbytes)
    ctx.ls_setup_band(ml, mu, dA, dP)
    ctx.ls_solve_band(ml, mu, dA, dP, dX, dX)
    t = ctx.timing_get()
    emit({"what": "wide band (generic kernels), raw setup + solve", "ml": ml, "mu": mu, "n": n, "B": B, "getrf_ms": t["lu"]["ms"],
          "getrs_ms": t["solve"]["ms"]})
    ctx.close()
    if a.json:
        with open(a.json, "w") as f:
            json.dump(LINES, f, indent=1)


if __name__ == "__main__":
    main()
