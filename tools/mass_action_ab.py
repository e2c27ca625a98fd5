"""What interpreting a reaction network costs, on one box in one process, the variants alternating, medians of --reps runs after a
warm-up pass of each (the IDAHIP_MASS_ACTION section).

Line "bruss": the Brusselator at m = 16 (n = 32), B = 16384, dense ctx, idaens_solve_schedule to t = 0.5, three ways:
  network    problems.bruss1d_network on the device lock-step rounds (the table-driven kernels)
  builtin    problems.bruss1d, the compiled kind, on the device lock-step rounds: the price of interpreting a table
  callback   the same systems as a host-callback problem on the host stepper -- what a user with a problem of their own had before.
             The callbacks are vectorised numpy (about 20 us a call), --callback-batch systems (1024): seconds are also given scaled
             to the full batch, which flatters it (its cost per system does not fall with the batch).
Line "chain": problems.reaction_chain(n = 64), B = 16384 (256 generated systems, tiled), to its first output, on the device rounds
with the wave-per-system residual (four systems per workgroup) against the workgroup-per-system residual (IDAHIP_MA_WG=1, a
measurement switch read at idahip_create): what the packing is worth; with the device time of the residual class of one extra,
timed pass of each (idahip_timing_enable perturbs the wall time, so that pass is not among the repetitions).

    python tools/mass_action_ab.py [--json profiles/mass_action_ab.json] [--reps 7] [--small]
"""
import argparse
import json
import os
import socket
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "rust-ida_amd"))


def bruss_callbacks(p):
    """the Brusselator of problems.bruss1d as host callbacks, vectorised (by value: a measurement, not a check)"""
    import numpy as np
    from idahip import problems
    P, n = p["params"], p["n"]
    ends = np.array([0, 1, n - 2, n - 1])

    def res(s, t, y, yp):
        prm = P[s]
        r = yp - problems.bruss1d_rhs(prm, y)
        r[ends] = y[ends] - np.array([prm[3], prm[4], prm[3], prm[4]])
        return r

    def jac(s, t, cj, y, yp, rr):
        a, b, d = P[s][:3]
        J = np.zeros((n, n))  # (row, column)
        i = np.arange(2, n - 2, 2)
        u, v = y[i], y[i + 1]
        t2, uu = (2.0 * u) * v, u * u
        J[i, i - 2] = J[i, i + 2] = J[i + 1, i - 1] = J[i + 1, i + 3] = -d
        J[i, i] = cj - ((t2 - (b + 1.0)) - 2.0 * d)
        J[i, i + 1] = -uu
        J[i + 1, i] = -(b - t2)
        J[i + 1, i + 1] = cj + (uu + 2.0 * d)
        J[ends, ends] = 1.0
        return J

    out = {k: v for k, v in p.items() if k != "params"}
    out.update(kind="host_callback", res=res, jac=jac)
    return out


def timed(ctx, p, touts, want_active, timing=False):
    import idahip
    ens = idahip.Ensemble(ctx, p["yy0"], p["yp0"])
    if want_active == 0:
        ens.set_device_controller(0)
    assert ens.device_controller_active() == want_active
    if timing:
        ctx.timing_reset()
        ctx.timing(1)
    ctx.H.idahip_sync(ctx.h)
    t0 = time.perf_counter()
    status = ens.solve_schedule(touts)[0]
    ctx.H.idahip_sync(ctx.h)
    sec = time.perf_counter() - t0
    c = ens.counters()
    rec = {"seconds": sec, "finished": int((status == 0).sum()), "rounds": int(ens.total_rounds()),
           **{k: int(c[k].sum()) for k in ("nst", "nni", "nre", "nje", "nsetups", "netf", "ncfn")}}
    if timing:
        rec["sys_ms"] = ctx.timing_get()["sys"]["ms"]
        ctx.timing(0)
    ens.close()
    return rec


def summary(runs, batch):
    import numpy as np
    secs = sorted(r["seconds"] for r in runs)
    last = runs[-1]
    med = float(np.median(secs))
    return {"batch": batch, "seconds_median": round(med, 5), "seconds_min": round(secs[0], 5), "seconds_max": round(secs[-1], 5),
            "newton_iters_per_s_median": round(last["nni"] / med, 1),
            **{k: last[k] for k in ("finished", "rounds", "nst", "nni", "nre", "nje", "nsetups", "netf", "ncfn")}}


def alternate(variants, reps):
    """variants: {name: callable -> record}; the first pass of each is dropped"""
    runs = {k: [] for k in variants}
    for rep in range(reps + 1):
        for name, fn in variants.items():
            r = fn()
            if rep > 0:
                runs[name].append(r)
    return runs


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--json", default=None)
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--callback-batch", type=int, default=1024)
    ap.add_argument("--small", action="store_true", help="toy batches: a rehearsal of the script, not a measurement")
    a = ap.parse_args()
    import numpy as np
    from idahip import problems
    B = 64 if a.small else 16384
    Bc = min(B, 16 if a.small else a.callback_batch)
    base = {"host": socket.gethostname(), "reps": a.reps,
            "command": "python tools/mass_action_ab.py --reps %d --callback-batch %d%s" % (a.reps, a.callback_batch, " --small" if a.small else "")}
    lines = []
    # ---- the Brusselator three ways
    m, touts = 16, [0.5]
    net, blt = problems.bruss1d_network(m, B), problems.bruss1d(m, B)
    small = problems.bruss1d(m, Bc)
    cb = bruss_callbacks(small)
    c_net, c_blt, c_cb = problems.make_ctx(net), problems.make_ctx(blt), problems.make_ctx(cb)
    runs = alternate({"network": lambda: timed(c_net, net, touts, 2), "builtin": lambda: timed(c_blt, blt, touts, 2),
                      "callback": lambda: timed(c_cb, cb, touts, 0)}, a.reps)
    out = dict(base, case="bruss", n=2 * m, horizon=touts[-1], nreac=int(net["params"].shape[1]), pattern=list(c_net.mass_action_pattern()))
    for name, batch in (("network", B), ("builtin", B), ("callback", Bc)):
        out[name] = summary(runs[name], batch)
    out["callback"]["seconds_median_scaled_to_full_batch"] = round(out["callback"]["seconds_median"] * B / Bc, 4)
    out["network_over_builtin"] = round(out["network"]["seconds_median"] / out["builtin"]["seconds_median"], 3)
    out["callback_scaled_over_network"] = round(out["callback"]["seconds_median_scaled_to_full_batch"] / out["network"]["seconds_median"], 2)
    out["builtin_spread_seconds"] = round(out["builtin"]["seconds_max"] - out["builtin"]["seconds_min"], 5)
    print(json.dumps(out), flush=True)
    lines.append(json.dumps(out))
    for c in (c_net, c_blt, c_cb):
        c.close()
    # ---- the packing of the wave-per-system residual
    gen = problems.reaction_chain(64, min(B, 256), seed=64)
    ch = dict(gen)
    rep_ = B // gen["yy0"].shape[0]
    for k in ("yy0", "yp0", "params"):
        ch[k] = np.ascontiguousarray(np.tile(gen[k], (rep_, 1)))
    touts = [float(gen["touts"][0])]
    ctxs = {}
    for name, env in (("wave_per_system", "0"), ("workgroup_per_system", "1")):
        os.environ["IDAHIP_MA_WG"] = env
        ctxs[name] = problems.make_ctx(ch)
    os.environ.pop("IDAHIP_MA_WG")
    runs = alternate({k: (lambda c=c: timed(c, ch, touts, 2)) for k, c in ctxs.items()}, a.reps)
    out = dict(base, case="chain", n=64, horizon=touts[-1], nreac=int(ch["params"].shape[1]), generated_systems=int(gen["yy0"].shape[0]))
    for name, c in ctxs.items():
        out[name] = summary(runs[name], B)
        out[name]["residual_class_device_ms_one_timed_pass"] = round(timed(c, ch, touts, 2, timing=True)["sys_ms"], 3)
    out["workgroup_over_wave_seconds"] = round(out["workgroup_per_system"]["seconds_median"] / out["wave_per_system"]["seconds_median"], 3)
    out["workgroup_over_wave_residual_ms"] = round(out["workgroup_per_system"]["residual_class_device_ms_one_timed_pass"] /
                                                   out["wave_per_system"]["residual_class_device_ms_one_timed_pass"], 3)
    out["wave_spread_seconds"] = round(out["wave_per_system"]["seconds_max"] - out["wave_per_system"]["seconds_min"], 5)
    print(json.dumps(out), flush=True)
    lines.append(json.dumps(out))
    for c in ctxs.values():
        c.close()
    if a.json:
        open(a.json, "w").write("\n".join(lines) + "\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
