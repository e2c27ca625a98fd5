"""What an event costs: idaens_reinit_at_return for a quarter of the systems against the only alternative there was before it -- download
yy / yp, change them on the host, idaens_destroy + idaens_create of the whole ensemble (which also throws away every other system's
history and cannot set a start time). One box, one process, the two alternating, medians of --reps after a warm-up of each; every timed
call sits between two idahip_sync calls on a host clock.

  lorenz      problems.lorenz63's 70 systems of tests/roots_cases.py tiled to B = 16384 (n = 3, the one-thread device stepper)
  linear512   problems.linear_dense(n = 512), B = 4096 (the device lock-step rounds)

Before every timed call the ensemble is solved to the next tout (untimed), so that every system has returned; the jump is
dy = -0.5 * y at component 0 of the listed systems (b % 4 == rep % 4), dy' = none.

    python tools/reinit_ab.py [--json profiles/reinit_ab.json] [--reps 7] [--small]
"""
import argparse
import json
import os
import socket
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "rust-ida_amd"))


def tiled(p, batch):
    import numpy as np
    B = p["yy0"].shape[0]
    reps = (batch + B - 1) // B
    out = dict(p)
    for k, v in p.items():
        if isinstance(v, np.ndarray) and v.ndim >= 1 and v.shape[0] == B and k not in ("atol", "touts"):
            out[k] = np.ascontiguousarray(np.concatenate([v] * reps)[:batch])
    return out


def stats(v):
    v = sorted(v)
    return {"median": v[len(v) // 2], "min": v[0], "max": v[-1], "spread": v[-1] - v[0], "runs": v}


def measure(name, p, dt, reps):
    import numpy as np
    import idahip
    from idahip import problems
    B, n = p["yy0"].shape
    ctx = problems.make_ctx(p)
    ens = idahip.Ensemble(ctx, p["yy0"], p["yp0"])
    active = ens.device_controller_active()
    sync = lambda: ctx.H.idahip_sync(ctx.h)
    t_reinit, t_recreate = [], []
    step, failed = [0], [0]

    def advance():
        step[0] += 1
        st, _ = ens.solve(dt * step[0])
        failed[0] += int((st < 0).sum())  # (a measurement of the call, not a check of the integration: counted and reported)

    for rep in range(-1, reps):  # rep -1: the warm-up of each
        listed = np.arange(rep % 4, B, 4, dtype=np.int32)
        # A: the jump crosses to the device, the listed systems restart where they are
        advance()
        dy = np.zeros((listed.size, n))
        dy[:, 0] = -0.5 * ens.yy()[listed, 0]
        sync()
        t0 = time.perf_counter()
        ens.reinit_at_return(listed, dy=dy)
        sync()
        ta = time.perf_counter() - t0
        # B: everything comes back, the ensemble is made anew (at t = 0: it has no other start time)
        advance()
        sync()
        t0 = time.perf_counter()
        yy, yp = ens.yy(), ens.yp()
        yy[listed, 0] += -0.5 * yy[listed, 0]
        ens.close()
        ens = idahip.Ensemble(ctx, yy, yp)
        sync()
        tb = time.perf_counter() - t0
        step[0] = 0
        if rep >= 0:
            t_reinit.append(ta)
            t_recreate.append(tb)
    ens.close()
    ctx.close()
    a, b = stats(t_reinit), stats(t_recreate)
    rec = {"case": name, "n": n, "batch": B, "listed": int(np.arange(0, B, 4).size), "stepper": active, "failed_statuses": failed[0], "reinit_at_return_s": a,
           "download_destroy_create_s": b, "ratio_recreate_over_reinit": b["median"] / a["median"]}
    print("%-10s n=%d B=%d listed=%d stepper=%d: reinit_at_return %.6f s (%.6f .. %.6f), download+destroy+create %.6f s (%.6f .. %.6f), x%.1f"
          % (name, n, B, rec["listed"], active, a["median"], a["min"], a["max"], b["median"], b["min"], b["max"], rec["ratio_recreate_over_reinit"]))
    return rec


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--json", default=None)
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--small", action="store_true", help="B = 512 and n = 64, B = 64: a quick check of the script, not a measurement")
    a = ap.parse_args()
    from idahip import problems
    out = {"host": socket.gethostname(), "reps": a.reps, "small": a.small, "cases": []}
    out["cases"].append(measure("lorenz", tiled(problems.lorenz63(batch=70), 512 if a.small else 16384), 0.01, a.reps))
    lin = problems.linear_dense(n=64, batch=64, procs=1) if a.small else problems.linear_dense(n=512, batch=4096, procs=16)
    out["cases"].append(measure("linear%d" % lin["n"], lin, 0.01, a.reps))
    if a.json:
        with open(a.json, "w") as f:
            json.dump(out, f, indent=1)
            f.write("\n")
    print(json.dumps({"reinit_ab": [{k: c[k] for k in ("case", "ratio_recreate_over_reinit")} for c in out["cases"]]}))


if __name__ == "__main__":
    main()
