"""What rate laws cost, on one box.

(a) The price for polynomial networks: tools/mass_action_ab.py's two device cases -- the Brusselator network at n = 32, B = 16384 to
    t = 0.5, and reaction_chain(64) at B = 16384 to its first output, both on the device lock-step rounds -- with THIS build and with
    a build of the parent commit (--parent-tree: a checkout of it with its libraries built), as alternating FRESH PROCESSES, each
    with a warm-up pass of its own, medians of --reps. The new build passes if its median lies within the parent's own run-to-run
    spread (not above the parent's slowest run).
(b) For the record, one process, the variants alternating: problems.enzyme_chain(32) at B = 16384 (256 generated systems, tiled) on
    the device rounds to t = 0.03, against the same network with its factors removed -- the cost of the divisions; both integrate
    different systems, so the seconds per Newton iteration and, from one extra timed pass of each, the device time of the residual and
    Jacobian kernel classes per evaluation are given as well --, and against its host-callback twin (vectorised
    numpy callbacks, by value) at --callback-batch systems (1024) on the host stepper.

    python tools/rate_laws_ab.py --parent-tree ../parent [--json profiles/rate_laws_ab.json] [--reps 7] [--small]
"""
import argparse
import json
import os
import socket
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def tiled(gen, B):
    import numpy as np
    out = dict(gen)
    rep = max(1, B // gen["yy0"].shape[0])
    for k in ("yy0", "yp0", "params"):
        out[k] = np.ascontiguousarray(np.tile(gen[k], (rep, 1)))
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
    rec = {"seconds": sec, "finished": int((status == 0).sum()), **{k: int(c[k].sum()) for k in ("nst", "nni", "nre", "nje", "netf", "ncfn")}}
    if timing:
        t = ctx.timing_get()
        rec["sys_ms"], rec["jac_ms"] = t["sys"]["ms"], t["jac"]["ms"]
        ctx.timing(0)
    ens.close()
    return rec


def polynomial_case(name, B):
    from idahip import problems
    if name == "bruss":
        return problems.bruss1d_network(16, B), [0.5]
    gen = problems.reaction_chain(64, min(B, 256), seed=64)
    return tiled(gen, B), [float(gen["touts"][0])]


def child(name, B):
    """one fresh process: a warm-up pass, then the timed one"""
    from idahip import problems
    p, touts = polynomial_case(name, B)
    ctx = problems.make_ctx(p)
    timed(ctx, p, touts, 2)
    rec = timed(ctx, p, touts, 2)
    ctx.close()
    print("RESULT " + json.dumps(rec), flush=True)


def spawn(tree, name, B):
    env = dict(os.environ, PYTHONPATH=os.path.join(tree, "rust-ida_amd"))
    out = subprocess.run([sys.executable, os.path.abspath(__file__), "--child", name, "--batch", str(B)], env=env, capture_output=True, text=True,
                         timeout=300)
    if out.returncode != 0:
        raise SystemExit("child (%s, %s) ended with %d:\n%s" % (tree, name, out.returncode, out.stderr[-2000:]))
    return json.loads([l for l in out.stdout.splitlines() if l.startswith("RESULT ")][-1][7:])


def stats(runs):
    import numpy as np
    s = sorted(r["seconds"] for r in runs)
    return {"seconds_median": round(float(np.median(s)), 5), "seconds_min": round(s[0], 5), "seconds_max": round(s[-1], 5),
            "seconds": [round(x, 5) for x in (r["seconds"] for r in runs)], **{k: runs[-1][k] for k in ("finished", "nst", "nni", "nre", "nje", "netf", "ncfn")}}


def without_factors(p):
    q = dict(p)
    q["reactions"] = [(r[0], r[1]) for r in p["reactions"]]
    return q


def enzyme_callbacks(p):
    """enzyme_chain as host callbacks, vectorised numpy, by value (a measurement, not a check)"""
    import numpy as np
    n, P = p["n"], p["params"]
    m = n - 1
    R = 2 * m + 3
    i = np.arange(m - 1)
    h = 1 + i % 3

    def parts(s, y):
        k, K = P[s][:R], P[s][R:]
        feed = k[0] * K[0] ** 2 / (K[0] ** 2 + y[m - 1] ** 2)
        yh, Kh = y[i] ** h, K[1 + i] ** h
        step = k[1 + i] * yh / (Kh + yh)
        dstep = k[1 + i] * h * Kh * y[i] ** (h - 1) / (Kh + yh) ** 2
        inh, sat = K[0] / (K[0] + y[2]), y[0] ** 2 / (K[1] ** 2 + y[0] ** 2)
        return k, K, feed, step, dstep, inh, sat

    def res(s, t, y, yp):
        k, K, feed, step, dstep, inh, sat = parts(s, y)
        f = np.zeros(n)
        f[0] += feed
        f[i] -= step
        f[i + 1] += step
        f[m - 1] -= k[m] * y[m - 1]
        b = k[m + 1] * y[0] * y[1] * inh * sat
        f[0] -= b
        f[1] -= b
        f[2] += b
        r = yp - f
        r[n - 1] = -(y[:m].sum() - y[n - 1])
        return r

    def jac(s, t, cj, y, yp, rr):
        k, K, feed, step, dstep, inh, sat = parts(s, y)
        J = np.zeros((n, n))  # (row, column): d(yp - f)
        J[0, m - 1] += k[0] * K[0] ** 2 * 2.0 * y[m - 1] / (K[0] ** 2 + y[m - 1] ** 2) ** 2
        J[i, i] += dstep
        J[i + 1, i] -= dstep
        J[m - 1, m - 1] += k[m]
        kb = k[m + 1]
        db = np.zeros(n)
        db[0] = kb * y[1] * inh * sat + kb * y[0] * y[1] * inh * (2.0 * K[1] ** 2 * y[0] / (K[1] ** 2 + y[0] ** 2) ** 2)
        db[1] = kb * y[0] * inh * sat
        db[2] = -kb * y[0] * y[1] * sat * K[0] / (K[0] + y[2]) ** 2
        J[0] += db
        J[1] += db
        J[2] -= db
        J[np.arange(m), np.arange(m)] += cj
        J[n - 1, :m] = -1.0
        J[n - 1, n - 1] = 1.0
        return J

    out = {k: v for k, v in p.items() if k not in ("params", "reactions", "d", "nconst")}
    out.update(kind="host_callback", res=res, jac=jac)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--json", default=None)
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--parent-tree", default=None, help="a checkout of the parent commit with its libraries built; without it (a) is left out")
    ap.add_argument("--callback-batch", type=int, default=1024)
    ap.add_argument("--callback-reps", type=int, default=3)
    ap.add_argument("--small", action="store_true", help="toy batches: a rehearsal of the script, not a measurement")
    ap.add_argument("--child", default=None)
    ap.add_argument("--batch", type=int, default=16384)
    a = ap.parse_args()
    if a.child:
        return child(a.child, a.batch)
    sys.path.insert(0, os.path.join(ROOT, "rust-ida_amd"))
    import numpy as np
    from idahip import problems
    B = 64 if a.small else 16384
    Bc = min(B, 16 if a.small else a.callback_batch)
    base = {"host": socket.gethostname(), "reps": a.reps, "batch": B}
    lines = []
    # ---- (a) polynomial networks, this build against the parent's
    if a.parent_tree:
        trees = {"new": ROOT, "parent": os.path.abspath(a.parent_tree)}
        for name in ("bruss", "chain"):
            runs = {k: [] for k in trees}
            for rep in range(a.reps):
                for k in (("new", "parent") if rep % 2 == 0 else ("parent", "new")):
                    runs[k].append(spawn(trees[k], name, B))
            out = dict(base, part="a", case=name, new=stats(runs["new"]), parent=stats(runs["parent"]))
            out["parent_spread_seconds"] = round(out["parent"]["seconds_max"] - out["parent"]["seconds_min"], 5)
            out["new_minus_parent_median_seconds"] = round(out["new"]["seconds_median"] - out["parent"]["seconds_median"], 5)
            out["new_over_parent"] = round(out["new"]["seconds_median"] / out["parent"]["seconds_median"], 4)
            out["new_median_within_parent_spread"] = bool(out["new"]["seconds_median"] <= out["parent"]["seconds_max"])
            out["same_counters"] = all(out["new"][k] == out["parent"][k] for k in ("finished", "nst", "nni", "nre", "nje", "netf", "ncfn"))
            print(json.dumps(out), flush=True)
            lines.append(json.dumps(out))
    # ---- (b) the divisions, and the host-callback twin
    n, touts = 32, [0.03]
    gen = problems.enzyme_chain(n, min(B, 256))
    laws = tiled(gen, B)
    poly = without_factors(laws)
    small = {k: (v[:Bc] if k in ("yy0", "yp0", "params") else v) for k, v in laws.items()}
    cb = enzyme_callbacks(small)
    ctxs = {"laws": (problems.make_ctx(laws), laws, 2), "factors_removed": (problems.make_ctx(poly), poly, 2)}
    runs = {k: [] for k in ctxs}
    for rep in range(a.reps + 1):
        for k, (c, p, act) in ctxs.items():
            r = timed(c, p, touts, act)
            if rep > 0:
                runs[k].append(r)
    c_cb = problems.make_ctx(cb)
    cb_runs = [timed(c_cb, cb, touts, 0) for _ in range(a.callback_reps)]
    out = dict(base, part="b", case="enzyme_chain", n=n, horizon=touts[-1], nreac=2 * (n - 1) + 3, nconst=n - 1,
               pattern=list(ctxs["laws"][0].mass_action_pattern()), generated_systems=int(gen["yy0"].shape[0]))
    for k in ctxs:
        out[k] = stats(runs[k])
        out[k]["us_per_newton_iteration"] = round(1e6 * out[k]["seconds_median"] / out[k]["nni"], 5)
        t = timed(ctxs[k][0], ctxs[k][1], touts, 2, timing=True)  # (one extra pass: idahip_timing_enable perturbs the wall time)
        out[k]["residual_class_device_ms_one_timed_pass"] = round(t["sys_ms"], 3)
        out[k]["jacobian_class_device_ms_one_timed_pass"] = round(t["jac_ms"], 3)
        out[k]["residual_ns_per_evaluation"] = round(1e6 * t["sys_ms"] / t["nre"], 3)
        out[k]["jacobian_ns_per_evaluation"] = round(1e6 * t["jac_ms"] / t["nje"], 3)
    out["callback"] = dict(stats(cb_runs), batch=Bc)
    out["callback"]["us_per_newton_iteration"] = round(1e6 * out["callback"]["seconds_median"] / out["callback"]["nni"], 3)
    out["laws_over_factors_removed_residual_ns"] = round(out["laws"]["residual_ns_per_evaluation"] / out["factors_removed"]["residual_ns_per_evaluation"], 3)
    out["laws_over_factors_removed_jacobian_ns"] = round(out["laws"]["jacobian_ns_per_evaluation"] / out["factors_removed"]["jacobian_ns_per_evaluation"], 3)
    out["laws_over_factors_removed_per_newton_iteration"] = round(out["laws"]["us_per_newton_iteration"] / out["factors_removed"]["us_per_newton_iteration"], 3)
    out["callback_over_laws_per_newton_iteration"] = round(out["callback"]["us_per_newton_iteration"] / out["laws"]["us_per_newton_iteration"], 1)
    print(json.dumps(out), flush=True)
    lines.append(json.dumps(out))
    for c, _, _ in ctxs.values():
        c.close()
    c_cb.close()
    if a.json:
        open(a.json, "w").write("\n".join(lines) + "\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
