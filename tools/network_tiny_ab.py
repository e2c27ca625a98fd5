"""What the one-thread stepper is worth for a reaction network of n <= 8 species (idahip_set_mass_action_tiny; DESIGN.md section 4m+),
on one box in one process, the variants alternating, medians of --reps runs after a warm-up pass of each. The time is the wall time of
idaens_solve_schedule, ending in a device synchronise.

Cases (B systems, one output at the horizon):
  roberts    problems.roberts_network, the three kinetic constants of system s scaled by 1 + (s mod 64)/64, B = 65536, to t = 4.0
  lorenz     problems.lorenz63_network, B = 1024 and B = 65536, to t = 1.0
  enzyme8    problems.enzyme_chain(8) (rate laws), 256 generated systems tiled to B = 65536, to t = 0.03
Variants:
  host       the network on the host stepper: what a network of this size runs on with the switch off
  tiny       the network on the one-thread stepper (tiny_net_ida_kernel)
  builtin    Roberts and Lorenz63 only: the compiled kind on the one-thread stepper (tiny_ida_kernel) -- the price of interpreting the
             tables and of a run-time n. (The compiled Roberts has its constants built in: its B systems are all system 0, so for
             Roberts the ratio to take is the one of the Newton iteration rates.)
--spw: instead of the A/B, the tiny variant of the lorenz (n = 3) and enzyme8 (n = 8) cases at B = 65536 under IDAHIP_TINY_SPW = 8, 16,
32, 64 and without it (the library's rule), alternating in the same way: the measurement behind the launch-shape rule.

    python tools/network_tiny_ab.py [--json profiles/network_tiny_ab.json] [--reps 7] [--small] [--spw]
"""
import argparse
import json
import os
import socket
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "rust-ida_amd"))

CNT = ("nst", "nni", "nre", "nje", "nsetups", "netf", "ncfn")


def tiled(gen, B):
    import numpy as np
    out = dict(gen)
    rep = (B + gen["yy0"].shape[0] - 1) // gen["yy0"].shape[0]
    for k in ("yy0", "yp0", "params"):
        out[k] = np.ascontiguousarray(np.tile(gen[k], (rep, 1))[:B])
    return out


def roberts_scaled(B):
    import numpy as np
    from idahip import mass_action, problems
    p = problems.roberts_network()
    m = min(B, 64)
    k = np.tile(p["params"], (m, 1))
    k[:, :3] *= (1.0 + np.arange(m) / 64.0)[:, None]
    tab = mass_action.tables(3, p["reactions"], p["d"])
    p["params"], p["yy0"] = k, np.tile(p["yy0"], (m, 1))
    p["yp0"] = np.stack([mass_action.rhs(tab, k[s], p["yy0"][s]) * p["d"] for s in range(m)])
    return tiled(p, B)


def roberts_builtin(B):
    import numpy as np
    from idahip import problems
    p = problems.roberts()
    p["yy0"], p["yp0"] = np.tile(p["yy0"], (B, 1)), np.tile(p["yp0"], (B, 1))
    return p


def timed(ctx, p, touts, want_active):
    import idahip
    ens = idahip.Ensemble(ctx, p["yy0"], p["yp0"])
    if want_active == 0:
        ens.set_device_controller(0)
    assert ens.device_controller_active() == want_active, (ens.device_controller_active(), want_active)
    ctx.H.idahip_sync(ctx.h)
    t0 = time.perf_counter()
    status = ens.solve_schedule(touts)[0]
    ctx.H.idahip_sync(ctx.h)
    sec = time.perf_counter() - t0
    c = ens.counters()
    rec = {"seconds": sec, "finished": int((status == 0).sum()), "rounds": int(ens.total_rounds()), **{k: int(c[k].sum()) for k in CNT}}
    ens.close()
    return rec


def summary(runs, batch):
    import numpy as np
    secs = sorted(r["seconds"] for r in runs)
    last = runs[-1]
    med = float(np.median(secs))
    return {"batch": batch, "seconds_median": round(med, 5), "seconds_min": round(secs[0], 5), "seconds_max": round(secs[-1], 5),
            "newton_iters_per_s_median": round(last["nni"] / med, 1), **{k: last[k] for k in ("finished", "rounds") + CNT}}


def alternate(variants, reps):
    """variants: {name: callable -> record}; the first pass of each is dropped"""
    runs = {k: [] for k in variants}
    for rep in range(reps + 1):
        for name, fn in variants.items():
            r = fn()
            if rep > 0:
                runs[name].append(r)
    return runs


def cases(small):
    from idahip import problems
    big, mid = (256, 64) if small else (65536, 1024)
    yield "roberts", big, roberts_scaled(big), [4.0], roberts_builtin(big)
    for B in (mid, big):
        yield "lorenz", B, problems.lorenz63_network(B), [1.0], problems.lorenz63(B)
    yield "enzyme8", big, tiled(problems.enzyme_chain(8, min(big, 256)), big), [0.03], None


def ab(a, base):
    from idahip import problems
    lines = []
    for name, B, net, touts, blt in cases(a.small):
        c_host, c_tiny = problems.make_ctx(net), problems.make_ctx(net)
        c_tiny.set_mass_action_tiny()
        variants = {"host": lambda: timed(c_host, net, touts, 0), "tiny": lambda: timed(c_tiny, net, touts, 1)}
        ctxs = [c_host, c_tiny]
        if blt is not None:
            c_blt = problems.make_ctx(blt)
            ctxs.append(c_blt)
            variants["builtin"] = lambda: timed(c_blt, blt, touts, 1)
        runs = alternate(variants, a.reps)
        out = dict(base, case=name, n=int(net["n"]), batch=B, horizon=touts[-1])
        for v in variants:
            out[v] = summary(runs[v], B)
        out["host_over_tiny_seconds"] = round(out["host"]["seconds_median"] / out["tiny"]["seconds_median"], 3)
        out["tiny_beats_host"] = out["tiny"]["seconds_median"] < out["host"]["seconds_median"]
        if blt is not None:
            if name != "roberts":  # (the compiled Roberts runs B copies of system 0: another workload, its seconds do not compare)
                out["tiny_over_builtin_seconds"] = round(out["tiny"]["seconds_median"] / out["builtin"]["seconds_median"], 3)
            out["tiny_over_builtin_newton_rate"] = round(out["tiny"]["newton_iters_per_s_median"] / out["builtin"]["newton_iters_per_s_median"], 3)
        print(json.dumps(out), flush=True)
        lines.append(json.dumps(out))
        for c in ctxs:
            c.close()
    return lines


def spw_sweep(a, base):
    from idahip import problems
    lines = []
    for name, B, net, touts, _ in cases(a.small):
        if name == "roberts" or (name == "lorenz" and B < (256 if a.small else 65536)):
            continue
        ctx = problems.make_ctx(net)
        ctx.set_mass_action_tiny()

        def run(spw):
            if spw:
                os.environ["IDAHIP_TINY_SPW"] = str(spw)
            try:
                return timed(ctx, net, touts, 1)
            finally:
                os.environ.pop("IDAHIP_TINY_SPW", None)

        runs = alternate({("spw%d" % s if s else "rule"): (lambda s=s: run(s)) for s in (8, 16, 32, 64, 0)}, a.reps)
        out = dict(base, case=name + "_spw", n=int(net["n"]), batch=B, horizon=touts[-1])
        for v in runs:
            out[v] = summary(runs[v], B)
        print(json.dumps(out), flush=True)
        lines.append(json.dumps(out))
        ctx.close()
    return lines


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--json", default=None)
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--small", action="store_true", help="toy batches: a rehearsal of the script, not a measurement")
    ap.add_argument("--spw", action="store_true", help="the launch-shape sweep instead of the A/B")
    a = ap.parse_args()
    base = {"host": socket.gethostname(), "reps": a.reps,
            "command": "python tools/network_tiny_ab.py --reps %d%s%s" % (a.reps, " --small" if a.small else "", " --spw" if a.spw else "")}
    lines = spw_sweep(a, base) if a.spw else ab(a, base)
    if a.json:
        open(a.json, "w").write("\n".join(lines) + "\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
