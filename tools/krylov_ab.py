"""The linear solvers on the same integrations, on one box in one call: a dense ctx, a band ctx (heat only), a Krylov ctx
(matrix-free SPGMR) and, for heat, a Krylov ctx with the (1, 1) band preconditioner (section 4i). Cases: heat
n = 4096, B = 256; linear dense n = 512, B = 4096. Recorded per solver: wall time of idaens_solve_schedule to the common horizon (a
host clock around a call that ends in a device synchronise), Newton iterations per second, the sums of nst / nni / nli / ncfl / ncfn /
npe / nps over the ensemble, the statuses, and the device memory the ctx took (the preconditioner's storage included).

The solvers differ by factors, in memory or in whether they reach the horizon at all, and no speed claim rests on the times: the
runs are not alternated and a timed window is one schedule call (0.1 to 0.7 s), repeated once after a warm-up pass.
Every (case, solver) run is a child process of its own under `timeout -k 10`, and the chain stops at the first one that fails.
One JSON object per line on stdout; --json also writes them to a file.

    python tools/krylov_ab.py [--json profiles/krylov_ab.json] [--cases heat linear] [--outputs 1] [--limit 300] [--small]
    python tools/krylov_ab.py --cases heat --json profiles/krylov_prec_ab.json     (the figures of section 4i)

--rounds is another measurement, and this one is an A/B: the Krylov ctx of each case (heat: with the (1, 1) preconditioner) on the
host stepper against the device lock-step rounds (idahip_set_krylov_rounds), in one process on one ctx, the two alternating over
--reps repetitions after a warm-up pass of each. Per case one line with the medians, the host stepper's spread (max - min) next to
the difference of the medians, and for heat a second line: idaens_stream over --stream-rounds rounds, Newton iterations per second.

    python tools/krylov_ab.py --rounds --json profiles/krylov_rounds_ab.json
"""
import argparse
import json
import os
import socket
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "rust-ida_amd"))

CASES = {"heat": ("heat1d", 4096, 256, ("dense", "band", "krylov", "krylov_prec")), "linear": ("linear_dense", 512, 4096, ("dense", "krylov"))}
SMALL = {"heat": ("heat1d", 256, 16, ("dense", "band", "krylov", "krylov_prec")), "linear": ("linear_dense", 64, 32, ("dense", "krylov"))}


def one(case, solver, outputs, small):
    import numpy as np
    import torch
    import idahip
    from idahip import problems
    kind, n, batch, _ = (SMALL if small else CASES)[case]
    p = problems.heat1d(n=n, batch=batch) if kind == "heat1d" else problems.linear_dense(n=n, batch=batch, procs=8)
    touts = p["touts"][:outputs]
    torch.cuda.init()
    free0 = torch.cuda.mem_get_info()[0]
    ctx = problems.make_ctx(p, band=(solver == "band"), krylov=(0 if solver.startswith("krylov") else None))
    if solver == "krylov_prec":
        ctx.set_krylov_band_prec(1, 1)
    mem = free0 - torch.cuda.mem_get_info()[0]
    recs = []
    for rep in range(2):  # the first pass warms the code objects up; the second is the figure
        ens = idahip.Ensemble(ctx, p["yy0"], p["yp0"])
        ctx.H.idahip_sync(ctx.h)
        t0 = time.perf_counter()
        status, tret, reached = ens.solve_schedule(touts)
        ctx.H.idahip_sync(ctx.h)
        sec = time.perf_counter() - t0
        c = ens.counters()
        recs.append({"case": case, "kind": kind, "n": n, "batch": batch, "solver": solver, "pass": rep, "horizon": float(touts[-1]),
                     "seconds": round(sec, 4), "newton_iters_per_s": round(float(c["nni"].sum()) / sec, 1),
                     "device_controller": ens.device_controller_active(), "ctx_device_bytes": int(mem),
                     "finished": int((status == 0).sum()), "conv_fail": int((status == -4).sum()), "other_status": int(((status != 0) & (status != -4)).sum()),
                     **{k: int(c[k].sum()) for k in ("nst", "nni", "nli", "ncfl", "ncfn", "netf", "nsetups", "nje", "nre", "nre_dq", "npe", "nps")},
                     "host": socket.gethostname(), "command": "python tools/krylov_ab.py --cases %s --outputs %d%s" % (case, outputs, " --small" if small else "")})
        ens.close()
    ctx.close()
    for r in recs:
        print(json.dumps(r), flush=True)


def rounds_ab(case, outputs, small, reps, stream_rounds):
    """The Krylov ctx of the case (heat: with the (1, 1) band preconditioner) on the host stepper against the device lock-step rounds
    (idahip_set_krylov_rounds): one process, one ctx, the two variants alternating over `reps` repetitions after a warm-up pass of
    each; medians, and the spread of the host-stepper runs next to the difference. heat also: idaens_stream for a fixed number of
    rounds, Newton iterations per second."""
    import numpy as np
    import idahip
    from idahip import problems
    kind, n, batch, _ = (SMALL if small else CASES)[case]
    p = problems.heat1d(n=n, batch=batch) if kind == "heat1d" else problems.linear_dense(n=n, batch=batch, procs=8)
    touts = p["touts"][:outputs]
    ctx = problems.make_ctx(p, krylov=0)
    if kind == "heat1d":
        ctx.set_krylov_band_prec(1, 1)
    base = {"case": case, "kind": kind, "n": n, "batch": batch, "solver": "krylov_prec" if kind == "heat1d" else "krylov", "host": socket.gethostname(),
            "command": "python tools/krylov_ab.py --rounds --cases %s --outputs %d --reps %d%s" % (case, outputs, reps, " --small" if small else "")}

    def timed(rounds, stream):
        ctx.set_krylov_rounds(rounds)
        ens = idahip.Ensemble(ctx, p["yy0"], p["yp0"])
        assert ens.device_controller_active() == (2 if rounds else 0)
        ctx.H.idahip_sync(ctx.h)
        t0 = time.perf_counter()
        if stream:  # "finished": integrations completed inside the stream
            finished = ens.stream(touts, stream_rounds, stagger_rounds=stream_rounds // 3)
        else:
            finished = int((ens.solve_schedule(touts)[0] == 0).sum())
        ctx.H.idahip_sync(ctx.h)
        sec = time.perf_counter() - t0
        c = ens.counters()
        rec = {"seconds": sec, "nni": int(ens.total_newton_iters()), "rounds": int(ens.total_rounds()), "finished": int(finished),
               **{k: int(c[k].sum()) for k in ("nst", "nli", "ncfl", "npe", "nps")}}
        ens.close()
        return rec

    for mode in (("schedule", "stream") if kind == "heat1d" else ("schedule",)):
        stream = mode == "stream"
        runs = {False: [], True: []}
        for rep in range(reps + 1):  # the first pass of each variant warms the code objects up and is dropped
            for rounds in (False, True):
                r = timed(rounds, stream)
                if rep > 0:
                    runs[rounds].append(r)
        out = dict(base, mode=mode, reps=reps)
        if stream:
            out["stream_rounds"] = stream_rounds
        else:
            out["horizon"] = float(touts[-1])
        for rounds, name in ((False, "host_stepper"), (True, "device_rounds")):
            secs = sorted(r["seconds"] for r in runs[rounds])
            last = runs[rounds][-1]
            out[name] = {"seconds_median": round(float(np.median(secs)), 5), "seconds_min": round(secs[0], 5), "seconds_max": round(secs[-1], 5),
                         "newton_iters_per_s_median": round(last["nni"] / float(np.median(secs)), 1),
                         **{k: last[k] for k in ("nni", "rounds", "finished", "nst", "nli", "ncfl", "npe", "nps")}}
        h, d = out["host_stepper"], out["device_rounds"]
        out["device_minus_host_seconds"] = round(d["seconds_median"] - h["seconds_median"], 5)
        out["host_spread_seconds"] = round(h["seconds_max"] - h["seconds_min"], 5)
        out["host_over_device"] = round(h["seconds_median"] / d["seconds_median"], 3)
        print(json.dumps(out), flush=True)
    ctx.close()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--json", default=None)
    ap.add_argument("--cases", nargs="+", default=["heat", "linear"], choices=["heat", "linear"])
    ap.add_argument("--outputs", type=int, default=1, help="outputs of the case's schedule to integrate to (1: heat 0.01, linear dense 0.1)")
    ap.add_argument("--limit", type=int, default=300, help="seconds granted to each (case, solver) child")
    ap.add_argument("--small", action="store_true", help="toy sizes: a rehearsal of the script, not a measurement")
    ap.add_argument("--rounds", action="store_true", help="the Krylov ctx of each case on the host stepper against the device lock-step rounds, alternating")
    ap.add_argument("--reps", type=int, default=7, help="--rounds: timed repetitions of each variant")
    ap.add_argument("--stream-rounds", type=int, default=120, help="--rounds, heat: rounds of the idaens_stream figure")
    ap.add_argument("--one", nargs=2, default=None, help=argparse.SUPPRESS)
    a = ap.parse_args()
    if a.one and a.rounds:
        return rounds_ab(a.one[0], a.outputs, a.small, a.reps, a.stream_rounds)
    if a.one:
        return one(a.one[0], a.one[1], a.outputs, a.small)
    lines = []
    for case, (_, _, _, solvers) in (SMALL if a.small else CASES).items():
        if case not in a.cases:
            continue
        for solver in (("rounds_ab",) if a.rounds else solvers):
            cmd = ["timeout", "-k", "10", str(a.limit), sys.executable, os.path.abspath(__file__), "--one", case, solver, "--outputs", str(a.outputs)]
            if a.rounds:
                cmd += ["--rounds", "--reps", str(a.reps), "--stream-rounds", str(a.stream_rounds)]
            if a.small:
                cmd.append("--small")
            r = subprocess.run(cmd, capture_output=True, text=True)
            sys.stdout.write(r.stdout)
            sys.stdout.flush()
            lines += [l for l in r.stdout.splitlines() if l.startswith("{")]
            if r.returncode != 0:  # the chain ends here: nothing more is started on the device
                sys.stderr.write(r.stderr[-2000:])
                print(json.dumps({"case": case, "solver": solver, "failed": r.returncode}), flush=True)
                lines.append(json.dumps({"case": case, "solver": solver, "failed": r.returncode}))
                if a.json:
                    open(a.json, "w").write("\n".join(lines) + "\n")
                return 1
    if a.json:
        open(a.json, "w").write("\n".join(lines) + "\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
