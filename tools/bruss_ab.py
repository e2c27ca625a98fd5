"""The 1-D Brusselator (IDAHIP_BRUSS1D) at m = 2048 (n = 4096), B = 256, to t = 0.5 on four contexts, on one box
in one call: the dense ctx with the super-panel LU on and off (idahip_set_lu_superpanel), the band ctx (2, 2) and a Krylov ctx with the
(2, 2) band preconditioner. Recorded per run: wall time of idaens_solve_schedule to the horizon (a host clock around a call that ends
in a device synchronise), steps, Newton iterations per second, the device memory the ctx took, and how many systems finished.

The variants alternate: --reps passes over the list dense_sp1, dense_sp0, band, krylov_prec, each run a child process of its own under
`timeout -k 10` that integrates once to warm the code objects up and once for the figure; the chain stops at the first child that
fails. The summary lines give the median and the spread of each variant's timed passes. No threshold is set anywhere: the file is where
the numbers go. One JSON object per line on stdout; --json also writes them to a file.

    python tools/bruss_ab.py [--json profiles/bruss_ab.json] [--reps 3] [--limit 300] [--small]
"""
import argparse
import json
import os
import socket
import statistics
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "rust-ida_amd"))

VARIANTS = ("dense_sp1", "dense_sp0", "band", "krylov_prec")
FULL, SMALL = (2048, 256), (128, 16)
HORIZON = 0.5
SUMS = ("nst", "nni", "nli", "ncfl", "ncfn", "netf", "nsetups", "nje", "nre", "nre_dq", "npe", "nps")


def one(variant, small, rep):
    import torch
    import idahip
    from idahip import problems
    m, batch = SMALL if small else FULL
    p = problems.bruss1d(m=m, batch=batch)
    torch.cuda.init()
    free0 = torch.cuda.mem_get_info()[0]
    ctx = problems.make_ctx(p, band=(variant == "band"), krylov=(0 if variant == "krylov_prec" else None))
    if variant == "krylov_prec":
        ctx.set_krylov_band_prec(2, 2)
    if variant.startswith("dense"):
        ctx.set_lu_superpanel(1 if variant == "dense_sp1" else 0)
    mem = free0 - torch.cuda.mem_get_info()[0]
    for timed in (0, 1):  # the first pass warms the code objects up; the second is the figure
        ens = idahip.Ensemble(ctx, p["yy0"], p["yp0"])
        ctx.H.idahip_sync(ctx.h)
        t0 = time.perf_counter()
        status, tret, reached = ens.solve_schedule([HORIZON])
        ctx.H.idahip_sync(ctx.h)
        sec = time.perf_counter() - t0
        c = ens.counters()
        rec = {"variant": variant, "m": m, "n": 2 * m, "batch": batch, "rep": rep, "timed": timed, "horizon": HORIZON,
               "seconds": round(sec, 4), "steps": int(c["nst"].sum()), "newton_iters_per_s": round(float(c["nni"].sum()) / sec, 1),
               "device_controller": ens.device_controller_active(), "ctx_device_bytes": int(mem), "finished": int((status == 0).sum()),
               **{k: int(c[k].sum()) for k in SUMS}, "host": socket.gethostname(),
               "command": "python tools/bruss_ab.py%s" % (" --small" if small else "")}
        ens.close()
        print(json.dumps(rec), flush=True)
    ctx.close()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--json", default=None)
    ap.add_argument("--reps", type=int, default=3, help="passes over the list of variants")
    ap.add_argument("--limit", type=int, default=300, help="seconds granted to each child")
    ap.add_argument("--small", action="store_true", help="toy sizes: a rehearsal of the script, not a measurement")
    ap.add_argument("--one", nargs=2, default=None, help=argparse.SUPPRESS)
    a = ap.parse_args()
    if a.one:
        return one(a.one[0], a.small, int(a.one[1]))
    lines, rc = [], 0

    def emit(obj):
        s = json.dumps(obj)
        print(s, flush=True)
        lines.append(s)

    for rep in range(a.reps):
        for variant in VARIANTS:
            cmd = ["timeout", "-k", "10", str(a.limit), sys.executable, os.path.abspath(__file__), "--one", variant, str(rep)]
            if a.small:
                cmd.append("--small")
            r = subprocess.run(cmd, capture_output=True, text=True)
            sys.stdout.write(r.stdout)
            sys.stdout.flush()
            lines += [l for l in r.stdout.splitlines() if l.startswith("{")]
            if r.returncode != 0:  # the chain ends here: nothing more is started on the device
                sys.stderr.write(r.stderr[-2000:])
                emit({"variant": variant, "rep": rep, "failed": r.returncode})
                rc = 1
                break
        if rc:
            break
    recs = [json.loads(l) for l in lines]
    for variant in VARIANTS:
        t = [r["seconds"] for r in recs if r.get("variant") == variant and r.get("timed") == 1]
        if t:
            last = [r for r in recs if r.get("variant") == variant and r.get("timed") == 1][-1]
            emit({"summary": variant, "passes": len(t), "seconds_median": round(statistics.median(t), 4), "seconds_min": min(t),
                  "seconds_max": max(t), "steps": last["steps"], "nni": last["nni"],
                  "newton_iters_per_s_median": round(last["nni"] / statistics.median(t), 1), "ctx_device_bytes": last["ctx_device_bytes"],
                  "finished": last["finished"], "batch": last["batch"]})
    if a.json:
        open(a.json, "w").write("\n".join(lines) + "\n")
    return rc


if __name__ == "__main__":
    sys.exit(main())
