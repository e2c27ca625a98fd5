#!/usr/bin/env python3
"""Development tool (GPU box): device time of one batched setup (idahip_nls_lsetup) and one Newton iteration (idahip_newton_iter)
of config-3 matrices with the ctx's factors staged (idahip_set_lu_staged) and in the reference layout, alternating, one library.
usage: python tools/lu_staged_ab.py [n] [batch] [reps]   -- class timers in ms per call; run-to-run variation is a few per cent."""
import os, sys
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "rust-ida_amd"))
import numpy as np
import idahip
from idahip import problems

KEYS = ("lu", "lu_panel", "lu_trail", "lu_finalize", "newton_iter")


def main():
    n = int(sys.argv[1]) if len(sys.argv) > 1 else 512
    B = int(sys.argv[2]) if len(sys.argv) > 2 else 1312
    reps = int(sys.argv[3]) if len(sys.argv) > 3 else 4
    p = problems.linear_dense(n=n, batch=B, procs=int(os.environ.get("IDAHIP_GEN_PROCS", "16")))
    ctxs = {}
    for on in (0, 1):
        ctx = problems.make_ctx(p)
        ctx.set_lu_staged(bool(on))
        ctx.upload(idahip.F_YY, p["yy0"]); ctx.upload(idahip.F_YP, p["yp0"])
        ctx.upload(idahip.F_EWT, np.ones((B, n)))
        ctx.timing(True)
        ctxs[on] = ctx
    rhs = np.random.Generator(np.random.PCG64(1)).standard_normal((B, n))
    for r in range(reps + 1):  # (the first repetition warms up and is not printed)
        for on in (0, 1):
            ctx = ctxs[on]
            ctx.upload(idahip.F_DELTA, rhs)
            ctx.timing_reset()
            rc, info = ctx.nls_lsetup(0.0, 100.0)
            ctx.newton_iter(1.0)
            t = ctx.timing_get()
            if r:
                print("n %d batch %d rep %d staged %d: " % (n, B, r, on) + "  ".join("%s %.3f" % (k, t[k]["ms"]) for k in KEYS)
                      + "  lu+newton %.3f  info_any=%d" % (t["lu"]["ms"] + t["newton_iter"]["ms"], int(info.any())))


if __name__ == "__main__":  # (the input generator starts worker processes that import this module)
    main()
