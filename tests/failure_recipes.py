"""Recipes that drive the steppers through their failure and recovery paths, and an oracle-side census of the path each one takes.

TEST INFRASTRUCTURE ONLY (a helper module like band_problems.py, no conftest). The standard schedules of linear_dense and heat1d
finish without one failed attempt, so the restore kernel, the three branches of handle_n_flag, the ERR_FAIL exit and the rescaling
of phi[1] after a failure before the first step never ran under a test on the device lock-step stepper. Two constructions change that
without a new problem kind:

  jump        oracle::LinearDense does not own A, B, c: OracleIda._keep[4..6] are the arrays it reads, so editing them in place between
              two solve calls changes the oracle's problem exactly as Ctx.set_linear_dense changes the product's. The step size and
              order the controller had settled on no longer fit and the next step fails its error test several times in a row.
  first step  y'(0) = 0 (not consistent) with a first tout far away: h0 = 0.001 * tout is far too long and the attempts before the
              first step fail (quirk Q5: reset() rescales phi[1] only).

A case is a plain dict: the problem (idahip.problems' dict shape), the systems the recipe is applied to (`edited`; the others are the
untouched neighbours every batch keeps), the touts before and after the jump, the optional mxstep, and `expect`, the path the case is
named for. tests/test_failure_recipes.py asserts with `census` -- on the oracle alone -- that every case the GPU tests use really
takes that path; tests/test_gpu_failure_paths.py compares the product with the oracle on them."""
import numpy as np

import oracle_lib as O

ONE_STEP = 1
T_JUMP = 0.3
BEFORE = [0.1, 0.2, 0.3]

# name -> (edit, expect). An edit is ("scale", field, factor) or ("zero_column", j); expect is the path of the step after the jump:
#   deep      >= 3 error-test failures inside one step (the third forces order 1), final status 0
#   second    >= 2 error-test failures inside one step, final status 0
#   terminal  status -3 (ERR_FAIL) with exactly 10 failures in the step
#   mixed     both of the above in one batch
#   singular  the linear setup fails at every attempt of the step (recoverable each time, then fatal)
JUMPS = {
    "A*3": (("scale", "A", 3.0), "deep"),
    "A*0.01": (("scale", "A", 0.01), "deep"),
    "c*1.0001": (("scale", "c", 1.0001), "second"),
    "c*1.01": (("scale", "c", 1.01), "deep"),
    "B*1.5": (("scale", "B", 1.5), "mixed"),
    "c*-20": (("scale", "c", -20.0), "terminal"),
    "zero_column": (("zero_column", 5), "singular"),
}


# What tests/test_gpu_failure_paths.py runs (and tests/test_failure_recipes.py therefore checks on the oracle):
# jumps on both lock-step steppers: n = 24 (one wavefront per vector kernel), 200 (several), 704 (workgroup-per-matrix panels of the LU),
# 1100 (the large-n pipeline: the LU list's length is read back)
GPU_JUMPS = [("A*3", 24), ("c*1.01", 24), ("B*1.5", 24), ("c*-20", 24), ("A*3", 200), ("c*1.01", 200), ("B*1.5", 200), ("c*-20", 200),
             ("c*1.01", 704), ("c*-20", 704), ("c*1.01", 1100), ("c*-20", 1100)]
LONG_JUMP = ("A*0.01", 24)  # about 1800 steps and up to a hundred error-test failures per system, to t = 1
# (kind, n, first tout, expect)
GPU_FIRST_STEPS = [("linear_dense", 24, 1.0, "recover"), ("linear_dense", 200, 1.0, "recover"), ("linear_dense", 704, 1.0, "recover"),
                   ("heat1d", 40, 1.0e2, "recover"), ("heat1d", 1100, 1.0, "recover"), ("lorenz63", 3, 1.0, "recover"),
                   ("linear_dense", 24, 1.0e2, "first_terminal"), ("heat1d", 40, 1.0e4, "first_terminal"),
                   ("lorenz63", 3, 1.0e4, "first_terminal")]
BAND_FIRST_STEPS = [(257, (1, 1)), (257, (2, 3))]  # heat1d, y'(0) = 0, first tout 1.0, on a band ctx
DQ_FIRST_STEPS = [("heat1d", 257), ("linear_dense", 24)]
SINGULAR_SIZES = [200, 704, 1100]
SINGULAR_BAND = (257, 2, 3)  # band_problems.banded_linear through band callbacks


def batch_of(n):
    return 5 if n <= 256 else 4 if n <= 1024 else 3


def edited_of(n):
    """The systems a recipe is applied to: the first ones; the last (two) of the batch stay untouched."""
    return [0, 1, 2] if n <= 1024 else [0, 1]


def edit_arrays(edit, A, B, c):
    """Apply an edit IN PLACE to arrays of one system or of several ([..., n, n] column-major, [..., n])."""
    if edit[0] == "scale":
        {"A": A, "B": B, "c": c}[edit[1]][...] *= edit[2]
    elif edit[0] == "zero_column":  # storage is [col][row]: column j of A and of B, so that B + cj A is singular for every cj
        A[..., edit[1], :] = 0.0
        B[..., edit[1], :] = 0.0
    else:
        raise ValueError(edit)


def jump_case(name, n, after=None, mxstep=None):
    """linear_dense(n): integrate to T_JUMP, apply JUMPS[name] to the systems `edited`, integrate on to the touts `after` (default:
    0.4 and 0.5, at n > 256 only 0.4)."""
    from idahip import problems
    edit, expect = JUMPS[name]
    p = problems.linear_dense(n=n, batch=batch_of(n), procs=1)
    if after is None:
        after = (0.4,) if n > 256 else (0.4, 0.5)
    return {"name": "%s n=%d" % (name, n), "prob": p, "edited": edited_of(n), "edit": edit, "expect": expect, "before": list(BEFORE),
            "after": [float(t) for t in after], "mxstep": mxstep}


# repeated jump: Newton's restart with a stale Jacobian (ConvergenceRecover, then a setup and the iterations again; newton.rs:146-152),
# several times per system. After the three quiet touts A is scaled by 3 and by 1/3 alternately before each of eight further touts 0.05
# apart: the Jacobian a system holds is that of another A every time. tests/test_gpu_newton_restarts.py runs it at these sizes.
REPEATED_SIZES = [24, 200]
REPEATED_TOUTS = [T_JUMP + 0.05 * k for k in range(1, 9)]


def repeated_jump_case(n):
    """linear_dense(n), batch of five: `edits` maps the index of a tout to the edit made before it, for the systems `edited`."""
    from idahip import problems
    p = problems.linear_dense(n=n, batch=batch_of(n), procs=1)
    edits = {len(BEFORE) + k: ("scale", "A", 3.0 if k % 2 == 0 else 1.0 / 3.0) for k in range(len(REPEATED_TOUTS))}
    return {"name": "A*3, A/3 repeated n=%d" % n, "prob": p, "edited": edited_of(n), "edit": None, "edits": edits, "expect": "restarts",
            "before": list(BEFORE), "after": list(REPEATED_TOUTS), "mxstep": None}


def apply_edits_to_ctx(ctx, case, i, cur):
    """The edit a repeated-jump case makes before tout i (if any), through idahip_set_linear_dense. cur: {system: (A, B, c)}, the arrays
    as edited so far -- filled here with copies on first use, edited in place like the oracle's."""
    edit = case.get("edits", {}).get(i)
    if edit is None:
        return
    p = case["prob"]
    for s in case["edited"]:
        if s not in cur:
            cur[s] = (p["A"][s:s + 1].copy(), p["B"][s:s + 1].copy(), p["c"][s:s + 1].copy())
        edit_arrays(edit, *cur[s])
        ctx.set_linear_dense(*cur[s], first=s)


def singular_case(n, when, band=None, only=None):
    """One system of the batch (system 1) gets an exactly zero column in A and in B: from the start, or at T_JUMP ("mid").
    band = (ml, mu): band_problems.banded_linear instead of linear_dense, for a band ctx with host callbacks.
    only: keep these systems of the batch and edit none (the run without the failing system)."""
    from idahip import problems
    import band_problems as BP
    p = problems.linear_dense(n=n, batch=batch_of(n), procs=1) if band is None else BP.banded_linear(n, band[0], band[1], 4)
    if only is not None:
        p = sub_problem(p, only)
    if band is not None:
        p = BP.as_host_callback(p)
    mid = when == "mid"
    return {"name": "zero column n=%d %s" % (n, when), "prob": p, "edited": [1] if only is None else [], "edit": JUMPS["zero_column"][0], "expect": "singular",
            "before": list(BEFORE) if mid else [], "after": [0.4] if mid else [0.1], "mxstep": None}


def apply_to_oracle(o, edit):
    """The edit on the arrays one OracleIda reads (its problem does not own them)."""
    edit_arrays(edit, o._keep[4], o._keep[5], o._keep[6])


def apply_to_ctx(ctx, case):
    """The same edit through idahip_set_linear_dense, for the edited systems only. A host-callback problem (band_problems) reads
    the case's own arrays at every call: there the edit is made in place, so build such a case anew for every run."""
    p = case["prob"]
    if p["kind"] == "host_callback":
        for s in case["edited"]:
            edit_arrays(case["edit"], p["A"][s], p["B"][s], p["c"][s])
        return
    for s in case["edited"]:
        A, B, c = p["A"][s:s + 1].copy(), p["B"][s:s + 1].copy(), p["c"][s:s + 1].copy()
        edit_arrays(case["edit"], A, B, c)
        ctx.set_linear_dense(A, B, c, first=s)


def first_step_case(kind, n, tout, batch=None, later=(), expect="recover", edited=None):
    """y'(0) = 0 for the systems `edited` (default: all but the last two of a small batch, two of three in a large one) and a first
    tout so far away that the attempts before the first step fail.
    expect: recover (failures at nst == 0, then the integration goes on) or first_terminal (-3 at nst == 0)."""
    from idahip import problems
    if kind == "linear_dense":
        p = problems.linear_dense(n=n, batch=batch or batch_of(n), procs=1)
    elif kind == "heat1d":
        p = problems.heat1d(n=n, batch=batch or batch_of(n))
    else:
        p = problems.lorenz63(batch=batch or 64)
    B = p["yy0"].shape[0]
    if edited is None:
        edited = list(range(0, B - 2)) if B <= 8 else [b for b in range(B) if b % 3 != 2]
    p = dict(p, yp0=p["yp0"].copy())
    p["yp0"][edited] = 0.0
    return {"name": "%s n=%d yp0=0 tout=%g" % (kind, p["n"], tout), "prob": p, "edited": edited, "edit": None, "expect": expect, "before": [],
            "after": [float(tout)] + [float(t) for t in later], "mxstep": None}


def too_much_acc_case(kind):
    """rtol = 1e-17, atol = 1e-20: tolsf > 1 at the first loop-top check, TOO_MUCH_ACC (-2) at nst == 0 for every system."""
    from idahip import problems
    p = problems.linear_dense(n=24, batch=5, procs=1) if kind == "linear_dense" else problems.lorenz63(batch=64)
    p = dict(p, rtol=1.0e-17, atol=np.array([1.0e-20]))
    return {"name": "%s too much accuracy" % kind, "prob": p, "edited": list(range(p["yy0"].shape[0])), "edit": None, "expect": "too_much_acc",
            "before": [], "after": [float(p["touts"][0])], "mxstep": None}


def sub_problem(p, ids):
    """The systems `ids` of a problem dict as a problem of their own."""
    B = p["yy0"].shape[0]
    return {k: (v[ids] if isinstance(v, np.ndarray) and v.ndim >= 1 and v.shape[0] == B and k not in ("atol", "touts") else v)
            for k, v in p.items()}


def oracle_of(p, s):
    """One OracleIda for system s of a problem dict, with copies of its arrays (an edit touches this object only)."""
    kw = {}
    if p.get("params") is not None:
        kw["params"] = np.array(p["params"][s], dtype=np.float64)
    for k in ("A", "B", "c"):
        if p.get(k) is not None:
            kw[k] = np.array(p[k][s], dtype=np.float64)
    kind = p["kind"] if p["kind"] != "host_callback" else p["oracle_kind"]
    return O.OracleIda(kind, p["n"], p["yy0"][s], p["yp0"][s], p["rtol"], p["atol"], **kw)


def census(case, systems=None):
    """Drive the oracle through the case step by step (ONE_STEP after the jump) and count what happened, per system of `systems`
    (default: the edited ones) -> list of dicts:
      status        the last return of solve
      max_etf       the most error-test failures inside one step after the jump
      max_cf        the most convergence-type failures (Newton or linear setup) inside one step after the jump
      nfail_first   failures while nst == 0
      min_k         the lowest order of a step taken after the jump
      nst_jump, nst, netf, ncfn   step count at the jump; step and failure counts at the end"""
    out = []
    t_end = case["after"][-1]
    for s in (case["edited"] if systems is None else systems):
        o = oracle_of(case["prob"], s)
        if case["mxstep"]:
            o.set("mxstep", case["mxstep"])
        for t in case["before"]:
            assert o.solve(t)[0] == 0, (case["name"], s, t)
        if case["edit"] is not None and s in case["edited"]:
            apply_to_oracle(o, case["edit"])
        r = {"sys": s, "nst_jump": int(o.get("nst")), "max_etf": 0, "max_cf": 0, "nfail_first": 0, "min_k": 99, "status": 0}
        for _ in range(1000000):
            nst0, etf0, cf0 = int(o.get("nst")), int(o.get("netf")), int(o.get("ncfn"))
            st, tret = o.solve(case["after"][0] if nst0 == 0 else t_end, itask=ONE_STEP)
            nst1, d_etf, d_cf = int(o.get("nst")), int(o.get("netf")) - etf0, int(o.get("ncfn")) - cf0
            r["max_etf"], r["max_cf"] = max(r["max_etf"], d_etf), max(r["max_cf"], d_cf)
            if nst0 == 0:
                r["nfail_first"] += d_etf + d_cf
            if nst1 > nst0:
                r["min_k"] = min(r["min_k"], int(o.get("kused")))
            r["status"] = st
            if st != 0 or tret >= t_end:
                break
        r.update(nst=int(o.get("nst")), netf=int(o.get("netf")), ncfn=int(o.get("ncfn")))
        out.append(r)
    return out


REF_COUNTERS = ("nst", "nre", "nje", "nsetups", "nni", "netf", "ncfn", "n_attempts", "nls_nconvfails")


def oracle_reference(case, nthreads=16):
    """The case as the product's caller runs it -- Ida::solve(tout) in NORMAL mode for every tout, the edit between the last tout before
    and the first one after the jump -- for EVERY system of the batch, one oracle object each. A system whose call returned a fatal
    error is left alone from then on and keeps reporting that return (include/ida_ensemble.h: a negative status is sticky;
    TOO_MUCH_WORK, -1, is the exception: the next call continues).
    -> dict: status [ntout][B], tret [ntout][B], yy / yp [ntout][B][n] at every tout; counters {name: [B]}, kused, hused [B] at the
    end; nfail_first [B]: the failures of a first step taken alone (ONE_STEP with the first tout) on a second object."""
    from concurrent.futures import ThreadPoolExecutor
    p = case["prob"]
    B, n = p["yy0"].shape
    touts = case["before"] + case["after"]
    T = len(touts)
    ref = {"status": np.zeros((T, B), dtype=np.int32), "tret": np.zeros((T, B)), "yy": np.zeros((T, B, n)), "yp": np.zeros((T, B, n)),
           "counters": {k: np.zeros(B, dtype=np.int64) for k in REF_COUNTERS}, "kused": np.zeros(B, dtype=np.int64),
           "hused": np.zeros(B), "nfail_first": np.zeros(B, dtype=np.int64)}

    def one(s):
        first = oracle_of(p, s)
        if case["edit"] is not None and not case["before"] and s in case["edited"]:
            apply_to_oracle(first, case["edit"])
        first.solve(touts[0], itask=ONE_STEP)
        ref["nfail_first"][s] = int(first.get("netf")) + int(first.get("ncfn"))
        o = oracle_of(p, s)
        if case["mxstep"]:
            o.set("mxstep", case["mxstep"])
        dead = False
        for i, t in enumerate(touts):
            if i == len(case["before"]) and case["edit"] is not None and s in case["edited"]:
                apply_to_oracle(o, case["edit"])
            if i in case.get("edits", {}) and s in case["edited"]:
                apply_to_oracle(o, case["edits"][i])
            if not dead:
                st, tret = o.solve(t)
                rec = (st, tret, o.getv("yy"), o.getv("yp"))
                dead = st < 0 and st != -1
            ref["status"][i, s], ref["tret"][i, s], ref["yy"][i, s], ref["yp"][i, s] = rec
        c = o.counters()
        for k in REF_COUNTERS:
            ref["counters"][k][s] = c[k]
        ref["kused"][s], ref["hused"][s] = int(o.get("kused")), o.get("hused")

    O.lib()
    with ThreadPoolExecutor(max(1, min(nthreads, B))) as pool:  # the oracle's calls release the interpreter lock
        list(pool.map(one, range(B)))
    return ref


def jump_after_attempts(case, touts, attempts, one_step=False, nthreads=16):
    """The jump inside a round-limited schedule, on the oracle: a lock-step round is one step attempt of every system, so after
    `attempts` rounds every system has made that many attempts -- here ONE_STEP calls, every one a step (asserted: no attempt fails
    before the jump, and no tout has been passed) --, then the edit, then Ida::solve(tout) for every tout.
    -> the dict of oracle_reference (without nfail_first); one_step=True: the census rows of the edited systems instead, the run
    continued step by step to touts[-1]."""
    from concurrent.futures import ThreadPoolExecutor
    p = case["prob"]
    B, n = p["yy0"].shape
    touts = [float(t) for t in touts]
    T = len(touts)
    ref = {"status": np.zeros((T, B), dtype=np.int32), "tret": np.zeros((T, B)), "yy": np.zeros((T, B, n)), "yp": np.zeros((T, B, n)),
           "counters": {k: np.zeros(B, dtype=np.int64) for k in REF_COUNTERS}, "kused": np.zeros(B, dtype=np.int64), "hused": np.zeros(B)}
    rows = {}

    def one(s):
        o = oracle_of(p, s)
        for _ in range(attempts):
            st, tret = o.solve(touts[0], itask=ONE_STEP)
            assert st == 0 and tret < touts[0], (s, st, tret)
        assert int(o.get("n_attempts")) == attempts == int(o.get("nst"))
        if s in case["edited"]:
            apply_to_oracle(o, case["edit"])
        if one_step:
            r = {"sys": s, "nst_jump": attempts, "max_etf": 0, "max_cf": 0, "nfail_first": 0, "min_k": 99, "status": 0}
            while o.get("tn") < touts[-1] and r["status"] == 0:
                etf0, cf0 = int(o.get("netf")), int(o.get("ncfn"))
                r["status"] = o.solve(touts[-1], itask=ONE_STEP)[0]
                r["max_etf"], r["max_cf"] = max(r["max_etf"], int(o.get("netf")) - etf0), max(r["max_cf"], int(o.get("ncfn")) - cf0)
                r["min_k"] = min(r["min_k"], int(o.get("kused")))
            r.update(nst=int(o.get("nst")), netf=int(o.get("netf")), ncfn=int(o.get("ncfn")))
            rows[s] = r
            return
        for i, t in enumerate(touts):
            st, tret = o.solve(t)
            ref["status"][i, s], ref["tret"][i, s], ref["yy"][i, s], ref["yp"][i, s] = st, tret, o.getv("yy"), o.getv("yp")
            assert st == 0, (s, t, st)
        c = o.counters()
        for k in REF_COUNTERS:
            ref["counters"][k][s] = c[k]
        ref["kused"][s], ref["hused"][s] = int(o.get("kused")), o.get("hused")

    O.lib()
    with ThreadPoolExecutor(max(1, min(nthreads, B))) as pool:
        list(pool.map(one, case["edited"] if one_step else range(B)))
    return [rows[s] for s in case["edited"]] if one_step else ref


def meets(expect, rows):
    """Does the census of a case's edited systems show the path the case is named for? -> (bool, reason)"""
    ok0 = [r for r in rows if r["status"] == 0]
    bad = [r for r in rows if r["status"] == -3]
    moved = all(r["nst"] > r["nst_jump"] for r in ok0)
    if expect == "deep":
        return len(ok0) == len(rows) and moved and any(r["max_etf"] >= 3 and r["min_k"] == 1 for r in rows), "status 0, >= 3 failures in a step"
    if expect == "second":
        return len(ok0) == len(rows) and moved and any(r["max_etf"] >= 2 for r in rows), "status 0, >= 2 failures in a step"
    if expect == "terminal":
        return len(bad) == len(rows) and all(r["max_etf"] == 10 for r in rows), "-3 with exactly 10 error-test failures in the step"
    if expect == "mixed":
        return len(ok0) > 0 and len(bad) > 0 and len(ok0) + len(bad) == len(rows) and moved and all(r["max_etf"] == 10 for r in bad) and \
            any(r["max_etf"] >= 3 for r in ok0), "both a recovery and -3 in one batch"
    if expect == "recover":
        return len(ok0) == len(rows) and all(r["nfail_first"] > 0 and r["nst"] > 0 for r in rows), "failures at nst == 0, then recovery"
    if expect == "first_terminal":
        return len(bad) == len(rows) and all(r["nst"] == 0 and r["max_etf"] == 10 and r["nfail_first"] >= 10 for r in rows), "-3 at nst == 0"
    if expect == "singular":
        return all(r["status"] < 0 and r["max_cf"] == 10 and r["nst"] == r["nst_jump"] for r in rows), "10 failed setups in one step"
    if expect == "too_much_acc":
        return all(r["status"] == -2 and r["nst"] == 0 for r in rows), "-2 at nst == 0"
    raise ValueError(expect)
