"""The cases of the stop-time and masked-norm tests, shared by the CPU census (tests/test_tstop_oracle.py) and the GPU tests
(tests/test_gpu_stop_time.py, tests/test_gpu_suppress_alg.py). TEST INFRASTRUCTURE ONLY.

A run is driven through a small interface -- stop(values), stop_rel(frac, ids), solve(tout, itask) -> statuses, stop_times() -- that
the harness (HarnessDriver here) and the product (the GPU tests' driver) both implement, so both follow the same sequence of calls.
"""
import numpy as np

import tstop_oracle as T

NAN = float("nan")
# stop times by b % 7, in units of the first tout: none, inside the first call, tiny (the first step is clipped), the first tout itself,
# between the second and the third tout, far beyond the last, behind t0
RESIDUES = (None, 0.25, 1e-9, 1.0, 3.0, 1e6, -1.0)


def roberts_batch(batch):
    """The reference's Roberts example and consistently perturbed copies of it (y1 + y2 + y3 = 1 kept)."""
    from idahip import problems
    p = problems.roberts()
    rng = np.random.Generator(np.random.PCG64(5))
    y0 = np.tile(p["yy0"], (batch, 1))
    y0[1:, 0] -= 1e-3 * rng.uniform(0, 1, batch - 1)
    y0[1:, 2] = 1.0 - y0[1:, 0] - y0[1:, 1]
    yp0 = np.stack([-0.04 * y0[:, 0] + 1e4 * y0[:, 1] * y0[:, 2], 0.04 * y0[:, 0] - 1e4 * y0[:, 1] * y0[:, 2] - 3e7 * y0[:, 1] ** 2,
                    np.zeros(batch)], axis=1)
    yp0[:, 2] = -(yp0[:, 0] + yp0[:, 1])
    p.update(yy0=y0, yp0=yp0)
    return p


def third_algebraic(n):
    """id_i = 0 where i % 3 == 2: the true algebraic components of these problems change no step at short horizons."""
    return (np.arange(n) % 3 != 2).astype(np.float64)


def _problem(name):
    from idahip import problems
    if name == "roberts":
        return roberts_batch(70), [0.4, 0.8, 1.6], np.array([1.0, 1.0, 0.0])
    if name == "linear12":
        return problems.linear_dense(n=12, batch=5), [0.1, 0.2, 0.4], third_algebraic(12)
    if name == "linear300":
        return problems.linear_dense(n=300, batch=3), [0.1, 0.2, 0.4], third_algebraic(300)
    if name == "heat20":
        return problems.heat1d(n=20, batch=3), [0.1, 0.2, 0.4], third_algebraic(20)
    raise KeyError(name)


PROBLEMS = ("roberts", "linear12", "linear300", "heat20")
_CACHE = {}


def problem(name):
    if name not in _CACHE:
        _CACHE[name] = _problem(name)
    return _CACHE[name]


# ------------------------------------------------------------------------------------------------ masked norms
MASK_CASES = PROBLEMS
# steps at the first return (tout = touts[0]), unmasked and masked, of the systems the figures were taken for
MEASURED = {"linear12": {0: (34, 32), 1: (36, 35)}, "linear300": {0: (34, 33), 1: (36, 33)}, "heat20": {0: (31, 32)}, "roberts": {0: (27, 22)}}


def mask_case(name):
    prob, touts, id = problem(name)
    return {"name": name, "prob": prob, "touts": touts, "id": id, "roots": name == "roberts"}


# ------------------------------------------------------------------------------------------------ stop times
STOP_CASES = PROBLEMS + ("entry", "linear12_masked")


def stop_case(name):
    """how: the harness' switches; script: "residues" (per-system stop times by b % 7) or "entry" (stop times set between calls,
    at and just beyond tn, in both tasks)."""
    if name == "entry":
        prob, touts, _ = problem("linear12")
        return {"name": name, "prob": prob, "touts": touts, "how": {}, "script": "entry", "id": None}
    if name == "linear12_masked":
        prob, touts, id = problem("linear12")
        return {"name": name, "prob": prob, "touts": touts, "how": {"id": id, "suppress": True}, "script": "residues", "id": id}
    prob, touts, _ = problem(name)
    return {"name": name, "prob": prob, "touts": touts, "how": {}, "script": "residues", "id": None}


def drive(case, d):
    """Run the case's script on driver d. -> the ops it made, in order (for a replay on another driver)."""
    B = case["prob"]["yy0"].shape[0]
    touts = case["touts"]
    ops = []

    def stop(v):
        ops.append(("stop", None if v is None else np.array(v, dtype=np.float64)))
        d.stop(v)

    def stop_rel(frac):
        ops.append(("stop_rel", frac, list(range(B))))
        d.stop_rel(frac, list(range(B)))

    def solve(t, itask=T.NORMAL):
        ops.append(("solve", float(t), itask))
        return d.solve(float(t), itask)

    def until_done(t):  # at most four calls per tout, until every system reports SUCCESS or a negative status
        for _ in range(4):
            st = solve(t)
            if ((st == T.SUCCESS) | (st < 0)).all():
                break
        return st

    if case["script"] == "residues":
        t1 = touts[0]
        stop(T.by_residue(B, [None if r is None else r * t1 for r in RESIDUES]))
        st = until_done(t1)
        behind = np.arange(B) % 7 == 6
        assert np.array_equal(st == T.ILL_INPUT, behind), st  # a stop time behind t0: the system has not started
        if behind.any():
            cur = d.stop_times()
            cur[behind] = NAN
            stop(cur)  # clear theirs, keep the others'
            until_done(t1)
        for t in touts[1:]:
            until_done(t)
    else:
        t1, t2, t3 = touts[0], 2 * touts[0], 3 * touts[0]
        assert (solve(t1) == T.SUCCESS).all()
        stop_rel(0.5)            # just beyond tn: stop_test1 clips hh at the entry of the next call
        assert (solve(t2) == T.TSTOP_RETURN).all()
        assert (solve(t2) == T.SUCCESS).all()
        stop_rel(0.0)            # tn itself: TSTOP at the entry of the next call, no step taken
        assert (solve(t3) == T.TSTOP_RETURN).all()
        assert (solve(t3) == T.SUCCESS).all()
        for _ in range(3):
            solve(t3 * 10, T.ONE_STEP)
        stop_rel(0.0)            # the same in IDA_ONE_STEP: quirk Q15, the stop time is consumed
        assert (solve(t3 * 10, T.ONE_STEP) == T.TSTOP_RETURN).all()
        assert np.isnan(d.stop_times()).all()
        for _ in range(2):
            assert (solve(t3 * 10, T.ONE_STEP) == T.SUCCESS).all()
        stop_rel(0.3)            # inside the next step: clipped at the entry, TSTOP after the step
        assert (solve(t3 * 10, T.ONE_STEP) == T.TSTOP_RETURN).all()
        assert (solve(t3 * 10, T.ONE_STEP) == T.SUCCESS).all()
        stop(None)
        solve(t3 * 10, T.ONE_STEP)
    return ops


class HarnessDriver:
    def __init__(self, case, ids=None):
        prob = case["prob"]
        self.ids = list(range(prob["yy0"].shape[0])) if ids is None else list(ids)
        self.B = prob["yy0"].shape[0]
        self.hs = [T.Harness(prob, s, **case["how"]) for s in self.ids]

    def stop(self, v):
        for q, h in enumerate(self.hs):
            h.set_stop_time(None if v is None else np.broadcast_to(v, (self.B,))[self.ids[q]])

    def stop_rel(self, frac, ids):
        for q, h in enumerate(self.hs):
            if self.ids[q] in ids:
                h.set_stop_time(h.get("tn") + frac * h.get("hh"))

    def stop_times(self):
        return np.array([h.stop_time() for h in self.hs])

    def solve(self, tout, itask):
        return np.array([h.solve(tout, itask)[0] for h in self.hs], dtype=np.int32)


def ops_on_harness(case):
    """The case's ops as the harness itself drives them (the CPU census; the GPU tests replay the product's ops instead)."""
    return drive(case, HarnessDriver(case))


# ------------------------------------------------------------------------------------------------ the product behind the same interface
INT_FIELDS = ("kused", "nst", "nre", "nni", "netf", "ncfn", "nsetups")


class ProductDriver:
    """An idahip.Ensemble behind drive()'s interface; keeps one record per solve call, shaped like tstop_oracle.run_ops' records."""

    def __init__(self, ens):
        self.ens = ens
        self.rec = []

    def stop(self, v):
        self.ens.set_stop_time(v)

    def stop_rel(self, frac, ids):
        cur, tn, hh = self.ens.stop_time(), self.ens.real("tn"), self.ens.real("hh")
        cur[ids] = tn[ids] + frac * hh[ids]
        self.ens.set_stop_time(cur)

    def stop_times(self):
        return self.ens.stop_time()

    def solve(self, tout, itask):
        e = self.ens
        before = e.stop_time()
        st, tret = e.solve(tout, itask=itask)
        r = {"status": st.copy(), "tret": tret.copy(), "yy": e.yy(), "yp": e.yp(), "tstop": e.stop_time(), "tstop_before": before}
        for k in ("tn", "hh", "hused"):
            r[k] = e.real(k)
        for k in INT_FIELDS:
            r[k] = e.counter(k)
        self.rec.append(r)
        return st


def compare(got, want, by_value=False, what=""):
    """The product's records against the harness': status, tret, yy, yp, tn, hh, hused, kused, nst, nre, nni, netf, ncfn, nsetups and
    the stop time left, per call; bit for bit (by_value: yy and yp by value -- a band ctx against the oracle's dense solver)."""
    import stepper_ref as R
    assert len(got) == len(want), (len(got), len(want))
    for i, (g, w) in enumerate(zip(got, want)):
        print(what, "call", i, "status", g["status"].tolist(), "tret", g["tret"].tolist(), "nst", g["nst"].tolist())
        assert np.array_equal(g["status"], w["status"]), (what, i, g["status"], w["status"])
        assert R.same_bits(g["tret"], w["tret"]), (what, i, g["tret"], w["tret"])
        for k in ("tn", "hh", "hused", "tstop"):
            assert R.same_bits(g[k], w[k]), (what, i, k, g[k], w[k])
        for k in INT_FIELDS:
            assert np.array_equal(g[k], w[k].astype(np.int64)), (what, i, k, g[k], w[k])
        for k in ("yy", "yp"):
            assert np.array_equal(g[k], w[k]) if by_value else R.same_bits(g[k], w[k]), (what, i, k)
        # no step has gone beyond the stop time it was taken under
        ts = g["tstop_before"]
        on = ~np.isnan(ts) & (g["nst"] > 0)
        assert ((g["tn"][on] - ts[on]) * g["hused"][on] <= 0.0).all(), (what, i, g["tn"], ts)
        assert (g["tret"][g["status"] == T.TSTOP_RETURN] == ts[g["status"] == T.TSTOP_RETURN]).all()
