"""IDAReInit on the CPU oracle: tests/native/reinit_oracle.cpp (roots_oracle.cpp plus a creator that passes t0 to oracle/ida.hpp's `Ida`
constructor, quirk Q13), compiled as tests/tstop_oracle.compile_lib compiles its library and driven through ctypes.

TEST INFRASTRUCTURE ONLY. `Harness` is roots_oracle's with reinit(t0, yy0, yp0): the oracle object is destroyed and created anew at t0
with the new values and the same root functions, and everything the library's idaens_reinit starts over starts over here --
  * the id vector, suppressalg and mxstep are the ensemble's and the ctx's, not the system's: they are set again on the new object;
  * no stop time remains (a restarted system is Ida::new, which has none);
  * a sticky status is gone; the harness' t0 (the tret of an ILL_INPUT before the first step) is the new t0;
  * the library's record is Sys() with tn = t0, so the tret a CLOSE_ROOTS return would repeat is 0.0 until the first return.

The event runs of tests/test_gpu_reinit.py and their census in tests/test_reinit_oracle.py share `drive_events`: the touts of a
roots_cases case as roots_cases.drive drives them, and after every solve op the systems that returned ROOT_RETURN (optionally only those
`only` admits) are reinitialised with the jump dy = -0.5 * y (JUMPS: 4 * y on Lorenz) at the components of the root functions that
fired, zero elsewhere, and y' as reported. how = "at_return": t0 = tret and the jump is added by the callee; how = "host": t0 = tret + 0.25 and the sum y + dy is
formed by the caller with numpy's addition (one IEEE addition per component either way). A system restarted beyond the tout of the
next call integrates backwards to it, and every later tout lies behind it: IDAENS_BAD_T, sticky, with the root functions not
evaluated at the refused tout by r_check3 (tests/roots_oracle.py models it, include/ida_ensemble.h states it). Both variants drive every tout.
"""
import ctypes as C

import numpy as np

import oracle_lib as O
import roots_cases as RC
import roots_oracle as RO
import tstop_oracle as T

MAX_RETURNS = 40  # per tout: a halved component may cross its threshold again on its way back
EXTRA_COUNTERS = ("nje", "n_attempts", "nls_nconvfails")
JUMP = -0.5
JUMPS = {"lorenz": 4.0}  # by case: where -0.5 leaves every early step smooth on the oracle (tests/test_reinit_oracle.py says how it was found)
T0_SHIFT = 0.25
# jumps per system and run; a root return beyond them is continued as roots_cases.drive continues it. Without a cap a run need not
# end: how = "host" moves a system 0.25 past its root and the next solve integrates back over it; Lorenz' x 5 meets its threshold again
MAX_JUMPS = {"at_return": 3, "host": 2}
_LIB = None


def lib():
    global _LIB
    if _LIB is None:
        L = T.compile_lib("reinit_oracle.cpp", "reinit_oracle")
        dp = O.dp
        L.roots_oracle_create.argtypes = [C.c_int, C.c_int, dp, dp, dp, dp, dp, dp, C.c_double, dp, C.c_int, C.c_int, O.i32p, dp]
        L.roots_oracle_create.restype = C.c_void_p
        L.reinit_oracle_create.argtypes = L.roots_oracle_create.argtypes + [C.c_double]
        L.reinit_oracle_create.restype = C.c_void_p
        _LIB = L
    return _LIB


class Harness(RO.Harness):
    """roots_oracle.Harness created through reinit_oracle_create (t0 = 0 until reinit says otherwise)."""

    def __init__(self, prob, s, roots=None, **how):
        self._prob, self._how, self._t0_create = prob, dict(how), 0.0
        RO.Harness.__init__(self, prob, s, roots=roots, **how)

    def _lib(self):
        return lib()

    def _create(self, prob):
        yy0_, yp0_, atol_, p_, A_, B_, c_ = self._keep
        ptr = O._ptr
        comps, thr = (None, None) if self.roots is None else self.roots
        h = self.L.reinit_oracle_create(O.KIND[prob["kind"]], prob["n"], ptr(p_), ptr(A_), ptr(B_), ptr(c_), ptr(yy0_), ptr(yp0_),
                                        float(prob["rtol"]), ptr(atol_), atol_.size, -1 if comps is None else comps.size,
                                        None if comps is None else ptr(comps, O.i32p), None if comps is None else ptr(thr),
                                        float(self._t0_create))
        assert h, "reinit_oracle_create refused the components"
        return h

    def reinit(self, t0, yy0, yp0):
        self.L.oracle_ida_destroy(self.h)
        self.h = None
        self._keep[0], self._keep[1] = O.f64(yy0).copy(), O.f64(yp0).copy()
        self._t0_create = float(t0)
        self.h = self._create(self._prob)
        self.t0 = self.get("tn")
        how = self._how
        if how.get("id") is not None:
            a = O.f64(how["id"])
            assert self.L.tstop_oracle_set_id(self.h, O._ptr(a), a.size) == 0
        if how.get("suppress"):
            self.set("suppressalg", 1.0)
        if how.get("mxstep") is not None:
            self.set("mxstep", how["mxstep"])
        self.L.oracle_ida_record_steps(self.h, 1)
        self.dead = None
        self.calls = []
        self.last_tret = self.prev_tret = 0.0
        self.refused_evals = 0  # nge starts over with the new object

    def state(self):
        d = RO.Harness.state(self)
        for k in EXTRA_COUNTERS:
            d[k] = self.get(k)
        return d


def jump_of(c, yy, iroots):
    """dy [n] for one system: JUMP * y at the component of every root function that fired, zero elsewhere."""
    dy = np.zeros_like(yy)
    f = JUMPS.get(c["name"].split("/")[0], JUMP)
    for i, comp in enumerate(c["roots"][0]):
        if iroots[i] != 0:
            dy[comp] = f * yy[comp]
    return dy


class HarnessEvents:
    """The harness side of drive_events / replay: one Harness per system of ids."""

    def __init__(self, c, ids=None):
        prob = c["prob"]
        self.c = c
        self.B = prob["yy0"].shape[0]
        self.ids = list(range(self.B)) if ids is None else list(ids)
        self.hs = [Harness(prob, s, **c["how"]) for s in self.ids]
        self.rec = []
        self.last = None

    def solve(self, tout):
        out = [h.solve(tout, T.NORMAL) for h in self.hs]
        sts = [h.state() for h in self.hs]
        r = {"status": np.array([o[0] for o in out], dtype=np.int32), "tret": np.array([o[1] for o in out])}
        for k in sts[0]:
            r[k] = np.array([s[k] for s in sts])
        self.rec.append(r)
        self.last = r
        return r["status"]

    def jump(self, who, how):
        for b in who:
            q = self.ids.index(b)
            r, h = self.last, self.hs[q]
            yy, yp = r["yy"][q], r["yp"][q]
            y_new = yy + jump_of(self.c, yy, r["iroots"][q])
            h.reinit(r["tret"][q] + (T0_SHIFT if how == "host" else 0.0), y_new, yp)


class ProductEvents(RC.ProductDriver):
    """The product side: roots_cases.ProductDriver plus the jump through reinit_at_return / reinit."""

    def __init__(self, c, ens):
        RC.ProductDriver.__init__(self, ens)
        self.c = c

    def solve(self, tout):
        st = RC.ProductDriver.solve(self, tout, T.NORMAL)
        for k in EXTRA_COUNTERS:
            self.rec[-1][k] = self.ens.counter(k)
        return st

    def jump(self, who, how):
        r = self.rec[-1]
        who = np.asarray(who, dtype=np.int32)
        dy = np.array([jump_of(self.c, r["yy"][b], r["iroots"][b]) for b in who])
        if how == "host":
            self.ens.reinit(who, r["tret"][who] + T0_SHIFT, r["yy"][who] + dy, r["yp"][who])
        else:
            self.ens.reinit_at_return(who, dy=dy, dyp=None)


def drive_events(c, d, how="at_return", only=None):
    """-> the ops made: ("solve", tout) and ("jump", [systems])."""
    ops = []
    jumps = {}
    cap = MAX_JUMPS[how]
    for t in c["touts"]:
        for _ in range(MAX_RETURNS):
            ops.append(("solve", float(t)))
            st = d.solve(float(t))
            who = [int(b) for b in np.nonzero(st == T.ROOT_RETURN)[0] if only is None or only(int(b))]
            who = [b for b in who if jumps.get(b, 0) < cap]
            for b in who:
                jumps[b] = jumps.get(b, 0) + 1
            if who:
                ops.append(("jump", who))
                d.jump(who, how)
            if ((st == T.SUCCESS) | (st < 0)).all():
                break
        else:
            raise AssertionError("%s: no end of returns at tout %g: %s" % (c["name"], t, st))
    return ops


def replay(c, ops, how="at_return", ids=None):
    """The ops on the harness -> its records, one per solve op."""
    d = HarnessEvents(c, ids=ids)
    for op in ops:
        if op[0] == "solve":
            d.solve(op[1])
        else:
            d.jump([b for b in op[1] if b in d.ids], how)
    return d.rec


def compare(got, want, by_value=False, what=""):
    """roots_cases.compare plus the oracle's remaining counters. No tolerances."""
    RC.compare(got, want, by_value=by_value, what=what)
    for i, (g, w) in enumerate(zip(got, want)):
        for k in EXTRA_COUNTERS:
            assert np.array_equal(g[k], w[k].astype(np.int64)), (what, i, k, g[k], w[k])
