"""The CPU oracle with a stop time and masked error norms switched on: tests/native/tstop_oracle.cpp (oracle/capi.cpp plus three
setters), compiled into a temporary directory with the oracle Makefile's flags and driven through ctypes.

TEST INFRASTRUCTURE ONLY. `Harness` is one `Ida` object that follows the library's calling rules where they differ from the oracle's:
  * a negative status is sticky (the library leaves such a system alone), except IDAENS_TOO_MUCH_WORK and an IDAENS_ILL_INPUT of a
    system that has not started (tret = t0 then);
  * IDAENS_BAD_T (a tout behind the last step) sets no tret: the reference returns an Err there. The library's tret stays what the
    previous return left, and so does the harness';
  * quirk Q15: after a TSTOP return of an IDA_ONE_STEP call the oracle, like the reference, keeps the stop time; the library clears
    it as C IDA does, and so does this helper, by hand.
A run is a list of ops, the same list for the product (tests/test_gpu_stop_time.py) and for the harness:
  ("stop", values)          values: [batch] with NaN = none, or None = clear all
  ("stop_rel", frac, ids)   tstop_b = tn_b + frac * hh_b for the systems in ids, from the driver's OWN tn and hh
  ("solve", tout, itask)
"""
import atexit
import ctypes as C
import os
import shutil
import subprocess
import tempfile

import numpy as np

import oracle_lib as O

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EPS = np.finfo(np.float64).eps
SUCCESS, TSTOP_RETURN, ROOT_RETURN = 0, 1, 2
TOO_MUCH_WORK, ILL_INPUT, BAD_T, BAD_TSTOP = -1, -22, -26, -27
NORMAL, ONE_STEP = 0, 1
SCALARS = ("tn", "hh", "hused", "kused", "nst", "nre", "nni", "netf", "ncfn", "nsetups")
_LIB = None


def oracle_cxxflags():
    """CXXFLAGS of oracle/Makefile (the line `CXXFLAGS ?= ...`)."""
    for line in open(os.path.join(ROOT, "oracle", "Makefile")):
        if line.startswith("CXXFLAGS"):
            return line.split("=", 1)[1].split()
    raise RuntimeError("oracle/Makefile has no CXXFLAGS line")


def compile_lib(source, prefix):
    """tests/native/<source> as a shared library in a temporary directory, with the oracle's flags; the entry points it has from
    oracle/capi.cpp and tests/native/tstop_oracle.cpp declared."""
    d = tempfile.mkdtemp(prefix=prefix + "_")
    atexit.register(shutil.rmtree, d, True)
    so = os.path.join(d, "lib%s.so" % prefix)
    subprocess.check_call([os.environ.get("CXX", "g++")] + oracle_cxxflags() + ["-shared", "-o", so, os.path.join(ROOT, "tests", "native", source)])
    L = C.CDLL(so)
    dp = O.dp
    L.oracle_ida_create.argtypes = [C.c_int, C.c_int, dp, dp, dp, dp, dp, dp, C.c_double, dp, C.c_int]
    L.oracle_ida_create.restype = C.c_void_p
    L.oracle_ida_destroy.argtypes = [C.c_void_p]
    L.oracle_ida_destroy.restype = None
    L.oracle_ida_solve.argtypes = [C.c_void_p, C.c_double, dp, C.c_int]
    L.oracle_ida_get_scalar.argtypes = [C.c_void_p, C.c_char_p, dp]
    L.oracle_ida_set_scalar.argtypes = [C.c_void_p, C.c_char_p, C.c_double]
    L.oracle_ida_get_vec.argtypes = [C.c_void_p, C.c_char_p, dp, C.c_int]
    L.oracle_ida_record_steps.argtypes = [C.c_void_p, C.c_int]
    L.oracle_ida_record_steps.restype = None
    L.oracle_ida_num_recorded.argtypes = [C.c_void_p]
    L.oracle_ida_num_recorded.restype = C.c_long
    L.oracle_ida_get_recorded.argtypes = [C.c_void_p, dp]
    L.oracle_ida_get_recorded.restype = None
    L.oracle_norm_wrms_masked.argtypes = [dp, dp, C.POINTER(C.c_uint8), C.c_int]
    L.oracle_norm_wrms_masked.restype = C.c_double
    L.tstop_oracle_set_id.argtypes = [C.c_void_p, dp, C.c_int]
    L.tstop_oracle_set_tstop.argtypes = [C.c_void_p, C.c_int, C.c_double]
    L.tstop_oracle_set_tstop.restype = None
    L.tstop_oracle_has_tstop.argtypes = [C.c_void_p, dp]
    return L


def lib():
    global _LIB
    if _LIB is None:
        _LIB = compile_lib("tstop_oracle.cpp", "tstop_oracle")
    return _LIB


class Harness(O.OracleIda):
    """System s of a generated problem (idahip.problems) as one oracle `Ida` with the library's calling rules."""

    def __init__(self, prob, s, id=None, suppress=False, mxstep=None):
        kw = {k.lower() if k == "params" else k: prob[k][s] for k in ("params", "A", "B", "c") if k in prob}
        O.OracleIda.__init__(self, prob["kind"], prob["n"], prob["yy0"][s], prob["yp0"][s], prob["rtol"], prob["atol"], **kw)
        real, mine = self.L, self._lib()  # the object was created by oracle_lib's library: make it anew in this one
        real.oracle_ida_destroy(self.h)
        self.L = mine
        self.h = self._create(prob)
        self.t0 = self.get("tn")
        if id is not None:
            a = O.f64(id)
            assert mine.tstop_oracle_set_id(self.h, O._ptr(a), a.size) == 0
        if suppress:
            self.set("suppressalg", 1.0)
        if mxstep is not None:
            self.set("mxstep", mxstep)
        mine.oracle_ida_record_steps(self.h, 1)
        self.dead = None      # (status, tret) once a status is sticky
        self.prev_tret = self.t0  # what the previous return left
        self.calls = []       # census: one dict per solve call

    def _lib(self):
        return lib()

    def _create(self, prob):
        yy0_, yp0_, atol_, p_, A_, B_, c_ = self._keep
        ptr = O._ptr
        return self.L.oracle_ida_create(O.KIND[prob["kind"]], prob["n"], ptr(p_), ptr(A_), ptr(B_), ptr(c_), ptr(yy0_), ptr(yp0_),
                                        float(prob["rtol"]), ptr(atol_), atol_.size)

    def set_stop_time(self, t):
        if t is None or t != t:
            self.L.tstop_oracle_set_tstop(self.h, 0, 0.0)
        else:
            self.L.tstop_oracle_set_tstop(self.h, 1, float(t))

    def stop_time(self):
        t = C.c_double(0.0)
        return t.value if self.L.tstop_oracle_has_tstop(self.h, C.byref(t)) == 1 else float("nan")

    def solve(self, tout, itask=NORMAL):
        if self.dead is not None:
            return self.dead
        nst0, tstop0, tn0, hh0 = int(self.get("nst")), self.stop_time(), self.get("tn"), self.get("hh")
        st, tret = O.OracleIda.solve(self, tout, itask)
        nst1 = int(self.get("nst"))
        if st == BAD_T:
            tret = self.prev_tret
        if st == ILL_INPUT and nst1 == 0:
            tret = self.t0  # the system has not started
        elif st < 0 and st != TOO_MUCH_WORK:
            self.dead = (st, tret)
        self.prev_tret = tret
        if st == TSTOP_RETURN and itask == ONE_STEP and nst1 == nst0:
            self.set_stop_time(None)  # Q15
        self.calls.append({"tout": tout, "itask": itask, "status": st, "nst0": nst0, "nst1": nst1, "tstop0": tstop0, "tn0": tn0, "hh0": hh0,
                           "h0u": self.get("h0u")})
        return st, tret

    def state(self):
        d = {k: self.get(k) for k in SCALARS}
        if d["nst"] == 0 and self.calls and self.calls[-1]["status"] == ILL_INPUT:
            d["hh"] = 0.0  # not started: the library's record is untouched (the oracle has tried a step size on its own)
        d["yy"], d["yp"] = self.getv("yy"), self.getv("yp")
        d["tstop"] = self.stop_time()
        return d

    def census(self):
        """Which of the oracle's stop-time branches this object's calls took (read off its own records: the clipped step size
        (tstop - tn)(1 - 4 eps) is recognised by its bits)."""
        seen = set()
        steps = self.recorded_steps()  # tn, hused, kused, nni, nsetups per accepted step
        for c in self.calls:
            ts = c["tstop0"]
            if ts != ts:
                continue
            if c["tout"] == ts:
                seen.add("tstop_eq_tout")
            if c["nst0"] == 0:
                if c["status"] == ILL_INPUT and c["nst1"] == 0:
                    seen.add("first_ill_input")
                    continue
                if c["h0u"] == (ts - self.t0) * (1.0 - 4.0 * EPS):
                    seen.add("first_clip")
            for i in range(max(c["nst0"], 1), c["nst1"]):
                if steps[i, 1] == (ts - steps[i - 1, 0]) * (1.0 - 4.0 * EPS):
                    seen.add("clip_stop_test1" if i == c["nst0"] else "clip_stop_test2")
                    assert steps[i, 0] <= ts if steps[i, 1] > 0 else steps[i, 0] >= ts
            if c["status"] == TSTOP_RETURN:
                where = "stop_test1" if c["nst1"] == c["nst0"] else "stop_test2"
                seen.add("tstop_%s_%s" % (where, "normal" if c["itask"] == NORMAL else "one_step"))
        return seen


BRANCHES = {"first_clip", "first_ill_input", "clip_stop_test1", "clip_stop_test2", "tstop_stop_test2_normal", "tstop_stop_test1_normal",
            "tstop_stop_test1_one_step", "tstop_stop_test2_one_step", "tstop_eq_tout"}


def run_ops(prob, ops, ids=None, harness=None, **how):
    """The ops on one Harness (or the subclass `harness`) per system of ids (default: all). -> (records, harnesses): records[k] = per
    solve op a dict of arrays over the systems (status, tret, yy, yp, the SCALARS, tstop and whatever else the harness' state() has)."""
    ids = list(range(prob["yy0"].shape[0])) if ids is None else list(ids)
    hs = [(harness or Harness)(prob, s, **how) for s in ids]
    rec = []
    for op in ops:
        if op[0] == "stop":
            for q, h in enumerate(hs):
                h.set_stop_time(None if op[1] is None else np.broadcast_to(op[1], (prob["yy0"].shape[0],))[ids[q]])
        elif op[0] == "stop_rel":
            for q, h in enumerate(hs):
                if ids[q] in op[2]:
                    h.set_stop_time(h.get("tn") + op[1] * h.get("hh"))
        else:
            out = [h.solve(op[1], op[2]) for h in hs]
            sts = [h.state() for h in hs]
            r = {"status": np.array([o[0] for o in out], dtype=np.int32), "tret": np.array([o[1] for o in out])}
            for k in sts[0]:
                r[k] = np.array([s[k] for s in sts])
            rec.append(r)
    return rec, hs


def by_residue(batch, values):
    """Stop times by b % len(values) (None = none) -> [batch] with NaN."""
    return np.array([np.nan if values[b % len(values)] is None else values[b % len(values)] for b in range(batch)], dtype=np.float64)
