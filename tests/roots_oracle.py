"""The CPU oracle with the product's root function family on any of its problems: tests/native/roots_oracle.cpp (tstop_oracle.cpp plus a
`Problem` decorator that answers num_roots() / root() with g_i = y[comp_i] - thr_i), compiled into a temporary directory with the oracle
Makefile's flags and driven through ctypes, as tests/tstop_oracle.py does with its library.

TEST INFRASTRUCTURE ONLY. `Harness` is tstop_oracle's, with roots=(comps, thresholds) next to id / suppress / mxstep; ops and run_ops
are tstop_oracle's. Where the library's calling rules differ from the oracle's for roots:
  * the oracle numbers IdaError::CloseRoots -30, the library IDAENS_CLOSE_ROOTS = -10: the harness reports -10;
  * that return sets no tret (the reference returns an Err there): the library's tret stays what the previous return left, and so does
    the harness';
  * a tout behind the last step (IDAENS_BAD_T) with root functions: the reference's r_check3 ignores the refusal of its interpolation
    at thi = tout (impl_r_check.rs:236), evaluates g on the values the previous return left and counts that evaluation before
    stop_test1 returns the refusal; the library returns the refusal from r_check3 itself, before any evaluation
    (include/ida_ensemble.h, "A tout behind the last step"). The status is the same and sticky; the harness takes the evaluation
    that the library never made out of nge (`refused_evals`).
roots=None leaves the problem as the oracle has it (Roberts then has its own two functions); roots=([], []) is the problem with no
root function at all, Roberts included.
"""
import ctypes as C

import numpy as np

import oracle_lib as O
import tstop_oracle as T

ROOT_RETURN = T.ROOT_RETURN
ORACLE_CLOSE_ROOTS, CLOSE_ROOTS = -30, -10
BAD_T = T.BAD_T
_LIB = None


def lib():
    global _LIB
    if _LIB is None:
        L = T.compile_lib("roots_oracle.cpp", "roots_oracle")
        dp = O.dp
        L.roots_oracle_create.argtypes = [C.c_int, C.c_int, dp, dp, dp, dp, dp, dp, C.c_double, dp, C.c_int, C.c_int, O.i32p, dp]
        L.roots_oracle_create.restype = C.c_void_p
        _LIB = L
    return _LIB


class Harness(T.Harness):
    """System s of a generated problem with the root functions y[comps[i]] - thr[i]."""

    def __init__(self, prob, s, roots=None, **how):
        self.roots = None if roots is None else (np.ascontiguousarray(roots[0], dtype=np.int32), O.f64(roots[1]))
        assert self.roots is None or self.roots[0].size == self.roots[1].size
        self.refused_evals = 0
        T.Harness.__init__(self, prob, s, **how)
        self.last_tret = self.t0

    def _lib(self):
        return lib()

    def _create(self, prob):
        if self.roots is None:
            return T.Harness._create(self, prob)
        yy0_, yp0_, atol_, p_, A_, B_, c_ = self._keep
        ptr = O._ptr
        comps, thr = self.roots
        h = self.L.roots_oracle_create(O.KIND[prob["kind"]], prob["n"], ptr(p_), ptr(A_), ptr(B_), ptr(c_), ptr(yy0_), ptr(yp0_),
                                       float(prob["rtol"]), ptr(atol_), atol_.size, comps.size, ptr(comps, O.i32p), ptr(thr))
        assert h, "roots_oracle_create refused the components %s" % comps.tolist()
        return h

    def solve(self, tout, itask=T.NORMAL):
        if self.dead is not None:
            return self.dead
        refuses, nge0 = self._r_check3_refuses(tout, itask), self.get("nge")
        st, tret = T.Harness.solve(self, tout, itask)
        if st == BAD_T and refuses:
            # r_check2 before it: at most two evaluations; r_check3 on the stale values: ghi == glo, no sign change, one evaluation
            assert 1 <= self.get("nge") - nge0 <= 3, (nge0, self.get("nge"))
            self.refused_evals += 1
        if st == ORACLE_CLOSE_ROOTS:
            st, tret = CLOSE_ROOTS, self.last_tret
            self.dead = (st, tret)
            self.calls[-1]["status"] = st
        self.last_tret = tret
        return st, tret

    def _r_check3_refuses(self, tout, itask):
        """Whether this call enters r_check3 with thi = tout outside the last step (oracle/ida.hpp:343-345, 995-997, 735-737)."""
        if self.roots is not None and self.roots[0].size == 0:
            return False
        tn, hh, hused, nst = self.get("tn"), self.get("hh"), self.get("hused"), self.get("nst")
        if nst == 0 or itask != T.NORMAL:
            return False
        fuzz = (abs(tn) + abs(hh)) * T.EPS * 100.0
        tp = tn - hused - (fuzz if hh >= 0.0 else -fuzz)
        return abs(tn - self.get("tretlast")) > fuzz and (tout - tn) * hh < 0.0 and (tout - tp) * hh < 0.0

    def state(self):
        d = T.Harness.state(self)
        none = self.roots is not None and self.roots[0].size == 0  # (an empty vector has no address to read from)
        d["iroots"] = np.zeros(0, dtype=np.int32) if none else self.getv("iroots").astype(np.int32)
        d["nge"] = self.get("nge") - self.refused_evals
        return d


def run_ops(prob, ops, ids=None, **how):
    """tstop_oracle.run_ops on this module's Harness: the records also hold iroots [systems][nroots] and nge."""
    return T.run_ops(prob, ops, ids=ids, harness=Harness, **how)
