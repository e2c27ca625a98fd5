"""The stepper's vector entry points with the masked error norms of idahip_set_suppress_alg, one system at a time: tests/stepper_ref.py
and tests/constr_ref.py with every LOCAL ERROR norm replaced by the oracle's own masked sum (oracle_norm_wrms_masked,
oracle/dense.hpp:100-107: p = (x_i w_i) m_i, m_i = 1.0 where id_i != 0 and 0.0 elsewhere, p p added left to right, / n, sqrt).

TEST INFRASTRUCTURE ONLY (tests/test_tstop_oracle.py pins it on the oracle; tests/test_gpu_suppress_alg.py compares the device
with it). Everything that is not a norm -- yy, yp, ee, phi, ewt, the constraint check's own norm, flag and rr -- is the unmasked
restatement's, unchanged."""
import ctypes as C

import numpy as np

import constr_ref as CR
import oracle_lib as O
import stepper_ref as R


def wrms_masked(x, w, id):
    x, w = O.f64(x), O.f64(w)
    m = np.ascontiguousarray(np.asarray(id) != 0, dtype=np.uint8)
    assert x.size == w.size == m.size
    return O.lib().oracle_norm_wrms_masked(O._ptr(x), O._ptr(w), m.ctypes.data_as(C.POINTER(C.c_uint8)), x.size)


def init_first(phi, rtol, atol, id):
    ewt = R.ewt_set(phi[0], rtol, atol)
    return ewt, wrms_masked(phi[1], ewt, id), wrms_masked(phi[0], ewt, id)


def error_norms(ee, ewt, phi, kk, id):
    """The four sums of post_newton (src/lib.rs:983-1004, src/impl_complete_step.rs:74-77), masked."""
    norms = np.zeros(4)
    with np.errstate(all="ignore"):
        norms[0] = wrms_masked(ee, ewt, id)
        if kk > 1:
            d = phi[kk] + ee
            norms[1] = wrms_masked(d, ewt, id)
            if kk > 2:
                d = d + phi[kk - 1]
                norms[2] = wrms_masked(d, ewt, id)
        if kk + 1 < R.MXORDP1:
            norms[3] = wrms_masked(ee - phi[kk + 1], ewt, id)
    return norms


def post_newton(yypredict, yppredict, ee, ewt, phi, cj, kk, id):
    yy, yp, _ = R.post_newton(yypredict, yppredict, ee, ewt, phi, cj, kk)
    return yy, yp, error_norms(ee, ewt, phi, kk, id)


def post_newton_constr(yypredict, yppredict, ee, ewt, phi, cj, kk, c, eps_newt, check, id):
    """constr_ref.post_newton_constr with its four sums masked; the norm of the correction that decides the flag is not."""
    yy, yp, ee2, norms, flag, rr = CR.post_newton_constr(yypredict, yppredict, ee, ewt, phi, cj, kk, c, eps_newt, check)
    if flag != 2:
        norms = error_norms(ee2, ewt, phi, kk, id)
    return yy, yp, ee2, norms, flag, rr


def complete_step(phi, ee, kused, ck, maxord, rtol, atol, id):
    phi2, ee2, ewt, _, bad = R.complete_step(phi, ee, kused, ck, maxord, rtol, atol)
    return phi2, ee2, ewt, wrms_masked(phi2[0], ewt, id), bad
