"""The constrained integrations that tests/test_constr_ref.py takes the census of and tests/test_gpu_constraints.py runs on the device:
inputs only (idahip.problems generators, a constraint vector, a schedule), shared so that both files speak of the same runs.

A case is dict(prob, c [n], touts, mxstep). The constraint vector is shared by the batch, as the ABI's is."""
import functools

import numpy as np


def _roberts(batch):
    from idahip import problems
    p = problems.roberts()
    rng = np.random.Generator(np.random.PCG64(5))
    y0 = np.tile(p["yy0"], (batch, 1))
    if batch > 1:
        y0[1:, 0] -= 1e-3 * rng.uniform(0, 1, batch - 1)  # y1 + y2 + y3 = 1 kept
        y0[1:, 2] = 1.0 - y0[1:, 0] - y0[1:, 1]
    yp0 = np.stack([-0.04 * y0[:, 0] + 1e4 * y0[:, 1] * y0[:, 2], 0.04 * y0[:, 0] - 1e4 * y0[:, 1] * y0[:, 2] - 3e7 * y0[:, 1] ** 2,
                    np.zeros(batch)], axis=1)
    yp0[:, 2] = -(yp0[:, 0] + yp0[:, 1])
    p.update(yy0=y0, yp0=yp0)
    return p


def roberts_loose(batch=5):
    """Roberts at rtol 1e-2, atol (1e-6, 1e-4, 1e-4), every concentration >= 0, to t = 4e10: the solution leaves the feasible
    set inside the tolerance and is put back by corrections; every system finishes."""
    p = _roberts(batch)
    p.update(rtol=1.0e-2, atol=np.array([1.0e-6, 1.0e-4, 1.0e-4]))
    return {"prob": p, "c": np.array([1.0, 1.0, 1.0]), "touts": p["touts"], "mxstep": 500}


def roberts_inconsistent(batch=5):
    """Roberts from the inconsistent y0 = (1, 0.5, 0) (system 0; the others start next to it): the first step cannot be taken --
    convergence failures and constraint failures share the ten attempts."""
    p = _roberts(batch)
    p["yy0"][:, 1] = 0.5 + 1e-3 * np.arange(batch)
    return {"prob": p, "c": np.array([1.0, 1.0, 1.0]), "touts": p["touts"][:2], "mxstep": 500}


def lorenz_x_nonneg(batch=5, mxstep=500):
    """Lorenz63 with x >= 0: the attractor's x changes sign, so corrections and constraint failures alternate until mxstep."""
    from idahip import problems
    p = problems.lorenz63(batch=batch)
    return {"prob": p, "c": np.array([1.0, 0.0, 0.0]), "touts": np.array([1.0, 5.0]), "mxstep": mxstep}


def lorenz_start_violated(batch=5):
    """Lorenz63 with y <= 0 although y(0) is about 1: refused at the start."""
    from idahip import problems
    p = problems.lorenz63(batch=batch)
    return {"prob": p, "c": np.array([0.0, -1.0, 0.0]), "touts": p["touts"][:2], "mxstep": 500}


def heat_nonneg(batch=3):
    """heat1d n = 40, every temperature >= 0, to t = 0.1: the decaying profile is corrected near the ends."""
    from idahip import problems
    p = problems.heat1d(n=40, batch=batch)
    return {"prob": p, "c": np.ones(40), "touts": p["touts"], "mxstep": 500}


def heat_positive(batch=3):
    """heat1d n = 40, every temperature > 0: the end nodes are exactly 0, refused at the start."""
    from idahip import problems
    p = problems.heat1d(n=40, batch=batch)
    return {"prob": p, "c": 2.0 * np.ones(40), "touts": p["touts"][:2], "mxstep": 500}


def _shared_pattern(want, y_start):
    """System 0's pattern want[0], with 0 wherever a system of the batch would violate it at t0."""
    c = want[0].copy()
    for b in range(y_start.shape[0]):
        yc = y_start[b] * c
        c[((np.abs(c) > 1.5) & (yc <= 0.0)) | ((np.abs(c) > 0.5) & (yc < 0.0))] = 0.0
    return c


def linear_monotone(n=24, batch=5, mxstep=500):
    """linear_dense: every differential component is asked to keep the sign of its initial slope (y0 = 0 there), every algebraic one
    the sign of its initial value -- which the solution does not do for long."""
    from idahip import problems
    p = problems.linear_dense(n=n, batch=batch)
    nd = (3 * n) // 4
    want = np.sign(p["yp0"])
    want[:, nd:] = np.sign(p["yy0"][:, nd:])
    return {"prob": p, "c": _shared_pattern(want, p["yy0"]), "touts": p["touts"][:2], "mxstep": mxstep}


def linear_negated(n=24, batch=5):
    """linear_dense with the algebraic components of y0 given the signs opposite to system 0's consistent values and required to keep
    them: for system 0 (every algebraic component negated) the Newton solve of the first step puts them back where the algebraic
    equations want them and every attempt ends in a constraint failure; the other systems have some components negated."""
    from idahip import problems
    p = problems.linear_dense(n=n, batch=batch)
    nd = (3 * n) // 4
    target = -np.sign(p["yy0"][0, nd:])
    p["yy0"][:, nd:] = np.abs(p["yy0"][:, nd:]) * target
    c = np.zeros(n)
    c[nd:] = target
    return {"prob": p, "c": c, "touts": p["touts"][:2], "mxstep": 500}


# the case lists of the two steppers that check constraints (name -> constructor); the census must cover every branch on each
HOST_CASES = {
    "roberts_loose": roberts_loose, "roberts_inconsistent": roberts_inconsistent, "lorenz_x_nonneg": lorenz_x_nonneg,
    "lorenz_start_violated": lorenz_start_violated, "heat_nonneg": heat_nonneg, "heat_positive": heat_positive,
    "linear_monotone_24": functools.partial(linear_monotone, 24, 5), "linear_monotone_200": functools.partial(linear_monotone, 200, 4, 60),
    "linear_negated_24": functools.partial(linear_negated, 24, 5), "linear_negated_200": functools.partial(linear_negated, 200, 4),
}
TINY_CASES = {"roberts_loose": roberts_loose, "roberts_inconsistent": roberts_inconsistent, "lorenz_x_nonneg": lorenz_x_nonneg,
              "lorenz_start_violated": lorenz_start_violated}


@functools.lru_cache(maxsize=None)
def reference(name, batch=None, ids=None, itask=0, ncalls=None):
    """The reference run of a case (tests/constr_ref.py), computed once per process and shared: (case, ref). Not to be modified.
    batch: another batch size than the case's own; ids: only these systems of the batch (a tuple); itask / ncalls: IDA_ONE_STEP walks
    (ncalls calls with the case's first tout)."""
    import constr_ref as CR
    make = HOST_CASES.get(name) or TINY_CASES[name]
    case = make() if batch is None else make(batch)
    touts = case["touts"] if ncalls is None else [case["touts"][0]] * ncalls
    return case, CR.run(case["prob"], case["c"], touts, mxstep=case["mxstep"], itask=itask, ids=None if ids is None else list(ids))
