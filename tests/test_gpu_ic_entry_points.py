"""The device side of idaens_calc_ic, entry point by entry point (idahip_ic_begin, _reset, _res, _setup, _setup_dq, _solve, _trial,
_accept, _commit; include/ida_hip.h), on state the test uploads, against the step functions of calcic_ref.py
that calcic_ref.calc_ic itself is made of (ic_entry.Harness keeps the host mirror and makes every comparison).

What the whole calc_ic runs of test_gpu_calc_ic.py cannot show and these calls can:
  * every call over a list takes tn, cj, lambda and hh that differ from position to position, on the whole batch and on a permuted
    strict subset of it, and every system off the list must keep every watched field bit for bit;
  * the setup finds a rejected trial point in yy, yp and a stale direction in delta, and must put the iterate and savres there;
  * accept with IDAHIP_IC_Y follows a trial that moved y', which must not reach the iterate;
  * the weights' edge: +0.0 and negative weights are bad, NaN is not;
  * sizes on both sides of the 64-row blocks of the solve, of the 256-thread stride, the benchmark's n = 512, n > 1024 (the large-n
    LU pipelines, and at n = 2112 the zero-matrix shortcut of the stencil Jacobian and the factors' zero map), band widths other
    than (1, 1) at launch widths that leave the last workgroup partly empty, and one-thread systems across the 64-lane boundary.

Comparisons: a dense ctx bit for bit, a band ctx by value, norms and flags identical; factors against the oracle's getrf by value (as
everywhere in the suite; the solves then use the factors downloaded from the ctx). No tolerance appears in this file."""
import numpy as np
import pytest

import calcic_cases as K
import calcic_ref as IC
import ic_entry as E

pytestmark = pytest.mark.gpu


# ------------------------------------------------------------------------------------------------ the problems
def uniform_point(B, n, lo=-1.0, hi=1.0):
    return lambda rng: (rng.uniform(lo, hi, (B, n)), rng.uniform(-1.0, 1.0, (B, n)))


def linear_case(n, B, singular=None, dq=False):
    c = K.linear(n, "mixed", dq=dq, B=B)
    if singular is not None:  # a zero row in A and in B: a singular Jacobian at every cj
        sys, row = singular
        c["data"]["A"][sys, :, row] = 0.0
        c["data"]["B"][sys, :, row] = 0.0
    return dict(c, point=uniform_point(B, n))


def stencil_case(kind, n, B, band=None, dq=False):
    from idahip import problems
    if kind == "heat1d":
        p = problems.heat1d(n=n, batch=B)
        point = uniform_point(B, n)
    else:
        p = problems.bruss1d(m=n // 2, batch=B)
        point = lambda rng: (rng.uniform(0.5, 3.0, (B, n)), rng.uniform(-1.0, 1.0, (B, n)))
    ends = 1 if kind == "heat1d" else 2
    id_ = np.ones(n)
    id_[:ends] = id_[-ends:] = 0.0
    return {"kind": kind, "n": n, "band": band, "dq": dq, "id": id_, "rtol": p["rtol"], "atol": p["atol"], "yy0": p["yy0"],
            "data": {"params": p["params"]}, "point": point}


def tiny_case(kind, B):
    from idahip import problems
    if kind == "roberts":
        scale = np.array([1.0, 1.0e-4, 1.0])
        return {"kind": kind, "n": 3, "band": None, "dq": False, "id": np.array([1.0, 1.0, 0.0]), "rtol": 1.0e-4,
                "atol": np.array([1.0e-8, 1.0e-14, 1.0e-6]), "yy0": np.zeros((B, 3)), "data": {},
                "point": lambda rng: (rng.uniform(0.05, 1.0, (B, 3)) * scale, 0.1 * rng.uniform(-1.0, 1.0, (B, 3)))}
    p = problems.lorenz63(batch=B)
    return {"kind": kind, "n": 3, "band": None, "dq": False, "id": np.array([1.0, 0.0, 1.0]), "rtol": p["rtol"], "atol": p["atol"],
            "yy0": p["yy0"], "data": {"params": p["params"]}, "point": uniform_point(B, 3, -10.0, 10.0)}


def network_case(name, n, B):
    from idahip import problems
    p = problems.reaction_chain(n, B, seed=n) if name == "reaction_chain" else problems.enzyme_chain(n, B)
    data = {k: p[k] for k in ("reactions", "d", "params", "nconst") if k in p}
    spread = np.abs(p["yp0"]) + 1.0
    return {"kind": "mass_action", "n": n, "band": None, "dq": False, "id": p["d"].copy(), "rtol": p["rtol"], "atol": p["atol"],
            "yy0": p["yy0"], "data": data,
            "point": lambda rng: (p["yy0"] * rng.uniform(0.8, 1.2, (B, n)), p["yp0"] + 0.1 * spread * rng.uniform(-1.0, 1.0, (B, n)))}


def run_chain(h, rng, idx, singular=None):
    """One pass over the nine entry points on the list idx, in an order in which every call finds state that shows what it does.
    A singular system is set up (and reports its column) but neither solved nor tried."""
    m = idx.size
    rest = idx if singular is None else idx[idx != singular]
    h.fresh(rng)
    h.begin(idx)
    h.res(E.per_position(rng, m), idx)
    # what a rejected trial leaves behind: another point in yy, yp and a direction in delta
    y, yp = h.c["point"](rng)
    h.put("yy", y)
    h.put("yp", yp)
    h.put("delta", np.abs(y).mean() * rng.standard_normal(y.shape))
    info = h.setup(E.per_position(rng, m), idx)
    for q, s in enumerate(idx):  # hInfo goes by list position
        assert (info[q] != 0) == (s == singular), ("hInfo", q, s, info)
    h.solve(rest)
    h.trial(IC.Y_INIT, E.per_position(rng, rest.size), rest)
    h.trial(IC.YA_YDP_INIT, E.per_position(rng, rest.size), rest)  # ... moves y' in the differential components,
    h.accept(IC.Y_INIT, rest)                                      # which this accept must leave out of the iterate
    h.trial(IC.YA_YDP_INIT, E.per_position(rng, rest.size), rest)
    h.accept(IC.YA_YDP_INIT, rest)
    h.reset(idx)                                                   # (the iterate had moved away from the guess)
    y, yp = h.c["point"](rng)
    h.put("y0", y)
    h.put("yp0", yp)
    h.commit(idx)


def run_case(c, seed, singular=None, restate_jac=True, list_seed=None):
    h = E.Harness(c, restate_jac=restate_jac)
    rng = np.random.default_rng(seed)
    try:
        for idx in E.lists(h.B, seed if list_seed is None else list_seed):
            run_chain(h, rng, idx, singular)
    finally:
        h.close()


# ------------------------------------------------------------------------------------------------ linear dense, dense ctx
@pytest.mark.parametrize("n", [9, 10, 63, 64, 65, 255, 256, 257, 512, 513, 1030])
def test_linear_dense(n):
    """Both VEC instantiations of linear_sys_kernel<.., SysArgsIC> and ic_solve_kernel, the 64-row blocks of wg_getrs, the 256-thread
    stride, the benchmark's n, and n = 1030 on the large-n LU pipeline (there the factors are compared with idahip_nls_lsetup on a
    fresh ctx). One system has a zero row in A and B: it reports its column and leaves the other systems' factors alone."""
    B = 5 if n < 512 else 3
    run_case(linear_case(n, B, singular=(1, n // 2)), 7000 + n, singular=1, restate_jac=n <= 513)


def test_linear_dense_dq():
    run_case(linear_case(9, 5, dq=True), 7100)


# ------------------------------------------------------------------------------------------------ stencil kinds
@pytest.mark.parametrize("n", [9, 65, 257])
def test_heat_dense(n):
    run_case(stencil_case("heat1d", n, 5), 7200 + n)


def test_bruss_dense():
    run_case(stencil_case("bruss1d", 32, 5), 7300)


@pytest.mark.parametrize("superpanel", [0, 1])
def test_heat_2112_setups_in_a_row(superpanel):
    """n = 2112, every super-panel 64 wide: with set_lu_superpanel(1) a factorisation leaves the work matrix all zero and the next
    stencil Jacobian takes the shortcut (jwzero), and the factors carry a zero map. idahip_ic_setup, idahip_ic_setup at another cj,
    then idahip_nls_lsetup on one ctx: after each the factors are a fresh ctx's idahip_nls_lsetup at that point and cj, bit for
    bit, and idahip_ic_solve / idahip_ic_trial agree with the oracle's getrs on the factors downloaded."""
    n, B = 2112, 2
    c = stencil_case("heat1d", n, B)
    h = E.Harness(c, restate_jac=False)
    h.ctx.set_lu_superpanel(superpanel)
    rng = np.random.default_rng(7400 + superpanel)
    try:
        for idx in (np.arange(B, dtype=np.int32), np.array([1], dtype=np.int32)):
            m = idx.size
            h.fresh(rng)
            h.begin(idx)
            h.res(E.per_position(rng, m), idx)
            for rep in range(2):
                assert (h.setup(E.per_position(rng, m), idx) == 0).all()
                h.solve(idx)
                h.trial(IC.YA_YDP_INIT, E.per_position(rng, m), idx)
            a = E.per_position(rng, m)
            h.lsetup(a, idx)
            h.put("delta", rng.standard_normal((B, n)))
            h.solve(idx)
            h.trial(IC.Y_INIT, E.per_position(rng, m), idx)
    finally:
        h.close()


BAND_CASES = [("heat1d", n, w) for n in (9, 65, 130) for w in ((1, 1), (2, 2), (2, 3))] + \
             [("bruss1d", n, w) for n in (10, 66, 130) for w in ((2, 2), (2, 3))]


@pytest.mark.parametrize("spw", [4, 64])
@pytest.mark.parametrize("kind,n,width", BAND_CASES, ids=["%s-%d-%d_%d" % (k, n, w[0], w[1]) for k, n, w in BAND_CASES])
def test_band_ctx(kind, n, width, spw, monkeypatch):
    """ic_band_solve_kernel<1, 1> and <-1, -1> (generic widths) with IDAHIP_BAND_SPW (read at every call) packing 4 and 64 systems
    into a workgroup: 67 listed systems of 70 leave the last workgroup partly empty. (The Brusselator's n is even: 10 and 66 stand
    for 9 and 65.) Residual and solve are two launches on a band ctx."""
    monkeypatch.setenv("IDAHIP_BAND_SPW", str(spw))
    B, m = 70, 67
    h = E.Harness(stencil_case(kind, n, B, band=width))
    rng = np.random.default_rng(7500 + n + 10 * width[1] + spw)
    try:
        run_chain(h, rng, rng.permutation(B)[:m].astype(np.int32))
    finally:
        h.close()


@pytest.mark.parametrize("spw", [4, 64])
def test_band_ctx_of_width_0_0(spw, monkeypatch):
    """A diagonal Jacobian (ml = mu = 0), which only a host-callback band ctx takes: F_i = g_s id_i y_i' + a_i y_i + 0.1 y_i^3 - t,
    so the residual shows the tn of its list position. 67 listed systems of 70, as above."""
    import idahip
    monkeypatch.setenv("IDAHIP_BAND_SPW", str(spw))
    n, B, m = 9, 70, 67
    id_ = np.where(np.arange(n) % 3 == 1, 0.0, 1.0)
    a = 2.0 + np.sin(np.arange(n))
    res = lambda s, t, y, yp: (1.0 + s / 8.0) * id_ * yp + a * y + 0.1 * (y * y * y) - t
    diag = lambda s, cj, y: cj * ((1.0 + s / 8.0) * id_) + a + 0.3 * (y * y)
    c = {"kind": "host_callback", "n": n, "band": (0, 0), "dq": False, "id": id_, "rtol": 1.0e-6, "atol": np.array([1.0e-8]),
         "yy0": np.zeros((B, n)), "point": uniform_point(B, n, -2.0, 2.0),
         "data": {"res": res, "jac": lambda s, t, cj, y, yp, r: np.diag(diag(s, cj, y)),
                  "bjac": lambda s, t, cj, y, yp, r, ab: diag(s, cj, y).reshape(n, idahip.band_ldab(0, 0))}}
    h = E.Harness(c)
    rng = np.random.default_rng(7550 + spw)
    try:
        run_chain(h, rng, rng.permutation(B)[:m].astype(np.int32))
    finally:
        h.close()


def test_heat_band_dq():
    run_case(stencil_case("heat1d", 16, 5, band=(1, 1), dq=True), 7600)


# ------------------------------------------------------------------------------------------------ one thread per system
@pytest.mark.parametrize("kind", ["roberts", "lorenz63"])
def test_one_thread_fused_trial(kind):
    """ic_tiny_sys_kernel with the solve in the same thread: 130 systems, the whole batch (three wavefronts, the last with two
    lanes) and 86 of them in a permuted order."""
    run_case(tiny_case(kind, 130), 7700)


# ------------------------------------------------------------------------------------------------ mass action
@pytest.mark.parametrize("name,n", [("reaction_chain", 12), ("reaction_chain", 65), ("enzyme_chain", 9)])
def test_mass_action(name, n):
    """reaction_chain(12): the wave-per-system layout, residual and solve in two launches; (65): a workgroup per system and the fused
    trial (ma_sys_kernel with a.lu set); enzyme_chain(9): a network with rate laws (idahip_set_rate_network)."""
    run_case(network_case(name, n, 5), 7800 + n)


# ------------------------------------------------------------------------------------------------ host callbacks
def test_host_callback_split_path():
    """The two-unknown DAE of the line-search case (system 4's Jacobian is singular): the residual crosses to the host between the
    point kernel and the solve. The callback is called once per listed system, in list order, with that position's tn."""
    c = K.linesearch()
    B = c["yy0"].shape[0]
    seen = []

    def res(sys, t, y, yp):
        seen.append((int(sys), float(t)))
        return K.ls_res(sys, t, y, yp)

    c = dict(c, data={"res": res, "jac": K.ls_jac}, point=uniform_point(B, 2, -2.0, 2.0))
    h = E.Harness(c)
    rng = np.random.default_rng(7900)
    try:
        for idx in E.lists(B, 3):  # (seed 3: the subset holds the singular system)
            run_chain(h, rng, idx, singular=4 if 4 in idx else None)
            a = E.per_position(rng, idx.size)
            for call in (lambda: h.res(a, idx), lambda: h.trial(IC.YA_YDP_INIT, a, idx)):
                del seen[:]
                call()
                mine = [(s, t) for s, t in seen]  # (the harness calls the same function for its own reference afterwards)
                assert mine[:idx.size] == [(int(s), float(t)) for s, t in zip(idx, a["tn"])], (mine, idx)
    finally:
        h.close()


# ------------------------------------------------------------------------------------------------ the weights' edge
@pytest.mark.parametrize("n", [9, 300])
def test_bad_weights_in_begin_and_commit(n):
    """ewtbad of ic_begin_kernel and ic_commit_kernel: 1 exactly for the systems with a weight <= 0 -- +0.0 from an infinite
    component, a negative one from a negative entry of a vector atol where rtol |y| stays below it -- and 0 for a NaN weight."""
    B = 5
    c = stencil_case("heat1d", n, B)
    h = E.Harness(c)
    rng = np.random.default_rng(8000 + n)
    j = n - 2  # (past the first 256-thread pass at n = 300)
    try:
        for idx in E.lists(B, 1):
            pos = {int(s): q for q, s in enumerate(idx)}
            for field, call in (("g0", h.begin), ("y0", h.commit)):
                h.ctx.set_tolerances(c["rtol"], c["atol"])
                h.atol = np.full(n, float(c["atol"][0]))
                h.fresh(rng)
                y = h.v[field].copy()
                y[0, j], y[1, j], y[2, 0], y[4, 1] = np.inf, np.nan, -np.inf, np.nan
                h.put(field, y)
                out = call(idx)
                bad = out[1] if field == "g0" else out
                assert [int(bad[pos[s]]) for s in sorted(pos)] == [int(s in (0, 2)) for s in sorted(pos)], (field, idx, bad)
                # a vector atol with one negative entry: the weight there is negative while rtol |y_j| < 1e-3
                atol = np.full(n, 1.0e-8)
                atol[j] = -1.0e-3
                h.ctx.set_tolerances(c["rtol"], atol)
                h.atol = atol
                h.fresh(rng)
                y = h.v[field].copy()
                y[:, j] = np.array([1.0, 1.0e6, -1.0e6, -1.0, np.nan])  # rtol = 1e-5: weights -, +, +, -, NaN
                h.put(field, y)
                out = call(idx)
                bad = out[1] if field == "g0" else out
                assert [int(bad[pos[s]]) for s in sorted(pos)] == [int(s in (0, 3)) for s in sorted(pos)], (field, idx, bad)
    finally:
        h.close()
