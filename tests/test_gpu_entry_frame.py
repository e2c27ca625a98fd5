"""The protocol that every entry point of libidahip.so over a host list of system ids (hIdx, nsys) shares, pinned through the raw
handle (idahip.Ctx.H): the list check, the null-argument check, the function's own refusals and which of them wins when a call is
wrong in two ways at once, the empty list, and what one valid call on the list [2, 0] adds to idahip_timing_get's launch and
system counts per kernel class.

EXPECTED is what the library returned before these entry points were rewritten over one shared frame (csrc/list_call.hpp): return
codes, idahip_last_error texts and timing deltas, taken from a run and kept as literals. observe() makes every call once, in
table order (some valid calls prepare the state of later ones); the tests compare function by function. No values are compared:
the files named in DESIGN.md check those against the oracle. NULL is passed only for pointers that the library tests before use.

Contexts, 4 systems of 9 unknowns each: linear dense; band heat (1, 1); Krylov heat, maxl = 5, without and with the band
preconditioner (1, 1); a dense heat ctx with difference-quotient Jacobians; a dense heat ctx with constraints and an id vector;
a host-callback ctx without callbacks (refusals only)."""
import ctypes as C

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

N, BATCH = 9, 4
LIST = [2, 0]
IC_YA_YDP, IC_Y = 1, 2
F_PHI0 = 8


# ---- argument kinds: (kind, ...) -> a ctypes value for a list of m systems; pointers are the ones the library null-checks
def hd(per=1, val=1.0):
    return ("hd", per, val)


def hi(per=1, val=1):
    return ("hi", per, val)


def dv(key):
    return ("dev", key)


def sc(v):
    return ("sc", v)


def spec(ctx, args=(), krylov=False, refuse=(), both=(), also=()):
    """ctx: where the list, null, empty and valid calls run. krylov: refused on a Krylov ctx. refuse / both: (label, ctx,
    {argument: replacement}, hook) -- a call on the list [2, 0] unless `list` is replaced too. also: further ctxs for a valid call
    (another launch path)."""
    return {"ctx": ctx, "args": list(args), "krylov": krylov, "refuse": list(refuse), "both": list(both), "also": list(also)}


TN_CJ = [("hTn", hd()), ("hCj", hd())]
KKNS = ("hKkNs", hi(2, [2, 1]))
DUP, NULL = {"list": [1, 1]}, None
NOT_KRYLOV_BOTH = [("dup_not_krylov", "dense", DUP, None)]

CALLS = {
    "idahip_ls_setup": spec("dense", [("dA", dv("A")), ("dPiv", dv("P")), ("hInfo", hi())],
                            refuse=[("band", "band", {}, None), ("krylov", "kry", {}, None)]),
    "idahip_ls_solve": spec("dense", [("dLU", dv("A")), ("dPiv", dv("P")), ("dX", dv("X")), ("dB", dv("B")), ("tol", sc(0.0))]),
    "idahip_ls_setup_band": spec("band", [("ml", sc(1)), ("mu", sc(1)), ("dAB", dv("AB")), ("dPiv", dv("P")), ("hInfo", hi())],
                                 refuse=[("bandwidth", "band", {"ml": sc(-1)}, None)]),
    "idahip_ls_solve_band": spec("band", [("ml", sc(1)), ("mu", sc(1)), ("dAB", dv("AB")), ("dPiv", dv("P")), ("dX", dv("X")), ("dB", dv("B")),
                                          ("tol", sc(0.0))], refuse=[("bandwidth", "band", {"mu": sc(9)}, None)]),
    "idahip_wrms": spec("dense", [("dX", dv("X")), ("dW", dv("W")), ("hOut", hd())]),
    "idahip_wrms_masked": spec("con", [("dX", dv("X")), ("dW", dv("W")), ("hOut", hd())], refuse=[("no_id", "dense", {}, None)]),
    "idahip_nls_sys": spec("dense", TN_CJ + [("reset_ee", sc(1))]),
    "idahip_nls_lsetup": spec("band", TN_CJ + [("hInfo", hi())], krylov=True, refuse=[("dq", "dq", {}, None)]),
    "idahip_nls_sys_setup": spec("dense", TN_CJ + [("reset_ee", sc(1)), ("hInfo", hi())], krylov=True, refuse=[("dq", "dq", {}, None)], also=["band"]),
    "idahip_nls_lsetup_dq": spec("dq", TN_CJ + [("hHh", hd(1, 0.01)), ("hInfo", hi())], krylov=True, refuse=[("not_dq", "dense", {}, None)]),
    "idahip_jac_dq": spec("dq", TN_CJ + [("hHh", hd(1, 0.01)), ("hJ", hd(N * N))]),
    "idahip_newton_iter": spec("band", [("hScale", hd()), ("hDelnrm", hd())], krylov=True, also=["dense"]),
    "idahip_newton_iter2": spec("dense", [("hScale", hd()), ("hTn", hd()), ("hCj", hd()), ("hToldel", hd(1, 1.0e-4)), ("hSs", hd(1, 20.0)),
                                          ("hEpsNewt", hd(1, 0.33)), ("hDelnrm", hd(2)), ("hConv", hi())], krylov=True,
                                refuse=[("host_callback", "cb", {}, None)]),
    "idahip_krylov_psetup": spec("kryp", TN_CJ + [("hHh", hd(1, 0.01)), ("hInfo", hi())],
                                 refuse=[("not_krylov", "dense", {}, None), ("no_prec", "kry", {}, None)],
                                 both=NOT_KRYLOV_BOTH + [("null_no_prec", "kry", {"hInfo": NULL}, None)]),
    "idahip_krylov_psolve": spec("kryp", [("hR", hd(N)), ("hZ", hd(N))],
                                 refuse=[("not_krylov", "dense", {}, None), ("no_prec", "kry", {}, None), ("not_ready", "kryp", {"list": [1]}, None)],
                                 both=NOT_KRYLOV_BOTH + [("null_no_prec", "kry", {"hZ": NULL}, None), ("null_not_ready", "kryp", {"list": [1], "hR": NULL}, None)]),
    "idahip_krylov_solve": spec("kry", TN_CJ + [("hTol", hd(1, 1.0e-3)), ("hB", hd(N)), ("hX", hd(N)), ("hNli", hi()), ("hFlag", hi()), ("hResNorm", hd())],
                                refuse=[("not_krylov", "dense", {}, None), ("not_ready", "kryp", {"list": [1]}, None)],
                                both=NOT_KRYLOV_BOTH + [("null_not_krylov", "dense", {"hX": NULL}, None), ("null_not_ready", "kryp", {"list": [1], "hTol": NULL}, None)], also=["kryp"]),
    "idahip_newton_iter_krylov": spec("kry", TN_CJ + [("hEpsNewt", hd(1, 0.33)), ("hDelnrm", hd()), ("hNli", hi()), ("hFlag", hi())],
                                      refuse=[("not_krylov", "band", {}, None), ("not_ready", "kryp", {"list": [3]}, None)],
                                      both=NOT_KRYLOV_BOTH + [("null_not_krylov", "dense", {"hFlag": NULL}, None)]),
    "idahip_init_first": spec("dense", [("hYpnorm", hd()), ("hPhi0Nrm", hd())], refuse=[("missing_id", "dense", {}, "suppress")],
                              both=[("null_missing_id", "dense", {"hYpnorm": NULL}, "suppress")]),
    "idahip_scale_phi1": spec("dense", [("hFac", hd(1, 0.5))]),
    "idahip_predict": spec("dense", [KKNS, ("hBeta", hd(6)), ("hGamma", hd(6))],
                           refuse=[("kk", "dense", {"hKkNs": hi(2, [6, 1])}, None), ("ns", "dense", {"hKkNs": hi(2, [2, -1])}, None)]),
    "idahip_post_newton": spec("dense", [("hCj", hd()), ("hKk", hi(1, 2)), ("hNorms", hd(4))],
                               refuse=[("missing_id", "dense", {}, "suppress"), ("kk", "dense", {"hKk": hi(1, 0)}, None)],
                               both=[("missing_id_kk", "dense", {"hKk": hi(1, 6)}, "suppress")]),
    "idahip_post_newton_constr": spec("con", [("hCj", hd()), ("hKk", hi(1, 2)), ("hEpsNewt", hd(1, 0.33)), ("hCheck", hi()), ("hNorms", hd(4)),
                                              ("hFlag", hi()), ("hRr", hd())],
                                      refuse=[("missing_id", "dense", {}, "suppress"), ("no_constraints", "dense", {}, None),
                                              ("kk", "con", {"hKk": hi(1, 6)}, None)],
                                      both=[("no_constraints_kk", "dense", {"hKk": hi(1, 0)}, None)]),
    "idahip_constr_check": spec("con", [("field", sc(F_PHI0)), ("hViolated", hi())],
                                refuse=[("no_constraints", "dense", {}, None), ("field", "con", {"field": sc(99)}, None)],
                                both=[("no_constraints_field", "dense", {"field": sc(99)}, None)]),
    "idahip_restore": spec("dense", [KKNS, ("hCvals", hd(6))], refuse=[("kk", "dense", {"hKkNs": hi(2, [0, 1])}, None)]),
    "idahip_complete_step": spec("dense", [("hKused", hi(1, 2)), ("hCk", hd()), ("maxord", sc(5)), ("hPhi0Nrm", hd()), ("hEwtBad", hi())],
                                 refuse=[("missing_id", "dense", {}, "suppress"), ("maxord", "dense", {"maxord": sc(6)}, None),
                                         ("kused", "dense", {"hKused": hi(1, 4), "maxord": sc(3)}, None)],
                                 both=[("missing_id_maxord", "dense", {"maxord": sc(0)}, "suppress")]),
    "idahip_get_solution": spec("dense", [("hKord", hi(1, 2)), ("hCvals", hd(6)), ("hDvals", hd(5))],
                                refuse=[("kord", "dense", {"hKord": hi(1, 6)}, None)]),
    "idahip_get_dky": spec("dense", [("hKfirst", hi(1, 0)), ("hKlast", hi(1, 1)), ("hCjk", hd(6)), ("hOut", hd(N))],
                           refuse=[("range", "dense", {"hKfirst": hi(1, 2)}, None), ("klast", "dense", {"hKlast": hi(1, 6)}, None)]),
    "idahip_restore_initial": spec("dense", [], refuse=[("no_snapshot", "band", {}, None)]),
    "idahip_ic_begin": spec("dense", [("hYpnorm", hd()), ("hEwtBad", hi())], krylov=True),
    "idahip_ic_reset": spec("dense", [], krylov=True),
    "idahip_ic_res": spec("dense", TN_CJ, krylov=True),
    "idahip_ic_setup": spec("band", TN_CJ + [("hInfo", hi())], krylov=True, refuse=[("dq", "dq", {}, None)]),
    "idahip_ic_setup_dq": spec("dq", TN_CJ + [("hHh", hd(1, 0.01)), ("hInfo", hi())], krylov=True, refuse=[("not_dq", "band", {}, None)]),
    "idahip_ic_solve": spec("band", [("hFnorm", hd())], krylov=True),
    "idahip_ic_trial": spec("dense", [("icopt", sc(IC_Y))] + TN_CJ + [("hLambda", hd()), ("hFnormp", hd())], krylov=True,
                            refuse=[("icopt", "dense", {"icopt": sc(7)}, None), ("ya_ydp_no_id", "dense", {"icopt": sc(IC_YA_YDP)}, None)],
                            both=[("null_icopt", "dense", {"icopt": sc(7), "hLambda": NULL}, None)], also=["band"]),
    "idahip_ic_accept": spec("dense", [("icopt", sc(IC_Y))], krylov=True, refuse=[("icopt", "dense", {"icopt": sc(0)}, None)]),
    "idahip_ic_commit": spec("dense", [("hEwtBad", hi())], krylov=True),
}


# ---- the contexts
class Env:
    def __init__(self, ctx):
        self.ctx = ctx
        self.dev = {}
        ctx.set_tolerances(1.0e-5, 1.0e-8)
        B = ctx.batch
        import idahip
        for f, v in ((idahip.F_YY, 1.0), (idahip.F_YP, 0.1), (idahip.F_YYPREDICT, 1.0), (idahip.F_YPPREDICT, 0.1), (idahip.F_EWT, 1.0),
                     (idahip.F_EE, 0.0), (idahip.F_DELTA, 0.1), (idahip.F_SAVRES, 0.1)):
            ctx.upload(f, np.full((B, N), v))
        for j in range(6):
            ctx.upload(idahip.F_PHI0 + j, np.full((B, N), 0.01 * (j + 1)))
        eye_band = np.zeros((B, N, 4))
        eye_band[:, :, 2] = 1.0  # the diagonal's row of the (1, 1) band storage
        for key, host in (("A", np.tile(np.eye(N), (B, 1, 1))), ("AB", eye_band), ("P", np.zeros((B, N), dtype=np.int64)),
                          ("X", np.ones((B, N))), ("B", np.ones((B, N))), ("W", np.ones((B, N)))):
            self.dev[key] = ctx.dev_array(host)

    def close(self):
        for d in self.dev.values():
            self.ctx.dev_free(d)
        self.ctx.close()


def make_envs():
    import idahip
    from idahip import problems
    lin = problems.linear_dense(n=N, batch=BATCH)
    heat = problems.heat1d(n=N, batch=BATCH)
    envs = {
        "dense": Env(problems.make_ctx(lin)),
        "band": Env(problems.make_ctx(heat, band=True)),
        "kry": Env(problems.make_ctx(heat, krylov=5)),
        "kryp": Env(problems.make_ctx(heat, krylov=5)),
        "dq": Env(problems.make_ctx(heat)),
        "con": Env(problems.make_ctx(heat)),
        "cb": Env(idahip.Ctx("host_callback", N, BATCH)),
    }
    envs["kryp"].ctx.set_krylov_band_prec(1, 1)
    envs["dq"].ctx.set_jacobian_dq(True)
    envs["con"].ctx.set_constraints(np.ones(N))
    envs["con"].ctx.set_id(np.array([0.0] + [1.0] * (N - 2) + [0.0]))
    envs["dense"].ctx.snapshot_initial()
    # pivots that the stand-alone solves may follow, for every system: one factorisation of the identities
    for key, fn, pre in (("dense", "idahip_ls_setup", []), ("band", "idahip_ls_setup_band", [1, 1])):
        e = envs[key]
        info = (C.c_int32 * BATCH)()
        idx = (C.c_int32 * BATCH)(*range(BATCH))
        rc = getattr(e.ctx.H, fn)(e.ctx.h, *pre, e.dev["A" if key == "dense" else "AB"], e.dev["P"], info, idx, BATCH)
        assert rc == 0, (fn, rc)
    return envs


def build(env, kind, m):
    """-> (ctypes value, keep-alive)"""
    if kind is None:
        return None, None
    if kind[0] == "sc":
        return (C.c_double(kind[1]) if isinstance(kind[1], float) else int(kind[1])), None
    if kind[0] == "dev":
        return env.dev[kind[1]], None
    per, val = kind[1], kind[2]
    dtype, ptr = (np.float64, C.POINTER(C.c_double)) if kind[0] == "hd" else (np.int32, C.POINTER(C.c_int32))
    a = np.ascontiguousarray(np.tile(np.atleast_1d(np.asarray(val, dtype=dtype)), per * max(m, 1) // np.size(val)))
    assert a.size == per * max(m, 1)
    return a.ctypes.data_as(ptr), a


def call(envs, name, ctxkey, lst, nsys=None, replace=None, hook=None):
    """One call -> [rc, message if rc < 0]; lst None: a NULL list."""
    env = envs[ctxkey]
    H, h = env.ctx.H, env.ctx.h
    replace = replace or {}
    m = len(lst) if lst is not None else 2
    vals, keep = [], []
    for argname, kind in CALLS[name]["args"]:
        v, k = build(env, replace.get(argname, kind), m)
        vals.append(v)
        keep.append(k)
    idx = None if lst is None else (C.c_int32 * max(m, 1))(*lst)
    if hook == "suppress":
        assert H.idahip_set_suppress_alg(h, 1) == 0
    rc = getattr(H, name)(h, *vals, idx, m if nsys is None else nsys)
    if hook == "suppress":
        assert H.idahip_set_suppress_alg(h, 0) == 0
    return [rc, H.idahip_last_error(h).decode() if rc < 0 else ""]


def counts(env):
    t = env.ctx.timing_get()
    return {k: (v["launches"], v["systems"]) for k, v in t.items()}


def timed(envs, name, ctxkey, lst, replace=None):
    """A call that is expected to run -> [rc, {class: [launches added, systems added]}] (classes that moved only)"""
    before = counts(envs[ctxkey])
    rc, msg = call(envs, name, ctxkey, lst, replace=replace)
    assert rc >= 0, (name, rc, msg)
    after = counts(envs[ctxkey])
    return [rc, {k: [after[k][0] - before[k][0], after[k][1] - before[k][1]] for k in after if after[k] != before[k]}]


def observe_one(envs, name):
    s = CALLS[name]
    ck = s["ctx"]
    out = {}
    # (a) the list check
    out["list"] = [call(envs, name, ck, LIST, nsys=BATCH + 1), call(envs, name, ck, LIST, nsys=-1), call(envs, name, ck, None),
                   call(envs, name, ck, [1, BATCH]), call(envs, name, ck, [1, 1])]
    # (b) every pointer the library tests for NULL
    out["null"] = {a: call(envs, name, ck, LIST, replace={a: NULL}) for a, kind in s["args"] if kind[0] != "sc"}
    # (c) the function's own refusals
    out["refuse"] = {}
    for label, ctxkey, rep, hook in s["refuse"]:
        rep = dict(rep)
        lst = rep.pop("list", LIST)
        out["refuse"][label] = call(envs, name, ctxkey, lst, replace=rep, hook=hook)
    if s["krylov"]:
        out["refuse"]["krylov_ctx"] = call(envs, name, "kry", LIST)
    # (d) wrong in two ways at once
    out["both"] = {}
    if s["args"] and any(kind[0] != "sc" for _, kind in s["args"]):
        first = [a for a, kind in s["args"] if kind[0] != "sc"][0]
        out["both"]["dup_null"] = call(envs, name, ck, [1, 1], replace={first: NULL})
    if s["krylov"]:
        out["both"]["krylov_dup"] = call(envs, name, "kry", [1, 1])
    for label, ctxkey, rep, hook in s["both"]:
        rep = dict(rep)
        lst = rep.pop("list", LIST)
        out["both"][label] = call(envs, name, ctxkey, lst, replace=rep, hook=hook)
    # (e) the empty list: 0, and nothing launched
    before = counts(envs[ck])
    out["empty"] = [call(envs, name, ck, [], nsys=0), call(envs, name, ck, None, nsys=0)]
    out["empty_launched"] = counts(envs[ck]) != before
    # (f) one valid call
    out["valid"] = {key: timed(envs, name, key, LIST) for key in [ck] + s["also"]}
    return out


def observe():
    envs = make_envs()
    try:
        return {name: observe_one(envs, name) for name in CALLS}
    finally:
        for e in envs.values():
            e.close()


# ---- what the library answered before the rewrite
NULL_ARGUMENT = [-2, "null argument"]
TWICE = [-2, "system id 1 listed twice (again at list position 1)"]
LISTED = [[-2, "nsys = 5 out of range (batch = 4)"], [-2, "nsys = -1 out of range (batch = 4)"], [-2, "null system list"],
          [-2, "system id 4 out of range at list position 1"], TWICE]


def exp(null, refuse, both, valid):
    """null: the pointers that are refused with NULL_ARGUMENT; refuse / both: [code, text]; valid: ctx -> [return code, {kernel class:
    [launches added, systems added]}]. The list check and the empty list answer the same for every function."""
    return {"list": LISTED, "null": {a: NULL_ARGUMENT for a in null}, "refuse": refuse, "both": both, "empty": [[0, ""], [0, ""]],
            "empty_launched": False, "valid": valid}


EXPECTED = {
    "idahip_ls_setup": exp(null=["dA", "dPiv", "hInfo"],
        refuse={"band": [-2, "idahip_ls_setup on a band ctx (no dense work matrices): idahip_ls_setup_band"],
                "krylov": [-2, "idahip_ls_setup on a Krylov ctx (idahip_create_krylov): it holds no dense work matrices"]},
        both={"dup_null": TWICE},
        valid={"dense": [0, {"lu": [1, 2], "lu_finalize": [1, 2], "lu_panel": [1, 2]}]}),
    "idahip_ls_solve": exp(null=["dB", "dLU", "dPiv", "dX"],
        refuse={},
        both={"dup_null": TWICE},
        valid={"dense": [0, {"solve": [1, 2]}]}),
    "idahip_ls_setup_band": exp(null=["dAB", "dPiv", "hInfo"],
        refuse={"bandwidth": [-2, "bandwidths ml = -1, mu = 1 outside [0, n)"]},
        both={"dup_null": TWICE},
        valid={"band": [0, {"lu": [1, 2]}]}),
    "idahip_ls_solve_band": exp(null=["dAB", "dB", "dPiv", "dX"],
        refuse={"bandwidth": [-2, "bandwidths ml = 1, mu = 9 outside [0, n)"]},
        both={"dup_null": TWICE},
        valid={"band": [0, {"solve": [1, 2]}]}),
    "idahip_wrms": exp(null=["dW", "dX", "hOut"],
        refuse={},
        both={"dup_null": TWICE},
        valid={"dense": [0, {"vector": [1, 2]}]}),
    "idahip_wrms_masked": exp(null=["dW", "dX", "hOut"],
        refuse={"no_id": [-2, "idahip_wrms_masked: no id vector is set (idahip_set_id)"]},
        both={"dup_null": TWICE},
        valid={"con": [0, {"vector": [1, 2]}]}),
    "idahip_nls_sys": exp(null=["hCj", "hTn"],
        refuse={},
        both={"dup_null": TWICE},
        valid={"dense": [0, {"sys": [1, 2]}]}),
    "idahip_nls_lsetup": exp(null=["hCj", "hInfo", "hTn"],
        refuse={"dq": [-2, "a DQ ctx forms its Jacobians with the step sizes: idahip_nls_lsetup_dq"],
                "krylov_ctx": [-2, "idahip_nls_lsetup on a Krylov ctx (idahip_create_krylov): it forms, factors and solves with no matrix"]},
        both={"dup_null": TWICE,
              "krylov_dup": [-2, "idahip_nls_lsetup on a Krylov ctx (idahip_create_krylov): it forms, factors and solves with no matrix"]},
        valid={"band": [0, {"jac": [1, 2], "lu": [1, 2]}]}),
    "idahip_nls_sys_setup": exp(null=["hCj", "hInfo", "hTn"],
        refuse={"dq": [-2, "a DQ ctx forms its Jacobians with the step sizes: idahip_nls_sys, then idahip_nls_lsetup_dq"],
                "krylov_ctx": [-2, "idahip_nls_sys_setup on a Krylov ctx (idahip_create_krylov): it forms, factors and solves with no matrix"]},
        both={"dup_null": TWICE,
              "krylov_dup": [-2, "idahip_nls_sys_setup on a Krylov ctx (idahip_create_krylov): it forms, factors and solves with no matrix"]},
        valid={"band": [0, {"jac": [1, 2], "lu": [1, 2], "sys": [1, 2]}], "dense": [0, {"lu": [1, 2], "lu_finalize": [1, 2], "lu_panel": [1, 2], "sys_jac": [1, 2]}]}),
    "idahip_nls_lsetup_dq": exp(null=["hCj", "hHh", "hInfo", "hTn"],
        refuse={"krylov_ctx": [-2, "idahip_nls_lsetup_dq on a Krylov ctx (idahip_create_krylov): it forms, factors and solves with no matrix"],
                "not_dq": [-2, "idahip_nls_lsetup_dq on a ctx with analytic Jacobians (idahip_set_jacobian_dq)"]},
        both={"dup_null": TWICE,
              "krylov_dup": [-2, "idahip_nls_lsetup_dq on a Krylov ctx (idahip_create_krylov): it forms, factors and solves with no matrix"]},
        valid={"dq": [0, {"jac": [1, 2], "lu": [1, 2], "lu_finalize": [1, 2], "lu_panel": [1, 2]}]}),
    "idahip_jac_dq": exp(null=["hCj", "hHh", "hJ", "hTn"],
        refuse={},
        both={"dup_null": TWICE},
        valid={"dq": [0, {"jac": [1, 2]}]}),
    "idahip_newton_iter": exp(null=["hDelnrm", "hScale"],
        refuse={"krylov_ctx": [-2, "idahip_newton_iter on a Krylov ctx (idahip_create_krylov): it forms, factors and solves with no matrix"]},
        both={"dup_null": TWICE,
              "krylov_dup": [-2, "idahip_newton_iter on a Krylov ctx (idahip_create_krylov): it forms, factors and solves with no matrix"]},
        valid={"band": [0, {"newton_iter": [1, 2]}], "dense": [0, {"newton_iter": [1, 2]}]}),
    "idahip_newton_iter2": exp(null=["hCj", "hConv", "hDelnrm", "hEpsNewt", "hScale", "hSs", "hTn", "hToldel"],
        refuse={"host_callback": [-2, "idahip_newton_iter2 needs a device residual (not for IDAHIP_HOST_CALLBACK)"],
                "krylov_ctx": [-2, "idahip_newton_iter2 on a Krylov ctx (idahip_create_krylov): it forms, factors and solves with no matrix"]},
        both={"dup_null": TWICE,
              "krylov_dup": [-2, "idahip_newton_iter2 on a Krylov ctx (idahip_create_krylov): it forms, factors and solves with no matrix"]},
        valid={"dense": [0, {"newton_iter": [2, 2], "sys": [1, 0]}]}),
    "idahip_krylov_psetup": exp(null=["hCj", "hHh", "hInfo", "hTn"],
        refuse={"no_prec": [-2, "idahip_krylov_psetup: the ctx has no band preconditioner (idahip_set_krylov_band_prec)"],
                "not_krylov": [-2, "idahip_krylov_psetup: not a Krylov ctx (idahip_create_krylov)"]},
        both={"dup_not_krylov": TWICE,
              "dup_null": TWICE,
              "null_no_prec": [-2, "idahip_krylov_psetup: the ctx has no band preconditioner (idahip_set_krylov_band_prec)"]},
        valid={"kryp": [0, {"jac": [1, 2], "lu": [1, 2]}]}),
    "idahip_krylov_psolve": exp(null=["hR", "hZ"],
        refuse={"no_prec": [-2, "idahip_krylov_psolve: the ctx has no band preconditioner (idahip_set_krylov_band_prec)"],
                "not_krylov": [-2, "idahip_krylov_psolve: not a Krylov ctx (idahip_create_krylov)"],
                "not_ready": [-2, "idahip_krylov_psolve: system 1 has no preconditioner yet (idahip_krylov_psetup or idahip_krylov_upload_prec first)"]},
        both={"dup_not_krylov": TWICE,
              "dup_null": TWICE,
              "null_no_prec": [-2, "idahip_krylov_psolve: the ctx has no band preconditioner (idahip_set_krylov_band_prec)"],
              "null_not_ready": NULL_ARGUMENT},
        valid={"kryp": [0, {"solve": [1, 2]}]}),
    "idahip_krylov_solve": exp(null=["hB", "hCj", "hFlag", "hNli", "hResNorm", "hTn", "hTol", "hX"],
        refuse={"not_krylov": [-2, "idahip_krylov_solve: not a Krylov ctx (idahip_create_krylov)"],
                "not_ready": [-2, "idahip_krylov_solve: system 1 has no preconditioner yet (idahip_krylov_psetup or idahip_krylov_upload_prec first)"]},
        both={"dup_not_krylov": TWICE,
              "dup_null": TWICE,
              "null_not_krylov": [-2, "idahip_krylov_solve: not a Krylov ctx (idahip_create_krylov)"],
              "null_not_ready": NULL_ARGUMENT},
        valid={"kry": [0, {"solve": [1, 2]}], "kryp": [0, {"solve": [1, 2]}]}),
    "idahip_newton_iter_krylov": exp(null=["hCj", "hDelnrm", "hEpsNewt", "hFlag", "hNli", "hTn"],
        refuse={"not_krylov": [-2, "idahip_newton_iter_krylov: not a Krylov ctx (idahip_create_krylov)"],
                "not_ready": [-2, "idahip_newton_iter_krylov: system 3 has no preconditioner yet (idahip_krylov_psetup or idahip_krylov_upload_prec first)"]},
        both={"dup_not_krylov": TWICE,
              "dup_null": TWICE,
              "null_not_krylov": [-2, "idahip_newton_iter_krylov: not a Krylov ctx (idahip_create_krylov)"]},
        valid={"kry": [0, {"newton_iter": [1, 2]}]}),
    "idahip_init_first": exp(null=["hPhi0Nrm", "hYpnorm"],
        refuse={"missing_id": [-2, "idahip_init_first: suppress_alg is on and no id vector is set (idahip_set_id)"]},
        both={"dup_null": TWICE, "null_missing_id": NULL_ARGUMENT},
        valid={"dense": [0, {"vector": [1, 2]}]}),
    "idahip_scale_phi1": exp(null=["hFac"],
        refuse={},
        both={"dup_null": TWICE},
        valid={"dense": [0, {"vector": [1, 2]}]}),
    "idahip_predict": exp(null=["hBeta", "hGamma", "hKkNs"],
        refuse={"kk": [-2, "bad kk/ns at list position 0"], "ns": [-2, "bad kk/ns at list position 0"]},
        both={"dup_null": TWICE},
        valid={"dense": [0, {"vector": [1, 2]}]}),
    "idahip_post_newton": exp(null=["hCj", "hKk", "hNorms"],
        refuse={"kk": [-2, "bad kk at list position 0"],
                "missing_id": [-2, "idahip_post_newton: suppress_alg is on and no id vector is set (idahip_set_id)"]},
        both={"dup_null": TWICE, "missing_id_kk": [-2, "idahip_post_newton: suppress_alg is on and no id vector is set (idahip_set_id)"]},
        valid={"dense": [0, {"vector": [1, 2]}]}),
    "idahip_post_newton_constr": exp(null=["hCheck", "hCj", "hEpsNewt", "hFlag", "hKk", "hNorms", "hRr"],
        refuse={"kk": [-2, "bad kk at list position 0"],
                "missing_id": [-2, "idahip_post_newton_constr: suppress_alg is on and no id vector is set (idahip_set_id)"],
                "no_constraints": [-2, "idahip_post_newton_constr on a ctx without constraints (idahip_set_constraints)"]},
        both={"dup_null": TWICE, "no_constraints_kk": [-2, "idahip_post_newton_constr on a ctx without constraints (idahip_set_constraints)"]},
        valid={"con": [0, {"vector": [1, 2]}]}),
    "idahip_constr_check": exp(null=["hViolated"],
        refuse={"field": [-2, "unknown field 99"],
                "no_constraints": [-2, "idahip_constr_check on a ctx without constraints (idahip_set_constraints)"]},
        both={"dup_null": TWICE, "no_constraints_field": [-2, "idahip_constr_check on a ctx without constraints (idahip_set_constraints)"]},
        valid={"con": [0, {"vector": [1, 2]}]}),
    "idahip_restore": exp(null=["hCvals", "hKkNs"],
        refuse={"kk": [-2, "bad kk/ns at list position 0"]},
        both={"dup_null": TWICE},
        valid={"dense": [0, {"vector": [1, 2]}]}),
    "idahip_complete_step": exp(null=["hCk", "hEwtBad", "hKused", "hPhi0Nrm"],
        refuse={"kused": [-2, "bad kused at list position 0"],
                "maxord": [-2, "bad maxord"],
                "missing_id": [-2, "idahip_complete_step: suppress_alg is on and no id vector is set (idahip_set_id)"]},
        both={"dup_null": TWICE, "missing_id_maxord": [-2, "idahip_complete_step: suppress_alg is on and no id vector is set (idahip_set_id)"]},
        valid={"dense": [0, {"vector": [1, 2]}]}),
    "idahip_get_solution": exp(null=["hCvals", "hDvals", "hKord"],
        refuse={"kord": [-2, "bad kord at list position 0"]},
        both={"dup_null": TWICE},
        valid={"dense": [0, {"vector": [1, 2]}]}),
    "idahip_get_dky": exp(null=["hCjk", "hKfirst", "hKlast", "hOut"],
        refuse={"klast": [-2, "bad derivative range at list position 0"], "range": [-2, "bad derivative range at list position 0"]},
        both={"dup_null": TWICE},
        valid={"dense": [0, {"vector": [1, 2]}]}),
    "idahip_restore_initial": exp(null=[],
        refuse={"no_snapshot": [-2, "idahip_restore_initial before idahip_snapshot_initial"]},
        both={},
        valid={"dense": [0, {"vector": [1, 2]}]}),
    "idahip_ic_begin": exp(null=["hEwtBad", "hYpnorm"],
        refuse={"krylov_ctx": [-2, "idahip_ic_begin on a Krylov ctx (idahip_create_krylov): it forms, factors and solves with no matrix"]},
        both={"dup_null": TWICE,
              "krylov_dup": [-2, "idahip_ic_begin on a Krylov ctx (idahip_create_krylov): it forms, factors and solves with no matrix"]},
        valid={"dense": [0, {"vector": [1, 2]}]}),
    "idahip_ic_reset": exp(null=[],
        refuse={"krylov_ctx": [-2, "idahip_ic_reset on a Krylov ctx (idahip_create_krylov): it forms, factors and solves with no matrix"]},
        both={"krylov_dup": [-2, "idahip_ic_reset on a Krylov ctx (idahip_create_krylov): it forms, factors and solves with no matrix"]},
        valid={"dense": [0, {"vector": [1, 2]}]}),
    "idahip_ic_res": exp(null=["hCj", "hTn"],
        refuse={"krylov_ctx": [-2, "idahip_ic_res on a Krylov ctx (idahip_create_krylov): it forms, factors and solves with no matrix"]},
        both={"dup_null": TWICE,
              "krylov_dup": [-2, "idahip_ic_res on a Krylov ctx (idahip_create_krylov): it forms, factors and solves with no matrix"]},
        valid={"dense": [0, {"sys": [1, 2]}]}),
    "idahip_ic_setup": exp(null=["hCj", "hInfo", "hTn"],
        refuse={"dq": [-2, "a DQ ctx forms its Jacobians with the step sizes: idahip_ic_setup_dq"],
                "krylov_ctx": [-2, "idahip_ic_setup on a Krylov ctx (idahip_create_krylov): it forms, factors and solves with no matrix"]},
        both={"dup_null": TWICE,
              "krylov_dup": [-2, "idahip_ic_setup on a Krylov ctx (idahip_create_krylov): it forms, factors and solves with no matrix"]},
        valid={"band": [0, {"jac": [1, 2], "lu": [1, 2], "vector": [1, 2]}]}),
    "idahip_ic_setup_dq": exp(null=["hCj", "hHh", "hInfo", "hTn"],
        refuse={"krylov_ctx": [-2, "idahip_ic_setup_dq on a Krylov ctx (idahip_create_krylov): it forms, factors and solves with no matrix"],
                "not_dq": [-2, "idahip_ic_setup_dq on a ctx with analytic Jacobians (idahip_set_jacobian_dq)"]},
        both={"dup_null": TWICE,
              "krylov_dup": [-2, "idahip_ic_setup_dq on a Krylov ctx (idahip_create_krylov): it forms, factors and solves with no matrix"]},
        valid={"dq": [0, {"jac": [1, 2], "lu": [1, 2], "lu_finalize": [1, 2], "lu_panel": [1, 2], "vector": [1, 2]}]}),
    "idahip_ic_solve": exp(null=["hFnorm"],
        refuse={"krylov_ctx": [-2, "idahip_ic_solve on a Krylov ctx (idahip_create_krylov): it forms, factors and solves with no matrix"]},
        both={"dup_null": TWICE,
              "krylov_dup": [-2, "idahip_ic_solve on a Krylov ctx (idahip_create_krylov): it forms, factors and solves with no matrix"]},
        valid={"band": [0, {"solve": [1, 2]}]}),
    "idahip_ic_trial": exp(null=["hCj", "hFnormp", "hLambda", "hTn"],
        refuse={"icopt": [-2, "unknown icopt 7"],
                "krylov_ctx": [-2, "idahip_ic_trial on a Krylov ctx (idahip_create_krylov): it forms, factors and solves with no matrix"],
                "ya_ydp_no_id": [-2, "IDAHIP_IC_YA_YDP needs the id vector (idahip_set_id)"]},
        both={"dup_null": TWICE,
              "krylov_dup": [-2, "idahip_ic_trial on a Krylov ctx (idahip_create_krylov): it forms, factors and solves with no matrix"],
              "null_icopt": NULL_ARGUMENT},
        valid={"band": [0, {"solve": [1, 2], "sys": [1, 2]}], "dense": [0, {"sys": [1, 2]}]}),
    "idahip_ic_accept": exp(null=[],
        refuse={"icopt": [-2, "unknown icopt 0"],
                "krylov_ctx": [-2, "idahip_ic_accept on a Krylov ctx (idahip_create_krylov): it forms, factors and solves with no matrix"]},
        both={"krylov_dup": [-2, "idahip_ic_accept on a Krylov ctx (idahip_create_krylov): it forms, factors and solves with no matrix"]},
        valid={"dense": [0, {"vector": [1, 2]}]}),
    "idahip_ic_commit": exp(null=["hEwtBad"],
        refuse={"krylov_ctx": [-2, "idahip_ic_commit on a Krylov ctx (idahip_create_krylov): it forms, factors and solves with no matrix"]},
        both={"dup_null": TWICE,
              "krylov_dup": [-2, "idahip_ic_commit on a Krylov ctx (idahip_create_krylov): it forms, factors and solves with no matrix"]},
        valid={"dense": [0, {"vector": [1, 2]}]}),
}


@pytest.fixture(scope="module")
def observed():
    return observe()


def test_table_covers_every_listed_entry_point():
    """every function of include/ida_hip.h that takes (hIdx, nsys) is in the table"""
    import os
    import re
    header = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "ida_hip.h")).read()
    names = set(re.findall(r"int\s+(idahip_\w+)\s*\([^;]*?const\s+int32_t\s*\*\s*hIdx\s*,\s*int\s+nsys\s*\)\s*;", header))
    assert names == set(CALLS), (sorted(names - set(CALLS)), sorted(set(CALLS) - names))
    assert set(EXPECTED) == set(CALLS)


@pytest.mark.parametrize("name", sorted(CALLS))
def test_entry_point_protocol(observed, name):
    got, want = observed[name], EXPECTED[name]
    for part in ("list", "null", "refuse", "both", "empty", "empty_launched", "valid"):
        assert got[part] == want[part], (name, part, got[part], want[part])
