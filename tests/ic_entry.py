"""The nine idahip_ic_* entry points (include/ida_hip.h) called one by one on a ctx whose state the test owns:
a host mirror of every vector the calls read or write, updated for the listed systems with the step functions of calcic_ref.py --
the ones calcic_ref.calc_ic itself is made of -- and compared field by field after every call.

A problem is a case dict as calcic_cases.py builds them (kind, n, band, dq, id, rtol, atol, data, yy0 for the batch size), plus
"point": rng -> (y [B][n], y' [B][n]), random points at which the kind's residual and Jacobian are well behaved.

Comparisons: a dense ctx bit for bit (stepper_ref.same_bits: the sign of a zero counts, any NaN for a NaN), a band ctx by value
(np.array_equal), a system off the list bit for bit on either; norms and flags identical. No tolerance appears.

TEST INFRASTRUCTURE ONLY."""
import numpy as np

import calcic_cases as K
import calcic_ref as IC
import oracle_lib as O
import stepper_ref as SR

NAMES = ("g0", "g1", "y0", "yp0", "delnew", "delta", "savres", "yy", "yp", "ewt")


def field_ids():
    import idahip
    return {"g0": idahip.F_PHI0, "g1": idahip.F_PHI0 + 1, "y0": idahip.F_PHI0 + 2, "yp0": idahip.F_PHI0 + 3, "delnew": idahip.F_PHI0 + 4,
            "delta": idahip.F_DELTA, "savres": idahip.F_SAVRES, "yy": idahip.F_YY, "yp": idahip.F_YP, "ewt": idahip.F_EWT}


def lists(B, seed):
    """the whole batch in order, and a permuted strict subset of it"""
    return [np.arange(B, dtype=np.int32), np.random.default_rng(seed).permutation(B)[:max(2, (2 * B) // 3)].astype(np.int32)]


def per_position(rng, m):
    """tn, cj, lambda and hh of a call over m list positions, no two positions alike"""
    lam = np.array([1.0, 0.5, 0.25, 2.0 ** -7, 2.0 ** -3, 0.75])
    lam = np.concatenate([lam, 2.0 ** -rng.integers(1, 20, size=max(0, m - lam.size)).astype(np.float64)])[:m]
    return {"tn": rng.uniform(0.0, 1.0, m), "cj": 10.0 ** rng.uniform(1.0, 4.0, m), "lam": rng.permutation(lam),
            "hh": rng.choice([-1.0, 1.0], m) * 10.0 ** rng.uniform(-4.0, -1.0, m)}


class Harness:
    def __init__(self, c, restate_jac=True):
        self.c, self.n, self.B = c, c["n"], c["yy0"].shape[0]
        self.ctx = K.make_ctx(c)
        self.exact = c["band"] is None
        self.restate_jac = restate_jac  # False: the factors are compared with a fresh ctx's idahip_nls_lsetup (large n)
        self.probs = [K.ref_problem(c, b) for b in range(self.B)]
        self.ids = field_ids()
        atol = np.asarray(c["atol"], dtype=np.float64)
        self.atol = atol if atol.size == self.n else np.full(self.n, float(atol.ravel()[0]))
        self.v = {}
        self.fac = {}  # system -> its factors as downloaded since the last setup

    def close(self):
        self.ctx.close()

    # ---- state
    def fresh(self, rng):
        """independent random values in every watched field, on the host and on the device"""
        (g0, g1), (y0, yp0), (yy, yp) = (self.c["point"](rng) for _ in range(3))
        scale = np.abs(y0).mean()
        self.v = {"g0": g0, "g1": g1, "y0": y0, "yp0": yp0, "yy": yy, "yp": yp, "ewt": rng.uniform(0.5, 2.0, (self.B, self.n)) / scale}
        for f in ("delnew", "delta", "savres"):
            self.v[f] = scale * rng.standard_normal((self.B, self.n))
        for f in NAMES:
            self.put(f, self.v[f])

    def put(self, f, arr):
        self.v[f] = np.array(arr, dtype=np.float64)
        self.ctx.upload(self.ids[f], self.v[f])

    def same(self, got, want):
        return SR.same_bits(got, want) if self.exact else bool(np.array_equal(got, want))

    def check(self, what, idx):
        """every watched field of every system: the listed ones as the mirror says, the others bit for bit as they were"""
        listed = np.zeros(self.B, dtype=bool)
        listed[idx] = True
        for f in NAMES:
            got = self.ctx.download(self.ids[f])
            for s in range(self.B):
                ok = self.same(got[s], self.v[f][s]) if listed[s] else SR.same_bits(got[s], self.v[f][s])
                assert ok, (what, f, s, "listed" if listed[s] else "off the list", float(np.nanmax(np.abs(got[s] - self.v[f][s]))))

    def same_norm(self, got, want, what):
        assert SR.same_bits(np.float64(got), np.float64(want)), (what, got, want)

    def factors(self, s, ctx=None):
        """(dense factors, logical [n][n]; pivots) of one system"""
        import idahip
        if ctx is None:
            if int(s) not in self.fac:
                self.fac[int(s)] = self.factors(s, self.ctx)
            return self.fac[int(s)]
        if self.c["band"] is None:
            return ctx.download_lu(int(s))
        ab, piv = ctx.download_lu_band(int(s))
        return idahip.band_expand_factors(ab, piv, self.n, *self.c["band"]), piv

    # ---- the calls
    def _p(self, a, t=None):
        import idahip
        return idahip._p(a, t or idahip.dp)

    def _i(self, idx):
        import idahip
        return idahip._p(idx, idahip.i32p), int(idx.size)

    def begin(self, idx):
        nrm, bad = np.full(idx.size, -1.0), np.full(idx.size, -1, dtype=np.int32)
        self.ctx._chk(self.ctx.H.idahip_ic_begin(self.ctx.h, self._p(nrm), self._i(bad)[0], *self._i(idx)), "ic_begin")
        for q, s in enumerate(idx):
            ewt, wbad, ypnorm = IC.begin(self.v["g0"][s], self.v["g1"][s], self.c["rtol"], self.atol)
            self.v["ewt"][s], self.v["y0"][s], self.v["yp0"][s] = ewt, self.v["g0"][s], self.v["g1"][s]
            self.same_norm(nrm[q], ypnorm, ("ic_begin ypnorm", q, s))
            assert bad[q] == int(wbad), ("ic_begin ewtbad", q, s, bad[q])
        self.check("ic_begin", idx)
        return nrm, bad

    def commit(self, idx):
        bad = np.full(idx.size, -1, dtype=np.int32)
        self.ctx._chk(self.ctx.H.idahip_ic_commit(self.ctx.h, self._i(bad)[0], *self._i(idx)), "ic_commit")
        for q, s in enumerate(idx):
            ewt, wbad = IC.commit(self.v["y0"][s], self.c["rtol"], self.atol)
            self.v["ewt"][s] = ewt
            for f, src in (("g0", "y0"), ("yy", "y0"), ("g1", "yp0"), ("yp", "yp0")):
                self.v[f][s] = self.v[src][s]
            assert bad[q] == int(wbad), ("ic_commit ewtbad", q, s, bad[q])
        self.check("ic_commit", idx)
        return bad

    def reset(self, idx):
        self.ctx._chk(self.ctx.H.idahip_ic_reset(self.ctx.h, *self._i(idx)), "ic_reset")
        for s in idx:
            self.v["y0"][s], self.v["yp0"][s] = self.v["g0"][s], self.v["g1"][s]
        self.check("ic_reset", idx)

    def accept(self, icopt, idx):
        self.ctx._chk(self.ctx.H.idahip_ic_accept(self.ctx.h, int(icopt), *self._i(idx)), "ic_accept")
        for s in idx:
            self.v["y0"][s], self.v["yp0"][s], self.v["delta"][s] = IC.accept(self.v["y0"][s], self.v["yp0"][s], self.v["yy"][s], self.v["yp"][s],
                                                                              self.v["delnew"][s], icopt)
        self.check("ic_accept icopt %d" % icopt, idx)

    def res(self, a, idx):
        self.ctx._chk(self.ctx.H.idahip_ic_res(self.ctx.h, self._p(a["tn"]), self._p(a["cj"]), *self._i(idx)), "ic_res")
        for q, s in enumerate(idx):
            r = self.residual(s, a["tn"][q], self.v["y0"][s], self.v["yp0"][s])
            self.v["delta"][s], self.v["savres"][s] = r, r.copy()
            self.v["yy"][s], self.v["yp"][s] = self.v["y0"][s], self.v["yp0"][s]
        self.check("ic_res", idx)

    def residual(self, s, tn, y, yp):
        if self.c["kind"] == "host_callback":  # (the only kind whose residual sees t)
            return np.asarray(self.c["data"]["res"](int(s), float(tn), y, yp), dtype=np.float64)
        return self.probs[s].res(y, yp)

    def setup(self, a, idx):
        """idahip_ic_setup, or idahip_ic_setup_dq on a DQ ctx -> info. The point and delta <- savres on the mirror; the listed
        systems' info, pivots and factors against the oracle's getrf of the restated Jacobian (by value, as everywhere in the
        suite) or, with restate_jac off, bit for bit against idahip_nls_lsetup on a fresh ctx at the same point and cj."""
        info = np.full(idx.size, -1, dtype=np.int32)
        H, h = self.ctx.H, self.ctx.h
        if self.c["dq"]:
            rc = H.idahip_ic_setup_dq(h, self._p(a["tn"]), self._p(a["cj"]), self._p(a["hh"]), self._i(info)[0], *self._i(idx))
        else:
            rc = H.idahip_ic_setup(h, self._p(a["tn"]), self._p(a["cj"]), self._i(info)[0], *self._i(idx))
        self.ctx._chk(rc, "ic_setup")
        self.fac.clear()
        for s in idx:
            self.v["yy"][s], self.v["yp"][s], self.v["delta"][s] = self.v["y0"][s], self.v["yp0"][s], self.v["savres"][s]
        self.check("ic_setup", idx)
        if self.restate_jac:
            for q, s in enumerate(idx):
                J = self.probs[s].jac(a["cj"][q], self.v["y0"][s], self.v["yp0"][s], self.v["savres"][s], a["hh"][q], self.v["ewt"][s])
                oinfo, olu, opiv = O.getrf(np.ascontiguousarray(J.T))
                assert info[q] == oinfo, ("ic_setup info", q, s, info[q], oinfo)
                if oinfo == 0:
                    lu, piv = self.factors(s)
                    assert np.array_equal(piv, opiv) and np.array_equal(lu, olu), ("ic_setup factors", q, s)
        else:
            self.against_fresh_ctx(a, idx, info, "ic_setup")
        return info

    def against_fresh_ctx(self, a, idx, info, what):
        """the listed systems' info, pivots and factors bit for bit against idahip_nls_lsetup on a fresh ctx with the mirror's yy, yp,
        savres and ewt"""
        twin = K.make_ctx(self.c)
        try:
            for f in ("yy", "yp", "savres", "ewt"):
                twin.upload(self.ids[f], self.v[f])
            _, tinfo = twin.nls_lsetup_dq(a["tn"], a["cj"], a["hh"], idx) if self.c["dq"] else twin.nls_lsetup(a["tn"], a["cj"], idx)
            assert np.array_equal(info, tinfo), (what, "info", info, tinfo)
            for q, s in enumerate(idx):
                if tinfo[q] == 0:
                    (lu, piv), (tlu, tpiv) = self.factors(s), self.factors(s, twin)
                    assert np.array_equal(piv, tpiv) and SR.same_bits(lu, tlu), (what, "factors against a fresh ctx", q, s)
        finally:
            twin.close()

    def lsetup(self, a, idx):
        """idahip_nls_lsetup (the stepper's setup, at the ctx's yy, yp) on the ctx the IC calls have used"""
        _, info = self.ctx.nls_lsetup(a["tn"], a["cj"], idx)
        self.fac.clear()
        assert (info == 0).all(), info
        self.against_fresh_ctx(a, idx, info, "nls_lsetup")
        self.check("nls_lsetup", idx)
        return info

    def solve(self, idx):
        nrm = np.full(idx.size, -1.0)
        self.ctx._chk(self.ctx.H.idahip_ic_solve(self.ctx.h, self._p(nrm), *self._i(idx)), "ic_solve")
        for q, s in enumerate(idx):
            lu, piv = self.factors(s)
            self.v["delta"][s], want = IC.solve_norm(lu, piv, self.v["delta"][s], self.v["ewt"][s])
            self.same_norm(nrm[q], want, ("ic_solve fnorm", q, s))
        self.check("ic_solve", idx)
        return nrm

    def trial(self, icopt, a, idx):
        nrm = np.full(idx.size, -1.0)
        self.ctx._chk(self.ctx.H.idahip_ic_trial(self.ctx.h, int(icopt), self._p(a["tn"]), self._p(a["cj"]), self._p(a["lam"]), self._p(nrm),
                                                 *self._i(idx)), "ic_trial")
        diff = (np.asarray(self.c["id"]) == 1.0) if icopt == IC.YA_YDP_INIT else np.zeros(self.n, dtype=bool)
        for q, s in enumerate(idx):
            y, yp = IC.trial_point(self.v["y0"][s], self.v["yp0"][s], self.v["delta"][s], a["lam"][q], a["cj"][q], diff)
            self.v["yy"][s], self.v["yp"][s] = y, yp
            self.v["savres"][s] = self.residual(s, a["tn"][q], y, yp)
            lu, piv = self.factors(s)
            self.v["delnew"][s], want = IC.solve_norm(lu, piv, self.v["savres"][s], self.v["ewt"][s])
            self.same_norm(nrm[q], want, ("ic_trial fnormp icopt %d" % icopt, q, s))
        self.check("ic_trial icopt %d" % icopt, idx)
        return nrm
