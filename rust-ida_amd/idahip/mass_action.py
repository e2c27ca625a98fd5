"""IDAHIP_MASS_ACTION on the Python side, without a device: the network a caller writes as a list of reactions, checked and
flattened into the arrays idahip_set_mass_action takes, and the two tables the library builds from them (the residual's row-CSR, the
Jacobian pattern's CSR) restated in numpy -- Ctx.set_mass_action checks with `flatten` before it calls the library, the tests compare
`tables` with what the library reports (idahip_mass_action_pattern). include/ida_hip.h has the definition. `flatten_laws`,
`tables_laws` and `rhs_laws` are the same for a network with rate laws (idahip_set_rate_network), further down.

A network is (reactions, d): reactions = [(reactants, {row: nu, ...}), ...] with `reactants` a sequence of at most three species
indices (repeats allowed) and the dict's items in the order the caller wrote them; d [n] the coefficients of y'. Entries are
numbered reaction by reaction, so within a row they keep the order of the reactions (and of a dict's items).
"""
import numpy as np


class NetworkError(ValueError):
    pass


def flatten(n, reactions, d):
    """-> (reactants int32 [R][3], rows int32 [E], reacs int32 [E], nu float64 [E], d float64 [n]); NetworkError naming the first
    offending item, in the order the library checks: reactions, then entries, then d."""
    n = int(n)
    reactions = list(reactions)
    R = len(reactions)
    if R < 1:
        raise NetworkError("nreac = %d, at least one reaction" % R)
    slots = np.full((R, 3), -1, dtype=np.int32)
    for r, (reactants, _) in enumerate(reactions):
        reactants = list(reactants)
        if len(reactants) > 3:
            raise NetworkError("reaction %d: order %d, at most 3" % (r, len(reactants)))
        ended = False
        for p, sp in enumerate(reactants):
            sp = int(sp)
            if sp < -1 or sp >= n:
                raise NetworkError("reaction %d, slot %d: species %d outside [0, %d)" % (r, p, sp, n))
            if sp == -1:
                ended = True
            elif ended:
                raise NetworkError("reaction %d, slot %d: a species after an unused slot (-1 only in trailing slots)" % (r, p))
            slots[r, p] = sp
    rows, reacs, nu = [], [], []
    for r, (_, stoich) in enumerate(reactions):
        for row, v in (stoich.items() if hasattr(stoich, "items") else stoich):
            e = len(rows)
            if int(row) < 0 or int(row) >= n:
                raise NetworkError("entry %d: row %d outside [0, %d)" % (e, int(row), n))
            if not np.isfinite(v):
                raise NetworkError("entry %d: nu = %g is not finite" % (e, v))
            rows.append(int(row))
            reacs.append(r)
            nu.append(float(v))
    d = np.ascontiguousarray(np.asarray(d, dtype=np.float64))
    if d.shape != (n,):
        raise NetworkError("d has shape %s, not (%d,)" % (d.shape, n))
    for i in range(n):
        if not np.isfinite(d[i]):
            raise NetworkError("d[%d] = %g is not finite" % (i, d[i]))
    return slots, np.array(rows, dtype=np.int32), np.array(reacs, dtype=np.int32), np.array(nu, dtype=np.float64), d


def tables(n, reactions, d):
    """The library's two tables: dict(slots, d, rows: per row the list of (nu, r) in entry order, pattern: {(i, j): [(nu, r, others)]}
    in the header's term order with every diagonal position present, order: the positions column-major, nnz, ml, mu)."""
    slots, rows, reacs, nu, d = flatten(n, reactions, d)
    by_row = [[] for _ in range(n)]
    for e in range(rows.size):
        by_row[rows[e]].append((float(nu[e]), int(reacs[e])))
    pattern = {(i, i): [] for i in range(n)}
    for i in range(n):
        for v, r in by_row[i]:
            s = [int(x) for x in slots[r] if x >= 0]
            for p, j in enumerate(s):
                pattern.setdefault((i, j), []).append((v, r, tuple(s[:p] + s[p + 1:])))
    order = sorted(pattern, key=lambda ij: (ij[1], ij[0]))
    return {"slots": slots, "d": d, "rows": by_row, "pattern": pattern, "order": order, "nnz": len(order),
            "ml": max(i - j for i, j in order), "mu": max(j - i for i, j in order)}


def rhs(tab, k, y):
    """acc_i of every row in the header's operation order (F_i = d_i y'_i - acc_i): the right-hand side a generator needs for
    consistent initial derivatives. tab = tables(...); k [R]; y [n]."""
    k, y = np.asarray(k, dtype=np.float64), np.asarray(y, dtype=np.float64)
    slots = tab["slots"]
    out = np.zeros(y.size)
    with np.errstate(all="ignore"):
        for i, row in enumerate(tab["rows"]):
            acc = None
            for v, r in row:
                q = k[r]
                for sp in slots[r]:
                    if sp >= 0:
                        q = q * y[sp]
                t = np.float64(v) * q
                acc = t if acc is None else acc + t
            out[i] = 0.0 if acc is None else acc
    return out


# ------------------------------------------------------------------------------------------------ rate laws (idahip_set_rate_network)
# A reaction may carry a third item: factors = [(op, species, constant, h), ...], at most 4, op "sat" (y^h / (K^h + y^h)) or "inh"
# (K^h / (K^h + y^h)) -- or the header's numbers 1 and 2 --, 1 <= h <= 4. A system's parameters are [k_0 .. k_{R-1}, K_0 ..
# K_{nconst-1}]. include/ida_hip.h has the operation order.
RATE_SAT, RATE_INH, RATE_MAX_FACTORS = 1, 2, 4
_OPS = {"sat": RATE_SAT, "inh": RATE_INH, RATE_SAT: RATE_SAT, RATE_INH: RATE_INH}


def _factors_of(reaction):
    return list(reaction[2]) if len(reaction) > 2 else []


def flatten_laws(n, reactions, d, nconst):
    """-> (reactants [R][3], factors int32 [nfac][5] = (reaction, op, species, constant, exponent), rows, reacs, nu, d); NetworkError
    naming the first offending item, in the order and with the texts of the library: reactions, then factors, then entries, then d."""
    n, nconst = int(n), int(nconst)
    reactions = [tuple(r) for r in reactions]
    plain = [(r[0], r[1]) for r in reactions]
    R = len(plain)
    if R < 1:
        raise NetworkError("nreac = %d, at least one reaction" % R)
    if nconst < 0:
        raise NetworkError("nconst = %d is negative" % nconst)
    # (reactions first: flatten's own checks of the slots; its entry and d checks come after the factors')
    flatten(n, [(r[0], {}) for r in plain], np.zeros(n))
    fac, count = [], [0] * R
    for r, reaction in enumerate(reactions):
        for op, sp, c, h in _factors_of(reaction):
            f = len(fac)
            code = _OPS.get(op, op)
            if code not in (RATE_SAT, RATE_INH):
                raise NetworkError("factor %d: op %s is neither IDAHIP_RATE_SAT (1) nor IDAHIP_RATE_INH (2)" % (f, code))
            sp, c, h = int(sp), int(c), int(h)
            if sp < 0 or sp >= n:
                raise NetworkError("factor %d: species %d outside [0, %d)" % (f, sp, n))
            if c < 0 or c >= nconst:
                raise NetworkError("factor %d: constant %d outside [0, %d)" % (f, c, nconst))
            if h < 1 or h > 4:
                raise NetworkError("factor %d: exponent %d outside [1, 4]" % (f, h))
            count[r] += 1
            if count[r] > RATE_MAX_FACTORS:
                raise NetworkError("factor %d: reaction %d has more than %d factors" % (f, r, RATE_MAX_FACTORS))
            fac.append((r, code, sp, c, h))
    slots, rows, reacs, nu, d = flatten(n, plain, d)
    return slots, np.array(fac, dtype=np.int32).reshape(-1, 5), rows, reacs, nu, d


def tables_laws(n, reactions, d, nconst):
    """tables() with rate laws: the same dict, and nreac, nconst, factors: per reaction the list of (op, species, constant, h) in the
    caller's order. A pattern term is (nu, r, slots, dfac): dfac = -1 for a slot's term (slots: the OTHER slots), and for the term of
    the reaction's factor number dfac all the slots. Within an entry the slots' terms come first, then the factors'."""
    slots, fac, rows, reacs, nu, d = flatten_laws(n, reactions, d, nconst)
    R = slots.shape[0]
    factors = [[] for _ in range(R)]
    for r, op, sp, c, h in fac:
        factors[r].append((int(op), int(sp), int(c), int(h)))
    by_row = [[] for _ in range(n)]
    for e in range(rows.size):
        by_row[rows[e]].append((float(nu[e]), int(reacs[e])))
    pattern = {(i, i): [] for i in range(n)}
    for i in range(n):
        for v, r in by_row[i]:
            s = [int(x) for x in slots[r] if x >= 0]
            for p, j in enumerate(s):
                pattern.setdefault((i, j), []).append((v, r, tuple(s[:p] + s[p + 1:]), -1))
            for q, (_, sp, _, _) in enumerate(factors[r]):
                pattern.setdefault((i, sp), []).append((v, r, tuple(s), q))
    order = sorted(pattern, key=lambda ij: (ij[1], ij[0]))
    return {"slots": slots, "d": d, "rows": by_row, "pattern": pattern, "order": order, "nnz": len(order), "nreac": R, "nconst": int(nconst),
            "factors": factors, "ml": max(i - j for i, j in order), "mu": max(j - i for i, j in order)}


def _pw(x, h):
    p = x
    for _ in range(h - 1):
        p = p * x
    return p


def factor_value(op, y, K, h):
    """f(factor) in the header's operation order, as np.float64 (a zero denominator gives what IEEE gives, no exception)"""
    y, K = np.float64(y), np.float64(K)
    with np.errstate(all="ignore"):
        yh, Kh = _pw(y, h), _pw(K, h)
        den = Kh + yh
        return (yh if op == RATE_SAT else Kh) / den


def rhs_laws(tab, params, y):
    """rhs() with rate laws: tab = tables_laws(...); params [R + nconst] = the rate constants, then the constants; y [n]."""
    params, y = np.asarray(params, dtype=np.float64), np.asarray(y, dtype=np.float64)
    slots, R = tab["slots"], tab["nreac"]
    out = np.zeros(y.size)
    with np.errstate(all="ignore"):
        for i, row in enumerate(tab["rows"]):
            acc = None
            for v, r in row:
                q = params[r]
                for sp in slots[r]:
                    if sp >= 0:
                        q = q * y[sp]
                for op, sp, c, h in tab["factors"][r]:
                    q = q * factor_value(op, y[sp], params[R + c], h)
                t = np.float64(v) * q
                acc = t if acc is None else acc + t
            out[i] = 0.0 if acc is None else acc
    return out
