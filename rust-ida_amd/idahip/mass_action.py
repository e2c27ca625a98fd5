"""IDAHIP_MASS_ACTION on the Python side, without a device: the network a caller writes as a list of reactions, checked and
flattened into the arrays idahip_set_mass_action takes, and the two tables the library builds from them (the residual's row-CSR, the
Jacobian pattern's CSR) restated in numpy -- Ctx.set_mass_action checks with `flatten` before it calls the library, the tests compare
`tables` with what the library reports (idahip_mass_action_pattern). include/ida_hip.h has the definition.

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
