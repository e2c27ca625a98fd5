"""Launch sizes of the batched LU inside the device lock-step rounds (idahip_round_solve, include/ida_hip.h:
idahip_set_lu_count_on_host, idahip_set_lu_slow_grid). With the count on the host every LU launch of a round has exactly the
workgroups its list needs and a round without setups launches none; with the count on the device the launches are sized for the
batch. The panels' SLOW launches walk the list their FAST launches wrote, with any grid. None of this may show in a result: both
count paths, every SLOW grid and the CPU oracle agree bit for bit -- states, step sizes, orders, counters, factors, pivots, info."""
import functools

import numpy as np
import pytest

import oracle_lib as O
from test_gpu_ensemble import CNT, run_oracle
from test_gpu_device_controller import same, state
from test_gpu_lsolver import colmajor, oracle_lu

pytestmark = pytest.mark.gpu
BATCH = 24


def make(prob, host_count, period=1, jac_in_lu=None, slow_grid=0):
    import idahip
    from idahip import problems
    ctx = problems.make_ctx(prob)
    ctx.set_lu_count_on_host(host_count)
    assert ctx.lu_count_on_host() == host_count  # the path that will really run
    ctx.set_lu_period(period)
    ctx.set_lu_slow_grid(slow_grid)
    if jac_in_lu is not None:
        ctx.set_jac_in_lu(jac_in_lu)
        assert ctx.jac_in_lu() == (2 if jac_in_lu else 0)
    ens = idahip.Ensemble(ctx, prob["yy0"], prob["yp0"])
    ens.set_device_controller(1)
    assert ens.device_controller_active() == 2  # the lock-step rounds, not the host stepper
    return ctx, ens


@functools.lru_cache(maxsize=None)
def dense_case(n):
    """The problem and the oracle's whole schedule, computed once per size."""
    from idahip import problems
    prob = problems.linear_dense(n=n, batch=BATCH, procs=1)
    ref = run_oracle(prob)
    assert (ref["status"] == 0).all()
    return prob, ref


def equals_oracle_at_the_end(ens, ref):
    c = ens.counters()
    for k in CNT:
        assert np.array_equal(c[k], ref["counters"][k]), k
    assert np.array_equal(c["kused"], ref["kused"]) and np.array_equal(ens.real("hused"), ref["hused"])
    assert np.array_equal(ens.yy(), ref["yy"][-1]) and np.array_equal(ens.yp(), ref["yp"][-1])


# n = 64: one super-panel, no trailing launch; 72: a partial second super-panel; 200: partial strips and column blocks; 512: eight slots,
# J formed by the first launches (the library's choice above 448 rows); 200 with J formed inside on request: the <false, 0, LuJac> launch
@pytest.mark.parametrize("n,jac_in_lu", [(64, None), (72, None), (200, None), (512, None), (200, 1)])
def test_factorisation_through_the_round_path_at_exact_size(n, jac_in_lu):
    prob, ref = dense_case(n)
    cd, dev = make(prob, 0, jac_in_lu=jac_in_lu)
    ch, host = make(prob, 1, jac_in_lu=jac_in_lu)
    if n == 512:
        assert ch.jac_in_lu() == 1
    for i, t in enumerate(prob["touts"]):
        sd, td = dev.solve(t)
        sh, th = host.solve(t)
        assert (sh == 0).all() and np.array_equal(sd, sh) and np.array_equal(td, th)
        same(state(host), state(dev))
        assert np.array_equal(host.yy(), ref["yy"][i]) and np.array_equal(host.yp(), ref["yp"][i])
    equals_oracle_at_the_end(host, ref)
    equals_oracle_at_the_end(dev, ref)
    assert host.total_rounds() == dev.total_rounds()
    # the same kernels served the same systems: the statistics of every kernel class agree
    td_, th_ = cd.timing_get(), ch.timing_get()
    for k in ("sys", "sys_jac", "jac", "lu", "newton_iter"):
        assert td_[k]["systems"] == th_[k]["systems"], k
    for e in (dev, host):
        e.close()
    for c in (cd, ch):
        c.close()


def lu_count(ctx, before):
    now = ctx.timing_get()["lu"]["systems"]
    return now - before, now


def test_counts_at_the_edges_of_a_workgroup_octet():
    """The trailing grid is ((nsys + 7) / 8) * 8 * ncb workgroups. n = 200, 24 systems, setups batched over 3 rounds; calls of one
    and two rounds, so that the host's wait for the count is met at a call's first and last round. (a) the schedule from a common
    start: all 24 set up in round 0, later rounds as the systems ask, postponed rounds set up none -- to the end, against the oracle;
    (b) staggered starts in throughput mode: with a stagger of 24 rounds one system enters per round, of 12 two, of 3 eight -- a
    system sets up in its first round, so the first lists have 1, 2 and 8 entries -- and the lists then grow with the systems under
    way, through 7 and 9. The count of every one-round call is read from the kernel statistics; the test insists that the lengths
    it is about have occurred."""
    prob, ref = dense_case(200)
    touts = prob["touts"]
    seen = set()
    # (a)
    cd, dev = make(prob, 0, period=3)
    ch, host = make(prob, 1, period=3)
    lud = luh = 0
    for i in range(20000):
        k = 1 + i % 2
        sd, _, rd = dev.solve_schedule(touts, max_rounds=k)
        sh, _, rh = host.solve_schedule(touts, max_rounds=k)
        assert np.array_equal(sd, sh) and np.array_equal(rd, rh)
        same(state(host), state(dev))
        nd, lud = lu_count(cd, lud)
        nh, luh = lu_count(ch, luh)
        assert nd == nh
        if k == 1:
            seen.add(nh)
        if (sh != 99).all():
            break
    assert (sh == 0).all()
    equals_oracle_at_the_end(host, ref)
    assert {0, BATCH} <= seen, sorted(seen)
    for e in (dev, host):
        e.close()
    for c in (cd, ch):
        c.close()
    # (b)
    for stagger in (24, 12, 3):
        cd, dev = make(prob, 0, period=3)
        ch, host = make(prob, 1, period=3)
        lud = luh = 0
        for i in range(36):
            k = 1 if i < 30 else 2
            assert dev.stream(touts, k, stagger_rounds=stagger) == host.stream(touts, k, stagger_rounds=stagger)
            same(state(host), state(dev))
            nd, lud = lu_count(cd, lud)
            nh, luh = lu_count(ch, luh)
            assert nd == nh
            if k == 1:
                seen.add(nh)
        for e in (dev, host):
            e.close()
        for c in (cd, ch):
            c.close()
    print("list lengths of the one-round calls:", sorted(seen))
    assert {0, 1, 7, 8, 9, BATCH} <= seen, sorted(seen)


def special_matrices(n, nspecial, total=8):
    """`total` random matrices of which the first `nspecial` leave the panels' FAST mode: exact zeros, a NaN, an infinity, pivot ties
    (the constructions of tests/test_gpu_lsolver.py), in turn."""
    rng = np.random.default_rng(1000 * n + nspecial)
    mats = rng.standard_normal((total, n, n))
    for s in range(nspecial):
        what = s % 4
        if what == 0:  # exact zeros, many of them
            mats[s] = np.where(rng.random((n, n)) < 0.3, 0.0, mats[s]) + 3.0 * np.eye(n)
        elif what == 1:  # a NaN below the diagonal: never chosen in its column, poisons its row
            mats[s, n - 2, 3] = np.nan
        elif what == 2:  # an infinity wins its column
            mats[s, 7, 70 % n] = np.inf
        else:  # many exact ties in |a|, many zeros
            mats[s] = rng.integers(-2, 3, size=(n, n)).astype(float) + 3.0 * np.eye(n)
    return mats


@functools.lru_cache(maxsize=None)
def special_case(n, nspecial):
    mats = special_matrices(n, nspecial)
    return mats, oracle_lu(mats)


@pytest.mark.parametrize("grid", [1, 2, 0], ids=["grid1", "grid2", "auto"])
@pytest.mark.parametrize("nspecial", [0, 1, 5, 8])
@pytest.mark.parametrize("n", [128, 200])
def test_slow_list_with_any_grid(n, nspecial, grid):
    """The SLOW launches take their matrices from the list the FAST launches wrote. Grid 1 and 2: one or two waves walk it, several
    entries each; automatic: a wave per listed system. Factors, pivots and info against the oracle."""
    import idahip
    mats, (info_o, lu_o, piv_o) = special_case(n, nspecial)
    B = mats.shape[0]
    ctx = idahip.Ctx("linear_dense", n, B)
    ctx.set_lu_slow_grid(grid)
    dA = ctx.dev_array(colmajor(mats))
    dP = ctx.dev_empty(8 * B * n)
    rc, info = ctx.ls_setup(dA, dP, None)
    lu = np.transpose(ctx.to_host(dA, (B, n, n)), (0, 2, 1))
    piv = ctx.to_host(dP, (B, n), dtype=np.int64)
    assert np.array_equal(info, info_o)
    ok = info_o == 0
    assert np.array_equal(piv[ok], piv_o[ok])
    assert np.array_equal(np.isnan(lu[ok]), np.isnan(lu_o[ok]))
    assert np.array_equal(lu[ok], lu_o[ok], equal_nan=True)
    ctx.close()


@pytest.mark.parametrize("grid", [1, 2, 0], ids=["grid1", "grid2", "auto"])
@pytest.mark.parametrize("n", [128, 200])
def test_a_zero_pivot_in_the_slow_pass_spares_the_entries_behind_it(n, grid):
    """System 0 has exact zeros (its panels go to the SLOW pass from the first block on) and an all-zero column 70: the SLOW pass of
    the second super-panel meets the zero pivot, sets info and must go on to the next entries of its list -- five more matrices with
    zeros, a NaN, an infinity and ties, walked by one or two waves -- and the later super-panels must leave system 0 alone."""
    import idahip
    mats = special_matrices(n, 6).copy()
    mats[0, :, 70] = 0.0
    info_o, lu_o, piv_o = oracle_lu(mats)
    assert info_o[0] == 71 and (info_o[1:] == 0).sum() >= 5
    B = mats.shape[0]
    ctx = idahip.Ctx("linear_dense", n, B)
    ctx.set_lu_slow_grid(grid)
    dA = ctx.dev_array(colmajor(mats))
    dP = ctx.dev_empty(8 * B * n)
    rc, info = ctx.ls_setup(dA, dP, None)
    lu = np.transpose(ctx.to_host(dA, (B, n, n)), (0, 2, 1))
    piv = ctx.to_host(dP, (B, n), dtype=np.int64)
    assert rc == 1 and np.array_equal(info, info_o)
    ok = info_o == 0
    assert np.array_equal(piv[ok], piv_o[ok])
    assert np.array_equal(np.isnan(lu[ok]), np.isnan(lu_o[ok]))
    assert np.array_equal(lu[ok], lu_o[ok], equal_nan=True)
    ctx.close()


@pytest.mark.parametrize("grid", [0, 2], ids=["auto", "grid2"])
def test_slow_list_inside_the_rounds(grid):
    """A banded Jacobian in dense storage (the heat equation's) sends every super-panel of every matrix through the SLOW launch. 40
    systems with the count on the host: the automatic grid of the first round is 32 workgroups for 40 entries, later ones follow
    the last round's list; both count paths and the oracle agree."""
    from idahip import problems
    prob = problems.heat1d(n=72, batch=40)
    touts = [float(t) for t in prob["touts"][:4]]
    cd, dev = make(prob, 0)
    ch, host = make(prob, 1, slow_grid=grid)
    for t in touts:
        sd, td = dev.solve(t)
        sh, th = host.solve(t)
        assert (sh == 0).all() and np.array_equal(sd, sh) and np.array_equal(td, th)
        same(state(host), state(dev))
    ref = run_oracle(prob, touts)
    c = host.counters()
    for k in CNT:
        assert np.array_equal(c[k], ref["counters"][k]), k
    assert np.array_equal(host.yy(), ref["yy"][-1]) and np.array_equal(host.yp(), ref["yp"][-1])
    for e in (dev, host):
        e.close()
    for c in (cd, ch):
        c.close()


def test_two_groups_with_the_count_on_the_host_equal_the_single_ensemble():
    """Two groups of 12 at n = 64 side by side on two streams, each waiting for its own count every round, against the same 24
    systems as one ensemble with the count on the device: per-system states, counters and totals after the same rounds."""
    import idahip
    from idahip import problems
    prob, _ = dense_case(64)
    touts = prob["touts"]
    parts = [{k: (v[lo:lo + 12] if isinstance(v, np.ndarray) and v.ndim >= 1 and v.shape[0] == BATCH else v) for k, v in prob.items()}
             for lo in (0, 12)]
    made = [make(p, 1) for p in parts]
    side = [e for _, e in made]
    c1, one = make(prob, 0)
    for k in (40, 1, 17):  # (no stagger: a system's start round would depend on the size of its group)
        done = idahip.stream_group(side, touts, k, stagger_rounds=0, offset_us=200)
        assert sum(done) == one.stream(touts, k)
        assert all(e.total_rounds() == one.total_rounds() for e in side)
        assert sum(e.total_newton_iters() for e in side) == one.total_newton_iters()
        parts_state = [state(e) for e in side]
        same({k_: np.concatenate([s[k_] for s in parts_state]) for k_ in parts_state[0]}, state(one))
    assert sum(done) > 0
    for e in side + [one]:
        e.close()
    for c in [c for c, _ in made] + [c1]:
        c.close()
