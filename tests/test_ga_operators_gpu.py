"""monsoon_ga_offspring (k_ga_offspring) and monsoon_ga_select (k_ga_select) beyond power-of-two mu and plain sigmas: the
cases of tests/ga_cases.py against the host GA run by numpy itself right here -- mu that is no power of two (the
rejection loop of NpStream::interval takes its back edge), mu = 1, dim 1..16, the min_sigma clamp firing, inf and NaN
sigmas, every kind of stream state to enter with --, a chain of calls against one continuous stream, the Population
wrapper at the project's default mu = lambda = 10, the selection order at the sizes around its 256-thread block with
ties, signed zeros, infinities and subnormals, and the refusals of both entry points.

Bounds: parents, polar-method rounds and the stream state are identical; the cached normal within 4 ulp, sigmas within
4 ulp, weights within 1e-15 -- what test_gpu_parity.test_ga_operators_on_device holds the device to (exp / log / sqrt are
the device library's)."""
import ctypes

import numpy as np
import pytest

import ga_cases as G
from monsoon_amd import _lib
from monsoon_amd.config import EvolutionaryConfig
from monsoon_amd.engine import BatchEngine
from monsoon_amd.population import Population
from test_oracle_golden import orc_ga_arrays, ulps

pytestmark = pytest.mark.gpu

GAUSS_ULP, SIGMA_ULP, WEIGHT_ABS = 4, 4, 1e-15


@pytest.fixture(scope="module")
def eng():
    e = BatchEngine(64)   # the GA operators need no loaded games
    yield e
    e.close()


def _same_state(state, want):
    (k, p, h, g), (wk, wp, wh, wg) = G.abs_state(state), G.abs_state(want)
    assert np.array_equal(k, wk) and (p, h) == (wp, wh)
    assert ulps([g], [wg]).max() <= GAUSS_ULP


def test_offspring_over_the_case_table(eng):
    worst = {}
    for i, case in enumerate(G.cases()):
        ref = G.reference(i)
        ow, osg, par, tries, st1 = eng.ga_offspring(case.entry, case.pw, case.ps, case.lam, case.tau, case.tau_prime, case.min_sigma)
        o = orc_ga_arrays(*G.abs_state(case.entry), case.pw, case.ps, case.lam, case.tau, case.tau_prime, case.min_sigma)
        want_parent, want_tries = ref.parent, o[3]
        assert np.array_equal(par, want_parent), case.name
        assert np.array_equal(tries, want_tries), case.name
        _same_state(st1, ref.state)
        worst_s, worst_w = G.compare(ow, osg, ref, ulps)
        print(f"{case.name}: sigmas within {worst_s} ulp, weights within {worst_w:.2e}")
        family = case.name.split("/")[0].split("-")[0]
        worst[family] = tuple(max(a, b) for a, b in zip(worst.get(family, (0, 0.0)), (worst_s, worst_w)))
        assert worst_s <= SIGMA_ULP and worst_w <= WEIGHT_ABS, (case.name, worst_s, worst_w)
    print("device GA offspring vs numpy, worst per family:", {k: (v[0], f"{v[1]:.2e}") for k, v in worst.items()})


def test_chain_of_calls_equals_one_continuous_stream(eng):
    """Five calls with the returned state fed forward against numpy drawing all 165 children in one go: the cached normal
    crosses every call boundary, and the state after the fifth is numpy's."""
    case, ref = G.chain_case(), G.chain_reference()
    state, ws, ss, ps, cached = case.entry, [], [], [], []
    for _ in range(G.CHAIN[3]):
        ow, osg, par, _, state = eng.ga_offspring(state, case.pw, case.ps, case.lam, case.tau, case.tau_prime, case.min_sigma)
        ws.append(ow), ss.append(osg), ps.append(par), cached.append(state[3])
    assert cached == [1, 0, 1, 0, 1]
    got_parent, want_parent = np.concatenate(ps), ref.parent
    assert np.array_equal(got_parent, want_parent)
    _same_state(state, ref.state)
    worst_s, worst_w = G.compare(np.concatenate(ws), np.concatenate(ss), ref, ulps)
    print(f"chain: sigmas within {worst_s} ulp, weights within {worst_w:.2e}")
    assert worst_s <= SIGMA_ULP and worst_w <= WEIGHT_ABS, (worst_s, worst_w)


def test_wrapper_at_the_default_population(eng):
    """Population at the project's default mu = lambda_ = 10 (numpy rejects 38 % of the parent draws): three consecutive
    generate_offspring calls on the host and on the device from the same numpy state.  Between calls the parents become
    the HOST's children on both sides, so a difference of a few ulp cannot grow into another parent set."""
    saved = np.random.get_state()
    try:
        cfg = EvolutionaryConfig(seed=20261)
        assert cfg.mu == 10 and cfg.lambda_ == 10
        pop = Population(cfg)
        pop.initialize_population(10)
        first, start = list(pop.individuals), np.random.get_state()
        host = []
        for _ in range(3):
            host.append(pop.generate_offspring())
            pop.individuals = host[-1]
        host_state = np.random.get_state()
        np.random.set_state(start)
        pop.individuals = first
        for r in range(3):
            kids = pop.generate_offspring(engine=eng)
            w0, s0 = np.stack([k.weights for k in host[r]]), np.stack([k.sigmas for k in host[r]])
            w1, s1 = np.stack([k.weights for k in kids]), np.stack([k.sigmas for k in kids])
            worst_w, worst_s = float(np.abs(w0 - w1).max()), int(ulps(s0, s1).max())
            assert worst_w <= WEIGHT_ABS and worst_s <= SIGMA_ULP, (r, worst_w, worst_s)
            pop.individuals = host[r]
        k0, p0, h0, g0 = G.abs_state(host_state)
        k1, p1, h1, g1 = G.abs_state(np.random.get_state())
        assert np.array_equal(k0, k1) and (p0, h0) == (p1, h1) and ulps([g0], [g1]).max() <= GAUSS_ULP
    finally:
        np.random.set_state(saved)


def _fitness_patterns(n):
    rs = np.random.RandomState(n)
    tiny = np.float64(5e-324)
    zeros = np.where(rs.randint(0, 2, n) == 1, 0.0, -0.0)
    yield "all equal", np.full(n, 0.25)
    yield "ascending", np.arange(n) / 8.0 - 3.0
    yield "descending", 3.0 - np.arange(n) / 8.0
    yield "dense ties", np.round(rs.uniform(0, 1, n), 1)
    yield "signed zeros", zeros
    yield "signed zeros among values", np.where(rs.randint(0, 3, n) == 0, rs.choice([-0.5, 0.5], n), zeros)
    yield "infinities", rs.choice([np.inf, -np.inf, 0.0, 1.5, -1.5, 1e308, -1e308], n)
    yield "subnormals", rs.randint(-3, 4, n) * tiny
    yield "subnormals among values", rs.choice([tiny, -tiny, 0.0, -0.0, 2.2250738585072014e-308, 1e-310, -1e-310], n)


@pytest.mark.parametrize("n", [1, 2, 255, 256, 257, 513])
def test_select_equals_pythons_stable_sort(eng, n):
    """n = 1, 2, both sides of one 256-thread block and into a third block; equal keys keep their original order, -0.0
    equals 0.0 as it does to Python's sort."""
    for name, fit in _fitness_patterns(n):
        fit = np.asarray(fit, dtype=np.float64)
        want = [i for _, i in sorted(zip(fit.tolist(), range(n)), key=lambda p: p[0], reverse=True)]
        got = eng.ga_select(fit)
        assert got.dtype == np.int32 and got.tolist() == want, (name, n)


def _np_state(state):
    st = _lib.NpState()
    key, st.pos, st.has_gauss, st.gauss = G.abs_state(state)
    ctypes.memmove(st.key, np.ascontiguousarray(key).ctypes.data, 624 * 4)
    return st


def test_refusals_write_nothing_and_leave_the_handle_usable(eng):
    """monsoon_ga_offspring with dim 0 or 17, mu 0, lambda 0, a position of -1 or 625, and monsoon_ga_select with a NaN
    fitness or n = 0: MONSOON_ERR_ARG, the outputs and the passed state keep their bytes, and a valid call on the same
    handle afterwards gives the known answer."""
    i = next(k for k, c in enumerate(G.cases()) if c.name == "shape-10-10-64/mid-gauss")
    case, ref = G.cases()[i], G.reference(i)
    p = lambda a: a.ctypes.data_as(ctypes.c_void_p)   # noqa: E731
    pw, ps = np.ascontiguousarray(case.pw), np.ascontiguousarray(case.ps)
    for what, mu, dim, lam, pos in (("dim 0", 10, 0, 64, None), ("dim 17", 10, 17, 64, None), ("mu 0", 0, 10, 64, None), ("lambda 0", 10, 10, 0, None),
                                    ("pos -1", 10, 10, 64, -1), ("pos 625", 10, 10, 64, 625)):
        st = _np_state(case.entry)
        if pos is not None:
            st.pos = pos
        before = bytes(st)
        ow, osg = np.full((64, 17), 7.5), np.full((64, 17), 7.5)   # room for what a call that went through would write
        par, tries = np.full(64, -7, dtype=np.int32), np.full(64, -7, dtype=np.int64)
        rc = eng.lib.monsoon_ga_offspring(eng.h, ctypes.byref(st), p(pw), p(ps), mu, dim, lam, case.tau, case.tau_prime, case.min_sigma,
                                          p(ow), p(osg), p(par), p(tries))
        assert rc == _lib.ERR_ARG, what
        assert bytes(st) == before, what
        assert (ow == 7.5).all() and (osg == 7.5).all() and (par == -7).all() and (tries == -7).all(), what
    fit = np.array([0.5, np.nan, 0.25, 1.0])
    order = np.full(4, -7, dtype=np.int32)
    assert eng.lib.monsoon_ga_select(eng.h, p(fit), 4, p(order)) == _lib.ERR_ARG and (order == -7).all()
    fit[1] = 0.5
    assert eng.lib.monsoon_ga_select(eng.h, p(fit), 0, p(order)) == _lib.ERR_ARG and (order == -7).all()
    assert eng.ga_select(fit).tolist() == [3, 0, 1, 2]
    ow, osg, par, _, st1 = eng.ga_offspring(case.entry, case.pw, case.ps, case.lam, case.tau, case.tau_prime, case.min_sigma)
    want_parent = ref.parent
    assert np.array_equal(par, want_parent)
    _same_state(st1, ref.state)
    worst_s, worst_w = G.compare(ow, osg, ref, ulps)
    assert worst_s <= SIGMA_ULP and worst_w <= WEIGHT_ABS
