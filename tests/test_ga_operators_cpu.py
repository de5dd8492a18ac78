"""orc_ga_offspring, the CPU restatement of monsoon_ga_offspring, over the cases of tests/ga_cases.py against the host GA
run by numpy itself right here: mu that is no power of two (the rejection loop of randint's masked draw takes its back
edge), mu = 1 (no draw), dim 1..16, the min_sigma clamp firing, inf and NaN sigmas, and stream states entered freshly
seeded, mid-block with and without a cached normal and at positions 623, 1 and 0.  The conditions that say a case
reaches its branch are asserted on the reference alone."""
import numpy as np
import pytest

import ga_cases as G
from test_oracle_golden import orc_ga_arrays, ulps

SIGMA_ULP, WEIGHT_ABS = 2, 4e-16   # the bounds of test_ga_offspring_restatement_vs_numpy (numpy's array exp is its own SIMD routine)


def _orc(case, entry=None):
    key, pos, hg, gs = G.abs_state(case.entry if entry is None else entry)
    return orc_ga_arrays(key, pos, hg, gs, case.pw, case.ps, case.lam, case.tau, case.tau_prime, case.min_sigma)


def _same_state(key, pos, hg, gs, state):
    k, p, h, g = G.abs_state(state)
    assert np.array_equal(key, k) and (pos, hg) == (p, h)
    assert ulps([gs], [g]).max() == 0   # the cached normal, bit for bit


@pytest.mark.parametrize("index", range(len(G.cases())), ids=[c.name for c in G.cases()])
def test_restatement_equals_numpy(index):
    case, ref = G.cases()[index], G.reference(index)
    ow, osg, par, tries, key, pos, hg, gs = _orc(case)
    want_parent = ref.parent
    assert np.array_equal(par, want_parent)
    _same_state(key, pos, hg, gs, ref.state)
    worst_s, worst_w = G.compare(ow, osg, ref, ulps)
    assert worst_s <= SIGMA_ULP and worst_w <= WEIGHT_ABS, (worst_s, worst_w)
    assert (np.diff(tries) >= case.dim).all() and tries[0] >= case.dim   # 1 + 2 dim normals a child: at least dim rounds


def test_chain_of_calls_equals_one_continuous_stream():
    """Five calls, each entering with the state the one before handed back, against numpy drawing all 165 children in one
    go: the cached normal crosses every call boundary."""
    case, ref = G.chain_case(), G.chain_reference()
    lam, calls = G.CHAIN[2], G.CHAIN[3]
    state, ws, ss, ps, cached = case.entry, [], [], [], []
    for _ in range(calls):
        ow, osg, par, _, key, pos, hg, gs = _orc(case, state)
        state = ("MT19937", key, pos, hg, gs)
        ws.append(ow), ss.append(osg), ps.append(par), cached.append(hg)
    assert cached == [1, 0, 1, 0, 1]
    got_parent, want_parent = np.concatenate(ps), ref.parent
    assert np.array_equal(got_parent, want_parent)
    _same_state(*state[1:], ref.state)
    worst_s, worst_w = G.compare(np.concatenate(ws), np.concatenate(ss), ref, ulps)
    assert worst_s <= SIGMA_ULP and worst_w <= WEIGHT_ABS, (worst_s, worst_w)
    assert len(ref.parent) == lam * calls


def test_cases_reach_their_branches():
    """Conditions on the inputs, from the reference alone."""
    cases = G.cases()
    assert len(cases) == (len(G.SHAPES) + 2) * len(G.ENTRIES)
    exits, entries = set(), set()
    for i, case in enumerate(cases):
        ref = G.reference(i)
        _, pos0, hg0, _ = G.abs_state(case.entry)
        entries.add((pos0 if pos0 in (0, 1, 623, 624) else "mid", hg0))
        exits.add(G.abs_state(ref.state)[2])
        if case.mu & (case.mu - 1):   # no power of two: the mask admits values above mu - 1
            if case.lam > 1:
                assert ref.parent_outputs > case.lam, (case.name, ref.parent_outputs)
            else:   # one child rejects with probability 28 / 128 at mu = 100: asked of its entry states together
                family = [j for j, c in enumerate(cases) if c.name.split("/")[0] == case.name.split("/")[0]]
                assert sum(G.reference(j).parent_outputs for j in family) > len(family), case.name
            if case.mu <= 10:
                assert set(ref.parent.tolist()) == set(range(case.mu)), case.name
        elif case.mu == 1:
            assert ref.parent_outputs == 0 and not ref.parent.any()
        else:
            assert ref.parent_outputs == case.lam
        if case.lam >= 40:   # a block refill inside the run (a freshly seeded stream refills at its first draw as well)
            assert ref.refills - (pos0 == 624) >= 1, (case.name, ref.refills)
        if case.name.startswith(("clamp", "nonfinite")):
            assert (ref.s == case.min_sigma).sum() >= 100, (case.name, int((ref.s == case.min_sigma).sum()))
            assert (ref.w == 0.0).any() and (ref.w == 1.0).any()
        if case.name.startswith("nonfinite"):
            assert np.isnan(ref.s).any() and np.isinf(ref.s).any() and np.isnan(ref.w).any()
        else:
            assert np.isfinite(ref.s).all() and np.isfinite(ref.w).all()
    assert exits == {0, 1}
    assert entries == {(624, 0), ("mid", 1), ("mid", 0), (623, 0), (1, 0), (0, 0)}
