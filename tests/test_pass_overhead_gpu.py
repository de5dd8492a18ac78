"""The glue around the rules core in a pass of the hot kernel's decision loop: the pass's actions are handed to the
candidate lanes from the scalar unit (monsoon_amd/csrc/pass_glue.h), and the pass's first maximum joins the running best.
Every (U, W) of the three builds plays the 64 games of tests/pass_overhead_trace.py and must stay on the recursive
oracle's line (run with -m gpu on an MI355X).

What can go wrong shows in which action a lane steps (the score row: every legal action scored once, at its own index),
in the first maximum (the action and the best score, ties within a pass and across passes included) and in what is
committed (the state hash).  The CPU side first makes sure that the games hold the cases that matter for each U."""
import numpy as np
import pytest

import kernel_variants
import pass_overhead_trace as T
from monsoon_amd.cards import deck_indices

VARIANTS, VARIANT_IDS = kernel_variants.matrix()
# the legal counts named for each U that seeds 0..63 hold exactly (the others fall back to the largest count below them)
EXACT = {4: (1, 3, 4, 5, 8, 9), 8: (1, 7, 8, 9, 16, 17), 16: (1, 15, 16, 17, 32, 33), 32: (1, 31, 32, 33, 64), 64: (1, 64)}


def _check_cases():
    """The oracle's own trace of the games: for every U of the matrix a decision with 1, U - 1, U, U + 1, 2U and 2U + 1 legal
    actions (or the largest count below, where the games hold none: nothing above 64 here), a maximal score shared within
    one pass, and one shared across two passes wherever a decision of these games has two passes of U."""
    for ext in (False, True, 2):
        t = T.trace(ext)
        counts = T.legal_counts(t)
        assert len(counts) == len(T.SEEDS) * T.DECISIONS   # no game ends within the 40 decisions
        have = set(int(c) for c in counts)
        for u in sorted({u for e, u, _ in VARIANTS if e == ext}):
            want = T.wanted_counts(u, counts)
            assert all(v is not None for v in want.values()), (u, want)
            assert all(want[c] == c for c in EXACT[u]), (u, want)
            assert all(v == max(have) for k, v in want.items() if k not in EXACT[u] and k > max(have)), (u, want)
            assert all(v in have for v in want.values())
            same, cross = T.ties(t, u)
            assert same > 0, u
            assert cross > 0 or max(have) <= u, (u, cross)
    assert all(u in EXACT for _, u, _ in VARIANTS)


def test_the_games_hold_every_case():
    """CPU: the fixture cannot silently lose a case (the GPU test asserts the same before it plays)."""
    _check_cases()


def _bits(x):
    return np.ascontiguousarray(x, dtype=np.float64).view(np.uint64)


def _engine(ext):
    from monsoon_amd.engine import BatchEngine
    n = len(T.SEEDS)
    deck = deck_indices("N12M")
    eng = BatchEngine(n, extended=ext)
    eng.reset(np.array(T.SEEDS, dtype=np.uint32), np.stack([deck, deck]))
    return eng


@pytest.mark.gpu
@pytest.mark.parametrize("ext,u,w", VARIANTS, ids=VARIANT_IDS)
def test_every_round_stays_on_the_oracle_line(monkeypatch, ext, u, w):
    """40 decision rounds with scores written: after every round the chosen action, the whole score row (NaN exactly at
    the actions that are not legal, bit patterns elsewhere), the best score and the state hash equal the oracle's.  Then
    the same games in five launches of play_rounds(8): the state hash after each equals the same line."""
    _check_cases()
    kernel_variants.select(monkeypatch, u, w)
    t = T.trace(ext)
    n = len(T.SEEDS)
    weights = np.broadcast_to(np.stack([T.W0, T.W1]), (n, 2, 10)).copy()
    eng = _engine(ext)
    assert eng.variant() == (u, w)
    for r in range(T.DECISIONS):
        action, best, scores = eng.decide(weights, want_scores=True)
        hashes = eng.state_hash()
        assert np.array_equal(action, t["action"][r]), (r, np.nonzero(action != t["action"][r])[0][:8])
        nan = np.isnan(t["scores"][r])
        assert np.array_equal(np.isnan(scores), nan), r
        assert np.array_equal(_bits(scores)[~nan], _bits(t["scores"][r])[~nan]), r
        live = t["live"][r]
        assert np.array_equal(_bits(best)[live], _bits(t["best"][r])[live]) and np.isnan(best[~live]).all(), r
        clean = t["clean"][r]
        assert np.array_equal(hashes[clean], t["hash"][r][clean]), (r, np.nonzero(hashes != t["hash"][r])[0][:8])
    st = eng.stats()
    assert st["capacity_faults"] == 0 and st["lookahead_capacity_faults"] == 0
    assert st["lookahead_steps"] == int(T.legal_counts(t).sum())
    eng.close()

    eng = _engine(ext)
    eng.upload_weights(np.stack([T.W0, T.W1]))
    eng.assign_players(np.zeros(n, dtype=np.int32), np.ones(n, dtype=np.int32))
    for k in range(T.DECISIONS // 8):
        eng.play_rounds(8)
        eng.sync()
        r = 8 * k + 7
        clean = t["clean"][r]
        assert np.array_equal(eng.state_hash()[clean], t["hash"][r][clean]), ("play_rounds", k)
    assert eng.stats()["lookahead_steps"] == int(T.legal_counts(t).sum())
    eng.close()
