"""Target scans inside a look-ahead step that read only the tiles their caller keeps (monsoon_amd/csrc/rules.h
get_targets, shape_targets, shape_any, targets_any, target_has), in whole games on the device: every standard hot-kernel variant and the default variant of the extended and the large build play
64 games x 40 decisions on N12M and on a deck made only of cards whose ability code scans for targets
(tests/target_scan_trace.py), and every decision's action, score vector and canonical hash must equal the recursive
oracle's line (run with -m gpu on an MI355X).  The forms themselves against the full-board text, input by input:
tests/test_target_scan_cpu.py."""
import numpy as np
import pytest

import kernel_variants
import target_scan_trace as T

CASES = [(False, u, w) for u, w in kernel_variants.variants(False)] + [(True,) + kernel_variants.variants(True)[0], (2,) + kernel_variants.variants(2)[0]]
IDS = [f"{kernel_variants.BUILD_NAMES[e]}-{u}x{w}" for e, u, w in CASES]


def test_the_games_reach_every_converted_call_site():
    """CPU: the oracle's states say which scans the legal actions' steps begin with (the GPU test asserts the same first)."""
    for ext in (False, True, 2):
        T.check_reached(ext)


def _bits(x):
    return np.ascontiguousarray(x, dtype=np.float64).view(np.uint64)


@pytest.mark.gpu
@pytest.mark.parametrize("ext,u,w", CASES, ids=IDS)
def test_every_decision_stays_on_the_oracle_line(monkeypatch, ext, u, w):
    from monsoon_amd.engine import BatchEngine
    T.check_reached(ext)
    kernel_variants.select(monkeypatch, u, w)
    n = len(T.SEEDS)
    weights = np.broadcast_to(np.stack([T.W0, T.W1]), (n, 2, 10)).copy()
    for deck_name in ("N12M", "touched"):
        t = T.trace(deck_name, ext)
        deck = T.deck(deck_name, ext)
        eng = BatchEngine(n, extended=ext)
        eng.reset(np.array(T.SEEDS, dtype=np.uint32), np.stack([deck, deck]))
        assert eng.variant() == (u, w)
        for r in range(T.DECISIONS):
            action, _, scores = eng.decide(weights, want_scores=True)
            hashes = eng.state_hash()
            assert np.array_equal(action, t["action"][r]), (deck_name, r, np.nonzero(action != t["action"][r])[0][:8])
            nan = np.isnan(t["scores"][r])
            assert np.array_equal(np.isnan(scores), nan), (deck_name, r)
            assert np.array_equal(_bits(scores)[~nan], _bits(t["scores"][r])[~nan]), (deck_name, r)
            clean = t["clean"][r]
            assert np.array_equal(hashes[clean], t["hash"][r][clean]), (deck_name, r, np.nonzero(hashes != t["hash"][r])[0][:8])
        st = eng.stats()
        assert st["capacity_faults"] == 0 and st["lookahead_capacity_faults"] == 0, (deck_name, st)
        assert st["lookahead_steps"] == int(T.legal_counts(t).sum()), deck_name
        eng.close()
