"""The logged rollouts asked for only some of their log's columns (csrc/host_layout.h LOG_COLUMN), which the Python wrapper
never does: monsoon_rollout_sample, monsoon_rollout_explore and monsoon_rollout_logged through ctypes with NULL for the
absent arrays.  17 N12M matches of max_turns 201 on a handle of 7 games: batches of 7 + 7 + 3, and 7 x 201 = 1 407 entries
per full batch, an odd count, so a device log whose columns were not laid out by falling element size would misalign one.
Every array a call asks for equals that array of the entry point's all-columns call bit for bit, padding included, and so
do counts, results, steps, fault codes and the last batch's state hashes; the all-columns sampling log is the model's over
the CPU oracle (tests/sample_model.py).  Every call is a valid one."""
import ctypes

import numpy as np
import pytest

import sample_model as S
from monsoon_amd import EXPERT, _lib
from monsoon_amd.cards import deck_indices
from monsoon_amd.engine import BatchEngine, Explore, RolloutLog, _ptr
from monsoon_amd.fitness import MATCH_DTYPE, hash32_array

pytestmark = pytest.mark.gpu

N, T, CAP = 17, 201, 7
W2 = np.stack([np.random.RandomState(2024).uniform(0, 1, 10), np.random.RandomState(7).uniform(0, 1, 10)])
RULE = Explore(0.5, 9, temperature=1.0)
# name, dtype, the value behind a game's last step (include/monsoon.h), in the order of the three structs of host pointers
COLUMNS = (("action", np.uint8, 255), ("score", np.float64, np.nan), ("n_legal", np.int16, 0),
           ("greedy", np.uint8, 255), ("explored", np.uint8, 0), ("taken_score", np.float64, np.nan),
           ("weight_total", np.uint32, 0), ("taken_weight", np.uint32, 0))
OPTIONAL = tuple(c[0] for c in COLUMNS[1:])
ENTRY_COLUMNS = {"monsoon_rollout_logged": OPTIONAL[:2], "monsoon_rollout_explore": OPTIONAL[:5], "monsoon_rollout_sample": OPTIONAL}


def _matches():
    """A third each of bot-FIRST, bot-SECOND and plain, over the two rows of W2."""
    m = np.zeros(N, dtype=MATCH_DTYPE)
    k = np.arange(N)
    row, third = k % 2, k % 3
    m["seed"] = hash32_array(5, k, 0xC)
    m["p1"] = np.where(third == 0, EXPERT, row)
    m["p2"] = np.where(third == 1, EXPERT, np.where(third == 0, row, 1 - row))
    return m


def _pairs():
    d = deck_indices("N12M")
    return np.ascontiguousarray(np.stack([d, d])[None])


def _masks(optional):
    """All columns, none, each optional column alone, each alone absent."""
    masks = [frozenset(optional), frozenset()] + [frozenset([c]) for c in optional] + [frozenset(optional) - {c} for c in optional]
    return list(dict.fromkeys(masks))   # (two optional columns: alone and alone-absent coincide)


def _call(eng, entry, asked):
    """One call of `entry` with the columns `asked` (action always) and NULL for every other array.  Arrays are filled with
    a value no column pads with beforehand, so whatever the call leaves unwritten shows."""
    log = {name: np.full((N, T), 0x5A, dtype=dtype) for name, dtype, _ in COLUMNS if name == "action" or name in asked}
    ptr = lambda name: _ptr(log.get(name))   # noqa: E731
    counts, results, steps = np.zeros((2, 3), dtype=np.int32), np.zeros(N, dtype=np.int8), np.zeros(N, dtype=np.int32)
    extra = [ctypes.byref(_lib.RolloutLog(ptr("action"), ptr("score"), ptr("n_legal")))]
    if entry != "monsoon_rollout_logged":
        rule = RULE.c_sample() if entry == "monsoon_rollout_sample" else RULE.c_struct()
        extra += [ctypes.byref(rule), ctypes.byref(_lib.ExploreLog(ptr("greedy"), ptr("explored"), ptr("taken_score")))]
    if entry == "monsoon_rollout_sample":
        extra += [ctypes.byref(_lib.SampleLog(ptr("weight_total"), ptr("taken_weight")))]
    m, pairs = _matches(), _pairs()
    rc = getattr(eng.lib, entry)(eng.h, _ptr(np.ascontiguousarray(W2)), 2, _ptr(m), N, _ptr(pairs), 1, T, _ptr(counts), _ptr(results),
                                 _ptr(steps), *extra)
    assert rc == _lib.OK, (entry, sorted(asked), rc)
    eng.n = N - (N - 1) // CAP * CAP   # the handle holds the last batch: 3 games
    assert eng.n == 3
    return dict(log=log, counts=counts, results=results, steps=steps, faults=eng.rollout_faults(N), hashes=eng.state_hash())


def _bits(a):
    return a.view(np.uint64) if a.dtype == np.float64 else a


@pytest.fixture(scope="module")
def engine():
    import torch   # (torch loads its runtime before the library does, as in the other logged-rollout tests)
    assert torch.cuda.is_available()
    eng = BatchEngine(CAP)
    yield eng
    eng.close()


@pytest.fixture(scope="module")
def full(engine):
    """The all-columns call of every entry point: computed once, read by every test, never written."""
    return {entry: _call(engine, entry, frozenset(cols)) for entry, cols in ENTRY_COLUMNS.items()}


@pytest.mark.parametrize("entry", list(ENTRY_COLUMNS))
def test_a_call_with_some_columns_writes_what_the_all_columns_call_writes(engine, full, entry):
    ref = full[entry]
    masks = _masks(ENTRY_COLUMNS[entry])
    assert len(masks) == {"monsoon_rollout_logged": 4, "monsoon_rollout_explore": 12, "monsoon_rollout_sample": 16}[entry]
    for asked in masks[1:]:
        got = _call(engine, entry, asked)
        assert set(got["log"]) == {"action"} | asked
        for name, a in got["log"].items():
            assert np.array_equal(_bits(a), _bits(ref["log"][name])), (entry, sorted(asked), name)
        for key in ("counts", "results", "steps", "faults", "hashes"):
            assert np.array_equal(got[key], ref[key]), (entry, sorted(asked), key)


def test_all_columns_calls_pad_behind_the_last_step(full):
    """The padding is what include/monsoon.h promises, in every array of every entry point; the games cross the batch
    boundaries (every batch holds decisions that sampled)."""
    for entry, ref in full.items():
        behind = np.arange(T)[None, :] >= ref["steps"][:, None]
        assert (ref["steps"] > 0).all() and behind.any(), entry
        for name, _, pad in COLUMNS:
            if name in ref["log"]:
                a = ref["log"][name][behind]
                assert np.isnan(a).all() if pad != pad else (a == pad).all(), (entry, name)
    sampled = full["monsoon_rollout_sample"]["log"]["explored"] != 0
    assert all(sampled[a:b].any() for a, b in ((0, 7), (7, 14), (14, 17)))


def test_all_columns_sampling_log_equals_the_model_over_the_cpu_oracle(full):
    dev = full["monsoon_rollout_sample"]
    model = S.ModelEngine(0)
    counts, results, steps, log = model.rollout_logged(W2, _matches(), _pairs(), T, explore=RULE)
    assert np.array_equal(dev["counts"], counts) and np.array_equal(dev["results"], results) and np.array_equal(dev["steps"], steps)
    assert np.array_equal(dev["faults"], model.rollout_faults(N))
    for name in ("action", "n_legal", "greedy", "explored", "weight_total", "taken_weight"):
        assert np.array_equal(dev["log"][name], getattr(log, name)), name
    assert S.same_log(RolloutLog(steps=dev["steps"], **dev["log"]), log)   # (score and taken_score bit for bit among them)
    ok = model.faults[14:] == 0   # (behind a faulting step the kernel and the oracle stop at different points)
    assert np.array_equal(dev["hashes"][ok], model.finals[14:][ok])
