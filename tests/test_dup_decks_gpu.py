"""Decks that list a card more than once on the device: the reference's own games on such decks
(tests/golden/trace_dup.npz, trace_heuristic_dup.npz, trace_vs_expert_dup.npz; conditions and CPU side in
tests/test_dup_decks_cpu.py) through the step interface, the decision and rollout kernels, the vector env and the replay
on the extended and the large record, and the standard build's refusal of a repeated unit / structure card."""
import os

import numpy as np
import pytest

try:
    # torch's own HIP runtime must be the first one the process loads (tests/test_deep_steps_gpu.py has the reason): in a
    # run of the whole suite it is; this keeps the vector-env tests below running when the file is run on its own
    import torch  # noqa: F401
except ImportError:
    pass

import kernel_variants
from monsoon_amd import EXPERT, MonsoonError, game_log
from monsoon_amd.cards import CARD_INDEX, deck_indices, needs_extended_each, repeats_card
from monsoon_amd.engine import BatchEngine
from monsoon_amd.fitness import MATCH_DTYPE
from test_gpu_parity import _fnv1a64_rows, _heuristic_selfplay

pytestmark = pytest.mark.gpu

GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
SLOTS = 64


def _gold(name):
    return np.load(os.path.join(GOLD, name + ".npz"))


def _spells_only(g):
    return g["klass"] == list(g["class_names"]).index("spells_only")


def _lockstep(eng, g, games, fillers):
    """The fixture's `games` spread over the slots of one batch, shallow filler games (N12M, PASS every step: other records in
    the same wavefronts) in between, through monsoon_step: legal mask, reward / done, state hash and observation of every
    step equal the fixture's; a game the reference ended by an exception stops there on the device too."""
    n = len(games) + fillers
    assert n <= SLOTS
    slot = np.arange(len(games)) * n // len(games)   # spread over the batch
    seeds = np.arange(n, dtype=np.uint32) + 777
    n12m = deck_indices("N12M")
    decks = np.tile(np.stack([n12m, n12m]), (n, 1, 1))
    seeds[slot] = g["seeds"][games]
    decks[slot, 0], decks[slot, 1] = g["deck0"][games], g["deck1"][games]
    eng.reset(seeds, decks)
    assert np.array_equal(eng.state_hash()[slot], g["init_hash"][games])
    off = g["offsets"]
    lens = (off[1:] - off[:-1])[games]
    compared = 0
    for t in range(int(lens.max())):
        live = np.nonzero(lens > t)[0]
        masks = eng.legal_mask()
        acts = np.full(n, 155, dtype=np.uint8)   # fillers pass; finished fixture games sit out
        acts[slot[lens <= t]] = 255
        for j in live:
            i = off[games[j]] + t
            assert np.array_equal(masks[slot[j]], g["legal"][i]), (games[j], t)
            acts[slot[j]] = g["action"][i]
        reward, done, fault = eng.step(acts)
        hashes = eng.state_hash()
        obs, raises = eng.observe()
        obs_hash = _fnv1a64_rows(obs.reshape(n, -1).view(np.uint8))
        for j in live:
            k, s, i = games[j], slot[j], off[games[j]] + t
            if g["fault"][k] and t == lens[j] - 1:
                assert fault[s] != 0 or raises[s], (k, t)
                continue
            assert fault[s] == 0 and hashes[s] == g["hash"][i], (k, t, fault[s])
            assert (reward[s], done[s]) == (g["reward"][i], g["done"][i]), (k, t)
            assert not raises[s] and obs_hash[s] == g["obs"][i], (k, t)
            compared += 1
    return compared


@pytest.mark.parametrize("build", [1, 2])
def test_step_interface_plays_repeated_decks_as_the_reference(build):
    g = _gold("trace_dup")
    n = len(g["seeds"])
    eng = BatchEngine(SLOTS, extended=build)
    compared = _lockstep(eng, g, np.arange(n), SLOTS - n)
    eng.close()
    assert compared == len(g["action"]) - int(g["fault"].sum())


def test_standard_build_plays_the_spells_only_games():
    g = _gold("trace_dup")
    games = np.nonzero(_spells_only(g))[0]
    eng = BatchEngine(SLOTS)
    compared = _lockstep(eng, g, games, 9)
    eng.close()
    assert len(games) >= 4 and compared == int(np.diff(g["offsets"])[games].sum() - g["fault"][games].sum())


def _matches(g, bot=False):
    n = len(g["seeds"])
    m = np.zeros(n, dtype=MATCH_DTYPE)
    m["seed"], m["deck"] = g["seeds"], np.arange(n)
    if bot:
        m["p1"] = np.where(g["bot_side"] == 1, 0, EXPERT)
        m["p2"] = np.where(g["bot_side"] == 1, EXPERT, 0)
    return m


VARIANTS = [(True, u, w) for u, w in kernel_variants.variants(True)] + [(2,) + kernel_variants.variants(2)[0]]


@pytest.mark.parametrize("ext,u,w", VARIANTS, ids=[f"{kernel_variants.BUILD_NAMES[e]}-{u}x{w}" for e, u, w in VARIANTS])
def test_decisions_and_logged_rollout_of_the_heuristic_games(monkeypatch, ext, u, w):
    """trace_heuristic_dup.npz on every hot-kernel variant of the extended build and the large build's default: one
    rollout_logged call pins action, best score (bit for bit) and legal count of every decision; monsoon_decide the
    score-vector hash and the committed state at every decision."""
    g = _gold("trace_heuristic_dup")
    kernel_variants.select(monkeypatch, u, w)
    eng = BatchEngine(32, extended=ext)
    try:
        assert eng.variant() == (u, w)
        _, results, steps, log = eng.rollout_logged(g["w0"][None], _matches(g), g["decks"], int(g["max_turns"]))
        lengths = np.diff(g["offsets"])
        assert np.array_equal(steps, lengths) and np.array_equal(log.steps, lengths) and np.array_equal(results, g["result"])
        assert not eng.rollout_faults(len(lengths)).any()
        for k in range(len(lengths)):
            lo, hi, ln = int(g["offsets"][k]), int(g["offsets"][k + 1]), int(lengths[k])
            assert np.array_equal(log.action[k, :ln], g["action"][lo:hi]), k
            assert np.array_equal(log.score[k, :ln].view(np.uint64), g["best"][lo:hi].view(np.uint64)), k
            assert np.array_equal(log.n_legal[k, :ln], g["nlegal"][lo:hi]), k
            assert (log.action[k, ln:] == 255).all() and np.isnan(log.score[k, ln:]).all() and not log.n_legal[k, ln:].any()
        _heuristic_selfplay(eng, g, "trace_heuristic_dup.npz")
    finally:
        eng.close()


def test_expert_games_through_both_rollouts():
    """trace_vs_expert_dup.npz, the bot on each side: rollout_vs_expert gives the reference's result, steps, fault and final
    state; the logged rollout every action of either side, a NaN score and a legal count of 0 exactly on the bot's steps."""
    g = _gold("trace_vs_expert_dup")
    n, m, T = len(g["seeds"]), _matches(g, bot=True), int(g["max_turns"])
    pairs = np.stack([g["deck0"], g["deck1"]], axis=1)
    ok = g["fault"] == 0
    eng = BatchEngine(SLOTS, extended=1)
    counts, results, steps = eng.rollout_vs_expert(g["w0"][None], m, pairs, T, want_results=True)
    assert np.array_equal(results, g["result"]) and np.array_equal(steps, g["steps"])
    assert np.array_equal(eng.rollout_faults(n) != 0, g["fault"] != 0) and np.array_equal(eng.state_hash()[ok], g["final"][ok])
    agent_wins = int((results == np.where(g["bot_side"] == 1, 0, 1)).sum())
    assert counts.tolist() == [[agent_wins, int((results == -1).sum()), n]]
    counts2, results2, steps2, log = eng.rollout_logged(g["w0"][None], m, pairs, T)
    assert np.array_equal(counts2, counts) and np.array_equal(results2, results) and np.array_equal(steps2, steps)
    assert np.array_equal(eng.state_hash()[ok], g["final"][ok])
    eng.close()
    for k in range(n):
        lo, hi, ln = int(g["offsets"][k]), int(g["offsets"][k + 1]), int(steps[k])
        bot = g["bot"][lo:hi] == 1
        assert hi - lo == ln and np.array_equal(log.action[k, :ln], g["action"][lo:hi]), k
        assert np.array_equal(np.isnan(log.score[k, :ln]), bot) and np.array_equal(log.n_legal[k, :ln] == 0, bot), k


def test_vec_env_afterstates_at_fixture_decisions():
    """A VecEnv(extended=1) on the fixture games' seeds and decks, stepped with the fixture's actions: at three decisions its
    afterstates() hold, for the action the fixture commits next, status 0 and the features of the fixture's next state
    (a nonzero status or a raising observation where the reference raised)."""
    import torch
    from monsoon_amd.vec_env import VecEnv
    g = _gold("trace_dup")
    n = len(g["seeds"])
    off = g["offsets"]
    lens = off[1:] - off[:-1]
    foff = np.concatenate([[0], np.cumsum(lens - g["fault"].astype(np.int64))])
    env = VecEnv(n, extended=1)
    env.reset(g["seeds"], np.stack([g["deck0"], g["deck1"]], axis=1))   # no opponent: the caller plays both sides
    checked = 0
    for t in range(9):
        live = np.nonzero(lens > t)[0]
        if t in (0, 4, 8):
            after = env.afterstates(obs=False)
            action, status, feat = (after[k].cpu().numpy() for k in ("action", "status", "features"))
            for k in live:
                a = int(g["action"][off[k] + t])
                j = np.nonzero(action[k] == a)[0]
                assert len(j) == 1, (k, t)
                if g["fault"][k] and t == lens[k] - 1:
                    assert status[k, j[0]] != 0, (k, t)
                    continue
                assert status[k, j[0]] == 0, (k, t)
                assert np.array_equal(feat[k, j[0]].view(np.uint64), g["feat"][foff[k] + t].view(np.uint64)), (k, t)
                checked += 1
        acts = np.full(n, 155, dtype=np.uint8)   # a game past its trace passes
        acts[live] = g["action"][off[live] + t]
        env.step(torch.from_numpy(acts).cuda())
    env.close()
    assert checked >= 2.5 * n


def test_dataset_replays_a_logged_repeated_deck_game_to_its_final_hash():
    g = _gold("trace_heuristic_dup")
    k = int(np.argmax(g["cov_shared"]))
    m = _matches(g)[k:k + 1].copy()
    m["deck"] = 0
    pairs = g["decks"][k][None]
    eng = BatchEngine(SLOTS, extended=1)
    _, results, steps, log = eng.rollout_logged(g["w0"][None], m, pairs, int(g["max_turns"]))
    final = eng.state_hash()[0]
    lo, hi = int(g["offsets"][k]), int(g["offsets"][k + 1])
    assert final == g["hash"][hi - 1] and steps[0] == hi - lo
    d = game_log.dataset(eng, m, pairs, log, columns=("legal", "state_hash", "step"))
    assert not d["status"].any() and d["replayed"].tolist() == [hi - lo] and eng.state_hash()[0] == final
    rows = d["state_hash"].cpu().numpy().view(np.uint64)
    assert np.array_equal(rows[1:], g["hash"][lo:hi - 1]) and np.array_equal(d["action"].cpu().numpy(), g["action"][lo:hi])
    eng.close()


def test_standard_build_refuses_a_repeated_unit_or_structure_card():
    """monsoon_reset, monsoon_rollout / _vs_expert / _logged and monsoon_env_reset with explicit decks: MONSOON_ERR_ARG with a
    message naming the card and extended=1; loaded games stay untouched and the handle usable.  The spells-only pair is
    accepted."""
    from monsoon_amd.vec_env import VecEnv
    g = _gold("trace_dup")
    spells = _spells_only(g)
    plain = ~np.isin(np.stack([g["deck0"], g["deck1"]], axis=1), [CARD_INDEX["ua20"], CARD_INDEX["b005"]]).any(axis=(1, 2))
    k = int(np.nonzero(~spells & plain)[0][0])
    bad = np.stack([g["deck0"][k], g["deck1"][k]])
    assert repeats_card(bad).all()
    n12m = deck_indices("N12M")
    good = np.stack([n12m, n12m])
    only_second = np.stack([n12m, bad[1]])
    ks = int(np.nonzero(spells)[0][0])
    spell_pair = np.stack([g["deck0"][ks], g["deck1"][ks]])
    assert not needs_extended_each(spell_pair[None])[0] and len(set(spell_pair[0].tolist())) < 12
    eng = BatchEngine(SLOTS)
    seeds = np.arange(5, dtype=np.uint32)
    eng.reset(seeds, good)
    eng.step(np.full(5, 155, dtype=np.uint8))
    before = eng.state_hash().copy()
    m = np.zeros(3, dtype=MATCH_DTYPE)
    m["seed"] = np.arange(3)
    mb = m.copy()
    mb["p2"] = EXPERT
    w = np.zeros((1, 10))
    for pair in (bad, only_second):
        table = np.stack([good, pair])   # the repeat sits in a pair no match names: the table is refused all the same
        for call in (lambda: eng.reset(seeds, np.stack([good, good, pair, good, good])),
                     lambda: eng.rollout(w, m, table, 5),
                     lambda: eng.rollout_vs_expert(w, mb, table, 5),
                     lambda: eng.rollout_logged(w, m, table, 5)):
            with pytest.raises(MonsoonError, match=r"more than once.*extended=1") as err:
                call()
            assert "status 1" in str(err.value)
            assert eng.n == 5 and np.array_equal(eng.state_hash(), before)   # nothing was loaded or launched
    counts = eng.rollout(w, m, np.stack([good, spell_pair]), 5)   # usable, and a repeated spell is no repeat
    assert counts[0, 2] == 3
    eng.close()
    env = VecEnv(4)
    env.reset(np.arange(4, dtype=np.uint32), good)
    h0 = env.state_hash().copy()
    with pytest.raises(MonsoonError, match=r"more than once.*extended=1"):
        env.reset(np.arange(4, dtype=np.uint32), np.stack([good, good, bad, good]))
    env.reset(np.arange(4, dtype=np.uint32), good)
    assert np.array_equal(env.state_hash(), h0)
    env.reset(np.arange(4, dtype=np.uint32), spell_pair)
    env.close()


def test_standard_env_refuses_an_explore_generation_that_can_repeat_a_card():
    """VecEnv.reset(deck_schedule=) and set_deck_schedule on the standard record: an explore generation that keeps some but
    not all of the archetype is refused with a message naming extended=1 -- its pools hold neither ua20 nor b005, the
    draw itself can repeat a card -- and the running env goes on; exploit, balance, keep-all and keep-none are accepted."""
    import torch
    from monsoon_amd.vec_env import VecEnv
    from vec_env_schedule_model import FACTIONS, standard_schedule
    n = 4
    seed0 = np.arange(n, dtype=np.uint32) + 50
    facs = np.tile(np.array(FACTIONS, dtype=np.uint8), (n, 1))
    env = VecEnv(n)
    for params in (standard_schedule(1, n_preserve=1), standard_schedule(1, n_preserve=11)):
        with pytest.raises(MonsoonError, match=r"explore generation.*extended=1"):
            env.reset(seed0, factions=facs, deck_schedule=params)
    for params in (standard_schedule(0), standard_schedule(2, ratio=0.5), standard_schedule(1, n_preserve=12), standard_schedule(1, n_preserve=0)):
        env.reset(seed0, factions=facs, deck_schedule=params)
        assert not repeats_card(env.decks().cpu().numpy().reshape(-1, 12)).any()
    with pytest.raises(MonsoonError, match=r"explore generation.*extended=1"):
        env.set_deck_schedule(7, standard_schedule(1, n_preserve=6, generation=7))
    views = env.step(torch.full((n,), 155, dtype=torch.uint8, device="cuda"))   # the refused schedule changed nothing
    assert not bool(views["illegal"].any().item())
    doubled = standard_schedule(2, ratio=0.5)
    doubled["pool"][0, 1] = doubled["pool"][0, 0]   # a pool that lists a unit / structure twice can draw it twice
    with pytest.raises(MonsoonError, match=r"pool.*more than once"):
        env.engine.env_set_schedule(doubled)
    env.close()
    ext = VecEnv(n, extended=1)
    ext.reset(seed0, factions=facs, deck_schedule=standard_schedule(1, n_preserve=6))
    ext.close()


def test_schedule_games_end_to_end_on_their_tiers():
    """FitnessEvaluator on the per-game schedule of the GA configuration at generation 5 (explore), 4 individuals and 64
    games: the pairs that repeat a unit / structure card start on tier 1, and the fitness is the CPU path's."""
    from oracle_rollout import oracle_rollout_fn
    from monsoon_amd.cards import DECKS
    from monsoon_amd.config import EvolutionaryConfig
    from monsoon_amd.decks import DeckEvolutionConfig
    from monsoon_amd.fitness import FitnessEvaluator
    from monsoon_amd.weights import WeightVector
    np.random.seed(17)
    pop = [WeightVector(10) for _ in range(4)]
    cfg = EvolutionaryConfig(mu=4, lambda_=4, schedule="ring", games_per_individual=16, max_turns=40, max_concurrent_games=64)
    seen = []

    def cpu(weights, matches, deck_pairs, max_turns):
        seen.append(np.array(deck_pairs))
        return oracle_rollout_fn(weights, matches, deck_pairs, max_turns)

    def dc():
        return DeckEvolutionConfig(DECKS["IRONCLAD"], DECKS["SWARM"], exploit_generations=2, explore_generations=6, seed=123, per_game=True)
    f_cpu = FitnessEvaluator(cfg, dc(), rollout_fn=cpu).evaluate_population(pop, generation=5)
    ev = FitnessEvaluator(cfg, dc())
    f_hip = ev.evaluate_population(pop, generation=5)
    pairs = seen[0]
    need = needs_extended_each(pairs)
    repeated = repeats_card(pairs.reshape(-1, 12)).reshape(-1, 2).any(axis=1)
    assert len(pairs) == 64 and repeated.sum() >= 8 and (need & ~repeated).sum() + (~need).sum() > 0
    assert ev.tier_games == [int((~need).sum()), int(need.sum())] and ev.tier_games[1] >= int(repeated.sum())
    assert f_hip == f_cpu
