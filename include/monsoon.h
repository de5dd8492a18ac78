/* monsoon.h -- C ABI of the MI355X batched Stormbound engine (libmonsoon_hip.so).
 *
 * Drop-in boundary for ONE path of dvrp0/Monsoon: the game step / legal-action / observation
 * surface and the heuristic self-play rollouts that score an evolutionary population.  The
 * reference has no FFI (it is pure Python); each entry point below names the Python interface
 * it replaces.  INTEGRATION.md shows the ctypes stubs a maintainer of the reference would add.
 *
 * Conventions: plain C, opaque handle, int status returns (0 = MONSOON_OK), caller-owned HOST
 * buffers unless a name ends in _dev, no callbacks, no global state.  One handle = one HIP
 * device + one stream; a handle is not thread-safe, independent handles are.  Per-game faults
 * (the reference's swallowed Python exceptions) are reported as bytes, never as
 * error returns.  There is no CPU backend: every call fails with MONSOON_ERR_DEVICE when no
 * gfx950 device is usable.
 */
#ifndef MONSOON_H
#define MONSOON_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define MONSOON_OK 0
#define MONSOON_ERR_ARG 1       /* bad argument (null pointer, size, illegal action, unsupported card or deck) */
/* What the standard build (libmonsoon_hip.so) refuses in every deck it is handed -- monsoon_reset, monsoon_rollout*,
 * monsoon_replay*, monsoon_env_reset, monsoon_env_set_schedule's archetypes: the cards ua20 and b005, and a 12-card deck
 * that lists a unit or structure card more than once (spells and up01 / up02 / up03 may repeat; a card in both players'
 * decks is no repeat).  The reference's list.remove takes the first EQUAL card, so with such a deck the drawn object
 * stays in the deck while it sits in the hand; only the extended record (libmonsoon_hip_ext.so, same ABI) plays that as
 * the reference does.  The check runs before anything is loaded or launched; monsoon_last_error names the card. */
#define MONSOON_ERR_DEVICE 2    /* HIP error; see monsoon_last_error */
#define MONSOON_ERR_STATE 3     /* call order (e.g. step before reset) */

#define MONSOON_NUM_ACTIONS 156 /* enums.py:10-36 */
#define MONSOON_OBS_INTS 540    /* (27,5,4) int32, games/stormbound.py:376-399 */
#define MONSOON_DECK_SIZE 12
#define MONSOON_NUM_FEATURES 10 /* evo/features.py:327-342 */

typedef struct monsoon monsoon_t;

typedef struct {
  int32_t device;          /* HIP device ordinal */
  int32_t max_games;       /* capacity of the batch */
  int32_t lanes_per_game;  /* candidate lanes (successor states stepped at once) per game: 4, 8, 16, 32 or 64; 0 = default.
                              Must be a kernel variant of the build (monsoon_amd/csrc/variants.def), else create fails.
                              (Development knobs read at create: MONSOON_LANES, MONSOON_WPE = waves per SIMD.) */
  int32_t stack_bytes;     /* ignored since the rules core keeps an explicit work stack (kept for ABI compatibility) */
} monsoon_config;

/* One scheduled game of a fitness evaluation (evo/fitness.py:53-59,133-157). */
typedef struct {
  int32_t p1;     /* index into the weight table: row individual, plays FIRST */
  int32_t p2;     /* opponent, plays SECOND */
  uint32_t seed;  /* numpy.random.RandomState(seed) of the game (games/stormbound.py:294) */
  uint32_t deck;  /* index into the deck-pair table passed to monsoon_rollout */
} monsoon_match;

typedef struct {
  uint64_t lookahead_steps;  /* Stormbound.step transitions executed as 1-ply look-ahead */
  uint64_t decisions;        /* committed decisions (each commits one of its look-ahead results) */
  uint64_t games_finished;   /* games that ended with a winner */
  uint64_t faults;           /* games stopped by a fault (reference: swallowed exception -> draw) */
  uint64_t capacity_faults;  /* of those, build-limit faults (must be 0 for a valid run) */
  uint64_t lookahead_capacity_faults;  /* games in which a LOOK-AHEAD hit a build limit: that action scored 0.0 where the
                                          reference computes a score (must be 0 for a valid run) */
} monsoon_stats;

int monsoon_create(const monsoon_config* cfg, monsoon_t** out);
void monsoon_destroy(monsoon_t* h);
const char* monsoon_last_error(monsoon_t* h);   /* h may be NULL: last create() error */
/* bits 0-15: the ABI generation (3); bits 16 / 17: the record build (extended / large extended); bits 24-31: the
 * generation's revision, raised when calls are added (1: monsoon_env_save_dev / monsoon_env_load_dev) */
int monsoon_version(void);
/* the hot-kernel variant the handle runs (any pointer may be NULL) */
int monsoon_variant(monsoon_t* h, int32_t* lanes_per_game, int32_t* waves_per_simd);
/* card id string ("u007") -> table index used in deck arrays; -1 if unknown.  card.py:15 */
int monsoon_card_index(const char* card_id);
/* 1 if the card's ability is implemented by this build (decks with other cards are refused) */
int monsoon_card_supported(int card_index);

/* Stormbound.__init__ for n games (games/stormbound.py:293-304, player.py:13-37):
 * seeds[n]; decks[n][2][12] card indices in constructor order; factions[n][2] (enums.py:44-49). */
int monsoon_reset(monsoon_t* h, int32_t n, const uint32_t* seeds, const uint8_t* decks, const uint8_t* factions);

/* Stormbound.legal_actions (games/stormbound.py:528-557) as a 156-bit mask per game: out[n][3]. */
int monsoon_legal_mask(monsoon_t* h, uint64_t* out);

/* Stormbound.step (games/stormbound.py:318-373) for every game; actions[n] must be legal
 * (PASS = 155 is always accepted, as the reference's scripted bot relies on; actions[i] = 255 leaves game i untouched).
 * An illegal entry refuses the whole call (MONSOON_ERR_ARG) before any game is stepped.  reward[n] in {0,1}, done[n], fault[n] (0 = none). */
int monsoon_step(monsoon_t* h, const uint8_t* actions, int8_t* reward, uint8_t* done, uint8_t* fault);

/* Stormbound.expert_action (games/stormbound.py:563-637), the reference's scripted opponent, for every game:
 * out_action[n] (may be PASS while plays remain -- that is how the bot ends a turn); fault[n] (may be NULL)
 * is non-zero where the reference would raise.  Draws from the game's own stream, like the reference. */
int monsoon_expert_action(monsoon_t* h, uint8_t* out_action, uint8_t* fault);

/* Stormbound.get_observation (games/stormbound.py:400-526): out[n][27][5][4] int32.
 * raises[n] = 1 where the reference would raise (int(card) on up01/up02/up03, card.py:46). */
int monsoon_observe(monsoon_t* h, int32_t* out, uint8_t* raises);

/* The same into caller-owned DEVICE memory (a torch-ROCm tensor view (B,27,5,4) int32
 * without a host round trip): out_dev = n*540 int32, raises_dev = n bytes or NULL.  Returns after the
 * handle's stream has finished writing. */
int monsoon_observe_dev(monsoon_t* h, void* out_dev, void* raises_dev);

/* StateFeatures.get_feature_vector (evo/features.py:12-342): out[n][10] float64. */
int monsoon_features(monsoon_t* h, double* out);

/* Stormbound.to_play / have_winner (games/stormbound.py:312-313, 560-561) + bases: out[n][4] =
 * {to_play, have_winner, base_first, base_second}. */
int monsoon_status(monsoon_t* h, int32_t* out);

/* The fault code that stopped each loaded game, else the first build-limit code one of its look-aheads hit (0 = none): out[n].  The reference's exceptions are swallowed by
 * its agent layer (evo/heuristic_agent.py:48-51, evo/fitness.py:170-174,208-210); codes in msb_base.h, >= 16 are
 * limits of this build -- except 18, the recursion guard (40 nested abilities / moves: the reference's own recursion ends in
 * RecursionError there, on every record alike).  29 is the work stack's word budget running out before that guard trips: a
 * limit of this build that no record changes; no game of the searches behind tests/golden/deep_steps.json.gz reports it. */
int monsoon_game_faults(monsoon_t* h, uint8_t* out);

/* Canonical state record of game idx (layout: monsoon_amd/csrc/canon.h), the comparand of the
 * bit-exactness tests.  buf must hold 2048 bytes (the standard and the extended record never need more than 1024). */
int monsoon_state_export(monsoon_t* h, int32_t idx, uint8_t* buf, int32_t* len);

/* copy.deepcopy(game) across the boundary (evo/game_adapter.py:280-287 clone_state): the COMPLETE device state of game
 * idx -- record, bookkeeping row, numpy stream position -- as an opaque blob of monsoon_state_blob_bytes() bytes.
 * monsoon_state_load puts a blob into slot idx of any handle of the same build (idx <= number of loaded games; idx ==
 * that number appends a game, max_games permitting): the clone then continues bit-identically to the original. */
int32_t monsoon_state_blob_bytes(void);
int monsoon_state_save(monsoon_t* h, int32_t idx, uint8_t* buf, int32_t buf_bytes);
int monsoon_state_load(monsoon_t* h, int32_t idx, const uint8_t* buf, int32_t buf_bytes);

/* Diagnostics behind the scenario tests (the reference's own unit tests, test.py:11-147 and the <ID>Test classes, replayed
 * call by call: tests/scenario_lib.py).  monsoon_debug_build puts game idx (idx <= loaded games) into a described
 * state: an int32 stream (layout: monsoon_amd/csrc/scenario.inc) and the position of its numpy stream,
 * RandomState(seed) advanced by stream_pos outputs.  monsoon_debug_op makes ONE call into the engine on that game
 * (Unit.play, activate_ability, deal_damage, destroy, command, respawn, Board.spawn_token_*, to_next_turn,
 * Player.play / discard): *fault = the fault code, log = {card, position} of every ability that ran, in order. */
int monsoon_debug_build(monsoon_t* h, int32_t idx, uint32_t seed, uint32_t stream_pos, const int32_t* state, int32_t n_state, int32_t* fault);
int monsoon_debug_op(monsoon_t* h, int32_t idx, const int32_t* op, int32_t n_op, int32_t* fault, int32_t* log, int32_t log_cap, int32_t* n_log);

/* Diagnostics: the device's numpy-stream draws and score arithmetic on caller-given inputs (numpy.random.RandomState
 * legacy API: player.py:28,49, unit.py:95, cards; np.dot of evo/weights.py:60), for known-answer tests.  kind 0: n raw
 * u32 outputs of RandomState(seed); 1: n random(); 2: randint(0, in[i]) for n int32 bounds; 3: n times
 * shuffle(list(range(12))) (out int32[n][12]); 4: n scores of in = double[n][30] {weights, before, after}.  n <= 4096.
 * Re-seeds the stream buffers of game slot 0. */
int monsoon_debug_kat(monsoon_t* h, int32_t kind, uint32_t seed, int32_t n, const void* in, void* out);

/* Known-answer entry of the sampler of monsoon_rollout_sample (below), no game involved: row i is a decision with the
 * legal list of ranks 0 .. n_legal[i] - 1 (1 .. 156), scores[i][j] the j-th action's score (double[m][156], entries behind
 * n_legal[i] are not read), best[i], inv_temperature[i] and draw1[i].  Per row: out_rank[i] = j* (-1 where total == 0),
 * out_total[i] = the sum of the weights, out_weight[i] = w_{j*} (0 where total == 0).  Computed by the device function the
 * rollout kernel calls, one wavefront per row.  1 <= m <= 65536; MONSOON_ERR_ARG for a null pointer, an m or an n_legal
 * out of range.  The values of best and inv_temperature are not checked: this entry is how their corner cases are put to
 * the device. */
int monsoon_debug_sample_kat(monsoon_t* h, int32_t m, const double* scores, const int32_t* n_legal, const double* best,
                             const double* inv_temperature, const uint32_t* draw1, int32_t* out_rank, uint32_t* out_total,
                             uint32_t* out_weight);

/* Debugging aid: the raw HBM record of game idx (monsoon_amd/csrc/state.h layout); buf must hold 4096 bytes. */
int monsoon_debug_raw(monsoon_t* h, int32_t idx, uint8_t* buf, int32_t* len);

/* FNV-1a 64 of the canonical record of every game: out[n].  Lets a caller compare a whole batch
 * against a replay without exporting 65 536 records one by one. */
int monsoon_state_hash(monsoon_t* h, uint64_t* out);

/* HeuristicAgent.select_action + adapter.apply_action for every live game
 * (evo/heuristic_agent.py:53-80, evo/game_adapter.py:320-325): 1-ply look-ahead over all legal
 * actions, score, first-max argmax, commit.  weights[n][2][10]: the weight vector of the FIRST
 * and SECOND player of each game.  out_action[n] (255 = game already over), out_score[n]
 * (best score), out_scores[n][156] (NaN = illegal; may be NULL). */
int monsoon_decide(monsoon_t* h, const double* weights, uint8_t* out_action, double* out_score, double* out_scores);

/* FitnessEvaluator rollouts (evo/fitness.py:123-228 with the corrected loop of SURVEY.md §8c):
 * plays n_matches games to the end (winner, fault, or max_turns decisions), at most
 * cfg.max_games at a time.  weights[n_individuals][10]; deck_pairs[n_decks][2][12];
 * out_counts[n_individuals][3] = {wins, draws, games} of each individual as p1, ACCUMULATED
 * into the caller's buffer; out_results[n_matches] (may be NULL): -1 draw, 0 p1, 1 p2;
 * out_steps[n_matches] (may be NULL): decisions played. */
int monsoon_rollout(monsoon_t* h, const double* weights, int32_t n_individuals, const monsoon_match* matches,
                    int32_t n_matches, const uint8_t* deck_pairs, int32_t n_decks, int32_t max_turns,
                    int32_t* out_counts, int8_t* out_results, int32_t* out_steps);
/* Fault code of every game of the last completed monsoon_rollout, out[n_matches] (same meaning as monsoon_game_faults:
 * the fault that stopped the game, else the first capacity code one of its look-aheads hit).  Codes >= 16 are limits
 * of this build's record, not reference behaviour (the exception the reference swallows at evo/fitness.py:170-174,
 * 208-210 is code 1): such games are replayed on a build with a larger record -- libmonsoon_hip_ext.so ->
 * libmonsoon_hip_big.so, as monsoon_amd/fitness.py does -- and their rows of the result replaced.  18 (the recursion guard: the
 * reference raises RecursionError at that step) is not replayed; 29 (the work stack's word budget) is, and stays. */
int monsoon_rollout_faults(monsoon_t* h, uint8_t* out, int32_t n_matches);

/* The evolved agent against the reference's scripted bot (play_vs_expert.py: HeuristicAgent.select_action on one side,
 * Stormbound.expert_action on the other; evo/EVOLUTIONARY_PLAN.md's yardstick).  monsoon_rollout's arguments and rollout
 * contract, with one more kind of player: p1, p2 or both of a match may be MONSOON_PLAYER_EXPERT.
 *
 *   steps = 0
 *   while not have_winner() and steps < max_turns:
 *       side = to_play()
 *       if side is the bot:  a = expert_action()        -- draws from the game's own stream, like the reference
 *       else:                a = HeuristicAgent(weights[row]).select_action()   -- exactly monsoon_decide's decision
 *       state = step(a); steps += 1
 *
 *  - The result follows the one rule of monsoon_rollout (FIRST wins iff SECOND's base < 0 <= FIRST's base, ...), not
 *    play_vs_expert.py's "<= 0" test: have_winner is strict.
 *  - An expert_action that raises (random.choice([]) inside the bot) ends the game as a draw with that fault code and
 *    without a step, as in the vector env.  The reference's fallback there -- Python's unseeded random.choice over the
 *    legal list -- is not reproducible and is not restated.
 *  - A committed step that faults, or whose observation raises (the reference's step returns get_observation()), ends
 *    the game as a draw with that code, the bot's step or the agent's.
 *  - There is no guard like FAULT_BOT_BOUND / FAULT_OPP_BOUND: every committed step counts towards max_turns, so a bot
 *    that repeats a USE which does nothing runs the game into max_turns, as it does in the reference's loop.
 *  - out_steps counts all committed steps; monsoon_stats.decisions only the heuristic agent's decisions and
 *    lookahead_steps only its look-aheads (a bot step is one committed transition and no look-ahead).
 *  - out_counts[n_individuals][3] is accumulated into the row of the match's INDIVIDUAL: p1 if it is one (a win = FIRST
 *    won), else p2 (a win = SECOND won); a match of the bot against itself touches no row.  out_results stays
 *    FIRST / SECOND (-1 draw, 0 FIRST, 1 SECOND).
 * A match without a bot is played exactly as monsoon_rollout plays it, so a schedule may mix both kinds.  The kernel is
 * the build's default variant, whatever lanes_per_game the handle was created with.  monsoon_rollout_faults,
 * monsoon_get_stats, monsoon_state_hash (final records of the last batch) and the replay of record-limited games on a
 * larger build work as after monsoon_rollout.  The games stay loaded with the bot's row in place: monsoon_decide_round_dev
 * / monsoon_play_rounds_dev refuse them (MONSOON_ERR_STATE) until players are assigned again; monsoon_rollout itself and
 * monsoon_assign_players keep refusing negative rows, and monsoon_state_load never loads one. */
#define MONSOON_PLAYER_EXPERT (-1)
int monsoon_rollout_vs_expert(monsoon_t* h, const double* weights, int32_t n_individuals, const monsoon_match* matches,
                              int32_t n_matches, const uint8_t* deck_pairs, int32_t n_decks, int32_t max_turns,
                              int32_t* out_counts, int8_t* out_results, int32_t* out_steps);

/* A rollout that writes down what it plays: everything monsoon_rollout_vs_expert does with the same arguments
 * (MONSOON_PLAYER_EXPERT rows included: counts, results, steps, monsoon_rollout_faults, monsoon_get_stats,
 * monsoon_state_hash of the last batch, the bot's rows staying in place), plus one log entry per COMMITTED STEP of every
 * game.  Entry k of match i, at [i * max_turns + k], is the game's k-th committed step, so out_steps[i] is the number of
 * entries of row i; behind them the row holds the padding values.
 *  - A heuristic decision logs the action it committed, its best score -- the value monsoon_decide reports as out_score,
 *    bit for bit -- and the number of legal actions it looked ahead over.  A decision whose commit faults is a logged
 *    step, as it is a counted one.
 *  - A step of the scripted bot logs its action, a NaN score and a legal count of 0 (the bot computes neither).  A bot
 *    whose expert_action raises steps nothing and logs nothing.
 * The log arrays are caller-owned HOST buffers; the device side lives in the handle, is grown on demand and copied out
 * batch by batch.  A logged call plays min(max_games, max(1, 256 MiB / (11 * max_turns))) games per batch, so that a long
 * max_turns cannot ask for tens of GB of device log; at max_turns = 200 this does not bind up to 65 536 games.  The kernel
 * is one more instantiation of the decision loop at the build's default variant (k_play_log), whatever lanes_per_game the
 * handle was created with.  MONSOON_ERR_ARG: a NULL log or log->action, and whatever monsoon_rollout_vs_expert refuses. */
typedef struct {            /* caller-owned HOST buffers, row stride max_turns */
  uint8_t* action;          /* [n_matches][max_turns]  required; 255 behind the game's last step */
  double*  score;           /* [n_matches][max_turns]  may be NULL; the decision's best score (monsoon_decide's out_score);
                                                       a NaN for a bot step and behind the last step */
  int16_t* n_legal;         /* [n_matches][max_turns]  may be NULL; legal actions of the decision; 0 for a bot step and behind */
} monsoon_rollout_log;
int monsoon_rollout_logged(monsoon_t* h, const double* weights, int32_t n_individuals, const monsoon_match* matches,
                           int32_t n_matches, const uint8_t* deck_pairs, int32_t n_decks, int32_t max_turns,
                           int32_t* out_counts, int8_t* out_results, int32_t* out_steps, const monsoon_rollout_log* log);

/* A logged rollout whose heuristic decisions may explore (epsilon-greedy), with the greedy choice kept in the log:
 * monsoon_rollout_logged's contract word for word, with one change at a heuristic decision.  Let k be the committed-step
 * index of the decision (its entry of the log), n_legal >= 1 its legal count and s the side to play.  The decision
 * EXPLORES when bit s of ex->sides is set, and ex->until_step <= 0 or k < ex->until_step, and draw0 < ex->threshold; it
 * then commits the r-th action of the ascending legal list instead of the arg-max:
 *
 *   draw0 = hash32(ex->seed, match.seed, k, 0)
 *   draw1 = hash32(ex->seed, match.seed, k, 1)
 *   r     = ((uint64_t)draw1 * n_legal) >> 32
 *
 * hash32 is monsoon_amd/fitness.py's hash32 (32-bit integer arithmetic only), so the host reproduces every draw exactly.
 * The draws are keyed by the match's seed and the step index -- not by the slot, the batch or the record build:
 *  - the games per batch never change a game;
 *  - a game that is played again on a larger record (monsoon_rollout_faults, fitness._ladder) explores exactly as it did
 *    on the smaller one, step for step, for as long as the two games see the same legal counts;
 *  - two matches with the same seed share their draws (they differ only through their decks and players): give the
 *    matches of a schedule distinct seeds, or expect correlated exploration.
 * What does not change: the arg-max still runs over all candidates; log->score stays the decision's best score
 * (monsoon_decide's out_score), log->action is what was COMMITTED, log->n_legal the legal count; every legal action is
 * stepped exactly once (lookahead_steps and decisions count as before) and the commit re-executes nothing -- the committed
 * successor is the taken candidate's look-ahead record, its fault or raising observation ends the game as a draw with that
 * code, its features are the next decision's "before" side, exactly as for the arg-max winner.  The scripted bot's steps
 * never explore.  No draw touches the game's own numpy stream.  out_counts, out_results, out_steps, monsoon_rollout_faults,
 * monsoon_get_stats and monsoon_state_hash work as after monsoon_rollout_logged and describe the games that were played:
 * THE COUNTS OF AN EXPLORING CALL ARE NOT FITNESS (an individual that explored did not play its own policy).
 * xlog (may be NULL, each array may be NULL) adds per entry: greedy, the arg-max action of the decision (what
 * monsoon_rollout_logged would have logged there); explored, 1 where the draw said "explore" (also when the drawn action
 * is the greedy one); taken_score, the score of the committed action.
 * ex == NULL or ex->threshold == 0: no decision explores and every output of monsoon_rollout_logged is what that call
 * writes, bit for bit; greedy == action, explored == 0 and taken_score == score on decisions.
 * Device log: an entry takes B = 1 + 8 [score] + 2 [n_legal] + 1 [greedy] + 1 [explored] + 8 [taken_score] bytes, 1 .. 21,
 * counting the arrays asked for, and a call plays min(max_games, max(1, 256 MiB / (B * max_turns))) games per batch
 * (without an exploring rule and without an array of xlog the call is monsoon_rollout_logged itself, batch cap included).
 * The kernel is one more instantiation of the decision loop at the build's default variant (k_play_explore).
 * MONSOON_ERR_ARG with nothing launched: whatever monsoon_rollout_logged refuses, and ex->sides with a bit above bit 1. */
typedef struct {
  uint32_t seed;        /* names the stream of exploration draws */
  uint32_t threshold;   /* a decision explores iff draw0 < threshold; 0 = never */
  uint32_t sides;       /* bit 0: FIRST's decisions may explore, bit 1: SECOND's */
  int32_t  until_step;  /* only decisions at committed-step index k < until_step; <= 0 = no limit */
} monsoon_explore;
typedef struct {        /* caller-owned HOST buffers, row stride max_turns, each may be NULL */
  uint8_t* greedy;      /* [n_matches][max_turns] the arg-max action of the decision; 255 for a bot step and behind the last step */
  uint8_t* explored;    /* [n_matches][max_turns] 1 = this decision's draw said "explore"; 0 for a bot step and behind */
  double*  taken_score; /* [n_matches][max_turns] score of the action that was committed; NaN for a bot step and behind */
} monsoon_explore_log;
int monsoon_rollout_explore(monsoon_t* h, const double* weights, int32_t n_individuals, const monsoon_match* matches,
                            int32_t n_matches, const uint8_t* deck_pairs, int32_t n_decks, int32_t max_turns,
                            int32_t* out_counts, int8_t* out_results, int32_t* out_steps, const monsoon_rollout_log* log,
                            const monsoon_explore* ex, const monsoon_explore_log* xlog);

/* A logged rollout whose heuristic decisions may SAMPLE: softmax over the decision's scores with a temperature.
 * WHEN a decision leaves its arg-max is monsoon_rollout_explore's rule word for word -- the side's bit in sm->rule.sides,
 * until_step, draw0 = hash32(seed, match.seed, k, 0) < threshold, draw1 = hash32(seed, match.seed, k, 1) -- only WHAT it
 * commits instead changes.  Let s_j be the score of the j-th action of the ascending legal list (what monsoon_decide
 * reports in out_scores: 0.0 for a look-ahead that raised or faulted) and best the decision's best score (log->score):
 *
 *   x_j   = (s_j - best) * inv_temperature      two operations, each rounded once; inv_temperature = 1.0 / T, the caller's
 *   w_j   = weight24(x_j)                       uint32 in [0, 2**24]
 *   total = sum_j w_j                           <= 156 * 2**24 < 2**32: exact, whatever the order
 *   r     = ((uint64_t)draw1 * total) >> 32     in [0, total)
 *   j*    = the smallest j with w_0 + ... + w_j > r
 *
 * weight24(x) = floor(exp(x) * 2**24), computed without a library exponential and with no term contracted into an fma
 * (monsoon_amd/csrc/sample_weight.h; monsoon_amd/game_log.py sample_weights is the same function in numpy, bit for bit):
 *
 *   if !(x >= -32.0) return 0                   also NaN and -inf
 *   n = floor(x * 0x1.71547652b82fep+0 + 0.5)
 *   r = (x - n * 0x1.62e42feep-1) - n * 0x1.a39ef35793c76p-33
 *   p = c10; for k = 9 .. 0: p = p * r + c_k    c_k = the double nearest 1 / k!
 *   return (uint32) floor(ldexp(p, (int)n + 24))
 *
 * weight24(0) = 2**24: the arg-max weighs 2**24 and so does every action tied with it, so total >= 2**24 whenever best is
 * a finite number.  TIES: actions tied for the best score share the probability equally -- a sampling decision may commit
 * an action other than the arg-max whose score equals the best one; that is the rule's meaning, not an accident.
 * total == 0 happens only when best is NaN or infinite: the decision commits its arg-max, explored is still 1 (the draw
 * said so), weight_total and taken_weight are 0.
 * What does not change from monsoon_rollout_explore: the arg-max runs over all candidates; log->score is the best score,
 * log->action what was committed; xlog->greedy, explored and taken_score mean what they mean there; a committed
 * candidate's fault or raising observation ends the game as a draw with that code; no draw touches the game's numpy
 * stream; a game's draws depend on its seed and step alone, not on the batch or the record build; THE COUNTS OF SUCH A
 * CALL ARE NOT FITNESS.
 * What does change: the choice is known only after the last look-ahead, so a decision that samples an action other than
 * its arg-max steps that action once more from the parent record (bit-identical to its look-ahead: the clone carries the
 * stream window).  lookahead_steps keeps counting n_legal per decision: A SAMPLING DECISION EXECUTES ONE STEP MORE THAN
 * IT COUNTS (none where it drew its arg-max).
 * slog (may be NULL, each array may be NULL) adds per entry weight_total = total and taken_weight = w of the committed
 * action.  BEHAVIOUR PROBABILITY: taken_weight / weight_total is the probability of the committed action GIVEN THAT THE
 * DECISION SAMPLED.  For a learner that weights off-policy: a decision of a side and step the rule covers samples with
 * probability eps = threshold / 2**32, so the behaviour policy gave the committed action a
 *   mu(a) = (1 - eps) * [a == greedy] + eps * taken_weight / weight_total     where explored == 1 and weight_total > 0,
 * and for an entry with explored == 0 (action == greedy) mu(a) = (1 - eps) + eps * p_greedy, whose p_greedy the log does
 * not carry (weight_total is 0 there; monsoon_rollout_policies, below, writes the weights on those entries too); with
 * eps == 1 every covered decision sampled and mu is the ratio itself.
 * sm == NULL or sm->rule.threshold == 0: no decision samples and every output of monsoon_rollout_logged is what that
 * call writes, bit for bit; greedy == action, explored == 0, taken_score == score on decisions, both weights 0.
 * Device log: an entry takes B = monsoon_rollout_explore's bytes + 4 [weight_total] + 4 [taken_weight], 1 .. 29, counting
 * the arrays asked for, and a call plays min(max_games, max(1, 256 MiB / (B * max_turns))) games per batch.  The call
 * also keeps the handle's score table ([max_games][156] doubles, monsoon_decide's) on the device: the kernel parks a
 * decision's scores there.  The kernel is one more instantiation of the decision loop at the build's default variant
 * (k_play_sample).
 * MONSOON_ERR_ARG with nothing launched: whatever monsoon_rollout_explore refuses, and an inv_temperature that is NaN,
 * infinite or <= 0. */
typedef struct { monsoon_explore rule; double inv_temperature; } monsoon_sample;    /* inv_temperature finite and > 0 */
typedef struct { uint32_t* weight_total; uint32_t* taken_weight; } monsoon_sample_log; /* HOST [n_matches][max_turns], each may be NULL;
                                                                                         0 for a bot step, a decision that did not sample, and behind */
int monsoon_rollout_sample(monsoon_t* h, const double* weights, int32_t n_individuals, const monsoon_match* matches,
                           int32_t n_matches, const uint8_t* deck_pairs, int32_t n_decks, int32_t max_turns,
                           int32_t* out_counts, int8_t* out_results, int32_t* out_steps, const monsoon_rollout_log* log,
                           const monsoon_sample* sm, const monsoon_explore_log* xlog, const monsoon_sample_log* slog);

/* A logged rollout in which every individual explores by a rule of its own, with the behaviour probability of every
 * decision in the log: monsoon_rollout_sample's contract word for word -- the draws and their hash32 keys, x_j, weight24,
 * total, r and j*, the re-step of a drawn action that is not the arg-max, the counters, the faults, the batch cap by the log
 * bytes asked for (1 .. 29 per entry), the score table kept on the device, THE COUNTS ARE NOT FITNESS -- with two changes.
 *  1. THE ROW OF THE MOVER.  A heuristic decision reads pol->threshold[r] and pol->inv_temperature[r], r = match.p1 when
 *     FIRST is to play and match.p2 when SECOND is: the row whose weights score the decision (a hall-of-fame row is a row
 *     like any other).  seed, sides and until_step stay call-wide.  The scripted bot never explores.  So one call plays a
 *     greedy champion (threshold 0) against the same weights played loosely, a uniformly exploring copy, a cold softmax.
 *  2. WEIGHTS ON EVERY COVERED DECISION.  A decision is COVERED when its side's bit is set in pol->sides, until_step allows
 *     its step k, and threshold[r] > 0.  Every covered decision writes weight_total = total and taken_weight, whether
 *     draw0 < threshold[r] said "sample" or not; one that did not sample commits its arg-max, whose weight is weight24(0) =
 *     2**24 where total > 0, and 0 otherwise.  explored still says what the draw said.  A decision that is not covered
 *     writes 0 in both, as do bot steps and the padding.  With eps_r = threshold[r] / 2**32 the behaviour policy gave the
 *     committed action of a covered decision with weight_total > 0
 *       mu(a) = (1 - eps_r) * [a == greedy] + eps_r * taken_weight / weight_total
 *     exactly, sampled or not (monsoon_amd/game_log.py behaviour_prob); every other decision committed its arg-max with
 *     probability 1.
 * inv_temperature[r] == 0.0 is the uniform rule through the same formulas, no branch: x_j = (s_j - best) * 0.0 weighs
 * every finite score 2**24, so j* = ((draw1 * n_legal * 2**24) >> 32) >> 24 = (draw1 * n_legal) >> 32, which is
 * monsoon_rollout_explore's rank.  With a NaN or infinite best score total is 0 and the decision commits its arg-max, as in
 * monsoon_rollout_sample (there monsoon_rollout_explore would commit its rank).
 * Every threshold 0: every output of monsoon_rollout_logged is what that call writes, bit for bit; greedy == action,
 * explored == 0, taken_score == score on decisions, both weights 0 (without an array of xlog or slog the call is
 * monsoon_rollout_logged itself, batch cap included).
 * The two tables are copied to device buffers of the handle, grown on demand, once per call before the first batch.  The
 * kernel is one more instantiation of the decision loop at the build's default variant (k_play_policy).
 * MONSOON_ERR_ARG with nothing launched and the loaded games untouched: whatever monsoon_rollout_sample refuses; a NULL
 * pol, threshold or inv_temperature; an inv_temperature[r] that is NaN, infinite or < 0 for any r < n_individuals, also
 * where threshold[r] == 0. */
typedef struct {
  uint32_t seed;                  /* as monsoon_explore.seed */
  uint32_t sides;                 /* as monsoon_explore.sides; a bit above bit 1: MONSOON_ERR_ARG */
  int32_t  until_step;            /* as monsoon_explore.until_step */
  const uint32_t* threshold;      /* HOST [n_individuals]; row r's decisions leave the arg-max iff draw0 < threshold[r]; 0 = never */
  const double*   inv_temperature;/* HOST [n_individuals]; finite and >= 0; 0.0 = the uniform rule */
} monsoon_policies;
int monsoon_rollout_policies(monsoon_t* h, const double* weights, int32_t n_individuals, const monsoon_match* matches,
                             int32_t n_matches, const uint8_t* deck_pairs, int32_t n_decks, int32_t max_turns,
                             int32_t* out_counts, int8_t* out_results, int32_t* out_steps, const monsoon_rollout_log* log,
                             const monsoon_policies* pol, const monsoon_explore_log* xlog, const monsoon_sample_log* slog);

/* Logged games played again on the device into the (state, action) rows a learner trains on: one row per kept log entry,
 * holding the state BEFORE that entry's step.  No decision is recomputed: every entry costs one committed step.
 * matches, deck_pairs, the log (log_action[n_matches][log_stride], log_steps[n_matches] entries per row, what
 * monsoon_rollout_logged wrote as log->action and out_steps), keep and the three out_* arrays are HOST buffers; the rows
 * are DEVICE buffers of the caller.  p1 / p2 of a match are read only for MONSOON_PLAYER_EXPERT: no weight table is needed.
 * Every game is reset from its seed and deck pair, then for entry k = 0 .. log_steps[g]-1 with action a, in this order:
 *  1. the game is over by the rollout's rules -- a winner, a fault, or an observation that raised after the step before:
 *     it stops with MONSOON_REPLAY_ENDED_EARLY;
 *  2. a is not < 156 or not legal (PASS, 155, is always accepted, as monsoon_step accepts it): MONSOON_REPLAY_ILLEGAL;
 *  3. if keep is NULL or keep[g][k] != 0 the entry's row is written (below);
 *  4. if the side to play is MONSOON_PLAYER_EXPERT in the match, the bot's expert_action runs and consumes the game's
 *     stream as it did in the rollout; it raises: MONSOON_REPLAY_BOT_RAISED; its action is not a: MONSOON_REPLAY_BOT_DIFFERS;
 *  5. a is stepped.  A step that faults, or after which the observation raises, ends the game (the code in out_fault,
 *     as monsoon_rollout_faults reports it: a code >= 16 other than 18 is a limit of this build's record).
 * out_status[g] = 0 or the stop's code, out_replayed[g] = the steps committed, out_fault[g] = the game's fault code.
 * Rows are in match order, then entry order: game g's first kept entry is row base[g] = the kept entries k < log_steps of
 * the games before it, S of them in all (*out_rows).  action[0 .. S) is filled with 255 before anything is replayed, so the
 * rows of a stopped game from its stop on read action 255; THEIR OTHER COLUMNS ARE UNSPECIFIED.
 * At most max_games games are played at a time, as the rollouts do; the last batch stays loaded in its final states
 * (monsoon_state_hash, monsoon_get_stats work as after a rollout; every side that is not the bot holds weight row 0).  The
 * device copy of the log lives in the handle and grows on demand.  The call returns when the host outputs are written,
 * and counts as one timed launch per batch (monsoon_kernel_time).
 * MONSOON_ERR_ARG, with nothing launched, no output written and the loaded games untouched: a NULL h / matches /
 * deck_pairs / log_action / log_steps / rows / rows->action, n_matches / n_decks / log_stride <= 0, a deck index outside
 * n_decks, a card this build does not support, log_steps[g] outside 0 .. log_stride, S > rows_cap, legal / obs / game / step
 * not 4-byte or state_hash not 8-byte aligned.  out_rows, out_status, out_replayed, out_fault may be NULL. */
#define MONSOON_REPLAY_OK          0
#define MONSOON_REPLAY_ILLEGAL     1   /* a logged action that is not legal where it is replayed */
#define MONSOON_REPLAY_BOT_DIFFERS 2   /* the bot's expert_action is not the logged action */
#define MONSOON_REPLAY_BOT_RAISED  3   /* the bot's expert_action raised where the log has a step */
#define MONSOON_REPLAY_ENDED_EARLY 4   /* the game ended before its last entry */
typedef struct {          /* DEVICE pointers, S rows; all but action may be NULL and then cost nothing */
  int32_t*  obs;          /* [S][27][5][4] the observation BEFORE the step, 0 where it raises */
  uint8_t*  legal;        /* [S][156] 1 = legal (monsoon_env_views' layout) */
  uint8_t*  obs_raises;   /* [S] */
  uint8_t*  to_play;      /* [S] */
  uint8_t*  action;       /* [S] required; 255 = a row the replay did not reach */
  uint8_t*  bot;          /* [S] 1 = a step of the scripted bot */
  int32_t*  game;         /* [S] match index */
  int32_t*  step;         /* [S] entry index k */
  uint64_t* state_hash;   /* [S] canonical hash of the state before the step (what monsoon_state_hash reports) */
} monsoon_replay_rows;
int monsoon_replay_logged_dev(monsoon_t* h, const monsoon_match* matches, int32_t n_matches,
                              const uint8_t* deck_pairs, int32_t n_decks,
                              const uint8_t* log_action, int32_t log_stride, const int32_t* log_steps,
                              const uint8_t* keep /* [n_matches][log_stride], NULL = every entry */,
                              const monsoon_replay_rows* rows, int64_t rows_cap, int64_t* out_rows,
                              uint8_t* out_status, int32_t* out_replayed, uint8_t* out_fault);

/* monsoon_replay_logged_dev whose rows also carry the candidates the choice was made among: for every kept entry the
 * afterstates of the state its row shows, K = max_after entries per row.  Row r of `after` is what
 * monsoon_env_afterstates_dev (below) writes for a slot in that state, with monsoon_env_after's meaning word for word --
 * the order of the entries, n_legal beyond K, action 255 for k >= min(n_legal, K), the status codes, reward 0 and winner -2
 * where the step raised, features and obs only where status == 0 -- except that before_features reads zeros where the
 * row's observation raises.  chosen[r] is the rank of the row's logged action in the ascending legal list, so
 * action[r][chosen[r]] is rows->action[r] wherever 0 <= chosen[r] < K; it is -1 for a PASS that is accepted without being
 * in the legal set.  Entries k >= min(n_legal, K) of every column but action, what monsoon_env_after leaves unwritten,
 * and every column of the rows behind a game's stop (rows->action 255) are UNSPECIFIED.
 * The look-ahead of a row happens in step 3 of the order above, when the row is written and before the bot's
 * expert_action, and consumes nothing: the game's cursor, stream blocks and record, the rows, out_status, out_replayed and
 * out_fault are those of monsoon_replay_logged_dev with the same arguments.  A candidate that hits a limit of this
 * build's record (a code >= 16 other than 18) shows it in status only; out_fault reports committed steps.
 * monsoon_get_stats after the call: lookahead_steps counts the candidates stepped, min(n_legal, K) per kept entry that was
 * reached; decisions counts nothing, as after monsoon_replay_logged_dev.
 * after == NULL: the call is monsoon_replay_logged_dev (max_after is not read).  Otherwise MONSOON_ERR_ARG, with nothing
 * launched, no output written and the loaded games untouched, for whatever monsoon_replay_logged_dev refuses, max_after
 * outside 1..156, a NULL after->n_legal or after->action, n_legal or obs not 4-byte, chosen not 2-byte, features or
 * before_features not 8-byte aligned. */
typedef struct {            /* DEVICE pointers; S rows, K = max_after entries per row; any may be NULL except n_legal and action */
  int32_t* n_legal;         /* [S]        legal actions of the row's state (the full count, also beyond K) */
  int16_t* chosen;          /* [S]        rank of the row's logged action in the ascending legal list (may be >= K); -1 if it is not in the legal set */
  uint8_t* action;          /* [S][K]     k-th legal action, ascending; 255 for k >= min(n_legal, K) */
  uint8_t* status;          /* [S][K]     monsoon_env_after's status */
  int8_t*  reward;          /* [S][K] */
  int8_t*  winner;          /* [S][K] */
  double*  features;        /* [S][K][10] only where status == 0 */
  double*  before_features; /* [S][10]    zeros where the row's observation raises */
  int32_t* obs;             /* [S][K][27][5][4] only where status == 0 */
} monsoon_replay_after;
int monsoon_replay_logged_after_dev(monsoon_t* h, const monsoon_match* matches, int32_t n_matches,
                                    const uint8_t* deck_pairs, int32_t n_decks,
                                    const uint8_t* log_action, int32_t log_stride, const int32_t* log_steps,
                                    const uint8_t* keep /* [n_matches][log_stride], NULL = every entry */,
                                    const monsoon_replay_rows* rows, int64_t rows_cap, int64_t* out_rows,
                                    uint8_t* out_status, int32_t* out_replayed, uint8_t* out_fault,
                                    const monsoon_replay_after* after, int32_t max_after /* 1..156 */);

/* Per-game decks of configuration C5 on the device: for every seed, numpy.random.RandomState(seed).choice(pool, 12,
 * replace=False) twice -> out_pairs[n][2][12] (card indices taken from pool[pool_n], 12 <= pool_n <= 128).  The caller
 * passes the pre-stream seeds (game seed ^ 0x9E3779B9).  Host buffers in and out; needs no loaded games.
 * Replaces the per-game Python draw of games/evolutionary_stormbound.py:52 + utils.py:26-119 for this configuration
 * (150 us per game in numpy, 79 s for one C5 generation). */
int monsoon_draw_decks(monsoon_t* h, const uint32_t* seeds, int32_t n, const uint8_t* pool, int32_t pool_n, uint8_t* out_pairs);

/* Per-game decks of a deck schedule on the device (utils.py:121-242, DeckEvolutionConfig; the per-game mode of
 * monsoon_amd/decks.py): for every game seed the pair that get_deck_configuration(generation) draws from a stream of the
 * game's own -> out_pairs[n][2][12], P1's deck first.
 *
 * The stream is Python's generator, random.Random(seed | generation << 32 | game_seed << 64 | tag << 96): CPython seeds an
 * int with init_by_array over its 32-bit words, here always the four words {seed, generation, game_seed, tag} since
 * tag != 0 (the Python layer: 1 = evaluate_population, 2 = evaluate_vs_expert).  A game's pair depends on these four words
 * and the schedule below, not on its place in game_seeds, on the device or rank, or on any other game.
 *
 * The draws, as Lib/random.py makes them (random: two outputs; _randbelow(n): u32 >> (32 - n.bit_length()) until < n;
 * sample(pop, k): the pool path for len(pop) <= 21 (+ 64 for k > 5), else the set path):
 *   phase 1 (explore), per side, P1 first: sample(archetype, n_preserve), then sample(pool, 12 - n_preserve); preserved
 *           and new cards may repeat, as in the reference.  n_preserve = 12 is the archetype itself without a draw
 *           (generate_random_deck with preserve_ratio == 1.0).  The caller computes n_preserve =
 *           min(int(12 * (1.0 - ratio)), 12) in the reference's own float arithmetic; the device does none of it.
 *   phase 2 (balance): random() < balance_archetype_ratio for P1, then for P2; then sample(pool, 12) for each side whose
 *           test failed, P1 first; the other side plays its archetype.  n_preserve is ignored.
 * The exploit phase draws nothing and monsoon_draw_schedule refuses its phase number (0; monsoon_env_set_schedule takes
 * it).  pool[side][0..pool_n[side]) are card indices in
 * available_cards order (utils.py:63-88), 12 <= pool_n <= 128: random.choices, which the reference falls back to for a
 * pool of fewer than 12 cards, is not restated (no faction has such a pool).
 *
 * A game may use the first 624 outputs of its stream (one twist; the draws above took at most 90 in 72 000 test games).  Games that
 * would need more are counted and the call fails with MONSOON_ERR_STATE: none is truncated silently.
 * Host buffers in and out; needs no loaded games.  MONSOON_ERR_ARG: n <= 0, tag == 0, a phase other than 1 / 2,
 * n_preserve outside 0..12, a pool size outside 12..128, an archetype or pool entry that is not a card index. */
typedef struct {
  uint32_t seed;         /* the schedule's seed, low 32 bits */
  uint32_t generation;
  uint32_t tag;          /* != 0 */
  int32_t phase;         /* 1 explore, 2 balance; 0 static (monsoon_env_set_schedule only): both sides play their archetype */
  int32_t n_preserve;    /* explore: archetype cards kept, 0..12 */
  int32_t pool_n[2];
  double balance_archetype_ratio;
  uint8_t archetype[2][12];
  uint8_t pool[2][128];
} monsoon_deck_schedule;
int monsoon_draw_schedule(monsoon_t* h, const monsoon_deck_schedule* schedule, const uint32_t* game_seeds, int32_t n, uint8_t* out_pairs);
/* HIP-event time of the kernel inside the handle's last monsoon_draw_schedule call, without its copies (0 before one). */
int monsoon_draw_schedule_time(monsoon_t* h, double* kernel_ms);

/* GA operators on the device.  The host GA (monsoon_amd/population.py, as the reference's
 * evo/population.py) stays the default and the bit-exact path; these are the same operators over the same numpy stream
 * for a driver that wants the population to stay next to the rollouts.
 *
 * monsoon_np_state = numpy.random.RandomState.get_state(legacy=False) of the GLOBAL stream the reference draws from
 * (np.random.*): the mt19937 key, its position, and the cached second normal of legacy_gauss; in/out.
 *
 * monsoon_ga_offspring: Population.generate_offspring, evo/population.py:75-89 with WeightVector.copy / mutate,
 * evo/weights.py:12-40: lambda offspring of parents[mu][dim] (weights, sigmas).  out_parent[lambda] = the parent drawn for
 * each child, out_tries[lambda] = polar-method rounds consumed up to and including that child (both optional).  Every
 * draw and every accept / reject decision is numpy's own, so the parents and the returned stream state (key, position,
 * has_gauss) are bit-identical to the host's; exp / log / sqrt are the device library's, within 1 ulp of the host's,
 * so weights and sigmas agree with the host's to a few ulp (tests/test_gpu_parity.py; tests/test_ga_operators_gpu.py at mu
 * that is no power of two, dim 1..16, clamped, infinite and NaN sigmas and every kind of state to enter with).
 *
 * monsoon_ga_select: the order of select_from_combined, evo/population.py:91-103: indices of all n individuals by
 * descending fitness, equal fitness in original order (Python's stable sort with reverse=True). */
typedef struct {
  uint32_t key[624];
  int32_t pos;        /* 0..624 (624 = the next draw regenerates the key) */
  int32_t has_gauss;
  double gauss;
} monsoon_np_state;
int monsoon_ga_offspring(monsoon_t* h, monsoon_np_state* st, const double* parents_w, const double* parents_s, int32_t mu, int32_t dim,
                         int32_t lambda, double tau, double tau_prime, double min_sigma, double* out_w, double* out_s, int32_t* out_parent,
                         int64_t* out_tries);
int monsoon_ga_select(monsoon_t* h, const double* fitness, int32_t n, int32_t* out_order);

/* Diagnostics: 192 raw counter words (words 0-4 back monsoon_get_stats; words 6 / 7 count the vector env's committed
 * agent / opponent steps since monsoon_env_reset, word 7 those of either opponent kind, scripted bot or heuristic agent;
 * word 16 the heuristic opponent's look-ahead transitions since monsoon_env_reset; word 17 the episodes of a schedule-mode
 * env since monsoon_env_reset whose deck walk ran past the 624 outputs of its stream (monsoon_env_set_schedule); a profiling build (-DMSB_PROF=1,
 * scripts only) adds k_decide phase cycles at 8..15, per-function cycles / calls at 32..63 / 64..95, last-launch
 * occupancy at 96..101 and call entry / exit cycles at 128..159 / 160..191; the rest is zero).
 * No reference counterpart. */
int monsoon_debug_counters(monsoon_t* h, unsigned long long* out192);

/* Device-resident variant used by bench.py: one decision round over the games already loaded by
 * monsoon_reset, weights taken from a table uploaded once.  Nothing crosses PCIe. */
int monsoon_upload_weights(monsoon_t* h, const double* weights, int32_t n_individuals);
int monsoon_assign_players(monsoon_t* h, const int32_t* p1, const int32_t* p2);   /* [n] indices */
int monsoon_decide_round_dev(monsoon_t* h);   /* asynchronous on the handle's stream */
/* `rounds` decisions of every loaded game in one launch (evo/fitness.py:193-211, a slice of the _play_game loop): a
 * game's record stays on chip from its first to its last decision of the call.  Asynchronous like the call above.
 *
 * Both calls may play the second half of a large batch on a second stream of the handle, so that the next call's first
 * half fills the GPU while this call's second half runs out of games (MONSOON_SPLIT=0 in the environment, read per
 * call: always one launch on the handle's stream).  Every other entry point, monsoon_sync and monsoon_stream included,
 * first makes the handle's stream wait for that half: a caller that orders work of its own behind these two calls
 * fetches monsoon_stream after them, or calls monsoon_sync.  While the handle's stream is being captured into a graph
 * both calls record a single launch of one workgroup per game (never split, untimed), which may be replayed any number
 * of times in a row; fetch monsoon_stream after the last eager call and before the capture begins. */
int monsoon_play_rounds_dev(monsoon_t* h, int32_t rounds);
int monsoon_sync(monsoon_t* h);

int monsoon_get_stats(monsoon_t* h, monsoon_stats* out);
int monsoon_reset_stats(monsoon_t* h);
/* HIP-event timing of the decide kernel since the last reset_stats: total ms and launch count. */
int monsoon_kernel_time(monsoon_t* h, double* total_ms, int64_t* launches);
/* The stream the handle launches on (hipStream_t) so a caller can order its own work; NULL-safe.  Every handle has a
 * stream of its own (one handle = one device + one stream; independent handles are independent).  MONSOON_OWN_STREAM=0
 * in the environment puts all handles on the device's default stream (returned as NULL), as round 2 had to. */
void* monsoon_stream(monsoon_t* h);

/* Device-resident vector environment (Seam G, batched: games/abstract_game.py step / to_play / legal_actions / reset /
 * expert_agent): n independent slots, each an endless sequence of episodes.  monsoon_env_step_dev checks every action
 * against its slot's legal set, steps it, lets the reference's scripted bot answer (opponent 1), ends finished episodes,
 * starts the next one in the same slot and writes the observation and legal mask of the state each slot is now in -- all
 * on the handle's stream, without a host round trip, so a caller can capture it into a graph.
 *
 * Episode k of slot i starts from seed seed0[i] + k * seed_stride (mod 2^32).  Without a pool it is
 * monsoon_reset(seed, decks[i], factions) with factions[i] for episode 0 and {0, 0} (monsoon_reset's NULL factions) for
 * the later ones; episode 0 equals monsoon_reset(seed0[i], decks[i], factions[i]) bit for bit.  With a pool, every
 * episode (episode 0 included) plays the decks monsoon_draw_decks draws from seed ^ 0x9E3779B9 (configuration C5).  Without
 * decks and without a pool -- schedule mode, after monsoon_env_set_schedule -- every episode (episode 0 included) plays the
 * pair the handle's deck schedule draws for its seed, see there; factions as without a pool.
 *
 * An episode ends after a committed step (the agent's or the bot's) that faults, whose observation would raise
 * (FAULT_INT_CARD: the reference's step returns get_observation()), that leaves a winner (have_winner), or that brings its
 * committed steps to max_steps (truncated).  A bot whose expert_action raises ends it with that fault.  The bot plays at
 * most 64 actions per call: a bot still to play after that ends the episode with fault 27 (a guard of this library: the
 * reference's bot can pick a USE whose index does nothing and costs nothing -- action 64 + 21 * c + 20 -- over and over
 * and never end its turn; the tests require every fault 27 to be such a turn).  An episode can also end before the agent acts (the bot's opening turn,
 * or a first state whose observation raises): the slot then reports that end at the next step, whatever its action.
 *
 * Opponent 2 is the reference's HeuristicAgent (evo/heuristic_agent.py) with the weights monsoon_env_set_opponents gives
 * each slot.  It plays the side agent_side does not play, while that side is to play; each of its decisions is exactly
 * monsoon_decide's (1-ply look-ahead over every legal action, score, first maximum, commit), and the episode ends by the
 * rules above after each of its committed steps.  It plays at most 64 decisions per call: an opponent still to play
 * after that ends the episode with fault 28 (FAULT_OPP_BOUND, the same guard as fault 27: a no-op USE that wins the
 * argmax once wins it for ever from the identical state).  With agent_side 1 it plays the opening turn of every episode. */
typedef struct {
  int32_t opponent;      /* 0 = none (the caller acts for whichever side is to play), 1 = the reference's scripted bot,
                            2 = the reference's HeuristicAgent (monsoon_env_set_opponents first) */
  int32_t agent_side;    /* with opponent 1 or 2: 0 = agent plays FIRST, 1 = SECOND (the opponent plays the other side) */
  uint32_t seed_stride;  /* episode k of slot i starts from seed0[i] + k * seed_stride (mod 2^32); 0 = n */
  int32_t max_steps;     /* an episode reaching this many committed steps (agent + bot) ends truncated; 0 = no limit, <= 65535 */
  int32_t pool_n;        /* 0 = every episode of slot i uses the slot's reset decks (NULL decks: the handle's schedule draws
                            them per episode, monsoon_env_set_schedule); 12..128 = fresh decks per episode */
  uint8_t pool[128];     /*   drawn as monsoon_draw_decks draws them, from the episode seed ^ 0x9E3779B9 */
} monsoon_env_config;

typedef struct {          /* caller-owned DEVICE buffers, n entries each; any may be NULL except done; obs and legal 4-byte aligned */
  int32_t* obs;           /* n*540: observation of the state the slot is now in (after auto-reset / the bot's turn); 0 where it raises */
  uint8_t* legal;         /* n*156 bytes 0/1 (viewable as torch.bool) */
  uint8_t* obs_raises;    /* as monsoon_observe's raises */
  uint8_t* to_play;
  int8_t*  reward;        /* the reference's reward of the AGENT's own step, {0,1} (games/stormbound.py:366) */
  uint8_t* done;          /* the episode ended in this call (winner, fault or truncation) */
  int8_t*  winner;        /* at done: 0 FIRST, 1 SECOND, -1 draw/fault/truncated (rollout contract); -2 otherwise */
  uint8_t* truncated;
  uint8_t* fault;         /* fault code that ended the episode (msb_base.h), 0 = none */
  uint8_t* illegal;       /* the action was not legal: the slot was left untouched */
  int32_t* episode;       /* episodes completed by the slot so far */
  uint64_t* final_hash;   /* at done: FNV-1a 64 of the canonical record the episode ended in (as monsoon_state_hash); 0 otherwise */
} monsoon_env_views;

/* Allocates the env's workspace, binds the views (kept until the next monsoon_env_reset), loads episode 0 of every slot
 * (with opponent 1 and agent_side 1 the bot's opening turn is played) and writes its observation and legal mask; the
 * per-call views read as after a step that ended nothing.  Host arguments: seed0[n], decks[n][2][12] (NULL, and only NULL,
 * with a pool; NULL without a pool = schedule mode, MONSOON_ERR_ARG unless the handle holds a schedule), factions[n][2] or
 * NULL.  A deck or pool card this build does not support is refused (MONSOON_ERR_ARG).
 * Synchronises.  The env's slots are the handle's loaded games: monsoon_state_hash, monsoon_observe, monsoon_state_save
 * and the rest work on them; monsoon_reset or monsoon_rollout ends env mode. */
int monsoon_env_reset(monsoon_t* h, const monsoon_env_config* cfg, const monsoon_env_views* views, int32_t n,
                      const uint32_t* seed0, const uint8_t* decks, const uint8_t* factions);
/* One step of every slot; actions_dev = n bytes of DEVICE memory: 255 leaves the slot untouched, 155 (PASS) is always
 * accepted, any other action must be legal, else illegal[i] = 1 and the slot is left untouched.  A slot whose episode
 * ended gets done / winner / truncated / fault / final_hash of that episode, episode[i] + 1, and the observation and legal
 * mask of its next episode's first state.  Asynchronous: enqueues three launches on the handle's stream (seven with
 * opponent 2; no allocation, copy or synchronisation); MONSOON_ERR_STATE without a preceding monsoon_env_reset or after
 * monsoon_reset. */
int monsoon_env_step_dev(monsoon_t* h, const uint8_t* actions_dev);

/* The heuristic opponents of opponent 2: weights[n_individuals][10] (host), and rows[n] (host), the weight row slot i's
 * opponent plays (NULL = row 0 for every slot).  Required before monsoon_env_reset with opponent 2 (else it returns
 * MONSOON_ERR_STATE), whose n must equal this n.  May be called again between steps: the new table and rows apply from the
 * next decision (a league update).  The table is allocated for the n_individuals given before the reset and never
 * reallocated while an opponent-2 env is loaded, so a captured step stays valid: a call with more rows then, a row outside
 * [0, n_individuals) or an n different from the loaded env's returns MONSOON_ERR_ARG.  Synchronises. */
int monsoon_env_set_opponents(monsoon_t* h, const double* weights, int32_t n_individuals, const int32_t* rows, int32_t n);

/* Epsilon-greedy heuristic opponents, epsilon per slot: the env's form of monsoon_rollout_explore's rule.
 *
 * Take a decision of slot i's heuristic opponent over n_legal >= 1 actions.  Let k be the number of steps the episode has
 * committed so far, the agent's and the opponent's together (the count max_steps is compared with), and
 * s = seed0[i] + episode[i] * seed_stride (mod 2^32) the seed of the slot's current episode, as the slot holds seed0, its
 * episode count and the stride at that moment.  With hash32 of monsoon_amd/fitness.py,
 *     draw0 = hash32(ex.seed, s, k, 0)      draw1 = hash32(ex.seed, s, k, 1)      r = ((uint64_t)draw1 * n_legal) >> 32
 * the decision EXPLORES when (until_step <= 0 || k < until_step) and draw0 < thresholds[i]: it then commits the r-th action
 * of the ascending legal list instead of the arg-max.  The arg-max still runs over all candidates; every legal action is
 * stepped exactly once (monsoon_debug_counters word 16 counts as before); the commit re-executes nothing: the committed
 * successor is the taken candidate's look-ahead record, and a fault or a raising observation of the taken candidate ends the
 * episode by the env's rules exactly as for the arg-max winner.  No draw touches the game's numpy stream.  The 64-decision
 * guard (fault 28) is unchanged.  Consequences: a rewind (monsoon_env_load_dev into the slot the entry came from) explores
 * exactly as the first run did; a fork into slots with other seed0 explores differently per slot (Monte-Carlo playouts from
 * a snapshot); two slots with equal seed0 share their draws.
 *
 * Which kernel plays the opponent is decided at monsoon_env_reset, so that a captured step never changes kernels: if the
 * handle holds a rule when an opponent-2 env is reset, every step of that env launches the exploring kernel where it
 * would launch the plain one (still seven launches on one stream); otherwise the env plays exactly as without this call.
 * The rule's two words and the n thresholds live in device buffers that are allocated by the first call (for max_games
 * slots) and never moved.  A call validates, copies them behind everything already enqueued on the handle's stream and
 * synchronises; it takes effect from the next decision, also under a captured step: the graph holds the addresses, not the
 * contents.  All thresholds 0 plays the non-exploring env bit for bit: that is how an env is armed for later use.
 *
 * thresholds: HOST uint32[n]; 0 = never, 0xFFFFFFFF = all but one draw in 2^32.  ex == NULL clears the rule (thresholds
 * and n are not read); MONSOON_ERR_STATE while an env that was reset with a rule is loaded.  MONSOON_ERR_STATE also when an
 * opponent-2 env that was reset WITHOUT a rule is loaded.  MONSOON_ERR_ARG: NULL thresholds with a non-NULL ex, n <= 0,
 * n > max_games, an n that differs from the loaded env's; monsoon_env_reset with opponent 2 and a rule whose n differs from
 * the reset's n returns MONSOON_ERR_ARG too.  Opponents 0 and 1 ignore the rule. */
typedef struct {
  uint32_t seed;        /* names the stream of exploration draws */
  int32_t  until_step;  /* only decisions at episode step index k < until_step explore; <= 0 = no limit */
} monsoon_env_explore;
int monsoon_env_set_opponent_explore(monsoon_t* h, const monsoon_env_explore* ex, const uint32_t* thresholds, int32_t n);
/* DEVICE uint32[n] -> out_dev: the decisions of slot i's opponent whose draw said "explore", since monsoon_env_reset (which
 * zeroes them; like monsoon_debug_counters words 6 / 7 / 16 they are neither saved nor restored by snapshots).  One
 * device-to-device copy on the handle's stream: asynchronous, no allocation or synchronisation, capturable.
 * MONSOON_ERR_STATE without a loaded env or when the env has no rule, MONSOON_ERR_ARG for a NULL out_dev. */
int monsoon_env_opponent_explored_dev(monsoon_t* h, void* out_dev);

/* Softmax heuristic opponents, a temperature per slot: monsoon_env_set_opponent_explore's rule for WHEN a decision leaves
 * its arg-max, monsoon_rollout_sample's rule for WHAT it then commits.
 *
 * WHEN.  Word for word the rule above: with k, s, draw0 and draw1 as defined there, a decision of slot i's opponent over
 * n_legal >= 1 actions SAMPLES when (until_step <= 0 || k < until_step) and draw0 < thresholds[i].
 * WHAT.  monsoon_rollout_sample's x_j, w_j, total, r and j* with the slot's own inverse temperature: over the ascending
 * legal list, x_j = (score_j - best) * inv_temperature[i], w_j = weight24(x_j), total = sum w_j,
 * r = ((uint64_t)draw1 * total) >> 32, and j* the smallest j whose inclusive prefix sum exceeds r; the decision commits
 * action j*.  Ties share the probability: an action tied with the arg-max weighs 2**24 as it does and may be committed
 * instead of it.  total == 0 (best is NaN or infinite) commits the arg-max and still counts as explored.
 * The arg-max runs over all candidates as ever.  The choice is known only after the last look-ahead, so a decision that
 * samples an action other than its arg-max steps that action once more from the parent record (bit-identical to its
 * look-ahead: the clone carries the stream window); that successor's fault or raising observation ends the episode by the
 * env's rules exactly as for the arg-max winner.  monsoon_debug_counters word 16 keeps counting n_legal per decision: A
 * DECISION THAT SAMPLED ANOTHER ACTION THAN ITS ARG-MAX EXECUTES ONE STEP MORE THAN IT COUNTS.  No draw touches the game's
 * numpy stream.  The 64-decision guard (fault 28) is unchanged.  A rewind samples exactly as the first run did; a fork into
 * slots with other seed0 samples differently per slot; two slots with equal seed0 and inverse temperature share their choices.
 *
 * WHICH KERNEL PLAYS.  The handle holds at most ONE opponent rule, uniform (monsoon_env_set_opponent_explore) or sampling
 * (this call): while no opponent-2 env is loaded either call replaces whatever rule is held.  Which of the three kernels --
 * plain, exploring, sampling -- plays the opponent is settled at monsoon_env_reset by the rule the handle then holds, and
 * never changes under a captured step (still seven launches on one stream).
 * DEVICE BUFFERS.  The inverse temperatures live beside the thresholds, in the buffer that the first call of either setter
 * allocates for max_games slots and that is never moved.  The kernel parks every decision's scores in the slot's row of the
 * handle's score table ([max_games][156] doubles, monsoon_decide's), which the first call allocates if monsoon_decide has
 * not and which is never moved either; only the sampling kernel is handed it.  A call validates, copies behind everything
 * already enqueued on the handle's stream and synchronises; it holds from the next decision on, also under a captured step.
 * All thresholds 0 plays the plain env bit for bit.  monsoon_env_opponent_explored_dev counts the decisions whose draw said
 * "sample" and serves both kinds.
 *
 * thresholds: HOST uint32[n]; inv_temperature: HOST double[n], 1 / T of slot i.  ex == NULL clears the rule (the other
 * arguments are not read).
 * MONSOON_ERR_ARG with nothing launched: whatever monsoon_env_set_opponent_explore refuses, a NULL inv_temperature with a
 * non-NULL ex, an entry that is NaN, infinite or <= 0.
 * MONSOON_ERR_STATE, for this call and for monsoon_env_set_opponent_explore alike: a non-NULL ex while an opponent-2 env
 * is loaded that was reset under the OTHER kind of rule or under no rule; ex == NULL while an env that uses the rule is
 * loaded. */
int monsoon_env_set_opponent_sample(monsoon_t* h, const monsoon_env_explore* ex, const uint32_t* thresholds,
                                    const double* inv_temperature, int32_t n);

/* Schedule mode: the third source of episode decks, beside the reset decks and the pool.  The handle keeps ONE deck schedule
 * in a device buffer that is allocated by the first call and never moved while an env is loaded.  monsoon_env_reset with
 * decks == NULL and pool_n == 0 plays schedule mode if the handle holds a schedule (MONSOON_ERR_ARG otherwise); with decks
 * or a pool it plays as ever and ignores the stored schedule.
 *
 * Episode k of slot i starts from s = seed0[i] + k * seed_stride as in the other modes.  Its decks are the pair
 * get_deck_configuration(generation) draws from random.Random(seed | generation << 32 | s << 64 | tag << 96): the
 * monsoon_draw_schedule contract above, keyed by the episode's seed, with seed, generation, tag, phase, n_preserve, ratio,
 * archetypes and pools those of the schedule the handle holds AT THE MOMENT THE EPISODE STARTS, drawn on the device by the
 * kernel that seeds the episode.  Episode 0 draws too.  The Python layer uses tag 3 (decks.TAG_ENV), so that an env episode
 * never shares its decks with the population's (1) or the bot's (2) game of the same seed.  Factions: factions[i] for
 * episode 0, {0, 0} afterwards.  Episode rules, opponents, afterstates and snapshots are those of the other modes: a
 * restored slot keeps the decks of its entry until that episode ends and then draws from the schedule current then, with the
 * destination's seed.
 *
 * Phase 0 (static; here only, monsoon_draw_schedule refuses it) is the schedule's exploit phase: both sides play their
 * archetype, no stream is read, n_preserve, pool_n and pool are ignored.
 *
 * monsoon_env_set_schedule(sc != NULL) validates, stores the schedule behind everything already enqueued on the handle's
 * stream, and synchronises.  With a schedule-mode env loaded the new schedule applies to every episode that starts from the
 * next monsoon_env_step_dev on -- also a captured one: the graph holds the buffer's address, not its contents -- while
 * running episodes keep their decks.  MONSOON_ERR_ARG: tag == 0, a phase outside 0..2, n_preserve outside 0..12, in phases
 * 1 / 2 a pool size outside 12..128, an archetype entry or (phases 1 / 2) a pool entry that is not a card index or that
 * this record build does not support (ua20 and b005 need the extended record; every faction's pool holds ua20); on the
 * standard build also an archetype or a pool that lists a unit or structure card twice, and phase 1 with 0 < n_preserve
 * < 12: the kept and the drawn cards of such a deck may repeat a card, which only the extended record plays as the
 * reference does, and the host never sees a deck drawn on the device.
 * sc == NULL clears the schedule; MONSOON_ERR_STATE while a schedule-mode env is loaded.
 *
 * A walk that would read past the first 624 outputs of its stream cannot fail an asynchronous step: such an episode is
 * counted (monsoon_debug_counters word 17, per env since monsoon_env_reset) and plays a pair of valid card indices that is
 * not the specification's draw.  No test game came near (at most 90 outputs). */
int monsoon_env_set_schedule(monsoon_t* h, const monsoon_deck_schedule* schedule);

/* The decks of every slot's current episode -> out_dev, uint8[n][2][12] of caller-owned DEVICE memory, P1's deck first: what
 * a learner on drawn decks is playing (the observation shows the hand, not the deck).  All three deck modes.  One
 * device-to-device copy on the handle's stream: asynchronous, no allocation or synchronisation, capturable.
 * MONSOON_ERR_STATE without a loaded env, MONSOON_ERR_ARG for a NULL out_dev. */
int monsoon_env_decks_dev(monsoon_t* h, void* out_dev);

/* Measurement: the HIP-event time of the reseed kernel -- the launch that seeds, and in pool and schedule mode draws the
 * decks of, the episodes that start -- inside the handle's last monsoon_env_step_dev -> *kernel_ms (0 if that step was not
 * timed).  enable != 0: every later step records an event pair round that launch (two host calls per step; never while the
 * stream is being captured); enable == 0 stops that.  Off by default.  Synchronises.  MONSOON_ERR_ARG for a NULL argument. */
int monsoon_env_reseed_time(monsoon_t* h, int32_t enable, double* kernel_ms);

/* Afterstates: the successor of every legal action of every slot's current state, for a learner that evaluates them
 * itself (afterstate TD, a value network over the successor's observation).  It is the reference's 1-ply look-ahead
 * (evo/heuristic_agent.py: copy.deepcopy of the game, stream included, then apply_action) without the score: the successor
 * of action a is exactly the state monsoon_env_step_dev would commit for a, before any opponent answers, and it is read
 * the way monsoon_step, monsoon_observe and monsoon_features read a plain handle.  The env's episode rules are NOT applied
 * to afterstates: no max_steps, no auto-reset, no bot turn.  The call works for whichever side is to play, with every
 * opponent kind (with opponent 1 or 2 that side is always the agent's).
 *
 * K = max_after entries per slot.  Entry k < min(n_legal, K) is the k-th legal action in ascending order; n_legal is the
 * full count, also where it exceeds K.  Entries k >= min(n_legal, K) get action = 255 and are otherwise not written.  An
 * entry whose status is not 0 gets action, status, reward and winner, but no features and no observation; where the step
 * itself raised (any status but FAULT_INT_CARD) the reference defines neither a reward nor a winner, and 0 and -2 are
 * written.  A slot whose episode already ended before the agent acts (the pending end monsoon_env_step_dev reports at the
 * next step) has n_legal = 0.
 *
 * The call changes nothing of the handle: no record, meta row, stream cursor, stream block, statistic or counter.  It is
 * asynchronous on the handle's stream: one launch, no allocation, host copy or synchronisation, so it captures into a
 * graph next to monsoon_env_step_dev.  MONSOON_ERR_STATE without a loaded env (before monsoon_env_reset, after
 * monsoon_reset / monsoon_rollout); MONSOON_ERR_ARG for max_after outside 1..156, a NULL out, n_legal or action, an n_legal
 * or obs that is not 4-byte aligned, or features / before_features that are not 8-byte aligned. */
typedef struct {            /* caller-owned DEVICE buffers; K = max_after; any may be NULL except n_legal and action;
                               n_legal and obs 4-byte aligned, features and before_features 8-byte aligned */
  int32_t* n_legal;         /* [n]       legal actions of the slot's current state (may exceed K); 0 for a slot whose episode
                                         already ended before the agent acts */
  uint8_t* action;          /* [n][K]    entry k = the k-th legal action in ascending order; 255 for k >= min(n_legal, K) */
  uint8_t* status;          /* [n][K]    0, or the fault code of the look-ahead step (msb_base.h), FAULT_INT_CARD (2) where the
                                         successor's observation would raise */
  int8_t*  reward;          /* [n][K]    the reference's reward of that step, as monsoon_step's */
  int8_t*  winner;          /* [n][K]    -2 = no winner after the step; else 0 / 1 / -1 by the rollout contract */
  double*  features;        /* [n][K][10] monsoon_features of the successor (status 0 only) */
  int32_t* obs;             /* [n][K][540] monsoon_observe of the successor (status 0 only); 4-byte aligned */
  double*  before_features; /* [n][10]   monsoon_features of the current state (not written where its observation raises,
                                         nor for a slot with n_legal = 0 by a pending end) */
} monsoon_env_after;

int monsoon_env_afterstates_dev(monsoon_t* h, const monsoon_env_after* out, int32_t max_after);   /* 1..156 */

/* Saving and restoring slots on the device (snapshot / fork): what a search deeper than one ply needs -- keep a state, put
 * it back into a slot, or into many slots at once -- without a host round trip.  (monsoon_state_save / monsoon_state_load
 * move one game per call through host memory, synchronise, and know nothing of the env's own per-slot state.)
 *
 * An ENTRY is monsoon_env_entry_bytes() of caller-owned DEVICE memory (a multiple of 16; 8 320 on the standard record)
 * and holds everything that makes the slot's future a function of the actions it is given: a 16-byte header (a magic
 * value, monsoon_version(), the record's size in words, the slot's episode count), the slot's bookkeeping row, the 24 deck
 * bytes of its current episode, its record, and its stream (the raw state and both resident blocks).  entries_dev is an
 * array of entries, 16-byte aligned.
 *
 * An entry does NOT hold the slot's configuration: the loading env's seed0[dst], seed_stride, opponent kind, agent_side,
 * max_steps, pool and -- with opponent 2 -- weight table and row of slot dst apply.  Of the bookkeeping row only the
 * episode's own fields are loaded (result, fault, last action, flags, committed steps, stream cursor); the weight rows p1 /
 * p2 and the schedule index belong to the handle (the env's opponent 2 never reads them: it plays the row
 * monsoon_env_set_opponents gave slot dst), and the row's look-ahead statistics stay the destination's.  The statistics
 * counters (monsoon_get_stats, monsoon_debug_counters words 6 / 7 / 16) are neither saved nor restored.
 *
 * What follows:
 *  - Loading an entry into the slot it came from is a rewind: every later step reproduces the first run bit for bit, for
 *    ever (the same actions given).
 *  - Loading it into another slot reproduces the source until that episode ends; the next episode then follows the
 *    destination's seed schedule with the carried episode count k: seed0[dst] + k * seed_stride.
 *  - A slot saved with an end pending (an episode that ended before the agent could act) is restored with it pending: the
 *    next step reports it.
 *  - Entries are plain device bytes: they can be copied, kept and loaded into any handle of the same record build and
 *    library version.  Nothing else is promised: an entry of another build or version, or a zero-filled one, never loads.
 *
 * monsoon_env_save_dev: entry j receives slot slots_dev[j] (DEVICE int32[m]; NULL = slot j, and then m <= n).  A slot
 * index outside [0, n) writes an entry whose header is zero.  Nothing of the handle changes.  One launch.
 *
 * monsoon_env_load_dev: for j < m, slot dst_dev[j] (NULL = j, and then m <= n) becomes entry src_dev[j] (NULL = j) of the
 * n_entries at entries_dev; m <= max_games.  A pair is skipped -- the slot and its views stay untouched -- when src is
 * outside [0, n_entries), dst is outside [0, n), or the entry's header does not match this library (magic, version, record
 * size) or its stream cursor is out of range.  loaded_dev[j] (DEVICE bytes, may be NULL) is set to 1 when pair j was
 * loaded and to 0 when it was skipped.  The same src may appear many times: that is the fork.  The same dst appearing
 * twice is the caller's error: which of the entries the slot ends up with, or which mixture of them, is unspecified.
 * After the call the views of every loaded slot read as after a step that ended nothing: obs, legal, obs_raises and
 * to_play of the restored state; done 0, reward 0, winner -2, truncated 0, fault 0, illegal 0, final_hash 0; episode = the
 * entry's count.  For a slot with a pending end they are what monsoon_env_reset / the step that started that episode left:
 * the views of the state the episode ended in.  Two launches.
 *
 * Both are asynchronous on the handle's stream: no allocation, host copy or synchronisation, so they capture into a graph
 * next to monsoon_env_step_dev.  MONSOON_ERR_STATE without a loaded env (all three calls); MONSOON_ERR_ARG for a NULL
 * entries_dev, one that is not 16-byte aligned, m < 0, n_entries < 0, m > n with NULL slots_dev / dst_dev, or a load with
 * m > max_games. */
int monsoon_env_entry_bytes(monsoon_t* h, int32_t* out);
int monsoon_env_save_dev(monsoon_t* h, void* entries_dev, const int32_t* slots_dev, int32_t m);
int monsoon_env_load_dev(monsoon_t* h, const void* entries_dev, int32_t n_entries, const int32_t* src_dev, const int32_t* dst_dev,
                         int32_t m, uint8_t* loaded_dev);

/* Determinized forks (information-set search).  An entry is the TRUE game: loaded as it is, a fork plays with the opponent's
 * hand and deck face up and with the game's own future draws, random picks and bot choices.  monsoon_env_load_determinized_dev
 * is monsoon_env_load_dev that draws again what an observer cannot see -- same arguments, same skipped pairs, same meaning
 * of loaded_dev, same views, same asynchrony (no allocation, host copy or synchronisation: it captures into a graph); three
 * launches.  Entries stay interchangeable with monsoon_env_load_dev, and monsoon_version() is the same.
 *
 * Pair j has the seed s = seeds_dev[j] and the observer O = observers_dev[j] (0 or 1: that side; 255: the side to move in
 * the entry's state; observers_dev NULL = 255 for every pair).  An observer byte other than 0, 1 or 255 skips the pair
 * (loaded 0, the slot and its views untouched).  An entry whose episode has ended or has its end pending is loaded
 * verbatim: nothing is left to search.  Otherwise, by `what`:
 *
 *  MONSOON_DET_STREAM (1), every record build.  The loaded slot's stream is numpy.random.RandomState(s): its raw state
 *    and its first two tempered blocks, the slot's stream cursor at block 0, word 0 -- what a new episode of seed s starts
 *    with.  Nothing else differs from monsoon_env_load_dev.
 *  MONSOON_DET_STREAM | MONSOON_DET_HAND (3), standard record only.  In addition the hand of the hidden side S = 1 - O is
 *    drawn again from its hand and deck.  Its hand entries, in record order, whose flags carry neither the alias flag nor
 *    the kept-strength flag (b305's returned object: the observer watched it return, it stays where it is) are the k
 *    movable places; with the d deck entries behind them they form A, L = k + d long.  For i = 0 .. k-1:
 *    r = hash32(s, i, 0xD7) (monsoon_amd/fitness.py hash32), j = i + ((r * (L - i)) >> 32), swap A[i], A[j]; then A is
 *    written back to the same places.  The 4-byte entries {card, cost, flags, x} move whole; the two counts and the
 *    twelve age bytes stay (an age belongs to its deck position).  The hand becomes a uniformly chosen k-subset of the
 *    hidden cards in uniform order -- uniform, not weighted by the draw's ages, which the observer does not know
 *    (DESIGN.md §9).  k = 0 or L <= 1 changes nothing.  monsoon_amd.vec_env.determinize_order recomputes the permutation.
 *    What O sees -- its own block, the board, mana, bases, the last plays -- is the entry's: the observation of a slot
 *    loaded with O = 255 is the one monsoon_env_load_dev gives.
 *
 * MONSOON_ERR_ARG in addition to monsoon_env_load_dev's cases: seeds_dev NULL; what outside {1, 3}; MONSOON_DET_HAND on the
 * extended or the large build (the message names the standard record). */
#define MONSOON_DET_STREAM 1
#define MONSOON_DET_HAND 2
int monsoon_env_load_determinized_dev(monsoon_t* h, const void* entries_dev, int32_t n_entries, const int32_t* src_dev,
                                      const int32_t* dst_dev, int32_t m, const uint32_t* seeds_dev /* DEVICE uint32[m] */,
                                      const uint8_t* observers_dev /* DEVICE uint8[m]; NULL = 255 for all */, int32_t what,
                                      uint8_t* loaded_dev);

#ifdef __cplusplus
}
#endif
#endif /* MONSOON_H */
