// How the host side cuts its device workspaces into fields: one function per workspace, byte offsets and a total for the
// sizes it is given (plain C++, checked by tests/host_layout_check.cpp).  Whoever sets a pointer into a workspace or reads
// one back goes through these; the constants of the kernels' headers are passed in.
#pragma once
#include <stddef.h>

namespace layout {

// d_env, the vector env's per-slot rows for `cap` slots
struct Env {
  size_t seed0 = 0;      // u32 [cap]
  size_t episode;        // i32 [cap]
  size_t agent_steps;    // u32 [cap]
  size_t bot_steps;      // u32 [cap]
  size_t decks;          // u8 [cap][24]
  size_t factions;       // u8 [cap][2]
  size_t mark;           // u8 [cap]
  size_t pool;           // u8 [128]
  size_t snap_flag;      // u8 [cap]: the loaded flags of a load whose caller keeps none
  size_t total;
};
inline Env env(size_t cap) {
  Env l;
  l.episode = l.seed0 + 4 * cap;
  l.agent_steps = l.episode + 4 * cap;
  l.bot_steps = l.agent_steps + 4 * cap;
  l.decks = l.bot_steps + 4 * cap;
  l.factions = l.decks + 24 * cap;
  l.mark = l.factions + 2 * cap;
  l.pool = l.mark + cap;
  l.snap_flag = l.pool + 128;
  l.total = l.snap_flag + 2 * cap;   // (one spare byte per slot behind the flags)
  return l;
}

// d_opp, the env's heuristic opponent: `count` and `pop`, the end of the block, are cleared as one range
struct Opp {
  size_t rows = 0;       // i32 [cap]: weight row per slot
  size_t list;           // i32 [2][cap]: slot lists
  size_t lookahead;      // u32 [cap]: look-ahead transitions
  size_t count;          // i32 [2 * count_stride]: list lengths
  size_t pop;            // i32 [2][pop_parts * pop_stride]: pop counters
  size_t total;
};
inline Opp opp(size_t cap, size_t count_stride, size_t pop_parts, size_t pop_stride) {
  Opp l;
  l.list = l.rows + 4 * cap;
  l.lookahead = l.list + 8 * cap;
  l.count = l.lookahead + 4 * cap;
  l.pop = l.count + 4 * 2 * count_stride;
  l.total = l.pop + 4 * 2 * pop_parts * pop_stride;
  return l;
}

// d_bytes, the staging buffer of the small API calls: one allocation, cut anew by every call that uses it
constexpr size_t BYTES_MIN = 16384;
inline size_t bytes_total(size_t cap) { return 8 * cap > BYTES_MIN ? 8 * cap : BYTES_MIN; }
struct Step { size_t actions = 0, reward, done, fault, illegal, total; };   // u8 / i8 [n] each; reward..fault come back in one copy
inline Step step(size_t n) { return {0, n, 2 * n, 3 * n, 4 * n, 5 * n}; }
struct Expert { size_t action = 0, fault, total; };                          // u8 [n] each
inline Expert expert(size_t n) { return {0, n, 2 * n}; }
struct Export { size_t buf = 0, len, total; };                               // u8 [2048] | i32
constexpr Export state_export() { return {0, 2048, 2048 + 4}; }
constexpr size_t DEBUG_STREAM_MAX = 3000;
struct Debug { size_t stream = 0, out, out_words, total; };                  // i32 [3000] | fault, n, trace i32 [trace_cap][2]
inline Debug debug(size_t trace_cap) { return {0, DEBUG_STREAM_MAX * 4, 2 + 2 * trace_cap, DEBUG_STREAM_MAX * 4 + (2 + 2 * trace_cap) * 4}; }
// the state blob (k_blob): magic, record size | meta row | record | stream state | tempered outputs
constexpr size_t blob_bytes(size_t meta_bytes, size_t state_bytes, size_t mt_n) { return 8 + meta_bytes + state_bytes + mt_n * 4 + 2 * mt_n * 4; }

// monsoon_ga_offspring's one allocation
struct GaOffspring {
  size_t key = 0;        // u32 [mt_n]
  size_t pos_gauss;      // i32 [2]: position, has_gauss
  size_t gauss;          // f64
  size_t parents_w, parents_s;   // f64 [mu][dim] each
  size_t out_w, out_s;           // f64 [lambda][dim] each
  size_t parent;         // i32 [lambda]
  size_t tries;          // i64 [lambda]
  size_t parents_bytes, out_bytes, total;
};
inline GaOffspring ga_offspring(size_t mu, size_t dim, size_t lambda, size_t mt_n) {
  GaOffspring l;
  l.parents_bytes = mu * dim * 8;
  l.out_bytes = lambda * dim * 8;
  l.pos_gauss = l.key + mt_n * 4;
  l.gauss = l.pos_gauss + 8;
  l.parents_w = l.gauss + 8;
  l.parents_s = l.parents_w + l.parents_bytes;
  l.out_w = l.parents_s + l.parents_bytes;
  l.out_s = l.out_w + l.out_bytes;
  l.parent = l.out_s + l.out_bytes;
  l.tries = (l.parent + lambda * 4 + 7) & ~(size_t)7;
  l.total = l.tries + lambda * 8;
  return l;
}

// d_log, the device log of one rollout batch: `entries` = games x max_turns per array; an array the caller does not ask
// for takes no room (its offset is NONE)
constexpr size_t NONE = ~(size_t)0;
struct RolloutLog { size_t score, n_legal, action, total; };                 // f64 | i16 | u8, [entries] each
inline RolloutLog rollout_log(size_t entries, bool score, bool n_legal) {
  RolloutLog l;
  l.score = score ? 0 : NONE;
  const size_t after_score = score ? entries * 8 : 0;
  l.n_legal = n_legal ? after_score : NONE;
  l.action = after_score + (n_legal ? entries * 2 : 0);
  l.total = l.action + entries;
  return l;
}

// d_log of monsoon_rollout_explore: the same three arrays, then the three the exploring kernel adds, the 8-byte ones
// first; an array the caller does not ask for takes no room.  explore_entry_bytes is what one entry takes (1 .. 21), the
// figure the call's batch cap is cut by.
struct ExploreLog { size_t score, taken_score, n_legal, action, greedy, explored, total; };   // f64 | f64 | i16 | u8 | u8 | u8, [entries] each
constexpr size_t explore_entry_bytes(bool score, bool n_legal, bool greedy, bool explored, bool taken_score) {
  return 1 + (score ? 8 : 0) + (n_legal ? 2 : 0) + (greedy ? 1 : 0) + (explored ? 1 : 0) + (taken_score ? 8 : 0);
}
inline ExploreLog explore_log(size_t entries, bool score, bool n_legal, bool greedy, bool explored, bool taken_score) {
  ExploreLog l;
  size_t at = 0;
  const auto field = [&](bool on, size_t bytes) {
    const size_t off = on ? at : NONE;
    if (on) at += entries * bytes;
    return off;
  };
  l.score = field(score, 8);
  l.taken_score = field(taken_score, 8);
  l.n_legal = field(n_legal, 2);
  l.action = field(true, 1);
  l.greedy = field(greedy, 1);
  l.explored = field(explored, 1);
  l.total = at;
  return l;
}
// d_log of monsoon_rollout_sample: the exploring call's arrays and the two the sampling kernel adds, by falling element
// size; an array the caller does not ask for takes no room.  sample_entry_bytes is what one entry takes (1 .. 29).
struct SampleLog { size_t score, taken_score, weight_total, taken_weight, n_legal, action, greedy, explored, total; };   // f64 | f64 | u32 | u32 | i16 | u8 | u8 | u8
constexpr size_t sample_entry_bytes(bool score, bool n_legal, bool greedy, bool explored, bool taken_score, bool weight_total, bool taken_weight) {
  return explore_entry_bytes(score, n_legal, greedy, explored, taken_score) + (weight_total ? 4 : 0) + (taken_weight ? 4 : 0);
}
inline SampleLog sample_log(size_t entries, bool score, bool n_legal, bool greedy, bool explored, bool taken_score, bool weight_total,
                            bool taken_weight) {
  SampleLog l;
  size_t at = 0;
  const auto field = [&](bool on, size_t bytes) {
    const size_t off = on ? at : NONE;
    if (on) at += entries * bytes;
    return off;
  };
  l.score = field(score, 8);
  l.taken_score = field(taken_score, 8);
  l.weight_total = field(weight_total, 4);
  l.taken_weight = field(taken_weight, 4);
  l.n_legal = field(n_legal, 2);
  l.action = field(true, 1);
  l.greedy = field(greedy, 1);
  l.explored = field(explored, 1);
  l.total = at;
  return l;
}
// games per batch of a logged call: as many as `budget` bytes of device log hold, one at least, max_games at most
constexpr size_t log_batch_cap(size_t max_games, size_t budget, size_t entry_bytes, size_t max_turns) {
  return budget / (entry_bytes * max_turns) < 1 ? 1 : budget / (entry_bytes * max_turns) < max_games ? budget / (entry_bytes * max_turns) : max_games;
}

// d_replay, what one batch of monsoon_replay_logged_dev takes to the device and brings back: `games` games, `entries` =
// games x log_stride; without a keep mask its array takes no room (NONE).  status .. fault come back in three copies.
struct Replay { size_t base = 0, steps, replayed, action, keep, status, fault, total; };   // i64 | i32 | i32 [games], u8 | u8 [entries], u8 | u8 [games]
inline Replay replay(size_t games, size_t entries, bool keep) {
  Replay l;
  l.steps = l.base + 8 * games;
  l.replayed = l.steps + 4 * games;
  l.action = l.replayed + 4 * games;
  l.keep = keep ? l.action + entries : NONE;
  l.status = l.action + (keep ? 2 : 1) * entries;
  l.fault = l.status + games;
  l.total = l.fault + games;
  return l;
}

// d_results of a rollout: results, then fault codes (monsoon_rollout_faults)
struct Results { size_t result = 0, fault, total; };                         // i8 [cap] | u8 [cap]
inline Results results(size_t cap) { return {0, cap, 2 * cap}; }

}  // namespace layout
