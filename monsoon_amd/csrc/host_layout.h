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

// d_log, the device log of one batch of a logged rollout (monsoon_rollout_logged / _explore / _sample): one array of
// `entries` = games x max_turns elements per column the caller asks for, in the order of this table -- by falling element
// size, so every array is aligned to its element whatever the entry count.  `fill` is the byte the array is set to before
// the launch: what an entry behind a game's last step reads, and a bot step in the columns the bot does not write.
enum LogColumn { LOG_SCORE, LOG_TAKEN_SCORE, LOG_WEIGHT_TOTAL, LOG_TAKEN_WEIGHT, LOG_N_LEGAL, LOG_ACTION, LOG_GREEDY, LOG_EXPLORED, LOG_COLUMNS };
struct LogColumnInfo { size_t bytes; int fill; };
constexpr LogColumnInfo LOG_COLUMN[LOG_COLUMNS] = {
    {8, 0xFF},   // score         f64  NaN (all ones)
    {8, 0xFF},   // taken_score   f64  NaN
    {4, 0},      // weight_total  u32
    {4, 0},      // taken_weight  u32
    {2, 0},      // n_legal       i16
    {1, 0xFF},   // action        u8   255; always present
    {1, 0xFF},   // greedy        u8   255
    {1, 0},      // explored      u8
};
constexpr unsigned log_bit(LogColumn c) { return 1u << c; }
// what one entry takes: the columns of `mask` and action (1 .. 29 bytes), the figure a call's batch cap is cut by
constexpr size_t log_entry_bytes(unsigned mask) {
  size_t bytes = 0;
  for (int c = 0; c < LOG_COLUMNS; c++)
    if ((mask | log_bit(LOG_ACTION)) >> c & 1u) bytes += LOG_COLUMN[c].bytes;
  return bytes;
}
constexpr size_t NONE = ~(size_t)0;
struct Log { size_t at[LOG_COLUMNS], total; };   // a column that is not asked for takes no room: its offset is NONE
inline Log log_layout(size_t entries, unsigned mask) {
  Log l;
  l.total = 0;
  for (int c = 0; c < LOG_COLUMNS; c++) {
    const bool on = (mask | log_bit(LOG_ACTION)) >> c & 1u;
    l.at[c] = on ? l.total : NONE;
    if (on) l.total += entries * LOG_COLUMN[c].bytes;
  }
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
