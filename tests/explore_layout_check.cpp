// Host check of the device log of the logged rollouts (monsoon_amd/csrc/host_layout.h LOG_COLUMN, log_layout, log_entry_bytes,
// log_batch_cap), built with the address and UB sanitizers by tests/test_rollout_explore_cpu.py.  Never loaded into Python.
// For every choice of the seven optional columns, at caps 1, 63, 64, 65, 2 048, 65 536 and max_turns 1, 40, 200: every
// column is aligned to its element type, the columns are disjoint and inside the total, a column not asked for takes no
// room, and the total is entries x log_entry_bytes.  The layouts the one table replaced are restated here as they were
// written -- monsoon_rollout_logged's three arrays, monsoon_rollout_explore's six, monsoon_rollout_sample's eight -- and every
// mask within each gives those offsets.  Batch cap: the formula of include/monsoon.h, and its log fits the budget wherever
// one game does.
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>

#include <algorithm>
#include <vector>

#include "host_layout.h"

static void fail(const char* what, size_t a, size_t b) {
  printf("FAIL %s (%zu, %zu)\n", what, a, b);
  exit(1);
}
#define EXPECT(cond, a, b) \
  do {                     \
    if (!(cond)) fail(#cond, (size_t)(a), (size_t)(b)); \
  } while (0)

struct Field {
  size_t off, elem, bytes;
};
static void check_fields(std::vector<Field> f, size_t total) {
  for (const Field& x : f) {
    EXPECT(x.off % x.elem == 0, x.off, x.elem);
    EXPECT(x.off + x.bytes <= total, x.off + x.bytes, total);
  }
  std::sort(f.begin(), f.end(), [](const Field& a, const Field& b) { return a.off < b.off; });
  for (size_t i = 1; i < f.size(); i++) EXPECT(f[i - 1].off + f[i - 1].bytes <= f[i].off, f[i - 1].off + f[i - 1].bytes, f[i].off);
}

// The layouts as they were written before the table, field by field (expected values: nothing here calls log_layout).
struct Old {
  size_t score, taken_score, weight_total, taken_weight, n_legal, action, greedy, explored, total;
};
static const size_t NO = ~(size_t)0;
static Old former_logged(size_t entries, bool score, bool n_legal) {
  Old l = {NO, NO, NO, NO, NO, NO, NO, NO, 0};
  l.score = score ? 0 : NO;
  const size_t after_score = score ? entries * 8 : 0;
  l.n_legal = n_legal ? after_score : NO;
  l.action = after_score + (n_legal ? entries * 2 : 0);
  l.total = l.action + entries;
  return l;
}
static Old former_sampling(size_t entries, bool score, bool n_legal, bool greedy, bool explored, bool taken_score, bool weight_total,
                          bool taken_weight) {
  Old l;
  size_t at = 0;
  const auto field = [&](bool on, size_t bytes) {
    const size_t off = on ? at : NO;
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
static Old former_exploring(size_t entries, bool score, bool n_legal, bool greedy, bool explored, bool taken_score) {
  Old l = {NO, NO, NO, NO, NO, NO, NO, NO, 0};
  size_t at = 0;
  const auto field = [&](bool on, size_t bytes) {
    const size_t off = on ? at : NO;
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
static void expect_same(const layout::Log& l, const Old& o, int flags) {
  using namespace layout;
  EXPECT(l.at[LOG_SCORE] == o.score && l.at[LOG_TAKEN_SCORE] == o.taken_score, flags, 0);
  EXPECT(l.at[LOG_WEIGHT_TOTAL] == o.weight_total && l.at[LOG_TAKEN_WEIGHT] == o.taken_weight, flags, 1);
  EXPECT(l.at[LOG_N_LEGAL] == o.n_legal && l.at[LOG_ACTION] == o.action, flags, 2);
  EXPECT(l.at[LOG_GREEDY] == o.greedy && l.at[LOG_EXPLORED] == o.explored && l.total == o.total, flags, 3);
}

int main() {
  using namespace layout;
  const size_t BUDGET = (size_t)256 << 20;
  long n_layouts = 0, n_caps = 0;
  EXPECT(NONE == NO && LOG_COLUMNS == 8, NONE, LOG_COLUMNS);
  // the table itself: element sizes fall, and the padding bytes are what include/monsoon.h promises behind a game's last step
  for (int c = 1; c < LOG_COLUMNS; c++) EXPECT(LOG_COLUMN[c].bytes <= LOG_COLUMN[c - 1].bytes, c, LOG_COLUMN[c].bytes);
  const size_t elem[LOG_COLUMNS] = {8, 8, 4, 4, 2, 1, 1, 1};
  const int fill[LOG_COLUMNS] = {0xFF, 0xFF, 0, 0, 0, 0xFF, 0xFF, 0};
  for (int c = 0; c < LOG_COLUMNS; c++) EXPECT(LOG_COLUMN[c].bytes == elem[c] && LOG_COLUMN[c].fill == fill[c], c, LOG_COLUMN[c].bytes);
  for (size_t cap : {(size_t)1, (size_t)63, (size_t)64, (size_t)65, (size_t)2048, (size_t)65536})
    for (size_t max_turns : {(size_t)1, (size_t)40, (size_t)200})
      for (int flags = 0; flags < 128; flags++) {
        const size_t n = cap * max_turns;
        const bool sc = flags & 1, nl = flags & 2, gr = flags & 4, xp = flags & 8, ts = flags & 16, wt = flags & 32, tw = flags & 64;
        const unsigned mask = (sc ? log_bit(LOG_SCORE) : 0) | (nl ? log_bit(LOG_N_LEGAL) : 0) | (gr ? log_bit(LOG_GREEDY) : 0) |
                              (xp ? log_bit(LOG_EXPLORED) : 0) | (ts ? log_bit(LOG_TAKEN_SCORE) : 0) | (wt ? log_bit(LOG_WEIGHT_TOTAL) : 0) |
                              (tw ? log_bit(LOG_TAKEN_WEIGHT) : 0);
        const Log l = log_layout(n, mask);
        const size_t per = log_entry_bytes(mask);
        EXPECT(per == (size_t)(1 + (sc ? 8 : 0) + (nl ? 2 : 0) + (gr ? 1 : 0) + (xp ? 1 : 0) + (ts ? 8 : 0) + (wt ? 4 : 0) + (tw ? 4 : 0)), per, flags);
        EXPECT(per == log_entry_bytes(mask | log_bit(LOG_ACTION)), per, flags);   // action is always on, asked for or not
        EXPECT(l.total == n * per, l.total, n * per);
        std::vector<Field> f;
        for (int c = 0; c < LOG_COLUMNS; c++) {
          const bool on = c == LOG_ACTION || (mask >> c & 1u);
          if (on) f.push_back({l.at[c], elem[c], elem[c] * n});
          EXPECT(on ? l.at[c] != NONE : l.at[c] == NONE, c, l.at[c]);
        }
        check_fields(f, l.total);
        expect_same(l, former_sampling(n, sc, nl, gr, xp, ts, wt, tw), flags);
        if (!wt && !tw) expect_same(l, former_exploring(n, sc, nl, gr, xp, ts), flags);   // the exploring call's six arrays alone: its layout
        if (!wt && !tw && !gr && !xp && !ts) {                                           // the logged call's three arrays alone: its layout
          const Old r = former_logged(n, sc, nl);
          expect_same(l, r, flags);
          EXPECT(r.score == (sc ? 0 : NO) && r.n_legal == (nl ? (sc ? 8 * n : 0) : NO) && r.action == (sc ? 8 * n : 0) + (nl ? 2 * n : 0), flags, n);
        }
        n_layouts++;
      }
  const unsigned LOGGED = log_bit(LOG_SCORE) | log_bit(LOG_N_LEGAL), EXPLORE = LOGGED | log_bit(LOG_GREEDY) | log_bit(LOG_EXPLORED) | log_bit(LOG_TAKEN_SCORE);
  static_assert(log_entry_bytes(0) == 1 && log_entry_bytes(~0u) == 29, "entry bytes are a constant expression");
  EXPECT(log_entry_bytes(EXPLORE) == 21 && log_entry_bytes(LOGGED) == 11, 0, 0);
  EXPECT(log_entry_bytes(EXPLORE | log_bit(LOG_WEIGHT_TOTAL) | log_bit(LOG_TAKEN_WEIGHT)) == 29 && log_entry_bytes(0) == 1, 0, 0);
  for (size_t max_games : {(size_t)1, (size_t)64, (size_t)1024, (size_t)65536})
    for (size_t max_turns : {(size_t)1, (size_t)200, (size_t)30000})
      for (size_t per : {(size_t)1, (size_t)11, (size_t)13, (size_t)21}) {
        const size_t cap = log_batch_cap(max_games, BUDGET, per, max_turns);
        EXPECT(cap == std::min(max_games, std::max<size_t>(1, BUDGET / (per * max_turns))), cap, max_games);
        EXPECT(cap >= 1 && cap <= max_games, cap, max_games);
        EXPECT(cap * per * max_turns <= BUDGET, cap * per * max_turns, BUDGET);   // (one game always fits: 21 x 30 000 bytes)
        n_caps++;
      }
  // the figures the header and the tests quote
  EXPECT(log_batch_cap(1024, BUDGET, 11, 30000) == 813, 0, 0);       // monsoon_rollout_logged's cut
  EXPECT(log_batch_cap(1024, BUDGET, 21, 30000) == 426, 0, 0);       // every array of the exploring call
  EXPECT(log_batch_cap(65536, BUDGET, 21, 200) == 63913, 0, 0);      // at max_turns 200 the full log binds just below 65 536 games
  printf("ok %ld layouts %ld caps\n", n_layouts, n_caps);
  return 0;
}
