// Host check of the device log of monsoon_rollout_explore (monsoon_amd/csrc/host_layout.h explore_log, explore_entry_bytes,
// log_batch_cap), built with the address and UB sanitizers by tests/test_rollout_explore_cpu.py.  Never loaded into Python.
// For every choice of the five optional arrays, at caps 1, 63, 64, 65, 2 048, 65 536 and max_turns 1, 40, 200: every field
// is aligned to its element type, the fields are disjoint and inside the total, an array not asked for takes no room, the
// total is entries x explore_entry_bytes, and with nothing but the three arrays of monsoon_rollout_logged the layout is
// rollout_log's.  Batch cap: the formula of include/monsoon.h, and its log fits the budget wherever one game does.
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

int main() {
  using namespace layout;
  const size_t BUDGET = (size_t)256 << 20;
  long n_layouts = 0, n_caps = 0;
  for (size_t cap : {(size_t)1, (size_t)63, (size_t)64, (size_t)65, (size_t)2048, (size_t)65536})
    for (size_t max_turns : {(size_t)1, (size_t)40, (size_t)200})
      for (int flags = 0; flags < 32; flags++) {
        const size_t n = cap * max_turns;
        const bool sc = flags & 1, nl = flags & 2, gr = flags & 4, xp = flags & 8, ts = flags & 16;
        const ExploreLog l = explore_log(n, sc, nl, gr, xp, ts);
        const size_t per = explore_entry_bytes(sc, nl, gr, xp, ts);
        EXPECT(per == (size_t)(1 + (sc ? 8 : 0) + (nl ? 2 : 0) + (gr ? 1 : 0) + (xp ? 1 : 0) + (ts ? 8 : 0)), per, flags);
        EXPECT(l.total == n * per, l.total, n * per);
        std::vector<Field> f = {{l.action, 1, n}};
        if (sc) f.push_back({l.score, 8, 8 * n});
        if (ts) f.push_back({l.taken_score, 8, 8 * n});
        if (nl) f.push_back({l.n_legal, 2, 2 * n});
        if (gr) f.push_back({l.greedy, 1, n});
        if (xp) f.push_back({l.explored, 1, n});
        EXPECT(sc || l.score == NONE, l.score, 0);
        EXPECT(ts || l.taken_score == NONE, l.taken_score, 0);
        EXPECT(nl || l.n_legal == NONE, l.n_legal, 0);
        EXPECT(gr || l.greedy == NONE, l.greedy, 0);
        EXPECT(xp || l.explored == NONE, l.explored, 0);
        check_fields(f, l.total);
        if (!gr && !xp && !ts) {   // the logged call's three arrays alone: its layout
          const RolloutLog r = rollout_log(n, sc, nl);
          EXPECT(r.score == l.score && r.n_legal == l.n_legal && r.action == l.action && r.total == l.total, r.total, l.total);
        }
        n_layouts++;
      }
  EXPECT(explore_entry_bytes(true, true, true, true, true) == 21 && explore_entry_bytes(true, true, false, false, false) == 11, 0, 0);
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
