// Host check of the library's workspace layouts (monsoon_amd/csrc/host_layout.h) and of the owner of its device memory
// (host_mem.h), built with the address and UB sanitizers by tests/test_host_layout_cpu.py, once per record build
// (-DMSB_EXT=0/1/2: state.h gives that build's record size).  Never loaded into Python.
//
// Layouts: for every cap below, every field is aligned to its element type, the fields are disjoint and inside the total,
// and the totals are the formulas the allocations have always used.  Owner: a counting allocator that fails the k-th
// allocation, for every k of a sequence shaped like a handle's life; the allocator aborts on a block freed twice or never
// allocated, and whatever is still live at the end is a failure (the sanitizers' leak check sees the same blocks).
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>

#include <algorithm>
#include <set>
#include <vector>

#define HOST_MEM_ALLOCATOR
static std::set<void*> g_live;
static long g_allocs = 0, g_frees = 0, g_fail_at = 0;   // g_fail_at = k: the k-th allocation from now fails (0 = none)
static int host_mem_alloc(void** p, size_t bytes) {
  if (g_fail_at && --g_fail_at == 0) return 2;   // (the runtime's out-of-memory code)
  *p = malloc(bytes ? bytes : 1);
  g_live.insert(*p);
  g_allocs++;
  return 0;
}
static int host_mem_free(void* p) {
  if (!g_live.erase(p)) {
    printf("FAIL free of a block that is not live: %p\n", p);
    abort();
  }
  free(p);
  g_frees++;
  return 0;
}
#include "host_layout.h"
#include "host_mem.h"
#include "mt19937.h"
#include "state.h"

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
// aligned to the element type, disjoint, inside the total
static void check_fields(std::vector<Field> f, size_t total) {
  for (const Field& x : f) {
    EXPECT(x.off % x.elem == 0, x.off, x.elem);
    EXPECT(x.off + x.bytes <= total, x.off + x.bytes, total);
  }
  std::sort(f.begin(), f.end(), [](const Field& a, const Field& b) { return a.off < b.off; });
  for (size_t i = 1; i < f.size(); i++) EXPECT(f[i - 1].off + f[i - 1].bytes <= f[i].off, f[i - 1].off + f[i - 1].bytes, f[i].off);
}

// The kernels' constants the layouts are handed (env.h ENV_COUNT_STRIDE, kernels.h POP_PARTS / POP_STRIDE and
// sizeof(GameMeta), monsoon_hip.hip DBG_TRACE_CAP): those headers need the HIP compiler, so they are restated here.
static const size_t K_ENV_COUNT_STRIDE = 32, K_POP_PARTS = 8, K_POP_STRIDE = 32, K_DBG_TRACE_CAP = 256, K_META_BYTES = 32;

static long n_layouts = 0;
static void check_layouts(size_t cap) {
  using namespace layout;
  const size_t blob = blob_bytes(K_META_BYTES, msb::STATE_BYTES, msb::MT_N);
  {
    const Env l = env(cap);
    EXPECT(l.total == 45 * cap + 128, l.total, cap);
    check_fields({{l.seed0, 4, 4 * cap}, {l.episode, 4, 4 * cap}, {l.agent_steps, 4, 4 * cap}, {l.bot_steps, 4, 4 * cap}, {l.decks, 1, 24 * cap},
                  {l.factions, 1, 2 * cap}, {l.mark, 1, cap}, {l.pool, 1, 128}, {l.snap_flag, 1, cap}},
                 l.total);
    n_layouts++;
  }
  {
    const Opp l = opp(cap, K_ENV_COUNT_STRIDE, K_POP_PARTS, K_POP_STRIDE);
    EXPECT(l.total == 16 * cap + 4 * (2 * K_ENV_COUNT_STRIDE + 2 * K_POP_PARTS * K_POP_STRIDE), l.total, cap);
    EXPECT(l.pop + 4 * 2 * K_POP_PARTS * K_POP_STRIDE == l.total, l.pop, l.total);   // count and pop end the block: cleared as one range
    check_fields({{l.rows, 4, 4 * cap}, {l.list, 4, 8 * cap}, {l.lookahead, 4, 4 * cap}, {l.count, 4, 4 * 2 * K_ENV_COUNT_STRIDE},
                  {l.pop, 4, 4 * 2 * K_POP_PARTS * K_POP_STRIDE}},
                 l.total);
    n_layouts++;
  }
  {   // d_bytes: every use fits, with all `cap` games loaded where the use is per game
    const size_t total = bytes_total(cap);
    EXPECT(total == std::max<size_t>(8 * cap, 16384), total, cap);
    const Step s = step(cap);
    EXPECT(s.total <= total, s.total, total);
    check_fields({{s.actions, 1, cap}, {s.reward, 1, cap}, {s.done, 1, cap}, {s.fault, 1, cap}, {s.illegal, 1, cap}}, s.total);
    const Expert e = expert(cap);
    EXPECT(e.total <= total, e.total, total);
    check_fields({{e.action, 1, cap}, {e.fault, 1, cap}}, e.total);
    const Export x = state_export();
    EXPECT(x.total <= total, x.total, total);
    check_fields({{x.buf, 1, 2048}, {x.len, 4, 4}}, x.total);
    const Debug d = debug(K_DBG_TRACE_CAP);
    EXPECT(d.total <= total, d.total, total);
    check_fields({{d.stream, 4, DEBUG_STREAM_MAX * 4}, {d.out, 4, d.out_words * 4}}, d.total);
    EXPECT(d.out_words == 2 + 2 * K_DBG_TRACE_CAP, d.out_words, 0);
    EXPECT(blob <= total && blob % 4 == 0, blob, total);
    n_layouts += 5;
  }
  {
    const Results l = results(cap);
    EXPECT(l.total == 2 * cap, l.total, cap);
    check_fields({{l.result, 1, cap}, {l.fault, 1, cap}}, l.total);
    n_layouts++;
  }
  for (size_t max_turns : {(size_t)1, (size_t)40})
    for (int flags = 0; flags < 4; flags++) {
      const size_t n = cap * max_turns;
      const bool sc = flags & 1, nl = flags & 2;
      const Log l = log_layout(n, (sc ? log_bit(LOG_SCORE) : 0) | (nl ? log_bit(LOG_N_LEGAL) : 0));   // monsoon_rollout_logged's three arrays
      EXPECT(l.total == n * ((sc ? 8 : 0) + (nl ? 2 : 0) + 1), l.total, n);
      std::vector<Field> f = {{l.at[LOG_ACTION], 1, n}};
      if (sc) f.push_back({l.at[LOG_SCORE], 8, 8 * n});
      if (nl) f.push_back({l.at[LOG_N_LEGAL], 2, 2 * n});
      EXPECT(sc || l.at[LOG_SCORE] == NONE, l.at[LOG_SCORE], 0);
      EXPECT(nl || l.at[LOG_N_LEGAL] == NONE, l.at[LOG_N_LEGAL], 0);
      // score at 0, n_legal behind it, action behind that; no other column
      EXPECT(l.at[LOG_SCORE] == (sc ? 0 : NONE) && l.at[LOG_N_LEGAL] == (nl ? (sc ? 8 * n : 0) : NONE), l.at[LOG_N_LEGAL], n);
      EXPECT(l.at[LOG_ACTION] == (sc ? 8 * n : 0) + (nl ? 2 * n : 0) && l.total == l.at[LOG_ACTION] + n, l.at[LOG_ACTION], n);
      for (int c : {LOG_TAKEN_SCORE, LOG_WEIGHT_TOTAL, LOG_TAKEN_WEIGHT, LOG_GREEDY, LOG_EXPLORED}) EXPECT(l.at[c] == NONE, c, l.at[c]);
      check_fields(f, l.total);
      n_layouts++;
    }
}

static void check_ga_offspring() {
  const size_t N = msb::MT_N;
  for (size_t dim : {(size_t)1, (size_t)10, (size_t)16})
    for (size_t lambda : {(size_t)1, (size_t)3, (size_t)7, (size_t)101, (size_t)4})
      for (size_t mu : {(size_t)1, (size_t)5}) {
        const layout::GaOffspring l = layout::ga_offspring(mu, dim, lambda, N);
        // the packing monsoon_ga_offspring has always used
        const size_t pb = mu * dim * 8, ob = lambda * dim * 8;
        const size_t o_pg = N * 4, o_g = o_pg + 8, o_pw = o_g + 8, o_ps = o_pw + pb, o_ow = o_ps + pb, o_os = o_ow + ob, o_par = o_os + ob,
                     o_tr = (o_par + lambda * 4 + 7) & ~(size_t)7, total = o_tr + lambda * 8;
        EXPECT(l.key == 0 && l.pos_gauss == o_pg && l.gauss == o_g && l.parents_w == o_pw && l.parents_s == o_ps, dim, lambda);
        EXPECT(l.out_w == o_ow && l.out_s == o_os && l.parent == o_par && l.tries == o_tr && l.total == total, dim, lambda);
        EXPECT(l.parents_bytes == pb && l.out_bytes == ob, pb, ob);
        check_fields({{l.key, 4, N * 4}, {l.pos_gauss, 4, 8}, {l.gauss, 8, 8}, {l.parents_w, 8, pb}, {l.parents_s, 8, pb}, {l.out_w, 8, ob},
                      {l.out_s, 8, ob}, {l.parent, 4, lambda * 4}, {l.tries, 8, lambda * 8}},
                     l.total);
        n_layouts++;
      }
}

// A handle's life in small: create-time blocks, lazily allocated ones, both grow policies twice, a call with temporaries
// of its own, one that hands its block over.  Returns the allocations it asked for; stops at the first failure like
// HIP_TRY does.  What must hold whichever allocation failed is checked on the way.
namespace {
struct Life {
  DevOwner mem;
  uint8_t* fixed[4] = {};
  double* weights = nullptr;
  int weights_cap = 0;
  uint32_t* ovf = nullptr;
  size_t ovf_lanes = 0;
  uint32_t* table = nullptr;
};
}  // namespace
static int live_life(Life& h, long* asked, long* frees_before_destroy) {
#define TRY(call)          \
  do {                     \
    (*asked)++;            \
    if (int e_ = (call)) return e_; \
  } while (0)
  const long frees0 = g_frees;
  long expect_frees = 0;
  for (int i = 0; i < 4; i++) TRY(h.mem.alloc(&h.fixed[i], 100 + i));
  TRY(h.mem.grow(h.ovf, h.ovf_lanes, (size_t)64, 64 * 4, Grow::Retire));
  for (int rows : {4, 2, 9}) {   // replace: 2 asks for nothing
    double* const old = h.weights;
    const int old_cap = h.weights_cap;
    if (rows > old_cap) {
      (*asked)++;
      expect_frees += old ? 1 : 0;
    }
    if (int e = h.mem.grow(h.weights, h.weights_cap, rows, (size_t)rows * 80, Grow::Replace)) {
      EXPECT(h.weights == nullptr && h.weights_cap == 0, old_cap, rows);   // a failed replace: null, capacity 0
      return e;
    }
    EXPECT(h.weights != nullptr && h.weights_cap == std::max(rows, old_cap), h.weights_cap, rows);
    EXPECT(rows > old_cap || h.weights == old, rows, old_cap);
  }
  for (size_t lanes : {(size_t)32, (size_t)128, (size_t)512}) {   // retire: 32 asks for nothing
    uint32_t* const old = h.ovf;
    const size_t old_lanes = h.ovf_lanes;
    if (lanes > old_lanes) (*asked)++;
    if (int e = h.mem.grow(h.ovf, h.ovf_lanes, lanes, lanes * 4, Grow::Retire)) {
      EXPECT(h.ovf == old && h.ovf_lanes == old_lanes, lanes, old_lanes);   // a failed retire: the old block stays in use
      EXPECT(g_live.count(old) == 1, lanes, 0);
      return e;
    }
    EXPECT(g_live.count(old) == 1, lanes, 0);   // ... and a retired block stays alive
    if (lanes > old_lanes) old[0] = 0xC0FFEEu;  // (a captured launch may still write to it)
  }
  {   // a call with temporaries of its own: all gone when it returns, on every path
    const size_t live0 = g_live.size();
    int e = [&]() -> int {
      DevOwner tmp;
      void *a = nullptr, *b = nullptr, *c = nullptr;
      TRY(tmp.alloc(&a, 10));
      TRY(tmp.alloc(&b, 20));
      TRY(tmp.alloc(&c, 30));
      return 0;
    }();
    EXPECT(g_live.size() == live0, g_live.size(), live0);
    expect_frees += e ? 0 : 3;
    if (e) {
      *frees_before_destroy = -1;   // (how many temporaries existed depends on k: not counted)
      return e;
    }
  }
  {   // a call that prepares a block and hands it to the handle once it is filled
    DevOwner tmp;
    uint32_t* d = nullptr;
    TRY(tmp.alloc(&d, 624 * 4));
    h.mem.adopt(tmp);
    h.table = d;
    EXPECT(tmp.blocks.empty() && g_live.count(d) == 1, 0, 0);
  }
  EXPECT(g_frees - frees0 == expect_frees, g_frees - frees0, expect_frees);   // nothing else was freed before destroy
  *frees_before_destroy = expect_frees;
  return 0;
#undef TRY
}

static long n_lives = 0;
static void check_owner() {
  long total_asks = 0;
  {   // without a failure: how many allocations the sequence makes
    const long a0 = g_allocs, f0 = g_frees;
    long before = 0;
    {
      Life h;
      EXPECT(live_life(h, &total_asks, &before) == 0, 0, 0);
      EXPECT((long)g_live.size() == (g_allocs - a0) - before, g_live.size(), before);
      EXPECT(h.mem.blocks.size() == g_live.size(), h.mem.blocks.size(), g_live.size());   // retired blocks included
    }
    EXPECT(g_live.empty() && g_allocs - a0 == g_frees - f0 && g_allocs - a0 == total_asks, g_allocs - a0, g_frees - f0);
    n_lives++;
  }
  for (long k = 1; k <= total_asks; k++) {   // the k-th allocation fails
    const long a0 = g_allocs, f0 = g_frees;
    long asked = 0, before = 0;
    {
      Life h;
      g_fail_at = k;
      const int e = live_life(h, &asked, &before);
      g_fail_at = 0;
      EXPECT(e == 2 && asked == k, e, asked);
      EXPECT(g_allocs - a0 == k - 1, g_allocs - a0, k);
    }   // (as monsoon_create does after a failure: destroy what there is)
    EXPECT(g_live.empty() && g_allocs - a0 == g_frees - f0, g_allocs - a0, g_frees - f0);
    n_lives++;
  }
  {   // free_all is what destroy calls; the destructor after it has nothing left to free
    DevOwner o;
    void* p = nullptr;
    EXPECT(o.alloc(&p, 8) == 0, 0, 0);
    o.free_all();
    EXPECT(g_live.empty() && o.blocks.empty(), g_live.size(), 0);
  }
}

static void check_lazy_objects() {
  LazyObjects<int*> ev;
  int made = 0, destroyed = 0;
  int* slot[3] = {};
  auto make = [&](int** p) {
    *p = new int(made++);
    return 0;
  };
  for (int round = 0; round < 3; round++)
    for (int i = 0; i < 3; i++) EXPECT(ev.get(slot[i], make) == 0 && slot[i] && *slot[i] == i, round, i);
  EXPECT(made == 3 && ev.all.size() == 3, made, ev.all.size());
  int* none = nullptr;
  EXPECT(ev.get(none, [](int**) { return 7; }) == 7 && !none && ev.all.size() == 3, 0, 0);   // a failed creation is not recorded
  ev.destroy_all([&](int* p) {
    delete p;   // (twice would be the sanitizer's to catch)
    destroyed++;
  });
  ev.destroy_all([&](int*) { destroyed++; });
  EXPECT(destroyed == 3 && ev.all.empty(), destroyed, 0);
}

int main() {
  for (size_t cap : {(size_t)1, (size_t)63, (size_t)64, (size_t)65, (size_t)2048, (size_t)65536, (size_t)1048576}) check_layouts(cap);
  check_ga_offspring();
  check_owner();
  check_lazy_objects();
  printf("ok %ld layouts %ld lives state_bytes %d\n", n_layouts, n_lives, (int)msb::STATE_BYTES);
  return 0;
}
