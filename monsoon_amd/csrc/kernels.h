// kernels.h -- device code shared by every translation unit of libmonsoon_hip.so: per-game buffers, stream-block
// maintenance, the pieces of a decision's look-ahead (PlayLds<U>, legal_set, MSB_EACH_GRANULE), the decision loop made of
// them (play_game), the pop loop of the persistent kernels (pop_games), the hot kernel k_play as a template over
// {candidate lanes per game U, waves per SIMD W}, and the launch-table base and default variant every kernel file uses.
// Each instantiation is a full compilation of the rules core, so every variant lives in a translation unit of its own
// (variant.hip, built in parallel by the Makefile); vs_expert.hip, the three logging kernels' play_log.hip, play_explore.hip
// and play_sample.hip (one launcher type, LoggedOps, and one argument struct on the host side, PlayLogged), env_opp.hip,
// env_opp_explore.hip and env_after.hip hold one further instantiation each, replay_log.hip and replay_after.hip one of the
// rules core without the decision loop; monsoon_hip.hip holds the API kernels and the host side.
//
// Execution model
//   * Hot kernel k_play<U,W>: ONE WAVEFRONT PER GAME at a time (a persistent grid of resident wavefronts, each popping
//     game indices from its range's counter).  The game's record is loaded from HBM into REGISTERS once and stays
//     there for up to `rounds` decisions: a record is SG granules of 16 bytes, and lane l keeps granules l, l + 64, ...
//     of the current record (v_par) and of the best successor found so far in this decision (v_best) -- one granule =
//     four VGPRs each on the standard record.  Per decision: up to U candidate actions are advanced at once, lane l
//     stepping its own private copy of the state in LDS.  On the standard record every private copy is one
//     contiguous column, STATE_BYTES apart (752 = -16 mod 128: lanes touching the same field hit distinct LDS
//     banks, and a field's address is the lane's column base plus an offset); the extended and the large record, and on
//     the standard record k_play_vs, k_play_log, k_play_explore and k_env_after (PLAY_LDS_COLUMNS_BOT / _AFTER below), keep the copies
//     interleaved across lanes in 16-byte granules (granule c of lane l at (c*U + l)*16).  Both maps: lds_layout.h.  A whole entity is one
//     ds_read_b128; cloning is U 16-byte LDS writes per lane straight from registers, lane l carrying granule l.  The
//     functions that read the current record (end of game, legal mask, features, stream cursor) find its image in
//     candidate column 0, written there from the registers before they run (Col0Mem, state.h).  Scores are reduced
//     with shuffles over the U candidate lanes (first maximum in ascending action order = np.argmax over the sorted
//     legal list); a new best is one 16-byte LDS read per lane into v_best, and the commit is a register move.
//     Nothing is re-executed: the committed successor IS one of the look-ahead results, also when the legal set
//     needs several passes of U lanes, and its features are the next decision's "before" features.
//   * The game's MT19937 stream lives in HBM as two blocks of tempered outputs (current + next) plus the raw
//     state; candidate steps read it through a private cursor, the committed cursor travels with the record and
//     the wave regenerates a block (twist in LDS) when it is used up.
//   * Integer/index work: no MFMA.  f64 appears only in the weighted draw and the score.
#pragma once
#include <hip/hip_runtime.h>

#include <math.h>
#include <stdint.h>

#include "../../include/monsoon.h"
#include "rules.h"
#include "canon.h"
#include "coop_features.h"
#include "coop_draw.h"
#include "coop_legal.h"
#include "pass_glue.h"
#include "sample_weight.h"

namespace msbk {
using namespace msb;


constexpr int SW = STATE_WORDS;               // record stride in HBM, words (STATE_BYTES is a multiple of 16)
constexpr int SG = STATE_BYTES / 16;         // 16-byte granules per record
static_assert(STATE_BYTES % 16 == 0, "record must be whole granules");
typedef uint32_t u32x4 __attribute__((ext_vector_type(4)));
constexpr int RNG_WORDS = 2 * MT_N;          // tempered outputs: two blocks per game

struct GameMeta {
  int32_t p1, p2;          // weight-table rows of the FIRST / SECOND player
  int8_t result;           // -2 running, -1 draw, 0 FIRST won, 1 SECOND won
  uint8_t fault;
  uint8_t last_action;
  uint8_t flags;           // b0: ended with a winner (have_winner), as opposed to max_turns / a fault
  uint16_t steps;          // committed steps (decisions and monsoon_step calls)
  uint16_t decided;        // decisions committed by k_decide
  uint32_t rng;            // cursor (bits 0-15) | current block (bit 16)
  uint32_t lookahead;      // look-ahead transitions executed for this game
  uint32_t match;          // schedule index (rollout)
  uint8_t la_fault;        // first build-limit fault (code >= 16) a LOOK-AHEAD of this game hit: that action was scored
                           // 0.0 where the reference computes a score, so the game may have left the reference's line
  uint8_t pad_[3];
};
static_assert(sizeof(GameMeta) == 32, "one 32-byte row per game");

struct DevBuffers {
  uint32_t* state;     // [cap][SW]
  uint32_t* rng_out;   // [cap][2][624]
  uint32_t* rng_mt;    // [cap][624]
  GameMeta* meta;      // [cap]
  double* weights;     // [n_individuals][10]
  unsigned long long* stats;  // [8]: lookahead, decisions, finished, faults, capacity_faults, look-ahead capacity faults
  double* scores;      // [cap][156] or null
  double* best;        // [cap]
  int* pop;            // [SPLIT_MAX][2][POP_PARTS * POP_STRIDE] game-index counters of the persistent k_decide: per sub-batch of a split call (k_play) a pair alternating between launches
  unsigned long long* prof;   // [cap][..] phase cycles, scope cycles, scope calls (profiling build), profiling build only (else null)
  uint32_t* wk_ovf;    // overflow blocks of the rules core's work stack: [workgroup][SK_CAP - SKW][lanes stepping games in it]
};

// Work-stack words per game kept in LDS (state.h LaneMem, rules.h wk_reserve): 98 % of the steps of a neutral-deck game
// never hold more than 8; a step that wants more than SKW - SK_NEED when it enters an ability or a move parks what it has
// in the workgroup's eviction block in HBM.
#if defined(MSB_SKW)
constexpr int SKW = MSB_SKW;
#else
constexpr int SKW = 21;
#endif
static_assert(SKW >= SK_NEED + 9 && SKW * 4 >= 80, "room for the largest frame + the eviction mark + what a handler pushes; the candidates' features overlay their stacks");
constexpr int OVF_WORDS = SK_CAP;   // per stepping lane

enum { ST_LOOKAHEAD = 0, ST_DECISIONS = 1, ST_FINISHED = 2, ST_FAULTS = 3, ST_CAPFAULTS = 4, ST_LACAPFAULTS = 5, ST_N = 6, ST_PROF = 8, ST_WORDS = 32, PROF_WORDS = 138 };
// Phase timing of k_play (profiling build only, -DMSB_PROF=1 -> libmonsoon_hip_prof.so; never the product):
// wave cycles per phase (PROF_MARK(0..7) in play_game) accumulated into the game's row of b.prof.
#if defined(MSB_PROF) && MSB_PROF
#define PROF_DECL()                                                                                   \
  unsigned long long prof_acc[8] = {0, 0, 0, 0, 0, 0, 0, 0};                                          \
  const unsigned long long prof_wall0 = wall_clock64();                                               \
  for (int i_ = lane; i_ < (928 - 16) / 4; i_ += 64) *(MSB_AS_LDS unsigned*)(uintptr_t)(MSB_PROF_LDS + 4 * i_) = 0u; \
  __syncthreads();                                                                                    \
  unsigned long long prof_t = __builtin_readcyclecounter()
#define PROF_MARK(ph)                                         \
  do {                                                        \
    unsigned long long now_ = __builtin_readcyclecounter();   \
    prof_acc[ph] += now_ - prof_t;                            \
    prof_t = now_;                                            \
  } while (0)
#define PROF_FLUSH()                                                        \
  do {                                                                      \
    __syncthreads();                                                        \
    if (lane == 0)                                                          \
      for (int i_ = 0; i_ < 8; i_++) b.prof[(size_t)g * PROF_WORDS + i_] += prof_acc[i_]; \
    if (lane == 0) {                                                        \
      b.prof[(size_t)g * PROF_WORDS + 136] = prof_wall0;                    \
      b.prof[(size_t)g * PROF_WORDS + 137] = wall_clock64();                \
    }                                                                       \
    if (lane < 32) {                                                        \
      b.prof[(size_t)g * PROF_WORDS + 8 + lane] += *(MSB_AS_LDS unsigned long long*)(uintptr_t)(MSB_PROF_LDS + 8 * lane); \
      b.prof[(size_t)g * PROF_WORDS + 40 + lane] += *(MSB_AS_LDS unsigned*)(uintptr_t)(MSB_PROF_LDS + 256 + 4 * lane);   \
      b.prof[(size_t)g * PROF_WORDS + 72 + lane] += *(MSB_AS_LDS unsigned long long*)(uintptr_t)(MSB_PROF_LDS + 384 + 8 * lane); \
      b.prof[(size_t)g * PROF_WORDS + 104 + lane] += *(MSB_AS_LDS unsigned long long*)(uintptr_t)(MSB_PROF_LDS + 640 + 8 * lane); \
    }                                                                       \
  } while (0)
#else
#define PROF_DECL() do {} while (0)
#define PROF_MARK(ph) do {} while (0)
#define PROF_FLUSH() do {} while (0)
#endif

// ------------------------------------------------------------------------------------------------
// RNG block maintenance (wave-cooperative, in LDS)
// ------------------------------------------------------------------------------------------------
// In-place MT19937 twist of 624 words in LDS by one wavefront.  Within one pass all lanes read
// before any lane writes (a wave executes in lockstep), and passes are ordered by barriers.
__device__ inline void wave_twist_lds(MSB_AS_LDS uint32_t* mt, int lane) {
  for (int k0 = 0; k0 < MT_N - MT_M; k0 += 64) {
    int k = k0 + lane;
    uint32_t v = 0;
    bool on = k < MT_N - MT_M;
    if (on) v = mt[k + MT_M] ^ mt_mix(mt[k], mt[k + 1]);
    __syncthreads();
    if (on) mt[k] = v;
    __syncthreads();
  }
  for (int k0 = MT_N - MT_M; k0 < MT_N - 1; k0 += 64) {
    int k = k0 + lane;
    uint32_t v = 0;
    bool on = k < MT_N - 1;
    if (on) v = mt[k + (MT_M - MT_N)] ^ mt_mix(mt[k], mt[k + 1]);
    __syncthreads();
    if (on) mt[k] = v;
    __syncthreads();
  }
  if (lane == 0) mt[MT_N - 1] = mt[MT_M - 1] ^ mt_mix(mt[MT_N - 1], mt[0]);
  __syncthreads();
}

// Regenerate tempered block `which` of game g from the raw state (advancing it one twist).
__device__ inline void wave_refill(const DevBuffers& b, int g, int which, MSB_AS_LDS uint32_t* tmp, int lane) {
  uint32_t* mt = b.rng_mt + (size_t)g * MT_N;
  for (int k = lane; k < MT_N; k += 64) tmp[k] = mt[k];
  __syncthreads();
  wave_twist_lds(tmp, lane);
  uint32_t* out = b.rng_out + (size_t)g * RNG_WORDS + which * MT_N;
  for (int k = lane; k < MT_N; k += 64) {
    uint32_t v = tmp[k];
    mt[k] = v;
    out[k] = mt_temper(v);
  }
  __syncthreads();
}

// Attach game g's stream window to the record an engine works on (fields H_RNGCUR/NXT/POS).
template <class E>
__device__ MSB_INL void attach_rng(E& e, const DevBuffers& b, int g, uint32_t rng) {
  const uint32_t* base = b.rng_out + (size_t)g * RNG_WORDS;
  int cur = (rng >> 16) & 1;
  e.rng_attach(base + cur * MT_N, base + (cur ^ 1) * MT_N, rng & 0xffffu);
}
__device__ MSB_INL uint32_t peek_u32(const DevBuffers& b, int g, uint32_t rng) {
  const uint32_t* base = b.rng_out + (size_t)g * RNG_WORDS;
  int cur = (rng >> 16) & 1;
  uint32_t pos = rng & 0xffffu;
  return pos < (uint32_t)MT_N ? base[cur * MT_N + pos] : base[(cur ^ 1) * MT_N + pos - MT_N];
}

// Serial form for the lane-per-game API kernels: one lane owns the game.
__device__ inline void lane_commit_rng(const DevBuffers& b, int g, GameMeta& m, uint32_t pos) {
  int cur = (m.rng >> 16) & 1;
  if (pos >= (uint32_t)MT_N) {
    pos -= MT_N;
    uint32_t* mt = b.rng_mt + (size_t)g * MT_N;
    mt_twist(mt);
    uint32_t* out = b.rng_out + (size_t)g * RNG_WORDS + cur * MT_N;
    for (int k = 0; k < MT_N; k++) out[k] = mt_temper(mt[k]);
    cur ^= 1;
  }
  m.rng = pos | ((uint32_t)cur << 16);
}

// [16,928) holds the function-scope counters of the profiling build (msb_base.h); then the weight table (state.h).
constexpr int LDS_ORIGIN = LDS_RECORDS;

// ------------------------------------------------------------------------------------------------
// Hot kernel: a wavefront takes a game, keeps its record in registers and plays up to `rounds` decisions of it
// (look-ahead + score + argmax + commit each) before it writes the record back and takes the next game.
// Dynamic LDS map (bytes): weight table | [PRIV, +SG*U*16) candidate records -- standard record: column c is the
// contiguous [PRIV + c*STATE_BYTES, +STATE_BYTES); extended records: lane-interleaved in 16-byte granules; PlayLds::Map
// (column 0 doubles as the image of the current record, the whole area as the twist buffer) |
// 10 weights + 10 "before" + 10 "best after" features | the candidates' work stacks (SKW words each, interleaved word by
// word), which hold their "after" features once a pass has stepped
// ------------------------------------------------------------------------------------------------
__device__ MSB_INL unsigned long long uni64(unsigned long long v) {   // a wave-uniform 64-bit value into scalar registers
  unsigned lo = (unsigned)__builtin_amdgcn_readfirstlane((int)(unsigned)v);
  unsigned hi = (unsigned)__builtin_amdgcn_readfirstlane((int)(unsigned)(v >> 32));
  return ((unsigned long long)hi << 32) | lo;
}

// The pieces of a decision's look-ahead, named once per U: the LDS map, the engines, which forms the build uses, and the
// steps of a decision that work on LDS and scalars.  play_game (below) and after_slot (env_after.h) compose them; a new
// consumer of the look-ahead does too.
template <bool COLS, class Columns, class Interleaved>
struct LdsPick {
  typedef Columns T;
};
template <class Columns, class Interleaved>
struct LdsPick<false, Columns, Interleaved> {
  typedef Interleaved T;
};
// COLS: the candidate records' map.  A kernel takes the build's (PLAY_LDS_COLUMNS) unless it is one of the four that came
// out of the compiler larger on columns than on the interleave on the standard record, which keep the interleave there
// (profiles/lds_columns_isa_diff.txt: k_play_vs and k_play_log a private segment of 16 bytes more, k_play_explore and
// k_env_after one and three scratch instructions more; none of them is on the path bench.py measures).  On the large
// record, were it built on columns (state.h MSB_LDS_COLUMNS_LARGE), every kernel shrank: they would all take them.
#if defined(MSB_EXT) && MSB_EXT == 2
constexpr bool LARGE_RECORD = true;
#else
constexpr bool LARGE_RECORD = false;
#endif
constexpr bool PLAY_LDS_COLUMNS_BOT = PLAY_LDS_COLUMNS && LARGE_RECORD;     // k_play_vs, k_play_log, k_play_explore (play_game<.., VS, !SAMPLE>)
constexpr bool PLAY_LDS_COLUMNS_AFTER = PLAY_LDS_COLUMNS && LARGE_RECORD;   // k_env_after (after_slot)
template <int U, bool COLS_ = PLAY_LDS_COLUMNS>
struct PlayLds {
  static constexpr int PRIV = LDS_ORIGIN;
  static constexpr int PRIV_BYTES = SG * U * 16 > MT_N * 4 ? SG * U * 16 : ((MT_N * 4 + 15) & ~15);   // doubles as the twist buffer
  static constexpr int WF = PRIV + PRIV_BYTES;       // 10 weights + 10 "before" features + 10 features of the best successor (f64)
  static constexpr int SKB = WF + 240;               // work stacks of the U candidate lanes ...
  static constexpr int CF = SKB;                     // ... and, once a pass has stepped (stacks empty), their ten "after" features each (f64)
  static constexpr int TOTAL = SKB + U * SKW * 4;
  // The candidate records' map (lds_layout.h): a contiguous column each where the record's size keeps the columns off each
  // other's banks, the 16-byte interleave elsewhere (state.h PLAY_LDS_COLUMNS).  Both fill exactly SG * U * 16 bytes: TOTAL
  // is the same for either.
  static constexpr bool COLS = COLS_;
  typedef lds_layout::RecordMap<U, PRIV, STATE_BYTES, COLS> Map;
  static_assert(Map::AREA <= PRIV_BYTES && Map::granule(U - 1, SG - 1) + 16 == PRIV + Map::AREA, "the records lie inside the candidate area");
  template <class Columns, class Interleaved> using Pick = typename LdsPick<COLS, Columns, Interleaved>::T;
  typedef Engine<Pick<Col0ColMem<U, PRIV>, Col0Mem<U, PRIV>>> ParEngine;                           // the current record: candidate column 0
  typedef Engine<Pick<LaneColMem<U, PRIV, SKB, SKW>, LaneMem<U, PRIV, SKB, SKW>>> CandEngine;      // candidate `lane`'s private copy
  typedef Engine<Pick<SubColColMem<U, PRIV>, SubColMem<U, PRIV>>> SubEngine;   // candidate (lane % U)'s record, read only: the wave-cooperative features
  static constexpr int GPL = (SG + 63) / 64;   // granules of a record per lane
  // Features by the whole wave (coop_features.h) where a candidate has sub-lanes to spare, on the standard record.  The
  // extended records keep the serial form: with 2 x 12 VGPRs of record per lane next to the phase's temporaries the
  // register allocator spilled them (k_play<8,2>: 0 -> 312 spilled VGPRs, scratch 3 168 -> 3 408 B), see DESIGN.md section 4.
  static constexpr bool COOP = U < 64 && GPL == 1;
  // The weighted draw of the REPLACE candidates resolved once per decision by the whole wave (coop_draw.h): standard record.
#if MSB_COOP_DRAW && !(defined(MSB_EXT) && MSB_EXT)
  static constexpr bool COOP_DRAW = GPL == 1;
#else
  static constexpr bool COOP_DRAW = false;
#endif
  static __device__ MSB_INL MSB_AS_LDS u32x4* priv() { return (MSB_AS_LDS u32x4*)(uintptr_t)PRIV; }   // the area as the twist buffer
  // Granule g of candidate column c: what every whole-wave move of a record reads and writes, by the accessors' own map.
  static __device__ MSB_INL MSB_AS_LDS u32x4* gran(const int c, const int g) {
    if constexpr (COLS) return (MSB_AS_LDS u32x4*)(uintptr_t)Map::granule(c, g);
    else return priv() + (g * U + c);   // (RecordMap<.., false>::granule, spelled as the interleaved accessors spell it)
  }
  static __device__ MSB_INL MSB_AS_LDS double* wf() { return (MSB_AS_LDS double*)(uintptr_t)WF; }
  // What the first draw of this decision's REPLACE steps (actions 148..151) will find, into DRAW_HINT_LDS (coop_draw.h);
  // the candidates read it after the next barrier, wherever in the passes they sit.  A decision without such a
  // candidate clears the word the one before it left.
  static __device__ MSB_INL void draw_hint(ParEngine& pe, const DevBuffers& b, const int g, const uint32_t rng, const uint64_t mask2, const int lane) {
    if constexpr (COOP_DRAW) {
      uint32_t hint = 0u;
      if ((mask2 >> (148 - 128)) & 0xfull) {   // (uniform)
        const bool u_ok = (rng & 0xffffu) + 1u < (uint32_t)(2 * MT_N);
        const uint32_t ra = u_ok ? peek_u32(b, g, rng) : 0u, rb = u_ok ? peek_u32(b, g, rng + 1u) : 0u;
        int sl = lane;   // (opaque, as for the features below)
        asm volatile("" : "+v"(sl));
        hint = coop_draw(pe, sl, ra, rb, u_ok);
      }
      if (lane == 0) *(MSB_AS_LDS uint32_t*)(uintptr_t)DRAW_HINT_LDS = hint;
    }
  }
  // The features of the candidates in `part` (a ballot over lanes 0 .. U-1) by the whole wave: lane l is sub-lane l / U of
  // candidate l % U, whose ten values land in LDS at dst + (l % U) * 80.  Returns that row.
  static __device__ MSB_INL MSB_AS_LDS double* coop_cand_features(const unsigned long long part, const int lane, const int dst) {
    int sl = lane;   // (opaque: what derives from it is computed here, not hoisted out of the game loop and spilled)
    asm volatile("" : "+v"(sl));
    const int col = sl % U;
    const bool on = (part >> col) & 1;
    SubEngine se;
    se.m.set_col(col);
    MSB_AS_LDS double* cfc = (MSB_AS_LDS double*)(uintptr_t)(dst + col * 80);
    coop_features<U>(se, sl, on, cfc);
    return cfc;
  }
  // The serial form: candidate `lane` computes its own ten values (fa, for the score) and leaves them at dst.
  template <class P>
  static __device__ MSB_INL void cand_features(CandEngine& ce, double (&fa)[10], P dst) {
    ce.features(fa);
    for (int i = 0; i < 10; i++) dst[i] = fa[i];
  }
};

// The legal set of the current record as wave-uniform scalars; `rem` loses the U lowest actions with every pass.
struct LegalSet {
  uint64_t mask[3], rem[3];
  int n;
};
// The whole wave computes it from tile and hand masks (coop_legal.h) on the standard record; the extended records keep
// the serial legal_mask_v(), as they keep the serial features and draw.  -DMSB_COOP_LEGAL=0 builds the serial form everywhere.
#if MSB_COOP_LEGAL && !(defined(MSB_EXT) && MSB_EXT)
constexpr bool COOP_LEGAL = SG <= 64;
#else
constexpr bool COOP_LEGAL = false;
#endif
template <class E>
__device__ MSB_INL LegalSet legal_set(E& pe) {
  msb_u64x4 lm;
  if constexpr (COOP_LEGAL) lm = coop_legal_v<E>();
  else lm = pe.legal_mask_v();
  const uint64_t m0 = uni64(lm[0]), m1 = uni64(lm[1]), m2 = uni64(lm[2]);
  const int n = __popcll(m0) + __popcll(m1) + __popcll(m2);
  return LegalSet{{m0, m1, m2}, {m0, m1, m2}, n};
}

// Lane `lane_`'s share of a record: granules lane_, lane_ + 64, ... (gr_), the j_-th of them in element j_ of a register
// array u32x4[GPL_].  The moves of a record between HBM, registers and the candidate columns are spelled with it in
// place -- load: v[j_] = grec[gr_]; column c: *L::gran(c, gr_) -- and not as functions: handed the register array by
// reference, pointer, value or lambda capture, a function cost k_play<8,5> up to 16 bytes of scratch.
#define MSB_EACH_GRANULE(GPL_, lane_, body_)            \
  _Pragma("unroll") for (int j_ = 0; j_ < GPL_; j_++) { \
    const int gr_ = lane_ + 64 * j_;                    \
    if (gr_ < SG) { body_; }                            \
  }

// The vector env's heuristic opponent (opponent 2, env_opp.hip): what play_game<U, true> needs beyond DevBuffers.
constexpr int ENV_OPP_BOUND = 64;   // opponent decisions per call before FAULT_OPP_BOUND (a guard, include/monsoon.h)
struct EnvPolicy {
  const int32_t* rows;   // [n]: the weight-table row slot g's opponent plays
  uint32_t* steps;       // [n]: the opponent's committed steps (monsoon_debug_counters word 7)
  uint32_t* lookahead;   // [n]: its look-ahead transitions (word 16)
  int agent_side, max_steps;
};

// Where play_game<.., LOG = true> writes down what it commits (k_play_log, play_log.hip): row g of each array, `stride`
// entries apart, entry k being the game's k-th committed step.  score and n_legal may be null.
struct PlayLog {
  uint8_t* action;    // [n][stride]
  double* score;      // [n][stride] the decision's best score (what b.best reports), NaN for a bot step
  int16_t* n_legal;   // [n][stride] legal actions of the decision, 0 for a bot step
  int stride;
};
// Entry meta.steps (before its increment) of game g, by lane 0: plain stores, like b.best[g].
__device__ MSB_INL void log_step(const PlayLog& lg, const int g, const int lane, const int k, const int action, const double score,
                                 const int n_legal) {
  if (lane == 0 && k < lg.stride) {   // (k < max_turns = stride by the loop's own end rule)
    const size_t at = (size_t)g * lg.stride + k;
    lg.action[at] = (uint8_t)action;
    if (lg.score) lg.score[at] = score;
    if (lg.n_legal) lg.n_legal[at] = (int16_t)n_legal;
  }
}

// What play_game<.., EXPLORE = true> needs beyond the PlayLog (k_play_explore, play_explore.hip; include/monsoon.h
// monsoon_rollout_explore): the rule's four words, the match seed of every game of the batch, and the three further log
// arrays (rows like the PlayLog's, each may be null).
struct PlayExplore {
  uint32_t seed, threshold, sides;
  int until_step;
  const uint32_t* match_seed;   // [n]
  uint8_t* greedy;              // [n][stride] the decision's arg-max action
  uint8_t* explored;            // [n][stride] 1 = the decision's draw said "explore"
  double* taken_score;          // [n][stride] score of the committed action
};
// monsoon_amd/fitness.py hash32 over four words: integer arithmetic only, so the host reproduces every draw.
__device__ MSB_INL uint32_t explore_hash32(const uint32_t a, const uint32_t b, const uint32_t c, const uint32_t d) {
  const uint32_t v[4] = {a, b, c, d};
  uint32_t h = 0x9E3779B9u;
  _Pragma("unroll") for (int i = 0; i < 4; i++) {
    h ^= v[i] + 0x7F4A7C15u + (h << 6) + (h >> 2);
    h *= 0x85EBCA6Bu;
    h ^= h >> 13;
    h *= 0xC2B2AE35u;
    h ^= h >> 16;
  }
  return h;
}
// The rank in the ascending legal list that the decision at committed step k commits instead of its arg-max, -1 where it
// does not explore (all arguments wave-uniform, so is the result).
__device__ MSB_INL int explore_rank(const PlayExplore& ex, const uint32_t match_seed, const int side, const int k, const int n_legal) {
  if (!((ex.sides >> side) & 1u) || (ex.until_step > 0 && k >= ex.until_step) || n_legal <= 0) return -1;
  if (explore_hash32(ex.seed, match_seed, (uint32_t)k, 0u) >= ex.threshold) return -1;
  return (int)(((unsigned long long)explore_hash32(ex.seed, match_seed, (uint32_t)k, 1u) * (unsigned)n_legal) >> 32);
}
// What an exploring decision carries from its passes to its commit: the rank it commits (-1: its arg-max), that action
// and its score.  It lives in the caller (k_play_explore) and reaches play_game as a pointer: declared in play_game, three
// dead scalars changed the register allocation of every existing instantiation, and even an empty struct that of
// k_env_opp.
struct ExploreTake {
  int r = -1, a = 0;
  double s = 0.0;
};
// What play_game<U, true, false, false, true> needs beyond the EnvPolicy (k_env_opp_explore, env_opp_explore.hip;
// include/monsoon.h monsoon_env_set_opponent_explore): an argument of that kernel alone, as EnvSched is of its kernel --
// EnvDev, EnvPolicy, PlayExplore and ExploreTake keep their layout.  The rule and the thresholds are device words that the
// host rewrites between steps, so every decision reads them anew (a captured step holds the addresses, not the contents).
struct EnvExplore {
  const uint32_t* rule;         // [2]: the exploration seed, until_step (int32)
  const uint32_t* thresholds;   // [n]: slot g's opponent explores iff draw0 < thresholds[g]
  uint32_t* explored;           // [n]: decisions whose draw said "explore", since monsoon_env_reset
  const uint32_t* seed0;        // [n] (EnvDev's): the episode seed is seed0[g] + episode[g] * stride ...
  const int32_t* episode;       // [n] ... as env.inc env_seed computes it
  uint32_t stride;
};
// explore_rank for slot g's opponent at committed step k of its episode.  g is wave-uniform and so is every word loaded here;
// readfirstlane says so to the compiler.
__device__ MSB_INL int env_explore_rank(const EnvExplore& ee, const int g, const int k, const int n_legal) {
  const int until_step = __builtin_amdgcn_readfirstlane((int)ee.rule[1]);
  if ((until_step > 0 && k >= until_step) || n_legal <= 0) return -1;
  const uint32_t seed = (uint32_t)__builtin_amdgcn_readfirstlane((int)ee.rule[0]);
  const uint32_t threshold = (uint32_t)__builtin_amdgcn_readfirstlane((int)ee.thresholds[g]);
  const uint32_t s = (uint32_t)__builtin_amdgcn_readfirstlane((int)(ee.seed0[g] + (uint32_t)ee.episode[g] * ee.stride));
  if (explore_hash32(seed, s, (uint32_t)k, 0u) >= threshold) return -1;
  return (int)(((unsigned long long)explore_hash32(seed, s, (uint32_t)k, 1u) * (unsigned)n_legal) >> 32);
}
__device__ MSB_INL void log_explore(const PlayExplore& ex, const PlayLog& lg, const int g, const int lane, const int k, const int greedy,
                                    const int explored, const double taken_score) {
  if (lane == 0 && k < lg.stride) {
    const size_t at = (size_t)g * lg.stride + k;
    if (ex.greedy) ex.greedy[at] = (uint8_t)greedy;
    if (ex.explored) ex.explored[at] = (uint8_t)explored;
    if (ex.taken_score) ex.taken_score[at] = taken_score;
  }
}

// What play_game<.., SAMPLE = true> needs beyond the PlayLog and the PlayExplore (k_play_sample, play_sample.hip;
// include/monsoon.h monsoon_rollout_sample): the inverse temperature and the two further log arrays (rows like the
// PlayLog's, each may be null).  An argument of that kernel alone; play_game sees a pointer to it.
struct PlaySample {
  double inv_temperature;
  uint32_t* weight_total;   // [n][stride] sum of the decision's weights
  uint32_t* taken_weight;   // [n][stride] weight of the committed action
};
// The draw of a sampling decision over the actions in the masks (bit l of m_i = action 64 i + l, whose score is sc[64 i + l]),
// by the whole wavefront: lane l takes actions l, l + 64 and l + 128, w = weight24((score - best) * inv_t) where the
// action is legal and 0 elsewhere, an inclusive integer scan across the wave in ascending action order, r = (draw1 * total)
// >> 32, and the first action whose prefix exceeds r (a ballot) -- its weight is not 0, because the prefix before it does
// not exceed r.  Everything is integer from the weights on, so no order of summation is imposed.  total == 0 (best is NaN
// or infinite): pos = -1.  All arguments but `lane` are wave-uniform and so is the result.
struct SamplePick {
  int pos;
  uint32_t total, w;
};
__device__ MSB_INL SamplePick sample_pick(const double* sc, const uint64_t m0, const uint64_t m1, const uint64_t m2, const double best,
                                          const double inv_t, const uint32_t draw1, const int lane) {
  const uint64_t m[3] = {m0, m1, m2};
  uint32_t w[3], p[3];
  uint32_t before = 0u;
  _Pragma("unroll") for (int i = 0; i < 3; i++) {
    w[i] = 0u;
    if ((m[i] >> lane) & 1ull) w[i] = weight24((sc[64 * i + lane] - best) * inv_t);
    uint32_t q = w[i];
    for (int off = 1; off < 64; off <<= 1) {
      const uint32_t t = __shfl_up(q, off);
      if (lane >= off) q += t;
    }
    p[i] = before + q;
    before = (uint32_t)__builtin_amdgcn_readlane((int)p[i], 63);
  }
  const uint32_t total = before;   // <= 156 * 2**24
  if (total) {
    const uint32_t r = (uint32_t)(((unsigned long long)draw1 * total) >> 32);   // in [0, total)
    _Pragma("unroll") for (int i = 0; i < 3; i++) {
      const unsigned long long bal = __ballot(p[i] > r);
      if (bal) {
        const int l = __builtin_ctzll(bal);
        return SamplePick{64 * i + l, total, (uint32_t)__builtin_amdgcn_readlane((int)w[i], l)};
      }
    }
  }
  return SamplePick{-1, 0u, 0u};
}
// Does the decision at committed step k leave its arg-max (explore_rank's three conditions and draw0), and with which draw1.
__device__ MSB_INL bool sample_draw(const PlayExplore& ex, const uint32_t match_seed, const int side, const int k, const int n_legal, uint32_t& draw1) {
  draw1 = 0u;
  if (!((ex.sides >> side) & 1u) || (ex.until_step > 0 && k >= ex.until_step) || n_legal <= 0) return false;
  if (explore_hash32(ex.seed, match_seed, (uint32_t)k, 0u) >= ex.threshold) return false;
  draw1 = explore_hash32(ex.seed, match_seed, (uint32_t)k, 1u);
  return true;
}
__device__ MSB_INL void log_sample(const PlaySample& sp, const PlayLog& lg, const int g, const int lane, const int k, const uint32_t total,
                                   const uint32_t taken) {
  if (lane == 0 && k < lg.stride) {
    const size_t at = (size_t)g * lg.stride + k;
    if (sp.weight_total) sp.weight_total[at] = total;
    if (sp.taken_weight) sp.taken_weight[at] = taken;
  }
}

// What play_game<.., SAMPLE = true, POLICY = true> needs beyond the PlayLog and the PlayExplore (k_play_policy,
// play_policy.hip; include/monsoon.h monsoon_rollout_policies): a threshold and an inverse temperature per weight row --
// the decision reads those of the row that moves -- and the two weight arrays of the log (rows like the PlayLog's, each may
// be null).  An argument of that kernel alone; play_game sees a pointer to it.  PlayExplore's threshold is not read.
struct PlayPolicy {
  const uint32_t* threshold;       // [n_individuals]: row r's decisions leave the arg-max iff draw0 < threshold[r]
  const double* inv_temperature;   // [n_individuals]: finite, >= 0 (0: every finite score weighs 2**24, the uniform rule)
  uint32_t* weight_total;          // [n][stride] sum of the decision's weights, on every decision the rule covers
  uint32_t* taken_weight;          // [n][stride] weight of the committed action, likewise
};
// sample_draw with the mover's own threshold (weight row `row`, wave-uniform like every word loaded here): `covered` says
// whether the side's bit, the step limit and a threshold > 0 let the decision leave its arg-max at all -- the decisions whose
// weights the log carries -- and then inv_t is the row's inverse temperature; the result says whether draw0 did.
__device__ MSB_INL bool policy_draw(const PlayPolicy& pp, const PlayExplore& ex, const int row, const uint32_t match_seed, const int side, const int k,
                                    const int n_legal, bool& covered, uint32_t& draw1, double& inv_t) {
  draw1 = 0u;
  inv_t = 0.0;
  covered = false;
  if (!((ex.sides >> side) & 1u) || (ex.until_step > 0 && k >= ex.until_step) || n_legal <= 0) return false;
  const uint32_t threshold = (uint32_t)__builtin_amdgcn_readfirstlane((int)pp.threshold[row]);
  if (!threshold) return false;
  covered = true;
  inv_t = __longlong_as_double((long long)uni64((unsigned long long)__double_as_longlong(pp.inv_temperature[row])));
  if (explore_hash32(ex.seed, match_seed, (uint32_t)k, 0u) >= threshold) return false;
  draw1 = explore_hash32(ex.seed, match_seed, (uint32_t)k, 1u);
  return true;
}

// What play_game<U, true, false, false, false, true> needs beyond the EnvPolicy (k_env_opp_sample, env_opp_sample.hip;
// include/monsoon.h monsoon_env_set_opponent_sample): the EnvExplore of the rule -- WHEN a decision leaves its arg-max is
// env_explore_rank's conditions word for word -- and the slots' inverse temperatures, device words like the thresholds.  An
// argument of that kernel alone; play_game sees it through its EnvExplore pointer, so no other form gains an argument.
struct EnvSample : EnvExplore {
  const double* inv_temperature;   // [n]: slot g's opponent weighs with inv_temperature[g] (finite, > 0)
};
// sample_draw for slot g's opponent at committed step k of its episode: does the decision leave its arg-max, and with which
// draw1 and inverse temperature.  Every word is loaded anew and is wave-uniform (readfirstlane; the double as two halves).
__device__ MSB_INL bool env_sample_draw(const EnvSample& es, const int g, const int k, const int n_legal, uint32_t& draw1, double& inv_t) {
  draw1 = 0u;
  inv_t = 0.0;
  const int until_step = __builtin_amdgcn_readfirstlane((int)es.rule[1]);
  if ((until_step > 0 && k >= until_step) || n_legal <= 0) return false;
  const uint32_t seed = (uint32_t)__builtin_amdgcn_readfirstlane((int)es.rule[0]);
  const uint32_t threshold = (uint32_t)__builtin_amdgcn_readfirstlane((int)es.thresholds[g]);
  const uint32_t s = (uint32_t)__builtin_amdgcn_readfirstlane((int)(es.seed0[g] + (uint32_t)es.episode[g] * es.stride));
  if (explore_hash32(seed, s, (uint32_t)k, 0u) >= threshold) return false;
  draw1 = explore_hash32(seed, s, (uint32_t)k, 1u);
  inv_t = __longlong_as_double((long long)uni64((unsigned long long)__double_as_longlong(es.inv_temperature[g])));
  return true;
}

// Up to `rounds` decisions of game g by the calling wavefront.  The record lives in registers from the first decision
// to the last; HBM sees one read and one write of it per call.
// ENV = false: the rollout (k_play).  ENV = true: the vector env's opponent turn -- it stops when the agent's side is to
// play, plays the weights of row pol.rows[g], ends the episode by the env's rules after every commit (fault, winner,
// max_steps: include/monsoon.h), stops after `rounds` decisions with FAULT_OPP_BOUND, and writes no scores / best.
// VS = true (k_play_vs, vs_expert.hip; with ENV = false): a side whose weight row is MONSOON_PLAYER_EXPERT is the
// reference's scripted bot.  Its round runs no legal mask, clone, features or arg-max: candidate lane 0 runs
// expert_action() and, unless that raised, step() on column 0 -- the current record's image with the stream window
// attached -- and column 0 is then "the best successor" that the commit takes over.
// LOG = true (k_play_log, play_log.hip; with VS = true): every committed step is written down in `lg`.
// EXPLORE = true (k_play_explore, play_explore.hip, with LOG = true; k_env_opp_explore, env_opp_explore.hip, with ENV = true
// and the draw of env_explore_rank from `ee`): a decision whose draw says so (explore_rank) commits
// the r-th legal action (xt->r) instead of the arg-max.  Everything new is wave-uniform: the pass that holds rank r takes
// lane r - base -- its record into v_best, its fault and feature flag, its features into wf[20..29], its score -- and on
// such a decision the running arg-max moves run_a / run_s only, so v_best is written exactly once, in whichever pass.
// SAMPLE = true (k_play_sample, play_sample.hip, with LOG = true; k_env_opp_sample, env_opp_sample.hip, with ENV = true, the
// draw of env_sample_draw and the slot's inverse temperature from `ee`, an EnvSample; EXPLORE = false): the passes run as without a rule --
// the arg-max and its record in v_best -- and every candidate's score also goes to the game's row of b.scores.  After the
// last pass a decision whose draw says so (sample_draw) draws an action from the softmax over those scores (sample_pick)
// and, unless that is the arg-max, steps it once more from the parent record on column 0 (the clone carries the stream
// window, so the step is the look-ahead's bit for bit): that successor, its fault and no features are what the commit takes.
// The decision's scalars live and die in that one block in front of the commit; `sp` is the kernel's.  The env's form logs
// nothing: lane 0 counts the decision in ee->explored, and the commit, the end rules and the 64-decision guard are ENV's.
// POLICY = true (k_play_policy, play_policy.hip, with SAMPLE and LOG): the sampling form whose threshold and inverse
// temperature are those of the weight row that moves (`pp`, policy_draw), and which weighs the actions of every decision
// the rule covers, drawn or not, so that the log carries the behaviour probability of every row.
//
// MSB_COMMIT_BEST is the commit: adapter = adapter.apply_action(best).  v_best becomes the record (column 0 and v_par);
// the successor carries its own stream cursor (H_RNGPOS), so the cursor is committed and a used-up block refilled by the
// whole wave (the used-up block becomes the new "next" block; the twist buffer is the column area, hence the second copy
// of v_best); the committed successor's features (feat_ok: wf[20..29] holds them) become the "before" side of the next
// decision.  It and MSB_TAKE_LANE (the exploring form's) are the macros local to play_game: it moves the register arrays, and the bot's round expands it a
// second time.
#define MSB_COMMIT_BEST()                                                                           \
  __syncthreads();                                                                                  \
  MSB_EACH_GRANULE(L::GPL, lane, *L::gran(0, gr_) = v_best[j_])                                                      \
  __syncthreads();                                                                                  \
  {                                                                                                 \
    uint32_t new_pos = (uint32_t)__builtin_amdgcn_readfirstlane((int)pe.rng_pos());                 \
    int cur = (meta.rng >> 16) & 1;                                                                 \
    if (new_pos >= (uint32_t)MT_N) {                                                                \
      new_pos -= MT_N;                                                                              \
      wave_refill(b, g, cur, (MSB_AS_LDS uint32_t*)priv, lane);                                     \
      MSB_EACH_GRANULE(L::GPL, lane, *L::gran(0, gr_) = v_best[j_])                                                  \
      __syncthreads();                                                                              \
      cur ^= 1;                                                                                     \
      if (lane == 0) pe.rng_block_advance();                                                        \
    }                                                                                               \
    meta.rng = new_pos | ((uint32_t)cur << 16);                                                     \
    if (lane == 0) attach_rng(pe, b, g, meta.rng);                                                  \
    have_before = feat_ok != 0;                                                                     \
    if (have_before && lane < 10) wf[10 + lane] = wf[20 + lane];                                    \
    __syncthreads();                                                                                \
    MSB_EACH_GRANULE(L::GPL, lane, v_par[j_] = *L::gran(0, gr_))                                                     \
  }
// EXPLORE: candidate lane wl_ of this pass is what the commit takes -- its fault, its feature flag and features, its record.
#define MSB_TAKE_LANE(wl_)                                                                          \
  cfault = __builtin_amdgcn_readlane(my_fault, wl_);                                                \
  feat_ok = __builtin_amdgcn_readlane(my_feat, wl_);                                                \
  if (feat_ok && lane < 10) wf[20 + lane] = ((MSB_AS_LDS const double*)(uintptr_t)L::CF)[wl_ * 10 + lane]; \
  __syncthreads();                                                                                  \
  MSB_EACH_GRANULE(L::GPL, lane, v_best[j_] = *L::gran(wl_, gr_))
template <int U, bool ENV = false, bool VS = false, bool LOG = false, bool EXPLORE = false, bool SAMPLE = false, bool POLICY = false>
__device__ MSB_INL void play_game(const DevBuffers& b, const int g, const int lane, int max_turns, int rounds, int write_scores,
                                  const EnvPolicy& pol, const PlayLog& lg = PlayLog{}, const PlayExplore& ex = PlayExplore{},
                                  ExploreTake* const xt = nullptr, const EnvExplore* const ee = nullptr, const PlaySample* const sp = nullptr,
                                  const PlayPolicy* const pp = nullptr) {
  static_assert(!EXPLORE || (LOG && !ENV) || (ENV && !VS && !LOG), "the exploring form is a logging rollout or the env's opponent");
  static_assert(!SAMPLE || (!EXPLORE && ((LOG && !ENV) || (ENV && !VS && !LOG))),
                "the sampling form is a logging rollout with a rule of its own or the env's opponent");
  static_assert(!POLICY || (SAMPLE && LOG && !ENV), "the per-row form is a sampling logged rollout");
  typedef PlayLds<U, (VS && !SAMPLE) ? PLAY_LDS_COLUMNS_BOT : PLAY_LDS_COLUMNS> L;
  GameMeta meta = b.meta[g];
  const uint32_t lookahead0 = meta.lookahead;
  if (meta.result != -2) {
    if (!ENV && lane == 0) {
      b.meta[g].last_action = 255;
      if (b.best) b.best[g] = NAN;
    }
    return;
  }
  PROF_DECL();
  MSB_AS_LDS u32x4* priv = L::priv();
  MSB_AS_LDS double* wf = L::wf();
  MSB_AS_LDS double* cf = (MSB_AS_LDS double*)(uintptr_t)(L::CF + (lane < U ? lane : 0) * 80);   // this candidate lane's features
  u32x4* grec = (u32x4*)(b.state + (size_t)g * SW);
  u32x4 v_par[L::GPL], v_best[L::GPL];   // granules lane, lane + 64, ... of the current record / of the best successor so far
  _Pragma("unroll") for (int j_ = 0; j_ < L::GPL; j_++) v_par[j_] = u32x4{0u, 0u, 0u, 0u};
  MSB_EACH_GRANULE(L::GPL, lane, v_par[j_] = grec[gr_])   // coalesced 16-B-per-lane loads, straight into registers
  _Pragma("unroll") for (int j_ = 0; j_ < L::GPL; j_++) v_best[j_] = v_par[j_];
  typename L::ParEngine pe;
  typename L::CandEngine ce;
  // stage: the image of the current record in column 0; with the stream window attached it is also what the clones start from
  MSB_EACH_GRANULE(L::GPL, lane, *L::gran(0, gr_) = v_par[j_])
  __syncthreads();
  if (lane == 0) attach_rng(pe, b, g, meta.rng);
  __syncthreads();
  MSB_EACH_GRANULE(L::GPL, lane, v_par[j_] = *L::gran(0, gr_))
  bool have_before = false;   // wf[10..19] holds the features of the CURRENT state (the committed successor's)
  double last_score = NAN;
  int played = 0;
  PROF_MARK(0);   // stage

  for (int round = 0; round < rounds; round++) {   // (column 0 == v_par here)
    if constexpr (ENV) {
      if (pe.local() == pol.agent_side) break;   // the agent's turn (the env's end rules ran after the last commit)
    } else if (pe.have_winner() || meta.steps >= max_turns) {   // rollout contract: while not have_winner() and steps < max_turns
      int b0 = pe.pl_base(0), b1 = pe.pl_base(1);
      int res = -1;
      if (pe.have_winner()) res = pe.winner_of(b0, b1);
      meta.result = (int8_t)res;
      if (pe.have_winner()) meta.flags |= 1;
      if (played == 0) {
        meta.last_action = 255;
        last_score = NAN;
      }
      break;
    }
    if constexpr (VS) {
      if ((pe.local() == 0 ? meta.p1 : meta.p2) < 0) {   // (uniform) the scripted bot is to play
        int a = 155, f = 0, fs = 0;
        if (lane == 0) {   // (the other lanes wait at the barrier)
          if constexpr (L::COOP_DRAW) *(MSB_AS_LDS uint32_t*)(uintptr_t)DRAW_HINT_LDS = 0u;   // the bot's own REPLACE draws serially
          a = ce.expert_action();
          f = ce.fault();   // random.choice([]) inside the bot: nothing is stepped, the game ends
          if (!f) {
            ce.step(a);
            fs = ce.fault();
            if (!fs && ce.observation_raises()) fs = FAULT_INT_CARD;
          }
        }
        __syncthreads();
        a = __builtin_amdgcn_readfirstlane(a);
        f = __builtin_amdgcn_readfirstlane(f);
        fs = __builtin_amdgcn_readfirstlane(fs);
        MSB_EACH_GRANULE(L::GPL, lane, v_best[j_] = *L::gran(0, gr_))   // the successor (if the bot raised: the record with its cursor moved on)
        constexpr int feat_ok = 0;   // the bot's successor has no features: the next decision computes its "before" side
        MSB_COMMIT_BEST()
        if (!f) {   // one committed transition, no decision, no look-ahead
          if constexpr (LOG) log_step(lg, g, lane, meta.steps, a, NAN, 0);
          meta.steps++;
          meta.last_action = (uint8_t)a;
        }
        played++;
        if (f | fs) {   // a draw with that code, as after a decision's commit below
          meta.fault = (uint8_t)(f ? f : fs);
          meta.result = -1;
          break;
        }
        continue;
      }
    }
#if defined(MSB_STUDY_LEGAL)
    {   // study build (scripts/step_cost.sh): the legal mask computed once more
      const LegalSet ls2 = legal_set(pe);   // (in the form this build uses)
      asm volatile("" : : "s"(ls2.mask[0]), "s"(ls2.mask[1]), "s"(ls2.mask[2]) : "memory");
    }
#endif
    LegalSet ls = legal_set(pe);
    const int n_legal = ls.n;
    PROF_MARK(1);   // legal mask
    L::draw_hint(pe, b, g, meta.rng, ls.mask[2], lane);
    const bool before_raises = pe.observation_raises();
    // weights and "before" features are parked in LDS: 40 fewer live VGPRs across the recursive step calls
    {
      const double* wt = b.weights + (size_t)(ENV ? pol.rows[g] : (pe.local() == 0 ? meta.p1 : meta.p2)) * 10;
      if (lane < 10) wf[lane] = wt[lane];
      // The "before" features of this decision are the "after" features the previous decision computed for the
      // successor it committed (same state, same mover); only the first decision of a call computes them.
      // (in place, like the hand-out of a pass's actions below: as a PlayLds function each of the two gave the extended
      // record's k_play<4,3> seven scratch instructions more)
      if (!before_raises && !have_before) {   // (uniform)
        if constexpr (!L::COOP) {
          if (lane == 0) pe.features(wf + 10);
        } else {
          int sl = lane;   // (opaque: what derives from it is computed here, not hoisted out of the game loop and spilled)
          asm volatile("" : "+v"(sl));
          coop_features<U>(pe, sl, true, wf + 10);   // every lane reads column 0: all U columns compute the same ten values
        }
      }
    }
    __syncthreads();
    PROF_MARK(2);   // before-features

    // Running best over the passes (uniform across the wave); its record is v_best.
    constexpr int NONE_A = 1 << 20;
    double run_s = 0.0;
    int run_a = NONE_A;
    int cfault = 0;
    int feat_ok = 0;                  // wf[20..29] holds the features of the best successor so far
    int la_fault = 0;                 // first build-limit fault a look-ahead of this decision hit
    if constexpr (EXPLORE && ENV)
      xt->r = env_explore_rank(*ee, g, meta.steps, n_legal);
    else if constexpr (EXPLORE)
      xt->r = explore_rank(ex, (uint32_t)__builtin_amdgcn_readfirstlane((int)ex.match_seed[g]), __builtin_amdgcn_readfirstlane(pe.local()),
                        meta.steps, n_legal);
    for (int base = 0; base < n_legal; base += U) {
      double s = 0.0;   // except Exception -> 0.0 (evo/heuristic_agent.py:48-51)
      int my_fault = 0;
      int my_feat = 0;
      int f = 0;
      bool raises = false;
      const int n_act = n_legal - base < U ? n_legal - base : U;   // (uniform) the candidates of this pass: lanes 0 .. n_act-1
      {   // clone: copy.deepcopy (stream window included) for the whole pass, lane l writes granule l of every column in use
        __syncthreads();
        for (int col = 0; col < n_act; col++) MSB_EACH_GRANULE(L::GPL, lane, *L::gran(col, gr_) = v_par[j_])
        __syncthreads();
      }
      const bool active = lane < n_act;
      // lane l takes the (base + l)-th legal action, handed out by the scalar unit; `rem` loses them (pass_glue.h)
      int a = NONE_A;
      pass_actions(ls.rem, n_act, [&](const int l, const int act) { a = lane == l ? act : a; });
#if defined(MSB_STUDY_REPEAT)
      // study build only (scripts/step_cost.sh): the look-ahead step (or a prefix of it, MSB_STUDY_CUT_AT) and its clone
      // executed once more, so that the difference of two counter runs is the cost of exactly that
      for (int rep = 0; rep < MSB_STUDY_REPEAT; rep++) {
#if defined(MSB_STUDY_CUT_AT)
        if (active) ce.step(a, MSB_STUDY_CUT_AT);
#else
        if (active) ce.step(a);
#endif
        __syncthreads();
        for (int col = 0; col < n_act; col++) MSB_EACH_GRANULE(L::GPL, lane, *L::gran(col, gr_) = v_par[j_])
        __syncthreads();
      }
#endif
      PROF_MARK(3);   // clone
      if (active) {
        ce.step(a);
        f = ce.fault();
        raises = f == 0 && ce.observation_raises();
      }
      PROF_MARK(4);   // step
      // The candidates that get features and a score; all of them run the same code now, so the whole wave works on it:
      // lane l is sub-lane l / U of candidate l % U (coop_features.h).  !COOP: the serial form.
      const bool scored = active && f == 0 && !before_raises && !raises;
      if constexpr (!L::COOP) {
        if (scored) {
          // the ten values go to LDS for the winner's sake (argmax below) and feed the score from registers
          double fa[10];
#if defined(MSB_STUDY_FEATURES)
          {   // study build: the candidate's features and its score computed once more
            double fb[10];
            ce.features(fb);
            double s2 = L::CandEngine::action_score_lds(wf, fb);
            asm volatile("" : : "v"(s2), "v"(fb[0]), "v"(fb[9]) : "memory");
          }
#endif
          L::cand_features(ce, fa, cf);
          s = L::CandEngine::action_score_lds(wf, fa);
          my_feat = 1;
        }
      } else {
        const unsigned long long part = __ballot(scored);   // (candidates sit on lanes 0 .. U-1)
        if (part) {
          // the ten values go to LDS (CF), for the score and for the winner's sake (argmax below)
#if defined(MSB_STUDY_FEATURES)
          {   // study build: the candidates' features and their scores computed once more
            double s2 = coop_score(wf, L::coop_cand_features(part, lane, L::CF));
            asm volatile("" : : "v"(s2) : "memory");
          }
#endif
          MSB_AS_LDS double* cfc = L::coop_cand_features(part, lane, L::CF);
          if (scored) {
            s = coop_score(wf, cfc);
            my_feat = 1;
          }
        }
      }
      if (active) {
        if constexpr (SAMPLE) b.scores[(size_t)g * MONSOON_NUM_ACTIONS + a] = s;   // (what the sampler reads after the last pass)
        else if (!ENV && write_scores) b.scores[(size_t)g * MONSOON_NUM_ACTIONS + a] = s;
        my_fault = f ? f : (raises ? FAULT_INT_CARD : 0);
      }
      PROF_MARK(5);   // after-features + score
      {
        // A look-ahead that hits a limit of this build scores 0.0 where the reference would compute a score: the game
        // is marked (meta.la_fault), counted (monsoon_stats.lookahead_capacity_faults), reported (monsoon_game_faults).
        const unsigned long long lfb = __ballot(active && f >= FAULT_CAPACITY);
        if (lfb && !la_fault) la_fault = __builtin_amdgcn_readlane(f, __builtin_ctzll(lfb));
      }
      // first maximum over the ascending legal list == (max score, then min action id)
      // only lanes 0..U-1 hold candidates: butterfly over those, then broadcast lane 0's result to the wave
      double cs = s;
      int ca = a;
      for (int off = U / 2; off >= 1; off >>= 1) {
        double os = __shfl_xor(cs, off);
        int oa = __shfl_xor(ca, off);
        bool take = (oa != NONE_A) && (ca == NONE_A || os > cs || (os == cs && oa < ca));
        if (take) {
          cs = os;
          ca = oa;
        }
      }
      cs = __longlong_as_double((long long)uni64((unsigned long long)__double_as_longlong(cs)));
      ca = __builtin_amdgcn_readfirstlane(ca);
      if (ca != NONE_A && (run_a == NONE_A || cs > run_s)) {   // later passes hold larger action ids: strict >
        run_s = cs;
        run_a = ca;
        if constexpr (!EXPLORE) {
          unsigned long long bal = __ballot(a == ca);
          const int wl = __ffsll((long long)bal) - 1;
          cfault = __builtin_amdgcn_readlane(my_fault, wl);
          feat_ok = __builtin_amdgcn_readlane(my_feat, wl);
          if (feat_ok && lane < 10)   // the winner keeps its features: the next decision's "before" side
            wf[20 + lane] = ((MSB_AS_LDS const double*)(uintptr_t)L::CF)[wl * 10 + lane];
          __syncthreads();
          MSB_EACH_GRANULE(L::GPL, lane, v_best[j_] = *L::gran(wl, gr_))   // the best successor so far, into registers
        } else if (xt->r < 0) {   // (a decision that explores moves the two scalars only: its v_best is the explored lane's, below)
          const int wl = __ffsll((long long)__ballot(a == ca)) - 1;
          MSB_TAKE_LANE(wl)
        }
      }
      if constexpr (EXPLORE) {
        if (xt->r >= base && xt->r < base + U) {   // (uniform) the pass that holds the explored rank: lane r - base is what the commit takes
          const int wl = __builtin_amdgcn_readfirstlane(xt->r - base);   // (< n_act: xt->r < n_legal)
          xt->a = __builtin_amdgcn_readlane(a, wl);
          if constexpr (LOG) {   // (the committed action's score is the log's)
            const unsigned long long sb = (unsigned long long)__double_as_longlong(s);
            xt->s = __longlong_as_double((long long)(((unsigned long long)(unsigned)__builtin_amdgcn_readlane((int)(unsigned)(sb >> 32), wl) << 32) |
                                                      (unsigned)__builtin_amdgcn_readlane((int)(unsigned)sb, wl)));
          }
          MSB_TAKE_LANE(wl)
        }
      }
      PROF_MARK(6);   // argmax + new best into registers
    }
    if constexpr (POLICY) {
      // The sampling block below with the mover's own rule (a block of its own: the existing forms keep their code).  The
      // threshold and the inverse temperature are those of the weight row that scored this decision; every decision the rule
      // covers weighs its actions and logs total and the committed action's weight -- 2**24 for an arg-max that was not
      // drawn, weight24(0) -- and only a drawn action other than the arg-max is stepped once more.
      __syncthreads();
      MSB_EACH_GRANULE(L::GPL, lane, *L::gran(0, gr_) = v_par[j_])
      __syncthreads();
      uint32_t draw1, total = 0u, taken_w = 0u;
      double inv_t;
      bool covered;
      const bool on = policy_draw(*pp, ex, __builtin_amdgcn_readfirstlane(pe.local() == 0 ? meta.p1 : meta.p2),
                                  (uint32_t)__builtin_amdgcn_readfirstlane((int)ex.match_seed[g]), __builtin_amdgcn_readfirstlane(pe.local()),
                                  meta.steps, n_legal, covered, draw1, inv_t);
      int take = run_a;
      double take_s = run_s;
      if (covered) {   // (uniform)
        const double* row = b.scores + (size_t)g * MONSOON_NUM_ACTIONS;   // this decision's scores: the barriers above made them visible
        const SamplePick pk = sample_pick(row, ls.mask[0], ls.mask[1], ls.mask[2], run_s, inv_t, draw1, lane);
        total = pk.total;   // (0: the best score is NaN or infinite, the decision commits its arg-max)
        taken_w = !pk.total ? 0u : on ? pk.w : 1u << 24;
        if (on && pk.total && pk.pos != run_a) {   // (the arg-max's record is in v_best already: nothing to step)
          take = pk.pos;
          take_s = row[take];
          int fs = 0;
          if (lane == 0) {   // (the other lanes wait at the barrier, as in the bot's round)
            ce.step(take);
            fs = ce.fault();
            if (!fs && ce.observation_raises()) fs = FAULT_INT_CARD;
          }
          __syncthreads();
          cfault = __builtin_amdgcn_readfirstlane(fs);
          feat_ok = 0;   // the next decision computes its "before" side
          MSB_EACH_GRANULE(L::GPL, lane, v_best[j_] = *L::gran(0, gr_))
        }
      }
      log_explore(ex, lg, g, lane, meta.steps, run_a, on, take_s);
      log_sample(PlaySample{0.0, pp->weight_total, pp->taken_weight}, lg, g, lane, meta.steps, total, taken_w);
      run_a = take;
    }
    if constexpr (SAMPLE && !POLICY) {
      // column 0 is the current record again: the rule asks whose turn it is, and a sampled action is stepped from it
      __syncthreads();
      MSB_EACH_GRANULE(L::GPL, lane, *L::gran(0, gr_) = v_par[j_])
      __syncthreads();
      uint32_t draw1, total = 0u, taken_w = 0u;
      double slot_inv_t = 0.0;   // (ENV: the slot's own, read with the draw)
      bool on;
      if constexpr (ENV)
        on = env_sample_draw(*static_cast<const EnvSample*>(ee), g, meta.steps, n_legal, draw1, slot_inv_t);
      else
        on = sample_draw(ex, (uint32_t)__builtin_amdgcn_readfirstlane((int)ex.match_seed[g]), __builtin_amdgcn_readfirstlane(pe.local()),
                         meta.steps, n_legal, draw1);
      int take = run_a;
      double take_s = run_s;
      if (on) {   // (uniform)
        const double* row = b.scores + (size_t)g * MONSOON_NUM_ACTIONS;   // this decision's scores: the barriers above made them visible
        double inv_t;
        if constexpr (ENV) inv_t = slot_inv_t;
        else inv_t = sp->inv_temperature;
        const SamplePick pk = sample_pick(row, ls.mask[0], ls.mask[1], ls.mask[2], run_s, inv_t, draw1, lane);
        total = pk.total;   // (0: the best score is NaN or infinite, the decision commits its arg-max)
        taken_w = pk.w;
        if (pk.total && pk.pos != run_a) {   // (the arg-max's record is in v_best already: nothing to step)
          take = pk.pos;
          take_s = row[take];
          int fs = 0;
          if (lane == 0) {   // (the other lanes wait at the barrier, as in the bot's round)
            ce.step(take);
            fs = ce.fault();
            if (!fs && ce.observation_raises()) fs = FAULT_INT_CARD;
          }
          __syncthreads();
          cfault = __builtin_amdgcn_readfirstlane(fs);
          feat_ok = 0;   // the next decision computes its "before" side
          MSB_EACH_GRANULE(L::GPL, lane, v_best[j_] = *L::gran(0, gr_))
        }
      }
      if constexpr (ENV) {   // the env counts the slot's decisions whose draw said "sample", as k_env_opp_explore does
        if (on && lane == 0) atomicAdd(&ee->explored[g], 1u);
      } else {
        log_explore(ex, lg, g, lane, meta.steps, run_a, on, take_s);   // (greedy = the arg-max; run_s stays the decision's best score)
        log_sample(*sp, lg, g, lane, meta.steps, total, taken_w);
      }
      run_a = take;
    }
    MSB_COMMIT_BEST()
    if constexpr (EXPLORE) {   // the log keeps the arg-max next to what was committed; the env counts the slot's explored decisions
      if constexpr (LOG) log_explore(ex, lg, g, lane, meta.steps, run_a, xt->r >= 0, xt->r >= 0 ? xt->s : run_s);
      else if (xt->r >= 0 && lane == 0) atomicAdd(&ee->explored[g], 1u);   // (one wavefront plays a slot: no contention; nothing waits for it)
      if (xt->r >= 0) run_a = xt->a;   // (run_s stays the decision's best score)
    }
    if constexpr (LOG) log_step(lg, g, lane, meta.steps, run_a, run_s, n_legal);
    meta.steps++;
    meta.last_action = (uint8_t)run_a;
    meta.lookahead += (uint32_t)n_legal;   // every legal action is stepped exactly once; the commit re-executes nothing
    meta.decided++;   // statistics are per-game fields reduced on demand (k_stats): no same-address atomics here
    if (la_fault && !meta.la_fault) meta.la_fault = (uint8_t)la_fault;
    last_score = run_s;
    played++;
    PROF_MARK(7);   // commit + refill
    if (cfault) {
      // evo/fitness.py:208-210: an exception while applying the action ends the game as a draw
      meta.fault = (uint8_t)cfault;
      meta.result = -1;
      break;
    }
    if constexpr (ENV) {   // the env's end rules (env.inc env_after_step): the fault above, then a winner, then truncation
      if (pe.have_winner()) {
        meta.result = (int8_t)pe.winner_of(pe.pl_base(0), pe.pl_base(1));
        meta.flags |= 1;
        break;
      }
      if (pol.max_steps && meta.steps >= pol.max_steps) {
        meta.result = -1;
        meta.flags |= 2;   // truncated
        break;
      }
    }
  }
  if constexpr (ENV) {
    // still to play after `rounds` decisions: a USE that does nothing and costs nothing won the argmax and wins it for
    // ever from the identical state (the reference's loop only ends such a turn through max_turns)
    if (meta.result == -2 && pe.local() != pol.agent_side) {
      meta.result = -1;
      meta.fault = FAULT_OPP_BOUND;
    }
  }
  MSB_EACH_GRANULE(L::GPL, lane, grec[gr_] = v_par[j_])
#undef MSB_COMMIT_BEST
#undef MSB_TAKE_LANE
  if (lane == 0) {
    b.meta[g] = meta;
    if constexpr (ENV) {
      pol.steps[g] += (uint32_t)played;
      pol.lookahead[g] += meta.lookahead - lookahead0;
    } else if (b.best) {
      b.best[g] = last_score;
    }
  }
  PROF_FLUSH();
}

// Persistent wavefronts: the grid is what the GPU holds at once.  The games are split into POP_PARTS contiguous
// ranges; wavefront w works on range w % POP_PARTS (workgroups are dealt to the 8 XCDs round-robin, so a range stays
// on one XCD and its L2): it starts with the game given by its index and then pops further ones from the range's
// counter, the pop being issued before the current game is played so that its latency is hidden.  Games stay in
// index order -- neighbouring records, stream blocks and meta rows are touched together; sorting the games by
// expected cost was measured 5-8 % slower.  One counter per range, 128 bytes apart: atomics on ONE address serialise
// at ~25 ns each, which capped a launch at 65 536 x 25 ns (the same trap as per-game statistics counters; see
// k_stats).  Every wave reaches its exit (t >= hi): counters only grow.  b.pop[parity] is this launch's set; the
// other one is cleared for the next launch.  persistent = 0: one workgroup per game.  The host launches the
// persistent form only with at least POP_PARTS workgroups (a range without a wavefront would never be played).
// rounds = 1 is one decision round over the batch; rounds > max_turns plays every game to its end (rollouts).
// The launch plays games [g0, g0 + n).  A call split into sub-batches (monsoon_hip.hip launch_play) is SPLIT_MAX or
// fewer launches in flight at once, on a stream each: sub-batch `half` has its own pair of counter sets and its own
// overflow blocks behind those of the sub-batches before it, so no two launches in flight share or clear anything.
constexpr int POP_PARTS = 8, POP_STRIDE = 32, SPLIT_MAX = 2;
// The loop itself, for every persistent kernel (k_play, k_play_vs, k_play_log, k_play_explore, k_play_sample, k_play_policy, k_replay_log, k_env_opp, k_env_opp_explore): `mine` / `other` are this launch's counter
// set and the one it clears, the indices are [g0, g0 + n), and play(t) plays index t.  A wavefront whose range holds
// nothing for it leaves before enter(), which runs once ahead of the first game.
template <class Enter, class Play>
__device__ MSB_INL void pop_games(int* mine, int* other, const int n, const int g0, const int persistent, const int lane, Enter enter, Play play) {
  if (persistent && blockIdx.x == 0 && lane < POP_PARTS) other[lane * POP_STRIDE] = 0;
  const int part = blockIdx.x % POP_PARTS, rank = blockIdx.x / POP_PARTS;
  const int waves = ((int)gridDim.x - part + POP_PARTS - 1) / POP_PARTS;   // wavefronts working on this range
  const int lo = g0 + (persistent ? (int)((long long)n * part / POP_PARTS) : 0);
  const int hi = g0 + (persistent ? (int)((long long)n * (part + 1) / POP_PARTS) : n);
  int t = persistent ? lo + rank : g0 + (int)blockIdx.x;
  if (t >= hi) return;   // uniform
  enter();
  while (t < hi) {
    int nxt = 0x7fffffff;
    if (persistent && lane == 0) nxt = lo + waves + atomicAdd(&mine[part * POP_STRIDE], 1);
    play(t);
    __syncthreads();   // the LDS image is reused by the next game
    t = __builtin_amdgcn_readfirstlane(nxt);
  }
}

template <int U, int WPE>
__global__ void __launch_bounds__(64, WPE) k_play(DevBuffers b, int n, int max_turns, int rounds, int write_scores, int persistent, int parity,
                                                  int g0, int half) {
  const int lane = threadIdx.x;
  lds_init_wtab(b.wk_ovf + ((size_t)half * gridDim.x + blockIdx.x) * (U * OVF_WORDS));
  // one body for both forms (play_game is the whole rules core, inlined once): the non-persistent form is a "range" of
  // one game that is never refilled
  int* mine = b.pop + (2 * half + parity) * POP_PARTS * POP_STRIDE;
  int* other = b.pop + (2 * half + (parity ^ 1)) * POP_PARTS * POP_STRIDE;
  pop_games(mine, other, n, g0, persistent, lane, [] {},
            [&](const int t) { play_game<U, false>(b, t, lane, max_turns, rounds, write_scores, EnvPolicy{}); });
}

// What the host needs to launch a kernel that instantiates the look-ahead.
struct KernelOps {
  int lanes, wpe;           // U, W
  int lds_bytes;            // dynamic LDS of one workgroup
  hipError_t (*occupancy)(int* blocks_per_cu, int lds_bytes);
};
// ... one k_play variant (variant.hip defines one getter per instantiation)
struct VariantOps : KernelOps {
  void (*play)(int grid, int lds_bytes, hipStream_t stream, DevBuffers b, int n, int max_turns, int rounds, int write_scores, int persistent,
               int parity, int g0, int half);   // games [g0, g0 + n) as sub-batch `half` (k_play_vs: 0, 0 only)
};

// The build's default variant, the first entry of variants.def: k_play_vs, k_env_opp and k_env_after exist at this one only
// (each instantiation is a full compilation of the rules core) and serve every handle, whatever lanes_per_game it has.
#include "variants.def"
#define X(U, W) {U, W},
constexpr int kVariants[][2] = {MSB_VARIANTS(X)};
#undef X
constexpr int DEFAULT_U = kVariants[0][0], DEFAULT_W = kVariants[0][1];

// k_play_vs<DEFAULT_U, DEFAULT_W> (vs_expert.hip): the rollout kernel that knows the scripted bot.
const VariantOps* monsoon_vs_expert_ops();

// The three logging kernels, one launcher type: k_play_log<DEFAULT_U, DEFAULT_W> (play_log.hip) is k_play_vs that writes
// every committed step into a PlayLog, k_play_explore (play_explore.hip) is k_play_log whose decisions may explore
// (PlayExplore), k_play_sample (play_sample.hip) is k_play_log whose decisions may sample (PlayExplore's rule, PlaySample).
// k_play_policy (play_policy.hip) is k_play_sample whose rule is the moving row's own (PlayPolicy) -- a fourth logging kernel.
// The host hands every one of them the same PlayLogged; each file's stub passes its kernel the members it takes.
struct PlayLogged {
  PlayLog lg;
  PlayExplore ex;
  PlaySample sp;
  PlayPolicy pp;
};
struct LoggedOps : KernelOps {
  void (*play)(int grid, int lds_bytes, hipStream_t stream, DevBuffers b, int n, int max_turns, int rounds, int persistent, int parity,
               const PlayLogged& a);   // never split: the whole batch, the first pair of counter sets
};
const LoggedOps* monsoon_play_log_ops();
const LoggedOps* monsoon_play_explore_ops();
const LoggedOps* monsoon_play_sample_ops();
const LoggedOps* monsoon_play_policy_ops();

// k_sample_kat (play_sample.hip): sample_pick on caller-given rows (monsoon_debug_sample_kat), one wavefront per row.
void monsoon_sample_kat_launch(hipStream_t stream, int m, const double* scores, const int32_t* n_legal, const double* best, const double* inv_t,
                               const uint32_t* draw1, int32_t* out_rank, uint32_t* out_total, uint32_t* out_weight);

}  // namespace msbk
