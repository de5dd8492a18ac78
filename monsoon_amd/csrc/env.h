// env.h -- what the vector env's two translation units share: the device-side view of the env (EnvDev) and the launch
// table of the heuristic opponent's kernel (k_env_opp, env_opp.hip).  monsoon_hip.hip holds the env's lane-per-slot
// kernels (env.inc) and the host side.
#pragma once
#include "kernels.h"

namespace msbk {

constexpr int ENV_COUNT_STRIDE = 32;   // the two slot lists' counters, 128 bytes apart

struct EnvDev {
  monsoon_env_views v;      // the caller's views (any pointer but done may be null)
  const uint32_t* seed0;    // [n]
  uint8_t* decks;           // [n][24]: the decks of the slot's current episode
  const uint8_t* factions;  // [n][2]: episode 0's factions (later episodes: 0, 0)
  int32_t* episode;         // [n]: episodes completed
  uint8_t* mark;            // [n]: 1 = the slot's episode ended, k_env_reseed / k_env_init start the next one
  uint32_t* agent_steps;    // [n]: committed steps of the agent since monsoon_env_reset (monsoon_debug_counters word 6)
  uint32_t* bot_steps;      // [n]: ... of the opponent, scripted bot or heuristic (word 7)
  const uint8_t* pool;      // [128]
  // opponent 2 (the heuristic agent) only, else null
  const int32_t* opp_rows;  // [n]: the weight-table row of slot g's opponent
  int32_t* opp_list;        // [2][cap]: slots whose opponent is to play -- list 0 after the agent's step, list 1 new episodes
  int32_t* opp_count;       // [2 * ENV_COUNT_STRIDE]: the lists' lengths (list l at l * ENV_COUNT_STRIDE)
  int* opp_pop;             // [2][POP_PARTS * POP_STRIDE]: k_env_opp's pop counters, set l for list l
  uint32_t* opp_lookahead;  // [n]: the opponent's look-ahead transitions since monsoon_env_reset (monsoon_debug_counters word 16)
  int pool_n, opponent, agent_side, max_steps;
  uint32_t stride;
  int cap;                  // max_games: the stride of opp_list
};

// What a schedule-mode env (monsoon_env_reset without decks or pool after monsoon_env_set_schedule) needs on top: an
// argument of k_env_reseed_schedule alone.  EnvDev stays as it is, so every other env kernel keeps its argument block and
// its code (scripts/isa_diff.sh).  sched null = the loaded env is not in schedule mode.
struct EnvSched {
  const monsoon_deck_schedule* sched;   // the handle's schedule: read when an episode starts, rewritten between steps
  const uint32_t* mt_init;              // [624]: init_genrand(19650218), where every key mixing starts
  uint32_t* over;                       // episodes since monsoon_env_reset whose walk ran past the 624 outputs (monsoon_debug_counters word 17)
};

// k_env_opp<U, W> at the build's default variant (env_opp.hip): one wavefront per listed slot plays the opponent's turn.
struct EnvOppOps : KernelOps {
  void (*launch)(int grid, int lds_bytes, hipStream_t stream, DevBuffers b, EnvDev v, int list);
};
const EnvOppOps* monsoon_env_opp_ops();

// k_env_opp_explore<U, W> (env_opp_explore.hip): the same turn, epsilon-greedy by the rule the handle holds
// (kernels.h EnvExplore).  The host picks one of the tables at monsoon_env_reset.
struct EnvOppExploreOps : KernelOps {
  void (*launch)(int grid, int lds_bytes, hipStream_t stream, DevBuffers b, EnvDev v, int list, EnvExplore ee);
};
const EnvOppExploreOps* monsoon_env_opp_explore_ops();

// k_env_opp_sample<U, W> (env_opp_sample.hip): the same turn, sampling from the softmax over a decision's scores by the rule
// the handle holds (kernels.h EnvSample); b.scores is the handle's score table.  The host picks one of the three tables at
// monsoon_env_reset.
struct EnvOppSampleOps : KernelOps {
  void (*launch)(int grid, int lds_bytes, hipStream_t stream, DevBuffers b, EnvDev v, int list, EnvSample es);
};
const EnvOppSampleOps* monsoon_env_opp_sample_ops();

}  // namespace msbk
