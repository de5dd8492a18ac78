// env_opp.hip -- the vector env's heuristic opponent (monsoon_env_config.opponent = 2): k_env_opp plays the reference's
// HeuristicAgent for every slot on one of the env's two slot lists, with the hot kernel's decision loop
// (kernels.h play_game<U, true>).  One instantiation per record build, at the build's default variant (kernels.h
// DEFAULT_U, DEFAULT_W).
#include "env.h"

using namespace msbk;

namespace {

// Persistent wavefronts over list `list` (k_play's scheme, kernels.h pop_games: POP_PARTS ranges, one pop counter per
// range).  The list's length is read on the device, so the launch captures into a graph; the waves of an empty range
// leave at once -- most steps leave most waves nothing to do.  The two launches of an env step use list 0 and list 1, and
// with them counter sets 0 and 1: each launch clears the other set, so every replay of a captured step starts from
// cleared counters (monsoon_env_reset zeroes both).
template <int U, int WPE>
__global__ void __launch_bounds__(64, WPE) k_env_opp(DevBuffers b, EnvDev v, int list) {
  const int lane = threadIdx.x;
  const int n = __builtin_amdgcn_readfirstlane(v.opp_count[list * ENV_COUNT_STRIDE]);
  pop_games(
      v.opp_pop + list * POP_PARTS * POP_STRIDE, v.opp_pop + (list ^ 1) * POP_PARTS * POP_STRIDE, n, 0, 1, lane,
      [&] { lds_init_wtab(b.wk_ovf + (size_t)blockIdx.x * (U * OVF_WORDS)); },
      [&](const int t) {
        const int32_t* slots = v.opp_list + (size_t)list * v.cap;
        const EnvPolicy pol{v.opp_rows, v.bot_steps, v.opp_lookahead, v.agent_side, v.max_steps};
        const int g = __builtin_amdgcn_readfirstlane(slots[t]);
        play_game<U, true>(b, g, lane, 0x7fff, ENV_OPP_BOUND, 0, pol);
      });
}

hipError_t o_occupancy(int* blocks_per_cu, int lds_bytes) {
  return hipOccupancyMaxActiveBlocksPerMultiprocessor(blocks_per_cu, k_env_opp<DEFAULT_U, DEFAULT_W>, 64, lds_bytes);
}
void o_launch(int grid, int lds_bytes, hipStream_t stream, DevBuffers b, EnvDev v, int list) {
  hipLaunchKernelGGL((k_env_opp<DEFAULT_U, DEFAULT_W>), dim3(grid), dim3(64), lds_bytes, stream, b, v, list);
}
const EnvOppOps kOps = {{DEFAULT_U, DEFAULT_W, PlayLds<DEFAULT_U>::TOTAL, o_occupancy}, o_launch};

}  // namespace

const EnvOppOps* msbk::monsoon_env_opp_ops() { return &kOps; }
