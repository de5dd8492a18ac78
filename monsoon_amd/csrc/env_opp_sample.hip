// env_opp_sample.hip -- the vector env's heuristic opponent, sampling (monsoon_env_set_opponent_sample, include/monsoon.h):
// k_env_opp_sample is k_env_opp with the env's sampling form of the decision loop (kernels.h
// play_game<U, true, false, false, false, true>): a decision whose draw -- k_env_opp_explore's, hash32 of the rule's seed, the
// slot's episode seed and the episode's committed-step index, against the slot's own threshold -- says so commits an action
// drawn from the softmax over the decision's scores at the slot's own inverse temperature (sample_weight.h weight24,
// kernels.h sample_pick) instead of its arg-max, and lane 0 counts it for the slot.  Every candidate's score is parked in the
// slot's row of the handle's score table (b.scores, which launch_env_opp hands to this kernel alone).  The rule's words, the
// thresholds and the inverse temperatures are read from device memory at every decision, so the host retunes a captured
// step between replays.  One instantiation per record build, at the build's default variant (kernels.h DEFAULT_U,
// DEFAULT_W); an env that was reset with a sampling rule launches it where it would launch k_env_opp.
#include "env.h"

using namespace msbk;

namespace {

// k_env_opp's persistent grid, slot lists and pop-counter sets (env_opp.hip): list `list`, counter set `list`, the other
// set cleared.
template <int U, int WPE>
__global__ void __launch_bounds__(64, WPE) k_env_opp_sample(DevBuffers b, EnvDev v, int list, EnvSample es) {
  const int lane = threadIdx.x;
  const int n = __builtin_amdgcn_readfirstlane(v.opp_count[list * ENV_COUNT_STRIDE]);
  pop_games(
      v.opp_pop + list * POP_PARTS * POP_STRIDE, v.opp_pop + (list ^ 1) * POP_PARTS * POP_STRIDE, n, 0, 1, lane,
      [&] { lds_init_wtab(b.wk_ovf + (size_t)blockIdx.x * (U * OVF_WORDS)); },
      [&](const int t) {
        const int32_t* slots = v.opp_list + (size_t)list * v.cap;
        const EnvPolicy pol{v.opp_rows, v.bot_steps, v.opp_lookahead, v.agent_side, v.max_steps};
        const int g = __builtin_amdgcn_readfirstlane(slots[t]);
        play_game<U, true, false, false, false, true>(b, g, lane, 0x7fff, ENV_OPP_BOUND, 0, pol, PlayLog{}, PlayExplore{}, nullptr, &es);
      });
}

hipError_t s_occupancy(int* blocks_per_cu, int lds_bytes) {
  return hipOccupancyMaxActiveBlocksPerMultiprocessor(blocks_per_cu, k_env_opp_sample<DEFAULT_U, DEFAULT_W>, 64, lds_bytes);
}
void s_launch(int grid, int lds_bytes, hipStream_t stream, DevBuffers b, EnvDev v, int list, EnvSample es) {
  hipLaunchKernelGGL((k_env_opp_sample<DEFAULT_U, DEFAULT_W>), dim3(grid), dim3(64), lds_bytes, stream, b, v, list, es);
}
const EnvOppSampleOps kOps = {{DEFAULT_U, DEFAULT_W, PlayLds<DEFAULT_U>::TOTAL, s_occupancy}, s_launch};

}  // namespace

const EnvOppSampleOps* msbk::monsoon_env_opp_sample_ops() { return &kOps; }
