// play_policy.hip -- logged rollouts whose exploration is the moving individual's own (monsoon_rollout_policies,
// include/monsoon.h): k_play_policy is k_play_sample with the per-row form of the decision loop (kernels.h play_game<U, false,
// true, true, false, true, true>): a heuristic decision reads the threshold and the inverse temperature of the weight row
// that moves -- the row whose weights score it -- and every decision that rule covers weighs its actions (kernels.h
// sample_pick), drawn or not, so that lane 0 stores the sum of the weights and the committed action's weight for each of
// them: the behaviour probability of every row of the log.  One instantiation per record build, at the build's default
// variant (kernels.h DEFAULT_U, DEFAULT_W).
#include "kernels.h"

using namespace msbk;

namespace {

// k_play_log's persistent grid, ranges and pop counters (kernels.h pop_games): never split, the first pair of counter sets.
template <int U, int WPE>
__global__ void __launch_bounds__(64, WPE) k_play_policy(DevBuffers b, int n, int max_turns, int rounds, int persistent, int parity, PlayLog lg,
                                                         PlayExplore ex, PlayPolicy pp) {
  const int lane = threadIdx.x;
  lds_init_wtab(b.wk_ovf + (size_t)blockIdx.x * (U * OVF_WORDS));
  pop_games(b.pop + parity * POP_PARTS * POP_STRIDE, b.pop + (parity ^ 1) * POP_PARTS * POP_STRIDE, n, 0, persistent, lane, [] {}, [&](const int t) {
    play_game<U, false, true, true, false, true, true>(b, t, lane, max_turns, rounds, 0, EnvPolicy{}, lg, ex, nullptr, nullptr, nullptr, &pp);
  });
}

hipError_t policy_occupancy(int* blocks_per_cu, int lds_bytes) {
  return hipOccupancyMaxActiveBlocksPerMultiprocessor(blocks_per_cu, k_play_policy<DEFAULT_U, DEFAULT_W>, 64, lds_bytes);
}
void policy_play(int grid, int lds_bytes, hipStream_t stream, DevBuffers b, int n, int max_turns, int rounds, int persistent, int parity,
                 const PlayLogged& a) {
  hipLaunchKernelGGL((k_play_policy<DEFAULT_U, DEFAULT_W>), dim3(grid), dim3(64), lds_bytes, stream, b, n, max_turns, rounds, persistent, parity, a.lg,
                     a.ex, a.pp);
}
const LoggedOps kOps = {{DEFAULT_U, DEFAULT_W, PlayLds<DEFAULT_U>::TOTAL, policy_occupancy}, policy_play};

}  // namespace

const LoggedOps* msbk::monsoon_play_policy_ops() { return &kOps; }
