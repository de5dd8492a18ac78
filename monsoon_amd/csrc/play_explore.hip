// play_explore.hip -- logged rollouts that explore (monsoon_rollout_explore, include/monsoon.h): k_play_explore is k_play_log
// with the exploring form of the decision loop (kernels.h play_game<U, false, true, true, true>): a decision whose draw --
// hash32 of the call's exploration seed, the match's seed and the committed-step index -- says so commits the r-th legal
// action instead of its arg-max, and lane 0 also stores the arg-max, the draw's verdict and the committed action's score.
// One instantiation per record build, at the build's default variant (kernels.h DEFAULT_U, DEFAULT_W).
#include "kernels.h"

using namespace msbk;

namespace {

// k_play_log's persistent grid, ranges and pop counters (kernels.h pop_games): never split, the first pair of counter sets.
template <int U, int WPE>
__global__ void __launch_bounds__(64, WPE) k_play_explore(DevBuffers b, int n, int max_turns, int rounds, int persistent, int parity, PlayLog lg,
                                                          PlayExplore ex) {
  const int lane = threadIdx.x;
  lds_init_wtab(b.wk_ovf + (size_t)blockIdx.x * (U * OVF_WORDS));
  ExploreTake xt;   // (scalars of the decision in flight; play_game declares nothing for them, kernels.h)
  pop_games(b.pop + parity * POP_PARTS * POP_STRIDE, b.pop + (parity ^ 1) * POP_PARTS * POP_STRIDE, n, 0, persistent, lane, [] {},
            [&](const int t) { play_game<U, false, true, true, true>(b, t, lane, max_turns, rounds, 0, EnvPolicy{}, lg, ex, &xt); });
}

hipError_t explore_occupancy(int* blocks_per_cu, int lds_bytes) {
  return hipOccupancyMaxActiveBlocksPerMultiprocessor(blocks_per_cu, k_play_explore<DEFAULT_U, DEFAULT_W>, 64, lds_bytes);
}
void explore_play(int grid, int lds_bytes, hipStream_t stream, DevBuffers b, int n, int max_turns, int rounds, int persistent, int parity,
                  const PlayLogged& a) {
  hipLaunchKernelGGL((k_play_explore<DEFAULT_U, DEFAULT_W>), dim3(grid), dim3(64), lds_bytes, stream, b, n, max_turns, rounds, persistent, parity, a.lg,
                     a.ex);
}
const LoggedOps kOps = {{DEFAULT_U, DEFAULT_W, PlayLds<DEFAULT_U>::TOTAL, explore_occupancy}, explore_play};

}  // namespace

const LoggedOps* msbk::monsoon_play_explore_ops() { return &kOps; }
