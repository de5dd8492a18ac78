// vs_expert.hip -- rollouts in which either side of a match may be the reference's scripted bot
// (monsoon_rollout_vs_expert, include/monsoon.h): k_play_vs is k_play with the bot round of the decision loop compiled in
// (kernels.h play_game<U, false, true>).  One instantiation per record build, at the build's default variant (kernels.h
// DEFAULT_U, DEFAULT_W), launched through the same table as a k_play variant.
#include "kernels.h"

using namespace msbk;

namespace {

// k_play's persistent grid, ranges and pop counters (kernels.h pop_games): the two kernels alternate over the same two
// counter sets.
template <int U, int WPE>
__global__ void __launch_bounds__(64, WPE) k_play_vs(DevBuffers b, int n, int max_turns, int rounds, int write_scores, int persistent, int parity) {
  const int lane = threadIdx.x;
  lds_init_wtab(b.wk_ovf + (size_t)blockIdx.x * (U * OVF_WORDS));
  pop_games(b.pop + parity * POP_PARTS * POP_STRIDE, b.pop + (parity ^ 1) * POP_PARTS * POP_STRIDE, n, 0, persistent, lane, [] {},
            [&](const int t) { play_game<U, false, true>(b, t, lane, max_turns, rounds, write_scores, EnvPolicy{}); });
}

hipError_t vs_occupancy(int* blocks_per_cu, int lds_bytes) {
  return hipOccupancyMaxActiveBlocksPerMultiprocessor(blocks_per_cu, k_play_vs<DEFAULT_U, DEFAULT_W>, 64, lds_bytes);
}
void vs_play(int grid, int lds_bytes, hipStream_t stream, DevBuffers b, int n, int max_turns, int rounds, int write_scores, int persistent,
             int parity, int /*g0*/, int /*half*/) {   // never split: the whole batch, the first pair of counter sets
  hipLaunchKernelGGL((k_play_vs<DEFAULT_U, DEFAULT_W>), dim3(grid), dim3(64), lds_bytes, stream, b, n, max_turns, rounds, write_scores, persistent,
                     parity);
}
const VariantOps kOps = {{DEFAULT_U, DEFAULT_W, PlayLds<DEFAULT_U>::TOTAL, vs_occupancy}, vs_play};

}  // namespace

const VariantOps* msbk::monsoon_vs_expert_ops() { return &kOps; }
