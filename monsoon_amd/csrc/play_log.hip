// play_log.hip -- rollouts that write down what they play (monsoon_rollout_logged, include/monsoon.h): k_play_log is
// k_play_vs with the logging form of the decision loop (kernels.h play_game<U, false, true, true>): lane 0 stores action,
// best score and legal count of every committed step into the call's PlayLog.  The bot's round is compiled in, so the one
// kernel serves schedules with and without the bot.  One instantiation per record build, at the build's default variant
// (kernels.h DEFAULT_U, DEFAULT_W).
#include "kernels.h"

using namespace msbk;

namespace {

// k_play_vs's persistent grid, ranges and pop counters (kernels.h pop_games): never split, the first pair of counter sets.
template <int U, int WPE>
__global__ void __launch_bounds__(64, WPE) k_play_log(DevBuffers b, int n, int max_turns, int rounds, int persistent, int parity, PlayLog lg) {
  const int lane = threadIdx.x;
  lds_init_wtab(b.wk_ovf + (size_t)blockIdx.x * (U * OVF_WORDS));
  pop_games(b.pop + parity * POP_PARTS * POP_STRIDE, b.pop + (parity ^ 1) * POP_PARTS * POP_STRIDE, n, 0, persistent, lane, [] {},
            [&](const int t) { play_game<U, false, true, true>(b, t, lane, max_turns, rounds, 0, EnvPolicy{}, lg); });
}

hipError_t log_occupancy(int* blocks_per_cu, int lds_bytes) {
  return hipOccupancyMaxActiveBlocksPerMultiprocessor(blocks_per_cu, k_play_log<DEFAULT_U, DEFAULT_W>, 64, lds_bytes);
}
void log_play(int grid, int lds_bytes, hipStream_t stream, DevBuffers b, int n, int max_turns, int rounds, int persistent, int parity,
              const PlayLogged& a) {
  hipLaunchKernelGGL((k_play_log<DEFAULT_U, DEFAULT_W>), dim3(grid), dim3(64), lds_bytes, stream, b, n, max_turns, rounds, persistent, parity, a.lg);
}
const LoggedOps kOps = {{DEFAULT_U, DEFAULT_W, PlayLds<DEFAULT_U>::TOTAL, log_occupancy}, log_play};

}  // namespace

const LoggedOps* msbk::monsoon_play_log_ops() { return &kOps; }
