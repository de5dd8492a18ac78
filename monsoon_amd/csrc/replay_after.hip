// replay_after.hip -- logged games played again into rows that carry every legal action's afterstate
// (monsoon_replay_logged_after_dev, include/monsoon.h): k_replay_after is k_replay_log with after_slot's look-ahead run on the
// state of every kept row (replay_log.h replay_game<U, true>, env_after.h MSB_AFTER_STATE).  One instantiation per record
// build, at the build's default variant (kernels.h DEFAULT_U, DEFAULT_W).
#include "replay_log.h"

using namespace msbk;

namespace {

// k_replay_log's persistent grid, ranges and pop counters (kernels.h pop_games), the first pair of counter sets.
template <int U, int WPE>
__global__ void __launch_bounds__(64, WPE) k_replay_after(DevBuffers b, ReplayArgs ra, monsoon_replay_after o, int max_after, int n, int persistent,
                                                          int parity) {
  const int lane = threadIdx.x;
  lds_init_wtab(b.wk_ovf + (size_t)blockIdx.x * (U * OVF_WORDS));
  // per entry a row of the replay is a slot of monsoon_env_afterstates_dev
  const monsoon_env_after oa = {o.n_legal, o.action, o.status, o.reward, o.winner, o.features, o.obs, o.before_features};
  pop_games(b.pop + parity * POP_PARTS * POP_STRIDE, b.pop + (parity ^ 1) * POP_PARTS * POP_STRIDE, n, 0, persistent, lane, [] {},
            [&](const int t) { replay_game<U, true>(b, ra, t, lane, oa, o.chosen, max_after); });
}

hipError_t ra_occupancy(int* blocks_per_cu, int lds_bytes) {
  return hipOccupancyMaxActiveBlocksPerMultiprocessor(blocks_per_cu, k_replay_after<DEFAULT_U, DEFAULT_W>, 64, lds_bytes);
}
void ra_launch(int grid, int lds_bytes, hipStream_t stream, DevBuffers b, ReplayArgs ra, monsoon_replay_after after, int max_after, int n,
               int persistent, int parity) {
  hipLaunchKernelGGL((k_replay_after<DEFAULT_U, DEFAULT_W>), dim3(grid), dim3(64), lds_bytes, stream, b, ra, after, max_after, n, persistent,
                     parity);
}
const ReplayAfterOps kOps = {{DEFAULT_U, DEFAULT_W, PlayLds<DEFAULT_U>::TOTAL, ra_occupancy}, ra_launch};

}  // namespace

const ReplayAfterOps* msbk::monsoon_replay_after_ops() { return &kOps; }
