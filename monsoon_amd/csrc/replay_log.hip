// replay_log.hip -- logged games played again into (observation, action) rows (monsoon_replay_logged_dev,
// include/monsoon.h): k_replay_log commits one step per log entry and decides nothing (replay_log.h replay_game<U>).  One
// instantiation per record build, at the build's default variant (kernels.h DEFAULT_U, DEFAULT_W).
#include "replay_log.h"

using namespace msbk;

namespace {

// k_play_log's persistent grid, ranges and pop counters (kernels.h pop_games), the first pair of counter sets: a game has
// as many steps as its log has entries, 4 to 200 of them, so the games are popped, not dealt out in advance.
template <int U, int WPE>
__global__ void __launch_bounds__(64, WPE) k_replay_log(DevBuffers b, ReplayArgs ra, int n, int persistent, int parity) {
  const int lane = threadIdx.x;
  lds_init_wtab(b.wk_ovf + (size_t)blockIdx.x * (U * OVF_WORDS));
  pop_games(b.pop + parity * POP_PARTS * POP_STRIDE, b.pop + (parity ^ 1) * POP_PARTS * POP_STRIDE, n, 0, persistent, lane, [] {},
            [&](const int t) { replay_game<U>(b, ra, t, lane); });
}

hipError_t r_occupancy(int* blocks_per_cu, int lds_bytes) {
  return hipOccupancyMaxActiveBlocksPerMultiprocessor(blocks_per_cu, k_replay_log<DEFAULT_U, DEFAULT_W>, 64, lds_bytes);
}
void r_launch(int grid, int lds_bytes, hipStream_t stream, DevBuffers b, ReplayArgs ra, int n, int persistent, int parity) {
  hipLaunchKernelGGL((k_replay_log<DEFAULT_U, DEFAULT_W>), dim3(grid), dim3(64), lds_bytes, stream, b, ra, n, persistent, parity);
}
const ReplayOps kOps = {{DEFAULT_U, DEFAULT_W, PlayLds<DEFAULT_U>::TOTAL, r_occupancy}, r_launch};

}  // namespace

const ReplayOps* msbk::monsoon_replay_log_ops() { return &kOps; }
