// play_sample.hip -- logged rollouts that sample (monsoon_rollout_sample, include/monsoon.h): k_play_sample is k_play_log
// with the sampling form of the decision loop (kernels.h play_game<U, false, true, true, false, true>): a decision whose
// draw -- hash32 of the call's exploration seed, the match's seed and the committed-step index -- says so commits an action
// drawn from the softmax over the decision's scores (sample_weight.h weight24, kernels.h sample_pick) instead of its
// arg-max, and lane 0 also stores the arg-max, the draw's verdict, the committed action's score, the sum of the weights and
// the committed action's weight.  One instantiation per record build, at the build's default variant (kernels.h DEFAULT_U,
// DEFAULT_W).  k_sample_kat puts sample_pick itself to caller-given rows (monsoon_debug_sample_kat).
#include "kernels.h"

using namespace msbk;

namespace {

// k_play_log's persistent grid, ranges and pop counters (kernels.h pop_games): never split, the first pair of counter sets.
template <int U, int WPE>
__global__ void __launch_bounds__(64, WPE) k_play_sample(DevBuffers b, int n, int max_turns, int rounds, int persistent, int parity, PlayLog lg,
                                                         PlayExplore ex, PlaySample sp) {
  const int lane = threadIdx.x;
  lds_init_wtab(b.wk_ovf + (size_t)blockIdx.x * (U * OVF_WORDS));
  pop_games(b.pop + parity * POP_PARTS * POP_STRIDE, b.pop + (parity ^ 1) * POP_PARTS * POP_STRIDE, n, 0, persistent, lane, [] {},
            [&](const int t) { play_game<U, false, true, true, false, true>(b, t, lane, max_turns, rounds, 0, EnvPolicy{}, lg, ex, nullptr, nullptr, &sp); });
}

// Row i: the actions are ranks 0 .. n_legal[i] - 1 of a legal list, scores[i][j] the j-th one's; one wavefront per row.
__global__ void __launch_bounds__(64) k_sample_kat(int m, const double* scores, const int32_t* n_legal, const double* best, const double* inv_t,
                                                   const uint32_t* draw1, int32_t* out_rank, uint32_t* out_total, uint32_t* out_weight) {
  const int i = blockIdx.x, lane = threadIdx.x;
  if (i >= m) return;
  const int n = n_legal[i] < 0 ? 0 : n_legal[i] > MONSOON_NUM_ACTIONS ? MONSOON_NUM_ACTIONS : n_legal[i];
  const auto low = [](const int k) { return k <= 0 ? 0ull : k >= 64 ? ~0ull : (1ull << k) - 1ull; };   // the k lowest bits
  const SamplePick pk = sample_pick(scores + (size_t)i * MONSOON_NUM_ACTIONS, uni64(low(n)), uni64(low(n - 64)), uni64(low(n - 128)), best[i], inv_t[i],
                                    draw1[i], lane);
  if (lane == 0) {
    out_rank[i] = pk.pos;
    out_total[i] = pk.total;
    out_weight[i] = pk.w;
  }
}

hipError_t sample_occupancy(int* blocks_per_cu, int lds_bytes) {
  return hipOccupancyMaxActiveBlocksPerMultiprocessor(blocks_per_cu, k_play_sample<DEFAULT_U, DEFAULT_W>, 64, lds_bytes);
}
void sample_play(int grid, int lds_bytes, hipStream_t stream, DevBuffers b, int n, int max_turns, int rounds, int persistent, int parity,
                 const PlayLogged& a) {
  hipLaunchKernelGGL((k_play_sample<DEFAULT_U, DEFAULT_W>), dim3(grid), dim3(64), lds_bytes, stream, b, n, max_turns, rounds, persistent, parity, a.lg,
                     a.ex, a.sp);
}
const LoggedOps kOps = {{DEFAULT_U, DEFAULT_W, PlayLds<DEFAULT_U>::TOTAL, sample_occupancy}, sample_play};

}  // namespace

const LoggedOps* msbk::monsoon_play_sample_ops() { return &kOps; }
void msbk::monsoon_sample_kat_launch(hipStream_t stream, int m, const double* scores, const int32_t* n_legal, const double* best, const double* inv_t,
                                     const uint32_t* draw1, int32_t* out_rank, uint32_t* out_total, uint32_t* out_weight) {
  hipLaunchKernelGGL(k_sample_kat, dim3(m), dim3(64), 0, stream, m, scores, n_legal, best, inv_t, draw1, out_rank, out_total, out_weight);
}
