// vs_expert.hip -- rollouts in which either side of a match may be the reference's scripted bot
// (monsoon_rollout_vs_expert, include/monsoon.h): k_play_vs is k_play with the bot round of the decision loop compiled in
// (kernels.h play_game<U, false, true>).  One instantiation per record build, at the build's default variant (the first
// entry of variants.def): each instantiation is a full compilation of the rules core.  It serves every handle, whatever
// lanes_per_game it was opened with, and is launched through the same table as a k_play variant.
#include "kernels.h"

using namespace msbk;

namespace {

#include "variants.def"
#define X(U, W) {U, W},
constexpr int kVariants[][2] = {MSB_VARIANTS(X)};
#undef X
constexpr int VS_U = kVariants[0][0], VS_W = kVariants[0][1];

// k_play's persistent grid, ranges and pop counters (kernels.h): the two kernels alternate over the same two counter sets.
template <int U, int WPE>
__global__ void __launch_bounds__(64, WPE) k_play_vs(DevBuffers b, int n, int max_turns, int rounds, int write_scores, int persistent, int parity) {
  const int lane = threadIdx.x;
  lds_init_wtab(b.wk_ovf + (size_t)blockIdx.x * (U * OVF_WORDS));
  int* mine = b.pop + parity * POP_PARTS * POP_STRIDE;
  int* other = b.pop + (parity ^ 1) * POP_PARTS * POP_STRIDE;
  if (persistent && blockIdx.x == 0 && lane < POP_PARTS) other[lane * POP_STRIDE] = 0;
  const int part = blockIdx.x % POP_PARTS, rank = blockIdx.x / POP_PARTS;
  const int waves = ((int)gridDim.x - part + POP_PARTS - 1) / POP_PARTS;   // wavefronts working on this range
  const int lo = persistent ? (int)((long long)n * part / POP_PARTS) : 0;
  const int hi = persistent ? (int)((long long)n * (part + 1) / POP_PARTS) : n;
  int t = persistent ? lo + rank : (int)blockIdx.x;
  while (t < hi) {
    int nxt = 0x7fffffff;
    if (persistent && lane == 0) nxt = lo + waves + atomicAdd(&mine[part * POP_STRIDE], 1);
    play_game<U, false, true>(b, t, lane, max_turns, rounds, write_scores, EnvPolicy{});
    __syncthreads();   // the LDS image is reused by the next game
    t = __builtin_amdgcn_readfirstlane(nxt);
  }
}

hipError_t vs_occupancy(int* blocks_per_cu, int lds_bytes) {
  return hipOccupancyMaxActiveBlocksPerMultiprocessor(blocks_per_cu, k_play_vs<VS_U, VS_W>, 64, lds_bytes);
}
void vs_play(int grid, int lds_bytes, hipStream_t stream, DevBuffers b, int n, int max_turns, int rounds, int write_scores, int persistent,
             int parity, int /*g0*/, int /*half*/) {   // never split: the whole batch, the first pair of counter sets
  hipLaunchKernelGGL((k_play_vs<VS_U, VS_W>), dim3(grid), dim3(64), lds_bytes, stream, b, n, max_turns, rounds, write_scores, persistent, parity);
}
const VariantOps kOps = {VS_U, VS_W, PlayLds<VS_U>::TOTAL, vs_occupancy, vs_play};

}  // namespace

const VariantOps* msbk::monsoon_vs_expert_ops() { return &kOps; }
