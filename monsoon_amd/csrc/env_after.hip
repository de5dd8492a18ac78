// env_after.hip -- the afterstates of every legal action of every vector-env slot (monsoon_env_afterstates_dev,
// include/monsoon.h): k_env_after runs the hot kernel's look-ahead for a learner instead of a score (env_after.h
// after_slot<U>).  One instantiation per record build, at the build's default variant (kernels.h DEFAULT_U, DEFAULT_W).
#include "env_after.h"

using namespace msbk;

namespace {

// One wavefront per slot at a time: the grid is the wavefronts the GPU holds at once (at most n), and wavefront w takes
// slots w, w + grid, ...  Every slot is one decision's worth of look-ahead, so the slots are dealt out in advance: no pop
// counters (b.pop and the two sets of k_env_opp stay as they are), nothing to clear between the replays of a graph.
template <int U, int WPE>
__global__ void __launch_bounds__(64, WPE) k_env_after(DevBuffers b, monsoon_env_after o, int n, int max_after) {
  const int lane = threadIdx.x;
  lds_init_wtab(b.wk_ovf + (size_t)blockIdx.x * (U * OVF_WORDS));
  for (int g = blockIdx.x; g < n; g += gridDim.x) {
    after_slot<U>(b, o, max_after, g, lane);
    __syncthreads();   // the LDS image is reused by the next slot
  }
}

hipError_t a_occupancy(int* blocks_per_cu, int lds_bytes) {
  return hipOccupancyMaxActiveBlocksPerMultiprocessor(blocks_per_cu, k_env_after<DEFAULT_U, DEFAULT_W>, 64, lds_bytes);
}
void a_launch(int grid, int lds_bytes, hipStream_t stream, DevBuffers b, monsoon_env_after out, int n, int max_after) {
  hipLaunchKernelGGL((k_env_after<DEFAULT_U, DEFAULT_W>), dim3(grid), dim3(64), lds_bytes, stream, b, out, n, max_after);
}
const EnvAfterOps kOps = {{DEFAULT_U, DEFAULT_W, PlayLds<DEFAULT_U>::TOTAL, a_occupancy}, a_launch};

}  // namespace

const EnvAfterOps* msbk::monsoon_env_after_ops() { return &kOps; }
