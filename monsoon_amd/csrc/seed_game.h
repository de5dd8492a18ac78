// seed_game.h -- a game's numpy stream from a seed, by one wavefront: what k_seed, k_env_reseed (monsoon_hip.hip, env.inc)
// and k_env_determinize (env_determinize.hip) share.
#pragma once
#include "kernels.h"

namespace msbk {

// init_genrand(seed) into t[0..623] (a serial recurrence: lane 0)
__device__ inline void wave_init_genrand(MSB_AS_LDS uint32_t* t, uint32_t seed, int lane) {
  if (lane == 0) {
    uint32_t x = seed;
    t[0] = x;
    for (int i = 1; i < MT_N; i++) {
      x = 1812433253u * (x ^ (x >> 30)) + (uint32_t)i;
      t[i] = x;
    }
  }
  __syncthreads();
}

// game g's stream = RandomState(seed): the raw state and its first two tempered blocks (t = 624 words of LDS)
__device__ inline void wave_seed_game(const DevBuffers& b, int g, uint32_t seed, MSB_AS_LDS uint32_t* t, int lane) {
  wave_init_genrand(t, seed, lane);
  uint32_t* mt = b.rng_mt + (size_t)g * MT_N;
  for (int k = lane; k < MT_N; k += 64) mt[k] = t[k];
  __syncthreads();
  wave_refill(b, g, 0, t, lane);
  wave_refill(b, g, 1, t, lane);
}

}  // namespace msbk
