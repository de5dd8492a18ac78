// env_determinize.hip -- loading saved vector-env slots as determinizations (monsoon_env_load_determinized_dev,
// include/monsoon.h): the fork of an information-set search, in which what the observer cannot see is drawn again.  Two
// kernels between which the host launches nothing, and k_env_view (env.inc) after them:
//
//   k_env_load_det     k_env_load (env_snap.hip; the same checks and the same copy, env_snap.h) that also skips a pair
//                      whose observer byte names no side.
//   k_env_determinize  one wavefront per loaded pair whose episode is running: the hidden side's hand is drawn again from
//                      its hand and deck (MONSOON_DET_HAND, standard record; the rule is determinize.h), then the slot's
//                      stream becomes RandomState(seed) with the cursor at its start (wave_seed_game, as k_env_reseed).
//
// The re-draw reads the hidden player's block from the ENTRY, which nothing writes, and stores into the slot that the
// launch before filled: lane l < L holds place l of A (the movable hand entries, then the deck), finds the entry that ends
// there from the wave's swaps and moves that one word.  No lane reads what another lane of the launch wrote.
// The serial init_genrand recurrence (lane 0, 623 dependent steps) is most of the kernel's time, as in k_env_reseed.
#include "determinize.h"
#include "env_snap.h"
#include "seed_game.h"

using namespace msbk;

namespace {

__global__ void __launch_bounds__(64 * SNAP_WAVES) k_env_load_det(DevBuffers b, EnvDev v, int n, const u32x4* entries, int n_entries,
                                                                  const int32_t* src, const int32_t* dst, int m, const uint8_t* observers,
                                                                  uint8_t* loaded, uint32_t version) {
  SNAP_WAVE_LOOP() {
    const int s = src ? __builtin_amdgcn_readfirstlane(src[j]) : j;
    const int g = dst ? __builtin_amdgcn_readfirstlane(dst[j]) : j;
    const int o = observers ? __builtin_amdgcn_readfirstlane((int)observers[j]) : 255;
    uint32_t episode = 0;
    u32x4* ent = (o == 0 || o == 1 || o == 255) ? snap_load_entry(entries, n_entries, s, g, n, version, episode) : nullptr;   // (uniform)
    if (lane == 0) loaded[j] = ent ? 1 : 0;
    if (!ent) continue;   // (uniform)
    snap_load_slot(b, v, g, ent, episode, lane);
  }
}

#if !(defined(MSB_EXT) && MSB_EXT)
static_assert(HAND_CAP == DET_HAND_MAX && DECK_CAP == DET_DECK_MAX, "determinize.h restates the standard record's caps");
static_assert(P_HAND_N / 4 == P_DECK_N / 4 && P_HAND % 4 == 0 && P_DECK == P_HAND + 4 * HAND_CAP && P_AGE == P_DECK + 4 * DECK_CAP,
              "hand and deck are consecutive 4-byte entries; both counts sit in one word");

// The word of the player's block that holds place a of A: the a-th movable hand entry, then the deck in order.
__device__ MSB_INL int det_word(uint32_t movable, const int k, const int a) {
  if (a >= k) return P_DECK / 4 + (a - k);
  for (int i = 0; i < a; i++) movable &= movable - 1;
  return P_HAND / 4 + __builtin_ctz(movable);
}

// Player 1 - o of the entry's record: its movable hand entries and its deck, re-dealt into slot g by the rule's swaps.
__device__ MSB_INL void redraw_hand(const DevBuffers& b, const int g, const u32x4* ent, int o, const uint32_t seed, const int lane) {
  const uint32_t* rec = (const uint32_t*)(ent + SNAP_HEAD_G);
  if (o == 255) o = (int)(__builtin_amdgcn_readfirstlane(rec[H_TOPLAY / 4]) >> (8 * (H_TOPLAY & 3))) & 1;
  const int side = 1 - o;
  const uint32_t* pw = rec + (OFF_PL + PL_SIZE * side) / 4;
  const uint32_t counts = __builtin_amdgcn_readfirstlane(pw[P_HAND_N / 4]);
  const int hn = (int)(counts >> (8 * (P_HAND_N & 3))) & 0xff, dn = (int)(counts >> (8 * (P_DECK_N & 3))) & 0xff;
  if (hn > HAND_CAP || dn > DECK_CAP) return;   // (uniform) no record of this library: the copy stands
  const uint32_t flags = lane < hn ? (pw[P_HAND / 4 + lane] >> 16) & 0xffu : 0u;   // entry = {card, cost, flags, x}
  const uint32_t movable = (uint32_t)__ballot(lane < hn && !(flags & (uint32_t)(CF_ALIAS | CF_STR)));
  const int k = __popc(movable), L = k + dn;
  if (k == 0 || L <= 1) return;   // (uniform)
  int j[DET_HAND_MAX];
  det_swaps(seed, k, dn, j);   // wave-uniform values
  if (lane < L) {
    uint32_t* out = b.state + (size_t)g * SW + (OFF_PL + PL_SIZE * side) / 4;
    out[det_word(movable, k, lane)] = pw[det_word(movable, k, det_source(j, k, lane))];
  }
}
#endif

// Grid m, a wavefront per pair.  loaded is k_env_load_det's: a set byte says that src and dst are in range.
__global__ void __launch_bounds__(64) k_env_determinize(DevBuffers b, const u32x4* entries, const int32_t* src, const int32_t* dst, int m,
                                                         const uint32_t* seeds, const uint8_t* observers, int what, const uint8_t* loaded) {
  __shared__ uint32_t mt[MT_N];
  const int lane = threadIdx.x, j = blockIdx.x;
  if (j >= m || !__builtin_amdgcn_readfirstlane((int)loaded[j])) return;   // (uniform)
  const int s = src ? __builtin_amdgcn_readfirstlane(src[j]) : j;
  const int g = dst ? __builtin_amdgcn_readfirstlane(dst[j]) : j;
  const u32x4* ent = entries + (size_t)s * (SNAP_BYTES / 16);
  // GameMeta.result: an episode that has ended, or whose end is pending, is loaded as it is
  if ((int8_t)(__builtin_amdgcn_readfirstlane(ent[1].z) & 0xffu) != -2) return;   // (uniform)
  const uint32_t seed = __builtin_amdgcn_readfirstlane(seeds[j]);
#if !(defined(MSB_EXT) && MSB_EXT)
  if (what & MONSOON_DET_HAND) redraw_hand(b, g, ent, observers ? __builtin_amdgcn_readfirstlane((int)observers[j]) : 255, seed, lane);
#endif
  wave_seed_game(b, g, seed, (MSB_AS_LDS uint32_t*)mt, lane);
  if (lane == 0) b.meta[g].rng = 0;   // block 0, cursor 0
}

void d_load(int grid, hipStream_t stream, DevBuffers b, EnvDev v, int n, const void* entries, int n_entries, const int32_t* src,
            const int32_t* dst, int m, const uint8_t* observers, uint8_t* loaded, uint32_t version) {
  hipLaunchKernelGGL(k_env_load_det, dim3(grid), dim3(64 * SNAP_WAVES), 0, stream, b, v, n, (const u32x4*)entries, n_entries, src, dst, m,
                     observers, loaded, version);
}
void d_determinize(hipStream_t stream, DevBuffers b, const void* entries, const int32_t* src, const int32_t* dst, int m, const uint32_t* seeds,
                   const uint8_t* observers, int what, const uint8_t* loaded) {
  hipLaunchKernelGGL(k_env_determinize, dim3(m), dim3(64), 0, stream, b, (const u32x4*)entries, src, dst, m, seeds, observers, what, loaded);
}
const EnvDetOps kOps = {d_load, d_determinize};

}  // namespace

const EnvDetOps* msbk::monsoon_env_det_ops() { return &kOps; }
