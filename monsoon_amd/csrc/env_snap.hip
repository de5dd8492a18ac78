// env_snap.hip -- saving and restoring vector-env slots on the device (monsoon_env_save_dev / monsoon_env_load_dev,
// include/monsoon.h; entry layout in env_snap.h).  Pure data movement: one wavefront moves one entry at a time in 16-byte
// granules, lane l taking granules l, l + 64, ... so that every load and every store of the wave covers 1 024
// consecutive bytes on the slot side and on the entry side (at the seams between record, rng_mt and rng_out one
// instruction covers the end of one row and the start of the next).  A pass loads up to SNAP_PASS granules per lane
// before it stores the first, so a wave has a whole standard or extended entry in flight; the large entry's body (989
// granules) takes a second pass of 349, whose sixth load is live on 29 lanes.  The kernels touch no rules code: one
// instantiation per record build because SW and with it the layout differ.
#include "env_snap.h"

using namespace msbk;

namespace {

// Entry j = slot slots[j] (null: slot j).  A slot outside [0, n) leaves an entry with a zero header, which never loads.
__global__ void __launch_bounds__(64 * SNAP_WAVES) k_env_save(DevBuffers b, EnvDev v, int n, u32x4* entries, const int32_t* slots, int m,
                                                              uint32_t version) {
  SNAP_WAVE_LOOP() {
    const int g = slots ? __builtin_amdgcn_readfirstlane(slots[j]) : j;
    u32x4* ent = entries + (size_t)j * (SNAP_BYTES / 16);
    if (g < 0 || g >= n) {   // (uniform)
      if (lane == 0) ent[0] = u32x4{0u, 0u, 0u, 0u};
      continue;
    }
    if (lane == 0) {
      ent[0] = u32x4{SNAP_MAGIC, version, (uint32_t)SW, (uint32_t)v.episode[g]};
    } else if (lane < 3) {
      ent[lane] = ((const u32x4*)(b.meta + g))[lane - 1];
    } else if (lane < 5) {
      const uint32_t* d = (const uint32_t*)(v.decks + (size_t)g * 24);
      ent[lane] = lane == 3 ? u32x4{d[0], d[1], d[2], d[3]} : u32x4{d[4], d[5], 0u, 0u};
    }
    copy_body<true>(b, g, ent, lane);
  }
}

// Slot dst[j] (null: j) becomes entry src[j] (null: j).  The index checks and the header check are the wave's, not the
// lane's: src, dst, the header granule and the cursor word are read at one address by all lanes and made uniform.  Of the
// meta row the episode's fields are taken (result, fault, last_action, flags, steps, rng); the players' rows, the schedule
// index and the look-ahead statistics (p1, p2, match, decided, lookahead, la_fault) stay the destination's.
// (env_snap.h restates the checks and the head copy as snap_load_entry / snap_load_slot for k_env_load_det,
// env_determinize.hip; called from here they change this kernel's register allocation, and its code is kept as it was.)
__global__ void __launch_bounds__(64 * SNAP_WAVES) k_env_load(DevBuffers b, EnvDev v, int n, const u32x4* entries, int n_entries,
                                                              const int32_t* src, const int32_t* dst, int m, uint8_t* loaded, uint32_t version) {
  SNAP_WAVE_LOOP() {
    const int s = src ? __builtin_amdgcn_readfirstlane(src[j]) : j;
    const int g = dst ? __builtin_amdgcn_readfirstlane(dst[j]) : j;
    bool ok = s >= 0 && s < n_entries && g >= 0 && g < n;
    u32x4* ent = nullptr;
    uint32_t episode = 0;
    if (ok) {   // (uniform)
      ent = (u32x4*)entries + (size_t)s * (SNAP_BYTES / 16);
      const u32x4 hd = ent[0];
      const uint32_t magic = __builtin_amdgcn_readfirstlane(hd.x), ver = __builtin_amdgcn_readfirstlane(hd.y),
                     sw = __builtin_amdgcn_readfirstlane(hd.z);
      episode = __builtin_amdgcn_readfirstlane(hd.w);
      const uint32_t rng = __builtin_amdgcn_readfirstlane(ent[2].x);
      // a stream cursor outside the two resident blocks would be read out of bounds by the next step (as monsoon_state_load)
      ok = magic == SNAP_MAGIC && ver == version && sw == (uint32_t)SW && (rng & 0xffffu) < (uint32_t)(2 * MT_N) && (rng >> 17) == 0;
    }
    if (lane == 0) loaded[j] = ok ? 1 : 0;
    if (!ok) continue;   // (uniform)
    u32x4* mrow = (u32x4*)(b.meta + g);
    if (lane == 0) {
      v.episode[g] = (int32_t)episode;
    } else if (lane == 1) {
      const u32x4 e = ent[1], d = mrow[0];
      mrow[0] = u32x4{d.x, d.y, e.z, (e.w & 0xffffu) | (d.w & 0xffff0000u)};
    } else if (lane == 2) {
      const u32x4 e = ent[2], d = mrow[1];
      mrow[1] = u32x4{e.x, d.y, d.z, d.w};
    } else if (lane < 5) {
      const u32x4 e = ent[lane];
      uint32_t* d = (uint32_t*)(v.decks + (size_t)g * 24) + (lane == 3 ? 0 : 4);
      d[0] = e.x;
      d[1] = e.y;
      if (lane == 3) {
        d[2] = e.z;
        d[3] = e.w;
      }
    }
    copy_body<false>(b, g, ent, lane);
  }
}

hipError_t s_occupancy(int* blocks_per_cu, int lds_bytes) {
  int a = 0, c = 0;
  hipError_t e = hipOccupancyMaxActiveBlocksPerMultiprocessor(&a, k_env_save, 64 * SNAP_WAVES, lds_bytes);
  if (e != hipSuccess) return e;
  e = hipOccupancyMaxActiveBlocksPerMultiprocessor(&c, k_env_load, 64 * SNAP_WAVES, lds_bytes);
  *blocks_per_cu = a < c ? a : c;
  return e;
}
void s_save(int grid, hipStream_t stream, DevBuffers b, EnvDev v, int n, void* entries, const int32_t* slots, int m, uint32_t version) {
  hipLaunchKernelGGL(k_env_save, dim3(grid), dim3(64 * SNAP_WAVES), 0, stream, b, v, n, (u32x4*)entries, slots, m, version);
}
void s_load(int grid, hipStream_t stream, DevBuffers b, EnvDev v, int n, const void* entries, int n_entries, const int32_t* src,
            const int32_t* dst, int m, uint8_t* loaded, uint32_t version) {
  hipLaunchKernelGGL(k_env_load, dim3(grid), dim3(64 * SNAP_WAVES), 0, stream, b, v, n, (const u32x4*)entries, n_entries, src, dst, m, loaded,
                     version);
}
const EnvSnapOps kOps = {SNAP_BYTES, s_occupancy, s_save, s_load};

}  // namespace

const EnvSnapOps* msbk::monsoon_env_snap_ops() { return &kOps; }
