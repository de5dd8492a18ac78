// env_snap.h -- saved vector-env slots (monsoon_env_save_dev / monsoon_env_load_dev, include/monsoon.h): the layout of an
// entry and the launch table of the two copy kernels (k_env_save / k_env_load, env_snap.hip).  The views of the loaded
// slots are written by k_env_view (env.inc), lane per slot, after the copy.
//
// An entry is SNAP_BYTES of device memory, every part on a 16-byte boundary:
//
//   [0, 16)     header: SNAP_MAGIC, monsoon_version(), SW, the slot's episode count
//   [16, 48)    the GameMeta row
//   [48, 80)    the 24 deck bytes of the current episode (EnvDev::decks), 8 bytes of zero
//   [80, ..)    the record (STATE_BYTES), the raw stream state (rng_mt, 2 496 bytes), the two tempered blocks (rng_out,
//               4 992 bytes)
//
// The standard record gives 8 320 bytes = 520 granules.  On the slot side the record, rng_mt and rng_out rows and the
// meta row are whole 16-byte granules too (STATE_BYTES, 2 496, 4 992 and 32 are multiples of 16 and the arrays come from
// hipMalloc); the deck row (24 bytes) is 4-byte aligned only and moves as six words.
#pragma once
#include <cstddef>

#include "env.h"

namespace msbk {

constexpr uint32_t SNAP_MAGIC = 0x50414e53u;   // "SNAP"
constexpr int SNAP_META = 16, SNAP_DECKS = 48, SNAP_REC = 80;
constexpr int SNAP_HEAD_G = SNAP_REC / 16;             // granules of header, meta row and decks
constexpr int SNAP_MT_G = MT_N * 4 / 16, SNAP_OUT_G = RNG_WORDS * 4 / 16;
constexpr int SNAP_BODY_G = SG + SNAP_MT_G + SNAP_OUT_G;   // granules of record and stream
constexpr int SNAP_BYTES = (SNAP_HEAD_G + SNAP_BODY_G) * 16;
constexpr int SNAP_WAVES = 4;                          // wavefronts of a workgroup, an entry each at a time
static_assert(MT_N * 4 % 16 == 0 && RNG_WORDS * 4 % 16 == 0 && sizeof(GameMeta) == 32, "whole granules");
static_assert(offsetof(GameMeta, result) == 8 && offsetof(GameMeta, steps) == 12 && offsetof(GameMeta, decided) == 14 &&
                  offsetof(GameMeta, rng) == 16,
              "k_env_load merges the meta row by words");

// ---- device side, shared by the copy kernels (env_snap.hip) and the determinizing load (env_determinize.hip) ----
static_assert(SW * 4 == STATE_BYTES, "the record's stride is the record");
constexpr int SNAP_PASS = 10;   // granules per lane and pass: 9 cover the standard body (515), 10 the extended one (618); large: 2 passes

// Body granule i of slot g: the record, then rng_mt, then rng_out.
__device__ MSB_INL u32x4* slot_granule(const DevBuffers& b, const int g, const int i) {
  uint32_t* p = i < SG                 ? b.state + (size_t)g * SW + 4 * i
                : i < SG + SNAP_MT_G ? b.rng_mt + (size_t)g * MT_N + 4 * (i - SG)
                                     : b.rng_out + (size_t)g * RNG_WORDS + 4 * (i - SG - SNAP_MT_G);
  return (u32x4*)p;
}

// SAVE: body of slot g -> ent; else ent -> body of slot g.
template <bool SAVE>
__device__ MSB_INL void copy_body(const DevBuffers& b, const int g, u32x4* ent, const int lane) {
  u32x4* body = ent + SNAP_HEAD_G;
  for (int base = 0; base < SNAP_BODY_G; base += 64 * SNAP_PASS) {
    u32x4 r[SNAP_PASS];
#pragma unroll
    for (int j = 0; j < SNAP_PASS; j++) {
      const int i = base + 64 * j + lane;
      if (i < SNAP_BODY_G) r[j] = SAVE ? *slot_granule(b, g, i) : body[i];
    }
#pragma unroll
    for (int j = 0; j < SNAP_PASS; j++) {
      const int i = base + 64 * j + lane;
      if (i < SNAP_BODY_G) {
        if (SAVE) body[i] = r[j];
        else *slot_granule(b, g, i) = r[j];
      }
    }
  }
}

#define SNAP_WAVE_LOOP()                                                                                \
  const int lane = (int)threadIdx.x & 63;                                                               \
  const int wave0 = __builtin_amdgcn_readfirstlane((int)blockIdx.x * SNAP_WAVES + ((int)threadIdx.x >> 6)); \
  const int waves = (int)gridDim.x * SNAP_WAVES;                                                        \
  for (int j = wave0; j < m; j += waves)

// snap_load_entry / snap_load_slot: k_env_load's checks and copy as functions, for k_env_load_det (k_env_load keeps its own
// text: env_snap.hip says why).
// The wave's checks of the pair (entry s, slot g) of a load, on values it has made uniform: the entry, or null where the
// pair is skipped -- an index out of range, a header that is not this library's, or a stream cursor outside the two
// resident blocks, which the next step would read out of bounds (as monsoon_state_load).
__device__ MSB_INL u32x4* snap_load_entry(const u32x4* entries, const int n_entries, const int s, const int g, const int n,
                                          const uint32_t version, uint32_t& episode) {
  if (!(s >= 0 && s < n_entries && g >= 0 && g < n)) return nullptr;
  u32x4* ent = (u32x4*)entries + (size_t)s * (SNAP_BYTES / 16);
  const u32x4 hd = ent[0];
  const uint32_t magic = __builtin_amdgcn_readfirstlane(hd.x), ver = __builtin_amdgcn_readfirstlane(hd.y),
                 sw = __builtin_amdgcn_readfirstlane(hd.z);
  episode = __builtin_amdgcn_readfirstlane(hd.w);
  const uint32_t rng = __builtin_amdgcn_readfirstlane(ent[2].x);
  const bool ok = magic == SNAP_MAGIC && ver == version && sw == (uint32_t)SW && (rng & 0xffffu) < (uint32_t)(2 * MT_N) && (rng >> 17) == 0;
  return ok ? ent : nullptr;
}

// Slot g becomes the entry.  Of the meta row the episode's fields are taken (result, fault, last_action, flags, steps,
// rng); the players' rows, the schedule index and the look-ahead statistics (p1, p2, match, decided, lookahead, la_fault)
// stay the destination's.
__device__ MSB_INL void snap_load_slot(const DevBuffers& b, const EnvDev& v, const int g, u32x4* ent, const uint32_t episode, const int lane) {
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

struct EnvSnapOps {
  int entry_bytes;
  hipError_t (*occupancy)(int* blocks_per_cu, int lds_bytes);   // of the copy kernels (the smaller of the two).  lds_bytes is 0 for them: the argument is there so that the host's resident_waves() takes this query like a KernelOps one
  // grid = workgroups of SNAP_WAVES wavefronts
  void (*save)(int grid, hipStream_t stream, DevBuffers b, EnvDev v, int n, void* entries, const int32_t* slots, int m, uint32_t version);
  void (*load)(int grid, hipStream_t stream, DevBuffers b, EnvDev v, int n, const void* entries, int n_entries, const int32_t* src,
               const int32_t* dst, int m, uint8_t* loaded, uint32_t version);
};
const EnvSnapOps* monsoon_env_snap_ops();

// The determinizing load (env_determinize.hip): k_env_load_det on the copy kernels' grid, then k_env_determinize, a
// wavefront per pair (grid m).
struct EnvDetOps {
  void (*load)(int grid, hipStream_t stream, DevBuffers b, EnvDev v, int n, const void* entries, int n_entries, const int32_t* src,
               const int32_t* dst, int m, const uint8_t* observers, uint8_t* loaded, uint32_t version);
  void (*determinize)(hipStream_t stream, DevBuffers b, const void* entries, const int32_t* src, const int32_t* dst, int m,
                      const uint32_t* seeds, const uint8_t* observers, int what, const uint8_t* loaded);
};
const EnvDetOps* monsoon_env_det_ops();

}  // namespace msbk
