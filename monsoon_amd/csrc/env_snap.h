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

struct EnvSnapOps {
  int entry_bytes;
  hipError_t (*occupancy)(int* blocks_per_cu, int lds_bytes);   // of the copy kernels (the smaller of the two).  lds_bytes is 0 for them: the argument is there so that the host's resident_waves() takes this query like a KernelOps one
  // grid = workgroups of SNAP_WAVES wavefronts
  void (*save)(int grid, hipStream_t stream, DevBuffers b, EnvDev v, int n, void* entries, const int32_t* slots, int m, uint32_t version);
  void (*load)(int grid, hipStream_t stream, DevBuffers b, EnvDev v, int n, const void* entries, int n_entries, const int32_t* src,
               const int32_t* dst, int m, uint8_t* loaded, uint32_t version);
};
const EnvSnapOps* monsoon_env_snap_ops();

}  // namespace msbk
