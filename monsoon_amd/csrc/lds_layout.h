// lds_layout.h -- where byte o of candidate record c sits in the LDS area of a wavefront-per-game kernel.  Plain constexpr
// C++ and nothing else.  The column accessors (state.h LaneColMem / Col0ColMem / SubColColMem), the whole-wave moves of a
// record onto columns (kernels.h PlayLds<U>::gran) and the host check (tests/lds_layout_check.cpp) all call this one map,
// so the copy that fills a column and the accessor that reads it cannot disagree.  The interleaved accessors (LaneMem /
// Col0Mem / SubColMem) and the interleaved branch of gran() are older than this header and keep the same formula spelled
// in place: written through the map they compiled to other code in kernels this layout does not concern (the lane-per-game
// kernels, every kernel of the extended record), which stay instruction-identical to their parents this way.  For that
// map the host check pins the formula as written here, the device's copy of it is covered by the GPU tests alone.
//
// Two maps of U records of BYTES bytes (whole 16-byte granules) into [BASE, BASE + U * BYTES):
//   COLUMNS     record c is the contiguous column [BASE + c * BYTES, + BYTES): byte o of it at BASE + c * BYTES + o.  One
//               add for an offset the compiler does not know, and the constant part of it goes into the instruction's
//               offset field.  A whole-wave move of a record -- lane l carries granule l -- touches 64 consecutive
//               granules: no bank conflict.  Lanes 0..7 touching the same field of their own records are BYTES apart, which
//               is conflict-free at every access width iff BYTES = +-16 (mod 128) (stride_conflict_free below: 32 banks of
//               4 bytes for 4-byte accesses and wide stores, 64 for 8- and 16-byte reads).
//   interleaved granule g of record c at BASE + (g * U + c) * 16: byte o at BASE + (o >> 4) * (U * 16) + (o & 15) + c * 16.
//               Same-field accesses of neighbouring records hit neighbouring granules (conflict-free for any BYTES); an
//               offset the compiler does not know pays the shift, the mask and the scale, and a whole-wave move of a
//               record has a lane stride of U * 16 bytes (U = 8: 8 lanes per bank).
// A column is named either by its index c or by its offset col_off(c), the value an accessor may carry (SubColMem).
#pragma once

namespace msb {
namespace lds_layout {

constexpr int GRANULE = 16;
// (inlined before anything else is: to the compiler an accessor that calls the map is the accessor with the map written out)
#define MSB_LDS_MAP_FN __attribute__((always_inline)) static constexpr int

template <int U, int BASE, int BYTES, bool COLUMNS>
struct RecordMap {
  static_assert(BYTES % GRANULE == 0, "a record is whole granules");
  static constexpr bool columns = COLUMNS;
  static constexpr int AREA = U * BYTES;                             // both maps fill exactly [BASE, BASE + AREA)
  static constexpr int STRIDE = COLUMNS ? BYTES : GRANULE;           // from a byte of record c to the same byte of record c + 1
  static constexpr int GRANULE_STEP = COLUMNS ? GRANULE : U * GRANULE;   // from granule g of a record to its granule g + 1
  MSB_LDS_MAP_FN col_off(int c) { return c * STRIDE; }
  // byte o of the record whose column offset is `coff`
  MSB_LDS_MAP_FN byte_at(int coff, int o) {
    return COLUMNS ? BASE + coff + o : BASE + (o >> 4) * (U * GRANULE) + (o & 15) + coff;
  }
  // byte k of granule g of it: one scale for a granule the compiler does not know, the rest is constant
  MSB_LDS_MAP_FN gbyte_at(int coff, int g, int k) {
    return COLUMNS ? BASE + coff + g * GRANULE + k : BASE + g * (U * GRANULE) + k + coff;
  }
  MSB_LDS_MAP_FN byte(int c, int o) { return byte_at(col_off(c), o); }
  MSB_LDS_MAP_FN gbyte(int c, int g, int k) { return gbyte_at(col_off(c), g, k); }
  MSB_LDS_MAP_FN granule(int c, int g) { return gbyte(c, g, 0); }   // what a whole-wave move reads and writes
};

#undef MSB_LDS_MAP_FN

// 8 lanes `stride` bytes apart touch disjoint banks at 1, 2, 4, 8 and 16 bytes per lane.
constexpr bool stride_conflict_free(int stride) { return (stride & 127) == 16 || (stride & 127) == 112; }

// LDS bank of byte address a: 32 banks of 4 bytes (4-byte and narrower accesses, every store) or 64 (8- and 16-byte reads).
constexpr int bank(int a, int banks) { return (a / 4) % banks; }

}  // namespace lds_layout
}  // namespace msb
