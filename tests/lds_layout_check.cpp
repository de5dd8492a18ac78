// Host check of the candidate records' LDS map (monsoon_amd/csrc/lds_layout.h), compiled once per record build (no flag,
// -DMSB_EXT=1, -DMSB_EXT=2) with the address and UB sanitizers into a stand-alone program (tests/test_lds_layout_cpu.py).
// The column accessors (state.h LaneColMem / Col0ColMem / SubColColMem) and the whole-wave moves of a record onto columns
// (kernels.h PlayLds<U>::gran) compute every address with RecordMap's functions; the interleaved ones spell the formula of
// RecordMap<.., false> in place.  This program calls the map's functions on a simulated LDS byte array, for U in {4, 8, 16, 32, 64}, both maps, and the record size of this build:
//   (a) bounds      the whole-wave granule map writes every byte of [BASE, BASE + U * STATE_BYTES) exactly once and nothing
//                   else (the array ends where the area ends: the address sanitizer sees a byte past it), columns of the
//                   column map are disjoint byte ranges, and the area is no larger than the kernels' PRIV_BYTES;
//   (b) round trip  a record written into every column by the whole-wave map (lane l carries granules l, l + 64, ...) is
//                   read back byte for byte through byte_at(col_off(c), ..) -- the per-lane and the sub-lane accessor form,
//                   which differ in where c comes from -- and byte_at(0, ..), the column-0 form, at every aligned offset
//                   and width 1, 2, 4, 8, 16, and through gbyte_at at every (granule, byte, width);
//   (c) banks       by the bank rules of the LDS (32 banks of 4 bytes for accesses up to 4 bytes and for every store, 64 for
//                   8- and 16-byte reads): lanes 0 .. min(U, 8) - 1 accessing one offset of their own records hit disjoint
//                   banks at every width on the map the build selects (PLAY_LDS_COLUMNS); the stride rule the selection
//                   rests on (stride_conflict_free) says exactly what the enumeration finds for the column map of this
//                   record size; and the whole-wave moves have the conflict degree listed in expected_move_degree() --
//                   1 on columns, the known collisions of the interleave spelled out.
// Prints one "ok ..." line with what it found; any mismatch prints the place and exits 1.
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <vector>

#include "state.h"
#include "mt19937.h"

using namespace msb;

static int g_fail = 0;
#define CHECK(cond, ...)             \
  do {                               \
    if (!(cond)) {                   \
      if (g_fail < 20) {             \
        printf("FAIL %s: ", #cond);  \
        printf(__VA_ARGS__);         \
        printf("\n");                \
      }                              \
      g_fail++;                      \
    }                                \
  } while (0)

constexpr int BASE = LDS_RECORDS;   // kernels.h LDS_ORIGIN
constexpr int SGR = STATE_BYTES / 16;
constexpr int WIDTHS[5] = {1, 2, 4, 8, 16};
static long g_reads = 0, g_bank_cases = 0;

static uint8_t rec_byte(int c, int o) { return (uint8_t)(((unsigned)c * 131u + (unsigned)o * 7u + ((unsigned)o >> 8) * 29u + 3u) & 0xffu); }

// kernels.h PRIV_BYTES: the candidate area doubles as the twist buffer of a stream block
static constexpr int priv_bytes(int u) { return SGR * u * 16 > MT_N * 4 ? SGR * u * 16 : ((MT_N * 4 + 15) & ~15); }

template <class M>
static void read_back(const std::vector<uint8_t>& lds, const char* what, int U, int coff, int c) {
  for (int wi = 0; wi < 5; wi++) {
    const int w = WIDTHS[wi];
    for (int o = 0; o + w <= STATE_BYTES; o += w) {   // naturally aligned, as every field of the record is
      const int a = M::byte_at(coff, o);
      for (int i = 0; i < w; i++) {
        CHECK(a + i >= BASE && a + i < BASE + M::AREA, "%s U=%d cols=%d column %d offset %d width %d: address %d outside the area", what, U, (int)M::columns, c, o, w, a + i);
        if (a + i >= BASE && a + i < BASE + M::AREA)
          CHECK(lds[a + i] == rec_byte(c, o + i), "%s U=%d cols=%d column %d offset %d width %d byte %d", what, U, (int)M::columns, c, o, w, i);
      }
      g_reads++;
    }
    for (int g = 0; g < SGR; g++)
      for (int k = 0; k + w <= 16; k += w) {
        const int a = M::gbyte_at(coff, g, k);
        CHECK(a == M::byte_at(coff, g * 16 + k), "%s U=%d cols=%d: gbyte_at(%d, %d) and byte_at disagree", what, U, (int)M::columns, g, k);
        for (int i = 0; i < w; i++)
          if (a + i >= BASE && a + i < BASE + M::AREA)
            CHECK(lds[a + i] == rec_byte(c, g * 16 + k + i), "%s U=%d cols=%d column %d granule %d byte %d width %d", what, U, (int)M::columns, c, g, k, w);
          else
            CHECK(false, "%s U=%d cols=%d column %d granule %d byte %d: address %d outside the area", what, U, (int)M::columns, c, g, k, a + i);
        g_reads++;
      }
  }
}

// worst number of distinct addresses on one bank among `n` lanes accessing `w` bytes at addr[l] (identical addresses broadcast)
static int conflict_degree(const int* addr, int n, int w, int banks) {
  int worst = 1;
  for (int bk = 0; bk < banks; bk++) {
    int distinct = 0;
    int seen[64];
    for (int l = 0; l < n; l++)
      for (int d = 0; d < (w + 3) / 4; d++) {
        const int dw = addr[l] / 4 + d;
        if (dw % banks != bk) continue;
        bool dup = false;
        for (int s = 0; s < distinct; s++) dup |= seen[s] == dw;
        if (!dup) seen[distinct++] = dw;
      }
    if (distinct > worst) worst = distinct;
  }
  return worst;
}

// lanes 0 .. n-1 at one offset of their own records: the worst conflict degree over every aligned offset and width (reads
// and stores: stores use 32 banks at every width)
template <class M>
static int lane_access_degree(int n, int* worst_w = nullptr, int* worst_o = nullptr) {
  int worst = 1;
  for (int wi = 0; wi < 5; wi++) {
    const int w = WIDTHS[wi];
    for (int o = 0; o + w <= STATE_BYTES; o += w) {
      int addr[8];
      for (int l = 0; l < n; l++) addr[l] = M::byte_at(l * M::STRIDE, o);
      const int rd = conflict_degree(addr, n, w, w >= 8 ? 64 : 32), st = conflict_degree(addr, n, w, 32);
      const int d = rd > st ? rd : st;
      if (d > worst) {
        worst = d;
        if (worst_w) *worst_w = w;
        if (worst_o) *worst_o = o;
      }
      g_bank_cases++;
    }
  }
  return worst;
}

// A whole-wave move of column c (16 bytes per lane, lane l granule l): stores in groups of 8 consecutive lanes on 32 banks,
// reads in the four 16-lane groups of ds_read_b128 on 64 banks.
static const int READ_GROUPS[4][16] = {{0, 1, 2, 3, 12, 13, 14, 15, 20, 21, 22, 23, 24, 25, 26, 27},
                                       {4, 5, 6, 7, 8, 9, 10, 11, 16, 17, 18, 19, 28, 29, 30, 31},
                                       {32, 33, 34, 35, 44, 45, 46, 47, 52, 53, 54, 55, 56, 57, 58, 59},
                                       {36, 37, 38, 39, 40, 41, 42, 43, 48, 49, 50, 51, 60, 61, 62, 63}};
template <class M>
static void move_degree(int U, int& store_deg, int& read_deg) {
  store_deg = read_deg = 1;
  const int lanes = SGR < 64 ? SGR : 64;   // (the first 64 granules; the later ones repeat the pattern)
  for (int c = 0; c < U; c++) {
    for (int g0 = 0; g0 < lanes; g0 += 8) {
      int addr[8], n = 0;
      for (int l = g0; l < g0 + 8 && l < lanes; l++) addr[n++] = M::granule(c, l);
      const int d = conflict_degree(addr, n, 16, 32);
      if (d > store_deg) store_deg = d;
    }
    for (int gi = 0; gi < 4; gi++) {
      int addr[16], n = 0;
      for (int i = 0; i < 16; i++)
        if (READ_GROUPS[gi][i] < lanes) addr[n++] = M::granule(c, READ_GROUPS[gi][i]);
      if (!n) continue;
      const int d = conflict_degree(addr, n, 16, 64);
      if (d > read_deg) read_deg = d;
    }
  }
}
// What the moves are known to cost.  Columns: lane l touches bytes [16 l, 16 l + 16) of the column, no conflict.  Interleave:
// the lane stride is U * 16 bytes = 4 U banks, so a store group's 8 lanes fall on 32 / (4 U) bank sets (U = 4: two, 4-way;
// U >= 8: one, 8-way) and a read group's 16 lanes on 64 / (4 U) (U = 4: four, 4-way; U = 8: two, 8-way; U >= 16: one, 16-way).
static void expected_move_degree(bool columns, int U, int& store_deg, int& read_deg) {
  if (columns) {
    store_deg = read_deg = 1;
    return;
  }
  store_deg = U == 4 ? 4 : 8;
  read_deg = U == 4 ? 4 : U == 8 ? 8 : 16;
}

template <int U, bool COLS>
static void check_map() {
  typedef lds_layout::RecordMap<U, BASE, STATE_BYTES, COLS> M;
  // (a) bounds
  CHECK(M::AREA == U * STATE_BYTES && M::AREA <= priv_bytes(U), "U=%d: area %d, PRIV_BYTES %d", U, M::AREA, priv_bytes(U));
  CHECK(priv_bytes(U) == (U * STATE_BYTES > 2496 ? U * STATE_BYTES : 2496), "U=%d: PRIV_BYTES grew to %d", U, priv_bytes(U));
  if (COLS)
    for (int c = 0; c < U; c++) {
      CHECK(M::byte(c, 0) == BASE + c * STATE_BYTES && M::byte(c, STATE_BYTES - 1) == BASE + c * STATE_BYTES + STATE_BYTES - 1,
            "U=%d column %d is not [BASE + c * STATE_BYTES, + STATE_BYTES)", U, c);
      if (c) CHECK(M::byte(c, 0) == M::byte(c - 1, STATE_BYTES - 1) + 1, "U=%d: columns %d and %d overlap or leave a gap", U, c - 1, c);
    }
  std::vector<uint8_t> lds((size_t)BASE + M::AREA, 0);   // ends with the area: a byte past it is the sanitizer's
  std::vector<uint8_t> hits((size_t)BASE + M::AREA, 0);
  // the whole-wave move of a record into every column: lane l carries granules l, l + 64, ... (kernels.h MSB_EACH_GRANULE)
  for (int c = 0; c < U; c++)
    for (int lane = 0; lane < 64; lane++)
      for (int j = 0; lane + 64 * j < SGR; j++) {
        const int gr = lane + 64 * j, a = M::granule(c, gr);
        CHECK(a >= BASE && a + 16 <= BASE + M::AREA && a % 16 == 0, "U=%d cols=%d: granule %d of column %d at %d", U, (int)COLS, gr, c, a);
        if (!(a >= BASE && a + 16 <= BASE + M::AREA)) continue;
        for (int i = 0; i < 16; i++) {
          lds[a + i] = rec_byte(c, gr * 16 + i);
          hits[a + i]++;
        }
      }
  long once = 0;
  for (int a = BASE; a < BASE + M::AREA; a++) once += hits[a] == 1;
  CHECK(once == M::AREA, "U=%d cols=%d: %ld of %d bytes of the area written exactly once", U, (int)COLS, once, M::AREA);
  // (b) round trip through the three accessor forms
  // (the three forms differ only in where the column offset comes from: col_off(work-item id) in LaneColMem, col_off(the
  // caller's column) in SubColColMem, 0 in Col0ColMem; the structs themselves are device code, tests/test_lds_layout_gpu.py)
  for (int c = 0; c < U; c++) read_back<M>(lds, "column", U, M::col_off(c), c);
  read_back<M>(lds, "col0", U, 0, 0);
  // (c) the moves
  int sd, rd, esd, erd;
  move_degree<M>(U, sd, rd);
  expected_move_degree(COLS, U, esd, erd);
  CHECK(sd == esd && rd == erd, "U=%d cols=%d: a record's move is %d-way on stores, %d-way on reads; listed %d, %d", U, (int)COLS, sd, rd, esd, erd);
}

template <int U>
static void check_u(int& sel_move_store, int& sel_move_read) {
  check_map<U, false>();
  check_map<U, true>();
  typedef lds_layout::RecordMap<U, BASE, STATE_BYTES, PLAY_LDS_COLUMNS> Sel;   // what PlayLds<U> uses in this build
  typedef lds_layout::RecordMap<U, BASE, STATE_BYTES, true> Col;
  const int n = U < 8 ? U : 8;
  int w = 0, o = 0;
  const int d = lane_access_degree<Sel>(n, &w, &o);
  CHECK(d == 1, "U=%d: lanes 0..%d collide %d-way at offset %d, width %d on the selected map", U, n - 1, d, o, w);
  // the rule the selection rests on, against the enumeration (8 lanes: the rule is stated for 8)
  if (U >= 8) {
    const int dc = lane_access_degree<Col>(8, &w, &o);
    CHECK((dc == 1) == lds_layout::stride_conflict_free(STATE_BYTES), "stride rule says %d for %d bytes, the enumeration finds %d-way (offset %d, width %d)",
          (int)lds_layout::stride_conflict_free(STATE_BYTES), STATE_BYTES, dc, o, w);
  }
  int sd, rd;
  move_degree<Sel>(U, sd, rd);
  if (sd > sel_move_store) sel_move_store = sd;
  if (rd > sel_move_read) sel_move_read = rd;
}

int main() {
  int ms = 1, mr = 1;
  check_u<4>(ms, mr);
  check_u<8>(ms, mr);
  check_u<16>(ms, mr);
  check_u<32>(ms, mr);
  check_u<64>(ms, mr);
  // the column map of THIS record size at 8 lanes, whether selected or not: what the build's choice is made of
  int w = 0, o = 0;
  const int col8 = lane_access_degree<lds_layout::RecordMap<8, BASE, STATE_BYTES, true>>(8, &w, &o);
  if (g_fail) {
    printf("%d failures\n", g_fail);
    return 1;
  }
  printf("ok state_bytes %d columns %d stride_mod128 %d column_lane_degree %d move_store_degree %d move_read_degree %d area8 %d origin %d reads %ld bank_cases %ld\n",
         STATE_BYTES, (int)PLAY_LDS_COLUMNS, STATE_BYTES & 127, col8, ms, mr, priv_bytes(8), BASE, g_reads, g_bank_cases);
  return 0;
}
