// Host run of monsoon_amd/csrc/deck_schedule.h (the text k_draw_schedule compiles) for tests/test_deck_schedule_cpu.py:
// reads cases from the file named on the command line, prints every game's pair.  Built with the address and UB
// sanitizers into a stand-alone program.
//
// input (whitespace separated):  n_cases, then per case
//     seed generation tag phase n_preserve ratio(hex float) pool_n0 pool_n1 n_games
//     archetype[24]  pool0[pool_n0]  pool1[pool_n1]  game_seeds[n_games]
// output: per case a line "case <i> over <games past the window> maxpos <most outputs one game used>", then one line of
// 48 hex digits per game.
#include <stdio.h>
#include <stdlib.h>

#include <vector>

#include "deck_schedule.h"

using namespace msb;

int main(int argc, char** argv) {
  if (argc != 2) return 2;
  FILE* f = fopen(argv[1], "r");
  if (!f) return 2;
  uint32_t mt_init[MT_N];
  mt_seed(mt_init, DS_INIT_SEED);
  int n_cases = 0;
  if (fscanf(f, "%d", &n_cases) != 1) return 2;
  for (int c = 0; c < n_cases; c++) {
    uint32_t seed, generation, tag;
    int phase, n_preserve, n_games;
    int32_t pool_n[2];
    char ratio_text[64];
    if (fscanf(f, "%u %u %u %d %d %63s %d %d %d", &seed, &generation, &tag, &phase, &n_preserve, ratio_text, &pool_n[0], &pool_n[1], &n_games) != 9) return 2;
    const double ratio = strtod(ratio_text, nullptr);
    if (pool_n[0] < 12 || pool_n[0] > DS_POOL_MAX || pool_n[1] < 12 || pool_n[1] > DS_POOL_MAX || n_preserve < 0 || n_preserve > 12) return 2;
    std::vector<uint8_t> arch(24);
    std::vector<uint8_t> pool[2] = {std::vector<uint8_t>(pool_n[0]), std::vector<uint8_t>(pool_n[1])};   // exact sizes: a read past a pool is caught
    unsigned v;
    for (auto& a : arch) {
      if (fscanf(f, "%u", &v) != 1) return 2;
      a = (uint8_t)v;
    }
    for (auto& p : pool)
      for (auto& a : p) {
        if (fscanf(f, "%u", &v) != 1) return 2;
        a = (uint8_t)v;
      }
    std::vector<uint32_t> seeds(n_games);
    for (auto& s : seeds)
      if (fscanf(f, "%u", &s) != 1) return 2;
    std::vector<uint8_t> out((size_t)n_games * 24);
    int over = 0, maxpos = 0;
    for (int g = 0; g < n_games; g++) {
      uint32_t mt[MT_N];
      for (int i = 0; i < MT_N; i++) mt[i] = mt_init[i];
      const uint32_t key[4] = {seed, generation, seeds[g], tag};
      ds_key_mix(mt, key);
      mt_twist(mt);
      for (int i = 0; i < MT_N; i++) mt[i] = mt_temper(mt[i]);
      // the walk's scratch copies; the pools side by side as the kernel lays them out, the second one exact-sized at the end
      std::vector<uint8_t> a = arch, p(DS_POOL_MAX + pool_n[1]);
      for (int i = 0; i < pool_n[0]; i++) p[i] = pool[0][i];
      for (int i = 0; i < pool_n[1]; i++) p[DS_POOL_MAX + i] = pool[1][i];
      DsStream s{mt, 0, 0};
      ds_walk(s, phase, n_preserve, ratio, a.data(), p.data(), pool_n, &out[(size_t)g * 24]);
      over += s.over != 0;
      if (s.pos > maxpos) maxpos = s.pos;
    }
    printf("case %d over %d maxpos %d\n", c, over, maxpos);
    for (int g = 0; g < n_games; g++) {
      for (int i = 0; i < 24; i++) printf("%02x", out[(size_t)g * 24 + i]);
      printf("\n");
    }
  }
  fclose(f);
  return 0;
}
