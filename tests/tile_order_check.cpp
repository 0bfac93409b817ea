// Stand-alone host check of vl-bert_amd/csrc/tile_order.h (built and run by tests/test_tile_order_cpu.py with the address and
// undefined-behaviour sanitizers): the work-item -> tile map is a bijection onto the tile grid for any tile count and group height,
// every XCD owns one contiguous run of the list, and the host rule for the group height gives the documented values.
#include <stdio.h>

#include <vector>

#include "../vl-bert_amd/csrc/tile_order.h"

static int g_fail = 0;
#define CHECK(cond, ...)                 \
  do {                                   \
    if (!(cond)) {                       \
      if (++g_fail <= 20) {              \
        printf("FAIL %s: ", #cond);      \
        printf(__VA_ARGS__);             \
        printf("\n");                    \
      }                                  \
    }                                    \
  } while (0)

static void check_grid(int ntm, int ntn) {
  const int nt = ntm * ntn;
  // every XCD's work items w = x, x + 8, ... take consecutive ascending positions, and the eight runs partition [0, nt)
  std::vector<int> pos_seen(nt, 0);
  int run_begin[8], run_end[8];      // [begin, end) of XCD x's positions
  for (int x = 0; x < 8; ++x) {
    run_begin[x] = run_end[x] = -1;
    for (int w = x; w < nt; w += 8) {
      const int t = vlb_xcd_order(w, nt);
      CHECK(t >= 0 && t < nt, "%dx%d: w=%d -> position %d", ntm, ntn, w, t);
      if (t < 0 || t >= nt) continue;
      ++pos_seen[t];
      if (run_begin[x] < 0) run_begin[x] = t;
      else CHECK(t == run_end[x], "%dx%d: XCD %d: w=%d -> %d, expected %d", ntm, ntn, x, w, t, run_end[x]);
      run_end[x] = t + 1;
    }
  }
  for (int t = 0; t < nt; ++t) CHECK(pos_seen[t] == 1, "%dx%d: position %d taken %d times", ntm, ntn, t, pos_seen[t]);
  int next = 0;      // the runs follow each other in XCD order (an XCD without items has an empty run)
  for (int x = 0; x < 8; ++x) {
    if (run_begin[x] < 0) continue;
    CHECK(run_begin[x] == next, "%dx%d: XCD %d starts at %d, expected %d", ntm, ntn, x, run_begin[x], next);
    next = run_end[x];
  }
  CHECK(next == nt, "%dx%d: runs end at %d", ntm, ntn, next);

  for (int gi = 1; gi <= 9; ++gi) {
    const int group = gi <= 8 ? gi : ntm + 3;
    std::vector<int> hit(nt, 0);
    for (int w = 0; w < nt; ++w) {
      int tm = -1, tn = -1;
      vlb_tile_of(vlb_xcd_order(w, nt), ntm, ntn, group, tm, tn);
      const bool inside = tm >= 0 && tm < ntm && tn >= 0 && tn < ntn;
      CHECK(inside, "%dx%d group %d: w=%d -> tile (%d, %d)", ntm, ntn, group, w, tm, tn);
      if (inside) ++hit[tm * ntn + tn];
    }
    for (int i = 0; i < nt; ++i) CHECK(hit[i] == 1, "%dx%d group %d: tile (%d, %d) visited %d times", ntm, ntn, group, i / ntn, i % ntn, hit[i]);
  }

  const int g = vlb_square_tile_group(ntm, ntn);
  CHECK(g >= 1 && g <= ntm, "%dx%d: vlb_square_tile_group = %d", ntm, ntn, g);
}

int main() {
  for (int ntm = 1; ntm <= 13; ++ntm)
    for (int ntn = 1; ntn <= 13; ++ntn) check_grid(ntm, ntn);
  const int extra[][2] = {{26, 6}, {239, 6}, {6, 24}, {101, 12}, {51, 3}};
  for (const auto& e : extra) check_grid(e[0], e[1]);
  const int rule[][3] = {{26, 6, 1}, {239, 6, 1}, {6, 24, 4}, {24, 24, 8}, {1, 40, 1}, {7, 16, 4}};      // (7, 16): sqrt(14) = 3.74 rounds UP
  for (const auto& r : rule) {
    const int g = vlb_square_tile_group(r[0], r[1]);
    CHECK(g == r[2], "vlb_square_tile_group(%d, %d) = %d, expected %d", r[0], r[1], g, r[2]);
  }
  if (g_fail) {
    printf("%d checks failed\n", g_fail);
    return 1;
  }
  printf("tile order ok\n");
  return 0;
}
