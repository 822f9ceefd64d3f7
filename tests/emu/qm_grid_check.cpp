// tests/emu/qm_grid_check.cpp -- TEST-ONLY command-line face of rapmap_amd/csrc/qm_grid.h (tests/test_launch_grid.py): every argument is
// one question, "fn:a,b,..", and gets one line with the answer.  A program of its own, so that the test can ask under a chosen environment.
#include "../../rapmap_amd/csrc/qm_grid.h"
#include <cstdio>
#include <cstring>

int main(int argc, char** argv) {
  for (int i = 1; i < argc; ++i) {
    char fn[32]; long long a[4] = {0, 0, 0, 0};
    const char* colon = strchr(argv[i], ':');
    const size_t fl = colon ? (size_t)(colon - argv[i]) : strlen(argv[i]);
    if (fl >= sizeof(fn)) return 2;
    memcpy(fn, argv[i], fl); fn[fl] = 0;
    if (colon) sscanf(colon + 1, "%lld,%lld,%lld,%lld", &a[0], &a[1], &a[2], &a[3]);
    long long r;
    if (!strcmp(fn, "blocks")) r = qm::grid_blocks(a[0], (int)a[1], (int)a[2], (int)a[3]);
    else if (!strcmp(fn, "clamp")) r = qm::grid_clamp(a[0], (int)a[1], (int)a[2], (int)a[3]);
    else if (!strcmp(fn, "resident")) r = qm::resident_grid(a[0], (int)a[1]);
    else if (!strcmp(fn, "sweep")) r = qm::sweep_grid(a[0], (int)a[1], (int)a[2], (int)a[3]);
    else if (!strcmp(fn, "map")) r = qm::map_grid(a[0], (int)a[1], a[2] != 0);
    else if (!strcmp(fn, "lean")) r = qm::lean_iters(a[0], a[1] != 0);
    else if (!strcmp(fn, "pair")) r = qm::pair_iters(a[0]);
    else if (!strcmp(fn, "oversub")) r = qm::grid_oversub();
    else if (!strcmp(fn, "oversub_ph")) r = qm::grid_oversub_ph();
    else return 2;
    printf("%lld\n", r);
  }
  return 0;
}
