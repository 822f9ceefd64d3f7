// tests/emu/qm_runs_check.cpp -- TEST-ONLY command-line face of the run schedule in rapmap_amd/csrc/qm_grid.h (tests/test_wave_runs.py):
// every argument is one question, "fn:a,b,..", and gets one line with the answer.  A program of its own, so that the test can ask under
// a chosen environment.
#include "../../rapmap_amd/csrc/qm_grid.h"
#include <cstdio>
#include <cstring>
#include <vector>

// every wave gw of nw walks its trips with run_next from run_trip(0, ..), as the wave drivers do: trips visited, trips not visited exactly
// once, steps that do not ascend or leave a run before run_ends says so, steps that differ from run_trip(t, ..), most and fewest trips of a wave
static void walk(long long trips, int nw, int rs) {
  std::vector<unsigned char> seen((size_t)trips + 1, 0);
  long long visited = 0, order = 0, differ = 0, most = 0, fewest = -1;
  for (int gw = 0; gw < nw; ++gw) {
    const long long t0 = qm::run_trip(0, gw, nw, rs);
    long long t = 0, prev = -1;
    for (int it = t0 < trips ? (int)t0 : (int)trips; it < trips; it = qm::run_next(it, (int)trips, nw, rs), ++t) {
      if (seen[(size_t)it] < 2) ++seen[(size_t)it];
      ++visited;
      if (it != qm::run_trip(t, gw, nw, rs)) ++differ;
      if (it <= prev) ++order;
      if (prev >= 0 && !qm::run_ends((int)prev, (int)trips, rs) && it != prev + 1) ++order;      // inside a run: the neighbour
      if (prev >= 0 && qm::run_ends((int)prev, (int)trips, rs) && (it & ((1 << rs) - 1)) != 0) ++order;   // behind a run: the start of another
      prev = it;
    }
    if (qm::run_trip(t, gw, nw, rs) < trips) ++differ;        // run_trip says the wave has more to do
    if (t > most) most = t;
    if (fewest < 0 || t < fewest) fewest = t;
  }
  long long bad = 0;
  for (long long i = 0; i < trips; ++i) if (seen[(size_t)i] != 1) ++bad;
  printf("%lld %lld %lld %lld %lld %lld\n", visited, bad, order, differ, most, fewest);
}

int main(int argc, char** argv) {
  for (int i = 1; i < argc; ++i) {
    char fn[32]; long long a[4] = {0, 0, 0, 0};
    const char* colon = strchr(argv[i], ':');
    const size_t fl = colon ? (size_t)(colon - argv[i]) : strlen(argv[i]);
    if (fl >= sizeof(fn)) return 2;
    memcpy(fn, argv[i], fl); fn[fl] = 0;
    if (colon) sscanf(colon + 1, "%lld,%lld,%lld,%lld", &a[0], &a[1], &a[2], &a[3]);
    long long r;
    if (!strcmp(fn, "walk")) { walk(a[0], (int)a[1], (int)a[2]); continue; }
    if (!strcmp(fn, "wave")) {                                  // the trips of wave a[3] of a[1] over a[0] trips at run shift a[2]
      const long long t0 = qm::run_trip(0, (int)a[3], (int)a[1], (int)a[2]);
      for (int it = t0 < a[0] ? (int)t0 : (int)a[0]; it < a[0]; it = qm::run_next(it, (int)a[0], (int)a[1], (int)a[2])) printf("%d ", it);
      printf("\n");
      continue;
    }
    if (!strcmp(fn, "shift")) r = qm::run_shift(a[0], a[1], (int)a[2]);
    else if (!strcmp(fn, "count")) r = qm::run_count(a[0], (int)a[1]);
    else if (!strcmp(fn, "trip")) r = qm::run_trip(a[0], (int)a[1], (int)a[2], (int)a[3]);
    else if (!strcmp(fn, "ahead")) r = qm::run_ahead((int)a[0], (int)a[1], (int)a[2], 3, (int)a[3]);   // (run shift 3)
    else if (!strcmp(fn, "wave_blocks")) r = qm::wave_blocks((int)a[0], (int)a[1]);
    else if (!strcmp(fn, "wave_run")) r = qm::wave_run();
    else if (!strcmp(fn, "grid")) { const qm::WaveGrid g = qm::wave_grid(a[0], (int)a[1], (int)a[2], (int)a[3]); printf("%d %d\n", g.blocks * QM_WG_WAVES, g.rs); continue; }   // waves, run shift
    else return 2;
    printf("%lld\n", r);
  }
  return 0;
}
