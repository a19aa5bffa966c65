// Prints the planner's decision -- kernel kind, T, the LD handed to the kernel, G, LDS bytes and
// 64-chain workspace bytes per shard -- over a grid of (d, C, n) that reaches every kind, as JSON.
// Host only: runs without a GPU.  Its output is tests/golden/sweep_launch.json, which
// tests/test_host_sweep_launch.py holds stk_sweep_launch_info to.  The file was recorded from the
// scattered routing code that stk_sweep_plan replaced and is regenerated ONLY by a change that
// means to alter routing; any other change must reproduce it byte for byte:
//   hipcc -O1 --offload-arch=gfx950 -std=c++17 tools/sweep_launch_dump.hip -o tools/_bin/sweep_launch_dump
//   tools/_bin/sweep_launch_dump | cmp - tests/golden/sweep_launch.json
// (No -DSTK_SWEEP_TU: the three kernel files are one translation unit here, every family instantiated where used.)
#include "../stark_amd/csrc/sweep.hip"
#include "../stark_amd/csrc/sweep16.hip"
#include "../stark_amd/csrc/sweep16w.hip"
#include <stdio.h>

int main() {
  const int ds[] = {1, 4, 5, 20, 33, 50, 100, 104, 106, 120, 128, 129, 300, 700, 1024};
  const int Cs[] = {1, 2, 4, 8, 16, 64};
  const int64_t ns[] = {1, 77, 600, 1500, 2000000, 12500000, (int64_t)1 << 31};
  printf("{\"columns\": [\"n\", \"d\", \"C\", \"kind\", \"T\", \"LD\", \"G\", \"lds_bytes\", \"ws_bytes_per_shard\"],\n \"rows\": [\n");
  bool first = true;
  for (const int d : ds)
    for (const int C : Cs)
      for (const int64_t n : ns) {
        printf("%s", first ? "" : ",\n");
        first = false;
        const SweepLaunch p = stk_sweep_plan(n, d, C, 0);
        if (p.kind == SWEEP_NONE) {   // refused: nothing else is recorded
          printf("  [%lld, %d, %d, 0]", (long long)n, d, C);
          continue;
        }
        printf("  [%lld, %d, %d, %d, %d, %d, %d, %zu, %zu]", (long long)n, d, C, (int)p.kind, p.T, stk_sweep_args_ld(p), p.G,
               p.lds, p.ws_bytes);
      }
  printf("\n ]}\n");
  return 0;
}
