// spec_trace -- drives the forward's speculation policy (ggd_spec.h) on a CPU, as the host code of ggd_capi.hip does for one frame
// after another: plan, three-pass decision, then the frame's report.  Reads one command per line from stdin:
//   frame FOLDED FLAT MSD_OK KMIN KMAX FLAGS [ABANDONED]   one speculative frame and the report its front end delivers
//   opts FOLD_OPT MSD_OPT MSD_SUPPORTED                     GGD_OPT_FOLD, GGD_OPT_MSD_SORT, ggd_sort32_msd_supported (default 1 1 1)
//   reset                                                   what setting either option does
// and prints one line per frame: msd lo shift three_passes render_again reruns msd_frames flat_streak pause
#include <stdio.h>
#include <string.h>

#include "ggd_spec.h"

int main() {
  ggd_spec spec;
  int fold_opt = 1, msd_opt = 1, supported = 1;
  char line[256];
  while (fgets(line, sizeof line, stdin)) {
    unsigned folded, flat, ok, kmin, kmax, flags, abandoned = 0;
    if (strncmp(line, "reset", 5) == 0) {
      spec.reset();
    } else if (sscanf(line, "opts %d %d %d", &fold_opt, &msd_opt, &supported) == 3) {
    } else if (sscanf(line, "frame %u %u %u %u %u %u %u", &folded, &flat, &ok, &kmin, &kmax, &flags, &abandoned) >= 6) {
      const ggd_spec_plan plan = spec.plan(fold_opt, msd_opt, supported != 0);
      const bool three = spec.three_passes(plan, folded != 0, true, fold_opt);
      ggd_spec_report r;
      r.folded = folded != 0; r.flat = flat != 0; r.msd_ok = ok != 0; r.kmin = kmin; r.kmax = kmax; r.msd_flags = flags;
      const bool again = spec.observe(plan, three, r, abandoned != 0);
      printf("%d %u %d %d %d %llu %llu %d %d\n", plan.msd ? 1 : 0, plan.lo, plan.shift, three ? 1 : 0, again ? 1 : 0, spec.reruns,
             spec.msd_frames, spec.flat_streak, spec.msd_ban);
    } else if (line[0] != '\n' && line[0] != '#') {
      fprintf(stderr, "spec_trace: bad line: %s", line);
      return 2;
    }
  }
  return 0;
}
