// l1_counted_layout -- prints the row binning's scratch layout with the counted level 1's row tables (csrc/ggd_binning_layout.h),
// for tests/test_level1_counted_host.py.  Includes nothing else of the library.  Reads lines `P capacity W H` from stdin and
// prints one line of `name=value` pairs (byte offsets) per input line; `touch` walks the first and last word of both tables in a
// buffer of total_counted bytes, so that the sanitizers see an offset that leaves it.
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include "ggd_binning_layout.h"

int main() {
  long long P, cap;
  int W, H;
  while (scanf("%lld %lld %d %d", &P, &cap, &W, &H) == 4) {
    const ggd_rowbin_tmp r = ggd_rowbin_layout((int)P, (uint32_t)cap, W, H);
    int touch = 0;
    if (r.total_counted <= ((size_t)1 << 28)) {
      unsigned char* buf = static_cast<unsigned char*>(malloc(r.total_counted > 0 ? r.total_counted : 1));
      if (!buf) return 1;
      const size_t chunks = (size_t)rb_blocks1((int)P);
      uint32_t one = 1u;
      memcpy(buf + r.bucket_rows, &one, 4);
      memcpy(buf + r.bucket_rows + ((size_t)GGD_MSD_BINS * 64 - 1) * 4, &one, 4);
      if (chunks > 0) {
        memcpy(buf + r.boundary_rows, &one, 4);
        memcpy(buf + r.boundary_rows + (chunks * 64 - 1) * 4, &one, 4);
      }
      touch = 1;
      free(buf);
    }
    printf("rb_packed=%zu rb_counts1=%zu rb_tab=%zu rb_ent=%zu rb_counts2=%zu rb_total=%zu rb_bucket_rows=%zu rb_boundary_rows=%zu "
           "rb_total_counted=%zu msd_bins=%d chunks=%d touch=%d\n",
           r.packed, r.counts1, r.tab, r.ent, r.counts2, r.total, r.bucket_rows, r.boundary_rows, r.total_counted, GGD_MSD_BINS,
           rb_blocks1((int)P), touch);
  }
  return 0;
}
