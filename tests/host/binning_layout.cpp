// binning_layout -- prints what csrc/ggd_binning_layout.h computes, for tests/test_binning_layout_host.py to compare with the
// formulas of the code the header was lifted from.  Includes nothing else of the library.  Reads lines `P capacity W H` from stdin
// and prints one line of `name=value` pairs per input line:
//   rb_*            byte offsets and total of ggd_rowbin_tmp
//   tmp_* clean_* fold_*   word offsets of ggd_sort_ctl's fields in its three forms (head fields relative to the block that holds
//                   them, status relative to the buffer that holds the status words), and reps
//   gshift_tiles gshift_chunks status_words fold_ctl_words fold_l1_offset sort_tmp_bytes sort32_tmp_bytes msd_table_bytes
#include <stdio.h>

#include "ggd_binning_layout.h"

static uint32_t tmp[1 << 15], clean[1 << 12], fold[1 << 15];   // large enough for every field's first word

static void print_ctl(const char* name, const ggd_sort_ctl& c, const uint32_t* head, const uint32_t* status_base) {
  printf("%s_ghist=%td %s_tickets=%td %s_n_valid=%td %s_flat=%td %s_status=%td %s_reps=%d ", name, c.ghist - head, name,
         c.tickets - head, name, c.n_valid - head, name, c.flat - head, name, c.status - status_base, name, c.reps);
}

int main() {
  long long P, cap;
  int W, H;
  while (scanf("%lld %lld %d %d", &P, &cap, &W, &H) == 4) {
    const ggd_rowbin_tmp r = ggd_rowbin_layout((int)P, (uint32_t)cap, W, H);
    printf("rb_packed=%zu rb_counts1=%zu rb_tab=%zu rb_ent=%zu rb_counts2=%zu rb_total=%zu ", r.packed, r.counts1, r.tab, r.ent,
           r.counts2, r.total);
    print_ctl("tmp", ggd_sort_ctl::in_tmp(tmp), tmp, tmp);
    print_ctl("clean", ggd_sort_ctl::in_clean(clean, tmp), clean, tmp);
    print_ctl("fold", ggd_sort_ctl::in_fold(fold), fold, fold);
    const ggd_sort_ctl s0 = ggd_sort_ctl::select(tmp, nullptr, nullptr), s1 = ggd_sort_ctl::select(tmp, clean, nullptr),
                       s2 = ggd_sort_ctl::select(tmp, clean, fold);
    const long long tiles = (long long)ggd_tiles(P, RS32_TILE), chunks = (P + 1023) / 1024;
    printf("select=%d%d%d ", s0.n_valid == tmp + RS_HWORDS + RS_MAX_PASSES, s1.n_valid == ggd_sort_ctl::in_clean(clean, tmp).n_valid,
           s2.flat == ggd_sort_ctl::in_fold(fold).flat);
    printf("pass1_status=%td rowtot=%td l1_status=%td ", s0.pass_status(1, tiles) - s0.status, ggd_fold_rowtot(fold) - fold,
           ggd_fold_l1_status(fold, P) - fold);
    printf("gshift_tiles=%d gshift_chunks=%d status_words=%lld fold_ctl_words=%zu fold_l1_offset=%zu sort_tmp_bytes=%zu "
           "sort32_tmp_bytes=%zu msd_table_bytes=%zu ctrl_words=%zu\n",
           ggd_group_shift(tiles), ggd_group_shift(chunks > 0 ? chunks : 1), (long long)rs_status_words(tiles), ggd_fold_ctl_words(P),
           ggd_fold_l1_offset(P), ggd_sort_tmp_bytes(P), ggd_sort32_tmp_bytes(P), ggd_sort32_msd_table_bytes(P), ggd_sort_ctrl_words());
  }
  return 0;
}
