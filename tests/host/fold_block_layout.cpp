// fold_block_layout.cpp -- stand-alone check of the fold block's appended region (csrc/ggd_binning_layout.h: the instances per
// tile row behind the level-1 status words).  Reads "P" lines from stdin; for each it allocates a block of
// ggd_fold_block_words(P) words as the library does, writes every word of the level-1 status rows and of the new region through
// the header's own pointer functions (under -fsanitize=address a region outside the allocation aborts here) and prints the
// figures for tests/test_fold_block_layout_host.py to compare with the formulas restated there.
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "ggd_binning_layout.h"

int main() {
  long long P;
  while (std::scanf("%lld", &P) == 1) {
    const size_t words = ggd_fold_block_words(P);
    std::vector<uint32_t> block(words, 0u);
    const long long chunks = (P + 1023) / 1024;
    const size_t l1_rows = (size_t)(chunks + (1ll << ggd_group_shift(chunks > 0 ? chunks : 1)) + 2);
    uint32_t* l1 = ggd_fold_l1_status(block.data(), P);
    for (size_t w = 0; w < l1_rows * 64; ++w) l1[w] += 1u;
    uint32_t* inst = ggd_fold_rowinst(block.data(), P);
    for (int w = 0; w < GGD_FOLD_REPS * 64; ++w) inst[w] += 2u;
    size_t ones = 0, twos = 0, other = 0;
    for (size_t w = 0; w < words; ++w) { ones += block[w] == 1u; twos += block[w] == 2u; other += block[w] > 2u; }
    std::printf("P=%lld rowinst_offset=%zu block_words=%zu ctl_words=%zu l1_offset=%zu l1_end=%zu ones=%zu twos=%zu overlap=%zu "
                "rowtot=%d head=%d reps=%d tab_rowstart=%d tab_rowblk=%d tab_tilestart=%d tab_rowinst=%d tab_flag=%d tab_words=%d "
                "max_blocks=%u blocks_cube=%u blocks_shell=%u\n",
                P, ggd_fold_rowinst_offset(P), words, ggd_fold_ctl_words(P), ggd_fold_l1_offset(P),
                ggd_fold_l1_offset(P) + l1_rows * 64, ones, twos, other, GGD_FOLD_ROWTOT, GGD_FOLD_HEAD, GGD_FOLD_REPS,
                RB_TAB_ROWSTART, RB_TAB_ROWBLK, RB_TAB_TILESTART, RB_TAB_ROWINST, RB_TAB_FLAG, RB_TAB_WORDS,
                RB_SCAN_IN_SCATTER_MAX_BLOCKS, rb_blocks2(5931642u, false), rb_blocks2(16777217u, false));
  }
  return 0;
}
