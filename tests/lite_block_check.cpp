// Stand-alone host program (tests/test_abi_cpu.py builds it with g++; bbx_common.h is all it includes): prints the output
// block's layout and round-trips the status word, for the test to compare with the documented layout.  Also the program to
// build with -fsanitize=address,undefined when the block's definition changes.
#include <stdio.h>

#include "bbx_common.h"

int main() {
  const size_t Bs[] = {1, 8, 64, 4096};
  for (size_t B : Bs) {
    const BbxOutLayout o = bbx_out_layout(B);
    printf("layout %zu %zu %zu %zu %zu %zu\n", B, o.lite, o.rewards, o.rows, o.dones, o.bytes);
  }
  printf("seq_of %d %d %d %d\n", bbx_lite_seq_of(0), bbx_lite_seq_of(BBX_LITE_SEQ_MOD - 1), bbx_lite_seq_of(BBX_LITE_SEQ_MOD), bbx_lite_seq_of((1 << 30) - 1));
  const int seqs[] = {1, BBX_LITE_SEQ_MOD, bbx_lite_seq_of(BBX_LITE_SEQ_MOD - 1), bbx_lite_seq_of(BBX_LITE_SEQ_MOD)};
  int bad = 0;
  for (int status = 0; status <= BBX_LITE_STATUS_MASK; status++)
    for (int trunc = 0; trunc < 2; trunc++)
      for (int seq : seqs) {
        const int32_t w = bbx_lite_word0(status, trunc, seq);
        const int back = bbx_lite_status(w) == status && ((w & BBX_LITE_OBS_TRUNC) != 0) == (trunc != 0) && bbx_lite_seq(w) == seq && w >= 0;
        bad += !back;
        if (status <= BBX_ST_TIMESLICE) printf("word0 %d %d %d %d %d %d %d\n", status, trunc, seq, (int)w, bbx_lite_status(w), (w & BBX_LITE_OBS_TRUNC) ? 1 : 0, bbx_lite_seq(w));
      }
  BbxLite l = {bbx_lite_word0(BBX_ST_OK, 0, 1), 2, ((1 << 30) - 1) | BBX_LITE_GONE, 4};
  printf("gone %d %d\n", (l.budget & BBX_LITE_GONE) != 0, l.budget & ~BBX_LITE_GONE);
  printf("bad %d\n", bad);
  return bad != 0;
}
