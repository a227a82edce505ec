// Stand-alone host program (tests/test_prio_phase_cpu.py builds it with g++ -fsanitize=address,undefined and runs it;
// bbx_common.h is all it includes): bbx_prio_phase, the one statement of the step kernels' priority rotation, over sweeps of
// the 100 MHz clock's low 32 bits — from 0, around the slot boundaries of a far-away stretch and across the wrap.  One line
// per property: "<name> cases <n> bad <n>".
#include <stdint.h>
#include <stdio.h>

#include "bbx_common.h"

int main() {
  const uint32_t slot = 1u << BBX_PRIO_TICK_SHIFT, cycle = 4u * slot;
  long long n_range = 0, bad_range = 0, n_distinct = 0, bad_distinct = 0, n_share = 0, bad_share = 0, n_wrap = 0, bad_wrap = 0;
  // a window of three cycles starting at each of these ticks, every tick of it (the last one runs through the wrap to 2 cycles
  // past 0; the one before starts in the middle of a slot just under 2^31, where a signed shift would go wrong)
  const uint32_t starts[] = {0u, 12345u, 0x7fffffffu - slot / 2, 0x80000000u - cycle, 0u - cycle};
  for (uint32_t start : starts) {
    long long held[4][4] = {{0}};                       // [rank][priority]: ticks of the window's first WHOLE cycle
    const uint32_t first_whole = (start + cycle - 1) / cycle * cycle;   // (wraps to 0 for the last window: its cycle begins at tick 0)
    for (uint32_t d = 0; d < 3 * cycle; d++) {
      const uint32_t t = start + d;
      int seen = 0;
      for (int rank = 0; rank < 4; rank++) {
        const int pr = bbx_prio_phase(t, rank);
        n_range++; bad_range += !(pr >= 0 && pr <= 3);
        if (pr >= 0 && pr <= 3) {
          seen |= 1 << pr;
          if ((uint32_t)(t - first_whole) < cycle) held[rank][pr]++;
        }
      }
      n_distinct++; bad_distinct += seen != 15;          // the four ranks hold the four priorities
    }
    for (int rank = 0; rank < 4; rank++)
      for (int pr = 0; pr < 4; pr++) { n_share++; bad_share += held[rank][pr] != (long long)slot; }
  }
  // the wrap is no seam: the tick before 0 and tick 0 are neighbours in the rotation (the slot ends there, the next priority follows)
  for (int rank = 0; rank < 4; rank++) {
    n_wrap++; bad_wrap += bbx_prio_phase(0u, rank) != ((bbx_prio_phase(0xffffffffu, rank) + 1) & 3);
    n_wrap++; bad_wrap += bbx_prio_phase(0xffffffffu, rank) != bbx_prio_phase(0u - slot, rank);
  }
  printf("shift cases %d bad 0\n", BBX_PRIO_TICK_SHIFT);
  printf("range cases %lld bad %lld\n", n_range, bad_range);
  printf("distinct cases %lld bad %lld\n", n_distinct, bad_distinct);
  printf("share cases %lld bad %lld\n", n_share, bad_share);
  printf("wrap cases %lld bad %lld\n", n_wrap, bad_wrap);
  return (bad_range || bad_distinct || bad_share || bad_wrap) ? 1 : 0;
}
