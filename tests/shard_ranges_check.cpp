// shard_ranges_check.cpp — prints shard_ranges (csrc/prover/shard_ranges.h) for a grid of small shapes, one line per
// (shape, count, rank); tests/test_shard_ranges.py checks the lines' properties.  Stand-alone: no device, no library.
#include <stdio.h>

#include "prover/shard_ranges.h"

int main()
{
  const uint32_t n_vars_set[] = {1, 2, 7, 64, 1000, 1025};
  const uint32_t domains[] = {1024, 4096, 8192};
  for (uint32_t n_vars : n_vars_set)
    for (int pub = 0; pub < 3; pub++) {
      const uint32_t n_public = pub == 0 ? 0 : pub == 1 ? 1 : n_vars - 1;
      if (n_public + 1 > n_vars || (pub == 2 && n_public <= 1)) continue; // (not a key; or one of the first two again)
      for (uint32_t domain : domains)
        for (int count = 1; count <= 8; count++)
          for (int rank = 0; rank < count; rank++) {
            const isnark::prover::ShardRanges r = isnark::prover::shard_ranges(n_vars, n_public, domain, rank, count);
            printf("%u %u %u %d %d  %u %u  %u %u  %u %u %u %u  %d %d\n", n_vars, n_public, domain, count, rank, r.wlo, r.whi, r.clo, r.chi, r.hlo, r.hhi, r.h_stride, r.h_first,
                   (int)r.slice_aligned, (int)r.h_strided);
          }
    }
  return 0;
}
