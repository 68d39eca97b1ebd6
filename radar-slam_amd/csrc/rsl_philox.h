// rsl_philox.h — the counter-based generator of the library: the synthetic cube's noise (rsl_synth.hip) and the
// consensus solver's hypothesis draws (rsl_vel_consensus.hip).  tests/philox_ref.py mirrors it.
#pragma once
#include "rsl_common.h"

namespace rsl {

// Philox-4x32-10 (Salmon et al., SC'11): counter ctr, key (k0, k1).
RSL_DEV uint4 philox4x32_10(uint4 ctr, unsigned k0, unsigned k1) {
#pragma unroll
  for (int r = 0; r < 10; ++r) {
    const unsigned long long p0 = (unsigned long long)0xD2511F53u * ctr.x;
    const unsigned long long p1 = (unsigned long long)0xCD9E8D57u * ctr.z;
    ctr = make_uint4((unsigned)(p1 >> 32) ^ ctr.y ^ k0, (unsigned)p1, (unsigned)(p0 >> 32) ^ ctr.w ^ k1, (unsigned)p0);
    k0 += 0x9E3779B9u;
    k1 += 0xBB67AE85u;
  }
  return ctr;
}

}  // namespace rsl
