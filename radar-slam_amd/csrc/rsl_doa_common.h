// rsl_doa_common.h — what the direction-of-arrival kernels (rsl_doa.hip, rsl_doa_toep.hip, rsl_ssmusic.hip), their
// launchers and the C-ABI layer share: the cell list and the steering table's layout.
#pragma once
#include <hip/hip_runtime.h>

#include "rsl_common.h"
#include "rsl_internal.h"

namespace rsl {

// The cells of a DoA call: cell c is the A-antenna signature at (frame[c], rc[c] = range * C + doppler) of the
// range-Doppler spectrum rds c64 [F, A, S, C].  The list holds n_host cells, or min(*n_dev, n_host) when the count
// lives on the device (n_host is then the capacity).  Passed by value from the C-ABI layer through the launchers into
// the kernels.
struct CellList {
  const float2* rds;
  int A, S, C;
  const int* frame;
  const int* rc;
  const long long* n_dev;
  long long n_host;
  // The count is wave-uniform, but a pointer inside a struct carries no `__restrict__`, so the compiler cannot prove
  // that *n_dev stays as it is under the kernel and loads it per lane: readfirstlane moves it to the scalar registers,
  // where the kernels' loop bounds belong (two VGPRs less in every loop that tests it).
  RSL_DEV long long count() const {
    const long long n = list_count(n_dev, n_host);
    const unsigned lo = __builtin_amdgcn_readfirstlane((unsigned)n);
    const unsigned hi = __builtin_amdgcn_readfirstlane((unsigned)(n >> 32));
    return (long long)(((unsigned long long)hi << 32) | lo);
  }
  RSL_DEV size_t plane() const { return (size_t)S * C; }          // one antenna of one frame
  RSL_DEV size_t fstride() const { return (size_t)A * plane(); }  // one frame
  // antenna 0 of cell c; antenna m is plane() elements further
  RSL_DEV const float2* sig(long long c) const { return rds + (size_t)frame[c] * fstride() + rc[c]; }
  // antenna m of cell c, for a kernel that reads one antenna per lane
  RSL_DEV float2 at(long long c, int m) const { return rds[((size_t)frame[c] * A + m) * plane() + rc[c]]; }
};

// The sections of the steering table (rsl_steer_table_build), in floats from its start:
//  (1) the f32 MFMA operand of k_doa_scan / k_doa_argmax: ntiles16 tiles of 16 rows ([Re; Im] of 8 grid points), each
//      ks k-steps of 4 stacked-signature rows in ksg float4 groups per lane;
//  (2) the Toeplitz f16 hi/lo operand of k_doa_toep: nt32 tiles of 32 grid points (an even count), kb k-blocks of 16;
//      the kernel keeps all of it in LDS, so the path applies only where it fits 64 KiB (toep_fits);
//  (3) the fp64 steering matrix transposed, steerT[m][g] (double2), for k_doa_fixup's coalesced exact re-scan; at a
//      16-B aligned float offset (both sections before it are multiples of 4 floats).
struct SteerLayout {
  int ks, ksg, ntiles16;
  long long f32_floats;
  int kb, nt32;
  long long toep_floats;
  size_t toep_bytes;
  bool toep_fits;
  long long t64_offset, total_floats;
};

inline SteerLayout steer_layout(int G, int M) {
  SteerLayout l;
  l.ks = (2 * M + 3) / 4;
  l.ksg = (l.ks + 3) / 4;
  l.ntiles16 = (int)((2LL * G + 15) / 16);
  l.f32_floats = (long long)l.ntiles16 * l.ksg * 64 * 4;
  l.kb = M <= 8 ? 1 : 2;
  l.nt32 = (G + 31) / 32;
  l.nt32 += l.nt32 & 1;
  l.toep_floats = (long long)l.nt32 * l.kb * 2 * 64 * 4;
  l.toep_bytes = (size_t)l.toep_floats * sizeof(float);
  l.toep_fits = l.toep_bytes <= 64 * 1024;
  l.t64_offset = l.f32_floats + l.toep_floats;
  l.total_floats = l.t64_offset + 4LL * G * M;
  return l;
}

}  // namespace rsl
