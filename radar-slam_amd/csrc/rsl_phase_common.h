// rsl_phase_common.h — what the phase-model solvers share (the linear ones in rsl_aux.hip, the wrapped ones in
// rsl_wrap.hip): the Jacobian row of the model k (v + w x p).d = k J . [v; w], and the workgroup argmin their searches
// end in.
#pragma once
#include "rsl_common.h"

namespace rsl {

// J = [d, p x d], d = (cos el cos az, cos el sin az, sin el)  (velocity_solver.py:94-109); pos [3], ang [2] = (az, el).
RSL_DEV void jacobian_row(const double* pos, const double* ang, double* J) {
  const double az = ang[0], el = ang[1];
  const double ce = cos(el);
  const double d0 = ce * cos(az), d1 = ce * sin(az), d2 = sin(el);
  // (w x p).d = w . (p x d)
  const double px = pos[0], py = pos[1], pz = pos[2];
  J[0] = d0;
  J[1] = d1;
  J[2] = d2;
  J[3] = py * d2 - pz * d1;
  J[4] = pz * d0 - px * d2;
  J[5] = px * d1 - py * d0;
}

// Argmin of (key, idx) over the workgroup's NT threads: the lowest key wins, then the lowest idx; idx < 0 is "no
// candidate" and never wins.  sd, si: NT entries of LDS each.  The winner is in sd[0] / si[0] (si[0] < 0: there was
// none), readable by every thread on return; a barrier must come before the arrays are written again.
template <int NT>
RSL_DEV void block_argmin(double key, long idx, double* sd, long* si) {
  const int t = threadIdx.x;
  sd[t] = key;
  si[t] = idx;
  __syncthreads();
  for (int off = NT / 2; off > 0; off >>= 1) {
    if (t < off) {
      const double od = sd[t + off];
      const long oi = si[t + off];
      if (oi >= 0 && (si[t] < 0 || od < sd[t] || (od == sd[t] && oi < si[t]))) {
        sd[t] = od;
        si[t] = oi;
      }
    }
    __syncthreads();
  }
}

}  // namespace rsl
