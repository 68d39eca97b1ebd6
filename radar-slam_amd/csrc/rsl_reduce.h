// rsl_reduce.h — the one workgroup reduction of the fp64 kernels (the velocity solvers, rsl_aux.hip, rsl_eval.hip).
//
// The scheme, in two stages.  The order of operations is part of the interface: the outputs of these kernels are
// compared bit for bit (tools/chain_hash.py, tools/solver_hash.py).
//
//   Stage A  wg_partials   each wave combines its 64 lanes by a shuffle-down tree (offsets 32, 16, ..., 1; lane 0 ends
//                          with the wave's value, the other lanes with values nobody may use) and lane 0 stores it to
//                          red[wave * K + q]; then ONE __syncthreads().  K values go through in one pass, each with
//                          its own combine.
//   Stage B  wg_fold       one value q: init, then the wave partials combined onto it in ascending wave order.  Plain
//                          LDS reads, no barrier, callable by any thread after stage A: thread 0 into registers,
//                          thread 0 into LDS (the caller's barrier then publishes it), or thread q < K into a global
//                          partial.  init is the caller's: 0.0 for a sum (0.0 + -0.0 is +0.0, so a sum never returns
//                          -0.0), below every operand for a maximum.
//
// The contract, for every function here:
//   - Every thread of the workgroup makes the call (stage A holds a barrier), with all 64 lanes of its wave active.
//   - red is the caller's LDS, kWaves * K elements; no function here declares LDS of its own.
//   - Stage A holds the only barrier, between the wave stores and the fold.  There is none in front of the stores and
//     none behind the fold.  So before red is written again (the next stage A on it, or any other use) the caller owes
//     a barrier after the last fold that reads it; and where a fold's result goes to LDS for other threads, that same
//     barrier is the one that publishes it.
//   - Stage A's barrier also orders, like any barrier, whatever the threads did before the call against what they do
//     after it; a call site that relies on this says so.
//
// wg_sums and wg_one are the two stages put together for the common cases, with the same barrier and the same debt.
// Every helper is force-inlined; see the fp-contract note of rsl_vel_common.h on why their text stays as it is.
#pragma once
#include "rsl_common.h"

namespace rsl {

enum class Red { Sum, Max };

template <Red op>
RSL_DEV double red_op(double a, double b) {
  return op == Red::Sum ? a + b : fmax(a, b);
}
template <Red op>
RSL_DEV unsigned long long red_op(unsigned long long a, unsigned long long b) {
  return op == Red::Sum ? a + b : (b > a ? b : a);
}

// Stage A.  op: one combine for all K values, or K of them, one per value.  T: double or unsigned long long.
template <Red... op, class T, int K>
RSL_DEV void wg_partials(const T (&v)[K], T* red) {
  static_assert(sizeof...(op) == 1 || sizeof...(op) == K, "one combine for all values, or one per value");
  constexpr Red ops[] = {op...};
  const int t = threadIdx.x;
  // All K trees, then all K stores under one branch.  With the store inside the loop every value gets a basic block of
  // its own and the K chains of 6 dependent shuffles run one after the other, not interleaved: k_velocity_robust took
  // 2.258 instead of 2.223 ms per 2000 cfg2 frames (Huber, given scale) that way.
  T x[K];
#pragma unroll
  for (int q = 0; q < K; ++q) {
    const bool sum = ops[sizeof...(op) == 1 ? 0 : q] == Red::Sum;
    x[q] = v[q];
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) {
      const T o = __shfl_down(x[q], off);
      x[q] = sum ? red_op<Red::Sum>(x[q], o) : red_op<Red::Max>(x[q], o);
    }
  }
  if ((t & 63) == 0)
#pragma unroll
    for (int q = 0; q < K; ++q) red[(t >> 6) * K + q] = x[q];
  __syncthreads();
}

// Stage B: value q of K over the kWaves waves of the workgroup.
template <int kWaves, int K, Red op, class T>
RSL_DEV T wg_fold(const T* red, int q, T init) {
  T r = init;
#pragma unroll
  for (int w = 0; w < kWaves; ++w) r = red_op<op>(r, red[w * K + q]);
  return r;
}

// K sums in one pass, folded by thread 0 into dst[0..K) (registers or LDS; other threads leave dst alone).
template <int kWaves, int K>
RSL_DEV void wg_sums(const double (&v)[K], double* red, double* dst) {
  wg_partials<Red::Sum>(v, red);
  if (threadIdx.x == 0)
    for (int q = 0; q < K; ++q) dst[q] = wg_fold<kWaves, K, Red::Sum>(red, q, 0.0);
}

// One value; the result is valid on thread 0 (the other threads get init).
template <int kWaves, Red op>
RSL_DEV double wg_one(double v, double* red, double init) {
  const double a[1] = {v};
  wg_partials<op>(a, red);
  return threadIdx.x == 0 ? wg_fold<kWaves, 1, op>(red, 0, init) : init;
}

}  // namespace rsl
