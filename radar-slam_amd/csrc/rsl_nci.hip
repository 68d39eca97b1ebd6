// rsl_nci.hip — non-coherent integration for gfx950 (rsl_power_integrate, include/rsl.h): the antenna-summed power map
//   P[f, i, j] = ((p_0 + p_1) + p_2) + ... + p_{A-1},   p_a = cabs2(rds[f, a, i, j])   (fp32, antenna order fixed)
// that rsl_detect_power runs the three detection rules on.  For A = 1 it is the power the detectors form themselves.
//
// Purely HBM-bound: 8 A bytes read and 4 written per cell, no reuse.  A lane owns four consecutive cells of a frame's
// [S * C] plane: per antenna plane two 16-B loads (32 contiguous bytes per lane, 2 KiB per wave), one 16-B store.  The
// loads of up to kNciPlanes = 8 planes (16 loads, 64 VGPRs) are issued before the first add; with more antennas the
// planes go in groups of 8, in antenna order, so the sum's order is the header's at every A.  Shapes whose planes do
// not keep the 16-B alignment (S * C not a multiple of 4, or an unaligned pointer) take the scalar form of the same
// body: one cell per lane, 8-B loads, a 4-B store.
#if defined(__HIP_DEVICE_COMPILE__)
#pragma clang attribute push(__attribute__((target("no-packed-fp32-ops"))), apply_to = function)
#endif
#include "rsl_common.h"
#include "rsl_internal.h"

namespace rsl {

namespace {

constexpr int kNciPlanes = 8;  // planes whose loads are in flight together

// V consecutive cells of one plane, as the lane loads them.
template <int V>
struct NciCells;
template <>
struct NciCells<4> {
  float4 lo, hi;  // (re, im) of cells 0, 1 and of cells 2, 3
  RSL_DEV void load(const float2* p) {
    const float4* q = reinterpret_cast<const float4*>(p);
    lo = q[0];
    hi = q[1];
  }
  RSL_DEV void add_to(float* acc) const {
    acc[0] += cabs2(make_float2(lo.x, lo.y));
    acc[1] += cabs2(make_float2(lo.z, lo.w));
    acc[2] += cabs2(make_float2(hi.x, hi.y));
    acc[3] += cabs2(make_float2(hi.z, hi.w));
  }
};
template <>
struct NciCells<1> {
  float2 z;
  RSL_DEV void load(const float2* p) { z = *p; }
  RSL_DEV void add_to(float* acc) const { acc[0] += cabs2(z); }
};

// acc += the powers of NA planes from `src` on (plane stride N values), every load before the first add.
template <int V, int NA>
RSL_DEV void nci_add_planes(const float2* __restrict__ src, size_t N, float* acc) {
  NciCells<V> z[NA];
#pragma unroll
  for (int k = 0; k < NA; ++k) z[k].load(src + (size_t)k * N);
#pragma unroll
  for (int k = 0; k < NA; ++k) z[k].add_to(acc);
}

}  // namespace

// rds c64 [F][A][N] -> power f32 [F][N], N = S * C; V cells per lane (4: N % 4 == 0 and both pointers 16-B aligned).
// Block b covers lanes' cell groups (b % nb) * 256 .. of frame b / nb, nb = ceil(N / V / 256).
template <int V>
__global__ __launch_bounds__(256) void k_power_integrate(const float2* __restrict__ rds, int A, size_t N, unsigned nb,
                                                         float* __restrict__ power) {
  const size_t f = blockIdx.x / nb;
  const size_t c0 = ((size_t)(blockIdx.x % nb) * 256 + threadIdx.x) * V;  // the lane's first cell
  if (c0 >= N) return;  // V divides N: a lane's cells are all inside or all outside
  const float2* src = rds + f * A * N + c0;
  float acc[V];
#pragma unroll
  for (int v = 0; v < V; ++v) acc[v] = 0.f;  // 0 + p_0 = p_0 exactly (p_0 >= +0)
  int a = 0;
  for (; a + kNciPlanes <= A; a += kNciPlanes) nci_add_planes<V, kNciPlanes>(src + (size_t)a * N, N, acc);
  switch (A - a) {  // the rest, wave-uniform
    case 1: nci_add_planes<V, 1>(src + (size_t)a * N, N, acc); break;
    case 2: nci_add_planes<V, 2>(src + (size_t)a * N, N, acc); break;
    case 3: nci_add_planes<V, 3>(src + (size_t)a * N, N, acc); break;
    case 4: nci_add_planes<V, 4>(src + (size_t)a * N, N, acc); break;
    case 5: nci_add_planes<V, 5>(src + (size_t)a * N, N, acc); break;
    case 6: nci_add_planes<V, 6>(src + (size_t)a * N, N, acc); break;
    case 7: nci_add_planes<V, 7>(src + (size_t)a * N, N, acc); break;
    default: break;
  }
  float* dst = power + f * N + c0;
  if constexpr (V == 4) {
    *reinterpret_cast<float4*>(dst) = make_float4(acc[0], acc[1], acc[2], acc[3]);
  } else {
    dst[0] = acc[0];
  }
}

hipError_t launch_power_integrate(hipStream_t st, const float2* rds, int F, int A, int S, int C, float* power) {
  if (F <= 0 || A <= 0 || S <= 0 || C <= 0) return hipSuccess;
  const size_t N = (size_t)S * C;
  const bool vec = N % 4 == 0 && ((reinterpret_cast<size_t>(rds) | reinterpret_cast<size_t>(power)) & 15) == 0;
  const size_t per = vec ? 4 * 256 : 256;
  const size_t nb = (N + per - 1) / per;
  return launch(st, vec ? k_power_integrate<4> : k_power_integrate<1>, (long long)(nb * (size_t)F), 256, 0, rds, A, N,
                (unsigned)nb, power);
}

}  // namespace rsl

#if defined(__HIP_DEVICE_COMPILE__)
#pragma clang attribute pop
#endif
