// rsl_packed.h — the packed `work` format K1 (rsl_fft.hip) writes and K2 (rsl_doppler_detect.hip) reads at the
// work_packed_supported shapes: the 16-B / 8-B global accesses with the optional non-temporal hint, the 23-bit field
// codec with a per-bin exponent, K1's packed epilogue and K2's unit load.  Both files include it inside their
// no-packed-fp32-ops region.
#pragma once
#include "rsl_common.h"

namespace rsl {

// Global accesses with an optional non-temporal hint (`nt`: streamed once, not kept in L2 / MALL).
typedef float f4v __attribute__((ext_vector_type(4)));
typedef float f2v __attribute__((ext_vector_type(2)));
template <bool NTH>
RSL_DEV float4 ld16(const float4* p) {
  if constexpr (NTH) {
    return __builtin_bit_cast(float4, __builtin_nontemporal_load(reinterpret_cast<const f4v*>(p)));
  } else {
    return *p;
  }
}
template <bool NTH>
RSL_DEV void st16(float4* p, float4 x) {
  if constexpr (NTH) {
    f4v v = {x.x, x.y, x.z, x.w};
    __builtin_nontemporal_store(v, reinterpret_cast<f4v*>(p));
  } else {
    *p = x;
  }
}
template <bool NTH>
RSL_DEV float2 ld8(const float2* p) {
  if constexpr (NTH) {
    return __builtin_bit_cast(float2, __builtin_nontemporal_load(reinterpret_cast<const f2v*>(p)));
  } else {
    return *p;
  }
}
template <bool NTH>
RSL_DEV void st8(float2* p, float2 x) {
  if constexpr (NTH) {
    f2v v = {x.x, x.y};
    __builtin_nontemporal_store(v, reinterpret_cast<f2v*>(p));
  } else {
    *p = x;
  }
}

// Packed `work` (K1 -> K2 at the work_packed_supported shapes).  Per K1 tile (frame, antenna, chirp
// class cb) a block of 6 planes x S / 2 bin pairs x 16 B (24 KiB at S = 512; pk_plane_bytes, pk_tile_bytes): planes
// 0-2 hold the even bin 2p of pair p, planes 3-5 the odd bin 2p + 1, each bin's 8 rows x (re, im) as 16 fields of 23
// bits plus the bin's exponent (12 dwords, 3 x 16 B).
// Every K1 store and every K2 load is a 16-B access: a K1 wave stores 1 KiB runs (lane = pair), a K2 lane loads the 3
// chunks of one (bin, chirp block) and a wave's loads cover whole 128-B lines (16 bins = 8 pairs of one plane, or the
// other plane).  Each bin of a tile has its own exponent e (int8); a field is n = rint(v 2^(22 - e)), |n| < 2^22, stored
// offset-binary (the low 23 bits of the f32 1.5 2^23 + n: every such f32 has exponent 2^23), so the value's error is
// <= 2^(e - 23) = two fp32 ulps of the bin's largest component, fp32-class for the RDS (1e-5 max-relative tolerance)
// and the peak decisions.  The exponent byte sits in the 4 spare bits of the first two field groups (round 3; it was
// a separate [tile][512] byte array before, 0.26 GB of extra K1 writes and K2 byte loads per 2000 frames, and the
// fields were 24-bit with the 24th bit always 0: the same values, bit for bit).
// 6 B per value instead of 8: K1 + K2 move 14.0 instead of 16.8 MB per cfg2 frame.
constexpr float kPkMagic = 12582912.0f;  // 1.5 * 2^23
constexpr int pk_plane_bytes(int S) { return 8 * S; }                 // one plane of one tile: S / 2 pairs x 16 B
constexpr int pk_tile_bytes(int S) { return 6 * pk_plane_bytes(S); }  // one tile
// frexp exponent of the largest |component| (abs bits), clamped so that both scale factors are normal floats
RSL_DEV int pk_exp(unsigned mbits) {
  const int e = (int)((mbits >> 23) & 0xFFu) - 126;
  return e < -100 ? -100 : (e > 127 ? 127 : e);
}
RSL_DEV float pk_pow2(int k) { return __uint_as_float((unsigned)(127 + k) << 23); }
// 16 fields (8 complex) of one bin with its exponent e -> 12 dwords: field group g (u0..u3, 23 bits each) and a nibble
// x_g in 96 bits, u0 | u1 << 23, u1 >> 9 | u2 << 14, u2 >> 18 | u3 << 5 | x_g << 28; x_0 / x_1 = the low / high nibble
// of the int8 e, x_2 = x_3 = 0
RSL_DEV void pk_pack16(const float (&f)[16], int e, uint4 (&o)[3]) {
  const float s = pk_pow2(22 - e);
  const rsl_f2v s2 = {s, s}, mg = {kPkMagic, kPkMagic};
  unsigned u[16], d[12];
#pragma unroll
  for (int c = 0; c < 16; c += 2) {
    // fma rounds v s to the nearest integer (|v s| < 2^22; one packed fma per complex value); the min keeps a value
    // that rounds up to 2^22 in range
    const rsl_f2v q = __builtin_elementwise_fma((rsl_f2v){f[c], f[c + 1]}, s2, mg);
    u[c] = min(__float_as_uint(q.x), 0x4B7FFFFFu) & 0x7FFFFFu;
    u[c + 1] = min(__float_as_uint(q.y), 0x4B7FFFFFu) & 0x7FFFFFu;
  }
  const unsigned eb = (unsigned)e & 0xFFu;
#pragma unroll
  for (int g = 0; g < 4; ++g) {
    const unsigned x = g == 0 ? (eb & 0xFu) : (g == 1 ? (eb >> 4) : 0u);
    d[3 * g] = u[4 * g] | (u[4 * g + 1] << 23);
    d[3 * g + 1] = (u[4 * g + 1] >> 9) | (u[4 * g + 2] << 14);
    d[3 * g + 2] = (u[4 * g + 2] >> 18) | (u[4 * g + 3] << 5) | (x << 28);
  }
  o[0] = make_uint4(d[0], d[1], d[2], d[3]);
  o[1] = make_uint4(d[4], d[5], d[6], d[7]);
  o[2] = make_uint4(d[8], d[9], d[10], d[11]);
}
RSL_DEV void pk_unpack16(const uint4 (&w)[3], float (&f)[16]) {
  const unsigned d[12] = {w[0].x, w[0].y, w[0].z, w[0].w, w[1].x, w[1].y, w[1].z, w[1].w,
                          w[2].x, w[2].y, w[2].z, w[2].w};
  const int e = (int)(signed char)((d[2] >> 28) | ((d[5] >> 28) << 4));
  const float s = pk_pow2(e - 22);
  const float off = -kPkMagic * s;
  const rsl_f2v s2 = {s, s}, o2 = {off, off};
  // (field & 0x7FFFFF) | 0x4B000000 as one bit-field insert; the two fields of a complex value decoded by one packed fma
  auto m = [](unsigned x) { return __uint_as_float(__builtin_amdgcn_ubfe(x, 0, 23) | 0x4B000000u); };
#pragma unroll
  for (int g = 0; g < 4; ++g) {
    const unsigned u0 = d[3 * g];
    const unsigned u1 = __builtin_amdgcn_alignbit(d[3 * g + 1], d[3 * g], 23);
    const unsigned u2 = __builtin_amdgcn_alignbit(d[3 * g + 2], d[3 * g + 1], 14);
    const unsigned u3 = d[3 * g + 2] >> 5;
    // 0x4B000000 | u = 2^23 + u = 1.5 2^23 + n exactly; (that - 1.5 2^23) s in one rounding (exact: n s)
    const rsl_f2v a = __builtin_elementwise_fma((rsl_f2v){m(u0), m(u1)}, s2, o2);
    const rsl_f2v b = __builtin_elementwise_fma((rsl_f2v){m(u2), m(u3)}, s2, o2);
    f[4 * g] = a.x;
    f[4 * g + 1] = a.y;
    f[4 * g + 2] = b.x;
    f[4 * g + 3] = b.y;
  }
}

// K1's packed epilogue (k_range_fft_r512 / _r1024 / _r256): the thread in slot `slot` holds bins 2 slot, 2 slot + 1 of
// the tile's 8 rows (chirps cb + (C / 8) q), at obuf[q * pitch + pos] (one 16-B read per row; pos carries the kernel's
// bank swizzle).  The Doppler transform's first step runs here in registers, Y[k1] = W_C^(cb k1) DFT8_q (K2 starts from
// the step over the classes), and both bins are stored packed: six 16-B stores.  NTW: stored with the nt hint.
template <int S, bool NTW>
RSL_DEV void k1_packed_store(const float2* obuf, int pitch, int pos, int cb, const float2* __restrict__ tw,
                             float2* __restrict__ work, size_t tile, int slot) {
  float2 y0[8], y1[8];
#pragma unroll
  for (int q = 0; q < 8; ++q) {
    const float4 ab = *reinterpret_cast<const float4*>(obuf + q * pitch + pos);
    y0[q] = make_float2(ab.x, ab.y);
    y1[q] = make_float2(ab.z, ab.w);
  }
  Dft<8>::run(y0);
  Dft<8>::run(y1);
  const int cbs = __builtin_amdgcn_readfirstlane(cb);  // the tile is workgroup-uniform
#pragma unroll
  for (int k = 1; k < 8; ++k) {
    const float2 wk = tw[4 * cbs * k];  // W_C^(cb k) = W_S^(4 cb k), 4 cb k < 7 S / 8 (workgroup-uniform: scalar loads)
    y0[k] = cmul(y0[k], wk);
    y1[k] = cmul(y1[k], wk);
  }
  float f0[16], f1[16];
  unsigned m0 = 0u, m1 = 0u;
#pragma unroll
  for (int q = 0; q < 8; ++q) {
    f0[2 * q] = y0[q].x;
    f0[2 * q + 1] = y0[q].y;
    f1[2 * q] = y1[q].x;
    f1[2 * q + 1] = y1[q].y;
    m0 = max(m0, max(__float_as_uint(y0[q].x) & 0x7FFFFFFFu, __float_as_uint(y0[q].y) & 0x7FFFFFFFu));
    m1 = max(m1, max(__float_as_uint(y1[q].x) & 0x7FFFFFFFu, __float_as_uint(y1[q].y) & 0x7FFFFFFFu));
  }
  const int e0 = pk_exp(m0), e1 = pk_exp(m1);
  uint4 w0[3], w1[3];
  pk_pack16(f0, e0, w0);
  pk_pack16(f1, e1, w1);
  constexpr int PL = pk_plane_bytes(S) / 16;
  uint4* dst = reinterpret_cast<uint4*>(reinterpret_cast<unsigned char*>(work) + tile * pk_tile_bytes(S)) + slot;
#pragma unroll
  for (int jj = 0; jj < 3; ++jj) {
    st16<NTW>(reinterpret_cast<float4*>(dst + jj * PL), __builtin_bit_cast(float4, w0[jj]));
    st16<NTW>(reinterpret_cast<float4*>(dst + (jj + 3) * PL), __builtin_bit_cast(float4, w1[jj]));
  }
}

// K2's packed prologue (k_doppler_detect_r128 / _r256 / _r64): the unit (3 x 16 B) of range bin k in chirp class cls of
// the (frame, antenna) whose first K1 tile is tile0.  DBG 6 (development builds): no work loads, a constant fill.
template <int S, int DBG>
RSL_DEV void pk_load_unit(const float2* __restrict__ work, size_t tile0, int k, int cls, uint4 (&w)[3]) {
  constexpr int PL = pk_plane_bytes(S);
  const uint4* src = reinterpret_cast<const uint4*>(reinterpret_cast<const unsigned char*>(work) +
                                                    (tile0 + cls) * pk_tile_bytes(S) + (size_t)(3 * (k & 1)) * PL) +
                     (k >> 1);
#pragma unroll
  for (int jj = 0; jj < 3; ++jj) {
    if constexpr (DBG == 6)
      w[jj] = make_uint4(0x4B4000u + threadIdx.x, 0x5Au * jj, 0x4B40u + k, 0x12345u);
    else
      w[jj] = src[jj * (PL / 16)];
  }
}

}  // namespace rsl
