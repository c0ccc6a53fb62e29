// Band-limited SO(2) fields on a channels-last map, shared by fourier_act.hip (FourierELU) and field_norm.hip (the field norm's
// training kernels).  A field is 9 consecutive fp32: a_0, then (Re c_m, Im c_m) for m = 1..4; it describes
//   f(phi) = a_0 + sum_m sqrt(2) (Re c_m cos(m phi) + Im c_m sin(m phi)).
// A is the 16 x 9 matrix of its samples at phi_i = 2 pi i / 16 (A^T A = 16 I).  The two 16 x 9 products are straight-line code over
// compile-time constants (zeros and ones fold away).  The 36-byte rows of a run of fields are contiguous bytes: a block moves them
// between global memory and LDS as whole 16-byte lines, and a thread reads / writes its nine values in LDS at a stride of 9 dwords
// (odd: no bank conflicts).
#pragma once

#include "eqa_common.hpp"

namespace eqa {

constexpr int kFieldDim = 9;                          // 1 + 2 * 4 coefficients
constexpr int kSamples = 16;
constexpr int kTileFloats = kThreads * kFieldDim;     // 2304 floats = 576 float4 per block
constexpr int kTileVec = kTileFloats / 4;

// cos(k pi / 8), k = 0..15
constexpr double kCos16[16] = {1.0, 0.92387953251128674, 0.70710678118654752, 0.38268343236508977, 0.0, -0.38268343236508977,
                               -0.70710678118654752, -0.92387953251128674, -1.0, -0.92387953251128674, -0.70710678118654752,
                               -0.38268343236508977, 0.0, 0.38268343236508977, 0.70710678118654752, 0.92387953251128674};
constexpr double kSqrt2 = 1.41421356237309505;

// A[i][j]: j = 0 -> 1;  j = 2m-1 -> sqrt2 cos(m phi_i);  j = 2m -> sqrt2 sin(m phi_i) = sqrt2 cos(m phi_i - pi/2)
constexpr float sample_coeff(int i, int j) {
  if (j == 0) return 1.0f;
  const int m = (j + 1) / 2;
  const int k = (j & 1) ? (m * i) % 16 : (m * i + 12) % 16;
  return (float)(kSqrt2 * kCos16[k]);
}

template <int I, int J>
struct Coeff {
  static constexpr float value = sample_coeff(I, J);
};

template <int I, int J = 0>
__device__ __forceinline__ float sample_row(const float (&u)[kFieldDim]) {      // sum_j A[I][j] u[j]
  if constexpr (J == kFieldDim) {
    return 0.0f;
  } else {
    constexpr float a = Coeff<I, J>::value;
    const float rest = sample_row<I, J + 1>(u);
    if constexpr (a == 0.0f) return rest;
    else if constexpr (a == 1.0f) return rest + u[J];
    else if constexpr (a == -1.0f) return rest - u[J];
    else return fmaf(a, u[J], rest);
  }
}

template <int I = 0>
__device__ __forceinline__ void sample_all(const float (&u)[kFieldDim], float (&s)[kSamples]) {
  if constexpr (I < kSamples) {
    s[I] = sample_row<I>(u);
    sample_all<I + 1>(u, s);
  }
}

template <int J, int I = 0>
__device__ __forceinline__ float project_col(const float (&s)[kSamples]) {       // sum_i A[i][J] s[i]
  if constexpr (I == kSamples) {
    return 0.0f;
  } else {
    constexpr float a = Coeff<I, J>::value;
    const float rest = project_col<J, I + 1>(s);
    if constexpr (a == 0.0f) return rest;
    else if constexpr (a == 1.0f) return rest + s[I];
    else if constexpr (a == -1.0f) return rest - s[I];
    else return fmaf(a, s[I], rest);
  }
}

template <int J = 0>
__device__ __forceinline__ void project_all(const float (&s)[kSamples], float (&v)[kFieldDim]) {
  if constexpr (J < kFieldDim) {
    v[J] = project_col<J>(s);
    project_all<J + 1>(s, v);
  }
}

// the first nvec 16-byte lines of the tile at float offset `base` of a map of n floats -> LDS (or back), 16 bytes per lane; the
// last line of the map may be partial
__device__ __forceinline__ void tile_load(const float* __restrict__ g, float* lds, size_t base, size_t n, int nvec = kTileVec) {
  for (int v = threadIdx.x; v < nvec; v += kThreads) {
    const size_t at = base + (size_t)v * 4;
    if (at + 4 <= n) {
      *reinterpret_cast<float4*>(lds + v * 4) = *reinterpret_cast<const float4*>(g + at);
    } else {
      for (int e = 0; e < 4; ++e)
        if (at + e < n) lds[v * 4 + e] = g[at + e];
    }
  }
}
__device__ __forceinline__ void tile_store(float* __restrict__ g, const float* lds, size_t base, size_t n, int nvec = kTileVec) {
  for (int v = threadIdx.x; v < nvec; v += kThreads) {
    const size_t at = base + (size_t)v * 4;
    if (at + 4 <= n) {
      *reinterpret_cast<float4*>(g + at) = *reinterpret_cast<const float4*>(lds + v * 4);
    } else {
      for (int e = 0; e < 4; ++e)
        if (at + e < n) g[at + e] = lds[v * 4 + e];
    }
  }
}

// sc[0..4]: the field's per-frequency scales (1 when there is no table), sh: its shift on a_0 (0 when there is none)
__device__ __forceinline__ void field_table(const float* __restrict__ scale, const float* __restrict__ shift, int field, float (&sc)[5],
                                            float& sh) {
#pragma unroll
  for (int m = 0; m < 5; ++m) sc[m] = scale ? scale[field * 5 + m] : 1.0f;
  sh = shift ? shift[field] : 0.0f;
}
// u = scale (.) x + shift
__device__ __forceinline__ void field_affine(const float* lds_row, const float (&sc)[5], float sh, float (&u)[kFieldDim]) {
  u[0] = fmaf(sc[0], lds_row[0], sh);
#pragma unroll
  for (int j = 1; j < kFieldDim; ++j) u[j] = sc[(j + 1) / 2] * lds_row[j];
}
__device__ __forceinline__ void field_affine(const float* lds_row, const float* __restrict__ scale, const float* __restrict__ shift,
                                             int field, float (&sc)[5], float (&u)[kFieldDim]) {
  float sh;
  field_table(scale, shift, field, sc, sh);
  field_affine(lds_row, sc, sh, u);
}

// du = A^T [ELU'(A u) (.) (A dy / 16)]: the gradient of y = A^T ELU(A u) / 16 with respect to u, the 16 samples recomputed from u
__device__ __forceinline__ void field_elu_grad(const float (&u)[kFieldDim], const float* lds_grad_row, float (&du)[kFieldDim]) {
  float s[kSamples], g[kFieldDim], gs[kSamples];
  sample_all(u, s);
#pragma unroll
  for (int j = 0; j < kFieldDim; ++j) g[j] = lds_grad_row[j] * (1.0f / kSamples);
  sample_all(g, gs);                                   // A dy / 16: the gradient at the 16 samples
#pragma unroll
  for (int i = 0; i < kSamples; ++i) gs[i] = s[i] > 0.0f ? gs[i] : gs[i] * expf(s[i]);
  project_all(gs, du);
}

// field index of this thread's item, (blockIdx.x * 256 + threadIdx.x) % fields: the 64-bit remainder once per block (uniform), a
// 32-bit one per thread
__device__ __forceinline__ int field_of_item(int fields) {
  const unsigned first = (unsigned)(((size_t)blockIdx.x * kThreads) % (size_t)fields);
  return (int)((first + threadIdx.x) % (unsigned)fields);
}

}  // namespace eqa
