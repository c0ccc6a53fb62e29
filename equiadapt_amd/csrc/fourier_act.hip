// FourierELU over band-limited SO(2) fields (ESCNNSteerableNetwork's hidden activation), fused with the field norm's eval-mode
// affine map.  A field is 9 consecutive fp32 of a channels-last map: a_0, then (Re c_m, Im c_m) for m = 1..4; it describes
//   f(phi) = a_0 + sum_m sqrt(2) (Re c_m cos(m phi) + Im c_m sin(m phi)).
// Forward, per (pixel, field):  u = scale (.) x + shift (a_0 only),  s_i = f_u(2 pi i / 16) for i = 0..15,  y = A^T ELU(s) / 16, where
// A is the 16 x 9 sampling matrix above (A^T A = 16 I).  Backward: dx = scale (.) A^T [ELU'(s) (.) (A dy / 16)], s recomputed from x.
//
// One thread per (pixel, field).  The 36-byte rows of a block's 256 fields are 9216 contiguous bytes: the block moves them between
// global memory and LDS as whole 16-byte lines, and a thread reads / writes its nine values in LDS at a stride of 9 dwords (odd: no
// bank conflicts).  The two 16 x 9 products are straight-line code over compile-time constants (zeros and ones fold away).  No
// atomics: the result does not depend on the launch.
#include "eqa_common.hpp"

namespace {

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

// n floats starting at the block's tile -> LDS (or back), 16 bytes per lane; the last line of the map may be partial
__device__ __forceinline__ void tile_load(const float* __restrict__ g, float* lds, size_t base, size_t n) {
  for (int v = threadIdx.x; v < kTileVec; v += kThreads) {
    const size_t at = base + (size_t)v * 4;
    if (at + 4 <= n) {
      *reinterpret_cast<float4*>(lds + v * 4) = *reinterpret_cast<const float4*>(g + at);
    } else {
      for (int e = 0; e < 4; ++e)
        if (at + e < n) lds[v * 4 + e] = g[at + e];
    }
  }
}
__device__ __forceinline__ void tile_store(float* __restrict__ g, const float* lds, size_t base, size_t n) {
  for (int v = threadIdx.x; v < kTileVec; v += kThreads) {
    const size_t at = base + (size_t)v * 4;
    if (at + 4 <= n) {
      *reinterpret_cast<float4*>(g + at) = *reinterpret_cast<const float4*>(lds + v * 4);
    } else {
      for (int e = 0; e < 4; ++e)
        if (at + e < n) g[at + e] = lds[v * 4 + e];
    }
  }
}

// u = scale (.) x + shift; sc[0..4] the field's per-frequency scales (1 when there is no table)
__device__ __forceinline__ void field_affine(const float* lds_row, const float* __restrict__ scale, const float* __restrict__ shift,
                                             int field, float (&sc)[5], float (&u)[kFieldDim]) {
#pragma unroll
  for (int m = 0; m < 5; ++m) sc[m] = scale ? scale[field * 5 + m] : 1.0f;
  u[0] = fmaf(sc[0], lds_row[0], shift ? shift[field] : 0.0f);
#pragma unroll
  for (int j = 1; j < kFieldDim; ++j) u[j] = sc[(j + 1) / 2] * lds_row[j];
}

// field index of this thread's item, (blockIdx.x * 256 + threadIdx.x) % fields: the 64-bit remainder once per block (uniform), a
// 32-bit one per thread
__device__ __forceinline__ int field_of_item(int fields) {
  const unsigned first = (unsigned)(((size_t)blockIdx.x * kThreads) % (size_t)fields);
  return (int)((first + threadIdx.x) % (unsigned)fields);
}

__global__ __launch_bounds__(kThreads) void fourier_elu_fwd_kernel(const float* __restrict__ x, const float* __restrict__ scale,
                                                                   const float* __restrict__ shift, float* __restrict__ y,
                                                                   size_t items, int fields) {
  __shared__ __attribute__((aligned(16))) float tile[kTileFloats];
  const size_t n = items * kFieldDim;
  const size_t base = (size_t)blockIdx.x * kTileFloats;
  tile_load(x, tile, base, n);
  __syncthreads();
  const size_t item = (size_t)blockIdx.x * kThreads + threadIdx.x;
  float* row = tile + threadIdx.x * kFieldDim;
  if (item < items) {
    float sc[5], u[kFieldDim], s[kSamples], v[kFieldDim];
    field_affine(row, scale, shift, field_of_item(fields), sc, u);
    sample_all(u, s);
#pragma unroll
    for (int i = 0; i < kSamples; ++i) s[i] = s[i] > 0.0f ? s[i] : expm1f(s[i]);
    project_all(s, v);
#pragma unroll
    for (int j = 0; j < kFieldDim; ++j) row[j] = v[j] * (1.0f / kSamples);
  }
  __syncthreads();
  tile_store(y, tile, base, n);
}

__global__ __launch_bounds__(kThreads) void fourier_elu_bwd_kernel(const float* __restrict__ x, const float* __restrict__ scale,
                                                                   const float* __restrict__ shift, const float* __restrict__ dy,
                                                                   float* __restrict__ dx, size_t items, int fields) {
  __shared__ __attribute__((aligned(16))) float tile_x[kTileFloats];
  __shared__ __attribute__((aligned(16))) float tile_g[kTileFloats];
  const size_t n = items * kFieldDim;
  const size_t base = (size_t)blockIdx.x * kTileFloats;
  tile_load(x, tile_x, base, n);
  tile_load(dy, tile_g, base, n);
  __syncthreads();
  const size_t item = (size_t)blockIdx.x * kThreads + threadIdx.x;
  float* grow = tile_g + threadIdx.x * kFieldDim;
  if (item < items) {
    float sc[5], u[kFieldDim], s[kSamples], g[kFieldDim], gs[kSamples], du[kFieldDim];
    field_affine(tile_x + threadIdx.x * kFieldDim, scale, shift, field_of_item(fields), sc, u);
    sample_all(u, s);
#pragma unroll
    for (int j = 0; j < kFieldDim; ++j) g[j] = grow[j] * (1.0f / kSamples);
    sample_all(g, gs);                                   // A dy / 16: the gradient at the 16 samples
#pragma unroll
    for (int i = 0; i < kSamples; ++i) gs[i] = s[i] > 0.0f ? gs[i] : gs[i] * expf(s[i]);
    project_all(gs, du);
    grow[0] = du[0] * sc[0];
#pragma unroll
    for (int j = 1; j < kFieldDim; ++j) grow[j] = du[j] * sc[(j + 1) / 2];
  }
  __syncthreads();
  tile_store(dx, tile_g, base, n);
}

// items = npix * fields <= 2^31 - 1 blocks of 256: far beyond any map that fits the device
int check_args(const void* a, const void* b, long long npix, int fields, size_t* items, unsigned* blocks) {
  if (!a || !b || npix <= 0 || fields <= 0) return EQA_ERR_INVALID_ARG;
  if (npix > (long long)(0x7fffffffffffLL / kFieldDim / fields)) return EQA_ERR_UNSUPPORTED;
  *items = (size_t)npix * (size_t)fields;
  const size_t nb = (*items + kThreads - 1) / kThreads;
  if (nb > 0x7fffffffULL) return EQA_ERR_UNSUPPORTED;
  *blocks = (unsigned)nb;
  return EQA_OK;
}

}  // namespace

int eqa_fourier_elu_fwd(const float* x, const float* scale, const float* shift, float* y, long long npix, int fields, void* stream) {
  size_t items;
  unsigned blocks;
  const int st = check_args(x, y, npix, fields, &items, &blocks);
  if (st != EQA_OK) return st;
  if (((uintptr_t)x | (uintptr_t)y) & 15) return EQA_ERR_UNSUPPORTED;
  hipLaunchKernelGGL(fourier_elu_fwd_kernel, dim3(blocks), dim3(kThreads), 0, (hipStream_t)stream, x, scale, shift, y, items, fields);
  return launch_status();
}

int eqa_fourier_elu_bwd(const float* x, const float* scale, const float* shift, const float* dy, float* dx, long long npix, int fields,
                        void* stream) {
  size_t items;
  unsigned blocks;
  const int st = check_args(x, dx, npix, fields, &items, &blocks);
  if (st != EQA_OK) return st;
  if (!dy) return EQA_ERR_INVALID_ARG;
  if (((uintptr_t)x | (uintptr_t)dy | (uintptr_t)dx) & 15) return EQA_ERR_UNSUPPORTED;
  hipLaunchKernelGGL(fourier_elu_bwd_kernel, dim3(blocks), dim3(kThreads), 0, (hipStream_t)stream, x, scale, shift, dy, dx, items, fields);
  return launch_status();
}
