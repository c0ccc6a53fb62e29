// FourierELU over band-limited SO(2) fields (ESCNNSteerableNetwork's hidden activation), fused with the field norm's eval-mode
// affine map.  A field is 9 consecutive fp32 of a channels-last map: a_0, then (Re c_m, Im c_m) for m = 1..4; it describes
//   f(phi) = a_0 + sum_m sqrt(2) (Re c_m cos(m phi) + Im c_m sin(m phi)).
// Forward, per (pixel, field):  u = scale (.) x + shift (a_0 only),  s_i = f_u(2 pi i / 16) for i = 0..15,  y = A^T ELU(s) / 16, where
// A is the 16 x 9 sampling matrix above (A^T A = 16 I).  Backward: dx = scale (.) A^T [ELU'(s) (.) (A dy / 16)], s recomputed from x.
//
// One thread per (pixel, field).  The 36-byte rows of a block's 256 fields are 9216 contiguous bytes: the block moves them between
// global memory and LDS as whole 16-byte lines, and a thread reads / writes its nine values in LDS at a stride of 9 dwords (odd: no
// bank conflicts).  The field arithmetic and the tile moves are in fourier_field.hpp, shared with field_norm.hip.  No atomics: the
// result does not depend on the launch.
#include "fourier_field.hpp"

namespace {

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
    float sc[5], u[kFieldDim], du[kFieldDim];
    field_affine(tile_x + threadIdx.x * kFieldDim, scale, shift, field_of_item(fields), sc, u);
    field_elu_grad(u, grow, du);
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
