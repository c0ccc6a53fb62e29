// The field norm of ESCNNSteerableNetwork in training mode, around the FourierELU kernels of fourier_act.hip (layout and field
// arithmetic: fourier_field.hpp).  Per field the norm is batch norm on a_0 and a division of c_m by its root mean square:
//   u = scale (.) x + shift,  scale = weight (.) rsqrt(var + eps),  shift = bias - mean scale_0,
//   var_0 = E[a_0^2] - mean^2,  var_m = E[(Re^2 + Im^2) / 2].
// Forward: eqa_field_norm_stats gives the six sums per field behind (mean, var); eqa_fourier_elu_fwd then applies scale and shift.
// Backward, with du = A^T [ELU'(A u) (.) (A dy / 16)] the gradient at u (what eqa_fourier_elu_bwd forms before its last multiply):
//   eqa_field_norm_elu_bwd_reduce   S_0 = sum du_0,  S_1 = sum du_0 a_0,  T_m = sum (du_Re Re + du_Im Im) of frequency m
//   eqa_field_norm_elu_bwd_apply    dx_0 = scale_0 du_0 - k_0 - c_1 (a_0 - mean),  dx_j = scale_m du_j - c_{1+m} x_j
// with (k_0, mean, c_1..c_5) per field made from those sums by the caller.  The apply pass forms du again from x and dy: no map
// besides x and dy is read, none besides dx written.
//
// Walk.  An item is one (pixel, field); a tile is S consecutive items, S the largest multiple of lcm(fields, 4) that is <= 256, so
// that item i of every tile belongs to field i % fields and every tile starts on a 16-byte line.  A block owns T consecutive
// tiles; thread i < S keeps item i of each of them, hence ONE field: its six fp64 sums stay in registers for the whole walk.
// (Threads >= S idle: none for a power of two, 16 of 256 for 5 fields, 72 for 23, the worst count up to 32.)  The next tile's
// lines are loaded into registers before the current tile is worked on and put into LDS after it.
// Sums.  Every fp32 term (both fp32 factors of a product) is converted to fp64 first, and all adds are fp64: products are exact,
// the sums are sums of exact terms.  At the end a block adds the threads of each field through LDS in thread order and writes one
// row of `partial`; the caller adds the rows.  No atomics: two launches on the same input give the same bits.
#include "fourier_field.hpp"

namespace {

constexpr int kMaxFields = 64;                                  // lcm(fields, 4) <= 256 for every fields <= 64, not for 65
constexpr int kSums = 6;
constexpr int kPre = (kTileVec + kThreads - 1) / kThreads;      // 16-byte lines per thread and tile
constexpr int kMinTiles = 8, kMaxTiles = 64;                    // tiles per block
constexpr long long kAimBlocks = 4096;

struct Walk {
  int S, T;
  size_t items;
  unsigned blocks;
};

// T grows with the map from 8 to 64 tiles (16384 items) per block, aiming at 4096 blocks: `partial` (48 bytes per block and field)
// stays below 1/200 of the map (36 bytes per item) even at T = 8, S = 240, and small maps still spread over the device
int plan(long long npix, int fields, Walk* w) {
  if (fields > kMaxFields) return EQA_ERR_UNSUPPORTED;
  if (npix <= 0 || fields <= 0) return EQA_ERR_INVALID_ARG;
  if (npix > (long long)(0x7fffffffffffLL / kFieldDim / fields)) return EQA_ERR_UNSUPPORTED;
  int lcm = fields;
  while (lcm % 4) lcm += fields;
  w->S = kThreads / lcm * lcm;
  w->items = (size_t)npix * (size_t)fields;
  const long long tiles = (long long)((w->items + w->S - 1) / w->S);
  const long long want = (tiles + kAimBlocks - 1) / kAimBlocks;
  w->T = (int)std::min<long long>(std::max<long long>(want, kMinTiles), kMaxTiles);
  const long long nb = (tiles + w->T - 1) / w->T;
  if (nb > 0x7fffffffLL) return EQA_ERR_UNSUPPORTED;
  w->blocks = (unsigned)nb;
  return EQA_OK;
}

// the first nvec 16-byte lines of the tile at float offset `base` -> registers (zeros past the end of the map), and on to LDS
__device__ __forceinline__ void tile_fetch(const float* __restrict__ g, float4 (&pre)[kPre], size_t base, size_t n, int nvec) {
#pragma unroll
  for (int k = 0; k < kPre; ++k) {
    const int v = threadIdx.x + k * kThreads;
    const size_t at = base + (size_t)v * 4;
    float4 q = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
    if (v < nvec) {
      if (at + 4 <= n) {
        q = *reinterpret_cast<const float4*>(g + at);
      } else {
        if (at + 0 < n) q.x = g[at + 0];
        if (at + 1 < n) q.y = g[at + 1];
        if (at + 2 < n) q.z = g[at + 2];
      }
    }
    pre[k] = q;
  }
}
__device__ __forceinline__ void tile_put(float* lds, const float4 (&pre)[kPre], int nvec) {
#pragma unroll
  for (int k = 0; k < kPre; ++k) {
    const int v = threadIdx.x + k * kThreads;
    if (v < nvec) *reinterpret_cast<float4*>(lds + v * 4) = pre[k];
  }
}

// The block's tiles of one map (a -> lds_a) or two (b -> lds_b as well), one after the other.  body(first): first = the tile's first
// item; the tile is in LDS, all threads call it, and it may write the tile (a barrier follows it).
template <int MAPS, typename Body>
__device__ __forceinline__ void walk_tiles(const float* __restrict__ a, const float* __restrict__ b, float* lds_a, float* lds_b,
                                           size_t items, int S, int T, Body&& body) {
  const size_t n = items * kFieldDim;
  const int nvec = S * kFieldDim / 4;
  const size_t tile0 = (size_t)blockIdx.x * T;
  float4 pre_a[kPre], pre_b[kPre];
  tile_fetch(a, pre_a, tile0 * S * kFieldDim, n, nvec);
  if constexpr (MAPS == 2) tile_fetch(b, pre_b, tile0 * S * kFieldDim, n, nvec);
  for (int t = 0; t < T; ++t) {
    const size_t first = (tile0 + t) * S;
    if (first >= items) break;                                   // uniform over the block
    tile_put(lds_a, pre_a, nvec);
    if constexpr (MAPS == 2) tile_put(lds_b, pre_b, nvec);
    __syncthreads();
    if (t + 1 < T) {                                             // (a tile past the end of the map: no load is issued)
      tile_fetch(a, pre_a, (first + S) * kFieldDim, n, nvec);
      if constexpr (MAPS == 2) tile_fetch(b, pre_b, (first + S) * kFieldDim, n, nvec);
    }
    body(first);
    __syncthreads();
  }
}

// acc of the threads i, i + fields, i + 2 fields, ... < S, added in that order -> row blockIdx.x of partial:(blocks, fields, 6)
__device__ __forceinline__ void write_partial(const double (&acc)[kSums], double* red, double* __restrict__ partial, int fields, int S) {
#pragma unroll
  for (int q = 0; q < kSums; ++q) red[threadIdx.x * kSums + q] = acc[q];
  __syncthreads();
  for (int o = threadIdx.x; o < fields * kSums; o += kThreads) {
    const int f = o / kSums, q = o - f * kSums;
    double sum = 0.0;
    for (int i = f; i < S; i += fields) sum += red[i * kSums + q];
    partial[(size_t)blockIdx.x * fields * kSums + o] = sum;
  }
}

__global__ __launch_bounds__(kThreads) void field_norm_stats_kernel(const float* __restrict__ x, double* __restrict__ partial,
                                                                    size_t items, int fields, int S, int T) {
  __shared__ __attribute__((aligned(16))) float tile[kTileFloats];
  __shared__ double red[kThreads * kSums];
  double acc[kSums] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
  const float* row = tile + threadIdx.x * kFieldDim;
  walk_tiles<1>(x, nullptr, tile, nullptr, items, S, T, [&](size_t first) {
    if ((int)threadIdx.x < S && first + threadIdx.x < items) {
      const double a0 = (double)row[0];
      acc[0] += a0;
      acc[1] += a0 * a0;
#pragma unroll
      for (int m = 1; m <= 4; ++m) {
        const double re = (double)row[2 * m - 1], im = (double)row[2 * m];
        acc[1 + m] += re * re + im * im;
      }
    }
  });
  write_partial(acc, red, partial, fields, S);
}

__global__ __launch_bounds__(kThreads) void field_norm_elu_bwd_reduce_kernel(const float* __restrict__ x, const float* __restrict__ scale,
                                                                             const float* __restrict__ shift,
                                                                             const float* __restrict__ dy, double* __restrict__ partial,
                                                                             size_t items, int fields, int S, int T) {
  __shared__ __attribute__((aligned(16))) float tile_x[kTileFloats];
  __shared__ __attribute__((aligned(16))) float tile_g[kTileFloats];
  __shared__ double red[kThreads * kSums];
  double acc[kSums] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
  float sc[5], sh;
  field_table(scale, shift, (int)(threadIdx.x % (unsigned)fields), sc, sh);
  const float* xrow = tile_x + threadIdx.x * kFieldDim;
  const float* grow = tile_g + threadIdx.x * kFieldDim;
  walk_tiles<2>(x, dy, tile_x, tile_g, items, S, T, [&](size_t first) {
    if ((int)threadIdx.x < S && first + threadIdx.x < items) {
      float u[kFieldDim], du[kFieldDim];
      field_affine(xrow, sc, sh, u);
      field_elu_grad(u, grow, du);
      acc[0] += (double)du[0];
      acc[1] += (double)du[0] * (double)xrow[0];
#pragma unroll
      for (int m = 1; m <= 4; ++m)
        acc[1 + m] += (double)du[2 * m - 1] * (double)xrow[2 * m - 1] + (double)du[2 * m] * (double)xrow[2 * m];
    }
  });
  write_partial(acc, red, partial, fields, S);
}

__global__ __launch_bounds__(kThreads) void field_norm_elu_bwd_apply_kernel(const float* __restrict__ x, const float* __restrict__ scale,
                                                                            const float* __restrict__ shift, const float* __restrict__ dy,
                                                                            const float* __restrict__ coef, float* __restrict__ dx,
                                                                            size_t items, int fields, int S, int T) {
  __shared__ __attribute__((aligned(16))) float tile_x[kTileFloats];
  __shared__ __attribute__((aligned(16))) float tile_g[kTileFloats];
  const int field = (int)(threadIdx.x % (unsigned)fields);
  float sc[5], sh, c[5];
  field_table(scale, shift, field, sc, sh);
  const float k0 = coef[field * 7], mean = coef[field * 7 + 1];
#pragma unroll
  for (int m = 0; m < 5; ++m) c[m] = coef[field * 7 + 2 + m];
  const float* xrow = tile_x + threadIdx.x * kFieldDim;
  float* grow = tile_g + threadIdx.x * kFieldDim;
  const size_t n = items * kFieldDim;
  const int nvec = S * kFieldDim / 4;
  walk_tiles<2>(x, dy, tile_x, tile_g, items, S, T, [&](size_t first) {
    if ((int)threadIdx.x < S && first + threadIdx.x < items) {
      float u[kFieldDim], du[kFieldDim];
      field_affine(xrow, sc, sh, u);
      field_elu_grad(u, grow, du);
      grow[0] = sc[0] * du[0] - k0 - c[0] * (xrow[0] - mean);     // a_0 - mean first: a large mean costs no accuracy
#pragma unroll
      for (int j = 1; j < kFieldDim; ++j) grow[j] = sc[(j + 1) / 2] * du[j] - c[(j + 1) / 2] * xrow[j];
    }
    __syncthreads();
    tile_store(dx, tile_g, first * kFieldDim, n, nvec);
  });
}

// the maps a, b, c on 16-byte lines, the table (partial: fp64, coef: fp32) on its element size
int check_args(const void* a, const void* b, const void* c, const void* table, int table_align) {
  if (!a || !b || !c || !table) return EQA_ERR_INVALID_ARG;
  if (((uintptr_t)a | (uintptr_t)b | (uintptr_t)c) & 15) return EQA_ERR_UNSUPPORTED;
  if ((uintptr_t)table & (uintptr_t)(table_align - 1)) return EQA_ERR_UNSUPPORTED;
  return EQA_OK;
}

}  // namespace

int eqa_field_norm_max_fields(void) { return kMaxFields; }

long long eqa_field_norm_blocks(long long npix, int fields) {
  Walk w;
  const int st = plan(npix, fields, &w);
  return st == EQA_OK ? (long long)w.blocks : (long long)st;
}

int eqa_field_norm_stats(const float* x, double* partial, long long npix, int fields, void* stream) {
  Walk w;
  int st = plan(npix, fields, &w);
  if (st == EQA_OK) st = check_args(x, x, x, partial, 8);
  if (st != EQA_OK) return st;
  hipLaunchKernelGGL(field_norm_stats_kernel, dim3(w.blocks), dim3(kThreads), 0, (hipStream_t)stream, x, partial, w.items, fields, w.S,
                     w.T);
  return launch_status();
}

int eqa_field_norm_elu_bwd_reduce(const float* x, const float* scale, const float* shift, const float* dy, double* partial,
                                  long long npix, int fields, void* stream) {
  Walk w;
  int st = plan(npix, fields, &w);
  if (st == EQA_OK) st = check_args(x, dy, dy, partial, 8);
  if (st != EQA_OK) return st;
  hipLaunchKernelGGL(field_norm_elu_bwd_reduce_kernel, dim3(w.blocks), dim3(kThreads), 0, (hipStream_t)stream, x, scale, shift, dy,
                     partial, w.items, fields, w.S, w.T);
  return launch_status();
}

int eqa_field_norm_elu_bwd_apply(const float* x, const float* scale, const float* shift, const float* dy, const float* coef, float* dx,
                                 long long npix, int fields, void* stream) {
  Walk w;
  int st = plan(npix, fields, &w);
  if (st == EQA_OK) st = check_args(x, dy, dx, coef, 4);
  if (st != EQA_OK) return st;
  hipLaunchKernelGGL(field_norm_elu_bwd_apply_kernel, dim3(w.blocks), dim3(kThreads), 0, (hipStream_t)stream, x, scale, shift, dy, coef,
                     dx, w.items, fields, w.S, w.T);
  return launch_status();
}
