// Shared by the translation units that hold FFT-48 kernels (fftconv.hip, fft_filter.hip, lift_fft.hip): the tile / spectrum
// constants, the index of a stored frequency, the pitched buffer rule, the generated 48-point transforms and, at the end, what the
// two units of the FFT convolution agree on.  Include INSIDE the unit's anonymous namespace.
#pragma once

constexpr int kFftN = 48, kFftH = 25, kFftO = 44;
#include "fft48.inc"

// Stored frequencies.  A real tile's spectrum is Hermitian: X[-ky][-kx] = conj(X[ky][kx]).  Keeping kx = 0..24 uses that for
// 0 < kx < 24; in the columns kx = 0 and kx = 24 (their own mirror images) the rows ky = 25..47 are the conjugates of rows
// 23..1 and are not stored either: 48 x 23 + 2 x 25 = 1154 frequencies instead of 1200 (the GEMM runs per frequency).
// Index: f = ky * 23 + (kx - 1) for 0 < kx < 24, then 1104 + 2 ky + (kx == 24) for the two edge columns, ky <= 24.
constexpr int kFftInner = kFftH - 2;
constexpr int kFftF = kFftN * kFftInner + 2 * kFftH;
__device__ __forceinline__ bool fft_edge(int kx) { return kx == 0 || kx == kFftH - 1; }
__device__ __forceinline__ int fft_f0(int kx) { return kx == 0 ? kFftN * kFftInner : (kx == kFftH - 1 ? kFftN * kFftInner + 1 : kx - 1); }
__device__ __forceinline__ int fft_fstep(int kx) { return fft_edge(kx) ? 2 : kFftInner; }
__device__ __forceinline__ int fft_nky(int kx) { return fft_edge(kx) ? kFftH : kFftN; }

// Rows per stored frequency of V, Mo, G and the gradient products: the tile count made odd.  With M = 1024 tiles of 256
// channels a frequency is exactly 2 MB apart from the next, and the 1154 128-byte pieces a block gathers all fall into the
// same HBM channel / bank group: one row of padding takes the fused inverse from 1.23 to 1.01 ms.
__host__ __device__ inline size_t fft_pitch(size_t M) { return M | 1; }


// ---- fftconv.hip (transforms) and fft_filter.hip (filter spectra / gradients) ----------------------------------------------------
// A block of a fused transform owns one tile x kFusCh channels, in both directions.  Its row spectra (forward) or column
// transforms (inverse) pass through LDS as 25 kx slabs of 48 rows x [Re x 16 | Im x 16].
constexpr int kFusCh = 16;
constexpr int kFusKxPitch = kFftN * 2 * kFusCh + kFusCh;          // floats per kx slab (+16: slabs start 16 banks apart)
constexpr int kFusLds = kFftH * kFusKxPitch;                      // 38,800 floats
constexpr int kFusLdsBytes = kFusLds * (int)sizeof(float);        // 155,200 bytes
// channels per [Re | Im] group in the rows of V (and of the filter spectra that multiply them)
inline int fft_group_in(int C) { return C % kFusCh == 0 ? kFusCh : 1; }

// Kernel sizes: k x k filters give O = 49 - k outputs per 48 x 48 tile.  EQA_FFT_K(ksize, Plan, expr) returns `expr` with
// K_ = Plan<ksize>.
inline bool fft_ksize_ok(int k) { return k == 3 || k == 5 || k == 7 || k == 9; }
inline int fft_ntiles(int n, int O) { return (n + O - 1) / O; }                                  // tiles of O outputs that cover n
inline int fft_tiles_k(int n, int k) { return n < k ? 0 : fft_ntiles(n - (k - 1), kFftN + 1 - k); }   // ... that cover an INPUT extent n
#define EQA_FFT_K(ksize, Plan, expr)             \
  switch (ksize) {                               \
    case 3: { using K_ = Plan<3>; return expr; } \
    case 5: { using K_ = Plan<5>; return expr; } \
    case 7: { using K_ = Plan<7>; return expr; } \
    case 9: { using K_ = Plan<9>; return expr; } \
    default: return EQA_ERR_UNSUPPORTED;         \
  }
