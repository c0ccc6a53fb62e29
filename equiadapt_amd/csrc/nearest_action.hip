// libeqa_hip.so, part 7 of 7 -- the nearest-neighbour group action on masks and images (I6, GroupInference) and the action on
// bounding boxes.  C ABI: include/eqa_hip.h.
#include "eqa_common.hpp"

namespace {

// ablation switch for tools/ablate.sh (never set in the product build)
#ifndef EQA_ABL_MASKGUARD
#define EQA_ABL_MASKGUARD 0     // -DEQA_ABL_MASKGUARD=1: the guard ring of mask_action_u8_kernel's staged box (rounds 1-3)
#endif

// ------------------------------------------------------------------------------------------------
// I6: nearest-neighbour action on uint8 masks (torchvision.transforms.functional.rotate defaults on a uint8 tensor:
// half-pixel base grid, theta rescaled by (0.5 W, 0.5 H), grid_sample(nearest, zeros, align_corners=False), round;
// images/utils.py:125-136, optionally after flip_masks :112-122).  rtheta[e] = the RESCALED 3x2 matrix in the order
// (r00, r10, r20, r01, r11, r21): gx = xb*r00 + yb*r10 + r20, gy = xb*r01 + yb*r11 + r21.
// One thread = 4 consecutive output pixels (one 32-bit store).
// ------------------------------------------------------------------------------------------------
// Generic form (T = uint8 masks or fp32 images): output plane p of (n_planes) samples source plane p % src_mod with
// element eidx[p]; the sampling frame is the source plane edge-padded by `pad`, the output the (OH,OW) window at
// (top,left) of the frame -- GroupInference's pad(0.4 H) -> [hflip] -> rotate(+deg) -> CenterCrop on float images
// (examples/images/classification/inference_utils.py:100-123: torchvision rotate defaults to NEAREST) uses all of it.
template <typename T>
struct Pack4;
template <>
struct Pack4<uint8_t> {
  typedef uint32_t type;
  static __device__ __forceinline__ type make(const uint8_t (&v)[4]) {
    return (uint32_t)v[0] | ((uint32_t)v[1] << 8) | ((uint32_t)v[2] << 16) | ((uint32_t)v[3] << 24);
  }
};
template <>
struct Pack4<float> {
  typedef float4 type;
  static __device__ __forceinline__ type make(const float (&v)[4]) { return make_float4(v[0], v[1], v[2], v[3]); }
};

// The sampling frame of one plane: the rescaled matrix of its element and the (OH, OW) window at (top, left) of the (Hp, Wp) frame.
struct NearestFrame {
  float t0, t1, t2, t3, t4, t5;
  int top, left, Hp, Wp;
};
// The sample point of output pixel (i, j), in frame pixels, before rounding.  One copy for the three kernels below, which must
// agree bit for bit.  No `fp contract` pragma here: which of these multiply-adds are fused is left to the compiler, as it always
// was, and the bit-exact mask tests pin the outcome.
__device__ __forceinline__ void nearest_raw_xy(const NearestFrame& f, const int i, const int j, float& fx, float& fy) {
  const float yb = ((float)(f.top + i) + 0.5f) - 0.5f * (float)f.Hp;
  const float xb = ((float)(f.left + j) + 0.5f) - 0.5f * (float)f.Wp;
  const float gx = xb * f.t0 + yb * f.t1 + f.t2;
  const float gy = xb * f.t3 + yb * f.t4 + f.t5;
  fx = ((gx + 1.0f) * (float)f.Wp - 1.0f) / 2.0f;
  fy = ((gy + 1.0f) * (float)f.Hp - 1.0f) / 2.0f;
}
// ... and the frame pixel it rounds to (std::nearbyint: round half to even)
__device__ __forceinline__ void nearest_source_xy(const NearestFrame& f, const int i, const int j, float& xr, float& yr) {
  float fx, fy;
  nearest_raw_xy(f, i, j, fx, fy);
  xr = rintf(fx);
  yr = rintf(fy);
}
// Source box of the output tile [i0, i1] x [j0, j1], in frame pixels clamped to the frame and mirrored for a pre-flipped source:
// the map is affine before rounding and the rounded coordinate monotone along rows and columns, so the four corners bound it
// exactly.  (No guard ring: a pixel that landed outside the box all the same is read from global memory.)
__device__ __forceinline__ void nearest_corner_box(const NearestFrame& f, const bool flip, const int i0, const int j0, const int i1,
                                                   const int j1, int& fx0, int& fx1, int& fy0, int& fy1) {
  float xa, ya, xb_, yb_, xc, yc, xd, yd;
  nearest_source_xy(f, i0, j0, xa, ya); nearest_source_xy(f, i0, j1, xb_, yb_);
  nearest_source_xy(f, i1, j0, xc, yc); nearest_source_xy(f, i1, j1, xd, yd);
  fx0 = (int)fminf(fminf(xa, xb_), fminf(xc, xd)) - EQA_ABL_MASKGUARD; fx1 = (int)fmaxf(fmaxf(xa, xb_), fmaxf(xc, xd)) + EQA_ABL_MASKGUARD;
  fy0 = (int)fminf(fminf(ya, yb_), fminf(yc, yd)) - EQA_ABL_MASKGUARD; fy1 = (int)fmaxf(fmaxf(ya, yb_), fmaxf(yc, yd)) + EQA_ABL_MASKGUARD;
  fx0 = max(fx0, 0); fx1 = min(fx1, f.Wp - 1); fy0 = max(fy0, 0); fy1 = min(fy1, f.Hp - 1);
  if (flip) { const int a = f.Wp - 1 - fx1, b = f.Wp - 1 - fx0; fx0 = a; fx1 = b; }
}

template <typename T>
__global__ __launch_bounds__(kThreads) void nearest_action_kernel(const T* __restrict__ m, T* __restrict__ out,
                                                                 const int32_t* __restrict__ eidx,
                                                                 const float* __restrict__ rtheta,
                                                                 const int32_t* __restrict__ flags, int E, int H, int W,
                                                                 int pad, int OH, int OW, int top, int left, int src_mod) {
  const int p = blockIdx.z;
  const int i = blockIdx.y;
  const int jb = (blockIdx.x * kThreads + threadIdx.x) * 4;
  if (jb >= OW) return;
  const int Hp = H + 2 * pad, Wp = W + 2 * pad;
  const int e = min(max(eidx[p], 0), E - 1);
  const float* t = rtheta + e * 6;
  const NearestFrame f = {t[0], t[1], t[2], t[3], t[4], t[5], top, left, Hp, Wp};
  const bool flip = flags && (flags[e] & EQA_FLIP_SRC);
  const T* src = m + (size_t)(src_mod > 0 ? p % src_mod : p) * H * W;
  T v[4];
#pragma unroll
  for (int k = 0; k < 4; ++k) {
    float xr, yr;
    nearest_source_xy(f, i, jb + k, xr, yr);
    T val = (T)0;
    if (xr >= 0.0f && xr <= (float)(Wp - 1) && yr >= 0.0f && yr <= (float)(Hp - 1)) {
      const int fx = flip ? (Wp - 1 - (int)xr) : (int)xr;
      const int sx = min(max(fx - pad, 0), W - 1), sy = min(max((int)yr - pad, 0), H - 1);
      val = src[(size_t)sy * W + sx];
    }
    v[k] = val;
  }
  T* o = out + (size_t)p * OH * OW + (size_t)i * OW + jb;
  typedef typename Pack4<T>::type P4;
  if (jb + 3 < OW && ((((uintptr_t)o) & (sizeof(P4) - 1)) == 0)) {
    *reinterpret_cast<P4*>(o) = Pack4<T>::make(v);
  } else {
#pragma unroll
    for (int k = 0; k < 4; ++k)
      if (jb + k < OW) o[k] = v[k];
  }
}

// Tiled form of the kernel above: one block = a 64 x 64 output tile whose source bounding box (the tile corners' images,
// one pixel of rounding slack) is first staged into LDS row by row, so that the 90-degree elements of C4 / D4 -- whose
// output rows are source COLUMNS -- no longer touch one cache line per pixel (config 5: 96 uint8 masks of 1024^2 took
// 0.50 ms, 12x their HBM time, in the row-per-block kernel).  Same arithmetic per pixel, bit-identical results; a pixel
// whose source falls outside the staged box (never for rotations) is read from global memory.
constexpr int kNearTile = 64, kNearBox = 96;

template <typename T>
__global__ __launch_bounds__(kThreads) void nearest_action_tile_kernel(const T* __restrict__ m, T* __restrict__ out,
                                                                      const int32_t* __restrict__ eidx,
                                                                      const float* __restrict__ rtheta,
                                                                      const int32_t* __restrict__ flags, int E, int H, int W,
                                                                      int pad, int OH, int OW, int top, int left, int src_mod) {
  __shared__ T s_src[kNearBox * kNearBox];
  const int p = blockIdx.z;
  const int i0 = blockIdx.y * kNearTile, j0 = blockIdx.x * kNearTile;
  const int Hp = H + 2 * pad, Wp = W + 2 * pad;
  const int e = min(max(eidx[p], 0), E - 1);
  const float* t = rtheta + e * 6;
  const NearestFrame f = {t[0], t[1], t[2], t[3], t[4], t[5], top, left, Hp, Wp};
  const bool flip = flags && (flags[e] & EQA_FLIP_SRC);
  const T* src = m + (size_t)(src_mod > 0 ? p % src_mod : p) * H * W;
  const int i1 = min(i0 + kNearTile, OH) - 1, j1 = min(j0 + kNearTile, OW) - 1;
  int fx0, fx1, fy0, fy1;
  nearest_corner_box(f, flip, i0, j0, i1, j1, fx0, fx1, fy0, fy1);
  const int sx0 = min(max(fx0 - pad, 0), W - 1), sx1 = min(max(fx1 - pad, 0), W - 1);
  const int sy0 = min(max(fy0 - pad, 0), H - 1), sy1 = min(max(fy1 - pad, 0), H - 1);
  const int bw = sx1 - sx0 + 1, bh = sy1 - sy0 + 1;
  const bool staged = bw > 0 && bh > 0 && bw <= kNearBox && bh <= kNearBox;  // block-uniform
  if (staged) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    for (int r = wave; r < bh; r += kThreads / 64) {
      const T* grow = src + (size_t)(sy0 + r) * W + sx0;
      for (int c = lane; c < bw; c += 64) s_src[r * kNearBox + c] = grow[c];
    }
  }
  __syncthreads();
  const int jb = j0 + (threadIdx.x & 15) * 4;
#pragma unroll
  for (int g = 0; g < 4; ++g) {
    const int i = i0 + (threadIdx.x >> 4) + 16 * g;
    if (i >= OH || jb >= OW) continue;
    T v[4];
#pragma unroll
    for (int k = 0; k < 4; ++k) {
      float xr, yr;
      nearest_source_xy(f, i, jb + k, xr, yr);
      T val = (T)0;
      if (xr >= 0.0f && xr <= (float)(Wp - 1) && yr >= 0.0f && yr <= (float)(Hp - 1)) {
        const int fx = flip ? (Wp - 1 - (int)xr) : (int)xr;
        const int sx = min(max(fx - pad, 0), W - 1), sy = min(max((int)yr - pad, 0), H - 1);
        const int lx = sx - sx0, ly = sy - sy0;
        val = (staged && (unsigned)lx < (unsigned)bw && (unsigned)ly < (unsigned)bh) ? s_src[ly * kNearBox + lx]
                                                                                     : src[(size_t)sy * W + sx];
      }
      v[k] = val;
    }
    T* o = out + (size_t)p * OH * OW + (size_t)i * OW + jb;
    typedef typename Pack4<T>::type P4;
    if (jb + 3 < OW && ((((uintptr_t)o) & (sizeof(P4) - 1)) == 0)) {
      *reinterpret_cast<P4*>(o) = Pack4<T>::make(v);
    } else {
#pragma unroll
      for (int k = 0; k < 4; ++k)
        if (jb + k < OW) o[k] = v[k];
    }
  }
}

// uint8 masks, the config-5 case (96 masks of 1024 x 1024 per step): the tiled kernel above staged its source box byte by
// byte (one 64-byte wave load per 64 pixels) and stored 4 bytes per lane -- 0.21 ms for 0.2 GB = 1 TB/s, bound by the number
// of memory instructions.  Same tile, same per-pixel arithmetic (bit-identical results), but the box is staged in whole dwords
// (rows start 4-byte aligned: W % 4 == 0) and a thread owns 16 consecutive pixels of one row = one 16-byte store.  The source
// planes come either from one contiguous tensor or from a table of per-plane pointers (the masks of a batch live in one
// tensor per sample: no concatenation pass in front of the kernel).
constexpr int kU8Pitch = 104;  // bytes per staged row: 96 + 3 (alignment slack), rounded to a dword multiple + 1 dword
__global__ __launch_bounds__(kThreads) void mask_action_u8_kernel(const uint8_t* __restrict__ m, const uint8_t* const* __restrict__ planes,
                                                                 uint8_t* __restrict__ out, const int32_t* __restrict__ eidx,
                                                                 const float* __restrict__ rtheta, const int32_t* __restrict__ flags, int E,
                                                                 int H, int W) {
  __shared__ __attribute__((aligned(16))) uint8_t s_src[kNearBox * kU8Pitch + 8];  // + 8: the fifth dword of a row run at the very end
  const int p = blockIdx.z;
  const int i0 = blockIdx.y * kNearTile, j0 = blockIdx.x * kNearTile;
  const int e = min(max(eidx[p], 0), E - 1);
  const float* t = rtheta + e * 6;
  const NearestFrame f = {t[0], t[1], t[2], t[3], t[4], t[5], 0, 0, H, W};   // the frame is the mask itself: pad = top = left = 0
  const bool flip = flags && (flags[e] & EQA_FLIP_SRC);
  const uint8_t* src = planes ? planes[p] : m + (size_t)p * H * W;
  const int i1 = min(i0 + kNearTile, H) - 1, j1 = min(j0 + kNearTile, W) - 1;
  // The box needs no guard ring for correctness (nearest_corner_box).  With one (rounds 1-3) the staged rows of an axis-aligned
  // element were 66 bytes starting one byte in front of the tile's 64: two 128-byte lines per row instead of one.
  int fx0, fx1, fy0, fy1;
  nearest_corner_box(f, flip, i0, j0, i1, j1, fx0, fx1, fy0, fy1);
  const int sx0 = fx0 & ~3, sx1 = fx1;               // dword-aligned left edge
  const int sy0 = fy0, sy1 = fy1;
  const int bw = sx1 - sx0 + 1, bh = sy1 - sy0 + 1;
  const bool staged = bw > 0 && bh > 0 && bw <= kU8Pitch - 4 && bh <= kNearBox;  // block-uniform
  // Axis-aligned elements on aligned tiles (every element of C4 / D4 on the 1024 x 1024 masks of config 5): the box is 64 rows of 64
  // bytes starting on a 16-byte boundary -- ONE 16-byte load and two 8-byte LDS stores per thread instead of twelve predicated
  // dword passes (a third of whose lanes and passes carry data): the staging was half of the kernel's instructions.
  const bool staged16 = staged && bw <= 64 && bh <= 64 && (sx0 & 15) == 0 && (W & 15) == 0 && sx0 + 64 <= W &&
                        (reinterpret_cast<uintptr_t>(src) & 15) == 0;   // block-uniform
  if (staged16) {
    const int r = threadIdx.x >> 2, q = threadIdx.x & 3;
    if (r < bh) {
      const uint4 v = *reinterpret_cast<const uint4*>(src + (size_t)(sy0 + r) * W + sx0 + 16 * q);
      uint2* d = reinterpret_cast<uint2*>(s_src + r * kU8Pitch + 16 * q);
      d[0] = make_uint2(v.x, v.y);
      d[1] = make_uint2(v.z, v.w);
    }
  } else if (staged) {
    const int nd = (bw + 3) >> 2;                     // dwords per row (the last one may reach past sx1: still inside the row, W % 4 == 0)
    // 32 dword slots per row (nd <= 25), 8 rows per pass, all 12 passes' loads in flight before the first LDS store (a rolled
    // load -> store loop pays one HBM round trip per pass: 0.14 instead of 0.21 ms was all the dword staging bought that way)
    constexpr int kPasses = kNearBox * 32 / kThreads;
    const int d = threadIdx.x & 31, r0 = threadIdx.x >> 5;
    uint32_t w[kPasses];
#pragma unroll
    for (int k = 0; k < kPasses; ++k) {
      const int r = r0 + 8 * k;
      const bool on = d < nd && r < bh;
      const uint32_t v = *reinterpret_cast<const uint32_t*>(src + (size_t)(sy0 + (on ? r : 0)) * W + sx0 + 4 * (on ? d : 0));
      w[k] = v;
    }
#pragma unroll
    for (int k = 0; k < kPasses; ++k) {
      const int r = r0 + 8 * k;
      if (d < nd && r < bh) *reinterpret_cast<uint32_t*>(s_src + r * kU8Pitch + 4 * d) = w[k];
    }
  }
  __syncthreads();
  const int i = i0 + (threadIdx.x >> 2);
  const int jb = j0 + (threadIdx.x & 3) * 16;
  if (i >= H || jb >= W) return;
  uint32_t w4[4] = {0u, 0u, 0u, 0u};
  // Axis-aligned elements (every element of C4 / D4: the config-5 case) move a run of 16 output pixels onto 16 consecutive
  // source pixels of one row or one column.  The run's two END pixels go through the reference's arithmetic; if they land 15
  // apart along one axis, on the same line of the other, both inside the frame and the staged box, and their unrounded
  // coordinates are within 0.25 of the integers they round to, then the 14 pixels between them round to the integers between
  // (the coordinate is affine in the pixel index up to ~1e-4 of fp32 noise at |x| <= 2^15: an interior pixel could only round
  // elsewhere from within that noise of a .5 tie, and a quarter pixel is far from it) -- bit-identical to evaluating all 16,
  // at 2 coordinate evaluations instead of 16 (the kernel was bound by its ~28 vector instructions per pixel: 1.9 TB/s).
  bool fast = false;
  if (staged && jb + 15 < W) {
    float fxa, fya, fxb, fyb;
    nearest_raw_xy(f, i, jb, fxa, fya);
    nearest_raw_xy(f, i, jb + 15, fxb, fyb);
    const float xra = rintf(fxa), yra = rintf(fya), xrb = rintf(fxb), yrb = rintf(fyb);
    const bool inside = fminf(xra, xrb) >= 0.0f && fmaxf(xra, xrb) <= (float)(W - 1) && fminf(yra, yrb) >= 0.0f && fmaxf(yra, yrb) <= (float)(H - 1);
    const bool snug = fabsf(fxa - xra) < 0.25f && fabsf(fya - yra) < 0.25f && fabsf(fxb - xrb) < 0.25f && fabsf(fyb - yrb) < 0.25f;
    const int sxa = flip ? (W - 1 - (int)xra) : (int)xra, sxb = flip ? (W - 1 - (int)xrb) : (int)xrb;
    const int sya = (int)yra, syb = (int)yrb;
    const int ddx = sxb - sxa, ddy = syb - sya;
    const bool line = (ddy == 0 && (ddx == 15 || ddx == -15)) || (ddx == 0 && (ddy == 15 || ddy == -15));
    const int lxa = sxa - sx0, lya = sya - sy0, lxb = sxb - sx0, lyb = syb - sy0;
    const bool boxed = (unsigned)lxa < (unsigned)bw && (unsigned)lya < (unsigned)bh && (unsigned)lxb < (unsigned)bw && (unsigned)lyb < (unsigned)bh;
    fast = inside && snug && line && boxed;
    if (fast) {
      if (ddy == 0) {
        // along a source row: the 16 bytes [lo, lo + 16) come out of 5 aligned dword reads and 4 funnel shifts; a run that walks
        // the row backwards (flips, 180 degrees) is the same bytes in reverse order
        const int lo = lya * kU8Pitch + min(lxa, lxb);
        const uint32_t* q = reinterpret_cast<const uint32_t*>(s_src + (lo & ~3));
        const uint32_t sh = (uint32_t)(lo & 3);
        const uint32_t d0 = q[0], d1 = q[1], d2 = q[2], d3 = q[3], d4 = q[4];
        const uint32_t f0 = __builtin_amdgcn_alignbyte(d1, d0, sh), f1 = __builtin_amdgcn_alignbyte(d2, d1, sh);
        const uint32_t f2 = __builtin_amdgcn_alignbyte(d3, d2, sh), f3 = __builtin_amdgcn_alignbyte(d4, d3, sh);
        const bool rev = ddx < 0;
        w4[0] = rev ? __builtin_bswap32(f3) : f0;
        w4[1] = rev ? __builtin_bswap32(f2) : f1;
        w4[2] = rev ? __builtin_bswap32(f1) : f2;
        w4[3] = rev ? __builtin_bswap32(f0) : f3;
      } else {
        const int stride = (ddy / 15) * kU8Pitch;
        const uint8_t* sp = s_src + lya * kU8Pitch + lxa;
#pragma unroll
        for (int k = 0; k < 16; ++k) w4[k >> 2] |= (uint32_t)sp[k * stride] << (8 * (k & 3));
      }
    }
  }
  if (!fast) {
#pragma unroll
    for (int k = 0; k < 16; ++k) {
      float xr, yr;
      nearest_source_xy(f, i, jb + k, xr, yr);
      uint32_t val = 0u;
      if (xr >= 0.0f && xr <= (float)(W - 1) && yr >= 0.0f && yr <= (float)(H - 1)) {
        const int sx = flip ? (W - 1 - (int)xr) : (int)xr, sy = (int)yr;
        const int lx = sx - sx0, ly = sy - sy0;
        val = (staged && (unsigned)lx < (unsigned)bw && (unsigned)ly < (unsigned)bh) ? s_src[ly * kU8Pitch + lx] : src[(size_t)sy * W + sx];
      }
      w4[k >> 2] |= val << (8 * (k & 3));
    }
  }
  uint8_t* o = out + (size_t)p * H * W + (size_t)i * W + jb;
  if (jb + 15 < W) {
    *reinterpret_cast<uint4*>(o) = make_uint4(w4[0], w4[1], w4[2], w4[3]);
  } else {
    for (int k = 0; k < 16; ++k)
      if (jb + k < W) o[k] = (uint8_t)(w4[k >> 2] >> (8 * (k & 3)));
  }
}

int launch_mask_u8(const uint8_t* m, const uint8_t* const* planes, uint8_t* out, const int32_t* eidx, const float* rtheta,
                   const int32_t* flags, int E, int n_planes, int H, int W, void* stream) {
  if ((!m && !planes) || !out || !eidx || !rtheta || E <= 0 || n_planes < 0 || H <= 0 || W <= 0) return EQA_ERR_INVALID_ARG;
  if (n_planes > 65535 || H > 65535 * kNearTile || (W & 15) || ((uintptr_t)out & 15) || ((uintptr_t)m & 3)) return EQA_ERR_UNSUPPORTED;
  if (n_planes == 0) return EQA_OK;
  hipLaunchKernelGGL(mask_action_u8_kernel, dim3((W + kNearTile - 1) / kNearTile, (H + kNearTile - 1) / kNearTile, n_planes), dim3(kThreads),
                     0, (hipStream_t)stream, m, planes, out, eidx, rtheta, flags, E, H, W);
  return hipGetLastError() == hipSuccess ? EQA_OK : EQA_ERR_LAUNCH;
}

template <typename T>
int launch_nearest(const T* m, T* out, const int32_t* eidx, const float* rtheta, const int32_t* flags, int E,
                          int n_planes, int H, int W, int pad, int OH, int OW, int top, int left, int src_mod, void* stream) {
  if (!m || !out || !eidx || !rtheta || E <= 0 || n_planes < 0 || H <= 0 || W <= 0 || pad < 0 || OH <= 0 || OW <= 0 ||
      top < 0 || left < 0 || top + OH > H + 2 * pad || left + OW > W + 2 * pad || src_mod < 0)
    return EQA_ERR_INVALID_ARG;
  if (n_planes > 65535 || OH > 65535) return EQA_ERR_UNSUPPORTED;
  if (n_planes == 0) return EQA_OK;
  if (g_force_direct)  // eqa_set_option(0, 1): the row-per-block kernel without LDS staging (tests compare the two)
    hipLaunchKernelGGL((nearest_action_kernel<T>), dim3((OW / 4 + kThreads) / kThreads, OH, n_planes), dim3(kThreads), 0,
                       (hipStream_t)stream, m, out, eidx, rtheta, flags, E, H, W, pad, OH, OW, top, left, src_mod);
  else
    hipLaunchKernelGGL((nearest_action_tile_kernel<T>),
                       dim3((OW + kNearTile - 1) / kNearTile, (OH + kNearTile - 1) / kNearTile, n_planes), dim3(kThreads), 0,
                       (hipStream_t)stream, m, out, eidx, rtheta, flags, E, H, W, pad, OH, OW, top, left, src_mod);
  return hipGetLastError() == hipSuccess ? EQA_OK : EQA_ERR_LAUNCH;
}

// ------------------------------------------------------------------------------------------------
// I6, boxes: flip_boxes (images/utils.py:97-109) + rotate_boxes (:161-187, rotate_points :139-158) for every box of the
// batch in one launch.  The reference does this per sample with a dozen element-wise launches each; the batched torch form
// still was ~55 launches of 1-2 us spaced ~10 us apart -- 0.6 of config 5's 1.9 ms step.  Same fp32 arithmetic in the same
// order, no fused multiply-adds: rad = deg * (pi/180); x' = ox + cos*(x-ox) - sin*(y-oy); y' = oy + sin*(x-ox) + cos*(y-oy)
// about (W/2, W/2); the box is then re-sorted corner-wise.
// ------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(kThreads) void boxes_action_kernel(const float* __restrict__ boxes, const int32_t* __restrict__ img_of_box,
                                                               const float* __restrict__ rotation_deg, float* __restrict__ flipped,
                                                               float* __restrict__ out, int n, float width, int flip_all) {
#pragma clang fp contract(off)
  const int i = blockIdx.x * kThreads + threadIdx.x;
  if (i >= n) return;
  float4 b = reinterpret_cast<const float4*>(boxes)[i];
  if (flip_all) {  // boxes[:, [0, 2]] = width - boxes[:, [2, 0]]
    const float x0 = width - b.z, x1 = width - b.x;
    b.x = x0;
    b.z = x1;
    if (flipped) reinterpret_cast<float4*>(flipped)[i] = b;
  }
  const float rad = rotation_deg[img_of_box[i]] * 0.017453292519943295f;  // torch.deg2rad
  const float c = cosf(rad), sn = sinf(rad);
  const float o = width / 2;
  const float x0 = o + c * (b.x - o) - sn * (b.y - o), y0 = o + sn * (b.x - o) + c * (b.y - o);
  const float x1 = o + c * (b.z - o) - sn * (b.w - o), y1 = o + sn * (b.z - o) + c * (b.w - o);
  reinterpret_cast<float4*>(out)[i] = make_float4(fminf(x0, x1), fminf(y0, y1), fmaxf(x0, x1), fmaxf(y0, y1));
}

}  // namespace

extern "C" {

int eqa_mask_action_nearest(const uint8_t* m, uint8_t* out, const int32_t* eidx, const float* rtheta, const int32_t* flags,
                            int num_elements, int n_masks, int H, int W, void* stream) {
  if (!g_force_direct && m && (W & 15) == 0 && (((uintptr_t)out & 15) | ((uintptr_t)m & 3)) == 0 && n_masks <= 65535)
    return launch_mask_u8(m, nullptr, out, eidx, rtheta, flags, num_elements, n_masks, H, W, stream);
  return launch_nearest<uint8_t>(m, out, eidx, rtheta, flags, num_elements, n_masks, H, W, 0, H, W, 0, 0, 0, stream);
}

int eqa_mask_action_nearest_planes(const uint8_t* const* planes, uint8_t* out, const int32_t* eidx, const float* rtheta,
                                   const int32_t* flags, int num_elements, int n_masks, int H, int W, void* stream) {
  return launch_mask_u8(nullptr, planes, out, eidx, rtheta, flags, num_elements, n_masks, H, W, stream);
}

int eqa_boxes_action(const float* boxes, const int32_t* img_of_box, const float* rotation_deg, float* flipped, float* out,
                     int n, float width, int flip_all, void* stream) {
  if (n == 0) return EQA_OK;
  if (!boxes || !img_of_box || !rotation_deg || !out || n < 0) return EQA_ERR_INVALID_ARG;
  if ((((uintptr_t)boxes | (uintptr_t)out | (uintptr_t)flipped) & 15)) return EQA_ERR_UNSUPPORTED;
  hipLaunchKernelGGL(boxes_action_kernel, dim3((n + kThreads - 1) / kThreads), dim3(kThreads), 0, (hipStream_t)stream, boxes,
                     img_of_box, rotation_deg, flipped, out, n, width, flip_all);
  return launch_status();
}

int eqa_image_action_nearest(const float* x, float* out, const int32_t* eidx, const float* rtheta, const int32_t* flags,
                             int num_elements, int n_planes, int src_mod, int H, int W, int pad, int OH, int OW, int top,
                             int left, void* stream) {
  return launch_nearest<float>(x, out, eidx, rtheta, flags, num_elements, n_planes, H, W, pad, OH, OW, top, left, src_mod, stream);
}

}  // extern "C"
