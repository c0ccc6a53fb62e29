// libeqa_hip.so, part 28 -- the convolutions of WideResNet50Network / WideResNet101Network's bottleneck blocks
// (custom_nonequivariant_networks.py:133-230 of the reference: torchvision's wide_resnet50_2 / wide_resnet101_2 behind the stem) on a
// channels-last fp32 map: eqa_conv3x3_nhwc's function (conv3x3.hip),
//     z[n][oy][ox][o] = sum_{dy,dx,c} x[n][s oy + dy - pad][s ox + dx - pad][c] W[o][c][dy][dx] + bias[o] (+ res[n][oy][ox][o])
//     y = relu ? max(z, 0) : z                        taps = 9: 3 x 3, pad 1;  taps = 1: 1 x 1, pad 0;  stride s in {1, 2}
// up to 2048 channels, with the K loop (taps x Cin/16 stages) split over waves as well as the output.  The wide bottlenecks have small
// maps and long K loops: layer4's 3 x 3 layer is 1024 -> 1024, 576 stages, and at 256 views of 96 x 96 it has 576 wave tiles for the
// chip's 1024 SIMDs.  Same matrix instruction (v_mfma_f32_32x32x2_f32), same fragment layouts, same packed filters
// (ops.pack_conv3x3_weights), same range-checked buffer loads, same rule for padding taps and rows past P (the lane offset kOob) as
// conv3x3_kernel; the wave tile is its 64 pixels x 32 NT channels.
// K split.  The T = taps Cin / 16 stages make T / 2 stage pairs (a pair is 32 channels of one tap); slice i of `ksplit` takes the
// pairs [floor(i (T/2) / ksplit), floor((i + 1) (T/2) / ksplit)): contiguous, never empty for ksplit <= T/2.  The work unit is
// (wave tile, slice), slices of one tile adjacent (they share their rows of x in L2); every unit accumulates from zero, stages in
// ascending order.
//   ksplit = 1: one launch, the epilogue (bias, res, ReLU) in the kernel: conv3x3_kernel's fmaf chains in its order -- equal bits.
//   ksplit > 1: every unit stores its fp32 partial tile to workspace[slice][P][Cout] with vector stores; convwide_reduce_kernel adds
//               the slices of an output in index order in fp64, rounds once, then applies bias, res and ReLU in the first form's
//               order.  No atomics: two calls give the same bits.  Rows >= P of y and of the workspace are never written.
#include "eqa_common.hpp"

namespace {

typedef float f32x4 __attribute__((ext_vector_type(4)));
typedef float f32x16 __attribute__((ext_vector_type(16)));
typedef unsigned u32x4 __attribute__((ext_vector_type(4)));

constexpr int kMinCh = 32, kMaxCh = 2048;                 // channel counts eqa_convwide_supported admits (multiples of 32)
constexpr int kMaxSplit = 16;
constexpr int kChipWaves = 1024;                          // one wave per SIMD; a constant, never a device query
constexpr unsigned long long kMaxBytes = 0xffffff00ULL;   // of x, res and y each: one 32-bit buffer range; tile and row counters are ints
constexpr unsigned kOob = 0xffffff00u;                    // a lane offset no admitted descriptor covers (+ 48 does not wrap)

template <int NT>
struct CwOps {              // one K-stage of operands
  f32x4 v[2][2];            // [row subtile m][b]
  f32x4 u[NT][2];           // [column subtile n][b]
};

__device__ __forceinline__ f32x4 cw_ld(__amdgpu_buffer_rsrc_t r, unsigned voff, unsigned soff) {
  return __builtin_bit_cast(f32x4, __builtin_amdgcn_raw_buffer_load_b128(r, voff, soff, 0));
}

template <int NT>
__device__ __forceinline__ void cw_load(CwOps<NT>& o, __amdgpu_buffer_rsrc_t rv, __amdgpu_buffer_rsrc_t ru, unsigned voff0, unsigned voff1,
                                        unsigned uoff, unsigned sv, unsigned su) {
#pragma unroll
  for (int b = 0; b < 2; ++b) {
    o.v[0][b] = cw_ld(rv, voff0 + 32 * b, sv);
    o.v[1][b] = cw_ld(rv, voff1 + 32 * b, sv);
#pragma unroll
    for (int n = 0; n < NT; ++n) o.u[n][b] = cw_ld(ru, uoff + (n * 2 + b) * 1024, su);
  }
}

template <int NT>
__device__ __forceinline__ void cw_mma(const CwOps<NT>& o, f32x16 (&acc)[2][NT]) {
#pragma unroll
  for (int b = 0; b < 2; ++b)
#pragma unroll
    for (int t = 0; t < 4; ++t)
#pragma unroll
      for (int m = 0; m < 2; ++m)
#pragma unroll
        for (int n = 0; n < NT; ++n) acc[m][n] = __builtin_amdgcn_mfma_f32_32x32x2f32(o.u[n][b][t], o.v[m][b][t], acc[m][n], 0, 0, 0);
}

struct CwGeom {
  int H, W, OH, OW, Cin, Cout, stride, pad, ksz;   // ksz: 3 or 1 (taps = ksz * ksz)
};

// first stage pair of slice i (i = ksplit: one past the last pair)
__host__ __device__ inline int cw_slice_begin(int i, int pairs, int ksplit) { return (int)((long long)i * pairs / ksplit); }

// x (N, H, W, Cin); Wpk (taps, Cin/16, Cout/32, 2, 64, 4); bias (Cout); res, y (P = N OH OW, Cout); part (ksplit, P, Cout), read
// and written only where ksplit > 1 (bias, res, relu and y are then the reduction's).  total = wave tiles x ksplit units.
template <int NT>
__global__ __launch_bounds__(256, 1) void convwide_kernel(const float* __restrict__ x, const float* __restrict__ Wpk, const float* __restrict__ bias,
                                                          const float* __restrict__ res, float* __restrict__ y, float* __restrict__ part, int relu,
                                                          int P, CwGeom g, unsigned x_bytes, int n_ct, int ksplit, int total, int nwaves) {
  const int lane = threadIdx.x & 63;
  const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const int q = blockIdx.x * 4 + wave;                   // this wave's slot among the grid's waves
  if (q >= total) return;
  const int Cin = g.Cin, Cout = g.Cout;
  const int S = Cin / 16;                                // even: Cin is a multiple of 32
  const int taps = g.ksz * g.ksz;
  const int pairs = taps * (S / 2);
  const int j = lane & 31, h = lane >> 5;
  const unsigned u_stage_bytes = (unsigned)(Cout / 32) * 2 * 1024;  // bytes of one K-stage of Wpk
  const unsigned uoff = lane * 16;
  const __amdgpu_buffer_rsrc_t ru =
      __builtin_amdgcn_make_buffer_rsrc(const_cast<float*>(Wpk), 0, (unsigned)(taps * S) * u_stage_bytes, 0x00020000);
  const __amdgpu_buffer_rsrc_t rx = __builtin_amdgcn_make_buffer_rsrc(const_cast<float*>(x), 0, x_bytes, 0x00020000);
  const unsigned opix = (unsigned)(g.OH * g.OW);

  struct Unit {
    unsigned su;        // scalar byte offset of the tile's first column subtile inside a K-stage of Wpk
    int row0, ct, slice;
    int p0, p1;         // the slice's stage pairs [p0, p1)
    int tap0, s0;       // (tap, stage inside the tap) of pair p0
    // per lane and row subtile m: the byte offset of tap (0, 0)'s channels 4 h .. 4 h + 3 (it wraps below zero on the top / left
    // border, where it is not used) and that tap's input row and column; a row past P has iy0 = -4: no tap is inside
    unsigned base[2];
    int iy0[2], ix0[2];
  };
  auto locate = [&](int u) {
    Unit t;
    const int tile = u / ksplit;
    t.slice = u - tile * ksplit;
    const int rt = tile / n_ct;
    t.ct = tile - rt * n_ct;
    t.row0 = rt * 64;
    t.su = (unsigned)(t.ct * NT) * 2048u;
    t.p0 = cw_slice_begin(t.slice, pairs, ksplit);
    t.p1 = cw_slice_begin(t.slice + 1, pairs, ksplit);
    t.tap0 = (2 * t.p0) / S;
    t.s0 = 2 * t.p0 - t.tap0 * S;
#pragma unroll
    for (int m = 0; m < 2; ++m) {
      const unsigned p = (unsigned)(t.row0 + 32 * m + j);
      const unsigned n = p / opix, r = p - n * opix;
      const unsigned oy = r / (unsigned)g.OW, ox = r - oy * (unsigned)g.OW;
      const int iy0 = (int)oy * g.stride - g.pad, ix0 = (int)ox * g.stride - g.pad;
      t.iy0[m] = p < (unsigned)P ? iy0 : -4;
      t.ix0[m] = ix0;
      t.base[m] = (unsigned)(((int)n * g.H + iy0) * g.W + ix0) * (unsigned)Cin * 4u + 16u * (unsigned)h;
    }
    return t;
  };
  // this lane's offsets of one tap: the neighbour's row where it is inside the lane's own image, kOob on the padding
  auto tap_off = [&](const Unit& t, int tap, unsigned& v0, unsigned& v1) {
    const int dy = tap / g.ksz, dx = tap - dy * g.ksz;
    const unsigned d = (unsigned)((dy * g.W + dx) * Cin) * 4u;
    const bool in0 = (unsigned)(t.iy0[0] + dy) < (unsigned)g.H && (unsigned)(t.ix0[0] + dx) < (unsigned)g.W;
    const bool in1 = (unsigned)(t.iy0[1] + dy) < (unsigned)g.H && (unsigned)(t.ix0[1] + dx) < (unsigned)g.W;
    v0 = in0 ? t.base[0] + d : kOob;
    v1 = in1 ? t.base[1] + d : kOob;
  };

  Unit cur = locate(q);
  unsigned voff0, voff1;
  tap_off(cur, cur.tap0, voff0, voff1);
  CwOps<NT> s0, s1;
  // (stage tap S + s of Wpk is stage 2 p of the flattened loop: the pair index addresses the filters directly)
  cw_load<NT>(s0, rx, ru, voff0, voff1, uoff, (unsigned)cur.s0 * 64u, cur.su + (unsigned)(2 * cur.p0) * u_stage_bytes);
  for (int u = q; u < total; u += nwaves) {
    f32x16 acc[2][NT];
#pragma unroll
    for (int m = 0; m < 2; ++m)
#pragma unroll
      for (int n = 0; n < NT; ++n)
#pragma unroll
        for (int e = 0; e < 16; ++e) acc[m][n][e] = 0.f;
    // the unit after this one (or this one again when it is the last: a harmless reload instead of a conditional load)
    const Unit nxt = locate(u + nwaves < total ? u + nwaves : u);
    unsigned su = cur.su + (unsigned)(2 * cur.p0) * u_stage_bytes;   // of the stage in s0: (tap, s)
    int tap = cur.tap0, s = cur.s0;
    for (int p = cur.p0; p < cur.p1; ++p) {
      // the scheduling barriers keep the next stage's loads inside this stage's MFMA stream (see planegemm.hip).  S is even: the
      // second stage of a pair is always of the same tap as the first
      cw_load<NT>(s1, rx, ru, voff0, voff1, uoff, (unsigned)(s + 1) * 64u, su + u_stage_bytes);
      __builtin_amdgcn_sched_barrier(0);
      cw_mma<NT>(s0, acc);
      __builtin_amdgcn_sched_barrier(0);
      su += 2 * u_stage_bytes;
      s += 2;
      if (p + 1 >= cur.p1) {                             // (wave-uniform) the first stage of the next unit
        tap_off(nxt, nxt.tap0, voff0, voff1);
        s = nxt.s0;
        su = nxt.su + (unsigned)(2 * nxt.p0) * u_stage_bytes;
      } else if (s >= S) {                               // the next tap
        s = 0;
        ++tap;
        tap_off(cur, tap, voff0, voff1);
      }
      cw_load<NT>(s0, rx, ru, voff0, voff1, uoff, (unsigned)s * 64u, su);
      __builtin_amdgcn_sched_barrier(0);
      cw_mma<NT>(s1, acc);
      __builtin_amdgcn_sched_barrier(0);
    }
    // epilogue: accumulator register e of lane (h, j) is output channel (e & 3) + 8 (e >> 2) + 4 h of its 32-channel subtile, pixel
    // j of its 32-row subtile: register group e >> 2 is 16 contiguous bytes of y (and of res, bias, the partial tile)
    {
      const int rows = min(64, P - cur.row0);
      const int col0 = cur.ct * (32 * NT);
      const size_t base = (size_t)cur.row0 * Cout + col0;
      const unsigned bytes = (unsigned)(((size_t)(rows - 1) * Cout + Cout - col0) * 4);
      const bool whole = ksplit == 1;
      float* const out = whole ? y + base : part + (size_t)cur.slice * (size_t)P * Cout + base;
      const __amdgpu_buffer_rsrc_t ry = __builtin_amdgcn_make_buffer_rsrc(out, 0, bytes, 0x00020000);
      // (without a residual the descriptor covers nothing: the loads below are not issued either)
      const bool has_res = whole && res;
      const __amdgpu_buffer_rsrc_t rr =
          __builtin_amdgcn_make_buffer_rsrc(const_cast<float*>(has_res ? res + base : x), 0, has_res ? bytes : 0u, 0x00020000);
      const unsigned moff = (unsigned)(j * Cout + 4 * h) * 4u;
#pragma unroll
      for (int n = 0; n < NT; ++n)
#pragma unroll
        for (int gq = 0; gq < 4; ++gq) {
          const int c = col0 + 32 * n + 8 * gq + 4 * h;                // < Cout, a multiple of 4
          f32x4 bv = {0.f, 0.f, 0.f, 0.f};
          if (whole) bv = *reinterpret_cast<const f32x4*>(bias + c);
#pragma unroll
          for (int m = 0; m < 2; ++m) {
            // (the row subtile's offset rides in the lane offset, which the range check certainly covers)
            const unsigned off = moff + (unsigned)(32 * n + 8 * gq) * 4u + (unsigned)m * 32u * (unsigned)Cout * 4u;
            f32x4 v;
#pragma unroll
            for (int k = 0; k < 4; ++k) v[k] = acc[m][n][4 * gq + k];
            if (whole) {
#pragma unroll
              for (int k = 0; k < 4; ++k) v[k] += bv[k];
              if (has_res) {
                const f32x4 r = cw_ld(rr, off, 0);
#pragma unroll
                for (int k = 0; k < 4; ++k) v[k] += r[k];
              }
              if (relu) {
#pragma unroll
                for (int k = 0; k < 4; ++k) v[k] = fmaxf(v[k], 0.f);
              }
            }
            __builtin_amdgcn_raw_buffer_store_b128(__builtin_bit_cast(u32x4, v), ry, off, 0, 0);
          }
        }
    }
    cur = nxt;
  }
}

// y[i] = [relu]((float)(sum_slices part[slice][i], in index order, in fp64) + bias (+ res)): n4 = P Cout / 4 groups of four channels
__global__ __launch_bounds__(256) void convwide_reduce_kernel(const float* __restrict__ part, const float* __restrict__ bias,
                                                              const float* __restrict__ res, float* __restrict__ y, int relu, size_t n4,
                                                              int cout4, int ksplit) {
  const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
  if (i >= n4) return;
  const f32x4* p4 = reinterpret_cast<const f32x4*>(part);
  double a[4] = {0.0, 0.0, 0.0, 0.0};
  for (int sl = 0; sl < ksplit; ++sl) {
    const f32x4 v = p4[(size_t)sl * n4 + i];
#pragma unroll
    for (int k = 0; k < 4; ++k) a[k] += (double)v[k];
  }
  const f32x4 bv = reinterpret_cast<const f32x4*>(bias)[i % (size_t)cout4];
  f32x4 v;
#pragma unroll
  for (int k = 0; k < 4; ++k) v[k] = (float)a[k] + bv[k];
  if (res) {
    const f32x4 r = reinterpret_cast<const f32x4*>(res)[i];
#pragma unroll
    for (int k = 0; k < 4; ++k) v[k] += r[k];
  }
  if (relu) {
#pragma unroll
    for (int k = 0; k < 4; ++k) v[k] = fmaxf(v[k], 0.f);
  }
  reinterpret_cast<f32x4*>(y)[i] = v;
}

// output size of one axis, or 0 where the filter does not fit
inline long long cw_out(int n, int k, int pad, int stride) { return n + 2 * pad < k ? 0 : (n + 2 * pad - k) / stride + 1; }

struct CwPlan {
  int ksz, pad, OH, OW, NT, n_ct, pairs;
  long long P, tiles;
};

// (for a shape eqa_convwide_supported admits)
inline CwPlan cw_plan(long long N, int H, int W, int Cin, int Cout, int taps, int stride) {
  CwPlan p;
  p.ksz = taps == 9 ? 3 : 1;
  p.pad = taps == 9 ? 1 : 0;
  p.OH = (int)cw_out(H, p.ksz, p.pad, stride);
  p.OW = (int)cw_out(W, p.ksz, p.pad, stride);
  p.P = N * p.OH * p.OW;                                  // P * Cout * 4 < 2^32
  p.NT = Cout % 64 == 0 ? 2 : 1;
  p.n_ct = Cout / (32 * p.NT);
  p.tiles = (p.P + 63) / 64 * p.n_ct;                     // < 2^31
  p.pairs = taps * (Cin / 32);
  return p;
}

}  // namespace

extern "C" {

int eqa_convwide_supported(long long N, int H, int W, int Cin, int Cout, int taps, int stride) {
  if (N < 0 || H <= 0 || W <= 0 || Cin < kMinCh || Cout < kMinCh || Cin > kMaxCh || Cout > kMaxCh || Cin % 32 || Cout % 32) return 0;
  if (!(taps == 9 || taps == 1) || !(stride == 1 || stride == 2)) return 0;
  const int k = taps == 9 ? 3 : 1, pad = taps == 9 ? 1 : 0;
  const long long OH = cw_out(H, k, pad, stride), OW = cw_out(W, k, pad, stride);
  if (OH < 1 || OW < 1) return 0;
  // (H, W < 2^31 and N < 2^63 / 2^62: compare by division, nothing overflows)
  const unsigned long long in_px = (unsigned long long)H * (unsigned long long)W, out_px = (unsigned long long)OH * (unsigned long long)OW;
  const unsigned long long lim_in = kMaxBytes / (4ULL * (unsigned long long)Cin), lim_out = kMaxBytes / (4ULL * (unsigned long long)Cout);
  if (in_px > lim_in || out_px > lim_out) return 0;
  if (N > 0 && ((unsigned long long)N > lim_in / in_px || (unsigned long long)N > lim_out / out_px)) return 0;
  return 1;
}

int eqa_convwide_ksplit(long long N, int H, int W, int Cin, int Cout, int taps, int stride) {
  if (!eqa_convwide_supported(N, H, W, Cin, Cout, taps, stride)) return 0;
  const CwPlan p = cw_plan(N, H, W, Cin, Cout, taps, stride);
  // the smallest power of two that brings tiles x ksplit to the chip's 1024 waves, inside the admitted range
  int k = 1;
  while (k < kMaxSplit && p.tiles * k < kChipWaves) k *= 2;
  return std::max(1, std::min(k, std::min(kMaxSplit, p.pairs)));
}

long long eqa_convwide_workspace_bytes(long long N, int H, int W, int Cin, int Cout, int taps, int stride, int ksplit) {
  if (!eqa_convwide_supported(N, H, W, Cin, Cout, taps, stride)) return 0;
  const CwPlan p = cw_plan(N, H, W, Cin, Cout, taps, stride);
  if (ksplit == 0) ksplit = eqa_convwide_ksplit(N, H, W, Cin, Cout, taps, stride);
  if (ksplit <= 1 || ksplit > std::min(kMaxSplit, p.pairs)) return 0;
  return (long long)ksplit * p.P * Cout * 4;
}

int eqa_convwide_nhwc(const float* x, const float* Wpk, const float* bias, const float* res, int relu, float* y, void* workspace, long long N,
                      int H, int W, int Cin, int Cout, int taps, int stride, int ksplit, void* stream) {
  if (N < 0 || H <= 0 || W <= 0 || Cin <= 0 || Cout <= 0) return EQA_ERR_INVALID_ARG;
  if (!eqa_convwide_supported(N, H, W, Cin, Cout, taps, stride)) return EQA_ERR_UNSUPPORTED;
  const CwPlan p = cw_plan(N, H, W, Cin, Cout, taps, stride);
  if (ksplit == 0) ksplit = eqa_convwide_ksplit(N, H, W, Cin, Cout, taps, stride);
  if (ksplit < 1 || ksplit > std::min(kMaxSplit, p.pairs)) return EQA_ERR_UNSUPPORTED;
  if (N == 0) return EQA_OK;
  if (!x || !Wpk || !bias || !y || (ksplit > 1 && !workspace)) return EQA_ERR_INVALID_ARG;
  if (y == x || y == res) return EQA_ERR_INVALID_ARG;
  if (ksplit > 1 && (workspace == x || workspace == Wpk || workspace == bias || workspace == res || workspace == y)) return EQA_ERR_INVALID_ARG;
  if ((((uintptr_t)x | (uintptr_t)Wpk | (uintptr_t)bias | (uintptr_t)res | (uintptr_t)y | (ksplit > 1 ? (uintptr_t)workspace : 0)) & 15))
    return EQA_ERR_UNSUPPORTED;
  CwGeom g;
  g.ksz = p.ksz, g.pad = p.pad, g.OH = p.OH, g.OW = p.OW;
  g.H = H, g.W = W, g.Cin = Cin, g.Cout = Cout, g.stride = stride;
  const unsigned x_bytes = (unsigned)((unsigned long long)N * H * W * Cin * 4ULL);
  const long long total = p.tiles * ksplit;                 // < 2^35: the unit counter is an int
  if (total > 0x7fffffffLL) return EQA_ERR_UNSUPPORTED;
  // persistent waves: one per SIMD, 1024 on the chip; fewer when there is less work
  const int nwaves = (int)std::min<long long>(kChipWaves, (total + 3) / 4 * 4);
  const dim3 grid((unsigned)(nwaves / 4));
  hipStream_t st = (hipStream_t)stream;
  float* part = ksplit > 1 ? (float*)workspace : nullptr;
  if (p.NT == 2)
    hipLaunchKernelGGL((convwide_kernel<2>), grid, dim3(256), 0, st, x, Wpk, bias, res, y, part, relu, (int)p.P, g, x_bytes, p.n_ct, ksplit,
                       (int)total, nwaves);
  else
    hipLaunchKernelGGL((convwide_kernel<1>), grid, dim3(256), 0, st, x, Wpk, bias, res, y, part, relu, (int)p.P, g, x_bytes, p.n_ct, ksplit,
                       (int)total, nwaves);
  if (ksplit > 1) {
    const int st1 = launch_status();
    if (st1 != EQA_OK) return st1;
    const size_t n4 = (size_t)p.P * Cout / 4;
    hipLaunchKernelGGL(convwide_reduce_kernel, dim3((unsigned)((n4 + 255) / 256)), dim3(256), 0, st, part, bias, res, y, relu, n4, Cout / 4,
                       ksplit);
  }
  return launch_status();
}

}  // extern "C"
