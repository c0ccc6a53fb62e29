// libeqa_hip.so, part 27 -- ResNet18Network's basic blocks in TRAINING (custom_nonequivariant_networks.py:83-130 of the reference:
// torchvision's resnet18 behind the stem, with batch statistics): the filter gradient of eqa_conv3x3_nhwc (conv3x3.hip; its data
// gradient is a mode of that kernel and stands beside it) and the batch-norm block with the residual inside it.
//
// -- filter gradient --------------------------------------------------------------------------------------------------------------
//     dW[o][c][dy][dx] = sum_{n,oy,ox} dz[n][oy][ox][o] x[n][s oy + dy - pad][s ox + dx - pad][c]      (taps on the padding add 0)
// One tap is gconv1x1_wgrad_kernel's contraction (gconv1x1.hip) with x's rows gathered: the contraction runs over the output pixels,
// a K-step of v_mfma_f32_32x32x2_f32 is a PAIR of them (k = h, the lane's half), and a lane's row / column of the tile stands for a
// channel, so no operand needs a transpose:
//   dz fragment (the A operand, output channel = row i):   lane 32 h + i holds dz[r0 + 2 t + h][o0 + VA i + a], a = 0..VA-1
//   x fragment  (the B operand, input channel = column j): lane 32 h + j holds x[tap's neighbour of pixel r0 + 2 t + h][c0 + VB j + b]
// With the input channels on the lanes a wave's partial tile is rows of dW's own (Cout, Cin) order.  The neighbour is a per-lane byte
// offset into ONE descriptor over the whole of x, as in conv3x3_kernel: the 32 lanes of a half share their pixel, whose (n, oy, ox)
// is found by division once per wave and carried from pair to pair; a tap on the zero padding -- the test is on the pixel's own
// image coordinates, so nothing leaks across an image seam -- and a pixel past the wave's range take the lane offset kOob, which no
// admitted descriptor covers: the load is dropped and returns zero.  dz's descriptor covers the wave's range alone.
// Work: wave = (one tap, one 32 VA x 32 VB tile of it, one contiguous range of L output pixels); the ranges split the contraction
// over the chip's waves (one per SIMD, up to 1024), chosen from the sizes: stage 1 of the recipe (64 x 576 over 147 k pixels) gets
// 113 ranges, stage 4 (512 x 4608 over 2.3 k) seven.  Every wave writes its partial tile to part[split][tap][Cout][Cin];
// conv3x3_wgrad_reduce adds the splits in a fixed order in fp64 and writes (Cout, Cin, k, k).  No atomics anywhere.
//
// -- batch-norm (given scale / shift) + residual + ReLU on (npix, C), C % 4 == 0 --------------------------------------------------
//     t = fmaf(scale[c], z, shift[c]) (+ res),   y = relu ? max(t, 0) : t
// and its backward in the two passes of eqa_bn_act_bwd_* (convnet_train.hip): per-channel sums of g = gy [t > 0] and g zhat as fp64
// partials per block, in the layout eqa_bn_act_bwd_finalize reads, then dz = gscale (g - m1 - zhat m2) with dres = g beside it.
// t is one function (bra_t) in all three kernels: the backward's mask is the forward's mask.
#include "eqa_common.hpp"

namespace {

typedef float f32x2 __attribute__((ext_vector_type(2)));
typedef float f32x4 __attribute__((ext_vector_type(4)));
typedef float f32x16 __attribute__((ext_vector_type(16)));

constexpr unsigned kOob = 0xffffff00u;   // a lane offset no admitted descriptor covers (conv3x3.hip)
constexpr int kWgPairs = 4;              // output-pixel pairs per stage: 8 pixels in flight per operand and buffer
constexpr int kWgWaves = 1024;           // one wave per SIMD
constexpr int kWgRedGroups = 16;         // waves of a reduce block: each adds every 16th split, wave 0 adds the sixteen

struct W3Geom {
  int H, W, OH, OW, Cin, Cout, stride, pad, ksz;   // ksz: 3 or 1 (taps = ksz * ksz)
};

struct W3Plan {
  int va, vb;        // floats per lane and load of dz, of x
  int n_nt, units;   // column (Cin) tiles; (tap, tile) pairs
  int L, ns;         // output pixels per wave; splits
};

inline int w3_width(int C) { return C % 128 == 0 ? 4 : C % 64 == 0 ? 2 : 1; }

inline W3Plan w3_plan(long long P, int Cin, int Cout, int taps) {
  W3Plan p;
  p.va = w3_width(Cout);
  p.vb = w3_width(Cin);
  p.n_nt = Cin / (32 * p.vb);
  p.units = taps * (Cout / (32 * p.va)) * p.n_nt;                  // <= 9 * 16
  const long long want = std::max(1, kWgWaves / p.units);          // >= 7
  const long long L = std::max<long long>(16, ((P + want - 1) / want + 15) / 16 * 16);
  p.L = (int)L;
  p.ns = (int)std::max<long long>(1, (P + L - 1) / L);             // <= want
  return p;
}

template <int V>
__device__ __forceinline__ void w3_ld(float (&d)[V], __amdgpu_buffer_rsrc_t r, unsigned voff) {
  if constexpr (V == 4) {
    const f32x4 t = __builtin_bit_cast(f32x4, __builtin_amdgcn_raw_buffer_load_b128(r, voff, 0, 0));
#pragma unroll
    for (int k = 0; k < 4; ++k) d[k] = t[k];
  } else if constexpr (V == 2) {
    const f32x2 t = __builtin_bit_cast(f32x2, __builtin_amdgcn_raw_buffer_load_b64(r, voff, 0, 0));
    d[0] = t[0];
    d[1] = t[1];
  } else {
    d[0] = __builtin_bit_cast(float, __builtin_amdgcn_raw_buffer_load_b32(r, voff, 0, 0));
  }
}

// the output pixel of this lane's half, carried from pair to pair: one step is one carry chain, whatever OW and OH are
struct W3Pos {
  int n, oy, ox, rel;    // rel: the pixel's index inside the wave's range
};
__device__ __forceinline__ void w3_step(W3Pos& p, int OH, int OW) {
  p.ox += 1;
  const bool cx = p.ox == OW;
  p.ox = cx ? 0 : p.ox;
  p.oy += (int)cx;
  const bool cy = p.oy == OH;
  p.oy = cy ? 0 : p.oy;
  p.n += (int)cy;
  p.rel += 1;
}

template <int VA, int VB>
struct W3Ops {              // one stage of operands
  float a[kWgPairs][VA];
  float b[kWgPairs][VB];
};

// (dz: the whole offset rides in the lane offset, which the range check covers)
template <int VA, int VB>
__device__ __forceinline__ void w3_load(W3Ops<VA, VB>& o, __amdgpu_buffer_rsrc_t ra, __amdgpu_buffer_rsrc_t rx, unsigned& aoff, unsigned apair,
                                        W3Pos& pos, int rows, const W3Geom& g, int dy, int dx, unsigned choff) {
#pragma unroll
  for (int t = 0; t < kWgPairs; ++t) {
    w3_ld<VA>(o.a[t], ra, aoff);
    aoff += apair;
    const int iy = pos.oy * g.stride + dy - g.pad, ix = pos.ox * g.stride + dx - g.pad;
    const bool in = pos.rel < rows && (unsigned)iy < (unsigned)g.H && (unsigned)ix < (unsigned)g.W;
    // (inside the range and the image the product is below x's size, itself below 2^32; elsewhere it is not used)
    const unsigned off = (unsigned)((pos.n * g.H + iy) * g.W + ix) * (unsigned)g.Cin * 4u + choff;
    w3_ld<VB>(o.b[t], rx, in ? off : kOob);
    w3_step(pos, g.OH, g.OW);
    w3_step(pos, g.OH, g.OW);
  }
}

template <int VA, int VB>
__device__ __forceinline__ void w3_mma(const W3Ops<VA, VB>& o, f32x16 (&acc)[VA][VB]) {
#pragma unroll
  for (int t = 0; t < kWgPairs; ++t)
#pragma unroll
    for (int a = 0; a < VA; ++a)
#pragma unroll
      for (int b = 0; b < VB; ++b) acc[a][b] = __builtin_amdgcn_mfma_f32_32x32x2f32(o.a[t][a], o.b[t][b], acc[a][b], 0, 0, 0);
}

// x (N, H, W, Cin); dz (P = N OH OW, Cout); part (ns, taps, Cout, Cin)
template <int VA, int VB>
__global__ __launch_bounds__(256, 1) void conv3x3_wgrad_kernel(const float* __restrict__ x, const float* __restrict__ dz, float* __restrict__ part,
                                                               int P, W3Geom g, unsigned x_bytes, int n_nt, int units, int total, int L) {
  const int lane = threadIdx.x & 63;
  const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const int q = blockIdx.x * 4 + wave;                   // tiles fastest, then taps: the waves of a block share their pixels
  if (q >= total) return;
  const int Cin = g.Cin, Cout = g.Cout;
  const int taps = g.ksz * g.ksz, tiles = units / taps;
  const int split = q / units, unit = q - split * units;
  const int tap = unit / tiles, tile = unit - tap * tiles;
  const int mt = tile / n_nt, nt = tile - mt * n_nt;
  const int o0 = mt * 32 * VA, c0 = nt * 32 * VB;
  const int dy = tap / g.ksz, dx = tap - dy * g.ksz;
  const int r0 = split * L;
  const int rows = min(L, P - r0);                       // >= 1: ns = ceil(P / L)
  const int i = lane & 31, h = lane >> 5;
  const __amdgpu_buffer_rsrc_t ra =
      __builtin_amdgcn_make_buffer_rsrc(const_cast<float*>(dz) + (size_t)r0 * Cout, 0, (unsigned)rows * (unsigned)Cout * 4u, 0x00020000);
  const __amdgpu_buffer_rsrc_t rx = __builtin_amdgcn_make_buffer_rsrc(const_cast<float*>(x), 0, x_bytes, 0x00020000);
  const unsigned apair = 2u * (unsigned)Cout * 4u;       // bytes from one pair of dz's rows to the next
  unsigned aoff = (unsigned)(h * Cout + o0 + VA * i) * 4u;
  const unsigned choff = (unsigned)(c0 + VB * i) * 4u;
  W3Pos pos;
  {
    const unsigned p = (unsigned)(r0 + h), opix = (unsigned)(g.OH * g.OW);
    const unsigned n = p / opix, r = p - n * opix;
    const unsigned oy = r / (unsigned)g.OW;
    pos.n = (int)n, pos.oy = (int)oy, pos.ox = (int)(r - oy * (unsigned)g.OW), pos.rel = h;
  }

  f32x16 acc[VA][VB];
#pragma unroll
  for (int a = 0; a < VA; ++a)
#pragma unroll
    for (int b = 0; b < VB; ++b)
#pragma unroll
      for (int e = 0; e < 16; ++e) acc[a][b][e] = 0.f;
  W3Ops<VA, VB> s0, s1;
  w3_load<VA, VB>(s0, ra, rx, aoff, apair, pos, rows, g, dy, dx, choff);
  const int stages = (rows + 2 * kWgPairs - 1) / (2 * kWgPairs);
  // two stages per trip, each loaded under the other's matrix instructions; a stage past the range loads zeros (dz: at most
  // (L + 24) rows of 2 KB from the descriptor's base, L <= P / 7 + 16: the offsets stay far inside 32 bits; x: kOob)
  for (int s = 0; s < stages; s += 2) {
    w3_load<VA, VB>(s1, ra, rx, aoff, apair, pos, rows, g, dy, dx, choff);
    __builtin_amdgcn_sched_barrier(0);
    w3_mma<VA, VB>(s0, acc);
    __builtin_amdgcn_sched_barrier(0);
    w3_load<VA, VB>(s0, ra, rx, aoff, apair, pos, rows, g, dy, dx, choff);
    __builtin_amdgcn_sched_barrier(0);
    w3_mma<VA, VB>(s1, acc);
    __builtin_amdgcn_sched_barrier(0);
  }
  // accumulator register e of lane (h, j) of subtile (a, b) is row (e & 3) + 8 (e >> 2) + 4 h, column j: channel pair
  // (o0 + VA row + a, c0 + VB j + b) -- the VB subtiles of a lane are 4 VB contiguous bytes of a row of the partial tile
  float* const pt = part + ((size_t)split * taps + tap) * (size_t)Cout * Cin;
#pragma unroll
  for (int a = 0; a < VA; ++a)
#pragma unroll
    for (int e = 0; e < 16; ++e) {
      const int row = (e & 3) + 8 * (e >> 2) + 4 * h;
      float* const dst = pt + (size_t)(o0 + VA * row + a) * Cin + c0 + VB * i;
      if constexpr (VB == 4) {
        *reinterpret_cast<f32x4*>(dst) = f32x4{acc[a][0][e], acc[a][1][e], acc[a][2][e], acc[a][3][e]};
      } else if constexpr (VB == 2) {
        *reinterpret_cast<f32x2*>(dst) = f32x2{acc[a][0][e], acc[a][1][e]};
      } else {
        *dst = acc[a][0][e];
      }
    }
}

// part (ns, taps, Cout, Cin) -> dW (Cout, Cin, k, k).  Block = 64 consecutive entries x 16 waves: wave g adds the splits g, g + 16,
// ... of its entries in fp64, wave 0 adds the sixteen sums in order.
__global__ __launch_bounds__(64 * kWgRedGroups) void conv3x3_wgrad_reduce(const float* __restrict__ part, float* __restrict__ dW, int ns, int taps,
                                                                         int Cin, int Cout) {
  __shared__ double sm[kWgRedGroups][64];
  const int lane = threadIdx.x & 63, g = threadIdx.x >> 6;
  const int plane = Cout * Cin, n = taps * plane;          // <= 9 * 2^18
  const int e = blockIdx.x * 64 + lane;
  double s = 0.0;
  if (e < n)
    for (int k = g; k < ns; k += kWgRedGroups) s += (double)part[(size_t)k * n + e];
  sm[g][lane] = s;
  __syncthreads();
  if (g != 0 || e >= n) return;
  double t = 0.0;
#pragma unroll
  for (int k = 0; k < kWgRedGroups; ++k) t += sm[k][lane];
  const int tap = e / plane, oc = e - tap * plane;
  dW[(size_t)oc * taps + tap] = (float)t;
}

template <int VA>
void w3_launch(int vb, dim3 grid, hipStream_t st, const float* x, const float* dz, float* part, int P, const W3Geom& g, unsigned x_bytes,
               const W3Plan& p) {
  const int total = p.units * p.ns;
  if (vb == 4)
    hipLaunchKernelGGL((conv3x3_wgrad_kernel<VA, 4>), grid, dim3(256), 0, st, x, dz, part, P, g, x_bytes, p.n_nt, p.units, total, p.L);
  else if (vb == 2)
    hipLaunchKernelGGL((conv3x3_wgrad_kernel<VA, 2>), grid, dim3(256), 0, st, x, dz, part, P, g, x_bytes, p.n_nt, p.units, total, p.L);
  else
    hipLaunchKernelGGL((conv3x3_wgrad_kernel<VA, 1>), grid, dim3(256), 0, st, x, dz, part, P, g, x_bytes, p.n_nt, p.units, total, p.L);
}

inline W3Geom w3_geom(int H, int W, int Cin, int Cout, int taps, int stride) {
  W3Geom g;
  g.ksz = taps == 9 ? 3 : 1;
  g.pad = taps == 9 ? 1 : 0;
  g.H = H, g.W = W, g.Cin = Cin, g.Cout = Cout, g.stride = stride;
  g.OH = (H + 2 * g.pad - g.ksz) / stride + 1;             // >= 1 for every admitted shape
  g.OW = (W + 2 * g.pad - g.ksz) / stride + 1;
  return g;
}

// ---------------------------------------------------------------------------------------------------------------------------------
// batch-norm + residual + ReLU
// ---------------------------------------------------------------------------------------------------------------------------------
__device__ __forceinline__ float bra_t(float sc, float z, float sh, bool has_res, float r) {
  const float t = fmaf(sc, z, sh);
  return has_res ? t + r : t;
}
__device__ __forceinline__ float bra_g(float gy, float t, int relu) { return (relu && !(t > 0.0f)) ? 0.0f : gy; }

__global__ __launch_bounds__(kThreads) void bn_res_act_fwd_kernel(const float* __restrict__ z, const float* __restrict__ scale,
                                                                 const float* __restrict__ shift, const float* __restrict__ res, int relu,
                                                                 float* __restrict__ y, size_t nquad, int Q) {
  const size_t i0 = (size_t)blockIdx.x * kThreads + threadIdx.x, stride = (size_t)gridDim.x * kThreads;
  QuadWalk w(i0, stride, Q);
  const bool hr = res != nullptr;
  for (size_t i = i0; i < nquad; i += stride, w.next()) {
    const int q = (int)w.q;
    const float4 v = reinterpret_cast<const float4*>(z)[i];
    const float4 r = hr ? reinterpret_cast<const float4*>(res)[i] : make_float4(0.f, 0.f, 0.f, 0.f);
    const float4 sc = reinterpret_cast<const float4*>(scale)[q], sh = reinterpret_cast<const float4*>(shift)[q];
    float4 t = make_float4(bra_t(sc.x, v.x, sh.x, hr, r.x), bra_t(sc.y, v.y, sh.y, hr, r.y), bra_t(sc.z, v.z, sh.z, hr, r.z),
                           bra_t(sc.w, v.w, sh.w, hr, r.w));
    if (relu) t = make_float4(fmaxf(t.x, 0.f), fmaxf(t.y, 0.f), fmaxf(t.z, 0.f), fmaxf(t.w, 0.f));
    reinterpret_cast<float4*>(y)[i] = t;
  }
}

// partial[(blk * C + c) * 2 + {0, 1}] = sum of g, sum of g * zhat over the block's pixels (bn_act_bwd_reduce_kernel's layout)
__global__ __launch_bounds__(kThreads) void bn_res_act_bwd_reduce_kernel(const float* __restrict__ gy, const float* __restrict__ z,
                                                                        const float* __restrict__ scale, const float* __restrict__ shift,
                                                                        const float* __restrict__ res, int relu, const float* __restrict__ mean,
                                                                        const float* __restrict__ rstd, double* __restrict__ partial, size_t npix,
                                                                        int C, int pix_per_block) {
  __shared__ float4 s_red[2][kThreads];
  const int Q = C >> 2;
  const int lanes = min(Q, kThreads);
  const int rows = kThreads / lanes;
  const int q0 = threadIdx.x % lanes, r0 = threadIdx.x / lanes;
  const size_t p0 = min(npix, (size_t)blockIdx.x * pix_per_block);
  const size_t p1 = min(npix, p0 + pix_per_block);
  const bool hr = res != nullptr;
  for (int qb = 0; qb < Q; qb += lanes) {      // uniform trip count: every thread reaches both barriers of every trip
    const int q = qb + q0;
    const bool has_q = q < Q;
    const int qc = has_q ? q : 0;
    const float4 sc = reinterpret_cast<const float4*>(scale)[qc], sh = reinterpret_cast<const float4*>(shift)[qc];
    const float4 mu = reinterpret_cast<const float4*>(mean)[qc], rs = reinterpret_cast<const float4*>(rstd)[qc];
    float4 s = make_float4(0.f, 0.f, 0.f, 0.f), sx = s;
    if (r0 < rows && has_q) {
      for (size_t p = p0 + r0; p < p1; p += rows) {
        const size_t i = p * Q + q;
        const float4 g4 = reinterpret_cast<const float4*>(gy)[i];
        const float4 v = reinterpret_cast<const float4*>(z)[i];
        const float4 r = hr ? reinterpret_cast<const float4*>(res)[i] : make_float4(0.f, 0.f, 0.f, 0.f);
        const float g0 = bra_g(g4.x, bra_t(sc.x, v.x, sh.x, hr, r.x), relu), g1 = bra_g(g4.y, bra_t(sc.y, v.y, sh.y, hr, r.y), relu);
        const float g2 = bra_g(g4.z, bra_t(sc.z, v.z, sh.z, hr, r.z), relu), g3 = bra_g(g4.w, bra_t(sc.w, v.w, sh.w, hr, r.w), relu);
        s.x += g0; s.y += g1; s.z += g2; s.w += g3;
        sx.x += g0 * (v.x - mu.x) * rs.x; sx.y += g1 * (v.y - mu.y) * rs.y;
        sx.z += g2 * (v.z - mu.z) * rs.z; sx.w += g3 * (v.w - mu.w) * rs.w;
      }
    }
    __syncthreads();
    s_red[0][threadIdx.x] = s;
    s_red[1][threadIdx.x] = sx;
    __syncthreads();
    if (r0 == 0 && has_q) {
      for (int r = 1; r < rows; ++r) {
        const float4 a = s_red[0][r * lanes + q0], b = s_red[1][r * lanes + q0];
        s.x += a.x; s.y += a.y; s.z += a.z; s.w += a.w;
        sx.x += b.x; sx.y += b.y; sx.z += b.z; sx.w += b.w;
      }
      double* o = partial + ((size_t)blockIdx.x * C + 4 * q) * 2;
      o[0] = s.x; o[1] = sx.x; o[2] = s.y; o[3] = sx.y; o[4] = s.z; o[5] = sx.z; o[6] = s.w; o[7] = sx.w;
    }
  }
}

// dz = gscale[c] * (g - m1[c] - zhat * m2[c]);  dres = g where it is asked for
__global__ __launch_bounds__(kThreads) void bn_res_act_bwd_apply_kernel(const float* __restrict__ gy, const float* __restrict__ z,
                                                                       const float* __restrict__ scale, const float* __restrict__ shift,
                                                                       const float* __restrict__ res, int relu, const float* __restrict__ mean,
                                                                       const float* __restrict__ rstd, const float* __restrict__ gscale,
                                                                       const float* __restrict__ m1, const float* __restrict__ m2,
                                                                       float* __restrict__ dz, float* __restrict__ dres, size_t nquad, int Q) {
  const size_t i0 = (size_t)blockIdx.x * kThreads + threadIdx.x, stride = (size_t)gridDim.x * kThreads;
  QuadWalk w(i0, stride, Q);
  const bool hr = res != nullptr;
  for (size_t i = i0; i < nquad; i += stride, w.next()) {
    const int q = (int)w.q;
    const float4 g4 = reinterpret_cast<const float4*>(gy)[i];
    const float4 v = reinterpret_cast<const float4*>(z)[i];
    const float4 r = hr ? reinterpret_cast<const float4*>(res)[i] : make_float4(0.f, 0.f, 0.f, 0.f);
    const float4 sc = reinterpret_cast<const float4*>(scale)[q], sh = reinterpret_cast<const float4*>(shift)[q];
    const float4 mu = reinterpret_cast<const float4*>(mean)[q], rs = reinterpret_cast<const float4*>(rstd)[q];
    const float4 gs = reinterpret_cast<const float4*>(gscale)[q], a1 = reinterpret_cast<const float4*>(m1)[q],
                 a2 = reinterpret_cast<const float4*>(m2)[q];
    const float4 g = make_float4(bra_g(g4.x, bra_t(sc.x, v.x, sh.x, hr, r.x), relu), bra_g(g4.y, bra_t(sc.y, v.y, sh.y, hr, r.y), relu),
                                 bra_g(g4.z, bra_t(sc.z, v.z, sh.z, hr, r.z), relu), bra_g(g4.w, bra_t(sc.w, v.w, sh.w, hr, r.w), relu));
    float4 o;
    o.x = gs.x * (g.x - a1.x - (v.x - mu.x) * rs.x * a2.x);
    o.y = gs.y * (g.y - a1.y - (v.y - mu.y) * rs.y * a2.y);
    o.z = gs.z * (g.z - a1.z - (v.z - mu.z) * rs.z * a2.z);
    o.w = gs.w * (g.w - a1.w - (v.w - mu.w) * rs.w * a2.w);
    reinterpret_cast<float4*>(dz)[i] = o;
    if (dres) reinterpret_cast<float4*>(dres)[i] = g;
  }
}

inline unsigned bra_stream_blocks(size_t nquad) { return (unsigned)std::min<size_t>((nquad + kThreads - 1) / kThreads, 256 * 16); }

}  // namespace

extern "C" {

int eqa_conv3x3_wgrad_supported(long long N, int H, int W, int Cin, int Cout, int taps, int stride) {
  return eqa_conv3x3_supported(N, H, W, Cin, Cout, taps, stride);
}

long long eqa_conv3x3_wgrad_workspace_bytes(long long N, int H, int W, int Cin, int Cout, int taps, int stride) {
  if (N <= 0 || !eqa_conv3x3_supported(N, H, W, Cin, Cout, taps, stride)) return 0;
  const W3Geom g = w3_geom(H, W, Cin, Cout, taps, stride);
  return (long long)w3_plan(N * g.OH * g.OW, Cin, Cout, taps).ns * taps * Cin * Cout * 4LL;
}

int eqa_conv3x3_wgrad(const float* x, const float* dz, void* workspace, float* dW, long long N, int H, int W, int Cin, int Cout, int taps,
                      int stride, void* stream) {
  if (N < 0 || H <= 0 || W <= 0 || Cin <= 0 || Cout <= 0) return EQA_ERR_INVALID_ARG;
  if (!eqa_conv3x3_supported(N, H, W, Cin, Cout, taps, stride)) return EQA_ERR_UNSUPPORTED;
  if (!dW || (const float*)dW == x || (const float*)dW == dz) return EQA_ERR_INVALID_ARG;
  hipStream_t st = (hipStream_t)stream;
  if (N == 0) {
    if ((uintptr_t)dW & 15) return EQA_ERR_UNSUPPORTED;
    return hipMemsetAsync(dW, 0, (size_t)Cout * Cin * taps * 4, st) == hipSuccess ? EQA_OK : EQA_ERR_LAUNCH;
  }
  if (!x || !dz || !workspace || x == dz || workspace == (const void*)x || workspace == (const void*)dz || workspace == (void*)dW)
    return EQA_ERR_INVALID_ARG;
  if ((((uintptr_t)x | (uintptr_t)dz | (uintptr_t)dW | (uintptr_t)workspace) & 15)) return EQA_ERR_UNSUPPORTED;
  const W3Geom g = w3_geom(H, W, Cin, Cout, taps, stride);
  const long long P = N * g.OH * g.OW;                      // P * Cout * 4 < 2^32
  const unsigned x_bytes = (unsigned)((unsigned long long)N * H * W * Cin * 4ULL);
  const W3Plan p = w3_plan(P, Cin, Cout, taps);
  const dim3 grid((unsigned)((p.units * p.ns + 3) / 4));
  float* part = (float*)workspace;
  if (p.va == 4)
    w3_launch<4>(p.vb, grid, st, x, dz, part, (int)P, g, x_bytes, p);
  else if (p.va == 2)
    w3_launch<2>(p.vb, grid, st, x, dz, part, (int)P, g, x_bytes, p);
  else
    w3_launch<1>(p.vb, grid, st, x, dz, part, (int)P, g, x_bytes, p);
  if (launch_status() != EQA_OK) return EQA_ERR_LAUNCH;
  const int n = taps * Cin * Cout;
  hipLaunchKernelGGL(conv3x3_wgrad_reduce, dim3((unsigned)((n + 63) / 64)), dim3(64 * kWgRedGroups), 0, st, part, dW, p.ns, taps, Cin, Cout);
  return launch_status();
}

int eqa_bn_res_act_fwd(const float* z, const float* scale, const float* shift, const float* res, int relu, float* y, int64_t npix, int C,
                       void* stream) {
  if (npix < 0 || C <= 0) return EQA_ERR_INVALID_ARG;
  if (npix == 0) return EQA_OK;
  if (!z || !scale || !shift || !y) return EQA_ERR_INVALID_ARG;
  if ((C & 3) || (((uintptr_t)z | (uintptr_t)y | (uintptr_t)res | (uintptr_t)scale | (uintptr_t)shift) & 15)) return EQA_ERR_UNSUPPORTED;
  const size_t nquad = (size_t)npix * (C >> 2);
  hipLaunchKernelGGL(bn_res_act_fwd_kernel, dim3(bra_stream_blocks(nquad)), dim3(kThreads), 0, (hipStream_t)stream, z, scale, shift, res,
                     relu, y, nquad, C >> 2);
  return launch_status();
}

int eqa_bn_res_act_bwd_reduce(const float* gy, const float* z, const float* scale, const float* shift, const float* res, int relu,
                              const float* mean, const float* rstd, double* partial, int64_t npix, int C, void* stream) {
  if (npix < 0 || C <= 0) return EQA_ERR_INVALID_ARG;
  if (npix == 0) return EQA_OK;
  if (!gy || !z || !scale || !shift || !mean || !rstd || !partial) return EQA_ERR_INVALID_ARG;
  if ((C & 3) || (((uintptr_t)gy | (uintptr_t)z | (uintptr_t)res | (uintptr_t)scale | (uintptr_t)shift | (uintptr_t)mean | (uintptr_t)rstd) & 15))
    return EQA_ERR_UNSUPPORTED;
  // as many partial rows as eqa_bn_act_bwd_finalize sums; the pixels dealt evenly over them
  const int64_t blocks = eqa_bn_act_partial_blocks(npix);
  const int per = (int)((npix + blocks - 1) / blocks);
  hipLaunchKernelGGL(bn_res_act_bwd_reduce_kernel, dim3((unsigned)blocks), dim3(kThreads), 0, (hipStream_t)stream, gy, z, scale, shift, res,
                     relu, mean, rstd, partial, (size_t)npix, C, per);
  return launch_status();
}

int eqa_bn_res_act_bwd_apply(const float* gy, const float* z, const float* scale, const float* shift, const float* res, int relu,
                             const float* mean, const float* rstd, const float* gscale, const float* m1, const float* m2, float* dz,
                             float* dres, int64_t npix, int C, void* stream) {
  if (npix < 0 || C <= 0) return EQA_ERR_INVALID_ARG;
  if (npix == 0) return EQA_OK;
  if (!gy || !z || !scale || !shift || !mean || !rstd || !gscale || !m1 || !m2 || !dz) return EQA_ERR_INVALID_ARG;
  if ((C & 3) || (((uintptr_t)gy | (uintptr_t)z | (uintptr_t)res | (uintptr_t)dz | (uintptr_t)dres | (uintptr_t)scale | (uintptr_t)shift |
                   (uintptr_t)mean | (uintptr_t)rstd | (uintptr_t)gscale | (uintptr_t)m1 | (uintptr_t)m2) & 15))
    return EQA_ERR_UNSUPPORTED;
  const size_t nquad = (size_t)npix * (C >> 2);
  hipLaunchKernelGGL(bn_res_act_bwd_apply_kernel, dim3(bra_stream_blocks(nquad)), dim3(kThreads), 0, (hipStream_t)stream, gy, z, scale, shift,
                     res, relu, mean, rstd, gscale, m1, m2, dz, dres, nquad, C >> 2);
  return launch_status();
}

}  // extern "C"
