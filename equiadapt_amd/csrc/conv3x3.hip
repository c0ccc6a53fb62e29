// libeqa_hip.so, part 26 -- the dense 3 x 3 convolutions (and the 1 x 1 stride-2 shortcuts) of ResNet18Network's basic blocks
// (custom_nonequivariant_networks.py:83-130 of the reference: torchvision's resnet18 behind the stem) on a channels-last fp32 map,
// with the block's glue in the epilogue:
//     z[n][oy][ox][o] = sum_{dy,dx,c} x[n][s oy + dy - pad][s ox + dx - pad][c] W[o][c][dy][dx] + bias[o] (+ res[n][oy][ox][o])
//     y = relu ? max(z, 0) : z                        taps = 9: 3 x 3, pad 1;  taps = 1: 1 x 1, pad 0;  stride s in {1, 2}
// It is gconv1x1_kernel (gconv1x1.hip) with a K loop of taps x Cin/16 stages instead of Cin/16: one wave per SIMD, no LDS, no
// barriers; every wave streams its MFMA operand fragments from global memory / L2 into registers one K-stage (16 channels of one
// tap) ahead through range-checked buffer loads; v_mfma_f32_32x32x2_f32 (f32 in, f32 accumulate: exact fmaf chains, taps outermost,
// channels inside, in a fixed order).  Fragments as there:
//   x fragment (the B operand, output pixel = column j):  lane l = 32 h + j holds x[neighbour (dy, dx) of pixel j][16 s + 8 b + 4 h + t]
//   W fragment (the A operand, output channel = row i):   lane l = 32 h + i holds W[col i][16 s + 8 b + 4 h + t][dy][dx]; the host
//       packs W in exactly this order, tap-major (ops.pack_conv3x3_weights), so a wave's W loads are contiguous 1 KB runs
// A lane's output pixel p = row0 + 32 m + j is decomposed ONCE per tile into (n, oy, ox); a tap is then a per-lane byte offset of the
// neighbour's row in ONE descriptor over the whole of x.  A tap on the zero padding -- and every tap of a row past P -- gets the lane
// offset kOob, which by itself lies at or past the descriptor's size (the admitted maps end at or below it): the lane's load is
// dropped and returns zero, whatever the scalar stage offset.  A tile may span several images: a border pixel's neighbour in memory
// belongs to the adjacent image, and the padding test (on iy, ix of the lane's own image) is what keeps it out.
// Work: wave-tile = (64 output pixels, 32 NT output channels), column tiles fastest, so the waves of a block share their rows of x.
// Rows past P are never stored (they lie outside the tile's y descriptor).  No atomics: two launches give the same bits.
// The data gradient (eqa_conv3x3_dgrad) is a mode of the same kernel over dz with another tap-offset function; the filter gradient
// stands in conv3x3_train.hip.
#include "eqa_common.hpp"

namespace {

typedef float f32x4 __attribute__((ext_vector_type(4)));
typedef float f32x16 __attribute__((ext_vector_type(16)));
typedef unsigned u32x4 __attribute__((ext_vector_type(4)));

constexpr int kMinCh = 32, kMaxCh = 512;                  // channel counts eqa_conv3x3_supported admits (multiples of 32)
constexpr unsigned long long kMaxBytes = 0xffffff00ULL;   // of x, res and y each: one 32-bit buffer range; tile and row counters are ints
constexpr unsigned kOob = 0xffffff00u;                    // a lane offset no admitted descriptor covers (+ 48 does not wrap)

template <int NT>
struct C3Ops {              // one K-stage of operands
  f32x4 v[2][2];            // [row subtile m][b]
  f32x4 u[NT][2];           // [column subtile n][b]
};

__device__ __forceinline__ f32x4 c3_ld(__amdgpu_buffer_rsrc_t r, unsigned voff, unsigned soff) {
  return __builtin_bit_cast(f32x4, __builtin_amdgcn_raw_buffer_load_b128(r, voff, soff, 0));
}

template <int NT>
__device__ __forceinline__ void c3_load(C3Ops<NT>& o, __amdgpu_buffer_rsrc_t rv, __amdgpu_buffer_rsrc_t ru, unsigned voff0, unsigned voff1,
                                        unsigned uoff, unsigned sv, unsigned su) {
#pragma unroll
  for (int b = 0; b < 2; ++b) {
    o.v[0][b] = c3_ld(rv, voff0 + 32 * b, sv);
    o.v[1][b] = c3_ld(rv, voff1 + 32 * b, sv);
#pragma unroll
    for (int n = 0; n < NT; ++n) o.u[n][b] = c3_ld(ru, uoff + (n * 2 + b) * 1024, su);
  }
}

template <int NT>
__device__ __forceinline__ void c3_mma(const C3Ops<NT>& o, f32x16 (&acc)[2][NT]) {
#pragma unroll
  for (int b = 0; b < 2; ++b)
#pragma unroll
    for (int t = 0; t < 4; ++t)
#pragma unroll
      for (int m = 0; m < 2; ++m)
#pragma unroll
        for (int n = 0; n < NT; ++n) acc[m][n] = __builtin_amdgcn_mfma_f32_32x32x2f32(o.u[n][b][t], o.v[m][b][t], acc[m][n], 0, 0, 0);
}

struct C3Geom {
  int H, W, OH, OW, Cin, Cout, stride, pad, ksz;   // ksz: 3 or 1 (taps = ksz * ksz)
};

// x (N, H, W, Cin); Wpk (taps, Cin/16, Cout/32, 2, 64, 4); bias (Cout); res, y (P = N OH OW, Cout)
// DG, the data gradient (eqa_conv3x3_dgrad): the same walk with the roles exchanged -- "x" is dz, "y" is dx, Wpk the flipped and
// transposed pack, g.H x g.W the map that is READ (dz's), g.OH x g.OW the one that is written (dx's), no bias.  Tap (dy, dx) of
// output pixel (iy, ix) reads dz at ((iy + dy - pad) / s, (ix + dx - pad) / s) where both divide and the quotients are inside; every
// other tap -- three in four at stride 2 -- takes kOob like a tap on the padding.
template <int NT, bool DG>
__global__ __launch_bounds__(256, 1) void conv3x3_kernel(const float* __restrict__ x, const float* __restrict__ Wpk, const float* __restrict__ bias,
                                                         const float* __restrict__ res, float* __restrict__ y, int relu, int P, C3Geom g,
                                                         unsigned x_bytes, int n_ct, int total, int nwaves) {
  const int lane = threadIdx.x & 63;
  const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const int q = blockIdx.x * 4 + wave;                   // this wave's slot among the grid's waves
  if (q >= total) return;
  const int Cin = g.Cin, Cout = g.Cout;
  const int S = Cin / 16;                                // even: Cin is a multiple of 32
  const int taps = g.ksz * g.ksz;
  const int j = lane & 31, h = lane >> 5;
  const unsigned u_stage_bytes = (unsigned)(Cout / 32) * 2 * 1024;  // bytes of one K-stage of Wpk
  const unsigned uoff = lane * 16;
  const __amdgpu_buffer_rsrc_t ru =
      __builtin_amdgcn_make_buffer_rsrc(const_cast<float*>(Wpk), 0, (unsigned)(taps * S) * u_stage_bytes, 0x00020000);
  const __amdgpu_buffer_rsrc_t rx = __builtin_amdgcn_make_buffer_rsrc(const_cast<float*>(x), 0, x_bytes, 0x00020000);
  const unsigned opix = (unsigned)(g.OH * g.OW);

  struct Tile {
    unsigned su;        // scalar byte offset of the tile's first column subtile inside a K-stage of Wpk
    int row0, ct;
    // per lane and row subtile m: the byte offset of tap (0, 0)'s channels 4 h .. 4 h + 3 (it wraps below zero on the top / left
    // border, where it is not used) and that tap's input row and column; a row past P has iy0 = -4: no tap is inside
    unsigned base[2];
    int iy0[2], ix0[2];
  };
  auto locate = [&](int u) {
    Tile t;
    const int rt = u / n_ct;
    t.ct = u - rt * n_ct;
    t.row0 = rt * 64;
    t.su = (unsigned)(t.ct * NT) * 2048u;
#pragma unroll
    for (int m = 0; m < 2; ++m) {
      const unsigned p = (unsigned)(t.row0 + 32 * m + j);
      const unsigned n = p / opix, r = p - n * opix;
      const unsigned oy = r / (unsigned)g.OW, ox = r - oy * (unsigned)g.OW;
      const int iy0 = (int)oy * (DG ? 1 : g.stride) - g.pad, ix0 = (int)ox * (DG ? 1 : g.stride) - g.pad;
      t.iy0[m] = p < (unsigned)P ? iy0 : -4;
      t.ix0[m] = ix0;
      if constexpr (DG)       // the image's first pixel: the neighbour's own row and column come with the tap
        t.base[m] = (unsigned)((int)n * g.H * g.W) * (unsigned)Cin * 4u + 16u * (unsigned)h;
      else
        t.base[m] = (unsigned)(((int)n * g.H + iy0) * g.W + ix0) * (unsigned)Cin * 4u + 16u * (unsigned)h;
    }
    return t;
  };
  // this lane's offsets of one tap: the neighbour's row where it is inside the lane's own image, kOob on the padding
  auto tap_off = [&](const Tile& t, int tap, unsigned& v0, unsigned& v1) {
    const int dy = tap / g.ksz, dx = tap - dy * g.ksz;
    if constexpr (DG) {
      const int sh = g.stride - 1, lo = g.stride - 1;      // stride 1 or 2: the quotient is a shift, the remainder a mask
#pragma unroll
      for (int m = 0; m < 2; ++m) {
        const int ty = t.iy0[m] + dy, tx = t.ix0[m] + dx;  // (a negative one fails the unsigned comparison)
        const bool in = !((ty | tx) & lo) && (unsigned)ty < (unsigned)(g.H << sh) && (unsigned)tx < (unsigned)(g.W << sh);
        const unsigned off = t.base[m] + (unsigned)(((ty >> sh) * g.W + (tx >> sh)) * Cin) * 4u;
        (m == 0 ? v0 : v1) = in ? off : kOob;
      }
      return;
    }
    const unsigned d = (unsigned)((dy * g.W + dx) * Cin) * 4u;
    const bool in0 = (unsigned)(t.iy0[0] + dy) < (unsigned)g.H && (unsigned)(t.ix0[0] + dx) < (unsigned)g.W;
    const bool in1 = (unsigned)(t.iy0[1] + dy) < (unsigned)g.H && (unsigned)(t.ix0[1] + dx) < (unsigned)g.W;
    v0 = in0 ? t.base[0] + d : kOob;
    v1 = in1 ? t.base[1] + d : kOob;
  };

  Tile cur = locate(q);
  unsigned voff0, voff1;
  tap_off(cur, 0, voff0, voff1);
  C3Ops<NT> s0, s1;
  c3_load<NT>(s0, rx, ru, voff0, voff1, uoff, 0, cur.su);
  for (int u = q; u < total; u += nwaves) {
    f32x16 acc[2][NT];
#pragma unroll
    for (int m = 0; m < 2; ++m)
#pragma unroll
      for (int n = 0; n < NT; ++n)
#pragma unroll
        for (int e = 0; e < 16; ++e) acc[m][n][e] = 0.f;
    // the tile after this one (or this one again when it is the last: a harmless reload instead of a conditional load)
    const Tile nxt = locate(u + nwaves < total ? u + nwaves : u);
    unsigned su = cur.su;                                // of the stage in s0: (tap, s)
    for (int tap = 0; tap < taps; ++tap) {
      for (int s = 0; s < S; s += 2) {
        // the scheduling barriers keep the next stage's loads inside this stage's MFMA stream (see planegemm.hip).  S is even: the
        // second stage of a trip is always of the same tap as the first
        c3_load<NT>(s1, rx, ru, voff0, voff1, uoff, (unsigned)(s + 1) * 64u, su + u_stage_bytes);
        __builtin_amdgcn_sched_barrier(0);
        c3_mma<NT>(s0, acc);
        __builtin_amdgcn_sched_barrier(0);
        su += 2 * u_stage_bytes;
        unsigned sv = (unsigned)(s + 2) * 64u;
        if (s + 2 >= S) {                                // (wave-uniform) the next tap, or tap 0 of the next tile
          sv = 0;
          if (tap + 1 < taps) {
            tap_off(cur, tap + 1, voff0, voff1);
          } else {
            tap_off(nxt, 0, voff0, voff1);
            su = nxt.su;
          }
        }
        c3_load<NT>(s0, rx, ru, voff0, voff1, uoff, sv, su);
        __builtin_amdgcn_sched_barrier(0);
        c3_mma<NT>(s1, acc);
        __builtin_amdgcn_sched_barrier(0);
      }
    }
    // epilogue: accumulator register e of lane (h, j) is output channel (e & 3) + 8 (e >> 2) + 4 h of its 32-channel subtile, pixel
    // j of its 32-row subtile: register group e >> 2 is 16 contiguous bytes of y (and of res, bias)
    {
      const int rows = min(64, P - cur.row0);
      const int col0 = cur.ct * (32 * NT);
      const size_t base = (size_t)cur.row0 * Cout + col0;
      const unsigned bytes = (unsigned)(((size_t)(rows - 1) * Cout + Cout - col0) * 4);
      const __amdgpu_buffer_rsrc_t ry = __builtin_amdgcn_make_buffer_rsrc(y + base, 0, bytes, 0x00020000);
      // (without a residual the descriptor covers nothing: the loads below are not issued either)
      const __amdgpu_buffer_rsrc_t rr = __builtin_amdgcn_make_buffer_rsrc(const_cast<float*>(res ? res + base : x), 0, res ? bytes : 0u, 0x00020000);
      const unsigned moff = (unsigned)(j * Cout + 4 * h) * 4u;
#pragma unroll
      for (int n = 0; n < NT; ++n)
#pragma unroll
        for (int gq = 0; gq < 4; ++gq) {
          const int c = col0 + 32 * n + 8 * gq + 4 * h;                // < Cout, a multiple of 4
          f32x4 bv = {0.f, 0.f, 0.f, 0.f};
          if constexpr (!DG) bv = *reinterpret_cast<const f32x4*>(bias + c);
#pragma unroll
          for (int m = 0; m < 2; ++m) {
            // (the row subtile's offset rides in the lane offset, which the range check certainly covers)
            const unsigned off = moff + (unsigned)(32 * n + 8 * gq) * 4u + (unsigned)m * 32u * (unsigned)Cout * 4u;
            f32x4 v;
#pragma unroll
            for (int k = 0; k < 4; ++k) v[k] = acc[m][n][4 * gq + k] + bv[k];
            if (res) {
              const f32x4 r = c3_ld(rr, off, 0);
#pragma unroll
              for (int k = 0; k < 4; ++k) v[k] += r[k];
            }
            if (relu) {
#pragma unroll
              for (int k = 0; k < 4; ++k) v[k] = fmaxf(v[k], 0.f);
            }
            __builtin_amdgcn_raw_buffer_store_b128(__builtin_bit_cast(u32x4, v), ry, off, 0, 0);
          }
        }
    }
    cur = nxt;
  }
}

// output size of one axis, or 0 where the filter does not fit
inline long long c3_out(int n, int k, int pad, int stride) { return n + 2 * pad < k ? 0 : (n + 2 * pad - k) / stride + 1; }

}  // namespace

extern "C" {

int eqa_conv3x3_supported(long long N, int H, int W, int Cin, int Cout, int taps, int stride) {
  if (N < 0 || H <= 0 || W <= 0 || Cin < kMinCh || Cout < kMinCh || Cin > kMaxCh || Cout > kMaxCh || Cin % 32 || Cout % 32) return 0;
  if (!(taps == 9 || taps == 1) || !(stride == 1 || stride == 2) || (taps == 1 && stride != 2)) return 0;
  const int k = taps == 9 ? 3 : 1, pad = taps == 9 ? 1 : 0;
  const long long OH = c3_out(H, k, pad, stride), OW = c3_out(W, k, pad, stride);
  if (OH < 1 || OW < 1) return 0;
  // (H, W < 2^31 and N < 2^63 / 2^62: compare by division, nothing overflows)
  const unsigned long long in_px = (unsigned long long)H * (unsigned long long)W, out_px = (unsigned long long)OH * (unsigned long long)OW;
  const unsigned long long lim_in = kMaxBytes / (4ULL * (unsigned long long)Cin), lim_out = kMaxBytes / (4ULL * (unsigned long long)Cout);
  if (in_px > lim_in || out_px > lim_out) return 0;
  if (N > 0 && ((unsigned long long)N > lim_in / in_px || (unsigned long long)N > lim_out / out_px)) return 0;
  return 1;
}

int eqa_conv3x3_nhwc(const float* x, const float* Wpk, const float* bias, const float* res, int relu, float* y, long long N, int H, int W,
                     int Cin, int Cout, int taps, int stride, void* stream) {
  if (N < 0 || H <= 0 || W <= 0 || Cin <= 0 || Cout <= 0) return EQA_ERR_INVALID_ARG;
  if (!eqa_conv3x3_supported(N, H, W, Cin, Cout, taps, stride)) return EQA_ERR_UNSUPPORTED;
  if (N == 0) return EQA_OK;
  if (!x || !Wpk || !bias || !y) return EQA_ERR_INVALID_ARG;
  if (y == x || y == res) return EQA_ERR_INVALID_ARG;
  if ((((uintptr_t)x | (uintptr_t)Wpk | (uintptr_t)bias | (uintptr_t)res | (uintptr_t)y) & 15)) return EQA_ERR_UNSUPPORTED;
  C3Geom g;
  g.ksz = taps == 9 ? 3 : 1;
  g.pad = taps == 9 ? 1 : 0;
  g.H = H, g.W = W, g.Cin = Cin, g.Cout = Cout, g.stride = stride;
  g.OH = (int)c3_out(H, g.ksz, g.pad, stride);
  g.OW = (int)c3_out(W, g.ksz, g.pad, stride);
  const long long P = N * g.OH * g.OW;                      // P * Cout * 4 < 2^32
  const unsigned x_bytes = (unsigned)((unsigned long long)N * H * W * Cin * 4ULL);
  const int NT = Cout % 64 == 0 ? 2 : 1;
  const long long n_rt = (P + 63) / 64;
  const int n_ct = Cout / (32 * NT);
  const long long total = n_rt * n_ct;                      // < 2^31
  // persistent waves: one per SIMD, 1024 on the chip; fewer when there is less work
  const int nwaves = (int)std::min<long long>(1024, (total + 3) / 4 * 4);
  const dim3 grid((unsigned)(nwaves / 4));
  hipStream_t st = (hipStream_t)stream;
  if (NT == 2)
    hipLaunchKernelGGL((conv3x3_kernel<2, false>), grid, dim3(256), 0, st, x, Wpk, bias, res, y, relu, (int)P, g, x_bytes, n_ct, (int)total, nwaves);
  else
    hipLaunchKernelGGL((conv3x3_kernel<1, false>), grid, dim3(256), 0, st, x, Wpk, bias, res, y, relu, (int)P, g, x_bytes, n_ct, (int)total, nwaves);
  return launch_status();
}

int eqa_conv3x3_dgrad_supported(long long N, int H, int W, int Cin, int Cout, int taps, int stride) {
  return eqa_conv3x3_supported(N, H, W, Cin, Cout, taps, stride);      // dx is x's size, dz is y's
}

int eqa_conv3x3_dgrad(const float* dz, const float* Wdpk, const float* res, float* dx, long long N, int H, int W, int Cin, int Cout, int taps,
                      int stride, void* stream) {
  if (N < 0 || H <= 0 || W <= 0 || Cin <= 0 || Cout <= 0) return EQA_ERR_INVALID_ARG;
  if (!eqa_conv3x3_supported(N, H, W, Cin, Cout, taps, stride)) return EQA_ERR_UNSUPPORTED;
  if (N == 0) return EQA_OK;
  if (!dz || !Wdpk || !dx) return EQA_ERR_INVALID_ARG;
  if (dx == dz || dx == res) return EQA_ERR_INVALID_ARG;
  if ((((uintptr_t)dz | (uintptr_t)Wdpk | (uintptr_t)res | (uintptr_t)dx) & 15)) return EQA_ERR_UNSUPPORTED;
  C3Geom g;                                                 // the kernel's roles: it reads dz (Cout channels), writes dx (Cin)
  g.ksz = taps == 9 ? 3 : 1;
  g.pad = taps == 9 ? 1 : 0;
  g.H = (int)c3_out(H, g.ksz, g.pad, stride);
  g.W = (int)c3_out(W, g.ksz, g.pad, stride);
  g.OH = H, g.OW = W, g.Cin = Cout, g.Cout = Cin, g.stride = stride;
  const long long P = N * H * W;                            // P * Cin * 4 < 2^32
  const unsigned dz_bytes = (unsigned)((unsigned long long)N * g.H * g.W * Cout * 4ULL);
  const int NT = Cin % 64 == 0 ? 2 : 1;
  const long long n_rt = (P + 63) / 64;
  const int n_ct = Cin / (32 * NT);
  const long long total = n_rt * n_ct;                      // < 2^31
  const int nwaves = (int)std::min<long long>(1024, (total + 3) / 4 * 4);
  const dim3 grid((unsigned)(nwaves / 4));
  hipStream_t st = (hipStream_t)stream;
  if (NT == 2)
    hipLaunchKernelGGL((conv3x3_kernel<2, true>), grid, dim3(256), 0, st, dz, Wdpk, nullptr, res, dx, 0, (int)P, g, dz_bytes, n_ct, (int)total, nwaves);
  else
    hipLaunchKernelGGL((conv3x3_kernel<1, true>), grid, dim3(256), 0, st, dz, Wdpk, nullptr, res, dx, 0, (int)P, g, dz_bytes, n_ct, (int)total, nwaves);
  return launch_status();
}

}  // extern "C"
