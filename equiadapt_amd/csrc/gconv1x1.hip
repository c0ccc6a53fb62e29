// libeqa_hip.so, part 24 -- the 1 x 1 group convolutions of the wide-ResNet canonicalization network's bottleneck blocks
// (escnn_networks.py:261-285 of the reference: R2Conv(in, mid, 1) and R2Conv(out, in, 1) around the k x k layer, the `out += x`
// behind them, and -- :474-479 -- the InnerBatchNorm + ReLU that follow the block) on a channels-last map: one REAL GEMM over the
// pixels with everything that would otherwise be a pass of its own over the map in the epilogue,
//     z[p][o] = sum_c x[p][c] W[c][o] + bias[o] (+ res[p][o])
//     y[p][o] = relu ? max(s[o] z + t[o], 0) : s[o] z + t[o]                    (s, t NULL: identity)
// It is plane_gemm_kernel (planegemm.hip) with one plane: one wave per SIMD, no LDS, no barriers; every wave streams its MFMA
// operand fragments from global memory / L2 into registers one K-stage (16 channels) ahead through range-checked buffer loads;
// v_mfma_f32_32x32x2_f32 (f32 in, f32 accumulate: exact fmaf chains).  Fragments as there:
//   x fragment (the B operand, pixel = column j):   lane l = 32 h + j holds x[row j][16 s + 8 b + 4 h + t], t = 0..3
//   W fragment (the A operand, channel = row i):    lane l = 32 h + i holds W[16 s + 8 b + 4 h + t][col i]; the host packs W in
//       exactly this order (ops.pack_gconv1x1_weights), so a wave's W loads are contiguous 1 KB runs
// With the channels as accumulator ROWS a lane ends up with 4 consecutive output channels of one pixel per register group: the
// epilogue reads bias / s / t and the residual sixteen bytes at a time in that layout and stores sixteen bytes from the registers.
// Work: wave-tile = (64 pixels, 32 NT output channels), column tiles fastest, so the waves of a block share their 64 rows of x.
// Rows past P lie outside every descriptor of their tile: they load as zero and their stores are dropped.
// The filter and bias gradient (eqa_gconv1x1_wgrad: the contraction over the pixels, split over the chip's waves) stands behind the
// forward kernel with its own operand layout; the data gradient is the forward kernel on the packed transpose of W.
#include "eqa_common.hpp"

namespace {

typedef float f32x4 __attribute__((ext_vector_type(4)));
typedef float f32x16 __attribute__((ext_vector_type(16)));
typedef unsigned u32x4 __attribute__((ext_vector_type(4)));

constexpr int kMinCh = 32, kMaxCh = 512;       // channel counts eqa_gconv1x1_supported admits (multiples of 32)
constexpr unsigned long long kMaxBytes = 0xffffff00ULL;   // of x, res and y each: one 32-bit buffer range; tile and row counters are ints

template <int NT>
struct G1Ops {              // one K-stage of operands
  f32x4 v[2][2];            // [row subtile m][b]
  f32x4 u[NT][2];           // [column subtile n][b]
};

__device__ __forceinline__ f32x4 g1_ld(__amdgpu_buffer_rsrc_t r, unsigned voff, unsigned soff) {
  return __builtin_bit_cast(f32x4, __builtin_amdgcn_raw_buffer_load_b128(r, voff, soff, 0));
}

template <int NT>
__device__ __forceinline__ void g1_load(G1Ops<NT>& o, __amdgpu_buffer_rsrc_t rv, __amdgpu_buffer_rsrc_t ru, unsigned voff0, unsigned voff1,
                                        unsigned uoff, unsigned sv, unsigned su) {
#pragma unroll
  for (int b = 0; b < 2; ++b) {
    o.v[0][b] = g1_ld(rv, voff0 + 32 * b, sv);
    o.v[1][b] = g1_ld(rv, voff1 + 32 * b, sv);
#pragma unroll
    for (int n = 0; n < NT; ++n) o.u[n][b] = g1_ld(ru, uoff + (n * 2 + b) * 1024, su);
  }
}

template <int NT>
__device__ __forceinline__ void g1_mma(const G1Ops<NT>& o, f32x16 (&acc)[2][NT]) {
#pragma unroll
  for (int b = 0; b < 2; ++b)
#pragma unroll
    for (int t = 0; t < 4; ++t)
#pragma unroll
      for (int m = 0; m < 2; ++m)
#pragma unroll
        for (int n = 0; n < NT; ++n) acc[m][n] = __builtin_amdgcn_mfma_f32_32x32x2f32(o.u[n][b][t], o.v[m][b][t], acc[m][n], 0, 0, 0);
}

// x (P, Cin); Wpk (Cin/16, Cout/32, 2, 64, 4); bias, s, t (Cout); res, y (P, Cout)
template <int NT>
__global__ __launch_bounds__(256, 1) void gconv1x1_kernel(const float* __restrict__ x, const float* __restrict__ Wpk, const float* __restrict__ bias,
                                                          const float* __restrict__ res, const float* __restrict__ sc, const float* __restrict__ sh,
                                                          float* __restrict__ y, int relu, int P, int Cin, int Cout, int n_ct, int total,
                                                          int nwaves) {
  const int lane = threadIdx.x & 63;
  const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const int q = blockIdx.x * 4 + wave;                   // this wave's slot among the grid's waves
  if (q >= total) return;
  const int S = Cin / 16;
  const int j = lane & 31, h = lane >> 5;
  const unsigned u_stage_bytes = (unsigned)(Cout / 32) * 2 * 1024;  // bytes of one K-stage of Wpk
  const unsigned uoff = lane * 16;
  const __amdgpu_buffer_rsrc_t ru = __builtin_amdgcn_make_buffer_rsrc(const_cast<float*>(Wpk), 0, (unsigned)S * u_stage_bytes, 0x00020000);

  struct Tile {
    __amdgpu_buffer_rsrc_t rv;
    unsigned su;       // scalar byte offset of the tile's first column subtile inside a K-stage of Wpk
    int row0, ct;
  };
  auto locate = [&](int u) {
    Tile t;
    const int rt = u / n_ct;
    t.ct = u - rt * n_ct;
    t.row0 = rt * 64;
    const int rows = min(64, P - t.row0);
    // rows beyond P fall outside the descriptor: they read as zero (and their stores are dropped, below)
    t.rv = __builtin_amdgcn_make_buffer_rsrc(const_cast<float*>(x) + (size_t)t.row0 * Cin, 0, (unsigned)rows * (unsigned)Cin * 4u, 0x00020000);
    t.su = (unsigned)(t.ct * NT) * 2048u;
    return t;
  };
  const unsigned voff0 = (unsigned)(j * Cin + 4 * h) * 4u;          // this lane's row of the first 32-row subtile
  const unsigned voff1 = voff0 + 32u * (unsigned)Cin * 4u;

  Tile cur = locate(q);
  G1Ops<NT> s0, s1;
  g1_load<NT>(s0, cur.rv, ru, voff0, voff1, uoff, 0, cur.su);
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
    for (int s = 0; s < S; s += 2) {
      // the scheduling barriers keep the next stage's loads inside this stage's MFMA stream (see planegemm.hip)
      g1_load<NT>(s1, cur.rv, ru, voff0, voff1, uoff, (unsigned)(s + 1) * 64u, cur.su + (unsigned)(s + 1) * u_stage_bytes);
      __builtin_amdgcn_sched_barrier(0);
      g1_mma<NT>(s0, acc);
      __builtin_amdgcn_sched_barrier(0);
      const bool more = s + 2 < S;
      g1_load<NT>(s0, more ? cur.rv : nxt.rv, ru, voff0, voff1, uoff, more ? (unsigned)(s + 2) * 64u : 0u,
                  more ? cur.su + (unsigned)(s + 2) * u_stage_bytes : nxt.su);
      __builtin_amdgcn_sched_barrier(0);
      g1_mma<NT>(s1, acc);
      __builtin_amdgcn_sched_barrier(0);
    }
    // epilogue: accumulator register e of lane (h, j) is output channel (e & 3) + 8 (e >> 2) + 4 h of its 32-channel subtile, pixel
    // j of its 32-row subtile: register group g = e >> 2 is 16 contiguous bytes of y (and of res, bias, s, t)
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
        for (int g = 0; g < 4; ++g) {
          const int c = col0 + 32 * n + 8 * g + 4 * h;                 // < Cout, a multiple of 4
          const f32x4 bv = *reinterpret_cast<const f32x4*>(bias + c);
          f32x4 sv = {1.f, 1.f, 1.f, 1.f}, tv = {0.f, 0.f, 0.f, 0.f};
          if (sc) {
            sv = *reinterpret_cast<const f32x4*>(sc + c);
            tv = *reinterpret_cast<const f32x4*>(sh + c);
          }
#pragma unroll
          for (int m = 0; m < 2; ++m) {
            // (the row subtile's offset rides in the lane offset, which the range check certainly covers)
            const unsigned off = moff + (unsigned)(32 * n + 8 * g) * 4u + (unsigned)m * 32u * (unsigned)Cout * 4u;
            f32x4 v;
#pragma unroll
            for (int k = 0; k < 4; ++k) v[k] = acc[m][n][4 * g + k] + bv[k];
            if (res) {
              const f32x4 r = g1_ld(rr, off, 0);
#pragma unroll
              for (int k = 0; k < 4; ++k) v[k] += r[k];
            }
            if (sc) {
#pragma unroll
              for (int k = 0; k < 4; ++k) v[k] = sv[k] * v[k] + tv[k];
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

// -- filter and bias gradient ------------------------------------------------------------------------------------------------------
//     dW[c][o] = sum_p x[p][c] dz[p][o],   dbias[o] = sum_p dz[p][o]
// The contraction runs over the pixels, and both operands are pixel-major: a K-step of v_mfma_f32_32x32x2_f32 is a PAIR of pixel
// rows (k = h, the lane's half), and a lane's row / column index of the tile is free to stand for any channel.  So the fragments
// need no transpose: lane l = 32 h + i fetches V consecutive channels of pixel row 2 t + h with one 4 V-byte load (V = 4, 2, 1:
// the widest that divides the channel count into whole 32 V tiles), and component a of that load is the operand of the a-th
// 32-channel subtile, whose row i stands for channel c0 + V i + a:
//   x fragment  (the A operand, channel = row i):     lane 32 h + i holds x [r0 + 2 t + h][c0 + VA i + a], a = 0..VA-1
//   dz fragment (the B operand, channel = column j):  lane 32 h + j holds dz[r0 + 2 t + h][o0 + VB j + b], b = 0..VB-1
// One pair of loads feeds VA x VB matrix instructions; a wave's 32 lanes of a half read one contiguous 128 V-byte run of a row.
// Work: wave = (32 VA x 32 VB tile of dW, one contiguous range of L pixel rows); the pixel ranges split the contraction over the
// chip's waves (one per SIMD, up to 1024).  Every wave writes its partial tile -- and, the waves of the first tile row, the column
// sums of their dz range, added per lane on the vector ALU beside the matrix instructions -- to the workspace
// part[split][Cin + 1][Cout]; gconv1x1_wgrad_reduce adds the splits in a fixed order in fp64.  No atomics anywhere.
// Rows past a wave's range (and so past P) lie outside its two descriptors: they load as zero and add nothing.
typedef float f32x2 __attribute__((ext_vector_type(2)));
typedef unsigned u32x2 __attribute__((ext_vector_type(2)));

constexpr int kWgPairs = 4;        // pixel-row pairs per stage: 8 rows in flight per operand and buffer
constexpr int kWgWaves = 1024;     // one wave per SIMD
constexpr int kWgRedGroups = 16;   // waves of a reduce block: each adds every 16th split, wave 0 adds the sixteen

struct WgPlan {
  int va, vb;       // floats per lane and load of x, of dz
  int n_nt, tiles;  // column tiles; tiles of dW
  int L, ns;        // pixel rows per wave; splits
};

inline int wg_width(int C) { return C % 128 == 0 ? 4 : C % 64 == 0 ? 2 : 1; }

inline WgPlan wg_plan(long long P, int Cin, int Cout) {
  WgPlan p;
  p.va = wg_width(Cin);
  p.vb = wg_width(Cout);
  p.n_nt = Cout / (32 * p.vb);
  p.tiles = Cin / (32 * p.va) * p.n_nt;                            // <= 225
  const long long want = std::max(1, kWgWaves / p.tiles);
  const long long L = std::max<long long>(16, ((P + want - 1) / want + 15) / 16 * 16);
  p.L = (int)L;                                                    // P * 4 * 32 < 2^32
  p.ns = (int)std::max<long long>(1, (P + L - 1) / L);             // <= want
  return p;
}

template <int V>
__device__ __forceinline__ void wg_ld(float (&d)[V], __amdgpu_buffer_rsrc_t r, unsigned voff) {
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

template <int VA, int VB>
struct WgOps {              // one stage of operands
  float a[kWgPairs][VA];
  float b[kWgPairs][VB];
};

// (the whole offset rides in the lane offset, which the range check covers)
template <int VA, int VB>
__device__ __forceinline__ void wg_load(WgOps<VA, VB>& o, __amdgpu_buffer_rsrc_t ra, __amdgpu_buffer_rsrc_t rb, unsigned aoff, unsigned boff,
                                        unsigned apair, unsigned bpair) {
#pragma unroll
  for (int t = 0; t < kWgPairs; ++t) {
    wg_ld<VA>(o.a[t], ra, aoff + (unsigned)t * apair);
    wg_ld<VB>(o.b[t], rb, boff + (unsigned)t * bpair);
  }
}

template <int VA, int VB>
__device__ __forceinline__ void wg_mma(const WgOps<VA, VB>& o, f32x16 (&acc)[VA][VB], float (&bs)[VB]) {
#pragma unroll
  for (int t = 0; t < kWgPairs; ++t) {
#pragma unroll
    for (int a = 0; a < VA; ++a)
#pragma unroll
      for (int b = 0; b < VB; ++b) acc[a][b] = __builtin_amdgcn_mfma_f32_32x32x2f32(o.a[t][a], o.b[t][b], acc[a][b], 0, 0, 0);
#pragma unroll
    for (int b = 0; b < VB; ++b) bs[b] += o.b[t][b];
  }
}

// x (P, Cin); dz (P, Cout); part (ns, Cin + 1, Cout): row Cin of a split holds its column sums of dz
template <int VA, int VB>
__global__ __launch_bounds__(256, 1) void gconv1x1_wgrad_kernel(const float* __restrict__ x, const float* __restrict__ dz, float* __restrict__ part,
                                                                int P, int Cin, int Cout, int n_nt, int tiles, int total, int L) {
  const int lane = threadIdx.x & 63;
  const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const int q = blockIdx.x * 4 + wave;                   // tiles fastest: the waves of a block share their pixel rows
  if (q >= total) return;
  const int split = q / tiles, tile = q - split * tiles;
  const int mt = tile / n_nt, nt = tile - mt * n_nt;
  const int c0 = mt * 32 * VA, o0 = nt * 32 * VB;
  const int r0 = split * L;
  const int rows = min(L, P - r0);                       // >= 1: ns = ceil(P / L)
  const int i = lane & 31, h = lane >> 5;
  const __amdgpu_buffer_rsrc_t ra =
      __builtin_amdgcn_make_buffer_rsrc(const_cast<float*>(x) + (size_t)r0 * Cin, 0, (unsigned)rows * (unsigned)Cin * 4u, 0x00020000);
  const __amdgpu_buffer_rsrc_t rb =
      __builtin_amdgcn_make_buffer_rsrc(const_cast<float*>(dz) + (size_t)r0 * Cout, 0, (unsigned)rows * (unsigned)Cout * 4u, 0x00020000);
  const unsigned apair = 2u * (unsigned)Cin * 4u, bpair = 2u * (unsigned)Cout * 4u;        // bytes from one pair of rows to the next
  unsigned aoff = (unsigned)(h * Cin + c0 + VA * i) * 4u;
  unsigned boff = (unsigned)(h * Cout + o0 + VB * i) * 4u;

  f32x16 acc[VA][VB];
  float bs[VB];
#pragma unroll
  for (int b = 0; b < VB; ++b) {
    bs[b] = 0.f;
#pragma unroll
    for (int a = 0; a < VA; ++a)
#pragma unroll
      for (int e = 0; e < 16; ++e) acc[a][b][e] = 0.f;
  }
  WgOps<VA, VB> s0, s1;
  wg_load<VA, VB>(s0, ra, rb, aoff, boff, apair, bpair);
  const int stages = (rows + 2 * kWgPairs - 1) / (2 * kWgPairs);
  // two stages per trip, each loaded under the other's matrix instructions; a stage past the range loads zeros (at most
  // (L + 16) rows of 2 KB from the descriptor's base: the offsets stay far inside 32 bits)
  for (int s = 0; s < stages; s += 2) {
    aoff += kWgPairs * apair;
    boff += kWgPairs * bpair;
    wg_load<VA, VB>(s1, ra, rb, aoff, boff, apair, bpair);
    __builtin_amdgcn_sched_barrier(0);
    wg_mma<VA, VB>(s0, acc, bs);
    __builtin_amdgcn_sched_barrier(0);
    aoff += kWgPairs * apair;
    boff += kWgPairs * bpair;
    wg_load<VA, VB>(s0, ra, rb, aoff, boff, apair, bpair);
    __builtin_amdgcn_sched_barrier(0);
    wg_mma<VA, VB>(s1, acc, bs);
    __builtin_amdgcn_sched_barrier(0);
  }
  // accumulator register e of lane (h, j) of subtile (a, b) is row (e & 3) + 8 (e >> 2) + 4 h, column j: channel pair
  // (c0 + VA row + a, o0 + VB j + b) -- the VB subtiles of a lane are 4 VB contiguous bytes of a row of the partial tile
  float* const pt = part + (size_t)split * (size_t)(Cin + 1) * Cout;
#pragma unroll
  for (int a = 0; a < VA; ++a)
#pragma unroll
    for (int e = 0; e < 16; ++e) {
      const int row = (e & 3) + 8 * (e >> 2) + 4 * h;
      float* const dst = pt + (size_t)(c0 + VA * row + a) * Cout + o0 + VB * i;
      if constexpr (VB == 4) {
        *reinterpret_cast<f32x4*>(dst) = f32x4{acc[a][0][e], acc[a][1][e], acc[a][2][e], acc[a][3][e]};
      } else if constexpr (VB == 2) {
        *reinterpret_cast<f32x2*>(dst) = f32x2{acc[a][0][e], acc[a][1][e]};
      } else {
        *dst = acc[a][0][e];
      }
    }
  if (mt == 0) {                                          // (wave-uniform) even rows + odd rows of the range, in that order
#pragma unroll
    for (int b = 0; b < VB; ++b) {
      const float other = __shfl_xor(bs[b], 32);
      if (h == 0) pt[(size_t)Cin * Cout + o0 + VB * i + b] = bs[b] + other;
    }
  }
}

// part (ns, n) with n = (Cin + 1) Cout -> dW (Cout, Cin), dbias (Cout).  Block = 64 consecutive entries x 16 waves: wave g adds the
// splits g, g + 16, ... of its entries in fp64, wave 0 adds the sixteen sums in order.
__global__ __launch_bounds__(64 * kWgRedGroups) void gconv1x1_wgrad_reduce(const float* __restrict__ part, float* __restrict__ dW,
                                                                          float* __restrict__ dbias, int ns, int Cin, int Cout) {
  __shared__ double sm[kWgRedGroups][64];
  const int lane = threadIdx.x & 63, g = threadIdx.x >> 6;
  const int n = (Cin + 1) * Cout;
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
  const int c = e / Cout, o = e - c * Cout;
  if (c < Cin)
    dW[(size_t)o * Cin + c] = (float)t;
  else
    dbias[o] = (float)t;
}

template <int VA>
void wg_launch(int vb, dim3 grid, hipStream_t st, const float* x, const float* dz, float* part, int P, int Cin, int Cout, const WgPlan& p) {
  const int total = p.tiles * p.ns;
  if (vb == 4)
    hipLaunchKernelGGL((gconv1x1_wgrad_kernel<VA, 4>), grid, dim3(256), 0, st, x, dz, part, P, Cin, Cout, p.n_nt, p.tiles, total, p.L);
  else if (vb == 2)
    hipLaunchKernelGGL((gconv1x1_wgrad_kernel<VA, 2>), grid, dim3(256), 0, st, x, dz, part, P, Cin, Cout, p.n_nt, p.tiles, total, p.L);
  else
    hipLaunchKernelGGL((gconv1x1_wgrad_kernel<VA, 1>), grid, dim3(256), 0, st, x, dz, part, P, Cin, Cout, p.n_nt, p.tiles, total, p.L);
}

}  // namespace

extern "C" {

int eqa_gconv1x1_wgrad_supported(long long P, int Cin, int Cout) { return eqa_gconv1x1_supported(P, Cin, Cout); }

long long eqa_gconv1x1_wgrad_workspace_bytes(long long P, int Cin, int Cout) {
  if (!eqa_gconv1x1_supported(P, Cin, Cout) || P == 0) return 0;
  return (long long)wg_plan(P, Cin, Cout).ns * (Cin + 1) * Cout * 4LL;
}

int eqa_gconv1x1_wgrad(const float* x, const float* dz, float* dW, float* dbias, void* workspace, long long P, int Cin, int Cout,
                       void* stream) {
  if (P < 0 || Cin <= 0 || Cout <= 0) return EQA_ERR_INVALID_ARG;
  if (!eqa_gconv1x1_supported(P, Cin, Cout)) return EQA_ERR_UNSUPPORTED;
  if (!dW || !dbias || (const float*)dW == x || (const float*)dW == dz || (const float*)dbias == x || (const float*)dbias == dz || dW == dbias)
    return EQA_ERR_INVALID_ARG;
  hipStream_t st = (hipStream_t)stream;
  if (P == 0) {
    if (hipMemsetAsync(dW, 0, (size_t)Cin * Cout * 4, st) != hipSuccess || hipMemsetAsync(dbias, 0, (size_t)Cout * 4, st) != hipSuccess)
      return EQA_ERR_LAUNCH;
    return EQA_OK;
  }
  if (!x || !dz || !workspace || workspace == (void*)x || workspace == (void*)dz || workspace == (void*)dW || workspace == (void*)dbias)
    return EQA_ERR_INVALID_ARG;
  if ((((uintptr_t)x | (uintptr_t)dz | (uintptr_t)dW | (uintptr_t)dbias | (uintptr_t)workspace) & 15)) return EQA_ERR_UNSUPPORTED;
  const WgPlan p = wg_plan(P, Cin, Cout);
  const dim3 grid((unsigned)((p.tiles * p.ns + 3) / 4));
  float* part = (float*)workspace;
  if (p.va == 4)
    wg_launch<4>(p.vb, grid, st, x, dz, part, (int)P, Cin, Cout, p);
  else if (p.va == 2)
    wg_launch<2>(p.vb, grid, st, x, dz, part, (int)P, Cin, Cout, p);
  else
    wg_launch<1>(p.vb, grid, st, x, dz, part, (int)P, Cin, Cout, p);
  if (launch_status() != EQA_OK) return EQA_ERR_LAUNCH;
  const int n = (Cin + 1) * Cout;
  hipLaunchKernelGGL(gconv1x1_wgrad_reduce, dim3((unsigned)((n + 63) / 64)), dim3(64 * kWgRedGroups), 0, st, part, dW, dbias, p.ns, Cin, Cout);
  return launch_status();
}

int eqa_gconv1x1_supported(long long P, int Cin, int Cout) {
  if (P < 0 || Cin < kMinCh || Cout < kMinCh || Cin > kMaxCh || Cout > kMaxCh || Cin % 32 || Cout % 32) return 0;
  return (unsigned long long)P * (unsigned long long)std::max(Cin, Cout) * 4ULL <= kMaxBytes;
}

int eqa_gconv1x1_nhwc(const float* x, const float* Wpk, const float* bias, const float* res, const float* s, const float* t, int relu,
                      float* y, long long P, int Cin, int Cout, void* stream) {
  if (P < 0 || Cin <= 0 || Cout <= 0) return EQA_ERR_INVALID_ARG;
  if (!eqa_gconv1x1_supported(P, Cin, Cout)) return EQA_ERR_UNSUPPORTED;
  if (P == 0) return EQA_OK;
  if (!x || !Wpk || !bias || !y || (s == nullptr) != (t == nullptr)) return EQA_ERR_INVALID_ARG;
  if (y == x || y == res) return EQA_ERR_INVALID_ARG;
  if ((((uintptr_t)x | (uintptr_t)Wpk | (uintptr_t)bias | (uintptr_t)res | (uintptr_t)s | (uintptr_t)t | (uintptr_t)y) & 15)) return EQA_ERR_UNSUPPORTED;
  const int NT = Cout % 64 == 0 ? 2 : 1;
  const long long n_rt = (P + 63) / 64;
  const int n_ct = Cout / (32 * NT);
  const long long total = n_rt * n_ct;                      // < 2^31: P * Cout * 4 < 2^32
  // persistent waves: one per SIMD, 1024 on the chip; fewer when there is less work
  const int nwaves = (int)std::min<long long>(1024, (total + 3) / 4 * 4);
  const dim3 grid((unsigned)(nwaves / 4));
  hipStream_t st = (hipStream_t)stream;
  if (NT == 2)
    hipLaunchKernelGGL(gconv1x1_kernel<2>, grid, dim3(256), 0, st, x, Wpk, bias, res, s, t, y, relu, (int)P, Cin, Cout, n_ct, (int)total, nwaves);
  else
    hipLaunchKernelGGL(gconv1x1_kernel<1>, grid, dim3(256), 0, st, x, Wpk, bias, res, s, t, y, relu, (int)P, Cin, Cout, n_ct, (int)total, nwaves);
  return launch_status();
}

}  // extern "C"
