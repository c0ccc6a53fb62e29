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

}  // namespace

extern "C" {

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
