// libeqa_hip.so, part 10c -- the channel contraction of the FFT convolution for channel counts that are multiples of 16 but not of
// what cgemm3m.hip takes (Cin % 32, Cout % 64): 144 = 16 fields x 9 of the steerable network's hidden layers, 288, 48, 80, ...
// C ABI: include/eqa_hip.h.  The arithmetic, the operand path and the epilogue are those of fft_cgemm3m_kernel (cgemm3m.hip: read
// its header first):
//     T1 = Ar.Br    T2 = Ai.Bi    T3 = (Ar + Ai).(Br + Bi)          Cr = T1 - T2    Ci = T3 - T1 - T2
// on v_mfma_f32_32x32x2_f32 with fp32 accumulation, operands straight from global memory / L2 into registers through buffer
// descriptors one K-stage ahead, a finished tile parked in LDS and flushed under the next tile's matrix stream.  What differs:
//   * the wave tile is 64 rows x 32 complex columns (6 accumulators, 96 registers): B3 is padded to whole 32-column tiles in the
//     packed operand only -- (F, S, ceil(Cout / 32), 3, 2, 64, 4), columns >= Cout zero -- so 144 columns cost 160 / 144 = 1.11 x the
//     matrix work (64-column tiles: 192 / 144 = 1.33 x, which would give the 3-multiplication form's whole advantage away);
//   * any number of K-stages S = Cin / 16 >= 1: the stage loop runs pairs (the two operand sets swap roles) and, for odd S, one
//     tail stage that loads the next tile's first stage into the other set and moves it over after the tile is parked (56
//     register moves per tile of >= 48 matrix instructions);
//   * a parked tile is 64 rows of 256 bytes: one ds_read_b128 + one 16-byte store per lane move FOUR rows (lanes 16 r .. 16 r + 15
//     carry row 4 p + r), 16 such quads per tile, ceil(16 / S) per K-stage;
//   * columns >= Cout are never stored: Mo's rows are 2 Cout floats and the next row follows directly, so the descriptor's range
//     cannot drop them -- a lane whose two complex columns lie beyond Cout gets a byte offset of 2^31, beyond every range (all of them
//     are < 2^31: host-checked), and its stores are dropped by the hardware like those of rows >= M.  No branch in the stream.
// A 48-column tile on v_mfma_f32_16x16x4_f32 would have no padding at 144 but 36 four-register accumulators: the form whose
// register allocation sank the first wgrad3m (cgemm3m.hip); not built.
// Measured (profiles/cgemm3m_c16/): 1024 tiles, 144 -> 144: 1.38 ms against the library's 1.99 on the real form
// (142 TFLOP/s on the four-product flops); 288 -> 288: 4.59 against 6.28 ms.  B3 is written by fft_filter.hip (eqa_fft48*_filter_spectra3m_c16).
#include <type_traits>

#include "eqa_common.hpp"

namespace {

#include "cgemm3m_common.inc"   // vector types, StageAddr, buf_ld, the persistent grid

constexpr int kC16TileN = 32;                                // complex columns of a wave tile
constexpr unsigned kC16BTileBytes = 3 * 2 * 64 * 4 * 4;      // B3 per (K-stage, 32-column tile): [part r/i/s][b] fragments of 1 KB
constexpr int kC16LdsRowFloats = 2 * kC16TileN;              // one parked row: 32 complex = 256 bytes
constexpr int kC16LdsWaveFloats = kTileM * kC16LdsRowFloats; // 16 KB per wave
constexpr int kC16Quads = kTileM / 4;                        // 4-row groups of a parked tile
constexpr unsigned kC16Masked = 0x80000000u;                 // a lane offset beyond every descriptor range

struct C16Ops {                           // one K-stage of MFMA operands: 56 registers
  f32x4 ar[2][2], ai[2][2];               // [m][b]
  f32x4 b[3][2];                          // [part r/i/s][b]
};

// as load_stage of cgemm3m.hip with one 32-column tile of B
__device__ __forceinline__ void c16_load_stage(C16Ops& o, const StageAddr& at, unsigned aoff0, unsigned aoff1, unsigned boff) {
#pragma unroll
  for (int b = 0; b < 2; ++b) {
    o.ar[0][b] = buf_ld<f32x4>(at.a, aoff0 + 32 * b, at.sa);
    o.ai[0][b] = buf_ld<f32x4>(at.a, aoff0 + 32 * b + 64, at.sa);
    o.ar[1][b] = buf_ld<f32x4>(at.a, aoff1 + 32 * b, at.sa);
    o.ai[1][b] = buf_ld<f32x4>(at.a, aoff1 + 32 * b + 64, at.sa);
#pragma unroll
    for (int p = 0; p < 3; ++p) o.b[p][b] = buf_ld<f32x4>(at.b, boff + (p * 2 + b) * 1024, at.sb);
  }
}

// FIRST: the tile's first K-stage -- the first product into each accumulator starts from zero (no accumulator is ever cleared)
template <bool FIRST>
__device__ __forceinline__ void c16_mma_stage(const C16Ops& o, f32x16 (&acc)[3][2]) {
  const f32x16 zero = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
#pragma unroll
  for (int b = 0; b < 2; ++b) {
    const f32x4 as0 = o.ar[0][b] + o.ai[0][b], as1 = o.ar[1][b] + o.ai[1][b];
#pragma unroll
    for (int t = 0; t < 4; ++t) {
#pragma unroll
      for (int m = 0; m < 2; ++m) {
        const float ar = o.ar[m][b][t], ai = o.ai[m][b][t], as = (m ? as1 : as0)[t];
        const bool fresh = FIRST && b == 0 && t == 0;
        acc[0][m] = __builtin_amdgcn_mfma_f32_32x32x2f32(ar, o.b[0][b][t], fresh ? zero : acc[0][m], 0, 0, 0);
        acc[1][m] = __builtin_amdgcn_mfma_f32_32x32x2f32(ai, o.b[1][b][t], fresh ? zero : acc[1][m], 0, 0, 0);
        acc[2][m] = __builtin_amdgcn_mfma_f32_32x32x2f32(as, o.b[2][b][t], fresh ? zero : acc[2][m], 0, 0, 0);
      }
    }
  }
}

// Where a parked tile goes: a buffer over the tile's rows inside M, the lane's byte offset for quad 0 (kC16Masked: its columns lie
// beyond Cout), the step to the next quad.
struct C16Dst {
  __amdgpu_buffer_rsrc_t rsrc;
  unsigned voff, quad_bytes;
};

// quad p of the parked tile -> Mo.  p >= 16 (a stage count that does not divide 16): the LDS read is clamped into the tile and the
// store lands on row >= 64, outside the descriptor
__device__ __forceinline__ f32x4 c16_read_quad(const float* lds_lane, int p) {
  return *reinterpret_cast<const f32x4*>(lds_lane + min(p, kC16Quads - 1) * (4 * kC16LdsRowFloats));
}
__device__ __forceinline__ void c16_store_quad(const C16Dst& d, int p, f32x4 v) {
  __builtin_amdgcn_raw_buffer_store_b128(__builtin_bit_cast(u32x4, v), d.rsrc, d.voff + (unsigned)min(p, kC16Quads) * d.quad_bytes, 0, 0);
}

// One K-stage: request the next stage's operands, send NQ quads of the parked tile on their way, 48 MFMAs -- one scheduling region
// with pinned order: the LDS reads first, one global load behind every second MFMA, one store behind each of the next NQ.
template <int NQ, bool FIRST>
__device__ __forceinline__ void c16_run_stage(C16Ops& nxt, const C16Ops& cur, f32x16 (&acc)[3][2], const StageAddr& at, unsigned aoff0,
                                              unsigned aoff1, unsigned boff, const float* lds_lane, const C16Dst& dst, int p0) {
  f32x4 park[NQ];
#pragma unroll
  for (int k = 0; k < NQ; ++k) park[k] = c16_read_quad(lds_lane, p0 + k);
  c16_load_stage(nxt, at, aoff0, aoff1, boff);
  c16_mma_stage<FIRST>(cur, acc);
#pragma unroll
  for (int k = 0; k < NQ; ++k) c16_store_quad(dst, p0 + k, park[k]);
  __builtin_amdgcn_sched_group_barrier(0x100, NQ, 0);               // DS reads
#pragma unroll
  for (int k = 0; k < 14; ++k) {
    __builtin_amdgcn_sched_group_barrier(0x008, 2, 0);              // 2 MFMAs
    __builtin_amdgcn_sched_group_barrier(0x020, 1, 0);              // 1 global load
  }
#pragma unroll
  for (int k = 0; k < NQ; ++k) {
    __builtin_amdgcn_sched_group_barrier(0x008, 1, 0);
    __builtin_amdgcn_sched_group_barrier(0x040, 1, 0);              // 1 global store
  }
  __builtin_amdgcn_sched_group_barrier(0x008, 20 - NQ, 0);
}

// The walk of one wave over its wave tiles (frequency, 64 rows, 32 complex columns): WaveTileWalk of cgemm3m_common.inc with this
// tile's geometry -- neighbouring waves take the column tiles of one (f, row tile), the frequencies are dealt to the XCDs.
struct C16Walk {
  const float* V;
  const float* B;
  float* Mo;
  int M, pitch, Cout;
  int xcd, wpf, n_ct, S;
  int lane;
  size_t rowf, mo_row;             // floats per row of V / Mo
  unsigned b_stage_bytes;          // bytes per (f, stage) of B3

  __device__ __forceinline__ C16Walk(const float* V_, const float* B_, float* Mo_, int M_, int pitch_, int Cin, int Cout_, int xcd_, int wpf_,
                                     int n_ct_, int S_, int lane_)
      : V(V_), B(B_), Mo(Mo_), M(M_), pitch(pitch_), Cout(Cout_), xcd(xcd_), wpf(wpf_), n_ct(n_ct_), S(S_), lane(lane_),
        rowf((size_t)2 * Cin), mo_row((size_t)2 * Cout_), b_stage_bytes((unsigned)n_ct_ * kC16BTileBytes) {}

  __device__ __forceinline__ void locate(int u, StageAddr& at, unsigned& aoff0, unsigned& aoff1, int& f, int& row0, int& ct) const {
    const int fi = u / wpf, r = u - fi * wpf;
    f = xcd + kXcd * fi;
    const int rt = r / n_ct;
    ct = r - rt * n_ct;
    row0 = rt * kTileM;
    const int i = lane & 31, h = lane >> 5;
    at.a = __builtin_amdgcn_make_buffer_rsrc(const_cast<float*>(V) + (size_t)f * pitch * rowf, 0, (unsigned)((size_t)pitch * rowf * 4), 0x00020000);
    at.sa = 0;
    aoff0 = (unsigned)((size_t)(row0 + i) * rowf + 4 * h) * 4u;        // rows >= pitch fall outside the descriptor and read as 0
    aoff1 = aoff0 + 32 * (unsigned)rowf * 4u;
    at.b = __builtin_amdgcn_make_buffer_rsrc(const_cast<float*>(B) + (size_t)f * S * (b_stage_bytes / 4u), 0, (unsigned)S * b_stage_bytes, 0x00020000);
    at.sb = (unsigned)ct * kC16BTileBytes;
  }
  __device__ __forceinline__ StageAddr at_stage(const StageAddr& t, int s) const {
    return StageAddr{t.a, t.b, t.sa + s * (32u * 4u), t.sb + s * b_stage_bytes};
  }
  // destination of the tile (f, row0, ct) once it is parked: lane l carries row 4 p + l / 16, complex columns 32 ct + 2 (l % 16), + 1
  __device__ __forceinline__ C16Dst parked(int f, int row0, int ct) const {
    const int rows = min(kTileM, M - row0);
    C16Dst d;
    d.rsrc = __builtin_amdgcn_make_buffer_rsrc(Mo + ((size_t)f * pitch + row0) * mo_row, 0, (unsigned)(rows * mo_row * 4), 0x00020000);
    const int col = ct * kC16TileN + 2 * (lane & 15);
    d.voff = col < Cout ? (unsigned)(((lane >> 4) * mo_row + 2 * (size_t)col) * 4) : kC16Masked;
    d.quad_bytes = 4u * (unsigned)mo_row * 4u;
    return d;
  }
  // before the wave's first tile is finished nothing is parked: an empty buffer drops the stores of the first tile's stage loop
  __device__ __forceinline__ C16Dst nothing_parked(int f, int row0, int ct) const {
    C16Dst d = parked(f, row0, ct);
    d.rsrc = __builtin_amdgcn_make_buffer_rsrc(Mo, 0, 0, 0x00020000);
    return d;
  }
};

// park_tile of cgemm3m_common.inc for one column block: accumulator register e of lane (h, j = i) is row (e & 3) + 8 (e >> 2) + 4 h
__device__ __forceinline__ void c16_park_tile(const f32x16 (&acc)[3][2], float* lds_w, int i, int h) {
#pragma unroll
  for (int m = 0; m < 2; ++m)
#pragma unroll
    for (int e = 0; e < 16; ++e) {
      const int r = 32 * m + (e & 3) + 8 * (e >> 2) + 4 * h;
      const float t1 = acc[0][m][e], t2 = acc[1][m][e], t3 = acc[2][m][e];
      f32x2v c;
      c[0] = t1 - t2;
      c[1] = t3 - t1 - t2;
      *reinterpret_cast<f32x2v*>(lds_w + r * kC16LdsRowFloats + i * 2) = c;
    }
}

// V (F, pitch, 2 Cin) rows [Re x 16 | Im x 16] per 16 channels; B3 (F, S, n_ct, 3, 2, 64, 4), columns >= Cout zero; Mo (F, pitch, 2 Cout)
// interleaved complex.  NQ = ceil(16 / S): quads of the parked tile flushed per K-stage.
template <int NQ>
__global__ __launch_bounds__(256, 1) void fft_cgemm3m_c16_kernel(const float* __restrict__ V, const float* __restrict__ B3,
                                                                 float* __restrict__ Mo, int M, int pitch, int Cin, int Cout, int F,
                                                                 int n_rt, int n_ct, int waves_per_xcd) {
  const int lane = threadIdx.x & 63;
  const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const int xcd = blockIdx.x & (kXcd - 1);
  const int q = (blockIdx.x >> 3) * 4 + wave;          // this wave's slot among the XCD's waves
  const int S = Cin / kStageK;
  const int wpf = n_rt * n_ct;                          // wave tiles per frequency
  const int nf_x = (F - xcd + kXcd - 1) / kXcd;         // frequencies of this XCD: xcd, xcd + 8, ...
  const int total = nf_x * wpf;                         // < 2^31: checked by the host
  if (q >= total) return;
  const int i = lane & 31, h = lane >> 5;
  __shared__ __attribute__((aligned(16))) float lds_all[4 * kC16LdsWaveFloats];
  float* lds_w = lds_all + wave * kC16LdsWaveFloats;    // this wave's parking space for one finished tile
  const float* lds_lane = lds_w + lane * 4;             // quad p: + p * 256 floats (4 rows of 64)
  const C16Walk walk(V, B3, Mo, M, pitch, Cin, Cout, xcd, wpf, n_ct, S, lane);
  const unsigned boff = lane * 16;

  StageAddr at;
  unsigned aoff0, aoff1;
  int f, row0, ct;
  walk.locate(q, at, aoff0, aoff1, f, row0, ct);
  C16Dst dst = walk.nothing_parked(f, row0, ct);
  C16Ops s0, s1;
  c16_load_stage(s0, at, aoff0, aoff1, boff);
  for (int u = q; u < total; u += waves_per_xcd) {
    f32x16 acc[3][2];         // never cleared: the first stage's products start from zero
    // the tile after this one (or this one again when it is the last: a harmless reload instead of a conditional load)
    StageAddr nat;
    unsigned naoff0, naoff1;
    int nf, nrow0, nct;
    walk.locate(u + waves_per_xcd < total ? u + waves_per_xcd : u, nat, naoff0, naoff1, nf, nrow0, nct);
    // stages s, s + 1: s0 -> s1 -> s0 (the scheduling barriers keep the next stage's loads inside this stage's MFMA stream)
    auto stage_pair = [&](int s, auto first_tag) {
      constexpr bool kFirst = decltype(first_tag)::value;
      const bool more = s + 2 < S;
      __builtin_amdgcn_sched_barrier(0);
      c16_run_stage<NQ, kFirst>(s1, s0, acc, walk.at_stage(at, s + 1), aoff0, aoff1, boff, lds_lane, dst, s * NQ);
      __builtin_amdgcn_sched_barrier(0);
      c16_run_stage<NQ, false>(s0, s1, acc, more ? walk.at_stage(at, s + 2) : nat, more ? aoff0 : naoff0, more ? aoff1 : naoff1, boff,
                               lds_lane, dst, (s + 1) * NQ);
      __builtin_amdgcn_sched_barrier(0);
    };
    // the last stage of an odd S: the next tile's first stage arrives in s1
    auto stage_tail = [&](auto first_tag) {
      constexpr bool kFirst = decltype(first_tag)::value;
      __builtin_amdgcn_sched_barrier(0);
      c16_run_stage<NQ, kFirst>(s1, s0, acc, nat, naoff0, naoff1, boff, lds_lane, dst, (S - 1) * NQ);
      __builtin_amdgcn_sched_barrier(0);
    };
    if (S == 1) {
      stage_tail(std::true_type{});
    } else {
      stage_pair(0, std::true_type{});
      int s = 2;
      for (; s + 1 < S; s += 2) stage_pair(s, std::false_type{});
      if (s < S) stage_tail(std::false_type{});
    }
    c16_park_tile(acc, lds_w, i, h);
    if (S & 1) s0 = s1;
    dst = walk.parked(f, row0, ct);
    at = nat; aoff0 = naoff0; aoff1 = naoff1; f = nf; row0 = nrow0; ct = nct;
  }
#pragma unroll
  for (int p = 0; p < kC16Quads; ++p) c16_store_quad(dst, p, c16_read_quad(lds_lane, p));       // the wave's last tile
}

// ---------------------------------------------------------------------------------------------------------------------------
// The filter gradient's contraction for the same channel counts:  D[f] (Cin x Cout, complex) = V[f]^T . conj(G[f]) over the M tiles,
//     P1 = Vr^T Gr    P2 = Vi^T Gi    P3 = (Vr - Vi)^T (Gr + Gi)          Dr = P1 + P2    Di = P1 - P2 - P3
// as fft_wgrad3m_kernel (cgemm3m.hip), with a wave tile of 32 input x 32 output channels (three 32 x 32 accumulators): 160 x 160 at
// 144 channels, 1.23 x the matrix work (64-channel tiles: 1.78 x).  A lane's operand is ONE channel of its tile row (4-byte loads:
// lane l = 32 h + i holds row 2 k + h, channel i of the tile's two [Re x 16 | Im x 16] groups), so the accumulator rows / columns
// are the channels in plain order.  48 + 2 x 32 registers: two waves per SIMD cover each other's load latency.  Lanes whose channel
// lies beyond Cin / Cout read through an offset of 2^31 (zeros: the next row follows directly, the range alone does not mask them)
// and store nothing.  Rows beyond M fall outside the descriptors.  D3 (F, Cin, 2, Cout) as fft_wgrad3m_kernel writes it.
// Measured: (1024 tiles, 144, 144) 1.49 ms against torch.bmm's 1.86; with a padding ratio >= 4/3 (48 x 80, 80 x 80) it ties with the
// library from 512 tiles up -- fftconv.wgrad_c16_admitted keeps those on the library.
constexpr int kWg16Steps = 8;       // MFMA k-steps (2 tiles each) per stage
constexpr int kWg16GridBlocks = 2 * kGridBlocks;
constexpr int kWg16WavesPerXcd = (kWg16GridBlocks / kXcd) * 4;

struct Wg16Ops {
  float ar[kWg16Steps], ai[kWg16Steps], br[kWg16Steps], bi[kWg16Steps];
};

__device__ __forceinline__ float buf_ld1(__amdgpu_buffer_rsrc_t r, unsigned voff, unsigned soff) {
  return __builtin_bit_cast(float, __builtin_amdgcn_raw_buffer_load_b32(r, voff, soff, 0));
}

__device__ __forceinline__ void wg16_load(Wg16Ops& o, __amdgpu_buffer_rsrc_t ra, __amdgpu_buffer_rsrc_t rb, unsigned aoff, unsigned boff,
                                          unsigned sa, unsigned sb, unsigned step_a, unsigned step_b) {
#pragma unroll
  for (int k = 0; k < kWg16Steps; ++k) {
    o.ar[k] = buf_ld1(ra, aoff, sa + k * step_a);
    o.ai[k] = buf_ld1(ra, aoff + 64, sa + k * step_a);
    o.br[k] = buf_ld1(rb, boff, sb + k * step_b);
    o.bi[k] = buf_ld1(rb, boff + 64, sb + k * step_b);
  }
}

// one stage (16 tiles, 24 MFMAs) with the next stage's 32 loads spread through them
__device__ __forceinline__ void wg16_stage(Wg16Ops& nxt, const Wg16Ops& cur, f32x16 (&acc)[3], __amdgpu_buffer_rsrc_t ra,
                                           __amdgpu_buffer_rsrc_t rb, unsigned aoff, unsigned boff, unsigned sa, unsigned sb,
                                           unsigned step_a, unsigned step_b) {
  wg16_load(nxt, ra, rb, aoff, boff, sa, sb, step_a, step_b);
#pragma unroll
  for (int k = 0; k < kWg16Steps; ++k) {
    const float as = cur.ar[k] - cur.ai[k], bs = cur.br[k] + cur.bi[k];
    acc[0] = __builtin_amdgcn_mfma_f32_32x32x2f32(cur.ar[k], cur.br[k], acc[0], 0, 0, 0);
    acc[1] = __builtin_amdgcn_mfma_f32_32x32x2f32(cur.ai[k], cur.bi[k], acc[1], 0, 0, 0);
    acc[2] = __builtin_amdgcn_mfma_f32_32x32x2f32(as, bs, acc[2], 0, 0, 0);
  }
#pragma unroll
  for (int k = 0; k < kWg16Steps; ++k) {
    __builtin_amdgcn_sched_group_barrier(0x008, 3, 0);
    __builtin_amdgcn_sched_group_barrier(0x020, 4, 0);
  }
}

__global__ __launch_bounds__(256, 2) void fft_wgrad3m_c16_kernel(const float* __restrict__ V, const float* __restrict__ G,
                                                                 float* __restrict__ D, int M, int pitch, int Cin, int Cout, int F, int n_it,
                                                                 int n_ot, int waves_per_xcd) {
  const int lane = threadIdx.x & 63;
  const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const int xcd = blockIdx.x & (kXcd - 1);
  const int q = (blockIdx.x >> 3) * 4 + wave;
  const int wpf = n_it * n_ot;                          // wave tiles per frequency; neighbouring waves share the input-channel tile
  const int nf_x = (F - xcd + kXcd - 1) / kXcd;
  const int total = nf_x * wpf;
  const int i = lane & 31, h = lane >> 5;
  const size_t rowa = (size_t)2 * Cin, rowb = (size_t)2 * Cout;
  const unsigned step_a = 2u * (unsigned)rowa * 4u, step_b = 2u * (unsigned)rowb * 4u;   // 2 tiles further
  const int steps = (M + 1) / 2;
  for (int u = q; u < total; u += waves_per_xcd) {
    const int fi = u / wpf, r = u - fi * wpf;
    const int f = xcd + kXcd * fi;
    const int it = r / n_ot, ot = r - it * n_ot;
    const __amdgpu_buffer_rsrc_t ra = __builtin_amdgcn_make_buffer_rsrc(const_cast<float*>(V) + (size_t)f * pitch * rowa, 0,
                                                                        (unsigned)((size_t)M * rowa * 4), 0x00020000);
    const __amdgpu_buffer_rsrc_t rb = __builtin_amdgcn_make_buffer_rsrc(const_cast<float*>(G) + (size_t)f * pitch * rowb, 0,
                                                                        (unsigned)((size_t)M * rowb * 4), 0x00020000);
    // this lane's channel of tile row h: group i / 16 of the wave tile's two [Re x 16 | Im x 16] groups, float i % 16 (Im: + 16)
    const int ci = it * 32 + i, co = ot * 32 + i;
    const unsigned aoff = ci < Cin ? (unsigned)((size_t)h * rowa + (size_t)it * 64 + (i >> 4) * 32 + (i & 15)) * 4u : kC16Masked;
    const unsigned boff = co < Cout ? (unsigned)((size_t)h * rowb + (size_t)ot * 64 + (i >> 4) * 32 + (i & 15)) * 4u : kC16Masked;
    f32x16 acc[3];
#pragma unroll
    for (int p = 0; p < 3; ++p)
#pragma unroll
      for (int e = 0; e < 16; ++e) acc[p][e] = 0.f;
    Wg16Ops s0, s1;
    wg16_load(s0, ra, rb, aoff, boff, 0, 0, step_a, step_b);
    for (int s = 0; s < steps; s += 2 * kWg16Steps) {   // steps past the last read beyond the descriptors: zeros, harmless
      __builtin_amdgcn_sched_barrier(0);
      wg16_stage(s1, s0, acc, ra, rb, aoff, boff, (s + kWg16Steps) * step_a, (s + kWg16Steps) * step_b, step_a, step_b);
      __builtin_amdgcn_sched_barrier(0);
      wg16_stage(s0, s1, acc, ra, rb, aoff, boff, (s + 2 * kWg16Steps) * step_a, (s + 2 * kWg16Steps) * step_b, step_a, step_b);
      __builtin_amdgcn_sched_barrier(0);
    }
    // accumulator register e of lane (h, j = i): input channel 32 it + (e & 3) + 8 (e >> 2) + 4 h, output channel 32 ot + j:
    // the 32 lanes of a half wave store one 128-byte run
    float* Df = D + (size_t)f * (2 * (size_t)Cin) * Cout;           // D3[f][ci][Dr | Di][co]
    if (co < Cout) {
#pragma unroll
      for (int e = 0; e < 16; ++e) {
        const int cr = it * 32 + (e & 3) + 8 * (e >> 2) + 4 * h;
        if (cr < Cin) {
          const float p1 = acc[0][e], p2 = acc[1][e], p3 = acc[2][e];
          Df[(2 * (size_t)cr) * Cout + co] = p1 + p2;
          Df[(2 * (size_t)cr + 1) * Cout + co] = p1 - p2 - p3;
        }
      }
    }
  }
}

// what both contractions ask of their arguments (kNothingToDo: M == 0)
int c16_args(const void* V, const void* B, const void* O, int64_t M, int Cin, int Cout, int supported) {
  if (!V || !B || !O || M < 0 || Cin <= 0 || Cout <= 0) return EQA_ERR_INVALID_ARG;
  if (M == 0) return kNothingToDo;
  // every descriptor range and lane offset must stay below 2^31 (the masked lanes' offset): one frequency of V / G / Mo
  const int64_t fm_bytes = ((M | 1) + 64) * 2 * (int64_t)std::max(Cin, Cout) * 4;
  if (!supported || M > 0x3fffff || fm_bytes > 0x7fffffffLL || (((uintptr_t)V | (uintptr_t)B | (uintptr_t)O) & 15))
    return EQA_ERR_UNSUPPORTED;
  return EQA_OK;
}

}  // namespace

extern "C" {

int eqa_fft48_cgemm3m_c16_supported(int Cin, int Cout) { return Cin > 0 && Cout > 0 && Cin % 16 == 0 && Cout % 16 == 0; }

int64_t eqa_fft48_spectra3m_c16_floats(int Cin, int Cout) {
  if (!eqa_fft48_cgemm3m_c16_supported(Cin, Cout)) return 0;
  return (int64_t)eqa_fft48k5_frequencies() * Cin * ((Cout + 31) / 32 * 32) * 3;
}

int eqa_fft48_cgemm3m_c16(const float* V, const float* B3, float* Mo, int64_t M, int Cin, int Cout, void* stream) {
  const int st = c16_args(V, B3, Mo, M, Cin, Cout, eqa_fft48_cgemm3m_c16_supported(Cin, Cout));
  if (st != EQA_OK) return st == kNothingToDo ? EQA_OK : st;
  const int F = eqa_fft48k5_frequencies();
  const int n_rt = (int)((M + kTileM - 1) / kTileM), n_ct = (Cout + kC16TileN - 1) / kC16TileN;
  const int S = Cin / kStageK;
  if ((int64_t)S * n_ct * kC16BTileBytes > 0x7fffffffLL) return EQA_ERR_UNSUPPORTED;      // one frequency of B3: a descriptor range
  if ((int64_t)((F + kXcd - 1) / kXcd) * n_rt * n_ct > 0x7fffffffLL) return EQA_ERR_UNSUPPORTED;
#define EQA_C16_LAUNCH(NQ)                                                                                                       \
  hipLaunchKernelGGL(fft_cgemm3m_c16_kernel<NQ>, dim3(kGridBlocks), dim3(256), 0, (hipStream_t)stream, V, B3, Mo, (int)M,        \
                     (int)eqa_fft48k5_tile_pitch(M), Cin, Cout, F, n_rt, n_ct, kWavesPerXcd)
  switch (S >= kC16Quads ? 1 : (kC16Quads + S - 1) / S) {     // quads of the parked tile that leave per K-stage
    case 16: EQA_C16_LAUNCH(16); break;   // S = 1
    case 8: EQA_C16_LAUNCH(8); break;     // 2
    case 6: EQA_C16_LAUNCH(6); break;     // 3
    case 4: EQA_C16_LAUNCH(4); break;     // 4, 5
    case 3: EQA_C16_LAUNCH(3); break;     // 6, 7
    case 2: EQA_C16_LAUNCH(2); break;     // 8 .. 15 (144 channels: 9)
    default: EQA_C16_LAUNCH(1); break;    // >= 16
  }
#undef EQA_C16_LAUNCH
  return launch_status();
}

int eqa_fft48_wgrad3m_c16_supported(int Cin, int Cout) { return eqa_fft48_cgemm3m_c16_supported(Cin, Cout); }

int eqa_fft48_wgrad3m_c16(const float* V, const float* G, float* D, int64_t M, int Cin, int Cout, void* stream) {
  const int st = c16_args(V, G, D, M, Cin, Cout, eqa_fft48_wgrad3m_c16_supported(Cin, Cout));
  if (st != EQA_OK) return st == kNothingToDo ? EQA_OK : st;
  const int F = eqa_fft48k5_frequencies();
  const int n_it = (Cin + 31) / 32, n_ot = (Cout + 31) / 32;
  if ((int64_t)((F + kXcd - 1) / kXcd) * n_it * n_ot > 0x7fffffffLL) return EQA_ERR_UNSUPPORTED;
  hipLaunchKernelGGL(fft_wgrad3m_c16_kernel, dim3(kWg16GridBlocks), dim3(256), 0, (hipStream_t)stream, V, G, D, (int)M,
                     (int)eqa_fft48k5_tile_pitch(M), Cin, Cout, F, n_it, n_ot, kWg16WavesPerXcd);
  return launch_status();
}

}  // extern "C"
