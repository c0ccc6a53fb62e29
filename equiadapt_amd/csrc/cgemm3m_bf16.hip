// libeqa_hip.so, part 11 -- the channel contraction of the overlap-save FFT convolution (cgemm3m.hip) on the bf16 matrix cores,
// EXACT in the sense the fp32 matrix instruction is: every fp32 operand is split without error into three bf16 pieces
//     x = p1 + p2 + p3,     p1 = the top 16 bits of x, p2 = the top 16 bits of x - p1, p3 = x - p1 - p2   (8 significant bits each:
//     3 x 8 = the 24 of an fp32 significand; truncation keeps the remainders' signs equal, so no bit is spent twice)
// and the product of two operands is the sum of the nine products of their pieces, each of which the matrix core forms exactly
// (8 x 8 significant bits) and accumulates in fp32 -- the same "exact products, fp32 accumulation" contract as
// v_mfma_f32_32x32x2_f32, in a different summation order.  v_mfma_f32_32x32x16_bf16 retires 16 k per 32 cycles where the fp32
// form retires 2 per 64: nine piece products cost 288 cycles per 16 k against 512.  C ABI: include/eqa_hip.h; HISTORY.md 3.8.
//
// TERMS = 9: all piece products (the default when this path is selected).  TERMS = 6: the three products of relative size
// <= 2^-24 (p2.p3, p3.p2, p3.p3) are left out -- an error of at most 2^-23 |a||b| per product, the size of the rounding a single
// fp32 multiply-add commits; opt-in (the caller passes terms = 6), reported beside the exact form, never silently.
//
// Same work decomposition, operand flow and epilogue as fft_cgemm3m_kernel: a wave-tile is (frequency, 64 rows, 64 complex
// columns), three accumulator sets (T1 = Ar.Br, T2 = Ai.Bi, T3 = (Ar + Ai).(Br + Bi)), one wave per SIMD, no LDS for operands,
// operands one K-stage (16 complex k) ahead, the finished tile parked in LDS and flushed under the next tile's MFMA stream.
// A (the spectra of the activations, fp32 in HBM) is split in registers: 48 values per lane and stage, ~6 VALU instructions each,
// in the shadow of the matrix instructions (tools/micro/bf16x3_rate.hip: 3925 cycles per stage with the split, 3465 without,
// 6144 in the fp32 form).  B (the filter spectra) is split once per weight version (eqa_fft48k5_spectra3m_split) into the
// fragment order of the bf16 instruction: (F, S, Cout / 32, 3 parts, 3 pieces, 64 lanes, 8 bf16).
// The instruction sums over k in any order, so a lane keeps the 16 + 16 bytes it loads today: slot e = 4 b + t of lane (i, h) is
// channel 16 s + 8 b + 4 h + t on both sides.
#include "eqa_common.hpp"

// The one debug build that is kept (tools/kbench_gemm_clock.py): -DEQA_BLK_CLOCK=1 stamps the first / last shader cycle and the
// constant 100 MHz counter of block 100's first thread and the cycles of its tile epilogues; =2 adds an s_memtime at every region
// boundary of a K-stage.  The product build's BlkClock is empty: the block kernel calls it unconditionally.
#ifdef EQA_BLK_CLOCK
namespace {
__device__ long long g_blk_clock[16];
struct BlkClock {
  long long c0, w0, e0, t_epi;
  unsigned long long tk[8], tot[8];
  __device__ __forceinline__ BlkClock() : c0(clock64()), w0(wall_clock64()), e0(0), t_epi(0), tk{}, tot{} {}
  __device__ __forceinline__ void tick(int i) {
    if constexpr (EQA_BLK_CLOCK >= 2) {
      __builtin_amdgcn_sched_barrier(0);
      asm volatile("s_memtime %0" : "=s"(tk[i]));
    }
  }
  __device__ __forceinline__ void stage_end() {          // behind the stage's barrier
    if constexpr (EQA_BLK_CLOCK >= 2) {
      tick(5);
      asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
#pragma unroll
      for (int i = 0; i < 5; ++i) tot[i] += tk[i + 1] - tk[i];
    }
  }
  __device__ __forceinline__ void tile_epilogue_begin() { e0 = clock64(); }
  __device__ __forceinline__ void tile_epilogue_end() { t_epi += clock64() - e0; }
  __device__ __forceinline__ void publish() {
    if (blockIdx.x == 100 && threadIdx.x == 0) {
      g_blk_clock[0] = clock64() - c0; g_blk_clock[1] = wall_clock64() - w0; g_blk_clock[2] = t_epi;
      for (int i = 0; i < 7; ++i) g_blk_clock[3 + i] = (long long)tot[i];
    }
  }
};
}  // namespace
extern "C" int eqa_debug_blk_clock(long long* out) { return (int)hipMemcpyFromSymbol(out, HIP_SYMBOL(g_blk_clock), 80); }
#else
namespace {
struct BlkClock {
  __device__ __forceinline__ void tick(int) {}
  __device__ __forceinline__ void stage_end() {}
  __device__ __forceinline__ void tile_epilogue_begin() {}
  __device__ __forceinline__ void tile_epilogue_end() {}
  __device__ __forceinline__ void publish() {}
};
}  // namespace
#endif

namespace {

#include "cgemm3m_common.inc"   // the wave-tile walk, the buffer descriptors, the parked tile: shared with cgemm3m.hip

typedef __bf16 bf16x8 __attribute__((ext_vector_type(8)));
typedef unsigned u32x2 __attribute__((ext_vector_type(2)));

constexpr unsigned kHi = 0xffff0000u;

// The three-piece split of one value: bit patterns whose top 16 bits are p1, p2, p3 (x = p1 + p2 + p3)
__device__ __forceinline__ void split3(const float a, unsigned (&x)[3]) {
  const float p1 = __builtin_bit_cast(float, __builtin_bit_cast(unsigned, a) & kHi);
  const float r1 = a - p1;                                       // exact: the low 16 bits of the significand
  const float p2 = __builtin_bit_cast(float, __builtin_bit_cast(unsigned, r1) & kHi);
  const float r2 = r1 - p2;                                      // exact: at most 8 significant bits -> a bf16 as it stands
  x[0] = __builtin_bit_cast(unsigned, a);
  x[1] = __builtin_bit_cast(unsigned, r1);
  x[2] = __builtin_bit_cast(unsigned, r2);
}
// the high halves of two such patterns -> one dword of two bf16 (v_perm_b32)
__device__ __forceinline__ unsigned pack_hi(const unsigned lo, const unsigned hi) { return __builtin_amdgcn_perm(hi, lo, 0x07060302u); }

// 8 fp32 values (two 16-byte loads) -> three packed operands of the bf16 instruction
struct Pieces {
  u32x4 p[3];
};
__device__ __forceinline__ Pieces split8(const f32x4 lo, const f32x4 hi) {
  Pieces o;
  unsigned x[8][3];
#pragma unroll
  for (int e = 0; e < 8; ++e) split3(e < 4 ? lo[e & 3] : hi[e & 3], x[e]);
#pragma unroll
  for (int j = 0; j < 4; ++j)
#pragma unroll
    for (int q = 0; q < 3; ++q) o.p[q][j] = pack_hi(x[2 * j][q], x[2 * j + 1][q]);
  return o;
}
// 4 values -> their three pieces, 8 bytes each
__device__ __forceinline__ void split4(const f32x4 v, u32x2 (&o)[3]) {
  unsigned x[4][3];
#pragma unroll
  for (int t = 0; t < 4; ++t) split3(v[t], x[t]);
#pragma unroll
  for (int q = 0; q < 3; ++q) {
    o[q][0] = pack_hi(x[0][q], x[1][q]);
    o[q][1] = pack_hi(x[2][q], x[3][q]);
  }
}

// Registers: 192 accumulators (AGPRs) leave 256 + 64 for everything else, and the register allocator shuttles operands between
// the two files once the architectural half overflows (first version: 576 v_accvgpr copies per 216 matrix instructions, no faster
// than the fp32 kernel).  So B is held by HALF stages -- the 36 registers of one 32-column half in use, the other half in flight --
// and a stage runs column half by column half: [n = 0: m = 0, m = 1] [n = 1: m = 0, m = 1] with the pieces of both row halves of A
// (72 registers) split once per stage.
struct ARaw {                    // the rows of one 32-row half of a K-stage of A as loaded: fp32, [b]
  f32x4 ar[2], ai[2];
};
struct BHalf {                   // one 32-column half of a K-stage of B: [part r/i/s][piece]
  u32x4 b[3][3];
};
struct APieces {
  Pieces a[2][3];                // [m][part]
};

constexpr unsigned kBFrag = 64 * 16;    // bytes of one (part, piece) fragment of a 32-column tile
constexpr unsigned kBTileBytes = 9 * kBFrag;   // Bp per (K-stage, 32-column tile): [part r/i/s][piece]

__device__ __forceinline__ void load_a(ARaw& o, const StageAddr& at, unsigned aoff) {
#pragma unroll
  for (int b = 0; b < 2; ++b) {
    o.ar[b] = buf_ld<f32x4>(at.a, aoff + 32 * b, at.sa);
    o.ai[b] = buf_ld<f32x4>(at.a, aoff + 32 * b + 64, at.sa);
  }
}
__device__ __forceinline__ void load_b(BHalf& o, const StageAddr& at, unsigned boff, int n) {
#pragma unroll
  for (int p = 0; p < 3; ++p)
#pragma unroll
    for (int q = 0; q < 3; ++q) o.b[p][q] = buf_ld<u32x4>(at.b, boff + ((n * 3 + p) * 3 + q) * kBFrag, at.sb);
}

__device__ __forceinline__ void split_a(APieces& P, const ARaw& r, int m) {
  P.a[m][0] = split8(r.ar[0], r.ar[1]);
  P.a[m][1] = split8(r.ai[0], r.ai[1]);
  P.a[m][2] = split8(r.ar[0] + r.ai[0], r.ar[1] + r.ai[1]);
}

__device__ __forceinline__ f32x16 mma(const u32x4 a, const u32x4 b, const f32x16 c) {
  return __builtin_amdgcn_mfma_f32_32x32x16_bf16(__builtin_bit_cast(bf16x8, a), __builtin_bit_cast(bf16x8, b), c, 0, 0, 0);
}

// the matrix instructions of one (column half n, row half m): consecutive ones go to different accumulators, large products first
template <int TERMS>
__device__ __forceinline__ void mma_quarter(const APieces& P, const BHalf& B, f32x16 (&acc)[3][2][2], int m, int n) {
#pragma unroll
  for (int w = 0; w < 5; ++w)         // w = pa + pb
#pragma unroll
    for (int pa = 0; pa < 3; ++pa) {
      const int pb = w - pa;
      if (pb < 0 || pb > 2 || (TERMS == 6 && w > 2)) continue;
#pragma unroll
      for (int p = 0; p < 3; ++p) acc[p][m][n] = mma(P.a[m][p].p[pa], B.b[p][pb], acc[p][m][n]);
    }
}

// One K-stage = four quarters (column half n, row half m), 3 x TERMS matrix instructions each, every quarter one scheduling region
// in which the instruction order is pinned: the wave issues in order, so whatever is to run in the shadow of the matrix pipe has
// to sit BETWEEN two matrix instructions.
//   quarter (0,0): + split of THIS stage's row half 1 (its pieces are dead since the previous stage's last quarter)
//                  + requests: this stage's column half 1 of B, the next stage's row half 0 of A
//   quarter (1,0): + request: the next stage's row half 1 of A (its registers were read by the split just done)
//   quarter (0,1): + request: the next stage's column half 0 of B (half 0 was last read in the previous quarter); parked rows leave
//   quarter (1,1): + split of the NEXT stage's row half 0 (requested three quarters ago)
// so a B half is requested half a stage before its use, A a whole stage, and the 280 VALU instructions of a stage's splits are
// spread over two quarters.  On entry: P.a[0] = pieces of this stage's row half 0, raw1 = this stage's row half 1 as loaded,
// B0 = this stage's column half 0.
template <int NMMA, int NVALU, int NLOAD, int NSTORE, int NDS>
__device__ __forceinline__ void pin_quarter() {
  if (NDS) __builtin_amdgcn_sched_group_barrier(0x100, NDS, 0);
  constexpr int kMem = NLOAD + NSTORE;
  constexpr int kValuPer = (NVALU + NMMA - 1) / NMMA;
#pragma unroll
  for (int k = 0; k < NMMA; ++k) {
    __builtin_amdgcn_sched_group_barrier(0x008, 1, 0);                       // one matrix instruction
    if (k < NLOAD) __builtin_amdgcn_sched_group_barrier(0x020, 1, 0);        // one load behind each of the first ones
    else if (k < kMem) __builtin_amdgcn_sched_group_barrier(0x040, 1, 0);    // ... then the stores
    if (NVALU) __builtin_amdgcn_sched_group_barrier(0x002, kValuPer, 0);     // its share of the vector arithmetic
  }
}

template <int NPAIR, int TERMS>
__device__ __forceinline__ void run_stage(APieces& P, ARaw& raw0, ARaw& raw1, BHalf& B0, BHalf& B1, f32x16 (&acc)[3][2][2],
                                          const StageAddr& cur, const StageAddr& nxt, unsigned naoff0, unsigned naoff1, unsigned boff,
                                          const float* lds_lane, const ParkedDst& dst, int p0) {
  constexpr int kQ = 3 * TERMS;          // matrix instructions per quarter
  constexpr int kSplit = 150;            // vector instructions of one row half's split (an upper bound for the pinning)
  f32x4 park[NPAIR > 0 ? NPAIR : 1];
  __builtin_amdgcn_sched_barrier(0);
  // (Tried: one dword per lane of A three stages ahead, to pull the lines into L2 early -- SLOWER, 3.455 vs 3.32 ms:
  // profiles/r04/kbench_gemm_pieces.txt.  A's three quarters of a stage of lead are not what is missing.)
  load_b(B1, cur, boff, 1);
  load_a(raw0, nxt, naoff0);
  split_a(P, raw1, 1);
  mma_quarter<TERMS>(P, B0, acc, 0, 0);
  pin_quarter<kQ, kSplit, 13, 0, 0>();
  __builtin_amdgcn_sched_barrier(0);
  load_a(raw1, nxt, naoff1);
  mma_quarter<TERMS>(P, B0, acc, 1, 0);
  pin_quarter<kQ, 0, 4, 0, 0>();
  __builtin_amdgcn_sched_barrier(0);
#pragma unroll
  for (int k = 0; k < NPAIR; ++k) park[k] = *reinterpret_cast<const f32x4*>(lds_lane + (p0 + k) * (2 * kLdsRowFloats));
  load_b(B0, nxt, boff, 0);
  mma_quarter<TERMS>(P, B1, acc, 0, 1);
#pragma unroll
  for (int k = 0; k < NPAIR; ++k) store_pair(dst, p0 + k, park[k]);
  pin_quarter<kQ, 0, 9, NPAIR, NPAIR>();
  __builtin_amdgcn_sched_barrier(0);
  split_a(P, raw0, 0);
  mma_quarter<TERMS>(P, B1, acc, 1, 1);
  pin_quarter<kQ, kSplit, 0, 0, 0>();
  __builtin_amdgcn_sched_barrier(0);
}

template <int NPAIR, int TERMS>
__global__ __launch_bounds__(256, 1) void fft_cgemm3m_bf16_kernel(const float* __restrict__ V, const uint16_t* __restrict__ Bp,
                                                                  float* __restrict__ Mo, int M, int pitch, int Cin, int Cout, int F,
                                                                  int n_rt, int n_ct, int waves_per_xcd) {
  const int lane = threadIdx.x & 63;
  const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const int xcd = blockIdx.x & (kXcd - 1);
  const int q = (blockIdx.x >> 3) * 4 + wave;
  const int S = Cin / kStageK;
  const int wpf = n_rt * n_ct;
  const int nf_x = (F - xcd + kXcd - 1) / kXcd;
  const int total = nf_x * wpf;
  if (q >= total) return;
  const int i = lane & 31, h = lane >> 5;
  __shared__ __attribute__((aligned(16))) float lds_all[4 * kLdsWaveFloats];
  float* lds_w = lds_all + wave * kLdsWaveFloats;
  const float* lds_lane = lds_w + h * kLdsRowFloats + i * 4;
  const WaveTileWalk<uint16_t, kBTileBytes> walk(V, Bp, Mo, M, pitch, Cin, Cout, xcd, wpf, n_ct, S, i, h);
  const unsigned boff = lane * 16;

  StageAddr at;
  unsigned aoff0, aoff1;
  int f, row0, ct;
  walk.locate(q, at, aoff0, aoff1, f, row0, ct);
  ParkedDst dst = walk.nothing_parked(f, row0, ct);
  ARaw raw0, raw1;
  APieces P;
  BHalf B0, B1;
  load_a(raw0, at, aoff0);
  load_a(raw1, at, aoff1);
  load_b(B0, at, boff, 0);
  split_a(P, raw0, 0);
  for (int u = q; u < total; u += waves_per_xcd) {
    f32x16 acc[3][2][2];
#pragma unroll
    for (int p = 0; p < 3; ++p)
#pragma unroll
      for (int m = 0; m < 2; ++m)
#pragma unroll
        for (int n = 0; n < 2; ++n)
#pragma unroll
          for (int e = 0; e < 16; ++e) acc[p][m][n][e] = 0.f;
    // the tile after this one (or this one again when it is the last: a harmless reload instead of a conditional load)
    StageAddr nat;
    unsigned naoff0, naoff1;
    int nf, nrow0, nct;
    walk.locate(u + waves_per_xcd < total ? u + waves_per_xcd : u, nat, naoff0, naoff1, nf, nrow0, nct);
    for (int s = 0; s < S; ++s) {
      const bool more = s + 1 < S;
      if (NPAIR == 0) flush_rows(lds_lane, dst, (32 * s) / S, (32 * (s + 1)) / S);
      run_stage<NPAIR, TERMS>(P, raw0, raw1, B0, B1, acc, walk.at_stage(at, s), more ? walk.at_stage(at, s + 1) : nat,
                              more ? aoff0 : naoff0, more ? aoff1 : naoff1, boff, lds_lane, dst, s * NPAIR);
    }
    park_tile(acc, lds_w, i, h);
    dst = walk.parked(f, row0, ct);
    at = nat; aoff0 = naoff0; aoff1 = naoff1; f = nf; row0 = nrow0; ct = nct;
  }
  flush_rows(lds_lane, dst, 0, 32);       // the wave's last tile
}

// ---------------------------------------------------------------------------------------------------------------------------
// The BLOCK form (Cout a multiple of 128).  What bounds the wave form is not the matrix pipe but the vector L1: a 1-KB wave load
// returns every ~22 cycles per CU, and a wave-tile of 64 x 64 asks for 18 fragments of B and 8 loads of A per K-stage -- 104 loads
// per CU and stage = 2.3 k cycles against 2.3 k (six products) / 3.5 k (nine) of matrix instructions.  Here a block works on
// 128 rows x 128 columns of one frequency, wave w on columns 32 w .. 32 w + 31 of all 128 rows:
//   * A's K-stage is the same for the four waves: loaded and split ONCE per block (two rows per thread) and shared through LDS in
//     the fragment order of the instruction -- a half of the wave form's split arithmetic per matrix instruction, no A load per wave;
//   * B's K-stage is 9 fragments per wave instead of 18: 36 + 16 loads per CU and stage (1.1 k cycles of the L1).
//   LDS: three K-stages of A's pieces, 36 fragments [row quarter m][part r/i/s][piece] of 64 lanes x 16 bytes = 36 KB a stage.
//        Stage g + 2 is written while stage g is multiplied and stage g + 1 stands published: ONE barrier per stage, at the stage
//        boundary, and nothing is read right behind it (a stage's first fragments are read before the barrier that ends the
//        stage before: they were published a stage earlier).
//   splitter: thread (wave w, lane l) owns rows 16 w + (l >> 1 & 15) and + 64, k = 8 (l & 1) + 4 (l >> 5) + 0..3 of the stage:
//        four 16-byte loads (re, im of two rows), 24 values split, eighteen 8-byte LDS writes (lanes 0..31 of a write cover 512
//        contiguous bytes: no conflict).  The raw values of stage g + 4 are requested when those of g + 2 have been split.
//   B: a K-stage (9 fragments, 36 registers) a stage ahead in a second register set, requested in the stage's first quarter.
//   matrix instructions of a stage: four regions (row quarter m), each the three A pieces against every B piece: 27 (TERMS = 6:
//        18) instructions; a region reads the nine fragments it needs next from LDS behind its first nine matrix instructions.
//   the finished tile leaves straight from the accumulators: lane (column i, h) holds (Cr, Ci) of 16 rows per m -- 8-byte stores,
//        256 contiguous bytes per row.
constexpr int kBlkM = 128, kBlkN = 128;
constexpr int kFragBytes = 64 * 16;
constexpr int kABufs = 3;
typedef _Float16 f16x8 __attribute__((ext_vector_type(8)));

// TERMS = 3: the fp16 form.  An fp32 operand x, scaled by a power of two into the top of the fp16 range, is split into TWO fp16
// pieces h1 = rn(x), h2 = rn(x - h1): 11 + 11 significant bits and a sign -> |x - h1 - h2| <= 2^-23 |x|, one fp32 ulp at worst (a third of one in rms); the
// product x y is taken as h1 k1 + h1 k2 + h2 k1 (each exact in v_mfma_f32_32x32x16_f16, fp32 accumulate; h2 k2 <= 2^-22 |x y| is
// left out).  Three matrix instructions per product instead of six, and -- fewer accumulator roundings -- CLOSER to an fp64
// product than the six bf16 pieces or the fp32 instruction (tools/micro/f16x2_gemm_check.hip, profiles/r06/f16x2_gemm_check.txt:
// rms 3.9e-8 / 5.1e-8 / 5.7e-8 on the parity test's magnitudes).  The price is the range: the caller hands over an upper bound of
// |V| (the DC bins of non-negative activations bound every other bin) and the filter spectra are scaled when they are split;
// values 2^16 below the bound keep full precision, smaller ones lose it gradually (fp16 subnormals: honoured by the instruction).
constexpr int pieces_of(int terms) { return terms == 3 ? 2 : 3; }
constexpr int a_stage_bytes(int terms) { return 12 * pieces_of(terms) * kFragBytes; }

template <int NP>
struct BSet {
  u32x4 b[3][NP];                 // [part][piece] of the wave's 32 columns
};
struct AFrags {
  u32x4 a[3];                     // [part] of one (row quarter, piece)
};
struct RawA {
  f32x4 re[2], im[2];             // rows r and r + 64
};
struct TileAt {                   // uniform: where a block tile's operands are
  __amdgpu_buffer_rsrc_t a, b;
  unsigned sb;
};

// two fp16 pieces of four (already scaled) values: v_cvt_pk_f16_f32 (round to nearest even), the remainder, again
typedef _Float16 f16x2v __attribute__((ext_vector_type(2)));
__device__ __forceinline__ void split4h(const f32x4 v, u32x2 (&o)[2]) {
#pragma unroll
  for (int j = 0; j < 2; ++j) {
    const float a = v[2 * j], b = v[2 * j + 1];
    const f16x2v h = {(_Float16)a, (_Float16)b};
    const f16x2v l = {(_Float16)(a - (float)h[0]), (_Float16)(b - (float)h[1])};
    o[0][j] = __builtin_bit_cast(unsigned, h);
    o[1][j] = __builtin_bit_cast(unsigned, l);
  }
}
// one part (0 re, 1 im, 2 re + im) of row ROW's 4 k: split, NP 8-byte writes into the stage being built (row r + 64 is row
// quarter m + 2: 6 NP fragments further).  NP = 2: the values are scaled first (`scale`: a power of two).
template <int NP, int ROW, int PART>
__device__ __forceinline__ void split_part(const RawA& r, unsigned char* wr, const float scale) {
  const f32x4 v = PART == 0 ? r.re[ROW] : PART == 1 ? r.im[ROW] : r.re[ROW] + r.im[ROW];
  u32x2 o[NP];
  if constexpr (NP == 3) split4(v, o);
  else split4h(v * scale, o);
#pragma unroll
  for (int q = 0; q < NP; ++q) *reinterpret_cast<u32x2*>(wr + (ROW * 6 * NP + PART * NP + q) * kFragBytes) = o[q];
}
template <int ROW>
__device__ __forceinline__ void load_raw(RawA& o, const TileAt& t, unsigned voff, unsigned row64, unsigned soff) {
  o.re[ROW] = buf_ld<f32x4>(t.a, voff + ROW * row64, soff);
  o.im[ROW] = buf_ld<f32x4>(t.a, voff + ROW * row64 + 64, soff);
}
template <int NP>
__device__ __forceinline__ void load_bset(BSet<NP>& o, const TileAt& t, unsigned voff, unsigned soff) {
#pragma unroll
  for (int k = 0; k < 3 * NP; ++k) o.b[k / NP][k % NP] = buf_ld<u32x4>(t.b, voff + k * kBFrag, t.sb + soff);
}
template <int NP, int M, int PA>
__device__ __forceinline__ void read_frags(AFrags& o, const unsigned char* rd) {
#pragma unroll
  for (int p = 0; p < 3; ++p) o.a[p] = *reinterpret_cast<const u32x4*>(rd + ((M * 3 + p) * NP + PA) * kFragBytes);
}
template <int TERMS>
__device__ __forceinline__ f32x16 mma_t(const u32x4 a, const u32x4 b, const f32x16 c) {
  if constexpr (TERMS == 3) return __builtin_amdgcn_mfma_f32_32x32x16_f16(__builtin_bit_cast(f16x8, a), __builtin_bit_cast(f16x8, b), c, 0, 0, 0);
  else return mma(a, b, c);
}
// FIRST: the tile's first K-stage -- the first product into an accumulator starts from zero (no accumulator is ever cleared)
template <int TERMS, int M, int PA, bool FIRST>
__device__ __forceinline__ void mma_rows(const AFrags& A, const BSet<pieces_of(TERMS)>& B, f32x16 (&acc)[3][4]) {
  const f32x16 zero = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
#pragma unroll
  for (int pb = 0; pb < pieces_of(TERMS); ++pb) {
    if ((TERMS == 6 && PA + pb > 2) || (TERMS == 3 && PA + pb > 1)) continue;
#pragma unroll
    for (int p = 0; p < 3; ++p) acc[p][M] = mma_t<TERMS>(A.a[p], B.b[p][pb], FIRST && PA == 0 && pb == 0 ? zero : acc[p][M]);
  }
}
// the order of a region's instructions: behind each matrix instruction its share of the LDS reads, loads, vector arithmetic, writes
template <int NMMA, int NDSR, int NLOAD, int NVALU, int NDSW>
__device__ __forceinline__ void pin_region() {
  constexpr int kValuPer = (NVALU + NMMA - 1) / NMMA;
#pragma unroll
  for (int k = 0; k < NMMA; ++k) {
    __builtin_amdgcn_sched_group_barrier(0x008, 1, 0);
    if (k < NDSR) __builtin_amdgcn_sched_group_barrier(0x100, 1, 0);
    if (k < NLOAD) __builtin_amdgcn_sched_group_barrier(0x020, 1, 0);
    if (NVALU) __builtin_amdgcn_sched_group_barrier(0x002, kValuPer, 0);
    if (k >= NMMA - NDSW) __builtin_amdgcn_sched_group_barrier(0x200, 1, 0);
  }
}

// One K-stage.  On entry: Bc = this stage's B, F0 = the fragments (row quarter 0, piece 0), raw = the raw values of stage g + 2
// (arrived); rd / rd_next = this lane's read address in this stage's / the next stage's LDS buffer, wr = its write address in
// stage g + 2's.  On exit: Bn = the next stage's B (requested), F0 = the next stage's (0, 0), raw = stage g + 4 (requested).
template <int TERMS, bool FIRST>
__device__ __forceinline__ void run_stage_block(const BSet<pieces_of(TERMS)>& Bc, BSet<pieces_of(TERMS)>& Bn, RawA& raw, AFrags& F0,
                                                AFrags& F1, AFrags& F2, AFrags& F3,
                                                f32x16 (&acc)[3][4], const unsigned char* rd, const unsigned char* rd_next,
                                                unsigned char* wr, const TileAt& tb, unsigned sb_off, unsigned b_voff, const TileAt& ta,
                                                unsigned sa_off, unsigned a_voff, unsigned row64, const float scale, BlkClock& clk) {
  constexpr int NP = pieces_of(TERMS);
  constexpr int kN = TERMS == 9 ? 27 : TERMS == 6 ? 18 : 9;   // matrix instructions of a region
  constexpr int kSplit = NP == 3 ? 32 : 20;                   // vector instructions of one split_part (an upper bound for the pinning)
  constexpr int kRd = 3 * NP;                                 // fragments a region reads: pieces 1.. of its row quarter, piece 0 of the next
  clk.tick(0);
  // region m = 0: B of the next stage; row r: re
  __builtin_amdgcn_sched_barrier(0);
  read_frags<NP, 0, 1>(F1, rd);
  if constexpr (NP == 3) read_frags<NP, 0, 2>(F2, rd);
  read_frags<NP, 1, 0>(F3, rd);
  load_bset<NP>(Bn, tb, b_voff, sb_off);
  split_part<NP, 0, 0>(raw, wr, scale);
  mma_rows<TERMS, 0, 0, FIRST>(F0, Bc, acc); mma_rows<TERMS, 0, 1, FIRST>(F1, Bc, acc);
  if constexpr (NP == 3) mma_rows<TERMS, 0, 2, FIRST>(F2, Bc, acc);
  pin_region<kN, kRd, kRd, kSplit, NP>();
  clk.tick(1);
  // region m = 1: row r: im, re + im
  __builtin_amdgcn_sched_barrier(0);
  read_frags<NP, 1, 1>(F1, rd);
  if constexpr (NP == 3) read_frags<NP, 1, 2>(F2, rd);
  read_frags<NP, 2, 0>(F0, rd);
  split_part<NP, 0, 1>(raw, wr, scale); split_part<NP, 0, 2>(raw, wr, scale);
  mma_rows<TERMS, 1, 0, FIRST>(F3, Bc, acc); mma_rows<TERMS, 1, 1, FIRST>(F1, Bc, acc);
  if constexpr (NP == 3) mma_rows<TERMS, 1, 2, FIRST>(F2, Bc, acc);
  pin_region<kN, kRd, 0, 2 * kSplit + 4, 2 * NP>();
  clk.tick(2);
  // region m = 2: row r + 64: re, im
  __builtin_amdgcn_sched_barrier(0);
  read_frags<NP, 2, 1>(F1, rd);
  if constexpr (NP == 3) read_frags<NP, 2, 2>(F2, rd);
  read_frags<NP, 3, 0>(F3, rd);
  split_part<NP, 1, 0>(raw, wr, scale); split_part<NP, 1, 1>(raw, wr, scale);
  mma_rows<TERMS, 2, 0, FIRST>(F0, Bc, acc); mma_rows<TERMS, 2, 1, FIRST>(F1, Bc, acc);
  if constexpr (NP == 3) mma_rows<TERMS, 2, 2, FIRST>(F2, Bc, acc);
  pin_region<kN, kRd, 0, 2 * kSplit, 2 * NP>();
  clk.tick(3);
  // region m = 3: row r + 64: re + im; the raw values of stage g + 4
  __builtin_amdgcn_sched_barrier(0);
  read_frags<NP, 3, 1>(F1, rd);
  if constexpr (NP == 3) read_frags<NP, 3, 2>(F2, rd);
  read_frags<NP, 0, 0>(F0, rd_next);
  split_part<NP, 1, 2>(raw, wr, scale);
  load_raw<0>(raw, ta, a_voff, row64, sa_off);
  mma_rows<TERMS, 3, 0, FIRST>(F3, Bc, acc); mma_rows<TERMS, 3, 1, FIRST>(F1, Bc, acc);
  if constexpr (NP == 3) mma_rows<TERMS, 3, 2, FIRST>(F2, Bc, acc);
  pin_region<kN, kRd, 2, kSplit + 4, NP>();
  __builtin_amdgcn_sched_barrier(0);
  load_raw<1>(raw, ta, a_voff, row64, sa_off);
  clk.tick(4);
  __builtin_amdgcn_sched_barrier(0);
  // the stage's pieces are written (mine: lgkmcnt), every wave is done with the buffer that stage g + 3 will be built in
  asm volatile("s_waitcnt lgkmcnt(0)\n\ts_barrier" ::: "memory");
  clk.stage_end();
}

template <int TERMS>
__global__ __launch_bounds__(256, 1) void fft_cgemm3m_bf16_block_kernel(const float* __restrict__ V, const uint16_t* __restrict__ Bp,
                                                                        float* __restrict__ Mo, int M, int pitch, int Cin, int Cout, int F,
                                                                        int n_rt, int n_cg, int blocks_per_xcd,
                                                                        const float* __restrict__ vbound, int nbound, float b_scale) {
  constexpr int NP = pieces_of(TERMS);
  constexpr int kAStageBytes = a_stage_bytes(TERMS);
  const int lane = threadIdx.x & 63;
  const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const int xcd = blockIdx.x & (kXcd - 1);
  const int q = blockIdx.x >> 3;
  const int S = Cin / kStageK;
  const int tpf = n_rt * n_cg;                                    // block tiles per frequency
  const int nf_x = (F - xcd + kXcd - 1) / kXcd;
  const int total = nf_x * tpf;
  if (q >= total) return;
  BlkClock clk;
  extern __shared__ __attribute__((aligned(16))) unsigned char lds[];      // kABufs * kAStageBytes
  const size_t rowf = (size_t)2 * Cin, mo_row = (size_t)2 * Cout;
  const unsigned b_stage_bytes = (unsigned)(Cout / 32) * 3 * NP * kBFrag;
  const unsigned a_stage = 32u * 4u;
  const unsigned b_voff = lane * 16;
  const unsigned row64 = (unsigned)(64 * rowf * 4);
  // splitter: rows 16 w + (l >> 1 & 15) and + 64, k = 8 (l & 1) + 4 (l >> 5) + t
  const int sp_b = lane & 1, sp_r = (lane >> 1) & 15, sp_h = lane >> 5;
  const int sp_row = 16 * wave + sp_r;
  const unsigned sp_lds = (unsigned)((sp_row >> 5) * 3 * NP * kFragBytes + ((sp_row & 31) + 32 * sp_h) * 16 + 8 * sp_b);
  const unsigned sp_k = (unsigned)(8 * sp_b + 4 * sp_h) * 4u;

  auto locate = [&](int u, TileAt& at, unsigned& aoff, int& f, int& row0, int& ct) {
    const bool live = u < total;
    const int uu = live ? u : 0;
    const int fi = uu / tpf, r = uu - fi * tpf;
    f = xcd + kXcd * fi;
    const int rt = r / n_cg, cg = r - rt * n_cg;
    row0 = rt * kBlkM;
    ct = 4 * cg + wave;                                            // in units of 32 columns
    // past the block's last tile: empty descriptors (the look-ahead reads zeros, no traffic); rows past the pitch likewise
    at.a = __builtin_amdgcn_make_buffer_rsrc(const_cast<float*>(V) + (size_t)f * pitch * rowf, 0, live ? (unsigned)((size_t)pitch * rowf * 4) : 0u, 0x00020000);
    aoff = (unsigned)((size_t)(row0 + sp_row) * rowf * 4) + sp_k;
    at.b = __builtin_amdgcn_make_buffer_rsrc(const_cast<uint16_t*>(Bp) + (size_t)f * S * (b_stage_bytes / 2), 0, live ? (unsigned)S * b_stage_bytes : 0u, 0x00020000);
    at.sb = (unsigned)ct * (3 * NP * kBFrag);
  };

  // three positions in the block's sequence of K-stages: A's loads (4 stages ahead), B's loads (1 ahead), the matrix instructions
  TileAt ta, tb;
  unsigned a_voff, b_unused;
  int ua = q, sa = 0, ub = q, sb = 0;
  int fa, rowa, cta, f, row0, ct;
  locate(q, ta, a_voff, f, row0, ct);
  tb = ta;
  auto next_a = [&]() {
    if (++sa == S) { sa = 0; ua += blocks_per_xcd; locate(ua, ta, a_voff, fa, rowa, cta); }
  };
  auto next_b = [&]() {
    if (++sb == S) { sb = 0; ub += blocks_per_xcd; locate(ub, tb, b_unused, fa, rowa, cta); }
  };

  // TERMS = 3: A is scaled by the power of two that takes the caller's bound of |V| (vbound[0 .. nbound): the largest counts) to
  // 2^14 (re + im then stays below 2^15.5 < 65504); the result is scaled back with B's factor in the epilogue.  Powers of two: exact.
  float a_scale = 1.0f, out_scale = 1.0f;
  if constexpr (TERMS == 3) {
    float mx = 0.0f;
    for (int t = lane; t < nbound; t += 64) mx = fmaxf(mx, vbound[t]);
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) mx = fmaxf(mx, __shfl_xor(mx, o));
    int ex = 0;
    if (mx > 0.0f && mx < 3.0e38f) (void)frexpf(mx, &ex);      // mx <= 2^ex
    ex = min(max(14 - ex, -100), 100);
    ex = __builtin_amdgcn_readfirstlane(ex);
    a_scale = ldexpf(1.0f, ex);
    out_scale = ldexpf(1.0f, -ex) / b_scale;
  }
  RawA raw0, raw1;
  BSet<NP> B0, B1;
  AFrags F0, F1, F2, F3;
  // prologue: stages 0 and 1 of A built in buffers 0 and 1, stages 2 and 3 requested, stage 0 of B requested
  load_raw<0>(raw0, ta, a_voff, row64, sa * a_stage); load_raw<1>(raw0, ta, a_voff, row64, sa * a_stage); next_a();
  load_raw<0>(raw1, ta, a_voff, row64, sa * a_stage); load_raw<1>(raw1, ta, a_voff, row64, sa * a_stage); next_a();
  load_bset<NP>(B0, tb, b_voff, sb * b_stage_bytes); next_b();
  {
    unsigned char* w0p = lds + sp_lds;
    unsigned char* w1p = lds + kAStageBytes + sp_lds;
    split_part<NP, 0, 0>(raw0, w0p, a_scale); split_part<NP, 0, 1>(raw0, w0p, a_scale); split_part<NP, 0, 2>(raw0, w0p, a_scale);
    split_part<NP, 1, 0>(raw0, w0p, a_scale); split_part<NP, 1, 1>(raw0, w0p, a_scale); split_part<NP, 1, 2>(raw0, w0p, a_scale);
    split_part<NP, 0, 0>(raw1, w1p, a_scale); split_part<NP, 0, 1>(raw1, w1p, a_scale); split_part<NP, 0, 2>(raw1, w1p, a_scale);
    split_part<NP, 1, 0>(raw1, w1p, a_scale); split_part<NP, 1, 1>(raw1, w1p, a_scale); split_part<NP, 1, 2>(raw1, w1p, a_scale);
  }
  load_raw<0>(raw0, ta, a_voff, row64, sa * a_stage); load_raw<1>(raw0, ta, a_voff, row64, sa * a_stage); next_a();
  load_raw<0>(raw1, ta, a_voff, row64, sa * a_stage); load_raw<1>(raw1, ta, a_voff, row64, sa * a_stage); next_a();
  asm volatile("s_waitcnt lgkmcnt(0)\n\ts_barrier" ::: "memory");
  unsigned rbuf = 0;                                               // byte offset of the LDS buffer of the stage being multiplied
  read_frags<NP, 0, 0>(F0, lds + lane * 16);
  auto step = [&](unsigned o) { return o + kAStageBytes >= kABufs * kAStageBytes ? o + kAStageBytes - kABufs * kAStageBytes : o + kAStageBytes; };

  for (int u = q; u < total; u += blocks_per_xcd) {
    f32x16 acc[3][4];
#define EQA_STAGE(FIRST, BC, BN, RAW)                                                                                                 \
  {                                                                                                                                  \
    const unsigned r1 = step(rbuf), r2 = step(r1);                                                                                   \
    run_stage_block<TERMS, FIRST>(BC, BN, RAW, F0, F1, F2, F3, acc, lds + rbuf + lane * 16, lds + r1 + lane * 16, lds + r2 + sp_lds, \
                                  tb, sb * b_stage_bytes, b_voff, ta, sa * a_stage, a_voff, row64, a_scale, clk);                            \
    next_a(); next_b();                                                                                                              \
    rbuf = r1;                                                                                                                       \
  }
    EQA_STAGE(true, B0, B1, raw0)
    EQA_STAGE(false, B1, B0, raw1)
    for (int s = 2; s < S; s += 2) {
      EQA_STAGE(false, B0, B1, raw0)
      EQA_STAGE(false, B1, B0, raw1)
    }
#undef EQA_STAGE
    // Cr = T1 - T2, Ci = T3 - T1 - T2, straight from the accumulators: lane (i, h), slot e = row (e & 3) + 8 (e >> 2) + 4 h, column i
    clk.tile_epilogue_begin();
    {
      const int rows = __builtin_amdgcn_readfirstlane(min(kBlkM, M - row0));
      const __amdgpu_buffer_rsrc_t dr =
          __builtin_amdgcn_make_buffer_rsrc(Mo + ((size_t)f * pitch + row0) * mo_row, 0, (unsigned)(rows * mo_row * 4), 0x00020000);
      const int i = lane & 31, h = lane >> 5;
      const unsigned voff = (unsigned)((4 * h * mo_row + (size_t)(32 * ct + i) * 2) * 4);
#pragma unroll
      for (int m = 0; m < 4; ++m)
#pragma unroll
        for (int e = 0; e < 16; ++e) {
          const unsigned roff = voff + (unsigned)((32 * m + (e & 3) + 8 * (e >> 2)) * mo_row * 4);     // in the range-checked offset
          const float t1 = acc[0][m][e], t2 = acc[1][m][e], t3 = acc[2][m][e];
          u32x2 c;
          c[0] = __builtin_bit_cast(unsigned, TERMS == 3 ? (t1 - t2) * out_scale : t1 - t2);
          c[1] = __builtin_bit_cast(unsigned, TERMS == 3 ? (t3 - t1 - t2) * out_scale : t3 - t1 - t2);
          __builtin_amdgcn_raw_buffer_store_b64(c, dr, roff, 0, 0);
        }
    }
    int nf, nrow0, nct;
    TileAt unused_t;
    unsigned unused_o;
    locate(u + blocks_per_xcd, unused_t, unused_o, nf, nrow0, nct);
    f = nf; row0 = nrow0; ct = nct;
    clk.tile_epilogue_end();
  }
  clk.publish();
}

// B3 (F, S, Cout/32, 3, 2, 64, 4) fp32 -> Bp (F, S, Cout/32, 3, 3, 64, 8) bf16: one thread per (f, s, column tile, part, lane)
__global__ __launch_bounds__(256) void spectra3m_split_kernel(const float* __restrict__ B3, uint16_t* __restrict__ Bp, size_t groups) {
  const size_t t = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (t >= groups * 64) return;
  const size_t g = t >> 6;            // (f, s, nt, part)
  const int lane = (int)(t & 63);
  const float* src = B3 + g * (2 * 64 * 4) + lane * 4;
  const f32x4 lo = *reinterpret_cast<const f32x4*>(src), hi = *reinterpret_cast<const f32x4*>(src + 64 * 4);
  const Pieces p = split8(lo, hi);
  u32x4* dst = reinterpret_cast<u32x4*>(Bp + g * (3 * 64 * 8)) + lane;
#pragma unroll
  for (int q = 0; q < 3; ++q) dst[q * 64] = p.p[q];
}


// ... -> Bh (F, S, Cout/32, 3, 2, 64, 8) fp16: the two pieces of b_scale * B3 (b_scale: a power of two that takes max |B3| to 2^14)
__global__ __launch_bounds__(256) void spectra3m_split_f16_kernel(const float* __restrict__ B3, uint16_t* __restrict__ Bh, size_t groups,
                                                                  float b_scale) {
  const size_t t = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (t >= groups * 64) return;
  const size_t g = t >> 6;            // (f, s, nt, part)
  const int lane = (int)(t & 63);
  const float* src = B3 + g * (2 * 64 * 4) + lane * 4;
  const f32x4 lo = *reinterpret_cast<const f32x4*>(src) * b_scale, hi = *reinterpret_cast<const f32x4*>(src + 64 * 4) * b_scale;
  u32x2 a[2], b[2];
  split4h(lo, a);
  split4h(hi, b);
  u32x4* dst = reinterpret_cast<u32x4*>(Bh + g * (2 * 64 * 8)) + lane;
#pragma unroll
  for (int q = 0; q < 2; ++q) {
    const u32x4 v = {a[q][0], a[q][1], b[q][0], b[q][1]};
    dst[q * 64] = v;
  }
}

// the block form's launch: 128 x 128 tiles, one block per CU, three K-stages of A's pieces in dynamic LDS
template <int TERMS>
int launch_block(const float* V, const void* B, float* Mo, int64_t M, int Cin, int Cout, const float* vbound, int nbound, float b_scale,
                 void* stream) {
  const int n_rb = (int)((M + kBlkM - 1) / kBlkM), n_cg = Cout / kBlkN;
  constexpr int kLds = kABufs * a_stage_bytes(TERMS);
  if (!allow_dynamic_lds((const void*)fft_cgemm3m_bf16_block_kernel<TERMS>, kLds)) return EQA_ERR_LAUNCH;
  hipLaunchKernelGGL((fft_cgemm3m_bf16_block_kernel<TERMS>), dim3(kGridBlocks), dim3(256), kLds, (hipStream_t)stream, V,
                     static_cast<const uint16_t*>(B), Mo, (int)M, (int)eqa_fft48k5_tile_pitch(M), Cin, Cout, eqa_fft48k5_frequencies(), n_rb,
                     n_cg, kBlocksPerXcd, vbound, nbound, b_scale);
  return launch_status();
}

// ---------------------------------------------------------------------------------------------------------------------------
// The fp16 block form on v_mfma_f32_16x16x32_f16 (round 27).  Same operands, same two-piece split, same three products
// (h1 k1 + h1 k2 + h2 k1), same 3M arithmetic and scaling as TERMS = 3 above; what differs is the instruction shape -- the chip
// holds a higher clock on 16x16x32 than on 32x32x16 at equal cycles per FLOP -- and with it the K-stage, the fragment orders and
// the store map.  The sum inside an accumulator now runs over 32 k per rounding instead of 16.
//   work: as above -- a block per 128 x 128 tile of one frequency, wave w on columns 32 w .. 32 w + 31 of all 128 rows, one wave per
//        SIMD, the XCD-aware persistent walk, the bound reduction, range-checked descriptors.
//   wave tile: 8 row tiles x 2 column tiles x 3 parts = 48 accumulators of 4 registers.  Lane l of an instruction holds
//        A[row l & 15][k = 8 (l >> 4) + j], B[k = 8 (l >> 4) + j][column l & 15], C[row 4 (l >> 4) + reg][column l & 15].
//   K-stage: 32 complex k = two consecutive [16 re | 16 im] groups of V.  A's pieces of a stage: 48 fragments [row tile][part]
//        [piece] of 64 lanes x 16 bytes = 48 KB; three buffers (144 KB), stage g + 2 written while g is multiplied and g + 1
//        stands published: ONE barrier per stage, Cin / 32 per tile (half of the form above).
//   splitter: thread (wave w, lane l) owns rows 16 w + (l >> 1 & 15) and + 64 (row tiles w and w + 4), k = 8 (l >> 5) + 4 (l & 1)
//        + 0..3 and + 16 of the stage: eight 16-byte loads, 48 values split, twenty-four 8-byte LDS writes to lane
//        (r & 15) + 16 (k >> 3), byte 2 (k & 7) of the fragment (the 64 lanes of a write cover 512 contiguous bytes: no conflict).
//        The raw values of stage g + 3 are requested group by group as those of g + 2 have been split: A two of the old stages
//        ahead of the LDS image, B (12 fragments, 48 registers, a second set) one stage ahead -- the depth in bytes of the form above.
//   matrix instructions of a stage: eight regions (row tile), each the row tile's 6 A fragments against the 12 B fragments:
//        18 instructions, six independent accumulators in a row (2 column tiles x 3 parts) per (A piece, B piece); a region
//        reads its own piece-1 fragments and the next row tile's piece-0 fragments behind its first six instructions.  The next
//        stage's B is asked for three fragments per region over the first four: all twelve behind the stage's barrier, from four
//        waves at once, held the first region for ~800 cycles (profiles/r27/README.md).
//   B: (F, Cin/32, Cout/32, 2 column tiles, 3 parts, 2 pieces, 64 lanes, 8 fp16); column tile t, lane column i = output channel
//        32 c + 2 i + t, so lane (i, q) holds (Cr, Ci) of channels 2 i and 2 i + 1 for rows 4 q .. 4 q + 3 of a row tile:
//        16-byte stores, 32 per wave and tile, 256 contiguous bytes per row.
constexpr int kK32AStageBytes = 8 * 3 * 2 * kFragBytes;        // 48 KB
constexpr unsigned kK32BTileBytes = 2 * 3 * 2 * kBFrag;        // Bk per (K-stage, 32 columns)

struct BSet32 {
  u32x4 b[2][3][2];               // [column tile][part][piece]
};
struct AFrags32 {
  u32x4 a[3];                     // [part] of one (row tile, piece)
};
struct RawA32 {
  f32x4 re[2][2], im[2][2];       // [rows r, r + 64][k group of 16]
};

// split4h with the remainder taken by one mixed-precision multiply-add per value (v_fma_mix_f32: a - h with h read as fp16, exact
// as the subtraction is) instead of a conversion and a subtraction: a 16x16x32 instruction leaves the vector issue half the room of
// a 32x32x16 one, and the split is what fills it.  The same pieces, bit for bit.  `m1` is -1 in a register the compiler cannot see
// through (written as a constant, the multiply-add is folded back into the subtraction).
__device__ __forceinline__ void split4h_mix(const f32x4 v, u32x2 (&o)[2], const float m1) {
#pragma unroll
  for (int j = 0; j < 2; ++j) {
    const float a = v[2 * j], b = v[2 * j + 1];
    const f16x2v hr = {(_Float16)a, (_Float16)b};
    unsigned hp = __builtin_bit_cast(unsigned, hr);
    asm("" : "+v"(hp));                               // the packed pair is the multiply-add's source: no second conversion per half
    const f16x2v h = __builtin_bit_cast(f16x2v, hp);
    const f16x2v l = {(_Float16)__builtin_fmaf((float)h[0], m1, a), (_Float16)__builtin_fmaf((float)h[1], m1, b)};
    o[0][j] = hp;
    o[1][j] = __builtin_bit_cast(unsigned, l);
  }
}
// one part of (row ROW, k group KG)'s 4 k: scaled, split, two 8-byte writes into the stage being built (row r + 64 is row tile
// w + 4: 24 fragments further; k group 1 is lanes 32..63 of the fragment: 512 bytes further)
template <int ROW, int KG, int PART>
__device__ __forceinline__ void split_part32(const RawA32& r, unsigned char* wr, const float scale, const float m1) {
  // element by element: on the whole vector the sum and the scaling come out as packed fp32 instructions, which cost more than two
  // plain ones beside matrix instructions
  f32x4 v;
#pragma unroll
  for (int e = 0; e < 4; ++e) v[e] = (PART == 0 ? r.re[ROW][KG][e] : PART == 1 ? r.im[ROW][KG][e] : r.re[ROW][KG][e] + r.im[ROW][KG][e]) * scale;
  u32x2 o[2];
  split4h_mix(v, o, m1);
#pragma unroll
  for (int q = 0; q < 2; ++q) *reinterpret_cast<u32x2*>(wr + (ROW * 24 + PART * 2 + q) * kFragBytes + KG * 512) = o[q];
}
template <int ROW, int KG>
__device__ __forceinline__ void split_group32(const RawA32& r, unsigned char* wr, const float scale, const float m1) {
  split_part32<ROW, KG, 0>(r, wr, scale, m1); split_part32<ROW, KG, 1>(r, wr, scale, m1); split_part32<ROW, KG, 2>(r, wr, scale, m1);
}
template <int ROW, int KG>
__device__ __forceinline__ void load_raw32(RawA32& o, const TileAt& t, unsigned voff, unsigned row64, unsigned soff) {
  o.re[ROW][KG] = buf_ld<f32x4>(t.a, voff + ROW * row64 + KG * 128, soff);
  o.im[ROW][KG] = buf_ld<f32x4>(t.a, voff + ROW * row64 + KG * 128 + 64, soff);
}
__device__ __forceinline__ void load_stage32(RawA32& o, const TileAt& t, unsigned voff, unsigned row64, unsigned soff) {
  load_raw32<0, 0>(o, t, voff, row64, soff); load_raw32<0, 1>(o, t, voff, row64, soff);
  load_raw32<1, 0>(o, t, voff, row64, soff); load_raw32<1, 1>(o, t, voff, row64, soff);
}
// fragments K0 .. K0 + N - 1 of a stage's 12
template <int K0, int N>
__device__ __forceinline__ void load_bset32(BSet32& o, const TileAt& t, unsigned voff, unsigned soff) {
#pragma unroll
  for (int k = K0; k < K0 + N; ++k) o.b[k / 6][(k / 2) % 3][k % 2] = buf_ld<u32x4>(t.b, voff + k * kBFrag, t.sb + soff);
}
template <int RT, int PA>
__device__ __forceinline__ void read_frags32(AFrags32& o, const unsigned char* rd) {
#pragma unroll
  for (int p = 0; p < 3; ++p) o.a[p] = *reinterpret_cast<const u32x4*>(rd + (RT * 6 + p * 2 + PA) * kFragBytes);
}
__device__ __forceinline__ f32x4 mma16(const u32x4 a, const u32x4 b, const f32x4 c) {
  return __builtin_amdgcn_mfma_f32_16x16x32_f16(__builtin_bit_cast(f16x8, a), __builtin_bit_cast(f16x8, b), c, 0, 0, 0);
}
// the 18 matrix instructions of row tile RT: h1 k1, h1 k2, h2 k1, each over the six accumulators (column tile, part) in a row
template <int RT, bool FIRST>
__device__ __forceinline__ void mma_row_tile(const AFrags32& A0, const AFrags32& A1, const BSet32& B, f32x4 (&acc)[3][8][2]) {
  const f32x4 zero = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
  for (int w = 0; w < 3; ++w) {
    const int pa = w == 2 ? 1 : 0, pb = w == 1 ? 1 : 0;
#pragma unroll
    for (int t = 0; t < 2; ++t)
#pragma unroll
      for (int p = 0; p < 3; ++p) acc[p][RT][t] = mma16(pa ? A1.a[p] : A0.a[p], B.b[t][p][pb], FIRST && w == 0 ? zero : acc[p][RT][t]);
  }
}

// An accumulator element where the epilogue wants it: left to the register allocator, the 192 reads of a tile are all hoisted in
// front of the first store and take the invariants of the stage loop out of the file.  (The compiler pads nothing around inline
// assembly: the tile epilogue opens with the wait states a matrix instruction's result asks for before it is read.)
__device__ __forceinline__ float acc_read(const float a) {
  float v;
  asm volatile("v_accvgpr_read_b32 %0, %1" : "=v"(v) : "a"(a));
  return v;
}

// One K-stage of 32.  On entry: Bc = this stage's B, FA = the fragments (row tile 0, piece 0), raw = the raw values of stage g + 2
// (arrived); rd / rd_next / wr as in run_stage_block.  On exit: Bn = the next stage's B (requested), FA = the next stage's (row
// tile 0, piece 0), raw = stage g + 3 (requested).  Regions 2 j and 2 j + 1 split raw group j = (rows r / r + 64, k group) -- one part in the
// first, two in the second -- and the group's registers are asked for again behind the second.
template <bool FIRST>
__device__ __forceinline__ void run_stage_k32(const BSet32& Bc, BSet32& Bn, RawA32& raw, AFrags32& FA, AFrags32& FB, AFrags32& F1,
                                              f32x4 (&acc)[3][8][2], const unsigned char* rd, const unsigned char* rd_next, unsigned char* wr, const TileAt& tb,
                                              unsigned sb_off, unsigned b_voff, const TileAt& ta, unsigned sa_off, unsigned a_voff,
                                              unsigned row64, const float scale, const float m1, BlkClock& clk) {
  constexpr int kN = 18, kRd = 6, kSplit = 12;
  clk.tick(0);
#define EQA_REGION_PAIR(J, ROW, KG, NLOAD, RD_LAST)                                                                         \
  __builtin_amdgcn_sched_barrier(0);                                                                                         \
  read_frags32<2 * J, 1>(F1, rd); read_frags32<2 * J + 1, 0>(FB, rd);                                                                                        \
  load_bset32<6 * J, NLOAD>(Bn, tb, b_voff, sb_off);                                                                          \
  split_part32<ROW, KG, 0>(raw, wr, scale, m1);                                                                                \
  mma_row_tile<2 * J, FIRST>(FA, F1, Bc, acc);                                                                                \
  pin_region<kN, kRd, NLOAD, kSplit, 2>();                                                                                   \
  __builtin_amdgcn_sched_barrier(0);                                                                                         \
  read_frags32<2 * J + 1, 1>(F1, rd); read_frags32<(2 * J + 2) & 7, 0>(FA, RD_LAST);                                        \
  load_bset32<6 * J + NLOAD, NLOAD>(Bn, tb, b_voff, sb_off);                                                                             \
  split_part32<ROW, KG, 1>(raw, wr, scale, m1); split_part32<ROW, KG, 2>(raw, wr, scale, m1);                                \
  mma_row_tile<2 * J + 1, FIRST>(FB, F1, Bc, acc);                                                                            \
  pin_region<kN, kRd, NLOAD, 2 * kSplit + 4, 4>();                                                                             \
  __builtin_amdgcn_sched_barrier(0);                                                                                         \
  load_raw32<ROW, KG>(raw, ta, a_voff, row64, sa_off);                                                                       \
  clk.tick(J + 1);
  EQA_REGION_PAIR(0, 0, 0, 3, rd)
  EQA_REGION_PAIR(1, 0, 1, 3, rd)
  EQA_REGION_PAIR(2, 1, 0, 0, rd)
  EQA_REGION_PAIR(3, 1, 1, 0, rd_next)
#undef EQA_REGION_PAIR
  __builtin_amdgcn_sched_barrier(0);
  // the stage's pieces are written (mine: lgkmcnt), every wave is done with the buffer that stage g + 3 will be built in
  asm volatile("s_waitcnt lgkmcnt(0)\n\ts_barrier" ::: "memory");
  clk.stage_end();
}

// ODD: Cin / 32 is odd
template <bool ODD>
__global__ __launch_bounds__(256, 1) void fft_cgemm3m_f16_k32_block_kernel(const float* __restrict__ V, const uint16_t* __restrict__ Bk,
                                                                           float* __restrict__ Mo, int M, int pitch, int Cin, int Cout, int F,
                                                                           int n_rt, int n_cg, int blocks_per_xcd,
                                                                           const float* __restrict__ vbound, int nbound, float b_scale) {
  const int lane = threadIdx.x & 63;
  const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const int xcd = blockIdx.x & (kXcd - 1);
  const int q = blockIdx.x >> 3;
  const int S = Cin / 32;
  const int tpf = n_rt * n_cg;                                    // block tiles per frequency
  const int nf_x = (F - xcd + kXcd - 1) / kXcd;
  const int total = nf_x * tpf;
  if (q >= total) return;
  BlkClock clk;
  extern __shared__ __attribute__((aligned(16))) unsigned char lds[];      // kABufs * kK32AStageBytes
  const size_t rowf = (size_t)2 * Cin, mo_row = (size_t)2 * Cout;
  const unsigned b_stage_bytes = (unsigned)(Cout / 32) * kK32BTileBytes;
  const unsigned a_stage = 64u * 4u;
  const unsigned b_voff = lane * 16;
  const unsigned row64 = (unsigned)(64 * rowf * 4);
  // splitter: rows 16 w + (l >> 1 & 15) and + 64, k = 8 (l >> 5) + 4 (l & 1) + t and + 16
  const int sp_b = lane & 1, sp_r = (lane >> 1) & 15, sp_h = lane >> 5;
  const int sp_row = 16 * wave + sp_r;
  const unsigned sp_lds = (unsigned)(wave * 6 * kFragBytes + (sp_r + 16 * sp_h) * 16 + 8 * sp_b);
  const unsigned sp_k = (unsigned)(8 * sp_h + 4 * sp_b) * 4u;

  auto locate = [&](int u, TileAt& at, unsigned& aoff, int& f, int& row0, int& ct) {
    const bool live = u < total;
    const int uu = live ? u : 0;
    const int fi = uu / tpf, r = uu - fi * tpf;
    f = xcd + kXcd * fi;
    const int rt = r / n_cg, cg = r - rt * n_cg;
    row0 = rt * kBlkM;
    ct = 4 * cg + wave;                                            // in units of 32 columns
    // past the block's last tile: empty descriptors (the look-ahead reads zeros, no traffic); rows past the pitch likewise
    at.a = __builtin_amdgcn_make_buffer_rsrc(const_cast<float*>(V) + (size_t)f * pitch * rowf, 0, live ? (unsigned)((size_t)pitch * rowf * 4) : 0u, 0x00020000);
    aoff = (unsigned)((size_t)(row0 + sp_row) * rowf * 4) + sp_k;
    at.b = __builtin_amdgcn_make_buffer_rsrc(const_cast<uint16_t*>(Bk) + (size_t)f * S * (b_stage_bytes / 2), 0, live ? (unsigned)S * b_stage_bytes : 0u, 0x00020000);
    at.sb = (unsigned)ct * kK32BTileBytes;
  };

  // three positions in the block's sequence of K-stages: A's loads (3 stages ahead), B's loads (1 ahead), the matrix instructions
  TileAt ta, tb;
  unsigned a_voff, b_unused;
  int ua = q, sa = 0, ub = q, sb = 0;
  int fa, rowa, cta, f, row0, ct;
  locate(q, ta, a_voff, f, row0, ct);
  tb = ta;
  auto next_a = [&]() {
    if (++sa == S) { sa = 0; ua += blocks_per_xcd; locate(ua, ta, a_voff, fa, rowa, cta); }
  };
  auto next_b = [&]() {
    if (++sb == S) { sb = 0; ub += blocks_per_xcd; locate(ub, tb, b_unused, fa, rowa, cta); }
  };

  // the scaling of the form above: the caller's bound of |V| goes to 2^14, the result is scaled back with B's factor
  float mx = 0.0f;
  for (int t = lane; t < nbound; t += 64) mx = fmaxf(mx, vbound[t]);
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) mx = fmaxf(mx, __shfl_xor(mx, o));
  int ex = 0;
  if (mx > 0.0f && mx < 3.0e38f) (void)frexpf(mx, &ex);      // mx <= 2^ex
  ex = min(max(14 - ex, -100), 100);
  ex = __builtin_amdgcn_readfirstlane(ex);
  const float a_scale = ldexpf(1.0f, ex);
  const float out_scale = ldexpf(1.0f, -ex) / b_scale;
  float m1 = -1.0f;
  asm volatile("" : "+s"(m1));

  RawA32 raw;
  BSet32 B0, B1;
  AFrags32 FA, FB, F1;
  // prologue: stages 0 and 1 of A built in buffers 0 and 1, stage 2 requested, stage 0 of B requested
  load_stage32(raw, ta, a_voff, row64, sa * a_stage); next_a();
  load_bset32<0, 12>(B0, tb, b_voff, sb * b_stage_bytes); next_b();
#pragma unroll
  for (int g = 0; g < 2; ++g) {
    unsigned char* wp = lds + g * kK32AStageBytes + sp_lds;
    split_group32<0, 0>(raw, wp, a_scale, m1); split_group32<0, 1>(raw, wp, a_scale, m1);
    split_group32<1, 0>(raw, wp, a_scale, m1); split_group32<1, 1>(raw, wp, a_scale, m1);
    load_stage32(raw, ta, a_voff, row64, sa * a_stage); next_a();
  }
  asm volatile("s_waitcnt lgkmcnt(0)\n\ts_barrier" ::: "memory");
  unsigned rbuf = 0;                                               // byte offset of the LDS buffer of the stage being multiplied
  read_frags32<0, 0>(FA, lds + lane * 16);
  auto step = [&](unsigned o) { return o + kK32AStageBytes >= kABufs * kK32AStageBytes ? o + kK32AStageBytes - kABufs * kK32AStageBytes : o + kK32AStageBytes; };
  // Cr = T1 - T2, Ci = T3 - T1 - T2, straight from the accumulators: lane (i, q4), register e = row 16 rt + 4 q4 + e, channels
  // 32 ct + 2 i (column tile 0) and + 1 (column tile 1); then the coordinates of the block's next tile
#define EQA_FINISH_TILE32 {                                                                                                                 \
    clk.tile_epilogue_begin();                                                                                                              \
    asm volatile("s_nop 7\n\ts_nop 7\n\ts_nop 3");                                                                                          \
    {                                                                                                                                       \
      const int rows = __builtin_amdgcn_readfirstlane(min(kBlkM, M - row0));                                                                \
      const __amdgpu_buffer_rsrc_t dr =                                                                                                     \
          __builtin_amdgcn_make_buffer_rsrc(Mo + ((size_t)f * pitch + row0) * mo_row, 0, (unsigned)(rows * mo_row * 4), 0x00020000);        \
      const int i = lane & 15, q4 = lane >> 4;                                                                                              \
      const unsigned voff = (unsigned)((4 * q4 * mo_row + (size_t)(32 * ct + 2 * i) * 2) * 4);                                              \
_Pragma("unroll")                                                                                                                           \
      for (int rt = 0; rt < 8; ++rt) {                                                                                                      \
_Pragma("unroll")                                                                                                                           \
        for (int e = 0; e < 4; ++e) {                                                                                                       \
          const unsigned roff = voff + (unsigned)((16 * rt + e) * mo_row * 4);                                                              \
          u32x4 c;                                                                                                                          \
_Pragma("unroll")                                                                                                                           \
          for (int t = 0; t < 2; ++t) {                                                                                                     \
            const float t1 = acc_read(acc[0][rt][t][e]), t2 = acc_read(acc[1][rt][t][e]), t3 = acc_read(acc[2][rt][t][e]);                  \
            c[2 * t] = __builtin_bit_cast(unsigned, (t1 - t2) * out_scale);                                                                 \
            c[2 * t + 1] = __builtin_bit_cast(unsigned, (t3 - t1 - t2) * out_scale);                                                        \
          }                                                                                                                                 \
          __builtin_amdgcn_raw_buffer_store_b128(c, dr, roff, 0, 0);                                                                        \
        }                                                                                                                                   \
      }                                                                                                                                     \
    }                                                                                                                                       \
    int nf, nrow0, nct;                                                                                                                     \
    TileAt unused_t;                                                                                                                        \
    unsigned unused_o;                                                                                                                      \
    locate(u + blocks_per_xcd, unused_t, unused_o, nf, nrow0, nct);                                                                         \
    f = nf; row0 = nrow0; ct = nct;                                                                                                         \
    clk.tile_epilogue_end();                                                                                                                \
  }                                                                                                                                         

  // B0 / B1 swap roles from stage to stage, statically: an even Cin / 32 brings every tile back to B0; an odd one (96, 160) makes the
  // block's tiles alternate, so its loop body is two tiles
#define EQA_STAGE32(FIRST, BC, BN)                                                                                              \
  {                                                                                                                            \
    const unsigned r1 = step(rbuf), r2 = step(r1);                                                                             \
    run_stage_k32<FIRST>(BC, BN, raw, FA, FB, F1, acc, lds + rbuf + lane * 16, lds + r1 + lane * 16, lds + r2 + sp_lds, tb,        \
                         sb * b_stage_bytes, b_voff, ta, sa * a_stage, a_voff, row64, a_scale, m1, clk);                         \
    next_a(); next_b();                                                                                                        \
    rbuf = r1;                                                                                                                 \
  }
#define EQA_TILE32(BX, BY)                                                                                                      \
  {                                                                                                                            \
    f32x4 acc[3][8][2];                                                                                                        \
    EQA_STAGE32(true, BX, BY)                                                                                                  \
    if constexpr (ODD) {                                                                                                       \
      for (int s = 1; s < S; s += 2) {                                                                                         \
        EQA_STAGE32(false, BY, BX)                                                                                             \
        EQA_STAGE32(false, BX, BY)                                                                                             \
      }                                                                                                                        \
    } else {                                                                                                                   \
      EQA_STAGE32(false, BY, BX)                                                                                               \
      for (int s = 2; s < S; s += 2) {                                                                                         \
        EQA_STAGE32(false, BX, BY)                                                                                             \
        EQA_STAGE32(false, BY, BX)                                                                                             \
      }                                                                                                                        \
    }                                                                                                                          \
    EQA_FINISH_TILE32                                                                                                              \
    u += blocks_per_xcd;                                                                                                       \
  }
  for (int u = q; u < total;) {
    EQA_TILE32(B0, B1)
    if constexpr (ODD) {
      if (u >= total) break;
      EQA_TILE32(B1, B0)
    }
  }
#undef EQA_TILE32
#undef EQA_FINISH_TILE32
#undef EQA_STAGE32
  clk.publish();
}

// B3 (F, Cin/16, Cout/32, 3, 2, 64, 4) fp32 -> Bk (F, Cin/32, Cout/32, 2 column tiles, 3 parts, 2 pieces, 64 lanes, 8) fp16: the
// two pieces of b_scale * B3 in the fragment order of the 16x16x32 instruction, one thread per (f, stage, c, column tile, part, lane).
// Lane l holds k = 8 (l >> 4) + j of the 32-k stage (the old stage 2 S + (l >> 5), its slot b = (l >> 4) & 1, h = j >> 2, t = j & 3)
// and column 2 (l & 15) + column tile of the 32.
__global__ __launch_bounds__(256) void spectra3m_split_f16_k32_kernel(const float* __restrict__ B3, uint16_t* __restrict__ Bk, size_t groups,
                                                                      int NT, float b_scale) {
  const size_t t = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (t >= groups * 64) return;
  size_t g = t >> 6;                  // (f, S, c, column tile, part)
  const int lane = (int)(t & 63);
  const int part = (int)(g % 3); g /= 3;
  const int tile = (int)(g % 2); g /= 2;
  const int c = (int)(g % NT); g /= NT;      // g: f * (Cin / 32) + S
  const size_t s16 = 2 * g + (lane >> 5);
  const float* src = B3 + ((((s16 * NT + c) * 3 + part) * 2 + ((lane >> 4) & 1)) * 64 + 2 * (lane & 15) + tile) * 4;
  const f32x4 lo = *reinterpret_cast<const f32x4*>(src) * b_scale, hi = *reinterpret_cast<const f32x4*>(src + 32 * 4) * b_scale;
  u32x2 a[2], b[2];
  split4h(lo, a);
  split4h(hi, b);
  u32x4* dst = reinterpret_cast<u32x4*>(Bk + (t >> 6) * (2 * 64 * 8)) + lane;
#pragma unroll
  for (int q = 0; q < 2; ++q) {
    const u32x4 v = {a[q][0], a[q][1], b[q][0], b[q][1]};
    dst[q * 64] = v;
  }
}

}  // namespace

namespace eqa {
int g_cgemm_bf16_form = 0;     // eqa_set_option key 2: 0 = the block form where it applies (Cout % 128 == 0), 1 = always the wave form
}

extern "C" {

int64_t eqa_fft48k5_spectra3m_bf16_bytes(int Cin, int Cout) {
  if (!eqa_fft48k5_cgemm3m_supported(Cin, Cout)) return 0;
  return (int64_t)eqa_fft48k5_frequencies() * Cin * Cout * 3 * 3 * 2;
}

int eqa_fft48k5_spectra3m_split(const float* B3, void* Bp, int Cin, int Cout, void* stream) {
  if (!B3 || !Bp) return EQA_ERR_INVALID_ARG;
  if (!eqa_fft48k5_cgemm3m_supported(Cin, Cout) || (((uintptr_t)B3 | (uintptr_t)Bp) & 15)) return EQA_ERR_UNSUPPORTED;
  const size_t groups = (size_t)eqa_fft48k5_frequencies() * (Cin / kStageK) * (Cout / 32) * 3;
  const size_t threads = groups * 64;
  hipLaunchKernelGGL(spectra3m_split_kernel, dim3((unsigned)((threads + 255) / 256)), dim3(256), 0, (hipStream_t)stream, B3,
                     static_cast<uint16_t*>(Bp), groups);
  return launch_status();
}

int eqa_fft48k5_cgemm3m_bf16x3(const float* V, const void* Bp, float* Mo, int64_t M, int Cin, int Cout, int terms, void* stream) {
  if (terms != 9 && terms != 6) return EQA_ERR_INVALID_ARG;
  const int st = check_contraction_args(V, Bp, Mo, M, Cin, Cout);
  if (st != EQA_OK) return st == kNothingToDo ? EQA_OK : st;
  if ((int64_t)Cin * Cout * 9 * 2 > 0x7fffffffLL) return EQA_ERR_UNSUPPORTED;      // one frequency of Bp: a descriptor range
  if (Cout % kBlkN == 0 && eqa::g_cgemm_bf16_form != 1) {      // the block form: A split once per block, shared through LDS
    return terms == 9 ? launch_block<9>(V, Bp, Mo, M, Cin, Cout, nullptr, 0, 1.0f, stream)
                      : launch_block<6>(V, Bp, Mo, M, Cin, Cout, nullptr, 0, 1.0f, stream);
  }
  const int F = eqa_fft48k5_frequencies();
  const int n_rt = (int)((M + kTileM - 1) / kTileM), n_ct = Cout / kTileN;
  const int S = Cin / kStageK;
#define EQA_CG_LAUNCH(NP, T)                                                                                                            \
  hipLaunchKernelGGL((fft_cgemm3m_bf16_kernel<NP, T>), dim3(kGridBlocks), dim3(256), 0, (hipStream_t)stream, V,                         \
                     static_cast<const uint16_t*>(Bp), Mo, (int)M, (int)eqa_fft48k5_tile_pitch(M), Cin, Cout, F, n_rt, n_ct, kWavesPerXcd)
#define EQA_CG_TERMS(NP) do { if (terms == 9) EQA_CG_LAUNCH(NP, 9); else EQA_CG_LAUNCH(NP, 6); } while (0)
  switch (32 % S == 0 ? 32 / S : 0) {
    case 4: EQA_CG_TERMS(4); break;
    case 2: EQA_CG_TERMS(2); break;
    case 1: EQA_CG_TERMS(1); break;
    default: EQA_CG_TERMS(0); break;
  }
#undef EQA_CG_TERMS
#undef EQA_CG_LAUNCH
  return launch_status();
}


int64_t eqa_fft48k5_spectra3m_f16_bytes(int Cin, int Cout) {
  if (!eqa_fft48k5_cgemm3m_supported(Cin, Cout) || Cout % kBlkN != 0) return 0;
  return (int64_t)eqa_fft48k5_frequencies() * Cin * Cout * 3 * 2 * 2;
}

int eqa_fft48k5_spectra3m_split_f16(const float* B3, void* Bh, int Cin, int Cout, float b_scale, void* stream) {
  if (!B3 || !Bh || !(b_scale > 0.0f)) return EQA_ERR_INVALID_ARG;
  if (eqa_fft48k5_spectra3m_f16_bytes(Cin, Cout) == 0 || (((uintptr_t)B3 | (uintptr_t)Bh) & 15)) return EQA_ERR_UNSUPPORTED;
  int ex = 0;
  if (frexpf(b_scale, &ex) != 0.5f) return EQA_ERR_INVALID_ARG;            // a power of two: the scaling must be exact
  const size_t groups = (size_t)eqa_fft48k5_frequencies() * (Cin / kStageK) * (Cout / 32) * 3;
  const size_t threads = groups * 64;
  hipLaunchKernelGGL(spectra3m_split_f16_kernel, dim3((unsigned)((threads + 255) / 256)), dim3(256), 0, (hipStream_t)stream, B3,
                     static_cast<uint16_t*>(Bh), groups, b_scale);
  return launch_status();
}

int eqa_fft48k5_cgemm3m_f16x2(const float* V, const void* Bh, float* Mo, int64_t M, int Cin, int Cout, const float* vbound, int nbound,
                              float b_scale, void* stream) {
  if (!vbound || nbound <= 0 || !(b_scale > 0.0f)) return EQA_ERR_INVALID_ARG;
  const int st = check_contraction_args(V, Bh, Mo, M, Cin, Cout);
  if (st != EQA_OK) return st == kNothingToDo ? EQA_OK : st;
  // the block form only; its K loop runs stage pairs; one frequency of Bh: a descriptor range
  if (Cout % kBlkN != 0 || (Cin / kStageK) % 2 != 0 || (int64_t)Cin * Cout * 6 * 2 > 0x7fffffffLL) return EQA_ERR_UNSUPPORTED;
  return launch_block<3>(V, Bh, Mo, M, Cin, Cout, vbound, nbound, b_scale, stream);
}

int eqa_fft48k5_spectra3m_split_f16_k32(const float* B3, void* Bk, int Cin, int Cout, float b_scale, void* stream) {
  if (!B3 || !Bk || !(b_scale > 0.0f)) return EQA_ERR_INVALID_ARG;
  if (eqa_fft48k5_spectra3m_f16_bytes(Cin, Cout) == 0 || (((uintptr_t)B3 | (uintptr_t)Bk) & 15)) return EQA_ERR_UNSUPPORTED;
  int ex = 0;
  if (frexpf(b_scale, &ex) != 0.5f) return EQA_ERR_INVALID_ARG;            // a power of two: the scaling must be exact
  const size_t groups = (size_t)eqa_fft48k5_frequencies() * (Cin / 32) * (Cout / 32) * 2 * 3;
  const size_t threads = groups * 64;
  hipLaunchKernelGGL(spectra3m_split_f16_k32_kernel, dim3((unsigned)((threads + 255) / 256)), dim3(256), 0, (hipStream_t)stream, B3,
                     static_cast<uint16_t*>(Bk), groups, Cout / 32, b_scale);
  return launch_status();
}

int eqa_fft48k5_cgemm3m_f16x2_k32(const float* V, const void* Bk, float* Mo, int64_t M, int Cin, int Cout, const float* vbound,
                                  int nbound, float b_scale, void* stream) {
  if (!vbound || nbound <= 0 || !(b_scale > 0.0f)) return EQA_ERR_INVALID_ARG;
  const int st = check_contraction_args(V, Bk, Mo, M, Cin, Cout);
  if (st != EQA_OK) return st == kNothingToDo ? EQA_OK : st;
  // a K-stage is 32 channels; one frequency of Bk: a descriptor range
  if (Cout % kBlkN != 0 || Cin % 32 != 0 || (int64_t)Cin * Cout * 6 * 2 > 0x7fffffffLL) return EQA_ERR_UNSUPPORTED;
  const int n_rb = (int)((M + kBlkM - 1) / kBlkM), n_cg = Cout / kBlkN;
  constexpr int kLds = kABufs * kK32AStageBytes;
  const bool odd = (Cin / 32) % 2 != 0;
  const void* kernel = odd ? (const void*)fft_cgemm3m_f16_k32_block_kernel<true> : (const void*)fft_cgemm3m_f16_k32_block_kernel<false>;
  if (!allow_dynamic_lds(kernel, kLds)) return EQA_ERR_LAUNCH;
#define EQA_K32_LAUNCH(ODD)                                                                                                          \
  hipLaunchKernelGGL((fft_cgemm3m_f16_k32_block_kernel<ODD>), dim3(kGridBlocks), dim3(256), kLds, (hipStream_t)stream, V,            \
                     static_cast<const uint16_t*>(Bk), Mo, (int)M, (int)eqa_fft48k5_tile_pitch(M), Cin, Cout, eqa_fft48k5_frequencies(), \
                     n_rb, n_cg, kBlocksPerXcd, vbound, nbound, b_scale)
  if (odd) EQA_K32_LAUNCH(true);
  else EQA_K32_LAUNCH(false);
#undef EQA_K32_LAUNCH
  return launch_status();
}

}  // extern "C"
