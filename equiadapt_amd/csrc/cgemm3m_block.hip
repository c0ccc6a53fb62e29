// libeqa_hip.so, part 11b -- the BLOCK form of the piece contractions on v_mfma_f32_32x32x16 (Cout a multiple of 128): the bf16
// pieces of cgemm3m_bf16.hip with nine / six products (TERMS = 9 / 6), and the fp16 two-piece form (TERMS = 3, below).
// The same form on 16x16x32 instructions: cgemm3m_block_k32.hip.  What the two share: cgemm3m_pieces.inc.
//
// What bounds the wave form is not the matrix pipe but the vector L1: a 1-KB wave load
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
#include "eqa_common.hpp"

namespace {

#include "cgemm3m_common.inc"   // the buffer descriptors, the persistent grid, the common argument checks
#include "cgemm3m_pieces.inc"   // the piece splits, the block's walk, the fp16 scaling, the launch

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
  const BlockWalk walk{V, Bp, total, tpf, xcd, n_cg, wave, pitch, S, sp_row, rowf, b_stage_bytes, 3 * NP * kBFrag, sp_k};

  // three positions in the block's sequence of K-stages: A's loads (4 stages ahead), B's loads (1 ahead), the matrix instructions
  TileAt ta, tb;
  unsigned a_voff, b_unused;
  int ua = q, sa = 0, ub = q, sb = 0;
  int f, row0, ct;
  walk.locate(q, ta, a_voff, f, row0, ct);
  tb = ta;
  auto next_a = [&]() { walk.advance(ua, sa, blocks_per_xcd, ta, a_voff); };
  auto next_b = [&]() { walk.advance(ub, sb, blocks_per_xcd, tb, b_unused); };

  // TERMS = 3: the scaling of f16_scale_exponent
  float a_scale = 1.0f, out_scale = 1.0f;
  if constexpr (TERMS == 3) {
    const int ex = f16_scale_exponent(vbound, nbound, lane);
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

  // (a lambda in each block kernel: as a function of cgemm3m_pieces.inc it swapped the operands of adds inside the K-stages)
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
    // the block's next tile.  (Kept in this form in both block kernels: with a member of BlockWalk that hands back the coordinates
    // alone, the stage loops of all five came out re-allocated and the even 16x16x32 kernel with 400 registers for 396.)
    int nf, nrow0, nct;
    TileAt unused_t;
    unsigned unused_o;
    walk.locate(u + blocks_per_xcd, unused_t, unused_o, nf, nrow0, nct);
    f = nf; row0 = nrow0; ct = nct;
    clk.tile_epilogue_end();
  }
  clk.publish();
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

template <int TERMS>
int launch_block(const float* V, const void* B, float* Mo, int64_t M, int Cin, int Cout, const float* vbound, int nbound, float b_scale,
                 void* stream) {
  return launch_block_form(fft_cgemm3m_bf16_block_kernel<TERMS>, kABufs * a_stage_bytes(TERMS), V, B, Mo, M, Cin, Cout, vbound, nbound,
                           b_scale, stream);
}

}  // namespace

namespace eqa {
int launch_cgemm3m_bf16_block(int terms, const float* V, const void* Bp, float* Mo, int64_t M, int Cin, int Cout, void* stream) {
  return terms == 9 ? launch_block<9>(V, Bp, Mo, M, Cin, Cout, nullptr, 0, 1.0f, stream)
                    : launch_block<6>(V, Bp, Mo, M, Cin, Cout, nullptr, 0, 1.0f, stream);
}
#ifdef EQA_BLK_CLOCK
const void* g_blk_clock_symbol = nullptr;
#endif
}  // namespace eqa

extern "C" {

#ifdef EQA_BLK_CLOCK
int eqa_debug_blk_clock(long long* out) {
  return eqa::g_blk_clock_symbol ? (int)hipMemcpyFromSymbol(out, eqa::g_blk_clock_symbol, 80) : EQA_ERR_INVALID_ARG;
}
#endif

int64_t eqa_fft48k5_spectra3m_f16_bytes(int Cin, int Cout) {
  if (!eqa_fft48k5_cgemm3m_supported(Cin, Cout) || Cout % kBlkN != 0) return 0;
  return (int64_t)eqa_fft48k5_frequencies() * Cin * Cout * 3 * 2 * 2;
}

int eqa_fft48k5_spectra3m_split_f16(const float* B3, void* Bh, int Cin, int Cout, float b_scale, void* stream) {
  const int st = check_f16_split_args(B3, Bh, Cin, Cout, b_scale);
  if (st != EQA_OK) return st;
  const size_t groups = (size_t)eqa_fft48k5_frequencies() * (Cin / kStageK) * (Cout / 32) * 3;
  const size_t threads = groups * 64;
  hipLaunchKernelGGL(spectra3m_split_f16_kernel, dim3((unsigned)((threads + 255) / 256)), dim3(256), 0, (hipStream_t)stream, B3,
                     static_cast<uint16_t*>(Bh), groups, b_scale);
  return launch_status();
}

int eqa_fft48k5_cgemm3m_f16x2(const float* V, const void* Bh, float* Mo, int64_t M, int Cin, int Cout, const float* vbound, int nbound,
                              float b_scale, void* stream) {
  const int st = check_f16_contraction_args(V, Bh, Mo, M, Cin, Cout, vbound, nbound, b_scale);
  if (st != EQA_OK) return st == kNothingToDo ? EQA_OK : st;
  if ((Cin / kStageK) % 2 != 0) return EQA_ERR_UNSUPPORTED;      // the K loop runs stage pairs
  return launch_block<3>(V, Bh, Mo, M, Cin, Cout, vbound, nbound, b_scale, stream);
}

}  // extern "C"
