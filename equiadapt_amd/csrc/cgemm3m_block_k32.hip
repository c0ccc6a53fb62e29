// libeqa_hip.so, part 11c -- the fp16 block form of the piece contraction on v_mfma_f32_16x16x32_f16 (round 27).  Same operands,
// same two-piece split, same three products
// (h1 k1 + h1 k2 + h2 k1), same 3M arithmetic and scaling as TERMS = 3 of cgemm3m_block.hip; what differs is the instruction shape -- the chip
// holds a higher clock on 16x16x32 than on 32x32x16 at equal cycles per FLOP -- and with it the K-stage, the fragment orders and
// the store map.  The sum inside an accumulator now runs over 32 k per rounding instead of 16.
//   work: as there -- a block per 128 x 128 tile of one frequency, wave w on columns 32 w .. 32 w + 31 of all 128 rows, one wave per
//        SIMD, the XCD-aware persistent walk, the bound reduction, range-checked descriptors (cgemm3m_pieces.inc).
//   wave tile: 8 row tiles x 2 column tiles x 3 parts = 48 accumulators of 4 registers.  Lane l of an instruction holds
//        A[row l & 15][k = 8 (l >> 4) + j], B[k = 8 (l >> 4) + j][column l & 15], C[row 4 (l >> 4) + reg][column l & 15].
//   K-stage: 32 complex k = two consecutive [16 re | 16 im] groups of V.  A's pieces of a stage: 48 fragments [row tile][part]
//        [piece] of 64 lanes x 16 bytes = 48 KB; three buffers (144 KB), stage g + 2 written while g is multiplied and g + 1
//        stands published: ONE barrier per stage, Cin / 32 per tile (half of the 32x32x16 form).
//   splitter: thread (wave w, lane l) owns rows 16 w + (l >> 1 & 15) and + 64 (row tiles w and w + 4), k = 8 (l >> 5) + 4 (l & 1)
//        + 0..3 and + 16 of the stage: eight 16-byte loads, 48 values split, twenty-four 8-byte LDS writes to lane
//        (r & 15) + 16 (k >> 3), byte 2 (k & 7) of the fragment (the 64 lanes of a write cover 512 contiguous bytes: no conflict).
//        The raw values of stage g + 3 are requested group by group as those of g + 2 have been split: A two of the old stages
//        ahead of the LDS image, B (12 fragments, 48 registers, a second set) one stage ahead -- the depth in bytes of the 32x32x16 form.
//   matrix instructions of a stage: eight regions (row tile), each the row tile's 6 A fragments against the 12 B fragments:
//        18 instructions, six independent accumulators in a row (2 column tiles x 3 parts) per (A piece, B piece); a region
//        reads its own piece-1 fragments and the next row tile's piece-0 fragments behind its first six instructions.  The next
//        stage's B is asked for three fragments per region over the first four: all twelve behind the stage's barrier, from four
//        waves at once, held the first region for ~800 cycles (profiles/r27/README.md).
//   B: (F, Cin/32, Cout/32, 2 column tiles, 3 parts, 2 pieces, 64 lanes, 8 fp16); column tile t, lane column i = output channel
//        32 c + 2 i + t, so lane (i, q) holds (Cr, Ci) of channels 2 i and 2 i + 1 for rows 4 q .. 4 q + 3 of a row tile:
//        16-byte stores, 32 per wave and tile, 256 contiguous bytes per row.
#include "eqa_common.hpp"

namespace {

#include "cgemm3m_common.inc"   // the buffer descriptors, the persistent grid, the common argument checks
#include "cgemm3m_pieces.inc"   // the fp16 split, the block's walk, the fp16 scaling, the launch

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
  const BlockWalk walk{V, Bk, total, tpf, xcd, n_cg, wave, pitch, S, sp_row, rowf, b_stage_bytes, kK32BTileBytes, sp_k};

  // three positions in the block's sequence of K-stages: A's loads (3 stages ahead), B's loads (1 ahead), the matrix instructions
  TileAt ta, tb;
  unsigned a_voff, b_unused;
  int ua = q, sa = 0, ub = q, sb = 0;
  int f, row0, ct;
  walk.locate(q, ta, a_voff, f, row0, ct);
  tb = ta;
  auto next_a = [&]() { walk.advance(ua, sa, blocks_per_xcd, ta, a_voff); };
  auto next_b = [&]() { walk.advance(ub, sb, blocks_per_xcd, tb, b_unused); };

  const int ex = f16_scale_exponent(vbound, nbound, lane);
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
  // 32 ct + 2 i (column tile 0) and + 1 (column tile 1); then the coordinates of the block's next tile (in the form of
  // fft_cgemm3m_bf16_block_kernel: see there)
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
    walk.locate(u + blocks_per_xcd, unused_t, unused_o, nf, nrow0, nct);                                                                    \
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

extern "C" {

int eqa_fft48k5_spectra3m_split_f16_k32(const float* B3, void* Bk, int Cin, int Cout, float b_scale, void* stream) {
  const int st = check_f16_split_args(B3, Bk, Cin, Cout, b_scale);
  if (st != EQA_OK) return st;
  const size_t groups = (size_t)eqa_fft48k5_frequencies() * (Cin / 32) * (Cout / 32) * 2 * 3;
  const size_t threads = groups * 64;
  hipLaunchKernelGGL(spectra3m_split_f16_k32_kernel, dim3((unsigned)((threads + 255) / 256)), dim3(256), 0, (hipStream_t)stream, B3,
                     static_cast<uint16_t*>(Bk), groups, Cout / 32, b_scale);
  return launch_status();
}

int eqa_fft48k5_cgemm3m_f16x2_k32(const float* V, const void* Bk, float* Mo, int64_t M, int Cin, int Cout, const float* vbound,
                                  int nbound, float b_scale, void* stream) {
  const int st = check_f16_contraction_args(V, Bk, Mo, M, Cin, Cout, vbound, nbound, b_scale);
  if (st != EQA_OK) return st == kNothingToDo ? EQA_OK : st;
  if (Cin % 32 != 0) return EQA_ERR_UNSUPPORTED;      // a K-stage is 32 channels
  const bool odd = (Cin / 32) % 2 != 0;
  return launch_block_form(odd ? fft_cgemm3m_f16_k32_block_kernel<true> : fft_cgemm3m_f16_k32_block_kernel<false>, kABufs * kK32AStageBytes,
                           V, Bk, Mo, M, Cin, Cout, vbound, nbound, b_scale, stream);
}

}  // extern "C"
