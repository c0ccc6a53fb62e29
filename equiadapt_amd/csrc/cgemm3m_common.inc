// The wave-tile machinery of the channel contraction, shared by fft_cgemm3m_kernel (cgemm3m.hip: the fp32 matrix instruction) and
// fft_cgemm3m_bf16_kernel (cgemm3m_bf16.hip: the bf16 pieces): which tile a wave works on, where its operands are, where the
// finished tile goes.  The two kernels differ only in B: its element type and the bytes of one (K-stage, 32-column tile).
// The block forms of the piece contractions (cgemm3m_block.hip, cgemm3m_block_k32.hip) take the typedefs, buf_ld, the persistent
// grid and check_contraction_args from here; what they share beyond that is in cgemm3m_pieces.inc.
// Included inside each file's anonymous namespace, after eqa_common.hpp.

typedef float f32x4 __attribute__((ext_vector_type(4)));
typedef float f32x16 __attribute__((ext_vector_type(16)));
typedef float f32x2v __attribute__((ext_vector_type(2)));
typedef unsigned u32x4 __attribute__((ext_vector_type(4)));

constexpr int kTileM = 64, kTileN = 64;   // wave tile: rows (tiles of the FFT convolution) x complex output channels
constexpr int kStageK = 16;               // complex k per stage = one [Re x 16 | Im x 16] group of V
constexpr int kLdsRowFloats = 2 * kTileN;                 // one parked row: 64 complex = 128 floats = 512 bytes
constexpr int kLdsWaveFloats = kTileM * kLdsRowFloats;    // 32 KB per wave

// Persistent grid: one block of 4 waves per CU (the register budget admits one wave per SIMD); block b runs on XCD b mod 8.
constexpr int kGridBlocks = 256;
constexpr int kBlocksPerXcd = kGridBlocks / kXcd;         // 32
constexpr int kWavesPerXcd = kBlocksPerXcd * 4;

// Operand loads go through buffer descriptors: a wave-uniform descriptor (rebuilt per tile by scalar code) + a scalar byte offset
// (frequency / K-stage, advanced by scalar adds) + a 32-bit lane offset that is constant within a tile.  No vector address
// arithmetic in the MFMA stream (a VALU instruction there costs ~6 MFMA cycles), and rows beyond the buffer read as zero instead
// of needing a clamp.
struct StageAddr {
  __amdgpu_buffer_rsrc_t a, b;   // rows of V the tile reads; B[f]
  unsigned sa, sb;               // scalar byte offsets of the stage
};

template <typename T>
__device__ __forceinline__ T buf_ld(__amdgpu_buffer_rsrc_t r, unsigned voff, unsigned soff) {
  return __builtin_bit_cast(T, __builtin_amdgcn_raw_buffer_load_b128(r, voff, soff, 0));
}

// Where a parked tile goes: a buffer over the tile's rows that lie inside M (rows beyond it fall outside num_records and are
// dropped by the hardware: no branch), the lane's byte offset for row pair 0, the step to the next pair, a scalar offset.
struct ParkedDst {
  __amdgpu_buffer_rsrc_t rsrc;
  int voff, pair_bytes;
  unsigned soff;
};

__device__ __forceinline__ void store_pair(const ParkedDst& d, int p, f32x4 v) {
  __builtin_amdgcn_raw_buffer_store_b128(__builtin_bit_cast(u32x4, v), d.rsrc, d.voff + p * d.pair_bytes, d.soff, 0);
}

// row pairs [p0, p1) of the parked tile -> Mo: lanes 0..31 carry row 2p, lanes 32..63 row 2p + 1, 16 bytes each
__device__ __forceinline__ void flush_rows(const float* lds_lane, const ParkedDst& d, int p0, int p1) {
  for (int p = p0; p < p1; ++p) store_pair(d, p, *reinterpret_cast<const f32x4*>(lds_lane + p * (2 * kLdsRowFloats)));
}

// The walk of one wave over its wave-tiles (frequency, 64 rows, 64 complex columns).  The 4 waves of a block take the column tiles
// of one (f, row tile) (they share the rows of V through L1 / L2); the frequencies are dealt to the XCDs (f mod 8, block b runs
// on XCD b mod 8) so that a frequency's B panel is read from HBM once and then served by that XCD's L2 to its row tiles.
// V (F, pitch, 2 Cin) rows [Re x 16 | Im x 16] per 16 channels; B (F, S, Cout/32, kBTileBytes); Mo (F, pitch, 2 Cout) interleaved
// complex.  BT: B's element type; kBTileBytes: bytes of B per (K-stage, 32-column tile).  All sizes are < 2^32 bytes
// (host-checked).  A kernel builds it behind its `q >= total` return, in this member order: built in front of the return, or with
// the row sizes recomputed where they are used, every instantiation came out with another register allocation.
template <typename BT, unsigned kBTileBytes>
struct WaveTileWalk {
  const float* V;
  const BT* B;
  float* Mo;
  int M, pitch;
  int xcd, wpf, n_ct, S;           // blockIdx.x mod 8; wave-tiles per frequency; column tiles; K-stages
  int i, h;                        // the lane's row / column of a 32 x 32 block, and its half
  size_t rowf, mo_row;             // floats per row of V / Mo
  unsigned b_stage_bytes;          // bytes per (f, stage) of B

  __device__ __forceinline__ WaveTileWalk(const float* V_, const BT* B_, float* Mo_, int M_, int pitch_, int Cin, int Cout, int xcd_, int wpf_,
                                          int n_ct_, int S_, int i_, int h_)
      : V(V_), B(B_), Mo(Mo_), M(M_), pitch(pitch_), xcd(xcd_), wpf(wpf_), n_ct(n_ct_), S(S_), i(i_), h(h_),
        rowf((size_t)2 * Cin), mo_row((size_t)2 * Cout), b_stage_bytes((unsigned)(Cout / 32) * kBTileBytes) {}

  // wave-tile u (index in this XCD's sequence): operand descriptors + scalar offsets at stage 0, the lane's row offsets (the two
  // 32-row subtiles), its coordinates.  (Reference outputs, not a struct: the tile's values live in scalar registers across the
  // stage loop, and a struct copied per tile changed their allocation throughout the kernel.)
  __device__ __forceinline__ void locate(int u, StageAddr& at, unsigned& aoff0, unsigned& aoff1, int& f, int& row0, int& ct) const {
    const int fi = u / wpf, r = u - fi * wpf;
    f = xcd + kXcd * fi;
    const int rt = r / n_ct;
    ct = r - rt * n_ct;
    row0 = rt * kTileM;
    at.a = __builtin_amdgcn_make_buffer_rsrc(const_cast<float*>(V) + (size_t)f * pitch * rowf, 0, (unsigned)((size_t)pitch * rowf * 4), 0x00020000);
    at.sa = 0;
    aoff0 = (unsigned)((size_t)(row0 + i) * rowf + 4 * h) * 4u;        // rows >= pitch fall outside the descriptor and read as 0
    aoff1 = aoff0 + 32 * (unsigned)rowf * 4u;
    at.b = __builtin_amdgcn_make_buffer_rsrc(const_cast<BT*>(B) + (size_t)f * S * (b_stage_bytes / (unsigned)sizeof(BT)), 0, (unsigned)S * b_stage_bytes, 0x00020000);
    at.sb = (unsigned)(2 * ct) * kBTileBytes;
  }
  // a row's K-stage is 32 floats further, B's one b_stage_bytes
  __device__ __forceinline__ StageAddr at_stage(const StageAddr& t, int s) const {
    return StageAddr{t.a, t.b, t.sa + s * (32u * 4u), t.sb + s * b_stage_bytes};
  }
  // destination of the tile (f, row0, ct) once it is parked
  __device__ __forceinline__ ParkedDst parked(int f, int row0, int ct) const {
    const int rows = min(kTileM, M - row0);
    ParkedDst d;
    d.rsrc = __builtin_amdgcn_make_buffer_rsrc(Mo + ((size_t)f * pitch + row0) * mo_row, 0, (unsigned)(rows * mo_row * 4), 0x00020000);
    d.voff = (h * (int)mo_row + ct * kLdsRowFloats + i * 4) * 4;
    d.pair_bytes = 2 * (int)mo_row * 4;
    d.soff = 0;
    return d;
  }
  // before the wave's first tile is finished nothing is parked: an empty buffer drops the stores of the first tile's stage loop
  __device__ __forceinline__ ParkedDst nothing_parked(int f, int row0, int ct) const {
    ParkedDst d = parked(f, row0, ct);
    d.rsrc = __builtin_amdgcn_make_buffer_rsrc(Mo, 0, 0, 0x00020000);
    return d;
  }
};

// The tile's epilogue: Cr = T1 - T2, Ci = T3 - T1 - T2 into the wave's LDS tile [row][complex column]; accumulator register e of
// lane (h, j = i) is row (e & 3) + 8 (e >> 2) + 4 h, column j of its 32 x 32 block (the bf16 instruction's accumulator layout is
// that of the fp32 one).  (All of the previous tile's rows have left the LDS: the stage loop flushed its 32 row pairs; LDS
// operations of one wave execute in order.)
__device__ __forceinline__ void park_tile(const f32x16 (&acc)[3][2][2], float* lds_w, int i, int h) {
#pragma unroll
  for (int m = 0; m < 2; ++m)
#pragma unroll
    for (int e = 0; e < 16; ++e) {
      const int r = 32 * m + (e & 3) + 8 * (e >> 2) + 4 * h;
#pragma unroll
      for (int n = 0; n < 2; ++n) {
        const float t1 = acc[0][m][n][e], t2 = acc[1][m][n][e], t3 = acc[2][m][n][e];
        f32x2v c;
        c[0] = t1 - t2;
        c[1] = t3 - t1 - t2;
        *reinterpret_cast<f32x2v*>(lds_w + r * kLdsRowFloats + (32 * n + i) * 2) = c;
      }
    }
}

// What the three forward contractions (fp32, bf16 pieces, fp16 pieces) ask of their common arguments.  kNothingToDo: M == 0.
constexpr int kNothingToDo = 1;
inline int check_contraction_args(const void* V, const void* B, const void* Mo, int64_t M, int Cin, int Cout) {
  if (!V || !B || !Mo || M < 0 || Cin <= 0 || Cout <= 0) return EQA_ERR_INVALID_ARG;
  if (M == 0) return kNothingToDo;
  // every descriptor range and lane offset must fit 32 bits: one frequency of V / Mo (one of B: the caller, per form)
  const int64_t fm_bytes = ((M | 1) + 64) * 2 * (int64_t)std::max(Cin, Cout) * 4;
  if (!eqa_fft48k5_cgemm3m_supported(Cin, Cout) || M > 0x3fffff || fm_bytes > 0x7fffffffLL ||
      (((uintptr_t)V | (uintptr_t)B | (uintptr_t)Mo) & 15))
    return EQA_ERR_UNSUPPORTED;
  return EQA_OK;
}
