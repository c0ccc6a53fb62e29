// What the piece forms of the channel contraction share: the exact splits of an fp32 operand (three bf16 pieces, two fp16 pieces),
// the bf16 matrix instruction, and the parts of the two BLOCK forms (cgemm3m_block.hip: 32x32x16 instructions; cgemm3m_block_k32.hip:
// 16x16x32) that are the same in both -- the walk of a block over its tiles, the fp16 scaling, the pinning of a region, the launch
// and the argument checks of the fp16 entries.  The wave form (cgemm3m_bf16.hip) uses the splits and the instruction.
// Included inside each unit's anonymous namespace, behind cgemm3m_common.inc.

typedef __bf16 bf16x8 __attribute__((ext_vector_type(8)));
typedef _Float16 f16x8 __attribute__((ext_vector_type(8)));
typedef _Float16 f16x2v __attribute__((ext_vector_type(2)));
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
// two fp16 pieces of four (already scaled) values: v_cvt_pk_f16_f32 (round to nearest even), the remainder, again
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

__device__ __forceinline__ f32x16 mma(const u32x4 a, const u32x4 b, const f32x16 c) {
  return __builtin_amdgcn_mfma_f32_32x32x16_bf16(__builtin_bit_cast(bf16x8, a), __builtin_bit_cast(bf16x8, b), c, 0, 0, 0);
}

// ---------------------------------------------------------------------------------------------------------------------------
// The block forms: a block works on 128 rows x 128 columns of one frequency, wave w on columns 32 w .. 32 w + 31 of all 128 rows,
// A's K-stage split once per block into a ring of kABufs LDS buffers, B a stage ahead in registers.
constexpr int kBlkM = 128, kBlkN = 128;
constexpr int kFragBytes = 64 * 16;
constexpr unsigned kBFrag = 64 * 16;    // bytes of one (part, piece) fragment of a 32-column tile
constexpr int kABufs = 3;

// The one debug build that is kept (tools/kbench_gemm_clock.py): -DEQA_BLK_CLOCK=1 stamps the first / last shader cycle and the
// constant 100 MHz counter of block 100's first thread and the cycles of its tile epilogues; =2 adds an s_memtime at every region
// boundary of a K-stage.  The product build's BlkClock is empty: the block kernels call it unconditionally.  A kernel reaches only
// its own unit's device globals, so each unit has its g_blk_clock; launch_block_form names the one the last launch wrote to
// eqa_debug_blk_clock (cgemm3m_block.hip).
#ifdef EQA_BLK_CLOCK
[[maybe_unused]] __device__ long long g_blk_clock[16];
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
#else
struct BlkClock {
  __device__ __forceinline__ void tick(int) {}
  __device__ __forceinline__ void stage_end() {}
  __device__ __forceinline__ void tile_epilogue_begin() {}
  __device__ __forceinline__ void tile_epilogue_end() {}
  __device__ __forceinline__ void publish() {}
};
#endif

struct TileAt {                   // uniform: where a block tile's operands are
  __amdgpu_buffer_rsrc_t a, b;
  unsigned sb;
};

// The walk of one block over its block tiles, in the order of its XCD's sequence (the frequencies are dealt to the XCDs as in
// WaveTileWalk).  V (F, pitch, 2 Cin); B (F, S, Cout/32, b_tile_bytes) in the form's fragment order.  The forms differ in S (K-stages
// of 16 / 32), in the splitter's k offset sp_k and in B's bytes per (stage, 32 columns): the kernel states those and builds the
// walk behind its `q >= total` return.
struct BlockWalk {
  const float* V;
  const uint16_t* B;
  int total, tpf, xcd, n_cg, wave;   // block tiles of this XCD / per frequency; blockIdx.x mod 8; column groups; the wave
  int pitch, S, sp_row;              // rows of a frequency of V; K-stages; the splitter thread's row of the block tile
  size_t rowf;                       // floats per row of V
  unsigned b_stage_bytes, b_tile_bytes, sp_k;

  // block tile u: operand descriptors, the splitter thread's byte offset into A at stage 0, the tile's coordinates (reference
  // outputs, not a struct: see WaveTileWalk::locate)
  __device__ __forceinline__ void locate(int u, TileAt& at, unsigned& aoff, int& f, int& row0, int& ct) const {
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
    at.b = __builtin_amdgcn_make_buffer_rsrc(const_cast<uint16_t*>(B) + (size_t)f * S * (b_stage_bytes / 2), 0, live ? (unsigned)S * b_stage_bytes : 0u, 0x00020000);
    at.sb = (unsigned)ct * b_tile_bytes;
  }
  // a position (tile u, stage s) in the block's sequence of K-stages, one stage on; behind a tile's last stage: the next tile's operands
  __device__ __forceinline__ void advance(int& u, int& s, int stride, TileAt& at, unsigned& aoff) const {
    if (++s == S) {
      s = 0;
      u += stride;
      int f, row0, ct;
      locate(u, at, aoff, f, row0, ct);
    }
  }
};

// The fp16 forms' scaling: A is scaled by the power of two that takes the caller's bound of |V| (vbound[0 .. nbound): the largest
// counts) to 2^14 (re + im then stays below 2^15.5 < 65504); the result is scaled back with B's factor in the epilogue.  Powers of
// two: exact.  Returns the exponent, the same in every lane and wave.
__device__ __forceinline__ int f16_scale_exponent(const float* __restrict__ vbound, int nbound, int lane) {
  float mx = 0.0f;
  for (int t = lane; t < nbound; t += 64) mx = fmaxf(mx, vbound[t]);
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) mx = fmaxf(mx, __shfl_xor(mx, o));
  int ex = 0;
  if (mx > 0.0f && mx < 3.0e38f) (void)frexpf(mx, &ex);      // mx <= 2^ex
  ex = min(max(14 - ex, -100), 100);
  return __builtin_amdgcn_readfirstlane(ex);
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

// The block forms' launch: 128 x 128 tiles, one block per CU, kABufs K-stages of A's pieces in dynamic LDS.
using BlockKernel = void (*)(const float*, const uint16_t*, float*, int, int, int, int, int, int, int, int, const float*, int, float);
inline int launch_block_form(BlockKernel kernel, int lds_bytes, const float* V, const void* B, float* Mo, int64_t M, int Cin, int Cout,
                             const float* vbound, int nbound, float b_scale, void* stream) {
  const int n_rb = (int)((M + kBlkM - 1) / kBlkM), n_cg = Cout / kBlkN;
  if (!allow_dynamic_lds((const void*)kernel, lds_bytes)) return EQA_ERR_LAUNCH;
#ifdef EQA_BLK_CLOCK
  eqa::g_blk_clock_symbol = HIP_SYMBOL(g_blk_clock);
#endif
  hipLaunchKernelGGL(kernel, dim3(kGridBlocks), dim3(256), lds_bytes, (hipStream_t)stream, V, static_cast<const uint16_t*>(B), Mo, (int)M,
                     (int)eqa_fft48k5_tile_pitch(M), Cin, Cout, eqa_fft48k5_frequencies(), n_rb, n_cg, kBlocksPerXcd, vbound, nbound, b_scale);
  return launch_status();
}

// What the entries of the two fp16 forms ask of their arguments (EQA_OK, kNothingToDo or an error); the form's own condition on Cin
// (whole stage pairs of 16 / whole stages of 32) stays with the entry.
inline int check_f16_contraction_args(const void* V, const void* B, const void* Mo, int64_t M, int Cin, int Cout, const float* vbound,
                                      int nbound, float b_scale) {
  if (!vbound || nbound <= 0 || !(b_scale > 0.0f)) return EQA_ERR_INVALID_ARG;
  const int st = check_contraction_args(V, B, Mo, M, Cin, Cout);
  if (st != EQA_OK) return st;
  // the block form only; one frequency of B: a descriptor range
  if (Cout % kBlkN != 0 || (int64_t)Cin * Cout * 6 * 2 > 0x7fffffffLL) return EQA_ERR_UNSUPPORTED;
  return EQA_OK;
}
inline int check_f16_split_args(const float* B3, const void* Bh, int Cin, int Cout, float b_scale) {
  if (!B3 || !Bh || !(b_scale > 0.0f)) return EQA_ERR_INVALID_ARG;
  if (eqa_fft48k5_spectra3m_f16_bytes(Cin, Cout) == 0 || (((uintptr_t)B3 | (uintptr_t)Bh) & 15)) return EQA_ERR_UNSUPPORTED;
  int ex = 0;
  if (frexpf(b_scale, &ex) != 0.5f) return EQA_ERR_INVALID_ARG;            // a power of two: the scaling must be exact
  return EQA_OK;
}
