// The first layer of ESCNNSteerableNetwork: the scalar -> Fourier-field convolution (reference network: escnn_networks.py:178-186,
// the first R2Conv), 1 or 3 input channels -> 9 F channels (F fields of a_0, Re / Im c_1..c_4), k x k, stride 1, no padding, no bias.
// The kernels see a dense real bank (SteerableConv.expanded_weights()); the steerable structure stays in Python.
// C ABI: include/eqa_hip.h (eqa_steer_lift_*).
//
//   y[n,oy,ox,co] = sum_{ky,kx,ci} x[n,oy+ky,ox+kx,ci] * w[co,ci,ky,kx]                     channels-last fp32
//
// Implicit GEMM on v_mfma_f32_16x16x4_f32, the register-resident-weights form of lift_conv_wide.hip at 16-channel granularity
// (9 F is rarely a multiple of 64 or of 16: 144 at the reference's configuration, 36 in the tests).
//  * Channels are cut into 16-channel blocks, C9 = 9 F padded up to nblk = ceil(C9 / 16) blocks; the blocks are dealt to
//    ngroups = ceil(nblk / 3) groups of bpw = ceil(nblk / ngroups) <= 3 blocks (144 channels: 3 groups of 3).  A wave owns one
//    group for the whole kernel and keeps its bpw x STEPS weight registers; wave gw of the 1024 is group gw % ngroups, stream
//    gw / ngroups of nstreams = 1024 / ngroups (the 1024 % ngroups waves left over leave at once).
//  * A stream walks tiles of 32 consecutive pixels of one output row, tile t = stream, stream + nstreams, ...  Tiles never
//    overlap (a pixel counts once in the statistics); pixels past the row's end are computed and not stored.
//  * Taps.  A filter row is RW = K Cin floats, padded to RWP = 4 ceil(RW / 4); step s = ky (RWP / 4) + cs of a matrix
//    instruction takes the four taps (ky, column 4 cs + q), q = lane >> 4.  The lane's B operand is then
//    buf[ky SEG + 4 cs + pix Cin + q]: one base register and a compile-time offset, no address arithmetic per step.  Cost: RWP / RW
//    of the matrix work (24 / 21 at 7 x 7 x 3, 28 / 27 at 9 x 9 x 3; 8 / 5 at 5 x 5 x 1).  The padded taps carry weight 0 and read
//    real input (the staged row segment is RWP - RW floats longer, clamped to the row's last float).
//  * The K input-row segments of a tile go HBM -> registers -> the wave's private LDS double buffer one tile ahead; no barrier
//    anywhere.  Two pixel halves x bpw blocks = 2 bpw independent accumulator chains (the instruction's dependent latency is 40
//    cycles against 32 of issue); the B reads run one chunk of steps ahead of the instructions that use them.
//  * Epilogue: accumulator e of lane (pix = lane & 15, q = lane >> 4) is channel 16 blk + 4 q + e of pixel pix: one 16-byte store
//    where C9 % 4 == 0, scalar stores otherwise; channels >= C9 are never stored.
//  * Statistics (part != NULL): every lane adds its stored values and their squares in fp64 (converted first: the squares are
//    exact) over its whole walk; at the end the 16 pixel lanes of a channel are added in a fixed butterfly and row `stream` of
//    part:(nstreams, C9, 2) is written -- every row, zeros from a stream without tiles.  No atomics.  The caller folds
//    (sum, sum of squares) per channel into the field norm's six sums per field (ops.steer_lift).
//
// Packed weights, wpk:(ngroups, bpw, STEPS, 64) fp32:
//   wpk[g][b][s][lane] = w[co][ci][ky][kx],  co = 16 (g bpw + b) + (lane & 15),  ky = s / (RWP/4),  c = 4 (s % (RWP/4)) + (lane >> 4),
//   kx = c / Cin, ci = c % Cin;  0 where c >= RW or co >= C9.
//
// Filter gradient, dbank[co][ci][ky][kx] = sum over (n, oy, ox) of dy[n,oy,ox,co] x[n,oy+ky,ox+kx,ci]: the contraction runs over
// the pixels, four per matrix instruction.  A = dy (row = channel, read from HBM one tile ahead: the big operand is read once),
// B = the staged input rows (column = tap r = (ky K + kx) Cin + ci, unpadded: ceil(R / 16) tap blocks).  Same waves, groups,
// streams and tiles as the forward; a wave keeps bpw x ceil(R / 16) accumulators over its whole walk and leaves them in the
// workspace; steer_lift_wgrad_reduce_kernel adds the streams of a channel in stream order in fp64 (deterministic).
#include "eqa_common.hpp"

namespace {

typedef float f32x4 __attribute__((ext_vector_type(4)));

constexpr int kLiftWaves = 1024;          // persistent waves: 256 CUs x 4 SIMDs
constexpr int kLiftMaxBpw = 3;            // 16-channel blocks per wave at most
constexpr int kLiftFieldDim = 9;
constexpr int kLiftMaxFields = 64;        // == eqa_field_norm_max_fields(): the norm behind the layer takes no more

template <int KS, int CIN>
struct LiftShape {
  static constexpr int R = KS * KS * CIN, RW = KS * CIN, RWP = (RW + 3) / 4 * 4, CS = RWP / 4, STEPS = KS * CS;
  static constexpr int SEG = (31 + KS) * CIN + (RWP - RW);    // floats of a tile's staged row segment
  static constexpr int NLD = (KS * SEG + 63) / 64;            // staging loads per lane and tile
  static constexpr int BUF = NLD * 64;                        // floats of one LDS buffer
  static constexpr int TB = (R + 15) / 16;                    // 16-tap blocks of the filter gradient
};

struct LiftPlan {
  int C9, nblk, ngroups, bpw, nstreams;
};

inline bool lift_supported(int Cin, int K, int fields) {
  return (Cin == 1 || Cin == 3) && (K == 5 || K == 7 || K == 9) && fields >= 1 && fields <= kLiftMaxFields;
}

inline LiftPlan lift_plan(int fields) {
  LiftPlan p;
  p.C9 = kLiftFieldDim * fields;
  p.nblk = (p.C9 + 15) / 16;
  p.ngroups = (p.nblk + kLiftMaxBpw - 1) / kLiftMaxBpw;
  p.bpw = (p.nblk + p.ngroups - 1) / p.ngroups;
  p.nstreams = kLiftWaves / p.ngroups;
  return p;
}

// a tile's position (tile column, output row, image), advanced by the stream's stride without divisions; all wave-uniform
struct LiftPos {
  unsigned tx, oy, n;
};
struct LiftWalk {
  unsigned tpr, OH;
  LiftPos d;
  __device__ __forceinline__ LiftWalk(unsigned tpr_, unsigned OH_, unsigned stride) : tpr(tpr_), OH(OH_) { d = at(stride); }
  __device__ __forceinline__ LiftPos at(unsigned t) const {
    const unsigned r = t / tpr;
    return LiftPos{t % tpr, r % OH, r / OH};
  }
  __device__ __forceinline__ LiftPos next(const LiftPos& p) const {
    LiftPos q;
    q.tx = p.tx + d.tx;
    unsigned c = q.tx >= tpr ? 1u : 0u;
    q.tx -= c ? tpr : 0u;
    q.oy = p.oy + d.oy + c;                      // <= 2 OH - 1
    c = q.oy >= OH ? 1u : 0u;
    q.oy -= c ? OH : 0u;
    q.n = p.n + d.n + c;
    return q;
  }
};

// The K row segments of the tile at p: element id = lane + 64 j of the KS x SEG block, clamped to the last float of its input row
template <int KS, int CIN>
struct LiftStage {
  using S = LiftShape<KS, CIN>;
  int off[S::NLD], col[S::NLD];                  // row * W * CIN, column
  float v[S::NLD];
  __device__ __forceinline__ LiftStage(int lane, int W) {
#pragma unroll
    for (int j = 0; j < S::NLD; ++j) {
      const int id = min(lane + 64 * j, KS * S::SEG - 1);
      const int row = id / S::SEG;
      col[j] = id - row * S::SEG;
      off[j] = row * W * CIN;
    }
  }
  __device__ __forceinline__ void request(const float* __restrict__ x, const LiftPos& p, int H, int W) {
    const int ox0 = (int)p.tx * 32;
    const float* base = x + ((size_t)p.n * H + p.oy) * (size_t)W * CIN + (size_t)ox0 * CIN;
    const int lim = (W - ox0) * CIN - 1;
#pragma unroll
    for (int j = 0; j < S::NLD; ++j) v[j] = base[off[j] + min(col[j], lim)];
  }
  __device__ __forceinline__ void deposit(float* buf, int lane) const {
#pragma unroll
    for (int j = 0; j < S::NLD; ++j) buf[lane + 64 * j] = v[j];
  }
};

__device__ __forceinline__ double lift_pixel_sum(double v) {      // over the 16 lanes lane & 15 of one lane >> 4, fixed order
  v += __shfl_xor(v, 1);
  v += __shfl_xor(v, 2);
  v += __shfl_xor(v, 4);
  v += __shfl_xor(v, 8);
  return v;
}

template <int KS, int CIN, int BPW>
__global__ __launch_bounds__(256, 1) void steer_lift_fwd_kernel(const float* __restrict__ x, const float* __restrict__ wpk,
                                                                float* __restrict__ y, double* __restrict__ part, int nimg, int H,
                                                                int W, int C9, int ngroups, int tiles_per_row) {
  using S = LiftShape<KS, CIN>;
  __shared__ float lds_all[4 * 2 * S::BUF];
  const int lane = threadIdx.x & 63;
  const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const int gw = blockIdx.x * 4 + wave;
  const int nstreams = kLiftWaves / ngroups;
  if (gw >= nstreams * ngroups) return;                       // (no barrier in this kernel: a wave may leave alone)
  const int group = gw % ngroups, stream = gw / ngroups;
  const int OH = H - KS + 1, OW = W - KS + 1;
  const long long ntiles = (long long)nimg * OH * tiles_per_row;
  float* lds = lds_all + wave * 2 * S::BUF;
  const int pix = lane & 15, q = lane >> 4;

  float wreg[BPW][S::STEPS];
  {
    const float* wp = wpk + (size_t)group * BPW * S::STEPS * 64 + lane;
#pragma unroll
    for (int b = 0; b < BPW; ++b)
#pragma unroll
      for (int s = 0; s < S::STEPS; ++s) wreg[b][s] = wp[(b * S::STEPS + s) * 64];
  }
  double ssum[BPW][4], ssq[BPW][4];
#pragma unroll
  for (int b = 0; b < BPW; ++b)
#pragma unroll
    for (int e = 0; e < 4; ++e) ssum[b][e] = ssq[b][e] = 0.0;

  const LiftWalk walk((unsigned)tiles_per_row, (unsigned)OH, (unsigned)nstreams);
  LiftStage<KS, CIN> stage(lane, W);
  const bool vec = (C9 & 3) == 0;
  const int ch0 = 16 * group * BPW + 4 * q;                   // the lane's first channel of block 0

  long long t = stream;
  if (t < ntiles) {
    LiftPos pos = walk.at((unsigned)stream);
    stage.request(x, pos, H, W);
    stage.deposit(lds, lane);
    int cur = 0;
    for (; t < ntiles; t += nstreams) {
      const LiftPos pn = t + nstreams < ntiles ? walk.next(pos) : pos;
      stage.request(x, pn, H, W);                             // next tile's rows: in flight during this tile's matrix instructions
      const float* bp = lds + cur * S::BUF + pix * CIN + q;
      f32x4 acc[BPW][2];
#pragma unroll
      for (int b = 0; b < BPW; ++b)
#pragma unroll
        for (int h = 0; h < 2; ++h) acc[b][h] = f32x4{0.0f, 0.0f, 0.0f, 0.0f};
      // B operands: one ds_read_b32 per step and pixel half, read one chunk of steps ahead of their matrix instructions
      constexpr int kChunk = 4, kNch = (S::STEPS + kChunk - 1) / kChunk;
      float bq[2][kChunk][2];
#pragma unroll
      for (int j = 0; j < kChunk; ++j)
        if (j < S::STEPS) {
          bq[0][j][0] = bp[(j / S::CS) * S::SEG + 4 * (j % S::CS)];
          bq[0][j][1] = bp[(j / S::CS) * S::SEG + 4 * (j % S::CS) + 16 * CIN];
        }
#pragma unroll
      for (int c = 0; c < kNch; ++c) {
        __builtin_amdgcn_sched_barrier(0);
#pragma unroll
        for (int j = 0; j < kChunk; ++j) {
          const int sn = (c + 1) * kChunk + j;
          if (sn < S::STEPS) {
            bq[(c + 1) & 1][j][0] = bp[(sn / S::CS) * S::SEG + 4 * (sn % S::CS)];
            bq[(c + 1) & 1][j][1] = bp[(sn / S::CS) * S::SEG + 4 * (sn % S::CS) + 16 * CIN];
          }
        }
#pragma unroll
        for (int j = 0; j < kChunk; ++j) {
          const int sc = c * kChunk + j;
          if (sc < S::STEPS) {
#pragma unroll
            for (int b = 0; b < BPW; ++b) {
              acc[b][0] = __builtin_amdgcn_mfma_f32_16x16x4f32(wreg[b][sc], bq[c & 1][j][0], acc[b][0], 0, 0, 0);
              acc[b][1] = __builtin_amdgcn_mfma_f32_16x16x4f32(wreg[b][sc], bq[c & 1][j][1], acc[b][1], 0, 0, 0);
            }
          }
        }
#pragma unroll
        for (int j = 0; j < 2 * kChunk; ++j) {
          __builtin_amdgcn_sched_group_barrier(0x008, BPW, 0);
          __builtin_amdgcn_sched_group_barrier(0x100, 1, 0);
        }
      }
      __builtin_amdgcn_sched_barrier(0);
      stage.deposit(lds + (cur ^ 1) * S::BUF, lane);
      cur ^= 1;
      // epilogue: the lane's 4 consecutive channels per block of pixel ox0 + 16 h + pix
#pragma unroll
      for (int h = 0; h < 2; ++h) {
        const int ox = (int)pos.tx * 32 + 16 * h + pix;
        if (ox < OW) {
          float* o = y + (((size_t)pos.n * OH + pos.oy) * OW + ox) * (size_t)C9 + ch0;
#pragma unroll
          for (int b = 0; b < BPW; ++b) {
            const int ch = ch0 + 16 * b;
            if (vec) {
              if (ch < C9) *reinterpret_cast<f32x4*>(o + 16 * b) = acc[b][h];
            } else {
#pragma unroll
              for (int e = 0; e < 4; ++e)
                if (ch + e < C9) o[16 * b + e] = acc[b][h][e];
            }
            if (part) {
#pragma unroll
              for (int e = 0; e < 4; ++e) {
                const double v = (double)acc[b][h][e];
                ssum[b][e] += v;
                ssq[b][e] += v * v;
              }
            }
          }
        }
      }
      pos = pn;
    }
  }
  if (part) {
    double* row = part + (size_t)stream * C9 * 2;
#pragma unroll
    for (int b = 0; b < BPW; ++b)
#pragma unroll
      for (int e = 0; e < 4; ++e) {
        const double s = lift_pixel_sum(ssum[b][e]), s2 = lift_pixel_sum(ssq[b][e]);
        const int ch = ch0 + 16 * b + e;
        if (pix == 0 && ch < C9) {
          row[2 * ch] = s;
          row[2 * ch + 1] = s2;
        }
      }
  }
}

template <int KS, int CIN, int BPW>
__global__ __launch_bounds__(256, 1) void steer_lift_wgrad_kernel(const float* __restrict__ x, const float* __restrict__ dy,
                                                                  float* __restrict__ part, int nimg, int H, int W, int C9, int ngroups,
                                                                  int tiles_per_row, int nused) {
  using S = LiftShape<KS, CIN>;
  __shared__ float lds_all[4 * 2 * S::BUF];
  const int lane = threadIdx.x & 63;
  const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const int gw = blockIdx.x * 4 + wave;
  const int nstreams = kLiftWaves / ngroups;
  if (gw >= nstreams * ngroups) return;
  const int group = gw % ngroups, stream = gw / ngroups;
  if (stream >= nused) return;                                // nused = min(nstreams, tiles): every remaining stream has a tile
  const int OH = H - KS + 1, OW = W - KS + 1;
  const long long ntiles = (long long)nimg * OH * tiles_per_row;
  float* lds = lds_all + wave * 2 * S::BUF;
  const int li = lane & 15, q = lane >> 4;

  // B operand: tap 16 tb + li of pixel q (+ 4 per step); taps past R read element 0 (their columns are never read back)
  int boff[S::TB];
#pragma unroll
  for (int tb = 0; tb < S::TB; ++tb) {
    const int tap = 16 * tb + li;
    boff[tb] = (tap < S::R ? (tap / S::RW) * S::SEG + tap % S::RW : 0) + q * CIN;
  }
  // A operand: channel 16 (group BPW + b) + li of pixel q (+ 4 per step), read through a buffer descriptor that spans the tile's
  // pixels inside the row: its range check returns zero for the pixels past the row's end, and a lane whose channel is past C9
  // asks far past the descriptor's end.  (Plain loads behind a select became one branch and one full wait per load.)
  unsigned dyoff[BPW];
#pragma unroll
  for (int b = 0; b < BPW; ++b) {
    const int ch = 16 * (group * BPW + b) + li;
    dyoff[b] = ch < C9 ? (unsigned)(q * C9 + ch) * 4u : 0x80000000u;
  }
  const LiftWalk walk((unsigned)tiles_per_row, (unsigned)OH, (unsigned)nstreams);
  LiftStage<KS, CIN> stage(lane, W);
  float dyr[8][BPW];
  auto request_dy = [&](const LiftPos& p) {
    const int ox0 = (int)p.tx * 32;
    const float* dbase = dy + (((size_t)p.n * OH + p.oy) * OW + ox0) * (size_t)C9;
    const unsigned bytes = (unsigned)min(32, OW - ox0) * (unsigned)C9 * 4u;
    const __amdgpu_buffer_rsrc_t rsrc = __builtin_amdgcn_make_buffer_rsrc(const_cast<float*>(dbase), 0, bytes, 0x00020000);
#pragma unroll
    for (int s = 0; s < 8; ++s)
#pragma unroll
      for (int b = 0; b < BPW; ++b)
        dyr[s][b] = __builtin_bit_cast(float, __builtin_amdgcn_raw_buffer_load_b32(rsrc, dyoff[b] + (unsigned)(16 * s * C9), 0, 0));
  };

  f32x4 acc[BPW][S::TB];
#pragma unroll
  for (int b = 0; b < BPW; ++b)
#pragma unroll
    for (int tb = 0; tb < S::TB; ++tb) acc[b][tb] = f32x4{0.0f, 0.0f, 0.0f, 0.0f};

  LiftPos pos = walk.at((unsigned)stream);
  stage.request(x, pos, H, W);
  stage.deposit(lds, lane);
  request_dy(pos);
  int cur = 0;
  for (long long t = stream; t < ntiles; t += nstreams) {
    float a[8][BPW];
#pragma unroll
    for (int s = 0; s < 8; ++s)
#pragma unroll
      for (int b = 0; b < BPW; ++b) a[s][b] = dyr[s][b];
    const LiftPos pn = t + nstreams < ntiles ? walk.next(pos) : pos;
    // next tile: in flight during this tile's matrix instructions.  (Requested and deposited inside one trip, as in the forward:
    // with the deposit at the top of the next trip the compiler folds the loads into it and waits for each where it is issued.)
    stage.request(x, pn, H, W);
    request_dy(pn);
    __builtin_amdgcn_sched_barrier(0);
    const float* buf = lds + cur * S::BUF;
#pragma unroll
    for (int s = 0; s < 8; ++s) {
      float bx[S::TB];
#pragma unroll
      for (int tb = 0; tb < S::TB; ++tb) bx[tb] = buf[boff[tb] + 4 * s * CIN];
#pragma unroll
      for (int tb = 0; tb < S::TB; ++tb)
#pragma unroll
        for (int b = 0; b < BPW; ++b) acc[b][tb] = __builtin_amdgcn_mfma_f32_16x16x4f32(a[s][b], bx[tb], acc[b][tb], 0, 0, 0);
    }
    __builtin_amdgcn_sched_barrier(0);
    stage.deposit(lds + (cur ^ 1) * S::BUF, lane);
    cur ^= 1;
    pos = pn;
  }
  // the wave's partial: part[gw][channel 0 .. 16 BPW)[tap 0 .. 16 TB); accumulator e of lane (li, q): row 4 q + e, column li
  float* pw = part + (size_t)gw * (16 * BPW) * (16 * S::TB);
#pragma unroll
  for (int b = 0; b < BPW; ++b)
#pragma unroll
    for (int tb = 0; tb < S::TB; ++tb)
#pragma unroll
      for (int e = 0; e < 4; ++e) pw[(size_t)(16 * b + 4 * q + e) * (16 * S::TB) + 16 * tb + li] = acc[b][tb][e];
}

// dbank[co][ci][ky][kx] = sum over the streams of co's group, in stream order; one thread per (co, tap)
__global__ __launch_bounds__(256) void steer_lift_wgrad_reduce_kernel(const float* __restrict__ part, float* __restrict__ dbank, int C9,
                                                                      int Cin, int K, int ngroups, int bpw, int nused) {
  const int R = K * K * Cin, RP = (R + 15) / 16 * 16;
  const int id = blockIdx.x * blockDim.x + threadIdx.x;
  if (id >= C9 * R) return;
  const int co = id / R, r = id - co * R;
  const int group = co / (16 * bpw), cl = co - group * 16 * bpw;
  double sum = 0.0;
  for (int s = 0; s < nused; ++s) sum += (double)part[((size_t)(s * ngroups + group) * (16 * bpw) + cl) * RP + r];
  const int ci = r % Cin, kx = (r / Cin) % K, ky = r / (Cin * K);
  dbank[((size_t)(co * Cin + ci) * K + ky) * K + kx] = (float)sum;
}

template <int KS, int CIN>
int lift_fwd_launch(const float* x, const float* wpk, float* y, double* part, int nimg, int H, int W, const LiftPlan& p, hipStream_t st) {
  const int tpr = (W - KS + 1 + 31) / 32;
  const dim3 grid(kLiftWaves / 4), block(256);
#define EQA_LIFT_BPW(N) \
  if (p.bpw == N) hipLaunchKernelGGL((steer_lift_fwd_kernel<KS, CIN, N>), grid, block, 0, st, x, wpk, y, part, nimg, H, W, p.C9, p.ngroups, tpr)
  EQA_LIFT_BPW(1); EQA_LIFT_BPW(2); EQA_LIFT_BPW(3);
#undef EQA_LIFT_BPW
  return launch_status();
}

template <int KS, int CIN>
int lift_wgrad_launch(const float* x, const float* dy, float* part, float* dbank, int nimg, int H, int W, const LiftPlan& p, hipStream_t st) {
  const int tpr = (W - KS + 1 + 31) / 32;
  const long long ntiles = (long long)nimg * (H - KS + 1) * tpr;
  const int nused = (int)std::min<long long>(p.nstreams, ntiles);
  const dim3 grid(kLiftWaves / 4), block(256);
#define EQA_LIFT_BPW(N) \
  if (p.bpw == N) hipLaunchKernelGGL((steer_lift_wgrad_kernel<KS, CIN, N>), grid, block, 0, st, x, dy, part, nimg, H, W, p.C9, p.ngroups, tpr, nused)
  EQA_LIFT_BPW(1); EQA_LIFT_BPW(2); EQA_LIFT_BPW(3);
#undef EQA_LIFT_BPW
  const int n = p.C9 * KS * KS * CIN;
  hipLaunchKernelGGL(steer_lift_wgrad_reduce_kernel, dim3((n + 255) / 256), dim3(256), 0, st, part, dbank, p.C9, CIN, KS, p.ngroups, p.bpw,
                     nused);
  return launch_status();
}

// the checks the two entries share, in the order the header documents (the pointers come after them, and after nimg == 0)
int lift_check(int nimg, int H, int W, int Cin, int K, int fields) {
  if (!lift_supported(Cin, K, fields)) return EQA_ERR_UNSUPPORTED;
  if (nimg < 0 || H <= 0 || W <= 0) return EQA_ERR_INVALID_ARG;
  if (H < K || W < K) return EQA_ERR_UNSUPPORTED;
  if ((long long)nimg * (H - K + 1) * ((W - K + 32) / 32) > 0x7fffffffLL) return EQA_ERR_UNSUPPORTED;   // tiles are counted in 32 bits
  if ((long long)nimg * H * W * Cin > 0x7fffffffLL) return EQA_ERR_UNSUPPORTED;                        // staging offsets are ints
  return EQA_OK;
}

}  // namespace

extern "C" {

int eqa_steer_lift_supported(int Cin, int K, int fields) { return lift_supported(Cin, K, fields) ? 1 : 0; }

int64_t eqa_steer_lift_packed_floats(int Cin, int K, int fields) {
  if (!lift_supported(Cin, K, fields)) return 0;
  const LiftPlan p = lift_plan(fields);
  const int steps = K * ((K * Cin + 3) / 4);
  return (int64_t)p.ngroups * p.bpw * steps * 64;
}

long long eqa_steer_lift_stat_rows(int fields) {
  if (fields < 1 || fields > kLiftMaxFields) return EQA_ERR_UNSUPPORTED;
  return lift_plan(fields).nstreams;
}

int eqa_steer_lift_fwd(const float* x, const float* wpk, float* y, double* part, int nimg, int H, int W, int Cin, int K, int fields,
                       void* stream) {
  const int st = lift_check(nimg, H, W, Cin, K, fields);
  if (st != EQA_OK) return st;
  if (nimg == 0) return EQA_OK;                     // (an empty batch has no storage: nothing to check, nothing launched)
  if (!x || !wpk || !y) return EQA_ERR_INVALID_ARG;
  if (((uintptr_t)y & 15) || ((uintptr_t)part & 7)) return EQA_ERR_UNSUPPORTED;
  const LiftPlan p = lift_plan(fields);
  hipStream_t hs = (hipStream_t)stream;
#define EQA_LIFT(KK, C) if (K == KK && Cin == C) return lift_fwd_launch<KK, C>(x, wpk, y, part, nimg, H, W, p, hs)
  EQA_LIFT(5, 1); EQA_LIFT(7, 1); EQA_LIFT(9, 1); EQA_LIFT(5, 3); EQA_LIFT(7, 3); EQA_LIFT(9, 3);
#undef EQA_LIFT
  return EQA_ERR_UNSUPPORTED;
}

int64_t eqa_steer_lift_wgrad_workspace_bytes(int Cin, int K, int fields) {
  if (!lift_supported(Cin, K, fields)) return 0;
  const LiftPlan p = lift_plan(fields);
  const int RP = (K * K * Cin + 15) / 16 * 16;
  return (int64_t)p.nstreams * p.ngroups * (16 * p.bpw) * RP * (int64_t)sizeof(float);
}

int eqa_steer_lift_wgrad(const float* x, const float* dy, void* workspace, float* dbank, int nimg, int H, int W, int Cin, int K,
                         int fields, void* stream) {
  const int st = lift_check(nimg, H, W, Cin, K, fields);
  if (st != EQA_OK) return st;
  if (nimg == 0) return EQA_OK;
  if (!x || !dy || !workspace || !dbank) return EQA_ERR_INVALID_ARG;
  if (((uintptr_t)dy & 15) || ((uintptr_t)workspace & 3)) return EQA_ERR_UNSUPPORTED;
  const LiftPlan p = lift_plan(fields);
  hipStream_t hs = (hipStream_t)stream;
  float* part = static_cast<float*>(workspace);
#define EQA_LIFT(KK, C) if (K == KK && Cin == C) return lift_wgrad_launch<KK, C>(x, dy, part, dbank, nimg, H, W, p, hs)
  EQA_LIFT(5, 1); EQA_LIFT(7, 1); EQA_LIFT(9, 1); EQA_LIFT(5, 3); EQA_LIFT(7, 3); EQA_LIFT(9, 3);
#undef EQA_LIFT
  return EQA_ERR_UNSUPPORTED;
}

}  // extern "C"
