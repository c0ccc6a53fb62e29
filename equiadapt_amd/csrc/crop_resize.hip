// libeqa_hip.so, part 6 of 7 -- centre crop + antialiased bilinear resize (I1).  C ABI: include/eqa_hip.h.
#include "eqa_common.hpp"

namespace {

// ------------------------------------------------------------------------------------------------
// I1: centre crop + antialiased bilinear resize (torchvision CenterCrop + Resize on a tensor ==
// F.interpolate(bilinear, antialias=True, align_corners=False); discrete_group.py:174-188).
// Separable like torch's kernel and in the same order: horizontal pass (fp32 intermediates), then vertical pass.
// The per-output-index tap ranges and normalised triangle weights are built on the host with torch's own formula
// (UpSampleKernel.cpp _compute_indices_min_size_weights_aa) and passed as small tables; the crop is folded into the
// tap start indices.  One block = one (image, channel) plane x a band of kAaBand output rows; the band's horizontally
// resampled input rows live in LDS.
// ------------------------------------------------------------------------------------------------
constexpr int kAaBand = 8;  // = the `band` the host tables are built for (geometry.aa_resize_tables); 16 / 32 measured slower
#ifndef EQA_AA_WIDE_MIN_K
#define EQA_AA_WIDE_MIN_K 8  // filters wider than this take the LDS row-staged kernel
#endif
constexpr int kAaMaxK = 20;  // taps kept in registers by the wide-filter kernel (K = 17 at 8x down-sampling)

__global__ __launch_bounds__(kThreads) void crop_resize_aa_kernel(const float* __restrict__ x, float* __restrict__ y,
                                                                 const float* __restrict__ wx, const int32_t* __restrict__ x0,
                                                                 const float* __restrict__ wy, const int32_t* __restrict__ y0,
                                                                 int H, int W, int OH, int OW, int K, int max_rows) {
  extern __shared__ __attribute__((aligned(16))) float aa_tmp[];  // [max_rows][OW]
  const int plane = blockIdx.y;
  const int r0 = blockIdx.x * kAaBand, r1 = min(r0 + kAaBand, OH);
  const int ybeg = y0[r0];
  const int yend = min(y0[r1 - 1] + K, H);  // taps past a row's own range carry zero weight
  const int nrows = min(yend - ybeg, max_rows);
  const float* src = x + (size_t)plane * H * W;
  // K <= EQA_AA_WIDE_MIN_K here.  A thread keeps ONE output column (kThreads / OW rows are worked on at a time, the
  // threads beyond that idle): tap start and weights are loaded once per block instead of once per value, no division per
  // value, and the K loads of a value go out together (unrolled with a predicate).  Measured at 256 x 3 x 224^2 -> 96^2:
  // 123 us with one (row, column) pair per thread and trip, of which 100 us were this pass.
  const int rows_par = kThreads / OW;
  if (rows_par >= 1) {
    const int ox = threadIdx.x % OW, rsub = threadIdx.x / OW;
    if (rsub < rows_par) {
      const int xs = x0[ox];
      float wv[EQA_AA_WIDE_MIN_K];
      int xo[EQA_AA_WIDE_MIN_K];
#pragma unroll
      for (int j = 0; j < EQA_AA_WIDE_MIN_K; ++j) {
        wv[j] = j < K ? wx[ox * K + j] : 0.0f;
        xo[j] = min(xs + j, W - 1);
      }
      // (keeping four row trips' loads in flight at once was tried: 84 -> 92 us, the extra registers cost more occupancy than the
      // shorter dependency chain gains)
      for (int ry = rsub; ry < nrows; ry += rows_par) {
        const float* row = src + (size_t)(ybeg + ry) * W;
        float xv[EQA_AA_WIDE_MIN_K];
#pragma unroll
        for (int j = 0; j < EQA_AA_WIDE_MIN_K; ++j) xv[j] = j < K ? row[xo[j]] : 0.0f;
        float acc = 0.0f;
#pragma unroll
        for (int j = 0; j < EQA_AA_WIDE_MIN_K; ++j)
          if (j < K) acc += wv[j] * xv[j];
        aa_tmp[ry * OW + ox] = acc;
      }
    }
  } else {
    for (int idx = threadIdx.x; idx < nrows * OW; idx += kThreads) {
      const int ry = idx / OW, ox = idx - ry * OW;
      const float* row = src + (size_t)(ybeg + ry) * W;
      const int xs = x0[ox];
      float acc = 0.0f;
#pragma unroll
      for (int j = 0; j < EQA_AA_WIDE_MIN_K; ++j)
        if (j < K) acc += wx[ox * K + j] * row[min(xs + j, W - 1)];
      aa_tmp[ry * OW + ox] = acc;
    }
  }
  __syncthreads();
  float* dst = y + (size_t)plane * OH * OW;
  for (int idx = threadIdx.x; idx < (r1 - r0) * OW; idx += kThreads) {
    const int r = idx / OW, ox = idx - r * OW;
    const int oy = r0 + r;

    const int ys = y0[oy] - ybeg;
    float acc = 0.0f;
#pragma unroll
    for (int j = 0; j < EQA_AA_WIDE_MIN_K; ++j)
      if (j < K) acc += wy[oy * K + j] * aa_tmp[min(ys + j, nrows - 1) * OW + ox];
    dst[(size_t)oy * OW + ox] = acc;
  }
}

// Narrow filters over 16-byte aligned rows (the headline's 224 -> crop 180 -> 96, K = 5), round 3.  The kernel above gathers its K
// taps from global memory (two input rows per trip, one dependent round trip per trip) and chains table load -> address -> data
// load: ~11 us per block whatever its size, 1.65 TB/s.  Here a block keeps ONE band of kAaBand output rows and walks over planes
// (the tables of a band are the same for every plane: loaded once), stages the band's input rows in LDS with 16-byte loads of the
// aligned column window -- the NEXT plane's rows are requested (registers) before this plane's two passes run from LDS, so the
// HBM round trip hides behind the LDS work -- and writes the band.

template <int K, int BAND, int NL>   // K: taps per output index; BAND: output rows per block; NL: 16-byte loads per thread and plane (a template argument: no branch per tap, and the wait counts stay exact)
__global__ __launch_bounds__(kThreads, (NL > 5 && K > 5) ? 2 : 4) void crop_resize_aa_staged_kernel(   // (wide prefetch + many taps: 128 registers spill)
    const float* __restrict__ x, float* __restrict__ y,
                                                                        const float* __restrict__ wx, const int32_t* __restrict__ x0,
                                                                        const float* __restrict__ wy, const int32_t* __restrict__ y0,
                                                                        int planes, int H, int W, int OH, int OW, int cap_rows,
                                                                        int xb, int xl) {
  extern __shared__ __attribute__((aligned(16))) float aa_tmp[];  // rows [cap_rows][xl], the horizontal pass [cap_rows][OW], tables
  float* rows = aa_tmp;
  float* tmp = aa_tmp + (size_t)cap_rows * xl;
  float* tabw = tmp + (size_t)cap_rows * OW;                              // [BAND][K] vertical weights of the band
  int* taby = reinterpret_cast<int*>(tabw + BAND * K);  // [BAND] first input row of each output row
  // grid (8, bands, plane groups): blockIdx.x is the XCD the dispatcher deals the block to (x is the fastest grid axis and 8 wide),
  // so the bands of one plane -- whose input rows overlap by K - 1 and share the cache lines at the window's edges -- are worked on
  // by blocks of ONE XCD at about the same time and meet in its L2 (round 3: band b of every plane on XCD b % 8, the overlap rows
  // fetched from HBM twice: 1.38 x the algorithmic bytes)
  const int r0 = blockIdx.y * BAND, r1 = min(r0 + BAND, OH);
  const int nband = r1 - r0;
  const int plane0 = (int)(blockIdx.z * kXcd + blockIdx.x), plane_step = (int)(gridDim.z * kXcd);
  const int rows_par = kThreads / OW;
  const int ox = rows_par >= 1 ? threadIdx.x % OW : 0, rsub = rows_par >= 1 ? threadIdx.x / OW : 0;
  const int xs_g = x0[ox];
  float wv[K];
  int xo[K];
#pragma unroll
  for (int j = 0; j < K; ++j) {
    wv[j] = wx[ox * K + j];
    xo[j] = min(xs_g - xb + j, xl - 1);
  }
  if ((int)threadIdx.x < nband * K) tabw[threadIdx.x] = wy[r0 * K + threadIdx.x];
  const int ybeg = y0[r0];
  if ((int)threadIdx.x < nband) taby[threadIdx.x] = y0[r0 + threadIdx.x] - ybeg;
  const int yend = min(y0[r1 - 1] + K, H);
  const int nrows = min(yend - ybeg, cap_rows);
  const int nq = xl >> 2;
  const int tq = threadIdx.x & 63, tr = threadIdx.x >> 6;
  const bool prefetch = nq <= 64 && nrows <= 4 * NL;   // uniform: one 16-byte load per (thread, row group member)
  const size_t plane_sz = (size_t)H * W;
  const float* src0 = x + (size_t)ybeg * W + xb;
  typedef float aa_f4 __attribute__((ext_vector_type(4)));
  aa_f4 v[NL];
  // (a macro, not a lambda: called from two places the lambda is not inlined and v[] goes to scratch)
#define EQA_AA_PF_LOAD(plane_)                                                                                          \
  do {                                                                                                                  \
    const float* src_ = src0 + (size_t)(plane_) * plane_sz;                                                             \
    _Pragma("unroll") for (int k = 0; k < NL; ++k)                                                           \
      v[k] = *reinterpret_cast<const aa_f4*>(src_ + (size_t)min(tr + 4 * k, nrows - 1) * W + 4 * min(tq, nq - 1));     \
  } while (0)
  // the tables have arrived before the first row is requested: from here on only row loads are ever outstanding, and the waits
  // the compiler places inside the passes are for those it names (a pending table load made them vmcnt(0): the prefetch drained)
  __builtin_amdgcn_s_waitcnt(0x0070);
  if (prefetch && plane0 < planes) EQA_AA_PF_LOAD(plane0);
  for (int plane = plane0; plane < planes; plane += plane_step) {
    if (prefetch) {
      if (tq < nq) {
#pragma unroll
        for (int k = 0; k < NL; ++k)
          if (tr + 4 * k < nrows) *reinterpret_cast<aa_f4*>(rows + (tr + 4 * k) * xl + 4 * tq) = v[k];
      }
      if (plane + plane_step < planes) EQA_AA_PF_LOAD(plane + plane_step);
    } else {
      const float* src = src0 + (size_t)plane * plane_sz;
      for (int q = tq; q < nq; q += 64)
        for (int rb = tr; rb < nrows; rb += 4) *reinterpret_cast<aa_f4*>(rows + rb * xl + 4 * q) = *reinterpret_cast<const aa_f4*>(src + (size_t)rb * W + 4 * q);
    }
    __syncthreads();
    // horizontal pass (fp32 intermediates, as torch's kernel): a thread keeps one output column -- tap starts and weights in registers
    if (rows_par >= 1) {
      if (rsub < rows_par) {
        for (int ry0 = rsub; ry0 < nrows; ry0 += 4 * rows_par) {   // four rows' taps in flight at once (LDS latency, not bandwidth)
          float acc[4] = {0.0f, 0.0f, 0.0f, 0.0f};
#pragma unroll
          for (int u = 0; u < 4; ++u) {
            const float* row = rows + min(ry0 + u * rows_par, nrows - 1) * xl;
#pragma unroll
            for (int j = 0; j < K; ++j)
              acc[u] += wv[j] * row[xo[j]];
          }
#pragma unroll
          for (int u = 0; u < 4; ++u)
            if (ry0 + u * rows_par < nrows) tmp[(ry0 + u * rows_par) * OW + ox] = acc[u];
        }
      }
    } else {
      for (int idx = threadIdx.x; idx < nrows * OW; idx += kThreads) {
        const int ry = idx / OW, oxx = idx - ry * OW;
        const float* row = rows + ry * xl;
        const int xs = x0[oxx] - xb;
        float acc = 0.0f;
#pragma unroll
        for (int j = 0; j < K; ++j)
          acc += wx[oxx * K + j] * row[min(xs + j, xl - 1)];
        tmp[ry * OW + oxx] = acc;
      }
    }
    __syncthreads();
    float* dst = y + (size_t)plane * OH * OW;
    for (int idx = threadIdx.x; idx < nband * OW; idx += kThreads) {
      const int r = idx / OW, oxx = idx - r * OW;
      const int ys = taby[r];
      float acc = 0.0f;
#pragma unroll
      for (int j = 0; j < K; ++j)
        acc += tabw[r * K + j] * tmp[min(ys + j, nrows - 1) * OW + oxx];
      dst[(size_t)(r0 + r) * OW + oxx] = acc;
    }
    __syncthreads();   // the next plane's horizontal pass overwrites tmp
  }
#undef EQA_AA_PF_LOAD
}

// Wide filters (K > 8, i.e. down-sampling by more than ~3.5x: config 5 resizes 1024 -> 128 with 17 taps): the K strided
// global loads per intermediate value of the kernel above become the bottleneck (0.73 ms for 32 x 3 x 1024^2, 9x its HBM
// time).  Here every needed input row segment is first staged into LDS with coalesced loads, `rpi` rows per iteration,
// and the taps are taken from LDS.  Neighbouring lanes read addresses ~scale apart; for an even integer stride s = 2^a m
// (m odd) the row is stored with one pad float every 2^a elements, which makes the lane stride s + m odd (conflict-free).
__global__ __launch_bounds__(kThreads) void crop_resize_aa_wide_kernel(const float* __restrict__ x, float* __restrict__ y,
                                                                      const float* __restrict__ wx, const int32_t* __restrict__ x0,
                                                                      const float* __restrict__ wy, const int32_t* __restrict__ y0,
                                                                      int H, int W, int OH, int OW, int K, int max_rows, int xbeg,
                                                                      int xlen, int pad_shift, int row_stride, int rpi) {
  extern __shared__ __attribute__((aligned(16))) float aa_tmp[];  // [max_rows][OW] then [rpi][row_stride]
  float* rowbuf = aa_tmp + (size_t)max_rows * OW;
  const int plane = blockIdx.y;
  const int r0 = blockIdx.x * kAaBand, r1 = min(r0 + kAaBand, OH);
  const int ybeg = y0[r0];
  const int yend = min(y0[r1 - 1] + K, H);
  const int nrows = min(yend - ybeg, max_rows);
  const float* src = x + (size_t)plane * H * W;
  auto pos = [&](int e) { return pad_shift ? e + (e >> pad_shift) : e; };
  const bool fixed_col = (kThreads % OW) == 0 && K <= kAaMaxK;
  // whole float4s of 16-byte aligned rows (uniform): the staging below then loads 16 bytes per lane
  const bool vec_stage = rpi <= 8 && (xlen & 3) == 0 && (xbeg & 3) == 0 && (W & 3) == 0 && ((((uintptr_t)src) & 15) == 0);
  const int ox_fixed = threadIdx.x % OW;
  const int xs_fixed = x0[ox_fixed] - xbeg;
  float wreg[kAaMaxK];
#pragma unroll
  for (int j = 0; j < kAaMaxK; ++j) wreg[j] = (fixed_col && j < K) ? wx[ox_fixed * K + j] : 0.0f;
  // Rows no wider than one float4 per thread (1024 floats: config 5): the NEXT iteration's rows are requested before this
  // iteration's taps are taken, so the HBM round trip of an iteration hides behind the previous one's LDS work (round 3; a block
  // runs ~10 iterations and only two blocks fit a CU, so each exposed round trip was paid in full: 171 -> see DESIGN 3.7).
  const bool prefetch = vec_stage && xlen <= 4 * kThreads;
  const int e_pf = 4 * threadIdx.x;
  float4 pf[8];
  auto pf_load = [&](int ry0) {
    const int nr = min(rpi, nrows - ry0);
#pragma unroll
    for (int rr = 0; rr < 8; ++rr)
      pf[rr] = *reinterpret_cast<const float4*>(src + (size_t)(ybeg + ry0 + min(rr, nr - 1)) * W + xbeg + min(e_pf, xlen - 4));
  };
  if (prefetch && nrows > 0) pf_load(0);
  for (int ry0 = 0; ry0 < nrows; ry0 += rpi) {
    const int nr = min(rpi, nrows - ry0);
    if (prefetch) {
      if (e_pf < xlen) {
#pragma unroll
        for (int rr = 0; rr < 8; ++rr) {
          if (rr < nr) {
            float* lrow = rowbuf + rr * row_stride;
            lrow[pos(e_pf)] = pf[rr].x; lrow[pos(e_pf + 1)] = pf[rr].y; lrow[pos(e_pf + 2)] = pf[rr].z; lrow[pos(e_pf + 3)] = pf[rr].w;
          }
        }
      }
      if (ry0 + rpi < nrows) pf_load(ry0 + rpi);
    } else if (vec_stage) {
      // 16-byte loads, one per (row, thread) and trip, ALL rows' loads in flight before the first LDS store: the rolled
      // load -> store loop paid one HBM round trip per row and 256 floats (32 trips per iteration of 8 rows of 1024)
      for (int e = 4 * threadIdx.x; e < xlen; e += 4 * kThreads) {
        float4 v[8];
#pragma unroll
        for (int rr = 0; rr < 8; ++rr)
          v[rr] = *reinterpret_cast<const float4*>(src + (size_t)(ybeg + ry0 + min(rr, nr - 1)) * W + xbeg + e);
#pragma unroll
        for (int rr = 0; rr < 8; ++rr) {
          if (rr < nr) {
            float* lrow = rowbuf + rr * row_stride;
            lrow[pos(e)] = v[rr].x; lrow[pos(e + 1)] = v[rr].y; lrow[pos(e + 2)] = v[rr].z; lrow[pos(e + 3)] = v[rr].w;
          }
        }
      }
    } else {
      for (int rr = 0; rr < nr; ++rr) {
        const float* grow = src + (size_t)(ybeg + ry0 + rr) * W + xbeg;
        float* lrow = rowbuf + rr * row_stride;
        for (int e = threadIdx.x; e < xlen; e += kThreads) lrow[pos(e)] = grow[e];  // xbeg + xlen <= W
      }
    }
    __syncthreads();
    if (fixed_col) {  // kThreads % OW == 0: the thread keeps its output column, weights and tap start live in registers
      for (int rr = threadIdx.x / OW; rr < nr; rr += kThreads / OW) {
        const float* row = rowbuf + rr * row_stride;
        float acc = 0.0f;
#pragma unroll
        for (int j = 0; j < kAaMaxK; ++j)
          if (j < K) acc += wreg[j] * row[pos(min(xs_fixed + j, xlen - 1))];
        aa_tmp[(ry0 + rr) * OW + ox_fixed] = acc;
      }
    } else {
      for (int idx = threadIdx.x; idx < nr * OW; idx += kThreads) {
        const int rr = idx / OW, ox = idx - rr * OW;
        const float* row = rowbuf + rr * row_stride;
        const int xs = x0[ox] - xbeg;
        float acc = 0.0f;
        for (int j = 0; j < K; ++j) acc += wx[ox * K + j] * row[pos(min(xs + j, xlen - 1))];
        aa_tmp[(ry0 + rr) * OW + ox] = acc;
      }
    }
    __syncthreads();
  }
  float* dst = y + (size_t)plane * OH * OW;
  for (int idx = threadIdx.x; idx < (r1 - r0) * OW; idx += kThreads) {
    const int r = idx / OW, ox = idx - r * OW;
    const int oy = r0 + r;
    const int ys = y0[oy] - ybeg;
    float acc = 0.0f;
    for (int j = 0; j < K; ++j) acc += wy[oy * K + j] * aa_tmp[min(ys + j, nrows - 1) * OW + ox];
    dst[(size_t)oy * OW + ox] = acc;
  }
}

// The same for rows no wider than one float4 per thread (x_span <= 1024: config 5), VERTICAL pass first and without staging the
// input: the row-staged kernel above keeps one block per CU (74 KB intermediate band + 37 KB of staged rows) and 32 KB of loads in
// flight between two barriers per eight input rows -- 155 us for 32 x 3 x 1024^2 (2.6 TB/s).  Here a thread owns four columns:
// every input row of the band's span is loaded ONCE, 16 bytes per lane, eight rows ahead, and added to the band's eight output
// rows with its (uniform) vertical weight -- zero outside a row's K taps, so any overlap of the windows is handled -- and only the
// eight finished 1024-wide rows go through LDS (four at a time, 18 KB) for the horizontal taps.  Four blocks per CU, 128 KB of loads
// in flight per CU, four barriers per block.  (Summation order: vertical taps first; the staged kernels sum the horizontal taps first.)
constexpr int kAaStreamRows = 8;
__global__ __launch_bounds__(kThreads) void crop_resize_aa_stream_kernel(const float* __restrict__ x, float* __restrict__ y,
                                                                        const float* __restrict__ wx, const int32_t* __restrict__ x0,
                                                                        const float* __restrict__ wy, const int32_t* __restrict__ y0,
                                                                        int H, int W, int OH, int OW, int K, int xbeg, int xlen,
                                                                        int pad_shift, int row_stride) {
  extern __shared__ __attribute__((aligned(16))) float aa_rows[];   // [kAaBand / 2][row_stride]
  const int plane = blockIdx.y;
  const int r0 = blockIdx.x * kAaBand, nr_out = min(kAaBand, OH - r0);
  int ys[kAaBand];                                                   // first input row of each output row (uniform)
#pragma unroll
  for (int r = 0; r < kAaBand; ++r) ys[r] = y0[r0 + min(r, nr_out - 1)];
  const int ybeg = ys[0];
  const int span = ys[kAaBand - 1] + K - ybeg;                       // input rows the band touches (ys is non-decreasing)
  const float* src = x + (size_t)plane * H * W + xbeg;
  const int e = 4 * (int)threadIdx.x;
  const int e_ld = min(e, xlen - 4);
  auto pos = [&](int i) { return pad_shift ? i + (i >> pad_shift) : i; };
  float4 acc[kAaBand];
#pragma unroll
  for (int r = 0; r < kAaBand; ++r) acc[r] = make_float4(0.f, 0.f, 0.f, 0.f);
  auto load8 = [&](float4 (&v)[kAaStreamRows], int yc) {           // rows ybeg + yc .. + 7 (clamped to the image: their weights are 0)
#pragma unroll
    for (int q = 0; q < kAaStreamRows; ++q)
      v[q] = *reinterpret_cast<const float4*>(src + (size_t)min(ybeg + yc + q, H - 1) * W + e_ld);
  };
  // the 8 x 8 vertical weights of a trip (input row q of the trip, output row r): lane 8 q + r loads its one weight, the others
  // get it by v_readlane (64 scalar loads in a chain, one per weight, cost 13 k cycles a trip: every one waited out its latency)
  const int lane = threadIdx.x & 63;
  const int wq = lane >> 3, wr = lane & 7;
  const int ys_w = y0[r0 + min(wr, nr_out - 1)];
  auto wload = [&](int yc) {
    const int t = ybeg + yc + wq - ys_w;
    const bool ok = wr < nr_out && t >= 0 && t < K && yc + wq < span;
    return ok ? wy[(size_t)(r0 + wr) * K + min(max(t, 0), K - 1)] : 0.0f;
  };
  auto add8 = [&](const float4 (&v)[kAaStreamRows], float wv) {
#pragma unroll
    for (int q = 0; q < kAaStreamRows; ++q) {
#pragma unroll
      for (int r = 0; r < kAaBand; ++r) {
        const float w = __builtin_bit_cast(float, __builtin_amdgcn_readlane(__builtin_bit_cast(int, wv), 8 * q + r));
        acc[r].x += w * v[q].x; acc[r].y += w * v[q].y; acc[r].z += w * v[q].z; acc[r].w += w * v[q].w;
      }
    }
  };
  static_assert(kAaStreamRows == 8 && kAaBand == 8, "one weight per lane: 8 rows of a trip x 8 output rows = 64 lanes");
  float4 va[kAaStreamRows], vb[kAaStreamRows];
  float wa, wb = 0.0f;
  load8(va, 0);
  wa = wload(0);
  for (int yc = 0; yc < span; yc += 2 * kAaStreamRows) {
    if (yc + kAaStreamRows < span) { load8(vb, yc + kAaStreamRows); wb = wload(yc + kAaStreamRows); }
    add8(va, wa);
    if (yc + 2 * kAaStreamRows < span) { load8(va, yc + 2 * kAaStreamRows); wa = wload(yc + 2 * kAaStreamRows); }
    if (yc + kAaStreamRows < span) add8(vb, wb);
  }
  float* dst = y + (size_t)plane * OH * OW;
#pragma unroll
  for (int half = 0; half < 2; ++half) {
    if (e < xlen) {
#pragma unroll
      for (int rr = 0; rr < kAaBand / 2; ++rr) {
        float* lrow = aa_rows + rr * row_stride;
        const float4 v = acc[half * (kAaBand / 2) + rr];
        lrow[pos(e)] = v.x; lrow[pos(e + 1)] = v.y; lrow[pos(e + 2)] = v.z; lrow[pos(e + 3)] = v.w;
      }
    }
    __syncthreads();
    for (int idx = threadIdx.x; idx < (kAaBand / 2) * OW; idx += kThreads) {
      const int rr = idx / OW, ox = idx - rr * OW;
      const int r = half * (kAaBand / 2) + rr;
      if (r < nr_out) {
        const float* row = aa_rows + rr * row_stride;
        const int xs = x0[ox] - xbeg;
        float a = 0.0f;
        for (int j = 0; j < K; ++j) a += wx[ox * K + j] * row[pos(min(xs + j, xlen - 1))];
        dst[(size_t)(r0 + r) * OW + ox] = a;
      }
    }
    __syncthreads();
  }
}

// The staged kernel for a consumer that reads pixels, not planes (the fused lifting kernel: (B, H, W, C)), and that wants a bound on
// |y| beside them (it scales its pixels under one).  A block owns a band of IMAGES, not of planes: it runs the staged kernel's two
// passes for the C planes of an image in turn -- same tables, same taps, same order of additions, so every pixel has the bits the
// planar kernel gives it; the next plane's rows are requested before this one's passes run from LDS, across image boundaries as
// well -- keeps the band's C x BAND x OW results in registers and stores them as ONE contiguous run of BAND * OW * C floats (as a
// planar result the consumer's .contiguous(channels_last) was a 28 MB permute per step at the headline, and the bound a second
// pass over the same 28 MB).  The largest |y| a block has stored goes to slots[block]: no atomics, nothing to clear; fmaxf drops
// a NaN and carries an infinity, as absmax_slots_kernel (lift_fft.hip) does.
constexpr int kAaNhwcTrips = 6;   // results per thread and plane: BAND * OW <= 6 * 256 (16 rows of 96)

// (the C x kAaNhwcTrips results on top of the staged kernel's 127 registers: three blocks per CU -- what the 45 KB of a 16-row band
// admit anyway -- instead of four; at four, 42 registers of the headline's instance went to scratch)
template <int K, int BAND, int NL, int C>
__global__ __launch_bounds__(kThreads, (NL > 5 && K > 5) ? 2 : 3) void crop_resize_aa_nhwc_kernel(
    const float* __restrict__ x, float* __restrict__ y, const float* __restrict__ wx, const int32_t* __restrict__ x0,
    const float* __restrict__ wy, const int32_t* __restrict__ y0, int nimg, int H, int W, int OH, int OW, int cap_rows, int xb, int xl,
    float* __restrict__ slots) {
  extern __shared__ __attribute__((aligned(16))) float aa_tmp[];  // as crop_resize_aa_staged_kernel
  float* rows = aa_tmp;
  float* tmp = aa_tmp + (size_t)cap_rows * xl;
  float* tabw = tmp + (size_t)cap_rows * OW;
  int* taby = reinterpret_cast<int*>(tabw + BAND * K);
  __shared__ float s_max[kThreads / 64];
  // grid (8, bands, image groups): the bands of one image on one XCD, as the planar kernel keeps the bands of a plane
  const int r0 = blockIdx.y * BAND, r1 = min(r0 + BAND, OH);
  const int nband = r1 - r0;
  const int img0 = (int)(blockIdx.z * kXcd + blockIdx.x), img_step = (int)(gridDim.z * kXcd);
  const int rows_par = kThreads / OW;   // >= 1: OW <= kThreads (the host checks)
  const int ox = threadIdx.x % OW, rsub = threadIdx.x / OW;
  const int xs_g = x0[ox];
  float wv[K];
  int xo[K];
#pragma unroll
  for (int j = 0; j < K; ++j) {
    wv[j] = wx[ox * K + j];
    xo[j] = min(xs_g - xb + j, xl - 1);
  }
  if ((int)threadIdx.x < nband * K) tabw[threadIdx.x] = wy[r0 * K + threadIdx.x];
  const int ybeg = y0[r0];
  if ((int)threadIdx.x < nband) taby[threadIdx.x] = y0[r0 + threadIdx.x] - ybeg;
  const int yend = min(y0[r1 - 1] + K, H);
  const int nrows = min(yend - ybeg, cap_rows);
  const int nq = xl >> 2;
  const int tq = threadIdx.x & 63, tr = threadIdx.x >> 6;
  const bool prefetch = nq <= 64 && nrows <= 4 * NL;
  const size_t plane_sz = (size_t)H * W;
  const float* src0 = x + (size_t)ybeg * W + xb;
  typedef float aa_f4 __attribute__((ext_vector_type(4)));
  aa_f4 v[NL];
#define EQA_AA_PF_LOAD(plane_)                                                                                          \
  do {                                                                                                                  \
    const float* src_ = src0 + (size_t)(plane_) * plane_sz;                                                             \
    _Pragma("unroll") for (int k = 0; k < NL; ++k)                                                           \
      v[k] = *reinterpret_cast<const aa_f4*>(src_ + (size_t)min(tr + 4 * k, nrows - 1) * W + 4 * min(tq, nq - 1));     \
  } while (0)
  __builtin_amdgcn_s_waitcnt(0x0070);   // the tables have arrived: from here on only row loads are outstanding (see above)
  if (prefetch && img0 < nimg) EQA_AA_PF_LOAD((size_t)img0 * C);
  const int nout = nband * OW;          // <= kAaNhwcTrips * kThreads (the host checks)
  float mx = 0.0f;
  for (int img = img0; img < nimg; img += img_step) {
    float o[kAaNhwcTrips][C];
#pragma unroll
    for (int c = 0; c < C; ++c) {
      const size_t plane = (size_t)img * C + c;
      if (prefetch) {
        if (tq < nq) {
#pragma unroll
          for (int k = 0; k < NL; ++k)
            if (tr + 4 * k < nrows) *reinterpret_cast<aa_f4*>(rows + (tr + 4 * k) * xl + 4 * tq) = v[k];
        }
        if (c + 1 < C) EQA_AA_PF_LOAD(plane + 1);
        else if (img + img_step < nimg) EQA_AA_PF_LOAD((size_t)(img + img_step) * C);
      } else {
        const float* src = src0 + plane * plane_sz;
        for (int q = tq; q < nq; q += 64)
          for (int rb = tr; rb < nrows; rb += 4) *reinterpret_cast<aa_f4*>(rows + rb * xl + 4 * q) = *reinterpret_cast<const aa_f4*>(src + (size_t)rb * W + 4 * q);
      }
      __syncthreads();
      // horizontal pass: crop_resize_aa_staged_kernel's, addition for addition
      if (rsub < rows_par) {
        for (int ry0 = rsub; ry0 < nrows; ry0 += 4 * rows_par) {
          float acc[4] = {0.0f, 0.0f, 0.0f, 0.0f};
#pragma unroll
          for (int u = 0; u < 4; ++u) {
            const float* row = rows + min(ry0 + u * rows_par, nrows - 1) * xl;
#pragma unroll
            for (int j = 0; j < K; ++j)
              acc[u] += wv[j] * row[xo[j]];
          }
#pragma unroll
          for (int u = 0; u < 4; ++u)
            if (ry0 + u * rows_par < nrows) tmp[(ry0 + u * rows_par) * OW + ox] = acc[u];
        }
      }
      __syncthreads();
      // vertical pass, into registers: result t of this thread is element threadIdx.x + t * kThreads of the band's (row, column)
      // run, i.e. (r, oxx) stepped from (rsub, ox) by kThreads elements a trip (no division per value)
      int r = rsub, oxx = ox;
#pragma unroll
      for (int t = 0; t < kAaNhwcTrips; ++t) {
        float acc = 0.0f;
        if (r < nband) {
          const int ys = taby[r];
#pragma unroll
          for (int j = 0; j < K; ++j)
            acc += tabw[r * K + j] * tmp[min(ys + j, nrows - 1) * OW + oxx];
        }
        o[t][c] = acc;
        r += rows_par;
        oxx += kThreads - rows_par * OW;
        if (oxx >= OW) { oxx -= OW; ++r; }
      }
      __syncthreads();   // the next plane's passes overwrite rows and tmp
    }
    float* dst = y + ((size_t)img * OH + r0) * OW * C;   // the band of an image: one run of nout * C floats
#pragma unroll
    for (int t = 0; t < kAaNhwcTrips; ++t) {
      const int idx = (int)threadIdx.x + t * kThreads;
      if (idx < nout) {
#pragma unroll
        for (int c = 0; c < C; ++c) {
          dst[(size_t)idx * C + c] = o[t][c];
          mx = fmaxf(mx, fabsf(o[t][c]));
        }
      }
    }
  }
#undef EQA_AA_PF_LOAD
  if (slots) {   // one per block, written whatever the block did (a block without an image: 0)
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) mx = fmaxf(mx, __shfl_xor(mx, off));
    if ((threadIdx.x & 63) == 0) s_max[threadIdx.x >> 6] = mx;
    __syncthreads();
    if (threadIdx.x == 0)
      slots[((size_t)blockIdx.z * gridDim.y + blockIdx.y) * gridDim.x + blockIdx.x] = fmaxf(fmaxf(s_max[0], s_max[1]), fmaxf(s_max[2], s_max[3]));
  }
}

// what the channels-last launch and its slot query share: the staged kernel's band and LDS rules, and a grid of image groups
struct AaNhwcPlan {
  int band, cap_rows, xb, xl, nbands, groups;
  size_t lds;
  bool few;
};

int aa_nhwc_plan(int nimg, int C, int H, int W, int OH, int OW, int K, int max_rows, int x_begin, int x_span, AaNhwcPlan& p) {
  if (nimg < 0 || C <= 0 || H <= 0 || W <= 0 || OH <= 0 || OW <= 0 || K <= 0 || max_rows <= 0) return EQA_ERR_INVALID_ARG;
  if ((C != 1 && C != 3) || K > EQA_AA_WIDE_MIN_K || (W & 3) != 0 || x_span <= 0 || x_begin < 0 || x_begin + x_span > W) return EQA_ERR_UNSUPPORTED;
  p.xb = x_begin & ~3;
  p.xl = std::min(W, (x_begin + x_span + 3) & ~3) - p.xb;
  auto staged_lds = [&](int bnd) { return ((size_t)(bnd / kAaBand) * max_rows * (p.xl + OW) + bnd * (EQA_AA_WIDE_MIN_K + 1)) * sizeof(float); };
  p.band = OH >= 64 ? 16 : 8;
  if (p.band == 16 && (staged_lds(16) > 64 * 1024 || 16 * K > kThreads || 16 * OW > kAaNhwcTrips * kThreads)) p.band = 8;
  p.cap_rows = (p.band / kAaBand) * max_rows;
  p.lds = staged_lds(p.band);
  if (p.lds > 64 * 1024 || p.band * K > kThreads || p.band * OW > kAaNhwcTrips * kThreads || OW > kThreads) return EQA_ERR_UNSUPPORTED;
  // about three resident blocks per CU in all (what the band's LDS admits at the headline), each walking images: every block is
  // resident from the start, and the consumer reads one slot per block
  static const int per_cu = [] { const char* e = getenv("EQA_AA_NHWC_BLOCKS_PER_CU"); return e ? std::max(1, atoi(e)) : 3; }();
  p.nbands = (OH + p.band - 1) / p.band;
  p.groups = std::max(1, (std::min(nimg, (256 * per_cu + p.nbands - 1) / p.nbands) + kXcd - 1) / kXcd);
  p.few = p.cap_rows <= 20;
  return p.groups > 65535 ? EQA_ERR_UNSUPPORTED : EQA_OK;
}

}  // namespace

extern "C" {

int eqa_crop_resize_aa_nhwc_slots(int nimg, int C, int H, int W, int OH, int OW, int K, int max_rows, int x_begin, int x_span) {
  AaNhwcPlan p;
  const int rc = aa_nhwc_plan(nimg, C, H, W, OH, OW, K, max_rows, x_begin, x_span, p);
  return rc != EQA_OK ? rc : kXcd * p.nbands * p.groups;
}

int eqa_crop_resize_aa_nhwc(const float* x, float* y, const float* wx, const int32_t* x0, const float* wy, const int32_t* y0, int nimg,
                            int C, int H, int W, int OH, int OW, int K, int max_rows, int x_begin, int x_span, float* slots, void* stream) {
  if (!x || !y || !wx || !x0 || !wy || !y0) return EQA_ERR_INVALID_ARG;
  AaNhwcPlan p;
  const int rc = aa_nhwc_plan(nimg, C, H, W, OH, OW, K, max_rows, x_begin, x_span, p);
  if (rc != EQA_OK) return rc;
  if ((((uintptr_t)x) & 15) != 0) return EQA_ERR_UNSUPPORTED;
  const dim3 grid(kXcd, p.nbands, p.groups);   // (no images: every block still writes its slot, 0)
#define EQA_AA_NHWC_C(K_, C_)                                                                                                          \
  do {                                                                                                                                 \
    if (p.band == 16)                                                                                                                  \
      hipLaunchKernelGGL((crop_resize_aa_nhwc_kernel<K_, 16, 10, C_>), grid, dim3(kThreads), p.lds, (hipStream_t)stream, x, y, wx, x0, wy, \
                         y0, nimg, H, W, OH, OW, p.cap_rows, p.xb, p.xl, slots);                                                       \
    else if (p.few)                                                                                                                    \
      hipLaunchKernelGGL((crop_resize_aa_nhwc_kernel<K_, 8, 5, C_>), grid, dim3(kThreads), p.lds, (hipStream_t)stream, x, y, wx, x0, wy,  \
                         y0, nimg, H, W, OH, OW, p.cap_rows, p.xb, p.xl, slots);                                                       \
    else                                                                                                                               \
      hipLaunchKernelGGL((crop_resize_aa_nhwc_kernel<K_, 8, 10, C_>), grid, dim3(kThreads), p.lds, (hipStream_t)stream, x, y, wx, x0, wy, \
                         y0, nimg, H, W, OH, OW, p.cap_rows, p.xb, p.xl, slots);                                                       \
  } while (0)
#define EQA_AA_NHWC(K_)                                    \
  case K_:                                                 \
    if (C == 3) EQA_AA_NHWC_C(K_, 3);                      \
    else EQA_AA_NHWC_C(K_, 1);                             \
    break
  switch (K) {
    EQA_AA_NHWC(1); EQA_AA_NHWC(2); EQA_AA_NHWC(3); EQA_AA_NHWC(4); EQA_AA_NHWC(5); EQA_AA_NHWC(6); EQA_AA_NHWC(7); EQA_AA_NHWC(8);
    default: return EQA_ERR_UNSUPPORTED;
  }
#undef EQA_AA_NHWC
#undef EQA_AA_NHWC_C
  return launch_status();
}

int eqa_crop_resize_aa(const float* x, float* y, const float* wx, const int32_t* x0, const float* wy, const int32_t* y0,
                       int planes, int H, int W, int OH, int OW, int K, int max_rows, int x_begin, int x_span, void* stream) {
  if (!x || !y || !wx || !x0 || !wy || !y0 || planes < 0 || H <= 0 || W <= 0 || OH <= 0 || OW <= 0 || K <= 0 || max_rows <= 0)
    return EQA_ERR_INVALID_ARG;
  const size_t lds = (size_t)max_rows * OW * sizeof(float);
  if (lds > 96 * 1024 || planes > 65535) return EQA_ERR_UNSUPPORTED;
  if (planes == 0) return EQA_OK;
  const dim3 grid((OH + kAaBand - 1) / kAaBand, planes);
  if (K > EQA_AA_WIDE_MIN_K && x_span > 0 && x_begin >= 0 && x_begin + x_span <= W) {
    // wide filters: stage the input rows in LDS.  Lanes read ~x_span / OW floats apart; make that stride odd.
    const int stride = (x_span + OW / 2) / OW;
    const int pad_shift = (stride >= 2 && (stride & 1) == 0) ? __builtin_ctz((unsigned)stride) : 0;
    const int row_stride = x_span + (pad_shift ? (x_span >> pad_shift) : 0) + 1;
    // input rows staged per iteration: as many as fit next to the intermediate band (fewer barrier rounds), at most 8
    const size_t row_bytes = (size_t)row_stride * sizeof(float);
    const int rpi = (int)std::min<size_t>(8, lds + row_bytes <= 96 * 1024 ? (96 * 1024 - lds) / row_bytes : 0);
    const size_t lds2 = lds + (size_t)rpi * row_bytes;
    static const bool stream_off = [] { const char* e = getenv("EQA_AA_STREAM"); return e && e[0] == '0'; }();
    if (!stream_off && x_span <= 4 * kThreads && (x_span & 3) == 0 && (x_begin & 3) == 0 && (W & 3) == 0 && (((uintptr_t)x) & 15) == 0 &&
        (size_t)(kAaBand / 2) * row_bytes <= 64 * 1024) {
      hipLaunchKernelGGL(crop_resize_aa_stream_kernel, grid, dim3(kThreads), (kAaBand / 2) * row_bytes, (hipStream_t)stream, x, y, wx, x0, wy,
                         y0, H, W, OH, OW, K, x_begin, x_span, pad_shift, row_stride);
      return launch_status();
    }
    if (rpi >= 1) {
      hipLaunchKernelGGL(crop_resize_aa_wide_kernel, grid, dim3(kThreads), lds2, (hipStream_t)stream, x, y, wx, x0, wy, y0, H, W, OH,
                         OW, K, max_rows, x_begin, x_span, pad_shift, row_stride, rpi);
      return launch_status();
    }
  }
  // narrow filters over aligned rows: the LDS-staged form (whole band requested at once)
  static const bool staged_off = [] { const char* e = getenv("EQA_AA_STAGED"); return e && e[0] == '0'; }();
  if (!staged_off && K <= EQA_AA_WIDE_MIN_K && (W & 3) == 0 && (((uintptr_t)x) & 15) == 0 && x_span > 0 && x_begin >= 0 &&
      x_begin + x_span <= W) {
    const int xb = x_begin & ~3, xl = std::min(W, (x_begin + x_span + 3) & ~3) - xb;
    // 16 output rows per block where the map has at least four such bands: 4 of 34 staged rows are shared with the next band instead of
    // 4 of 19 (with the bands of a plane on one XCD -- round 4 -- 35.9 us per 256 x 3 planes of 224 -> 180 -> 96 against 39-40 for
    // bands of 8; before that mapping the larger band was the slower one).  EQA_AA_BAND=8 / 16 forces either.
    static const int band_env = [] { const char* e = getenv("EQA_AA_BAND"); return e ? atoi(e) : 0; }();
    int band = band_env == 16 ? 16 : (band_env == 8 ? 8 : (OH >= 64 ? 16 : 8));
    auto staged_lds = [&](int bnd) { return ((size_t)(bnd / kAaBand) * max_rows * (xl + OW) + bnd * (EQA_AA_WIDE_MIN_K + 1)) * sizeof(float); };
    if (band == 16 && band_env != 16 && (staged_lds(16) > 64 * 1024 || 16 * K > kThreads)) band = 8;   // the smaller band may still fit
    const int cap_rows = (band / kAaBand) * max_rows;   // a band of 16 rows = two of the 8-row bands `max_rows` was taken over
    const size_t lds3 = staged_lds(band);
    if (lds3 <= 64 * 1024 && band * K <= kThreads) {
      // persistent over planes: about 8 resident blocks per CU in all, each walking planes with a stride of gridDim.y
      static const int per_cu = [] { const char* e = getenv("EQA_AA_BLOCKS_PER_CU"); return e ? std::max(1, atoi(e)) : 12; }();
      const int nbands = (OH + band - 1) / band;
      const int groups = std::max(1, (std::min(planes, (256 * per_cu + nbands - 1) / nbands) + kXcd - 1) / kXcd);   // plane groups of 8 (one plane per XCD)
      const bool few = cap_rows <= 20;   // 5 loads per thread cover the band's rows (else 10: up to 40 rows)
#define EQA_AA_STAGED(K_)                                                                                                              \
  case K_:                                                                                                                             \
    if (band == 16)                                                                                                                    \
      hipLaunchKernelGGL((crop_resize_aa_staged_kernel<K_, 16, 10>), dim3(kXcd, nbands, groups), dim3(kThreads), lds3, (hipStream_t)stream, x, \
                         y, wx, x0, wy, y0, planes, H, W, OH, OW, cap_rows, xb, xl);                                                   \
    else if (few)                                                                                                                      \
      hipLaunchKernelGGL((crop_resize_aa_staged_kernel<K_, 8, 5>), dim3(kXcd, nbands, groups), dim3(kThreads), lds3, (hipStream_t)stream, x,  \
                         y, wx, x0, wy, y0, planes, H, W, OH, OW, cap_rows, xb, xl);                                                   \
    else                                                                                                                               \
      hipLaunchKernelGGL((crop_resize_aa_staged_kernel<K_, 8, 10>), dim3(kXcd, nbands, groups), dim3(kThreads), lds3, (hipStream_t)stream, x, \
                         y, wx, x0, wy, y0, planes, H, W, OH, OW, cap_rows, xb, xl);                                                   \
    break
      switch (K) {
        EQA_AA_STAGED(1); EQA_AA_STAGED(2); EQA_AA_STAGED(3); EQA_AA_STAGED(4); EQA_AA_STAGED(5); EQA_AA_STAGED(6); EQA_AA_STAGED(7);
        EQA_AA_STAGED(8);
        default: return EQA_ERR_UNSUPPORTED;
      }
#undef EQA_AA_STAGED
      return launch_status();
    }
  }
  hipLaunchKernelGGL(crop_resize_aa_kernel, grid, dim3(kThreads), lds, (hipStream_t)stream, x, y, wx, x0, wy, y0, H, W, OH, OW, K,
                     max_rows);
  return launch_status();
}

}  // extern "C"
