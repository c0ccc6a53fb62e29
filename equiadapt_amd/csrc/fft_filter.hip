// libeqa_hip.so, part 8b -- the filter side of the FFT convolution (fftconv.hip holds the transforms): filter banks -> spectra for the
// per-frequency channel contraction, and the filter gradient back out of the frequency domain.  Any odd kernel size 3 .. 9; the
// eqa_fft48k5_* entry points are the k = 5 plan with its own choices.  C ABI: include/eqa_hip.h.  Design notes: HISTORY.md section 3.4.
#include "eqa_common.hpp"

namespace {

#include "fft_common.inc"

// Filter spectra for the batched GEMM: bank (Cout, Cin, 5, 5) -> B (F, 2 Cin, 2 Cout), B[f] = [[Br, Bi], [-Bi, Br]] with
// Br + i Bi = conj(FFT48x48(filter))[ky][kx] / 48^2 = sum_{u,v} w[u][v] (cos t + i sin t) / 2304, t = 2 pi (ky u + kx v) / 48.
// Rows follow the rows of V ([Re x G | Im x G] per group of G input channels), columns the rows of Mo (interleaved complex).
// One thread per (ci, co) keeps its 25 taps in registers and walks the frequencies (fp64 accumulation, twiddles from a
// 48-entry table): 0.3 ms for 256 x 256 filters, against 13.6 ms for the same through torch.fft + concatenations -- cheap
// enough to run every training step.
// `sgn` = +1: the correlation form above (forward pass); -1: FFT(filter) itself, for the convolution of the input gradient.
// C16: the same thread, the same sums, another store -- the operand of cgemm3m_c16.hip, B3 (F, Cin/16, n_ct = ceil(Cout/32), 3 [Br | Bi |
// Br + Bi], 2 [b], 64 [lane = 32 h + j], 4 [t]) with input channel 16 s + 8 b + 4 h + t, output channel 32 c + j and the columns
// Cout .. 32 n_ct - 1 zero (G is then n_ct).  It is this kernel and not fft48_filter_spectra3m_kernel below so that Br, Bi are the
// floats of B bit for bit: the two kernels' fp64 sums are contracted into fused multiply-adds differently and differ by an ulp in a
// few entries per 10^7 (heavily cancelled ones).  Br + Bi: the correctly rounded sum of the two stored floats, as below.
template <int KS, bool C16 = false>
__global__ __launch_bounds__(kThreads) void fft48_filter_spectra_kernel(const float* __restrict__ bank, float* __restrict__ B, int Cout,
                                                                       int Cin, int G, float sgn) {
  __shared__ double tw_c[kFftN], tw_s[kFftN];
  if (threadIdx.x < kFftN) {
    const double t = 6.283185307179586476925286766559 * threadIdx.x / kFftN;
    tw_c[threadIdx.x] = cos(t);
    tw_s[threadIdx.x] = sin(t);
  }
  __syncthreads();
  const int co = blockIdx.y * kThreads + threadIdx.x;
  const int ci = blockIdx.x;
  // C16: element (part 0, this ci, this co) of frequency 0; parts are 512 floats apart, frequencies f3
  const size_t f3 = C16 ? (size_t)Cin * 32 * G * 3 : 0;
  float* o3 = C16 ? B + ((((size_t)(ci / 16) * G + co / 32) * 3 * 2 + (ci % 16) / 8) * 64 + 32 * ((ci % 8) / 4) + co % 32) * 4 + ci % 4 : nullptr;
  if (C16 && co >= Cout) {
    if (co < 32 * G)
      for (int f = 0; f < kFftF; ++f) o3[f * f3] = o3[f * f3 + 512] = o3[f * f3 + 1024] = 0.f;
    return;
  }
  if (co >= Cout) return;
  double w[KS * KS];
#pragma unroll
  for (int i = 0; i < KS * KS; ++i) w[i] = bank[((size_t)co * Cin + ci) * (KS * KS) + i];
  const int r0 = C16 ? 0 : (ci / G) * 2 * G + ci % G, r1 = r0 + G;
  const size_t fstride = (size_t)2 * Cin * 2 * Cout;
  float2* o0 = reinterpret_cast<float2*>(B + (size_t)r0 * 2 * Cout) + co;
  float2* o1 = reinterpret_cast<float2*>(B + (size_t)r1 * 2 * Cout) + co;
  constexpr double inv = 1.0 / (kFftN * kFftN);
  // separable: S_u(kx) = sum_v w[u][v] e^{i t kx v} once per kx, then sum_u e^{i t ky u} S_u for the 48 ky
  // (25 x (50 + 48 x 20) multiply-adds per filter instead of 1200 x 50 in the direct form, and a fifth of the table look-ups)
  for (int kx = 0; kx < kFftH; ++kx) {
    double sr[KS], si[KS];
#pragma unroll
    for (int u = 0; u < KS; ++u) {
      sr[u] = 0.0;
      si[u] = 0.0;
#pragma unroll
      for (int v = 0; v < KS; ++v) {
        const int t = (kx * v) % kFftN;
        sr[u] += w[u * KS + v] * tw_c[t];
        si[u] += w[u * KS + v] * tw_s[t];
      }
    }
    const int nky = fft_nky(kx), f0 = fft_f0(kx), fstep = fft_fstep(kx);
    for (int ky = 0; ky < nky; ++ky) {
      double br = 0.0, bi = 0.0;
#pragma unroll
      for (int u = 0; u < KS; ++u) {
        const int t = (ky * u) % kFftN;
        const double c = tw_c[t], sn = tw_s[t];
        br += c * sr[u] - sn * si[u];
        bi += c * si[u] + sn * sr[u];
      }
      const float fr = (float)(br * inv), fi = sgn * (float)(bi * inv);
      if (C16) {
        float* of = o3 + (size_t)(f0 + ky * fstep) * f3;
        of[0] = fr;
        of[512] = fi;
        of[1024] = (float)((double)fr + (double)fi);
        continue;
      }
      const size_t f = (size_t)(f0 + ky * fstep) * (fstride / 2);  // in float2
      o0[f] = make_float2(fr, fi);
      o1[f] = make_float2(-fi, fr);
    }
  }
}

// The same filter spectra in the operand order of the hand-written 3-multiplication complex GEMM (cgemm3m.hip):
// B3 (F, S = Cin/16, Cout/32, 3 [Br | Bi | Br + Bi], 2 [b], 64 [lane = 32 h + j], 4 [t]) with k = 16 s + 8 b + 4 h + t the input
// channel and 32 c + j the output channel: a wave's B fragment of one MFMA k-block is one contiguous 1 KB run.  Thread = (output
// channel, 4 consecutive input channels = t) for one kx: three 16-byte stores per frequency, fully coalesced over the lanes.
// Br + Bi is the correctly rounded sum of the two STORED floats (fp64 add of the rounded values), so that
// Ci = (Ar + Ai)(Br + Bi) - Ar Br - Ai Bi cancels against exactly the Br, Bi the other two products see.
template <int KS>
__global__ __launch_bounds__(kThreads) void fft48_filter_spectra3m_kernel(const float* __restrict__ bank, float* __restrict__ B3, int Cout,
                                                                         int Cin, float sgn) {
  __shared__ double tw_c[kFftN], tw_s[kFftN];
  if (threadIdx.x < kFftN) {
    const double t = 6.283185307179586476925286766559 * threadIdx.x / kFftN;
    tw_c[threadIdx.x] = cos(t);
    tw_s[threadIdx.x] = sin(t);
  }
  __syncthreads();
  const int co = blockIdx.y * kThreads + threadIdx.x;
  const int cq = blockIdx.x;                      // quad of input channels 4 cq .. 4 cq + 3
  const int kx = blockIdx.z;
  if (co >= Cout) return;
  constexpr double inv = 1.0 / (kFftN * kFftN);
  // S_u(kx) = sum_v w[u][v] e^{i t kx v} for the 4 filters of this thread
  double sr[4][KS], si[4][KS];
#pragma unroll
  for (int c = 0; c < 4; ++c) {
    const float* w = bank + ((size_t)co * Cin + 4 * cq + c) * (KS * KS);
#pragma unroll
    for (int u = 0; u < KS; ++u) {
      sr[c][u] = 0.0;
      si[c][u] = 0.0;
#pragma unroll
      for (int v = 0; v < KS; ++v) {
        const int t = (kx * v) % kFftN;
        const double wv = w[u * KS + v];
        sr[c][u] += wv * tw_c[t];
        si[c][u] += wv * tw_s[t];
      }
    }
  }
  const int S = Cin / 16;
  const int k0 = 4 * cq, s = k0 / 16, b = (k0 % 16) / 8, h = (k0 % 8) / 4;
  const int c32 = co / 32, lane = 32 * h + (co % 32);
  const size_t per_f = (size_t)Cin * Cout * 3;
  float4* o = reinterpret_cast<float4*>(B3 + (((((size_t)s * (Cout / 32) + c32) * 3) * 2 + b) * 64 + lane) * 4);   // part 0
  const size_t part = (size_t)2 * 64;             // float4 between the parts
  (void)S;
  const int nky = fft_nky(kx), f0 = fft_f0(kx), fstep = fft_fstep(kx);
  for (int ky = 0; ky < nky; ++ky) {
    float fr[4], fi[4], fs[4];
#pragma unroll
    for (int c = 0; c < 4; ++c) {
      double br = 0.0, bi = 0.0;
#pragma unroll
      for (int u = 0; u < KS; ++u) {
        const int t = (ky * u) % kFftN;
        const double cs = tw_c[t], sn = tw_s[t];
        br += cs * sr[c][u] - sn * si[c][u];
        bi += cs * si[c][u] + sn * sr[c][u];
      }
      fr[c] = (float)(br * inv);
      fi[c] = sgn * (float)(bi * inv);
      fs[c] = (float)((double)fr[c] + (double)fi[c]);
    }
    float4* of = o + (size_t)(f0 + ky * fstep) * (per_f / 4);
    of[0] = make_float4(fr[0], fr[1], fr[2], fr[3]);
    of[part] = make_float4(fi[0], fi[1], fi[2], fi[3]);
    of[2 * part] = make_float4(fs[0], fs[1], fs[2], fs[3]);
  }
}

// Filter gradient in the frequency domain (training).  With G = the spectra of the output-gradient tiles (44 x 44, zero-padded
// to 48: eqa_fft48k5_grad_transform) and V those of the input tiles, D[f] = V[f]^T . G[f] (real form, one batched GEMM over
// the tiles) holds  Dr = D[re ci][re co] + D[im ci][im co],  Di = D[im ci][re co] - D[re ci][im co]  of  X_f^T conj(G_f), and
//   dW[co][ci][u][v] = 1/48^2 sum_f wgt(f) (cos t Dr - sin t Di),  t = 2 pi (ky u + kx v) / 48,
// wgt = 2 for the stored frequencies whose conjugate partner is not stored, 1 for the self-conjugate ones -- the correlation theorem; no
// wrap-around because a 44-wide gradient tile shifted by up to 4 stays inside the 48-wide input tile.
// PACKED: D3 (F, Cin, 2, Cout) as eqa_fft48k5_wgrad3m writes it -- Dr | Di per input channel, plain channel order.
template <bool PACKED, int KS>
__global__ __launch_bounds__(kThreads) void fft48_filter_grad_kernel(const float* __restrict__ D, float* __restrict__ dbank, int Cout,
                                                                    int Cin, int Gin, int Gout) {
  __shared__ double tw_c[kFftN], tw_s[kFftN];
  if (threadIdx.x < kFftN) {
    const double t = 6.283185307179586476925286766559 * threadIdx.x / kFftN;
    tw_c[threadIdx.x] = cos(t);
    tw_s[threadIdx.x] = sin(t);
  }
  __syncthreads();
  const int co = blockIdx.y * kThreads + threadIdx.x;
  const int ci = blockIdx.x;
  if (co >= Cout) return;
  const int r0 = (ci / Gin) * 2 * Gin + ci % Gin, r1 = r0 + Gin;
  const int c0 = (co / Gout) * 2 * Gout + co % Gout, c1 = c0 + Gout;
  const size_t ld = (size_t)2 * Cout, fstride = (size_t)2 * Cin * (PACKED ? (size_t)Cout : ld);
  const size_t p_dr = ((size_t)2 * ci) * Cout + co, p_di = p_dr + Cout;   // PACKED
  double acc[KS * KS];
#pragma unroll
  for (int i = 0; i < KS * KS; ++i) acc[i] = 0.0;
  // separable, like the spectra kernel: A_u(kx) = sum_ky e^{i t ky u} D(ky, kx), then dW[u][v] += Re(e^{i t kx v} A_u(kx))
  for (int kx = 0; kx < kFftH; ++kx) {
    const bool edge = fft_edge(kx);
    const int nky = fft_nky(kx), f0 = fft_f0(kx), fstep = fft_fstep(kx);
    double ar[KS], ai[KS];
#pragma unroll
    for (int u = 0; u < KS; ++u) { ar[u] = 0.0; ai[u] = 0.0; }
    // one block per CU and one thread per filter: the loop is a chain of round trips unless several frequencies are requested
    // together (0.56 ms for 1.26 GB at one ky per trip).  Eight per trip; the sums run over ky in the same order.
    constexpr int kKyBatch = 8;
    for (int ky0 = 0; ky0 < nky; ky0 += kKyBatch) {
      float q[kKyBatch][PACKED ? 2 : 4];
#pragma unroll
      for (int b = 0; b < kKyBatch; ++b) {
        const float* d = D + (size_t)(f0 + min(ky0 + b, nky - 1) * fstep) * fstride;
        if (PACKED) {
          q[b][0] = d[p_dr];
          q[b][1] = d[p_di];
        } else {
          q[b][0] = d[r0 * ld + c0];
          q[b][1] = d[r1 * ld + c1];
          q[b][PACKED ? 0 : 2] = d[r1 * ld + c0];
          q[b][PACKED ? 1 : 3] = d[r0 * ld + c1];
        }
      }
#pragma unroll
      for (int b = 0; b < kKyBatch; ++b) {
        const int ky = ky0 + b;
        if (ky < nky) {
          // weight 2 for every stored frequency whose conjugate partner is not stored; 1 for the four self-conjugate ones
          const double wgt = (edge && (ky == 0 || ky == kFftH - 1)) ? 1.0 : 2.0;
          const double dr = PACKED ? wgt * (double)q[b][0] : wgt * ((double)q[b][0] + (double)q[b][1]);
          const double di = PACKED ? wgt * (double)q[b][1] : wgt * ((double)q[b][PACKED ? 0 : 2] - (double)q[b][PACKED ? 1 : 3]);
#pragma unroll
          for (int u = 0; u < KS; ++u) {
            const int t = (ky * u) % kFftN;
            const double c = tw_c[t], sn = tw_s[t];
            ar[u] += c * dr - sn * di;
            ai[u] += c * di + sn * dr;
          }
        }
      }
    }
#pragma unroll
    for (int u = 0; u < KS; ++u)
#pragma unroll
      for (int v = 0; v < KS; ++v) {
        const int t = (kx * v) % kFftN;
        acc[u * KS + v] += tw_c[t] * ar[u] - tw_s[t] * ai[u];
      }
  }
  constexpr double inv = 1.0 / (kFftN * kFftN);
  float* o = dbank + ((size_t)co * Cin + ci) * (KS * KS);
#pragma unroll
  for (int i = 0; i < KS * KS; ++i) o[i] = (float)(acc[i] * inv);
}

// The same reduction with one thread per (ci, co, filter ROW u = blockIdx.z): KS x the blocks and 1 / KS of the accumulators.  With
// few channels the kernel above is a handful of blocks of long serial threads (64 x 64 channels at k = 9: 64 blocks, 81 fp64
// accumulators per thread, 0.52 ms -- 5 % of the reference tutorial's training step); the KS rows re-read D from L2.  Same sums
// in the same order per element, so both forms give identical filters.
template <bool PACKED, int KS>
__global__ __launch_bounds__(kThreads) void fft48_filter_grad_rows_kernel(const float* __restrict__ D, float* __restrict__ dbank, int Cout,
                                                                         int Cin, int Gin, int Gout) {
  __shared__ double tw_c[kFftN], tw_s[kFftN];
  if (threadIdx.x < kFftN) {
    const double t = 6.283185307179586476925286766559 * threadIdx.x / kFftN;
    tw_c[threadIdx.x] = cos(t);
    tw_s[threadIdx.x] = sin(t);
  }
  __syncthreads();
  const int co = blockIdx.y * kThreads + threadIdx.x;
  const int ci = blockIdx.x;
  const int u = blockIdx.z;
  if (co >= Cout) return;
  const int r0 = (ci / Gin) * 2 * Gin + ci % Gin, r1 = r0 + Gin;
  const int c0 = (co / Gout) * 2 * Gout + co % Gout, c1 = c0 + Gout;
  const size_t ld = (size_t)2 * Cout, fstride = (size_t)2 * Cin * (PACKED ? (size_t)Cout : ld);
  const size_t p_dr = ((size_t)2 * ci) * Cout + co, p_di = p_dr + Cout;
  double acc[KS];
#pragma unroll
  for (int v = 0; v < KS; ++v) acc[v] = 0.0;
  for (int kx = 0; kx < kFftH; ++kx) {
    const bool edge = fft_edge(kx);
    const int nky = fft_nky(kx), f0 = fft_f0(kx), fstep = fft_fstep(kx);
    double ar = 0.0, ai = 0.0;
    constexpr int kKyBatch = 8;
    for (int ky0 = 0; ky0 < nky; ky0 += kKyBatch) {
      float q[kKyBatch][PACKED ? 2 : 4];
#pragma unroll
      for (int b = 0; b < kKyBatch; ++b) {
        const float* d = D + (size_t)(f0 + min(ky0 + b, nky - 1) * fstep) * fstride;
        if (PACKED) {
          q[b][0] = d[p_dr];
          q[b][1] = d[p_di];
        } else {
          q[b][0] = d[r0 * ld + c0];
          q[b][1] = d[r1 * ld + c1];
          q[b][PACKED ? 0 : 2] = d[r1 * ld + c0];
          q[b][PACKED ? 1 : 3] = d[r0 * ld + c1];
        }
      }
#pragma unroll
      for (int b = 0; b < kKyBatch; ++b) {
        const int ky = ky0 + b;
        if (ky < nky) {
          const double wgt = (edge && (ky == 0 || ky == kFftH - 1)) ? 1.0 : 2.0;
          const double dr = PACKED ? wgt * (double)q[b][0] : wgt * ((double)q[b][0] + (double)q[b][1]);
          const double di = PACKED ? wgt * (double)q[b][1] : wgt * ((double)q[b][PACKED ? 0 : 2] - (double)q[b][PACKED ? 1 : 3]);
          const int t = (ky * u) % kFftN;
          const double c = tw_c[t], sn = tw_s[t];
          ar += c * dr - sn * di;
          ai += c * di + sn * dr;
        }
      }
    }
#pragma unroll
    for (int v = 0; v < KS; ++v) {
      const int t = (kx * v) % kFftN;
      acc[v] += tw_c[t] * ar - tw_s[t] * ai;
    }
  }
  constexpr double inv = 1.0 / (kFftN * kFftN);
  float* o = dbank + ((size_t)co * Cin + ci) * (KS * KS) + u * KS;
#pragma unroll
  for (int v = 0; v < KS; ++v) o[v] = (float)(acc[v] * inv);
}

// The one place that launches a filter kernel.  KS = the filter size; what the two families of entry points decide differently is
// an argument, not a consequence of KS.
template <int KS>
struct FftFilterK {
  static dim3 grid(int Cout, int Cin, int z = 1) { return dim3(Cin, (Cout + kThreads - 1) / kThreads, z); }

  static int spectra(const float* bank, float* B, int Cout, int Cin, int correlate, hipStream_t st) {
    hipLaunchKernelGGL(fft48_filter_spectra_kernel<KS>, grid(Cout, Cin), dim3(kThreads), 0, st, bank, B, Cout, Cin, fft_group_in(Cin),
                       correlate ? 1.0f : -1.0f);
    return launch_status();
  }
  static int spectra3m_c16(const float* bank, float* B3, int Cout, int Cin, int correlate, hipStream_t st) {
    const int n_ct = (Cout + 31) / 32;
    hipLaunchKernelGGL((fft48_filter_spectra_kernel<KS, true>), grid(32 * n_ct, Cin), dim3(kThreads), 0, st, bank, B3, Cout, Cin, n_ct,
                       correlate ? 1.0f : -1.0f);
    return launch_status();
  }
  static int spectra3m(const float* bank, float* B3, int Cout, int Cin, int correlate, hipStream_t st) {
    hipLaunchKernelGGL(fft48_filter_spectra3m_kernel<KS>, grid(Cout, Cin / 4, kFftH), dim3(kThreads), 0, st, bank, B3, Cout, Cin,
                       correlate ? 1.0f : -1.0f);
    return launch_status();
  }
  // PACKED: D as eqa_fft48k5_wgrad3m writes it.  row_form: with fewer than ~2 blocks per CU in the one-thread-per-filter form, one
  // thread per filter ROW instead (the eqa_fft48k5_* entry points never ask for it).
  template <bool PACKED>
  static int filter_grad(const float* D, float* dbank, int Cout, int Cin, bool row_form, hipStream_t st) {
    const int gin = PACKED ? kFusCh : fft_group_in(Cin), gout = PACKED ? kFusCh : fft_group_in(Cout);
    if (row_form && (size_t)Cin * ((Cout + kThreads - 1) / kThreads) < 512)
      hipLaunchKernelGGL((fft48_filter_grad_rows_kernel<PACKED, KS>), grid(Cout, Cin, KS), dim3(kThreads), 0, st, D, dbank, Cout, Cin, gin, gout);
    else
      hipLaunchKernelGGL((fft48_filter_grad_kernel<PACKED, KS>), grid(Cout, Cin), dim3(kThreads), 0, st, D, dbank, Cout, Cin, gin, gout);
    return launch_status();
  }
};

// argument checks, shared by the two families (EQA_OK: go on)
int spectra_args(const float* bank, const float* B, int Cout, int Cin) {
  if (!bank || !B || Cout <= 0 || Cin <= 0) return EQA_ERR_INVALID_ARG;
  return (((uintptr_t)B & 7) || Cin > 65535) ? EQA_ERR_UNSUPPORTED : EQA_OK;
}
int spectra3m_args(const float* bank, const float* B3, int Cout, int Cin) {
  if (!bank || !B3 || Cout <= 0 || Cin <= 0) return EQA_ERR_INVALID_ARG;
  return (((uintptr_t)B3 & 15) || Cin % 32 || Cout % 64 || Cin / 4 > 65535) ? EQA_ERR_UNSUPPORTED : EQA_OK;
}
int spectra3m_c16_args(const float* bank, const float* B3, int Cout, int Cin) {
  if (!bank || !B3 || Cout <= 0 || Cin <= 0) return EQA_ERR_INVALID_ARG;
  return (((uintptr_t)B3 & 15) || Cin % 16 || Cout % 16 || Cin > 65535) ? EQA_ERR_UNSUPPORTED : EQA_OK;
}
int filter_grad_args(const float* D, const float* dbank, int Cout, int Cin, bool packed) {
  if (!D || !dbank || Cout <= 0 || Cin <= 0) return EQA_ERR_INVALID_ARG;
  return (Cin > 65535 || (packed && (Cin % kFusCh || Cout % kFusCh))) ? EQA_ERR_UNSUPPORTED : EQA_OK;
}

}  // namespace

extern "C" {

int eqa_fft48k5_group(int C, int side) {
  if (C <= 0 || (side != 0 && side != 1)) return EQA_ERR_INVALID_ARG;
  return side == 0 ? fft_group_in(C) : 1;
}

int eqa_fft48k5_filter_spectra(const float* bank, float* B, int Cout, int Cin, int correlate, void* stream) {
  if (const int rc = spectra_args(bank, B, Cout, Cin)) return rc;
  return FftFilterK<5>::spectra(bank, B, Cout, Cin, correlate, (hipStream_t)stream);
}

int eqa_fft48k5_filter_spectra3m(const float* bank, float* B3, int Cout, int Cin, int correlate, void* stream) {
  if (const int rc = spectra3m_args(bank, B3, Cout, Cin)) return rc;
  return FftFilterK<5>::spectra3m(bank, B3, Cout, Cin, correlate, (hipStream_t)stream);
}

int eqa_fft48k5_filter_spectra3m_c16(const float* bank, float* B3, int Cout, int Cin, int correlate, void* stream) {
  if (const int rc = spectra3m_c16_args(bank, B3, Cout, Cin)) return rc;
  return FftFilterK<5>::spectra3m_c16(bank, B3, Cout, Cin, correlate, (hipStream_t)stream);
}

int eqa_fft48k5_filter_grad(const float* D, float* dbank, int Cout, int Cin, void* stream) {
  if (const int rc = filter_grad_args(D, dbank, Cout, Cin, false)) return rc;
  return FftFilterK<5>::filter_grad<false>(D, dbank, Cout, Cin, /*row_form=*/false, (hipStream_t)stream);
}

int eqa_fft48k5_filter_grad3m(const float* D, float* dbank, int Cout, int Cin, void* stream) {
  if (const int rc = filter_grad_args(D, dbank, Cout, Cin, true)) return rc;
  return FftFilterK<5>::filter_grad<true>(D, dbank, Cout, Cin, /*row_form=*/false, (hipStream_t)stream);
}

int eqa_fft48_filter_spectra(const float* bank, float* B, int Cout, int Cin, int ksize, int correlate, void* stream) {
  if (const int rc = spectra_args(bank, B, Cout, Cin)) return rc;
  EQA_FFT_K(ksize, FftFilterK, K_::spectra(bank, B, Cout, Cin, correlate, (hipStream_t)stream));
}

int eqa_fft48_filter_spectra3m(const float* bank, float* B3, int Cout, int Cin, int ksize, int correlate, void* stream) {
  if (const int rc = spectra3m_args(bank, B3, Cout, Cin)) return rc;
  EQA_FFT_K(ksize, FftFilterK, K_::spectra3m(bank, B3, Cout, Cin, correlate, (hipStream_t)stream));
}

int eqa_fft48_filter_spectra3m_c16(const float* bank, float* B3, int Cout, int Cin, int ksize, int correlate, void* stream) {
  if (const int rc = spectra3m_c16_args(bank, B3, Cout, Cin)) return rc;
  EQA_FFT_K(ksize, FftFilterK, K_::spectra3m_c16(bank, B3, Cout, Cin, correlate, (hipStream_t)stream));
}

int eqa_fft48_filter_grad(const float* D, float* dbank, int Cout, int Cin, int ksize, int packed, void* stream) {
  if (const int rc = filter_grad_args(D, dbank, Cout, Cin, packed != 0)) return rc;
  EQA_FFT_K(ksize, FftFilterK, packed ? K_::template filter_grad<true>(D, dbank, Cout, Cin, /*row_form=*/true, (hipStream_t)stream)
                                      : K_::template filter_grad<false>(D, dbank, Cout, Cin, /*row_form=*/true, (hipStream_t)stream));
}

}  // extern "C"
