// libeqa_hip.so, part 7 -- training passes of VNSmall's first block (P1 + the conv_pos half of P2): kNN graph -> cross edge
// features -> VNLinearLeakyReLU(3 -> 21, slope 0) with TRAINING-mode VN batch-norm -> mean over the k neighbours
// (reference: pointcloud/canonicalization_networks/equivariant_networks.py:15-76, :128-140; vector_neuron_layers.py:251-273,
// :303-324).  Op by op the block materialises ~150 element-wise passes over (B, 21, 3, N, k) tensors (330 MB each at B = 64):
// 14 of the 15.9 ms of a training step.  Here nothing of that size exists: every pass re-derives the edge features from the
// 12 KB cloud in LDS and the (B, N, k) neighbour indices, one thread per point:
//   eqa_vn_knn                 neighbour indices (the queued insertion of the fused eval kernel)
//   eqa_vn_convpos_stats       per-channel sums of n and n^2, n = |W_f f| + EPS, over all edges  -> batch statistics
//   eqa_vn_convpos_fwd         q = W_f f; q <- q / n * (n * scale + shift); gate by d = W_d f; mean over k  -> (B, 21, 3, N)
//   eqa_vn_convpos_bwd_reduce  per-channel sums of g and g * nhat (g = dL/d BN output): d beta, d gamma, batch-norm terms
//   eqa_vn_convpos_bwd_apply   d W_f, d W_d (126 partial sums per block)
// pooling = "max" (VNMaxPool, vector_neuron_layers.py:327-364) instead of the mean: per (cloud, channel, point) the edge with the
// largest <h_c, (W_p h)_c> is gathered, h = the block's 21 output vectors of that edge.  Statistics, finalize: the passes above.
//   eqa_vn_convpos_max_fwd         the gathered vectors (B, 21, 3, N) and the winner's position in the point's neighbour list
//                                  sel (B, 21, N) uint8: first maximum in list order, as torch.max
//   eqa_vn_convpos_max_bwd_reduce  the mean pass's sums with the output gradient given whole to edge sel, nothing to the others
//   eqa_vn_convpos_max_bwd_apply   d W_f, d W_d likewise.  The edges that lost still move with the batch statistics (the -m1 - nhat m2
//                                  terms of the batch-norm backward), so this pass walks all k edges, with a zero output gradient
//                                  off the winner.  W_p only feeds the argmax: no gradient.
// No gradient w.r.t. the point coordinates (the cloud is data).  C ABI: include/eqa_hip.h.
#include "vn_common.hpp"

namespace {

// (the edge features VnEdge / vn_edge / vn_mix and conv_pos's output vector vn_convpos_h: vn_common.hpp, shared with the eval kernels)
// block-wide sum of NV per-thread values -> out[0..NV) (deterministic: shuffles, then a fixed-order sum over the waves)
template <int NV>
__device__ __forceinline__ void vn_block_sum(float (&v)[NV], float* s_red /* [waves][NV] */, float* __restrict__ out) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  __syncthreads();  // the scratch may still be read from a previous call
#pragma unroll
  for (int i = 0; i < NV; ++i) {
    const float s = wave_sum_f(v[i]);
    if (lane == 0) s_red[wave * NV + i] = s;
  }
  __syncthreads();
  for (int i = threadIdx.x; i < NV; i += kVnThreads) {
    float s = 0.f;
    for (int w = 0; w < kVnThreads / 64; ++w) s += s_red[w * NV + i];
    out[i] = s;
  }
}

// The same in two halves for sums formed inside a loop: every wave parks its NV sums at s_red[wave][at + i] (no barrier), and after
// the loop one barrier and a fixed-order sum over the waves writes all `total` values.
template <int NV>
__device__ __forceinline__ void vn_wave_part(const float (&v)[NV], float* s_red, int total, int at) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
#pragma unroll
  for (int i = 0; i < NV; ++i) {
    const float s = wave_sum_f(v[i]);
    if (lane == 0) s_red[wave * total + at + i] = s;
  }
}
__device__ __forceinline__ void vn_block_finish(const float* s_red, int total, float* __restrict__ out) {
  __syncthreads();
  for (int i = threadIdx.x; i < total; i += kVnThreads) {
    float s = 0.f;
    for (int w = 0; w < kVnThreads / 64; ++w) s += s_red[w * total + i];
    out[i] = s;
  }
}

// Four lanes per point (vn_common.hpp): the quad's distributed sorted list IS the neighbour list, lane `sub` stores the ranks
// [SEG sub, SEG sub + SEG) below k.  (One thread per point this was the largest kernel of a training step at B = 64: 157 us.)
template <int SEG>
__global__ __launch_bounds__(kVnQThreads, 4) void vn_knn_kernel(const float* __restrict__ x, int32_t* __restrict__ idx, int N, int k) {
  extern __shared__ __attribute__((aligned(16))) float vn_smem[];
  float4* pts = reinterpret_cast<float4*>(vn_smem);
  const int b = blockIdx.y, tid = threadIdx.x, sub = tid & 3;
  const int Npad = (N + 15) & ~15;
  vn_stage_cloud<kVnQThreads>(x + (size_t)b * 3 * N, N, Npad, pts, tid);
  __syncthreads();
  const int n = blockIdx.x * kVnQPts + (tid >> 2);
  const bool active = n < N;
  const float4 c4 = pts[active ? n : N - 1];
  float bv[SEG];
  int bi[SEG];
  vn_knn_quad<SEG>(pts, Npad, reinterpret_cast<float2*>(vn_smem + 4 * Npad), v3(c4.x, c4.y, c4.z), c4.w, tid, bv, bi);
  if (active) {
    int32_t* o = idx + ((size_t)b * N + n) * k;
#pragma unroll
    for (int t = 0; t < SEG; ++t)
      if (SEG * sub + t < k) o[SEG * sub + t] = bi[t];
  }
}

// Four lanes per point, five of its twenty edges each (kVnSplit x kVnEdges = kVnK): with one thread per point a batch of 64
// clouds is 65 k threads = one wave per SIMD walking 20 edges x 21 channels of dependent arithmetic (the four passes took
// 0.05 + 0.13 + 0.15 + 0.19 ms); split, there are four waves per SIMD and a quarter of the chain each.  Sums over a point's
// edges: the block sums already cover all lanes; the forward pass adds the four lanes of a quad with two DPP quad permutes.
// Any k <= 32: lane `sub` takes the edges [E sub, min(E sub + E, k)), E = ceil(k / 4); the kernels are instantiated for E <= 5
// (k <= 20; k = 20 is E = 5 exactly, every lane busy) and E <= 8 (k <= 32).
constexpr int kVnSplit = 4, kVnPts = kVnThreads / kVnSplit;

// common prologue of the four conv_pos passes: cloud in LDS, this thread's point and its share of the neighbour list
#define VN_PASS_PROLOGUE                                                                           \
  extern __shared__ __attribute__((aligned(16))) float vn_smem[];                                  \
  float4* pts = reinterpret_cast<float4*>(vn_smem);                                                \
  const int b = blockIdx.y, tid = threadIdx.x;                                                     \
  const int Npad = (N + 3) & ~3;                                                                   \
  vn_stage_cloud<kVnThreads>(x + (size_t)b * 3 * N, N, Npad, pts, tid);                            \
  __syncthreads();                                                                                 \
  const int n = blockIdx.x * kVnPts + tid / kVnSplit, sub = tid % kVnSplit;                        \
  const bool active = n < N;                                                                       \
  const float4 c4 = pts[active ? n : N - 1];                                                       \
  const V3 ctr = v3(c4.x, c4.y, c4.z);                                                             \
  const int edges = (k + kVnSplit - 1) / kVnSplit;                                                 \
  const int cnt = min(max(k - sub * edges, 0), edges);                                             \
  const int32_t* nbr = idx + ((size_t)b * N + (active ? n : N - 1)) * k + min(sub * edges, k - 1);

template <int EMAX>
__global__ __launch_bounds__(kVnThreads) void vn_convpos_stats_kernel(const float* __restrict__ x, const int32_t* __restrict__ idx,
                                                                     const float* __restrict__ Wf, float* __restrict__ partial,
                                                                     int N, int k) {
  __shared__ float s_red[(kVnThreads / 64) * 2 * kVnC];
  VN_PASS_PROLOGUE
  // channel-outer, edge-inner (as the fused eval kernel): the lane's edges are set up once, a channel's three weights are loaded
  // once for all of them, and the EMAX norm chains of a channel are independent
  VnEdge e[EMAX];
  float live[EMAX];
#pragma unroll
  for (int t = 0; t < EMAX; ++t) {
    e[t] = vn_edge(ctr, pts[nbr[t < cnt ? t : 0]]);
    live[t] = active && t < cnt ? 1.0f : 0.0f;
  }
  float acc[2 * kVnC];
#pragma unroll
  for (int c = 0; c < kVnC; ++c) {
    asm volatile("" ::: "memory");  // one channel at a time (see vnsmall_fwd.hip)
    float s0 = 0.f, s1 = 0.f;
#pragma unroll
    for (int t = 0; t < EMAX; ++t) {
      const V3 q = vn_mix(Wf + 3 * c, e[t]);
      const float nr = live[t] * (vn_sqrt(dot3(q, q)) + kVnEps);
      s0 += nr;
      s1 += nr * nr;
    }
    acc[2 * c] = s0;
    acc[2 * c + 1] = s1;
  }
  vn_block_sum<2 * kVnC>(acc, s_red, partial + ((size_t)b * gridDim.x + blockIdx.x) * (2 * kVnC));
}

template <int EMAX>
__global__ __launch_bounds__(kVnThreads) void vn_convpos_fwd_kernel(const float* __restrict__ x, const int32_t* __restrict__ idx,
                                                                   const float* __restrict__ Wf, const float* __restrict__ Wd,
                                                                   const float* __restrict__ scale, const float* __restrict__ shift,
                                                                   float* __restrict__ pooled, int N, int k) {
  VN_PASS_PROLOGUE
  VnEdge e[EMAX];
  float m[EMAX];
#pragma unroll
  for (int t = 0; t < EMAX; ++t) {
    e[t] = vn_edge(ctr, pts[nbr[t < cnt ? t : 0]]);
    m[t] = t < cnt ? 1.0f : 0.0f;   // (k = 20: every lane has its five edges and m == 1 throughout)
  }
  V3 acc[kVnC];
#pragma unroll
  for (int c = 0; c < kVnC; ++c) {
    asm volatile("" ::: "memory");  // one channel at a time
    const float sc = scale[c], sh = shift[c];
    V3 a = v3(0.f, 0.f, 0.f);
#pragma unroll
    for (int t = 0; t < EMAX; ++t) {
      const V3 q = vn_convpos_h(Wf + 3 * c, Wd + 3 * c, sc, sh, e[t]);
      a.x += m[t] * q.x; a.y += m[t] * q.y; a.z += m[t] * q.z;
    }
    acc[c] = a;
  }
  // the four lanes of a point: butterfly over the quad, every lane ends up with the point's sums; lane `sub` stores channels
  // c = sub, sub + 4, ...
  const float inv_k = 1.0f / (float)k;
  float* o = pooled + (size_t)b * kVnC * 3 * N + (active ? n : N - 1);  // (B, 21, 3, N)
#pragma unroll
  for (int c = 0; c < kVnC; ++c) {
    const float sx = vn_quad_sum(acc[c].x), sy = vn_quad_sum(acc[c].y), sz = vn_quad_sum(acc[c].z);
    if (active && (c % kVnSplit) == sub) {
      o[(size_t)(3 * c) * N] = sx * inv_k;
      o[(size_t)(3 * c + 1) * N] = sy * inv_k;
      o[(size_t)(3 * c + 2) * N] = sz * inv_k;
    }
  }
}

// The quad's best (score, list position) of one channel, to all four lanes: the larger score, on equal scores the lower position
// (the first maximum of the list, torch.max's).  A lane without a live edge holds (-inf, 255) and never wins.  This merge carries
// list positions and compares them; the fused eval kernel's (vnsmall_fwd.hip) has none and decides equal scores by lane parity
// ('>=' towards the lower lane, '>' towards the higher), so the two stay separate.
template <int CTRL>
__device__ __forceinline__ void vn_quad_better(float& s, int& p) {
  const float os = vn_dpp_f<CTRL>(s);
  const int op = vn_dpp_i<CTRL>(p);
  const bool take = os > s || (os == s && op < p);
  s = take ? os : s;
  p = take ? op : p;
}

// VNMaxPool over the point's k edges.  Edge-outer (one edge's 21 vectors h are all needed for its 21 scores), the channel loops
// unrolled.  Only the running best score and its position are kept per channel (42 registers beside the 63 of h); once the quad
// has agreed on the winners, lane `sub` evaluates the winning edge again for the channels c = sub, sub + 4, ... it stores: six
// (edge, channel) evaluations per lane after 21 x edges, instead of 63 more live registers and three selects per score.
// The edge loop is rolled (its trip count is ceil(k / 4) for the whole wave), so one kernel serves every k <= 32.
// hipcc -Rpass-analysis=kernel-resource-usage, gfx950: 126 VGPRs, 106 SGPRs, scratch 0 -> 4 waves per SIMD (512 registers per lane).
__global__ __launch_bounds__(kVnThreads) void vn_convpos_max_fwd_kernel(const float* __restrict__ x, const int32_t* __restrict__ idx,
                                                                       const float* __restrict__ Wf, const float* __restrict__ Wd,
                                                                       const float* __restrict__ scale, const float* __restrict__ shift,
                                                                       const float* __restrict__ Wp, float* __restrict__ pooled,
                                                                       uint8_t* __restrict__ sel, int N, int k) {
  VN_PASS_PROLOGUE
  float best[kVnC];
  int pos[kVnC];
#pragma unroll
  for (int c = 0; c < kVnC; ++c) {
    best[c] = -INFINITY;
    pos[c] = 255;
  }
#pragma unroll 1
  for (int t = 0; t < edges; ++t) {      // lane 0 of every quad owns `edges` positions: wave-uniform trip count
    asm volatile("" ::: "memory");       // keep the weights in the scalar cache, not hoisted into VGPRs (see vnsmall_fwd.hip)
    const bool live = active && t < cnt;
    const VnEdge e = vn_edge(ctr, pts[nbr[t < cnt ? t : 0]]);
    V3 h[kVnC];
#pragma unroll
    for (int c = 0; c < kVnC; ++c) h[c] = vn_convpos_h(Wf + 3 * c, Wd + 3 * c, scale[c], shift[c], e);
    const int p = sub * edges + t;
#pragma unroll
    for (int c = 0; c < kVnC; ++c) {
      if (c % 3 == 0) asm volatile("" ::: "memory");
      V3 d = v3(0.f, 0.f, 0.f);
#pragma unroll
      for (int a = 0; a < kVnC; ++a) {
        const float w = Wp[c * kVnC + a];
        d.x += w * h[a].x; d.y += w * h[a].y; d.z += w * h[a].z;
      }
      const float s = dot3(h[c], d);
      const bool take = live && s > best[c];   // strict: the first maximal edge (lowest position) wins, as torch.max does
      best[c] = take ? s : best[c];
      pos[c] = take ? p : pos[c];
    }
  }
#pragma unroll
  for (int c = 0; c < kVnC; ++c) {
    vn_quad_better<0xB1>(best[c], pos[c]);  // [1,0,3,2]
    vn_quad_better<0x4E>(best[c], pos[c]);  // [2,3,0,1]
  }
  const int32_t* row = idx + ((size_t)b * N + (active ? n : N - 1)) * k;
  float* o = pooled + (size_t)b * kVnC * 3 * N + (active ? n : N - 1);  // (B, 21, 3, N)
  uint8_t* os = sel + (size_t)b * kVnC * N + (active ? n : N - 1);      // (B, 21, N)
#pragma unroll
  for (int c0 = 0; c0 < kVnC; c0 += kVnSplit) {
    int p = pos[c0];
#pragma unroll
    for (int u = 1; u < kVnSplit; ++u)
      if (c0 + u < kVnC) p = sub == u ? pos[c0 + u] : p;
    p = min(p, k - 1);   // (255 is left only where no score compared greater than -inf: NaN input)
    const int c = min(c0 + sub, kVnC - 1);
    const V3 hv = vn_convpos_h(Wf + 3 * c, Wd + 3 * c, scale[c], shift[c], vn_edge(ctr, pts[row[p]]));
    if (active && c0 + sub < kVnC) {
      o[(size_t)(3 * c) * N] = hv.x;
      o[(size_t)(3 * c + 1) * N] = hv.y;
      o[(size_t)(3 * c + 2) * N] = hv.z;
      os[(size_t)c * N] = (uint8_t)p;
    }
  }
}

// One (edge, channel) of the block: mix the edge features, then the shared layer gradient (vn_common.hpp)
__device__ __forceinline__ VnGrad vn_edge_grad(const float* __restrict__ wf, const float* __restrict__ wd, const VnEdge& e,
                                               float scale, float shift, const V3& g_out) {
  return vn_gate_grad(vn_mix(wf, e), vn_mix(wd, e), scale, shift, g_out);
}

// The two backward passes serve both poolings (MAXPOOL: compile time).  mean: every edge of the point gets the channel's output
// gradient / k.  max: the edge at list position sel gets it whole, the others none.  `sel` is a kernel argument of the max
// instantiation only (the trailing pack), so the mean instantiation's argument block is what it was.
__device__ __forceinline__ const uint8_t* vn_sel_arg() { return nullptr; }
__device__ __forceinline__ const uint8_t* vn_sel_arg(const uint8_t* sel) { return sel; }

template <int EMAX, bool MAXPOOL = false, class... Sel>
__global__ __launch_bounds__(kVnThreads) void vn_convpos_bwd_reduce_kernel(const float* __restrict__ x, const int32_t* __restrict__ idx,
                                                                          const float* __restrict__ Wf, const float* __restrict__ Wd,
                                                                          const float* __restrict__ scale, const float* __restrict__ shift,
                                                                          const float* __restrict__ mean, const float* __restrict__ rstd,
                                                                          const float* __restrict__ gpool, float* __restrict__ partial,
                                                                          int N, int k, Sel... sel) {
  __shared__ float s_red[(kVnThreads / 64) * 2 * kVnC];   // per wave, all channels: ONE barrier after the channel loop, not two per channel
  VN_PASS_PROLOGUE
  // an edge's share of the channel's output gradient: 1 / k, or all of it for the winner; idle threads contribute nothing
  const float share = active ? (MAXPOOL ? 1.0f : 1.0f / (float)k) : 0.0f;
  const float* gp = gpool + (size_t)b * kVnC * 3 * N + (active ? n : N - 1);
  const uint8_t* sp = MAXPOOL ? vn_sel_arg(sel...) + (size_t)b * kVnC * N + (active ? n : N - 1) : nullptr;
  int nb[EMAX];
#pragma unroll
  for (int t = 0; t < EMAX; ++t) nb[t] = nbr[t < cnt ? t : 0];
  float* out = partial + ((size_t)b * gridDim.x + blockIdx.x) * (2 * kVnC);
  // channel by channel (the output gradient of a channel is the same for all k edges of the point): two accumulators live
#pragma unroll 1
  for (int c = 0; c < kVnC; ++c) {
    const V3 g_out = v3(gp[(size_t)(3 * c) * N] * share, gp[(size_t)(3 * c + 1) * N] * share, gp[(size_t)(3 * c + 2) * N] * share);
    const float sc = scale[c], sh = shift[c], mu = mean[c], rs = rstd[c];
    float acc[2] = {0.f, 0.f};
    if constexpr (MAXPOOL) {
      // the sums are over g_nbn, which is zero off the winner: one edge of the point, in the lane that owns its position
      const int t = (int)sp[(size_t)c * N] - sub * edges;
      if (t >= 0 && t < cnt) {
        const VnGrad r = vn_edge_grad(Wf + 3 * c, Wd + 3 * c, vn_edge(ctr, pts[nbr[t]]), sc, sh, g_out);
        acc[0] += r.g_nbn;
        acc[1] += r.g_nbn * (r.nr - mu) * rs;
      }
    } else {
#pragma unroll
    for (int t = 0; t < EMAX; ++t) {
      if (t < cnt) {   // (k = 20, EMAX = 5: always true)
        const VnGrad r = vn_edge_grad(Wf + 3 * c, Wd + 3 * c, vn_edge(ctr, pts[nb[t]]), sc, sh, g_out);
        acc[0] += r.g_nbn;
        acc[1] += r.g_nbn * (r.nr - mu) * rs;
      }
    }
    }
    vn_wave_part<2>(acc, s_red, 2 * kVnC, 2 * c);
  }
  vn_block_finish(s_red, 2 * kVnC, out);
}

// dW_f[c][i] = sum <g_q, f_i>, dW_d[c][i] = sum <g_d, f_i>;  g_q = dL/dq through the direction u = q/n and through the norm:
//   g_n = gamma rstd (g_nbn - m1 - nhat m2)   (m1 = sum g_nbn / M, m2 = sum g_nbn nhat / M; both 0 with running statistics)
//   g_q = (g_u - u <g_u, q> / |q|) / n + g_n q / |q|,   g_u = g_qn * nbn
// max pooling: g_nbn is zero off the winner but m1 and m2 are not, so with batch statistics every edge has a g_n: all k edges
// are walked, the losers with a zero output gradient.
template <int EMAX, bool MAXPOOL = false, class... Sel>
__global__ __launch_bounds__(kVnThreads) void vn_convpos_bwd_apply_kernel(const float* __restrict__ x, const int32_t* __restrict__ idx,
                                                                         const float* __restrict__ Wf, const float* __restrict__ Wd,
                                                                         const float* __restrict__ scale, const float* __restrict__ shift,
                                                                         const float* __restrict__ mean, const float* __restrict__ rstd,
                                                                         const float* __restrict__ m1, const float* __restrict__ m2,
                                                                         const float* __restrict__ gpool, float* __restrict__ partial,
                                                                         int N, int k, Sel... sel) {
  __shared__ float s_red[(kVnThreads / 64) * 6 * kVnC];
  VN_PASS_PROLOGUE
  const float share = active ? (MAXPOOL ? 1.0f : 1.0f / (float)k) : 0.0f;
  const float* gp = gpool + (size_t)b * kVnC * 3 * N + (active ? n : N - 1);
  const uint8_t* sp = MAXPOOL ? vn_sel_arg(sel...) + (size_t)b * kVnC * N + (active ? n : N - 1) : nullptr;
  int nb[EMAX];
#pragma unroll
  for (int t = 0; t < EMAX; ++t) nb[t] = nbr[t < cnt ? t : 0];
  float* out = partial + ((size_t)b * gridDim.x + blockIdx.x) * (6 * kVnC);  // [c][W_f 0..2, W_d 0..2]
#pragma unroll 1
  for (int c = 0; c < kVnC; ++c) {
    const V3 g_out = v3(gp[(size_t)(3 * c) * N] * share, gp[(size_t)(3 * c + 1) * N] * share, gp[(size_t)(3 * c + 2) * N] * share);
    const float sc = scale[c], sh = shift[c], mu = mean[c], rs = rstd[c], mm1 = m1[c], mm2 = m2[c];
    float acc[6] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
    const int won = MAXPOOL ? (int)sp[(size_t)c * N] - sub * edges : 0;   // the winner's slot in this lane's share, if it is here
#pragma unroll
    for (int t = 0; t < EMAX; ++t) {
      if (t < cnt) {
        const VnEdge e = vn_edge(ctr, pts[nb[t]]);
        const VnGrad r = vn_edge_grad(Wf + 3 * c, Wd + 3 * c, e, sc, sh, MAXPOOL && t != won ? v3(0.f, 0.f, 0.f) : g_out);
        const V3 g_q = vn_norm_input_grad(r, sc, mu, rs, mm1, mm2, active);
        acc[0] += dot3(g_q, e.f0);
        acc[1] += dot3(g_q, e.f1);
        acc[2] += dot3(g_q, e.f2);
        acc[3] += dot3(r.g_d, e.f0);
        acc[4] += dot3(r.g_d, e.f1);
        acc[5] += dot3(r.g_d, e.f2);
      }
    }
    vn_wave_part<6>(acc, s_red, 6 * kVnC, 6 * c);
  }
  vn_block_finish(s_red, 6 * kVnC, out);
}

inline int vn_check(const void* x, const void* idx, int B, int N, int k, size_t& lds, bool knn) {
  if (B < 0 || N <= 0 || k <= 0) return EQA_ERR_INVALID_ARG;
  if (N < k || k > 32) return EQA_ERR_UNSUPPORTED;
  lds = knn ? ((size_t)4 * ((N + 15) & ~15) + 2 * kVnQSlots * kVnQThreads) * sizeof(float) : (size_t)4 * ((N + 3) & ~3) * sizeof(float);
  // the kNN kernel raises its dynamic-LDS limit (eqa_vn_knn); the four passes hold only the cloud and stay inside the default 64 KB
  if (lds > (knn ? 128 : 64) * 1024 || B > 65535) return EQA_ERR_UNSUPPORTED;
  if (B == 0) return EQA_OK;
  if (!x || !idx) return EQA_ERR_INVALID_ARG;
  return 1;  // go
}

}  // namespace

extern "C" {

// blocks per cloud of the four conv_pos passes (32 points per block: four lanes per point); the kNN kernel keeps one thread per point
int eqa_vn_blocks(int N) { return N <= 0 ? 0 : (N + kVnPts - 1) / kVnPts; }
static int vn_knn_blocks(int N) { return (N + kVnQPts - 1) / kVnQPts; }

int eqa_vn_knn(const float* x, int32_t* idx, int B, int N, int k, void* stream) {
  size_t lds;
  const int rc = vn_check(x, idx, B, N, k, lds, true);
  if (rc != 1) return rc;
  const dim3 grid(vn_knn_blocks(N), B);
  if (lds > 64 * 1024 && !allow_dynamic_lds(k <= 20 ? (const void*)vn_knn_kernel<5> : (const void*)vn_knn_kernel<8>, 128 * 1024))
    return EQA_ERR_UNSUPPORTED;
  if (k <= 20)
    hipLaunchKernelGGL(vn_knn_kernel<5>, grid, dim3(kVnQThreads), lds, (hipStream_t)stream, x, idx, N, k);
  else
    hipLaunchKernelGGL(vn_knn_kernel<8>, grid, dim3(kVnQThreads), lds, (hipStream_t)stream, x, idx, N, k);
  return launch_status();
}

#define VN_LAUNCH_E(kernel, ...)                                                                                          \
  do {                                                                                                                    \
    if (k <= 20)                                                                                                          \
      hipLaunchKernelGGL(kernel<5>, dim3(eqa_vn_blocks(N), B), dim3(kVnThreads), lds, (hipStream_t)stream, __VA_ARGS__);  \
    else                                                                                                                  \
      hipLaunchKernelGGL(kernel<8>, dim3(eqa_vn_blocks(N), B), dim3(kVnThreads), lds, (hipStream_t)stream, __VA_ARGS__);  \
  } while (0)

int eqa_vn_convpos_stats(const float* x, const int32_t* idx, const float* Wf, float* partial, int B, int N, int k, void* stream) {
  size_t lds;
  const int rc = vn_check(x, idx, B, N, k, lds, false);
  if (rc != 1) return rc;
  if (!Wf || !partial) return EQA_ERR_INVALID_ARG;
  VN_LAUNCH_E(vn_convpos_stats_kernel, x, idx, Wf, partial, N, k);
  return launch_status();
}

int eqa_vn_convpos_fwd(const float* x, const int32_t* idx, const float* Wf, const float* Wd, const float* scale, const float* shift,
                       float* pooled, int B, int N, int k, void* stream) {
  size_t lds;
  const int rc = vn_check(x, idx, B, N, k, lds, false);
  if (rc != 1) return rc;
  if (!Wf || !Wd || !scale || !shift || !pooled) return EQA_ERR_INVALID_ARG;
  VN_LAUNCH_E(vn_convpos_fwd_kernel, x, idx, Wf, Wd, scale, shift, pooled, N, k);
  return launch_status();
}

int eqa_vn_convpos_bwd_reduce(const float* x, const int32_t* idx, const float* Wf, const float* Wd, const float* scale,
                              const float* shift, const float* mean, const float* rstd, const float* gpool, float* partial, int B,
                              int N, int k, void* stream) {
  size_t lds;
  const int rc = vn_check(x, idx, B, N, k, lds, false);
  if (rc != 1) return rc;
  if (!Wf || !Wd || !scale || !shift || !mean || !rstd || !gpool || !partial) return EQA_ERR_INVALID_ARG;
  VN_LAUNCH_E(vn_convpos_bwd_reduce_kernel, x, idx, Wf, Wd, scale, shift, mean, rstd, gpool, partial, N, k);
  return launch_status();
}

int eqa_vn_convpos_bwd_apply(const float* x, const int32_t* idx, const float* Wf, const float* Wd, const float* scale,
                             const float* shift, const float* mean, const float* rstd, const float* m1, const float* m2,
                             const float* gpool, float* partial, int B, int N, int k, void* stream) {
  size_t lds;
  const int rc = vn_check(x, idx, B, N, k, lds, false);
  if (rc != 1) return rc;
  if (!Wf || !Wd || !scale || !shift || !mean || !rstd || !m1 || !m2 || !gpool || !partial) return EQA_ERR_INVALID_ARG;
  VN_LAUNCH_E(vn_convpos_bwd_apply_kernel, x, idx, Wf, Wd, scale, shift, mean, rstd, m1, m2, gpool, partial, N, k);
  return launch_status();
}

// ---- pooling = "max"
#define VN_LAUNCH_E_MAX(kernel, ...)                                                                                     \
  do {                                                                                                                   \
    if (k <= 20)                                                                                                         \
      hipLaunchKernelGGL((kernel<5, true, const uint8_t*>), dim3(eqa_vn_blocks(N), B), dim3(kVnThreads), lds,            \
                         (hipStream_t)stream, __VA_ARGS__);                                                              \
    else                                                                                                                 \
      hipLaunchKernelGGL((kernel<8, true, const uint8_t*>), dim3(eqa_vn_blocks(N), B), dim3(kVnThreads), lds,            \
                         (hipStream_t)stream, __VA_ARGS__);                                                              \
  } while (0)

int eqa_vn_convpos_max_fwd(const float* x, const int32_t* idx, const float* Wf, const float* Wd, const float* scale,
                           const float* shift, const float* Wp, float* pooled, uint8_t* sel, int B, int N, int k, void* stream) {
  size_t lds;
  const int rc = vn_check(x, idx, B, N, k, lds, false);
  if (rc != 1) return rc;
  if (!Wf || !Wd || !scale || !shift || !Wp || !pooled || !sel) return EQA_ERR_INVALID_ARG;
  hipLaunchKernelGGL(vn_convpos_max_fwd_kernel, dim3(eqa_vn_blocks(N), B), dim3(kVnThreads), lds, (hipStream_t)stream, x, idx, Wf, Wd,
                     scale, shift, Wp, pooled, sel, N, k);
  return launch_status();
}

int eqa_vn_convpos_max_bwd_reduce(const float* x, const int32_t* idx, const float* Wf, const float* Wd, const float* scale,
                                  const float* shift, const float* mean, const float* rstd, const float* gpool,
                                  const uint8_t* sel, float* partial, int B, int N, int k, void* stream) {
  size_t lds;
  const int rc = vn_check(x, idx, B, N, k, lds, false);
  if (rc != 1) return rc;
  if (!Wf || !Wd || !scale || !shift || !mean || !rstd || !gpool || !sel || !partial) return EQA_ERR_INVALID_ARG;
  VN_LAUNCH_E_MAX(vn_convpos_bwd_reduce_kernel, x, idx, Wf, Wd, scale, shift, mean, rstd, gpool, partial, N, k, sel);
  return launch_status();
}

int eqa_vn_convpos_max_bwd_apply(const float* x, const int32_t* idx, const float* Wf, const float* Wd, const float* scale,
                                 const float* shift, const float* mean, const float* rstd, const float* m1, const float* m2,
                                 const float* gpool, const uint8_t* sel, float* partial, int B, int N, int k, void* stream) {
  size_t lds;
  const int rc = vn_check(x, idx, B, N, k, lds, false);
  if (rc != 1) return rc;
  if (!Wf || !Wd || !scale || !shift || !mean || !rstd || !m1 || !m2 || !gpool || !sel || !partial) return EQA_ERR_INVALID_ARG;
  VN_LAUNCH_E_MAX(vn_convpos_bwd_apply_kernel, x, idx, Wf, Wd, scale, shift, mean, rstd, m1, m2, gpool, partial, N, k, sel);
  return launch_status();
}

}  // extern "C"
