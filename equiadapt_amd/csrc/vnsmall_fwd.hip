// libeqa_hip.so, part 5b -- point clouds in eval mode: the fused kNN + VNSmall forward (P1, P2) with one thread or four lanes per
// point, and the one-launch tail of the canonicalizer behind it (network output -> Gram-Schmidt frame -> canonical cloud).
// Shared VN arithmetic and the packed parameter layout: vn_common.hpp.  C ABI: include/eqa_hip.h.  HISTORY.md section 3.3.
#include "vn_common.hpp"

namespace {

// P1 + P2: fused VNSmall forward (eval mode, mean pooling): kNN graph -> cross edge features -> VN linear / VN batch-norm
// / direction-gated ReLU (3->21) -> mean over neighbours -> (21->21) + VN batch-norm -> (21->4) -> mean over points.
// Reference: pointcloud/canonicalization_networks/equivariant_networks.py:15-76 (knn, get_graph_feature_cross),
// :128-150 (VNSmall.forward), vector_neuron_layers.py:251-273, :303-324.
// The reference materialises ten (B,21,3,N,k) tensors (5 MB per cloud each); here a cloud is 12 KB in LDS and every
// intermediate lives in registers: one thread = one point, its k nearest neighbours kept as a sorted register list
// while it streams over the cloud (LDS broadcast reads), then its k edges are pushed through the layers one by one.
// Packed parameter buffer: vn_prm (vn_common.hpp).
// MAXPOOL (VNMaxPool, vector_neuron_layers.py:349-364): per point and channel the edge with the largest <q_c, (W_p q)_c> is kept
// instead of the mean over the edges -- the first such edge, like torch.max; W_p mixes all 21 channels of an edge, so the edge's
// 21 vectors stay in registers until its 21 scores exist (two waves per SIMD instead of three).
template <bool MAXPOOL>
__global__ __launch_bounds__(kVnThreads, MAXPOOL ? 2 : EQA_VN_MIN_BLOCKS) void vnsmall_fwd_kernel(const float* __restrict__ x,
                                                                                                const float* __restrict__ prm,
                                                                                                float* __restrict__ partial, int N,
                                                                                                int nblk) {
  extern __shared__ __attribute__((aligned(16))) float vn_smem[];
  float4* pts = reinterpret_cast<float4*>(vn_smem);  // [Npad] (x, y, z, |p|^2): one ds_read_b128 per candidate
  __shared__ float s_part[kVnThreads / 64][12];
  const int b = blockIdx.y, tid = threadIdx.x;
  const int Npad = (N + 3) & ~3;
  vn_stage_cloud<kVnThreads>(x + (size_t)b * 3 * N, N, Npad, pts, tid);
  __syncthreads();
  const int n = blockIdx.x * kVnThreads + tid;
  const bool active = n < N;
  const float4 c4 = pts[active ? n : N - 1];
  const V3 ctr = v3(c4.x, c4.y, c4.z);
  int bi[kVnK];
  vn_knn(pts, Npad, reinterpret_cast<float2*>(vn_smem + 4 * Npad) + tid, ctr, c4.w, bi);

  // ---- conv_pos on the k edges + mean over neighbours
  V3 pooled[kVnC];
  float best[MAXPOOL ? kVnC : 1];
#pragma unroll
  for (int c = 0; c < kVnC; ++c) pooled[c] = v3(0.f, 0.f, 0.f);
#pragma unroll
  for (int c = 0; c < (MAXPOOL ? kVnC : 1); ++c) best[c] = 0.f;
  const float* Wf = prm + vn_prm::pos_wf;
  const float* Wd = prm + vn_prm::pos_wd;
  const float* bsc = prm + vn_prm::pos_scale;
  const float* bsh = prm + vn_prm::pos_shift;
#pragma unroll 1
  for (int t = 0; t < kVnK; ++t) {
    // compiler barrier: otherwise the 168 loop-invariant scalar weights are hoisted out of the loop and, for want of
    // SGPRs, parked in VGPRs for its whole duration (the kernel then needs > 256 VGPRs: one wave per SIMD)
    asm volatile("" ::: "memory");
    // (dynamic t: pick the t-th neighbour index through a select chain, the list lives in registers)
    int j = bi[0];
#pragma unroll
    for (int u = 1; u < kVnK; ++u) j = (t == u) ? bi[u] : j;
    const VnEdge e = vn_edge(ctr, pts[j]);
    V3 qe[MAXPOOL ? kVnC : 1];
#pragma unroll
    for (int c = 0; c < kVnC; ++c) {
      V3 q = vn_mix(Wf + c * 3, e);
      const V3 d = vn_mix(Wd + c * 3, e);
      q = vn_relu(vn_bn(q, bsc[c], bsh[c]), d);
      if (MAXPOOL) {
        qe[c] = q;
      } else {
        pooled[c].x += q.x; pooled[c].y += q.y; pooled[c].z += q.z;
      }
    }
    if (MAXPOOL) {
      const float* Wp = prm + vn_prm::pool_wd;
#pragma unroll
      for (int c = 0; c < kVnC; ++c) {
        if (c % 3 == 0) asm volatile("" ::: "memory");     // keeps the 441 scalar weights of W_p from being hoisted out of the edge loop
        V3 dp = v3(0.f, 0.f, 0.f);
#pragma unroll
        for (int a = 0; a < kVnC; ++a) {
          const float w = Wp[c * kVnC + a];
          dp.x += w * qe[a].x; dp.y += w * qe[a].y; dp.z += w * qe[a].z;
        }
        const float sc = qe[c].x * dp.x + qe[c].y * dp.y + qe[c].z * dp.z;
        const bool take = t == 0 || sc > best[c];          // strict: the first maximal edge wins, as torch.max does
        best[c] = take ? sc : best[c];
        pooled[c].x = take ? qe[c].x : pooled[c].x;
        pooled[c].y = take ? qe[c].y : pooled[c].y;
        pooled[c].z = take ? qe[c].z : pooled[c].z;
      }
    }
  }
  if (!MAXPOOL) {
    const float inv_k = 1.0f / (float)kVnK;
#pragma unroll
    for (int c = 0; c < kVnC; ++c) { pooled[c].x *= inv_k; pooled[c].y *= inv_k; pooled[c].z *= inv_k; }
  }

  // ---- conv1 (21->21) + its VN-BN + ReLU, then bn1; every output channel is folded into conv2's (21->4) two linear
  // maps as soon as it exists, so the 21 x 3 intermediate never has to be held in registers
  V3 q2[4], d2[4];
#pragma unroll
  for (int o = 0; o < 4; ++o) { q2[o] = v3(0.f, 0.f, 0.f); d2[o] = v3(0.f, 0.f, 0.f); }
  {
    const float* W1f = prm + vn_prm::c1_wf;
    const float* W1d = prm + vn_prm::c1_wd;
    const float* s1 = prm + vn_prm::c1_scale;
    const float* t1 = prm + vn_prm::c1_shift;
    const float* s2 = prm + vn_prm::bn1_scale;
    const float* t2 = prm + vn_prm::bn1_shift;
    const float* W2f = prm + vn_prm::c2_wf;
    const float* W2d = prm + vn_prm::c2_wd;
#pragma unroll 1  // rolled: fully unrolled (882 scalar weights in flight) the kernel needs > 256 VGPRs
    for (int c = 0; c < kVnC; ++c) {
      asm volatile("" ::: "memory");
      V3 q = v3(0.f, 0.f, 0.f), d = v3(0.f, 0.f, 0.f);
#pragma unroll
      for (int a = 0; a < kVnC; ++a) {
        const float wf = W1f[c * kVnC + a], wd = W1d[c * kVnC + a];
        q.x += wf * pooled[a].x; q.y += wf * pooled[a].y; q.z += wf * pooled[a].z;
        d.x += wd * pooled[a].x; d.y += wd * pooled[a].y; d.z += wd * pooled[a].z;
      }
      q = vn_relu(vn_bn(q, s1[c], t1[c]), d);
      const V3 hc = vn_bn(q, s2[c], t2[c]);
#pragma unroll
      for (int o = 0; o < 4; ++o) {
        const float wf = W2f[o * kVnC + c], wd = W2d[o * kVnC + c];
        q2[o].x += wf * hc.x; q2[o].y += wf * hc.y; q2[o].z += wf * hc.z;
        d2[o].x += wd * hc.x; d2[o].y += wd * hc.y; d2[o].z += wd * hc.z;
      }
    }
  }
  // ---- conv2's VN-BN + ReLU -> this point's contribution to the mean over points
  float outv[12];
  {
    const float* s3 = prm + vn_prm::c2_scale;
    const float* t3 = prm + vn_prm::c2_shift;
#pragma unroll
    for (int c = 0; c < 4; ++c) {
      const V3 q = vn_relu(vn_bn(q2[c], s3[c], t3[c]), d2[c]);
      outv[c * 3] = active ? q.x : 0.f;
      outv[c * 3 + 1] = active ? q.y : 0.f;
      outv[c * 3 + 2] = active ? q.z : 0.f;
    }
  }
#pragma unroll
  for (int c = 0; c < 12; ++c) {
    const float sres = wave_sum_f(outv[c]);
    if ((tid & 63) == 0) s_part[tid >> 6][c] = sres;
  }
  __syncthreads();
  if (tid < 12) {
    float acc = 0.f;
#pragma unroll
    for (int w = 0; w < kVnThreads / 64; ++w) acc += s_part[w][tid];
    partial[((size_t)b * nblk + blockIdx.x) * 12 + tid] = acc;
  }
}

// The same network with FOUR LANES PER POINT (vn_common.hpp, "quad" kernels) and any k <= 4 SEG: the quad scans the candidates
// together (distributed sorted list), each lane pushes its share of the point's edges (ranks SEG sub + t < k) through conv_pos,
// the pooled features are combined over the quad by DPP (sum, or first-maximum for VNMaxPool), conv1 / bn1 / conv2 are split
// over the quad by OUTPUT channel (lane `sub` takes c = sub, sub + 4, ...; those weights are lane-dependent, so they come from a
// re-packed copy in LDS: rows padded to 24 floats for ds_read_b128, rows 21..23 zero so that the idle sixth trip of lanes 1..3
// contributes exact zeros), and lane `sub` finishes output channel `sub`.  4 x the waves of the one-thread-per-point kernel at
// the same total instruction count: a batch of 64 clouds fills 4 waves per SIMD instead of one.
// LDS floats: [4 Npad] cloud | [2 * 12 * 256] queue | tail parameters:
//   W1f [24][24] | W1d [24][24] | (s1, t1, s2, t2) [24][4] | W2T [24][8] = (W2f[0..3][c], W2d[0..3][c]) | (s3, t3) [4][2]
constexpr int kVnTailLds = 2 * 24 * 24 + 24 * 4 + 24 * 8 + 8;   // 1448 floats

template <int SEG, bool MAXPOOL>
__global__ __launch_bounds__(kVnQThreads, MAXPOOL ? 2 : EQA_VN_QUAD_WAVES) void vnsmall_fwd_quad_kernel(const float* __restrict__ x,
                                                                                         const float* __restrict__ prm,
                                                                                         float* __restrict__ partial, int N, int k,
                                                                                         int nblk) {
  extern __shared__ __attribute__((aligned(16))) float vn_smem[];
  const int b = blockIdx.y, tid = threadIdx.x, sub = tid & 3;
  const int Npad = (N + 15) & ~15;
  float4* pts = reinterpret_cast<float4*>(vn_smem);
  float2* queue = reinterpret_cast<float2*>(vn_smem + 4 * Npad);
  float* tl = vn_smem + 4 * Npad + 2 * kVnQSlots * kVnQThreads;
  __shared__ float s_part[kVnQThreads / 64][12];
  vn_stage_cloud<kVnQThreads>(x + (size_t)b * 3 * N, N, Npad, pts, tid);
  // tail parameters, re-packed (see above)
  for (int i = tid; i < kVnTailLds; i += kVnQThreads) {
    float v = 0.f;
    if (i < 2 * 576) {                       // W1f | W1d rows
      const int m = i / 576, r = (i - m * 576) / 24, a = i % 24;
      if (r < kVnC && a < kVnC) v = prm[(m ? vn_prm::c1_wd : vn_prm::c1_wf) + r * kVnC + a];
    } else if (i < 2 * 576 + 96) {           // (s1, t1, s2, t2)[c]
      const int c = (i - 1152) >> 2, w = (i - 1152) & 3;
      if (c < kVnC) v = prm[(w == 0 ? vn_prm::c1_scale : w == 1 ? vn_prm::c1_shift : w == 2 ? vn_prm::bn1_scale : vn_prm::bn1_shift) + c];
    } else if (i < 2 * 576 + 96 + 192) {     // W2T[c][0..3] = W2f[o][c], [4..7] = W2d[o][c]
      const int c = (i - 1248) >> 3, w = (i - 1248) & 7;
      if (c < kVnC) v = prm[(w < 4 ? vn_prm::c2_wf : vn_prm::c2_wd) + (w & 3) * kVnC + c];
    } else {                                 // (s3, t3)[o]
      const int o = (i - 1440) >> 1, w = (i - 1440) & 1;
      v = prm[(w ? vn_prm::c2_shift : vn_prm::c2_scale) + o];
    }
    tl[i] = v;
  }
  __syncthreads();
  const int n = blockIdx.x * kVnQPts + (tid >> 2);
  const bool active = n < N;
  const float4 c4 = pts[active ? n : N - 1];
  const V3 ctr = v3(c4.x, c4.y, c4.z);
  float bv[SEG];
  int bi[SEG];
  vn_knn_quad<SEG>(pts, Npad, queue, ctr, c4.w, tid, bv, bi);

  // ---- conv_pos on this lane's edges (ranks SEG * sub + t < k)
  V3 pooled[kVnC];
  float best[MAXPOOL ? kVnC : 1];
#pragma unroll
  for (int c = 0; c < kVnC; ++c) pooled[c] = v3(0.f, 0.f, 0.f);
#pragma unroll
  for (int c = 0; c < (MAXPOOL ? kVnC : 1); ++c) best[c] = -INFINITY;
  const float* Wf = prm + vn_prm::pos_wf;
  const float* Wd = prm + vn_prm::pos_wd;
  const float* bsc = prm + vn_prm::pos_scale;
  const float* bsh = prm + vn_prm::pos_shift;
  if constexpr (!MAXPOOL) {
    // mean pooling: channel-outer, edge-inner.  The lane's SEG edges are set up once (6 registers each); a channel's 8 scalars are
    // then loaded once for all of them (edge-outer: once per edge, with a scalar-cache wait per channel), the SEG dependent
    // root / reciprocal chains of a channel are independent of each other, and only one accumulator triple is live at a time.
    VnEdge e[SEG];
    float m[SEG];
#pragma unroll
    for (int t = 0; t < SEG; ++t) {
      e[t] = vn_edge(ctr, pts[bi[t]]);
      m[t] = SEG * sub + t < k ? 1.0f : 0.0f;
    }
#pragma unroll
    for (int c = 0; c < kVnC; ++c) {
      asm volatile("" ::: "memory");   // one channel at a time: without it the scheduler interleaves all 21 and spills
      const float a0 = Wf[c * 3], a1 = Wf[c * 3 + 1], a2 = Wf[c * 3 + 2];
      const float d0 = Wd[c * 3], d1 = Wd[c * 3 + 1], d2 = Wd[c * 3 + 2];
      const float sc = bsc[c], sh = bsh[c];
      const V3 qc = v3(a1 * ctr.x, a1 * ctr.y, a1 * ctr.z), dc = v3(d1 * ctr.x, d1 * ctr.y, d1 * ctr.z);  // the centre's share: same for all edges
      V3 acc = v3(0.f, 0.f, 0.f);
#pragma unroll
      for (int t = 0; t < SEG; ++t) {
        V3 q = vn_mix_hoisted(a0, qc, a2, e[t]);
        const V3 d = vn_mix_hoisted(d0, dc, d2, e[t]);
        q = vn_relu_sel(vn_bn(q, sc, sh), d);
        acc.x += m[t] * q.x; acc.y += m[t] * q.y; acc.z += m[t] * q.z;
      }
      pooled[c] = acc;
    }
  } else {
#pragma unroll 1
    for (int t = 0; t < SEG; ++t) {
      if (!__any(SEG * sub + t < k)) break;   // wave-uniform
      asm volatile("" ::: "memory");          // keep the weights in the scalar cache, not hoisted into VGPRs (see above)
      int j = bi[0];
#pragma unroll
      for (int u = 1; u < SEG; ++u) j = (t == u) ? bi[u] : j;
      const bool valid = SEG * sub + t < k;
      const VnEdge e = vn_edge(ctr, pts[j]);
      V3 qe[kVnC];
#pragma unroll
      for (int c = 0; c < kVnC; ++c) {
        // all six weights are fetched before either mix, as this loop always has (the register allocation follows the load order)
        const float wf[3] = {Wf[c * 3], Wf[c * 3 + 1], Wf[c * 3 + 2]}, wd[3] = {Wd[c * 3], Wd[c * 3 + 1], Wd[c * 3 + 2]};
        const V3 q = vn_mix(wf, e), d = vn_mix(wd, e);
        qe[c] = vn_relu(vn_bn(q, bsc[c], bsh[c]), d);
      }
      const float* Wp = prm + vn_prm::pool_wd;
#pragma unroll
      for (int c = 0; c < kVnC; ++c) {
        if (c % 3 == 0) asm volatile("" ::: "memory");
        V3 dp = v3(0.f, 0.f, 0.f);
#pragma unroll
        for (int a = 0; a < kVnC; ++a) {
          const float w = Wp[c * kVnC + a];
          dp.x += w * qe[a].x; dp.y += w * qe[a].y; dp.z += w * qe[a].z;
        }
        const float sc = qe[c].x * dp.x + qe[c].y * dp.y + qe[c].z * dp.z;
        const bool take = valid && sc > best[c];   // strict: the first maximal edge (lowest rank) wins, as torch.max does
        best[c] = take ? sc : best[c];
        pooled[c].x = take ? qe[c].x : pooled[c].x;
        pooled[c].y = take ? qe[c].y : pooled[c].y;
        pooled[c].z = take ? qe[c].z : pooled[c].z;
      }
    }
  }
  // ---- the point's pooled features in all four lanes
  if (MAXPOOL) {
    // lane `sub` holds the ranks below lane sub + 1's: on equal scores the lower lane's pick stands.  No list positions are kept
    // here, so equal scores are decided by lane parity ('>=' when the partner is the lower lane, '>' when it is the higher); the
    // training pass (vn_quad_better, vnsmall_train.hip) carries positions and compares those instead, so the two merges stay separate.
#pragma unroll
    for (int c = 0; c < kVnC; ++c) {
      {
        const float os = vn_dpp_f<0xB1>(best[c]);
        const float ox = vn_dpp_f<0xB1>(pooled[c].x), oy = vn_dpp_f<0xB1>(pooled[c].y), oz = vn_dpp_f<0xB1>(pooled[c].z);
        const bool take = (sub & 1) ? (os >= best[c]) : (os > best[c]);
        best[c] = take ? os : best[c];
        pooled[c].x = take ? ox : pooled[c].x; pooled[c].y = take ? oy : pooled[c].y; pooled[c].z = take ? oz : pooled[c].z;
      }
      {
        const float os = vn_dpp_f<0x4E>(best[c]);
        const float ox = vn_dpp_f<0x4E>(pooled[c].x), oy = vn_dpp_f<0x4E>(pooled[c].y), oz = vn_dpp_f<0x4E>(pooled[c].z);
        const bool take = (sub & 2) ? (os >= best[c]) : (os > best[c]);
        pooled[c].x = take ? ox : pooled[c].x; pooled[c].y = take ? oy : pooled[c].y; pooled[c].z = take ? oz : pooled[c].z;
      }
    }
  } else {
    const float inv_k = 1.0f / (float)k;
#pragma unroll
    for (int c = 0; c < kVnC; ++c) {
      pooled[c].x = vn_quad_sum(pooled[c].x) * inv_k;
      pooled[c].y = vn_quad_sum(pooled[c].y) * inv_k;
      pooled[c].z = vn_quad_sum(pooled[c].z) * inv_k;
    }
  }

  // ---- conv1 + its VN-BN + ReLU + bn1 for the output channels c = sub, sub + 4, ..., folded into conv2's two maps
  V3 q2[4], d2[4];
#pragma unroll
  for (int o = 0; o < 4; ++o) { q2[o] = v3(0.f, 0.f, 0.f); d2[o] = v3(0.f, 0.f, 0.f); }
#pragma unroll 1
  for (int ci = 0; ci < 6; ++ci) {
    const int c = sub + 4 * ci;   // <= 23; rows 21..23 are zero
    const float4* rf = reinterpret_cast<const float4*>(tl + c * 24);
    const float4* rd = reinterpret_cast<const float4*>(tl + 576 + c * 24);
    V3 q = v3(0.f, 0.f, 0.f), d = v3(0.f, 0.f, 0.f);
#pragma unroll
    for (int a4 = 0; a4 < 6; ++a4) {
      const float4 wf = rf[a4], wd = rd[a4];
      const float wfa[4] = {wf.x, wf.y, wf.z, wf.w}, wda[4] = {wd.x, wd.y, wd.z, wd.w};
#pragma unroll
      for (int u = 0; u < 4; ++u) {
        const int a = a4 * 4 + u;
        if (a < kVnC) {
          q.x += wfa[u] * pooled[a].x; q.y += wfa[u] * pooled[a].y; q.z += wfa[u] * pooled[a].z;
          d.x += wda[u] * pooled[a].x; d.y += wda[u] * pooled[a].y; d.z += wda[u] * pooled[a].z;
        }
      }
    }
    const float4 st = *reinterpret_cast<const float4*>(tl + 1152 + c * 4);
    q = vn_relu(vn_bn(q, st.x, st.y), d);
    const V3 hc = vn_bn(q, st.z, st.w);
    const float4 w2f = *reinterpret_cast<const float4*>(tl + 1248 + c * 8), w2d = *reinterpret_cast<const float4*>(tl + 1248 + c * 8 + 4);
    const float wfo[4] = {w2f.x, w2f.y, w2f.z, w2f.w}, wdo[4] = {w2d.x, w2d.y, w2d.z, w2d.w};
#pragma unroll
    for (int o = 0; o < 4; ++o) {
      q2[o].x += wfo[o] * hc.x; q2[o].y += wfo[o] * hc.y; q2[o].z += wfo[o] * hc.z;
      d2[o].x += wdo[o] * hc.x; d2[o].y += wdo[o] * hc.y; d2[o].z += wdo[o] * hc.z;
    }
  }
  // ---- conv2's VN-BN + ReLU: lane `sub` finishes output channel `sub`
  V3 qs = v3(0.f, 0.f, 0.f), ds = v3(0.f, 0.f, 0.f);
#pragma unroll
  for (int o = 0; o < 4; ++o) {
    const float qx = vn_quad_sum(q2[o].x), qy = vn_quad_sum(q2[o].y), qz = vn_quad_sum(q2[o].z);
    const float dx = vn_quad_sum(d2[o].x), dy = vn_quad_sum(d2[o].y), dz = vn_quad_sum(d2[o].z);
    if (sub == o) { qs = v3(qx, qy, qz); ds = v3(dx, dy, dz); }
  }
  const V3 qo = vn_relu(vn_bn(qs, tl[1440 + 2 * sub], tl[1441 + 2 * sub]), ds);
#pragma unroll
  for (int o = 0; o < 4; ++o) {
    const bool mine = active && sub == o;
    const float sx = wave_sum_f(mine ? qo.x : 0.f), sy = wave_sum_f(mine ? qo.y : 0.f), sz = wave_sum_f(mine ? qo.z : 0.f);
    if ((tid & 63) == 0) { s_part[tid >> 6][o * 3] = sx; s_part[tid >> 6][o * 3 + 1] = sy; s_part[tid >> 6][o * 3 + 2] = sz; }
  }
  __syncthreads();
  if (tid < 12) {
    float acc = 0.f;
#pragma unroll
    for (int w = 0; w < kVnQThreads / 64; ++w) acc += s_part[w][tid];
    partial[((size_t)b * nblk + blockIdx.x) * 12 + tid] = acc;
  }
}

// (B, nblk, 12) partial sums -> (B,3,3): mean over the N points, first three of the four output channels
__global__ void vnsmall_finalize_kernel(const float* __restrict__ partial, float* __restrict__ out, int B, int nblk, float inv_n) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= B * 9) return;
  const int b = i / 9, c = i - b * 9;
  float acc = 0.f;
  for (int k = 0; k < nblk; ++k) acc += partial[((size_t)b * nblk + k) * 12 + c];
  out[i] = acc * inv_n;
}

// The whole tail of the eval-mode point-cloud canonicalizer in ONE launch per batch (one block per cloud): the partial sums of the
// fused VNSmall kernel -> the network's (3, 3) output vectors (vnsmall_finalize_kernel's sums) -> their Gram-Schmidt frame
// (gram_schmidt_kernel's arithmetic; equiadapt/common/utils.py:22-51) -> the canonical cloud y = R x (so3_rotate_kernel's;
// pointcloud/canonicalization/continuous_group.py:74-79).  As three launches behind the network kernel these cost three kernel
// boundaries of a 0.12 ms step (ModelNet40-shaped batches of 64 clouds).
__global__ __launch_bounds__(kThreads) void vnsmall_canon_tail_kernel(const float* __restrict__ partial, const float* __restrict__ x,
                                                                     float* __restrict__ vec, float* __restrict__ R,
                                                                     float* __restrict__ y, int N, int nblk, float inv_n) {
  __shared__ float s_v[9], s_r[9];
  const int b = blockIdx.x;
  if (threadIdx.x < 9) {
    float acc = 0.f;
    for (int k = 0; k < nblk; ++k) acc += partial[((size_t)b * nblk + k) * 12 + threadIdx.x];
    acc *= inv_n;
    s_v[threadIdx.x] = acc;
    vec[(size_t)b * 9 + threadIdx.x] = acc;
  }
  __syncthreads();
  if (threadIdx.x == 0) gram_schmidt_rows(s_v, s_r);
  __syncthreads();
  float m[9];
#pragma unroll
  for (int k = 0; k < 9; ++k) m[k] = s_r[k];
  if (threadIdx.x < 9) R[(size_t)b * 9 + threadIdx.x] = m[threadIdx.x];
  const float* xb = x + (size_t)b * 3 * N;
  float* yb = y + (size_t)b * 3 * N;
  if ((N & 3) == 0 && ((((uintptr_t)x | (uintptr_t)y) & 15) == 0)) {
    for (int k = threadIdx.x; k < (N >> 2); k += kThreads) {
      const float4 p0 = reinterpret_cast<const float4*>(xb)[k];
      const float4 p1 = reinterpret_cast<const float4*>(xb + N)[k];
      const float4 p2 = reinterpret_cast<const float4*>(xb + 2 * (size_t)N)[k];
#pragma unroll
      for (int r = 0; r < 3; ++r) {
        float4 o;
        o.x = m[r * 3] * p0.x + m[r * 3 + 1] * p1.x + m[r * 3 + 2] * p2.x;
        o.y = m[r * 3] * p0.y + m[r * 3 + 1] * p1.y + m[r * 3 + 2] * p2.y;
        o.z = m[r * 3] * p0.z + m[r * 3 + 1] * p1.z + m[r * 3 + 2] * p2.z;
        o.w = m[r * 3] * p0.w + m[r * 3 + 1] * p1.w + m[r * 3 + 2] * p2.w;
        reinterpret_cast<float4*>(yb + (size_t)r * N)[k] = o;
      }
    }
  } else {
    for (int k = threadIdx.x; k < N; k += kThreads) {
      const float p0 = xb[k], p1 = xb[N + k], p2 = xb[2 * (size_t)N + k];
#pragma unroll
      for (int r = 0; r < 3; ++r) yb[(size_t)r * N + k] = m[r * 3] * p0 + m[r * 3 + 1] * p1 + m[r * 3 + 2] * p2;
    }
  }
}

}  // namespace

// eqa_set_option key 1: 0 = choose the VNSmall forward kernel by size (default), 1 = always one thread per point (k = 20 only),
// 2 = always four lanes per point
int eqa::g_vn_kernel_choice = 0;
#ifndef EQA_VN_SINGLE_MIN_POINTS
#define EQA_VN_SINGLE_MIN_POINTS (1LL << 20)   // B * N from which the one-thread-per-point kernel is preferred for max pooling
#endif

extern "C" {

int64_t eqa_vnsmall_workspace_bytes(int B, int N) {
  if (B <= 0 || N <= 0) return 0;
  return (int64_t)B * ((N + kVnQPts - 1) / kVnQPts) * 12 * (int64_t)sizeof(float);   // the finer of the two block sizes
}

static int vnsmall_main(const float* x, const float* params, void* workspace, int B, int N, int k, int pooling, void* stream, int* nblk_out);

int eqa_vnsmall_fwd(const float* x, const float* params, float* out, void* workspace, int B, int N, int k, int pooling,
                    void* stream) {
  if (!out) return EQA_ERR_INVALID_ARG;
  int nblk = 0;
  const int rc = vnsmall_main(x, params, workspace, B, N, k, pooling, stream, &nblk);
  if (rc != EQA_OK || B == 0) return rc;
  hipLaunchKernelGGL(vnsmall_finalize_kernel, dim3((B * 9 + 255) / 256), dim3(256), 0, (hipStream_t)stream, (const float*)workspace, out, B,
                     nblk, 1.0f / (float)N);
  return launch_status();
}

int eqa_vnsmall_canonicalize(const float* x, const float* params, float* vectors, float* R, float* y, void* workspace, int B, int N, int k,
                             int pooling, void* stream) {
  if (B == 0 && N > 0) return EQA_OK;     // (empty tensors have null data pointers)
  if (!vectors || !R || !y) return EQA_ERR_INVALID_ARG;
  int nblk = 0;
  const int rc = vnsmall_main(x, params, workspace, B, N, k, pooling, stream, &nblk);
  if (rc != EQA_OK || B == 0) return rc;
  hipLaunchKernelGGL(vnsmall_canon_tail_kernel, dim3(B), dim3(kThreads), 0, (hipStream_t)stream, (const float*)workspace, x, vectors, R, y,
                     N, nblk, 1.0f / (float)N);
  return launch_status();
}

static int vnsmall_main(const float* x, const float* params, void* workspace, int B, int N, int k, int pooling, void* stream, int* nblk_out) {
  if (!x || !params || !workspace || B < 0 || N <= 0 || k <= 0) return EQA_ERR_INVALID_ARG;
  if (k > 32 || (pooling != 0 && pooling != 1) || N < k) return EQA_ERR_UNSUPPORTED;  // pooling 0 mean, 1 max
  if (B > 65535) return EQA_ERR_UNSUPPORTED;
  if (B == 0) return EQA_OK;
  hipStream_t st = (hipStream_t)stream;
  // one thread per point: fewer, longer instruction streams.  Mean pooling: the quad kernel is ahead at every batch size (B = 64:
  // 137 vs 250 us, B = 2048: 3.11 vs 3.21 ms); max pooling (two waves per SIMD either way): ahead only once the batch alone fills
  // the chip (B = 2048: 5.2 vs 6.0 ms; B = 256: 0.91 vs 0.84)
  // (its LDS -- 16 B per point + the 12 KB queue -- must fit the default 64 KB of a launch: clouds beyond 3,328 points always take
  // the quad kernel, whatever the batch; only the FORCED choice reports them as unsupported)
  const size_t lds_single = (size_t)4 * ((N + 3) & ~3) * sizeof(float) + (size_t)kVnThreads * kVnQueue * sizeof(float2);
  if (g_vn_kernel_choice == 1 && k == kVnK && lds_single > 64 * 1024) return EQA_ERR_UNSUPPORTED;
  const bool single = k == kVnK && lds_single <= 64 * 1024 &&
                      (g_vn_kernel_choice == 1 || (g_vn_kernel_choice == 0 && pooling == 1 && (long long)B * N >= EQA_VN_SINGLE_MIN_POINTS));
  int nblk;
  if (single) {
    const size_t lds = lds_single;
    nblk = (N + kVnThreads - 1) / kVnThreads;
    if (pooling == 1)
      hipLaunchKernelGGL(vnsmall_fwd_kernel<true>, dim3(nblk, B), dim3(kVnThreads), lds, st, x, params, (float*)workspace, N, nblk);
    else
      hipLaunchKernelGGL(vnsmall_fwd_kernel<false>, dim3(nblk, B), dim3(kVnThreads), lds, st, x, params, (float*)workspace, N, nblk);
  } else {
    const size_t lds = ((size_t)4 * ((N + 15) & ~15) + 2 * kVnQSlots * kVnQThreads + kVnTailLds) * sizeof(float);
    if (lds > 128 * 1024) return EQA_ERR_UNSUPPORTED;
    nblk = (N + kVnQPts - 1) / kVnQPts;
    const dim3 grid(nblk, B), blk(kVnQThreads);
    float* ws = (float*)workspace;
    // clouds beyond ~2,500 points need more dynamic LDS than the default 64 KB limit of a launch
#define EQA_VN_QUAD_LAUNCH(SEG_, MAX_)                                                                                              \
  do {                                                                                                                             \
    if (lds > 64 * 1024 && !allow_dynamic_lds((const void*)vnsmall_fwd_quad_kernel<SEG_, MAX_>, 128 * 1024))                       \
      return EQA_ERR_UNSUPPORTED;                                                                                                  \
    hipLaunchKernelGGL((vnsmall_fwd_quad_kernel<SEG_, MAX_>), grid, blk, lds, st, x, params, ws, N, k, nblk);                       \
  } while (0)
    if (k <= 20) {
      if (pooling == 1) EQA_VN_QUAD_LAUNCH(5, true); else EQA_VN_QUAD_LAUNCH(5, false);
    } else {
      if (pooling == 1) EQA_VN_QUAD_LAUNCH(8, true); else EQA_VN_QUAD_LAUNCH(8, false);
    }
#undef EQA_VN_QUAD_LAUNCH
  }
  if (hipGetLastError() != hipSuccess) return EQA_ERR_LAUNCH;
  *nblk_out = nblk;
  return EQA_OK;
}

}  // extern "C"
