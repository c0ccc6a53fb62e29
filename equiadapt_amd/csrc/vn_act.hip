// The directional nonlinearity of the vector-neuron layers, stand-alone: VNLeakyReLU and VNSoftplus of
// pointcloud/canonicalization_networks/vector_neuron_layers.py:93-207, forward and backward, one read of x and one write of y.
//
// x viewed as (B, C, 3, P) fp32, Wd:(D, C), D = C or 1 (share_nonlinearity).  Per point (b, p) and channel c, x_c is a 3-vector,
//   d_o = sum_i Wd[o, i] x_i   (o = c, or 0 for every channel when D = 1),   t = <x, d> / (|d|^2 + EPS),
//   y = slope x + (1 - slope) (mask x + (1 - mask) (x - t d))  =  x - f d,   f = (1 - slope) (1 - mask) t,
//   LeakyReLU: mask = [<x, d> >= 0];   Softplus: mask = cos^2(acos(c) / 2) = (1 + c) / 2,  c = <x, d> / (|x| |d| + EPS).
// The closed form of the softplus mask has no acos (nbody.hip uses the same form), so its gradient is finite where d is parallel to x
// (c = +-1); the reference's gradient through acos is not finite there (C = 1: d = w x is parallel to x at every point).
//
// Shape of the kernels.  A block of 512 threads takes tiles of 32 consecutive points q = b P + p (consecutive lanes, consecutive p:
// every global load and store is a run of 128 contiguous bytes per channel row) and walks the tiles with a grid stride.  A tile's
// 3 C rows are staged in LDS once (row pitch 33; the forward fetches the next tile's rows into registers before it works on the
// current one); Wd is staged once per block, transposed ([i][o], pitch a multiple of 8) so that
// the OB weights a thread needs for one input channel are one or two 16-byte broadcast reads.  Thread (group g = tid / 32, lane)
// owns the point `lane` and the OB channels [g OB, g OB + OB): 16 groups cover C <= 16 OB, OB = 2 / 4 / 8 by C, so a thread owns at
// most one channel block and the backward keeps the direct term of gx in registers across its barriers.
// Backward (d and the gate recomputed from x, nothing else saved):  with G = gy, A = -<G, d>,
//   df = alpha (d.dx + x.dd) + beta (d.dd) + gamma (x.dx)      (leaky, <x,d> < 0: alpha = k / q, beta = -2 k t / q, gamma = 0,
//        q = |d|^2 + EPS, k = 1 - slope -- the branch of vn_gate_grad; softplus: see gate_grad),
//   gx (direct) = G + A (alpha d + gamma x),   g_d = -f G + A (alpha x + beta d),   gx_i += sum_o Wd[o, i] g_d_o,
//   dL/dWd[o, i] = sum over points and axes of g_d_o x_i: summed per block in LDS by one fixed thread per entry in a fixed order,
//   written as partial:(blocks, D, C).  No atomics anywhere: two launches on the same input give the same bits.
// LDS at the limit C = 96: forward 73 KB, backward 150 KB of the CU's 160 KB.  IEEE division and sqrtf: the kernels are bound by
// memory and LDS traffic, and the accuracy margin of the tests is measured against the reference's own fp32 evaluation.
#include "vn_common.hpp"

namespace {

constexpr int kActThreads = 512, kActT = 32, kActTS = kActT + 1, kActGroups = kActThreads / kActT;
constexpr int kActMaxC = 96;          // 16 groups x OB = 8 would reach 128; the backward's LDS (2 x 3 C x 33 + 2 C^2 floats) stops at 96
constexpr int kActFwdBlocks = 2048;   // 256 CUs x 8
constexpr int kActBwdBlocks = 512;    // 2 per CU; partial is (blocks, D, C): 14.8 MB at C = 85, 0.9 MB at C = 21
constexpr int kActPartRows = 3 * (1 + kActGroups);   // D = 1: rows 0..2 the point's g_d, then one (3, T) partial per group

struct ActCfg {
  int C, D, CP, CR, softplus;  // CP: pitch of the transposed Wd rows, CR: channel rows held in LDS; both C (D) rounded up to 8
  float k;                     // 1 - slope
  long long P, Q;              // trailing size, points B * P
};

__host__ __device__ inline int round_up8(int v) { return (v + 7) & ~7; }

template <int OB>
__device__ __forceinline__ void load_w(const float* p, float (&w)[OB]) {
  if constexpr (OB == 2) {
    const float2 v = *reinterpret_cast<const float2*>(p);
    w[0] = v.x; w[1] = v.y;
  } else {
#pragma unroll
    for (int j = 0; j < OB; j += 4) {
      const float4 v = *reinterpret_cast<const float4*>(p + j);
      w[j] = v.x; w[j + 1] = v.y; w[j + 2] = v.z; w[j + 3] = v.w;
    }
  }
}

// Wd:(D, C) -> wt[i * CP + o], zero in the padding (rows up to CR, columns up to CP)
__device__ __forceinline__ void stage_w(const ActCfg& c, const float* __restrict__ Wd, float* wt, int tid) {
  for (int e = tid; e < c.CR * c.CP; e += kActThreads) {
    const int i = e / c.CP, o = e - i * c.CP;
    wt[e] = (i < c.C && o < c.D) ? Wd[(size_t)o * c.C + i] : 0.0f;
  }
}

struct Tile {
  size_t base;   // offset of x[b, 0, 0, p]
  bool valid;
};
__device__ __forceinline__ Tile make_tile(const ActCfg& c, long long tile, int lane) {
  const long long q = tile * kActT + lane;
  Tile t;
  t.valid = q < c.Q;
  const long long b = t.valid ? q / c.P : 0, p = t.valid ? q - b * c.P : 0;
  t.base = (size_t)b * c.C * 3 * (size_t)c.P + (size_t)p;
  return t;
}
// rows of src (row r at base + r P) -> dst[r * TS + lane], zero for the points past the end
__device__ __forceinline__ void stage_rows(const ActCfg& c, const Tile& t, const float* __restrict__ src, float* dst, int g, int lane) {
#pragma unroll 4
  for (int r = g; r < 3 * c.C; r += kActGroups) dst[r * kActTS + lane] = t.valid ? src[t.base + (size_t)r * (size_t)c.P] : 0.0f;
}
// the same in two halves, for the forward: the rows of the NEXT tile are fetched into registers (row g + 16 s in v[s]) before the
// current tile is worked on and go to LDS when it is done, so that a block has loads in flight while it computes
template <int NS>
__device__ __forceinline__ void fetch_rows(const ActCfg& c, const Tile& t, const float* __restrict__ src, int g, float (&v)[NS]) {
#pragma unroll
  for (int s = 0; s < NS; ++s) {
    const int r = g + s * kActGroups;
    v[s] = (t.valid && r < 3 * c.C) ? src[t.base + (size_t)r * (size_t)c.P] : 0.0f;
  }
}
template <int NS>
__device__ __forceinline__ void store_rows(const ActCfg& c, const float (&v)[NS], float* dst, int g, int lane) {
#pragma unroll
  for (int s = 0; s < NS; ++s) {
    const int r = g + s * kActGroups;
    if (r < 3 * c.C) dst[r * kActTS + lane] = v[s];
  }
}

// d of the thread's channels: d[j] = sum_i Wd[o0 + j, i] x_i, or d[0] = sum_i Wd[0, i] x_i when the direction is shared
template <int OB, bool SHARED>
__device__ __forceinline__ void directions(const ActCfg& c, const float* wt, const float* xs, int lane, int o0,
                                           V3 (&d)[SHARED ? 1 : OB]) {
  constexpr int ND = SHARED ? 1 : OB;
#pragma unroll
  for (int j = 0; j < ND; ++j) d[j] = v3(0.f, 0.f, 0.f);
#pragma unroll 2
  for (int i = 0; i < c.C; ++i) {
    const float* xr = xs + 3 * i * kActTS + lane;
    const float x0 = xr[0], x1 = xr[kActTS], x2 = xr[2 * kActTS];
    if constexpr (SHARED) {
      const float w = wt[i * c.CP];
      d[0].x = fmaf(w, x0, d[0].x); d[0].y = fmaf(w, x1, d[0].y); d[0].z = fmaf(w, x2, d[0].z);
    } else {
      float w[OB];
      load_w<OB>(wt + i * c.CP + o0, w);
#pragma unroll
      for (int j = 0; j < OB; ++j) {
        d[j].x = fmaf(w[j], x0, d[j].x); d[j].y = fmaf(w[j], x1, d[j].y); d[j].z = fmaf(w[j], x2, d[j].z);
      }
    }
  }
}

// f of y = x - f d
__device__ __forceinline__ float gate_factor(const ActCfg& c, const V3& x, const V3& d) {
  const float dot = dot3(x, d), q = dot3(d, d) + kVnEps;
  if (!c.softplus) return dot >= 0.0f ? 0.0f : c.k * (dot / q);
  const float cs = dot / (sqrtf(dot3(x, x)) * sqrtf(dot3(d, d)) + kVnEps);
  return c.k * 0.5f * (1.0f - cs) * (dot / q);
}

// f and the coefficients of df = alpha (d.dx + x.dd) + beta (d.dd) + gamma (x.dx)
struct GateGrad {
  float f, alpha, beta, gamma;
};
__device__ __forceinline__ GateGrad gate_grad(const ActCfg& c, const V3& x, const V3& d) {
  const float dot = dot3(x, d), dsq = dot3(d, d), q = dsq + kVnEps;
  const float t = dot / q;
  GateGrad r;
  if (!c.softplus) {
    const bool keep = dot >= 0.0f;
    r.f = keep ? 0.0f : c.k * t;
    r.alpha = keep ? 0.0f : c.k / q;
    r.beta = keep ? 0.0f : -2.0f * c.k * t / q;
    r.gamma = 0.0f;
  } else {
    // f = (k / 2) (1 - c) t,  c = dot / r,  r = |x| |d| + EPS:  df = (k / 2) ((1 - c) dt - t dc),
    //   dt = (d.dx + x.dd) / q - 2 t (d.dd) / q,   dc = (d.dx + x.dd) / r - (dot / r^2) (|d| / |x| (x.dx) + |x| / |d| (d.dd))
    const float nx = sqrtf(dot3(x, x)), nd = sqrtf(dsq), rr = nx * nd + kVnEps;
    const float cs = dot / rr, h = 0.5f * c.k, u = t * dot / (rr * rr);
    const float inv_nx = nx > 0.0f ? 1.0f / nx : 0.0f, inv_nd = nd > 0.0f ? 1.0f / nd : 0.0f;
    r.f = h * (1.0f - cs) * t;
    r.alpha = h * ((1.0f - cs) / q - t / rr);
    r.beta = h * (-2.0f * (1.0f - cs) * t / q + u * nx * inv_nd);
    r.gamma = h * u * nd * inv_nx;
  }
  return r;
}

template <int OB, bool SHARED>
__global__ __launch_bounds__(kActThreads) void vn_act_fwd_kernel(ActCfg c, const float* __restrict__ x, const float* __restrict__ Wd,
                                                                 float* __restrict__ y) {
  extern __shared__ __align__(16) float smem[];
  float* wt = smem;
  float* xs = wt + c.CR * c.CP;
  const int tid = threadIdx.x, lane = tid % kActT, g = tid / kActT, o0 = g * OB;
  constexpr int NS = OB == 8 ? (3 * kActMaxC + kActGroups - 1) / kActGroups : 3 * OB;   // rows per thread: 3 C <= 16 NS
  stage_w(c, Wd, wt, tid);
  const long long tiles = (c.Q + kActT - 1) / kActT;
  Tile next = make_tile(c, blockIdx.x, lane);
  float pre[NS];
  fetch_rows<NS>(c, next, x, g, pre);
  for (long long tile = blockIdx.x; tile < tiles; tile += gridDim.x) {
    const Tile t = next;
    __syncthreads();   // the previous tile is read out (first trip: Wd is staged)
    store_rows<NS>(c, pre, xs, g, lane);
    __syncthreads();
    if (tile + gridDim.x < tiles) {
      next = make_tile(c, tile + gridDim.x, lane);
      fetch_rows<NS>(c, next, x, g, pre);
    }
    if (o0 < c.C) {
      V3 d[SHARED ? 1 : OB];
      directions<OB, SHARED>(c, wt, xs, lane, o0, d);
#pragma unroll
      for (int j = 0; j < OB; ++j) {
        const int o = o0 + j;
        if (o < c.C && t.valid) {
          const float* xr = xs + 3 * o * kActTS + lane;
          const V3 xv = v3(xr[0], xr[kActTS], xr[2 * kActTS]);
          const V3& dv = d[SHARED ? 0 : j];
          const float f = gate_factor(c, xv, dv);
          float* yo = y + t.base + (size_t)(3 * o) * (size_t)c.P;
          yo[0] = xv.x - f * dv.x;
          yo[(size_t)c.P] = xv.y - f * dv.y;
          yo[2 * (size_t)c.P] = xv.z - f * dv.z;
        }
      }
    }
  }
}

// PB: side of the (o, i) block of dL/dWd one thread sums per trip
template <int OB, bool SHARED, int PB>
__global__ __launch_bounds__(kActThreads) void vn_act_bwd_kernel(ActCfg c, const float* __restrict__ x, const float* __restrict__ Wd,
                                                                 const float* __restrict__ gy, float* __restrict__ gx,
                                                                 float* __restrict__ partial) {
  extern __shared__ __align__(16) float smem[];
  float* wt = smem;
  float* xs = wt + c.CR * c.CP;
  float* gds = xs + 3 * c.CR * kActTS;                                  // g_d rows, (3 D) used; D = 1: kActPartRows rows
  float* gw = gds + (SHARED ? kActPartRows : 3 * c.CR) * kActTS;        // (D, C) sums of this block
  const int tid = threadIdx.x, lane = tid % kActT, g = tid / kActT, o0 = g * OB;
  stage_w(c, Wd, wt, tid);
  for (int e = tid; e < c.D * c.C; e += kActThreads) gw[e] = 0.0f;
  const long long tiles = (c.Q + kActT - 1) / kActT;
  const int nob = (c.D + PB - 1) / PB, nib = (c.C + PB - 1) / PB;
  for (long long tile = blockIdx.x; tile < tiles; tile += gridDim.x) {
    const Tile t = make_tile(c, tile, lane);
    __syncthreads();
    stage_rows(c, t, x, xs, g, lane);
    __syncthreads();
    // ---- A: gate gradients of the thread's channels; the direct term of gx stays in registers
    V3 direct[OB];
    V3 gsum = v3(0.f, 0.f, 0.f);
#pragma unroll
    for (int j = 0; j < OB; ++j) direct[j] = v3(0.f, 0.f, 0.f);
    if (o0 < c.C) {
      V3 d[SHARED ? 1 : OB];
      directions<OB, SHARED>(c, wt, xs, lane, o0, d);
#pragma unroll
      for (int j = 0; j < OB; ++j) {
        const int o = o0 + j;
        if (o < c.C) {
          const float* xr = xs + 3 * o * kActTS + lane;
          const V3 xv = v3(xr[0], xr[kActTS], xr[2 * kActTS]);
          const V3& dv = d[SHARED ? 0 : j];
          const float* go = gy + t.base + (size_t)(3 * o) * (size_t)c.P;
          const V3 G = t.valid ? v3(go[0], go[(size_t)c.P], go[2 * (size_t)c.P]) : v3(0.f, 0.f, 0.f);
          const GateGrad r = gate_grad(c, xv, dv);
          const float A = -dot3(G, dv);
          const float ad = A * r.alpha, ag = A * r.gamma, ab = A * r.beta;
          direct[j] = v3(G.x + ad * dv.x + ag * xv.x, G.y + ad * dv.y + ag * xv.y, G.z + ad * dv.z + ag * xv.z);
          V3 gd = v3(-r.f * G.x + ad * xv.x + ab * dv.x, -r.f * G.y + ad * xv.y + ab * dv.y, -r.f * G.z + ad * xv.z + ab * dv.z);
          if (!t.valid) gd = v3(0.f, 0.f, 0.f);
          if constexpr (SHARED) {
            gsum.x += gd.x; gsum.y += gd.y; gsum.z += gd.z;
          } else {
            float* gr = gds + 3 * o * kActTS + lane;
            gr[0] = gd.x; gr[kActTS] = gd.y; gr[2 * kActTS] = gd.z;
          }
        }
      }
    }
    if constexpr (SHARED) {
      float* pr = gds + (3 + 3 * g) * kActTS + lane;   // every group, idle ones with zeros
      pr[0] = gsum.x; pr[kActTS] = gsum.y; pr[2 * kActTS] = gsum.z;
      __syncthreads();
      if (tid < 3 * kActT) {                           // group g = axis: the groups' partial sums in the order of the groups
        float acc = 0.0f;
#pragma unroll
        for (int k = 0; k < kActGroups; ++k) acc += gds[(3 + 3 * k + g) * kActTS + lane];
        gds[g * kActTS + lane] = acc;
      }
    }
    __syncthreads();
    // ---- B: gx_i = direct_i + sum_o Wd[o, i] g_d_o for the same channels
    if (o0 < c.C) {
      if constexpr (SHARED) {
        const V3 gd = v3(gds[lane], gds[kActTS + lane], gds[2 * kActTS + lane]);
#pragma unroll
        for (int j = 0; j < OB; ++j) {
          const float w = wt[(o0 + j) * c.CP];
          direct[j].x = fmaf(w, gd.x, direct[j].x); direct[j].y = fmaf(w, gd.y, direct[j].y); direct[j].z = fmaf(w, gd.z, direct[j].z);
        }
      } else {
#pragma unroll 2
        for (int o = 0; o < c.C; ++o) {
          const float* gr = gds + 3 * o * kActTS + lane;
          const float g0 = gr[0], g1 = gr[kActTS], g2 = gr[2 * kActTS];
#pragma unroll
          for (int j = 0; j < OB; ++j) {
            const float w = wt[(o0 + j) * c.CP + o];
            direct[j].x = fmaf(w, g0, direct[j].x); direct[j].y = fmaf(w, g1, direct[j].y); direct[j].z = fmaf(w, g2, direct[j].z);
          }
        }
      }
#pragma unroll
      for (int j = 0; j < OB; ++j) {
        const int i = o0 + j;
        if (i < c.C && t.valid) {
          float* xo = gx + t.base + (size_t)(3 * i) * (size_t)c.P;
          xo[0] = direct[j].x;
          xo[(size_t)c.P] = direct[j].y;
          xo[2 * (size_t)c.P] = direct[j].z;
        }
      }
    }
    // ---- C: gw[o, i] += sum over the tile's points and axes of g_d_o x_i; entry (o, i) always by the same thread.  The walk over
    // the points starts at a column that depends on the i block, so that the lanes of a wave read different LDS banks.
    // Rows past 3 D of gds / 3 C of xs are read only into sums that are not stored.
    for (int e = tid; e < nob * nib; e += kActThreads) {
      const int ob = e / nib, ib = e - ob * nib;
      float acc[PB][PB];
#pragma unroll
      for (int jo = 0; jo < PB; ++jo)
#pragma unroll
        for (int ji = 0; ji < PB; ++ji) acc[jo][ji] = 0.0f;
      const float* gr = gds + 3 * ob * PB * kActTS;
      const float* xr = xs + 3 * ib * PB * kActTS;
#pragma unroll 2
      for (int s = 0; s < kActT; ++s) {
        const int pt = (s + ib) & (kActT - 1);
#pragma unroll
        for (int a = 0; a < 3; ++a) {
          float gv[PB], xv[PB];
#pragma unroll
          for (int jj = 0; jj < PB; ++jj) {
            gv[jj] = gr[(3 * jj + a) * kActTS + pt];
            xv[jj] = xr[(3 * jj + a) * kActTS + pt];
          }
#pragma unroll
          for (int jo = 0; jo < PB; ++jo)
#pragma unroll
            for (int ji = 0; ji < PB; ++ji) acc[jo][ji] = fmaf(gv[jo], xv[ji], acc[jo][ji]);
        }
      }
#pragma unroll
      for (int jo = 0; jo < PB; ++jo)
#pragma unroll
        for (int ji = 0; ji < PB; ++ji) {
          const int o = ob * PB + jo, i = ib * PB + ji;
          if (o < c.D && i < c.C) gw[o * c.C + i] += acc[jo][ji];
        }
    }
  }
  __syncthreads();
  float* out = partial + (size_t)blockIdx.x * c.D * c.C;
  for (int e = tid; e < c.D * c.C; e += kActThreads) out[e] = gw[e];
}

int act_cfg(ActCfg& c, int B, int C, long long P, int D, int softplus, float slope) {
  if (B <= 0 || C <= 0 || P <= 0 || (D != 1 && D != C)) return EQA_ERR_INVALID_ARG;
  if (C > kActMaxC || P > (1LL << 40) || (long long)B * P > (1LL << 40)) return EQA_ERR_UNSUPPORTED;
  c.C = C; c.D = D; c.CP = round_up8(D); c.CR = round_up8(C); c.softplus = softplus ? 1 : 0;
  c.k = 1.0f - slope; c.P = P; c.Q = (long long)B * P;
  return EQA_OK;
}

template <int OB, bool SHARED>
int launch_fwd(const ActCfg& c, const float* x, const float* Wd, float* y, hipStream_t st) {
  const int lds = (c.CR * c.CP + 3 * c.CR * kActTS) * (int)sizeof(float);
  if (lds > 64 * 1024 && !allow_dynamic_lds((const void*)vn_act_fwd_kernel<OB, SHARED>, 160 * 1024)) return EQA_ERR_UNSUPPORTED;
  const long long tiles = (c.Q + kActT - 1) / kActT;
  const unsigned blocks = (unsigned)std::min<long long>(tiles, kActFwdBlocks);
  hipLaunchKernelGGL((vn_act_fwd_kernel<OB, SHARED>), dim3(blocks), dim3(kActThreads), lds, st, c, x, Wd, y);
  return launch_status();
}

template <int OB, bool SHARED, int PB>
int launch_bwd(const ActCfg& c, const float* x, const float* Wd, const float* gy, float* gx, float* partial, hipStream_t st) {
  const int lds = (c.CR * c.CP + 3 * c.CR * kActTS + (SHARED ? kActPartRows : 3 * c.CR) * kActTS + c.D * c.C) * (int)sizeof(float);
  if (lds > 64 * 1024 && !allow_dynamic_lds((const void*)vn_act_bwd_kernel<OB, SHARED, PB>, 160 * 1024)) return EQA_ERR_UNSUPPORTED;
  const unsigned blocks = (unsigned)eqa_vn_act_bwd_blocks(c.Q);
  hipLaunchKernelGGL((vn_act_bwd_kernel<OB, SHARED, PB>), dim3(blocks), dim3(kActThreads), lds, st, c, x, Wd, gy, gx, partial);
  return launch_status();
}

}  // namespace

int eqa_vn_act_max_channels(void) { return kActMaxC; }

int eqa_vn_act_bwd_blocks(long long points) {
  if (points <= 0) return EQA_ERR_INVALID_ARG;
  return (int)std::min<long long>((points + kActT - 1) / kActT, kActBwdBlocks);
}

int eqa_vn_act_fwd(const float* x, const float* Wd, float* y, int B, int C, long long P, int D, int softplus, float slope,
                   void* stream) {
  if (!x || !Wd || !y) return EQA_ERR_INVALID_ARG;
  ActCfg c;
  const int st = act_cfg(c, B, C, P, D, softplus, slope);
  if (st != EQA_OK) return st;
  hipStream_t s = (hipStream_t)stream;
  const bool shared = D == 1 && C > 1;      // C = 1: both forms are the same map
  if (C <= 2 * kActGroups) return shared ? launch_fwd<2, true>(c, x, Wd, y, s) : launch_fwd<2, false>(c, x, Wd, y, s);
  if (C <= 4 * kActGroups) return shared ? launch_fwd<4, true>(c, x, Wd, y, s) : launch_fwd<4, false>(c, x, Wd, y, s);
  return shared ? launch_fwd<8, true>(c, x, Wd, y, s) : launch_fwd<8, false>(c, x, Wd, y, s);
}

int eqa_vn_act_bwd(const float* x, const float* Wd, const float* gy, float* gx, float* partial, int B, int C, long long P, int D,
                   int softplus, float slope, void* stream) {
  if (!x || !Wd || !gy || !gx || !partial) return EQA_ERR_INVALID_ARG;
  ActCfg c;
  const int st = act_cfg(c, B, C, P, D, softplus, slope);
  if (st != EQA_OK) return st;
  hipStream_t s = (hipStream_t)stream;
  const bool shared = D == 1 && C > 1;
  if (C <= 16) return shared ? launch_bwd<2, true, 1>(c, x, Wd, gy, gx, partial, s) : launch_bwd<2, false, 1>(c, x, Wd, gy, gx, partial, s);
  if (C <= 2 * kActGroups)
    return shared ? launch_bwd<2, true, 2>(c, x, Wd, gy, gx, partial, s) : launch_bwd<2, false, 2>(c, x, Wd, gy, gx, partial, s);
  if (C <= 4 * kActGroups)
    return shared ? launch_bwd<4, true, 2>(c, x, Wd, gy, gx, partial, s) : launch_bwd<4, false, 2>(c, x, Wd, gy, gx, partial, s);
  return shared ? launch_bwd<8, true, 4>(c, x, Wd, gy, gx, partial, s) : launch_bwd<8, false, 4>(c, x, Wd, gy, gx, partial, s);
}
