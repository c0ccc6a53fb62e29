// VNDeepSets, the n-body canonicalization network (equiadapt/nbody/canonicalization_networks/custom_equivariant_networks.py:13-281),
// as one launch: centring, features (with the cross product), every set layer, the final pooling, the output layer and the
// broadcast to a system's five bodies.  A training pair (forward that keeps each layer's input; backward for the parameters)
// and the small kernel that turns an edge list into per-system in-edge counts.
//
// Layout.  One lane per (system, body, axis): 15 lanes per system, 4 systems per wave, lanes 60..63 idle; one wave per block.  A
// lane holds its H channels in registers (H = 8, 16 or 32: compiled widths; the caller zero-pads any other hidden_dim).  The sum over a node's incoming edges and the sum over a system's bodies read the
// five lanes of the same axis; the dot product over the three axes reads the three lanes of the same body: cross-lane reads inside
// 15 contiguous lanes.  Weights are read at wave-uniform addresses straight from the packed parameter buffer (they arrive through
// the scalar data cache: no staging).  Packed parameters, in the order of `VNDeepSets.parameters()`:
//   per layer  identity_linear.weight (H, Cin), .bias (H), pooling_linear.weight (H, Cin), .bias (H), map_to_dir.weight (H, H)
//   then       output_layer.weight (4, H), .bias (4);          Cin = the number of input features (1..4) for layer 0, else H.
// The backward gives every block a row of a (blocks, n_params) buffer: the block's lanes put their factors into LDS, each lane
// sums a few entries of the outer products over the 60 rows (per system, the four sums added pairwise), and adds them to the block's own row -- plain loads and stores in a
// fixed order.  No float atomics anywhere: two launches on the same input give the same bits.
#include "eqa_common.hpp"

namespace {

constexpr int kWave = 64;
constexpr int kBodies = 5;                    // bodies per system: hard-wired in the reference (`repeat(1, 5)`)
constexpr int kSysLanes = 3 * kBodies;        // 15
constexpr int kSysPerWave = 4;
constexpr int kMaxLayers = 8;
constexpr int kMaxBwdBlocks = 256;
constexpr float kEps = 1e-6f;                 // EPS of custom_group_equivariant_layers.py:4
constexpr int kFeatVel = 1, kFeatAngular = 2, kFeatCharge = 4;

constexpr int kFlagRange = 1, kFlagCross = 2, kFlagLastNode = 4;     // eqa_nbody_adjacency's verdict bits

struct NbCfg {
  int S, H, L, feat, cin0, softplus;
  float slope;
  int layer_mean, final_mean, ct;
};

__host__ __device__ inline int layer_offset(int H, int cin0, int l) {
  return l == 0 ? 0 : 2 * (H * cin0 + H) + H * H + (l - 1) * (3 * H * H + 2 * H);
}
__host__ __device__ inline int param_count(int H, int cin0, int L) { return layer_offset(H, cin0, L) + 4 * H + 4; }

// ---------------------------------------------------------------------------------------------------------------- adjacency
__global__ __launch_bounds__(kThreads) void nbody_adjacency_kernel(const int64_t* __restrict__ rows, const int64_t* __restrict__ cols,
                                                                   size_t E, long long M, int32_t* __restrict__ adj,
                                                                   int32_t* __restrict__ flag) {
  const size_t e = (size_t)blockIdx.x * kThreads + threadIdx.x;
  if (e >= E) return;
  const long long r = rows[e], c = cols[e];
  if (r < 0 || r >= M || c < 0 || c >= M) {
    atomicOr(flag, kFlagRange);
    return;
  }
  const long long sr = r / kBodies, sc = c / kBodies;
  if (sr != sc) {
    atomicOr(flag, kFlagCross);
    return;
  }
  if (c == M - 1) atomicOr(flag, kFlagLastNode);
  atomicAdd(adj + (size_t)sc * 25 + (int)(c - sc * kBodies) * kBodies + (int)(r - sr * kBodies), 1);   // [system][target][source]
}

// ------------------------------------------------------------------------------------------------------------------- lanes
struct Lane {
  int base, b, a;     // first lane of the system, body, axis
  bool valid;         // carries a node of a system < S (the others compute on a clamped system and store nothing)
  size_t m;           // node
  float cnt[kBodies];   // edges body j -> this body
  float cntT[kBodies];  // edges this body -> body j
  float deg;          // what the layer pooling divides by: max(in-degree, 1) for the mean, 1 for the sum
};

__device__ __forceinline__ Lane make_lane(const NbCfg& c, size_t group, const int32_t* __restrict__ adj) {
  Lane t;
  const int lane = threadIdx.x;
  int sl = lane / kSysLanes;
  const int r = lane - sl * kSysLanes;
  const bool idle = sl >= kSysPerWave;
  if (idle) sl = kSysPerWave - 1;
  size_t s = group * kSysPerWave + sl;
  t.valid = !idle && s < (size_t)c.S;
  if (s >= (size_t)c.S) s = (size_t)c.S - 1;
  t.base = sl * kSysLanes;
  t.b = r / 3;
  t.a = r - t.b * 3;
  t.m = s * kBodies + t.b;
  const int32_t* A = adj + s * 25;
  int deg = 0;
#pragma unroll
  for (int j = 0; j < kBodies; ++j) {
    const int v = A[t.b * kBodies + j];
    deg += v;
    t.cnt[j] = (float)v;
    t.cntT[j] = (float)A[j * kBodies + t.b];
  }
  t.deg = c.layer_mean ? (float)(deg > 1 ? deg : 1) : 1.0f;
  return t;
}

__device__ __forceinline__ float body_sum(float v, const Lane& t) {     // over the system's bodies, same axis; to every lane of it
  float acc = 0.0f;
#pragma unroll
  for (int j = 0; j < kBodies; ++j) acc += __shfl(v, t.base + j * 3 + t.a);
  return acc;
}
__device__ __forceinline__ float axis_sum(float v, const Lane& t) {     // over the node's three axes
  const int l0 = t.base + t.b * 3;
  return (__shfl(v, l0) + __shfl(v, l0 + 1)) + __shfl(v, l0 + 2);
}

// the input features of layer 0 (custom_equivariant_networks.py:129-152) and the system's pooled position
template <int HP>
__device__ __forceinline__ void input_features(const NbCfg& c, const Lane& t, const float* __restrict__ loc,
                                               const float* __restrict__ vel, const float* __restrict__ charges, float (&x)[HP],
                                               float& mean_loc) {
  const float p = loc[t.m * 3 + t.a];
  float ml = body_sum(p, t);
  if (c.layer_mean) ml = ml / (float)kBodies;      // (the reference pools the positions with layer_pooling: a sum stays a sum)
  mean_loc = ml;
  const float cl = p - ml;
  const float v = (c.feat & kFeatVel) ? vel[t.m * 3 + t.a] : 0.0f;
  float ang = 0.0f, ch = 0.0f;
  if (c.feat & kFeatAngular) {
    const int l0 = t.base + t.b * 3, a1 = t.a == 2 ? 0 : t.a + 1, a2 = t.a == 0 ? 2 : t.a - 1;
    ang = __shfl(cl, l0 + a1) * __shfl(v, l0 + a2) - __shfl(cl, l0 + a2) * __shfl(v, l0 + a1);
  }
  if (c.feat & kFeatCharge) ch = cl * charges[t.m];
#pragma unroll
  for (int i = 0; i < HP; ++i) x[i] = 0.0f;
  x[0] = cl;                                       // "p", "pv", "pva", "pvc", "pvac": channels in the string's order
  x[1] = v;
  x[2] = (c.feat & kFeatAngular) ? ang : ch;
  x[3] = ch;
}

// pooled input, pre-activation z, direction d = map_to_dir z and the per-channel <z, d>, |d|^2 of one layer.
// CP: width of the layer's input held in x (4 for layer 0, whose Cin = c.cin0; HP for the others, whose Cin = H).
template <int HP, int CP>
__device__ __forceinline__ void layer_pre(const NbCfg& c, const float* __restrict__ W, const Lane& t, const float (&x)[HP],
                                          float (&p)[HP], float (&z)[HP], float (&d)[HP], float (&dot)[HP], float (&q)[HP]) {
  constexpr int H = HP;      // the kernels are compiled for the widths 8, 16, 32; c.H == HP
  const int Cin = CP == HP ? H : c.cin0;
  const float* WI = W;
  const float* bI = WI + H * Cin;
  const float* WP = bI + H;
  const float* bP = WP + H * Cin;
  const float* Wd = bP + H;
#pragma unroll
  for (int i = 0; i < HP; ++i) p[i] = 0.0f;
#pragma unroll
  for (int i = 0; i < CP; ++i) {
    if (i < Cin) {
      float acc = 0.0f;
#pragma unroll
      for (int j = 0; j < kBodies; ++j) acc = fmaf(t.cnt[j], __shfl(x[i], t.base + j * 3 + t.a), acc);
      p[i] = acc / t.deg;
    }
  }
#pragma unroll
  for (int o = 0; o < HP; ++o) {
    z[o] = 0.0f;
    if (o < H) {
      float acc = bI[o] + bP[o];
#pragma unroll
      for (int i = 0; i < CP; ++i) {
        if (i < Cin) {
          acc = fmaf(WI[o * Cin + i], x[i], acc);
          acc = fmaf(WP[o * Cin + i], p[i], acc);
        }
      }
      z[o] = acc;
    }
  }
#pragma unroll
  for (int o = 0; o < HP; ++o) {
    d[o] = 0.0f;
    dot[o] = 0.0f;
    q[o] = 0.0f;
    if (o < H) {
      float acc = 0.0f;
#pragma unroll
      for (int i = 0; i < HP; ++i)
        if (i < H) acc = fmaf(Wd[o * H + i], z[i], acc);
      d[o] = acc;
      dot[o] = axis_sum(z[o] * acc, t);
      q[o] = axis_sum(acc * acc, t);
    }
  }
}

// the vector nonlinearity (custom_group_equivariant_layers.py:31-99): slope z + (1 - slope) (mask z + (1 - mask) (z - t d)),
// t = <z, d> / (|d|^2 + EPS), written as z - (1 - slope) (1 - mask) t d.  LeakyReLU: mask = [<z, d> >= 0].  Softplus (slope 0):
// mask = cos^2(acos(c) / 2) = (1 + c) / 2, c = <z, d> / (|z| |d| + EPS).
template <int HP>
__device__ __forceinline__ void activation(const NbCfg& c, const Lane& t, const float (&z)[HP], const float (&d)[HP],
                                           const float (&dot)[HP], const float (&q)[HP], float (&y)[HP]) {
  constexpr int H = HP;      // the kernels are compiled for the widths 8, 16, 32; c.H == HP
  if (!c.softplus) {
    const float k = 1.0f - c.slope;
#pragma unroll
    for (int o = 0; o < HP; ++o) {
      y[o] = 0.0f;
      if (o < H) y[o] = dot[o] >= 0.0f ? z[o] : z[o] - k * (dot[o] / (q[o] + kEps)) * d[o];
    }
  } else {
#pragma unroll
    for (int o = 0; o < HP; ++o) {
      y[o] = 0.0f;
      if (o < H) {
        const float nz = sqrtf(axis_sum(z[o] * z[o], t));
        const float cs = dot[o] / (nz * sqrtf(q[o]) + kEps);
        const float mask = 0.5f * (1.0f + cs);
        y[o] = z[o] - (1.0f - mask) * (dot[o] / (q[o] + kEps)) * d[o];
      }
    }
  }
}

// one layer forward, in place: x <- dropout(activation) (+ x)
template <int HP, int CP>
__device__ __forceinline__ void layer_forward(const NbCfg& c, const float* __restrict__ P, int l, const Lane& t,
                                              const float* __restrict__ mask, float (&x)[HP]) {
  constexpr int H = HP;      // the kernels are compiled for the widths 8, 16, 32; c.H == HP
  float p[HP], z[HP], d[HP], dot[HP], q[HP], y[HP];
  layer_pre<HP, CP>(c, P + layer_offset(c.H, c.cin0, l), t, x, p, z, d, dot, q);
  activation<HP>(c, t, z, d, dot, q, y);
  if (mask) {
    const float* mrow = mask + (((size_t)l * c.S * kBodies + t.m) * 3 + t.a) * H;
#pragma unroll
    for (int o = 0; o < HP; ++o)
      if (o < H) y[o] *= mrow[o];
  }
#pragma unroll
  for (int o = 0; o < HP; ++o) x[o] = CP == HP ? y[o] + x[o] : y[o];     // residual on every layer but the first
}

// ----------------------------------------------------------------------------------------------------------------- forward
// mask: (L, M, 3, H) dropout factors or NULL; saved: (L - 1, M, 3, H), the inputs of layers 1 .. L-1, or NULL
template <int HP>
__global__ __launch_bounds__(kWave) void vndeepsets_fwd_kernel(NbCfg c, const float* __restrict__ loc, const float* __restrict__ vel,
                                                               const float* __restrict__ charges, const int32_t* __restrict__ adj,
                                                               const float* __restrict__ P, const float* __restrict__ mask,
                                                               float* __restrict__ saved, float* __restrict__ rot,
                                                               float* __restrict__ trans) {
  constexpr int H = HP;      // the kernels are compiled for the widths 8, 16, 32; c.H == HP
  const Lane t = make_lane(c, blockIdx.x, adj);
  float x[HP], mean_loc;
  input_features<HP>(c, t, loc, vel, charges, x, mean_loc);
  layer_forward<HP, 4>(c, P, 0, t, mask, x);
#pragma unroll 1
  for (int l = 1; l < c.L; ++l) {
    if (saved && t.valid) {
      float* srow = saved + (((size_t)(l - 1) * c.S * kBodies + t.m) * 3 + t.a) * H;
#pragma unroll
      for (int i = 0; i < HP; ++i)
        if (i < H) srow[i] = x[i];
    }
    layer_forward<HP, HP>(c, P, l, t, mask, x);
  }
  const float* Wout = P + layer_offset(c.H, c.cin0, c.L);
  const float* bout = Wout + 4 * H;
  float out[4] = {bout[0], bout[1], bout[2], bout[3]};
  const float fdiv = c.final_mean ? (float)kBodies : 1.0f;
#pragma unroll
  for (int i = 0; i < HP; ++i) {
    if (i < H) {
      const float pf = body_sum(x[i], t) / fdiv;
#pragma unroll
      for (int k = 0; k < 4; ++k) out[k] = fmaf(Wout[k * H + i], pf, out[k]);
    }
  }
  if (t.valid) {
    float* r = rot + t.m * 9 + t.a * 3;
    r[0] = out[0];
    r[1] = out[1];
    r[2] = out[2];
    trans[t.m * 3 + t.a] = (c.ct ? out[3] : 0.0f) + mean_loc;
  }
}

// ---------------------------------------------------------------------------------------------------------------- backward
// dst[o * nb + i] (+)= sum over the 60 rows k of A[k][o] B[k][i]; A, B: LDS, rows of HP floats at a stride of HP + 1 (odd: the 64
// lanes' stores of one column fall into different banks).  The rows are summed per system (15 rows each, four independent chains)
// and the four sums added pairwise: shorter chains than one of 60, less rounding.  Entry e belongs to lane e % 64 in every call,
// so a block's read-modify-write of its own row needs no ordering beyond program order.
template <int HP>
__device__ __forceinline__ void outer_accumulate(float* __restrict__ dst, const float* A, const float* B, int na, int nb, bool first) {
  constexpr int LD = HP + 1;
  const int n = na * nb;
  for (int e = threadIdx.x; e < n; e += kWave) {
    const int o = e / nb, i = e - o * nb;
    float acc[kSysPerWave] = {0.0f, 0.0f, 0.0f, 0.0f};
#pragma unroll 3
    for (int k = 0; k < kSysLanes; ++k) {
#pragma unroll
      for (int s = 0; s < kSysPerWave; ++s) {
        const int row = s * kSysLanes + k;
        acc[s] = fmaf(A[row * LD + o], B[row * LD + i], acc[s]);
      }
    }
    const float sum = (acc[0] + acc[1]) + (acc[2] + acc[3]);
    dst[e] = first ? sum : dst[e] + sum;
  }
}
template <int HP>
__device__ __forceinline__ void column_accumulate(float* __restrict__ dst, const float* A, int na, bool first) {
  constexpr int LD = HP + 1;
  for (int o = threadIdx.x; o < na; o += kWave) {
    float acc[kSysPerWave] = {0.0f, 0.0f, 0.0f, 0.0f};
#pragma unroll 3
    for (int k = 0; k < kSysLanes; ++k) {
#pragma unroll
      for (int s = 0; s < kSysPerWave; ++s) acc[s] += A[(s * kSysLanes + k) * LD + o];
    }
    const float sum = (acc[0] + acc[1]) + (acc[2] + acc[3]);
    dst[o] = first ? sum : dst[o] + sum;
  }
}

template <int HP>
struct BwdLds {
  static constexpr int LD = HP + 1;
  static constexpr int kFloats = kWave * LD;
  float gz[kFloats], x[kFloats], p[kFloats], gd[kFloats], z[kFloats];
};

// One layer backward.  x: the layer's input; g: dL/d(layer output) on entry, dL/d(layer input) on return (not formed for layer 0,
// whose input has no parameters behind it).  The last layer also finishes the forward (final pooling) for the output layer's
// gradient and forms g from `go`, dL/d(output layer's result) summed over the system's bodies.
template <int HP, int CP>
__device__ __forceinline__ void layer_backward(const NbCfg& c, const float* __restrict__ P, float* __restrict__ out, int l,
                                               const Lane& t, const float* __restrict__ mask, const float (&x)[HP],
                                               const float (&go)[4], float (&g)[HP], BwdLds<HP>& lds, bool first) {
  constexpr int H = HP;      // the kernels are compiled for the widths 8, 16, 32; c.H == HP
  const int Cin = CP == HP ? H : c.cin0;
  const int lane = threadIdx.x;
  const int off = layer_offset(c.H, c.cin0, l);
  const float* W = P + off;
  const float* WI = W;
  const float* WP = WI + H * Cin + H;
  const float* Wd = WP + H * Cin + H;
  const float* mrow = mask ? mask + (((size_t)l * c.S * kBodies + t.m) * 3 + t.a) * H : nullptr;
  float p[HP], z[HP], d[HP], dot[HP], q[HP];
  layer_pre<HP, CP>(c, W, t, x, p, z, d, dot, q);

  if (l == c.L - 1) {
    float y[HP];
    activation<HP>(c, t, z, d, dot, q, y);
    const int offo = layer_offset(c.H, c.cin0, c.L);
    const float* Wout = P + offo;
    const float fdiv = c.final_mean ? (float)kBodies : 1.0f;
    const bool head = t.valid && t.b == 0;        // one lane per (system, axis) carries the output layer's gradient
#pragma unroll
    for (int i = 0; i < HP; ++i) {
      float pf = 0.0f;
      if (i < H) {
        float yi = y[i];
        if (mrow) yi *= mrow[i];
        if (CP == HP) yi += x[i];
        pf = body_sum(yi, t) / fdiv;
      }
      lds.x[lane * BwdLds<HP>::LD + i] = pf;
    }
#pragma unroll
    for (int k = 0; k < 4; ++k) lds.gz[lane * BwdLds<HP>::LD + k] = head ? go[k] : 0.0f;
    __syncthreads();
    outer_accumulate<HP>(out + offo, lds.gz, lds.x, 4, H, first);
    column_accumulate<HP>(out + offo + 4 * H, lds.gz, 4, first);
    __syncthreads();
#pragma unroll
    for (int i = 0; i < HP; ++i) {
      g[i] = 0.0f;
      if (i < H && t.valid) {
        float acc = 0.0f;
#pragma unroll
        for (int k = 0; k < 4; ++k) acc = fmaf(Wout[k * H + i], go[k], acc);
        g[i] = acc / fdiv;
      }
    }
  }

  // through dropout and the nonlinearity: out = z - k [<z, d> < 0] t d, t = <z, d> / (|d|^2 + EPS), k = 1 - slope
  const float kk = 1.0f - c.slope;
  float gz[HP], gd[HP];
#pragma unroll
  for (int o = 0; o < HP; ++o) {
    gz[o] = 0.0f;
    gd[o] = 0.0f;
    if (o < H) {
      const float gy = mrow ? g[o] * mrow[o] : g[o];
      const float gdot3 = axis_sum(gy * d[o], t);
      gz[o] = gy;
      if (dot[o] < 0.0f) {
        const float rq = 1.0f / (q[o] + kEps);
        const float tt = dot[o] * rq;
        const float g_t = -kk * gdot3;
        const float g_dot = g_t * rq;
        const float g_q = -g_t * tt * rq;
        gz[o] = fmaf(g_dot, d[o], gy);
        gd[o] = fmaf(-kk * tt, gy, fmaf(g_dot, z[o], 2.0f * g_q * d[o]));
      }
    }
  }
#pragma unroll
  for (int i = 0; i < HP; ++i) {       // d = map_to_dir z
    if (i < H) {
      float acc = gz[i];
#pragma unroll
      for (int o = 0; o < HP; ++o)
        if (o < H) acc = fmaf(Wd[o * H + i], gd[o], acc);
      lds.gz[lane * BwdLds<HP>::LD + i] = acc;
      lds.gd[lane * BwdLds<HP>::LD + i] = gd[i];
      lds.z[lane * BwdLds<HP>::LD + i] = z[i];
    }
  }
#pragma unroll
  for (int i = 0; i < CP; ++i) {
    if (i < Cin) {
      lds.x[lane * BwdLds<HP>::LD + i] = x[i];
      lds.p[lane * BwdLds<HP>::LD + i] = p[i];
    }
  }
  __syncthreads();
  float* dW = out + off;
  outer_accumulate<HP>(dW, lds.gz, lds.x, H, Cin, first);                              // identity_linear.weight
  column_accumulate<HP>(dW + H * Cin, lds.gz, H, first);                               // identity_linear.bias
  outer_accumulate<HP>(dW + H * Cin + H, lds.gz, lds.p, H, Cin, first);                // pooling_linear.weight
  column_accumulate<HP>(dW + 2 * H * Cin + H, lds.gz, H, first);                       // pooling_linear.bias
  outer_accumulate<HP>(dW + 2 * H * Cin + 2 * H, lds.gd, lds.z, H, H, first);          // map_to_dir.weight

  if (CP == HP) {      // dL/d(input): identity path, residual, and the pooled path spread back along the edges
    float gzt[HP];
#pragma unroll
    for (int o = 0; o < HP; ++o) gzt[o] = o < H ? lds.gz[lane * BwdLds<HP>::LD + o] : 0.0f;
#pragma unroll
    for (int i = 0; i < HP; ++i) {
      if (i < H) {
        float gi = g[i], gp = 0.0f;
#pragma unroll
        for (int o = 0; o < HP; ++o) {
          if (o < H) {
            gi = fmaf(WI[o * H + i], gzt[o], gi);
            gp = fmaf(WP[o * H + i], gzt[o], gp);
          }
        }
        gp = gp / t.deg;
#pragma unroll
        for (int j = 0; j < kBodies; ++j) gi = fmaf(t.cntT[j], __shfl(gp, t.base + j * 3 + t.a), gi);
        g[i] = gi;
      }
    }
  }
  __syncthreads();
}

// partial: (gridDim.x, n_params); every block writes its whole row (a block always has at least one group)
template <int HP>
__global__ __launch_bounds__(kWave) void vndeepsets_bwd_kernel(NbCfg c, const float* __restrict__ loc, const float* __restrict__ vel,
                                                               const float* __restrict__ charges, const int32_t* __restrict__ adj,
                                                               const float* __restrict__ P, const float* __restrict__ mask,
                                                               const float* __restrict__ saved, const float* __restrict__ grot,
                                                               const float* __restrict__ gtrans, float* __restrict__ partial,
                                                               int n_params, unsigned groups) {
  __shared__ BwdLds<HP> lds;
  constexpr int H = HP;      // the kernels are compiled for the widths 8, 16, 32; c.H == HP
  float* out = partial + (size_t)blockIdx.x * n_params;
  bool first = true;
  for (int i = threadIdx.x; i < BwdLds<HP>::kFloats; i += kWave) {      // rows and columns the layers never write stay zero
    lds.gz[i] = 0.0f; lds.x[i] = 0.0f; lds.p[i] = 0.0f; lds.gd[i] = 0.0f; lds.z[i] = 0.0f;
  }
  __syncthreads();
#pragma unroll 1
  for (unsigned group = blockIdx.x; group < groups; group += gridDim.x) {
    const Lane t = make_lane(c, group, adj);
    float go[4];
#pragma unroll
    for (int k = 0; k < 3; ++k) go[k] = body_sum(t.valid ? grot[t.m * 9 + t.a * 3 + k] : 0.0f, t);
    go[3] = c.ct ? body_sum(t.valid ? gtrans[t.m * 3 + t.a] : 0.0f, t) : 0.0f;
    float g[HP], x[HP];
#pragma unroll
    for (int i = 0; i < HP; ++i) g[i] = 0.0f;
#pragma unroll 1
    for (int l = c.L - 1; l >= 1; --l) {
      const float* srow = saved + (((size_t)(l - 1) * c.S * kBodies + t.m) * 3 + t.a) * H;
#pragma unroll
      for (int i = 0; i < HP; ++i) x[i] = i < H ? srow[i] : 0.0f;
      layer_backward<HP, HP>(c, P, out, l, t, mask, x, go, g, lds, first);
    }
    float mean_loc;
    input_features<HP>(c, t, loc, vel, charges, x, mean_loc);
    layer_backward<HP, 4>(c, P, out, 0, t, mask, x, go, g, lds, first);
    first = false;
  }
}

int check_cfg(const NbCfg& c, const void* loc, const void* vel, const void* charges, const void* adj, const void* params) {
  if (!loc || !adj || !params || c.S <= 0 || c.H <= 0 || c.L <= 0) return EQA_ERR_INVALID_ARG;
  if (c.feat < 0 || c.feat > 7) return EQA_ERR_INVALID_ARG;
  if (c.feat != 0 && !(c.feat & kFeatVel)) return EQA_ERR_INVALID_ARG;            // "p", "pv", "pva", "pvc", "pvac" only
  if (((c.feat & kFeatVel) && !vel) || ((c.feat & kFeatCharge) && !charges)) return EQA_ERR_INVALID_ARG;
  if ((c.H != 8 && c.H != 16 && c.H != 32) || c.L > kMaxLayers || c.S > (1 << 26)) return EQA_ERR_UNSUPPORTED;
  return EQA_OK;
}

NbCfg make_cfg(int S, int H, int L, int features, int softplus, float slope, int layer_mean, int final_mean, int ct) {
  NbCfg c;
  c.S = S; c.H = H; c.L = L; c.feat = features;
  c.cin0 = 1 + ((features & kFeatVel) ? 1 : 0) + ((features & kFeatAngular) ? 1 : 0) + ((features & kFeatCharge) ? 1 : 0);
  c.softplus = softplus; c.slope = slope; c.layer_mean = layer_mean; c.final_mean = final_mean; c.ct = ct;
  return c;
}

// hidden widths the kernels are compiled for; another hidden_dim is zero-padded to the next one by the caller (a channel whose
// weights and biases are zero stays exactly zero through every layer, forward and backward)
#define EQA_NBODY_DISPATCH(KERNEL, H, ...)       \
  do {                                           \
    if ((H) == 32) KERNEL<32> __VA_ARGS__;       \
    else if ((H) == 16) KERNEL<16> __VA_ARGS__;  \
    else KERNEL<8> __VA_ARGS__;                  \
  } while (0)

int launch_forward(const NbCfg& c, const float* loc, const float* vel, const float* charges, const int32_t* adj, const float* params,
                   const float* mask, float* saved, float* rot, float* trans, hipStream_t stream) {
  const unsigned blocks = (unsigned)((c.S + kSysPerWave - 1) / kSysPerWave);
  EQA_NBODY_DISPATCH(vndeepsets_fwd_kernel, c.H, <<<dim3(blocks), dim3(kWave), 0, stream>>>(c, loc, vel, charges, adj, params, mask,
                                                                                             saved, rot, trans));
  return launch_status();
}

}  // namespace

int eqa_vndeepsets_param_count(int H, int L, int features) {
  if (H <= 0 || L <= 0 || features < 0 || features > 7) return EQA_ERR_INVALID_ARG;
  return param_count(H, make_cfg(1, H, L, features, 0, 0.0f, 0, 0, 0).cin0, L);
}

int eqa_vndeepsets_bwd_blocks(int S) {
  if (S <= 0) return EQA_ERR_INVALID_ARG;
  return std::min((S + kSysPerWave - 1) / kSysPerWave, kMaxBwdBlocks);
}

int eqa_nbody_adjacency(const int64_t* rows, const int64_t* cols, long long E, int S, int32_t* adj, int32_t* flag, void* stream) {
  if (!rows || !cols || !adj || !flag || E <= 0 || S <= 0) return EQA_ERR_INVALID_ARG;
  const size_t nb = ((size_t)E + kThreads - 1) / kThreads;
  if (nb > 0x7fffffffULL || S > (1 << 26)) return EQA_ERR_UNSUPPORTED;
  hipLaunchKernelGGL(nbody_adjacency_kernel, dim3((unsigned)nb), dim3(kThreads), 0, (hipStream_t)stream, rows, cols, (size_t)E,
                     (long long)S * kBodies, adj, flag);
  return launch_status();
}

int eqa_vndeepsets_fwd(const float* loc, const float* vel, const float* charges, const int32_t* adj, const float* params, float* rot,
                       float* trans, int S, int H, int L, int features, int softplus, float slope, int layer_mean, int final_mean,
                       int canon_translation, void* stream) {
  const NbCfg c = make_cfg(S, H, L, features, softplus, slope, layer_mean, final_mean, canon_translation);
  const int st = check_cfg(c, loc, vel, charges, adj, params);
  if (st != EQA_OK) return st;
  if (!rot || !trans) return EQA_ERR_INVALID_ARG;
  return launch_forward(c, loc, vel, charges, adj, params, nullptr, nullptr, rot, trans, (hipStream_t)stream);
}

int eqa_vndeepsets_train_fwd(const float* loc, const float* vel, const float* charges, const int32_t* adj, const float* params,
                             const float* mask, float* saved, float* rot, float* trans, int S, int H, int L, int features,
                             int softplus, float slope, int layer_mean, int final_mean, int canon_translation, void* stream) {
  const NbCfg c = make_cfg(S, H, L, features, softplus, slope, layer_mean, final_mean, canon_translation);
  const int st = check_cfg(c, loc, vel, charges, adj, params);
  if (st != EQA_OK) return st;
  if (!rot || !trans || (L > 1 && !saved)) return EQA_ERR_INVALID_ARG;
  return launch_forward(c, loc, vel, charges, adj, params, mask, L > 1 ? saved : nullptr, rot, trans, (hipStream_t)stream);
}

int eqa_vndeepsets_bwd(const float* loc, const float* vel, const float* charges, const int32_t* adj, const float* params,
                       const float* mask, const float* saved, const float* grad_rot, const float* grad_trans, float* partial, int S,
                       int H, int L, int features, int softplus, float slope, int layer_mean, int final_mean, int canon_translation,
                       void* stream) {
  const NbCfg c = make_cfg(S, H, L, features, softplus, slope, layer_mean, final_mean, canon_translation);
  const int st = check_cfg(c, loc, vel, charges, adj, params);
  if (st != EQA_OK) return st;
  if (!grad_rot || !grad_trans || !partial || (L > 1 && !saved)) return EQA_ERR_INVALID_ARG;
  if (softplus) return EQA_ERR_UNSUPPORTED;       // the backward covers the mask form of the nonlinearity
  const unsigned groups = (unsigned)((S + kSysPerWave - 1) / kSysPerWave);
  const unsigned blocks = (unsigned)eqa_vndeepsets_bwd_blocks(S);
  const int n_params = param_count(H, c.cin0, L);
  EQA_NBODY_DISPATCH(vndeepsets_bwd_kernel, c.H, <<<dim3(blocks), dim3(kWave), 0, (hipStream_t)stream>>>(
                         c, loc, vel, charges, adj, params, mask, saved, grad_rot, grad_trans, partial, n_params, groups));
  return launch_status();
}
