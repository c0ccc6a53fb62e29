// libeqa_hip.so, part 5 of 7 -- point clouds: the SO(3) action (P4), batched Gram-Schmidt (P3) and its backward.  The fused VNSmall
// forward and the canonicalizer's one-launch tail are in vnsmall_fwd.hip, the n-body frame in nbody_frame.hip.
// C ABI: include/eqa_hip.h.  HISTORY.md section 3.3.
#include "eqa_common.hpp"
#include "vn_common.hpp"

namespace {

template <bool VEC>
__global__ __launch_bounds__(kThreads) void so3_rotate_kernel(const float* __restrict__ x, const float* __restrict__ R,
                                                             float* __restrict__ y, int N, int transpose) {
  const int b = blockIdx.y;
  const float* Rb = R + (size_t)b * 9;
  float m[9];
#pragma unroll
  for (int k = 0; k < 9; ++k) m[k] = transpose ? Rb[(k % 3) * 3 + k / 3] : Rb[k];
  const float* xb = x + (size_t)b * 3 * N;
  float* yb = y + (size_t)b * 3 * N;
  if (VEC) {
    const int n4 = N >> 2;
    const int k = blockIdx.x * kThreads + threadIdx.x;
    if (k >= n4) return;
    const float4 p0 = reinterpret_cast<const float4*>(xb)[k];
    const float4 p1 = reinterpret_cast<const float4*>(xb + N)[k];
    const float4 p2 = reinterpret_cast<const float4*>(xb + 2 * (size_t)N)[k];
#pragma unroll
    for (int r = 0; r < 3; ++r) {
      // same accumulation order as a k-ordered dot product: (m0*x0 + m1*x1) + m2*x2
      float4 o;
      o.x = m[r * 3] * p0.x + m[r * 3 + 1] * p1.x + m[r * 3 + 2] * p2.x;
      o.y = m[r * 3] * p0.y + m[r * 3 + 1] * p1.y + m[r * 3 + 2] * p2.y;
      o.z = m[r * 3] * p0.z + m[r * 3 + 1] * p1.z + m[r * 3 + 2] * p2.z;
      o.w = m[r * 3] * p0.w + m[r * 3 + 1] * p1.w + m[r * 3 + 2] * p2.w;
      reinterpret_cast<float4*>(yb + (size_t)r * N)[k] = o;
    }
  } else {
    const int k = blockIdx.x * kThreads + threadIdx.x;
    if (k >= N) return;
    const float p0 = xb[k], p1 = xb[N + k], p2 = xb[2 * (size_t)N + k];
#pragma unroll
    for (int r = 0; r < 3; ++r) yb[(size_t)r * N + k] = m[r * 3] * p0 + m[r * 3 + 1] * p1 + m[r * 3 + 2] * p2;
  }
}

// (the arithmetic: gram_schmidt_rows, vn_common.hpp -- shared with the fused canonicalizer tail)
__global__ __launch_bounds__(kThreads) void gram_schmidt_kernel(const float* __restrict__ v, float* __restrict__ out, int B) {
  const int b = blockIdx.x * kThreads + threadIdx.x;
  if (b >= B) return;
  gram_schmidt_rows(v + (size_t)b * 9, out + (size_t)b * 9);
}

// Backward of the classical Gram-Schmidt above: g:(B,3,3) = dL/d(e1,e2,e3) -> gv:(B,3,3) = dL/d(v1,v2,v3).  With e = u / |u|,
// dL/du = (g - e <e, g>) / |u|;  u3 = v3 - <v3,e1> e1 - <v3,e2> e2 and u2 = v2 - <v2,e1> e1 feed gradients back into e1, e2:
//   d/de of -<v,e> e against gu:  -(<v,e> gu + <gu,e> v).
// (As 100 element-wise autograd launches on (B,3) tensors this was the largest host cost of a point-cloud training step.)
__global__ __launch_bounds__(kThreads) void gram_schmidt_bwd_kernel(const float* __restrict__ v, const float* __restrict__ g,
                                                                   float* __restrict__ gv, int B) {
  const int b = blockIdx.x * kThreads + threadIdx.x;
  if (b >= B) return;
  const float* p = v + (size_t)b * 9;
  const float* q = g + (size_t)b * 9;
  const V3 v1 = v3(p[0], p[1], p[2]), v2 = v3(p[3], p[4], p[5]), vv3 = v3(p[6], p[7], p[8]);
  auto scaled = [](const V3& a, float s) { return v3(a.x * s, a.y * s, a.z * s); };
  auto sub = [](const V3& a, const V3& c) { return v3(a.x - c.x, a.y - c.y, a.z - c.z); };
  auto add = [](const V3& a, const V3& c) { return v3(a.x + c.x, a.y + c.y, a.z + c.z); };
  // forward, keeping the lengths
  const float n1 = sqrtf(dot3(v1, v1));
  const V3 e1 = scaled(v1, 1.0f / n1);
  const float c = dot3(v2, e1);
  const V3 u2 = sub(v2, scaled(e1, c));
  const float n2 = sqrtf(dot3(u2, u2));
  const V3 e2 = scaled(u2, 1.0f / n2);
  const float a1 = dot3(vv3, e1), a2 = dot3(vv3, e2);
  const V3 u3 = sub(sub(vv3, scaled(e1, a1)), scaled(e2, a2));
  const float n3 = sqrtf(dot3(u3, u3));
  const V3 e3 = scaled(u3, 1.0f / n3);
  // backward
  V3 g1 = v3(q[0], q[1], q[2]), g2 = v3(q[3], q[4], q[5]);
  const V3 g3 = v3(q[6], q[7], q[8]);
  const V3 gu3 = scaled(sub(g3, scaled(e3, dot3(e3, g3))), 1.0f / n3);
  const float s31 = dot3(gu3, e1), s32 = dot3(gu3, e2);
  const V3 gv3 = sub(sub(gu3, scaled(e1, s31)), scaled(e2, s32));
  g1 = sub(g1, add(scaled(gu3, a1), scaled(vv3, s31)));
  g2 = sub(g2, add(scaled(gu3, a2), scaled(vv3, s32)));
  const V3 gu2 = scaled(sub(g2, scaled(e2, dot3(e2, g2))), 1.0f / n2);
  const float s21 = dot3(gu2, e1);
  const V3 gv2 = sub(gu2, scaled(e1, s21));
  g1 = sub(g1, add(scaled(gu2, c), scaled(v2, s21)));
  const V3 gv1 = scaled(sub(g1, scaled(e1, dot3(e1, g1))), 1.0f / n1);
  float* o = gv + (size_t)b * 9;
  o[0] = gv1.x; o[1] = gv1.y; o[2] = gv1.z; o[3] = gv2.x; o[4] = gv2.y; o[5] = gv2.z; o[6] = gv3.x; o[7] = gv3.y; o[8] = gv3.z;
}

}  // namespace

extern "C" {

int eqa_so3_rotate(const float* x, const float* R, float* y, int B, int N, int transpose, void* stream) {
  if (B == 0 && N > 0) return EQA_OK;
  if (!x || !R || !y || B < 0 || N <= 0) return EQA_ERR_INVALID_ARG;
  if (B > 65535) return EQA_ERR_UNSUPPORTED;
  hipStream_t st = (hipStream_t)stream;
  const bool vec = (N % 4 == 0) && ((((uintptr_t)x | (uintptr_t)y) & 15) == 0);
  if (vec)
    hipLaunchKernelGGL((so3_rotate_kernel<true>), dim3(((N >> 2) + kThreads - 1) / kThreads, B), dim3(kThreads), 0, st, x, R, y, N, transpose);
  else
    hipLaunchKernelGGL((so3_rotate_kernel<false>), dim3((N + kThreads - 1) / kThreads, B), dim3(kThreads), 0, st, x, R, y, N, transpose);
  return launch_status();
}

int eqa_gram_schmidt_bwd(const float* v, const float* grad_out, float* grad_v, int B, void* stream) {
  if (B == 0) return EQA_OK;
  if (!v || !grad_out || !grad_v || B < 0) return EQA_ERR_INVALID_ARG;
  hipLaunchKernelGGL(gram_schmidt_bwd_kernel, dim3((B + kThreads - 1) / kThreads), dim3(kThreads), 0, (hipStream_t)stream, v, grad_out,
                     grad_v, B);
  return launch_status();
}

int eqa_gram_schmidt(const float* v, float* out, int B, void* stream) {
  if (B == 0) return EQA_OK;
  if (!v || !out || B < 0) return EQA_ERR_INVALID_ARG;
  hipLaunchKernelGGL(gram_schmidt_kernel, dim3((B + kThreads - 1) / kThreads), dim3(kThreads), 0, (hipStream_t)stream, v, out, B);
  return launch_status();
}

}  // extern "C"
