// libeqa_hip.so, part 5c -- (f).4, the frame of the n-body E(3) canonicalizer: modified Gram-Schmidt and the per-row rigid action
// (nbody/canonicalization/euclidean_group.py:87-157), forward and backward; nbody.hip holds the VNDeepSets network in front of it.
// Tiny tensors (nodes x 3): one thread per row.  The arithmetic of a row is stated once, in the two __device__ functions below, for the
// separate kernels and for the one-launch training forward.  C ABI: include/eqa_hip.h.  HISTORY.md section 3.5.
#include "eqa_common.hpp"

namespace {

// modified Gram-Schmidt of the three rows of p -> o (both 9 floats): fp64 inside, rounded once (see gram_schmidt_rows, vn_common.hpp)
__device__ __forceinline__ void modified_gram_schmidt_rows(const float* p, float* o) {
  double a0 = p[0], a1 = p[1], a2 = p[2], b0 = p[3], b1 = p[4], b2 = p[5], c0 = p[6], c1 = p[7], c2 = p[8];
  double n = sqrt(a0 * a0 + a1 * a1 + a2 * a2);
  a0 /= n; a1 /= n; a2 /= n;
  double d = b0 * a0 + b1 * a1 + b2 * a2;
  b0 -= d * a0; b1 -= d * a1; b2 -= d * a2;
  n = sqrt(b0 * b0 + b1 * b1 + b2 * b2);
  b0 /= n; b1 /= n; b2 /= n;
  d = c0 * a0 + c1 * a1 + c2 * a2;
  c0 -= d * a0; c1 -= d * a1; c2 -= d * a2;
  d = c0 * b0 + c1 * b1 + c2 * b2;  // modified GS: second projection uses the UPDATED third vector
  c0 -= d * b0; c1 -= d * b1; c2 -= d * b2;
  n = sqrt(c0 * c0 + c1 * c1 + c2 * c2);
  c0 /= n; c1 /= n; c2 /= n;
  o[0] = (float)a0; o[1] = (float)a1; o[2] = (float)a2; o[3] = (float)b0; o[4] = (float)b1; o[5] = (float)b2;
  o[6] = (float)c0; o[7] = (float)c1; o[8] = (float)c2;
}

// one row under its frame r (9 floats), o: 3 floats
// mode 0: out = x R + t            (invert_canonicalization :126-137; t may be NULL)
// mode 1: out = x R^T - t R^T      (canonicalize :108-124, the two products subtracted as the reference does)
// Each three-term dot product is written out with the multiply-adds rigid_rows_kernel has always had (which product is rounded on
// its own differs between the components), and contraction is off, so every kernel that calls this gives rigid_rows_kernel's bits
// whatever surrounds the call.
__device__ __forceinline__ void rigid_row(const float* x, const float* r, const float* t, float* o, int mode) {
#pragma clang fp contract(off)
  const float x0 = x[0], x1 = x[1], x2 = x[2];
  const float t0 = t ? t[0] : 0.f, t1 = t ? t[1] : 0.f, t2 = t ? t[2] : 0.f;
  if (mode == 0) {
    o[0] = __builtin_fmaf(x2, r[6], __builtin_fmaf(x1, r[3], x0 * r[0])) + t0;
    o[1] = __builtin_fmaf(x2, r[7], __builtin_fmaf(x0, r[1], x1 * r[4])) + t1;
    o[2] = (__builtin_fmaf(x0, r[2], x1 * r[5]) + x2 * r[8]) + t2;
  } else {
    const float a0 = __builtin_fmaf(x2, r[2], __builtin_fmaf(x1, r[1], x0 * r[0]));
    const float a1 = __builtin_fmaf(x2, r[5], __builtin_fmaf(x0, r[3], x1 * r[4]));
    const float a2 = __builtin_fmaf(x0, r[6], x1 * r[7]) + x2 * r[8];
    const float b0 = __builtin_fmaf(t2, r[2], __builtin_fmaf(t0, r[0], t1 * r[1]));
    const float b1 = __builtin_fmaf(t2, r[5], __builtin_fmaf(t0, r[3], t1 * r[4]));
    const float b2 = __builtin_fmaf(t2, r[8], __builtin_fmaf(t0, r[6], t1 * r[7]));
    o[0] = t ? a0 - b0 : a0;
    o[1] = t ? a1 - b1 : a1;
    o[2] = t ? a2 - b2 : a2;
  }
}

__global__ __launch_bounds__(kThreads) void modified_gram_schmidt_kernel(const float* __restrict__ v, float* __restrict__ out, int B) {
  const int b = blockIdx.x * kThreads + threadIdx.x;
  if (b >= B) return;
  modified_gram_schmidt_rows(v + (size_t)b * 9, out + (size_t)b * 9);
}

__global__ __launch_bounds__(kThreads) void rigid_rows_kernel(const float* __restrict__ x, const float* __restrict__ R,
                                                             const float* __restrict__ t, float* __restrict__ out, int M, int mode) {
  const int m = blockIdx.x * kThreads + threadIdx.x;
  if (m >= M) return;
  rigid_row(x + (size_t)m * 3, R + (size_t)m * 9, t ? t + (size_t)m * 3 : nullptr, out + (size_t)m * 3, mode);
}

// The canonicalizer's forward in one launch: R = MGS(v), cloc = loc R^T - t R^T, cvel = vel R^T, the frame rounded to fp32 before it
// is applied -- the bits of modified_gram_schmidt_kernel followed by rigid_rows_kernel mode 1 with and without t.
__global__ __launch_bounds__(kThreads) void nbody_frame_fwd_kernel(const float* __restrict__ v, const float* __restrict__ t,
                                                                  const float* __restrict__ loc, const float* __restrict__ vel,
                                                                  float* __restrict__ R, float* __restrict__ cloc,
                                                                  float* __restrict__ cvel, int M) {
  const int m = blockIdx.x * kThreads + threadIdx.x;
  if (m >= M) return;
  float r[9];
  modified_gram_schmidt_rows(v + (size_t)m * 9, r);
#pragma unroll
  for (int k = 0; k < 9; ++k) R[(size_t)m * 9 + k] = r[k];
  rigid_row(loc + (size_t)m * 3, r, t + (size_t)m * 3, cloc + (size_t)m * 3, 1);
  rigid_row(vel + (size_t)m * 3, r, nullptr, cvel + (size_t)m * 3, 1);
}

struct D3 {
  double x, y, z;
};
__device__ __forceinline__ D3 d3(double x, double y, double z) { return D3{x, y, z}; }
__device__ __forceinline__ double ddot(const D3& a, const D3& b) { return a.x * b.x + a.y * b.y + a.z * b.z; }
__device__ __forceinline__ D3 dscaled(const D3& a, double s) { return d3(a.x * s, a.y * s, a.z * s); }
__device__ __forceinline__ D3 dsub(const D3& a, const D3& b) { return d3(a.x - b.x, a.y - b.y, a.z - b.z); }
// a - (s b + u c)
__device__ __forceinline__ D3 dsub2(const D3& a, double s, const D3& b, double u, const D3& c) {
  return d3(a.x - (s * b.x + u * c.x), a.y - (s * b.y + u * c.y), a.z - (s * b.z + u * c.z));
}

// Backward of nbody_frame_fwd_kernel.  Incoming gR:(M,3,3), gcloc, gcvel:(M,3), each NULL for zero; outgoing gv:(M,3,3), gt, gloc,
// gvel:(M,3), each NULL for not wanted.  With the frame R the forward applied (fp32):
//   gloc = gcloc R,  gt = -gloc,  gvel = gcvel R,  G[j,:] = gR[j,:] + gcloc_j (loc - t) + gcvel_j vel   (dL/dR, row j)
// and gv is the reverse pass of the modified Gram-Schmidt on G, in fp64 with the intermediates recomputed from v, rounded once.
// With e = u / |u|: dL/du = (g - e <e, g>) / |u|; a step u = w - <w, e> e hands  gw = gu - <gu, e> e  down and
// -(<gu, e> w + <w, e> gu) back to e.
__global__ __launch_bounds__(kThreads) void nbody_frame_bwd_kernel(const float* __restrict__ v, const float* __restrict__ t,
                                                                  const float* __restrict__ loc, const float* __restrict__ vel,
                                                                  const float* __restrict__ R, const float* __restrict__ gR,
                                                                  const float* __restrict__ gcloc, const float* __restrict__ gcvel,
                                                                  float* __restrict__ gv, float* __restrict__ gt,
                                                                  float* __restrict__ gloc, float* __restrict__ gvel, int M) {
  const int m = blockIdx.x * kThreads + threadIdx.x;
  if (m >= M) return;
  const size_t m3 = (size_t)m * 3, m9 = (size_t)m * 9;
  double gl[3] = {0.0, 0.0, 0.0}, gw[3] = {0.0, 0.0, 0.0};   // gcloc, gcvel of the row
  if (gcloc) { gl[0] = gcloc[m3]; gl[1] = gcloc[m3 + 1]; gl[2] = gcloc[m3 + 2]; }
  if (gcvel) { gw[0] = gcvel[m3]; gw[1] = gcvel[m3 + 1]; gw[2] = gcvel[m3 + 2]; }
  if (gloc || gt || gvel) {
    double r[9];
#pragma unroll
    for (int k = 0; k < 9; ++k) r[k] = R[m9 + k];
#pragma unroll
    for (int k = 0; k < 3; ++k) {
      const float a = (float)(gl[0] * r[k] + gl[1] * r[3 + k] + gl[2] * r[6 + k]);
      if (gloc) gloc[m3 + k] = a;
      if (gt) gt[m3 + k] = -a;
      if (gvel) gvel[m3 + k] = (float)(gw[0] * r[k] + gw[1] * r[3 + k] + gw[2] * r[6 + k]);
    }
  }
  if (!gv) return;
  D3 G[3];
#pragma unroll
  for (int j = 0; j < 3; ++j) G[j] = gR ? d3(gR[m9 + 3 * j], gR[m9 + 3 * j + 1], gR[m9 + 3 * j + 2]) : d3(0.0, 0.0, 0.0);
  if (gcloc) {
    const D3 p = d3((double)loc[m3] - (double)t[m3], (double)loc[m3 + 1] - (double)t[m3 + 1], (double)loc[m3 + 2] - (double)t[m3 + 2]);
#pragma unroll
    for (int j = 0; j < 3; ++j) G[j] = d3(G[j].x + gl[j] * p.x, G[j].y + gl[j] * p.y, G[j].z + gl[j] * p.z);
  }
  if (gcvel) {
    const D3 q = d3(vel[m3], vel[m3 + 1], vel[m3 + 2]);
#pragma unroll
    for (int j = 0; j < 3; ++j) G[j] = d3(G[j].x + gw[j] * q.x, G[j].y + gw[j] * q.y, G[j].z + gw[j] * q.z);
  }
  const float* p = v + m9;
  const D3 v1 = d3(p[0], p[1], p[2]), v2 = d3(p[3], p[4], p[5]), vv3 = d3(p[6], p[7], p[8]);
  // forward, keeping the lengths (the steps of modified_gram_schmidt_rows)
  const double n1 = sqrt(ddot(v1, v1));
  const D3 e1 = d3(v1.x / n1, v1.y / n1, v1.z / n1);
  const double c = ddot(v2, e1);
  const D3 u2 = dsub(v2, dscaled(e1, c));
  const double n2 = sqrt(ddot(u2, u2));
  const D3 e2 = d3(u2.x / n2, u2.y / n2, u2.z / n2);
  const double a1 = ddot(vv3, e1);
  const D3 w = dsub(vv3, dscaled(e1, a1));
  const double a2 = ddot(w, e2);
  const D3 u3 = dsub(w, dscaled(e2, a2));
  const double n3 = sqrt(ddot(u3, u3));
  const D3 e3 = d3(u3.x / n3, u3.y / n3, u3.z / n3);
  // backward
  D3 g1 = G[0], g2 = G[1];
  const D3 t3 = dsub(G[2], dscaled(e3, ddot(e3, G[2])));
  const D3 gu3 = d3(t3.x / n3, t3.y / n3, t3.z / n3);
  const double s32 = ddot(gu3, e2);
  const D3 gwv = dsub(gu3, dscaled(e2, s32));        // dL/dw
  g2 = dsub2(g2, s32, w, a2, gu3);
  const double s31 = ddot(gwv, e1);
  const D3 gv3 = dsub(gwv, dscaled(e1, s31));
  g1 = dsub2(g1, s31, vv3, a1, gwv);
  const D3 t2 = dsub(g2, dscaled(e2, ddot(e2, g2)));
  const D3 gu2 = d3(t2.x / n2, t2.y / n2, t2.z / n2);
  const double s21 = ddot(gu2, e1);
  const D3 gv2 = dsub(gu2, dscaled(e1, s21));
  g1 = dsub2(g1, s21, v2, c, gu2);
  const D3 t1 = dsub(g1, dscaled(e1, ddot(e1, g1)));
  float* o = gv + m9;
  o[0] = (float)(t1.x / n1); o[1] = (float)(t1.y / n1); o[2] = (float)(t1.z / n1);
  o[3] = (float)gv2.x; o[4] = (float)gv2.y; o[5] = (float)gv2.z; o[6] = (float)gv3.x; o[7] = (float)gv3.y; o[8] = (float)gv3.z;
}

// Backward of rigid_rows_kernel mode 0 (out = x R + t): gx = g R^T, gR[i][j] = x_i g_j; either may be NULL.  (gt is g itself.)
__global__ __launch_bounds__(kThreads) void rigid_rows_bwd_kernel(const float* __restrict__ x, const float* __restrict__ R,
                                                                 const float* __restrict__ g, float* __restrict__ gx,
                                                                 float* __restrict__ gR, int M) {
  const int m = blockIdx.x * kThreads + threadIdx.x;
  if (m >= M) return;
  const size_t m3 = (size_t)m * 3, m9 = (size_t)m * 9;
  const float g0 = g[m3], g1 = g[m3 + 1], g2 = g[m3 + 2];
  if (gx) {
    const float* r = R + m9;
#pragma unroll
    for (int i = 0; i < 3; ++i) gx[m3 + i] = g0 * r[3 * i] + g1 * r[3 * i + 1] + g2 * r[3 * i + 2];
  }
  if (gR) {
#pragma unroll
    for (int i = 0; i < 3; ++i) {
      const float xi = x[m3 + i];
      gR[m9 + 3 * i] = xi * g0; gR[m9 + 3 * i + 1] = xi * g1; gR[m9 + 3 * i + 2] = xi * g2;
    }
  }
}

}  // namespace

extern "C" {

int eqa_modified_gram_schmidt(const float* v, float* out, int B, void* stream) {
  if (B == 0) return EQA_OK;
  if (!v || !out || B < 0) return EQA_ERR_INVALID_ARG;
  hipLaunchKernelGGL(modified_gram_schmidt_kernel, dim3((B + kThreads - 1) / kThreads), dim3(kThreads), 0, (hipStream_t)stream, v, out, B);
  return launch_status();
}

int eqa_rigid_rows(const float* x, const float* R, const float* t, float* out, int M, int mode, void* stream) {
  if (M == 0) return EQA_OK;
  if (!x || !R || !out || M < 0 || (mode != 0 && mode != 1)) return EQA_ERR_INVALID_ARG;
  hipLaunchKernelGGL(rigid_rows_kernel, dim3((M + kThreads - 1) / kThreads), dim3(kThreads), 0, (hipStream_t)stream, x, R, t, out, M, mode);
  return launch_status();
}

int eqa_nbody_frame_fwd(const float* v, const float* t, const float* loc, const float* vel, float* R, float* cloc, float* cvel, int M,
                        void* stream) {
  if (M == 0) return EQA_OK;
  if (!v || !t || !loc || !vel || !R || !cloc || !cvel || M < 0) return EQA_ERR_INVALID_ARG;
  hipLaunchKernelGGL(nbody_frame_fwd_kernel, dim3((M + kThreads - 1) / kThreads), dim3(kThreads), 0, (hipStream_t)stream, v, t, loc, vel, R,
                     cloc, cvel, M);
  return launch_status();
}

int eqa_nbody_frame_bwd(const float* v, const float* t, const float* loc, const float* vel, const float* R, const float* gR,
                        const float* gcloc, const float* gcvel, float* gv, float* gt, float* gloc, float* gvel, int M, void* stream) {
  if (M == 0) return EQA_OK;
  if (M < 0 || (!gv && !gt && !gloc && !gvel)) return EQA_ERR_INVALID_ARG;
  if ((gt || gloc || gvel) && !R) return EQA_ERR_INVALID_ARG;                       // the frame the forward applied
  if (gv && (!v || (gcloc && (!loc || !t)) || (gcvel && !vel))) return EQA_ERR_INVALID_ARG;
  hipLaunchKernelGGL(nbody_frame_bwd_kernel, dim3((M + kThreads - 1) / kThreads), dim3(kThreads), 0, (hipStream_t)stream, v, t, loc, vel, R,
                     gR, gcloc, gcvel, gv, gt, gloc, gvel, M);
  return launch_status();
}

int eqa_rigid_rows_bwd(const float* x, const float* R, const float* g, float* gx, float* gR, int M, void* stream) {
  if (M == 0) return EQA_OK;
  if (!g || M < 0 || (!gx && !gR) || (gx && !R) || (gR && !x)) return EQA_ERR_INVALID_ARG;
  hipLaunchKernelGGL(rigid_rows_bwd_kernel, dim3((M + kThreads - 1) / kThreads), dim3(kThreads), 0, (hipStream_t)stream, x, R, g, gx, gR, M);
  return launch_status();
}

}  // extern "C"
