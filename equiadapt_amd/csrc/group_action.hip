// libeqa_hip.so, part 1 of 7 -- the group action on images: fused pad / rotate / flip / crop resampling (I5, I7, I8) and its
// backward.  (The nearest-neighbour action on masks, images and boxes: nearest_action.hip; crop + antialiased resize: crop_resize.hip.)
// HBM-bound gathers: coalesced global access, LDS-staged source tiles fed by global->LDS DMA, XCD-aware block->image
// mapping (each XCD's private L2 sees whole images).  C ABI: include/eqa_hip.h.  Design notes: HISTORY.md section 3.1.
#include "eqa_common.hpp"

namespace eqa {
int g_force_direct = 0;  // eqa_set_option key 0; read by nearest_action.hip too
}

namespace {


constexpr int kTile = 32;      // output tile edge (px): 256 threads x 4 px
constexpr int kBox = 47;       // staged source window edge: floor(31*sqrt(2)) + neighbour + floor/guard slack = 47
constexpr int kLdsStride = 47; // odd dword stride: the 8x4-lane gather pattern is bank-conflict-free at 0/90/180/270 deg
                               // 3 channels x 47 x 47 x 4 B = 26.5 KB -> 6 blocks per CU (160 KB LDS)
constexpr int kMaxMapG = 64;   // channel-map row cached in LDS
constexpr int kRowIters = (kBox + 3) / 4;  // window rows per wave (4 waves interleave rows)

struct ActionArgs {
  const float* src;
  float* dst;
  const int32_t* gidx;
  const float* theta;
  const int32_t* flags;
  const int32_t* chan_map;
  int E, G, n_out, B, C;
  int H, W, pad, Hp, Wp;
  int OH, OW, top, left;
  float half_w, half_h, step_x, step_y;
  int force_direct;
  int lds_rows;       // window rows the launch reserved LDS for (kBox unless the caller bounds the window: eqa_group_action_fwd_hint)
  // backward only
  const float* gout;  // dL/d(output), shape of dst
  float* gsrc;        // dL/d(source), shape of src, pre-zeroed (nullable)
  float* partial;     // per (output image, tile) partial of dL/d(angle [rad]) (nullable)
};

typedef const __attribute__((address_space(1))) void* gptr_t;
typedef __attribute__((address_space(3))) void* lptr_t;

// torch.linspace(-1, 1, steps) as the CPU kernel evaluates it (symmetric halves), fp32.
// Written select-style (one integer select, one fma-shaped op, one select) so it stays branch-free.
// Every multiply-add of the coordinate arithmetic is spelled out (contraction off, explicit fma) so that two evaluations of the same
// pixel are the same bits wherever they are inlined: the source window of a tile is derived from the sample points of its four
// corner pixels (tile_window).
__device__ __forceinline__ float lin_m1_p1(int idx, int steps, float step) {
#pragma clang fp contract(off)
  const bool lo = idx < (steps >> 1);
  const float k = (float)(lo ? idx : steps - 1 - idx);
  const float up = __builtin_fmaf(step, k, -1.0f), dn = __builtin_fmaf(-step, k, 1.0f);
  return lo ? up : dn;
}
// affine_grid: [xn, yn, 1] . theta^T ; grid_sample(align_corners=True): ((g + 1) / 2) * (size - 1).  Monotone in xn for a fixed yn
// and in yn for a fixed xn (every step is a correctly rounded monotone function of its varying operand).
// Which fp32 spelling of the three-term dot product is "the reference's" depends on the host: torch's CPU affine_grid is a batched
// matrix product, and the same torch build evaluates it as x * t0, fma(y, t1, .), + t2 on an 8-thread container and as
// (x * t0 + y * t1) + t2 with every operation rounded on the 128-thread host of the GPU box (tests/cpu_arith_probe.py, both outputs
// in profiles/r04/cpu_arith_probe.txt); a GPU run of the reference goes through yet another BLAS.  The kernel pins the second,
// plain IEEE form: together with the weights and the blend below (blend4, the same on both hosts) it reproduces the oracle of the
// GPU box bit for bit on most pixels of every element, and EVERY host's oracle bit for bit for the elements that are multiples
// of 90 degrees (tests/parity_scan.py, profiles/r04/parity_scan.txt).  Rounds 1-3 left the contraction to the compiler, which
// rounded t1 * y first and fused the final multiply into the fractional part: 1.5e-4 from the oracle on white noise.
__device__ __forceinline__ void sample_point(float t0, float t1, float t2, float t3, float t4, float t5, float xn, float yn,
                                             float half_w, float half_h, float& ix, float& iy) {
#pragma clang fp contract(off)
  ix = (((t0 * xn + t1 * yn) + t2) + 1.0f) * half_w;
  iy = (((t3 * xn + t4 * yn) + t5) + 1.0f) * half_h;
}
// F.grid_sample's CPU kernel blends the four neighbours as one multiply and three fused multiply-adds in the order nw, ne, sw, se
__device__ __forceinline__ float blend4(float nw, float ne, float sw, float se, float w_nw, float w_ne, float w_sw, float w_se) {
#pragma clang fp contract(off)
  return __builtin_fmaf(se, w_se, __builtin_fmaf(sw, w_sw, __builtin_fmaf(ne, w_ne, nw * w_nw)));
}


// ablation switches for tools/ablate.sh (never set in the product build)
#ifndef EQA_ABL_BOXGUARD
#define EQA_ABL_BOXGUARD 0.0f   // -DEQA_ABL_BOXGUARD=1e-3f: the guarded window of rounds 1-3
#endif
#ifdef EQA_ABL_NOLOAD
#define EQA_ABL_YB(yb) (a.force_direct == 12345 ? (yb) : 0)
#else
#define EQA_ABL_YB(yb) (yb)
#endif
#ifdef EQA_ABL_NOSTORE
#define EQA_ABL_STORE_OK(v) ((v) == 123.456f)
#else
#define EQA_ABL_STORE_OK(v) true
#endif
#ifndef EQA_ACTION_WAVES
#define EQA_ACTION_WAVES 1
#endif
#ifndef EQA_FORCE_CH
#define EQA_FORCE_CH 0
#endif

// Which (image, tile) does this block work on?  Full groups of 8 images: image n = 8 * bz + xcd, tile (blockIdx.x >> 3, blockIdx.y)
// -- an image per XCD.  The last, ragged group (r = n_out - 8 * bz < 8 images; the whole job when n_out < 8: config 5 runs B = 4)
// would leave 8 - r XCDs without work that way, so its r * tiles work items are dealt to the 8 XCDs in contiguous runs instead
// (an XCD still sees neighbouring tiles of one image: the overlapping source windows keep hitting in its L2); the 8 * tiles blocks
// of the group's grid slice beyond those exit at once.  Same tile, same arithmetic: results are bit-identical either way.
// The two scalar divisions are paid by the blocks of a ragged group only.
__device__ __forceinline__ bool block_tile(const int n_out, const int bz, int& n, int& tx, int& ty) {
  const int xcd = (int)(blockIdx.x & (kXcd - 1));
  tx = (int)(blockIdx.x >> 3);
  ty = (int)blockIdx.y;
  const int first = bz * kXcd, r = n_out - first;
  if (r >= kXcd) {
    n = first + xcd;
    return true;
  }
  const int tiles_x = (int)(gridDim.x >> 3), tiles = tiles_x * (int)gridDim.y;
  const int per = (r * tiles + kXcd - 1) >> 3;
  const int slot = ty * tiles_x + tx;
  const int w = xcd * per + slot;
  if (slot >= per || w >= r * tiles) return false;
  const int img = w / tiles, t = w - img * tiles;
  ty = t / tiles_x;
  tx = t - ty * tiles_x;
  n = first + img;
  return true;
}

// ------------------------------------------------------------------------------------------------
// The resampling rules of the bilinear family, each stated once: every kernel below is built from these functions (small structs
// that dissolve into registers), which is what makes the kernels' results the same bits.
// The group element of output image n: its index, the source image it acts on, its sampling matrix and flip bits.
struct Element {
  int e, b;
  float t0, t1, t2, t3, t4, t5;
  int fl;  // EQA_FLIP_* bits (kept as the word and tested where used: one scalar register, not a lane mask per bit)
  __device__ __forceinline__ bool flip_dst() const { return (fl & EQA_FLIP_DST) != 0; }
  __device__ __forceinline__ bool flip_src() const { return (fl & EQA_FLIP_SRC) != 0; }
};
__device__ __forceinline__ Element load_element(const ActionArgs& a, const int n) {
  Element el;
  if (a.gidx) {
    el.e = a.gidx[n];
    el.b = n;
  } else {  // orbit mode: element-major output, n = e * B + b
    el.e = n / a.B;
    el.b = n - el.e * a.B;
  }
  el.e = min(max(el.e, 0), a.E - 1);
  el.fl = a.flags ? a.flags[el.e] : 0;
  const float* th = a.theta + el.e * 6;
  el.t0 = th[0]; el.t1 = th[1]; el.t2 = th[2]; el.t3 = th[3]; el.t4 = th[4]; el.t5 = th[5];
  return el;
}

// frame column of output column j (post-flip: hflip of the rotated frame, then the crop)
__device__ __forceinline__ int frame_x(const ActionArgs& a, const Element& el, const int j) {
  return el.flip_dst() ? (a.Wp - 1 - (a.left + j)) : (a.left + j);
}
// source column of frame column fx: optional pre-flip, edge-replicated pad
__device__ __forceinline__ int src_col(const ActionArgs& a, const Element& el, const int fx) {
  return min(max((el.flip_src() ? (a.Wp - 1 - fx) : fx) - a.pad, 0), a.W - 1);
}
// frame pixel -> source offset (edge-replicated pad, optional pre-flip); `inside` = not zero padding
__device__ __forceinline__ int src_offset(const ActionArgs& a, const Element& el, const int fy, const int fx, bool& inside) {
  inside = ((unsigned)fx < (unsigned)a.Wp) && ((unsigned)fy < (unsigned)a.Hp);
  const int sy = min(max(fy - a.pad, 0), a.H - 1);
  return sy * a.W + src_col(a, el, fx);
}

// ---- source window of a tile = the bounding box of the north-west neighbours its pixels have, + 1 for the south-east ones.
// The sample point is monotone along a row and along a column of the tile (sample_point), so its extremes over the tile are
// those of the four corner pixels -- evaluated here with the per-pixel arithmetic itself, which makes the box EXACT.  Rounds 1-3
// bounded it with the corners of the real-valued map and a 1e-3 px guard for the rounding difference.  For elements whose
// sample points are whole pixels (every multiple of 90 degrees: all of C4 / D4, half of C8) that guard always added the column
// left of the tile, which lies in the PREVIOUS 128-byte line: three line requests per window row instead of two.  The copy model
// (tools/micro/pc_tile.hip, window 35 vs 33) prices that at 7 % on 224 x 224 planes and 12 % on 1024 x 1024 ones; the exact box
// has the extra column only where rounding really puts a sample point below its pixel (a fifth of the tiles).
struct Window {
  int x_lo, y_lo, bw, bh;  // north-west corner (frame pixels, >= -1) and size
  __device__ __forceinline__ int x_hi() const { return x_lo + bw - 1; }
  __device__ __forceinline__ int y_hi() const { return y_lo + bh - 1; }
};
__device__ __forceinline__ Window tile_window(const ActionArgs& a, const Element& el, const int i0, const int j0, const int i1,
                                              const int j1) {
  const float xa = lin_m1_p1(frame_x(a, el, j0), a.Wp, a.step_x), xb = lin_m1_p1(frame_x(a, el, j1), a.Wp, a.step_x);
  const float ya = lin_m1_p1(a.top + i0, a.Hp, a.step_y), yb = lin_m1_p1(a.top + i1, a.Hp, a.step_y);
  float cx[4], cy[4];
  sample_point(el.t0, el.t1, el.t2, el.t3, el.t4, el.t5, xa, ya, a.half_w, a.half_h, cx[0], cy[0]);
  sample_point(el.t0, el.t1, el.t2, el.t3, el.t4, el.t5, xb, ya, a.half_w, a.half_h, cx[1], cy[1]);
  sample_point(el.t0, el.t1, el.t2, el.t3, el.t4, el.t5, xa, yb, a.half_w, a.half_h, cx[2], cy[2]);
  sample_point(el.t0, el.t1, el.t2, el.t3, el.t4, el.t5, xb, yb, a.half_w, a.half_h, cx[3], cy[3]);
  const float minx_f = floorf(fminf(fminf(cx[0], cx[1]), fminf(cx[2], cx[3])) - EQA_ABL_BOXGUARD);
  const float maxx_f = floorf(fmaxf(fmaxf(cx[0], cx[1]), fmaxf(cx[2], cx[3])) + EQA_ABL_BOXGUARD);
  const float miny_f = floorf(fminf(fminf(cy[0], cy[1]), fminf(cy[2], cy[3])) - EQA_ABL_BOXGUARD);
  const float maxy_f = floorf(fmaxf(fmaxf(cy[0], cy[1]), fmaxf(cy[2], cy[3])) + EQA_ABL_BOXGUARD);
  Window w;
  // keep at most one ring of off-frame (zero) pixels; a tile entirely off the frame keeps a 2 x 2 window at the frame's edge
  w.x_lo = (int)fminf(fmaxf(minx_f, -1.0f), (float)(a.Wp - 1));
  w.y_lo = (int)fminf(fmaxf(miny_f, -1.0f), (float)(a.Hp - 1));
  // at least 2x2 so the clamped neighbour reads of fully off-frame pixels stay inside staged data
  const int x_hi = max((int)fminf(fmaxf(maxx_f, -1.0f), (float)(a.Wp - 1)) + 1, w.x_lo + 1);
  const int y_hi = max((int)fminf(fmaxf(maxy_f, -1.0f), (float)(a.Hp - 1)) + 1, w.y_lo + 1);
  w.bw = x_hi - w.x_lo + 1;
  w.bh = y_hi - w.y_lo + 1;
  return w;
}

// (frame column, frame row) -> sample point as an affine map p = A o + b
struct SamplingMap { float a00, a01, a10, a11, b0, b1; };
__device__ __forceinline__ SamplingMap sampling_map(const ActionArgs& a, const Element& el) {
  SamplingMap s;
  s.a00 = a.half_w * el.t0 * a.step_x; s.a01 = a.half_w * el.t1 * a.step_y; s.b0 = a.half_w * ((el.t2 - el.t0 - el.t1) + 1.0f);
  s.a10 = a.half_h * el.t3 * a.step_x; s.a11 = a.half_h * el.t4 * a.step_y; s.b1 = a.half_h * ((el.t5 - el.t3 - el.t4) + 1.0f);
  return s;
}
// ... and its inverse o = M (p - b), once per element; !ok: a singular map (or -DEQA_ABL_NOMASK), every lane is kept
struct SamplingInverse { float m00, m01, m10, m11, b0, b1; bool ok; };
__device__ __forceinline__ SamplingInverse sampling_inverse(const ActionArgs& a, const Element& el) {
  SamplingInverse inv = {0.0f, 0.0f, 0.0f, 0.0f, 0.0f, 0.0f, false};
#ifndef EQA_ABL_NOMASK
  const SamplingMap s = sampling_map(a, el);
  inv.b0 = s.b0; inv.b1 = s.b1;
  const float det = s.a00 * s.a11 - s.a01 * s.a10;
  if (fabsf(det) > 1e-12f) {  // (uniform)
    const float rdet = 1.0f / det;
    inv.m00 = s.a11 * rdet; inv.m01 = -s.a01 * rdet; inv.m10 = -s.a10 * rdet; inv.m11 = s.a00 * rdet;
    inv.ok = true;
  }
#endif
  return inv;
}

// Staging role of a lane: window column `lane` of every window row (the 4 waves interleave the rows).
// Which window pixels does the tile actually sample?  The window is the bounding BOX of the tile's pre-image; for an element
// that is not a multiple of 90 degrees the pre-image is a rotated square and fills about half of it (45 degrees: 1250 of the
// 47 x 47 = 2209 pixels).  Requesting the rest costs L2 -> LDS traffic and cache-line requests for nothing: the copy model
// (tools/micro/pc_tile.hip, profiles/r04/pc_tile.txt) moves 47-wide windows at 4.81 TB/s and the same windows with the lanes
// outside the 45-degree diamond switched off at 5.43.  A frame pixel p is a neighbour of some output pixel o of the tile iff o's
// sample point lies within one pixel of p; the sampling map is affine, o = M (p - b), so p is wanted iff M (p - b) lies in the
// tile's rectangle grown by the pre-image of that unit square (the row L1 norms of M) -- plus a quarter pixel of slack, three
// orders of magnitude above the rounding difference between this evaluation and the per-pixel one (sample_pixel).  Per lane (window
// column) the two coordinates are affine in the row: two adds and two compares per DMA row.
struct WindowLane {
  bool col_ok, col_inside;  // the window has this column; it is a frame column (not zero padding)
  unsigned col_off;         // its byte offset inside a source row
  float mask_uj, mask_ui, mask_dj, mask_di, mask_hj, mask_hi;  // pre-image test of window row y: |u + d * y| <= h, both axes
};
__device__ __forceinline__ WindowLane lane_mask(const ActionArgs& a, const Element& el, const SamplingInverse& inv, const Window& w,
                                                const int lane, const int i0, const int j0, const int i1, const int j1) {
  WindowLane wl;
  const int col_fx = w.x_lo + lane;
  wl.col_ok = lane < w.bw;
  wl.col_inside = (unsigned)col_fx < (unsigned)a.Wp;
  wl.col_off = (unsigned)src_col(a, el, col_fx) * 4u;
  wl.mask_uj = 0.0f; wl.mask_ui = 0.0f; wl.mask_dj = inv.m01; wl.mask_di = inv.m11;
  wl.mask_hj = __builtin_inff(); wl.mask_hi = __builtin_inff();
  if (inv.ok) {
    const float jfa = (float)frame_x(a, el, j0), jfb = (float)frame_x(a, el, j1);
    const float px = (float)col_fx - inv.b0, py = (float)w.y_lo - inv.b1;
    wl.mask_uj = (inv.m00 * px + inv.m01 * py) - 0.5f * (jfa + jfb);
    wl.mask_ui = (inv.m10 * px + inv.m11 * py) - ((float)a.top + 0.5f * (float)(i0 + i1));
    wl.mask_hj = 0.5f * fabsf(jfb - jfa) + fabsf(inv.m00) + fabsf(inv.m01) + 0.25f;
    wl.mask_hi = 0.5f * (float)(i1 - i0) + fabsf(inv.m10) + fabsf(inv.m11) + 0.25f;
  }
  return wl;
}

// Stage one window with direct-to-LDS DMA (global_load_lds_dword): each instruction moves one window-row
// segment L2/HBM -> LDS.  LDS address = M0 (row base, per channel) + lane*4; global address = plane (SGPR
// pair, saddr form) + [clamped row offset (SALU) + clamped/flipped column offset] (one VGPR add per row, shared
// by the CH channels).  No staging VGPRs, no ds_write, no select, no 64-bit address VALU.
// Off-frame rows/columns (padding_mode="zeros") are zero-filled afterwards by the lanes/rows that own them (zero_fill_window);
// those never issue a DMA, so there is no ordering problem.
// Inline asm because hipcc will not pick the saddr form for the builtin.  It does not count these loads:
// the caller's s_waitcnt vmcnt(0) does.  M0 (compiler-reserved) is saved once before the row loop and restored
// after it; every statement that reads M0 writes it first (cdna guide 5.7).
// LDS layout [window row][channel][column] at `win`: one M0 write per row serves all CH channels, each DMA adding its
// channel's row offset through the instruction's immediate (which shifts the global address too, so the plane
// base handed to the DMA is pre-biased by -cc*kRowB).
template <int CH>
__device__ __forceinline__ void stage_window_rows(const ActionArgs& a, float* const win, const Window& w, const WindowLane& wl,
                                                  const int wave, const float* const (&planes)[CH]) {
  constexpr int kRowB = kLdsStride * 4;  // bytes of one channel's row
  if (wl.col_ok && wl.col_inside) {
    // window rows inside the frame: [ya, yb); this wave takes ya + ((wave - ya) mod 4), +4, ...
    const int ya = max(-w.y_lo, 0), yb = min(w.bh, a.Hp - w.y_lo);
    const char* p0 = reinterpret_cast<const char*>(planes[0]);
    const char* p1 = reinterpret_cast<const char*>(planes[CH > 1 ? 1 : 0]) - kRowB;
    const char* p2 = reinterpret_cast<const char*>(planes[CH > 2 ? 2 : 0]) - 2 * kRowB;
    unsigned keep;
    asm volatile("s_mov_b32 %0, m0" : "=s"(keep));
    const int y_first = ya + ((wave - ya) & 3);
    float vj = wl.mask_uj + wl.mask_dj * (float)y_first, vi = wl.mask_ui + wl.mask_di * (float)y_first;
    const float sj = 4.0f * wl.mask_dj, si = 4.0f * wl.mask_di;
#pragma unroll 1
    for (int y = y_first; y < EQA_ABL_YB(yb); y += 4, vj += sj, vi += si) {
      const int fy = w.y_lo + y;
      const unsigned voff = (unsigned)(min(max(fy - a.pad, 0), a.H - 1) * a.W) * 4u + wl.col_off;
      const unsigned lrow = (unsigned)(uintptr_t)(lptr_t)(win + y * (CH * kLdsStride));
      if (!(fabsf(vj) <= wl.mask_hj && fabsf(vi) <= wl.mask_hi)) continue;   // this lane's pixel of the row is outside the tile's pre-image
      if (CH == 1) {
        asm volatile("s_mov_b32 m0, %[l]\n\ts_nop 0\n\tglobal_load_lds_dword %[v], %[p0]"
                     :: [v] "v"(voff), [l] "s"(lrow), [p0] "s"(p0) : "memory");
      } else if (CH == 2) {
        asm volatile("s_mov_b32 m0, %[l]\n\ts_nop 0\n\tglobal_load_lds_dword %[v], %[p0]\n\t"
                     "global_load_lds_dword %[v], %[p1] offset:%[o1]"
                     :: [v] "v"(voff), [l] "s"(lrow), [p0] "s"(p0), [p1] "s"(p1), [o1] "i"(kRowB) : "memory");
      } else {
        asm volatile("s_mov_b32 m0, %[l]\n\ts_nop 0\n\tglobal_load_lds_dword %[v], %[p0]\n\t"
                     "global_load_lds_dword %[v], %[p1] offset:%[o1]\n\t"
                     "global_load_lds_dword %[v], %[p2] offset:%[o2]"
                     :: [v] "v"(voff), [l] "s"(lrow), [p0] "s"(p0), [p1] "s"(p1), [p2] "s"(p2), [o1] "i"(kRowB),
                        [o2] "i"(2 * kRowB) : "memory");
      }
    }
    asm volatile("s_mov_b32 m0, %0" :: "s"(keep));
  }
}
// rare: tiles touching the zero ring of an unpadded frame (`any_zero`: window_any_zero, evaluated once by a caller that stages often)
__device__ __forceinline__ bool window_any_zero(const ActionArgs& a, const Window& w) {
  return (w.x_lo < 0) || (w.y_lo < 0) || (w.x_hi() > a.Wp - 1) || (w.y_hi() > a.Hp - 1);
}
template <int CH>
__device__ __forceinline__ void zero_fill_window(const ActionArgs& a, float* const win, const Window& w, const WindowLane& wl,
                                                 const bool any_zero, const int wave, const int lane) {
  if (any_zero && wl.col_ok) {
#pragma unroll 1
    for (int y = wave; y < w.bh; y += 4) {
      if (!(wl.col_inside && ((unsigned)(w.y_lo + y) < (unsigned)a.Hp))) {
#pragma unroll
        for (int cc = 0; cc < CH; ++cc) win[(y * CH + cc) * kLdsStride + lane] = 0.0f;
      }
    }
  }
}

// The sample point of output pixel (pi, pj) and what every kernel derives from it the same way: its floor (the north-west
// neighbour), the fractional parts, and the neighbour's frame coordinates with the range test of padding_mode="zeros".
struct PixelSample {
  float xn, yn;    // normalised frame coordinates of the output pixel
  float ix, iy;    // sample point (frame pixels)
  float xf, yf;    // its floor
  float wx1, wy1;  // fractional parts
  int xi, yi;      // north-west neighbour, -1 where that axis is out of range
  bool live;       // false: all four neighbours are off the frame -> exact zero
};
__device__ __forceinline__ PixelSample sample_pixel(const ActionArgs& a, const Element& el, const int pi, const int pj) {
  PixelSample s;
#ifdef EQA_ABL_CHEAPSETUP  // ablation (tools/ablate.sh): what a kernel costs without the per-pixel coordinate arithmetic (wrong pixels:
                           // every output pixel samples the centre of its own frame pixel's south-east quad)
  s.xn = 0.0f; s.yn = 0.0f;
  s.xi = min(frame_x(a, el, pj), a.Wp - 2); s.yi = min(a.top + pi, a.Hp - 2);
  s.xf = (float)s.xi; s.yf = (float)s.yi;
  s.wx1 = 0.5f; s.wy1 = 0.5f;
  s.ix = s.xf + 0.5f; s.iy = s.yf + 0.5f;
  s.live = true;
  return s;
#endif
  // affine_grid: [xn, yn, 1] . theta^T ; grid_sample(align_corners=True): ((g + 1) / 2) * (size - 1)
  s.yn = lin_m1_p1(a.top + pi, a.Hp, a.step_y);
  s.xn = lin_m1_p1(frame_x(a, el, pj), a.Wp, a.step_x);
  sample_point(el.t0, el.t1, el.t2, el.t3, el.t4, el.t5, s.xn, s.yn, a.half_w, a.half_h, s.ix, s.iy);
  s.xf = floorf(s.ix); s.yf = floorf(s.iy);
  s.wx1 = s.ix - s.xf; s.wy1 = s.iy - s.yf;
  // neighbours entirely off the frame contribute zero (grid_sample padding_mode="zeros")
  const bool xin = (s.xf >= -1.0f) && (s.xf <= (float)(a.Wp - 1));
  const bool yin = (s.yf >= -1.0f) && (s.yf <= (float)(a.Hp - 1));
  s.live = xin && yin;
  s.xi = xin ? (int)s.xf : -1;
  s.yi = yin ? (int)s.yf : -1;
  return s;
}
// validation build (tools/fuzz_r03.py --lib): a stored pixel whose neighbours are not in the corner-derived window
__device__ __forceinline__ void check_window(const ActionArgs& a, const Window& w, const bool live, const int xi, const int yi,
                                             const int pi, const int pj) {
#ifdef EQA_CHECK_WINDOW
  if (live && pi < a.OH && pj < a.OW && (xi < w.x_lo || xi + 1 > w.x_hi() || yi < w.y_lo || yi + 1 > w.y_hi())) __builtin_trap();
#endif
}

// Direct-gather fallback of the staged kernels (window too large for LDS, or forced): the same arithmetic from global memory.
// Its callers run it in ROLLED loops on purpose: it must not inflate the register budget of the LDS path it shares a kernel with.
// (dynamic k: read the per-pixel state through selects, not indexed registers)
template <typename T>
__device__ __forceinline__ T pick4(const T (&v)[4], const int k) {
  const T v0 = v[0], v1 = v[1], v2 = v[2];  // (read first, then one select per step: no conditional reads, no branch tree)
  T r = v[3];
  r = k == 2 ? v2 : r;
  r = k == 1 ? v1 : r;
  r = k == 0 ? v0 : r;
  return r;
}
template <int CH>
__device__ __forceinline__ const float* pick_plane(const float* const (&planes)[CH], const int cc) {
  const float* const both[4] = {planes[0], planes[CH > 1 ? 1 : 0], planes[CH > 2 ? 2 : 0], planes[CH > 2 ? 2 : 0]};
  return pick4(both, cc);
}
// the four neighbours of north-west frame pixel (gx, gy), zero where they are off the frame
__device__ __forceinline__ void load4_direct(const float* plane, const ActionArgs& a, const Element& el, const int gx, const int gy,
                                             float& nw, float& ne, float& sw, float& se) {
  bool in00, in01, in10, in11;
  const int o00 = src_offset(a, el, gy, gx, in00), o01 = src_offset(a, el, gy, gx + 1, in01);
  const int o10 = src_offset(a, el, gy + 1, gx, in10), o11 = src_offset(a, el, gy + 1, gx + 1, in11);
  const float v00 = plane[o00], v01 = plane[o01], v10 = plane[o10], v11 = plane[o11];
  nw = in00 ? v00 : 0.0f; ne = in01 ? v01 : 0.0f; sw = in10 ? v10 : 0.0f; se = in11 ? v11 : 0.0f;
}
__device__ __forceinline__ float gather4_direct(const float* plane, const ActionArgs& a, const Element& el, const int gx, const int gy,
                                                const float w_nw, const float w_ne, const float w_sw, const float w_se, const bool live) {
  float nw, ne, sw, se;
  load4_direct(plane, a, el, gx, gy, nw, ne, sw, se);
  const float v = blend4(nw, ne, sw, se, w_nw, w_ne, w_sw, w_se);
  return live ? v : 0.0f;
}

// One block = one 32x32 output tile of one output image, all channels, CH channels per LDS stage.
//   grid = (8 * tiles_x, tiles_y, ceil(n_out / 8)):  blockIdx.x & 7 is the XCD the dispatcher deals the block
//   to, so each XCD works on whole images (n = 8*z + xcd) and the overlapping source windows of neighbouring
//   tiles hit in that XCD's private L2 (block_tile above; a ragged last group is split by tiles instead).
// Thread t owns 4 consecutive pixels of tile row t/8 (float4 stores, 128 B per 8 lanes).
// Sampling arithmetic = torch affine_grid + grid_sample(bilinear, zeros, align_corners=True) on the
// (Hp, Wp) frame, the frame itself being the edge-replicated (pad) and optionally h-flipped source.
// `bz` = the block's image-group index (blockIdx.z of a single job; blockIdx.z minus the first job's groups in a pair launch).
// MODE 0: the action itself (dst).  MODE 1: its derivative with respect to the rotation angle contracted with an output gradient
// (a.gout), one partial sum per (output image, tile) in a.partial -- the training step's angle gradient, with the same staged window
// (the derivative samples the same four neighbours the forward blends): round 3's group_action_bwd_kernel<1, false> gathered them
// from global memory, 119-169 us per 256 images; it remains the fallback for forced-direct runs and the reference of the tests.
template <int CH, bool VEC, int MODE = 0>
__device__ __forceinline__ void group_action_body(const ActionArgs& a, const int bz) {
  extern __shared__ __attribute__((aligned(16))) float smem[];

  const int tid = threadIdx.x;
  const int lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);  // provably uniform: row math stays on the SALU
  int n, tile_x, tile_y;
  if (!block_tile(a.n_out, bz, n, tile_x, tile_y)) return;

  const Element el = load_element(a, n);
#ifndef EQA_ABL_ROWWALK
  // Quarter turns read source ROWS along output COLUMNS: the blocks of an image then walk its tiles column by column, so that the
  // blocks in flight together read whole source rows (DRAM pages) -- rows of output tiles read 128-byte pieces of 32 rows 4 KB
  // apart on config 5's planes.  tools/micro/tile_shape.hip: 0.592 -> 0.629 of the HBM peak on 1024 x 1024 planes, no difference on
  // 224 x 224 ones; the kernel (profiles/r04/kbench_exact_window.txt): a batch of quarter turns 171 -> 157 us per 32 frames of
  // config 5, mixed batches and the metric's 224 x 224 frames unchanged.  (Any bijection of the image's tiles serves here.)
  if (fabsf(el.t1) > fabsf(el.t0) && gridDim.y > 1) {
    const int tiles_x = (int)(gridDim.x >> 3), tiles_y = (int)gridDim.y;
    const int lin = tile_y * tiles_x + tile_x;
    tile_x = lin / tiles_y;
    tile_y = lin - tile_x * tiles_y;
  }
#endif
  const int j0 = tile_x * kTile, i0 = tile_y * kTile;
  const int i1 = min(i0 + kTile - 1, a.OH - 1), j1 = min(j0 + kTile - 1, a.OW - 1);
  const Window w = tile_window(a, el, i0, j0, i1, j1);
  const int bw = w.bw, bh = w.bh;
  const bool use_lds = (bw <= kBox) && (bh <= a.lds_rows) && !a.force_direct;

  // ---- per-thread output pixels
  const int r = tid >> 3, q = tid & 7;
  const int i = i0 + r, jb = j0 + 4 * q;
  int lidx[4];         // LDS path: index of the north-west neighbour inside the staged window
  int gx0[4], gy0[4];  // direct path: frame coords of the north-west neighbour
  bool live[4];        // false: all four neighbours are off the frame -> exact zero
  float w00[4], w01[4], w10[4], w11[4];
  auto pixel_setup = [&](int pi, int pj) {
#pragma unroll
    for (int k = 0; k < 4; ++k) {
      const PixelSample s = sample_pixel(a, el, pi, pj + k);
      live[k] = s.live;
      gx0[k] = s.xi;
      gy0[k] = s.yi;
      // (pixels of a partial tile beyond OW/OH are computed but never stored: keep their reads in the window)
      const int lx = min(max(s.xi - w.x_lo, 0), bw - 2), ly = min(max(s.yi - w.y_lo, 0), bh - 2);
      check_window(a, w, s.live, s.xi, s.yi, pi, pj + k);
      lidx[k] = ly * (CH * kLdsStride) + lx;
      if (MODE == 0) {
        const float wx0 = 1.0f - s.wx1, wy0 = 1.0f - s.wy1;
        w00[k] = wy0 * wx0;      // nw
        w01[k] = wy0 * s.wx1;    // ne
        w10[k] = s.wy1 * wx0;    // sw
        w11[k] = s.wy1 * s.wx1;  // se
      } else {
        // the angle derivative needs the fractional parts themselves and the lever arm of the sample point about the frame
        // centre (ds/dphi = (-(s_y - c_y), s_x - c_x) per radian; see group_action_bwd_kernel)
        live[k] = live[k] && (pi < a.OH) && (pj + k < a.OW);
        w00[k] = s.wx1;
        w01[k] = s.wy1;
        w10[k] = -(s.iy - a.half_h);
        w11[k] = s.ix - a.half_w;
      }
    }
  };

  // the element's channel-map row (regular features) goes to LDS once
  int* s_cmap = reinterpret_cast<int*>(smem + CH * a.lds_rows * kLdsStride);
  const bool has_cmap = a.chan_map != nullptr;
  if (has_cmap) {
    if (tid < a.G) s_cmap[tid] = a.chan_map[el.e * a.G + tid];
    __syncthreads();
  }

  const WindowLane wl = lane_mask(a, el, sampling_inverse(a, el), w, lane, i0, j0, i1, j1);
  const bool any_zero = window_any_zero(a, w);
  const unsigned src_plane = (unsigned)(a.H * a.W);
  const unsigned dst_plane = (unsigned)(a.OH * a.OW);
  const bool row_ok = i < a.OH;
  float* const dst_img = a.dst + (size_t)n * ((size_t)a.C * dst_plane);

  // plane base pointers of one stage (wave-uniform; readfirstlane makes that provable)
  const float* const src_img = a.src + (size_t)el.b * ((size_t)a.C * src_plane);  // one 64-bit multiply per block
  auto stage_planes = [&](int c0, const float* (&planes)[CH]) {
#pragma unroll
    for (int cc = 0; cc < CH; ++cc) {
      const int c = min(c0 + cc, a.C - 1);
      const int cs = __builtin_amdgcn_readfirstlane(has_cmap ? (c / a.G) * a.G + s_cmap[c % a.G] : c);
      planes[cc] = src_img + (unsigned)cs * (unsigned)src_plane;  // C*H*W < 2^30 (checked on the host)
    }
  };
  auto stage_issue = [&](const float* const (&planes)[CH]) {
    stage_window_rows<CH>(a, smem, w, wl, wave, planes);
    zero_fill_window<CH>(a, smem, w, wl, any_zero, wave, lane);
  };
  auto stage_wait = [&]() {
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");  // this wave's DMA has landed in LDS
    __syncthreads();                                   // ... and so has every other wave's
  };

  const float* planes[CH];
  stage_planes(0, planes);
  if (use_lds) stage_issue(planes);
  {
    // the per-pixel setup does not depend on the loads: it runs while the DMA is in flight.  The empty asm makes
    // its inputs opaque here so the compiler cannot hoist the arithmetic above the DMA issue.
    int pi = i, pj = jb;
    asm volatile("" : "+v"(pi), "+v"(pj));
    pixel_setup(pi, pj);
  }

  float angle_sum = 0.0f;   // MODE 1
  for (int c0 = 0; c0 < a.C; c0 += CH) {
    float acc[CH][4];
    if (MODE == 1) {
      const float* const gout_img = a.gout + (size_t)n * ((size_t)a.C * dst_plane);
      if (!use_lds) {
        // window too large for LDS (never for a rotation) or forced: everything from global memory, pixel by pixel in ROLLED loops
        // with the coordinates recomputed per pixel -- slow and rare, and it must not inflate the staged path's register budget
        if (c0 > 0) stage_planes(c0, planes);
#pragma unroll 1
        for (int cc = 0; cc < CH; ++cc) {
          if (c0 + cc >= a.C) break;
          const float* pl = pick_plane<CH>(planes, cc);
#pragma unroll 1
          for (int k = 0; k < 4; ++k) {
            const PixelSample s = sample_pixel(a, el, i, jb + k);
            const bool lv = s.live && row_ok && (jb + k < a.OW);
            float nw, ne, sw, se;
            load4_direct(pl, a, el, s.xi, s.yi, nw, ne, sw, se);
            const float g = gout_img[(unsigned)(c0 + cc) * dst_plane + (lv ? (unsigned)(i * a.OW + jb + k) : 0u)];
            const float wx0 = 1.0f - s.wx1, wy0 = 1.0f - s.wy1;
            const float dix = wy0 * (ne - nw) + s.wy1 * (se - sw), diy = wx0 * (sw - nw) + s.wx1 * (se - ne);
            angle_sum += lv ? g * (dix * (-(s.iy - a.half_h)) + diy * (s.ix - a.half_w)) : 0.0f;
          }
        }
        continue;
      }
      // the output gradient of this stage's channels (a dead pixel reads the plane's first value), requested before the wait
      // for the window so that both are in flight together; same order of additions as group_action_bwd_kernel<1, false>
      float gv[CH][4];
#pragma unroll
      for (int cc = 0; cc < CH; ++cc) {
        const unsigned cpl = (unsigned)min(c0 + cc, a.C - 1) * dst_plane;
#pragma unroll
        for (int k = 0; k < 4; ++k) gv[cc][k] = gout_img[cpl + (live[k] ? (unsigned)(i * a.OW + jb + k) : 0u)];
      }
      if (c0 > 0) {
        stage_planes(c0, planes);
        __syncthreads();
        stage_issue(planes);
      }
      stage_wait();
#pragma unroll
      for (int cc = 0; cc < CH; ++cc) {
        const float* s = smem + cc * kLdsStride;
#pragma unroll
        for (int k = 0; k < 4; ++k) {
          const float nw = s[lidx[k]], ne = s[lidx[k] + 1];
          const float sw = s[lidx[k] + CH * kLdsStride], se = s[lidx[k] + CH * kLdsStride + 1];
          const float wx1 = w00[k], wy1 = w01[k];
          const float wx0 = 1.0f - wx1, wy0 = 1.0f - wy1;
          const float dix = wy0 * (ne - nw) + wy1 * (se - sw);
          const float diy = wx0 * (sw - nw) + wx1 * (se - ne);
          // (a dead pixel contributes nothing -- a select, not g = 0: a non-finite neighbour must not turn 0 * inf into NaN)
          if (c0 + cc < a.C) angle_sum += live[k] ? gv[cc][k] * (dix * w10[k] + diy * w11[k]) : 0.0f;
        }
      }
      continue;
    }
    if (use_lds) {
      if (c0 > 0) {
        stage_planes(c0, planes);
        __syncthreads();  // previous stage's gathers are done with the window
        stage_issue(planes);
      }
      stage_wait();
#pragma unroll
      for (int cc = 0; cc < CH; ++cc) {
        const float* s = smem + cc * kLdsStride;
#pragma unroll
        for (int k = 0; k < 4; ++k) {
          const float nw = s[lidx[k]], ne = s[lidx[k] + 1];
          const float sw = s[lidx[k] + CH * kLdsStride], se = s[lidx[k] + CH * kLdsStride + 1];
          const float v = blend4(nw, ne, sw, se, w00[k], w01[k], w10[k], w11[k]);
          acc[cc][k] = live[k] ? v : 0.0f;
        }
      }
    } else {
      // direct gather (window too large for LDS, or forced): rare fallback, same arithmetic.  Rolled loops on
      // purpose: it must not inflate the register budget of the LDS path it shares the kernel with.
      if (c0 > 0) stage_planes(c0, planes);
#pragma unroll
      for (int cc = 0; cc < CH; ++cc) {
#pragma unroll
        for (int k = 0; k < 4; ++k) acc[cc][k] = 0.0f;
      }
#pragma unroll 1
      for (int t = 0; t < 4 * CH; ++t) {
        const int cc = t >> 2, k = t & 3;
        const float v = gather4_direct(pick_plane<CH>(planes, cc), a, el, pick4(gx0, k), pick4(gy0, k), pick4(w00, k), pick4(w01, k),
                                       pick4(w10, k), pick4(w11, k), pick4(live, k));
#pragma unroll
        for (int c2 = 0; c2 < CH; ++c2) {
#pragma unroll
          for (int k2 = 0; k2 < 4; ++k2)
            if (c2 == cc && k2 == k) acc[c2][k2] = v;
        }
      }
    }
    if (row_ok) {
#pragma unroll
      for (int cc = 0; cc < CH; ++cc) {
        if (c0 + cc < a.C) {
          float* o = dst_img + (unsigned)(c0 + cc) * dst_plane + (unsigned)(i * a.OW + jb);
          if (VEC) {  // OW % 4 == 0 and jb % 4 == 0: a pixel quad is entirely inside or entirely outside the row
            if (jb < a.OW && EQA_ABL_STORE_OK(acc[cc][0]))
#ifdef EQA_ACTION_NT
            {
              // opt-in: non-temporal stores.  They win only while the SOURCE fits the 256 MB Infinity Cache (B = 256 launched
              // back to back: 47 vs 58 us); with the working set in HBM (B = 1024, or inside the real step) both forms run
              // at the copy ceiling (226 us per 1024 images = 5.44 TB/s) and the regular stores drain after the kernel
              typedef float f4v __attribute__((ext_vector_type(4)));
              f4v v4 = {acc[cc][0], acc[cc][1], acc[cc][2], acc[cc][3]};
              __builtin_nontemporal_store(v4, reinterpret_cast<f4v*>(o));
            }
#else
              *reinterpret_cast<float4*>(o) = make_float4(acc[cc][0], acc[cc][1], acc[cc][2], acc[cc][3]);
#endif
          } else {
#pragma unroll
            for (int k = 0; k < 4; ++k)
              if (jb + k < a.OW) o[k] = acc[cc][k];
          }
        }
      }
    }
  }
  if (MODE == 1) {
    __shared__ float s_red[kThreads / 64];
    const float ws = wave_sum_f(angle_sum);
    if (lane == 0) s_red[wave] = ws;
    __syncthreads();
    if (tid == 0) {
      const int tiles_x = (int)(gridDim.x >> 3);
      a.partial[((size_t)n * gridDim.y + tile_y) * tiles_x + tile_x] = (s_red[0] + s_red[1]) + (s_red[2] + s_red[3]);
    }
  }
}

template <int CH, bool VEC>
__global__ __launch_bounds__(kThreads, EQA_ACTION_WAVES) void group_action_kernel(const ActionArgs a) {
  group_action_body<CH, VEC>(a, (int)blockIdx.z);
}

template <int CH>
__global__ __launch_bounds__(kThreads) void group_action_angle_kernel(const ActionArgs a) {
  group_action_body<CH, false, 1>(a, (int)blockIdx.z);
}

// Two jobs with the same tile grid in ONE launch (eqa_group_action_pair: canonicalize x / invert f with the same group
// index): blocks [0, zsplit) of the z axis run job 0, the rest job 1.  The dispatcher walks z last, so job 1's first blocks
// fill the CUs that job 0's tail leaves idle -- the ~12 us drain + launch gap between two dependent-looking launches
// (they are independent) disappears.  Each block executes exactly one of the two bodies: no register or LDS cost.
template <int CH, bool VEC>
__global__ __launch_bounds__(kThreads, EQA_ACTION_WAVES) void group_action_pair_kernel(const ActionArgs a0, const ActionArgs a1,
                                                                                      const int zsplit) {
  if ((int)blockIdx.z < zsplit)
    group_action_body<CH, VEC>(a0, (int)blockIdx.z);
  else
    group_action_body<CH, VEC>(a1, (int)blockIdx.z - zsplit);
}

// ------------------------------------------------------------------------------------------------
// One-channel maps (configs[4]'s inverse on a (B, 1, 1024, 1024) output; discrete_group.py:204-238): NT tiles per block.  With one
// channel a block of the kernel above moves 4.6 KB in and 4 KB out over a life of three dependent memory round trips (element ->
// matrix -> window -> stores), and the eight blocks a CU holds keep 2.5 TB/s in flight (105 us per 32 maps of 1024 x 1024).  Here
// a block requests the windows of NT consecutive tiles of the walk TOGETHER (NT windows in LDS), then gathers and stores them one
// after the other, with the window, staging and per-pixel functions of group_action_body: the output is bit-identical.
// grid = (8 * ceil(tiles / NT), 1, ceil(n_out / 8)): block_tile deals (image, slot) as it deals (image, tile).
// 32 maps of 1024 x 1024, random D4 (profiles/r06/kbench_invert_c1.txt): 97 us in the general kernel, 70 / 66 us with 2 / 4 tiles
// per block (8: 95 us -- the per-tile scalars no longer fit the SGPR file), torch's copy of the same bytes 51 us.  What is left
// is vector arithmetic: the per-pixel coordinates of a tile cost the same for one channel as for three.
#ifndef EQA_ACTION_C1_TILES
#define EQA_ACTION_C1_TILES 4
#endif
int g_c1_tiles = EQA_ACTION_C1_TILES;   // eqa_set_option(3, 0 | 2 | 4): 0 = one-channel maps through group_action_kernel<1>

template <int NT, bool VEC>
__global__ __launch_bounds__(kThreads) void group_action_c1_kernel(const ActionArgs a, const int tiles_x, const int tiles_y) {
  extern __shared__ __attribute__((aligned(16))) float smem[];
  const int tid = threadIdx.x;
  const int lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  int n, slot, ty_unused;
  if (!block_tile(a.n_out, (int)blockIdx.z, n, slot, ty_unused)) return;
  Element el = load_element(a, n);
  el.e = __builtin_amdgcn_readfirstlane(el.e);   // (block-uniform; the DMA below wants its plane pointer in SGPRs)
  el.b = __builtin_amdgcn_readfirstlane(el.b);
  n = __builtin_amdgcn_readfirstlane(n);
  slot = __builtin_amdgcn_readfirstlane(slot);
  const bool col_walk = fabsf(el.t1) > fabsf(el.t0) && tiles_y > 1;   // quarter turns walk the tiles column by column (group_action_body)
  const int tiles = tiles_x * tiles_y;
  const int win_floats = a.lds_rows * kLdsStride;
  const unsigned src_plane = (unsigned)(a.H * a.W), dst_plane = (unsigned)(a.OH * a.OW);
  const float* const plane[1] = {a.src + (size_t)el.b * src_plane};
  float* const dst_img = a.dst + (size_t)n * dst_plane;
  const SamplingInverse inv = sampling_inverse(a, el);

  // ---- the windows of the slot's NT tiles: lane t of every wave evaluates tile t (one pass of the corner arithmetic per wave
  // instead of NT), v_readlane hands the results to the wave as scalars.  (With every lane evaluating every tile this part was
  // a third of the kernel's vector instructions: profiles/r06/kbench_invert_c1_v1_ablations.txt.)
  int v_i0, v_j0, v_xl, v_yl, v_bw, v_bh, v_in;
  {
    const int lin = slot * NT + min(lane, NT - 1);
    const int lc = min(lin, tiles - 1);
    int tile_x, tile_y;
    if (col_walk) { tile_x = lc / tiles_y; tile_y = lc - tile_x * tiles_y; }
    else { tile_y = lc / tiles_x; tile_x = lc - tile_y * tiles_x; }
    const int j0 = tile_x * kTile, i0 = tile_y * kTile;
    const int i1 = min(i0 + kTile - 1, a.OH - 1), j1 = min(j0 + kTile - 1, a.OW - 1);
    const Window w = tile_window(a, el, i0, j0, i1, j1);
    v_i0 = i0; v_j0 = j0; v_xl = w.x_lo; v_yl = w.y_lo;
    v_bw = lin < tiles ? w.bw : 0;                     // 0: no such tile
    v_bh = w.bh;
    // a whole tile whose window lies inside the frame: no pixel of it needs a range check or a clamp
    v_in = (w.x_lo >= 0 && w.y_lo >= 0 && w.x_hi() <= a.Wp - 1 && w.y_hi() <= a.Hp - 1 && i0 + kTile <= a.OH && j0 + kTile <= a.OW) ? 1 : 0;
  }
  int wi0[NT], wj0[NT], x_lo[NT], y_lo[NT], bw[NT], bh[NT];
  bool use_lds[NT];
#pragma unroll
  for (int t = 0; t < NT; ++t) {
    wi0[t] = __builtin_amdgcn_readlane(v_i0, t); wj0[t] = __builtin_amdgcn_readlane(v_j0, t);
    x_lo[t] = __builtin_amdgcn_readlane(v_xl, t); y_lo[t] = __builtin_amdgcn_readlane(v_yl, t);
    bw[t] = __builtin_amdgcn_readlane(v_bw, t); bh[t] = __builtin_amdgcn_readlane(v_bh, t);
    use_lds[t] = (bw[t] != 0) && (bw[t] <= kBox) && (bh[t] <= a.lds_rows) && !a.force_direct;
  }
#pragma unroll
  for (int t = 0; t < NT; ++t) {
    if (bw[t] != 0 && use_lds[t]) {               // block-uniform
      // ---- request the window: lane = window column, the four waves interleave the window rows (global -> LDS DMA)
      const int i0 = wi0[t], j0 = wj0[t];
      const int i1 = min(i0 + kTile - 1, a.OH - 1), j1 = min(j0 + kTile - 1, a.OW - 1);
      const Window w = {x_lo[t], y_lo[t], bw[t], bh[t]};
      const WindowLane wl = lane_mask(a, el, inv, w, lane, i0, j0, i1, j1);
      float* const win = smem + t * win_floats;
      stage_window_rows<1>(a, win, w, wl, wave, plane);
      zero_fill_window<1>(a, win, w, wl, window_any_zero(a, w), wave, lane);
    }
  }

  const int r = tid >> 3, q = tid & 7;
  // one tile: per-pixel setup (under the DMA for the first tile), gather, store.  INNER (block-uniform per tile): a whole tile
  // whose window lies inside the frame -- every neighbour is a frame pixel inside the window, the range checks and clamps of the
  // general form are identities and are not evaluated.
  auto do_tile = [&](const int t, auto inner_c) {
    constexpr bool INNER = decltype(inner_c)::value;
    const int i = wi0[t] + r, jb = wj0[t] + 4 * q;
    int pi = i, pj = jb;
    if (t == 0) asm volatile("" : "+v"(pi), "+v"(pj));   // the first tile's setup runs under the DMA
    int lidx[4], gx0[4], gy0[4];
    bool live[4];
    float w00[4], w01[4], w10[4], w11[4];
#pragma unroll
    for (int k = 0; k < 4; ++k) {
      const PixelSample s = sample_pixel(a, el, pi, pj + k);
      const float wx0 = 1.0f - s.wx1, wy0 = 1.0f - s.wy1;
      int xi, yi, lx, ly;
      if (INNER) {
        live[k] = true;
        xi = (int)s.xf; yi = (int)s.yf;
        lx = xi - x_lo[t]; ly = yi - y_lo[t];
      } else {
        live[k] = s.live;
        xi = s.xi; yi = s.yi;
        lx = min(max(xi - x_lo[t], 0), bw[t] - 2); ly = min(max(yi - y_lo[t], 0), bh[t] - 2);
      }
      gx0[k] = xi;
      gy0[k] = yi;
      check_window(a, Window{x_lo[t], y_lo[t], bw[t], bh[t]}, live[k], xi, yi, pi, pj + k);
      lidx[k] = ly * kLdsStride + lx;
      w00[k] = wy0 * wx0;
      w01[k] = wy0 * s.wx1;
      w10[k] = s.wy1 * wx0;
      w11[k] = s.wy1 * s.wx1;
    }
    if (t == 0) {
      asm volatile("s_waitcnt vmcnt(0)" ::: "memory");   // this wave's DMA (every tile's) has landed in LDS
      __syncthreads();                                    // ... and so has every other wave's
    }
    float acc[4];
    if (use_lds[t]) {
      const float* s = smem + t * win_floats;
#pragma unroll
      for (int k = 0; k < 4; ++k) {
        const float nw = s[lidx[k]], ne = s[lidx[k] + 1];
        const float sw = s[lidx[k] + kLdsStride], se = s[lidx[k] + kLdsStride + 1];
        const float v = blend4(nw, ne, sw, se, w00[k], w01[k], w10[k], w11[k]);
        acc[k] = (INNER || live[k]) ? v : 0.0f;
      }
    } else {
      // window too large for LDS, or forced: rare, the same arithmetic from global memory
#pragma unroll
      for (int k = 0; k < 4; ++k) acc[k] = 0.0f;
#pragma unroll 1
      for (int k = 0; k < 4; ++k) {
        const float v = gather4_direct(plane[0], a, el, pick4(gx0, k), pick4(gy0, k), pick4(w00, k), pick4(w01, k), pick4(w10, k),
                                       pick4(w11, k), pick4(live, k));
#pragma unroll
        for (int k2 = 0; k2 < 4; ++k2)
          if (k2 == k) acc[k2] = v;
      }
    }
    if (i < a.OH) {
      float* o = dst_img + (unsigned)(i * a.OW + jb);
      if (VEC) {
        if (jb < a.OW && EQA_ABL_STORE_OK(acc[0])) *reinterpret_cast<float4*>(o) = make_float4(acc[0], acc[1], acc[2], acc[3]);
      } else {
#pragma unroll
        for (int k = 0; k < 4; ++k)
          if (jb + k < a.OW) o[k] = acc[k];
      }
    }
  };
#pragma unroll
  for (int t = 0; t < NT; ++t) {
    if (bw[t] == 0) break;          // block-uniform: the tiles of a slot are consecutive
    // (v_in is read here, not kept per tile: a lane mask per tile across the whole kernel is what the SGPR file cannot spare)
    if (__builtin_amdgcn_readlane(v_in, t) != 0) do_tile(t, std::true_type());
    else do_tile(t, std::false_type());
  }
}

// ------------------------------------------------------------------------------------------------
// Backward of the group action.  y[n,c,i,j] = sum_k w_k(phi) * frame[c, nbr_k(i,j; phi)]  (bilinear, 4 neighbours)
//   ANGLE: dL/dphi = sum gy * (dy/dix * dix/dphi + dy/diy * diy/dphi), with the source point rotating about the frame
//          centre c:  s = c + R(phi)^-1 (dst - c)  =>  ds/dphi = (-(s_y - c_y), s_x - c_x)  [per radian],
//          dy/dix = wy0 (ne - nw) + wy1 (se - sw),  dy/diy = wx0 (sw - nw) + wx1 (se - ne)
//          (what autograd derives through kornia's rotation-matrix -> affine_grid -> grid_sample chain,
//          discrete_group.py:213 / images/utils.py:57).  One partial per (output image, tile): deterministic.
//   INPUT: adjoint of the gather: scatter gy * w_k to the (clamped = replicate-pad adjoint, flipped, channel-mapped)
//          source pixels with hardware float atomics (same approach as torch's grid_sampler backward).
//   THETA (GRAD == 2): dL/dtheta[6] for a per-sample affine matrix (continuous groups: K.geometry.warp_affine in
//          images/canonicalization/continuous_group.py:203): ix = ((t0 xn + t1 yn + t2) + 1) half_w  =>
//          d ix / d(t0, t1, t2) = half_w (xn, yn, 1), likewise iy with half_h; six partials per (output image, tile).
// Same grid decomposition as the forward kernel; direct gathers (L1/L2), no LDS staging: correctness first.
template <int GRAD, bool INPUT>  // GRAD: 0 none, 1 rotation angle, 2 affine matrix
__global__ __launch_bounds__(kThreads) void group_action_bwd_kernel(const ActionArgs a) {
  constexpr bool ANGLE = GRAD != 0;  // needs the image gradient at the sample point
  constexpr int NS = GRAD == 2 ? 6 : 1;
  __shared__ float s_red[4][NS];
  const int tid = threadIdx.x;
  int n, tile_x, tile_y;
  if (!block_tile(a.n_out, (int)blockIdx.z, n, tile_x, tile_y)) return;
  const int j0 = tile_x * kTile, i0 = tile_y * kTile;
  const Element el = load_element(a, n);
  const int e = el.e, b = el.b;

  const int r = tid >> 3, q = tid & 7;
  const int i = i0 + r, jb = j0 + 4 * q;
  const bool row_ok = i < a.OH;
  int gx0[4], gy0[4];
  bool live[4];
  float wx1[4], wy1[4], armx[4], army[4], xns[4];
  float yn = 0.0f;
#pragma unroll
  for (int k = 0; k < 4; ++k) {
    const PixelSample s = sample_pixel(a, el, i, jb + k);
    wx1[k] = s.wx1;
    wy1[k] = s.wy1;
    live[k] = s.live && row_ok && (jb + k < a.OW);
    gx0[k] = s.xi;
    gy0[k] = s.yi;
    armx[k] = -(s.iy - a.half_h);  // lever arm about the frame centre ((Wp-1)/2, (Hp-1)/2)
    army[k] = s.ix - a.half_w;
    xns[k] = s.xn;
    yn = s.yn;
  }
  int off[4][4];
  bool in[4][4];
#pragma unroll
  for (int k = 0; k < 4; ++k) {
    off[k][0] = src_offset(a, el, gy0[k], gx0[k], in[k][0]);
    off[k][1] = src_offset(a, el, gy0[k], gx0[k] + 1, in[k][1]);
    off[k][2] = src_offset(a, el, gy0[k] + 1, gx0[k], in[k][2]);
    off[k][3] = src_offset(a, el, gy0[k] + 1, gx0[k] + 1, in[k][3]);
  }

  const unsigned src_plane = (unsigned)(a.H * a.W), dst_plane = (unsigned)(a.OH * a.OW);
  const size_t img_off = (size_t)b * ((size_t)a.C * src_plane);
  const float* const src_img = a.src + img_off;
  const float* const gout_img = a.gout + (size_t)n * ((size_t)a.C * dst_plane);
  float sum = 0.0f;
  float sx[4] = {0.f, 0.f, 0.f, 0.f}, sy[4] = {0.f, 0.f, 0.f, 0.f};  // GRAD == 2: per-pixel sums of g*dix, g*diy over channels
#pragma unroll 1
  for (int c = 0; c < a.C; ++c) {
    const int cs = a.chan_map ? (c / a.G) * a.G + a.chan_map[e * a.G + c % a.G] : c;
    const float* pl = src_img + (unsigned)cs * src_plane;
    const float* go = gout_img + (unsigned)c * dst_plane + (unsigned)(i * a.OW + jb);
    // (ANGLE without INPUT -- the training step's angle gradient -- requests a channel's 16 neighbours and 4 gradient values
    // together: the offsets are clamped into the plane, so the loads need no predicate, only the values a select; as conditional
    // loads behind `if (!live) continue` every one of them was waited for on the spot: 174 us per 256 images)
    float nbv[4][4], gv[4];
    if (ANGLE && !INPUT) {
#pragma unroll
      for (int k = 0; k < 4; ++k) {
        gv[k] = gout_img[(unsigned)c * dst_plane + (live[k] ? (unsigned)(i * a.OW + jb + k) : 0u)];   // (a dead pixel reads the plane's first value)
#pragma unroll
        for (int t = 0; t < 4; ++t) nbv[k][t] = pl[off[k][t]];
      }
    }
#pragma unroll
    for (int k = 0; k < 4; ++k) {
      if (!(ANGLE && !INPUT) && !live[k]) continue;
      const float g = (ANGLE && !INPUT) ? (live[k] ? gv[k] : 0.0f) : go[k];
      const float wx0 = 1.0f - wx1[k], wy0 = 1.0f - wy1[k];
      if (ANGLE) {
        float nw, ne, sw, se;
        if (!INPUT) {
          nw = in[k][0] ? nbv[k][0] : 0.0f; ne = in[k][1] ? nbv[k][1] : 0.0f;
          sw = in[k][2] ? nbv[k][2] : 0.0f; se = in[k][3] ? nbv[k][3] : 0.0f;
        } else {
          nw = in[k][0] ? pl[off[k][0]] : 0.0f; ne = in[k][1] ? pl[off[k][1]] : 0.0f;
          sw = in[k][2] ? pl[off[k][2]] : 0.0f; se = in[k][3] ? pl[off[k][3]] : 0.0f;
        }
        const float dix = wy0 * (ne - nw) + wy1[k] * (se - sw);
        const float diy = wx0 * (sw - nw) + wx1[k] * (se - ne);
        // (a dead pixel contributes nothing -- a select, not g = 0: a non-finite neighbour must not turn 0 * inf into NaN)
        if (GRAD == 1) sum += live[k] ? g * (dix * armx[k] + diy * army[k]) : 0.0f;
        else { sx[k] += live[k] ? g * dix : 0.0f; sy[k] += live[k] ? g * diy : 0.0f; }
      }
      if (INPUT) {
        float* gp = a.gsrc + img_off + (size_t)cs * src_plane;
        if (in[k][0]) unsafeAtomicAdd(gp + off[k][0], g * wy0 * wx0);
        if (in[k][1]) unsafeAtomicAdd(gp + off[k][1], g * wy0 * wx1[k]);
        if (in[k][2]) unsafeAtomicAdd(gp + off[k][2], g * wy1[k] * wx0);
        if (in[k][3]) unsafeAtomicAdd(gp + off[k][3], g * wy1[k] * wx1[k]);
      }
    }
  }
  if (ANGLE) {
    float v[NS];
    if (GRAD == 1) {
      v[0] = sum;
    } else {
#pragma unroll
      for (int m = 0; m < NS; ++m) v[m] = 0.0f;
#pragma unroll
      for (int k = 0; k < 4; ++k) {
        v[0] += sx[k] * xns[k]; v[1] += sx[k] * yn; v[2] += sx[k];
        v[NS - 3] += sy[k] * xns[k]; v[NS - 2] += sy[k] * yn; v[NS - 1] += sy[k];
      }
#pragma unroll
      for (int m = 0; m < NS; ++m) v[m] *= (m < 3 ? a.half_w : a.half_h);
    }
#pragma unroll
    for (int m = 0; m < NS; ++m) {
      const float w = wave_sum_f(v[m]);
      if ((tid & 63) == 0) s_red[tid >> 6][m] = w;
    }
    __syncthreads();
    if (tid < NS) {
      const int tiles_x = (int)(gridDim.x >> 3);
      const size_t t = ((size_t)n * gridDim.y + tile_y) * tiles_x + tile_x;
      a.partial[t * NS + tid] = (s_red[0][tid] + s_red[1][tid]) + (s_red[2][tid] + s_red[3][tid]);
    }
  }
}

// Input gradient as a GATHER (no atomics, deterministic, no pre-zeroed buffer) for the un-padded, one-output-per-image
// case -- the invert action I7 on image-shaped network outputs, which is what a segmentation loss differentiates through.
// A source pixel s receives g[o] * w(o, s) from the output pixels o whose sample point p(o) lies within one pixel of s;
// p is affine in o, so the candidates are the integer points of A^-1(s + (-1,1)^2): at most 3 x 3 for a rotation, 4 x 4
// slots here.  Each candidate's weight is recomputed exactly as the forward computes it (floor, fractional parts).
// Measured against the atomic scatter: 3.4 ms -> see HISTORY.md for 256 x 3 x 224 x 224.
template <bool MAPPED>
__global__ __launch_bounds__(kThreads) void group_action_bwd_gather_kernel(const ActionArgs a) {
  __shared__ int s_inv[kMaxMapG];
  const Element el = load_element(a, (int)blockIdx.z);   // (a.gidx is set: one output per image)
  const int b = el.b, e = el.e;
  if (MAPPED) {
    if (threadIdx.x < a.G) s_inv[a.chan_map[e * a.G + threadIdx.x]] = threadIdx.x;  // inverse of the channel permutation
    __syncthreads();
  }
  const int sx = blockIdx.x * 64 + (threadIdx.x & 63), sy = blockIdx.y * 4 + (threadIdx.x >> 6);
  if (sx >= a.W || sy >= a.H) return;
  const bool flip_dst = el.flip_dst(), flip_src = el.flip_src();
  const int fx = flip_src ? (a.Wp - 1 - sx) : sx, fy = sy;  // pad == 0: the frame is the source
  // (jf, i') -> sample point, as an affine map, and its inverse -- by division, not sampling_inverse's multiplication by 1 / det:
  // the candidate ranges below were validated with these bits
  const SamplingMap sm = sampling_map(a, el);
  const float b0 = sm.b0, b1 = sm.b1;
  const float det = sm.a00 * sm.a11 - sm.a01 * sm.a10;
  const float m00 = sm.a11 / det, m01 = -sm.a01 / det, m10 = -sm.a10 / det, m11 = sm.a00 / det;
  const float px = (float)fx - b0, py = (float)fy - b1;
  const float jc = m00 * px + m01 * py, ic = m10 * px + m11 * py;
  const float dj = fabsf(m00) + fabsf(m01) + 0.05f, di = fabsf(m10) + fabsf(m11) + 0.05f;
  const int j_lo = max((int)ceilf(jc - dj), 0), j_hi = min((int)floorf(jc + dj), a.Wp - 1);
  const int i_lo = max((int)ceilf(ic - di), 0), i_hi = min((int)floorf(ic + di), a.Hp - 1);
  float w[16];
  int off[16];
#pragma unroll
  for (int r = 0; r < 4; ++r) {
#pragma unroll
    for (int c = 0; c < 4; ++c) {
      const int ii = i_lo + r, jf = j_lo + c;
      float wt = 0.0f;
      int o = 0;
      const int i = ii - a.top, j = (flip_dst ? (a.Wp - 1 - jf) : jf) - a.left;
      if (ii <= i_hi && jf <= j_hi && i >= 0 && i < a.OH && j >= 0 && j < a.OW) {
        const float xn = lin_m1_p1(jf, a.Wp, a.step_x), yn = lin_m1_p1(ii, a.Hp, a.step_y);
        float ix, iy;
        sample_point(el.t0, el.t1, el.t2, el.t3, el.t4, el.t5, xn, yn, a.half_w, a.half_h, ix, iy);
        const float xf = floorf(ix), yf = floorf(iy);
        const float wx1 = ix - xf, wy1 = iy - yf;
        const float ffx = (float)fx, ffy = (float)fy;
        const float wx = (ffx == xf) ? 1.0f - wx1 : ((ffx == xf + 1.0f) ? wx1 : 0.0f);
        const float wy = (ffy == yf) ? 1.0f - wy1 : ((ffy == yf + 1.0f) ? wy1 : 0.0f);
        wt = wy * wx;
        o = i * a.OW + j;
      }
      w[r * 4 + c] = wt;
      off[r * 4 + c] = o;
    }
  }
  const size_t src_plane = (size_t)a.H * a.W, dst_plane = (size_t)a.OH * a.OW;
  const float* gimg = a.gout + (size_t)b * a.C * dst_plane;
  float* simg = a.gsrc + (size_t)b * a.C * src_plane + (size_t)sy * a.W + sx;
  for (int cs = 0; cs < a.C; ++cs) {
    const int c = MAPPED ? (cs / a.G) * a.G + s_inv[cs % a.G] : cs;
    const float* gp = gimg + (size_t)c * dst_plane;
    float acc = 0.0f;
#pragma unroll
    for (int k = 0; k < 16; ++k)
      if (w[k] != 0.0f) acc += gp[off[k]] * w[k];
    simg[(size_t)cs * src_plane] = acc;
  }
}

// Adjoint of the replicate ("edge") padding: gsrc[sy][sx] = sum of gframe over the frame pixels that clamp to (sy, sx) --
// itself for interior pixels, a strip of pad+1 pixels on the borders, a (pad+1)^2 square in the corners.  Together with the
// gather above run on the padded frame as its source this is the deterministic input gradient of the canonicalizing
// transform I5 (pad -> [flip] -> rotate -> crop).  Separable: fold the columns of every frame row (the two border sums
// by a block reduction), then the rows of every column (one thread per column, coalesced over columns).
__global__ __launch_bounds__(kThreads) void fold_edge_pad_x_kernel(const float* __restrict__ gframe, float* __restrict__ tmp,
                                                                  int W, int pad) {
  __shared__ float s_red[2][kThreads / 64];
  const int Wp = W + 2 * pad;
  const size_t row = blockIdx.x;  // plane * Hp + fy
  const float* g = gframe + row * Wp;
  float* o = tmp + row * W;
  for (int sx = 1 + threadIdx.x; sx < W - 1; sx += kThreads) o[sx] = g[sx + pad];
  float l = 0.f, r = 0.f;  // left border: frame columns [0, pad]; right border: [pad + W - 1, Wp - 1]
  for (int k = threadIdx.x; k <= pad; k += kThreads) { l += g[k]; r += g[pad + W - 1 + k]; }
  l = wave_sum_f(l);
  r = wave_sum_f(r);
  if ((threadIdx.x & 63) == 0) { s_red[0][threadIdx.x >> 6] = l; s_red[1][threadIdx.x >> 6] = r; }
  __syncthreads();
  if (threadIdx.x == 0) {
    float a = 0.f, c = 0.f;
    for (int w = 0; w < kThreads / 64; ++w) { a += s_red[0][w]; c += s_red[1][w]; }
    if (W == 1) o[0] = a + c - g[pad];  // both strips contain the single column once too often
    else { o[0] = a; o[W - 1] = c; }
  }
}

__global__ __launch_bounds__(kThreads) void fold_edge_pad_y_kernel(const float* __restrict__ tmp, float* __restrict__ gsrc,
                                                                  int H, int W, int pad) {
  const int sx = blockIdx.x * kThreads + threadIdx.x;
  if (sx >= W) return;
  const int Hp = H + 2 * pad;
  const size_t plane = blockIdx.y;
  const float* t = tmp + plane * (size_t)Hp * W + sx;
  float* o = gsrc + plane * (size_t)H * W + sx;
  float top = 0.f, bot = 0.f;
  for (int k = 0; k <= pad; ++k) { top += t[(size_t)k * W]; bot += t[(size_t)(pad + H - 1 + k) * W]; }
  if (H == 1) { o[0] = top + bot - t[(size_t)pad * W]; return; }
  o[0] = top;
  o[(size_t)(H - 1) * W] = bot;
  for (int sy = 1; sy < H - 1; ++sy) o[(size_t)sy * W] = t[(size_t)(sy + pad) * W];
}

template <int CH>
int launch_action_ch(const ActionArgs& a, bool vec, hipStream_t st) {
  const int tiles_x = (a.OW + kTile - 1) / kTile, tiles_y = (a.OH + kTile - 1) / kTile;
  const int groups = (a.n_out + kXcd - 1) / kXcd;
  if (tiles_y > 65535 || groups > 65535) return EQA_ERR_UNSUPPORTED;
  const dim3 grid((unsigned)(kXcd * tiles_x), (unsigned)tiles_y, (unsigned)groups);
  const size_t lds = (size_t)CH * a.lds_rows * kLdsStride * sizeof(float) + (a.chan_map ? kMaxMapG * sizeof(int) : 0);
  if (vec)
    hipLaunchKernelGGL((group_action_kernel<CH, true>), grid, dim3(kThreads), lds, st, a);
  else
    hipLaunchKernelGGL((group_action_kernel<CH, false>), grid, dim3(kThreads), lds, st, a);
  return hipGetLastError() == hipSuccess ? EQA_OK : EQA_ERR_LAUNCH;
}

template <int NT>
int launch_action_c1_nt(const ActionArgs& a, bool vec, hipStream_t st) {
  const int tiles_x = (a.OW + kTile - 1) / kTile, tiles_y = (a.OH + kTile - 1) / kTile;
  const long long slots = ((long long)tiles_x * tiles_y + NT - 1) / NT;
  const int groups = (a.n_out + kXcd - 1) / kXcd;
  if (slots * kXcd > 0x7fffffffLL || groups > 65535) return EQA_ERR_UNSUPPORTED;
  const dim3 grid((unsigned)(kXcd * slots), 1u, (unsigned)groups);
  const size_t lds = (size_t)NT * a.lds_rows * kLdsStride * sizeof(float);
  if (vec)
    hipLaunchKernelGGL((group_action_c1_kernel<NT, true>), grid, dim3(kThreads), lds, st, a, tiles_x, tiles_y);
  else
    hipLaunchKernelGGL((group_action_c1_kernel<NT, false>), grid, dim3(kThreads), lds, st, a, tiles_x, tiles_y);
  return hipGetLastError() == hipSuccess ? EQA_OK : EQA_ERR_LAUNCH;
}

// one-channel maps: NT tiles per block where the map has enough tiles to fill the chip that way
int launch_action_c1(const ActionArgs& a, bool vec, hipStream_t st) {
  const long long tiles = (long long)((a.OW + kTile - 1) / kTile) * ((a.OH + kTile - 1) / kTile);
  if (tiles * a.n_out < 4096) return EQA_ERR_UNSUPPORTED;      // small jobs: a tile per block fills the CUs better
  if (g_c1_tiles >= 4) return launch_action_c1_nt<4>(a, vec, st);
  return launch_action_c1_nt<2>(a, vec, st);
}

int fill_action_args(ActionArgs& a, const float* src, float* dst, const int32_t* gidx, const float* theta,
                     const int32_t* flags, const int32_t* chan_map, int E, int G, int n_out, int B, int C, int H, int W,
                     int pad, int OH, int OW, int top, int left) {
  if (n_out == 0 && B >= 0) {  // empty batch: nothing to validate against (empty tensors have null data pointers)
    a.n_out = 0;
    return EQA_OK;
  }
  if (!src || !theta || E <= 0 || n_out < 0 || B <= 0 || C <= 0 || H <= 0 || W <= 0 || pad < 0 || OH <= 0 || OW <= 0 ||
      top < 0 || left < 0)
    return EQA_ERR_INVALID_ARG;
  const int Hp = H + 2 * pad, Wp = W + 2 * pad;
  if (Hp < 2 || Wp < 2 || top + OH > Hp || left + OW > Wp) return EQA_ERR_INVALID_ARG;
  if (chan_map && (G <= 0 || C % G != 0)) return EQA_ERR_INVALID_ARG;
  if (chan_map && G > kMaxMapG) return EQA_ERR_UNSUPPORTED;
  if ((long long)C * H * W >= (1LL << 30) || (long long)C * OH * OW >= (1LL << 30)) return EQA_ERR_UNSUPPORTED;  // 32-bit offsets inside one image
  a.src = src; a.dst = dst; a.gidx = gidx; a.theta = theta; a.flags = flags; a.chan_map = chan_map;
  a.E = E; a.G = chan_map ? G : 1; a.n_out = n_out; a.B = B; a.C = C;
  a.H = H; a.W = W; a.pad = pad; a.Hp = Hp; a.Wp = Wp;
  a.OH = OH; a.OW = OW; a.top = top; a.left = left;
  a.half_w = (float)(Wp - 1) / 2.0f;
  a.half_h = (float)(Hp - 1) / 2.0f;
  a.step_x = 2.0f / (float)(Wp - 1);
  a.step_y = 2.0f / (float)(Hp - 1);
  a.force_direct = g_force_direct;
  a.lds_rows = kBox;
  a.gout = nullptr; a.gsrc = nullptr; a.partial = nullptr;
  return EQA_OK;
}

int launch_action(const float* src, float* dst, const int32_t* gidx, const float* theta, const int32_t* flags,
                  const int32_t* chan_map, int E, int G, int n_out, int B, int C, int H, int W, int pad, int OH,
                  int OW, int top, int left, void* stream, int max_window = 0) {
  if (!dst && n_out != 0) return EQA_ERR_INVALID_ARG;
  ActionArgs a;
  const int rc = fill_action_args(a, src, dst, gidx, theta, flags, chan_map, E, G, n_out, B, C, H, W, pad, OH, OW, top, left);
  if (rc != EQA_OK) return rc;
  if (n_out == 0) return EQA_OK;
  // the caller's bound on a tile's source window (right-angle elements: 35 rows instead of 47 -> 19.7 KB of LDS per block at three
  // channels, 8 blocks per CU instead of 6); a window that turns out larger takes the direct path: slow, never wrong
  if (max_window > 0) a.lds_rows = std::min(std::max(max_window, 2), kBox);
  const bool vec = (OW % 4 == 0) && (((uintptr_t)dst & 15) == 0);
  hipStream_t st = (hipStream_t)stream;
#if EQA_FORCE_CH
  return launch_action_ch<EQA_FORCE_CH>(a, vec, st);
#else
  if (C == 1 && !chan_map && g_c1_tiles > 0) {
    const int rc1 = launch_action_c1(a, vec, st);
    if (rc1 != EQA_ERR_UNSUPPORTED) return rc1;
  }
  if (C % 3 == 0) return launch_action_ch<3>(a, vec, st);
  if (C % 2 == 0) return launch_action_ch<2>(a, vec, st);
  return launch_action_ch<1>(a, vec, st);
#endif
}

template <int CH>
int launch_pair_ch(const ActionArgs& a0, const ActionArgs& a1, bool vec, hipStream_t st) {
  const int tiles_x = (a0.OW + kTile - 1) / kTile, tiles_y = (a0.OH + kTile - 1) / kTile;
  const int g0 = (a0.n_out + kXcd - 1) / kXcd, g1 = (a1.n_out + kXcd - 1) / kXcd;
  if (tiles_y > 65535 || g0 + g1 > 65535) return EQA_ERR_UNSUPPORTED;
  const dim3 grid((unsigned)(kXcd * tiles_x), (unsigned)tiles_y, (unsigned)(g0 + g1));
  const size_t lds = (size_t)CH * kBox * kLdsStride * sizeof(float) + ((a0.chan_map || a1.chan_map) ? kMaxMapG * sizeof(int) : 0);
  if (vec)
    hipLaunchKernelGGL((group_action_pair_kernel<CH, true>), grid, dim3(kThreads), lds, st, a0, a1, g0);
  else
    hipLaunchKernelGGL((group_action_pair_kernel<CH, false>), grid, dim3(kThreads), lds, st, a0, a1, g0);
  return hipGetLastError() == hipSuccess ? EQA_OK : EQA_ERR_LAUNCH;
}

inline int action_ch(int C) { return C % 3 == 0 ? 3 : (C % 2 == 0 ? 2 : 1); }

// canonicalize x (edge-padded frame, crop back) and invert f (whole frame, optional regular-representation roll) for the same
// per-image group index.  One launch when the two jobs share the tile grid, the channel staging width and the store width
// (always the case for x, f of the same H x W with 3 | C or equal parity); two launches otherwise -- same results either way.
int launch_pair(const float* x, float* y, const float* theta_c, const int32_t* flags_c, int pad, int C, const float* f, float* out,
                const float* theta_i, const int32_t* flags_i, const int32_t* chan_map, int G, int Cf, const int32_t* gidx, int E,
                int B, int H, int W, void* stream) {
  if (B == 0) return EQA_OK;
  if (!gidx || !y || !out) return EQA_ERR_INVALID_ARG;
  ActionArgs a0, a1;
  int rc = fill_action_args(a0, x, y, gidx, theta_c, flags_c, nullptr, E, 1, B, B, C, H, W, pad, H, W, pad, pad);
  if (rc != EQA_OK) return rc;
  rc = fill_action_args(a1, f, out, gidx, theta_i, flags_i, chan_map, E, G, B, B, Cf, H, W, 0, H, W, 0, 0);
  if (rc != EQA_OK) return rc;
  hipStream_t st = (hipStream_t)stream;
  const bool v0 = (W % 4 == 0) && (((uintptr_t)y & 15) == 0), v1 = (W % 4 == 0) && (((uintptr_t)out & 15) == 0);
  const int ch0 = EQA_FORCE_CH ? EQA_FORCE_CH : action_ch(C), ch1 = EQA_FORCE_CH ? EQA_FORCE_CH : action_ch(Cf);
  if (ch0 == ch1 && v0 == v1) {
    if (ch0 == 3) return launch_pair_ch<3>(a0, a1, v0, st);
    if (ch0 == 2) return launch_pair_ch<2>(a0, a1, v0, st);
    return launch_pair_ch<1>(a0, a1, v0, st);
  }
  rc = launch_action(x, y, gidx, theta_c, flags_c, nullptr, E, 1, B, B, C, H, W, pad, H, W, pad, pad, stream);
  if (rc != EQA_OK) return rc;
  return launch_action(f, out, gidx, theta_i, flags_i, chan_map, E, G, B, B, Cf, H, W, 0, H, W, 0, 0, stream);
}

// dL/d(angle) partials alone: the LDS-staged form (the forward's window, gathered for the derivative), or with eqa_set_option(0, 1)
// round 3's direct-gather kernel
int launch_angle_grad(const ActionArgs& a, const dim3& grid, hipStream_t st) {
  if (a.force_direct) {
    hipLaunchKernelGGL((group_action_bwd_kernel<1, false>), grid, dim3(kThreads), 0, st, a);
    return launch_status();
  }
  const int ch = action_ch(a.C);
  const size_t lds = (size_t)ch * kBox * kLdsStride * sizeof(float) + (a.chan_map ? kMaxMapG * sizeof(int) : 0);
  if (ch == 3) hipLaunchKernelGGL(group_action_angle_kernel<3>, grid, dim3(kThreads), lds, st, a);
  else if (ch == 2) hipLaunchKernelGGL(group_action_angle_kernel<2>, grid, dim3(kThreads), lds, st, a);
  else hipLaunchKernelGGL(group_action_angle_kernel<1>, grid, dim3(kThreads), lds, st, a);
  return launch_status();
}

int launch_action_bwd(int grad_mode, const float* src, const float* grad_out, const int32_t* gidx, const float* theta,
                      const int32_t* flags, const int32_t* chan_map, float* grad_src, float* partial, int num_elements, int G,
                      int n_out, int B, int C, int H, int W, int pad, int OH, int OW, int top, int left, void* stream) {
  if (n_out == 0 && B >= 0) return EQA_OK;
  if (!grad_out || (!grad_src && !partial)) return EQA_ERR_INVALID_ARG;
  ActionArgs a;
  const int rc = fill_action_args(a, src, nullptr, gidx, theta, flags, chan_map, num_elements, G, n_out, B, C, H, W, pad,
                                  OH, OW, top, left);
  if (rc != EQA_OK) return rc;
  if (n_out == 0) return EQA_OK;
  a.gout = grad_out; a.gsrc = grad_src; a.partial = partial;
  const int tiles_x = (OW + kTile - 1) / kTile, tiles_y = (OH + kTile - 1) / kTile;
  const int groups = (n_out + kXcd - 1) / kXcd;
  if (tiles_y > 65535 || groups > 65535) return EQA_ERR_UNSUPPORTED;
  const dim3 grid((unsigned)(kXcd * tiles_x), (unsigned)tiles_y, (unsigned)groups);
  hipStream_t st = (hipStream_t)stream;
  // un-padded, one output per image, whole-frame output: the input gradient is an exact gather (no atomics; grad_src need
  // not be zeroed).  The transform gradient, if wanted too, comes from its own launch of the scatter-free mode.
  const bool gather = grad_src && pad == 0 && gidx && n_out == B && !g_force_direct;
  if (gather) {
    const dim3 ggrid((W + 63) / 64, (H + 3) / 4, B);
    if (ggrid.y > 65535 || ggrid.z > 65535) return EQA_ERR_UNSUPPORTED;
    if (chan_map)
      hipLaunchKernelGGL((group_action_bwd_gather_kernel<true>), ggrid, dim3(kThreads), 0, st, a);
    else
      hipLaunchKernelGGL((group_action_bwd_gather_kernel<false>), ggrid, dim3(kThreads), 0, st, a);
    if (hipGetLastError() != hipSuccess) return EQA_ERR_LAUNCH;
    if (!partial) return EQA_OK;
    if (grad_mode == 1) return launch_angle_grad(a, grid, st);
    hipLaunchKernelGGL((group_action_bwd_kernel<2, false>), grid, dim3(kThreads), 0, st, a);
    return launch_status();
  }
  if (!partial)
    hipLaunchKernelGGL((group_action_bwd_kernel<0, true>), grid, dim3(kThreads), 0, st, a);
  else if (grad_mode == 1 && grad_src)
    hipLaunchKernelGGL((group_action_bwd_kernel<1, true>), grid, dim3(kThreads), 0, st, a);
  else if (grad_mode == 1)
    return launch_angle_grad(a, grid, st);
  else if (grad_src)
    hipLaunchKernelGGL((group_action_bwd_kernel<2, true>), grid, dim3(kThreads), 0, st, a);
  else
    hipLaunchKernelGGL((group_action_bwd_kernel<2, false>), grid, dim3(kThreads), 0, st, a);
  return launch_status();
}

}  // namespace

extern "C" {

int eqa_abi_version(void) { return EQA_ABI_VERSION; }

int eqa_get_option(int key) {
  if (key == 100) return kMaxWinK;   // read-only: the largest window the window-sum kernels take (ops.MAX_WINDOW_K must equal it)
  return key == 0 ? g_force_direct : key == 1 ? eqa::g_vn_kernel_choice : key == 2 ? eqa::g_cgemm_bf16_form : key == 3 ? g_c1_tiles : EQA_ERR_INVALID_ARG;
}

int64_t eqa_fold_edge_pad_workspace_bytes(int planes, int H, int W, int pad) {
  if (planes <= 0 || H <= 0 || W <= 0 || pad < 0) return 0;
  return (int64_t)planes * (H + 2 * pad) * W * (int64_t)sizeof(float);
}

int eqa_fold_edge_pad(const float* gframe, float* gsrc, void* workspace, int planes, int H, int W, int pad, void* stream) {
  if (planes < 0 || H <= 0 || W <= 0 || pad < 0) return EQA_ERR_INVALID_ARG;
  if (planes == 0) return EQA_OK;
  if (!gframe || !gsrc || !workspace) return EQA_ERR_INVALID_ARG;
  const size_t rows = (size_t)planes * (H + 2 * pad);
  if (rows > 0x7fffffffULL || planes > 65535) return EQA_ERR_UNSUPPORTED;
  hipStream_t st = (hipStream_t)stream;
  hipLaunchKernelGGL(fold_edge_pad_x_kernel, dim3((unsigned)rows), dim3(kThreads), 0, st, gframe, (float*)workspace, W, pad);
  if (hipGetLastError() != hipSuccess) return EQA_ERR_LAUNCH;
  hipLaunchKernelGGL(fold_edge_pad_y_kernel, dim3((W + kThreads - 1) / kThreads, planes), dim3(kThreads), 0, st,
                     (const float*)workspace, gsrc, H, W, pad);
  return launch_status();
}

int eqa_set_option(int key, int value) {
  if (key == 0) {
    g_force_direct = value ? 1 : 0;
    return EQA_OK;
  }
  if (key == 1 && value >= 0 && value <= 2) {
    eqa::g_vn_kernel_choice = value;
    return EQA_OK;
  }
  if (key == 2 && value >= 0 && value <= 1) {
    eqa::g_cgemm_bf16_form = value;
    return EQA_OK;
  }
  if (key == 3 && (value == 0 || value == 2 || value == 4)) {
    g_c1_tiles = value;
    return EQA_OK;
  }
  return EQA_ERR_INVALID_ARG;
}

int eqa_group_action_fwd(const float* src, float* dst, const int32_t* gidx, const float* theta, const int32_t* flags,
                         const int32_t* chan_map, int num_elements, int G, int n_out, int B, int C, int H, int W,
                         int pad, int OH, int OW, int top, int left, void* stream) {
  return launch_action(src, dst, gidx, theta, flags, chan_map, num_elements, G, n_out, B, C, H, W, pad, OH, OW, top,
                       left, stream);
}

int eqa_group_action_fwd_hint(const float* src, float* dst, const int32_t* gidx, const float* theta, const int32_t* flags,
                              const int32_t* chan_map, int num_elements, int G, int n_out, int B, int C, int H, int W,
                              int pad, int OH, int OW, int top, int left, int max_window, void* stream) {
  if (max_window < 0) return EQA_ERR_INVALID_ARG;
  return launch_action(src, dst, gidx, theta, flags, chan_map, num_elements, G, n_out, B, C, H, W, pad, OH, OW, top, left, stream,
                       max_window);
}

int eqa_canon_transform_fwd(const float* x, float* y, const int32_t* gidx, const float* theta, const int32_t* flags,
                            int num_elements, int B, int C, int H, int W, int pad, void* stream) {
  if (B == 0) return EQA_OK;
  if (!gidx) return EQA_ERR_INVALID_ARG;
  // CenterCrop offset of torchvision: int(round((Hp - H) / 2)) == pad exactly, since Hp - H = 2*pad
  return launch_action(x, y, gidx, theta, flags, nullptr, num_elements, 1, B, B, C, H, W, pad, H, W, pad, pad, stream);
}

int eqa_invert_action_fwd(const float* f, float* out, const int32_t* gidx, const float* theta, const int32_t* flags,
                          const int32_t* chan_map, int num_elements, int G, int B, int C, int H, int W, void* stream) {
  if (B == 0) return EQA_OK;
  if (!gidx) return EQA_ERR_INVALID_ARG;
  return launch_action(f, out, gidx, theta, flags, chan_map, num_elements, G, B, B, C, H, W, 0, H, W, 0, 0, stream);
}

int eqa_group_action_pair(const float* x, float* y, const float* theta_canon, const int32_t* flags_canon, int pad, int C,
                          const float* f, float* out, const float* theta_inv, const int32_t* flags_inv, const int32_t* chan_map,
                          int G, int Cf, const int32_t* gidx, int num_elements, int B, int H, int W, void* stream) {
  return launch_pair(x, y, theta_canon, flags_canon, pad, C, f, out, theta_inv, flags_inv, chan_map, G, Cf, gidx, num_elements, B, H,
                     W, stream);
}

int eqa_orbit_expand_fwd(const float* x, float* y, const float* theta, const int32_t* flags, int num_elements, int B,
                         int C, int S, int pad, void* stream) {
  if (B == 0 && num_elements > 0) return EQA_OK;
  if (num_elements <= 0 || B <= 0) return EQA_ERR_INVALID_ARG;
  if ((long long)num_elements * B > 0x7fffffffLL) return EQA_ERR_UNSUPPORTED;
  return launch_action(x, y, nullptr, theta, flags, nullptr, num_elements, 1, num_elements * B, B, C, S, S, pad, S, S,
                       pad, pad, stream);
}

int eqa_group_action_bwd_tiles(int OH, int OW) {
  if (OH <= 0 || OW <= 0) return 0;
  return ((OH + kTile - 1) / kTile) * ((OW + kTile - 1) / kTile);
}

int eqa_group_action_bwd(const float* src, const float* grad_out, const int32_t* gidx, const float* theta,
                         const int32_t* flags, const int32_t* chan_map, float* grad_src, float* grad_angle_partial,
                         int num_elements, int G, int n_out, int B, int C, int H, int W, int pad, int OH, int OW,
                         int top, int left, void* stream) {
  return launch_action_bwd(1, src, grad_out, gidx, theta, flags, chan_map, grad_src, grad_angle_partial, num_elements, G, n_out,
                           B, C, H, W, pad, OH, OW, top, left, stream);
}

int eqa_group_action_bwd_theta(const float* src, const float* grad_out, const int32_t* gidx, const float* theta,
                               const int32_t* flags, const int32_t* chan_map, float* grad_src, float* grad_theta_partial,
                               int num_elements, int G, int n_out, int B, int C, int H, int W, int pad, int OH, int OW,
                               int top, int left, void* stream) {
  return launch_action_bwd(2, src, grad_out, gidx, theta, flags, chan_map, grad_src, grad_theta_partial, num_elements, G, n_out,
                           B, C, H, W, pad, OH, OW, top, left, stream);
}

}  // extern "C"
