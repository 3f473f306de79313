// Depthwise 2-D convolution (Keras DepthwiseConv2D, the depthwise stage of SeparableConv2D) for gfx950:
// forward, data gradient and weight gradient over NHWC bf16 activations.
//
// Output channel co reads input channel co / M (M = depth_multiplier).  The kernel is the fp32 master
// itself, [KH][KW][C*M] = Keras' depthwise_kernel [KH, KW, C, M] flattened: a few tens of KB, L2-resident,
// so there is no bf16 compute copy.  A depthwise conv is not GEMM-shaped (one input channel per output
// channel: nothing for the MFMA K dimension to sum), so the three passes are memory-bound stencils:
//
//   * vector path (M == 1, C % 8 == 0, 16-byte aligned pointers): a lane owns 8 adjacent channels and moves
//     them as one 16-byte access; lanes of a wave are adjacent channel vectors, then adjacent columns, so a
//     wave-instruction reads whole contiguous pixel rows.  The 3x3 kernels (row stride 1 or 2) walk DOWN
//     the output rows with the 3 x 3 input window in registers: every input row is fetched once per work
//     item and serves all three kernel rows.  The stride-1 data gradient is the same walk over dY with the
//     kernel flipped; the weight gradient walks the same window against dY.
//   * every other geometry (any KH x KW, strides, M >= 1, any C) takes the generic kernels: one output
//     element (or 8 channels of it) per thread, taps in a runtime loop over cached rows.
//
// Weight gradient: dw[kh][kw][co] = sum over (b, oh, ow) of dy * x and db[co] = sum dy, in fp32, bitwise
// reproducible and without float atomics: each workgroup keeps its partial sums in registers over a
// fixed set of positions, reduces them across its position lanes through LDS in a fixed order and writes
// one slab [(KH*KW + 1)][C*M] of the caller's workspace; a second small launch sums the slabs in slab order.
// The slab count depends on the shapes only.
//
// All loops over register arrays are fully unrolled (static indices): no kernel here uses scratch
// (tests/test_depthwise_cpu.py checks the compiler's ScratchSize).
#include "common.h"
#include "kernels.h"

namespace dfa {
namespace {

constexpr int kDwBlock = 256;
constexpr int kDwMaxGrid = 2048;    // streaming passes: ~8 workgroups per CU, grid-stride the rest
constexpr int kDwMaxSlabs = 1024;   // weight-gradient workgroups (= slabs of the second launch)
constexpr int kDwRows = 8;          // output rows a 3x3 work item walks down

__device__ __forceinline__ bf16x8 zero8() {
  bf16x8 z;
#pragma unroll
  for (int j = 0; j < 8; ++j) z[j] = f2bf(0.f);
  return z;
}

// 8 channels of pixel (b, ih, iw) of an NHWC map [.][SH][SW][C], zero outside the map
__device__ __forceinline__ bf16x8 load_px8(const bf16* __restrict__ src, long long b, int ih, int iw, int SH, int SW,
                                           int C, int c0) {
  if (ih < 0 || ih >= SH || iw < 0 || iw >= SW) return zero8();
  return *reinterpret_cast<const bf16x8*>(src + ((b * SH + ih) * SW + iw) * (long long)C + c0);
}

// ---------------------------------------------------------------------------------------------------------
// 3x3 vector kernels: a work item is (image, chunk of kDwRows destination rows, destination column, channel
// vector); it walks down its rows keeping source rows ih .. ih+2 (3 pixels each) in registers.
struct Dw3Args {
  const bf16* src;    // forward: x; data gradient: dy
  bf16* dst;          // forward: y; data gradient: dx
  const float* w;     // [3][3][C]
  const float* bias;  // forward (nullable)
  const bf16* mask;   // data gradient: dx = 0 where mask <= 0 (nullable), at the destination's positions
  const bf16* dy;     // weight gradient: [B][DH][DW][C]
  float* slab;        // weight gradient: [gridDim.x][10][C]
  int B, SH, SW, DH, DW, C;  // source map, destination map (weight gradient: the positions of dy), channels
  int sw, pt, pl;            // column stride, top / left padding (row stride: template parameter)
  int nchunk, relu;
};

// rows [FROM, TO) of the window from source rows ih + FROM ..: a step keeps rows [0, 3 - SH) and loads the rest
template <int FROM, int TO>
__device__ __forceinline__ void dw3_load_rows(bf16x8 (&win)[3][3], const Dw3Args& a, long long b, int ih, int iw0,
                                              int c0) {
#pragma unroll
  for (int r = FROM; r < TO; ++r)
#pragma unroll
    for (int k = 0; k < 3; ++k) win[r][k] = load_px8(a.src, b, ih + r, iw0 + k, a.SH, a.SW, a.C, c0);
}

template <int SH>
__device__ __forceinline__ void dw3_shift(bf16x8 (&win)[3][3]) {
#pragma unroll
  for (int r = 0; r + SH < 3; ++r)
#pragma unroll
    for (int k = 0; k < 3; ++k) win[r][k] = win[r + SH][k];
}

// forward (DGRAD 0): y = [relu](bias + sum x * w); stride-1 data gradient (DGRAD 1): the same walk over dy
// with the kernel flipped and padding (2 - pt, 2 - pl) (set by the launcher), masked by relu'(x)
template <int SH, bool DGRAD>
__global__ void __launch_bounds__(kDwBlock) dw3x3_kernel(Dw3Args a) {
  const int CC = a.C / 8;
  const long long total = (long long)a.B * a.nchunk * a.DW * CC;
  float wr[3][3][8];
  float bs[8];
  int ccw = -1;
  for (long long i = blockIdx.x * (long long)kDwBlock + threadIdx.x; i < total; i += (long long)gridDim.x * kDwBlock) {
    const int cc = (int)(i % CC);
    long long t = i / CC;
    const int ow = (int)(t % a.DW);
    t /= a.DW;
    const int chunk = (int)(t % a.nchunk);
    const long long b = t / a.nchunk;
    const int c0 = cc * 8;
    if (cc != ccw) {  // this lane's 72 weights (and bias); cc changes only when the grid stride is no multiple of CC
      ccw = cc;
#pragma unroll
      for (int kh = 0; kh < 3; ++kh)
#pragma unroll
        for (int kw = 0; kw < 3; ++kw) {
          const int tap = DGRAD ? (2 - kh) * 3 + (2 - kw) : kh * 3 + kw;
          const float* p = a.w + (long long)tap * a.C + c0;
          const f32x4 lo = *reinterpret_cast<const f32x4*>(p), hi = *reinterpret_cast<const f32x4*>(p + 4);
#pragma unroll
          for (int j = 0; j < 4; ++j) { wr[kh][kw][j] = lo[j]; wr[kh][kw][4 + j] = hi[j]; }
        }
#pragma unroll
      for (int j = 0; j < 8; ++j) bs[j] = 0.f;
      if (!DGRAD && a.bias) {
        const f32x4 lo = *reinterpret_cast<const f32x4*>(a.bias + c0), hi = *reinterpret_cast<const f32x4*>(a.bias + c0 + 4);
#pragma unroll
        for (int j = 0; j < 4; ++j) { bs[j] = lo[j]; bs[4 + j] = hi[j]; }
      }
    }
    const int oh0 = chunk * kDwRows, oh1 = min(oh0 + kDwRows, a.DH);
    const int iw0 = ow * a.sw - a.pl;
    int ih = oh0 * SH - a.pt;
    bf16x8 win[3][3];
#pragma unroll
    // the rows a step keeps from the one before; written out here because through dw3_load_rows hipcc gives
    // the data-gradient variant 176 VGPRs instead of 142 (2 waves per SIMD instead of 3, measured 18 % slower)
    for (int r = 0; r < 3 - SH; ++r)
#pragma unroll
      for (int k = 0; k < 3; ++k) win[r][k] = load_px8(a.src, b, ih + r, iw0 + k, a.SH, a.SW, a.C, c0);
    for (int oh = oh0; oh < oh1; ++oh) {
      dw3_load_rows<3 - SH, 3>(win, a, b, ih, iw0, c0);
      float acc[8];
#pragma unroll
      for (int j = 0; j < 8; ++j) acc[j] = bs[j];
#pragma unroll
      for (int kh = 0; kh < 3; ++kh)
#pragma unroll
        for (int kw = 0; kw < 3; ++kw)
#pragma unroll
          for (int j = 0; j < 8; ++j) acc[j] = fmaf((float)win[kh][kw][j], wr[kh][kw][j], acc[j]);
      const long long o = ((b * a.DH + oh) * a.DW + ow) * (long long)a.C + c0;
      if (DGRAD) {
        if (a.mask) {
          const bf16x8 m = *reinterpret_cast<const bf16x8*>(a.mask + o);
#pragma unroll
          for (int j = 0; j < 8; ++j)
            if (!((float)m[j] > 0.f)) acc[j] = 0.f;
        }
      } else if (a.relu) {
#pragma unroll
        for (int j = 0; j < 8; ++j) acc[j] = fmaxf(acc[j], 0.f);
      }
      bf16x8 out;
#pragma unroll
      for (int j = 0; j < 8; ++j) out[j] = f2bf(acc[j]);
      *reinterpret_cast<bf16x8*>(a.dst + o) = out;
      dw3_shift<SH>(win);
      ih += SH;
    }
  }
}

// Cross-lane sum of one row of per-thread partials (NV values per thread) and its slab write: threads of a
// workgroup are [PL position lanes][CVB channel units]; unit u of lane p holds red[(p * CVB + u) * NV ..].
// Column r < CVB * NV (up to NV columns per thread: the row is wider than the workgroup when CVB * NV > 256) is
// summed over the lanes in lane order and written to element ch0 + r of the row.
template <int NV>
__device__ __forceinline__ void dw_slab_row(float* red, const float (&v)[NV], bool live, int CVB, int PL, float* row,
                                            int ch0, int CO) {
  const int t = threadIdx.x;
  if (live) {
#pragma unroll
    for (int j = 0; j < NV; ++j) red[t * NV + j] = v[j];
  }
  __syncthreads();
  for (int r = t; r < CVB * NV && ch0 + r < CO; r += kDwBlock) {
    float s = 0.f;
    for (int p = 0; p < PL; ++p) s += red[p * CVB * NV + r];
    row[ch0 + r] = s;
  }
  __syncthreads();
}

// 3x3 weight gradient: the forward's walk, accumulating dy * window (and dy for the bias) per lane.
// grid (slabs, channel blocks of CVB = min(C / 8, 256) vectors); block = [PL = 256 / CVB][CVB].
template <int SH>
__global__ void __launch_bounds__(kDwBlock) dw3x3_wgrad_kernel(Dw3Args a) {
  __shared__ float red[kDwBlock * 8];
  const int CC = a.C / 8;
  const int CVB = min(CC, kDwBlock), PL = kDwBlock / CVB;
  const int u = threadIdx.x % CVB, lane = threadIdx.x / CVB;
  const int cc = blockIdx.y * CVB + u;
  const bool live = lane < PL && cc < CC;
  const int c0 = cc * 8;
  float acc[3][3][8];
  float accb[8];
#pragma unroll
  for (int kh = 0; kh < 3; ++kh)
#pragma unroll
    for (int kw = 0; kw < 3; ++kw)
#pragma unroll
      for (int j = 0; j < 8; ++j) acc[kh][kw][j] = 0.f;
#pragma unroll
  for (int j = 0; j < 8; ++j) accb[j] = 0.f;
  const long long items = (long long)a.B * a.nchunk * a.DW;
  if (live) {
    for (long long q = blockIdx.x * (long long)PL + lane; q < items; q += (long long)gridDim.x * PL) {
      const int ow = (int)(q % a.DW);
      long long t = q / a.DW;
      const int chunk = (int)(t % a.nchunk);
      const long long b = t / a.nchunk;
      const int oh0 = chunk * kDwRows, oh1 = min(oh0 + kDwRows, a.DH);
      const int iw0 = ow * a.sw - a.pl;
      int ih = oh0 * SH - a.pt;
      bf16x8 win[3][3];
      dw3_load_rows<0, 3 - SH>(win, a, b, ih, iw0, c0);
      for (int oh = oh0; oh < oh1; ++oh) {
        dw3_load_rows<3 - SH, 3>(win, a, b, ih, iw0, c0);
        const bf16x8 gv = *reinterpret_cast<const bf16x8*>(a.dy + ((b * a.DH + oh) * a.DW + ow) * (long long)a.C + c0);
        float g[8];
#pragma unroll
        for (int j = 0; j < 8; ++j) { g[j] = (float)gv[j]; accb[j] += g[j]; }
#pragma unroll
        for (int kh = 0; kh < 3; ++kh)
#pragma unroll
          for (int kw = 0; kw < 3; ++kw)
#pragma unroll
            for (int j = 0; j < 8; ++j) acc[kh][kw][j] = fmaf(g[j], (float)win[kh][kw][j], acc[kh][kw][j]);
        dw3_shift<SH>(win);
        ih += SH;
      }
    }
  }
  float* slab = a.slab + (long long)blockIdx.x * 10 * a.C;
  const int ch0 = blockIdx.y * CVB * 8;
#pragma unroll
  for (int kh = 0; kh < 3; ++kh)
#pragma unroll
    for (int kw = 0; kw < 3; ++kw)
      dw_slab_row<8>(red, acc[kh][kw], live, CVB, PL, slab + (long long)(kh * 3 + kw) * a.C, ch0, a.C);
  dw_slab_row<8>(red, accb, live, CVB, PL, slab + 9LL * a.C, ch0, a.C);
}

// ---------------------------------------------------------------------------------------------------------
// Generic kernels: any KH x KW, strides, padding, depth multiplier.  VEC: M == 1, C % 8 == 0, 8 channels per
// thread; else one channel per thread.
template <bool VEC>
__global__ void __launch_bounds__(kDwBlock) dw_fwd_kernel(const bf16* __restrict__ x, const float* __restrict__ w,
                                                          const float* __restrict__ bias, bf16* __restrict__ y,
                                                          DwConvGeom g, int relu) {
  constexpr int NV = VEC ? 8 : 1;
  const int CO = g.C * g.M, CU = CO / NV;
  const long long total = (long long)g.B * g.OH * g.OW * CU;
  for (long long i = blockIdx.x * (long long)kDwBlock + threadIdx.x; i < total; i += (long long)gridDim.x * kDwBlock) {
    const int co = (int)(i % CU) * NV;
    long long t = i / CU;
    const int ow = (int)(t % g.OW);
    t /= g.OW;
    const int oh = (int)(t % g.OH);
    const long long b = t / g.OH;
    const int ci = VEC ? co : co / g.M;
    float acc[NV];
#pragma unroll
    for (int j = 0; j < NV; ++j) acc[j] = bias ? bias[co + j] : 0.f;
    const int kh0 = max(0, g.pt - oh * g.sh), kh1 = min(g.KH, g.H + g.pt - oh * g.sh);
    const int kw0 = max(0, g.pl - ow * g.sw), kw1 = min(g.KW, g.W + g.pl - ow * g.sw);
    for (int kh = kh0; kh < kh1; ++kh) {
      const int ih = oh * g.sh - g.pt + kh;
      for (int kw = kw0; kw < kw1; ++kw) {
        const int iw = ow * g.sw - g.pl + kw;
        const bf16* px = x + ((b * g.H + ih) * g.W + iw) * (long long)g.C + ci;
        const float* pw = w + (long long)(kh * g.KW + kw) * CO + co;
        if constexpr (VEC) {
          const bf16x8 v = *reinterpret_cast<const bf16x8*>(px);
          const f32x4 lo = *reinterpret_cast<const f32x4*>(pw), hi = *reinterpret_cast<const f32x4*>(pw + 4);
#pragma unroll
          for (int j = 0; j < 4; ++j) {
            acc[j] = fmaf((float)v[j], lo[j], acc[j]);
            acc[4 + j] = fmaf((float)v[4 + j], hi[j], acc[4 + j]);
          }
        } else {
          acc[0] = fmaf((float)px[0], pw[0], acc[0]);
        }
      }
    }
    if (relu) {
#pragma unroll
      for (int j = 0; j < NV; ++j) acc[j] = fmaxf(acc[j], 0.f);
    }
    if constexpr (VEC) {
      bf16x8 o;
#pragma unroll
      for (int j = 0; j < 8; ++j) o[j] = f2bf(acc[j]);
      *reinterpret_cast<bf16x8*>(y + i * 8) = o;
    } else {
      y[i] = f2bf(acc[0]);
    }
  }
}

// dx(b, ih, iw, ci) = [x > 0] * sum over taps (kh, kw) with (ih + pt - kh) % sh == 0, (iw + pl - kw) % sw == 0
// and the output position inside the map, and over the M outputs of the channel, of dy * w
template <bool VEC>
__global__ void __launch_bounds__(kDwBlock) dw_dgrad_kernel(const bf16* __restrict__ dy, const float* __restrict__ w,
                                                            const bf16* __restrict__ mask, bf16* __restrict__ dx,
                                                            DwConvGeom g) {
  constexpr int NV = VEC ? 8 : 1;
  const int CO = g.C * g.M, CU = g.C / NV;
  const long long total = (long long)g.B * g.H * g.W * CU;
  for (long long i = blockIdx.x * (long long)kDwBlock + threadIdx.x; i < total; i += (long long)gridDim.x * kDwBlock) {
    const int ci = (int)(i % CU) * NV;
    long long t = i / CU;
    const int iw = (int)(t % g.W);
    t /= g.W;
    const int ih = (int)(t % g.H);
    const long long b = t / g.H;
    float acc[NV];
#pragma unroll
    for (int j = 0; j < NV; ++j) acc[j] = 0.f;
    // the taps that reach this pixel: kh = (ih + pt) % sh, + sh, ... with oh = (ih + pt) / sh, - 1, ...
    // (ih + pt - kh == oh * sh), likewise kw / ow: one division per axis, none per tap
    const int th = ih + g.pt, tw = iw + g.pl;
    const int qh = th / g.sh, rh = th - qh * g.sh, qw = tw / g.sw, rw = tw - qw * g.sw;
    for (int kh = rh, oh = qh; kh < g.KH && oh >= 0; kh += g.sh, --oh) {
      if (oh >= g.OH) continue;
      for (int kw = rw, ow = qw; kw < g.KW && ow >= 0; kw += g.sw, --ow) {
        if (ow >= g.OW) continue;
        const bf16* pg = dy + ((b * g.OH + oh) * g.OW + ow) * (long long)CO;
        const float* pw = w + (long long)(kh * g.KW + kw) * CO;
        if constexpr (VEC) {
          const bf16x8 v = *reinterpret_cast<const bf16x8*>(pg + ci);
          const f32x4 lo = *reinterpret_cast<const f32x4*>(pw + ci), hi = *reinterpret_cast<const f32x4*>(pw + ci + 4);
#pragma unroll
          for (int j = 0; j < 4; ++j) {
            acc[j] = fmaf((float)v[j], lo[j], acc[j]);
            acc[4 + j] = fmaf((float)v[4 + j], hi[j], acc[4 + j]);
          }
        } else {
          for (int m = 0; m < g.M; ++m) acc[0] = fmaf((float)pg[ci * g.M + m], pw[ci * g.M + m], acc[0]);
        }
      }
    }
    if constexpr (VEC) {
      bf16x8 o;
      if (mask) {
        const bf16x8 mv = *reinterpret_cast<const bf16x8*>(mask + i * 8);
#pragma unroll
        for (int j = 0; j < 8; ++j)
          if (!((float)mv[j] > 0.f)) acc[j] = 0.f;
      }
#pragma unroll
      for (int j = 0; j < 8; ++j) o[j] = f2bf(acc[j]);
      *reinterpret_cast<bf16x8*>(dx + i * 8) = o;
    } else {
      if (mask && !((float)mask[i] > 0.f)) acc[0] = 0.f;
      dx[i] = f2bf(acc[0]);
    }
  }
}

// Generic weight gradient: grid (slabs, channel blocks, KH * KW taps); workgroup z sums tap z (and, for tap
// 0, the bias row) over its positions.  Slab layout as the 3x3 kernel's: [slab][KH*KW + 1][C*M].
template <bool VEC>
__global__ void __launch_bounds__(kDwBlock) dw_wgrad_kernel(const bf16* __restrict__ dy, const bf16* __restrict__ x,
                                                            float* __restrict__ slabs, DwConvGeom g) {
  constexpr int NV = VEC ? 8 : 1;
  __shared__ float red[kDwBlock * NV];
  const int CO = g.C * g.M, CU = CO / NV, T = g.KH * g.KW;
  const int CVB = min(CU, kDwBlock), PL = kDwBlock / CVB;
  const int u = threadIdx.x % CVB, lane = threadIdx.x / CVB;
  const int cu = blockIdx.y * CVB + u;
  const bool live = lane < PL && cu < CU;
  const int co = cu * NV, ci = VEC ? co : co / g.M;
  const int tap = blockIdx.z, kh = tap / g.KW, kw = tap - kh * g.KW;
  float acc[NV], accb[NV];
#pragma unroll
  for (int j = 0; j < NV; ++j) acc[j] = accb[j] = 0.f;
  const long long P = (long long)g.B * g.OH * g.OW;
  if (live) {
    for (long long p = blockIdx.x * (long long)PL + lane; p < P; p += (long long)gridDim.x * PL) {
      const int ow = (int)(p % g.OW);
      long long t = p / g.OW;
      const int oh = (int)(t % g.OH);
      const long long b = t / g.OH;
      const int ih = oh * g.sh - g.pt + kh, iw = ow * g.sw - g.pl + kw;
      const bool in = ih >= 0 && ih < g.H && iw >= 0 && iw < g.W;
      if (!in && tap != 0) continue;
      const bf16* pg = dy + p * CO + co;
      const long long xo = in ? ((b * g.H + ih) * g.W + iw) * (long long)g.C + ci : 0;
      if constexpr (VEC) {
        const bf16x8 gv = *reinterpret_cast<const bf16x8*>(pg);
        const bf16x8 xv = in ? *reinterpret_cast<const bf16x8*>(x + xo) : zero8();
#pragma unroll
        for (int j = 0; j < 8; ++j) {
          const float gj = (float)gv[j];
          accb[j] += gj;
          acc[j] = fmaf(gj, (float)xv[j], acc[j]);
        }
      } else {
        const float gj = (float)pg[0];
        accb[0] += gj;
        if (in) acc[0] = fmaf(gj, (float)x[xo], acc[0]);
      }
    }
  }
  float* slab = slabs + (long long)blockIdx.x * (T + 1) * CO;
  const int ch0 = blockIdx.y * CVB * NV;
  dw_slab_row<NV>(red, acc, live, CVB, PL, slab + (long long)tap * CO, ch0, CO);
  if (tap == 0) dw_slab_row<NV>(red, accb, live, CVB, PL, slab + (long long)T * CO, ch0, CO);
}

// gw[e] / gb[e - T*CO] = sum over the S slabs, in slab order: 16 elements x 16 slab lanes per workgroup, each
// lane sums slabs lane, lane + 16, ...; the 16 lane sums are added in lane order
__global__ void __launch_bounds__(kDwBlock) dw_wgrad_reduce_kernel(const float* __restrict__ slabs,
                                                                   float* __restrict__ gw, float* __restrict__ gb,
                                                                   int S, int TCO, int E) {
  __shared__ float red[16][16];
  const int el = threadIdx.x & 15, sl = threadIdx.x >> 4;
  const int e = blockIdx.x * 16 + el;
  float s = 0.f;
  if (e < E)
    for (int k = sl; k < S; k += 16) s += slabs[(long long)k * E + e];
  red[sl][el] = s;
  __syncthreads();
  if (sl == 0 && e < E) {
    float tot = 0.f;
#pragma unroll
    for (int k = 0; k < 16; ++k) tot += red[k][el];
    if (e < TCO) gw[e] = tot;
    else if (gb) gb[e - TCO] = tot;
  }
}

int stream_grid(long long total) {
  const long long g = (total + kDwBlock - 1) / kDwBlock;
  return (int)(g < 1 ? 1 : (g > kDwMaxGrid ? kDwMaxGrid : g));
}

// The bindings validate the geometry itself (positive sizes, padding < kernel, windows inside the padded image);
// here only what the kernels' int index math and grid dimensions need: channels < 2^24, taps < 2^16.
bool geom_ok(const DwConvGeom& g) {
  return (long long)g.C * g.M < (1LL << 24) && (long long)g.KH * g.KW < (1LL << 16);
}

bool aligned16(const void* p) { return (reinterpret_cast<uintptr_t>(p) & 15) == 0; }

// vector path: a lane owns 8 adjacent channels (16-byte bf16 accesses, two 16-byte fp32 weight reads)
bool vec_ok(const DwConvGeom& g, const void* a, const void* b, const void* c, const void* d, const void* e = nullptr) {
  return g.M == 1 && g.C % 8 == 0 && aligned16(a) && aligned16(b) && aligned16(c) && aligned16(d) && aligned16(e);
}

Dw3Args dw3_args(const DwConvGeom& g) {
  Dw3Args a{};
  a.B = g.B; a.SH = g.H; a.SW = g.W; a.DH = g.OH; a.DW = g.OW; a.C = g.C;
  a.sw = g.sw; a.pt = g.pt; a.pl = g.pl;
  a.nchunk = cdiv(g.OH, kDwRows);
  return a;
}

}  // namespace

long long dwconv_wgrad_slab_floats(const DwConvGeom& g) { return (long long)(g.KH * g.KW + 1) * g.C * g.M; }

hipError_t dwconv_fwd(const bf16* x, const float* w, const float* bias, bf16* y, const DwConvGeom& g, int relu,
                      hipStream_t st) {
  if (!geom_ok(g)) return hipErrorInvalidValue;
  const int CO = g.C * g.M;
  if (vec_ok(g, x, w, bias, y)) {
    if (g.KH == 3 && g.KW == 3 && g.sh <= 2) {
      Dw3Args a = dw3_args(g);
      a.src = x; a.dst = y; a.w = w; a.bias = bias; a.relu = relu;
      const dim3 grid(stream_grid((long long)g.B * a.nchunk * g.OW * (g.C / 8)));
      if (g.sh == 1) hipLaunchKernelGGL((dw3x3_kernel<1, false>), grid, dim3(kDwBlock), 0, st, a);
      else hipLaunchKernelGGL((dw3x3_kernel<2, false>), grid, dim3(kDwBlock), 0, st, a);
    } else {
      const dim3 grid(stream_grid((long long)g.B * g.OH * g.OW * (CO / 8)));
      hipLaunchKernelGGL(dw_fwd_kernel<true>, grid, dim3(kDwBlock), 0, st, x, w, bias, y, g, relu);
    }
  } else {
    const dim3 grid(stream_grid((long long)g.B * g.OH * g.OW * CO));
    hipLaunchKernelGGL(dw_fwd_kernel<false>, grid, dim3(kDwBlock), 0, st, x, w, bias, y, g, relu);
  }
  return hipGetLastError();
}

hipError_t dwconv_dgrad(const bf16* dy, const float* w, const bf16* mask, bf16* dx, const DwConvGeom& g,
                        hipStream_t st) {
  if (!geom_ok(g)) return hipErrorInvalidValue;
  if (vec_ok(g, dy, w, mask, dx)) {
    if (g.KH == 3 && g.KW == 3 && g.sh == 1 && g.sw == 1) {
      // dx = dy (*) flipped kernel: source dy [OH][OW], destination dx [H][W], padding (2 - pt, 2 - pl)
      Dw3Args a{};
      a.src = dy; a.dst = dx; a.w = w; a.mask = mask;
      a.B = g.B; a.SH = g.OH; a.SW = g.OW; a.DH = g.H; a.DW = g.W; a.C = g.C;
      a.sw = 1; a.pt = 2 - g.pt; a.pl = 2 - g.pl;
      a.nchunk = cdiv(g.H, kDwRows);
      const dim3 grid(stream_grid((long long)g.B * a.nchunk * g.W * (g.C / 8)));
      hipLaunchKernelGGL((dw3x3_kernel<1, true>), grid, dim3(kDwBlock), 0, st, a);
    } else {
      const dim3 grid(stream_grid((long long)g.B * g.H * g.W * (g.C / 8)));
      hipLaunchKernelGGL(dw_dgrad_kernel<true>, grid, dim3(kDwBlock), 0, st, dy, w, mask, dx, g);
    }
  } else {
    const dim3 grid(stream_grid((long long)g.B * g.H * g.W * g.C));
    hipLaunchKernelGGL(dw_dgrad_kernel<false>, grid, dim3(kDwBlock), 0, st, dy, w, mask, dx, g);
  }
  return hipGetLastError();
}

hipError_t dwconv_wgrad(const bf16* dy, const bf16* x, float* gw, float* gb, float* ws, size_t ws_floats,
                        const DwConvGeom& g, hipStream_t st) {
  if (!geom_ok(g) || !ws) return hipErrorInvalidValue;
  const int CO = g.C * g.M, T = g.KH * g.KW;
  const long long E = dwconv_wgrad_slab_floats(g);
  if (E >= (1LL << 30)) return hipErrorInvalidValue;
  const bool vec = vec_ok(g, dy, x, ws, ws);
  const int CU = vec ? CO / 8 : CO, CVB = CU < kDwBlock ? CU : kDwBlock, PL = kDwBlock / CVB;
  const bool k3 = vec && g.KH == 3 && g.KW == 3 && g.sh <= 2;
  // work items a position lane strides over: (image, row chunk, column) walks, or single positions
  const long long items = k3 ? (long long)g.B * cdiv(g.OH, kDwRows) * g.OW : (long long)g.B * g.OH * g.OW;
  // slabs: one per workgroup, as many as there is work for, capped, and they must fit the workspace
  long long S = (items + PL - 1) / PL;
  if (S > kDwMaxSlabs) S = kDwMaxSlabs;
  if (S > (long long)(ws_floats / (size_t)E)) S = (long long)(ws_floats / (size_t)E);
  if (S < 1) return hipErrorInvalidValue;  // the workspace does not hold one slab
  const dim3 block(kDwBlock);
  if (k3) {
    Dw3Args a = dw3_args(g);
    a.src = x; a.dy = dy; a.slab = ws;
    const dim3 grid((unsigned)S, cdiv(CU, CVB));
    if (g.sh == 1) hipLaunchKernelGGL(dw3x3_wgrad_kernel<1>, grid, block, 0, st, a);
    else hipLaunchKernelGGL(dw3x3_wgrad_kernel<2>, grid, block, 0, st, a);
  } else {
    const dim3 grid((unsigned)S, cdiv(CU, CVB), T);
    if (vec) hipLaunchKernelGGL(dw_wgrad_kernel<true>, grid, block, 0, st, dy, x, ws, g);
    else hipLaunchKernelGGL(dw_wgrad_kernel<false>, grid, block, 0, st, dy, x, ws, g);
  }
  DFA_HIP_CHECK(hipGetLastError());
  hipLaunchKernelGGL(dw_wgrad_reduce_kernel, dim3(cdiv((int)E, 16)), block, 0, st, ws, gw, gb, (int)S, T * CO, (int)E);
  return hipGetLastError();
}

}  // namespace dfa
