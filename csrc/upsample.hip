// Decoder-side streaming kernels for gfx950: UpSampling2D forward / backward (nearest and bilinear) and the
// per-channel sum that is the bias gradient of a transposed convolution.  NHWC bf16 activations.
//
// All three are memory bound (no reuse beyond what L2 gives the 2 x 2 bilinear footprint), so the layout is
// the one of csrc/dwconv.hip: with C % 8 == 0 and 16-byte aligned pointers a lane owns 8 adjacent channels
// and moves them as one 16-byte access, lanes of a wave are adjacent channel vectors, then adjacent columns;
// any other C takes the scalar-channel instantiation of the same kernels.
//
//   * forward: one destination pixel (x 8 channels) per work item.  Nearest copies pixel (oh / sh, ow / sw).
//     Bilinear samples at src = (dst + off) / s - off (off = 0.5: half-pixel centres, Keras / TF2; off = 0:
//     tf.js' resizeBilinear), lower index max(floor(src), 0), upper index min(ceil(src), n - 1), weight
//     src - floor(src); fp32 arithmetic, one rounding to bf16.
//   * backward: gather form, one source pixel (x 8 channels) per work item.  Nearest sums its sh x sw block;
//     bilinear walks the bounded window of destination rows / columns whose lower or upper index can be this
//     pixel, recomputing the forward's indices and weights, in row-major order.  fp32 sums, one rounding, no
//     atomics: the same bits for the same inputs.  An optional mask (the layer's input, a fused-ReLU output)
//     zeroes the gradient where it is not positive.
//   * channel_sum: gb[c] = scale * sum_m dy[m][c].  Workgroups own row ranges and write one fp32 slab [C] each
//     into the caller's workspace (register partials, combined across the workgroup's row lanes through LDS
//     in a fixed order); slab_reduce (csrc/convpool.hip) sums the slabs in slab order.  The slab count
//     depends on the shapes and the workspace size only.
//
// Loops over register arrays are fully unrolled (static indices): no kernel here uses scratch.
#include "common.h"
#include "kernels.h"

namespace dfa {
namespace {

constexpr int kUpBlock = 256;
constexpr int kUpMaxGrid = 2048;   // ~8 workgroups per CU, grid-stride the rest
constexpr int kCsMaxSlabs = 1024;  // channel_sum workgroups per channel block (= slabs of the second launch)
constexpr int kCsRowsPerLane = 16; // rows a lane sums before another slab pays

int up_grid(long long total) {
  const long long g = (total + kUpBlock - 1) / kUpBlock;
  return (int)(g < 1 ? 1 : (g > kUpMaxGrid ? kUpMaxGrid : g));
}

// lower / upper source index and the upper one's weight of destination index d (n source positions, scale s)
__device__ __forceinline__ void up_src(int d, int s, int n, float off, int& lo, int& hi, float& wt) {
  const float src = ((float)d + off) / (float)s - off;
  const float fl = floorf(src);
  lo = min(max((int)fl, 0), n - 1);
  hi = max(min((int)ceilf(src), n - 1), 0);
  wt = src - fl;
}

template <bool VEC>
__device__ __forceinline__ void up_load(const bf16* __restrict__ p, float (&v)[VEC ? 8 : 1]) {
  if (VEC) {
    const bf16x8 t = *reinterpret_cast<const bf16x8*>(p);
#pragma unroll
    for (int j = 0; j < 8; ++j) v[j] = (float)t[j];
  } else {
    v[0] = (float)p[0];
  }
}

template <bool VEC>
__device__ __forceinline__ void up_store(bf16* __restrict__ p, const float (&v)[VEC ? 8 : 1]) {
  if (VEC) {
    bf16x8 t;
#pragma unroll
    for (int j = 0; j < 8; ++j) t[j] = f2bf(v[j]);
    *reinterpret_cast<bf16x8*>(p) = t;
  } else {
    p[0] = f2bf(v[0]);
  }
}

// work item i -> (image, row, column, channel offset) of a map [B][RH][RW][C]
template <bool VEC>
__device__ __forceinline__ void up_decode(long long i, int RH, int RW, int C, long long& b, int& r, int& q, int& c0) {
  const int CC = VEC ? C / 8 : C;
  c0 = (int)(i % CC) * (VEC ? 8 : 1);
  long long t = i / CC;
  q = (int)(t % RW);
  t /= RW;
  r = (int)(t % RH);
  b = t / RH;
}

template <bool VEC, bool BIL>
__global__ void __launch_bounds__(kUpBlock) upsample2d_fwd_kernel(const bf16* __restrict__ x, bf16* __restrict__ y,
                                                                  UpGeom g) {
  constexpr int V = VEC ? 8 : 1;
  const int OH = g.H * g.sh, OW = g.W * g.sw;
  const long long total = (long long)g.B * OH * OW * (g.C / V);
  for (long long i = blockIdx.x * (long long)blockDim.x + threadIdx.x; i < total;
       i += (long long)gridDim.x * blockDim.x) {
    long long b;
    int oh, ow, c0;
    up_decode<VEC>(i, OH, OW, g.C, b, oh, ow, c0);
    const bf16* img = x + b * g.H * g.W * g.C + c0;
    float o[V];
    if (BIL) {
      int h0, h1, w0, w1;
      float wh, ww;
      up_src(oh, g.sh, g.H, g.off, h0, h1, wh);
      up_src(ow, g.sw, g.W, g.off, w0, w1, ww);
      float a[V], bq[V], c[V], d[V];
      up_load<VEC>(img + ((long long)h0 * g.W + w0) * g.C, a);
      up_load<VEC>(img + ((long long)h0 * g.W + w1) * g.C, bq);
      up_load<VEC>(img + ((long long)h1 * g.W + w0) * g.C, c);
      up_load<VEC>(img + ((long long)h1 * g.W + w1) * g.C, d);
#pragma unroll
      for (int j = 0; j < V; ++j) {
        const float top = (1.f - ww) * a[j] + ww * bq[j];
        const float bot = (1.f - ww) * c[j] + ww * d[j];
        o[j] = (1.f - wh) * top + wh * bot;
      }
    } else {
      up_load<VEC>(img + ((long long)(oh / g.sh) * g.W + ow / g.sw) * g.C, o);
    }
    up_store<VEC>(y + ((b * OH + oh) * OW + ow) * g.C + c0, o);
  }
}

template <bool VEC, bool BIL>
__global__ void __launch_bounds__(kUpBlock) upsample2d_bwd_kernel(const bf16* __restrict__ dy,
                                                                  const bf16* __restrict__ mask,
                                                                  bf16* __restrict__ dx, UpGeom g) {
  constexpr int V = VEC ? 8 : 1;
  const int OH = g.H * g.sh, OW = g.W * g.sw;
  const long long total = (long long)g.B * g.H * g.W * (g.C / V);
  for (long long i = blockIdx.x * (long long)blockDim.x + threadIdx.x; i < total;
       i += (long long)gridDim.x * blockDim.x) {
    long long b;
    int h, w, c0;
    up_decode<VEC>(i, g.H, g.W, g.C, b, h, w, c0);
    const bf16* img = dy + b * OH * OW * g.C + c0;
    float acc[V];
#pragma unroll
    for (int j = 0; j < V; ++j) acc[j] = 0.f;
    if (BIL) {
      // destination rows whose lower or upper index can be h: src in (h - 1, h + 1), or clamped onto an edge
      // row; every candidate recomputes the forward's indices, so a row outside the set contributes nothing
      const int r_lo = max((h - 1) * g.sh, 0), r_hi = min((h + 2) * g.sh, OH - 1);
      const int q_lo = max((w - 1) * g.sw, 0), q_hi = min((w + 2) * g.sw, OW - 1);
      for (int oh = r_lo; oh <= r_hi; ++oh) {
        int lo, hi;
        float wt;
        up_src(oh, g.sh, g.H, g.off, lo, hi, wt);
        const float ah = (lo == h ? 1.f - wt : 0.f) + (hi == h ? wt : 0.f);
        if (lo != h && hi != h) continue;
        for (int ow = q_lo; ow <= q_hi; ++ow) {
          up_src(ow, g.sw, g.W, g.off, lo, hi, wt);
          const float aw = (lo == w ? 1.f - wt : 0.f) + (hi == w ? wt : 0.f);
          if (lo != w && hi != w) continue;
          float v[V];
          up_load<VEC>(img + ((long long)oh * OW + ow) * g.C, v);
          const float a = ah * aw;
#pragma unroll
          for (int j = 0; j < V; ++j) acc[j] += a * v[j];
        }
      }
    } else {
      for (int r = 0; r < g.sh; ++r)
        for (int q = 0; q < g.sw; ++q) {
          float v[V];
          up_load<VEC>(img + ((long long)(h * g.sh + r) * OW + (w * g.sw + q)) * g.C, v);
#pragma unroll
          for (int j = 0; j < V; ++j) acc[j] += v[j];
        }
    }
    const long long o = ((b * g.H + h) * g.W + w) * g.C + c0;
    if (mask) {
      float m[V];
      up_load<VEC>(mask + o, m);
#pragma unroll
      for (int j = 0; j < V; ++j)
        if (!(m[j] > 0.f)) acc[j] = 0.f;
    }
    up_store<VEC>(dx + o, acc);
  }
}

// Slab s = blockIdx.x holds the sums of rows [s * rows_per, (s + 1) * rows_per) for every channel.  The 256
// lanes are R row lanes x CW channel units (CW a power of two, V channels per unit): lane (r, cw) sums rows
// r, r + R, ... of its range, then row lane 0 adds the R partials in row-lane order.
template <int V>
__global__ void __launch_bounds__(kUpBlock) channel_sum_kernel(const bf16* __restrict__ dy, float* __restrict__ slabs,
                                                               long long M, int C, int CW, int rows_per) {
  __shared__ float red[kUpBlock][V];
  const int R = kUpBlock / CW;
  const int cw = threadIdx.x % CW, r = threadIdx.x / CW;
  const int c0 = (blockIdx.y * CW + cw) * V;
  const long long m0 = (long long)blockIdx.x * rows_per;
  const long long m1 = m0 + rows_per < M ? m0 + rows_per : M;
  float acc[2][V];
#pragma unroll
  for (int j = 0; j < V; ++j) acc[0][j] = acc[1][j] = 0.f;
  if (c0 < C) {
    long long m = m0 + r;
    for (; m + R < m1; m += 2 * R) {  // two independent loads in flight
      float u[V], v[V];
      up_load<V == 8>(dy + m * C + c0, u);
      up_load<V == 8>(dy + (m + R) * C + c0, v);
#pragma unroll
      for (int j = 0; j < V; ++j) acc[0][j] += u[j], acc[1][j] += v[j];
    }
    if (m < m1) {
      float u[V];
      up_load<V == 8>(dy + m * C + c0, u);
#pragma unroll
      for (int j = 0; j < V; ++j) acc[0][j] += u[j];
    }
  }
#pragma unroll
  for (int j = 0; j < V; ++j) red[threadIdx.x][j] = acc[0][j] + acc[1][j];
  __syncthreads();
  if (r == 0 && c0 < C) {
    float s[V];
#pragma unroll
    for (int j = 0; j < V; ++j) s[j] = 0.f;
    for (int q = 0; q < R; ++q) {
#pragma unroll
      for (int j = 0; j < V; ++j) s[j] += red[q * CW + cw][j];
    }
#pragma unroll
    for (int j = 0; j < V; ++j) slabs[(long long)blockIdx.x * C + c0 + j] = s[j];
  }
}

bool up_ok(const UpGeom& g) {
  return g.B > 0 && g.H > 0 && g.W > 0 && g.C > 0 && g.sh > 0 && g.sw > 0 && (g.off == 0.f || g.off == 0.5f) &&
         (long long)g.H * g.sh < (1LL << 30) && (long long)g.W * g.sw < (1LL << 30);
}

bool up_vec(const UpGeom& g, const void* a, const void* b, const void* c) {
  return g.C % 8 == 0 && (((uintptr_t)a | (uintptr_t)b | (uintptr_t)c) & 15) == 0;
}

}  // namespace

hipError_t upsample2d_fwd(const bf16* x, bf16* y, const UpGeom& g, hipStream_t st) {
  if (!up_ok(g)) return hipErrorInvalidValue;
  const bool vec = up_vec(g, x, y, nullptr);
  const long long total = (long long)g.B * g.H * g.sh * g.W * g.sw * (vec ? g.C / 8 : g.C);
  const dim3 grid(up_grid(total)), block(kUpBlock);
  if (vec && g.bilinear) hipLaunchKernelGGL((upsample2d_fwd_kernel<true, true>), grid, block, 0, st, x, y, g);
  else if (vec) hipLaunchKernelGGL((upsample2d_fwd_kernel<true, false>), grid, block, 0, st, x, y, g);
  else if (g.bilinear) hipLaunchKernelGGL((upsample2d_fwd_kernel<false, true>), grid, block, 0, st, x, y, g);
  else hipLaunchKernelGGL((upsample2d_fwd_kernel<false, false>), grid, block, 0, st, x, y, g);
  return hipGetLastError();
}

hipError_t upsample2d_bwd(const bf16* dy, const bf16* mask, bf16* dx, const UpGeom& g, hipStream_t st) {
  if (!up_ok(g)) return hipErrorInvalidValue;
  const bool vec = up_vec(g, dy, dx, mask);
  const long long total = (long long)g.B * g.H * g.W * (vec ? g.C / 8 : g.C);
  const dim3 grid(up_grid(total)), block(kUpBlock);
  if (vec && g.bilinear) hipLaunchKernelGGL((upsample2d_bwd_kernel<true, true>), grid, block, 0, st, dy, mask, dx, g);
  else if (vec) hipLaunchKernelGGL((upsample2d_bwd_kernel<true, false>), grid, block, 0, st, dy, mask, dx, g);
  else if (g.bilinear) hipLaunchKernelGGL((upsample2d_bwd_kernel<false, true>), grid, block, 0, st, dy, mask, dx, g);
  else hipLaunchKernelGGL((upsample2d_bwd_kernel<false, false>), grid, block, 0, st, dy, mask, dx, g);
  return hipGetLastError();
}

hipError_t channel_sum(const bf16* dy, float* gb, float* ws, size_t ws_floats, long long M, int C, float scale,
                       hipStream_t st) {
  if (M <= 0 || C <= 0 || C > (1 << 20) || M > (1LL << 40) || ws_floats < (size_t)C) return hipErrorInvalidValue;
  const bool vec = C % 8 == 0 && ((uintptr_t)dy & 15) == 0;
  const int units = vec ? C / 8 : C;
  int CW = 1;
  while (CW < units && CW < kUpBlock) CW *= 2;
  const int R = kUpBlock / CW;
  long long S = (M + (long long)R * kCsRowsPerLane - 1) / ((long long)R * kCsRowsPerLane);
  if (S > kCsMaxSlabs) S = kCsMaxSlabs;
  if (S > (long long)(ws_floats / (size_t)C)) S = (long long)(ws_floats / (size_t)C);
  const long long rows_per = (M + S - 1) / S;
  if (rows_per >= (1LL << 31)) return hipErrorInvalidValue;
  S = (M + rows_per - 1) / rows_per;  // no empty slab
  const dim3 grid((unsigned)S, (unsigned)cdiv(units, CW)), block(kUpBlock);
  if (vec) hipLaunchKernelGGL(channel_sum_kernel<8>, grid, block, 0, st, dy, ws, M, C, CW, (int)rows_per);
  else hipLaunchKernelGGL(channel_sum_kernel<1>, grid, block, 0, st, dy, ws, M, C, CW, (int)rows_per);
  DFA_HIP_CHECK(hipGetLastError());
  return slab_reduce(ws, gb, nullptr, 1, C, C, (int)S, scale, st);
}

}  // namespace dfa
