// MFMA B fragments of the fused LeNet-5 step's conv weights (csrc/lenet_fused.hip), shared by its
// prep launch and by the optimizer (csrc/optim.hip), which rebuilds them from the weights it just
// updated so that a training step needs no separate prep launch.
//   [NFRAG][64 lanes] x 8 bf16:  conv1 banded, two kernel rows per K-step (f = ks * 3 + T, 9 fragments:
//   column n = (output x offset j = n & 7, channel 2T + (n >> 3)); k = (s, p) = 16 s + p: kernel row
//   2 ks + s, input column p = j + kx of 16, so each weight sits at 8 positions: lenet_conv1_frag_pos;
//   fragments 9 .. 14 are unused and stay zero), conv2 forward (step s: column n, k = (tap 4s + g,
//   channel e)), conv2 data gradient pair-banded (step s: column (b = j >> 3, c = j & 7),
//   k = ((ky, u), n) with kx = u - 1 + b).
// Behind them the six dense weight matrices of the step (forward [N][K] and transposed [K][N] of the
// three layers) in the same lane-linear form: a matrix M[R][C] (R = MFMA row / column index, padded to
// 16; C = reduction length, padded to 32; KS = C / 32) is tiles x KS fragments in [tile][k-step] order,
// element (r, c) in fragment (r / 16) * KS + c / 32, lane 16 * ((c % 32) / 8) + r % 16, element c % 8:
// what lane (i = r % 16, g = (c % 32) / 8) of a 16x16x32 MFMA takes as its 8 operand values.  Padding
// elements are zero.
#pragma once
#include "common.h"

namespace dfa {

constexpr int FR_C1 = 0, FR_C2 = 15, FR_DG = 22;
constexpr int NFRAG_CONV = 37;
// dense ranges: forward d1w [128][416], d2w [96][128], d3w [16][96]; transposed d3wt [96][32],
// d2wt [128][96], d1wt [400][128]
constexpr int FR_D1W = NFRAG_CONV, FR_D2W = FR_D1W + 8 * 13, FR_D3W = FR_D2W + 6 * 4, FR_D3WT = FR_D3W + 1 * 3,
              FR_D2WT = FR_D3WT + 6 * 1, FR_D1WT = FR_D2WT + 8 * 3;
constexpr int NFRAG = FR_D1WT + 25 * 4;
static_assert(NFRAG == 298, "37 conv + 261 dense fragments");

constexpr int kLeNetFragLanes = NFRAG_CONV * 64;            // conv fragment lanes (lenet_frag_lane)
constexpr int kLeNetDenseFragLanes = (NFRAG - NFRAG_CONV) * 64;
constexpr int kLeNetConvW = 2550;  // conv1 kernel [6][25] then conv2 kernel [16][150]

// conv1 fragments in use (3 K-steps of two kernel rows x 3 channel pairs); FR_C1 + kConv1Frags .. FR_C2 - 1
// are allocated and zero
constexpr int kConv1Frags = 9;
// THE position rule of the conv1 fragments: bf16 element index (into the fragment buffer) of conv1 weight
// j = (channel * 5 + ky) * 5 + kx in the band of output column offset jj (0 .. 7).  Fragment
// f = (ky >> 1) * 3 + (channel >> 1); B row k = 16 (ky & 1) + p with input column p = jj + kx (< 12), i.e.
// lane group g = 2 (ky & 1) + (p >> 3), element p & 7; B column n = 8 (channel & 1) + jj.  The gather
// (lenet_frag_lane), the scatter (lenet_frag_scatter) and the host's map (lenet_conv1_frag_map) all go
// through this function.
__host__ __device__ constexpr int lenet_conv1_frag_pos(int j, int jj) {
  const int ch = j / 25, r = j - 25 * ch, ky = r / 5, kx = r - 5 * ky, p = jj + kx;
  const int f = FR_C1 + (ky >> 1) * 3 + (ch >> 1), lane = (2 * (ky & 1) + (p >> 3)) * 16 + (ch & 1) * 8 + jj;
  return (f * 64 + lane) * 8 + (p & 7);
}

// Fragment lane fl (fragment fl / 64, lane fl % 64); W(j) = conv weight j of the 2550 above.
template <typename W>
__device__ __forceinline__ bf16x8 lenet_frag_lane(int fl, W&& wt) {
  const int f = fl >> 6, lane = fl & 63, i = lane & 15, g = lane >> 4;
  bf16x8 o;
  if (f < FR_C2) {
    // the lane's column is (channel ch, offset jj), its B rows lie in kernel row ky: the weights (ch, ky, kx)
    // whose position for jj falls into this lane
    const int ks = f / 3, T = f - 3 * (f / 3), ch = 2 * T + (i >> 3), jj = i & 7, ky = 2 * ks + (g >> 1);
    const bool live = f < FR_C1 + kConv1Frags && ky < 5;
#pragma unroll
    for (int e = 0; e < 8; ++e) {
      float v = 0.f;
#pragma unroll
      for (int kx = 0; kx < 5; ++kx) {
        const int j = live ? (ch * 5 + ky) * 5 + kx : 0;
        if (live && lenet_conv1_frag_pos(j, jj) == fl * 8 + e) v = wt(j);
      }
      o[e] = f2bf(v);
    }
  } else if (f < FR_DG) {
    const int s = f - FR_C2, tap = 4 * s + g;
#pragma unroll
    for (int e = 0; e < 8; ++e) o[e] = f2bf((tap < 25 && e < 6) ? wt(150 + i * 150 + tap * 6 + e) : 0.f);
  } else {
    const int s = f - FR_DG, P = 2 * s + (g >> 1), ky = P / 6, u = P - 6 * (P / 6);
    const int b = i >> 3, c = i & 7, kx = u - 1 + b;
    const bool ok = P < 30 && kx >= 0 && kx < 5 && c < 6;
#pragma unroll
    for (int e = 0; e < 8; ++e) {
      const int n = 8 * (g & 1) + e;
      o[e] = f2bf(ok ? wt(150 + n * 150 + (ky * 5 + kx) * 6 + c) : 0.f);
    }
  }
  return o;
}

// Inverse of lenet_frag_lane: store bf16(w) of conv weight j into every fragment element that holds it
// (conv1: 8 banded positions; conv2: 1 forward + 2 pair-banded data-gradient positions).  The update
// workgroup that owns weight j scatters it right after updating it, so the next step's fragments are
// complete when the launch ends (no last-arriver rebuild); elements that hold no weight stay zero from
// the buffer's initial build.
__device__ __forceinline__ void lenet_frag_scatter(void* frag_buf, int j, float w) {
  bf16* fr = reinterpret_cast<bf16*>(frag_buf);
  const bf16 v = f2bf(w);
  auto put = [&](int f, int lane, int e) { fr[((f * 64) + lane) * 8 + e] = v; };
  if (j < 150) {  // conv1 [c][ky][kx]
#pragma unroll
    for (int jj = 0; jj < 8; ++jj) fr[lenet_conv1_frag_pos(j, jj)] = v;
    return;
  }
  // conv2 [n][tap = ky * 5 + kx][c]
  const int q = j - 150, n = q / 150, r = q - 150 * n, tap = r / 6, c = r - 6 * tap;
  put(FR_C2 + (tap >> 2), (tap & 3) * 16 + n, c);
  const int ky = tap / 5, kx = tap - 5 * ky;
#pragma unroll
  for (int b = 0; b < 2; ++b) {
    const int P = ky * 6 + kx + 1 - b;
    put(FR_DG + (P >> 1), ((P & 1) * 2 + (n >> 3)) * 16 + b * 8 + c, n & 7);
  }
}

// ---- dense fragments.  Layer l (0 .. 2): N outputs, K inputs; the forward matrix has R = N, C = K, the
// transposed one R = K, C = N.
struct LeNetDenseFrag {
  int N, K, fw, fwt;  // first fragment of the forward / transposed matrix
};
__host__ __device__ constexpr LeNetDenseFrag lenet_dense_frag(int l) {
  return l == 0 ? LeNetDenseFrag{120, 400, FR_D1W, FR_D1WT}
                : (l == 1 ? LeNetDenseFrag{84, 120, FR_D2W, FR_D2WT} : LeNetDenseFrag{10, 84, FR_D3W, FR_D3WT});
}
// bf16 element index (into the whole fragment buffer) of element (r, c) of the matrix that starts at
// fragment f0 and has C reduction columns
__host__ __device__ constexpr int lenet_dense_frag_pos(int f0, int C, int r, int c) {
  return (((f0 + (r >> 4) * ((C + 31) >> 5) + (c >> 5)) * 64) + 16 * ((c & 31) >> 3) + (r & 15)) * 8 + (c & 7);
}
// store weight (n, k) of dense layer l (already bf16) at its forward and its transposed position
__device__ __forceinline__ void lenet_dense_frag_scatter(void* frag_buf, int l, int n, int k, bf16 v) {
  bf16* fr = reinterpret_cast<bf16*>(frag_buf);
  const LeNetDenseFrag d = lenet_dense_frag(l);
  fr[lenet_dense_frag_pos(d.fw, d.K, n, k)] = v;
  fr[lenet_dense_frag_pos(d.fwt, d.N, k, n)] = v;
}
// Dense fragment lane dl (fragment NFRAG_CONV + dl / 64, lane dl % 64) gathered from the layers' fp32
// [N][K] kernels W(l, n * K + k); padding elements are zero.
template <typename W>
__device__ __forceinline__ bf16x8 lenet_dense_frag_lane(int dl, W&& wt) {
  const int f = NFRAG_CONV + (dl >> 6), lane = dl & 63, i = lane & 15, g = lane >> 4;
  // which matrix: the ranges in buffer order
  int l, f0;
  bool tr;
  if (f < FR_D2W) l = 0, f0 = FR_D1W, tr = false;
  else if (f < FR_D3W) l = 1, f0 = FR_D2W, tr = false;
  else if (f < FR_D3WT) l = 2, f0 = FR_D3W, tr = false;
  else if (f < FR_D2WT) l = 2, f0 = FR_D3WT, tr = true;
  else if (f < FR_D1WT) l = 1, f0 = FR_D2WT, tr = true;
  else l = 0, f0 = FR_D1WT, tr = true;
  const LeNetDenseFrag d = lenet_dense_frag(l);
  const int R = tr ? d.K : d.N, C = tr ? d.N : d.K, KS = (C + 31) >> 5;
  const int q = f - f0, t = q / KS, s = q - t * KS;
  const int r = 16 * t + i;
  bf16x8 o;
#pragma unroll
  for (int e = 0; e < 8; ++e) {
    const int c = 32 * s + 8 * g + e;
    const bool ok = r < R && c < C;
    o[e] = f2bf(ok ? wt(l, tr ? c * d.K + r : r * d.K + c) : 0.f);
  }
  return o;
}

// ---- transposed dense activations / output gradients (H^T, dZ^T: train kernel writes, reduce launch reads)
// in the same operand form: [rows padded to 16][ldt batch columns] as blocks of 16 rows x 32 columns (1 KB)
// in [row tile][k-step] order, inside a block piece (col % 32) / 8, row r % 16, element col % 8 -- a
// reduce wave's operand of one row tile and k-step is one lane-linear 1 KB load.  Element index of
// (row, col) in a buffer of ldt columns (ldt % 32 == 0):
__host__ __device__ constexpr long long lenet_act_pos(int row, int col, int ldt) {
  return (((long long)(row >> 4) * (ldt >> 5) + (col >> 5)) * 64 + 16 * ((col & 31) >> 3) + (row & 15)) * 8 + (col & 7);
}

// w: the 2550 conv weights (any memory); nt threads of a block build every fragment
__device__ __forceinline__ void lenet_build_frags(const float* w, bf16x8* __restrict__ frag, int tid, int nt) {
  for (int fl = tid; fl < kLeNetFragLanes; fl += nt) frag[fl] = lenet_frag_lane(fl, [&](int j) { return w[j]; });
}

// The SGD update of one parameter with every operation rounded on its own, so the optimizer's fragment
// rebuild and the owning workgroup's update produce the same bits whatever they are inlined into.
// (HIP's __fmul_rn / __fadd_rn are plain operators that -ffp-contract may still fuse into an FMA after
// inlining; the pragma keeps the multiplies and adds created here separate.)
__device__ __forceinline__ float sgd_new_weight(float w, float gr, float m, float lr, float mom, float wd, float gs,
                                                bool nesterov, float* m_out) {
#pragma clang fp contract(off)
  float g = gr * gs;
  if (wd != 0.f) g = g + wd * w;
  if (mom != 0.f) {
    const float v = mom * m + g;
    if (m_out) *m_out = v;
    g = nesterov ? g + mom * v : v;
  }
  return w - lr * g;
}

}  // namespace dfa
