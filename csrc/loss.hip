// Fused training loss for any lossesMap entry (gfx950): one launch turns fp32 model outputs z [B][ldl]
// (C columns used) into the per-row loss, its gradient w.r.t. z and the accuracy count.
//
//   p = act(z)                          act: 0 linear, 1 softmax over the row, 2 sigmoid (classifier_metrics' encoding)
//   L_b = loss_kind(t_b, p_b)           MetricKind; the definitions of distriflow_amd/losses.py, which csrc/metrics.hip
//                                       reports: evaluate()[0] is the objective minimised here
//   dlogits[b][c] = grad_scale * dL_b/dz_bc   (bf16, ld = ldg; a pure function of row b: deterministic)
//   stats[0] += sum_b L_b ; stats[1] += #correct                  (fp32 atomics, as softmax_ce)
//
// Reference: DistributedDynamicModel.fit minimises whatever lossesMap entry it is given (src/common/models.ts;
// lossesMap: src/common/utils.ts:19-30), where DistributedTfModel.fit hard-codes softmax cross-entropy.
//
// Targets: int32 labels (one-hot, clamped to [0, C-1]) or dense fp32 rows [.][ldt]; either is read through
// idx (int64 [B], clamped to the table's rows) when given, the LabelRef convention: a dataset-bound step needs
// no gather launch.  "Correct": argmax z == label, or == argmax t for dense targets; the first maximum wins.
//
// With g_c = dL_b/dp_c:  linear dz = g;  sigmoid dz_c = g_c p_c (1 - p_c);  softmax dz_c = p_c (g_c - sum_k g_k p_k).
// Nothing of a row is kept between passes (no bound on C): a row is re-read from L1/L2 up to five times.
// Row-per-thread for C <= 32, wave-per-row (four rows per workgroup, lanes striding the row) above.
#include "common.h"
#include "kernels.h"
#include "loss_elem.h"

namespace dfa {
namespace {

struct LossArgs {
  const float* z;
  const int* labels;
  const float* targets;
  const long long* idx;
  bf16* dlogits;
  float* stats;
  long long nrows;  // rows of the label / target table
  int B, C, ldl, ldt, ldg, kind, out_act;
  float grad_scale;
};

// One row by one thread (WAVE false) or by the 64 lanes of a wave (WAVE true); returns the row's loss and
// whether it is correct (every lane of a wave holds both).
template <bool WAVE>
__device__ __forceinline__ void loss_row(const LossArgs& a, int b, float& loss, float& corr) {
  const int c0 = WAVE ? (int)(threadIdx.x & 63) : 0;
  constexpr int cs = WAVE ? 64 : 1;
  const int C = a.C, kind = a.kind, act = a.out_act;
  const float* z = a.z + (long long)b * a.ldl;
  long long r = b;
  if (a.idx) r = min(max(a.idx[b], 0ll), a.nrows - 1);  // never read outside the table
  const float* t = a.targets ? a.targets + r * a.ldt : nullptr;

  // pass 1: max / first argmax of z, and of the dense targets; sum t
  float mx = -INFINITY, tmx = -INFINITY, tsum = 0.f;
  int am = 0x7fffffff, tam = 0x7fffffff;
  for (int c = c0; c < C; c += cs) {
    const float v = z[c];
    if (v > mx) { mx = v; am = c; }
    if (t) {
      const float tv = t[c];
      tsum += tv;
      if (tv > tmx) { tmx = tv; tam = c; }
    }
  }
  if (WAVE) {
    for (int off = 32; off > 0; off >>= 1) {
      const float om = __shfl_xor(mx, off, 64), otm = __shfl_xor(tmx, off, 64);
      const int oa = __shfl_xor(am, off, 64), ota = __shfl_xor(tam, off, 64);
      if (om > mx || (om == mx && oa < am)) { mx = om; am = oa; }
      if (otm > tmx || (otm == tmx && ota < tam)) { tmx = otm; tam = ota; }
    }
    tsum = wave_sum(tsum);
  }
  int y = -1;  // the one-hot class (int labels)
  if (!t) {
    y = min(max(a.labels[r], 0), C - 1);
    tam = y;
    tsum = 1.f;
  }
  corr = am == tam ? 1.f : 0.f;

  // pass 2 (softmax output): sum of exponentials
  float inv = 1.f;
  if (act == 1) {
    float se = 0.f;
    for (int c = c0; c < C; c += cs) se += expf(z[c] - mx);
    if (WAVE) se = wave_sum(se);
    inv = 1.f / se;
  }
  auto prob = [&](float v) -> float {
    return act == 1 ? expf(v - mx) * inv : (act == 2 ? 1.f / (1.f + expf(-v)) : v);
  };

  // pass 3 (softmaxCrossEntropy): log sum exp of the outputs; their maximum is act(max z), act being monotonic
  float lse = 0.f;
  if (kind == kMetricSoftmaxCE) {
    const float m2 = prob(mx);
    float s2 = 0.f;
    for (int c = c0; c < C; c += cs) s2 += expf(prob(z[c]) - m2);
    if (WAVE) s2 = wave_sum(s2);
    lse = m2 + logf(s2);
  }

  // pass 4: the loss and sum_k g_k p_k
  const float scale = kind <= kMetricSigmoidCE ? 1.f / (float)C : 1.f;  // the mean-over-classes kinds
  float l = 0.f, gp = 0.f;
  for (int c = c0; c < C; c += cs) {
    const float p = prob(z[c]);
    const float tv = t ? t[c] : (c == y ? 1.f : 0.f);
    float le, g;
    loss_elem(kind, p, tv, lse, tsum, le, g);
    l += le;
    gp += g * p;
  }
  if (WAVE) {
    l = wave_sum(l);
    gp = wave_sum(gp);
  }
  loss = l * scale;
  gp *= scale;

  // pass 5: dL/dz
  if (a.dlogits) {
    bf16* dl = a.dlogits + (long long)b * a.ldg;
    for (int c = c0; c < C; c += cs) {
      const float p = prob(z[c]);
      const float tv = t ? t[c] : (c == y ? 1.f : 0.f);
      float le, g;
      loss_elem(kind, p, tv, lse, tsum, le, g);
      g *= scale;
      const float dz = act == 1 ? p * (g - gp) : (act == 2 ? g * p * (1.f - p) : g);
      dl[c] = f2bf(dz * a.grad_scale);
    }
  }
}

__global__ void __launch_bounds__(256) loss_grad_small_kernel(LossArgs a) {
  __shared__ float s_loss[4], s_corr[4];
  const int b = blockIdx.x * blockDim.x + threadIdx.x;
  float loss = 0.f, corr = 0.f;
  if (b < a.B) loss_row<false>(a, b, loss, corr);
  loss = wave_sum(loss);
  corr = wave_sum(corr);
  const int lane = threadIdx.x & 63, wid = threadIdx.x >> 6;
  if (lane == 0) { s_loss[wid] = loss; s_corr[wid] = corr; }
  __syncthreads();
  if (threadIdx.x == 0 && a.stats) {
    float l = 0.f, c = 0.f;
    for (int w = 0; w < 4; ++w) { l += s_loss[w]; c += s_corr[w]; }
    atomicAdd(&a.stats[0], l);
    atomicAdd(&a.stats[1], c);
  }
}

__global__ void __launch_bounds__(256) loss_grad_wave_kernel(LossArgs a) {
  const int b = blockIdx.x * 4 + (threadIdx.x >> 6);
  if (b >= a.B) return;  // whole waves leave together
  float loss, corr;
  loss_row<true>(a, b, loss, corr);
  if ((threadIdx.x & 63) == 0 && a.stats) {
    atomicAdd(&a.stats[0], loss);
    atomicAdd(&a.stats[1], corr);
  }
}

}  // namespace

hipError_t loss_grad(const float* z, const int* labels, const float* targets, const long long* idx, long long nrows,
                     bf16* dlogits, float* stats, int B, int C, int ldl, int ldt, int ldg, int kind, int out_act,
                     float grad_scale, hipStream_t st) {
  if (B <= 0) return hipSuccess;
  if (C <= 0 || ldl < C || ldg < C || kind < 0 || kind > kMetricCategoricalCE || out_act < 0 || out_act > 2 ||
      nrows <= 0 || (labels == nullptr) == (targets == nullptr) || (targets && ldt < C) || (!idx && nrows < B))
    return hipErrorInvalidValue;
  const LossArgs a{z, labels, targets, idx, dlogits, stats, nrows, B, C, ldl, ldt, ldg, kind, out_act, grad_scale};
  if (C <= 32)
    hipLaunchKernelGGL(loss_grad_small_kernel, dim3(cdiv(B, 256)), dim3(256), 0, st, a);
  else
    hipLaunchKernelGGL(loss_grad_wave_kernel, dim3(cdiv(B, 4)), dim3(256), 0, st, a);
  return hipGetLastError();
}

}  // namespace dfa
