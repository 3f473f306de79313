// Element formulas of the lossesMap losses, shared by the training-loss kernels: csrc/loss.hip (fp32 rows of
// a Dense output) and csrc/loss_image.hip (bf16 output maps).  The definitions of distriflow_amd/losses.py.
#pragma once
#include "common.h"
#include "kernels.h"

namespace dfa {

constexpr float kLossEps = 1e-7f;

__device__ __forceinline__ float loss_sgn(float d) { return d > 0.f ? 1.f : (d < 0.f ? -1.f : 0.f); }

// the sigmoid output activation of both kernels
__device__ __forceinline__ float loss_sigmoid(float v) { return 1.f / (1.f + expf(-v)); }

// loss term and dL/dp of one element, before the 1/C of the mean kinds.  lse / tsum: log sum exp(p) and
// sum t of the row (softmaxCrossEntropy only).
__device__ __forceinline__ void loss_elem(int kind, float p, float t, float lse, float tsum, float& l, float& g) {
  const float d = p - t;
  switch (kind) {
    case kMetricMSE:
      l = d * d;
      g = 2.f * d;
      break;
    case kMetricAbs:
      l = fabsf(d);
      g = loss_sgn(d);
      break;
    case kMetricHinge: {
      const float s = 2.f * t - 1.f, m = 1.f - s * p;
      l = fmaxf(m, 0.f);
      g = m > 0.f ? -s : 0.f;
      break;
    }
    case kMetricHuber: {
      const float a = fabsf(d);
      l = a <= 1.f ? 0.5f * d * d : a - 0.5f;
      g = a <= 1.f ? d : loss_sgn(d);
      break;
    }
    case kMetricLog:
      l = -(t * logf(p + kLossEps) + (1.f - t) * logf(1.f - p + kLossEps));
      g = -t / (p + kLossEps) + (1.f - t) / (1.f - p + kLossEps);
      break;
    case kMetricSigmoidCE:
      l = fmaxf(p, 0.f) - p * t + log1pf(expf(-fabsf(p)));
      g = 1.f / (1.f + expf(-p)) - t;
      break;
    case kMetricSoftmaxCE:
      l = -t * (p - lse);
      g = expf(p - lse) * tsum - t;
      break;
    default:  // kMetricCategoricalCE
      l = -t * logf(fminf(fmaxf(p, kLossEps), 1.f));
      g = (p >= kLossEps && p <= 1.f) ? -t / p : 0.f;
      break;
  }
}

}  // namespace dfa
