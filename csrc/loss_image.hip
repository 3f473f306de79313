// Fused per-pixel training loss for a model whose output is an image (gfx950): one streaming pass over bf16
// outputs z [B][E] (E = H*W*C of the NHWC output map, viewed flat).
//
//   p        = act(z)                                   act: 0 linear, 2 sigmoid (elementwise; classifier_metrics' codes)
//   L_b      = (1/E) * sum_e loss_kind(t_be, p_be)      the mean kinds of MetricKind, codes 0..5 (csrc/loss_elem.h)
//   dz[b][e] = grad_scale * (1/E) * dloss/dp * act'     bf16, same shape as z; nullable.  out_relu: z is the
//                                                       output of a fused ReLU, whose relu' (z > 0) is applied too
//   stats[0] += sum_b L_b                               nullable (stats[1], the accuracy count, is not defined here)
//
// Reference: DistributedDynamicModel.fit minimises whatever lossesMap entry it is given on whatever the model
// outputs (src/common/models.ts); for an image-to-image model that is a mean over the output map.
//
// Targets: an fp32 table [nrows][E], or a uint8 table [nrows][E] with t = u8 * target_scale (the HBM dataset
// itself: an autoencoder's target is its input); image b reads table row idx[b] (clamped to the table) when idx
// is given, else row b.  No gather launch, no fp32 copy of the targets.
//
// Memory-bound: one read of z, one of t, one write of dz.  A workgroup works inside one image (the target
// indirection is per image) on kImageLossElems consecutive elements; the workgroup index, image included, is
// blockIdx.x.  Vector path: a lane owns 8 adjacent elements (16-byte z / dz accesses); it needs E % 8 == 0 and
// aligned base pointers, which the launcher checks; otherwise lanes stride the range element by element.
// The loss sum is bitwise reproducible: every workgroup writes one fp32 partial to the caller's workspace
// (lanes in order, wave butterfly, waves in order) and a second one-workgroup launch adds the partials in a
// fixed order to stats[0].  No float atomics, no LDS beyond the block reduction, no host synchronisation.
#include "common.h"
#include "kernels.h"
#include "loss_elem.h"

namespace dfa {
namespace {

constexpr int kSumBlock = 256;

struct ImageLossArgs {
  const bf16* z;
  const void* targets;   // fp32 or uint8 [nrows][E]
  const long long* idx;
  bf16* dz;
  float* partial;        // [B * wgs] or nullptr (no stats wanted)
  long long nrows, E, wgs;
  int kind, out_act, out_relu;
  float grad_scale, target_scale, inv_e;
};

template <bool U8>
__device__ __forceinline__ float target_at(const void* row, long long e, float scale) {
  if (U8) return (float)((const uint8_t*)row)[e] * scale;
  return ((const float*)row)[e];
}

__device__ __forceinline__ void image_loss_elem(const ImageLossArgs& a, float zv, float t, float& l, float& dzv) {
  const float p = a.out_act == 2 ? loss_sigmoid(zv) : zv;
  float g;
  loss_elem(a.kind, p, t, 0.f, 0.f, l, g);
  g *= a.inv_e;
  dzv = (a.out_act == 2 ? g * p * (1.f - p) : g) * a.grad_scale;
  if (a.out_relu && !(zv > 0.f)) dzv = 0.f;
}

template <bool VEC, bool U8>
__global__ void __launch_bounds__(256) image_loss_kernel(ImageLossArgs a) {
  __shared__ float s_part[4];
  const long long wg = blockIdx.x;
  const long long b = wg / a.wgs;
  const long long e0 = (wg - b * a.wgs) * kImageLossElems;
  const long long e1 = e0 + kImageLossElems < a.E ? e0 + kImageLossElems : a.E;
  long long r = b;
  if (a.idx) r = min(max(a.idx[b], 0ll), a.nrows - 1);  // never read outside the table
  const bf16* z = a.z + b * a.E;
  bf16* dz = a.dz ? a.dz + b * a.E : nullptr;
  const void* trow = U8 ? (const void*)((const uint8_t*)a.targets + r * a.E)
                        : (const void*)((const float*)a.targets + r * a.E);
  float sum = 0.f;
  if (VEC) {
    for (long long e = e0 + 8ll * threadIdx.x; e < e1; e += 8ll * blockDim.x) {  // E % 8 == 0: whole vectors
      const bf16x8 zv = *reinterpret_cast<const bf16x8*>(z + e);
      float t[8];
      if (U8) {
        const uint2 u = *reinterpret_cast<const uint2*>((const uint8_t*)trow + e);
#pragma unroll
        for (int j = 0; j < 4; ++j) {
          t[j] = (float)((u.x >> (8 * j)) & 0xffu) * a.target_scale;
          t[4 + j] = (float)((u.y >> (8 * j)) & 0xffu) * a.target_scale;
        }
      } else {
        const f32x4 t0 = *reinterpret_cast<const f32x4*>((const float*)trow + e);
        const f32x4 t1 = *reinterpret_cast<const f32x4*>((const float*)trow + e + 4);
#pragma unroll
        for (int j = 0; j < 4; ++j) t[j] = t0[j], t[4 + j] = t1[j];
      }
      bf16x8 out;
#pragma unroll
      for (int j = 0; j < 8; ++j) {
        float l, d;
        image_loss_elem(a, bf2f(zv[j]), t[j], l, d);
        sum += l;
        out[j] = f2bf(d);
      }
      if (dz) *reinterpret_cast<bf16x8*>(dz + e) = out;
    }
  } else {
    for (long long e = e0 + threadIdx.x; e < e1; e += blockDim.x) {
      float l, d;
      image_loss_elem(a, bf2f(z[e]), target_at<U8>(trow, e, a.target_scale), l, d);
      sum += l;
      if (dz) dz[e] = f2bf(d);
    }
  }
  if (!a.partial) return;  // uniform: no barrier is skipped by a part of the workgroup
  sum = wave_sum(sum);
  if ((threadIdx.x & 63) == 0) s_part[threadIdx.x >> 6] = sum;
  __syncthreads();
  if (threadIdx.x == 0) {
    float s = 0.f;
    for (int w = 0; w < (int)(blockDim.x >> 6); ++w) s += s_part[w];
    a.partial[wg] = s * a.inv_e;
  }
}

// stats[0] += the n partials, in a fixed order: lane i adds partials i, i + 256, ..., then the workgroup's
// 256 sums are added wave by wave.  One workgroup; plain read-modify-write of stats[0] (stream order).
__global__ void __launch_bounds__(kSumBlock) image_loss_sum_kernel(const float* __restrict__ partial, long long n,
                                                                    float* __restrict__ stats) {
  __shared__ float s_part[kSumBlock / 64];
  float s = 0.f;
  for (long long i = threadIdx.x; i < n; i += kSumBlock) s += partial[i];
  s = wave_sum(s);
  if ((threadIdx.x & 63) == 0) s_part[threadIdx.x >> 6] = s;
  __syncthreads();
  if (threadIdx.x == 0) {
    float t = 0.f;
    for (int w = 0; w < kSumBlock / 64; ++w) t += s_part[w];
    stats[0] += t;
  }
}

}  // namespace

ImageLossPlan image_loss_plan(long long B, long long E, bool aligned) {
  ImageLossPlan p{};
  if (B <= 0 || E <= 0 || E > (1ll << 40)) return p;
  p.vec = aligned && E % 8 == 0;
  p.elems_per_wg = kImageLossElems;
  p.wgs_per_image = (E + kImageLossElems - 1) / kImageLossElems;
  // lanes: one per 8 elements of the busiest workgroup, whole waves, at most four
  const long long span = E < kImageLossElems ? E : kImageLossElems;
  const long long waves = (span + 8 * kWave - 1) / (8 * kWave);
  p.threads = kWave * (int)(waves < 1 ? 1 : (waves > 4 ? 4 : waves));
  if (p.wgs_per_image > 0x7fffffffll / B) return p;  // blockIdx.x holds image and range
  p.grid = B * p.wgs_per_image;
  p.ws_floats = p.grid;
  p.ok = true;
  return p;
}

hipError_t image_loss_grad(const bf16* z, const float* t_f32, const uint8_t* t_u8, float target_scale,
                           const long long* idx, long long nrows, bf16* dz, float* stats, float* ws,
                           size_t ws_floats, long long B, long long E, int kind, int out_act, int out_relu,
                           float grad_scale, hipStream_t st) {
  if (B <= 0) return hipSuccess;
  if (!z || (t_f32 == nullptr) == (t_u8 == nullptr) || kind < 0 || kind > kMetricSigmoidCE ||
      (out_act != 0 && out_act != 2) || nrows <= 0 || (!idx && nrows < B))
    return hipErrorInvalidValue;
  if (!dz && !stats) return hipSuccess;
  const void* tp = t_f32 ? (const void*)t_f32 : (const void*)t_u8;
  // 16-byte z / dz vectors; a lane's 8 targets are 32 bytes of fp32 (two 16-byte loads) or 8 bytes of uint8
  const bool aligned = (((uintptr_t)z | (uintptr_t)dz) & 15) == 0 && ((uintptr_t)tp & (t_f32 ? 15 : 7)) == 0;
  const ImageLossPlan p = image_loss_plan(B, E, aligned);
  if (!p.ok || (stats && (!ws || ws_floats < (size_t)p.ws_floats))) return hipErrorInvalidValue;
  const ImageLossArgs a{z, tp, idx, dz, stats ? ws : nullptr, nrows, E, p.wgs_per_image, kind, out_act,
                        out_relu ? 1 : 0, grad_scale, target_scale, 1.f / (float)E};
  const dim3 grid((unsigned)p.grid), block(p.threads);
  if (p.vec && t_u8) hipLaunchKernelGGL((image_loss_kernel<true, true>), grid, block, 0, st, a);
  else if (p.vec) hipLaunchKernelGGL((image_loss_kernel<true, false>), grid, block, 0, st, a);
  else if (t_u8) hipLaunchKernelGGL((image_loss_kernel<false, true>), grid, block, 0, st, a);
  else hipLaunchKernelGGL((image_loss_kernel<false, false>), grid, block, 0, st, a);
  DFA_HIP_CHECK(hipGetLastError());
  if (stats) {
    hipLaunchKernelGGL(image_loss_sum_kernel, dim3(1), dim3(kSumBlock), 0, st, ws, p.grid, stats);
    DFA_HIP_CHECK(hipGetLastError());
  }
  return hipSuccess;
}

}  // namespace dfa
