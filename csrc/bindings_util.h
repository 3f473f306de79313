// Shared by the csrc/bindings_*.cpp translation units of module distriflow_amd._C.
//
// Every entry point validates shapes/dtypes/devices on the host BEFORE launching (a bad launch
// on a shared MI355X node can reset all GPUs), then launches on PyTorch's current HIP stream so
// the calls compose with torch.cuda graph capture and RCCL collectives on the same stream.
#pragma once
#include <torch/extension.h>
#include <c10/hip/HIPStream.h>
#include <c10/hip/HIPGuard.h>
#include <hip/hip_runtime_api.h>

#include "kernels.h"

namespace dfa_py {

inline hipStream_t cur_stream() { return c10::hip::getCurrentHIPStream().stream(); }

inline void check_hip(hipError_t e, const char* what) {
  TORCH_CHECK(e == hipSuccess, "distriflow_amd kernel '", what, "' failed: ", hipGetErrorString(e));
}

inline void need(const torch::Tensor& t, at::ScalarType dt, const char* name) {
  TORCH_CHECK(t.is_cuda(), name, " must be a GPU tensor");
  TORCH_CHECK(t.scalar_type() == dt, name, " has dtype ", t.scalar_type(), ", expected ", dt);
  TORCH_CHECK(t.is_contiguous(), name, " must be contiguous");
}

inline bool has(const c10::optional<torch::Tensor>& t) { return t.has_value() && t->defined(); }

template <typename T>
const T* cptr(const c10::optional<torch::Tensor>& t) {
  return has(t) ? reinterpret_cast<const T*>(t->data_ptr()) : nullptr;
}

// optional tensor: absent -> null; present -> need(dt, name), at least `min_numel` elements (else `small`)
template <typename T>
T* opt_ptr(const c10::optional<torch::Tensor>& t, at::ScalarType dt, const char* name, int64_t min_numel = 0, const char* small = "") {
  if (!has(t)) return nullptr;
  need(*t, dt, name);
  TORCH_CHECK(t->numel() >= min_numel, small);
  return reinterpret_cast<T*>(t->data_ptr());
}

// Conv geometry [SH, SW, SC, OH, OW, KH, KW, stride, pad(, stride_w, pad_w)] (the launch's source / output
// dims: for the data gradient the source is dY and the output dX).  stride / pad are the row stride and the
// top padding; the output size may imply more padding at the bottom / right than at the top / left (Keras
// 'same' with an odd total).  Anything but one stride, one symmetric padding and a square kernel is
// 'irregular': the specialised kernels refuse it and the generic implicit GEMM runs.
template <typename A>
void set_conv_geom(A& a, const std::vector<int64_t>& geom, int mode) {
  TORCH_CHECK(geom.size() == 9 || geom.size() == 11, "geometry must have 9 or 11 ints");
  int g[11];
  for (size_t i = 0; i < geom.size(); ++i) g[i] = (int)geom[i];
  if (geom.size() == 9) g[9] = g[7], g[10] = g[8];
  a.SH = g[0]; a.SW = g[1]; a.SC = g[2]; a.OH = g[3]; a.OW = g[4]; a.KH = g[5]; a.KW = g[6];
  a.stride = g[7]; a.pad = g[8]; a.stride_w = g[9]; a.pad_w = g[10];
  a.irregular = 0;
  if (mode == dfa::MODE_DIRECT) return;
  TORCH_CHECK(a.stride >= 1 && a.stride_w >= 1 && a.pad >= 0 && a.pad_w >= 0 && a.KH >= 1 && a.KW >= 1,
              "conv geometry: stride >= 1, pad >= 0");
  const bool fwd = mode == dfa::MODE_FWD;
  const int ih = fwd ? a.SH : a.OH, iw = fwd ? a.SW : a.OW, oh = fwd ? a.OH : a.SH, ow = fwd ? a.OW : a.SW;
  a.irregular = a.KH != a.KW || a.stride_w != a.stride || a.pad_w != a.pad ||
                oh != (ih + 2 * a.pad - a.KH) / a.stride + 1 || ow != (iw + 2 * a.pad - a.KW) / a.stride + 1;
}

inline dfa::DropSpec drop_from(double p, int64_t seed, const c10::optional<torch::Tensor>& step, int64_t step_add) {
  TORCH_CHECK(p >= 0.0 && p < 1.0, "dropout p must be in [0,1)");
  const long long* sp = opt_ptr<const long long>(step, at::kLong, "dropout step");
  return dfa::make_drop((float)p, (unsigned long long)seed, sp, (int)step_add);
}
}  // namespace dfa_py
