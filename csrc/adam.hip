// Fused multi-tensor Adam / AdamW (gfx950): one launch updates every parameter of the model.
//
// The same launch shape as sgd_multi (csrc/optim.hip): the same descriptors, the same grid (1024 elements
// or one 32 x 32 tile per workgroup), the same bf16 compute copies through multi_tensor_body /
// emit_copies (csrc/optim_device.h), and the same extra workgroup that stages the next step's batch
// indices and accumulates the run statistics.  What differs is the per-element update and its state:
//   hyper (fp32, device) = [lr, beta1, beta2, eps, weight_decay, grad_scale, decoupled, 1-beta1, 1-beta2]
//     g = grad_scale * grad            (+ wd * w when not decoupled: L2, "adam")
//     m = beta1 * m + (1 - beta1) * g
//     v = beta2 * v + (1 - beta2) * g * g
//     w = w - lr * (m / c1) / (sqrt(v / c2) + eps)      c = 1 - beta^t, the bias corrections
//     decoupled ("adamw"): w is first multiplied by (1 - lr * wd)
//   every operation rounded on its own (no FMA contraction), as sgd_new_weight (csrc/lenet_frag.h).
//   1 - beta travels as its own fp32 value (rounded from the host's double): 1.f - 0.999f is 1.3e-5 off
//   0.001, which would be a different optimizer.
//
// Step state (device, 4 x 64 bit) = [c1, c2 (doubles), t, ticket].  The bias corrections of step t + 1
// are c' = (1 - beta) + beta * c in double, from c = 0: every workgroup computes them from the state it
// reads at entry, and the launch itself advances the state, so a replayed step graph (or a multi-step
// graph) takes the right correction on every replay with no host write and no extra launch.  No
// workgroup waits on another: each takes a ticket when it has read the state, and the one that takes
// the last ticket stores c', t + 1 and resets the ticket.  Every read of the state therefore precedes
// its only write, and the next launch (stream order) sees the advanced state.
//
// The tickets are relaxed device-scope atomics in two levels: workgroup b counts in ticket word
// b % kAdamTicketGroups (one 512-byte-strided word per group), the last of a group counts in the state's
// ticket word, and the last group advances the state.  One word for all would serialize a device-scope
// read-modify-write per workgroup on one address (11 k of them for ResNet-18), and release / acquire
// tickets would add a device-scope cache write-back per workgroup; neither is needed, because a
// workgroup's state loads have completed (their values are in LDS) before it issues its ticket, and a
// completed load cannot observe a later store.
//
// Not here: the LeNet-5 fragment workgroups (their rebuild recomputes the SGD update; under Adam the
// store reports the fragments stale and the next fused train step runs its prep kernel) and the async
// parameter server's gate / mirror.
#include "common.h"
#include "kernels.h"
#include "optim_device.h"

namespace dfa {

struct AdamCoef {
  float lr, b1, b2, eps, wd, gs, omb1, omb2, c1, c2;
  bool decoupled;
};

__device__ __forceinline__ float adam_new_weight(float w, float gr, float m, float v, const AdamCoef& c,
                                                 float* m_out, float* v_out) {
#pragma clang fp contract(off)
  float g = gr * c.gs;
  if (c.wd != 0.f) {
    if (c.decoupled) w = w * (1.f - c.lr * c.wd);
    else g = g + c.wd * w;
  }
  const float mn = c.b1 * m + c.omb1 * g;
  const float vn = c.b2 * v + (c.omb2 * g) * g;
  *m_out = mn;
  *v_out = vn;
  return w - (c.lr * (mn / c.c1)) / (sqrtf(vn / c.c2) + c.eps);
}

// the bias corrections of the step after the one whose corrections are (c1, c2)
__device__ __forceinline__ double adam_next_corr(double c, float beta, float omb) {
#pragma clang fp contract(off)
  return (double)omb + (double)beta * c;
}

template <bool INL>
__global__ void __launch_bounds__(256) adam_multi_kernel(const ParamDesc* __restrict__ descs,
                                                         const ParamDescTable tab, int ndesc,
                                                         float* __restrict__ master, const float* __restrict__ grad,
                                                         float* __restrict__ m_buf, float* __restrict__ v_buf,
                                                         bf16* __restrict__ wbf, const float* __restrict__ hyper,
                                                         unsigned long long* state,
                                                         unsigned long long* tickets, int total_blocks,
                                                         IndexStream is) {
  if ((int)blockIdx.x >= total_blocks) {
    index_stream_body(is);  // the single index-stream / run-statistics workgroup
    return;
  }
  // thread 0 reads the step state and hands it to the workgroup through LDS: its loads have completed
  // (their values are stored) before any thread passes the barrier, so the ticket it takes at the end
  // is taken after every read of the state by this workgroup
  __shared__ double corr[2];
  double n1 = 0., n2 = 0.;
  unsigned long long t = 0;
  if (threadIdx.x == 0) {
    const double c1 = __longlong_as_double((long long)__hip_atomic_load(state + 0, __ATOMIC_RELAXED,
                                                                        __HIP_MEMORY_SCOPE_AGENT));
    const double c2 = __longlong_as_double((long long)__hip_atomic_load(state + 1, __ATOMIC_RELAXED,
                                                                        __HIP_MEMORY_SCOPE_AGENT));
    t = __hip_atomic_load(state + 2, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    n1 = adam_next_corr(c1, hyper[1], hyper[7]);
    n2 = adam_next_corr(c2, hyper[2], hyper[8]);
    corr[0] = n1;
    corr[1] = n2;
  }
  __syncthreads();
  AdamCoef c;
  c.lr = hyper[0], c.b1 = hyper[1], c.b2 = hyper[2], c.eps = hyper[3], c.wd = hyper[4], c.gs = hyper[5];
  c.decoupled = hyper[6] != 0.f;
  c.omb1 = hyper[7], c.omb2 = hyper[8];
  c.c1 = (float)corr[0], c.c2 = (float)corr[1];
  auto update = [&](const ParamDesc& d) {
    return [&, off = d.off](int i) -> float {
      float mn, vn;
      const float w = adam_new_weight(master[off + i], grad[off + i], m_buf[off + i], v_buf[off + i], c, &mn, &vn);
      m_buf[off + i] = mn;
      v_buf[off + i] = vn;
      master[off + i] = w;
      return w;
    };
  };
  if (INL) {
    const ParamDesc d = tab.d[find_desc(tab.d, ndesc, blockIdx.x)];
    multi_tensor_body(d, wbf, blockIdx.x, update(d));
  } else {
    const ParamDesc d = descs[find_desc(descs, ndesc, blockIdx.x)];
    multi_tensor_body(d, wbf, blockIdx.x, update(d));
  }
  if (threadIdx.x == 0) {
    // (thread 0 passed the barrier above after storing the loaded state to LDS: its loads are complete)
    const int grp = blockIdx.x % kAdamTicketGroups;
    const int in_grp = (total_blocks - 1 - grp) / kAdamTicketGroups + 1;  // workgroups b with b % groups == grp
    unsigned long long* tw = tickets + (size_t)grp * kAdamTicketStride;
    if (__hip_atomic_fetch_add(tw, 1ull, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) !=
        (unsigned long long)in_grp - 1)
      return;
    __hip_atomic_store(tw, 0ull, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    const int ngroups = min(total_blocks, kAdamTicketGroups);
    const unsigned long long tk = __hip_atomic_fetch_add(state + 3, 1ull, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    if (tk == (unsigned long long)ngroups - 1) {  // the last arriver: every workgroup has read the state
      __hip_atomic_store(state + 0, (unsigned long long)__double_as_longlong(n1), __ATOMIC_RELAXED,
                         __HIP_MEMORY_SCOPE_AGENT);
      __hip_atomic_store(state + 1, (unsigned long long)__double_as_longlong(n2), __ATOMIC_RELAXED,
                         __HIP_MEMORY_SCOPE_AGENT);
      __hip_atomic_store(state + 2, t + 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
      __hip_atomic_store(state + 3, 0ull, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    }
  }
}

hipError_t adam_multi(const ParamDesc* descs, int ndesc, int total_blocks, float* master, const float* grad,
                      float* m_buf, float* v_buf, bf16* wbf, const float* hyper, unsigned long long* state,
                      unsigned long long* tickets, hipStream_t st, const IndexStream* is,
                      const ParamDesc* host_descs) {
  if (ndesc <= 0 || total_blocks <= 0 || m_buf == nullptr || v_buf == nullptr || state == nullptr ||
      tickets == nullptr)
    return hipErrorInvalidValue;
  IndexStream isv{};
  if (is != nullptr) {
    if (is->gate != nullptr || is->mirror != nullptr || is->frag != nullptr) return hipErrorInvalidValue;
    isv = *is;
  }
  const bool stream = isv.src != nullptr || isv.run_stats != nullptr;
  const int grid = total_blocks + (stream ? 1 : 0);
  ParamDescTable tab{};
  if (host_descs != nullptr && ndesc <= kInlineDescs) {
    for (int i = 0; i < ndesc; ++i) tab.d[i] = host_descs[i];
    hipLaunchKernelGGL(adam_multi_kernel<true>, dim3(grid), dim3(256), 0, st, descs, tab, ndesc, master, grad, m_buf,
                       v_buf, wbf, hyper, state, tickets, total_blocks, isv);
  } else {
    hipLaunchKernelGGL(adam_multi_kernel<false>, dim3(grid), dim3(256), 0, st, descs, tab, ndesc, master, grad,
                       m_buf, v_buf, wbf, hyper, state, tickets, total_blocks, isv);
  }
  return hipGetLastError();
}

}  // namespace dfa
