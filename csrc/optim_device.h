// Device helpers of the SGD update shared by the multi-tensor optimizer (csrc/optim.hip) and the
// single-rank LeNet-5 reduce kernel that applies the update itself (csrc/lenet_fused.hip).
#pragma once
#include "common.h"
#include "kernels.h"
#include "lenet_frag.h"

namespace dfa {

// The bf16 compute copies of element i (value w) of a matrix parameter.
__device__ __forceinline__ void emit_copies(const ParamDesc& d, int i, float w, bf16* __restrict__ wbf) {
  if (d.bf_off < 0) return;
  const int K = d.T * d.Ci;
  const int n = i / K;
  const int kk = i - n * K;
  const bf16 wb = f2bf(w);
  if ((d.pad_ >> 28) & 1) {  // tile-mode layouts, element-wise (the LeNet fragment workgroup's path)
    const int t = kk / d.Ci, ci = kk - t * d.Ci;
    wbf[d.bf_off + (long long)n * round_up(K, 32) + kk] = wb;
    wbf[d.bft_off + (long long)ci * round_up(d.T * d.N, 32) + t * d.N + n] = wb;
    return;
  }
  // d.pad_ = KW | Cp << 16 (KW > 0): the primary copy uses the row-segment layout of the fused
  // conv+pool forward, [Npad16][round32(KH * round8(KW*Cp))], column ky*round8(KW*Cp) + kx*Cp + ci
  // d.pad_ = KW | Cp << 16 | pair << 30: pair layout (N <= 8) = 16 rows, rows 8+n hold channel n
  // shifted right by one kernel column (the fused conv+pool forward computes pixels x and x+1)
  const int rKW = d.pad_ & 0xffff;
  // d.pad_ bit 29: the dgrad copy uses the conv+pool dgrad pair layout (csrc/convpool.hip make_dgrad),
  // [16][round32(KH*(KW+1)*N)]: row ci col (a*(KW+1) + KW-1-kx)*N + n and row 8+ci col (a*(KW+1) + KW-kx)*N + n,
  // a = KH-1-ky (the kernel flip of the transposed convolution)
  const int rCp = ((d.pad_ >> 16) & 0xfff) > 0 ? ((d.pad_ >> 16) & 0xfff) : d.Ci;
  const bool rpair = (d.pad_ >> 30) & 1;
  const bool tpair = rKW > 0 && ((d.pad_ >> 29) & 1);
  const int RLp = rKW > 0 ? round_up((rKW + (rpair ? 1 : 0)) * rCp, 8) : K;
  const int Kpad = round_up(rKW > 0 ? (d.T / rKW) * RLp : K, 32);
  const int KpadT = round_up(tpair ? (d.T / rKW) * (rKW + 1) * d.N : d.T * d.N, 32);
  int col = kk;
  if (rKW > 0) {
    const int t = kk / d.Ci, ci = kk - (kk / d.Ci) * d.Ci;
    const int ky = t / rKW, kx = t - (t / rKW) * rKW;
    col = ky * RLp + kx * rCp + ci;
  }
  wbf[d.bf_off + (long long)n * Kpad + col] = wb;
  if (rpair) wbf[d.bf_off + (long long)(n + 8) * Kpad + col + rCp] = wb;
  if (d.bft_off >= 0) {
    const int t = kk / d.Ci;
    const int ci = kk - t * d.Ci;
    if (tpair) {
      const int ky = t / rKW, kx = t - ky * rKW;
      const int c0 = ((d.T / rKW - 1 - ky) * (rKW + 1) + rKW - 1 - kx) * d.N + n;
      wbf[d.bft_off + (long long)ci * KpadT + c0] = wb;
      wbf[d.bft_off + (long long)(ci + 8) * KpadT + c0 + d.N] = wb;
    } else {
      wbf[d.bft_off + (long long)ci * KpadT + t * d.N + n] = wb;
    }
  }
}

// One parameter element: w <- SGD(w, g) with the optimizer's exact (non-contracted) arithmetic,
// momentum written back, bf16 compute copies re-emitted.  hyper = [lr, momentum, wd, grad_scale,
// nesterov].  Returns the new weight.
__device__ __forceinline__ float sgd_apply_one(const ParamDesc& d, int i, float g, float* __restrict__ master,
                                               float* __restrict__ mom_buf, bf16* __restrict__ wbf,
                                               const float* __restrict__ hyper) {
  const float lr = hyper[0], mom = hyper[1], wd = hyper[2], gs = hyper[3];
  const bool nesterov = hyper[4] != 0.f;
  const long long o = d.off + i;
  float v = 0.f;
  const float w = sgd_new_weight(master[o], g, mom != 0.f ? mom_buf[o] : 0.f, lr, mom, wd, gs, nesterov, &v);
  if (mom != 0.f) mom_buf[o] = v;
  master[o] = w;
  emit_copies(d, i, w, wbf);
  return w;
}

// ---- the grid and the copy layouts shared by every multi-tensor optimizer (csrc/optim.hip, csrc/adam.hip)
constexpr int SGD_ELEMS_PER_BLOCK = 1024;

template <typename DT>
__device__ __forceinline__ int find_desc(const DT& d, int n, int bid) {
  int lo = 0, hi = n - 1;
  while (lo < hi) {
    const int mid = (lo + hi + 1) >> 1;
    if (d[mid].block_start <= bid) lo = mid; else hi = mid - 1;
  }
  return lo;
}

// Workgroup ``bid`` of a multi-tensor optimizer launch, d = descs[find_desc(descs, ndesc, bid)] its
// tensor: calls update(i) -> the (new) fp32 value of element i for every element the workgroup owns and
// writes that value's bf16 compute copies.
// The optimizers differ in ``update`` only; which workgroup owns which element and where the copies go
// is decided here, once.
// ``tile_emit(n, k, wb)``: a further consumer of every new bf16 value of a tile-mode matrix (the fused
// LeNet-5 step's dense fragments).
struct NoTileEmit {
  __device__ __forceinline__ void operator()(int, int, bf16) const {}
};
template <typename U, typename E = NoTileEmit>
__device__ __forceinline__ void multi_tensor_body(const ParamDesc& d, bf16* __restrict__ wbf, int bid, const U& update,
                                                  const E& tile_emit = E{}) {
  const int base = (bid - d.block_start) * SGD_ELEMS_PER_BLOCK;
  const int K = d.T * d.Ci;
  // d.pad_ bit 28: tile mode for a plain [N][K] matrix with a plain dgrad copy [Ci][T*N]: the workgroup
  // owns a 32 (n) x 32 (k) tile; the update and the primary copy run along k (coalesced), and the
  // dgrad copy is written through an LDS transpose as 64-byte runs along n (instead of 2-byte
  // scatters one KpadT row apart)
  if ((d.pad_ >> 28) & 1) {
    __shared__ bf16 tt[32][34];
    const int ntk = cdiv(K, 32);
    const int tl = bid - d.block_start;
    const int n0 = (tl / ntk) * 32, k0 = (tl % ntk) * 32;
    const int Kp = round_up(K, 32);
    const int KpT = round_up(d.T * d.N, 32);
    const int cc = threadIdx.x & 31, r0 = threadIdx.x >> 5;
#pragma unroll
    for (int rr = 0; rr < 4; ++rr) {
      const int n = n0 + r0 + 8 * rr, k = k0 + cc;
      if (n < d.N && k < K) {
        const bf16 wb = f2bf(update(n * K + k));
        wbf[d.bf_off + (long long)n * Kp + k] = wb;
        tt[cc][r0 + 8 * rr] = wb;
        tile_emit(n, k, wb);
      }
    }
    __syncthreads();
#pragma unroll
    for (int rr = 0; rr < 4; ++rr) {
      const int k = k0 + r0 + 8 * rr, n = n0 + cc;
      if (n < d.N && k < K) {
        const int t = k / d.Ci, ci = k - t * d.Ci;
        wbf[d.bft_off + (long long)ci * KpT + t * d.N + n] = tt[r0 + 8 * rr][cc];
      }
    }
    return;
  }
#pragma unroll
  for (int r = 0; r < SGD_ELEMS_PER_BLOCK / 256; ++r) {
    const int i = base + r * 256 + threadIdx.x;
    if (i >= d.numel) break;
    emit_copies(d, i, update(i), wbf);
  }
}

// Device-resident index stream: the optimizer is the last kernel of a training step, so one extra
// workgroup of the same launch stages the NEXT step's batch indices (src[(cursor+1) % nsteps]) into
// the static index buffer the step's first kernels read, then advances the cursor.  A replayed step
// graph then needs no host-side copy (and no extra launch) to move to the next batch.
__device__ __forceinline__ void index_stream_body(const IndexStream& is) {
  if (is.src == nullptr) {  // run statistics only (no index stream bound)
    if (threadIdx.x == 0 && is.run_stats != nullptr) {
      is.run_stats[0] += is.step_stats[0];
      is.run_stats[1] += is.step_stats[1];
      is.run_stats[2] += 1.f;
    }
    return;
  }
  __shared__ long long next;
  // thread 0 loads the cursor and, with it, the running / step statistics it updates at the end: one round
  // trip for all of them (the statistics used to be read after the index copy, a third round trip on the
  // launch's critical path)
  float rs[3] = {0.f, 0.f, 0.f}, ss[2] = {0.f, 0.f};
  if (threadIdx.x == 0) {
    const long long c = *is.cursor;
    if (is.run_stats != nullptr) {
      rs[0] = is.run_stats[0], rs[1] = is.run_stats[1], rs[2] = is.run_stats[2];
      ss[0] = is.step_stats[0], ss[1] = is.step_stats[1];
    }
    next = (c + 1) % is.nsteps;
  }
  __syncthreads();
  const long long* src = is.src + next * is.B;
  // all loads of a thread are issued before its stores (one memory round trip for B <= 8192)
  constexpr int R = 16;
  long long v[R];
#pragma unroll
  for (int r = 0; r < R; ++r) {
    const int i = threadIdx.x + 256 * r;
    v[r] = src[min(i, is.B - 1)];
  }
#pragma unroll
  for (int r = 0; r < R; ++r) {
    const int i = threadIdx.x + 256 * r;
    if (i < is.B) is.dst[i] = v[r];
  }
  for (int i = threadIdx.x + 256 * R; i < is.B; i += 256) is.dst[i] = src[i];
  if (threadIdx.x == 0) {
    *is.cursor = next;
    if (is.run_stats != nullptr) {  // this step's stats are final: every step kernel precedes this launch
      is.run_stats[0] = rs[0] + ss[0];
      is.run_stats[1] = rs[1] + ss[1];
      is.run_stats[2] = rs[2] + 1.f;
    }
  }
}

}  // namespace dfa
