// Single-kernel launches: implicit GEMM, pooling, losses, dropout, gather, merge, activations, GAP, metrics;
// BatchNorm (csrc/bn.hip); the optimizers (csrc/optim.hip, csrc/adam.hip) and the fp32 buffer arithmetic.
#include "bindings_util.h"

namespace dfa_py {
namespace {

void igemm_fwd_py(torch::Tensor src, torch::Tensor w, c10::optional<torch::Tensor> bias,
                  c10::optional<torch::Tensor> mask, torch::Tensor out, int64_t M, int64_t N, int64_t K, int64_t Kpad,
                  int64_t lda, int64_t ldc, std::vector<int64_t> geom, int64_t mode, bool relu, double alpha,
                  c10::optional<torch::Tensor> res, c10::optional<torch::Tensor> resmask, double drop_p,
                  int64_t drop_seed, c10::optional<torch::Tensor> drop_step, c10::optional<torch::Tensor> pool_code,
                  int64_t drop_step_add, c10::optional<torch::Tensor> bacc, int64_t bacc_mode,
                  std::vector<torch::Tensor> bacc_in, c10::optional<torch::Tensor> bacc2,
                  std::vector<torch::Tensor> bacc2_in) {
  need(src, at::kBFloat16, "src");
  need(w, at::kBFloat16, "w");
  TORCH_CHECK(out.is_cuda() && out.is_contiguous(), "out must be a contiguous GPU tensor");
  TORCH_CHECK(out.scalar_type() == at::kBFloat16 || out.scalar_type() == at::kFloat, "out must be bf16 or fp32");
  TORCH_CHECK(Kpad % 32 == 0 && Kpad >= K, "Kpad must be a multiple of 32 and >= K");
  TORCH_CHECK(w.numel() >= ((N + 15) / 16 * 16) * Kpad, "weight buffer smaller than [Npad16][Kpad]");
  const bool pooled = has(pool_code);
  if (pooled) {
    TORCH_CHECK(mode == 1 && M % 4 == 0 && ldc == N, "pooled conv: forward conv, M % 4 == 0, ldc == N");
    TORCH_CHECK(pool_code->is_cuda() && pool_code->is_contiguous() && pool_code->scalar_type() == at::kByte &&
                    pool_code->numel() >= M / 4 * N,
                "pool_code must be a uint8 GPU tensor of [M/4][N]");
    TORCH_CHECK(out.numel() >= M / 4 * N, "pooled out too small for [M/4][N]");
  } else {
    TORCH_CHECK(out.numel() >= (M - 1) * ldc + N, "out too small for [M][ldc]");
  }
  TORCH_CHECK(ldc >= N, "ldc < N");
  dfa::IGemmArgs a{};
  set_conv_geom(a, geom, (int)mode);
  if (mode == 0) {
    TORCH_CHECK(src.numel() >= (M - 1) * lda + K, "src too small for [M][lda]");
  } else {
    TORCH_CHECK(a.OH > 0 && a.OW > 0 && M % (a.OH * a.OW) == 0, "M must be B*OH*OW");
    const int64_t Bn = M / (a.OH * a.OW);
    TORCH_CHECK(src.numel() >= Bn * a.SH * a.SW * a.SC, "src too small for the conv geometry");
    TORCH_CHECK(K == (int64_t)a.KH * a.KW * a.SC, "K must be KH*KW*C");
    TORCH_CHECK(a.KH < 128 && a.KW < 128 && a.SC < 65536, "conv geometry out of range");
  }
  a.bias = opt_ptr<const float>(bias, at::kFloat, "bias", N, "bias too small");
  a.mask = opt_ptr<const dfa::bf16>(mask, at::kBFloat16, "mask", (M - 1) * ldc + N, "mask too small");
  a.res = opt_ptr<const dfa::bf16>(res, at::kBFloat16, "residual", (M - 1) * ldc + N, "residual too small");
  a.resmask = opt_ptr<const dfa::bf16>(resmask, at::kBFloat16, "residual", (M - 1) * ldc + N, "residual too small");
  TORCH_CHECK(!has(resmask) || has(res), "resmask without res");
  a.src = reinterpret_cast<const dfa::bf16*>(src.data_ptr());
  a.w = reinterpret_cast<const dfa::bf16*>(w.data_ptr());
  a.out = out.data_ptr();
  a.M = (int)M; a.N = (int)N; a.K = (int)K; a.Kpad = (int)Kpad; a.lda = (int)lda; a.ldc = (int)ldc;
  a.relu = relu ? 1 : 0;
  a.out_f32 = out.scalar_type() == at::kFloat ? 1 : 0;
  a.alpha = (float)alpha;
  a.drop = drop_from(drop_p, drop_seed, drop_step, drop_step_add);
  if (pooled) a.pool_code = pool_code->data_ptr<uint8_t>();
  if (has(bacc)) {
    // BatchNorm sums accumulated by the epilogue (kernels.h BnAcc): acc [nrep][2][N] fp64; mode 1 inputs
    // [x, mean, invstd] of the BatchNorm (and of a second one sharing the gradient)
    need(*bacc, at::kDouble, "bacc");
    TORCH_CHECK(bacc->numel() % (2 * N) == 0, "bacc must be [nrep][2][N]");
    dfa::BnAcc& e = a.bacc;
    e.acc = bacc->data_ptr<double>();
    e.nrep = (int)(bacc->numel() / (2 * N));
    e.mode = (int)bacc_mode;
    TORCH_CHECK(bacc_mode == 0 || bacc_mode == 1, "bacc_mode 0 (forward) or 1 (backward)");
    auto inputs = [&](const std::vector<torch::Tensor>& v, const dfa::bf16** x, const float** mu, const float** is) {
      TORCH_CHECK(v.size() == 3, "bacc mode 1 inputs: [x, mean, invstd]");
      need(v[0], at::kBFloat16, "bacc x");
      TORCH_CHECK(v[0].numel() >= (M - 1) * ldc + N, "bacc x too small");
      need(v[1], at::kFloat, "bacc mean");
      need(v[2], at::kFloat, "bacc invstd");
      TORCH_CHECK(v[1].numel() >= N && v[2].numel() >= N, "bacc mean / invstd smaller than N");
      *x = reinterpret_cast<const dfa::bf16*>(v[0].data_ptr());
      *mu = v[1].data_ptr<float>();
      *is = v[2].data_ptr<float>();
    };
    if (bacc_mode == 1) inputs(bacc_in, &e.x, &e.mean, &e.invstd);
    if (has(bacc2)) {
      TORCH_CHECK(bacc_mode == 1, "a second BatchNorm's sums: backward only");
      need(*bacc2, at::kDouble, "bacc2");
      TORCH_CHECK(bacc2->numel() == bacc->numel(), "bacc2 must match bacc");
      e.acc2 = bacc2->data_ptr<double>();
      inputs(bacc2_in, &e.x2, &e.mean2, &e.invstd2);
    }
  }
  TORCH_CHECK(!a.drop.on || (ldc == N && !a.out_f32), "folded dropout needs a dense bf16 output (ldc == N)");
  // the one plan of this launch: what it may carry, the scratch
  const dfa::ConvPlan plan = dfa::conv_plan(a, (int)mode);
  TORCH_CHECK(!pooled || plan.pool, "pooled conv: unsupported geometry / alignment");
  TORCH_CHECK(!has(bacc) || plan.bacc_ok, "bacc: this launch cannot accumulate BatchNorm sums");
  // split-K partials for the under-filled (small-M, long-K) shapes: PyTorch's caching allocator is
  // stream ordered and graph-capture aware, so the scratch is safe to drop right after the launch
  torch::Tensor splitk;
  if (plan.splitk_floats > 0) {
    splitk = torch::empty({plan.splitk_floats}, out.options().dtype(at::kFloat));
    a.splitk_ws = splitk.data_ptr<float>();
  }
  check_hip(dfa::igemm_fwd(a, plan, (int)mode, cur_stream()), "igemm_fwd");
}

// The plan of a launch with these shapes before any tensor exists: 16-byte aligned dummy operands stand in
// for the real ones (torch allocations are at least that aligned).  bacc_mode >= 0: with BatchNorm sums.
py::dict conv_plan_py(int64_t M, int64_t N, int64_t K, int64_t Kpad, std::vector<int64_t> geom, int64_t mode,
                      int64_t bacc_mode, bool two, bool has_res, bool has_mask, bool pooled, int64_t lda, bool drop,
                      bool has_bias) {
  static dfa::bf16 dummy[8] __attribute__((aligned(16)));
  static double dacc[2] __attribute__((aligned(16)));
  static float dvec[2] __attribute__((aligned(16)));
  dfa::IGemmArgs a{};
  set_conv_geom(a, geom, (int)mode);
  a.M = (int)M; a.N = (int)N; a.K = (int)K; a.Kpad = (int)Kpad; a.ldc = (int)N; a.lda = (int)lda;
  a.src = dummy; a.w = dummy; a.out = dummy;
  if (has_res) a.res = dummy;
  if (has_mask) a.mask = dummy;
  if (has_bias) a.bias = dvec;
  if (pooled) a.pool_code = reinterpret_cast<uint8_t*>(dummy);
  if (drop) a.drop.on = 1;
  if (bacc_mode >= 0) {
    a.bacc.acc = dacc;
    a.bacc.nrep = 1;
    a.bacc.mode = (int)bacc_mode;
    if (bacc_mode == 1) a.bacc.x = dummy, a.bacc.mean = dvec, a.bacc.invstd = dvec;
    if (two) a.bacc.acc2 = dacc, a.bacc.x2 = dummy, a.bacc.mean2 = dvec, a.bacc.invstd2 = dvec;
  }
  const dfa::ConvPlan p = dfa::conv_plan(a, (int)mode);
  static const char* const kFamily[] = {"nop", "invalid", "halo_c64", "halo", "igemm64", "smallc", "generic"};
  using namespace pybind11::literals;
  return py::dict("family"_a = kFamily[p.family], "BM"_a = p.BM, "BN"_a = p.BN, "fast"_a = p.fast, "par"_a = p.par,
                  "pool"_a = p.pool, "splits"_a = p.splits, "wide"_a = p.wide, "row"_a = p.row, "fold"_a = p.fold,
                  "ks"_a = p.ks, "vec"_a = p.vec, "grid"_a = p.grid, "block"_a = p.block, "combine"_a = p.combine,
                  "drop_after"_a = p.drop_after, "splitk_floats"_a = p.splitk_floats,
                  "bacc_ok"_a = p.bacc_ok);
}

// the conv / dense geometry and sizes of a weight gradient (operands and outputs: the caller's)
dfa::WgradArgs wgrad_shape(int64_t M, int64_t N, int64_t K, int64_t ldd, int64_t lda, const std::vector<int64_t>& geom,
                           int64_t mode) {
  dfa::WgradArgs a{};
  set_conv_geom(a, geom, (int)mode);
  a.M = (int)M; a.N = (int)N; a.K = (int)K; a.ldd = (int)ldd; a.lda = (int)lda;
  return a;
}

void igemm_wgrad_py(torch::Tensor dy, torch::Tensor src, torch::Tensor gw, c10::optional<torch::Tensor> gb,
                    torch::Tensor workspace, int64_t M, int64_t N, int64_t K, int64_t ldd, int64_t lda,
                    std::vector<int64_t> geom, int64_t mode, double scale) {
  need(dy, at::kBFloat16, "dy");
  need(src, at::kBFloat16, "src");
  need(gw, at::kFloat, "gw");
  need(workspace, at::kFloat, "workspace");
  TORCH_CHECK(gw.numel() >= N * K, "gw too small");
  TORCH_CHECK(dy.numel() >= (M - 1) * ldd + N, "dy too small");
  dfa::WgradArgs a = wgrad_shape(M, N, K, ldd, lda, geom, mode);
  if (mode == 0) {
    TORCH_CHECK(src.numel() >= (M - 1) * lda + K, "src too small");
  } else {
    TORCH_CHECK(M % (a.OH * a.OW) == 0, "M must be B*OH*OW");
    TORCH_CHECK(src.numel() >= (M / (a.OH * a.OW)) * a.SH * a.SW * a.SC, "src too small");
    TORCH_CHECK(K == (int64_t)a.KH * a.KW * a.SC, "K must be KH*KW*C");
  }
  a.gb = opt_ptr<float>(gb, at::kFloat, "gb", N, "gb too small");
  a.dy = reinterpret_cast<const dfa::bf16*>(dy.data_ptr());
  a.src = reinterpret_cast<const dfa::bf16*>(src.data_ptr());
  a.gw = gw.data_ptr<float>();
  a.with_bias = a.gb ? 1 : 0;
  a.scale = (float)scale;
  // the one plan of this launch: a smaller workspace gives fewer splits, but the C = 1 kernels always
  // write at least one slab
  const dfa::WgradPlan plan = dfa::wgrad_plan(a, (int)mode, (size_t)workspace.numel());
  TORCH_CHECK(workspace.numel() >= plan.scratch_floats, "igemm_wgrad: workspace of ", workspace.numel(),
              " floats, the launch writes ", plan.scratch_floats);
  check_hip(dfa::igemm_wgrad(a, plan, (int)mode, workspace.data_ptr<float>(), cur_stream()), "igemm_wgrad");
}

// The plan of a weight gradient with these shapes and this workspace size, before any tensor exists (16-byte
// aligned dummy operands, as conv_plan_py).
py::dict wgrad_plan_py(int64_t M, int64_t N, int64_t K, int64_t ldd, int64_t lda, std::vector<int64_t> geom,
                       int64_t mode, bool with_bias, int64_t ws_floats) {
  static dfa::bf16 dummy[8] __attribute__((aligned(16)));
  static float dvec[4] __attribute__((aligned(16)));
  dfa::WgradArgs a = wgrad_shape(M, N, K, ldd, lda, geom, mode);
  a.dy = dummy; a.src = dummy; a.gw = dvec;
  if (with_bias) a.gb = dvec, a.with_bias = 1;
  const dfa::WgradPlan p = dfa::wgrad_plan(a, (int)mode, (size_t)std::max<int64_t>(ws_floats, 0));
  static const char* const kFamily[] = {"nop", "halo", "tr", "c1", "smallc", "generic"};
  using namespace pybind11::literals;
  return py::dict("family"_a = kFamily[p.family], "BN"_a = p.BN, "BK"_a = p.BK, "WN"_a = p.WN, "WK"_a = p.WK,
                  "BM"_a = p.BM, "MAXOCC"_a = p.MAXOCC, "dvec"_a = p.dvec, "xvec"_a = p.xvec, "groups"_a = p.groups,
                  "R"_a = p.R, "TI"_a = p.TI, "tps"_a = p.tps, "splits"_a = p.splits, "m_per_split"_a = p.m_per_split,
                  "grid"_a = p.grid, "block"_a = p.block, "reduce"_a = p.reduce, "scratch_floats"_a = p.scratch_floats,
                  "wanted_floats"_a = p.wanted_floats, "capped"_a = p.capped);
}

void maxpool_fwd_py(torch::Tensor x, torch::Tensor y, int64_t B, int64_t H, int64_t W, int64_t C, int64_t P,
                    double drop_p, int64_t drop_seed, c10::optional<torch::Tensor> drop_step, int64_t drop_step_add) {
  need(x, at::kBFloat16, "x");
  need(y, at::kBFloat16, "y");
  TORCH_CHECK(P > 0 && H >= P && W >= P, "bad pool geometry");
  TORCH_CHECK(x.numel() >= B * H * W * C && y.numel() >= B * (H / P) * (W / P) * C, "pool buffers too small");
  check_hip(dfa::maxpool_fwd((const dfa::bf16*)x.data_ptr(), (dfa::bf16*)y.data_ptr(), B, H, W, C, P, cur_stream(),
                             drop_from(drop_p, drop_seed, drop_step, drop_step_add)),
            "maxpool_fwd");
}

void maxpool_bwd_py(torch::Tensor x, torch::Tensor dy, torch::Tensor dx, int64_t B, int64_t H, int64_t W, int64_t C,
                    int64_t P, bool relu_fused) {
  need(x, at::kBFloat16, "x");
  need(dy, at::kBFloat16, "dy");
  need(dx, at::kBFloat16, "dx");
  TORCH_CHECK(P > 0 && H >= P && W >= P, "bad pool geometry");
  TORCH_CHECK(x.numel() >= B * H * W * C && dx.numel() >= B * H * W * C &&
                  dy.numel() >= B * (H / P) * (W / P) * C,
              "pool buffers too small");
  check_hip(dfa::maxpool_bwd((const dfa::bf16*)x.data_ptr(), (const dfa::bf16*)dy.data_ptr(),
                             (dfa::bf16*)dx.data_ptr(), B, H, W, C, P, relu_fused ? 1 : 0, cur_stream()),
            "maxpool_bwd");
}

void softmax_ce_py(torch::Tensor logits, torch::Tensor labels, c10::optional<torch::Tensor> dlogits,
                   c10::optional<torch::Tensor> stats, int64_t B, int64_t C, int64_t ldl, int64_t ldg,
                   double grad_scale) {
  need(logits, at::kFloat, "logits");
  need(labels, at::kInt, "labels");
  TORCH_CHECK(logits.numel() >= (B - 1) * ldl + C && labels.numel() >= B, "softmax_ce inputs too small");
  dfa::bf16* dl = opt_ptr<dfa::bf16>(dlogits, at::kBFloat16, "dlogits", (B - 1) * ldg + C, "dlogits too small");
  float* sp = opt_ptr<float>(stats, at::kFloat, "stats", 2, "stats needs 2 floats");
  check_hip(dfa::softmax_ce(logits.data_ptr<float>(), labels.data_ptr<int>(), dl, sp, B, C, ldl, ldg,
                            (float)grad_scale, cur_stream()),
            "softmax_ce");
}

void dropout_py(torch::Tensor x, torch::Tensor y, double p, int64_t seed, c10::optional<torch::Tensor> mask,
                c10::optional<torch::Tensor> step) {
  const long long* sp = opt_ptr<const long long>(step, at::kLong, "step");
  need(x, at::kBFloat16, "x");
  need(y, at::kBFloat16, "y");
  TORCH_CHECK(y.numel() >= x.numel(), "dropout out too small");
  TORCH_CHECK(p >= 0.0 && p < 1.0, "dropout p must be in [0,1)");
  const auto* mp = opt_ptr<const dfa::bf16>(mask, at::kBFloat16, "mask", x.numel(), "dropout mask too small");
  check_hip(dfa::dropout((const dfa::bf16*)x.data_ptr(), (dfa::bf16*)y.data_ptr(), mp, x.numel(),
                         (float)p, (unsigned long long)seed, sp, cur_stream()),
            "dropout");
}

void gather_batch_py(torch::Tensor data, c10::optional<torch::Tensor> labels, torch::Tensor idx, torch::Tensor out,
                     c10::optional<torch::Tensor> out_labels, int64_t B, int64_t row, double scale,
                     c10::optional<torch::Tensor> step_inc) {
  TORCH_CHECK(data.is_cuda() && data.is_contiguous(), "data must be a contiguous GPU tensor");
  const bool u8 = data.scalar_type() == at::kByte;
  TORCH_CHECK(u8 || data.scalar_type() == at::kBFloat16, "data must be uint8 or bf16");
  need(idx, at::kLong, "idx");
  need(out, at::kBFloat16, "out");
  TORCH_CHECK(idx.numel() >= B && out.numel() >= B * row, "gather buffers too small");
  TORCH_CHECK(data.dim() >= 1 && data.size(0) > 0 && data.numel() / data.size(0) == row, "data row size mismatch");
  const int* lp = nullptr;
  int* olp = nullptr;
  if (has(labels)) {
    need(*labels, at::kInt, "labels");
    TORCH_CHECK(has(out_labels), "out_labels required with labels");
    need(*out_labels, at::kInt, "out_labels");
    lp = labels->data_ptr<int>();
    olp = out_labels->data_ptr<int>();
  }
  check_hip(dfa::gather_batch(data.data_ptr(), u8 ? 1 : 0, lp, reinterpret_cast<const long long*>(idx.data_ptr<int64_t>()), (dfa::bf16*)out.data_ptr(),
                              olp, B, row, (float)scale, (long long)data.size(0), cur_stream(),
                              has(step_inc)
                                  ? reinterpret_cast<long long*>(step_inc->data_ptr<int64_t>())
                                  : nullptr),
            "gather_batch");
}

// Keras merge layer (csrc/merge.hip): inputs [rows][w_i] bf16; fwd writes out, bwd writes grads[i]
static dfa::MergeArgs merge_args(std::vector<torch::Tensor> ins, int64_t kind, int64_t cout) {
  TORCH_CHECK(ins.size() >= 1 && ins.size() <= (size_t)dfa::kMergeMaxIn, "merge: 1..8 inputs");
  dfa::MergeArgs a{};
  a.n = (int)ins.size();
  a.kind = (int)kind;
  a.cout = (int)cout;
  for (int i = 0; i < a.n; ++i) {
    need(ins[i], at::kBFloat16, "merge input");
    const int64_t w = ins[i].size(-1);
    TORCH_CHECK(ins[i].numel() % w == 0, "merge: bad input");
    if (i == 0) a.rows = ins[i].numel() / w;
    TORCH_CHECK(ins[i].numel() / w == a.rows, "merge: inputs differ in rows");
    a.w[i] = (int)w;
    a.in[i] = (const dfa::bf16*)ins[i].data_ptr();
  }
  return a;
}
void merge_fwd_py(std::vector<torch::Tensor> ins, torch::Tensor out, int64_t kind) {
  need(out, at::kBFloat16, "merge out");
  dfa::MergeArgs a = merge_args(ins, kind, out.size(-1));
  TORCH_CHECK(out.numel() == a.rows * (int64_t)a.cout, "merge: out size");
  a.out = (dfa::bf16*)out.data_ptr();
  check_hip(dfa::merge_fwd(a, cur_stream()), "merge_fwd");
}
void merge_bwd_py(std::vector<torch::Tensor> ins, torch::Tensor dy, std::vector<torch::Tensor> grads, int64_t kind) {
  need(dy, at::kBFloat16, "merge dy");
  dfa::MergeArgs a = merge_args(ins, kind, dy.size(-1));
  TORCH_CHECK(grads.size() == ins.size() && dy.numel() == a.rows * (int64_t)a.cout, "merge: grads / dy size");
  a.dy = (const dfa::bf16*)dy.data_ptr();
  for (int i = 0; i < a.n; ++i) {
    need(grads[i], at::kBFloat16, "merge grad");
    TORCH_CHECK(grads[i].numel() == ins[i].numel(), "merge: grad size");
    a.grad[i] = (dfa::bf16*)grads[i].data_ptr();
  }
  check_hip(dfa::merge_bwd(a, cur_stream()), "merge_bwd");
}

void add_act_py(torch::Tensor a, torch::Tensor b, torch::Tensor out, bool relu) {
  need(a, at::kBFloat16, "a");
  need(b, at::kBFloat16, "b");
  need(out, at::kBFloat16, "out");
  TORCH_CHECK(a.numel() == b.numel() && out.numel() >= a.numel(), "add_act size mismatch");
  check_hip(dfa::add_act((const dfa::bf16*)a.data_ptr(), (const dfa::bf16*)b.data_ptr(), (dfa::bf16*)out.data_ptr(),
                         a.numel(), relu ? 1 : 0, cur_stream()),
            "add_act");
}

void relu_bwd_py(torch::Tensor y, torch::Tensor dy, torch::Tensor dx) {
  need(y, at::kBFloat16, "y");
  need(dy, at::kBFloat16, "dy");
  need(dx, at::kBFloat16, "dx");
  TORCH_CHECK(y.numel() == dy.numel() && dx.numel() >= y.numel(), "relu_bwd size mismatch");
  check_hip(dfa::relu_bwd((const dfa::bf16*)y.data_ptr(), (const dfa::bf16*)dy.data_ptr(), (dfa::bf16*)dx.data_ptr(),
                          y.numel(), cur_stream()),
            "relu_bwd");
}

// ---- generic Keras layers (csrc/act.hip)
void act_fwd_py(torch::Tensor x, torch::Tensor y, int64_t kind) {
  need(x, at::kBFloat16, "act x");
  need(y, at::kBFloat16, "act y");
  TORCH_CHECK(y.numel() >= x.numel(), "act: output too small");
  TORCH_CHECK(kind >= dfa::kActLinear && kind <= dfa::kActExp, "act: unknown kind");
  check_hip(dfa::act_fwd((const dfa::bf16*)x.data_ptr(), (dfa::bf16*)y.data_ptr(), x.numel(), (int)kind,
                         cur_stream()),
            "act_fwd");
}

void act_bwd_py(torch::Tensor x, torch::Tensor dy, torch::Tensor dx, int64_t kind, bool in_relu) {
  need(x, at::kBFloat16, "act x");
  need(dy, at::kBFloat16, "act dy");
  need(dx, at::kBFloat16, "act dx");
  TORCH_CHECK(dy.numel() == x.numel() && dx.numel() >= x.numel(), "act_bwd: size mismatch");
  TORCH_CHECK(kind >= dfa::kActLinear && kind <= dfa::kActExp, "act: unknown kind");
  check_hip(dfa::act_bwd((const dfa::bf16*)x.data_ptr(), (const dfa::bf16*)dy.data_ptr(), (dfa::bf16*)dx.data_ptr(),
                         x.numel(), (int)kind, in_relu ? 1 : 0, cur_stream()),
            "act_bwd");
}

void sigmoid_ce_py(torch::Tensor logits, torch::Tensor labels, c10::optional<torch::Tensor> dlogits,
                   c10::optional<torch::Tensor> stats, int64_t B, int64_t C, int64_t ldl, int64_t ldg,
                   double grad_scale) {
  need(logits, at::kFloat, "logits");
  need(labels, at::kInt, "labels");
  TORCH_CHECK(B > 0 && C > 0 && ldl >= C && ldg >= C, "sigmoid_ce: bad shape");
  TORCH_CHECK(logits.numel() >= (B - 1) * ldl + C && labels.numel() >= B, "sigmoid_ce inputs too small");
  dfa::bf16* dl = opt_ptr<dfa::bf16>(dlogits, at::kBFloat16, "dlogits", (B - 1) * ldg + C, "dlogits too small");
  float* sp = opt_ptr<float>(stats, at::kFloat, "stats", 2, "stats needs 2 floats");
  check_hip(dfa::sigmoid_ce(logits.data_ptr<float>(), labels.data_ptr<int>(), dl, sp, B, C, ldl, ldg,
                            (float)grad_scale, cur_stream()),
            "sigmoid_ce");
}

// a [rows][C] matrix of leading dimension ld: a contiguous tensor, or a column slice [:, :C] of a wider
// contiguous buffer (row stride ld); its rows must lie inside the tensor's storage
static void need_rows(const torch::Tensor& t, at::ScalarType dt, const char* name, int64_t rows, int64_t C, int64_t ld) {
  TORCH_CHECK(t.is_cuda(), name, " must be a GPU tensor");
  TORCH_CHECK(t.scalar_type() == dt, name, " has dtype ", t.scalar_type(), ", expected ", dt);
  int64_t avail = t.numel();
  if (!t.is_contiguous()) {
    TORCH_CHECK(t.dim() == 2 && t.size(1) == C && t.stride(1) == 1 && t.stride(0) == ld, name,
                " must be contiguous or a column slice [:, :C] with row stride ld");
    avail = (int64_t)(t.storage().nbytes() / t.element_size()) - t.storage_offset();
  }
  TORCH_CHECK(rows >= 1 && avail >= (rows - 1) * ld + C, name, " too small");
}

void loss_grad_py(torch::Tensor logits, c10::optional<torch::Tensor> labels, c10::optional<torch::Tensor> targets,
                  c10::optional<torch::Tensor> idx, c10::optional<torch::Tensor> dlogits,
                  c10::optional<torch::Tensor> stats, int64_t B, int64_t C, int64_t ldl, int64_t ldt, int64_t ldg,
                  int64_t kind, int64_t out_act, double grad_scale) {
  const int64_t lim = 1ll << 31;
  TORCH_CHECK(B > 0 && B < lim, "loss_grad: B must be in [1, 2^31)");
  TORCH_CHECK(C > 0 && C < lim, "loss_grad: C must be in [1, 2^31)");
  TORCH_CHECK(ldl >= C && ldl < lim, "loss_grad: ldl must be in [C, 2^31)");
  TORCH_CHECK(ldt >= C && ldt < lim, "loss_grad: ldt must be in [C, 2^31)");
  TORCH_CHECK(ldg >= C && ldg < lim, "loss_grad: ldg must be in [C, 2^31)");
  TORCH_CHECK(kind >= 0 && kind <= dfa::kMetricCategoricalCE, "loss_grad: unknown loss kind ", kind);
  TORCH_CHECK(out_act >= 0 && out_act <= 2, "loss_grad: out_act is 0 (linear), 1 (softmax) or 2 (sigmoid)");
  TORCH_CHECK(has(labels) != has(targets), "loss_grad: exactly one of labels and targets");
  need_rows(logits, at::kFloat, "logits", B, C, ldl);
  const long long* ip = opt_ptr<const long long>(idx, at::kLong, "idx", B, "idx needs B entries");
  int64_t nrows;  // rows of the label / target table: all of them through idx, the first B without
  if (has(labels)) {
    need(*labels, at::kInt, "labels");
    nrows = labels->numel();
  } else {
    nrows = targets->dim() == 2 ? targets->size(0) : targets->numel() / ldt;
    need_rows(*targets, at::kFloat, "targets", nrows, C, ldt);
  }
  TORCH_CHECK(nrows >= (ip ? 1 : B), "loss_grad: labels / targets need B rows");
  dfa::bf16* dl = nullptr;
  if (has(dlogits)) {
    need_rows(*dlogits, at::kBFloat16, "dlogits", B, C, ldg);
    dl = reinterpret_cast<dfa::bf16*>(dlogits->data_ptr());
  }
  float* sp = opt_ptr<float>(stats, at::kFloat, "stats", 2, "stats needs 2 floats");
  check_hip(dfa::loss_grad(logits.data_ptr<float>(), cptr<int>(labels), cptr<float>(targets), ip, nrows, dl, sp, B, C,
                           ldl, ldt, ldg, kind, out_act, (float)grad_scale, cur_stream()),
            "loss_grad");
}

// The launch plan of the image loss as a dict (no GPU needed): what the launcher will do for these sizes.
py::dict image_loss_plan_py(int64_t B, int64_t E, bool aligned) {
  using namespace pybind11::literals;
  const dfa::ImageLossPlan p = dfa::image_loss_plan(B, E, aligned);
  return py::dict("ok"_a = p.ok, "vec"_a = p.vec, "threads"_a = p.threads, "elems_per_wg"_a = p.elems_per_wg,
                  "wgs_per_image"_a = p.wgs_per_image, "grid"_a = p.grid, "ws_floats"_a = p.ws_floats);
}

void image_loss_grad_py(torch::Tensor z, torch::Tensor targets, c10::optional<torch::Tensor> idx,
                        c10::optional<torch::Tensor> dz, c10::optional<torch::Tensor> stats,
                        c10::optional<torch::Tensor> ws, int64_t B, int64_t E, int64_t kind, int64_t out_act,
                        double grad_scale, double target_scale, bool out_relu) {
  TORCH_CHECK(B > 0 && E > 0 && E <= (1ll << 40), "image_loss_grad: B and E must be positive (E <= 2^40)");
  TORCH_CHECK(kind >= 0 && kind <= dfa::kMetricSigmoidCE,
              "image_loss_grad: the loss kind must be one of the mean kinds 0..5, got ", kind);
  TORCH_CHECK(out_act == 0 || out_act == 2, "image_loss_grad: out_act is 0 (linear) or 2 (sigmoid)");
  need(z, at::kBFloat16, "image_loss_grad z");
  TORCH_CHECK(z.numel() == B * E, "image_loss_grad: z must hold [B][E]");
  TORCH_CHECK(targets.is_cuda() && targets.is_contiguous(), "image_loss_grad: targets must be a contiguous GPU tensor");
  const bool u8 = targets.scalar_type() == at::kByte;
  TORCH_CHECK(u8 || targets.scalar_type() == at::kFloat, "image_loss_grad: targets must be fp32 or uint8");
  TORCH_CHECK(targets.numel() % E == 0, "image_loss_grad: the target table must be [N][E]");
  const int64_t nrows = targets.numel() / E;
  const long long* ip = opt_ptr<const long long>(idx, at::kLong, "idx", B, "image_loss_grad: idx needs B entries");
  TORCH_CHECK(nrows >= (ip ? 1 : B), "image_loss_grad: the target table needs B rows");
  dfa::bf16* dp = nullptr;
  if (has(dz)) {
    need(*dz, at::kBFloat16, "image_loss_grad dz");
    TORCH_CHECK(dz->numel() == B * E, "image_loss_grad: dz must hold [B][E]");
    dp = reinterpret_cast<dfa::bf16*>(dz->data_ptr());
  }
  float* sp = opt_ptr<float>(stats, at::kFloat, "stats", 2, "image_loss_grad: stats needs 2 floats");
  const dfa::ImageLossPlan p = dfa::image_loss_plan(B, E, false);  // grid and workspace do not depend on alignment
  TORCH_CHECK(p.ok, "image_loss_grad: B * ceil(E / ", dfa::kImageLossElems, ") workgroups exceed 2^31 - 1");
  float* wp = nullptr;
  size_t wn = 0;
  if (sp) {
    TORCH_CHECK(has(ws), "image_loss_grad: stats needs a workspace of ", p.ws_floats, " floats");
    wp = opt_ptr<float>(ws, at::kFloat, "workspace", p.ws_floats, "image_loss_grad: the workspace is too small");
    wn = (size_t)ws->numel();
  }
  check_hip(dfa::image_loss_grad(reinterpret_cast<const dfa::bf16*>(z.data_ptr()),
                                 u8 ? nullptr : targets.data_ptr<float>(), u8 ? targets.data_ptr<uint8_t>() : nullptr,
                                 (float)target_scale, ip, nrows, dp, sp, wp, wn, B, E, (int)kind, (int)out_act,
                                 out_relu ? 1 : 0, (float)grad_scale, cur_stream()),
            "image_loss_grad");
}

static dfa::Pool2DGeom pool_geom(const std::vector<int64_t>& g) {
  TORCH_CHECK(g.size() == 12, "pool2d: geom = [B, H, W, C, OH, OW, ph, pw, sh, sw, pt, pl]");
  dfa::Pool2DGeom p{};
  p.B = (int)g[0]; p.H = (int)g[1]; p.W = (int)g[2]; p.C = (int)g[3]; p.OH = (int)g[4]; p.OW = (int)g[5];
  p.ph = (int)g[6]; p.pw = (int)g[7]; p.sh = (int)g[8]; p.sw = (int)g[9]; p.pt = (int)g[10]; p.pl = (int)g[11];
  TORCH_CHECK(p.B > 0 && p.H > 0 && p.W > 0 && p.C > 0 && p.OH > 0 && p.OW > 0 && p.ph > 0 && p.pw > 0 && p.sh > 0 &&
                  p.sw > 0 && p.pt >= 0 && p.pl >= 0 && p.pt < p.ph && p.pl < p.pw,
              "pool2d: bad geometry");
  // every window starts inside the padded image
  TORCH_CHECK((p.OH - 1) * p.sh - p.pt < p.H && (p.OW - 1) * p.sw - p.pl < p.W, "pool2d: output too large");
  return p;
}

void pool2d_fwd_py(torch::Tensor x, torch::Tensor y, std::vector<int64_t> geom, bool avg) {
  const dfa::Pool2DGeom g = pool_geom(geom);
  need(x, at::kBFloat16, "pool x");
  need(y, at::kBFloat16, "pool y");
  TORCH_CHECK(x.numel() == (int64_t)g.B * g.H * g.W * g.C && y.numel() == (int64_t)g.B * g.OH * g.OW * g.C,
              "pool2d: tensor sizes do not match the geometry");
  check_hip(dfa::pool2d_fwd((const dfa::bf16*)x.data_ptr(), (dfa::bf16*)y.data_ptr(), g, avg ? 1 : 0, cur_stream()),
            "pool2d_fwd");
}

void pool2d_bwd_py(torch::Tensor x, torch::Tensor dy, torch::Tensor dx, std::vector<int64_t> geom, bool avg,
                   bool in_relu) {
  const dfa::Pool2DGeom g = pool_geom(geom);
  need(x, at::kBFloat16, "pool x");
  need(dy, at::kBFloat16, "pool dy");
  need(dx, at::kBFloat16, "pool dx");
  TORCH_CHECK(x.numel() == (int64_t)g.B * g.H * g.W * g.C && dx.numel() == x.numel() &&
                  dy.numel() == (int64_t)g.B * g.OH * g.OW * g.C,
              "pool2d: tensor sizes do not match the geometry");
  check_hip(dfa::pool2d_bwd((const dfa::bf16*)x.data_ptr(), (const dfa::bf16*)dy.data_ptr(), (dfa::bf16*)dx.data_ptr(),
                            g, avg ? 1 : 0, in_relu ? 1 : 0, cur_stream()),
            "pool2d_bwd");
}

// ---- depthwise convolution (csrc/dwconv.hip)
static dfa::DwConvGeom dw_geom(const std::vector<int64_t>& g) {
  TORCH_CHECK(g.size() == 13, "dwconv: geom = [B, H, W, C, M, OH, OW, KH, KW, sh, sw, pt, pl]");
  for (int64_t v : g) TORCH_CHECK(v >= 0 && v < (1LL << 30), "dwconv: bad geometry");
  dfa::DwConvGeom p{};
  p.B = (int)g[0]; p.H = (int)g[1]; p.W = (int)g[2]; p.C = (int)g[3]; p.M = (int)g[4]; p.OH = (int)g[5];
  p.OW = (int)g[6]; p.KH = (int)g[7]; p.KW = (int)g[8]; p.sh = (int)g[9]; p.sw = (int)g[10]; p.pt = (int)g[11];
  p.pl = (int)g[12];
  TORCH_CHECK(p.B > 0 && p.H > 0 && p.W > 0 && p.C > 0 && p.M > 0 && p.OH > 0 && p.OW > 0 && p.KH > 0 && p.KW > 0 &&
                  p.sh > 0 && p.sw > 0 && p.pt < p.KH && p.pl < p.KW,
              "dwconv: bad geometry");
  // every window starts inside the padded image
  TORCH_CHECK((int64_t)(p.OH - 1) * p.sh - p.pt < p.H && (int64_t)(p.OW - 1) * p.sw - p.pl < p.W,
              "dwconv: output too large");
  return p;
}

static void dw_sizes(const dfa::DwConvGeom& g, const torch::Tensor& x, const torch::Tensor& y, const torch::Tensor& w) {
  const int64_t CO = (int64_t)g.C * g.M;
  TORCH_CHECK(x.numel() == (int64_t)g.B * g.H * g.W * g.C && y.numel() == (int64_t)g.B * g.OH * g.OW * CO &&
                  w.numel() == (int64_t)g.KH * g.KW * CO,
              "dwconv: tensor sizes do not match the geometry");
}

void dwconv_fwd_py(torch::Tensor x, torch::Tensor w, c10::optional<torch::Tensor> bias, torch::Tensor y,
                   std::vector<int64_t> geom, bool relu) {
  const dfa::DwConvGeom g = dw_geom(geom);
  need(x, at::kBFloat16, "dwconv x");
  need(w, at::kFloat, "dwconv kernel");
  need(y, at::kBFloat16, "dwconv y");
  dw_sizes(g, x, y, w);
  const float* bp = opt_ptr<const float>(bias, at::kFloat, "dwconv bias", (int64_t)g.C * g.M, "dwconv bias too small");
  check_hip(dfa::dwconv_fwd((const dfa::bf16*)x.data_ptr(), w.data_ptr<float>(), bp, (dfa::bf16*)y.data_ptr(), g,
                            relu ? 1 : 0, cur_stream()),
            "dwconv_fwd");
}

void dwconv_dgrad_py(torch::Tensor dy, torch::Tensor w, c10::optional<torch::Tensor> mask, torch::Tensor dx,
                     std::vector<int64_t> geom) {
  const dfa::DwConvGeom g = dw_geom(geom);
  need(dy, at::kBFloat16, "dwconv dy");
  need(w, at::kFloat, "dwconv kernel");
  need(dx, at::kBFloat16, "dwconv dx");
  dw_sizes(g, dx, dy, w);
  const dfa::bf16* mp = opt_ptr<const dfa::bf16>(mask, at::kBFloat16, "dwconv mask", dx.numel(), "dwconv mask too small");
  check_hip(dfa::dwconv_dgrad((const dfa::bf16*)dy.data_ptr(), w.data_ptr<float>(), mp, (dfa::bf16*)dx.data_ptr(), g,
                              cur_stream()),
            "dwconv_dgrad");
}

void dwconv_wgrad_py(torch::Tensor dy, torch::Tensor x, torch::Tensor gw, c10::optional<torch::Tensor> gb,
                     torch::Tensor ws, std::vector<int64_t> geom) {
  const dfa::DwConvGeom g = dw_geom(geom);
  need(dy, at::kBFloat16, "dwconv dy");
  need(x, at::kBFloat16, "dwconv x");
  need(gw, at::kFloat, "dwconv kernel gradient");
  need(ws, at::kFloat, "dwconv workspace");
  dw_sizes(g, x, dy, gw);
  float* gbp = opt_ptr<float>(gb, at::kFloat, "dwconv bias gradient", (int64_t)g.C * g.M, "dwconv bias gradient too small");
  TORCH_CHECK(ws.numel() >= dfa::dwconv_wgrad_slab_floats(g), "dwconv_wgrad: the workspace does not hold one slab");
  check_hip(dfa::dwconv_wgrad((const dfa::bf16*)dy.data_ptr(), (const dfa::bf16*)x.data_ptr(), gw.data_ptr<float>(), gbp,
                              ws.data_ptr<float>(), (size_t)ws.numel(), g, cur_stream()),
            "dwconv_wgrad");
}

// ---- up-sampling and the transposed conv's bias gradient (csrc/upsample.hip)
static dfa::UpGeom up_geom(const std::vector<int64_t>& g, bool bilinear, bool half_pixel) {
  TORCH_CHECK(g.size() == 6, "upsample2d: geom = [B, H, W, C, sh, sw]");
  for (int64_t v : g) TORCH_CHECK(v > 0 && v < (1LL << 30), "upsample2d: bad geometry");
  TORCH_CHECK(g[1] * g[4] < (1LL << 30) && g[2] * g[5] < (1LL << 30), "upsample2d: output too large");
  dfa::UpGeom p{};
  p.B = (int)g[0]; p.H = (int)g[1]; p.W = (int)g[2]; p.C = (int)g[3]; p.sh = (int)g[4]; p.sw = (int)g[5];
  p.bilinear = bilinear ? 1 : 0;
  p.off = half_pixel ? 0.5f : 0.f;
  return p;
}

void upsample2d_fwd_py(torch::Tensor x, torch::Tensor y, std::vector<int64_t> geom, bool bilinear, bool half_pixel) {
  const dfa::UpGeom g = up_geom(geom, bilinear, half_pixel);
  need(x, at::kBFloat16, "upsample2d x");
  need(y, at::kBFloat16, "upsample2d y");
  const int64_t n = (int64_t)g.B * g.H * g.W * g.C;
  TORCH_CHECK(x.numel() == n && y.numel() == n * g.sh * g.sw, "upsample2d: tensor sizes do not match the geometry");
  check_hip(dfa::upsample2d_fwd((const dfa::bf16*)x.data_ptr(), (dfa::bf16*)y.data_ptr(), g, cur_stream()),
            "upsample2d_fwd");
}

void upsample2d_bwd_py(torch::Tensor dy, c10::optional<torch::Tensor> mask, torch::Tensor dx, std::vector<int64_t> geom,
                       bool bilinear, bool half_pixel) {
  const dfa::UpGeom g = up_geom(geom, bilinear, half_pixel);
  need(dy, at::kBFloat16, "upsample2d dy");
  need(dx, at::kBFloat16, "upsample2d dx");
  const int64_t n = (int64_t)g.B * g.H * g.W * g.C;
  TORCH_CHECK(dx.numel() == n && dy.numel() == n * g.sh * g.sw, "upsample2d: tensor sizes do not match the geometry");
  const dfa::bf16* mp = opt_ptr<const dfa::bf16>(mask, at::kBFloat16, "upsample2d mask", n, "upsample2d mask too small");
  check_hip(dfa::upsample2d_bwd((const dfa::bf16*)dy.data_ptr(), mp, (dfa::bf16*)dx.data_ptr(), g, cur_stream()),
            "upsample2d_bwd");
}

void channel_sum_py(torch::Tensor dy, torch::Tensor gb, torch::Tensor ws, int64_t M, int64_t C, double scale) {
  need(dy, at::kBFloat16, "channel_sum dy");
  need(gb, at::kFloat, "channel_sum gb");
  need(ws, at::kFloat, "channel_sum workspace");
  TORCH_CHECK(M > 0 && C > 0 && C <= (1 << 20) && M < (1LL << 40), "channel_sum: bad sizes");
  TORCH_CHECK(dy.numel() == M * C && gb.numel() >= C, "channel_sum: tensor sizes do not match [M][C]");
  TORCH_CHECK(ws.numel() >= C, "channel_sum: the workspace does not hold one slab");
  check_hip(dfa::channel_sum((const dfa::bf16*)dy.data_ptr(), gb.data_ptr<float>(), ws.data_ptr<float>(),
                             (size_t)ws.numel(), M, (int)C, (float)scale, cur_stream()),
            "channel_sum");
}

void gap_fwd_py(torch::Tensor x, torch::Tensor y, int64_t B, int64_t HW, int64_t C) {
  need(x, at::kBFloat16, "x");
  need(y, at::kBFloat16, "y");
  TORCH_CHECK(x.numel() >= B * HW * C && y.numel() >= B * C, "gap buffers too small");
  check_hip(dfa::gap_fwd((const dfa::bf16*)x.data_ptr(), (dfa::bf16*)y.data_ptr(), B, HW, C, cur_stream()), "gap_fwd");
}

void gap_bwd_py(torch::Tensor dy, torch::Tensor dx, int64_t B, int64_t HW, int64_t C) {
  need(dy, at::kBFloat16, "dy");
  need(dx, at::kBFloat16, "dx");
  TORCH_CHECK(dx.numel() >= B * HW * C && dy.numel() >= B * C, "gap buffers too small");
  check_hip(dfa::gap_bwd((const dfa::bf16*)dy.data_ptr(), (dfa::bf16*)dx.data_ptr(), B, HW, C, cur_stream()),
            "gap_bwd");
}

void gather_labels_py(torch::Tensor labels, torch::Tensor idx, torch::Tensor out) {
  need(labels, at::kInt, "labels");
  need(idx, at::kLong, "idx");
  need(out, at::kInt, "out");
  TORCH_CHECK(out.numel() >= idx.numel() && labels.numel() > 0, "gather_labels sizes");
  check_hip(dfa::gather_labels(labels.data_ptr<int>(), reinterpret_cast<const long long*>(idx.data_ptr<int64_t>()),
                               out.data_ptr<int>(), (int)idx.numel(), labels.numel(), cur_stream()),
            "gather_labels");
}

void classifier_metrics_py(torch::Tensor z, torch::Tensor labels, int64_t kind, int64_t out_act, torch::Tensor out) {
  need(z, at::kFloat, "metrics logits");
  need(labels, at::kInt, "metrics labels");
  need(out, at::kFloat, "metrics out");
  TORCH_CHECK(z.dim() == 2 && labels.numel() == z.size(0) && out.numel() >= 2, "metrics: z [B][C], labels [B]");
  check_hip(dfa::classifier_metrics(z.data_ptr<float>(), labels.data_ptr<int>(), (int)z.size(0), (int)z.size(1),
                                    (int)kind, (int)out_act, out.data_ptr<float>(), cur_stream()),
            "classifier_metrics");
}

// ---- BatchNorm (csrc/bn.hip)
void bn_check_vec(const torch::Tensor& t, int64_t n, const char* name) {
  need(t, at::kFloat, name);
  TORCH_CHECK(t.numel() >= n, name, " too small");
}

void bn_check_act(const torch::Tensor& t, int64_t n, const char* name) {
  need(t, at::kBFloat16, name);
  TORCH_CHECK(t.numel() >= n, name, " too small");
}

void bn_check_stats_ws(const torch::Tensor& ws, const torch::Tensor& counter, int64_t M, int64_t C) {
  TORCH_CHECK(C > 0 && C <= 1024 && M > 0, "bn: need 0 < C <= 1024 and M > 0");
  TORCH_CHECK(C % 8 == 0 || C <= 256, "bn: C must be a multiple of 8 or <= 256");
  bn_check_vec(ws, dfa::bn_stats_ws_floats((int)M, (int)C), "bn workspace");
  need(counter, at::kInt, "bn counter");
  TORCH_CHECK(counter.numel() >= dfa::bn_stats_counters((int)M, (int)C), "bn counter: need ",
              dfa::bn_stats_counters((int)M, (int)C), " int32 tickets");
}

// the running statistics go together; returns whether they are given
bool bn_check_run(const c10::optional<torch::Tensor>& run_mean, const c10::optional<torch::Tensor>& run_var, int64_t C,
                  const char* alone = "run_var required with run_mean") {
  if (!has(run_mean)) return false;
  bn_check_vec(*run_mean, C, "run_mean");
  TORCH_CHECK(has(run_var), alone);
  bn_check_vec(*run_var, C, "run_var");
  return true;
}

// launch arguments of the forward statistics (tensors already checked)
dfa::BnStatsArgs bn_fwd_args(torch::Tensor& x, torch::Tensor& mean, torch::Tensor& invstd,
                             c10::optional<torch::Tensor>& run_mean, c10::optional<torch::Tensor>& run_var, bool run,
                             torch::Tensor& ws, torch::Tensor& counter, int64_t M, int64_t C, double momentum,
                             double eps) {
  dfa::BnStatsArgs a{};
  a.x = (const dfa::bf16*)x.data_ptr();
  a.mean_out = mean.data_ptr<float>();
  a.invstd_out = invstd.data_ptr<float>();
  a.run_mean = run ? run_mean->data_ptr<float>() : nullptr;
  a.run_var = run ? run_var->data_ptr<float>() : nullptr;
  a.ws = ws.data_ptr<float>();
  a.counter = reinterpret_cast<unsigned*>(counter.data_ptr<int>());
  a.M = (int)M; a.C = (int)C; a.momentum = (float)momentum; a.eps = (float)eps;
  return a;
}

// checks and launch arguments of the backward statistics
dfa::BnStatsArgs bn_bwd_args(torch::Tensor& x, c10::optional<torch::Tensor>& mask, torch::Tensor& dy,
                             torch::Tensor& gamma, torch::Tensor& mean, torch::Tensor& invstd, torch::Tensor& dgamma,
                             torch::Tensor& dbeta, torch::Tensor& coef, torch::Tensor& ws, torch::Tensor& counter,
                             int64_t M, int64_t C, double gscale) {
  bn_check_act(x, M * C, "x");
  bn_check_act(dy, M * C, "dy");
  if (has(mask)) bn_check_act(*mask, M * C, "mask");
  bn_check_vec(gamma, C, "gamma");
  bn_check_vec(mean, C, "mean");
  bn_check_vec(invstd, C, "invstd");
  bn_check_vec(dgamma, C, "dgamma");
  bn_check_vec(dbeta, C, "dbeta");
  bn_check_vec(coef, 3 * C, "coef");
  bn_check_stats_ws(ws, counter, M, C);
  dfa::BnStatsArgs a{};
  a.x = (const dfa::bf16*)x.data_ptr();
  a.mask = cptr<dfa::bf16>(mask);
  a.dy = (const dfa::bf16*)dy.data_ptr();
  a.gamma = gamma.data_ptr<float>();
  a.mean = mean.data_ptr<float>();
  a.invstd = invstd.data_ptr<float>();
  a.dgamma = dgamma.data_ptr<float>();
  a.dbeta = dbeta.data_ptr<float>();
  a.coef = coef.data_ptr<float>();
  a.ws = ws.data_ptr<float>();
  a.counter = reinterpret_cast<unsigned*>(counter.data_ptr<int>());
  a.M = (int)M; a.C = (int)C; a.gscale = (float)gscale;
  return a;
}

// the residual join of an apply: r, or bn_r(r) when the residual BatchNorm's vectors are given
void bn_set_residual(dfa::BnApplyArgs& a, c10::optional<torch::Tensor>& r, c10::optional<torch::Tensor>& rgamma,
                     c10::optional<torch::Tensor>& rbeta, c10::optional<torch::Tensor>& rmean,
                     c10::optional<torch::Tensor>& rinvstd, int64_t M, int64_t C) {
  if (!has(r)) return;
  bn_check_act(*r, M * C, "residual");
  a.r = (const dfa::bf16*)r->data_ptr();
  if (!has(rgamma)) return;
  for (auto* t : {&rgamma, &rbeta, &rmean, &rinvstd}) {
    TORCH_CHECK(has(*t), "residual BN needs gamma, beta, mean, invstd");
    bn_check_vec(**t, C, "residual bn vector");
  }
  a.rgamma = rgamma->data_ptr<float>();
  a.rbeta = rbeta->data_ptr<float>();
  a.rmean = rmean->data_ptr<float>();
  a.rinvstd = rinvstd->data_ptr<float>();
}

// forward statistics: batch mean / invstd (+ running statistics) in one launch
void bn_stats_fwd_py(torch::Tensor x, torch::Tensor mean, torch::Tensor invstd, c10::optional<torch::Tensor> run_mean,
                     c10::optional<torch::Tensor> run_var, torch::Tensor ws, torch::Tensor counter, int64_t M,
                     int64_t C, double momentum, double eps) {
  bn_check_act(x, M * C, "x");
  bn_check_vec(mean, C, "mean");
  bn_check_vec(invstd, C, "invstd");
  const bool run = bn_check_run(run_mean, run_var, C);
  bn_check_stats_ws(ws, counter, M, C);
  dfa::BnStatsArgs a = bn_fwd_args(x, mean, invstd, run_mean, run_var, run, ws, counter, M, C, momentum, eps);
  check_hip(dfa::bn_stats(a, 0, cur_stream()), "bn_stats_fwd");
}

// backward statistics: dgamma/dbeta + dx coefficients coef[3][C]; g = dy * (mask > 0) when mask is given
void bn_stats_bwd_py(torch::Tensor x, c10::optional<torch::Tensor> mask, torch::Tensor dy, torch::Tensor gamma,
                     torch::Tensor mean, torch::Tensor invstd, torch::Tensor dgamma, torch::Tensor dbeta,
                     torch::Tensor coef, torch::Tensor ws, torch::Tensor counter, int64_t M, int64_t C, double gscale) {
  dfa::BnStatsArgs a = bn_bwd_args(x, mask, dy, gamma, mean, invstd, dgamma, dbeta, coef, ws, counter, M, C, gscale);
  check_hip(dfa::bn_stats(a, 1, cur_stream()), "bn_stats_bwd");
}

// y = act(bn(x) [+ r | + bn_r(r)]); eval: mean/invstd are the running mean / variance
void bn_apply_py(torch::Tensor x, torch::Tensor y, torch::Tensor gamma, torch::Tensor beta, torch::Tensor mean,
                 torch::Tensor invstd, c10::optional<torch::Tensor> r, c10::optional<torch::Tensor> rgamma,
                 c10::optional<torch::Tensor> rbeta, c10::optional<torch::Tensor> rmean,
                 c10::optional<torch::Tensor> rinvstd, int64_t M, int64_t C, bool relu, bool eval, double eps) {
  bn_check_act(x, M * C, "x");
  bn_check_act(y, M * C, "y");
  for (auto* t : {&gamma, &beta, &mean, &invstd}) bn_check_vec(*t, C, "bn vector");
  dfa::BnApplyArgs a{};
  a.x = (const dfa::bf16*)x.data_ptr();
  a.y = (dfa::bf16*)y.data_ptr();
  a.gamma = gamma.data_ptr<float>();
  a.beta = beta.data_ptr<float>();
  a.mean = mean.data_ptr<float>();
  a.invstd = invstd.data_ptr<float>();
  bn_set_residual(a, r, rgamma, rbeta, rmean, rinvstd, M, C);
  a.M = (int)M; a.C = (int)C; a.relu = relu ? 1 : 0; a.eval = eval ? 1 : 0; a.eps = (float)eps;
  check_hip(dfa::bn_apply(a, cur_stream()), "bn_apply");
}

void bn_dx_py(torch::Tensor x, c10::optional<torch::Tensor> mask, torch::Tensor dy, torch::Tensor dx,
              torch::Tensor coef, int64_t M, int64_t C) {
  bn_check_act(x, M * C, "x");
  bn_check_act(dy, M * C, "dy");
  bn_check_act(dx, M * C, "dx");
  if (has(mask)) bn_check_act(*mask, M * C, "mask");
  bn_check_vec(coef, 3 * C, "coef");
  check_hip(dfa::bn_dx((const dfa::bf16*)x.data_ptr(), cptr<dfa::bf16>(mask), (const dfa::bf16*)dy.data_ptr(),
                       (dfa::bf16*)dx.data_ptr(), coef.data_ptr<float>(), (int)M, (int)C, cur_stream()),
            "bn_dx");
}

// BatchNorm consumers that finalise epilogue-accumulated sums (csrc/bn.hip, kernels.h BnAccFin)
static dfa::BnAccFin bn_fin(const torch::Tensor& acc, const c10::optional<torch::Tensor>& zero, int64_t C) {
  need(acc, at::kDouble, "bn acc");
  TORCH_CHECK(acc.numel() % (2 * C) == 0 && acc.numel() / (2 * C) <= dfa::kBnAccMaxRep, "bn acc must be [nrep][2][C]");
  dfa::BnAccFin f{};
  f.acc = acc.data_ptr<double>();
  f.nrep = (int)(acc.numel() / (2 * C));
  if (has(zero)) {
    need(*zero, at::kDouble, "bn acc zero");
    TORCH_CHECK(zero->numel() == acc.numel(), "bn acc zero must match acc");
    f.zero = zero->data_ptr<double>();
  }
  return f;
}

// y = act(bn(x) [+ r | + bn_r(r)]) in training mode, statistics from the producer's sums; workgroup 0
// writes mean / invstd / running statistics (of the residual BN too) and clears `zero` / `rzero`
void bn_apply_acc_py(torch::Tensor x, torch::Tensor y, torch::Tensor gamma, torch::Tensor beta, torch::Tensor acc,
                     c10::optional<torch::Tensor> zero, torch::Tensor mean, torch::Tensor invstd,
                     c10::optional<torch::Tensor> run_mean, c10::optional<torch::Tensor> run_var,
                     c10::optional<torch::Tensor> r, std::vector<torch::Tensor> rbn, int64_t M, int64_t C, bool relu,
                     double momentum, double eps) {
  TORCH_CHECK(C % 8 == 0 && C <= 1024, "bn_apply_acc: C % 8 == 0, C <= 1024");
  bn_check_act(x, M * C, "x");
  bn_check_act(y, M * C, "y");
  for (auto* t : {&gamma, &beta, &mean, &invstd}) bn_check_vec(*t, C, "bn vector");
  dfa::BnApplyArgs a{};
  a.x = (const dfa::bf16*)x.data_ptr();
  a.y = (dfa::bf16*)y.data_ptr();
  a.gamma = gamma.data_ptr<float>();
  a.beta = beta.data_ptr<float>();
  a.M = (int)M; a.C = (int)C; a.relu = relu ? 1 : 0; a.eval = 0; a.eps = (float)eps;
  dfa::BnAccFin f = bn_fin(acc, zero, C);
  f.mean = mean.data_ptr<float>();
  f.invstd = invstd.data_ptr<float>();
  if (bn_check_run(run_mean, run_var, C, "run_var with run_mean")) {
    f.run_mean = run_mean->data_ptr<float>();
    f.run_var = run_var->data_ptr<float>();
  }
  f.momentum = (float)momentum;
  f.eps = (float)eps;
  dfa::BnAccFin fr{};
  const bool has_rbn = !rbn.empty();
  if (has(r)) {
    bn_check_act(*r, M * C, "residual");
    a.r = (const dfa::bf16*)r->data_ptr();
    if (has_rbn) {
      // [gamma, beta, acc, zero (or empty), mean, invstd, run_mean, run_var]
      TORCH_CHECK(rbn.size() == 8, "residual BN: [gamma, beta, acc, zero, mean, invstd, run_mean, run_var]");
      for (int i : {0, 1, 4, 5, 6, 7}) bn_check_vec(rbn[i], C, "residual bn vector");
      a.rgamma = rbn[0].data_ptr<float>();
      a.rbeta = rbn[1].data_ptr<float>();
      fr = bn_fin(rbn[2], rbn[3].numel() ? c10::optional<torch::Tensor>(rbn[3]) : c10::nullopt, C);
      fr.mean = rbn[4].data_ptr<float>();
      fr.invstd = rbn[5].data_ptr<float>();
      fr.run_mean = rbn[6].data_ptr<float>();
      fr.run_var = rbn[7].data_ptr<float>();
      fr.momentum = (float)momentum;
      fr.eps = (float)eps;
      a.rmean = fr.mean;  // non-null marks RES 2
      a.rinvstd = fr.invstd;
    }
  } else {
    TORCH_CHECK(!has_rbn, "residual BN without a residual");
  }
  check_hip(dfa::bn_apply_acc(a, f, has_rbn ? &fr : nullptr, cur_stream()), "bn_apply_acc");
}

// dx = k1 g + k2 x + k3 from the producer's backward sums; workgroup 0 writes dgamma / dbeta (x gscale) and
// coef, and clears `zero`
void bn_dx_acc_py(torch::Tensor x, torch::Tensor g, torch::Tensor dx, torch::Tensor acc,
                  c10::optional<torch::Tensor> zero, torch::Tensor gamma, torch::Tensor mean, torch::Tensor invstd,
                  torch::Tensor dgamma, torch::Tensor dbeta, torch::Tensor coef, int64_t M, int64_t C, double gscale) {
  TORCH_CHECK(C % 8 == 0 && C <= 1024, "bn_dx_acc: C % 8 == 0, C <= 1024");
  bn_check_act(x, M * C, "x");
  bn_check_act(g, M * C, "g");
  bn_check_act(dx, M * C, "dx");
  for (auto* t : {&gamma, &mean, &invstd, &dgamma, &dbeta}) bn_check_vec(*t, C, "bn vector");
  bn_check_vec(coef, 3 * C, "coef");
  dfa::BnAccFin f = bn_fin(acc, zero, C);
  f.mean = mean.data_ptr<float>();
  f.invstd = invstd.data_ptr<float>();
  f.gamma = gamma.data_ptr<float>();
  f.dgamma = dgamma.data_ptr<float>();
  f.dbeta = dbeta.data_ptr<float>();
  f.coef = coef.data_ptr<float>();
  f.gscale = (float)gscale;
  check_hip(dfa::bn_dx_acc((const dfa::bf16*)x.data_ptr(), (const dfa::bf16*)g.data_ptr(), (dfa::bf16*)dx.data_ptr(),
                           f, (int)M, (int)C, cur_stream()),
            "bn_dx_acc");
}

// GAP backward with relu' (mask) and the BatchNorm backward sums of the result (ResNet's last block)
void gap_bwd_bn_py(torch::Tensor dy, torch::Tensor mask, torch::Tensor dx, int64_t B, int64_t HW, int64_t C,
                   torch::Tensor acc, std::vector<torch::Tensor> bn_in) {
  need(dy, at::kBFloat16, "dy");
  need(mask, at::kBFloat16, "mask");
  need(dx, at::kBFloat16, "dx");
  TORCH_CHECK(dy.numel() >= B * C && mask.numel() >= B * HW * C && dx.numel() >= B * HW * C, "gap_bwd_bn sizes");
  TORCH_CHECK(C % 4 == 0 && C <= 1024 && 256 % (C / 4) == 0, "gap_bwd_bn: C / 4 must divide 256");
  need(acc, at::kDouble, "bn acc");
  TORCH_CHECK(acc.numel() % (2 * C) == 0, "bn acc must be [nrep][2][C]");
  TORCH_CHECK(bn_in.size() == 3, "gap_bwd_bn: [x, mean, invstd]");
  need(bn_in[0], at::kBFloat16, "bn x");
  TORCH_CHECK(bn_in[0].numel() >= B * HW * C, "bn x too small");
  bn_check_vec(bn_in[1], C, "bn mean");
  bn_check_vec(bn_in[2], C, "bn invstd");
  dfa::BnAcc e{};
  e.acc = acc.data_ptr<double>();
  e.nrep = (int)(acc.numel() / (2 * C));
  e.mode = 1;
  e.x = (const dfa::bf16*)bn_in[0].data_ptr();
  e.mean = bn_in[1].data_ptr<float>();
  e.invstd = bn_in[2].data_ptr<float>();
  check_hip(dfa::gap_bwd_bn((const dfa::bf16*)dy.data_ptr(), (const dfa::bf16*)mask.data_ptr(),
                            (dfa::bf16*)dx.data_ptr(), (int)B, (int)HW, (int)C, e, cur_stream()),
            "gap_bwd_bn");
}

// ---- optimizers
// the optimizer launch's extra workgroup (csrc/optim_device.h index_stream_body): next-batch index staging
// and / or the device run statistics
static void fill_index_stream(dfa::IndexStream& is, const c10::optional<torch::Tensor>& idx_stream,
                              const c10::optional<torch::Tensor>& idx_cursor,
                              const c10::optional<torch::Tensor>& idx_dst,
                              const c10::optional<torch::Tensor>& step_stats,
                              const c10::optional<torch::Tensor>& run_stats) {
  if (has(idx_stream)) {
    TORCH_CHECK(idx_cursor.has_value() && idx_dst.has_value(), "index stream needs cursor and dst");
    need(*idx_stream, at::kLong, "idx_stream");
    need(*idx_cursor, at::kLong, "idx_cursor");
    need(*idx_dst, at::kLong, "idx_dst");
    TORCH_CHECK(idx_stream->dim() == 2 && idx_stream->size(1) == idx_dst->numel() && idx_cursor->numel() >= 1,
                "idx_stream must be [nsteps][B] with B = idx_dst.numel()");
    is.src = reinterpret_cast<const long long*>(idx_stream->data_ptr());
    is.cursor = reinterpret_cast<long long*>(idx_cursor->data_ptr());
    is.dst = reinterpret_cast<long long*>(idx_dst->data_ptr());
    is.B = (int)idx_dst->numel();
    is.nsteps = (int)idx_stream->size(0);
  }
  // device run statistics, with or without an index stream (the same extra workgroup accumulates them)
  if (has(run_stats)) {
    TORCH_CHECK(has(step_stats), "run_stats needs step_stats");
    need(*run_stats, at::kFloat, "run_stats");
    need(*step_stats, at::kFloat, "step_stats");
    TORCH_CHECK(run_stats->numel() >= 3 && step_stats->numel() >= 2, "run_stats [3] / step_stats [2]");
    is.run_stats = run_stats->data_ptr<float>();
    is.step_stats = step_stats->data_ptr<float>();
  }
}

// the descriptor table's host copy (or null), passed in the kernel arguments
const dfa::ParamDesc* host_descs(const c10::optional<torch::Tensor>& descs_host, const torch::Tensor& descs) {
  if (!has(descs_host)) return nullptr;
  TORCH_CHECK(!descs_host->is_cuda() && descs_host->scalar_type() == at::kLong && descs_host->is_contiguous() &&
                  descs_host->numel() == descs.numel(),
              "descs_host must be the int64 CPU copy of descs");
  return reinterpret_cast<const dfa::ParamDesc*>(descs_host->data_ptr());
}

// descs: int64 GPU tensor [ndesc][6] laid out as ParamDesc (see optim.hip)
void sgd_multi_py(torch::Tensor descs, int64_t ndesc, int64_t total_blocks, torch::Tensor master, torch::Tensor grad,
                  c10::optional<torch::Tensor> mom, torch::Tensor wbf, torch::Tensor hyper, bool apply_update,
                  c10::optional<torch::Tensor> idx_stream, c10::optional<torch::Tensor> idx_cursor,
                  c10::optional<torch::Tensor> idx_dst, c10::optional<torch::Tensor> descs_host,
                  c10::optional<torch::Tensor> lenet_frag, int64_t frag_w1, int64_t frag_w2,
                  std::vector<int64_t> frag_dense, c10::optional<torch::Tensor> lenet_snap, c10::optional<torch::Tensor> step_stats,
                  c10::optional<torch::Tensor> run_stats, uintptr_t gate, uintptr_t mirror) {
  TORCH_CHECK(descs.is_cuda() && descs.scalar_type() == at::kLong && descs.is_contiguous(), "descs must be int64 GPU");
  const dfa::ParamDesc* hd = host_descs(descs_host, descs);
  static_assert(sizeof(dfa::ParamDesc) == 48, "ParamDesc layout");
  TORCH_CHECK(descs.numel() * 8 >= ndesc * (int64_t)sizeof(dfa::ParamDesc), "descs too small");
  need(master, at::kFloat, "master");
  need(grad, at::kFloat, "grad");
  need(wbf, at::kBFloat16, "wbf");
  need(hyper, at::kFloat, "hyper");
  TORCH_CHECK(hyper.numel() >= 5, "hyper needs [lr, momentum, wd, grad_scale, nesterov]");
  TORCH_CHECK(grad.numel() >= master.numel(), "grad smaller than master");
  float* mp = opt_ptr<float>(mom, at::kFloat, "mom", master.numel(), "momentum buffer too small");
  dfa::IndexStream is{};
  fill_index_stream(is, idx_stream, idx_cursor, idx_dst, step_stats, run_stats);
  if (has(lenet_frag)) {
    TORCH_CHECK(lenet_frag->is_cuda() && lenet_frag->is_contiguous() &&
                    (size_t)lenet_frag->nbytes() >= dfa::lenet_frag_bytes(),
                "lenet_frag: fragment buffer too small");
    TORCH_CHECK(frag_w1 >= 0 && frag_w1 + 150 <= master.numel() && frag_w2 >= 0 && frag_w2 + 2400 <= master.numel(),
                "lenet_frag: conv kernel offsets out of range");
    TORCH_CHECK(!apply_update || has(lenet_snap), "lenet_frag: an update needs the pre-update snapshot (lenet_snap)");
    is.snap = opt_ptr<float>(lenet_snap, at::kFloat, "lenet_snap", 2 * 2550, "lenet_snap must hold 2 x 2550 floats");
    is.frag = lenet_frag->data_ptr();
    is.frag_w1 = frag_w1;
    is.frag_w2 = frag_w2;
    // the three dense kernels: their tile workgroups scatter every new value into the dense fragment
    // ranges, whose shapes are LeNet-5's (csrc/lenet_frag.h), so the descriptors must be exactly those
    TORCH_CHECK(frag_dense.size() == 3 && hd != nullptr,
                "lenet_frag: the three dense kernel offsets and the host descriptor table are required");
    const int64_t NK[3][2] = {{120, 400}, {84, 120}, {10, 84}};
    for (int l = 0; l < 3; ++l) {
      bool found = false;
      for (int64_t k = 0; k < ndesc; ++k)
        if (hd[k].off == frag_dense[l])
          found = ((hd[k].pad_ >> 28) & 1) && hd[k].N == NK[l][0] && hd[k].T == 1 && hd[k].Ci == NK[l][1];
      TORCH_CHECK(found, "lenet_frag: dense kernel ", l, " is not a tile-mode [", NK[l][0], "][", NK[l][1], "] matrix");
      is.frag_d[l] = frag_dense[l];
    }
  }
  // async PS exclusive writer (PSComm.excl_gate / excl_mirror): the update gated on the admission word, the
  // new weights mirrored into the rank's shard
  TORCH_CHECK((gate == 0) == (mirror == 0), "sgd_multi: gate and mirror go together");
  TORCH_CHECK(gate == 0 || (apply_update && !is.frag), "sgd_multi: a gated update without LeNet fragments");
  is.gate = reinterpret_cast<const unsigned*>(gate);
  is.mirror = reinterpret_cast<float*>(mirror);
  const bool any = is.src || is.frag || is.run_stats || is.gate;
  check_hip(dfa::sgd_multi(reinterpret_cast<const dfa::ParamDesc*>(descs.data_ptr()), (int)ndesc, (int)total_blocks,
                           master.data_ptr<float>(), grad.data_ptr<float>(), mp, (dfa::bf16*)wbf.data_ptr(),
                           hyper.data_ptr<float>(), apply_update ? 1 : 0, cur_stream(), any ? &is : nullptr, hd),
            "sgd_multi");
}

// Adam / AdamW twin of sgd_multi (csrc/adam.hip).  The LeNet-5 fragment rebuild is SGD-only (no argument
// for it here) and so are the async parameter server's gate / mirror, which are rejected.
void adam_multi_py(torch::Tensor descs, int64_t ndesc, int64_t total_blocks, torch::Tensor master, torch::Tensor grad,
                   torch::Tensor m, torch::Tensor v, torch::Tensor wbf, torch::Tensor hyper, torch::Tensor state,
                   torch::Tensor tickets, c10::optional<torch::Tensor> idx_stream, c10::optional<torch::Tensor> idx_cursor,
                   c10::optional<torch::Tensor> idx_dst, c10::optional<torch::Tensor> descs_host,
                   c10::optional<torch::Tensor> step_stats, c10::optional<torch::Tensor> run_stats,
                   uintptr_t gate, uintptr_t mirror) {
  TORCH_CHECK(gate == 0 && mirror == 0,
              "adam_multi: the async parameter server's exclusive-writer gate / mirror take SGD only");
  TORCH_CHECK(descs.is_cuda() && descs.scalar_type() == at::kLong && descs.is_contiguous(), "descs must be int64 GPU");
  const dfa::ParamDesc* hd = host_descs(descs_host, descs);
  TORCH_CHECK(ndesc > 0 && total_blocks > 0, "adam_multi: nothing to update");
  TORCH_CHECK(descs.numel() * 8 >= ndesc * (int64_t)sizeof(dfa::ParamDesc), "descs too small");
  need(master, at::kFloat, "master");
  need(grad, at::kFloat, "grad");
  need(m, at::kFloat, "m");
  need(v, at::kFloat, "v");
  need(wbf, at::kBFloat16, "wbf");
  need(hyper, at::kFloat, "hyper");
  need(state, at::kLong, "state");
  TORCH_CHECK(hyper.numel() >= dfa::kAdamHyper,
              "hyper needs [lr, beta1, beta2, eps, wd, grad_scale, decoupled, 1-beta1, 1-beta2]");
  TORCH_CHECK(state.numel() >= dfa::kAdamState, "state needs [c1, c2, t, ticket]");
  need(tickets, at::kLong, "tickets");
  TORCH_CHECK(tickets.numel() >= dfa::kAdamTicketGroups * dfa::kAdamTicketStride, "ticket buffer too small");
  TORCH_CHECK(grad.numel() >= master.numel() && m.numel() >= master.numel() && v.numel() >= master.numel(),
              "grad / m / v smaller than master");
  dfa::IndexStream is{};
  fill_index_stream(is, idx_stream, idx_cursor, idx_dst, step_stats, run_stats);
  const bool any = is.src || is.run_stats;
  check_hip(dfa::adam_multi(reinterpret_cast<const dfa::ParamDesc*>(descs.data_ptr()), (int)ndesc, (int)total_blocks,
                            master.data_ptr<float>(), grad.data_ptr<float>(), m.data_ptr<float>(),
                            v.data_ptr<float>(), (dfa::bf16*)wbf.data_ptr(), hyper.data_ptr<float>(),
                            reinterpret_cast<unsigned long long*>(state.data_ptr()),
                            reinterpret_cast<unsigned long long*>(tickets.data_ptr()), cur_stream(),
                            any ? &is : nullptr, hd),
            "adam_multi");
}

void sum_buffers_py(torch::Tensor ptrs, int64_t nin, torch::Tensor out, double scale) {
  TORCH_CHECK(ptrs.is_cuda() && ptrs.scalar_type() == at::kLong && ptrs.numel() >= nin, "ptrs must be int64 GPU");
  need(out, at::kFloat, "out");
  check_hip(dfa::sum_buffers(reinterpret_cast<const float* const*>(ptrs.data_ptr()), (int)nin, out.data_ptr<float>(),
                             out.numel(), (float)scale, cur_stream()),
            "sum_buffers");
}

void axpby_py(torch::Tensor out, torch::Tensor a, torch::Tensor b, double alpha, double beta) {
  need(out, at::kFloat, "out");
  need(a, at::kFloat, "a");
  need(b, at::kFloat, "b");
  TORCH_CHECK(a.numel() == out.numel() && b.numel() == out.numel(), "axpby size mismatch");
  check_hip(dfa::axpby(out.data_ptr<float>(), a.data_ptr<float>(), b.data_ptr<float>(), (float)alpha, (float)beta,
                       out.numel(), cur_stream()),
            "axpby");
}

}  // namespace

void bind_layers(py::module_& m) {
  m.def("igemm_fwd", &igemm_fwd_py, "implicit-GEMM MFMA (dense/conv fwd, dgrad)", py::arg("src"), py::arg("w"),
        py::arg("bias"), py::arg("mask"), py::arg("out"), py::arg("M"), py::arg("N"), py::arg("K"), py::arg("Kpad"),
        py::arg("lda"), py::arg("ldc"), py::arg("geom"), py::arg("mode"), py::arg("relu"), py::arg("alpha"),
        py::arg("res") = py::none(), py::arg("resmask") = py::none(), py::arg("drop_p") = 0.0,
        py::arg("drop_seed") = 0, py::arg("drop_step") = py::none(), py::arg("pool_code") = py::none(),
        py::arg("drop_step_add") = 0, py::arg("bacc") = py::none(), py::arg("bacc_mode") = 0,
        py::arg("bacc_in") = std::vector<torch::Tensor>{},
        py::arg("bacc2") = py::none(), py::arg("bacc2_in") = std::vector<torch::Tensor>{});
  m.def("conv_plan", &conv_plan_py, "the launch plan of igemm_fwd for these shapes (csrc/conv_plan.hip), as a dict",
        py::arg("M"), py::arg("N"), py::arg("K"), py::arg("Kpad"), py::arg("geom"), py::arg("mode"),
        py::arg("bacc_mode") = -1, py::arg("two") = false, py::arg("has_res") = false, py::arg("has_mask") = false,
        py::arg("pooled") = false, py::arg("lda") = 0, py::arg("drop") = false, py::arg("has_bias") = false);
  m.def("unpool2", [](torch::Tensor dyp, torch::Tensor code, torch::Tensor dy) {
    need(dyp, at::kBFloat16, "unpool dyp");
    need(dy, at::kBFloat16, "unpool dy");
    TORCH_CHECK(dy.dim() == 4 && code.is_cuda() && code.is_contiguous() && code.scalar_type() == at::kByte,
                "unpool2: dy [B][OH][OW][N], code uint8");
    const int64_t B = dy.size(0), OH = dy.size(1), OW = dy.size(2), N = dy.size(3);
    TORCH_CHECK(dyp.numel() == B * (OH / 2) * (OW / 2) * N && code.numel() == dyp.numel(), "unpool2: sizes");
    check_hip(dfa::unpool2(reinterpret_cast<const dfa::bf16*>(dyp.data_ptr()), code.data_ptr<uint8_t>(),
                           reinterpret_cast<dfa::bf16*>(dy.data_ptr()), (int)B, (int)OH, (int)OW, (int)N,
                           cur_stream()),
              "unpool2");
  });
  m.def("igemm_wgrad", &igemm_wgrad_py, "implicit-GEMM MFMA weight gradient (split-m slabs + reduce)");
  m.def("wgrad_plan", &wgrad_plan_py, "the launch plan of igemm_wgrad for these shapes and this workspace size, as a dict",
        py::arg("M"), py::arg("N"), py::arg("K"), py::arg("ldd"), py::arg("lda"), py::arg("geom"), py::arg("mode"),
        py::arg("with_bias"), py::arg("ws_floats"));
  m.def("maxpool_fwd", &maxpool_fwd_py, py::arg("x"), py::arg("y"), py::arg("B"), py::arg("H"), py::arg("W"),
        py::arg("C"), py::arg("P"), py::arg("drop_p") = 0.0, py::arg("drop_seed") = 0,
        py::arg("drop_step") = py::none(), py::arg("drop_step_add") = 0);
  m.def("maxpool_bwd", &maxpool_bwd_py);
  m.def("softmax_ce", &softmax_ce_py);
  m.def("dropout", &dropout_py);
  m.def("gather_batch", &gather_batch_py, py::arg("data"), py::arg("labels"), py::arg("idx"), py::arg("out"),
        py::arg("out_labels"), py::arg("B"), py::arg("row"), py::arg("scale"), py::arg("step_inc") = py::none());
  m.def("add_act", &add_act_py);
  m.def("merge_fwd", &merge_fwd_py, "Keras merge layer forward (Add / Subtract / Multiply / Average / Maximum / "
        "Minimum / Concatenate)");
  m.def("merge_bwd", &merge_bwd_py, "Keras merge layer: gradient of every input");
  m.def("relu_bwd", &relu_bwd_py);
  m.def("gap_fwd", &gap_fwd_py);
  m.def("gap_bwd", &gap_bwd_py);
  m.def("classifier_metrics", &classifier_metrics_py,
        "[loss sum, correct] of a classifier batch (one launch); out_act 0 logits, 1 softmax, 2 sigmoid output");
  m.def("act_fwd", &act_fwd_py, "standalone activation y = act(x) (csrc/act.hip)");
  m.def("act_bwd", &act_bwd_py, "dx = dy * act'(x) [* relu'(x)]");
  m.def("sigmoid_ce", &sigmoid_ce_py, "sigmoid cross-entropy on logits vs one-hot labels (+ dlogits)");
  m.def("loss_grad", &loss_grad_py,
        "any lossesMap loss on act(logits) vs int labels or dense targets, optionally through idx (+ dlogits, stats)");
  m.def("image_loss_grad", &image_loss_grad_py,
        "a mean lossesMap loss on act(z) of a bf16 output map vs an fp32 / uint8 target table, optionally through "
        "idx (+ dz, stats; fixed-order sums)",
        py::arg("z"), py::arg("targets"), py::arg("idx"), py::arg("dz"), py::arg("stats"), py::arg("workspace"),
        py::arg("B"), py::arg("E"), py::arg("kind"), py::arg("out_act"), py::arg("grad_scale"),
        py::arg("target_scale") = 1.0, py::arg("out_relu") = false);
  m.def("image_loss_plan", &image_loss_plan_py, "the launch plan of image_loss_grad", py::arg("B"), py::arg("E"),
        py::arg("aligned") = true);
  m.def("pool2d_fwd", &pool2d_fwd_py, "general 2-D max / average pooling, any window / stride / padding");
  m.def("pool2d_bwd", &pool2d_bwd_py, "backward of pool2d_fwd (input-centric, no atomics)");
  m.def("dwconv_fwd", &dwconv_fwd_py, "depthwise conv forward, fp32 kernel [KH][KW][C*M] (csrc/dwconv.hip)");
  m.def("dwconv_dgrad", &dwconv_dgrad_py, "depthwise conv data gradient [* relu'(mask)]");
  m.def("dwconv_wgrad", &dwconv_wgrad_py, "depthwise conv weight / bias gradient (fixed-order slab sums)");
  m.def("upsample2d_fwd", &upsample2d_fwd_py, "UpSampling2D forward, nearest / bilinear (csrc/upsample.hip)");
  m.def("upsample2d_bwd", &upsample2d_bwd_py, "UpSampling2D backward, gather form [* relu'(mask)]");
  m.def("channel_sum", &channel_sum_py, "gb[c] = scale * sum_m dy[m][c] (fixed-order slab sums)");
  m.def("gather_labels", &gather_labels_py);
  m.def("bn_stats_fwd", &bn_stats_fwd_py, "BN forward statistics (partials + last-workgroup finalize, one launch)");
  m.def("bn_stats_bwd", &bn_stats_bwd_py, "BN backward statistics: dgamma, dbeta and dx coefficients");
  m.def("bn_apply", &bn_apply_py, "BN normalize (+ residual join, + ReLU)");
  m.def("bn_dx", &bn_dx_py, "BN input gradient dx = k1*g + k2*x + k3");
  m.def("bn_apply_acc", &bn_apply_acc_py, "BN training apply, statistics finalised from epilogue-accumulated sums");
  m.def("bn_dx_acc", &bn_dx_acc_py, "BN input gradient, coefficients finalised from epilogue-accumulated sums");
  m.def("gap_bwd_bn", &gap_bwd_bn_py, "GAP backward with relu' and BatchNorm backward sums");
  m.def("bn_stats_grid", &dfa::bn_stats_grid, "partial-slab count of a BN statistics launch");
  m.def("sgd_multi", &sgd_multi_py, py::arg("descs"), py::arg("ndesc"), py::arg("total_blocks"), py::arg("master"),
        py::arg("grad"), py::arg("mom"), py::arg("wbf"), py::arg("hyper"), py::arg("apply_update"),
        py::arg("idx_stream") = py::none(), py::arg("idx_cursor") = py::none(), py::arg("idx_dst") = py::none(),
        py::arg("descs_host") = py::none(), py::arg("lenet_frag") = py::none(), py::arg("frag_w1") = 0,
        py::arg("frag_w2") = 0, py::arg("frag_dense") = std::vector<int64_t>{}, py::arg("lenet_snap") = py::none(), py::arg("step_stats") = py::none(),
        py::arg("run_stats") = py::none(), py::arg("gate") = 0, py::arg("mirror") = 0);
  m.def("adam_multi", &adam_multi_py, py::arg("descs"), py::arg("ndesc"), py::arg("total_blocks"), py::arg("master"),
        py::arg("grad"), py::arg("m"), py::arg("v"), py::arg("wbf"), py::arg("hyper"), py::arg("state"),
        py::arg("tickets"), py::arg("idx_stream") = py::none(), py::arg("idx_cursor") = py::none(), py::arg("idx_dst") = py::none(),
        py::arg("descs_host") = py::none(), py::arg("step_stats") = py::none(), py::arg("run_stats") = py::none(),
        py::arg("gate") = 0, py::arg("mirror") = 0,
        "Fused multi-tensor Adam / AdamW: master, m, v, bf16 compute copies and the step state in one launch");
  m.attr("ADAM_TICKET_WORDS") = dfa::kAdamTicketGroups * dfa::kAdamTicketStride;
  m.def("sum_buffers", &sum_buffers_py);
  m.def("graph_upload", [](uintptr_t exec) {
    // stage an instantiated graph's kernel arguments / launch packets on the device now, outside any
    // timed region, instead of on its first hipGraphLaunch
    check_hip(hipGraphUpload(reinterpret_cast<hipGraphExec_t>(exec), cur_stream()), "hipGraphUpload");
  }, "hipGraphUpload of a captured graph (torch.cuda.CUDAGraph.raw_cuda_graph_exec()) on the current stream");
  m.def("axpby", &axpby_py);
}

}  // namespace dfa_py
