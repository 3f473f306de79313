// Fused blocks: conv+pool, the dense heads, the reference CNN's conv block, whole-network LeNet-5; and the
// Python classes of the communicators, which lenet_train takes (so this file parses bindings_comm.h anyway).
#include "bindings_comm.h"

namespace dfa_py {
namespace {

// geometry: [B, H, W, C, KH, KW, pad, N]
struct CPIn {
  const void* x = nullptr;
  int u8 = 0;
  const long long* idx = nullptr;
  long long nrows = 0;
};

CPIn cp_input(const torch::Tensor& x, const c10::optional<torch::Tensor>& idx, int64_t B, int64_t HWC) {
  CPIn r;
  TORCH_CHECK(x.is_cuda() && x.is_contiguous(), "x must be a contiguous GPU tensor");
  if (has(idx)) {
    need(*idx, at::kLong, "idx");
    TORCH_CHECK(idx->numel() >= B, "idx shorter than the batch");
    TORCH_CHECK(x.scalar_type() == at::kByte || x.scalar_type() == at::kBFloat16, "dataset must be u8 or bf16");
    TORCH_CHECK(x.dim() >= 1 && x.size(0) > 0 && x.numel() / x.size(0) == HWC, "dataset row size mismatch");
    TORCH_CHECK(x.scalar_type() == at::kByte, "indexed input must be a uint8 dataset");
    r.u8 = 1;
    r.idx = reinterpret_cast<const long long*>(idx->data_ptr<int64_t>());
    r.nrows = x.size(0);
  } else {
    TORCH_CHECK(x.scalar_type() == at::kBFloat16, "x must be bf16");
    TORCH_CHECK(x.numel() >= B * HWC, "x too small");
  }
  r.x = x.data_ptr();
  return r;
}

// the prologue of the three launches: the plan of the geometry (fetched once), the batch, the pooled elements
struct CPCall {
  const dfa::CPPlan& p;
  int64_t B, pn;
};

CPCall cp_call(const std::vector<int64_t>& geom) {
  TORCH_CHECK(geom.size() == 8, "geom = [B,H,W,C,KH,KW,pad,N]");
  const dfa::CPPlan& p = dfa::convpool_plan(geom[1], geom[2], geom[3], geom[4], geom[5], geom[6], geom[7]);
  TORCH_CHECK(p.ok, "convpool: unsupported geometry");
  return {p, geom[0], geom[0] * p.g.PH * p.g.PW * p.g.N};
}

void convpool_fwd_py(torch::Tensor x, c10::optional<torch::Tensor> idx, double scale, torch::Tensor w,
                     c10::optional<torch::Tensor> bias, torch::Tensor p, c10::optional<torch::Tensor> code,
                     std::vector<int64_t> geom) {
  const CPCall c = cp_call(geom);
  const dfa::CPGeom& g = c.p.g;
  CPIn in = cp_input(x, idx, c.B, (int64_t)g.H * g.W * g.C);
  need(w, at::kBFloat16, "w");
  // row-segment layout [Npad16][Kpad2] (ParamSpec.row_pad / row_cp)
  TORCH_CHECK(w.numel() >= (int64_t)((g.N + 15) / 16 * 16) * g.wKpad2 && w.size(-1) == g.wKpad2,
              "w must be the row-segment layout [Npad16][", g.wKpad2, "] (channel stride ", g.Cp, ")");
  need(p, at::kBFloat16, "p");
  TORCH_CHECK(p.numel() >= c.pn, "p too small");
  uint8_t* cp = opt_ptr<uint8_t>(code, at::kByte, "code", c.pn, "code too small");
  const float* bp = opt_ptr<const float>(bias, at::kFloat, "bias", g.N, "bias too small");
  check_hip(dfa::convpool_fwd(c.p, c.B, in.x, in.u8, in.idx, in.nrows, (float)scale, (const dfa::bf16*)w.data_ptr(), bp,
                              (dfa::bf16*)p.data_ptr(), cp, cur_stream()),
            "convpool_fwd");
}

int64_t convpool_wgrad_py(torch::Tensor x, c10::optional<torch::Tensor> idx, double scale, torch::Tensor dp,
                          torch::Tensor code, torch::Tensor gw, c10::optional<torch::Tensor> gb, torch::Tensor ws,
                          std::vector<int64_t> geom, bool defer) {
  const CPCall c = cp_call(geom);
  const dfa::CPGeom& g = c.p.g;
  CPIn in = cp_input(x, idx, c.B, (int64_t)g.H * g.W * g.C);
  need(dp, at::kBFloat16, "dp");
  need(code, at::kByte, "code");
  TORCH_CHECK(dp.numel() >= c.pn && code.numel() >= c.pn, "dp/code too small");
  need(gw, at::kFloat, "gw");
  TORCH_CHECK(gw.numel() >= (int64_t)g.N * g.K, "gw too small");
  float* gbp = opt_ptr<float>(gb, at::kFloat, "gb", g.N, "gb too small");
  need(ws, at::kFloat, "workspace");
  int slabs = 0;
  check_hip(dfa::convpool_wgrad(c.p, c.B, in.x, in.u8, in.idx, in.nrows, (float)scale, (const dfa::bf16*)dp.data_ptr(),
                                code.data_ptr<uint8_t>(), gw.data_ptr<float>(), gbp, ws.data_ptr<float>(),
                                (size_t)ws.numel(), cur_stream(), defer ? &slabs : nullptr),
            "convpool_wgrad");
  return slabs;  // > 0: the slab reduction was deferred (run it with slab_reduce_multi)
}

// One launch for several deferred slab reductions: segs = [(partial, gw, gb|None, N, K, Kt, S, scale), ...]
void slab_reduce_multi_py(std::vector<py::tuple> segs) {
  TORCH_CHECK(!segs.empty() && (int)segs.size() <= dfa::kMaxSlabSegs, "slab_reduce_multi: 1..8 segments");
  dfa::SlabSegs ss{};
  ss.n = (int)segs.size();
  for (size_t i = 0; i < segs.size(); ++i) {
    const py::tuple& t = segs[i];
    TORCH_CHECK(t.size() == 8, "segment = (partial, gw, gb, N, K, Kt, S, scale)");
    auto partial = t[0].cast<torch::Tensor>();
    auto gw = t[1].cast<torch::Tensor>();
    const int N = t[3].cast<int>(), K = t[4].cast<int>(), Kt = t[5].cast<int>(), S = t[6].cast<int>();
    need(partial, at::kFloat, "partial");
    need(gw, at::kFloat, "gw");
    TORCH_CHECK(N > 0 && K > 0 && Kt >= K && S > 0, "slab_reduce_multi: bad segment sizes");
    TORCH_CHECK(partial.numel() >= (int64_t)S * N * Kt && gw.numel() >= (int64_t)N * K, "slab_reduce_multi: buffers too small");
    dfa::SlabSeg& sg = ss.s[i];
    sg.partial = partial.data_ptr<float>();
    sg.gw = gw.data_ptr<float>();
    sg.gb = nullptr;
    if (!t[2].is_none()) {
      auto gb = t[2].cast<torch::Tensor>();
      need(gb, at::kFloat, "gb");
      TORCH_CHECK(gb.numel() >= N, "gb too small");
      sg.gb = gb.data_ptr<float>();
    }
    sg.N = N; sg.K = K; sg.Kt = Kt; sg.S = S;
    sg.scale = t[7].cast<float>();
  }
  check_hip(dfa::slab_reduce_multi(ss, cur_stream()), "slab_reduce_multi");
}

void convpool_dgrad_py(torch::Tensor dp, torch::Tensor code, torch::Tensor wt, torch::Tensor dx,
                       std::vector<int64_t> geom) {
  const CPCall c = cp_call(geom);
  const dfa::CPGeom& g = c.p.g;
  const dfa::CPDgrad& d = c.p.d;
  need(dp, at::kBFloat16, "dp");
  need(code, at::kByte, "code");
  TORCH_CHECK(dp.numel() >= c.pn && code.numel() >= c.pn, "dp/code too small");
  need(wt, at::kBFloat16, "wt");
  const int rows = d.pair ? 16 : (g.C + 15) / 16 * 16;
  TORCH_CHECK(wt.size(-1) == d.K2pad && wt.numel() >= (int64_t)rows * d.K2pad, "wt must be the dgrad layout [", rows,
              "][", d.K2pad, "] (pair ", d.pair, ")");
  need(dx, at::kBFloat16, "dx");
  TORCH_CHECK(dx.numel() >= (int64_t)c.B * g.H * g.W * g.C, "dx too small");
  check_hip(dfa::convpool_dgrad(c.p, c.B, (const dfa::bf16*)dp.data_ptr(), code.data_ptr<uint8_t>(),
                                (const dfa::bf16*)wt.data_ptr(), (dfa::bf16*)dx.data_ptr(), cur_stream()),
            "convpool_dgrad");
}

// The plan of a geometry as a dict (no GPU needed).  B > 0 adds the launch sizes for that batch and a weight-
// gradient workspace of ws_floats (these ask the device for the kernels' occupancy; nothing is launched; the
// data gradient is sized for aligned dp / code).
py::dict convpool_plan_py(int64_t H, int64_t W, int64_t C, int64_t KH, int64_t KW, int64_t pad, int64_t N, int64_t B,
                          int64_t ws_floats) {
  using namespace pybind11::literals;
  const dfa::CPPlan& p = dfa::convpool_plan(H, W, C, KH, KW, pad, N);
  py::dict r("ok"_a = p.ok, "Cp"_a = p.g.Cp, "Kpad2"_a = p.g.wKpad2, "pair"_a = p.g.pair, "dgrad_pair"_a = p.d.pair,
             "K2pad"_a = p.d.K2pad);
  if (!p.ok) return r;
  auto launch = [&](const char* name, py::tuple key, int inst, const int* have, auto size) {
    py::list l;
    for (; *have; ++have) l.append(*have);
    py::dict d("key"_a = key, "instance"_a = inst, "instantiated"_a = l);
    if (B > 0) {
      const dfa::CPSizing z = size();
      d["imgs"] = z.imgs, d["grid"] = z.grid, d["lds"] = z.lds;
    }
    r[name] = d;
  };
  static const char* const kKind[] = {"pair", "vec", "scalar"};
  launch("fwd", py::make_tuple(p.g.pair, p.fwd_NT, p.fwd_nk), p.fwd_NK, p.fwd_list,
         [&] { return dfa::convpool_size_fwd(p, (int)B); });
  launch("wgrad", py::make_tuple(p.wg_NT, p.wg_KT), p.wg_KTMAX, p.wg_list,
         [&] { return dfa::convpool_size_wgrad(p, (int)B, (size_t)ws_floats); });
  launch("dgrad", py::make_tuple(kKind[p.dg_kind], p.dg_nk), p.dg_NKMAX, p.dg_list,
         [&] { return dfa::convpool_size_dgrad(p, (int)B); });
  return r;
}

// a dense head's labels: read through idx (a dataset of any length) or row by row (at least B)
template <typename A>
void set_labels(A& a, const torch::Tensor& labels, const c10::optional<torch::Tensor>& idx, int64_t B,
                const char* idx_small, const char* labels_small) {
  need(labels, at::kInt, "labels");
  a.labels = labels.data_ptr<int>();
  a.nrows = labels.numel();
  a.idx = opt_ptr<const long long>(idx, at::kLong, "idx", B, idx_small);
  TORCH_CHECK(a.idx || labels.numel() >= B, labels_small);
}

// Fused dense head: per layer l tensors (w, wt?, b?, gw, gb?, hT?, dzT) and dims (K, N).
void head_train_py(std::vector<torch::Tensor> w, std::vector<c10::optional<torch::Tensor>> wt,
                   std::vector<c10::optional<torch::Tensor>> b, std::vector<torch::Tensor> gw,
                   std::vector<c10::optional<torch::Tensor>> gb, std::vector<c10::optional<torch::Tensor>> hT,
                   std::vector<torch::Tensor> dzT, std::vector<int64_t> K, std::vector<int64_t> N, torch::Tensor x,
                   bool x_relu, torch::Tensor xT, c10::optional<torch::Tensor> dx,
                   c10::optional<torch::Tensor> logits, torch::Tensor labels, c10::optional<torch::Tensor> idx,
                   double grad_scale, torch::Tensor loss_part, torch::Tensor stats, int64_t phases,
                   double dx_scale) {
  const int nl = (int)w.size();
  TORCH_CHECK(phases >= 1 && phases <= 3, "head: phases must be 1, 2 or 3");
  TORCH_CHECK(nl >= 1 && nl <= dfa::kHeadMaxLayers, "head: 1..", dfa::kHeadMaxLayers, " layers");
  TORCH_CHECK((int)wt.size() == nl && (int)b.size() == nl && (int)gw.size() == nl && (int)gb.size() == nl &&
                  (int)hT.size() == nl && (int)dzT.size() == nl && (int)K.size() == nl && (int)N.size() == nl,
              "head: per-layer lists must have equal length");
  need(x, at::kBFloat16, "x");
  TORCH_CHECK(x.dim() >= 2, "x must be [B, ...]");
  const int64_t B = x.size(0);
  const int64_t ldt = (B + 31) / 32 * 32;
  TORCH_CHECK(x.numel() == B * K[0], "x must have B*K0 elements");
  // (the weight-gradient phase alone streams X^T: any K0; the forward phase stages X rows in LDS, 16 bytes at a
  // time when K0 is a multiple of 8 and element by element otherwise)
  TORCH_CHECK(K[0] >= 1 && (K[0] <= 1024 || phases == 2), "head: K0 must be in [1, 1024]");
  TORCH_CHECK(N[nl - 1] <= 16, "head: at most 16 classes");
  dfa::HeadArgs a{};
  a.nl = nl;
  a.B = (int)B;
  a.ldt = (int)ldt;
  a.x_relu = x_relu ? 1 : 0;
  for (int l = 0; l < nl; ++l) {
    dfa::HeadLayer& L = a.L[l];
    L.K = (int)K[l];
    L.N = (int)N[l];
    TORCH_CHECK(L.N <= 256 || l == 0, "head: hidden widths must be <= 256");
    TORCH_CHECK(l == 0 || K[l] == N[l - 1], "head: layer ", l, " input width must equal layer ", l - 1, " width");
    L.Kpad = (L.K + 31) / 32 * 32;
    L.ldwt = (L.N + 31) / 32 * 32;
    need(w[l], at::kBFloat16, "w");
    TORCH_CHECK(w[l].numel() >= (int64_t)((L.N + 15) / 16 * 16) * L.Kpad && w[l].size(-1) == L.Kpad,
                "head: w must be [Npad16][Kpad32]");
    L.w = reinterpret_cast<const dfa::bf16*>(w[l].data_ptr());
    const bool need_wt = l > 0 || has(dx);
    if (need_wt) {
      TORCH_CHECK(has(wt[l]), "head: dgrad-layout weights required for layer ", l);
      need(*wt[l], at::kBFloat16, "wt");
      TORCH_CHECK(wt[l]->size(-1) == L.ldwt && wt[l]->numel() >= (int64_t)((L.K + 15) / 16 * 16) * L.ldwt,
                  "head: wt must be [Kpad16][pad32(N)]");
      L.wt = reinterpret_cast<const dfa::bf16*>(wt[l]->data_ptr());
    }
    L.b = opt_ptr<float>(b[l], at::kFloat, "b", L.N, "head: bias too small");
    need(gw[l], at::kFloat, "gw");
    TORCH_CHECK(gw[l].numel() >= (int64_t)L.N * L.K, "head: gw too small");
    L.gw = gw[l].data_ptr<float>();
    L.gb = opt_ptr<float>(gb[l], at::kFloat, "gb", L.N, "head: gb too small");
    if (l < nl - 1) {
      TORCH_CHECK(has(hT[l]), "head: hT required for hidden layers");
      need(*hT[l], at::kBFloat16, "hT");
      TORCH_CHECK(hT[l]->numel() >= (int64_t)L.N * ldt, "head: hT must be [N][round32(B)]");
      L.hT = reinterpret_cast<dfa::bf16*>(hT[l]->data_ptr());
    }
    need(dzT[l], at::kBFloat16, "dzT");
    TORCH_CHECK(dzT[l].numel() >= (int64_t)L.N * ldt, "head: dzT must be [N][round32(B)]");
    L.dzT = reinterpret_cast<dfa::bf16*>(dzT[l].data_ptr());
  }
  a.x = reinterpret_cast<const dfa::bf16*>(x.data_ptr());
  need(xT, at::kBFloat16, "xT");
  TORCH_CHECK(xT.numel() >= K[0] * ldt, "head: xT must be [K0][round32(B)]");
  a.xT = reinterpret_cast<dfa::bf16*>(xT.data_ptr());
  a.dx = opt_ptr<dfa::bf16>(dx, at::kBFloat16, "dx", B * K[0], "head: dx too small");
  a.logits = opt_ptr<float>(logits, at::kFloat, "logits", B * N[nl - 1], "head: logits too small");
  set_labels(a, labels, idx, B, "head: idx too small", "head: labels too small");
  a.grad_scale = (float)grad_scale;
  need(loss_part, at::kFloat, "loss_part");
  TORCH_CHECK(loss_part.numel() >= 2 * ((B + 15) / 16), "head: loss_part must hold 2 floats per 16 rows");
  a.loss_part = loss_part.data_ptr<float>();
  need(stats, at::kFloat, "stats");
  TORCH_CHECK(stats.numel() >= 2, "head: stats must hold 2 floats");
  a.stats = stats.data_ptr<float>();
  TORCH_CHECK(phases == 2 || dfa::head_train_lds(a) <= 160 * 1024, "head: LDS footprint too large");
  a.dx_scale = (float)dx_scale;
  check_hip(dfa::head_train(a, (int)phases, cur_stream()), "head_train");
}

// The reference CNN's dense head (csrc/khead.hip): forward, softmax-CE and both data gradients in one
// launch; the weight gradients then come from head_train(phases=2) over (pT, h1T, dz1T, dz2T).
void khead_train_py(torch::Tensor p, torch::Tensor pT, c10::optional<torch::Tensor> dp, torch::Tensor w1,
                    torch::Tensor w1t, c10::optional<torch::Tensor> b1, torch::Tensor w2, torch::Tensor w2t,
                    c10::optional<torch::Tensor> b2, double drop_p, int64_t drop_seed,
                    c10::optional<torch::Tensor> drop_step, int64_t drop_step_add, double dh_scale, double dp_scale,
                    bool dp_mask, torch::Tensor h1T, torch::Tensor dz1T, torch::Tensor dz2T,
                    c10::optional<torch::Tensor> logits, torch::Tensor labels, c10::optional<torch::Tensor> idx,
                    double grad_scale, torch::Tensor loss_part, torch::Tensor ws) {
  need(p, at::kBFloat16, "p");
  TORCH_CHECK(p.dim() >= 2, "p must be [B, ...]");
  const int64_t B = p.size(0), K = p.numel() / std::max<int64_t>(B, 1);
  const int64_t ldt = (B + 31) / 32 * 32;
  const int64_t C = dz2T.size(0);
  TORCH_CHECK(dfa::khead_supported((int)K, (int)C), "khead: K must be a multiple of 256 (LDS-bounded), 1 <= C <= 16");
  const int N1 = dfa::kKHeadN1;
  dfa::KHeadArgs a{};
  a.B = (int)B;
  a.K = (int)K;
  a.C = (int)C;
  a.ldt = (int)ldt;
  a.p = reinterpret_cast<const dfa::bf16*>(p.data_ptr());
  need(pT, at::kBFloat16, "pT");
  TORCH_CHECK(pT.numel() >= K * ldt, "khead: pT must be [K][round32(B)]");
  a.pT = reinterpret_cast<dfa::bf16*>(pT.data_ptr());
  a.dp = opt_ptr<dfa::bf16>(dp, at::kBFloat16, "dp", B * K, "khead: dp too small");
  need(w1, at::kBFloat16, "w1");
  TORCH_CHECK(w1.dim() == 2 && w1.size(0) >= N1 && w1.size(1) >= K, "khead: w1 must be [128][>= K]");
  a.w1 = reinterpret_cast<const dfa::bf16*>(w1.data_ptr());
  a.ldw1 = (int)w1.size(1);
  need(w1t, at::kBFloat16, "w1t");
  TORCH_CHECK(w1t.dim() == 2 && w1t.size(0) >= K && w1t.size(1) == N1, "khead: w1t must be [>= K][128]");
  a.w1t = reinterpret_cast<const dfa::bf16*>(w1t.data_ptr());
  need(w2, at::kBFloat16, "w2");
  TORCH_CHECK(w2.dim() == 2 && w2.size(0) >= 16 && w2.size(1) == N1, "khead: w2 must be [16][128]");
  a.w2 = reinterpret_cast<const dfa::bf16*>(w2.data_ptr());
  need(w2t, at::kBFloat16, "w2t");
  TORCH_CHECK(w2t.dim() == 2 && w2t.size(0) >= N1 && w2t.size(1) == 32, "khead: w2t must be [128][32]");
  a.w2t = reinterpret_cast<const dfa::bf16*>(w2t.data_ptr());
  a.b1 = opt_ptr<float>(b1, at::kFloat, "b1", N1, "khead: b1 too small");
  a.b2 = opt_ptr<float>(b2, at::kFloat, "b2", C, "khead: b2 too small");
  a.drop = drop_from(drop_p, drop_seed, drop_step, drop_step_add);
  a.dh_scale = (float)dh_scale;
  a.dp_scale = (float)dp_scale;
  a.dp_mask = dp_mask ? 1 : 0;
  for (auto* t : {&h1T, &dz1T}) {
    need(*t, at::kBFloat16, "h1T/dz1T");
    TORCH_CHECK(t->numel() >= N1 * ldt, "khead: h1T / dz1T must be [128][round32(B)]");
  }
  need(dz2T, at::kBFloat16, "dz2T");
  TORCH_CHECK(dz2T.numel() >= C * ldt, "khead: dz2T must be [C][round32(B)]");
  a.h1T = reinterpret_cast<dfa::bf16*>(h1T.data_ptr());
  a.dz1T = reinterpret_cast<dfa::bf16*>(dz1T.data_ptr());
  a.dz2T = reinterpret_cast<dfa::bf16*>(dz2T.data_ptr());
  a.logits = opt_ptr<float>(logits, at::kFloat, "logits", B * C, "khead: logits too small");
  set_labels(a, labels, idx, B, "khead: idx too small", "khead: labels too small");
  a.grad_scale = (float)grad_scale;
  need(loss_part, at::kFloat, "loss_part");
  TORCH_CHECK(loss_part.numel() >= 2 * ((B + 15) / 16), "khead: loss_part must hold 2 floats per 16 rows");
  a.loss_part = loss_part.data_ptr<float>();
  need(ws, at::kFloat, "ws");
  TORCH_CHECK(ws.numel() >= (int64_t)dfa::khead_ws_floats((int)B, (int)K), "khead: workspace too small");
  const int64_t nt = (B + 31) / 32;
  float* base = ws.data_ptr<float>();
  a.slab = base;
  a.dz1 = reinterpret_cast<dfa::bf16*>(base + nt * dfa::kKHeadChunks * 32 * N1);
  a.sync = reinterpret_cast<unsigned*>(base + nt * dfa::kKHeadChunks * 32 * N1 + nt * 32 * N1 / 2);
  check_hip(dfa::khead_train(a, cur_stream()), "khead_train");
}

// Weight gradients of that head (csrc/khead.hip khead_wgrad_kernel) + the stats reduction: one launch.
void khead_wgrad_py(torch::Tensor pT, torch::Tensor h1T, torch::Tensor dz1T, torch::Tensor dz2T, torch::Tensor gw1,
                    c10::optional<torch::Tensor> gb1, torch::Tensor gw2, c10::optional<torch::Tensor> gb2, int64_t B,
                    int64_t K, int64_t C, torch::Tensor loss_part, torch::Tensor stats) {
  const int64_t ldt = (B + 31) / 32 * 32;
  const int N1 = dfa::kKHeadN1;
  for (auto* t : {&pT, &h1T, &dz1T, &dz2T}) need(*t, at::kBFloat16, "khead wgrad operand");
  TORCH_CHECK(pT.numel() >= K * ldt && h1T.numel() >= N1 * ldt && dz1T.numel() >= N1 * ldt &&
                  dz2T.numel() >= C * ldt, "khead_wgrad: operands must be [rows][round32(B)]");
  need(gw1, at::kFloat, "gw1");
  need(gw2, at::kFloat, "gw2");
  TORCH_CHECK(gw1.numel() >= N1 * K && gw2.numel() >= C * N1, "khead_wgrad: gradient buffers too small");
  dfa::KHeadWgradArgs a{};
  a.ldt = (int)ldt;
  a.L[0] = {reinterpret_cast<const dfa::bf16*>(dz1T.data_ptr()), reinterpret_cast<const dfa::bf16*>(pT.data_ptr()),
            gw1.data_ptr<float>(), nullptr, N1, (int)K, 0, 0};
  a.L[1] = {reinterpret_cast<const dfa::bf16*>(dz2T.data_ptr()), reinterpret_cast<const dfa::bf16*>(h1T.data_ptr()),
            gw2.data_ptr<float>(), nullptr, (int)C, N1, 0, 0};
  a.L[0].gb = opt_ptr<float>(gb1, at::kFloat, "gb1");
  a.L[1].gb = opt_ptr<float>(gb2, at::kFloat, "gb2");
  need(loss_part, at::kFloat, "loss_part");
  need(stats, at::kFloat, "stats");
  a.nloss = (int)((B + 15) / 16);
  TORCH_CHECK(loss_part.numel() >= 2 * a.nloss && stats.numel() >= 2, "khead_wgrad: loss_part / stats too small");
  a.loss_part = loss_part.data_ptr<float>();
  a.stats = stats.data_ptr<float>();
  check_hip(dfa::khead_wgrad(a, cur_stream()), "khead_wgrad");
}

// Whole-network LeNet-5 training step (csrc/lenet_fused.hip): fills the gradients of all ten
// parameters and stats = [loss sum, correct].  x: uint8 dataset [nrows][28][28][1] read through idx,
// or a bf16 batch [B][28][28][1].  With ``sgd_*`` the reduce launch applies the update; with ``ll``
// (a world > 1 P2PComm) it first sums every gradient over the ranks in-kernel (no all-reduce launch).
void lenet_train_py(torch::Tensor x, c10::optional<torch::Tensor> idx, double scale, torch::Tensor labels,
                    std::vector<torch::Tensor> conv, std::vector<torch::Tensor> dense_w,
                    std::vector<torch::Tensor> dense_b,
                    std::vector<torch::Tensor> conv_grads, std::vector<torch::Tensor> dense_gw,
                    std::vector<torch::Tensor> dense_gb, std::vector<torch::Tensor> hT, std::vector<torch::Tensor> dzT,
                    torch::Tensor conv_part, torch::Tensor dense_part, torch::Tensor loss_part, torch::Tensor stats,
                    torch::Tensor frag, torch::Tensor ftab, torch::Tensor pxtab, int64_t B, double grad_scale,
                    bool prep, c10::optional<torch::Tensor> snap, std::vector<torch::Tensor> conv_mom,
                    c10::optional<torch::Tensor> sgd_master, c10::optional<torch::Tensor> sgd_mom,
                    c10::optional<torch::Tensor> sgd_wbf, c10::optional<torch::Tensor> sgd_hyper,
                    c10::optional<torch::Tensor> sgd_descs, c10::optional<torch::Tensor> idx_stream,
                    c10::optional<torch::Tensor> idx_cursor, c10::optional<torch::Tensor> idx_dst,
                    const P2PComm* ll, int64_t exch_blocks, c10::optional<torch::Tensor> run_stats,
                    const PSComm* ps, c10::optional<torch::Tensor> ps_perm, c10::optional<torch::Tensor> ps_idx,
                    double ps_lr, int64_t ps_max_stale, bool red_succ) {
  TORCH_CHECK(conv.size() == 4 && conv_grads.size() == 4, "lenet: conv = [w1, b1, w2, b2]");
  TORCH_CHECK(dense_w.size() == 3 && dense_b.size() == 3 && dense_gw.size() == 3 &&
                  dense_gb.size() == 3 && hT.size() == 3 && dzT.size() == 3,
              "lenet: three dense layers");
  TORCH_CHECK(B > 0 && B < (1 << 30), "lenet: bad batch");
  dfa::LeNetArgs a{};
  const int64_t ldt = (B + 31) / 32 * 32;  // batch columns of H^T / dZ^T the reduce sums over
  // row stride of H^T / dZ^T: any multiple of 32 >= ldt (the trainer pads it off a power of two)
  const int64_t lds = hT.size() == 3 && hT[0].dim() == 2 ? hT[0].size(1) : 0;
  TORCH_CHECK(lds >= ldt && lds % 32 == 0, "lenet: hT rows must hold round32(B) columns, stride a multiple of 32");
  if (x.scalar_type() == at::kByte) {
    TORCH_CHECK(x.is_cuda() && x.is_contiguous() && x.numel() % 784 == 0, "lenet: uint8 dataset [N][28][28][1]");
    a.x_u8 = x.data_ptr<uint8_t>();
    a.nrows = x.numel() / 784;
    TORCH_CHECK(has(idx) || a.nrows >= B,
                "lenet: a uint8 dataset without batch indices must hold the batch (rows 0 .. B-1)");
  } else {
    need(x, at::kBFloat16, "lenet x");
    TORCH_CHECK(x.numel() == B * 784, "lenet: x must be [B][28][28][1]");
    a.x_bf = reinterpret_cast<const dfa::bf16*>(x.data_ptr());
    a.nrows = B;
  }
  if (has(idx)) {
    need(*idx, at::kLong, "lenet idx");
    TORCH_CHECK(idx->numel() == B, "lenet: idx must have B entries");
    a.idx = reinterpret_cast<const long long*>(idx->data_ptr());
    if (a.x_u8 == nullptr) a.nrows = labels.numel();
  }
  need(labels, at::kInt, "lenet labels");
  TORCH_CHECK(labels.numel() >= (a.idx ? 1 : B), "lenet: labels too small");
  if (a.idx) a.nrows = std::min<int64_t>(a.nrows, labels.numel());
  a.labels = labels.data_ptr<int>();
  a.scale = (float)scale;
  const int64_t conv_n[4] = {150, 6, 2400, 16};
  for (int k = 0; k < 4; ++k) {
    need(conv[k], at::kFloat, "lenet conv param");
    need(conv_grads[k], at::kFloat, "lenet conv grad");
    TORCH_CHECK(conv[k].numel() == conv_n[k] && conv_grads[k].numel() == conv_n[k], "lenet: conv param size");
  }
  a.w1 = conv[0].data_ptr<float>();
  a.b1 = conv[1].data_ptr<float>();
  a.w2 = conv[2].data_ptr<float>();
  a.b2 = conv[3].data_ptr<float>();
  const int64_t NK[3][2] = {{120, 400}, {84, 120}, {10, 84}};
  const float* dw[3];
  const float* db[3];
  for (int l = 0; l < 3; ++l) {
    // the fp32 master kernels [N][K]: the prep launch builds the dense fragments from them (the train
    // kernel itself reads the fragment buffer only)
    need(dense_w[l], at::kFloat, "lenet dense w");
    need(dense_b[l], at::kFloat, "lenet dense b");
    TORCH_CHECK(dense_w[l].numel() == NK[l][0] * NK[l][1], "lenet: dense ", l, " kernel must be [", NK[l][0], "][",
                NK[l][1], "]");
    TORCH_CHECK(dense_b[l].numel() == NK[l][0], "lenet: dense bias size");
    need(dense_gw[l], at::kFloat, "lenet dense gw");
    need(dense_gb[l], at::kFloat, "lenet dense gb");
    TORCH_CHECK(dense_gw[l].numel() == NK[l][0] * NK[l][1] && dense_gb[l].numel() == NK[l][0],
                "lenet: dense grad size");
    need(hT[l], at::kBFloat16, "lenet hT");
    need(dzT[l], at::kBFloat16, "lenet dzT");
    // block layout (csrc/lenet_frag.h lenet_act_pos): whole 16-row tiles, the padding rows zero
    TORCH_CHECK(hT[l].dim() == 2 && hT[l].size(0) >= (NK[l][1] + 15) / 16 * 16 && hT[l].size(1) == lds,
                "lenet: hT must be [>= round16(K)][ldt]");
    TORCH_CHECK(dzT[l].dim() == 2 && dzT[l].size(0) >= (NK[l][0] + 15) / 16 * 16 && dzT[l].size(1) == lds,
                "lenet: dzT must be [>= round16(N)][ldt]");
    dw[l] = dense_w[l].data_ptr<float>();
    db[l] = dense_b[l].data_ptr<float>();
  }
  a.d1m = dw[0]; a.d2m = dw[1]; a.d3m = dw[2];
  a.d1b = db[0]; a.d2b = db[1]; a.d3b = db[2];
  const int nblk = dfa::lenet_blocks((int)B);
  need(conv_part, at::kFloat, "lenet conv_part");
  need(loss_part, at::kFloat, "lenet loss_part");
  need(stats, at::kFloat, "lenet stats");
  TORCH_CHECK(conv_part.numel() >= (int64_t)dfa::kLeNetConvStride * nblk, "lenet: conv_part too small");
  TORCH_CHECK(loss_part.numel() >= 2 * nblk && stats.numel() >= 2, "lenet: loss buffers too small");
  a.conv_part = conv_part.data_ptr<float>();
  a.loss_part = loss_part.data_ptr<float>();
  auto bp = [](torch::Tensor& t) { return reinterpret_cast<dfa::bf16*>(t.data_ptr()); };
  a.h0T = bp(hT[0]); a.h1T = bp(hT[1]); a.h2T = bp(hT[2]);
  a.dz1T = bp(dzT[0]); a.dz2T = bp(dzT[1]); a.dz3T = bp(dzT[2]);
  TORCH_CHECK(frag.is_cuda() && frag.is_contiguous() && (size_t)frag.nbytes() >= dfa::lenet_frag_bytes(),
              "lenet: fragment buffer too small");
  TORCH_CHECK(ftab.is_cuda() && ftab.scalar_type() == at::kByte && ftab.numel() == 98 * 2 * 16, "lenet: ftab");
  TORCH_CHECK(pxtab.is_cuda() && pxtab.scalar_type() == at::kShort && pxtab.numel() == 832 + 104, "lenet: pxtab");
  a.frag = frag.data_ptr();
  a.prep = prep ? 1 : 0;
  a.ftab = ftab.data_ptr<uint8_t>();
  a.pxtab = reinterpret_cast<const unsigned short*>(pxtab.data_ptr());
  a.B = (int)B;
  a.ldt = (int)lds;
  a.grad_scale = (float)grad_scale;
  dfa::LeNetRedArgs r{};
  r.kcols = (int)ldt;
  // reduce scratch: job slabs, then the arrival tickets (zero-initialised by the trainer)
  need(dense_part, at::kFloat, "lenet dense_part");
  TORCH_CHECK(dense_part.numel() >= dfa::lenet_dense_part_floats((int)B),
              "lenet: dense_part must hold lenet_dense_part_floats(B) zero-initialised floats");
  dfa::lenet_red_bind_scratch(dense_part.data_ptr<float>(), r);
  r.succ = red_succ ? 1 : 0;  // (the launcher falls back to tickets where successor ownership cannot run)
  r.conv_part = a.conv_part;
  r.loss_part = a.loss_part;
  r.stats = stats.data_ptr<float>();
  r.g_w1 = conv_grads[0].data_ptr<float>();
  r.g_b1 = conv_grads[1].data_ptr<float>();
  r.g_w2 = conv_grads[2].data_ptr<float>();
  r.g_b2 = conv_grads[3].data_ptr<float>();
  for (int l = 0; l < 3; ++l) {
    r.L[l].dzT = reinterpret_cast<const dfa::bf16*>(dzT[l].data_ptr());
    r.L[l].hT = reinterpret_cast<const dfa::bf16*>(hT[l].data_ptr());
    r.L[l].gw = dense_gw[l].data_ptr<float>();
    r.L[l].gb = dense_gb[l].data_ptr<float>();
    r.L[l].N = (int)NK[l][0];
    r.L[l].K = (int)NK[l][1];
  }
  // optional pre-update snapshot of the conv kernels (weights, momentum) for the optimizer's fragment rebuild
  r.w1 = a.w1;
  r.w2 = a.w2;
  if (has(snap)) {
    need(*snap, at::kFloat, "lenet snap");
    TORCH_CHECK(snap->numel() >= 2 * 2550, "lenet: snap must hold 2 x 2550 floats");
    r.snap = snap->data_ptr<float>();
    TORCH_CHECK(conv_mom.empty() || conv_mom.size() == 2, "lenet: conv_mom = [m1, m2] or []");
    if (conv_mom.size() == 2) {
      need(conv_mom[0], at::kFloat, "lenet m1");
      need(conv_mom[1], at::kFloat, "lenet m2");
      TORCH_CHECK(conv_mom[0].numel() == 150 && conv_mom[1].numel() == 2400, "lenet: conv momentum sizes");
      r.m1 = conv_mom[0].data_ptr<float>();
      r.m2 = conv_mom[1].data_ptr<float>();
    }
  }
  if (has(sgd_master)) {
    // single-rank fast path: the reduce kernel applies the SGD update (see LeNetSgd)
    need(*sgd_master, at::kFloat, "lenet sgd master");
    TORCH_CHECK(sgd_wbf.has_value() && sgd_hyper.has_value() && sgd_descs.has_value(),
                "lenet sgd: wbf, hyper and descs are required");
    need(*sgd_wbf, at::kBFloat16, "lenet sgd wbf");
    need(*sgd_hyper, at::kFloat, "lenet sgd hyper");
    TORCH_CHECK(sgd_hyper->numel() >= 5, "lenet sgd: hyper size");
    const torch::Tensor& dh = *sgd_descs;
    TORCH_CHECK(!dh.is_cuda() && dh.scalar_type() == at::kLong && dh.is_contiguous() &&
                    dh.numel() * 8 >= 10 * (int64_t)sizeof(dfa::ParamDesc),
                "lenet sgd: descs must be the host int64 table of the 10 parameters");
    r.sgd_on = 1;
    r.sgd.master = sgd_master->data_ptr<float>();
    r.sgd.mom = has(sgd_mom) ? sgd_mom->data_ptr<float>() : nullptr;
    r.sgd.wbf = reinterpret_cast<dfa::bf16*>(sgd_wbf->data_ptr());
    r.sgd.hyper = sgd_hyper->data_ptr<float>();
    const auto* hd = reinterpret_cast<const dfa::ParamDesc*>(dh.data_ptr());
    for (int k = 0; k < 10; ++k) {
      r.sgd.d[k] = hd[k];
      TORCH_CHECK(hd[k].off >= 0 && hd[k].off + hd[k].numel <= sgd_master->numel(), "lenet sgd: descriptor range");
    }
    TORCH_CHECK(r.sgd.d[0].off == conv[0].data_ptr<float>() - r.sgd.master &&
                    r.sgd.d[2].off == conv[2].data_ptr<float>() - r.sgd.master,
                "lenet sgd: descriptors do not match the conv parameters");
    if (has(idx_stream)) {
      need(*idx_stream, at::kLong, "lenet idx_stream");
      TORCH_CHECK(idx_cursor.has_value() && idx_dst.has_value(), "lenet sgd: index stream needs cursor and dst");
      TORCH_CHECK(idx_stream->dim() == 2 && idx_stream->size(1) == idx_dst->numel(), "lenet sgd: stream shape");
      r.sgd.src = reinterpret_cast<const long long*>(idx_stream->data_ptr());
      r.sgd.cursor = reinterpret_cast<long long*>(idx_cursor->data_ptr());
      r.sgd.dst = reinterpret_cast<long long*>(idx_dst->data_ptr());
      r.sgd.B = (int)idx_dst->numel();
      r.sgd.nsteps = (int)idx_stream->size(0);
    }
    r.sgd.run_stats = opt_ptr<float>(run_stats, at::kFloat, "run_stats", 3,
                                     "run_stats must hold [loss sum, correct, updates]");
    r.sgd.frag = frag.data_ptr();
  }
  if (ll != nullptr) {
    TORCH_CHECK(r.sgd_on, "lenet: the in-kernel LL exchange needs the fused update (sgd_* arguments)");
    r.ll = ll->ll_args();
    TORCH_CHECK(r.ll.world > 1, "lenet: LL exchange needs world > 1");
    r.ll_on = 1;
  }
  if (ps != nullptr) {
    TORCH_CHECK(r.sgd_on && !r.ll_on, "lenet: the parameter-server mode needs the fused update and no LL exchange");
    TORCH_CHECK(r.sgd.mom == nullptr, "lenet: the parameter server applies plain SGD (no momentum)");
    TORCH_CHECK(!has(idx_stream), "lenet: the parameter server stages the next microbatch itself (no index stream)");
    TORCH_CHECK(has(ps_perm) && has(ps_idx),
                "lenet: the parameter-server mode needs the microbatch table and the index buffer");
    TORCH_CHECK(a.idx == reinterpret_cast<const long long*>(ps_idx->data_ptr()),
                "lenet: the parameter server must stage into the batch index buffer the step reads");
    r.ps = ps->lenet_args(*ps_perm, *ps_idx, ps_lr, ps_max_stale);
    r.ps_on = 1;
  }
  TORCH_CHECK(exch_blocks >= 0 && exch_blocks <= 512, "lenet: exch_blocks out of range");
  r.exch_blocks = (int)exch_blocks;
  check_hip(dfa::lenet_train(a, r, cur_stream()), "lenet_train");
}

// The reference CNN's conv block (csrc/kcnn_fused.hip).  x: uint8 dataset [nrows][28][28][1] (idx
// required), bf16 dataset rows (idx + scale), or a bf16 batch [B][28][28][1].
static dfa::KcnnArgs kcnn_args(torch::Tensor x, c10::optional<torch::Tensor> idx, double scale, int64_t B,
                               torch::Tensor w1, torch::Tensor b1, int64_t kpad1, torch::Tensor code) {
  dfa::KcnnArgs a{};
  TORCH_CHECK(B > 0 && B < (1 << 30), "kcnn: bad batch");
  TORCH_CHECK(x.is_cuda() && x.is_contiguous() && x.numel() % 784 == 0, "kcnn: x must be [.][28][28][1] on GPU");
  if (has(idx)) {
    need(*idx, at::kLong, "kcnn idx");
    TORCH_CHECK(idx->numel() == B, "kcnn: idx must have B entries");
    a.idx = reinterpret_cast<const long long*>(idx->data_ptr());
  }
  if (x.scalar_type() == at::kByte) {
    TORCH_CHECK(a.idx, "kcnn: a uint8 dataset needs batch indices");
    a.x_u8 = x.data_ptr<uint8_t>();
  } else {
    TORCH_CHECK(x.scalar_type() == at::kBFloat16, "kcnn: x must be uint8 or bf16");
    a.x_bf = reinterpret_cast<const dfa::bf16*>(x.data_ptr());
    TORCH_CHECK(a.idx || x.numel() == B * 784, "kcnn: x must be [B][28][28][1]");
  }
  a.nrows = x.numel() / 784;
  a.scale = (float)scale;
  need(w1, at::kBFloat16, "kcnn w1");
  need(b1, at::kFloat, "kcnn b1");
  TORCH_CHECK(kpad1 >= 9 && w1.numel() >= 32 * kpad1 && b1.numel() == 32, "kcnn: conv1 weights [32][kpad1]");
  a.w1 = reinterpret_cast<const dfa::bf16*>(w1.data_ptr());
  a.b1 = b1.data_ptr<float>();
  a.kpad1 = (int)kpad1;
  TORCH_CHECK(code.is_cuda() && code.is_contiguous() && code.scalar_type() == at::kByte && code.numel() == B * 144 * 32,
              "kcnn: code must be uint8 [B][12][12][32]");
  a.code = code.data_ptr<uint8_t>();
  a.B = (int)B;
  return a;
}

void kcnn_fwd_py(torch::Tensor x, c10::optional<torch::Tensor> idx, double scale, int64_t B, torch::Tensor w1,
                 torch::Tensor b1, int64_t kpad1, torch::Tensor w2, torch::Tensor b2, torch::Tensor pooled,
                 torch::Tensor code, double drop_p, int64_t drop_seed, c10::optional<torch::Tensor> drop_step,
                 int64_t drop_step_add) {
  dfa::KcnnArgs a = kcnn_args(x, idx, scale, B, w1, b1, kpad1, code);
  need(w2, at::kBFloat16, "kcnn w2");
  need(b2, at::kFloat, "kcnn b2");
  need(pooled, at::kBFloat16, "kcnn pooled");
  TORCH_CHECK(w2.numel() >= 32 * 288 && b2.numel() == 32 && pooled.numel() == B * 144 * 32, "kcnn: conv2 / pooled");
  a.w2 = reinterpret_cast<const dfa::bf16*>(w2.data_ptr());
  a.b2 = b2.data_ptr<float>();
  a.pooled = reinterpret_cast<dfa::bf16*>(pooled.data_ptr());
  a.drop = drop_from(drop_p, drop_seed, drop_step, drop_step_add);
  check_hip(dfa::kcnn_fwd(a, cur_stream()), "kcnn_fwd");
}

void kcnn_bwd_py(torch::Tensor x, c10::optional<torch::Tensor> idx, double scale, int64_t B, torch::Tensor w1,
                 torch::Tensor b1, int64_t kpad1, torch::Tensor w2t, torch::Tensor dyp, torch::Tensor code,
                 torch::Tensor slabs, torch::Tensor g_w1, torch::Tensor g_b1, torch::Tensor g_w2, torch::Tensor g_b2,
                 c10::optional<torch::Tensor> step_inc) {
  dfa::KcnnArgs a = kcnn_args(x, idx, scale, B, w1, b1, kpad1, code);
  need(w2t, at::kBFloat16, "kcnn w2t");
  need(dyp, at::kBFloat16, "kcnn dyp");
  need(slabs, at::kFloat, "kcnn slabs");
  TORCH_CHECK(w2t.numel() >= 32 * 288 && dyp.numel() == B * 144 * 32, "kcnn: dgrad weights / pooled gradient");
  TORCH_CHECK((size_t)slabs.numel() >= dfa::kcnn_slab_floats((int)B), "kcnn: slab workspace too small");
  for (auto* t : {&g_w1, &g_b1, &g_w2, &g_b2}) need(*t, at::kFloat, "kcnn grad");
  TORCH_CHECK(g_w1.numel() == 288 && g_b1.numel() == 32 && g_w2.numel() == 32 * 288 && g_b2.numel() == 32,
              "kcnn: gradient sizes");
  a.w2t = reinterpret_cast<const dfa::bf16*>(w2t.data_ptr());
  a.dyp = reinterpret_cast<const dfa::bf16*>(dyp.data_ptr());
  a.slab2 = slabs.data_ptr<float>();
  a.slab1 = a.slab2 + (size_t)dfa::kcnn_blocks((int)B) * 32 * 289;
  long long* sp = opt_ptr<long long>(step_inc, at::kLong, "kcnn step");
  check_hip(dfa::kcnn_bwd(a, g_w1.data_ptr<float>(), g_b1.data_ptr<float>(), g_w2.data_ptr<float>(),
                          g_b2.data_ptr<float>(), sp, cur_stream()),
            "kcnn_bwd");
}

}  // namespace

void bind_fused(py::module_& m) {
  m.def("convpool_fwd", &convpool_fwd_py, "fused conv+bias+relu+maxpool2x2 (pooled map + argmax codes)");
  m.def("convpool_wgrad", &convpool_wgrad_py, "weight gradient through the fused conv+pool", py::arg("x"),
        py::arg("idx"), py::arg("scale"), py::arg("dp"), py::arg("code"), py::arg("gw"), py::arg("gb"), py::arg("ws"),
        py::arg("geom"), py::arg("defer") = false);
  m.def("slab_reduce_multi", &slab_reduce_multi_py, "several deferred split-m slab reductions in one launch");
  m.def("convpool_dgrad", &convpool_dgrad_py, "data gradient through the fused conv+pool");
  m.def("convpool_set_stamps", [](c10::optional<torch::Tensor> buf) {
    if (has(buf)) {
      TORCH_CHECK(buf->is_cuda() && buf->scalar_type() == at::kLong && buf->numel() >= 4096 * 32,
                  "stamp buffer: int64 GPU tensor of >= 4096*32 elements");
      dfa::convpool_set_stamps(buf->data_ptr());
      dfa::head_set_stamps(buf->data_ptr());
      dfa::lenet_set_stamps(buf->data_ptr());
    } else {
      dfa::convpool_set_stamps(nullptr);
      dfa::head_set_stamps(nullptr);
      dfa::lenet_set_stamps(nullptr);
    }
  }, "profiling aid: per-block phase stamps of the convpool kernels");
  m.def("convpool_plan", &convpool_plan_py, "the launch plan of a fused conv+pool geometry", py::arg("H"), py::arg("W"),
        py::arg("C"), py::arg("KH"), py::arg("KW"), py::arg("pad"), py::arg("N"), py::arg("B") = 0,
        py::arg("ws_floats") = 0);
  m.def("head_train", &head_train_py, "fused dense head: forward + softmax-CE + backward (2 launches)",
        py::arg("w"), py::arg("wt"), py::arg("b"), py::arg("gw"), py::arg("gb"), py::arg("hT"), py::arg("dzT"),
        py::arg("K"), py::arg("N"), py::arg("x"), py::arg("x_relu"), py::arg("xT"), py::arg("dx"), py::arg("logits"),
        py::arg("labels"), py::arg("idx"), py::arg("grad_scale"), py::arg("loss_part"), py::arg("stats"),
        py::arg("phases"), py::arg("dx_scale") = 1.0);
  m.def("khead_train", &khead_train_py,
        "reference CNN dense head: forward + softmax-CE + both data gradients (1 launch, split-K)", py::arg("p"),
        py::arg("pT"), py::arg("dp"), py::arg("w1"), py::arg("w1t"), py::arg("b1"), py::arg("w2"), py::arg("w2t"),
        py::arg("b2"), py::arg("drop_p"), py::arg("drop_seed"), py::arg("drop_step"), py::arg("drop_step_add"),
        py::arg("dh_scale"), py::arg("dp_scale"), py::arg("dp_mask"),
        py::arg("h1T"), py::arg("dz1T"), py::arg("dz2T"), py::arg("logits"), py::arg("labels"), py::arg("idx"),
        py::arg("grad_scale"), py::arg("loss_part"), py::arg("ws"));
  m.def("khead_wgrad", &khead_wgrad_py, "reference CNN dense head: weight gradients + loss stats (1 launch)");
  m.def("khead_set_grid_cap", [](int64_t cus) { dfa::khead_set_grid_cap((int)cus); },
        "persistent dense-head grid cap (CUs) for ranks time-sharing one GPU; 0 = the whole chip");
  m.def("kcnn_set_stamps", [](c10::optional<torch::Tensor> buf) {
    dfa::kcnn_set_stamps(has(buf) ? buf->data_ptr() : nullptr);
  }, "profiling aid: per-image phase clocks of the reference CNN's fused backward ([G][2][16] int64)");
  m.def("khead_set_stamps", [](c10::optional<torch::Tensor> buf) {
    dfa::khead_set_stamps(has(buf) ? buf->data_ptr() : nullptr);
  }, "profiling aid: per-workgroup phase clocks of the khead launch into buf ([G][16] int64), None = off");
  m.def("khead_ws_floats", [](int64_t B, int64_t K) { return (int64_t)dfa::khead_ws_floats((int)B, (int)K); });
  m.def("khead_err_offset", [](int64_t B) { return (int64_t)dfa::khead_err_offset((int)B); });
  m.def("khead_supported", [](int64_t K, int64_t C) { return dfa::khead_supported((int)K, (int)C); });
  m.def("kcnn_fwd", &kcnn_fwd_py,"reference CNN conv block forward (conv1 + conv2 + pool [+ dropout], 1 launch)",
        py::arg("x"), py::arg("idx"), py::arg("scale"), py::arg("B"), py::arg("w1"), py::arg("b1"), py::arg("kpad1"),
        py::arg("w2"), py::arg("b2"), py::arg("pooled"), py::arg("code"), py::arg("drop_p") = 0.0,
        py::arg("drop_seed") = 0, py::arg("drop_step") = py::none(), py::arg("drop_step_add") = 0);
  m.def("kcnn_bwd", &kcnn_bwd_py, "reference CNN conv block backward (both weight gradients, 2 launches)",
        py::arg("x"), py::arg("idx"), py::arg("scale"), py::arg("B"), py::arg("w1"), py::arg("b1"), py::arg("kpad1"),
        py::arg("w2t"), py::arg("dyp"), py::arg("code"), py::arg("slabs"), py::arg("g_w1"), py::arg("g_b1"),
        py::arg("g_w2"), py::arg("g_b2"), py::arg("step_inc") = py::none());
  m.def("kcnn_slab_floats", [](int64_t B) { return (int64_t)dfa::kcnn_slab_floats((int)B); });
  m.def("lenet_train", &lenet_train_py, "whole-network LeNet-5 training step (fwd + CE + bwd, 2 launches)",
        py::arg("x"), py::arg("idx"), py::arg("scale"), py::arg("labels"), py::arg("conv"), py::arg("dense_w"),
        py::arg("dense_b"), py::arg("conv_grads"), py::arg("dense_gw"), py::arg("dense_gb"),
        py::arg("hT"), py::arg("dzT"), py::arg("conv_part"), py::arg("dense_part"), py::arg("loss_part"),
        py::arg("stats"), py::arg("frag"), py::arg("ftab"), py::arg("pxtab"), py::arg("B"), py::arg("grad_scale"),
        py::arg("prep") = true, py::arg("snap") = py::none(),
        py::arg("conv_mom") = std::vector<torch::Tensor>{}, py::arg("sgd_master") = py::none(),
        py::arg("sgd_mom") = py::none(), py::arg("sgd_wbf") = py::none(), py::arg("sgd_hyper") = py::none(),
        py::arg("sgd_descs") = py::none(), py::arg("idx_stream") = py::none(), py::arg("idx_cursor") = py::none(),
        py::arg("idx_dst") = py::none(), py::arg("ll") = nullptr, py::arg("exch_blocks") = 0, py::arg("run_stats") = py::none(),
        py::arg("ps") = nullptr, py::arg("ps_perm") = py::none(), py::arg("ps_idx") = py::none(),
        py::arg("ps_lr") = 0.0, py::arg("ps_max_stale") = -1, py::arg("red_succ") = true);
  m.def("lenet_blocks", [](int64_t B) { return dfa::lenet_blocks((int)B); });
  m.def("lenet_frag_bytes", []() { return (int64_t)dfa::lenet_frag_bytes(); });
  m.def("lenet_act_map", [](int64_t rows, int64_t ldt) {
    TORCH_CHECK(rows > 0 && ldt > 0 && ldt % 32 == 0 && rows * ldt < (1LL << 31), "lenet_act_map: bad shape");
    auto mp = torch::empty({rows, ldt}, torch::kLong);
    dfa::lenet_act_map((int)rows, (int)ldt, reinterpret_cast<long long*>(mp.data_ptr()));
    return mp;
  }, "element index of (row, batch column) in a transposed LeNet activation buffer of ldt columns (block layout)");
  m.def("lenet_dense_frag_map", [](int64_t l) {
    TORCH_CHECK(l >= 0 && l < 3, "lenet_dense_frag_map: layer 0 .. 2");
    int N = 0, K = 0;
    dfa::lenet_dense_frag_map((int)l, &N, &K, nullptr, nullptr);
    auto fwd = torch::empty({N, K}, torch::kLong), tr = torch::empty({K, N}, torch::kLong);
    dfa::lenet_dense_frag_map((int)l, &N, &K, reinterpret_cast<long long*>(fwd.data_ptr()),
                              reinterpret_cast<long long*>(tr.data_ptr()));
    return std::make_tuple(fwd, tr);
  }, "bf16 element index in the LeNet fragment buffer of every weight of dense layer l: (forward [N][K], transposed [K][N])");
  m.def("lenet_conv1_frag_map", []() {
    auto mp = torch::empty({150, 8}, torch::kInt);
    dfa::lenet_conv1_frag_map(reinterpret_cast<int*>(mp.data_ptr()));
    return mp;
  }, "bf16 element index in the LeNet fragment buffer of conv1 weight j = (c * 5 + ky) * 5 + kx at each of its 8 band positions: [150][8]");
  m.def("lenet_dense_part_floats", [](int64_t B) { return (int64_t)dfa::lenet_dense_part_floats((int)B); });
  m.def("lenet_red_err_offset", []() { return (int64_t)dfa::lenet_red_err_offset(); });
}

// the communicators' Python classes (bindings_comm.h)
void bind_comm(py::module_& m) {
  py::class_<P2PComm>(m, "P2PComm", "one-shot xGMI all-reduce over IPC-mapped peer buffers")
      .def(py::init<int64_t, int64_t, int64_t, double, int64_t>(), py::arg("rank"), py::arg("world"),
           py::arg("max_floats"), py::arg("timeout_s") = 2.0, py::arg("ll_slots") = 256)
      .def("handle", &P2PComm::handle)
      .def("open", &P2PComm::open)
      .def("allreduce", &P2PComm::allreduce, py::arg("t"), py::arg("scale") = 1.0)
      .def("error", &P2PComm::error)
      .def("host_error", &P2PComm::host_error)
      .def("ll_selftest", &P2PComm::ll_selftest, py::arg("inp"), py::arg("out"))
      .def("set_timeout", &P2PComm::set_timeout)
      .def_property_readonly("max_floats", &P2PComm::max_floats)
      .def_property_readonly("ll_slots", &P2PComm::ll_slots);
  py::class_<PSComm>(m, "PSComm", "device-resident bounded-staleness parameter server, master sharded over the ranks")
      .def(py::init<int64_t, int64_t, int64_t, int64_t, double, bool, bool>(), py::arg("rank"), py::arg("world"),
           py::arg("server_rank"), py::arg("n"), py::arg("timeout_s") = 30.0, py::arg("joiner") = false,
           py::arg("joinable") = false)
      .def("joiner", &PSComm::joiner)
      .def("handle", &PSComm::handle)
      .def("shard_handle", &PSComm::shard_handle)
      .def("open", &PSComm::open, py::arg("ctrl"), py::arg("shards"))
      .def("init_master", &PSComm::init_master)
      .def("selftest_add", &PSComm::selftest_add)
      .def("selftest_check", &PSComm::selftest_check)
      .def("set_lr_source", &PSComm::set_lr_source)
      .def_property_readonly("shard_len", &PSComm::shard_len)
      .def_property_readonly("nshards_used", &PSComm::nshards_used)
      .def("excl_step", &PSComm::excl_step, py::arg("max_stale"), py::arg("perm") = py::none(),
           py::arg("idx") = py::none())
      .def("excl_gate", &PSComm::excl_gate)
      .def("excl_mirror", &PSComm::excl_mirror)
      .def("fetch_pull", &PSComm::fetch_pull, py::arg("w"), py::arg("perm") = py::none(), py::arg("idx") = py::none(),
           py::arg("bid") = py::none())
      .def("export_state", &PSComm::export_state)
      .def("import_state", &PSComm::import_state, py::arg("state"))
      .def("inflight_bid", &PSComm::inflight_bid)
      .def("apply", &PSComm::apply, py::arg("g"), py::arg("lr"), py::arg("max_stale"))
      .def("stats", &PSComm::stats)
      .def("host_error", &PSComm::host_error)
      .def("set_schedule", &PSComm::set_schedule, py::arg("nbatches"), py::arg("max_epochs") = 0)
      .def("schedule_stats", &PSComm::schedule_stats)
      .def("done_epochs", &PSComm::done_epochs)
      .def("copy_master", &PSComm::copy_master)
      .def("stats_tensor", &PSComm::stats_tensor)
      .def("set_audit", &PSComm::set_audit, py::arg("rows"))
      .def("owner_init", &PSComm::owner_init, py::arg("ring"))
      .def("owner_open", &PSComm::owner_open, py::arg("handles"), py::arg("enable") = true, py::arg("ring") = 0)
      .def("owner_enable", &PSComm::owner_enable, py::arg("on"))
      .def("owner_applies", &PSComm::owner_applies)
      .def("owner_ring", &PSComm::owner_ring)
      .def("drain", &PSComm::drain, py::arg("w"), py::arg("quiesced") = false)
      .def("owner_prefix", &PSComm::owner_prefix)
      .def("calibrate", &PSComm::calibrate, py::arg("mode"), py::arg("reps") = 20)
      .def("fed_init", &PSComm::fed_init, py::arg("K"))
      .def("fed_open", &PSComm::fed_open, py::arg("handles"), py::arg("K") = 0)
      .def("fed_pull", &PSComm::fed_pull)
      .def("fed_upload", &PSComm::fed_upload, py::arg("g"), py::arg("drop_land") = false)
      .def("fed_apply", &PSComm::fed_apply, py::arg("lr"))
      .def("set_fed_audit", &PSComm::set_fed_audit, py::arg("rows"))
      .def("fed_stats", &PSComm::fed_stats)
      .def("fed_stats_tensor", &PSComm::fed_stats_tensor)
      .def("fed_seq_tensor", &PSComm::fed_seq_tensor);
}

}  // namespace dfa_py
