// The xGMI communicators of module distriflow_amd._C: P2PComm (one-shot all-reduce, LL exchange) and
// PSComm (device parameter server).  A header, since lenet_train (bindings_fused.cpp) takes both.
#pragma once
#include "bindings_util.h"

namespace dfa_py {

// Zeroed device memory that other processes map: uncached, so every rank's access sees the others'
// without L2 maintenance (fine-grained where the runtime has no uncached allocation).
inline char* alloc_uncached(size_t bytes, const char* what, const char* what_memset = nullptr) {
  void* p = nullptr;
  hipError_t e = hipExtMallocWithFlags(&p, bytes, hipDeviceMallocUncached);
  if (e != hipSuccess) {
    (void)hipGetLastError();
    check_hip(hipExtMallocWithFlags(&p, bytes, hipDeviceMallocFinegrained), what);
  }
  check_hip(hipMemset(p, 0, bytes), what_memset ? what_memset : what);
  return (char*)p;
}
inline py::bytes ipc_export(void* p) {
  hipIpcMemHandle_t h;
  check_hip(hipIpcGetMemHandle(&h, p), "hipIpcGetMemHandle");
  return py::bytes(reinterpret_cast<const char*>(&h), sizeof(h));
}
inline void* ipc_open(const std::string& handle, const char* bad_size) {
  TORCH_CHECK(handle.size() == sizeof(hipIpcMemHandle_t), bad_size);
  hipIpcMemHandle_t h;
  memcpy(&h, handle.data(), sizeof(h));
  void* p = nullptr;
  check_hip(hipIpcOpenMemHandle(&p, h, hipIpcMemLazyEnablePeerAccess), "hipIpcOpenMemHandle");
  return p;
}

// A word of host-mapped, coherent pinned memory that kernels write with system-scope stores: the
// host watchdog (parallel/watchdog.py) polls it with a plain load, so a peer timeout seen on the
// device is noticed even while the GPU is busy or hung and without queueing any HIP call.
class HostFlag {
 public:
  HostFlag() {
    check_hip(hipHostMalloc((void**)&host_, 64, hipHostMallocMapped | hipHostMallocCoherent), "host flag alloc");
    memset(host_, 0, 64);
    check_hip(hipHostGetDevicePointer((void**)&dev_, host_, 0), "host flag device pointer");
  }
  ~HostFlag() {
    if (host_) (void)hipHostFree(host_);
  }
  HostFlag(const HostFlag&) = delete;
  HostFlag& operator=(const HostFlag&) = delete;
  int* device() const { return dev_; }
  int64_t read() const { return *reinterpret_cast<volatile int*>(host_); }

 private:
  int* host_ = nullptr;
  int* dev_ = nullptr;
};

// One-shot xGMI all-reduce communicator (csrc/allreduce_p2p.hip): owns this rank's IPC-exported
// flag+staging buffer and the peer mappings.  Handles are exchanged by the Python side over the
// process group (parallel/p2p.py); every launch goes onto PyTorch's current stream (graph capturable).
class P2PComm {
 public:
  P2PComm(int64_t rank, int64_t world, int64_t max_floats, double timeout_s, int64_t ll_slots)
      : rank_((int)rank), world_((int)world) {
    TORCH_CHECK(world >= 1 && world <= dfa::kP2PMaxRanks, "p2p: world must be in [1, 8]");
    TORCH_CHECK(rank >= 0 && rank < world, "p2p: bad rank");
    TORCH_CHECK(max_floats > 0 && max_floats <= (int64_t(1) << 28), "p2p: max_floats out of range");
    TORCH_CHECK(ll_slots >= 0 && ll_slots <= 4096, "p2p: ll_slots out of range");
    check_hip(hipGetDevice(&dev_), "p2p getDevice");
    max_blocks_ = (int)((max_floats + dfa::kP2PChunk - 1) / dfa::kP2PChunk);
    half_ = (int64_t)max_blocks_ * dfa::kP2PChunk;
    flag_bytes_ = ((int64_t)max_blocks_ * dfa::kP2PMaxRanks * 4 + 4095) / 4096 * 4096;
    // in-kernel LL exchange region (csrc/ll_exchange.h) after the staging halves, in the same IPC export
    ll_slots_ = (int)ll_slots;
    ll_off_ = flag_bytes_ + 2 * half_ * 4;
    bytes_ = ll_off_ + 2 * (int64_t)ll_slots_ * dfa::kP2PMaxRanks * dfa::kLLSlot * 8;
    local_ = alloc_uncached((size_t)bytes_, "p2p alloc", "p2p memset");
    // per-block counters, then per-slot LL counters, then per-(slot, part) LL counters
    const size_t nep = (size_t)max_blocks_ + (size_t)ll_slots_ * (1 + dfa::kLLParts);
    check_hip(hipMalloc((void**)&epochs_, nep * 4), "p2p epochs alloc");
    check_hip(hipMemset(epochs_, 0, nep * 4), "p2p epochs memset");
    check_hip(hipMalloc((void**)&err_, 4), "p2p err alloc");
    check_hip(hipMemset(err_, 0, 4), "p2p err memset");
    check_hip(hipDeviceSynchronize(), "p2p init sync");
    timeout_ticks_ = (int64_t)(timeout_s * 1e8);  // wall_clock64 runs at 100 MHz
    for (auto& b : bases_) b = nullptr;
    bases_[rank_] = local_;
  }
  ~P2PComm() {
    for (int r = 0; r < world_; ++r)
      if (r != rank_ && bases_[r]) (void)hipIpcCloseMemHandle(bases_[r]);
    if (local_) (void)hipFree(local_);
    if (epochs_) (void)hipFree(epochs_);
    if (err_) (void)hipFree(err_);
  }
  py::bytes handle() const { return ipc_export(local_); }
  void open(const std::vector<std::string>& handles) {
    TORCH_CHECK((int)handles.size() == world_, "p2p: need one handle per rank");
    for (int r = 0; r < world_; ++r)
      if (r != rank_) bases_[r] = (char*)ipc_open(handles[r], "p2p: bad handle size");
    opened_ = true;
  }
  void allreduce(torch::Tensor t, double scale) {
    need(t, at::kFloat, "p2p tensor");
    TORCH_CHECK(opened_ || world_ == 1, "p2p: open() the peer handles first");
    TORCH_CHECK(t.get_device() == dev_, "p2p: tensor on the wrong device");
    TORCH_CHECK(t.numel() <= half_, "p2p: tensor larger than the staging buffer");
    TORCH_CHECK(reinterpret_cast<uintptr_t>(t.data_ptr()) % 16 == 0, "p2p: tensor must be 16-byte aligned");
    dfa::P2PArgs a{};
    for (int r = 0; r < dfa::kP2PMaxRanks; ++r) a.bases[r] = bases_[r];
    a.data = t.data_ptr<float>();
    a.n = t.numel();
    a.epochs = epochs_;
    a.err = err_;
    a.herr = herr_.device();
    a.flag_bytes = flag_bytes_;
    a.half_floats = half_;
    a.timeout_ticks = timeout_ticks_;
    a.rank = rank_;
    a.world = world_;
    a.max_blocks = max_blocks_;
    a.scale = (float)scale;
    check_hip(dfa::p2p_allreduce(a, cur_stream()), "p2p_allreduce");
  }
  int64_t error() const {
    int v = 0;
    check_hip(hipMemcpy(&v, err_, 4, hipMemcpyDeviceToHost), "p2p error readback");
    return v;
  }
  int64_t host_error() const { return herr_.read(); }  // no HIP call: safe from a watchdog thread
  // LL exchange self-test over the first in.numel() / kLLSlot slots (every rank the same call)
  void ll_selftest(torch::Tensor in, torch::Tensor out) {
    need(in, at::kFloat, "ll in");
    need(out, at::kFloat, "ll out");
    TORCH_CHECK(in.numel() == out.numel() && in.numel() % dfa::kLLSlot == 0, "ll: whole slots of kLLSlot floats");
    TORCH_CHECK(in.get_device() == dev_ && out.get_device() == dev_, "ll: tensors on the wrong device");
    const int ns = (int)(in.numel() / dfa::kLLSlot);
    TORCH_CHECK(ns >= 1 && ns <= ll_slots_, "ll: more slots than the communicator holds");
    check_hip(dfa::ll_selftest(ll_args(), in.data_ptr<float>(), out.data_ptr<float>(), ns, cur_stream()), "ll_selftest");
  }
  int64_t max_floats() const { return half_; }
  int64_t ll_slots() const { return ll_slots_; }
  void set_timeout(double timeout_s) { timeout_ticks_ = (int64_t)(timeout_s * 1e8); }
  // launch arguments of the in-kernel LL exchange (kernels that fold the all-reduce into their epilogue)
  dfa::LLComm ll_args() const {
    TORCH_CHECK(opened_ || world_ == 1, "p2p: open() the peer handles first");
    TORCH_CHECK(ll_slots_ > 0, "p2p: communicator built without LL slots");
    dfa::LLComm c{};
    for (int r = 0; r < dfa::kP2PMaxRanks; ++r)
      c.bases[r] = bases_[r] ? reinterpret_cast<unsigned long long*>(bases_[r] + ll_off_) : nullptr;
    c.epochs = epochs_ + max_blocks_;
    c.part_epochs = epochs_ + max_blocks_ + ll_slots_;
    c.err = err_;
    c.herr = herr_.device();
    c.timeout_ticks = timeout_ticks_;
    c.rank = rank_;
    c.world = world_;
    c.nslots = ll_slots_;
    return c;
  }

 private:
  int rank_, world_, dev_ = 0, max_blocks_ = 0, ll_slots_ = 0;
  int64_t half_ = 0, flag_bytes_ = 0, bytes_ = 0, timeout_ticks_ = 0, ll_off_ = 0;
  char* local_ = nullptr;
  char* bases_[dfa::kP2PMaxRanks];
  unsigned* epochs_ = nullptr;
  int* err_ = nullptr;
  HostFlag herr_;
  bool opened_ = false;
};

// Device-resident async parameter server (csrc/async_ps.hip, csrc/ps_device.h).  The server rank owns
// the control buffer (version word, FCFS cursor, completion arrays); EVERY rank owns one shard of the fp32
// master (a contiguous, power-of-two-sized parameter range) in its own HBM.  Both kinds of buffer are
// uncached, IPC exported and mapped into every rank, so the applies of different ranks land on
// different shards in parallel over xGMI.  Each shard carries a 64-word self-test area after its range.
class PSComm {
 public:
  static constexpr int kTestWords = 64;
  // joiner: a worker outside the process group that attaches to a running server (late join, SURVEY §5.3
  // elastic membership): `rank` is its id (>= world, used as its drain-lock id), it owns no shard, no inbox
  // and no FedSGD slots, maps every member's, and never writes alone (no exclusive-writer shortcuts)
  // joinable (members): workers may attach later -- the buffers are uncached even at one rank and the
  // exclusive-writer shortcuts are off
  PSComm(int64_t rank, int64_t world, int64_t server_rank, int64_t n, double timeout_s, bool joiner, bool joinable)
      : rank_((int)rank), world_((int)world), server_((int)server_rank), n_(n), joiner_(joiner),
        joinable_(joinable || joiner) {
    TORCH_CHECK(n > 0 && n % 4 == 0, "ps: n must be a positive multiple of 4");
    TORCH_CHECK(world >= 1 && world <= dfa::kP2PMaxRanks, "ps: 1..8 ranks");
    TORCH_CHECK(server_rank >= 0 && server_rank < world, "ps: bad server rank");
    TORCH_CHECK(joiner ? (rank >= world && rank < 1024) : (rank >= 0 && rank < world), "ps: bad rank");
    check_hip(hipGetDevice(&dev_), "ps getDevice");
    // shard length: the smallest power of two >= 64 with world shards covering n
    shift_ = 6;
    while (((n_ - 1) >> shift_) >= world_) ++shift_;
    if (rank_ == server_) ctrl_ = (dfa::PSCtrl*)alloc_shared(dfa::ps_ctrl_bytes(), "ps control");
    if (!joiner_) own_ = (float*)alloc_shared(((size_t)1 << shift_) * 4 + kTestWords * 4, "ps shard");
    check_hip(hipMalloc((void**)&loc_, sizeof(dfa::PSLocal)), "ps local alloc");
    check_hip(hipMemset(loc_, 0, sizeof(dfa::PSLocal)), "ps local memset");
    // kPSVMin (csrc/ps_device.h): no refresh recorded yet
    check_hip(hipMemset(&loc_->scratch[dfa::kPSVMinWord], 0xff, 4), "ps vmin init");
    check_hip(hipDeviceSynchronize(), "ps init sync");
    timeout_ticks_ = (int64_t)(timeout_s * 1e8);
    for (auto& p : shard_) p = nullptr;
  }
  ~PSComm() {
    for (int k = 0; k < world_; ++k)
      if (inbox_[k] && k != rank_) (void)hipIpcCloseMemHandle(inbox_[k]);
    if (inbox_own_) (void)hipFree(inbox_own_);
    for (int k = 0; k < world_; ++k)
      if (fed_slot_[k] && k != rank_) (void)hipIpcCloseMemHandle(fed_slot_[k]);
    if (fed_own_) (void)hipFree(fed_own_);
    if (ctrl_ && rank_ != server_) (void)hipIpcCloseMemHandle(ctrl_);
    if (ctrl_ && rank_ == server_) (void)hipFree(ctrl_);
    for (int k = 0; k < world_; ++k)
      if (shard_[k] && k != rank_) (void)hipIpcCloseMemHandle(shard_[k]);
    if (own_) (void)hipFree(own_);
    if (loc_) (void)hipFree(loc_);
  }
  py::bytes handle() const {
    TORCH_CHECK(rank_ == server_, "ps: only the server rank exports the control buffer");
    return ipc_export(ctrl_);
  }
  py::bytes shard_handle() const {
    TORCH_CHECK(!joiner_, "ps: a joiner owns no shard");
    return ipc_export(own_);
  }
  bool joiner() const { return joiner_; }
  // ctrl: the server's control-buffer handle; shards[k]: rank k's shard handle (every rank's, own included)
  void open(const std::string& ctrl, std::vector<std::string> shards) {
    TORCH_CHECK((int)shards.size() == world_, "ps: one shard handle per rank");
    if (rank_ != server_) ctrl_ = (dfa::PSCtrl*)open_handle(ctrl);
    for (int k = 0; k < world_; ++k) shard_[k] = k == rank_ ? own_ : (float*)open_handle(shards[k]);
    std::vector<float*> tab(dfa::kP2PMaxRanks, nullptr);
    for (int k = 0; k < world_; ++k) tab[k] = shard_[k] + ((size_t)1 << shift_);  // self-test areas
    check_hip(hipMemcpy(loc_->selftest_tab, tab.data(), tab.size() * sizeof(float*), hipMemcpyHostToDevice), "ps tab");
  }
  int64_t shard_len() const { return (int64_t)1 << shift_; }
  int64_t nshards_used() const { return (n_ - 1) / shard_len() + 1; }
  // every rank: seed its own shard's range of the master (the ranks hold identical initial weights)
  void init_master(torch::Tensor w) {
    TORCH_CHECK(!joiner_, "ps: a joiner seeds no shard (it pulls the current master)");
    need(w, at::kFloat, "ps master");
    TORCH_CHECK(w.numel() == n_, "ps: master size mismatch");
    const int64_t lo = (int64_t)rank_ * shard_len(), hi = std::min<int64_t>(n_, lo + shard_len());
    if (hi > lo)
      check_hip(hipMemcpy(own_, w.data_ptr<float>() + lo, (size_t)(hi - lo) * 4, hipMemcpyDeviceToDevice), "ps init");
    check_hip(hipDeviceSynchronize(), "ps init sync");
  }
  // self-test of the element add on every shard (call on every rank between two barriers): every rank
  // adds (rank + 1) * (j + 1) to word j of every shard's test area
  void selftest_add() {
    TORCH_CHECK(!joiner_, "ps: the shard self-test runs among the members");
    dfa::PSArgs a = args();
    check_hip(dfa::ps_selftest_add(a, loc_->selftest_tab, kTestWords, (float)(rank_ + 1), cur_stream()), "ps selftest");
    check_hip(hipStreamSynchronize(cur_stream()), "ps selftest sync");
  }
  // after every rank's selftest_add: each test word must hold (j + 1) * W (W + 1) / 2 exactly
  bool selftest_check() const {
    std::vector<float> v(kTestWords);
    for (int k = 0; k < world_; ++k) {
      check_hip(hipMemcpy(v.data(), shard_[k] + shard_len(), kTestWords * 4, hipMemcpyDeviceToHost), "ps selftest rd");
      for (int j = 0; j < kTestWords; ++j)
        if (v[j] != (float)((j + 1) * world_ * (world_ + 1) / 2)) return false;
    }
    return true;
  }
  int64_t host_error() const { return herr_.read(); }  // no HIP call: safe from a watchdog thread
  // Epoch-scoped at-least-once dispatch over `nbatches` microbatch ids, `max_epochs` dataset epochs
  // (0 = unbounded).  Called with the same values on every rank before the first step.
  void set_schedule(int64_t nbatches, int64_t max_epochs) {
    TORCH_CHECK(nbatches > 0 && nbatches <= dfa::kPSMaxBatches, "ps: nbatches out of range");
    TORCH_CHECK(max_epochs >= 0, "ps: max_epochs must be >= 0");
    nbatches_ = nbatches;
    max_epochs_ = (int)max_epochs;
  }
  // the device learning rate the applies read (the trainer's hyper tensor; set_lr after capture holds)
  void set_lr_source(torch::Tensor hyper) {
    need(hyper, at::kFloat, "ps lr source");
    TORCH_CHECK(hyper.numel() >= 1 && hyper.get_device() == dev_, "ps: lr source on this device");
    lr_dev_ = hyper.data_ptr<float>();
    lr_keep_ = hyper;
  }
  // [epoch, completed in epoch, completed, redispatched, skipped, duplicates, finished]
  std::vector<int64_t> schedule_stats() const {
    unsigned e[2] = {0, 0};
    unsigned long long c[4] = {0, 0, 0, 0};
    peek(e, ctrl_->sched, "ps sched");
    peek(c, ctrl_->sched_ctr, "ps sched ctr");
    const bool fin = max_epochs_ > 0 && (int64_t)e[0] >= max_epochs_;
    return {(int64_t)e[0], (int64_t)e[1], (int64_t)c[0], (int64_t)c[1], (int64_t)c[2], (int64_t)c[3], fin ? 1 : 0};
  }
  // done_epoch[0:nbatches]: e + 1 of the last epoch in which each batch was applied
  std::vector<int64_t> done_epochs() const {
    std::vector<unsigned> v((size_t)nbatches_);
    if (nbatches_ > 0)
      check_hip(hipMemcpy(v.data(), ctrl_->done_epoch, (size_t)nbatches_ * 4, hipMemcpyDeviceToHost), "ps done");
    return std::vector<int64_t>(v.begin(), v.end());
  }
  // bid: take this microbatch id (epoch << 32 | batch: a checkpoint's in-flight claim) instead of claiming
  void fetch_pull(torch::Tensor w, c10::optional<torch::Tensor> perm, c10::optional<torch::Tensor> idx,
                  c10::optional<int64_t> bid = c10::nullopt) {
    dfa::PSArgs a = args();
    if (bid.has_value()) {
      TORCH_CHECK(has(perm), "ps: a given microbatch id needs the perm table");
      TORCH_CHECK(*bid >= 0 && (*bid & 0xffffffffLL) < perm->size(0), "ps: microbatch id out of range");
      a.claim_given = 1;
      a.claim_bid = *bid;
    }
    need(w, at::kFloat, "ps local master");
    TORCH_CHECK(w.numel() == n_ && w.get_device() == dev_, "ps: local master mismatch");
    a.w = w.data_ptr<float>();
    if (has(perm)) bind_schedule_table(a, *perm, idx);
    check_hip(dfa::ps_fetch_pull(a, cur_stream()), "ps_fetch_pull");
  }
  // exclusive writer (world 1): admission + next claim / index staging, one workgroup; the update is the
  // optimizer launch gated on excl_gate() that mirrors the new weights into excl_mirror() (ps_excl_step)
  void excl_step(int64_t max_stale, c10::optional<torch::Tensor> perm, c10::optional<torch::Tensor> idx) {
    TORCH_CHECK(world_ == 1 && !owner_on_, "ps: the exclusive-writer step needs one rank (CAS path)");
    dfa::PSArgs a = args();
    a.max_stale = (int)max_stale;
    if (has(perm)) bind_schedule_table(a, *perm, idx);
    check_hip(dfa::ps_excl_step(a, cur_stream()), "ps_excl_step");
  }
  uintptr_t excl_gate() const {
    TORCH_CHECK(world_ == 1, "ps: one rank");
    return reinterpret_cast<uintptr_t>(&loc_->scratch[dfa::kPSDecisionWord]);
  }
  uintptr_t excl_mirror() const {
    TORCH_CHECK(world_ == 1 && shard_[0] != nullptr, "ps: one rank, opened");
    return reinterpret_cast<uintptr_t>(shard_[0]);
  }
  void apply(torch::Tensor g, double lr, int64_t max_stale) {
    dfa::PSArgs a = args();
    need(g, at::kFloat, "ps grad");
    TORCH_CHECK(g.numel() == n_ && g.get_device() == dev_, "ps: gradient mismatch");
    a.g = g.data_ptr<float>();
    a.lr = (float)lr;
    a.max_stale = (int)max_stale;
    check_hip(dfa::ps_apply(a, cur_stream()), "ps_apply");
  }
  // device view of this rank's counters [accepted, rejected, sum staleness, max staleness, admission CAS
  // retries, err, no-op steps, -] (int64): read back asynchronously by the trainer's callbacks
  // audit rows (version at admission, vp, decision) of this rank's next `rows` decisions, written by the
  // admission itself (tests: the true staleness of every admitted gradient); an empty tensor disables it
  void set_audit(torch::Tensor rows) { audit_.set(rows, dev_, "ps audit", "ps: audit rows [n][3] int32"); }
  torch::Tensor stats_tensor() const { return device_view(loc_->stats, 8, torch::kLong); }
  // ---- device FedSGD count barrier (csrc/fedsgd_ps.hip) on the same shards: K gradient slots per shard
  // (every rank; call fed_init on every rank, exchange the handles, then fed_open)
  py::bytes fed_init(int64_t K) {
    TORCH_CHECK(K >= 1 && K <= dfa::kFedMaxK, "fedsgd: K must be 1..", dfa::kFedMaxK);
    TORCH_CHECK(fed_own_ == nullptr, "fedsgd: already initialised");
    fed_K_ = (int)K;
    fed_own_ = (float*)alloc_shared((size_t)K * ((size_t)1 << shift_) * 4, "fedsgd slots");
    for (auto& p : fed_slot_) p = nullptr;
    clear_fed_local();
    check_hip(hipDeviceSynchronize(), "fedsgd init sync");
    return ipc_export(fed_own_);
  }
  void fed_open(std::vector<std::string> handles, int64_t K) {
    TORCH_CHECK((joiner_ || fed_own_ != nullptr) && (int)handles.size() == world_,
                "fedsgd: fed_init first (members), one handle per rank");
    if (joiner_) {
      TORCH_CHECK(K >= 1 && K <= dfa::kFedMaxK, "fedsgd: K must be 1..", dfa::kFedMaxK);
      fed_K_ = (int)K;
      clear_fed_local();
    }
    for (int k = 0; k < world_; ++k) fed_slot_[k] = k == rank_ ? fed_own_ : (float*)open_handle(handles[k]);
  }
  dfa::FedArgs fed_args() const {
    TORCH_CHECK((joiner_ || fed_own_ != nullptr) && fed_slot_[0] != nullptr, "fedsgd: fed_open first");
    dfa::FedArgs a{};
    a.seq = &ctrl_->fed_seq;
    a.tick = &ctrl_->fed_tick;
    a.land = &ctrl_->fed_land;
    a.bad = &ctrl_->fed_bad;
    for (int k = 0; k < world_; ++k) a.shard[k] = shard_[k], a.slot[k] = fed_slot_[k];
    a.shard_shift = shift_;
    a.nshards = world_;
    a.K = fed_K_;
    a.n = n_;
    a.scratch = loc_->fed_scratch;
    a.stats = loc_->fed_stats;
    a.audit = fed_audit_.rows;
    a.audit_cap = fed_audit_.cap;
    a.lr_dev = lr_dev_;
    a.timeout_ticks = timeout_ticks_;
    a.herr = reinterpret_cast<unsigned*>(herr_.device());
    return a;
  }
  void fed_pull(torch::Tensor w) {
    need(w, at::kFloat, "fedsgd local master");
    TORCH_CHECK(w.numel() == n_ && w.get_device() == dev_, "fedsgd: local master mismatch");
    dfa::FedArgs a = fed_args();
    a.w = w.data_ptr<float>();
    check_hip(dfa::fed_pull(a, cur_stream()), "fed_pull");
  }
  // drop_land: fault injection (tests) -- the ticket is taken, nothing is stored or landed (a rank that dies
  // between its admission and its landing)
  void fed_upload(torch::Tensor g, bool drop_land) {
    need(g, at::kFloat, "fedsgd grad");
    TORCH_CHECK(g.numel() == n_ && g.get_device() == dev_, "fedsgd: gradient mismatch");
    dfa::FedArgs a = fed_args();
    a.g = g.data_ptr<float>();
    a.drop_land = drop_land ? 1 : 0;
    check_hip(dfa::fed_upload(a, cur_stream()), "fed_upload");
  }
  void fed_apply(double lr) {
    dfa::FedArgs a = fed_args();
    a.lr = (float)lr;
    check_hip(dfa::fed_apply(a, cur_stream()), "fed_apply");
  }
  void set_fed_audit(torch::Tensor rows) {
    fed_audit_.set(rows, dev_, "fedsgd audit", "fedsgd: audit rows [n][3] int32");
  }
  // [admitted, stale, full, failed, versions applied by this rank, error bits, version seqlock word,
  //  stuck versions this rank recovered]
  std::vector<int64_t> fed_stats() const {
    unsigned long long h[8] = {0};
    peek(h, loc_->fed_stats, "fedsgd stats");
    unsigned seq = 0;
    peek(seq, ctrl_->fed_seq, "fedsgd seq");
    return {(int64_t)h[0], (int64_t)h[1], (int64_t)h[2], (int64_t)h[3], (int64_t)h[4], (int64_t)h[7], (int64_t)seq,
            (int64_t)h[5]};
  }
  // device view of [admitted, stale, full, failed, applied-by-me, -, -, err] (trainer callbacks)
  torch::Tensor fed_stats_tensor() const {
    return device_view(loc_->fed_stats, 8, torch::kLong);
  }
  // device view of the version seqlock word (int32; version = word / 2)
  torch::Tensor fed_seq_tensor() const {
    return device_view(&ctrl_->fed_seq, 1, torch::kInt);
  }

  // ---- owner-applies (csrc/async_ps.hip): an inbox of `ring` slots of this rank's shard length (+ ring
  // flags) on every rank; call owner_init on every rank, exchange the handles, then owner_open
  py::bytes owner_init(int64_t ring) {
    TORCH_CHECK(ring >= 2 && ring <= 255, "ps owner-applies: ring must be 2..255");
    TORCH_CHECK(inbox_own_ == nullptr, "ps owner-applies: already initialised");
    owner_ring_ = (int)ring;
    inbox_own_ = (float*)alloc_shared((size_t)ring * ((size_t)1 << shift_) * 4 + (size_t)ring * 4 + 256,
                                        "ps owner inbox");
    return ipc_export(inbox_own_);
  }
  // enable = false: map the inboxes only (the apply-path calibration), owner_enable() switches the path
  void owner_open(std::vector<std::string> handles, bool enable, int64_t ring) {
    TORCH_CHECK((joiner_ || inbox_own_ != nullptr) && (int)handles.size() == world_, "ps owner-applies: owner_init first");
    if (joiner_) {
      TORCH_CHECK(ring >= 2 && ring <= 255, "ps owner-applies: a joiner passes the members' ring length");
      owner_ring_ = (int)ring;
    }
    for (int k = 0; k < world_; ++k) inbox_[k] = k == rank_ ? inbox_own_ : (float*)open_handle(handles[k]);
    owner_on_ = enable;
  }
  void owner_enable(bool on) {
    TORCH_CHECK(!on || inbox_[0] != nullptr, "ps owner-applies: owner_open first");
    owner_on_ = on;
  }
  bool owner_applies() const { return owner_on_; }
  int64_t owner_ring() const { return owner_ring_; }
  // apply-path calibration (collective: every rank calls it at once, between barriers, before init_master):
  // mean microseconds per launch of the CAS adds (mode 0) or the owner-applies traffic (mode 1, needs
  // owner_init / owner_open) over this rank's n elements, `reps` launches after one warm-up launch
  double calibrate(int64_t mode, int64_t reps) {
    dfa::PSArgs a = args();
    TORCH_CHECK(mode == 0 || mode == 1, "ps calibrate: mode 0 (CAS) or 1 (owner-applies)");
    TORCH_CHECK(reps >= 1, "ps calibrate: reps >= 1");
    if (mode == 1) {
      TORCH_CHECK(inbox_[0] != nullptr, "ps calibrate: owner_open first");
      set_owner(a);
    }
    hipStream_t st = cur_stream();
    check_hip(dfa::ps_calibrate(a, (int)mode, st), "ps_calibrate");
    hipEvent_t e0, e1;
    check_hip(hipEventCreate(&e0), "calib event");
    check_hip(hipEventCreate(&e1), "calib event");
    check_hip(hipEventRecord(e0, st), "calib record");
    for (int64_t r = 0; r < reps; ++r) check_hip(dfa::ps_calibrate(a, (int)mode, st), "ps_calibrate");
    check_hip(hipEventRecord(e1, st), "calib record");
    check_hip(hipEventSynchronize(e1), "calib sync");
    float ms = 0.f;
    check_hip(hipEventElapsedTime(&ms, e0, e1), "calib elapsed");
    (void)hipEventDestroy(e0);
    (void)hipEventDestroy(e1);
    return (double)ms * 1e3 / (double)reps;
  }
  // the owner's drain alone (a pull into `w` without a microbatch claim): adds every flagged slot of this
  // rank's inbox into its shard; after the last step of every rank, one drain per rank settles the master
  // quiesced (a checkpoint, nobody stepping): the drain claims no microbatch (the cursor, claimed_epoch and this
  // rank's claimed id stay) and the refresh record kPSVMin is put back, so the next step decides as without it
  void drain(torch::Tensor w, bool quiesced = false) {
    if (!quiesced) {
      fetch_pull(w, c10::nullopt, c10::nullopt, c10::nullopt);
      return;
    }
    dfa::PSArgs a = args();
    need(w, at::kFloat, "ps local master");
    TORCH_CHECK(w.numel() == n_ && w.get_device() == dev_, "ps: local master mismatch");
    a.w = w.data_ptr<float>();
    a.claim_given = 2;
    unsigned vmin = 0;
    check_hip(hipStreamSynchronize(cur_stream()), "ps drain sync");
    peek(vmin, loc_->scratch[dfa::kPSVMinWord], "ps vmin rd");
    check_hip(dfa::ps_fetch_pull(a, cur_stream()), "ps_fetch_pull");
    check_hip(hipStreamSynchronize(cur_stream()), "ps drain sync");
    poke(loc_->scratch[dfa::kPSVMinWord], vmin, "ps vmin wr");
  }
  // [drained sequence count of every owner]
  std::vector<int64_t> owner_prefix() const {
    std::vector<unsigned> v(world_, 0);
    check_hip(hipMemcpy(v.data(), ctrl_->pref, (size_t)world_ * 4, hipMemcpyDeviceToHost), "ps pref");
    return std::vector<int64_t>(v.begin(), v.end());
  }

  // launch arguments of the fused LeNet-5 reduce in parameter-server mode (lenet_train_py)
  dfa::PSArgs lenet_args(const torch::Tensor& perm, const torch::Tensor& idx, double lr, int64_t max_stale) const {
    dfa::PSArgs a = args();
    bind_schedule_table(a, perm, idx, "ps: perm [nbatches][B]");
    a.lr = (float)lr;
    a.max_stale = (int)max_stale;
    return a;
  }
  // [accepted, rejected, sum staleness, max staleness, admission CAS retries, err, version, batch cursor,
  //  no-op steps, fully applied]
  std::vector<int64_t> stats() const {
    unsigned long long h[8] = {0};
    peek(h, loc_->stats, "ps stats");
    unsigned ver = 0, applied = 0;
    unsigned long long ctr = 0;
    peek(ver, ctrl_->ver, "ps ver");
    peek(applied, ctrl_->applied, "ps ver");
    peek(ctr, ctrl_->batch_ctr, "ps ctr");
    return {(int64_t)h[0], (int64_t)h[1], (int64_t)h[2], (int64_t)h[3], (int64_t)h[4], (int64_t)h[5],
            (int64_t)ver, (int64_t)ctr, (int64_t)h[6], (int64_t)applied};
  }
  // ---- checkpoint / resume of the control state (the caller guarantees that nobody is stepping)
  // this rank's claimed microbatch (epoch << 32 | batch; negative: the schedule is finished)
  int64_t inflight_bid() const {
    long long b = 0;
    check_hip(hipDeviceSynchronize(), "ps inflight sync");
    peek(b, loc_->bid_out, "ps bid");
    return (int64_t)b;
  }
  py::dict export_state() const {
    TORCH_CHECK(ctrl_ != nullptr, "ps: open() the handles first");
    TORCH_CHECK(nbatches_ > 0, "ps export_state: set_schedule first");
    check_hip(hipDeviceSynchronize(), "ps export sync");
    unsigned ver = 0, applied32 = 0, sch[2] = {0, 0};
    unsigned long long cursor = 0, ctr[4] = {0, 0, 0, 0};
    peek(ver, ctrl_->ver, "ps export ver");
    peek(applied32, ctrl_->applied, "ps export ver");
    peek(cursor, ctrl_->batch_ctr, "ps export cursor");
    peek(sch, ctrl_->sched, "ps export sched");
    peek(ctr, ctrl_->sched_ctr, "ps export ctr");
    std::vector<unsigned> done((size_t)nbatches_), claimed((size_t)nbatches_);
    check_hip(hipMemcpy(done.data(), ctrl_->done_epoch, (size_t)nbatches_ * 4, hipMemcpyDeviceToHost), "ps export done");
    check_hip(hipMemcpy(claimed.data(), ctrl_->claimed_epoch, (size_t)nbatches_ * 4, hipMemcpyDeviceToHost),
              "ps export claimed");
    py::dict d;
    std::vector<int64_t> pref;
    int64_t applied = (int64_t)applied32;
    // owner-applies: the owners' drains publish (pref), the applied word is never written; "fully applied" is
    // the minimum prefix.  (Inboxes that are mapped for the calibration only carry no prefixes.)
    if (owner_on_) {
      pref = owner_prefix();
      applied = *std::min_element(pref.begin(), pref.end());
    }
    d["version"] = (int64_t)ver;
    d["applied"] = applied;
    d["cursor"] = (int64_t)cursor;
    d["epoch"] = (int64_t)sch[0];
    d["completed_in_epoch"] = (int64_t)sch[1];
    d["sched_ctr"] = std::vector<int64_t>{(int64_t)ctr[0], (int64_t)ctr[1], (int64_t)ctr[2], (int64_t)ctr[3]};
    d["done_epoch"] = std::vector<int64_t>(done.begin(), done.end());
    d["claimed_epoch"] = std::vector<int64_t>(claimed.begin(), claimed.end());
    d["owner_prefix"] = pref;
    return d;
  }
  // server rank, after open() / init_master() and before the first step: write a quiesced job's words back
  void import_state(py::dict st) {
    TORCH_CHECK(rank_ == server_ && !joiner_, "ps import_state: the server rank writes the control buffer");
    TORCH_CHECK(ctrl_ != nullptr && shard_[0] != nullptr, "ps: open() the handles first");
    TORCH_CHECK(nbatches_ > 0, "ps import_state: set_schedule first");
    const int64_t version = st["version"].cast<int64_t>(), applied = st["applied"].cast<int64_t>();
    const int64_t cursor = st["cursor"].cast<int64_t>(), epoch = st["epoch"].cast<int64_t>();
    const int64_t in_epoch = st["completed_in_epoch"].cast<int64_t>();
    const auto ctr = st["sched_ctr"].cast<std::vector<int64_t>>();
    const auto done = st["done_epoch"].cast<std::vector<int64_t>>();
    const auto claimed = st["claimed_epoch"].cast<std::vector<int64_t>>();
    std::vector<int64_t> pref;
    if (st.contains("owner_prefix") && !st["owner_prefix"].is_none()) pref = st["owner_prefix"].cast<std::vector<int64_t>>();
    TORCH_CHECK(version >= 0 && version <= 0xffffffffLL && cursor >= 0 && epoch >= 0 && epoch < 0xffffffffLL,
                "ps import_state: word out of range");
    TORCH_CHECK(version == applied, "ps import_state: version ", version, " != applied ", applied,
                " (the job was not quiesced)");
    for (int64_t p : pref)
      TORCH_CHECK(p == version, "ps import_state: an owner prefix (", p, ") differs from the version ", version);
    TORCH_CHECK((int64_t)done.size() == nbatches_ && (int64_t)claimed.size() == nbatches_,
                "ps import_state: completion arrays of ", done.size(), " / ", claimed.size(), " entries, schedule has ",
                nbatches_);
    TORCH_CHECK(ctr.size() == 4, "ps import_state: four schedule counters");
    int64_t cnt = 0;
    for (int64_t v : done) {
      TORCH_CHECK(v >= 0 && v <= 0xffffffffLL, "ps import_state: done_epoch out of range");
      cnt += v == epoch + 1 ? 1 : 0;
    }
    TORCH_CHECK(cnt == in_epoch, "ps import_state: completed_in_epoch ", in_epoch, " but ", cnt,
                " batches are done in epoch ", epoch);
    for (int64_t v : claimed) TORCH_CHECK(v >= 0 && v <= 0xffffffffLL, "ps import_state: claimed_epoch out of range");
    check_hip(hipDeviceSynchronize(), "ps import sync");
    const unsigned long long cur = (unsigned long long)cursor;
    const unsigned sch[2] = {(unsigned)epoch, (unsigned)in_epoch};
    const unsigned long long c4[4] = {(unsigned long long)ctr[0], (unsigned long long)ctr[1], (unsigned long long)ctr[2],
                                      (unsigned long long)ctr[3]};
    std::vector<unsigned> d32(done.begin(), done.end()), c32(claimed.begin(), claimed.end());
    poke(ctrl_->ver, (unsigned)version, "ps import ver");
    poke(ctrl_->applied, (unsigned)applied, "ps import ver");
    poke(ctrl_->batch_ctr, cur, "ps import cursor");
    poke(ctrl_->sched, sch, "ps import sched");
    poke(ctrl_->sched_ctr, c4, "ps import ctr");
    check_hip(hipMemcpy(ctrl_->done_epoch, d32.data(), d32.size() * 4, hipMemcpyHostToDevice), "ps import done");
    check_hip(hipMemcpy(ctrl_->claimed_epoch, c32.data(), c32.size() * 4, hipMemcpyHostToDevice), "ps import claimed");
    // (the fed_* words stay as they are)
    if (inbox_[0] != nullptr) {
      // Every owner's drained prefix = version.  Sequence numbers are the version word's values (ps_admit:
      // kPSSeq = v), so the next admitted gradient has q = version; the drain loop of ps_fetch_pull_kernel
      // starts at P = pref[k] and takes slot (P + n) % R only while its flag == P + n + 1 (>= 1).  A fresh
      // server's ring flags are all zero, so nothing is drained until a sender has flagged q + 1 for
      // q >= version: a resumed server with pref[k] = version is consistent with an empty ring.
      std::vector<unsigned> p32((size_t)world_, (unsigned)version);
      check_hip(hipMemcpy(ctrl_->pref, p32.data(), p32.size() * 4, hipMemcpyHostToDevice), "ps import pref");
    }
    check_hip(hipDeviceSynchronize(), "ps import sync");
  }
  // the master, gathered from the shards (call while no worker is stepping)
  void copy_master(torch::Tensor dst) const {
    need(dst, at::kFloat, "ps dst");
    TORCH_CHECK(dst.numel() == n_, "ps: dst size mismatch");
    check_hip(hipDeviceSynchronize(), "ps copy_master sync");
    for (int64_t k = 0; k < nshards_used(); ++k) {
      const int64_t lo = k * shard_len(), hi = std::min<int64_t>(n_, lo + shard_len());
      check_hip(hipMemcpyAsync(dst.data_ptr<float>() + lo, shard_[k], (size_t)(hi - lo) * 4, hipMemcpyDeviceToDevice,
                               cur_stream()),
                "ps copy_master");
    }
  }

 private:
  // Memory other processes map (world > 1): uncached.  One rank alone shares it with nobody: plain (cached)
  // device memory, whose accesses do not pay the uncached operation rate (~6 k per us chip-wide, profiles/r5/ps_cas_adds_per_us_1gpu.jsonl);
  // IPC export works on either.
  char* alloc_shared(size_t bytes, const char* what) const {
    if (world_ > 1 || joinable_) return alloc_uncached(bytes, what);
    void* p = nullptr;
    check_hip(hipMalloc(&p, bytes), what);
    check_hip(hipMemset(p, 0, bytes), what);
    return (char*)p;
  }
  static void* open_handle(const std::string& handle) { return ipc_open(handle, "ps: bad handle size"); }
  // audit rows [n][3] int32 that an admission fills (kept alive here); an empty tensor disables them
  struct Audit {
    unsigned* rows = nullptr;
    int64_t cap = 0;
    torch::Tensor keep;
    void set(torch::Tensor t, int dev, const char* name, const char* shape_msg) {
      if (!t.defined() || t.numel() == 0) {
        rows = nullptr, cap = 0, keep = torch::Tensor();
        return;
      }
      need(t, at::kInt, name);
      TORCH_CHECK(t.dim() == 2 && t.size(1) == 3 && t.get_device() == dev, shape_msg);
      rows = reinterpret_cast<unsigned*>(t.data_ptr<int>());
      cap = t.size(0);
      keep = t;
    }
  };
  // host <-> device copy of one field of ctrl_ / loc_ (an array field: the whole array)
  template <typename T>
  static void peek(T& host, const T& dev, const char* what) {
    check_hip(hipMemcpy(&host, &dev, sizeof(T), hipMemcpyDeviceToHost), what);
  }
  template <typename T>
  static void poke(T& dev, const T& host, const char* what) {
    check_hip(hipMemcpy(&dev, &host, sizeof(T), hipMemcpyHostToDevice), what);
  }
  torch::Tensor device_view(void* p, int64_t n, at::ScalarType dt) const {
    return torch::from_blob(p, {n}, torch::TensorOptions().dtype(dt).device(torch::kCUDA, dev_));
  }
  void clear_fed_local() {  // fed_scratch and everything after it
    check_hip(hipMemset(loc_->fed_scratch, 0, sizeof(dfa::PSLocal) - offsetof(dfa::PSLocal, fed_scratch)), "fedsgd local");
  }
  // the microbatch table [nbatches][B] and the index buffer a claim stages into (shape_msg: one combined check)
  void bind_schedule_table(dfa::PSArgs& a, const torch::Tensor& perm, const c10::optional<torch::Tensor>& idx,
                           const char* shape_msg = nullptr) const {
    need(perm, at::kLong, "ps perm");
    TORCH_CHECK(has(idx), "ps: idx required with perm");
    need(*idx, at::kLong, "ps idx");
    const bool shape = perm.dim() == 2 && perm.size(1) == idx->numel(), even = idx->numel() % 2 == 0;
    TORCH_CHECK(shape_msg == nullptr || (shape && even), shape_msg);
    TORCH_CHECK(shape, "ps: perm must be [nbatches][B]");
    TORCH_CHECK(even, "ps: batch size must be even");
    TORCH_CHECK(nbatches_ == 0 || perm.size(0) == nbatches_, "ps: perm rows != scheduled nbatches");
    a.perm = reinterpret_cast<const long long*>(perm.data_ptr());
    a.idx = reinterpret_cast<long long*>(idx->data_ptr());
    a.nbatches = perm.size(0);
    a.B = (int)idx->numel();
  }
  void set_owner(dfa::PSArgs& a) const {  // owner-applies: the ring, the drain words and every inbox
    a.owner_ring = owner_ring_;
    a.pref = ctrl_->pref;
    a.dlock = ctrl_->dlock;
    for (int k = 0; k < world_; ++k) a.inbox[k] = inbox_[k];
  }
  dfa::PSArgs args() const {
    TORCH_CHECK(ctrl_ != nullptr && shard_[0] != nullptr, "ps: open() the handles first");
    dfa::PSArgs a{};
    a.ver = &ctrl_->ver;
    a.batch_ctr = &ctrl_->batch_ctr;
    for (int k = 0; k < world_; ++k) a.shard[k] = shard_[k];
    a.shard_shift = shift_;
    a.nshards = world_;
    a.excl = (world_ == 1 && !joinable_) ? 1 : 0;
    a.n = n_;
    a.vpulled = &loc_->vpulled;
    a.applied = &ctrl_->applied;
    a.audit = audit_.rows;
    a.audit_cap = audit_.cap;
    a.bid_out = &loc_->bid_out;
    a.stats = loc_->stats;
    a.scratch = loc_->scratch;
    a.timeout_ticks = timeout_ticks_;
    a.max_stale = -1;
    a.lr_dev = lr_dev_;
    a.herr = reinterpret_cast<unsigned*>(herr_.device());
    a.rank = rank_;
    if (owner_on_) set_owner(a);
    if (nbatches_ > 0) {
      a.sched = ctrl_->sched;
      a.sched_ctr = ctrl_->sched_ctr;
      a.done_epoch = ctrl_->done_epoch;
      a.claimed_epoch = ctrl_->claimed_epoch;
      a.nbatches = nbatches_;
      a.max_epochs = max_epochs_;
    }
    return a;
  }
  HostFlag herr_;
  int rank_, world_, server_, dev_ = 0, shift_ = 6;
  bool joiner_ = false;
  bool joinable_ = false;  // other processes may attach: uncached buffers, no exclusive-writer shortcuts
  int max_epochs_ = 0;
  int64_t n_, timeout_ticks_ = 0, nbatches_ = 0;
  dfa::PSCtrl* ctrl_ = nullptr;  // the server's control buffer (csrc/ps_layout.h)
  float* own_ = nullptr;
  float* shard_[dfa::kP2PMaxRanks];
  dfa::PSLocal* loc_ = nullptr;  // this rank's protocol words
  float* lr_dev_ = nullptr;
  torch::Tensor lr_keep_;
  Audit audit_, fed_audit_;
  int owner_ring_ = 0;
  bool owner_on_ = false;
  float* inbox_own_ = nullptr;
  float* inbox_[dfa::kP2PMaxRanks] = {};
  int fed_K_ = 0;
  float* fed_own_ = nullptr;
  float* fed_slot_[dfa::kP2PMaxRanks] = {};
};

}  // namespace dfa_py
