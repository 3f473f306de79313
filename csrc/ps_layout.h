// Byte layout of the device parameter server's two raw buffers (host: PSComm in bindings_comm.h; device:
// the words PSArgs / FedArgs point at, csrc/async_ps.hip, csrc/fedsgd_ps.hip, csrc/ps_device.h).
// Plain C++: no HIP or torch types, usable from host and device translation units.  The static_asserts
// pin every offset; a protocol change edits the struct and its assert, nothing else.
#pragma once
#include <cstddef>

namespace dfa {

constexpr int kP2PMaxRanks = 8;
constexpr int kPSMaxGrid = 64;                // workgroups of a pull / apply launch
constexpr int kPSDecisionWord = 3;            // scratch word of the tagged admission decision (ps_device.h kPSDecision)
constexpr int kPSVMinWord = 4;                // scratch word of the refresh minimum (ps_device.h kPSVMin)
constexpr long long kPSMaxBatches = 1 << 20;  // capacity of the shared completion arrays

// The server rank's control buffer (uncached, IPC-mapped into every rank).
struct PSCtrl {
  unsigned ver;                      // admitted-gradient counter (the model version)
  unsigned pad0_;
  unsigned applied;                  // gradients whose every add has landed (CAS path)
  unsigned pad1_;
  unsigned long long batch_ctr;      // FCFS microbatch cursor
  unsigned long long pad2_;
  unsigned sched[2];                 // dataset epoch, batches completed in it
  unsigned long long pad3_;
  unsigned long long sched_ctr[4];   // completed, redispatched, skipped, duplicate
  unsigned fed_seq;                  // FedSGD version seqlock (2v stable, odd: being applied)
  unsigned pad4_;
  unsigned long long fed_tick;       // (seq << 32) | tickets taken for that version
  unsigned long long fed_land;       // (seq << 32) | mask of the landed slots
  unsigned long long fed_bad;        // (seq << 32) | mask of the slots landed as bad
  unsigned long long pad5_[10];
  unsigned pref[kP2PMaxRanks];       // owner-applies: drained sequence count of every owner
  unsigned dlock[kP2PMaxRanks];      // owner-applies: drain locks (0 free, rank + 1 held)
  unsigned done_epoch[kPSMaxBatches];     // e + 1 once batch b is applied in epoch e
  unsigned claimed_epoch[kPSMaxBatches];  // likewise for its first dispatch
};
constexpr size_t ps_ctrl_bytes() { return sizeof(PSCtrl); }

// Every rank's own 4 KiB of protocol words (plain device memory).
struct PSLocal {
  unsigned vpulled;                  // vp of the last admission
  unsigned pad0_;
  long long bid_out;                 // claimed microbatch (epoch << 32 | batch), -1 = dataset finished
  unsigned long long pad1_[6];
  unsigned long long stats[8];       // PSArgs::stats
  unsigned long long pad2_[112];
  unsigned scratch[256];             // PSArgs::scratch (word indices: ps_device.h)
  float* selftest_tab[kP2PMaxRanks];  // the shards' self-test areas (ps_selftest_add)
  unsigned long long pad3_[56];
  unsigned fed_scratch[256];         // FedArgs::scratch (word indices: fedsgd_ps.hip)
  unsigned long long fed_stats[8];   // FedArgs::stats
  unsigned long long pad4_[56];
};

#define DFA_PS_AT(S, f, off) static_assert(offsetof(S, f) == (off), #S "::" #f " moved")
DFA_PS_AT(PSCtrl, ver, 0);
DFA_PS_AT(PSCtrl, applied, 8);
DFA_PS_AT(PSCtrl, batch_ctr, 16);
DFA_PS_AT(PSCtrl, sched, 32);
DFA_PS_AT(PSCtrl, sched_ctr, 48);
DFA_PS_AT(PSCtrl, fed_seq, 80);
DFA_PS_AT(PSCtrl, fed_tick, 88);
DFA_PS_AT(PSCtrl, fed_land, 96);
DFA_PS_AT(PSCtrl, fed_bad, 104);
DFA_PS_AT(PSCtrl, pref, 192);
DFA_PS_AT(PSCtrl, dlock, 224);
DFA_PS_AT(PSCtrl, done_epoch, 256);
DFA_PS_AT(PSCtrl, claimed_epoch, 256 + kPSMaxBatches * 4);
static_assert(ps_ctrl_bytes() == 256 + 2 * kPSMaxBatches * 4, "PSCtrl size");
DFA_PS_AT(PSLocal, vpulled, 0);
DFA_PS_AT(PSLocal, bid_out, 8);
DFA_PS_AT(PSLocal, stats, 64);
DFA_PS_AT(PSLocal, scratch, 1024);
DFA_PS_AT(PSLocal, selftest_tab, 2048);
DFA_PS_AT(PSLocal, fed_scratch, 2560);
DFA_PS_AT(PSLocal, fed_stats, 3584);
#undef DFA_PS_AT
static_assert(sizeof(PSLocal) == 4096, "PSLocal size");
static_assert(sizeof(PSLocal::scratch) == 1024 && sizeof(PSLocal::fed_scratch) == 1024, "scratch areas");
static_assert(offsetof(PSLocal, fed_scratch) + sizeof(PSLocal::fed_scratch) == offsetof(PSLocal, fed_stats),
              "fed_scratch ends where fed_stats begins");
// the device-side word indices must fit their area (asserted next to their definitions)
constexpr int kPSScratchWords = sizeof(PSLocal::scratch) / 4, kFedScratchWords = sizeof(PSLocal::fed_scratch) / 4;
static_assert(kPSDecisionWord < kPSScratchWords && kPSVMinWord < kPSScratchWords, "scratch words");

}  // namespace dfa
