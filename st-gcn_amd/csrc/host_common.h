// Host-side helpers of the C-ABI entry points (capi.hip, train_ops.hip,
// optim.hip, input_stage.hip): the error return, the alignment check and the
// side stream of stgcn_block_bwd.
#pragma once
#include <hip/hip_runtime.h>

#include <atomic>
#include <cstdint>
#include <initializer_list>
#include <mutex>
#include <string>

#include "../../include/stgcn_hip.h"

namespace stgcn {

void set_last_error(const std::string &msg);  // capi.hip (stgcn_last_error)

inline int fail(int code, const std::string &msg) {
  set_last_error(msg);
  return code;
}

// The alignment contract of stgcn_hip.h (Conventions): the first pointer of the
// list that is off `align` bytes fails the call, by name, before any launch.
// Null pointers pass (optional arguments; the null checks come first).
struct NamedPtr {
  const void *p;
  const char *name;
};
inline int check_aligned(std::initializer_list<NamedPtr> ptrs, unsigned align) {
  for (const NamedPtr &q : ptrs)
    if (((uintptr_t)q.p & (align - 1)) != 0)
      return fail(STGCN_E_INVALID,
                  std::string(q.name) + ": must be " + std::to_string(align) + "-byte aligned");
  return STGCN_OK;
}

// ---- the side stream of stgcn_block_bwd (DESIGN.md "Backward small kernels
// beside the GEMMs") ----
// One library-owned stream per device, non-blocking, with a fixed set of untimed
// events. Created by the first call that is not under stream capture and never
// destroyed (process exit cleans up). At the default priority on purpose: with a
// high-priority side stream the captured cfg2 step replayed at 20.5 - 20.8
// ms/step against 14.9 serial, at the default priority at 14.6.
constexpr int kSideDevices = 64;
constexpr int kSideEvents = 6;  // (a forked call orders the two streams at most 5 times)

struct SideSlot {
  std::mutex mu;  // held while a call is forked: one user of the stream and events at a time
  hipStream_t stream = nullptr;
  hipEvent_t ev[kSideEvents] = {};
};

inline SideSlot *side_slots() {
  static SideSlot slots[kSideDevices];
  return slots;
}

// process-wide mode of stgcn_bwd_overlap: 1 = fork where it applies, 0 = serial
inline std::atomic<int> &bwd_overlap_mode() {
  static std::atomic<int> mode{1};
  return mode;
}

// Fork / join of one call: begin() forks the side stream from the caller's
// stream (everything enqueued there so far precedes the side stream's work),
// to_side() / to_main() order one stream after what the other holds so far, and
// join() -- also run by the destructor, so on every exit path -- makes the
// caller's stream wait for the side stream's last work. Not forked (never
// begun, begin() refused, or joined): side() is the caller's stream, nothing is
// recorded, and the launches are the serial sequence. Under stream capture the
// first wait pulls the side stream into the capture and join() ends its branch.
class SideFork {
 public:
  SideFork() = default;
  SideFork(const SideFork &) = delete;
  SideFork &operator=(const SideFork &) = delete;
  ~SideFork() { (void)join(); }

  hipStream_t side() const { return slot_ ? slot_->stream : main_; }
  bool forked() const { return slot_ != nullptr; }

  // Refused (the call stays serial, no error): mode 0, a capture status that
  // cannot be read, or a capture in progress before the device's slot exists --
  // nothing is created during a capture.
  hipError_t begin(hipStream_t main) {
    main_ = main;
    if (!bwd_overlap_mode().load(std::memory_order_relaxed)) return hipSuccess;
    hipStreamCaptureStatus st = hipStreamCaptureStatusNone;
    int dev = -1;
    if (hipStreamIsCapturing(main, &st) != hipSuccess || hipGetDevice(&dev) != hipSuccess ||
        dev < 0 || dev >= kSideDevices) {
      (void)hipGetLastError();
      return hipSuccess;
    }
    SideSlot *slot = side_slots() + dev;
    std::unique_lock<std::mutex> lock(slot->mu);
    if (!slot->stream) {
      if (st != hipStreamCaptureStatusNone) return hipSuccess;
      if (!create(slot)) return hipSuccess;
    }
    lock_ = std::move(lock);
    slot_ = slot;
    hipError_t e = to_side();
    if (e != hipSuccess) release();  // (nothing is on the side stream yet)
    return e;
  }

  hipError_t to_side() { return slot_ ? order(main_, slot_->stream) : hipSuccess; }
  hipError_t to_main() { return slot_ ? order(slot_->stream, main_) : hipSuccess; }

  hipError_t join() {
    if (!slot_) return hipSuccess;
    hipError_t e = to_main();
    release();
    return e;
  }

 private:
  // `after` waits for everything `before` holds now
  hipError_t order(hipStream_t before, hipStream_t after) {
    hipEvent_t ev = slot_->ev[next_++ % kSideEvents];
    hipError_t e = hipEventRecord(ev, before);
    return e != hipSuccess ? e : hipStreamWaitEvent(after, ev, 0);
  }
  void release() {
    slot_ = nullptr;
    if (lock_.owns_lock()) lock_.unlock();
  }
  static bool create(SideSlot *slot) {
    hipStream_t s = nullptr;
    hipEvent_t ev[kSideEvents] = {};
    bool ok = hipStreamCreateWithFlags(&s, hipStreamNonBlocking) == hipSuccess;
    for (int i = 0; ok && i < kSideEvents; ++i)
      ok = hipEventCreateWithFlags(&ev[i], hipEventDisableTiming) == hipSuccess;
    if (!ok) {  // (serial from now on for this call; the next one tries again)
      for (hipEvent_t e : ev)
        if (e) (void)hipEventDestroy(e);
      if (s) (void)hipStreamDestroy(s);
      (void)hipGetLastError();
      return false;
    }
    for (int i = 0; i < kSideEvents; ++i) slot->ev[i] = ev[i];
    slot->stream = s;
    return true;
  }

  hipStream_t main_ = nullptr;
  SideSlot *slot_ = nullptr;
  std::unique_lock<std::mutex> lock_;
  unsigned next_ = 0;
};

}  // namespace stgcn

#define NP(v) stgcn::NamedPtr{v, #v}

#define HIP_TRY(expr)                                                                       \
  do {                                                                                      \
    hipError_t e_ = (expr);                                                                 \
    if (e_ != hipSuccess)                                                                   \
      return stgcn::fail(STGCN_E_HIP, std::string(#expr) + ": " + hipGetErrorString(e_));  \
  } while (0)
