// uwvk_stage.hpp — the host arrays of one device-resident run call
// (uwvk_bottom_run_log, uwvk_ipose_run_log: the epoch table and the shared
// visual inputs; uwvk_pose_run_log_visual: the shared visual inputs of all the
// rows of the call): written into pinned host memory before the call returns,
// copied to the device on the handle's stream.  A slot is free again once the
// event behind its last launch has passed, so a later call never overwrites
// what a queued launch still reads (StageDone records that event for every
// caller).  What the visual rows put into a slot: uwvk_visual_rows.hpp.
#pragma once
#include <hip/hip_runtime.h>

#include <algorithm>
#include <vector>

namespace uwvk {

struct StageSlot {
  char* host = nullptr;  // pinned
  char* dev = nullptr;
  size_t cap = 0;        // bytes
  hipEvent_t done = nullptr;
  bool used = false;
};

inline void stage_release(std::vector<StageSlot>& stages) {
  for (StageSlot& s : stages) {
    if (s.host) (void)hipHostFree(s.host);
    if (s.dev) (void)hipFree(s.dev);
    if (s.done) (void)hipEventDestroy(s.done);
  }
  stages.clear();
}

// a slot of at least `bytes` that no queued launch reads any more
inline StageSlot* stage_acquire(std::vector<StageSlot>& stages, size_t bytes) {
  StageSlot* s = nullptr;
  for (StageSlot& c : stages)
    if (!c.used || hipEventQuery(c.done) == hipSuccess) {
      c.used = false;
      if (!s) s = &c;
    }
  if (!s) {
    stages.emplace_back();
    s = &stages.back();
    if (hipEventCreateWithFlags(&s->done, hipEventDisableTiming) != hipSuccess) {
      s->done = nullptr;
      stages.pop_back();
      return nullptr;
    }
  }
  if (s->cap < bytes) {
    if (s->host) (void)hipHostFree(s->host);
    if (s->dev) (void)hipFree(s->dev);
    s->host = s->dev = nullptr;
    s->cap = 0;
    const size_t cap = std::max<size_t>(bytes, 32768);
    if (hipHostMalloc((void**)&s->host, cap, hipHostMallocDefault) != hipSuccess ||
        hipMalloc((void**)&s->dev, cap) != hipSuccess) {
      if (s->host) (void)hipHostFree(s->host);
      s->host = s->dev = nullptr;
      return nullptr;
    }
    s->cap = cap;
  }
  return s;
}

// Marks a slot whose copy has been queued (`used` set) as free again once the
// launches queued so far have passed: the event is recorded when the scope
// ends, an early return after a failed copy or launch included (a return
// before `used` is set leaves the slot free).  If the event cannot be
// recorded there is no telling when the slot is free: wait now.
struct StageDone {
  StageSlot* sg;  // nullable
  hipStream_t st;
  ~StageDone() {
    if (sg && sg->used && hipEventRecord(sg->done, st) != hipSuccess) {
      (void)hipStreamSynchronize(st);
      sg->used = false;
    }
  }
};

}  // namespace uwvk
