// plan_check.hpp — what the plan tests (plan_test.cpp, fix_plan_test.cpp,
// delayed_plan_test.cpp) share: the check macro, the flag names, the default
// handle facts, and a plan printed and compared launch by launch.
#pragma once
#include <cstdio>
#include <initializer_list>
#include <string>
#include <utility>
#include <vector>

#include "../../slam-uwv_kalman_filters_amd/csrc/uwvk_plan.hpp"

using namespace uwvk;

inline int g_fail = 0;
#define CHECK(c)                                               \
  do {                                                         \
    if (!(c)) {                                                \
      std::printf("FAIL %s:%d: %s\n", __FILE__, __LINE__, #c); \
      g_fail++;                                                \
    }                                                          \
  } while (0)

constexpr uint32_t IMU = UWVK_EV_ACC, P = UWVK_EV_PRESSURE, A = UWVK_EV_ADCP, E = UWVK_EV_EFFORTS,
                   VO = UWVK_EV_EFFORTS_VELOCITY_ONLY;
constexpr uint32_t XY = UWVK_FIX_XY, Z = UWVK_FIX_Z, GEO = UWVK_FIX_GEO;
constexpr uint32_t ARR = kDelayedArrive, LAT = kDelayedLatch;

// dof 53, an even batch, every option at its default, a decoupled state and a
// simple, parameter-diagonal Q
inline EpochFacts defaults() { return {53, 64, 1, 1, 1, 0, false, true, true, true}; }

// "PAIR[0,60)pd EFFORTS(59,vo=0) FIX(59,m=9) LATCH(59) REC(59) ONE[60,120) pdec=0"; a dense epoch "DENSE[3,4) "
inline std::string show(const EpochPlan& p) {
  std::string s;
  for (const Launch& l : p.launches) {
    const std::string e = std::to_string(l.first);
    if (l.kind == EFFORTS) s += "EFFORTS(" + e + ",vo=" + std::to_string(l.vo) + ") ";
    else if (l.kind == FIX) s += "FIX(" + e + ",m=" + std::to_string(l.ev_any) + ") ";
    else if (l.kind == LATCH) s += "LATCH(" + e + ") ";
    else if (l.kind == RECORD) s += "REC(" + e + ") ";
    else
      s += std::string(l.kind == EPOCH_PAIR ? "PAIR[" : l.kind == EPOCH_DENSE ? "DENSE[" : "ONE[") + e + "," +
           std::to_string(l.first + l.count) + ")" + (l.pd ? "pd " : " ");
  }
  return s + "pdec=" + std::to_string((int)p.pdec);
}
// the launches alone: what calls over adjacent ranges concatenate
inline std::string show_launches(const EpochPlan& p) {
  const std::string t = show(p);
  return t.substr(0, t.rfind("pdec="));
}

// n epochs of `base`, ev's (epoch, bits) ORed in
using Ev = std::initializer_list<std::pair<int64_t, uint32_t>>;
inline std::vector<uint32_t> flags(int64_t n, uint32_t base, Ev ev = {}) {
  std::vector<uint32_t> f((size_t)n, base);
  for (auto& e : ev) f[(size_t)e.first] |= e.second;
  return f;
}

inline bool same(const EpochPlan& a, const EpochPlan& b) {
  if (a.pdec != b.pdec || a.launches.size() != b.launches.size()) return false;
  for (size_t i = 0; i < a.launches.size(); i++) {
    const Launch &x = a.launches[i], &y = b.launches[i];
    if (x.kind != y.kind || x.first != y.first || x.count != y.count || x.pd != y.pd || x.vo != y.vo ||
        x.ev_any != y.ev_any)
      return false;
  }
  return true;
}

inline void expect_plan(const EpochPlan& p, const char* want, int line) {
  const std::string got = show(p);
  if (got != want) {
    std::printf("FAIL line %d:\n  got  %s\n  want %s\n", line, got.c_str(), want);
    g_fail++;
  }
}
