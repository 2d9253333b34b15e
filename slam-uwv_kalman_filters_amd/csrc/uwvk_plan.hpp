// uwvk_plan.hpp — the host planning of uwvk_pose_run_log, as pure functions of
// integers and host arrays (plain C++17, no HIP): which epoch kernel a handle
// runs, the one launch list of a call (plan_run: epochs, BodyEfforts, position
// fixes, latches and track records), the checks of the fix and delayed
// arguments and of the track argument (track_args_valid, which the run_log
// calls of the other filters share), the grid and tail layout of one launch,
// and the process-noise tables.  uwvk_pose.hip does the copies and walks the list;
// tests/cpp/plan_test.cpp, track_plan_test.cpp, fix_plan_test.cpp,
// delayed_plan_test.cpp and visual_plan_test.cpp check this file on the CPU.
#pragma once
#include <algorithm>
#include <cstdint>
#include <utility>
#include <vector>

#include "../../include/uwvk.h"

namespace uwvk {

// Qh: the host copy of Q, dof x dof row-major, or empty (all zero)
inline double q_at(int dof, const std::vector<double>& Qh, int i, int j) {
  return Qh.empty() ? 0.0 : Qh[(size_t)i * dof + j];
}

// lane-resident Q (psp::LaneQ): no coupling of the rewritten rows (< 9) with
// anything but their own diagonal / the orientation block, and a band of at
// most 2 below the diagonal in rows >= 9 (the epoch kernel's QM = 1)
inline bool q_is_simple(int dof, const std::vector<double>& Qh) {
  for (int i = 0; i < dof; i++)
    for (int j = 0; j < i; j++) {
      if (q_at(dof, Qh, i, j) == 0.0) continue;
      const bool ori = i >= 3 && i < 6 && j >= 3 && j < 6;
      if ((i < 9 || j < 9) ? !ori : (i - j > 2)) return false;
    }
  return true;
}

// the process noise leaves the parameter block decoupled: no Q entry in a
// parameter row / column (tangent 19..45) off the diagonal
inline bool q_params_diag(int dof, const std::vector<double>& Qh) {
  if (dof != 53) return false;
  for (int i = 0; i < 53; i++)
    for (int j = 0; j < 53; j++)
      if (i != j && ((i >= 19 && i <= 45) || (j >= 19 && j <= 45)) && q_at(53, Qh, i, j) != 0.0) return false;
  return true;
}

// the parameter block of Sigma decoupled (PD kernel): every lower-triangle
// entry in a parameter row or column (tangent 19..45) off the diagonal is zero
// in every instance.  Pp: [batch] packed lower triangles
inline bool param_block_decoupled(int dof, int64_t batch, const double* Pp) {
  if (dof != 53) return false;
  const int tn = 53 * 54 / 2;
  for (int64_t b = 0; b < batch; b++)
    for (int i = 19, k0 = 19 * 20 / 2; i < 53; k0 += ++i)
      for (int j = 0; j < i; j++)
        if ((i <= 45 || (j >= 19 && j <= 45)) && Pp[b * tn + k0 + j] != 0.0) return false;
  return true;
}

// DOF d of the PD kernel's 26-DOF subset in the 53-DOF tangent (the 27
// parameters, 19..45, taken out)
constexpr int pd_dof(int d) { return d < 19 ? d : d + 27; }

// What the PSP kernels read of Q for one dt.  qp: {A_ii A_jj, dt^2 Q_ij} per
// packed entry; band: dt^2 Q of the rows >= 9, row i's columns [qlo[i], i] at
// qoff[i] (q_band 0 when it does not fit), q_bw its widest row; qpd: the PD
// kernel's table (below)
constexpr int kQBand = 128, kQpdEntries = 351 + 32;
struct QTables {
  std::vector<double> qp, band, qpd;
  int qlo[56] = {}, qoff[56] = {}, q_band = 1, q_bw = 0, q_simple = 1;
};

// ntau: -1 / tau of {gyro bias, acc bias, inertia, lin damping, quad damping,
// water velocity, ADCP bias, density} (PoseShared::ntau)
inline QTables build_q_tables(int dof, const std::vector<double>& Qh, const double ntau[8], double dt) {
  const int n = dof;
  QTables t;
  // A_ii: the diagonal of the process model's Jacobian, the same expressions as
  // psp::proc_diag (1 + dt (-1/tau) per Markov block, 1 otherwise)
  struct Block { int d0, len, tau; };  // tangent offsets of Lay<53> / Lay<26>
  static const std::vector<Block> b53 = {{12, 3, 0}, {15, 3, 1}, {19, 9, 2}, {28, 9, 3},
                                         {37, 9, 4}, {46, 4, 5}, {50, 2, 6}, {52, 1, 7}};
  static const std::vector<Block> b26 = {{12, 3, 0}, {15, 3, 1}, {19, 4, 5}, {23, 2, 6}, {25, 1, 7}};
  std::vector<double> ad(n, 1.0);
  for (const Block& b : n == 53 ? b53 : b26)
    for (int d = b.d0; d < b.d0 + b.len; d++) ad[d] = 1.0 + dt * ntau[b.tau];
  auto rewritten = [](int d) { return d < 9; };  // pos, ori, vel rows: rewritten by the kernel
  auto Qij = [&](int i, int j) { return q_at(n, Qh, i, j); };
  t.qp.resize((size_t)n * (n + 1));
  const double dt2 = dt * dt;
  for (int i = 0, k = 0; i < n; i++)
    for (int j = 0; j <= i; j++, k++) {
      t.qp[2 * k] = (rewritten(i) || rewritten(j)) ? 0.0 : ad[i] * ad[j];
      t.qp[2 * k + 1] = dt2 * Qij(i, j);
    }
  // band of rows >= 9: first nonzero column >= 9 .. diagonal
  t.band.assign(kQBand, 0.0);
  for (int i = 0, off = 0; i < n; i++) {
    int lo = i + 1;
    if (i >= 9)
      for (int j = 9; j <= i; j++)
        if (Qij(i, j) != 0.0) { lo = j; break; }
    t.qlo[i] = lo;
    t.qoff[i] = off;
    for (int j = lo; j <= i; j++, off++) {
      if (off < kQBand) t.band[off] = dt2 * Qij(i, j);
      else t.q_band = 0;
    }
  }
  for (int i = 9; i < n; i++) t.q_bw = std::max(t.q_bw, i - t.qlo[i]);
  t.q_simple = q_is_simple(n, Qh) ? 1 : 0;
  // the PD kernel's table: the 26-DOF subset's entries in its packed order,
  // then parameter p's (19 + p, 19 + p) entry at 351 + p (psp::lane_q PD)
  t.qpd.assign(kQpdEntries * 2, 0.0);
  if (n == 53) {
    for (int i = 0, k = 0; i < 26; i++)
      for (int j = 0; j <= i; j++, k++) {
        const int I = pd_dof(i), J = pd_dof(j), k53 = I * (I + 1) / 2 + J;
        t.qpd[2 * k] = t.qp[2 * k53];
        t.qpd[2 * k + 1] = t.qp[2 * k53 + 1];
      }
    for (int p = 0; p < 27; p++) {
      const int d = 19 + p, k53 = d * (d + 1) / 2 + d;
      t.qpd[2 * (351 + p)] = t.qp[2 * k53];
      t.qpd[2 * (351 + p) + 1] = t.qp[2 * k53 + 1];
    }
  }
  return t;
}

// what run_log's kernel choice depends on, taken from the handle once per call
struct EpochFacts {
  int dof;
  int64_t batch;
  int pd_opt, pair_opt, persist;  // UWVK_OPT_PARAM_BLOCK, UWVK_OPT_PAIR, UWVK_OPT_PERSIST
  uint32_t lds_pad;               // UWVK_OPT_LDS_PAD
  bool dense;                     // the literal kernels (no PSP launch at all)
  bool pdec;                      // Sigma's parameter block decoupled at init and since
  bool q_simple, q_params_diag;   // of the current host Q
};

// the one-instance parameter-decoupled kernel (psp::PspSmemPD)
inline bool runs_pd(const EpochFacts& f) {
  return f.pd_opt && f.pdec && f.dof == 53 && f.q_simple && f.q_params_diag;
}

// the two-instances-per-wave kernel (UWVK_OPT_PAIR): the parameter-decoupled
// state of a 53-DOF handle, or a 26-DOF handle's own state (r06), on the
// persistent scheduler, an even batch, the lane-resident Q and no LDS pad
inline bool runs_pair(const EpochFacts& f) {
  if (!f.pair_opt || !f.persist || f.batch % 2 != 0 || f.lds_pad != 0 || f.dense) return false;
  return f.dof == 26 ? f.q_simple : runs_pd(f);
}

enum LaunchKind { EPOCH_ONE, EPOCH_PAIR, EPOCH_DENSE, EFFORTS, FIX, LATCH, RECORD, VISUAL };
struct Launch {
  LaunchKind kind;
  int64_t first, count;  // absolute epochs [first, first + count); all but EPOCH_ONE / EPOCH_PAIR: the one epoch
  int pd;                // EPOCH_*: the parameter-decoupled form
  int vo;                // EFFORTS: the velocity-only form (UWVK_EV_EFFORTS_VELOCITY_ONLY)
  uint32_t ev_any;       // the OR of the epochs' flags (the kernel instantiation)
};
struct EpochPlan {
  std::vector<Launch> launches;
  bool pdec;  // EpochFacts::pdec after the last launch
};

// a run of epochs without pressure shorter than this stays on the one-instance
// kernel: each extra launch costs a Sigma round trip and a ramp
constexpr int64_t kPairMinRun = 48;

// One epoch launch per run of epochs up to and including the next BodyEfforts
// epoch (its predict and other updates); that epoch's efforts update alone
// then runs in its own one-wave kernel (EFFORTS: the full model or its
// velocity-only form).  Efforts is the last update of an epoch (the fused
// literal order), so the split is exact.  The full model couples the
// parameters: no PD or pair kernel after it.
// The pair kernel runs the epochs without a pressure update (its 39 sigma
// points do not fit a half-wave): a range with pressure epochs is split around
// them when the runs between them are long (kPairMinRun), the pressure epochs
// and short runs on the one-instance kernel.
// host_flags: the flags of epochs first .. first + count - 1
inline EpochPlan plan_epochs(const uint32_t* host_flags, int64_t first, int64_t count, EpochFacts f) {
  EpochPlan p;
  const int64_t end = first + count;
  auto flags = [&](int64_t k) { return host_flags[k - first]; };
  auto epochs = [&](LaunchKind kind, int64_t s0, int64_t s1) {
    uint32_t ev_any = 0;
    for (int64_t k = s0; k < s1; k++) ev_any |= flags(k);
    p.launches.push_back({kind, s0, s1 - s0, runs_pd(f) ? 1 : 0, 0, ev_any});
  };
  for (int64_t e = first; e < end;) {
    int64_t r = e;
    while (r < end && !(flags(r) & UWVK_EV_EFFORTS)) r++;
    const int64_t last = r < end ? r + 1 : r;
    if (!runs_pair(f)) {
      epochs(EPOCH_ONE, e, last);
    } else {
      int64_t s0 = e;  // start of the pending one-instance segment
      for (int64_t k = e; k < last;) {
        if (flags(k) & UWVK_EV_PRESSURE) { k++; continue; }
        int64_t q = k;  // a run of epochs without pressure: [k, q)
        while (q < last && !(flags(q) & UWVK_EV_PRESSURE)) q++;
        if (q - k >= kPairMinRun || (k == e && q == last)) {
          if (k > s0) epochs(EPOCH_ONE, s0, k);
          epochs(EPOCH_PAIR, k, q);
          s0 = q;
        }
        k = q;
      }
      if (last > s0) epochs(EPOCH_ONE, s0, last);
    }
    if (r < end) {
      const int vo = (flags(r) & UWVK_EV_EFFORTS_VELOCITY_ONLY) ? 1 : 0;
      if (!vo) f.pdec = false;
      p.launches.push_back({EFFORTS, r, 1, 0, vo, flags(r)});
    }
    e = last;
  }
  p.pdec = f.pdec;
  return p;
}

// The track of uwvk_pose_run_log_track: a record is taken after each absolute
// epoch e with (e + 1) % every == 0.  Records in [first, first + count), every > 0:
inline int64_t track_records(int64_t first, int64_t count, int64_t every) {
  return (first + count) / every - first / every;
}
// The track argument of every run_log entry point (PoseUKF, BottomUKF,
// IndirectPoseUKF, VelocityUKF), after the range check (first, count >= 0): a
// positive stride, at least one output array, and room for the range's records.
inline bool track_args_valid(int64_t every, int64_t capacity, bool any_output, int64_t first, int64_t count) {
  return every > 0 && any_output && capacity >= track_records(first, count, every);
}

// Delayed XY (uwvk_pose_run_log_delayed): per epoch two internal bits, made by
// delayed_events (below) from uwvk_pose_delayed's index and latch_epoch arrays;
// they lie outside UWVK_FIX_*, so a FIX launch's mask can hold the fix kinds
// and the arrival bit.
constexpr uint32_t kDelayedArrive = 0x8u;  // a delayed row arrives at this epoch (its update runs)
constexpr uint32_t kDelayedLatch = 0x10u;  // rows latch the position after this epoch's updates

// The launch list of one run_log call, in stream order.  One rule: the range
// [first, first + count) is cut after every epoch with an event (a fix flag,
// an arrival, a visual row, a latch, or a track record: (e + 1) % every == 0); each piece is
// planned by plan_epochs on its own, pdec carried from piece to piece; then the
// epoch's events follow the piece (and its EFFORTS launch, if the epoch has
// one) in the order of uwvk.h: one FIX launch if the epoch has fixes or an
// arrival (ev_any the UWVK_FIX_* kinds plus kDelayedArrive: the delayed update
// is the last position update, in the same launch), one VISUAL launch if the
// epoch has visual-landmark rows (uwvk_pose_run_log_visual: all of its rows, in
// row order), one LATCH (the latch sees all updates of its epoch), one RECORD.  So a call with events is the calls
// of its pieces, launch for launch, and without events it is plan_epochs' plan.
// The position updates are linear in the position rows and leave the
// parameter block decoupled: pd / pair go on after them.  The visual update is
// the literal augmented one (all sigma points), as the single call: pdec is
// false after a VISUAL launch and the later pieces run the general kernel.
// A dense handle (the literal kernels) runs one fused EPOCH_DENSE launch per
// epoch instead, its efforts update included (no EFFORTS launch; host_flags is
// not read), and is never parameter-decoupled afterwards.
// host_flags, fix_flags, delayed_flags, visual_flags: those of epochs first ..
// first + count - 1, the last three or null (none); visual_flags[k] != 0: epoch
// first + k has a visual row; every: the track's stride, or 0 (no track)
inline EpochPlan plan_run(const uint32_t* host_flags, const uint32_t* fix_flags, const uint32_t* delayed_flags,
                          int64_t every, int64_t first, int64_t count, EpochFacts f,
                          const uint32_t* visual_flags = nullptr) {
  EpochPlan p;
  if (f.dense) f.pdec = false;
  p.pdec = f.pdec;
  const int64_t end = first + count;
  auto fixes = [&](int64_t k) { return fix_flags ? fix_flags[k - first] : 0u; };
  auto delayed = [&](int64_t k) { return delayed_flags ? delayed_flags[k - first] & (kDelayedArrive | kDelayedLatch) : 0u; };
  auto record = [&](int64_t k) { return every > 0 && (k + 1) % every == 0; };
  auto visual = [&](int64_t k) { return visual_flags && visual_flags[k - first] != 0u; };
  for (int64_t e = first; e < end;) {
    int64_t stop = e;
    while (stop < end && !(fixes(stop) || delayed(stop) || visual(stop) || record(stop))) stop++;
    const bool event = stop < end;
    if (event) stop++;  // the piece includes its event epoch
    if (f.dense) {
      for (int64_t k = e; k < stop; k++) p.launches.push_back({EPOCH_DENSE, k, 1, 0, 0, 0});
    } else {
      const EpochPlan piece = plan_epochs(host_flags + (e - first), e, stop - e, f);
      p.launches.insert(p.launches.end(), piece.launches.begin(), piece.launches.end());
      f.pdec = p.pdec = piece.pdec;
    }
    if (event) {
      const int64_t k = stop - 1;
      const uint32_t fix = fixes(k) | (delayed(k) & kDelayedArrive);
      if (fix) p.launches.push_back({FIX, k, 1, 0, 0, fix});
      if (visual(k)) {
        p.launches.push_back({VISUAL, k, 1, 0, 0, 0});
        f.pdec = p.pdec = false;
      }
      if (delayed(k) & kDelayedLatch) p.launches.push_back({LATCH, k, 1, 0, 0, kDelayedLatch});
      if (record(k)) p.launches.push_back({RECORD, k, 1, 0, 0, 0});
    }
    e = stop;
  }
  return p;
}

// uwvk_pose_run_log_fixes' argument check over epochs [first, first + count):
// every flagged kind has its index and payload arrays and a row inside them
// (an out-of-range row would be an out-of-bounds device read).  Reads the host
// arrays only; the device pointers are tested for null.
inline bool fixes_valid(const uwvk_pose_fixes* fx, int64_t first, int64_t count) {
  if (!fx->host_flags) return false;
  struct K {
    uint32_t bit;
    const int32_t* index;
    const double* rows;
    int64_t n;
  } ks[3] = {{UWVK_FIX_XY, fx->xy_index, fx->xy, fx->n_xy},
             {UWVK_FIX_Z, fx->z_index, fx->z, fx->n_z},
             {UWVK_FIX_GEO, fx->geo_index, fx->geo, fx->n_geo}};
  for (int64_t e = first; e < first + count; e++) {
    const uint32_t f = fx->host_flags[e];
    if (f & ~(UWVK_FIX_XY | UWVK_FIX_Z | UWVK_FIX_GEO)) return false;
    for (const K& k : ks)
      if ((f & k.bit) && (!k.index || !k.rows || k.index[e] < 0 || k.index[e] >= k.n)) return false;
  }
  return true;
}

// uwvk_pose_run_log_delayed's argument check (epochs: the log's), and what
// [first, first + count) holds of the rows (out): plan_run's delayed flags and
// the latches to run.  An out-of-range row would be an out-of-bounds device
// access.  Reads the host arrays only, like fixes_valid.
struct DelayedEvents {
  std::vector<uint32_t> flags;                       // kDelayedArrive / kDelayedLatch of epoch first + k
  std::vector<std::pair<int64_t, int32_t>> latches;  // (latch epoch, row) of the range, ascending
};
inline bool delayed_events(const uwvk_pose_delayed* d, int64_t epochs, int64_t first, int64_t count,
                           DelayedEvents* out) {
  if (d->n < 0) return false;
  if (d->n > 0 && (!d->index || !d->latch_epoch || !d->xy || !d->latched)) return false;
  out->flags.assign((size_t)count, 0u);
  out->latches.clear();
  for (int64_t r = 0; r < d->n; r++) {
    const int64_t L = d->latch_epoch[r];
    if (L < -1 || L >= epochs) return false;
    if (L >= first && L < first + count) {
      out->flags[(size_t)(L - first)] |= kDelayedLatch;
      out->latches.emplace_back(L, (int32_t)r);
    }
  }
  std::sort(out->latches.begin(), out->latches.end());
  if (!d->index) return true;  // n == 0, no index array: no events
  for (int64_t e = first; e < first + count; e++) {
    const int64_t r = d->index[e];
    if (r < -1 || r >= d->n) return false;
    if (r < 0) continue;
    if (d->latch_epoch[r] >= e) return false;
    out->flags[(size_t)(e - first)] |= kDelayedArrive;
  }
  return true;
}

// Last-generation spreading.  Blocks of one XCD are dispatched in order to
// its s resident slots; wave speeds differ (the first generation's waves end
// anywhere between 0.8 and 1.25 of the mean), so after a few generations the
// slots free up at scattered times and a launch of whole-instance blocks of
// duration D ends with a ramp: the slots idle for D / 2 on average while the
// last blocks finish.  Spreading ends the launch on short blocks instead: the
// last m = C s instances of each XCD run as C epoch chunks, grouped by chunk
// (all chunk-0 blocks after the whole instances, then all chunk-1 blocks,
// ...), so each group keeps the XCD busy for about D and a chunk's
// predecessor, m blocks earlier, has long finished; the ramp shrinks to
// D / (2 C), for (C - 1) m extra block prologues and epilogues (Sigma~ and
// its time scale reloaded and stored, the IMU prefetch restarted: about 0.75
// epoch each, r02 timeline).  C minimises
// count / (2 C) + 0.3 C (C - 1) epochs; none below a 10 % gain or when the
// XCD has under (C + 1) s instances.
constexpr double kTailChunkOverhead = 0.75;  // epochs per extra chunk (r02 timeline)
// chunks per tail instance for n instances over s resident blocks in a
// count-epoch launch (1: no tail spreading)
inline int plan_tail(int64_t n, int64_t s, int64_t count) {
  if (s <= 0 || count < 4) return 1;
  const double base = 0.5 * (double)count;
  double best = 0.9 * base;
  int chunks = 1;
  for (int c = 2; c <= 8 && 2 * c <= count; c++) {
    if (n < (c + 1) * s) break;
    const double cost = (double)count / (2.0 * c) + kTailChunkOverhead * c * (c - 1);
    if (cost < best) {
      best = cost;
      chunks = c;
    }
  }
  return chunks;
}

// the planner's chunk count, or the forced one (UWVK_OPT_TAIL_CHUNKS >= 2,
// tests: every chunk count, where the shape allows it)
inline int tail_chunks(int64_t n, int64_t s, int64_t count, int tail_force) {
  if (tail_force < 2) return plan_tail(n, s, count);
  return (s > 0 && tail_force <= 8 && tail_force * s <= n && tail_force <= count) ? tail_force : 1;
}

// EpochArgs' layout fields, the grid, and the tail buffers the launch needs
// (tail_need instances now, tail_cap when they have to be allocated; 0: none)
struct Geometry {
  int chunks = 1;
  int64_t n_x = 0, tail0 = 0, r_x = 0;
  uint32_t units = 0;
  int64_t grid = 0;  // 0: one block per instance
  uint32_t wait_bound = 0;
  int64_t tail_need = 0, tail_cap = 0;
};

// tail_wait's sleeps before a hand-off counts as lost (UWVK_OPT_WAIT_BOUND >= 0 overrides: tests)
inline uint32_t tail_wait_bound(uint64_t sleeps_per_epoch, int64_t count, int wait_bound_override) {
  if (wait_bound_override >= 0) return (uint32_t)wait_bound_override;
  return (uint32_t)std::min<uint64_t>(0xffffffffull, (1ull << 20) + sleeps_per_epoch * (uint64_t)count);
}

// Persistent launch (UWVK_OPT_PERSIST): grid = resident blocks (or fewer
// units); the last r = chunks x slots units run as epoch chunks, claimed in
// chunk order (uwvk_psp_k.hip, k_psp_epoch_p).  tail_slots (UWVK_OPT_TAIL_SLOTS)
// < 0 turns the chunks off, > 0 plans for that many slots per XCD.
// units_base: the instances, or (pair) the pair kernel's pairs of instances;
// slots: the kernel's resident blocks on the device (> 0)
inline Geometry persist_geometry(int64_t units_base, int64_t slots, int64_t tail_slots, int tail_force,
                                 uint32_t lds_pad, int64_t count, int pair, int wait_bound_override) {
  Geometry g;
  const int64_t s = tail_slots > 0 ? 8 * tail_slots : slots;
  int c = tail_slots < 0 || lds_pad > 0 || s <= 0 ? 1 : tail_chunks(units_base, s, count, tail_force);
  // the pair kernel's default: no spreading (r06v, interleaved: off +2.4% at 20
  // epochs, a tie at 200; forced 3 / 4 chunks -6% / -18% at 20); an explicit
  // UWVK_OPT_TAIL_SLOTS > 0 or UWVK_OPT_TAIL_CHUNKS still spreads (tests)
  if (pair && tail_slots == 0 && tail_force < 2) c = 1;
  g.tail0 = units_base;
  if (c > 1) {
    g.chunks = c;
    g.r_x = c * s;
    g.tail0 = units_base - g.r_x;
    g.tail_need = g.r_x;
    g.tail_cap = 8 * s;
    // a chunk waits at most for its predecessor's unit and the unit its block
    // held before it: ~2 of the launch's epochs per wave, see static_geometry
    g.wait_bound = tail_wait_bound(128, count, wait_bound_override);
  }
  // the first grid units are the blocks' own; the counter then numbers units
  // grid .. units - 1 and one failing ticket per block: units - grid + grid
  const int64_t units = g.tail0 + (int64_t)g.chunks * g.r_x;
  g.units = (uint32_t)units;
  g.grid = std::min(units, slots);
  return g;
}

// the static launch spreads its tail at all: an LDS pad lowers the resident
// blocks below what the tail plan assumes (UWVK_OPT_LDS_PAD is a diagnostic of
// the unspread launch), and the XCD-ordered layout needs 8 equal shares
inline bool static_may_spread(int64_t batch, int64_t tail_slots, uint32_t lds_pad) {
  return tail_slots >= 0 && lds_pad == 0 && batch % 8 == 0;
}

// Static launch (UWVK_OPT_PERSIST 0): the XCD-ordered tail of k_psp_epoch, per
// XCD n_x = batch / 8 instances over slots_per_xcd resident blocks (tail_slots
// > 0 replaces them)
inline Geometry static_geometry(int64_t batch, int64_t slots_per_xcd, int64_t tail_slots, int tail_force,
                                uint32_t lds_pad, int64_t count, int wait_bound_override) {
  Geometry g;
  if (!static_may_spread(batch, tail_slots, lds_pad)) return g;
  const int64_t n = batch / 8, s = tail_slots > 0 ? tail_slots : slots_per_xcd;
  const int c = tail_chunks(n, s, count, tail_force);
  if (c <= 1) return g;
  const int64_t r = c * s;
  g.chunks = c;
  g.n_x = n;
  g.tail0 = n - r;
  g.r_x = r;
  g.tail_need = 8 * r;
  g.tail_cap = 8 * std::max<int64_t>(r, 8 * s);
  // a chunk waits at most for its predecessors' (c - 1) / c of the launch's
  // epochs; one sleep is ~1.7 us and an epoch ~20 us per wave at full
  // occupancy: 64 sleeps per epoch is a wide margin, plus ~2 s of slack
  g.wait_bound = tail_wait_bound(64, count, wait_bound_override);
  g.grid = 8 * (n + (c - 1) * r);
  return g;
}

}  // namespace uwvk
