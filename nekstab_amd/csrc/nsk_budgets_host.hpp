// Launch budgets and the verdict after a map: the host policy between two maps, free of HIP and of nsk_ctx so that a plain
// CPU program can check it (tests/budgets_host_check.cpp, built under AddressSanitizer and UBSan by tests/test_budgets_host.py).
//
// Every velocity (CG) and pressure (GMRES) solve of a time step is queued as a fixed number of launches, its launch budget:
// one pair per step CLASS, and on graph-replayed single-rank contexts one pair per TIME STEP.  A solve that runs out of
// launches is counted on the device (Stats::unconverged); LaunchBudgets::verdict says what becomes of the attempt, and
// update_class / update_steps adapt the budgets behind an attempt that stands.
#pragma once
#include <algorithm>
#include <cmath>
#include <vector>

#ifdef __HIPCC__
#define NSK_HOST_DEVICE __host__ __device__
#else
#define NSK_HOST_DEVICE
#endif

namespace nsk {

// Step classes: one captured hipGraph and one launch budget each.  Time steps 1, 2, 3 differ in BDF/EXT order and
// in how much of the input's divergence they remove; steps 4-6 and 7-16 still carry that transient.  Cutting the
// tail (>= 17) further does not pay: its per-class iteration maxima are the same (measured with 8 classes).
constexpr int NCLS = 6;
constexpr int CLS_ISTEP[NCLS] = {1, 2, 3, 4, 7, 17};    // first step of every class
NSK_HOST_DEVICE constexpr int step_class(int istep) {
  return istep <= 3 ? istep - 1 : (istep <= 6 ? 3 : (istep <= 16 ? 4 : 5));
}

// what a map driver does with the attempt it just ran
enum class Verdict {
  STANDS,           // converged everywhere: the caller adapts the budgets (update_class, update_steps)
  REDO,             // a solve ran out of launches: redo the map (the budgets have grown, or the redo takes the class budgets)
  FAIL_NAN,         // non-finite state inside the map
  FAIL_COMM,        // a verified all-reduce differed between the ranks
  FAIL_NOCONV,      // a solve ran out of launches AT the caps
  FAIL_SYNC,        // a grid barrier of a persistent kernel gave up
  TAILS_OFF_REDO,   // ... of a persistent TAIL: the caller switches the tails off for good and redoes the map
};

// the facts of one attempt (counters of Stats, and how the attempt ran)
struct MapFacts {
  long long unconverged = 0, nonfinite = 0, allred_mismatch = 0, sync_timeouts = 0;
  bool per_step = false;          // it took the per-step budgets
  bool hostchecked = false;       // host-checked eager steps: they iterate to the caps whatever the budgets say
  int nsteps = 0;
  bool fused = false;             // persistent velocity solve (one launch per step: no velocity budget)
  int tail = 0;                   // option "tail"
};

struct ClassBudgets { int helm[NCLS] = {}, pres[NCLS] = {}; };       // a saved set (0: none yet)

struct LaunchBudgets {
  static constexpr int BW = 8;             // maps in the window of the class budgets
  static constexpr int SBW = 8, SBN = 2;   // maps in the window of the per-step budgets / steps to either side
  int max_helm = 60, max_pres = 40, min_pres = 0;       // the solvers' caps (min_pres: option "min_pres_iter")
  int cur_helm[NCLS] = {}, cur_pres[NCLS] = {};         // launch budgets per step class
  int bh_helm[NCLS][BW] = {}, bh_pres[NCLS][BW] = {}, bh_n = 0;      // iteration maxima of the last maps (update_class)
  int freeze = 0;                          // option "budget_freeze": the budgets stay where the caller put them
  struct StepBudgets {                     // one history per kind of map (0 direct, 1 adjoint): their solves differ
    std::vector<int> hist_h[SBW], hist_p[SBW];
    int n = 0;                             // maps in the history (ring slot = n % SBW)
    std::vector<int> bh, bp;               // budgets of the next map of this kind (empty: class budgets)
  } sb[2];
  int last_kind = 0;                       // kind of the map just run
  bool last_per_step = false;              // ... and whether it took the per-step budgets
  bool force_class = false;                // the redo of an overflowed map runs on the class budgets

  // back to full budgets: the caps, as a new context has them (clear_history: the window of the class budgets too)
  void reset_to_caps(bool clear_history) {
    for (int k = 0; k < NCLS; ++k) { cur_helm[k] = max_helm; cur_pres[k] = max_pres; }
    if (clear_history) bh_n = 0;
  }
  void forget_steps() { for (auto& b : sb) { b.n = 0; b.bh.clear(); b.bp.clear(); } }      // the per-step history (a new operator: its solves behave differently)

  ClassBudgets save() const {
    ClassBudgets s;
    for (int k = 0; k < NCLS; ++k) { s.helm[k] = cur_helm[k]; s.pres[k] = cur_pres[k]; }
    return s;
  }
  void restore(const ClassBudgets& s) { for (int k = 0; k < NCLS; ++k) { cur_helm[k] = s.helm[k]; cur_pres[k] = s.pres[k]; } }
  void at_least(const ClassBudgets& s) { for (int k = 0; k < NCLS; ++k) { cur_helm[k] = std::max(cur_helm[k], s.helm[k]); cur_pres[k] = std::max(cur_pres[k], s.pres[k]); } }

  // options "budget_helm" / "budget_pres" (add = false) and "budget_add_helm" / "budget_add_pres": every class, within [1, cap]
  void set_all(bool pres, bool add, int v) {
    int* cur = pres ? cur_pres : cur_helm;
    const int cap = pres ? max_pres : max_helm;
    for (int k = 0; k < NCLS; ++k) cur[k] = std::min(cap, std::max(1, (add ? cur[k] : 0) + v));
  }

  // the next map of `kind` runs on per-step budgets (the caller adds what it alone knows: the option, the device record)
  bool steps_ready(int kind, int nsteps, bool fused) const {
    if (kind < 0 || kind > 1) return false;
    return !force_class && !fused && !freeze && (int)sb[kind].bh.size() == nsteps && (int)sb[kind].bp.size() == nsteps;
  }

  // Launch budgets of the step classes from the iteration maxima of the maps run so far.  The maxima of one
  // class move by +-3 between consecutive Krylov vectors; budgets that follow the last map alone are cut after a
  // cheap map, the next map runs out of launches and is redone as a whole (measured on cfg 2: 29 redone maps and
  // 449 graph re-captures in 130 maps).  So: a window of the last BW maps; grow at once; shrink to the window
  // maximum + head-room only when the window is full, or when the budget is more than twice what the window asks
  // for (start-up budgets, doubled budgets after a redone map).  bhead: head-room above the window maximum.
  void update_class(const long long* max_helm_k, const long long* max_pres_k, int nsteps, bool fused, int bhead) {
    if (freeze) return;
    const int slot = bh_n % BW;
    for (int k = 0; k < NCLS; ++k) { bh_helm[k][slot] = (int)max_helm_k[k]; bh_pres[k][slot] = (int)max_pres_k[k]; }
    bh_n++;
    const int nv = std::min(bh_n, BW);
    for (int k = 0; k < NCLS; ++k) {
      if (CLS_ISTEP[k] > nsteps) break;
      int mh = 0, mp = 0;
      for (int i = 0; i < nv; ++i) { mh = std::max(mh, bh_helm[k][i]); mp = std::max(mp, bh_pres[k][i]); }
      // the classes of time steps 1..6 hold one to three steps per map and their counts vary most (pressure
      // solves of steps 2-3: 4 to 23 iterations): spare launches there cost microseconds, a redone map 0.1 s
      const int xh = k <= 3 ? std::max(4, mh / 2) : (k == 4 ? 1 : 0), xp = k <= 3 ? std::max(4, mp) : (k == 4 ? 1 : 0);
      // the first maps of a run differ most from one another (noise seed, empty projection space): wider margin
      const int sh = nv < 4 ? std::max(2, mh / 4) : 0, sp = nv < 4 ? std::max(4, mp) : 0;
      const int th = std::min(max_helm, mh + bhead + xh + sh), tp = std::min(max_pres, mp + bhead + xp + sp);
      // before the window is full only the long classes are cut (their spare launches are what costs); the classes of
      // steps 1-6 keep what they have: the second Krylov vector of a run can need 34 pressure iterations where the
      // noise seed needed 4
      const bool early = nv < BW && k >= 4;
      if (!fused && (th > cur_helm[k] || (nv == BW ? th < cur_helm[k] - 1 : (early && cur_helm[k] > 2 * th)))) cur_helm[k] = th;   // fused: the solve ends on the device
      if (tp > cur_pres[k] || (nv == BW ? tp < cur_pres[k] - 1 : (early && cur_pres[k] > 2 * tp))) cur_pres[k] = tp;
    }
  }

  // Per-step budgets of the NEXT map of `kind` from the per-step iteration counts of the last SBW maps.  iters: [2 * ns], the
  // velocity and pressure counts of every time step of the map just run (null: no record, or the option is off); ns: the
  // steps it holds, nsteps: the steps of a map.
  // Helmholtz: launches = largest count at steps s-SBN..s+SBN + 3 (a solve that took I iterations needs I + 1 launches: 2 spare);
  // pressure: + 2.  Steps 1-6 and the first maps of a run vary most (the class budgets' rule): wider margins there.
  // net: a persistent tail runs behind the budgets; tail: option "tail" (1: the budgets are HEADS); off_h / off_p: options
  // "tail_off_h" / "tail_off_p"; pct: option "sb_pct"; env_h / env_p: head-rooms from the environment (< 0: the defaults).
  void update_steps(int kind, const int* iters, int ns, int nsteps, bool net, int tail, int off_h, int off_p, int pct_opt, int env_h, int env_p) {
    if (kind < 0 || kind > 1) return;
    StepBudgets& b = sb[kind];
    if (!iters || ns != nsteps || ns < 3) { b.bh.clear(); b.bp.clear(); return; }
    if (b.n > 0 && (int)b.hist_h[0].size() != ns) b.n = 0;                     // (nsteps changed under us: start again)
    const int slot = b.n % SBW;
    b.hist_h[slot].resize(ns); b.hist_p[slot].resize(ns);
    for (int s = 0; s < ns; ++s) { b.hist_h[slot][s] = iters[2 * s]; b.hist_p[slot][s] = iters[2 * s + 1]; }
    b.n++;
    const int nv = std::min(b.n, SBW);
    b.bh.assign(ns, 0); b.bp.assign(ns, 0);
    // (net, tail = 2: the budgets below + a persistent tail behind them as a SAFETY NET: a solve that outruns its budget continues
    //  in the tail instead of costing a redone map)
    // (options "tail_off_h" / "tail_off_p" > 0 add to the head-room of the plain budgets too: tests use it for a reference run that cannot overflow)
    const int head_h = (env_h >= 0 ? env_h : (net ? 1 : 3)) + std::max(0, off_h), head_p = (env_p >= 0 ? env_p : (net ? 0 : 2)) + std::max(0, off_p);
    if (net && tail == 1) {
      // HEADS for the persistent tails: the MEDIAN count of this step over the window (offline on 56 maps of config 2: the cheapest
      // predictor, 0.44 launches that find nothing to do and 0.56 tail iterations per pressure solve; profiles/r05_step_budgets.txt).
      // Velocity: a solve of I iterations is found finished by launch I (0-based), i.e. I + 1 launches.
      int vh[SBW], vp[SBW];
      for (int s = 0; s < ns; ++s) {
        for (int i = 0; i < nv; ++i) { vh[i] = b.hist_h[i][s]; vp[i] = b.hist_p[i][s]; }
        std::sort(vh, vh + nv); std::sort(vp, vp + nv);
        const int mh = vh[nv / 2], mp = vp[nv / 2];
        b.bh[s] = std::max(1, std::min(max_helm - 1, mh + 1 + off_h));
        b.bp[s] = std::max(0, std::min(max_pres, mp + off_p));
      }
      return;
    }
    // (option "sb_pct" < 100, with the safety-net tail only: the budget is that PERCENTILE of the counts at steps s-1..s+1 of the window
    //  instead of the largest at s-2..s+2 -- fewer launches that find nothing to do, more solves that end in the tail; offline on the
    //  recorded counts of 64 maps the 85th-90th percentile is the cheapest: DESIGN.md section 7)
    const int pct = (net && nv >= 4) ? std::max(50, std::min(100, pct_opt)) : 100;
    const int win = pct < 100 ? 1 : SBN;
    for (int s = 0; s < ns; ++s) {
      int mh = 0, mp = 0;
      if (pct < 100) {
        int vh[SBW * 3], vp[SBW * 3], n = 0;
        for (int i = 0; i < nv; ++i)
          for (int t = std::max(0, s - win); t <= std::min(ns - 1, s + win); ++t) { vh[n] = b.hist_h[i][t]; vp[n] = b.hist_p[i][t]; ++n; }
        std::sort(vh, vh + n); std::sort(vp, vp + n);
        const int k = std::min(n - 1, (int)std::ceil(0.01 * pct * (n - 1)));
        mh = vh[k]; mp = vp[k];
      } else
        for (int i = 0; i < nv; ++i)
          for (int t = std::max(0, s - SBN); t <= std::min(ns - 1, s + SBN); ++t) { mh = std::max(mh, b.hist_h[i][t]); mp = std::max(mp, b.hist_p[i][t]); }
      int xh = 0, xp = 0;
      if (s < 6) { xh = std::max(4, mh / 2); xp = std::max(4, mp); }                    // time steps 1-6: counts vary most (noise left by the input vector)
      if (nv < 4 && !net) { xh += std::max(2, mh / 4); xp += std::max(3, mp / 2); }    // first maps of a run: noise seed, empty projection space (with the safety-net tail an early overflow costs a tail iteration, not a map)
      b.bh[s] = std::min(max_helm, mh + head_h + xh);
      b.bp[s] = std::min(max_pres, std::max(min_pres, mp) + head_p + xp);
    }
  }

  // The one decision behind a map attempt, for single-rank contexts and shards.  An attempt with a solve that ran out of
  // launches is redone: on the class budgets as they stand when a PER-STEP budget overflowed (they cover the class maxima of
  // the last maps), else with the class budgets doubled (+ 4).  "At the caps" and the doubling both range over the classes
  // the map RUNS (CLS_ISTEP[k] <= nsteps): a short map cannot be redone for ever on budgets that only its absent classes
  // could still grow.  The growth happens here; error codes, messages and side effects (solver state, graphs, counters) are
  // the caller's.
  Verdict verdict(const MapFacts& m) {
    if (m.allred_mismatch) return Verdict::FAIL_COMM;        // (exact integer sums: every rank reaches this verdict together)
    if (m.sync_timeouts) return (!m.fused && m.tail != 0 && m.per_step) ? Verdict::TAILS_OFF_REDO : Verdict::FAIL_SYNC;
    if (m.nonfinite) return Verdict::FAIL_NAN;
    if (m.unconverged == 0) { force_class = false; return Verdict::STANDS; }
    if (m.per_step) { force_class = true; return Verdict::REDO; }
    bool capped = true;                                       // the budgets the map just ran with: test before growing
    for (int k = 0; k < NCLS && CLS_ISTEP[k] <= m.nsteps; ++k) capped = capped && cur_helm[k] >= max_helm && cur_pres[k] >= max_pres;
    // (host-checked: redoing the map with doubled budgets the mode ignores would only repeat it)
    if (capped || m.hostchecked) return Verdict::FAIL_NOCONV;
    for (int k = 0; k < NCLS && CLS_ISTEP[k] <= m.nsteps; ++k) {
      cur_helm[k] = std::min(max_helm, 2 * cur_helm[k] + 4);
      cur_pres[k] = std::min(max_pres, 2 * cur_pres[k] + 4);
    }
    return Verdict::REDO;
  }
};

}  // namespace nsk
