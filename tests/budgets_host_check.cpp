// Stand-alone check of nekstab_amd/csrc/nsk_budgets_host.hpp: the launch-budget policy and the verdict after a map.
//   budgets_host_check <trace.txt>            properties, verdict table, replay of the recorded trace
//   budgets_host_check --replay <trace.txt>   the replay alone (tests/test_budgets_trace_gpu.py: a trace of the running library)
// The trace is the flat text twin that tests/golden/make_budgets_trace.py writes next to budgets_trace.json.
#include <cstdio>
#include <cstdlib>
#include <fstream>
#include <sstream>
#include <string>
#include <vector>

#include "../nekstab_amd/csrc/nsk_budgets_host.hpp"

using namespace nsk;

static int g_fail = 0;
#define CHECK(cond, ...)                                                    \
  do {                                                                      \
    if (!(cond)) {                                                          \
      ++g_fail;                                                             \
      std::fprintf(stderr, "FAIL %s:%d: %s -- ", __FILE__, __LINE__, #cond); \
      std::fprintf(stderr, __VA_ARGS__);                                    \
      std::fprintf(stderr, "\n");                                           \
    }                                                                       \
  } while (0)

static unsigned g_rng = 12345u;
static int rnd(int n) { g_rng = g_rng * 1664525u + 1013904223u; return (int)((g_rng >> 8) % (unsigned)n); }

static LaunchBudgets fresh(int max_helm = 100, int max_pres = 48, int min_pres = 2) {
  LaunchBudgets lb;
  lb.max_helm = max_helm; lb.max_pres = max_pres; lb.min_pres = min_pres;
  lb.reset_to_caps(true);
  return lb;
}
static long long sum(const std::vector<int>& v) { long long s = 0; for (int x : v) s += x; return s; }

// ---- replay of a recorded trace: the counts of every map into update_class / update_steps, every recorded budget out
static std::vector<long long> ints(std::istringstream& ss) { std::vector<long long> v; long long x; while (ss >> x) v.push_back(x); return v; }

static int replay(const char* path) {
  std::ifstream in(path);
  if (!in) { std::fprintf(stderr, "cannot read %s\n", path); return 1; }
  std::string line, key;
  LaunchBudgets lb;
  int nsteps = 0, tail = 0, net = 0, off_h = 0, off_p = 0, pct = 0, bhead = 0, env_h = 0, env_p = 0, nctx = 0, nmap = 0;
  int kind = 0, nattempt = 0, iattempt = 0;
  long long cum_h = 0, cum_p = 0, sb_maps = 0, retries = 0, rec_sb_maps = 0, rec_h = 0, rec_p = 0, rec_retries = 0;
  std::vector<long long> last, ih;
  while (std::getline(in, line)) {
    std::istringstream ss(line);
    if (!(ss >> key)) continue;
    const std::vector<long long> v = ints(ss);
    if (key == "context") {
      CHECK(v.size() == 13, "context line");
      if (v.size() != 13) return 1;
      lb = fresh((int)v[0], (int)v[1], (int)v[2]);
      nsteps = (int)v[3]; tail = (int)v[4]; net = (int)v[5]; off_h = (int)v[6]; off_p = (int)v[7]; pct = (int)v[8]; bhead = (int)v[9]; env_h = (int)v[10]; env_p = (int)v[11];
      cum_h = cum_p = sb_maps = retries = 0; ++nctx; nmap = 0;
    } else if (key == "map") {
      CHECK(v.size() == 7 && nctx > 0, "map line");
      if (v.size() != 7) return 1;
      kind = (int)v[0]; nattempt = (int)v[1]; rec_sb_maps = v[2]; rec_h = v[3]; rec_p = v[4]; rec_retries = v[5]; iattempt = 0; ++nmap;
      CHECK(nattempt >= 1, "context %d map %d: no attempt recorded", nctx, nmap);
    } else if (key == "attempt") {
      CHECK(v.size() == 1 + 4 * NCLS, "attempt line");
      if (v.size() != 1 + 4 * NCLS) return 1;
      ++iattempt;
      for (int k = 0; k < NCLS; ++k) {          // the class budgets the library held while the attempt ran
        CHECK(lb.cur_helm[k] == v[1 + NCLS + k], "context %d map %d attempt %d: velocity budget of class %d: module %d, library %lld", nctx, nmap, iattempt, k, lb.cur_helm[k], v[1 + NCLS + k]);
        CHECK(lb.cur_pres[k] == v[1 + 3 * NCLS + k], "context %d map %d attempt %d: pressure budget of class %d: module %d, library %lld", nctx, nmap, iattempt, k, lb.cur_pres[k], v[1 + 3 * NCLS + k]);
      }
      MapFacts m;
      m.unconverged = v[0]; m.nsteps = nsteps; m.tail = tail;
      m.per_step = lb.steps_ready(kind, nsteps, false);      // (the recorded contexts replay graphs, option step_budgets on)
      lb.last_per_step = m.per_step; lb.last_kind = kind;
      if (m.per_step) { cum_h += sum(lb.sb[kind].bh); cum_p += sum(lb.sb[kind].bp); ++sb_maps; }
      const Verdict got = lb.verdict(m);
      CHECK(got == (iattempt == nattempt ? Verdict::STANDS : Verdict::REDO), "context %d map %d attempt %d of %d: verdict %d", nctx, nmap, iattempt, nattempt, (int)got);
      if (got == Verdict::REDO) ++retries;
      last = v;
    } else if (key == "iters_h") {
      ih = v;
    } else if (key == "iters_p") {
      CHECK(iattempt == nattempt, "context %d map %d: %d attempts of %d", nctx, nmap, iattempt, nattempt);
      CHECK(sb_maps == rec_sb_maps, "context %d map %d: maps on per-step budgets: module %lld, library %lld", nctx, nmap, sb_maps, rec_sb_maps);
      CHECK(cum_h == rec_h, "context %d map %d: budgeted velocity launches: module %lld, library %lld", nctx, nmap, cum_h, rec_h);
      CHECK(cum_p == rec_p, "context %d map %d: budgeted pressure iterations: module %lld, library %lld", nctx, nmap, cum_p, rec_p);
      CHECK(retries == rec_retries, "context %d map %d: redone maps: module %lld, library %lld", nctx, nmap, retries, rec_retries);
      CHECK(ih.size() == v.size() && (int)v.size() == nsteps && last.size() == 1 + 4 * NCLS, "context %d map %d: record sizes", nctx, nmap);
      if (ih.size() != v.size() || last.size() != 1 + 4 * NCLS) return 1;
      long long mh[NCLS], mp[NCLS];
      for (int k = 0; k < NCLS; ++k) { mh[k] = last[1 + k]; mp[k] = last[1 + 2 * NCLS + k]; }
      std::vector<int> it(2 * v.size());
      for (size_t s = 0; s < v.size(); ++s) { it[2 * s] = (int)ih[s]; it[2 * s + 1] = (int)v[s]; }
      lb.update_class(mh, mp, nsteps, false, bhead);
      lb.update_steps(kind, it.data(), (int)v.size(), nsteps, net != 0, tail, off_h, off_p, pct, env_h, env_p);
    } else {
      CHECK(false, "unknown line '%s'", key.c_str());
      return 1;
    }
  }
  CHECK(nctx >= 1 && nmap >= 1, "empty trace");
  std::printf("replay: %d contexts, last one %d maps\n", nctx, nmap);
  return 0;
}

// ---- the properties the comments of the module promise
static void feed_class(LaunchBudgets& lb, const int* h, const int* p, int nsteps, int bhead = 3) {
  long long mh[NCLS], mp[NCLS];
  for (int k = 0; k < NCLS; ++k) { mh[k] = h[k]; mp[k] = p[k]; }
  lb.update_class(mh, mp, nsteps, false, bhead);
}

static void class_properties() {
  for (int trial = 0; trial < 40; ++trial) {
    LaunchBudgets lb = fresh(60 + rnd(60), 20 + rnd(40), rnd(3));
    const int nsteps = 1 + rnd(40), bhead = rnd(5);
    if (trial % 5 == 4) { lb.set_all(false, false, 1 + rnd(10)); lb.set_all(true, false, 1 + rnd(10)); }      // start-up budgets below the counts
    for (int map = 0; map < 30; ++map) {
      int h[NCLS], p[NCLS];
      const int lvl = map < 15 ? 40 : 8;          // a cheap stretch behind an expensive one: the window must empty before budgets fall
      for (int k = 0; k < NCLS; ++k) { h[k] = rnd(lvl + (map % 7 == 0 ? 100 : 0)); p[k] = rnd(lvl); }      // (some counts beyond the caps)
      const ClassBudgets before = lb.save();
      feed_class(lb, h, p, nsteps, bhead);
      const bool full = lb.bh_n >= LaunchBudgets::BW;
      for (int k = 0; k < NCLS; ++k) {
        CHECK(lb.cur_helm[k] >= 1 && lb.cur_helm[k] <= lb.max_helm && lb.cur_pres[k] >= 1 && lb.cur_pres[k] <= lb.max_pres, "class %d out of [1, cap]: %d %d", k, lb.cur_helm[k], lb.cur_pres[k]);
        if (CLS_ISTEP[k] > nsteps) {              // a class the map does not run keeps its budgets
          CHECK(lb.cur_helm[k] == before.helm[k] && lb.cur_pres[k] == before.pres[k], "class %d beyond nsteps %d changed", k, nsteps);
          continue;
        }
        // a larger count grows the budget at once: it covers the count + head-room (or sits at the cap)
        CHECK(lb.cur_helm[k] >= std::min(lb.max_helm, h[k] + bhead), "class %d: velocity budget %d below count %d + %d", k, lb.cur_helm[k], h[k], bhead);
        CHECK(lb.cur_pres[k] >= std::min(lb.max_pres, p[k] + bhead), "class %d: pressure budget %d below count %d + %d", k, lb.cur_pres[k], p[k], bhead);
        // it shrinks only when the window is full, or (long classes) when it exceeded twice the request
        if (lb.cur_helm[k] < before.helm[k]) CHECK(full || (k >= 4 && before.helm[k] > 2 * lb.cur_helm[k]), "class %d: velocity budget cut %d -> %d with %d maps", k, before.helm[k], lb.cur_helm[k], lb.bh_n);
        if (lb.cur_pres[k] < before.pres[k]) CHECK(full || (k >= 4 && before.pres[k] > 2 * lb.cur_pres[k]), "class %d: pressure budget cut %d -> %d with %d maps", k, before.pres[k], lb.cur_pres[k], lb.bh_n);
      }
    }
  }
  // frozen budgets stay; the persistent velocity solve keeps its velocity budgets
  LaunchBudgets lb = fresh();
  lb.set_all(false, false, 20); lb.set_all(true, false, 10); lb.freeze = 1;
  const int big[NCLS] = {50, 50, 50, 50, 50, 50};
  feed_class(lb, big, big, 20);
  CHECK(lb.cur_helm[0] == 20 && lb.cur_pres[5] == 10 && lb.bh_n == 0, "frozen budgets moved");
  lb.freeze = 0;
  long long m[NCLS] = {30, 30, 30, 30, 30, 30};
  lb.update_class(m, m, 20, true, 3);
  CHECK(lb.cur_helm[2] == 20 && lb.cur_pres[2] > 30, "fused: velocity budget moved or pressure budget did not");
  // options, save / restore / at_least, back to the caps
  lb = fresh(100, 48, 0);
  lb.set_all(false, false, 500); CHECK(lb.cur_helm[3] == 100, "budget_helm above the cap");
  lb.set_all(true, false, -3); CHECK(lb.cur_pres[3] == 1, "budget_pres below 1");
  lb.set_all(true, true, 6); CHECK(lb.cur_pres[0] == 7, "budget_add_pres");
  lb.set_all(false, true, -40); CHECK(lb.cur_helm[5] == 60, "budget_add_helm");
  const ClassBudgets s = lb.save();
  lb.set_all(false, false, 10); lb.set_all(true, false, 20);
  lb.at_least(s); CHECK(lb.cur_helm[1] == 60 && lb.cur_pres[1] == 20, "at_least");
  lb.restore(s); CHECK(lb.cur_helm[1] == 60 && lb.cur_pres[1] == 7, "restore");
  lb.bh_n = 5; lb.reset_to_caps(false); CHECK(lb.cur_helm[4] == 100 && lb.cur_pres[4] == 48 && lb.bh_n == 5, "reset_to_caps(false)");
  lb.reset_to_caps(true); CHECK(lb.bh_n == 0, "reset_to_caps(true)");
}

static std::vector<int> random_iters(int ns, int lvl_h, int lvl_p) {
  std::vector<int> it(2 * ns);
  for (int s = 0; s < ns; ++s) { it[2 * s] = rnd(lvl_h); it[2 * s + 1] = rnd(lvl_p); }
  return it;
}

static void step_properties() {
  // every mode, every window fill, short and long maps, percentiles from 50 to 100 (the sanitizers watch the scratch arrays)
  for (int net = 0; net <= 1; ++net)
    for (int tail = 0; tail <= 2; ++tail)
      for (int ns : {3, 4, 7, 20, 61})
        for (int pct : {0, 50, 77, 90, 99, 100, 250}) {
          LaunchBudgets lb = fresh(100, 48, 2);
          const int off_h = tail == 1 ? -rnd(4) : rnd(3), off_p = tail == 1 ? -rnd(3) : rnd(3);
          for (int map = 0; map < 2 * LaunchBudgets::SBW + 3; ++map) {
            const std::vector<int> it = random_iters(ns, map % 5 == 0 ? 140 : 30, map % 4 == 0 ? 70 : 12);
            lb.update_steps(map % 2, it.data(), ns, ns, net != 0, tail, off_h, off_p, pct, -1, -1);
            const LaunchBudgets::StepBudgets& b = lb.sb[map % 2];
            CHECK((int)b.bh.size() == ns && (int)b.bp.size() == ns, "budget sizes");
            const bool heads = net && tail == 1;
            const int head_h = (net ? 1 : 3) + std::max(0, off_h), head_p = (net ? 0 : 2) + std::max(0, off_p);
            const int nv = std::min(b.n, LaunchBudgets::SBW);
            const bool largest = !heads && !(net && nv >= 4 && pct < 100);      // the budget covers the largest count of the window
            for (int s = 0; s < ns; ++s) {
              CHECK(b.bh[s] >= 1 && b.bh[s] <= lb.max_helm && b.bp[s] >= (heads ? 0 : lb.min_pres) && b.bp[s] <= lb.max_pres, "step %d out of range: %d %d", s, b.bh[s], b.bp[s]);
              if (largest) {                      // a larger count grows the budget at once
                CHECK(b.bh[s] >= std::min(lb.max_helm, it[2 * s] + head_h), "step %d: velocity budget %d below count %d + %d", s, b.bh[s], it[2 * s], head_h);
                CHECK(b.bp[s] >= std::min(lb.max_pres, it[2 * s + 1] + head_p), "step %d: pressure budget %d below count %d + %d", s, b.bp[s], it[2 * s + 1], head_p);
              }
            }
            CHECK(lb.steps_ready(map % 2, ns, false) && !lb.steps_ready(map % 2, ns + 1, false) && !lb.steps_ready(map % 2, ns, true) && !lb.steps_ready(2, ns, false), "steps_ready");
          }
        }
  // heads behind persistent tails (tail = 1): the median of the window + 1 (velocity) / + 0 (pressure), + the offsets
  {
    LaunchBudgets lb = fresh(100, 48, 2);
    const int hist[5][3][2] = {{{9, 4}, {20, 0}, {7, 7}}, {{11, 2}, {22, 1}, {7, 9}}, {{30, 8}, {2, 5}, {7, 8}}, {{10, 3}, {21, 2}, {99, 47}}, {{12, 6}, {23, 3}, {99, 48}}};
    for (int map = 0; map < 5; ++map) lb.update_steps(0, &hist[map][0][0], 3, 3, true, 1, 0, 0, 90, -1, -1);
    // sorted: step 0: 9 10 11 12 30 / 2 3 4 6 8; step 1: 2 20 21 22 23 / 0 1 2 3 5; step 2: 7 7 7 99 99 / 7 8 9 47 48
    const int want_h[3] = {12, 22, 8}, want_p[3] = {4, 2, 9};
    for (int s = 0; s < 3; ++s) CHECK(lb.sb[0].bh[s] == want_h[s] && lb.sb[0].bp[s] == want_p[s], "median heads, step %d: %d %d", s, lb.sb[0].bh[s], lb.sb[0].bp[s]);
    lb.update_steps(0, &hist[0][0][0], 3, 3, true, 1, -6, -3, 90, -1, -1);      // six maps: the upper median; offsets below the counts
    // sorted: step 0: 9 9 10 11 12 30 / 2 3 4 4 6 8; step 2: 7 7 7 7 99 99 / 7 7 8 9 47 48
    CHECK(lb.sb[0].bh[0] == 11 + 1 - 6 && lb.sb[0].bp[0] == 4 - 3 && lb.sb[0].bh[2] == 7 + 1 - 6 && lb.sb[0].bp[2] == 9 - 3, "median heads with offsets");
    CHECK(lb.sb[0].bp[1] == 0 && lb.sb[0].bh[1] >= 1, "heads: floors 1 / 0");
    CHECK(lb.sb[1].bh.empty() && lb.sb[1].n == 0, "the adjoint history is its own");
  }
  // the plain rule by hand: one map, no tail: largest count at s-2..s+2 + 3 / + 2, + the margins of steps 1-6 and of the first maps
  {
    LaunchBudgets lb = fresh(100, 48, 2);
    std::vector<int> it(2 * 10);
    for (int s = 0; s < 10; ++s) { it[2 * s] = 20 - s; it[2 * s + 1] = s == 8 ? 0 : 5; }
    lb.update_steps(1, it.data(), 10, 10, false, 0, 0, 0, 90, -1, -1);
    CHECK(lb.sb[1].bh[9] == 13 + 3 + std::max(2, 13 / 4) && lb.sb[1].bp[9] == 5 + 2 + std::max(3, 5 / 2), "plain rule, last step: %d %d", lb.sb[1].bh[9], lb.sb[1].bp[9]);
    CHECK(lb.sb[1].bh[0] == 20 + 3 + 10 + 5 && lb.sb[1].bp[0] == 5 + 2 + 5 + 3, "plain rule, first step: %d %d", lb.sb[1].bh[0], lb.sb[1].bp[0]);
    LaunchBudgets e = fresh(100, 48, 2);          // head-rooms from the environment replace the defaults
    e.update_steps(1, it.data(), 10, 10, false, 0, 0, 0, 90, 0, 7);
    CHECK(e.sb[1].bh[9] == lb.sb[1].bh[9] - 3 && e.sb[1].bp[9] == lb.sb[1].bp[9] + 5, "head-rooms from the environment");
  }
  // nsteps changing between maps restarts the history; no record, a short record or a short map clears the budgets
  {
    LaunchBudgets lb = fresh(100, 48, 2), one = fresh(100, 48, 2);
    for (int map = 0; map < 5; ++map) { const std::vector<int> it = random_iters(10, 60, 30); lb.update_steps(0, it.data(), 10, 10, true, 2, 0, 0, 90, -1, -1); }
    const std::vector<int> it = random_iters(12, 10, 5);
    lb.update_steps(0, it.data(), 12, 12, true, 2, 0, 0, 90, -1, -1);
    one.update_steps(0, it.data(), 12, 12, true, 2, 0, 0, 90, -1, -1);
    CHECK(lb.sb[0].n == 1 && lb.sb[0].bh == one.sb[0].bh && lb.sb[0].bp == one.sb[0].bp, "history not restarted when nsteps changed");
    lb.update_steps(0, it.data(), 12, 13, true, 2, 0, 0, 90, -1, -1);
    CHECK(lb.sb[0].bh.empty() && lb.sb[0].bp.empty() && !lb.steps_ready(0, 12, false), "a record shorter than the map kept its budgets");
    lb.update_steps(0, it.data(), 12, 12, true, 2, 0, 0, 90, -1, -1);
    CHECK(lb.steps_ready(0, 12, false), "budgets not back");
    lb.update_steps(0, nullptr, 12, 12, true, 2, 0, 0, 90, -1, -1);
    CHECK(lb.sb[0].bh.empty(), "no record kept its budgets");
    lb.update_steps(0, it.data(), 2, 2, true, 2, 0, 0, 90, -1, -1);
    CHECK(lb.sb[0].bh.empty(), "a two-step map got budgets");
    lb.update_steps(0, it.data(), 12, 12, true, 2, 0, 0, 90, -1, -1);
    lb.freeze = 1; CHECK(!lb.steps_ready(0, 12, false), "frozen budgets: per-step budgets ready"); lb.freeze = 0;
    lb.force_class = true; CHECK(!lb.steps_ready(0, 12, false), "forced class budgets: per-step budgets ready"); lb.force_class = false;
    lb.forget_steps(); CHECK(lb.sb[0].n == 0 && lb.sb[0].bh.empty() && lb.sb[1].bp.empty(), "forget_steps");
  }
}

// ---- the verdict: every combination of the counters and of how the attempt ran, against the order of precedence stated here
static void verdict_table() {
  for (int bits = 0; bits < 256; ++bits) {
    MapFacts m;
    m.unconverged = (bits & 1) ? 3 : 0; m.nonfinite = (bits & 2) ? 1 : 0; m.allred_mismatch = (bits & 4) ? 2 : 0; m.sync_timeouts = (bits & 8) ? 1 : 0;
    m.per_step = bits & 16; m.hostchecked = bits & 32; m.fused = bits & 64;
    m.tail = (bits & 128) ? 2 : 0; m.nsteps = 20;
    for (int at_caps = 0; at_caps <= 1; ++at_caps) {
      LaunchBudgets lb = fresh(100, 48, 2);
      if (!at_caps) { lb.set_all(false, false, 30); lb.set_all(true, false, 10); }
      lb.force_class = (bits & 1) == 0;            // (STANDS clears it, an overflowed per-step budget sets it)
      const ClassBudgets before = lb.save();
      Verdict want;
      bool grown = false;
      if (m.allred_mismatch) want = Verdict::FAIL_COMM;
      else if (m.sync_timeouts) want = (m.per_step && m.tail != 0 && !m.fused) ? Verdict::TAILS_OFF_REDO : Verdict::FAIL_SYNC;
      else if (m.nonfinite) want = Verdict::FAIL_NAN;
      else if (!m.unconverged) want = Verdict::STANDS;
      else if (m.per_step) want = Verdict::REDO;
      else if (m.hostchecked || at_caps) want = Verdict::FAIL_NOCONV;
      else { want = Verdict::REDO; grown = true; }
      const bool force_before = lb.force_class;
      const Verdict got = lb.verdict(m);
      CHECK(got == want, "facts %d, at caps %d: verdict %d, expected %d", bits, at_caps, (int)got, (int)want);
      for (int k = 0; k < NCLS; ++k) {
        CHECK(lb.cur_helm[k] == (grown ? std::min(100, 2 * before.helm[k] + 4) : before.helm[k]), "facts %d: velocity budget of class %d", bits, k);
        CHECK(lb.cur_pres[k] == (grown ? std::min(48, 2 * before.pres[k] + 4) : before.pres[k]), "facts %d: pressure budget of class %d", bits, k);
      }
      const bool force_want = want == Verdict::STANDS ? false : (want == Verdict::REDO && m.per_step ? true : force_before);
      CHECK(lb.force_class == force_want, "facts %d: force_class %d", bits, (int)lb.force_class);
    }
  }
  // Growth and "at the caps" range over the classes the map runs.  The regression: classes 0-3 at the caps, classes 4-5
  // below (a longer map shrank them), a 6-step map with an unconverged solve.  The rule before this module judged "capped" over
  // ALL six classes -- never true here -- and (on shards) doubled only classes 0-3 -- already at the caps: the same map on
  // the same budgets, redone for ever; on one rank classes 4-5 doubled several times for nothing before the failure was reported.
  LaunchBudgets lb = fresh(100, 48, 2);
  lb.cur_helm[4] = 20; lb.cur_pres[4] = 9; lb.cur_helm[5] = 15; lb.cur_pres[5] = 7;
  MapFacts m;
  m.unconverged = 2; m.nsteps = 6;
  CHECK(lb.verdict(m) == Verdict::FAIL_NOCONV, "short map at its caps: not reported");
  CHECK(lb.cur_helm[4] == 20 && lb.cur_pres[5] == 7, "short map at its caps: absent classes grown");
  m.nsteps = 7;                                     // class 4 runs: there is room, and only the classes that run grow
  CHECK(lb.verdict(m) == Verdict::REDO && lb.cur_helm[4] == 44 && lb.cur_pres[4] == 22 && lb.cur_helm[5] == 15 && lb.cur_pres[5] == 7, "7-step map: growth of the classes it runs");
  int redo = 0;
  while (lb.verdict(m) == Verdict::REDO && redo < 100) ++redo;      // every redo grows a budget the map uses: the chain ends
  CHECK(redo < 4 && lb.cur_helm[4] == 100 && lb.cur_pres[4] == 48 && lb.cur_helm[5] == 15, "redo chain of a 7-step map: %d", redo);
  m.nsteps = 2;
  lb = fresh(100, 48, 2);
  for (int k = 2; k < NCLS; ++k) { lb.cur_helm[k] = 5; lb.cur_pres[k] = 5; }
  CHECK(lb.verdict(m) == Verdict::FAIL_NOCONV, "two-step map at its caps");
}

int main(int argc, char** argv) {
  const bool only_replay = argc > 2 && std::string(argv[1]) == "--replay";
  const char* trace = argc > 1 ? argv[argc - 1] : nullptr;
  if (!trace) { std::fprintf(stderr, "usage: budgets_host_check [--replay] <trace.txt>\n"); return 2; }
  static_assert(step_class(1) == 0 && step_class(3) == 2 && step_class(4) == 3 && step_class(6) == 3 && step_class(7) == 4 && step_class(16) == 4 && step_class(17) == 5, "step classes");
  for (int k = 0; k < NCLS; ++k) CHECK(step_class(CLS_ISTEP[k]) == k && (k == 0 || step_class(CLS_ISTEP[k] - 1) == k - 1), "CLS_ISTEP[%d]", k);
  if (!only_replay) { class_properties(); step_properties(); verdict_table(); }
  if (replay(trace)) ++g_fail;
  if (g_fail) { std::fprintf(stderr, "budgets_host_check: %d failures\n", g_fail); return 1; }
  std::printf("budgets_host_check ok\n");
  return 0;
}
