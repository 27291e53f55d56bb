// Host steps of the set-up that build (quadrilaterals), build3 (hexahedra) and shard_fill share: the gather-scatter tables
// every gather kernel trusts, the spacing table of the CFL rule, the section timer.  Standard library only (no HIP header), so a
// CPU program can compile and check them: tests/setup_host_check.cpp.
#pragma once
#include <algorithm>
#include <array>
#include <chrono>
#include <cstdio>
#include <cstdlib>
#include <utility>
#include <vector>

namespace nsk_setup {
namespace {        // internal linkage: the including library exports none of this

// (gid, local index) pairs into ascending (gid, index) order.  The pairs arrive in ascending index, so a counting sort on the
// gid is stable and O(n): 1 s instead of the 6 s std::sort takes on the 1e8 nodes of config 5.  Sparse numberings (a rank's
// sub-mesh keeps the global ids) fall back to the comparison sort when the id range is more than 8x the node count.
inline void sort_gid_pairs(std::vector<std::pair<long long, int>>& srt) {
  const size_t n = srt.size();
  long long mx = -1;
  bool neg = false;
  for (const auto& p : srt) { mx = std::max(mx, p.first); neg = neg || p.first < 0; }
  if (neg || mx + 1 > 8 * (long long)n + 1024) { std::sort(srt.begin(), srt.end()); return; }
  std::vector<unsigned> start((size_t)mx + 2, 0u);
  for (const auto& p : srt) start[(size_t)p.first + 1]++;
  for (size_t g = 0; g + 1 < start.size(); ++g) start[g + 1] += start[g];
  std::vector<std::pair<long long, int>> out(n);
  for (const auto& p : srt) out[start[(size_t)p.first]++] = p;
  srt.swap(out);
}

// gather-scatter CSR of a numbering: the list of node l, gs_idx[gs_off[l] .. gs_off[l + 1]), holds every node with l's id in
// ascending local index (l itself among them)
inline void gs_csr(const long long* gid, long long nloc, std::vector<int>& gs_off, std::vector<int>& gs_idx) {
  std::vector<std::pair<long long, int>> srt(nloc);
  for (long long l = 0; l < nloc; ++l) srt[l] = {gid[l], (int)l};
  sort_gid_pairs(srt);
  std::vector<int> grp_start(nloc), grp_cnt(nloc);
  for (long long a = 0; a < nloc;) {
    long long b = a;
    while (b < nloc && srt[b].first == srt[a].first) ++b;
    for (long long k = a; k < b; ++k) { grp_start[srt[k].second] = (int)a; grp_cnt[srt[k].second] = (int)(b - a); }
    a = b;
  }
  gs_off.assign(nloc + 1, 0);
  for (long long l = 0; l < nloc; ++l) gs_off[l + 1] = gs_off[l] + grp_cnt[l];
  gs_idx.resize(gs_off[nloc]);
  for (long long l = 0; l < nloc; ++l)
    for (int k = 0; k < grp_cnt[l]; ++k) gs_idx[gs_off[l] + k] = srt[grp_start[l] + k].second;
}

// one row of the four-integer gather table (Dev::gs_tab): a list of at most 4 entries, -1 padded; a longer one is marked -2
// (the kernels then walk the CSR arrays)
inline std::array<int, 4> gs_row(const int* ent, size_t n) {
  std::array<int, 4> v = {-1, -1, -1, -1};
  if (n <= 4) std::copy(ent, ent + n, v.begin());
  else v[0] = -2;
  return v;
}

// direct-stiffness sum on the host: o[l] = the sum of f over l's list
inline std::vector<double> dssum_h(const std::vector<int>& gs_off, const std::vector<int>& gs_idx, const std::vector<double>& f) {
  const size_t nloc = gs_off.size() - 1;
  std::vector<double> o(nloc);
  for (size_t l = 0; l < nloc; ++l) { double s = 0; for (int k = gs_off[l]; k < gs_off[l + 1]; ++k) s += f[gs_idx[k]]; o[l] = s; }
  return o;
}

// inverse GLL spacings of the CFL rule (core/matvec.f:26-46, [UPSTREAM compute_cfl])
inline std::vector<double> dri_table(const std::vector<double>& z1) {
  const int N = (int)z1.size();
  std::vector<double> dri(N);
  dri[0] = 1.0 / (z1[1] - z1[0]); dri[N - 1] = 1.0 / (z1[N - 1] - z1[N - 2]);
  for (int i = 1; i < N - 1; ++i) dri[i] = 1.0 / (0.5 * (z1[i + 1] - z1[i - 1]));
  return dri;
}

// [nel][8][8] gather lists of the element corners (Dev::gs_corner): the CSR list of corner node (k, j, i) in {0, N-1}^3 of every
// element, -1 padded; a list longer than 8 is marked -2 (the kernels then walk the CSR arrays)
inline std::vector<int> corner_table(int N, int nel, const std::vector<int>& gs_off, const std::vector<int>& gs_idx) {
  std::vector<int> t((size_t)nel * 64, -1);
  const int NN = N * N * N;
  for (int e = 0; e < nel; ++e)
    for (int cc = 0; cc < 8; ++cc) {
      const int k = (cc & 4) ? N - 1 : 0, j = (cc & 2) ? N - 1 : 0, i = (cc & 1) ? N - 1 : 0;
      const long long l = (long long)e * NN + (k * N + j) * N + i;
      const int n = gs_off[l + 1] - gs_off[l];
      int* row = &t[((size_t)e * 8 + cc) * 8];
      if (n > 8) { row[0] = -2; continue; }
      for (int q = 0; q < n; ++q) row[q] = gs_idx[gs_off[l] + q];
    }
  return t;
}

// seconds per set-up section on stderr (NSK_SETUP_TIMING)
struct SectionTimer {
  const bool on = std::getenv("NSK_SETUP_TIMING") != nullptr;
  std::chrono::steady_clock::time_point last = std::chrono::steady_clock::now();
  void operator()(const char* what) {
    if (!on) return;
    const auto now = std::chrono::steady_clock::now();
    fprintf(stderr, "set-up %-44s %7.3f s\n", what, std::chrono::duration<double>(now - last).count());
    last = now;
  }
};

}  // namespace
}  // namespace nsk_setup
