// Stand-alone check of nekstab_amd/csrc/nsk_setup_host.hpp (tests/test_setup_host.py compiles it with the host compiler and
// -fsanitize=address,undefined and runs it): the gather-scatter tables of three small numberings against their definition.
#include "../nekstab_amd/csrc/nsk_setup_host.hpp"

#include <cstdio>
#include <map>
#include <random>

using namespace nsk_setup;

static int failures = 0;
#define CHECK(cond, ...)                                        \
  do {                                                          \
    if (!(cond)) {                                              \
      if (++failures <= 20) { fprintf(stderr, "FAIL %s:%d %s: ", __FILE__, __LINE__, #cond); fprintf(stderr, __VA_ARGS__); fprintf(stderr, "\n"); } \
    }                                                           \
  } while (0)

// global ids of an nx x ny (x nz) block of elements of order N - 1 on the tensor grid of their nodes; px: periodic in x
static std::vector<long long> numbering(int N, int nx, int ny, int nz, bool px) {
  const int gx = px ? nx * (N - 1) : nx * (N - 1) + 1, gy = ny * (N - 1) + 1;
  const int kn = nz ? N : 1;
  std::vector<long long> gid;
  for (int ez = 0; ez < std::max(nz, 1); ++ez)
    for (int ey = 0; ey < ny; ++ey)
      for (int ex = 0; ex < nx; ++ex)
        for (int k = 0; k < kn; ++k)
          for (int j = 0; j < N; ++j)
            for (int i = 0; i < N; ++i) {
              const long long X = (ex * (N - 1) + i) % gx, Y = ey * (N - 1) + j, Z = ez * (N - 1) + k;
              gid.push_back((Z * gy + Y) * gx + X);
            }
  return gid;
}

static void check_numbering(const char* name, const std::vector<long long>& gid, int N, int nel3d, int want_valence) {
  const long long nloc = (long long)gid.size();
  std::vector<int> gs_off, gs_idx;
  gs_csr(gid.data(), nloc, gs_off, gs_idx);
  CHECK((long long)gs_off.size() == nloc + 1 && gs_off[0] == 0 && gs_off[nloc] == (int)gs_idx.size(), "%s: CSR shape", name);
  std::map<long long, std::vector<int>> same;          // id -> its nodes, ascending local index
  for (long long l = 0; l < nloc; ++l) same[gid[l]].push_back((int)l);
  int valence = 0;
  for (long long l = 0; l < nloc; ++l) {
    const std::vector<int>& ref = same[gid[l]];
    const std::vector<int> got(gs_idx.begin() + gs_off[l], gs_idx.begin() + gs_off[l + 1]);
    CHECK(got == ref, "%s: list of node %lld", name, l);
    CHECK(std::find(got.begin(), got.end(), (int)l) != got.end(), "%s: node %lld not in its own list", name, l);
    valence = std::max(valence, (int)got.size());
    const std::array<int, 4> row = gs_row(got.data(), got.size());
    if (got.size() <= 4) {
      for (size_t k = 0; k < 4; ++k) CHECK(row[k] == (k < got.size() ? got[k] : -1), "%s: table row of node %lld", name, l);
    } else {
      CHECK(row[0] == -2, "%s: marker of node %lld", name, l);
    }
  }
  CHECK(valence == want_valence, "%s: largest valence %d, expected %d", name, valence, want_valence);
  const std::vector<double> mult = dssum_h(gs_off, gs_idx, std::vector<double>(nloc, 1.0));
  for (long long l = 0; l < nloc; ++l) CHECK(mult[l] == (double)same[gid[l]].size(), "%s: multiplicity of node %lld", name, l);
  if (nel3d) {
    const std::vector<int> ct = corner_table(N, nel3d, gs_off, gs_idx);
    CHECK(ct.size() == (size_t)nel3d * 64, "%s: corner table size", name);
    for (int e = 0; e < nel3d; ++e)
      for (int cc = 0; cc < 8; ++cc) {
        const int k = (cc & 4) ? N - 1 : 0, j = (cc & 2) ? N - 1 : 0, i = (cc & 1) ? N - 1 : 0;
        const long long l = (long long)e * N * N * N + (k * N + j) * N + i;
        const int n = gs_off[l + 1] - gs_off[l];
        const int* row = &ct[((size_t)e * 8 + cc) * 8];
        if (n > 8) { CHECK(row[0] == -2, "%s: corner marker", name); continue; }
        for (int q = 0; q < 8; ++q) CHECK(row[q] == (q < n ? gs_idx[gs_off[l] + q] : -1), "%s: corner %d of element %d", name, cc, e);
      }
  }
}

static void check_sort(const char* name, const std::vector<long long>& gid) {
  std::vector<std::pair<long long, int>> a(gid.size());
  for (size_t l = 0; l < gid.size(); ++l) a[l] = {gid[l], (int)l};
  std::vector<std::pair<long long, int>> b = a;
  sort_gid_pairs(a);
  std::sort(b.begin(), b.end());
  CHECK(a == b, "%s: sort_gid_pairs differs from std::sort", name);
}

int main() {
  const std::vector<long long> q22 = numbering(6, 2, 2, 0, false), qper = numbering(6, 3, 1, 0, true), h222 = numbering(6, 2, 2, 2, false);
  check_numbering("2 x 2 quadrilaterals", q22, 6, 0, 4);
  check_numbering("periodic line of 3 quadrilaterals", qper, 6, 0, 2);
  check_numbering("2 x 2 x 2 hexahedra", h222, 6, 8, 8);
  // a periodic line of ONE element: a node meets its own element's far side
  check_numbering("one periodic quadrilateral", numbering(6, 1, 1, 0, true), 6, 0, 2);
  check_sort("dense", h222);
  std::vector<long long> sparse = h222;                  // a rank's sub-mesh keeps the global ids: range > 8 n
  for (auto& g : sparse) g = g * 1000 + 7;
  check_sort("sparse", sparse);
  std::mt19937 rng(3);
  std::shuffle(sparse.begin(), sparse.end(), rng);
  check_sort("sparse, shuffled", sparse);
  const std::vector<double> dri = dri_table({-1.0, -0.5, 0.25, 1.0});
  CHECK(dri.size() == 4 && dri[0] == 2.0 && dri[1] == 1.0 / 0.625 && dri[2] == 1.0 / 0.75 && dri[3] == 1.0 / 0.75, "dri_table");
  if (failures) { fprintf(stderr, "%d checks failed\n", failures); return 1; }
  printf("setup_host_check ok\n");
  return 0;
}
