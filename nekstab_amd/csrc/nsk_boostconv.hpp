// BoostConv on the device (core/fixedp.f:282-468, uparam(1) = 1.2): the residual-recombination accelerator of the fixed-point
// iteration v <- v + r(v), r = the velocity after a time step minus the velocity before it.
//
// The reference's boostconv_core keeps snp pairs X(j), Y(j) of velocity fields and a 1-based column `rot`:
//   first call:  Y(1) = X(1) = r;  rot = 1;  xi = r
//   later calls: Y(rot) -= r;  X(rot) -= Y(rot)
//                c = argmin |Y c - r| in the bm1 inner product (qr_dec: modified Gram-Schmidt over all snp columns, redone at
//                every call; linear_system: back substitution)
//                rot = mod(rot, snp) + 1;  Y(rot) = r;  xi = r + sum_j c_j X(j) (the OLD X(rot) included);  X(rot) = xi
// and BoostConv (:282-329) wraps it:  r = v - vlag(1);  residu = normvc l2 of r;  v = vlag(1) + xi.
//
// Here a call is three launches and about 2 snp + 6 passes over the velocity:
//   k_bcv_dots   r = a - b on the fly, Y(rot) and X(rot) updated in place, and per workgroup the 2 snp + 1 sums
//                sum bm1 r^2, <Y(j), Y(rot)> and <Y(j), r> for all j.  Only column `rot` of the Gram matrix D = Y^T bm1 Y changes
//                per call, so D is kept and one column is refreshed: no Q copy, no snp^2 / 2 inner products.
//   k_bcv_solve  one workgroup: the partials in a fixed order (or the ranks' all-reduced totals), row and column `rot` of D,
//                the safeguarded solve of D c = Y^T bm1 r, c and residu to device memory.  No host read.
//   k_bcv_apply  Y(rot') = r;  xi = r + sum_j c_j X(j);  X(rot') = xi;  u = b + xi.
// The first call is k_bcv_dots with `first` set (X(1) = Y(1) = r, the residual sum, which is D(1,1) too) and k_bcv_solve; the
// velocity is left alone (xi = r).  `b` is the velocity before the step (the map) or absent (nsk_boostconv_core: r = a, u = xi).
//
// The solve: D is scaled symmetrically by its diagonal; columns with D_jj < 1e-60 get c_j = 0 (the reference's rule, :436);
// Cholesky with diagonal pivoting; a scaled pivot below snp 2^-52 ends the factorisation and the columns left get c = 0.
// ONE DEVIATION from the reference: where two stored differences are parallel to within about 1e-8 (the pivot is the squared
// sine of the angle to the span of the columns taken before), qr_dec divides by a tiny R_jj; this code drops the column.
//
// State per context: X and Y, snp x ndim x nloc doubles each -- 2 snp velocity vectors, about 48 GB at config 5's size with
// snp = 10 -- D (16 x 16), c (16), the totals and the residual history on the device; `rot` and the call count are functions of
// the number of calls and travel as kernel arguments.  A MAP (nsk_boostconv_map) holds a copy of X, Y, D besides, taken when it
// starts: a map whose solves outrun the launch budgets is redone as a whole, and the calls it made have advanced the state.
// Every array is read and written at the thread's own nodes only.
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>

#include "nsk_kernels.hpp"

namespace nsk {
namespace bcv {

enum { SNP_MAX = 16 };

struct BcvCall {
  const double* a;          // velocity behind the step [ndim], component stride cs
  const double* b;          // velocity before it [ndim], component stride cs; nullptr: absent (r = a)
  double* u;                // k_bcv_apply: b + xi [ndim], component stride cs (may be a)
  const double* bm1;
  double *X, *Y;            // [snp][ndim][nloc]
  double* part;             // k_bcv_dots: [2 snp + 1][workgroups]: sum bm1 r^2, <Y(j), Y(rot)> (j < snp), <Y(j), r> (j < snp)
  const double* c;          // k_bcv_apply: the coefficients [snp]
  long long nloc, cs;
  int snp, rot, first;      // rot: 0-based column (k_bcv_dots: the one updated; k_bcv_apply: the one overwritten)
};

template <int V>
__device__ inline void ld(double (&x)[V], const double* p, long long i) {
  if constexpr (V == 2) { const double2 t = *reinterpret_cast<const double2*>(p + i); x[0] = t.x; x[1] = t.y; }
  else x[0] = p[i];
}
template <int V>
__device__ inline void st(double* p, long long i, const double (&x)[V]) {
  if constexpr (V == 2) *reinterpret_cast<double2*>(p + i) = make_double2(x[0], x[1]);
  else p[i] = x[0];
}

// V nodes per thread (2: 16-byte accesses; nloc, cs even and every array 16-byte aligned -- the launcher checks), 256 threads.
// CAP >= snp: the 2 CAP + 1 accumulators are registers (the loops over the columns are unrolled, columns >= snp skipped).
template <int NDIM, int V, int CAP>
__global__ void __launch_bounds__(256) k_bcv_dots(const BcvCall s) {
  __shared__ double sred[16 * (2 * CAP + 1)];
  const int tid = threadIdx.x;
  const long long l = ((long long)blockIdx.x * 256 + tid) * V;
  const long long nv = (long long)NDIM * s.nloc;
  double acc[2 * CAP + 1];
#pragma unroll
  for (int q = 0; q < 2 * CAP + 1; ++q) acc[q] = 0.0;
  if (l < s.nloc) {                                             // (V == 2: nloc is even, so l + 1 < nloc as well)
    double bm[V];
    ld<V>(bm, s.bm1, l);
#pragma unroll
    for (int c = 0; c < NDIM; ++c) {
      const long long o = c * s.nloc + l, ou = c * s.cs + l;
      double r[V];
      ld<V>(r, s.a, ou);
      if (s.b) {
        double b[V];
        ld<V>(b, s.b, ou);
#pragma unroll
        for (int k = 0; k < V; ++k) r[k] -= b[k];
      }
#pragma unroll
      for (int k = 0; k < V; ++k) acc[0] += bm[k] * (r[k] * r[k]);
      if (s.first) {
        st<V>(s.X, o, r);
        st<V>(s.Y, o, r);
      } else {
        const long long ok = (long long)s.rot * nv + o;
        double yk[V], xk[V];
        ld<V>(yk, s.Y, ok);
        ld<V>(xk, s.X, ok);
#pragma unroll
        for (int k = 0; k < V; ++k) { yk[k] -= r[k]; xk[k] -= yk[k]; }
        st<V>(s.Y, ok, yk);
        st<V>(s.X, ok, xk);
#pragma unroll
        for (int j = 0; j < CAP; ++j) {
          if (j < s.snp) {
            double yj[V];
            if (j == s.rot) {
#pragma unroll
              for (int k = 0; k < V; ++k) yj[k] = yk[k];
            } else {
              ld<V>(yj, s.Y, (long long)j * nv + o);
            }
#pragma unroll
            for (int k = 0; k < V; ++k) {
              const double w = bm[k] * yj[k];
              acc[1 + j] += w * yk[k];
              acc[1 + CAP + j] += w * r[k];
            }
          }
        }
      }
    }
  }
  block_reduce<2 * CAP + 1>(acc, sred, tid, 256);
  if (tid == 0) {
    const size_t nwg = gridDim.x;
    s.part[blockIdx.x] = acc[0];
    if (!s.first) {
#pragma unroll
      for (int j = 0; j < CAP; ++j)
        if (j < s.snp) {
          s.part[(size_t)(1 + j) * nwg + blockIdx.x] = acc[1 + j];
          s.part[(size_t)(1 + s.snp + j) * nwg + blockIdx.x] = acc[1 + CAP + j];
        }
    }
  }
}

// One workgroup of 256 threads.  nwg > 0: the 2 snp + 1 rows of per-workgroup partials are summed here in a fixed order
// (first call: row 0 only) into tot; nwg == 0: tot holds the totals already (shards: rank totals, all-reduced).  Then thread 0:
// row and column `rot` of D, the solve, c and residu = sqrt(tot[0] / vol).
__global__ void __launch_bounds__(256) k_bcv_solve(const double* __restrict__ part, int nwg, double* __restrict__ tot, double* __restrict__ D,
                                                  double* __restrict__ cvec, double* __restrict__ residu, int snp, int rot, int first, double vol) {
  __shared__ double sred[16];
  __shared__ double W[SNP_MAX * SNP_MAX], w[SNP_MAX], sc[SNP_MAX], z[SNP_MAX];
  __shared__ int idx[SNP_MAX];
  const int tid = threadIdx.x;
  if (nwg > 0) {
    const int rows = first ? 1 : 2 * snp + 1;
    for (int k = 0; k < rows; ++k) {
      double v[1];
      sum_partials<1>(part + (size_t)k * nwg, nwg, v, sred, tid, 256);
      if (tid == 0) tot[k] = v[0];
    }
  }
  if (tid != 0) return;
  *residu = sqrt(tot[0] / vol);
  for (int j = 0; j < snp; ++j) cvec[j] = 0.0;
  if (first) {
    for (int k = 0; k < SNP_MAX * SNP_MAX; ++k) D[k] = 0.0;
    D[0] = tot[0];
    return;
  }
  for (int j = 0; j < snp; ++j) D[j * SNP_MAX + rot] = D[rot * SNP_MAX + j] = tot[1 + j];
  // the columns that are there (D_jj >= 1e-60), scaled to a unit diagonal
  int m = 0;
  for (int j = 0; j < snp; ++j) {
    const double djj = D[j * SNP_MAX + j];
    if (djj >= 1e-60) { idx[m] = j; sc[m] = 1.0 / sqrt(djj); ++m; }
  }
  for (int t = 0; t < m; ++t) {
    for (int u = 0; u < m; ++u) W[t * SNP_MAX + u] = D[idx[t] * SNP_MAX + idx[u]] * sc[t] * sc[u];
    w[t] = tot[1 + snp + idx[t]] * sc[t];
  }
  // Cholesky with diagonal pivoting (the first of equal diagonals); L in the lower triangle
  const double floor_ = (double)snp * 0x1p-52;
  int rank = m;
  for (int k = 0; k < m; ++k) {
    int q = k;
    double best = W[k * SNP_MAX + k];
    for (int t = k + 1; t < m; ++t)
      if (W[t * SNP_MAX + t] > best) { best = W[t * SNP_MAX + t]; q = t; }
    if (!(best >= floor_)) { rank = k; break; }
    if (q != k) {
      for (int u = 0; u < m; ++u) { const double x = W[k * SNP_MAX + u]; W[k * SNP_MAX + u] = W[q * SNP_MAX + u]; W[q * SNP_MAX + u] = x; }
      for (int u = 0; u < m; ++u) { const double x = W[u * SNP_MAX + k]; W[u * SNP_MAX + k] = W[u * SNP_MAX + q]; W[u * SNP_MAX + q] = x; }
      { const double x = w[k]; w[k] = w[q]; w[q] = x; }
      { const double x = sc[k]; sc[k] = sc[q]; sc[q] = x; }
      { const int x = idx[k]; idx[k] = idx[q]; idx[q] = x; }
    }
    const double d = sqrt(best);
    W[k * SNP_MAX + k] = d;
    for (int t = k + 1; t < m; ++t) W[t * SNP_MAX + k] /= d;
    for (int t = k + 1; t < m; ++t)
      for (int u = k + 1; u <= t; ++u) {
        const double x = W[t * SNP_MAX + u] - W[t * SNP_MAX + k] * W[u * SNP_MAX + k];
        W[t * SNP_MAX + u] = x;
        W[u * SNP_MAX + t] = x;
      }
  }
  for (int t = 0; t < rank; ++t) {                                // L y = w
    double x = w[t];
    for (int u = 0; u < t; ++u) x -= W[t * SNP_MAX + u] * z[u];
    z[t] = x / W[t * SNP_MAX + t];
  }
  for (int t = rank - 1; t >= 0; --t) {                           // L^T z = y
    double x = z[t];
    for (int u = t + 1; u < rank; ++u) x -= W[u * SNP_MAX + t] * z[u];
    z[t] = x / W[t * SNP_MAX + t];
  }
  for (int t = 0; t < rank; ++t) cvec[idx[t]] = z[t] * sc[t];
}

template <int NDIM, int V>
__global__ void __launch_bounds__(256) k_bcv_apply(const BcvCall s) {
  const long long l = ((long long)blockIdx.x * 256 + threadIdx.x) * V;
  const long long nv = (long long)NDIM * s.nloc;
  if (l >= s.nloc) return;
#pragma unroll
  for (int c = 0; c < NDIM; ++c) {
    const long long o = c * s.nloc + l, ou = c * s.cs + l;
    double r[V], b[V], xi[V];
    ld<V>(r, s.a, ou);
#pragma unroll
    for (int k = 0; k < V; ++k) b[k] = 0.0;
    if (s.b) {
      ld<V>(b, s.b, ou);
#pragma unroll
      for (int k = 0; k < V; ++k) r[k] -= b[k];
    }
#pragma unroll
    for (int k = 0; k < V; ++k) xi[k] = r[k];
#pragma unroll 4
    for (int j = 0; j < s.snp; ++j) {
      const double cj = s.c[j];
      if (cj != 0.0) {                                            // (uniform: a dropped or still empty column is not read)
        double x[V];
        ld<V>(x, s.X, (long long)j * nv + o);
#pragma unroll
        for (int k = 0; k < V; ++k) xi[k] += cj * x[k];
      }
    }
    const long long ok = (long long)s.rot * nv + o;
    st<V>(s.Y, ok, r);
    st<V>(s.X, ok, xi);
#pragma unroll
    for (int k = 0; k < V; ++k) xi[k] += b[k];
    st<V>(s.u, ou, xi);
  }
}

// workgroups of a call (= entries of a row of BcvCall::part)
inline unsigned grid(long long nloc, int v) { return (unsigned)((nloc + 256LL * v - 1) / (256LL * v)); }

inline bool aligned16(const void* p) { return (reinterpret_cast<uintptr_t>(p) & 15) == 0; }
inline int width(const BcvCall& s) {
  const bool ok = s.nloc % 2 == 0 && s.cs % 2 == 0 && aligned16(s.a) && aligned16(s.b) && aligned16(s.u) && aligned16(s.bm1) && aligned16(s.X) && aligned16(s.Y);
  return ok ? 2 : 1;
}

template <int NDIM, int V>
inline void launch_dots_nv(hipStream_t stream, const BcvCall& s, const dim3 g) {
  const dim3 b(256);
  if (s.snp <= 4) hipLaunchKernelGGL((k_bcv_dots<NDIM, V, 4>), g, b, 0, stream, s);
  else if (s.snp <= 10) hipLaunchKernelGGL((k_bcv_dots<NDIM, V, 10>), g, b, 0, stream, s);
  else hipLaunchKernelGGL((k_bcv_dots<NDIM, V, SNP_MAX>), g, b, 0, stream, s);
}
inline void launch_dots(hipStream_t stream, int ndim, const BcvCall& s, int v) {
  const dim3 g(grid(s.nloc, v));
  if (ndim == 2) { if (v == 2) launch_dots_nv<2, 2>(stream, s, g); else launch_dots_nv<2, 1>(stream, s, g); }
  else { if (v == 2) launch_dots_nv<3, 2>(stream, s, g); else launch_dots_nv<3, 1>(stream, s, g); }
}
inline void launch_apply(hipStream_t stream, int ndim, const BcvCall& s, int v) {
  const dim3 g(grid(s.nloc, v)), b(256);
  if (ndim == 2) {
    if (v == 2) hipLaunchKernelGGL((k_bcv_apply<2, 2>), g, b, 0, stream, s);
    else hipLaunchKernelGGL((k_bcv_apply<2, 1>), g, b, 0, stream, s);
  } else {
    if (v == 2) hipLaunchKernelGGL((k_bcv_apply<3, 2>), g, b, 0, stream, s);
    else hipLaunchKernelGGL((k_bcv_apply<3, 1>), g, b, 0, stream, s);
  }
}

}  // namespace bcv
}  // namespace nsk
