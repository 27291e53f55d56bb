// Selective frequency damping on the device (core/fixedp.f:114-242, uparam(1) = 1.1): the low-pass filter state, the force
// that pulls the velocity towards it and the per-step residual, advanced inside the step loop of a map of the full equations.
//
// The reference calls SFD from userchk after every time step; call j (istep = j) sees v^j, the velocity after step j:
//   call 0:      qbar^0 given, vxo = v^0, lags uta = utb = utc = 0
//   call j >= 1: utc <- utb, utb <- uta, uta <- vxo - qbar^{j-1}                 (vxo still holds v^{j-1})
//                qbar^j = qbar^{j-1} + omega_c dt (a uta + b utb + c utc)        (setab3)
//   every call:  force of step j + 1 = -chi (vxo - qbar^j)                       -- v^{j-1}, ONE STEP BEHIND: the reference's order
//   call j >= 1: residu_j = sqrt(sum_c sum bm1 (v^{j-1} - v^j)_c^2 / volume),  then vxo <- v^j
// k_sfd is one call, one pass over the nodes: it runs behind the convection kernel of step j + 1 (where k_add_force runs),
// adds bm1 x force to that step's forcing array ahead of the EXT extrapolation, and once more behind the last step of the map
// (filter and residual only).  The reference spends about fourteen op* passes on the same.
//
// State per context: vxo and the two older lags (utb, utc of the NEXT call), three velocity-sized arrays; uta is recomputed.
// Every array is read and written at the thread's own nodes only, so the filter input and output may be one array.
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>

#include "nsk_kernels.hpp"

namespace nsk {
namespace sfd {

enum { CALL0 = 0, CALLJ = 1, LAST = 2 };

struct SfdCall {
  const double* u;          // velocity after the last step [ndim], component stride cs
  double* bf;               // forcing array of the step about to run [ndim], component stride cs (LAST: unused)
  const double* bm1;
  const double* qin;        // filter state [ndim][nloc] before the call
  double* qout;             // ... and behind it (CALL0: a copy of qin; may be qin)
  double *vxo, *l1, *l2;    // [ndim][nloc] each: velocity at the previous call; uta and utb of the previous call
  double* part;             // per-workgroup sums of bm1 (vxo - u)^2 over the components (CALLJ, LAST)
  long long nloc, cs;
  double a, b, c, wdt, gain;   // setab3's coefficients, omega_c dt, -chi
  int kind;
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
template <int NDIM, int V>
__global__ void __launch_bounds__(256) k_sfd(const SfdCall s) {
  __shared__ double sred[16];
  const int tid = threadIdx.x;
  const long long l = ((long long)blockIdx.x * 256 + tid) * V;
  double r[1] = {0.0};
  if (l < s.nloc) {                                             // (V == 2: nloc is even, so l + 1 < nloc as well)
    double bm[V];
    ld<V>(bm, s.bm1, l);
#pragma unroll
    for (int c = 0; c < NDIM; ++c) {
      const long long o = c * s.nloc + l, ou = c * s.cs + l;
      double v[V], q[V], vo[V], f[V];
      ld<V>(v, s.u, ou);
      ld<V>(q, s.qin, o);
      if (s.kind == CALL0) {
        double z[V];
#pragma unroll
        for (int k = 0; k < V; ++k) { vo[k] = v[k]; z[k] = 0.0; }
        st<V>(s.l1, o, z);
        st<V>(s.l2, o, z);
      } else {
        double ub[V], uc[V], ua[V];
        ld<V>(vo, s.vxo, o);
        ld<V>(ub, s.l1, o);
        ld<V>(uc, s.l2, o);
#pragma unroll
        for (int k = 0; k < V; ++k) {
          ua[k] = vo[k] - q[k];
          double t = s.a * ua[k];                                 // (the reference's order of operations: :176-191)
          t += s.b * ub[k];
          t += s.c * uc[k];
          q[k] += s.wdt * t;
          const double d = vo[k] - v[k];
          r[0] += bm[k] * (d * d);
        }
        if (s.kind == CALLJ) {
          st<V>(s.l2, o, ub);
          st<V>(s.l1, o, ua);
        }
      }
      st<V>(s.qout, o, q);
      if (s.kind != LAST) {
        ld<V>(f, s.bf, ou);
#pragma unroll
        for (int k = 0; k < V; ++k) f[k] += bm[k] * (s.gain * (vo[k] - q[k]));
        st<V>(s.bf, ou, f);
        st<V>(s.vxo, o, v);
      }
    }
  }
  if (s.kind == CALL0) return;                                  // (uniform over the grid)
  block_reduce<1>(r, sred, tid, 256);
  if (tid == 0) s.part[blockIdx.x] = r[0];
}

// workgroups of a call (= entries of SfdCall::part)
inline unsigned grid(long long nloc, int v) { return (unsigned)((nloc + 256LL * v - 1) / (256LL * v)); }

inline bool aligned16(const void* p) { return (reinterpret_cast<uintptr_t>(p) & 15) == 0; }
inline int width(const SfdCall& s) {
  const bool ok = s.nloc % 2 == 0 && s.cs % 2 == 0 && aligned16(s.u) && aligned16(s.bf) && aligned16(s.bm1) && aligned16(s.qin) &&
                  aligned16(s.qout) && aligned16(s.vxo) && aligned16(s.l1) && aligned16(s.l2);
  return ok ? 2 : 1;
}

inline void launch(hipStream_t stream, int ndim, const SfdCall& s, int v) {
  const dim3 g(grid(s.nloc, v)), b(256);
  if (ndim == 2) {
    if (v == 2) hipLaunchKernelGGL((k_sfd<2, 2>), g, b, 0, stream, s);
    else hipLaunchKernelGGL((k_sfd<2, 1>), g, b, 0, stream, s);
  } else {
    if (v == 2) hipLaunchKernelGGL((k_sfd<3, 2>), g, b, 0, stream, s);
    else hipLaunchKernelGGL((k_sfd<3, 1>), g, b, 0, stream, s);
  }
}

}  // namespace sfd
}  // namespace nsk
