// Sensitivity post-processing on the device (core/sensitivity.f): wavemaker, base-flow sensitivity, biorthogonalisation,
// the steady body force of the forced linearised maps (core/utils.f:160-162), and the stability energy budget
// (core/postproc.f:657-872), followed by the vorticity of the Rv files (comp_vort3) and, at the end of this file, the
// vortex-identification criteria of the vox / omg files (vortex_core: lambda2, Q, Omega; core/postproc.f:2-79, 374-403).
//
// The base-flow sensitivity is linear in each mode's gradient times the other modes' values, so it is built one mode
// COMPONENT at a time: k_sens_grad writes the element-local physical gradient of that component (ndim fields, gradm1 with
// the metrics derived in the kernel from the GLL coordinates), k_sens_acc averages it over shared nodes (dsavg through the
// gather tables of the dssum) and adds its products with the other modes' values into the outputs.  Scratch: ndim
// velocity-sized fields (the context's state-sized scratch vector); nothing is kept between calls.
// On an element shard (nsk_group_* entries) the gradient fields carry ghost slots behind their nloc entries (component stride
// Dev::cs) and are exchanged between k_sens_grad and the gathering kernel; the kernels take that stride as an argument.
#pragma once
#include <hip/hip_runtime.h>

#include "nsk_dev.hpp"
#include "nsk_kernels.hpp"

namespace nsk {
namespace sens {

template <int N, int NDIM>
struct SensCfg {
  static constexpr int NP = NDIM == 3 ? N * N * N : N * N;     // GLL nodes of one element
  static constexpr int NT = ((NP + 63) / 64) * 64;
};

// g[i * gs + l] = d f / d x_i at the element-local node l (no averaging): (r_x f_r + s_x f_s [+ t_x f_t]) with the
// inverse mapping from the coordinates' own derivatives (Nek5000 gradm1: cofactors over the Jacobian).  One workgroup per element.
// gs: component stride of g -- nloc on a full-mesh context, nloc + ghost slots (Dev::cs) on a shard, whose gradient is
// exchanged (k_halo_pack / k_halo_unpack fill g[i * gs + nloc ..]) before it is gathered.
template <int N, int NDIM>
__global__ void __launch_bounds__((SensCfg<N, NDIM>::NT)) k_sens_grad(const double* __restrict__ D, const double* __restrict__ xyz,
                                                                    const double* __restrict__ f, double* __restrict__ g, long long nloc,
                                                                    long long gs) {
  constexpr int NP = SensCfg<N, NDIM>::NP;
  __shared__ double sD[N * N];
  __shared__ double sf[NP], sx[NP], sy[NP], sz[NDIM == 3 ? NP : 1];
  const int tid = threadIdx.x;
  const long long e0 = (long long)blockIdx.x * NP;
  if (tid < N * N) sD[tid] = D[tid];
  const bool act = tid < NP;
  if (act) {
    sf[tid] = f[e0 + tid];
    sx[tid] = xyz[e0 + tid];
    sy[tid] = xyz[nloc + e0 + tid];
    if constexpr (NDIM == 3) sz[tid] = xyz[2 * nloc + e0 + tid];
  }
  __syncthreads();
  if (!act) return;
  const int i = tid % N, j = (tid / N) % N, k = NDIM == 3 ? tid / (N * N) : 0;
  const int bj = NDIM == 3 ? (k * N * N + i) : i;           // line of constant (i, k) runs over j with stride N
  const int bi = tid - i, bk = j * N + i;                   // line of constant (j, k) over i; of constant (i, j) over k (stride N*N)
  double fr = 0, fs = 0, ft = 0, xr = 0, xs = 0, xt = 0, yr = 0, ys = 0, yt = 0, zr = 0, zs = 0, zt = 0;
#pragma unroll
  for (int q = 0; q < N; ++q) {
    const double di = sD[i * N + q], dj = sD[j * N + q];
    fr += di * sf[bi + q]; xr += di * sx[bi + q]; yr += di * sy[bi + q];
    fs += dj * sf[bj + q * N]; xs += dj * sx[bj + q * N]; ys += dj * sy[bj + q * N];
    if constexpr (NDIM == 3) {
      const double dk = sD[k * N + q];
      zr += di * sz[bi + q]; zs += dj * sz[bj + q * N];
      ft += dk * sf[bk + q * N * N]; xt += dk * sx[bk + q * N * N]; yt += dk * sy[bk + q * N * N]; zt += dk * sz[bk + q * N * N];
    }
  }
  const long long l = e0 + tid;
  if constexpr (NDIM == 2) {
    const double jinv = 1.0 / (xr * ys - xs * yr);
    g[l] = (ys * fr - yr * fs) * jinv;                      // r_x = y_s / J, s_x = -y_r / J
    g[gs + l] = (xr * fs - xs * fr) * jinv;                 // r_y = -x_s / J, s_y = x_r / J
  } else {
    const double c_rx = ys * zt - yt * zs, c_ry = xt * zs - xs * zt, c_rz = xs * yt - xt * ys;
    const double c_sx = yt * zr - yr * zt, c_sy = xr * zt - xt * zr, c_sz = xt * yr - xr * yt;
    const double c_tx = yr * zs - ys * zr, c_ty = xs * zr - xr * zs, c_tz = xr * ys - xs * yr;
    const double jinv = 1.0 / (xr * c_rx + yr * c_ry + zr * c_rz);
    g[l] = (c_rx * fr + c_sx * fs + c_tx * ft) * jinv;
    g[gs + l] = (c_ry * fr + c_sy * fs + c_ty * ft) * jinv;
    g[2 * gs + l] = (c_rz * fr + c_sz * fs + c_tz * ft) * jinv;
  }
}

template <int N, int NDIM>
inline void launch_sens_grad(hipStream_t st, int nel, const double* D, const double* xyz, const double* f, double* g, long long nloc,
                             long long gs) {
  hipLaunchKernelGGL((k_sens_grad<N, NDIM>), dim3(nel), dim3(SensCfg<N, NDIM>::NT), 0, st, D, xyz, f, g, nloc, gs);
}

// Accumulation of one mode component's averaged gradient G_i = dsavg(g_i) (sensitivity.f:215-256, Marquet et al. 2008):
//   transport (the mode is direct, component j):      outR_i += wR sR_j G_i,         outI_i += wI sI_j G_i
//   production (the mode is adjoint, component i):     outR_i += wR sum_j sR_j G_j,   outI_i += wI sum_j sI_j G_j
// s* are velocity fields with component stride nloc (the other mode's values), out* the output vectors; g has component
// stride gs (as k_sens_grad wrote it; on a shard its ghost slots hold the peers' partial sums and Dev::minv is the global
// multiplicity, so the gather below is the dsavg over ALL ranks).
struct SensAcc {
  const double *sR, *sI;
  double *outR, *outI;
  double wR, wI;
  int comp, production;
};

template <int NDIM>
__global__ void k_sens_acc(const Dev d, const double* __restrict__ g, long long gs, const SensAcc a) {
  const long long l = (long long)blockIdx.x * blockDim.x + threadIdx.x;
  if (l >= d.nloc) return;
  const long long n = d.nloc;
  const double mi = d.minv[l];
  double G[NDIM];
#pragma unroll
  for (int q = 0; q < NDIM; ++q) G[q] = gs_gather(g + q * gs, d, l) * mi;
  if (!a.production) {
    const double cr = a.wR * a.sR[a.comp * n + l], ci = a.wI * a.sI[a.comp * n + l];
#pragma unroll
    for (int q = 0; q < NDIM; ++q) {
      a.outR[q * n + l] += cr * G[q];
      a.outI[q * n + l] += ci * G[q];
    }
  } else {
    double r = 0.0, m = 0.0;
#pragma unroll
    for (int q = 0; q < NDIM; ++q) {
      r += a.sR[q * n + l] * G[q];
      m += a.sI[q * n + l] * G[q];
    }
    a.outR[a.comp * n + l] += a.wR * r;
    a.outI[a.comp * n + l] += a.wI * m;
  }
}

// wave_maker (sensitivity.f:70-72): |d| |a| pointwise, velocity components only
__global__ void k_wavemaker(const double* __restrict__ dR, const double* __restrict__ dI, const double* __restrict__ aR,
                            const double* __restrict__ aI, double* __restrict__ wm, long long nloc, int ndim) {
  const long long l = (long long)blockIdx.x * blockDim.x + threadIdx.x;
  if (l >= nloc) return;
  double sd = 0.0, sa = 0.0;
  for (int c = 0; c < ndim; ++c) {
    const long long o = c * nloc + l;
    sd += dR[o] * dR[o] + dI[o] * dI[o];
    sa += aR[o] * aR[o] + aI[o] * aI[o];
  }
  wm[l] = sqrt(sd) * sqrt(sa);
}

// biorthogonalize (sensitivity.f:487-501): a <- a / conj(gamma + i delta), i.e. aR' = p aR - q aI, aI' = p aI + q aR
// with p = gamma / (gamma^2 + delta^2), q = delta / (gamma^2 + delta^2)
__global__ void k_cdiv(double* __restrict__ aR, double* __restrict__ aI, double p, double q, long long n) {
  const long long l = (long long)blockIdx.x * blockDim.x + threadIdx.x;
  if (l >= n) return;
  const double r = aR[l], m = aI[l];
  aR[l] = p * r - q * m;
  aI[l] = p * m + q * r;
}

// out = a + b over n entries (sr = tr + pr, si = ti + pi)
__global__ void k_add3(double* __restrict__ out, const double* __restrict__ a, const double* __restrict__ b, long long n) {
  const long long l = (long long)blockIdx.x * blockDim.x + threadIdx.x;
  if (l < n) out[l] = a[l] + b[l];
}

// Steady body force of a forced map (nekStab_forcing, core/utils.f:160-162, made mass-weighted by makeuf): bf += B f,
// after the convection kernel has written this step's sponge + convection term and before the EXT extrapolation reads it.
__global__ void k_add_force(double* __restrict__ bf, long long cs, const double* __restrict__ bm1, const double* __restrict__ f,
                            long long nloc, int ndim) {
  const long long l = (long long)blockIdx.x * blockDim.x + threadIdx.x;
  if (l >= nloc) return;
  const double b = bm1[l];
  for (int c = 0; c < ndim; ++c) bf[c * cs + l] += b * f[c * nloc + l];
}

// ---- stability_energy_budget (core/postproc.f:657-872, uparam(1) = 4.1) ------------------------------------------------
// Production P[c][j] = w uu_cj dU_c/dx_j (w = -1/2 / ||u||^2, uu_cj = uR_c uR_j + uI_c uI_j, base-flow gradient element-local:
// gradm1 without dsavg) by k_budget_prod; dissipation D = 1/2 nu / ||u||^2 sum over the 2 ndim mode components a of a Lap(a),
// Lap(a) = dsavg(sum_i d/dx_i dsavg(d a / dx_i)), one component at a time: k_sens_grad (gradient into scratch), k_budget_div
// (gather-average of the gradient, divergence, element-local), k_budget_diss (gather-average of the divergence, product,
// accumulation).  Every kernel writes bm1-weighted per-workgroup partials; k_reduce_final sums them in a fixed order.

// inverse mapping at element-local node tid: m[r][a] = d r_r / d x_a (cofactors over the Jacobian, as k_sens_grad)
template <int N, int NDIM>
__device__ inline void elem_inv_metric(const double* sD, const double* sx, const double* sy, const double* sz, int tid,
                                       double (&m)[NDIM][NDIM]) {
  const int i = tid % N, j = (tid / N) % N, k = NDIM == 3 ? tid / (N * N) : 0;
  const int bj = NDIM == 3 ? (k * N * N + i) : i, bi = tid - i, bk = j * N + i;
  double xr = 0, xs = 0, xt = 0, yr = 0, ys = 0, yt = 0, zr = 0, zs = 0, zt = 0;
#pragma unroll
  for (int q = 0; q < N; ++q) {
    const double di = sD[i * N + q], dj = sD[j * N + q];
    xr += di * sx[bi + q]; yr += di * sy[bi + q];
    xs += dj * sx[bj + q * N]; ys += dj * sy[bj + q * N];
    if constexpr (NDIM == 3) {
      const double dk = sD[k * N + q];
      zr += di * sz[bi + q]; zs += dj * sz[bj + q * N];
      xt += dk * sx[bk + q * N * N]; yt += dk * sy[bk + q * N * N]; zt += dk * sz[bk + q * N * N];
    }
  }
  if constexpr (NDIM == 2) {
    const double jinv = 1.0 / (xr * ys - xs * yr);
    m[0][0] = ys * jinv; m[0][1] = -xs * jinv;
    m[1][0] = -yr * jinv; m[1][1] = xr * jinv;
  } else {
    const double c_rx = ys * zt - yt * zs, c_ry = xt * zs - xs * zt, c_rz = xs * yt - xt * ys;
    const double c_sx = yt * zr - yr * zt, c_sy = xr * zt - xt * zr, c_sz = xt * yr - xr * yt;
    const double c_tx = yr * zs - ys * zr, c_ty = xs * zr - xr * zs, c_tz = xr * ys - xs * yr;
    const double jinv = 1.0 / (xr * c_rx + yr * c_ry + zr * c_rz);
    m[0][0] = c_rx * jinv; m[0][1] = c_ry * jinv; m[0][2] = c_rz * jinv;
    m[1][0] = c_sx * jinv; m[1][1] = c_sy * jinv; m[1][2] = c_sz * jinv;
    m[2][0] = c_tx * jinv; m[2][1] = c_ty * jinv; m[2][2] = c_tz * jinv;
  }
}

// reference-space derivatives (f_r, f_s [, f_t]) of the element field sf at node tid
template <int N, int NDIM>
__device__ inline void elem_ref_deriv(const double* sD, const double* sf, int tid, double (&fd)[NDIM]) {
  const int i = tid % N, j = (tid / N) % N, k = NDIM == 3 ? tid / (N * N) : 0;
  const int bj = NDIM == 3 ? (k * N * N + i) : i, bi = tid - i, bk = j * N + i;
  double fr = 0, fs = 0, ft = 0;
#pragma unroll
  for (int q = 0; q < N; ++q) {
    fr += sD[i * N + q] * sf[bi + q];
    fs += sD[j * N + q] * sf[bj + q * N];
    if constexpr (NDIM == 3) ft += sD[k * N + q] * sf[bk + q * N * N];
  }
  fd[0] = fr; fd[1] = fs;
  if constexpr (NDIM == 3) fd[2] = ft;
}

template <int N, int NDIM>
__device__ inline void elem_load_geom(const double* __restrict__ D, const double* __restrict__ xyz, long long e0, long long nloc,
                                      int tid, double* sD, double* sx, double* sy, double* sz) {
  constexpr int NP = SensCfg<N, NDIM>::NP;
  if (tid < N * N) sD[tid] = D[tid];
  if (tid < NP) {
    sx[tid] = xyz[e0 + tid];
    sy[tid] = xyz[nloc + e0 + tid];
    if constexpr (NDIM == 3) sz[tid] = xyz[2 * nloc + e0 + tid];
  }
}

// production: prod[c] (may be null) receives P[c][j] in its velocity component j; part[(3 c + j) * nel + e] the bm1-weighted
// sum over element e (9 rows; rows of a missing third dimension are 0).  One workgroup per element.
struct BudgetProd { double* p[3]; };

template <int N, int NDIM>
__global__ void __launch_bounds__((SensCfg<N, NDIM>::NT)) k_budget_prod(const double* __restrict__ D, const double* __restrict__ xyz,
    const double* __restrict__ ub, const double* __restrict__ uR, const double* __restrict__ uI, const double* __restrict__ bm1,
    const BudgetProd prod, double w, double* __restrict__ part, long long nloc) {
  constexpr int NP = SensCfg<N, NDIM>::NP, NT = SensCfg<N, NDIM>::NT;
  __shared__ double sD[N * N];
  __shared__ double sf[NP], sx[NP], sy[NP], sz[NDIM == 3 ? NP : 1];
  __shared__ double sred[3 * 16];
  const int tid = threadIdx.x;
  const long long e0 = (long long)blockIdx.x * NP, l = e0 + tid;
  const bool act = tid < NP;
  elem_load_geom<N, NDIM>(D, xyz, e0, nloc, tid, sD, sx, sy, sz);
  __syncthreads();
  double m[NDIM][NDIM] = {};
  if (act) elem_inv_metric<N, NDIM>(sD, sx, sy, sz, tid, m);
  double r[NDIM] = {}, im[NDIM] = {};
  if (act) {
#pragma unroll
    for (int c = 0; c < NDIM; ++c) { r[c] = uR[c * nloc + l]; im[c] = uI[c * nloc + l]; }
  }
  const double b = act ? bm1[l] : 0.0;
#pragma unroll
  for (int c = 0; c < 3; ++c) {                               // row c of the partials (c = 2 in 2-D: zeros)
    double v[3] = {0.0, 0.0, 0.0};
    if (c < NDIM) {
      if (act) sf[tid] = ub[c * nloc + l];
      __syncthreads();
      if (act) {
        double fd[NDIM];
        elem_ref_deriv<N, NDIM>(sD, sf, tid, fd);
#pragma unroll
        for (int j = 0; j < NDIM; ++j) {
          double g = 0.0;
#pragma unroll
          for (int q = 0; q < NDIM; ++q) g += m[q][j] * fd[q];   // d U_c / d x_j
          const double P = w * (r[c] * r[j] + im[c] * im[j]) * g;
          if (prod.p[c]) prod.p[c][j * nloc + l] = P;
          v[j] = b * P;
        }
      }
    }
    block_reduce<3>(v, sred, tid, NT);                          // its barriers also end the reads of sf
    if (tid == 0) {
#pragma unroll
      for (int j = 0; j < 3; ++j) part[(size_t)(3 * c + j) * gridDim.x + blockIdx.x] = v[j];
    }
  }
}

// div[l] = sum_i d/dx_i dsavg(g_i) at the element-local node l (g: ndim gradient fields, stride gs as k_sens_grad wrote them).
// One workgroup per element.  On a shard div has room for the ghost slots behind its nloc entries: it is averaged again.
template <int N, int NDIM>
__global__ void __launch_bounds__((SensCfg<N, NDIM>::NT)) k_budget_div(const Dev d, const double* __restrict__ xyz,
                                                                     const double* __restrict__ g, long long gs,
                                                                     double* __restrict__ div) {
  constexpr int NP = SensCfg<N, NDIM>::NP;
  __shared__ double sD[N * N];
  __shared__ double sf[NP], sx[NP], sy[NP], sz[NDIM == 3 ? NP : 1];
  const int tid = threadIdx.x;
  const long long nloc = d.nloc, e0 = (long long)blockIdx.x * NP, l = e0 + tid;
  const bool act = tid < NP;
  elem_load_geom<N, NDIM>(d.D, xyz, e0, nloc, tid, sD, sx, sy, sz);
  const double mi = act ? d.minv[l] : 0.0;
  __syncthreads();
  double m[NDIM][NDIM] = {};
  if (act) elem_inv_metric<N, NDIM>(sD, sx, sy, sz, tid, m);
  double acc = 0.0;
#pragma unroll
  for (int a = 0; a < NDIM; ++a) {
    if (a) __syncthreads();
    if (act) sf[tid] = gs_gather(g + a * gs, d, l) * mi;
    __syncthreads();
    if (!act) continue;
    double fd[NDIM];
    elem_ref_deriv<N, NDIM>(sD, sf, tid, fd);
#pragma unroll
    for (int q = 0; q < NDIM; ++q) acc += m[q][a] * fd[q];
  }
  if (act) div[l] = acc;
}

// D += w a dsavg(div) (diss may be null; first: D = instead of +=), part[blockIdx] = the bm1-weighted sum.  256 threads.
__global__ void __launch_bounds__(256) k_budget_diss(const Dev d, const double* __restrict__ div, const double* __restrict__ a,
                                                     double* __restrict__ diss, double w, int first, double* __restrict__ part) {
  __shared__ double sred[16];
  const int tid = threadIdx.x;
  const long long l = (long long)blockIdx.x * 256 + tid;
  double v[1] = {0.0};
  if (l < d.nloc) {
    const double t = w * a[l] * (gs_gather(div, d, l) * d.minv[l]);
    if (diss) diss[l] = first ? t : diss[l] + t;
    v[0] = d.bm1[l] * t;
  }
  block_reduce<1>(v, sred, tid, 256);
  if (tid == 0) part[blockIdx.x] = v[0];
}

// ---- comp_vort3 (the Rv files of outpost_ks, core/eigensolvers.f:629-637) ------------------------------------------------
// Vorticity of the velocity of a state vector, averaged over shared nodes with the MASS as weight: element-local curl times the
// unassembled bm1, summed over co-located nodes, divided by the assembled bm1 -- NOT dsavg (multiplicity) and without the
// Dirichlet mask (Dev::binv carries it: it would zero the wall nodes, where a mode's vorticity is largest).  Two launches:
// k_vort (all derivatives of all components in one pass over the element) and k_vort_avg (gather, divide, fill the output).

// g[c * gs + l] = bm1[l] * curl(u)_c at the element-local node l: one field in 2-D (dv/dx - du/dy), three in 3-D.
// u: velocity with component stride nloc; gs: component stride of g (nloc, or Dev::cs on a shard: ghost slots behind).
// One workgroup per element; D, the ndim velocity components and the ndim coordinates in LDS, metrics derived here.
template <int N, int NDIM>
__global__ void __launch_bounds__((SensCfg<N, NDIM>::NT)) k_vort(const double* __restrict__ D, const double* __restrict__ xyz,
                                                               const double* __restrict__ u, const double* __restrict__ bm1,
                                                               double* __restrict__ g, long long nloc, long long gs) {
  constexpr int NP = SensCfg<N, NDIM>::NP;
  __shared__ double sD[N * N];
  __shared__ double su[NDIM][NP], sx[NP], sy[NP], sz[NDIM == 3 ? NP : 1];
  const int tid = threadIdx.x;
  const long long e0 = (long long)blockIdx.x * NP, l = e0 + tid;
  const bool act = tid < NP;
  elem_load_geom<N, NDIM>(D, xyz, e0, nloc, tid, sD, sx, sy, sz);
  if (act) {
#pragma unroll
    for (int c = 0; c < NDIM; ++c) su[c][tid] = u[c * nloc + l];
  }
  __syncthreads();
  if (!act) return;
  double m[NDIM][NDIM];
  elem_inv_metric<N, NDIM>(sD, sx, sy, sz, tid, m);
  double du[NDIM][NDIM];                                       // du[c][a] = d u_c / d x_a
#pragma unroll
  for (int c = 0; c < NDIM; ++c) {
    double fd[NDIM];
    elem_ref_deriv<N, NDIM>(sD, su[c], tid, fd);
#pragma unroll
    for (int a = 0; a < NDIM; ++a) {
      double s = 0.0;
#pragma unroll
      for (int q = 0; q < NDIM; ++q) s += m[q][a] * fd[q];
      du[c][a] = s;
    }
  }
  const double b = bm1[l];
  if constexpr (NDIM == 2) {
    g[l] = b * (du[1][0] - du[0][1]);
  } else {
    g[l] = b * (du[2][1] - du[1][2]);
    g[gs + l] = b * (du[0][2] - du[2][0]);
    g[2 * gs + l] = b * (du[1][0] - du[0][1]);
  }
}

template <int N, int NDIM>
inline void launch_vort(hipStream_t st, int nel, const double* D, const double* xyz, const double* u, const double* bm1, double* g,
                        long long nloc, long long gs) {
  hipLaunchKernelGGL((k_vort<N, NDIM>), dim3(nel), dim3(SensCfg<N, NDIM>::NT), 0, st, D, xyz, u, bm1, g, nloc, gs);
}

// the assembled, UNMASKED mass: out[l] = sum of bm1 over the nodes co-located with l (f: bm1, on a shard with the peers'
// partial sums in the ghost slots behind its nloc entries)
__global__ void k_vort_mass(const Dev d, const double* __restrict__ f, double* __restrict__ out) {
  const long long l = (long long)blockIdx.x * blockDim.x + threadIdx.x;
  if (l < d.nloc) out[l] = gs_gather(f, d, l);
}

// w = the state vector whose velocity is dssum(g) / mass: 2-D (omega, 0), 3-D (omega_x, omega_y, omega_z); pressure and scalar
// slots 0.  One thread per entry of w (nstate of them); the gather adds in ascending order of the co-located nodes, no atomics.
template <int NDIM>
__global__ void k_vort_avg(const Dev d, const double* __restrict__ g, long long gs, const double* __restrict__ mass,
                           double* __restrict__ w, long long nstate) {
  constexpr int NC = NDIM == 3 ? 3 : 1;
  const long long l = (long long)blockIdx.x * blockDim.x + threadIdx.x;
  if (l >= nstate) return;
  if (l < d.nloc) {
    const double mi = mass[l];
#pragma unroll
    for (int c = 0; c < NC; ++c) w[c * d.nloc + l] = gs_gather(g + c * gs, d, l) / mi;
  }
  if (l >= NC * d.nloc) w[l] = 0.0;
}

// ---- vortex_core('lambda2' / 'q' / 'omega') of nekStab_outpost (the vox and omg files, core/usr_extra.f:269-281) -------------
// With g[i][j] = d u_i / d x_j at the element-local node (comp_gije: no averaging), S = (g + g^T) / 2, O = (g - g^T) / 2,
// ndim x ndim (2 x 2 on quadrilaterals):
//   lambda2  the second largest eigenvalue of A = S S + O O (Jeong & Hussain): the middle of three, the smaller of two
//   Q        compute_secondInv (core/postproc.f:374-403): 3-D the sum of the three principal 2 x 2 minors of g; 2-D the
//            reference's (g11 + g22)^2 - 2 g12 g21 - g11^2 - g22^2 = 2 det g, which is TWICE the 3-D expression of a z-invariant
//            field (its minors with the third direction vanish and one det g is left) -- kept as the reference has it
//   Omega    compute_omega_jc (core/postproc.f:31-79): b / (a + b + 1e-5), a = (||S||_F^2)^2, b = (||O||_F^2)^2; the constant
//            is the reference's and is not scaled
// each then filtered as filter_s0(f, wght, 1, .) does: f <- (F x F [x F]) f along the reference directions of the element.
// Everything is element-local and pointwise: no gather, no exchange on shards, no atomics, one order of operations.
//
// Eigenvalues: cyclic Jacobi sweeps on the six (three) entries of A in registers, eigenvalues only.  The closed-form
// trigonometric root formula loses half its digits where two eigenvalues meet -- and for a z-invariant, divergence-free field
// A = diag(c, c, 0) at EVERY node; a Jacobi rotation is an orthogonal similarity whatever the gaps are, so the diagonal it
// leaves is within a few ulp of ||A|| of the eigenvalues, degenerate or not.  A 2 x 2 matrix is diagonal after one rotation.
// For 3 x 3, JACOBI_SWEEPS = 5: over 4e5 random matrices S S + O O the largest off-diagonal norm after sweeps 1 .. 4 is
// 5e-1, 7e-2, 2e-5, 6e-21 of ||A|| (the convergence is quadratic and better), nearly degenerate ones are there after two; the
// fifth sweep is margin, and a rotation whose pivot is already 0 changes nothing.
constexpr int JACOBI_SWEEPS = 5;

// one rotation in the (p, q) plane of a symmetric matrix, annihilating apq; arp, arq: the entries coupling p and q to the third
// index (2 x 2: pass two dummies).  t = tan of the smaller angle (|t| <= 1); apq = 0, or so small that theta^2 overflows: t = 0.
__device__ inline void jacobi_rotate(double& app, double& aqq, double& apq, double& arp, double& arq) {
  const double theta = (aqq - app) / (2.0 * apq);
  const double t = apq == 0.0 ? 0.0 : copysign(1.0, theta) / (fabs(theta) + sqrt(theta * theta + 1.0));
  const double c = 1.0 / sqrt(t * t + 1.0), s = t * c;
  app -= t * apq;
  aqq += t * apq;
  apq = 0.0;
  const double p = arp, q = arq;
  arp = c * p - s * q;
  arq = s * p + c * q;
}

// (lambda2, Q, Omega) of the velocity gradient g[i][j] = d u_i / d x_j at one node
template <int NDIM>
__device__ inline void vortex_point(const double (&g)[NDIM][NDIM], double (&v)[3]) {
  double S[NDIM][NDIM], O[NDIM][NDIM];
  double ns = 0.0, no = 0.0;
#pragma unroll
  for (int i = 0; i < NDIM; ++i)
#pragma unroll
    for (int j = 0; j < NDIM; ++j) {
      S[i][j] = 0.5 * (g[i][j] + g[j][i]);
      O[i][j] = 0.5 * (g[i][j] - g[j][i]);
      ns += S[i][j] * S[i][j];
      no += O[i][j] * O[i][j];
    }
  double A[NDIM][NDIM];                                          // the upper triangle is used
#pragma unroll
  for (int i = 0; i < NDIM; ++i)
#pragma unroll
    for (int j = i; j < NDIM; ++j) {
      double s = 0.0;
#pragma unroll
      for (int k = 0; k < NDIM; ++k) s += S[i][k] * S[k][j] + O[i][k] * O[k][j];
      A[i][j] = s;
    }
  if constexpr (NDIM == 2) {
    double d0 = 0.0, d1 = 0.0;
    jacobi_rotate(A[0][0], A[1][1], A[0][1], d0, d1);
    v[0] = fmin(A[0][0], A[1][1]);
    v[1] = (g[0][0] + g[1][1]) * (g[0][0] + g[1][1]) - 2.0 * g[0][1] * g[1][0] - g[0][0] * g[0][0] - g[1][1] * g[1][1];
  } else {
#pragma unroll
    for (int sweep = 0; sweep < JACOBI_SWEEPS; ++sweep) {
      jacobi_rotate(A[0][0], A[1][1], A[0][1], A[0][2], A[1][2]);
      jacobi_rotate(A[0][0], A[2][2], A[0][2], A[0][1], A[1][2]);
      jacobi_rotate(A[1][1], A[2][2], A[1][2], A[0][1], A[0][2]);
    }
    const double lo = fmin(A[0][0], A[1][1]), hi = fmax(A[0][0], A[1][1]);
    v[0] = fmax(lo, fmin(hi, A[2][2]));                           // the middle of three
    v[1] = (g[1][1] * g[2][2] - g[1][2] * g[2][1]) + (g[0][0] * g[1][1] - g[0][1] * g[1][0]) + (g[2][2] * g[0][0] - g[0][2] * g[2][0]);
  }
  const double a = ns * ns, b = no * no;
  v[2] = b / (a + b + 1.0e-5);
}

// w: lambda2 and Q in the first two velocity components and, in 3-D, Omega in the third (component stride nloc); om (may be
// null): Omega in its first component.  F: null (no filter: the criteria leave as they were computed) or the lx1 x lx1 filter
// matrix, row-major.  One workgroup per element; D, the ndim velocity components and the ndim coordinates in LDS, the gradient
// in registers as in k_vort; the three filtered fields then pass through the first three of those LDS buffers, which are free
// once every thread holds its gradient: one tensor-product pass per direction for all three fields, each thread keeping its
// results in registers across the barrier that ends the reads of the pass.
template <int N, int NDIM>
__global__ void __launch_bounds__((SensCfg<N, NDIM>::NT)) k_vortex(const double* __restrict__ D, const double* __restrict__ xyz,
                                                                 const double* __restrict__ u, const double* __restrict__ F,
                                                                 double* __restrict__ w, double* __restrict__ om, long long nloc) {
  constexpr int NP = SensCfg<N, NDIM>::NP;
  __shared__ double sD[N * N], sF[N * N];
  __shared__ double sb[2 * NDIM][NP];                            // [0, NDIM): velocity, then x, y [, z]; the filter: [0, 3)
  static_assert(2 * NDIM >= 3, "three buffers for the filter passes");
  const int tid = threadIdx.x;
  const long long e0 = (long long)blockIdx.x * NP, l = e0 + tid;
  const bool act = tid < NP;
  elem_load_geom<N, NDIM>(D, xyz, e0, nloc, tid, sD, sb[NDIM], sb[NDIM + 1], sb[2 * NDIM - 1]);
  if (F && tid < N * N) sF[tid] = F[tid];
  if (act) {
#pragma unroll
    for (int c = 0; c < NDIM; ++c) sb[c][tid] = u[c * nloc + l];
  }
  __syncthreads();
  double v[3] = {0.0, 0.0, 0.0};
  if (act) {
    double m[NDIM][NDIM];
    elem_inv_metric<N, NDIM>(sD, sb[NDIM], sb[NDIM + 1], sb[2 * NDIM - 1], tid, m);
    double g[NDIM][NDIM];                                        // g[c][a] = d u_c / d x_a
#pragma unroll
    for (int c = 0; c < NDIM; ++c) {
      double fd[NDIM];
      elem_ref_deriv<N, NDIM>(sD, sb[c], tid, fd);
#pragma unroll
      for (int a = 0; a < NDIM; ++a) {
        double s = 0.0;
#pragma unroll
        for (int q = 0; q < NDIM; ++q) s += m[q][a] * fd[q];
        g[c][a] = s;
      }
    }
    vortex_point<NDIM>(g, v);
  }
  if (F) {                                                       // (the same for every thread of the grid)
    const int i = tid % N, j = (tid / N) % N, k = NDIM == 3 ? tid / (N * N) : 0;
    // lines through this node: over i (stride 1), over j (stride N), over k (stride N * N)
    const int base[3] = {tid - i, NDIM == 3 ? k * N * N + i : i, j * N + i};
    const int stride[3] = {1, N, N * N};
    const int row[3] = {i, j, k};
#pragma unroll
    for (int dir = 0; dir < NDIM; ++dir) {
      __syncthreads();                                           // the reads of the gradients / of the last pass are over
      if (act) {
#pragma unroll
        for (int f = 0; f < 3; ++f) sb[f][tid] = v[f];
      }
      __syncthreads();
      if (act) {
#pragma unroll
        for (int f = 0; f < 3; ++f) {
          double t = 0.0;
#pragma unroll
          for (int q = 0; q < N; ++q) t += sF[row[dir] * N + q] * sb[f][base[dir] + q * stride[dir]];
          v[f] = t;
        }
      }
    }
  }
  if (!act) return;
  w[l] = v[0];
  w[nloc + l] = v[1];
  if constexpr (NDIM == 3) w[2 * nloc + l] = v[2];
  if (om) om[l] = v[2];
}

template <int N, int NDIM>
inline void launch_vortex(hipStream_t st, int nel, const double* D, const double* xyz, const double* u, const double* F, double* w,
                          double* om, long long nloc) {
  hipLaunchKernelGGL((k_vortex<N, NDIM>), dim3(nel), dim3(SensCfg<N, NDIM>::NT), 0, st, D, xyz, u, F, w, om, nloc);
}

}  // namespace sens
}  // namespace nsk
