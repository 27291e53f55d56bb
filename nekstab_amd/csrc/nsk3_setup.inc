// Set-up of a hexahedral (ndim = 3) context: geometry [UPSTREAM coef.f geom1/geom2, 3-D branches],
// gather-scatter tables, dt rule, Jacobi diagonals, element-wise fast-diagonalisation factors of
// E = D B^-1 D^T and the vertex coarse operator.  Included by nsk.hip.

// cyclic Jacobi eigen-decomposition of a small symmetric matrix: A = V diag(w) V^T
static void jacobi_eig(std::vector<double>& A, int n, std::vector<double>& V, std::vector<double>& w) {
  V.assign((size_t)n * n, 0.0);
  for (int i = 0; i < n; ++i) V[(size_t)i * n + i] = 1.0;
  for (int sweep = 0; sweep < 100; ++sweep) {
    double off = 0.0, diag = 0.0;
    for (int i = 0; i < n; ++i) for (int j = 0; j < n; ++j) (i == j ? diag : off) += A[(size_t)i * n + j] * A[(size_t)i * n + j];
    if (off <= 1e-30 * diag) break;
    for (int p = 0; p < n - 1; ++p)
      for (int q = p + 1; q < n; ++q) {
        const double apq = A[(size_t)p * n + q];
        if (apq == 0.0) continue;
        const double theta = (A[(size_t)q * n + q] - A[(size_t)p * n + p]) / (2.0 * apq);
        const double t = (theta >= 0 ? 1.0 : -1.0) / (std::fabs(theta) + std::sqrt(theta * theta + 1.0));
        const double cth = 1.0 / std::sqrt(t * t + 1.0), sth = t * cth;
        for (int k = 0; k < n; ++k) {
          const double akp = A[(size_t)k * n + p], akq = A[(size_t)k * n + q];
          A[(size_t)k * n + p] = cth * akp - sth * akq; A[(size_t)k * n + q] = sth * akp + cth * akq;
        }
        for (int k = 0; k < n; ++k) {
          const double apk = A[(size_t)p * n + k], aqk = A[(size_t)q * n + k];
          A[(size_t)p * n + k] = cth * apk - sth * aqk; A[(size_t)q * n + k] = sth * apk + cth * aqk;
        }
        for (int k = 0; k < n; ++k) {
          const double vkp = V[(size_t)k * n + p], vkq = V[(size_t)k * n + q];
          V[(size_t)k * n + p] = cth * vkp - sth * vkq; V[(size_t)k * n + q] = sth * vkp + cth * vkq;
        }
      }
  }
  w.resize(n);
  for (int i = 0; i < n; ++i) w[i] = A[(size_t)i * n + i];
}

// generalised symmetric eigenproblem A s = lambda B s, B SPD:  S^T B S = I,  S^T A S = diag(lam); S[row*n + mode]
static bool gen_eig(const std::vector<double>& A, const std::vector<double>& B, int n, std::vector<double>& S, std::vector<double>& lam) {
  std::vector<double> L((size_t)n * n, 0.0);
  for (int i = 0; i < n; ++i)
    for (int j = 0; j <= i; ++j) {
      double s = B[(size_t)i * n + j];
      for (int k = 0; k < j; ++k) s -= L[(size_t)i * n + k] * L[(size_t)j * n + k];
      if (i == j) { if (!(s > 0.0)) return false; L[(size_t)i * n + i] = std::sqrt(s); }
      else L[(size_t)i * n + j] = s / L[(size_t)j * n + j];
    }
  // C = L^-1 A L^-T
  std::vector<double> X((size_t)n * n), Cm((size_t)n * n);
  for (int c = 0; c < n; ++c)                        // X = L^-1 A (column by column)
    for (int i = 0; i < n; ++i) {
      double s = A[(size_t)i * n + c];
      for (int k = 0; k < i; ++k) s -= L[(size_t)i * n + k] * X[(size_t)k * n + c];
      X[(size_t)i * n + c] = s / L[(size_t)i * n + i];
    }
  for (int r = 0; r < n; ++r)                        // C^T = L^-1 X^T  => C[r][i]
    for (int i = 0; i < n; ++i) {
      double s = X[(size_t)r * n + i];
      for (int k = 0; k < i; ++k) s -= L[(size_t)i * n + k] * Cm[(size_t)r * n + k];
      Cm[(size_t)r * n + i] = s / L[(size_t)i * n + i];
    }
  for (int i = 0; i < n; ++i) for (int j = 0; j < i; ++j) { const double a = 0.5 * (Cm[(size_t)i * n + j] + Cm[(size_t)j * n + i]); Cm[(size_t)i * n + j] = Cm[(size_t)j * n + i] = a; }
  std::vector<double> V;
  jacobi_eig(Cm, n, V, lam);
  S.assign((size_t)n * n, 0.0);                      // S = L^-T V
  for (int m = 0; m < n; ++m)
    for (int i = n - 1; i >= 0; --i) {
      double s = V[(size_t)i * n + m];
      for (int k = i + 1; k < n; ++k) s -= L[(size_t)k * n + i] * S[(size_t)k * n + m];
      S[(size_t)i * n + m] = s / L[(size_t)i * n + i];
    }
  return true;
}

// ---- set-up: colour probing of A_c = R E R^T on the device (the probe vector of a colour, the E apply and the projection
// back on the vertex functions never leave the GPU; per colour only nvert doubles come back: at config 5's size the host
// version moved 2 x 407 MB over PCIe for each of its ~700 colours, 27 s of a 58 s set-up)
__global__ void k_probe_colour(const int* __restrict__ colour, const int* __restrict__ evert, const double* __restrict__ hat,
                               int MM, int cc, double* __restrict__ pv) {
  const long long e = blockIdx.x;
  __shared__ int on[8];
  if (threadIdx.x < 8) on[threadIdx.x] = colour[evert[e * 8 + threadIdx.x]] == cc;
  __syncthreads();
  for (int q = threadIdx.x; q < MM; q += blockDim.x) {
    double s = 0.0;
#pragma unroll
    for (int c = 0; c < 8; ++c) if (on[c]) s += hat[(size_t)c * MM + q];
    pv[e * MM + q] = s;
  }
}
// ec[e*8 + corner] = hat_corner . w_e   (one wavefront per corner; launch with 512 threads)
__global__ void k_corner_dots(const double* __restrict__ hat, const double* __restrict__ w, int MM, double* __restrict__ ec) {
  const long long e = blockIdx.x;
  const int c = threadIdx.x >> 6, lane = threadIdx.x & 63;
  double s = 0.0;
  for (int q = lane; q < MM; q += 64) s += hat[(size_t)c * MM + q] * w[e * MM + q];
  s = nsk::wave_sum63(s);
  if (lane == 63) ec[e * 8 + c] = s;
}
__global__ void k_vertex_gather(const int* __restrict__ v_off, const int* __restrict__ v_ent, const double* __restrict__ ec, int nvert,
                                double* __restrict__ rc) {
  const int v = blockIdx.x * 256 + threadIdx.x;
  if (v >= nvert) return;
  double s = 0.0;
  for (int k = v_off[v]; k < v_off[v + 1]; ++k) s += ec[v_ent[k]];
  rc[v] = s;
}

__global__ void k_coarse_restrict_csr(Dev d, double* __restrict__ rc) {
  if (d.gsc->done) return;
  const int v = blockIdx.x * 256 + threadIdx.x;
  if (v >= d.coarse_lda) return;
  double s = 0.0;
  if (v < d.nvert)
    for (int k = d.v_off[v]; k < d.v_off[v + 1]; ++k) s += d.ec[d.v_ent[k]];
  if (d.gs_lag && d.gsc->pending) s *= d.gsc->phinv;       // ec is the restriction of the un-normalised w' (k_gs_lag)
  rc[v] = s;
}

// One step of the Chebyshev-Jacobi coarse solve (sparse A_c, nvert rows):
//   first: r = b, x = 0, d = z/theta;   else: r -= A d_in (d_in complete from the previous launch), then
//   x += d_in,  z = D^-1 r,  d_out = c1 d_in + c2 z     (coefficients fixed => a linear operator)
// A_c is stored row-major with a fixed, padded row length wp (a multiple of 16; padding = (row, 0.0)) and SIXTEEN lanes
// share a row: they read 16 consecutive entries per step (coalesced) and are summed with DPP row shifts (a DPP row is 16
// lanes).  One thread per row walked its 49 entries serially, a dependent gather each: 93 us per launch at 51 k vertices
// (47 us in column-major ELL form); 16 lanes per row give the memory system 16x the loads in flight.
__global__ __launch_bounds__(256) void k_cheb_coarse(Dev d, int wp, const int* __restrict__ ci,
                                                     const double* __restrict__ va, const double* __restrict__ dinv,
                                                     const double* __restrict__ b, double* __restrict__ r,
                                                     const double* __restrict__ din, double* __restrict__ dout,
                                                     double c1, double c2, int first, int last) {
  if (d.gsc->done) return;
  const int u = blockIdx.x * 16 + (threadIdx.x >> 4), j = threadIdx.x & 15;
  if (u >= d.nvert) return;                            // the 16 lanes of a row leave together
  double t = 0.0;
  if (!first) {
    const size_t o = (size_t)u * wp + j;
    for (int k = 0; k < wp; k += 16) t += va[o + k] * din[ci[o + k]];
    t += dpp_get<0x111, 0xf>(t);                       // row_shr:1
    t += dpp_get<0x112, 0xf>(t);                       // row_shr:2
    t += dpp_get<0x114, 0xf>(t);                       // row_shr:4
    t += dpp_get<0x118, 0xf>(t);                       // row_shr:8 -> lane 15 of the row holds the row sum
  }
  if (j != 15) return;
  double ru, xu;
  if (first) { ru = b[u]; xu = 0.0; }
  else { ru = r[u] - t; xu = d.xc[u] + din[u]; }
  const double dn = (first ? 0.0 : c1 * din[u]) + c2 * dinv[u] * ru;
  r[u] = ru;
  dout[u] = dn;
  d.xc[u] = last ? xu + dn : xu;
}

// ---------------------------------------------------------------------------
// Block-circulant coarse solve.  Meshes that are a 2-D mesh extruded over nz uniform periodic layers (BASELINE config 4:
// the backward-facing step over 30 spanwise layers; the z-extruded cylinder) have a vertex operator that is invariant under
// a shift by one layer and under z-reflection:  A_c = sum_d C_|d| (x) P^d  with symmetric nv2 x nv2 blocks C_d.  The real
// Fourier transform in z block-diagonalises it:  B_m = sum_d C_|d| cos(2 pi m d / nz), m = 0 .. nz/2 (the cos and the sin
// column of a wavenumber share B_m), so the EXACT coarse solve is
//   r^[m] = sum_z F[z][m] r[., z]      (k_circ_fwd)
//   x^[m] = B_m^-1 r^[m]               (k_circ_solve: one pass over the (nz/2 + 1) stored fp32 inverses, both columns of a
//                                       wavenumber per matrix read)
//   x[., z] = sum_m F[z][m] x^[m]      (k_circ_bwd)
// -- three launches per GMRES iteration instead of the ~40-90 of the Chebyshev polynomial (19 % of config 4's kernel time).
// The structure is DETECTED from the probed sparse operator (no mesh flag in the C-ABI): see build3.
// ---------------------------------------------------------------------------
__global__ __launch_bounds__(256) void k_circ_fwd(Dev d, int nv2, int nz, const double* __restrict__ F, const double* __restrict__ rc,
                                                  double* __restrict__ rh) {
  if (d.gsc->done) return;
  const int v = blockIdx.x * 256 + threadIdx.x, m = blockIdx.y;
  if (v >= nv2) return;
  double s = 0.0;
  for (int z = 0; z < nz; ++z) s += F[z * nz + m] * rc[(size_t)z * nv2 + v];
  rh[(size_t)m * nv2 + v] = s;
}
// grid (ceil(nv2 / 4), nmat): one wavefront per matrix row; column m1 (and m2 >= 0) of the transformed right-hand side
__global__ __launch_bounds__(256) void k_circ_solve(Dev d, int nv2, int lda2, const float* __restrict__ Binv, const int2* __restrict__ cols,
                                                    const double* __restrict__ rh, double* __restrict__ xh) {
  if (d.gsc->done) return;
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
  const int row = blockIdx.x * 4 + w, mat = blockIdx.y;
  if (row >= nv2) return;
  const int2 cm = cols[mat];
  const float4* A = reinterpret_cast<const float4*>(Binv + ((size_t)mat * nv2 + row) * lda2) + lane;
  const double* r1 = rh + (size_t)cm.x * nv2;
  const double* r2 = rh + (size_t)(cm.y >= 0 ? cm.y : cm.x) * nv2;
  const int nit = lda2 / 256;
  double s1 = 0.0, s2 = 0.0;
#pragma unroll 4
  for (int i = 0; i < nit; ++i) {
    const float4 a = A[i * 64];
    const int c0 = i * 256 + lane * 4;
    double x1[4], x2[4];
#pragma unroll
    for (int q = 0; q < 4; ++q) { const bool in = c0 + q < nv2; x1[q] = in ? r1[c0 + q] : 0.0; x2[q] = in ? r2[c0 + q] : 0.0; }
    s1 += (double)a.x * x1[0] + (double)a.y * x1[1] + (double)a.z * x1[2] + (double)a.w * x1[3];
    s2 += (double)a.x * x2[0] + (double)a.y * x2[1] + (double)a.z * x2[2] + (double)a.w * x2[3];
  }
  s1 = wave_sum63(s1); s2 = wave_sum63(s2);
  if (lane == 63) {
    xh[(size_t)cm.x * nv2 + row] = s1;
    if (cm.y >= 0) xh[(size_t)cm.y * nv2 + row] = s2;
  }
}
__global__ __launch_bounds__(256) void k_circ_bwd(Dev d, int nv2, int nz, const double* __restrict__ F, const double* __restrict__ xh) {
  if (d.gsc->done) return;
  const int v = blockIdx.x * 256 + threadIdx.x, z = blockIdx.y;
  if (v >= nv2) return;
  double s = 0.0;
  for (int m = 0; m < nz; ++m) s += F[z * nz + m] * xh[(size_t)m * nv2 + v];
  d.xc[(size_t)z * nv2 + v] = s;
}
static int coarse_circulant(nsk_ctx* c, const double* rc) {
  const int nv2 = c->circ_nv2, nz = c->circ_nz;
  hipLaunchKernelGGL(k_circ_fwd, dim3((nv2 + 255) / 256, nz), dim3(256), 0, c->stream, c->d, nv2, nz, c->circ_F, rc, c->circ_rh);
  hipLaunchKernelGGL(k_circ_solve, dim3((nv2 + 3) / 4, c->circ_nmat), dim3(256), 0, c->stream, c->d, nv2, c->circ_lda, c->circ_Binv, c->circ_cols,
                     (const double*)c->circ_rh, c->circ_xh);
  hipLaunchKernelGGL(k_circ_bwd, dim3((nv2 + 255) / 256, nz), dim3(256), 0, c->stream, c->d, nv2, nz, c->circ_F, (const double*)c->circ_xh);
  return 0;
}

static int coarse_iterative(nsk_ctx* c, const double* rc) {
  if (c->circ_nz) return coarse_circulant(c, rc);
  // rho_0 = 1/sigma, d_0 = z_0/theta; rho_{k+1} = 1/(2 sigma - rho_k), d_{k+1} = rho_{k+1} rho_k d_k + (2 rho_{k+1}/delta) z_{k+1}
  const double sigma = c->cheb_theta / c->cheb_delta;
  double rho = 1.0 / sigma;
  double* din = c->cw_d0; double* dout = c->cw_d1;
  const unsigned grid = (unsigned)((c->d.nvert + 15) / 16);          // 16 rows per workgroup, 16 lanes per row
  for (int k = 0; k < c->cheb_deg; ++k) {
    double c1, c2;
    if (k == 0) { c1 = 0.0; c2 = 1.0 / c->cheb_theta; }
    else { const double rn = 1.0 / (2.0 * sigma - rho); c1 = rn * rho; c2 = 2.0 * rn / c->cheb_delta; rho = rn; }
    hipLaunchKernelGGL(k_cheb_coarse, dim3(grid), dim3(256), 0, c->stream, c->d, c->cA_width, c->cA_ci, c->cA_va, c->cA_dinv, rc, c->cw_r,
                       (const double*)din, dout, c1, c2, k == 0 ? 1 : 0, k == c->cheb_deg - 1 ? 1 : 0);
    std::swap(din, dout);
  }
  return 0;
}

// The coarse solve from the sparse rows of A_c (rows[u] = sorted (v, A_c(u, v)), all vertices): symmetrisation, then the
// block-circulant solve where the mesh is uniform periodic layers, the dense inverse for small vertex counts, the
// Chebyshev-Jacobi polynomial otherwise.  Called by build3 (single-rank set-up) and by nsk_local_finish (rank-local set-up:
// the rows of all ranks gathered).
static int coarse_build3(nsk_ctx* c, std::vector<std::vector<std::pair<int, double>>>& rows, bool has_outflow) {
  Dev& d = c->d;
  const int nvert = c->nvert, lda = c->coarse_lda;
  int rc;
  for (auto& r : rows) std::sort(r.begin(), r.end());
  auto entry = [&](int u, int v) -> double {
    const auto& r = rows[u];
    auto it = std::lower_bound(r.begin(), r.end(), std::make_pair(v, -1e300));
    return (it != r.end() && it->first == v) ? it->second : 0.0;
  };
  // symmetrise (E is symmetric; removes probing round-off)
  for (int u = 0; u < nvert; ++u)
    for (auto& uv : rows[u]) if (uv.first > u) { const double a = 0.5 * (uv.second + entry(uv.first, u)); uv.second = a; }
  for (int u = 0; u < nvert; ++u)
    for (auto& uv : rows[u]) if (uv.first < u) uv.second = entry(uv.first, u);
  const char* itenv = std::getenv("NSK_COARSE_ITER");
  const bool iterative = itenv ? std::atoi(itenv) != 0 : nvert > 12000;
  // ---- block-circulant structure (uniform periodic layers): exact coarse solve by a real Fourier transform in z
  // NSK_COARSE_CIRC: 1 = use it whenever the structure is there (tests), 0 = never, default = where the alternative is the polynomial
  bool circ_done = false;
  {
    const char* cenv = std::getenv("NSK_COARSE_CIRC");
    const bool want = cenv ? std::atoi(cenv) != 0 : iterative;
    int nzl = 0;
    if (want) {
      double dmax = 0.0;
      for (int u = 0; u < nvert; ++u) dmax = std::max(dmax, std::fabs(entry(u, u)));
      const double tolc = 1e-9 * dmax;
      for (int cand = nvert / 2; cand >= 3 && !nzl; --cand) {          // the largest layer count that passes
        if (nvert % cand) continue;
        const int nv2 = nvert / cand;
        if (nv2 < 4) continue;
        bool ok = true;
        // layer 0 against layers 1 and cand / 2 (shift invariance), reflection symmetry and block symmetry on layer 0
        for (int u = 0; u < nv2 && ok; ++u) {
          for (const auto& uv : rows[u]) {
            const int v2 = uv.first % nv2, dz = uv.first / nv2;
            for (int sh : {1, cand / 2}) {
              const int u2 = u + sh * nv2, w2 = v2 + ((dz + sh) % cand) * nv2;
              if (std::fabs(entry(u2, w2) - uv.second) > tolc) { ok = false; break; }
            }
            if (!ok) break;
            const int dzr = (cand - dz) % cand;                         // reflection: C_d = C_{-d}
            if (std::fabs(entry(u, v2 + dzr * nv2) - uv.second) > tolc) { ok = false; break; }
            if (std::fabs(entry(v2, u + dz * nv2) - uv.second) > tolc) { ok = false; break; }     // C_d symmetric
          }
          if (ok && (rows[u + nv2].size() != rows[u].size() || rows[u + (cand / 2) * nv2].size() != rows[u].size())) ok = false;
        }
        if (ok) nzl = cand;
      }
    }
    if (nzl >= 3) {
      const int nz = nzl, nv2 = nvert / nz, nmat = nz / 2 + 1;
      const int lda2 = ((nv2 + 255) / 256) * 256;
      // real orthonormal Fourier matrix F[z][col]: col 0 constant; 2m-1 / 2m = cos / sin of wavenumber m; last = alternating (nz even)
      std::vector<double> F((size_t)nz * nz);
      std::vector<int2> cols(nmat);
      const double PI = 3.14159265358979323846;
      for (int z = 0; z < nz; ++z) F[(size_t)z * nz] = 1.0 / std::sqrt((double)nz);
      cols[0] = make_int2(0, -1);
      int col = 1;
      for (int m = 1; m < nmat; ++m) {
        if (2 * m == nz) {
          for (int z = 0; z < nz; ++z) F[(size_t)z * nz + col] = ((z & 1) ? -1.0 : 1.0) / std::sqrt((double)nz);
          cols[m] = make_int2(col, -1); col += 1;
        } else {
          for (int z = 0; z < nz; ++z) {
            F[(size_t)z * nz + col] = std::sqrt(2.0 / nz) * std::cos(2.0 * PI * m * z / nz);
            F[(size_t)z * nz + col + 1] = std::sqrt(2.0 / nz) * std::sin(2.0 * PI * m * z / nz);
          }
          cols[m] = make_int2(col, col + 1); col += 2;
        }
      }
      float* dBinv = nullptr; double *dB = nullptr, *drow = nullptr, *dcol = nullptr;
      if ((rc = dalloc(c, &dBinv, (size_t)nmat * nv2 * lda2)) || (rc = dalloc(c, &dB, (size_t)nv2 * nv2)) || (rc = dalloc(c, &drow, nv2)) || (rc = dalloc(c, &dcol, nv2))) return rc;
      std::vector<double> B((size_t)nv2 * nv2);
      std::vector<float> Bf((size_t)nv2 * lda2);
      for (int m = 0; m < nmat; ++m) {
        std::fill(B.begin(), B.end(), 0.0);
        for (int u = 0; u < nv2; ++u)
          for (const auto& uv : rows[u]) {
            const int v2 = uv.first % nv2, dz = uv.first / nv2;
            B[(size_t)u * nv2 + v2] += uv.second * std::cos(2.0 * PI * m * dz / nz);
          }
        if (m == 0 && !has_outflow) {               // constant null space lives in wavenumber 0: shift it out (as the dense path does)
          double tr = 0; for (int v = 0; v < nv2; ++v) tr += B[(size_t)v * nv2 + v];
          const double shf = tr / nv2 / nv2;
          for (double& x : B) x += shf;
        }
        HIPCHK(hipMemcpy(dB, B.data(), B.size() * sizeof(double), hipMemcpyHostToDevice));
        for (int k = 0; k < nv2; ++k) {
          hipLaunchKernelGGL(k_gj_extract, dim3((nv2 + 255) / 256), dim3(256), 0, c->stream, (const double*)dB, nv2, k, drow, dcol);
          hipLaunchKernelGGL(k_gj_update, dim3((nv2 + 255) / 256, nv2), dim3(256), 0, c->stream, dB, nv2, k, (const double*)drow, (const double*)dcol);
        }
        HIPCHK(hipStreamSynchronize(c->stream));
        HIPCHK(hipMemcpy(B.data(), dB, B.size() * sizeof(double), hipMemcpyDeviceToHost));
        std::fill(Bf.begin(), Bf.end(), 0.0f);
        for (int r = 0; r < nv2; ++r) for (int q = 0; q < nv2; ++q) Bf[(size_t)r * lda2 + q] = (float)B[(size_t)r * nv2 + q];
        HIPCHK(hipMemcpy(dBinv + (size_t)m * nv2 * lda2, Bf.data(), Bf.size() * sizeof(float), hipMemcpyHostToDevice));
      }
      { nsk_vec a = dB, b2 = drow, c2 = dcol; nsk_vec_free(c, 1, &a); nsk_vec_free(c, 1, &b2); nsk_vec_free(c, 1, &c2); }
      c->circ_nz = nz; c->circ_nv2 = nv2; c->circ_nmat = nmat; c->circ_lda = lda2; c->circ_Binv = dBinv;
      if ((rc = dupload(c, &c->circ_F, F)) || (rc = dupload(c, &c->circ_cols, cols)) || (rc = dalloc_mut(c, &c->circ_rh, (size_t)nz * nv2)) ||
          (rc = dalloc_mut(c, &c->circ_xh, (size_t)nz * nv2))) return rc;
      c->coarse_iter = 1;                                   // same call sites as the polynomial (coarse_iterative dispatches)
      c->coarse_bytes = 4.0 * nmat * nv2 * lda2 + 8.0 * (2.0 * nz * nz + 4.0 * nz * nv2);      // stored inverses (fp32) + the two z-transforms
      d.Aci = nullptr; d.Acif = nullptr;
      circ_done = true;
      if (std::getenv("NSK_DEBUG")) fprintf(stderr, "coarse: %d vertices = %d layers x %d: block-circulant solve, %d stored inverses (%.0f MB fp32)\n", nvert, nz, nv2, nmat, 4e-6 * nmat * nv2 * lda2);
    }
  }
  if (circ_done) {
  } else if (!iterative) {
    // dense inverse (Gauss-Jordan on the device): O(nvert^2) memory, fine up to ~10^4 vertices
    std::vector<double> Ac((size_t)nvert * nvert, 0.0);
    for (int u = 0; u < nvert; ++u) for (auto& uv : rows[u]) Ac[(size_t)u * nvert + uv.first] = uv.second;
    if (!has_outflow) {
      double tr = 0; for (int v = 0; v < nvert; ++v) tr += Ac[(size_t)v * nvert + v];
      const double sh = tr / nvert / nvert;
      for (size_t k = 0; k < Ac.size(); ++k) Ac[k] += sh;
    }
    double* dA = nullptr; double *drow = nullptr, *dcol = nullptr;
    if ((rc = dalloc(c, &dA, Ac.size())) || (rc = dalloc(c, &drow, nvert)) || (rc = dalloc(c, &dcol, nvert))) return rc;
    HIPCHK(hipMemcpy(dA, Ac.data(), Ac.size() * sizeof(double), hipMemcpyHostToDevice));
    for (int k = 0; k < nvert; ++k) {
      hipLaunchKernelGGL(k_gj_extract, dim3((nvert + 255) / 256), dim3(256), 0, c->stream, (const double*)dA, nvert, k, drow, dcol);
      hipLaunchKernelGGL(k_gj_update, dim3((nvert + 255) / 256, nvert), dim3(256), 0, c->stream, dA, nvert, k, (const double*)drow, (const double*)dcol);
    }
    HIPCHK(hipStreamSynchronize(c->stream));
    d.Aci = dA;
    std::vector<double> Ah(Ac.size());
    HIPCHK(hipMemcpy(Ah.data(), dA, Ah.size() * sizeof(double), hipMemcpyDeviceToHost));
    std::vector<float> Af((size_t)nvert * lda, 0.0f);
    for (int r = 0; r < nvert; ++r) for (int q = 0; q < nvert; ++q) Af[(size_t)r * lda + q] = (float)Ah[(size_t)r * nvert + q];
    if ((rc = dupload(c, &d.Acif, Af))) return rc;
    c->coarse_bytes = 4.0 * nvert * lda + 16.0 * nvert;
  } else {
    // large coarse spaces: sparse A_c (CSR) + a fixed-degree Chebyshev-Jacobi polynomial as the (linear) coarse
    // solve.  Spectrum bounds of D^-1 A from a host Lanczos run; the degree makes the polynomial reduce the
    // error by 10x on [lmin, lmax] (below lmin it still contracts, only more slowly).
    std::vector<int> rp(nvert + 1, 0), ci;
    std::vector<double> va, dinvc(nvert);
    for (int u = 0; u < nvert; ++u) {
      for (auto& uv : rows[u]) { ci.push_back(uv.first); va.push_back(uv.second); if (uv.first == u) dinvc[u] = 1.0 / uv.second; }
      rp[u + 1] = (int)ci.size();
    }
    auto spmv = [&](const std::vector<double>& x, std::vector<double>& y) {
      for (int u = 0; u < nvert; ++u) { double t = 0; for (int k = rp[u]; k < rp[u + 1]; ++k) t += va[k] * x[ci[k]]; y[u] = t; }
    };
    // Lanczos on D^-1/2 A D^-1/2
    const int mL = std::min(60, nvert - 1);
    std::vector<double> qv(nvert), qp(nvert, 0.0), wv2(nvert), tmp(nvert), al, be;
    { double nn = 0; for (int u = 0; u < nvert; ++u) { qv[u] = std::sin(0.37 * u + 1.0) + 0.5 * std::cos(1.3 * u); nn += qv[u] * qv[u]; }
      nn = std::sqrt(nn); for (double& x : qv) x /= nn; }
    double bprev = 0.0;
    for (int it = 0; it < mL; ++it) {
      for (int u = 0; u < nvert; ++u) tmp[u] = qv[u] * std::sqrt(dinvc[u]);
      spmv(tmp, wv2);
      double a2 = 0;
      for (int u = 0; u < nvert; ++u) { wv2[u] = wv2[u] * std::sqrt(dinvc[u]) - bprev * qp[u]; a2 += wv2[u] * qv[u]; }
      double b2 = 0;
      for (int u = 0; u < nvert; ++u) { wv2[u] -= a2 * qv[u]; b2 += wv2[u] * wv2[u]; }
      b2 = std::sqrt(b2);
      al.push_back(a2); be.push_back(b2);
      if (!(b2 > 1e-14)) break;
      for (int u = 0; u < nvert; ++u) { qp[u] = qv[u]; qv[u] = wv2[u] / b2; }
      bprev = b2;
    }
    const int mt = (int)al.size();
    std::vector<double> T((size_t)mt * mt, 0.0), Vt, ev;
    for (int i = 0; i < mt; ++i) { T[(size_t)i * mt + i] = al[i]; if (i + 1 < mt) T[(size_t)i * mt + i + 1] = T[(size_t)(i + 1) * mt + i] = be[i]; }
    jacobi_eig(T, mt, Vt, ev);
    std::sort(ev.begin(), ev.end());
    double lmax = 1.05 * ev.back(), lmin = ev[0];
    if (!has_outflow && mt > 1 && lmin < 1e-8 * lmax) lmin = ev[1];   // constant null space: smallest non-zero one
    lmin = std::max(0.7 * lmin, 1e-4 * lmax);
    const double theta = 0.5 * (lmax + lmin), delta = 0.5 * (lmax - lmin), sigma = theta / delta;
    // error reduction of the polynomial: 1/4 (NSK_CHEB_RED overrides).  A cheaper, less exact coarse solve trades launches
    // per GMRES iteration against GMRES iterations; measured at config 4's size, ms per time step / pressure iterations per
    // step: 1/20: 99.5 / 8.8, 1/8: 98.4 / 9.8, 1/4: 94.7 / 10.2, 1/3: 95.0 / 10.7, 1/2: 101.8 / 13.7; a 24^3 box of
    // config 5's family: 242.9 -> 234.4 ms at the same 34 iterations.
    double red = 4.0;
    if (const char* g = std::getenv("NSK_CHEB_RED")) red = std::max(2.0, std::atof(g));
    int deg = (int)std::ceil(std::acosh(red) / std::acosh(sigma));
    deg = std::max(4, std::min(deg, 96));
    c->cheb_deg = deg; c->cheb_theta = theta; c->cheb_delta = delta;
    int width = 0;
    for (int u = 0; u < nvert; ++u) width = std::max(width, rp[u + 1] - rp[u]);
    width = ((width + 15) / 16) * 16;                    // padded row length: 16 lanes per row read 16 entries per step
    std::vector<int> eci((size_t)width * nvert);
    std::vector<double> eva((size_t)width * nvert, 0.0);
    for (int u = 0; u < nvert; ++u)
      for (int k = 0; k < width; ++k) {
        const bool in = rp[u] + k < rp[u + 1];
        eci[(size_t)u * width + k] = in ? ci[rp[u] + k] : u;
        if (in) eva[(size_t)u * width + k] = va[rp[u] + k];
      }
    c->cA_width = width;
    if ((rc = dupload(c, &c->cA_rp, rp)) || (rc = dupload(c, &c->cA_ci, eci)) || (rc = dupload(c, &c->cA_va, eva)) ||
        (rc = dupload(c, &c->cA_dinv, dinvc)) || (rc = dalloc_mut(c, &c->cw_d0, lda)) || (rc = dalloc_mut(c, &c->cw_d1, lda)) ||
        (rc = dalloc_mut(c, &c->cw_r, lda))) return rc;
    c->coarse_iter = 1;
    c->coarse_bytes = (double)deg * ((double)width * nvert * 12.0 + 5.0 * 8.0 * nvert);       // per degree: padded rows (value + column) + five vectors
    d.Aci = nullptr; d.Acif = nullptr;
    if (std::getenv("NSK_DEBUG")) fprintf(stderr, "coarse: %d vertices, %zu nnz, D^-1A in [%.3e, %.3e], Chebyshev degree %d\n", nvert, va.size(), lmin, lmax, deg);
  }
  return 0;
}

// host loops over elements (geometry, Jacobi diagonals, fast-diagonalisation factors: 1e8 points at config 5's size) on up to 16 threads
template <class F>
static void parallel_elems(int nel, F&& fn) {
  const int nth = std::max(1, std::min<int>(16, (int)std::thread::hardware_concurrency()));
  auto run = [&](int t) {
    const int lo = (int)((long long)nel * t / nth), hi = (int)((long long)nel * (t + 1) / nth);
    for (int e = lo; e < hi; ++e) fn(e);
  };
  std::vector<std::thread> pool;
  for (int t = 1; t < nth; ++t) pool.emplace_back(run, t);
  run(0);
  for (auto& th : pool) th.join();
}

static int build3(nsk_ctx* c, const nsk_case& cs) {
  const int N = cs.lx1, NN = N * N * N, M = N - 2, MM = M * M * M, ND = cs.lxd > 0 ? cs.lxd : 3 * N / 2, NDD = ND * ND * ND;
  if (!(N == 6 || N == 8 || N == 10)) return fail(NSK_EINVAL, "3-D: lx1 must be 6, 8 or 10 in this build");
  if (ND != 3 * N / 2) return fail(NSK_EINVAL, "lxd must be 3*lx1/2");
  if (!cs.z || !cs.wb) return fail(NSK_EINVAL, "3-D case needs z and wb");
  const int nel = cs.nel;
  nsk_setup::SectionTimer tick;
  c->key = 100 + N; c->hrows = 12; c->hstride = 16;
  if (const char* g = std::getenv("NSK_ZERO_METRICS")) c->zero_metrics = std::atoi(g);
  int rc;
  if ((rc = build_open(c, cs, 3, 1))) return rc;
  c->NT = ((NN + 63) / 64) * 64; c->NTD = c->NT;
  c->layers = 0;
  const long long nloc = c->nloc, npr = c->npr;
  const size_t nfine = (size_t)nel * NDD;
  Dev& d = c->d;
  d.nfine = (long long)nfine; d.use_tot = 1;

  std::vector<double> z1, w1, z2, w2, zd, wd;
  zwgll(N, z1, w1); zwgl(M, z2, w2); zwgl(ND, zd, wd);
  std::vector<double> D = deriv_matrix(z1), J12 = interp_matrix(z1, z2), Jd = interp_matrix(z1, zd), Dd = deriv_matrix(zd);
  std::vector<double> D12 = matmul(J12, D, M, N, N);
  std::vector<double> hat((size_t)8 * MM + 2 * M);       // + the 1-D factors [2][M] behind the eight vertex functions (k_schwarz_p builds the products itself)
  for (int a = 0; a < M; ++a) { hat[(size_t)8 * MM + a] = 0.5 * (1 - z2[a]); hat[(size_t)8 * MM + M + a] = 0.5 * (1 + z2[a]); }
  for (int cc = 0; cc < M; ++cc)
    for (int b = 0; b < M; ++b)
      for (int a = 0; a < M; ++a)
        for (int v = 0; v < 8; ++v) {
          const double hr = (v & 1) ? 0.5 * (1 + z2[a]) : 0.5 * (1 - z2[a]);
          const double hs = (v & 2) ? 0.5 * (1 + z2[b]) : 0.5 * (1 - z2[b]);
          const double ht = (v & 4) ? 0.5 * (1 + z2[cc]) : 0.5 * (1 - z2[cc]);
          hat[(size_t)v * MM + (cc * M + b) * M + a] = hr * hs * ht;
        }
  if ((rc = dupload(c, &d.D, D)) || (rc = dupload(c, &d.J12, J12)) || (rc = dupload(c, &d.D12, D12)) ||
      (rc = dupload(c, &d.Jd, Jd)) || (rc = dupload(c, &d.Dd, Dd)) || (rc = dupload(c, &d.hat, hat))) return rc;

  // ---- geometry
  std::vector<double> G[6], bm1(nloc), jac(nloc), met[9];
  for (auto& g : G) g.resize(nloc);
  for (auto& m : met) m.resize(nloc);
  // Structural zeros of the mapping (Nek5000 skips the cross terms of its undeformed elements by flag -- ifdfrm, hmholtz.f axhelm --;
  // here: by array).  A derivative d x_q / d xi_a that is rounding noise on EVERY node of the mesh (a spanwise-extruded mesh:
  // x_t, y_t, z_r, z_s; a box mesh: all six off-diagonal ones) is set to zero exactly.  The metric terms, G factors and
  // dealiasing-mesh metrics built from it are then exact zeros over whole arrays, and Dev::zmask tells the kernels not to load them.
  bool dx_zero[3][3] = {{false, false, false}, {false, false, false}, {false, false, false}};
  {
    const double* X[3] = {cs.x, cs.y, cs.z};
    if (c->zero_metrics) {
      std::vector<double> emax((size_t)nel * 9, 0.0);
      parallel_elems(nel, [&](int e) {
        double mx[9] = {0, 0, 0, 0, 0, 0, 0, 0, 0};
        for (int k = 0; k < N; ++k)
          for (int j = 0; j < N; ++j)
            for (int i = 0; i < N; ++i) {
              const size_t o = (size_t)e * NN;
              for (int q = 0; q < 3; ++q) {
                double r = 0, s = 0, t = 0;
                for (int m = 0; m < N; ++m) {
                  r += D[i * N + m] * X[q][o + (k * N + j) * N + m];
                  s += D[j * N + m] * X[q][o + (k * N + m) * N + i];
                  t += D[k * N + m] * X[q][o + (m * N + j) * N + i];
                }
                mx[q * 3 + 0] = std::max(mx[q * 3 + 0], std::fabs(r)); mx[q * 3 + 1] = std::max(mx[q * 3 + 1], std::fabs(s)); mx[q * 3 + 2] = std::max(mx[q * 3 + 2], std::fabs(t));
              }
            }
        for (int q = 0; q < 9; ++q) emax[(size_t)e * 9 + q] = mx[q];
      });
      double gm[9] = {0, 0, 0, 0, 0, 0, 0, 0, 0}, scale = 0.0;
      for (int e = 0; e < nel; ++e)
        for (int q = 0; q < 9; ++q) gm[q] = std::max(gm[q], emax[(size_t)e * 9 + q]);
      for (int q = 0; q < 9; ++q) scale = std::max(scale, gm[q]);
      for (int q = 0; q < 9; ++q) dx_zero[q / 3][q % 3] = gm[q] <= 1e-11 * scale;
    }
    std::atomic<int> bad_el{-1};
    parallel_elems(nel, [&](int e) {
      for (int k = 0; k < N; ++k)
        for (int j = 0; j < N; ++j)
          for (int i = 0; i < N; ++i) {
            const size_t o = (size_t)e * NN, l = o + (k * N + j) * N + i;
            double dx[3][3];                         // dx[coord][axis]
            for (int q = 0; q < 3; ++q) {
              double r = 0, s = 0, t = 0;
              for (int m = 0; m < N; ++m) {
                r += D[i * N + m] * X[q][o + (k * N + j) * N + m];
                s += D[j * N + m] * X[q][o + (k * N + m) * N + i];
                t += D[k * N + m] * X[q][o + (m * N + j) * N + i];
              }
              dx[q][0] = dx_zero[q][0] ? 0.0 : r; dx[q][1] = dx_zero[q][1] ? 0.0 : s; dx[q][2] = dx_zero[q][2] ? 0.0 : t;
            }
            const double xr = dx[0][0], xs = dx[0][1], xt = dx[0][2], yr = dx[1][0], ys = dx[1][1], yt = dx[1][2],
                         zr = dx[2][0], zs = dx[2][1], zt = dx[2][2];
            const double J = xr * ys * zt + xt * yr * zs + xs * yt * zr - xr * yt * zs - xs * yr * zt - xt * ys * zr;
            if (!(J > 0.0)) { bad_el = e; return; }
            const double m9[9] = {ys * zt - yt * zs, xt * zs - xs * zt, xs * yt - xt * ys,
                                  yt * zr - yr * zt, xr * zt - xt * zr, xt * yr - xr * yt,
                                  yr * zs - ys * zr, xs * zr - xr * zs, xr * ys - xs * yr};
            for (int q = 0; q < 9; ++q) met[q][l] = m9[q];
            jac[l] = J;
            const double W = w1[i] * w1[j] * w1[k];
            bm1[l] = J * W;
            auto dot = [&](int a, int b) { return (m9[a * 3] * m9[b * 3] + m9[a * 3 + 1] * m9[b * 3 + 1] + m9[a * 3 + 2] * m9[b * 3 + 2]) * W / J; };
            G[0][l] = dot(0, 0); G[1][l] = dot(1, 1); G[2][l] = dot(2, 2); G[3][l] = dot(0, 1); G[4][l] = dot(0, 2); G[5][l] = dot(1, 2);
          }
    });
    if (bad_el >= 0) return fail(NSK_EINVAL, "non-positive Jacobian in element " + std::to_string((int)bad_el));
    // bit q < 9: metric term q (Gauss-mesh w2m[q], dealiasing-mesh mtd[q]) is zero on every node; bit 9 + m: G factor 4 + m is
    d.zmask = 0;
    if (c->zero_metrics) {
      auto all_zero = [&](const std::vector<double>& v) { for (double x : v) if (x != 0.0) return false; return true; };
      for (int q = 0; q < 9; ++q) if (all_zero(met[q])) d.zmask |= 1u << q;
      for (int m = 0; m < 3; ++m) if (all_zero(G[3 + m])) d.zmask |= 1u << (9 + m);
    }
    c->zmask_built = d.zmask;
  }
  auto interp3 = [&](const std::vector<double>& Jm, int nt, const double* f, double* out, std::vector<double>& ta, std::vector<double>& tb) {
    ta.resize((size_t)N * N * nt); tb.resize((size_t)N * nt * nt);
    for (int kj = 0; kj < N * N; ++kj)
      for (int a = 0; a < nt; ++a) { double s = 0; for (int i = 0; i < N; ++i) s += Jm[a * N + i] * f[kj * N + i]; ta[(size_t)kj * nt + a] = s; }
    for (int k = 0; k < N; ++k)
      for (int b = 0; b < nt; ++b)
        for (int a = 0; a < nt; ++a) { double s = 0; for (int j = 0; j < N; ++j) s += Jm[b * N + j] * ta[((size_t)k * N + j) * nt + a]; tb[((size_t)k * nt + b) * nt + a] = s; }
    for (int cc = 0; cc < nt; ++cc)
      for (int ba = 0; ba < nt * nt; ++ba) { double s = 0; for (int k = 0; k < N; ++k) s += Jm[cc * N + k] * tb[(size_t)k * nt * nt + ba]; out[(size_t)cc * nt * nt + ba] = s; }
  };
  // Dealiasing-mesh metrics: 9 x nfine doubles (24 GB at config 5's size) -- built in element chunks and uploaded as they
  // are made, so that the host never holds more than one chunk of them.
  std::vector<double> w2m((size_t)9 * npr);
  {
    double* dmtd = nullptr;
    if ((rc = dalloc(c, &dmtd, (size_t)9 * nfine))) return rc;
    d.mtd = dmtd;
    const int CH = 2048;
    std::vector<double> chunk((size_t)9 * CH * NDD);
    const int nthr = (int)std::max(1u, std::min(16u, std::thread::hardware_concurrency()));
    for (int e0 = 0; e0 < nel; e0 += CH) {
      const int ne = std::min(CH, nel - e0);
      auto work = [&](int t) {                               // elements e0 + t, e0 + t + nthr, ... of this chunk
        std::vector<double> ta, tb, o2(MM), od(NDD);
        for (int e = e0 + t; e < e0 + ne; e += nthr)
          for (int q = 0; q < 9; ++q) {
            interp3(J12, M, met[q].data() + (size_t)e * NN, o2.data(), ta, tb);
            for (int cc = 0; cc < M; ++cc) for (int b = 0; b < M; ++b) for (int a = 0; a < M; ++a)
              w2m[(size_t)q * npr + (size_t)e * MM + (cc * M + b) * M + a] = o2[(cc * M + b) * M + a] * w2[a] * w2[b] * w2[cc];
            interp3(Jd, ND, met[q].data() + (size_t)e * NN, od.data(), ta, tb);
            for (int cc = 0; cc < ND; ++cc) for (int b = 0; b < ND; ++b) for (int a = 0; a < ND; ++a)
              chunk[((size_t)q * CH + (e - e0)) * NDD + (cc * ND + b) * ND + a] = od[(cc * ND + b) * ND + a] * wd[a] * wd[b] * wd[cc];
          }
      };
      std::vector<std::thread> pool;
      for (int t = 1; t < nthr; ++t) pool.emplace_back(work, t);
      work(0);
      for (auto& th : pool) th.join();
      for (int q = 0; q < 9; ++q)
        HIPCHK(hipMemcpy(dmtd + (size_t)q * nfine + (size_t)e0 * NDD, chunk.data() + (size_t)q * CH * NDD, (size_t)ne * NDD * sizeof(double), hipMemcpyHostToDevice));
    }
  }

  tick("bases + geometry");
  // ---- gather-scatter CSR from the global numbering
  std::vector<int> gs_off, gs_idx;
  nsk_setup::gs_csr(cs.gid, nloc, gs_off, gs_idx);
  if ((rc = dupload(c, &d.gs_tab, gs_table(gs_off, gs_idx))) || (rc = dupload(c, &d.gs_corner, nsk_setup::corner_table(N, nel, gs_off, gs_idx)))) return rc;
  auto dssum_h = [&](const std::vector<double>& f) { return nsk_setup::dssum_h(gs_off, gs_idx, f); };
  // (component masks, nsk_init_masks: mask and binv [3][nloc], component mc from the caller's cmask[mc], cs.mask is not read; behind
  //  them what the <.., CM = true> kernel forms load -- nsk3_kernels.hpp, cm_bits: the three masks of a node as the bits of a 32-bit
  //  word behind mask, the unmasked 1 / B as a fourth row of binv)
  const int nmc = c->cm ? 3 : 1;
  if (c->cm && c->local) return fail(NSK_EINVAL, "component masks: not with a rank-local set-up");
  std::vector<double> mask((size_t)nmc * nloc + (c->cm ? (nloc + 1) / 2 : 0)), minv(nloc), binv((size_t)(c->cm ? 4 : 1) * nloc), spng(cs.spng, cs.spng + nloc), bm1s(nloc);
  std::vector<double> bs = dssum_h(bm1);
  {
    double vol = 0;
    int* bits = c->cm ? reinterpret_cast<int*>(mask.data() + (size_t)3 * nloc) : nullptr;
    for (long long l = 0; l < nloc; ++l) {
      // a node fixed in any copy is fixed in all
      double mk = 1.0;
      if (c->cm) {
        int fb = 0;
        for (int mc = 0; mc < 3; ++mc) {
          double m = 1.0;
          for (int k = gs_off[l]; k < gs_off[l + 1]; ++k) m = std::min(m, c->cmask_in[mc][gs_idx[k]]);
          mask[(size_t)mc * nloc + l] = m;
          binv[(size_t)mc * nloc + l] = m / bs[l];
          if (m != 0.0) fb |= 1 << mc;
        }
        bits[l] = fb;
        binv[(size_t)3 * nloc + l] = 1.0 / bs[l];
      } else {
        for (int k = gs_off[l]; k < gs_off[l + 1]; ++k) mk = std::min(mk, cs.mask[gs_idx[k]]);
        mask[l] = mk;
        binv[l] = mk / bs[l];
      }
      minv[l] = 1.0 / (gs_off[l + 1] - gs_off[l]);
      bm1s[l] = (spng[l] != 0.0) ? 0.0 : bm1[l];
      vol += bm1[l];
      if (c->local && c->local_own[l / NN]) c->vol_own += bm1[l];
    }
    d.vol = vol;
  }
  c->bm1s_host = bm1s;

  tick("gather-scatter tables, masks");
  // ---- dt rule  (core/matvec.f:26-46, [UPSTREAM compute_cfl] 3-D)
  c->cfl_target = cs.cfl;
  {
    c->h_cflg.resize((size_t)9 * nloc);
    const std::vector<double> dri = nsk_setup::dri_table(z1);
    const double* U[3] = {cs.ub, cs.vb, cs.wb};
    double ctarg = 0;
    for (int e = 0; e < nel; ++e)
      for (int k = 0; k < N; ++k)
        for (int j = 0; j < N; ++j)
          for (int i = 0; i < N; ++i) {
            const size_t l = (size_t)e * NN + (k * N + j) * N + i;
            const int idx[3] = {i, j, k};
            double s = 0;
            for (int a = 0; a < 3; ++a) {
              double t = 0;
              for (int q = 0; q < 3; ++q) {
                const double f = met[a * 3 + q][l] / jac[l] * dri[idx[a]];
                c->h_cflg[9 * l + a * 3 + q] = f;
                t += U[q][l] * f;
              }
              s += std::fabs(t);
            }
            ctarg = std::max(ctarg, s);
          }
    if (!(ctarg > 0.0)) return fail(NSK_EINVAL, "base flow is zero");
    c->ctarg = ctarg;
    const double dt = cs.cfl / ctarg;
    c->nsteps = (int)std::ceil(cs.endtime / dt);
    c->dt = cs.endtime / c->nsteps;
    d.dt = c->dt;
  }
  for (auto& m : met) std::vector<double>().swap(m);         // 9 x nloc host doubles (7 GB at config 5's size): done with them
  std::vector<double>().swap(jac);

  // ---- Jacobi preconditioner of H
  std::vector<double> dinv((size_t)3 * nloc);
  {
    std::vector<double> dA(nloc);
    parallel_elems(nel, [&](int e) {
      for (int k = 0; k < N; ++k)
        for (int j = 0; j < N; ++j)
          for (int i = 0; i < N; ++i) {
            const size_t o = (size_t)e * NN, l = o + (k * N + j) * N + i;
            double s = 0;
            for (int m = 0; m < N; ++m)
              s += D[m * N + i] * D[m * N + i] * G[0][o + (k * N + j) * N + m] + D[m * N + j] * D[m * N + j] * G[1][o + (k * N + m) * N + i] +
                   D[m * N + k] * D[m * N + k] * G[2][o + (m * N + j) * N + i];
            s += 2.0 * (D[i * N + i] * D[j * N + j] * G[3][l] + D[i * N + i] * D[k * N + k] * G[4][l] + D[j * N + j] * D[k * N + k] * G[5][l]);
            dA[l] = s;
          }
    });
    std::vector<double> dAs = dssum_h(dA);
    c->h_dAs = dAs; c->h_bs = bs; c->h_mask.assign(mask.begin(), mask.begin() + (size_t)nmc * nloc);
    const double bd0[3] = {1.0, 1.5, 11.0 / 6.0};
    for (int k = 0; k < 3; ++k)      // (component masks: the unmasked diagonal, as jacobi_diagonals rebuilds it)
      for (long long l = 0; l < nloc; ++l) dinv[(size_t)k * nloc + l] = (c->cm ? 1.0 : mask[l]) / (d.nu * dAs[l] + bd0[k] / c->dt * bs[l]);
  }
  // (component masks: `mask` and `binv` are uploaded WHOLE -- [3][nloc] plus the packed words / the unmasked fourth row that the CM
  //  kernel forms read, nsk3_kernels.hpp cm_bits; code that slices or copies Dev::mask / Dev::binv by [nmc][nloc] would lose that tail:
  //  nsk_clone takes quadrilaterals only and the shards refuse such a context, see there)
  if ((rc = dupload(c, &d.g1, G[0])) || (rc = dupload(c, &d.g2, G[1])) || (rc = dupload(c, &d.g3, G[2])) ||
      (rc = dupload(c, &d.g4, G[3])) || (rc = dupload(c, &d.g5, G[4])) || (rc = dupload(c, &d.g6, G[5])) ||
      (rc = dupload(c, &d.bm1, bm1)) || (rc = dupload(c, &d.mask, mask)) || (rc = dupload(c, &d.minv, minv)) ||
      (rc = dupload(c, &d.binv, binv)) || (rc = dupload(c, &d.spng, spng)) || (rc = dupload(c, &d.bm1s, bm1s)) ||
      (rc = dupload(c, &d.dinv, dinv)) || (rc = dupload(c, &d.w2m, w2m)) ||
      (rc = dupload(c, &d.gs_off, gs_off)) || (rc = dupload(c, &d.gs_idx, gs_idx))) return rc;
  d.nl_spng_str = 0.0; d.spng_vr = nullptr; d.bstep = nullptr; d.bf_stride = 0;
  for (auto& g : G) std::vector<double>().swap(g);           // uploaded: free the host copies before the big device allocations
  std::vector<double>().swap(w2m); std::vector<double>().swap(dinv);

  tick("dt rule, Jacobi diagonals, uploads");
  // ---- state + solver work arrays
  double* bfc = nullptr;
  if ((rc = dalloc(c, &bfc, (size_t)12 * nfine))) return rc;
  d.bfc = bfc; d.cUr = bfc;                                         // nsk_set_baseflow writes through cUr
  if ((rc = alloc_core_state(c, 3, d.cs, d.ps, npr, nel, c->nblk, 8, d.nproj_max)) || (rc = alloc_totals(c)) || (rc = dalloc_mut(c, &d.dpw, npr)) ||
      (rc = alloc_scratch(c, 3, d.cs, npr))) return rc;

  tick("work arrays");
  // ---- base-flow constants on the dealiasing mesh (device)
  {
    double* xyz = nullptr;                                 // GLL coordinates for nsk_seed_noise
    if ((rc = dalloc(c, &xyz, (size_t)3 * nloc))) return rc;
    HIPCHK(hipMemcpy(xyz, cs.x, nloc * sizeof(double), hipMemcpyHostToDevice));
    HIPCHK(hipMemcpy(xyz + nloc, cs.y, nloc * sizeof(double), hipMemcpyHostToDevice));
    HIPCHK(hipMemcpy(xyz + 2 * nloc, cs.z, nloc * sizeof(double), hipMemcpyHostToDevice));
    c->xyz = xyz;
  }
  HIPCHK(hipMemcpy(c->scratch, cs.ub, nloc * sizeof(double), hipMemcpyHostToDevice));
  HIPCHK(hipMemcpy(c->scratch + nloc, cs.vb, nloc * sizeof(double), hipMemcpyHostToDevice));
  HIPCHK(hipMemcpy(c->scratch + 2 * nloc, cs.wb, nloc * sizeof(double), hipMemcpyHostToDevice));
  DISPATCH_N(c->key, {
    hipLaunchKernelGGL(k_baseflow<N>, dim3(nel), dim3(Cfg<N>::NTD), 0, c->stream, d, (const double*)c->scratch, bfc, nullptr, nullptr, nullptr, nullptr, nullptr);
  });
  if ((rc = scan_bfmask(c))) return rc;

  tick("base-flow constants (dealiasing mesh)");
  // ---- fast-diagonalisation factors of the overlapping Schwarz patches of E: element + one Gauss layer of every
  // face neighbour = an lx1^3 tensor grid (the neighbours' layers arrive through the velocity-mesh gather tables,
  // which also resolves their orientation).  Per element and direction the 1-D operators A = D B^-1 D^T and
  // M = J B^-1 J^T of the three-element line (neighbour, element, neighbour) restricted to the patch;
  // E_patch ~ M_t x M_s x A_r + M_t x A_s x M_r + A_t x M_s x M_r   [UPSTREAM hsmg.f: same idea, Nek solves a Laplacian]
  {
    const int P = N;
    std::vector<double> fdS((size_t)nel * 3 * P * P), fdL((size_t)nel * 3 * P);
    const double* X[3] = {cs.x, cs.y, cs.z};
    // element lengths per direction and face data
    std::vector<double> Ld((size_t)nel * 3), rho((size_t)nel * 6);
    std::vector<int> nbr_el((size_t)nel * 6, -1), nbr_ax((size_t)nel * 6, 0);
    for (int e = 0; e < nel; ++e) {
      const size_t o = (size_t)e * NN;
      for (int a = 0; a < 3; ++a) {
        const int st = (a == 0) ? 1 : (a == 1 ? N : N * N);
        const int s1 = (a == 0) ? N : 1, s2 = (a == 2) ? N : N * N;
        double L = 0.0, rlo = 0.0, rhi = 0.0; int nf = 0;
        // component masks: the ratio of the component along the face's normal (the one D B^-1 D^T couples across the face) -- the
        // coordinate that varies least over the face; a boundary face that fixes only some components is planar and axis-aligned,
        // on every other face the three masks agree
        size_t clo = 0, chi = 0;
        if (c->cm)
          for (int side = 0; side < 2; ++side) {
            double best = 0.0; int comp = 0;
            for (int x = 0; x < 3; ++x) {
              double mn = 1e300, mx = -1e300;
              for (int p = 0; p < N; ++p)
                for (int q = 0; q < N; ++q) {
                  const double v = X[x][o + (size_t)p * s1 + (size_t)q * s2 + (size_t)(side ? N - 1 : 0) * st];
                  mn = std::min(mn, v); mx = std::max(mx, v);
                }
              if (x == 0 || mx - mn < best) { best = mx - mn; comp = x; }
            }
            (side ? chi : clo) = (size_t)comp * nloc;
          }
        for (int p = 0; p < N; ++p)
          for (int q = 0; q < N; ++q) {
            const size_t lo = o + (size_t)p * s1 + (size_t)q * s2, hi = lo + (size_t)(N - 1) * st;
            double d2 = 0; for (int x = 0; x < 3; ++x) d2 += (X[x][hi] - X[x][lo]) * (X[x][hi] - X[x][lo]);
            L += std::sqrt(d2);
            if (p > 0 && p < N - 1 && q > 0 && q < N - 1) { rlo += binv[clo + lo] * bm1[lo]; rhi += binv[chi + hi] * bm1[hi]; ++nf; }
          }
        Ld[(size_t)e * 3 + a] = L / (N * N);
        rho[(size_t)e * 6 + 2 * a] = rlo / nf; rho[(size_t)e * 6 + 2 * a + 1] = rhi / nf;
        for (int side = 0; side < 2; ++side) {                      // face-centre node -> the other copy
          const size_t l = o + (size_t)(N / 2) * s1 + (size_t)(N / 2) * s2 + (size_t)(side ? N - 1 : 0) * st;
          if (gs_off[l + 1] - gs_off[l] != 2) continue;
          const int other = (gs_idx[gs_off[l]] == (int)l) ? gs_idx[gs_off[l] + 1] : gs_idx[gs_off[l]];
          const int f = other / NN, nd = other % NN;
          if (f == e) continue;
          const int idx[3] = {nd % N, (nd / N) % N, nd / (N * N)};
          int ax = -1;
          for (int x = 0; x < 3; ++x) if (idx[x] == 0 || idx[x] == N - 1) ax = x;
          nbr_el[(size_t)e * 6 + 2 * a + side] = f; nbr_ax[(size_t)e * 6 + 2 * a + side] = ax;
        }
      }
    }
    double lmax = 0.0;
    std::vector<double> lamsum_el(nel, 0.0);
    std::atomic<int> fd_bad{-1};
    parallel_elems(nel, [&](int e) {
      std::vector<double> A, Bm, S, lam;
      double lamsum = 0.0;
      for (int a = 0; a < 3; ++a) {
        const int flo = nbr_el[(size_t)e * 6 + 2 * a], fhi = nbr_el[(size_t)e * 6 + 2 * a + 1];
        const double L0 = Ld[(size_t)e * 3 + a];
        // line of up to three elements: [lo] own [hi]
        double len[3]; int present[3] = {flo >= 0, 1, fhi >= 0};
        len[0] = flo >= 0 ? Ld[(size_t)flo * 3 + nbr_ax[(size_t)e * 6 + 2 * a]] : 0.0;
        len[1] = L0;
        len[2] = fhi >= 0 ? Ld[(size_t)fhi * 3 + nbr_ax[(size_t)e * 6 + 2 * a + 1]] : 0.0;
        const int nvn = 3 * (N - 1) + 1;                            // velocity nodes of the full line
        std::vector<double> bl(nvn, 0.0), bi(nvn, 0.0);
        for (int el = 0; el < 3; ++el)
          if (present[el]) for (int i = 0; i < N; ++i) bl[el * (N - 1) + i] += 0.5 * len[el] * w1[i];
        for (int n = 0; n < nvn; ++n) bi[n] = bl[n] > 0.0 ? 1.0 / bl[n] : 0.0;
        if (present[0]) bi[0] *= 0.5;                               // far ends: assume the line continues
        if (present[2]) bi[nvn - 1] *= 0.5;
        bi[(N - 1)] = rho[(size_t)e * 6 + 2 * a] / (0.5 * L0 * w1[0]);            // the element's own end nodes: true
        bi[2 * (N - 1)] = rho[(size_t)e * 6 + 2 * a + 1] / (0.5 * L0 * w1[N - 1]);  // assembled / masked mass ratio
        // patch dofs: (el, a): lo last Gauss, own all, hi first Gauss
        int pel[24], pa[24];
        pel[0] = 0; pa[0] = M - 1;
        for (int q = 0; q < M; ++q) { pel[1 + q] = 1; pa[1 + q] = q; }
        pel[P - 1] = 2; pa[P - 1] = 0;
        A.assign((size_t)P * P, 0.0); Bm.assign((size_t)P * P, 0.0);
        for (int r = 0; r < P; ++r)
          for (int q = 0; q < P; ++q) {
            if (!present[pel[r]] || !present[pel[q]]) continue;
            if (pel[r] != pel[q] && std::abs(pel[r] - pel[q]) > 1) continue;
            double sa = 0, sb = 0;
            for (int i = 0; i < N; ++i)
              for (int i2 = 0; i2 < N; ++i2) {
                if (pel[r] * (N - 1) + i != pel[q] * (N - 1) + i2) continue;      // same velocity node of the line
                const double b = bi[pel[r] * (N - 1) + i];
                sa += w2[pa[r]] * D12[pa[r] * N + i] * b * w2[pa[q]] * D12[pa[q] * N + i2];
                sb += 0.5 * len[pel[r]] * w2[pa[r]] * J12[pa[r] * N + i] * b * 0.5 * len[pel[q]] * w2[pa[q]] * J12[pa[q] * N + i2];
              }
            A[(size_t)r * P + q] = sa; Bm[(size_t)r * P + q] = sb;
          }
        for (int r = 0; r < P; ++r)
          if (!present[pel[r]]) { A[(size_t)r * P + r] = 1.0; Bm[(size_t)r * P + r] = 1.0; }     // inert slot (no neighbour)
        if (!gen_eig(A, Bm, P, S, lam)) { fd_bad = e; return; }
        for (int q = 0; q < P * P; ++q) fdS[((size_t)e * 3 + a) * P * P + q] = S[q];
        double lm = 0;
        for (int q = 0; q < P; ++q) { fdL[((size_t)e * 3 + a) * P + q] = lam[q]; lm = std::max(lm, lam[q]); }
        lamsum += lm;
      }
      lamsum_el[e] = lamsum;
    });
    if (fd_bad >= 0) return fail(NSK_EINVAL, "fast-diagonalisation set-up failed in element " + std::to_string((int)fd_bad));
    for (int e = 0; e < nel; ++e)
      if (!c->local || c->local_own[e]) lmax = std::max(lmax, lamsum_el[e]);     // (rank-local: the outer ring has no neighbours)
    c->fd_lmax = lmax;
    d.fd_eps = 1e-11 * lmax;
    // ---- velocity solves: element-block fast-diagonalisation preconditioner (k_helm_fa / k_helm_fb), where the cells are
    // anisotropic enough for it to pay: option "helm_fdm" (-1: from the largest ratio of an element's lengths, >= 12; config 5: 29)
    {
      double aspect = 1.0;
      for (int e = 0; e < nel; ++e) {
        const double a0 = Ld[(size_t)e * 3], a1 = Ld[(size_t)e * 3 + 1], a2 = Ld[(size_t)e * 3 + 2];
        aspect = std::max(aspect, std::max(a0, std::max(a1, a2)) / std::min(a0, std::min(a1, a2)));
      }
      if (const char* g = std::getenv("NSK_HELM_FDM")) c->helm_fdm = std::atoi(g);
      // Measured (round 4): NOT a gain.  Blocks without overlap plateau at the element interfaces: 24^3 box (cell ratio 15) 26 against
      // 36 Jacobi iterations per step at 1.7x the cost per iteration (115 against 106 ms per step); config 5 at full size (ratio 29)
      // 49 against 64 iterations, 1.32 against 1.17 s per step.  Kept as an option (NSK_HELM_FDM=1 / "helm_fdm"), never chosen by itself.
      if (c->cm && c->helm_fdm > 0) return fail(NSK_EINVAL, "helm_fdm (NSK_HELM_FDM): k_helm_fa / k_helm_fb have no component-mask form (context of nsk_init_masks)");
      const bool on = !c->local && c->helm_fdm > 0;
      if (std::getenv("NSK_DEBUG")) fprintf(stderr, "velocity solves: largest element aspect ratio %.1f -> %s\n", aspect, on ? "fast-diagonalisation blocks" : "Jacobi");
      d.helm_fdm = 0;
      if (on) {
        std::vector<double> A1((size_t)N * N, 0.0);                   // 1-D stiffness on [-1, 1]: D^T W D
        for (int p = 0; p < N; ++p)
          for (int q = 0; q < N; ++q) { double s = 0; for (int i = 0; i < N; ++i) s += w1[i] * D[(size_t)i * N + p] * D[(size_t)i * N + q]; A1[(size_t)p * N + q] = s; }
        std::vector<double> hfS((size_t)nel * 3 * N * N, 0.0), hfL((size_t)nel * 3 * N, 1.0);
        std::atomic<int> bad{-1};
        parallel_elems(nel, [&](int e) {
          const size_t o = (size_t)e * NN;
          for (int a = 0; a < 3; ++a) {
            const int st = (a == 0) ? 1 : (a == 1 ? N : N * N);
            const int s1 = (a == 0) ? N : 1, s2 = (a == 2) ? N : N * N;
            const double L = Ld[(size_t)e * 3 + a];
            bool dir[2];
            for (int side = 0; side < 2; ++side)                      // a wall face: its centre node is masked
              dir[side] = cs.mask[o + (size_t)(N / 2) * s1 + (size_t)(N / 2) * s2 + (size_t)(side ? N - 1 : 0) * st] == 0.0;
            const int i0 = dir[0] ? 1 : 0, i1 = dir[1] ? N - 1 : N, n = i1 - i0;
            std::vector<double> A((size_t)n * n), B((size_t)n * n, 0.0), S, lam;
            for (int p = 0; p < n; ++p) {
              for (int q = 0; q < n; ++q) A[(size_t)p * n + q] = (2.0 / L) * A1[(size_t)(p + i0) * N + (q + i0)];
              B[(size_t)p * n + p] = 0.5 * L * w1[p + i0];
            }
            if (!gen_eig(A, B, n, S, lam)) { bad = e; return; }
            for (int p = 0; p < n; ++p)
              for (int m = 0; m < n; ++m) hfS[((size_t)e * 3 + a) * N * N + (size_t)(p + i0) * N + m] = S[(size_t)p * n + m];
            for (int m = 0; m < n; ++m) hfL[((size_t)e * 3 + a) * N + m] = lam[m];      // (modes n .. N-1: zero columns, eigenvalue 1)
          }
        });
        if (bad >= 0) return fail(NSK_EINVAL, "velocity fast-diagonalisation set-up failed in element " + std::to_string((int)bad));
        const double amin = std::getenv("NSK_HELM_FDM_ASPECT") ? std::atof(std::getenv("NSK_HELM_FDM_ASPECT")) : 0.0;      // (0: every element a block -- mixing Jacobi pieces in for the isotropic elements was measured WORSE than either pure form: 53-74 against 26 / 36 iterations on a 24^3 box)
        std::vector<int> hfT(nel, 0);
        int nblock = 0;
        for (int e = 0; e < nel; ++e) {
          const double a0 = Ld[(size_t)e * 3], a1 = Ld[(size_t)e * 3 + 1], a2 = Ld[(size_t)e * 3 + 2];
          hfT[e] = std::max(a0, std::max(a1, a2)) / std::min(a0, std::min(a1, a2)) >= amin ? 1 : 0;
          nblock += hfT[e];
        }
        if (std::getenv("NSK_DEBUG")) fprintf(stderr, "velocity solves: %d of %d elements take a fast-diagonalisation block (aspect ratio >= %.1f)\n", nblock, nel, amin);
        if ((rc = dupload(c, &d.hfT, hfT))) return rc;
        if ((rc = dupload(c, &d.hfS, hfS)) || (rc = dupload(c, &d.hfL, hfL)) || (rc = dalloc_mut(c, &d.hz, 3 * d.cs)) || (rc = dalloc_mut(c, &d.hy, 3 * d.cs))) return rc;
        d.helm_fdm = 1;
      }
    }
    if ((rc = dupload(c, &d.fdS, fdS)) || (rc = dupload(c, &d.fdL, fdL))) return rc;
    // patch gather table: pressure dof behind every position of the lx1^3 patch (-1: none).  Face positions take the
    // face neighbour's adjacent Gauss layer, edge / corner positions the diagonal neighbours' (a box patch fed with
    // zeros there loses the Schwarz convergence: measured 28 -> 200+ iterations on a 27-element box).
    std::vector<int> sw((size_t)nloc, -1);
    auto gmap = [&](int n) { return n == 0 ? 0 : (n == N - 1 ? M - 1 : n - 1); };
    auto dof_of = [&](int other) {
      const int f = other / NN, nd = other % NN;
      return f * MM + (gmap(nd / (N * N)) * M + gmap((nd / N) % N)) * M + gmap(nd % N);
    };
    std::vector<std::vector<int>> edgeNbr(nel);
    auto is_face_nbr = [&](int e, int f) { for (int q = 0; q < 6; ++q) if (nbr_el[(size_t)e * 6 + q] == f) return true; return false; };
    for (int pass = 0; pass < 2; ++pass)
      for (int e = 0; e < nel; ++e)
        for (int nd = 0; nd < NN; ++nd) {
          const int i = nd % N, j = (nd / N) % N, k = nd / (N * N);
          const int nend = (i == 0 || i == N - 1) + (j == 0 || j == N - 1) + (k == 0 || k == N - 1);
          const size_t l = (size_t)e * NN + nd;
          if (pass == 0 && nend == 0) { sw[l] = e * MM + ((k - 1) * M + (j - 1)) * M + (i - 1); continue; }
          if ((pass == 0 && (nend == 0 || nend == 3)) || (pass == 1 && nend != 3)) continue;
          int found = -1, cnt = 0;
          for (int q = gs_off[l]; q < gs_off[l + 1]; ++q) {
            const int other = gs_idx[q], f = other / NN;
            if (f == e) continue;
            if (nend >= 2 && is_face_nbr(e, f)) continue;
            if (nend == 3 && std::find(edgeNbr[e].begin(), edgeNbr[e].end(), f) != edgeNbr[e].end()) continue;
            found = other; ++cnt;
          }
          if (cnt != 1) continue;
          if (nend == 1 && !is_face_nbr(e, found / NN)) continue;
          if (nend == 2 && std::find(edgeNbr[e].begin(), edgeNbr[e].end(), found / NN) == edgeNbr[e].end()) edgeNbr[e].push_back(found / NN);
          sw[l] = dof_of(found);
        }
    if ((rc = dupload(c, &d.p_idx, sw))) return rc;
    c->h_pidx = sw; c->PS = NN;                           // element sharding: patch positions -> global pressure dofs
  }

  tick("fast-diagonalisation factors + patch tables");
  // ---- coarse space: trilinear vertex functions; A_c = R E R^T probed through the device E-apply
  const int nvert = (int)cs.nvert;
  c->nvert = nvert; d.nvert = nvert;
  std::vector<int> evert((size_t)nel * 8);
  for (size_t k = 0; k < evert.size(); ++k) {
    evert[k] = (int)cs.vert[k];
    if (evert[k] < 0 || evert[k] >= nvert) return fail(NSK_EINVAL, "vertex id out of range");
  }
  std::vector<int> v_off(nvert + 1, 0), v_ent((size_t)nel * 8);
  for (size_t k = 0; k < evert.size(); ++k) v_off[evert[k] + 1]++;
  for (int v = 0; v < nvert; ++v) v_off[v + 1] += v_off[v];
  { std::vector<int> pos(v_off.begin(), v_off.end() - 1); for (size_t k = 0; k < evert.size(); ++k) v_ent[pos[evert[k]]++] = (int)k; }
  c->h_evert = evert;
  const int lda = ((nvert + 255) / 256) * 256;
  d.coarse_lda = lda; c->coarse_lda = lda;
  if ((rc = dupload(c, &d.v_off, v_off)) || (rc = dupload(c, &d.v_ent, v_ent)) || (rc = dupload(c, &d.evert, evert)) ||
      (rc = dalloc_mut(c, &d.xc, nvert)) || (rc = dalloc_mut(c, &c->rc_big, lda))) return rc;
  d.vtab = nullptr; d.p_inv = nullptr; d.p_stride = 0;
  {
    // vertex graph: neighbours share an element
    std::vector<std::vector<int>> vnb(nvert);
    for (int e = 0; e < nel; ++e)
      for (int a = 0; a < 8; ++a)
        for (int b = 0; b < 8; ++b) if (a != b) vnb[evert[e * 8 + a]].push_back(evert[e * 8 + b]);
    for (auto& v : vnb) { std::sort(v.begin(), v.end()); v.erase(std::unique(v.begin(), v.end()), v.end()); }
    auto bfs = [&](int v0, int depth, std::vector<int>& out, std::vector<int>& mark, int stamp) {
      out.clear(); out.push_back(v0); mark[v0] = stamp;
      size_t head = 0;
      for (int dd = 0; dd < depth; ++dd) {
        const size_t tail = out.size();
        for (; head < tail; ++head)
          for (int u : vnb[out[head]]) if (mark[u] != stamp) { mark[u] = stamp; out.push_back(u); }
      }
    };
    std::vector<int> colour(nvert, -1), mark(nvert, -1), reach;
    int ncolour = 0;
    std::vector<char> used;
    for (int v = 0; v < nvert; ++v) {
      bfs(v, 4, reach, mark, v);
      used.assign(ncolour + 1, 0);
      for (int u : reach) if (colour[u] >= 0) used[colour[u]] = 1;
      int cc = 0;
      while (cc < ncolour && used[cc]) ++cc;
      colour[v] = cc;
      if (cc == ncolour) ++ncolour;
    }
    // sparse rows of A_c: for every probed column v the entries (u, v), u within two vertex hops
    std::vector<std::vector<std::pair<int, double>>> rows(nvert);
    std::vector<double> rcol(nvert);
    const int* dcolour = nullptr;
    if ((rc = dupload(c, &dcolour, colour))) return rc;
    std::vector<std::vector<int>> of_colour(ncolour);
    for (int v = 0; v < nvert; ++v) of_colour[colour[v]].push_back(v);
    std::fill(mark.begin(), mark.end(), -1);
    for (int cc = 0; cc < ncolour; ++cc) {
      // probe vector = sum of the vertex functions of this colour; w = E probe; column entries (u, v) = hat_u . w for the vertices u
      // within two hops of the one probed vertex v they can see (distance-4 colouring)
      hipLaunchKernelGGL(k_probe_colour, dim3(nel), dim3(256), 0, c->stream, dcolour, d.evert, d.hat, MM, cc, c->wp1);
      if ((rc = eapply(c, c->wp1, c->wp2))) return rc;
      hipLaunchKernelGGL(k_corner_dots, dim3(nel), dim3(512), 0, c->stream, d.hat, (const double*)c->wp2, MM, d.ec);
      hipLaunchKernelGGL(k_vertex_gather, dim3((nvert + 255) / 256), dim3(256), 0, c->stream, d.v_off, d.v_ent, (const double*)d.ec, nvert, c->rc_big);
      HIPCHK(hipMemcpyAsync(rcol.data(), c->rc_big, (size_t)nvert * sizeof(double), hipMemcpyDeviceToHost, c->stream));
      HIPCHK(hipStreamSynchronize(c->stream));
      for (int v : of_colour[cc]) {
        bfs(v, 2, reach, mark, nvert + v);
        for (int u : reach) rows[u].push_back({v, rcol[u]});
      }
    }
    { nsk_vec a = (void*)dcolour; nsk_vec_free(c, 1, &a); }
    for (auto& r : rows) std::sort(r.begin(), r.end());
    if (c->local) {
      // rank-local set-up: keep the rows of the vertices this rank owns (lowest element at the vertex is its own: every element
      // at such a vertex, the neighbours E couples them to and the assembled mass of their nodes are inside the two rings)
      for (int u = 0; u < nvert; ++u) {
        if (v_off[u + 1] == v_off[u] || !c->local_own[v_ent[v_off[u]] / 8]) continue;
        for (auto& uv : rows[u]) { c->crow_u.push_back(u); c->crow_v.push_back(uv.first); c->crow_a.push_back(uv.second); }
      }
    } else if ((rc = coarse_build3(c, rows, cs.has_outflow != 0))) return rc;
  }
  tick("coarse operator probed + coarse solve built");
  c->lb.reset_to_caps(false);
  d.proj_reset = 1;       // hexahedra: a map that starts from the previous map's projection space needs 15-20 % more Helmholtz iterations (DESIGN section 8)
  env_overrides(c);
  if (c->cm) {
    // component masks (nsk_init_masks): k_divgs_w has no such form.  Asked for through the environment: refused.
    const char* dw = std::getenv("NSK_DIVGS_WAVE");
    if (c->eapply_pipe == 3 || (dw && std::atoi(dw) != 0))
      return fail(NSK_EINVAL, "NSK_EAPPLY_PIPE=3 / NSK_DIVGS_WAVE: the wavefront divergence kernel (k_divgs_w) has no component-mask form (context of nsk_init_masks)");
  }
  HIPCHK(hipStreamSynchronize(c->stream));
  return 0;
}
