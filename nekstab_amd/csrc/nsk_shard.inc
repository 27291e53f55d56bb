// ===========================================================================
// Element sharding (SURVEY 8(e)): one shard = the elements of one rank, cut out of a full-mesh
// parent context whose set-up (geometry, Jacobi diagonal, Schwarz patches, coarse inverse) is
// replicated.  Exchange steps of one time step:
//   * dssum halo: per (peer, shared global node) the rank's partial sum -> peer's ghost slot
//     (k_halo_pack / transport / k_halo_unpack); the gather tables of interface nodes include
//     the ghost slots, so the consuming kernels are unchanged;
//   * Schwarz overlap halo of the current GMRES basis vector;
//   * all-reduce of the dot-product totals and of the coarse-grid restriction.
// Transport: loop-back copies between virtual ranks of one process (what the 1-GPU tests run)
// or RCCL send/recv + all-reduce between processes (nsk_comm_init_rccl).
// ===========================================================================
#include <dlfcn.h>
// RCCL is bound at run time (dlopen) so that the library has no link-time dependency on it and
// shares whichever librccl the process already loaded (PyTorch-ROCm's copy when torch is imported).
namespace rccl_rt {
typedef struct { char internal[128]; } UniqueId;
typedef void* Comm;
enum { kDouble = 8, kSum = 0 };                      // ncclFloat64, ncclSum
static void* lib = nullptr;
static int (*GetUniqueId)(UniqueId*) = nullptr;
static int (*CommInitRank)(Comm*, int, UniqueId, int) = nullptr;
static int (*CommDestroy)(Comm) = nullptr;
static int (*Send)(const void*, size_t, int, int, Comm, hipStream_t) = nullptr;
static int (*Recv)(void*, size_t, int, int, Comm, hipStream_t) = nullptr;
static int (*AllReduce)(const void*, void*, size_t, int, int, Comm, hipStream_t) = nullptr;
static int (*GroupStart)() = nullptr;
static int (*GroupEnd)() = nullptr;
static bool load() {
  if (lib) return true;
  const char* names[] = {"librccl.so.1", "librccl.so", "/opt/rocm/lib/librccl.so.1", "/opt/rocm/lib/librccl.so"};
  for (const char* n : names) { lib = dlopen(n, RTLD_NOW | RTLD_GLOBAL); if (lib) break; }
  if (!lib) return false;
#define RS(sym, name) *(void**)(&sym) = dlsym(lib, name); if (!sym) { lib = nullptr; return false; }
  RS(GetUniqueId, "ncclGetUniqueId"); RS(CommInitRank, "ncclCommInitRank"); RS(CommDestroy, "ncclCommDestroy");
  RS(Send, "ncclSend"); RS(Recv, "ncclRecv"); RS(AllReduce, "ncclAllReduce"); RS(GroupStart, "ncclGroupStart"); RS(GroupEnd, "ncclGroupEnd");
#undef RS
  return true;
}
}  // namespace rccl_rt
#define NSK_WITH_RCCL 1
#define ncclGroupStart rccl_rt::GroupStart
#define ncclGroupEnd rccl_rt::GroupEnd
#define ncclSend rccl_rt::Send
#define ncclRecv rccl_rt::Recv
#define ncclAllReduce rccl_rt::AllReduce
#define ncclDouble rccl_rt::kDouble
#define ncclSum rccl_rt::kSum
typedef rccl_rt::Comm ncclComm_t;
// every RCCL call is checked: a failed send / recv / all-reduce comes back as NSK_EHIP from the call that issued it
#define RCCLCHK(x)                                                                                         \
  do {                                                                                                     \
    int r_ = (x);                                                                                          \
    if (r_ != 0) return fail(NSK_EHIP, std::string(#x) + ": RCCL error " + std::to_string(r_) + " @" + std::to_string(__LINE__)); \
  } while (0)

typedef nsk::LoopPack PtrPack;

template <class T>
static int slice_elems(nsk_ctx* c, nsk_ctx* P, const T* src, const T** dst, const int* d_elems, int nel, int per) {
  T* q = nullptr;
  int rc = dalloc(c, &q, (size_t)nel * per);
  if (rc) return rc;
  const long long n = (long long)nel * per;
  hipLaunchKernelGGL(k_slice_elems<T>, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, P->stream, src, q, d_elems, nel, per);
  *dst = q;
  return 0;
}

static int shard_fill(nsk_ctx* c, nsk_ctx* P, const int* part, int rank, int nranks, const long long* eglob);
static int shard_create(nsk_ctx* P, const int* part, int rank, int nranks, nsk_ctx** out, const long long* eglob = nullptr) {
  if (nranks < 1 || nranks > 16) return fail(NSK_EINVAL, "nranks must be 1..16");
  if (P->parent) return fail(NSK_EINVAL, "parent must be a full-mesh context");
  if (rank < 0 || rank >= nranks) return fail(NSK_EINVAL, "rank outside 0..nranks-1");
  for (int e = 0; e < P->nel; ++e)
    if (part[e] < 0 || part[e] >= nranks) return fail(NSK_EINVAL, "part[" + std::to_string(e) + "] outside 0..nranks-1");
  nsk_ctx* c = new nsk_ctx();
  int rcs = shard_fill(c, P, part, rank, nranks, eglob);
  if (rcs) { std::string keep = g_err; nsk_finalize(c); g_err = keep; return rcs; }     // no leaked context / device arrays on a failed creation
  *out = c;
  return 0;
}

// eglob (rank-local set-up, nsk_shard_create_local): P covers a sub-mesh, eglob[e] = global id of its element e (ascending).
// Everything two ranks must order identically is then keyed by GLOBAL ids: velocity-interface nodes by their gslib id (as
// always), pressure-halo dofs by global element id * lx2^dim + node.
static int shard_fill(nsk_ctx* c, nsk_ctx* P, const int* part, int rank, int nranks, const long long* eglob) {
  const int N = P->N, NN = P->NN, MM = P->MM, NDD = P->NDD, PS = P->PS;
  c->parent = P; c->rank = rank; c->nranks = nranks;
  c->N = N; c->NN = NN; c->M = P->M; c->MM = MM; c->ND = P->ND; c->NDD = NDD; c->EPB = P->EPB; c->NT = P->NT; c->NTD = P->NTD;
  c->ndim = P->ndim; c->key = P->key;
  // (Dev::use_tot is cleared below: shards take the all-reduced totals path)
  c->dt = P->dt; c->re = P->re; c->endtime = P->endtime; c->nsteps = P->nsteps;
  c->lb.max_helm = P->lb.max_helm; c->lb.max_pres = P->lb.max_pres; c->lb.min_pres = P->lb.min_pres; c->layers = P->layers;
  c->helm_guess = P->helm_guess; c->early_pres_mul = P->early_pres_mul; c->use_graph = P->use_graph; c->PS = PS; c->coarse_lda = P->coarse_lda;
  c->coarse_iter = P->coarse_iter; c->cA_width = P->cA_width; c->cheb_deg = P->cheb_deg; c->cheb_theta = P->cheb_theta; c->cheb_delta = P->cheb_delta;
  c->cA_rp = P->cA_rp; c->cA_ci = P->cA_ci; c->cA_va = P->cA_va; c->cA_dinv = P->cA_dinv;      // replicated coarse operator (shared)
  c->circ_nz = P->circ_nz; c->circ_nv2 = P->circ_nv2; c->circ_nmat = P->circ_nmat; c->circ_lda = P->circ_lda;       // block-circulant coarse solve (replicated)
  c->circ_Binv = P->circ_Binv; c->circ_F = P->circ_F; c->circ_cols = P->circ_cols; c->circ_rh = P->circ_rh; c->circ_xh = P->circ_xh;
  c->cw_d0 = P->cw_d0; c->cw_d1 = P->cw_d1; c->cw_r = P->cw_r;                                    // work vectors: ranks of one process run in stream order
  c->stream = P->stream;                                   // virtual ranks share the parent's stream
  c->lb.reset_to_caps(false);
  // local element order: BOUNDARY elements (a node of theirs is shared with another rank) first, interior elements behind, each
  // group in ascending global id -- so that the workgroups whose results travel in the halo are the first ones of a launch
  // (halo / interior overlap of the velocity solve, group_step)
  // which ranks touch each global node (the dssum interface below and the boundary / interior split here)
  long long ng = 0;
  for (long long g : P->h_gid) ng = std::max(ng, g + 1);
  std::vector<unsigned> rmask(ng, 0u);
  for (int e = 0; e < P->nel; ++e)
    for (int nd2 = 0; nd2 < P->NN; ++nd2) rmask[P->h_gid[(size_t)e * P->NN + nd2]] |= 1u << part[e];
  int n_boundary = 0;
  {
    std::vector<int> own;
    for (int e = 0; e < P->nel; ++e) if (part[e] == rank) own.push_back(e);
    if (own.empty()) return fail(NSK_EINVAL, "empty shard");
    std::vector<int> inner;
    for (int e : own) {
      bool bnd = false;
      for (int nd2 = 0; nd2 < NN && !bnd; ++nd2) bnd = (rmask[P->h_gid[(size_t)e * NN + nd2]] & ~(1u << rank)) != 0;
      if (bnd) c->elems.push_back(e); else inner.push_back(e);
    }
    n_boundary = (int)c->elems.size();
    c->elems.insert(c->elems.end(), inner.begin(), inner.end());
  }
  const int nel = (int)c->elems.size();
  c->nbb = (n_boundary + c->EPB - 1) / c->EPB;
  for (int e : c->elems) c->elems_glob.push_back(eglob ? eglob[e] : (long long)e);
  std::vector<int> g2l(P->nel, -1);
  for (int le = 0; le < nel; ++le) g2l[c->elems[le]] = le;
  c->nel = nel; c->nblk = (nel + c->EPB - 1) / c->EPB; c->nvert = P->nvert;
  const int nd = P->ndim, NCORN = (nd == 3) ? 8 : 4;
  c->hrows = P->hrows; c->hstride = P->hstride;
  c->nloc = (long long)nel * NN; c->npr = (long long)nel * MM; c->nstate = nd * c->nloc + c->npr;
  const long long nloc = c->nloc, npr = c->npr;
  int rc;

  // ---- dssum interface (rmask: which ranks touch each global node, above)
  std::map<long long, std::vector<int>> loc_of;            // interface gid -> local nodes (ascending)
  std::vector<long long> lgid(nloc);
  for (int le = 0; le < nel; ++le)
    for (int nd = 0; nd < NN; ++nd) {
      const long long g = P->h_gid[(size_t)c->elems[le] * NN + nd];
      lgid[(size_t)le * NN + nd] = g;
      if (rmask[g] & ~(1u << rank)) loc_of[g].push_back(le * NN + nd);
    }
  std::vector<int> vh_off(1, 0), vh_idx;
  std::map<std::pair<int, long long>, int> slot;           // (peer, gid) -> ghost slot
  for (int p = 0; p < nranks; ++p) {
    if (p == rank) continue;
    int cnt = 0;
    const int off = (int)vh_off.size() - 1;
    for (auto& kv : loc_of)                                 // std::map: ascending gid on both sides
      if (rmask[kv.first] & (1u << p)) {
        slot[{p, kv.first}] = (int)vh_off.size() - 1;
        vh_idx.insert(vh_idx.end(), kv.second.begin(), kv.second.end());
        vh_off.push_back((int)vh_idx.size());
        ++cnt;
      }
    if (cnt) { c->peers.push_back(p); c->vh_poff.push_back(off); c->vh_pcnt.push_back(cnt); }
  }
  c->nvh = (int)vh_off.size() - 1;
  // gather tables: local copies (ascending) then the ghost slots of every sharing peer
  std::vector<int4> tab(nloc);
  std::vector<int> gs_off(nloc + 1, 0), gs_idx;
  {
    std::vector<int> loc_off, loc_idx, ent;
    nsk_setup::gs_csr(lgid.data(), nloc, loc_off, loc_idx);
    for (long long l = 0; l < nloc; ++l) {
      ent.assign(loc_idx.begin() + loc_off[l], loc_idx.begin() + loc_off[l + 1]);
      const long long g = lgid[l];
      if (rmask[g] & ~(1u << rank))
        for (int p = 0; p < nranks; ++p)
          if (p != rank && (rmask[g] & (1u << p))) ent.push_back((int)nloc + slot[{p, g}]);
      const auto v = nsk_setup::gs_row(ent.data(), ent.size());
      tab[l] = make_int4(v[0], v[1], v[2], v[3]);
      gs_idx.insert(gs_idx.end(), ent.begin(), ent.end());
      gs_off[l + 1] = (int)gs_idx.size();
    }
  }
  Dev& d = c->d;
  d = P->d;                                                // shared: bases, Acif, vtab is rebuilt below
  d.stepctr = nullptr; d.step_iters = nullptr;             // (no per-step iteration record on shards: their budgets stay per step class)
  d.ecv = nullptr; d.ecslot = nullptr;                     // (the merged coarse-solve kernel and its vertex-major slots are single-rank)
  d.use_tot = 0;                                           // shards: totals come from the all-reduce path
  d.nel = nel; d.nblk = c->nblk; d.nloc = nloc; d.npr = npr; d.npr_glob = P->npr_glob ? P->npr_glob : P->npr;
  d.cs = nloc + c->nvh; d.nranks = nranks; d.rank = rank; d.dbg = nullptr;
  d.nproj_max = P->d.nproj_max;                            // the projection space of the pinned operator (Nek's residualProj), per shard
  d.PX = d.PEX = d.PD = d.PED = d.ppart = nullptr;
  d.spng_vr = nullptr; d.nl_spng_str = 0.0; d.bstep = nullptr; d.bf_stride = 0; d.forb = 0;

  // ---- Schwarz overlap halo of the pressure vector
  std::vector<int> p_idx((size_t)nel * PS, -1);
  std::vector<std::vector<long long>> need(nranks);        // global dofs needed from each peer
  auto gkey = [&](int gd) -> long long { return eglob ? eglob[gd / MM] * (long long)MM + gd % MM : (long long)gd; };
  for (int le = 0; le < nel; ++le)
    for (int k = 0; k < PS; ++k) {
      const int gd = P->h_pidx[(size_t)c->elems[le] * PS + k];
      if (gd >= 0 && g2l[gd / MM] < 0) need[part[gd / MM]].push_back(gkey(gd));
    }
  std::map<long long, int> gslot;
  int npg = 0;
  c->ph_goff.assign(nranks, 0); c->ph_gcnt.assign(nranks, 0);
  for (int p = 0; p < nranks; ++p) {
    std::sort(need[p].begin(), need[p].end());
    need[p].erase(std::unique(need[p].begin(), need[p].end()), need[p].end());
    c->ph_goff[p] = npg; c->ph_gcnt[p] = (int)need[p].size();
    for (long long gd : need[p]) gslot[gd] = npg++;
  }
  c->npg = npg;
  for (int le = 0; le < nel; ++le)
    for (int k = 0; k < PS; ++k) {
      const int gd = P->h_pidx[(size_t)c->elems[le] * PS + k];
      if (gd < 0) continue;
      const int ol = g2l[gd / MM];
      p_idx[(size_t)le * PS + k] = (ol >= 0) ? ol * MM + gd % MM : (int)npr + gslot[gkey(gd)];
    }
  // what every peer needs from me: scan the peer's patches (same rule, same order)
  std::vector<int> ph_sidx;
  c->ph_soff.assign(nranks, 0); c->ph_scnt.assign(nranks, 0);
  for (int p = 0; p < nranks; ++p) {
    if (p == rank) continue;
    std::vector<std::pair<long long, int>> want;          // (global key, local dof)
    for (int e = 0; e < P->nel; ++e) {
      if (part[e] != p) continue;
      for (int k = 0; k < PS; ++k) {
        const int gd = P->h_pidx[(size_t)e * PS + k];
        if (gd >= 0 && g2l[gd / MM] >= 0) want.push_back({gkey(gd), g2l[gd / MM] * MM + gd % MM});
      }
    }
    std::sort(want.begin(), want.end());
    want.erase(std::unique(want.begin(), want.end()), want.end());
    c->ph_soff[p] = (int)ph_sidx.size(); c->ph_scnt[p] = (int)want.size();
    for (auto& w : want) ph_sidx.push_back(w.second);
  }
  c->nps = (int)ph_sidx.size();
  d.ps = npr + npg;

  // ---- slices of the parent's element-major arrays
  const int* d_elems = nullptr;
  if ((rc = dupload(c, &d_elems, c->elems))) return rc;
  const Dev& pd = P->d;
#define SL(field, T, per) if ((rc = slice_elems<T>(c, P, pd.field, &d.field, d_elems, nel, per))) return rc
  auto slice_rows = [&](const double* src, size_t src_stride, int rows, int per, const double** dst) -> int {
    double* q = nullptr;                                   // [rows][nel*per] cut out of [rows][P->nel*per]
    int r2 = dalloc(c, &q, (size_t)rows * nel * per);
    if (r2) return r2;
    const long long n = (long long)nel * per;
    for (int k = 0; k < rows; ++k)
      hipLaunchKernelGGL(k_slice_elems<double>, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, P->stream, src + (size_t)k * src_stride, q + (size_t)k * n, d_elems, nel, per);
    *dst = q;
    return 0;
  };
  SL(g1, double, NN); SL(g2, double, NN); SL(g4, double, NN); SL(bm1, double, NN); SL(mask, double, NN);
  SL(minv, double, NN); SL(binv, double, NN); SL(spng, double, NN); SL(bm1s, double, NN);
  if (nd == 2) {
    SL(w2rx, double, MM); SL(w2ry, double, MM); SL(w2sx, double, MM); SL(w2sy, double, MM);
    SL(cUr, double, NDD); SL(cUs, double, NDD); SL(GUx, double, NDD); SL(GUy, double, NDD); SL(GVx, double, NDD); SL(GVy, double, NDD);
    SL(rxd, double, NDD); SL(ryd, double, NDD); SL(sxd, double, NDD); SL(syd, double, NDD);     // full-equation convection (nonlinear map)
    SL(p_inv, float, PS * MM); SL(evert, int, 4);
  } else {
    SL(g3, double, NN); SL(g5, double, NN); SL(g6, double, NN);
    SL(fdS, double, 3 * N * N); SL(fdL, double, 3 * N); SL(evert, int, 8);
    if ((rc = slice_rows(pd.w2m, (size_t)P->npr, 9, MM, &d.w2m)) || (rc = slice_rows(pd.bfc, (size_t)pd.nfine, 12, NDD, &d.bfc)) ||
        (rc = slice_rows(pd.mtd, (size_t)pd.nfine, 9, NDD, &d.mtd))) return rc;
    d.nfine = (long long)nel * NDD; d.cUr = d.bfc;
  }
#undef SL
  if ((rc = slice_rows(pd.dinv, (size_t)P->nloc, 3, NN, &d.dinv))) return rc;
  // GLL coordinates of the shard's own elements (k_sens_grad / k_budget_prod derive the inverse mapping from them): memory of
  // the shard, so the post-processing entries outlive nsk_shard_release_parent
  c->xyz = nullptr;
  if (P->xyz && (rc = slice_rows(P->xyz, (size_t)P->nloc, nd, NN, &c->xyz))) return rc;
  // coarse: this rank's element corners per *global* vertex
  if (nd == 2) {
    std::vector<int> vtab((size_t)P->nvert * CVT, -1), fill(P->nvert, 0);
    for (int le = 0; le < nel; ++le)
      for (int cc = 0; cc < 4; ++cc) {
        const int v = P->h_evert[(size_t)c->elems[le] * 4 + cc];
        if (fill[v] >= CVT) return fail(NSK_EINVAL, "vertex valence too large");
        vtab[(size_t)v * CVT + fill[v]++] = le * 4 + cc;
      }
    if ((rc = dupload(c, &d.vtab, vtab))) return rc;
  } else {
    std::vector<int> v_off(P->nvert + 1, 0), v_ent((size_t)nel * 8);
    for (int le = 0; le < nel; ++le) for (int cc = 0; cc < 8; ++cc) v_off[P->h_evert[(size_t)c->elems[le] * 8 + cc] + 1]++;
    for (int v = 0; v < P->nvert; ++v) v_off[v + 1] += v_off[v];
    std::vector<int> pos(v_off.begin(), v_off.end() - 1);
    for (int le = 0; le < nel; ++le) for (int cc = 0; cc < 8; ++cc) v_ent[pos[P->h_evert[(size_t)c->elems[le] * 8 + cc]]++] = le * 8 + cc;
    if ((rc = dupload(c, &d.v_off, v_off)) || (rc = dupload(c, &d.v_ent, v_ent))) return rc;
  }
  d.gs_corner = nullptr; d.dpw = nullptr;                  // (shards run the element-kernel forms of the once-per-step sums)
  if (c->ndim == 3 && (rc = dupload(c, &d.gs_corner, nsk_setup::corner_table(c->N, nel, gs_off, gs_idx)))) return rc;
  if ((rc = dupload(c, &d.gs_tab, tab)) || (rc = dupload(c, &d.gs_off, gs_off)) || (rc = dupload(c, &d.gs_idx, gs_idx)) ||
      (rc = dupload(c, &d.p_idx, p_idx)) || (rc = dupload(c, &c->vh_off, vh_off)) || (rc = dupload(c, &c->vh_idx, vh_idx)) ||
      (rc = dupload(c, &c->ph_sidx, ph_sidx))) return rc;
  // ---- rank-local state and work arrays
  const long long cs = d.cs;
  // (of the parent's mutable arrays a shard keeps, through `d = P->d` and the copies above: rch, Wr / hz, hy, cw_*, circ_*; they stay
  //  in the parent's record)
  if ((rc = alloc_core_state(c, nd, cs, d.ps, npr, nel, c->nblk, NCORN, d.nproj_max)) || (rc = alloc_totals(c)) ||
      (rc = dalloc_mut(c, &d.xc, P->nvert)) || (rc = dalloc_mut(c, &c->rc_part, c->coarse_lda)) ||
      (rc = dalloc(c, &c->vsend, (size_t)4 * std::max(c->nvh, 1))) || (rc = dalloc(c, &c->vrecv, (size_t)4 * std::max(c->nvh, 1))) ||
      (rc = dalloc(c, &c->psend, std::max(c->nps, 1))) || (rc = dalloc(c, &c->precv, std::max(c->npg, 1))) ||
      (rc = alloc_scratch(c, nd, cs, npr))) return rc;
  {
    std::vector<int2> seg(std::max(c->nvh, 1), make_int2(0, 0));      // halo slot -> {first slot, slot count} of its peer (packed messages)
    for (size_t pi = 0; pi < c->peers.size(); ++pi)
      for (int k = 0; k < c->vh_pcnt[pi]; ++k) seg[c->vh_poff[pi] + k] = make_int2(c->vh_poff[pi], c->vh_pcnt[pi]);
    if ((rc = dupload(c, &c->vh_seg, seg))) return rc;
  }
  c->mfma_convect = P->mfma_convect; c->helm_pf = P->helm_pf; c->helm_pf_grid = P->helm_pf_grid; c->debug = P->debug; c->gmres_cycle = P->gmres_cycle; c->gs2_from = P->gs2_from;
  HIPCHK(hipStreamSynchronize(P->stream));
  return 0;
}

// ---------------------------------------------------------------------------
// transports.  G = the ranks that live in this process (all of them for virtual ranks; one for RCCL)
// ---------------------------------------------------------------------------
static int find_peer(const nsk_ctx* c, int p) {
  for (size_t k = 0; k < c->peers.size(); ++k) if (c->peers[k] == p) return (int)k;
  return -1;
}


static int verify_allreduce(nsk_ctx* c, const double* res, int n, hipStream_t st);

// ---- host-staged transport (nsk_comm_init_host): device -> pinned host -> callback -> device
static int hs_reserve(nsk_ctx* c, size_t n) {
  if (n <= c->hs_cap) return 0;
  if (c->hs_send) (void)hipHostFree(c->hs_send);
  if (c->hs_recv) (void)hipHostFree(c->hs_recv);
  c->hs_send = c->hs_recv = nullptr; c->hs_cap = 0;
  HIPCHK(hipHostMalloc((void**)&c->hs_send, n * sizeof(double)));
  HIPCHK(hipHostMalloc((void**)&c->hs_recv, n * sizeof(double)));
  c->hs_cap = n;
  return 0;
}
static int hs_allreduce(nsk_ctx* c, double* dbuf, int n) {
  int rc = hs_reserve(c, (size_t)n);
  if (rc) return rc;
  HIPCHK(hipMemcpyAsync(c->hs_send, dbuf, n * sizeof(double), hipMemcpyDeviceToHost, c->stream));
  HIPCHK(hipStreamSynchronize(c->stream));
  if (c->host_allred(c->host_user, c->hs_send, n) != 0) return fail(NSK_EHIP, "host all-reduce callback failed");
  HIPCHK(hipMemcpyAsync(dbuf, c->hs_send, n * sizeof(double), hipMemcpyHostToDevice, c->stream));
  return 0;
}

// xs != nullptr: the whole exchange (pack, transport, unpack) runs on that stream instead of the ranks' own (halo / interior
// overlap: the caller orders it against the compute stream with events)
// ar / nar: an all-reduce (sum over ranks, in place) that rides in the same RCCL group as the halo messages (fused_allreduce_ok)
// xchg_vel_at: the field of rank G[r] is base[r] (ncomp <= 4 components of stride Dev::cs, ghost slots behind the nloc entries of
// each) -- any array of that shape, not only a member of Dev (the post-processing entries exchange their own work arrays)
static int xchg_vel_at(std::vector<nsk_ctx*>& G, double* const* base, int ncomp, hipStream_t xs = nullptr, double* ar = nullptr, int nar = 0) {
  auto S = [&](nsk_ctx* c) { return xs ? xs : c->stream; };
  // send / receive buffers: [peer][component][entry] (k_halo_pack), so every peer gets ONE contiguous message per exchange
  for (size_t r = 0; r < G.size(); ++r) {
    nsk_ctx* c = G[r];
    if (c->nvh) hipLaunchKernelGGL(k_halo_pack, dim3((c->nvh + 255) / 256), dim3(256), 0, S(c), (const double*)base[r], c->d.cs, ncomp, c->vh_off, c->vh_idx, c->vh_seg, c->nvh, c->vsend);
  }
  if (G.size() == 1 && G[0]->host_xchg) {                    // host-staged
    nsk_ctx* c = G[0];
    const size_t tot = (size_t)ncomp * c->nvh;
    int rc = hs_reserve(c, tot);
    if (rc) return rc;
    if (c->nvh) {
      HIPCHK(hipMemcpyAsync(c->hs_send, c->vsend, tot * sizeof(double), hipMemcpyDeviceToHost, S(c)));
      HIPCHK(hipStreamSynchronize(S(c)));
      const int np = (int)c->peers.size();
      std::vector<int> cnt(np); std::vector<const double*> sp(np); std::vector<double*> rp(np);
      for (int pi = 0; pi < np; ++pi) {
        cnt[pi] = ncomp * c->vh_pcnt[pi];
        sp[pi] = c->hs_send + (size_t)ncomp * c->vh_poff[pi]; rp[pi] = c->hs_recv + (size_t)ncomp * c->vh_poff[pi];
      }
      if (c->host_xchg(c->host_user, np, c->peers.data(), cnt.data(), sp.data(), rp.data()) != 0) return fail(NSK_EHIP, "host exchange callback failed");
      HIPCHK(hipMemcpyAsync(c->vrecv, c->hs_recv, tot * sizeof(double), hipMemcpyHostToDevice, S(c)));
    }
  } else
#ifdef NSK_WITH_RCCL
  if (G.size() == 1 && G[0]->comm) {
    nsk_ctx* c = G[0];
    RCCLCHK(ncclGroupStart());
    if (ar) RCCLCHK(ncclAllReduce(ar, ar, nar, ncclDouble, ncclSum, (ncclComm_t)c->comm, S(c)));
    for (size_t pi = 0; pi < c->peers.size(); ++pi) {
      const size_t o = (size_t)ncomp * c->vh_poff[pi], n = (size_t)ncomp * c->vh_pcnt[pi];
      RCCLCHK(ncclSend(c->vsend + o, n, ncclDouble, c->peers[pi], (ncclComm_t)c->comm, S(c)));
      RCCLCHK(ncclRecv(c->vrecv + o, n, ncclDouble, c->peers[pi], (ncclComm_t)c->comm, S(c)));
    }
    RCCLCHK(ncclGroupEnd());
    if (ar) { int rcv = verify_allreduce(c, ar, nar, S(c)); if (rcv) return rcv; }      // (the all-reduce that rode in the group: the form no hardware had run before this round)
  } else
#endif
  {
    for (nsk_ctx* c : G)
      for (size_t pi = 0; pi < c->peers.size(); ++pi) {
        nsk_ctx* o = nullptr;
        for (nsk_ctx* x : G) if (x->rank == c->peers[pi]) o = x;
        if (!o) return fail(NSK_EINVAL, "peer rank not in this process and no RCCL communicator");
        const int qi = find_peer(o, c->rank);
        if (qi < 0 || o->vh_pcnt[qi] != c->vh_pcnt[pi]) return fail(NSK_EINVAL, "halo tables of two ranks disagree");
        HIPCHK(hipMemcpyAsync(o->vrecv + (size_t)ncomp * o->vh_poff[qi], c->vsend + (size_t)ncomp * c->vh_poff[pi],
                              (size_t)ncomp * c->vh_pcnt[pi] * sizeof(double), hipMemcpyDeviceToDevice, S(c)));
      }
  }
  for (size_t r = 0; r < G.size(); ++r) {
    nsk_ctx* c = G[r];
    if (c->nvh) hipLaunchKernelGGL(k_halo_unpack, dim3((c->nvh + 255) / 256), dim3(256), 0, S(c), base[r], c->d.cs, c->d.nloc, ncomp, c->vh_seg, c->nvh, (const double*)c->vrecv);
  }
  return 0;
}
static int xchg_vel(std::vector<nsk_ctx*>& G, double* nsk::Dev::*field, long long extra, int ncomp, hipStream_t xs = nullptr, double* ar = nullptr, int nar = 0) {
  double* base[16];                                          // (nranks <= 16: shard_create)
  if (G.size() > 16) return fail(NSK_EINVAL, "more than 16 ranks in one process");
  for (size_t r = 0; r < G.size(); ++r) base[r] = G[r]->d.*field + extra * G[r]->d.cs;
  return xchg_vel_at(G, base, ncomp, xs, ar, nar);
}

static int xchg_pres(std::vector<nsk_ctx*>& G, int j, hipStream_t xs = nullptr, double* ar = nullptr, int nar = 0) {      // ghost part of the GMRES basis vector V[j]; xs, ar: as xchg_vel
  auto S = [&](nsk_ctx* c) { return xs ? xs : c->stream; };
  for (nsk_ctx* c : G)
    if (c->nps) hipLaunchKernelGGL(k_phalo_pack, dim3((c->nps + 255) / 256), dim3(256), 0, S(c), (const double*)(c->d.V + (size_t)j * c->d.ps), c->ph_sidx, c->nps, c->psend);
  if (G.size() == 1 && G[0]->host_xchg) {
    nsk_ctx* c = G[0];
    int rc = hs_reserve(c, (size_t)std::max(c->nps, c->npg) + 1);
    if (rc) return rc;
    if (c->nps) HIPCHK(hipMemcpyAsync(c->hs_send, c->psend, c->nps * sizeof(double), hipMemcpyDeviceToHost, S(c)));
    HIPCHK(hipStreamSynchronize(S(c)));
    // send and receive counts differ per peer here: two one-directional exchanges through the same callback are avoided by
    // padding both directions of a peer to the larger count
    std::vector<int> peers, cnt; std::vector<const double*> sp; std::vector<double*> rp;
    std::vector<std::vector<double>> sb, rb;
    for (int p = 0; p < c->nranks; ++p) {
      if (p == c->rank || (!c->ph_scnt[p] && !c->ph_gcnt[p])) continue;
      const int n = std::max(c->ph_scnt[p], c->ph_gcnt[p]);
      peers.push_back(p); cnt.push_back(n);
      sb.emplace_back(n, 0.0); rb.emplace_back(n, 0.0);
      std::memcpy(sb.back().data(), c->hs_send + c->ph_soff[p], c->ph_scnt[p] * sizeof(double));
    }
    for (size_t k = 0; k < peers.size(); ++k) { sp.push_back(sb[k].data()); rp.push_back(rb[k].data()); }
    if (!peers.empty() && c->host_xchg(c->host_user, (int)peers.size(), peers.data(), cnt.data(), sp.data(), rp.data()) != 0)
      return fail(NSK_EHIP, "host exchange callback failed");
    for (size_t k = 0; k < peers.size(); ++k)
      std::memcpy(c->hs_recv + c->ph_goff[peers[k]], rb[k].data(), c->ph_gcnt[peers[k]] * sizeof(double));
    if (c->npg) HIPCHK(hipMemcpyAsync(c->d.V + (size_t)j * c->d.ps + c->d.npr, c->hs_recv, c->npg * sizeof(double), hipMemcpyHostToDevice, S(c)));
    return 0;
  }
#ifdef NSK_WITH_RCCL
  if (G.size() == 1 && G[0]->comm) {
    nsk_ctx* c = G[0];
    RCCLCHK(ncclGroupStart());
    if (ar) RCCLCHK(ncclAllReduce(ar, ar, nar, ncclDouble, ncclSum, (ncclComm_t)c->comm, S(c)));
    for (int p = 0; p < c->nranks; ++p) {
      if (p == c->rank) continue;
      if (c->ph_scnt[p]) RCCLCHK(ncclSend(c->psend + c->ph_soff[p], c->ph_scnt[p], ncclDouble, p, (ncclComm_t)c->comm, S(c)));
      if (c->ph_gcnt[p]) RCCLCHK(ncclRecv(c->d.V + (size_t)j * c->d.ps + c->d.npr + c->ph_goff[p], c->ph_gcnt[p], ncclDouble, p, (ncclComm_t)c->comm, S(c)));
    }
    RCCLCHK(ncclGroupEnd());
    return ar ? verify_allreduce(c, ar, nar, S(c)) : 0;
  }
#endif
  for (nsk_ctx* c : G)
    for (nsk_ctx* o : G) {
      if (o == c || !c->ph_scnt[o->rank]) continue;
      if (o->ph_gcnt[c->rank] != c->ph_scnt[o->rank]) return fail(NSK_EINVAL, "pressure halo tables of two ranks disagree");
      HIPCHK(hipMemcpyAsync(o->d.V + (size_t)j * o->d.ps + o->d.npr + o->ph_goff[c->rank], c->psend + c->ph_soff[o->rank],
                            c->ph_scnt[o->rank] * sizeof(double), hipMemcpyDeviceToDevice, S(c)));
    }
  return 0;
}

// The first `arv_left` all-reduces of a context with a real transport are VERIFIED: do all ranks hold the same bits?  (k_ar_chunks:
// exact integer sums, so every rank reaches the same verdict; a mismatch is counted in Stats::allred_mismatch and the map returns
// NSK_ECOMM.)  Not inside a stream capture (the first maps of a sharded run are eager); `res` = the all-reduced values on the device.
static int verify_allreduce(nsk_ctx* c, const double* res, int n, hipStream_t st) {
  if (c->arv_left <= 0 || n <= 0 || !(c->comm || c->host_allred) || stream_capturing(st)) return 0;
  c->arv_left--;
  if (!c->arv_buf) { int rc = dalloc(c, &c->arv_buf, 64); if (rc) return rc; }
  const int nn = std::min(n, 8);
  hipLaunchKernelGGL(k_ar_chunks, dim3(1), dim3(64), 0, st, res, nn, c->arv_buf);
  if (c->host_allred) {
    if (st != c->stream) HIPCHK(hipStreamSynchronize(st));
    int rc = hs_allreduce(c, c->arv_buf, 8 * nn);
    if (rc) return rc;
    hipLaunchKernelGGL(k_ar_check, dim3(1), dim3(64), 0, c->stream, (const double*)c->arv_buf, nn, c->d.nranks, c->d.stats);
    return 0;
  }
#ifdef NSK_WITH_RCCL
  RCCLCHK(ncclAllReduce(c->arv_buf, c->arv_buf, 8 * nn, ncclDouble, ncclSum, (ncclComm_t)c->comm, st));
#endif
  hipLaunchKernelGGL(k_ar_check, dim3(1), dim3(64), 0, st, (const double*)c->arv_buf, nn, c->d.nranks, c->d.stats);
  return 0;
}

static int allreduce(std::vector<nsk_ctx*>& G, double* nsk::Dev::*buf, long long off, int n) {
  if (G.size() == 1 && G[0]->host_allred) { int rc = hs_allreduce(G[0], G[0]->d.*buf + off, n); return rc ? rc : verify_allreduce(G[0], G[0]->d.*buf + off, n, G[0]->stream); }
#ifdef NSK_WITH_RCCL
  if (G.size() == 1 && G[0]->comm) {
    nsk_ctx* c = G[0];
    RCCLCHK(ncclAllReduce(c->d.*buf + off, c->d.*buf + off, n, ncclDouble, ncclSum, (ncclComm_t)c->comm, c->stream));
    return verify_allreduce(c, c->d.*buf + off, n, c->stream);
  }
#endif
  PtrPack pp;
  for (size_t r = 0; r < G.size(); ++r) pp.p[r] = G[r]->d.*buf + off;
  hipLaunchKernelGGL(k_loop_allreduce_pack, dim3((n + 255) / 256), dim3(256), 0, G[0]->stream, pp, (int)G.size(), n);
  return 0;
}
static int allreduce_ptr(std::vector<nsk_ctx*>& G, double* nsk_ctx::*buf, int n) {
  if (G.size() == 1 && G[0]->host_allred) { int rc = hs_allreduce(G[0], G[0]->*buf, n); return rc ? rc : verify_allreduce(G[0], G[0]->*buf, n, G[0]->stream); }
#ifdef NSK_WITH_RCCL
  if (G.size() == 1 && G[0]->comm) {
    nsk_ctx* c = G[0];
    RCCLCHK(ncclAllReduce(c->*buf, c->*buf, n, ncclDouble, ncclSum, (ncclComm_t)c->comm, c->stream));
    return verify_allreduce(c, c->*buf, n, c->stream);
  }
#endif
  PtrPack pp;
  for (size_t r = 0; r < G.size(); ++r) pp.p[r] = G[r]->*buf;
  hipLaunchKernelGGL(k_loop_allreduce_pack, dim3((n + 255) / 256), dim3(256), 0, G[0]->stream, pp, (int)G.size(), n);
  return 0;
}

// ---------------------------------------------------------------------------
// one time step, all ranks of this process in lock-step (eager launches)
// ---------------------------------------------------------------------------
#define FORALL for (nsk_ctx* c : G)
static bool group_hostcheck(const std::vector<nsk_ctx*>& G) {
  const nsk_ctx* c = G[0];
  if (c->shard_hostcheck >= 0) return c->shard_hostcheck != 0;
  return c->comm || c->host_xchg || c->host_allred;
}
// the convergence flags of rank G[0] (all ranks hold the same: they follow from all-reduced sums): velocity solve after launch
// `it` (which = 0), pressure solve (which = 1).  One small device-to-host copy and a stream synchronisation.
static int group_flags_done(std::vector<nsk_ctx*>& G, int which, int it, bool* done) {
  int rc = flags_done(G[0], which, it, done);
  if (rc) return rc;
  for (size_t r = 1; r < G.size(); ++r) HIPCHK(hipStreamSynchronize(G[r]->stream));      // (virtual ranks share the stream: no-ops)
  return 0;
}

// hexahedra at lx1 = 10: the E-apply kernels in the forms the single-rank context runs (k_schwarz_q: four wavefronts per element;
// k_divgs_c3: the components' pass chains side by side) -- same arguments, element offset and grid as k_schwarz / k_divgs
#define SH_SCHWARZ(grid, dev, ...) do { bool q_ = false; \
    if constexpr (N == 10) { if (nd == 3) { hipLaunchKernelGGL(nsk::k3::k_schwarz_q<10>, dim3(grid), dim3(256), 0, c->stream, dev, __VA_ARGS__); q_ = true; } } \
    if (!q_) hipLaunchKernelGGL(k_schwarz<N>, dim3(grid), dim3(NT), 0, c->stream, dev, __VA_ARGS__); } while (0)
// ... and the CG iteration as resident workgroups with LDS-DMA prefetch (k_helm_p<10>; it >= 1): `cnt` elements from dev.boff on
#define SH_HELM(cnt, dev) do { bool q_ = false; \
    if constexpr (N == 10) { if (nd == 3 && it >= 1 && c->helm_pf != 0 && (cnt) > 0) { \
      hipLaunchKernelGGL(nsk::k3::k_helm_p<10>, dim3(std::min((int)(cnt), helm_pf_grid(c))), dim3(nsk::k3::Cfg<10>::NT), 0, c->stream, dev, sc, it, (int)(cnt)); q_ = true; } } \
    if (!q_) hipLaunchKernelGGL(k_helm<N>, dim3(cnt), dim3(NT), 0, c->stream, dev, sc, it, (const double*)c->d.rloc); } while (0)
#define SH_DIVGS(grid, dev, ...) do { bool q_ = false; \
    if constexpr (N == 10) { if (nd == 3) { hipLaunchKernelGGL(nsk::k3::k_divgs_c3<10>, dim3(grid), dim3(nsk::k3::Cfg<10>::NT), 0, c->stream, dev, __VA_ARGS__); q_ = true; } } \
    if (!q_) hipLaunchKernelGGL(k_divgs<N>, dim3(grid), dim3(NT), 0, c->stream, dev, __VA_ARGS__); } while (0)
static int group_step(std::vector<nsk_ctx*>& G, int istep, int adjoint) {
  nsk_ctx* c0 = G[0];
  const StepCoef sc = make_coef(c0, istep, adjoint);
  const bool hc = group_hostcheck(G) && !stream_capturing(c0->stream);
  // host-checked: iterate until the device flags say converged (up to the caps); otherwise the launch budgets of the step class
  int nh = hc ? c0->lb.max_helm : c0->lb.cur_helm[sc.cls];
  const int np = hc ? c0->lb.max_pres : c0->lb.cur_pres[sc.cls];                              // beyond gmres_cycle iterations: restarted cycles
  const double scale = 1.0 / (sc.h2 * std::sqrt(c0->d.vol));
  const int nd = c0->ndim, hrows = c0->hrows, hstride = c0->hstride;
  const bool proj = c0->d.nproj_max > 0, singular = !c0->d.has_outflow;
  int rc;
  // rank totals of `rows` rows of per-workgroup partials, then the sum over ranks
  auto totals = [&](double* nsk::Dev::*part, long long part_off_rows, int rows, double* nsk::Dev::*tot, long long tot_off) -> int {
    FORALL hipLaunchKernelGGL(k_tot2, dim3(rows), dim3(256), 0, c->stream, (const double*)(c->d.*part + (size_t)part_off_rows * c->nblk), c->nblk, c->d.*tot + tot_off, (const int*)nullptr);
    return allreduce(G, tot, tot_off, rows);
  };
  // one RCCL rank per process: the all-reduce of an iteration rides in the group of that iteration's halo messages
  const bool fuse = G.size() == 1 && c0->comm && !c0->host_xchg && !c0->host_allred && c0->rccl_fuse;
  DISPATCH_N(c0->key, {
    constexpr int NT = Cfg<N>::NT;
    FORALL {
      if (c->d.forb && adjoint != 2)  // Fourier orbit: the base flow of this step into the rank's steady slot (hexahedra: cUr is the 12-constant array)
        hipLaunchKernelGGL(k_baseflow_fourier<N>, dim3(c->nel), dim3(Cfg<N>::NTD), 0, c->stream, c->d, (double*)c->d.cUr, (double*)c->d.cUs,
                           (double*)c->d.GUx, (double*)c->d.GUy, (double*)c->d.GVx, (double*)c->d.GVy);
      launch_convect<N>(c, c->d, adjoint);
      if (c->force)                     // forced map (nsk_group_forced_map; eager steps only): + B f of the rank's own elements, as step()
        hipLaunchKernelGGL(nsk::sens::k_add_force, dim3((unsigned)((c->d.nloc + 255) / 256)), dim3(256), 0, c->stream, c->d.bf, c->d.cs, c->d.bm1, c->force, c->d.nloc, c->ndim);
      if (c->sfd.on) sfd_call(c, istep - 1);      // SFD map (nsk_group_sfd_map; eager steps only): the rank's own elements, as step()
      hipLaunchKernelGGL(k_rhs<N>, dim3(c->nblk), dim3(NT), 0, c->stream, c->d, sc);
    }
    if ((rc = xchg_vel(G, &Dev::rloc, 0, nd)) || (rc = xchg_vel(G, &Dev::bloc, 0, nd))) return rc;
    // halo / interior overlap (eager launches): the boundary workgroups first, their halo on the exchange stream
    // while the interior workgroups run; the all-reduce of the dot products waits for both
    bool ov = c0->halo_overlap && !stream_capturing(c0->stream);
    if (ov) {
      for (nsk_ctx* c : G) ov = ov && c->nbb > 0 && c->nbb < c->nblk && c->stream == c0->stream;
      if (ov && !c0->comm_stream) {
        HIPCHK(hipStreamCreateWithFlags(&c0->comm_stream, hipStreamNonBlocking));
        for (auto& e : c0->orth_ev) HIPCHK(hipEventCreateWithFlags(&e, hipEventDisableTiming));
      }
      if (ov && !c0->ov_ev[0]) for (auto& e : c0->ov_ev) HIPCHK(hipEventCreateWithFlags(&e, hipEventDisableTiming));
    }
    for (int it = 0; it < nh; ++it) {
      if (ov) {
        if constexpr (N == 6 || N == 8 || N == 10 || N == 12) {
          FORALL { Dev de = c->d; de.boff = 0; SH_HELM(c->nbb, de); }
          HIPCHK(hipEventRecord(c0->ov_ev[0], c0->stream));
          HIPCHK(hipStreamWaitEvent(c0->comm_stream, c0->ov_ev[0], 0));
          FORALL { Dev de = c->d; de.boff = c->nbb; SH_HELM(c->nblk - c->nbb, de); }
          if ((rc = xchg_vel(G, &Dev::hwl, (long long)(it & 1) * nd, nd, c0->comm_stream))) return rc;
          HIPCHK(hipEventRecord(c0->ov_ev[1], c0->comm_stream));
          HIPCHK(hipStreamWaitEvent(c0->stream, c0->ov_ev[1], 0));
          if ((rc = totals(&Dev::hpart, (long long)(it & 1) * hrows, hrows, &Dev::htot, (it & 1) * hstride))) return rc;
        }
      } else {
      FORALL SH_HELM(c->nblk, c->d);
      if (fuse) {
        hipLaunchKernelGGL(k_tot2, dim3(hrows), dim3(256), 0, c0->stream, (const double*)(c0->d.hpart + (size_t)(it & 1) * hrows * c0->nblk), c0->nblk, c0->d.htot + (it & 1) * hstride, (const int*)nullptr);
        if ((rc = xchg_vel(G, &Dev::hwl, (long long)(it & 1) * nd, nd, nullptr, c0->d.htot + (it & 1) * hstride, hrows))) return rc;
      } else if ((rc = totals(&Dev::hpart, (long long)(it & 1) * hrows, hrows, &Dev::htot, (it & 1) * hstride)) ||
          (rc = xchg_vel(G, &Dev::hwl, (long long)(it & 1) * nd, nd))) return rc;
      }
      // launch `it` has written the flags that follow from launch it - 1's residual: first look where the previous solve of this
      // class ended, then after every second launch
      if (hc && it >= 1 && it >= c0->hc_helm[sc.cls] && ((it - c0->hc_helm[sc.cls]) % 2 == 0)) {
        bool done = false;
        if ((rc = group_flags_done(G, 0, it, &done))) return rc;
        if (done) { for (nsk_ctx* c : G) c->hc_helm[sc.cls] = std::max(1, it - 1); nh = it + 1; break; }
      }
    }
    FORALL hipLaunchKernelGGL(k_pres_rhs<N>, dim3(c->nblk), dim3(NT), 0, c->stream, c->d, sc, (nh - 1) & 1, nh - 1);
    // |g|^2 (+ sum(g) with the pressure null space), then the projection dots (x_i, g): sums over ranks
    if ((rc = totals(&Dev::gpart, 0, singular ? 2 : 1, &Dev::gtot, 0))) return rc;
    if (proj && (rc = totals(&Dev::ppart, 0, MAXPROJ + 1, &Dev::ptot, 0))) return rc;
    if (singular) {                                        // [UPSTREAM navier1.f ortho]: mean over ALL ranks' Gauss nodes (Dev::npr_glob)
      FORALL hipLaunchKernelGGL(k_ortho, dim3(c->nblk), dim3(256), 0, c->stream, c->d);
      if ((rc = totals(&Dev::gpart, 0, 1, &Dev::gtot, 0))) return rc;
    }
    if (proj) {
      FORALL hipLaunchKernelGGL(k_proj_apply, dim3(c->nblk), dim3(256), 0, c->stream, c->d);
      if ((rc = totals(&Dev::gpart, 0, 1, &Dev::gtot, 0))) return rc;
    }
    const double emul = istep <= 3 ? c0->early_pres_mul : 1.0;      // same early-step tolerance as the single-rank driver
    FORALL { Dev de = c->d; de.tol_pres = early_tol(de, emul); hipLaunchKernelGGL(k_gmres_update<N>, dim3(c->nblk), dim3(NT), 0, c->stream, de, -1, scale, c->lb.min_pres, sc.cls); }
    bool pres_done0 = false;
    if (hc && c0->hc_pres[sc.cls] <= 1) {                   // the last solve of this class needed (almost) nothing: the projection may have solved this one
      if ((rc = group_flags_done(G, 1, 0, &pres_done0))) return rc;
      if (pres_done0) for (nsk_ctx* c : G) c->hc_pres[sc.cls] = 0;
    }
    for (int jt = 0; jt < np && !pres_done0; ++jt) {
      const int j = jt % c0->gmres_cycle;                  // index inside the current GMRES cycle
      if (jt > 0 && j == 0) {                              // cycle full and not converged: restart on the residual (as pres_solve_launch)
        FORALL hipLaunchKernelGGL(k_gmres_restart, dim3(c->nblk), dim3(256), 0, c->stream, c->d, c->gmres_cycle);
        if ((rc = totals(&Dev::gpart, 0, 1, &Dev::gtot, 0))) return rc;
        FORALL { Dev de = c->d; de.tol_pres = early_tol(de, emul); hipLaunchKernelGGL(k_gmres_update<N>, dim3(c->nblk), dim3(NT), 0, c->stream, de, -2, scale, c->lb.min_pres, sc.cls); }
      }
      if (ov) {
        // halo / interior overlap of the pressure iteration: the coarse restriction and its all-reduce first (the exchange stream
        // carries point-to-point traffic only BETWEEN collectives), then the ghost part of V[j] travels while the coarse solve and
        // the Schwarz solves of the interior elements run (an interior element shares no node with another rank, so neither its
        // patch nor its dssum reaches a ghost); the boundary elements follow; the same for D^T z and the E apply.
        FORALL {
          if (nd == 3) hipLaunchKernelGGL(k_coarse_restrict_csr, dim3(c->coarse_lda / 256), dim3(256), 0, c->stream, c->d, c->rc_part);
          else hipLaunchKernelGGL(k_coarse_restrict, dim3(c->coarse_lda / 256), dim3(256), 0, c->stream, c->d, c->rc_part);
        }
        if ((rc = allreduce_ptr(G, &nsk_ctx::rc_part, c0->coarse_lda))) return rc;
        HIPCHK(hipEventRecord(c0->ov_ev[0], c0->stream));
        HIPCHK(hipStreamWaitEvent(c0->comm_stream, c0->ov_ev[0], 0));
        FORALL {                                             // (queued before the exchange is started: a host-staged transport blocks the host)
          if (c->coarse_iter) { if ((rc = coarse_iterative(c, c->rc_part))) return rc; }
          else hipLaunchKernelGGL(k_coarse_big, dim3((c->d.nvert + 3) / 4), dim3(256), 0, c->stream, c->d, (const double*)c->rc_part);
          Dev de = c->d; de.boff = c->nbb;
          SH_SCHWARZ(c->nblk - c->nbb, de, (const double*)(c->d.V + (size_t)j * c->d.ps), c->d.Z + (size_t)j * c->d.npr, 1, 1);
        }
        if ((rc = xchg_pres(G, j, c0->comm_stream))) return rc;
        HIPCHK(hipEventRecord(c0->ov_ev[1], c0->comm_stream));
        HIPCHK(hipStreamWaitEvent(c0->stream, c0->ov_ev[1], 0));
        FORALL SH_SCHWARZ(c->nbb, c->d, (const double*)(c->d.V + (size_t)j * c->d.ps), c->d.Z + (size_t)j * c->d.npr, 1, 1);
        HIPCHK(hipEventRecord(c0->ov_ev[0], c0->stream));
        HIPCHK(hipStreamWaitEvent(c0->comm_stream, c0->ov_ev[0], 0));
        FORALL { Dev de = c->d; de.boff = c->nbb; SH_DIVGS(c->nblk - c->nbb, de, (const double*)c->d.yl, c->d.V + (size_t)(j + 1) * c->d.ps, j, 1); }
        if ((rc = xchg_vel(G, &Dev::yl, 0, nd, c0->comm_stream))) return rc;
        HIPCHK(hipEventRecord(c0->ov_ev[1], c0->comm_stream));
        HIPCHK(hipStreamWaitEvent(c0->stream, c0->ov_ev[1], 0));
        FORALL SH_DIVGS(c->nbb, c->d, (const double*)c->d.yl, c->d.V + (size_t)(j + 1) * c->d.ps, j, 1);
      } else if (fuse) {                                     // the coarse restriction's all-reduce rides with the ghost part of V[j]
        if (nd == 3) hipLaunchKernelGGL(k_coarse_restrict_csr, dim3(c0->coarse_lda / 256), dim3(256), 0, c0->stream, c0->d, c0->rc_part);
        else hipLaunchKernelGGL(k_coarse_restrict, dim3(c0->coarse_lda / 256), dim3(256), 0, c0->stream, c0->d, c0->rc_part);
        if ((rc = xchg_pres(G, j, nullptr, c0->rc_part, c0->coarse_lda))) return rc;
      } else {
      if ((rc = xchg_pres(G, j))) return rc;
      FORALL {
        if (nd == 3) hipLaunchKernelGGL(k_coarse_restrict_csr, dim3(c->coarse_lda / 256), dim3(256), 0, c->stream, c->d, c->rc_part);
        else hipLaunchKernelGGL(k_coarse_restrict, dim3(c->coarse_lda / 256), dim3(256), 0, c->stream, c->d, c->rc_part);
      }
      if ((rc = allreduce_ptr(G, &nsk_ctx::rc_part, c0->coarse_lda))) return rc;
      }
      if (!ov) {
      FORALL {
        if (c->coarse_iter) { if ((rc = coarse_iterative(c, c->rc_part))) return rc; }
        else hipLaunchKernelGGL(k_coarse_big, dim3((c->d.nvert + 3) / 4), dim3(256), 0, c->stream, c->d, (const double*)c->rc_part);
        SH_SCHWARZ(c->nblk, c->d, (const double*)(c->d.V + (size_t)j * c->d.ps), c->d.Z + (size_t)j * c->d.npr, 1, 1);
      }
      if ((rc = xchg_vel(G, &Dev::yl, 0, nd))) return rc;
      FORALL SH_DIVGS(c->nblk, c->d, (const double*)c->d.yl, c->d.V + (size_t)(j + 1) * c->d.ps, j, 1);
      }
      if ((rc = totals(&Dev::gpart, 0, j + 2, &Dev::gtot, 0))) return rc;
      const bool two = nd == 3 || j >= c0->gs2_from;        // second Gram-Schmidt pass (hexahedra: always; quadrilaterals: long solves)
      if (two) {
        FORALL hipLaunchKernelGGL(k_gmres_reorth<N>, dim3(c->nblk), dim3(NT), 0, c->stream, c->d, j);
        if ((rc = totals(&Dev::gpart2, 0, j + 2, &Dev::gtot2, 0))) return rc;
      }
      FORALL { Dev de = c->d; de.tol_pres = early_tol(de, emul); de.gs2 = two ? 1 : 0; hipLaunchKernelGGL(k_gmres_update<N>, dim3(c->nblk), dim3(NT), 0, c->stream, de, j, scale, c->lb.min_pres, sc.cls); }
      if (hc && jt + 1 < np && jt + 4 >= c0->hc_pres[sc.cls]) {          // (iteration counts of consecutive steps differ more than the velocity solve's: every iteration from three before the last count)
        bool done = false;
        if ((rc = group_flags_done(G, 1, 0, &done))) return rc;
        if (done) { for (nsk_ctx* c : G) c->hc_pres[sc.cls] = jt + 1; break; }
      }
    }
    FORALL hipLaunchKernelGGL(k_pres_update<N>, dim3(c->nblk), dim3(NT), 0, c->stream, c->d, sc);
    if ((rc = xchg_vel(G, &Dev::yl, 0, nd))) return rc;
    if (proj) {                                            // velocity correction + E dp and its dots for the projection space
      FORALL hipLaunchKernelGGL(k_vel_update_proj<N>, dim3(c->nblk), dim3(NT), 0, c->stream, c->d, sc);
      if ((rc = totals(&Dev::ppart, 0, MAXPROJ + 1, &Dev::ptot, 0))) return rc;
      FORALL hipLaunchKernelGGL(k_proj_update, dim3(c->nblk), dim3(256), 0, c->stream, c->d);
    } else {
      FORALL hipLaunchKernelGGL(k_vel_update, dim3((unsigned)((c->d.nloc + 255) / 256)), dim3(256), 0, c->stream, c->d, sc);
    }
  });
  return 0;
}

// The sharded step makes no host decision (budgets are launch counts, every solve ends on its device flag), so it captures
// like the single-rank one: ONE graph per step class holds the kernels of every rank of this process, the halo copies between
// them and -- with a communicator -- the RCCL send / recv / all-reduce calls (capturable; opt-in through `shard_graph`, because
// that combination has not run on hardware yet).  The host-staged transport synchronises the stream and stays eager.
static bool group_graph_ok(const std::vector<nsk_ctx*>& G) {
  const nsk_ctx* c = G[0];
  if (!c->use_graph || c->host_xchg || c->host_allred) return false;
  if (c->shard_hostcheck == 1) return false;                // host-checked convergence needs the host between iterations
  return c->comm ? c->shard_graph == 1 : c->shard_graph != 0;
}
static int group_ensure_graph(std::vector<nsk_ctx*>& G, int cls, int adjoint) {
  nsk_ctx* c = G[0];
  nsk_ctx::StepGraph& g = c->graphs[adjoint][cls];
  if (g.exec && g.nh == c->lb.cur_helm[cls] && g.np == c->lb.cur_pres[cls] && c->graph_members == G) return 0;
  if (c->graph_members != G) {                              // another set of ranks: every class is stale
    for (auto& a : c->graphs) for (auto& x : a) if (x.exec) { (void)hipGraphExecDestroy(x.exec); x.exec = nullptr; x.nh = -1; }
    c->graph_members = G;
  }
  int rc = capture_exec(c, [&] { return group_step(G, CLS_ISTEP[cls], adjoint); }, &g.exec, " (sharded step)");
  if (rc) return rc;
  g.nh = c->lb.cur_helm[cls]; g.np = c->lb.cur_pres[cls];
  return 0;
}

static int group_run_map(std::vector<nsk_ctx*>& G, int adjoint, double* const* f, const double* const* q) {
  const bool graph = group_graph_ok(G);
  if (graph)
    for (nsk_ctx* c : G) if (c->stream != G[0]->stream) return fail(NSK_EINVAL, "ranks of one process must share a stream");
  // Fourier orbit: every rank owns its table of cos / sin factors (its own orbit_phase); before any capture, and a rebuilt
  // table (address, row count) makes the group's graphs stale -- the members' kernels live in the graphs G[0] holds
  if (adjoint != 2)
    for (nsk_ctx* c : G)
      if (c->d.forb) {
        bool rebuilt = false;
        int rc = forb_trig_ensure(c, &rebuilt);
        if (rc) return rc;
        if (rebuilt) invalidate_graphs(G[0]);
      }
  for (;;) {
    if (graph)
      for (int k = 0; k < NCLS; ++k) { int rc = group_ensure_graph(G, k, adjoint); if (rc) return rc; }
    for (size_t r = 0; r < G.size(); ++r) { int rc = map_begin(G[r], q[r], adjoint); if (rc) return rc; }
    { int rc = bcv_open(G); if (rc) return rc; }             // BoostConv map (nsk_group_boostconv_map), as run_map
    for (int istep = 1; istep <= G[0]->nsteps; ++istep) {
      if (graph) { HIPCHK(hipGraphLaunch(G[0]->graphs[adjoint][step_class(istep)].exec, G[0]->stream)); continue; }
      int rc = group_step(G, istep, adjoint);
      if (rc) return rc;
      if (G[0]->debug) {
        for (nsk_ctx* c : G) {
          GmresScal Gs; double hs[32]; Stats s2;
          HIPCHK(hipStreamSynchronize(c->stream));
          HIPCHK(hipMemcpy(&Gs, c->d.gsc, sizeof(Gs), hipMemcpyDeviceToHost));
          HIPCHK(hipMemcpy(hs, c->d.hscal, sizeof(hs), hipMemcpyDeviceToHost));
          HIPCHK(hipMemcpy(&s2, c->d.stats, sizeof(s2), hipMemcpyDeviceToHost));
          fprintf(stderr, "rank %d step %3d: helm_it=%lld pres_it=%lld |g|=%.3e |g'|=%.3e nit=%d resid=%.3e nproj=%d helm ref %.3e %.3e done %g %g res %.3e %.3e\n", c->rank, istep,
                  s2.helm_iters, s2.pres_iters, Gs.gnorm0, Gs.beta0, Gs.nit, Gs.resid, Gs.nproj, hs[16], hs[17], hs[2], hs[6], hs[3], hs[7]);
        }
      }
      if (G[0]->bcv.on && (G[0]->bcv.step0 + istep) % G[0]->bcv.skip == 0) { int rc2 = bcv_call(G, nullptr, true); if (rc2) return rc2; }
    }
    for (nsk_ctx* c : G) if (c->sfd.on) sfd_call(c, c->nsteps);
    Stats h;
    HIPCHK(hipMemcpyAsync(&h, G[0]->d.stats, sizeof(Stats), hipMemcpyDeviceToHost, G[0]->stream));
    HIPCHK(hipStreamSynchronize(G[0]->stream));
    // The verdict (LaunchBudgets::verdict): the counters come from all-reduced sums, and the ranks of a group hold the same budgets:
    // every rank reaches the same one (and grows its own budgets for a redo); host-checked steps iterate to the caps whatever
    // the budgets say.  The error paths that reset the solver state or fail without booking leave hstats as it was.
    const bool hcm = !graph && group_hostcheck(G);
    Verdict v = Verdict::STANDS;
    for (size_t r = G.size(); r-- > 0;) v = G[r]->lb.verdict(map_facts(G[r], h, false, hcm));      // (G[0]'s is the one that counts)
    if (v == Verdict::FAIL_COMM || v == Verdict::FAIL_NAN) for (nsk_ctx* c : G) (void)reset_solver_state(c);
    if (v == Verdict::FAIL_COMM)
      return fail(NSK_ECOMM, "the ranks received different results from " + std::to_string((long long)h.allred_mismatch) + " of the verified all-reduces: the collective is not "
                  "rank-deterministic, device-side convergence flags would diverge (sharded map refused)");
    if (v == Verdict::FAIL_NAN)
      return fail(NSK_ENAN, "non-finite state inside the sharded map: " + std::to_string((long long)h.nonfinite) + " time steps with a NaN / Inf pressure right-hand side");
    if (v == Verdict::FAIL_SYNC || v == Verdict::TAILS_OFF_REDO)      // (shards run no persistent tails)
      return fail(NSK_EHIP, "grid barrier of the persistent velocity solve timed out (workgroups not co-resident?): set option fused = 0");
    // Stats booking: a shard's hstats IS the last attempt's counters (a full-mesh context accumulates the attempts and maps of
    // one nsk_matvec instead: map_finish)
    for (nsk_ctx* c : G) { c->hstats = h; c->hstats.steps = c->nsteps; }
    if (v == Verdict::FAIL_NOCONV)
      return fail(NSK_ENOCONV, "inner solve hit its iteration cap (sharded run): " + std::to_string(h.unconverged) + " solves, worst Helmholtz " +
                  std::to_string(h.max_helm) + " / pressure " + std::to_string(h.max_pres) + " iterations");
    if (v == Verdict::STANDS) {
      for (nsk_ctx* c : G) budgets_update(c, h);
      break;
    }
    for (nsk_ctx* c : G) c->retries++;
  }
  for (size_t r = 0; r < G.size(); ++r) { int rc = state_store(G[r], f[r]); if (rc) return rc; }
  HIPCHK(hipStreamSynchronize(G[0]->stream));
  return 0;
}
#undef FORALL
