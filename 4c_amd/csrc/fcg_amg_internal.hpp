// fcg_amg_internal.hpp -- the structural AMG's handle and types, shared by its three translation
// units: fcg_amg_solver.hip (host hierarchy build, single-rank numeric setup, smoother, V-cycle,
// flexible CG), fcg_amg_coupled.hip (the coarse levels coupled across ranks) and fcg_amg_api.hip
// (the C ABI).  Not part of the public ABI.
#pragma once

#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstdint>
#include <string>
#include <vector>

#include "fcg_amg_shared.hpp"
#include "fcg_internal.hpp"
#include "fcg_status.hpp"
#include "fourc_gpu.h"

namespace fcg_amgs {

inline unsigned blocks_for(int64_t n) { return unsigned((n + kBlock - 1) / kBlock); }

struct Bsr {
  int64_t n = 0, nnzb = 0, n_cols = 0;
  int br = 0, bc = 0;
  std::vector<int64_t> ptr_h;
  std::vector<int32_t> col_h;
  int64_t* ptr = nullptr;
  int32_t* col = nullptr;
  double* vals = nullptr;
};

// product plan of one Galerkin SpGEMM (fcg_bsr_product_plan): per C block its (A, B) block pairs
struct Plan {
  int64_t* ptr = nullptr;
  int32_t *a = nullptr, *b = nullptr;
  int64_t* order = nullptr;  // C blocks by (aggregate of the row, row), or NULL
};

struct Step {  // level l -> l + 1
  int bs = 3;
  int64_t n_agg = 0;
  Bsr T, P, AT, AP, Pt;
  Plan pAT, pAP, pC;  // A T, A P, P^T (A P); empty: the searching kernel (FCG_AMG_PLAN=0)
  int32_t* agg = nullptr;
  double* tent = nullptr;   // [n][bs][6], every row's T_i
  int64_t* perm = nullptr;  // P^T block -> P block
};

struct Level {  // coarse level (6 x 6 blocks)
  Bsr A;
  int64_t* diag = nullptr;
  double* dinv = nullptr;
  double lmax = 0.0;
  double *x = nullptr, *b = nullptr, *r = nullptr, *d = nullptr, *z = nullptr, *p = nullptr, *q = nullptr;
};

struct Coupled;  // (below: the handle and it point at each other)

}  // namespace fcg_amgs

struct fcg_amg {
  fcg_ctx* ctx = nullptr;
  int device = 0;
  fcg_amg_options opt{};
  int64_t n0 = 0, nb0 = 0;
  fcg_amgs::Bsr A0;
  int64_t* A0_diag = nullptr;
  double* A0_dinv = nullptr;    // BSR block inverses of level 0 (prolongator smoothing)
  double* ctx_dinv = nullptr;   // the context's block-Jacobi of level 0 (smoother)
  double* mask0 = nullptr;      // 0 on the Dirichlet rows
  double lmax0 = 0.0;
  double *r0 = nullptr, *d0 = nullptr, *z0 = nullptr, *q0 = nullptr, *p0 = nullptr, *ro0 = nullptr,
         *fr = nullptr, *fz = nullptr, *fx = nullptr;
  std::vector<fcg_amgs::Step> steps;
  std::vector<fcg_amgs::Level> levels;  // levels[l] = hierarchy level l + 1
  double* partial = nullptr;  // dot partials
  double* sc = nullptr;       // device scalars
  int32_t* flag = nullptr;
  double* agree = nullptr;    // [2] fcg_amg_precond_setup's go/no-go all-reduce
  std::string last_error;
  std::vector<void*> allocs;
  double setup_ms = 0.0;
  bool ready = false;  // a numeric setup has been made (fcg_amg_setup or the coupled setup)
  // the rank-local hierarchy (lmax0, the Galerkin levels, the coarse inverse) matches the last K:
  // set by fcg_amg_setup, cleared by the coupled numeric setup, which refreshes only the block
  // inverses the coupled V-cycle smooths with -- fcg_amg_apply / fcg_amg_iterate need it
  bool local_ready = false;
  // rank-local preconditioner of a multi-rank context: level 0 is the owned block (ghost column
  // triples dropped) and is applied through its BSR copy instead of the context's fcg_spmv
  bool local = false;
  std::vector<double> ns1;  // level 1's near-null space [n_agg][6][6] (R factors of step 0)
  std::vector<int64_t> full_ptr;  // local: block pattern of the rank's whole rows (column nodes)
  std::vector<int32_t> full_col;
  // the coarse levels coupled across ranks (fcg_dfcg_solve with a local handle): built on the
  // first solve through its transport, see fcg_amgs::Coupled
  fcg_amgs::Coupled* cpl = nullptr;
  // the coarsest level's dense inverse (coarse_solve applies it when set; else block-Jacobi CG):
  // formed per tangent by block Gauss-Jordan between the two buffers when the level has at most
  // kDenseMax DOFs (FCG_AMG_DENSE=0: never)
  double* cbuf[2] = {nullptr, nullptr};
  double* cwork = nullptr;  // the block elimination's pivot inverse and panels
  double* cinv = nullptr;
  int64_t cn = 0;
  // one FCG iteration of fcg_amg_iterate captured as a HIP graph on a private stream (re-captured
  // after every numeric setup and when K or x move), opt-in with FCG_AMG_GRAPH=1: at the 1M-element
  // scale the kernels leave no launch gaps to remove and the replay measured 1-2 % slower.  Only
  // with the dense coarsest inverse: the CG coarse solve reads its residual on the host.
  hipStream_t gs = nullptr;
  hipEvent_t gev[2] = {nullptr, nullptr};
  hipGraphExec_t gexec = nullptr;
  const double* g_K = nullptr;
  double* g_x = nullptr;
  bool graph_off = false;
  int graph_launches = 0;
  // single rank: level 0 renumbered in the Morton order of the node coordinates (a renumbered
  // mesh's input order scatters every row's neighbours over the vectors; FCG_AMG_REORDER=0 keeps
  // the context's order).  Level 0 is then the BSR copy A0 in that order: its SpMV and block
  // Jacobi run on A0, the iteration's vectors are permuted on entry and exit.
  int32_t* new2old = nullptr;  // [nb0] context node of level-0 node p (NULL: no reordering)
  int32_t* old_k = nullptr;    // [A0.nnzb] triple index of each A0 block in its context row
  double *pb = nullptr, *px = nullptr;  // permuted right-hand side / solution
};

namespace fcg_amgs {

struct Fail {
  int code;
  std::string msg;
};

inline void ck(hipError_t e, const char* what)
{
  if (e != hipSuccess)
  {
    (void)hipGetLastError();  // leave no sticky status for the caller (fcg_status.hpp)
    throw Fail{FCG_ERR_DEVICE, std::string(what) + ": " + hipGetErrorString(e)};
  }
}
inline void ck(int rc, const char* what)
{
  if (rc != FCG_OK) throw Fail{rc, what};
}

template <typename T>
T* dalloc(fcg_amg* h, int64_t n)
{
  void* p = nullptr;
  ck(hipMalloc(&p, sizeof(T) * size_t(std::max<int64_t>(n, 1))), "hipMalloc");
  h->allocs.push_back(p);
  return static_cast<T*>(p);
}
template <typename T>
T* upload(fcg_amg* h, const std::vector<T>& v)
{
  T* d = dalloc<T>(h, int64_t(v.size()));
  if (!v.empty()) ck(hipMemcpy(d, v.data(), sizeof(T) * v.size(), hipMemcpyHostToDevice), "hipMemcpy");
  return d;
}

// ---- coarse levels coupled across ranks (fcg_dfcg_solve with a rank-local handle) -------------
// 4C's MueLu hierarchy spans every rank (4C_linear_solver_preconditioner_muelu.cpp:97: one
// Xpetra operator over the global matrix).  Here the aggregation stays rank-local (as MueLu's
// uncoupled aggregation), everything else is of the GLOBAL matrix, solved redundantly on every rank
// below level 1:
//   * T_0's rows of the ghost nodes come from their owners through the transport's import (the
//     global aggregate id, then the 3 x 6 block's six columns), so that the prolongator is smoothed
//     with the global operator, P = (I - omega D^-1 A) T_ext, lambda_max of D^-1 A by a Lanczos over
//     the ranks: P's rows near a rank boundary reach the neighbours' aggregates;
//   * P's ghost rows the same way (fixed-width channels per block slot, M the widest row over the
//     ranks), then this rank's part of A_1 = P^T (A_full P_ext) by the block SpGEMM on host-built
//     patterns (A_full: the rank's whole rows, ghost columns included);
//   * the global A_1 pattern is the union of the ranks' parts (their (row, column) pairs gathered
//     once, sorted identically everywhere); per tangent each rank scatters its blocks into a zeroed
//     global buffer and the transport's all-reduce sums them;
//   * a hierarchy built from the gathered A_1 by the same aggregation code (coarsen), replicated and
//     identical on every rank (same input, deterministic build and kernels);
//   * application: one V-cycle of the global system -- Chebyshev on the global operator (each of
//     its SpMVs one import + the rank's rows), the residual restricted into the global level-1
//     vector (all-reduce), the replicated hierarchy, prolongation, Chebyshev again (coupled_apply).
struct DevBuf {
  double* p = nullptr;
  explicit DevBuf(int64_t n) { ck(hipMalloc(&p, sizeof(double) * size_t(std::max<int64_t>(1, n))), "hipMalloc"); }
  ~DevBuf() { if (p) (void)hipFree(p); }
  DevBuf(const DevBuf&) = delete;
  DevBuf& operator=(const DevBuf&) = delete;
};

// a fixed point-to-point exchange pattern of the distributed level: items per rank in rank
// order (the width of an item is chosen per call)
struct Xch {
  std::vector<int64_t> scnt, rcnt;  // items to / from each rank
  int64_t ns = 0, nr = 0;
  std::vector<int64_t> sd, rd;      // the current call's doubles per rank
  void finish()
  {
    ns = nr = 0;
    for (int64_t v : scnt) ns += v;
    for (int64_t v : rcnt) nr += v;
  }
};

// Level 1 distributed across the ranks (fcg_transport::exchange_fn; MueLu keeps every level of its
// hierarchy a distributed Xpetra operator, 4C_linear_solver_preconditioner_muelu.cpp:97).  Global
// aggregate ids are numbered by rank (rank q owns [agg_off[q], agg_off[q + 1])).  Each rank keeps
//   * LA: the aggregates its P_0 rows and their ghost rows reach, ascending global id (its own at
//     [own0, own0 + na)); P_0, P_0^T, P_ext and this rank's partial A_1 = P^T A P_ext (C) use it;
//   * A: the owned rows of A_1, columns DA = ascending global ids (own at [d0, d0 + na)), summed
//     from C's own rows and the partial rows the other ranks send to the owner (fixed order: own
//     blocks, then the senders in rank order -- bitwise reproducible);
//   * three exchange patterns: the partial rows (36 doubles per block, per numeric setup), the
//     import of A's ghost columns (per level-1 SpMV), and LA's other-rank entries with their owners
//     (restriction: sent and added by the owner; prolongation: the reverse);
//   * level 2: a rank-local aggregation of A's owned block, its tentative prolongator T_1 smoothed
//     with the distributed A_1, P_1 = (I - w D^-1 A_1) T_1,ext (T_1's ghost rows imported once,
//     P_1's per tangent in M1 fixed slots), and A_2 = P_1^T (A_1 P_1,ext) gathered by the all-reduce
//     and solved redundantly by the replicated hierarchy (the replication moves down one level;
//     with T_1 unsmoothed, 32^3 hex27 on 4 ranks took 184 FCG iterations against 130 on one);
//   * or, while level 2 is still past the replication threshold (distribute_level), level 2 is a
//     Dist of its own (next) built the same way from C2, down to the level that is replicated:
//     the replicated bytes then stay bounded by the threshold whatever the rank count.
struct Dist {
  int R = 1, me = 0;
  std::vector<int64_t> agg_off;  // [R + 1]
  int64_t na = 0, off = 0;
  int64_t NL = 0, own0 = 0;
  int64_t NA = 0, d0 = 0;
  Bsr A;
  int64_t* diag = nullptr;
  double* dinv = nullptr;
  double lmax = 0.0;
  int64_t c_lo = 0, c_hi = 0;  // C's owned-row blocks
  int64_t* pos_own = nullptr;  // [c_hi - c_lo] their blocks of A
  Xch rows;
  int64_t* pos_recv = nullptr;  // [rows.nr] A block of each received partial block
  double *rows_s = nullptr, *rows_r = nullptr;
  Xch imp;
  int32_t* imp_idx = nullptr;  // [imp.ns] owned aggregate of each item sent
  std::vector<int32_t> imp_idx_h;
  double *imp_s = nullptr, *imp_r = nullptr, *xe = nullptr;
  Xch pex;
  int32_t* pex_idx = nullptr;  // [pex.nr] owned aggregate of each item received (restriction)
  double *pex_s = nullptr, *pex_r = nullptr, *y = nullptr;
  double *x = nullptr, *b = nullptr, *r = nullptr, *dd = nullptr, *z = nullptr, *p = nullptr, *q = nullptr;
  int64_t n2 = 0, off2 = 0, n2_tot = 0;
  int32_t* agg1 = nullptr;  // [na] global level-2 aggregate of each owned level-1 node (-1 = none)
  double* tent1 = nullptr;  // [na][6][6] T_1's blocks
  Bsr T1ext;  // NA x n2_tot: T_1's rows of A's columns (global level-2 ids)
  Bsr AT1;    // na x n2_tot
  Bsr P1;     // na x n2_tot: (I - w D^-1 A) T_1,ext
  Bsr P1t;    // n2_tot x na
  int64_t* p1_perm = nullptr;
  int M1 = 0;        // blocks per row of P_1, widest over the ranks
  Bsr P1ext;  // NA x n2_tot: P_1's rows of A's columns, the ghost ones imported per tangent
  double *p1_s = nullptr, *p1_r = nullptr;
  Bsr AP1;    // na x n2_tot
  Bsr C2;     // n2_tot x n2_tot: this rank's part of A_2 = P_1^T A P_1,ext
  // the next level distributed in turn (its global size past the replication threshold): the
  // columns of P_1 (and P_1,ext, AP_1, C2's rows and columns, agg1) are then numbered by the next
  // level's LA (its NL entries) instead of the global level-2 ids, and C2 is its partial-rows input
  int level = 1;
  int64_t n2_cols = 0;  // the column space of P_1: n2_tot, or the next level's NL
  Dist* next = nullptr;
  ~Dist() { delete next; }
};

struct Coupled {
  int rank = 0, nranks = 1;
  int64_t nc_nodes = 0;            // column nodes of the context (owned first, then ghosts)
  int64_t off = 0, n_agg_tot = 0;  // this rank's first global aggregate; all ranks' aggregates
  int M = 0;                       // blocks per row of P, widest over the ranks
  Bsr Afull;                       // owned block rows x column nodes (3 x 3)
  Bsr Text;                        // column nodes x aggregates: T_0 rows, ghosts imported
  Bsr AT;                          // owned block rows x aggregates (3 x 6)
  Bsr P;                           // owned block rows x aggregates: (I - w D^-1 A) T
  Bsr Pt;                          // its transpose: aggregates x owned block rows
  int64_t* p_perm = nullptr;       // P^T block -> P block
  int32_t* agg = nullptr;          // [nb0] aggregate of each owned node in P's numbering (-1 = none)
  Bsr Pext;                        // column nodes x aggregates: P rows, ghosts imported
  Bsr AP;                          // owned block rows x aggregates (3 x 6)
  Bsr C;                           // this rank's part of A_1 = P^T A P
  // the replicated level (A_1, or A_2 with a distributed level 1): this rank's blocks and their
  // positions in the replicated operator, which the all-reduce sums
  const Bsr* rep_part = nullptr;
  int64_t* rep_pos = nullptr;      // [rep_part->nnzb] block position in the replicated operator
  int64_t rep_nnzb = 0, rep_n = 0; // replicated operator: blocks, block rows
  double *chan = nullptr, *chan_col = nullptr, *q = nullptr, *w = nullptr, *gb = nullptr, *ge = nullptr;
  fcg_amg* g = nullptr;            // the replicated hierarchy: g->levels[0].A = the replicated operator
  double lmax0 = 0.0;              // lambda_max of D^-1 A for the global operator
  Dist* d = nullptr;               // level 1 distributed (with exchange_fn), else NULL (A_1 replicated)
  // collective traffic (doubles; fcg_amg_coupled_stats): counters of the running phase, and the
  // last numeric setup's and preconditioner application's totals
  int64_t ctr_ar = 0, ctr_x = 0;
  int64_t ar_setup = 0, ar_apply = 0, x_setup = 0, x_apply = 0;
  ~Coupled() { delete d; }
};

// A transport whose every collective is preceded by a status all-reduce (one double: 0 on a rank
// still going).  The coupled build and numeric setup run over it, so a rank that throws between
// two collectives (a malformed pattern, a singular level-1 block found by dist_setup, a HIP error)
// joins the other ranks at their next collective with its status 1 instead of its payload
// (guard_fail below); every rank then stops there together and returns an error.  The status
// all-reduce is a host round trip per collective of the setup, never of the application.
struct Guard {
  const fcg_transport* in = nullptr;
  fcg_amg* h = nullptr;
  hipStream_t s = nullptr;
  bool remote = false;   // a checkpoint saw another rank's failure (this rank joined it)
  int64_t checkpoints = 0;
  int64_t fail_at = -1;  // test hook: throw on reaching this checkpoint (a failure inside the build)
};

// level 0: the context's SpMV (single rank), or the owned block's BSR copy (local)
void apply_A0(fcg_amg* h, const double* K, const double* x, double* y, hipStream_t s);
// the operators of the coupled levels (fcg_amg_coupled.hip): level 0's global one, a distributed
// level's owned rows and its block Jacobi
void coupled_spmv(fcg_amg* h, const double* K, const fcg_transport* tr, const double* x, double* y, hipStream_t s);
void dist_spmv(fcg_amg* h, Dist* d, const fcg_transport* tr, const double* x, double* y, hipStream_t s);
void dist_dinv(fcg_amg* h, const Dist* d, const double* r, double* z, double scale, bool acc, hipStream_t s);

// a level's operator and smoother pieces: l = 0 the context, l >= 1 levels[l - 1]
struct Ops {
  fcg_amg* h;
  int l;
  const double* K;  // level 0 values
  hipStream_t s;
  // level 0 of a rank-local handle with coupled coarse levels: the global operator (import + the
  // rank's SpMV) and its lambda_max instead of the owned block's
  const fcg_transport* tr = nullptr;
  Dist* dl = nullptr;  // the distributed level 1 (tr: its imports and inner products)
  int64_t n() const { return dl ? 6 * dl->na : l == 0 ? h->n0 : h->levels[size_t(l - 1)].A.n * 6; }
  void spmv(const double* x, double* y) const
  {
    if (dl)
      dist_spmv(h, dl, tr, x, y, s);
    else if (l == 0 && tr)
      coupled_spmv(h, K, tr, x, y, s);
    else if (l == 0)
      apply_A0(h, K, x, y, s);
    else
    {
      const Bsr& A = h->levels[size_t(l - 1)].A;
      ck(fcg_bsr_spmv(h->device, 6, 6, A.n, A.ptr, A.col, A.vals, x, y, 1.0, 0, s), "fcg_bsr_spmv");
    }
  }
  void dinv(const double* r, double* z, double scale, bool acc) const
  {
    if (dl)
      dist_dinv(h, dl, r, z, scale, acc, s);
    else if (l == 0 && h->new2old)  // reordered level 0: its BSR block inverses
      ck(fcg_bsr_block_jacobi_apply(h->device, 3, h->nb0, h->A0_dinv, r, z, scale, acc ? 1 : 0, s),
          "fcg_bsr_block_jacobi_apply (level 0)");
    else if (l == 0)
      ck(fcg_block_jacobi_apply(h->ctx, h->ctx_dinv, r, z, scale, acc ? 1 : 0, s), "fcg_block_jacobi_apply");
    else
    {
      const Level& L = h->levels[size_t(l - 1)];
      ck(fcg_bsr_block_jacobi_apply(h->device, 6, L.A.n, L.dinv, r, z, scale, acc ? 1 : 0, s),
          "fcg_bsr_block_jacobi_apply");
    }
  }
  double& lmax() const
  {
    return dl ? dl->lmax : l == 0 ? (tr ? h->cpl->lmax0 : h->lmax0) : h->levels[size_t(l - 1)].lmax;
  }
  double* r() const { return dl ? dl->r : l == 0 ? h->r0 : h->levels[size_t(l - 1)].r; }
  double* d() const { return dl ? dl->dd : l == 0 ? h->d0 : h->levels[size_t(l - 1)].d; }
  double* z() const { return dl ? dl->z : l == 0 ? h->z0 : h->levels[size_t(l - 1)].z; }
  double* p() const { return dl ? dl->p : l == 0 ? h->p0 : h->levels[size_t(l - 1)].p; }
  double* q() const { return dl ? dl->q : l == 0 ? h->q0 : h->levels[size_t(l - 1)].q; }
};

// ---- fcg_amg_solver.hip -----------------------------------------------------------------------
bool env_off(const char* name);  // the environment variable is set to "0"
void make_bsr(fcg_amg* h, Bsr& M, std::vector<int64_t> ptr, std::vector<int32_t> col, int br, int bc,
    int64_t n_cols);
void symbolic(const Bsr& A, const std::vector<int64_t>& bp, const std::vector<int32_t>& bc_,
    int64_t n_cols, std::vector<int64_t>& cp, std::vector<int32_t>& cc);
std::vector<int64_t> diag_index(const Bsr& A);
void coarsen(fcg_amg* h, const Bsr* A_start, int bs, std::vector<double> ns, const uint8_t* skip);
void rsub(const double* b, double* y, int64_t n, hipStream_t s);  // y = b - y
// node triples from the context's order into level 0's (to_ctx = 0) or back (to_ctx = 1)
void node_perm(fcg_amg* h, const double* src, double* dst, int to_ctx, hipStream_t s);
void estimate_lmax(const Ops& o);
void cheb(const fcg_amg* hc, const Ops& o, const double* b, double* x, bool x_zero);
void vcycle(fcg_amg* h, int l, const double* K, const double* b, double* x, hipStream_t s);
void galerkin_from(fcg_amg* h, size_t l0, const double* K, hipStream_t s);
void setup(fcg_amg* h, const double* K, hipStream_t s);
void setup_coupled_local(fcg_amg* h, const double* K, hipStream_t s);
void run_fcg(fcg_amg* h, const double* K, const double* b, double* x, double rtol, int max_iter,
    int* iterations, double* rel, hipStream_t s);

// ---- fcg_amg_coupled.hip ----------------------------------------------------------------------
void coupled_build(fcg_amg* h, const fcg_transport* tr, hipStream_t s);
void coupled_setup(fcg_amg* h, const double* K, const fcg_transport* tr, hipStream_t s);
void coupled_apply(fcg_amg* h, const double* K, const fcg_transport* tr, const double* r, double* z,
    hipStream_t s);
int64_t hierarchy_bytes(const fcg_amg* g);
bool guard_checkpoint(Guard* g, double mine);
fcg_transport guarded(const fcg_transport* tr, Guard* g);

}  // namespace fcg_amgs
