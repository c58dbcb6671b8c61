// fcg_context.cpp -- C ABI entry points: context creation (the stages of fcg_create_plan.cpp,
// this path's FillComplete, and the upload of their tables), device-resident and host-pointer
// evaluate, timing and info.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <chrono>
#include <climits>
#include <cstdlib>
#include <cstring>
#include <mutex>
#include <string>
#include <thread>
#include <vector>

#include "fcg_internal.hpp"
#include "fcg_status.hpp"
#include "fcg_shape.hpp"
#include "fcg_upload.hpp"

namespace {

namespace plan = fcg::create;  // the host stages of fcg_create (fcg_create_plan.cpp)

std::mutex g_err_mutex;
std::string g_create_error;

void set_create_error(const std::string& s)
{
  std::lock_guard<std::mutex> lk(g_err_mutex);
  g_create_error = s;
}

using fcg::upload;

void free_mesh(fcg::DeviceMesh& m)
{
  void* ptrs[] = {m.node_dof_row, m.node_dof_kcol, m.mass_ptr, m.mass_inc, m.mass_tab, m.mass_rho, m.mass_bad, m.stress_tab, m.stress_bad, m.stress_slot, m.explicit_work, m.ele_mat, m.apply_ye, m.apply_dof, m.diag_de, m.diag_dbc, m.gather_dummy, m.multi_ptr, m.rec_row0, m.rec_meta, m.rec_base, m.rec_ele, m.rec_a, m.rec_tmap, m.ele_orig, m.inc_ele, m.inc_a, m.asm_order, m.ele_x,
      m.ele_dof, m.ele_nodes, m.ele_gid, m.node_x, m.node_dof_col, m.inc_of, m.inc_ptr,
      m.rownode_row0, m.inc_pos, m.rowptr, m.scratch, m.err, m.elem_at, m.lat_x, m.lat_dof,
      m.plane_rec, m.reg_rec, m.reg_tile, m.reg_pos,
      m.tables, m.stamps, m.col_lid, m.diag_pos, m.pcg_work, m.krylov_work, m.col_ele, m.ele_ft, m.inc_row0, m.ele_gp,
      m.pen_ptr, m.ele_nb, m.h27_rows, m.h27_rslot0, m.h27_slot};
  for (void* p : ptrs)
    if (p) (void)hipFree(p);
  if (m.err_host) (void)hipHostFree(m.err_host);
  m = fcg::DeviceMesh{};
}

// The CSR graph of the owned rows from the column elements, built by fcg_graph_build_device (the
// sorted-row graph Epetra_CrsMatrix::FillComplete gives 4C after the first assembly through the
// unfilled path, 4C_linalg_sparsematrix.cpp:578-611, 843-865), columns in the matrix column map
// (kcol), brought back to the host for the plan builders below.
int graph_on_device(const fcg_desc* d, const int32_t* kcol, std::vector<int64_t>& rowptr,
    std::vector<int32_t>& col, std::string& why)
{
  const int npe = d->celltype == FCG_HEX27 ? 27 : 8;
  if (d->n_rows % 3 != 0)
  {
    why = "n_rows must be 3 x owned nodes";
    return FCG_ERR_ARG;
  }
  for (int64_t n = 0; n < d->n_node; ++n)
    if (kcol[n] < 0 || (d->node_dof_row[n] >= 0 && d->node_dof_row[n] % 3 != 0))
    {
      why = "node DOF LIDs must be non-negative and owned rows start at multiples of 3";
      return FCG_ERR_ARG;
    }
  if (!fcg_use_device(d->device))
  {
    why = "hipSetDevice failed";
    return fcg_device_error();
  }
  int32_t *en = nullptr, *dc = nullptr, *dr = nullptr, *cl = nullptr;
  int64_t* rp = nullptr;
  int64_t bytes = 0, nnz = 0;
  hipError_t he = hipSuccess;
  auto chk = [&](hipError_t x) {
    if (he == hipSuccess) he = x;
  };
  chk(upload(&en, d->ele_nodes, d->n_ele * npe, bytes));
  chk(upload(&dc, kcol, d->n_node, bytes));
  chk(upload(&dr, d->node_dof_row, d->n_node, bytes));
  chk(upload<int64_t>(&rp, nullptr, d->n_rows + 1, bytes));
  int rc = FCG_OK;
  if (he == hipSuccess)
    rc = fcg_graph_build_device(d->device, d->celltype, d->n_ele, en, d->n_node, dc, dr, d->n_rows, rp,
        nullptr, 0, &nnz, nullptr);
  if (he == hipSuccess && rc == FCG_OK)
  {
    chk(upload<int32_t>(&cl, nullptr, std::max<int64_t>(nnz, 1), bytes));
    if (he == hipSuccess)
      rc = fcg_graph_build_device(d->device, d->celltype, d->n_ele, en, d->n_node, dc, dr, d->n_rows,
          rp, cl, nnz, &nnz, nullptr);
  }
  if (he == hipSuccess && rc == FCG_OK)
  {
    rowptr.resize(d->n_rows + 1);
    col.resize(nnz);
    chk(hipMemcpy(rowptr.data(), rp, sizeof(int64_t) * rowptr.size(), hipMemcpyDeviceToHost));
    if (nnz > 0) chk(hipMemcpy(col.data(), cl, sizeof(int32_t) * size_t(nnz), hipMemcpyDeviceToHost));
  }
  for (void* p : {static_cast<void*>(en), static_cast<void*>(dc), static_cast<void*>(dr),
           static_cast<void*>(rp), static_cast<void*>(cl)})
    if (p) (void)hipFree(p);
  if (he != hipSuccess)
  {
    why = hipGetErrorString(he);
    return fcg_device_error();
  }
  if (rc != FCG_OK) why = rc == FCG_ERR_ARG ? "row LIDs inconsistent or more than 16 elements at a node"
                                            : "device error";
  return rc;
}

// rowptr = col_lid = NULL: the graph is built on the device and `d` continues as a copy of the
// descriptor that points to it
struct DeviceGraph {
  fcg_desc desc;
  std::vector<int64_t> rowptr;
  std::vector<int32_t> col;
};
int use_device_graph(const fcg_desc*& d, DeviceGraph& G, std::string& why)
{
  if (!(d->n_rows > 0 && !d->rowptr && !d->col_lid)) return FCG_OK;
  const int rc = graph_on_device(d, plan::kcol_of(d), G.rowptr, G.col, why);
  if (rc != FCG_OK)
  {
    why = "graph on the device: " + why;
    return rc;
  }
  G.desc = *d;
  G.desc.rowptr = G.rowptr.data();
  G.desc.col_lid = G.col.data();
  d = &G.desc;
  return FCG_OK;
}

// compute units (the sweep's segment count and the hex27 element grid depend on them; 256 when
// the device cannot be queried, e.g. plan checks on a host without GPU) and memory of the device
struct DeviceFigures { int cus = 256; int64_t mem_total = 0; };
DeviceFigures query_device(int device)
{
  DeviceFigures f;
  hipDeviceProp_t prop;
  if (hipGetDeviceProperties(&prop, device) == hipSuccess)
  {
    if (prop.multiProcessorCount > 0) f.cus = prop.multiProcessorCount;
    f.mem_total = int64_t(prop.totalGlobalMem);
  }
  else
    (void)hipGetLastError();
  return f;
}

int open_context(const fcg_desc* d, fcg_ctx*& ctx, std::string& why)
{
  ctx = new fcg_ctx();
  ctx->device = d->device;
  hipError_t he = hipSetDevice(d->device);
  if (he == hipSuccess) he = hipStreamCreateWithFlags(&ctx->stream, hipStreamDefault);  // ordered with the null stream (torch's default)
  if (he != hipSuccess)
  {
    why = std::string("HIP: ") + hipGetErrorString(he);
    delete ctx;
    ctx = nullptr;
    return fcg_device_error();
  }
  fcg::upload_constant_tables(d->celltype);
  return FCG_OK;
}

// Uploads into a context's mesh: the first error wins, the later calls still run, and
// device_bytes counts what was allocated.
struct Uploader {
  fcg_ctx* ctx;
  hipError_t he = hipSuccess;
  void chk(hipError_t x)
  {
    if (he == hipSuccess) he = x;
  }
  template <class T>
  void up(T** dst, const T* src, int64_t n)
  {
    chk(upload(dst, src, n, ctx->device_bytes));
  }
  template <class T>
  void up(T** dst, const std::vector<T>& src)
  {
    up(dst, src.data(), int64_t(src.size()));
  }
  // arrays of 256 MB and more go through the context's pinned staging chunks (threaded host copy
  // overlapped with the DMA) instead of a pageable hipMemcpy: 1M hex27 moves 18.5 GB of column
  // indices and 1.5 GB of incidence positions here
  template <class T>
  void up_big(T** dst, const T* src, int64_t n)
  {
    const int64_t nbytes = n * int64_t(sizeof(T));
    if (nbytes < (int64_t(256) << 20)) return up(dst, src, n);
    hipError_t e = upload<T>(dst, nullptr, n, ctx->device_bytes);
    if (e == hipSuccess) e = fcg::staged_copy(ctx->staging, ctx->device, *dst, src, nbytes, true);
    chk(e);
  }
};

// sizes, material constants and the arrays every path reads
void upload_common(Uploader& U, const fcg_desc* d, const plan::NodeRows& N, int64_t n_inc)
{
  fcg::DeviceMesh& m = U.ctx->mesh;
  m.celltype = d->celltype;
  m.kinem = d->kinematics;
  m.npe = d->celltype == FCG_HEX27 ? 27 : 8;
  m.n_ele = d->n_ele;
  m.n_node = d->n_node;
  m.n_rows = d->n_rows;
  m.n_cols = d->n_cols;
  m.nnz = d->n_rows ? d->rowptr[d->n_rows] : 0;
  m.n_rownodes = N.nrn();
  m.n_inc = n_inc;
  m.max_rowlen = N.max_rowlen;
  // StVK constants, fill_cmat (4C_mat_stvenantkirchhoff.cpp:123-144)
  const double nu = d->poisson;
  const double mfac = d->youngs / ((1.0 + nu) * (1.0 - 2.0 * nu));
  m.cdiag = mfac * (1.0 - nu);
  m.lambda = mfac * nu;
  m.mu = mfac * 0.5 * (1.0 - 2.0 * nu);
  // Mat::Elastic::PAR::CoupNeoHooke (4C_mat_elast_coupneohooke.cpp): c, beta
  m.material = d->material;
  m.nh_c = d->youngs / (4.0 * (1.0 + nu));
  m.nh_beta = nu / (1.0 - 2.0 * nu);
  std::vector<int32_t> eg;
  if (!d->ele_gid)
  {
    eg.resize(d->n_ele);
    for (int64_t e = 0; e < d->n_ele; ++e) eg[e] = int32_t(e);
  }
  U.up_big(&m.ele_nodes, d->ele_nodes, d->n_ele * m.npe);
  U.up(&m.ele_gid, d->ele_gid ? d->ele_gid : eg.data(), d->n_ele);
  U.up(&m.node_x, d->node_x, d->n_node * 3);
  U.up(&m.node_dof_col, d->node_dof_col, d->n_node);
  // the path-independent node -> row map and matrix-column LIDs the mass kernels need
  U.up(&m.node_dof_row, d->node_dof_row, d->n_node);
  if (d->node_dof_kcol) U.up(&m.node_dof_kcol, d->node_dof_kcol, d->n_node);
  U.up(&m.rownode_row0, N.row0);
  U.up_big(&m.rowptr, d->rowptr, d->n_rows + 1);
  // operator support: column LIDs, diagonal positions (the Dirichlet rows and the Jacobi
  // preconditioner need them) and whether the matrix column map is the row map (single rank)
  m.square_local = N.square_local;
  m.owned_cols_first = N.owned_cols_first;
  m.triple_rows = N.triple_rows;
  U.up_big(&m.col_lid, d->col_lid, m.nnz);
  U.up(&m.diag_pos, N.diag);
  U.up<int32_t>(&m.err, nullptr, 3);
  if (U.he == hipSuccess) U.he = hipHostMalloc(reinterpret_cast<void**>(&m.err_host), 2 * sizeof(int32_t),
      hipHostMallocDefault);
}

void upload_structured(Uploader& U, const fcg_desc* d, const plan::StructHost& sp)
{
  fcg::DeviceMesh& m = U.ctx->mesh;
  m.path = FCG_PATH_STRUCTURED;
  m.tiles_x = sp.tiles_x;
  m.tiles_y = sp.tiles_y;
  m.tiles_z = sp.tiles_z;
  m.seg_planes = sp.seg;
  m.I0 = sp.lo[0]; m.J0 = sp.lo[1]; m.K0 = sp.lo[2];
  m.NI = sp.n[0]; m.NJ = sp.n[1]; m.NK = sp.n[2];
  m.EX0 = sp.elo[0]; m.EY0 = sp.elo[1]; m.EZ0 = sp.elo[2];
  m.EX = sp.en[0]; m.EY = sp.en[1]; m.EZ = sp.en[2];
  // The linear sweep defers each row's lower-plane blocks by one layer (MODE 3), so that a row's
  // cache lines are filled within one layer: rows not in lattice order (input-file numbering,
  // renumbered 1M box: 3.41 -> 2.23 GB written, 1.45 -> 1.30-1.35 ms, profiles/r03/defer/) and,
  // since the deferred kernel has the regular-layer emit and the branch-free hold, lattice-ordered
  // rows too (1M box: 2.34 -> 2.04 GB written, profiles/sweep_rows/).  TotLag keeps MODE 0: its
  // sweep is bound by the arithmetic at one workgroup per CU, and the extra LDS round trip cost
  // 4-6 % there.  FCG_SWEEP_DEFER=0/1 forces the choice (A/B runs, tests)
  const char* de = std::getenv("FCG_SWEEP_DEFER");
  m.sweep_defer = de && de[0] ? de[0] == '1' : d->kinematics == FCG_LINEAR;
  // FCG_SWEEP_SKIP_EMPTY=0: the element-free layers run as every other layer (A/B runs, tests)
  const char* se = std::getenv("FCG_SWEEP_SKIP_EMPTY");
  m.sweep_skip_empty = !(se && se[0] == '0');
  U.up(&m.elem_at, sp.elem_at);
  U.up(&m.lat_x, sp.lat_x);
  U.up(&m.lat_dof, sp.lat_dof);
  U.up(&m.plane_rec, sp.plane_rec);
  // regular lattice tiles (classify_regular_tiles): the unchecked linear kernels (MODE 0 and the
  // deferred MODE 3) take their closed-form row bookkeeping for the layers inside a tile's run.  A
  // context that launches other kernels, or FCG_SWEEP_REGULAR=0 at fcg_create (A/B runs, tests),
  // gets empty runs: the records' path
  const char* rg = std::getenv("FCG_SWEEP_REGULAR");
  const bool regular = !(rg && rg[0] == '0') && d->kinematics == FCG_LINEAR;
  m.layers_total = sp.layers_total;
  m.reg_layers = regular ? sp.reg_layers : 0;
  if (m.reg_layers > 0)
  {
    U.up(&m.reg_rec, sp.reg_rec);
    U.up(&m.reg_tile, sp.reg_tile);
  }
  else
  {
    const std::vector<uint32_t> no_rec(fcg::REG_REC_WORDS, 0u);
    const std::vector<int32_t> no_run(sp.reg_tile.size(), 0);
    U.up(&m.reg_rec, no_rec);
    U.up(&m.reg_tile, no_run);
  }
  int32_t pos32[32] = {};  // (indexed by the visit words' 5-bit block fields)
  std::copy(sp.reg_pos, sp.reg_pos + 27, pos32);
  U.up(&m.reg_pos, pos32, 32);
  // dN at the GPs [192] | dN at the nodes [192] | weights [8] | GP coordinates [24]
  std::vector<double> tab(8 * 8 * 3 * 2 + 8 + 24);
  double xi[81], w[27], xn[81];
  fcg::gauss_rule(fcg::kHex8, xi, w);
  fcg::node_param_coords(fcg::kHex8, xn);
  for (int g = 0; g < 8; ++g) fcg::shape_deriv(fcg::kHex8, &xi[3 * g], &tab[24 * g]);
  for (int g = 0; g < 8; ++g) fcg::shape_deriv(fcg::kHex8, &xn[3 * g], &tab[192 + 24 * g]);
  for (int g = 0; g < 8; ++g) tab[384 + g] = w[g];
  for (int k = 0; k < 24; ++k) tab[392 + k] = xi[k];
  U.up(&m.tables, tab);
  // the checks that depend on the reference coordinates alone, once: a context they pass runs the
  // sweep without them.  FCG_SWEEP_CHECKED=1 keeps the checked kernels (A/B runs, tests)
  const char* ck = std::getenv("FCG_SWEEP_CHECKED");
  if (U.he == hipSuccess) U.chk(fcg::sweep_geometry_pass(m, ck && ck[0] == '1', U.ctx->stream));
}

void upload_colored(Uploader& U, const fcg_desc* d, const plan::Incidences& I, const plan::ColorHost& cp)
{
  fcg::DeviceMesh& m = U.ctx->mesh;
  m.path = FCG_PATH_COLORED;
  U.up(&m.inc_of, I.inc_of);
  U.up(&m.inc_pos, I.inc_pos);
  U.up(&m.inc_row0, I.inc_row0);
  // hex27 StVK: the matrix-core element kernel in pencil order (4 launches, fcg_hex27.hip);
  // another material: the eight-colour element_kernel launches
  m.h27_pencil = d->material == FCG_MAT_STVK;
  if (m.h27_pencil)
  {
    fcg::upload_h27_tables();
    U.up(&m.col_ele, cp.pen_ele.data(), d->n_ele);
    U.up(&m.pen_ptr, cp.pen_ptr);
    U.up(&m.ele_nb, cp.nb.data(), d->n_ele);
    for (int c = 0; c < 5; ++c) m.pen_color[c] = cp.pen_color[c];
  }
  else
  {
    U.up(&m.col_ele, cp.col_ele.data(), d->n_ele);
    U.up(&m.ele_ft, cp.ft.data(), d->n_ele);
    for (int c = 0; c < 9; ++c) m.color_ptr[c] = cp.color_ptr[c];
  }
}

void upload_gather(Uploader& U, const fcg_desc* d, const plan::GatherHost& G)
{
  fcg::DeviceMesh& m = U.ctx->mesh;
  m.path = FCG_PATH_GATHER;
  m.n_rec = G.n_rec;
  m.n_rec_single = G.n_single;
  m.n_multi = int64_t(G.multi_ptr.size()) - 1;
  U.up(&m.ele_orig, G.eorig);
  U.up(&m.multi_ptr, G.multi_ptr);
  U.up(&m.rec_row0, G.rec_row0);
  U.up(&m.rec_meta, G.rec_meta);
  U.up(&m.rec_base, G.rec_base);
  U.up(&m.rec_ele, G.rec_ele);
  U.up(&m.rec_a, G.rec_a);
  U.up(&m.rec_tmap, G.rec_tmap);
  U.up(&m.ele_x, G.ex);
  U.up(&m.ele_dof, G.edof);
  U.up<double>(&m.gather_dummy, nullptr, 4);
  U.up(&m.tables, G.gauss);
  // the Gauss points' reference Jacobians, inverted, once for the context's lifetime
  U.up<double>(&m.ele_gp, nullptr, d->n_ele * 80);
  U.chk(fcg::gather_precompute(m, d->n_ele, U.ctx->stream));
}

// hex27 StVK on the general path: the matrix-core element kernel (fcg_hex27.hip) writing the
// incidence records, one per incidence or, under the slab schedule, in a ring
bool uses_h27s(const fcg_desc* d) { return d->celltype == FCG_HEX27 && d->material == FCG_MAT_STVK; }

void upload_hex27(Uploader& U, const fcg_desc* d, const plan::Incidences& I,
    const std::vector<int64_t>& order, const DeviceFigures& dev)
{
  fcg::DeviceMesh& m = U.ctx->mesh;
  const int64_t nrn = m.n_rownodes;
  fcg::upload_h27_tables();
  U.up(&m.inc_ele, I.inc_ele);
  U.up(&m.inc_a, I.inc_a);
  // assembly order: Morton order of the row nodes' coordinates
  std::vector<int32_t> ord32(order.begin(), order.end());
  U.up(&m.asm_order, ord32);
  size_t mem_free = 0, mem_tot = 0;
  const bool known = hipMemGetInfo(&mem_free, &mem_tot) == hipSuccess;
  if (!known) (void)hipGetLastError();
  const plan::H27Schedule s = plan::h27_schedule(d->n_ele, I.n_inc, m.nnz,
      fcg::record_doubles(27) * int64_t(sizeof(double)), known ? int64_t(mem_free) : -1, dev.mem_total,
      dev.cus, std::getenv("FCG_H27_SLAB"), std::getenv("FCG_H27_EL_GRID"));
  m.h27_el_grid = s.el_grid;
  int64_t n_slots = I.n_inc;
  if (s.slab > 0 && s.slab < d->n_ele)
  {
    plan::H27Ring R;
    plan::build_h27_ring(d->n_ele, s.slab, 0, I.inc_ptr, I.inc_ele, I.inc_a, order, R);
    m.h27_nslab = R.nslab;
    m.h27_slab = s.slab;
    m.h27_ring = R.ring;
    m.h27_asm_ptr = R.asm_ptr;
    n_slots = R.ring;
    U.up(&m.h27_rows, R.rows.data(), nrn);
    U.up(&m.h27_rslot0, R.rslot0.data(), nrn);
    U.up(&m.h27_slot, R.slot.data(), d->n_ele * 27);
  }
  U.up<double>(&m.scratch, nullptr, n_slots * fcg::record_doubles(27));
}

void upload_general(Uploader& U, const fcg_desc* d, const plan::Incidences& I,
    const std::vector<int64_t>& h27_order, const DeviceFigures& dev)
{
  fcg::DeviceMesh& m = U.ctx->mesh;
  m.path = FCG_PATH_GENERAL;
  U.up(&m.inc_of, I.inc_of);
  U.up(&m.inc_ptr, I.inc_ptr);
  U.up_big(&m.inc_pos, I.inc_pos.data(), int64_t(I.inc_pos.size()));
  m.h27s = uses_h27s(d);
  if (m.h27s)
    upload_hex27(U, d, I, h27_order, dev);
  else
    U.up<double>(&m.scratch, nullptr, I.n_inc * fcg::record_doubles(m.npe));
}

// diagnostics (tools/stamps.py): FCG_STAMPS=1 turns on the kernels' per-phase s_memtime counters
void upload_stamps(Uploader& U)
{
  const char* st = std::getenv("FCG_STAMPS");
  if (!(st && st[0] == '1')) return;
  const unsigned long long zero[16] = {};
  U.up(&U.ctx->mesh.stamps, zero, 16);
}

// wall time of fcg_create's phases (fcg_get_create_phases)
struct PhaseClock {
  double ph[8] = {0, 0, 0, 0, 0, 0, 0, 0};
  const std::chrono::steady_clock::time_point t_start = std::chrono::steady_clock::now();
  std::chrono::steady_clock::time_point t_last = t_start;
  void done(int i)
  {
    const auto now = std::chrono::steady_clock::now();
    ph[i] += std::chrono::duration<double>(now - t_last).count();
    t_last = now;
  }
};

}  // namespace

extern "C" {

const char* fcg_last_error(const fcg_ctx* ctx)
{
  if (ctx) return ctx->last_error.c_str();
  std::lock_guard<std::mutex> lk(g_err_mutex);
  return g_create_error.c_str();
}

// The stages of a context's creation, in order; the host ones are fcg_create_plan.cpp's.  Every
// FCG_ERR_ARG is found before the first device call (the device graph, else open_context).
int fcg_create(const fcg_desc* d, fcg_ctx** out)
{
  PhaseClock clock;
  if (!d || !out) return FCG_ERR_ARG;
  *out = nullptr;
  std::string why;
  int rc = FCG_OK;
  auto failed = [&](int code) {
    rc = code;
    if (rc != FCG_OK) set_create_error(why);
    return rc != FCG_OK;
  };
  if (failed(plan::check_descriptor(d, why))) return rc;
  clock.done(0);
  DeviceGraph graph;
  if (failed(use_device_graph(d, graph, why))) return rc;
  clock.done(1);
  plan::NodeRows rows;
  if (failed(plan::build_node_rows(d, rows, why))) return rc;
  clock.done(2);
  const DeviceFigures dev = query_device(d->device);
  plan::PathChoice choice;
  if (failed(plan::choose_path(d, rows, dev.cus, choice, why))) return rc;
  clock.done(3);
  plan::Incidences inc;
  if (failed(plan::build_incidences(d, rows, choice, inc, why))) return rc;
  clock.done(4);
  if (failed(plan::build_incidence_positions(d, rows, choice, inc, why))) return rc;
  clock.done(5);
  // the rest of the chosen path's host plan (no error exit)
  plan::build_operator_support(d, rows);
  plan::GatherHost gather;
  if (choice.gather) plan::build_gather_plan(d, rows, inc, gather);
  std::vector<int64_t> h27_order;  // hex27 StVK assembly order
  if (choice.path() == FCG_PATH_GENERAL && uses_h27s(d)) h27_order = plan::rownode_morton_order(d, rows);

  fcg_ctx* ctx = nullptr;
  if (failed(open_context(d, ctx, why))) return rc;
  Uploader U{ctx};
  upload_common(U, d, rows, inc.n_inc);
  switch (choice.path())
  {
    case FCG_PATH_STRUCTURED: upload_structured(U, d, choice.sp); break;
    case FCG_PATH_COLORED: upload_colored(U, d, inc, choice.cp); break;
    case FCG_PATH_GATHER: upload_gather(U, d, gather); break;
    default: upload_general(U, d, inc, h27_order, dev);
  }
  upload_stamps(U);
  for (auto& ev : ctx->timing.ev) U.chk(hipEventCreate(&ev));
  if (U.he != hipSuccess)
  {
    set_create_error(std::string("HIP allocation/copy failed: ") + hipGetErrorString(U.he));
    fcg_destroy(ctx);
    return fcg_device_error();
  }
  clock.done(6);
  clock.ph[7] = std::chrono::duration<double>(clock.t_last - clock.t_start).count();
  for (int i = 0; i < 8; ++i) ctx->create_phase_s[i] = clock.ph[i];
  *out = ctx;
  return FCG_OK;
}

int fcg_destroy(fcg_ctx* ctx)
{
  if (!ctx) return FCG_OK;
  (void)hipSetDevice(ctx->device);
  free_mesh(ctx->mesh);
  for (auto& ev : ctx->timing.ev)
    if (ev) (void)hipEventDestroy(ev);
  if (ctx->stream) (void)hipStreamDestroy(ctx->stream);
  if (ctx->h_u) (void)hipFree(ctx->h_u);
  if (ctx->h_f) (void)hipFree(ctx->h_f);
  if (ctx->h_k) (void)hipFree(ctx->h_k);
  fcg::staging_free(ctx->staging);
  delete ctx;
  return FCG_OK;
}

}  // extern "C"

namespace {

// The error flags of the evaluates queued since the last check (4C's throws).
int report_error(fcg_ctx* ctx, int32_t* bad_ele_gid)
{
  fcg::DeviceMesh& m = ctx->mesh;
  const int32_t* errv = m.err_host;
  m.err_clean = errv[0] == 0;  // no failing element: err still {0, INT32_MAX}
  if (errv[0] == 0) return FCG_OK;
  int32_t gid = -1;
  if (errv[1] >= 0 && errv[1] < m.n_ele)
    (void)hipMemcpy(&gid, m.ele_gid + errv[1], sizeof(int32_t), hipMemcpyDeviceToHost);
  if (bad_ele_gid) *bad_ele_gid = gid;
  ctx->last_error = errv[0] == FCG_ERR_NODAL_DETJ
                        ? "determinant of jacobian <= 0 at one node of element " + std::to_string(gid)
                        : "singular 3x3 matrix in element " + std::to_string(gid);
  return errv[0];
}

void read_timing(fcg::Timing& T)
{
  if (!T.pending) return;
  T.pending = false;
  float a = 0.f, b = 0.f;
  if (hipEventSynchronize(T.ev[2]) != hipSuccess) return;
  (void)hipEventElapsedTime(&a, T.ev[0], T.ev[1]);
  (void)hipEventElapsedTime(&b, T.ev[1], T.ev[2]);
  T.ms_element = a;
  // fused kernels and the hex27 slab schedule: evaluate + assembly in ms_element
  T.ms_element = T.fused ? a + b : a;
  T.ms_assemble = T.path == FCG_PATH_GENERAL && !T.fused ? b : 0.0;
}

}  // namespace

namespace fcg {

hipError_t staged_copy(HostStaging& st, int device, void* dst, const void* src, int64_t bytes,
    bool to_device)
{
  if (bytes <= 0) return hipSuccess;
  if (st.threads <= 0)
    return hipMemcpy(dst, src, bytes, to_device ? hipMemcpyHostToDevice : hipMemcpyDeviceToHost);
  hipError_t he = hipSuccess;
  if (!st.stream)
  {
    st.chunk = int64_t(32) << 20;  // bytes per chunk
    he = hipStreamCreateWithFlags(&st.stream, hipStreamNonBlocking);
    for (int b = 0; b < 2 && he == hipSuccess; ++b)
    {
      he = hipHostMalloc(reinterpret_cast<void**>(&st.pin[b]), st.chunk);
      if (he == hipSuccess) he = hipEventCreateWithFlags(&st.ev[b], hipEventDisableTiming);
    }
    if (he != hipSuccess) return he;
  }
  (void)device;
  const int64_t n_chunks = (bytes + st.chunk - 1) / st.chunk;
  auto host_copy = [&](char* d, const char* s, int64_t len) {
    const int nt = int(std::min<int64_t>(st.threads, std::max<int64_t>(1, len >> 22)));
    if (nt <= 1)
    {
      std::memcpy(d, s, len);
      return;
    }
    std::vector<std::thread> th;
    const int64_t part = (len + nt - 1) / nt;
    for (int t = 0; t < nt; ++t)
    {
      const int64_t a = t * part, e = std::min(len, a + part);
      if (a < e) th.emplace_back([=]() { std::memcpy(d + a, s + a, e - a); });
    }
    for (auto& x : th) x.join();
  };
  char* D = static_cast<char*>(dst);
  const char* S = static_cast<const char*>(src);
  if (to_device)
  {
    // host copy of chunk i into pin[i % 2] overlaps the DMA of chunk i - 1
    for (int64_t i = 0; i < n_chunks && he == hipSuccess; ++i)
    {
      const int b = int(i & 1);
      const int64_t off = i * st.chunk, len = std::min(st.chunk, bytes - off);
      if (i >= 2) he = hipEventSynchronize(st.ev[b]);  // the DMA that last read pin[b] is done
      if (he != hipSuccess) break;
      host_copy(reinterpret_cast<char*>(st.pin[b]), S + off, len);
      he = hipMemcpyAsync(D + off, st.pin[b], len, hipMemcpyHostToDevice, st.stream);
      if (he == hipSuccess) he = hipEventRecord(st.ev[b], st.stream);
    }
  }
  else
  {
    // DMA of chunk i + 1 overlaps the host copy of chunk i
    auto issue = [&](int64_t i) {
      const int b = int(i & 1);
      const int64_t off = i * st.chunk, len = std::min(st.chunk, bytes - off);
      hipError_t e = hipMemcpyAsync(st.pin[b], S + off, len, hipMemcpyDeviceToHost, st.stream);
      if (e == hipSuccess) e = hipEventRecord(st.ev[b], st.stream);
      return e;
    };
    he = issue(0);
    for (int64_t i = 0; i < n_chunks && he == hipSuccess; ++i)
    {
      const int b = int(i & 1);
      he = hipEventSynchronize(st.ev[b]);
      if (he == hipSuccess && i + 1 < n_chunks) he = issue(i + 1);
      if (he != hipSuccess) break;
      const int64_t off = i * st.chunk, len = std::min(st.chunk, bytes - off);
      host_copy(D + off, reinterpret_cast<const char*>(st.pin[b]), len);
    }
  }
  if (he == hipSuccess) he = hipStreamSynchronize(st.stream);
  return he;
}

void staging_free(HostStaging& st)
{
  for (int b = 0; b < 2; ++b)
  {
    if (st.pin[b]) (void)hipHostFree(st.pin[b]);
    if (st.ev[b]) (void)hipEventDestroy(st.ev[b]);
    st.pin[b] = nullptr;
    st.ev[b] = nullptr;
  }
  if (st.stream) (void)hipStreamDestroy(st.stream);
  st.stream = nullptr;
}

}  // namespace fcg

extern "C" {

int fcg_evaluate_device(fcg_ctx* ctx, int action, int mode, const double* d_u_col,
    double* d_fint_row, double* d_K_vals, void* stream_ptr, int32_t* bad_ele_gid)
{
  if (!ctx) return FCG_ERR_ARG;
  fcg::DeviceMesh& m = ctx->mesh;
  const bool want_k = (action == FCG_CALC_NLNSTIFF);
  if ((action != FCG_CALC_NLNSTIFF && action != FCG_CALC_INTERNALFORCE) ||
      (mode != FCG_ACCUMULATE && mode != FCG_OVERWRITE) ||
      (m.n_ele > 0 && !d_u_col) || (m.n_rows > 0 && !d_fint_row) ||
      (want_k && m.nnz > 0 && !d_K_vals))
  {
    ctx->last_error = "invalid evaluate arguments";
    return FCG_ERR_ARG;
  }
  (void)hipSetDevice(ctx->device);
  hipStream_t s = stream_ptr ? static_cast<hipStream_t>(stream_ptr) : ctx->stream;
  const int32_t init[2] = {0, INT32_MAX};
  hipError_t he = hipSuccess;
  // a pending evaluate on another stream must have written its flags first
  if (ctx->pending && ctx->pending_stream != s) he = hipStreamSynchronize(ctx->pending_stream);
  if (he == hipSuccess && !m.err_clean)
  {
    he = hipMemcpyAsync(m.err, init, sizeof(init), hipMemcpyHostToDevice, s);
    m.err_clean = true;  // re-initialised in stream order
  }
  auto& T = ctx->timing;
  if (T.enabled && he == hipSuccess) he = hipEventRecord(T.ev[0], s);
  if (m.path == FCG_PATH_STRUCTURED)
  {
    if (he == hipSuccess)
      he = fcg::launch_sweep_h8(m, d_u_col, want_k, mode == FCG_OVERWRITE, d_K_vals, d_fint_row, s);
    if (T.enabled && he == hipSuccess) he = hipEventRecord(T.ev[1], s);
  }
  else if (m.path == FCG_PATH_COLORED)
  {
    if (he == hipSuccess)
      he = m.h27_pencil ? fcg::launch_h27_pencil(m, d_u_col, want_k, mode == FCG_OVERWRITE, d_K_vals,
                              d_fint_row, s)
                        : fcg::launch_element_colored(m, d_u_col, want_k, mode == FCG_OVERWRITE,
                              d_K_vals, d_fint_row, s);
    if (T.enabled && he == hipSuccess) he = hipEventRecord(T.ev[1], s);
  }
  else if (m.path == FCG_PATH_GATHER)
  {
    if (he == hipSuccess)
      he = fcg::launch_gather_h8(m, d_u_col, want_k, mode == FCG_OVERWRITE, d_K_vals, d_fint_row, s);
    if (T.enabled && he == hipSuccess) he = hipEventRecord(T.ev[1], s);
  }
  else if (m.h27_nslab > 1)
  {
    // hex27 slab schedule: slab s's elements, then the rows whose last element it holds
    for (int64_t sl = 0; sl < m.h27_nslab && he == hipSuccess; ++sl)
    {
      he = fcg::launch_h27_element(m, d_u_col, want_k, s, sl * m.h27_slab,
          std::min(m.n_ele, (sl + 1) * m.h27_slab));
      if (he == hipSuccess)
        he = fcg::launch_assemble27_slab(m, sl, want_k, mode == FCG_OVERWRITE, d_K_vals, d_fint_row, s);
    }
    if (T.enabled && he == hipSuccess) he = hipEventRecord(T.ev[1], s);
  }
  else
  {
    if (he == hipSuccess)
      he = m.h27s ? fcg::launch_h27_element(m, d_u_col, want_k, s)
                  : fcg::launch_element(m, d_u_col, want_k, s);
    if (T.enabled && he == hipSuccess) he = hipEventRecord(T.ev[1], s);
    if (he == hipSuccess)
      he = fcg::launch_assemble(m, want_k, mode == FCG_OVERWRITE, d_K_vals, d_fint_row, s);
  }
  if (T.enabled && he == hipSuccess)
  {
    he = hipEventRecord(T.ev[2], s);
    T.pending = true;
    T.path = m.path;
    T.fused = m.path == FCG_PATH_GENERAL && m.h27_nslab > 1;
  }
  // async: the flags stay sticky on the device across queued evaluates and fcg_check_error reads
  // them once (a read-back per evaluate would put a copy between every two evaluates' kernels)
  if (he == hipSuccess && !ctx->async)
    he = hipMemcpyAsync(m.err_host, m.err, 2 * sizeof(int32_t), hipMemcpyDeviceToHost, s);
  if (he == hipSuccess && ctx->async)
  {
    ctx->pending = true;
    ctx->pending_stream = s;
    return FCG_OK;  // fcg_check_error reports what the queued work finds
  }
  if (he == hipSuccess) he = hipStreamSynchronize(s);
  if (he != hipSuccess)
  {
    m.err_clean = false;
    ctx->pending = false;
    ctx->last_error = std::string("HIP: ") + hipGetErrorString(he);
    return fcg_device_error();
  }
  ctx->pending = false;
  read_timing(T);
  return report_error(ctx, bad_ele_gid);
}

int fcg_set_async(fcg_ctx* ctx, int enable)
{
  if (!ctx) return FCG_ERR_ARG;
  if (!enable && ctx->pending)
  {
    const int rc = fcg_check_error(ctx, nullptr);
    ctx->async = false;
    return rc;
  }
  ctx->async = enable != 0;
  return FCG_OK;
}

int fcg_check_error(fcg_ctx* ctx, int32_t* bad_ele_gid)
{
  if (!ctx) return FCG_ERR_ARG;
  if (!ctx->pending) return FCG_OK;
  (void)hipSetDevice(ctx->device);
  ctx->pending = false;
  if (hipMemcpyAsync(ctx->mesh.err_host, ctx->mesh.err, 2 * sizeof(int32_t), hipMemcpyDeviceToHost,
          ctx->pending_stream) != hipSuccess ||
      hipStreamSynchronize(ctx->pending_stream) != hipSuccess)
  {
    ctx->mesh.err_clean = false;
    ctx->last_error = "HIP: stream failed";
    return fcg_device_error();
  }
  return report_error(ctx, bad_ele_gid);
}

int fcg_evaluate_host(fcg_ctx* ctx, int action, int mode, const double* u_col, double* fint_row,
    double* K_vals, int32_t* bad_ele_gid)
{
  if (!ctx) return FCG_ERR_ARG;
  fcg::DeviceMesh& m = ctx->mesh;
  const bool want_k = (action == FCG_CALC_NLNSTIFF) && K_vals;
  if ((action != FCG_CALC_NLNSTIFF && action != FCG_CALC_INTERNALFORCE) ||
      (mode != FCG_ACCUMULATE && mode != FCG_OVERWRITE) || (m.n_cols && !u_col) ||
      (m.n_rows && !fint_row))
  {
    ctx->last_error = "invalid evaluate arguments";
    return FCG_ERR_ARG;
  }
  (void)hipSetDevice(ctx->device);
  if (ctx->pending)
  {
    const int rc = fcg_check_error(ctx, bad_ele_gid);
    if (rc != FCG_OK) return rc;
  }
  static const char* thr = std::getenv("FCG_HOST_COPY_THREADS");
  ctx->staging.threads = thr ? std::atoi(thr) : 8;
  hipError_t he = hipSuccess;
  if (!ctx->h_u && m.n_cols) he = hipMalloc(&ctx->h_u, sizeof(double) * m.n_cols);
  if (he == hipSuccess && !ctx->h_f && m.n_rows) he = hipMalloc(&ctx->h_f, sizeof(double) * m.n_rows);
  if (he == hipSuccess && want_k && !ctx->h_k && m.nnz) he = hipMalloc(&ctx->h_k, sizeof(double) * m.nnz);
  const bool acc = mode == FCG_ACCUMULATE;
  if (he == hipSuccess)
    he = fcg::staged_copy(ctx->staging, ctx->device, ctx->h_u, u_col, sizeof(double) * m.n_cols, true);
  if (he == hipSuccess && acc)
    he = fcg::staged_copy(ctx->staging, ctx->device, ctx->h_f, fint_row, sizeof(double) * m.n_rows, true);
  if (he == hipSuccess && acc && want_k)
    he = fcg::staged_copy(ctx->staging, ctx->device, ctx->h_k, K_vals, sizeof(double) * m.nnz, true);
  if (he != hipSuccess)
  {
    ctx->last_error = std::string("HIP: ") + hipGetErrorString(he);
    return fcg_device_error();
  }
  const bool was_async = ctx->async;
  ctx->async = false;
  const int rc = fcg_evaluate_device(ctx, want_k ? FCG_CALC_NLNSTIFF : FCG_CALC_INTERNALFORCE, mode,
      ctx->h_u, ctx->h_f, ctx->h_k, nullptr, bad_ele_gid);
  ctx->async = was_async;
  if (rc != FCG_OK) return rc;
  he = fcg::staged_copy(ctx->staging, ctx->device, fint_row, ctx->h_f, sizeof(double) * m.n_rows, false);
  if (he == hipSuccess && want_k)
    he = fcg::staged_copy(ctx->staging, ctx->device, K_vals, ctx->h_k, sizeof(double) * m.nnz, false);
  if (he != hipSuccess)
  {
    ctx->last_error = std::string("HIP: ") + hipGetErrorString(he);
    return fcg_device_error();
  }
  return FCG_OK;
}

int fcg_evaluate(fcg_ctx* ctx, int action, const double* u_col, double* fint_row, double* K_vals,
    int32_t* bad_ele_gid)
{
  return fcg_evaluate_host(ctx, action, FCG_ACCUMULATE, u_col, fint_row, K_vals, bad_ele_gid);
}

int fcg_set_timing(fcg_ctx* ctx, int enable)
{
  if (!ctx) return FCG_ERR_ARG;
  ctx->timing.enabled = enable != 0;
  return FCG_OK;
}

int fcg_get_timing(const fcg_ctx* ctx, double* ms_element, double* ms_assemble)
{
  if (!ctx) return FCG_ERR_ARG;
  read_timing(const_cast<fcg_ctx*>(ctx)->timing);
  if (ms_element) *ms_element = ctx->timing.ms_element;
  if (ms_assemble) *ms_assemble = ctx->timing.ms_assemble;
  return 2;
}

int fcg_get_diagnostics(const fcg_ctx* ctx, uint64_t* out, int n)
{
  if (!ctx || !out || n < 0) return FCG_ERR_ARG;
  const fcg::DeviceMesh& m = ctx->mesh;
  unsigned long long v[16] = {};
  if (m.stamps && hipMemcpy(v, m.stamps, sizeof(v), hipMemcpyDeviceToHost) != hipSuccess)
    return fcg_device_error();
  // slot 15 (no kernel counts there): the sweep kernels of this context
  v[15] = m.path != FCG_PATH_STRUCTURED ? FCG_SWEEP_KERNEL_NA
                                        : (m.sweep_checked ? FCG_SWEEP_KERNEL_CHECKED : FCG_SWEEP_KERNEL_UNCHECKED);
  // slots 13, 14 (no kernel counts there either): the (tile, layer) pairs of the structured sweep
  // that take the regular-tile path (none in a context that keeps the checked kernels), and all
  v[13] = m.path == FCG_PATH_STRUCTURED && !m.sweep_checked ? uint64_t(m.reg_layers) : 0;
  v[14] = m.path == FCG_PATH_STRUCTURED ? uint64_t(m.layers_total) : 0;
  // slot 12 (no kernel counts there either): how the sweep's tangent kernels write a row
  v[12] = m.path != FCG_PATH_STRUCTURED ? FCG_SWEEP_ROWS_NA
                                        : (m.sweep_defer ? FCG_SWEEP_ROWS_DEFERRED : FCG_SWEEP_ROWS_DIRECT);
  for (int i = 0; i < n && i < 16; ++i) out[i] = v[i];
  return m.stamps ? 16 : 0;
}

int fcg_get_create_phases(const fcg_ctx* ctx, double* out, int n)
{
  if (!ctx || (!out && n > 0)) return FCG_ERR_ARG;
  for (int i = 0; i < n && i < 8; ++i) out[i] = ctx->create_phase_s[i];
  return 8;
}

int fcg_get_info(const fcg_ctx* ctx, fcg_info* info)
{
  if (!ctx || !info) return FCG_ERR_ARG;
  const fcg::DeviceMesh& m = ctx->mesh;
  info->n_ele = m.n_ele;
  info->n_node = m.n_node;
  info->n_rows = m.n_rows;
  info->n_cols = m.n_cols;
  info->nnz = m.nnz;
  info->n_incidences = m.n_inc;
  info->scratch_bytes = !m.scratch ? 0
                                   : (m.h27_nslab > 1 ? m.h27_ring : m.n_inc) *
                                         fcg::record_doubles(m.npe) * int64_t(sizeof(double));
  info->device_bytes = ctx->device_bytes;
  info->path = m.path;
  info->h27_slabs =
      m.path == FCG_PATH_GENERAL && m.h27s ? int32_t(std::max<int64_t>(1, m.h27_nslab)) : 0;
  return FCG_OK;
}

int fcg_set_element_materials(fcg_ctx* ctx, int32_t n_mat, const double* youngs,
    const double* poisson, const int32_t* ele_mat)
{
  if (!ctx) return FCG_ERR_ARG;
  fcg::DeviceMesh& m = ctx->mesh;
  auto refuse = [&](const std::string& why) {
    ctx->last_error = "fcg_set_element_materials: " + why;
    return FCG_ERR_ARG;
  };
  // every check comes before the first change: a refused call leaves the context as it was
  if (n_mat < 0) return refuse("n_mat = " + std::to_string(n_mat) + " must be >= 0");
  if (n_mat > 0)
  {
    if (m.path == FCG_PATH_STRUCTURED || m.path == FCG_PATH_COLORED)
      return refuse(std::string("the ") + (m.path == FCG_PATH_STRUCTURED ? "structured sweep" : "coloured lattice assembly") +
                    " takes one material per context; create the context with FCG_PATH_GATHER (hex8) "
                    "or FCG_PATH_GENERAL");
    if (!youngs || !poisson || (m.n_ele > 0 && !ele_mat))
      return refuse("n_mat > 0 needs youngs, poisson and ele_mat (one of them is NULL)");
    // Mat::PAR::StVenantKirchhoff parameter checks, as fcg_create's
    for (int32_t k = 0; k < n_mat; ++k)
    {
      if (!(youngs[k] > 0.0))
        return refuse("youngs[" + std::to_string(k) + "] = " + std::to_string(youngs[k]) + " must be > 0");
      if (!(poisson[k] < 0.5) || !(poisson[k] >= -1.0))
        return refuse("poisson[" + std::to_string(k) + "] = " + std::to_string(poisson[k]) +
                      " must lie in [-1;0.5)");
    }
    for (int64_t e = 0; e < m.n_ele; ++e)
      if (ele_mat[e] < 0 || ele_mat[e] >= n_mat)
        return refuse("ele_mat[" + std::to_string(e) + "] = " + std::to_string(ele_mat[e]) +
                      " outside [0, n_mat = " + std::to_string(n_mat) + ")");
  }
  (void)hipSetDevice(ctx->device);
  // queued evaluates read the table that is about to go
  hipError_t he = hipStreamSynchronize(ctx->stream);
  if (he == hipSuccess && ctx->pending && ctx->pending_stream != ctx->stream)
    he = hipStreamSynchronize(ctx->pending_stream);
  const int64_t tab_bytes = m.n_ele * 4 * int64_t(sizeof(double));
  double* fresh = nullptr;
  if (he == hipSuccess && n_mat > 0 && m.n_ele > 0)
  {
    // the constants of fcg_create, by the same host arithmetic
    std::vector<double> c(size_t(n_mat) * 4, 0.0);
    for (int32_t k = 0; k < n_mat; ++k)
    {
      const double nu = poisson[k];
      if (m.material == FCG_MAT_STVK)
      {
        const double mfac = youngs[k] / ((1.0 + nu) * (1.0 - 2.0 * nu));
        c[4 * k + 0] = mfac * nu;
        c[4 * k + 1] = mfac * 0.5 * (1.0 - 2.0 * nu);
        c[4 * k + 2] = mfac * (1.0 - nu);
      }
      else
      {
        c[4 * k + 0] = youngs[k] / (4.0 * (1.0 + nu));
        c[4 * k + 1] = nu / (1.0 - 2.0 * nu);
      }
    }
    // FCG_PATH_GATHER keeps its elements in storage-slot (Morton) order
    std::vector<int32_t> orig;
    if (m.path == FCG_PATH_GATHER)
    {
      orig.resize(m.n_ele);
      he = hipMemcpy(orig.data(), m.ele_orig, sizeof(int32_t) * size_t(m.n_ele), hipMemcpyDeviceToHost);
    }
    std::vector<double> tab(size_t(m.n_ele) * 4);
    for (int64_t i = 0; i < m.n_ele; ++i)
    {
      const int64_t e = orig.empty() ? i : orig[i];
      for (int q = 0; q < 4; ++q) tab[4 * i + q] = c[4 * size_t(ele_mat[e]) + q];
    }
    int64_t unused = 0;
    if (he == hipSuccess) he = upload(&fresh, tab.data(), m.n_ele * 4, unused);
  }
  if (he != hipSuccess)
  {
    if (fresh) (void)hipFree(fresh);
    ctx->last_error = std::string("fcg_set_element_materials: HIP: ") + hipGetErrorString(he);
    return fcg_device_error();
  }
  if (m.ele_mat)
  {
    (void)hipFree(m.ele_mat);
    ctx->device_bytes -= tab_bytes;
  }
  m.ele_mat = fresh;
  if (fresh) ctx->device_bytes += tab_bytes;
  m.n_mat = n_mat;
  return FCG_OK;
}

int fcg_get_graph(const fcg_ctx* ctx, int64_t* rowptr, int32_t* col_lid, int64_t col_capacity,
    int64_t* nnz)
{
  if (!ctx || !nnz) return FCG_ERR_ARG;
  const fcg::DeviceMesh& m = ctx->mesh;
  *nnz = m.nnz;
  if (col_lid && col_capacity < m.nnz) return FCG_ERR_ARG;
  if (!fcg_use_device(ctx->device)) return fcg_device_error();
  hipError_t he = hipSuccess;
  if (rowptr && m.n_rows > 0)
    he = hipMemcpy(rowptr, m.rowptr, sizeof(int64_t) * size_t(m.n_rows + 1), hipMemcpyDeviceToHost);
  else if (rowptr)
    rowptr[0] = 0;
  if (he == hipSuccess && col_lid && m.nnz > 0)
    he = hipMemcpy(col_lid, m.col_lid, sizeof(int32_t) * size_t(m.nnz), hipMemcpyDeviceToHost);
  return he == hipSuccess ? FCG_OK : fcg_device_error();
}

int fcg_device_alloc(int device, int64_t bytes, void** d_ptr)
{
  if (!d_ptr || bytes < 0) return FCG_ERR_ARG;
  if (!fcg_use_device(device)) return fcg_device_error();
  return hipMalloc(d_ptr, bytes > 0 ? bytes : 1) == hipSuccess ? FCG_OK : fcg_device_error();
}
int fcg_device_free(void* p) { return hipFree(p) == hipSuccess ? FCG_OK : fcg_device_error(); }
int fcg_memcpy_h2d(void* dst, const void* src, int64_t n)
{
  return hipMemcpy(dst, src, n, hipMemcpyHostToDevice) == hipSuccess ? FCG_OK : fcg_device_error();
}
int fcg_memcpy_d2h(void* dst, const void* src, int64_t n)
{
  return hipMemcpy(dst, src, n, hipMemcpyDeviceToHost) == hipSuccess ? FCG_OK : fcg_device_error();
}
int fcg_memset_device(void* dst, int v, int64_t n)
{
  return hipMemset(dst, v, n) == hipSuccess ? FCG_OK : fcg_device_error();
}

}  // extern "C"
