// fcg_internal.hpp -- context layout and kernel launch interface shared by the HIP translation
// units of libfourc_gpu.  Not part of the public ABI (include/fourc_gpu.h).
#pragma once

#include <hip/hip_runtime.h>

#include <cstdint>
#include <string>
#include <vector>

#include "fcg_create_plan.hpp"  // PLANE_REC_WORDS, the host plan structs
#include "fourc_gpu.h"

namespace fcg {

// Per-incidence scratch record written by the element kernel and consumed by the row-assembly
// kernel: the element's block-row of node a (3 rows x 3*npe columns, b-major) then f_a (3).
// One owned incidence's block row (3 x 3 npe) and its 3 residual entries.  hex27: padded to
// FCG_REC27 = 256 doubles so that records start on 128-byte lines.  Unpadded (246) measured the
// same (profiles/r06/r06_h27_record_store_ab.txt); shrinking it changes scratch_bytes and the
// memory the context takes, so that is a change of its own.
#ifndef FCG_REC27
#define FCG_REC27 256
#endif
constexpr int64_t record_doubles(int npe) { return npe == 27 ? int64_t(FCG_REC27) : 9 * int64_t(npe) + 3; }

struct DeviceMesh {
  int celltype = 0, kinem = 0, npe = 8;
  int64_t n_ele = 0, n_node = 0, n_rows = 0, n_cols = 0, nnz = 0;
  int64_t n_rownodes = 0, n_inc = 0;
  double lambda = 0, mu = 0, cdiag = 0;  // StVK: C_00 = cdiag, C_01 = lambda, C_33 = mu
  int material = FCG_MAT_STVK;
  double nh_c = 0, nh_beta = 0;          // ElastHyper/CoupNeoHooke constants
  // Per-element material constants (fcg_set_element_materials), NULL = the uniform ones above:
  // [n_ele][4] = lambda, mu, cdiag, 0 (StVK) or nh_c, nh_beta, 0, 0 (CoupNeoHooke), one 32-byte
  // record per element in the order the path's kernels walk the elements -- column-element order,
  // FCG_PATH_GATHER: storage-slot (Morton) order, ele_mat[slot] belongs to element ele_orig[slot].
  // The kernels that honour it are separate instantiations (template parameter TAB).
  double* ele_mat = nullptr;
  int32_t n_mat = 0;

  int32_t* ele_nodes = nullptr;     // [n_ele][npe]
  int32_t* ele_gid = nullptr;       // [n_ele]
  double* node_x = nullptr;         // [n_node][3]
  int32_t* node_dof_col = nullptr;  // [n_node]
  int32_t* inc_of = nullptr;        // [n_ele][npe] incidence id or -1
  int64_t* inc_ptr = nullptr;       // [n_rownodes+1]
  int32_t* rownode_row0 = nullptr;  // [n_rownodes]
  uint16_t* inc_pos = nullptr;      // [n_inc][npe] column position of node b in the row
  int64_t* rowptr = nullptr;        // [n_rows+1]
  double* scratch = nullptr;        // [n_inc][record_doubles(npe)]
  int32_t* err = nullptr;           // [3]: code, min failing element index; [2] the solver flag
  // (Dirichlet / block-Jacobi / PCG kernels write only err[2], so a failed element's flags from an
  // async evaluate survive them until fcg_check_error reads them)
  // evaluate's error-flag protocol: err holds {0, INT32_MAX} between calls while err_clean is set
  // (no per-call re-initialisation); whatever else writes err clears err_clean.  The flags come
  // back through the pinned err_host (a DMA, not a staged pageable copy).
  int32_t* err_host = nullptr;      // [2], pinned host memory
  bool err_clean = false;
  int32_t max_rowlen = 0;

  // colour-ordered direct assembly (hex27 on a verified lattice, FCG_PATH_COLORED)
  int32_t* col_ele = nullptr;       // [n_ele] elements sorted by colour (lattice parity), then index
  int64_t color_ptr[9] = {0, 0, 0, 0, 0, 0, 0, 0, 0};  // col_ele range of colour c
  uint8_t* ele_ft = nullptr;        // [n_ele] first-touch bits (see fcg_kernels.hip)
  int32_t* inc_row0 = nullptr;      // [n_inc] row LID of the incidence's node
  // hex27 StVK on a verified lattice: the matrix-core element kernel in pencil order (fcg_hex27.hip)
  bool h27_pencil = false;
  int64_t* pen_ptr = nullptr;       // [n_pencils+1] pencil ranges in col_ele (pencil order)
  int64_t pen_color[5] = {0, 0, 0, 0, 0};  // pencil range of colour c
  uint32_t* ele_nb = nullptr;       // [n_ele] lattice neighbours present | ey & 1 << 27 | ez & 1 << 28

  // node-row gather plan (hex8, FCG_PATH_GATHER): a row node's incidences in records of <= 8
  // records: one per node with <= 8 elements [0, n_rec_single), then those of the other nodes
  int64_t n_rec = 0, n_rec_single = 0, n_multi = 0;
  int64_t* multi_ptr = nullptr;     // [n_multi+1] record range of each node with > 8 elements
  int32_t* rec_row0 = nullptr;      // [n_rec] first row LID of the record's node
  int32_t* rec_meta = nullptr;      // [n_rec] slots | first record << 4 | last record << 5 | row length << 8
  int64_t* rec_base = nullptr;      // [n_rec] CSR offset of the node's first row
  int32_t* rec_ele = nullptr;       // [n_rec][8] element of each slot, -1 = empty
  uint8_t* rec_a = nullptr;         // [n_rec][8] local node of the row node in the slot's element
  uint32_t* rec_tmap = nullptr;     // [n_rec][32] per column triple: slot s's element node in nibble s (8 = none)
  // hex27 StVK general path (fcg_hex27.hip): the matrix-core element kernel writes the incidence
  // records in `scratch`, assemble27_kernel sums them
  bool h27s = false;
  int32_t* inc_ele = nullptr;       // [n_inc] element of each incidence
  uint8_t* inc_a = nullptr;         // [n_inc] local node of the row node in that element
  int32_t* asm_order = nullptr;     // [n_rownodes] row nodes in Morton order of their coordinates
  int32_t* ele_orig = nullptr;      // [n_ele] column element index of each storage slot (Morton order)
  double* ele_x = nullptr;          // [n_ele][8][3] element node coordinates (storage slot order)
  double* ele_gp = nullptr;         // [n_ele][8][10] Gauss-point factors (gather_precompute)
  int32_t gp_bad_code = 0, gp_bad_ele = 0;  // a Jacobian failure found by gather_precompute
  int32_t* ele_dof = nullptr;       // [n_ele][8] column LID of each element node's first DOF
  double* gather_dummy = nullptr;   // [4] store target of a row without columns
  double* apply_ye = nullptr;       // [n_inc][3] fcg_tangent_apply's node parts (allocated on first use)
  int32_t* apply_dof = nullptr;     // [n_ele][27] column LID of each element node's first DOF (idem)
  double* diag_de = nullptr;        // [n_inc + 1][6] fcg_tangent_diag's incidence blocks (allocated on first use)
  uint8_t* diag_dbc = nullptr;      // [n_rows] fcg_tangent_diag's Dirichlet row marks (idem)
  // hex27 slab schedule (FCG_H27_SLAB): the elements run in slabs of h27_slab consecutive
  // elements; after slab s the row nodes whose last incident element lies in slab s are assembled,
  // so an incidence record lives only from its slab to its row's slab, in a ring of h27_ring
  // records (instead of one record per incidence)
  int64_t h27_nslab = 0, h27_slab = 0, h27_ring = 0;
  int h27_el_grid = 512;             // element workgroups per slab launch (the resident ones)
  std::vector<int64_t> h27_asm_ptr;  // [h27_nslab + 1] range of h27_rows assembled after slab s
  int32_t* h27_rows = nullptr;       // [n_rownodes] row nodes by completing slab, then Morton order
  int32_t* h27_rslot0 = nullptr;     // [n_rownodes] ring slot of the row node's first record
  int32_t* h27_slot = nullptr;       // [n_ele][27] ring slot of incidence (e, a), -1 = not owned

  // structured (row-block sweep) plan, hex8 only
  int path = FCG_PATH_GENERAL;
  int32_t tiles_x = 0, tiles_y = 0, tiles_z = 0, seg_planes = 0;
  int32_t I0 = 0, J0 = 0, K0 = 0, NI = 0, NJ = 0, NK = 0;  // owned-node lattice box
  int32_t EX0 = 0, EY0 = 0, EZ0 = 0, EX = 0, EY = 0, EZ = 0;  // column-element lattice box
  bool sweep_defer = false;         // linear kinematics: sweep MODE 3, whole rows in one layer (fcg_sweep.hip)
  // the linear structural sweep leaves out the layers that hold no element (below and above the
  // element box); FCG_SWEEP_SKIP_EMPTY=0 at fcg_create runs them as every other layer
  bool sweep_skip_empty = true;
  // the reference-geometry checks, taken once at create (sweep_geometry_pass): the worst code, the
  // lowest rejected column element and whether some evaluated element has fac < 0 at a Gauss point.
  // sweep_checked: the evaluates launch the kernels that repeat these checks (something was found,
  // or FCG_SWEEP_CHECKED=1); else the CHECKED = false instantiations.
  int32_t geom_code = 0, geom_ele = INT32_MAX;
  bool geom_neg = false, sweep_checked = true;
  int32_t* elem_at = nullptr;       // [EZ][EY][EX] column element or -1
  double* lat_x = nullptr;          // [EZ+1][EY+1][EX+1][3] node coordinates on the lattice
  int32_t* lat_dof = nullptr;       // [EZ+1][EY+1][EX+1] column LID of the node's first DOF or -1
  uint32_t* plane_rec = nullptr;    // [tiles_y][tiles_x][NK][PLANE_REC_WORDS] row bookkeeping
  // regular lattice tiles (fcg_create_plan.hpp, classify_regular_tiles): compact records, the plane
  // run of each tile (empty when the context does not use them) and the neighbour-position pattern
  uint32_t* reg_rec = nullptr;      // [tiles_y][tiles_x][NK][REG_REC_WORDS]
  int32_t* reg_tile = nullptr;      // [tiles_y][tiles_x][2]
  int32_t* reg_pos = nullptr;       // [32], 27 used
  int64_t reg_layers = 0, layers_total = 0;  // (tile, layer) pairs on the regular path / in all
  double* tables = nullptr;         // dN at GPs [192], dN at nodes [192], weights [8]
  unsigned long long* stamps = nullptr;  // diagnostic phase timers (FCG_STAMPS=1), else NULL

  // operator / solver support (fcg_solver.hip)
  int32_t* col_lid = nullptr;       // [nnz] CSR column LIDs (matrix column map)
  int64_t* diag_pos = nullptr;      // [n_rows] position of the diagonal entry in K values, -1 = none
  bool square_local = false;        // matrix column map == row map (single rank)
  bool owned_cols_first = false;    // column LID of every owned DOF == its row LID (ghosts after)
  bool triple_rows = true;          // every node row is made of DOF triples (c, c+1, c+2) only
  double* pcg_work = nullptr;       // PCG vectors and partial sums (allocated on first solve)
  int64_t pcg_n = 0;

  // mass (fcg_mass.hip).  The node -> row map and the matrix-column LIDs are kept by fcg_create on
  // every path (the sweep and the gather hold no inc_of); the plan is built on the first mass call.
  int32_t* node_dof_row = nullptr;   // [n_node] row LID of the node's first DOF, -1 = not owned
  int32_t* node_dof_kcol = nullptr;  // [n_node] matrix-column LID, NULL = node_dof_col
  int64_t* mass_ptr = nullptr;       // [n_node+1] incidence range of each column node with a row
  int64_t* mass_inc = nullptr;       // element * 32 + local node, ascending per node
  double* mass_tab = nullptr;        // N | dN | w at the Gauss points of the stiffness rule
  double* mass_rho = nullptr;        // [n_ele] per-element densities of the last call that gave them
  int32_t* mass_bad = nullptr;       // [1] lowest column element with det J <= 0 at a Gauss point

  // stress output (fcg_stress.hip), built on the first fcg_gp_stress / fcg_gp_to_nodes
  double* stress_tab = nullptr;      // dN | w at the Gauss points of the stiffness rule | X^-1
  double* stress_xinv = nullptr;     // [npe][ngp] inside stress_tab: Gauss points -> nodes
  int32_t* stress_bad = nullptr;     // [2] lowest column element with det J <= 0 / with det F == 0
  int32_t* stress_slot = nullptr;    // [n_ele] FCG_PATH_GATHER: ele_mat record of column element e

  // explicit dynamics (fcg_explicit.hip), allocated on the first call that reduces: the
  // per-workgroup partials of the kinetic energy / the row bound (calls on one context that use
  // it must be stream-ordered, as with pcg_work), then the bound and the lowest refused row
  double* explicit_work = nullptr;   // [kExplicitPartials + 2]

  // FGMRES (fcg_krylov.hip): both bases, the partial sums, the scalar block and the front's
  // preconditioner blocks, allocated on the first solve and regrown when a solve needs more
  double* krylov_work = nullptr;
  int64_t krylov_doubles = 0;
};
constexpr int kExplicitPartials = 2048;  // the grid cap of the streaming kernels of fcg_explicit.hip

// Launches the structured hex8 row-block sweep (element evaluation + assembly, fcg_sweep.hip).
hipError_t launch_sweep_h8(const DeviceMesh& m, const double* d_u_col, bool want_k,
    bool overwrite, double* d_K, double* d_fint, hipStream_t stream);

// The sweep's reference-geometry checks, once per context, after lat_x, elem_at and the tile plan
// are on the device; fills m.geom_* and m.sweep_checked (drains the stream).
hipError_t sweep_geometry_pass(DeviceMesh& m, bool force_checked, hipStream_t stream);

// Fused TSI blocks of the structured sweep (fcg_tsi_evaluate_fused): linear kinematics, StVK,
// node-consistent thermo numbering (thermo LID = structural LID / 3, see fcg_tsi.hip).
struct SweepTsi {
  const double* v_col = nullptr;
  const double* T_col = nullptr;
  const double* Ngp = nullptr;  // shape values at the hex8 Gauss points [8][8]
  double* Kst = nullptr;
  double* Kts = nullptr;
  double* Ktt = nullptr;
  double* fT = nullptr;
  double m = 0, T0 = 0, conduct = 0, kts = 0;  // kts = -timefac timefac_d
  bool split = true;  // structural sweep + thermal-only pass (FCG_TSI_SPLIT=0: one fused pass)
};
hipError_t launch_sweep_h8_tsi(const DeviceMesh& m, const double* d_u_col, bool overwrite,
    double* d_K, double* d_fint, const SweepTsi& t, hipStream_t stream);

struct Timing {
  bool enabled = false;
  bool pending = false;  // events recorded, durations not read yet (async evaluate)
  int path = 0;
  bool fused = false;  // ev[1] marks no element/assembly boundary (hex27 slab schedule)
  hipEvent_t ev[3] = {nullptr, nullptr, nullptr};
  double ms_element = 0.0, ms_assemble = 0.0;
};

// Host <-> device copies of the host-buffer entry points through pinned staging chunks: the DMA
// of one chunk overlaps the host-side copy of the previous one (threads > 0), or one pageable
// hipMemcpy (threads == 0).
struct HostStaging {
  double* pin[2] = {nullptr, nullptr};
  hipEvent_t ev[2] = {nullptr, nullptr};
  hipStream_t stream = nullptr;
  int64_t chunk = 0;  // doubles per chunk
  int threads = 8;
};
hipError_t staged_copy(HostStaging& st, int device, void* dst, const void* src, int64_t bytes,
    bool to_device);
void staging_free(HostStaging& st);

void upload_constant_tables(int celltype);  // GP / nodal derivative tables -> __constant__
hipError_t launch_element(const DeviceMesh& m, const double* d_u_col, bool want_k,
    hipStream_t stream);
// Colour-ordered direct assembly (FCG_PATH_COLORED): eight element launches, one per colour,
// each adding (or, first in colour order, writing) its blocks straight into the CSR rows.
hipError_t launch_element_colored(const DeviceMesh& m, const double* d_u_col, bool want_k,
    bool overwrite, double* d_K, double* d_fint, hipStream_t stream);
hipError_t launch_assemble(const DeviceMesh& m, bool want_k, bool overwrite, double* d_K,
    double* d_fint, hipStream_t stream);
// hex27 StVK on any mesh (fcg_hex27.hip): the element kernel writes one record per owned
// incidence (its 3 x 81 block row + f_a) for elements [e_begin, e_end) (e_end < 0: all), which
// launch_assemble (assemble27_kernel) sums per owned row node.
void upload_h27_tables();
hipError_t launch_h27_element(const DeviceMesh& m, const double* d_u_col, bool want_k,
    hipStream_t stream, int64_t e_begin = 0, int64_t e_end = -1);
// hex27 slab schedule: the row assembly of the row nodes completed by slab s
hipError_t launch_assemble27_slab(const DeviceMesh& m, int64_t s, bool want_k, bool overwrite,
    double* d_K, double* d_fint, hipStream_t stream);
// hex27 StVK on a verified lattice: the same element kernel adding its blocks straight into the
// CSR rows, four colour launches of pencils (runs of elements along x, one workgroup each)
hipError_t launch_h27_pencil(const DeviceMesh& m, const double* d_u_col, bool want_k,
    bool overwrite, double* d_K, double* d_fint, hipStream_t stream);
// Matrix-free tangent action y_row = K(u) x_col of hex27 StVK (fcg_tangent_apply): the element
// kernel writes each owned incidence's 3 values to m.apply_ye, a row-node pass sums them.
hipError_t launch_h27_apply(const DeviceMesh& m, const double* d_u_col, const double* d_x_col,
    double* d_y_row, hipStream_t stream);
hipError_t launch_h27_apply_plan(const DeviceMesh& m, hipStream_t stream);  // fills m.apply_dof
// Matrix-free nodal diagonal blocks of K(u) of hex27 StVK (fcg_tangent_diag): the element kernel
// writes each owned incidence's 6 values to m.diag_de, a row-node pass sums them, replaces the
// Dirichlet rows by unit rows and writes the blocks and / or their inverses (9 per row node,
// row-major).  flag: the solver flag word (1: singular or NaN block, 2: a row outside the map).
hipError_t launch_h27_diag(const DeviceMesh& m, const double* d_u_col, int64_t n_dbc,
    const int32_t* d_dbc_rows, double* d_diag, double* d_dinv, int32_t* flag, hipStream_t stream);
// Node-row gather (FCG_PATH_GATHER, hex8 StVK or ElastHyper/CoupNeoHooke on any mesh): one
// wavefront per owned row node (fcg_gather.hip).
hipError_t gather_precompute(DeviceMesh& m, int64_t n_ele, hipStream_t stream);
hipError_t launch_gather_h8(const DeviceMesh& m, const double* d_u_col, bool want_k, bool overwrite,
    double* d_K, double* d_fint, hipStream_t stream);
// Mass (fcg_mass.hip).  mass_plan_build: the per-node incidence lists and the shape table, once
// per context (bytes: added to the context's device_bytes; drains the stream).  launch_mass: one
// wavefront per owned row node integrates its mass row into the CSR values (d_M), the compact
// node form (d_m_node, nnz / 9) and / or the row sums (d_lumped); det J <= 0 at a Gauss point sets
// the solver flag word and m.mass_bad.  launch_effective_tangent: K <- cK K + cM M in place
// (cK == 0: K is not read) and / or y_row = M x_col from the compact form.
hipError_t mass_plan_build(DeviceMesh& m, int64_t& bytes, hipStream_t stream);
hipError_t launch_mass(const DeviceMesh& m, double density, const double* d_ele_density, double* d_M,
    bool overwrite, double* d_m_node, double* d_lumped, hipStream_t stream);
hipError_t launch_effective_tangent(const DeviceMesh& m, double cK, double cM, const double* d_m_node,
    double* d_K, const double* d_x_col, double* d_y_row, hipStream_t stream);
// Stress output (fcg_stress.hip).  stress_tables_build: the stiffness rule's dN | w table, the
// Gauss-point-to-node matrix X^-1 and the failing-element words, once per context (drains the
// stream); stress_slots_build: FCG_PATH_GATHER's inverse of ele_orig for the material table.
// launch_gp_stress: one lane per (column element, Gauss point), column-element order;
// launch_gp_to_nodes: one wavefront per column node with an owned row over the mass plan's lists.
hipError_t stress_tables_build(DeviceMesh& m, int64_t& bytes, hipStream_t stream);
hipError_t stress_slots_build(DeviceMesh& m, int64_t& bytes, hipStream_t stream);
hipError_t launch_gp_stress(const DeviceMesh& m, bool cauchy, bool ea, const double* d_u_col,
    double* d_stress, double* d_strain, double* d_energy, hipStream_t stream);
hipError_t launch_gp_to_nodes(const DeviceMesh& m, const double* d_gp, double* d_node,
    hipStream_t stream);

}  // namespace fcg

struct fcg_ctx {
  int device = 0;
  hipStream_t stream = nullptr;
  fcg::DeviceMesh mesh;
  fcg::Timing timing;
  std::string last_error;
  int64_t device_bytes = 0;
  // device buffers of the host-pointer entry points
  double* h_u = nullptr;
  double* h_f = nullptr;
  double* h_k = nullptr;
  fcg::HostStaging staging;
  // deferred error check (fcg_set_async)
  bool async = false;
  bool pending = false;
  hipStream_t pending_stream = nullptr;
  double create_phase_s[8] = {0, 0, 0, 0, 0, 0, 0, 0};  // fcg_get_create_phases
};

// fcg_dfcg_solve's AMG preconditioner (fcg_amg_api.hip; not part of the C ABI): numeric setup
// and one application, with the coarse levels coupled across the ranks of the transport when the
// handle is rank-local (fcg_amgs::Coupled), else the handle's own V-cycle
extern "C" {
int fcg_amg_precond_setup(fcg_amg* h, const double* d_K, const fcg_transport* tr, void* stream);
int fcg_amg_precond_apply(fcg_amg* h, const double* d_K, const fcg_transport* tr, const double* d_r,
    double* d_z, void* stream);
}
