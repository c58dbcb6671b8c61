/*
 * fourc_gpu.h -- C ABI of the MI355X-native solid element evaluation + global assembly path.
 *
 * Drop-in boundary for 4C's
 *   Core::FE::Discretization::evaluate(params, systemmatrix1, systemmatrix2,
 *                                      systemvector1, systemvector2, systemvector3)
 *     (src/core/fem/src/discretization/4C_fem_discretization_evaluate.cpp:31-61,65-103)
 * for the actions struct_calc_nlnstiff / struct_calc_internalforce
 *     (src/core/legacy_enum_definitions/4C_legacy_enum_definitions_element_actions.hpp:19-75)
 * of SOLID hex8 / hex27 elements with DisplacementBased(LinearKinematics)Formulation and
 * Mat::StVenantKirchhoff (src/solid_3D_ele/4C_solid_3D_ele_evaluate.cpp:57-117,
 * src/solid_3D_ele/4C_solid_3D_ele_calc.cpp:110-240, src/mat/4C_mat_stvenantkirchhoff.cpp:169-177).
 *
 * The element loop, the Gauss-point loop and SparseMatrix::assemble / LinAlg::assemble(Vector)
 * (src/core/linalg/src/sparse/4C_linalg_sparsematrix.cpp:426-576,
 *  src/core/linalg/src/sparse/4C_linalg_utils_sparse_algebra_assemble.cpp:72-92) run as HIP
 * kernels on gfx950.  Plain pointers and sizes only; no torch/HIP types in the signatures.
 * See INTEGRATION.md for the 4C-side binding.
 */
#ifndef FOURC_GPU_H
#define FOURC_GPU_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define FCG_ABI_VERSION 2  /* 2: fcg_transport gained exchange_fn */

/* Cell types (Core::FE::CellType::hex8 / hex27) */
enum fcg_celltype { FCG_HEX8 = 0, FCG_HEX27 = 1 };
/* Kinematics (Inpar::Solid::KinemType::linear / nonlinearTotLag) */
enum fcg_kinem { FCG_LINEAR = 0, FCG_TOTLAG = 1 };
/* Actions (Core::Elements::ActionType struct_calc_nlnstiff / struct_calc_internalforce) */
enum fcg_action { FCG_CALC_NLNSTIFF = 0, FCG_CALC_INTERNALFORCE = 1 };
/* Assembly mode: ACCUMULATE is the reference's `+=` into caller-zeroed storage
 * (SparseMatrix::assemble); OVERWRITE fuses SparseMatrix::zero() + assemble
 * (4C_structure_new_model_evaluator_structure.cpp:143-151 followed by evaluate): every owned
 * row is written exactly once, untouched entries become 0. */
enum fcg_mode { FCG_ACCUMULATE = 0, FCG_OVERWRITE = 1 };

/* Return codes.  The host shim turns non-zero codes into exceptions, like FOUR_C_THROW. */
enum fcg_status {
  FCG_OK = 0,
  FCG_ERR_NODAL_DETJ = 1,   /* det J <= 0 at an element node (4C_solid_3D_ele_calc_lib.hpp:475-496) */
  FCG_ERR_SINGULAR = 2,     /* det == 0 in invert3x3 (4C_linalg_fixedsizematrix.hpp:1394) */
  FCG_ERR_ARG = 3,          /* invalid argument / unsupported layout */
  FCG_ERR_DEVICE = 4        /* HIP / RCCL failure */
};

/*
 * Everything the element loop needs from a 4C discretization on ONE rank, in the rank's local
 * numbering.  All arrays are host memory and are copied; nothing is retained after fcg_create.
 *   - column elements (owned + ghost, 4C_fem_discretization_evaluate.cpp:83) with their local
 *     column-node ids in 4C node order;
 *   - column nodes with reference coordinates, the column-map LID of their first DOF
 *     (Map::LID of DofSet::dof(node, 0); DOFs of a node are consecutive LIDs) and, if the node is
 *     owned (lmowner == myrank), the row-map LID of its first DOF, else -1;
 *   - the CSR graph of the Epetra_CrsMatrix after FillComplete (ExtractCrsDataPointers): int64
 *     row pointers over the owned DOF rows and int32 column LIDs sorted within each row.
 */
typedef struct fcg_desc {
  int32_t abi_version;    /* FCG_ABI_VERSION */
  int32_t celltype;       /* fcg_celltype */
  int32_t kinematics;     /* fcg_kinem */
  int32_t device;         /* HIP device ordinal */
  double youngs;          /* MAT_Struct_StVenantKirchhoff YOUNG (> 0) */
  double poisson;         /* NUE, in [-1, 0.5) */
  int64_t n_ele;          /* column elements */
  int64_t n_node;         /* column nodes */
  int64_t n_rows;         /* owned DOF rows (dof row map size) */
  int64_t n_cols;         /* dof column map size (length of u_col) */
  const int32_t* ele_nodes;    /* [n_ele][nodes per element] column-node ids */
  const int32_t* ele_gid;      /* [n_ele] element GIDs (error reporting); may be NULL */
  const double* node_x;        /* [n_node][3] reference coordinates */
  const int32_t* node_dof_col; /* [n_node] column LID of the node's first DOF */
  const int32_t* node_dof_row; /* [n_node] row LID of the node's first DOF, -1 if not owned */
  const int32_t* node_dof_kcol;/* [n_node] LID of the node's first DOF in the MATRIX column map
                                  (Epetra_CrsMatrix::ColMap after FillComplete); NULL = same as
                                  node_dof_col */
  const int64_t* rowptr;       /* [n_rows + 1]; rowptr = col_lid = NULL: fcg_create builds the graph
                                  on the device (fcg_graph_build_device: rows = owned DOFs, columns
                                  = DOFs of the nodes sharing an element, sorted) and
                                  fcg_get_graph returns it -- 4C's first assembly through the
                                  unfilled path + FillComplete, 4C_linalg_sparsematrix.cpp:578-611,
                                  843-865.  Needs n_rows = 3 x owned nodes. */
  const int32_t* col_lid;      /* [rowptr[n_rows]] */
  /* Optional structured-lattice hint (GridGenerator meshes): [n_ele][3] element lattice
   * position (ex, ey, ez) = (gid % nx, gid / nx % ny, gid / (nx ny)), 4C_io_gridgenerator.cpp:336-338.
   * fcg_create verifies it against the connectivity and then uses the fused z-sweep kernel
   * (hex8) or the colour-ordered direct assembly (hex27) -- no scratch round trip either way.
   * NULL = general (unstructured) path. */
  const int32_t* ele_ijk;
  int32_t path;                /* fcg_path: FCG_PATH_AUTO / _GENERAL / _STRUCTURED / _COLORED / _GATHER */
  int32_t material;            /* fcg_material (0 = StVenantKirchhoff) */
} fcg_desc;

/* Materials.  FCG_MAT_STVK: MAT_Struct_StVenantKirchhoff YOUNG NUE (4C_mat_stvenantkirchhoff.cpp).
 * FCG_MAT_ELASTHYPER_COUPNEOHOOKE: MAT_ElastHyper with one ELAST_CoupNeoHooke summand, youngs /
 * poisson = the summand's YOUNG / NUE (4C_mat_elasthyper_service.cpp:19-215,
 * 4C_mat_elast_coupneohooke.cpp); FCG_TOTLAG only.  hex8: FCG_PATH_GENERAL (what FCG_PATH_AUTO
 * takes) or, on request, FCG_PATH_GATHER; hex27: FCG_PATH_GENERAL or the colour-ordered assembly.
 * The structured sweep implements StVenantKirchhoff only. */
enum fcg_material { FCG_MAT_STVK = 0, FCG_MAT_ELASTHYPER_COUPNEOHOOKE = 1 };

/* Evaluation paths.  AUTO picks the hex8 row-block sweep (FCG_PATH_STRUCTURED) when the lattice
 * hint verifies -- or, without a hint, when fcg_create finds the lattice in the connectivity
 * (elements stacked like a GridGenerator box, each element's local numbering any proper rotation
 * of 4C's -- a mirrored element frame is no lattice; FCG_DETECT_LATTICE=0
 * in the environment turns the search off); other hex8 StVK meshes take FCG_PATH_GATHER (one wavefront per owned row node
 * recomputes the node's elements and writes its 3 CSR rows once: no scratch, no atomics, any
 * conforming mesh with <= 27 neighbour nodes per node); everything else GENERAL (element kernel +
 * incidence scratch + row assembly).  GATHER requests the node-row gather explicitly: hex8 only,
 * StVenantKirchhoff (both kinematics) or ElastHyper/CoupNeoHooke -- AUTO keeps hex8 CoupNeoHooke on
 * GENERAL, so that material reaches the gather (no incidence scratch, each CSR row written once,
 * bitwise reproducible, ghosted partitions) only by this request.  STRUCTURED requests the lattice path and fails fcg_create with
 * FCG_ERR_ARG when the hint does not verify: for hex8 the fused row-block sweep, for hex27 the
 * colour-ordered direct assembly (reported as FCG_PATH_COLORED: for StVK four launches of
 * pencils -- runs of elements along x walked by one workgroup each -- in (y, z)-parity colours,
 * otherwise eight launches, one per element-parity colour; each element adds its blocks straight
 * into the CSR rows, the first holder of a matrix entry in that order writes it -- no scratch
 * records, no atomics, fixed order).
 * COLORED requests the latter explicitly (hex27 only). */
enum fcg_path { FCG_PATH_AUTO = 0, FCG_PATH_GENERAL = 1, FCG_PATH_STRUCTURED = 2, FCG_PATH_COLORED = 3,
  FCG_PATH_GATHER = 4 };

typedef struct fcg_ctx fcg_ctx;

/* Builds the device-resident mirror of the element set and the assembly plan
 * (the "FillComplete" of this path).  Returns FCG_OK and *out, or an error code. */
int fcg_create(const fcg_desc* desc, fcg_ctx** out);
int fcg_destroy(fcg_ctx* ctx);
/* Text of the last error on this context (or of the last failed fcg_create when ctx == NULL). */
const char* fcg_last_error(const fcg_ctx* ctx);

/* Per-element material parameters (a discretization with several MAT ids of one kind, as
 * Solid::evaluate asks each element's So3Material): element e (column-element order of
 * desc->ele_nodes) takes youngs[ele_mat[e]], poisson[ele_mat[e]] of the context's fcg_material.
 * Host arrays, copied.  n_mat = 0 (arrays NULL) returns to the uniform material of fcg_create.
 * Checks as fcg_create's (youngs > 0, poisson in [-1, 0.5), 0 <= ele_mat[e] < n_mat); a violation
 * returns FCG_ERR_ARG, fcg_last_error names the offending entry and the context stays as it was.
 * The constants are formed per material with fcg_create's host arithmetic and stored per element on
 * the device (32 bytes per element, counted in fcg_info.device_bytes), so a table whose entries
 * all equal the context's own material reproduces the uniform results bit for bit.
 * Honoured by the FCG_PATH_GATHER (hex8, both kinematics, both materials) and FCG_PATH_GENERAL
 * (hex8 and hex27, both kinematics, both materials) kernels and by fcg_tangent_apply / fcg_tangent_diag.  A context on FCG_PATH_STRUCTURED
 * or FCG_PATH_COLORED refuses a table with FCG_ERR_ARG (create it with FCG_PATH_GATHER /
 * FCG_PATH_GENERAL), and fcg_tsi_evaluate_fused refuses a structural context that carries one.
 * The call drains the context's stream before it swaps the tables; it must not run concurrently
 * with evaluates of the context on other streams. */
int fcg_set_element_materials(fcg_ctx* ctx, int32_t n_mat, const double* youngs,
    const double* poisson, const int32_t* ele_mat);

/*
 * Discretization::evaluate on host buffers (blocking, reference semantics):
 *   u_col    [n_cols]   displacement column vector (Discretization::set_state("displacement"))
 *   fint_row [n_rows]   systemvector1, += on owned rows
 *   K_vals   [nnz]      systemmatrix1 values in the CSR order of desc->col_lid, += (may be NULL
 *                       for FCG_CALC_INTERNALFORCE)
 *   bad_ele_gid         on FCG_ERR_NODAL_DETJ / FCG_ERR_SINGULAR: GID of the failing element
 */
int fcg_evaluate(fcg_ctx* ctx, int action, const double* u_col, double* fint_row, double* K_vals,
    int32_t* bad_ele_gid);

/*
 * The same on device-resident buffers (HBM) for a GPU-resident Newton loop.
 *   mode    fcg_mode (ACCUMULATE = +=, OVERWRITE = zero + assemble fused)
 *   stream  hipStream_t to run on (NULL = the context's own stream, a blocking stream: ordered
 *           with the null stream, so work the caller queued there -- e.g. torch's default
 *           stream filling d_u_col -- completes first); the call returns after the stream has
 *           drained (matching the synchronous Newton loop of the reference).
 */
int fcg_evaluate_device(fcg_ctx* ctx, int action, int mode, const double* d_u_col,
    double* d_fint_row, double* d_K_vals, void* stream, int32_t* bad_ele_gid);

/* Device allocations owned by the caller (convenience for hosts without a HIP toolchain). */
int fcg_device_alloc(int device, int64_t bytes, void** d_ptr);
int fcg_device_free(void* d_ptr);
int fcg_memcpy_h2d(void* d_dst, const void* h_src, int64_t bytes);
int fcg_memcpy_d2h(void* h_dst, const void* d_src, int64_t bytes);
int fcg_memset_device(void* d_dst, int value, int64_t bytes);

/* Per-kernel timing of the last evaluate on the launch stream, measured with hipEvents
 * (enable before the call).  GENERAL path: element kernel, assemble kernel.  STRUCTURED path:
 * the fused kernel in ms_element, 0 in ms_assemble.  hex27 slab schedule (fcg_info.h27_slabs > 1):
 * the slabs' element and row launches interleave, so ms_element holds both and ms_assemble is 0.
 * Returns the number of kernels timed. */
int fcg_set_timing(fcg_ctx* ctx, int enable);
int fcg_get_timing(const fcg_ctx* ctx, double* ms_element, double* ms_assemble);

/* Sizes of what fcg_create built (for roofline bookkeeping). */
typedef struct fcg_info {
  int64_t n_ele, n_node, n_rows, n_cols, nnz;
  int64_t n_incidences;     /* (element, owned local node) pairs */
  int64_t scratch_bytes;    /* device scratch for element block-rows */
  int64_t device_bytes;     /* total device memory held by the context */
  int32_t path;             /* fcg_path actually used (GENERAL, STRUCTURED or COLORED) */
  /* hex27 incidence records (GENERAL path): 1 = one record per incidence (the full scratch, the
   * fast mode), > 1 = the slab schedule with that many slabs (a ring of records, DESIGN §7e: less
   * memory, about +25 % per evaluate), 0 = not the hex27 record path.  By default the slab
   * schedule is taken only when the full scratch plus the K values would not fit the device's free
   * memory at fcg_create; FCG_H27_SLAB = elements per slab forces it (0 = one slab). */
  int32_t h27_slabs;
} fcg_info;
int fcg_get_info(const fcg_ctx* ctx, fcg_info* info);

/* The context's CSR graph (host copies): rowptr [n_rows + 1] when non-NULL, col_lid [nnz] when
 * non-NULL and col_capacity >= nnz; *nnz always.  For a context created with rowptr = col_lid =
 * NULL this is the graph fcg_create built on the device -- what a 4C host then hands to its
 * Epetra_CrsGraph / SparseMatrix (the FillComplete'd graph of the first assembly). */
int fcg_get_graph(const fcg_ctx* ctx, int64_t* rowptr, int32_t* col_lid, int64_t col_capacity,
    int64_t* nnz);

/* On-box peaks for the roofline (SURVEY §8d asks to re-measure the spec figures): STREAM triad
 * bandwidth over 3 x 1 GiB HBM arrays (GB/s), FP64 VALU FMA and FP64 MFMA (v_mfma_f64_16x16x4_f64)
 * throughput (TFLOP/s), each on every CU of `device`.  Outputs may be NULL. */
int fcg_measure_peaks(int device, double* hbm_triad_gbs, double* fp64_valu_tflops,
    double* fp64_mfma_tflops);

/* The HBM patterns beside the triad (GB/s, best over in-flight depths, grid sizes and store
 * policies): a 16-byte-per-lane copy of 2 GiB (read + write, the pattern of the guide's measured
 * 6.29 TB/s) and a write-only fill of 2 GiB (the pattern of the assembly's K stores).  Outputs may
 * be NULL. */
int fcg_measure_hbm(int device, double* copy_gbs, double* write_gbs);

/* Diagnostics only: with FCG_STAMPS=1 in the environment at fcg_create, the fused kernel sums
 * per-phase cycle counts (s_memtime, thread 0 of every workgroup) into 16 counters: commit,
 * Gauss-point stage, node-row stage, accumulation, flush, workgroups (index 5); the hex27 element
 * kernel's layout is in fcg_hex27.hip.  Returns the number of counters (0 when off).
 * out[15] is no counter and is filled whether the counters are on or off: which kernels the
 * structured sweep of this context launches -- FCG_SWEEP_KERNEL_UNCHECKED when the geometry pass
 * of fcg_create found no rejected element and no negative det J w (the reference coordinates do
 * not change during a context's life, so the evaluates need not look again),
 * FCG_SWEEP_KERNEL_CHECKED when it found one or FCG_SWEEP_CHECKED=1 was set at fcg_create,
 * FCG_SWEEP_KERNEL_NA on every other path.
 * out[13], out[14] are no counters either and are always filled: the (tile, layer) pairs of the
 * structured sweep that take the regular-tile path (closed-form row bookkeeping for tiles whose
 * rows fcg_create found to be 81 entries long with one neighbour pattern and rows and bases in
 * arithmetic progression; the unchecked linear kernels only, none with FCG_SWEEP_REGULAR=0 at
 * fcg_create), and all pairs the sweep's workgroups run; both 0 on every other path.
 * out[12], always filled as well: how the structured sweep's tangent kernels write a row's blocks
 * -- FCG_SWEEP_ROWS_DIRECT: the blocks with the plane below in the layer that finishes them, the
 * others one layer later; FCG_SWEEP_ROWS_DEFERRED: all of a row within one layer (the lower-plane
 * blocks wait in LDS; rows not in lattice order, or FCG_SWEEP_DEFER=1 at fcg_create);
 * FCG_SWEEP_ROWS_NA on every other path. */
#define FCG_SWEEP_KERNEL_NA 0
#define FCG_SWEEP_KERNEL_CHECKED 1
#define FCG_SWEEP_KERNEL_UNCHECKED 2
#define FCG_SWEEP_ROWS_NA 0
#define FCG_SWEEP_ROWS_DIRECT 1
#define FCG_SWEEP_ROWS_DEFERRED 2
int fcg_get_diagnostics(const fcg_ctx* ctx, uint64_t* out, int n);

/* Wall time (seconds) of fcg_create's phases, the setup counterpart of 4C's FillComplete and
 * DofSet numbering (4C_linalg_sparsematrix.cpp:843-865, 4C_fem_dofset.cpp:128-366): out[i] for
 * i < n of 0 checks, 1 graph on the device (rowptr = col_lid = NULL), 2 node rows and their CSR
 * pattern, 3 lattice / colour plans, 4 incidences, 5 incidence column positions, 6 device
 * buffers and path plans (uploads, Morton orders, gather records, hex27 ring), 7 total.
 * Returns the number of phases (8). */
int fcg_get_create_phases(const fcg_ctx* ctx, double* out, int n);

/* ------------------------------------------------------------------------------------------
 * Around the assembly: what one Newton step of Solid statics needs on the device
 * (NOX full Newton, 4C_solver_nonlin_nox_linearsystem.cpp:275-353, with the structure's
 * Dirichlet handling, 4C_structure_new_dbc.cpp:221-295).  All vectors are device-resident
 * (owned DOF rows unless stated); `stream` as for fcg_evaluate_device; the calls return after
 * the stream has drained.
 * ---------------------------------------------------------------------------------------- */
/* y_row = K x_col (Epetra_CrsMatrix::Multiply on the owned rows).  Asynchronous: queued on
 * `stream` (NULL: the context's stream), which orders it with the caller's later work.  Right on
 * every graph fcg_create accepts: node rows made of DOF triples only go triple by triple, a graph
 * with other columns as well (a caller's extra couplings) goes row by row.  A context without
 * rows is a no-op (FCG_OK, the buffers may be NULL), here and in the calls below. */
int fcg_spmv(fcg_ctx* ctx, const double* d_K_vals, const double* d_x_col, double* d_y_row,
    void* stream);
/* Dirichlet rows (row LIDs d_rows[n_dbc], device array): freact[row] = -rhs[row] (if freact is not
 * NULL, Solid::Dbc::extract_freact: with rhs = F = f_int - f_ext the reaction is f_ext - f_int), rhs[row] = 0 (apply_dirichlet_to_system with zeros),
 * K row -> unit row (SparseMatrix::apply_dirichlet, diagonalblock = true,
 * 4C_linalg_sparsematrix.cpp:978-1097).  K or rhs may be NULL.  The rows of d_rows must be
 * distinct: a row listed twice is handled by two wavefronts in no fixed order, and the second may
 * read the rhs the first already zeroed (freact = -0.0).  A row LID outside [0, n_rows) or a row
 * without a diagonal entry gives FCG_ERR_ARG; the other rows listed are still applied. */
int fcg_dirichlet_apply(fcg_ctx* ctx, int64_t n_dbc, const int32_t* d_rows, double* d_K_vals,
    double* d_rhs_row, double* d_freact_row, void* stream);
/* Inertia (DYNAMICTYPE GenAlpha; 4c_amd/dynamics.py).  The consistent mass block between nodes a
 * and b of displacement-based solid elements is m_ab I_3,
 *   m_ab = sum_e sum_g rho_e w_g det J_g N_a(xi_g) N_b(xi_g)
 * on the element's stiffness Gauss rule (8 / 27 points; the 27-point rule's constants in full double
 * precision, so that the total mass is rho V to rounding), J from the reference coordinates
 * (struct_calc_nlnstiffmass, 4C_solid_3D_ele_calc.cpp; independent of kinematics and material).
 * Every context fcg_create accepts, on every path; as in evaluate only owned rows are written and
 * all column elements (ghosts included) contribute; columns are LIDs of the matrix column map.
 * density > 0, or ele_density[e] > 0 per column element (host [n_ele], copied; density is then
 * ignored): a violation returns FCG_ERR_ARG and fcg_last_error names the entry.  A Gauss point with
 * det J <= 0 returns FCG_ERR_NODAL_DETJ through the solver flag word, as fcg_tangent_diag's
 * errors (never evaluate's sticky flags), fcg_last_error names the element GID.  Each entry is
 * summed over its elements in ascending column-element index, no atomics on doubles: two calls
 * give the same bits.  A per-context plan (the nodes' element lists, counted in device_bytes) is
 * built on the first mass call.  Both mass calls return after the stream has drained.
 * fcg_mass_assemble: the CSR form on the context's graph (4C's systemmatrix2).  OVERWRITE writes
 * every owned entry (exact 0 off the block diagonals and in columns that are no element node's),
 * ACCUMULATE adds the block diagonals onto the caller's values. */
int fcg_mass_assemble(fcg_ctx* ctx, double density, const double* ele_density /* host [n_ele] or NULL */,
    int mode /* fcg_mode */, double* d_M_vals /* [nnz] */, void* stream);
/* The compact node form and / or the row-sum lumped mass (4C's LUMPMASS); needs a context whose
 * rows are all owned nodes' DOF triples (else FCG_ERR_ARG).  For the context's k-th row node (the
 * block order of fcg_block_jacobi_setup) with first row row0, the entry of its t-th column triple
 * -- columns col_lid[rowptr[row0] + 3 t .. + 2] -- is m_node[rowptr[row0] / 9 + t];
 * m_lumped_row[r] = sum_b m_ab of r's node, the same value on the node's three rows. */
int fcg_mass_nodal(fcg_ctx* ctx, double density, const double* ele_density,
    double* d_m_node /* [nnz/9] or NULL */, double* d_m_lumped_row /* [n_rows] or NULL */, void* stream);
/* K <- cK K + cM M in place and y_row = M x_col, in one pass over the node rows (the context
 * requirement of fcg_mass_nodal): every stored entry becomes cK K[j], the three diagonal entries of
 * each 3 x 3 block get fma(cM, m_ab, cK K[j]).  cK == 0: K is not read, the result is exactly
 * cM M whatever the buffer held.  With d_x_col and d_y_row, y_row = M x_col in the same pass (sums
 * in a fixed lane order: deterministic); d_K_vals NULL: only y.  All three NULL: FCG_ERR_ARG.
 * Asynchronous on `stream` like fcg_spmv. */
int fcg_effective_tangent(fcg_ctx* ctx, double cK, double cM, const double* d_m_node,
    double* d_K_vals /* may be NULL */, const double* d_x_col, double* d_y_row /* both may be NULL */,
    void* stream);
/* Output (struct_calc_stress / struct_calc_energy: SolidEleCalc::calculate_stress and
 * calculate_internal_energy, 4C_solid_3D_ele_calc.cpp): stresses, strains and the strain energy of
 * every column element at the displacement u_col, in one pass.  Elements in the column-element
 * order of desc->ele_nodes on every path (ghosts included: the host picks the elements it owns);
 * Gauss points of the element's stiffness rule (8 / 27, the reference's 13-digit hex27 constants)
 * in the rule's order; components in 4C's stress Voigt order xx yy zz xy yz xz for stresses and
 * strains alike, strains in stress-like form (tensor components: eps_xy, not 2 eps_xy).
 *   FCG_STRAIN_GL  E = 1/2 (F^T F - I); FCG_LINEAR: the symmetric displacement gradient, F := I
 *   FCG_STRAIN_EA  e = F^-T E F^-1
 *   FCG_STRESS_PK2 the material's S(E);  FCG_STRESS_CAUCHY  sigma = 1 / det F  F S F^T
 *   (FCG_LINEAR: EA equals GL and Cauchy equals PK2)
 *   d_energy[e] = sum_g w_g det J_g psi(E_g) in Gauss-point order; StVK psi = 1/2 E^T C E
 *   (Mat::StVenantKirchhoff::strain_energy), CoupNeoHooke psi = c (I1 - 3) + c / beta (J^(-2 beta) - 1)
 * Material: the context's, or the per-element table of fcg_set_element_materials on the paths that
 * carry one.  d_stress goes with stress_type and d_strain with strain_type: a buffer whose type is
 * NONE, a type without its buffer, or all three outputs NULL return FCG_ERR_ARG.  d_u_col may be
 * NULL for FCG_LINEAR (u = 0).  det J <= 0 at a Gauss point returns FCG_ERR_NODAL_DETJ; det F == 0
 * returns FCG_ERR_SINGULAR where F^-1 or 1 / det F is needed (EA or Cauchy under FCG_TOTLAG); both
 * report the lowest failing column element through bad_ele_gid and fcg_last_error, through the
 * solver flag word (never evaluate's sticky flags).  The call returns after the stream has drained.
 * No atomics on doubles: two calls give the same bits. */
enum fcg_stress_type { FCG_STRESS_NONE = 0, FCG_STRESS_PK2 = 1, FCG_STRESS_CAUCHY = 2 };
enum fcg_strain_type { FCG_STRAIN_NONE = 0, FCG_STRAIN_GL = 1, FCG_STRAIN_EA = 2 };
int fcg_gp_stress(fcg_ctx* ctx, int stress_type, int strain_type, const double* d_u_col,
    double* d_stress /* [n_ele][ngp][6] or NULL */, double* d_strain /* [n_ele][ngp][6] or NULL */,
    double* d_energy /* [n_ele] or NULL */, void* stream, int32_t* bad_ele_gid);
/* The nodal form of Gauss-point data (GAUSS_POINT_DATA_OUTPUT_TYPE nodes:
 * Core::FE::extrapolate_gauss_points_to_nodes, then the division by the nodal element count): an
 * element's nodal values are X^-1 gp with X[g][a] = N_a(xi_g) on the stiffness rule (square for
 * both cell types; inverted once on the host with partial pivoting and kept on the context); every
 * column node with an owned row gets the mean over all its column elements, summed in ascending
 * element index (the mass plan's lists, built here if no mass call has).  d_node is indexed by
 * column node; rows of nodes without an owned row are not touched.  Asynchronous on `stream`
 * like fcg_spmv. */
int fcg_gp_to_nodes(fcg_ctx* ctx, const double* d_gp /* [n_ele][ngp][6] */,
    double* d_node /* [n_node][6] */, void* stream);
/* Explicit dynamics (DYNAMICTYPE CentrDiff, Solid::EXPLICIT::CentrDiff; 4c_amd/dynamics.py).  The
 * vector update of one central-difference step with the lumped mass of fcg_mass_nodal, one launch
 * over the owned DOF rows.  On entry d = d_{n+1}, vhalf = v_{n+1/2}, fint = f_int(d_{n+1}),
 * fext = f_ext(t_{n+1}); per free row
 *   a      = (fext - fint) / m - damp_m vhalf    a_{n+1}; mass-proportional damping C = damp_m M,
 *                                                taken at the half-step velocity: the step stays explicit
 *   v      = vhalf + dt_prev / 2 a               v_{n+1}   -> d_v_row, d_a_row
 *   vhalf' = v + dt_next / 2 a                   v_{n+3/2} -> d_vhalf_row
 *   d'     = d + dt_next vhalf'                  d_{n+2}   -> d_d_row
 * which is 4C's sequence half kick, drift, evaluate, a = M^-1 (f_ext - f_int - f_visc), half kick
 * written as one pass per evaluate.  Rows with d_fixed_row[r] != 0 (homogeneous-in-time Dirichlet
 * rows) get a = v = vhalf' = 0 and keep d.  dt_prev = 0 with vhalf = v_0 starts a run: it forms
 * a_0 and takes the first half kick and drift.  dt_next = 0 finishes a step without advancing: d
 * stays, vhalf' = v.  A variable step is different dt_prev / dt_next.  m > 0 on the free rows is
 * the caller's guarantee.  d_d_row and d_vhalf_row are updated in place; no output may alias an
 * input otherwise.  *d_ekin = 1/2 sum m v^2 over the owned rows (a multi-rank caller adds the
 * ranks'), summed in a fixed order: per-workgroup partials in a per-context buffer (counted in
 * device_bytes, allocated on first use; calls on one context that ask for it must be
 * stream-ordered), then one small second launch -- no atomics on doubles, two calls give the same
 * bits.  Negative or non-finite dt_prev, dt_next or damp_m, or a NULL required pointer, return
 * FCG_ERR_ARG; a context without rows returns FCG_OK before looking at its pointers.
 * Asynchronous on `stream` like fcg_spmv. */
int fcg_centrdiff_step(fcg_ctx* ctx, double dt_prev, double dt_next, double damp_m,
    const double* d_fext_row, const double* d_fint_row, const double* d_m_lumped_row,
    const uint8_t* d_fixed_row /* [n_rows], != 0: Dirichlet row; may be NULL */,
    double* d_d_row, double* d_vhalf_row, double* d_v_row /* may be NULL */,
    double* d_a_row /* may be NULL */, double* d_ekin /* 1 double, may be NULL */, void* stream);
/* The stable step of the central-difference scheme is 2 / omega_max, omega_max^2 the largest
 * eigenvalue of M_l^-1 K.  lambda_bound = max over the free rows i of (sum_j |K_ij|) / m_i is
 * Gershgorin's bound on that spectrum, so dt_crit = 2 / sqrt(lambda_bound) is never above the
 * true limit.  Rows with d_fixed_row[r] != 0 are skipped; their columns stay in the other rows'
 * sums, which only enlarges the bound.  Every graph fcg_create accepts, row by row over rowptr;
 * ghost columns count, so the bound is row-local: a multi-rank caller takes the maximum of
 * lambda_bound (the minimum of dt_crit) over the ranks with its own all-reduce.  The maximum is
 * taken in two stages without atomics on doubles.  Blocking: the call drains the stream to return
 * the two numbers (either pointer may be NULL).  A free row with m <= 0, a non-finite mass or a
 * non-finite row sum returns FCG_ERR_ARG through the solver flag word (never evaluate's sticky
 * flags) and fcg_last_error names the lowest such row.  No free row (and a context without
 * rows): lambda_bound = 0, dt_crit = +inf. */
int fcg_stable_dt(fcg_ctx* ctx, const double* d_K_vals /* [nnz] */, const double* d_m_lumped_row,
    const uint8_t* d_fixed_row /* may be NULL */, double* lambda_bound, double* dt_crit, void* stream);
/* K x = b by CG preconditioned with the inverse 3x3 nodal diagonal blocks (block Jacobi) from x = 0 until |r| <= rtol |b| or max_iter iterations;
 * single-rank systems only (matrix column map = row map), else FCG_ERR_ARG.  Deterministic. */
/* y_row = K x_col with the matrix values stored in FP32 (vectors and sums FP64): the multigrid
 * smoother's reduced-precision copy of K (4c_amd/multigrid.py, mixed=True), half the bytes of
 * fcg_spmv.  Asynchronous on `stream` like fcg_spmv. */
int fcg_spmv_f32(fcg_ctx* ctx, const float* d_K32, const double* d_x_col, double* d_y_row,
    void* stream);
/* y_row = K(u) x_col without a matrix: the tangent the context's evaluate assembles at the
 * displacement u_col (before Dirichlet rows), applied element by element from X, u and x
 * (B^T C B + K_geo per Gauss point, 4C_solid_3D_ele_calc_lib.hpp:872-927) and summed per owned
 * row node in incidence order -- deterministic, equal to fcg_spmv on that K to rounding.  hex27
 * St.Venant-Kirchhoff contexts only (else FCG_ERR_ARG); u_col may be NULL for linear kinematics.
 * The multigrid smoother's level-0 operator (4c_amd/multigrid.py, matrix_free=True): 81 + 162
 * doubles of input per element instead of the 6,561 matrix entries an SpMV reads.  Uses a
 * per-context buffer (3 doubles per owned incidence, allocated on the first call): calls on one
 * context must not run concurrently.  Asynchronous on `stream` like fcg_spmv. */
int fcg_tangent_apply(fcg_ctx* ctx, const double* d_u_col, const double* d_x_col, double* d_y_row,
    void* stream);
int fcg_pcg_solve(fcg_ctx* ctx, const double* d_K_vals, const double* d_b_row, double* d_x_row,
    double rtol, int max_iter, int* iterations, double* rel_residual, void* stream);
/* Pieces of the geometric multigrid preconditioner (4c_amd/multigrid.py; the MueLu
 * preconditioner 4C hands to Belos, 4C_linear_solver_preconditioner_muelu.cpp, restated for
 * structured boxes).  d_dinv: 9 doubles per owned node (row-major inverse 3x3 nodal diagonal
 * blocks of K, FCG_ERR_SINGULAR if one is singular).  apply: z = scale D^-1 r (+ z if accumulate).
 * fcg_node_transfer: y[dst_row0[o] + d] = (accumulate ? y : 0) + sum_{j in [ptr[o], ptr[o+1])}
 * w[j] x[src_row0[j] + d] for d = 0..2 and dst_row0[o] >= 0 (all device arrays; stream may be
 * NULL: the context's stream for the ctx calls, the null stream for fcg_node_transfer).
 * Asynchronous on `stream` except fcg_block_jacobi_setup, which returns after it drained.
 * On a context without rows (a rank that owns none) fcg_block_jacobi_setup, fcg_block_jacobi_apply
 * and fcg_chebyshev_step return FCG_OK before they look at their pointers, as fcg_spmv does: the
 * rank's empty buffers may be NULL. */
int fcg_block_jacobi_setup(fcg_ctx* ctx, const double* d_K_vals, double* d_dinv, void* stream);
int fcg_block_jacobi_apply(fcg_ctx* ctx, const double* d_dinv, const double* d_r_row, double* d_z_row,
    double scale, int accumulate, void* stream);
/* The 3 x 3 nodal diagonal blocks of K(u) without a matrix: what fcg_block_jacobi_setup picks out
 * of the assembled tangent, formed element by element.  Per element, node a and Gauss point, with
 * n = grad_X N_a and v = F n (F = I for linear kinematics),
 *   K_aa = sum_g fac [ (lambda + mu) v v^T + mu |n|^2 F F^T + (n . S n) I ],  S = C E(u)
 * (B_a^T C B_a + K_geo,aa of 4C_solid_3D_ele_calc_lib.hpp:872-927 for the isotropic StVK C), summed
 * per owned row node in incidence order -- deterministic, equal to the assembled K's blocks to
 * rounding.  The n_dbc rows d_dbc_rows (device, row LIDs) are replaced by unit rows, their columns
 * stay (fcg_dirichlet_apply on K); n_dbc = 0: the blocks of K(u) before Dirichlet rows.  d_diag:
 * the blocks, d_dinv: their inverses (fcg_block_jacobi_setup's arithmetic), 9 doubles per owned
 * node, row-major, block k of the context's k-th row node as fcg_block_jacobi_setup's d_dinv;
 * either may be NULL, not both.  hex27 St.Venant-Kirchhoff contexts whose owned rows are all owned
 * nodes' DOF triples (else FCG_ERR_ARG); u_col may be NULL for linear kinematics.  With d_dinv the
 * call returns after `stream` drained, FCG_ERR_SINGULAR for a singular or non-finite block and
 * FCG_ERR_ARG for a Dirichlet row outside the row map (the solver flag word, never evaluate's
 * sticky flags); with d_diag only it is asynchronous like fcg_tangent_apply and such a row is
 * skipped.  Uses per-context buffers (6 doubles per owned incidence and a byte per row, allocated
 * on the first call, counted in device_bytes): calls on one context must not run concurrently. */
int fcg_tangent_diag(fcg_ctx* ctx, const double* d_u_col, int64_t n_dbc, const int32_t* d_dbc_rows,
    double* d_diag, double* d_dinv, void* stream);
/* One Chebyshev smoothing step with the block-Jacobi preconditioner, fused per node (the update of
 * the multigrid smoother, 4c_amd/multigrid.py CycleFCG._cheb): with r = b - y (y = A x, computed
 * by the caller) and z = D^-1 r,
 *   mode 0: d = c_r z,           x += d
 *   mode 1: d = c_d d + c_r z,   x += d
 *   mode 2: d = c_r D^-1 b,      x  = d   (first step from x = 0; y is not read)
 * -- the arithmetic of the separate r = b - y, d *= c_d, d += c_r D^-1 r, x += d passes in one
 * read of b, y, d, x and the nodal inverses. */
int fcg_chebyshev_step(fcg_ctx* ctx, const double* d_dinv, const double* d_b_row, const double* d_y_row,
    double* d_d_row, double* d_x_row, double c_d, double c_r, int mode, void* stream);
int fcg_node_transfer(int device, int64_t n_out, const int64_t* d_ptr, const int32_t* d_src_row0,
    const double* d_w, const int32_t* d_dst_row0, const double* d_x, double* d_y, int accumulate,
    void* stream);
/* y = K x of a hex8 GridGenerator box whose elements are all the same parallelepiped (the
 * multigrid's rediscretised coarse levels, 4c_amd/multigrid.py): nx x ny x nz nodes (x fastest,
 * each >= 2), d_row_of[node] = row LID of its first DOF (-1: no row), d_clamped[node] != 0 makes
 * the node's rows unit rows (fcg_dirichlet_apply's), d_S[27 classes][27 offsets][3 x 3] the
 * stencil blocks summed from the element matrix (class = low face / interior / high face per axis,
 * offset (dx, dy, dz) in {-1, 0, 1}^3, both x fastest).  Equal to fcg_spmv on that box's assembled
 * K to rounding, without reading K.  Asynchronous on `stream`. */
int fcg_box_stencil_apply(int device, int nx, int ny, int nz, const int32_t* d_row_of,
    const uint8_t* d_clamped, const double* d_S, const double* d_x, double* d_y, void* stream);
/* The multigrid's transfer between a box lattice and its 2:1 coarsening (fine = 2 coarse - 1
 * points per axis: hex27 -> hex8 on the same elements, hex8 n -> n / 2) with the trilinear weights
 * implicit: mode 0 prolongation y_fine (+)= P x_coarse, mode 1 restriction y_coarse = P^T x_fine;
 * rows of nodes flagged in d_zero_out (the output level's lattice) are set to 0.  Row tables as
 * fcg_box_stencil_apply's.  The same operator as fcg_node_transfer on multigrid.transfer_tables. */
int fcg_box_transfer(int device, int mode, int fnx, int fny, int fnz, int cnx, int cny, int cnz,
    const int32_t* d_fine_row_of, const int32_t* d_coarse_row_of, const uint8_t* d_zero_out,
    const double* d_x, double* d_y, int accumulate, void* stream);

/* Smoothed-aggregation AMG for meshes without a box hierarchy (replaces the MueLu preconditioner
 * 4C builds in 4C_linear_solver_preconditioner_muelu.cpp; algorithm in fcg_amg_setup.cpp).
 * Host, graph only (block = node): fcg_amg_aggregate returns the number of aggregates (-1 on bad
 * input) and agg[i] (-1 for skipped nodes); fcg_amg_tentative factors each aggregate's stacked
 * near-null space ns[n][bs][6] into the tentative blocks p_vals[n][bs][6] and the coarse near-null
 * space ns_coarse[n_agg][6][6]; fcg_bsr_symbolic gives the block pattern of C = A B (count pass
 * with c_col = NULL, then fill pass; columns ascending); fcg_bsr_transpose_pattern the pattern of
 * A^T with perm[t] = A's block index.
 * Device (BSR: int64 block row pointers, int32 block columns, row-major blocks; asynchronous on
 * `stream` except fcg_bsr_block_jacobi_setup, which drains it to read the flag):
 * fcg_bsr_spmv y = alpha A x (+ y), blocks br x bc in {3,6}^2; fcg_bsr_spgemm C = A B on C's
 * pattern for (br, bk, bc) in {(3,3,6), (6,3,6), (6,6,6), (3,3,3)}; fcg_bsr_transpose_values
 * (3x6 and 6x6); fcg_bsr_from_node_csr copies a context's node-triple K (rows 3b..3b+2 = block
 * row b) into 3 x 3 blocks; fcg_bsr_block_jacobi_setup inverts the diagonal blocks (b = 3, 6; a
 * scalar row empty across its block row first gets a unit diagonal in d_vals) and returns
 * FCG_ERR_SINGULAR for a missing or singular block; fcg_bsr_block_jacobi_apply z = scale D^-1 r
 * (+ z); fcg_amg_smooth_prolongator P = T - omega D^-1 (A T) on P's pattern (br = 3, 6; 6
 * columns); fcg_bsr_to_dense fills a zeroed row-major dense matrix.
 * fcg_bsr_product_plan (host) lists once, per block of C = A B on C's pattern, the (A block,
 * B block) pairs whose products land there, in A's row order (count pass with pair_a = pair_b =
 * NULL fills pair_ptr[0..nnzb_c]; returns the pair count, -1 on bad input);
 * fcg_bsr_spgemm_planned forms C from such a plan -- the same products in the same order as
 * fcg_bsr_spgemm, without its per-block column searches; d_order (or NULL = storage order) is the
 * order in which the C blocks are formed (thread t forms block d_order[t]: e.g. rows grouped by
 * aggregate, so that the B rows of neighbouring rows are re-read from cache). */
int64_t fcg_amg_aggregate(int64_t n, const int64_t* ptr, const int32_t* adj, const uint8_t* skip,
    int32_t* agg);
int fcg_amg_tentative(int64_t n, int bs, const double* ns, const int32_t* agg, int64_t n_agg,
    double* p_vals, double* ns_coarse, int64_t* n_deficient);
int64_t fcg_bsr_symbolic(int64_t n_rows, const int64_t* a_ptr, const int32_t* a_col,
    const int64_t* b_ptr, const int32_t* b_col, int64_t n_cols, int64_t* c_ptr, int32_t* c_col);
int fcg_bsr_transpose_pattern(int64_t n_rows, int64_t n_cols, const int64_t* ptr,
    const int32_t* col, int64_t* t_ptr, int32_t* t_col, int64_t* perm);
int fcg_bsr_spmv(int device, int br, int bc, int64_t n_brows, const int64_t* d_ptr,
    const int32_t* d_col, const double* d_vals, const double* d_x, double* d_y, double alpha,
    int accumulate, void* stream);
int fcg_bsr_spgemm(int device, int br, int bk, int bc, int64_t n_brows, const int64_t* d_a_ptr,
    const int32_t* d_a_col, const double* d_a_vals, const int64_t* d_b_ptr, const int32_t* d_b_col,
    const double* d_b_vals, const int64_t* d_c_ptr, const int32_t* d_c_col, double* d_c_vals,
    void* stream);
int64_t fcg_bsr_product_plan(int64_t n_rows, const int64_t* a_ptr, const int32_t* a_col,
    const int64_t* b_ptr, const int32_t* b_col, const int64_t* c_ptr, const int32_t* c_col,
    int64_t n_cols, int64_t* pair_ptr, int32_t* pair_a, int32_t* pair_b);
int fcg_bsr_spgemm_planned(int device, int br, int bk, int bc, int64_t nnzb_c, const int64_t* d_pair_ptr,
    const int32_t* d_pair_a, const int32_t* d_pair_b, const double* d_a_vals, const double* d_b_vals,
    double* d_c_vals, const int64_t* d_order, void* stream);
int fcg_bsr_transpose_values(int device, int br, int bc, int64_t nnzb, const int64_t* d_perm,
    const double* d_vals, double* d_t_vals, void* stream);
int fcg_bsr_from_node_csr(int device, int64_t n_brows, const int64_t* d_rowptr,
    const int64_t* d_b_ptr, const double* d_K, double* d_b_vals, void* stream);
int fcg_bsr_block_jacobi_setup(int device, int b, int64_t n_brows, const int64_t* d_ptr,
    const int64_t* d_diag_idx, double* d_vals, double* d_dinv, int32_t* d_flag, void* stream);
int fcg_bsr_block_jacobi_apply(int device, int b, int64_t n_brows, const double* d_dinv,
    const double* d_r, double* d_z, double scale, int accumulate, void* stream);
int fcg_amg_smooth_prolongator(int device, int br, int64_t n_brows, const int64_t* d_p_ptr,
    const int32_t* d_p_col, const int32_t* d_agg, const double* d_tent, const double* d_dinv,
    const double* d_at, double omega, double* d_p_vals, void* stream);
int fcg_bsr_to_dense(int device, int b, int64_t n_brows, const int64_t* d_ptr, const int32_t* d_col,
    const double* d_vals, double* d_dense, void* stream);

/* The smoothed-aggregation AMG solve as one native object (fcg_amg_api.hip, over fcg_amg_solver.hip
 * and fcg_amg_coupled.hip): what a C++ host calls instead of its Belos CG + MueLu preconditioner on
 * a tangent the context assembled.
 * fcg_amg_create: the context's own CSR graph (host rowptr / col_lid as in fcg_desc; rows 3b..3b+2
 * = the DOFs of block row b, single rank), node_x[b][3] the reference coordinates of block row b's
 * node, the Dirichlet rows (unit rows of K); builds the hierarchy's patterns on the host.  A
 * context whose rows hold columns that are not node DOF triples is refused (FCG_ERR_ARG).
 * fcg_amg_solve: numeric setup for d_K_vals (the tangent after fcg_dirichlet_apply) and flexible
 * CG with one V-cycle per iteration from x = 0 to |r| <= rtol |b|; returns FCG_ERR_SINGULAR when
 * the V-cycle turns indefinite or the iteration diverges.  fcg_amg_level_info: DOFs, blocks and
 * the lambda_max estimate of level 0 .. fcg_amg_levels() - 1; fcg_amg_setup_ms: the last numeric
 * setup (hipEvent time). */
typedef struct fcg_amg fcg_amg;
typedef struct fcg_amg_options {
  int32_t nu;               /* Chebyshev degree of the smoother (2) */
  int32_t max_levels;       /* (10) */
  int64_t coarse_max;       /* coarsen until a level has at most this many DOFs (3000) */
  int32_t coarse_max_iter;  /* block-Jacobi CG iterations on the coarsest level, at most (500) */
  double coarse_rtol;       /* ... until |r| <= coarse_rtol |b| (1e-2) */
  double omega;             /* prolongator damping times 1 / lambda_max(D^-1 A) (4/3) */
  double ratio, boost;      /* Chebyshev eigenvalue ratio (20) and lambda_max boost (1.1) */
} fcg_amg_options;
void fcg_amg_default_options(fcg_amg_options* opt);
int fcg_amg_create(fcg_ctx* ctx, const int64_t* rowptr, const int32_t* col_lid,
    const double* node_x, int64_t n_dbc, const int32_t* dbc_rows, const fcg_amg_options* opt,
    fcg_amg** out);
int fcg_amg_solve(fcg_amg* amg, const double* d_K_vals, const double* d_b_row, double* d_x_row,
    double rtol, int max_iter, int* iterations, double* rel_residual, void* stream);
/* fcg_amg_solve = fcg_amg_setup (numeric setup for d_K_vals) + fcg_amg_iterate (the flexible CG
 * on the last setup): a constant operator -- e.g. a linear coarse level of a geometric hierarchy
 * -- is set up once and iterated many times. */
int fcg_amg_setup(fcg_amg* amg, const double* d_K_vals, void* stream);
int fcg_amg_iterate(fcg_amg* amg, const double* d_K_vals, const double* d_b_row, double* d_x_row,
    double rtol, int max_iter, int* iterations, double* rel_residual, void* stream);
int fcg_amg_levels(const fcg_amg* amg);
int fcg_amg_level_info(const fcg_amg* amg, int level, int64_t* dofs, int64_t* blocks, double* lmax);
double fcg_amg_setup_ms(const fcg_amg* amg);
/* How the last numeric setup / iterations ran: *coarse_dense = 1 when the coarsest level is
 * applied as its dense inverse (formed per tangent, at most 4096 DOFs; 0: block-Jacobi CG),
 * *graph_launches = FCG iterations replayed from the captured HIP graph since creation (opt-in:
 * FCG_AMG_GRAPH=1 in the environment; FCG_AMG_DENSE=0 keeps the CG coarse solve).  (Either
 * pointer may be NULL.) */
int fcg_amg_stats(const fcg_amg* amg, int* coarse_dense, int* graph_launches);
const char* fcg_amg_last_error(const fcg_amg* amg);
/* Host copies of what the last fcg_amg_setup left on the device (read-only: synchronises the
 * device and copies; no kernel, nothing in the handle changes).  fcg_amg_level_matrix, `which`:
 *   0  A_level in BSR (block row pointers, block columns, row-major blocks): level 0 in 3 x 3
 *      blocks, the copy of K the hierarchy was built from, in level 0's order; 6 x 6 below
 *   1  P_level and 2 T_level (the tentative prolongator), level < fcg_amg_levels() - 1: blocks of
 *      3 x 6 on level 0, 6 x 6 below
 *   3  the block inverses the level's smoother applies, [n][b][b] (ptr, col ignored)
 *   4  the dense inverse of the coarsest level, n x n row-major (ptr, col ignored); only for the
 *      last level and only when fcg_amg_stats reports coarse_dense
 * Returns the number of doubles in vals (the blocks of ptr / col are that over the block's size);
 * with ptr = col = vals = NULL only that count.  -1: no such level or matrix, capacity (doubles)
 * below the count, no numeric setup of the handle's own hierarchy, or the copy failed.
 * fcg_amg_level_order: new2old[p] = the context's node (block row) of level 0's node p, n0 / 3
 * entries; the identity when level 0 keeps the context's order. */
int64_t fcg_amg_level_matrix(const fcg_amg* amg, int level, int which, int64_t* ptr, int32_t* col,
    double* vals, int64_t capacity);
int fcg_amg_level_order(const fcg_amg* amg, int32_t* new2old);
int fcg_amg_destroy(fcg_amg* amg);

/* Neumann loads (host arrays; added into fext_row, owned rows only).  funct[d] > 0 selects a
 * spatial function evaluated through `fn` at the reference position of each integration point
 * (Core::Utils::FunctionOfSpaceTime::evaluate); funct may be NULL.
 *   surface: live load on the material configuration, 4C_solid_3D_ele_surface_evaluate.cpp:262-320;
 *            face_nodes[n_faces][4 (hex8 -> quad4) or 9 (hex27 -> quad9)] in 4C surface order
 *   volume:  4C_solid_3D_ele_neumann_evaluator.cpp:45-110; ele_nodes[n_ele][8 or 27] */
typedef double (*fcg_funct_fn)(int funct_id, const double* x, double time, void* user);
int fcg_neumann_surface(int celltype, int64_t n_faces, const int32_t* face_nodes,
    const double* node_x, const int32_t* node_dof_row, const int32_t* onoff, const double* val,
    const int32_t* funct, fcg_funct_fn fn, void* user, double time, double* fext_row);
int fcg_neumann_volume(int celltype, int64_t n_ele, const int32_t* ele_nodes, const double* node_x,
    const int32_t* node_dof_row, const int32_t* onoff, const double* val, const int32_t* funct,
    fcg_funct_fn fn, void* user, double time, double* fext_row);

/* ------------------------------------------------------------------------------------------
 * The matrix graph on the device: what Epetra_CrsMatrix::FillComplete produces
 * after 4C's first assembly through the unfilled path (4C_linalg_sparsematrix.cpp:578-611,
 * 843-865): one row per owned DOF, columns = the DOFs of every node sharing an element with the
 * row's node, sorted by column LID.  All arrays are device memory:
 *   d_ele_nodes [n_ele][8|27] column-node ids; d_node_dof_col [n_node] column LID of the node's
 *   first DOF; d_node_dof_row [n_node] row LID (a multiple of 3) or -1; n_rows = 3 x owned nodes.
 * Fills d_rowptr [n_rows + 1] and *nnz; writes d_col_lid only when it is non-NULL and
 * col_capacity >= *nnz (call once to size, allocate, call again).  At most 16 elements per node.
 * ---------------------------------------------------------------------------------------- */
int fcg_graph_build_device(int device, int celltype, int64_t n_ele, const int32_t* d_ele_nodes,
    int64_t n_node, const int32_t* d_node_dof_col, const int32_t* d_node_dof_row, int64_t n_rows,
    int64_t* d_rowptr, int32_t* d_col_lid, int64_t col_capacity, int64_t* nnz, void* stream);

/* ------------------------------------------------------------------------------------------
 * Non-symmetric systems: restarted flexible GMRES (fcg_krylov.hip).  Right-preconditioned
 * FGMRES(restart) from x = 0 with twice-applied classical Gram-Schmidt; both bases are stored
 * (restart + 1 vectors V, restart vectors Z), so any preconditioner -- an inexact multigrid cycle
 * included -- is admissible.  Stops when the Givens estimate of |r| falls to rtol |b|; the true
 * residual b - A x is recomputed at every restart and before returning, and `rel_residual` is
 * that true |b - A x| / |b|.  The host reads the device's scalar block once per burst of 8 inner
 * steps; steps after convergence or an exact breakdown are no-ops, and `iterations` counts the
 * inner steps actually taken (it may pass the first converged step by fewer than 8).  Every sum
 * runs in a fixed order (no atomics on doubles): two solves of one system give bitwise equal x.
 *   restart in [1, 128], max_iter >= 0, rtol >= 0, else FCG_ERR_ARG
 *   precond   fcg_tsi_gmres_solve: 0 block diagonal, 1 block Gauss-Seidel; ignored here
 * Reaching max_iter returns FCG_OK with the true rel_residual, as fcg_pcg_solve does.  Non-finite
 * b, Hessenberg entry or residual, or a singular Hessenberg matrix: FCG_ERR_SINGULAR.  Work space
 * ((2 restart + 1) n doubles, the partial sums and the preconditioner's blocks) is allocated on
 * the context at the first solve, reused, freed by the destroy call and counted in device_bytes;
 * solves on one context must not run concurrently.  Blocking.
 *
 * fcg_gmres_solve: K x = b for any values on the context's CSR graph (symmetry is not assumed), on
 * a single-rank context whose rows are node DOF triples (else FCG_ERR_ARG, as fcg_pcg_solve).
 * amg NULL: the 3 x 3 nodal block Jacobi of fcg_block_jacobi_setup (FCG_ERR_SINGULAR for a
 * singular block); else one fcg_amg_apply per step -- the caller has run fcg_amg_setup on this K
 * (without it fcg_amg_apply's own error is returned).  With the unit rows of fcg_dirichlet_apply
 * and b = 0 on them, x comes back exactly 0.0 there.
 * ---------------------------------------------------------------------------------------- */
typedef struct fcg_gmres_options {
  int32_t restart;   /* inner steps per cycle (50) */
  int32_t max_iter;  /* inner steps in all (10000) */
  double rtol;       /* |r| <= rtol |b| (1e-10) */
  int32_t precond;   /* fcg_tsi_gmres_solve: 0 block diagonal, 1 block Gauss-Seidel (1) */
  int32_t reserved;
} fcg_gmres_options;
void fcg_gmres_default_options(fcg_gmres_options* opt);
/* Measurement aid (tools/tsi_solve_bench.py), per process and not thread-safe: while enabled, every
 * FGMRES solve records hipEvents around the preconditioner, the operator and the orthogonalisation
 * (Gram-Schmidt, scalar step, scaling) of each inner step it launches, the no-op steps after
 * convergence included; fcg_gmres_get_timing returns the sums (ms) and the step count since
 * fcg_gmres_set_timing was last called.  The events are created on the device current at enable. */
int fcg_gmres_set_timing(int enable);
int fcg_gmres_get_timing(double* ms_precond, double* ms_operator, double* ms_orth, int64_t* steps);
/* One orthogonalisation of the solver on its own, with its kernels (for tests and measurement):
 * w is orthogonalised against the nv vectors d_V + i ld, i < nv, by classical Gram-Schmidt applied
 * twice -- per pass h'_i = v_i . w for all i (one kernel, block partials, fixed-order second
 * stage), then w -= sum_i h'_i v_i -- and d_h receives [nv + 1]: the sums h_i of both passes'
 * coefficients, then |w| of the new w (w is not scaled).  d_V and d_w 16-byte aligned, ld >= n
 * and even, 1 <= nv <= 128, d_work of fcg_gmres_orthogonalize_work(n, nv) doubles (-1: bad
 * arguments); else FCG_ERR_ARG.  Deterministic, asynchronous on `stream`. */
int64_t fcg_gmres_orthogonalize_work(int64_t n, int nv);
int fcg_gmres_orthogonalize(int device, int64_t n, int nv, const double* d_V, int64_t ld, double* d_w,
    double* d_h, double* d_work, void* stream);
int fcg_gmres_solve(fcg_ctx* ctx, fcg_amg* amg_or_null, const double* d_K_vals,
    const double* d_b_row, double* d_x_row, const fcg_gmres_options* opt, int* iterations,
    double* rel_residual, void* stream);

/* ------------------------------------------------------------------------------------------
 * Thermo-structure interaction (TSI), geometrically linear: the temperature-dependent blocks of
 * 4C's monolithic TSI system (TSI::Monolithic, src/tsi/4C_tsi_monolithic.cpp:982-1005, 1694-1869)
 * for SOLIDSCATRA hex8/hex27 elements with MAT_Struct_ThermoStVenantK (constant Young's modulus)
 * and the cloned thermo elements with MAT_Fourier (constant conductivity).  The structural block
 * k_SS and the mechanical part of f_S come from fcg_evaluate_device on an fcg_ctx of the same
 * discretization (linear kinematics: k_SS does not depend on T).
 *   FCG_TSI_STRUCT_FORCE     f_S += thermal-stress part  sum fac B^T m (T - T0) (1,1,1,0,0,0)
 *                            (struct_calc_nlnstiff with the temperature state,
 *                             4C_solid_scatra_3D_ele_calc.cpp:272-403; 4C_mat_thermostvenantkirchhoff.cpp:141-174)
 *   FCG_TSI_STIFFTEMP        k_ST  (struct_calc_stifftemp, 4C_solid_scatra_3D_ele_calc.cpp:405-490,
 *                            AssembleStrategy(0, 1, k_st), 4C_tsi_monolithic.cpp:1724-1732)
 *   FCG_TSI_THERMO_FINTCOND  k_TT and f_T (calc_thermo_fintcond, 4C_thermo_ele_impl.cpp:802-1043)
 *   FCG_TSI_COUPLTANG        k_TS  (calc_thermo_coupltang, 4C_thermo_ele_impl.cpp:1046-1194)
 * ---------------------------------------------------------------------------------------- */
enum fcg_tsi_part {
  FCG_TSI_STRUCT_FORCE = 1,
  FCG_TSI_STIFFTEMP = 2,
  FCG_TSI_THERMO_FINTCOND = 4,
  FCG_TSI_COUPLTANG = 8
};

/* One rank's view of both fields.  The thermo discretization is the structure's clone (same
 * nodes, elements and owners); a node's thermo DOF is owned iff its structural DOFs are.  The
 * graphs are those of the Epetra_CrsMatrix blocks after FillComplete, columns in the matrix
 * column maps = the DOF column maps (node_dof_col_s / node_dof_col_t). */
typedef struct fcg_tsi_desc {
  int32_t abi_version;         /* FCG_ABI_VERSION */
  int32_t celltype;            /* FCG_HEX8 / FCG_HEX27 */
  int32_t device;
  int32_t reserved;
  double youngs, poisson;      /* MAT_Struct_ThermoStVenantK YOUNG (constant), NUE */
  double thexpans;             /* THEXPANS (alpha_T) */
  double inittemp;             /* INITTEMP (reference temperature of the thermal stress) */
  double conduct;              /* MAT_Fourier CONDUCT (isotropic, constant) */
  int64_t n_ele, n_node;       /* column elements / column nodes */
  int64_t n_rows_s, n_cols_s;  /* structural DOF row / column map sizes */
  int64_t n_rows_t, n_cols_t;  /* thermo DOF row / column map sizes */
  const int32_t* ele_nodes;    /* [n_ele][8 or 27] column-node ids, 4C node order */
  const int32_t* ele_gid;      /* [n_ele] (error reporting); may be NULL */
  const double* node_x;        /* [n_node][3] */
  const int32_t* node_dof_col_s, * node_dof_row_s;  /* first structural DOF: column LID, row LID or -1 */
  const int32_t* node_dof_col_t, * node_dof_row_t;  /* thermo DOF: column LID, row LID or -1 */
  const int64_t* rowptr_st; const int32_t* col_st;  /* k_ST: structural rows, thermo columns */
  const int64_t* rowptr_ts; const int32_t* col_ts;  /* k_TS: thermo rows, structural columns */
  const int64_t* rowptr_tt; const int32_t* col_tt;  /* k_TT */
} fcg_tsi_desc;

typedef struct fcg_tsi_ctx fcg_tsi_ctx;
int fcg_tsi_create(const fcg_tsi_desc* desc, fcg_tsi_ctx** out);
int fcg_tsi_destroy(fcg_tsi_ctx* ctx);
const char* fcg_tsi_last_error(const fcg_tsi_ctx* ctx);
/*
 * Device-resident evaluation of the requested parts (bitmask of fcg_tsi_part):
 *   d_v_col   structural velocity, DOF column map (statics: (D_{n+1} - D_n)/dt,
 *             TSI::Algorithm::calc_velocity); needed for FCG_TSI_THERMO_FINTCOND
 *   d_T_col   temperature, thermo DOF column map
 *   timefac, timefac_d   k_TS = -timefac timefac_d (...) (4C_thermo_ele_impl.cpp:1094-1132;
 *                        statics: 1 and 1/dt)
 *   mode      applies to k_ST, k_TS, k_TT and f_T (OVERWRITE = zero + assemble); f_S always `+=`
 *             (its mechanical part comes from fcg_evaluate_device)
 * Error codes as fcg_evaluate_device (FCG_ERR_NODAL_DETJ also for the thermo element's
 * det J < 1e-16, 4C_thermo_ele_impl.cpp:2663-2664, which both thermo actions check:
 * FCG_TSI_THERMO_FINTCOND and FCG_TSI_COUPLTANG, alone or together).
 */
int fcg_tsi_evaluate_device(fcg_tsi_ctx* ctx, int parts, int mode, const double* d_v_col,
    const double* d_T_col, double timefac, double timefac_d, double* d_fs_row, double* d_Kst,
    double* d_fT_row, double* d_Ktt, double* d_Kts, void* stream, int32_t* bad_ele_gid);
/*
 * The whole monolithic TSI tangent and both residuals in ONE pass of the structured hex8 sweep:
 * what fcg_evaluate_device(sctx, FCG_ACTION_NLNSTIFF, mode, d_u_col, d_fs_row, d_Kss) followed by
 * fcg_tsi_evaluate_device(ctx, all parts, mode, ...) computes (TSI::Monolithic::evaluate,
 * 4C_tsi_monolithic.cpp: apply_str_coupl_matrix / apply_thr_coupl_matrix_conv_heat plus the two
 * field evaluates), with each element's Gauss-point work done once for all five blocks.
 *   sctx   structured (FCG_PATH_STRUCTURED) hex8, FCG_LINEAR, FCG_MAT_STVK with the TSI material's
 *          E and nu, on the same mesh, elements and column DOFs as ctx
 *   ctx    node-consistent thermo numbering: thermo LID = structural LID / 3 in the row and
 *          column maps, k_ST / k_TS / k_TT rows the node graph's expansions (what 4C's cloned
 *          thermo discretization with one DOF per node yields)
 *   mode   applies to all outputs (f_S is the full residual: K u + thermal stress part)
 * Returns FCG_ERR_ARG (last_error says why) when the contexts do not qualify; the first call
 * with a structural context checks mesh and graph identity on the device.
 * Environment, read at every call: FCG_TSI_SPLIT=0 runs the one fused pass; unset or anything
 * else (the default) the structural sweep followed by a thermal-only pass of the same kernel.
 */
int fcg_tsi_evaluate_fused(fcg_ctx* sctx, fcg_tsi_ctx* ctx, int mode, const double* d_u_col,
    const double* d_v_col, const double* d_T_col, double timefac, double timefac_d,
    double* d_fs_row, double* d_Kss, double* d_Kst, double* d_fT_row, double* d_Ktt,
    double* d_Kts, void* stream, int32_t* bad_ele_gid);
/*
 * The monolithic system [[K_SS, K_ST], [K_TS, K_TT]] on the device (fcg_tsi_solve.hip): what 4C
 * hands to Belos GMRES with a 2 x 2 block preconditioner (TSI::Monolithic::linear_solve).
 * All three calls need a TSI context with node-consistent numbering (thermo LID = structural
 * LID / 3, the three block graphs expansions of the k_TT node graph; hex8 or hex27) on a single
 * rank (n_cols = n_rows in both fields); the two that take sctx need it on the same device, single
 * rank, with a CSR graph that is the 3 x 3 expansion of the k_TT graph (checked on the device at
 * the first call with that context and cached).  Anything else: FCG_ERR_ARG, and
 * fcg_tsi_last_error names the condition.
 *
 * fcg_tsi_block_apply: y_S = K_SS x_S + K_ST x_T, y_T = K_TS x_S + K_TT x_T in one kernel: a
 * group of lanes per owned node walks the node's k_TT neighbour list once (up to 125 neighbours)
 * and reads the 9 + 3 + 3 + 1 values and the neighbour's four unknowns; the four row sums are
 * reduced across the lanes in a fixed order.  Deterministic, asynchronous on `stream`.
 *
 * fcg_tsi_dirichlet_apply: the structural Dirichlet rows of K_ST and the thermal Dirichlet rows
 * of K_TS become zero rows, the thermal ones of K_TT unit rows, rhs_T is set to 0 there; columns
 * stay (K_SS and rhs_S go through fcg_dirichlet_apply on the structural context).  Any value
 * pointer may be NULL.  A row outside the map or a thermal row without a diagonal entry:
 * FCG_ERR_ARG (the other rows are still applied).  Blocking.
 *
 * fcg_tsi_gmres_solve: FGMRES (above) on the stacked vector [x_S; x_T] with the block apply as
 * operator and the 2-norm of the stacked residual as stopping norm.  P_S is the nodal block Jacobi
 * of K_SS, or fcg_amg_apply on amg_s (set up on K_SS by the caller); D_TT the diagonal of K_TT (a
 * zero, missing or non-finite entry: FCG_ERR_SINGULAR).  opt->precond 0: z_S = P_S r_S,
 * z_T = D_TT^-1 r_T; 1 (block Gauss-Seidel, the BGS of 4C's 2 x 2 block preconditioners):
 * z_S = P_S r_S, z_T = D_TT^-1 (r_T - K_TS z_S), one pass over K_TS fused with the scaling.
 */
int fcg_tsi_block_apply(fcg_ctx* sctx, fcg_tsi_ctx* tctx, const double* d_Kss, const double* d_Kst,
    const double* d_Kts, const double* d_Ktt, const double* d_xs, const double* d_xt, double* d_ys,
    double* d_yt, void* stream);
int fcg_tsi_dirichlet_apply(fcg_tsi_ctx* tctx, int64_t n_dbc_s, const int32_t* d_rows_s,
    int64_t n_dbc_t, const int32_t* d_rows_t, double* d_Kst, double* d_Kts, double* d_Ktt,
    double* d_rhs_T, void* stream);
int fcg_tsi_gmres_solve(fcg_ctx* sctx, fcg_tsi_ctx* tctx, fcg_amg* amg_s_or_null,
    const double* d_Kss, const double* d_Kst, const double* d_Kts, const double* d_Ktt,
    const double* d_bs, const double* d_bt, double* d_xs, double* d_xt,
    const fcg_gmres_options* opt, int* iterations, double* rel_residual, void* stream);

/*
 * The transient thermal field (fcg_thermo.hip): 4C's THERMAL DYNAMIC / DYNAMICTYPE OneStepTheta
 * on the thermo context.  Both calls work on the k_TT graph of any context fcg_tsi_create accepts
 * (hex8 and hex27, any numbering, ranked contexts: owned rows, ghost elements contribute, columns
 * in the thermo column map).
 *
 * fcg_tsi_capacity: the capacity matrix C_ab = sum_e sum_g capa_e w_g det J_g N_a N_b of the thermo
 * element (MAT_Fourier CAPA, the volumetric heat capacity), with the Gauss rule of
 * FCG_TSI_THERMO_FINTCOND and J from the reference coordinates.  capa > 0, or a host table
 * ele_capa[n_ele] of positive entries (column-element order); anything else: FCG_ERR_ARG, and
 * fcg_tsi_last_error names the entry.  OVERWRITE writes every owned entry (entries that belong to
 * no element pair become 0), ACCUMULATE adds.  det J < 1e-16 at a Gauss point (the check of
 * FCG_TSI_THERMO_FINTCOND): FCG_ERR_NODAL_DETJ with the lowest failing element GID.  One wavefront
 * per owned node sums the node's elements in ascending column-element order in LDS: no atomics on
 * doubles, two calls give the same bits.  The kernel's plan (5 bytes per incidence) is part of the
 * context from fcg_tsi_create on; the staging copy of ele_capa is allocated by the first call that
 * is given a table and counted in the context's device memory: calls on one context must not run
 * concurrently.  Blocking, like fcg_mass_assemble.
 *
 * fcg_tsi_ost_combine: one pass over the owned thermo rows per Newton iteration.  On entry d_Ktt
 * and d_fT_row hold what FCG_TSI_THERMO_FINTCOND produced at T_{n+1}; on return
 *   K_TT[j] = fma(theta, K_TT[j], C[j] / dt)                            tangent  C/dt + theta K_TT
 *   f_T[i]  = theta f_T[i] + (1/dt) sum_j C_ij (T_j - Tn_j) + h_i       residual
 * (Thermo::TimIntOneStepTheta: r = C (T_{n+1} - T_n)/dt + theta (F_int,n+1 - F_ext,n+1) +
 * (1 - theta)(F_int,n - F_ext,n), with h = (1 - theta)(f_int,n - f_ext,n) - theta f_ext,n+1 the
 * caller's step-constant vector, NULL = 0).  The difference T_j - Tn_j is formed before the product
 * with C_ij, as the element's ecapa (T_{n+1} - T_n).  d_T_col / d_Tn_col: thermo column map.
 * d_Ktt NULL: residual only; d_fT_row NULL: tangent only; both NULL, theta outside (0, 1], or dt
 * not finite or <= 0: FCG_ERR_ARG.  4 / 16 / 64 lanes per row by the longest row, partial sums in
 * a fixed lane order: deterministic.  Asynchronous on `stream`, like fcg_spmv; a context without
 * rows returns FCG_OK before it looks at its pointers.
 */
int fcg_tsi_capacity(fcg_tsi_ctx* ctx, double capa, const double* ele_capa /* host [n_ele] or NULL */,
    int mode /* fcg_mode */, double* d_Ctt /* [nnz_tt] */, void* stream, int32_t* bad_ele_gid);
int fcg_tsi_ost_combine(fcg_tsi_ctx* ctx, double theta, double dt, const double* d_Ctt,
    const double* d_T_col, const double* d_Tn_col, const double* d_h_row /* may be NULL */,
    double* d_Ktt /* in/out, may be NULL */, double* d_fT_row /* in/out, may be NULL */, void* stream);

/*
 * Thermal boundary conditions on the thermo context (fcg_tsi_surface_plan.cpp, fcg_tsi_surface.hip):
 * 4C's DESIGN THERMO CONVECTION SURF CONDITIONS (a heat transfer coefficient against a surrounding
 * temperature; 4C_thermo_ele_boundary_impl.cpp, calc_thermo_fextconvection, and
 * Thermo::TimInt::apply_force_external_conv) and a surface heat flux.  With linear kinematics the
 * area elements are the reference configuration's and the coefficient is constant per face, so a
 * surface is a fixed sparse operator on its nodes:
 *   M_f,ab = sum_g w_g |dA_g| N_a(g) N_b(g),  m_f,a = sum_g w_g |dA_g| N_a(g)   (quad4: 2x2 Gauss,
 *   quad9: 3x3, the rules and shape functions of fcg_neumann_surface; |dA| = |X,r x X,s|)
 *   A = sum_f coeff_f M_f,   g = sum_f coeff_f surtemp_f m_f,   q = sum_f flux_f m_f
 * and per evaluate f_T += s_c (A T - s_t g), K_TT += s_c A; the heat flux load is f_ext += s_q q.
 * s_c, s_t, s_q: the values at the current time of the condition's time functions.
 *
 * fcg_tsi_surface_create: face_nodes[n_faces][4 or 9] are column node ids of tctx in any valid
 * quad4 / quad9 order (corners cyclic, then mid-edge nodes, then the centre; orientation does not
 * matter).  A node id outside the column nodes, a node twice in a face, n_faces < 0 or an entry that
 * the k_TT graph lacks: FCG_ERR_ARG, fcg_tsi_last_error(tctx) names the face.  Works on any context
 * fcg_tsi_create accepts (hex8 and hex27, any numbering, ranked contexts: pass every face that
 * touches an owned node; owned rows only are written, columns may be ghosts; a face without an owned
 * node contributes nothing).  The surface rows are the owned nodes on a face, ascending by thermo
 * row; each keeps a compact row of the thermo columns of its faces' nodes with the position of every
 * entry in the k_TT value array.  Blocking.  Destroy the surface before its context.
 * fcg_tsi_surface_set: the condition's values, each a scalar or a host table per face (a table
 * takes the scalar's place).  A coefficient that is negative or not finite, a surrounding
 * temperature or flux that is not finite: FCG_ERR_ARG with the face in *bad_face and in
 * fcg_tsi_last_error, and the tables of an earlier set stay as they were.  Runs the setup kernel (one
 * wavefront per surface row, its faces in ascending order, sums in Gauss-point order: no atomics on
 * doubles, two calls give the same bits); |dA| zero or not finite at a Gauss point: FCG_ERR_SINGULAR
 * with the lowest failing face index, and the surface counts as not set.  Blocking.
 * fcg_tsi_convection: one pass over the surface rows, 4 / 16 / 64 lanes per row by the longest
 * compact row: d_fT_row[row] += s_c (sum_k A_k T[col_k] - s_t g), d_Ktt[pos_k] = fma(s_c, A_k,
 * d_Ktt[pos_k]).  d_Ktt NULL: residual only (with d_T_col = T_n 4C's explicit Tempn variant);
 * d_fT_row NULL: tangent only; both NULL, or before a successful set: FCG_ERR_ARG.  Rows that are not
 * surface rows and entries outside the compact rows are never touched.  Asynchronous on `stream`,
 * no allocation, deterministic; a surface without rows returns FCG_OK before it looks at its
 * pointers.  Several surfaces of one context are applied one after the other, each call adds.
 * fcg_tsi_surface_flux: d_f_row[row] += scale q.  Asynchronous.
 * fcg_tsi_surface_tables: the device arrays of the surface (rows [n_rows], ptr [n_rows + 1], col /
 * pos / A [n_entries], g / q [n_rows]), for tests and tools; any pointer may be NULL.
 */
typedef struct fcg_tsi_surface fcg_tsi_surface;
int fcg_tsi_surface_create(fcg_tsi_ctx* tctx, int64_t n_faces, const int32_t* face_nodes,
    fcg_tsi_surface** out);
int fcg_tsi_surface_set(fcg_tsi_surface* s, double coeff, const double* face_coeff /* host [n_faces] or NULL */,
    double surtemp, const double* face_surtemp, double flux, const double* face_flux, int64_t* bad_face);
int fcg_tsi_surface_info(const fcg_tsi_surface* s, int64_t* n_rows, int64_t* n_entries,
    int64_t* device_bytes);
int fcg_tsi_surface_tables(const fcg_tsi_surface* s, const int32_t** d_rows, const int64_t** d_ptr,
    const int32_t** d_col, const int64_t** d_pos, const double** d_A, const double** d_g,
    const double** d_q);
int fcg_tsi_convection(fcg_tsi_surface* s, double coeff_scale, double surtemp_scale,
    const double* d_T_col, double* d_fT_row /* += , may be NULL */, double* d_Ktt /* += , may be NULL */,
    void* stream);
int fcg_tsi_surface_flux(fcg_tsi_surface* s, double scale, double* d_f_row /* += */, void* stream);
int fcg_tsi_surface_destroy(fcg_tsi_surface* s);

/*
 * Scalar smoothed-aggregation AMG of K_TT (fcg_samg_plan.cpp, fcg_samg.hip): the multigrid of the
 * thermal block, one DOF per node, the constant as near-null space -- what MueLu builds for the
 * thermal field of 4C's TSI block preconditioners, and a solver for a conduction problem on its
 * own.  Two stages as fcg_amg: a host plan at create, a numeric setup per matrix.
 *
 * fcg_samg_create: a single-rank thermo context with node-consistent numbering (n_cols_t =
 * n_rows_t, else FCG_ERR_ARG), its k_TT node graph on the host (int64 rowptr_tt, int32 col_tt,
 * columns ascending) and the thermal Dirichlet rows, which join no aggregate: their prolongator
 * rows stay empty (a row outside the map: FCG_ERR_ARG).  opt as fcg_amg_options (coarse_max_iter
 * and coarse_rtol are not used: the coarsest level is always inverted densely, so a hierarchy that
 * ends above 4096 rows is refused with FCG_ERR_ARG); NULL takes fcg_samg_default_options, the
 * structural defaults with coarse_max = 300 rows (the structural 3000 DOFs are 500 coarse nodes of
 * six DOFs; here a row is a node).  The tentative prolongator of node i is 1 / sqrt |agg(i)| on
 * level 0 (B_i / |B_agg|_2 with the level's near-null-space vector B below), the coarse near-null
 * space sqrt |agg|.  Errors of create are reported through fcg_tsi_last_error of the context;
 * device memory is counted in the context's device_bytes.  Destroy the handle before the context.
 *
 * fcg_samg_setup: the numeric setup for d_Ktt (K_TT with its Dirichlet rows applied), read in
 * place as level 0 -- no copy is kept, so the same buffer is passed to apply / solve and must stay
 * unchanged until the next setup.  Per level: 1 / diag (a zero, missing or non-finite entry:
 * FCG_ERR_SINGULAR), lambda_max(D^-1 A) by a 10-step Lanczos, P = T - (omega / lambda_max) D^-1
 * (A T), A P and A_c = P^T (A P) from product plans, one thread per entry; the coarsest level's
 * dense inverse (a pivot <= 0: FCG_ERR_SINGULAR).  Blocking.
 * fcg_samg_apply: one V-cycle z = M r from z = 0: nu Chebyshev degrees before and after (each one
 * fused kernel: residual, Jacobi scaling, update), the dense coarsest inverse.  Asynchronous on
 * `stream`; before any setup FCG_ERR_ARG.
 * fcg_samg_solve: flexible CG from x = 0 with one V-cycle per step to |r| <= rtol |b|;
 * rel_residual is the true residual at return; FCG_ERR_SINGULAR when the cycle turns indefinite.
 * With unit Dirichlet rows and b = 0 on them x comes back exactly 0.0 there.  Blocking.
 * Every sum runs in a fixed order, no atomics on doubles: two setups, applies or solves give the
 * same bits.
 * fcg_samg_level_info: rows, non-zeros and the lambda_max estimate of level 0 .. levels - 1 (0 on
 * the coarsest).  fcg_samg_level_matrix: a host copy of the level's CSR after the last setup,
 * which = 0: A_l, 1: P_l (l < levels - 1); ptr[rows + 1], col / vals[capacity]; returns the
 * non-zero count (ptr = col = vals = NULL: a size query), -1 on bad arguments.
 * fcg_samg_setup_ms: host time of level's share of the last numeric setup (level l < levels - 1:
 * the Lanczos estimate, P_l, A_l P_l and A_{l+1}; the coarsest level: its dense inverse), level
 * -1: the whole setup.
 *
 * fcg_tsi_gmres_solve_amg: fcg_tsi_gmres_solve (= this call with amg_t NULL) with the thermal
 * half of the preconditioner one V-cycle M_T of amg_t in place of D_TT^-1: precond 0
 * z_T = M_T r_T, 1 z_T = M_T (r_T - K_TS z_S), the bracket formed in one pass over K_TS.  The
 * caller has run fcg_samg_setup on this d_Ktt; a handle of another thermo context: FCG_ERR_ARG.
 *
 * fcg_scsr_spmv / fcg_scsr_chebyshev_step: the level kernels on any scalar CSR matrix in device
 * memory (row_width: its longest row; it selects 4, 16 or 64 lanes per row).  spmv mode 0:
 * y = alpha A x, 1: y += alpha A x, 2: y = b - A x.  chebyshev_step, with z = (b - A x) / a_ii
 * and d_dinv = 1 / a_ii, the modes of fcg_chebyshev_step: 0: d = c_r z, 1: d = c_d d + c_r z,
 * then x_out = x + d; 2: d = x_out = c_r b / a_ii (A and x are not read).  x_out must not be x.
 */
typedef struct fcg_samg fcg_samg;
void fcg_samg_default_options(fcg_amg_options* opt);
int fcg_samg_create(fcg_tsi_ctx* tctx, const int64_t* rowptr_tt, const int32_t* col_tt,
    int64_t n_dbc, const int32_t* dbc_rows_t, const fcg_amg_options* opt, fcg_samg** out);
int fcg_samg_setup(fcg_samg* amg, const double* d_Ktt, void* stream);
int fcg_samg_apply(fcg_samg* amg, const double* d_Ktt, const double* d_r, double* d_z, void* stream);
int fcg_samg_solve(fcg_samg* amg, const double* d_Ktt, const double* d_b, double* d_x, double rtol,
    int max_iter, int* iterations, double* rel_residual, void* stream);
int fcg_samg_levels(const fcg_samg* amg);
int fcg_samg_level_info(const fcg_samg* amg, int level, int64_t* rows, int64_t* nnz, double* lmax);
int64_t fcg_samg_level_matrix(const fcg_samg* amg, int level, int which, int64_t* ptr, int32_t* col,
    double* vals, int64_t capacity);
double fcg_samg_setup_ms(const fcg_samg* amg, int level);
const char* fcg_samg_last_error(const fcg_samg* amg);
int fcg_samg_destroy(fcg_samg* amg);
int fcg_tsi_gmres_solve_amg(fcg_ctx* sctx, fcg_tsi_ctx* tctx, fcg_amg* amg_s_or_null,
    fcg_samg* amg_t_or_null, const double* d_Kss, const double* d_Kst, const double* d_Kts,
    const double* d_Ktt, const double* d_bs, const double* d_bt, double* d_xs, double* d_xt,
    const fcg_gmres_options* opt, int* iterations, double* rel_residual, void* stream);
int fcg_scsr_spmv(int device, int64_t n, int64_t row_width, const int64_t* d_ptr, const int32_t* d_col,
    const double* d_vals, const double* d_x, const double* d_b, double* d_y, double alpha, int mode,
    void* stream);
int fcg_scsr_chebyshev_step(int device, int64_t n, int64_t row_width, const int64_t* d_ptr,
    const int32_t* d_col, const double* d_vals, const double* d_dinv, const double* d_b,
    const double* d_x, double* d_d, double* d_x_out, double c_d, double c_r, int mode, void* stream);

/* ------------------------------------------------------------------------------------------
 * Structured-box discretization builder: a restatement of 4C's GridGenerator
 * (src/core/io/src/4C_io_gridgenerator.cpp:41-392), node ownership of Rebalance::build_graph
 * (src/core/rebalance/src/4C_rebalance_graph_based.cpp:159-215), DofSet numbering
 * (src/core/fem/src/dofset/4C_fem_dofset.cpp:343-351) and the Epetra graph after FillComplete.
 * It produces exactly what a 4C rank would hand to fcg_create, for synthetic meshes.
 * ---------------------------------------------------------------------------------------- */
typedef struct fcg_box {
  int32_t celltype;        /* FCG_HEX8 / FCG_HEX27 */
  int32_t interval[3];     /* INTERVALS */
  double lower[3];         /* LOWER_BOUND */
  double upper[3];         /* UPPER_BOUND */
  double rotation[3];      /* ROTATION (degrees) */
  int64_t first_node_gid;  /* node_gid_of_first_new_node */
  double jitter;           /* interior-node jitter as a fraction of h (0 = none) */
  uint64_t jitter_seed;    /* SplitMix64 seed */
} fcg_box;

typedef struct fcg_box_mesh fcg_box_mesh;

/* Builds rank `rank` of `nranks` (PARTITION structured box split). */
int fcg_box_mesh_create(const fcg_box* box, int rank, int nranks, fcg_box_mesh** out);
int fcg_box_mesh_destroy(fcg_box_mesh* m);
/* Fills a descriptor that points into the mesh's arrays (valid while the mesh lives). */
int fcg_box_mesh_desc(const fcg_box_mesh* m, int kinematics, double youngs, double poisson,
    int device, fcg_desc* out);
/* Global numbering of the rank's maps: DOF GIDs of the row map [n_rows] and column map [n_cols],
 * node GIDs of the column nodes [n_node], owner rank of each column node [n_node]. */
int fcg_box_mesh_maps(const fcg_box_mesh* m, const int32_t** row_gid, const int32_t** col_gid,
    const int64_t** node_gid, const int32_t** node_owner);
/* Total number of elements (all ranks) and owned (row) elements of this rank. */
int fcg_box_mesh_counts(const fcg_box_mesh* m, int64_t* n_ele_global, int64_t* n_ele_row);
/* fcg_box_mesh_create with options.  FCG_BOX_STRICT: strict element partition (SURVEY §8e option
 * B): the rank holds only its row elements (no ghost layer); every node those elements touch gets a
 * row -- the owned DOF rows first (LIDs [0, n_owned_rows), as without the flag), then one extended
 * row triple per touched node owned by another rank, so the row map equals the column map.  The
 * extended rows collect the rank's partial sums for the interface DOFs, which fcg_shared_reduce
 * completes.  fcg_box_mesh_maps' row_gid then lists the extended rows' GIDs after the owned ones. */
enum fcg_box_flags { FCG_BOX_GHOSTED = 0, FCG_BOX_STRICT = 1 };
int fcg_box_mesh_create_ex(const fcg_box* box, int rank, int nranks, int flags, fcg_box_mesh** out);
/* Owned DOF rows of the rank (= n_rows without FCG_BOX_STRICT). */
int fcg_box_mesh_owned_rows(const fcg_box_mesh* m, int64_t* n_owned_rows);

/* ------------------------------------------------------------------------------------------
 * Multi-GPU: one rank per GPU, elements partitioned like GridGenerator's box split.
 * The collectives on 4C's path map onto RCCL over xGMI:
 *   Discretization::set_state's row -> column Epetra_Import (4C_fem_discretization.cpp:542-548)
 *       -> fcg_halo_import: grouped ncclSend / ncclRecv of the ghost DOFs with the neighbours;
 *   Core::Communication::sum_all (4C_comm_mpi_utils.hpp:294-306) on the shared-DOF residual of a
 *       strict element partition -> fcg_shared_reduce: ncclAllReduce of a compact interface buffer;
 *   the NOX residual norm (Epetra Norm2 -> MPI_Allreduce) -> fcg_norm2.
 * Plans are built on the host from the maps a 4C rank holds, with one host exchange callback
 * (fcg_alltoallv_fn: an MPI_Alltoallv wrapper in 4C, fcg_comm_alltoallv over RCCL); a host that
 * moves the bytes itself (MPI, host-staged) uses the pack / unpack halves instead of the RCCL
 * entry points.  All device calls are asynchronous on `stream` unless stated.
 * ---------------------------------------------------------------------------------------- */
typedef struct fcg_comm fcg_comm;
#define FCG_COMM_ID_BYTES 128
enum fcg_op { FCG_OP_SUM = 0, FCG_OP_MAX = 1 };
/* Rank 0 makes the id (ncclGetUniqueId); the host broadcasts its FCG_COMM_ID_BYTES bytes. */
int fcg_comm_unique_id(void* id);
/* Collective over nranks: one RCCL communicator per rank, on HIP device `device`. */
int fcg_comm_create(const void* id, int nranks, int rank, int device, fcg_comm** out);
int fcg_comm_destroy(fcg_comm* comm);
/* The communicator's size as RCCL reports it (ncclCommCount); Epetra_Comm::NumProc in 4C. */
int fcg_comm_size(const fcg_comm* comm, int* nranks);
/* This rank in the communicator (ncclCommUserRank); Epetra_Comm::MyPID in 4C. */
int fcg_comm_rank(const fcg_comm* comm, int* rank);
/* In-place all-reduce of n doubles in device memory (ncclAllReduce). */
int fcg_comm_allreduce(fcg_comm* comm, double* d_buf, int64_t n, int op, void* stream);

/* Host exchange with MPI_Alltoallv semantics: this rank sends send_counts[p] items of item_bytes
 * bytes to every rank p (packed in rank order in send_buf) and receives recv_counts[p] items from
 * every p (packed in rank order in recv_buf).  Returns 0 on success. */
typedef int (*fcg_alltoallv_fn)(const void* send_buf, const int64_t* send_counts, void* recv_buf,
    const int64_t* recv_counts, int64_t item_bytes, void* user);
/* An fcg_alltoallv_fn over RCCL (user = the fcg_comm*); host buffers, blocking. */
int fcg_comm_alltoallv(const void* send_buf, const int64_t* send_counts, void* recv_buf,
    const int64_t* recv_counts, int64_t item_bytes, void* comm);

/* The row -> column import of one rank (what Epetra_Import(colmap, rowmap) holds: NumSameIDs,
 * PermuteFromLIDs / PermuteToLIDs, ExportLIDs / ExportPIDs, RemoteLIDs), peers in rank order. */
typedef struct fcg_import_plan {
  int32_t nranks, rank;
  int64_t n_rows, n_cols;
  int64_t n_same;               /* columns [0, n_same) take rows [0, n_same) */
  int64_t n_permute;
  const int32_t* permute_from;  /* [n_permute] row LIDs */
  const int32_t* permute_to;    /* [n_permute] column LIDs */
  const int64_t* send_counts;   /* [nranks] values this rank sends to every peer */
  const int32_t* send_row;      /* [sum send_counts] row LIDs, grouped by peer in rank order */
  const int64_t* recv_counts;   /* [nranks] values received from every peer */
  const int32_t* recv_col;      /* [sum recv_counts] column LIDs, grouped by peer in rank order */
} fcg_import_plan;
/* Builds the plan from the rank's maps (collective, two exchanges through xchg): row_gid [n_rows]
 * owned DOF GIDs; col_gid [n_cols] column DOF GIDs with their owners col_owner [n_cols] (4C:
 * node->owner()).  *out points into *storage, released by fcg_plan_free. */
int fcg_import_plan_build(int rank, int nranks, int64_t n_rows, const int32_t* row_gid,
    int64_t n_cols, const int32_t* col_gid, const int32_t* col_owner, fcg_alltoallv_fn xchg,
    void* user, fcg_import_plan* out, void** storage);
void fcg_plan_free(void* storage);

typedef struct fcg_halo fcg_halo;
/* Device copy of an import plan (the plan's arrays are copied). */
int fcg_halo_create(const fcg_import_plan* plan, int device, fcg_halo** out);
int fcg_halo_destroy(fcg_halo* h);
/* set_state: d_u_col = import of d_u_row, the ghost values over RCCL (grouped send / recv; peers
 * whose ghost columns are contiguous receive straight into d_u_col). */
int fcg_halo_import(fcg_halo* h, fcg_comm* comm, const double* d_u_row, double* d_u_col,
    void* stream);
/* Host-transport halves: pack copies the owned columns and writes the values every peer needs into
 * d_send [sum send_counts] (plan order); after the host moved d_send to the peers' d_recv
 * [sum recv_counts], unpack scatters d_recv into the ghost columns. */
int fcg_halo_pack(fcg_halo* h, const double* d_u_row, double* d_u_col, double* d_send, void* stream);
int fcg_halo_unpack(fcg_halo* h, const double* d_recv, double* d_u_col, void* stream);

/* Shared-DOF reduction of a strict element partition (FCG_BOX_STRICT layout: owned rows
 * [0, n_owned), extended rows n_owned + k for the non-owned DOFs ext_gid[k] the rank's elements
 * touch, owned by ext_owner[k]).  The interface = every DOF some rank holds as an extended row;
 * it is numbered globally by (owner rank, GID), so all ranks share one all-reduce buffer of
 * n_global doubles. */
typedef struct fcg_shared_plan {
  int32_t nranks, rank;
  int64_t n_global;             /* interface DOFs over all ranks (all-reduce length) */
  int64_t n_local;              /* interface entries of this rank */
  int64_t n_owned;              /* the first n_owned entries are owned rows: they get the sums */
  const int32_t* row;           /* [n_local] row LIDs (owned, then extended) */
  const int64_t* pos;           /* [n_local] position in the all-reduce buffer */
} fcg_shared_plan;
int fcg_shared_plan_build(int rank, int nranks, int64_t n_owned_rows, const int32_t* owned_gid,
    int64_t n_ext_rows, const int32_t* ext_gid, const int32_t* ext_owner, fcg_alltoallv_fn xchg,
    void* user, fcg_shared_plan* out, void** storage);

typedef struct fcg_shared fcg_shared;
int fcg_shared_create(const fcg_shared_plan* plan, int device, fcg_shared** out);
int fcg_shared_destroy(fcg_shared* s);
/* d_f [n_owned_rows + n_ext_rows] holds this rank's partial sums (an FCG_CALC_INTERNALFORCE
 * evaluate of its row elements); afterwards the owned interface rows hold the global sums
 * (pack -> ncclAllReduce(sum) -> unpack).  Rows away from the interface are already complete. */
int fcg_shared_reduce(fcg_shared* s, fcg_comm* comm, double* d_f, void* stream);
/* Host-transport halves: d_buf [n_global] = zero + this rank's interface partials; the host sums
 * d_buf over the ranks (MPI_Allreduce); unpack writes the sums into the owned interface rows. */
int fcg_shared_pack(fcg_shared* s, const double* d_f, double* d_buf, void* stream);
int fcg_shared_unpack(fcg_shared* s, const double* d_buf, double* d_f, void* stream);

/* ||x||_2 over all ranks (comm may be NULL: this rank only); fixed-order partial sums, blocking. */
int fcg_norm2(fcg_comm* comm, const double* d_x, int64_t n, void* stream, double* out);

/* ------------------------------------------------------------------------------------------
 * Linear solve across ranks (what 4C hands to Belos with a MueLu / Ifpack preconditioner on
 * every rank, 4C_solver_nonlin_nox_linearsystem.cpp:275-353,
 * 4C_linear_solver_preconditioner_muelu.cpp): flexible CG on the ghost-layer partition.  Per
 * iteration: one import of the search direction into the column map (Epetra_CrsMatrix::Multiply's
 * Importer), one fcg_spmv of the rank's owned rows, one preconditioner application local to the
 * rank -- the rank's fcg_amg on its owned block (subdomain AMG, additive Schwarz without overlap)
 * or, with amg = NULL, the nodal 3 x 3 block Jacobi -- and two all-reduces of a few scalars.
 * Data movement goes through an fcg_transport: fcg_transport_rccl (fcg_halo_import + ncclAllReduce
 * of a device buffer), or caller callbacks (MPI, or a host-staged rehearsal).  K holds the
 * Dirichlet unit rows (fcg_dirichlet_apply); the context's column map must start with its owned
 * DOFs in row order (Epetra's local-first column maps).  Collective: every rank calls it, and
 * either every rank passes an AMG handle or none does (fcg_amg_create refuses a rank without
 * rows; such a partition solves with the block Jacobi, amg = NULL).  Blocking; x starts at 0.
 * ---------------------------------------------------------------------------------------- */
typedef int (*fcg_import_fn)(void* user, const double* d_x_row, double* d_x_col, void* stream);
typedef int (*fcg_allreduce_fn)(void* user, double* d_vals, int64_t n, void* stream);  /* in place, sum */
/* Point-to-point exchange of device doubles with MPI_Alltoallv semantics (the Epetra_Import /
 * Export of a distributed coarse level): send_counts[p] doubles to rank p, packed in rank order in
 * d_send, recv_counts[p] from rank p into d_recv in rank order; counts are host arrays of nranks
 * entries, this rank's own entries 0.  Ordered after the work already queued on `stream`. */
typedef int (*fcg_exchange_fn)(void* user, const double* d_send, const int64_t* send_counts,
    double* d_recv, const int64_t* recv_counts, void* stream);
/* Zero-initialise the struct (`fcg_transport t = {0};` / `{}`) before filling it field by field:
 * members added in later ABI versions (exchange_fn in version 2) must read NULL, not garbage. */
typedef struct fcg_transport {
  fcg_import_fn import_fn;
  fcg_allreduce_fn allreduce_fn;
  void* user;
  /* this rank and the rank count of the partition (MPI_Comm_rank / _size in 4C).  With
   * nranks > 1 an AMG handle's coarse levels are coupled across the ranks; nranks <= 1 (a
   * zero-initialised struct) keeps the rank-local AMG.  Without exchange_fn the global Galerkin
   * operator A_1 = P_0^T A P_0 is gathered by allreduce_fn and solved redundantly on every rank;
   * with it, level 1 is distributed (each rank owns the rows of its aggregates, its own import
   * plan, the partial rows of the other ranks' aggregates sent to their owners) once its global
   * size passes FCG_AMG_DIST_MIN DOFs (default 50000; FCG_AMG_DIST=1 always, 0 never), and so
   * is every coarser level past that size (FCG_AMG_DIST_LEVELS caps the count, default 8): the
   * first level under it is the one replicated (fcg_amg_coupled_stats). */
  int32_t rank;
  int32_t nranks;
  fcg_exchange_fn exchange_fn;  /* may be NULL */
} fcg_transport;
/* The RCCL transport of (comm, halo): fills *out; `pair` (caller-owned, alive while used) holds
 * the two handles the callbacks receive as `user`. */
typedef struct fcg_rccl_pair {
  fcg_comm* comm;
  fcg_halo* halo;
} fcg_rccl_pair;
int fcg_transport_rccl(fcg_rccl_pair* pair, fcg_transport* out);
/* AMG as the rank's local preconditioner: one V-cycle z = M^-1 r on the owned block after
 * fcg_amg_setup (fcg_amg_create accepts a multi-rank context: ghost columns are dropped). */
int fcg_amg_apply(fcg_amg* amg, const double* d_K_vals, const double* d_r_row, double* d_z_row, void* stream);
/* Levels of the coarse hierarchy coupled across ranks that fcg_dfcg_solve built for this handle
 * (level 1 = the global A_1 and its coarsenings; 0 = none: single rank, or nranks <= 1). */
int fcg_amg_coupled_levels(const fcg_amg* amg);
/* What the coupled coarse levels cost this rank (after the first fcg_dfcg_solve), out[0..n):
 *   0 distributed levels (0: A_1 replicated, 1: A_1 distributed and A_2 replicated, k: levels
 *     1..k distributed and A_{k+1} replicated)
 *   1 level-1 block rows (6 DOFs each) this rank stores: its own (distributed) or all (replicated)
 *   2 level-1 block rows over all ranks
 *   3 doubles all-reduced per numeric setup (the replicated level's Galerkin operator)
 *   4 doubles all-reduced per preconditioner application (the replicated level's right-hand side)
 *   5 doubles this rank sends per numeric setup through exchange_fn (partial rows of every
 *     distributed level, P's ghost rows)
 *   6 doubles this rank sends per application through exchange_fn (imports, restriction and
 *     prolongation of every distributed level)
 *   7 bytes of the replicated hierarchy's matrices on this rank
 *   8 block rows of the replicated level (the first coarse level not distributed)
 * Returns the number of entries written (<= n). */
int fcg_amg_coupled_stats(const fcg_amg* amg, int64_t* out, int n);
/* fcg_exchange_fn over RCCL (user = fcg_comm*): grouped ncclSend / ncclRecv on `stream`. */
int fcg_comm_exchange_device(void* comm, const double* d_send, const int64_t* send_counts,
    double* d_recv, const int64_t* recv_counts, void* stream);
int fcg_dfcg_solve(fcg_ctx* ctx, fcg_amg* amg, const fcg_transport* tr, const double* d_K_vals,
    const double* d_b_row, double* d_x_row, double rtol, int max_iter, void* stream,
    int* iterations, double* rel_residual);

/* ------------------------------------------------------------------------------------------
 * Deferred error check.  With fcg_set_async(ctx, 1), fcg_evaluate_device returns once the work is
 * queued on the stream (no drain, no host round trip per call); 4C's throws (FCG_ERR_NODAL_DETJ,
 * FCG_ERR_SINGULAR) are then reported by fcg_check_error, which waits for the queued evaluates
 * and returns the first failure since the last check (sticky until checked: fcg_dirichlet_apply,
 * fcg_pcg_solve and fcg_block_jacobi_setup report through a flag word of their own, and
 * fcg_evaluate_host / fcg_tsi_evaluate_fused report a pending failure before they start).
 * ---------------------------------------------------------------------------------------- */
int fcg_set_async(fcg_ctx* ctx, int enable);
int fcg_check_error(fcg_ctx* ctx, int32_t* bad_ele_gid);

/* ------------------------------------------------------------------------------------------
 * Host-buffer evaluate with the matrix lifecycle of the caller: mode FCG_OVERWRITE fuses the
 * caller's SparseMatrix::zero() (4C re-creates the values from the saved graph right before the
 * evaluate, 4C_linalg_sparsematrix.cpp:353-378, 4C_structure_new_model_evaluator_structure.cpp:
 * 143-151): K_vals and fint_row are only written, never read, which halves the PCIe traffic.
 * FCG_ACCUMULATE is fcg_evaluate (+=).  Blocking.
 * ---------------------------------------------------------------------------------------- */
int fcg_evaluate_host(fcg_ctx* ctx, int action, int mode, const double* u_col, double* fint_row,
    double* K_vals, int32_t* bad_ele_gid);

#ifdef __cplusplus
}
#endif
#endif /* FOURC_GPU_H */
