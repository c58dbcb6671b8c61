"""ctypes binding of libfourc_gpu (include/fourc_gpu.h) for tests, bench and Python hosts.

This is glue, not the product: every evaluation goes through the C ABI into the HIP kernels of
4c_amd/csrc.  There is no CPU fallback -- if the shared library is missing the import fails loudly.
Device buffers are torch tensors on `cuda:N` (PyTorch supplies device memory and streams only).
"""

import ctypes
import os

import numpy as np

PKG_DIR = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.path.join(PKG_DIR, "lib", "libfourc_gpu.so")
# diagnostics / A-B timing only: FCG_LIB=<name> loads lib/libfourc_gpu_<name>.so instead
# (diag = the phase-stamp build, make -C 4c_amd diag)
if os.environ.get("FCG_LIB"):
    LIB_PATH = os.path.join(PKG_DIR, "lib", "libfourc_gpu_%s.so" % os.environ["FCG_LIB"])

HEX8, HEX27 = 0, 1
LINEAR, TOTLAG = 0, 1
CALC_NLNSTIFF, CALC_INTERNALFORCE = 0, 1
ACCUMULATE, OVERWRITE = 0, 1
PATH_AUTO, PATH_GENERAL, PATH_STRUCTURED, PATH_COLORED, PATH_GATHER = 0, 1, 2, 3, 4
MAT_STVK, MAT_ELASTHYPER_COUPNEOHOOKE = 0, 1
TSI_STRUCT_FORCE, TSI_STIFFTEMP, TSI_THERMO_FINTCOND, TSI_COUPLTANG = 1, 2, 4, 8
TSI_ALL = 15
STRESS_NONE, STRESS_PK2, STRESS_CAUCHY = 0, 1, 2
STRAIN_NONE, STRAIN_GL, STRAIN_EA = 0, 1, 2
ABI_VERSION = 2

FCG_OK, FCG_ERR_NODAL_DETJ, FCG_ERR_SINGULAR, FCG_ERR_ARG, FCG_ERR_DEVICE = 0, 1, 2, 3, 4
STATUS = {0: "FCG_OK", 1: "FCG_ERR_NODAL_DETJ", 2: "FCG_ERR_SINGULAR", 3: "FCG_ERR_ARG",
          4: "FCG_ERR_DEVICE"}

_i32p = ctypes.POINTER(ctypes.c_int32)
_i64p = ctypes.POINTER(ctypes.c_int64)
_dp = ctypes.POINTER(ctypes.c_double)


class FcgDesc(ctypes.Structure):
    _fields_ = [("abi_version", ctypes.c_int32), ("celltype", ctypes.c_int32),
                ("kinematics", ctypes.c_int32), ("device", ctypes.c_int32),
                ("youngs", ctypes.c_double), ("poisson", ctypes.c_double),
                ("n_ele", ctypes.c_int64), ("n_node", ctypes.c_int64), ("n_rows", ctypes.c_int64),
                ("n_cols", ctypes.c_int64), ("ele_nodes", _i32p), ("ele_gid", _i32p),
                ("node_x", _dp), ("node_dof_col", _i32p), ("node_dof_row", _i32p),
                ("node_dof_kcol", _i32p), ("rowptr", _i64p), ("col_lid", _i32p),
                ("ele_ijk", _i32p), ("path", ctypes.c_int32), ("material", ctypes.c_int32)]


class FcgBox(ctypes.Structure):
    _fields_ = [("celltype", ctypes.c_int32), ("interval", ctypes.c_int32 * 3),
                ("lower", ctypes.c_double * 3), ("upper", ctypes.c_double * 3),
                ("rotation", ctypes.c_double * 3), ("first_node_gid", ctypes.c_int64),
                ("jitter", ctypes.c_double), ("jitter_seed", ctypes.c_uint64)]


class FcgInfo(ctypes.Structure):
    _fields_ = [("n_ele", ctypes.c_int64), ("n_node", ctypes.c_int64), ("n_rows", ctypes.c_int64),
                ("n_cols", ctypes.c_int64), ("nnz", ctypes.c_int64),
                ("n_incidences", ctypes.c_int64), ("scratch_bytes", ctypes.c_int64),
                ("device_bytes", ctypes.c_int64), ("path", ctypes.c_int32),
                ("h27_slabs", ctypes.c_int32)]


class FcgImportPlan(ctypes.Structure):
    _fields_ = [("nranks", ctypes.c_int32), ("rank", ctypes.c_int32),
                ("n_rows", ctypes.c_int64), ("n_cols", ctypes.c_int64),
                ("n_same", ctypes.c_int64), ("n_permute", ctypes.c_int64),
                ("permute_from", _i32p), ("permute_to", _i32p),
                ("send_counts", _i64p), ("send_row", _i32p),
                ("recv_counts", _i64p), ("recv_col", _i32p)]


class FcgSharedPlan(ctypes.Structure):
    _fields_ = [("nranks", ctypes.c_int32), ("rank", ctypes.c_int32),
                ("n_global", ctypes.c_int64), ("n_local", ctypes.c_int64),
                ("n_owned", ctypes.c_int64), ("row", _i32p), ("pos", _i64p)]


# fcg_alltoallv_fn: (send_buf, send_counts, recv_buf, recv_counts, item_bytes, user) -> int
ALLTOALLV_FN = ctypes.CFUNCTYPE(ctypes.c_int, ctypes.c_void_p, _i64p, ctypes.c_void_p, _i64p,
                                ctypes.c_int64, ctypes.c_void_p)
FCG_OP_SUM, FCG_OP_MAX = 0, 1
BOX_GHOSTED, BOX_STRICT = 0, 1
# fcg_transport (distributed solve): import (user, d_x_row, d_x_col, stream), all-reduce (user,
# d_vals, n, stream), both -> int
IMPORT_FN = ctypes.CFUNCTYPE(ctypes.c_int, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p,
                             ctypes.c_void_p)
ALLREDUCE_FN = ctypes.CFUNCTYPE(ctypes.c_int, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_int64,
                                ctypes.c_void_p)
# (user, d_send, send_counts[nranks], d_recv, recv_counts[nranks], stream): MPI_Alltoallv of doubles
EXCHANGE_FN = ctypes.CFUNCTYPE(ctypes.c_int, ctypes.c_void_p, ctypes.c_void_p,
                               ctypes.POINTER(ctypes.c_int64), ctypes.c_void_p,
                               ctypes.POINTER(ctypes.c_int64), ctypes.c_void_p)


class FcgTransport(ctypes.Structure):
    _fields_ = [("import_fn", IMPORT_FN), ("allreduce_fn", ALLREDUCE_FN), ("user", ctypes.c_void_p),
                ("rank", ctypes.c_int32), ("nranks", ctypes.c_int32), ("exchange_fn", EXCHANGE_FN)]


class FcgRcclPair(ctypes.Structure):
    _fields_ = [("comm", ctypes.c_void_p), ("halo", ctypes.c_void_p)]


class FcgTsiDesc(ctypes.Structure):
    _fields_ = [("abi_version", ctypes.c_int32), ("celltype", ctypes.c_int32),
                ("device", ctypes.c_int32), ("reserved", ctypes.c_int32),
                ("youngs", ctypes.c_double), ("poisson", ctypes.c_double),
                ("thexpans", ctypes.c_double), ("inittemp", ctypes.c_double),
                ("conduct", ctypes.c_double),
                ("n_ele", ctypes.c_int64), ("n_node", ctypes.c_int64),
                ("n_rows_s", ctypes.c_int64), ("n_cols_s", ctypes.c_int64),
                ("n_rows_t", ctypes.c_int64), ("n_cols_t", ctypes.c_int64),
                ("ele_nodes", _i32p), ("ele_gid", _i32p), ("node_x", _dp),
                ("node_dof_col_s", _i32p), ("node_dof_row_s", _i32p),
                ("node_dof_col_t", _i32p), ("node_dof_row_t", _i32p),
                ("rowptr_st", _i64p), ("col_st", _i32p),
                ("rowptr_ts", _i64p), ("col_ts", _i32p),
                ("rowptr_tt", _i64p), ("col_tt", _i32p)]


# every symbol declared in include/fourc_gpu.h
class FcgAmgOptions(ctypes.Structure):
    """fcg_amg_options (include/fourc_gpu.h)."""
    _fields_ = [("nu", ctypes.c_int32), ("max_levels", ctypes.c_int32),
                ("coarse_max", ctypes.c_int64), ("coarse_max_iter", ctypes.c_int32),
                ("coarse_rtol", ctypes.c_double), ("omega", ctypes.c_double),
                ("ratio", ctypes.c_double), ("boost", ctypes.c_double)]


class FcgGmresOptions(ctypes.Structure):
    """fcg_gmres_options (include/fourc_gpu.h)."""
    _fields_ = [("restart", ctypes.c_int32), ("max_iter", ctypes.c_int32),
                ("rtol", ctypes.c_double), ("precond", ctypes.c_int32),
                ("reserved", ctypes.c_int32)]


EXPORTS = ["fcg_create", "fcg_destroy", "fcg_last_error", "fcg_evaluate", "fcg_evaluate_device",
           "fcg_device_alloc", "fcg_device_free", "fcg_memcpy_h2d", "fcg_memcpy_d2h",
           "fcg_memset_device", "fcg_set_timing", "fcg_get_timing", "fcg_get_info",
           "fcg_get_diagnostics", "fcg_get_create_phases", "fcg_measure_peaks", "fcg_measure_hbm", "fcg_spmv", "fcg_dirichlet_apply",
           "fcg_pcg_solve", "fcg_spmv_f32", "fcg_tangent_apply", "fcg_tangent_diag", "fcg_set_element_materials", "fcg_box_stencil_apply", "fcg_box_transfer", "fcg_block_jacobi_setup", "fcg_block_jacobi_apply", "fcg_chebyshev_step", "fcg_node_transfer",
           "fcg_neumann_surface", "fcg_neumann_volume",
           "fcg_graph_build_device", "fcg_get_graph",
           "fcg_tsi_create", "fcg_tsi_destroy", "fcg_tsi_last_error", "fcg_tsi_evaluate_device",
           "fcg_tsi_evaluate_fused", "fcg_tsi_capacity", "fcg_tsi_ost_combine",
           "fcg_tsi_surface_create", "fcg_tsi_surface_set", "fcg_tsi_surface_info", "fcg_tsi_surface_tables",
           "fcg_tsi_convection", "fcg_tsi_surface_flux", "fcg_tsi_surface_destroy",
           "fcg_box_mesh_create", "fcg_box_mesh_destroy", "fcg_box_mesh_desc", "fcg_box_mesh_maps",
           "fcg_box_mesh_counts", "fcg_box_mesh_create_ex", "fcg_box_mesh_owned_rows",
           "fcg_comm_unique_id", "fcg_comm_create", "fcg_comm_destroy", "fcg_comm_size", "fcg_comm_rank", "fcg_comm_allreduce",
           "fcg_comm_alltoallv", "fcg_import_plan_build", "fcg_plan_free", "fcg_halo_create",
           "fcg_halo_destroy", "fcg_halo_import", "fcg_halo_pack", "fcg_halo_unpack",
           "fcg_shared_plan_build", "fcg_shared_create", "fcg_shared_destroy", "fcg_shared_reduce",
           "fcg_shared_pack", "fcg_shared_unpack", "fcg_norm2", "fcg_set_async", "fcg_check_error",
           "fcg_evaluate_host",
           "fcg_amg_aggregate", "fcg_amg_tentative", "fcg_bsr_symbolic", "fcg_bsr_transpose_pattern",
           "fcg_bsr_spmv", "fcg_bsr_spgemm", "fcg_bsr_product_plan", "fcg_bsr_spgemm_planned", "fcg_bsr_transpose_values", "fcg_bsr_from_node_csr",
           "fcg_bsr_block_jacobi_setup", "fcg_bsr_block_jacobi_apply", "fcg_amg_smooth_prolongator",
           "fcg_bsr_to_dense", "fcg_amg_default_options", "fcg_amg_create", "fcg_amg_solve",
           "fcg_amg_levels", "fcg_amg_level_info", "fcg_amg_setup_ms", "fcg_amg_stats", "fcg_amg_last_error",
           "fcg_amg_destroy", "fcg_amg_setup", "fcg_amg_iterate", "fcg_amg_apply",
           "fcg_amg_level_matrix", "fcg_amg_level_order",
           "fcg_amg_coupled_levels", "fcg_amg_coupled_stats", "fcg_comm_exchange_device",
           "fcg_transport_rccl", "fcg_dfcg_solve",
           "fcg_mass_assemble", "fcg_mass_nodal", "fcg_effective_tangent",
           "fcg_gp_stress", "fcg_gp_to_nodes",
           "fcg_centrdiff_step", "fcg_stable_dt",
           "fcg_gmres_default_options", "fcg_gmres_solve", "fcg_gmres_set_timing",
           "fcg_gmres_get_timing", "fcg_gmres_orthogonalize_work", "fcg_gmres_orthogonalize",
           "fcg_tsi_block_apply", "fcg_tsi_dirichlet_apply", "fcg_tsi_gmres_solve",
           "fcg_samg_default_options", "fcg_samg_create", "fcg_samg_setup", "fcg_samg_apply",
           "fcg_samg_solve", "fcg_samg_levels", "fcg_samg_level_info", "fcg_samg_level_matrix",
           "fcg_samg_last_error", "fcg_samg_destroy", "fcg_samg_setup_ms", "fcg_tsi_gmres_solve_amg", "fcg_scsr_spmv",
           "fcg_scsr_chebyshev_step"]

_lib = None
FUNCT_FN = ctypes.CFUNCTYPE(ctypes.c_double, ctypes.c_int, _dp, ctypes.c_double, ctypes.c_void_p)


class FcgError(RuntimeError):
    def __init__(self, code, msg, bad_ele_gid=-1):
        super().__init__(f"{STATUS.get(code, code)}: {msg}")
        self.code = code
        self.bad_ele_gid = bad_ele_gid


def lib():
    """Load libfourc_gpu.so (built by `make -C 4c_amd`); raise if it is missing."""
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(LIB_PATH):
        raise ImportError(f"{LIB_PATH} not built: run `make -C 4c_amd` (no CPU fallback exists)")
    # One HIP runtime per process: when torch supplies the device buffers, its libamdhip64 must be
    # the one the library binds to, so torch is loaded first (same soname -> shared).
    try:
        import torch  # noqa: F401
    except ImportError:
        pass
    L = ctypes.CDLL(LIB_PATH)
    vp = ctypes.c_void_p
    L.fcg_create.argtypes = [ctypes.POINTER(FcgDesc), ctypes.POINTER(vp)]
    L.fcg_destroy.argtypes = [vp]
    L.fcg_last_error.argtypes = [vp]
    L.fcg_last_error.restype = ctypes.c_char_p
    L.fcg_evaluate.argtypes = [vp, ctypes.c_int, _dp, _dp, _dp, _i32p]
    L.fcg_evaluate_device.argtypes = [vp, ctypes.c_int, ctypes.c_int, vp, vp, vp, vp, _i32p]
    L.fcg_device_alloc.argtypes = [ctypes.c_int, ctypes.c_int64, ctypes.POINTER(vp)]
    L.fcg_device_free.argtypes = [vp]
    L.fcg_memcpy_h2d.argtypes = [vp, vp, ctypes.c_int64]
    L.fcg_memcpy_d2h.argtypes = [vp, vp, ctypes.c_int64]
    L.fcg_memset_device.argtypes = [vp, ctypes.c_int, ctypes.c_int64]
    L.fcg_set_timing.argtypes = [vp, ctypes.c_int]
    L.fcg_get_timing.argtypes = [vp, _dp, _dp]
    L.fcg_get_info.argtypes = [vp, ctypes.POINTER(FcgInfo)]
    L.fcg_get_diagnostics.argtypes = [vp, ctypes.POINTER(ctypes.c_uint64), ctypes.c_int]
    if hasattr(L, "fcg_get_create_phases"):  # absent from older A/B builds (FCG_LIB)
        L.fcg_get_create_phases.argtypes = [vp, ctypes.POINTER(ctypes.c_double), ctypes.c_int]
    if hasattr(L, "fcg_set_element_materials"):  # absent from older A/B builds (FCG_LIB)
        L.fcg_set_element_materials.argtypes = [vp, ctypes.c_int32, _dp, _dp, _i32p]
    L.fcg_spmv.argtypes = [vp, vp, vp, vp, vp]
    L.fcg_measure_peaks.argtypes = [ctypes.c_int, _dp, _dp, _dp]
    L.fcg_measure_hbm.argtypes = [ctypes.c_int, _dp, _dp]
    L.fcg_dirichlet_apply.argtypes = [vp, ctypes.c_int64, vp, vp, vp, vp, vp]
    L.fcg_pcg_solve.argtypes = [vp, vp, vp, vp, ctypes.c_double, ctypes.c_int,
                                ctypes.POINTER(ctypes.c_int), _dp, vp]
    L.fcg_spmv_f32.argtypes = [vp, vp, vp, vp, vp]
    L.fcg_tangent_apply.argtypes = [vp, vp, vp, vp, vp]
    L.fcg_tangent_diag.argtypes = [vp, vp, ctypes.c_int64, vp, vp, vp, vp]
    L.fcg_box_stencil_apply.argtypes = [ctypes.c_int, ctypes.c_int, ctypes.c_int, ctypes.c_int, vp, vp, vp, vp, vp, vp]
    L.fcg_box_transfer.argtypes = [ctypes.c_int] * 8 + [vp, vp, vp, vp, vp, ctypes.c_int, vp]
    L.fcg_block_jacobi_setup.argtypes = [vp, vp, vp, vp]
    L.fcg_block_jacobi_apply.argtypes = [vp, vp, vp, vp, ctypes.c_double, ctypes.c_int, vp]
    L.fcg_chebyshev_step.argtypes = [vp, vp, vp, vp, vp, vp, ctypes.c_double, ctypes.c_double, ctypes.c_int, vp]
    L.fcg_node_transfer.argtypes = [ctypes.c_int, ctypes.c_int64, vp, vp, vp, vp, vp, vp,
                                    ctypes.c_int, vp]
    neu = [ctypes.c_int, ctypes.c_int64, _i32p, _dp, _i32p, _i32p, _dp, _i32p, FUNCT_FN,
           ctypes.c_void_p, ctypes.c_double, _dp]
    L.fcg_neumann_surface.argtypes = neu
    L.fcg_neumann_volume.argtypes = neu
    L.fcg_box_mesh_create.argtypes = [ctypes.POINTER(FcgBox), ctypes.c_int, ctypes.c_int,
                                      ctypes.POINTER(vp)]
    L.fcg_box_mesh_destroy.argtypes = [vp]
    L.fcg_box_mesh_desc.argtypes = [vp, ctypes.c_int, ctypes.c_double, ctypes.c_double,
                                    ctypes.c_int, ctypes.POINTER(FcgDesc)]
    L.fcg_box_mesh_maps.argtypes = [vp, ctypes.POINTER(_i32p), ctypes.POINTER(_i32p),
                                    ctypes.POINTER(_i64p), ctypes.POINTER(_i32p)]
    L.fcg_box_mesh_counts.argtypes = [vp, _i64p, _i64p]
    L.fcg_box_mesh_create_ex.argtypes = [ctypes.POINTER(FcgBox), ctypes.c_int, ctypes.c_int,
                                         ctypes.c_int, ctypes.POINTER(vp)]
    L.fcg_box_mesh_owned_rows.argtypes = [vp, _i64p]
    L.fcg_comm_unique_id.argtypes = [vp]
    L.fcg_comm_create.argtypes = [vp, ctypes.c_int, ctypes.c_int, ctypes.c_int, ctypes.POINTER(vp)]
    L.fcg_comm_destroy.argtypes = [vp]
    L.fcg_comm_size.argtypes = [vp, ctypes.POINTER(ctypes.c_int)]
    L.fcg_comm_rank.argtypes = [vp, ctypes.POINTER(ctypes.c_int)]
    L.fcg_comm_allreduce.argtypes = [vp, vp, ctypes.c_int64, ctypes.c_int, vp]
    L.fcg_comm_alltoallv.argtypes = [vp, _i64p, vp, _i64p, ctypes.c_int64, vp]
    L.fcg_import_plan_build.argtypes = [ctypes.c_int, ctypes.c_int, ctypes.c_int64, _i32p,
                                        ctypes.c_int64, _i32p, _i32p, ALLTOALLV_FN, vp,
                                        ctypes.POINTER(FcgImportPlan), ctypes.POINTER(vp)]
    L.fcg_plan_free.argtypes = [vp]
    L.fcg_plan_free.restype = None
    L.fcg_halo_create.argtypes = [ctypes.POINTER(FcgImportPlan), ctypes.c_int, ctypes.POINTER(vp)]
    L.fcg_halo_destroy.argtypes = [vp]
    L.fcg_halo_import.argtypes = [vp, vp, vp, vp, vp]
    L.fcg_halo_pack.argtypes = [vp, vp, vp, vp, vp]
    L.fcg_halo_unpack.argtypes = [vp, vp, vp, vp]
    L.fcg_shared_plan_build.argtypes = [ctypes.c_int, ctypes.c_int, ctypes.c_int64, _i32p,
                                        ctypes.c_int64, _i32p, _i32p, ALLTOALLV_FN, vp,
                                        ctypes.POINTER(FcgSharedPlan), ctypes.POINTER(vp)]
    L.fcg_shared_create.argtypes = [ctypes.POINTER(FcgSharedPlan), ctypes.c_int, ctypes.POINTER(vp)]
    L.fcg_shared_destroy.argtypes = [vp]
    L.fcg_shared_reduce.argtypes = [vp, vp, vp, vp]
    L.fcg_shared_pack.argtypes = [vp, vp, vp, vp]
    L.fcg_shared_unpack.argtypes = [vp, vp, vp, vp]
    L.fcg_norm2.argtypes = [vp, vp, ctypes.c_int64, vp, _dp]
    L.fcg_set_async.argtypes = [vp, ctypes.c_int]
    L.fcg_check_error.argtypes = [vp, _i32p]
    L.fcg_evaluate_host.argtypes = [vp, ctypes.c_int, ctypes.c_int, _dp, _dp, _dp, _i32p]
    L.fcg_graph_build_device.argtypes = [ctypes.c_int, ctypes.c_int, ctypes.c_int64, vp,
                                         ctypes.c_int64, vp, vp, ctypes.c_int64, vp, vp,
                                         ctypes.c_int64, _i64p, vp]
    L.fcg_get_graph.argtypes = [vp, _i64p, _i32p, ctypes.c_int64, _i64p]
    L.fcg_tsi_create.argtypes = [ctypes.POINTER(FcgTsiDesc), ctypes.POINTER(vp)]
    L.fcg_tsi_destroy.argtypes = [vp]
    L.fcg_tsi_last_error.argtypes = [vp]
    L.fcg_tsi_last_error.restype = ctypes.c_char_p
    L.fcg_tsi_evaluate_device.argtypes = [vp, ctypes.c_int, ctypes.c_int, vp, vp, ctypes.c_double,
                                          ctypes.c_double, vp, vp, vp, vp, vp, vp, _i32p]
    L.fcg_tsi_evaluate_fused.argtypes = [vp, vp, ctypes.c_int, vp, vp, vp, ctypes.c_double,
                                         ctypes.c_double, vp, vp, vp, vp, vp, vp, vp, _i32p]
    L.fcg_tsi_capacity.argtypes = [vp, ctypes.c_double, _dp, ctypes.c_int, vp, vp, _i32p]
    L.fcg_tsi_ost_combine.argtypes = [vp, ctypes.c_double, ctypes.c_double, vp, vp, vp, vp, vp, vp, vp]
    L.fcg_tsi_surface_create.argtypes = [vp, ctypes.c_int64, _i32p, ctypes.POINTER(vp)]
    L.fcg_tsi_surface_set.argtypes = [vp, ctypes.c_double, _dp, ctypes.c_double, _dp, ctypes.c_double, _dp,
                                      _i64p]
    L.fcg_tsi_surface_info.argtypes = [vp, _i64p, _i64p, _i64p]
    L.fcg_tsi_surface_tables.argtypes = [vp] + [ctypes.POINTER(vp)] * 7
    L.fcg_tsi_convection.argtypes = [vp, ctypes.c_double, ctypes.c_double, vp, vp, vp, vp]
    L.fcg_tsi_surface_flux.argtypes = [vp, ctypes.c_double, vp, vp]
    L.fcg_tsi_surface_destroy.argtypes = [vp]
    i64, c_int, c_dbl = ctypes.c_int64, ctypes.c_int, ctypes.c_double
    L.fcg_amg_aggregate.argtypes = [i64, vp, vp, vp, vp]
    L.fcg_amg_aggregate.restype = i64
    L.fcg_amg_tentative.argtypes = [i64, c_int, vp, vp, i64, vp, vp, vp]
    L.fcg_bsr_symbolic.argtypes = [i64, vp, vp, vp, vp, i64, vp, vp]
    L.fcg_bsr_symbolic.restype = i64
    L.fcg_bsr_transpose_pattern.argtypes = [i64, i64, vp, vp, vp, vp, vp]
    L.fcg_bsr_spmv.argtypes = [c_int, c_int, c_int, i64, vp, vp, vp, vp, vp, c_dbl, c_int, vp]
    L.fcg_bsr_spgemm.argtypes = [c_int, c_int, c_int, c_int, i64, vp, vp, vp, vp, vp, vp, vp, vp,
                                 vp, vp]
    L.fcg_bsr_product_plan.argtypes = [i64, vp, vp, vp, vp, vp, vp, i64, vp, vp, vp]
    L.fcg_bsr_product_plan.restype = i64
    L.fcg_bsr_spgemm_planned.argtypes = [c_int, c_int, c_int, c_int, i64, vp, vp, vp, vp, vp, vp, vp, vp]
    L.fcg_bsr_transpose_values.argtypes = [c_int, c_int, c_int, i64, vp, vp, vp, vp]
    L.fcg_bsr_from_node_csr.argtypes = [c_int, i64, vp, vp, vp, vp, vp]
    L.fcg_bsr_block_jacobi_setup.argtypes = [c_int, c_int, i64, vp, vp, vp, vp, vp, vp]
    L.fcg_bsr_block_jacobi_apply.argtypes = [c_int, c_int, i64, vp, vp, vp, c_dbl, c_int, vp]
    L.fcg_amg_smooth_prolongator.argtypes = [c_int, c_int, i64, vp, vp, vp, vp, vp, vp, c_dbl, vp,
                                             vp]
    L.fcg_bsr_to_dense.argtypes = [c_int, c_int, i64, vp, vp, vp, vp, vp]
    L.fcg_amg_default_options.argtypes = [ctypes.POINTER(FcgAmgOptions)]
    L.fcg_amg_default_options.restype = None
    L.fcg_amg_create.argtypes = [vp, vp, vp, vp, i64, vp, ctypes.POINTER(FcgAmgOptions),
                                 ctypes.POINTER(vp)]
    L.fcg_amg_solve.argtypes = [vp, vp, vp, vp, c_dbl, c_int, ctypes.POINTER(c_int), _dp, vp]
    L.fcg_amg_setup.argtypes = [vp, vp, vp]
    L.fcg_amg_iterate.argtypes = [vp, vp, vp, vp, c_dbl, c_int, ctypes.POINTER(c_int), _dp, vp]
    L.fcg_amg_levels.argtypes = [vp]
    L.fcg_amg_level_info.argtypes = [vp, c_int, _i64p, _i64p, _dp]
    L.fcg_amg_setup_ms.argtypes = [vp]
    L.fcg_amg_setup_ms.restype = c_dbl
    L.fcg_amg_stats.argtypes = [vp, ctypes.POINTER(c_int), ctypes.POINTER(c_int)]
    L.fcg_amg_last_error.argtypes = [vp]
    L.fcg_amg_last_error.restype = ctypes.c_char_p
    L.fcg_amg_destroy.argtypes = [vp]
    L.fcg_amg_apply.argtypes = [vp, vp, vp, vp, vp]
    L.fcg_amg_level_matrix.argtypes = [vp, c_int, c_int, vp, vp, vp, i64]
    L.fcg_amg_level_matrix.restype = i64
    L.fcg_amg_level_order.argtypes = [vp, vp]
    L.fcg_amg_coupled_levels.argtypes = [vp]
    if hasattr(L, "fcg_amg_coupled_stats"):  # absent from older A/B builds (FCG_LIB)
        L.fcg_amg_coupled_stats.argtypes = [vp, ctypes.POINTER(ctypes.c_int64), c_int]
    L.fcg_transport_rccl.argtypes = [ctypes.POINTER(FcgRcclPair), ctypes.POINTER(FcgTransport)]
    L.fcg_dfcg_solve.argtypes = [vp, vp, ctypes.POINTER(FcgTransport), vp, vp, vp, c_dbl, c_int, vp,
                                 ctypes.POINTER(c_int), _dp]
    L.fcg_mass_assemble.argtypes = [vp, c_dbl, _dp, c_int, vp, vp]
    L.fcg_mass_nodal.argtypes = [vp, c_dbl, _dp, vp, vp, vp]
    L.fcg_effective_tangent.argtypes = [vp, c_dbl, c_dbl, vp, vp, vp, vp, vp]
    L.fcg_gp_stress.argtypes = [vp, c_int, c_int, vp, vp, vp, vp, vp, _i32p]
    L.fcg_gp_to_nodes.argtypes = [vp, vp, vp, vp]
    L.fcg_centrdiff_step.argtypes = [vp, c_dbl, c_dbl, c_dbl, vp, vp, vp, vp, vp, vp, vp, vp, vp, vp]
    L.fcg_stable_dt.argtypes = [vp, vp, vp, vp, _dp, _dp, vp]
    L.fcg_gmres_default_options.argtypes = [ctypes.POINTER(FcgGmresOptions)]
    L.fcg_gmres_default_options.restype = None
    L.fcg_gmres_solve.argtypes = [vp, vp, vp, vp, vp, ctypes.POINTER(FcgGmresOptions),
                                  ctypes.POINTER(c_int), _dp, vp]
    L.fcg_gmres_orthogonalize_work.argtypes = [i64, c_int]
    L.fcg_gmres_orthogonalize_work.restype = i64
    L.fcg_gmres_orthogonalize.argtypes = [c_int, i64, c_int, vp, i64, vp, vp, vp, vp]
    L.fcg_gmres_set_timing.argtypes = [c_int]
    L.fcg_gmres_get_timing.argtypes = [_dp, _dp, _dp, _i64p]
    L.fcg_tsi_block_apply.argtypes = [vp] * 11
    L.fcg_tsi_dirichlet_apply.argtypes = [vp, i64, vp, i64, vp, vp, vp, vp, vp, vp]
    L.fcg_tsi_gmres_solve.argtypes = [vp] * 11 + [ctypes.POINTER(FcgGmresOptions),
                                                  ctypes.POINTER(c_int), _dp, vp]
    L.fcg_samg_default_options.argtypes = [ctypes.POINTER(FcgAmgOptions)]
    L.fcg_samg_default_options.restype = None
    L.fcg_samg_create.argtypes = [vp, vp, vp, i64, vp, ctypes.POINTER(FcgAmgOptions), ctypes.POINTER(vp)]
    L.fcg_samg_setup.argtypes = [vp, vp, vp]
    L.fcg_samg_apply.argtypes = [vp, vp, vp, vp, vp]
    L.fcg_samg_solve.argtypes = [vp, vp, vp, vp, c_dbl, c_int, ctypes.POINTER(c_int), _dp, vp]
    L.fcg_samg_levels.argtypes = [vp]
    L.fcg_samg_level_info.argtypes = [vp, c_int, _i64p, _i64p, _dp]
    L.fcg_samg_level_matrix.argtypes = [vp, c_int, c_int, vp, vp, vp, i64]
    L.fcg_samg_level_matrix.restype = i64
    L.fcg_samg_last_error.argtypes = [vp]
    L.fcg_samg_last_error.restype = ctypes.c_char_p
    L.fcg_samg_destroy.argtypes = [vp]
    L.fcg_samg_setup_ms.argtypes = [vp, c_int]
    L.fcg_samg_setup_ms.restype = c_dbl
    L.fcg_tsi_gmres_solve_amg.argtypes = [vp] * 12 + [ctypes.POINTER(FcgGmresOptions),
                                                      ctypes.POINTER(c_int), _dp, vp]
    L.fcg_scsr_spmv.argtypes = [c_int, i64, i64, vp, vp, vp, vp, vp, vp, c_dbl, c_int, vp]
    L.fcg_scsr_chebyshev_step.argtypes = [c_int, i64, i64, vp, vp, vp, vp, vp, vp, vp, vp, c_dbl,
                                          c_dbl, c_int, vp]
    _lib = L
    return L


def _torch_stream(stream, device=None):
    """The HIP stream of a library call on torch tensors: the given torch stream, else torch's
    current stream of `device` (the context's device, not whichever device is current) -- never
    the context's own stream, which is not ordered with the torch work that produced or consumes
    the buffers."""
    import torch
    if stream is None:
        stream = torch.cuda.current_stream(device)
    return ctypes.c_void_p(stream.cuda_stream)


def _np_ptr(a, t):
    return a.ctypes.data_as(t)


def lattice_ijk(ele_nodes):
    """Element lattice positions (ex, ey, ez) of a hex8 mesh whose elements stack like a
    GridGenerator box: neighbours share whole faces in 4C node order (+x: nodes 1 2 6 5 of the
    element are 0 3 7 4 of the neighbour; +y: 3 2 6 7 -> 0 1 5 4; +z: 4 5 6 7 -> 0 1 2 3).
    Returns an int32 [n_ele][3] array (minimum 0), or None if the mesh is not such a lattice --
    the fcg_desc.ele_ijk hint, which fcg_create verifies again."""
    en = np.asarray(ele_nodes, dtype=np.int64).reshape(-1, 8)
    n = len(en)
    if n == 0:
        return None
    dirs = (((1, 2, 6, 5), (0, 3, 7, 4), (1, 0, 0)), ((3, 2, 6, 7), (0, 1, 5, 4), (0, 1, 0)),
            ((4, 5, 6, 7), (0, 1, 2, 3), (0, 0, 1)))
    maps = []
    for hi, lo, _ in dirs:
        mhi = {tuple(r): e for e, r in enumerate(en[:, list(hi)].tolist())}
        mlo = {tuple(r): e for e, r in enumerate(en[:, list(lo)].tolist())}
        maps.append((mhi, mlo))
    ijk = np.full((n, 3), np.iinfo(np.int64).min, dtype=np.int64)
    ijk[0] = 0
    stack = [0]
    while stack:
        e = stack.pop()
        for (hi, lo, off), (mhi, mlo) in zip(dirs, maps):
            for nb, sgn in ((mlo.get(tuple(en[e, list(hi)].tolist())), 1),
                            (mhi.get(tuple(en[e, list(lo)].tolist())), -1)):
                if nb is None:
                    continue
                want = ijk[e] + sgn * np.asarray(off)
                if ijk[nb, 0] == np.iinfo(np.int64).min:
                    ijk[nb] = want
                    stack.append(nb)
                elif not np.array_equal(ijk[nb], want):
                    return None
    if (ijk[:, 0] == np.iinfo(np.int64).min).any():
        return None
    ijk -= ijk.min(axis=0)
    if len(np.unique(ijk, axis=0)) != n or ijk.max() >= 2 ** 31:
        return None
    return np.ascontiguousarray(ijk, dtype=np.int32)


class Discretization:
    """Arrays of one rank's discretization as 4C holds them after FillComplete (the fcg_desc
    contents), for meshes that are not GridGenerator boxes -- e.g. the reference's input files."""

    def __init__(self, celltype, ele_nodes, node_x, node_dof_col, node_dof_row, rowptr, col_lid,
                 n_cols=None, ele_gid=None):
        self.celltype = celltype
        self.npe = 8 if celltype == HEX8 else 27
        self.ele_nodes = np.ascontiguousarray(ele_nodes, dtype=np.int32).reshape(-1, self.npe)
        self.node_x = np.ascontiguousarray(node_x, dtype=np.float64).reshape(-1, 3)
        self.node_dof_col = np.ascontiguousarray(node_dof_col, dtype=np.int32)
        self.node_dof_row = np.ascontiguousarray(node_dof_row, dtype=np.int32)
        self.rowptr = np.ascontiguousarray(rowptr, dtype=np.int64)
        self.col_lid = np.ascontiguousarray(col_lid, dtype=np.int32)
        self.ele_gid = (np.ascontiguousarray(ele_gid, dtype=np.int32) if ele_gid is not None
                        else np.arange(len(self.ele_nodes), dtype=np.int32))
        self.n_ele, self.n_node = len(self.ele_nodes), len(self.node_x)
        self.n_rows = len(self.rowptr) - 1
        self.n_cols = int(n_cols) if n_cols is not None else self.n_rows
        self.nnz = int(self.rowptr[-1])
        self.ele_ijk = None  # optional structured-lattice hint (lattice_ijk)

    @staticmethod
    def from_elements(celltype, ele_nodes, node_x, lattice=False):
        """Single-rank discretization: DOF LID = 3 * node + d, CSR graph of the element couplings.
        lattice=True attaches the structured-lattice hint (hex8 meshes stacked like a box)."""
        en = np.asarray(ele_nodes, dtype=np.int64)
        n_node = len(node_x)
        nbr = [set() for _ in range(n_node)]
        for el in en:
            for a in el:
                nbr[a].update(int(b) for b in el)
        rows, cols = [0], []
        for a in range(n_node):
            c = sorted(nbr[a])
            cd = [3 * b + d for b in c for d in range(3)]
            for _ in range(3):
                cols.extend(cd)
                rows.append(len(cols))
        dof = 3 * np.arange(n_node, dtype=np.int32)
        dis = Discretization(celltype, en, node_x, dof, dof, np.array(rows), np.array(cols))
        if lattice and celltype == HEX8:
            dis.ele_ijk = lattice_ijk(en)
        return dis

    def desc(self, kinematics, youngs, poisson, device=0, path=PATH_AUTO, material=MAT_STVK):
        d = FcgDesc()
        d.abi_version = ABI_VERSION
        d.celltype = self.celltype
        d.kinematics = kinematics
        d.device = device
        d.youngs = youngs
        d.poisson = poisson
        d.n_ele, d.n_node, d.n_rows, d.n_cols = self.n_ele, self.n_node, self.n_rows, self.n_cols
        d.ele_nodes = _np_ptr(self.ele_nodes, _i32p)
        d.ele_gid = _np_ptr(self.ele_gid, _i32p)
        d.node_x = _np_ptr(self.node_x, _dp)
        d.node_dof_col = _np_ptr(self.node_dof_col, _i32p)
        d.node_dof_row = _np_ptr(self.node_dof_row, _i32p)
        d.node_dof_kcol = None
        d.rowptr = _np_ptr(self.rowptr, _i64p)
        d.col_lid = _np_ptr(self.col_lid, _i32p)
        d.ele_ijk = (_np_ptr(self.ele_ijk, _i32p)
                     if self.ele_ijk is not None and path != PATH_GENERAL else None)
        d.path = path
        d.material = material
        return d

    @staticmethod
    def renumbered(box, seed=0):
        """A single-rank box mesh as an input-file mesh would arrive: random node and element
        numbering (DOF LID = 3 * node), no lattice hint; same geometry, graph and element
        orientation.  Vectorised, for benchmark-sized meshes."""
        assert box.n_rows == box.n_cols and np.array_equal(box.node_dof_col, 3 * np.arange(box.n_node))
        rng = np.random.default_rng(seed)
        nn = box.n_node
        perm = rng.permutation(nn)                 # new number of old node
        inv = np.argsort(perm)                     # old node of new number
        en = perm[box.ele_nodes][rng.permutation(box.n_ele)]
        X = np.empty_like(box.node_x)
        X[perm] = box.node_x
        rp = box.rowptr
        cnt = (rp[1::3][:nn] - rp[0::3][:nn]) // 3  # neighbour nodes of each old node
        cnt_new = cnt[inv]
        start = np.concatenate([[0], np.cumsum(cnt_new)])
        owner = np.repeat(np.arange(nn), cnt_new)
        k = np.arange(start[-1]) - start[owner]
        nb = perm[box.col_lid[rp[3 * inv[owner]] + 3 * k] // 3]
        nb = nb[np.lexsort((nb, owner))]
        rowlen = np.repeat(3 * cnt_new, 3)
        rowptr = np.concatenate([[0], np.cumsum(rowlen)]).astype(np.int64)
        row = np.repeat(np.arange(3 * nn), rowlen)
        off = np.arange(rowptr[-1]) - rowptr[row]
        col = (3 * nb[start[row // 3] + off // 3] + off % 3).astype(np.int32)
        dof = 3 * np.arange(nn, dtype=np.int32)
        dis = Discretization(box.celltype, en, X, dof, dof, rowptr, col)
        dis.node_perm = perm  # new number of every box node (DOF 3 * perm[old] + d)
        return dis


def _neumann(entry, celltype, conn, node_x, node_dof_row, onoff, val, funct, fn, time, fext):
    """fcg_neumann_surface / fcg_neumann_volume into the numpy vector `fext` (+=)."""
    conn = np.ascontiguousarray(conn, dtype=np.int32)
    node_x = np.ascontiguousarray(node_x, dtype=np.float64)
    node_dof_row = np.ascontiguousarray(node_dof_row, dtype=np.int32)
    oo = np.ascontiguousarray(onoff, dtype=np.int32)
    vv = np.ascontiguousarray(val, dtype=np.float64)
    ff = np.ascontiguousarray(funct if funct is not None else [0, 0, 0], dtype=np.int32)
    err = []

    def cb(fid, x, t, _user):
        try:
            return float(fn(fid, (x[0], x[1], x[2]), t))
        except Exception as e:  # surfaced after the call
            err.append(e)
            return 0.0

    cfn = FUNCT_FN(cb) if fn is not None else FUNCT_FN()
    n = conn.shape[0]
    rc = getattr(lib(), entry)(celltype, n, _np_ptr(conn, _i32p), _np_ptr(node_x, _dp),
                               _np_ptr(node_dof_row, _i32p), _np_ptr(oo, _i32p), _np_ptr(vv, _dp),
                               _np_ptr(ff, _i32p), cfn, None, float(time), _np_ptr(fext, _dp))
    if err:
        raise err[0]
    if rc != 0:
        raise FcgError(rc, entry + " failed")


def neumann_surface(celltype, face_nodes, node_x, node_dof_row, onoff, val, fext, funct=None,
                    fn=None, time=1.0):
    _neumann("fcg_neumann_surface", celltype, face_nodes, node_x, node_dof_row, onoff, val, funct,
             fn, time, fext)


def neumann_volume(celltype, ele_nodes, node_x, node_dof_row, onoff, val, fext, funct=None,
                   fn=None, time=1.0):
    _neumann("fcg_neumann_volume", celltype, ele_nodes, node_x, node_dof_row, onoff, val, funct,
             fn, time, fext)


def _tensor_ptr(t):
    return ctypes.c_void_p(t.data_ptr()) if t is not None else None


class _NativeBoxMesh:
    """Owner of an fcg_box_mesh: destroyed when the last numpy view of its arrays goes."""

    def __init__(self, h):
        self.h = h

    def __del__(self):
        if self.h:
            try:
                lib().fcg_box_mesh_destroy(self.h)
            except Exception:  # noqa: BLE001 - interpreter shutdown: the process frees it anyway
                pass
            self.h = None


class BoxMesh:
    """One rank of a GridGenerator box (the fcg_box_mesh_* builder), as numpy views."""

    def __init__(self, celltype, interval, lower=(0.0, 0.0, 0.0), upper=(1.0, 1.0, 1.0),
                 rotation=(0.0, 0.0, 0.0), first_node_gid=0, jitter=0.0, seed=20251015,
                 rank=0, nranks=1, strict=False):
        """strict=True: FCG_BOX_STRICT (row elements only, extended rows for the non-owned
        nodes they touch after the n_owned_rows owned rows)."""
        L = lib()
        box = FcgBox()
        box.celltype = celltype
        for d in range(3):
            box.interval[d] = int(interval[d])
            box.lower[d] = float(lower[d])
            box.upper[d] = float(upper[d])
            box.rotation[d] = float(rotation[d])
        box.first_node_gid = int(first_node_gid)
        box.jitter = float(jitter)
        box.jitter_seed = int(seed)
        self.box = box
        self.celltype = celltype
        self.npe = 8 if celltype == HEX8 else 27
        self.rank, self.nranks = rank, nranks
        self.strict = bool(strict)
        h = ctypes.c_void_p()
        rc = L.fcg_box_mesh_create_ex(ctypes.byref(box), rank, nranks,
                                      BOX_STRICT if strict else BOX_GHOSTED, ctypes.byref(h))
        if rc != 0:
            raise FcgError(rc, "fcg_box_mesh_create failed")
        self._h = h
        d = FcgDesc()
        L.fcg_box_mesh_desc(h, LINEAR, 1.0, 0.0, 0, ctypes.byref(d))
        self.n_ele, self.n_node = d.n_ele, d.n_node
        self.n_rows, self.n_cols = d.n_rows, d.n_cols

        # zero-copy views of the builder's arrays; the native mesh is released when the last
        # view is (a 1M-hex27 box holds 18.5 GB of column indices: no second copy)
        keeper = _NativeBoxMesh(h)
        ctype_of = {np.int32: ctypes.c_int32, np.int64: ctypes.c_int64, np.float64: ctypes.c_double}

        def view(p, n, dt):
            if n == 0:
                return np.zeros(0, dtype=dt)
            buf = (ctype_of[dt] * n).from_address(ctypes.cast(p, ctypes.c_void_p).value)
            buf._keep = keeper
            return np.frombuffer(buf, dtype=dt)

        self.ele_nodes = view(d.ele_nodes, d.n_ele * self.npe, np.int32).reshape(-1, self.npe)
        self.ele_gid = view(d.ele_gid, d.n_ele, np.int32)
        self.ele_ijk = view(d.ele_ijk, d.n_ele * 3, np.int32).reshape(-1, 3)
        self.node_x = view(d.node_x, d.n_node * 3, np.float64).reshape(-1, 3)
        self.node_dof_col = view(d.node_dof_col, d.n_node, np.int32)
        self.node_dof_row = view(d.node_dof_row, d.n_node, np.int32)
        self.rowptr = view(d.rowptr, d.n_rows + 1, np.int64)
        self.nnz = int(self.rowptr[-1]) if d.n_rows else 0
        self.col_lid = view(d.col_lid, self.nnz, np.int32)
        rg, cg, ng, no = _i32p(), _i32p(), _i64p(), _i32p()
        L.fcg_box_mesh_maps(h, ctypes.byref(rg), ctypes.byref(cg), ctypes.byref(ng), ctypes.byref(no))
        self.row_gid = view(rg, d.n_rows, np.int32)
        self.col_gid = view(cg, d.n_cols, np.int32)
        self.node_gid = view(ng, d.n_node, np.int64)
        self.node_owner = view(no, d.n_node, np.int32)
        ng_, nr_ = ctypes.c_int64(), ctypes.c_int64()
        L.fcg_box_mesh_counts(h, ctypes.byref(ng_), ctypes.byref(nr_))
        self.n_ele_global, self.n_ele_row = ng_.value, nr_.value
        no_ = ctypes.c_int64()
        L.fcg_box_mesh_owned_rows(h, ctypes.byref(no_))
        self.n_owned_rows = no_.value
        self._h = None  # owned by the views' keeper

    def desc(self, kinematics, youngs, poisson, device=0, path=PATH_AUTO, material=MAT_STVK):
        d = FcgDesc()
        d.abi_version = ABI_VERSION
        d.celltype = self.celltype
        d.kinematics = kinematics
        d.device = device
        d.youngs = youngs
        d.poisson = poisson
        d.n_ele, d.n_node, d.n_rows, d.n_cols = self.n_ele, self.n_node, self.n_rows, self.n_cols
        d.ele_nodes = _np_ptr(self.ele_nodes, _i32p)
        d.ele_gid = _np_ptr(self.ele_gid, _i32p)
        d.node_x = _np_ptr(self.node_x, _dp)
        d.node_dof_col = _np_ptr(self.node_dof_col, _i32p)
        d.node_dof_row = _np_ptr(self.node_dof_row, _i32p)
        d.node_dof_kcol = None
        d.rowptr = _np_ptr(self.rowptr, _i64p)
        d.col_lid = _np_ptr(self.col_lid, _i32p)
        d.ele_ijk = _np_ptr(self.ele_ijk, _i32p) if path != PATH_GENERAL else None
        d.path = path
        d.material = material
        return d

    def node_displacement(self, amplitude):
        """Synthetic state u(X) = A (sin2piX cospiY, sinpiY cos2piZ, sin2piZ cospiX)."""
        X = self.node_x
        u = np.empty_like(X)
        u[:, 0] = np.sin(2 * np.pi * X[:, 0]) * np.cos(np.pi * X[:, 1])
        u[:, 1] = np.sin(np.pi * X[:, 1]) * np.cos(2 * np.pi * X[:, 2])
        u[:, 2] = np.sin(2 * np.pi * X[:, 2]) * np.cos(np.pi * X[:, 0])
        return amplitude * u

    def u_col(self, amplitude):
        u = np.zeros(self.n_cols)
        un = self.node_displacement(amplitude)
        for d in range(3):
            u[self.node_dof_col + d] = un[:, d]
        return u


class Evaluator:
    """Device context (fcg_ctx): the MI355X replacement of Discretization::evaluate for SOLID
    hex8/hex27 with material=MAT_STVK or MAT_ELASTHYPER_COUPNEOHOOKE (TOTLAG only).  path:
    PATH_AUTO picks the sweep / gather / general path (hex8 CoupNeoHooke: PATH_GENERAL);
    PATH_GATHER requests the node-row gather, hex8 with either material.  Keeps 4C's error
    behaviour: a non-zero status raises FcgError."""

    def __init__(self, desc_or_mesh, kinematics=LINEAR, youngs=210.0, poisson=0.3, device=0,
                 path=PATH_AUTO, material=MAT_STVK):
        L = lib()
        if isinstance(desc_or_mesh, (BoxMesh, Discretization)):
            self._mesh = desc_or_mesh
            desc = desc_or_mesh.desc(kinematics, youngs, poisson, device, path, material)
        else:
            self._mesh = None
            desc = desc_or_mesh
        self.device = desc.device
        self.kinematics = int(desc.kinematics)
        self.ngp = 8 if int(desc.celltype) == HEX8 else 27  # the stiffness rule's Gauss points
        h = ctypes.c_void_p()
        rc = L.fcg_create(ctypes.byref(desc), ctypes.byref(h))
        if rc != 0:
            raise FcgError(rc, L.fcg_last_error(None).decode())
        self._h = h
        info = FcgInfo()
        L.fcg_get_info(h, ctypes.byref(info))
        self.info = info
        self._n_materials = 0
        self._async = False

    @property
    def n_materials(self):
        """Entries of the per-element material table in force (0: the uniform material)."""
        return self._n_materials

    def set_element_materials(self, youngs, poisson=None, ele_mat=None):
        """fcg_set_element_materials: element e (column-element order) takes youngs[ele_mat[e]],
        poisson[ele_mat[e]] of the context's material kind; set_element_materials(None) returns to
        the uniform material.  Honoured on PATH_GATHER (hex8, both materials) / PATH_GENERAL
        (evaluate, tangent_apply, tangent_diag); a PATH_STRUCTURED / PATH_COLORED context raises FcgError (code 3), as do
        parameters outside the ranges of fcg_create -- the context then stays as it was.  Waits for
        the context's stream; not to be called while evaluates run on other streams."""
        L = lib()
        if youngs is None:
            rc = L.fcg_set_element_materials(self._h, 0, None, None, None)
            n = 0
        else:
            E = np.ascontiguousarray(youngs, dtype=np.float64).ravel()
            nu = None if poisson is None else np.ascontiguousarray(poisson, dtype=np.float64).ravel()
            em = None if ele_mat is None else np.ascontiguousarray(ele_mat, dtype=np.int32).ravel()
            if nu is not None and nu.size != E.size:
                raise ValueError("youngs and poisson differ in length")
            if em is not None and em.size != self.info.n_ele:
                raise ValueError(f"ele_mat has {em.size} entries, the context {self.info.n_ele} elements")
            n = int(E.size)
            rc = L.fcg_set_element_materials(
                self._h, n, _np_ptr(E, _dp), _np_ptr(nu, _dp) if nu is not None else None,
                _np_ptr(em, _i32p) if em is not None else None)
        if rc != 0:
            self._raise(rc, -1)
        self._n_materials = n
        L.fcg_get_info(self._h, ctypes.byref(self.info))  # device_bytes counts the table

    def graph(self):
        """fcg_get_graph: (rowptr int64, col_lid int32) host copies of the context's CSR graph --
        the device-built one when the descriptor came without rowptr / col_lid."""
        L = lib()
        nnz = ctypes.c_int64(0)
        rc = L.fcg_get_graph(self._h, None, None, 0, ctypes.byref(nnz))
        if rc != 0:
            self._raise(rc, -1)
        rowptr = np.empty(self.info.n_rows + 1, dtype=np.int64)
        col = np.empty(max(nnz.value, 1), dtype=np.int32)
        rc = L.fcg_get_graph(self._h, _np_ptr(rowptr, _i64p), _np_ptr(col, _i32p), nnz.value,
                             ctypes.byref(nnz))
        if rc != 0:
            self._raise(rc, -1)
        return rowptr, col[:nnz.value]

    def close(self):
        if getattr(self, "_h", None):
            lib().fcg_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def _raise(self, rc, bad):
        raise FcgError(rc, lib().fcg_last_error(self._h).decode(), bad)

    def evaluate(self, action, u_col, fint_row, K_vals=None):
        """Host-pointer path (blocking, `+=` semantics like SparseMatrix::assemble)."""
        bad = ctypes.c_int32(-1)
        rc = lib().fcg_evaluate(self._h, action, _np_ptr(u_col, _dp), _np_ptr(fint_row, _dp),
                                _np_ptr(K_vals, _dp) if K_vals is not None else None,
                                ctypes.byref(bad))
        if rc != 0:
            self._raise(rc, bad.value)

    def evaluate_host(self, action, mode, u_col, fint_row, K_vals=None):
        """fcg_evaluate_host: host (numpy) buffers; mode OVERWRITE fuses the caller's zero()."""
        bad = ctypes.c_int32(-1)
        rc = lib().fcg_evaluate_host(self._h, action, mode, _np_ptr(u_col, _dp),
                                     _np_ptr(fint_row, _dp),
                                     _np_ptr(K_vals, _dp) if K_vals is not None else None,
                                     ctypes.byref(bad))
        if rc != 0:
            self._raise(rc, bad.value)

    def set_async(self, enable):
        """fcg_set_async: evaluate_device returns once queued; check_error reports failures."""
        rc = lib().fcg_set_async(self._h, 1 if enable else 0)
        self._async = bool(enable) and rc == 0  # a failed call leaves the context synchronous
        if rc != 0:
            self._raise(rc, -1)

    @property
    def async_enabled(self):
        """The setting of the last set_async (contexts start synchronous)."""
        return self._async

    def check_error(self):
        bad = ctypes.c_int32(-1)
        rc = lib().fcg_check_error(self._h, ctypes.byref(bad))
        if rc != 0:
            self._raise(rc, bad.value)

    def evaluate_device(self, action, mode, u_col, fint_row, K_vals=None, stream=None):
        """Device-resident path; tensors are float64 torch tensors on this device."""
        bad = ctypes.c_int32(-1)
        s = _torch_stream(stream, self.device)
        rc = lib().fcg_evaluate_device(self._h, action, mode, _tensor_ptr(u_col),
                                       _tensor_ptr(fint_row), _tensor_ptr(K_vals), s,
                                       ctypes.byref(bad))
        if rc != 0:
            self._raise(rc, bad.value)

    def _stream(self, stream):
        return _torch_stream(stream, self.device)

    def spmv(self, K_vals, x_col, y_row, stream=None):
        rc = lib().fcg_spmv(self._h, _tensor_ptr(K_vals), _tensor_ptr(x_col), _tensor_ptr(y_row),
                            self._stream(stream))
        if rc != 0:
            self._raise(rc, -1)

    def spmv_f32(self, K32, x_col, y_row, stream=None):
        """y = K x with an FP32 copy of the matrix values (asynchronous)."""
        rc = lib().fcg_spmv_f32(self._h, _tensor_ptr(K32), _tensor_ptr(x_col), _tensor_ptr(y_row),
                                self._stream(stream))
        if rc != 0:
            self._raise(rc, -1)

    def tangent_apply(self, u_col, x_col, y_row, stream=None):
        """y = K(u) x without a matrix (fcg_tangent_apply; hex27 StVK): the tangent the evaluate
        assembles at u, before Dirichlet rows, applied element by element (asynchronous).  u_col
        may be None for linear kinematics."""
        rc = lib().fcg_tangent_apply(self._h, _tensor_ptr(u_col), _tensor_ptr(x_col),
                                     _tensor_ptr(y_row), self._stream(stream))
        if rc != 0:
            self._raise(rc, -1)

    def tangent_diag(self, u_col, dbc_rows=None, diag=None, dinv=None, stream=None):
        """The 3 x 3 nodal diagonal blocks of K(u) without a matrix (fcg_tangent_diag; hex27 StVK):
        `diag` receives the blocks, `dinv` their inverses, 9 doubles per owned node, row-major, in
        the order of fcg_block_jacobi_setup's blocks; either may be None, not both.  dbc_rows
        (int32 device tensor): rows replaced by unit rows, as dirichlet_apply does to K.  u_col
        may be None for linear kinematics.  With dinv the call waits for the stream and raises for
        a singular block; with diag only it is asynchronous."""
        n_dbc = 0 if dbc_rows is None else int(dbc_rows.numel())
        rc = lib().fcg_tangent_diag(self._h, _tensor_ptr(u_col), n_dbc,
                                    _tensor_ptr(dbc_rows) if n_dbc else None, _tensor_ptr(diag),
                                    _tensor_ptr(dinv), self._stream(stream))
        if rc != 0:
            self._raise(rc, -1)

    def dirichlet_apply(self, rows, K_vals=None, rhs=None, freact=None, stream=None):
        """rows: int32 device tensor of DBC row LIDs."""
        rc = lib().fcg_dirichlet_apply(self._h, int(rows.numel()), _tensor_ptr(rows),
                                       _tensor_ptr(K_vals), _tensor_ptr(rhs), _tensor_ptr(freact),
                                       self._stream(stream))
        if rc != 0:
            self._raise(rc, -1)

    def pcg_solve(self, K_vals, b, x, rtol=1e-12, max_iter=10000, stream=None):
        """K x = b (block-Jacobi PCG from x = 0); returns (iterations, relative residual)."""
        it, rr = ctypes.c_int(0), ctypes.c_double(0.0)
        rc = lib().fcg_pcg_solve(self._h, _tensor_ptr(K_vals), _tensor_ptr(b), _tensor_ptr(x),
                                 float(rtol), int(max_iter), ctypes.byref(it), ctypes.byref(rr),
                                 self._stream(stream))
        if rc != 0:
            self._raise(rc, -1)
        return it.value, rr.value

    def gmres_solve(self, K_vals, b, x, rtol=1e-10, max_iter=10000, restart=50, amg=None,
                    stream=None):
        """K x = b for any values on the context's graph (symmetry is not assumed) by restarted
        flexible GMRES from x = 0 (fcg_gmres_solve); the preconditioner is the nodal block Jacobi,
        or one cycle of `amg` (an amg.NativeAMG whose setup(K) the caller has run).  Returns
        (inner steps taken, true relative residual)."""
        opt = gmres_options(restart, max_iter, rtol)
        it, rr = ctypes.c_int(0), ctypes.c_double(0.0)
        rc = lib().fcg_gmres_solve(self._h, amg._h if amg is not None else None,
                                   _tensor_ptr(K_vals), _tensor_ptr(b), _tensor_ptr(x),
                                   ctypes.byref(opt), ctypes.byref(it), ctypes.byref(rr),
                                   self._stream(stream))
        if rc != 0:
            self._raise(rc, -1)
        return it.value, rr.value

    def _ele_density(self, ele_density):
        if ele_density is None:
            return None, None
        rho = np.ascontiguousarray(ele_density, dtype=np.float64).ravel()
        if rho.size != self.info.n_ele:
            raise ValueError(f"ele_density has {rho.size} entries, the context {self.info.n_ele} elements")
        return rho, _np_ptr(rho, _dp)

    def _f64(self, n):
        import torch
        return torch.empty(int(n), dtype=torch.float64, device=torch.device("cuda", self.device))

    def mass(self, density, ele_density=None, mode=OVERWRITE, out=None, stream=None):
        """fcg_mass_assemble: the consistent mass on the context's CSR graph (4C's systemmatrix2 of
        struct_calc_nlnstiffmass) into `out` ([nnz] device tensor; None: a new one, which
        ACCUMULATE starts from zeros).  ele_density: one density per column element (host array),
        `density` is then ignored.  Returns the tensor; the call waits for the stream."""
        if out is None:
            out = self._f64(self.info.nnz)
            if mode == ACCUMULATE:
                out.zero_()
        rho, rp = self._ele_density(ele_density)
        rc = lib().fcg_mass_assemble(self._h, float(density), rp, int(mode), _tensor_ptr(out),
                                     self._stream(stream))
        if rc != 0:
            self._raise(rc, -1)
        lib().fcg_get_info(self._h, ctypes.byref(self.info))  # device_bytes counts the mass plan
        return out

    def mass_nodal(self, density, ele_density=None, m_node=None, m_lumped=None, stream=None):
        """fcg_mass_nodal: the compact node form ([nnz / 9], one double per row node and neighbour
        node) and the row-sum lumped mass ([n_rows]).  With both None both are allocated; returns
        (m_node, m_lumped), None for a form not asked for.  Waits for the stream."""
        if m_node is None and m_lumped is None:
            m_node, m_lumped = self._f64(self.info.nnz // 9), self._f64(self.info.n_rows)
        rho, rp = self._ele_density(ele_density)
        rc = lib().fcg_mass_nodal(self._h, float(density), rp, _tensor_ptr(m_node),
                                  _tensor_ptr(m_lumped), self._stream(stream))
        if rc != 0:
            self._raise(rc, -1)
        lib().fcg_get_info(self._h, ctypes.byref(self.info))
        return m_node, m_lumped

    def effective_tangent(self, cK, cM, m_node, K_vals=None, x_col=None, y_row=None, stream=None):
        """fcg_effective_tangent: K_vals <- cK K_vals + cM M in place (cK == 0: K_vals is not read)
        and, with x_col and y_row, y_row = M x_col in the same pass; m_node from mass_nodal.
        Asynchronous."""
        rc = lib().fcg_effective_tangent(self._h, float(cK), float(cM), _tensor_ptr(m_node),
                                         _tensor_ptr(K_vals), _tensor_ptr(x_col), _tensor_ptr(y_row),
                                         self._stream(stream))
        if rc != 0:
            self._raise(rc, -1)

    def gp_stress_raw(self, stress_type, strain_type, u_col, stress=None, strain=None, energy=None,
                      stream=None):
        """fcg_gp_stress on the caller's buffers (device tensors or None), unchecked: the C entry
        point's own argument rules apply.  Waits for the stream."""
        bad = ctypes.c_int32(-1)
        rc = lib().fcg_gp_stress(self._h, int(stress_type), int(strain_type), _tensor_ptr(u_col),
                                 _tensor_ptr(stress), _tensor_ptr(strain), _tensor_ptr(energy),
                                 self._stream(stream), ctypes.byref(bad))
        if rc != 0:
            self._raise(rc, bad.value)
        lib().fcg_get_info(self._h, ctypes.byref(self.info))  # device_bytes counts the tables

    def gp_stress(self, u_col, stress=STRESS_PK2, strain=STRAIN_GL, energy=False, stream=None):
        """fcg_gp_stress (4C's struct_calc_stress / struct_calc_energy): the stresses and strains
        at the Gauss points of every column element, [n_ele, ngp, 6] in Voigt order
        xx yy zz xy yz xz (strains as tensor components), and with energy=True the elements' strain
        energies [n_ele].  stress: STRESS_NONE / STRESS_PK2 / STRESS_CAUCHY, strain: STRAIN_NONE /
        STRAIN_GL / STRAIN_EA.  Returns the tensors asked for, in the order stress, strain, energy
        (one tensor when only one is asked for).  u_col may be None for linear kinematics."""
        ngp, n_ele = self.ngp, int(self.info.n_ele)
        s = self._f64(n_ele * ngp * 6).view(n_ele, ngp, 6) if stress != STRESS_NONE else None
        e = self._f64(n_ele * ngp * 6).view(n_ele, ngp, 6) if strain != STRAIN_NONE else None
        w = self._f64(n_ele) if energy else None
        self.gp_stress_raw(stress, strain, u_col, s, e, w, stream)
        out = tuple(t for t in (s, e, w) if t is not None)
        return out[0] if len(out) == 1 else out

    def strain_energy(self, u_col, stream=None):
        """The elements' strain energies sum_g w_g det J_g psi(E_g), [n_ele] (struct_calc_energy)."""
        return self.gp_stress(u_col, STRESS_NONE, STRAIN_NONE, True, stream)

    def gp_to_nodes(self, gp, out=None, stream=None):
        """fcg_gp_to_nodes: Gauss-point data [n_ele, ngp, 6] extrapolated to the element nodes and
        averaged over each node's elements, [n_node, 6] by column node.  Rows of nodes without an
        owned row are not written: a fresh `out` is filled with NaN there.  Asynchronous."""
        import torch
        ngp = self.ngp
        if gp.dtype != torch.float64 or gp.numel() != int(self.info.n_ele) * ngp * 6:
            raise ValueError(f"gp must be float64 [{self.info.n_ele}, {ngp}, 6]")
        gp = gp.contiguous()
        if out is None:
            out = torch.full((int(self.info.n_node), 6), float("nan"), dtype=torch.float64,
                             device=gp.device)
        rc = lib().fcg_gp_to_nodes(self._h, _tensor_ptr(gp), _tensor_ptr(out), self._stream(stream))
        if rc != 0:
            self._raise(rc, -1)
        lib().fcg_get_info(self._h, ctypes.byref(self.info))
        return out

    def centrdiff_step(self, dt_prev, dt_next, damp_m, fext, fint, m_lumped, fixed, d, vhalf,
                       v=None, a=None, ekin=None, stream=None):
        """fcg_centrdiff_step: one central-difference update over the owned rows.  On entry d =
        d_{n+1}, vhalf = v_{n+1/2}, fint = f_int(d), fext = f_ext(t_{n+1}); d and vhalf advance in
        place to d_{n+2} and v_{n+3/2}, v and a (optional) receive v_{n+1} and a_{n+1}, ekin (one
        double, optional) 1/2 sum m v^2.  fixed: uint8 device tensor, != 0 marks a Dirichlet row,
        or None.  All float64 device tensors [n_rows].  Asynchronous."""
        rc = lib().fcg_centrdiff_step(self._h, float(dt_prev), float(dt_next), float(damp_m),
                                      _tensor_ptr(fext), _tensor_ptr(fint), _tensor_ptr(m_lumped),
                                      _tensor_ptr(fixed), _tensor_ptr(d), _tensor_ptr(vhalf),
                                      _tensor_ptr(v), _tensor_ptr(a), _tensor_ptr(ekin),
                                      self._stream(stream))
        if rc != 0:
            self._raise(rc, -1)
        if ekin is not None:
            lib().fcg_get_info(self._h, ctypes.byref(self.info))  # device_bytes counts the partials

    def stable_dt(self, K_vals, m_lumped, fixed=None, stream=None):
        """fcg_stable_dt: (dt_crit, lambda_bound) with lambda_bound = max over the free rows of
        sum_j |K_ij| / m_i (Gershgorin) and dt_crit = 2 / sqrt(lambda_bound), never above the
        central-difference limit 2 / omega_max.  This rank's rows only.  Waits for the stream."""
        lam, dt = ctypes.c_double(0.0), ctypes.c_double(0.0)
        rc = lib().fcg_stable_dt(self._h, _tensor_ptr(K_vals), _tensor_ptr(m_lumped),
                                 _tensor_ptr(fixed), ctypes.byref(lam), ctypes.byref(dt),
                                 self._stream(stream))
        if rc != 0:
            self._raise(rc, -1)
        lib().fcg_get_info(self._h, ctypes.byref(self.info))
        return dt.value, lam.value

    def set_timing(self, enable):
        lib().fcg_set_timing(self._h, 1 if enable else 0)

    def diagnostics(self):
        """Per-phase cycle counters of the fused kernel (FCG_STAMPS=1 at creation), or None."""
        buf = (ctypes.c_uint64 * 16)()
        n = lib().fcg_get_diagnostics(self._h, buf, 16)
        return list(buf) if n > 0 else None

    SWEEP_KERNELS = ("not applicable", "checked", "unchecked")

    def sweep_kernel(self):
        """Which kernels the structured sweep of this context launches (slot 15 of
        fcg_get_diagnostics): "unchecked" when fcg_create's geometry pass found nothing to reject,
        "checked" when it did or FCG_SWEEP_CHECKED=1 was set at creation, "not applicable" on
        the other paths."""
        buf = (ctypes.c_uint64 * 16)()
        lib().fcg_get_diagnostics(self._h, buf, 16)
        return self.SWEEP_KERNELS[int(buf[15])]

    SWEEP_ROWS = ("not applicable", "direct", "deferred")

    def sweep_rows(self):
        """How the structured sweep's tangent kernels write a row (slot 12 of
        fcg_get_diagnostics): "direct" -- the blocks with the plane below in the layer that
        finishes them, the rest one layer later -- or "deferred": the whole row within one layer
        (rows not in lattice order, or FCG_SWEEP_DEFER=1 at creation); "not applicable" on the
        other paths."""
        buf = (ctypes.c_uint64 * 16)()
        lib().fcg_get_diagnostics(self._h, buf, 16)
        return self.SWEEP_ROWS[int(buf[12])]

    def sweep_regular_layers(self):
        """(regular, total): the (tile, layer) pairs of the structured sweep that take the
        regular-tile path -- closed-form row bookkeeping, decided at fcg_create -- and all of them
        (slots 13, 14 of fcg_get_diagnostics).  regular is 0 for a context whose kernels keep
        the plane records (TotLag, rows in no arithmetic progression, the checked kernels) and with
        FCG_SWEEP_REGULAR=0 at creation; (0, 0) on the other paths."""
        buf = (ctypes.c_uint64 * 16)()
        lib().fcg_get_diagnostics(self._h, buf, 16)
        return int(buf[13]), int(buf[14])

    CREATE_PHASES = ("checks", "graph_device", "node_rows", "lattice_plans", "incidences",
                     "incidence_positions", "device_plans", "total")

    def create_phases(self):
        """fcg_create's phase wall times (s) by name (fcg_get_create_phases)."""
        buf = (ctypes.c_double * 8)()
        lib().fcg_get_create_phases(self._h, buf, 8)
        return dict(zip(self.CREATE_PHASES, list(buf)))

    def timing(self):
        a, b = ctypes.c_double(), ctypes.c_double()
        lib().fcg_get_timing(self._h, ctypes.byref(a), ctypes.byref(b))
        return a.value, b.value


def gmres_options(restart=None, max_iter=None, rtol=None, precond=None):
    """fcg_gmres_options: the library's defaults with the given fields replaced."""
    opt = FcgGmresOptions()
    lib().fcg_gmres_default_options(ctypes.byref(opt))
    for k, v in (("restart", restart), ("max_iter", max_iter), ("precond", precond)):
        if v is not None:
            setattr(opt, k, int(v))
    if rtol is not None:
        opt.rtol = float(rtol)
    return opt


def gmres_orthogonalize(V, w, h, work=None, stream=None):
    """fcg_gmres_orthogonalize on torch tensors: V [nv][ld] float64 (ld even, rows are the basis
    vectors, n = w.numel() <= ld), w [n] orthogonalised in place against them, h [nv + 1] the
    coefficients and |w|.  work: a float64 tensor of gmres_orthogonalize_work(n, nv) doubles
    (allocated when None).  Asynchronous."""
    import torch
    nv, ld, n = int(V.shape[0]), int(V.shape[1]), int(w.numel())
    if work is None:
        work = torch.empty(gmres_orthogonalize_work(n, nv), dtype=torch.float64, device=w.device)
    rc = lib().fcg_gmres_orthogonalize(w.device.index or 0, n, nv, _tensor_ptr(V), ld, _tensor_ptr(w),
                                       _tensor_ptr(h), _tensor_ptr(work),
                                       _torch_stream(stream, w.device))
    if rc != 0:
        raise FcgError(rc, "fcg_gmres_orthogonalize failed")
    return work


def gmres_orthogonalize_work(n, nv):
    k = lib().fcg_gmres_orthogonalize_work(int(n), int(nv))
    if k < 0:
        raise FcgError(3, "fcg_gmres_orthogonalize_work: bad n or nv")
    return int(k)


def gmres_timing(enable=None):
    """fcg_gmres_set_timing(enable) when `enable` is given; else the sums since it was set:
    {"precond_ms", "operator_ms", "orth_ms", "steps"} over the inner steps launched."""
    if enable is not None:
        rc = lib().fcg_gmres_set_timing(1 if enable else 0)
        if rc != 0:
            raise FcgError(rc, "fcg_gmres_set_timing failed")
        return None
    a, b, c, n = ctypes.c_double(), ctypes.c_double(), ctypes.c_double(), ctypes.c_int64()
    lib().fcg_gmres_get_timing(ctypes.byref(a), ctypes.byref(b), ctypes.byref(c), ctypes.byref(n))
    return {"precond_ms": a.value, "operator_ms": b.value, "orth_ms": c.value, "steps": n.value}


class TsiGraph:
    """The thermo field of a rank for TSI: one temperature DOF per node of the cloned thermo
    discretization (same nodes, elements and owners as the structure; thermo DOF GIDs follow the
    structural ones, 4C_fem_dofset.cpp:628-632) and the Epetra graphs of k_ST, k_TS and k_TT.
    Derived from the structural node graph of `mesh` (BoxMesh or Discretization), whose DOF
    column LIDs are 3 per node in node order."""

    def __init__(self, mesh):
        nn = mesh.n_node
        self.node_dof_col_t = np.ascontiguousarray(mesh.node_dof_col // 3, dtype=np.int32)
        self.node_dof_row_t = np.ascontiguousarray(
            np.where(mesh.node_dof_row >= 0, mesh.node_dof_row // 3, -1), dtype=np.int32)
        self.n_rows_t = int(mesh.n_rows) // 3
        self.n_cols_t = int(mesh.n_cols) // 3
        assert len(self.node_dof_col_t) == nn
        rp = np.asarray(mesh.rowptr, dtype=np.int64)
        cl = np.asarray(mesh.col_lid)
        starts = rp[0:-1:3]                     # first structural row of every owned node
        nnb = (rp[1::3] - rp[0:-1:3]) // 3      # neighbour nodes of the row
        tot = int(nnb.sum())
        self.rowptr_tt = np.concatenate([[0], np.cumsum(nnb)]).astype(np.int64)
        off = np.arange(tot, dtype=np.int64) - np.repeat(self.rowptr_tt[:-1], nnb)
        self.col_tt = np.ascontiguousarray(cl[np.repeat(starts, nnb) + 3 * off] // 3, dtype=np.int32)
        # k_ST: 3 rows per node with the node's thermo columns
        n3 = np.repeat(nnb, 3)
        self.rowptr_st = np.concatenate([[0], np.cumsum(n3)]).astype(np.int64)
        src = np.repeat(np.repeat(self.rowptr_tt[:-1], 3), n3)
        off3 = np.arange(int(n3.sum()), dtype=np.int64) - np.repeat(self.rowptr_st[:-1], n3)
        self.col_st = np.ascontiguousarray(self.col_tt[src + off3], dtype=np.int32)
        # k_TS: one row per node with the node's structural columns (= its structural row)
        self.rowptr_ts = np.concatenate([[0], np.cumsum(3 * nnb)]).astype(np.int64)
        off_ts = np.arange(3 * tot, dtype=np.int64) - np.repeat(self.rowptr_ts[:-1], 3 * nnb)
        self.col_ts = np.ascontiguousarray(cl[np.repeat(starts, 3 * nnb) + off_ts], dtype=np.int32)
        self.nnz_st, self.nnz_ts, self.nnz_tt = len(self.col_st), len(self.col_ts), len(self.col_tt)


class TsiEvaluator:
    """Device context (fcg_tsi_ctx) for the temperature-dependent TSI blocks of one rank."""

    def __init__(self, mesh, youngs, poisson, thexpans, inittemp, conduct, device=0, graph=None):
        L = lib()
        self.mesh = mesh
        self.graph = g = graph or TsiGraph(mesh)
        d = FcgTsiDesc()
        d.abi_version = ABI_VERSION
        d.celltype = mesh.celltype
        d.device = device
        d.youngs, d.poisson, d.thexpans = youngs, poisson, thexpans
        d.inittemp, d.conduct = inittemp, conduct
        d.n_ele, d.n_node = mesh.n_ele, mesh.n_node
        d.n_rows_s, d.n_cols_s = mesh.n_rows, mesh.n_cols
        d.n_rows_t, d.n_cols_t = g.n_rows_t, g.n_cols_t
        d.ele_nodes = _np_ptr(mesh.ele_nodes, _i32p)
        d.ele_gid = _np_ptr(mesh.ele_gid, _i32p)
        d.node_x = _np_ptr(mesh.node_x, _dp)
        d.node_dof_col_s = _np_ptr(mesh.node_dof_col, _i32p)
        d.node_dof_row_s = _np_ptr(mesh.node_dof_row, _i32p)
        d.node_dof_col_t = _np_ptr(g.node_dof_col_t, _i32p)
        d.node_dof_row_t = _np_ptr(g.node_dof_row_t, _i32p)
        d.rowptr_st, d.col_st = _np_ptr(g.rowptr_st, _i64p), _np_ptr(g.col_st, _i32p)
        d.rowptr_ts, d.col_ts = _np_ptr(g.rowptr_ts, _i64p), _np_ptr(g.col_ts, _i32p)
        d.rowptr_tt, d.col_tt = _np_ptr(g.rowptr_tt, _i64p), _np_ptr(g.col_tt, _i32p)
        self.device = device
        h = ctypes.c_void_p()
        rc = L.fcg_tsi_create(ctypes.byref(d), ctypes.byref(h))
        if rc != 0:
            raise FcgError(rc, L.fcg_tsi_last_error(None).decode())
        self._h = h

    def close(self):
        if getattr(self, "_h", None):
            lib().fcg_tsi_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def evaluate_device(self, parts, mode, v_col, T_col, timefac=1.0, timefac_d=1.0, fs=None,
                        Kst=None, fT=None, Ktt=None, Kts=None, stream=None):
        """Tensors: float64 on this device (v_col / T_col in the structural / thermo column maps)."""
        bad = ctypes.c_int32(-1)
        s = _torch_stream(stream, self.device)
        rc = lib().fcg_tsi_evaluate_device(self._h, parts, mode, _tensor_ptr(v_col),
                                           _tensor_ptr(T_col), float(timefac), float(timefac_d),
                                           _tensor_ptr(fs), _tensor_ptr(Kst), _tensor_ptr(fT),
                                           _tensor_ptr(Ktt), _tensor_ptr(Kts), s, ctypes.byref(bad))
        if rc != 0:
            raise FcgError(rc, lib().fcg_tsi_last_error(self._h).decode(), bad.value)

    def evaluate_fused(self, struct_ev, mode, u_col, v_col, T_col, timefac=1.0, timefac_d=1.0,
                       fs=None, Kss=None, Kst=None, fT=None, Ktt=None, Kts=None, stream=None):
        """fcg_tsi_evaluate_fused: the whole monolithic tangent (K_SS, k_ST, k_TS, k_TT) and both
        residuals in one sweep; `struct_ev` is the structured linear StVK Evaluator of the mesh."""
        bad = ctypes.c_int32(-1)
        s = _torch_stream(stream, self.device)
        rc = lib().fcg_tsi_evaluate_fused(struct_ev._h, self._h, mode, _tensor_ptr(u_col),
                                          _tensor_ptr(v_col), _tensor_ptr(T_col), float(timefac),
                                          float(timefac_d), _tensor_ptr(fs), _tensor_ptr(Kss),
                                          _tensor_ptr(Kst), _tensor_ptr(fT), _tensor_ptr(Ktt),
                                          _tensor_ptr(Kts), s, ctypes.byref(bad))
        if rc != 0:
            raise FcgError(rc, lib().fcg_tsi_last_error(self._h).decode(), bad.value)

    def capacity(self, capa, ele_capa=None, mode=OVERWRITE, out=None, stream=None):
        """fcg_tsi_capacity: the capacity matrix of the thermo elements (MAT_Fourier CAPA) on the
        k_TT graph into `out` ([nnz_tt] device tensor; None: a new one, which ACCUMULATE starts
        from zeros).  ele_capa: one capacity per column element (host array), `capa` is then
        ignored.  Returns the tensor; the call waits for the stream."""
        import torch
        if out is None:
            out = torch.empty(int(self.graph.nnz_tt), dtype=torch.float64,
                              device=torch.device("cuda", self.device))
            if mode == ACCUMULATE:
                out.zero_()
        cp = None
        if ele_capa is not None:
            ec = np.ascontiguousarray(ele_capa, dtype=np.float64).reshape(-1)
            if ec.size != self.mesh.n_ele:
                raise ValueError(f"ele_capa has {ec.size} entries, the context {self.mesh.n_ele} elements")
            cp = _np_ptr(ec, _dp)
        bad = ctypes.c_int32(-1)
        rc = lib().fcg_tsi_capacity(self._h, float(capa), cp, int(mode), _tensor_ptr(out),
                                    _torch_stream(stream, self.device), ctypes.byref(bad))
        if rc != 0:
            raise FcgError(rc, lib().fcg_tsi_last_error(self._h).decode(), bad.value)
        return out

    def ost_combine(self, theta, dt, C, T, Tn, h=None, Ktt=None, fT=None, stream=None):
        """fcg_tsi_ost_combine: Ktt <- C/dt + theta Ktt and fT <- theta fT + C (T - Tn)/dt + h in one
        pass over the owned thermo rows (asynchronous).  Ktt / fT hold the FINTCOND evaluate at T
        on entry; either may be None (residual only / tangent only), h None is 0."""
        rc = lib().fcg_tsi_ost_combine(self._h, float(theta), float(dt), _tensor_ptr(C),
                                       _tensor_ptr(T), _tensor_ptr(Tn), _tensor_ptr(h),
                                       _tensor_ptr(Ktt), _tensor_ptr(fT),
                                       _torch_stream(stream, self.device))
        if rc != 0:
            self._fail(rc)

    def _fail(self, rc):
        raise FcgError(rc, lib().fcg_tsi_last_error(self._h).decode())

    def block_apply(self, struct_ev, Kss, Kst, Kts, Ktt, xs, xt, ys, yt, stream=None):
        """fcg_tsi_block_apply: y_S = K_SS x_S + K_ST x_T, y_T = K_TS x_S + K_TT x_T in one kernel
        (asynchronous); `struct_ev` is the structural Evaluator of the mesh."""
        rc = lib().fcg_tsi_block_apply(struct_ev._h, self._h, *[_tensor_ptr(a) for a in
                                       (Kss, Kst, Kts, Ktt, xs, xt, ys, yt)],
                                       _torch_stream(stream, self.device))
        if rc != 0:
            self._fail(rc)

    def dirichlet_apply(self, rows_s=None, rows_t=None, Kst=None, Kts=None, Ktt=None, rhs_T=None,
                        stream=None):
        """fcg_tsi_dirichlet_apply: rows_s / rows_t are int32 device tensors of structural /
        thermal Dirichlet row LIDs (either may be None); K_ST rows_s and K_TS rows_t become zero
        rows, K_TT rows_t unit rows, rhs_T 0 there.  K_SS and rhs_S go through the structural
        Evaluator's dirichlet_apply."""
        ns = 0 if rows_s is None else int(rows_s.numel())
        nt = 0 if rows_t is None else int(rows_t.numel())
        rc = lib().fcg_tsi_dirichlet_apply(self._h, ns, _tensor_ptr(rows_s) if ns else None, nt,
                                           _tensor_ptr(rows_t) if nt else None, _tensor_ptr(Kst),
                                           _tensor_ptr(Kts), _tensor_ptr(Ktt), _tensor_ptr(rhs_T),
                                           _torch_stream(stream, self.device))
        if rc != 0:
            self._fail(rc)

    PRECOND = {"diag": 0, "bgs": 1, 0: 0, 1: 1}

    def gmres_solve(self, struct_ev, Kss, Kst, Kts, Ktt, bs, bt, xs, xt, rtol=1e-10,
                    max_iter=10000, restart=50, precond="bgs", amg=None, stream=None, amg_t=None):
        """fcg_tsi_gmres_solve: the monolithic system by restarted flexible GMRES on [x_S; x_T]
        from x = 0.  precond: "diag" (block diagonal) or "bgs" (block Gauss-Seidel); the
        structural block is the nodal block Jacobi of K_SS or one cycle of `amg` (an
        amg.NativeAMG set up on K_SS), the thermal one the diagonal of K_TT or one cycle of `amg_t`
        (an amg.ScalarAMG set up on this K_TT; fcg_tsi_gmres_solve_amg).  Returns (inner steps
        taken, true relative residual of the stacked system)."""
        opt = gmres_options(restart, max_iter, rtol, self.PRECOND[precond])
        it, rr = ctypes.c_int(0), ctypes.c_double(0.0)
        blocks = [_tensor_ptr(a) for a in (Kss, Kst, Kts, Ktt, bs, bt, xs, xt)]
        tail = (ctypes.byref(opt), ctypes.byref(it), ctypes.byref(rr), _torch_stream(stream, self.device))
        hs = amg._h if amg is not None else None
        if amg_t is not None:
            rc = lib().fcg_tsi_gmres_solve_amg(struct_ev._h, self._h, hs, amg_t._h, *blocks, *tail)
        else:
            rc = lib().fcg_tsi_gmres_solve(struct_ev._h, self._h, hs, *blocks, *tail)
        if rc != 0:
            self._fail(rc)
        return it.value, rr.value


# hex27 surface connectivity (4C_fem_general_utils_local_connectivity_matrices.hpp:51-54); the hex8
# faces are the first four entries of each row
HEX_SURFACES = np.array([[0, 3, 2, 1, 11, 10, 9, 8, 20], [0, 1, 5, 4, 8, 13, 16, 12, 21],
                         [1, 2, 6, 5, 9, 14, 17, 13, 22], [2, 3, 7, 6, 10, 15, 18, 14, 23],
                         [0, 4, 7, 3, 12, 19, 15, 11, 24], [4, 5, 6, 7, 16, 17, 18, 19, 25]])


def boundary_faces(mesh):
    """(face_nodes [n][4 or 9] int32, face_ele [n] int32): the faces that belong to exactly one column
    element of `mesh` (BoxMesh or Discretization), as column node ids in 4C's surface order, ordered by
    element and surface number; face_ele is the column element of each.  Meaningful on single-rank
    meshes, where these are the faces of the body's boundary: on a rank of a split mesh the faces on
    the edge of the ghost layer belong to one column element too."""
    en = np.asarray(mesh.ele_nodes)
    nfn = 4 if mesh.celltype == HEX8 else 9
    faces = en[:, HEX_SURFACES[:, :nfn]].reshape(-1, nfn)
    corners = np.sort(faces[:, :4], axis=1)
    order = np.lexsort(corners.T[::-1])
    sc = corners[order]
    same = np.all(sc[1:] == sc[:-1], axis=1)
    shared = np.zeros(len(sc), dtype=bool)
    shared[1:] |= same
    shared[:-1] |= same
    keep = np.ones(len(sc), dtype=bool)
    keep[order[shared]] = False
    ele = np.repeat(np.arange(len(en), dtype=np.int32), 6)
    return np.ascontiguousarray(faces[keep], dtype=np.int32), np.ascontiguousarray(ele[keep])


class TsiSurface:
    """A surface of a TsiEvaluator's mesh with a heat convection condition (coefficient, surrounding
    temperature) and a heat flux (fcg_tsi_surface): 4C's DESIGN THERMO CONVECTION SURF CONDITIONS and a
    thermal surface Neumann condition, integrated once on the device by set() and applied per Newton
    iteration by convection() / per load evaluation by flux().  face_nodes: [n_faces][4 or 9] column
    node ids in any valid quad4 / quad9 order (boundary_faces gives those of a whole single-rank
    body).  Close the surface before its evaluator."""

    def __init__(self, tev, face_nodes):
        self.tev = tev
        self.device = tev.device
        nfn = 4 if tev.mesh.celltype == HEX8 else 9
        fn = np.ascontiguousarray(face_nodes, dtype=np.int32)
        if fn.size % nfn or (fn.ndim == 2 and fn.shape[1] != nfn):
            raise ValueError(f"face_nodes: {nfn} nodes per face")
        self.face_nodes = fn = fn.reshape(-1, nfn)
        self.n_faces = len(fn)
        h = ctypes.c_void_p()
        rc = lib().fcg_tsi_surface_create(tev._h, self.n_faces, _np_ptr(fn, _i32p), ctypes.byref(h))
        if rc != 0:
            tev._fail(rc)
        self._h = h

    def close(self):
        if getattr(self, "_h", None):
            lib().fcg_tsi_surface_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    @property
    def info(self):
        """dict(n_faces, n_rows, n_entries, device_bytes): surface rows, compact-row entries."""
        a, b, c = ctypes.c_int64(), ctypes.c_int64(), ctypes.c_int64()
        lib().fcg_tsi_surface_info(self._h, ctypes.byref(a), ctypes.byref(b), ctypes.byref(c))
        return dict(n_faces=self.n_faces, n_rows=a.value, n_entries=b.value, device_bytes=c.value)

    def _face_arg(self, v, what):
        if np.ndim(v) == 0:
            return float(v), None, None
        a = np.ascontiguousarray(v, dtype=np.float64).reshape(-1)
        if a.size != self.n_faces:
            raise ValueError(f"{what} has {a.size} entries, the surface {self.n_faces} faces")
        return 0.0, _np_ptr(a, _dp), a

    def set(self, coeff=0.0, surtemp=0.0, flux=0.0):
        """fcg_tsi_surface_set: heat transfer coefficient (>= 0), surrounding temperature and heat
        flux, each a scalar or one value per face; runs the setup kernel and waits for it.  A refused
        value raises FcgError (code 3) naming the face and leaves the earlier tables in place."""
        c, cp, _c = self._face_arg(coeff, "coeff")
        t, tp, _t = self._face_arg(surtemp, "surtemp")
        q, qp, _q = self._face_arg(flux, "flux")
        bad = ctypes.c_int64(-1)
        rc = lib().fcg_tsi_surface_set(self._h, c, cp, t, tp, q, qp, ctypes.byref(bad))
        if rc != 0:
            raise FcgError(rc, lib().fcg_tsi_last_error(self.tev._h).decode(), bad.value)
        return self

    def _vec(self, t, n, what):
        if t is None:
            return None
        import torch
        if (t.dtype != torch.float64 or not t.is_cuda or t.device.index != self.device
                or not t.is_contiguous() or t.numel() != int(n)):
            raise ValueError(f"{what}: a contiguous float64 tensor of {int(n)} entries on cuda:{self.device}")
        return _tensor_ptr(t)

    def convection(self, T, fT=None, Ktt=None, coeff_scale=1.0, surtemp_scale=1.0, stream=None):
        """fcg_tsi_convection: fT += s_c (A T - s_t g) on the surface rows and Ktt += s_c A at the
        compact rows' positions, in one asynchronous pass.  T: thermo column map; fT / Ktt: the
        outputs of the FINTCOND evaluate; either may be None."""
        g = self.tev.graph
        rc = lib().fcg_tsi_convection(self._h, float(coeff_scale), float(surtemp_scale),
                                      self._vec(T, g.n_cols_t, "T"), self._vec(fT, g.n_rows_t, "fT"),
                                      self._vec(Ktt, g.nnz_tt, "Ktt"), _torch_stream(stream, self.device))
        if rc != 0:
            self.tev._fail(rc)

    def flux(self, f, scale=1.0, stream=None):
        """fcg_tsi_surface_flux: f += scale q on the surface rows (asynchronous)."""
        rc = lib().fcg_tsi_surface_flux(self._h, float(scale), self._vec(f, self.tev.graph.n_rows_t, "f"),
                                        _torch_stream(stream, self.device))
        if rc != 0:
            self.tev._fail(rc)

    def tables(self):
        """Copies of the surface's device arrays as torch tensors on the device: rows [n_rows] (thermo
        rows), ptr [n_rows + 1], col / pos / A [n_entries] (thermo column, position in the k_TT value
        array, convection operator), g / q [n_rows]; A, g and q are what the last set() made."""
        import torch
        i = self.info
        nr, ne = i["n_rows"], i["n_entries"]
        p = [ctypes.c_void_p() for _ in range(7)]
        lib().fcg_tsi_surface_tables(self._h, *[ctypes.byref(x) for x in p])
        spec = (("rows", np.int32, nr), ("ptr", np.int64, nr + 1), ("col", np.int32, ne), ("pos", np.int64, ne),
                ("A", np.float64, ne), ("g", np.float64, nr), ("q", np.float64, nr))
        out = {}
        dev = torch.device("cuda", self.device)
        for (name, dt, n), ptr in zip(spec, p):
            a = np.zeros(int(n) if nr else 0, dtype=dt)
            if a.size:
                rc = lib().fcg_memcpy_d2h(a.ctypes.data_as(ctypes.c_void_p), ptr, a.nbytes)
                if rc != 0:
                    raise FcgError(rc, "fcg_memcpy_d2h failed")
            out[name] = torch.from_numpy(a).to(dev)
        return out


def graph_build_device(celltype, ele_nodes, node_dof_col, node_dof_row, n_rows, device=0,
                       stream=None):
    """fcg_graph_build_device on torch tensors (int32, on `device`): returns (rowptr int64,
    col_lid int32) device tensors -- the FillComplete graph of the rank's owned rows."""
    import torch
    dev = torch.device("cuda", device)
    rowptr = torch.empty(int(n_rows) + 1, dtype=torch.int64, device=dev)
    nnz = ctypes.c_int64(0)
    s = _torch_stream(stream, device)
    args = (device, celltype, int(ele_nodes.numel() // (8 if celltype == HEX8 else 27)),
            _tensor_ptr(ele_nodes), int(node_dof_col.numel()), _tensor_ptr(node_dof_col),
            _tensor_ptr(node_dof_row), int(n_rows), _tensor_ptr(rowptr))
    rc = lib().fcg_graph_build_device(*args, None, 0, ctypes.byref(nnz), s)
    if rc != 0:
        raise FcgError(rc, "fcg_graph_build_device (sizing) failed")
    col = torch.empty(max(1, nnz.value), dtype=torch.int32, device=dev)
    rc = lib().fcg_graph_build_device(*args, _tensor_ptr(col), nnz.value, ctypes.byref(nnz), s)
    if rc != 0:
        raise FcgError(rc, "fcg_graph_build_device failed")
    return rowptr, col[:nnz.value]


def measure_peaks(device=0):
    """fcg_measure_peaks: (STREAM-triad GB/s, FP64 VALU TFLOP/s, FP64 MFMA TFLOP/s) on `device`."""
    a, b, c = ctypes.c_double(), ctypes.c_double(), ctypes.c_double()
    rc = lib().fcg_measure_peaks(int(device), ctypes.byref(a), ctypes.byref(b), ctypes.byref(c))
    if rc != 0:
        raise FcgError(rc, "fcg_measure_peaks failed")
    return a.value, b.value, c.value


def measure_hbm(device=0):
    """fcg_measure_hbm: (16-byte copy GB/s, write-only fill GB/s) on `device`."""
    a, b = ctypes.c_double(), ctypes.c_double()
    rc = lib().fcg_measure_hbm(int(device), ctypes.byref(a), ctypes.byref(b))
    if rc != 0:
        raise FcgError(rc, "fcg_measure_hbm failed")
    return a.value, b.value
