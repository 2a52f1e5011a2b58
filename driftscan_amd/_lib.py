"""ctypes binding of libdriftmi.so (the C ABI declared in include/driftmi.h).

The library is built in-tree by ``__graft_entry__.build()`` / ``make -C
driftscan_amd/csrc`` into ``driftscan_amd/lib/libdriftmi.so``.  Loading fails
loudly if it is missing; there is no alternative code path.
"""
import ctypes
import os

import numpy as np

_HERE = os.path.dirname(os.path.abspath(__file__))
LIBPATH = os.path.join(_HERE, "lib", "libdriftmi.so")
if os.environ.get("DRIFTMI_LIB"):  # a differently built libdriftmi.so (kernel tuning experiments)
    LIBPATH = os.environ["DRIFTMI_LIB"]

c_int = ctypes.c_int
c_i64 = ctypes.c_int64
c_dbl = ctypes.c_double
c_vp = ctypes.c_void_p
c_sz = ctypes.c_size_t

class ZgemmProblem(ctypes.Structure):
    """dm_zgemm_problem of include/driftmi.h."""
    _fields_ = [("A", c_vp), ("B", c_vp), ("C", c_vp), ("M", c_int), ("N", c_int), ("K", c_int),
                ("rsA", c_int), ("csA", c_int), ("rsB", c_int), ("csB", c_int), ("ldc", c_int),
                ("conjA", c_int), ("conjB", c_int), ("alpha", c_dbl), ("beta", c_dbl)]


class ZgemmProblemEx(ctypes.Structure):
    """dm_zgemm_problem_ex of include/driftmi.h."""
    _fields_ = [("A", c_vp), ("B", c_vp), ("C", c_vp), ("kscale", c_vp), ("bgather", c_vp),
                ("M", c_int), ("N", c_int), ("K", c_int),
                ("rsA", c_int), ("csA", c_int), ("rsB", c_int), ("csB", c_int), ("ldc", c_int), ("csc", c_int),
                ("flags", c_int), ("alpha", c_dbl), ("alpha_im", c_dbl), ("beta", c_dbl), ("launch", c_int)]


class ZgemmLaunchInfo(ctypes.Structure):
    """dm_zgemm_launch_info of include/driftmi.h."""
    _fields_ = [("launch", c_int), ("use4", c_int), ("deep", c_int), ("wide_r", c_int), ("tiles", c_int * 4),
                ("flat", c_int * 4), ("cells", c_int * 8 * 4)]   # [class][4 flat + 2 ragged + rmw]


# DM_ZGEMM_* of include/driftmi.h
ZGEMM_CONJ_A, ZGEMM_CONJ_B, ZGEMM_B_REAL, ZGEMM_LOWER = 1, 2, 4, 8
ZGEMM_ALL_REAL, ZGEMM_UPPER, ZGEMM_B_GATHER, ZGEMM_UPPER128 = 16, 32, 64, 128
ZGEMM_CLASSES = ("complex", "real_b", "all_real", "gathered")   # class index of dm_zgemm_launch_info


class JacobiProblemDesc(ctypes.Structure):
    """dm_jacobi_problem_desc of include/driftmi.h."""
    _fields_ = [("Z", c_vp), ("ld", c_int), ("row0", c_int), ("nrows", c_int), ("ncols", c_int), ("gc0", c_int),
                ("gc1", c_int)]


class JacobiOptions(ctypes.Structure):
    """dm_jacobi_options of include/driftmi.h."""
    _fields_ = [("unconverged", c_int), ("drop_below", c_dbl), ("one_stage_eig", c_int), ("subspace_cut", c_dbl),
                ("subspace_margin", c_dbl)]


class ZpotrfProblem(ctypes.Structure):
    """dm_zpotrf_problem of include/driftmi.h."""
    _fields_ = [("A", c_vp), ("n", c_int), ("ld", c_int)]


class ZtrsmProblem(ctypes.Structure):
    """dm_ztrsm_problem of include/driftmi.h."""
    _fields_ = [("L", c_vp), ("ldl", c_int), ("n", c_int), ("B", c_vp), ("ldb", c_int), ("nrhs", c_int)]


# name -> (restype, argtypes); mirrors include/driftmi.h one to one
SIGNATURES = {
    "dm_ctx_create": (c_int, [c_int, c_sz, c_vp, ctypes.POINTER(c_vp)]),
    "dm_ctx_destroy": (c_int, [c_vp]),
    "dm_ctx_sync": (c_int, [c_vp]),
    "dm_ctx_workspace_bytes": (c_sz, [c_vp]),
    "dm_ctx_workspace_reset": (c_int, [c_vp, c_sz]),
    "dm_last_error": (ctypes.c_char_p, [c_vp]),
    "dm_version": (c_int, []),
    "dm_prof_reset": (c_int, [c_vp, c_int]),
    "dm_prof_trd_stride": (c_int, []),
    "dm_prof_report": (c_int, [c_vp, ctypes.POINTER(c_dbl), ctypes.POINTER(c_dbl), ctypes.POINTER(ctypes.c_longlong)]),
    "dm_zgemm_strided_batched": (
        c_int,
        [c_vp, c_int, c_int, c_int, c_dbl, c_vp, c_int, c_int, c_int, c_i64, c_vp, c_int, c_int, c_int, c_i64,
         c_dbl, c_vp, c_int, c_i64, c_vp, c_i64, c_int],
    ),
    "dm_zgemm_grouped": (c_int, [c_vp, c_int, ctypes.POINTER(ZgemmProblem)]),
    "dm_zgemm_grouped_ex": (c_int, [c_vp, c_int, ctypes.POINTER(ZgemmProblemEx)]),
    "dm_zgemm_plan_info": (c_int, [c_int, ctypes.POINTER(ZgemmProblemEx), c_int, ctypes.POINTER(ZgemmLaunchInfo),
                                   ctypes.POINTER(c_int)]),
    "dm_zpotrf_batched": (c_int, [c_vp, c_int, c_vp, c_int, c_i64, c_int, ctypes.POINTER(c_int)]),
    "dm_ztrsm_left_lower_batched": (
        c_int, [c_vp, c_int, c_int, c_vp, c_int, c_i64, c_vp, c_int, c_i64, c_int, c_int]),
    "dm_zpotrf_problems": (c_int, [c_vp, c_int, ctypes.POINTER(ZpotrfProblem), ctypes.POINTER(c_int)]),
    "dm_ztrsm_problems": (c_int, [c_vp, c_int, ctypes.POINTER(ZtrsmProblem), c_int, c_int]),
    "dm_zpotrf_problems_check": (c_int, [c_int, ctypes.POINTER(ZpotrfProblem)]),
    "dm_ztrsm_problems_check": (c_int, [c_int, ctypes.POINTER(ZtrsmProblem), c_int, c_int]),
    "dm_jacobi_rows_batched": (
        c_int, [c_vp, c_int, c_int, c_int, c_int, c_vp, c_int, c_i64, c_int, c_vp, ctypes.POINTER(c_int)]),
    "dm_jacobi_rows_problems": (
        c_int, [c_vp, c_int, ctypes.POINTER(JacobiProblemDesc), c_vp, c_int, ctypes.POINTER(JacobiOptions),
                ctypes.POINTER(c_int)]),
    "dm_jacobi_herm_batched": (
        c_int, [c_vp, c_int, c_vp, c_int, c_i64, c_vp, c_int, c_i64, c_int, c_vp, ctypes.POINTER(c_int)]),
    "dm_herm_eig_batched": (c_int, [c_vp, c_int, c_vp, c_int, c_i64, c_vp, c_int, c_i64, c_int, c_vp]),
    "dm_svd_chain": (
        c_int, [c_vp, c_int, c_int, c_int, c_int, c_int, c_vp, c_vp, c_dbl, c_vp, c_vp, c_vp, c_vp,
                ctypes.POINTER(c_int), ctypes.POINTER(c_int)]),
    "dm_svd_chain_lmin": (
        c_int, [c_vp, c_int, c_int, c_int, c_int, c_int, ctypes.POINTER(c_int), c_vp, c_vp, c_dbl, c_vp, c_vp, c_vp, c_vp,
                ctypes.POINTER(c_int), ctypes.POINTER(c_int)]),
    "dm_project_cov": (
        c_int, [c_vp, c_int, c_int, c_int, c_int, c_int, c_vp, ctypes.POINTER(c_int), ctypes.POINTER(c_int), c_vp,
                c_int, ctypes.POINTER(c_int), c_vp, ctypes.POINTER(c_i64), c_int]),
    "dm_project_diag": (
        c_int, [c_vp, c_int, c_int, c_int, c_int, c_vp, ctypes.POINTER(c_int), c_vp, c_dbl, c_vp,
                ctypes.POINTER(c_i64), c_int]),
    "dm_regularise": (c_int, [c_vp, c_int, ctypes.POINTER(c_int), c_vp, ctypes.POINTER(c_i64), c_dbl]),
    "dm_eigh_gen": (
        c_int, [c_vp, c_int, ctypes.POINTER(c_int), c_vp, c_vp, ctypes.POINTER(c_i64), c_vp, ctypes.POINTER(c_i64),
                c_vp, ctypes.POINTER(c_dbl), ctypes.POINTER(c_int), c_int, c_dbl, ctypes.POINTER(c_int)]),
    "dm_kl_m": (
        c_int, [c_vp, c_int, c_int, c_int, c_int, c_int, c_int, c_vp, c_vp, ctypes.POINTER(c_int), ctypes.POINTER(c_int), c_vp,
                ctypes.POINTER(c_int), c_int, c_vp, ctypes.POINTER(c_int), c_int, c_vp, c_dbl, c_dbl, c_int, c_dbl, c_vp,
                ctypes.POINTER(c_i64), c_vp, ctypes.POINTER(c_i64), ctypes.POINTER(c_dbl), ctypes.POINTER(c_int)]),
    "dm_doublekl_m": (
        c_int, [c_vp, c_int, c_int, c_int, c_int, c_int, c_int, c_vp, c_vp, ctypes.POINTER(c_int), ctypes.POINTER(c_int), c_vp,
                ctypes.POINTER(c_int), c_int, c_vp, ctypes.POINTER(c_int), c_int, c_vp, c_dbl, c_dbl, c_dbl, c_int, c_dbl, c_vp,
                c_vp, ctypes.POINTER(c_i64), c_vp, ctypes.POINTER(c_i64), ctypes.POINTER(c_int), ctypes.POINTER(c_int),
                ctypes.POINTER(c_dbl)]),
    "dm_fisher": (
        c_int, [c_vp, c_int, c_int, c_int, c_int, c_int, c_vp, ctypes.POINTER(c_int), ctypes.POINTER(c_int), c_int,
                c_vp, c_vp, ctypes.POINTER(c_i64), ctypes.POINTER(c_int), c_vp, ctypes.POINTER(c_i64), c_vp, c_int]),
    "dm_qestimate": (
        c_int, [c_vp, c_int, c_int, c_int, c_int, c_int, c_vp, ctypes.POINTER(c_int), ctypes.POINTER(c_int), c_int,
                c_vp, c_vp, ctypes.POINTER(c_i64), ctypes.POINTER(c_int), c_vp, ctypes.POINTER(c_i64), c_int, c_vp, c_vp,
                ctypes.POINTER(c_i64), c_int, c_vp]),
    "dm_psmc_draw": (
        c_int, [c_vp, c_int, ctypes.POINTER(c_int), ctypes.POINTER(c_int), c_vp, ctypes.POINTER(c_i64), ctypes.c_uint64,
                c_int, c_int, c_int, c_int, c_int, c_vp, ctypes.POINTER(c_i64)]),
    "dm_psmc_moments": (c_int, [c_vp, c_int, c_int, c_int, c_vp, c_vp, c_vp]),
    "dm_psmc_alt": (
        c_int, [c_vp, c_int, c_int, c_int, c_int, c_int, c_vp, ctypes.POINTER(c_int), ctypes.POINTER(c_int), c_int,
                c_vp, c_vp, ctypes.POINTER(c_i64), ctypes.POINTER(c_int), c_vp, ctypes.POINTER(c_i64), c_int, c_vp,
                ctypes.POINTER(c_i64), c_int, c_vp, c_vp]),
    "dm_sky_draw": (
        c_int, [c_vp, c_int, c_int, c_int, c_vp, c_int, c_i64, ctypes.POINTER(c_int), ctypes.POINTER(c_i64), c_int, c_int,
                c_int, ctypes.c_uint64, c_int, c_int, c_int, c_vp, c_i64, c_i64, c_i64]),
    "dm_source_alm": (c_int, [c_vp, c_int, c_vp, c_vp, c_vp, c_int, c_int, c_vp, c_int, c_int, c_int, c_vp, c_sz]),
    "dm_alm_at_points": (
        c_int, [c_vp, c_int, c_vp, c_vp, c_vp, c_int, ctypes.POINTER(c_int), c_int, c_int, c_int, c_vp, c_i64, c_i64, c_i64,
                c_i64, c_vp, c_int, c_sz]),
    "dm_bt_beam_cyl": (
        c_int, [c_vp, c_int, ctypes.POINTER(c_dbl), ctypes.POINTER(c_dbl), ctypes.POINTER(c_dbl), c_int,
                ctypes.POINTER(c_dbl), ctypes.POINTER(c_dbl), ctypes.POINTER(c_dbl), c_int, c_dbl, c_vp]),
    "dm_bt_beams_cyl": (
        c_int, [c_vp, c_int, ctypes.POINTER(c_dbl), ctypes.POINTER(c_dbl), ctypes.POINTER(c_dbl), c_int,
                ctypes.POINTER(c_int), ctypes.POINTER(c_dbl), ctypes.POINTER(c_dbl), ctypes.POINTER(c_dbl),
                ctypes.POINTER(c_int), ctypes.POINTER(c_dbl), c_vp, ctypes.c_size_t]),
    "dm_bt_maps": (
        c_int, [c_vp, c_int, ctypes.POINTER(c_dbl), ctypes.POINTER(c_dbl), ctypes.POINTER(c_dbl), c_int, c_int, c_vp,
                c_int, ctypes.POINTER(c_dbl), ctypes.POINTER(c_int), ctypes.POINTER(c_int), c_vp]),
    "dm_bt_maps_c": (
        c_int, [c_vp, c_int, ctypes.POINTER(c_dbl), ctypes.POINTER(c_dbl), ctypes.POINTER(c_dbl), c_int, c_int, c_vp,
                c_int, ctypes.POINTER(c_dbl), ctypes.POINTER(c_int), ctypes.POINTER(c_int), c_vp]),
    "dm_bt_sht": (
        c_int, [c_vp, c_int, ctypes.POINTER(c_dbl), ctypes.POINTER(c_dbl), c_int, c_int, c_int, c_int, c_int, c_int,
                c_int, ctypes.POINTER(c_int), ctypes.POINTER(c_int), ctypes.POINTER(c_int), c_vp, c_vp]),
    "dm_bt_sht_range": (
        c_int, [c_vp, c_int, ctypes.POINTER(c_dbl), ctypes.POINTER(c_dbl), c_int, c_int, c_int, c_int, c_int, c_int,
                c_int, c_int, ctypes.POINTER(c_int), ctypes.POINTER(c_int), ctypes.POINTER(c_int), c_vp, c_vp]),
    "dm_bt_sht_opts": (
        c_int, [c_vp, c_int, ctypes.POINTER(c_dbl), ctypes.POINTER(c_dbl), c_int, c_int, c_int, c_int, c_int, c_int,
                c_int, c_int, ctypes.POINTER(c_int), ctypes.POINTER(c_int), ctypes.POINTER(c_int), c_vp, c_vp, c_int,
                ctypes.POINTER(c_dbl)]),
    "dm_bt_columns": (
        c_int, [c_vp, c_int, ctypes.POINTER(c_dbl), ctypes.POINTER(c_dbl), ctypes.POINTER(c_dbl), c_int, c_int, c_vp, c_int,
                ctypes.POINTER(c_dbl), ctypes.POINTER(c_int), ctypes.POINTER(c_int), c_int, c_int, c_int, c_int, c_int, c_int,
                ctypes.POINTER(c_int), ctypes.POINTER(c_int), ctypes.POINTER(c_int), c_vp, ctypes.POINTER(c_dbl)]),
    "dm_bt_columns_c": (
        c_int, [c_vp, c_int, ctypes.POINTER(c_dbl), ctypes.POINTER(c_dbl), ctypes.POINTER(c_dbl), c_int, c_int, c_vp, c_int,
                ctypes.POINTER(c_dbl), ctypes.POINTER(c_int), ctypes.POINTER(c_int), c_int, c_int, c_int, c_int, c_int, c_int,
                ctypes.POINTER(c_int), ctypes.POINTER(c_int), ctypes.POINTER(c_int), c_vp, ctypes.POINTER(c_dbl)]),
    "dm_bt_columns_iter": (
        c_int, [c_vp, c_int, ctypes.POINTER(c_dbl), ctypes.POINTER(c_dbl), ctypes.POINTER(c_dbl), c_int, c_int, c_vp, c_int, c_int,
                ctypes.POINTER(c_dbl), ctypes.POINTER(c_int), ctypes.POINTER(c_int), c_int, c_int, c_int, c_int, c_int, c_int,
                ctypes.POINTER(c_int), ctypes.POINTER(c_int), ctypes.POINTER(c_int), c_vp, ctypes.POINTER(c_dbl), c_int]),
    "dm_sht_synth": (
        c_int, [c_vp, c_int, ctypes.POINTER(c_dbl), ctypes.POINTER(c_dbl), c_int, c_int, c_int, c_int, c_vp, c_vp]),
    "dm_bt_alias_info": (
        c_int, [c_int, ctypes.POINTER(c_dbl), ctypes.POINTER(c_dbl), c_int, c_int, ctypes.POINTER(c_int),
                ctypes.POINTER(c_int)]),
    "dm_bt_ring_plan_info": (
        c_int, [c_int, c_int, c_int, c_int, c_int, c_int, c_int, ctypes.POINTER(c_int), ctypes.POINTER(c_int),
                ctypes.POINTER(c_int), ctypes.POINTER(c_int), ctypes.POINTER(c_int)]),
    "dm_bit_truncate_max_complex": (c_int, [c_vp, c_vp, c_i64, c_int, c_i64, c_dbl, c_dbl]),
    "dm_blockvec_grouped": (c_int, [c_vp, c_int, ctypes.POINTER(ZgemmProblem)]),
    "dm_mmode_twiddle": (c_int, [c_vp, c_int, c_int, c_vp]),
    "dm_ts_noise": (c_int, [c_vp, c_int, c_int, c_int, c_int, c_vp, ctypes.POINTER(c_int), ctypes.c_uint64, c_int, c_vp]),
    "dm_ts_gain_coeff": (
        c_int, [c_vp, c_int, c_int, c_int, c_int, ctypes.POINTER(c_int), c_int, ctypes.POINTER(c_dbl), c_dbl,
                ctypes.c_uint64, c_int, c_int, c_vp]),
    "dm_ts_gain_compose": (c_int, [c_vp, c_i64, c_vp, c_vp, c_vp]),
    "dm_ts_gain_tile": (c_int, [c_int]),
    "dm_ts_gain_apply": (
        c_int, [c_vp, c_int, c_int, c_int, c_int, c_int, c_int, ctypes.POINTER(c_int), ctypes.POINTER(c_int), c_vp, c_vp,
                c_vp, c_i64, c_int]),
    "dm_toeplitz_solve": (c_int, [c_vp, c_int, c_int, c_int, c_vp, c_vp, c_vp]),
    "dm_toeplitz_max_rhs": (c_int, [c_int]),
    "dm_toeplitz_solve_diag": (c_int, [c_vp, c_int, c_int, c_int, c_vp, c_vp, c_vp, c_vp]),
    "dm_vis_stack": (
        c_int, [c_vp, c_int, c_int, c_int, c_int, c_int, c_int, c_int, ctypes.POINTER(c_int), ctypes.POINTER(c_int), c_vp,
                c_vp, c_vp, ctypes.POINTER(c_dbl), c_vp, c_vp, c_i64, c_i64]),
    "dm_vis_expand": (
        c_int, [c_vp, c_int, c_int, c_int, c_int, c_int, c_int, ctypes.POINTER(c_int), ctypes.POINTER(c_int), c_vp, c_vp,
                c_vp, c_i64, c_i64, c_int]),
    "dm_redcal_solve": (
        c_int, [c_vp, c_int, c_int, c_int, c_int, c_int, c_int, ctypes.POINTER(c_int), ctypes.POINTER(c_int), c_vp, c_vp,
                ctypes.POINTER(c_dbl), c_vp, c_dbl, c_dbl, c_int, c_vp, c_vp, c_vp, c_vp, c_vp, c_i64]),
    "dm_modelcal_solve": (
        c_int, [c_vp, c_int, c_int, c_int, c_int, c_int, c_int, c_int, c_int, ctypes.POINTER(c_int), ctypes.POINTER(c_int),
                c_vp, c_vp, c_vp, ctypes.POINTER(c_dbl), c_vp, c_vp, c_dbl, c_dbl, c_int, c_vp, c_vp, c_vp, c_vp, c_vp, c_i64]),
    "dm_sidereal_regrid": (
        c_int, [c_vp, c_int, c_int, c_int, c_int, c_int, c_dbl, c_dbl, c_dbl, c_vp, c_vp, c_vp, c_vp, c_vp, c_vp, c_int]),
    "dm_sidereal_max_taps": (c_int, []),
    "dm_rfi_flag": (
        c_int, [c_vp, c_int, c_int, c_int, c_int, c_dbl, c_int, ctypes.POINTER(c_int), c_dbl, c_dbl, c_int, c_dbl, c_int,
                c_dbl, c_vp, c_vp, c_vp, c_vp, c_vp, c_vp]),
    "dm_rfi_max_segment": (c_int, []),
    "dm_rfi_flag_freq": (
        c_int, [c_vp, c_int, c_int, c_int, c_int, c_dbl, c_int, ctypes.POINTER(c_int), c_dbl, c_dbl, c_int, c_dbl, c_int,
                c_dbl, c_vp, c_vp, c_vp, c_vp, c_vp, c_vp]),
    "dm_rfi_freq_tile": (c_int, [c_int]),
    "dm_rfi_dilate": (c_int, [c_vp, c_int, c_int, c_int, c_int, c_dbl, c_vp, c_vp, c_vp, c_vp]),
    "dm_rfi_dilate_max_length": (c_int, [c_int]),
    "dm_delay_fit": (
        c_int, [c_vp, c_int, c_int, c_int, c_int, c_dbl, c_int, c_int, ctypes.POINTER(c_int), c_vp, c_vp, c_vp, c_vp, c_vp,
                c_vp, c_vp]),
    "dm_delay_max_nf": (c_int, []),
    "dm_delay_max_rank": (c_int, []),
    "dm_delay_tile": (c_int, [c_int, c_int]),
    "dm_ringmap": (
        c_int, [c_vp, c_int, c_int, c_int, c_int, ctypes.POINTER(c_int), ctypes.POINTER(c_int), c_vp, c_vp, c_vp, c_int, c_vp,
                c_int, c_vp, c_vp, c_vp, c_vp, c_vp]),
    "dm_formed_beam": (
        c_int, [c_vp, c_int, c_int, c_int, c_int, ctypes.POINTER(c_int), ctypes.POINTER(c_int), ctypes.POINTER(c_int),
                ctypes.POINTER(c_int), c_int, c_vp, c_int, c_vp, c_vp, c_vp, ctypes.POINTER(c_dbl), c_int, ctypes.POINTER(c_int),
                ctypes.POINTER(c_int), c_vp, c_vp, c_vp, c_vp, c_int, c_vp, c_vp, c_vp, c_vp, c_vp]),
    "dm_formedbeam_block": (c_int, []),
    "dm_formedbeam_max_nu": (c_int, []),
    "dm_delay_spectrum": (
        c_int, [c_vp, c_int, c_int, c_int, c_int, c_int, c_int, c_int, c_vp, c_vp, c_int, ctypes.POINTER(c_int), c_vp, c_vp,
                c_vp, c_vp, c_vp, c_vp, c_vp]),
    "dm_delayspec_max_nf": (c_int, []),
    "dm_delayspec_max_nd": (c_int, []),
    "dm_delayspec_segments": (c_int, [c_int, ctypes.POINTER(c_int)]),
}

_lib = None


class DriftMIError(RuntimeError):
    pass


def load():
    """Load libdriftmi.so and declare every prototype.  Raises if absent."""
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(LIBPATH):
        raise DriftMIError(
            "libdriftmi.so not found at %s — build it with `python -c 'import __graft_entry__ as g; g.build()'` "
            "(there is no CPU fallback)" % LIBPATH
        )
    lib = ctypes.CDLL(LIBPATH)
    for name, (res, args) in SIGNATURES.items():
        fn = getattr(lib, name)  # AttributeError if the symbol is missing: loud by design
        fn.restype = res
        fn.argtypes = args
    _lib = lib
    return lib


# ---- the grouped product with its whole descriptor (dm_zgemm_grouped_ex / dm_zgemm_plan_info) --------------------------
# A problem is a dict: M, N, K, rsA, csA, rsB, csB, ldc and optionally csc (1), flags (0), alpha (1), alpha_im (0),
# beta (0), launch (0), a_off, b_off, c_off, ks_off (element offsets of the views in their tensors, 0) and bgather
# (a host integer array (N, 2)); `Context.zgemm_grouped_ex` also wants the tensors A, B, C and, where used, kscale.
def _zgemm_ex_has_kscale(p):
    return p.get("kscale") is not None or bool(p.get("has_kscale", False))


def zgemm_ex_check_views(p, nA, nB, nC, nks=0):
    """Host arithmetic only: raise ValueError unless every element that the problem's kernel may touch lies inside a
    buffer of nA / nB / nC / nks elements (counted in the element type of that operand)."""
    M, N, K = int(p["M"]), int(p["N"]), int(p["K"])
    flags = int(p.get("flags", 0))
    strides = [int(p[k]) for k in ("rsA", "csA", "rsB", "csB", "ldc")] + [int(p.get("csc", 1))]
    offs = [int(p.get(k, 0)) for k in ("a_off", "b_off", "c_off", "ks_off")]
    if min(M, N, K) < 0 or min(strides) < 0 or min(offs) < 0:
        raise ValueError("zgemm_grouped_ex: negative size, stride or offset")
    if M == 0 or N == 0:
        return
    a_off, b_off, c_off, ks_off = offs
    rsA, csA, rsB, csB, ldc, csc = strides
    if c_off + (M - 1) * ldc + (N - 1) * csc >= nC:
        raise ValueError("zgemm_grouped_ex: the view of C reaches outside its tensor")
    g = p.get("bgather")
    if flags & ZGEMM_B_GATHER:
        if g is None or not _zgemm_ex_has_kscale(p):
            return  # the library refuses it before anything is launched
        g = np.asarray(g, dtype=np.int64)
        if g.shape != (N, 2) or g.min() < 0 or g.max() >= 2 ** 31:
            raise ValueError("zgemm_grouped_ex: bgather must be N pairs of non-negative 32-bit offsets")
    if K == 0:
        return
    if a_off + (M - 1) * rsA + (K - 1) * csA >= nA:
        raise ValueError("zgemm_grouped_ex: the view of A reaches outside its tensor")
    if flags & ZGEMM_B_GATHER:
        if b_off + int(g[:, 0].max()) + (K - 1) * rsB >= nB:
            raise ValueError("zgemm_grouped_ex: a gathered column of B reaches outside its tensor")
        if ks_off + int(g[:, 1].max()) + K - 1 >= nks:
            raise ValueError("zgemm_grouped_ex: a weight run of a gathered column reaches outside kscale")
        return
    if b_off + (K - 1) * rsB + (N - 1) * csB >= nB:
        raise ValueError("zgemm_grouped_ex: the view of B reaches outside its tensor")
    if _zgemm_ex_has_kscale(p) and ks_off + K - 1 >= nks:
        raise ValueError("zgemm_grouped_ex: kscale reaches outside its tensor")


def _zgemm_ex_record(q, p, ptrs):
    """Fill one ZgemmProblemEx from a problem dict; ptrs = addresses of (A, B, C, kscale, bgather), 0 for none."""
    q.A, q.B, q.C, q.kscale, q.bgather = [int(x) or None for x in ptrs]
    q.M, q.N, q.K = int(p["M"]), int(p["N"]), int(p["K"])
    q.rsA, q.csA, q.rsB, q.csB, q.ldc = (int(p[k]) for k in ("rsA", "csA", "rsB", "csB", "ldc"))
    q.csc, q.flags, q.launch = int(p.get("csc", 1)), int(p.get("flags", 0)), int(p.get("launch", 0))
    q.alpha, q.alpha_im, q.beta = float(p.get("alpha", 1.0)), float(p.get("alpha_im", 0.0)), float(p.get("beta", 0.0))


def zgemm_plan_info(problems):
    """What the planner of the grouped product decides for a list of problem dicts (dm_zgemm_plan_info; needs no GPU
    and looks at no memory: kscale counts as present with a `kscale` tensor or `has_kscale` true, bgather with a `bgather` array).  Returns
    one dict per launch, in ascending `launch` order: launch, use4, deep, wide_r, tiles and flat (per class, in the
    order of ZGEMM_CLASSES) and cells, an int array [class, flat, ragged, rmw] of tile counts.  Raises DriftMIError
    where the planner refuses a flag combination."""
    lib = load()
    n = len(problems)
    arr = (ZgemmProblemEx * max(n, 1))()
    for q, p in zip(arr, problems):
        full = int(p["M"]) > 0 and int(p["N"]) > 0
        _zgemm_ex_record(q, p, (full, full, full, _zgemm_ex_has_kscale(p), p.get("bgather") is not None))
    nl = len({int(p.get("launch", 0)) for p in problems})
    out = (ZgemmLaunchInfo * max(nl, 1))()
    got = c_int(0)
    rc = lib.dm_zgemm_plan_info(n, arr, nl, out, ctypes.byref(got))
    if rc != 0:
        raise DriftMIError("dm_zgemm_plan_info failed (%d)" % rc)
    assert got.value == nl
    return [dict(launch=o.launch, use4=bool(o.use4), deep=bool(o.deep), wide_r=bool(o.wide_r), tiles=list(o.tiles),
                 flat=list(o.flat), cells=np.array([list(c) for c in o.cells], dtype=np.int64).reshape(4, 2, 2, 2))
            for o in out[:nl]]


# ---- Cholesky and triangular solves for a ragged list of problems (dm_zpotrf_problems / dm_ztrsm_problems) ----------------
# A factorisation problem is a dict: n, ld and a_off (element offset of the matrix in its tensor, 0); a solve: n, nrhs,
# ldl, ldb, l_off (0), b_off (0).  The `Context` methods also want the tensors (A; L and B).  Without tensors (the host
# checks) a matrix counts as present unless the dict says a_null / l_null / b_null.
def zpotrf_check_view(p, nA):
    """Host arithmetic only: raise ValueError unless the n x n window (leading dimension ld) at a_off lies inside a
    buffer of nA elements.  Sizes the library refuses (ld < n) are left to the library."""
    n, ld, off = int(p["n"]), int(p["ld"]), int(p.get("a_off", 0))
    if min(n, ld, off) < 0:
        raise ValueError("zpotrf_problems: negative size, leading dimension or offset")
    if n > 0 and off + (n - 1) * ld + n > nA:
        raise ValueError("zpotrf_problems: the matrix reaches outside its tensor")


def ztrsm_check_views(p, nL, nB):
    """The same for a solve: the n x n window of L (ldl, l_off) and the n x nrhs window of B (ldb, b_off)."""
    n, nrhs, ldl, ldb = (int(p[k]) for k in ("n", "nrhs", "ldl", "ldb"))
    l_off, b_off = int(p.get("l_off", 0)), int(p.get("b_off", 0))
    if min(n, nrhs, ldl, ldb, l_off, b_off) < 0:
        raise ValueError("ztrsm_problems: negative size, leading dimension or offset")
    if n == 0 or nrhs == 0:
        return
    if l_off + (n - 1) * ldl + n > nL:
        raise ValueError("ztrsm_problems: L reaches outside its tensor")
    if b_off + (n - 1) * ldb + nrhs > nB:
        raise ValueError("ztrsm_problems: B reaches outside its tensor")


def _zpotrf_records(problems, ptrs=None):
    arr = (ZpotrfProblem * max(len(problems), 1))()
    for i, (q, p) in enumerate(zip(arr, problems)):
        q.A = (ptrs[i] if ptrs is not None else (0 if p.get("a_null") else 16)) or None
        q.n, q.ld = int(p["n"]), int(p["ld"])
    return arr


def _ztrsm_records(problems, ptrs=None):
    arr = (ZtrsmProblem * max(len(problems), 1))()
    for i, (q, p) in enumerate(zip(arr, problems)):
        pl, pb = ptrs[i] if ptrs is not None else (0 if p.get("l_null") else 16, 0 if p.get("b_null") else 16)
        q.L, q.B = pl or None, pb or None
        q.ldl, q.n, q.ldb, q.nrhs = int(p["ldl"]), int(p["n"]), int(p["ldb"]), int(p["nrhs"])
    return arr


def zpotrf_problems_check(problems):
    """Status of dm_zpotrf_problems_check for a list of problem dicts (0 or DM_EARG = -1; needs no GPU)."""
    return int(load().dm_zpotrf_problems_check(len(problems), _zpotrf_records(problems)))


def ztrsm_problems_check(problems, conjtrans=False, upper_only=False):
    """Status of dm_ztrsm_problems_check for a list of problem dicts (0 or DM_EARG = -1; needs no GPU)."""
    return int(load().dm_ztrsm_problems_check(len(problems), _ztrsm_records(problems), int(bool(conjtrans)),
                                              int(bool(upper_only))))


class Context(object):
    """One per GPU / process. Binds to torch's current stream on that device so
    that torch.cuda events bracket the work."""

    def __init__(self, device=0, workspace_bytes=1 << 30):
        import torch

        if not torch.cuda.is_available():
            raise DriftMIError("no GPU visible: libdriftmi has no CPU fallback")
        self.torch = torch
        self.lib = load()
        self.device = int(device)
        torch.cuda.set_device(self.device)
        stream = torch.cuda.current_stream(self.device).cuda_stream
        h = c_vp()
        rc = self.lib.dm_ctx_create(self.device, int(workspace_bytes), c_vp(stream), ctypes.byref(h))
        if rc != 0:
            raise DriftMIError("dm_ctx_create failed with code %d" % rc)
        self.h = h

    def close(self):
        if getattr(self, "h", None):
            self.lib.dm_ctx_destroy(self.h)
            self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def check(self, rc, what=""):
        """Raise on every non-zero status of the C ABI: < 0 argument/runtime errors, > 0 the LAPACK-`info`-like numerical
        failures (an eigen-iteration that did not converge, a B that stays indefinite) — none of the entry points hands
        back usable products with one (a chain that went on after a failed Gram eigenproblem would be silently wrong)."""
        if rc != 0:
            msg = self.lib.dm_last_error(self.h)
            kind = "failed" if rc < 0 else "numerical failure, info ="
            raise DriftMIError("%s %s (%d): %s" % (what, kind, rc, msg.decode() if msg else ""))
        return rc

    def sync(self):
        self.check(self.lib.dm_ctx_sync(self.h), "dm_ctx_sync")

    # ---- device array helpers (torch is used for memory only) -------------
    def to_device(self, arr):
        t = self.torch.from_numpy(np.ascontiguousarray(arr))
        return t.to("cuda:%d" % self.device)

    def workspace_reset(self, nbytes=0):
        """Give the (idle) workspace arena back to the driver and optionally reserve ``nbytes`` afresh."""
        self.check(self.lib.dm_ctx_workspace_reset(self.h, int(nbytes)), "dm_ctx_workspace_reset")

    def to_host(self, t):
        """Device tensor -> numpy through page-locked memory (torch's caching host allocator re-uses the
        blocks): several times the rate of a pageable copy, which is what bounds the file output."""
        h = self.torch.empty(t.shape, dtype=t.dtype, pin_memory=True)
        h.copy_(t)
        return h.numpy()

    def defer_host(self, t, event=None, resident=False):
        """Device tensor -> `storage.Deferred`: the host copy is made by the writer pool's copy thread, behind an event
        recorded here (or ``event``, for several views of one result), so the caller goes straight on.  The tensor must
        not be written to afterwards."""
        from . import storage

        if event is None:
            event = self.record_event()
        return storage.Deferred(self, t, event, resident=resident)

    def record_event(self):
        ev = self.torch.cuda.Event()
        ev.record(self.torch.cuda.current_stream(self.device))
        return ev

    def empty(self, shape, dtype):
        tdt = {np.dtype(np.complex128): self.torch.complex128, np.dtype(np.float64): self.torch.float64,
               np.dtype(np.int32): self.torch.int32, np.dtype(np.int64): self.torch.int64}[np.dtype(dtype)]
        return self.torch.empty(shape, dtype=tdt, device="cuda:%d" % self.device)

    def zeros(self, shape, dtype):
        t = self.empty(shape, dtype)
        t.zero_()
        return t

    @staticmethod
    def ptr(t):
        return c_vp(t.data_ptr()) if t is not None else c_vp(0)

    # ---- thin wrappers over the dense building blocks ---------------------
    def zgemm(self, A, B, C, M, N, K, rsA, csA, rsB, csB, ldc, conjA=False, conjB=False, alpha=1.0, beta=0.0,
              kscale=None, batch=1, strideA=0, strideB=0, strideC=0, stride_kscale=0):
        rc = self.lib.dm_zgemm_strided_batched(
            self.h, M, N, K, alpha, self.ptr(A), rsA, csA, int(conjA), strideA, self.ptr(B), rsB, csB, int(conjB),
            strideB, beta, self.ptr(C), ldc, strideC, self.ptr(kscale), stride_kscale, batch)
        self.check(rc, "dm_zgemm_strided_batched")

    def zgemm_grouped(self, problems):
        """One launch for a ragged list of products.  Each problem is a dict with device tensors A, B, C and
        M, N, K, rsA, csA, rsB, csB, ldc (+ optional conjA, conjB, alpha, beta)."""
        n = len(problems)
        if n == 0:
            return
        arr = (ZgemmProblem * n)()
        for q, p in zip(arr, problems):
            q.A, q.B, q.C = p["A"].data_ptr(), p["B"].data_ptr(), p["C"].data_ptr()
            q.M, q.N, q.K = int(p["M"]), int(p["N"]), int(p["K"])
            q.rsA, q.csA, q.rsB, q.csB, q.ldc = int(p["rsA"]), int(p["csA"]), int(p["rsB"]), int(p["csB"]), int(p["ldc"])
            q.conjA, q.conjB = int(bool(p.get("conjA", False))), int(bool(p.get("conjB", False)))
            q.alpha, q.beta = float(p.get("alpha", 1.0)), float(p.get("beta", 0.0))
        self.check(self.lib.dm_zgemm_grouped(self.h, n, arr), "dm_zgemm_grouped")

    def zgemm_grouped_ex(self, problems):
        """The grouped product with every field of its descriptor (dm_zgemm_grouped_ex, exposed for the parity tests).
        Each problem is a dict as described above `zgemm_ex_check_views`, with contiguous device tensors A, B, C
        (complex128; float64 for B with ZGEMM_B_REAL and for all three with ZGEMM_ALL_REAL) and optionally kscale
        (float64).  Problems with the same `launch` share one grouped launch; the launches run in ascending order.
        Every view is checked against its tensor on the host first (ValueError): a wrong stride or offset would be an
        out-of-bounds access on the device."""
        n = len(problems)
        if n == 0:
            return
        torch = self.torch
        arr = (ZgemmProblemEx * n)()
        keep = []
        for q, p in zip(arr, problems):
            flags = int(p.get("flags", 0))
            A, B, C, ks = p["A"], p["B"], p["C"], p.get("kscale")
            want = [torch.float64 if flags & ZGEMM_ALL_REAL else torch.complex128,
                    torch.float64 if flags & (ZGEMM_ALL_REAL | ZGEMM_B_REAL) else torch.complex128,
                    torch.float64 if flags & ZGEMM_ALL_REAL else torch.complex128, torch.float64]
            for t, dt in zip((A, B, C, ks), want):
                if t is not None and not (t.dtype == dt and t.is_contiguous() and t.is_cuda):
                    raise ValueError("zgemm_grouped_ex: contiguous device tensors of the class's element types expected")
            zgemm_ex_check_views(p, A.numel(), B.numel(), C.numel(), ks.numel() if ks is not None else 0)
            a_off, b_off, c_off, ks_off = (int(p.get(k, 0)) for k in ("a_off", "b_off", "c_off", "ks_off"))
            g = None
            if p.get("bgather") is not None:
                g = self.to_device(np.asarray(p["bgather"], dtype=np.int32))
                keep.append(g)
            _zgemm_ex_record(q, p, (A.data_ptr() + A.element_size() * a_off, B.data_ptr() + B.element_size() * b_off,
                                    C.data_ptr() + C.element_size() * c_off,
                                    ks.data_ptr() + 8 * ks_off if ks is not None else 0,
                                    g.data_ptr() if g is not None else 0))
        self.check(self.lib.dm_zgemm_grouped_ex(self.h, n, arr), "dm_zgemm_grouped_ex")

    def bit_truncate_max_complex(self, t, prec, prec_max_row):
        """In place on a contiguous complex device tensor whose LAST axis is the row (drift/core/beamtransfer.py:641-646)."""
        ncols = int(t.shape[-1])
        nrows = int(t.numel() // max(ncols, 1))
        assert t.is_contiguous()
        self.check(self.lib.dm_bit_truncate_max_complex(self.h, self.ptr(t), nrows, ncols, ncols, float(prec),
                                                        float(prec_max_row)), "dm_bit_truncate_max_complex")

    def zpotrf(self, A, n, ld, stride=0, batch=1):
        info = (c_int * batch)()
        self.check(self.lib.dm_zpotrf_batched(self.h, n, self.ptr(A), ld, stride, batch, info), "dm_zpotrf_batched")
        return np.array(info[:], dtype=np.int64)

    def ztrsm(self, L, B, n, nrhs, ldl, ldb, conjtrans=False, strideL=0, strideB=0, batch=1):
        self.check(self.lib.dm_ztrsm_left_lower_batched(self.h, n, nrhs, self.ptr(L), ldl, strideL, self.ptr(B), ldb,
                                                        strideB, int(conjtrans), batch), "dm_ztrsm")

    def _c128_device(self, t, what):
        if not (t.is_complex() and t.element_size() == 16 and t.is_contiguous() and t.is_cuda):
            raise ValueError("%s: contiguous complex128 device tensors expected" % what)

    def zpotrf_problems(self, problems):
        """Lower Cholesky factors of a ragged list of matrices in one chain of launches (dm_zpotrf_problems, exposed for
        the parity tests).  Each problem is a dict with the device tensor A and n, ld, a_off (see `zpotrf_check_view`,
        which every problem passes first: a wrong offset would be an out-of-bounds access on the device).  Returns the
        `info` of every problem (0, or the 1-based index of the first failing pivot)."""
        n = len(problems)
        ptrs = []
        for p in problems:
            self._c128_device(p["A"], "zpotrf_problems")
            zpotrf_check_view(p, int(p["A"].numel()))
            ptrs.append(p["A"].data_ptr() + 16 * int(p.get("a_off", 0)) if int(p["n"]) > 0 else 0)
        info = (c_int * max(n, 1))()
        self.check(self.lib.dm_zpotrf_problems(self.h, n, _zpotrf_records(problems, ptrs), info), "dm_zpotrf_problems")
        return np.array(info[:n], dtype=np.int64)

    def ztrsm_problems(self, problems, conjtrans=False, upper_only=False):
        """L X = B (or L^H X = B) for a ragged list of problems in one chain of launches (dm_ztrsm_problems, exposed for
        the parity tests).  Each problem is a dict with the device tensors L and B and n, nrhs, ldl, ldb, l_off, b_off
        (see `ztrsm_check_views`, which every problem passes first).  upper_only: forward solves with nrhs == n whose
        result is wanted on and above the diagonal only."""
        ptrs = []
        for p in problems:
            self._c128_device(p["L"], "ztrsm_problems")
            self._c128_device(p["B"], "ztrsm_problems")
            ztrsm_check_views(p, int(p["L"].numel()), int(p["B"].numel()))
            full = int(p["n"]) > 0 and int(p["nrhs"]) > 0
            ptrs.append((p["L"].data_ptr() + 16 * int(p.get("l_off", 0)) if full else 0,
                         p["B"].data_ptr() + 16 * int(p.get("b_off", 0)) if full else 0))
        self.check(self.lib.dm_ztrsm_problems(self.h, len(problems), _ztrsm_records(problems, ptrs),
                                              int(bool(conjtrans)), int(bool(upper_only))), "dm_ztrsm_problems")

    def jacobi_rows(self, Z, rows, cols, gc0, gc1, ld, stride=0, batch=1):
        sigma = self.empty((batch, max(rows, 1)), np.float64)
        sw = c_int(0)
        self.check(self.lib.dm_jacobi_rows_batched(self.h, rows, cols, gc0, gc1, self.ptr(Z), ld, stride, batch,
                                                   self.ptr(sigma), ctypes.byref(sw)), "dm_jacobi_rows_batched")
        return sigma, sw.value

    def jacobi_rows_problems(self, Z, problems, sigma=None, sigma_stride=None, **opts):
        """The ragged form of `jacobi_rows` (dm_jacobi_rows_problems).  Z: one complex128 device tensor that holds every
        matrix; each problem is a dict with `off` (element offset of its matrix in Z), ld, row0, nrows, ncols, gc0, gc1.
        Options by keyword: unconverged, drop_below, one_stage_eig, subspace_cut, subspace_margin (none given: the
        library gets no option block).  Every problem must lie inside Z (a wrong offset would be an out-of-bounds access
        on the device).  Returns (sigma (nprob, sigma_stride) f64 on the device, sweeps)."""
        n = len(problems)
        unknown = set(opts) - {f[0] for f in JacobiOptions._fields_}
        if unknown:
            raise ValueError("jacobi_rows_problems: unknown option(s) %s" % sorted(unknown))
        if n and not (Z.is_complex() and Z.element_size() == 16 and Z.is_contiguous()):
            raise ValueError("jacobi_rows_problems: a contiguous complex128 device tensor expected")
        arr = (JacobiProblemDesc * max(n, 1))()
        for q, p in zip(arr, problems):
            off, ld, row0, nrows, ncols = (int(p[k]) for k in ("off", "ld", "row0", "nrows", "ncols"))
            if min(off, ld, row0, nrows, ncols) < 0 or ncols > ld:
                raise ValueError("jacobi_rows_problems: negative size or ncols > ld")
            if nrows > 0 and ncols > 0 and off + (row0 + nrows - 1) * ld + ncols > int(Z.numel()):
                raise ValueError("jacobi_rows_problems: a problem reaches outside its buffer")
            q.Z = Z.data_ptr() + 16 * off if nrows > 0 else None
            q.ld, q.row0, q.nrows, q.ncols, q.gc0, q.gc1 = ld, row0, nrows, ncols, int(p["gc0"]), int(p["gc1"])
        if sigma_stride is None:
            sigma_stride = max([int(p["nrows"]) for p in problems] + [1])
        if sigma is None:
            sigma = self.zeros((max(n, 1), sigma_stride), np.float64)
        elif n and (sigma.dtype != self.torch.float64 or not sigma.is_contiguous() or sigma.numel() < n * sigma_stride):
            raise ValueError("jacobi_rows_problems: sigma must be a contiguous float64 tensor of nprob * sigma_stride")
        o = None
        if opts:
            o = JacobiOptions(int(bool(opts.get("unconverged", False))), float(opts.get("drop_below", 0.0)),
                              int(bool(opts.get("one_stage_eig", False))), float(opts.get("subspace_cut", 0.0)),
                              float(opts.get("subspace_margin", 0.0)))
        sw = c_int(0)
        self.check(self.lib.dm_jacobi_rows_problems(self.h, n, arr, self.ptr(sigma), int(sigma_stride),
                                                    ctypes.byref(o) if o is not None else None, ctypes.byref(sw)),
                   "dm_jacobi_rows_problems")
        return sigma, sw.value

    def jacobi_herm(self, C, n, ldc, strideC=0, batch=1):
        W = self.empty((batch, n, n), np.complex128)
        ev = self.empty((batch, max(n, 1)), np.float64)
        sw = c_int(0)
        self.check(self.lib.dm_jacobi_herm_batched(self.h, n, self.ptr(C), ldc, strideC, self.ptr(W), n, n * n, batch,
                                                   self.ptr(ev), ctypes.byref(sw)), "dm_jacobi_herm_batched")
        return ev, W, sw.value


# ---- block-apply of stored product blocks to a few vectors (dm_blockvec_grouped) ---------------------------------------
# A problem TABLE is a numpy record array, one row per problem y = op(A) x: element offsets of the problem's A, x and y in
# three buffers shared by the whole call, its shape and strides.  The tables are made by plain numpy code
# (`blockvec_table` and the builders in beamtransfer.py / kltransform.py) that needs no device, so the packed layouts are
# testable on the host; `Context.blockvec_grouped` turns the offsets into addresses.
BLOCKVEC_FIELDS = ("a0", "x0", "y0", "M", "K", "rsA", "csA", "rsB", "csB", "ldc", "conjA", "conjB")
BLOCKVEC_TABLE = np.dtype([(k, np.int64) for k in BLOCKVEC_FIELDS])
_ZGEMM_RECORD = np.dtype([("A", np.uint64), ("B", np.uint64), ("C", np.uint64), ("M", np.int32), ("N", np.int32),
                          ("K", np.int32), ("rsA", np.int32), ("csA", np.int32), ("rsB", np.int32), ("csB", np.int32),
                          ("ldc", np.int32), ("conjA", np.int32), ("conjB", np.int32), ("alpha", np.float64),
                          ("beta", np.float64)], align=True)
assert _ZGEMM_RECORD.itemsize == ctypes.sizeof(ZgemmProblem)
BLOCKVEC_MAX_R = 8      # right-hand sides the kernel keeps in registers; wider calls go to the grouped ZGEMM
BLOCKVEC_LEAN_R = 6     # up to here the kernel was at least as fast as the grouped ZGEMM on every measured batch
BLOCKVEC_LONG_K = 256   # one LDS chunk of x (BV_KC of dm_modes.hip)


def blockvec_route(table, R):
    """Which kernel takes a table at R right-hand sides, from the rates of DESIGN.md section 4.11: the streaming kernel
    up to 6 right-hand sides; for 7 and 8 only where most of A lies in rows longer than one LDS chunk of x (the KL
    eigenvector blocks: measured 1.1 to 4.5 times the ZGEMM's rate at R = 8) — on short rows (the `beam_ut` blocks,
    K = ntel) it is 20 % behind the ZGEMM at R = 8; the grouped ZGEMM above 8."""
    if R <= BLOCKVEC_LEAN_R:
        return "blockvec"
    if R > BLOCKVEC_MAX_R:
        return "zgemm"
    work = table["M"] * table["K"]
    return "blockvec" if 2 * int(work[table["K"] > BLOCKVEC_LONG_K].sum()) >= int(work.sum()) else "zgemm"


def blockvec_table(**cols):
    """Record array of problems from per-problem columns (scalars broadcast); conjA / conjB default to 0."""
    cols.setdefault("conjA", 0)
    cols.setdefault("conjB", 0)
    arrs = np.broadcast_arrays(*[np.asarray(cols[k], dtype=np.int64) for k in BLOCKVEC_FIELDS])
    tab = np.zeros(arrs[0].shape, dtype=BLOCKVEC_TABLE).reshape(-1)
    for k, a in zip(BLOCKVEC_FIELDS, arrs):
        tab[k] = a.reshape(-1)
    return tab


def _blockvec_grouped(self, A, x, y, table, R, route=None):
    """y_p = op(A_p) x_p for every row of `table` (offsets into the device tensors A, x, y; R right-hand sides) in one
    launch.  Problems with M = 0 or K = 0 are left out: nothing is written for them.  route: None (`blockvec_route`),
    "blockvec" or "zgemm"."""
    R = int(R)
    if R < 1:
        raise ValueError("blockvec_grouped: R must be positive")
    if route == "blockvec" and R > BLOCKVEC_MAX_R:
        raise ValueError("blockvec_grouped: the kernel takes at most %d right-hand sides" % BLOCKVEC_MAX_R)
    table = np.asarray(table)
    table = table[(table["M"] > 0) & (table["K"] > 0)]
    n = int(table.shape[0])
    if n == 0:
        return
    if route is None:
        route = blockvec_route(table, R)
    for t in (A, x, y):
        if not (t.is_complex() and t.element_size() == 16 and t.is_contiguous()):
            raise ValueError("blockvec_grouped: contiguous complex128 device tensors expected")
    # every problem must lie inside its buffers (a wrong offset would be an out-of-bounds access on the device)
    M1, K1 = table["M"] - 1, table["K"] - 1
    for lo, hi, t, what in (
            (table["a0"] + np.minimum(0, M1 * table["rsA"]) + np.minimum(0, K1 * table["csA"]),
             table["a0"] + np.maximum(0, M1 * table["rsA"]) + np.maximum(0, K1 * table["csA"]), A, "A"),
            (table["x0"] + np.minimum(0, K1 * table["rsB"]) + np.minimum(0, (R - 1) * table["csB"]),
             table["x0"] + np.maximum(0, K1 * table["rsB"]) + np.maximum(0, (R - 1) * table["csB"]), x, "x"),
            (table["y0"], table["y0"] + M1 * table["ldc"] + (R - 1), y, "y")):
        if int(lo.min()) < 0 or int(hi.max()) >= int(t.numel()):
            raise ValueError("blockvec_grouped: a problem reaches outside its %s buffer" % what)
    if int(table["ldc"].min()) < R:
        raise ValueError("blockvec_grouped: ldc < R")
    rec = np.zeros(n, dtype=_ZGEMM_RECORD)
    rec["A"] = A.data_ptr() + 16 * table["a0"]
    rec["B"] = x.data_ptr() + 16 * table["x0"]
    rec["C"] = y.data_ptr() + 16 * table["y0"]
    rec["N"] = R
    for k in ("M", "K", "rsA", "csA", "rsB", "csB", "ldc", "conjA", "conjB"):
        rec[k] = table[k]
    rec["alpha"] = 1.0
    arr = rec.ctypes.data_as(ctypes.POINTER(ZgemmProblem))
    if route == "blockvec":
        self.check(self.lib.dm_blockvec_grouped(self.h, n, arr), "dm_blockvec_grouped")
    elif route == "zgemm":
        self.check(self.lib.dm_zgemm_grouped(self.h, n, arr), "dm_zgemm_grouped")
    else:
        raise ValueError("blockvec_grouped: unknown route %r" % (route,))


def _mmode_twiddle(self, ntime, mmax):
    """(ntime, mmax + 1) c128 table W[t, m] = exp(-2 pi i m t / ntime) / ntime on the device (dm_mmode_twiddle)."""
    W = self.empty((int(ntime), int(mmax) + 1), np.complex128)
    self.check(self.lib.dm_mmode_twiddle(self.h, int(ntime), int(mmax), self.ptr(W)), "dm_mmode_twiddle")
    return W


def _mmode_transform(self, X, mmax, out=None):
    """Pruned time -> m transform of timestreams X (nf, npairs, ntime) on the device: out[m, f, 0] = the +m bin of
    fft(X) / ntime, out[m, f, 1] = the conjugate of the -m bin (zero for m = 0) — the [m][f][2][npairs] layout of the
    mode.hdf5 files.  Two strided-batched ZGEMMs with the twiddle table: the same table against conj(X) gives slot 1,
    conj(Xhat[ntime - m]) = sum_t conj(x_t) exp(-2 pi i m t / ntime)."""
    nf, npairs, ntime = (int(v) for v in X.shape)
    mmax = int(mmax)
    if ntime < 2 * mmax + 1:
        raise ValueError("mmode_transform: %d time samples cannot hold m up to %d" % (ntime, mmax))
    if not X.is_contiguous():
        X = X.contiguous()
    if out is None:
        out = self.empty((mmax + 1, nf, 2, npairs), np.complex128)
    if tuple(out.shape) != (mmax + 1, nf, 2, npairs) or not out.is_contiguous():
        raise ValueError("mmode_transform: out must be a contiguous (mmax + 1, nf, 2, npairs) tensor")
    if nf == 0 or npairs == 0:
        return out
    W = self.mmode_twiddle(ntime, mmax)
    flat = out.view(-1)
    for slot in (0, 1):
        self.zgemm(W, X, flat[slot * npairs:], mmax + 1, npairs, ntime, rsA=1, csA=mmax + 1, rsB=1, csB=ntime,
                   ldc=nf * 2 * npairs, conjB=bool(slot), batch=nf, strideA=0, strideB=npairs * ntime, strideC=2 * npairs)
    out[0, :, 1].zero_()
    return out


def _mmode_synthesis(self, V, ntime, out=None, accumulate=False):
    """The inverse of `mmode_transform`: m-modes V (mmax + 1, nf, 2, npairs) on the device, the layout of the mode files,
    to timestreams out (nf, npairs, ntime),

        out[f, p, t] = sum_{m=0..mmax} V[m, f, 0, p] e^{+2 pi i m t / ntime}
                     + sum_{m=1..mmax} conj(V[m, f, 1, p]) e^{-2 pi i m t / ntime}

    (slot 1 of m = 0 is not read) — what `timestream.simulate` computes as ifft(col_vis) ntime.  Two strided-batched
    ZGEMMs over the frequencies against ntime times the table of `mmode_twiddle`: its conjugate for slot 0, the table
    itself against conj(V) for slot 1.  accumulate=True adds to what `out` holds (the noise `ts_noise` has just drawn
    there)."""
    if V.dim() != 4 or int(V.shape[2]) != 2 or not (V.is_complex() and V.element_size() == 16):
        raise ValueError("mmode_synthesis: m-modes (mmax + 1, nf, 2, npairs) complex128 expected, got %s" % (tuple(V.shape),))
    nm, nf, _, npairs = (int(v) for v in V.shape)
    mmax, ntime = nm - 1, int(ntime)
    if nm < 1 or ntime < 2 * mmax + 1:
        raise ValueError("mmode_synthesis: %d time samples cannot hold m up to %d" % (ntime, mmax))
    # V may be one column of a contiguous (mmax + 1, nf, 2, npairs, R) array (the batched projection's output): the
    # products read it through its element stride, without a copy
    s = int(V.stride(3))
    if s < 1 or tuple(V.stride()) != (nf * 2 * npairs * s, 2 * npairs * s, npairs * s, s):
        V, s = V.contiguous(), 1
    if out is None:
        if accumulate:
            raise ValueError("mmode_synthesis: accumulate needs the buffer to add to")
        out = self.empty((nf, npairs, ntime), np.complex128)
    if tuple(out.shape) != (nf, npairs, ntime) or not out.is_contiguous() or not (out.is_complex() and out.element_size() == 16):
        raise ValueError("mmode_synthesis: out must be a contiguous (nf, npairs, ntime) complex128 tensor")
    if nf == 0 or npairs == 0:
        return out
    W = self.mmode_twiddle(ntime, mmax)
    row = nf * 2 * npairs * s
    self.zgemm(V, W, out, npairs, ntime, mmax + 1, rsA=s, csA=row, rsB=1, csB=mmax + 1, ldc=ntime, conjB=True,
               alpha=float(ntime), beta=1.0 if accumulate else 0.0, batch=nf, strideA=2 * npairs * s, strideB=0,
               strideC=npairs * ntime)
    if mmax > 0:   # slot 1 from m = 1: A starts at V[1, 0, 1], the table at its column 1
        self.zgemm(V[1, 0, 1], W[0, 1:], out, npairs, ntime, mmax, rsA=s, csA=row, rsB=1, csB=mmax + 1, ldc=ntime,
                   conjA=True, alpha=float(ntime), beta=1.0, batch=nf, strideA=2 * npairs * s, strideB=0,
                   strideC=npairs * ntime)
    return out


def _ts_noise(self, sigma, fglobal, ntime, nreal, seed, first=0, out=None):
    """Receiver noise out[r, i, p, t] = sigma[i, p] z on the device (dm_ts_noise): sigma (nf, npairs) f64 (numpy or
    device), `fglobal` the global frequency index of every row of sigma, z the unit complex normal of (seed, pair, global
    frequency, t, realisation first + r) — `skysim.noise_host` restates it.  Every element of `out`
    (nreal, nf, npairs, ntime) is written."""
    if isinstance(sigma, np.ndarray) or not hasattr(sigma, "data_ptr"):
        sigma = self.to_device(np.asarray(sigma, dtype=np.float64))
    if sigma.dim() != 2 or sigma.dtype != self.torch.float64:
        raise ValueError("ts_noise: sigma (nf, npairs) float64 expected")
    sigma = sigma.contiguous()
    nf, npairs = (int(v) for v in sigma.shape)
    fg, fgp = _iarr(fglobal)
    ntime, nreal, first = int(ntime), int(nreal), int(first)
    if fg.shape != (nf,) or (nf and int(fg.min()) < 0):
        raise ValueError("ts_noise: one non-negative global frequency index per row of sigma expected")
    if ntime < 0 or nreal < 0 or first < 0:
        raise ValueError("ts_noise: ntime, nreal and first must not be negative")
    if out is None:
        out = self.empty((nreal, nf, npairs, ntime), np.complex128)
    if tuple(out.shape) != (nreal, nf, npairs, ntime) or not out.is_contiguous() or not (out.is_complex() and out.element_size() == 16):
        raise ValueError("ts_noise: out must be a contiguous (nreal, nf, npairs, ntime) complex128 tensor")
    rc = self.lib.dm_ts_noise(self.h, nreal, nf, npairs, ntime, self.ptr(sigma), fgp, int(seed) & 0xFFFFFFFFFFFFFFFF, first,
                              self.ptr(out))
    self.check(rc, "dm_ts_noise")
    return out


Context.blockvec_grouped = _blockvec_grouped
Context.mmode_twiddle = _mmode_twiddle
Context.mmode_transform = _mmode_transform
Context.mmode_synthesis = _mmode_synthesis
Context.ts_noise = _ts_noise


def _iarr(a):
    a = np.ascontiguousarray(a, dtype=np.int32)
    return a, a.ctypes.data_as(ctypes.POINTER(c_int))


def _larr(a):
    a = np.ascontiguousarray(a, dtype=np.int64)
    return a, a.ctypes.data_as(ctypes.POINTER(c_i64))


def _is_c128(t, shape=None):
    return (hasattr(t, "data_ptr") and t.is_complex() and t.element_size() == 16 and t.is_contiguous()
            and (shape is None or tuple(t.shape) == tuple(shape)))


def _rstride_of(t, complex_):
    """Element stride between the realisations of a (nreal, nf, rows, ntime) tensor of complex128 (complex_) or float64
    elements that is contiguous apart from it (a frequency slice of a contiguous array), or None."""
    if not (hasattr(t, "data_ptr") and t.dim() == 4 and t.is_complex() == complex_
            and t.element_size() == (16 if complex_ else 8)):
        return None
    nreal, nf, rows, ntime = (int(v) for v in t.shape)
    if t.numel() and tuple(t.stride())[1:] != (rows * ntime, ntime, 1) and not t[0].is_contiguous():
        return None
    rs = int(t.stride(0)) if nreal > 1 else nf * rows * ntime
    return rs if rs >= nf * rows * ntime else None


def _rows_overlap(a, b):
    """Whether two tensors that `_rstride_of` accepts, of one shape and (beyond one realisation) one stride, share an
    element: some row of `b` begins less than a row's length from some row of `a`."""
    nreal, row = int(a.shape[0]), 16 * int(a[0].numel())
    if row == 0 or nreal == 0:
        return False
    rs, d = 16 * _rstride_of(a, True), b.data_ptr() - a.data_ptr()
    near = -d // rs                                         # d + k rs is smallest in size at k = near or near + 1
    return any(abs(d + min(max(k, 1 - nreal), nreal - 1) * rs) < row for k in (near, near + 1))


def _class_table(who, class_off, members):
    off, offp = _iarr(class_off)
    mem, memp = _iarr(np.asarray(members, dtype=np.int32).reshape(-1, 2))
    if off.ndim != 1 or off.shape[0] < 1 or mem.shape[0] != int(off[-1]):
        raise ValueError("%s: class_off (npairs + 1) and members (class_off[-1], 2) expected" % who)
    return off, offp, mem, memp


def _weights_arg(who, w, shape, nreal=None):
    """The float64 weights of the feed-pair chain: of exactly `shape` (x's), or with `nreal` (1 or nreal, *shape); returns
    the number of realisations they hold."""
    ok = hasattr(w, "data_ptr") and not w.is_complex() and w.element_size() == 8 and w.is_contiguous()
    if nreal is None:
        if not (ok and w.dtype.is_floating_point and tuple(w.shape) == tuple(shape)):
            raise ValueError("%s: w must be a contiguous float64 tensor of x's shape" % who)
        return None
    if not (ok and w.dim() == 4 and tuple(w.shape)[1:] == tuple(shape) and int(w.shape[0]) in (1, nreal)):
        raise ValueError("%s: w must be a contiguous float64 tensor (1 or nreal, nf, nmem, ntime)" % who)
    return int(w.shape[0])


def _gains_arg(who, g, nreal, nf, ntime):
    """The calibration gains (1 or nreal, nf, nfeed, ntime); returns (g_nreal, nfeed)."""
    if not (_is_c128(g) and g.dim() == 4 and int(g.shape[1]) == nf and int(g.shape[3]) == ntime
            and int(g.shape[0]) in (1, nreal)):
        raise ValueError("%s: g must be a contiguous complex128 tensor (1 or nreal, nf, nfeed, ntime)" % who)
    return int(g.shape[0]), int(g.shape[2])


def _feed_weight_arg(who, feed_weight, nfeed, exact=False):
    """feed_weight with one entry per feed, at least `nfeed` of them (exactly, with `exact`); returns (the array, which
    the caller keeps until the call is over, its pointer, nfeed) — (None, None, nfeed) without feed_weight."""
    if feed_weight is None:
        return None, None, nfeed
    fw = np.ascontiguousarray(feed_weight, dtype=np.float64)
    if fw.ndim != 1 or (exact and fw.shape[0] != nfeed) or fw.shape[0] < nfeed:
        raise ValueError("%s: feed_weight must have one entry per feed" % who)
    return fw, fw.ctypes.data_as(ctypes.POINTER(c_dbl)), int(fw.shape[0])


def _out_arg(ctx, who, out, shapes):
    """`out` of the solvers, a dict of preallocated tensors under names of `shapes` (name -> (shape, dtype)), filled with
    new tensors where a name is missing."""
    out = dict(out or {})
    if set(out) - set(shapes):
        raise ValueError("%s: out holds %s" % (who, sorted(set(out) - set(shapes))))
    for name, (shape, dt) in shapes.items():
        if out.get(name) is None:
            out[name] = ctx.empty(shape, dt)
        t = out[name]
        if not (hasattr(t, "data_ptr") and tuple(t.shape) == shape and t.is_contiguous()
                and t.dtype == ctx.empty((0,), dt).dtype):
            raise ValueError("%s: out[%r] must be a contiguous %s tensor of shape %s" % (who, name, np.dtype(dt), shape))
    return out


# ---- the arguments of the kernels that take a data cube (nf, nrow, nt) of a Timestream directory ----------------------
def _cube_arg(who, x, w, name="x"):
    """The cube `name`, a contiguous complex128 tensor (nf, nrow, nt), and its weights `w`, float64 of that shape or
    None; returns (nf, nrow, nt)."""
    if not (_is_c128(x) and x.dim() == 3):
        raise ValueError("%s: contiguous complex128 tensor %s (nf, nrow, nt) expected" % (who, name))
    if w is not None:
        _weights_arg(who, w, x.shape)
    return tuple(int(v) for v in x.shape)


def _is_tensor(t, dtype, shape):
    return hasattr(t, "data_ptr") and t.dtype == dtype and t.is_contiguous() and tuple(t.shape) == tuple(shape)


def _out_tuple(who, out, shapes, dtypes, device, optional=(), expected=""):
    """The tuple of outputs of a kernel: new tensors of `shapes` and `dtypes` on `device` when `out` is None, else `out`
    itself once every entry is such a tensor (None is allowed at the positions `optional`: that output is not written).
    `expected` is what the ValueError says after `who`."""
    import torch

    if out is None:
        return tuple(torch.empty(s, dtype=d, device=device) for s, d in zip(shapes, dtypes))
    out = tuple(out)
    if len(out) != len(shapes) or not all((o is None and i in optional) or _is_tensor(o, d, s)
                                          for i, (o, s, d) in enumerate(zip(out, shapes, dtypes))):
        raise ValueError("%s: %s" % (who, expected))
    return out


def _f64_table(who, t, n, name, device):
    """The table `name` of `n` float64 values (None: of any length) on `device`: a tensor as it is, anything else through
    numpy."""
    import torch

    if not hasattr(t, "data_ptr"):
        t = torch.from_numpy(np.ascontiguousarray(np.asarray(t, dtype=np.float64).reshape(-1))).to(device)
    if not (t.dtype == torch.float64 and t.is_contiguous() and t.dim() == 1 and n in (None, int(t.shape[0]))):
        raise ValueError("%s: %s must be a contiguous float64 tensor (%s,)" % (who, name, "n" if n is None else n))
    return t


def _f64_out(who, t, shape, name, device):
    """The float64 output `name` of `shape`: `t`, or a new tensor on `device` when it is None."""
    import torch

    if t is None:
        return torch.empty(shape, dtype=torch.float64, device=device)
    if not _is_tensor(t, torch.float64, shape):
        raise ValueError("%s: %s must be a contiguous float64 tensor %s" % (who, name, shape))
    return t


def _group_table(who, group_off, members, nrow):
    """The groups of rows of a cube as host integers: group g is members[group_off[g]:group_off[g + 1]], every member a
    row below `nrow`; returns (group_off, its pointer, members, its pointer)."""
    off, offp = _iarr(group_off)
    mem, memp = _iarr(members)
    if off.ndim != 1 or off.shape[0] < 1 or mem.ndim != 1 or off[0] != 0 or np.any(np.diff(off) < 0) or mem.shape[0] != int(off[-1]):
        raise ValueError("%s: group_off (ngroup + 1), from 0 and not decreasing, and members (group_off[-1]) expected" % who)
    if mem.size and (mem.min() < 0 or mem.max() >= nrow):
        raise ValueError("%s: a member is no row of vis" % who)
    return off, offp, mem, memp


def _same_gpu(who, tensors, what):
    """Every tensor of `tensors` (None: left out) is on the GPU of the first one, the cube; else ValueError naming `what`.
    A kernel gets nothing but `data_ptr()`, so a host tensor must stop here."""
    dev = tensors[0].device
    if not all(t is None or (t.is_cuda and t.device == dev) for t in tensors):
        raise ValueError("%s: %s must be tensors on one GPU" % (who, what))


def _ts_gain_coeff(self, nreal, fglobal, nfeed, ck, sigma, seed, first=0, stream=25, broadband=False, out=None):
    """Fourier coefficients out[r, i, a, k] = sigma ck[k] (A_k - i B_k) of one component of the feed gains on the device
    (dm_ts_gain_coeff; `skysim.gain_coeff_host` restates it): `fglobal` the global frequency index of every row i, `ck`
    the (K + 1) weights, stream 25 (amplitude) or 26 (phase), broadband=True one draw for all frequencies.  Every element
    of `out` (nreal, nf, nfeed, K + 1) is written."""
    fg, fgp = _iarr(fglobal)
    ck = np.ascontiguousarray(ck, dtype=np.float64)
    nreal, nfeed, first, nf, nk = int(nreal), int(nfeed), int(first), int(fg.shape[0]), int(ck.shape[0])
    if fg.ndim != 1 or ck.ndim != 1 or (nf and int(fg.min()) < 0):
        raise ValueError("ts_gain_coeff: non-negative global frequency indices (nf) and weights (K + 1) expected")
    if nreal < 0 or nfeed < 0 or first < 0:
        raise ValueError("ts_gain_coeff: nreal, nfeed and first must not be negative")
    if out is None:
        out = self.empty((nreal, nf, nfeed, nk), np.complex128)
    if not _is_c128(out, (nreal, nf, nfeed, nk)):
        raise ValueError("ts_gain_coeff: out must be a contiguous (nreal, nf, nfeed, K + 1) complex128 tensor")
    rc = self.lib.dm_ts_gain_coeff(self.h, nreal, nf, nfeed, nk, fgp, int(bool(broadband)),
                                   ck.ctypes.data_as(ctypes.POINTER(c_dbl)), float(sigma), int(seed) & 0xFFFFFFFFFFFFFFFF,
                                   first, int(stream), self.ptr(out))
    self.check(rc, "dm_ts_gain_coeff")
    return out


def _ts_gain_compose(self, xamp, xphase, out=None):
    """g = (1 + Re xamp) exp(i Re xphase) elementwise on the device (dm_ts_gain_compose): complex128 tensors of one shape
    (the series as the ZGEMM leaves them)."""
    if not (_is_c128(xamp) and _is_c128(xphase, xamp.shape)):
        raise ValueError("ts_gain_compose: two contiguous complex128 tensors of one shape expected")
    if out is None:
        out = self.empty(tuple(xamp.shape), np.complex128)
    if not _is_c128(out, xamp.shape):
        raise ValueError("ts_gain_compose: out must be a contiguous complex128 tensor of the inputs' shape")
    self.check(self.lib.dm_ts_gain_compose(self.h, int(xamp.numel()), self.ptr(xamp), self.ptr(xphase), self.ptr(out)),
               "dm_ts_gain_compose")
    return out


def _ts_gain_apply(self, g, class_off, members, sky, out=None, accumulate=False):
    """Per-feed gains on stacked visibilities (dm_ts_gain_apply): out[r, f, c, t] (+)= G[r, f, c, t] sky[r, f, c, t] with
    G = (1 / n_c) sum_{(i, j) in class c} g_i conj(g_j) over the pair table (`class_off`, `members`) of
    `TransitTelescope.redundant_pairs` — `skysim.baseline_gains_host` restates G.  g is contiguous
    (g_nreal, nf, nfeed, ntime) with g_nreal 1 (one array for all realisations) or nreal; sky and out are
    (nreal, nf, npairs, ntime), contiguous or frequency slices [:, f0:f1] of contiguous arrays with one stride between
    realisations; out (a new tensor by default) must share no element with sky.  accumulate=True adds to what out holds:
    the noise `ts_noise` drew there, so the gains multiply the sky part only and the noise keeps its level — the convention
    of this package.  An empty class, a feed index outside g or more feeds than one time sample of LDS holds are refused before
    anything is launched."""
    if not (_is_c128(g) and g.dim() == 4) or _rstride_of(sky, True) is None:
        raise ValueError("ts_gain_apply: complex128 tensors g (g_nreal, nf, nfeed, ntime) and sky "
                         "(nreal, nf, npairs, ntime) expected")
    g_nreal, nf, nfeed, ntime = (int(v) for v in g.shape)
    nreal, _, npairs, _ = (int(v) for v in sky.shape)
    if tuple(sky.shape) != (nreal, nf, npairs, ntime) or g_nreal not in (1, nreal):
        raise ValueError("ts_gain_apply: g %s does not fit sky %s" % (tuple(g.shape), tuple(sky.shape)))
    off, offp, mem, memp = _class_table("ts_gain_apply", class_off, members)
    if off.shape[0] != npairs + 1:
        raise ValueError("ts_gain_apply: class_off (npairs + 1) and members (class_off[-1], 2) expected")
    if out is None:
        if accumulate:
            raise ValueError("ts_gain_apply: accumulate needs the buffer to add to")
        out = self.empty((nreal, nf, npairs, ntime), np.complex128)
    if (_rstride_of(out, True) is None or tuple(out.shape) != tuple(sky.shape) or (nreal > 1 and _rstride_of(out, True) != _rstride_of(sky, True))
            or _rows_overlap(sky, out)):
        raise ValueError("ts_gain_apply: out must be a complex128 tensor of sky's shape and strides that shares no "
                         "element with sky")
    rc = self.lib.dm_ts_gain_apply(self.h, nreal, g_nreal, nf, nfeed, npairs, ntime, offp, memp, self.ptr(g), self.ptr(sky),
                                   self.ptr(out), _rstride_of(sky, True), int(bool(accumulate)))
    self.check(rc, "dm_ts_gain_apply")
    return out


Context.ts_gain_coeff = _ts_gain_coeff
Context.ts_gain_compose = _ts_gain_compose
Context.ts_gain_apply = _ts_gain_apply


def _vis_stack(self, vis, class_off, members, w=None, g=None, feed_weight=None, out=None, wout=None):
    """Stack unstacked (per-feed-pair) visibilities into unique baselines (dm_vis_stack, DESIGN.md section 4.17;
    `timestream.vis_stack_host` restates it): with the class table of `TransitTelescope.redundant_pairs`,

        N = sum_{m in c} w_m conj(g_i) g_j V_m,  D = sum_{m in c} w_m |g_i|^2 |g_j|^2,  out = N / D,  wout = D / n_c

    and both 0 where D == 0.  vis (nreal, nf, nmem, ntime) complex128, contiguous or a frequency slice of a contiguous
    array; w float64 >= 0 (1 or nreal, nf, nmem, ntime), flags or inverse variances relative to the nominal per-pair
    noise; g (1 or nreal, nf, nfeed, ntime) complex128 calibration gains; feed_weight (nfeed) >= 0 on the host (0: a dead
    feed), the weight of a member is w_m feed_weight[i] feed_weight[j].  Returns (out complex128, wout float64), both
    (nreal, nf, npairs, ntime) with one stride between realisations.  wout is the `weight` of section 4.16: the inverse
    noise variance of out relative to the nominal one of the stacked baseline, exactly 1.0 for a complete class with
    unit weights and no gains.  The bits of a class do not depend on the batch it is stacked in."""
    rs = _rstride_of(vis, True)
    if rs is None:
        raise ValueError("vis_stack: complex128 tensor vis (nreal, nf, nmem, ntime) expected")
    nreal, nf, nmem, ntime = (int(v) for v in vis.shape)
    off, offp, mem, memp = _class_table("vis_stack", class_off, members)
    npairs = off.shape[0] - 1
    if mem.shape[0] != nmem:
        raise ValueError("vis_stack: vis has %d rows, the table %d members" % (nmem, mem.shape[0]))
    w_nreal = g_nreal = 1
    nfeed = int(mem.max()) + 1 if mem.size else 0
    if w is not None:
        w_nreal = _weights_arg("vis_stack", w, (nf, nmem, ntime), nreal)
    if g is not None:
        g_nreal, nfeed = _gains_arg("vis_stack", g, nreal, nf, ntime)
    fw, fwp, nfeed = _feed_weight_arg("vis_stack", feed_weight, nfeed, exact=g is not None)
    if out is None:
        out = self.empty((nreal, nf, npairs, ntime), np.complex128)
    if wout is None:
        wout = self.empty(tuple(out.shape), np.float64)
        if nreal > 1 and out.stride(0) != wout.stride(0):
            wout = self.torch.empty_strided(tuple(out.shape), tuple(out.stride()), dtype=self.torch.float64, device=out.device)
    ors = _rstride_of(out, True)
    if (ors is None or tuple(out.shape) != (nreal, nf, npairs, ntime) or tuple(wout.shape) != tuple(out.shape)
            or _rstride_of(wout, False) != ors):
        raise ValueError("vis_stack: out (complex128) and wout (float64) must be (nreal, nf, npairs, ntime) tensors with "
                         "one stride between realisations")
    rc = self.lib.dm_vis_stack(self.h, nreal, w_nreal, g_nreal, nf, nfeed, npairs, ntime, offp, memp, self.ptr(vis),
                               self.ptr(w), self.ptr(g), fwp, self.ptr(out), self.ptr(wout), rs, ors)
    self.check(rc, "dm_vis_stack")
    return out, wout


def _vis_expand(self, sky, class_off, members, g=None, out=None, accumulate=False):
    """A stacked sky spread over the feed pairs (dm_vis_expand; `timestream.vis_expand_host`
    restates it): out[r, f, m, t] (+)= g_i conj(g_j) sky[r, f, c(m), t] for member m = (i, j) of class c(m).  sky
    (nreal, nf, npairs, ntime) and out (nreal, nf, nmem, ntime) complex128, contiguous or frequency slices of contiguous
    arrays; g (1 or nreal, nf, nfeed, ntime) or None (the class row is copied).  accumulate=True adds to what out holds:
    the noise `ts_noise` drew there at the per-member level, so the gains multiply the sky part only."""
    rs = _rstride_of(sky, True)
    if rs is None:
        raise ValueError("vis_expand: complex128 tensor sky (nreal, nf, npairs, ntime) expected")
    nreal, nf, npairs, ntime = (int(v) for v in sky.shape)
    off, offp, mem, memp = _class_table("vis_expand", class_off, members)
    if off.shape[0] != npairs + 1:
        raise ValueError("vis_expand: sky has %d rows, the table %d classes" % (npairs, off.shape[0] - 1))
    nmem = mem.shape[0]
    g_nreal, nfeed = 1, (int(mem.max()) + 1 if mem.size else 0)
    if g is not None:
        g_nreal, nfeed = _gains_arg("vis_expand", g, nreal, nf, ntime)
    if out is None:
        if accumulate:
            raise ValueError("vis_expand: accumulate needs the buffer to add to")
        out = self.empty((nreal, nf, nmem, ntime), np.complex128)
    ors = _rstride_of(out, True)
    if ors is None or tuple(out.shape) != (nreal, nf, nmem, ntime):
        raise ValueError("vis_expand: out must be a complex128 tensor (nreal, nf, nmem, ntime)")
    rc = self.lib.dm_vis_expand(self.h, nreal, g_nreal, nf, nfeed, npairs, ntime, offp, memp, self.ptr(g), self.ptr(sky),
                                self.ptr(out), rs, ors, int(bool(accumulate)))
    self.check(rc, "dm_vis_expand")
    return out


Context.vis_stack = _vis_stack
Context.vis_expand = _vis_expand


def _sidereal_regrid(self, x, phi0, dphi, ntime, w=None, a=3, min_share=1.0, acc=None, variance=True):
    """One day of every row resampled onto the sidereal grid and written to, or added to, the accumulators of the stack
    (dm_sidereal_regrid; `timestream.sidereal_regrid_host` restates one day).  x (nf, nrow,
    nt_in) complex128, contiguous, sampled at phi0 + j dphi; w float64 of that shape or None (ones): the inverse noise
    variance of a sample relative to nominal, flagged where `w > 0` is false, and the data of a flagged sample reaches
    nothing.  Returns the accumulator tuple (sum, wsum, sq, hits), each (nf, nrow, ntime): complex128, float64, float64
    and int32.  acc=None allocates and writes it (sq and hits are None with variance=False); an `acc` given is added to
    and returned, its samples that are not valid this day untouched.  mean = sum / wsum where wsum > 0, and
    (sq - |sum|^2 / wsum) / (hits - 1) estimates the variance of one nominal input sample where hits >= 2.  wsum is the
    diagonal weight only: neighbouring samples share taps and are correlated.  The bits of a row do not depend on the
    batch it is in."""
    torch = self.torch
    nf, nrow, nt_in = _cube_arg("sidereal_regrid", x, w)
    ntime = int(ntime)
    shape = (nf, nrow, max(ntime, 0))
    accumulate = int(acc is not None)
    if acc is None and not variance:
        acc = (torch.empty(shape, dtype=torch.complex128, device=x.device),
               torch.empty(shape, dtype=torch.float64, device=x.device), None, None)
    acc = _out_tuple("sidereal_regrid", acc, (shape,) * 4, (torch.complex128, torch.float64, torch.float64, torch.int32),
                     x.device, optional=(2, 3), expected="acc must hold contiguous tensors (nf, nrow, ntime): sum complex128, "
                     "wsum float64, sq float64 or None, hits int32 or None")
    _same_gpu("sidereal_regrid", (x, w) + acc, "x, w and acc")
    s_, ws_, sq_, h_ = acc
    rc = self.lib.dm_sidereal_regrid(self.h, nf, nrow, nt_in, ntime, int(a), float(phi0), float(dphi), float(min_share),
                                     self.ptr(x), self.ptr(w), self.ptr(s_), self.ptr(ws_), self.ptr(sq_), self.ptr(h_),
                                     accumulate)
    self.check(rc, "dm_sidereal_regrid")
    return acc


Context.sidereal_regrid = _sidereal_regrid


def _rfi_flag(self, x, w=None, segment=1024, kernel_sigma=2.5, windows=(1, 2, 4, 8, 16), chi1=6.0, rho=1.5, niter=3,
              base=2.0, min_good=16, row_share=1.0, out=None):
    """RFI flags of one day along time by an iterated SumThreshold (dm_rfi_flag, DESIGN.md section 4.20;
    `timestream.rfi_flag_host` restates it).  x (nf, nrow, nt) complex128, contiguous; w float64 of that shape or None
    (ones), flagged on input where `w > 0` is false, and the data of such a sample reaches nothing.  Every series is cut
    into ceil(nt / segment) balanced segments that are judged independently.  Returns (w_out, noise, nflag, occupancy):
    w_out (nf, nrow, nt) float64 is w (or 1) where the sample is kept and 0 where it is flagged; noise (nf, nrow, nseg)
    float64 the noise scale of a segment, median |residual| / sqrt(ln 2), 0 where the segment had fewer than min_good
    usable samples and is flagged whole; nflag (nf, nrow) int32 the new flags of detection; occupancy (nf, nt) int32 the
    rows where detection flagged the sample anew.  With row_share < 1 a sample that detection flagged in more than
    row_share of the rows where it was not input flagged is flagged in every row of its frequency.  `out` takes that
    tuple of tensors to write into; its w_out may be w itself.  The bits of a row do not depend on the batch it is in."""
    return _rfi_flag_along(self, "time", x, w, segment, kernel_sigma, windows, chi1, rho, niter, base, min_good, row_share, out)


def _rfi_flag_freq(self, x, w=None, segment=1024, kernel_sigma=2.5, windows=(1, 2, 4, 8, 16), chi1=6.0, rho=1.5, niter=3,
                   base=2.0, min_good=16, row_share=1.0, out=None):
    """RFI flags along frequency (dm_rfi_flag_freq; `timestream.rfi_flag_freq_host` restates it):
    the method and the parameters of `rfi_flag` on the series x[:, row, j], with nf in the place of nt.  x (nf, nrow, nt)
    complex128, contiguous; w float64 of that shape or None.  Returns (w_out, noise, nflag, occupancy): w_out
    (nf, nrow, nt) float64; noise (nseg, nrow, nt) float64, nseg = ceil(nf / segment); nflag (nrow, nt) int32, the new
    flags of every series; occupancy (nf, nt) int32 — bit for bit what `rfi_flag` returns for the data transposed to
    (nt, nrow, nf), transposed back.  `out` takes that tuple of tensors to write into; its w_out may be w itself."""
    return _rfi_flag_along(self, "freq", x, w, segment, kernel_sigma, windows, chi1, rho, niter, base, min_good, row_share, out)


def _rfi_flag_along(self, axis, x, w, segment, kernel_sigma, windows, chi1, rho, niter, base, min_good, row_share, out):
    """The body of `rfi_flag` ("time") and `rfi_flag_freq` ("freq"): one method, and noise and nflag take the shape of x
    with the flagged axis cut into segments and dropped."""
    torch = self.torch
    who = "rfi_flag" if axis == "time" else "rfi_flag_freq"
    nf, nrow, nt = _cube_arg(who, x, w)
    segment = int(segment)
    if segment < 1:
        raise ValueError("%s: segment < 1" % who)
    windows = [int(v) for v in windows]
    if axis == "time":
        shapes, said = ((nf, nrow, -(-nt // segment)), (nf, nrow)), "noise (nf, nrow, nseg) float64, nflag (nf, nrow)"
    else:
        shapes, said = ((-(-nf // segment), nrow, nt), (nrow, nt)), "noise (nseg, nrow, nt) float64, nflag (nrow, nt)"
    out = _out_tuple(who, out, ((nf, nrow, nt),) + shapes + ((nf, nt),), (torch.float64, torch.float64, torch.int32, torch.int32),
                     x.device, expected="out must hold contiguous tensors w_out (nf, nrow, nt) float64, %s int32 and occupancy "
                     "(nf, nt) int32" % said)
    _same_gpu(who, (x, w) + out, "x, w and out")
    win = (c_int * max(len(windows), 1))(*windows)
    rc = getattr(self.lib, "dm_" + who)(self.h, nf, nrow, nt, segment, float(kernel_sigma), len(windows), win, float(chi1),
                                        float(rho), int(niter), float(base), int(min_good), float(row_share), self.ptr(x),
                                        self.ptr(w), *(self.ptr(o) for o in out))
    self.check(rc, "dm_" + who)
    return out


Context.rfi_flag = _rfi_flag
Context.rfi_flag_freq = _rfi_flag_freq

RFI_AXES = {"time": 0, "freq": 1}


def _rfi_dilate(self, w, eta, axis="time", ref=None, out=None):
    """Dilate the flags of w (nf, nrow, nt) float64 along `axis`, "time" or "freq", by the scale-invariant rank operator
    in exact integers (dm_rfi_dilate; `timestream.rfi_dilate_host` restates it): a sample is
    flagged when some window of its series that holds it has at least the share rint((1 - eta) 65536) / 65536 of its
    samples flagged.  eta in [0, 1); 0 changes nothing.  ref, of the shape of w or None: the samples where `ref > 0` is
    false are missing — they stay as they are and count neither as flags nor as length.  Returns (w_out, nadded): w_out is
    w where kept and 0 where newly flagged; nadded int32, the new flags of every series, (nf, nrow) along time and
    (nrow, nt) along frequency.  `out` takes that tuple of tensors to write into; its w_out may be w itself."""
    torch = self.torch
    if axis not in RFI_AXES:
        raise ValueError('rfi_dilate: axis is "time" or "freq"')
    if not (hasattr(w, "data_ptr") and w.dim() == 3 and w.dtype == torch.float64 and w.is_contiguous()):
        raise ValueError("rfi_dilate: contiguous float64 tensor w (nf, nrow, nt) expected")
    nf, nrow, nt = (int(v) for v in w.shape)
    if ref is not None:
        _weights_arg("rfi_dilate", ref, w.shape)
    out = _out_tuple("rfi_dilate", out, ((nf, nrow, nt), (nf, nrow) if axis == "time" else (nrow, nt)), (torch.float64, torch.int32),
                     w.device, expected="out must hold contiguous tensors w_out (nf, nrow, nt) float64 and nadded int32, "
                     "(nf, nrow) along time or (nrow, nt) along frequency")
    _same_gpu("rfi_dilate", (w, ref) + out, "w, ref and out")
    rc = self.lib.dm_rfi_dilate(self.h, nf, nrow, nt, RFI_AXES[axis], float(eta), self.ptr(w), self.ptr(ref),
                                self.ptr(out[0]), self.ptr(out[1]))
    self.check(rc, "dm_rfi_dilate")
    return out


Context.rfi_dilate = _rfi_dilate

DELAY_MODES = {"model": 0, "filter": 1, "inpaint": 2}


def _delay_pack(self, bases, device=None):
    """The basis table of `delay_fit` from a sequence of real matrices A_k (nf, r_k), numpy or torch: (table, ranks) with
    table a float64 device tensor that holds basis k as (r_k, nf) row-major behind the bases before it."""
    import numpy as np

    torch = self.torch
    mats = [np.ascontiguousarray(np.asarray(b.detach().cpu().numpy() if hasattr(b, "detach") else b, dtype=np.float64))
            for b in bases]
    if not mats or any(a.ndim != 2 for a in mats) or len({a.shape[0] for a in mats}) != 1:
        raise ValueError("delay_fit: basis must be a sequence of real matrices (nf, r_k) of one nf")
    table = np.concatenate([a.T.reshape(-1) for a in mats])
    dev = device if device is not None else "cuda:%d" % self.device
    return torch.from_numpy(table).to(dev), [int(a.shape[1]) for a in mats]


Context.delay_pack = _delay_pack


def _delay_fit(self, x, w=None, basis=None, basis_of=None, mode="inpaint", ridge=0.0, min_valid=None, out=None):
    """The band-limited weighted least-squares fit along frequency (dm_delay_fit, DESIGN.md section 4.23;
    `timestream.delay_fit_host` restates it).  x (nf, nrow, nt) complex128, contiguous; w float64 of that shape or None
    (ones): a sample is kept iff w > 0.  basis: a sequence of real matrices A_k (nf, r_k), or the pair (table, ranks)
    of `delay_pack`; basis_of (nrow,) int32 tensor (or a sequence of ints), the basis of every row.  mode "model",
    "filter" or "inpaint"; ridge >= 0, relative to the mean weight; min_valid: the kept samples a series needs to be
    solved (None: the rank).  Returns (x_out, w_out, info): x_out complex128 and w_out float64 of x's shape, info
    (nrow, nt) int32: 0 solved, -1 too few kept samples, -2 a basis_of entry outside the table, j + 1 a pivot of the
    Cholesky factorisation that was not positive at column j.  `out` takes that tuple of tensors to write into; its
    x_out may be x and its w_out may be w."""
    torch = self.torch
    if mode not in DELAY_MODES:
        raise ValueError('delay_fit: mode is "model", "filter" or "inpaint"')
    nf, nrow, nt = _cube_arg("delay_fit", x, w)
    if basis is None or basis_of is None:
        raise ValueError("delay_fit: basis and basis_of are required")
    if isinstance(basis, tuple) and len(basis) == 2 and hasattr(basis[0], "data_ptr") and basis[0].dim() == 1:
        table, ranks = basis[0], [int(r) for r in basis[1]]
    else:
        table, ranks = self.delay_pack(basis, device=x.device)
        if int(table.numel()) != nf * sum(ranks):
            raise ValueError("delay_fit: basis must be a sequence of real matrices (nf, r_k) with x's nf")
    if not (table.dtype == torch.float64 and table.is_contiguous() and int(table.numel()) == nf * sum(ranks)):
        raise ValueError("delay_fit: the basis table must be a contiguous float64 tensor of nf * sum(ranks) elements")
    if not hasattr(basis_of, "data_ptr"):
        basis_of = torch.tensor([int(v) for v in basis_of], dtype=torch.int32, device=x.device)
    if not (basis_of.dtype == torch.int32 and basis_of.is_contiguous() and tuple(basis_of.shape) == (nrow,)):
        raise ValueError("delay_fit: basis_of must be a contiguous int32 tensor (nrow,)")
    out = _out_tuple("delay_fit", out, ((nf, nrow, nt), (nf, nrow, nt), (nrow, nt)), (torch.complex128, torch.float64, torch.int32),
                     x.device, expected="out must hold contiguous tensors x_out (nf, nrow, nt) complex128, w_out "
                     "(nf, nrow, nt) float64 and info (nrow, nt) int32")
    _same_gpu("delay_fit", (x, w, table, basis_of) + out, "x, w, the basis table, basis_of and out")
    rk = (c_int * max(len(ranks), 1))(*ranks)
    rc = self.lib.dm_delay_fit(self.h, nf, nrow, nt, DELAY_MODES[mode], float(ridge), 0 if min_valid is None else int(min_valid),
                               len(ranks), rk, self.ptr(table), self.ptr(basis_of), self.ptr(x), self.ptr(w),
                               self.ptr(out[0]), self.ptr(out[1]), self.ptr(out[2]))
    self.check(rc, "dm_delay_fit")
    return out


Context.delay_fit = _delay_fit


def _ringmap(self, vis, group_off, members, v, scale, sinza, w=None, taper=None, parts=1, out=None, norm=None, norm2=None):
    """Ring maps: the stacked visibilities of every sample beamformed north-south (dm_ringmap, DESIGN.md section 4.25;
    `timestream.ringmap_host` restates it).  vis (nf, nrow, nt) complex128, contiguous; w float64 of that shape or None
    (ones): a sample is kept iff w > 0.  group_off (ngroup + 1) and members (group_off[-1]) are host integers: group g
    is the rows members[group_off[g]:group_off[g + 1]] of vis.  v and taper (per member; taper None: ones), scale (nf,)
    and sinza (nel,) are float64 device tensors, or anything numpy turns into such arrays.  parts 1 (the real part) or
    2 (real and imaginary part).  Returns (map, norm, norm2): map (nf, ngroup, parts, nel, nt) and norm = D,
    norm2 = D2 (nf, ngroup, nt), float64.  `out`, `norm` and `norm2` take tensors to write into; norm=False or
    norm2=False leaves that output out (None is returned in its place)."""
    who = "ringmap"
    nf, nrow, nt = _cube_arg(who, vis, w, "vis")
    dev = vis.device
    if parts not in (1, 2):
        raise ValueError("ringmap: parts is 1 or 2")
    off, offp, mem, memp = _group_table(who, group_off, members, nrow)
    ngroup, nmem = off.shape[0] - 1, mem.shape[0]
    v = _f64_table(who, v, nmem, "v", dev)
    taper = None if taper is None else _f64_table(who, taper, nmem, "taper", dev)
    scale = _f64_table(who, scale, nf, "scale", dev)
    sinza = _f64_table(who, sinza, None, "sinza", dev)
    nel = int(sinza.shape[0])
    out = _f64_out(who, out, (nf, ngroup, parts, nel, nt), "out", dev)
    norm = None if norm is False else _f64_out(who, norm, (nf, ngroup, nt), "norm", dev)
    norm2 = None if norm2 is False else _f64_out(who, norm2, (nf, ngroup, nt), "norm2", dev)
    _same_gpu(who, (vis, w, v, taper, scale, sinza, out, norm, norm2), "vis, w, v, taper, scale, sinza and the outputs")
    rc = self.lib.dm_ringmap(self.h, nf, nrow, nt, ngroup, offp, memp, self.ptr(v), self.ptr(taper), self.ptr(scale), nel,
                             self.ptr(sinza), int(parts), self.ptr(vis), self.ptr(w), self.ptr(out), self.ptr(norm),
                             self.ptr(norm2))
    self.check(rc, "dm_ringmap")
    return out, norm, norm2


Context.ringmap = _ringmap

DELAYSPEC_WEIGHTINGS = {"mask": 0, "weight": 1}


def delayspec_bins(nt, bins=None):
    """The bin table of `Context.delay_spectrum` as int32 (nbin + 1): None is one bin over all nt samples, an int bins of
    that many samples (the last one short), an array the table itself (ascending, within [0, nt])."""
    nt = int(nt)
    if bins is None:
        off = np.array([0, nt], dtype=np.int32)
    elif np.ndim(bins) == 0:
        n = int(bins)
        if n < 1:
            raise ValueError("delay_spectrum: bins of at least one sample expected")
        off = np.append(np.arange(0, nt, n), nt).astype(np.int32)
    else:
        off = np.ascontiguousarray(np.asarray(bins).reshape(-1), dtype=np.int32)
        if not np.array_equal(off, np.asarray(bins).reshape(-1)):
            raise ValueError("delay_spectrum: the bin table must hold integers")
    if off.shape[0] < 1 or off[0] < 0 or off[-1] > nt or np.any(np.diff(off) < 0):
        raise ValueError("delay_spectrum: the bin table (nbin + 1) must ascend within [0, nt]")
    return off


def _delay_spectrum(self, x, w=None, taper=None, step=None, nd=None, a0=None, weighting="mask", min_valid=1, bins=None,
                    out=None):
    """Delay power spectra with their window function (dm_delay_spectrum, DESIGN.md section 4.27;
    `timestream.delay_spectrum_host` restates it).  x (nf, nrow, nt) complex128, contiguous; w float64 of that shape or
    None (ones): a sample is kept iff w > 0.  taper (nf,) or None (ones) and step (nf,), the turns per delay step of every
    channel ((nu_f - nu_ref) dtau, `timestream.delay_grid`), are float64 device tensors, or anything numpy turns into
    such arrays.  nd delays a = 0 .. nd - 1 at (a - a0) steps (a0 None: nd // 2) and lags 0 .. nd - 1.  weighting "mask"
    (omega = 1 on kept samples) or "weight" (omega = w); a series with fewer than min_valid kept channels is dropped.
    bins: None (one bin over all samples), an int (bins of that many samples, the last one short) or the table (nbin + 1)
    of ascending sample offsets.  Returns (q, h, s1, s2, count): q and h (nrow, nbin, nd), s1 and s2 (nrow, nbin) float64,
    count (nrow, nbin) int32.  `out` takes that tuple of tensors to write into; None in the place of h, s1, s2 or count
    leaves that output out (None is returned in its place)."""
    torch = self.torch
    if weighting not in DELAYSPEC_WEIGHTINGS:
        raise ValueError('delay_spectrum: weighting is "mask" or "weight"')
    nf, nrow, nt = _cube_arg("delay_spectrum", x, w)
    if step is None or nd is None:
        raise ValueError("delay_spectrum: step and nd are required")
    nd = int(nd)
    a0 = nd // 2 if a0 is None else int(a0)
    min_valid = int(min_valid)
    if nd < 0 or (nd > 0 and not 0 <= a0 < nd) or min_valid < 1:
        raise ValueError("delay_spectrum: nd >= 0, a0 in [0, nd) and min_valid >= 1 expected")
    off = delayspec_bins(nt, bins)
    nbin = int(off.shape[0]) - 1
    step = _f64_table("delay_spectrum", step, nf, "step", x.device)
    taper = None if taper is None else _f64_table("delay_spectrum", taper, nf, "taper", x.device)
    out = _out_tuple("delay_spectrum", out, ((nrow, nbin, nd),) * 2 + ((nrow, nbin),) * 3, (torch.float64,) * 4 + (torch.int32,),
                     x.device, optional=(1, 2, 3, 4), expected="out must hold contiguous tensors q, h (nrow, nbin, nd), s1, s2 "
                     "(nrow, nbin) float64 and count (nrow, nbin) int32 (None for h, s1, s2 or count: not written)")
    _same_gpu("delay_spectrum", (x, w, taper, step) + out, "x, w, taper, step and the outputs")
    rc = self.lib.dm_delay_spectrum(self.h, nf, nrow, nt, nd, a0, DELAYSPEC_WEIGHTINGS[weighting], min_valid,
                                    self.ptr(taper), self.ptr(step), nbin, off.ctypes.data_as(ctypes.POINTER(c_int)),
                                    self.ptr(x), self.ptr(w), *(self.ptr(o) for o in out))
    self.check(rc, "dm_delay_spectrum")
    return out


Context.delay_spectrum = _delay_spectrum


def _formed_beam(self, vis, group_off, members, iu, iv, uvals, vvals, scale, env, k0, half, turn, sinth, yc0, yc1, w=None,
                 taper=None, parts=1, out=None, norm=None, norm2=None):
    """Formed beams: a tracking beam on every catalogue position from stacked visibilities (dm_formed_beam, DESIGN.md
    section 4.26; `timestream.formed_beam_host` restates it).  vis (nf, nrow, nt) complex128, contiguous; w float64 of
    that shape or None (ones): a sample is kept iff w > 0.  group_off (ngroup + 1), members, iu and iv (group_off[-1]),
    k0 and half (nsrc) are host integers and env (nf) host float64: group p is the rows
    members[group_off[p]:group_off[p + 1]] of vis, member m has u = uvals[iu[m]] and v = vvals[iv[m]], source s takes the
    samples k0[s] - half[s] .. k0[s] + half[s] (mod nt), half = -1 drops it.  uvals, vvals, taper (per member; None:
    ones), scale (nf,), turn, sinth, yc0 and yc1 (nsrc,) are float64 device tensors, or anything numpy turns into such
    arrays.  parts 1 (the real part) or 2.  Returns (beam, norm, norm2): beam (nf, ngroup, parts, nsrc), norm = D and
    norm2 = D2 (nf, ngroup, nsrc), float64.  `out`, `norm` and `norm2` take tensors to write into; norm=False or
    norm2=False leaves that output out (None is returned in its place)."""
    who = "formed_beam"
    nf, nrow, nt = _cube_arg(who, vis, w, "vis")
    dev = vis.device
    if parts not in (1, 2):
        raise ValueError("formed_beam: parts is 1 or 2")
    off, offp, mem, memp = _group_table(who, group_off, members, nrow)
    iu, iup = _iarr(iu)
    iv, ivp = _iarr(iv)
    if iu.shape != mem.shape or iv.shape != mem.shape:
        raise ValueError("formed_beam: iu and iv hold one index per member")
    ngroup, nmem = off.shape[0] - 1, mem.shape[0]
    k0, k0p = _iarr(k0)
    half, halfp = _iarr(half)
    if k0.ndim != 1 or half.shape != k0.shape:
        raise ValueError("formed_beam: k0 and half (nsrc,) expected")
    nsrc = k0.shape[0]
    if nsrc and (k0.min() < 0 or k0.max() >= max(nt, 1) or half.min() < -1 or 2 * int(half.max()) + 1 > nt):
        raise ValueError("formed_beam: k0 in [0, nt), half >= -1 and 2 half + 1 <= nt expected")
    env = np.ascontiguousarray(env, dtype=np.float64)
    if env.shape != (nf,) or not np.all(np.isfinite(env) & (env >= 0)):
        raise ValueError("formed_beam: env holds one finite value >= 0 per frequency")
    uvals, vvals = _f64_table(who, uvals, None, "uvals", dev), _f64_table(who, vvals, None, "vvals", dev)
    nu, nv = int(uvals.shape[0]), int(vvals.shape[0])
    if nmem and (iu.min() < 0 or iu.max() >= nu or iv.min() < 0 or iv.max() >= nv):
        raise ValueError("formed_beam: iu or iv points outside uvals or vvals")
    taper = None if taper is None else _f64_table(who, taper, nmem, "taper", dev)
    scale = _f64_table(who, scale, nf, "scale", dev)
    turn, sinth, yc0, yc1 = (_f64_table(who, t, nsrc, n, dev)
                             for t, n in ((turn, "turn"), (sinth, "sinth"), (yc0, "yc0"), (yc1, "yc1")))
    out = _f64_out(who, out, (nf, ngroup, parts, nsrc), "out", dev)
    norm = None if norm is False else _f64_out(who, norm, (nf, ngroup, nsrc), "norm", dev)
    norm2 = None if norm2 is False else _f64_out(who, norm2, (nf, ngroup, nsrc), "norm2", dev)
    _same_gpu(who, (vis, w, uvals, vvals, taper, scale, turn, sinth, yc0, yc1, out, norm, norm2), "vis, w, the tables and the outputs")
    rc = self.lib.dm_formed_beam(self.h, nf, nrow, nt, ngroup, offp, memp, iup, ivp, nu, self.ptr(uvals), nv, self.ptr(vvals),
                                 self.ptr(taper), self.ptr(scale), env.ctypes.data_as(ctypes.POINTER(c_dbl)), nsrc, k0p, halfp,
                                 self.ptr(turn), self.ptr(sinth), self.ptr(yc0), self.ptr(yc1), int(parts), self.ptr(vis),
                                 self.ptr(w), self.ptr(out), self.ptr(norm), self.ptr(norm2))
    self.check(rc, "dm_formed_beam")
    return out, norm, norm2


Context.formed_beam = _formed_beam


def _redcal_solve(self, vis, class_off, members, w=None, feed_weight=None, g0=None, damping=0.4, tol=1e-10, maxiter=500,
                  out=None):
    """Redundant-baseline calibration (dm_redcal_solve; `timestream.redcal_solve_host` restates
    it): the per-feed gains g (nreal, nf, nfeed, ntime) and class visibilities y (nreal, nf, npairs, ntime) that minimise
    sum_m omega_m |V_m - g_i conj(g_j) y_c|^2 per (realisation, frequency, time sample), by the damped alternating fixed
    point from g0 (ones when None).  vis, w and feed_weight as for `vis_stack`; omega_m = w_m fw_i fw_j, 0 for
    autocorrelations and for classes that constrain nothing.  Returns (g, y, info), info a dict of device tensors
    (nreal, nf, ntime): `iters` int32, `step` (the last step; the sample converged iff step < tol) and `chi2` at the
    result.  The solution carries the degeneracies of the table: `timestream.fix_degeneracies` removes them.  out: a dict
    of preallocated contiguous tensors under the names g, y, iters, step, chi2 (any subset).  The bits of a sample do not
    depend on the batch it is solved in."""
    rs = _rstride_of(vis, True)
    if rs is None:
        raise ValueError("redcal_solve: complex128 tensor vis (nreal, nf, nmem, ntime) expected")
    nreal, nf, nmem, ntime = (int(v) for v in vis.shape)
    off, offp, mem, memp = _class_table("redcal_solve", class_off, members)
    npairs = off.shape[0] - 1
    if mem.shape[0] != nmem:
        raise ValueError("redcal_solve: vis has %d rows, the table %d members" % (nmem, mem.shape[0]))
    nfeed = int(mem.max()) + 1 if mem.size else 0
    w_nreal = 1
    if w is not None:
        w_nreal = _weights_arg("redcal_solve", w, (nf, nmem, ntime), nreal)
    fw, fwp, nfeed = _feed_weight_arg("redcal_solve", feed_weight, nfeed)
    if g0 is not None:
        if not (_is_c128(g0) and g0.dim() == 4 and (int(g0.shape[0]), int(g0.shape[1]), int(g0.shape[3])) == (nreal, nf, ntime)
                and int(g0.shape[2]) >= nfeed and (feed_weight is None or int(g0.shape[2]) == nfeed)):
            raise ValueError("redcal_solve: g0 must be a contiguous complex128 tensor (nreal, nf, nfeed, ntime)")
        nfeed = int(g0.shape[2])
    shapes = dict(g=((nreal, nf, nfeed, ntime), np.complex128), y=((nreal, nf, npairs, ntime), np.complex128),
                  iters=((nreal, nf, ntime), np.int32), step=((nreal, nf, ntime), np.float64),
                  chi2=((nreal, nf, ntime), np.float64))
    out = _out_arg(self, "redcal_solve", out, shapes)
    rc = self.lib.dm_redcal_solve(self.h, nreal, w_nreal, nf, nfeed, npairs, ntime, offp, memp, self.ptr(vis), self.ptr(w),
                                  fwp, self.ptr(g0), float(damping), float(tol), int(maxiter), self.ptr(out["g"]),
                                  self.ptr(out["y"]), self.ptr(out["iters"]), self.ptr(out["step"]), self.ptr(out["chi2"]), rs)
    self.check(rc, "dm_redcal_solve")
    return out["g"], out["y"], dict(iters=out["iters"], step=out["step"], chi2=out["chi2"])


Context.redcal_solve = _redcal_solve


def _modelcal_solve(self, vis, model, class_off, members, interval, w=None, feed_weight=None, g0=None, active=None,
                    damping=0.5, tol=1e-10, maxiter=500, out=None):
    """Sky-model gain calibration (dm_modelcal_solve; `timestream.modelcal_solve_host` restates
    it): the per-feed gains g (nreal, nf, nfeed, nint), constant over a solution interval of `interval` consecutive samples
    (nint = ceil(ntime / interval), the last one may be shorter), that minimise sum_{t in q} sum_m omega_m |V_m - g_i
    conj(g_j) M_c|^2 per (realisation, frequency, interval) against the stacked model M (1 or nreal, nf, npairs, ntime), by
    the damped StEFCal fixed point from g0 (ones when None).  vis, w and feed_weight as for `vis_stack`; omega_m = w_m fw_i
    fw_j, 0 for autocorrelations.  active: an int32 tensor (nf, nint) or None; an interval whose entry is 0 is not solved
    and returns g0, iters 0, step 0, chi2 0 and gweight 0.  Returns (g, info), info a dict of device tensors: `iters`
    int32, `step` (the last step; the interval converged iff step < tol) and `chi2` at the result, each (nreal, nf, nint),
    and `gweight` (nreal, nf, nfeed, nint), the denominator of every gain at the result: the information it carries, 0
    where the gain is unconstrained.  A fixed model leaves one phase per connected component of the feed graph free:
    `timestream.modelcal_fix_phase` removes it.  out: a dict of preallocated contiguous tensors under the names g, iters,
    step, chi2, gweight (any subset).  The bits of an interval do not depend on the batch it is solved in."""
    rs = _rstride_of(vis, True)
    if rs is None:
        raise ValueError("modelcal_solve: complex128 tensor vis (nreal, nf, nmem, ntime) expected")
    nreal, nf, nmem, ntime = (int(v) for v in vis.shape)
    off, offp, mem, memp = _class_table("modelcal_solve", class_off, members)
    npairs = off.shape[0] - 1
    if mem.shape[0] != nmem:
        raise ValueError("modelcal_solve: vis has %d rows, the table %d members" % (nmem, mem.shape[0]))
    if not (_is_c128(model) and model.dim() == 4 and tuple(model.shape)[1:] == (nf, npairs, ntime)
            and int(model.shape[0]) in (1, nreal)):
        raise ValueError("modelcal_solve: model must be a contiguous complex128 tensor (1 or nreal, nf, npairs, ntime)")
    m_nreal = int(model.shape[0])
    interval = int(interval)
    nint = -(-ntime // interval) if interval >= 1 else 0
    nfeed = int(mem.max()) + 1 if mem.size else 0
    w_nreal = 1
    if w is not None:
        w_nreal = _weights_arg("modelcal_solve", w, (nf, nmem, ntime), nreal)
    fw, fwp, nfeed = _feed_weight_arg("modelcal_solve", feed_weight, nfeed)
    if g0 is not None:
        if not (_is_c128(g0) and g0.dim() == 4 and (int(g0.shape[0]), int(g0.shape[1]), int(g0.shape[3])) == (nreal, nf, nint)
                and int(g0.shape[2]) >= nfeed and (feed_weight is None or int(g0.shape[2]) == nfeed)):
            raise ValueError("modelcal_solve: g0 must be a contiguous complex128 tensor (nreal, nf, nfeed, nint)")
        nfeed = int(g0.shape[2])
    if active is not None and not (hasattr(active, "data_ptr") and active.dtype == self.torch.int32 and active.is_contiguous()
                                   and tuple(active.shape) == (nf, nint)):
        raise ValueError("modelcal_solve: active must be a contiguous int32 tensor (nf, nint)")
    shapes = dict(g=((nreal, nf, nfeed, nint), np.complex128), iters=((nreal, nf, nint), np.int32),
                  step=((nreal, nf, nint), np.float64), chi2=((nreal, nf, nint), np.float64),
                  gweight=((nreal, nf, nfeed, nint), np.float64))
    out = _out_arg(self, "modelcal_solve", out, shapes)
    rc = self.lib.dm_modelcal_solve(self.h, nreal, w_nreal, m_nreal, nf, nfeed, npairs, ntime, interval, offp, memp,
                                    self.ptr(vis), self.ptr(model), self.ptr(w), fwp, self.ptr(g0), self.ptr(active),
                                    float(damping), float(tol), int(maxiter), self.ptr(out["g"]), self.ptr(out["iters"]),
                                    self.ptr(out["step"]), self.ptr(out["chi2"]), self.ptr(out["gweight"]), rs)
    self.check(rc, "dm_modelcal_solve")
    return out["g"], dict(iters=out["iters"], step=out["step"], chi2=out["chi2"], gweight=out["gweight"])


Context.modelcal_solve = _modelcal_solve


def _toeplitz_max_rhs(self, n):
    """The most right-hand sides one `dm_toeplitz_solve` call takes for order n (0: the order does not fit in LDS)."""
    return int(self.lib.dm_toeplitz_max_rhs(int(n)))


def _toeplitz_solve(self, col, b, ridge=0.0, diag=False):
    """`batch` Hermitian positive-definite Toeplitz systems on the device (dm_toeplitz_solve, the Levinson recursion of
    DESIGN.md section 4.16; `timestream.toeplitz_levinson_host` restates it): col (batch, n) complex128 first columns
    (numpy or device; Im c_0 is ignored), b (batch, nrhs, n) right-hand sides.  `ridge` adds ridge * c_0 to c_0 on a copy.
    Returns (x, info): new device tensors (batch, nrhs, n) complex128 and (batch,) int32 — 0 solved, k < n: not positive
    definite at step k, n: c_0 <= 0; such a system's solutions are zeros.  More right-hand sides than
    `toeplitz_max_rhs(n)` go through several calls (the bits of a solution do not depend on its companions).

    diag=True: returns (x, info, d) with d (batch, n) float64 the diagonal of the inverse of the system as solved, that
    is of (A + ridge c_0 I)^-1 (dm_toeplitz_solve_diag; zeros for info != 0; taken from the first call when the right-hand
    sides are split).  x and info have the bits of diag=False."""
    torch = self.torch
    col = self.to_device(np.asarray(col, dtype=np.complex128)) if not hasattr(col, "data_ptr") else col
    b = self.to_device(np.asarray(b, dtype=np.complex128)) if not hasattr(b, "data_ptr") else b
    if col.dim() != 2 or b.dim() != 3 or not (col.is_complex() and col.element_size() == 16) or not (
            b.is_complex() and b.element_size() == 16):
        raise ValueError("toeplitz_solve: complex128 col (batch, n) and b (batch, nrhs, n) expected")
    batch, n = (int(v) for v in col.shape)
    nrhs = int(b.shape[1])
    if tuple(b.shape) != (batch, nrhs, n) or n < 1 or nrhs < 1:
        raise ValueError("toeplitz_solve: b %s does not fit col %s" % (tuple(b.shape), tuple(col.shape)))
    ridge = float(ridge)
    if not (ridge >= 0.0 and np.isfinite(ridge)):
        raise ValueError("toeplitz_solve: ridge must be finite and not negative")
    most = self.toeplitz_max_rhs(n)
    if most < 1:
        raise ValueError("toeplitz_solve: a system of order %d does not fit in the LDS of a CU" % n)
    col = col.contiguous()
    if ridge > 0.0:
        col = col.clone()
        col[:, 0] += ridge * col[:, 0].real
    x = b.clone(memory_format=torch.contiguous_format)
    info = self.empty((batch,), np.int32)
    d = self.empty((batch, n), np.float64) if diag else None

    def call(part, first):
        if diag and first:
            self.check(self.lib.dm_toeplitz_solve_diag(self.h, n, int(part.shape[1]), batch, self.ptr(col), self.ptr(part),
                                                       self.ptr(d), self.ptr(info)), "dm_toeplitz_solve_diag")
        else:
            self.check(self.lib.dm_toeplitz_solve(self.h, n, int(part.shape[1]), batch, self.ptr(col), self.ptr(part),
                                                  self.ptr(info)), "dm_toeplitz_solve")

    if nrhs <= most:
        call(x, True)
        return (x, info, d) if diag else (x, info)
    for r0 in range(0, nrhs, most):   # info depends on col alone: every call writes the same values
        part = x[:, r0 : r0 + most].contiguous()
        call(part, r0 == 0)
        x[:, r0 : r0 + most] = part
    return (x, info, d) if diag else (x, info)


def _toeplitz_inverse_diag(self, col, ridge=0.0):
    """The diagonals of the inverses of `batch` Hermitian positive-definite Toeplitz matrices given by their first
    columns col (batch, n) complex128 (numpy or device), with ridge * c_0 added to c_0: (d (batch, n) float64, info
    (batch,) int32) on the device, by dm_toeplitz_solve_diag without right-hand sides.  info as `toeplitz_solve`; a
    failed system has d = 0.  Host statement: `timestream.toeplitz_inverse_diag_host`."""
    col = self.to_device(np.asarray(col, dtype=np.complex128)) if not hasattr(col, "data_ptr") else col
    if col.dim() != 2 or not (col.is_complex() and col.element_size() == 16) or int(col.shape[1]) < 1:
        raise ValueError("toeplitz_inverse_diag: complex128 col (batch, n) expected")
    batch, n = (int(v) for v in col.shape)
    ridge = float(ridge)
    if not (ridge >= 0.0 and np.isfinite(ridge)):
        raise ValueError("toeplitz_inverse_diag: ridge must be finite and not negative")
    col = col.contiguous()
    if ridge > 0.0:
        col = col.clone()
        col[:, 0] += ridge * col[:, 0].real
    d = self.empty((batch, n), np.float64)
    info = self.empty((batch,), np.int32)
    self.check(self.lib.dm_toeplitz_solve_diag(self.h, n, 0, batch, self.ptr(col), self.ptr(None), self.ptr(d),
                                               self.ptr(info)), "dm_toeplitz_solve_diag")
    return d, info


def _mmode_weights(self, weight, nf, npairs, ntime):
    """The weights of `mmode_transform_weighted` as a device tensor (S, ntime) float64 with S = nf * npairs, nf or 1, and
    the shape of the systems along (frequency, pair); a shape that does not broadcast, a negative or a non-finite weight
    raise ValueError."""
    torch = self.torch
    if hasattr(weight, "data_ptr"):
        w = weight
        if w.dtype != torch.float64:
            raise ValueError("mmode_transform_weighted: float64 weights expected")
        bad = bool((~(torch.isfinite(w) & (w >= 0))).any()) if w.numel() else False
    else:
        w = np.asarray(weight, dtype=np.float64)
        bad = bool(w.size) and not bool(np.all(np.isfinite(w) & (w >= 0)))
    if tuple(w.shape) not in ((nf, npairs, ntime), (nf, ntime), (ntime,)):
        raise ValueError("mmode_transform_weighted: weights %s are not (nf, npairs, ntime), (nf, ntime) or (ntime,) of X "
                         "(%d, %d, %d)" % (tuple(w.shape), nf, npairs, ntime))
    if bad:
        raise ValueError("mmode_transform_weighted: weights must be finite and not negative")
    if not hasattr(w, "data_ptr"):
        w = self.to_device(w)
    lead = {3: (nf, npairs), 2: (nf, 1), 1: (1, 1)}[w.dim()]                  # the systems along (frequency, pair)
    return w.reshape(-1, ntime).contiguous(), lead


def _mmode_transform_weighted(self, X, weight, mmax, ridge=0.0, out=None, inflation=False):
    """Weighted least-squares m-modes of flagged timestreams on the device: the a_k, |k| <= mmax,
    that minimise sum_t w_t |x_t - sum_k a_k e^{2 pi i k t / ntime}|^2 (+ ridge * mean(w) * |a|^2), in the layout of
    `mmode_transform`, (mmax + 1, nf, 2, npairs): slot 1 is the conjugate of the -m mode, zero for m = 0.

    X (nf, npairs, ntime) complex128 on the device; `weight` float64 >= 0, numpy or device, of shape (nf, npairs, ntime),
    (nf, ntime) or (ntime,).  Returns (out, info) with info (nf, npairs) int32: 0 solved, -1 not solved (fewer than
    2 mmax + 1 samples of weight > 0 and ridge = 0, or none at all: the modes are zeros), > 0 the code of `toeplitz_solve`.

    The right-hand sides are `mmode_transform` of w x; the first columns c_d = mean_t w_t e^{-2 pi i d t / ntime},
    d <= 2 mmax, one ZGEMM of the weights against the twiddle table; per (frequency, baseline) one Toeplitz system of
    order 2 mmax + 1 (`toeplitz_solve`).  Without a pair axis the baselines of a frequency (of all frequencies for
    (ntime,)) are right-hand sides of one system.  A row of constant weight w_0 has A = w_0 I exactly and gets that
    column, so data without flags gives the bits of `mmode_transform`.  Host statement:
    `timestream.mmodes_weighted_host`.  (Device weights are checked with a torch reduction and a read-back.)

    inflation=True: a third return value, float64 (mmax + 1, nf, 2, npairs) in the layout of the modes, the noise
    variance of every mode relative to that of complete data: with circular white noise of per-sample variance
    ntime * noisepower on the data, Cov(a) = noisepower A^-1 and the pseudo-covariance vanishes, so the noise of an
    m-block stays diagonal with variance noisepower * d, d = diag(A^-1) at k = +m (slot 0) and k = -m (slot 1) — from
    the same launch as the modes (`toeplitz_solve(diag=True)`).  Exactly 1.0 at (m = 0, slot 1), where the data holds a
    zero and the nominal model unit noise; exactly 1 / w_0 on a row of constant weight w_0 (1.0 for complete data) when
    ridge = 0; 0.0 on rows with info != 0, whose modes are zeros and carry no noise; without a pair axis the diagonal of
    the one system for all its baselines.  For ridge = 0 this is the exact variance ratio; for ridge > 0 it is the
    diagonal of A_rho^-1, an upper bound of the variance, A_rho^-1 A A_rho^-1 <= A_rho^-1."""
    torch = self.torch
    if X.dim() != 3 or not (X.is_complex() and X.element_size() == 16):
        raise ValueError("mmode_transform_weighted: X (nf, npairs, ntime) complex128 expected")
    nf, npairs, ntime = (int(v) for v in X.shape)
    mmax, ridge = int(mmax), float(ridge)
    N = 2 * mmax + 1
    if mmax < 0 or ntime < N:
        raise ValueError("mmode_transform_weighted: %d time samples cannot hold m up to %d" % (ntime, mmax))
    if not (ridge >= 0.0 and np.isfinite(ridge)):
        raise ValueError("mmode_transform_weighted: ridge must be finite and not negative")
    w, lead = _mmode_weights(self, weight, nf, npairs, ntime)
    if out is None:
        out = self.empty((mmax + 1, nf, 2, npairs), np.complex128)
    if tuple(out.shape) != (mmax + 1, nf, 2, npairs) or not out.is_contiguous():
        raise ValueError("mmode_transform_weighted: out must be a contiguous (mmax + 1, nf, 2, npairs) tensor")
    S = int(w.shape[0])
    if nf == 0 or npairs == 0:
        info = self.zeros((nf, npairs), np.int32)
        return (out, info, self.zeros((mmax + 1, nf, 2, npairs), np.float64)) if inflation else (out, info)
    if self.toeplitz_max_rhs(N) < 1:
        raise ValueError("mmode_transform_weighted: systems of order %d do not fit in the LDS of a CU" % N)
    bm = self.mmode_transform(X * w.view(lead + (ntime,)), mmax)                                   # (mmax + 1, nf, 2, npairs)
    # c[s, d] = (1 / ntime) sum_t w[s, t] e^{-2 pi i d t / ntime}
    W2 = self.mmode_twiddle(ntime, 2 * mmax)
    col = self.empty((S, N), np.complex128)
    self.zgemm(w.to(torch.complex128), W2, col, S, N, ntime, rsA=ntime, csA=1, rsB=N, csB=1, ldc=N)
    wmin, wmax = w.amin(dim=1), w.amax(dim=1)
    flat = (wmin == wmax) & (wmin > 0)
    e0 = torch.zeros((S, N), dtype=torch.complex128, device=col.device)
    e0[:, 0] = wmin
    col = torch.where(flat[:, None], e0, col)
    short = (w > 0).sum(dim=1) < (N if ridge == 0.0 else 1)     # (the ridge is relative to mean(w): 0 for an empty row)
    e0[:, 0] = 1.0
    col = torch.where(short[:, None], e0, col)
    # right-hand sides in k = -mmax .. mmax order: (nf, npairs, N), the pair axis the right-hand sides of a system
    B = self.empty((nf, npairs, N), np.complex128)
    B[:, :, mmax:] = bm[:, :, 0].permute(1, 2, 0)
    if mmax > 0:
        B[:, :, :mmax] = bm[1:, :, 1].conj().permute(1, 2, 0).flip(-1)
    B = B.view(S, (nf * npairs) // S, N)
    B = torch.where(short[:, None, None], torch.zeros_like(B), B)
    if inflation:
        x, info, d = self.toeplitz_solve(col, B, ridge=ridge, diag=True)
    else:
        x, info = self.toeplitz_solve(col, B, ridge=ridge)
    x = x.view(nf, npairs, N)
    out[:, :, 0] = x[:, :, mmax:].permute(2, 0, 1)
    out[0, :, 1].zero_()
    if mmax > 0:
        out[1:, :, 1] = x[:, :, :mmax].flip(-1).conj().permute(2, 0, 1)
    info = torch.where(short, torch.full_like(info, -1), info)
    if inflation:
        d = torch.where(short[:, None], torch.zeros_like(d), d)                  # not solved: zeros, no noise
        d = d.view(lead + (N,)).expand(nf, npairs, N)
        infl = self.empty((mmax + 1, nf, 2, npairs), np.float64)
        infl[:, :, 0] = d[:, :, mmax:].permute(2, 0, 1)
        infl[0, :, 1] = 1.0
        if mmax > 0:
            infl[1:, :, 1] = d[:, :, :mmax].flip(-1).permute(2, 0, 1)
        return out, info.view(lead).expand(nf, npairs).contiguous(), infl
    return out, info.view(lead).expand(nf, npairs).contiguous()


Context.toeplitz_max_rhs = _toeplitz_max_rhs
Context.toeplitz_solve = _toeplitz_solve
Context.toeplitz_inverse_diag = _toeplitz_inverse_diag
Context.mmode_transform_weighted = _mmode_transform_weighted


def _svd_chain(self, beam_m, noisew, polsvcut, skip_svd_inv=False, max_bytes=None, lmin=None):
    """beam_m: device (nblk, F, T, P, L) c128; noisew: device (F, T) f64.
    Returns dict of device tensors + host nmodes (nblk, F) + sweeps[4].
    ``lmin`` (nblk ints, optional): block i is exactly zero in its columns l < lmin[i] (the m-block of m = lmin[i]) —
    the chains then work on the columns l >= lmin only (dm_svd_chain_lmin); the products come back padded.
    The (m, frequency) chains are independent: when the working set of all of them (augmented matrices,
    their row-mixing temporaries, Gram / eigenvector matrices and the eigensolver's workspace) exceeds
    ``max_bytes`` (default: DRIFTMI_SVD_CHUNK_GB, 96) the frequencies go through the library in slices."""
    nblk, F, T, P, L = [int(x) for x in beam_m.shape]
    K = min(L, T)
    _tm = os.environ.get("DRIFTMI_TIMING") == "1"   # (host-side stopwatch of this call on stderr: allocation / library / copies)
    if _tm:
        import sys
        import time
        self.sync(); _t0 = time.perf_counter(); _tc = 0.0
    out = dict(
        beam_svd=self.empty((nblk, F, K, P, L), np.complex128),
        invbeam_svd=None if skip_svd_inv else self.empty((nblk, F, P, L, K), np.complex128),
        beam_ut=self.empty((nblk, F, K, T), np.complex128),
        singularvalues=self.empty((nblk, F, K), np.float64),
    )
    if max_bytes is None:
        max_bytes = float(os.environ.get("DRIFTMI_SVD_CHUNK_GB", "96")) * (1 << 30)
    per_chain = 16.0 * (2.0 * T * (P * L + T) + 16.0 * T * T)
    fc = max(1, min(F, int(max_bytes // max(per_chain * max(nblk, 1), 1.0))))
    nmodes_all = np.zeros((nblk, F), dtype=np.int64)
    sweeps_all = [0, 0, 0, 0]
    lm = None
    if lmin is not None:
        lm_keep, lm = _iarr(np.clip(np.asarray(lmin, dtype=np.int64), 0, L - 1))
        if len(lm_keep) != nblk:
            raise ValueError("svd_chain: one lmin per block expected")
    for f0 in range(0, F, fc):
        f1 = min(F, f0 + fc)
        whole = f0 == 0 and f1 == F
        bm = beam_m if whole else beam_m[:, f0:f1].contiguous()
        nw = noisew if whole else noisew[f0:f1].contiguous()
        o = out if whole else dict(
            beam_svd=self.empty((nblk, f1 - f0, K, P, L), np.complex128),
            invbeam_svd=None if skip_svd_inv else self.empty((nblk, f1 - f0, P, L, K), np.complex128),
            beam_ut=self.empty((nblk, f1 - f0, K, T), np.complex128),
            singularvalues=self.empty((nblk, f1 - f0, K), np.float64))
        nmodes = (c_int * max(nblk * (f1 - f0), 1))()
        sweeps = (c_int * 4)()
        if _tm:
            self.sync(); _t1 = time.perf_counter()
        rc = self.lib.dm_svd_chain_lmin(self.h, nblk, f1 - f0, T, P, L, lm, self.ptr(bm), self.ptr(nw), float(polsvcut),
                                        self.ptr(o["beam_svd"]), self.ptr(o["invbeam_svd"]), self.ptr(o["beam_ut"]),
                                        self.ptr(o["singularvalues"]), nmodes, sweeps)
        if _tm:
            self.sync(); _tc += time.perf_counter() - _t1
        self.check(rc, "dm_svd_chain_lmin")
        nmodes_all[:, f0:f1] = np.array(nmodes[: nblk * (f1 - f0)], dtype=np.int64).reshape(nblk, f1 - f0)
        sweeps_all = [max(a, int(b)) for a, b in zip(sweeps_all, sweeps)]
        if not whole:
            for k in ("beam_svd", "invbeam_svd", "beam_ut", "singularvalues"):
                if out[k] is not None:
                    out[k][:, f0:f1].copy_(o[k])
            del o, bm
    out["nmodes"] = nmodes_all
    out["sweeps"] = sweeps_all
    if _tm:
        self.sync()
        _tt = time.perf_counter() - _t0
        sys.stderr.write("[timing] svd_chain %d blocks, %d slice(s): %.3f s, of it %.3f s in the library, %.3f s allocation + copies\n"
                         % (nblk, -(-F // fc), _tt, _tc, _tt - _tc))
    return out


def _block_offsets(ndofs):
    ndofs = np.asarray(ndofs, dtype=np.int64)
    off = np.concatenate([[0], np.cumsum(ndofs * ndofs)])
    return off[:-1].copy(), int(off[-1])


def _project_cov(self, beam_svd, svnum, cl_pfl, out, out_off, npol=None, polmask=None, l0=None, zero_first=True,
                 symmetric=False):
    """``symmetric``: the caller has checked cl[p,q,f,f',l] == cl[p,q,f',f,l]; only then may the library
    form the frequency blocks f' >= f alone and mirror them (the reference accepts any array)."""
    nblk, F, K, P, L = [int(x) for x in beam_svd.shape]
    sv, svp = _iarr(svnum)
    off, offp = _larr(out_off)
    npol = P if npol is None else int(npol)
    pm = pmp = None
    if polmask is not None:
        pm, pmp = _iarr(polmask)
    l0a = l0p = None
    if l0 is not None:
        l0a, l0p = _iarr(l0)
    rc = self.lib.dm_project_cov(self.h, nblk, F, K, P, L, self.ptr(beam_svd), svp, l0p, self.ptr(cl_pfl), npol, pmp,
                                 self.ptr(out), offp, int(bool(zero_first)) | (2 if symmetric else 0))
    self.check(rc, "dm_project_cov")


def _band_args(self, beam_svd, svnum, l0, cl_bands, evecs, evecs_off, nmodes, evals, evals_off):
    """What dm_fisher, dm_qestimate and dm_psmc_alt take alike: (their arguments from nblk to evals_off_host in the
    order of include/driftmi.h, nblk, nbands, nmodes as an int32 array).  The pointers keep their host arrays alive."""
    nblk, F, K, P, L = [int(x) for x in beam_svd.shape]
    nbands = int(cl_bands.shape[0])
    sv, svp = _iarr(svnum)
    l0a, l0p = _iarr(l0)
    eo, eop = _larr(evecs_off)
    vo, vop = _larr(evals_off)
    nm, nmp = _iarr(nmodes)
    args = (nblk, F, K, P, L, self.ptr(beam_svd), svp, l0p, nbands, self.ptr(cl_bands), self.ptr(evecs), eop, nmp,
            self.ptr(evals), vop)
    return args, nblk, nbands, nm


def _fisher(self, beam_svd, svnum, l0, cl_bands, evecs, evecs_off, nmodes, evals, evals_off, cl_symmetric=False):
    """Per-m Fisher matrices (nblk, nbands, nbands) complex; see dm_fisher in include/driftmi.h."""
    args, nblk, nbands, nm = _band_args(self, beam_svd, svnum, l0, cl_bands, evecs, evecs_off, nmodes, evals, evals_off)
    out = self.empty((nblk, nbands, nbands), np.complex128)
    rc = self.lib.dm_fisher(self.h, *args, self.ptr(out), int(bool(cl_symmetric)))
    self.check(rc, "dm_fisher")
    return out


Context.fisher = _fisher


QEST_NOISE, QEST_CROSSPOWER, QEST_ZERO_MEAN = 1, 2, 4   # flags of dm_qestimate (include/driftmi.h)


def _qestimate(self, beam_svd, svnum, l0, cl_bands, evecs, evecs_off, nmodes, evals, evals_off, R, x, x_off, y=None,
               noise=False, crosspower=False, zero_mean=False):
    """Band-power q of R data columns per m-block, (nblk, nbands [+1], R) f64 on the device; see dm_qestimate in
    include/driftmi.h.  x (and y): the (nmodes_b x R) c128 columns of every block at element offsets x_off."""
    args, nblk, nbands, nm = _band_args(self, beam_svd, svnum, l0, cl_bands, evecs, evecs_off, nmodes, evals, evals_off)
    xo, xop = _larr(x_off)
    flags = (QEST_NOISE if noise else 0) | (QEST_CROSSPOWER if crosspower else 0) | (QEST_ZERO_MEAN if zero_mean else 0)
    out = self.empty((nblk, nbands + (1 if noise else 0), int(R)), np.float64)
    rc = self.lib.dm_qestimate(self.h, *args, int(R), self.ptr(x), None if y is None else self.ptr(y), xop, flags,
                               self.ptr(out))
    self.check(rc, "dm_qestimate")
    return out


Context.qestimate = _qestimate


PSMC_NORMAL, PSMC_RADEMACHER = 0, 1   # kinds of dm_psmc_draw (include/driftmi.h)


def _psmc_draw(self, ms, nmodes, R, seed, stream=0, kind=PSMC_NORMAL, power=0, s0=0, evals=None, evals_off=None):
    """Sample columns of the Monte-Carlo estimators, (sum_b nmodes_b * R,) c128 on the device: block b's
    (nmodes_b x R) draws back to back; see dm_psmc_draw in include/driftmi.h."""
    mm, mmp = _iarr(ms)
    nm, nmp = _iarr(nmodes)
    off = np.concatenate([[0], np.cumsum(nm.astype(np.int64) * int(R))])
    xo, xop = _larr(off[:-1])
    vop = None
    if evals_off is not None:
        vo, vop = _larr(evals_off)
    out = self.empty((max(int(off[-1]), 1),), np.complex128)
    rc = self.lib.dm_psmc_draw(self.h, len(mm), mmp, nmp, None if evals is None else self.ptr(evals), vop,
                               int(seed) & 0xFFFFFFFFFFFFFFFF, int(stream), int(kind), int(power), int(s0), int(R),
                               self.ptr(out), xop)
    self.check(rc, "dm_psmc_draw")
    return out[: int(off[-1])]


def _sky_draw(self, T, jglobal, rowoff, nfreq, row0, nrows, M, seed, stream, first, nreal, out, strides):
    """Correlated a_lm draws of one group into `out` (c128 on the device, any shape): T (L, n, n) f64 roots on the
    device, `rowoff` (n) the offset of every component in `out` and `strides` those of (realisation, l, m), all in complex
    elements; see dm_sky_draw in include/driftmi.h.  Every element the call addresses must lie inside `out`."""
    L, n = int(T.shape[0]), int(T.shape[1])
    if tuple(T.shape) != (L, n, n) or T.is_complex() or not T.is_contiguous():
        raise ValueError("sky_draw: need contiguous float64 roots (L, n, n), got %s" % (tuple(T.shape),))
    if not (out.is_contiguous() and out.is_complex()):
        raise ValueError("sky_draw: need a contiguous complex128 output")
    jg, jgp = _iarr(jglobal)
    ro, rop = _larr(rowoff)
    sr, sl, sm = [int(x_) for x_ in strides]
    if jg.shape != (n,) or ro.shape != (n,) or not 0 <= int(row0) <= int(row0) + int(nrows) <= n or not 1 <= int(M) <= L:
        raise ValueError("sky_draw: tables, row range or M do not match the roots")
    if nrows > 0 and nreal > 0:
        rows = ro[int(row0) : int(row0) + int(nrows)]
        last = int(rows.max()) + (int(nreal) - 1) * sr + (L - 1) * sl + (int(M) - 1) * sm
        if int(rows.min()) < 0 or min(sr, sl, sm) < 0 or last >= out.numel():
            raise ValueError("sky_draw: the call would write outside its output")
    rc = self.lib.dm_sky_draw(self.h, n, L, int(M), self.ptr(T), n, n * n, jgp, rop, int(nfreq), int(row0), int(nrows),
                              int(seed) & 0xFFFFFFFFFFFFFFFF, int(stream), int(first), int(nreal), self.ptr(out), sr, sl, sm)
    self.check(rc, "dm_sky_draw")


def _source_alm(self, z, sth, phi, flux, lmax, m_lo, m_hi, out=None, max_bytes=2 << 30):
    """a_lm (nf, npol, lmax + 1, m_hi - m_lo + 1) c128 on the device of point sources at (z, sth, phi) (nsrc each) with
    fluxes (nf, npol, nsrc), npol 1 or 4; numpy or float64 device tensors (dm_source_alm in include/driftmi.h)."""
    def dev(a):
        if not hasattr(a, "data_ptr"):
            a = self.to_device(np.asarray(a, dtype=np.float64))
        if a.dtype != self.torch.float64:
            raise ValueError("source_alm: float64 expected")
        return a.contiguous()

    z, sth, phi, flux = dev(z), dev(sth), dev(phi), dev(flux)
    if flux.dim() != 3:
        raise ValueError("source_alm: flux (nf, npol, nsrc) expected")
    nf, npol, nsrc = (int(v) for v in flux.shape)
    if not (tuple(z.shape) == tuple(sth.shape) == tuple(phi.shape) == (nsrc,)):
        raise ValueError("source_alm: z, sth and phi need one entry per source")
    lmax, m_lo, m_hi = int(lmax), int(m_lo), int(m_hi)
    if lmax < 0 or not 0 <= m_lo <= m_hi:
        raise ValueError("source_alm: lmax >= 0 and 0 <= m_lo <= m_hi expected")
    shape = (nf, npol, lmax + 1, m_hi - m_lo + 1)
    if out is None:
        out = self.empty(shape, np.complex128)
    if tuple(out.shape) != shape or not out.is_contiguous() or not (out.is_complex() and out.element_size() == 16):
        raise ValueError("source_alm: out must be a contiguous %s complex128 tensor" % (shape,))
    rc = self.lib.dm_source_alm(self.h, nsrc, self.ptr(z), self.ptr(sth), self.ptr(phi), nf, npol, self.ptr(flux), lmax, m_lo,
                                m_hi, self.ptr(out), int(max_bytes))
    self.check(rc, "dm_source_alm")
    return out


def _alm_at_points(self, z, sth, phi, ms, alm, lmax, nf, npol, strides, out=None, accumulate=False, max_bytes=2 << 30):
    """Values (npts, npol, nf) f64 on the device of the coefficients `alm` at the points (z, sth, phi) (npts each; numpy or
    float64 device tensors): `alm` is a contiguous complex128 device tensor of any shape and a^p_lm(f) of column j
    (m = ms[j]) sits at f strides[0] + p strides[1] + l strides[2] + j strides[3] complex elements in it
    (dm_alm_at_points in include/driftmi.h).  Every element the call addresses must lie inside `alm`: checked here."""
    def dev(a):
        if not hasattr(a, "data_ptr"):
            a = self.to_device(np.asarray(a, dtype=np.float64))
        if a.dtype != self.torch.float64:
            raise ValueError("alm_at_points: float64 expected")
        return a.contiguous()

    z, sth, phi = dev(z), dev(sth), dev(phi)
    npts = int(z.shape[0]) if z.dim() == 1 else -1
    if npts < 0 or not (tuple(sth.shape) == tuple(phi.shape) == (npts,)):
        raise ValueError("alm_at_points: z, sth and phi need one entry per point")
    mm, mmp = _iarr(ms)
    nm, lmax, nf, npol = int(mm.shape[0]), int(lmax), int(nf), int(npol)
    sf, sp, sl, sm = [int(v) for v in strides]
    if not (alm.is_cuda and alm.is_complex() and alm.element_size() == 16 and alm.is_contiguous()):
        raise ValueError("alm_at_points: the coefficients must be a contiguous complex128 device tensor")
    if lmax < 0 or min(sf, sp, sl, sm) < 0:
        raise ValueError("alm_at_points: lmax >= 0 and non-negative strides expected")
    if nm and nf > 0 and npol > 0:
        last = (nf - 1) * sf + (npol - 1) * sp + lmax * sl + (nm - 1) * sm
        if last >= alm.numel():
            raise ValueError("alm_at_points: the call would read outside its coefficients")
    shape = (max(npts, 0), max(npol, 0), max(nf, 0))
    if out is None:
        if accumulate:
            raise ValueError("alm_at_points: accumulate needs the output to add to")
        out = self.empty(shape, np.float64)
    if tuple(out.shape) != shape or not out.is_contiguous() or out.dtype != self.torch.float64:
        raise ValueError("alm_at_points: out must be a contiguous %s float64 tensor" % (shape,))
    rc = self.lib.dm_alm_at_points(self.h, npts, self.ptr(z), self.ptr(sth), self.ptr(phi), nm, mmp, lmax, nf, npol, self.ptr(alm),
                                   sf, sp, sl, sm, self.ptr(out), int(bool(accumulate)), int(max_bytes))
    self.check(rc, "dm_alm_at_points")
    return out


def _psmc_moments(self, q):
    """(mean (nblk, nq), covariance (nblk, nq, nq)) on the device of q (nblk, nq, ns) f64; see dm_psmc_moments."""
    nblk, nq, ns = [int(x_) for x_ in q.shape]
    q = q.contiguous()
    mean = self.empty((nblk, nq), np.float64)
    cov = self.empty((nblk, nq, nq), np.float64)
    self.check(self.lib.dm_psmc_moments(self.h, nblk, nq, ns, self.ptr(q), self.ptr(mean), self.ptr(cov)),
               "dm_psmc_moments")
    return mean, cov


def _psmc_alt(self, beam_svd, svnum, l0, cl_bands, evecs, evecs_off, nmodes, evals, evals_off, R, x, x_off, nsamples,
              want_vecs=False):
    """Stochastic-trace Fisher matrices (nblk, nbands, nbands) c128 on the device of R weighted draws per block (and
    the band vectors (nbands, sum_b nmodes_b R) c128 with `want_vecs`); see dm_psmc_alt in include/driftmi.h."""
    args, nblk, nbands, nm = _band_args(self, beam_svd, svnum, l0, cl_bands, evecs, evecs_off, nmodes, evals, evals_off)
    xo, xop = _larr(x_off)
    out = self.empty((nblk, nbands, nbands), np.complex128)
    vecs = self.empty((nbands, max(int(nm.astype(np.int64).sum()) * int(R), 1)), np.complex128) if want_vecs else None
    rc = self.lib.dm_psmc_alt(self.h, *args, int(R), self.ptr(x), xop, int(nsamples), self.ptr(vecs), self.ptr(out))
    self.check(rc, "dm_psmc_alt")
    return (out, vecs) if want_vecs else out


Context.psmc_draw = _psmc_draw
Context.psmc_moments = _psmc_moments
Context.psmc_alt = _psmc_alt
Context.sky_draw = _sky_draw
Context.source_alm = _source_alm
Context.alm_at_points = _alm_at_points


def _project_diag(self, beam_ut, svnum, dmat, out, out_off, alpha=1.0, accumulate=False):
    nblk, F, K, T = [int(x) for x in beam_ut.shape]
    sv, svp = _iarr(svnum)
    off, offp = _larr(out_off)
    rc = self.lib.dm_project_diag(self.h, nblk, F, K, T, self.ptr(beam_ut), svp, self.ptr(dmat), float(alpha),
                                  self.ptr(out), offp, int(accumulate))
    self.check(rc, "dm_project_diag")


def _regularise(self, mats, ndofs, off, reg):
    n, np_ = _iarr(ndofs)
    o, op = _larr(off)
    self.check(self.lib.dm_regularise(self.h, len(n), np_, self.ptr(mats), op, float(reg)), "dm_regularise")


def _eigh_gen(self, A, B, ndofs, off, cut=None):
    """A, B: flat device c128 buffers holding the (n_b x n_b) blocks at `off`.  Destroys both.
    cut: None, ("upper", thr) — only the modes with eigenvalue >= thr (rows i >= searchsorted(evals, thr))
    are formed — or ("lower", thr) for the rows below; the other rows of a block are zero.
    Returns (evals flat device f64 [offsets evoff], evoff, evecs flat device c128 [same off], add_const, sweeps);
    the number of rows formed per block is left in ``self.last_nkeep``."""
    n, np_ = _iarr(ndofs)
    o, op = _larr(off)
    evoff = np.concatenate([[0], np.cumsum(n.astype(np.int64))])
    eo, eop = _larr(evoff[:-1])
    evals = self.empty((max(int(evoff[-1]), 1),), np.float64)
    evecs = self.empty((max(int(A.numel()), 1),), np.complex128)
    ac = (c_dbl * max(len(n), 1))()
    nk = (c_int * max(len(n), 1))()
    sw = c_int(0)
    mode, thr = 0, 0.0
    if cut is not None:
        mode = {"upper": 1, "lower": 2}[cut[0]]
        thr = float(cut[1])
    rc = self.lib.dm_eigh_gen(self.h, len(n), np_, self.ptr(A), self.ptr(B), op, self.ptr(evals), eop,
                              self.ptr(evecs), ac, ctypes.byref(sw), mode, thr, nk)
    self.check(rc, "dm_eigh_gen")
    self.last_nkeep = np.array(nk[: len(n)], dtype=np.int64)
    return evals, evoff, evecs, np.array(ac[: len(n)], dtype=np.float64), sw.value


def _kl_m(self, beam_svd, beam_ut, svnum, l0, cl_sg, sg_mask, sg_sym, cl_fg, fg_mask, fg_sym, npower, noise_scale, regulariser,
          cut=None):
    """dm_kl_m: covariances + generalised eigenproblem of a batch of m-blocks in one library call.  Returns
    (evals flat, evoff, evecs flat, off, add_const, nkeep)."""
    nblk, F, K, P, L = [int(x) for x in beam_svd.shape]
    T = int(beam_ut.shape[-1])
    sv, svp = _iarr(svnum)
    ndofs = np.asarray(svnum).reshape(nblk, F).sum(axis=1).astype(np.int64)
    off, tot = _block_offsets(ndofs)
    evoff = np.concatenate([[0], np.cumsum(ndofs)])
    o, op = _larr(off)
    eo, eop = _larr(evoff[:-1])
    l0a, l0p = (None, None) if l0 is None else _iarr(l0)
    sm, smp = (None, None) if sg_mask is None else _iarr(sg_mask)
    fm, fmp = (None, None) if fg_mask is None else _iarr(fg_mask)
    evals = self.empty((max(int(evoff[-1]), 1),), np.float64)
    evecs = self.empty((max(tot, 1),), np.complex128)
    ac = (c_dbl * max(nblk, 1))()
    nk = (c_int * max(nblk, 1))()
    mode, thr = (0, 0.0) if cut is None else ({"upper": 1, "lower": 2}[cut[0]], float(cut[1]))
    rc = self.lib.dm_kl_m(self.h, nblk, F, K, P, L, T, self.ptr(beam_svd), self.ptr(beam_ut), svp, l0p, self.ptr(cl_sg), smp,
                          int(bool(sg_sym)), self.ptr(cl_fg), fmp, int(bool(fg_sym)), self.ptr(npower), float(noise_scale),
                          float(regulariser), mode, thr, self.ptr(evals), eop, self.ptr(evecs), op, ac, nk)
    self.check(rc, "dm_kl_m")
    return evals, evoff, evecs, off, np.array(ac[:nblk]), np.array(nk[:nblk], dtype=np.int64)


def _doublekl_m(self, beam_svd, beam_ut, svnum, l0, cl_sg, sg_mask, sg_sym, cl_fg, fg_mask, fg_sym, npower, floor_scale,
                regulariser, foreground_threshold, cut=None):
    """dm_doublekl_m.  Returns (f_evals flat, evals flat, evoff, modes flat, off, nmodes, nkeep, add_const)."""
    nblk, F, K, P, L = [int(x) for x in beam_svd.shape]
    T = int(beam_ut.shape[-1])
    sv, svp = _iarr(svnum)
    ndofs = np.asarray(svnum).reshape(nblk, F).sum(axis=1).astype(np.int64)
    off, tot = _block_offsets(ndofs)
    evoff = np.concatenate([[0], np.cumsum(ndofs)])
    o, op = _larr(off)
    eo, eop = _larr(evoff[:-1])
    l0a, l0p = (None, None) if l0 is None else _iarr(l0)
    sm, smp = (None, None) if sg_mask is None else _iarr(sg_mask)
    fm, fmp = (None, None) if fg_mask is None else _iarr(fg_mask)
    f_evals = self.empty((max(int(evoff[-1]), 1),), np.float64)
    evals = self.zeros((max(int(evoff[-1]), 1),), np.float64)
    modes = self.zeros((max(tot, 1),), np.complex128)
    ac = (c_dbl * max(nblk, 1))()
    nm = (c_int * max(nblk, 1))()
    nk = (c_int * max(nblk, 1))()
    mode, thr = (0, 0.0) if cut is None else ({"upper": 1, "lower": 2}[cut[0]], float(cut[1]))
    rc = self.lib.dm_doublekl_m(self.h, nblk, F, K, P, L, T, self.ptr(beam_svd), self.ptr(beam_ut), svp, l0p, self.ptr(cl_sg), smp,
                                int(bool(sg_sym)), self.ptr(cl_fg), fmp, int(bool(fg_sym)), self.ptr(npower), float(floor_scale),
                                float(regulariser), float(foreground_threshold), mode, thr, self.ptr(f_evals), self.ptr(evals),
                                eop, self.ptr(modes), op, nm, nk, ac)
    self.check(rc, "dm_doublekl_m")
    return (f_evals, evals, evoff, modes, off, np.array(nm[:nblk], dtype=np.int64), np.array(nk[:nblk], dtype=np.int64),
            np.array(ac[:nblk]))


Context.kl_m = _kl_m
Context.doublekl_m = _doublekl_m
Context.svd_chain = _svd_chain
Context.project_cov = _project_cov
Context.project_diag = _project_diag
Context.regularise = _regularise
Context.eigh_gen = _eigh_gen
block_offsets = _block_offsets


def _darr(a):
    a = np.ascontiguousarray(a, dtype=np.float64)
    return a, a.ctypes.data_as(ctypes.POINTER(c_dbl))


def _bt_beam_cyl(self, nside, cth, sth, frame, kind, tab, fwhm_ns, out):
    c, cp = _darr(cth)
    s_, sp = _darr(sth)
    fr, frp = _darr(frame)
    tx, txp = _darr(tab[0])
    ty, typ = _darr(tab[1])
    t2, t2p = _darr(tab[2])
    rc = self.lib.dm_bt_beam_cyl(self.h, int(nside), cp, sp, frp, int(kind), txp, typ, t2p, len(tx), float(fwhm_ns),
                                 self.ptr(out))
    self.check(rc, "dm_bt_beam_cyl")


def _bt_beams_cyl(self, nside, cth, sth, frame, specs, out, rows):
    """Evaluate the cylinder patterns `specs` = [(kind, (x, y, y2), fwhm_ns), ...] into the rows `rows` of the 2-D
    float64 device tensor `out` — consecutive rows go up in one dm_bt_beams_cyl call each."""
    if not specs:
        return
    c, cp = _darr(cth)
    s_, sp = _darr(sth)
    fr, frp = _darr(frame)
    stride = int(out.stride(0))
    i = 0
    while i < len(specs):
        j = i + 1
        while j < len(specs) and rows[j] == rows[j - 1] + 1:
            j += 1
        kinds, kp = _iarr([sp_[0] for sp_ in specs[i:j]])
        fw, fwp = _darr([sp_[2] for sp_ in specs[i:j]])
        offs = np.concatenate([[0], np.cumsum([len(sp_[1][0]) for sp_ in specs[i:j]])])
        of, ofp = _iarr(offs)
        tx, txp = _darr(np.concatenate([sp_[1][0] for sp_ in specs[i:j]]))
        ty, typ = _darr(np.concatenate([sp_[1][1] for sp_ in specs[i:j]]))
        t2, t2p = _darr(np.concatenate([sp_[1][2] for sp_ in specs[i:j]]))
        rc = self.lib.dm_bt_beams_cyl(self.h, int(nside), cp, sp, frp, j - i, kp, txp, typ, t2p, ofp, fwp,
                                      self.ptr(out[rows[i]]), stride)
        self.check(rc, "dm_bt_beams_cyl")
        i = j


def _bt_maps(self, nside, cth, sth, frame, polarised, beams, uv, bi, bj, maps):
    c, cp = _darr(cth)
    s_, sp = _darr(sth)
    fr, frp = _darr(frame)
    u, up = _darr(uv)
    i_, ip = _iarr(bi)
    j_, jp = _iarr(bj)
    # complex128 beams take the complex-pattern kernels (second beam conjugated, |b|^2 solid angles)
    fn = self.lib.dm_bt_maps_c if beams.is_complex() else self.lib.dm_bt_maps
    rc = fn(self.h, int(nside), cp, sp, frp, int(bool(polarised)), int(beams.shape[0]),
            self.ptr(beams), len(i_), up, ip, jp, self.ptr(maps))
    self.check(rc, "dm_bt_maps")


def _bt_sht(self, nside, cth, sth, polarised, lside, mmax, lmax_grp, F, B, col_f, col_b, col_lmax, maps, beam_m,
            m_range=None, niter=0, ring_w=None):
    """m_range = (m_lo, m_hi): only those m-blocks are produced and `beam_m` has m_hi - m_lo + 1 of them.
    niter / ring_w: healpy.map2alm's `iter` and ring weights (see dm_bt_sht_opts)."""
    c, cp = _darr(cth)
    s_, sp = _darr(sth)
    f_, fp = _iarr(col_f)
    b_, bp = _iarr(col_b)
    l_, lp = _iarr(col_lmax)
    if niter or ring_w is not None:
        m_lo, m_hi = (0, int(mmax)) if m_range is None else (int(m_range[0]), int(m_range[1]))
        w, wp = (None, None) if ring_w is None else _darr(ring_w)
        if w is not None and w.size != 4 * int(nside) - 1:
            raise ValueError("ring weights: need one per ring (4 nside - 1 = %d), got %d" % (4 * int(nside) - 1, w.size))
        rc = self.lib.dm_bt_sht_opts(self.h, int(nside), cp, sp, int(bool(polarised)), int(lside), m_lo, m_hi,
                                     int(lmax_grp), int(F), int(B), len(f_), fp, bp, lp, self.ptr(maps), self.ptr(beam_m),
                                     int(niter), wp)
        self.check(rc, "dm_bt_sht_opts")
        return
    if m_range is None:
        rc = self.lib.dm_bt_sht(self.h, int(nside), cp, sp, int(bool(polarised)), int(lside), int(mmax), int(lmax_grp),
                                int(F), int(B), len(f_), fp, bp, lp, self.ptr(maps), self.ptr(beam_m))
    else:
        rc = self.lib.dm_bt_sht_range(self.h, int(nside), cp, sp, int(bool(polarised)), int(lside), int(m_range[0]),
                                      int(m_range[1]), int(lmax_grp), int(F), int(B), len(f_), fp, bp, lp,
                                      self.ptr(maps), self.ptr(beam_m))
    self.check(rc, "dm_bt_sht")


def _bt_columns(self, nside, cth, sth, frame, polarised, beams, uv, bi, bj, lside, mmax, lmax_grp, F, B, col_f, col_b,
                col_lmax, beam_m, m_range=None, ring_w=None, niter=0):
    """Beams -> beam_m rows of the given columns without materialising the Stokes maps (dm_bt_columns); with
    niter > 0 healpy's `iter` refinements in harmonic space (dm_bt_columns_iter)."""
    c, cp = _darr(cth)
    s_, sp = _darr(sth)
    fr, frp = _darr(frame)
    u, up = _darr(uv)
    i_, ip = _iarr(bi)
    j_, jp = _iarr(bj)
    f_, fp = _iarr(col_f)
    b_, bp = _iarr(col_b)
    l_, lp = _iarr(col_lmax)
    m_lo, m_hi = (0, int(mmax)) if m_range is None else (int(m_range[0]), int(m_range[1]))
    w, wp = (None, None) if ring_w is None else _darr(ring_w)
    # complex field patterns (a complex128 beams tensor) take the entry that forms _construct_pol_complex in the kernels
    if niter:
        rc = self.lib.dm_bt_columns_iter(self.h, int(nside), cp, sp, frp, int(bool(polarised)), int(beams.shape[0]),
                                         self.ptr(beams), int(beams.is_complex()), len(i_), up, ip, jp, int(lside), m_lo, m_hi,
                                         int(lmax_grp), int(F), int(B), fp, bp, lp, self.ptr(beam_m), wp, int(niter))
        self.check(rc, "dm_bt_columns_iter")
        return
    fn = self.lib.dm_bt_columns_c if beams.is_complex() else self.lib.dm_bt_columns
    rc = fn(self.h, int(nside), cp, sp, frp, int(bool(polarised)), int(beams.shape[0]), self.ptr(beams),
            len(i_), up, ip, jp, int(lside), m_lo, m_hi, int(lmax_grp), int(F), int(B), fp, bp, lp,
            self.ptr(beam_m), wp)
    self.check(rc, "dm_bt_columns")


def _sht_synth(self, nside, cth, sth, polarised, lmax, M, ncol, alm, maps):
    """(ncol, P, lmax + 1, M) c128 coefficients -> (ncol, P, 12 nside^2) f64 maps on the device (dm_sht_synth);
    P = 4 if polarised else 1.  Queued on the context's stream."""
    P = 4 if polarised else 1
    if tuple(alm.shape) != (int(ncol), P, int(lmax) + 1, int(M)) or tuple(maps.shape) != (int(ncol), P, 12 * int(nside) ** 2):
        raise ValueError("sht_synth: alm %s / maps %s do not match ncol %d, P %d, lmax %d, M %d, nside %d"
                         % (tuple(alm.shape), tuple(maps.shape), ncol, P, lmax, M, nside))
    if not (alm.is_contiguous() and maps.is_contiguous() and alm.is_complex() and not maps.is_complex()):
        raise ValueError("sht_synth: need contiguous complex128 alm and float64 maps")
    c, cp = _darr(cth)
    s_, sp = _darr(sth)
    rc = self.lib.dm_sht_synth(self.h, int(nside), cp, sp, int(bool(polarised)), int(lmax), int(M), int(ncol),
                               self.ptr(alm), self.ptr(maps))
    self.check(rc, "dm_sht_synth")


def bt_alias_info(nside, cth, sth, polarised, lmax_grp):
    """(alias rings per cap, mcut) of the harmonic-space refinement for one nside group (dm_bt_alias_info; host only)."""
    c, cp = _darr(cth)
    s_, sp = _darr(sth)
    nr, mc = c_int(0), c_int(0)
    rc = load().dm_bt_alias_info(int(nside), cp, sp, int(bool(polarised)), int(lmax_grp), ctypes.byref(nr), ctypes.byref(mc))
    if rc != 0:
        raise DriftMIError("dm_bt_alias_info failed (%d)" % rc)
    return nr.value, mc.value


def bt_ring_plan_info(nside, polarised, m_lo, m_hi, lmax_grp, complex_beams, ncol):
    """What the fused ring transform of `Context.bt_columns` launches for a call (dm_bt_ring_plan_info; host only): a dict
    with use_fft, fft_npt, fft_cpw (0 without FFT), nring_dft (rings left to the matrix form) and dft_row =
    (dft2, P, NMG, NCG) or None where no ring is left to it."""
    uf, npt, cpw, nrd = c_int(0), c_int(0), c_int(0), c_int(0)
    row = (c_int * 4)()
    rc = load().dm_bt_ring_plan_info(int(nside), int(bool(polarised)), int(m_lo), int(m_hi), int(lmax_grp),
                                     int(bool(complex_beams)), int(ncol), ctypes.byref(uf), ctypes.byref(npt),
                                     ctypes.byref(cpw), ctypes.byref(nrd), row)
    if rc != 0:
        raise DriftMIError("dm_bt_ring_plan_info failed (%d)" % rc)
    return dict(use_fft=bool(uf.value), fft_npt=npt.value, fft_cpw=cpw.value, nring_dft=nrd.value,
                dft_row=(bool(row[0]), row[1], row[2], row[3]) if nrd.value > 0 else None)


Context.bt_columns = _bt_columns
Context.bt_beam_cyl = _bt_beam_cyl
Context.bt_beams_cyl = _bt_beams_cyl
Context.bt_maps = _bt_maps
Context.bt_sht = _bt_sht
Context.sht_synth = _sht_synth


PROF_CLASSES = ["zgemm_grouped", "gemm_grouped_realB", "jac_gram", "jac_inner", "jac_apply", "dgemm_grouped",
                "trd_symv", "trd_wx",  # these two report algorithmic BYTES in the "flops" field (HBM-bound kernels)
                "sb_panel_qr", "sb_chase", "sb_q2_apply",   # two-stage tridiagonalisation (fp64 VALU)
                "zgemm_cov",                                  # gathered-B ZGEMM: the covariance projections
                # extended classes (profiling level 2, time only)
                "bt_ring", "bt_other", "trd_small", "dc", "chol_solve", "util", "eig_other", "svd_other",
                "blockvec",   # reports algorithmic BYTES of A in the "flops" field
                "unused21", "unused22", "unused23"]
PROF_NCLASS = len(PROF_CLASSES)


def _prof_reset(self, enable=True):
    """enable: False / True (the MFMA and HBM-bound classes) / 2 (every kernel of the path: the extended classes too)."""
    self.check(self.lib.dm_prof_reset(self.h, int(enable)), "dm_prof_reset")
    self._prof_level = int(enable)


def _prof_enabled(self):
    return bool(getattr(self, "_prof_level", 0))


def _prof_report(self):
    ms = (c_dbl * PROF_NCLASS)()
    fl = (c_dbl * PROF_NCLASS)()
    ln = (ctypes.c_longlong * PROF_NCLASS)()
    self.check(self.lib.dm_prof_report(self.h, ms, fl, ln), "dm_prof_report")
    return {name: dict(ms=ms[i], flops=fl[i], launches=int(ln[i])) for i, name in enumerate(PROF_CLASSES) if ln[i] > 0}


Context.prof_reset = _prof_reset
Context.prof_enabled = _prof_enabled
Context.prof_report = _prof_report


def _herm_eig(self, C, n, ldc, strideC=0, batch=1):
    W = self.empty((batch, n, n), np.complex128)
    ev = self.empty((batch, max(n, 1)), np.float64)
    rc = self.lib.dm_herm_eig_batched(self.h, n, self.ptr(C), ldc, strideC, self.ptr(W), n, n * n, batch, self.ptr(ev))
    self.check(rc, "dm_herm_eig_batched")
    return ev, W


Context.herm_eig = _herm_eig
