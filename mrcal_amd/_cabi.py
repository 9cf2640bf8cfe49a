"""ctypes binding of the C ABI: the structures, and the ONE table of every entry point's signature.

The SAME binding drives two shared libraries, because libmrcal_amd.so exports
the reference's own C entry points for this path (include/mrcal_amd.h, "drop-in
tier") with the reference's signatures (mrcal.h:374-853, internal.h:99-114):

  - mrcal_amd/libmrcal_amd.so      the product: HIP kernels behind the C ABI
  - any libmrcal.so-compatible lib e.g. the reference's own sources compiled as
                                   a CPU checker. Only tests/bench do that;
                                   nothing in this package loads anything but
                                   libmrcal_amd.so on its own.

SIGNATURES has a row for every function include/mrcal_amd.h declares (tests/test_cabi_symbols.py holds the two
together); MrcalLib applies them when it loads a library. Nothing else in the package sets a restype or argtypes.

This module is plumbing: no numerics happen here.
"""
import ctypes as C
import os
import numpy as np

c_double_p = C.POINTER(C.c_double)
c_int_p    = C.POINTER(C.c_int)


class Lensmodel(C.Structure):
    """mrcal_lensmodel_t: 16 bytes. types.h:131-145"""
    class _U(C.Union):
        class _Cahvore(C.Structure):
            _fields_ = [("linearity", C.c_double)]
        class _Splined(C.Structure):
            _fields_ = [("order", C.c_uint16), ("Nx", C.c_uint16),
                        ("Ny", C.c_uint16),    ("fov_x_deg", C.c_uint16)]
        _fields_ = [("cahvore", _Cahvore), ("splined", _Splined)]
    _anonymous_ = ("u",)
    _fields_ = [("type", C.c_int), ("u", _U)]
assert C.sizeof(Lensmodel) == 16


class ProblemSelections(C.Structure):
    """mrcal_problem_selections_t: 8 one-bit flags in one byte, passed by
    value. Bit order of types.h:283-301"""
    _fields_ = [("bits", C.c_uint8)]
    NAMES = ("do_optimize_intrinsics_core",
             "do_optimize_intrinsics_distortions",
             "do_optimize_extrinsics",
             "do_optimize_frames",
             "do_optimize_calobject_warp",
             "do_apply_regularization",
             "do_apply_outlier_rejection",
             "do_apply_regularization_unity_cam01")

    @classmethod
    def make(cls, **flags):
        bits = 0
        for i, name in enumerate(cls.NAMES):
            if flags.get(name, False):
                bits |= (1 << i)
        unknown = set(flags) - set(cls.NAMES)
        if unknown:
            raise TypeError(f"unknown problem selections: {unknown}")
        return cls(bits)

    def as_dict(self):
        return {name: bool(self.bits & (1 << i)) for i, name in enumerate(self.NAMES)}
assert C.sizeof(ProblemSelections) == 1


class Stats(C.Structure):
    """mrcal_stats_t. types.h:321-344"""
    _fields_ = [("rms_reproj_error__pixels",     C.c_double),
                ("Noutliers_board",              C.c_int),
                ("Noutliers_triangulated_point", C.c_int)]


class CholmodSparse(C.Structure):
    """The head of SuiteSparse's cholmod_sparse; only p,i,x are written by the
    callback (mrcal.c:4461-4463)"""
    _fields_ = [("nrow", C.c_size_t), ("ncol", C.c_size_t), ("nzmax", C.c_size_t),
                ("p", C.c_void_p), ("i", C.c_void_p), ("nz", C.c_void_p),
                ("x", C.c_void_p), ("z", C.c_void_p),
                ("stype", C.c_int), ("itype", C.c_int), ("xtype", C.c_int),
                ("dtype", C.c_int), ("sorted", C.c_int), ("packed", C.c_int)]


# observation records. types.h:195-263
observation_board_dtype = np.dtype([("icam_intrinsics", np.int32),
                                    ("icam_extrinsics", np.int32),
                                    ("iframe",          np.int32)])
observation_point_dtype = np.dtype([("icam_intrinsics", np.int32),
                                    ("icam_extrinsics", np.int32),
                                    ("i_point",         np.int32)])
# {int,int,bitfield byte(+7 pad), double[3]}: 40 bytes
observation_point_triangulated_dtype = np.dtype({
    "names":   ["icam_intrinsics", "icam_extrinsics", "flags", "px"],
    "formats": [np.int32, np.int32, np.uint8, (np.float64, 3)],
    "offsets": [0, 4, 8, 16],
    "itemsize": 40})
TRIANGULATED_LAST_IN_SET = 1
TRIANGULATED_OUTLIER     = 2


def _ptr(a, ctype=C.c_void_p):
    if a is None:
        return None
    return a.ctypes.data_as(ctype)


# ---------------------------------------------------------------------------------------------------------------------
# name -> (restype, argtypes), in the order of include/mrcal_amd.h. A pointer is c_void_p wherever the callers pass
# _ptr(array), C.addressof() or an address; a typed pointer where they pass C.byref() or a ctypes array of that type
vp, i, d, b, cp, sz = C.c_void_p, C.c_int, C.c_double, C.c_bool, C.c_char_p, C.c_size_t
u16, i64 = C.c_uint16, C.c_int64
ip, dp, i64p = c_int_p, c_double_p, C.POINTER(C.c_int64)
lm, sp, Sel = C.POINTER(Lensmodel), C.POINTER(CholmodSparse), ProblemSelections

SIGNATURES = {
    "mrcal_lensmodel_from_name": (b, [lm, cp]),
    "mrcal_lensmodel_name": (b, [vp, i, vp]),
    "mrcal_lensmodel_num_params": (i, [lm]),
    "mrcal_num_intrinsics_optimization_params": (i, [Sel, lm]),
    "mrcal_pack_solver_state_vector": (None, [dp] + [i]*6 + [Sel, lm]),
    "mrcal_unpack_solver_state_vector": (None, [dp] + [i]*6 + [Sel, lm]),
    "mrcal_corresponding_icam_extrinsics": (b, [ip] + [i]*4 + [vp, i, vp]),
    "mrcal_optimize": (Stats, [vp, i, vp, i] + [vp]*5 + [i]*5 + [vp, vp, i, i, vp, i, vp, vp, lm, vp, Sel, vp, d, i, i, b, b]),
    "mrcal_unproject": (b, [vp, vp, i, vp, vp]),
    "mrcal_amd_unproject": (b, [vp]*4 + [i, vp, vp, b]),
    "mrcal_project": (b, [vp]*4 + [i, vp, vp]),
    "mrcal_optimizer_callback": (b, [vp, i, vp, i, sp] + [vp]*5 + [i]*5 + [vp, vp, i, i, vp, i, vp, vp, lm, vp, Sel, vp, d, i, i, b]),
    "_mrcal_drt_cross_reprojection__dbpacked": (b, [vp, i, i]*4 + [i, vp, i, sp] + [i]*7 + [lm, Sel, i, i]),
    "mrcal_measurement_index_boards": (i, [i]*5),
    "mrcal_num_measurements_boards": (i, [i]*3),
    "mrcal_measurement_index_points": (i, [i]*5),
    "mrcal_num_measurements_points": (i, [i]),
    "mrcal_measurement_index_points_triangulated": (i, [i]*3 + [vp] + [i]*3),
    "mrcal_num_measurements_points_triangulated": (i, [vp, i]),
    "mrcal_num_measurements_points_triangulated_initial_Npoints": (i, [vp, i, i]),
    "mrcal_decode_observation_indices_points_triangulated": (b, [ip]*6 + [i, vp, i]),
    "mrcal_measurement_index_regularization": (i, [vp] + [i]*10 + [Sel, lm]),
    "mrcal_num_measurements_regularization": (i, [i]*6 + [Sel, lm]),
    "mrcal_num_measurements": (i, [i, i, vp] + [i]*8 + [Sel, lm]),
    "mrcal_num_states": (i, [i]*6 + [Sel, lm]),
    "mrcal_state_index_intrinsics": (i, [i]*7 + [Sel, lm]),
    "mrcal_num_states_intrinsics": (i, [i, Sel, lm]),
    "mrcal_state_index_extrinsics": (i, [i]*7 + [Sel, lm]),
    "mrcal_num_states_extrinsics": (i, [i, Sel]),
    "mrcal_state_index_frames": (i, [i]*7 + [Sel, lm]),
    "mrcal_num_states_frames": (i, [i, Sel]),
    "mrcal_state_index_points": (i, [i]*7 + [Sel, lm]),
    "mrcal_num_states_points": (i, [i, i, Sel]),
    "mrcal_state_index_calobject_warp": (i, [i]*6 + [Sel, lm]),
    "mrcal_num_states_calobject_warp": (i, [Sel, i]),
    "_mrcal_num_j_nonzero": (i, [i, i, vp] + [i]*8 + [vp, vp, Sel, lm]),
    "mrcal_read_cameramodel_string": (vp, [vp, i]),
    "mrcal_read_cameramodel_file": (vp, [vp]),
    "mrcal_free_cameramodel": (None, [vp]),
    "mrcal_read_cameramodel_string_into": (b, [vp]*3 + [i]),
    "mrcal_read_cameramodel_file_into": (b, [vp]*3),
    "mrcal_write_cameramodel_file": (b, [vp, vp]),
    "mrcal_amd_last_error": (cp, []),
    "mrcal_amd_device_count": (i, []),
    "mrcal_amd_device_buffers_live": (C.c_long, []),
    "mrcal_amd_problem_create": (vp, [vp]*5 + [i]*5 + [vp, vp, i, i, vp, i] + [vp]*4 + [Sel, d] + [i]*4 + [b]),
    "mrcal_amd_problem_create_sharded": (vp, [vp]*5 + [i]*5 + [vp, vp, i, i, vp, i, vp, vp, lm, vp, Sel, d] + [i]*8 + [b]),
    "mrcal_amd_problem_destroy": (None, [vp]),
    "mrcal_amd_problem_Nstate": (i, [vp]),
    "mrcal_amd_problem_Nmeasurements": (i, [vp]),
    "mrcal_amd_problem_Nnz": (i64, [vp]),
    "mrcal_amd_problem_jacobian_algorithmic_bytes": (i64, [vp]),
    "mrcal_amd_problem_synchronize": (b, [vp]),
    "mrcal_amd_problem_dev_b_packed": (vp, [vp]),
    "mrcal_amd_problem_dev_x": (vp, [vp]),
    "mrcal_amd_problem_dev_J_rowptr": (vp, [vp]),
    "mrcal_amd_problem_dev_J_colidx": (vp, [vp]),
    "mrcal_amd_problem_dev_J_values": (vp, [vp]),
    "mrcal_amd_problem_set_b_packed": (b, [vp, vp]),
    "mrcal_amd_problem_get_b_packed": (b, [vp, vp]),
    "mrcal_amd_problem_get_x": (b, [vp, vp]),
    "mrcal_amd_problem_get_J": (b, [vp]*4),
    "mrcal_amd_problem_evaluate": (b, [vp, b, b]),
    "mrcal_amd_problem_stream": (vp, [vp]),
    "mrcal_amd_problem_last_jacobian_kernel_ms": (d, [vp]),
    "mrcal_amd_problem_jacobian_timing_begin": (b, [vp, i]),
    "mrcal_amd_problem_jacobian_timing_begin_strided": (b, [vp, i, i]),
    "mrcal_amd_problem_jacobian_timing_end": (b, [vp, ip] + [dp]*3),
    "mrcal_amd_problem_dissection": (b, [vp, ip]),
    "mrcal_amd_comm_unique_id": (b, [vp]),
    "mrcal_amd_comm_create": (vp, [vp, i, i]),
    "mrcal_amd_comm_create_host": (vp, [cp, i, i]),
    "mrcal_amd_comm_destroy": (None, [vp]),
    "mrcal_amd_comm_rank": (i, [vp]),
    "mrcal_amd_comm_world": (i, [vp]),
    "mrcal_amd_comm_Ncollectives": (C.c_long, [vp]),
    "mrcal_amd_comm_Ndoubles": (C.c_longlong, [vp]),
    "mrcal_amd_comm_world_observed": (i, [vp]),
    "mrcal_amd_comm_allreduce_sum": (b, [vp, vp, i64, vp]),
    "mrcal_amd_problem_attach_comm": (b, [vp, vp]),
    "mrcal_amd_problem_gather_state": (b, [vp]),
    "mrcal_amd_problem_sharded_reset": (b, [vp, i, i, d]),
    "mrcal_amd_problem_sharded_enqueue": (b, [vp, i, i]),
    "mrcal_amd_problem_sharded_comm_buffer": (vp, [vp, i, i64p]),
    "mrcal_amd_problem_sharded_snapshot": (b, [vp, i]),
    "mrcal_amd_problem_sharded_wait": (b, [vp, i, ip]),
    "mrcal_amd_problem_sharded_finish": (b, [vp, ip, dp]),
    "mrcal_amd_problem_shard_info": (i, [vp, ip, i]),
    "mrcal_amd_set_elimination": (i, [i]),
    "mrcal_amd_set_test_hook": (i, [cp, i]),
    "mrcal_amd_problem_lchol_diag_ratio": (d, [vp]),
    "mrcal_amd_problem_uses_sweep": (i, [vp]),
    "mrcal_amd_problem_set_jacobian_stream": (i, [vp, i]),
    "mrcal_amd_problem_jacobian_stream_is_optional": (i, [vp]),
    "mrcal_amd_set_optimize_jacobian_stream": (i, [i]),
    "mrcal_amd_problem_partition": (None, [vp, ip]),
    "mrcal_amd_problem_get_triangulated_outliers": (i, [vp, vp, i, vp]),
    "mrcal_amd_problem_phase_outlier_stats": (b, [vp, i, d, vp, vp]),
    "mrcal_amd_problem_phase_mark_outliers": (b, [vp, i, d, vp]),
    "mrcal_amd_problem_set_current": (None, [vp, i]),
    "mrcal_amd_problem_current": (i, [vp]),
    "mrcal_amd_problem_solve": (d, [vp, i, ip]),
    "mrcal_amd_problem_run_steps": (i, [vp, i, dp]),
    "mrcal_amd_problem_solver_stats": (None, [vp] + [ip]*4 + [dp]*3),
    "mrcal_amd_problem_drt_cross_reprojection": (b, [vp, i, vp]),
    "mrcal_amd_problem_get_normal_equations": (b, [vp]*7),
    "mrcal_amd_problem_gauss_newton_step": (b, [vp, vp]),
    "mrcal_amd_problem_get_board_pool": (b, [vp, vp]),
    "mrcal_amd_factorization_create": (vp, [i, i] + [vp]*3 + [i]*4),
    "mrcal_amd_factorization_create_from_problem": (vp, [vp]),
    "mrcal_amd_factorization_last_status": (i, []),
    "mrcal_amd_factorization_Nmeasurements": (i, [vp]),
    "mrcal_amd_factorization_destroy": (None, [vp]),
    "mrcal_amd_factorization_Nstate": (i, [vp]),
    "mrcal_amd_factorization_solve": (b, [vp, vp, i, vp]),
    "mrcal_amd_factorization_solve_sys": (b, [vp, i, vp, i, vp]),
    "mrcal_amd_factorization_Jt_x": (b, [vp]*3),
    "mrcal_amd_factorization_A_Jt_J_At": (b, [vp, vp, i, i, vp]),
    "mrcal_amd_csr_Jt_x": (b, [i, i] + [vp]*5),
    "mrcal_amd_csr_A_Jt_J_At": (b, [i, i] + [vp]*4 + [i, i, vp]),
    "mrcal_amd_factorization_rcond": (d, [vp]),
    "mrcal_amd_uncertainty_create": (vp, [vp, i, i, d]),
    "mrcal_amd_uncertainty_evaluate": (b, [vp, vp, i, b, i, vp]),
    "mrcal_amd_uncertainty_observed_pixel_uncertainty": (d, [vp]),
    "mrcal_amd_uncertainty_destroy": (None, [vp]),
    "mrcal_amd_implied_rt10": (b, [vp]*9 + [i, i, b, vp, d]),
    "mrcal_amd_projection_diff_create": (vp, [i] + [vp]*3 + [i]),
    "mrcal_amd_projection_diff_evaluate": (b, [vp, vp, i, b, vp, b, vp, d] + [vp]*8),
    "mrcal_amd_projection_diff_time_fit": (d, [vp, b]),
    "mrcal_amd_projection_diff_destroy": (None, [vp]),
    "mrcal_amd_lensfit_create": (vp, []),
    "mrcal_amd_lensfit_fit": (b, [vp]*4 + [i] + [vp]*4 + [i] + [b]*3 + [i] + [vp]*7),
    "mrcal_amd_lensfit_last_ms": (d, [vp]),
    "mrcal_amd_lensfit_plan": (b, [vp, vp, i, i, vp] + [b]*3),
    "mrcal_amd_lensfit_destroy": (None, [vp]),
    "mrcal_amd_triangulate_geometric": (b, [i] + [vp]*7),
    "mrcal_amd_triangulate_lindstrom": (b, [i] + [vp]*7),
    "mrcal_amd_triangulate_leecivera_l1": (b, [i] + [vp]*7),
    "mrcal_amd_triangulate_leecivera_linf": (b, [i] + [vp]*7),
    "mrcal_amd_triangulate_leecivera_mid2": (b, [i] + [vp]*7),
    "mrcal_amd_triangulate_leecivera_wmid2": (b, [i] + [vp]*7),
    "mrcal_amd_triangulation_create": (vp, [vp, i, vp]),
    "mrcal_amd_triangulation_evaluate": (b, [vp, i, vp, vp, i] + [d]*3 + [b] + [vp]*3),
    "mrcal_amd_triangulation_observed_pixel_uncertainty": (d, [vp]),
    "mrcal_amd_triangulation_destroy": (None, [vp]),
    "mrcal_rectified_resolution": (b, [vp]*7 + [i]),
    "mrcal_rectified_system2": (b, [vp]*8 + [d] + [vp]*4 + [i] + [b]*4),
    "mrcal_rectified_system": (b, [vp]*12 + [i] + [b]*4),
    "mrcal_rectification_maps": (b, [vp]*7 + [i] + [vp]*3),
    "mrcal_stereo_range_sparse": (b, [vp]*3 + [i, d, d, i, vp, d]),
    "mrcal_stereo_range_dense": (b, [vp, vp] + [u16]*3 + [i, vp, d]),
    "mrcal_amd_stereo_range_sparse": (b, [vp]*4 + [i, d, d, i, vp, d]),
    "mrcal_amd_image_transformation_map": (b, [vp]*8 + [d, vp, i]),
    "mrcal_amd_transform_image": (b, [vp, vp] + [i]*4 + [vp] + [i]*4 + [vp]),
    "mrcal_amd_rectification_create": (vp, [vp]*6 + [i] + [vp]*3 + [d]),
    "mrcal_amd_rectification_maps": (b, [vp, vp]),
    "mrcal_amd_rectification_rectify": (b, [vp]*4 + [i, i, vp] + [i]*6 + [vp]),
    "mrcal_amd_rectification_range": (b, [vp]*3 + [u16]*3),
    "mrcal_amd_rectification_destroy": (None, [vp]),
    "mrcal_amd_feature_matcher_create": (vp, [vp, i, i, vp] + [i]*3),
    "mrcal_amd_feature_matcher_match": (b, [vp, i, vp, vp] + [i]*4 + [vp]*6),
    "mrcal_amd_feature_matcher_matchoutput": (b, [vp, i, vp]),
    "mrcal_amd_feature_matcher_template": (b, [vp, i, vp]),
    "mrcal_amd_feature_matcher_destroy": (None, [vp]),
    "mrcal_amd_stereo_sgm_create": (vp, [i]*3 + [vp]),
    "mrcal_amd_stereo_sgm_match": (b, [vp]*4),
    "mrcal_amd_stereo_sgm_stage_milliseconds": (b, [vp, vp]),
    "mrcal_amd_stereo_sgm_destroy": (None, [vp]),
    "mrcal_amd_rectification_disparity": (b, [vp, vp, i, i, vp] + [i]*3 + [vp, vp]),
    "mrcal_amd_stereo_sgm_set_speckle_filter": (b, [vp, i, i]),
    "mrcal_amd_stereo_sgm_speckle_milliseconds": (b, [vp, vp]),
    "mrcal_amd_rectification_disparity_filtered": (b, [vp, vp, i, i, vp] + [i]*3 + [vp, i, i, vp]),
    "mrcal_amd_speckle_filter_create": (vp, [i, i]),
    "mrcal_amd_speckle_filter_apply": (b, [vp]*3 + [i]*3),
    "mrcal_amd_speckle_filter_milliseconds": (b, [vp, vp]),
    "mrcal_amd_speckle_filter_pass_milliseconds": (b, [vp, vp]),
    "mrcal_amd_speckle_filter_destroy": (None, [vp]),
    "mrcal_amd_point_cloud_create": (vp, [i, vp, d, i, i, vp]),
    "mrcal_amd_point_cloud_set_map": (b, [vp, vp]),
    "mrcal_amd_point_cloud_compute": (b, [vp]*4),
    "mrcal_amd_point_cloud_read": (b, [vp]*4),
    "mrcal_amd_point_cloud_stage_milliseconds": (b, [vp, vp]),
    "mrcal_amd_point_cloud_destroy": (None, [vp]),
    "mrcal_amd_rectification_point_cloud": (b, [vp]*4),
    "mrcal_amd_rectification_point_cloud_of_images": (b, [vp, vp, i, i, vp] + [i]*3 + [vp, i, i, vp, vp]),
    "mrcal_amd_rectification_point_cloud_read": (b, [vp]*4),
    "mrcal_amd_rectification_point_cloud_stage_milliseconds": (b, [vp, vp]),
    "mrcal_amd_chessboard_detector_create": (vp, [i]*3 + [vp, sz]),
    "mrcal_amd_chessboard_detector_candidates": (b, [vp]*7),
    "mrcal_amd_chessboard_detector_find_board": (b, [vp, vp, i, i, vp, vp]),
    "mrcal_amd_chessboard_detector_read_response": (b, [vp]*4),
    "mrcal_amd_chessboard_detector_stage_milliseconds": (b, [vp, vp]),
    "mrcal_amd_chessboard_detector_destroy": (None, [vp]),
    "mrcal_amd_chessboard_detector_create_pyramid": (vp, [i]*3 + [vp, i, sz]),
    "mrcal_amd_chessboard_detector_find_board_pyramid": (b, [vp, vp, i, i] + [vp]*4),
    "mrcal_amd_chessboard_detector_read_level": (b, [vp, i, vp]),
    "mrcal_amd_chessboard_detector_pyramid_milliseconds": (b, [vp]*4),
    "mrcal_amd_chessboard_grid": (b, [i] + [vp]*3 + [i, i, vp, vp]),
    "mrcal_amd_equalizer_create": (vp, [i]*3 + [vp]),
    "mrcal_amd_equalizer_apply": (b, [vp]*3),
    "mrcal_amd_equalizer_stage_milliseconds": (b, [vp, vp]),
    "mrcal_amd_equalizer_destroy": (None, [vp]),
    "mrcal_amd_rectification_set_equalization": (b, [vp, vp]),
    "mrcal_amd_feature_matcher_create_equalized": (vp, [vp, i, i, vp] + [i]*3 + [vp]),
    "mrcal_amd_smoother_create": (vp, [i]*3 + [vp]),
    "mrcal_amd_smoother_apply": (b, [vp]*3),
    "mrcal_amd_smoother_milliseconds": (b, [vp, vp]),
    "mrcal_amd_smoother_destroy": (None, [vp]),
    "mrcal_amd_smooth_weights": (b, [d, ip, vp]),
    "mrcal_amd_rectification_set_antialias": (b, [vp, vp]),
    "mrcal_amd_transform_image_smoothed": (b, [vp, vp] + [i]*4 + [vp] + [i]*4 + [vp, vp]),
    "mrcal_amd_regional_statistics_create": (vp, [vp, i, i]),
    "mrcal_amd_regional_statistics_grid": (b, [vp, i, ip, ip]),
    "mrcal_amd_regional_statistics_get": (b, [vp, i] + [vp]*3),
    "mrcal_amd_regional_statistics_binning_ms": (d, [vp]),
    "mrcal_amd_regional_statistics_destroy": (None, [vp]),
    "mrcal_amd_valid_region_mask": (b, [vp, vp, i, vp, vp] + [i]*4 + [d]*5 + [vp, vp]),
    "mrcal_amd_region_outline": (i, [vp, i, i, vp, i, i64p]),
    "mrcal_amd_valid_region_lds_vertices": (i, []),
    "mrcal_amd_valid_region_contains": (b, [vp, vp, i64, vp, i]),
    "mrcal_amd_valid_region_image": (b, [vp, i, i, vp, i]),
}

# exported for the tests of the host-side planning code, and declared in no header: not part of the interface
DEBUG_SIGNATURES = {
    "mrcal_amd_debug_camblock_route": (i, [i]*7 + [ip]),
    "mrcal_amd_debug_lchol_plan": (None, [i]*4 + [ip]),
    "mrcal_amd_debug_plan_gen_rows": (i, [i]*5 + [ip]*3 + [i]),
    "mrcal_amd_debug_dest_lists": (i, [i] + [ip]*3 + [i]),
}


class MrcalLib:
    """One loaded shared library exporting the mrcal C ABI of this path"""

    def __init__(self, path):
        if not os.path.exists(path):
            raise OSError(f"{path} does not exist")
        self.path = path
        self.lib  = C.CDLL(path)
        # (a symbol the library lacks is passed over: the reference's own library has none of the mrcal_amd_* names)
        for table in (SIGNATURES, DEBUG_SIGNATURES):
            for name, (restype, argtypes) in table.items():
                f = getattr(self.lib, name, None)
                if f is not None:
                    f.restype, f.argtypes = restype, argtypes

    def has_symbol(self, name):
        return hasattr(self.lib, name)

    def lensmodel(self, name):
        m = Lensmodel()
        if not self.lib.mrcal_lensmodel_from_name(C.byref(m), name.encode()):
            raise RuntimeError(f"Couldn't parse 'lensmodel' argument '{name}'. "
                               "Is it a string of a known lens model?")
        return m
