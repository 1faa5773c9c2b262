"""The C ABI of libts2d.so as ctypes sees it, declared once: the mirrors of the structs of include/*.h and the signature of every function
they declare (and of the lab library's additions, csrc/ts2d_lab.h, and of the other eleven product libraries: libts_geom.so, include/ts_geom.h, libts_bvh.so, include/ts_bvh.h, libts_ray.so, include/ts_ray.h, libts_volume.so, include/ts_volume.h, libts_color.so, include/ts_color.h, libts_simplify.so, include/ts_simplify.h, libts_smooth.so, include/ts_smooth.h, libts_holes.so, include/ts_holes.h, libts_manifold.so, include/ts_manifold.h, libts_orient.so, include/ts_orient.h, and libts_atlas.so, include/ts_atlas.h).  Pure ctypes: no torch, no library is loaded here -- `_C.py` binds the
library the package loads, the CPU tests bind a CDLL of their own.  tests/test_cabi_cpu.py holds both tables against the headers: the structs
by sizeof / offsetof, the functions prototype by prototype.

Pointers to device memory and opaque handles (streams, workspaces) are c_void_p; a pointer the HOST dereferences is typed by what it points
at: POINTER(mirror) for a struct, POINTER(scalar) for a value the callee returns through it, POINTER(c_void_p) for an array of pointers.
"""
import ctypes as C

_vp = C.c_void_p


class _Camera(C.Structure):  # ts2d_camera
    _fields_ = [("width", C.c_int32), ("height", C.c_int32), ("tan_fovx", C.c_float), ("tan_fovy", C.c_float),
                ("viewmatrix", _vp), ("projmatrix", _vp), ("campos", _vp)]


class _Geometry(C.Structure):  # ts2d_geometry
    _fields_ = [("P", C.c_int32), ("sh_degree", C.c_int32), ("M", C.c_int32), ("C", C.c_int32),
                ("gamma", C.c_float), ("scale_modifier", C.c_float), ("background_depth", C.c_float),
                ("background", _vp), ("vertex", _vp), ("shs", _vp), ("feature", _vp), ("opacity", _vp), ("background_depth_dev", _vp)]


class _ForwardOut(C.Structure):  # ts2d_forward_out
    _fields_ = [("out_feature", _vp), ("depth", _vp), ("normal", _vp), ("contrib_sum", _vp), ("contrib_max", _vp)]


class _LossGrads(C.Structure):  # ts2d_loss_grads
    _fields_ = [("dL_dout_feature", _vp), ("dL_dout_depth", _vp), ("dL_dout_normal", _vp)]


class _BackwardOut(C.Structure):  # ts2d_backward_out
    _fields_ = [("dL_dvertex", _vp), ("dL_dcenter2D", _vp), ("dL_dshs", _vp), ("dL_dfeature", _vp),
                ("dL_dopacity", _vp)]


class _State(C.Structure):  # ts2d_state
    _fields_ = [("geometry", _vp), ("geometry_bytes", C.c_size_t), ("binning", _vp), ("binning_bytes", C.c_size_t),
                ("image", _vp), ("image_bytes", C.c_size_t)]


class _Slice(C.Structure):  # tso_adam_slice, include/ts_optim.h
    _fields_ = [("param", _vp), ("grad", _vp), ("exp_avg", _vp), ("exp_avg_sq", _vp), ("count", C.c_int64), ("step_size", C.c_float),
                ("bias2_sqrt", C.c_float), ("grad_scale", C.c_float), ("step_size_tail", C.c_float), ("index0", C.c_int64),
                ("period", C.c_int32), ("split", C.c_int32)]


class _RowSlice(C.Structure):  # tso_row_slice, include/ts_optim.h
    _fields_ = [("param", _vp), ("grad", _vp), ("exp_avg", _vp), ("exp_avg_sq", _vp), ("floats_per_row", C.c_int32), ("step_size", C.c_float),
                ("bias2_sqrt", C.c_float), ("grad_scale", C.c_float)]


SH_ROW_SLICES = 2  # TSO_SH_ROW_SLICES


class _ShFactoredStep(C.Structure):  # tso_sh_factored_step, include/ts_optim.h
    _fields_ = [("P", C.c_int32), ("M", C.c_int32), ("sh_degree", C.c_int32), ("V", C.c_int32), ("vertex", _vp), ("campos", _vp), ("dL_dcolor", _vp),
                ("param_dc", _vp), ("exp_avg_dc", _vp), ("exp_avg_sq_dc", _vp), ("param_rest", _vp), ("exp_avg_rest", _vp), ("exp_avg_sq_rest", _vp),
                ("dc_stride", C.c_int64), ("rest_stride", C.c_int64), ("step_size_dc", C.c_float), ("bias2_sqrt_dc", C.c_float),
                ("step_size_rest", C.c_float), ("bias2_sqrt_rest", C.c_float), ("grad_scale", C.c_float), ("num_rows", C.c_int32),
                ("rows", _RowSlice * SH_ROW_SLICES)]


# name -> (restype, argtypes), header by header in the headers' order
SIGNATURES = {
    # ---- include/ts2d.h
    "ts2d_version": (C.c_char_p, []),
    "ts2d_last_error": (C.c_char_p, []),
    "ts2d_geometry_state_bytes": (C.c_size_t, [C.c_int32]),
    "ts2d_binning_state_bytes": (C.c_size_t, [C.c_int64, C.c_int32, C.c_int32]),
    "ts2d_image_state_bytes": (C.c_size_t, [C.c_int32, C.c_int32]),
    "ts2d_backward_scratch_bytes": (C.c_size_t, [C.c_int32]),
    "ts2d_binning_capacity": (C.c_int64, [C.c_size_t, C.c_int32, C.c_int32]),
    "ts2d_forward_bin": (C.c_int, [C.POINTER(_Camera), C.POINTER(_Geometry), C.c_uint32, _vp, C.POINTER(_State), C.POINTER(C.c_int64), _vp]),
    "ts2d_forward_render": (C.c_int, [C.POINTER(_Camera), C.POINTER(_Geometry), C.c_uint32, C.c_int64, C.POINTER(_State), C.POINTER(_ForwardOut),
                                      _vp]),
    "ts2d_backward": (C.c_int, [C.POINTER(_Camera), C.POINTER(_Geometry), C.c_uint32, C.c_int64, _vp, C.POINTER(_State), C.POINTER(_LossGrads), _vp,
                                C.c_size_t, C.POINTER(_BackwardOut), _vp]),
    "ts2d_backward_ranged": (C.c_int, [C.POINTER(_Camera), C.POINTER(_Geometry), C.c_uint32, C.c_int64, _vp, C.POINTER(_State),
                                       C.POINTER(_LossGrads), _vp, C.c_size_t, C.POINTER(_BackwardOut), C.c_int32, C.POINTER(_vp), _vp]),
    "ts2d_backward_range_rows": (C.c_int32, [C.c_int32, C.c_int32]),
    "ts2d_forward": (C.c_int, [C.POINTER(_Camera), C.POINTER(_Geometry), C.c_uint32, _vp, C.POINTER(_State), C.c_int64, C.POINTER(_ForwardOut), _vp]),
    "ts2d_forward_speculative": (C.c_int, [C.POINTER(_Camera), C.POINTER(_Geometry), C.c_uint32, _vp, C.POINTER(_State), C.POINTER(_ForwardOut),
                                           C.POINTER(C.c_int64), _vp]),
    "ts2d_instance_capacity_hint": (C.c_int64, [C.c_int32, C.c_int32, C.c_int32, C.c_uint32]),
    "ts2d_set_capacity_hint_key": (None, [C.c_uint64]),
    "ts2d_speculative_overflow_count": (C.c_uint64, []),
    "ts2d_forward_status": (C.c_int, [C.POINTER(_State), C.c_int32, C.c_int32, C.c_int32, C.POINTER(C.c_int32), C.POINTER(C.c_int64), _vp]),
    "ts2d_sh_grad_expand": (C.c_int, [C.c_int32, C.c_int32, C.c_int32, C.c_int32, _vp, _vp, _vp, _vp, _vp]),
    "ts2d_profile_enable": (None, [C.c_int]),
    "ts2d_profile_only": (None, [C.c_char_p]),
    "ts2d_profile_reset": (None, []),
    "ts2d_profile_read": (C.c_int, [C.c_int32, C.c_char_p, C.c_size_t, C.POINTER(C.c_double), C.POINTER(C.c_int64)]),
    # ---- include/ts_loss.h
    "tsl_workspace_bytes": (C.c_size_t, [C.c_int32, C.c_int32, C.c_int32]),
    "tsl_photometric_forward": (C.c_int, [_vp, _vp, C.c_int32, C.c_int32, C.c_int32, C.c_float, C.c_float, C.c_int32, _vp, C.c_size_t, _vp, _vp]),
    "tsl_photometric_backward": (C.c_int, [_vp, _vp, C.c_int32, C.c_int32, C.c_int32, C.c_float, C.c_float, _vp, C.c_size_t, _vp, _vp, _vp]),
    "tsl_depth_normal_workspace_bytes": (C.c_size_t, [C.c_int32, C.c_int32, C.c_double]),
    "tsl_depth_normal_forward": (C.c_int, [_vp, _vp, C.c_int32, C.c_int32, C.c_float, C.c_float, C.c_double, C.c_float, _vp, C.c_size_t, _vp, _vp]),
    "tsl_depth_normal_backward": (C.c_int, [_vp, _vp, C.c_int32, C.c_int32, C.c_float, C.c_float, C.c_double, _vp, C.c_size_t, _vp, _vp, _vp, _vp]),
    "tsl_aux_loss_workspace_bytes": (C.c_size_t, [C.c_int32, C.c_int32, C.c_int32, C.c_double]),
    "tsl_dog_mask": (C.c_int, [_vp, C.c_int32, C.c_int32, C.c_int32, C.c_double, C.c_int32, C.c_double, C.c_int32, C.c_int32, C.c_double, _vp,
                               C.c_size_t, _vp, _vp]),
    "tsl_smoothness_mask": (C.c_int, [_vp, C.c_int32, C.c_int32, C.c_int32, C.c_double, C.c_float, _vp, C.c_size_t, _vp, _vp]),
    "tsl_masked_l1_forward": (C.c_int, [_vp, _vp, _vp, C.c_int32, C.c_int32, C.c_int32, _vp, C.c_size_t, _vp, _vp]),
    "tsl_masked_l1_backward": (C.c_int, [_vp, _vp, _vp, C.c_int32, C.c_int32, C.c_int32, _vp, _vp, _vp]),
    "tsl_scharr_smoothness_forward": (C.c_int, [_vp, _vp, C.c_int32, C.c_int32, C.c_int32, _vp, C.c_size_t, _vp, _vp]),
    "tsl_scharr_smoothness_backward": (C.c_int, [_vp, _vp, C.c_int32, C.c_int32, C.c_int32, _vp, C.c_size_t, _vp, _vp, _vp]),
    "tsl_downsample_forward": (C.c_int, [_vp, C.c_int32, C.c_int32, C.c_int32, C.c_int32, C.c_int32, _vp, _vp]),
    "tsl_downsample_backward": (C.c_int, [_vp, C.c_int32, C.c_int32, C.c_int32, C.c_int32, C.c_int32, _vp, _vp]),
    "tsl_downsample_forward_planes": (C.c_int, [C.c_int32, C.POINTER(_vp), C.c_int32, C.c_int32, C.c_int32, C.c_int32, C.POINTER(_vp), _vp]),
    "tsl_downsample_backward_planes": (C.c_int, [C.c_int32, C.POINTER(_vp), C.c_int32, C.c_int32, C.c_int32, C.c_int32, C.POINTER(_vp), _vp]),
    "tsl_reg_workspace_bytes": (C.c_size_t, []),
    "tsl_reg_prepared_bytes": (C.c_size_t, [C.c_int32]),
    "tsl_reg_prepare": (C.c_int, [C.c_int32, _vp, _vp, C.c_size_t, _vp]),
    "tsl_reg_forward": (C.c_int, [C.c_int32, _vp, _vp, _vp, C.c_float, C.c_float, C.c_int32, C.c_float, _vp, C.c_size_t, _vp, _vp]),
    "tsl_reg_backward": (C.c_int, [C.c_int32, _vp, _vp, _vp, _vp, C.c_size_t, C.c_float, C.c_float, C.c_int32, C.c_float, _vp, _vp, _vp, _vp]),
    "tsl_color_affine_forward": (C.c_int, [_vp, C.c_int32, C.c_int32, _vp, _vp, _vp, _vp]),
    "tsl_color_affine_backward": (C.c_int, [_vp, C.c_int32, C.c_int32, _vp, _vp, _vp, _vp, C.c_size_t, _vp, _vp, _vp, _vp]),
    # ---- include/ts_knn.h
    "tsk_workspace_bytes": (C.c_size_t, [C.c_int32]),
    "tsk_mean_dist3": (C.c_int, [C.c_int32, _vp, _vp, _vp, C.c_size_t, _vp]),
    "tsk_nearest_other": (C.c_int, [C.c_int32, C.c_int32, _vp, _vp, _vp, C.c_size_t, _vp]),
    # ---- include/ts_model.h
    "tsm_training_statistic": (C.c_int, [C.c_int32, C.c_int32, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp]),
    "tsm_select_scratch_bytes": (C.c_size_t, [C.c_int32]),
    "tsm_select_rows": (C.c_int, [C.c_int32, _vp, C.c_int32, _vp, _vp, C.c_size_t, C.POINTER(C.c_uint32), _vp]),
    "tsm_scatter_rows": (C.c_int, [C.c_int64, C.c_int32, _vp, _vp, _vp, C.c_int64, _vp]),
    "tsm_gather_rows": (C.c_int, [C.c_int64, C.c_int32, _vp, _vp, _vp, C.c_int64, _vp]),
    "tsm_grow_classify": (C.c_int, [C.c_int32, _vp, _vp, _vp, C.c_float, C.c_float, C.c_float, _vp, _vp]),
    "tsm_split_vertex": (C.c_int, [C.c_int32, _vp, _vp, _vp, _vp, _vp]),
    "tsm_update_mask": (C.c_int, [C.c_int32, C.c_int32, _vp, _vp, _vp, C.c_float, C.c_float, _vp, _vp]),
    "tsm_clip": (C.c_int, [C.c_int32, C.c_int32, _vp, C.c_float, _vp, _vp, _vp, _vp]),
    "tsm_opacity_reset": (C.c_int, [C.c_int32, C.c_float, _vp, _vp, _vp, _vp]),
    "tsm_max_vertex_distance": (C.c_int, [C.c_int32, _vp, _vp, _vp, _vp]),
    "tsm_state_digest": (C.c_int, [C.c_int32, C.POINTER(_vp), C.POINTER(C.c_uint64), _vp, _vp]),
    # ---- include/ts_optim.h
    "tso_adam_step": (C.c_int, [C.POINTER(_Slice), C.c_int32, C.c_double, C.c_double, C.c_double, _vp]),
    "tso_adam_step_sh_factored": (C.c_int, [C.POINTER(_ShFactoredStep), C.c_double, C.c_double, C.c_double, _vp]),
    # ---- include/ts_mesh.h
    "ts2d_mesh_geometry_state_bytes": (C.c_size_t, [C.c_int32]),
    "ts2d_mesh_bin": (C.c_int, [C.POINTER(_Camera), C.c_float, C.c_int32, _vp, C.c_int32, _vp, C.POINTER(_State), C.POINTER(C.c_int64), _vp]),
    "ts2d_mesh_render": (C.c_int, [C.POINTER(_Camera), C.c_int32, _vp, _vp, C.c_int64, C.POINTER(_State), _vp, _vp, _vp, _vp, _vp]),
    "ts2d_mesh_render_counted": (C.c_int, [C.POINTER(_Camera), C.c_int32, _vp, _vp, C.c_int64, C.POINTER(_State), _vp, _vp, _vp, _vp, _vp, _vp]),
    "ts2d_mesh_census_add": (C.c_int, [C.c_int32, C.c_int32, C.c_int32, _vp, _vp, _vp, _vp, _vp]),
    # ---- include/ts_weld.h
    "ts2d_weld_workspace_bytes": (C.c_size_t, [C.c_int32, C.c_int32]),
    "ts2d_weld_labels": (C.c_int, [C.c_int32, _vp, C.c_float, _vp, _vp, C.c_size_t, _vp]),
    "ts2d_weld_labels_counted": (C.c_int, [C.c_int32, _vp, C.c_float, _vp, _vp, _vp, C.c_size_t, _vp]),
    "ts2d_weld_face_components": (C.c_int, [C.c_int32, C.c_int32, _vp, _vp, _vp, _vp, C.c_size_t, _vp]),
    "ts2d_weld_compact": (C.c_int, [C.c_int32, _vp, _vp, C.c_int32, _vp, _vp, _vp, _vp, C.c_size_t, _vp]),
    "ts2d_weld_remap_faces": (C.c_int, [C.c_int32, C.c_int32, _vp, _vp, _vp, _vp, _vp]),
    "ts2d_weld_edge_census": (C.c_int, [C.c_int32, C.c_int32, _vp, _vp, _vp, _vp, C.c_size_t, _vp]),
}

# what csrc/ts2d_lab.h adds in tools/bin/libts2d_lab.so (the test hooks: only in a library built with them)
LAB_SIGNATURES = {
    "ts2d_debug_read_state": (C.c_int, [C.POINTER(_State), C.c_int32, C.c_int64, C.c_int32, C.c_int32, C.c_int32, _vp, C.c_size_t, _vp]),
    "ts2d_test_sort_pairs": (C.c_int, [_vp, _vp, _vp, _vp, C.c_size_t, C.c_int32, C.c_int32, _vp]),
    "ts2d_test_inclusive_scan_rocprim": (C.c_int, [_vp, _vp, C.c_size_t, _vp]),
    "ts2d_lab_force_ticket_passes": (None, [C.c_int]),
    "ts2d_lab_force_depth_pass4": (None, [C.c_int]),
    "ts2d_test_quantile_scratch_bytes": (C.c_size_t, []),
    "ts2d_test_quantile": (C.c_int, [_vp, C.c_size_t, C.c_float, _vp, _vp, _vp]),
    "ts2d_lab_depth_split": (None, [C.c_int, C.c_int]),
    "ts2d_lab_force_all_quadrants": (None, [C.c_int]),
    "ts2d_lab_force_kernel_cull": (None, [C.c_int]),
}

# include/ts_geom.h: the whole C ABI of diff_recon_hip/libts_geom.so, a library of its own (diff_recon_hip/mesh_distance.py loads and binds it)
GEOM_SIGNATURES = {
    "tsg_last_error": (C.c_char_p, []),
    "tsg_cross_workspace_bytes": (C.c_size_t, [C.c_int32, C.c_int32]),
    "tsg_nearest_cross": (C.c_int, [C.c_int32, _vp, C.c_int32, _vp, _vp, _vp, _vp, _vp, C.c_size_t, _vp]),
    "tsg_sample_workspace_bytes": (C.c_size_t, [C.c_int32]),
    "tsg_face_areas": (C.c_int, [C.c_int32, C.c_int32, _vp, _vp, _vp, _vp, _vp]),
    "tsg_sample_surface": (C.c_int, [C.c_int32, C.c_int32, _vp, _vp, _vp, C.c_int32, C.c_uint64, _vp, _vp, _vp, C.c_size_t, _vp]),
}


# include/ts_bvh.h: the whole C ABI of diff_recon_hip/libts_bvh.so, the third library (diff_recon_hip/mesh_surface.py loads and binds it)
BVH_SIGNATURES = {
    "tsb_last_error": (C.c_char_p, []),
    "tsb_bvh_bytes": (C.c_size_t, [C.c_int32]),
    "tsb_build_workspace_bytes": (C.c_size_t, [C.c_int32]),
    "tsb_build": (C.c_int, [C.c_int32, C.c_int32, _vp, _vp, _vp, _vp, C.c_size_t, _vp, C.c_size_t, _vp]),
    "tsb_closest_workspace_bytes": (C.c_size_t, [C.c_int32]),
    "tsb_closest": (C.c_int, [C.c_int32, _vp, C.c_int32, C.c_int32, _vp, _vp, _vp, C.c_size_t, _vp, _vp, _vp, _vp, _vp, C.c_size_t, _vp]),
}


# include/ts_ray.h: the whole C ABI of diff_recon_hip/libts_ray.so, the fourth library (diff_recon_hip/mesh_ray.py loads and binds it)
RAY_SIGNATURES = {
    "tsr_last_error": (C.c_char_p, []),
    "tsr_cast_workspace_bytes": (C.c_size_t, [C.c_int32]),
    "tsr_cast": (C.c_int, [C.c_int32, _vp, _vp, _vp, C.c_double, C.c_double, C.c_int32, C.c_int32, _vp, C.c_size_t, _vp, _vp, _vp, _vp, _vp, _vp,
                           C.c_size_t, _vp]),
}


# include/ts_volume.h: the whole C ABI of diff_recon_hip/libts_volume.so, the fifth library (diff_recon_hip/volume.py loads and binds it)
VOLUME_SIGNATURES = {
    "tsv_last_error": (C.c_char_p, []),
    "tsv_integrate": (C.c_int, [C.c_int32, C.c_int32, C.c_int32, C.c_float, C.c_float, C.c_float, C.c_float, C.c_float, _vp, C.c_float, C.c_float,
                                C.c_int32, C.c_int32, _vp, _vp, C.c_int32, _vp, _vp, _vp, _vp]),
    "tsv_field": (C.c_int, [C.c_int32, C.c_int32, C.c_int32, _vp, _vp, C.c_int32, _vp, _vp]),
    "tsv_extract_workspace_bytes": (C.c_size_t, [C.c_int32, C.c_int32, C.c_int32]),
    "tsv_extract": (C.c_int, [C.c_int32, C.c_int32, C.c_int32, C.c_float, C.c_float, C.c_float, C.c_float, _vp, C.c_float, C.c_int64, _vp, _vp, _vp,
                              _vp, C.c_size_t, _vp]),
}


# include/ts_color.h: the whole C ABI of diff_recon_hip/libts_color.so, the sixth library (diff_recon_hip/color_volume.py loads and binds it)
COLOR_SIGNATURES = {
    "tsc_last_error": (C.c_char_p, []),
    "tsc_integrate": (C.c_int, [C.c_int32, C.c_int32, C.c_int32, C.c_float, C.c_float, C.c_float, C.c_float, C.c_float, _vp, C.c_float, C.c_float,
                                C.c_int32, C.c_int32, _vp, _vp, _vp, _vp, _vp, _vp, _vp]),
    "tsc_color_field": (C.c_int, [C.c_int32, C.c_int32, C.c_int32, _vp, _vp, C.c_int32, _vp, _vp]),
    "tsc_sample": (C.c_int, [C.c_int32, C.c_int32, C.c_int32, C.c_float, C.c_float, C.c_float, C.c_float, C.c_int32, _vp, C.c_int32, _vp, _vp, _vp,
                             _vp]),
    "tsc_interpolate": (C.c_int, [_vp, C.c_float, C.c_float, C.c_int32, C.c_int32, C.c_int32, _vp, C.c_int32, _vp, _vp, C.c_int32, _vp, _vp, _vp,
                                  _vp, _vp]),
}


# include/ts_simplify.h: the whole C ABI of diff_recon_hip/libts_simplify.so, the seventh library (diff_recon_hip/mesh_simplify.py loads and binds it)
SIMPLIFY_SIGNATURES = {
    "tsq_last_error": (C.c_char_p, []),
    "tsq_workspace_bytes": (C.c_size_t, [C.c_int32, C.c_int32]),
    "tsq_cluster_labels": (C.c_int, [C.c_int32, _vp, C.c_float, C.c_float, C.c_float, C.c_float, _vp, _vp, C.c_size_t, _vp]),
    "tsq_place": (C.c_int, [C.c_int32, C.c_int32, _vp, _vp, _vp, C.c_float, C.c_float, C.c_float, C.c_float, C.c_float, C.c_int32, _vp, _vp,
                            C.c_int32, _vp, _vp, _vp, _vp, _vp, C.c_size_t, _vp]),
    "tsq_unique_faces": (C.c_int, [C.c_int32, C.c_int32, _vp, _vp, _vp, _vp, _vp, C.c_size_t, _vp]),
}


def bind_simplify(lib):
    """Sets restype and argtypes of every function of include/ts_simplify.h on `lib` (a ctypes.CDLL of libts_simplify.so); a library that
    lacks one is refused."""
    missing = [name for name in SIMPLIFY_SIGNATURES if not hasattr(lib, name)]
    if missing:
        raise ImportError(f"{getattr(lib, '_name', lib)} does not export {', '.join(missing)}: rebuild it with `python triangle-splatting_amd/build.py`")
    for name, (restype, argtypes) in SIMPLIFY_SIGNATURES.items():
        fn = getattr(lib, name)
        fn.restype, fn.argtypes = restype, argtypes
    return lib


def bind_color(lib):
    """Sets restype and argtypes of every function of include/ts_color.h on `lib` (a ctypes.CDLL of libts_color.so); a library that lacks one
    is refused."""
    missing = [name for name in COLOR_SIGNATURES if not hasattr(lib, name)]
    if missing:
        raise ImportError(f"{getattr(lib, '_name', lib)} does not export {', '.join(missing)}: rebuild it with `python triangle-splatting_amd/build.py`")
    for name, (restype, argtypes) in COLOR_SIGNATURES.items():
        fn = getattr(lib, name)
        fn.restype, fn.argtypes = restype, argtypes
    return lib


def bind_volume(lib):
    """Sets restype and argtypes of every function of include/ts_volume.h on `lib` (a ctypes.CDLL of libts_volume.so); a library that lacks
    one is refused."""
    missing = [name for name in VOLUME_SIGNATURES if not hasattr(lib, name)]
    if missing:
        raise ImportError(f"{getattr(lib, '_name', lib)} does not export {', '.join(missing)}: rebuild it with `python triangle-splatting_amd/build.py`")
    for name, (restype, argtypes) in VOLUME_SIGNATURES.items():
        fn = getattr(lib, name)
        fn.restype, fn.argtypes = restype, argtypes
    return lib


def bind_ray(lib):
    """Sets restype and argtypes of every function of include/ts_ray.h on `lib` (a ctypes.CDLL of libts_ray.so); a library that lacks one is
    refused."""
    missing = [name for name in RAY_SIGNATURES if not hasattr(lib, name)]
    if missing:
        raise ImportError(f"{getattr(lib, '_name', lib)} does not export {', '.join(missing)}: rebuild it with `python triangle-splatting_amd/build.py`")
    for name, (restype, argtypes) in RAY_SIGNATURES.items():
        fn = getattr(lib, name)
        fn.restype, fn.argtypes = restype, argtypes
    return lib


def bind_bvh(lib):
    """Sets restype and argtypes of every function of include/ts_bvh.h on `lib` (a ctypes.CDLL of libts_bvh.so); a library that lacks one is
    refused."""
    missing = [name for name in BVH_SIGNATURES if not hasattr(lib, name)]
    if missing:
        raise ImportError(f"{getattr(lib, '_name', lib)} does not export {', '.join(missing)}: rebuild it with `python triangle-splatting_amd/build.py`")
    for name, (restype, argtypes) in BVH_SIGNATURES.items():
        fn = getattr(lib, name)
        fn.restype, fn.argtypes = restype, argtypes
    return lib


def bind_geom(lib):
    """Sets restype and argtypes of every function of include/ts_geom.h on `lib` (a ctypes.CDLL of libts_geom.so); a library that lacks one is
    refused."""
    missing = [name for name in GEOM_SIGNATURES if not hasattr(lib, name)]
    if missing:
        raise ImportError(f"{getattr(lib, '_name', lib)} does not export {', '.join(missing)}: rebuild it with `python triangle-splatting_amd/build.py`")
    for name, (restype, argtypes) in GEOM_SIGNATURES.items():
        fn = getattr(lib, name)
        fn.restype, fn.argtypes = restype, argtypes
    return lib


def bind(lib):
    """Sets restype and argtypes of every function of the C ABI on `lib` (a ctypes.CDLL of libts2d.so or of one of its lab / variant builds),
    and of the lab entry points it has.  A library that lacks a product function is refused."""
    missing = [name for name in SIGNATURES if not hasattr(lib, name)]
    if missing:
        raise ImportError(f"{getattr(lib, '_name', lib)} does not export {', '.join(missing)}: rebuild it with `python triangle-splatting_amd/build.py`")
    for table in (SIGNATURES, LAB_SIGNATURES):
        for name, (restype, argtypes) in table.items():
            if table is SIGNATURES or hasattr(lib, name):
                fn = getattr(lib, name)
                fn.restype, fn.argtypes = restype, argtypes
    return lib


# include/ts_smooth.h: the whole C ABI of diff_recon_hip/libts_smooth.so, the eighth library (diff_recon_hip/mesh_smooth.py loads and binds it)
SMOOTH_SIGNATURES = {
    "tss_last_error": (C.c_char_p, []),
    "tss_workspace_bytes": (C.c_size_t, [C.c_int32, C.c_int32]),
    "tss_adjacency": (C.c_int, [C.c_int32, C.c_int32, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, C.c_size_t, _vp]),
    "tss_smooth": (C.c_int, [C.c_int32, _vp, _vp, _vp, _vp, C.c_int32, _vp, _vp, C.c_float, C.c_float, C.c_int32, C.c_int32, C.c_float, _vp, _vp,
                             C.c_size_t, _vp]),
    "tss_face_normals": (C.c_int, [C.c_int32, C.c_int32, _vp, _vp, _vp, _vp, _vp, _vp]),
    "tss_vertex_normals": (C.c_int, [C.c_int32, C.c_int32, _vp, _vp, _vp, C.c_int32, _vp, _vp, _vp, _vp, C.c_size_t, _vp]),
}


def bind_smooth(lib):
    """Sets restype and argtypes of every function of include/ts_smooth.h on `lib` (a ctypes.CDLL of libts_smooth.so); a library that
    lacks one is refused."""
    missing = [name for name in SMOOTH_SIGNATURES if not hasattr(lib, name)]
    if missing:
        raise ImportError(f"{getattr(lib, '_name', lib)} does not export {', '.join(missing)}: rebuild it with `python triangle-splatting_amd/build.py`")
    for name, (restype, argtypes) in SMOOTH_SIGNATURES.items():
        fn = getattr(lib, name)
        fn.restype, fn.argtypes = restype, argtypes
    return lib


# include/ts_holes.h: the whole C ABI of diff_recon_hip/libts_holes.so, the ninth library (diff_recon_hip/mesh_holes.py loads and binds it)
HOLES_SIGNATURES = {
    "tsh_last_error": (C.c_char_p, []),
    "tsh_workspace_bytes": (C.c_size_t, [C.c_int32, C.c_int32]),
    "tsh_loops": (C.c_int, [C.c_int32, C.c_int32, _vp, _vp, _vp, _vp, _vp, C.c_int32, _vp, _vp, _vp, _vp, _vp, C.c_size_t, _vp]),
    "tsh_fill": (C.c_int, [C.c_int32, C.c_int32, _vp, _vp, C.c_int32, _vp, _vp, C.c_int32, C.c_int32, _vp, _vp, C.c_int32, _vp, _vp, _vp, _vp, _vp,
                           _vp, _vp, _vp, C.c_size_t, _vp]),
}


def bind_holes(lib):
    """Sets restype and argtypes of every function of include/ts_holes.h on `lib` (a ctypes.CDLL of libts_holes.so); a library that
    lacks one is refused."""
    missing = [name for name in HOLES_SIGNATURES if not hasattr(lib, name)]
    if missing:
        raise ImportError(f"{getattr(lib, '_name', lib)} does not export {', '.join(missing)}: rebuild it with `python triangle-splatting_amd/build.py`")
    for name, (restype, argtypes) in HOLES_SIGNATURES.items():
        fn = getattr(lib, name)
        fn.restype, fn.argtypes = restype, argtypes
    return lib


# include/ts_manifold.h: the whole C ABI of diff_recon_hip/libts_manifold.so, the tenth library (diff_recon_hip/mesh_manifold.py loads and binds it)
MANIFOLD_SIGNATURES = {
    "tsf_last_error": (C.c_char_p, []),
    "tsf_workspace_bytes": (C.c_size_t, [C.c_int32, C.c_int32]),
    "tsf_fans": (C.c_int, [C.c_int32, C.c_int32, _vp, _vp, _vp, _vp, _vp, _vp, C.c_size_t, _vp]),
    "tsf_split": (C.c_int, [C.c_int32, C.c_int32, _vp, _vp, _vp, C.c_int32, _vp, _vp, _vp, _vp, _vp, C.c_size_t, _vp]),
}


def bind_manifold(lib):
    """Sets restype and argtypes of every function of include/ts_manifold.h on `lib` (a ctypes.CDLL of libts_manifold.so); a library that
    lacks one is refused."""
    missing = [name for name in MANIFOLD_SIGNATURES if not hasattr(lib, name)]
    if missing:
        raise ImportError(f"{getattr(lib, '_name', lib)} does not export {', '.join(missing)}: rebuild it with `python triangle-splatting_amd/build.py`")
    for name, (restype, argtypes) in MANIFOLD_SIGNATURES.items():
        fn = getattr(lib, name)
        fn.restype, fn.argtypes = restype, argtypes
    return lib


# include/ts_orient.h: the whole C ABI of diff_recon_hip/libts_orient.so, the eleventh library (diff_recon_hip/mesh_orient.py loads and binds it)
ORIENT_SIGNATURES = {
    "tsw_last_error": (C.c_char_p, []),
    "tsw_workspace_bytes": (C.c_size_t, [C.c_int32, C.c_int32]),
    "tsw_orient": (C.c_int, [C.c_int32, C.c_int32, _vp, _vp, _vp, C.c_int32, _vp, _vp, _vp, _vp, _vp, C.c_size_t, _vp]),
}


def bind_orient(lib):
    """Sets restype and argtypes of every function of include/ts_orient.h on `lib` (a ctypes.CDLL of libts_orient.so); a library that
    lacks one is refused."""
    missing = [name for name in ORIENT_SIGNATURES if not hasattr(lib, name)]
    if missing:
        raise ImportError(f"{getattr(lib, '_name', lib)} does not export {', '.join(missing)}: rebuild it with `python triangle-splatting_amd/build.py`")
    for name, (restype, argtypes) in ORIENT_SIGNATURES.items():
        fn = getattr(lib, name)
        fn.restype, fn.argtypes = restype, argtypes
    return lib


# include/ts_atlas.h: the whole C ABI of diff_recon_hip/libts_atlas.so, the twelfth library (diff_recon_hip/mesh_texture.py loads and binds it)
ATLAS_SIGNATURES = {
    "tsa_last_error": (C.c_char_p, []),
    "tsa_texel_index": (C.c_int, [_vp, C.c_float, C.c_float, C.c_int32, C.c_int32, C.c_int32, _vp, C.c_int32, _vp, _vp, C.c_int32, C.c_int32, _vp,
                                  _vp, _vp, _vp]),
    "tsa_face_totals": (C.c_int, [C.c_int32, C.c_int32, _vp, _vp, _vp]),
    "tsa_resolve": (C.c_int, [C.c_int32, C.c_int32, C.c_int32, C.c_int32, _vp, _vp, C.c_int32, _vp, C.POINTER(C.c_float), _vp, _vp, _vp, _vp]),
    "tsa_render": (C.c_int, [C.c_int32, C.c_int32, C.c_int32, C.c_int32, _vp, _vp, _vp, _vp, _vp]),
}


def bind_atlas(lib):
    """Sets restype and argtypes of every function of include/ts_atlas.h on `lib` (a ctypes.CDLL of libts_atlas.so); a library that
    lacks one is refused."""
    missing = [name for name in ATLAS_SIGNATURES if not hasattr(lib, name)]
    if missing:
        raise ImportError(f"{getattr(lib, '_name', lib)} does not export {', '.join(missing)}: rebuild it with `python triangle-splatting_amd/build.py`")
    for name, (restype, argtypes) in ATLAS_SIGNATURES.items():
        fn = getattr(lib, name)
        fn.restype, fn.argtypes = restype, argtypes
    return lib


# include/ts_inside.h: the whole C ABI of diff_recon_hip/libts_inside.so, the thirteenth library (diff_recon_hip/mesh_inside.py loads and binds it)
INSIDE_SIGNATURES = {
    "tsi_last_error": (C.c_char_p, []),
    "tsi_crossings_workspace_bytes": (C.c_size_t, [C.c_int32]),
    "tsi_crossings": (C.c_int, [C.c_int32, _vp, _vp, C.c_int32, _vp, C.c_double, C.c_double, C.c_int32, _vp, C.c_size_t, _vp, _vp, _vp, _vp, _vp,
                                C.c_size_t, _vp]),
    "tsi_signed_distance": (C.c_int, [C.c_int32, _vp, _vp, _vp, _vp, C.c_int32, C.c_int32, _vp, _vp, _vp]),
}


def bind_inside(lib):
    """Sets restype and argtypes of every function of include/ts_inside.h on `lib` (a ctypes.CDLL of libts_inside.so); a library that
    lacks one is refused."""
    missing = [name for name in INSIDE_SIGNATURES if not hasattr(lib, name)]
    if missing:
        raise ImportError(f"{getattr(lib, '_name', lib)} does not export {', '.join(missing)}: rebuild it with `python triangle-splatting_amd/build.py`")
    for name, (restype, argtypes) in INSIDE_SIGNATURES.items():
        fn = getattr(lib, name)
        fn.restype, fn.argtypes = restype, argtypes
    return lib


# include/ts_winding.h: the whole C ABI of diff_recon_hip/libts_winding.so, the fourteenth library (diff_recon_hip/mesh_winding.py loads and binds it)
WINDING_SIGNATURES = {
    "tsn_last_error": (C.c_char_p, []),
    "tsn_moments_bytes": (C.c_size_t, [C.c_int32]),
    "tsn_leaf_faces_bytes": (C.c_size_t, [C.c_int32]),
    "tsn_moments": (C.c_int, [C.c_int32, _vp, C.c_size_t, _vp, C.c_size_t, _vp, C.c_size_t, _vp]),
    "tsn_winding_workspace_bytes": (C.c_size_t, [C.c_int32]),
    "tsn_winding": (C.c_int, [C.c_int32, _vp, C.c_double, C.c_int32, _vp, C.c_size_t, _vp, C.c_size_t, _vp, _vp, _vp, C.c_size_t, _vp]),
    "tsn_sign_distance": (C.c_int, [C.c_int32, _vp, _vp, C.c_int64, _vp, _vp, _vp]),
}


def bind_winding(lib):
    """Sets restype and argtypes of every function of include/ts_winding.h on `lib` (a ctypes.CDLL of libts_winding.so); a library that
    lacks one is refused."""
    missing = [name for name in WINDING_SIGNATURES if not hasattr(lib, name)]
    if missing:
        raise ImportError(f"{getattr(lib, '_name', lib)} does not export {', '.join(missing)}: rebuild it with `python triangle-splatting_amd/build.py`")
    for name, (restype, argtypes) in WINDING_SIGNATURES.items():
        fn = getattr(lib, name)
        fn.restype, fn.argtypes = restype, argtypes
    return lib


# include/ts_overlap.h: the whole C ABI of diff_recon_hip/libts_overlap.so, the fifteenth library (diff_recon_hip/mesh_overlap.py loads and binds it)
OVERLAP_SIGNATURES = {
    "tsx_last_error": (C.c_char_p, []),
    "tsx_overlap": (C.c_int, [C.c_int32, _vp, C.c_size_t, _vp, C.c_int32, _vp, C.c_size_t, _vp, _vp, _vp, C.c_int32, _vp, _vp, _vp, _vp]),
    "tsx_sort_workspace_bytes": (C.c_size_t, [C.c_int32]),
    "tsx_sort_pairs": (C.c_int, [C.c_int32, C.c_int32, C.c_int32, _vp, _vp, _vp, C.c_size_t, _vp]),
}


def bind_overlap(lib):
    """Sets restype and argtypes of every function of include/ts_overlap.h on `lib` (a ctypes.CDLL of libts_overlap.so); a library that
    lacks one is refused."""
    missing = [name for name in OVERLAP_SIGNATURES if not hasattr(lib, name)]
    if missing:
        raise ImportError(f"{getattr(lib, '_name', lib)} does not export {', '.join(missing)}: rebuild it with `python triangle-splatting_amd/build.py`")
    for name, (restype, argtypes) in OVERLAP_SIGNATURES.items():
        fn = getattr(lib, name)
        fn.restype, fn.argtypes = restype, argtypes
    return lib


# include/ts_subdivide.h: the whole C ABI of diff_recon_hip/libts_subdivide.so, the sixteenth library (diff_recon_hip/mesh_subdivide.py loads and binds it)
SUBDIVIDE_SIGNATURES = {
    "tsd_last_error": (C.c_char_p, []),
    "tsd_workspace_bytes": (C.c_size_t, [C.c_int32, C.c_int32]),
    "tsd_edges": (C.c_int, [C.c_int32, C.c_int32, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, C.c_size_t, _vp]),
    "tsd_split": (C.c_int, [C.c_int32, C.c_int32, _vp, _vp, _vp, C.c_int32, C.c_float, _vp, _vp, _vp, C.c_int32, _vp, _vp, _vp, _vp, _vp, _vp, _vp,
                            _vp, C.c_size_t, _vp]),
}


def bind_subdivide(lib):
    """Sets restype and argtypes of every function of include/ts_subdivide.h on `lib` (a ctypes.CDLL of libts_subdivide.so); a library that
    lacks one is refused."""
    missing = [name for name in SUBDIVIDE_SIGNATURES if not hasattr(lib, name)]
    if missing:
        raise ImportError(f"{getattr(lib, '_name', lib)} does not export {', '.join(missing)}: rebuild it with `python triangle-splatting_amd/build.py`")
    for name, (restype, argtypes) in SUBDIVIDE_SIGNATURES.items():
        fn = getattr(lib, name)
        fn.restype, fn.argtypes = restype, argtypes
    return lib


# include/ts_flip.h: the whole C ABI of diff_recon_hip/libts_flip.so, the seventeenth library (diff_recon_hip/mesh_flip.py loads and binds it)
FLIP_SIGNATURES = {
    "tse_last_error": (C.c_char_p, []),
    "tse_workspace_bytes": (C.c_size_t, [C.c_int32, C.c_int32]),
    "tse_flip": (C.c_int, [C.c_int32, C.c_int32, _vp, _vp, _vp, C.c_float, C.c_uint32, _vp, _vp, _vp, _vp, _vp, _vp, _vp, C.c_size_t, _vp]),
}


def bind_flip(lib):
    """Sets restype and argtypes of every function of include/ts_flip.h on `lib` (a ctypes.CDLL of libts_flip.so); a library that lacks one
    is refused."""
    missing = [name for name in FLIP_SIGNATURES if not hasattr(lib, name)]
    if missing:
        raise ImportError(f"{getattr(lib, '_name', lib)} does not export {', '.join(missing)}: rebuild it with `python triangle-splatting_amd/build.py`")
    for name, (restype, argtypes) in FLIP_SIGNATURES.items():
        fn = getattr(lib, name)
        fn.restype, fn.argtypes = restype, argtypes
    return lib


# include/ts_collapse.h: the whole C ABI of diff_recon_hip/libts_collapse.so, the eighteenth library (diff_recon_hip/mesh_collapse.py loads and binds it)
COLLAPSE_SIGNATURES = {
    "tsp_last_error": (C.c_char_p, []),
    "tsp_workspace_bytes": (C.c_size_t, [C.c_int32, C.c_int32]),
    "tsp_collapse": (C.c_int, [C.c_int32, C.c_int32, _vp, _vp, _vp, _vp, C.c_int32, C.c_float, _vp, C.c_float, C.c_float, C.c_uint32, _vp, _vp, _vp,
                               _vp, _vp, _vp, _vp, _vp, _vp, C.c_size_t, _vp]),
}


def bind_collapse(lib):
    """Sets restype and argtypes of every function of include/ts_collapse.h on `lib` (a ctypes.CDLL of libts_collapse.so); a library that
    lacks one is refused."""
    missing = [name for name in COLLAPSE_SIGNATURES if not hasattr(lib, name)]
    if missing:
        raise ImportError(f"{getattr(lib, '_name', lib)} does not export {', '.join(missing)}: rebuild it with `python triangle-splatting_amd/build.py`")
    for name, (restype, argtypes) in COLLAPSE_SIGNATURES.items():
        fn = getattr(lib, name)
        fn.restype, fn.argtypes = restype, argtypes
    return lib


# include/ts_decimate.h: the whole C ABI of diff_recon_hip/libts_decimate.so, the nineteenth library (diff_recon_hip/mesh_decimate.py loads and binds it)
DECIMATE_SIGNATURES = {
    "tsz_last_error": (C.c_char_p, []),
    "tsz_workspace_bytes": (C.c_size_t, [C.c_int32, C.c_int32]),
    "tsz_vertex_quadrics": (C.c_int, [C.c_int32, C.c_int32, _vp, _vp, _vp, _vp, _vp, C.c_size_t, _vp]),
    "tsz_decimate": (C.c_int, [C.c_int32, C.c_int32, _vp, _vp, _vp, _vp, _vp, C.c_float, C.c_int32, C.c_float, C.c_float, C.c_uint32, _vp, _vp, _vp,
                               _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, C.c_size_t, _vp]),
}


def bind_decimate(lib):
    """Sets restype and argtypes of every function of include/ts_decimate.h on `lib` (a ctypes.CDLL of libts_decimate.so); a library that
    lacks one is refused."""
    missing = [name for name in DECIMATE_SIGNATURES if not hasattr(lib, name)]
    if missing:
        raise ImportError(f"{getattr(lib, '_name', lib)} does not export {', '.join(missing)}: rebuild it with `python triangle-splatting_amd/build.py`")
    for name, (restype, argtypes) in DECIMATE_SIGNATURES.items():
        fn = getattr(lib, name)
        fn.restype, fn.argtypes = restype, argtypes
    return lib


# include/ts_contract.h: the whole C ABI of diff_recon_hip/libts_contract.so, the twentieth library (diff_recon_hip/mesh_contract.py loads and binds it)
CONTRACT_SIGNATURES = {
    "tsu_last_error": (C.c_char_p, []),
    "tsu_workspace_bytes": (C.c_size_t, [C.c_int32, C.c_int32]),
    "tsu_contract": (C.c_int, [C.c_int32, C.c_int32, _vp, _vp, _vp, _vp, _vp, C.c_float, C.c_int32, C.c_float, C.c_float, C.c_float, C.c_float,
                               C.c_uint32, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, C.c_size_t, _vp]),
}


def bind_contract(lib):
    """Sets restype and argtypes of every function of include/ts_contract.h on `lib` (a ctypes.CDLL of libts_contract.so); a library that
    lacks one is refused."""
    missing = [name for name in CONTRACT_SIGNATURES if not hasattr(lib, name)]
    if missing:
        raise ImportError(f"{getattr(lib, '_name', lib)} does not export {', '.join(missing)}: rebuild it with `python triangle-splatting_amd/build.py`")
    for name, (restype, argtypes) in CONTRACT_SIGNATURES.items():
        fn = getattr(lib, name)
        fn.restype, fn.argtypes = restype, argtypes
    return lib
