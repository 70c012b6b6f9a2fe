"""ctypes binding of the C ABI declared in include/eppm.h.  Fails loudly if the library is missing."""
import ctypes as C
import os

from .build import lib_path


class EppmError(RuntimeError):
    pass


class CParams(C.Structure):
    _fields_ = [("patch_r", C.c_int), ("num_iter", C.c_int), ("search_range", C.c_int), ("num_guess", C.c_int),
                ("seg_len", C.c_int), ("wmf_iters", C.c_int), ("seed", C.c_ulonglong), ("propagation", C.c_int),
                ("levels", C.c_int)]


class CTrackParams(C.Structure):
    _fields_ = [("spacing", C.c_int), ("min_eig", C.c_int64), ("fb_alpha", C.c_float), ("fb_beta", C.c_float), ("mb_alpha", C.c_float),
                ("mb_beta", C.c_float), ("capacity", C.c_int)]


class CTFilterParams(C.Structure):
    _fields_ = [("thresh", C.c_float), ("n_max", C.c_int)]


class CStabParams(C.Structure):
    _fields_ = [("tau", C.c_float), ("iters", C.c_int), ("smooth", C.c_float)]


class CGMotionModel(C.Structure):
    _fields_ = [("p", C.c_double * 6), ("n_valid", C.c_int64), ("n_inliers", C.c_int64), ("valid", C.c_int), ("passes", C.c_int)]

    def as_dict(self):
        import numpy as np
        return dict(p=np.array(self.p[:], np.float64), n_valid=int(self.n_valid), n_inliers=int(self.n_inliers), valid=int(self.valid),
                    passes=int(self.passes))


class CCutParams(C.Structure):
    _fields_ = [("lost_permille", C.c_int), ("residual_max", C.c_float)]


class CCutStats(C.Structure):
    _fields_ = [("n", C.c_int64), ("c1", C.c_int64 * 4), ("c2", C.c_int64 * 4), ("n_tracked", C.c_int64), ("sad", C.c_int64), ("cut", C.c_int32),
                ("stepped", C.c_int32)]

    def as_dict(self):
        return dict(n=int(self.n), c1=[int(x) for x in self.c1], c2=[int(x) for x in self.c2], n_tracked=int(self.n_tracked), sad=int(self.sad),
                    cut=int(self.cut), stepped=int(self.stepped))


class CMBlurParams(C.Structure):
    _fields_ = [("shutter", C.c_float), ("max_radius", C.c_float), ("taps", C.c_int)]


class CCMapParams(C.Structure):
    _fields_ = [("thresh", C.c_float), ("tear", C.c_float), ("use_occ", C.c_int)]


class CObjectsParams(C.Structure):
    _fields_ = [("tau", C.c_float), ("iters", C.c_int), ("connectivity", C.c_int), ("min_area", C.c_int), ("max_objects", C.c_int),
                ("min_overlap", C.c_int)]


class CPlateParams(C.Structure):
    _fields_ = [("tau", C.c_float), ("iters", C.c_int), ("margin_x", C.c_int), ("margin_y", C.c_int), ("grow", C.c_int), ("accept_invalid", C.c_int),
                ("thresh", C.c_float), ("n_max", C.c_int), ("min_count", C.c_int)]


class CDefectParams(C.Structure):
    _fields_ = [("detect", C.c_float), ("agree", C.c_float), ("radius", C.c_int), ("grow", C.c_int)]


class CDefectStats(C.Structure):
    _fields_ = [("hit", C.c_int), ("grown", C.c_int), ("second_chance", C.c_int), ("undecided", C.c_int)]

    def as_dict(self):
        return {k: int(getattr(self, k)) for k, _ in self._fields_}


class CDeflickerParams(C.Structure):
    _fields_ = [("cell", C.c_int), ("iters", C.c_int), ("reject", C.c_float), ("tau", C.c_float), ("keep", C.c_float), ("n_min", C.c_int)]


class CDeflickerStats(C.Structure):
    _fields_ = [("used", C.c_int64), ("valid_cells", C.c_int32), ("cells", C.c_int32)]

    def as_dict(self):
        return {k: int(getattr(self, k)) for k, _ in self._fields_}


class CObject(C.Structure):
    _fields_ = [("id", C.c_int32), ("age", C.c_int32), ("area", C.c_int32), ("x0", C.c_int32), ("y0", C.c_int32), ("x1", C.c_int32),
                ("y1", C.c_int32), ("n_flow", C.c_int32), ("sum_x", C.c_int64), ("sum_y", C.c_int64), ("sum_qu", C.c_int64), ("sum_qv", C.c_int64)]

    def as_dict(self):
        return {k: int(getattr(self, k)) for k, _ in self._fields_}


class CObjectsCounts(C.Structure):
    _fields_ = [("n", C.c_int32), ("n_found", C.c_int32), ("n_components", C.c_int32), ("next_id", C.c_int32)]

    def as_dict(self):
        return {k: int(getattr(self, k)) for k, _ in self._fields_}


class CTrackCounts(C.Structure):
    _fields_ = [("live", C.c_int), ("ended", C.c_int), ("seeded", C.c_int), ("dropped", C.c_int), ("frame", C.c_int), ("next_id", C.c_int)]

    def as_dict(self):
        return {k: int(getattr(self, k)) for k, _ in self._fields_}


_lib = None

# every symbol include/eppm.h declares (tests check that the library exports all of them)
SYMBOLS = [
    "eppm_default_params", "eppm_create", "eppm_create_batch", "eppm_batch_size", "eppm_batch_set_images", "eppm_batch_set_images_device",
    "eppm_batch_compute", "eppm_batch_compute_device", "eppm_batch_compute_end", "eppm_batch_get_plane", "eppm_destroy", "eppm_set_stream", "eppm_set_images", "eppm_set_images_device",
    "eppm_compute", "eppm_compute_begin", "eppm_compute_end", "eppm_compute_device", "eppm_synchronize", "eppm_num_levels", "eppm_level_dims", "eppm_get_plane",
    "eppm_stage_times", "eppm_clear_stage_times", "eppm_enable_stage_timing", "eppm_last_error", "eppm_version",
    "eppm_device_count", "eppm_set_device", "eppm_malloc_device", "eppm_malloc_pitched", "eppm_free_device",
    "eppm_memcpy_h2d", "eppm_memcpy_d2h", "eppm_memcpy2d_h2d", "eppm_memcpy2d_d2h", "eppm_memset_device",
    "eppm_device_synchronize", "eppm_device_mem_info", "eppm_device_pci_bus_id", "eppm_bind_thread_to_device", "eppm_release_cached_memory", "eppm_set_launcher_stream", "eppm_set_launcher_params", "eppm_launcher_status",
    "baoCudaPatchMatchMultiscalePrepare", "baoCudaCensusTransform", "baoCudaPatchMatch", "baoCudaLeftRightCheck",
    "baoCudaOutlierRemoval", "baoCudaWeightedMedianFilter", "baoCudaFillHole", "baoCudaNNF2Flow", "baoCudaBLF_C2F",
    "baoCudaBLFCostFilterRefine", "baoCudaFlowSmoothing", "eppm_flow_to_color", "eppm_compute_color",
    "eppm_pm_rng_create", "eppm_pm_rng_reset", "eppm_pm_rng_destroy", "eppm_pm_rng_block_states", "eppm_pm_gen_rand_field",
    "eppm_pm_cost_field", "eppm_pm_seg_propagate", "eppm_pm_jump_propagate", "eppm_pm_parallel_propagate", "eppm_pm_random_search", "eppm_gauss_filter_rgba", "eppm_resize_rgba",
    "eppm_resize_flow",
    "eppm_host_register", "eppm_host_unregister", "eppm_host_is_registered", "eppm_host_alloc", "eppm_host_free",
    "eppm_compute_begin_into", "eppm_batch_compute_begin_into",
    "eppm_load_ppm", "eppm_ppm_size", "eppm_save_flo", "eppm_load_flo", "eppm_flo_size", "eppm_flow_error",
    "eppm_flow_error_border", "eppm_flow_error_percentage", "eppm_flow_cutoff", "eppm_flow_to_color_host",
    "eppm_compute_bidirectional", "eppm_compute_bidirectional_device", "eppm_batch_compute_bidirectional", "eppm_set_occlusion_params",
    "eppm_fb_occlusion", "eppm_fb_occlusion_host",
    "eppm_interpolate", "eppm_interpolate_device", "eppm_batch_interpolate", "eppm_interpolate_frames", "eppm_interpolate_host",
    "eppm_track_default_params", "eppm_track_capacity", "eppm_tracker_create", "eppm_tracker_destroy", "eppm_track_step",
    "eppm_track_step_frames", "eppm_tracker_get", "eppm_tracker_get_ended", "eppm_tracker_set", "eppm_track_step_host", "eppm_track_seeds_host",
    "eppm_push_image", "eppm_push_image_device", "eppm_set_temporal", "eppm_temporal_reset", "eppm_temporal_valid", "eppm_temporal_prior_host",
    "eppm_temporal_prior",
    "eppm_batch_set_temporal", "eppm_batch_push_images", "eppm_batch_push_images_device", "eppm_batch_temporal_valid", "eppm_batch_temporal_reset",
    "eppm_temporal_prior_batch",
    "eppm_set_stop_level", "eppm_stop_level", "eppm_flow_upsample",
    "eppm_tfilter_default_params", "eppm_tfilter_create", "eppm_tfilter_create_size", "eppm_tfilter_destroy", "eppm_tfilter_reset", "eppm_tfilter_step",
    "eppm_tfilter_step_frames", "eppm_tfilter_get", "eppm_tfilter_get_device", "eppm_tfilter_get_state", "eppm_tfilter_set_state",
    "eppm_tfilter_seed_host", "eppm_tfilter_step_host",
    "eppm_stab_default_params", "eppm_stab_create", "eppm_stab_create_size", "eppm_stab_destroy", "eppm_stab_reset", "eppm_stab_step",
    "eppm_stab_step_frames", "eppm_stab_get", "eppm_stab_get_device", "eppm_stab_get_mask", "eppm_stab_get_model", "eppm_stab_get_path",
    "eppm_stab_set_path", "eppm_gmotion_fit_host", "eppm_stab_update_host", "eppm_stab_warp_host",
    "eppm_cutdet_default_params", "eppm_cutdet_create", "eppm_cutdet_create_size", "eppm_cutdet_destroy", "eppm_cutdet_step",
    "eppm_cutdet_step_frames", "eppm_cutdet_get", "eppm_cutdet_cuts", "eppm_cutdet_host",
    "eppm_mblur_default_params", "eppm_motion_blur", "eppm_motion_blur_device", "eppm_batch_motion_blur", "eppm_motion_blur_frames",
    "eppm_motion_blur_host",
    "eppm_cmap_default_params", "eppm_cmap_create", "eppm_cmap_create_size", "eppm_cmap_destroy", "eppm_cmap_reset", "eppm_cmap_step",
    "eppm_cmap_step_frames", "eppm_cmap_get_state", "eppm_cmap_set_state", "eppm_cmap_set_layer", "eppm_cmap_render", "eppm_cmap_render_device",
    "eppm_cmap_age", "eppm_cmap_step_host", "eppm_cmap_render_host",
    "eppm_objects_default_params", "eppm_objects_create", "eppm_objects_create_size", "eppm_objects_destroy", "eppm_objects_reset",
    "eppm_objects_step", "eppm_objects_step_frames", "eppm_objects_get", "eppm_objects_get_labels", "eppm_objects_get_state",
    "eppm_objects_set_state", "eppm_objects_label_host", "eppm_objects_carry_host", "eppm_objects_assign_host",
    "eppm_plate_default_params", "eppm_plate_create", "eppm_plate_create_size", "eppm_plate_destroy", "eppm_plate_reset", "eppm_plate_canvas_dims",
    "eppm_plate_step", "eppm_plate_step_frames", "eppm_plate_render", "eppm_plate_render_frames", "eppm_plate_get", "eppm_plate_get_device",
    "eppm_plate_get_mask", "eppm_plate_get_path", "eppm_plate_set_path", "eppm_plate_get_state", "eppm_plate_set_state",
    "eppm_plate_forms_host", "eppm_plate_block_host", "eppm_plate_accumulate_host", "eppm_plate_render_host",
    "eppm_defect_default_params", "eppm_defect_create", "eppm_defect_create_size", "eppm_defect_destroy", "eppm_defect_reset", "eppm_defect_step",
    "eppm_defect_step_frames", "eppm_defect_get", "eppm_defect_get_device", "eppm_defect_get_mask", "eppm_defect_get_stats",
    "eppm_defect_get_state", "eppm_defect_set_state", "eppm_defect_step_host",
    "eppm_deflicker_default_params", "eppm_deflicker_create", "eppm_deflicker_create_size", "eppm_deflicker_destroy", "eppm_deflicker_reset",
    "eppm_deflicker_step", "eppm_deflicker_step_frames", "eppm_deflicker_get", "eppm_deflicker_get_device", "eppm_deflicker_get_field",
    "eppm_deflicker_get_stats", "eppm_deflicker_get_state", "eppm_deflicker_set_state", "eppm_deflicker_step_host",
]


# what include/eppm_test.h adds, exported by libeppm_hip_test.so and libeppm_hip_tol_test.so only (the parity tests' switches and arithmetic probes)
TEST_SYMBOLS = ["eppm_test_set_option", "eppm_test_c2f_refine_batch", "eppm_test_c2f_refine_pre", "eppm_test_c2f_refine_probe", "eppm_probe_c2f_pretest", "eppm_probe_c2f_window", "eppm_probe_dispatch", "eppm_probe_fast_exp", "eppm_probe_div_const", "eppm_probe_delta_table",
                "eppm_probe_unpack_texel", "eppm_probe_pm_parity", "eppm_probe_ctx_rng_states", "eppm_test_pm_search", "eppm_probe_search_pretest", "eppm_probe_launch_log"]

_variant = None


def select_library(variant):
    """Which build this PROCESS loads: "" the product library (default), "test" libeppm_hip_test.so (the same objects plus the test
    hooks of include/eppm_test.h: tests/conftest.py selects it for the pytest process; child processes -- bench.py, the CLI, smoke() --
    are not affected), "tol" the tolerance library (libeppm_hip_tol.so, not bit-identical), "tol_test" the tolerance library's objects plus
    the same test hooks (libeppm_hip_tol_test.so: what the children of tests/test_tolerance_stages_gpu.py load; the probes of formulas the
    tolerance patch term does not have return EPPM_ERR_ARG there).  Must be called before the first lib()."""
    global _variant
    if _lib is not None and variant != _variant:
        raise EppmError("select_library: a library is loaded already")
    _variant = variant


def lib():
    """Load libeppm_hip.so.  No fallback: a missing library is an error."""
    global _lib
    if _lib is None:
        path = lib_path(_variant)
        if not os.path.exists(path):
            raise EppmError(f"{path} is missing: run eppm_amd.build() (hipcc --offload-arch=gfx950); there is no CPU fallback")
        L = C.CDLL(path)
        L.eppm_last_error.restype = C.c_char_p
        L.eppm_version.restype = C.c_char_p
        _plate_signatures(L)
        _lib = L
    return _lib


def _plate_signatures(L):
    """argument types of eppm_plate_*: size_t and pointer arguments in the middle of long lists, so they are declared, not wrapped per call"""
    P, I, Z, F = C.c_void_p, C.c_int, C.c_size_t, C.c_float
    sig = {
        "eppm_plate_default_params": [P], "eppm_plate_create": [P, P, P], "eppm_plate_create_size": [I, I, I, I, P, P], "eppm_plate_destroy": [P],
        "eppm_plate_reset": [P, I], "eppm_plate_canvas_dims": [P, P, P], "eppm_plate_step": [P, P, P],
        "eppm_plate_step_frames": [P, I, P, Z, P, P, I], "eppm_plate_render": [P, P, I, P, Z, P],
        "eppm_plate_render_frames": [P, I, P, Z, P, P, P, Z, P], "eppm_plate_get": [P, I, P, Z, P], "eppm_plate_get_device": [P, I, P, Z],
        "eppm_plate_get_mask": [P, I, P], "eppm_plate_get_path": [P, I, P], "eppm_plate_set_path": [P, I, P], "eppm_plate_get_state": [P, I, P],
        "eppm_plate_set_state": [P, I, P], "eppm_plate_forms_host": [P, P, P, P], "eppm_plate_block_host": [P, P, I, I, P],
        "eppm_plate_accumulate_host": [P, P, P, P, I, I, P], "eppm_plate_render_host": [P, P, I, P, P, I, I, P, P, P],
    }
    for name, args in sig.items():
        fn = getattr(L, name, None)
        if fn is None:              # a library built before the plate existed still loads (A/B runs); its plate calls fail at the call
            continue
        fn.argtypes = args
        fn.restype = I


def check(status, what=""):
    if status != 0:
        raise EppmError(f"{what}: status {status}: {lib().eppm_last_error().decode()}")


def check_launcher(what=""):
    check(lib().eppm_launcher_status(), what)


LAUNCH_STAGES = ("smoothing", "jbu", "refine", "search", "sweep", "sweeps_merged")


class launch_log:
    """with launch_log() as log: ...; log.entries() -- what the launchers decided inside the block (test libraries; include/eppm_test.h,
    eppm_probe_launch_log): [(stage name, w, h, pairs in the launch, form, extra)] in launch order."""

    def __enter__(self):
        check(lib().eppm_test_set_option(b"launch_log", 1), "launch_log on")
        self._kept = None
        return self

    def entries(self):
        if self._kept is not None:
            return self._kept
        n = lib().eppm_probe_launch_log(None, 0)
        buf = (C.c_int * (6 * max(n, 1)))()
        n = min(n, lib().eppm_probe_launch_log(buf, n))
        return [(LAUNCH_STAGES[buf[6 * i]],) + tuple(buf[6 * i + 1:6 * i + 6]) for i in range(n)]

    def __exit__(self, *exc):
        self._kept = self.entries()
        lib().eppm_test_set_option(b"launch_log", 0)
        return False


def probe_dispatch(stage, *args, nout=1):
    """eppm_probe_dispatch (test libraries; include/eppm_test.h): what a launcher decides for a launch of that size -- the launchers' own
    host functions, no GPU needed.  Returns a tuple of nout ints."""
    a = (C.c_int * len(args))(*[int(v) for v in args])
    out = (C.c_int * nout)()
    check(lib().eppm_probe_dispatch(stage.encode(), a, len(args), out, nout), f"eppm_probe_dispatch {stage}")
    return tuple(out)
