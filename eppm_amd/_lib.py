"""ctypes binding of the C ABI declared in include/eppm.h.  Fails loudly if the library is missing."""
import ctypes as C
import os

from .build import lib_path


class EppmError(RuntimeError):
    pass


class _Record(C.Structure):
    """a struct of integer fields that the library fills in"""

    def as_dict(self):
        return {k: int(getattr(self, k)) for k, _ in self._fields_}


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


class CDefectStats(_Record):
    _fields_ = [("hit", C.c_int), ("grown", C.c_int), ("second_chance", C.c_int), ("undecided", C.c_int)]


class CDeflickerParams(C.Structure):
    _fields_ = [("cell", C.c_int), ("iters", C.c_int), ("reject", C.c_float), ("tau", C.c_float), ("keep", C.c_float), ("n_min", C.c_int)]


class CDeflickerStats(_Record):
    _fields_ = [("used", C.c_int64), ("valid_cells", C.c_int32), ("cells", C.c_int32)]


class CDeintParams(C.Structure):
    _fields_ = [("thresh", C.c_int), ("use_occ", C.c_int)]


class CDeintStats(_Record):
    _fields_ = [("temporal", C.c_int64), ("spatial", C.c_int64)]


class CRSParams(C.Structure):
    _fields_ = [("readout", C.c_float), ("anchor", C.c_float), ("iters", C.c_int), ("axis", C.c_int)]


class CYuvFormat(_Record):
    _fields_ = [("layout", C.c_int), ("depth", C.c_int), ("msb_aligned", C.c_int), ("matrix", C.c_int), ("full_range", C.c_int), ("siting", C.c_int)]


class CObject(_Record):
    _fields_ = [("id", C.c_int32), ("age", C.c_int32), ("area", C.c_int32), ("x0", C.c_int32), ("y0", C.c_int32), ("x1", C.c_int32),
                ("y1", C.c_int32), ("n_flow", C.c_int32), ("sum_x", C.c_int64), ("sum_y", C.c_int64), ("sum_qu", C.c_int64), ("sum_qv", C.c_int64)]


class CObjectsCounts(_Record):
    _fields_ = [("n", C.c_int32), ("n_found", C.c_int32), ("n_components", C.c_int32), ("next_id", C.c_int32)]


class CTrackCounts(_Record):
    _fields_ = [("live", C.c_int), ("ended", C.c_int), ("seeded", C.c_int), ("dropped", C.c_int), ("frame", C.c_int), ("next_id", C.c_int)]


_lib = None

_CODES = {"P": C.c_void_p, "S": C.c_char_p, "I": C.c_int, "Z": C.c_size_t, "F": C.c_float, "B": C.c_bool, "V": None}


def _signatures(text):
    """"name:ARGS" or "name:R>ARGS" per function, one letter per argument: P any pointer, S const char*, I int / int32_t, Z size_t, F float,
    B bool; R the return type, I where it is left out, S const char*, V void -> {name: (restype, argtypes)}"""
    out = {}
    for item in text.split():
        name, _, sig = item.partition(":")
        ret, _, args = sig.rpartition(">")
        out[name] = (_CODES[ret or "I"], [_CODES[c] for c in args])
    return out


# THE BINDING: every function include/eppm.h declares, in the header's order (tests/test_abi_cpu.py checks the table against the prototypes
# and that the library exports every name).  lib() declares these types, so a call passes addresses, sizes and floats as plain numbers.
_ABI = _signatures("""
eppm_default_params:P eppm_create:PIIIP eppm_destroy:P eppm_set_stream:PP eppm_set_images:PPPZ eppm_host_register:PZ eppm_host_unregister:P
eppm_host_is_registered:PZ eppm_host_alloc:PZ eppm_host_free:P eppm_set_images_device:PPPZ eppm_create_batch:PIIIPI eppm_batch_size:P
eppm_batch_set_images:PIPPZ eppm_batch_set_images_device:PIPPZ eppm_batch_compute:PPP eppm_batch_compute_device:PP eppm_batch_compute_end:PPP
eppm_batch_compute_begin_into:PPP eppm_batch_get_plane:PISIPZ eppm_compute:PPP eppm_compute_begin:P eppm_compute_end:PPP eppm_compute_begin_into:PPP
eppm_compute_color:PPZFF eppm_compute_device:PP eppm_synchronize:P eppm_num_levels:P eppm_level_dims:PIPP eppm_get_plane:PSIPZ
eppm_compute_bidirectional:PPPPPPP eppm_compute_bidirectional_device:PPPPP eppm_batch_compute_bidirectional:PPPPPPP eppm_set_occlusion_params:PFF
eppm_set_stop_level:PI eppm_stop_level:P eppm_fb_occlusion:PPPIIFF eppm_interpolate:PIPPZ eppm_interpolate_device:PIPPZ eppm_batch_interpolate:PIPPZ
eppm_interpolate_frames:PZPPZPPPIIF eppm_interpolate_host:PPPPPPPIIF eppm_mblur_default_params:P eppm_motion_blur:PPIPZ eppm_motion_blur_device:PPIPZ
eppm_batch_motion_blur:PPIPZ eppm_motion_blur_frames:PZPZPIIP eppm_motion_blur_host:PPPPIIP eppm_track_default_params:P eppm_track_capacity:PII
eppm_tracker_create:PPP eppm_tracker_destroy:P eppm_track_step:PPI eppm_track_step_frames:PPPZPPII eppm_tracker_get:PIPPPP
eppm_tracker_get_ended:PIPPPPP eppm_tracker_set:PIPPPII eppm_track_step_host:PPPPPPPIIIPPPIIPPPPPPPP eppm_track_seeds_host:PPIIIPP eppm_push_image:PPZ
eppm_push_image_device:PPZ eppm_set_temporal:PI eppm_temporal_reset:P eppm_temporal_valid:P eppm_temporal_prior_host:PPIII eppm_temporal_prior:PPIII
eppm_batch_set_temporal:PI eppm_batch_push_images:PIPZP eppm_batch_push_images_device:PIPZP eppm_batch_temporal_valid:PI eppm_batch_temporal_reset:PI
eppm_temporal_prior_batch:PPIIIIP eppm_tfilter_default_params:P eppm_tfilter_create:PPP eppm_tfilter_create_size:IIIIPP eppm_tfilter_destroy:P
eppm_tfilter_reset:PI eppm_tfilter_step:PPP eppm_tfilter_step_frames:PIPPZPPI eppm_tfilter_get:PIPZ eppm_tfilter_get_device:PIPZ
eppm_tfilter_get_state:PIP eppm_tfilter_set_state:PIP eppm_tfilter_seed_host:PPII eppm_tfilter_step_host:PPPPPPPPIII eppm_deflicker_default_params:P
eppm_deflicker_create:PPP eppm_deflicker_create_size:IIIIPP eppm_deflicker_destroy:P eppm_deflicker_reset:PI eppm_deflicker_step:PPP
eppm_deflicker_step_frames:PIPPZPPI eppm_deflicker_get:PIPZ eppm_deflicker_get_device:PIPZ eppm_deflicker_get_field:PIPP eppm_deflicker_get_stats:PIP
eppm_deflicker_get_state:PIPP eppm_deflicker_set_state:PIPI eppm_deflicker_step_host:PPPPPPPPPPIII eppm_defect_default_params:P eppm_defect_create:PPP
eppm_defect_create_size:IIIIPP eppm_defect_destroy:P eppm_defect_reset:PI eppm_defect_step:PPP eppm_defect_step_frames:PIPPZPPI eppm_defect_get:PIPZ
eppm_defect_get_device:PIPZ eppm_defect_get_mask:PIP eppm_defect_get_stats:PIP eppm_defect_get_state:PIPPP eppm_defect_set_state:PIPPI
eppm_defect_step_host:PPPPPPPPPPPII eppm_stab_default_params:P eppm_stab_create:PPP eppm_stab_create_size:IIIIPP eppm_stab_destroy:P
eppm_stab_reset:PI eppm_stab_step:PPP eppm_stab_step_frames:PIPZPPI eppm_stab_get:PIPZ eppm_stab_get_device:PIPZ eppm_stab_get_mask:PIP
eppm_stab_get_model:PIP eppm_stab_get_path:PIPPP eppm_stab_set_path:PIP eppm_gmotion_fit_host:PPPPIIPP eppm_stab_update_host:PPPPIP
eppm_stab_warp_host:PPIIP eppm_cutdet_default_params:P eppm_cutdet_create:PPP eppm_cutdet_create_size:IIIIPP eppm_cutdet_destroy:P eppm_cutdet_step:PP
eppm_cutdet_step_frames:PIPPZPPP eppm_cutdet_get:PIP eppm_cutdet_cuts:PIP eppm_cutdet_host:PPPPPPPIIP eppm_cmap_default_params:P eppm_cmap_create:PPP
eppm_cmap_create_size:IIIIPP eppm_cmap_destroy:P eppm_cmap_reset:PI eppm_cmap_step:PPP eppm_cmap_step_frames:PIPPZPPI eppm_cmap_get_state:PIP
eppm_cmap_set_state:PIPPZ eppm_cmap_set_layer:PIPZ eppm_cmap_render:PIPZ eppm_cmap_render_device:PIPZ eppm_cmap_age:PI eppm_cmap_step_host:PPPPPPPPIII
eppm_cmap_render_host:PPPPPII eppm_objects_default_params:P eppm_objects_create:PPP eppm_objects_create_size:IIIIPP eppm_objects_destroy:P
eppm_objects_reset:PI eppm_objects_step:PPP eppm_objects_step_frames:PIPPPPI eppm_objects_get:PIIPP eppm_objects_get_labels:PIP
eppm_objects_get_state:PIPPPP eppm_objects_set_state:PIPPPI eppm_objects_label_host:PPPPIIPPP eppm_objects_carry_host:PPPPIIP
eppm_objects_assign_host:PPPIIIPPPP eppm_plate_default_params:P eppm_plate_create:PPP eppm_plate_create_size:IIIIPP eppm_plate_destroy:P
eppm_plate_reset:PI eppm_plate_canvas_dims:PPP eppm_plate_step:PPP eppm_plate_step_frames:PIPZPPI eppm_plate_render:PPIPZP
eppm_plate_render_frames:PIPZPPPZP eppm_plate_get:PIPZP eppm_plate_get_device:PIPZ eppm_plate_get_mask:PIP eppm_plate_get_path:PIP
eppm_plate_set_path:PIP eppm_plate_get_state:PIP eppm_plate_set_state:PIP eppm_plate_forms_host:PPPP eppm_plate_block_host:PPIIP
eppm_plate_accumulate_host:PPPPIIP eppm_plate_render_host:PPIPPIIPPP eppm_stage_times:PPPI eppm_clear_stage_times:P eppm_enable_stage_timing:PI
eppm_last_error:S> eppm_version:S> eppm_device_count:P eppm_set_device:I eppm_malloc_device:PZ eppm_malloc_pitched:PPZZ eppm_free_device:P
eppm_memcpy_h2d:PPZ eppm_memcpy_d2h:PPZ eppm_memcpy2d_h2d:PZPZZZ eppm_memcpy2d_d2h:PZPZZZ eppm_memset_device:PIZ eppm_device_synchronize:
eppm_device_pci_bus_id:IPZ eppm_bind_thread_to_device:IPP eppm_device_mem_info:PP eppm_release_cached_memory: eppm_set_launcher_stream:P
eppm_set_launcher_params:P eppm_launcher_status: baoCudaPatchMatchMultiscalePrepare:V>PPPPPPPPPPIPPII baoCudaCensusTransform:V>PPPPIIZZ
baoCudaPatchMatch:V>PPPPPPIIZZZZ baoCudaLeftRightCheck:V>PPPPIIZZ baoCudaOutlierRemoval:V>PPIIZZ baoCudaWeightedMedianFilter:V>PPPIIZZZIB
baoCudaFillHole:V>PPPIIZZZ baoCudaNNF2Flow:V>PPIIZZ baoCudaBLF_C2F:V>PPPPPPPPPPPI baoCudaBLFCostFilterRefine:V>PPPPPIIZZ baoCudaFlowSmoothing:V>PPIIZZ
eppm_flow_to_color:PPIIFF eppm_pm_rng_create:PIIP eppm_pm_rng_reset:P eppm_pm_rng_destroy:P eppm_pm_rng_block_states:PPZ eppm_pm_gen_rand_field:PPIIZ
eppm_pm_cost_field:PPPPPPIIZZZZ eppm_pm_seg_propagate:PPPPPPIIZZZZI eppm_pm_jump_propagate:PPPPPPIIZZZZ eppm_pm_parallel_propagate:PPPPPPIIZZZZ
eppm_pm_random_search:PPPPPPPIIZZZZ eppm_gauss_filter_rgba:PPZIIFI eppm_resize_rgba:PZIIPZIIF eppm_resize_flow:PIIPIIF eppm_flow_upsample:PIIPIIPZ
eppm_load_ppm:SPIIP eppm_ppm_size:SPP eppm_save_flo:SPPII eppm_load_flo:SPPII eppm_flo_size:SPP eppm_flow_error:PPPPIIPP
eppm_flow_error_border:PPPPIIIPP eppm_flow_error_percentage:PPPPIIIPP eppm_flow_cutoff:PPPPIIII eppm_fb_occlusion_host:PPPPPIIFF
eppm_flow_to_color_host:PPPII""")

# what include/eppm_test.h adds, exported by libeppm_hip_test.so and libeppm_hip_tol_test.so only (the parity tests' switches and arithmetic probes)
_TEST_ABI = _signatures("""
eppm_test_set_option:SI eppm_probe_c2f_window:IPP eppm_test_c2f_refine_batch:PPPPPIII eppm_test_c2f_refine_pre:PPPPPIIIIP
eppm_test_c2f_refine_probe:PPPPPIIIP eppm_probe_c2f_pretest:IPP eppm_test_pm_search:PPPPPIIIIIPPP eppm_probe_search_pretest:IIIIIIPP
eppm_probe_dispatch:SPIPI eppm_probe_launch_log:PI eppm_probe_fast_exp:PPI eppm_probe_div_const:PPII eppm_probe_delta_table:PPII
eppm_probe_unpack_texel:PPI eppm_probe_pm_parity:PPPP eppm_probe_ctx_rng_states:PPZ""")

# what include/eppm_yuv.h declares, in its order (tests/test_yuv_cpu.py checks it as tests/test_abi_cpu.py checks the tables above): exported
# by all four libraries, applied by lib(), and kept out of SIGNATURES / SYMBOLS, which mirror include/eppm.h and eppm_test.h alone
_YUV_ABI = _signatures("""
eppm_yuv_default_format:P eppm_yuv_plane_dims:PIIIPP eppm_yuv_to_rgba:PPPPZIIP eppm_yuv_from_rgba:PPZPPIIP eppm_yuv_to_rgb_host:PPPPZII
eppm_yuv_from_rgb_host:PPZPPII eppm_yuv_set_images:PPPPP eppm_yuv_set_images_device:PPPPP eppm_yuv_push_image:PPPP eppm_yuv_push_image_device:PPPP
eppm_yuv_batch_set_images:PPIPPP eppm_yuv_batch_set_images_device:PPIPPP eppm_yuv_batch_push_images:PPIPPP
eppm_yuv_batch_push_images_device:PPIPPP eppm_y4m_open_read:PSPPPPP eppm_y4m_read_frame:PPPP eppm_y4m_open_write:PSIIPII eppm_y4m_write_frame:PPP
eppm_y4m_close:P""")

# what include/eppm_deint.h declares, in its order (tests/test_deint_cpu.py checks it the same way): exported by all four libraries, applied by
# lib() next to _YUV_ABI, and kept out of SIGNATURES / SYMBOLS
_DEINT_ABI = _signatures("""
eppm_deint_default_params:P eppm_deint_create:PPP eppm_deint_create_size:IIIIPP eppm_deint_destroy:P eppm_deint_reset:PI eppm_deint_step:PPPP
eppm_deint_step_frames:PIPPZPPII eppm_deint_get:PIPZ eppm_deint_get_device:PIPZ eppm_deint_get_mask:PIP eppm_deint_get_stats:PIP
eppm_deint_get_state:PIPP eppm_deint_set_state:PIPI eppm_deint_step_host:PPPPPPPPPIIII eppm_deint_bob:PZPZIII eppm_deint_bob_stream:PZPZIIIP
eppm_deint_bob_host:PPIII eppm_deint_y4m_open_read:PSPPPPPP""")

# what include/eppm_rshutter.h declares, in its order (tests/test_rshutter_cpu.py checks it the same way): exported by all four libraries,
# applied by lib() next to _YUV_ABI and _DEINT_ABI, and kept out of SIGNATURES / SYMBOLS
_RS_ABI = _signatures("""
eppm_rs_default_params:P eppm_rolling_shutter:PPIPZ eppm_rolling_shutter_device:PPIPZ eppm_batch_rolling_shutter:PPIPZ
eppm_rolling_shutter_frames:PZPZPIIIP eppm_rolling_shutter_host:PPPPIIIP""")

SIGNATURES = {**_ABI, **_TEST_ABI}
SYMBOLS, TEST_SYMBOLS = list(_ABI), list(_TEST_ABI)

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
        for name, (res, args) in {**SIGNATURES, **_YUV_ABI, **_DEINT_ABI, **_RS_ABI}.items():
            fn = getattr(L, name, None)
            if fn is None:      # a test hook in a product library, or a library built before the function existed (A/B runs): fails at the call
                continue
            fn.restype, fn.argtypes = res, args
        _lib = L
    return _lib


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
