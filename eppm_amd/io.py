"""PPM / .flo I/O and EPE through the C ABI (reference: bao_basic.cpp:137-218, flowIO.cpp:48-163,
bao_flow_tools.cpp:64-111)."""
import ctypes as C

import numpy as np

from ._lib import check, lib


def _p(a):
    """the address of an array, NULL for None; the caller keeps the array alive over the call"""
    return None if a is None else a.ctypes.data


def ppm_size(path):
    h, w = C.c_int(), C.c_int()
    check(lib().eppm_ppm_size(path.encode(), C.byref(h), C.byref(w)), f"eppm_ppm_size({path})")
    return h.value, w.value


def load_ppm(path):
    h, w = ppm_size(path)
    img = np.zeros((h, w, 3), np.uint8)
    nc = C.c_int()
    check(lib().eppm_load_ppm(path.encode(), img.ctypes.data, h, w, C.byref(nc)), f"eppm_load_ppm({path})")
    return img if nc.value == 3 else img.reshape(-1)[:h * w].reshape(h, w)


def save_flo(path, u, v):
    u = np.ascontiguousarray(u, np.float32)
    v = np.ascontiguousarray(v, np.float32)
    h, w = u.shape
    check(lib().eppm_save_flo(path.encode(), u.ctypes.data, v.ctypes.data, h, w), "eppm_save_flo")


def load_flo(path):
    h, w = C.c_int(), C.c_int()
    check(lib().eppm_flo_size(path.encode(), C.byref(h), C.byref(w)), f"eppm_flo_size({path})")
    u = np.empty((h.value, w.value), np.float32)
    v = np.empty((h.value, w.value), np.float32)
    check(lib().eppm_load_flo(path.encode(), u.ctypes.data, v.ctypes.data, h.value, w.value), "eppm_load_flo")
    return u, v


def flow_error(u, v, gu, gv, border=0):
    """(EPE, AAE) with the reference's validity rule (bao_calc_flow_error); border: pixels left out on every side."""
    arrs = [np.ascontiguousarray(a, np.float32) for a in (u, v, gu, gv)]
    h, w = arrs[0].shape
    epe, aae = C.c_float(), C.c_float()
    check(lib().eppm_flow_error_border(*[a.ctypes.data for a in arrs], h, w, int(border), C.byref(epe), C.byref(aae)), "eppm_flow_error_border")
    return epe.value, aae.value


def flow_error_percentage(u, v, gu, gv, error_thresh, want_map=False):
    """Fraction of the pixels with known ground truth whose end-point error exceeds error_thresh (bao_calc_flow_error_percentage);
    with want_map also the uint8 map (255 where it does)."""
    arrs = [np.ascontiguousarray(a, np.float32) for a in (u, v, gu, gv)]
    h, w = arrs[0].shape
    emap = np.empty((h, w), np.uint8) if want_map else None
    frac = C.c_float()
    check(lib().eppm_flow_error_percentage(*[a.ctypes.data for a in arrs], h, w, int(error_thresh),
                                           emap.ctypes.data if want_map else None, C.byref(frac)), "eppm_flow_error_percentage")
    return (frac.value, emap) if want_map else frac.value


def flow_cutoff(u, v, cutoff, cut_invalid=False):
    """Both components clamped to [-|cutoff|, |cutoff|]; unknown vectors pass through unless cut_invalid (bao_flow_cutoff)."""
    u = np.ascontiguousarray(u, np.float32)
    v = np.ascontiguousarray(v, np.float32)
    uo, vo = np.empty_like(u), np.empty_like(v)
    h, w = u.shape
    check(lib().eppm_flow_cutoff(uo.ctypes.data, vo.ctypes.data, u.ctypes.data, v.ctypes.data, h, w, int(cutoff), int(bool(cut_invalid))), "eppm_flow_cutoff")
    return uo, vo


def flow_to_color(u, v):
    """(h, w, 3) uint8 R,G,B colour coding scaled by the field's largest known radius (bao_convert_flow_to_colorshow, host)."""
    u = np.ascontiguousarray(u, np.float32)
    v = np.ascontiguousarray(v, np.float32)
    h, w = u.shape
    rgb = np.empty((h, w, 3), np.uint8)
    check(lib().eppm_flow_to_color_host(rgb.ctypes.data, u.ctypes.data, v.ctypes.data, h, w),
          "eppm_flow_to_color_host")
    return rgb


def fb_occlusion(u, v, bu, bv, alpha=0.01, beta=0.5):
    """(h, w) uint8 forward-backward occlusion mask of the pixels of (u, v)'s image against the other direction's flow (bu, bv):
    0 consistent, 1 inconsistent, 2 leaves the frame, 3 unknown vector (eppm_fb_occlusion_host; the bidirectional call's kernel)."""
    arrs = [np.ascontiguousarray(a, np.float32) for a in (u, v, bu, bv)]
    h, w = arrs[0].shape
    if any(a.shape != (h, w) for a in arrs):
        raise ValueError("fb_occlusion: the four planes must have one shape")
    occ = np.empty((h, w), np.uint8)
    check(lib().eppm_fb_occlusion_host(occ.ctypes.data, *[a.ctypes.data for a in arrs], h, w, alpha, beta), "eppm_fb_occlusion_host")
    return occ


def temporal_prior(prev, backward=False):
    """(h, w) short2 prior of a streaming context's next pair from a displacement snapshot of the previous one (eppm_temporal_prior_host,
    DESIGN.md section 13): prev holds displacements (a component <= -10000: unknown), the result absolute targets ((-10000, -10000): no prior)."""
    from .api import short2
    prev = np.ascontiguousarray(prev, short2)
    h, w = prev.shape
    out = np.empty((h, w), short2)
    check(lib().eppm_temporal_prior_host(out.ctypes.data, prev.ctypes.data, h, w, int(bool(backward))),
          "eppm_temporal_prior_host")
    return out


def interpolate(img1, img2, u, v, occ1, occ2, t):
    """(h, w, 3) uint8 frame at time t between img1 (t = 0) and img2 (t = 1) from the forward flow (u, v) and the occlusion masks of
    both images (eppm_interpolate_host; byte-identical to the kernels)."""
    a = np.ascontiguousarray(img1, np.uint8)
    b = np.ascontiguousarray(img2, np.uint8)
    u = np.ascontiguousarray(u, np.float32)
    v = np.ascontiguousarray(v, np.float32)
    o1 = np.ascontiguousarray(occ1, np.uint8)
    o2 = np.ascontiguousarray(occ2, np.uint8)
    h, w = u.shape
    if a.shape != (h, w, 3) or b.shape != (h, w, 3) or v.shape != (h, w) or o1.shape != (h, w) or o2.shape != (h, w):
        raise ValueError("interpolate: images (h, w, 3), flow and masks (h, w)")
    out = np.empty((h, w, 3), np.uint8)
    check(lib().eppm_interpolate_host(out.ctypes.data, *[x.ctypes.data for x in (a, b, u, v, o1, o2)], h, w, t), "eppm_interpolate_host")
    return out


def motion_blur_host(img, u, v, shutter=0.5, max_radius=16, taps=8):
    """(h, w, 3) uint8 frame: img as a camera with an open shutter would have recorded it, blurred along its flow (u, v)
    (eppm_motion_blur_host; byte-identical to the kernels).  shutter: the open fraction of the frame interval,
    max_radius: the longest half-vector in pixels, taps: taps to each side of a pixel."""
    from .api import MBlurParams
    a = np.ascontiguousarray(img, np.uint8)
    u = np.ascontiguousarray(u, np.float32)
    v = np.ascontiguousarray(v, np.float32)
    if u.ndim != 2 or a.shape != (*u.shape, 3) or v.shape != u.shape:
        raise ValueError("motion_blur_host: image (h, w, 3), flow (h, w)")
    h, w = u.shape
    p = MBlurParams(shutter=shutter, max_radius=max_radius, taps=taps)
    out = np.empty((h, w, 3), np.uint8)
    check(lib().eppm_motion_blur_host(out.ctypes.data, *[x.ctypes.data for x in (a, u, v)], h, w, C.byref(p)),
          "eppm_motion_blur_host")
    return out


def rolling_shutter_host(img, u, v, frame=0, readout=0.5, anchor=0.5, iters=3, axis=0):
    """(h, w, 3) uint8 frame: img as a global shutter would have recorded it, corrected along its flow (u, v) (eppm_rolling_shutter_host,
    DESIGN.md section 27; byte-identical to the kernels).  frame=0: the flow points to the next frame, 1: to the previous one; readout: the
    share of the frame interval the sensor takes to read a frame, anchor: the position along the axis whose sampling time is the frame's,
    iters: fixed-point steps, axis: 0 rows are read one after another, 1 columns."""
    from .api import RSParams
    a = np.ascontiguousarray(img, np.uint8)
    u = np.ascontiguousarray(u, np.float32)
    v = np.ascontiguousarray(v, np.float32)
    if u.ndim != 2 or a.shape != (*u.shape, 3) or v.shape != u.shape:
        raise ValueError("rolling_shutter_host: image (h, w, 3), flow (h, w)")
    h, w = u.shape
    p = RSParams(readout=readout, anchor=anchor, iters=iters, axis=axis)
    out = np.empty((h, w, 3), np.uint8)
    check(lib().eppm_rolling_shutter_host(out.ctypes.data, *[x.ctypes.data for x in (a, u, v)], h, w, int(frame), C.byref(p)),
          "eppm_rolling_shutter_host")
    return out


def _track_params(params, kw):
    from .api import TrackParams
    return TrackParams(params, **kw)


def track_seeds(img, params=None, **track_params):
    """(n, 2) float32: the seeds of the textured cells of an (h, w, 3) uint8 image in cell order (eppm_track_seeds_host, DESIGN.md
    section 12)."""
    p = _track_params(params, track_params)
    a = np.ascontiguousarray(img, np.uint8)
    h, w, _ = a.shape
    n = C.c_int()
    check(lib().eppm_track_seeds_host(C.byref(p), a.ctypes.data, h, w, 0, None, C.byref(n)), "eppm_track_seeds_host")
    xy = np.empty((n.value, 2), np.float32)
    check(lib().eppm_track_seeds_host(C.byref(p), a.ctypes.data, h, w, n.value, xy.ctypes.data, C.byref(n)),
          "eppm_track_seeds_host")
    return xy


def track_step_host(img1, img2, u, v, bu, bv, ids=(), starts=(), xy=(), next_id=0, frame=0, params=None, **track_params):
    """One track step on the host (eppm_track_step_host; byte-identical to the kernels).  img1 / img2: (h, w, 3)
    uint8 frames k and k+1; (u, v) forward, (bu, bv) backward flow; the state: tracks (ids, starts, xy (n, 2) in frame k), next_id, frame.
    Returns a dict: ids, starts, xy (the live tracks in frame k+1), ended_ids, ended_starts, ended_xy, reasons, and the counts."""
    from ._lib import CTrackCounts
    p = _track_params(params, track_params)
    a = np.ascontiguousarray(img1, np.uint8)
    b = np.ascontiguousarray(img2, np.uint8)
    fl = [np.ascontiguousarray(x, np.float32) for x in (u, v, bu, bv)]
    h, w = fl[0].shape
    if a.shape != (h, w, 3) or b.shape != (h, w, 3) or any(x.shape != (h, w) for x in fl):
        raise ValueError("track_step_host: images (h, w, 3), flows (h, w)")
    ids = np.ascontiguousarray(ids, np.int32).ravel()
    starts = np.ascontiguousarray(starts, np.int32).ravel()
    xy = np.ascontiguousarray(xy, np.float32).reshape(-1, 2)
    cap = lib().eppm_track_capacity(C.byref(p), h, w)
    if cap < 0:
        check(1, "eppm_track_capacity")
    o_ids, o_st, e_ids, e_st, why = (np.empty(cap, np.int32) for _ in range(5))
    o_xy, e_xy = np.empty((cap, 2), np.float32), np.empty((cap, 2), np.float32)
    cnt = CTrackCounts()
    check(lib().eppm_track_step_host(C.byref(p), _p(a), _p(b), *[_p(x) for x in fl], h, w, len(ids), _p(ids), _p(starts), _p(xy),
                                     int(next_id), int(frame), _p(o_ids), _p(o_st), _p(o_xy), _p(e_ids), _p(e_st), _p(e_xy), _p(why),
                                     C.byref(cnt)), "eppm_track_step_host")
    c = cnt.as_dict()
    n, m = c["live"], c["ended"]
    return dict(ids=o_ids[:n].copy(), starts=o_st[:n].copy(), xy=o_xy[:n].copy(), ended_ids=e_ids[:m].copy(), ended_starts=e_st[:m].copy(),
                ended_xy=e_xy[:m].copy(), reasons=why[:m].copy(), **c)


def _tfilter_params(thresh, n_max):
    from ._lib import CTFilterParams
    return CTFilterParams(float(thresh), int(n_max))


def tfilter_seed_host(img):
    """(h, w, 4) float32 {R, G, B, 1}: the temporal filter's state of a clip's first frame (eppm_tfilter_seed_host)."""
    a = np.ascontiguousarray(img, np.uint8)
    if a.ndim != 3 or a.shape[2] != 3:
        raise ValueError("tfilter_seed_host: the image must be (h, w, 3)")
    h, w, _ = a.shape
    acc = np.empty((h, w, 4), np.float32)
    check(lib().eppm_tfilter_seed_host(acc.ctypes.data, a.ctypes.data, h, w), "eppm_tfilter_seed_host")
    return acc


def tfilter_step_host(acc, img2, bu, bv, occ2, thresh=40.0, n_max=8, cut=False):
    """One step of the temporal filter on the host (eppm_tfilter_step_host; bit-identical to the kernel).  acc: the
    (h, w, 4) float32 state of image 1; img2: the new (h, w, 3) uint8 frame; (bu, bv): the backward flow image 2 -> image 1; occ2: the
    occlusion mask of image 2's pixels; cut: img2 starts another clip.  Returns (new state, filtered (h, w, 3) uint8 frame)."""
    p = _tfilter_params(thresh, n_max)
    acc = np.ascontiguousarray(acc, np.float32)
    b = np.ascontiguousarray(img2, np.uint8)
    bu = np.ascontiguousarray(bu, np.float32)
    bv = np.ascontiguousarray(bv, np.float32)
    o = np.ascontiguousarray(occ2, np.uint8)
    h, w = bu.shape
    if acc.shape != (h, w, 4) or b.shape != (h, w, 3) or bv.shape != (h, w) or o.shape != (h, w):
        raise ValueError("tfilter_step_host: state (h, w, 4), image (h, w, 3), flow and mask (h, w)")
    out, rgb = np.empty((h, w, 4), np.float32), np.empty((h, w, 3), np.uint8)
    check(lib().eppm_tfilter_step_host(C.byref(p), out.ctypes.data, rgb.ctypes.data,
                                       *[x.ctypes.data for x in (acc, b, bu, bv, o)], h, w, int(bool(cut))), "eppm_tfilter_step_host")
    return out, rgb


def defect_step_host(prev, cur, nxt, bu=None, bv=None, fu=None, fv=None, detect=60.0, agree=30.0, radius=3, grow=1):
    """One step of film-defect removal on the host (eppm_defect_step_host; bit-identical to the kernels).  cur: the
    (h, w, 3) uint8 frame to repair; prev / nxt: its neighbours (None: the passing step); (bu, bv) / (fu, fv): the (h, w) float32 vectors
    from cur into prev / into nxt.  Returns (rgb (h, w, 3) uint8, mask (h, w) uint8: 0 untouched, 1 hit, 2 grown, stats dict)."""
    from ._lib import CDefectParams, CDefectStats
    p = CDefectParams(float(detect), float(agree), int(radius), int(grow))
    c = np.ascontiguousarray(cur, np.uint8)
    if c.ndim != 3 or c.shape[2] != 3:
        raise ValueError("defect_step_host: the frame must be (h, w, 3)")
    h, w, _ = c.shape
    imgs = [None if a is None else np.ascontiguousarray(a, np.uint8) for a in (prev, nxt)]
    flows = [None if a is None else np.ascontiguousarray(a, np.float32) for a in (bu, bv, fu, fv)]
    if any(a is not None and a.shape != c.shape for a in imgs) or any(a is not None and a.shape != (h, w) for a in flows):
        raise ValueError("defect_step_host: frames (h, w, 3), flow planes (h, w)")
    out, mask, st = np.empty_like(c), np.empty((h, w), np.uint8), CDefectStats()
    check(lib().eppm_defect_step_host(C.byref(p), _p(out), _p(mask), C.byref(st), _p(imgs[0]), _p(c), _p(imgs[1]), *[_p(a) for a in flows],
                                      h, w), "eppm_defect_step_host")
    return out, mask, st.as_dict()


def deflicker_step_host(ref, cur, bu, bv, occ2, cell=32, iters=2, reject=60.0, tau=12.0, keep=1.0, n_min=32, cut=False):
    """One step of flicker removal on the host (eppm_deflicker_step_host; bit-identical to the kernels).  ref: the
    (h, w, 3) uint8 reference (the previous output; image 1 for an empty slot); cur: image 2; (bu, bv): the backward flow image 2 -> image
    1; occ2: the occlusion mask of image 2's pixels; cut: cur starts another clip.  Returns (rgb (h, w, 3) uint8, field (cells_y, cells_x,
    6) float32, valid (cells_y, cells_x) uint8, stats dict)."""
    from ._lib import CDeflickerParams, CDeflickerStats
    p = CDeflickerParams(int(cell), int(iters), float(reject), float(tau), float(keep), int(n_min))
    r, c = np.ascontiguousarray(ref, np.uint8), np.ascontiguousarray(cur, np.uint8)
    bu, bv, o = np.ascontiguousarray(bu, np.float32), np.ascontiguousarray(bv, np.float32), np.ascontiguousarray(occ2, np.uint8)
    if c.ndim != 3 or c.shape[2] != 3:
        raise ValueError("deflicker_step_host: the frame must be (h, w, 3)")
    h, w, _ = c.shape
    if r.shape != c.shape or bu.shape != (h, w) or bv.shape != (h, w) or o.shape != (h, w):
        raise ValueError("deflicker_step_host: frames (h, w, 3), flow and mask (h, w)")
    cy, cx = -(-h // max(int(cell), 1)), -(-w // max(int(cell), 1))
    out, field, valid, st = np.empty_like(c), np.empty((cy, cx, 6), np.float32), np.empty((cy, cx), np.uint8), CDeflickerStats()
    check(lib().eppm_deflicker_step_host(C.byref(p), out.ctypes.data, field.ctypes.data,
                                         valid.ctypes.data, C.byref(st), *[x.ctypes.data for x in (r, c, bu, bv, o)],
                                         h, w, int(bool(cut))), "eppm_deflicker_step_host")
    return out, field, valid, st.as_dict()


def deint_step_host(ref, cur, bu, bv, occ2, parity, thresh=24, use_occ=1, cut=False):
    """One deinterlacer step on the host (eppm_deint_step_host; byte-identical to the kernel).  ref: the (h, w, 3)
    uint8 reference (the previous output; image 1 for an empty slot); cur: image 2, a field frame whose rows of `parity` are real (its
    other rows are not read); (bu, bv): the backward flow image 2 -> image 1; occ2: the occlusion mask of image 2's pixels; cut: cur
    starts another clip.  Returns (rgb (h, w, 3) uint8, mask (h, w) uint8: 0 real row / 1 temporal / 2 spatial, stats dict)."""
    from ._lib import CDeintParams, CDeintStats
    p = CDeintParams(int(thresh), int(use_occ))
    r, c = np.ascontiguousarray(ref, np.uint8), np.ascontiguousarray(cur, np.uint8)
    bu, bv, o = np.ascontiguousarray(bu, np.float32), np.ascontiguousarray(bv, np.float32), np.ascontiguousarray(occ2, np.uint8)
    if c.ndim != 3 or c.shape[2] != 3:
        raise ValueError("deint_step_host: the frame must be (h, w, 3)")
    h, w, _ = c.shape
    if r.shape != c.shape or bu.shape != (h, w) or bv.shape != (h, w) or o.shape != (h, w):
        raise ValueError("deint_step_host: frames (h, w, 3), flow and mask (h, w)")
    out, mask, st = np.empty_like(c), np.empty((h, w), np.uint8), CDeintStats()
    check(lib().eppm_deint_step_host(C.byref(p), out.ctypes.data, mask.ctypes.data, C.byref(st), *[x.ctypes.data for x in (r, c, bu, bv, o)],
                                     h, w, int(parity), int(bool(cut))), "eppm_deint_step_host")
    return out, mask, st.as_dict()


def deint_bob_host(field, h, parity):
    """The full (h, w, 3) uint8 frame of a field picture ((h - parity + 1) // 2, w, 3) of parity 0 (top) or 1 (eppm_deint_bob_host): row
    2i + parity is field row i, every other row the line average of its neighbours."""
    f = np.ascontiguousarray(field, np.uint8)
    h, parity = int(h), int(parity)
    if f.ndim != 3 or f.shape[2] != 3 or parity not in (0, 1) or f.shape[0] != (h - parity + 1) // 2:
        raise ValueError("deint_bob_host: a field of ((h - parity + 1) // 2, w, 3) uint8 and parity 0 or 1")
    out = np.empty((h, f.shape[1], 3), np.uint8)
    check(lib().eppm_deint_bob_host(out.ctypes.data, f.ctypes.data, h, f.shape[1], parity), "eppm_deint_bob_host")
    return out


def cmap_seed(h, w):
    """(h, w, 2) float32: the seed of a correspondence map, map(x, y) = (x, y)."""
    m = np.empty((int(h), int(w), 2), np.float32)
    m[..., 0] = np.arange(int(w), dtype=np.float32)[None, :]
    m[..., 1] = np.arange(int(h), dtype=np.float32)[:, None]
    return m


def cmap_step_host(cmap, anchor, img2, bu, bv, occ2, thresh=90.0, tear=2.0, use_occ=1, cut=False):
    """One step of a correspondence map on the host (eppm_cmap_step_host; bit-identical to the kernel).  cmap: the
    (h, w, 2) float32 map of image 1, or None for the seed (what an empty slot reads); anchor: the (h, w, 3) uint8 anchor frame (image 1
    for an empty slot); img2: the new frame; (bu, bv): the backward flow image 2 -> image 1; occ2: the occlusion mask of image 2's pixels;
    cut: img2 starts another clip (the result is the seed, and img2 is the caller's next anchor).  Returns the new (h, w, 2) map."""
    from ._lib import CCMapParams
    p = CCMapParams(float(thresh), float(tear), int(use_occ))
    a = np.ascontiguousarray(anchor, np.uint8)
    b = np.ascontiguousarray(img2, np.uint8)
    bu = np.ascontiguousarray(bu, np.float32)
    bv = np.ascontiguousarray(bv, np.float32)
    o = np.ascontiguousarray(occ2, np.uint8)
    h, w = bu.shape
    m = None if cmap is None else np.ascontiguousarray(cmap, np.float32)
    if (m is not None and m.shape != (h, w, 2)) or a.shape != (h, w, 3) or b.shape != (h, w, 3) or bv.shape != (h, w) or o.shape != (h, w):
        raise ValueError("cmap_step_host: map (h, w, 2), images (h, w, 3), flow and mask (h, w)")
    out = np.empty((h, w, 2), np.float32)
    check(lib().eppm_cmap_step_host(C.byref(p), out.ctypes.data, _p(m),
                                    *[x.ctypes.data for x in (a, b, bu, bv, o)], h, w, int(bool(cut))), "eppm_cmap_step_host")
    return out


def cmap_render_host(cmap, cur, layer=None, anchor=None):
    """The render of a correspondence map on the host (eppm_cmap_render_host; bit-identical to the kernel): the (h, w, 4) uint8 RGBA layer
    (straight alpha, in the anchor frame's geometry) sampled at the (h, w, 2) map and composited over the current (h, w, 3) frame.
    layer=None: the default layer, the (h, w, 3) anchor frame with alpha 255.  Returns (h, w, 3) uint8."""
    m = np.ascontiguousarray(cmap, np.float32)
    c = np.ascontiguousarray(cur, np.uint8)
    h, w, _ = c.shape
    lay = None if layer is None else np.ascontiguousarray(layer, np.uint8)
    anc = None if anchor is None else np.ascontiguousarray(anchor, np.uint8)
    if lay is None and anc is None:
        raise ValueError("cmap_render_host: a layer or an anchor frame")
    if m.shape != (h, w, 2) or c.shape != (h, w, 3) or (lay is not None and lay.shape != (h, w, 4)) or (anc is not None and anc.shape != (h, w, 3)):
        raise ValueError("cmap_render_host: map (h, w, 2), frame and anchor (h, w, 3), layer (h, w, 4)")
    out = np.empty((h, w, 3), np.uint8)
    check(lib().eppm_cmap_render_host(out.ctypes.data, m.ctypes.data, c.ctypes.data, _p(lay),
                                      _p(anc), h, w), "eppm_cmap_render_host")
    return out


def _stab_params(tau, iters, smooth):
    from ._lib import CStabParams
    return CStabParams(float(tau), int(iters), float(smooth))


def gmotion_fit_host(u, v, occ1, tau=1.0, iters=3):
    """The camera motion of one pair on the host (eppm_gmotion_fit_host; bit-identical to the kernels).  (u, v): the
    forward flow; occ1: the occlusion mask of image 1's pixels.  Returns (model dict as Stabilizer.model, (h, w) uint8 motion mask)."""
    from ._lib import CGMotionModel
    p = _stab_params(tau, iters, 0.0)
    u = np.ascontiguousarray(u, np.float32)
    v = np.ascontiguousarray(v, np.float32)
    o = np.ascontiguousarray(occ1, np.uint8)
    h, w = u.shape
    if v.shape != (h, w) or o.shape != (h, w):
        raise ValueError("gmotion_fit_host: flow and mask (h, w)")
    m = CGMotionModel()
    mask = np.empty((h, w), np.uint8)
    check(lib().eppm_gmotion_fit_host(C.byref(p), *[x.ctypes.data for x in (u, v, o)], h, w, C.byref(m), mask.ctypes.data), "eppm_gmotion_fit_host")
    return m.as_dict(), mask


def stab_identity():
    """The paths of a clip's first frame: (C, S), the identity in (A, t) form."""
    one = np.array([1.0, 0.0, 0.0, 1.0, 0.0, 0.0])
    return one.copy(), one.copy()


def stab_update_host(c, s, model, smooth=0.9, cut=False, counts=(0, 0)):
    """One update of a slot's paths with a pair's model on the host (eppm_stab_update_host).  c, s: six float64 each (stab_identity() for
    a clip's first pair); model: a dict with p and valid.  Returns (C, S, wf (6 float32), (frames, invalid_steps))."""
    from ._lib import CGMotionModel
    p = _stab_params(1.0, 1, smooth)
    path = np.ascontiguousarray(np.concatenate([np.asarray(c, np.float64).ravel(), np.asarray(s, np.float64).ravel()]))
    if path.shape != (12,):
        raise ValueError("stab_update_host: C and S are six numbers each")
    m = CGMotionModel()
    m.p[:] = [float(x) for x in model["p"]]
    m.valid = int(model["valid"])
    n = (C.c_int64 * 2)(int(counts[0]), int(counts[1]))
    wf = np.empty(6, np.float32)
    check(lib().eppm_stab_update_host(C.byref(p), path.ctypes.data, n, C.byref(m), int(bool(cut)), wf.ctypes.data),
          "eppm_stab_update_host")
    return path[:6].copy(), path[6:].copy(), wf, (int(n[0]), int(n[1]))


def stab_warp_host(wf, img2):
    """The stabilised frame on the host (eppm_stab_warp_host): the (h, w, 3) uint8 image 2 sampled at the warp wf (6 float32)."""
    wf = np.ascontiguousarray(wf, np.float32)
    b = np.ascontiguousarray(img2, np.uint8)
    if wf.shape != (6,) or b.ndim != 3 or b.shape[2] != 3:
        raise ValueError("stab_warp_host: wf (6,), image (h, w, 3)")
    h, w, _ = b.shape
    out = np.empty((h, w, 3), np.uint8)
    check(lib().eppm_stab_warp_host(wf.ctypes.data, b.ctypes.data, h, w, out.ctypes.data),
          "eppm_stab_warp_host")
    return out


def cutdet_host(img1, img2, bu, bv, occ1, occ2, lost_permille=530, residual_max=-1.0):
    """The cut detector's record of one pair on the host (eppm_cutdet_host; equal to the kernels in every number).
    img1, img2: (h, w, 3) uint8; (bu, bv): the backward flow; occ1, occ2: the occlusion masks.  Returns the dict of CutDetector.stats."""
    from ._lib import CCutParams, CCutStats
    p = CCutParams(int(lost_permille), float(residual_max))
    a = np.ascontiguousarray(img1, np.uint8)
    b = np.ascontiguousarray(img2, np.uint8)
    bu = np.ascontiguousarray(bu, np.float32)
    bv = np.ascontiguousarray(bv, np.float32)
    o1 = np.ascontiguousarray(occ1, np.uint8)
    o2 = np.ascontiguousarray(occ2, np.uint8)
    if a.ndim != 3 or a.shape[2] != 3:
        raise ValueError("cutdet_host: images (h, w, 3)")
    h, w, _ = a.shape
    if b.shape != (h, w, 3) or any(x.shape != (h, w) for x in (bu, bv, o1, o2)):
        raise ValueError("cutdet_host: images (h, w, 3), flow and masks (h, w)")
    st = CCutStats()
    check(lib().eppm_cutdet_host(C.byref(p), *[x.ctypes.data for x in (a, b, bu, bv, o1, o2)], h, w, C.byref(st)), "eppm_cutdet_host")
    return st.as_dict()


def _objects_params(connectivity=8, min_area=16, max_objects=64, min_overlap=4, tau=1.0, iters=3):
    from ._lib import CObjectsParams
    return CObjectsParams(float(tau), int(iters), int(connectivity), int(min_area), int(max_objects), int(min_overlap))


def object_record(rec):
    """A record of the C ABI (eppm_object) as a dict, with what the host derives in float64: centroid (x, y) = sum / area and the mean
    velocity (u, v) = sum_q / (256 n_flow) in pixels per frame, None without a valid vector."""
    d = rec.as_dict()
    d["centroid"] = (d["sum_x"] / d["area"], d["sum_y"] / d["area"]) if d["area"] else None
    d["velocity"] = (d["sum_qu"] / (256.0 * d["n_flow"]), d["sum_qv"] / (256.0 * d["n_flow"])) if d["n_flow"] else None
    return d


def objects_label_host(mask, u, v, connectivity=8, min_area=16, max_objects=64):
    """Labelling on the host (eppm_objects_label_host; equal to the kernels in every number).  mask: (h, w) uint8,
    1 is foreground; (u, v): the forward flow.  Returns (labels (h, w) uint8, records: a list of n dicts with id and age 0, counts: dict
    n, n_found, n_components)."""
    from ._lib import CObject, CObjectsCounts
    p = _objects_params(connectivity, min_area, max_objects)
    m = np.ascontiguousarray(mask, np.uint8)
    u = np.ascontiguousarray(u, np.float32)
    v = np.ascontiguousarray(v, np.float32)
    if m.ndim != 2 or u.shape != m.shape or v.shape != m.shape:
        raise ValueError("objects_label_host: mask and flow (h, w)")
    h, w = m.shape
    labels = np.empty((h, w), np.uint8)
    rec = (CObject * max(int(max_objects), 1))()
    cnt = CObjectsCounts()
    check(lib().eppm_objects_label_host(C.byref(p), *[x.ctypes.data for x in (m, u, v)], h, w, labels.ctypes.data,
                                        rec, C.byref(cnt)), "eppm_objects_label_host")
    counts = cnt.as_dict()
    del counts["next_id"]
    return labels, [object_record(rec[k]) for k in range(cnt.n)], counts


def objects_carry_host(labels, bu, bv, occ2):
    """The labels as the next pair's image 1 sees them (eppm_objects_carry_host): (h, w) uint8."""
    lab = np.ascontiguousarray(labels, np.uint8)
    bu = np.ascontiguousarray(bu, np.float32)
    bv = np.ascontiguousarray(bv, np.float32)
    o = np.ascontiguousarray(occ2, np.uint8)
    if lab.ndim != 2 or any(x.shape != lab.shape for x in (bu, bv, o)):
        raise ValueError("objects_carry_host: labels, flow and mask (h, w)")
    h, w = lab.shape
    out = np.empty((h, w), np.uint8)
    check(lib().eppm_objects_carry_host(*[x.ctypes.data for x in (lab, bu, bv, o)], h, w, out.ctypes.data),
          "eppm_objects_carry_host")
    return out


def objects_state():
    """The state of an empty slot's tables: (prev_id, prev_age, next_id) = (256 zeros, 256 zeros, 1)."""
    return np.zeros(256, np.int32), np.zeros(256, np.int32), 1


def objects_assign_host(labels, n, carried, prev_id, prev_age, next_id, max_objects=64, min_overlap=4):
    """The identity rule on the host (eppm_objects_assign_host): the n objects of `labels` against the carried plane (None: all zero) and
    the previous objects' tables.  Returns (ids, ages: n ints each, prev_id, prev_age: the new 256-entry int32 tables, next_id)."""
    from ._lib import CObject
    p = _objects_params(8, 1, max_objects, min_overlap)
    lab = np.ascontiguousarray(labels, np.uint8)
    car = None if carried is None else np.ascontiguousarray(carried, np.uint8)
    if lab.ndim != 2 or (car is not None and car.shape != lab.shape):
        raise ValueError("objects_assign_host: labels and carried (h, w)")
    pid = np.array(prev_id, np.int32).copy()
    page = np.array(prev_age, np.int32).copy()
    if pid.shape != (256,) or page.shape != (256,):
        raise ValueError("objects_assign_host: prev_id and prev_age are 256 entries each")
    h, w = lab.shape
    rec = (CObject * max(int(n), 1))()
    nxt = C.c_int32(int(next_id))
    check(lib().eppm_objects_assign_host(C.byref(p), lab.ctypes.data, _p(car), h, w,
                                         int(n), pid.ctypes.data, page.ctypes.data, C.byref(nxt), rec),
          "eppm_objects_assign_host")
    return [int(rec[k].id) for k in range(n)], [int(rec[k].age) for k in range(n)], pid, page, int(nxt.value)


def _plate_params(margins=(0, 0), grow=2, accept_invalid=False, thresh=40.0, n_max=64, min_count=2):
    from ._lib import CPlateParams
    return CPlateParams(1.0, 3, int(margins[0]), int(margins[1]), int(grow), int(bool(accept_invalid)), float(thresh), int(n_max), int(min_count))


def plate_forms_host(path):
    """The two displacement forms of a camera path on the host (eppm_plate_forms_host; bit-identical to the
    kernel).  path: six float64 {a00, a01, a10, a11, tx, ty}.  Returns (fwd, inv (6 float32 each), ok)."""
    p = np.ascontiguousarray(path, np.float64)
    if p.shape != (6,):
        raise ValueError("plate_forms_host: a path is six numbers")
    fwd, inv = np.empty(6, np.float32), np.empty(6, np.float32)
    ok = C.c_int()
    check(lib().eppm_plate_forms_host(_p(p), _p(fwd), _p(inv), C.byref(ok)), "eppm_plate_forms_host")
    return fwd, inv, bool(ok.value)


def plate_block_host(mask, grow=2, accept_invalid=False):
    """The blocked plane of a motion mask on the host (eppm_plate_block_host): (h, w) uint8, 1 where a blocked byte lies within `grow`."""
    m = np.ascontiguousarray(mask, np.uint8)
    if m.ndim != 2:
        raise ValueError("plate_block_host: mask (h, w)")
    h, w = m.shape
    p = _plate_params(grow=grow, accept_invalid=accept_invalid)
    out = np.empty((h, w), np.uint8)
    check(lib().eppm_plate_block_host(C.byref(p), _p(m), h, w, _p(out)), "eppm_plate_block_host")
    return out


def plate_accumulate_host(state, fwd, img1, blocked, margins=(0, 0), thresh=40.0, n_max=64):
    """One frame accumulated into canvas states on the host (eppm_plate_accumulate_host).  state: (h + 2*my, w + 2*mx, 4) float32 {R, G, B,
    n} (all zero: an empty canvas); fwd: 6 float32; img1: (h, w, 3) uint8; blocked: (h, w) uint8.  Returns the new states (a copy)."""
    a = np.ascontiguousarray(img1, np.uint8)
    b = np.ascontiguousarray(blocked, np.uint8)
    f = np.ascontiguousarray(fwd, np.float32)
    if a.ndim != 3 or a.shape[2] != 3 or b.shape != a.shape[:2] or f.shape != (6,):
        raise ValueError("plate_accumulate_host: image (h, w, 3), blocked (h, w), fwd (6,)")
    h, w, _ = a.shape
    st = np.array(state, np.float32, order="C")
    if st.shape != (h + 2 * int(margins[1]), w + 2 * int(margins[0]), 4):
        raise ValueError("plate_accumulate_host: state (h + 2*my, w + 2*mx, 4)")
    p = _plate_params(margins=margins, thresh=thresh, n_max=n_max)
    check(lib().eppm_plate_accumulate_host(C.byref(p), _p(f), _p(a), _p(b), h, w, _p(st)), "eppm_plate_accumulate_host")
    return st


def plate_render_host(state, inv, ok, img1, blocked, margins=(0, 0), min_count=2):
    """A frame with its blocked pixels filled from canvas states on the host (eppm_plate_render_host).  Returns ((h, w, 3) uint8, fill
    (h, w) uint8: 0 free, 1 filled, 2 blocked and not filled)."""
    a = np.ascontiguousarray(img1, np.uint8)
    b = np.ascontiguousarray(blocked, np.uint8)
    f = np.ascontiguousarray(inv, np.float32)
    st = np.ascontiguousarray(state, np.float32)
    if a.ndim != 3 or a.shape[2] != 3 or b.shape != a.shape[:2] or f.shape != (6,):
        raise ValueError("plate_render_host: image (h, w, 3), blocked (h, w), inv (6,)")
    h, w, _ = a.shape
    if st.shape != (h + 2 * int(margins[1]), w + 2 * int(margins[0]), 4):
        raise ValueError("plate_render_host: state (h + 2*my, w + 2*mx, 4)")
    p = _plate_params(margins=margins, min_count=min_count)
    out, fill = np.empty((h, w, 3), np.uint8), np.empty((h, w), np.uint8)
    check(lib().eppm_plate_render_host(C.byref(p), _p(f), int(bool(ok)), _p(a), _p(b), h, w, _p(st), _p(out), _p(fill)),
          "eppm_plate_render_host")
    return out, fill

