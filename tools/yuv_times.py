"""Cost of the Y'CbCr 4:2:0 boundary at 1024x436 and 1920x1080:

  - k_yuv_to_rgba and k_rgba_to_yuv alone on caller planes (NV12, 8 bit): ms per conversion, the bytes each moves -- to RGBA 1.5 read and 4
    written per pixel, from RGBA 4 read and 1.5 written -- and that as a share of 8 TB/s;
  - a device NV12 push (eppm_yuv_push_image_device: the kernel writes the raw plane) against a device RGBA push (a 2-D copy), and
  - a host NV12 push (1.5 B/px over PCIe, converted on the device) against a host RGB push (3 B/px) of the same frames,
    each on a single context and on a batch of 8 slots, prepare included in both arms.

A figure is a host clock around `calls` calls that ends in a synchronise, per call.  The two arms of a comparison alternate in one process
after a warm-up, `repeats` times each: the median of each arm, its spread (max - min of its repeats) and the difference.  One library
per process:

    python tools/yuv_times.py [--lib exact|tol] [--calls N] [--repeats R] [--batch B]

Prints one JSON line."""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

SIZES = ((436, 1024), (1080, 1920))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--lib", default="exact", choices=["exact", "tol"])
    ap.add_argument("--calls", type=int, default=100)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--batch", type=int, default=8)
    a = ap.parse_args()
    import eppm_amd
    eppm_amd.select_library("tol" if a.lib == "tol" else "")
    from eppm_amd import synth, yuv
    from eppm_amd._lib import check, lib
    from eppm_amd.api import uchar4
    from eppm_amd.stages import Dev
    L = lib()
    fmt = yuv.YuvFormat()
    out = {"library": L.eppm_version().decode(), "calls": a.calls, "repeats": a.repeats, "batch": a.batch, "format": fmt.as_dict(), "sizes": {}}

    def timed(call, sync):
        """ms per call of `calls` calls that end in a synchronise"""
        t0 = time.perf_counter()
        for _ in range(a.calls):
            call()
        sync()
        return (time.perf_counter() - t0) * 1e3 / a.calls

    def arms(named, sync):
        """the arms in turn, `repeats` times, after one warm-up round -> per arm its median and spread, and the differences to the first"""
        for _, call in named:
            call()
        sync()
        runs = {n: [] for n, _ in named}
        for _ in range(a.repeats):
            for n, call in named:
                runs[n].append(timed(call, sync))
        r = {n: {"ms": float(np.median(v)), "spread_ms": max(v) - min(v)} for n, v in runs.items()}
        first = named[0][0]
        for n, _ in named[1:]:
            r[f"{n}_minus_{first}_ms"] = r[n]["ms"] - r[first]["ms"]
        return r

    def rgba_of(img):
        p = np.zeros(img.shape[:2], uchar4)
        p["x"], p["y"], p["z"] = img[..., 0], img[..., 1], img[..., 2]
        return p

    for h, w in SIZES:
        res = {}
        imgs = []
        for k in range(a.batch + 1):
            imgs += list(synth.make_pair_cached(h, w, seed=1234 + k)[:2])
        frames = [yuv.from_rgb(x, fmt) for x in imgs]
        rgbs = [yuv.to_rgb(f) for f in frames]                  # what the context holds either way: both arms prepare the same planes
        dev_yuv = [f.to_device(pitched=True) for f in frames]
        dev_rgba = [Dev(rgba_of(x), pitched=True) for x in rgbs]
        sync_dev = lambda: check(L.eppm_device_synchronize(), "sync")       # noqa: E731
        # -- the kernels alone
        plane = Dev(shape=(h, w), dtype=uchar4, pitched=True)
        back = yuv.from_rgba_device(fmt, dev_rgba[0])
        k = arms([("to_rgba", lambda: yuv.to_rgba_device(fmt, dev_yuv[0], plane)), ("from_rgba", lambda: yuv.from_rgba_device(fmt, dev_rgba[0], back))],
                 sync_dev)
        cw, ch = (w + 1) // 2, (h + 1) // 2
        moved = h * w + 2 * cw * ch + 4 * h * w
        for n in ("to_rgba", "from_rgba"):
            k[n]["bytes"] = moved
            k[n]["share_of_8TBs"] = moved / (k[n]["ms"] * 1e-3) / 8e12
        res["kernels"] = k
        # -- pushes: a single context, then a batch
        e = eppm_amd.EPPM()
        e.init(h, w)
        e.set_data(rgbs[0], rgbs[1])
        res["single_device_push"] = arms([("rgba", lambda: e.push_frame_device(dev_rgba[2].ptr, dev_rgba[2].pitch)),
                                          ("nv12", lambda: e.push_frame_yuv_device(fmt, dev_yuv[2]))], e.synchronize)
        res["single_host_push"] = arms([("rgb", lambda: e.push_frame(rgbs[2])), ("nv12", lambda: e.push_frame_yuv(frames[2]))], e.synchronize)
        e.close()
        n = a.batch
        b = eppm_amd.EPPMBatch(h, w, n)
        b.set_data([(rgbs[2 * i], rgbs[2 * i + 1]) for i in range(n)])
        nxt = list(range(2, 2 + n))
        res["batch_device_push"] = arms([("rgba", lambda: b.push_frames_device([dev_rgba[i].ptr for i in nxt], dev_rgba[2].pitch)),
                                         ("nv12", lambda: b.push_frames_yuv_device(fmt, [dev_yuv[i] for i in nxt]))], b.synchronize)
        res["batch_host_push"] = arms([("rgb", lambda: b.push_frames([rgbs[i] for i in nxt])), ("nv12", lambda: b.push_frames_yuv([frames[i] for i in nxt]))],
                                      b.synchronize)
        b.close()
        out["sizes"][f"{w}x{h}"] = res
    print(json.dumps(out))


if __name__ == "__main__":
    main()
