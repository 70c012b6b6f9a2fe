// The arithmetic of background plates (eppm_amd/csrc/plate.h: the per-pixel functions and the host forms, plain sequential code; no GPU
// code) under ASan + UBSan + float-cast checks: exactly sized heap planes from 1 x 1 up, so that an image tap, a blocked byte or a canvas
// state one pixel outside its plane is a report; paths with zero determinant, NaN, inf and huge entries, and forms that no path gives;
// masks of every byte under both accept_invalid settings, every grow from 0 to 8 (larger than the frames); states with NaN, inf, negative
// and huge counts and colours; thresh 0 and FLT_MAX, n_max and min_count at both ends.  Also the proof that plate.h builds without HIP.
// Built and run by tests/test_plate_cpu.py::test_semantics_under_sanitizers; prints "ok" when the sanitizers stayed silent.
#include <float.h>
#include <math.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <vector>
#include "../../eppm_amd/csrc/plate.h"
using namespace eppm;
static uint32_t st = 2222u;
static uint32_t rnd() { st = st * 1664525u + 1013904223u; return st >> 8; }
int main()
{
    static const double sp[] = {NAN, INFINITY, -INFINITY, 1e300, -1e300, 1e-300, 1e30, -1e30, 3.5e38, 1e-7, 0.0, -0.0, 1.0, -1.0, 0.5, 2.0, 8192.0, -8192.0, 1e9};
    static const float fs[] = {NAN, INFINITY, -INFINITY, FLT_MAX, -FLT_MAX, 1e30f, -1e30f, 1e-30f, -1e-45f, 0.0f, -0.0f, 0.5f, 1.0f, 2.0f, 64.0f, 255.0f, 256.0f, -1.0f, 1e9f};
    const int nsp = sizeof sp / sizeof *sp, nfs = sizeof fs / sizeof *fs;
    long valid = 0, changed = 0, filled = 0, kept = 0;
    for (int it = 0; it < 1500; it++) {
        const int h = 1 + rnd() % 9, w = 1 + rnd() % 9, mx = rnd() % 4 ? rnd() % 4 : w, my = rnd() % 4 ? rnd() % 3 : h;
        const int ch = h + 2 * my, cw = w + 2 * mx, grow = rnd() % (kPlateMaxGrow + 1);
        if (!plate_size_ok(h, w, mx, my)) return 1;
        const size_t px = (size_t)h * w, cpx = (size_t)ch * cw;
        double p[6];
        plate_identity(p);
        for (int k = 0; k < 6; k++)
            p[k] = rnd() % 4 == 0 ? sp[rnd() % nsp] : p[k] + ((double)(rnd() % 2001) - 1000.0) / (k < 4 ? 4000.0 : 100.0);
        float fwd[6], inv[6];
        bool ok = plate_forms(p, fwd, inv);
        valid += ok;
        if (it % 5 == 0) {              // forms that no path gives
            ok = true;
            for (int k = 0; k < 6; k++) fwd[k] = fs[rnd() % nfs], inv[k] = fs[rnd() % nfs];
        }
        std::vector<uint8_t> mask(px), blocked(px), rgb(px * 3), out(px * 3), fill(px);
        std::vector<TfState> state(cpx), before;
        for (size_t i = 0; i < px; i++) mask[i] = rnd() % (it % 2 ? 3 : 40) ? 0 : rnd() % 2 ? 1 : (uint8_t)rnd();
        for (size_t i = 0; i < px * 3; i++) rgb[i] = (uint8_t)rnd();
        for (size_t i = 0; i < cpx; i++) {
            float v[4];
            for (int k = 0; k < 4; k++) v[k] = rnd() % 3 == 0 ? fs[rnd() % nfs] : (float)(rnd() % 256);
            state[i] = TfState{v[0], v[1], v[2], v[3]};
        }
        before = state;
        plate_block_host(mask.data(), h, w, grow, it & 1, blocked.data());
        for (size_t i = 0; i < px; i++)
            if (blocked[i] > 1 || (plate_blocked(mask[i], it & 1) && !blocked[i])) return 2;
        const float thresh = it % 3 == 0 ? 0.0f : it % 3 == 1 ? 40.0f : FLT_MAX;
        const int n_max = it % 4 == 0 ? 1 : it % 4 == 1 ? kPlateMaxCount : 64, min_count = it % 3 == 0 ? 1 : it % 3 == 1 ? 2 : kPlateMaxCount;
        if (!plate_params_ok(mx, my, grow, thresh, n_max, min_count)) return 3;
        if (ok) plate_accumulate_host(fwd, rgb.data(), blocked.data(), h, w, mx, my, thresh, n_max, state.data());
        for (size_t i = 0; i < cpx; i++) changed += memcmp(&state[i], &before[i], sizeof(TfState)) != 0;
        plate_render_host(inv, ok, rgb.data(), blocked.data(), h, w, mx, my, min_count, state.data(), out.data(), it % 7 ? fill.data() : nullptr);
        if (it % 7)
            for (size_t i = 0; i < px; i++) {
                if (fill[i] > 2 || (fill[i] == 0) != (blocked[i] == 0)) return 4;
                if (fill[i] != 1 && memcmp(&out[i * 3], &rgb[i * 3], 3)) return 5;
                filled += fill[i] == 1;
                kept += fill[i] == 2;
            }
        for (size_t i = 0; i < cpx; i++) (void)plate_coverage(state[i].n);
    }
    if (!valid || !changed || !filled || !kept) return 6;
    printf("%ld valid paths, %ld changed states, %ld filled pixels, %ld blocked and kept\nok\n", valid, changed, filled, kept);
    return 0;
}
