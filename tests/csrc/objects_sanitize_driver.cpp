// The semantics of moving-object detection (eppm_amd/csrc/objects.h: the per-pixel functions and the three host forms, plain sequential
// code; no GPU code) under ASan + UBSan + float-cast checks: exactly sized heap planes from 1 x 1 up, so that a neighbour or a carried
// label one pixel outside the frame is a report; masks of every byte, both connectivities, every min_area / max_objects extreme; NaN, inf,
// huge, denormal and negative-zero vectors, one ulp either side of 8192; carried bytes above max_objects, ids of any value.  Also the
// proof that objects.h builds without HIP.  Built and run by tests/test_objects_cpu.py::test_semantics_under_sanitizers; prints "ok" when
// the sanitizers stayed silent.
#include <math.h>
#include <stdio.h>
#include <stdlib.h>
#include <vector>
#include "../../eppm_amd/csrc/objects.h"
using namespace eppm;
static uint32_t st = 12345u;
static uint32_t rnd() { st = st * 1664525u + 1013904223u; return st >> 8; }
int main()
{
    static const float sp[] = {NAN, INFINITY, -INFINITY, 1e10f, -1e10f, 3e38f, -3e38f, 1e9f, -1e9f, 1e-30f, -1e-45f, -0.0f, 0.0f, 8192.0f,
                               8192.001f, 8191.9995f, -8192.0f, -8192.001f, 0.5f, 1.5f, -0.5f, 2.0f, 6.5f, -6.5f};
    const int ns = sizeof sp / sizeof *sp;
    long objects = 0, carried_px = 0, inherited = 0;
    for (int it = 0; it < 600; it++) {
        // the first iterations: thin frames at kObjMaxDim and one of 65 chunks, with backward vectors that end on the last column and row
        // and just beyond them; then small random frames
        static const int big[3][2] = {{20, kObjMaxDim}, {kObjMaxDim, 20}, {256, 257}};
        const int h = it < 3 ? big[it][0] : 1 + rnd() % 9, w = it < 3 ? big[it][1] : 1 + rnd() % 9;
        const size_t px = (size_t)h * w;
        const int conn = it & 1 ? 4 : 8;
        const int min_area = it % 5 == 0 ? (int)px + 1 : 1 + rnd() % 4;
        const int max_objects = it % 3 == 0 ? 1 : it % 3 == 1 ? 1 + (int)(rnd() % 8) : kObjMaxObjects;
        std::vector<uint8_t> mask(px), occ(px), labels(px), carried(px), prev(px);
        std::vector<float> u(px), v(px), bu(px), bv(px);
        for (size_t i = 0; i < px; i++) {
            mask[i] = rnd() % 4 ? (rnd() % 3 ? 1 : 0) : (uint8_t)rnd();
            u[i] = rnd() % 3 ? (float)(rnd() % 64) / 8.0f - 4.0f : sp[rnd() % ns];
            v[i] = rnd() % 3 ? (float)(rnd() % 64) / 8.0f - 4.0f : sp[rnd() % ns];
            bu[i] = rnd() % 3 ? (float)(rnd() % 17) / 2.0f - 4.0f : sp[rnd() % ns];
            bv[i] = rnd() % 3 ? (float)(rnd() % 17) / 2.0f - 4.0f : sp[rnd() % ns];
            occ[i] = rnd() % 5 ? 0 : (uint8_t)rnd();
            prev[i] = rnd() % 3 ? (uint8_t)(rnd() % 4) : (uint8_t)rnd();
            if (it < 3 && rnd() % 4 == 0) {
                bu[i] = (float)(w - 1 - (int)(i % w)) + (rnd() % 2 ? 0.0f : 0.001f);
                bv[i] = (float)(h - 1 - (int)(i / w)) + (rnd() % 2 ? 0.0f : 0.001f);
            }
        }
        std::vector<ObjRecord> rec(max_objects);
        ObjCounts cnt{0, 0, 0, 0};
        obj_label_host(mask.data(), u.data(), v.data(), h, w, conn, min_area, max_objects, labels.data(), rec.data(), &cnt);
        if (cnt.n < 0 || cnt.n > max_objects || cnt.n > cnt.n_found || cnt.n_found > cnt.n_components) return 1;
        for (size_t i = 0; i < px; i++)
            if (labels[i] > cnt.n || (labels[i] && !obj_foreground(mask[i]))) return 2;
        int32_t pid[kObjTable], page[kObjTable], next = it % 7 == 0 ? kObjMaxNextId : 1 + (int32_t)(rnd() % 1000);
        for (int k = 0; k < kObjTable; k++) pid[k] = (int32_t)(rnd() << 8 | rnd()), page[k] = (int32_t)(rnd() % (1u << 30));
        obj_assign_host(labels.data(), it % 4 == 0 ? nullptr : prev.data(), px, cnt.n, max_objects, 1 + (int)(rnd() % 3), pid, page, &next, rec.data());
        if (next < 1 || next > kObjMaxNextId) return 3;
        for (int k = 0; k < cnt.n; k++) inherited += rec[k].age > 0;
        obj_carry_host(labels.data(), bu.data(), bv.data(), occ.data(), h, w, carried.data());
        for (size_t i = 0; i < px; i++) {
            if (carried[i] > cnt.n) return 4;
            carried_px += carried[i] != 0;
        }
        objects += cnt.n;
    }
    printf("%ld objects, %ld inherited, %ld carried pixels\nok\n", objects, inherited, carried_px);
    return 0;
}
