// The per-pixel arithmetic of the dense correspondence map (eppm_amd/csrc/cmap.h, what the kernels and the host forms share; no GPU code)
// under ASan + UBSan + float-cast checks: exactly sized heap planes from 1 x 1 up, so that a tap one pixel outside the frame is a report;
// NaN, inf, huge, denormal and negative-zero vectors and map values; every tear / thresh extreme, cut steps, use_occ 0 and 1.  Also the
// proof that cmap.h builds without HIP.  Built and run by tests/test_cmap_cpu.py::test_arithmetic_under_sanitizers; prints "ok" when the
// sanitizers stayed silent.
#include <math.h>
#include <stdio.h>
#include <stdlib.h>
#include <vector>
#include "../../eppm_amd/csrc/cmap.h"
using namespace eppm;
static uint32_t st = 12345u;
static uint32_t rnd() { st = st * 1664525u + 1013904223u; return st >> 8; }
int main()
{
    static const float sp[] = {NAN, INFINITY, -INFINITY, 1e10f, -1e10f, 3e38f, -3e38f, 1e9f, -1e9f, 1e-30f, -1e-45f, -0.0f, 0.0f, 62.0f, -61.99f, 0.5f, 1.5f, 2.0f};
    const int ns = sizeof sp / sizeof *sp;
    long kept = 0, total = 0;
    for (int it = 0; it < 400; it++) {
        const int h = 1 + rnd() % 9, w = 1 + rnd() % 9;
        std::vector<float> M((size_t)h * w * 2), bu((size_t)h * w), bv((size_t)h * w);
        std::vector<uint32_t> A((size_t)h * w), cur((size_t)h * w);
        std::vector<uint8_t> occ((size_t)h * w);
        for (size_t i = 0; i < (size_t)h * w; i++) {
            for (int c = 0; c < 2; c++) M[2 * i + c] = rnd() % 3 ? (float)(rnd() % (2 * (c ? h : w))) / 2.0f : sp[rnd() % ns];
            bu[i] = rnd() % 3 ? (float)(rnd() % 9) / 2.0f - 2.0f : sp[rnd() % ns];
            bv[i] = rnd() % 3 ? (float)(rnd() % 9) / 2.0f - 2.0f : sp[rnd() % ns];
            A[i] = rnd() << 8 | rnd(); cur[i] = rnd() << 8 | rnd(); occ[i] = rnd() % 5 ? 0 : rnd();
        }
        const float* mp = M.data(); const uint32_t* ap = A.data();
        auto Mf = [mp, w](int x, int y) { const float* q = mp + ((size_t)y * w + x) * 2; return CmPt{q[0], q[1]}; };
        auto Af = [ap, w](int x, int y) { return ap[(size_t)y * w + x]; };
        const float tears[] = {0.0f, 2.0f, 1e9f}, ths[] = {0.0f, 90.0f, 1e9f};
        for (int y = 0; y < h; y++)
            for (int x = 0; x < w; x++) {
                const size_t i = (size_t)y * w + x;
                const CmPt s = cmap_step_pixel(x, y, cur[i], bu[i], bv[i], occ[i], it % 7 == 0, h, w, ths[it % 3], tears[(it / 3) % 3], it & 1, Mf, Af);
                kept += fb_known(s.x, s.y); total++;
                (void)cmap_render_pixel(cur[i], s, h, w, Af);
                (void)cmap_render_pixel(cur[i], CmPt{M[2 * i], M[2 * i + 1]}, h, w, Af);
            }
    }
    printf("%ld of %ld kept\nok\n", kept, total);
    return 0;
}
