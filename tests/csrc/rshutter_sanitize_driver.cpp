// The host form of rolling-shutter correction (eppm_amd/csrc/eppm_io.cpp: eppm_rolling_shutter_host, no GPU code) under ASan + UBSan +
// float-cast checks: the case sizes of the tests, NaN, inf, huge, unknown and folding vectors, every parameter extreme.  Exactly sized heap
// planes, so that a tap one pixel outside a plane is a report.  Built and run by tests/test_rshutter_cpu.py::test_host_form_under_sanitizers;
// prints "ok" when every call returned what it should and the sanitizers stayed silent.
#include <math.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <vector>

#include "../../include/eppm_rshutter.h"

static int fails = 0;
#define CHECK(c) do { if (!(c)) { printf("FAIL line %d: %s\n", __LINE__, #c); fails++; } } while (0)

static uint32_t rnd_state = 12345u;
static uint32_t rnd() { rnd_state = rnd_state * 1664525u + 1013904223u; return rnd_state >> 8; }

// field kinds: 0 zero, 1 uniform, 2 random with NaN / inf / huge / unknown entries, 3 all NaN, 4 all inf, 5 all 3e38, 6 the largest known component
// (+-1e9) across the axis and half the frame along it (velocities up to 2e9, positions that overflow within the eight steps), 7 alternating signs far beyond the frame,
// 8 components around -+n, where sg + g*fa crosses one half
static void fill(std::vector<float>& u, std::vector<float>& v, int kind, int n)
{
    static const float special[] = {NAN, INFINITY, -INFINITY, 1e10f, -1e10f, 3e38f, -3e38f, 1e9f, -1e9f, 1e-30f, 1e-45f, -0.0f, 62.0f, -61.99f};
    for (size_t i = 0; i < u.size(); i++) {
        switch (kind) {
        case 0: u[i] = v[i] = 0.0f; break;
        case 1: u[i] = 57.0f; v[i] = -33.0f; break;
        case 2:
            u[i] = (float)(rnd() % 2001) / 10.0f - 100.0f;
            v[i] = (float)(rnd() % 2001) / 10.0f - 100.0f;
            if (rnd() % 5 == 0) u[i] = special[rnd() % (sizeof(special) / sizeof(special[0]))];
            if (rnd() % 5 == 0) v[i] = special[rnd() % (sizeof(special) / sizeof(special[0]))];
            break;
        case 3: u[i] = v[i] = NAN; break;
        case 4: u[i] = INFINITY; v[i] = -INFINITY; break;
        case 5: u[i] = v[i] = 3e38f; break;
        case 6: u[i] = (i & 1) ? 1e9f : -1e9f; v[i] = (i & 2) ? -0.5f * (float)n : 0.5f * (float)n; break;
        case 7: u[i] = (i & 1) ? 5000.0f : -5000.0f; v[i] = (i & 2) ? 5000.0f : -5000.0f; break;
        default: u[i] = (float)n * ((float)(rnd() % 401) / 100.0f - 2.0f); v[i] = (float)n * ((float)(rnd() % 401) / 100.0f - 2.0f); break;
        }
    }
}

int main()
{
    static const int sizes[][2] = {{1, 1}, {1, 2}, {2, 1}, {1, 9}, {9, 1}, {3, 3}, {31, 33}, {64, 64}, {65, 97}, {70, 200}};
    static const eppm_rs_params prms[] = {{0.5f, 0.5f, 3, 0}, {1.0f, 0.0f, 8, 0}, {-1.0f, 1.0f, 8, 1}, {1.0f, 1.0f, 1, 1}, {-0.75f, 0.5f, 3, 0},
                                          {1e-6f, 0.25f, 8, 1}, {0.0f, 0.5f, 8, 0}};
    for (const auto& sz : sizes) {
        const int h = sz[0], w = sz[1];
        const size_t n = (size_t)h * w;
        for (int kind = 0; kind < 9; kind++) {
            std::vector<float> u(n), v(n);
            fill(u, v, kind, h > w ? h : w);
            std::vector<uint8_t> img(n * 3), out(n * 3);
            for (auto& b : img) b = (uint8_t)rnd();
            for (const auto& p : prms)
                for (int frame = 0; frame < 2; frame++) {
                    memset(out.data(), 0xee, out.size());
                    CHECK(eppm_rolling_shutter_host(out.data(), img.data(), u.data(), v.data(), h, w, frame, &p) == EPPM_OK);
                    if (kind == 0 || kind == 3 || kind == 4 || kind == 5 || p.readout == 0.0f) CHECK(memcmp(out.data(), img.data(), out.size()) == 0);
                }
            CHECK(eppm_rolling_shutter_host(out.data(), img.data(), u.data(), v.data(), h, w, 0, NULL) == EPPM_OK);
            // in place
            std::vector<uint8_t> same(img);
            CHECK(eppm_rolling_shutter_host(same.data(), same.data(), u.data(), v.data(), h, w, 0, NULL) == EPPM_OK);
            CHECK(memcmp(same.data(), out.data(), out.size()) == 0);
        }
    }
    // arguments
    {
        std::vector<float> u(4, 0.0f);
        std::vector<uint8_t> img(12, 0), out(12);
        eppm_rs_params p;
        CHECK(eppm_rs_default_params(&p) == EPPM_OK && p.readout == 0.5f && p.anchor == 0.5f && p.iters == 3 && p.axis == 0);
        CHECK(eppm_rs_default_params(NULL) == EPPM_ERR_ARG);
        const eppm_rs_params bad[] = {{1.5f, 0.5f, 3, 0}, {-1.5f, 0.5f, 3, 0}, {NAN, 0.5f, 3, 0}, {INFINITY, 0.5f, 3, 0}, {0.5f, -0.1f, 3, 0},
                                      {0.5f, 1.1f, 3, 0}, {0.5f, NAN, 3, 0}, {0.5f, 0.5f, 0, 0}, {0.5f, 0.5f, 9, 0}, {0.5f, 0.5f, -1, 0},
                                      {0.5f, 0.5f, 3, 2}, {0.5f, 0.5f, 3, -1}};
        for (const auto& b : bad) CHECK(eppm_rolling_shutter_host(out.data(), img.data(), u.data(), u.data(), 2, 2, 0, &b) == EPPM_ERR_ARG);
        CHECK(eppm_rolling_shutter_host(NULL, img.data(), u.data(), u.data(), 2, 2, 0, &p) == EPPM_ERR_ARG);
        CHECK(eppm_rolling_shutter_host(out.data(), NULL, u.data(), u.data(), 2, 2, 0, &p) == EPPM_ERR_ARG);
        CHECK(eppm_rolling_shutter_host(out.data(), img.data(), NULL, u.data(), 2, 2, 0, &p) == EPPM_ERR_ARG);
        CHECK(eppm_rolling_shutter_host(out.data(), img.data(), u.data(), NULL, 2, 2, 0, &p) == EPPM_ERR_ARG);
        CHECK(eppm_rolling_shutter_host(out.data(), img.data(), u.data(), u.data(), 0, 2, 0, &p) == EPPM_ERR_ARG);
        CHECK(eppm_rolling_shutter_host(out.data(), img.data(), u.data(), u.data(), 2, -1, 0, &p) == EPPM_ERR_ARG);
        CHECK(eppm_rolling_shutter_host(out.data(), img.data(), u.data(), u.data(), 8193, 1, 0, &p) == EPPM_ERR_ARG);
        CHECK(eppm_rolling_shutter_host(out.data(), img.data(), u.data(), u.data(), 8192 * 2, 8192, 0, &p) == EPPM_ERR_ARG);
        CHECK(eppm_rolling_shutter_host(out.data(), img.data(), u.data(), u.data(), 2, 2, 2, &p) == EPPM_ERR_ARG);
        CHECK(eppm_rolling_shutter_host(out.data(), img.data(), u.data(), u.data(), 2, 2, -1, &p) == EPPM_ERR_ARG);
    }
    if (fails) return 1;
    printf("ok\n");
    return 0;
}
