// deint_sanitize_driver.cpp -- the deinterlacer's host forms and the interlaced y4m reader of eppm_io.cpp (include/eppm_deint.h) under
// ASan + UBSan + float-cast checks, built without HIP together with eppm_io.cpp alone (tests/test_deint_cpu.py).  Every plane is
// allocated at exactly its size, so a read or write outside it is a report; the vectors hold every hostile float.  Then interlaced
// files: good ones in every field order, every prefix of one, and malformed headers.  Prints "deint sanitize driver: ok".
#include <math.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <string>
#include <vector>

#include "../../include/eppm_deint.h"

#define REQUIRE(c) do { if (!(c)) { fprintf(stderr, "%s:%d: %s\n", __FILE__, __LINE__, #c); exit(1); } } while (0)

static uint32_t rng_state = 12345u;
static uint32_t rnd() { rng_state = rng_state * 1664525u + 1013904223u; return rng_state >> 8; }

static void steps(int w, int h)
{
    const size_t n = (size_t)w * h;
    const float special[] = {0.0f, -0.0f, 0.5f, -0.5f, 1.0f, -1.0f, 2.75f, (float)w, -(float)w, (float)h, -(float)h, 1e10f, -1e10f, 1e-45f, -1e-45f,
                             INFINITY, -INFINITY, NAN, 3e38f, -3e38f, 2147483648.0f, -2147483904.0f};
    const int ns = (int)(sizeof(special) / sizeof(special[0]));
    std::vector<uint8_t> ref(n * 3), cur(n * 3), out(n * 3), mask(n), occ(n);
    std::vector<float> bu(n), bv(n);
    for (int thresh : {0, 24, 765})
        for (int use_occ = 0; use_occ < 2; use_occ++)
            for (int parity = 0; parity < 2; parity++)
                for (int cut = 0; cut < 2; cut++) {
                    for (size_t i = 0; i < n * 3; i++) { ref[i] = (uint8_t)rnd(); cur[i] = (uint8_t)rnd(); }
                    for (size_t i = 0; i < n; i++) {
                        bu[i] = rnd() % 3 ? special[rnd() % ns] : (float)(rnd() % 2000) / 100.0f - 10.0f;
                        bv[i] = rnd() % 3 ? special[rnd() % ns] : (float)(rnd() % 2000) / 100.0f - 10.0f;
                        occ[i] = (uint8_t)(rnd() % 4 == 0);
                    }
                    const eppm_deint_params p = {thresh, use_occ};
                    eppm_deint_stats st;
                    REQUIRE(eppm_deint_step_host(&p, out.data(), mask.data(), &st, ref.data(), cur.data(), bu.data(), bv.data(), occ.data(), h, w, parity,
                                                 cut) == EPPM_OK);
                    int64_t t = 0, s = 0;
                    for (int y = 0; y < h; y++)
                        for (int x = 0; x < w; x++) {
                            const size_t i = (size_t)y * w + x;
                            if ((y & 1) == parity) REQUIRE(mask[i] == 0 && memcmp(&out[3 * i], &cur[3 * i], 3) == 0);
                            else REQUIRE(mask[i] == 1 || mask[i] == 2);
                            t += mask[i] == 1;
                            s += mask[i] == 2;
                        }
                    REQUIRE(t == st.temporal && s == st.spatial && (!cut || t == 0));
                }
    for (int parity = 0; parity < 2; parity++) {
        const int fh = (h - parity + 1) / 2;
        std::vector<uint8_t> field((size_t)fh * w * 3), full(n * 3);
        for (auto& b : field) b = (uint8_t)rnd();
        REQUIRE(eppm_deint_bob_host(full.data(), field.data(), h, w, parity) == EPPM_OK);
        for (int i = 0; i < fh; i++) REQUIRE(memcmp(&full[(size_t)(2 * i + parity) * w * 3], &field[(size_t)i * w * 3], (size_t)w * 3) == 0);
    }
}

static void put(const std::string& path, const std::string& bytes)
{
    FILE* f = fopen(path.c_str(), "wb");
    REQUIRE(f);
    REQUIRE(fwrite(bytes.data(), 1, bytes.size(), f) == bytes.size());
    fclose(f);
}

// opens with the interlaced reader and reads every frame: the count, or -1 at the first error; *mode: the file's field order
static int read_all(const std::string& path, int* mode)
{
    eppm_y4m* y = nullptr;
    int h = 0, w = 0, num = 0, den = 0;
    eppm_yuv_format f;
    *mode = -1;
    if (eppm_deint_y4m_open_read(&y, path.c_str(), &h, &w, &f, &num, &den, mode) != EPPM_OK) { REQUIRE(y == nullptr); return -1; }
    REQUIRE(h >= 1 && w >= 1 && *mode >= 0 && *mode <= 2 && (*mode == 0 || h % 4 == 0));
    const size_t sz = f.depth > 8 ? 2 : 1;
    std::vector<uint8_t> mem[3];
    void* p[3];
    size_t stride[3];
    for (int k = 0; k < 3; k++) {
        stride[k] = (size_t)(k ? (w + 1) / 2 : w) * sz;
        mem[k].assign(stride[k] * (k ? (h + 1) / 2 : h), 0);
        p[k] = mem[k].data();
    }
    int n = 0, got = 0, rc;
    while ((rc = eppm_y4m_read_frame(y, p, stride, &got)) == EPPM_OK && got) n++;
    REQUIRE(eppm_y4m_close(y) == EPPM_OK);
    return rc == EPPM_OK ? n : -1;
}

int main(int argc, char** argv)
{
    REQUIRE(argc == 2);
    const int sizes[][2] = {{1, 2}, {5, 3}, {63, 3}, {64, 4}, {65, 5}, {129, 9}, {200, 67}, {8192, 2}, {2, 8192}};
    for (const auto& s : sizes) steps(s[0], s[1]);
    // what the host forms refuse
    {
        uint8_t px[12] = {0}, m[2];
        float z[2] = {0, 0};
        eppm_deint_stats st;
        eppm_deint_params p = {24, 1}, bad = {766, 1};
        REQUIRE(eppm_deint_default_params(&p) == EPPM_OK && p.thresh == 24 && p.use_occ == 1 && eppm_deint_default_params(nullptr) != EPPM_OK);
        REQUIRE(eppm_deint_step_host(&p, px, m, &st, px + 6, px, z, z, m, 1, 2, 0, 0) != EPPM_OK);
        REQUIRE(eppm_deint_step_host(&bad, px, m, &st, px + 6, px, z, z, m, 2, 1, 0, 0) != EPPM_OK);
        REQUIRE(eppm_deint_step_host(&p, px, m, &st, px, px, z, z, m, 2, 1, 0, 0) != EPPM_OK);
        REQUIRE(eppm_deint_step_host(&p, px, m, &st, px + 6, px, z, z, m, 2, 1, 2, 0) != EPPM_OK);
        REQUIRE(eppm_deint_bob_host(px, px + 6, 1, 1, 0) != EPPM_OK && eppm_deint_bob_host(px, px + 6, 2, 1, 2) != EPPM_OK);
        REQUIRE(eppm_deint_bob_host(nullptr, px, 2, 1, 0) != EPPM_OK);
    }
    const std::string dir = argv[1], path = dir + "/i.y4m";
    int mode;
    const std::string body = std::string("FRAME\n") + std::string(8 * 6 * 3 / 2, 'x');
    for (int depth : {8, 10}) {
        const std::string ctag = depth == 8 ? " C420mpeg2" : " C420p10";
        const std::string frames = depth == 8 ? body + body : std::string("FRAME\n") + std::string(8 * 6 * 3, 'x');
        const char* tags[] = {"Ip", "It", "Ib"};
        for (int k = 0; k < 3; k++) {
            const std::string good = std::string("YUV4MPEG2 W6 H8 F25:1 ") + tags[k] + ctag + "\n" + frames;
            put(path, good);
            REQUIRE(read_all(path, &mode) == (depth == 8 ? 2 : 1) && mode == k);
            for (size_t n = 0; n < good.size(); n++) {          // every prefix: never more than its frames, never a crash
                put(dir + "/p.y4m", good.substr(0, n));
                REQUIRE(read_all(dir + "/p.y4m", &mode) < (depth == 8 ? 2 : 1));
            }
            eppm_y4m* y = nullptr;                              // the plain reader refuses the interlaced ones
            int h, w;
            eppm_yuv_format f;
            REQUIRE((eppm_y4m_open_read(&y, path.c_str(), &h, &w, &f, nullptr, nullptr) == EPPM_OK) == (k == 0));
            REQUIRE(eppm_y4m_close(y) == EPPM_OK);
        }
    }
    put(path, "YUV4MPEG2 W6 H8 F25:1 Im\n" + body);
    REQUIRE(read_all(path, &mode) == -1);
    put(path, "YUV4MPEG2 W6 H6 F25:1 It\n" + body);
    REQUIRE(read_all(path, &mode) == -1);
    put(path, "YUV4MPEG2 W6 H8 F25:1 It Ip\n" + body);          // a later tag replaces an earlier one
    REQUIRE(read_all(path, &mode) == 1 && mode == 0);
    put(path, "YUV4MPEG2 W6 H8 I It C422\n" + body);
    REQUIRE(read_all(path, &mode) == -1);
    put(path, "YUV4MPEG2 " + std::string(8000, 'I'));
    REQUIRE(read_all(path, &mode) == -1);
    put(path, "YUV4MPEG2 W2147483647 H2147483644 It\nFRAME\n");
    REQUIRE(read_all(path, &mode) == -1);
    eppm_y4m* y = nullptr;
    int a;
    eppm_yuv_format f;
    REQUIRE(eppm_deint_y4m_open_read(&y, path.c_str(), &a, &a, &f, nullptr, nullptr, nullptr) != EPPM_OK && y == nullptr);
    REQUIRE(eppm_deint_y4m_open_read(&y, (dir + "/absent.y4m").c_str(), &a, &a, &f, nullptr, nullptr, &mode) != EPPM_OK);
    printf("deint sanitize driver: ok\n");
    return 0;
}
