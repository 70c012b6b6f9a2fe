// y4m_sanitize_driver.cpp -- the y4m reader and writer of eppm_io.cpp (include/eppm_yuv.h) under ASan + UBSan, built without HIP together
// with eppm_io.cpp alone (tests/test_y4m_cpu.py).  Round trips at odd sizes and every depth with strides wider than rows, then hostile
// files: headers without end, absurd sizes, every prefix of a good file, junk tags.  Prints "ok".
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <string>
#include <vector>

#include "../../include/eppm_yuv.h"

#define REQUIRE(c) do { if (!(c)) { fprintf(stderr, "%s:%d: %s\n", __FILE__, __LINE__, #c); exit(1); } } while (0)

static void put(const std::string& path, const std::string& bytes)
{
    FILE* f = fopen(path.c_str(), "wb");
    REQUIRE(f);
    REQUIRE(fwrite(bytes.data(), 1, bytes.size(), f) == bytes.size());
    fclose(f);
}
static std::string get(const std::string& path)
{
    FILE* f = fopen(path.c_str(), "rb");
    REQUIRE(f);
    std::string s;
    char buf[4096];
    for (size_t n; (n = fread(buf, 1, sizeof(buf), f)) > 0;) s.append(buf, n);
    fclose(f);
    return s;
}

struct Frame {
    std::vector<uint8_t> mem[3];
    void* p[3];
    size_t stride[3];
    Frame(int h, int w, int depth, size_t pad)
    {
        const size_t sz = depth > 8 ? 2 : 1;
        const int rows[3] = {h, (h + 1) / 2, (h + 1) / 2}, cols[3] = {w, (w + 1) / 2, (w + 1) / 2};
        for (int k = 0; k < 3; k++) {
            stride[k] = cols[k] * sz + pad * sz;
            mem[k].assign(stride[k] * rows[k], 0);          // exactly rows x stride: a write past the last row's stride is out of bounds
            p[k] = mem[k].data();
        }
    }
};

// reads every frame the file gives; returns the count, or -1 at the first error
static int read_all(const std::string& path)
{
    eppm_y4m* y = nullptr;
    int h = 0, w = 0, num = 0, den = 0;
    eppm_yuv_format f;
    if (eppm_y4m_open_read(&y, path.c_str(), &h, &w, &f, &num, &den) != EPPM_OK) { REQUIRE(y == nullptr); return -1; }
    REQUIRE(h >= 1 && w >= 1);
    if ((long long)h * w > (1 << 24)) { eppm_y4m_close(y); return -2; }         // an absurd header opens; nobody is made to allocate for it
    Frame fr(h, w, f.depth, 3);
    int n = 0, got = 0, rc;
    while ((rc = eppm_y4m_read_frame(y, fr.p, fr.stride, &got)) == EPPM_OK && got) n++;
    REQUIRE(eppm_y4m_close(y) == EPPM_OK);
    return rc == EPPM_OK ? n : -1;
}

int main(int argc, char** argv)
{
    REQUIRE(argc == 2);
    const std::string dir = argv[1];
    const std::string path = dir + "/a.y4m";
    for (int depth : {8, 10, 12, 16})
        for (int siting : {EPPM_YUV_LEFT, EPPM_YUV_CENTER}) {
            const int h = 5, w = 7;
            eppm_yuv_format f = {EPPM_YUV_I420, depth, 0, EPPM_YUV_BT601, depth == 12, siting};
            Frame a(h, w, depth, 5), b(h, w, depth, 2);
            for (int k = 0; k < 3; k++)
                for (size_t i = 0; i < a.mem[k].size(); i++) a.mem[k][i] = (uint8_t)(i * 7 + k);
            eppm_y4m* y = nullptr;
            REQUIRE(eppm_y4m_open_write(&y, path.c_str(), h, w, &f, 24, 1) == EPPM_OK);
            for (int n = 0; n < 2; n++) REQUIRE(eppm_y4m_write_frame(y, a.p, a.stride) == EPPM_OK);
            REQUIRE(eppm_y4m_close(y) == EPPM_OK);
            int hh, ww, num, den, got;
            eppm_yuv_format g;
            REQUIRE(eppm_y4m_open_read(&y, path.c_str(), &hh, &ww, &g, &num, &den) == EPPM_OK);
            REQUIRE(hh == h && ww == w && num == 24 && den == 1 && memcmp(&f, &g, sizeof(f)) == 0);
            for (int n = 0; n < 2; n++) {
                REQUIRE(eppm_y4m_read_frame(y, b.p, b.stride, &got) == EPPM_OK && got == 1);
                const size_t sz = depth > 8 ? 2 : 1;
                for (int k = 0; k < 3; k++)
                    for (int r = 0; r < (k ? 3 : 5); r++)
                        REQUIRE(memcmp(&a.mem[k][r * a.stride[k]], &b.mem[k][r * b.stride[k]], (k ? 4 : 7) * sz) == 0);
            }
            REQUIRE(eppm_y4m_read_frame(y, b.p, b.stride, &got) == EPPM_OK && got == 0);
            size_t small[3] = {b.stride[0], 1, b.stride[2]};
            REQUIRE(eppm_y4m_read_frame(y, b.p, small, &got) == EPPM_OK && got == 0);      // the end comes first
            REQUIRE(eppm_y4m_close(y) == EPPM_OK);
            // every prefix of the good file: never more than its frames, never a crash
            const std::string good = get(path);
            REQUIRE(read_all(path) == 2);
            for (size_t n = 0; n < good.size(); n++) {
                put(dir + "/p.y4m", good.substr(0, n));
                REQUIRE(read_all(dir + "/p.y4m") < 2);
            }
        }
    const std::string bad = dir + "/b.y4m";
    put(bad, std::string(10000, 'Y'));                                      // a header line without end
    REQUIRE(read_all(bad) == -1);
    put(bad, "YUV4MPEG2 " + std::string(8000, 'W'));
    REQUIRE(read_all(bad) == -1);
    put(bad, "YUV4MPEG2 W2147483647 H2147483647 F1:1\nFRAME\n");
    REQUIRE(read_all(bad) == -1);
    put(bad, "YUV4MPEG2 W65536 H4 F1:1\nFRAME\n");
    REQUIRE(read_all(bad) == -1);
    put(bad, "YUV4MPEG2 W65535 H65535 F1:1 C420p16\nFRAME\n");
    REQUIRE(read_all(bad) == -2);
    put(bad, "YUV4MPEG2 W-4 H4 F1:1\nFRAME\n");
    REQUIRE(read_all(bad) == -1);
    put(bad, "YUV4MPEG2 W99999999999999999999 H4 F9999999999999:0 C X I A\nFRAME\n");
    (void)read_all(bad);
    put(bad, "YUV4MPEG2 W4 H4 F1:1 C\nFRAME\n");
    REQUIRE(read_all(bad) == -1);
    put(bad, "YUV4MPEG2 W4 H4\n" + std::string(1000, 'F'));               // a FRAME line without end
    REQUIRE(read_all(bad) == -1);
    put(bad, std::string("YUV4MPEG2 W4 H4\nFRAME\n") + std::string(24, '\0') + "FRAME\n" + std::string(23, '\0'));
    REQUIRE(read_all(bad) == -1);
    eppm_y4m* y = nullptr;
    int got;
    REQUIRE(eppm_y4m_open_read(&y, (dir + "/absent.y4m").c_str(), &got, &got, nullptr, nullptr, nullptr) != EPPM_OK);
    REQUIRE(eppm_y4m_read_frame(nullptr, nullptr, nullptr, nullptr) != EPPM_OK && eppm_y4m_close(nullptr) == EPPM_OK);
    printf("ok\n");
    return 0;
}
