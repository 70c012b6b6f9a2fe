// eppm_io.cpp -- file formats and error metrics of the reference's CLI path (main.cpp:56-69):
// PPM reader (basic/bao_basic.cpp:137-218), Middlebury .flo (3rdparty/middlebury/flowIO.cpp:5-20,
// :48-163), EPE/AAE (basic/bao_flow_tools.cpp:64-111); y4m files of 4:2:0 frames (include/eppm_yuv.h); the
// deinterlacer's host forms (include/eppm_deint.h); the rolling-shutter correction's host form (include/eppm_rshutter.h).  No GPU code here.
#include <limits.h>
#include <math.h>
#include <stdarg.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <vector>

#include "../../include/eppm.h"
#include "../../include/eppm_deint.h"
#include "../../include/eppm_rshutter.h"
#include "deint.h"
#include "fb_occlusion.h"
#include "interp.h"
#include "mblur.h"
#include "rshutter.h"
#include "temporal.h"
#include "yuv.h"

static int read_ppm_header(FILE* f, int* type, int* w, int* h)
{
    // "P<n>\n", then comment lines starting with '#', then "w h", then one line with maxval
    if (fgetc(f) != 'P') return -1;
    if (fscanf(f, "%d\n", type) != 1) return -1;
    char line[2048];
    *w = *h = 0;
    while (fgets(line, sizeof(line), f)) {
        if (line[0] == '#') continue;
        if (sscanf(line, "%d %d", w, h) != 2) return -1;
        break;
    }
    if (*w <= 0 || *h <= 0) return -1;
    if (!fgets(line, 100, f)) return -1;   // maxval line
    return 0;
}

extern "C" int eppm_ppm_size(const char* filename, int* h, int* w)
{
    if (!filename || !h || !w) return EPPM_ERR_ARG;
    FILE* f = fopen(filename, "rb");
    if (!f) return EPPM_ERR_ARG;
    int type = 0;
    const int r = read_ppm_header(f, &type, w, h);
    fclose(f);
    return r == 0 ? EPPM_OK : EPPM_ERR_ARG;
}

extern "C" int eppm_load_ppm(const char* filename, uint8_t* image, int h, int w, int* channels)
{
    if (!filename || !image || h <= 0 || w <= 0) return EPPM_ERR_ARG;
    FILE* f = fopen(filename, "rb");
    if (!f) return EPPM_ERR_ARG;
    int type = 0, fw = 0, fh = 0;
    if (read_ppm_header(f, &type, &fw, &fh) != 0) { fclose(f); return EPPM_ERR_ARG; }
    int rc = EPPM_OK;
    if (type == 6 || type == 5) {
        const int nc = (type == 6) ? 3 : 1;
        if (channels) *channels = nc;
        memset(image, 0, (size_t)h * w * nc);                       // as the reference does before fread
        size_t got = fread(image, 1, (size_t)h * w * nc, f);
        (void)got;                                                  // short files leave zeros (reference behaviour)
    } else {
        rc = EPPM_ERR_ARG;                                          // ASCII variants are not used by the flow path
    }
    fclose(f);
    return rc;
}

extern "C" int eppm_save_flo(const char* filename, const float* u, const float* v, int h, int w)
{
    if (!filename || !u || !v || h <= 0 || w <= 0) return EPPM_ERR_ARG;
    const char* dot = strrchr(filename, '.');
    if (!dot || strcmp(dot, ".flo") != 0) return EPPM_ERR_ARG;     // flowIO.cpp:127-133
    FILE* f = fopen(filename, "wb");
    if (!f) return EPPM_ERR_ARG;
    fwrite("PIEH", 1, 4, f);
    const int32_t ww = w, hh = h;
    fwrite(&ww, 4, 1, f);
    fwrite(&hh, 4, 1, f);
    std::vector<float> row((size_t)w * 2);
    for (int y = 0; y < h; y++) {
        for (int x = 0; x < w; x++) { row[2 * x] = u[(size_t)y * w + x]; row[2 * x + 1] = v[(size_t)y * w + x]; }
        if (fwrite(row.data(), 4, row.size(), f) != row.size()) { fclose(f); return EPPM_ERR_ARG; }
    }
    fclose(f);
    return EPPM_OK;
}

extern "C" int eppm_flo_size(const char* filename, int* h, int* w)
{
    if (!filename || !h || !w) return EPPM_ERR_ARG;
    FILE* f = fopen(filename, "rb");
    if (!f) return EPPM_ERR_ARG;
    float tag = 0;
    int32_t ww = 0, hh = 0;
    const bool ok = fread(&tag, 4, 1, f) == 1 && fread(&ww, 4, 1, f) == 1 && fread(&hh, 4, 1, f) == 1 && tag == 202021.25f &&
                    ww >= 1 && ww <= 99999 && hh >= 1 && hh <= 99999;       // flowIO.cpp:70-84
    fclose(f);
    if (!ok) return EPPM_ERR_ARG;
    *h = hh; *w = ww;
    return EPPM_OK;
}

extern "C" int eppm_load_flo(const char* filename, float* u, float* v, int h, int w)
{
    int fh = 0, fw = 0;
    if (!u || !v || eppm_flo_size(filename, &fh, &fw) != EPPM_OK || fh != h || fw != w) return EPPM_ERR_ARG;
    FILE* f = fopen(filename, "rb");
    if (!f) return EPPM_ERR_ARG;
    fseek(f, 12, SEEK_SET);
    std::vector<float> row((size_t)w * 2);
    for (int y = 0; y < h; y++) {
        if (fread(row.data(), 4, row.size(), f) != row.size()) { fclose(f); return EPPM_ERR_ARG; }
        for (int x = 0; x < w; x++) { u[(size_t)y * w + x] = row[2 * x]; v[(size_t)y * w + x] = row[2 * x + 1]; }
    }
    fclose(f);
    return EPPM_OK;
}

// basic/bao_flow_tools.cpp:64-111: a pixel counts when the ground truth is non-zero and known; `border` pixels on every side are left out
extern "C" int eppm_flow_error_border(const float* u, const float* v, const float* gu, const float* gv, int h, int w, int border, float* epe, float* aae)
{
    if (!u || !v || !gu || !gv || h <= 0 || w <= 0 || border < 0) return EPPM_ERR_ARG;
    int num_valid = 0;
    float total_angle = 0, total_epe = 0;
    for (int y = border; y < h - border; y++)
      for (int x = border; x < w - border; x++) {
        const size_t i = (size_t)y * w + x;
        const float gtuu = gu[i], gtvv = gv[i];
        if ((fabs(gtuu) > 0 && fabs(gtuu) <= 1e9) || (fabs(gtvv) > 0 && fabs(gtvv) <= 1e9)) {
            num_valid++;
            const float uu = u[i], vv = v[i];
            const float cos_val = (uu * gtuu + vv * gtvv + 1.0f) / (sqrt(uu * uu + vv * vv + 1.0f) * sqrt(gtuu * gtuu + gtvv * gtvv + 1.0f));
            const float angle_val = acos(cos_val);
            total_angle += angle_val;
            const float epe_val = sqrt((uu - gtuu) * (uu - gtuu) + (vv - gtvv) * (vv - gtvv));
            total_epe += epe_val;
        }
    }
    if (num_valid > 0) {
        if (aae) *aae = (total_angle / num_valid) * 180.0f / 3.14159f;
        if (epe) *epe = total_epe / num_valid;
    } else {
        if (aae) *aae = 0;
        if (epe) *epe = 0;
    }
    return EPPM_OK;
}
extern "C" int eppm_flow_error(const float* u, const float* v, const float* gu, const float* gv, int h, int w, float* epe, float* aae)
{
    return eppm_flow_error_border(u, v, gu, gv, h, w, 0, epe, aae);
}

// basic/bao_flow_tools.cpp:114-141: fraction of the pixels with a known ground truth whose end-point error exceeds error_thresh;
// error_map (h*w bytes, or NULL): 255 where it does, 0 elsewhere
extern "C" int eppm_flow_error_percentage(const float* u, const float* v, const float* gu, const float* gv, int h, int w, int error_thresh,
                                          uint8_t* error_map, float* fraction)
{
    if (!u || !v || !gu || !gv || !fraction || h <= 0 || w <= 0) return EPPM_ERR_ARG;
    if (error_map) memset(error_map, 0, (size_t)h * w);
    int num_valid = 0, num_correct = 0;
    for (size_t i = 0; i < (size_t)h * w; i++) {
        const float gtuu = gu[i], gtvv = gv[i];
        if (fabs(gtuu) <= 1e9 || fabs(gtvv) <= 1e9) {
            num_valid++;
            const float uu = u[i], vv = v[i];
            const float epe_val = sqrt((uu - gtuu) * (uu - gtuu) + (vv - gtvv) * (vv - gtvv));
            if (epe_val <= error_thresh) num_correct++;
            else if (error_map) error_map[i] = 255;
        }
    }
    *fraction = num_valid > 0 ? 1.0f - float(num_correct) / float(num_valid) : 0.0f;
    return EPPM_OK;
}

// basic/bao_flow_tools.cpp:166-197: both components clamped to [-|cutoff|, |cutoff|]; unknown vectors (a component above 1e9 in
// magnitude, flowIO.cpp:37-41) pass through unless cut_invalid is set
extern "C" int eppm_flow_cutoff(float* u_out, float* v_out, const float* u, const float* v, int h, int w, int cutoff, int cut_invalid)
{
    if (!u_out || !v_out || !u || !v || h <= 0 || w <= 0) return EPPM_ERR_ARG;
    const int c = (cutoff == INT_MIN) ? INT_MAX : abs(cutoff);      // fabs(INT_MIN) does not fit an int: undefined in the reference, the largest cutoff here
    for (size_t i = 0; i < (size_t)h * w; i++) {
        const float x = u[i], y = v[i];
        if (!cut_invalid && (fabs(x) > 1e9 || fabs(y) > 1e9)) { u_out[i] = x; v_out[i] = y; continue; }
        const float lx = (x < c) ? x : (float)c, ly = (y < c) ? y : (float)c;           // __min(val, cutoff), then __max(., -cutoff)
        u_out[i] = (lx > -c) ? lx : (float)-c;
        v_out[i] = (ly > -c) ? ly : (float)-c;
    }
    return EPPM_OK;
}

// Host colour coding of a flow field (basic/bao_flow_tools.cpp:200-231 on Middlebury's computeColor, colorcode.cpp:30-85): vectors are
// scaled by the largest known radius of the field, unknown vectors are black; rgb: h*w*3 bytes, R,G,B.  (The device routine of the
// optional color_flow output, k_color.hip, is the reference's CUDA port of the same wheel with a fixed scale.)
namespace {
struct Wheel {
    int n = 0, c[60][3];
    Wheel()
    {
        const int RY = 15, YG = 6, GC = 4, CB = 11, BM = 13, MR = 6;
        auto put = [&](int r, int g, int b) { c[n][0] = r; c[n][1] = g; c[n][2] = b; n++; };
        for (int i = 0; i < RY; i++) put(255, 255 * i / RY, 0);
        for (int i = 0; i < YG; i++) put(255 - 255 * i / YG, 255, 0);
        for (int i = 0; i < GC; i++) put(0, 255, 255 * i / GC);
        for (int i = 0; i < CB; i++) put(0, 255 - 255 * i / CB, 255);
        for (int i = 0; i < BM; i++) put(255 * i / BM, 0, 255);
        for (int i = 0; i < MR; i++) put(255, 0, 255 - 255 * i / MR);
    }
};
}  // namespace
extern "C" int eppm_flow_to_color_host(uint8_t* rgb, const float* u, const float* v, int h, int w)
{
    if (!rgb || !u || !v || h <= 0 || w <= 0) return EPPM_ERR_ARG;
    static const Wheel W;
    float maxrad = -1;
    for (size_t i = 0; i < (size_t)h * w; i++) {
        const float fx = u[i], fy = v[i];
        if (!(fabs(fx) <= 1e9) || !(fabs(fy) <= 1e9)) continue;
        const float rad = sqrt(fx * fx + fy * fy);
        maxrad = (maxrad > rad) ? maxrad : rad;
    }
    // A field with no motion (maxrad 0) or no known vector (-1) divides 0 by 0 in the reference and indexes the wheel with (int)NaN --
    // undefined there (a crash on x86); here the scale is 1 (Middlebury's own color_flow tool: "if (maxrad == 0) maxrad = 1"), and a
    // vector with a NaN component is drawn black like an unknown one.
    if (!(maxrad > 0)) maxrad = 1;
    for (size_t i = 0; i < (size_t)h * w; i++) {
        uint8_t* o = rgb + i * 3;
        if (!(fabs(u[i]) <= 1e9) || !(fabs(v[i]) <= 1e9)) { o[0] = o[1] = o[2] = 0; continue; }
        const float fx = u[i] / maxrad, fy = v[i] / maxrad;
        const float rad = sqrt(fx * fx + fy * fy);
        const float a = atan2(-fy, -fx) / M_PI;
        const float fk = (a + 1.0f) / 2.0f * (W.n - 1);
        const int k0 = (int)fk, k1 = (k0 + 1) % W.n;
        const float f = fk - k0;
        for (int b = 0; b < 3; b++) {
            const float col0 = W.c[k0][b] / 255.0f, col1 = W.c[k1][b] / 255.0f;
            float col = (1 - f) * col0 + f * col1;
            if (rad <= 1) col = 1 - rad * (1 - col);
            else col *= .75;
            o[b] = (uint8_t)(int)(255.0 * col);            // computeColor writes B,G,R; bao_convert_flow_to_colorshow swaps to R,G,B
        }
    }
    return EPPM_OK;
}

// the occlusion masks' criterion on host flows (fb_occlusion.h, the kernel's own per-pixel function): occ[y*w+x] for F = (u, v), G = (bu, bv)
extern "C" int eppm_fb_occlusion_host(uint8_t* occ, const float* u, const float* v, const float* bu, const float* bv, int h, int w, float alpha,
                                      float beta)
{
    if (!occ || !u || !v || !bu || !bv || h < 1 || w < 1) return EPPM_ERR_ARG;
    if (!(alpha >= 0 && isfinite(alpha)) || !(beta >= 0 && isfinite(beta))) return EPPM_ERR_ARG;
    const size_t n = (size_t)h * w;
    std::vector<float> G(n * 2);
    for (size_t i = 0; i < n; i++) { G[2 * i] = bu[i]; G[2 * i + 1] = bv[i]; }
    for (int y = 0; y < h; y++)
        for (int x = 0; x < w; x++) {
            const size_t i = (size_t)y * w + x;
            occ[i] = eppm::fb_occlusion_pixel(x, y, u[i], v[i], G.data(), h, w, alpha, beta);
        }
    return EPPM_OK;
}

// the temporal prior on host planes (temporal.h): the landing competition as a sequential minimum over the source
// indices, the targets by the kernels' own function.  prev: h*w displacements, prior: h*w absolute targets.
extern "C" int eppm_temporal_prior_host(eppm_short2* prior, const eppm_short2* prev, int h, int w, int backward)
{
    if (!prior || !prev || h < 1 || w < 1 || h > 32767 || w > 32767) return EPPM_ERR_ARG;
    const size_t n = (size_t)h * w;
    if (n >= ((size_t)1 << 30)) return EPPM_ERR_ARG;
    const int step = backward ? -1 : 1;
    std::vector<int> keys(n, eppm::kTemporalNoKey);
    for (int y = 0; y < h; y++)
        for (int x = 0; x < w; x++) {
            const int i = y * w + x;
            int qx, qy;
            if (eppm::temporal_landing(x, y, prev[i].x, prev[i].y, step, w, h, &qx, &qy) && i < keys[(size_t)qy * w + qx]) keys[(size_t)qy * w + qx] = i;
        }
    for (int y = 0; y < h; y++)
        for (int x = 0; x < w; x++) {
            const int i = y * w + x, k = keys[i];
            const bool won = k != eppm::kTemporalNoKey;
            eppm::temporal_target(x, y, won, won ? prev[k].x : 0, won ? prev[k].y : 0, w, h, &prior[i].x, &prior[i].y);
        }
    return EPPM_OK;
}

// frame interpolation on host planes.  The splat, the blend and every other float operation are interp.h's, the
// kernels' own; the minimum over the keys and the two fill passes are plain sequential loops written here (scans of the nearest filled pixel),
// independent of the kernels' searches.  rgb_out, rgb1, rgb2: h rows of w R,G,B triplets, packed.
extern "C" int eppm_interpolate_host(uint8_t* rgb_out, const uint8_t* rgb1, const uint8_t* rgb2, const float* u, const float* v, const uint8_t* occ1,
                                     const uint8_t* occ2, int h, int w, float t)
{
    if (!rgb_out || !rgb1 || !rgb2 || !u || !v || !occ1 || !occ2 || h < 1 || w < 1 || !eppm::interp_t_ok(t)) return EPPM_ERR_ARG;
    const size_t n = (size_t)h * w;
    if (eppm::interp_endpoint(t)) {
        memcpy(rgb_out, t == 0.0f ? rgb1 : rgb2, n * 3);
        return EPPM_OK;
    }
    auto word = [](const uint8_t* p) { return (uint32_t)p[0] | ((uint32_t)p[1] << 8) | ((uint32_t)p[2] << 16); };
    auto img1 = [&](int x, int y) { return word(rgb1 + ((size_t)y * w + x) * 3); };
    auto img2 = [&](int x, int y) { return word(rgb2 + ((size_t)y * w + x) * 3); };
    // (a) splat
    std::vector<uint64_t> key(n, eppm::kInterpHole);
    for (int y = 0; y < h; y++)
        for (int x = 0; x < w; x++) {
            const size_t i = (size_t)y * w + x;
            if (!eppm::fb_known(u[i], v[i])) continue;
            uint64_t k;
            int bx, by;
            if (!eppm::interp_splat_pixel(x, y, u[i], v[i], t, h, w, img1(x, y), occ1[i] != 0, img2, &k, &bx, &by)) continue;
            for (int ty = by; ty <= by + 1; ty++)
                for (int tx = bx; tx <= bx + 1; tx++)
                    if (ty >= 0 && ty < h && tx >= 0 && tx < w && k < key[(size_t)ty * w + tx]) key[(size_t)ty * w + tx] = k;
        }
    // (b) pass 1: nearest splatted pixel left, right, up, down (running last-seen indices), ties in that order
    std::vector<long long> src(n, -1);
    for (size_t i = 0; i < n; i++)
        if (key[i] != eppm::kInterpHole) src[i] = (long long)(uint32_t)key[i];
    std::vector<int> lft(n, -1), rgt(n, -1), up(n, -1), dn(n, -1);      // column / row of the nearest splatted pixel, -1 none
    for (int y = 0; y < h; y++) {
        int last = -1;
        for (int x = 0; x < w; x++) { lft[(size_t)y * w + x] = last; if (src[(size_t)y * w + x] >= 0) last = x; }
        last = -1;
        for (int x = w - 1; x >= 0; x--) { rgt[(size_t)y * w + x] = last; if (src[(size_t)y * w + x] >= 0) last = x; }
    }
    for (int x = 0; x < w; x++) {
        int last = -1;
        for (int y = 0; y < h; y++) { up[(size_t)y * w + x] = last; if (src[(size_t)y * w + x] >= 0) last = y; }
        last = -1;
        for (int y = h - 1; y >= 0; y--) { dn[(size_t)y * w + x] = last; if (src[(size_t)y * w + x] >= 0) last = y; }
    }
    std::vector<long long> f1(src);
    for (int y = 0; y < h; y++)
        for (int x = 0; x < w; x++) {
            const size_t i = (size_t)y * w + x;
            if (src[i] >= 0) continue;
            long long best = -1;
            int bd = INT_MAX;
            if (lft[i] >= 0 && x - lft[i] < bd) { bd = x - lft[i]; best = src[(size_t)y * w + lft[i]]; }
            if (rgt[i] >= 0 && rgt[i] - x < bd) { bd = rgt[i] - x; best = src[(size_t)y * w + rgt[i]]; }
            if (up[i] >= 0 && y - up[i] < bd) { bd = y - up[i]; best = src[(size_t)up[i] * w + x]; }
            if (dn[i] >= 0 && dn[i] - y < bd) { bd = dn[i] - y; best = src[(size_t)dn[i] * w + x]; }
            f1[i] = best;
        }
    // (b) pass 2: nearest filled pixel of pass 1's result in the row, ties to the left
    std::vector<long long> f2(f1);
    for (int y = 0; y < h; y++) {
        const long long* row = &f1[(size_t)y * w];
        int last = -1;
        std::vector<int> l(w), r(w);
        for (int x = 0; x < w; x++) { l[x] = last; if (row[x] >= 0) last = x; }
        last = -1;
        for (int x = w - 1; x >= 0; x--) { r[x] = last; if (row[x] >= 0) last = x; }
        for (int x = 0; x < w; x++) {
            if (row[x] >= 0) continue;
            if (l[x] >= 0 && (r[x] < 0 || x - l[x] <= r[x] - x)) f2[(size_t)y * w + x] = row[l[x]];
            else if (r[x] >= 0) f2[(size_t)y * w + x] = row[r[x]];
        }
    }
    // (c) blend
    auto o1 = [&](int x, int y) { return occ1[(size_t)y * w + x]; };
    auto o2 = [&](int x, int y) { return occ2[(size_t)y * w + x]; };
    for (int y = 0; y < h; y++)
        for (int x = 0; x < w; x++) {
            const size_t i = (size_t)y * w + x;
            const long long s = f2[i];
            const float ux = s >= 0 ? u[s] : 0.0f, uy = s >= 0 ? v[s] : 0.0f;
            const uint32_t p = eppm::interp_blend_pixel(x, y, ux, uy, t, h, w, img1, img2, o1, o2);
            rgb_out[i * 3] = (uint8_t)p; rgb_out[i * 3 + 1] = (uint8_t)(p >> 8); rgb_out[i * 3 + 2] = (uint8_t)(p >> 16);
        }
    return EPPM_OK;
}

// synthetic shutter on host planes.  The half-vector, the packed word, the key and the gather are mblur.h's, the
// kernels' own; the maximum over the keys is a plain scan written here (tile maxima, then the up to 3x3 tiles around each tile).
// rgb_out, rgb: h rows of w R,G,B triplets, packed.
extern "C" int eppm_mblur_default_params(eppm_mblur_params* p)
{
    if (!p) return EPPM_ERR_ARG;
    p->shutter = 0.5f;
    p->max_radius = 16.0f;
    p->taps = 8;
    return EPPM_OK;
}

extern "C" int eppm_motion_blur_host(uint8_t* rgb_out, const uint8_t* rgb, const float* u, const float* v, int h, int w, const eppm_mblur_params* params)
{
    eppm_mblur_params prm;
    if (params) prm = *params;
    else (void)eppm_mblur_default_params(&prm);
    if (!rgb_out || !rgb || !u || !v || h < 1 || w < 1 || h > 8192 || w > 8192 || (long long)h * w > (1LL << 26)) return EPPM_ERR_ARG;
    if (!eppm::mblur_params_ok(prm.shutter, prm.max_radius, prm.taps)) return EPPM_ERR_ARG;
    const size_t n = (size_t)h * w;
    const int T = eppm::kMBlurTile, tx = (w + T - 1) / T, ty = (h + T - 1) / T;
    std::vector<uint32_t> packed(n);
    std::vector<uint64_t> tkey((size_t)tx * ty, 0);
    for (int y = 0; y < h; y++)
        for (int x = 0; x < w; x++) {
            const size_t i = (size_t)y * w + x;
            const eppm::MBlurVec hv = eppm::mblur_half_vector(u[i], v[i], prm.shutter, prm.max_radius);
            packed[i] = eppm::mblur_pack((uint32_t)rgb[i * 3] | ((uint32_t)rgb[i * 3 + 1] << 8) | ((uint32_t)rgb[i * 3 + 2] << 16), hv.m);
            const uint64_t k = eppm::mblur_key(hv.m, (uint32_t)i);
            uint64_t& t = tkey[(size_t)(y / T) * tx + x / T];
            if (k > t) t = k;
        }
    auto pk = [&](int x, int y) { return packed[(size_t)y * w + x]; };
    for (int by = 0; by < ty; by++)
        for (int bx = 0; bx < tx; bx++) {
            uint64_t K = 0;
            for (int qy = by > 0 ? by - 1 : 0; qy <= by + 1 && qy < ty; qy++)
                for (int qx = bx > 0 ? bx - 1 : 0; qx <= bx + 1 && qx < tx; qx++)
                    if (tkey[(size_t)qy * tx + qx] > K) K = tkey[(size_t)qy * tx + qx];
            const size_t j = eppm::mblur_key_pixel(K);
            const eppm::MBlurVec d = eppm::mblur_half_vector(u[j], v[j], prm.shutter, prm.max_radius);
            for (int y = by * T; y < by * T + T && y < h; y++)
                for (int x = bx * T; x < bx * T + T && x < w; x++) {
                    const size_t i = (size_t)y * w + x;
                    const uint32_t p = eppm::mblur_gather_pixel(x, y, d.hx, d.hy, d.m, prm.taps, h, w, pk);
                    rgb_out[i * 3] = (uint8_t)p; rgb_out[i * 3 + 1] = (uint8_t)(p >> 8); rgb_out[i * 3 + 2] = (uint8_t)(p >> 16);
                }
        }
    return EPPM_OK;
}

// rolling-shutter correction on host planes.  The velocity and the gather are rshutter.h's, the kernels' own, in
// the kernels' two passes: the velocity plane first, then every output pixel.  rgb_out, rgb: h rows of w R,G,B triplets, packed.
extern "C" int eppm_rs_default_params(eppm_rs_params* p)
{
    if (!p) return EPPM_ERR_ARG;
    p->readout = 0.5f;
    p->anchor = 0.5f;
    p->iters = 3;
    p->axis = 0;
    return EPPM_OK;
}

extern "C" int eppm_rolling_shutter_host(uint8_t* rgb_out, const uint8_t* rgb, const float* u, const float* v, int h, int w, int frame,
                                         const eppm_rs_params* params)
{
    eppm_rs_params prm;
    if (params) prm = *params;
    else (void)eppm_rs_default_params(&prm);
    if (!rgb_out || !rgb || !u || !v || h < 1 || w < 1 || h > 8192 || w > 8192 || (long long)h * w > (1LL << 26)) return EPPM_ERR_ARG;
    if (!eppm::rs_params_ok(prm.readout, prm.anchor, prm.iters, prm.axis) || (frame != 0 && frame != 1)) return EPPM_ERR_ARG;
    const size_t n = (size_t)h * w;
    const eppm::RsConst k = eppm::rs_const(prm.readout, prm.anchor, prm.axis, frame, h, w);
    std::vector<eppm::RsVel> plane(n);
    for (size_t i = 0; i < n; i++) plane[i] = eppm::rs_velocity(u[i], v[i], k);
    auto vel = [&](int x, int y) { return plane[(size_t)y * w + x]; };
    auto px = [&](int x, int y) {
        const uint8_t* p = rgb + ((size_t)y * w + x) * 3;
        return (uint32_t)p[0] | ((uint32_t)p[1] << 8) | ((uint32_t)p[2] << 16);
    };
    std::vector<uint8_t> tmp;                   // rgb_out may be rgb: the gather reads the whole frame
    uint8_t* out = rgb_out;
    if (rgb_out == rgb) { tmp.resize(n * 3); out = tmp.data(); }
    for (int y = 0; y < h; y++)
        for (int x = 0; x < w; x++) {
            const size_t i = (size_t)y * w + x;
            const uint32_t p = eppm::rs_gather_pixel(x, y, k, prm.iters, h, w, vel, px);
            out[i * 3] = (uint8_t)p; out[i * 3 + 1] = (uint8_t)(p >> 8); out[i * 3 + 2] = (uint8_t)(p >> 16);
        }
    if (out != rgb_out) memcpy(rgb_out, out, n * 3);
    return EPPM_OK;
}

// ---- y4m (YUV4MPEG2) files: include/eppm_yuv.h.  I420 planes; the header's tags map to a format and back. ----
// A failure's message goes to eppm_last_error through the hook below, which the library sets to its set_err (api_common.cpp).  This file
// also builds alone, without HIP (the sanitizer drivers of the tests): there the hook stays null and a failure is its code alone.
int (*eppm_io_error_hook)(int code, const char* message) __attribute__((visibility("hidden"))) = nullptr;
static int y4m_err(int code, const char* fmt, ...) __attribute__((format(printf, 2, 3)));
static int y4m_err(int code, const char* fmt, ...)
{
    char msg[512];
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(msg, sizeof(msg), fmt, ap);
    va_end(ap);
    return eppm_io_error_hook ? eppm_io_error_hook(code, msg) : code;
}
using eppm::yuv_plane_size;

struct eppm_y4m {
    FILE* f = nullptr;
    bool writing = false;
    int h = 0, w = 0;
    eppm_yuv_format fmt;
    int rows[3];
    size_t row[3];
};

namespace {
// a line of at most n - 1 bytes without its '\n'; -1: end of file before any byte, -2: no '\n' within n - 1 bytes or before the end
int y4m_line(FILE* f, char* buf, int n)
{
    int len = 0;
    for (;;) {
        const int ch = fgetc(f);
        if (ch == EOF) return len == 0 ? -1 : -2;
        if (ch == '\n') break;
        if (len >= n - 1) return -2;
        buf[len++] = (char)ch;
    }
    buf[len] = 0;
    return len;
}
int y4m_fail(eppm_y4m* y, int code)
{
    if (y->f) fclose(y->f);
    delete y;
    return code;
}
// the number a tag's value starts with: its leading decimal digits alone (no sign, no blanks), 0 for none, INT_MAX beyond int; *end:
// the first character after them
int y4m_int(const char* v, const char** end = nullptr)
{
    long long n = 0;
    for (; *v >= '0' && *v <= '9'; v++) n = n > INT_MAX ? n : n * 10 + (*v - '0');
    if (end) *end = v;
    return n > INT_MAX ? INT_MAX : (int)n;
}
void y4m_dims(eppm_y4m* y)
{
    for (int p = 0; p < 3; p++) yuv_plane_size(y->fmt, y->h, y->w, p, &y->rows[p], &y->row[p]);
}
}  // namespace

// eppm_y4m_open_read (interlace NULL: interlaced files are refused) and eppm_deint_y4m_open_read (*interlace: 0 progressive, 1 top field
// first, 2 bottom field first); who: the call's name in the messages
static int y4m_open(const char* who, eppm_y4m** out, const char* path, int* h, int* w, eppm_yuv_format* f, int* fps_num, int* fps_den, int* interlace)
{
    if (!out || !path || !h || !w || !f) return y4m_err(EPPM_ERR_ARG, "%s: NULL argument", who);
    *out = nullptr;
    eppm_y4m* y = new eppm_y4m;
    y->f = fopen(path, "rb");
    if (!y->f) { const int r = y4m_err(EPPM_ERR_ARG, "%s: cannot open %s", who, path); return y4m_fail(y, r); }
    char line[4096];
    if (y4m_line(y->f, line, sizeof(line)) < 0 || strncmp(line, "YUV4MPEG2", 9) != 0 || (line[9] != ' ' && line[9] != 0))
        return y4m_fail(y, y4m_err(EPPM_ERR_ARG, "%s: %s: malformed: no YUV4MPEG2 header line", who, path));
    y->fmt = eppm_yuv_format{EPPM_YUV_I420, 8, 0, EPPM_YUV_BT709, 0, EPPM_YUV_LEFT};
    int num = 0, den = 0;
    bool center_x = false;
    int mode = 0;
    for (char* tok = strtok(line + 9, " "); tok; tok = strtok(nullptr, " ")) {
        const char* v = tok + 1;
        switch (tok[0]) {
        case 'W': y->w = y4m_int(v); break;
        case 'H': y->h = y4m_int(v); break;
        case 'F': {         // num:den, digits on both sides and nothing after them; anything else: unknown (0:0)
            const char *colon = nullptr, *end = nullptr;
            num = y4m_int(v, &colon);
            den = *colon == ':' ? y4m_int(colon + 1, &end) : 0;
            if (colon == v || *colon != ':' || end == colon + 1 || *end) num = den = 0;
            break;
        }
        case 'I':
            if (v[0] == 'm' || (!interlace && (v[0] == 't' || v[0] == 'b')))
                return y4m_fail(y, y4m_err(EPPM_ERR_ARG, "%s: %s: interlaced material (%s) is not supported", who, path, tok));
            mode = v[0] == 't' ? 1 : v[0] == 'b' ? 2 : 0;       // a later tag replaces an earlier one
            break;
        case 'C':
            y->fmt.siting = EPPM_YUV_LEFT;       // a tag names depth and siting both: a later tag replaces an earlier one whole
            if (!strcmp(v, "420jpeg")) { y->fmt.depth = 8; y->fmt.siting = EPPM_YUV_CENTER; }
            else if (!strcmp(v, "420mpeg2") || !strcmp(v, "420")) y->fmt.depth = 8;
            else if (!strcmp(v, "420p10")) y->fmt.depth = 10;
            else if (!strcmp(v, "420p12")) y->fmt.depth = 12;
            else if (!strcmp(v, "420p16")) y->fmt.depth = 16;
            else return y4m_fail(y, y4m_err(EPPM_ERR_ARG, "%s: %s: colour space %s is not supported (4:2:0 %s)", who, path, tok, interlace ? "only" : "progressive only"));
            break;
        case 'X':
            if (!strcmp(v, "COLORRANGE=FULL")) y->fmt.full_range = 1;
            else if (!strcmp(v, "COLORRANGE=LIMITED")) y->fmt.full_range = 0;
            else if (!strcmp(v, "EPPM_SITING=CENTER")) center_x = true;
            break;
        default: break;      // A (aspect) and anything unknown
        }
    }
    if (y->w < 1 || y->h < 1) return y4m_fail(y, y4m_err(EPPM_ERR_ARG, "%s: %s: malformed: missing W or H", who, path));
    if (y->w > eppm::kYuvMaxDim || y->h > eppm::kYuvMaxDim) return y4m_fail(y, y4m_err(EPPM_ERR_ARG, "%s: %s: malformed: W or H beyond %d", who, path, eppm::kYuvMaxDim));
    if (mode != 0 && y->h % 4 != 0)
        return y4m_fail(y, y4m_err(EPPM_ERR_ARG, "%s: %s: an interlaced 4:2:0 file needs H a multiple of 4 (H%d): each field is a 4:2:0 picture", who, path, y->h));
    if (center_x) y->fmt.siting = EPPM_YUV_CENTER;
    y->fmt.matrix = y->h < 720 ? EPPM_YUV_BT601 : EPPM_YUV_BT709;
    y4m_dims(y);
    *h = y->h; *w = y->w; *f = y->fmt;
    if (fps_num) *fps_num = num;
    if (fps_den) *fps_den = den;
    if (interlace) *interlace = mode;
    *out = y;
    return EPPM_OK;
}

extern "C" int eppm_y4m_open_read(eppm_y4m** out, const char* path, int* h, int* w, eppm_yuv_format* f, int* fps_num, int* fps_den)
{
    return y4m_open("eppm_y4m_open_read", out, path, h, w, f, fps_num, fps_den, nullptr);
}

extern "C" int eppm_y4m_read_frame(eppm_y4m* y, void* const* planes, const size_t* strides, int* got)
{
    if (!y || !planes || !strides || !got) return y4m_err(EPPM_ERR_ARG, "eppm_y4m_read_frame: NULL argument");
    if (y->writing) return y4m_err(EPPM_ERR_STATE, "eppm_y4m_read_frame: the file is open for writing");
    *got = 0;
    char line[256];
    const int n = y4m_line(y->f, line, sizeof(line));
    if (n == -1) return EPPM_OK;
    if (n < 0 || strncmp(line, "FRAME", 5) != 0 || (line[5] != ' ' && line[5] != 0))
        return y4m_err(EPPM_ERR_ARG, "eppm_y4m_read_frame: malformed: missing FRAME line");
    for (int p = 0; p < 3; p++) {
        if (!planes[p] || strides[p] < y->row[p]) return y4m_err(EPPM_ERR_ARG, "eppm_y4m_read_frame: NULL plane %d or stride below the row's %zu bytes", p, y->row[p]);
        for (int r = 0; r < y->rows[p]; r++)
            if (fread((uint8_t*)planes[p] + (size_t)r * strides[p], 1, y->row[p], y->f) != y->row[p])
                return y4m_err(EPPM_ERR_ARG, "eppm_y4m_read_frame: malformed: truncated frame");
    }
    *got = 1;
    return EPPM_OK;
}

extern "C" int eppm_y4m_open_write(eppm_y4m** out, const char* path, int h, int w, const eppm_yuv_format* f, int fps_num, int fps_den)
{
    if (!out || !path || !f) return y4m_err(EPPM_ERR_ARG, "eppm_y4m_open_write: NULL argument");
    *out = nullptr;
    const char* why = nullptr;
    if (!eppm::yuv_format_ok(*f, &why)) return y4m_err(EPPM_ERR_ARG, "eppm_y4m_open_write: bad format: %s", why);
    if (f->layout != EPPM_YUV_I420 || f->msb_aligned) return y4m_err(EPPM_ERR_ARG, "eppm_y4m_open_write: a y4m file holds I420 planes of low-aligned words");
    if (h < 1 || w < 1 || h > eppm::kYuvMaxDim || w > eppm::kYuvMaxDim || fps_num < 1 || fps_den < 1) return y4m_err(EPPM_ERR_ARG, "eppm_y4m_open_write: bad size %d x %d or rate %d:%d", w, h, fps_num, fps_den);
    eppm_y4m* y = new eppm_y4m;
    y->writing = true;
    y->h = h; y->w = w; y->fmt = *f;
    y4m_dims(y);
    y->f = fopen(path, "wb");
    if (!y->f) { const int r = y4m_err(EPPM_ERR_ARG, "eppm_y4m_open_write: cannot open %s", path); return y4m_fail(y, r); }
    char tag[64];
    if (f->depth == 8) snprintf(tag, sizeof(tag), "C420%s", f->siting == EPPM_YUV_CENTER ? "jpeg" : "mpeg2");
    else snprintf(tag, sizeof(tag), "C420p%d%s", f->depth, f->siting == EPPM_YUV_CENTER ? " XEPPM_SITING=CENTER" : "");
    if (fprintf(y->f, "YUV4MPEG2 W%d H%d F%d:%d Ip A1:1 %s XCOLORRANGE=%s\n", w, h, fps_num, fps_den, tag, f->full_range ? "FULL" : "LIMITED") < 0)
        return y4m_fail(y, y4m_err(EPPM_ERR_ARG, "eppm_y4m_open_write: cannot write %s", path));
    *out = y;
    return EPPM_OK;
}

extern "C" int eppm_y4m_write_frame(eppm_y4m* y, const void* const* planes, const size_t* strides)
{
    if (!y || !planes || !strides) return y4m_err(EPPM_ERR_ARG, "eppm_y4m_write_frame: NULL argument");
    if (!y->writing) return y4m_err(EPPM_ERR_STATE, "eppm_y4m_write_frame: the file is open for reading");
    for (int p = 0; p < 3; p++)
        if (!planes[p] || strides[p] < y->row[p]) return y4m_err(EPPM_ERR_ARG, "eppm_y4m_write_frame: NULL plane %d or stride below the row's %zu bytes", p, y->row[p]);
    bool ok = fputs("FRAME\n", y->f) >= 0;
    for (int p = 0; p < 3 && ok; p++)
        for (int r = 0; r < y->rows[p] && ok; r++) ok = fwrite((const uint8_t*)planes[p] + (size_t)r * strides[p], 1, y->row[p], y->f) == y->row[p];
    return ok ? EPPM_OK : y4m_err(EPPM_ERR_ARG, "eppm_y4m_write_frame: write failed");
}

extern "C" int eppm_y4m_close(eppm_y4m* y)
{
    if (!y) return EPPM_OK;
    const bool ok = fclose(y->f) == 0 || !y->writing;
    delete y;
    return ok ? EPPM_OK : y4m_err(EPPM_ERR_ARG, "eppm_y4m_close: write failed");
}

// ---- deinterlacing (include/eppm_deint.h): the interlaced reader and the host forms; the arithmetic is deint.h's ----
extern "C" int eppm_deint_y4m_open_read(eppm_y4m** out, const char* path, int* h, int* w, eppm_yuv_format* f, int* fps_num, int* fps_den, int* interlace)
{
    if (!interlace) return y4m_err(EPPM_ERR_ARG, "eppm_deint_y4m_open_read: NULL argument");
    return y4m_open("eppm_deint_y4m_open_read", out, path, h, w, f, fps_num, fps_den, interlace);
}

extern "C" int eppm_deint_default_params(eppm_deint_params* p)
{
    if (!p) return y4m_err(EPPM_ERR_ARG, "eppm_deint_default_params: NULL");
    p->thresh = 24;
    p->use_occ = 1;
    return EPPM_OK;
}

static uint32_t rgb_word(const uint8_t* rgb, size_t i) { return (uint32_t)rgb[3 * i] | (uint32_t)rgb[3 * i + 1] << 8 | (uint32_t)rgb[3 * i + 2] << 16; }
static void rgb_store(uint8_t* rgb, size_t i, uint32_t o) { rgb[3 * i] = (uint8_t)o; rgb[3 * i + 1] = (uint8_t)(o >> 8); rgb[3 * i + 2] = (uint8_t)(o >> 16); }

extern "C" int eppm_deint_step_host(const eppm_deint_params* p, uint8_t* rgb_out, uint8_t* mask_out, eppm_deint_stats* stats, const uint8_t* rgb_ref,
                                    const uint8_t* rgb_cur, const float* bu, const float* bv, const uint8_t* occ2, int h, int w, int parity, int cut)
{
    if (!p) return y4m_err(EPPM_ERR_ARG, "eppm_deint_step_host: NULL parameters");
    if (const char* why = eppm::deint_params_bad(p->thresh, p->use_occ)) return y4m_err(EPPM_ERR_ARG, "eppm_deint_step_host: %s", why);
    if (!rgb_out || !mask_out || !stats || !rgb_ref || !rgb_cur || !bu || !bv || !occ2) return y4m_err(EPPM_ERR_ARG, "eppm_deint_step_host: NULL argument");
    if (rgb_out == rgb_ref) return y4m_err(EPPM_ERR_ARG, "eppm_deint_step_host: the step gathers, rgb_out must not be rgb_ref");
    if (h < 2 || w < 1 || (long long)h * w >= (1LL << 31)) return y4m_err(EPPM_ERR_ARG, "eppm_deint_step_host: size %dx%d out of range (h >= 2)", w, h);
    if (parity != 0 && parity != 1) return y4m_err(EPPM_ERR_ARG, "eppm_deint_step_host: parity %d is not 0 or 1", parity);
    auto R = [&](int x, int y) { return rgb_word(rgb_ref, (size_t)y * w + x); };
    *stats = eppm_deint_stats{0, 0};
    for (int y = 0; y < h; y++)
        for (int x = 0; x < w; x++) {
            const size_t i = (size_t)y * w + x;
            if ((y & 1) == parity) {
                rgb_store(rgb_out, i, rgb_word(rgb_cur, i));
                mask_out[i] = 0;
                continue;
            }
            const uint32_t up = rgb_word(rgb_cur, (size_t)eppm::deint_row_up(y) * w + x), dn = rgb_word(rgb_cur, (size_t)eppm::deint_row_dn(y, h) * w + x);
            uint8_t m;
            rgb_store(rgb_out, i, eppm::deint_missing_pixel(x, y, up, dn, bu[i], bv[i], occ2[i], cut != 0, p->use_occ, p->thresh, h, w, R, &m));
            mask_out[i] = m;
            stats->temporal += m == 1;
            stats->spatial += m == 2;
        }
    return EPPM_OK;
}

extern "C" int eppm_deint_bob_host(uint8_t* rgb_out, const uint8_t* rgb_field, int h, int w, int parity)
{
    if (!rgb_out || !rgb_field) return y4m_err(EPPM_ERR_ARG, "eppm_deint_bob_host: NULL argument");
    if (h < 2 || w < 1 || (long long)h * w >= (1LL << 31)) return y4m_err(EPPM_ERR_ARG, "eppm_deint_bob_host: size %dx%d out of range (h >= 2)", w, h);
    if (parity != 0 && parity != 1) return y4m_err(EPPM_ERR_ARG, "eppm_deint_bob_host: parity %d is not 0 or 1", parity);
    auto F = [&](int x, int i) { return rgb_word(rgb_field, (size_t)i * w + x); };
    for (int y = 0; y < h; y++)
        for (int x = 0; x < w; x++) rgb_store(rgb_out, (size_t)y * w + x, eppm::deint_bob_pixel(x, y, parity, h, F));
    return EPPM_OK;
}
