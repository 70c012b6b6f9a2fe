// objects.h -- the semantics of moving-object detection: labelled connected components of the stabiliser's motion
// mask, one integer record per object, the carry of the labels to image 2 and the identity rule that makes an id survive from one pair
// to the next.  The kernels (k_objects.hip) and the host forms (objects.cpp) share the per-pixel functions; the host forms themselves
// (obj_label_host, obj_carry_host, obj_assign_host: plain sequential code) live here too, so that a program without HIP can run them.
// Everything is integer arithmetic apart from the comparisons of a vector and its quantisation, which are single float32 operations:
// there is no summation order to care about, and the kernels equal the host forms bit for bit.  Builds without HIP.
#pragma once

#include <string.h>
#include <vector>

#include "cmap.h"

namespace eppm {

constexpr int kObjTileW = 64, kObjTileH = 16;      // a labelling tile: k_gmotion_accumulate's shape
constexpr int kObjChunk = 1024;                    // consecutive linear indices numbered by one block
constexpr int kObjMaxObjects = 255;                // a label is a byte
constexpr int kObjTable = 256;                     // entries of a slot's prev_id / prev_age tables (entry 0 is unused)
constexpr int kObjMaxDim = 8192;                   // section 16's bounds: w, h <= 8192 and h*w <= 2^26
constexpr long long kObjMaxPixels = 1LL << 26;
constexpr int32_t kObjMaxNextId = 1 << 30;         // next_id beyond this is refused by set_state; a step that passes it starts again at 1
constexpr uint32_t kObjBackground = 0xffffffffu;   // the parent / root word of a background pixel

// one object.  The layout of eppm_object (include/eppm.h): 64 bytes
struct ObjRecord {
    int32_t id, age, area;
    int32_t x0, y0, x1, y1;            // inclusive bounding box
    int32_t n_flow;                    // pixels of the object whose forward vector is valid
    int64_t sum_x, sum_y;              // over the object's pixels
    int64_t sum_qu, sum_qv;            // over the n_flow pixels: the vector in 1/256 px
};

struct ObjCounts {
    int32_t n, n_found, n_components, next_id;
};

EPPM_HD inline bool obj_size_ok(int h, int w) { return h >= 1 && w >= 1 && h <= kObjMaxDim && w <= kObjMaxDim && (long long)h * w <= kObjMaxPixels; }

EPPM_HD inline bool obj_params_ok(int connectivity, int min_area, int max_objects, int min_overlap)
{
    return (connectivity == 4 || connectivity == 8) && min_area >= 1 && max_objects >= 1 && max_objects <= kObjMaxObjects && min_overlap >= 1;
}

// foreground: the stabiliser's "moves on its own"; 0, 2 and every other byte are background
EPPM_HD inline bool obj_foreground(uint8_t mask) { return mask == 1; }

// gmotion.h's validity test without the mask term, and its quantisation (1/256 px; exact product, rintf rounds half to even; |q| <= 2^21)
EPPM_HD inline bool obj_flow_ok(float u, float v) { return fb_known(u, v) && fabsf(u) <= 8192.0f && fabsf(v) <= 8192.0f; }
EPPM_HD inline int obj_quant(float u) { return (int)rintf(u * 256.0f); }

EPPM_HD inline void obj_record_clear(ObjRecord* r)
{
    r->id = r->age = r->area = 0;
    r->x0 = r->y0 = 0x7fffffff;
    r->x1 = r->y1 = -1;
    r->n_flow = 0;
    r->sum_x = r->sum_y = r->sum_qu = r->sum_qv = 0;
}

// The carried label of pixel (x, y) of image 2: the label of the pixel of image 1 nearest to where the backward vector (fx, fy) points, 0
// if the pixel is occluded (o != 0), the vector unknown or its end outside the frame (NaN too).  L(x, y): the label at an in-frame pixel;
// q inside [0, w-1] x [0, h-1] keeps floorf(q + 0.5f) inside the frame, so nothing outside the plane is read whatever the inputs hold.
template <class Lab>
EPPM_HD inline uint8_t obj_carry_pixel(int x, int y, float fx, float fy, uint8_t o, int h, int w, const Lab& L)
{
    if (o != 0 || !fb_known(fx, fy)) return 0;
    const float qx = (float)x + fx, qy = (float)y + fy;
    if (!cmap_in_frame(qx, qy, h, w)) return 0;
    return L((int)floorf(qx + 0.5f), (int)floorf(qy + 0.5f));
}

// a carried byte as the vote table reads it: an index beyond max_objects (only a loaded state can hold one) counts as none
EPPM_HD inline int obj_carried(uint8_t p, int max_objects) { return (int)p <= max_objects ? (int)p : 0; }

// next_id after a step: beyond kObjMaxNextId the count starts again
EPPM_HD inline int32_t obj_next_wrap(int32_t next) { return next > kObjMaxNextId ? 1 : next; }

// ---- host forms: plain sequential code ----

// Labelling by a queue flood fill in raster order: the first pixel of a component that the scan meets is its root (its smallest linear
// index), so components are found in increasing order of root.  labels: h*w bytes out; rec: max_objects records out (ids and ages 0);
// cnt: n, n_found, n_components (next_id is left alone).
inline void obj_label_host(const uint8_t* mask, const float* u, const float* v, int h, int w, int connectivity, int min_area, int max_objects,
                           uint8_t* labels, ObjRecord* rec, ObjCounts* cnt)
{
    const size_t px = (size_t)h * w;
    std::vector<uint8_t> seen(px, 0);
    std::vector<int32_t> queue(px);
    memset(labels, 0, px);
    for (int k = 0; k < max_objects; k++) obj_record_clear(&rec[k]);
    cnt->n = cnt->n_found = cnt->n_components = 0;
    static const int dx[8] = {1, -1, 0, 0, 1, -1, 1, -1}, dy[8] = {0, 0, 1, -1, 1, 1, -1, -1};
    for (size_t i = 0; i < px; i++) {
        if (seen[i] || !obj_foreground(mask[i])) continue;
        size_t head = 0, tail = 0;
        queue[tail++] = (int32_t)i;
        seen[i] = 1;
        while (head < tail) {
            const int32_t j = queue[head++];
            const int x = j % w, y = j / w;
            for (int k = 0; k < connectivity; k++) {
                const int nx = x + dx[k], ny = y + dy[k];
                if (nx < 0 || nx >= w || ny < 0 || ny >= h) continue;
                const size_t n = (size_t)ny * w + nx;
                if (seen[n] || !obj_foreground(mask[n])) continue;
                seen[n] = 1;
                queue[tail++] = (int32_t)n;
            }
        }
        cnt->n_components++;
        if (tail < (size_t)min_area) continue;
        cnt->n_found++;
        if (cnt->n_found > max_objects) continue;
        ObjRecord* r = &rec[cnt->n_found - 1];
        r->area = (int32_t)tail;
        for (size_t q = 0; q < tail; q++) {
            const int32_t j = queue[q];
            const int x = j % w, y = j / w;
            labels[j] = (uint8_t)cnt->n_found;
            r->x0 = x < r->x0 ? x : r->x0; r->x1 = x > r->x1 ? x : r->x1;
            r->y0 = y < r->y0 ? y : r->y0; r->y1 = y > r->y1 ? y : r->y1;
            r->sum_x += x; r->sum_y += y;
            if (obj_flow_ok(u[j], v[j])) {
                r->n_flow++;
                r->sum_qu += obj_quant(u[j]); r->sum_qv += obj_quant(v[j]);
            }
        }
    }
    cnt->n = cnt->n_found < max_objects ? cnt->n_found : max_objects;
}

// the labels as the next pair's image 1 will see them
inline void obj_carry_host(const uint8_t* labels, const float* bu, const float* bv, const uint8_t* occ2, int h, int w, uint8_t* carried)
{
    auto L = [labels, w](int x, int y) { return labels[(size_t)y * w + x]; };
    for (int y = 0; y < h; y++)
        for (int x = 0; x < w; x++) {
            const size_t i = (size_t)y * w + x;
            carried[i] = obj_carry_pixel(x, y, bu[i], bv[i], occ2[i], h, w, L);
        }
}

// The identity rule.  labels: the new labels (1 .. n); carried: the slot's carried plane, or NULL for all zero; prev_id / prev_age:
// kObjTable entries each, read at the carried indices and rewritten for the new objects (entries beyond n: 0); next_id: in and out;
// rec: n records, whose id and age are set.
inline void obj_assign_host(const uint8_t* labels, const uint8_t* carried, size_t px, int n, int max_objects, int min_overlap, int32_t* prev_id,
                            int32_t* prev_age, int32_t* next_id, ObjRecord* rec)
{
    const int S = max_objects + 1;
    std::vector<uint32_t> V((size_t)S * S, 0);
    if (carried)
        for (size_t i = 0; i < px; i++) {
            const int c = labels[i], p = obj_carried(carried[i], max_objects);
            if (c >= 1 && c <= n && p >= 1) V[(size_t)c * S + p]++;
        }
    std::vector<int> best(S, 0), winner(S, 0);
    std::vector<uint32_t> bestv(S, 0);
    for (int c = 1; c <= n; c++)
        for (int p = 1; p <= max_objects; p++)
            if (V[(size_t)c * S + p] > bestv[c]) bestv[c] = V[(size_t)c * S + p], best[c] = p;       // ties to the lower p
    for (int p = 1; p <= max_objects; p++) {
        uint32_t wv = 0;
        for (int c = 1; c <= n; c++)
            if (best[c] == p && bestv[c] > wv) wv = bestv[c], winner[p] = c;                          // ties to the lower c
    }
    int32_t next = *next_id;
    int32_t id[kObjTable] = {}, age[kObjTable] = {};
    for (int c = 1; c <= n; c++) {
        const int p = best[c];
        if (p && winner[p] == c && bestv[c] >= (uint32_t)min_overlap) id[c] = prev_id[p], age[c] = prev_age[p] + 1;
        else id[c] = next++, age[c] = 0;
        rec[c - 1].id = id[c];
        rec[c - 1].age = age[c];
    }
    for (int k = 0; k < kObjTable; k++) prev_id[k] = id[k], prev_age[k] = age[k];
    *next_id = obj_next_wrap(next);
}

}  // namespace eppm
