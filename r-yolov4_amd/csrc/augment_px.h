// Device helpers and table records of the loader's pixel and label stages that more than one translation unit uses (augment.hip: whole
// source images; scene.hip: windows of full-size scenes).  Moved here unchanged: both files compile the same arithmetic.
#pragma once
#include "common.h"

// Two horizontally adjacent BGR pixels (6 bytes) as ONE unaligned 8-byte load (hipcc emits a single global_load_dwordx2 for it on gfx950); the
// caller guarantees 8 readable bytes (pixel index + 3 <= pixels of the image).  Per-channel byte loads made the bilinear kernels request-bound:
// 12 loads per output pixel for 4 taps x 3 channels, now 2.
__device__ __forceinline__ unsigned long long load_px2(const uint8_t* p)
{
    unsigned long long v;
    __builtin_memcpy(&v, p, 8);
    return v;
}
__device__ __forceinline__ int px2_byte(unsigned long long v, int k) { return (int)((v >> (8 * k)) & 255ull); }

// cv::resize's whole-number test (`is_area_fast`, imgproc/src/resize.cpp): scale = 1 / ((double) dst / src) per axis, iscale = saturate_cast<int>
// (round half even); both |scale - iscale| < DBL_EPSILON.  INTER_AREA downscales by whole numbers take the integer block sum, and INTER_LINEAR
// at exactly 2 x 2 is switched to that path by OpenCV itself.  ix = iy = 0: generic path.
__device__ __forceinline__ void area_fast_scales(int SH, int SW, int NH, int NW, int& ix, int& iy)
{
    const double sx = 1.0 / ((double)NW / (double)SW), sy = 1.0 / ((double)NH / (double)SH);
    const int rx = (int)rint(sx), ry = (int)rint(sy);
    const bool fast = fabs(sx - rx) < 2.220446049250313e-16 && fabs(sy - ry) < 2.220446049250313e-16 && rx >= 1 && ry >= 1 && (rx > 1 || ry > 1);
    ix = fast ? rx : 0;
    iy = fast ? ry : 0;
}

// One row of ryolo_resize_hsv_batch's table (augment.hip): an SH x SW image of the pool -> NH x NW in the staging pool; interp 0 = INTER_LINEAR,
// 1 = INTER_AREA, 2 = copy; lut >= 0: index of this image's hsv tables.  scene.hip's WindowItem extends it by the window.
struct ResizeItem {
    int64_t src_off, dst_off;    // byte offsets into the source pool / the staging pool
    int SH, SW, NH, NW;
    int interp, lut;
};

// divtab (optional, LDS): [0..255] = OpenCV's sdiv_table, [256..511] = hdiv_table180 — the two double-precision divisions per pixel as table
// reads (what cv::cvtColor's 8-bit BGR2HSV does itself); same integers as the expressions below
__device__ __forceinline__ void hsv_lut_pixel(int& b, int& g, int& r, const uint8_t* __restrict__ lut, const int* divtab = nullptr)
{
    int v = max(b, max(g, r)), vmin = min(b, min(g, r));
    const int diff = v - vmin;
    const int vr = v == r ? -1 : 0, vg = v == g ? -1 : 0;
    const int sdiv = divtab ? divtab[v] : (v ? (int)rint((255 << 12) / (double)v) : 0);
    const int hdiv = divtab ? divtab[256 + diff] : (diff ? (int)rint((180 << 12) / (6.0 * diff)) : 0);
    const int s = (diff * sdiv + (1 << 11)) >> 12;
    int h = (vr & (g - b)) + (~vr & ((vg & (b - r + 2 * diff)) + ((~vg) & (r - g + 4 * diff))));
    h = (h * hdiv + (1 << 11)) >> 12;
    h += h < 0 ? 180 : 0;
    const int H = lut[h & 255], S = lut[256 + s], V = lut[512 + v];
    float hf = (float)H * (6.f / 180.f), sf = (float)S * (1.f / 255.f), vf = (float)V * (1.f / 255.f);
    float bb, gg, rr;
    if (sf == 0.f) {
        bb = gg = rr = vf;
    } else {
        static const int sector[6][3] = {{1, 3, 0}, {1, 0, 2}, {3, 0, 1}, {0, 2, 1}, {0, 1, 3}, {2, 1, 0}};
        if (hf < 0.f) { do hf += 6.f; while (hf < 0.f); }
        else if (hf >= 6.f) { do hf -= 6.f; while (hf >= 6.f); }
        const int sec = (int)floorf(hf);
        hf -= (float)sec;
        const int sc = (unsigned)sec >= 6u ? 0 : sec;
        if ((unsigned)sec >= 6u) hf = 0.f;
        float tab[4];
        tab[0] = vf;
        tab[1] = vf * (1.f - sf);
        tab[2] = vf * (1.f - sf * hf);
        tab[3] = vf * (1.f - sf * (1.f - hf));
        bb = tab[sector[sc][0]];
        gg = tab[sector[sc][1]];
        rr = tab[sector[sc][2]];
    }
    b = min(255, max(0, (int)rintf(bb * 255.f)));
    g = min(255, max(0, (int)rintf(gg * 255.f)));
    r = min(255, max(0, (int)rintf(rr * 255.f)));
}

// one axis of cv::computeResizeAreaTab for destination index d: source cells [s_lo, s_hi] with weights (first, 1/cell ..., last)
struct AreaAxis { int lo, hi; float wlo, wmid, whi; bool has_lo, has_hi; };
__device__ __forceinline__ AreaAxis area_axis(int d, int dn, int sn)
{
    const double scale = (double)sn / (double)dn;
    const double f1 = d * scale, f2 = f1 + scale;
    const double cell = fmin(scale, (double)sn - f1);
    int s1 = (int)ceil(f1), s2 = (int)floor(f2);
    s2 = min(s2, sn - 1);
    s1 = min(s1, s2);
    AreaAxis a;
    a.has_lo = s1 - f1 > 1e-3;
    a.wlo = (float)((s1 - f1) / cell);
    a.lo = s1;                                     // whole cells s1 .. s2 - 1; the leading partial cell is s1 - 1
    a.hi = s2;
    a.wmid = (float)(1.0 / cell);
    a.has_hi = f2 - s2 > 1e-3;
    a.whi = (float)(fmin(fmin(f2 - s2, 1.0), cell) / cell);
    return a;
}

struct LabelRow {
    float poly[8];               // as parsed from the label file
    float cls;
    int slot;                    // image slot of the batch (column 0 of the result)
    float w0, h0;                // original image size; 0: labels are already normalised (normalized_labels)
    float w1, h1;                // size after load_image's resize
    float bx1, bx2, by1, by2;    // `boarder` of load_target (source-image coordinates); bx2 < 0: no filter
    float padw, padh;
    float cx1, cx2, cy1, cy2;    // mosaic-9 crop window on the 3s canvas; cx2 < 0: none.  The origin (cx1, cy1) is subtracted afterwards
    int mat;                     // index into the warp matrices, -1: none
};
