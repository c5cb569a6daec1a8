// Device helpers and table records of the loader's pixel and label stages that more than one translation unit uses (augment.hip: whole
// source images; scene.hip: windows of full-size scenes; copypaste.hip: pasted objects).  Moved here unchanged: the files compile the same arithmetic.
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

// One destination pixel (x, y) of cv::warpPerspective with INTER_LINEAR and a constant border: m = the INVERSE map as 9 doubles, sb the
// SH x SW source, d the 3 bytes of the result.  warp_perspective_kernel (augment.hip) and paste_pixels_kernel (copypaste.hip) are this.
__device__ __forceinline__ void warp_bilinear_px(const uint8_t* __restrict__ sb, int SH, int SW, const double* __restrict__ m, int x, int y, int border,
                                                 uint8_t* __restrict__ d)
{
    // cv::warpPerspective: W = M20 x + M21 y + M22; fX = (M00 x + M01 y + M02) / W scaled by INTER_TAB_SIZE = 32 and rounded
    // (saturate_cast<int> of a double = cvRound: round half to even)
    double W = m[6] * x + m[7] * y + m[8];
    W = W ? 32.0 / W : 0.0;
    const double fX = fmax((double)INT_MIN, fmin((double)INT_MAX, (m[0] * x + m[1] * y + m[2]) * W));
    const double fY = fmax((double)INT_MIN, fmin((double)INT_MAX, (m[3] * x + m[4] * y + m[5]) * W));
    const int X = (int)rint(fX), Y = (int)rint(fY);
    const int sx = X >> 5, sy = Y >> 5, ax = X & 31, ay = Y & 31;
    // bilinear weights: OpenCV's table holds (1 - a/32, a/32) products scaled by 2^15 and rounded, corrected so the four sum to 2^15
    const float fx1 = ax * (1.f / 32.f), fy1 = ay * (1.f / 32.f);
    const float wf[4] = {(1.f - fy1) * (1.f - fx1), (1.f - fy1) * fx1, fy1 * (1.f - fx1), fy1 * fx1};
    int w[4], sum = 0, imax = 0, imin = 0;
    for (int k = 0; k < 4; k++) {
        w[k] = (int)rintf(wf[k] * 32768.f);
        sum += w[k];
        if (w[k] > w[imax]) imax = k;
        if (w[k] < w[imin]) imin = k;
    }
    // (initInterTab2D: the rounding error of the sum is pushed into the largest / smallest weight)
    if (sum != 32768) {
        const int diff = sum - 32768;
        if (diff < 0) w[imax] -= diff; else w[imin] -= diff;
    }
    if (sx >= 0 && sx + 1 < SW && sy >= 0 && sy + 1 < SH && (int64_t)(sy + 1) * SW + sx + 3 <= (int64_t)SH * SW) {
        // all four taps inside the image (and 8 readable bytes behind the lower pair): the same integer sums from two 8-byte loads
        const unsigned long long r0 = load_px2(sb + ((int64_t)sy * SW + sx) * 3), r1 = load_px2(sb + ((int64_t)(sy + 1) * SW + sx) * 3);
#pragma unroll
        for (int c = 0; c < 3; c++) {
            const int acc = px2_byte(r0, c) * w[0] + px2_byte(r0, c + 3) * w[1] + px2_byte(r1, c) * w[2] + px2_byte(r1, c + 3) * w[3];
            d[c] = (uint8_t)((acc + (1 << 14)) >> 15);
        }
        return;
    }
    for (int c = 0; c < 3; c++) {
        int acc = 0;
        for (int k = 0; k < 4; k++) {
            const int px = sx + (k & 1), py = sy + (k >> 1);
            const int v = ((unsigned)px < (unsigned)SW && (unsigned)py < (unsigned)SH) ? sb[((int64_t)py * SW + px) * 3 + c] : border;
            acc += v * w[k];
        }
        d[c] = (uint8_t)((acc + (1 << 14)) >> 15);
    }
}

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

// twice the signed area of the polygon (x[k], y[k]), k < n (scene.hip: a label quad clipped to its window; copypaste.hip: a destination quad
// and the part of a row that a pasted item covers)
__device__ __forceinline__ double shoelace(const double* x, const double* y, int n)
{
    double s = 0.0;
    for (int k = 0; k < n; k++) {
        const int j = k + 1 == n ? 0 : k + 1;
        s += x[k] * y[j] - x[j] * y[k];
    }
    return s;
}
