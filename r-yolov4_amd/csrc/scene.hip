// Training on full-size labelled scenes (datasets/scene_dataset.py): the first stage of the batch assembler when a sample's source image
// is a WINDOW of a scene held in the image pool instead of a whole pool image.  The reference trains on windows cut offline by an external
// devkit (data/DOTA.yaml: data/DOTA/split/train) and has no code for this; the semantics are this project's, pinned by tests/scene_ref.py.
//   resize_hsv_windows   ryolo_resize_hsv_batch (augment.hip) reading its source through a window: bit-identical to cutting the c x c window
//                        first (114 wherever it lies outside the scene) and resizing the cut, without the pass that writes and re-reads the cut;
//                        interp 3, the rotated cut: the result sampled from the scene through the item's affine map by warp_perspective's rule;
//   scene_label_rows     which of the scene's labels belong to a window: shift by the window origin, intersection-over-foreground of the
//                        quad with the window (Sutherland-Hodgman in fp64), rows below the threshold become NaN rows, which
//                        label_stage_kernel carries and ryolo_encode_labels removes in order.
// Built with -ffp-contract=off like augment.hip: the float sums of the area resize and the fp64 clip are compared bit for bit.
#include "common.h"
#include "augment_px.h"
// (WindowItem, the record of ryolo_resize_hsv_windows' table, and LabelRow: include/ryolo_params.h)

#define SCENE_FILL 114

// one channel of pixel (vy, vx) of the virtual cut
__device__ __forceinline__ int cut_tap(const uint8_t* __restrict__ scene, const WindowItem& it, int vy, int vx, int ch)
{
    const int sy = it.y0 + vy, sx = it.x0 + vx;
    return ((unsigned)sy < (unsigned)it.SH && (unsigned)sx < (unsigned)it.SW) ? (int)scene[((int64_t)sy * it.SW + sx) * 3 + ch] : SCENE_FILL;
}

typedef uint32_t scene_u32x4 __attribute__((ext_vector_type(4)));
typedef scene_u32x4 scene_u32x4_a4 __attribute__((aligned(4)));        // a dwordx4 access needs dword alignment only

#define SCENE_COPY_PX 16         // pixels per thread on the copy path: 48 bytes = three 16-byte stores

// ---- rotated cut (interp 3): every pixel of the NH x NW result is warp_bilinear_px of the scene under the item's affine map, what
// warp_perspective_kernel computes with Minv = {minv, 0, 0, 1}.  The workgroup walks 64 x 16 tiles of the result (16 x 16 threads of 4 adjacent
// pixels), so that the source footprint of a turn is a compact rotated rectangle; a thread's 12 bytes go out as three dwords when they start
// on a dword (dst 4-byte aligned and y NW + x a multiple of 4: every row when NW is one), byte by byte otherwise.  Inlined: the kernel
// keeps its 72 VGPRs and stays without scratch (as a call it took 98 and 112 bytes of scratch per lane); the map's six doubles sit in SGPRs.
#define SCENE_ROT_TW 64
#define SCENE_ROT_TH 16
__device__ __forceinline__ void rot_cut_item(const uint8_t* __restrict__ scene, const WindowItem& it, uint8_t* __restrict__ dst, bool hsv,
                                             const uint8_t* slut, const int* divtab)
{
    const double m[9] = {it.minv[0], it.minv[1], it.minv[2], it.minv[3], it.minv[4], it.minv[5], 0.0, 0.0, 1.0};
    const int NH = it.NH, NW = it.NW;
    const unsigned tiles_x = ((unsigned)NW + SCENE_ROT_TW - 1) / SCENE_ROT_TW, tiles_y = ((unsigned)NH + SCENE_ROT_TH - 1) / SCENE_ROT_TH;
    const unsigned ntiles = tiles_x * tiles_y;
    const int tx = (threadIdx.x & 15) * 4, ty = threadIdx.x >> 4;
    const bool dst_al = (((uintptr_t)dst) & 3) == 0;
    for (unsigned tile = blockIdx.x; tile < ntiles; tile += gridDim.x) {
        const unsigned tyi = tile / tiles_x;
        const int y = (int)tyi * SCENE_ROT_TH + ty, x = (int)(tile - tyi * tiles_x) * SCENE_ROT_TW + tx;
        if (y >= NH || x >= NW) continue;
        const int n = min(4, NW - x);
        uint32_t w[3] = {0u, 0u, 0u};
#pragma unroll
        for (int k = 0; k < 4; k++) {
            if (k < n) {
                uint8_t d[3];
                warp_bilinear_px(scene, it.SH, it.SW, m, x + k, y, SCENE_FILL, d);
                int px[3] = {d[0], d[1], d[2]};
                if (hsv) hsv_lut_pixel(px[0], px[1], px[2], slut, divtab);
#pragma unroll
                for (int ch = 0; ch < 3; ch++) { const int j = 3 * k + ch; w[j >> 2] |= (uint32_t)px[ch] << (8 * (j & 3)); }
            }
        }
        const int64_t p0 = (int64_t)y * NW + x;
        uint8_t* o = dst + p0 * 3;
        if (dst_al && n == 4 && (p0 & 3) == 0) {
            uint32_t* ov = reinterpret_cast<uint32_t*>(o);
            ov[0] = w[0]; ov[1] = w[1]; ov[2] = w[2];
        } else {
#pragma unroll
            for (int j = 0; j < 12; j++)
                if (j < 3 * n) o[j] = (uint8_t)((w[j >> 2] >> (8 * (j & 3))) & 255u);
        }
    }
}

__global__ __launch_bounds__(256) void resize_hsv_windows_kernel(const uint8_t* __restrict__ pool, const WindowItem* __restrict__ items,
                                                                 const uint8_t* __restrict__ luts, uint8_t* __restrict__ stage)
{
    const WindowItem it = items[blockIdx.y];
    __shared__ int divtab[512];
    __shared__ uint8_t slut[768];
    if (it.lut >= 0) {                                              // (block-uniform) the set-up of resize_hsv_batch_kernel
        const int t = threadIdx.x;
        divtab[t] = t ? (int)rint((255 << 12) / (double)t) : 0;
        divtab[256 + t] = t ? (int)rint((180 << 12) / (6.0 * t)) : 0;
        for (int k = t; k < 768; k += 256) slut[k] = luts[(int64_t)it.lut * 768 + k];
        __syncthreads();
    }
    const unsigned npix = (unsigned)it.NH * (unsigned)it.NW;
    const uint8_t* scene = pool + it.src_off;
    uint8_t* dst = stage + it.dst_off;
    const int64_t scene_bytes = (int64_t)it.SH * it.SW * 3;

    if (it.interp == 3) {                                           // (block-uniform, like the branches below)
        rot_cut_item(scene, it, dst, it.lut >= 0, slut, divtab);
        return;
    }

    if (it.interp == 2) {
        // ---- copy (window == network size: every source use of a rates=(1.0,) dataset).  A thread owns 16 consecutive pixels of the result,
        // 48 bytes at a 16-byte aligned address.  When they lie in one row of the window and inside the scene, their source is 48
        // contiguous bytes at an arbitrary address 3 (y SW + x0 + x): 13 ALIGNED dwords are loaded and shifted into place in registers.
        // The 13 dwords must end at or before the scene's last byte; the chunks for which they do not (the scene's last pixels), the ones
        // that straddle a row end or a scene border, and a pool or staging address off its alignment take the byte path.
        const bool src_al = (((uintptr_t)scene) & 3) == 0, dst_al = (((uintptr_t)dst) & 15) == 0;
        const unsigned nunits = (npix + SCENE_COPY_PX - 1) / SCENE_COPY_PX;
        for (unsigned u = blockIdx.x * 256u + threadIdx.x; u < nunits; u += gridDim.x * 256u) {
            const unsigned p0 = u * SCENE_COPY_PX;
            const int n = (int)min((unsigned)SCENE_COPY_PX, npix - p0);
            const int y = (int)(p0 / (unsigned)it.NW), x = (int)(p0 - (unsigned)y * (unsigned)it.NW);
            const int sy = it.y0 + y, sx = it.x0 + x;
            uint32_t w[12];
            bool wide = src_al && n == SCENE_COPY_PX && x + SCENE_COPY_PX <= it.NW && (unsigned)sy < (unsigned)it.SH && sx >= 0 &&
                        sx + SCENE_COPY_PX <= it.SW;
            if (wide) {
                const int64_t b = ((int64_t)sy * it.SW + sx) * 3;
                const int m = (int)(b & 3);
                const int64_t a = b - m;
                if (a + 52 <= scene_bytes) {
                    uint32_t r[13];
                    const scene_u32x4_a4* q = reinterpret_cast<const scene_u32x4_a4*>(scene + a);
#pragma unroll
                    for (int k = 0; k < 3; k++) {
                        const scene_u32x4 v = q[k];
                        r[4 * k] = v.x; r[4 * k + 1] = v.y; r[4 * k + 2] = v.z; r[4 * k + 3] = v.w;
                    }
                    r[12] = *reinterpret_cast<const uint32_t*>(scene + a + 48);
                    const int sh = 8 * m;
#pragma unroll
                    for (int k = 0; k < 12; k++) w[k] = (uint32_t)(((((uint64_t)r[k + 1]) << 32) | (uint64_t)r[k]) >> sh);
                } else {
                    wide = false;
                }
            }
            if (!wide) {
#pragma unroll
                for (int k = 0; k < 12; k++) w[k] = 0u;
#pragma unroll
                for (int k = 0; k < SCENE_COPY_PX; k++) {
                    if (k < n) {
                        int yy = y, xx = x + k;
                        while (xx >= it.NW) { xx -= it.NW; yy++; }          // (n == 16 chunks cross at most 16 / NW row ends)
#pragma unroll
                        for (int ch = 0; ch < 3; ch++) {
                            const int j = 3 * k + ch;
                            w[j >> 2] |= (uint32_t)cut_tap(scene, it, yy, xx, ch) << (8 * (j & 3));
                        }
                    }
                }
            }
            if (it.lut >= 0) {
#pragma unroll
                for (int k = 0; k < SCENE_COPY_PX; k++) {
                    int px[3];
#pragma unroll
                    for (int ch = 0; ch < 3; ch++) { const int j = 3 * k + ch; px[ch] = (int)((w[j >> 2] >> (8 * (j & 3))) & 255u); }
                    hsv_lut_pixel(px[0], px[1], px[2], slut, divtab);
#pragma unroll
                    for (int ch = 0; ch < 3; ch++) {
                        const int j = 3 * k + ch;
                        w[j >> 2] = (w[j >> 2] & ~(255u << (8 * (j & 3)))) | ((uint32_t)px[ch] << (8 * (j & 3)));
                    }
                }
            }
            uint8_t* d = dst + (int64_t)p0 * 3;
            if (dst_al && n == SCENE_COPY_PX) {
                scene_u32x4* dv = reinterpret_cast<scene_u32x4*>(d);
#pragma unroll
                for (int k = 0; k < 3; k++) { scene_u32x4 v; v.x = w[4 * k]; v.y = w[4 * k + 1]; v.z = w[4 * k + 2]; v.w = w[4 * k + 3]; dv[k] = v; }
            } else {
#pragma unroll
                for (int j = 0; j < 3 * SCENE_COPY_PX; j++)
                    if (j < 3 * n) d[j] = (uint8_t)((w[j >> 2] >> (8 * (j & 3))) & 255u);
            }
        }
        return;
    }

    // ---- resize: the arithmetic of resize_hsv_batch_kernel on a source of size c x c whose taps are read through the window
    const int c = it.c;
    int fx = 0, fy = 0;
    area_fast_scales(c, c, it.NH, it.NW, fx, fy);
    if (it.interp == 0 && !(fx == 2 && fy == 2)) fx = fy = 0;
    for (unsigned i = blockIdx.x * 256u + threadIdx.x; i < npix; i += gridDim.x * 256u) {
        const int y = (int)(i / (unsigned)it.NW), x = (int)(i - (unsigned)y * (unsigned)it.NW);
        int px[3];
        if (fx) {
            // cv::resizeAreaFast_ (area_fast_pixel of augment.hip): integer block sum
            int sum[3] = {0, 0, 0};
            for (int r = 0; r < fy; r++)
                for (int q = 0; q < fx; q++)
                    for (int ch = 0; ch < 3; ch++) sum[ch] += cut_tap(scene, it, y * fy + r, x * fx + q, ch);
            if (fx == 2 && fy == 2) { for (int ch = 0; ch < 3; ch++) px[ch] = (sum[ch] + 2) >> 2; }
            else {
                const float scale = 1.f / (float)(fx * fy);
                for (int ch = 0; ch < 3; ch++) px[ch] = min(255, max(0, (int)rintf((float)sum[ch] * scale)));
            }
        } else if (it.interp == 0) {
            auto coef = [](int o, int dn, int sn, int& s0, int& a0, int& a1) {
                const double scale = (double)sn / (double)dn;
                float f = (float)((o + 0.5) * scale - 0.5);
                int si = (int)floorf(f);
                f -= (float)si;
                if (si < 0) { f = 0.f; si = 0; }
                if (si >= sn - 1) { f = 0.f; si = sn - 1; }
                s0 = si;
                a0 = (int)rintf((1.f - f) * 2048.f);
                a1 = (int)rintf(f * 2048.f);
            };
            int vx, ax0, ax1, vy, by0, by1;
            coef(x, it.NW, c, vx, ax0, ax1);
            coef(y, it.NH, c, vy, by0, by1);
            const int vx1 = min(vx + 1, c - 1), vy1 = min(vy + 1, c - 1);
            const int X = it.x0 + vx, Y0 = it.y0 + vy, Y1 = it.y0 + vy1;
            // both pairs inside the scene, and 8 readable bytes behind the lower one (the pair-load guard of resize_hsv_batch_kernel, on the scene)
            if (vx1 == vx + 1 && X >= 0 && X + 1 < it.SW && Y0 >= 0 && Y1 < it.SH && (int64_t)Y1 * it.SW + X + 3 <= (int64_t)it.SH * it.SW) {
                const unsigned long long q0 = load_px2(scene + ((int64_t)Y0 * it.SW + X) * 3), q1 = load_px2(scene + ((int64_t)Y1 * it.SW + X) * 3);
#pragma unroll
                for (int ch = 0; ch < 3; ch++) {
                    const int r0 = px2_byte(q0, ch) * ax0 + px2_byte(q0, ch + 3) * ax1;
                    const int r1 = px2_byte(q1, ch) * ax0 + px2_byte(q1, ch + 3) * ax1;
                    px[ch] = (((by0 * (r0 >> 4)) >> 16) + ((by1 * (r1 >> 4)) >> 16) + 2) >> 2;
                }
            } else
            for (int ch = 0; ch < 3; ch++) {
                const int r0 = cut_tap(scene, it, vy, vx, ch) * ax0 + cut_tap(scene, it, vy, vx1, ch) * ax1;
                const int r1 = cut_tap(scene, it, vy1, vx, ch) * ax0 + cut_tap(scene, it, vy1, vx1, ch) * ax1;
                px[ch] = (((by0 * (r0 >> 4)) >> 16) + ((by1 * (r1 >> 4)) >> 16) + 2) >> 2;
            }
        } else {
            const AreaAxis ax = area_axis(x, it.NW, c), ay = area_axis(y, it.NH, c);
            float acc[3] = {0.f, 0.f, 0.f};
            auto row = [&](int vy, float beta) {                  // same order of float operations as resize_hsv_batch_kernel's row()
                float rsum[3] = {0.f, 0.f, 0.f};
                if (ax.has_lo) for (int ch = 0; ch < 3; ch++) rsum[ch] += cut_tap(scene, it, vy, ax.lo - 1, ch) * ax.wlo;
                for (int vx = ax.lo; vx < ax.hi; vx++) for (int ch = 0; ch < 3; ch++) rsum[ch] += cut_tap(scene, it, vy, vx, ch) * ax.wmid;
                if (ax.has_hi) for (int ch = 0; ch < 3; ch++) rsum[ch] += cut_tap(scene, it, vy, ax.hi, ch) * ax.whi;
                for (int ch = 0; ch < 3; ch++) acc[ch] += beta * rsum[ch];
            };
            if (ay.has_lo) row(ay.lo - 1, ay.wlo);
            for (int vy = ay.lo; vy < ay.hi; vy++) row(vy, ay.wmid);
            if (ay.has_hi) row(ay.hi, ay.whi);
            for (int ch = 0; ch < 3; ch++) px[ch] = min(255, max(0, (int)rintf(acc[ch])));
        }
        if (it.lut >= 0) hsv_lut_pixel(px[0], px[1], px[2], slut, divtab);
        uint8_t* d = dst + (int64_t)i * 3;
        d[0] = (uint8_t)px[0]; d[1] = (uint8_t)px[1]; d[2] = (uint8_t)px[2];
    }
}

extern "C" int ryolo_window_item_bytes(int* bytes) { if (!bytes) return RY_ERR_ARG; *bytes = (int)sizeof(WindowItem); return RY_OK; }

extern "C" int ryolo_resize_hsv_windows(const uint8_t* pool, const void* items_dev, int nitems, int64_t max_pixels, const uint8_t* luts, uint8_t* stage,
                                        hipStream_t stream)
{
    if (nitems < 0 || max_pixels < 0) return RY_ERR_ARG;
    if (nitems == 0 || max_pixels == 0) return RY_OK;
    if (!pool || !items_dev || !stage || nitems > 65535 || max_pixels >= (1ll << 31)) return RY_ERR_ARG;
    const int64_t bx = ry_cdiv(max_pixels, 256 * 8);                // as ryolo_resize_hsv_batch; copy items run fewer turns of their loop
    hipLaunchKernelGGL(resize_hsv_windows_kernel, dim3((unsigned)(bx < 1024 ? bx : 1024), (unsigned)nitems), dim3(256), 0, stream, pool,
                       reinterpret_cast<const WindowItem*>(items_dev), luts, stage);
    RY_CHECK_LAUNCH();
    return RY_OK;
}

// ---- labels.  One plane of Sutherland-Hodgman on (x[], y[]): AXIS 0 = x, 1 = y; GE: keep coordinate >= bound, else <= bound.  A vertex on
// the bound is inside.  n -> at most n + n / 2 * 2 vertices in general (every crossing edge has one inside and one outside end), so a quad
// stays within 4 -> 6 -> 9 -> 13 -> 19 whatever its shape (a convex one within 8); SCENE_MAXV bounds the stores regardless.
#define SCENE_MAXV 20
template <int AXIS, bool GE>
__device__ __forceinline__ int clip_plane(const double* ix, const double* iy, int n, double bound, double* ox, double* oy)
{
    int m = 0;
    for (int k = 0; k < n; k++) {
        const int j = k + 1 == n ? 0 : k + 1;
        const double ak = AXIS ? iy[k] : ix[k], ao = AXIS ? ix[k] : iy[k];
        const double bk = AXIS ? iy[j] : ix[j], bo = AXIS ? ix[j] : iy[j];
        const bool ain = GE ? ak >= bound : ak <= bound, bin = GE ? bk >= bound : bk <= bound;
        if (ain && m < SCENE_MAXV) { ox[m] = ix[k]; oy[m] = iy[k]; m++; }
        if (ain != bin && m < SCENE_MAXV) {
            const double t = (bound - ak) / (bk - ak);
            const double o = ao + t * (bo - ao);
            ox[m] = AXIS ? o : bound;
            oy[m] = AXIS ? bound : o;
            m++;
        }
    }
    return m;
}

__global__ __launch_bounds__(256) void scene_label_rows_kernel(LabelRow* __restrict__ rows, int64_t n, const int* __restrict__ win_of_row,
                                                               const int* __restrict__ wins, int nwin, double thr, double* __restrict__ iof_out)
{
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    LabelRow* r = rows + i;
    const int wi = win_of_row[i];
    if ((unsigned)wi >= (unsigned)nwin) {                           // no such window: a dropped row, and `wins` is not read
        const float nanv = __int_as_float(0x7fc00000);
#pragma unroll
        for (int k = 0; k < 8; k++) r->poly[k] = nanv;
        if (iof_out) iof_out[i] = 0.0;
        return;
    }
    const int* wn = wins + (int64_t)wi * 3;
    const float ox = (float)wn[0], oy = (float)wn[1];
    const float cf = (float)wn[2];
    float q[8];
#pragma unroll
    for (int k = 0; k < 8; k += 2) { q[k] = r->poly[k] - ox; q[k + 1] = r->poly[k + 1] - oy; }
    double ax[SCENE_MAXV], ay[SCENE_MAXV], bx[SCENE_MAXV], by[SCENE_MAXV];
    for (int k = 0; k < 4; k++) { ax[k] = (double)q[2 * k]; ay[k] = (double)q[2 * k + 1]; }
    const double area = fabs(shoelace(ax, ay, 4));
    const double c = (double)wn[2];
    int m = clip_plane<0, true>(ax, ay, 4, 0.0, bx, by);
    m = clip_plane<0, false>(bx, by, m, c, ax, ay);
    m = clip_plane<1, true>(ax, ay, m, 0.0, bx, by);
    m = clip_plane<1, false>(bx, by, m, c, ax, ay);
    double iof = 0.0;
    bool keep = false;
    if (area > 0.0) {                                               // (false for NaN coordinates too)
        iof = fmin(1.0, fabs(shoelace(ax, ay, m)) / area);
        keep = iof >= thr;
    }
    if (iof_out) iof_out[i] = iof;
    const float nanv = __int_as_float(0x7fc00000);
#pragma unroll
    for (int k = 0; k < 8; k++) r->poly[k] = keep ? q[k] : nanv;
    r->w0 = cf;
    r->h0 = cf;
}

extern "C" int ryolo_scene_label_rows(void* rows_dev, int64_t nrows, const int32_t* win_of_row, const int32_t* wins, int nwin, double iof_thr,
                                      double* iof_out, hipStream_t stream)
{
    if (nrows < 0 || nwin < 0 || !(iof_thr > 0.0 && iof_thr <= 1.0)) return RY_ERR_ARG;
    if (nrows == 0) return RY_OK;
    if (!rows_dev || !win_of_row || !wins || nrows > (int64_t)0x7fffffff * 256) return RY_ERR_ARG;
    hipLaunchKernelGGL(scene_label_rows_kernel, dim3((unsigned)ry_cdiv(nrows, 256)), dim3(256), 0, stream, reinterpret_cast<LabelRow*>(rows_dev), nrows,
                       win_of_row, wins, nwin, iof_thr, iof_out);
    RY_CHECK_LAUNCH();
    return RY_OK;
}
