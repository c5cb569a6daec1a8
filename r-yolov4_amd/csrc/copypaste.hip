// Object-level copy-paste for scene training (datasets/copy_paste.py): labelled objects taken out of the scenes that are resident for the
// batch, rotated and scaled, dropped onto the assembler's finished uint8 canvases before ryolo_to_tensor, with their labels appended and the
// labels they bury removed.  The reference has no such stage; the semantics are this project's, pinned by tests/copy_paste_ref.py.
//   paste_prepare   per item: destination quad = M . source quad (double, left to right, rounded to fp32) and its integer bounding box on
//                   the canvas;
//   paste_pixels    a grid over (item, 32 x 8 tile of its bounding box): a canvas pixel inside the item's quad, and inside no LATER item of
//                   the same slot, is sampled from the scene with ryolo_warp_perspective_u8's rule (warp_bilinear_px, border 114).  Work is
//                   proportional to the pasted area; every pixel is written at most once, so the result does not depend on scheduling;
//   paste_labels    one thread per output row: existing rows, then one row per item; a row of which a later-drawn item of its slot covers
//                   the share occ_thr or more (fp64 Sutherland-Hodgman against the item's four half-planes) becomes a NaN row, which
//                   ryolo_encode_labels removes in order.
// `first` [B + 1] groups the items by slot as ryolo_paste_rects_grouped's table does.  An item is VALID when 0 <= slot < B, first[slot] <= j <
// first[slot + 1] and its scene is not empty; it is LIVE when, in addition, its destination quad is finite and its shoelace sum is not zero.
// An item that is not live writes no pixel and buries no row; an item that is not valid gets the row (0, cls, NaN x 8).
// Built with -ffp-contract=off like scene.hip: the fp64 clip and the edge tests are compared bit for bit.
#include "common.h"
#include "augment_px.h"
// (PasteItem, the record of the item table: include/ryolo_params.h)

#define PASTE_FILL 114
#define PASTE_TW 32              // tile of the pixel kernel: 32 x 8 pixels, one per thread
#define PASTE_TH 8
#define PASTE_MAXV 20            // as SCENE_MAXV (scene.hip): the clip's vertex stores are bounded whatever the row's shape

// s . ((bx - ax)(py - ay) - (by - ay)(px - ax)): >= 0 on the inner side of edge a -> b of a quad whose shoelace sum has sign s
__device__ __forceinline__ double paste_edge(double ax, double ay, double bx, double by, double s, double px, double py)
{
    return s * ((bx - ax) * (py - ay) - (by - ay) * (px - ax));
}

// the destination quad of item k promoted to double and the sign of its shoelace sum; false: not finite or without area
__device__ __forceinline__ bool paste_quad(const float* __restrict__ dq, int k, double* qx, double* qy, double& sg)
{
    bool fin = true;
#pragma unroll
    for (int v = 0; v < 4; v++) {
        qx[v] = (double)dq[(int64_t)k * 8 + 2 * v];
        qy[v] = (double)dq[(int64_t)k * 8 + 2 * v + 1];
        fin = fin && isfinite(qx[v]) && isfinite(qy[v]);
    }
    const double s = shoelace(qx, qy, 4);
    sg = s > 0.0 ? 1.0 : -1.0;
    return fin && (s > 0.0 || s < 0.0);
}

__device__ __forceinline__ bool paste_inside(const double* qx, const double* qy, double sg, double px, double py)
{
    bool in = true;
#pragma unroll
    for (int e = 0; e < 4; e++) {
        const int f = (e + 1) & 3;
        in = in && paste_edge(qx[e], qy[e], qx[f], qy[f], sg, px, py) >= 0.0;
    }
    return in;
}

__device__ __forceinline__ bool paste_item_valid(const PasteItem* __restrict__ items, int j, int np, const int* __restrict__ first, int B)
{
    const int slot = items[j].slot;
    if ((unsigned)slot >= (unsigned)B) return false;
    return first[slot] <= j && j < first[slot + 1] && first[slot + 1] <= np && items[j].SH > 0 && items[j].SW > 0;
}

__global__ __launch_bounds__(256) void paste_prepare_kernel(const PasteItem* __restrict__ items, int np, const int* __restrict__ first, int B, int S,
                                                            float* __restrict__ dq, int32_t* __restrict__ bbox)
{
    const int j = blockIdx.x * 256 + threadIdx.x;
    if (j >= np) return;
    const PasteItem* it = items + j;
#pragma unroll
    for (int v = 0; v < 4; v++) {
        const double x = (double)it->quad[2 * v], y = (double)it->quad[2 * v + 1];
        dq[(int64_t)j * 8 + 2 * v] = (float)(it->M[0] * x + it->M[1] * y + it->M[2]);
        dq[(int64_t)j * 8 + 2 * v + 1] = (float)(it->M[3] * x + it->M[4] * y + it->M[5]);
    }
    double qx[4], qy[4], sg;
    const bool live = paste_quad(dq, j, qx, qy, sg) && paste_item_valid(items, j, np, first, B);
    int bb[4] = {0, 0, 0, 0};
    if (live) {
        double x0 = qx[0], x1 = qx[0], y0 = qy[0], y1 = qy[0];
#pragma unroll
        for (int v = 1; v < 4; v++) {
            x0 = fmin(x0, qx[v]); x1 = fmax(x1, qx[v]);
            y0 = fmin(y0, qy[v]); y1 = fmax(y1, qy[v]);
        }
        // pixels px with x0 <= px <= x1, clipped to the canvas; the clamp comes before the conversion to int
        const double Sd = (double)S;
        const int ix0 = (int)fmin(fmax(ceil(x0), 0.0), Sd), ix1 = (int)fmin(fmax(floor(x1) + 1.0, 0.0), Sd);
        const int iy0 = (int)fmin(fmax(ceil(y0), 0.0), Sd), iy1 = (int)fmin(fmax(floor(y1) + 1.0, 0.0), Sd);
        if (ix0 < ix1 && iy0 < iy1) { bb[0] = ix0; bb[1] = iy0; bb[2] = ix1; bb[3] = iy1; }
    }
#pragma unroll
    for (int k = 0; k < 4; k++) bbox[(int64_t)j * 4 + k] = bb[k];
}

__global__ __launch_bounds__(256) void paste_pixels_kernel(const uint8_t* __restrict__ pool, const PasteItem* __restrict__ items, int np, int j0,
                                                           const int* __restrict__ first, int B, const float* __restrict__ dq,
                                                           const int32_t* __restrict__ bbox, uint8_t* __restrict__ canvas, int S)
{
    const int j = j0 + (int)blockIdx.y;
    if (j >= np) return;
    const int x0 = bbox[(int64_t)j * 4], y0 = bbox[(int64_t)j * 4 + 1], x1 = bbox[(int64_t)j * 4 + 2], y1 = bbox[(int64_t)j * 4 + 3];
    // (an empty box: not live, or off the canvas; the bounds are checked again because they address memory)
    if (x0 < 0 || y0 < 0 || x1 > S || y1 > S || x0 >= x1 || y0 >= y1) return;
    if (!paste_item_valid(items, j, np, first, B)) return;
    const int slot = items[j].slot;
    const int hi = first[slot + 1];
    double qx[4], qy[4], sg;
    if (!paste_quad(dq, j, qx, qy, sg)) return;
    double m[9];
#pragma unroll
    for (int k = 0; k < 6; k++) m[k] = items[j].Minv[k];
    m[6] = 0.0; m[7] = 0.0; m[8] = 1.0;
    const int SH = items[j].SH, SW = items[j].SW;
    const uint8_t* scene = pool + items[j].src_off;
    const int tiles_x = (x1 - x0 + PASTE_TW - 1) / PASTE_TW, tiles_y = (y1 - y0 + PASTE_TH - 1) / PASTE_TH;
    const int ntiles = tiles_x * tiles_y;
    for (int t = blockIdx.x; t < ntiles; t += gridDim.x) {
        const int ty = t / tiles_x, tx = t - ty * tiles_x;
        const int px = x0 + tx * PASTE_TW + (int)(threadIdx.x & (PASTE_TW - 1)), py = y0 + ty * PASTE_TH + (int)(threadIdx.x / PASTE_TW);
        if (px >= x1 || py >= y1) continue;
        const double pxd = (double)px, pyd = (double)py;
        if (!paste_inside(qx, qy, sg, pxd, pyd)) continue;
        bool buried = false;                                        // a later item of the slot also contains the pixel: that item writes it
        for (int k = j + 1; k < hi; k++) {
            const int32_t* bk = bbox + (int64_t)k * 4;
            if (px < bk[0] || px >= bk[2] || py < bk[1] || py >= bk[3] || items[k].slot != slot) continue;
            double kx[4], ky[4], ks;
            if (paste_quad(dq, k, kx, ky, ks) && paste_inside(kx, ky, ks, pxd, pyd)) { buried = true; break; }
        }
        if (buried) continue;
        warp_bilinear_px(scene, SH, SW, m, px, py, PASTE_FILL, canvas + (((int64_t)slot * S + py) * S + px) * 3);
    }
}

// one half-plane of Sutherland-Hodgman: edge a -> b of a quad of sign s; a vertex on the line is inside; t = num / den as scene.hip's clip_plane
__device__ __forceinline__ int paste_clip_edge(const double* ix, const double* iy, int n, double ax, double ay, double bx, double by, double s,
                                               double* ox, double* oy)
{
    int m = 0;
    for (int k = 0; k < n; k++) {
        const int j = k + 1 == n ? 0 : k + 1;
        const double da = paste_edge(ax, ay, bx, by, s, ix[k], iy[k]), db = paste_edge(ax, ay, bx, by, s, ix[j], iy[j]);
        const bool ain = da >= 0.0, bin = db >= 0.0;
        if (ain && m < PASTE_MAXV) { ox[m] = ix[k]; oy[m] = iy[k]; m++; }
        if (ain != bin && m < PASTE_MAXV) {
            const double t = da / (da - db);
            ox[m] = ix[k] + t * (ix[j] - ix[k]);
            oy[m] = iy[k] + t * (iy[j] - iy[k]);
            m++;
        }
    }
    return m;
}

__global__ __launch_bounds__(256) void paste_labels_kernel(const float* __restrict__ tg, int64_t nt, const PasteItem* __restrict__ items, int np,
                                                           const int* __restrict__ first, int B, const float* __restrict__ dq, double occ_thr,
                                                           float* __restrict__ out)
{
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= nt + np) return;
    const float nanv = __int_as_float(0x7fc00000);
    float row[10];
    int slot = -1, lo = 0, hi = 0;
    if (i < nt) {
#pragma unroll
        for (int k = 0; k < 10; k++) row[k] = tg[i * 10 + k];
        if (row[0] >= 0.f && row[0] < (float)B) {                   // (false for NaN: such a row meets no item)
            slot = (int)row[0];
            lo = first[slot];
            hi = first[slot + 1];
        }
    } else {
        const int j = (int)(i - nt);
        row[1] = items[j].cls;
        if (!paste_item_valid(items, j, np, first, B)) {
            row[0] = 0.f;
#pragma unroll
            for (int k = 2; k < 10; k++) row[k] = nanv;
#pragma unroll
            for (int k = 0; k < 10; k++) out[i * 10 + k] = row[k];
            return;
        }
        slot = items[j].slot;
        row[0] = (float)slot;
#pragma unroll
        for (int k = 0; k < 8; k++) row[2 + k] = dq[(int64_t)j * 8 + k];
        lo = j + 1;
        hi = first[slot + 1];
    }
    lo = max(lo, 0);
    hi = min(hi, np);
    double ax[PASTE_MAXV], ay[PASTE_MAXV], bx[PASTE_MAXV], by[PASTE_MAXV];
    for (int k = 0; k < 4; k++) { ax[k] = (double)row[2 + 2 * k]; ay[k] = (double)row[3 + 2 * k]; }
    const double area = fabs(shoelace(ax, ay, 4));
    bool occluded = false;
    if (area > 0.0) {                                               // (false for NaN coordinates too: the row stays as it is)
        for (int k = lo; k < hi && !occluded; k++) {
            if (items[k].slot != slot || !paste_item_valid(items, k, np, first, B)) continue;
            double qx[4], qy[4], sg;
            if (!paste_quad(dq, k, qx, qy, sg)) continue;
            for (int v = 0; v < 4; v++) { ax[v] = (double)row[2 + 2 * v]; ay[v] = (double)row[3 + 2 * v]; }
            int m = paste_clip_edge(ax, ay, 4, qx[0], qy[0], qx[1], qy[1], sg, bx, by);
            m = paste_clip_edge(bx, by, m, qx[1], qy[1], qx[2], qy[2], sg, ax, ay);
            m = paste_clip_edge(ax, ay, m, qx[2], qy[2], qx[3], qy[3], sg, bx, by);
            m = paste_clip_edge(bx, by, m, qx[3], qy[3], qx[0], qy[0], sg, ax, ay);
            occluded = fabs(shoelace(ax, ay, m)) / area >= occ_thr;
        }
    }
#pragma unroll
    for (int k = 0; k < 10; k++) out[i * 10 + k] = (occluded && k >= 2) ? nanv : row[k];
}

extern "C" int ryolo_paste_item_bytes(int* bytes) { if (!bytes) return RY_ERR_ARG; *bytes = (int)sizeof(PasteItem); return RY_OK; }

extern "C" int ryolo_paste_prepare(const void* items_dev, int np, const int32_t* first_dev, int B, int S, float* dq, int32_t* bbox, hipStream_t stream)
{
    if (np < 0 || B < 0 || S <= 0) return RY_ERR_ARG;
    if (np == 0) return RY_OK;
    if (!items_dev || !first_dev || !dq || !bbox) return RY_ERR_ARG;
    hipLaunchKernelGGL(paste_prepare_kernel, dim3((unsigned)ry_cdiv(np, 256)), dim3(256), 0, stream, reinterpret_cast<const PasteItem*>(items_dev), np,
                       first_dev, B, S, dq, bbox);
    RY_CHECK_LAUNCH();
    return RY_OK;
}

extern "C" int ryolo_paste_pixels(const uint8_t* pool, const void* items_dev, int np, const int32_t* first_dev, int B, const float* dq,
                                  const int32_t* bbox, uint8_t* canvas, int S, int max_bw, int max_bh, hipStream_t stream)
{
    if (np < 0 || B < 0 || S <= 0) return RY_ERR_ARG;
    if (np == 0 || B == 0) return RY_OK;
    if (!pool || !items_dev || !first_dev || !dq || !bbox || !canvas) return RY_ERR_ARG;
    // max_bw x max_bh: the caller's bound on an item's bounding box (<= 0: the canvas).  It only sizes the grid: an item whose box needs more
    // tiles than the grid has walks them in a loop.
    const int bw = (max_bw <= 0 || max_bw > S) ? S : max_bw, bh = (max_bh <= 0 || max_bh > S) ? S : max_bh;
    const int64_t tiles = ry_cdiv(bw, PASTE_TW) * ry_cdiv(bh, PASTE_TH);
    const unsigned gx = (unsigned)(tiles < 65535 ? tiles : 65535);
    for (int j0 = 0; j0 < np; j0 += 65535) {
        const int cnt = np - j0 < 65535 ? np - j0 : 65535;
        hipLaunchKernelGGL(paste_pixels_kernel, dim3(gx, (unsigned)cnt), dim3(256), 0, stream, pool, reinterpret_cast<const PasteItem*>(items_dev), np,
                           j0, first_dev, B, dq, bbox, canvas, S);
    }
    RY_CHECK_LAUNCH();
    return RY_OK;
}

extern "C" int ryolo_paste_labels(const float* targets, int64_t nt, const void* items_dev, int np, const int32_t* first_dev, int B, const float* dq,
                                  double occ_thr, float* out, hipStream_t stream)
{
    if (nt < 0 || np < 0 || B < 0 || !(occ_thr > 0.0)) return RY_ERR_ARG;
    if (nt + np == 0) return RY_OK;
    if (!out || (nt && !targets) || (np && (!items_dev || !dq)) || !first_dev || nt + np > (int64_t)0x7fffffff * 256) return RY_ERR_ARG;
    hipLaunchKernelGGL(paste_labels_kernel, dim3((unsigned)ry_cdiv(nt + np, 256)), dim3(256), 0, stream, targets, nt,
                       reinterpret_cast<const PasteItem*>(items_dev), np, first_dev, B, dq, occ_thr, out);
    RY_CHECK_LAUNCH();
    return RY_OK;
}
