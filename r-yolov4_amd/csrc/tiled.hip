// Full-scene (tiled) detection for gfx950: a scene far larger than the network input is cut into overlapping windows, every group of
// windows goes through the captured forward + post_process (Yolo.capture_inference(..., post=...)), and the per-window detections are
// merged back in scene coordinates with CLASS-WISE rotated NMS — all on the device, no host read between groups (lib/tiled.py).
//
//   tile_cut_views_kernel  uint8 HWC BGR scene (pool base + byte offset) -> the graph's static input fp32 [B,3,S,S] as RGB / 255, 114 / 255
//                        outside the scene, every window written in one of the eight flip / 90-degree views (view code per table row;
//                        the four transposing views turn a 32 x 32 pixel tile through LDS); one launch per group of entries.  View id is
//                        bit-identical to ryolo_paste_rects(fill=114) + ryolo_to_tensor (the chain it replaces) without their
//                        intermediate canvas.
//   tile_collect_views_kernel  dets [B,mk,7] / num [B] of a group -> candidate rows in scene coordinates (the view's inverse map of point
//                        and angle, then the shift) at the fixed slot entry * mk + j and the per-class key rows key [nc][ld] (score in
//                        the row of the box's class, -inf elsewhere); every slot of the group is written exactly once (no fill pass, no
//                        atomics: deterministic).
//   (ryolo_topk_desc over the nc key rows)
//   tile_gather_kernel   per-class top-K slots -> NMS boxes [nc,K,5] in scene pixels, theta in degrees, NO class offset: the per-image path
//                        separates classes by cls * 4096 px (lib/general.py:14), which collides on scenes wider than 4096 px; here a
//                        class is its own NMS batch row (ryolo_nms_rotated_batched with batch = nc).
//   tile_mark_kernel     kept entries -> final key [ld] by slot (the collect pass reset it to -inf)
//   tile_fuse_kernel     (fused merge, in place of tile_mark_kernel, after ryolo_nms_owner) a kept box absorbs the boxes it suppressed:
//                        score-weighted rotated box into fused [ld][7] and the fused score into the final key, both at the owner's slot
//   (ryolo_topk_desc over the final key: score desc, slot asc, capped at max_det)
//   tile_emit_kernel     out [max_det,7] = candidate (or fused) rows in that order, zero padded.
// Compiled with -ffp-contract=off: the coordinate mapping (x + x0) / rate is restated bit for bit by numpy in the tests.
#include "common.h"

__global__ __launch_bounds__(256) void tile_gather_kernel(const float* __restrict__ cand, const float* __restrict__ skey,
                                                          const int64_t* __restrict__ order, int64_t K, float* __restrict__ rboxes)
{
    const int64_t k = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    const int c = blockIdx.y;
    if (k >= K) return;
    const int64_t e = (int64_t)c * K + k;
    float* r = rboxes + e * 5;
    if (!(skey[e] > -INFINITY)) {
        for (int t = 0; t < 5; t++) r[t] = 0.f;
        return;
    }
    const float* p = cand + order[e] * 7;
    r[0] = p[0]; r[1] = p[1]; r[2] = p[2]; r[3] = p[3];
    r[4] = p[4] / 3.14159265358979323846f * 180.f;                     // pp_gather_kernel's rad -> deg
}

__global__ __launch_bounds__(256) void tile_mark_kernel(const float* __restrict__ skey, const int64_t* __restrict__ order,
                                                        const int64_t* __restrict__ keep, const int32_t* __restrict__ num_keep, int64_t K,
                                                        int64_t keep_stride, float* __restrict__ fkey)
{
    const int64_t j = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    const int c = blockIdx.y;
    if (j >= keep_stride || j >= (int64_t)num_keep[c]) return;
    const int64_t e = (int64_t)c * K + keep[(int64_t)c * keep_stride + j];
    fkey[order[e]] = skey[e];                                          // a slot belongs to one class row: no two threads share it
}

// Cluster fusion (include/ryolo.h states the arithmetic): one wave = one kept box k of class blockIdx.y.  The wave reads the class's
// owner row from position k + 1 to the end of the selection, 256 positions per step (four coalesced dword loads per lane in flight),
// and takes one ballot per 64: the set bits are the cluster's members in ascending position.  A member's lane loads its candidate row
// and computes everything that depends on the member and the owner only (the wrapped angle difference, the w / h swap, the five
// products with its score); the six running sums are then advanced member by member in bit order on wave-uniform values (readlane), so
// the order of the additions is the defined one whatever the cluster's size.  Lane 0 writes the fused row and the fused score at the
// owner's slot: every output once, no atomics, cand is only read.
__device__ __forceinline__ float tf_lane(float v, int l)
{
    return __builtin_bit_cast(float, __builtin_amdgcn_readlane(__builtin_bit_cast(int, v), l));
}

__global__ __launch_bounds__(256) void tile_fuse_kernel(const float* __restrict__ cand, const int64_t* __restrict__ order,
                                                        const int32_t* __restrict__ nsel, const int64_t* __restrict__ keep,
                                                        const int32_t* __restrict__ num_keep, const int32_t* __restrict__ owner, int64_t K,
                                                        int64_t keep_stride, int64_t ld, int wbf, int n_ens, float* __restrict__ fused,
                                                        float* __restrict__ fkey)
{
    const float PI = 3.14159265358979323846f, HALF_PI = 1.57079632679489661923f, QUARTER_PI = 0.78539816339744830962f;
    const int c = blockIdx.y, lane = threadIdx.x & 63;
    const int64_t j = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
    int64_t nk = num_keep[c];
    if (nk > keep_stride) nk = keep_stride;
    if (j >= nk) return;                                                // wave-uniform, like every exit below
    int64_t n = nsel[c];
    if (n > K) n = K;
    const int64_t k = keep[(int64_t)c * keep_stride + j];
    if (k < 0 || k >= n) return;
    const int64_t* ord = order + (int64_t)c * K;
    const int32_t* own = owner + (int64_t)c * K;
    const int64_t slot = ord[k];
    if (slot < 0 || slot >= ld) return;
    const float* rk = cand + slot * 7;
    const float xk = rk[0], yk = rk[1], wk = rk[2], hk = rk[3], tk = rk[4], sk = rk[5];
    float W = sk, ax = 0.f, ay = 0.f, aw = sk * wk, ah = sk * hk, ad = 0.f;
    int m = 1;
    for (int64_t base = k + 1; base < n; base += 256) {
        int32_t o[4];
#pragma unroll
        for (int u = 0; u < 4; u++) {
            const int64_t p = base + 64 * u + lane;
            o[u] = p < n ? own[p] : -1;
        }
#pragma unroll
        for (int u = 0; u < 4; u++) {
            const bool hit = o[u] == (int32_t)k;
            unsigned long long mm = __ballot(hit);
            if (!mm) continue;
            float ts = 0.f, tx = 0.f, ty = 0.f, tw = 0.f, th = 0.f, td = 0.f;
            if (hit) {
                const int64_t si = ord[base + 64 * u + lane];
                if (si >= 0 && si < ld) {
                    const float* r = cand + si * 7;
                    float d = r[4] - tk;
                    if (d >= HALF_PI) d = d - PI;
                    if (d < -HALF_PI) d = d + PI;
                    float wi = r[2], hi = r[3];
                    if (d > QUARTER_PI) { const float t = wi; wi = hi; hi = t; d = d - HALF_PI; }
                    else if (d < -QUARTER_PI) { const float t = wi; wi = hi; hi = t; d = d + HALF_PI; }
                    ts = r[5];
                    tx = ts * (r[0] - xk);
                    ty = ts * (r[1] - yk);
                    tw = ts * wi;
                    th = ts * hi;
                    td = ts * d;
                }
            }
            while (mm) {
                const int l = __builtin_ctzll(mm);
                mm &= mm - 1;
                W = W + tf_lane(ts, l);
                ax = ax + tf_lane(tx, l);
                ay = ay + tf_lane(ty, l);
                aw = aw + tf_lane(tw, l);
                ah = ah + tf_lane(th, l);
                ad = ad + tf_lane(td, l);
                m++;
            }
        }
    }
    if (lane != 0) return;
    float* o7 = fused + slot * 7;
    if (m == 1) {
        o7[0] = xk; o7[1] = yk; o7[2] = wk; o7[3] = hk; o7[4] = tk;     // a lone box: its row on the bits, theta unwrapped
    } else {
        float t = tk + ad / W;
        if (t >= HALF_PI) t = t - PI;
        if (t < -HALF_PI) t = t + PI;
        o7[0] = xk + ax / W; o7[1] = yk + ay / W; o7[2] = aw / W; o7[3] = ah / W; o7[4] = t;
    }
    const float s = wbf ? (W / (float)m) * ((float)(m < n_ens ? m : n_ens) / (float)n_ens) : sk;
    o7[5] = s;
    o7[6] = rk[6];
    fkey[slot] = s;
}

__global__ __launch_bounds__(256) void tile_emit_kernel(const float* __restrict__ cand, const int64_t* __restrict__ order,
                                                        const int32_t* __restrict__ num, int64_t max_det, float* __restrict__ out)
{
    const int64_t j = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (j >= max_det) return;
    float* o = out + j * 7;
    if (j < (int64_t)num[0]) {
        const float* p = cand + order[j] * 7;
        for (int t = 0; t < 7; t++) o[t] = p[t];
    } else {
        for (int t = 0; t < 7; t++) o[t] = 0.f;
    }
}

// ------------------------------------------------------------------------------------------ cut and collect, in a flip / 90-degree view
// View codes (include/ryolo.h): 0 id, 1 hflip, 2 vflip, 3 rot180, 4 transpose, 5 rot90, 6 rot270, 7 antitranspose.  With `win` the
// S x S window at the entry's origin (114 outside the scene: the fill turns with the window), view pixel (y, x) is
//   codes 0-3:  win[fy ? S-1-y : y][fx ? S-1-x : x]     fx = code & 1, fy = code & 2
//   codes 4-7:  win[fr ? S-1-x : x][fc ? S-1-y : y]     fc = code == 5 || code == 7, fr = code == 6 || code == 7
// window table rows (int64 [nwin][6]): byte offset of the window's source image from `pool`, its height, width, window origin x0, y0,
// view code
#define TV_ROW 6
#define TV_TILE 32
#define TV_PITCH 33

// 4 consecutive pixels of a window row as 12 BGR bytes packed in 3 dwords (byte n of the 12 = TV_BYTE(q, n)), 114 outside the H x W
// source
#define TV_BYTE(q, n) (((q)[(n) >> 2] >> (8 * ((n) & 3))) & 255u)
__device__ __forceinline__ void tv_load4(const uint8_t* __restrict__ src, int H, int W, int sy, int sx, uint32_t* q)
{
    if (sy < H && sx + 4 <= W) {
        __builtin_memcpy(q, src + ((int64_t)sy * W + sx) * 3, 12);
    } else {
        q[0] = q[1] = q[2] = 0x72727272u;                               // 114 in every byte
        if (sy < H) {
            const uint8_t* sp = src + ((int64_t)sy * W + sx) * 3;
#pragma unroll
            for (int n = 0; n < 12; n++)
                if (sx + n / 3 < W) q[n >> 2] = (q[n >> 2] & ~(255u << (8 * (n & 3)))) | (uint32_t)sp[n] << (8 * (n & 3));
        }
    }
}

// One block = one window (blockIdx.y) and 256 threads x 4 output pixels; every thread reads 12 contiguous source bytes along a source
// row and stores one float4 per colour plane along an output row, whatever the view.
//   codes 0-3: a linear mapping, one thread = 4 consecutive output pixels of one window row (a block = 1024 consecutive output
//     pixels; blocks past S * S / 4 groups, which only S % 32 != 0 leaves, exit).  A reversed row is read forward from the
//     mirrored column S - 4 - x (S % 4 == 0 keeps the 4-pixel groups aligned under the mirror) and reversed in registers.
//   codes 4-7: a block turns the 32 x 32 pixel tile blockIdx.x = ty * ceil(S / 32) + tx through LDS, one dword (B | G << 8 | R << 16) per
//     pixel at tile[i][j] (i = output x, j = output y inside the tile), row pitch TV_PITCH = 33 dwords.
//       in:  thread (i = tid / 8, jg = tid % 8) reads source row r(xt + i), 4 pixels, and writes tile[i][4 jg + k], k = 0..3, as ds_write_b32:
//            bank (33 i + 4 jg + k) % 32 = (i + 4 jg + k) % 32; a 32-lane half holds i = i0..i0+3, jg = 0..7 -> 32 distinct banks.
//       out: thread (j = tid / 8, ig = tid % 8) reads tile[4 ig + k][j] as ds_read_b32: bank (33 (4 ig + k) + j) % 32 = (4 ig + k + j) % 32;
//            a half holds j = j0..j0+3, ig = 0..7 -> 32 distinct banks.
//     Conflict count by the (a / 4) % 32 rule per 32-lane half: 0 extra cycles on both sides (pitch 32 would put the column read of a
//     half on 4 banks, 8-way).  Any pitch = 1 mod 8 does the same; 33 is the smallest above the tile.  (The compiler pairs the four
//     accesses of a thread into two ds_write2_b32 / ds_read2_b32, which bank per dword by the same rule.)
//     The grid has ceil(S / 32)^2 blocks per window, never fewer than the linear mapping needs; groups of 4 pixels past S (S % 32 != 0)
//     are neither loaded nor stored, and S % 4 == 0 makes a group wholly inside or wholly outside.
__global__ __launch_bounds__(256) void tile_cut_views_kernel(const uint8_t* __restrict__ pool, const int64_t* __restrict__ win, int S,
                                                             float* __restrict__ dst)
{
    __shared__ uint32_t tile[TV_TILE * TV_PITCH];
    const int w = blockIdx.y;
    const int64_t* t = win + (int64_t)w * TV_ROW;
    const uint8_t* src = pool + t[0];
    const int H = (int)t[1], W = (int)t[2], x0 = (int)t[3], y0 = (int)t[4], code = (int)t[5];
    const int64_t plane = (int64_t)S * S;
    float* out = dst + (int64_t)w * 3 * plane;
    if (code < 0 || code > 7) return;                                   // block-uniform: the slot stays untouched
    if (code < 4) {
        const int sq = S >> 2;
        const int64_t q = (int64_t)blockIdx.x * 256 + threadIdx.x;
        if (q >= (int64_t)S * sq) return;
        const int y = (int)(q / sq);
        const int x = (int)(q - (int64_t)y * sq) * 4;
        const bool fx = code & 1, fy = code & 2;
        uint32_t q12[3];
        tv_load4(src, H, W, y0 + (fy ? S - 1 - y : y), x0 + (fx ? S - 4 - x : x), q12);
        float* o = out + (int64_t)y * S + x;
#pragma unroll
        for (int c = 0; c < 3; c++) {                                   // BGR -> RGB, .float() / 255 (ryolo_to_tensor's expression)
            float v[4];
#pragma unroll
            for (int k = 0; k < 4; k++) v[k] = (float)TV_BYTE(q12, k * 3 + (2 - c)) / 255.0f;
            *reinterpret_cast<float4*>(o + c * plane) = fx ? make_float4(v[3], v[2], v[1], v[0]) : make_float4(v[0], v[1], v[2], v[3]);
        }
        return;
    }
    const int nt = (S + TV_TILE - 1) / TV_TILE;
    const int ty = blockIdx.x / nt, tx = blockIdx.x - ty * nt;          // blockIdx.x < nt * nt (the launch's grid)
    const int xt = tx * TV_TILE, yt = ty * TV_TILE;                     // the tile's origin in the output
    const bool fc = code == 5 || code == 7, fr = code == 6 || code == 7;
    const int a = threadIdx.x >> 3, bg = (threadIdx.x & 7) * 4;
    if (xt + a < S && yt + bg < S) {                                    // in: i = a, j = bg .. bg + 3
        const int x = xt + a, y = yt + bg;
        uint32_t q12[3];
        tv_load4(src, H, W, y0 + (fr ? S - 1 - x : x), x0 + (fc ? S - 4 - y : y), q12);
        uint32_t p[4];
#pragma unroll
        for (int k = 0; k < 4; k++) p[k] = TV_BYTE(q12, 3 * k) | TV_BYTE(q12, 3 * k + 1) << 8 | TV_BYTE(q12, 3 * k + 2) << 16;
#pragma unroll
        for (int k = 0; k < 4; k++) tile[a * TV_PITCH + bg + k] = fc ? p[3 - k] : p[k];     // a reversed row: reversed in registers
    }
    __syncthreads();
    if (yt + a < S && xt + bg < S) {                                    // out: j = a, i = bg .. bg + 3
        uint32_t p[4];
#pragma unroll
        for (int k = 0; k < 4; k++) p[k] = tile[(bg + k) * TV_PITCH + a];
        float* o = out + (int64_t)(yt + a) * S + xt + bg;
#pragma unroll
        for (int c = 0; c < 3; c++) {
            float v[4];
#pragma unroll
            for (int k = 0; k < 4; k++) v[k] = (float)((p[k] >> (8 * (2 - c))) & 255u) / 255.0f;
            *reinterpret_cast<float4*>(o + c * plane) = make_float4(v[0], v[1], v[2], v[3]);
        }
    }
}

// One thread = one detection slot j of entry b of the group (global entry win0 + b): the view's inverse map, then the shift to scene
// pixels (x + x0) / rate.  geom rows (x0, y0, rate, view code), S the window size.  The
// point map and the angle (fp32, one rounding per step; -theta is exact) follow include/ryolo.h; the six views that change theta wrap it
// once through norm_angle's two selects (lib/general.py:14-15).  An entry with an unknown code is written as an empty slot.
__global__ __launch_bounds__(256) void tile_collect_views_kernel(const float* __restrict__ dets, const int32_t* __restrict__ num, int64_t mk,
                                                                 const float* __restrict__ geom, int64_t win0, int64_t nwin, int nc,
                                                                 int64_t ld, float S, float* __restrict__ cand, float* __restrict__ key,
                                                                 float* __restrict__ fkey)
{
    const int64_t j = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    const int b = blockIdx.y;
    if (j >= mk) return;
    const int64_t wg = win0 + b;
    const int64_t slot = wg * mk + j;
    float* c = cand + slot * 7;
    float s = -INFINITY;
    int cls = -1;
    const float* g = geom + wg * 4;
    const int code = wg < nwin ? (int)g[3] : -1;
    if (code >= 0 && code <= 7 && j < (int64_t)num[b]) {
        const float* d = dets + ((int64_t)b * mk + j) * 7;
        const float x0 = g[0], y0 = g[1], rate = g[2];
        const float HALF_PI = 1.57079632679489661923f, PI = 3.14159265358979323846f;
        const float vx = d[0], vy = d[1], th = d[4];
        float px, py, t;
        switch (code) {
            case 0: px = vx; py = vy; t = th; break;
            case 1: px = S - vx; py = vy; t = -th; break;
            case 2: px = vx; py = S - vy; t = -th; break;
            case 3: px = S - vx; py = S - vy; t = th; break;
            case 4: px = vy; py = vx; t = HALF_PI - th; break;
            case 5: px = S - vy; py = vx; t = th + HALF_PI; break;
            case 6: px = vy; py = S - vx; t = th - HALF_PI; break;
            default: px = S - vy; py = S - vx; t = HALF_PI - th; break;
        }
        if (code != 0 && code != 3) {
            if (t >= HALF_PI) t = t - PI;
            if (t < -HALF_PI) t = t + PI;
        }
        c[0] = (px + x0) / rate;
        c[1] = (py + y0) / rate;
        c[2] = d[2] / rate;
        c[3] = d[3] / rate;
        c[4] = t; c[5] = d[5]; c[6] = d[6];
        s = d[5];
        cls = (int)d[6];
    } else {
        for (int k = 0; k < 7; k++) c[k] = 0.f;
    }
    for (int k = 0; k < nc; k++) key[(int64_t)k * ld + slot] = k == cls ? s : -INFINITY;
    fkey[slot] = -INFINITY;
}

extern "C" int ryolo_tile_cut_views(const uint8_t* pool, const int64_t* win, int64_t win0, int count, int S, float* dst, hipStream_t stream)
{
    if (count < 0 || win0 < 0 || S <= 0) return RY_ERR_ARG;
    if (S % 4 != 0 || count > 65535) return RY_ERR_UNSUPPORTED;
    if (count == 0) return RY_OK;
    if (!pool || !win || !dst) return RY_ERR_ARG;
    const int64_t nt = ry_cdiv((int64_t)S, TV_TILE);                    // nt * nt tiles >= ceil(S * S / 1024) blocks of the linear mapping
    hipLaunchKernelGGL(tile_cut_views_kernel, dim3((unsigned)(nt * nt), count), dim3(256), 0, stream, pool, win + win0 * TV_ROW, S, dst);
    RY_CHECK_LAUNCH();
    return RY_OK;
}

extern "C" int ryolo_tile_collect_views(const float* dets, const int32_t* num, int batch, int64_t mk, const float* geom, int64_t win0,
                                        int64_t nwin, int nc, int64_t ld, int S, float* cand, float* key, float* fkey, hipStream_t stream)
{
    if (batch < 0 || mk < 0 || win0 < 0 || nwin < 0 || nc < 0 || ld < 0 || S <= 0) return RY_ERR_ARG;
    if ((win0 + batch) * mk > ld || batch > 65535) return RY_ERR_ARG;      // every slot of the group lies inside the candidate rows
    if (batch == 0 || mk == 0) return RY_OK;
    if (!dets || !num || !geom || !cand || !fkey || (nc && !key)) return RY_ERR_ARG;
    hipLaunchKernelGGL(tile_collect_views_kernel, dim3((unsigned)ry_cdiv(mk, 256), batch), dim3(256), 0, stream, dets, num, mk, geom, win0,
                       nwin, nc, ld, (float)S, cand, key, fkey);
    RY_CHECK_LAUNCH();
    return RY_OK;
}

extern "C" int ryolo_tile_merge_gather(const float* cand, const float* skey, const int64_t* order, int nc, int64_t K, float* rboxes,
                                       hipStream_t stream)
{
    if (nc < 0 || K < 0 || nc > 65535) return RY_ERR_ARG;
    if (nc == 0 || K == 0) return RY_OK;
    if (!cand || !skey || !order || !rboxes) return RY_ERR_ARG;
    hipLaunchKernelGGL(tile_gather_kernel, dim3((unsigned)ry_cdiv(K, 256), nc), dim3(256), 0, stream, cand, skey, order, K, rboxes);
    RY_CHECK_LAUNCH();
    return RY_OK;
}

extern "C" int ryolo_tile_mark(const float* skey, const int64_t* order, const int64_t* keep, const int32_t* num_keep, int nc, int64_t K,
                               int64_t keep_stride, float* fkey, hipStream_t stream)
{
    if (nc < 0 || K < 0 || keep_stride < 0 || keep_stride > K || nc > 65535) return RY_ERR_ARG;
    if (nc == 0 || keep_stride == 0) return RY_OK;
    if (!skey || !order || !keep || !num_keep || !fkey) return RY_ERR_ARG;
    hipLaunchKernelGGL(tile_mark_kernel, dim3((unsigned)ry_cdiv(keep_stride, 256), nc), dim3(256), 0, stream, skey, order, keep, num_keep, K,
                       keep_stride, fkey);
    RY_CHECK_LAUNCH();
    return RY_OK;
}

extern "C" int ryolo_tile_fuse(const float* cand, const int64_t* order, const int32_t* nsel, const int64_t* keep, const int32_t* num_keep,
                               const int32_t* owner, int nc, int64_t K, int64_t keep_stride, int64_t ld, int mode, int n_ens, float* fused,
                               float* fkey, hipStream_t stream)
{
    if (nc < 0 || K < 0 || keep_stride < 0 || keep_stride > K || ld < 0 || nc > 65535) return RY_ERR_ARG;
    if ((mode != 0 && mode != 1) || n_ens < 1) return RY_ERR_ARG;
    if (nc == 0 || keep_stride == 0) return RY_OK;
    if (!cand || !order || !nsel || !keep || !num_keep || !owner || !fused || !fkey || fused == cand) return RY_ERR_ARG;
    hipLaunchKernelGGL(tile_fuse_kernel, dim3((unsigned)ry_cdiv(keep_stride, 4), nc), dim3(256), 0, stream, cand, order, nsel, keep, num_keep,
                       owner, K, keep_stride, ld, mode, n_ens, fused, fkey);
    RY_CHECK_LAUNCH();
    return RY_OK;
}

extern "C" int ryolo_tile_emit(const float* cand, const int64_t* order, const int32_t* num, int64_t max_det, float* out, hipStream_t stream)
{
    if (max_det < 0) return RY_ERR_ARG;
    if (max_det == 0) return RY_OK;
    if (!cand || !order || !num || !out) return RY_ERR_ARG;
    hipLaunchKernelGGL(tile_emit_kernel, dim3((unsigned)ry_cdiv(max_det, 256)), dim3(256), 0, stream, cand, order, num, max_det, out);
    RY_CHECK_LAUNCH();
    return RY_OK;
}
