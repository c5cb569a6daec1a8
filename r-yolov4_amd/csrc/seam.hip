// Seam-aware full-scene merge for gfx950 (lib/tiled.py Seam; include/ryolo.h states the rules): a window border cuts an object into a
// fragment that the overlapping neighbour sees whole.  Two kernels around the untouched class-wise NMS of csrc/tiled.hip:
//
//   tile_seam_flags_kernel  (in front of the first ryolo_topk_desc) one thread = one candidate slot: the row's axis-aligned extent in the
//                        frame of its own rate, the four cut bits against its own window, and — rule 1 — whether another window of the
//                        same rate holds the whole row clear of its own borders (bit 16).  The scene's window table (x0, y0, rate per
//                        window) is staged in LDS once per block; windows are ordered by rate, so a thread walks down and up from its
//                        own window while the rate stays its own and never looks at another rate's windows.  key2 = key with -inf at
//                        the class row of every redundant slot: the selection that follows simply does not see them.  Row nc of key2
//                        is reset to -inf: a seam merge marks its kept slots there, not in the plain merge's fkey, whose stale
//                        marks of another keep set it would otherwise see (and leave its own behind).
//   seam_prep_kernel     (behind ryolo_tile_mark / ryolo_tile_fuse) per class the BoxPrep of every kept position, by keep-list index, and
//                        the keep-list indices of the cut ones, appended with an integer atomic: the list's order is arbitrary and
//                        nothing depends on it, since every cut box is decided on its own.
//   seam_cover_kernel    rule 2, one wave = one cut box a.  The lanes stride the class's kept boxes b; the area test and the circle
//                        test come first and the few survivors are compacted into a per-wave LDS queue, so the scratch-heavy pair
//                        function runs on dense lanes (64 queued pairs at a time, the rest at the end).  The wave leaves at its first
//                        hit: lane 0 writes fkey[slot of a] = -inf and counts one drop.
// Every output is written once; the only atomics are integer (list append, drop counts), so the results are deterministic.
// Compiled with -ffp-contract=off: tests/seam_ref.py restates the arithmetic in numpy fp32, one operation per step.
#include "common.h"
#include "rotated_iou.h"

#define SEAM_ROW 6                                                       // int64 columns of a window-table row (csrc/tiled.hip TV_ROW)
#define SEAM_CUT 15u
#define SEAM_REDUNDANT 16u
#define SEAM_MAX_WINDOWS 4096                                            // 16 B each: the 64 KiB a launch gets without an attribute

struct SeamRow { float X, Y, xl, xr, yt, yb; };

// window v = (x0, y0, rate, -) of the row's rate sees the row whole: holds its centre, and on every side either lies on the border of
// the resized scene or clears the row's extent by more than `margin`
__device__ __forceinline__ bool seam_sees_whole(const float4 v, const SeamRow& r, float S, float margin, float Wr, float Hr)
{
    const float vx1 = v.x + S, vy1 = v.y + S;
    if (!(v.x <= r.X && r.X < vx1 && v.y <= r.Y && r.Y < vy1)) return false;
    if (!(v.x == 0.f || r.xl > v.x + margin)) return false;
    if (!(vx1 >= Wr || r.xr < vx1 - margin)) return false;
    if (!(v.y == 0.f || r.yt > v.y + margin)) return false;
    if (!(vy1 >= Hr || r.yb < vy1 - margin)) return false;
    return true;
}

__global__ __launch_bounds__(256) void tile_seam_flags_kernel(const float* __restrict__ cand, const float* __restrict__ key,
                                                              const int64_t* __restrict__ win, const float* __restrict__ geom, int64_t nwin,
                                                              int nviews, int64_t mk, int64_t ld, int nc, float S, float margin, int whole,
                                                              uint8_t* __restrict__ flags, float* __restrict__ key2,
                                                              int32_t* __restrict__ counts)
{
    extern __shared__ float4 wtab[];                                    // [nwin / nviews] = (x0, y0, rate, 0) of every window
    const int64_t nW = nwin / nviews;
    for (int64_t i = threadIdx.x; i < nW; i += 256) {
        const float* g = geom + i * nviews * 4;                         // entries are window-major: a window's first entry
        wtab[i] = make_float4(g[0], g[1], g[2], 0.f);
    }
    __syncthreads();
    const int64_t slot = (int64_t)blockIdx.x * 256 + threadIdx.x;
    bool red = false;
    if (slot < ld) {
        unsigned f = 0;
        const float* p = cand + slot * 7;
        const float cf = p[6];
        const int c = (cf >= 0.f && cf < (float)nc) ? (int)cf : -1;
        const int64_t e = slot / mk;
        if (c >= 0 && e < nwin && key[(int64_t)c * ld + slot] > -INFINITY) {
            const float* g = geom + e * 4;
            const float x0 = g[0], y0 = g[1], r = g[2];
            const float Hr = (float)win[e * SEAM_ROW + 1], Wr = (float)win[e * SEAM_ROW + 2];
            const float w = p[2], h = p[3];
            const float cs = fabsf((float)cos((double)p[4])), sn = fabsf((float)sin((double)p[4]));
            const float ex = 0.5f * (cs * w + sn * h), ey = 0.5f * (sn * w + cs * h);
            const float EX = ex * r, EY = ey * r;
            SeamRow q;
            q.X = p[0] * r; q.Y = p[1] * r;
            q.xl = q.X - EX; q.xr = q.X + EX; q.yt = q.Y - EY; q.yb = q.Y + EY;
            const float x1 = x0 + S, y1 = y0 + S;
            if (x0 > 0.f && q.xl <= x0 + margin) f |= 1u;
            if (x1 < Wr && q.xr >= x1 - margin) f |= 2u;
            if (y0 > 0.f && q.yt <= y0 + margin) f |= 4u;
            if (y1 < Hr && q.yb >= y1 - margin) f |= 8u;
            if (whole && f) {
                const int64_t w0 = e / nviews;                          // the row's own window; its rate's windows surround it
                for (int64_t i = w0; i >= 0 && !red; i--) {
                    const float4 v = wtab[i];
                    if (v.z != r) break;
                    red = seam_sees_whole(v, q, S, margin, Wr, Hr);
                }
                for (int64_t i = w0 + 1; i < nW && !red; i++) {
                    const float4 v = wtab[i];
                    if (v.z != r) break;
                    red = seam_sees_whole(v, q, S, margin, Wr, Hr);
                }
                if (red) f |= SEAM_REDUNDANT;
            }
        }
        flags[slot] = (uint8_t)f;
        if (whole)
            for (int k = 0; k < nc; k++) {
                const int64_t at = (int64_t)k * ld + slot;
                key2[at] = (red && k == c) ? -INFINITY : key[at];
            }
        key2[(int64_t)nc * ld + slot] = -INFINITY;                       // row nc: the seam merge's own final key, reset per merge
    }
    const unsigned long long m = __ballot(red);
    if (m && (threadIdx.x & 63) == 0) atomicAdd(counts, (int32_t)__popcll(m));
}

// ------------------------------------------------------------------------------------------ rule 2
// workspace: ncut int32 [nc] | cut int32 [nc][K] | prep BoxPrep [nc][K]   (each part starts on a 256-byte step)
static inline size_t seam_off_cut(int nc) { return ry_align256((size_t)nc * sizeof(int32_t)); }
static inline size_t seam_off_prep(int nc, int64_t K) { return seam_off_cut(nc) + ry_align256((size_t)nc * K * sizeof(int32_t)); }

__global__ __launch_bounds__(256) void seam_prep_kernel(const float* __restrict__ rboxes, const int64_t* __restrict__ order,
                                                        const int32_t* __restrict__ nsel, const int64_t* __restrict__ keep,
                                                        const int32_t* __restrict__ num_keep, int64_t K, int64_t keep_stride,
                                                        const uint8_t* __restrict__ flags, int64_t ld, BoxPrep* __restrict__ prep,
                                                        int32_t* __restrict__ cut, int32_t* __restrict__ ncut)
{
    const int64_t j = (int64_t)blockIdx.x * 256 + threadIdx.x;
    const int c = blockIdx.y;
    int64_t nk = num_keep[c];
    if (nk > keep_stride) nk = keep_stride;
    if (j >= nk) return;
    int64_t n = nsel[c];
    if (n > K) n = K;
    const int64_t k = keep[(int64_t)c * keep_stride + j];
    BoxPrep p;
    bool is_cut = false;
    const int64_t slot = (k >= 0 && k < n) ? order[(int64_t)c * K + k] : -1;
    if (slot >= 0 && slot < ld) {
        box_prep(rboxes + ((int64_t)c * K + k) * 5, p);
        is_cut = (flags[slot] & SEAM_CUT) != 0;
    } else {                                                            // a table out of range: an empty box covers nothing
        p.x = p.y = p.w = p.h = p.sh = p.cw = p.ch = p.sw = p.area = p.rad = 0.f;
    }
    float4* o = reinterpret_cast<float4*>(prep + (int64_t)c * K + j);
    o[0] = make_float4(p.x, p.y, p.w, p.h);
    o[1] = make_float4(p.sh, p.cw, p.ch, p.sw);
    o[2] = make_float4(p.area, p.rad, 0.f, 0.f);
    if (is_cut) cut[(int64_t)c * K + atomicAdd(ncut + c, 1)] = (int32_t)j;
}

__device__ __forceinline__ BoxPrep seam_load_prep(const BoxPrep* __restrict__ src)
{
    const float4* s = reinterpret_cast<const float4*>(src);
    const float4 a = s[0], b = s[1], d = s[2];
    BoxPrep p;
    p.x = a.x; p.y = a.y; p.w = a.z; p.h = a.w;
    p.sh = b.x; p.cw = b.y; p.ch = b.z; p.sw = b.w;
    p.area = d.x; p.rad = d.y; p.pad0 = 0.f; p.pad1 = 0.f;
    return p;
}

// cov = inter / area_a written through the IoU the pair function returns: inter = iou * (area_a + area_b) / (1 + iou)
__device__ __forceinline__ bool seam_covered(const BoxPrep& A, const BoxPrep& B, float cover)
{
    const float iou = rotated_iou_pair(A, B);
    const float s = A.area + B.area;
    const float n = iou * s;
    const float d1 = 1.f + iou;
    const float d = d1 * A.area;
    return n / d >= cover;
}

// the lanes of a wave exchange queue entries through LDS: order the wave's own LDS accesses around the exchange
__device__ __forceinline__ void seam_wave_sync()
{
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
}

__global__ __launch_bounds__(256) void seam_cover_kernel(const BoxPrep* __restrict__ prep, const int32_t* __restrict__ cut,
                                                         const int32_t* __restrict__ ncut, const int64_t* __restrict__ order,
                                                         const int64_t* __restrict__ keep, const int32_t* __restrict__ num_keep, int64_t K,
                                                         int64_t keep_stride, int64_t ld, float cover, float* __restrict__ fkey,
                                                         int32_t* __restrict__ counts)
{
    __shared__ int32_t queue[4][128];
    const int c = blockIdx.y, wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    int32_t* q = queue[wave];
    int64_t nk = num_keep[c];
    if (nk > keep_stride) nk = keep_stride;
    if (nk < 0) nk = 0;
    int64_t na = ncut[c];
    if (na > nk) na = nk;
    const BoxPrep* pc = prep + (int64_t)c * K;
    const unsigned long long below = (1ull << lane) - 1ull;
    for (int64_t i = (int64_t)blockIdx.x * 4 + wave; i < na; i += (int64_t)gridDim.x * 4) {      // wave-uniform, like every branch below
        const int64_t ja = cut[(int64_t)c * K + i];
        if (ja < 0 || ja >= nk) continue;
        const BoxPrep A = seam_load_prep(pc + ja);
        int qn = 0;
        bool hit = false;
        for (int64_t base = 0; !hit; base += 64) {
            const bool last = base >= nk;                               // one more turn after the list: the queue's remainder
            if (!last) {
                const int64_t jb = base + lane;
                bool ok = jb < nk && jb != ja;
                if (ok) {
                    const BoxPrep B = seam_load_prep(pc + jb);
                    ok = B.area > A.area && !boxes_far_apart(A, B);
                }
                const unsigned long long m = __ballot(ok);
                if (ok) q[qn + __popcll(m & below)] = (int32_t)jb;      // qn < 64 here: the queue holds at most 127
                qn += __popcll(m);
                seam_wave_sync();
            }
            if (qn >= 64 || (last && qn)) {                             // a full wave of pairs, or what is left of them
                const int np = qn < 64 ? qn : 64;
                bool h = false;
                if (lane < np) {
                    const BoxPrep Q = seam_load_prep(pc + q[lane]);
                    h = seam_covered(A, Q, cover);
                }
                hit = __ballot(h) != 0ull;
                const int32_t t = lane < qn - np ? q[np + lane] : 0;    // np == 64 whenever something is behind it
                seam_wave_sync();
                if (lane < qn - np) q[lane] = t;
                qn -= np;
                seam_wave_sync();
            }
            if (last) break;
        }
        seam_wave_sync();                                               // the queue is reused by the wave's next cut box
        if (hit && lane == 0) {
            const int64_t k = keep[(int64_t)c * keep_stride + ja];      // seam_prep_kernel listed ja: k and its slot are in range
            fkey[order[(int64_t)c * K + k]] = -INFINITY;
            atomicAdd(counts + 1, 1);
        }
    }
}

// -------------------------------------------------------------------------------------------------- C ABI
extern "C" int ryolo_tile_seam_flags(const float* cand, const float* key, const int64_t* win, const float* geom, int64_t nwin, int nviews,
                                     int64_t mk, int64_t ld, int nc, int S, float margin, int whole, uint8_t* flags, float* key2,
                                     int32_t* counts, hipStream_t stream)
{
    if (nwin < 0 || nviews < 1 || mk < 0 || ld < 0 || nc < 0 || S <= 0) return RY_ERR_ARG;
    if (!(margin >= 0.f) || !(margin <= 3.0e38f) || (whole != 0 && whole != 1)) return RY_ERR_ARG;
    if (nwin % nviews != 0 || nwin * mk > ld || (ld > 0 && mk == 0)) return RY_ERR_ARG;
    if (!counts) return RY_ERR_ARG;
    if (ld > 0 && (!cand || !win || !geom || !flags || !key2 || (nc && !key))) return RY_ERR_ARG;
    if (key2 && key2 == key) return RY_ERR_ARG;
    const int64_t nW = nwin / nviews;
    if (nW > SEAM_MAX_WINDOWS || ry_cdiv(ld, 256) > 0x7fffffff) return RY_ERR_UNSUPPORTED;
    if (hipMemsetAsync(counts, 0, 2 * sizeof(int32_t), stream) != hipSuccess) return RY_ERR_LAUNCH;
    if (ld == 0) return RY_OK;
    hipLaunchKernelGGL(tile_seam_flags_kernel, dim3((unsigned)ry_cdiv(ld, 256)), dim3(256), (size_t)nW * sizeof(float4), stream, cand, key, win,
                       geom, nwin, nviews, mk, ld, nc, (float)S, margin, whole, flags, key2, counts);
    RY_CHECK_LAUNCH();
    return RY_OK;
}

extern "C" int ryolo_tile_seam_workspace_bytes(int nc, int64_t K, size_t* bytes)
{
    if (!bytes || nc < 0 || K < 0) return RY_ERR_ARG;
    *bytes = seam_off_prep(nc, K) + ry_align256((size_t)nc * K * sizeof(BoxPrep)) + 256;
    return RY_OK;
}

extern "C" int ryolo_tile_seam_cover(const float* rboxes, const int64_t* order, const int32_t* nsel, const int64_t* keep,
                                     const int32_t* num_keep, int nc, int64_t K, int64_t keep_stride, const uint8_t* flags, int64_t ld,
                                     float cover, float* fkey, int32_t* counts, void* ws, size_t ws_bytes, hipStream_t stream)
{
    if (nc < 0 || K < 0 || keep_stride < 0 || keep_stride > K || ld < 0 || nc > 65535) return RY_ERR_ARG;
    if (!(cover >= 0.05f) || !(cover <= 1.f)) return RY_ERR_ARG;
    if (nc == 0 || keep_stride == 0) return RY_OK;
    if (!rboxes || !order || !nsel || !keep || !num_keep || !flags || !fkey || !counts || !ws) return RY_ERR_ARG;
    if (K > 0x7fffffff) return RY_ERR_UNSUPPORTED;                      // keep-list indices are stored as int32
    size_t need;
    ryolo_tile_seam_workspace_bytes(nc, K, &need);
    if (ws_bytes < need) return RY_ERR_WORKSPACE;
    int32_t* ncut = reinterpret_cast<int32_t*>(ws);
    int32_t* cut = reinterpret_cast<int32_t*>(reinterpret_cast<char*>(ws) + seam_off_cut(nc));
    BoxPrep* prep = reinterpret_cast<BoxPrep*>(reinterpret_cast<char*>(ws) + seam_off_prep(nc, K));
    if (hipMemsetAsync(ncut, 0, (size_t)nc * sizeof(int32_t), stream) != hipSuccess) return RY_ERR_LAUNCH;
    hipLaunchKernelGGL(seam_prep_kernel, dim3((unsigned)ry_cdiv(keep_stride, 256), nc), dim3(256), 0, stream, rboxes, order, nsel, keep,
                       num_keep, K, keep_stride, flags, ld, prep, cut, ncut);
    const int64_t gx = ry_cdiv(keep_stride, 4);
    hipLaunchKernelGGL(seam_cover_kernel, dim3((unsigned)(gx < 64 ? gx : 64), nc), dim3(256), 0, stream, prep, cut, ncut, order, keep, num_keep,
                       K, keep_stride, ld, cover, fkey, counts);
    RY_CHECK_LAUNCH();
    return RY_OK;
}
