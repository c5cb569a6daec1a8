// Anchors fitted to a dataset, and the labels no anchor reaches — gfx950.
// The reference has no code for this stage: its nine anchors are constants of the model file.  The definitions are the standard
// auto-anchor ones (k-means start, fitness = mean best side ratio of the reached labels, mutation search), restated in numpy in
// tests/anchor_ref.py; the reach rule is the target-assignment rule of the fused loss (csrc/loss.hip, cand_test), written again here
// from its definition with the same float operations.
//
//   ryolo_anchor_reach    one thread per target row: per scale the number of anchors that pass the loss's rule; integer summary
//   ryolo_anchor_fitness  fitness / reached labels / anchor passes of one anchor set
//   ryolo_anchor_evolve   (1 + C) evolution strategy: per generation ONE pass over the labels scores all C children (anchor_score_kernel,
//                         children formed from k and the mutation table as the workgroup starts, never written to memory) and ONE
//                         single-workgroup launch sums the partials in a fixed two-level order, picks the best child and accepts or rejects it ON THE
//                         DEVICE (anchor_decide_kernel): no host read, no host decision between generations
//   ryolo_anchor_kmeans   Lloyd's k-means on (w, h): quantile start through ryolo_argsort_desc, two launches per iteration
// No allocation, no synchronisation, every launch capturable.  No float atomics anywhere: sums run over a grid whose size depends on n
// alone, per thread in index order, then lanes, waves and workgroups in a fixed order, in double; counts are integers.
// Compiled with -ffp-contract=off: the side ratios and squared distances are the float32 operations of the definitions, unfused.
#include "common.h"

#define AN_MAX_K 32
#define AN_MAX_C 16
#define AN_BLOCKS 1024            // upper bound of the scoring / k-means grids
#define AN_THREADS 256
#define KM_THREADS 64

// ------------------------------------------------------------------------------------------------ reach
// csrc/loss.hip, cand_test: gw = tg[4] * fg, rw = gw / aw, max(rw, 1 / rw) < 4 on both sides; modes != 0 also |cos(theta - anchor angle)| >
// 0.866.  The image index is not looked at (the loss drops rows whose index is outside the batch).
__global__ __launch_bounds__(AN_THREADS) void anchor_reach_kernel(const LossParams p, int* __restrict__ counts, unsigned long long* __restrict__ summary)
{
    const int64_t t = (int64_t)blockIdx.x * AN_THREADS + threadIdx.x;
    int c[3] = {0, 0, 0};
    if (t < p.nt) {
        const float* tg = p.targets + t * p.tcols;
        const float tw = tg[4], th = tg[5];
        const float ta = p.mode != 0 ? tg[6] : 0.f;
        for (int i = 0; i < 3; i++) {
            const float fg = (float)p.gs[i];
            const float gw = tw * fg, gh = th * fg;
            for (int a = 0; a < p.na; a++) {
                const float aw = p.anchors[i][a][0], ah = p.anchors[i][a][1];
                const float rw = gw / aw, rh = gh / ah;
                const float mw = fmaxf(rw, 1.0f / rw), mh = fmaxf(rh, 1.0f / rh);
                bool ok = fmaxf(mw, mh) < 4.0f;
                if (p.mode != 0) ok = ok && (fabsf(cosf(ta - p.anchors[i][a][2])) > 0.866f);
                c[i] += ok ? 1 : 0;
            }
            counts[t * 3 + i] = c[i];
        }
    }
    // summary: reached rows per scale, rows reached by no scale, anchor passes — integer sums, any order gives the same result
    int v[5] = {c[0] > 0, c[1] > 0, c[2] > 0, (t < p.nt) && (c[0] + c[1] + c[2] == 0), c[0] + c[1] + c[2]};
    __shared__ int ws_[AN_THREADS / 64][5];
#pragma unroll
    for (int k = 0; k < 5; k++) {
        for (int o = 32; o > 0; o >>= 1) v[k] += __shfl_xor(v[k], o, 64);
        if ((threadIdx.x & 63) == 0) ws_[threadIdx.x >> 6][k] = v[k];
    }
    __syncthreads();
    if (threadIdx.x < 5) {
        int s = 0;
        for (int w = 0; w < AN_THREADS / 64; w++) s += ws_[w][threadIdx.x];
        if (s) atomicAdd(&summary[threadIdx.x], (unsigned long long)s);
    }
}

extern "C" int ryolo_anchor_reach(const LossParams* p, int32_t* counts, int64_t* summary, hipStream_t stream)
{
    if (!p || !summary) return RY_ERR_ARG;
    if (p->mode < 0 || p->mode > 5 || p->na < 1 || p->na > LOSS_MAX_NA || p->nt < 0) return RY_ERR_ARG;
    if (p->nt > 0 && (!p->targets || !counts || p->tcols < (p->mode != 0 ? 7 : 6))) return RY_ERR_ARG;
    for (int i = 0; i < 3; i++)
        if (p->gs[i] <= 0) return RY_ERR_ARG;
    if (hipMemsetAsync(summary, 0, 5 * sizeof(int64_t), stream) != hipSuccess) return RY_ERR_LAUNCH;
    if (p->nt == 0) return RY_OK;
    hipLaunchKernelGGL(anchor_reach_kernel, dim3((unsigned)ry_cdiv(p->nt, AN_THREADS)), dim3(AN_THREADS), 0, stream, *p, counts,
                       reinterpret_cast<unsigned long long*>(summary));
    RY_CHECK_LAUNCH();
    return RY_OK;
}

// ------------------------------------------------------------------------------------------------ fitness and evolution
// stats (device, 4 x 8 bytes): [0] the fitness as a double, [1] reached labels, [2] anchor passes, [3] accepted generations.
struct AnStats { double fit; long long reached, passes, accepted; };
struct AnPart { double sum; long long reached, passes; };       // one per (workgroup, child)

static inline int an_blocks(int64_t n) { const int64_t b = ry_cdiv(n, AN_THREADS); return (int)(b < AN_BLOCKS ? (b < 1 ? 1 : b) : AN_BLOCKS); }

// Scores C <= CT anchor sets against every label in one pass.  v == null: the one set is k itself; else set c is max(k * v[c], 2.0f).
template <int CT>
__global__ __launch_bounds__(AN_THREADS) void anchor_score_kernel(const float2* __restrict__ wh, int64_t n, const float* __restrict__ k,
                                                                  const float* __restrict__ v, int K, int C, float inv, AnPart* __restrict__ part)
{
    __shared__ float2 ch[CT * AN_MAX_K];
    for (int idx = threadIdx.x; idx < C * K; idx += AN_THREADS) {
        const int j = idx % K;
        float2 a = make_float2(k[2 * j], k[2 * j + 1]);
        if (v) {
            a.x = fmaxf(a.x * v[2 * idx], 2.0f);
            a.y = fmaxf(a.y * v[2 * idx + 1], 2.0f);
        }
        ch[idx] = a;
    }
    __syncthreads();
    double s[CT];
    int rc[CT], pc[CT];
#pragma unroll
    for (int c = 0; c < CT; c++) { s[c] = 0.0; rc[c] = 0; pc[c] = 0; }
    for (int64_t i = (int64_t)blockIdx.x * AN_THREADS + threadIdx.x; i < n; i += (int64_t)gridDim.x * AN_THREADS) {
        const float2 l = wh[i];
#pragma unroll
        for (int c = 0; c < CT; c++) {
            if (c < C) {
                float x = 0.f;
                int np = 0;
                for (int j = 0; j < K; j++) {
                    const float2 a = ch[c * K + j];
                    const float rw = l.x / a.x, rh = l.y / a.y;
                    const float m = fminf(fminf(rw, 1.0f / rw), fminf(rh, 1.0f / rh));
                    np += m > inv ? 1 : 0;
                    x = j == 0 ? m : fmaxf(x, m);
                }
                if (x > inv) { s[c] += (double)x; rc[c]++; }
                pc[c] += np;
            }
        }
    }
    __shared__ double wsum[AN_THREADS / 64][CT];
    __shared__ int wrc[AN_THREADS / 64][CT], wpc[AN_THREADS / 64][CT];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
#pragma unroll
    for (int c = 0; c < CT; c++) {
        const double sd = wave_sum_d(s[c]);
        int r = rc[c], q = pc[c];
        for (int o = 32; o > 0; o >>= 1) { r += __shfl_xor(r, o, 64); q += __shfl_xor(q, o, 64); }
        if (lane == 0) { wsum[wave][c] = sd; wrc[wave][c] = r; wpc[wave][c] = q; }
    }
    __syncthreads();
    if ((int)threadIdx.x < C) {
        AnPart o;
        o.sum = 0.0; o.reached = 0; o.passes = 0;
        for (int w = 0; w < AN_THREADS / 64; w++) { o.sum += wsum[w][threadIdx.x]; o.reached += wrc[w][threadIdx.x]; o.passes += wpc[w][threadIdx.x]; }
        part[(int64_t)blockIdx.x * AN_MAX_C + threadIdx.x] = o;
    }
}

// One workgroup, one wave per child: lane l sums the partials of workgroups l, l + 64, ... in that order, lane 0 then adds the 64 lane
// sums in lane order (a fixed two-level order, 16 + 64 dependent additions instead of 1024); the best child (lowest c among equals)
// replaces k iff its fitness is strictly greater.  v == null: the scores are those of k itself and become the state.
__global__ __launch_bounds__(64 * AN_MAX_C) void anchor_decide_kernel(const AnPart* __restrict__ part, int nblk, int64_t n, float* __restrict__ k,
                                                                      const float* __restrict__ v, int K, int C, AnStats* __restrict__ st)
{
    __shared__ AnPart lanes[AN_MAX_C][64];
    __shared__ AnPart tot[AN_MAX_C];
    __shared__ int sel;
    const int c = threadIdx.x >> 6, lane = threadIdx.x & 63;
    if (c < C) {
        AnPart o;
        o.sum = 0.0; o.reached = 0; o.passes = 0;
        for (int b = lane; b < nblk; b += 64) {
            const AnPart q = part[(int64_t)b * AN_MAX_C + c];
            o.sum += q.sum; o.reached += q.reached; o.passes += q.passes;
        }
        lanes[c][lane] = o;
    }
    __syncthreads();
    if (c < C && lane == 0) {
        AnPart o;
        o.sum = 0.0; o.reached = 0; o.passes = 0;
        for (int l = 0; l < 64; l++) { o.sum += lanes[c][l].sum; o.reached += lanes[c][l].reached; o.passes += lanes[c][l].passes; }
        o.sum = o.sum / (double)n;
        tot[c] = o;
    }
    __syncthreads();
    if (threadIdx.x == 0) {
        int best = 0;
        for (int j = 1; j < C; j++)
            if (tot[j].sum > tot[best].sum) best = j;
        if (!v) {
            st->fit = tot[0].sum; st->reached = tot[0].reached; st->passes = tot[0].passes; st->accepted = 0;
            sel = -1;
        } else if (tot[best].sum > st->fit) {
            st->fit = tot[best].sum; st->reached = tot[best].reached; st->passes = tot[best].passes; st->accepted += 1;
            sel = best;
        } else {
            sel = -1;
        }
    }
    __syncthreads();
    const int s = sel;
    if (s >= 0 && (int)threadIdx.x < 2 * K) {
        const int e = threadIdx.x;                                   // element (anchor e / 2, side e % 2)
        k[e] = fmaxf(k[e] * v[(int64_t)s * K * 2 + e], 2.0f);
    }
}

static int an_score(const float* wh, int64_t n, const float* k, const float* v, int K, int C, float inv, AnPart* part, int nblk, hipStream_t stream)
{
    const float2* w2 = reinterpret_cast<const float2*>(wh);
#define AN_LAUNCH(CT) hipLaunchKernelGGL(anchor_score_kernel<CT>, dim3(nblk), dim3(AN_THREADS), 0, stream, w2, n, k, v, K, C, inv, part)
    if (C <= 1) AN_LAUNCH(1);
    else if (C <= 2) AN_LAUNCH(2);
    else if (C <= 4) AN_LAUNCH(4);
    else if (C <= 8) AN_LAUNCH(8);
    else AN_LAUNCH(16);
#undef AN_LAUNCH
    RY_CHECK_LAUNCH();
    return RY_OK;
}

extern "C" int ryolo_anchor_workspace_bytes(int64_t n, size_t* bytes)
{
    if (!bytes || n < 1) return RY_ERR_ARG;
    *bytes = ry_align256((size_t)AN_BLOCKS * AN_MAX_C * sizeof(AnPart));
    return RY_OK;
}

static bool an_args_ok(const float* wh, int64_t n, const float* k, int K, double thr, const void* ws, const void* stats)
{
    return wh && k && ws && stats && n >= 1 && n < (1ll << 31) && K >= 1 && K <= AN_MAX_K && thr > 0.0 && thr == thr;
}
static bool an_ws_ok(size_t ws_bytes) { return ws_bytes >= (size_t)AN_BLOCKS * AN_MAX_C * sizeof(AnPart); }

extern "C" int ryolo_anchor_fitness(const float* wh, int64_t n, const float* k, int K, double thr, void* ws, size_t ws_bytes, int64_t* stats,
                                    hipStream_t stream)
{
    if (!an_args_ok(wh, n, k, K, thr, ws, stats)) return RY_ERR_ARG;
    if (!an_ws_ok(ws_bytes)) return RY_ERR_WORKSPACE;
    const float inv = (float)(1.0 / thr);
    const int nblk = an_blocks(n);
    AnPart* part = reinterpret_cast<AnPart*>(ws);
    const int rc = an_score(wh, n, k, nullptr, K, 1, inv, part, nblk, stream);
    if (rc != RY_OK) return rc;
    hipLaunchKernelGGL(anchor_decide_kernel, dim3(1), dim3(64 * AN_MAX_C), 0, stream, part, nblk, n, (float*)nullptr, (const float*)nullptr, K, 1,
                       reinterpret_cast<AnStats*>(stats));
    RY_CHECK_LAUNCH();
    return RY_OK;
}

// k [K][2] is read and overwritten; v [G][C][K][2] is the mutation table.
extern "C" int ryolo_anchor_evolve(const float* wh, int64_t n, float* k, int K, const float* v, int G, int C, double thr, void* ws, size_t ws_bytes,
                                   int64_t* stats, hipStream_t stream)
{
    if (!an_args_ok(wh, n, k, K, thr, ws, stats)) return RY_ERR_ARG;
    if (G < 0 || C < 1 || C > AN_MAX_C || (G > 0 && !v)) return RY_ERR_ARG;
    if (!an_ws_ok(ws_bytes)) return RY_ERR_WORKSPACE;
    const float inv = (float)(1.0 / thr);
    const int nblk = an_blocks(n);
    AnPart* part = reinterpret_cast<AnPart*>(ws);
    AnStats* st = reinterpret_cast<AnStats*>(stats);
    int rc = an_score(wh, n, k, nullptr, K, 1, inv, part, nblk, stream);
    if (rc != RY_OK) return rc;
    hipLaunchKernelGGL(anchor_decide_kernel, dim3(1), dim3(64 * AN_MAX_C), 0, stream, part, nblk, n, (float*)nullptr, (const float*)nullptr, K, 1, st);
    RY_CHECK_LAUNCH();
    for (int g = 0; g < G; g++) {
        const float* vg = v + (int64_t)g * C * K * 2;
        rc = an_score(wh, n, k, vg, K, C, inv, part, nblk, stream);
        if (rc != RY_OK) return rc;
        hipLaunchKernelGGL(anchor_decide_kernel, dim3(1), dim3(64 * AN_MAX_C), 0, stream, part, nblk, n, k, vg, K, C, st);
        RY_CHECK_LAUNCH();
    }
    return RY_OK;
}

// ------------------------------------------------------------------------------------------------ k-means start
__global__ __launch_bounds__(AN_THREADS) void anchor_area_kernel(const float2* __restrict__ wh, int64_t n, float* __restrict__ area)
{
    for (int64_t i = (int64_t)blockIdx.x * AN_THREADS + threadIdx.x; i < n; i += (int64_t)gridDim.x * AN_THREADS) {
        const float2 l = wh[i];
        area[i] = l.x * l.y;
    }
}

// centroid j = the label at rank floor((j + 0.5) / K * n) of the labels in ascending area order (order = stable DESCENDING argsort)
__global__ __launch_bounds__(64) void kmeans_init_kernel(const float2* __restrict__ wh, int64_t n, const int64_t* __restrict__ order, int K, float* __restrict__ k)
{
    const int j = threadIdx.x;
    if (j >= K) return;
    int64_t q = ((int64_t)(2 * j + 1) * n) / (2 * K);
    q = q < 0 ? 0 : (q > n - 1 ? n - 1 : q);
    int64_t i = order[n - 1 - q];
    i = i < 0 ? 0 : (i > n - 1 ? n - 1 : i);                          // data-derived index: clamped
    const float2 l = wh[i];
    k[2 * j] = l.x; k[2 * j + 1] = l.y;
}

struct KmPart { double sw, sh; long long cnt; };

// One wave per workgroup over a contiguous range of labels; a thread keeps its own accumulator per cluster in LDS (no atomics), labels in
// index order; lane sums are then added in lane order.  Distances are float32 (dw * dw + dh * dh, unfused); equal distances: lowest centroid.
__global__ __launch_bounds__(KM_THREADS) void kmeans_assign_kernel(const float2* __restrict__ wh, int64_t n, int64_t per, const float* __restrict__ k, int K,
                                                                   int* __restrict__ assign, KmPart* __restrict__ part)
{
    extern __shared__ double km_lds[];
    double* aw = km_lds;                                              // [K][64]
    double* ah = aw + K * KM_THREADS;
    int* ac = reinterpret_cast<int*>(ah + K * KM_THREADS);
    __shared__ float2 cen[AN_MAX_K];
    const int t = threadIdx.x;
    if (t < K) cen[t] = make_float2(k[2 * t], k[2 * t + 1]);
    for (int j = 0; j < K; j++) { aw[j * KM_THREADS + t] = 0.0; ah[j * KM_THREADS + t] = 0.0; ac[j * KM_THREADS + t] = 0; }
    __syncthreads();
    const int64_t lo = (int64_t)blockIdx.x * per;
    const int64_t hi = lo + per < n ? lo + per : n;
    for (int64_t i = lo + t; i < hi; i += KM_THREADS) {
        const float2 l = wh[i];
        int best = 0;
        float bd = 0.f;
        for (int j = 0; j < K; j++) {
            const float dw = l.x - cen[j].x, dh = l.y - cen[j].y;
            const float d = dw * dw + dh * dh;
            if (j == 0 || d < bd) { bd = d; best = j; }
        }
        if (assign) assign[i] = best;
        aw[best * KM_THREADS + t] += (double)l.x;
        ah[best * KM_THREADS + t] += (double)l.y;
        ac[best * KM_THREADS + t] += 1;
    }
    __syncthreads();
    if (t < K) {
        KmPart o;
        o.sw = 0.0; o.sh = 0.0; o.cnt = 0;
        for (int u = 0; u < KM_THREADS; u++) { o.sw += aw[t * KM_THREADS + u]; o.sh += ah[t * KM_THREADS + u]; o.cnt += ac[t * KM_THREADS + u]; }
        part[(int64_t)blockIdx.x * AN_MAX_K + t] = o;
    }
}

// new centroid = double sum / count, cast to float32; an empty cluster keeps its centroid
__global__ __launch_bounds__(64) void kmeans_update_kernel(const KmPart* __restrict__ part, int nblk, int K, float* __restrict__ k)
{
    const int j = threadIdx.x;
    if (j >= K) return;
    double sw = 0.0, sh = 0.0;
    long long cnt = 0;
    for (int b = 0; b < nblk; b++) {
        const KmPart q = part[(int64_t)b * AN_MAX_K + j];
        sw += q.sw; sh += q.sh; cnt += q.cnt;
    }
    if (cnt > 0) {
        k[2 * j] = (float)(sw / (double)cnt);
        k[2 * j + 1] = (float)(sh / (double)cnt);
    }
}

static int km_layout(int64_t n, size_t* part_off, size_t* area_off, size_t* order_off, size_t* sort_off, size_t* sort_bytes, size_t* total)
{
    size_t sb = 0;
    const int rc = ryolo_sort_workspace_bytes(1, n, &sb);
    if (rc != RY_OK) return rc;
    size_t off = 0;
    *part_off = off; off += ry_align256((size_t)AN_BLOCKS * AN_MAX_K * sizeof(KmPart));
    *area_off = off; off += ry_align256((size_t)n * sizeof(float));
    *order_off = off; off += ry_align256((size_t)n * sizeof(int64_t));
    *sort_off = off; off += ry_align256(sb);
    *sort_bytes = sb;
    *total = off;
    return RY_OK;
}

extern "C" int ryolo_anchor_kmeans_workspace_bytes(int64_t n, size_t* bytes)
{
    if (!bytes || n < 1 || n > (1ll << 24)) return RY_ERR_ARG;
    size_t a, b, c, d, e;
    return km_layout(n, &a, &b, &c, &d, &e, bytes);
}

// init != 0: k is set to the quantile start first; else k [K][2] holds the start.  assign (optional, int32 [n]): the assignment made by the
// LAST iteration (against the centroids that iteration started from).
extern "C" int ryolo_anchor_kmeans(const float* wh, int64_t n, float* k, int K, int iters, int init, int32_t* assign, void* ws, size_t ws_bytes,
                                   hipStream_t stream)
{
    if (!wh || !k || !ws || n < 1 || n > (1ll << 24) || K < 1 || K > AN_MAX_K || iters < 0) return RY_ERR_ARG;
    size_t part_off, area_off, order_off, sort_off, sort_bytes, total;
    int rc = km_layout(n, &part_off, &area_off, &order_off, &sort_off, &sort_bytes, &total);
    if (rc != RY_OK) return rc;
    if (ws_bytes < total) return RY_ERR_WORKSPACE;
    char* base = reinterpret_cast<char*>(ws);
    const float2* w2 = reinterpret_cast<const float2*>(wh);
    KmPart* part = reinterpret_cast<KmPart*>(base + part_off);
    if (init) {
        float* area = reinterpret_cast<float*>(base + area_off);
        int64_t* order = reinterpret_cast<int64_t*>(base + order_off);
        hipLaunchKernelGGL(anchor_area_kernel, dim3(an_blocks(n)), dim3(AN_THREADS), 0, stream, w2, n, area);
        RY_CHECK_LAUNCH();
        rc = ryolo_argsort_desc(area, n, order, base + sort_off, sort_bytes, stream);
        if (rc != RY_OK) return rc;
        hipLaunchKernelGGL(kmeans_init_kernel, dim3(1), dim3(64), 0, stream, w2, n, order, K, k);
        RY_CHECK_LAUNCH();
    }
    int64_t nblk = ry_cdiv(n, 4 * KM_THREADS);
    if (nblk > AN_BLOCKS) nblk = AN_BLOCKS;
    const int64_t per = ry_cdiv(n, nblk);
    const size_t lds = (size_t)K * KM_THREADS * (2 * sizeof(double) + sizeof(int));
    for (int it = 0; it < iters; it++) {
        hipLaunchKernelGGL(kmeans_assign_kernel, dim3((unsigned)nblk), dim3(KM_THREADS), lds, stream, w2, n, per, k, K, assign, part);
        RY_CHECK_LAUNCH();
        hipLaunchKernelGGL(kmeans_update_kernel, dim3(1), dim3(64), 0, stream, part, (int)nblk, K, k);
        RY_CHECK_LAUNCH();
    }
    return RY_OK;
}
