// mAP evaluation, device side: the per-image true-positive matching of the reference's
// `get_batch_statistics` (test.py:102-149).  The reference loops over images and classes on the host, calls detectron2's
// pairwise_iou_rotated per (image, class) and walks the matches in Python with `.item()` syncs; here one workgroup per image
// does it in a single launch for the whole batch:
//   phase 1  every prediction finds its best-IoU label of the SAME class (first maximum, like torch.max) with the exact
//            pair function shared with NMS (rotated_iou.h; this file is compiled without FMA contraction like nms.hip);
//   phase 2  one thread per class walks that class's predictions in score order (post_process order) and claims labels:
//            a prediction is a TP at threshold k iff its best label is still free and IoU > iouv[k]; a prediction whose best
//            label is taken stays a false positive (the reference never falls back to the second-best label, :138-141).
// Side effect kept (test.py:126): theta of the predictions becomes DEGREES in place when the image has labels.
#include "common.h"
#include "rotated_iou.h"

#define MAP_MAX_CLASSES 256

__global__ __launch_bounds__(256) void map_match_kernel(float* __restrict__ preds, const int64_t* __restrict__ poff, const float* __restrict__ tg,
                                                        const int64_t* __restrict__ toff, const float* __restrict__ iouv, int niou,
                                                        unsigned char* __restrict__ tp, float* __restrict__ best_iou, int* __restrict__ best_t,
                                                        unsigned char* __restrict__ taken)
{
    const int b = blockIdx.x, tid = threadIdx.x;
    const int64_t p0 = poff[b], t0 = toff[b];
    const int n = (int)(poff[b + 1] - p0), nl = (int)(toff[b + 1] - t0);
    for (int k = tid; k < n * niou; k += 256) tp[p0 * niou + k] = 0;
    if (n == 0 || nl == 0) return;
    const float PI_F = 3.14159274f;                                   // float32(np.pi): `pred_boxes[:, 4] / np.pi * 180` on a float32 tensor
    for (int i = tid; i < n; i += 256) preds[(p0 + i) * 7 + 4] = preds[(p0 + i) * 7 + 4] / PI_F * 180.f;
    for (int t = tid; t < nl; t += 256) taken[t0 + t] = 0;
    __syncthreads();
    for (int i = tid; i < n; i += 256) {
        const float* pr = preds + (p0 + i) * 7;
        const float cls = pr[6];
        BoxPrep P;
        box_prep(pr, P);
        float bi = -1.f;
        int bt = -1;
        for (int t = 0; t < nl; t++) {
            const float* tr = tg + (t0 + t) * 7;
            if (tr[1] != cls) continue;
            const float tb[5] = {tr[2], tr[3], tr[4], tr[5], tr[6] / PI_F * 180.f};
            BoxPrep T;
            box_prep(tb, T);
            const float v = boxes_far_apart(P, T) ? 0.f : rotated_iou_pair(P, T);
            if (v > bi) { bi = v; bt = t; }
        }
        best_iou[p0 + i] = bi;
        best_t[p0 + i] = bt;
    }
    __syncthreads();
    // labels of different classes are disjoint, so the class threads never touch the same `taken` byte
    const float c = (float)tid, thr0 = iouv[0];
    for (int i = 0; i < n; i++) {
        if (preds[(p0 + i) * 7 + 6] != c) continue;
        const int bt = best_t[p0 + i];
        const float bi = best_iou[p0 + i];
        if (bt < 0 || !(bi > thr0) || taken[t0 + bt]) continue;
        taken[t0 + bt] = 1;
        for (int k = 0; k < niou; k++) tp[(p0 + i) * niou + k] = bi > iouv[k] ? 1 : 0;
    }
}

extern "C" int ryolo_map_match_workspace_bytes(int64_t npred, int64_t ntgt, size_t* bytes)
{
    if (!bytes || npred < 0 || ntgt < 0) return RY_ERR_ARG;
    *bytes = (size_t)npred * 8 + (size_t)ntgt + 256;
    return RY_OK;
}

extern "C" int ryolo_map_match(float* preds, const int64_t* pred_off, const float* targets, const int64_t* tgt_off, int batch, int64_t npred,
                               int64_t ntgt, const float* iouv, int niou, int num_classes, unsigned char* tp, void* ws, size_t ws_bytes,
                               hipStream_t stream)
{
    if (batch < 0 || npred < 0 || ntgt < 0 || niou < 1) return RY_ERR_ARG;
    if (num_classes > MAP_MAX_CLASSES) return RY_ERR_UNSUPPORTED;
    if (batch == 0 || npred == 0) return RY_OK;
    if (!preds || !pred_off || !tgt_off || !iouv || !tp || !ws || (ntgt > 0 && !targets)) return RY_ERR_ARG;
    if (ws_bytes < (size_t)npred * 8 + (size_t)ntgt + 256) return RY_ERR_WORKSPACE;
    float* best_iou = reinterpret_cast<float*>(ws);
    int* best_t = reinterpret_cast<int*>(best_iou + npred);
    unsigned char* taken = reinterpret_cast<unsigned char*>(best_t + npred);
    hipLaunchKernelGGL(map_match_kernel, dim3((unsigned)batch), dim3(256), 0, stream, preds, pred_off, targets, tgt_off, iouv, niou, tp, best_iou,
                       best_t, taken);
    RY_CHECK_LAUNCH();
    return RY_OK;
}

// ------------------------------------------------------------------------------------------------ AP from the statistics
// `ap_per_class` / `compute_ap` of the reference (test.py:16-99) on the device: the confidence sort (csrc/topk.hip), the per-class
// cumulative hit counts, recall / precision curves, the precision envelope, the 101-point interpolated integral for every IoU threshold
// and the 1000-point precision / recall curves over confidence.  What stays on the host is O(classes x 1000): F1, its mean, the argmax.
// The floating-point expressions are numpy's, restated: float64 throughout, `hits / (n_labels + 1e-16)`, `hits / rank`, np.interp
// (last knot <= x, slope * (x - xp[j]) + fp[j], exact hit returns fp[j]), np.trapz = pairwise-summed d * (y1 + y0) / 2 — compiled
// without FMA contraction like the rest of this file, so the numbers equal the host path's (lib/evaluate.py) bit for bit on the fixture.
#define AP_MAX_T 16
#define AP_THREADS 1024

// rows per class (cnt), where each class's rows start once they are grouped (off) and, for a caller with target classes, labels per class
// (nlab; the VOC back end has none: nl = 0 and nlab null).  Both AP back ends start here.
__global__ __launch_bounds__(AP_THREADS) void class_hist_kernel(const float* __restrict__ pcls, int64_t n, const float* __restrict__ tcls, int64_t nl,
                                                                int nc, int64_t* __restrict__ cnt, int64_t* __restrict__ nlab,
                                                                int64_t* __restrict__ off)
{
    __shared__ int c_p[MAP_MAX_CLASSES], c_l[MAP_MAX_CLASSES];
    const int tid = threadIdx.x;
    for (int k = tid; k < nc; k += AP_THREADS) { c_p[k] = 0; c_l[k] = 0; }
    __syncthreads();
    for (int64_t i = tid; i < n; i += AP_THREADS) {
        const float c = pcls[i];
        const int k = (int)c;
        if (k >= 0 && k < nc && (float)k == c) atomicAdd(&c_p[k], 1);
    }
    for (int64_t i = tid; i < nl; i += AP_THREADS) {
        const float c = tcls[i];
        const int k = (int)c;
        if (k >= 0 && k < nc && (float)k == c) atomicAdd(&c_l[k], 1);
    }
    __syncthreads();
    if (nlab)
        for (int k = tid; k < nc; k += AP_THREADS) nlab[k] = c_l[k];
    if (tid == 0) {
        int64_t run = 0;
        for (int k = 0; k < nc; k++) { cnt[k] = c_p[k]; off[k] = run; run += c_p[k]; }
    }
}

// one workgroup per class: walk the detections in confidence order, scan the class's hits per threshold, write the curves
__global__ __launch_bounds__(AP_THREADS) void ap_curves_kernel(const unsigned char* __restrict__ tp, const float* __restrict__ conf,
                                                               const float* __restrict__ pcls, const int64_t* __restrict__ order, int64_t n, int T,
                                                               const int64_t* __restrict__ cnt, const int64_t* __restrict__ nlab,
                                                               const int64_t* __restrict__ off, double* __restrict__ negc,
                                                               double* __restrict__ rec, double* __restrict__ prec)
{
    __shared__ unsigned wt[16][AP_MAX_T + 1], wp[16][AP_MAX_T + 1], tot[AP_MAX_T + 1];
    const int k = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    if (cnt[k] == 0 || nlab[k] == 0) return;
    const double denom = (double)nlab[k] + 1e-16;
    const int64_t o0 = off[k];
    const float kc = (float)k;
    const unsigned long long lt = (1ull << lane) - 1ull;
    int64_t run[AP_MAX_T + 1];
#pragma unroll
    for (int q = 0; q <= AP_MAX_T; q++) run[q] = 0;
    for (int64_t i0 = 0; i0 < n; i0 += AP_THREADS) {
        const int64_t i = i0 + tid;
        const int64_t idx = i < n ? order[i] : 0;
        const bool f0 = i < n && pcls[idx] == kc;
        unsigned pre[AP_MAX_T + 1];
        bool fl[AP_MAX_T + 1];
#pragma unroll
        for (int q = 0; q <= AP_MAX_T; q++) {
            fl[q] = q == 0 ? f0 : (q <= T && f0 && tp[idx * T + (q - 1)] != 0);
            const unsigned long long b = __ballot(fl[q]);
            pre[q] = (unsigned)__popcll(b & lt);
            if (lane == 0) wt[wave][q] = (unsigned)__popcll(b);
        }
        __syncthreads();
        if (tid <= T) {
            unsigned r = 0;
            for (int w = 0; w < 16; w++) { wp[w][tid] = r; r += wt[w][tid]; }
            tot[tid] = r;
        }
        __syncthreads();
        if (f0) {
            const int64_t pos = run[0] + wp[wave][0] + pre[0];
            negc[o0 + pos] = (double)(-conf[idx]);
#pragma unroll
            for (int q = 1; q <= AP_MAX_T; q++)
                if (q <= T) {
                    const int64_t hits = run[q] + wp[wave][q] + pre[q] + (fl[q] ? 1 : 0);
                    rec[(int64_t)(q - 1) * n + o0 + pos] = (double)hits / denom;
                    prec[(int64_t)(q - 1) * n + o0 + pos] = (double)hits / (double)(pos + 1);
                }
        }
#pragma unroll
        for (int q = 0; q <= AP_MAX_T; q++)
            if (q <= T) run[q] += tot[q];
        __syncthreads();
    }
}

// np.interp(x, xp, fp, left, right) for ONE x over virtual knot arrays given as functors (length L >= 1, xp non-decreasing)
template <class XP, class FP>
__device__ __forceinline__ double np_interp1(double x, int64_t L, XP xp, FP fp, double left, double right)
{
    if (x > xp(L - 1)) return right;
    if (x < xp(0)) return left;
    int64_t lo = 0, hi = L;                                       // j = (number of knots <= x) - 1
    while (lo < hi) {
        const int64_t mid = lo + ((hi - lo) >> 1);
        if (x >= xp(mid)) lo = mid + 1; else hi = mid;
    }
    const int64_t j = lo - 1;
    if (j == L - 1) return fp(j);
    const double xj = xp(j);
    if (xj == x) return fp(j);
    const double slope = (fp(j + 1) - fp(j)) / (xp(j + 1) - xj);
    double r = slope * (x - xj) + fp(j);
    if (r != r) {
        r = slope * (x - xp(j + 1)) + fp(j + 1);
        if (r != r && fp(j) == fp(j + 1)) r = fp(j);
    }
    return r;
}

// numpy's pairwise summation of a contiguous double vector, 8 <= n <= 128 (one block of the recursion) or n < 8
__device__ __forceinline__ double np_pairwise_sum(const double* a, int n)
{
    if (n < 8) {
        double r = 0.0;
        for (int i = 0; i < n; i++) r += a[i];
        return r;
    }
    double r[8];
    for (int j = 0; j < 8; j++) r[j] = a[j];
    int i = 8;
    for (; i < n - (n % 8); i += 8)
        for (int j = 0; j < 8; j++) r[j] += a[i + j];
    double res = ((r[0] + r[1]) + (r[2] + r[3])) + ((r[4] + r[5]) + (r[6] + r[7]));
    for (; i < n; i++) res += a[i];
    return res;
}

// The precision envelope of one class at one threshold, by the whole workgroup: e_[i] = max(p_[i], .., p_[m - 1], 0), the running maximum
// from the right, in chunks of AP_THREADS from the right end.  Returns the maximum over all m (0 when m == 0); e_ is visible to every
// thread on return.
__device__ __forceinline__ double suffix_max_envelope(const double* __restrict__ p_, double* __restrict__ e_, int64_t m)
{
    __shared__ double wmax[16], carry_s;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    if (tid == 0) carry_s = 0.0;                                     // precision right of the last row: the appended knot / mpre's final 0
    __syncthreads();
    for (int64_t hi = m; hi > 0; hi -= AP_THREADS) {               // chunks from the right end
        const int64_t i = hi - AP_THREADS + tid;                   // this chunk covers [hi - 1024, hi)
        double v = i >= 0 ? p_[i] : 0.0;
        for (int d = 1; d < 64; d <<= 1) {                         // suffix maximum inside the wave
            const double o = __shfl_down(v, d, 64);
            if (lane + d < 64) v = fmax(v, o);
        }
        if (lane == 0) wmax[wave] = v;
        __syncthreads();
        double later = carry_s;
        for (int w = wave + 1; w < 16; w++) later = fmax(later, wmax[w]);
        v = fmax(v, later);
        if (i >= 0) e_[i] = v;
        __syncthreads();
        if (tid == 0) {
            double c = carry_s;
            for (int w = 0; w < 16; w++) c = fmax(c, wmax[w]);
            carry_s = c;
        }
        __syncthreads();
    }
    __threadfence_block();
    __syncthreads();
    return carry_s;
}

// grid (T, classes): precision envelope, 101-point interpolation, trapezoid
__global__ __launch_bounds__(AP_THREADS) void ap_integrate_kernel(int64_t n, int T, const int64_t* __restrict__ cnt, const int64_t* __restrict__ nlab,
                                                                  const int64_t* __restrict__ off, const double* __restrict__ rec,
                                                                  const double* __restrict__ prec, double* __restrict__ env,
                                                                  const double* __restrict__ grid101, double* __restrict__ ap)
{
    __shared__ double y[101], term[100];
    const int t = blockIdx.x, k = blockIdx.y, tid = threadIdx.x;
    const int64_t m = cnt[k];
    if (m == 0 || nlab[k] == 0) { if (tid == 0) ap[(int64_t)k * T + t] = 0.0; return; }
    const double* r_ = rec + (int64_t)t * n + off[k];
    const double* p_ = prec + (int64_t)t * n + off[k];
    double* e_ = env + (int64_t)t * n + off[k];
    const double env0 = fmax(1.0, suffix_max_envelope(p_, e_, m));                        // leading knot (recall 0, precision 1)
    const double rlast = r_[m - 1] + 0.01;
    auto xp = [&](int64_t j) -> double { return j == 0 ? 0.0 : (j <= m ? r_[j - 1] : rlast); };
    auto fp = [&](int64_t j) -> double { return j == 0 ? env0 : (j <= m ? e_[j - 1] : 0.0); };
    if (tid < 101) y[tid] = np_interp1(grid101[tid], m + 2, xp, fp, fp(0), fp(m + 1));
    __syncthreads();
    if (tid < 100) term[tid] = (grid101[tid + 1] - grid101[tid]) * (y[tid + 1] + y[tid]) / 2.0;
    __syncthreads();
    if (tid == 0) ap[(int64_t)k * T + t] = np_pairwise_sum(term, 100);
}

// precision / recall at the first IoU threshold as functions of confidence: np.interp(-grid, -conf, curve, left = 0 / 1)
__global__ __launch_bounds__(AP_THREADS) void ap_pr_kernel(int64_t n, const int64_t* __restrict__ cnt, const int64_t* __restrict__ nlab,
                                                           const int64_t* __restrict__ off, const double* __restrict__ negc, const double* __restrict__ rec,
                                                           const double* __restrict__ prec, const double* __restrict__ cgrid, int ng,
                                                           double* __restrict__ prec_at, double* __restrict__ rec_at)
{
    const int k = blockIdx.x;
    const int64_t m = cnt[k];
    const bool dead = m == 0 || nlab[k] == 0;
    const double* x_ = negc + off[k];
    const double* r_ = rec + off[k];
    const double* p_ = prec + off[k];
    auto xp = [&](int64_t j) -> double { return x_[j]; };
    auto fr = [&](int64_t j) -> double { return r_[j]; };
    auto fq = [&](int64_t j) -> double { return p_[j]; };
    for (int i = threadIdx.x; i < ng; i += AP_THREADS) {
        double pr = 0.0, rc = 0.0;
        if (!dead) {
            const double x = -cgrid[i];
            rc = np_interp1(x, m, xp, fr, 0.0, r_[m - 1]);
            pr = np_interp1(x, m, xp, fq, 1.0, p_[m - 1]);
        }
        prec_at[(int64_t)k * ng + i] = pr;
        rec_at[(int64_t)k * ng + i] = rc;
    }
}

// every workspace of this file is carved front to back in 256-byte steps
template <class T>
static inline T* ws_take(unsigned char*& base, size_t bytes)
{
    T* p = reinterpret_cast<T*>(base);
    base += ry_align256(bytes);
    return p;
}

static inline size_t ap_rows(int64_t n) { return (size_t)(n > 0 ? n : 1); }

// Both AP workspaces begin  sort workspace | order [n]:  the size checks and the bytes of that head ...
static int ap_head_bytes(int64_t n, int niou, int nc, size_t* head)
{
    if (n < 0 || niou < 1 || niou > AP_MAX_T || nc < 1 || nc > MAP_MAX_CLASSES) return RY_ERR_ARG;
    size_t sort = 0;
    if (n > 0 && ryolo_sort_workspace_bytes(1, n, &sort) != RY_OK) return RY_ERR_ARG;
    *head = ry_align256(sort) + ry_align256(ap_rows(n) * 8);
    return RY_OK;
}

// ... and its carve, with the sort that fills `order`: (confidence desc, index asc), np.argsort(-conf) with ties fixed
static int ap_sorted_order(const float* conf, int64_t n, unsigned char*& base, int64_t*& order, hipStream_t stream)
{
    size_t sort = 0;
    if (n > 0) ryolo_sort_workspace_bytes(1, n, &sort);
    void* sort_ws = ws_take<unsigned char>(base, sort);
    order = ws_take<int64_t>(base, ap_rows(n) * 8);
    return n > 0 ? ryolo_argsort_desc(conf, n, order, sort_ws, sort, stream) : RY_OK;
}

extern "C" int ryolo_ap_workspace_bytes(int64_t n, int niou, int nc, size_t* bytes)
{
    size_t head = 0;
    if (!bytes || ap_head_bytes(n, niou, nc, &head) != RY_OK) return RY_ERR_ARG;
    const size_t nn = ap_rows(n);
    *bytes = head + ry_align256((size_t)3 * nc * 8) + ry_align256(nn * 8) + 3 * ry_align256(nn * niou * 8);
    return RY_OK;
}

extern "C" int ryolo_ap_per_class(const unsigned char* tp, const float* conf, const float* pred_cls, int64_t n, const float* target_cls, int64_t nl,
                                  int nc, int niou, const double* recall_grid, const double* conf_grid, int nconf, void* ws, size_t ws_bytes,
                                  double* ap, double* prec_at, double* rec_at, int64_t* n_labels, int64_t* n_pred, hipStream_t stream)
{
    size_t need = 0;
    if (ryolo_ap_workspace_bytes(n, niou, nc, &need) != RY_OK) return RY_ERR_ARG;
    if (!ws || ws_bytes < need) return RY_ERR_WORKSPACE;
    if (!ap || !prec_at || !rec_at || !n_labels || !n_pred || !recall_grid || !conf_grid || nconf < 1 || nl < 0) return RY_ERR_ARG;
    if (n > 0 && (!tp || !conf || !pred_cls)) return RY_ERR_ARG;
    if (nl > 0 && !target_cls) return RY_ERR_ARG;
    const size_t nn = ap_rows(n);
    unsigned char* base = reinterpret_cast<unsigned char*>(ws);
    int64_t* order = nullptr;
    const int rc = ap_sorted_order(conf, n, base, order, stream);
    if (rc) return rc;
    int64_t* off = ws_take<int64_t>(base, (size_t)3 * nc * 8);
    double* negc = ws_take<double>(base, nn * 8);
    double* rec = ws_take<double>(base, nn * niou * 8);
    double* prec = ws_take<double>(base, nn * niou * 8);
    double* env = ws_take<double>(base, nn * niou * 8);
    hipLaunchKernelGGL(class_hist_kernel, dim3(1), dim3(AP_THREADS), 0, stream, pred_cls, n, target_cls, nl, nc, n_pred, n_labels, off);
    hipLaunchKernelGGL(ap_curves_kernel, dim3(nc), dim3(AP_THREADS), 0, stream, tp, conf, pred_cls, order, n, niou, n_pred, n_labels, off, negc, rec, prec);
    hipLaunchKernelGGL(ap_integrate_kernel, dim3(niou, nc), dim3(AP_THREADS), 0, stream, n, niou, n_pred, n_labels, off, rec, prec, env, recall_grid, ap);
    hipLaunchKernelGGL(ap_pr_kernel, dim3(nc), dim3(AP_THREADS), 0, stream, n, n_pred, n_labels, off, negc, rec, prec, conf_grid, nconf, prec_at, rec_at);
    RY_CHECK_LAUNCH();
    return RY_OK;
}

// ------------------------------------------------------------------------------------------------ full-scene matching: the skeleton
// ONE scene of thousands of detections and labels, spread over the chip, under either of two protocols.  Neither falls back to a second-best
// label, so the outcome per label does not depend on a walk: the owner of label t is the SMALLEST detection index i (score order) whose best
// label of its own class (first maximum) is t with IoU above the threshold, and a detection's row follows from whether it owns its best label.
// Four launches, no serial phase, no host read: a thread per label prepares it and resets its owner slots; a wave per detection finds the best
// prepared label of its class and claims it with atomicMin; a thread per detection writes its row behind a device-side cursor; one workgroup
// moves the cursor.  A rule supplies what differs between the protocols and nothing else: the label row and the prepared label, the prepared
// detection, the IoU type and function, owner slots per label, the byte of a row at threshold k, whether positives are counted, the nl limit.
#define MATCH_WAVES 4

__device__ __forceinline__ int det_count(const int32_t* __restrict__ num, int64_t max_det)
{
    const int64_t n = *num;
    return (int)(n < 0 ? 0 : (n > max_det ? max_det : n));
}

// the prepared labels [lo, hi) of class `cls`: empty for a NaN, a non-integer or an out-of-range class, and clamped to [0, nl] — a bad
// table gives wrong numbers, never an access outside prep
__device__ __forceinline__ void class_range(float cls, const int32_t* __restrict__ cls_off, int nc, int64_t nl, int64_t& lo, int64_t& hi)
{
    lo = hi = 0;
    if (cls >= 0.f && cls < (float)nc) {                              // NaN fails both
        const int c = (int)cls;
        if ((float)c == cls && c >= 0 && c < nc) {
            lo = cls_off[c];
            hi = cls_off[c + 1];
            lo = lo < 0 ? 0 : (lo > nl ? nl : lo);
            hi = hi < lo ? lo : (hi > nl ? nl : hi);
        }
    }
}

// n rows fit behind the cursor; when they do not, nothing is written and match_advance_kernel raises the flag
__device__ __forceinline__ bool rows_fit(int64_t cur, int64_t n, int64_t cap) { return !(cur < 0 || cur > cap || n > cap - cur); }

// first maximum in label order over the wave: larger IoU wins, equal IoU the smaller label index, -1 (no label seen) loses to any index
template <class F>
__device__ __forceinline__ void wave_first_max(F& bi, int& bt)
{
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        const F oi = __shfl_xor(bi, o, 64);
        const int ot = __shfl_xor(bt, o, 64);
        if (ot >= 0 && (bt < 0 || oi > bi || (oi == bi && ot < bt))) { bi = oi; bt = ot; }
    }
}

// ---- the reference's rule (test.py:130-145; the one map_match_kernel applies per image): labels are rectangles, the IoU is the float pair
// function shared with NMS, and a detection is a true positive at threshold k iff it owns its best label — claimed at iouv[0], one owner for
// every threshold — and that IoU > iouv[k].
struct SceneRule {
    typedef float Iou;
    typedef BoxPrep Label;
    typedef BoxPrep Det;
    static constexpr int LABEL_FLOATS = 6;                            // cls, x, y, w, h, theta_rad
    static constexpr bool COUNTS_POSITIVES = false, LABELS_FIRST = true;     // workspace: prep | owner | best_iou | best_t
    static constexpr int64_t MAX_LABELS = INT_MAX;
    struct Extra { __host__ __device__ constexpr int slots() const { return 1; } };     // one owner slot per label, nothing else to carry
    struct Positives {};
    typedef bool Row;                                                 // the row owns its best label (claimed at iouv[0])
    static Extra extra(int, const Label*) { return Extra(); }

    static __device__ __forceinline__ void prep_rad(const float* __restrict__ b, BoxPrep& o)
    {
        const float PI_F = 3.14159274f;
        const float d[5] = {b[0], b[1], b[2], b[3], b[4] / PI_F * 180.f};     // degrees in registers: neither labels nor dets are written
        box_prep(d, o);
    }
    static __device__ __forceinline__ void prep_label(const float* __restrict__ row, Label& out) { prep_rad(row + 1, out); }
    static __device__ __forceinline__ void prep_det(const float* __restrict__ pr, Det& D) { prep_rad(pr, D); }
    static __device__ __forceinline__ Iou iou(const Det& P, const Label& L)
    {
        const BoxPrep T = L;
        return boxes_far_apart(P, T) ? 0.f : rotated_iou_pair(P, T);
    }
    static __device__ __forceinline__ Row row(const Extra&, const int32_t* __restrict__ owner, int bt, int i, Iou bi, const float* __restrict__ iouv)
    {
        return bi > iouv[0] && owner[bt] == i;
    }
    static __device__ __forceinline__ unsigned char status(const Extra&, Row hit, const int32_t* __restrict__, int, int, Iou bi,
                                                           const float* __restrict__ iouv, int k)
    {
        return hit && bi > iouv[k] ? 1 : 0;
    }
};

// ---- the DOTA / VOC rule (include/ryolo.h: ryolo_dota_match): the labels are the annotated quadrilaterals, the IoU is a float64
// Sutherland-Hodgman clip of the detection's rectangle against the label's quad, every threshold has its own owner slot, and a detection
// whose best label is "difficult" is ignored (status 2) instead of counted.
// The clip never holds more than 8 vertices (a convex quad cut by four half-planes); it lives in fixed-size arrays, every loop is
// unrolled and an append is a chain of selects, so nothing is indexed by a run-time value.
#define DM_LABEL 15     // floats per label row: cls, difficult, quad[8], rect[5]

struct QuadPrep {       // 14 doubles per prepared label
    double v[8];        // 4 vertices (x, y), counter-clockwise
    double area, x0, x1, y0, y1;
    double hard;        // difficult: 1.0 or 0.0
};

// corners of (x, y, w, h, theta_rad) in float64: h runs along x before the rotation (lib/general.py: xywha2xyxyxyxy)
__device__ __forceinline__ void dm_rect_corners(const float* __restrict__ b, double (&vx)[4], double (&vy)[4])
{
    const double x = (double)b[0], y = (double)b[1], hy = (double)b[2] / 2.0, hx = (double)b[3] / 2.0, th = (double)b[4];
    const double c = cos(th), s = sin(th);
    const double dx[4] = {-hx, hx, hx, -hx}, dy[4] = {-hy, -hy, hy, hy};
#pragma unroll
    for (int k = 0; k < 4; k++) {
        vx[k] = x + (dx[k] * c + dy[k] * s);
        vy[k] = y + (dy[k] * c - dx[k] * s);
    }
}

// twice the signed area of the first n vertices as a fan around vertex 0, terms added in ascending order
template <int N>
__device__ __forceinline__ double dm_fan(const double (&px)[N], const double (&py)[N], int n)
{
    double s = 0.0;
#pragma unroll
    for (int j = 1; j + 1 < N; j++)
        if (j + 1 < n) s += (px[j] - px[0]) * (py[j + 1] - py[0]) - (px[j + 1] - px[0]) * (py[j] - py[0]);
    return s;
}

__device__ __forceinline__ bool dm_finite4(const double (&vx)[4], const double (&vy)[4])
{
    bool ok = true;
#pragma unroll
    for (int k = 0; k < 4; k++) ok = ok && isfinite(vx[k]) && isfinite(vy[k]);
    return ok;
}

#define DM_APPEND(X, Y)                                           \
    {                                                             \
        _Pragma("unroll") for (int q_ = 0; q_ < 8; q_++)          \
            if (m == q_) { qx[q_] = (X); qy[q_] = (Y); }          \
        m += m < 8 ? 1 : 0;                                       \
    }

// area of (detection rectangle) ∩ (label quad L, counter-clockwise): four half-plane steps, a vertex on an edge is inside
__device__ __forceinline__ double dm_clip_area(const double (&dx)[4], const double (&dy)[4], const double* __restrict__ L)
{
    double px[8], py[8];
    int n = 4;
#pragma unroll
    for (int k = 0; k < 8; k++) { px[k] = k < 4 ? dx[k] : 0.0; py[k] = k < 4 ? dy[k] : 0.0; }
    double lx[4], ly[4];
#pragma unroll
    for (int k = 0; k < 4; k++) { lx[k] = L[2 * k]; ly[k] = L[2 * k + 1]; }
#pragma unroll
    for (int e = 0; e < 4; e++) {
        const double ax = lx[e], ay = ly[e], ex = lx[(e + 1) & 3] - ax, ey = ly[(e + 1) & 3] - ay;
        double d[8];
#pragma unroll
        for (int j = 0; j < 8; j++) d[j] = ex * (py[j] - ay) - ey * (px[j] - ax);
        double prx = px[0], pry = py[0], prd = d[0];                  // the vertex before vertex 0: vertex n - 1
#pragma unroll
        for (int j = 1; j < 8; j++)
            if (j == n - 1) { prx = px[j]; pry = py[j]; prd = d[j]; }
        double qx[8], qy[8];
#pragma unroll
        for (int k = 0; k < 8; k++) { qx[k] = 0.0; qy[k] = 0.0; }
        int m = 0;
#pragma unroll
        for (int j = 0; j < 8; j++) {
            if (j < n) {
                const bool ic = d[j] >= 0.0, ip = prd >= 0.0;
                if (ic != ip) {
                    const double u = prd / (prd - d[j]);
                    const double ix = prx + (px[j] - prx) * u, iy = pry + (py[j] - pry) * u;
                    DM_APPEND(ix, iy)
                }
                if (ic) DM_APPEND(px[j], py[j])
            }
            prx = px[j]; pry = py[j]; prd = d[j];
        }
#pragma unroll
        for (int k = 0; k < 8; k++) { px[k] = qx[k]; py[k] = qy[k]; }
        n = m;
    }
    return 0.5 * fabs(dm_fan<8>(px, py, n));
}

struct DotaRule {
    typedef double Iou;
    typedef QuadPrep Label;
    struct Det {
        double dx[4], dy[4], x0, x1, y0, y1, area;                    // corners, bounds, area
        bool live;                                                    // every corner finite
    };
    static constexpr int LABEL_FLOATS = DM_LABEL;
    static constexpr bool COUNTS_POSITIVES = true, LABELS_FIRST = false;     // workspace: best_iou | best_t | prep | owner (ryolo.h)
    static constexpr int64_t MAX_LABELS = INT_MAX / AP_MAX_T;         // owner [nl][niou] is addressed in int32 steps of niou
    struct Extra { int niou; const Label* prep; __host__ __device__ int slots() const { return niou; } };     // a slot per threshold; the flags
    struct Positives { const Label* prep; const int32_t* cls_off; int64_t nl; int nc; int64_t* npos; };      // what npos is counted from
    typedef bool Row;                                                 // the row's best label is difficult
    static Extra extra(int niou, const Label* prep) { return Extra{niou, prep}; }

    static __device__ __forceinline__ void prep_label(const float* __restrict__ r, Label& p)
    {
        double vx[4], vy[4];
#pragma unroll
        for (int k = 0; k < 4; k++) { vx[k] = (double)r[2 + 2 * k]; vy[k] = (double)r[3 + 2 * k]; }
        bool quad = dm_finite4(vx, vy);
        if (quad) {                                                   // strictly convex: the four turns all of one non-zero sign
            bool pos = true, neg = true;
#pragma unroll
            for (int e = 0; e < 4; e++) {
                const int f = (e + 1) & 3, g = (e + 2) & 3;
                const double cr = (vx[f] - vx[e]) * (vy[g] - vy[f]) - (vy[f] - vy[e]) * (vx[g] - vx[f]);
                pos = pos && cr > 0.0;
                neg = neg && cr < 0.0;
            }
            quad = pos || neg;
        }
        if (!quad) dm_rect_corners(r + 10, vx, vy);
        const bool live = dm_finite4(vx, vy);
        const double s = dm_fan<4>(vx, vy, 4);
        if (s < 0.0) {                                                // clockwise in these axes: walk it the other way round
            double u = vx[1]; vx[1] = vx[3]; vx[3] = u;
            u = vy[1]; vy[1] = vy[3]; vy[3] = u;
        }
        double x0 = vx[0], x1 = vx[0], y0 = vy[0], y1 = vy[0];
#pragma unroll
        for (int k = 0; k < 4; k++) {
            p.v[2 * k] = vx[k];
            p.v[2 * k + 1] = vy[k];
            x0 = vx[k] < x0 ? vx[k] : x0; x1 = vx[k] > x1 ? vx[k] : x1;
            y0 = vy[k] < y0 ? vy[k] : y0; y1 = vy[k] > y1 ? vy[k] : y1;
        }
        const double inf = __builtin_huge_val();
        p.area = 0.5 * fabs(s);
        p.x0 = live ? x0 : inf;                                      // a label without finite vertices has empty bounds: IoU 0 with everything
        p.x1 = live ? x1 : -inf;
        p.y0 = live ? y0 : inf;
        p.y1 = live ? y1 : -inf;
        p.hard = r[1] != 0.f ? 1.0 : 0.0;                            // NaN counts as difficult
    }
    static __device__ __forceinline__ void prep_det(const float* __restrict__ pr, Det& D)
    {
        dm_rect_corners(pr, D.dx, D.dy);
        D.live = dm_finite4(D.dx, D.dy);
        D.x0 = D.x1 = D.dx[0];
        D.y0 = D.y1 = D.dy[0];
#pragma unroll
        for (int k = 1; k < 4; k++) {
            D.x0 = D.dx[k] < D.x0 ? D.dx[k] : D.x0; D.x1 = D.dx[k] > D.x1 ? D.dx[k] : D.x1;
            D.y0 = D.dy[k] < D.y0 ? D.dy[k] : D.y0; D.y1 = D.dy[k] > D.y1 ? D.dy[k] : D.y1;
        }
        D.area = 0.5 * fabs(dm_fan<4>(D.dx, D.dy, 4));
    }
    static __device__ __forceinline__ Iou iou(const Det& D, const Label& L)
    {
        double v = 0.0;
        if (D.live && !(D.x1 < L.x0 || L.x1 < D.x0 || D.y1 < L.y0 || L.y1 < D.y0)) {     // disjoint bounds: IoU 0, exactly
            const double inter = dm_clip_area(D.dx, D.dy, L.v);
            const double den = D.area + L.area - inter;
            v = den <= 0.0 ? 0.0 : inter / den;
        }
        return v;
    }
    static __device__ __forceinline__ Row row(const Extra& x, const int32_t* __restrict__, int bt, int, Iou, const float* __restrict__)
    {
        return x.prep[bt].hard != 0.0;
    }
    static __device__ __forceinline__ unsigned char status(const Extra& x, Row hard, const int32_t* __restrict__ owner, int bt, int i, Iou bi,
                                                           const float* __restrict__ iouv, int k)
    {
        return bi > (double)iouv[k] ? (hard ? 2 : (owner[(int64_t)bt * x.niou + k] == i ? 1 : 0)) : 0;
    }
};

// ---- the four kernels
template <class R>
__global__ __launch_bounds__(256) void match_prep_kernel(const float* __restrict__ labels, int64_t nl, const typename R::Extra x,
                                                         typename R::Label* __restrict__ prep, int32_t* __restrict__ owner)
{
    const int64_t t = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (t >= nl) return;
    R::prep_label(labels + t * R::LABEL_FLOATS, prep[t]);
    const int S = x.slots();
    for (int k = 0; k < S; k++) owner[t * S + k] = INT_MAX;
}

template <class R>
__global__ __launch_bounds__(64 * MATCH_WAVES) void match_best_kernel(const float* __restrict__ dets, const int32_t* __restrict__ num, int64_t max_det,
                                                                      const typename R::Label* __restrict__ prep,
                                                                      const int32_t* __restrict__ cls_off, int64_t nl, int nc,
                                                                      const float* __restrict__ iouv, const typename R::Extra x,
                                                                      typename R::Iou* __restrict__ best_iou, int32_t* __restrict__ best_t,
                                                                      int32_t* __restrict__ owner)
{
    typedef typename R::Iou Iou;
    const int lane = threadIdx.x & 63;
    const int64_t i = (int64_t)blockIdx.x * MATCH_WAVES + (threadIdx.x >> 6);
    if (i >= det_count(num, max_det)) return;                         // wave-uniform
    const float* pr = dets + i * 7;
    const float box[5] = {pr[0], pr[1], pr[2], pr[3], pr[4]};         // fetched with the class, not after the class table has answered
    int64_t lo, hi;
    class_range(pr[6], cls_off, nc, nl, lo, hi);
    Iou bi = -1;
    int bt = -1;
    if (lo < hi) {
        typename R::Det D;
        R::prep_det(box, D);
        for (int64_t t = lo + lane; t < hi; t += 64) {
            const Iou v = R::iou(D, prep[t]);
            if (v > bi) { bi = v; bt = (int)t; }
        }
    }
    wave_first_max(bi, bt);
    if (lane == 0) {
        best_iou[i] = bi;
        best_t[i] = bt;
        if (bt >= 0 && bt < nl) {
            const int S = x.slots();
            for (int k = 0; k < S; k++)
                if (bi > (Iou)iouv[k]) atomicMin(&owner[(int64_t)bt * S + k], (int)i);
        }
    }
}

template <class R>
__global__ __launch_bounds__(256) void match_emit_kernel(const float* __restrict__ dets, const int32_t* __restrict__ num, int64_t max_det, int64_t nl,
                                                         const float* __restrict__ iouv, int niou, const typename R::Iou* __restrict__ best_iou,
                                                         const int32_t* __restrict__ best_t, const int32_t* __restrict__ owner,
                                                         const typename R::Extra x, unsigned char* __restrict__ rows,
                                                         float* __restrict__ conf, float* __restrict__ pcls, int64_t cap,
                                                         const int64_t* __restrict__ cursor)
{
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    const int64_t n = det_count(num, max_det);
    if (i >= n) return;
    const int64_t cur = *cursor;
    if (!rows_fit(cur, n, cap)) return;
    const int bt = best_t[i];
    const typename R::Iou bi = best_iou[i];
    const bool has = bt >= 0 && bt < nl;
    const typename R::Row r = has ? R::row(x, owner, bt, (int)i, bi, iouv) : typename R::Row();
    unsigned char* row = rows + (cur + i) * niou;
    for (int k = 0; k < niou; k++) row[k] = has ? R::status(x, r, owner, bt, (int)i, bi, iouv, k) : 0;
    conf[cur + i] = dets[i * 7 + 5];
    pcls[cur + i] = dets[i * 7 + 6];
}

// stream-ordered after every row is written and every read of the cursor: the cursor, the flag and, under a rule that counts them, the
// positives of the scene's classes (labels that are not difficult)
template <class R>
__global__ __launch_bounds__(64) void match_advance_kernel(const int32_t* __restrict__ num, int64_t max_det, int64_t cap, int64_t* __restrict__ cursor,
                                                           int32_t* __restrict__ overflow, const typename R::Positives p)
{
    if (blockIdx.x != 0) return;
    const int64_t n = det_count(num, max_det), cur = *cursor;
    const bool fits = rows_fit(cur, n, cap);
    if constexpr (R::COUNTS_POSITIVES) {
        __syncthreads();                                              // every thread has read the cursor before thread 0 moves it
        if (fits)
            for (int c = threadIdx.x; c < p.nc; c += 64) {
                int64_t lo, hi;
                class_range((float)c, p.cls_off, p.nc, p.nl, lo, hi);
                int64_t easy = 0;
                for (int64_t t = lo; t < hi; t++) easy += p.prep[t].hard == 0.0 ? 1 : 0;
                p.npos[c] += easy;
            }
    }
    if (threadIdx.x == 0) {
        if (fits) *cursor = cur + n;
        else *overflow = 1;
    }
}

// ---- the host side: the workspace holds  best_iou [max_det] Iou | best_t [max_det]  and  prep [nl] Label | owner [nl][slots],  in the
// rule's order
template <class R>
static size_t match_workspace_bytes(int64_t max_det, int64_t nl, int niou)
{
    return ry_align256((size_t)max_det * sizeof(typename R::Iou)) + ry_align256((size_t)max_det * 4) +
           ry_align256((size_t)nl * sizeof(typename R::Label)) + ry_align256((size_t)nl * R::extra(niou, nullptr).slots() * 4) + 256;
}

template <class R>
static int match_launch(const float* dets, const int32_t* num, int64_t max_det, const float* labels, const int32_t* cls_off, int64_t nl, int nc,
                        const float* iouv, int niou, unsigned char* rows, float* conf, float* pcls, int64_t cap, int64_t* cursor,
                        int32_t* overflow, int64_t* npos, void* ws, size_t ws_bytes, hipStream_t stream)
{
    typedef typename R::Iou Iou;
    typedef typename R::Label Label;
    if (max_det < 0 || nl < 0 || nc < 1 || niou < 1 || cap < 0) return RY_ERR_ARG;
    if (nc > MAP_MAX_CLASSES || niou > AP_MAX_T || max_det >= INT_MAX || nl >= R::MAX_LABELS) return RY_ERR_UNSUPPORTED;
    if (max_det == 0 && !R::COUNTS_POSITIVES) return RY_OK;           // no row to write and nothing to count: before any pointer is looked at
    if (!cls_off || !cursor || !overflow || !num || !ws || (nl > 0 && !labels) || (R::COUNTS_POSITIVES && !npos)) return RY_ERR_ARG;
    if (max_det > 0 && (!dets || !iouv || !rows || !conf || !pcls)) return RY_ERR_ARG;
    if (ws_bytes < match_workspace_bytes<R>(max_det, nl, niou)) return RY_ERR_WORKSPACE;
    unsigned char* base = reinterpret_cast<unsigned char*>(ws);
    const size_t owner_bytes = (size_t)nl * R::extra(niou, nullptr).slots() * 4;
    Label* prep = nullptr;
    int32_t* owner = nullptr;
    if (R::LABELS_FIRST) { prep = ws_take<Label>(base, (size_t)nl * sizeof(Label)); owner = ws_take<int32_t>(base, owner_bytes); }
    Iou* best_iou = ws_take<Iou>(base, (size_t)max_det * sizeof(Iou));
    int32_t* best_t = ws_take<int32_t>(base, (size_t)max_det * 4);
    if (!R::LABELS_FIRST) { prep = ws_take<Label>(base, (size_t)nl * sizeof(Label)); owner = ws_take<int32_t>(base, owner_bytes); }
    const typename R::Extra x = R::extra(niou, prep);
    if (nl > 0)
        hipLaunchKernelGGL(match_prep_kernel<R>, dim3((unsigned)ry_cdiv(nl, 256)), dim3(256), 0, stream, labels, nl, x, prep, owner);
    if (max_det > 0) {
        hipLaunchKernelGGL(match_best_kernel<R>, dim3((unsigned)ry_cdiv(max_det, MATCH_WAVES)), dim3(64 * MATCH_WAVES), 0, stream, dets, num, max_det,
                           prep, cls_off, nl, nc, iouv, x, best_iou, best_t, owner);
        hipLaunchKernelGGL(match_emit_kernel<R>, dim3((unsigned)ry_cdiv(max_det, 256)), dim3(256), 0, stream, dets, num, max_det, nl, iouv, niou,
                           best_iou, best_t, owner, x, rows, conf, pcls, cap, cursor);
    }
    typename R::Positives pos{};
    if constexpr (R::COUNTS_POSITIVES) pos = typename R::Positives{prep, cls_off, nl, nc, npos};
    hipLaunchKernelGGL(match_advance_kernel<R>, dim3(1), dim3(64), 0, stream, num, max_det, cap, cursor, overflow, pos);
    RY_CHECK_LAUNCH();
    return RY_OK;
}

extern "C" int ryolo_scene_match_workspace_bytes(int64_t max_det, int64_t nl, size_t* bytes)
{
    if (!bytes || max_det < 0 || nl < 0) return RY_ERR_ARG;
    *bytes = match_workspace_bytes<SceneRule>(max_det, nl, 1);
    return RY_OK;
}

extern "C" int ryolo_scene_match(const float* dets, const int32_t* num, int64_t max_det, const float* labels, const int32_t* cls_off, int64_t nl,
                                 int nc, const float* iouv, int niou, unsigned char* tp, float* conf, float* pcls, int64_t cap, int64_t* cursor,
                                 int32_t* overflow, void* ws, size_t ws_bytes, hipStream_t stream)
{
    return match_launch<SceneRule>(dets, num, max_det, labels, cls_off, nl, nc, iouv, niou, tp, conf, pcls, cap, cursor, overflow, nullptr, ws,
                                   ws_bytes, stream);
}

extern "C" int ryolo_dota_match_workspace_bytes(int64_t max_det, int64_t nl, int niou, size_t* bytes)
{
    if (!bytes || max_det < 0 || nl < 0 || niou < 1 || niou > AP_MAX_T) return RY_ERR_ARG;
    *bytes = match_workspace_bytes<DotaRule>(max_det, nl, niou);
    return RY_OK;
}

extern "C" int ryolo_dota_match(const float* dets, const int32_t* num, int64_t max_det, const float* labels, const int32_t* cls_off, int64_t nl,
                                int nc, const float* iouv, int niou, unsigned char* status, float* conf, float* pcls, int64_t cap, int64_t* cursor,
                                int32_t* overflow, int64_t* npos, void* ws, size_t ws_bytes, hipStream_t stream)
{
    return match_launch<DotaRule>(dets, num, max_det, labels, cls_off, nl, nc, iouv, niou, status, conf, pcls, cap, cursor, overflow, npos, ws,
                                  ws_bytes, stream);
}

// ------------------------------------------------------------------------------------------------ VOC AP from the DOTA statistics
// Per class and threshold: the rows of the class in confidence order (the sort of ryolo_ap_per_class), rows with status 2 left out, running
// true / false positive counts by the ballot / popcount scans of ap_curves_kernel, then the 11-point VOC07 mean or the VOC12 area.

// grid (T, classes): recall / precision after every counted row of the class at threshold t, and how many rows were counted
__global__ __launch_bounds__(AP_THREADS) void voc_curves_kernel(const unsigned char* __restrict__ status, const float* __restrict__ pcls,
                                                                const int64_t* __restrict__ order, int64_t n, int T, const int64_t* __restrict__ cnt,
                                                                const int64_t* __restrict__ npos, const int64_t* __restrict__ off,
                                                                double* __restrict__ rec, double* __restrict__ prec, int64_t* __restrict__ used)
{
    __shared__ unsigned wt[16][2], wp[16][2], tot[2];
    const int t = blockIdx.x, k = blockIdx.y, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int64_t np_ = npos[k];
    if (cnt[k] == 0 || np_ <= 0) { if (tid == 0) used[(int64_t)k * T + t] = 0; return; }
    const int64_t o0 = off[k];
    const float kc = (float)k;
    const unsigned long long lt = (1ull << lane) - 1ull;
    int64_t run_t = 0, run_f = 0;
    for (int64_t i0 = 0; i0 < n; i0 += AP_THREADS) {
        const int64_t i = i0 + tid;
        const int64_t idx = i < n ? order[i] : 0;
        const bool mine = i < n && pcls[idx] == kc;
        const unsigned char s = mine ? status[idx * T + t] : 2;
        const bool ft = s == 1, ff = s != 1 && s != 2;
        const unsigned long long bt_ = __ballot(ft), bf_ = __ballot(ff);
        const unsigned pt = (unsigned)__popcll(bt_ & lt), pf = (unsigned)__popcll(bf_ & lt);
        if (lane == 0) { wt[wave][0] = (unsigned)__popcll(bt_); wt[wave][1] = (unsigned)__popcll(bf_); }
        __syncthreads();
        if (tid < 2) {
            unsigned r = 0;
            for (int w = 0; w < 16; w++) { wp[w][tid] = r; r += wt[w][tid]; }
            tot[tid] = r;
        }
        __syncthreads();
        if (ft || ff) {
            const int64_t tpc = run_t + wp[wave][0] + pt + (ft ? 1 : 0), fpc = run_f + wp[wave][1] + pf + (ff ? 1 : 0);
            const int64_t pos = o0 + tpc + fpc - 1;
            rec[(int64_t)t * n + pos] = (double)tpc / (double)np_;
            prec[(int64_t)t * n + pos] = (double)tpc / fmax((double)(tpc + fpc), 2.220446049250313e-16);
        }
        run_t += tot[0];
        run_f += tot[1];
        __syncthreads();
    }
    if (tid == 0) used[(int64_t)k * T + t] = run_t + run_f;
}

// grid (T, classes): metric 0 the 11-point VOC07 mean, metric 1 the VOC12 area under the precision envelope
__global__ __launch_bounds__(AP_THREADS) void voc_integrate_kernel(int64_t n, int T, int metric, const int64_t* __restrict__ npos,
                                                                   const int64_t* __restrict__ off, const int64_t* __restrict__ used,
                                                                   const double* __restrict__ rec, const double* __restrict__ prec,
                                                                   double* __restrict__ env, const double* __restrict__ grid11, double* __restrict__ ap)
{
    __shared__ double wmax[16][11], term[AP_THREADS], sum_s;
    const int t = blockIdx.x, k = blockIdx.y, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    if (npos[k] <= 0) { if (tid == 0) ap[(int64_t)k * T + t] = __builtin_nan(""); return; }
    const int64_t m = used[(int64_t)k * T + t];
    const double* r_ = rec + (int64_t)t * n + off[k];
    const double* p_ = prec + (int64_t)t * n + off[k];
    double* e_ = env + (int64_t)t * n + off[k];
    if (metric == 0) {
        double g[11], mx[11];
#pragma unroll
        for (int q = 0; q < 11; q++) { g[q] = grid11[q]; mx[q] = 0.0; }     // precision is never negative: 0 is also "no such row"
        for (int64_t j = tid; j < m; j += AP_THREADS) {
            const double r = r_[j], p = p_[j];
#pragma unroll
            for (int q = 0; q < 11; q++)
                if (r >= g[q]) mx[q] = fmax(mx[q], p);
        }
#pragma unroll
        for (int q = 0; q < 11; q++) {
            double v = mx[q];
            for (int d = 32; d > 0; d >>= 1) v = fmax(v, __shfl_xor(v, d, 64));
            if (lane == 0) wmax[wave][q] = v;
        }
        __syncthreads();
        if (tid == 0) {
            double a = 0.0;
            for (int q = 0; q < 11; q++) {
                double v = 0.0;
                for (int w = 0; w < 16; w++) v = fmax(v, wmax[w][q]);
                a = a + v / 11.0;
            }
            ap[(int64_t)k * T + t] = a;
        }
        return;
    }
    if (tid == 0) sum_s = 0.0;
    suffix_max_envelope(p_, e_, m);                                    // mpre ends with 0
    // sum over j of (mrec[j + 1] - mrec[j]) * mpre[j + 1], ascending, one after the other; a term where mrec does not change is +0 and
    // leaves the sum as it is, and the last one, (1 - rec[m - 1]) * 0, likewise
    for (int64_t j0 = 0; j0 < m; j0 += AP_THREADS) {
        const int64_t j = j0 + tid;
        term[tid] = j < m ? (r_[j] - (j > 0 ? r_[j - 1] : 0.0)) * e_[j] : 0.0;
        __syncthreads();
        if (tid == 0) {
            double a = sum_s;
            const int lim = (int)(m - j0 < AP_THREADS ? m - j0 : AP_THREADS);
            for (int q = 0; q < lim; q++) a = a + term[q];
            sum_s = a;
        }
        __syncthreads();
    }
    if (tid == 0) ap[(int64_t)k * T + t] = sum_s;
}

extern "C" int ryolo_ap_voc_workspace_bytes(int64_t n, int niou, int nc, size_t* bytes)
{
    size_t head = 0;
    if (!bytes || ap_head_bytes(n, niou, nc, &head) != RY_OK) return RY_ERR_ARG;
    *bytes = head + ry_align256((size_t)nc * 8) + ry_align256((size_t)nc * niou * 8) + 3 * ry_align256(ap_rows(n) * niou * 8);
    return RY_OK;
}

extern "C" int ryolo_ap_voc(const unsigned char* status, const float* conf, const float* pred_cls, int64_t n, const int64_t* npos, int nc, int niou,
                            int metric, const double* grid11, void* ws, size_t ws_bytes, double* ap, int64_t* n_pred, hipStream_t stream)
{
    size_t need = 0;
    if (ryolo_ap_voc_workspace_bytes(n, niou, nc, &need) != RY_OK || (metric != 0 && metric != 1)) return RY_ERR_ARG;
    if (n >= INT_MAX) return RY_ERR_UNSUPPORTED;
    if (!ws || ws_bytes < need) return RY_ERR_WORKSPACE;
    if (!ap || !n_pred || !npos || !grid11) return RY_ERR_ARG;
    if (n > 0 && (!status || !conf || !pred_cls)) return RY_ERR_ARG;
    const size_t nn = ap_rows(n);
    unsigned char* base = reinterpret_cast<unsigned char*>(ws);
    int64_t* order = nullptr;
    const int rc = ap_sorted_order(conf, n, base, order, stream);
    if (rc) return rc;
    int64_t* off = ws_take<int64_t>(base, (size_t)nc * 8);
    int64_t* used = ws_take<int64_t>(base, (size_t)nc * niou * 8);
    double* rec = ws_take<double>(base, nn * niou * 8);
    double* prec = ws_take<double>(base, nn * niou * 8);
    double* env = ws_take<double>(base, nn * niou * 8);
    hipLaunchKernelGGL(class_hist_kernel, dim3(1), dim3(AP_THREADS), 0, stream, pred_cls, n, (const float*)nullptr, (int64_t)0, nc, n_pred,
                       (int64_t*)nullptr, off);
    hipLaunchKernelGGL(voc_curves_kernel, dim3(niou, nc), dim3(AP_THREADS), 0, stream, status, pred_cls, order, n, niou, n_pred, npos, off, rec, prec, used);
    hipLaunchKernelGGL(voc_integrate_kernel, dim3(niou, nc), dim3(AP_THREADS), 0, stream, n, niou, metric, npos, off, used, rec, prec, env, grid11, ap);
    RY_CHECK_LAUNCH();
    return RY_OK;
}

// ------------------------------------------------------------------------------------------------ full-scene error breakdown
// Why a scene's mAP is what it is (include/ryolo.h: ryolo_scene_errors states the rule): every detection gets one code — true positive,
// duplicate, right place / wrong class, wrong angle only, mislocated, both, background — and every label one status.  The launch shape is
// the skeleton's, with a matcher of its own: the wave of a detection scans the labels of EVERY class once and keeps two running first
// maxima (own class, other classes), then two lanes compute the IoUs of the detection turned to its best label's angle, then lane 0 claims
// the label.  Histograms are counted block-locally in LDS and flushed once per workgroup with integer atomics; the confusion matrix follows
// from the same counts except for its CLS cells, which are rare.  Nothing is read back, nothing allocates, every run gives the same bits.
#define ERR_CODES 8
#define ERR_BUCKETS 3
#define ERR_STATUSES 4
enum { ERR_BELOW = 0, ERR_TP, ERR_DUP, ERR_CLS, ERR_ANG, ERR_LOC, ERR_BOTH, ERR_BKG };

// a class column as a row of the histograms: the integer in [0, nc), or -1
__device__ __forceinline__ int class_index(float cls, int nc)
{
    if (!(cls >= 0.f && cls < (float)nc)) return -1;                  // NaN fails both
    const int c = (int)cls;
    return (float)c == cls && c >= 0 && c < nc ? c : -1;
}

__device__ __forceinline__ void hist_add(int64_t* __restrict__ cell, int v)
{
    atomicAdd(reinterpret_cast<unsigned long long*>(cell), (unsigned long long)v);
}

__global__ __launch_bounds__(256) void errors_prep_kernel(const float* __restrict__ labels, int64_t nl, int nc, BoxPrep* __restrict__ prep,
                                                          int32_t* __restrict__ owner, int32_t* __restrict__ cover, int32_t* __restrict__ lcls)
{
    const int64_t t = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (t >= nl) return;
    SceneRule::prep_label(labels + t * 6, prep[t]);
    owner[t] = INT_MAX;
    cover[t] = 0;
    lcls[t] = class_index(labels[t * 6], nc);
}

__global__ __launch_bounds__(64 * MATCH_WAVES) void errors_best_kernel(const float* __restrict__ dets, const int32_t* __restrict__ num, int64_t max_det,
                                                                       const float* __restrict__ labels, const BoxPrep* __restrict__ prep,
                                                                       const int32_t* __restrict__ cls_off, int64_t nl, int nc, float t_fg,
                                                                       float conf_thres, float* __restrict__ s_iou, int32_t* __restrict__ s_t,
                                                                       float* __restrict__ o_iou, int32_t* __restrict__ o_t,
                                                                       float* __restrict__ a_iou, int32_t* __restrict__ owner)
{
    const int lane = threadIdx.x & 63;
    const int64_t i = (int64_t)blockIdx.x * MATCH_WAVES + (threadIdx.x >> 6);
    if (i >= det_count(num, max_det)) return;                         // wave-uniform
    const float* pr = dets + i * 7;
    const float box[5] = {pr[0], pr[1], pr[2], pr[3], pr[4]};
    const float score = pr[5];
    int64_t lo, hi;
    class_range(pr[6], cls_off, nc, nl, lo, hi);
    int64_t g0 = cls_off[0], g1 = cls_off[nc];                        // every class's rows, clamped as class_range clamps
    g0 = g0 < 0 ? 0 : (g0 > nl ? nl : g0);
    g1 = g1 < g0 ? g0 : (g1 > nl ? nl : g1);
    const int64_t from = lo < hi && lo < g0 ? lo : g0, to = lo < hi && hi > g1 ? hi : g1;     // [g0, g1) with a good table
    float si = -1.f, oi = -1.f;
    int st = -1, ot = -1;
    BoxPrep D;
    SceneRule::prep_det(box, D);
    for (int64_t t = from + lane; t < to; t += 64) {
        const bool mine = t >= lo && t < hi;
        if (!mine && (t < g0 || t >= g1)) continue;
        const float v = SceneRule::iou(D, prep[t]);
        if (mine) { if (v > si) { si = v; st = (int)t; } }
        else if (v > oi) { oi = v; ot = (int)t; }
    }
    wave_first_max(si, st);
    wave_first_max(oi, ot);
    float ai = -1.f;
    if (st >= 0 && st < nl) {                                         // wave-uniform: lane 0 the box as written, lane 1 with w and h swapped
        const bool swap = lane & 1;
        const float turned[5] = {box[0], box[1], swap ? box[3] : box[2], swap ? box[2] : box[3], labels[(int64_t)st * 6 + 5]};
        BoxPrep A;
        SceneRule::prep_rad(turned, A);
        const float v = SceneRule::iou(A, prep[st]);
        const float w = __shfl_xor(v, 1, 64);
        ai = w > v ? w : v;
    }
    if (lane == 0) {
        s_iou[i] = si;
        s_t[i] = st;
        o_iou[i] = oi;
        o_t[i] = ot;
        a_iou[i] = ai;
        if (score >= conf_thres && st >= 0 && st < nl && si > t_fg) atomicMin(&owner[st], (int)i);
    }
}

// a thread per detection: its code, its row behind the cursor, the cover word of the label it points at, the histograms
__global__ __launch_bounds__(256) void errors_emit_kernel(const float* __restrict__ dets, const int32_t* __restrict__ num, int64_t max_det,
                                                          const float* __restrict__ labels, int64_t nl, int nc, float t_fg, float t_bg,
                                                          float conf_thres, const float* __restrict__ s_iou, const int32_t* __restrict__ s_t,
                                                          const float* __restrict__ o_iou, const int32_t* __restrict__ o_t,
                                                          const float* __restrict__ a_iou, const int32_t* __restrict__ owner,
                                                          int32_t* __restrict__ cover, const int32_t* __restrict__ lcls,
                                                          unsigned char* __restrict__ code, float* __restrict__ conf, float* __restrict__ pcls,
                                                          float* __restrict__ ocls, float* __restrict__ r_s, float* __restrict__ r_o,
                                                          float* __restrict__ r_a, int64_t* __restrict__ det_hist, int64_t* __restrict__ cm,
                                                          int64_t cap, const int64_t* __restrict__ cursor)
{
    __shared__ int h[(MAP_MAX_CLASSES + 1) * ERR_CODES];
    const int cells = (nc + 1) * ERR_CODES;
    for (int k = threadIdx.x; k < cells; k += 256) h[k] = 0;
    __syncthreads();
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    const int64_t n = det_count(num, max_det), cur = *cursor;
    if (!rows_fit(cur, n, cap)) return;                               // uniform over the grid: nothing moves
    if (i < n) {
        const float score = dets[i * 7 + 5], cls = dets[i * 7 + 6];
        const float si = s_iou[i], oi = o_iou[i], ai = a_iou[i];
        const int st = s_t[i], ot = o_t[i];
        const bool has_s = st >= 0 && st < nl, has_o = ot >= 0 && ot < nl;
        int c = ERR_BKG;
        if (!(score >= conf_thres)) c = ERR_BELOW;
        else if (has_s && si > t_fg) c = owner[st] == (int)i ? ERR_TP : ERR_DUP;
        else if (has_o && oi > t_fg) c = ERR_CLS;
        else if (has_s && si > t_bg) c = ai > t_fg ? ERR_ANG : ERR_LOC;
        else if (has_o && oi > t_bg) c = ERR_BOTH;
        const int64_t r = cur + i;
        code[r] = (unsigned char)c;
        conf[r] = score;
        pcls[r] = cls;
        ocls[r] = has_o ? labels[(int64_t)ot * 6] : -1.f;
        r_s[r] = si;
        r_o[r] = oi;
        r_a[r] = ai;
        if (c == ERR_CLS) atomicOr(&cover[ot], 1);
        if (c == ERR_ANG || c == ERR_LOC) atomicOr(&cover[st], 2);
        const int pc = class_index(cls, nc);
        atomicAdd(&h[(pc < 0 ? nc : pc) * ERR_CODES + c], 1);
        if (c == ERR_CLS && pc >= 0) {
            const int lc = lcls[ot];
            if (lc >= 0) hist_add(&cm[(int64_t)lc * (nc + 1) + pc], 1);
        }
    }
    __syncthreads();
    for (int k = threadIdx.x; k < cells; k += 256) {
        const int v = h[k];
        if (v == 0) continue;
        hist_add(&det_hist[k], v);
        const int pc = k / ERR_CODES, c = k % ERR_CODES;
        if (pc == nc || c == ERR_BELOW || c == ERR_CLS) continue;     // the other cells of cm follow from the counts
        hist_add(&cm[(int64_t)(c == ERR_TP ? pc : nc) * (nc + 1) + pc], v);
    }
}

// a thread per label: its status from the owner and the cover word, counted by class and size
__global__ __launch_bounds__(256) void errors_label_kernel(const float* __restrict__ labels, int64_t nl, int nc, float e0, float e1,
                                                           const int32_t* __restrict__ num, int64_t max_det, const int32_t* __restrict__ owner,
                                                           const int32_t* __restrict__ cover, const int32_t* __restrict__ lcls,
                                                           int64_t* __restrict__ lab_hist, int64_t* __restrict__ cm, int64_t cap,
                                                           const int64_t* __restrict__ cursor)
{
    __shared__ int h[MAP_MAX_CLASSES * ERR_BUCKETS * ERR_STATUSES];
    const int cells = nc * ERR_BUCKETS * ERR_STATUSES;
    for (int k = threadIdx.x; k < cells; k += 256) h[k] = 0;
    __syncthreads();
    const int64_t t = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (!rows_fit(*cursor, det_count(num, max_det), cap)) return;     // uniform over the grid
    if (t < nl) {
        const int lc = lcls[t];
        if (lc >= 0) {
            const int cv = cover[t];
            const int s = owner[t] != INT_MAX ? 0 : ((cv & 1) ? 1 : ((cv & 2) ? 2 : 3));
            const float area = labels[t * 6 + 3] * labels[t * 6 + 4];
            const int b = (area >= e0 ? 1 : 0) + (area >= e1 ? 1 : 0);
            atomicAdd(&h[(lc * ERR_BUCKETS + b) * ERR_STATUSES + s], 1);
        }
    }
    __syncthreads();
    for (int k = threadIdx.x; k < cells; k += 256) {
        const int v = h[k];
        if (v == 0) continue;
        hist_add(&lab_hist[k], v);
        if (k % ERR_STATUSES != 0) hist_add(&cm[(int64_t)(k / (ERR_BUCKETS * ERR_STATUSES)) * (nc + 1) + nc], v);
    }
}

// workspace:  prep [nl] | owner [nl] | cover [nl] | lcls [nl] | s_iou, s_t, o_iou, o_t, a_iou [max_det] each
static size_t errors_workspace_bytes(int64_t max_det, int64_t nl)
{
    return ry_align256((size_t)nl * sizeof(BoxPrep)) + 3 * ry_align256((size_t)nl * 4) + 5 * ry_align256((size_t)max_det * 4) + 256;
}

extern "C" int ryolo_scene_errors_workspace_bytes(int64_t max_det, int64_t nl, size_t* bytes)
{
    if (!bytes || max_det < 0 || nl < 0) return RY_ERR_ARG;
    *bytes = errors_workspace_bytes(max_det, nl);
    return RY_OK;
}

extern "C" int ryolo_scene_errors(const float* dets, const int32_t* num, int64_t max_det, const float* labels, const int32_t* cls_off, int64_t nl,
                                  int nc, float t_fg, float t_bg, float conf_thres, float e0, float e1, unsigned char* code, float* conf,
                                  float* pcls, float* ocls, float* s_iou, float* o_iou, float* a_iou, int64_t* det_hist, int64_t* cm,
                                  int64_t* lab_hist, int64_t cap, int64_t* cursor, int32_t* overflow, void* ws, size_t ws_bytes,
                                  hipStream_t stream)
{
    if (max_det < 0 || nl < 0 || nc < 1 || cap < 0) return RY_ERR_ARG;
    if (!(t_bg >= 0.f && t_bg < t_fg) || conf_thres != conf_thres || !(e0 <= e1)) return RY_ERR_ARG;     // NaN fails each
    if (nc > MAP_MAX_CLASSES || max_det >= INT_MAX || nl >= INT_MAX) return RY_ERR_UNSUPPORTED;
    if (!cls_off || !cursor || !overflow || !num || !ws || !det_hist || !cm || !lab_hist || (nl > 0 && !labels)) return RY_ERR_ARG;
    if (max_det > 0 && (!dets || !code || !conf || !pcls || !ocls || !s_iou || !o_iou || !a_iou)) return RY_ERR_ARG;
    if (ws_bytes < errors_workspace_bytes(max_det, nl)) return RY_ERR_WORKSPACE;
    unsigned char* base = reinterpret_cast<unsigned char*>(ws);
    BoxPrep* prep = ws_take<BoxPrep>(base, (size_t)nl * sizeof(BoxPrep));
    int32_t* owner = ws_take<int32_t>(base, (size_t)nl * 4);
    int32_t* cover = ws_take<int32_t>(base, (size_t)nl * 4);
    int32_t* lcls = ws_take<int32_t>(base, (size_t)nl * 4);
    float* w_s = ws_take<float>(base, (size_t)max_det * 4);
    int32_t* w_st = ws_take<int32_t>(base, (size_t)max_det * 4);
    float* w_o = ws_take<float>(base, (size_t)max_det * 4);
    int32_t* w_ot = ws_take<int32_t>(base, (size_t)max_det * 4);
    float* w_a = ws_take<float>(base, (size_t)max_det * 4);
    if (nl > 0)
        hipLaunchKernelGGL(errors_prep_kernel, dim3((unsigned)ry_cdiv(nl, 256)), dim3(256), 0, stream, labels, nl, nc, prep, owner, cover, lcls);
    if (max_det > 0) {
        hipLaunchKernelGGL(errors_best_kernel, dim3((unsigned)ry_cdiv(max_det, MATCH_WAVES)), dim3(64 * MATCH_WAVES), 0, stream, dets, num, max_det,
                           labels, prep, cls_off, nl, nc, t_fg, conf_thres, w_s, w_st, w_o, w_ot, w_a, owner);
        hipLaunchKernelGGL(errors_emit_kernel, dim3((unsigned)ry_cdiv(max_det, 256)), dim3(256), 0, stream, dets, num, max_det, labels, nl, nc, t_fg,
                           t_bg, conf_thres, w_s, w_st, w_o, w_ot, w_a, owner, cover, lcls, code, conf, pcls, ocls, s_iou, o_iou, a_iou, det_hist, cm,
                           cap, cursor);
    }
    if (nl > 0)
        hipLaunchKernelGGL(errors_label_kernel, dim3((unsigned)ry_cdiv(nl, 256)), dim3(256), 0, stream, labels, nl, nc, e0, e1, num, max_det, owner,
                           cover, lcls, lab_hist, cm, cap, cursor);
    hipLaunchKernelGGL(match_advance_kernel<SceneRule>, dim3(1), dim3(64), 0, stream, num, max_det, cap, cursor, overflow, SceneRule::Positives{});
    RY_CHECK_LAUNCH();
    return RY_OK;
}
