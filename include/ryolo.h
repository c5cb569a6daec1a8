/*
 * ryolo.h — C ABI of libryolo_hip.so (MI355X / gfx950 hot path of yingkunwu/R-YOLOv4).
 *
 * The reference has no C ABI of its own: its boundary is three Python call surfaces plus one torch-op schema
 * (SURVEY.md §8b).  Each entry point below names the reference interface it replaces (paths in /root/reference).
 *
 * Conventions (all entry points):
 *   - plain C, raw DEVICE pointers + explicit sizes, a hipStream_t; no torch types;
 *   - returns 0 on success, RY_ERR_* otherwise; never throws, never allocates, never synchronises:
 *     all outputs and workspaces are caller-allocated (query *_workspace_bytes first), so every call is
 *     hipGraph-capturable;
 *   - re-entrant across streams; the library keeps no mutable global state.
 */
#ifndef RYOLO_H
#define RYOLO_H
#include <stddef.h>
#include <stdint.h>
#include "ryolo_params.h"

#ifdef __cplusplus
extern "C" {
#endif

typedef struct ihipStream_t* ryolo_stream_t;   /* == hipStream_t */

#define RYOLO_OK 0
#define RYOLO_ERR_ARG 1
#define RYOLO_ERR_WORKSPACE 2
#define RYOLO_ERR_LAUNCH 3
#define RYOLO_ERR_UNSUPPORTED 4

/* ------------------------------------------------------------------------------------------------------------
 * Rotated NMS / SkewIoU — replaces torch.ops.detectron2.nms_rotated / box_iou_rotated
 * (detectron2 is un-vendored; call sites lib/general.py:177, test.py:135, dead code lib/loss.py:241).
 * Boxes are (xc, yc, w, h, angle_degrees), float32.
 * ------------------------------------------------------------------------------------------------------------ */
int ryolo_nms_workspace_bytes(int batch, int64_t nmax, size_t* bytes);

/* boxes [batch, nmax, 5] already sorted by score descending (lib/general.py:166-168);
 * counts [batch] (device, may be NULL = all nmax valid); gt_only=1: suppress iff IoU > thr (detectron2 CUDA kernel),
 * 0: IoU >= thr (detectron2 CPU kernel); keep [batch, keep_stride] receives POSITIONS in the sorted order, ascending;
 * at most max_keep (<=0: no cap) are produced (lib/general.py:178-179 keeps max_det=1500); num_keep [batch] (device). */
int ryolo_nms_rotated_batched(const float* boxes, const int32_t* counts, int batch, int64_t nmax, float iou_thr,
                              int gt_only, int64_t max_keep, void* workspace, size_t workspace_bytes, int64_t* keep,
                              int64_t keep_stride, int32_t* num_keep, ryolo_stream_t stream);

/* Cluster owners of the NMS that has just run: owner [batch, nmax] int32, per row b and sorted position p
 *   p >= counts[b]                     -1
 *   p kept                             p
 *   otherwise                          the smallest kept k < p whose suppression bit (k, p) is set (IoU > thr with gt_only, >= thr without:
 *                                      the very decision the NMS took; such a k exists by the greedy construction)
 * The bits are read from the mask ryolo_nms_rotated_batched left in its workspace ([batch][nmax][ceil(nmax / 64)] u64, upper triangle), so
 * the contract is: same workspace, same stream, same batch / nmax / counts, directly after that call, with its keep / keep_stride /
 * num_keep, and the NMS not cut short (max_keep <= 0 or >= nmax, keep_stride >= the number kept): a position left undecided by a capped
 * NMS gets -1.  No IoU is evaluated again. */
int ryolo_nms_owner(const int32_t* counts, int batch, int64_t nmax, const void* workspace, size_t workspace_bytes, const int64_t* keep,
                    int64_t keep_stride, const int32_t* num_keep, int32_t* owner, ryolo_stream_t stream);

/* IoU[n, m] row-major = pairwise_iou_rotated(b1[n,5], b2[m,5]) (test.py:135).
 * workspace >= align256(n*48) + m*48 bytes. */
int ryolo_box_iou_rotated(const float* b1, int n, const float* b2, int m, void* workspace, size_t workspace_bytes,
                          float* out, ryolo_stream_t stream);

/* out[i] = IoU(b1[i], b2[i]) — the element-wise SkewIoU score of the commented-out block lib/loss.py:233-245. */
int ryolo_diag_iou_rotated(const float* b1, const float* b2, int n, float* out, ryolo_stream_t stream);

/* mAP evaluation (test.py:102-149 `get_batch_statistics`): true-positive matrix for a whole batch in one launch.
 * preds [npred,7] = (x, y, w, h, theta_rad, score, cls), images concatenated, each image score-descending (post_process order);
 * pred_off / tgt_off [batch+1] row offsets (int64, device); targets [ntgt,7] = (img, cls, x, y, w, h, theta_rad) grouped by image in
 * the caller's order; iouv [niou] ascending thresholds (device); tp [npred,niou] bytes out.  Class ids must be integers in
 * [0, num_classes), num_classes <= 256.  Side effect of the reference kept: theta of preds becomes degrees in place for images
 * that have both predictions and labels (test.py:126). */
int ryolo_map_match_workspace_bytes(int64_t npred, int64_t ntgt, size_t* bytes);
int ryolo_map_match(float* preds, const int64_t* pred_off, const float* targets, const int64_t* tgt_off, int batch, int64_t npred,
                    int64_t ntgt, const float* iouv, int niou, int num_classes, unsigned char* tp, void* workspace, size_t workspace_bytes,
                    ryolo_stream_t stream);

/* AP from the concatenated statistics (test.py:16-99 `ap_per_class` + `compute_ap`), on the device: confidence sort (score desc, index
 * asc), per-class cumulative hits, recall = hits / (n_labels + 1e-16), precision = hits / rank, precision envelope, trapezoid over the
 * 101-point recall grid for every IoU threshold, and precision / recall at the first threshold interpolated over `conf_grid` (the
 * reference's 1000-point px) — numpy's float64 expressions restated (np.interp, pairwise-summed np.trapz).
 * tp [n][niou] bytes, conf / pred_cls [n] fp32, target_cls [nl] fp32 (class ids: integers in [0, nc), nc <= 256), recall_grid [101] and
 * conf_grid [nconf] float64 on the device (np.linspace values from the host).  Out, all classes 0 .. nc-1 (the caller keeps those with
 * n_labels > 0, like np.unique(target_cls)): ap [nc][niou], prec_at / rec_at [nc][nconf] (zero rows for classes without labels or
 * predictions), n_labels [nc], n_pred [nc].  No host synchronisation. */
int ryolo_ap_workspace_bytes(int64_t n, int niou, int nc, size_t* bytes);
int ryolo_ap_per_class(const unsigned char* tp, const float* conf, const float* pred_cls, int64_t n, const float* target_cls, int64_t nl,
                       int nc, int niou, const double* recall_grid, const double* conf_grid, int nconf, void* workspace, size_t workspace_bytes,
                       double* ap, double* prec_at, double* rec_at, int64_t* n_labels, int64_t* n_pred, ryolo_stream_t stream);

/* The matching of `get_batch_statistics` (test.py:130-145) for ONE full scene — thousands of detections and labels — spread over the
 * chip, its rows appended to device-side accumulators; nothing is read back (lib/scene_eval.py).
 * dets [max_det,7] = (x, y, w, h, theta_rad, score, cls), score descending (TiledDetector.run_async's `out`); num [1] its count on the
 * device, clamped to [0, max_det]; rows >= *num are never read.  dets is only read: theta goes to degrees in registers.
 * labels [nl,6] = (cls, x, y, w, h, theta_rad) GROUPED BY CLASS ascending, the caller's order kept inside a class; cls_off [nc+1] int32
 * (device): class c owns rows [cls_off[c], cls_off[c+1]).  nl == 0 is legal (labels may be NULL).  nc <= 256, niou <= 16
 * (RYOLO_ERR_UNSUPPORTED beyond); iouv [niou] ascending (device).
 * Rule.  best(i) = the label of detection i's own class with the largest IoU (theta of both as theta / 3.14159274f * 180.f, the pair
 * function of the NMS); a detection whose class is not an integer in [0, nc) (NaN included), or whose class has no label, has none.
 *   owner(t) = the SMALLEST detection index i with best(i) == t and IoU(i, t) > iouv[0]
 *   tp[i][k] = owner(best(i)) == i  &&  IoU(i, best(i)) > iouv[k]
 * This is the reference's walk in score order: a candidate is a true positive iff its best label is not yet claimed, and one whose best
 * label is taken stays a false positive — it never falls back to the second best — so who gets a label does not depend on the walk.
 * Ties.  Equal IoU: the first label in the caller's order inside the class (what torch.max returns).  Equal score: detections keep
 * their row order, i.e. the smaller row claims first.  IoU exactly equal to a threshold is not above it.
 * Accumulators (cap rows): tp [cap][niou] bytes, conf [cap] = score, pcls [cap] = cls; cursor [1] int64 and overflow [1] int32 on the
 * device, zeroed by the caller before the first scene.  With n = min(*num, max_det) and cur = *cursor the rows cur .. cur + n - 1 are
 * written and the cursor advances by n; if cur + n > cap nothing is written, the cursor stays and *overflow = 1.
 * Launches: label prologue + owner reset, one wave per detection (best label, one atomicMin on owner), a thread per detection (rows), the
 * cursor.  Deterministic.  Every index that comes from data (cls_off entries, the class, *num, the stored best label) is clamped or
 * checked before it addresses memory: a bad table gives wrong numbers, not a fault. */
int ryolo_scene_match_workspace_bytes(int64_t max_det, int64_t nl, size_t* bytes);
int ryolo_scene_match(const float* dets, const int32_t* num, int64_t max_det, const float* labels, const int32_t* cls_off, int64_t nl, int nc,
                      const float* iouv, int niou, unsigned char* tp, float* conf, float* pcls, int64_t cap, int64_t* cursor, int32_t* overflow,
                      void* workspace, size_t workspace_bytes, ryolo_stream_t stream);

/* The matching of the DOTA / VOC protocol for ONE full scene, in ryolo_scene_match's launch shape and with its accumulators
 * (lib/dota_eval.py; tests/dota_eval_ref.py restates it in numpy).  dets / num / max_det / cls_off / nc / niou / iouv / cap / cursor /
 * overflow: as for ryolo_scene_match; dets is only read.
 * labels [nl,15] = (cls, difficult, quad x1 y1 .. x4 y4, rect x y w h theta_rad) GROUPED BY CLASS ascending, the caller's order kept
 * inside a class.  The quad is used as annotated when its eight coordinates are finite and it is strictly convex (the four edge cross
 * products all of one non-zero sign); otherwise the four corners of `rect` (its xyxyxyxy2xywha rectangle, or the caller's box when the
 * labels were boxes: quad = NaN) take its place.  Either orientation is accepted (normalised by the sign of the shoelace area).
 * Rule, per threshold k.  IoU(i, t) in float64: the corners of detection i's rectangle, x + (dx cos + dy sin), y + (dy cos - dx sin) with
 * (dx, dy) = (-+h/2, -+w/2), are clipped against label t's quad by four Sutherland-Hodgman half-plane steps (a vertex on an edge is
 * inside; at most 8 vertices); IoU = inter / (area_det + area_label - inter), 0 when that denominator is <= 0.  Pairs with disjoint
 * axis-aligned bounds have IoU 0 without the clip, and so has every pair with a non-finite detection rectangle or label.
 *   best(i)     = the label of detection i's class with the largest IoU, difficult labels included; none for a class that is not an
 *                 integer in [0, nc) (NaN included) or has no label
 *   owner_k(t)  = the SMALLEST i with best(i) == t and IoU(i, t) > iouv[k]
 *   status[i][k] = 2 (ignored)  if IoU(i, best) > iouv[k] and best is difficult
 *                  1 (TP)       if IoU(i, best) > iouv[k], best is not difficult and owner_k(best) == i
 *                  0 (FP)       otherwise: a duplicate, an IoU at or below the threshold, no best label, a bad class
 *   npos[c]    += the labels of class c that are not difficult (int64 [nc] on the device, zeroed by the caller before the first scene)
 * Ties.  Equal IoU: the first label in the caller's order inside the class.  Equal score: the smaller row claims first.  IoU exactly
 * equal to a threshold is not above it; thresholds are float32 values compared in float64.
 * Accumulators: status [cap][niou] bytes, conf [cap], pcls [cap]; rows cur .. cur + n - 1 are written and the cursor advances by n; if
 * cur + n > cap nothing is written, the cursor and npos stay and *overflow = 1.  max_det == 0 is legal: only npos moves.
 * Launches: label prologue (quad or rectangle, orientation, vertices / area / bounds in float64, owner[nl][niou] reset), one wave per
 * detection (clip, first maximum, one atomicMin per threshold exceeded), a thread per detection (rows), the cursor and npos.
 * Deterministic, no float atomics, no host read, capturable.  Every index that comes from data is clamped or checked as in
 * ryolo_scene_match.  After the call the first max_det doubles of the workspace hold IoU(i, best(i)) per detection row (-1: no label
 * of its class; rows >= *num are not written) — read by the tests. */
int ryolo_dota_match_workspace_bytes(int64_t max_det, int64_t nl, int niou, size_t* bytes);
int ryolo_dota_match(const float* dets, const int32_t* num, int64_t max_det, const float* labels, const int32_t* cls_off, int64_t nl, int nc,
                     const float* iouv, int niou, unsigned char* status, float* conf, float* pcls, int64_t cap, int64_t* cursor,
                     int32_t* overflow, int64_t* npos, void* workspace, size_t workspace_bytes, ryolo_stream_t stream);

/* The error breakdown of ONE full scene, in ryolo_scene_match's launch shape and with its inputs (lib/scene_errors.py;
 * tests/scene_errors_ref.py restates it in numpy): why the scene's mAP is what it is.  dets / num / max_det / labels [nl,6] / cls_off /
 * nl / nc / cap / cursor / overflow: as for ryolo_scene_match; dets is only read.  Scalars, float32 by value: t_fg, t_bg with
 * 0 <= t_bg < t_fg (foreground / background IoU), conf_thres, and the size edges e0 <= e1 as label areas in px^2 (RYOLO_ERR_ARG
 * otherwise, NaN included).
 * IoU is ryolo_scene_match's: theta of both as theta / 3.14159274f * 180.f, the pair function of the NMS, 0 for boxes whose inflated
 * circumscribed circles do not meet.  Every comparison with a threshold is "above" (>): an IoU equal to a threshold is not above it.
 * Per detection i < n = min(max(*num, 0), max_det):
 *   active(i) = score_i >= conf_thres (a NaN score is inactive)
 *   same(i)   = (s_iou, s_t): the first maximum over the labels of detection i's own class — best(i) of ryolo_scene_match; none
 *               (-1, -1) for a class that is not an integer in [0, nc) (NaN included) or that has no label
 *   other(i)  = (o_iou, o_t): the first maximum, in row order, over the label rows in [cls_off[0], cls_off[nc]) (clamped to [0, nl])
 *               that are outside detection i's class range; for a detection with an invalid class these are all of them; none: (-1, -1)
 *   a_iou(i)  = with s_t >= 0, the larger of IoU((x_i, y_i, w_i, h_i, theta_L), label s_t) and IoU((x_i, y_i, h_i, w_i, theta_L),
 *               label s_t), theta_L the angle of label s_t (prepared exactly as the label's own): the detection turned to the label's
 *               angle, the second box resolving (w, h, theta) ~ (h, w, theta +- pi/2); -1 otherwise
 *   owner(t)  = the SMALLEST active i with s_t == t and s_iou > t_fg
 * code[i], the first that applies:   0 BELOW  not active
 *                                    1 TP     s_iou > t_fg and owner(s_t) == i
 *                                    2 DUP    s_iou > t_fg (an earlier detection owns the label)
 *                                    3 CLS    o_iou > t_fg (right place, wrong class)
 *                                    4 ANG    s_iou > t_bg and a_iou > t_fg (right place and size, wrong angle)
 *                                    5 LOC    s_iou > t_bg
 *                                    6 BOTH   o_iou > t_bg
 *                                    7 BKG    otherwise
 * status of label row t, the first that applies:  0 FOUND t has an owner;  1 CONFUSED some detection with code CLS has o_t == t;
 *   2 MISLOCATED some detection with code ANG or LOC has s_t == t;  3 MISSED otherwise.  Size bucket of a label:
 *   (w*h >= e0) + (w*h >= e1) in float32.  The class of a label row is its cls column; a row whose cls is not an integer in [0, nc)
 *   is counted nowhere.
 * Rows behind the cursor (cap each): code bytes; conf = score, pcls = cls, ocls = the cls column of label o_t or -1; s_iou, o_iou,
 * a_iou.  Histograms, int64 on the device, zeroed by the caller before the first scene, added to:
 *   det_hist [nc+1][8]     row = the predicted class (row nc: a class that is not an integer in [0, nc)), column = code
 *   cm [nc+1][nc+1]        cm[true][pred]: TP -> [c][c]; CLS -> [class(o_t)][c]; DUP, ANG, LOC, BOTH, BKG -> [nc][c]; a label that is
 *                          not FOUND -> [class(t)][nc]; detections with an invalid class and BELOW rows are not counted
 *   lab_hist [nc][3][4]    class, size bucket, status
 * With cur = *cursor the rows cur .. cur + n - 1 are written and the cursor advances by n; if cur + n > cap NOTHING moves — no row, no
 * histogram, no cursor — and *overflow = 1.  max_det == 0 is legal: only the label side moves, every label MISSED.
 * Launches: label prologue (prepared labels, owner / cover word reset), one wave per detection (ONE pass over the rows of every class
 * keeping both first maxima, the two turned IoUs on two lanes, one atomicMin), a thread per detection (code, row, atomicOr on the cover
 * word, histograms counted per workgroup in LDS and flushed once), a thread per label (status, histogram), the cursor.  Integer
 * atomics only: deterministic; no host read; capturable.  Every index that comes from data (cls_off entries, the classes, *num, the
 * stored s_t / o_t) is clamped or checked as in ryolo_scene_match.  nc <= 256 (RYOLO_ERR_UNSUPPORTED beyond). */
int ryolo_scene_errors_workspace_bytes(int64_t max_det, int64_t nl, size_t* bytes);
int ryolo_scene_errors(const float* dets, const int32_t* num, int64_t max_det, const float* labels, const int32_t* cls_off, int64_t nl, int nc,
                       float t_fg, float t_bg, float conf_thres, float e0, float e1, unsigned char* code, float* conf, float* pcls, float* ocls,
                       float* s_iou, float* o_iou, float* a_iou, int64_t* det_hist, int64_t* cm, int64_t* lab_hist, int64_t cap, int64_t* cursor,
                       int32_t* overflow, void* workspace, size_t workspace_bytes, ryolo_stream_t stream);

/* VOC AP from the accumulated rows of ryolo_dota_match, on the device.  status [n][niou] bytes (1 TP, 2 ignored, anything else FP),
 * conf / pred_cls [n] fp32, npos [nc] int64 (device), grid11 [11] float64 on the device (np.arange(0., 1.1, 0.1) from the host).
 * Per class c and threshold k: the rows of class c by confidence descending (equal confidence: the earlier row first), rows with
 * status 2 skipped; running counts tpc / fpc; rec = tpc / npos[c]; prec = tpc / max(tpc + fpc, 2.220446049250313e-16).
 *   metric 0 (voc07): ap = 0; for t in grid11: ap = ap + max(prec[rec >= t], 0 when there is none) / 11.0
 *   metric 1 (voc12): mrec = [0, rec.., 1], mpre = [0, prec.., 0] made non-increasing from the right; the sum of
 *                     (mrec[j+1] - mrec[j]) * mpre[j+1] over the j where mrec changes, added in ascending order one after the other
 * Out: ap [nc][niou] float64 (NaN for a class with npos <= 0, 0 for one with positives and no counted row), n_pred [nc] int64 = rows of
 * each class, ignored ones included.  n < 2^31 - 1, nc <= 256, niou <= 16.  No host synchronisation. */
int ryolo_ap_voc_workspace_bytes(int64_t n, int niou, int nc, size_t* bytes);
int ryolo_ap_voc(const unsigned char* status, const float* conf, const float* pred_cls, int64_t n, const int64_t* npos, int nc, int niou,
                 int metric, const double* grid11, void* workspace, size_t workspace_bytes, double* ap, int64_t* n_pred, ryolo_stream_t stream);

/* ------------------------------------------------------------------------------------------------------------
 * YoloLayer — replaces model/yololayer.py:15-56 (YoloCSLLayer.forward) and :66-105 (YoloKFIoULayer.forward).
 * ------------------------------------------------------------------------------------------------------------ */
/* in [batch, na*attrs, gs, gs] (NCHW conv output) -> out [batch, na, gs, gs, attrs]
 * == out[i].view(bs,na,attrs,gs,gs).permute(0,1,3,4,2).contiguous()  (model/yololayer.py:25, :76).
 * (The conv stack of this library emits that layout directly from the head-conv epilogue.) */
int ryolo_head_permute(const float* in, float* out, int batch, int na, int attrs, int gs, ryolo_stream_t stream);

/* Eval-time decode of ONE scale into its row slice of infer_out [batch, rows_per_image, nc+6]:
 * mode 0 = csl  (attrs = nc+185: x,y,w,h,obj,cls[nc],theta[180]; first-max argmax, model/yololayer.py:28-54),
 * mode 1 = kfiou(attrs = nc+6  : x,y,w,h,a,obj,cls[nc]; angle scale 0.5236, no norm_angle, :79-103).
 * head [batch, na, gs, gs, attrs]; anchors_host = HOST pointer to na*3 floats (w, h, angle_rad; csl ignores angle),
 * grid units (model/yolo.py:54-72); rows of this scale start at row_offset (scale order 8 -> 16 -> 32). */
int ryolo_decode(int mode, const float* head, float* infer_out, int batch, int na, int gs, int nc, float stride,
                 const float* anchors_host, int64_t row_offset, int64_t rows_per_image, ryolo_stream_t stream);

/* ------------------------------------------------------------------------------------------------------------
 * post_process stages — replace the per-image loop of lib/general.py:153-181.
 * ------------------------------------------------------------------------------------------------------------ */
/* pred [batch, M, nc+6] is MUTATED: cls *= obj (lib/general.py:155).  key[b,i] = max_k cls (first max) if it is
 * > conf_thres (strict, :161) else -inf; cls[b,i] = argmax as float; count[b] = number of passing candidates. */
int ryolo_pp_score(float* pred, int batch, int64_t M, int nc, float conf_thres, float* key, float* cls,
                   int32_t* count, ryolo_stream_t stream);

/* Score ordering on the device (csrc/topk.hip) — the `argsort(descending=True)[:max_nms]` of lib/general.py:166-168 and the score
 * sort inside detectron2's nms_rotated, ties broken by ascending index.  Workspace for both: ryolo_sort_workspace_bytes
 * (rows, n) with n = K resp. N.
 * ryolo_topk_desc: per row of key [batch, M] the K <= 16384 largest entries in (key desc, index asc) order -> skey [batch, K]
 * (-inf padded), order [batch, K] (-1 padded), nsel [batch] = entries selected (null ok); key == -inf is never selected.
 * ryolo_argsort_desc: order [N] = stable descending argsort of scores [N]. */
int ryolo_sort_workspace_bytes(int rows, int64_t n_sorted, size_t* bytes);
int ryolo_topk_desc(const float* key, int batch, int64_t M, int K, float* skey, int64_t* order, int32_t* nsel, void* workspace,
                    size_t workspace_bytes, ryolo_stream_t stream);
int ryolo_argsort_desc(const float* scores, int64_t N, int64_t* order, void* workspace, size_t workspace_bytes, ryolo_stream_t stream);

/* sorted_key/order (row stride `stride` >= K) = the top-K of key along M in (key desc, index asc) order.  Writes dets [batch,K,7] =
 * (x,y,w,h,theta_rad,score,cls) and rboxes [batch,K,5] = NMS boxes with class offset cls*max_wh on x,y and theta in
 * degrees (lib/general.py:166-174); count[b] is clamped to K. */
int ryolo_pp_gather(const float* pred, const float* sorted_key, const int64_t* order, const float* cls, int batch,
                    int64_t M, int nc, int64_t K, int64_t stride, float max_wh, float* dets, float* rboxes, int32_t* count,
                    ryolo_stream_t stream);

/* out [batch, keep_stride, 7]: out[b,j] = dets[b, keep[b,j]] for j < num_keep[b], zeros after (lib/general.py:181). */
int ryolo_pp_emit(const float* dets, const int64_t* keep, const int32_t* num_keep, int batch, int64_t K,
                  int64_t keep_stride, float* out, ryolo_stream_t stream);

/* ------------------------------------------------------------------------------------------------------------
 * Conv stack — replaces every nn.Conv2d / nn.BatchNorm2d / activation / MaxPool2d / Upsample / torch.cat of
 * model/utils.py:6-282, model/backbone.py, model/neck.py (cuDNN/ATen under the reference).  Activations are NHWC
 * bf16 with an explicit channel stride; parameter blocks are defined in ryolo_params.h.
 * ------------------------------------------------------------------------------------------------------------ */
/* implicit-GEMM convolution: forward (taps = kernel window), data gradient (mirrored taps, stride-2 as 4 parity
 * classes on grid.z).  Epilogues (p->epi): 0 raw bf16, 1 raw + per-tile BatchNorm partial sums, 2 folded-BN + activation,
 * 3 fp32 + bias (detection heads), 4 bf16 accumulate (tensor with several consumers). */
int ryolo_conv_gemm(const ConvGemmParams* p, ryolo_stream_t stream);
/* UPPER BOUND of the [2][Nout] partial-statistics rows epilogue 1 writes for an M x Nout problem (sizing only: the exact count, which
 * the reduction must use, depends on the tile ryolo_conv_gemm picks and is ryolo_conv_gemm_plan's stats_rows) */
int ryolo_conv_gemm_stats_rows(int64_t M, int Nout, int pipe, int* rows);
/* which kernel ryolo_conv_gemm runs for *p and the number of partial-statistics rows its epilogue 1 writes; `kernel` may be null.
 * *kernel & 0xff: 0 generic implicit GEMM, 1 the 3x3 stride-1 halo-patch kernel (pipe bit 0x200, eligible layers), 2 the weight-stationary
 * persistent 1x1 kernel (RYOLO_GEMM_WS and its tapped / pool-gradient instantiations), 3 the persistent weight-stationary 3x3 kernel for 64 -> <= 64
 * channels (conv3x3_ws.hip), 4 the 256-wide 8-wave pointwise kernel (gemm256.hip), 5 the streaming 3x3 stride-2 forward for 32 input channels
 * (conv3x3s2_c32.hip), 6 that layer's space-to-depth data gradient; for 0, 1 and 4 bits 16-19 = tile columns / 32; for 0 also bit 0x100 = the 1x1
 * instantiation and bits 12-15 = tile rows / 64.  stats_rows: pixel tiles (0, 1, 4), waves (2), workgroups (3, 5, 6) */
int ryolo_conv_gemm_plan(const ConvGemmParams* p, int* stats_rows, int* kernel);
/* weight gradient: split-K over output pixels into p->partial ([splitk][Cout][taps*Cin] fp32, size from _plan), then a
 * deterministic reduction that accumulates into the torch-layout .grad [Cout][Cin][kh*kw] (no float atomics). */
int ryolo_conv_wgrad_plan(const WgradParams* p, int* splitk, size_t* workspace_bytes);
int ryolo_conv_wgrad(const WgradParams* p, ryolo_stream_t stream);
/* which kernel ryolo_conv_wgrad launches for *p: 0 generic split-K (register-staged, or the LDS-DMA pointwise form), 1 the 3x3 stride-1 halo-ring
 * kernel (needs p->zeros), 2 the tapped LDS-DMA kernel (tapped / strided layers with > 64 output channels; needs p->zeros), 3 the 8-wave
 * 256 x 256-tile pointwise kernel (stride-1 1x1 layers with Cin >= 256 and Cout > 128; needs p->zeros).  (4, the parity-plane ring kernel for 3x3
 * stride-2 layers, was retired in round 6 and is no longer returned.)  Answers RY_OK with kernel 0 also for blocks ryolo_conv_wgrad rejects. */
int ryolo_conv_wgrad_kernel(const WgradParams* p, int* kernel);
/* which instantiation of that kernel, from the same decision the launch switches on (host only, like the plan).  *word & 0xff = the kernel code above;
 * kernel 0: bits 8-11 = output-channel tile / 64 (1: conv_wgrad_kernel<64, .>, 2: the 128-channel tiles), bits 12-15 = 0 register-staged with tap
 * addressing, 1 register-staged with pointwise addressing (conv_wgrad_kernel<., true>), 2 wgrad1x1_dma_kernel<32>, 3 wgrad1x1_dma_kernel<64>;
 * kernel 1: bits 8-11 = 0 the 4-wave kernels, 2 / 4 conv3x3_wgrad8_kernel<2 | 4>, bits 12-15 = its prefetch steps (1 or 2; 0 on 4 waves),
 * bit 16 = 64-pixel K steps (conv3x3_wgrad64_kernel; always set on 8 waves), bit 17 = the <= 64 output-channel form (two slabs per K range),
 * bit 18 = mirrored ring head; kernels 2 and 3 have one instantiation each (no further bits).  Returns the status ryolo_conv_wgrad_plan returns. */
int ryolo_conv_wgrad_variant(const WgradParams* p, int* word);
/* launch shape of that kernel: workgroups, waves per workgroup (8: a workgroup holds its CU exclusively and the grid is sized to part of the chip) */
int ryolo_conv_wgrad_grid(const WgradParams* p, int* workgroups, int* waves);
/* weights of a stride-2 3x3 (pad 1) data gradient in its space-to-depth form (ConvGemmParams.s2d_cin): w fp32 [Cout][Cin][3][3] ->
 * out bf16 [4 * Cin][4][round_up(Cout, 32)] */
int ryolo_pack_s2d(const float* w, int Cout, int Cin, bf16_t* out, ryolo_stream_t stream);

/* first layer, 3x3 stride 1 pad 1 on the fp32 NCHW image (Cin = 3, Cout <= 32), without the im2col round trip (csrc/stem.hip);
 * _plan: partial-statistics rows of epilogue 1 and the weight-gradient workspace; _wgrad needs Cout == 32 and W % 16 == 0 and
 * leaves dW in the [Cout][32] GEMM layout in p->scratch (ryolo_unpack_wgrad adds it to the torch-layout .grad). */
int ryolo_stem3x3_plan(int NB, int H, int W, int Cout, int* stats_rows, size_t* wgrad_workspace_bytes);
int ryolo_stem3x3_fwd(const StemParams* p, ryolo_stream_t stream);
int ryolo_stem3x3_wgrad(const StemWgradParams* p, ryolo_stream_t stream);
/* the whole backward of that layer (BatchNorm + activation backward, BatchNorm parameter gradients, weight gradient) in one pass over
 * dz with the conv output recomputed from the image: Cout == 32, W % 32 == 0 (ryolo_stem3x3_bwd_plan returns UNSUPPORTED otherwise) */
int ryolo_stem3x3_bwd_plan(int NB, int H, int W, int Cout, size_t* workspace_bytes);
int ryolo_stem3x3_bwd(const StemBwdParams* p, ryolo_stream_t stream);

/* training BatchNorm2d (eps, momentum of nn.BatchNorm2d; model/utils.py:17): partial [rows][2][C] (the buffer must have
 * room for 64 more rows: fold scratch for big layers) -> coeffs [4][C] =
 * mean, invstd, scale = gamma*invstd, shift = beta - mean*scale; running_mean/var updated in place (unbiased var). */
int ryolo_bn_finalize(const float* partial, int rows, int C, double count, float eps, float momentum, const float* gamma,
                      const float* beta, float* running_mean, float* running_var, float* coeffs, ryolo_stream_t stream);
/* the same for channels [c0, c0 + C) of partial rows that are [2][ld] wide: sibling convolutions of a block that read the same input
 * (ELAN / CSP / C3 / SPPCSPC cv1 + cv2, model/utils.py:49-143,264-282) are emitted as ONE GEMM with concatenated output channels;
 * each BatchNorm finalizes its own slice into its own coeffs [4][C] */
int ryolo_bn_finalize_slice(const float* partial, int rows, int ld, int c0, int C, double count, float eps, float momentum,
                            const float* gamma, const float* beta, float* running_mean, float* running_var, float* coeffs,
                            ryolo_stream_t stream);
/* eval BatchNorm2d: coeffs from the running statistics */
int ryolo_bn_eval_coeffs(const float* gamma, const float* beta, const float* running_mean, const float* running_var, float eps,
                         int C, float* coeffs, ryolo_stream_t stream);
/* ... into channels [c0, c0 + C) of a shared coeffs [4][ld] (folded-BN epilogue of a shared GEMM launch) */
int ryolo_bn_eval_coeffs_slice(const float* gamma, const float* beta, const float* running_mean, const float* running_var, float eps,
                               int C, float* coeffs, int ld, int c0, ryolo_stream_t stream);
/* z = act(bn1(y1) [+ bn2(y2)]) [+ residual]   (Conv / RepConv / Bottleneck of model/utils.py) */
int ryolo_bn_act_fwd(const BnActParams* p, ryolo_stream_t stream);
int ryolo_bn_act_bwd_blocks(int64_t M, int C, int* nblk, int* rows_per_block);
/* backward of the above: dy1 [, dy2] [, dres], dgamma/dbeta accumulated; p->partial needs (nblk+64)*K*C floats, bco 3*C.
 * frozen=1: the coefficients came from ryolo_bn_eval_coeffs (fixed affine map, no batch-statistics coupling).
 * p->dy1 == NULL (single branch, no residual): statistics only — bco [2][C] = mean g, mean g*xhat and dgamma/dbeta are produced and
 * the apply pass is left to the consumer (ryolo_stem3x3_wgrad with StemWgradParams.y set). */
int ryolo_bn_act_bwd(const BnActParams* p, float* dgamma1, float* dbeta1, float* dgamma2, float* dbeta2, float* bco,
                     int frozen, ryolo_stream_t stream);

int ryolo_maxpool_fwd(const PoolParams* p, ryolo_stream_t stream);      /* nn.MaxPool2d k2 s2 / k5,9,13 s1 (utils.py:152,231-233) */
int ryolo_maxpool_bwd(const PoolParams* p, ryolo_stream_t stream);
int ryolo_upsample2x_fwd(const UpParams* p, ryolo_stream_t stream);     /* nn.Upsample(scale_factor=2) nearest (neck.py) */
int ryolo_upsample2x_bwd(const UpParams* p, ryolo_stream_t stream);
/* first layer (Cin = 3): fp32 NCHW image -> bf16 [NB*OH*OW][Kpad] patches, k = (r*kw + s)*Cin + c */
int ryolo_im2col(const float* img, int NB, int Cin, int H, int W, int kh, int kw, int stride, int pad, int OH, int OW, int Kpad,
                 bf16_t* col, ryolo_stream_t stream);
/* detection head tail: pre [M][ldp] fp32 (conv + bias) [* ImplicitM] -> [B, na, gs, gs, attrs] (yololayer.py:25 fused) */
int ryolo_head_finish_fwd(const float* pre, int ldp, const float* mul, int B, int gs, int na, int attrs, float* out,
                          ryolo_stream_t stream);
/* backward of the head tail: dpre (bf16 GEMM operand), and ACCUMULATED into dbias (conv bias gradient = column sums of dpre, may be
 * null) and dmul (ImplicitM gradient, with mul).  scratch >= (B*ceil(gs*gs/128) + 64) * 2*na*attrs floats; dpre pad columns
 * (>= na*attrs) must be pre-zeroed by the caller */
int ryolo_head_finish_bwd(const float* dout, const float* pre, int ldp, const float* mul, int B, int gs, int na, int attrs,
                          bf16_t* dpre, int ldd, float* dbias, float* dmul, float* scratch, ryolo_stream_t stream);
/* the same over the sparse description of dout that ryolo_loss leaves (LossParams.objgrad, ryolo_loss_owner_grids): only the dense rows of matched cells
 * (owner[cell] >= 0) are read from dout, every other cell is zero except its objectness element objgrad[cell] at index och.  preobj (may be null) =
 * the compact objectness column of pre written by ryolo_head_finish_fwd_obj: with it, pre is read at matched cells only.  Bit-identical results.
 * (the reference has no counterpart: autograd walks the dense maps, lib/loss.py:282-331 -> model/yololayer.py:25) */
int ryolo_head_finish_bwd_sparse(const float* dout, const float* objgrad, const int* owner, int och, const float* preobj, const float* pre, int ldp,
                                 const float* mul, int B, int gs, int na, int attrs, bf16_t* dpre, int ldd, float* dbias, float* dmul,
                                 float* scratch, ryolo_stream_t stream);
/* ryolo_head_finish_fwd + preobj [B, na, gs, gs] fp32 = pre[.., a*attrs + och] (och: 4 csl, 5 kfiou) and, if xobj is given, the same column of
 * out (after ImplicitM) — LossParams.headobj */
int ryolo_head_finish_fwd_obj(const float* pre, int ldp, const float* mul, int B, int gs, int na, int attrs, float* out, int och, float* preobj,
                              float* xobj, ryolo_stream_t stream);
/* parameter gradients of a detection head whose ImplicitM is applied by the GEMM epilogue (ConvGemmParams.head_attrs), out = (W (x + a) + b) m:
 * G [Cout][K] = weight gradient of the UNSCALED head gradient against x, s [Cout] = its column sums, a = ImplicitA [K] or null;
 * Ge = G + s (x) a; dW += m Ge, db += m s, dm += rowdot(W, Ge) + b s, da += W^T (m s); G and s are cleared.
 * (model/neck.py:173-186 ImplicitA / ImplicitM; autograd's chain through the add and the multiply) */
int ryolo_head_wgrad_finish(float* G, float* s, const float* W, const float* b, const float* m, const float* a, int Cout, int K, float* dW, float* db,
                            float* dm, float* da, ryolo_stream_t stream);
/* out[c] = b[c] + sum_k W[c][k] a[k]: the bias of a head with ImplicitA folded in (W (x + a) + b = W x + out) */
int ryolo_head_bias_fold(const float* W, const float* b, const float* a, int Cout, int K, float* out, ryolo_stream_t stream);
int ryolo_chan_add(const bf16_t* x, int ldx, const float* a, int64_t M, int C, bf16_t* z, int ldz, ryolo_stream_t stream);  /* ImplicitA */
/* out[c] += sum_m x[m][c] for c < Cvalid; C = readable (padded, multiple of 8) width; scratch >= (ceil(M/256) + 64)*C floats */
int ryolo_colsum_bf16(const bf16_t* x, int ldx, int64_t M, int C, int Cvalid, float* out, float* scratch, ryolo_stream_t stream);

/* inference re-parameterisation of RepConv (model/utils.py:189-215 leaves the 3 branches un-fused): w3 fp32 [Cout][Cin][3][3],
 * w1 fp32 [Cout][Cin], coa / cob = ryolo_bn_eval_coeffs of the two BatchNorms -> wf bf16 [Cout][9][Cin] (GEMM image of the merged
 * 3x3 kernel) and co_out [4][Cout] (scale 1, shift = shift3 + shift1) for the EPI_AFFINE_ACT epilogue */
int ryolo_repconv_fold(const float* w3, const float* w1, const float* coa, const float* cob, int Cout, int Cin, bf16_t* wf, float* co_out,
                       ryolo_stream_t stream);
/* fp32 master weights (torch layout) -> bf16 GEMM images, all convolutions in one launch */
int ryolo_pack_weights(const PackEntry* table_dev, int n, int64_t total, ryolo_stream_t stream);
int ryolo_unpack_wgrad(const float* scratch, int Cout, int Cin, int taps, int CinP, float* grad, ryolo_stream_t stream);
/* torch.optim.SGD(momentum, nesterov=True) of train.py:156 over flat buffers: buf = mu*buf + g; p -= lr*(g + mu*buf) */
int ryolo_sgd_nesterov(float* p, float* g, float* buf, int64_t n, float lr, float mu, float gscale, int zero_grad,
                       ryolo_stream_t stream);   /* g is scaled by gscale on read; zero_grad=1 clears it (optimizer.zero_grad fused) */
/* torch.optim.Adam(lr) of train.py:153-154 (betas / eps from the caller, no weight decay, no amsgrad) over flat buffers, `step` = 1, 2, ...
 * (the bias corrections 1 - beta^step are formed in double on the host, as torch does): m = m + (1 - b1)(g - m); v = b2 v + (1 - b2) g^2;
 * p -= lr / (1 - b1^step) * m / (sqrt(v) / sqrt(1 - b2^step) + eps).  gscale / zero_grad as in ryolo_sgd_nesterov. */
int ryolo_adam(float* p, float* g, float* m, float* v, int64_t n, double lr, double beta1, double beta2, double eps, int64_t step, float gscale,
               int zero_grad, ryolo_stream_t stream);
/* ---- image-side augmentations of the loader on uint8 HWC (BGR) images in HBM (csrc/augment.hip; datasets/base_dataset.py:224-330,
 * lib/augmentations.py:8-74).  paste: `rects` = device array of nrect records {int64 src_off; int src_w, sx, sy, dx, dy, w, h, canvas}
 * (ryolo_paste_rect_bytes = sizeof), canvases [ncanvas, CH, CW, 3] filled with `fill` first, rectangles applied in order (later wins).
 * warp: dst[b] = cv2.warpPerspective(src[b], M[b], (DW, DH), borderValue = border) with Minv[b] = inverse(M[b]) as 9 doubles.
 * hsv: BGR->HSV, lut [3][256] (hue, sat, val), HSV->BGR, in place.  mixup: out = uint8(a*r + b*(1-r)). */
int ryolo_paste_rects(const uint8_t* pool, const void* rects_dev, int nrect, uint8_t* canvas, int ncanvas, int CH, int CW, int fill,
                      ryolo_stream_t stream);
/* the same with the rectangles grouped by canvas (first_dev [ncanvas + 1] ints: canvas b owns rects[first[b] .. first[b + 1])): a canvas pixel looks at
 * its own canvas's <= 9 rectangles instead of the whole batch's table (what BaseDataset.assemble_batch uses: load_mosaic / load_mosaic9 of every sample) */
int ryolo_paste_rects_grouped(const uint8_t* pool, const void* rects_dev, int nrect, const int* first_dev, uint8_t* canvas, int ncanvas, int CH, int CW,
                              int fill, ryolo_stream_t stream);
int ryolo_paste_rect_bytes(int* bytes);
int ryolo_warp_perspective_u8(const uint8_t* src, int batch, int SH, int SW, const double* Minv, uint8_t* dst, int DH, int DW, int border,
                              ryolo_stream_t stream);
int ryolo_hsv_gain_u8(uint8_t* img, int64_t npix, const uint8_t* lut, ryolo_stream_t stream);
int ryolo_mixup_u8(const uint8_t* a, const uint8_t* b, double r, int64_t n, uint8_t* out, ryolo_stream_t stream);
/* pad_to_square (datasets/base_dataset.py:33-56): src [SH, SW, 3] resized (cv2.resize INTER_LINEAR semantics) to NH x NW and placed at
 * (top, left) of the OH x OW canvas filled with `fill` */
int ryolo_letterbox_u8(const uint8_t* src, int SH, int SW, int NH, int NW, int top, int left, uint8_t* dst, int OH, int OW, int fill,
                       ryolo_stream_t stream);
/* load_image for a whole batch (datasets/base_dataset.py:170-186): `items` = device array of nitems records {int64 src_off, dst_off; int SH,
 * SW, NH, NW, interp, lut} (ryolo_resize_item_bytes = sizeof): image at pool + src_off resized to NH x NW into stage + dst_off; interp
 * 0 = cv2.INTER_LINEAR, 1 = cv2.INTER_AREA (downscaling, generic float form), 2 = copy; lut >= 0: hsv tables luts[lut][3][256] applied
 * to the resized pixel (lib/augmentations.py:8-21).  max_pixels = largest NH * NW of the batch (grid size). */
int ryolo_resize_item_bytes(int* bytes);
int ryolo_resize_hsv_batch(const uint8_t* pool, const void* items_dev, int nitems, int64_t max_pixels, const uint8_t* luts, uint8_t* stage,
                           ryolo_stream_t stream);
/* label side of the sample composition for every label row of a batch, element-wise (load_target datasets/base_dataset.py:188-222, the
 * mosaic-9 crop :318-330, the vertex warp lib/augmentations.py:67-74): `rows` = device array of LabelRow records (csrc/augment.hip;
 * ryolo_label_row_bytes = sizeof), mats = 3x3 double matrices (row-major) indexed by LabelRow.mat; out [nrows][10] = (slot, class, 8
 * vertex coordinates), NaN vertices for rows a filter dropped (ryolo_encode_labels then removes them, keeping the order). */
int ryolo_label_row_bytes(int* bytes);
int ryolo_label_stage(const void* rows_dev, int64_t nrows, const double* mats, float* out, ryolo_stream_t stream);

int ryolo_struct_sizes(int* sizes /* [11] */);

/* ------------------------------------------------------------------------------------------------------------
 * Loss — replaces ComputeCSLLoss.__call__/build_targets (lib/loss.py:191-331) and ComputeKFIoULoss (:368-492),
 * bbox_ciou (:36-78), KFLoss (:100-150).  Forward + gradient w.r.t. the head maps in one call; items[6] =
 * reg, conf, cls, theta, total (already scaled by the hyp gains), and the number of target rows whose image index lies outside
 * [0, batch) — the reference raises IndexError on those (lib/loss.py:209,385), this library skips them and reports the count.
 *
 * Ignore regions (LossParams.ignore / ni / ign_count; the reference has none — the rule is this build's, restated in numpy by
 * tests/ignore_ref.py).  Row r = (image, x1, y1, x2, y2, x3, y3, x4, y4), coordinates normalised like targets[:, 2:6].  Per scale i:
 *   v        = fl32(coordinate * (float)gs[i]), ONE fp32 multiply, then promoted to double: the GRID coordinates (X_k, Y_k), k = 0..3
 *   S        = sum over k of (X_k * Y_k+1 - X_k+1 * Y_k) in vertex order, left to right, in double (the shoelace sum); s = +1 if S > 0 else -1
 *   LIVE     image > -1.0f and image < (float)batch (for every finite value: 0 <= (int)image < batch; a NaN image is not live), all eight
 *            coordinates finite, S != 0.  Any other row is DEAD: it covers nothing and is never an error, so a padded static table may end
 *            in NaN rows.  b = (int)image.
 *   centre   of cell (gj, gi): (cx, cy) = (gi + 0.5, gj + 0.5)
 *   INSIDE   min X_k <= cx <= max X_k and min Y_k <= cy <= max Y_k (the bounding box the kernel walks; implied by the edge tests for a
 *            convex quad), and for each of the four edges a -> b, a = vertex k, b = vertex k + 1:
 *                s * ((bx - ax) * (cy - ay) - (by - ay) * (cx - ax)) >= 0
 *            in double, each operation rounded on its own, no contraction (ryolo_paste_pixels' test).  Either vertex order works; a centre
 *            on an edge is inside.
 *   IGNORED  cell (b, a, gj, gi), for EVERY anchor a alike, iff no match owns it and its centre is inside some live row of image b.
 * An ignored cell adds exactly 0 to the objectness sum; its objectness gradient is exactly 0.0f in grad[] and in objgrad[]; the rest of its
 * grad[] row is zero as for any unmatched cell.  The objectness mean still divides by ALL cells of the scale: ignoring does not re-weight the
 * other cells.  Matched cells are untouched (the owner's score stays their target even under a row), and so are the box, class and theta
 * terms, the target assignment and the match records.  Works with compute_grad == 0 and with nt == 0.  Without rows the call issues the
 * launches it issued before and every output is bit-identical.  ign_count (optional) is zeroed by the call and receives, per scale, the
 * number of ignored cells.
 * ------------------------------------------------------------------------------------------------------------ */
int ryolo_loss_workspace_bytes(const LossParams* p, size_t* bytes);
int ryolo_loss(const LossParams* p, ryolo_stream_t stream);
/* owner grids of the last ryolo_loss call with THESE params on this workspace: owner[i][cell] >= 0 iff cell of scale i was matched to a target; an
 * unmatched cell holds -1, or -2 when the call ignored it (LossParams.ignore).  Readers test >= 0.  (Valid until the next ryolo_loss on the workspace) */
int ryolo_loss_owner_grids(const LossParams* p, const int** owner);
/* autograd chain rule of the loss node (lib/loss.py:256,414 return a [1] tensor; `loss.backward()` hands back d(out)/d(loss) as a
 * device scalar): grad[0..n) *= *scale, skipped ON THE DEVICE when *scale == 1.0f (the usual case) — no host read, capturable */
int ryolo_loss_grad_scale(float* grad, int64_t n, const float* scale, ryolo_stream_t stream);
/* the same for count <= 8 arrays (host arrays of device pointers / lengths) in ONE launch: the three maps and their compact objectness copies */
int ryolo_loss_grad_scale_multi(float* const* grads, const int64_t* n, int count, const float* scale, ryolo_stream_t stream);
/* match counters / records of the last ryolo_loss call with THESE params: count[i] -> one int, rec[i] -> [count][8] ints (b, a, gj, gi, cls, target
 * row, cell, pad) in the reference's enumeration order (lib/loss.py:275-310, :432-471); for tests of the target assignment */
int ryolo_loss_match_records(const LossParams* p, const int** count, const int** rec);

/* ------------------------------------------------------------------------------------------------------------
 * Data side (SURVEY.md §8(f) N2 slice, N4): the batch-finalisation end of BaseDataset.__getitem__ + collate_fn and the box
 * geometry of the detect path.  uint8 images and polygon targets come from whatever produced them (the reference's cv2 pipeline, or
 * a decoded cache resident in HBM); everything after them runs on the device.
 * ------------------------------------------------------------------------------------------------------------ */
/* imgs uint8 [B][H][W][3] BGR -> dst fp32 [B][3][H][W] RGB / 255; flags[b] bit0 = fliplr, bit1 = flipud (null: none).
 * Replaces np.fliplr / np.flipud (lib/augmentations.py:33-42), transpose + [::-1] + float() / 255 (datasets/base_dataset.py:155-157),
 * torch.stack (:166).  Bit-exact. */
int ryolo_to_tensor(const uint8_t* imgs, int B, int H, int W, const uint8_t* flags, float* dst, ryolo_stream_t stream);
/* targets fp32 [nt][10] = (image slot, class, x1, y1, ..., x4, y4) in pixels of the H x W network input, clockwise vertices ->
 * out [count][7 | 187] = (sample, class, x, y, w, h, theta [, csl x180]) in the reference's row order, *count on the device.
 * Replaces BaseDataset.filtering (:340-352, border (0, W, 0, H)), normalize (:354-361), the label half of horizontal_flip /
 * vertical_flip (flags[slot], as above), xyxyxyxy2xywha (lib/general.py:70-104), gaussian_label (base_dataset.py:13-31,143-149)
 * and collate_fn's sample index (:161-164; sample_of_img[slot], null = identity).  workspace: nt ints (csl only). */
int ryolo_encode_labels(const float* targets, int64_t nt, int H, int W, const uint8_t* flags, const int* sample_of_img, int csl,
                        float* out, int* count, int* workspace, ryolo_stream_t stream);
/* xyxyxyxy2xywha (lib/general.py:70-104) alone: clockwise polygons fp32 [n][8] -> (x, y, w, h, theta) fp32 [n][5] */
int ryolo_polys_to_xywha(const float* polys, int64_t n, float* out, ryolo_stream_t stream);
/* dets fp32 [n][7] = (x, y, w, h, theta, conf, cls) as post_process returns them; rescale != 0: rescale_boxes (lib/plot.py:9-31) in
 * place on columns 0-3 with shapes[img_of_det[i]] = original (h, w) and the padded network size current_dim; then
 * xywha2xyxyxyxy (lib/general.py:41-67, cv2.getRotationMatrix2D restated) -> polys fp32 [n][4][2]. */
int ryolo_dets_to_polys(float* dets, const int* img_of_det, const int* shapes, int current_dim, int rescale, int64_t n, float* polys,
                        ryolo_stream_t stream);

/* ------------------------------------------------------------------------------------------------------------
 * Full-scene (tiled) detection (csrc/tiled.hip; lib/tiled.py).  The reference detects on offline-cut patches only (data/DOTA.yaml,
 * detect.py letterboxes a whole file to img_size); these stages cut a scene into overlapping windows, feed them group by group to the
 * captured forward + post_process, and merge the per-window detections in scene coordinates with class-wise rotated NMS on the device.
 * A scene of T entries (an entry is a window seen through a view, below) in groups of B: T_pad = ceil(T / B) * B, candidate slot of
 * detection j of entry e = e * mk + j, ld = T_pad * mk.
 * ------------------------------------------------------------------------------------------------------------ */
/* Every window is cut, and its detections are collected, through one of the eight flip / 90-degree views (test-time orientation
 * ensembling; lib/tiled.py VIEWS; plain detection is view id), and the tables have one row per entry.  With win the S x S x 3 window
 * at the entry's origin (114 outside the scene: the fill turns with the window) and continuous coordinates (pixel i covers [i, i + 1)):
 *   code  name           pixels (numpy)                        view point (x, y) -> window point   theta' before the wrap
 *   0     id             win                                   (x, y)                              theta (bits unchanged)
 *   1     hflip          win[:, ::-1]                          (S - x, y)                          -theta
 *   2     vflip          win[::-1]                             (x, S - y)                          -theta
 *   3     rot180         win[::-1, ::-1]                       (S - x, S - y)                      theta (bits unchanged)
 *   4     transpose      win.transpose(1, 0, 2)                (y, x)                              pi/2 - theta
 *   5     rot90          np.rot90(win, 1)                      (S - y, x)                          theta + pi/2
 *   6     rot270         np.rot90(win, 3)                      (y, S - x)                          theta - pi/2
 *   7     antitranspose  np.rot90(win, 2).transpose(1, 0, 2)   (S - y, S - x)                      pi/2 - theta
 * w and h are carried over unchanged (h stays the long side).  For the six codes that change theta, theta' goes once through norm_angle's
 * two selects (lib/general.py:14-15): >= pi/2 -> subtract pi, then < -pi/2 -> add pi; fp32 with (float)pi/2 and (float)pi, one
 * operation per step.
 *
 * The cut: entries win0 .. win0 + count - 1 of the table win int64 [nwin][6] = (byte offset of the entry's source image from pool (any
 * alignment), its height, width, window origin x0, y0, view code) -> dst fp32 [>= count, 3, S, S]: slot k holds view `code` of the
 * window of entry win0 + k as RGB / 255 (114 / 255 outside the source image); slots >= count are not touched.  S % 4 == 0.  No
 * intermediate canvas; for code 0 bit-identical to ryolo_paste_rects(fill = 114) + ryolo_to_tensor.  Codes 0-3 are index arithmetic
 * (a reversed row is read forward and reversed in registers); codes 4-7 turn 32 x 32 pixel tiles through LDS.  The table lives on the
 * device and the call does not read it back: a row whose code is outside 0-7 leaves its slot untouched (lib/tiled.py validates the
 * names it encodes). */
int ryolo_tile_cut_views(const uint8_t* pool, const int64_t* win, int64_t win0, int count, int S, float* dst, ryolo_stream_t stream);
/* The collect: one group's post_process output dets [batch, mk, 7] / num [batch] (entries win0 .. win0 + batch - 1 of a scene of nwin
 * entries; geom fp32 [nwin][4] = (x0, y0, rate, view code), S the window size).  The row of a detection (x, y, w, h, theta, score, cls)
 * is mapped to its window point (px, py) and theta' by the table above, then shifted to scene pixels: cand [ld][7] row
 * ((px + x0) / rate, (py + y0) / rate, w / rate, h / rate, theta', score, cls) at slot (win0 + b) * mk + j, key [nc][ld] = score in the
 * row of the class, -inf in the others, fkey [ld] = -inf.  Slots past num[b], entries at or past nwin and entries whose code is outside
 * 0-7: zero rows, -inf keys.  Every slot of the group is written exactly once; no atomics, deterministic.  (win0 + batch) * mk <= ld. */
int ryolo_tile_collect_views(const float* dets, const int32_t* num, int batch, int64_t mk, const float* geom, int64_t win0, int64_t nwin,
                             int nc, int64_t ld, int S, float* cand, float* key, float* fkey, ryolo_stream_t stream);
/* skey / order [nc, K] = ryolo_topk_desc of key -> rboxes [nc, K, 5] = (x, y, w, h, theta degrees) of the selected candidates in scene
 * pixels, no class offset (zero rows for -inf entries): the input of ryolo_nms_rotated_batched with batch = nc. */
int ryolo_tile_merge_gather(const float* cand, const float* skey, const int64_t* order, int nc, int64_t K, float* rboxes, ryolo_stream_t stream);
/* kept positions keep [nc, keep_stride] / num_keep [nc] of that NMS -> fkey[order[c, keep[c, j]]] = skey[c, keep[c, j]] */
int ryolo_tile_mark(const float* skey, const int64_t* order, const int64_t* keep, const int32_t* num_keep, int nc, int64_t K,
                    int64_t keep_stride, float* fkey, ryolo_stream_t stream);
/* Cluster fusion (lib/tiled.py fuse = "box" | "wbf"): in place of ryolo_tile_mark, after ryolo_nms_owner.  Per class c, positions
 * p = 0 .. nsel[c] - 1 are in (score desc, slot asc) order, rows r_p = cand[order[c, p]] = (x, y, w, h, theta rad, s, cls), K the keep set
 * of the NMS and owner [nc, K] int32 its clusters: every selected candidate belongs to the cluster of exactly one kept box; candidates
 * not selected (beyond K per class) belong to none.  Cluster k, members in ascending position, the owner first; fp32, one operation
 * per arrow, no FMA contraction, constants (float)pi, (float)pi/2, (float)pi/4:
 *   m = 1; W = s_k; ax = 0; ay = 0; aw = s_k*w_k; ah = s_k*h_k; ad = 0
 *   for each further member i, ascending position:
 *       d = theta_i - theta_k;  if d >= pi/2: d = d - pi;   if d < -pi/2: d = d + pi          (both tests, in this order)
 *       (wi, hi) = (w_i, h_i)
 *       if d > pi/4: swap wi, hi; d = d - pi/2     else if d < -pi/4: swap wi, hi; d = d + pi/2
 *       W = W + s_i;  ax = ax + s_i*(x_i - x_k);  ay = ay + s_i*(y_i - y_k)
 *       aw = aw + s_i*wi;  ah = ah + s_i*hi;  ad = ad + s_i*d;  m = m + 1
 *   x = x_k + ax/W;  y = y_k + ay/W;  w = aw/W;  h = ah/W
 *   theta = theta_k + ad/W;  if theta >= pi/2: theta = theta - pi;  if theta < -pi/2: theta = theta + pi
 * (theta has period pi, and (w, h, theta) and (h, w, theta +- pi/2) are the same box: near-square objects come back both ways from the
 * transposing views.)  A cluster with m == 1 emits its row bit for bit, theta unwrapped as the plain collect pass leaves it.  The class
 * column is the owner's; the fused box stays in the owner's frame (no canonical w / h swap afterwards).
 * Score, mode 0 ("box"): the owner's score, bits unchanged.  Mode 1 ("wbf"): (W / (float)m) * ((float)min(m, n_ens) / (float)n_ens) with
 * n_ens = rates x views of the scene: the mean member score, scaled down when fewer boxes than ensemble members support it (also for
 * m == 1, whose geometry is still copied).
 * Writes fused [ld][7] and fkey [ld] at the owner's slot order[c, k] only, each once; cand is not modified (fused != cand); no atomics,
 * deterministic.  The final order is then ryolo_topk_desc of fkey (fused score desc, owner's slot asc) and ryolo_tile_emit with fused as
 * its cand argument.  keep_stride <= K.
 * Precondition: keep, order and nsel are the NMS's and ryolo_topk_desc's own outputs, so every kept position is < min(nsel[c], K) and
 * every slot order[c, p] of a selected position is in [0, ld).  The arrays live on the device and the call does not read them back: a kept
 * box whose position or slot is outside these ranges writes nothing (its slot of fused and fkey keeps what it held), and a member whose
 * slot is outside [0, ld) is counted in m but adds zero to every sum.  No access leaves the buffers either way. */
int ryolo_tile_fuse(const float* cand, const int64_t* order, const int32_t* nsel, const int64_t* keep, const int32_t* num_keep,
                    const int32_t* owner, int nc, int64_t K, int64_t keep_stride, int64_t ld, int mode, int n_ens, float* fused, float* fkey,
                    ryolo_stream_t stream);
/* Seam-aware merge (csrc/seam.hip; lib/tiled.py Seam(margin, cover, whole)): a window border cuts an object into a fragment that ends at
 * the border, and the overlapping neighbour sees the same object whole.  Two rules around the NMS, which itself is unchanged; off unless
 * asked for.  All arithmetic fp32, one operation per step, no FMA contraction.
 *
 * Slots and frames.  A slot is live when cls = cand[slot][6] satisfies 0 <= cls < nc (compared in fp32), c = (int)cls, and
 * key[c][slot] > -inf.  Its entry is e = slot / mk (live needs e < nwin), its own window the entry's (x0, y0) and rate r from geom, and
 * (Hr, Wr) = (win[e][1], win[e][2]) the resized extent of that rate.  Per live row (x, y, w, h, theta):
 *   cs = |(float)cos((double)theta)|;  sn = |(float)sin((double)theta)|
 *   ex = 0.5f * (cs*w + sn*h);  ey = 0.5f * (sn*w + cs*h)
 *   X = x*r;  Y = y*r;  EX = ex*r;  EY = ey*r;  xl = X - EX;  xr = X + EX;  yt = Y - EY;  yb = Y + EY
 * Cut bits, against the row's own window (a side on the border of the resized scene never cuts), x1 = x0 + S, y1 = y0 + S:
 *   1 (L): x0 > 0  and xl <= x0 + margin        2 (R): x1 < Wr and xr >= x1 - margin
 *   4 (T): y0 > 0  and yt <= y0 + margin        8 (B): y1 < Hr and yb >= y1 - margin
 * Rule 1, "seen whole elsewhere" (whole = 1): a row with a cut bit is redundant (bit 16) when some window (vx, vy) of the same rate has
 *   vx <= X < vx + S and vy <= Y < vy + S,   vx == 0 or xl > vx + margin,   vx + S >= Wr or xr < (vx + S) - margin,
 *   vy == 0 or yt > vy + margin,   vy + S >= Hr or yb < (vy + S) - margin.
 * Windows are the entries 0, nviews, 2 * nviews, ... (entries are window-major) and are ordered by rate (tile_plan): the windows of the
 * row's rate are the run around its own window whose geom rate equals r; windows of another rate are not consulted.  The row's own
 * window can never qualify (a cut side fails its own clearance).  Rule 1 trusts that the other window reported the object.
 * flags uint8 [ld] = the row's bits, 0 for a dead slot.  key2 is [nc + 1][ld].  whole = 1: rows 0 .. nc - 1 = key with -inf at (c, slot)
 * of every redundant row; they take key's place in the first ryolo_topk_desc of the merge and nothing else of the merge changes.
 * whole = 0: only the cut bits are set and rows 0 .. nc - 1 are not written.  Row nc is set to -inf in both cases: it is the final key
 * of the seam merge (what fkey is to the plain one: ryolo_tile_mark / ryolo_tile_fuse / ryolo_tile_seam_cover and the last
 * ryolo_topk_desc take it as their fkey).  fkey is reset by the collect pass only, and marks of another keep set would survive in it;
 * with a key of its own a seam merge neither sees the plain merge's marks nor leaves any, so the merges can follow each other on the
 * same collected scene in any order.  counts int32 [2] is zeroed (both words) and counts[0] receives the number of redundant rows
 * (integer atomics).  cand, key, win and geom are only read; key2 != key.  The window table is staged in LDS, 16 bytes per window:
 * more than 4096 windows are unsupported.  Capturable: no allocation, no host read. */
int ryolo_tile_seam_flags(const float* cand, const float* key, const int64_t* win, const float* geom, int64_t nwin, int nviews, int64_t mk,
                          int64_t ld, int nc, int S, float margin, int whole, uint8_t* flags, float* key2, int32_t* counts,
                          ryolo_stream_t stream);
/* Rule 2, "covered fragment": behind ryolo_tile_mark or ryolo_tile_fuse, on the candidates' own geometry (under fusion the fused rows are
 * not used).  Per class c, a and b range over the kept positions keep[c, 0 .. num_keep[c] - 1]; A and B are their rboxes rows as the NMS
 * saw them (degrees, no class offset), area = w*h.  A kept a whose slot order[c, a] has a cut bit in flags is dropped when some kept
 * b != a has area_b > area_a and cov >= cover, with
 *   iou = the pair function of the NMS on (prep(A), prep(B)), the cut box first
 *   s = area_a + area_b;  n = iou*s;  d1 = 1 + iou;  d = d1*area_a;  cov = n / d            (= intersection / area_a through the IoU)
 * The decision depends on the keep set alone (a box that is itself dropped still counts as a b), so it is order-free and deterministic.
 * A dropped a gets fkey[order[c, a]] = -inf (under fusion its cluster goes with it) and counts[1] is incremented (integer atomic;
 * ryolo_tile_seam_flags zeroed it).  Pairs whose inflated circumscribed circles do not meet are rejected before the pair function; cover
 * lies in [0.05, 1], far above the ~1e-10 artefacts the pair function can return for disjoint boxes.  A fragment absorbed by a whole box
 * in the NMS has already entered the sums of ryolo_tile_fuse.  keep_stride <= K.  workspace: ryolo_tile_seam_workspace_bytes(nc, K).
 * As in ryolo_tile_fuse the device tables are not trusted: a kept position outside [0, min(nsel[c], K)) or a slot outside [0, ld) is an
 * empty box that is never cut and covers nothing; no access leaves the buffers.  Capturable: no allocation, no host read. */
int ryolo_tile_seam_workspace_bytes(int nc, int64_t K, size_t* bytes);
int ryolo_tile_seam_cover(const float* rboxes, const int64_t* order, const int32_t* nsel, const int64_t* keep, const int32_t* num_keep, int nc,
                          int64_t K, int64_t keep_stride, const uint8_t* flags, int64_t ld, float cover, float* fkey, int32_t* counts, void* ws,
                          size_t ws_bytes, ryolo_stream_t stream);
/* order [>= num[0]] = ryolo_topk_desc of fkey, num [1] its selection count -> out [max_det, 7] = cand[order[j]] for j < num[0], zeros after */
int ryolo_tile_emit(const float* cand, const int64_t* order, const int32_t* num, int64_t max_det, float* out, ryolo_stream_t stream);

/* ------------------------------------------------------------------------------------------------------------
 * Training on full-size scenes (csrc/scene.hip; datasets/scene_dataset.py): the source image of a sample is a WINDOW of a scene in the
 * pool.  The reference has no such stage (it trains on windows cut offline); tests/scene_ref.py restates these semantics in numpy.
 * ------------------------------------------------------------------------------------------------------------ */
/* ryolo_resize_hsv_batch through a window: `items` = device array of nitems records {int64 src_off, dst_off; int SH, SW, NH, NW, interp, lut,
 * x0, y0, c, pad} (ryolo_window_item_bytes = sizeof): the SH x SW scene at pool + src_off (4-byte aligned for the wide copy path; any
 * alignment is correct), the window [x0, x0 + c) x [y0, y0 + c) in scene pixels, which may hang over any border (negative origins
 * included) or miss the scene.  BIT-IDENTICAL to cutting the c x c window first (114 wherever it lies outside the scene) and running
 * ryolo_resize_hsv_batch on the cut with {SH = SW = c, NH, NW, interp, lut}: copy, the exact 2 x integer block path, generic INTER_LINEAR, both
 * INTER_AREA forms, taps that straddle the scene border.  No intermediate cut is written.  The copy path (interp 2, NH = NW = c) moves 16
 * pixels per thread with 16-byte loads and stores, realigning the arbitrary source row start in registers; it never reads past the scene's
 * last byte.  dst_off multiples of 16 (what datasets/augment.py lays out) get the wide stores.  The copy path never consults c: an item with
 * interp 2 and (NH, NW) != (c, c) copies the NH x NW window at (x0, y0), with the same fill and the same bounds on every access.
 * interp 3, the ROTATED CUT (the record ends in `double minv[6]`, read by this mode only): pixel (x, y) of the NH x NW result is
 * cv::warpPerspective's INTER_LINEAR sample of the scene at (minv[0] x + minv[1] y + minv[2], minv[3] x + minv[4] y + minv[5]) with the
 * constant border 114, then the hsv tables when lut >= 0: BIT-IDENTICAL to ryolo_warp_perspective_u8 on the whole scene (B = 1, Minv =
 * {minv[0..5], 0, 0, 1}, border 114) followed by ryolo_hsv_gain_u8, and the sampler of ryolo_paste_pixels.  x0, y0, c are not read.  Items
 * of all four modes may share one table and one launch.  A workgroup walks 64 x 16 tiles of the result, a thread owns 4 adjacent pixels
 * and writes them as three dwords where the address allows (always with a dst_off multiple of 4 and NW a multiple of 4), bytes otherwise;
 * no access leaves the scene or the NH NW 3 bytes of the result. */
int ryolo_window_item_bytes(int* bytes);
int ryolo_resize_hsv_windows(const uint8_t* pool, const void* items_dev, int nitems, int64_t max_pixels, const uint8_t* luts, uint8_t* stage,
                             ryolo_stream_t stream);
/* Which labels of a scene belong to a window — IN PLACE on an uploaded LabelRow table (before ryolo_label_stage) whose polygons are in scene
 * pixels; row i belongs to window wins[win_of_row[i]], wins int32 [nwin][3] = (x0, y0, c), |x0|, |y0|, c < 2^24.  A row whose index is outside
 * [0, nwin) is dropped (poly = NaN, IoF 0, w0 / h0 untouched) without reading `wins`.  Per row:
 *   shift   p' = fl32(p - origin) per coordinate, fp32;
 *   clip    in fp64, the quad p' against [0, c]^2 by Sutherland-Hodgman, planes in the order x >= 0, x <= c, y >= 0, y <= c (a vertex on a
 *           plane is inside); a crossing on edge a -> b is t = (bound - a_k) / (b_k - a_k), the other coordinate a_o + t (b_o - a_o), the
 *           clipped coordinate the bound itself;
 *   ratio   IoF = min(1, |shoelace(clipped)| / |shoelace(quad)|), shoelace = sum of (x_k y_k+1 - x_k+1 y_k) in vertex order, left to right;
 *           either orientation.  |shoelace(quad)| <= 0 (or NaN): the row is dropped and reports IoF 0;
 *   result  IoF >= iof_thr: poly = p' (NOT clipped: the filters downstream handle polygons that reach past a canvas); otherwise poly = NaN,
 *           which ryolo_label_stage carries and ryolo_encode_labels removes in order.  w0 = h0 = c for every row.
 * iof_out (optional): double [nrows].  0 < iof_thr <= 1.  The host leaves out labels whose bounding box misses the window (IoF 0). */
int ryolo_scene_label_rows(void* rows_dev, int64_t nrows, const int32_t* win_of_row, const int32_t* wins, int nwin, double iof_thr,
                           double* iof_out, ryolo_stream_t stream);

/* ------------------------------------------------------------------------------------------------------------
 * Anchors fitted to a dataset, and the labels no anchor reaches (csrc/anchors.hip; lib/anchors.py).  The reference has no
 * such stage (its anchors are constants); tests/anchor_ref.py restates these semantics in numpy.  No allocation, no synchronisation,
 * capturable; no float atomics: every sum runs in a fixed order that depends on n alone, in double; counts are integers.
 * ------------------------------------------------------------------------------------------------------------ */
/* Which target rows the loss can assign.  Reads of `p` only: targets [nt][tcols] (normalised, the loss's layout), nt, tcols, na, anchors, gs,
 * mode.  counts int32 [nt][3]: per row and scale the number of anchors that pass the loss's rule — both side ratios max(r, 1 / r) < 4 with
 * r = fl32(t * gs) / anchor, modes != 0 also |cos(theta - anchor angle)| > 0.866, the float operations of the loss's target assignment.  The
 * image index (column 0) is NOT looked at.  summary int64 [5]: rows reached on scale 0, 1, 2; rows reached on no scale (lost); anchor
 * passes over all rows and scales.  nt == 0: summary is zeroed, counts untouched. */
int ryolo_anchor_reach(const LossParams* p, int32_t* counts, int64_t* summary, ryolo_stream_t stream);
/* Sizes wh float32 [n][2] in pixels of the network input (finite, > 0), anchor set k float32 [K][2], 1 <= K <= 32, 1 <= n < 2^31.  Per label
 * x = max over anchors of min(min(rw, 1 / rw), min(rh, 1 / rh)), r = wh / k in float32; the label is reached iff x > (float)(1 / thr).
 * stats (device, 4 x 8 bytes): [0] fitness = (1 / n) * sum of x over the reached labels, a DOUBLE; [1] reached labels, [2] (label, anchor)
 * pairs whose own minimum passes, [3] accepted generations, int64.  Workspace: ryolo_anchor_workspace_bytes. */
int ryolo_anchor_workspace_bytes(int64_t n, size_t* bytes);
int ryolo_anchor_fitness(const float* wh, int64_t n, const float* k, int K, double thr, void* workspace, size_t workspace_bytes, int64_t* stats,
                         ryolo_stream_t stream);
/* (1 + C) evolution strategy, 1 <= C <= 16, G >= 0 generations, mutation table v float32 [G][C][K][2] on the device: the children of
 * generation g are max(k * v[g][c], 2.0f); the child of greatest fitness (lowest c among equals) replaces k iff its fitness is strictly
 * greater than k's.  One pass over the labels and one single-workgroup launch per generation; the decision is made on the device.  k is
 * read and overwritten; stats as above, for the final k. */
int ryolo_anchor_evolve(const float* wh, int64_t n, float* k, int K, const float* v, int G, int C, double thr, void* workspace,
                        size_t workspace_bytes, int64_t* stats, ryolo_stream_t stream);
/* Lloyd's k-means on (w, h), n <= 2^24.  init != 0: k = the labels at ranks floor((j + 0.5) / K * n) of the labels in ascending order of
 * fl32(w * h) (ryolo_argsort_desc read backwards: among equal areas the HIGHER index comes first); else k holds the start.  Per iteration:
 * nearest centroid by fl32(dw * dw + dh * dh), unfused, lowest centroid among equals; new centroid = (float)(double sum / count); an empty
 * cluster keeps its centroid.  assign (optional, int32 [n]): the assignment the LAST iteration made. */
int ryolo_anchor_kmeans_workspace_bytes(int64_t n, size_t* bytes);
int ryolo_anchor_kmeans(const float* wh, int64_t n, float* k, int K, int iters, int init, int32_t* assign, void* workspace,
                        size_t workspace_bytes, ryolo_stream_t stream);

/* ------------------------------------------------------------------------------------------------------------
 * Object-level copy-paste for scene training (csrc/copypaste.hip; datasets/copy_paste.py).  The reference has no such
 * stage; tests/copy_paste_ref.py restates these semantics in numpy.  No allocation, no synchronisation, capturable, deterministic.
 * `items` = device array of np records {int64 src_off; int SH, SW, slot; float cls, quad[8]; double M[6], Minv[6]}
 * (ryolo_paste_item_bytes = sizeof): the source label `quad` (scene pixels) of the SH x SW scene at pool + src_off, the affine map
 * M (scene -> canvas, row major 2 x 3) and its inverse.  Items are sorted by slot, inside a slot in paste order; first int32 [B + 1]: slot b
 * owns items[first[b] .. first[b + 1]).  Item j is VALID when 0 <= slot < B, first[slot] <= j < first[slot + 1] <= np and SH, SW > 0; it
 * is LIVE when it is valid, its destination quad is finite and that quad's shoelace sum (sum of x_k y_k+1 - x_k+1 y_k, in vertex order,
 * double) is not zero.  An item that is not live writes no pixel and buries no row (an item whose slot lies outside [0, B) is IGNORED
 * in this sense, not rejected: the table is on the device and is not read back).
 * ------------------------------------------------------------------------------------------------------------ */
int ryolo_paste_item_bytes(int* bytes);
/* One thread per item: dq fp32 [np][8] = the destination quad, x' = M0 x + M1 y + M2, y' = M3 x + M4 y + M5 in double, left to right,
 * rounded to float (written for every item); bbox int32 [np][4] = (x0, y0, x1, y1), the canvas pixels x0 <= px < x1, y0 <= py < y1 with
 * ceil(min x') <= px <= floor(max x') clipped to [0, S); all zero for an item that is not live or whose box misses the canvas. */
int ryolo_paste_prepare(const void* items_dev, int np, const int32_t* first_dev, int B, int S, float* dq, int32_t* bbox, ryolo_stream_t stream);
/* canvas uint8 [B][S][S][3] (BGR, the assembler's finished canvases before ryolo_to_tensor), in place.  Pixel (px, py) of canvas `slot` is
 * INSIDE live item j when for the four edges a -> b of dq[j] promoted to double s ((bx - ax)(py - ay) - (by - ay)(px - ax)) >= 0, s = +-1
 * the sign of the quad's shoelace sum.  A pixel takes the LAST item of its slot that it is inside: it is written once, with
 * ryolo_warp_perspective_u8's sample for the inverse map (Minv; 0 0 1) and border 114 (taps outside the scene read 114); pixels inside
 * no item are not touched.  Launch: a grid over (item, 32 x 8 tile of its bbox) — work follows the pasted area, not B S S; max_bw x
 * max_bh (<= 0: the canvas) is the caller's bound on a box and only sizes the grid (an item with more tiles loops). */
int ryolo_paste_pixels(const uint8_t* pool, const void* items_dev, int np, const int32_t* first_dev, int B, const float* dq, const int32_t* bbox,
                       uint8_t* canvas, int S, int max_bw, int max_bh, ryolo_stream_t stream);
/* targets [nt][10] = (slot, class, 8 coordinates), NaN rows allowed -> out [nt + np][10]: rows 0 .. nt - 1 the existing rows in order, row
 * nt + j = (slot, cls, dq[j]) of item j; a row for an item that is not valid is (0, cls, NaN x 8).  A row is OCCLUDED by live item k of
 * its own slot when |shoelace(clip(row, dq[k]))| / |shoelace(row)| >= occ_thr: for an existing row every item of the slot counts, for
 * the row of item j the items k > j of the slot.  The coordinates of an occluded row become NaN (slot and class stay), which
 * ryolo_encode_labels removes in order.  A row with a NaN coordinate or with |shoelace| <= 0 is copied as it is.  The clip is fp64
 * Sutherland-Hodgman of the row's quad against the four half-planes of dq[k] in its edge order (0 -> 1, 1 -> 2, 2 -> 3, 3 -> 0); with
 * d(p) the edge expression above, a vertex with d >= 0 is inside, an edge whose ends differ adds a + t (b - a), t = d(a) / (d(a) - d(b));
 * at most 20 vertices are kept.  One thread per output row.  occ_thr > 0. */
int ryolo_paste_labels(const float* targets, int64_t nt, const void* items_dev, int np, const int32_t* first_dev, int B, const float* dq,
                       double occ_thr, float* out, ryolo_stream_t stream);

#ifdef __cplusplus
}
#endif
#endif /* RYOLO_H */
