"""The parameter blocks of the convolution entry points as pure functions of their arguments: tap tables, output geometry and ONE builder
per block (ConvGemmParams, WgradParams, StemParams).  No Graph, no allocation, no tape — engine/graph.py, the plan probes and tools/ all
describe a launch through these, so a question asked of a plan entry point and the launch that follows are the same block."""
from . import structs as S


def _taps_fwd(k, pad):
    return [(r - pad, s - pad, r * k + s) for r in range(k) for s in range(k)]


def _taps_dgrad_s1(k, pad):
    """Stride-1 data gradient: a correlation of dY with mirrored taps; weight slot r * k + c of the [Cin][tap][Cout] image."""
    return [(pad - r, pad - c, r * k + c) for r in range(k) for c in range(k)]


def _classes_dgrad_s2(k, pad):
    """Stride-2 data gradient as four output-parity classes [(taps, ph, pw)]: dx[2a + ph][2b + pw] sums only the taps (r, c) whose
    input row 2 oh - pad + r can be 2a + ph, i.e. (ph + pad - r) even (1 / 2 / 2 / 4 live taps for k = 3, pad = 1), read at
    dY[a + (ph + pad - r) / 2][b + (pw + pad - c) / 2]."""
    classes = []
    for ph in range(2):
        for pw in range(2):
            taps = [((ph + pad - r) // 2, (pw + pad - c) // 2, r * k + c) for r in range(k) for c in range(k)
                    if (ph + pad - r) % 2 == 0 and (pw + pad - c) % 2 == 0]
            classes.append((taps, ph, pw))
    return classes


def _taps_dgrad_s2d():
    """Space-to-depth form of the 3x3 stride-2 pad-1 data gradient (weights from ryolo_pack_s2d): 2 x 2 taps over the dY grid."""
    return [(da, db, 2 * da + db) for da in range(2) for db in range(2)]


def _fill_class(tc, taps, oh_add=0, ow_add=0):
    tc.ntaps = len(taps)
    tc.oh_add, tc.ow_add = oh_add, ow_add
    for i, (dh, dw, wi) in enumerate(taps):
        tc.dh[i], tc.dw[i], tc.widx[i] = dh, dw, wi


def conv_out(H, W, k, s, pad):
    return (H + 2 * pad - k) // s + 1, (W + 2 * pad - k) // s + 1


class Rows:
    """Geometry of a plain [N * H * W, ld] bf16 tensor, so that it can stand where a gathered operand (a TRef) is expected."""

    def __init__(self, N, H, W, ld):
        self.N, self.H, self.W, self.ld = N, H, W, ld
        self.span_bytes = N * H * W * ld * 2


def _scale_shift(co):
    """Rows 2 (scale) and 3 (shift) of a [4][C] fp32 BatchNorm coefficient tensor."""
    return co.data_ptr() + 2 * co.shape[1] * 4, co.data_ptr() + 3 * co.shape[1] * 4


def gemm_params(A, Aptr, W, Nout, wtaps, gemm_cin, OH, OW, stride, classes, epi, out_ptr, ldC, zeros, pipe, full=None, coeffs=None, act=0,
                bias=None, s2d=0, pool=None, head=None):
    """ConvGemmParams of one ryolo_conv_gemm launch but for `stats` (sized by the library's plan for this very block).  A: geometry of the
    gathered operand (N, H, W, ld, span_bytes) at Aptr; W: the bf16 weight image; classes: [(taps, oh_add, ow_add)]; full = (oh_mul, ow_mul,
    OHf, OWf) of a parity-class store; coeffs [4][Nout]; pool = (idx, dz, ldi, ld); head = (attrs, och, ImplicitM pointer or None, compact
    objectness pointer or None)."""
    p = S.ConvGemmParams()
    p.A, p.NB, p.IH, p.IW, p.Cin, p.ldA = Aptr, A.N, A.H, A.W, gemm_cin, A.ld
    p.W, p.Nout, p.wtaps = W.data_ptr(), Nout, wtaps
    p.OH, p.OW, p.sh, p.sw = OH, OW, stride, stride
    p.oh_mul, p.ow_mul, p.OHf, p.OWf = (1, 1, OH, OW) if full is None else full
    p.nclasses = len(classes)
    for i, (taps, oa, wa) in enumerate(classes):
        _fill_class(p.cls[i], taps, oa, wa)
    p.epi, p.out, p.ldC = epi, out_ptr, ldC
    if coeffs is not None:
        p.scale, p.shift = _scale_shift(coeffs)
    p.act, p.bias, p.zeros, p.pipe, p.s2d_cin = act, bias, zeros, pipe, s2d
    p.a_bytes, p.w_bytes = A.span_bytes, W.numel() * 2
    if head is not None:
        p.head_attrs, p.head_och, p.scale, p.stats = head
    if pool is not None:
        p.pool_idx, p.pool_dz, p.pool_ldi, p.pool_ld = pool
    return p


def wgrad_params(dy, dy_ptr, cout, cout_pad, x, x_ptr, cin, k, s, pad, dW, dW2=None, cout1=0):
    """WgradParams of one ryolo_conv_wgrad launch but for `zeros` and the split-K workspace (Graph._emit_wgrad).  dy / x: geometry (ld; N, H, W,
    ld) of the output gradient at dy_ptr and of the forward input at x_ptr; dW2 / cout1: second destination of a sibling pair, rows >= cout1."""
    p = S.WgradParams()
    p.dY, p.ldY, p.Cout, p.CoutPad = dy_ptr, dy.ld, cout, cout_pad
    p.X, p.NB, p.IH, p.IW, p.Cin, p.ldX = x_ptr, x.N, x.H, x.W, cin, x.ld
    p.OH, p.OW = conv_out(x.H, x.W, k, s, pad)
    p.sh, p.sw = s, s
    taps = _taps_fwd(k, pad)
    p.ntaps = len(taps)
    for i, (dh, dw, _) in enumerate(taps):
        p.dh[i], p.dw[i] = dh, dw
    p.dW, p.dW2, p.Cout1 = dW, dW2, cout1
    return p


def stem_params(img_ptr, NB, H, W, wf, cout, epi, out=None, stats=None, coeffs=None, act=0):
    """StemParams of one ryolo_stem3x3_fwd launch.  out: TRef (None: statistics only); stats: the partial rows of EPI_STATS; coeffs [4][cout]."""
    p = S.StemParams()
    p.img, p.NB, p.H, p.W = img_ptr, NB, H, W
    p.wf, p.Cout, p.epi = wf.data_ptr(), cout, epi
    if out is not None:
        p.out, p.ldC = out.ptr(), out.ld
    if stats is not None:
        p.stats = stats.data_ptr()
    if coeffs is not None:
        p.scale, p.shift = _scale_shift(coeffs)
        p.act = act
    return p
