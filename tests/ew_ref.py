"""float64 references for the direct C-ABI tests of csrc/elementwise.hip (BatchNorm finalize / forward / backward, max pools, 2x
upsample), built from plain torch float64 operations that share no code with the kernels.  Every function works on whatever device
its inputs live on (the large cases keep their references on the GPU).

Besides the reference values, the BatchNorm functions return the per-element fp32 evaluation bound of the kernel's own formula
(the error the kernel may make BEFORE its single rounding to bf16); the tests add one bf16 ulp of the reference to it."""
import torch
import torch.nn.functional as F

LINEAR, MISH, LEAKY, SILU = 0, 1, 2, 3
ACTS = (LINEAR, MISH, LEAKY, SILU)


def act64(u, act):
    """act(u) and act'(u) in float64 (derivative by autograd).  torch's softplus threshold (20) is the kernel's Mish cut-off."""
    u = u.detach().double().requires_grad_(True)
    with torch.enable_grad():
        if act == MISH:
            f = F.mish(u)
        elif act == LEAKY:
            f = F.leaky_relu(u, 0.1)
        elif act == SILU:
            f = F.silu(u)
        else:
            f = u * 1.0
        (d,) = torch.autograd.grad(f.sum(), u)
    return f.detach(), d


# Evaluation error of the kernel's activation formulas (one v_exp_f32 of u * log2(e), one or two v_rcp_f32): the rounding of u * log2(e)
# moves e^u by up to |u| * log2(e) * 2^-24 relative, the exp and rcp approximations add a few 2^-24.  Relative to |act(u)| (value) and to
# max(|act'(u)|, 1) (derivative, which also suffers the cancellation in 1 - s and t^2 - 1).  LeakyReLU and linear are exact.
def act_eval_rel(u, act):
    if act in (MISH, SILU):
        return (2.0 * u.abs() + 16.0) * 2.0 ** -24
    return torch.zeros_like(u)


def bf16_ulp(x):
    """One bf16 ulp (8 significant bits) at |x|, floored at the smallest normal spacing."""
    e = torch.floor(torch.log2(x.abs().clamp_min(2.0 ** -126)))
    return torch.exp2(e - 7)


def round_bf16(x64):
    """float64 -> bf16, round to nearest even.  torch converts through fp32: exact for every lattice value of the tests; on random values
    the fp32 step can move a result that lies within 2^-24 of a bf16 midpoint, which the 1-ulp bounds absorb."""
    return x64.to(torch.float32).to(torch.bfloat16)


def f32(x64):
    return x64.double().to(torch.float32)


# ------------------------------------------------------------------------------------------------ BatchNorm forward finalize
def bn_finalize(partial, c0, C, count, eps, momentum, gamma, beta, rm=None, rv=None):
    """partial [rows][2][ld] (sum, sumsq) -> (mean, invstd, scale, shift) as the fp32 values the kernel must store, and the updated
    running statistics in float64 (compared with a bound: the kernel updates them with fp32 arithmetic).  mean and invstd are the float64
    values rounded once; scale = fp32(gamma * invstd); shift = beta - mean * scale rounded once (the kernel's fma)."""
    s = partial[:, 0, c0:c0 + C].double().sum(0)
    q = partial[:, 1, c0:c0 + C].double().sum(0)
    mean = s / count
    var = (q / count - mean * mean).clamp_min(0.0)
    invstd = f32(1.0 / torch.sqrt(var + float(torch.tensor(eps, dtype=torch.float32))))
    mean32 = f32(mean)
    sc = f32(gamma.double() * invstd.double())
    sh = f32(beta.double() - mean32.double() * sc.double())
    run = None
    if rm is not None:
        unb = var * count / (count - 1.0) if count > 1 else var
        m = float(torch.tensor(momentum, dtype=torch.float32))
        run = ((1 - m) * rm.double() + m * mean32.double(), (1 - m) * rv.double() + m * f32(unb).double())
    return mean32, invstd, sc, sh, run


# ------------------------------------------------------------------------------------------------ BatchNorm + activation
def _coef(co):
    co = co.double()
    return co[0], co[1], co[2], co[3]          # mean, invstd, scale, shift


def bn_act_fwd(y1, co1, act, y2=None, co2=None, res=None):
    """z = act(sc1*y1 + sh1 [+ sc2*y2 + sh2]) [+ res] in float64 and its fp32 evaluation bound:
    2^-22 * (|sc1 y1| + |sh1| + |sc2 y2| + |sh2|) * |act'(u)|  (u in fp32)  +  act_eval_rel * |act(u)|  +  2^-23 * (|act(u)| + |res|)."""
    _, _, sc1, sh1 = _coef(co1)
    a = y1.double()
    u = a * sc1 + sh1
    mag = (a * sc1).abs() + sh1.abs()
    if y2 is not None:
        _, _, sc2, sh2 = _coef(co2)
        b = y2.double()
        u = u + b * sc2 + sh2
        mag = mag + (b * sc2).abs() + sh2.abs()
    f, d = act64(u, act)
    eu = 2.0 ** -22 * mag
    bound = eu * d.abs() + act_eval_rel(u, act) * f.abs() + 2.0 ** -23 * f.abs()
    z = f
    if res is not None:
        z = z + res.double()
        bound = bound + 2.0 ** -23 * res.double().abs()
    return z, bound, u, eu


def leaky_kink(u, eu, act):
    """Elements whose fp32 u may land on the other side of LeakyReLU's kink at 0 (act' 1 against 0.1)."""
    if act != LEAKY:
        return torch.zeros_like(u, dtype=torch.bool)
    return u.abs() <= eu


def bn_act_bwd(dz, y1, co1, act, frozen, y2=None, co2=None):
    """Training-mode BatchNorm + activation backward sums in float64 with the statistics the forward used (mean and invstd = co[0], co[1],
    scale / shift = co[2], co[3]): g = dz * act'(u); S0 = sum g; S1 = sum g*y1; gx1 = invstd1 * (S1 - mean1 * S0) (S2, gx2 for the second
    branch); bco = (S0, gx1[, gx2]) * (1/M) rounded once (zero when frozen).  Also u, its fp32 evaluation error eu, g and eg, the absolute
    error of the kernel's fp32 g: act'' (<= 1.1 for Mish / SiLU) times eu, the activation's evaluation error, and 0.9 |dz| on LeakyReLU's
    kink.  The data gradient is apply_ref below (tests/test_ew_ref_cpu.py checks both against F.batch_norm's autograd)."""
    M = y1.shape[0]
    mu1, is1, sc1, sh1 = _coef(co1)
    a = y1.double()
    u = a * sc1 + sh1
    mag = (a * sc1).abs() + sh1.abs()
    if y2 is not None:
        mu2, is2, sc2, sh2 = _coef(co2)
        b = y2.double()
        u = u + b * sc2 + sh2
        mag = mag + (b * sc2).abs() + sh2.abs()
    _, d = act64(u, act)
    eu = 2.0 ** -22 * mag
    d64 = dz.double()
    g = d64 * d
    curv = 0.0 if act in (LINEAR, LEAKY) else 1.1
    kink = leaky_kink(u, eu, act)
    eg = d64.abs() * (curv * eu + 2 * act_eval_rel(u, act) + 0.9 * kink)
    S0 = g.sum(0)
    out = {"S0": S0, "gx": [is1 * ((g * a).sum(0) - mu1 * S0)], "u": u, "eu": eu, "g": g, "eg": eg, "kink": kink}
    if y2 is not None:
        out["gx"].append(is2 * ((g * b).sum(0) - mu2 * S0))
    rc = 1.0 / M
    out["bco"] = torch.stack([f32(torch.zeros_like(S0) if frozen else v * rc) for v in [S0] + out["gx"]])
    return out


def apply_ref(g, y, co, mg, mx):
    """dy = sc * (g - mg - (y - mean) * invstd * mx) in float64, and the fp32 evaluation bound of the kernel's sc*g + A*y + Bc with
    A = -sc*invstd*mx and Bc = sc*(invstd*mx*mean - mg) formed in fp32: 2^-22 * (|sc g| + |A y| + |A mean| + |Bc| + |sc mg|)."""
    mu, is_, sc, _ = _coef(co)
    y = y.double()
    A, Bc = -sc * is_ * mx, sc * (is_ * mx * mu - mg)
    dy = sc * (g - mg - (y - mu) * is_ * mx)
    return dy, 2.0 ** -22 * ((sc * g).abs() + (A * y).abs() + (A * mu).abs() + Bc.abs() + (sc * mg).abs())


# ------------------------------------------------------------------------------------------------ max pool
def maxpool(x, k, stride, pad, rows_per_chunk=None):
    """x [NB, H, W, C] (any float dtype; compared in fp32, which holds every bf16 value) -> z [NB, OH, OW, C] float32 and the FIRST-maximum
    window offset dy*k + dx (torch.argmax over the unfolded windows, -inf padding).  Floor mode.  rows_per_chunk bounds the unfolded copy."""
    NB, H, W, C = x.shape
    OH, OW = (H + 2 * pad - k) // stride + 1, (W + 2 * pad - k) // stride + 1
    xp = F.pad(x.float().permute(0, 3, 1, 2), (pad, pad, pad, pad), value=float("-inf"))
    z = torch.empty(NB, OH, OW, C, dtype=torch.float32, device=x.device)
    idx = torch.empty(NB, OH, OW, C, dtype=torch.int64, device=x.device)
    step = rows_per_chunk or OH
    for r0 in range(0, OH, step):
        r1 = min(OH, r0 + step)
        win = xp[:, :, r0 * stride:(r1 - 1) * stride + k].unfold(2, k, stride).unfold(3, k, stride)    # [NB, C, r, OW, k, k]
        win = win[:, :, :, :OW].reshape(NB, C, r1 - r0, OW, k * k)
        i = torch.argmax(win, dim=-1)
        z[:, r0:r1] = win.gather(-1, i[..., None])[..., 0].permute(0, 2, 3, 1)
        idx[:, r0:r1] = i.permute(0, 2, 3, 1)
    return z, idx


def maxpool_bwd(idx, dz, H, W, k, stride, pad):
    """dx [NB, H, W, C] float64: every output's gradient added to the input its window offset names (scatter in float64)."""
    NB, OH, OW, C = idx.shape
    oh = torch.arange(OH, device=idx.device).view(1, OH, 1, 1)
    ow = torch.arange(OW, device=idx.device).view(1, 1, OW, 1)
    ih = oh * stride - pad + idx // k
    iw = ow * stride - pad + idx % k
    n = torch.arange(NB, device=idx.device).view(NB, 1, 1, 1)
    c = torch.arange(C, device=idx.device).view(1, 1, 1, C)
    lin = (((n * H + ih) * W + iw) * C + c).reshape(-1)
    dx = torch.zeros(NB * H * W * C, dtype=torch.float64, device=idx.device)
    dx.index_add_(0, lin, dz.reshape(-1).double())
    return dx.view(NB, H, W, C)


# ------------------------------------------------------------------------------------------------ nearest 2x upsample
def upsample2x(x):
    """[NB, H, W, C] -> [NB, 2H, 2W, C] by repetition."""
    return x.repeat_interleave(2, dim=1).repeat_interleave(2, dim=2)


def upsample2x_bwd(dz):
    """[NB, 2H, 2W, C] -> [NB, H, W, C]: the sum of each 2x2 block in float64."""
    NB, H2, W2, C = dz.shape
    return dz.double().view(NB, H2 // 2, 2, W2 // 2, 2, C).sum((2, 4))
