"""Restatement in torch (any float dtype; the tests use float64) of the Gaussian box regressions of the fused loss — modes 3 KLD, 4 GWD,
5 ProbIoU of csrc/loss.hip, ryolov4_amd.lib.loss.ComputeKLDLoss / ComputeGWDLoss / ComputeProbIoULoss.  NO REFERENCE ORACLE EXISTS: the
reference has no code for any of the three; the definitions are this build's and this file is what the kernel is held to.

A box (x, y, w, h, theta) is the Gaussian N((x, y), R diag(w^2/4, h^2/4) R^T), R = [[c, -s], [s, c]] (lib/general.py xywhr2xywhrsigma).
`gauss_distance` is the closed form the kernel evaluates, `gauss_distance_matrix` the textbook matrix form it is checked against."""
import torch

from oracle import ref_ops

KINDS = ("kld", "gwd", "probiou")


def _clamp_wh(box):
    return box[:, 2].clamp(min=1e-4, max=1e4), box[:, 3].clamp(min=1e-4, max=1e4)


def gauss_distance(kind, pred, target, clamp=True):
    """pred, target [n, 5] -> D [n], clamped as the loss clamps it (>= 0 for kld / gwd, [1e-7, 100] for probiou) unless clamp=False."""
    wp, hp = _clamp_wh(pred)
    wt, ht = _clamp_wh(target)
    ap, bp, at, bt = wp ** 2 / 4, hp ** 2 / 4, wt ** 2 / 4, ht ** 2 / 4
    dx, dy = pred[:, 0] - target[:, 0], pred[:, 1] - target[:, 1]
    dr = pred[:, 4] - target[:, 4]
    c2, s2 = torch.cos(dr) ** 2, torch.sin(dr) ** 2
    e1, e2 = ap * at + bp * bt, ap * bt + bp * at
    T1 = e1 * c2 + e2 * s2                                  # tr(Sp St)
    T2 = e2 * c2 + e1 * s2                                  # det St * tr(St^-1 Sp)
    q = ap * bp * at * bt
    if kind == "kld":
        ct, st = torch.cos(target[:, 4]), torch.sin(target[:, 4])
        u, v = ct * dx + st * dy, -st * dx + ct * dy
        d = 0.5 * (u ** 2 / at + v ** 2 / bt + T2 / (at * bt) + torch.log(at * bt / (ap * bp))) - 1
        return d.clamp(min=0) if clamp else d
    if kind == "gwd":
        d = dx ** 2 + dy ** 2 + ap + bp + at + bt - 2 * torch.sqrt(T1 + 2 * torch.sqrt(q))
        return d.clamp(min=0) if clamp else d
    if kind == "probiou":
        cp, sp = torch.cos(pred[:, 4]), torch.sin(pred[:, 4])
        ct, st = torch.cos(target[:, 4]), torch.sin(target[:, 4])
        s00 = 0.5 * (ap * cp ** 2 + bp * sp ** 2 + at * ct ** 2 + bt * st ** 2)
        s11 = 0.5 * (ap * sp ** 2 + bp * cp ** 2 + at * st ** 2 + bt * ct ** 2)
        s01 = 0.5 * ((ap - bp) * cp * sp + (at - bt) * ct * st)
        det_s = 0.25 * (ap * bp + at * bt + T2)
        m = dx ** 2 * s11 - 2 * dx * dy * s01 + dy ** 2 * s00
        d = m / (8 * det_s) + 0.5 * torch.log(det_s / torch.sqrt(q))
        return d.clamp(min=1e-7, max=100) if clamp else d
    raise ValueError(kind)


def _sigma(box):
    w, h = _clamp_wh(box)
    c, s = torch.cos(box[:, 4]), torch.sin(box[:, 4])
    R = torch.stack((torch.stack((c, -s), -1), torch.stack((s, c), -1)), -2)
    return R @ torch.diag_embed(torch.stack((w ** 2 / 4, h ** 2 / 4), -1)) @ R.transpose(-1, -2)


def _sqrtm2(S):
    """Principal square root of a symmetric positive definite 2x2 matrix: (S + sqrt(det) I) / sqrt(tr + 2 sqrt(det))."""
    sd = torch.sqrt(torch.linalg.det(S))
    tr = S[:, 0, 0] + S[:, 1, 1]
    eye = torch.eye(2, dtype=S.dtype).expand_as(S)
    return (S + sd[:, None, None] * eye) / torch.sqrt(tr + 2 * sd)[:, None, None]


def gauss_distance_matrix(kind, pred, target):
    """The same distances from their textbook matrix forms (torch.linalg), unclamped."""
    Sp, St = _sigma(pred), _sigma(target)
    mu = (pred[:, :2] - target[:, :2])[:, :, None]
    if kind == "kld":
        Sti = torch.linalg.inv(St)
        tr = (Sti @ Sp).diagonal(dim1=-2, dim2=-1).sum(-1)
        maha = (mu.transpose(-1, -2) @ Sti @ mu)[:, 0, 0]
        return 0.5 * (tr + maha - 2 + torch.log(torch.linalg.det(St) / torch.linalg.det(Sp)))
    if kind == "gwd":
        rp = _sqrtm2(Sp)
        cross = _sqrtm2(rp @ St @ rp)
        tr = (Sp + St - 2 * cross).diagonal(dim1=-2, dim2=-1).sum(-1)
        return (mu[:, :, 0] ** 2).sum(-1) + tr
    if kind == "probiou":
        S = 0.5 * (Sp + St)
        maha = (mu.transpose(-1, -2) @ torch.linalg.inv(S) @ mu)[:, 0, 0]
        return maha / 8 + 0.5 * torch.log(torch.linalg.det(S) / torch.sqrt(torch.linalg.det(Sp) * torch.linalg.det(St)))
    raise ValueError(kind)


def loss_of_distance(kind, d):
    if kind == "probiou":
        return torch.sqrt(-torch.expm1(-d) + 1e-7)
    return 1 - 1 / (1 + torch.log1p(d))                     # tau = 1, f = log1p


def gauss_loss(kind, pred, target):
    """Per-match loss L [n]; the similarity (objectness target) is (1 - L).clamp(0)."""
    return loss_of_distance(kind, gauss_distance(kind, pred, target))


def compute_gauss_loss(kind, outputs, targets, anchors, nc, hyp):
    """The full loss, composed as oracle.ref_ops.compute_loss composes it for 'kfiou', in the dtype of `outputs`:
    outputs 3 x [B, na, gs, gs, nc + 6] (may require grad).  Returns (loss[1], dict of 0-d tensors)."""
    dt = outputs[0].dtype
    reg, conf, cls = torch.zeros(1, dtype=dt), torch.zeros(1, dtype=dt), torch.zeros(1, dtype=dt)
    tg = ref_ops.build_targets([(o.shape[2], o.shape[3]) for o in outputs], targets, anchors, "kfiou")
    fl = float(hyp.get("fl_gamma", 0.0))
    for i, pi in enumerate(outputs):
        m = tg[i]
        tconf = torch.zeros(pi.shape[:4], dtype=dt)
        n = m["b"].shape[0]
        if targets.shape[0] > 0 and n > 0:
            ps = pi[m["b"], m["a"], m["gj"], m["gi"]]
            anch, tbox = m["anch"].to(dt), m["tbox"].to(dt)
            pxy = ps[:, 0:2].sigmoid() * 2 - 0.5
            pwh = (ps[:, 2:4].sigmoid() * 2) ** 2 * anch[:, :2]
            pa = ref_ops.norm_angle((ps[:, 4:5].sigmoid() - 0.5) * 1.1 + anch[:, 2:])
            L = gauss_loss(kind, torch.cat((pxy, pwh, pa), -1), tbox)
            reg = reg + L.mean()
            score = (1 - L.detach()).clamp(0)
            flat = ((m["b"] * pi.shape[1] + m["a"]) * pi.shape[2] + m["gj"]) * pi.shape[3] + m["gi"]
            tc = tconf.view(-1)
            for k in range(n):                              # last writer wins on duplicate cells
                tc[flat[k]] = score[k]
            if nc > 1:
                onehot = torch.zeros(n, nc, dtype=dt)
                onehot[torch.arange(n), m["c"]] = 1
                cls = cls + ref_ops._bce_mean(ps[:, 6:6 + nc], onehot, hyp.get("cls_pw", 1.0), fl)
        conf = conf + ref_ops._bce_mean(pi[..., 5], tconf, hyp.get("obj_pw", 1.0), fl)
    reg, conf, cls = hyp["box"] * reg, hyp["obj"] * conf, hyp["cls"] * cls
    loss = reg + conf + cls
    return loss, {"reg_loss": reg, "conf_loss": conf, "cls_loss": cls, "total_loss": loss}
