"""GPU: teacher-forced layer check INSIDE the real training plans ("replace the vacuous train-mode backward test").

Whole-network batch-statistics BatchNorm at random init decorrelates any two roundings of the same computation (1 - cos between
the fp32 and the bf16-emulating ORACLES is ~0.9), so an end-to-end gradient comparison cannot be a parity criterion.  This test
removes the depth amplification instead of the network: the REAL plan of the full network runs — arena placement, the forked
forward branches, the weight-gradient side stream, merged sibling GEMMs, the stem recompute, the space-to-depth data gradient — and
around single launches of its tapes (Graph.probe) every conv + BatchNorm + activation node is fed the ORACLE's tensors:

  forward   before a convolution GEMM its input buffer is overwritten with the oracle's input activation; checked: the raw conv
            output y and the block output z = act(bn(y)) [+ residual]  (model/utils.py:6-32,35-46)
  backward  before a BatchNorm-backward launch the gradient of its block output is overwritten with the oracle's dL/dz; checked: dy,
            d gamma, d beta; before the weight / data gradient launches dy is overwritten with the oracle's; checked: dW and the
            data gradient this launch contributes to its input (accumulate targets are zeroed first)

against the bf16-storage-emulating torch-CPU oracle (tests/bf16_emu.py), rel-L2 <= 3e-2 per tensor (observed values are written to
gpurun_out/r03_teacher_forced.json).  The two plan features that move a node's reduction into ANOTHER node's launch (BatchNorm sums in
the completing data gradient's epilogue, MaxPool gradient in the sibling's store) are switched off here — with them a node's inputs
are consumed before they can be forced.  The first is no longer part of the plans; tests/gemm1x1_cases.py
(test_maxpool_gradient_in_the_store) holds the second to the plain pool backward."""
import json
import os

import pytest
import torch
import torch.nn as nn

from oracle import ref_model, ref_ops
from tests.bf16_emu import emulate_bf16
from ryolov4_amd.synth import CFG, HYP, fill_state, synth_targets

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TOL = 3e-2


def rel(a, b):
    a, b = a.detach().double().flatten().cpu(), b.detach().double().flatten().cpu()
    return float((a - b).norm() / (b.norm() + 1e-30))


def oracle_capture(orc, x, tg, nc, mode):
    """One train-mode forward + loss + backward of the bf16-emulating oracle; per nn.Conv2d: input x, raw output y, dL/dy, this conv's
    dL/dx; per Conv / Bottleneck / RepConv block: output z and dL/dz."""
    cap = {}

    def rec(name):
        return cap.setdefault(name, {})

    for n, m in orc.named_modules():
        if isinstance(m, nn.Conv2d):
            m.register_forward_hook(lambda mod, i, o, n=n: rec(n).update(x=i[0].detach(), y=o.detach()))
            m.register_full_backward_hook(lambda mod, gi, go, n=n: rec(n).update(dx=None if gi[0] is None else gi[0].detach(), dy=go[0].detach()))
        elif type(m).__name__ in ("Conv", "Bottleneck", "RepConv"):
            m.register_forward_hook(lambda mod, i, o, n=n: rec(n).update(z=o.detach()))          # after emulate_bf16's rounding hook
            m.register_full_backward_hook(lambda mod, gi, go, n=n: rec(n).update(dz=go[0].detach()))
    loss, items = ref_ops.compute_loss(orc(x, True), tg, orc.anchors, nc, mode, HYP)
    loss.backward()
    return cap, float(loss)


@pytest.mark.parametrize("ver,mode", [("yolov7", "kfiou"), ("yolov4", "csl")])
def test_every_conv_bn_act_node_of_the_training_plan_teacher_forced(ver, mode):
    from ryolov4_amd.engine import structs as S
    from ryolov4_amd.lib.loss import ComputeCSLLoss, ComputeKFIoULoss
    from ryolov4_amd.model.yolo import Yolo
    nc, B, Sz = 2, 4, 128
    net = Yolo(nc, CFG, mode, ver)
    sd = fill_state(net.state_dict())
    net.load_state_dict(sd)
    orc = ref_model.Yolo(nc, CFG, mode, ver)
    orc.load_state_dict(sd)
    emulate_bf16(orc)
    orc.train()
    x = torch.rand(B, 3, Sz, Sz, generator=torch.Generator().manual_seed(4))
    tg = synth_targets(B, 8, nc, mode == "csl", seed=6, img_size=Sz)
    cap, loss_o = oracle_capture(orc, x, tg, nc, mode)
    oparams, omods = dict(orc.named_parameters()), dict(orc.named_modules())

    net.to(DEV).train()
    rt = net.runtime()
    rt.record_tape = True
    rt.fuse_pool_grad = False
    g = rt.graph(B, Sz, Sz, True)
    names = {id(m): n for n, m in net.named_modules()}
    pnames = {id(p): n for n, p in net.named_parameters()}
    mods = dict(net.named_modules())

    # ---- what the plan knows about every convolution: (y, z, x) buffers, by pointer ---------------------------------------------
    convs = {}                         # conv name -> dict(y, z, x, conv, bn, block)
    for cid, (y, z, xin) in g.debug.items():
        n = names[cid]
        block = n.rsplit(".conv.", 1)[0] if ".conv." in n else None
        convs[n] = dict(y=y, z=z, x=xin, conv=mods[n], block=block)
    by_y = {c["y"].ptr(): n for n, c in convs.items() if c["x"] is not None}
    by_z = {}
    for n, c in convs.items():
        by_z.setdefault(c["z"].ptr(), []).append(n)
    # (gradient buffers are liveness-placed slots of the arena and SHARE addresses over time: backward launches are identified through
    # operands whose addresses are unique — the forward activation they re-read, the packed weight image, the flat gradient slice)
    by_dw = {rt.grad_ptr(c["conv"].weight): n for n, c in convs.items()}
    by_wd = {}
    for key, pk in rt._packed.items():
        if pk.get("group"):
            by_wd[pk["wd"].data_ptr()] = [names[id(m["conv"])] for m in pk["members"]]
        elif pk["wd"] is not None:
            by_wd[pk["wd"].data_ptr()] = [names[id(pk["conv"])]]
    for conv, img in rt._s2d.values():
        by_wd[img.data_ptr()] = [names[id(conv)]]

    def write(tref, nchw, grad=False):
        t = tref.buf.grad_tensor() if grad else tref.buf.t
        t.view(tref.N, tref.H, tref.W, tref.ld)[..., tref.c0:tref.c0 + tref.C] = nchw.permute(0, 2, 3, 1).to(device=DEV, dtype=torch.bfloat16)

    def read(tref, grad=False):
        torch.cuda.synchronize()
        return tref.to_nchw(grad).cpu()

    def zout(name):
        """oracle block output / its gradient for the device's z of conv `name`: the enclosing Bottleneck when the residual add is fused"""
        c = convs[name]
        blk = c["block"]
        parent = blk.rsplit(".", 1)[0] if blk else None
        if parent in cap and type(omods[parent]).__name__ == "Bottleneck" and blk.endswith(".cv2") and omods[parent].add:
            return cap[parent]
        if blk in cap and "z" in cap[blk]:
            return cap[blk]
        return None

    errs, probe = {}, {}
    fid, bid = id(g.fwd), id(g.bwd)

    def members(base, width, table):
        return sorted((n for p, n in table.items() if base <= p < base + 2 * width), key=lambda n: convs[n]["y"].c0)

    # ---- forward probes -----------------------------------------------------------------------------------------------------------
    for (tid, i), (name, args) in g.tape_args.items():
        if tid != fid:
            continue
        if name == "ryolo_conv_gemm":
            p = args[0]
            if p.epi == S.EPI_F32_BIAS:
                continue                                         # detection heads: tests/test_gpu_head.py
            mem = [n for n in members(p.out, p.Nout, by_y) if convs[n]["x"].ptr() == p.A]
            if not mem:
                continue

            def pre(mem=mem):
                write(convs[mem[0]]["x"], cap[mem[0]]["x"])

            def post(mem=mem):
                for n in mem:
                    errs[f"{n}:y"] = rel(read(convs[n]["y"]), cap[n]["y"])
            probe[(tid, i)] = (pre, post)
        elif name == "ryolo_bn_act_fwd":
            p = args[0]
            for n in by_z.get(p.z, []):
                ref = zout(n)
                if ref is None or p.y2:
                    continue

                def post(n=n, ref=ref):
                    errs[f"{n}:z"] = rel(read(convs[n]["z"]), ref["z"])
                probe[(tid, i)] = (None, post)

    # ---- backward probes ----------------------------------------------------------------------------------------------------------
    for (tid, i), (name, args) in g.tape_args.items():
        if tid != bid:
            continue
        if name == "ryolo_bn_act_bwd":
            q = args[0]
            if q.y2:
                continue                                         # RepConv (two branches into one activation): tests/test_gpu_blocks.py::rephead
            for n in ([by_y[q.y1]] if q.y1 in by_y else []):
                ref = zout(n)
                if ref is None or "dz" not in ref or convs[n]["x"] is None:
                    continue
                bn = mods[convs[n]["block"]].conv[1]

                def pre(n=n, ref=ref):
                    write(convs[n]["z"], ref["dz"], grad=True)

                def post(n=n, bn=bn):
                    errs[f"{n}:dy"] = rel(read(convs[n]["y"], grad=True), cap[n]["dy"])
                    torch.cuda.synchronize()
                    errs[f"{n}:dgamma"] = rel(rt.grad_view(bn.weight), oparams[pnames[id(bn.weight)]].grad)
                    errs[f"{n}:dbeta"] = rel(rt.grad_view(bn.bias), oparams[pnames[id(bn.bias)]].grad)
                probe[(tid, i)] = (pre, post)
        elif name == "ryolo_conv_wgrad":
            w = args[0]
            mem = [by_dw[q_] for q_ in (w.dW, w.dW2) if q_ and q_ in by_dw]
            mem = [n for n in mem if convs[n]["x"] is not None and "dy" in cap.get(n, {})]
            if not mem:
                continue

            def pre(mem=mem):
                for n in mem:
                    write(convs[n]["y"], cap[n]["dy"], grad=True)

            def post(mem=mem):
                torch.cuda.synchronize()
                for n in mem:
                    errs[f"{n}:dW"] = rel(rt.grad_view(convs[n]["conv"].weight), oparams[n + ".weight"].grad)
            probe[(tid, i)] = (pre, post)
        elif name == "ryolo_conv_gemm":
            p = args[0]
            mem = [n for n in by_wd.get(p.W, []) if n in convs and convs[n]["x"] is not None]
            mem = sorted(mem, key=lambda n: convs[n]["y"].c0)
            mem = [n for n in mem if convs[n]["x"].gptr() == p.out and cap.get(n, {}).get("dx") is not None]
            if not mem:
                continue

            def pre(mem=mem, accum=(p.epi == S.EPI_ACCUM)):
                for n in mem:                                    # (the weight-gradient probe already forced dy; repeated for plans that order differently)
                    write(convs[n]["y"], cap[n]["dy"], grad=True)
                if accum:
                    xr = convs[mem[0]]["x"]
                    write(xr, torch.zeros(xr.N, xr.C, xr.H, xr.W), grad=True)

            def post(mem=mem):
                want = sum(cap[n]["dx"] for n in mem)
                errs["+".join(mem) + ":dx"] = rel(read(convs[mem[0]]["x"], grad=True), want)
            probe[(tid, i)] = (pre, post)

    g.probe = probe
    crit = (ComputeCSLLoss if mode == "csl" else ComputeKFIoULoss)(net, HYP)
    loss, items = crit(net(x.to(DEV), training=True), tg.to(DEV))
    loss.backward()
    torch.cuda.synchronize()
    g.probe = None

    kinds = {}
    for k, v in errs.items():
        kinds.setdefault(k.rsplit(":", 1)[1], []).append(v)
    nconv = sum(1 for c in convs.values() if c["x"] is not None)
    summary = {k: dict(n=len(v), max=max(v), mean=sum(v) / len(v)) for k, v in kinds.items()}
    worst = sorted(errs.items(), key=lambda kv: -kv[1])[:12]
    path = os.path.join(ROOT, "gpurun_out", "r03_teacher_forced.json")
    os.makedirs(os.path.dirname(path), exist_ok=True)
    doc = json.load(open(path)) if os.path.exists(path) else {}
    doc[f"{ver}_{mode}"] = dict(convs_with_bn=nconv, checks=len(errs), per_quantity=summary, worst=worst, tolerance=TOL)
    json.dump(doc, open(path, "w"), indent=1, sort_keys=True)
    print("TEACHER", ver, mode, json.dumps(summary))
    # coverage: every conv + BN + act node but the stem and the RepConv branches was checked in all six quantities
    for kind in ("y", "z", "dy", "dgamma", "dbeta", "dW", "dx"):
        assert len(kinds.get(kind, [])) >= (0.8 * nconv if kind != "dx" else 0.5 * nconv), (kind, len(kinds.get(kind, [])), nconv)
    bad = {k: round(v, 4) for k, v in errs.items() if not v < TOL}
    assert not bad, (len(bad), sorted(bad.items(), key=lambda kv: -kv[1])[:10])
