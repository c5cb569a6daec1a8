"""tests/ew_ref.py (the float64 references of the elementwise C-ABI tests) against torch's float64 autograd of F.batch_norm + activation,
on the CPU: the written-out backward (sums, gx, the data gradient) is the gradient of the training-mode forward."""
import torch
import torch.nn.functional as F

from tests import ew_ref as R


def test_bn_act_backward_reference_equals_autograd():
    g = torch.Generator().manual_seed(0)
    for act in R.ACTS:
        for two in (False, True):
            M, C = 300, 16
            ys = [torch.randn(M, C, generator=g, dtype=torch.float64) * 2 + 1 for _ in range(2 if two else 1)]
            gam = [torch.rand(C, generator=g, dtype=torch.float64) + 0.5 for _ in ys]
            bet = [torch.rand(C, generator=g, dtype=torch.float64) - 0.5 for _ in ys]
            dz = torch.randn(M, C, generator=g, dtype=torch.float64)
            leaves = [t.clone().requires_grad_(True) for t in ys + gam + bet]
            yl, gl, bl = leaves[:len(ys)], leaves[len(ys):2 * len(ys)], leaves[2 * len(ys):]
            u = sum(F.batch_norm(y, None, None, gg, bb, training=True, eps=1e-5) for y, gg, bb in zip(yl, gl, bl))
            z = {R.MISH: F.mish, R.LEAKY: lambda t: F.leaky_relu(t, 0.1), R.SILU: F.silu, R.LINEAR: lambda t: t}[act](u)
            z.backward(dz)
            cos = []
            for y, gg, bb in zip(ys, gam, bet):
                mean, var = y.mean(0), y.var(0, unbiased=False)
                invstd = 1.0 / torch.sqrt(var + 1e-5)
                cos.append(torch.stack([mean, invstd, gg * invstd, bb - mean * gg * invstd]))
            ref = R.bn_act_bwd(dz, ys[0], cos[0], act, 0, ys[1] if two else None, cos[1] if two else None)
            for i, y in enumerate(ys):
                assert torch.allclose(ref["gx"][i], gl[i].grad, rtol=1e-9, atol=1e-9), "dgamma"
                assert torch.allclose(ref["S0"], bl[i].grad, rtol=1e-9, atol=1e-9), "dbeta"
                dy, _ = R.apply_ref(ref["g"], y, cos[i], ref["S0"] / M, ref["gx"][i] / M)
                assert torch.allclose(dy, yl[i].grad, rtol=1e-9, atol=1e-9), "dy"
            # forward reference: the same z
            zr, _, _, _ = R.bn_act_fwd(ys[0], cos[0], act, ys[1] if two else None, cos[1] if two else None)
            assert torch.allclose(zr, z.detach(), rtol=1e-12, atol=1e-12)


def test_pool_reference_first_maximum_and_gradient():
    x = torch.tensor([[1.0, 3.0, 3.0], [2.0, 3.0, 0.0], [3.0, 1.0, 1.0]]).view(1, 3, 3, 1)
    z, idx = R.maxpool(x, 2, 1, 0)
    assert z.view(-1).tolist() == [3.0, 3.0, 3.0, 3.0]
    assert idx.view(-1).tolist() == [1, 0, 1, 0]              # first maximum in (dy, dx) order, not torch.max_pool2d's choice
    dx = R.maxpool_bwd(idx, torch.ones(1, 2, 2, 1, dtype=torch.float64), 3, 3, 2, 1, 0)
    assert dx.view(-1).tolist() == [0.0, 2.0, 0.0, 0.0, 2.0, 0.0, 0.0, 0.0, 0.0]
    big = torch.randn(2, 9, 7, 3)
    zc, ic = R.maxpool(big, 5, 1, 2, rows_per_chunk=2)
    z1, i1 = R.maxpool(big, 5, 1, 2)
    assert torch.equal(zc, z1) and torch.equal(ic, i1)
    assert torch.equal(zc, F.max_pool2d(big.permute(0, 3, 1, 2), 5, 1, 2).permute(0, 2, 3, 1))
