"""The pre-split BatchNorm path of the residual units against fp64: every kernel mode on its own, then whole stages on the product path.

Part 1 - kernel anchors.  bn_apply_p16, bn_bwd_p16 and the BatchNorm sums fused into the two backward-data epilogues
(p16_conv2d_bwd_data_bnstats, p16_conv2d_bwd_data_masked_accum) are compared with the fp64 composite relu(bn(y) + shortcut) and its
autograd, batch statistics taken in fp64 from y; the device side is colstats -> bn_stats -> the kernel under test.  Bars: the forward
at the 2e-5 x max|ref| and the backward at the 1e-4 x max|ref| of test_kernels_gpu.py::test_batchnorm_train, backward-data products
at the 6e-5 of test_p16_gpu.py.  The backward references take the DEVICE's ReLU decisions (forward output > 0), so a pre-activation
that rounds across zero is no gradient error; the fused-sum legs differentiate with the device's own product dx as the upstream
gradient, which keeps the BatchNorm bar separable from the product's error.  The mask words are decoded on the host
(_resunit_ref.mask_decode) and must equal the decisions at every element; pair outputs must be the bit-exact P16 image of the fp32
output.  `frozen=True` has no legs: the product never passes it to bn_bwd_p16 (ops._p16_bn_backward hands False; moving-statistics
units run on the fp32 kernels).  The compact skip merge (old_even=) needs an even map and so has no leg on (3, 5, 7).

Part 2 - stage parity.  ResNet(stages=((64, 3, 1), (128, 2, 2), (256, 1, 2))) at batch 2 under gemm_precision('split') on a Tape: every
layer handle (captured by wrapping _ConvBN.call / ops.conv_bn_relu_maxpool, converted with ops.as_fp32 after the backward pass) and
the gradient of every kernel / bias / gamma / beta of the block layers against _resunit_ref.net in fp64, started from the captured
pool output.  Two geometries: prepared images of 32 x 48 (pooled 8 x 12 -> 4 x 6 -> 2 x 3: even-pixel apply, compact stride-2
gradients) and 34 x 26 (pooled 9 x 7: the dense fallbacks; the scatter form's even-pixel REDUCTION of bn_bwd_p16 serves odd maps too
and does run there).  The forward is compared with the reference's own ReLU decisions, the gradients with the device's injected.  A
device decision may differ from the fp64 one only where the fp64 pre-activation lies within the layer's forward allowance of zero,
and on at most 1e-4 of all elements.  Units applied at the even pixels only carry outputs and decisions at (2i, 2j).

Allowances are multiples of e32(t), the max-normalised deviation of the reference's own fp32 run from its fp64 run (a gradient's scale
is at least 1 % of the largest parameter gradient: convolution biases under train-mode BatchNorm have zero gradient up to round-off):
forward 16 x e32 (f16 pairs carry 2^-22 against fp32's 2^-24, times the 4x margin of grad_report), gradients 256 x e32 (bf16 pairs:
2^-18 against 2^-24, same margin).  Every tensor's measured / allowance ratio is printed.  Worst ratios measured on an MI355X with
the defaults (they are records, not bars - the allowance is never tightened towards them):
    32 x 48 (even maps):  outputs 0.103 (u0.short), gradients 0.026; over all switch legs 0.103 / 0.028
    34 x 26 (odd maps):   outputs 0.082 (u0.short), gradients 0.021; over all switch legs 0.082 / 0.025
    no ReLU decision differed from the fp64 one on either geometry; the three perturbed legs reach 12.3, 12.3 and 341
Switch legs turn ops.LAZY_SKIP, BN_FUSE, BN_FUSE2, EVEN_PIXELS, EVEN_APPLY, COMPACT_S2 off singly and together, against the same
reference.  The default leg on the even geometry must have launched every fused / even / compact form (counters around the kernels
entry points), the odd geometry none of the even-apply / compact ones.  Three legs perturb VALUES only (one unit's `pre` sums x 1.01,
the bn_ctx2 sums x 1.01, an all-ones mask in a skip merge) and must make the comparison raise with its worst tensor in the perturbed
unit u0 - for the skip merge of the identity unit u1, whose shortcut is u0's output, u0 is where the damage lands."""
import hashlib
import zlib

import pytest
import torch

import _resunit_ref as R
from test_kernels_gpu import close, dev, rnd
from test_p16_gpu import bits, p16_ref

pytestmark = pytest.mark.gpu

EPS = R.EPS


# =====================================================================================================================
# Part 1: kernel anchors
# =====================================================================================================================
def _stats(k, y):
    rows, C = y.shape
    return k.bn_stats(rows, C, k.colstats(y), EPS, 0.99, True, dev(torch.zeros(C)), dev(torch.ones(C)), like=y)


def _affine(C, seed):
    return 1 + 0.1 * rnd(C, seed=seed), 0.1 * rnd(C, seed=seed + 1)


def _f16_pair_value(x):
    """fp64 value of the f16 pair of an fp32 tensor (csrc/p16.h: hi = f16(x), lo = f16(x - hi), unscaled)."""
    hi = x.float().half()
    lo = (x.float() - hi.float()).half()
    return hi.double() + lo.double()


def _even(t, N, H, W):
    """The pixels (2i, 2j) of a [N*H*W, C] tensor."""
    return t.reshape(N, H, W, -1)[:, ::2, ::2]


FWD_DENSE = [(51, 8), (130, 64), (48, 256), (7, 2048)]              # (51, 8): the mask's last 64-float4 group is partial
FWD_EVEN = [(1, 2, 2, 256), (2, 4, 6, 256), (3, 6, 2, 512)]


@pytest.mark.parametrize("form", ["none", "fp32", "p16", "bn"])
@pytest.mark.parametrize("shape", FWD_DENSE + FWD_EVEN, ids=lambda s: "x".join(map(str, s)))
def test_bn_apply_p16_against_fp64(cuda, shape, form):
    from boosted_detr_amd import kernels as k
    even = shape[1:3] if len(shape) == 4 else None
    N, H, W = shape[:3] if even else (1, 1, shape[0])
    C = shape[-1]
    rows = N * H * W
    x = rnd(rows, C, seed=1) * 2 + 0.5
    gamma, beta = _affine(C, 2)
    xd = dev(x)
    mean, rstd = _stats(k, xd)
    pre = R.batchnorm(x.double(), gamma.double(), beta.double())
    residual, kw = None, {}
    if form in ("fp32", "p16"):
        resid = rnd(rows, C, seed=6)
        if form == "fp32":
            residual, pre = dev(resid), pre + resid.double()
        else:
            residual, kw = k.p16_pack(dev(resid), want_bf16=False)[0], {"residual_p16": True}
            pre = pre + _f16_pair_value(resid)
    elif form == "bn":
        y0 = rnd(rows, C, seed=7) * 3 - 0.2
        g0, b0 = _affine(C, 8)
        residual = dev(y0)
        kw = {"residual_bn": (*_stats(k, residual), dev(g0), dev(b0))}
        pre = pre + R.batchnorm(y0.double(), g0.double(), b0.double())
    want = R.relu(pre)
    o32, of, ob, mask = k.bn_apply_p16(xd, mean, rstd, dev(gamma), dev(beta), residual, True, want_fp32=True, want_mask=True, even_pixels=even, **kw)
    torch.cuda.synchronize()
    pick = (lambda t: _even(t, N, H, W)) if even else (lambda t: t)
    got = pick(o32.cpu())
    close(got, pick(want), rtol=2e-5)
    assert mask.dtype == torch.int64 and mask.numel() == ((rows * C // 4 + 63) // 64) * 4
    decoded = R.mask_decode(mask, rows * C).view(rows, C)
    assert torch.equal(pick(decoded), got > 0)                                       # every element, the partial tail group included
    assert 0.05 < float((got > 0).double().mean()) < 0.95                            # (both decisions occur: the comparison means something)
    assert torch.equal(pick(bits(of)), pick(p16_ref(o32.cpu(), True)))
    assert torch.equal(pick(bits(ob)), pick(p16_ref(o32.cpu(), False)))


# (gradient form, (N, H, W, C)); the even-pixel reduction also on an odd map; the compact form needs an even one
BWD_LEGS = [("dense", (1, 1, 51, 8)), ("dense", (1, 1, 130, 64)), ("dense", (1, 1, 7, 2048)),
            ("even", (2, 4, 6, 256)), ("even", (3, 9, 7, 64)), ("even", (1, 3, 3, 8)),
            ("compact", (2, 4, 6, 64)), ("compact", (3, 6, 2, 512)), ("compact", (1, 2, 2, 8))]


@pytest.mark.parametrize("source", ["recomputed", "fp32", "bf16", "bits"])
@pytest.mark.parametrize("form,shape", BWD_LEGS, ids=lambda v: v if isinstance(v, str) else "x".join(map(str, v)))
def test_bn_bwd_p16_against_fp64_autograd(cuda, form, shape, source):
    from boosted_detr_amd import kernels as k
    N, H, W, C = shape
    rows = N * H * W
    y = rnd(rows, C, seed=1) * 2 + 0.3
    gamma, beta = _affine(C, 2)
    resid = rnd(rows, C, seed=6) if source != "recomputed" else None
    yd, gd, bd = dev(y), dev(gamma), dev(beta)
    mean, rstd = _stats(k, yd)
    o32, _, ob, mask = k.bn_apply_p16(yd, mean, rstd, gd, bd, dev(resid) if resid is not None else None, True, want_fp32=True, want_f16=False,
                                      want_mask=True)
    decisions = (o32 > 0).cpu()
    src, mode = {"recomputed": (None, 0), "fp32": (o32, 0), "bf16": (ob, 1), "bits": (mask, 2)}[source]
    g = rnd(N, H, W, C, seed=7)
    if form == "dense":
        dout64, ddev = g.double(), dev(g)
    else:
        keep = torch.zeros(N, H, W, 1)
        keep[:, ::2, ::2] = 1
        dout64 = (g * keep).double()
        ddev = dev(g[:, ::2, ::2]) if form == "compact" else dev(g * keep)
    want_res = resid is not None and form != "compact"                               # (the compact form writes no residual gradient)
    dxb, dx32, dg, db, dres = k.bn_bwd_p16(ddev.view(-1, C), src, yd, mean, rstd, gd, True, False, want_residual_grad=want_res, beta=bd, want_fp32=True,
                                           out_p16=mode, even_pixels=None if form == "dense" else (N, H, W), dout_compact=form == "compact")
    torch.cuda.synchronize()
    y64, g64, b64 = (t.double().requires_grad_(True) for t in (y, gamma, beta))
    r64 = resid.double().requires_grad_(True) if resid is not None else None
    pre = R.batchnorm(y64, g64, b64)
    out = R.relu(pre + r64 if r64 is not None else pre, decisions)
    out.backward(dout64.view(rows, C))
    close(dx32, y64.grad, rtol=1e-4)
    close(dg, g64.grad, rtol=1e-4)
    close(db, b64.grad, rtol=1e-4)
    if want_res:
        close(dres, r64.grad, rtol=1e-4)
    else:
        assert dres is None
    assert torch.equal(bits(dxb), p16_ref(dx32.cpu(), False))


class _Unit:
    """A residual unit's closing BatchNorm on the device and on the host: y, its statistics, gamma / beta, the shortcut (fp32, or the raw
    output y0 of a projection with its own BatchNorm), the device's ReLU decisions and their bit mask."""

    def __init__(self, k, rows, C, seed, shortcut):
        self.y = rnd(rows, C, seed=seed) * 2 + 0.3
        self.gamma, self.beta = _affine(C, seed + 1)
        self.yd, self.gd, self.bd = dev(self.y), dev(self.gamma), dev(self.beta)
        self.mean, self.rstd = _stats(k, self.yd)
        self.resid = self.y0 = None
        res, kw = None, {}
        if shortcut == "fp32":
            self.resid = rnd(rows, C, seed=seed + 3)
            res = dev(self.resid)
        elif shortcut == "bn":
            self.y0 = rnd(rows, C, seed=seed + 4) * 1.5 - 0.2
            self.gamma0, self.beta0 = _affine(C, seed + 5)
            self.y0d, self.g0d, self.b0d = dev(self.y0), dev(self.gamma0), dev(self.beta0)
            self.mean0, self.rstd0 = _stats(k, self.y0d)
            res, kw = self.y0d, {"residual_bn": (self.mean0, self.rstd0, self.g0d, self.b0d)}
        o32, _, _, self.bits = k.bn_apply_p16(self.yd, self.mean, self.rstd, self.gd, self.bd, res, True, want_fp32=True, want_f16=False, want_bf16=False,
                                              want_mask=True, **kw)
        self.decisions = (o32 > 0).cpu()

    def ctx(self):
        return (self.yd, self.mean, self.rstd, self.gd, self.bd, self.bits)

    def autograd(self, upstream):
        """fp64 gradients of relu(bn(y) + shortcut) with the device's decisions: {'y', 'gamma', 'beta'[, 'y0', 'gamma0', 'beta0']}."""
        leaf = {n: getattr(self, n).double().requires_grad_(True) for n in ("y", "gamma", "beta") + (("y0", "gamma0", "beta0") if self.y0 is not None else ())}
        pre = R.batchnorm(leaf["y"], leaf["gamma"], leaf["beta"])
        if self.resid is not None:
            pre = pre + self.resid.double()
        if self.y0 is not None:
            pre = pre + R.batchnorm(leaf["y0"], leaf["gamma0"], leaf["beta0"])
        R.relu(pre, self.decisions).backward(upstream)
        return {n: t.grad for n, t in leaf.items()}


def _check_bn_backward(got, want_dx, want_dgamma, want_dbeta):
    dxb, dx32, dg, db, _ = got
    close(dx32, want_dx, rtol=1e-4)
    close(dg, want_dgamma, rtol=1e-4)
    close(db, want_dbeta, rtol=1e-4)
    assert torch.equal(bits(dxb), p16_ref(dx32.cpu(), False))


FUSED_GEOMS = [(2, 4, 6, 64, 256), (3, 5, 7, 256, 64), (2, 4, 6, 256, 256)]                  # N, H, W, C -> K
FUSED_LEGS = [(leg, geom) for geom in FUSED_GEOMS for leg in ("bnstats", "ctx", "ctx2", "old_even") if not (leg == "old_even" and geom[1] % 2)]


@pytest.mark.parametrize("leg,geom", FUSED_LEGS, ids=lambda v: v if isinstance(v, str) else "x".join(map(str, v)))
def test_fused_batchnorm_sums_against_fp64(cuda, leg, geom):
    from boosted_detr_amd import kernels as k
    N, H, W, C, K_ = geom
    g = k.ConvGeom(N, H, W, C, K_, 1, 1, 1, 0)
    rows = N * H * W
    w, dy = rnd(K_, 1, 1, C, seed=6, scale=C ** -0.5), rnd(N, H, W, K_, seed=7)
    _, wt = k.p16_pack_conv_weights(dev(w), want_fwd=False)
    _, dyb = k.p16_pack(dev(dy), want_f16=False)
    product = dy.double().reshape(rows, K_) @ w.double().reshape(K_, C)
    if leg == "bnstats":
        # the link inside a bottleneck: relu(bn(y)) with no residual, the mask recomputed from y
        u = _Unit(k, rows, C, 10, None)
        dx, parts = k.p16_conv2d_bwd_data_bnstats(dyb, wt, g, u.yd, u.mean, u.rstd, u.gd, u.bd, True)
        close(dx.view(rows, C), product, rtol=6e-5)
        want = u.autograd(dx.cpu().double().view(rows, C))
        got = k.bn_bwd_p16(dx.view(rows, C), None, u.yd, u.mean, u.rstd, u.gd, True, False, beta=u.bd, want_fp32=True, pre=parts)
        _check_bn_backward(got, want["y"], want["gamma"], want["beta"])
        return
    prev, this = _Unit(k, rows, C, 10, "bn" if leg == "ctx2" else "fp32"), _Unit(k, rows, C, 20, "fp32")
    d_out = rnd(N, H, W, C, seed=5)
    if leg == "old_even":
        keep = torch.zeros(N, H, W, 1)
        keep[:, ::2, ::2] = 1
        d_out = d_out * keep
        r = k.p16_conv2d_bwd_data_masked_accum(dyb, wt, g, torch.empty(N, H, W, C, device="cuda"), this.bits, bn_ctx=prev.ctx(),
                                               old_even=dev(d_out[:, ::2, ::2]))
    elif leg == "ctx2":
        r = k.p16_conv2d_bwd_data_masked_accum(dyb, wt, g, dev(d_out), this.bits, bn_ctx=prev.ctx(), bn_ctx2=(prev.y0d, prev.mean0, prev.rstd0))
    else:
        r = k.p16_conv2d_bwd_data_masked_accum(dyb, wt, g, dev(d_out), this.bits, bn_ctx=prev.ctx())
    dx, parts = r[0], r[1]
    torch.cuda.synchronize()
    close(dx.view(rows, C), product + d_out.double().reshape(rows, C) * this.decisions.double(), rtol=6e-5)
    dx2d = dx.view(rows, C)
    want = prev.autograd(dx2d.cpu().double())
    got = k.bn_bwd_p16(dx2d, prev.bits, prev.yd, prev.mean, prev.rstd, prev.gd, True, False, beta=prev.bd, want_fp32=True, out_p16=2, pre=parts)
    _check_bn_backward(got, want["y"], want["gamma"], want["beta"])
    if leg == "ctx2":
        # the shortcut's BatchNorm in relu(bn(y) + bn0(y0)): same gradient, the ReLU decision is the unit's bit mask
        got0 = k.bn_bwd_p16(dx2d, prev.bits, prev.y0d, prev.mean0, prev.rstd0, prev.g0d, True, False, beta=prev.b0d, want_fp32=True, out_p16=2, pre=r[2])
        _check_bn_backward(got0, want["y0"], want["gamma0"], want["beta0"])


# =====================================================================================================================
# Part 2: stage parity on the product path
# =====================================================================================================================
IMAGE_HW = {"even": (32, 48), "odd": (34, 26)}
SWITCHES = ("LAZY_SKIP", "BN_FUSE", "BN_FUSE2", "EVEN_PIXELS", "EVEN_APPLY", "COMPACT_S2")
FWD_FACTOR, GRAD_FACTOR, DECISION_CAP, GRAD_FLOOR = 16.0, 256.0, 1e-4, 1e-2


class ParityError(AssertionError):
    def __init__(self, msg, worst, ratio):
        super().__init__(msg)
        self.worst, self.ratio = worst, ratio


@pytest.fixture
def deterministic():
    from boosted_detr_amd import kernels as K
    prev = K.set_deterministic(True)
    yield
    K.set_deterministic(prev)


@pytest.fixture(scope="module")
def resnet(cuda):
    from boosted_detr_amd.backbone import ResNet
    from boosted_detr_amd.engine import bump_weights_version
    net = ResNet(stages=R.STAGES, name="r", seed=3)
    for blk in net.blocks:
        for layer in blk.values():
            if layer is not None:
                for var in (layer.bias, layer.bn.gamma, layer.bn.beta):          # away from their 0 / 1 initial values
                    var.value.add_(dev(rnd(*var.value.shape, seed=zlib.crc32(var.name.encode()) % 1000, scale=0.2)))
    bump_weights_version()
    return net


def _layer_names(net):
    return {id(layer): f"{R.unit_name(i)}.{n}" for i, blk in enumerate(net.blocks) for n, layer in blk.items() if layer is not None}


def _block_variables(net):
    """{'u3.c1.kernel': Variable} of the block layers."""
    out = {}
    for i, blk in enumerate(net.blocks):
        for n, layer in blk.items():
            if layer is not None:
                for vn, var in (("kernel", layer.kernel), ("bias", layer.bias), ("gamma", layer.bn.gamma), ("beta", layer.bn.beta)):
                    out[f"{R.unit_name(i)}.{n}.{vn}"] = var
    return out


class _Spy:
    """Counters around the kernels entry points of the path (and the 'compact tensor meets anything else' branch of ops._p16_input_grad),
    the record of which outputs were applied at the even pixels only, and - `perturb` - one of the three value perturbations."""

    def __init__(self, mp, net, perturb=None):
        from boosted_detr_amd import kernels as k, ops
        from boosted_detr_amd.engine import info
        self.count = {n: 0 for n in ("apply_even", "apply_residual_bn", "bwd_pre", "bwd_compact", "bwd_bits", "bwd_even", "bnstats", "accum", "accum_ctx2",
                                     "accum_old_even", "materialise_branch", "perturbed")}
        self.even_applied = {}                          # data_ptr of an f16 pair output -> (H, W)
        count, inside = self.count, [0]
        target_gamma = net.blocks[0]["c3"].bn.gamma.value.data_ptr()
        real_apply, real_bwd, real_bnstats, real_accum = k.bn_apply_p16, k.bn_bwd_p16, k.p16_conv2d_bwd_data_bnstats, k.p16_conv2d_bwd_data_masked_accum
        real_mat, real_input_grad = ops.materialise, ops._p16_input_grad

        def apply(*a, **kw):
            outs = real_apply(*a, **kw)
            count["apply_even"] += kw.get("even_pixels") is not None
            count["apply_residual_bn"] += kw.get("residual_bn") is not None
            if kw.get("even_pixels") is not None and outs[1] is not None:
                self.even_applied[outs[1].data_ptr()] = tuple(kw["even_pixels"])
            return outs

        def bwd(*a, **kw):
            count["bwd_pre"] += kw.get("pre") is not None
            count["bwd_compact"] += bool(kw.get("dout_compact"))
            count["bwd_bits"] += int(kw.get("out_p16", 0)) == 2
            count["bwd_even"] += kw.get("even_pixels") is not None
            if perturb == "pre" and kw.get("pre") is not None and a[5].data_ptr() == target_gamma:
                pg, pgx, n = kw["pre"]
                kw = dict(kw, pre=(pg * 1.01, pgx * 1.01, n))
                count["perturbed"] += 1
            return real_bwd(*a, **kw)

        def bnstats(*a, **kw):
            count["bnstats"] += 1
            return real_bnstats(*a, **kw)

        def accum(dyb, wt, g, dx, relu_mask, **kw):
            count["accum"] += 1
            count["accum_ctx2"] += kw.get("bn_ctx2") is not None
            count["accum_old_even"] += kw.get("old_even") is not None
            first_unit = kw.get("bn_ctx2") is not None and kw["bn_ctx2"][0].shape[-1] == 256          # the launch of u1's first convolution
            if perturb == "ones" and first_unit:
                relu_mask = torch.full_like(relu_mask, -1)
                count["perturbed"] += 1
            r = real_accum(dyb, wt, g, dx, relu_mask, **kw)
            if perturb == "ctx2" and first_unit:
                pg, pgx2, n = r[2]
                r = (r[0], r[1], (pg * 1.01, pgx2 * 1.01, n))
                count["perturbed"] += 1
            return r

        def input_grad(*a, **kw):
            inside[0] += 1
            try:
                return real_input_grad(*a, **kw)
            finally:
                inside[0] -= 1

        def mat(t):
            count["materialise_branch"] += bool(inside[0]) and info(t).compact_even is not None
            return real_mat(t)

        mp.setattr(k, "bn_apply_p16", apply)
        mp.setattr(k, "bn_bwd_p16", bwd)
        mp.setattr(k, "p16_conv2d_bwd_data_bnstats", bnstats)
        mp.setattr(k, "p16_conv2d_bwd_data_masked_accum", accum)
        mp.setattr(ops, "_p16_input_grad", input_grad)
        mp.setattr(ops, "materialise", mat)


def _device_run(net, geometry, mp=None, perturb=None):
    """One forward + backward of the backbone on the product path.  mp (a MonkeyPatch): capture every layer's handle and count the
    launches; without it nothing is wrapped.  Returns {'grads': {variable name: tensor}, 'layers': {name: fp32 tensor on the host},
    'pool', 'even': {layer name: (H, W)}, 'count'}."""
    from boosted_detr_amd import kernels as k, ops
    from boosted_detr_amd.backbone import _ConvBN
    from boosted_detr_amd.engine import Tape, join_side_stream, recording
    H, W = IMAGE_HW[geometry]
    x = dev(rnd(2, H, W, 4, seed=1, scale=40.0))
    x[..., 3] = 0                                                                # the padding channel image_prep adds
    handles, spy = [], None
    if mp is not None:
        names = _layer_names(net)
        real_call, real_stem = _ConvBN.call, ops.conv_bn_relu_maxpool

        def call(self, inputs, **kw):
            out = real_call(self, inputs, **kw)
            if id(self) in names:
                handles.append((names[id(self)], out))
            return out

        def stem(*a, **kw):
            out = real_stem(*a, **kw)
            handles.append(("pool", out))
            return out

        mp.setattr(_ConvBN, "call", call)
        mp.setattr(ops, "conv_bn_relu_maxpool", stem)
        spy = _Spy(mp, net, perturb)
    for v in net.variables:
        v.reset_grad()
    tape = Tape()
    with k.gemm_precision("split"):
        with recording(tape):
            out = net([x], training=True)
        assert not ops.is_p16_only(out)                                          # the gradient seed goes in at the fp32 output
        tape.backward({id(out): dev(rnd(*out.shape, seed=2))})
        join_side_stream()
        torch.cuda.synchronize()
        res = {"grads": {v.name: v.grad.clone() for v in net.variables if v.grad is not None}, "gout": rnd(*out.shape, seed=2)}
        if mp is not None:
            res["layers"] = {n: ops.as_fp32(h).cpu() for n, h in handles}
            res["even"] = {n: spy.even_applied[ops.act_info(h).f16.data_ptr()] for n, h in handles
                           if ops.act_info(h).f16 is not None and ops.act_info(h).f16.data_ptr() in spy.even_applied}
            res["count"] = spy.count
    torch.cuda.synchronize()
    return res


_REFS = {}


def _reference(net, pool, decisions=None, gout=None):
    """fp64 and fp32 runs of the reference from the captured pool output, cached on their inputs' bytes."""
    h = hashlib.sha1(pool.numpy().tobytes())
    for n in sorted(decisions or {}):
        h.update(n.encode())
        h.update(decisions[n].numpy().tobytes())
    key = (h.hexdigest(), gout is not None)
    if key not in _REFS:
        blocks = [{n: (None if l is None else {"kernel": l.kernel.value.cpu().numpy(), "bias": l.bias.value.cpu().numpy(),
                                               "gamma": l.bn.gamma.value.cpu().numpy(), "beta": l.bn.beta.value.cpu().numpy()}) for n, l in blk.items()}
                  for blk in net.blocks]
        _REFS[key] = tuple(R.run(R.STAGES, pool.numpy(), blocks, dtype=dt, decisions=decisions, gout=gout) for dt in (torch.float64, torch.float32))
    return _REFS[key]


def _compare(net, run, label):
    """Every captured layer output and every block-layer gradient of one device run against the reference; prints each tensor's
    measured / allowance ratio and raises ParityError naming the worst tensor if one exceeds 1."""
    layers, even = run["layers"], run["even"]
    pool = layers["pool"]
    (r64, _), (r32, _) = _reference(net, pool)
    rows, decisions, differ, total = [], {}, 0, 0

    def pick(name, t):
        return t[:, ::2, ::2] if name in even else t

    for name in (n for n in layers if n != "pool"):
        assert layers[name].shape == r64[name].shape, (name, layers[name].shape, r64[name].shape)
        scale = float(r64[name].abs().max())
        allow = FWD_FACTOR * R.deviation(r32[name], r64[name])                              # relative to max |ref| of the whole tensor
        measured = float((pick(name, layers[name]).double() - pick(name, r64[name])).abs().max()) / scale
        rows.append((measured / allow, f"{name} (output)", measured, allow))
        if not name.endswith(".short"):
            pre, on = r64[name + ".pre"], layers[name] > 0
            d = r64[name] > 0
            if name in even:                                                                # only (2i, 2j) was written: the rest decides for itself
                d[:, ::2, ::2] = on[:, ::2, ::2]
            else:
                d = on
            decisions[name] = d
            flips = pick(name, d != (pre > 0))
            differ, total = differ + int(flips.sum()), total + flips.numel()
            far = float((pick(name, pre).abs() * flips).max()) / scale                      # a flip is legitimate within the forward allowance of zero only
            rows.append((far / allow, f"{name} (decision margin)", far, allow))
    rows.append((differ / (DECISION_CAP * total), "ReLU decisions that differ from fp64", differ / total, DECISION_CAP))
    (_, g64), (_, g32) = _reference(net, pool, decisions, run["gout"].numpy())
    floor = GRAD_FLOOR * max(float(g.abs().max()) for g in g64.values())
    for name, var in _block_variables(net).items():
        got = run["grads"][var.name].cpu()
        allow = GRAD_FACTOR * R.deviation(g32[name], g64[name], floor)
        measured = R.deviation(got, g64[name], floor)
        rows.append((measured / allow if allow > 0 else (0.0 if measured == 0 else float("inf")), f"{name} (gradient)", measured, allow))
    print(f"\n[{label}] measured / allowance")
    for ratio, name, measured, allow in rows:
        print(f"  {ratio:9.3e}  {name:38s} {measured:.3e} / {allow:.3e}")
    ratio, name, measured, allow = max(rows, key=lambda r: (r[0] != r[0], r[0]))            # (a NaN ratio is the worst of all)
    fwd = max(r[0] for r in rows if "(output)" in r[1])
    grad = max(r[0] for r in rows if "(gradient)" in r[1])
    print(f"[{label}] worst ratio: outputs {fwd:.3f}, gradients {grad:.3f}, overall {ratio:.3f} at {name}")
    if not ratio <= 1.0:
        raise ParityError(f"{label}: {name}: {measured:.3e} > {allow:.3e} (ratio {ratio:.3f})", name, ratio)
    return rows


LEGS = [()] + [(s,) for s in SWITCHES] + [SWITCHES]


@pytest.mark.parametrize("off", LEGS, ids=lambda s: "defaults" if not s else ("all_off" if len(s) > 1 else s[0] + "_off"))
@pytest.mark.parametrize("geometry", ["even", "odd"])
def test_stage_parity_against_fp64(cuda, resnet, monkeypatch, geometry, off):
    from boosted_detr_amd import ops
    for name in SWITCHES:
        monkeypatch.setattr(ops, name, name not in off)
    run = _device_run(resnet, geometry, monkeypatch)
    assert set(run["layers"]) == {"pool"} | set(_layer_names(resnet).values())
    _compare(resnet, run, f"{geometry} / " + ("+".join(off) + " off" if off else "defaults"))
    c = run["count"]
    if not off and geometry == "even":
        # the topology reaches every fused / even / compact form of the path (stage 2 has two units for the materialise branch)
        for name in ("apply_even", "apply_residual_bn", "bwd_pre", "bwd_compact", "bwd_bits", "bnstats", "accum_ctx2", "accum_old_even", "materialise_branch"):
            assert c[name] > 0, (name, c)
        assert sorted(run["even"]) == ["u2.c3", "u4.c3"], run["even"]
    if geometry == "odd" or "EVEN_APPLY" in off:
        assert c["apply_even"] == 0 and not run["even"], c
    if geometry == "odd" or "COMPACT_S2" in off:
        assert c["bwd_compact"] == 0 and c["accum_old_even"] == 0 and c["materialise_branch"] == 0, c
    if len(off) > 1:
        assert c["bwd_pre"] == 0 and c["bnstats"] == 0 and c["accum"] == 0 and c["bwd_even"] == 0, c


@pytest.mark.parametrize("geometry", ["even", "odd"])
def test_capture_does_not_perturb_the_path(cuda, resnet, deterministic, geometry):
    """Deterministic mode: a run with every wrapper of this file in place and a run with none give equal gradients for every variable."""
    with pytest.MonkeyPatch.context() as mp:
        wrapped = _device_run(resnet, geometry, mp)
    plain = _device_run(resnet, geometry)
    assert "layers" in wrapped and "layers" not in plain
    assert set(wrapped["grads"]) == set(plain["grads"]) and len(plain["grads"]) >= 4 * len(_layer_names(resnet))
    bad = [n for n in plain["grads"] if not torch.equal(wrapped["grads"][n], plain["grads"][n])]
    assert not bad, bad


@pytest.mark.parametrize("perturb", ["pre", "ctx2", "ones"])
def test_a_perturbed_value_is_caught_and_named(cuda, resnet, monkeypatch, perturb):
    """Values only - no shape, pointer or mask size changes: the BatchNorm sums of u0's closing BatchNorm x 1.01, those of its projection
    shortcut's BatchNorm x 1.01, and u1's skip merge with an all-ones mask (which corrupts the gradient of u1's shortcut, u0's output)."""
    run = _device_run(resnet, "even", monkeypatch, perturb)
    assert run["count"]["perturbed"] == 1, run["count"]
    with pytest.raises(ParityError) as e:
        _compare(resnet, run, f"even / perturbed {perturb}")
    allowed = {"pre": ("u0.",), "ctx2": ("u0.short.",), "ones": ("u0.", "u1.")}[perturb]
    assert e.value.worst.startswith(allowed) and "(gradient)" in e.value.worst, (e.value.worst, e.value.ratio)
