"""AdamW without a GPU: the fp64 restatement the GPU tests compare against is pinned to torch.optim.AdamW, and the host side of
training.AdamW (per-step scalars, weight-decay exclusion, argument checks) is checked as plain arithmetic."""
import math

import numpy as np
import pytest
import torch

import _adamw_ref as R


def test_fp64_restatement_equals_torch_adamw():
    """With weight_decay_torch = wd / lr and a negligible epsilon (1e-30 on both sides: torch puts epsilon beside the bias-corrected
    sqrt(v), Keras beside the raw one) torch.optim.AdamW in fp64 is algebraically the same update.  50 steps, gradient magnitudes over
    four decades, no exact zeros (0 / (0 + 1e-30) is fine, but a zero gradient in step 1 makes both sides divide by 1e-30 only)."""
    rng = np.random.default_rng(7)
    n, lr, wd, b1, b2, eps = 1000, 1e-3, 1e-3, 0.9, 0.999, 1e-30
    w0 = rng.standard_normal(n)
    p = torch.nn.Parameter(torch.tensor(w0, dtype=torch.float64))
    opt = torch.optim.AdamW([p], lr=lr, betas=(b1, b2), eps=eps, weight_decay=wd / lr, amsgrad=False)
    w, m, v = w0.copy(), np.zeros(n), np.zeros(n)
    for t in range(1, 51):
        g = np.sign(rng.standard_normal(n)) * 10.0 ** rng.uniform(-4.0, 0.0, n)
        assert (g != 0).all()
        p.grad = torch.tensor(g, dtype=torch.float64)
        opt.step()
        w, m, v = R.adamw_step64(w, g, m, v, lr=lr, wd=wd, t=t, b1=b1, b2=b2, eps=eps)
        got = p.detach().numpy()
        rel = np.abs(w - got).max() / np.abs(got).max()
        assert rel <= 1e-12, (t, rel)
    print("fp64 restatement vs torch.optim.AdamW after 50 steps: max relative difference", rel)


def test_fp32_restatement_sits_within_a_few_ulp_of_fp64():
    """The fp32 restatement (the yardstick of the GPU tolerance) with well-formed 1-b is within a few units of 2^-24 of the operands'
    magnitude for m and v; with 1.0f - 0.999f computed in fp32 it would be off by 1.3e-5 relative in v, two hundred times fp32 rounding."""
    rng = np.random.default_rng(3)
    n = 4096
    g = (np.sign(rng.standard_normal(n)) * 10.0 ** rng.uniform(-4.0, 0.0, n)).astype(np.float32)
    w, m, v = (0.05 * rng.standard_normal(n)).astype(np.float32), (0.1 * g).astype(np.float32), (1e-3 * g * g).astype(np.float32)
    kw = dict(lr=1e-3, wd=1e-3, t=7, clipnorm=0.0)
    w64, m64, v64 = R.adamw_step64(w, g, m, v, **kw)
    w32, m32, v32 = R.adamw_step32(w, g, m, v, **kw)
    u = 2.0 ** -24
    assert np.abs(m32 - m64).max() <= 4 * u * np.abs(m64).max()
    assert (np.abs(v32 - v64) <= 4 * u * np.abs(v64) + 1e-45).all()
    assert np.abs(w32 - w64).max() <= 4 * u * np.abs(w64).max()
    assert abs(float(np.float32(1.0) - np.float32(0.999)) / 1e-3 - 1.0) > 1e-5          # the trap the C ABI avoids by taking 1-b as arguments


def test_staged_scalars_follow_the_double_precision_formula():
    from boosted_detr_amd.training import AdamW, CosineDecayRestarts
    sched = CosineDecayRestarts(1e-3, 4000, m_mul=.95, alpha=.1)
    wd = lambda it: 1e-3 * 0.5 ** (it // 1000)
    opt = AdamW(sched, weight_decay=wd, clipnorm=0.1)
    for t in (1, 2, 10, 1000, 10 ** 5):
        opt.iterations = t - 1
        lr_t, wd_t = opt.step_scalars()
        want = sched(t - 1) * math.sqrt(1.0 - 0.999 ** t) / (1.0 - 0.9 ** t)
        assert isinstance(lr_t, np.float32) and lr_t == np.float32(want), (t, lr_t, want)
        assert lr_t == np.float32(R.lr_t64(sched(t - 1), t, 0.9, 0.999))
        assert isinstance(wd_t, np.float32) and wd_t == np.float32(wd(t - 1)), (t, wd_t)
    # constant hyper-parameters; a rolled-back iteration count (the range guard's redo) rolls the bias correction back
    c = AdamW(1e-4, weight_decay=1e-3)
    c.iterations = 5
    a = c.step_scalars()
    c.iterations += 3
    c.iterations -= 3
    assert c.step_scalars() == a and a[1] == np.float32(1e-3)


def test_exclusion_regexes_defaults_and_argument_checks():
    from boosted_detr_amd.training import Adam, AdamW
    names = ["Encoder/block0/attention/kernel", "Encoder/block0/attention/bias", "Encoder/block0/LayerNorm/gamma",
             "Encoder/block0/LayerNorm/beta", "EncoderBackbone/resnet50/conv1_bn/gamma", "BoxPredictionHead/DenseOut/kernel"]
    opt = AdamW(weight_decay=1e-3, exclude_from_weight_decay=[r"/bias$", r"LayerNorm", r"_bn/"])
    assert [opt.decays(n) for n in names] == [True, False, False, False, False, True]
    assert all(AdamW(weight_decay=1e-3).decays(n) for n in names)                      # TFA's default: every variable decays
    d = AdamW(weight_decay=1e-3)
    assert (d.learning_rate, d.beta_1, d.beta_2, d.epsilon, d.clipnorm, d.iterations) == (0.001, 0.9, 0.999, 1e-7, 0.0, 0)
    with pytest.raises(NotImplementedError):
        AdamW(weight_decay=1e-3, amsgrad=True)
    with pytest.raises(TypeError):
        AdamW(1e-3)                                                                    # weight_decay is required
    a = Adam(1e-4, clipnorm=0.1)
    assert isinstance(a, AdamW) and a.weight_decay == 0.0 and a.step_scalars()[1] == 0.0
    # the hyper-parameter tuple a captured step is keyed by sees every by-value argument of the kernel
    h = d.hyper()
    d.beta_2 = 0.99
    assert d.hyper() != h
    import boosted_detr_amd
    assert boosted_detr_amd.AdamW is AdamW and boosted_detr_amd.Adam is Adam


def test_sgd_keeps_its_hyper_tuple():
    from boosted_detr_amd.training import SGD
    assert SGD(1e-3, momentum=.9, nesterov=True, clipnorm=.1).hyper() == (0.9, True, 0.1)
