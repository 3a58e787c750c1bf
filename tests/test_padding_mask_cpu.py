"""Padding masks without a GPU (include/bdetr.h K35; the batch key `valid_region`): known answers of the integer rule, the host
check's refusals, and the condition that keeps the GPU parity test (tests/test_padding_mask_gpu.py) from passing on a model that
ignores the key - on the model case the fp64 oracle with the mask and without it are far apart in everything that test compares."""
import numpy as np
import pytest

import _padding_mask_ref as R
from _close import RTOL


def _both(region, h, w, r, c):
    """The reference rule and the package's host function (what check_valid_region counts with) must agree."""
    from boosted_detr_amd import kernels as K
    want = R.token_keep(region, h, w, r, c)
    got = K.token_keep_host(np.asarray(region, np.int32), h, w, r, c)
    assert got.dtype == np.bool_ and got.shape == want.shape and np.array_equal(got, want)
    return want


def test_rule_model_case():
    keep = _both(R.MODEL_REGIONS, 224, 224, 7, 7)
    assert tuple(keep.sum(1)) == R.MODEL_KEPT == (49, 20)
    grid = keep[1].reshape(7, 7)
    want = np.zeros((7, 7), bool)
    want[0:4, 0:5] = True                          # centres 16 + 32 i: rows 16 .. 112 in [16, 136), columns 16 .. 144 in [0, 150)
    assert np.array_equal(grid, want)


def test_rule_full_region_keeps_everything():
    for h, w, r, c in ((224, 224, 7, 7), (200, 300, 7, 7), (560, 560, 18, 18), (800, 1333, 25, 42), (64, 64, 2, 2)):
        assert _both([[0, 0, h, w]], h, w, r, c).all()


def test_rule_one_pixel_between_centres_keeps_none():
    # centres of 224 on 7 sit at 16, 48, ...: pixel [17, 18) x [17, 18) holds none; pixel [16, 17) x [16, 17) holds token (0, 0)
    assert not _both([[17, 17, 1, 1]], 224, 224, 7, 7).any()
    assert np.flatnonzero(_both([[16, 16, 1, 1]], 224, 224, 7, 7)).tolist() == [0]
    assert not _both([[15, 15, 1, 1]], 224, 224, 7, 7).any()


def test_rule_edges_on_a_centre():
    # top / left ON a centre: inclusive.  bottom / right ON a centre: exclusive.
    assert _both([[48, 0, 176, 224]], 224, 224, 7, 7).reshape(7, 7)[:, 0].tolist() == [False] + [True] * 6
    assert _both([[49, 0, 175, 224]], 224, 224, 7, 7).reshape(7, 7)[:, 0].tolist() == [False, False] + [True] * 5
    assert _both([[0, 0, 48, 224]], 224, 224, 7, 7).reshape(7, 7)[:, 0].tolist() == [True] + [False] * 6
    assert _both([[0, 0, 49, 224]], 224, 224, 7, 7).reshape(7, 7)[:, 0].tolist() == [True, True] + [False] * 5
    assert _both([[0, 48, 224, 176]], 224, 224, 7, 7).reshape(7, 7)[0].tolist() == [False] + [True] * 6
    assert _both([[0, 0, 224, 48]], 224, 224, 7, 7).reshape(7, 7)[0].tolist() == [True] + [False] * 6


def test_rule_non_square_image():
    # 200 x 300 on 7 x 7: row centres (2i+1) 200/14 = 14.29, 42.86, 71.43, 100, ...; column centres (2j+1) 300/14 = 21.43, 64.29, 107.14, 150, ...
    keep = _both([[43, 22, 57, 128]], 200, 300, 7, 7).reshape(7, 7)          # rows [43, 100), columns [22, 150)
    want = np.zeros((7, 7), bool)
    want[2:3, 1:3] = True                                                     # row 71.43 only (42.86 < 43, 100 excluded); columns 64.29, 107.14
    assert np.array_equal(keep, want)
    keep = _both([[43, 22, 58, 129]], 200, 300, 7, 7).reshape(7, 7)          # one pixel more each way takes the centres at 100 and 150 in
    want[2:4, 1:4] = True
    assert np.array_equal(keep, want)


def test_rule_560_on_18():
    # centres (2i+1) 560/36 = 15.56, 46.67, 77.78, ...: a fraction, never hit exactly
    keep = _both([[16, 0, 62, 560], [0, 47, 560, 31]], 560, 560, 18, 18)
    assert keep[0].reshape(18, 18)[:, 0].tolist() == [False, True, True] + [False] * 15        # [16, 78): 46.67 and 77.78
    assert keep[1].reshape(18, 18)[0].tolist() == [False, False, True] + [False] * 15          # [47, 78): 77.78
    assert keep.sum(1).tolist() == [2 * 18, 18]


# ---------------------------------------------------------------- the host check
def _check(region, B=2, h=224, w=224, r=7, c=7):
    from boosted_detr_amd.model import check_valid_region
    return check_valid_region(region, B, h, w, r, c)


def test_host_check_accepts_the_model_case():
    out = _check(R.MODEL_REGIONS)
    assert isinstance(out, np.ndarray) and out.dtype == np.int32 and np.array_equal(out, R.MODEL_REGIONS)


GOOD = [0, 0, 224, 224]
BAD_HOST = {
    "shape [B,3]": np.zeros((2, 3), np.int32),
    "shape [3,4] for B=2": np.array([GOOD] * 3, np.int32),
    "shape [8]": np.array(GOOD * 2, np.int32),
    "dtype int64": np.array([GOOD, GOOD], np.int64),
    "dtype float32": np.array([GOOD, GOOD], np.float32),
    "top < 0": np.array([GOOD, [-1, 0, 100, 100]], np.int32),
    "left < 0": np.array([GOOD, [0, -1, 100, 100]], np.int32),
    "height < 1": np.array([GOOD, [10, 10, 0, 100]], np.int32),
    "width < 1": np.array([GOOD, [10, 10, 100, 0]], np.int32),
    "past the bottom": np.array([GOOD, [125, 0, 100, 100]], np.int32),
    "past the right": np.array([[0, 200, 100, 25], GOOD], np.int32),
    "no kept token": np.array([GOOD, [17, 17, 1, 1]], np.int32),
}


@pytest.mark.parametrize("what", sorted(BAD_HOST))
def test_host_check_refuses(what):
    with pytest.raises(ValueError):
        _check(BAD_HOST[what])


def test_host_check_takes_a_host_torch_tensor_as_a_host_array():
    import torch
    assert np.array_equal(_check(torch.from_numpy(R.MODEL_REGIONS.copy())), R.MODEL_REGIONS)
    with pytest.raises(ValueError):
        _check(torch.tensor([GOOD, [17, 17, 1, 1]], dtype=torch.int32))


# ---------------------------------------------------------------- the mask matters on the model case
def test_masked_and_unmasked_oracle_are_far_apart_on_the_model_case():
    """If they were close, a model that ignores `valid_region` could pass the GPU parity test.  Measured (fp64, image 1): 98.7 % of the
    category probabilities differ by more than 1e-2 relative, the match differs, 99 % of the gradient tensors differ by more than
    5e-2 in relative L2."""
    cfg, batch, params = R.model_case()
    masked, g_masked = R.reference("model", True, 64)
    plain, g_plain = R.reference("model", False, 64)
    assert set(masked.probes) == set(plain.probes)
    a, b = masked.cat_preds.detach().numpy()[1], plain.cat_preds.detach().numpy()[1]
    share = float((np.abs(a - b) > 10 * RTOL * np.abs(a)).mean())
    print(f"image 1 category probabilities differing by > {10 * RTOL:g} relative: {100 * share:.1f} %")
    assert share >= 0.90
    B, M = batch["bbox"].shape[:2]
    assert not np.array_equal(R.match_matrix(masked, B, M)[1], R.match_matrix(plain, B, M)[1])
    gmax = max(np.abs(g).max() for g in g_masked.values())
    names = [k for k, g in g_masked.items() if np.abs(g).max() >= 1e-6 * gmax]          # (the structurally-zero ones: check_grads skips them too)
    far = [k for k in names if R.grad_rel_l2(g_plain[k], g_masked[k]) > 5e-2]
    print(f"gradient tensors with relative L2 difference > 5e-2: {len(far)} of {len(names)}")
    assert len(names) > 100 and len(far) >= 0.90 * len(names)


def test_masked_net_masks_by_layer_name():
    masked, _ = R.reference("model", True, 64)
    cfg, batch, params = R.model_case()
    net = R.MaskedNet(cfg, params, R.keep_of(cfg, batch, R.MODEL_REGIONS))
    from oracle import detr_oracle as O
    O.forward(net, {"image": batch["image"]}, training=False)
    want = [f"ImageEncoderAttention/EncoderBlock_{i}/SelfAttentionBlock/AttentionLayer" for i in range(2)] + \
           [f"DecoderBlock_{i}/JointAttentionBlock/AttentionLayer" for i in range(2)]
    assert net.masked_layers == want
    assert R.masks_keys("ImageEncoderAttention_2/EncoderBlock_0/SelfAttentionBlock/AttentionLayer")
    assert not R.masks_keys("DecoderBlock_1/SelfAttentionBlock/AttentionLayer")
