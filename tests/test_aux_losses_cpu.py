"""Auxiliary decoder losses (DETR(use_intermediate_losses=True)): the CPU reference tests/_aux_ref.py against the oracle it is composed
from, the chained moving statistics of the shared heads, and the new C ABI symbols.  No GPU needed."""
import numpy as np
import torch

import _aux_ref as R
from oracle import detr_oracle as O

NEW_SYMBOLS = ("bdetr_bn_rows_stats", "bdetr_bn_rows_apply", "bdetr_bn_rows_bwd", "bdetr_cost_matrix_tiled", "bdetr_lsa_tiled", "bdetr_set_loss_tiled")


def test_one_block_reference_equals_oracle_forward():
    cfg = O.Config(image_size=(96, 96))
    batch = O.make_batch(cfg, 2, 20, seed=1234, num_objects=[3, 7])
    params = O.make_params(cfg, seed=0)
    want = O.forward(O.Net(cfg, params), batch, training=True)
    got = R.forward_aux(O.Net(cfg, params), batch)
    assert len(got.layers) == 1
    for a, b in ((got.layers[0].cat_preds, want.cat_preds), (got.layers[0].attribute_preds, want.attribute_preds), (got.layers[0].box_preds, want.box_preds),
                 (got.loss_vector, want.loss_vector)):
        assert torch.equal(a, b)
    for k, v in want.metrics.items():
        assert torch.equal(got.metrics[k], v), k
    assert sorted(got.new_moving) == sorted(want.new_moving)
    for k, v in want.new_moving.items():
        assert torch.equal(got.new_moving[k], v), k
    assert [(r.tolist(), c.tolist()) for r, c in got.layers[0].loss.matches] == [(r.tolist(), c.tolist()) for r, c in want.loss.matches]


def test_three_blocks_chain_the_heads_moving_statistics():
    cfg = R.SMALL_CFG
    batch = O.make_batch(cfg, seed=1234, **R.SMALL_BATCH_ARGS)
    params = O.make_params(cfg, seed=0)
    out = R.forward_aux(O.Net(cfg, params, dtype=torch.float64), batch)
    L, m = cfg.num_decoder_blocks, O.BN_MOMENTUM
    assert L == 3 and len(out.layers) == 3
    for h in R.HEAD_BN:
        for stat, per_block in (("moving_mean", out.head_means[h]), ("moving_variance", out.head_vars[h])):
            assert len(per_block) == L
            mm = torch.from_numpy(params[f"{h}/{stat}"]).double()
            closed = m ** L * mm + (1 - m) * sum(m ** (L - 1 - l) * per_block[l] for l in range(L))
            got = out.new_moving[f"{h}/{stat}"]
            assert torch.allclose(got, closed, rtol=1e-12, atol=1e-14), (h, stat, float((got - closed).abs().max()))
            # ... and it is NOT one update from the last block's statistics (what an un-chained reference would leave)
            assert not torch.allclose(got, m * mm + (1 - m) * per_block[-1], rtol=1e-6, atol=1e-9)
    # the summed loss is the sum of the three blocks' losses, IOU the last block's
    assert torch.equal(out.loss_vector, out.layers[0].loss.total + out.layers[1].loss.total + out.layers[2].loss.total)
    assert torch.equal(out.metrics["IOU"], out.layers[2].loss.iou)
    # moving statistics outside the heads are updated once, as in the plain step
    plain = O.forward(O.Net(cfg, params, dtype=torch.float64), batch, training=True)
    for k, v in plain.new_moving.items():
        if k not in R.HEAD_MOVING:
            assert torch.equal(out.new_moving[k], v), k


def test_new_abi_symbols_present_and_version_unchanged():
    import __graft_entry__
    __graft_entry__.build()
    from boosted_detr_amd import _lib
    for name in NEW_SYMBOLS:
        assert name in _lib.SIGNATURES
    text = (_lib.lib_path().parent.parent.parent / "include" / "bdetr.h").read_text()
    for name in NEW_SYMBOLS:
        assert f"int {name}(" in text, name
    h = _lib.lib()
    assert h.bdetr_abi_version() == 8
    for name in NEW_SYMBOLS:
        assert hasattr(h, name)
