"""The voxel-level training objective of the refinement CNN and of joint training.

The reference trains on torch.nn.CrossEntropyLoss(weight=class_weights) alone
(its model/cnn_model.py); "dice_ce" adds the soft Dice over the BraTS regions the evaluation
reports, fused with the cross-entropy in two HIP passes (gts.ops.dice_ce_loss).
"""
from gts import ops

VOXEL_LOSS_KINDS = ("ce", "dice_ce")


def make_voxel_loss(kind, class_weights, dice_weight=1.0, smooth=1.0, regions="brats"):
    """A callable (logits [V, C], labels int64 [V]) -> scalar loss.  kind "ce": the class-weighted cross-entropy
    every loop trained on so far, the very call they made; "dice_ce": that cross-entropy plus `dice_weight` times
    one minus the mean soft Dice over `regions` ("brats", "classes" or class-index sets)."""
    if kind == "ce":
        def voxel_loss(logits, labels):
            return ops.weighted_cross_entropy(logits, labels, class_weights)
    elif kind == "dice_ce":
        if dice_weight < 0 or not smooth > 0:
            raise ValueError("dice_weight must not be negative and smooth must be positive")

        def voxel_loss(logits, labels):
            return ops.dice_ce_loss(logits, labels, class_weights, regions=regions, ce_weight=1.0,
                                    dice_weight=dice_weight, smooth=smooth)
    else:
        raise ValueError(f"unknown voxel loss {kind!r}: one of {VOXEL_LOSS_KINDS}")
    voxel_loss.kind = kind
    return voxel_loss
