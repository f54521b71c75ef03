"""The joint GNN -> CNN training step's voxel path as ONE autograd node.

`joint_refinement_logits(node_logits, img, svs, box, bg_row, net)` crops and concatenates the image with
the node logits projected onto the partitioning (J1, channels-last), runs the two Conv3d layers of a
`model.networks.CnnRefinementNet` on the HIP kernels of gts.conv3d (C1, C2) and returns logits [V, Cout].
Backward gives the four CNN parameter gradients (C4, C3, C5, as `gts.conv3d.refinement_logits`) and,
through conv1's data gradient on the logit channels alone and the adjoint of J1 (J2), d node_logits [N, Ct].
The image, the box and the background row take no gradient.

With `augment` (a gts.augment.AugmentPlan) the assembled input is mirrored and its image channels jittered (A1,
gts.ops.augment_crop) before conv1; backward mirrors conv1's data gradient back (a mirror is its own adjoint)
before J2; under a spatial plan (a rotation and zoom, A3) it is the adjoint of the resample and the
mirror (A4, gts.ops.spatial_crop_bwd).  J1 and J2 are the same calls either way.
"""
import torch

from . import _lib, ops
from ._lib import require_device
from ._operands import f32
from .conv3d import conv3d_bwd_data, conv3d_bwd_weight, conv3d_fwd


class _JointRefinement(torch.autograd.Function):
    @staticmethod
    def forward(ctx, node_logits, w1, b1, w2, b2, img, svs, bg_row, box, lists, augment):
        table = node_logits.contiguous()
        x = ops.crop_concat_rows(img, svs, table, bg_row, box)
        if augment is not None:
            x = ops.augment_crop(x, None, augment)[0]       # the saved x is the augmented one: conv1's dW uses it
        h1 = conv3d_fwd(x, w1, b1, relu=True)
        y = conv3d_fwd(h1.view(*x.shape[:3], -1), w2, b2, relu=False)
        ctx.save_for_backward(x, h1, w1, w2)
        ctx.box, ctx.lists, ctx.ct = box, lists, table.shape[1]
        ctx.flips = augment.flips if augment is not None and any(augment.flips) else None
        ctx.spatial = augment if augment is not None and augment.spatial else None
        return y

    @staticmethod
    def backward(ctx, dy):
        x, h1, w1, w2 = ctx.saved_tensors
        dims = tuple(x.shape[:3])
        dy = dy.contiguous()
        dw2, db2 = conv3d_bwd_weight(h1.view(*dims, -1), dy, w2.shape[0])
        dz1 = conv3d_bwd_data(dy, w2, dims, h=h1)
        dw1, db1 = conv3d_bwd_weight(x, dz1, w1.shape[0])
        d_nodes = None
        if ctx.needs_input_grad[0]:
            # C3 for conv1 on the logit channels only: the image channels' gradient is never formed
            ci = x.shape[3] - ctx.ct
            dx_logits = conv3d_bwd_data(dz1, w1[:, ci:].contiguous(), dims)
            if ctx.spatial is not None:     # the logit channels were mirrored and resampled: the adjoint of both
                dx_logits = ops.spatial_crop_bwd(dx_logits, dims, ctx.spatial)
            elif ctx.flips is not None:     # the logit channels were mirrored only: the adjoint is the same mirror
                dx_logits = ops.flip_crop(dx_logits, dims, ctx.flips)
            d_nodes = ops.crop_concat_rows_bwd(dx_logits, ctx.lists, ctx.box, 0)
        return d_nodes, dw1, db1, dw2, db2, None, None, None, None, None, None


def joint_refinement_logits(node_logits, img, svs, box, bg_row, net, lists=None, augment=None):
    """node_logits: fp32 [N, Ct] on the GPU (may require a gradient, may be a slice of a larger autograd
    tensor); img [X, Y, Z, Ci] fp32; svs [X, Y, Z] int16; box: a gts.ops.CropBox over the same volume;
    bg_row [Ct]; net: a CnnRefinementNet with Ci + Ct input channels.  `lists`: the gts.ops.SupervoxelLists
    built from this very `svs` tensor (`svs` is then `lists.svs`) for N rows; built here when not given, so a
    caller that steps on the same sample again should build it once and keep it.  `augment`: a
    gts.augment.AugmentPlan for img.shape[3] image channels, applied to the assembled input (the caller mirrors its
    labels with the same plan); None: no augmentation, the calls of before.  Returns logits [cx * cy * cz, Cout]."""
    c1, c2 = net.conv_layers[0], net.conv_layers[1]
    params = (c1.weight, c1.bias, c2.weight, c2.bias)
    if node_logits.dim() != 2 or img.dim() != 4:
        raise _lib.GtsError("joint_refinement_logits takes node logits [N, C] and an image [X, Y, Z, C]")
    f32(node_logits, img, bg_row, *params)
    img, svs, bg_row = img.contiguous(), svs.contiguous(), bg_row.contiguous()
    require_device(node_logits.detach().contiguous(), img, svs, bg_row, *[p.detach() for p in params])
    if img.shape[3] + node_logits.shape[1] != c1.in_channels or c2.in_channels != c1.out_channels:
        raise _lib.GtsError(f"image and node logits do not make up the network's {c1.in_channels} input channels")
    if lists is None:
        lists = ops.SupervoxelLists(svs, node_logits.shape[0], node_logits.device)
    if lists.n_rows != node_logits.shape[0] or lists.svs.data_ptr() != svs.data_ptr() \
            or lists.volume_shape != tuple(svs.shape):
        raise _lib.GtsError("supervoxel lists were built for another partitioning or node count: pass lists.svs")
    if augment is not None and augment.channels != img.shape[3]:
        raise _lib.GtsError(f"the plan holds {augment.channels} channels, the image {img.shape[3]}")
    return _JointRefinement.apply(node_logits, *params, img, svs, bg_row, box, lists, augment)
