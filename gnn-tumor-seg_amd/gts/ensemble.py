"""Ensemble prediction: several weight sets (the folds of one training run) and mirrored views, averaged as
class probabilities before the arg-max.

M members (a GNN, plus a CNN in joint use) and V views (the subsets of the chosen mirror axes, identity first):

  1. node probabilities  P = mean over members of softmax(gnn_m(graph, feats))            (E1 on [N, 4])
  2. one crop box        gnn_crop_box(svs, P, cleanup): the existing arg-max + plane flags, fed probabilities
  3. per member          x_m = crop_concat_rows(img, svs, L_m, background, box)            (J1; its OWN node logits)
     per view            y_mv = unmirror_v(cnn_m(mirror_v(x_m)))                           (C1 + ReLU, C2)
  4. voxel probabilities mean over all M * V of softmax(y_mv), member-major, view-minor   (E1 on [V, 4])
  5. labels              first-maximum arg-max, relabelled and scattered at the box         (E2), then `cleanup`

A mirror is never applied to data.  CnnRefinementNet is conv -> ReLU -> conv with replicate padding, and replicate
padding is symmetric, so unmirror(cnn(mirror(x))) is the same net with both weight tensors flipped along the
mirrored axes: a view is a `torch.flip` of two small weight tensors, made once in the constructor.  The supervoxel
features are quantiles, which a mirror leaves alone, so views do not apply to the GNN.

The arg-max is taken on the SUM E1 leaves (the mean times M * V): it orders the classes as the mean does, with one
rounding less.  The single-model path (generate_joint_predictions.predict_one_sample) is not used and not changed.
"""
import torch

from . import _lib, ops
from .conv3d import MAX_CHANNELS, conv3d_fwd

MIRROR_AXES = "xyz"
MAX_HELD_LOGITS = 8     # logit tensors alive at a time: one E1 launch takes as many by value


def mirror_views(axes):
    """The views of the mirror axes `axes` (a string or iterable out of 'x', 'y', 'z'; empty or None: no mirrors) as
    flip triples (x, y, z): every subset of the axes, the identity first, the rest in ascending order of the mask
    x = 1, y = 2, z = 4 (the convention of gts.ops.flip_crop and AugmentPlan.flip_mask)."""
    axes = "" if axes is None else "".join(axes).lower()
    if any(a not in MIRROR_AXES for a in axes) or len(set(axes)) != len(axes):
        raise ValueError(f"mirror axes must be a subset of '{MIRROR_AXES}' without repeats, got {axes!r}")
    chosen = sum(1 << MIRROR_AXES.index(a) for a in axes)
    return [tuple(bool(mask >> a & 1) for a in range(3)) for mask in range(8) if mask & ~chosen == 0]


def mirrored_cnn_weights(net, flips):
    """(w1, b1, w2, b2) of a CnnRefinementNet for the view `flips` (x, y, z): both weight tensors flipped along the
    mirrored spatial axes, the biases as they are; detached and contiguous.  Running the net with them on x equals
    unmirror(net(mirror(x)))."""
    flips = tuple(bool(f) for f in flips)
    if len(flips) != 3:
        raise ValueError("flips are three booleans (x, y, z)")
    if len(net.conv_layers) != 2:
        raise _lib.GtsError("the mirrored weights are those of a two-layer CnnRefinementNet")
    dims = [2 + a for a in range(3) if flips[a]]       # Conv3d weight is [Cout, Cin, kx, ky, kz]
    out = []
    for conv in net.conv_layers:
        w = conv.weight.detach()
        out += [(torch.flip(w, dims) if dims else w).contiguous(), conv.bias.detach().contiguous()]
    return tuple(out)


class EnsemblePredictor:
    """graph_nets: the members' GNNs, on the GPU, in eval mode; conv_nets: their CnnRefinementNets in the same
    order, or None for GNN-only prediction; views: flip triples as mirror_views returns them (default: the identity
    alone).  Every method runs under torch.no_grad() and leaves the nets as they are."""

    def __init__(self, graph_nets, conv_nets=None, views=None):
        self.graph_nets = list(graph_nets)
        if not self.graph_nets:
            raise ValueError("an ensemble needs at least one member")
        self.views = [tuple(bool(f) for f in v) for v in (views if views is not None else mirror_views(""))]
        if not self.views or any(len(v) != 3 for v in self.views):
            raise ValueError("views are flip triples (x, y, z)")
        self.conv_weights = None
        if conv_nets is not None:
            conv_nets = list(conv_nets)
            if len(conv_nets) != len(self.graph_nets):
                raise ValueError(f"{len(self.graph_nets)} graph nets but {len(conv_nets)} convolutional nets")
            for net in conv_nets:
                self._check_cnn(net)
            if len({(n.conv_layers[0].in_channels, n.conv_layers[1].out_channels) for n in conv_nets}) != 1:
                raise _lib.GtsError("the members' CNNs disagree in their input or class counts")
            with torch.no_grad():
                self.conv_weights = [[mirrored_cnn_weights(net, v) for v in self.views] for net in conv_nets]

    @staticmethod
    def _check_cnn(net):
        layers = getattr(net, "conv_layers", ())
        if len(layers) != 2:
            raise _lib.GtsError("an ensemble member's CNN must be a two-layer CnnRefinementNet")
        c1, c2 = layers
        for conv in (c1, c2):
            if tuple(conv.kernel_size) != (5, 5, 5) or conv.padding_mode != "replicate" or conv.bias is None \
                    or tuple(conv.stride) != (1, 1, 1) or conv.weight.dtype != torch.float32:
                raise _lib.GtsError("the HIP convolutions take fp32 5x5x5 stride-1 replicate-padded layers with a bias")
            if not (1 <= conv.in_channels <= MAX_CHANNELS and 1 <= conv.out_channels <= MAX_CHANNELS):
                raise _lib.GtsError(f"conv3d: channel counts {conv.in_channels} -> {conv.out_channels} outside "
                                    f"1..{MAX_CHANNELS}")
        if c2.in_channels != c1.out_channels:
            raise _lib.GtsError("the CNN's layers do not chain")
        if not 1 <= c2.out_channels <= ops.SOFTMAX_ACCUMULATE_MAX_CLASSES:
            raise _lib.GtsError(f"the CNN's {c2.out_channels} classes are more than the probability kernel takes")

    @property
    def terms(self):
        """Number of CNN logit sets behind one voxel: members times views."""
        return len(self.graph_nets) * len(self.views)

    @staticmethod
    def _device():
        if not torch.cuda.is_available():
            raise RuntimeError("ensemble prediction needs an AMD GPU (no CPU fallback)")
        return torch.device("cuda", torch.cuda.current_device())

    @staticmethod
    def _on_device(x, device, dtype=None):
        import numpy as np

        t = x if isinstance(x, torch.Tensor) else torch.as_tensor(np.asarray(x), dtype=dtype)
        return t.to(device=device, dtype=dtype or t.dtype)

    def _node_logits(self, graph, feats):
        """(the members' node logits [N, C] in member order, the sum of their softmax)."""
        logits, total = [], None
        for first in range(0, len(self.graph_nets), MAX_HELD_LOGITS):
            held = [net(graph, feats).float().contiguous() for net in self.graph_nets[first:first + MAX_HELD_LOGITS]]
            total = ops.softmax_accumulate(held, total)
            logits += held          # [N, C] tables: kept, each member's CNN reads its own
        return logits, total

    def node_probabilities(self, graph, feats):
        """Step 1: the mean over the members of softmax(gnn(graph, feats)), fp32 [N, C] on the device."""
        device = self._device()
        with torch.no_grad():
            _, total = self._node_logits(graph.to(device), self._on_device(feats, device, torch.float32))
            return total.div_(len(self.graph_nets))

    def predict_gnn(self, graph, feats, svs, relabel=None, cleanup=None, return_uncertainty=False):
        """GNN-only prediction: int16 label volume of the partitioning's shape (numpy), project_argmax of the mean
        node probabilities, then the optional `cleanup` (which expects BraTS coding: relabel = INTERNAL_TO_BRATS).
        With return_uncertainty: (labels, uint8 [3, X, Y, Z] numpy), the region maps of DESIGN.md 4u over the
        members' node probabilities (U1n); `cleanup` changes labels only, never the maps."""
        device = self._device()
        with torch.no_grad():
            svs = self._on_device(svs, device)
            _, total = self._node_logits(graph.to(device), self._on_device(feats, device, torch.float32))
            pred = ops.project_argmax(svs, total, relabel)
            if cleanup is not None:
                pred = cleanup(pred)
            labels = pred.cpu().numpy()
            if return_uncertainty:
                return labels, ops.region_uncertainty_nodes(svs, total, len(self.graph_nets)).cpu().numpy()
            return labels

    def predict_joint(self, graph, feats, img, svs, relabel=None, cleanup=None, return_probabilities=False,
                      return_uncertainty=False):
        """Steps 1-5: int16 label volume of the partitioning's shape (numpy), the ensemble's CNN prediction inside
        the one crop box all members share, healthy outside.  Operands as predict_one_sample.  With
        return_probabilities: (labels, mean probabilities fp32 [cx, cy, cz, C] on the device, the CropBox).  With
        return_uncertainty a uint8 [3, X, Y, Z] numpy array follows the labels: the region maps of DESIGN.md 4u,
        from the class sums before the division (U1), 0 outside the box; `cleanup` never changes them."""
        from scripts.generate_joint_predictions import gnn_crop_box
        from utils.hyperparam_helpers import DEFAULT_BACKGROUND_NODE_LOGITS

        if self.conv_weights is None:
            raise _lib.GtsError("this ensemble holds no convolutional nets: use predict_gnn")
        device = self._device()
        with torch.no_grad():
            graph = graph.to(device)
            feats = self._on_device(feats, device, torch.float32)
            img = self._on_device(img, device, torch.float32).contiguous()
            svs = self._on_device(svs, device).contiguous()
            node_logits, node_total = self._node_logits(graph, feats)
            box = gnn_crop_box(svs, node_total, cleanup)        # an arg-max only: the sum serves as the mean does
            bg = torch.tensor(DEFAULT_BACKGROUND_NODE_LOGITS, dtype=torch.float32, device=device).reshape(-1)
            if img.dim() != 4 or img.shape[3] + node_logits[0].shape[1] != self.conv_weights[0][0][0].shape[1]:
                raise _lib.GtsError("image and node logits do not make up the CNNs' input channels")
            total, held = None, []
            for table, views in zip(node_logits, self.conv_weights):
                x = ops.crop_concat_rows(img, svs, table, bg, box)                                  # J1
                for w1, b1, w2, b2 in views:
                    h1 = conv3d_fwd(x, w1, b1, relu=True)                                           # C1
                    held.append(conv3d_fwd(h1.view(*x.shape[:3], -1), w2, b2, relu=False))          # C2
                    del h1
                    if len(held) == MAX_HELD_LOGITS:
                        total = ops.softmax_accumulate(held, total)                                 # E1
                        held = []
            if held:
                total = ops.softmax_accumulate(held, total)
            pred = ops.argmax_scatter_rows(total, box, relabel)                                     # E2
            if cleanup is not None:
                pred = cleanup(pred)
            labels = pred.cpu().numpy()
            first = (labels,)
            if return_uncertainty:
                first += (ops.region_uncertainty_rows(total, self.terms, box).cpu().numpy(),)                # U1
            if return_probabilities:
                return first + (total.div_(self.terms).view(*box.shape, -1), box)
            return first if return_uncertainty else labels
