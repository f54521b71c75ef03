"""Training harness that trains the GNN and the refinement CNN end to end.

The reference trains the two networks one after the other and names the joint form without building it
(/root/reference/scripts/train_refinement_cnn.py:21-22).  One step here, on one sample:

    node_logits  = graph_net(graph, feats)
    box          = tumour crop of argmax(node_logits) projected onto the partitioning (K12b, no gradient)
    voxel_logits = conv2(relu(conv1(cat([img, cat(node_logits, bg)[svs]], -1)[box])))        (J1, C1, C2)
    loss         = CE_w_cnn(voxel_logits, labels[box]) + gnn_loss_weight * CE_w_gnn(node_logits, node_labels)

and the backward pass carries the voxel loss through both convolutions, the crop and the projection (J2) into
the graph network.  `JointModel` has the surface utils.training_helpers.train_on_fold drives.
"""
import numpy as np
import torch
from torch.utils.data import DataLoader, Subset

from data_processing.image_processing import tumor_crop_from_plane_flags
from gts import dist as gdist
from gts import metrics as metrics_ops
from gts import nn as gnn
from gts import ops
from gts.conv3d import refinement_logits
from gts.joint import joint_refinement_logits
from gts.optim import FlatAdamW
from utils.hyperparam_helpers import DEFAULT_BACKGROUND_NODE_LOGITS

from . import evaluation
from .losses import make_voxel_loss
from .networks import CnnRefinementNet, init_graph_net

MAX_CACHED_SAMPLES = 32     # samples whose partitioning and voxel lists stay on the device between epochs


def _first(samples):
    return samples[0]


class JointModel:
    """GNN + refinement CNN trained on the sum of the voxel loss and `gnn_loss_weight` times the node loss.

    Batch of one sample, shuffled.  Each network has its own FlatAdamW and ExponentialLR (one step per
    epoch), built from its own hyper-parameter set; the class weights of the voxel loss come from the CNN
    set, those of the node loss from the GNN set.  `gnn_loss_weight = 0` trains both networks on the voxel
    loss alone.  `gnn_weights` / `cnn_weights`: optional checkpoints to start from (the intended use is
    fine-tuning a trained pair: an untrained GNN predicts tumour everywhere, so the crop is the whole
    brain).  `voxel_loss`: a callable (logits, labels) -> loss from model.losses.make_voxel_loss (soft Dice +
    cross-entropy) that replaces the voxel cross-entropy, in training and in column 0 of `evaluate`; None keeps the
    cross-entropy.  The node loss stays cross-entropy.  `augmenter`: a gts.augment.Augmenter; `run_epoch` then draws
    one plan per step, whose scale / shift go onto the node features before the graph network (so the crop comes from
    the augmented features) and onto the image channels of the CNN's input, and whose mirror goes onto that input, the
    labels and, backwards, the gradient (gts.ops.augment_features, gts.joint); a spatial plan (rotation and zoom) goes
    the same three ways, backwards as the adjoint of the resample.  `evaluate` is never augmented.
    Single GPU only."""

    def __init__(self, gnn_type, gnn_hp, cnn_hp, dataset, gnn_loss_weight=1.0, gnn_weights=None, cnn_weights=None,
                 voxel_loss=None, augmenter=None):
        if not torch.cuda.is_available():
            raise RuntimeError("JointModel needs an AMD GPU (MI355X): the HIP kernels have no CPU fallback")
        if gdist.world()[1] > 1:
            raise RuntimeError("JointModel trains on a single GPU: data-parallel joint training is not built")
        if gnn_loss_weight < 0:
            raise ValueError("gnn_loss_weight must not be negative")
        self.device = torch.device("cuda", torch.cuda.current_device())
        self.gnn_loss_weight = float(gnn_loss_weight)
        self.graph_net = init_graph_net(gnn_type, gnn_hp).to(self.device)
        self.conv_net = CnnRefinementNet(cnn_hp.in_feats, cnn_hp.out_classes, cnn_hp.layer_sizes).to(self.device)
        if gnn_weights:
            self.graph_net.load_state_dict(torch.load(gnn_weights, map_location=self.device, weights_only=True))
        if cnn_weights:
            self.conv_net.load_state_dict(torch.load(cnn_weights, map_location=self.device, weights_only=True))
        self.gnn_class_weights = torch.tensor(gnn_hp.class_weights, dtype=torch.float32, device=self.device)
        self.cnn_class_weights = torch.tensor(cnn_hp.class_weights, dtype=torch.float32, device=self.device)
        self.voxel_loss = voxel_loss if voxel_loss is not None else make_voxel_loss("ce", self.cnn_class_weights)
        self.bg_row = torch.tensor(DEFAULT_BACKGROUND_NODE_LOGITS, dtype=torch.float32, device=self.device).reshape(-1)
        self.gnn_optimizer = FlatAdamW(self.graph_net.parameters(), lr=gnn_hp.lr, weight_decay=gnn_hp.w_decay)
        self.cnn_optimizer = FlatAdamW(self.conv_net.parameters(), lr=cnn_hp.lr, weight_decay=cnn_hp.w_decay)
        self.gnn_lr_decay = torch.optim.lr_scheduler.ExponentialLR(self.gnn_optimizer, gnn_hp.lr_decay, last_epoch=-1)
        self.cnn_lr_decay = torch.optim.lr_scheduler.ExponentialLR(self.cnn_optimizer, cnn_hp.lr_decay, last_epoch=-1)
        self.grad_sink = gnn.GradSink(self.gnn_optimizer._params)
        self.train_loader = DataLoader(dataset, batch_size=1, shuffle=True, num_workers=0, collate_fn=_first) \
            if dataset is not None else None
        self._resident = {}
        self.augmenter = augmenter
        self.last_box = None              # the CropBox of the last training step
        self.last_node_logits = None      # ... and the node logits it was taken from (detached)

    # ---------------------------------------------------------------- samples
    @staticmethod
    def _source(dataset):
        return dataset.dataset if isinstance(dataset, Subset) else dataset

    def _partitioning(self, source, mri, n_nodes):
        """The sample's partitioning on the device with its per-node voxel lists: built on its first visit."""
        hit = self._resident.get(mri)
        if hit is None or hit.n_rows != n_nodes:
            hit = ops.SupervoxelLists(source.get_supervoxel_partitioning(mri), n_nodes, self.device)
            if len(self._resident) < MAX_CACHED_SAMPLES:
                self._resident[mri] = hit
        return hit

    def _to_device(self, source, sample):
        """(graph, feats, node_labels, img, svs, voxel_labels, lists) of one dataset item, on the device."""
        mri, graph, feats, node_labels, img, voxel_labels = sample
        feats = torch.as_tensor(np.asarray(feats), dtype=torch.float32).to(self.device)
        node_labels = torch.as_tensor(np.asarray(node_labels), dtype=torch.int64).to(self.device)
        img = torch.from_numpy(np.ascontiguousarray(img, dtype=np.float32)).to(self.device)
        voxel_labels = torch.from_numpy(np.ascontiguousarray(voxel_labels).astype(np.int64)).to(self.device)
        lists = self._partitioning(source, mri, feats.shape[0])
        return graph.to(self.device), feats, node_labels, img, lists.svs, voxel_labels, lists

    # ---------------------------------------------------------------- one step
    def crop_box(self, node_logits, svs):
        """The crop around the tumour the node logits predict (whole volume when they predict none), as the joint
        predictor takes it: K12b's plane flags, three small vectors to the host, 1-D dilation."""
        _, flags = ops.project_argmax_occupancy(svs, node_logits.detach())
        crop = tumor_crop_from_plane_flags(*[f.cpu().numpy() for f in flags])
        return ops.CropBox(*[c.reshape(-1) for c in crop], svs.shape, self.device)

    @staticmethod
    def cropped_labels(voxel_labels, box):
        xs, ys, zs = (d.long() for d in box.dev)
        return voxel_labels[xs[:, None, None], ys[None, :, None], zs[None, None, :]].reshape(-1)

    def _voxel_logits(self, graph, feats, img, svs, lists, plan=None):
        node_logits = self.graph_net(graph, feats).float()
        box = self.crop_box(node_logits, svs)
        return node_logits, box, joint_refinement_logits(node_logits, img, svs, box, self.bg_row, self.conv_net,
                                                         lists, augment=plan)

    def train_step(self, graph, feats, node_labels, img, svs, voxel_labels, lists=None, plan=None):
        """One forward / backward / two AdamW updates on one sample already on the device; returns the total loss
        as a device scalar.  `plan`: the gts.augment.AugmentPlan of this step (None: the sample as it is)."""
        if plan is not None:
            feats = ops.augment_features(feats, [feats.shape[0]], [plan])
        node_logits, box, voxel_logits = self._voxel_logits(graph, feats, img, svs, lists, plan)
        self.last_box, self.last_node_logits = box, node_logits.detach()
        labels = self.cropped_labels(voxel_labels, box)
        if plan is not None and (any(plan.flips) or plan.spatial):
            labels = ops.augment_crop(None, labels.view(box.shape), plan)[1].reshape(-1)
        loss = self.voxel_loss(voxel_logits, labels)
        if self.gnn_loss_weight:
            loss = loss + self.gnn_loss_weight * ops.weighted_cross_entropy(node_logits, node_labels,
                                                                            self.gnn_class_weights)
        self.gnn_optimizer.zero_grad()
        self.cnn_optimizer.zero_grad()
        flat = self.grad_sink.new_buffer()
        with gnn.grad_sink(self.grad_sink):
            loss.backward()
        if self.grad_sink.filled:          # the graph network was one fused stack: its gradients are in `flat`
            self.gnn_optimizer.step(flat_grad=flat)
        else:
            self.gnn_optimizer.step()
        self.cnn_optimizer.step()
        return loss.detach()

    def run_epoch(self):
        self.graph_net.train()
        self.conv_net.train()
        source = self._source(self.train_loader.dataset)
        if self.augmenter is None:
            losses = [self.train_step(*self._to_device(source, sample)) for sample in self.train_loader]
        else:
            losses = [self.train_step(*self._to_device(source, sample), plan=self.augmenter.draw())
                      for sample in self.train_loader]
        self.gnn_lr_decay.step()
        self.cnn_lr_decay.step()
        if not losses:
            return float("nan")
        return float(np.mean(torch.stack(losses).cpu().double().numpy()))

    # ---------------------------------------------------------------- evaluation
    @torch.no_grad()
    def evaluate(self, dataset):
        """Mean over `dataset` of [voxel loss, WT / CT / ET voxel Dice, WT / CT / ET HD95] inside each
        sample's own crop, from the joint forward (the columns of RefinementModel.evaluate)."""
        self.graph_net.eval()
        self.conv_net.eval()
        source = self._source(dataset)
        metrics = np.zeros((len(dataset), 7))
        for i in range(len(dataset)):
            graph, feats, _, img, svs, voxel_labels, _ = self._to_device(source, dataset[i])
            node_logits = self.graph_net(graph, feats).float()
            box = self.crop_box(node_logits, svs)
            x = ops.crop_concat_rows(img, svs, node_logits.contiguous(), self.bg_row, box)
            logits = refinement_logits(x, self.conv_net)
            y = self.cropped_labels(voxel_labels, box)
            loss = self.voxel_loss(logits, y)
            pred = torch.argmax(logits, dim=1).to(torch.int16)
            truth = y.to(torch.int16)
            confusion = ops.label_confusion(pred, truth)
            # as RefinementModel.evaluate: [1, cx, cy, cz] arrays, every region voxel is border
            hd95s = metrics_ops.hd95s(pred.reshape((1,) + box.shape), truth.reshape((1,) + box.shape))
            metrics[i][0] = float(loss)
            metrics[i][1:4] = evaluation.dices_from_confusion(confusion.cpu().numpy())
            metrics[i][4:] = hd95s
        return np.mean(metrics, axis=0)

    def save_weights(self, folder, name):
        torch.save(self.graph_net.state_dict(), f"{folder}{name}_gnn.pt")
        torch.save(self.conv_net.state_dict(), f"{folder}{name}_cnn.pt")
