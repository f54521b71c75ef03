"""Training harness and input assembly of the refinement CNN.

Counterpart of /root/reference/model/cnn_model.py:24-88: `RefinementModel` (constructor, `run_epoch`,
`evaluate`, `save_weights`) and `combine_logits_and_image`, plus the fused form the joint predictor uses
on the GPU.  Training runs both Conv3d layers and their backward on the HIP kernels of gts.conv3d
(C1-C5); `CnnRefinementNet.forward` itself is untouched.
"""
import queue
import threading

import numpy as np
import torch
from torch.utils.data import DataLoader

from data_processing.data_loader import collate_refinement_net
from gts import metrics as metrics_ops
from gts import ops
from gts.conv3d import refinement_logits
from gts.optim import FlatAdamW

from . import evaluation
from .losses import make_voxel_loss
from .networks import CnnRefinementNet


class RefinementModel:
    """Trains CnnRefinementNet on GNN voxel logits ++ image inside the crop around the GNN-predicted tumour.

    Same arithmetic as the reference: batch of one, shuffled; AdamW(lr, weight_decay) with ExponentialLR
    (one step per epoch); class-weighted cross-entropy (mean over the crop's voxels).  Differences:
      * everything runs on the GPU through HIP: both convolutions and their gradients (gts.conv3d), the loss
        (gts.ops.weighted_cross_entropy), AdamW (gts.optim.FlatAdamW), Dice counting (gts.ops.label_confusion);
        there is no CPU path;
      * the next sample's logits are decoded, concatenated and cropped on a host thread while the current step
        runs (`prefetch=True`; same samples, same order), and the loss is read back once per epoch;
      * `ExponentialLR(..., verbose=False)` raises on current PyTorch; the kwarg is dropped.
    Two reference quirks are kept on purpose, so results stay comparable with the reference's:
      * a sample whose logit file is missing is skipped (FileNotFoundError), in training and in evaluation;
      * in `evaluate` the row of such a sample stays all zeros and is still averaged into the returned mean.
    HD95 is computed, as in the reference, on the [1, cx, cy, cz] arrays of the crop.
    `voxel_loss`: a callable (logits, labels) -> loss from model.losses.make_voxel_loss (soft Dice + cross-entropy);
    None is the reference's class-weighted cross-entropy.  Column 0 of `evaluate` is the configured loss.
    `augmenter`: a gts.augment.Augmenter; `run_epoch` then draws one plan per sample and mirrors / jitters (and, where
    the plan is spatial, rotates and zooms) the uploaded crop on the GPU (gts.ops.augment_crop).  `evaluate` is never augmented.  None: no augmentation.
    """

    def __init__(self, hyperparameters, train_dataset, logit_dataset, prefetch=True, voxel_loss=None,
                 augmenter=None):
        if not torch.cuda.is_available():
            raise RuntimeError("RefinementModel trains on an AMD GPU only (no CPU path)")
        self.device = torch.device("cuda", torch.cuda.current_device())
        self.class_weights = torch.tensor(hyperparameters.class_weights, dtype=torch.float32, device=self.device)
        self.voxel_loss = voxel_loss if voxel_loss is not None else make_voxel_loss("ce", self.class_weights)
        self.net = CnnRefinementNet(hyperparameters.in_feats, hyperparameters.out_classes,
                                    hyperparameters.layer_sizes).to(self.device)
        self.optimizer = FlatAdamW(self.net.parameters(), lr=hyperparameters.lr,
                                   weight_decay=hyperparameters.w_decay)
        self.lr_decay = torch.optim.lr_scheduler.ExponentialLR(self.optimizer, hyperparameters.lr_decay,
                                                               last_epoch=-1)
        self.train_loader = DataLoader(train_dataset, batch_size=1, shuffle=True, num_workers=0,
                                       collate_fn=collate_refinement_net) if train_dataset is not None else None
        self.logit_dataset = logit_dataset
        self.prefetch = prefetch
        self.augmenter = augmenter

    def _cropped(self, mri, img, lab):
        """(input float32 [cx, cy, cz, C], labels int64 [V]) of one sample, or None when its logits are missing."""
        try:
            gnn_out, crop = self.logit_dataset.get_one(mri)
        except FileNotFoundError:
            return None
        img = np.asarray(img, dtype=np.float32)
        x = np.concatenate([img, np.asarray(gnn_out, dtype=np.float32)], axis=-1)[crop]
        y = np.asarray(lab)[crop].astype(np.int64).reshape(-1)
        return torch.from_numpy(np.ascontiguousarray(x)), torch.from_numpy(y)

    def _samples(self, items):
        """Cropped host samples of `items` in order (None for a skipped one), produced one ahead on a thread."""
        if not self.prefetch:
            for mri, img, lab in items:
                yield self._cropped(mri, img, lab)
            return
        box = queue.Queue(maxsize=1)
        stop = threading.Event()
        done = object()

        def put(item):
            """Hand one item over; give up when the consumer has gone away."""
            while not stop.is_set():
                try:
                    box.put(item, timeout=0.1)
                    return True
                except queue.Full:
                    pass
            return False

        def produce():
            try:
                for mri, img, lab in items:
                    if not put(self._cropped(mri, img, lab)):
                        return
            except BaseException as e:  # surfaced in the consuming thread
                put(e)
                return
            put(done)

        worker = threading.Thread(target=produce, name="gts-cnn-prefetch", daemon=True)
        worker.start()
        try:
            while True:
                item = box.get()
                if item is done:
                    break
                if isinstance(item, BaseException):
                    raise item
                yield item
        finally:            # also when the consumer stops early (an exception in its step, or close())
            stop.set()
            worker.join()

    def train_step(self, x, y):
        """One forward / backward / AdamW step on a cropped sample already on the device; returns the loss
        as a device scalar."""
        logits = refinement_logits(x, self.net)
        loss = self.voxel_loss(logits, y)
        self.optimizer.zero_grad()
        loss.backward()
        self.optimizer.step()
        return loss.detach()

    def run_epoch(self):
        self.net.train()
        losses = []
        for sample in self._samples(self.train_loader):
            if sample is None:
                continue
            x, y = (t.to(self.device, non_blocking=False) for t in sample)
            if self.augmenter is not None:
                x, y = ops.augment_crop(x, y, self.augmenter.draw())
            losses.append(self.train_step(x, y))
        self.lr_decay.step()
        if not losses:
            return float("nan")      # numpy.mean([]) in the reference
        return float(np.mean(torch.stack(losses).cpu().numpy()))

    @torch.no_grad()
    def evaluate(self, dataset=None):
        """Mean over `dataset` of [loss, WT / CT / ET voxel Dice, WT / CT / ET HD95] inside each sample's crop."""
        self.net.eval()
        metrics = np.zeros((len(dataset), 7))
        i = 0
        items = ((mri, img, lab) for mri, img, lab in dataset)
        for sample in self._samples(items):
            if sample is None:
                continue
            shape = tuple(sample[0].shape[:3])
            x, y = (t.to(self.device) for t in sample)
            logits = refinement_logits(x, self.net)
            loss = self.voxel_loss(logits, y)
            pred = torch.argmax(logits, dim=1).to(torch.int16)
            truth = y.to(torch.int16)
            confusion = ops.label_confusion(pred, truth)
            # the reference passes [1, cx, cy, cz] arrays: the unit axis makes every region voxel border
            hd95s = metrics_ops.hd95s(pred.reshape((1,) + shape), truth.reshape((1,) + shape))
            metrics[i][0] = float(loss)
            metrics[i][1:4] = evaluation.dices_from_confusion(confusion.cpu().numpy())
            metrics[i][4:] = hd95s
            i += 1
        return np.mean(metrics, axis=0)

    def save_weights(self, folder, name):
        torch.save(self.net.state_dict(), f"{folder}{name}.pt")


def combine_logits_and_image(gnn_out, img, tumor_crop):
    """[1, C_img + C_logits, cx, cy, cz] from channels-last voxel logits [X,Y,Z,Cl], image
    [X,Y,Z,Ci] and an np.ix_ crop — the reference's signature, for callers that already hold the
    voxel-logit volume (e.g. read back from disk)."""
    combined = torch.cat([img, gnn_out], dim=-1)[tumor_crop]
    return combined.movedim(-1, 0).unsqueeze(0)


def combine_node_logits_and_image(node_logits, background_logits, supervoxel_partitioning, img, box):
    """Same tensor straight from the NODE logits, in one K16 pass on the GPU:
    cat([img, cat(node_logits, background)[svs]], -1)[box] moved to channels-first; neither the
    voxel-logit volume nor the concatenation is materialised.  `box` is a gts.ops.CropBox."""
    bg = torch.as_tensor(background_logits, dtype=torch.float32, device=node_logits.device).reshape(-1)
    return ops.crop_concat(img, supervoxel_partitioning, node_logits.float(), bg, box)
