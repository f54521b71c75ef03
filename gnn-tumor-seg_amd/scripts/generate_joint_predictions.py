"""Chain a trained GNN and refinement CNN over a preprocessed dataset and save the predicted
segmentations.

Command line and output files follow /root/reference/scripts/generate_joint_predictions.py:
27-110.  Per sample everything between the graph forward pass and the finished label volume
stays on the GPU:

    node logits --K12 (arg-max + projection + tumour-plane flags)--> crop box (3 small vectors
    to the host, 1-D dilation) --K16 (crop + image/logit concat, channels-first)--> Conv3d x2
    (MIOpen) --K17 (channel arg-max scattered into the zero volume, BraTS relabel)--> host.

The reference materialises the [X,Y,Z,4] voxel logits, copies them to the host for an argmax
and a 3-D dilation, and builds the [X,Y,Z,8] concatenation before cropping.

--also_gnn_weights P [P ...] with --also_cnn_weights P [P ...] (further members, e.g. the other folds, paired in
order) and --tta_mirror AXES (mirrored views of the CNN, a non-empty subset of xyz) average class probabilities over
all members and views before the arg-max (gts.ensemble, DESIGN.md 4s: the convolutions then run on the HIP kernels).
Without them the path above runs, unchanged.
"""
import argparse
import os
import sys

import numpy as np
import torch

import Filepaths
from data_processing import data_loader, nifti_io
from data_processing.image_processing import (tumor_crop_from_plane_flags, uncrop_maps_to_brats_size,
                                              uncrop_to_brats_size)
from data_processing.labels import INTERNAL_TO_BRATS
from gts import ops
from model.cnn_model import combine_node_logits_and_image
from model.networks import CnnRefinementNet, init_graph_net
from scripts import cleanup as cleanup_flags
from scripts import ensemble_flags
from utils.hyperparam_helpers import DEFAULT_BACKGROUND_NODE_LOGITS, EvalParamSet

output_dir = None


def _device():
    if not torch.cuda.is_available():
        raise RuntimeError("generate_joint_predictions needs an AMD GPU (no CPU fallback)")
    return torch.device("cuda", torch.cuda.current_device())


def load_nets(gnn_type, gnn_weights, cnn_weights,
              gnn_hp=EvalParamSet(in_feats=20, out_classes=4, layer_sizes=[256] * 4, gat_heads=None,
                                  gat_residuals=None),
              cnn_hp=EvalParamSet(in_feats=8, out_classes=4, layer_sizes=[16], gat_heads=None,
                                  gat_residuals=None)):
    """Architectures must correspond to the weight files (the reference hard-codes these two)."""
    device = _device()
    graph_net = init_graph_net(gnn_type, gnn_hp).to(device)
    conv_net = CnnRefinementNet(cnn_hp.in_feats, cnn_hp.out_classes, cnn_hp.layer_sizes).to(device)
    graph_net.load_state_dict(torch.load(gnn_weights, map_location=device, weights_only=True))
    conv_net.load_state_dict(torch.load(cnn_weights, map_location=device, weights_only=True))
    graph_net.eval()
    conv_net.eval()
    return graph_net, conv_net


def _on_device(x, device, dtype=None):
    """A tensor (kept where it is when already on the device) or an array, as a tensor on device."""
    t = x if isinstance(x, torch.Tensor) else torch.as_tensor(np.asarray(x), dtype=dtype)
    return t.to(device=device, dtype=dtype or t.dtype)


def gnn_crop_box(svs, node_logits, cleanup=None):
    """The CNN's crop box: the (dilated) box around the GNN-predicted tumour, from K12's plane flags.
    With a `cleanup` that drops components, the box of the prediction that SURVIVES it: the arg-max is
    projected to voxels, filtered, and the plane flags are taken from what is left, so that one stray
    supervoxel does not inflate the box.  Nothing left: as for an empty prediction, the whole volume."""
    if cleanup is not None and cleanup.drops_components:
        kept = cleanup.surviving(ops.project_argmax(svs, node_logits)) != 0
        plane_flags = [torch.any(kept, dim=1).any(dim=1), torch.any(kept, dim=0).any(dim=1),
                       torch.any(kept, dim=0).any(dim=0)]
    else:
        _, plane_flags = ops.project_argmax_occupancy(svs, node_logits)                     # K12
    crop = tumor_crop_from_plane_flags(*[f.cpu().numpy() for f in plane_flags])
    return ops.CropBox(*[c.reshape(-1) for c in crop], svs.shape, svs.device)


def predict_one_sample(graph_net, conv_net, graph, node_feats, img, supervoxel_partitioning, relabel=None,
                       cleanup=None):
    """int16 label volume of the partitioning's shape: GNN prediction refined by the CNN inside
    the (dilated) box around the GNN-predicted tumour, healthy outside (reference :59-73).
    `relabel` (optional int16 table on the device) maps the labels on the way out.  The features,
    image and partitioning may be numpy arrays or tensors already on the device.
    `cleanup` (optional scripts.cleanup.Cleanup) removes small components on the device: from the GNN
    prediction the crop box is taken from, and from the finished volume, which it expects in BraTS
    coding (relabel = INTERNAL_TO_BRATS); its stats of the finished volume stay in cleanup.last_stats."""
    device = _device()
    with torch.no_grad():
        graph = graph.to(device)
        node_feats = _on_device(node_feats, device, torch.float32)
        img = _on_device(img, device, torch.float32)
        svs = _on_device(supervoxel_partitioning, device)
        node_logits = graph_net(graph, node_feats).float()
        box = gnn_crop_box(svs, node_logits, cleanup)
        cnn_in = combine_node_logits_and_image(node_logits, DEFAULT_BACKGROUND_NODE_LOGITS, svs, img, box)  # K16
        refined_voxel_logits = conv_net(cnn_in)
        pred = ops.argmax_scatter(refined_voxel_logits.float(), box, relabel)               # K17
        if cleanup is not None:
            pred = cleanup(pred)
        return pred.cpu().numpy()


def save_predictions(graph_net, conv_net, dataset, cleanup=None):
    relabel = torch.from_numpy(INTERNAL_TO_BRATS).to(_device())
    for mri, graph, node_feats, img in dataset:
        try:
            supervoxel_partitioning = dataset.get_supervoxel_partitioning(mri)
            raw_data_crop = dataset.get_crop(mri)
        except FileNotFoundError as e:
            raise FileNotFoundError(f"Couldnt predict {mri} because couldn't read in a required file: {e}")
        pred = predict_one_sample(graph_net, conv_net, graph, node_feats, img, supervoxel_partitioning, relabel,
                                  cleanup=cleanup)
        nifti_io.save_as_nifti(uncrop_to_brats_size(raw_data_crop, pred), f"{output_dir}{os.sep}{mri}.nii.gz")
        if cleanup is not None:
            print(f"{mri}: {cleanup.report()}")


def save_ensemble_predictions(predictor, dataset, cleanup=None, uncertainty_dir=None):
    """save_predictions for a gts.ensemble.EnsemblePredictor (--also_*_weights, --tta_mirror): same files, the
    ensemble's labels in them.  uncertainty_dir: the scan's three region maps go there as well."""
    relabel = torch.from_numpy(INTERNAL_TO_BRATS).to(_device())
    for mri, graph, node_feats, img in dataset:
        try:
            supervoxel_partitioning = dataset.get_supervoxel_partitioning(mri)
            raw_data_crop = dataset.get_crop(mri)
        except FileNotFoundError as e:
            raise FileNotFoundError(f"Couldnt predict {mri} because couldn't read in a required file: {e}")
        pred = predictor.predict_joint(graph, node_feats, img, supervoxel_partitioning, relabel, cleanup=cleanup,
                                       return_uncertainty=bool(uncertainty_dir))
        if uncertainty_dir:
            pred, unc = pred
            ensemble_flags.save_uncertainty_maps(uncertainty_dir, mri, uncrop_maps_to_brats_size(raw_data_crop, unc))
        nifti_io.save_as_nifti(uncrop_to_brats_size(raw_data_crop, pred), f"{output_dir}{os.sep}{mri}.nii.gz")
        if cleanup is not None:
            print(f"{mri}: {cleanup.report()}")


_ARGUMENTS = [
    ("-d", "--data_dir", Filepaths.PROCESSED_DATA_DIR, "path to the directory where data is stored"),
    ("-p", "--data_prefix", "", "A prefix that all data folders share, i.e. BraTS2021."),
    ("-o", "--output_dir", None, "Directory to save predictions to"),
    ("-m", "--gnn_type", "GSpool", "What graph learning layer the saved model uses. GSpool, GSmean, GSgcn, GAT"),
    ("-c", "--cnn_weights", "", "Path to weights file for convolutional net"),
    ("-g", "--gnn_weights", "", "Path to weights file for graph net"),
]


def build_parser():
    parser = argparse.ArgumentParser()
    for short, long_, default, text in _ARGUMENTS:
        parser.add_argument(short, long_, default=default, help=text, type=str)
    return ensemble_flags.add_flags(cleanup_flags.add_flags(parser))


def main(argv=None):
    global output_dir
    args = build_parser().parse_args(argv)
    gnn_weights, cnn_weights = os.path.expanduser(args.gnn_weights), os.path.expanduser(args.cnn_weights)
    try:
        members = ensemble_flags.from_args(args, gnn_weights, cnn_weights)
    except ensemble_flags.FlagError as exc:
        print(f"generate_joint_predictions: {exc}", file=sys.stderr)
        return 2
    # the reference falls back on an attribute its parser never defines (:97); predictions go to PRED_DIR
    output_dir = os.path.expanduser(args.output_dir if args.output_dir else Filepaths.PRED_DIR)
    if not os.path.isdir(output_dir):
        print(f"Creating save directory: {output_dir}")
        os.makedirs(output_dir)
    dataset = data_loader.ImageGraphDataset(os.path.expanduser(args.data_dir), args.data_prefix,
                                            read_image=True, read_graph=True, read_label=False)
    if members is not None:
        save_ensemble_predictions(members.predictor(args.gnn_type), dataset, cleanup_flags.from_args(args),
                                  ensemble_flags.uncertainty_dir(args))
        print(f"Finished saving predictions generated by an ensemble of {members.describe()} in folder {output_dir}")
        return 0
    graph_net, conv_net = load_nets(args.gnn_type, gnn_weights, cnn_weights)
    save_predictions(graph_net, conv_net, dataset, cleanup_flags.from_args(args))
    print(f"Finished saving predictions generated by {args.gnn_weights} and {args.cnn_weights} "
          f"in folder {output_dir}")
    return 0


if __name__ == "__main__":
    sys.exit(main())
