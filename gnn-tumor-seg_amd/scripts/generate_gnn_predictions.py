"""Run a trained GNN over a preprocessed dataset and save voxel logits or predictions.

Command line and output files match /root/reference/scripts/generate_gnn_predictions.py:76-100.
The forward pass, the argmax and the node -> voxel projection all stay on the GPU
(K12 kernels); only the finished volume crosses PCIe for the NIfTI writer.

--also_gnn_weights P [P ...] (with -f preds) averages the node class probabilities of further weight files, e.g. the
other folds, with the first one's before the arg-max (gts.ensemble).  Logit files stay per member:
they feed that member's CNN training.

--uncertainty_dir DIR (with -f preds) also writes the three region uncertainty maps of the members' mean node
probabilities per scan (gts.uncertainty); alone it runs a one-member ensemble.
"""
import argparse
import os
import sys

import numpy as np
import torch

import Filepaths
from data_processing import data_loader, graph_io, nifti_io
from data_processing.image_processing import uncrop_maps_to_brats_size, uncrop_to_brats_size
from data_processing.labels import INTERNAL_TO_BRATS
from gts import dist as gdist
from gts import ops
from model.networks import init_graph_net
from scripts import cleanup as cleanup_flags
from scripts import ensemble_flags
from utils.hyperparam_helpers import DEFAULT_BACKGROUND_NODE_LOGITS, EvalParamSet

output_dir = None


def _device():
    if not torch.cuda.is_available():
        raise RuntimeError("generate_gnn_predictions needs an AMD GPU (no CPU fallback)")
    return torch.device("cuda", torch.cuda.current_device())


def load_net_and_weights(weight_file, model_type="GSpool",
                         gnn_hp=EvalParamSet(in_feats=20, out_classes=4, layer_sizes=[256] * 4,
                                             gat_heads=None, gat_residuals=None)):
    """Architecture must correspond to the weight file (reference :27-34 hard-codes this one)."""
    net = init_graph_net(model_type, gnn_hp)
    net.load_state_dict(torch.load(weight_file, map_location=_device(), weights_only=True))
    net.eval()
    return net


def save_voxel_logits(mri_id, dataset, node_logits):
    svs = torch.from_numpy(dataset.get_supervoxel_partitioning(mri_id)).to(node_logits.device)
    voxel_logits = graph_io.project_node_logits_to_img(svs, node_logits.detach(),
                                                       DEFAULT_BACKGROUND_NODE_LOGITS)
    # the reference's numpy concatenate with a Python list promotes to float64 before saving
    nifti_io.save_as_nifti(voxel_logits.cpu().numpy().astype(np.float64),
                           f"{output_dir}{os.sep}{mri_id}_logits.nii.gz")


def save_voxel_preds(mri_id, dataset, node_logits, cleanup=None):
    dev = node_logits.device
    svs = torch.from_numpy(dataset.get_supervoxel_partitioning(mri_id)).to(dev)
    relabel = torch.from_numpy(INTERNAL_TO_BRATS).to(dev)
    voxels = ops.project_argmax(svs, node_logits.detach().float(), relabel)
    if cleanup is not None:
        voxels = cleanup(voxels)                 # on the device, in BraTS coding, before the copy and the uncrop
    full = uncrop_to_brats_size(dataset.get_crop(mri_id), voxels.cpu().numpy())
    nifti_io.save_as_nifti(full, f"{output_dir}{os.sep}{mri_id}.nii.gz")
    if cleanup is not None:
        print(f"{mri_id}: {cleanup.report()}")


def save_predictions(net, dataset, save_format="logits", cleanup=None):
    if save_format not in ("preds", "logits"):
        raise ValueError(f"Unrecognized save format {save_format}")
    if cleanup is not None and save_format != "preds":
        raise ValueError("the component clean-up works on label volumes: use it with -f preds")
    device = _device()
    net = net.to(device)
    # under torchrun the samples are dealt round-robin over the ranks; every rank writes its own volumes
    for index in gdist.rank_share(len(dataset)):
        mri_id, graph, feats = dataset[index]
        graph = graph.to(device)
        feats = torch.FloatTensor(feats).to(device)
        with torch.no_grad():
            logits = net(graph, feats)
        if save_format == "preds":
            save_voxel_preds(mri_id, dataset, logits, cleanup)
        else:
            save_voxel_logits(mri_id, dataset, logits)


def save_ensemble_predictions(predictor, dataset, cleanup=None, uncertainty_dir=None):
    """save_predictions -f preds for a gts.ensemble.EnsemblePredictor (--also_gnn_weights): the arg-max of the
    members' mean node probabilities, projected to voxels; the ranks of a torchrun share the samples as above.
    uncertainty_dir: the scan's three region maps go there as well."""
    device = _device()
    relabel = torch.from_numpy(INTERNAL_TO_BRATS).to(device)
    for index in gdist.rank_share(len(dataset)):
        mri_id, graph, feats = dataset[index]
        svs = dataset.get_supervoxel_partitioning(mri_id)
        voxels = predictor.predict_gnn(graph, feats, svs, relabel, cleanup=cleanup,
                                       return_uncertainty=bool(uncertainty_dir))
        if uncertainty_dir:
            voxels, unc = voxels
            ensemble_flags.save_uncertainty_maps(uncertainty_dir, mri_id,
                                                 uncrop_maps_to_brats_size(dataset.get_crop(mri_id), unc))
        nifti_io.save_as_nifti(uncrop_to_brats_size(dataset.get_crop(mri_id), voxels),
                               f"{output_dir}{os.sep}{mri_id}.nii.gz")
        if cleanup is not None:
            print(f"{mri_id}: {cleanup.report()}")


_FLAGS = (
    ("-d", "--data_dir", Filepaths.PROCESSED_DATA_DIR, "preprocessed dataset directory"),
    ("-p", "--data_prefix", "", "common prefix of the sample folders, e.g. BraTS2021"),
    ("-o", "--output_dir", None, "where the volumes are written"),
    ("-w", "--weight_file", "", "checkpoint (state_dict) to load"),
    ("-f", "--save_format", "preds", "preds (label volumes at BraTS size) or logits (4-channel volumes)"),
)


def build_parser():
    parser = argparse.ArgumentParser(description="GNN inference + node-to-voxel projection on MI355X")
    for short, long_name, default, text in _FLAGS:
        parser.add_argument(short, long_name, default=default, type=str, help=text)
    return ensemble_flags.add_flags(cleanup_flags.add_flags(parser), cnn=False)


def main(argv=None):
    global output_dir
    args = build_parser().parse_args(argv)
    weight_file = os.path.expanduser(args.weight_file)
    try:
        members = ensemble_flags.from_args(args, weight_file, None, args.save_format)
    except ensemble_flags.FlagError as exc:
        print(f"generate_gnn_predictions: {exc}", file=sys.stderr)
        return 2
    rank, world_size, _ = gdist.init_from_env()
    fallback = Filepaths.GNN_LOGIT_DIR if args.save_format == "logits" else Filepaths.PRED_DIR
    output_dir = os.path.expanduser(args.output_dir or fallback)
    if not os.path.isdir(output_dir):
        print(f"Creating save directory: {output_dir}")
        os.makedirs(output_dir, exist_ok=True)
    dataset = data_loader.ImageGraphDataset(os.path.expanduser(args.data_dir), args.data_prefix,
                                            read_image=False, read_graph=True, read_label=False)
    if members is not None:
        save_ensemble_predictions(members.predictor(), dataset, cleanup_flags.from_args(args),
                                  ensemble_flags.uncertainty_dir(args))
    else:
        net = load_net_and_weights(weight_file)
        save_predictions(net, dataset, args.save_format, cleanup_flags.from_args(args))
    if world_size > 1:
        torch.distributed.barrier()        # every rank's volumes are on disk before any rank reports completion
    print(f"Finished saving {args.save_format} generated by {args.weight_file} in folder {output_dir}")
    return 0


if __name__ == "__main__":
    sys.exit(main())
