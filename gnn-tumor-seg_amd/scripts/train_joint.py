"""Train the GNN and the refinement CNN end to end (k-fold validation or the full dataset) on MI355X.

  python -m scripts.train_joint -d DATA -o OUT -r RUN [-k FOLDS] [-p PREFIX] [-m GSpool] [-g GNN.pt] [-c CNN.pt]
                                [-w GNN_LOSS_WEIGHT] [-x] [--loss {ce,dice_ce}] [--dice_weight W]
                                [--dice_smooth S] [--dice_regions {brats,classes}] [--augment] [--aug_flip_axes xyz]
                                [--aug_flip_prob P] [--aug_scale S] [--aug_shift S] [--aug_noise SIGMA]
                                [--aug_noise_prob P] [--aug_seed N] [--aug_rotate DEGREES] [--aug_zoom Z]
                                [--aug_spatial_prob P]

The reference has no such script (its scripts/train_refinement_cnn.py:21-22 names joint training and declines
to build it); flags, console report, progress file and folds follow scripts/train_refinement_cnn.py.  DATA is
a preprocessed dataset with graphs, images and labels.  -g / -c are optional checkpoints to start from: the
intended use is fine-tuning a pair trained by train_gnn and train_refinement_cnn, because an untrained GNN
predicts tumour everywhere and the crop becomes the whole brain (correct, only slow).  The number of epochs
comes from the GNN hyper-parameter set.  Checkpoints: `{run}_f{k}_gnn.pt` and `{run}_f{k}_cnn.pt`, which
generate_joint_predictions and segment_scans load as they load separately trained ones.  `--loss dice_ce` replaces
the voxel cross-entropy by cross-entropy + soft Dice (model/losses.py); the node loss stays cross-entropy.
`--augment` draws one plan per step (gts/augment.py): its scale / shift per modality go onto the node features and
the image alike, its mirror onto the CNN's input, the labels and the gradient; evaluation is never augmented.
`--aug_rotate` / `--aug_zoom` (0 by default: off) add a rotation and zoom of the crop, which go the same three ways:
the gradient returns to the node logits through the resample's deterministic adjoint.
"""
import argparse
import os

from torch.utils.data import Subset

from data_processing.data_loader import ImageGraphDataset
from gts.augment import add_augment_arguments, augmenter_from_args
from model.joint_model import JointModel
from scripts.train_refinement_cnn import (add_voxel_loss_arguments, document_metrics, fold_splits,
                                          voxel_loss_from_args)
from utils.hyperparam_helpers import generate_random_hyperparameters, populate_hardcoded_hyperparameters
from utils.training_helpers import create_run_progress_file, train_on_fold


def _model(args, hyperparams, dataset):
    gnn_hp, cnn_hp = hyperparams
    return JointModel(args.gnn_type, gnn_hp, cnn_hp, dataset, gnn_loss_weight=args.gnn_loss_weight,
                      gnn_weights=os.path.expanduser(args.gnn_weights) if args.gnn_weights else None,
                      cnn_weights=os.path.expanduser(args.cnn_weights) if args.cnn_weights else None,
                      voxel_loss=voxel_loss_from_args(args, cnn_hp.class_weights),
                      augmenter=augmenter_from_args(args))


def train_on_full_dataset(args, hyperparams, progress_file_fd, dataset):
    print("Training on full dataset")
    model = _model(args, hyperparams, dataset)
    train_on_fold(model, args.output_dir + os.sep, hyperparams[0].n_epochs, args.run_name, 1)
    metrics = model.evaluate(Subset(dataset, range(len(dataset))))
    document_metrics(progress_file_fd, f"{args.run_name}_full", metrics)


def run_k_fold_val(args, hyperparams, progress_file_fd, dataset, k):
    assert k > 1
    for fold, (train_idx, val_idx) in enumerate(fold_splits(len(dataset), k), start=1):
        training, held_out = Subset(dataset, train_idx), Subset(dataset, val_idx)
        print(f"Fold contains {len(training)} examples")
        model = _model(args, hyperparams, training)
        train_on_fold(model, args.output_dir + os.sep, hyperparams[0].n_epochs, args.run_name, fold)
        document_metrics(progress_file_fd, f"{args.run_name}_f{fold}_train", model.evaluate(training))
        document_metrics(progress_file_fd, f"{args.run_name}_f{fold}_val", model.evaluate(held_out))


def build_parser():
    parser = argparse.ArgumentParser(description="Train the GNN and the refinement CNN end to end on MI355X")
    parser.add_argument("-d", "--data_dir", default=None, type=str,
                        help="folder of preprocessed samples (one sub-folder per MRI: graph, image, labels)")
    parser.add_argument("-o", "--output_dir", default=None, type=str,
                        help="where the model weights and the progress file go")
    parser.add_argument("-r", "--run_name", required=True, type=str,
                        help="run name: prefix of the progress file and checkpoints")
    parser.add_argument("-k", "--num_folds", default=5, type=int,
                        help="number of cross-validation folds; 1 trains one model on every sample")
    parser.add_argument("-p", "--data_prefix", default="", type=str,
                        help="common prefix of the sample folder names, e.g. BraTS2021")
    parser.add_argument("-m", "--gnn_type", default="GSpool", type=str,
                        help="graph learning layer: GSpool, GSmean, GSgcn, GAT")
    parser.add_argument("-g", "--gnn_weights", default="", type=str, help="GNN checkpoint to start from")
    parser.add_argument("-c", "--cnn_weights", default="", type=str, help="CNN checkpoint to start from")
    parser.add_argument("-w", "--gnn_loss_weight", default=1.0, type=float,
                        help="weight of the node-level loss beside the voxel loss; 0 trains on the voxel loss alone")
    parser.add_argument("-x", "--random_hyperparams", default=False, action="store_true",
                        help="draw random hyper-parameters instead of the fixed GNN and CNN sets")
    return parser


def build_cli_parser():
    """The command line `main` takes: the flags above plus the choice of the voxel objective and the augmentation."""
    parser = build_parser()
    add_voxel_loss_arguments(parser)
    add_augment_arguments(parser)
    return parser


def main(argv=None):
    args = build_cli_parser().parse_args(argv)
    if args.num_folds < 1:
        raise ValueError("Number of folds must be a positive integer")
    if args.gnn_loss_weight < 0:
        raise ValueError("The weight of the node-level loss must not be negative")
    if args.dice_weight < 0 or not args.dice_smooth > 0:
        raise ValueError("--dice_weight must not be negative and --dice_smooth must be positive")
    if args.augment:
        print(augmenter_from_args(args).describe())
    dataset = ImageGraphDataset(os.path.expanduser(args.data_dir), args.data_prefix, read_image=True,
                                read_graph=True, read_label=True)
    draw = generate_random_hyperparameters if args.random_hyperparams else populate_hardcoded_hyperparameters
    hyperparams = (draw(args.gnn_type), draw("CNN"))
    args.output_dir = os.path.expanduser(args.output_dir)
    progress_file_fd = f"{args.output_dir}{os.sep}{args.run_name}.txt"
    create_run_progress_file(progress_file_fd, args.gnn_type, hyperparams[0])
    if args.num_folds == 1:
        train_on_full_dataset(args, hyperparams, progress_file_fd, dataset)
    else:
        run_k_fold_val(args, hyperparams, progress_file_fd, dataset, args.num_folds)


if __name__ == "__main__":
    main()
