"""Train the refinement CNN on GNN output logits (k-fold validation or the full dataset) on MI355X.

Command line, console report, progress file and checkpoint names (`{run}_f{k}.pt`) match
/root/reference/scripts/train_refinement_cnn.py:
  python -m scripts.train_refinement_cnn -d DATA -l LOGITS -o OUT -r RUN [-k FOLDS] [-p PREFIX] [-x]
                                         [--loss {ce,dice_ce}] [--dice_weight W] [--dice_smooth S]
                                         [--dice_regions {brats,classes}] [--augment] [--aug_flip_axes xyz]
                                         [--aug_flip_prob P] [--aug_scale S] [--aug_shift S] [--aug_noise SIGMA]
                                         [--aug_noise_prob P] [--aug_seed N] [--aug_rotate DEGREES] [--aug_zoom Z]
                                         [--aug_spatial_prob P]
The logits are the `{id}_logits.nii.gz` files `generate_gnn_predictions -f logits` writes.

One deliberate difference: with k > 1 the reference builds every fold's model on the WHOLE dataset, so its
validation rows score samples the model was trained on.  Here fold f trains on everything outside its held-out
range, as scripts/train_gnn.py does.

One addition: `--loss dice_ce` trains on the class-weighted cross-entropy plus `--dice_weight` times the soft Dice
loss over `--dice_regions` (model/losses.py); the default `ce` is the reference's objective.  The progress file's
loss column is the configured loss.

Another: `--augment` mirrors every training crop along random axes, scales and shifts each image modality and adds
Gaussian noise to some, on the GPU (gts/augment.py); evaluation is never augmented.  The augmentation has
its own generator (`--aug_seed`), so the order of the samples does not change with it.  `--aug_rotate` / `--aug_zoom`
(both 0 by default: off) also rotate the crop about each axis and zoom it about its centre with probability
`--aug_spatial_prob`: trilinear for the channels, nearest for the labels, zero outside the crop.
"""
import argparse
import os

from numpy import around, r_
from torch.utils.data import Subset

from data_processing.data_loader import ImageGraphDataset, PredLogitDataset
from gts.augment import add_augment_arguments, augmenter_from_args
from model.cnn_model import RefinementModel
from model.losses import VOXEL_LOSS_KINDS, make_voxel_loss
from utils.hyperparam_helpers import generate_random_hyperparameters, populate_hardcoded_hyperparameters
from utils.training_helpers import (chunk_dataset_into_folds, create_run_progress_file, train_on_fold,
                                    update_progress_file)


def document_metrics(fp, description, metrics):
    """Console report + one progress-file row (loss and the three voxel Dice scores)."""
    metrics = around(metrics, 4)
    print(f"\n#{description} Results#")
    print("Loss:", metrics[0])
    print(f"WT Voxel Dice: {metrics[1]}, CT Voxel Dice: {metrics[2]}, ET Voxel Dice: {metrics[3]}")
    print(f"WT HD95: {metrics[4]}, CT HD95: {metrics[5]}, ET HD95: {metrics[6]}")
    update_progress_file(fp, description, metrics[0], metrics[1:4])


def fold_splits(n_samples, k):
    """[(train indices, held-out indices)] of each fold; the remainder n % k is never held out."""
    folds = []
    for start, end in chunk_dataset_into_folds(range(n_samples), k):
        folds.append(([int(i) for i in r_[0:start, end:n_samples]], list(range(start, end))))
    return folds


def add_voxel_loss_arguments(parser):
    """The flags that choose the voxel objective (shared with scripts/train_joint.py)."""
    parser.add_argument("--loss", default="ce", choices=VOXEL_LOSS_KINDS,
                        help="voxel objective: class-weighted cross-entropy, or that plus the soft Dice loss")
    parser.add_argument("--dice_weight", default=1.0, type=float, help="weight of the Dice term of --loss dice_ce")
    parser.add_argument("--dice_smooth", default=1.0, type=float,
                        help="smoothing constant of the soft Dice (added to numerator and denominator)")
    parser.add_argument("--dice_regions", default="brats", choices=("brats", "classes"),
                        help="regions the Dice is averaged over: WT / CT / ET, or each tumour class on its own")


def voxel_loss_from_args(args, class_weights):
    """None for the default cross-entropy (the models then build it themselves), else the configured callable."""
    if args.loss == "ce":
        return None
    import torch

    weights = torch.tensor(class_weights, dtype=torch.float32, device=torch.device("cuda", torch.cuda.current_device()))
    return make_voxel_loss(args.loss, weights, dice_weight=args.dice_weight, smooth=args.dice_smooth,
                           regions=args.dice_regions)


def train_on_full_dataset(args, hyperparams, progress_file_fd, image_dataset, logit_dataset):
    print("Training on full dataset")
    model = RefinementModel(hyperparams, image_dataset, logit_dataset,
                            voxel_loss=voxel_loss_from_args(args, hyperparams.class_weights),
                            augmenter=augmenter_from_args(args))
    train_on_fold(model, args.output_dir + os.sep, hyperparams.n_epochs, args.run_name, 1)
    metrics = model.evaluate(Subset(image_dataset, range(len(image_dataset))))
    document_metrics(progress_file_fd, f"{args.run_name}_full", metrics)


def run_k_fold_val(args, hyperparams, progress_file_fd, image_dataset, logit_dataset, k):
    assert k > 1
    for fold, (train_idx, val_idx) in enumerate(fold_splits(len(image_dataset), k), start=1):
        training, held_out = Subset(image_dataset, train_idx), Subset(image_dataset, val_idx)
        print(f"Fold contains {len(training)} examples")
        model = RefinementModel(hyperparams, training, logit_dataset,
                                voxel_loss=voxel_loss_from_args(args, hyperparams.class_weights),
                                augmenter=augmenter_from_args(args))
        train_on_fold(model, args.output_dir + os.sep, hyperparams.n_epochs, args.run_name, fold)
        document_metrics(progress_file_fd, f"{args.run_name}_f{fold}_train", model.evaluate(training))
        document_metrics(progress_file_fd, f"{args.run_name}_f{fold}_val", model.evaluate(held_out))


def build_parser():
    """Same flags and defaults as the reference CLI."""
    parser = argparse.ArgumentParser(description="Train the refinement CNN on MI355X")
    parser.add_argument("-d", "--data_dir", default=None, type=str,
                        help="folder of preprocessed samples (one sub-folder per MRI)")
    parser.add_argument("-l", "--saved_logit_dir", default=None, type=str,
                        help="folder holding the {id}_logits.nii.gz files of generate_gnn_predictions -f logits")
    parser.add_argument("-o", "--output_dir", default=None, type=str,
                        help="where the model weights and the progress file go")
    parser.add_argument("-r", "--run_name", required=True, type=str, help="run name: prefix of the progress file and checkpoints")
    parser.add_argument("-k", "--num_folds", default=5, type=int,
                        help="number of cross-validation folds; 1 trains one model on every sample")
    parser.add_argument("-p", "--data_prefix", default="", type=str,
                        help="common prefix of the sample folder names, e.g. BraTS2021")
    parser.add_argument("-x", "--random_hyperparams", default=False, action="store_true",
                        help="draw random hyper-parameters instead of the fixed CNN set")
    return parser


def build_cli_parser():
    """The command line `main` takes: the reference's flags plus the choice of the voxel objective and the
    augmentation."""
    parser = build_parser()
    add_voxel_loss_arguments(parser)
    add_augment_arguments(parser)
    return parser


def main(argv=None):
    args = build_cli_parser().parse_args(argv)
    if args.num_folds < 1:
        raise ValueError("Number of folds must be a positive integer")
    if args.dice_weight < 0 or not args.dice_smooth > 0:
        raise ValueError("--dice_weight must not be negative and --dice_smooth must be positive")
    if args.augment:
        print(augmenter_from_args(args).describe())
    image_dataset = ImageGraphDataset(os.path.expanduser(args.data_dir), args.data_prefix, read_image=True,
                                      read_graph=False, read_label=True)
    logit_dataset = PredLogitDataset(os.path.expanduser(args.saved_logit_dir))
    hyperparams = generate_random_hyperparameters("CNN") if args.random_hyperparams \
        else populate_hardcoded_hyperparameters("CNN")
    args.output_dir = os.path.expanduser(args.output_dir)
    progress_file_fd = f"{args.output_dir}{os.sep}{args.run_name}.txt"
    create_run_progress_file(progress_file_fd, "CNN", hyperparams)
    if args.num_folds == 1:
        train_on_full_dataset(args, hyperparams, progress_file_fd, image_dataset, logit_dataset)
    else:
        run_k_fold_val(args, hyperparams, progress_file_fd, image_dataset, logit_dataset, args.num_folds)


if __name__ == "__main__":
    main()
