"""The ensemble flags of the prediction CLIs (segment_scans, generate_gnn_predictions, generate_joint_predictions),
defined once.  With none of them given `from_args` returns None and gts.ensemble is never imported: the CLIs then
run the single-model path and write what they always wrote.

--uncertainty_dir DIR also writes the three region uncertainty maps of every scan as
DIR/{id}_unc_whole.nii.gz, _unc_core and _unc_enhance: uint8, 0..100, on the label file's grid.  The maps come from
the ensemble's probabilities, so the flag alone (one weight set, no mirrors) routes the scan through
gts.ensemble.EnsemblePredictor with one term; with -c the labels then come from the HIP convolutions and not from
the single-model path's torch convolutions, and may differ from it where two classes are within rounding."""
import os

MIRROR_AXES = "xyz"
MIRRORS_IGNORED = ("--tta_mirror is ignored without -c: supervoxel features are quantiles, so mirrors do not change a "
                   "GNN prediction")


class FlagError(ValueError):
    """A combination of ensemble flags that cannot be run; the CLIs turn it into a message and exit status 2."""


def mirror_axes(text):
    """argparse type of --tta_mirror: a non-empty subset of 'xyz', lower case, in x, y, z order."""
    import argparse

    axes = text.lower()
    if not axes or any(a not in MIRROR_AXES for a in axes) or len(set(axes)) != len(axes):
        raise argparse.ArgumentTypeError(f"{text!r} is not a non-empty subset of '{MIRROR_AXES}'")
    return "".join(a for a in MIRROR_AXES if a in axes)


def add_flags(parser, cnn=True):
    """cnn: the command line can run a refinement CNN, and so takes the flags that only concern one."""
    parser.add_argument("--also_gnn_weights", nargs="+", default=None, metavar="P",
                        help="weight files of further graph nets (e.g. the other folds): their class probabilities "
                             "are averaged with the first one's")
    if cnn:
        parser.add_argument("--also_cnn_weights", nargs="+", default=None, metavar="P",
                            help="weight files of the further members' convolutional nets, paired in order with "
                                 "--also_gnn_weights")
        parser.add_argument("--tta_mirror", type=mirror_axes, default=None, metavar="AXES",
                            help="also average the CNN's probabilities over the mirrored views along these axes, a "
                                 "non-empty subset of xyz (xyz: 8 views)")
    parser.add_argument("--uncertainty_dir", default=None, metavar="DIR",
                        help="also write {id}_unc_whole / _unc_core / _unc_enhance.nii.gz there: uint8 maps 0..100 of "
                             "how unsure the averaged probabilities are about each region (alone it runs a "
                             "one-member ensemble)")
    return parser


def uncertainty_dir(args):
    """The expanded --uncertainty_dir of parsed arguments, or None."""
    folder = getattr(args, "uncertainty_dir", None)
    return os.path.expanduser(folder) if folder else None


def save_uncertainty_maps(folder, scan_id, maps, affine=None):
    """Write uint8 maps [3, X, Y, Z] (WT, CT, ET) as the scan's three map files in `folder`."""
    from data_processing import nifti_io
    from gts.uncertainty import map_file_names

    os.makedirs(folder, exist_ok=True)
    for name, volume in zip(map_file_names(scan_id), maps):
        nifti_io.save_as_nifti(volume, os.path.join(folder, name), nifti_io.BRATS_AFFINE if affine is None else affine)


class Members:
    """What the flags ask for: the members' weight files in order (cnn None: GNN-only) and the mirror axes."""

    def __init__(self, gnn, cnn, axes):
        self.gnn, self.cnn, self.axes = list(gnn), (list(cnn) if cnn is not None else None), axes or ""

    def describe(self):
        from gts.ensemble import mirror_views

        views = len(mirror_views(self.axes)) if self.cnn is not None else 1
        return f"{len(self.gnn)} member(s) x {views} view(s)"

    def predictor(self, gnn_type="GSpool"):
        """The gts.ensemble.EnsemblePredictor of these files, nets loaded onto the current GPU."""
        from gts.ensemble import EnsemblePredictor, mirror_views

        if self.cnn is not None:
            from scripts.generate_joint_predictions import load_nets

            pairs = [load_nets(gnn_type, g, c) for g, c in zip(self.gnn, self.cnn)]
            return EnsemblePredictor([p[0] for p in pairs], [p[1] for p in pairs], mirror_views(self.axes))
        from scripts.generate_gnn_predictions import _device, load_net_and_weights

        return EnsemblePredictor([load_net_and_weights(g, gnn_type).to(_device()) for g in self.gnn])


def mirrors_ignored(args, cnn_weights):
    """--tta_mirror was given to a run without a CNN: the command line says MIRRORS_IGNORED once and goes on."""
    return bool(getattr(args, "tta_mirror", None)) and not cnn_weights


def from_args(args, gnn_weights, cnn_weights, save_format="preds"):
    """The Members of parsed arguments, or None when the single-model path is to run.  gnn_weights / cnn_weights:
    the first member's files (-g / -w, -c; cnn_weights empty or None: GNN-only).  Raises FlagError for flags that do
    not go together, before anything touches the GPU."""
    also_gnn = getattr(args, "also_gnn_weights", None)
    also_cnn = getattr(args, "also_cnn_weights", None)
    axes = getattr(args, "tta_mirror", None)
    maps = bool(getattr(args, "uncertainty_dir", None))
    if maps and getattr(args, "conform", False):
        raise FlagError("--uncertainty_dir does not go with --conform: the maps are written on the BraTS grid only")
    if not cnn_weights:         # mirrors are then ignored (mirrors_ignored)
        if also_cnn:
            raise FlagError("--also_cnn_weights needs the first member's convolutional net (-c)")
        if not also_gnn and not maps:
            return None
        if save_format != "preds":
            raise FlagError("--also_gnn_weights and --uncertainty_dir go with -f preds: logit files are written per "
                            "member, because they feed that member's CNN training")
        return Members([gnn_weights, *map(os.path.expanduser, also_gnn or ())], None, "")
    if not also_gnn and not also_cnn and not axes and not maps:
        return None
    if bool(also_gnn) != bool(also_cnn):
        raise FlagError("joint prediction pairs the members' nets: give both --also_gnn_weights and "
                        "--also_cnn_weights")
    if len(also_gnn or ()) != len(also_cnn or ()):
        raise FlagError(f"--also_gnn_weights names {len(also_gnn)} file(s) but --also_cnn_weights {len(also_cnn)}: "
                        "they are paired in order")
    expand = os.path.expanduser
    return Members([gnn_weights, *map(expand, also_gnn or ())], [cnn_weights, *map(expand, also_cnn or ())], axes)
