"""Raw BraTS scans -> segmentations, end to end on the MI355X: the four modality files of a scan in,
OUT/{id}.nii.gz out (int16, BraTS size, BraTS label coding).

Per scan: the stored volumes are uploaded as they are (int16 or float32), cropped, normalized and
standardized on the device (gts.intake, I1-I3), the supervoxel graph is built from the device image
(gts.graphgen.build_graph) and turned into a gts.Graph without networkx, and the GNN (and, with -c,
the refinement CNN through generate_joint_predictions.predict_one_sample) predicts.  The result equals
what `preprocess_dataset` followed by `generate_joint_predictions` (or, without -c,
`generate_gnn_predictions -f preds`) writes for the same scan and weights, without the intermediate
files.  Decoding of the next scans and encoding of finished ones run on a small thread pool.

INPUT is a folder that directly holds one scan's modality files (its id is the first modality's file
name without the suffix), or a folder of scan folders (found as preprocess_dataset finds them).
A scan that raises is reported and skipped; the exit status is 1 when any scan was skipped.

    python -m scripts.segment_scans -d INPUT -o OUT -g GNN.pt [-c CNN.pt] [-m GSpool] [-n 15000 -b 0.5 -k 10]
                                    [--min_component_voxels N --connectivity {6,26} --min_enhancing_voxels T]
                                    [--conform] [--coregister [MODALITY] [--coregister_header_only]
                                     --coregister_levels S [S ...] --coregister_bins {16,32,64}
                                     --coregister_max_rotate DEG --coregister_report FILE.json]
                                    [--also_gnn_weights P [P ...] --also_cnn_weights P [P ...]] [--tta_mirror AXES]
                                    [--uncertainty_dir DIR]
                                    [--bias_correct [--bias_levels L --bias_spans S --bias_iterations N --bias_tol T
                                     --bias_threshold V --bias_report FILE.json]]
                                    [--skull_strip [MODALITY] [--strip_radius R --strip_close R --strip_fraction F
                                     --strip_connectivity {6,26} --strip_report FILE.json --strip_mask_dir DIR]]

--also_gnn_weights / --also_cnn_weights name further members (the other folds' weight files, paired in order) and
--tta_mirror AXES (a non-empty subset of xyz) adds the CNN's mirrored views: class probabilities are averaged over
all members and views before the arg-max (gts.ensemble), and the result equals what
`generate_joint_predictions` (without -c: `generate_gnn_predictions`) writes with the same flags.  With none of them
the single-model path runs as before.

--uncertainty_dir DIR also writes DIR/{id}_unc_whole.nii.gz, {id}_unc_core.nii.gz and {id}_unc_enhance.nii.gz: uint8
maps 0..100 of how unsure the averaged class probabilities are about each region (gts.uncertainty), on
the grid and with the affine of the label file; scripts.score_predictions --uncertainty_dir scores them.  Given alone
it runs a one-member ensemble, so with -c the labels come from the HIP convolutions.  The clean-up flags change
labels only, never the maps.  Not with --conform.

--min_component_voxels N drops connected components of the predicted whole tumour with fewer than N voxels,
--min_enhancing_voxels T relabels the enhancing tumour to necrotic core when fewer than T voxels of it remain
(gts.components, on the device before the volume is copied to the host; with -c the CNN's crop box is the box of
the GNN prediction that survives the first rule).  Both are off by default, and the scan's line of output then
carries the counts.

--stats STATS.json standardizes with the values of a file written by scripts.compute_dataset_stats (the one the
dataset the weights were trained on was preprocessed with) instead of the BraTS-2021 constants.  Explicit
only: a standardization.json that happens to lie next to the weights is not picked up.

--conform reads each modality's affine from its NIfTI header and brings the scan into the frame the nets, SLIC and
the standardization constants were built for (LPS axis order and signs, 1 mm voxels: BRATS_AFFINE's frame) on the
device before the intake (gts.conform: permute, flip, trilinear resampling); the labels go back onto the scan's own
grid (nearest neighbour) and OUT/{id}.nii.gz has the scan's own shape and the first modality's own affine.  The
clean-up flags then count voxels of 1 mm^3.  The modalities of a scan must share one shape and agree in their
affines to 1e-3, else the scan is skipped.  Without the flag headers are not read: scans are taken as BraTS-shaped
LPS 1 mm volumes and written with the BraTS affine, as before.

--coregister [MODALITY] (implies --conform) lifts that last condition: the modalities of a scan may lie on different
grids and the patient may have moved between the series (gts.register).  MODALITY is the extension of
the reference modality (default: the first).  It is conformed as --conform conforms it; every other modality is
resampled from its own grid straight into that frame through the two header affines, one trilinear interpolation on
the device, after a six-parameter rigid refinement that maximises the mutual information with the reference
(--coregister_header_only skips the refinement; --coregister_levels are the sample strides of the search's levels,
--coregister_bins the histogram's bins per side, --coregister_max_rotate the bound on each rotation in degrees).
The labels go back onto the reference modality's grid with its affine.  --coregister_report FILE.json writes the
parameters, scores and launch counts found per scan and modality; the scan's line of output names the largest
translation and rotation.

--bias_correct removes each modality's bias field, the slow multiplicative intensity inhomogeneity of a scan as the
scanner writes it, on the device (gts.bias, DESIGN.md 4w: N4's scheme of histogram sharpening and multilevel B-spline
fitting) after --conform / --coregister or the plain upload and before the intake, once per modality.  The mask the
field is estimated from is every voxel above --bias_threshold (default 0): for a scan with its skull on, give
--skull_strip too, which runs first and leaves 0 outside the brain.  --bias_levels lattices, the coarsest with --bias_spans cells per axis and each finer one with twice
as many (at most 32), are fitted for at most --bias_iterations rounds each, a level ending early when no control point
moves by --bias_tol.  --bias_report FILE.json writes the rounds run, the last change and the field's range per scan
and modality; the scan's line of output names the field's range.  scripts.preprocess_dataset and
scripts.compute_dataset_stats take the same flags: the graphs and the statistics a model is trained on should see the
correction its scans will see here.  Without the flag nothing changes.

--skull_strip [MODALITY] sets every modality to 0 outside a brain mask found on the device (gts.brainmask, DESIGN.md 4x:
a threshold from the robust range of the positive voxels, an erosion by a ball, the largest connected component, a
dilation by the same ball, a closing and a hole fill), after --conform / --coregister or the plain upload and before
--bias_correct and the intake, which take their masks, crops and quantiles from the voxels that are not 0.  MODALITY is
the extension of the modality the mask is found from (default: _t1.nii.gz when it is among the extensions, else the
first).  --strip_radius and --strip_close are the radii of the two balls in voxels of the grid the step sees
(millimetres after --conform), --strip_fraction places the threshold between the 2nd and the 98th percentile,
--strip_connectivity is that of the component kept.  --strip_report FILE.json writes the threshold and the voxel counts
of every step per scan; the scan's line of output names the mask's volume, and says "check this scan" when a second
component has at least half the voxels of the one kept.  --strip_mask_dir DIR writes DIR/{id}_brainmask.nii.gz (int16
0/1) on the grid and with the affine of the label file.  scripts.preprocess_dataset and scripts.compute_dataset_stats
take the same flags; scripts.skull_strip does only this step.  The scheme is this project's own definition: it has not
been run on real anatomy, and agreement with BET, HD-BET or ROBEX is unknown.  Without the flag nothing changes.
"""
import argparse
import os
import sys
from concurrent.futures import ThreadPoolExecutor

import numpy as np
import torch

_PKG = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if _PKG not in sys.path:
    sys.path.insert(0, _PKG)

from data_processing import nifti_io, standardization  # noqa: E402
from data_processing.image_processing import (uncrop_maps_to_brats_size, uncrop_to_brats_size,  # noqa: E402
                                              uncrop_to_shape)
from data_processing.labels import INTERNAL_TO_BRATS  # noqa: E402
from gts import bias, brainmask, conform, graphgen, intake, ops, register  # noqa: E402
from scripts import cleanup as cleanup_flags  # noqa: E402
from scripts import ensemble_flags  # noqa: E402
from scripts import preprocess_dataset as prep  # noqa: E402

IO_WORKERS = 3     # threads for NIfTI decode / encode around the GPU work
READ_AHEAD = 2     # scans decoded ahead of the one on the GPU


def build_parser():
    """Graph flags: preprocess_dataset's (same defaults and meanings); model flags: generate_joint_predictions'."""
    parser = argparse.ArgumentParser(description="Segment raw BraTS scans on MI355X: NIfTI in, labels out")
    parser.add_argument("-d", "--data_dir", required=True,
                        help="folder of one scan's modality files, or a folder of scan folders")
    parser.add_argument("-o", "--output_dir", required=True, help="where {id}.nii.gz goes")
    parser.add_argument("-g", "--gnn_weights", required=True, help="Path to weights file for graph net")
    parser.add_argument("-c", "--cnn_weights", default="",
                        help="Path to weights file for convolutional net; without it the GNN prediction is written")
    parser.add_argument("-m", "--gnn_type", default="GSpool",
                        help="What graph learning layer the saved model uses. GSpool, GSmean, GSgcn, GAT")
    for short, long_name, default, kind, text in prep._FLAGS:
        if long_name in ("--num_nodes", "--num_neighbors", "--boxiness"):
            parser.add_argument(short, long_name, default=default, type=kind, help=text)
    parser.add_argument("-M", "--modality_extensions", nargs="+", default=list(prep.BRATS_MODALITIES),
                        help="file suffix of each modality, in channel order")
    parser.add_argument("-p", "--data_prefix", default="", help="common prefix of the scan folders, e.g. BraTS2021")
    parser.add_argument("--stats", default=None, metavar="STATS.json",
                        help="standardization statistics file of scripts.compute_dataset_stats "
                             "(default: the BraTS-2021 constants)")
    parser.add_argument("--conform", action="store_true",
                        help="read each scan's orientation and voxel spacing from its headers, segment it in the "
                             "LPS 1 mm frame and write the labels on the scan's own grid with its own affine")
    parser.add_argument("--coregister", nargs="?", const="", default=None, metavar="MODALITY",
                        help="co-register the modalities of each scan onto this one (its extension; default: the "
                             "first) on the device: header alignment plus a rigid mutual-information refinement.  "
                             "Implies --conform")
    parser.add_argument("--coregister_header_only", action="store_true",
                        help="with --coregister: align by the headers alone, no rigid refinement")
    parser.add_argument("--coregister_levels", nargs="+", type=int, default=list(register.DEFAULT_LEVELS),
                        metavar="S", help="sample strides of the search's levels, coarse to fine")
    parser.add_argument("--coregister_bins", type=int, choices=(16, 32, 64), default=register.DEFAULT_BINS,
                        help="bins per side of the joint histogram")
    parser.add_argument("--coregister_max_rotate", type=float, default=register.DEFAULT_MAX_ROTATE, metavar="DEG",
                        help="bound on each rotation angle of the search")
    parser.add_argument("--coregister_report", default=None, metavar="FILE.json",
                        help="write the parameters, scores and launch counts found per scan and modality")
    brainmask.add_flags(parser)
    parser.add_argument("--strip_mask_dir", default=None, metavar="DIR",
                        help="with --skull_strip: write {id}_brainmask.nii.gz (int16 0/1) on the label file's grid")
    return bias.add_flags(ensemble_flags.add_flags(cleanup_flags.add_flags(parser)))


def parse_args(argv=None):
    """The parsed flags, --coregister resolved: it turns --conform on and names the reference modality's index
    (args.coregister_ref; None without the flag), and the --bias_* flags as args.bias (None without --bias_correct,
    else gts.bias.correct_volume's settings), the --strip_* flags as args.strip (None without --skull_strip, else the
    index of the modality the mask is found from and gts.brainmask.brain_mask's settings).  Raises ValueError for flags that do not go together or cannot run."""
    args = build_parser().parse_args(argv)
    args.bias = bias.settings_from_args(args)
    args.strip = brainmask.settings_from_args(args)
    args.coregister_ref = None
    if args.coregister is None:
        if args.coregister_header_only or args.coregister_report:
            raise ValueError("--coregister_header_only and --coregister_report need --coregister")
        return args
    args.conform = True
    if args.coregister == "":
        args.coregister_ref = 0
    elif args.coregister in args.modality_extensions:
        args.coregister_ref = args.modality_extensions.index(args.coregister)
    else:
        raise ValueError(f"--coregister {args.coregister!r} is none of the modality extensions "
                         f"{args.modality_extensions}")
    if any(s < 1 for s in args.coregister_levels) or not args.coregister_max_rotate >= 0:
        raise ValueError("--coregister_levels are strides >= 1 and --coregister_max_rotate is not negative")
    return args


def find_inputs(data_dir, modality_exts, prefix=""):
    """{scan id: folder}.  A folder that directly holds a file ending with the first modality suffix is
    one scan, named after that file; otherwise its scan folders are found as preprocess_dataset does."""
    root = os.path.expanduser(data_dir)
    first = modality_exts[0]
    direct = sorted(f for f in os.listdir(root) if f.endswith(first) and os.path.isfile(os.path.join(root, f)))
    if len(direct) > 1:
        raise ValueError(f"{root} holds {len(direct)} files ending with {first!r}: one scan per folder")
    if direct:
        return {direct[0][:-len(first)]: root}
    return prep.find_scans(root, prefix)


def _device():
    if not torch.cuda.is_available():
        raise RuntimeError("segment_scans needs an AMD GPU (no CPU fallback)")
    return torch.device("cuda", torch.cuda.current_device())


class Segmenter:
    """Holds the nets and runs the per-scan pipeline."""

    def __init__(self, args):
        self.args = args
        self.device = _device()
        self.k = args.num_neighbors or 0
        self.cleanup = cleanup_flags.from_args(args)       # None with the flags at their defaults
        self.conform = bool(getattr(args, "conform", False))
        self.coregister_ref = getattr(args, "coregister_ref", None)     # None: the modalities share one grid
        self.coregister_report = {}                                     # scan id -> per-modality findings
        self.bias = getattr(args, "bias", None)                         # None: intensities are taken as stored
        self.bias_report = {}                                           # scan id -> per-modality reports
        self.strip = getattr(args, "strip", None)                       # None: the scans are taken as skull-stripped
        self.strip_report = {}                                          # scan id -> the mask's report
        self.strip_mask_dir = getattr(args, "strip_mask_dir", None)
        self.last_mask = None                   # the brain mask of the scan segment() saw last, on the label file's grid
        if getattr(args, "stats", None):
            self.mean, self.std = standardization.load_stats(os.path.expanduser(args.stats), args.modality_extensions)
        else:
            self.mean, self.std = (np.array(s, dtype=np.float32) for s in prep.STANDARDIZATION_STATS)
        gnn = os.path.expanduser(args.gnn_weights)
        members = ensemble_flags.from_args(args, gnn, os.path.expanduser(args.cnn_weights))   # None: one model
        self.ensemble = None
        self.uncertainty_dir = ensemble_flags.uncertainty_dir(args)     # with it, members is never None
        self.last_uncertainty = None            # the maps of the scan segment() saw last, uint8 [3, *BRATS_SHAPE]
        if members is not None:
            self.ensemble = members.predictor(args.gnn_type)
            self.graph_net, self.conv_net = None, None
            self.joint = members.cnn is not None
        elif args.cnn_weights:
            from scripts.generate_joint_predictions import load_nets

            self.graph_net, self.conv_net = load_nets(args.gnn_type, gnn, os.path.expanduser(args.cnn_weights))
        else:
            from scripts.generate_gnn_predictions import load_net_and_weights

            self.graph_net, self.conv_net = load_net_and_weights(gnn, args.gnn_type).to(self.device), None
        self.relabel = torch.from_numpy(INTERNAL_TO_BRATS).to(self.device)

    def load(self, folder):
        """Host stage: decode the modalities and stage them for the upload.  With --conform: (staged volumes, the
        conform plan of their headers' geometry, the first modality's affine); with --coregister: (one staged volume
        per modality, each on its own grid, None, every modality's affine)."""
        if not self.conform:
            return intake.stage_scan(nifti_io.read_in_patient_sample_raw(folder, self.args.modality_extensions))
        paths = nifti_io.find_modality_files(folder, self.args.modality_extensions)
        volumes = [nifti_io.read_nifti_raw(p) for p in paths]
        affines = [nifti_io.read_affine(p)[0] for p in paths]
        if self.coregister_ref is not None:         # each modality keeps its own grid: (volumes, None, affines)
            return [self._stage_volume(v) for v in volumes], None, affines
        plan = conform.plan_for_modalities(affines, [v.shape for v in volumes])
        return intake.stage_scan(volumes), plan, affines[0]

    @staticmethod
    def _stage_volume(volume):
        """One [X, Y, Z] volume as the host tensor [Z, Y, X] in its stored dtype (int16 or float32, else float32)."""
        volume = np.asarray(volume)
        if volume.dtype not in (np.int16, np.float32):
            volume = volume.astype(np.float32)
        return torch.from_numpy(np.array(volume.T, order="C"))      # a copy: the decoded bytes are read-only

    def align(self, loaded):
        """With --coregister: load's triple -> (the scan [C, OZ, OY, OX] float32 in the reference modality's
        conformed frame, its plan, the per-modality findings)."""
        volumes, _, affines = loaded
        a = self.args
        return register.align_study([v.to(self.device, non_blocking=True) for v in volumes], affines,
                                    self.coregister_ref, header_only=a.coregister_header_only,
                                    levels=tuple(a.coregister_levels), bins=a.coregister_bins,
                                    max_rotate=a.coregister_max_rotate)

    def segment(self, staged, timer=None):
        """Device stage: int16 label volume in BraTS coding, at BraTS size; with --conform (staged is load's
        triple) on the scan's own grid."""
        tick = timer or (lambda name: None)
        plan = None
        self.last_registration = None
        if self.coregister_ref is not None:
            staged, plan, self.last_registration = self.align(staged)
            self.last_plan = plan                   # of the reference modality: run() describes it
            tick("coregister")
        elif self.conform:
            staged, plan, _ = staged
            staged = conform.conform_scan(staged.to(self.device, non_blocking=True), plan)
            tick("conform")
        if self.strip is not None:
            staged, mask, self.last_strip = brainmask.strip_scan(staged.to(self.device, non_blocking=True), self.strip[0],
                                                                 **self.strip[1])
            tick("strip")
            if self.strip_mask_dir:
                self.last_mask = self.mask_on_scan_grid(mask, plan)
        if self.bias is not None:
            staged, self.last_bias = bias.correct_scan(staged.to(self.device, non_blocking=True), **self.bias)
            tick("bias")
        image, crop, _ = intake.prepare_scan(staged, self.mean, self.std, timer=tick)
        res = graphgen.build_graph(image, None, self.args.num_nodes, self.args.boxiness, self.k, keep_on_device=True)
        graph = graphgen.graph_from_edges(res["edges"], res["feats"].shape[0])
        norm = torch.pow(graph.in_degrees().float(), -0.5)          # data_loader.ImageGraphDataset.get_graph
        norm[torch.isinf(norm)] = 0
        graph.ndata["norm"] = norm.unsqueeze(1)
        feats = res["feats"].to(torch.float32)
        partition = res["partition"]
        tick("graph")
        if self.ensemble is not None:
            maps = dict(return_uncertainty=True) if self.uncertainty_dir else {}
            if self.joint:
                pred = self.ensemble.predict_joint(graph, feats, image, partition, self.relabel, cleanup=self.cleanup,
                                                   **maps)
            else:
                pred = self.ensemble.predict_gnn(graph, feats, partition, self.relabel, cleanup=self.cleanup, **maps)
            if maps:
                pred, unc = pred
                self.last_uncertainty = uncrop_maps_to_brats_size(crop, unc)
        elif self.conv_net is not None:
            from scripts.generate_joint_predictions import predict_one_sample

            pred = predict_one_sample(self.graph_net, self.conv_net, graph, feats, image, partition, self.relabel,
                                      cleanup=self.cleanup)
        else:
            with torch.no_grad():
                logits = self.graph_net(graph.to(self.device), feats)
            pred = ops.project_argmax(partition, logits.float(), self.relabel)
            if self.cleanup is not None:
                pred = self.cleanup(pred)        # cropped volume, BraTS coding, still on the device
            pred = pred.cpu().numpy()
        tick("predict")
        if plan is None:
            return uncrop_to_brats_size(crop, pred)
        full = uncrop_to_shape(crop, pred, plan.out_shape)
        if plan.is_identity:
            return full
        back = conform.unconform_labels(torch.from_numpy(full).to(self.device), plan, z_fastest=True)
        tick("unconform")
        return back.cpu().numpy().T          # [X, Y, Z], x fastest: the order the file stores

    def mask_on_scan_grid(self, mask, plan):
        """The brain mask [Z, Y, X] of the frame the step saw -> int16 [X, Y, Z] on the grid the labels are written on."""
        if plan is None or plan.is_identity:
            return mask.cpu().numpy().T
        return conform.unconform_labels(mask, plan).cpu().numpy().T

    def store(self, scan_id, volume, affine=nifti_io.BRATS_AFFINE, maps=None, mask=None):
        """Host stage: gzip NIfTI encode."""
        nifti_io.save_as_nifti(volume, os.path.join(self.output_dir, scan_id + ".nii.gz"), affine)
        if mask is not None:
            os.makedirs(os.path.expanduser(self.strip_mask_dir), exist_ok=True)
            nifti_io.save_as_nifti(mask, os.path.join(os.path.expanduser(self.strip_mask_dir),
                                                      scan_id + brainmask.MASK_SUFFIX), affine)
        if maps is not None:
            ensemble_flags.save_uncertainty_maps(self.uncertainty_dir, scan_id, maps, affine)

    def run(self, scans, output_dir):
        """Segment every scan of {id: folder}; returns the ids that were skipped."""
        self.output_dir = output_dir
        os.makedirs(output_dir, exist_ok=True)
        ids = sorted(scans)
        failed, writes = [], []
        with ThreadPoolExecutor(max_workers=IO_WORKERS) as pool:
            pending = {i: pool.submit(self.load, scans[ids[i]]) for i in range(min(READ_AHEAD, len(ids)))}
            for i, scan_id in enumerate(ids):
                if i + READ_AHEAD < len(ids):
                    pending[i + READ_AHEAD] = pool.submit(self.load, scans[ids[i + READ_AHEAD]])
                try:
                    staged = pending.pop(i).result()
                    volume = self.segment(staged)
                    maps = self.last_uncertainty if self.uncertainty_dir else None
                    mask = self.last_mask if self.strip_mask_dir else None
                    note = f" ({self.cleanup.report()})" if self.cleanup is not None else ""
                    if self.coregister_ref is not None:
                        self.coregister_report[scan_id] = self.last_registration
                        note += f" ({self.last_plan.describe()}) ({self.registration_note()})"
                    elif self.conform:
                        note += f" ({staged[1].describe()})"
                    if self.strip is not None:
                        self.strip_report[scan_id] = self.last_strip
                        note += f" ({brainmask.describe(self.last_strip)})"
                    if self.bias is not None:
                        self.bias_report[scan_id] = self.last_bias
                        note += f" ({bias.describe(self.last_bias)})"
                except Exception as exc:
                    print(f"{scan_id}: skipped ({exc!r})")
                    failed.append(scan_id)
                    continue
                if self.coregister_ref is not None:
                    affine = staged[2][self.coregister_ref]
                else:
                    affine = staged[2] if self.conform else nifti_io.BRATS_AFFINE
                writes.append((scan_id, note, pool.submit(self.store, scan_id, volume, affine, maps, mask)))
            for scan_id, note, job in writes:
                try:
                    job.result()
                    print(f"{scan_id}: done{note}")
                except Exception as exc:
                    print(f"{scan_id}: writing failed ({exc!r})")
                    failed.append(scan_id)
        if getattr(self.args, "coregister_report", None):
            import json

            with open(os.path.expanduser(self.args.coregister_report), "w") as f:
                json.dump({"reference": self.args.modality_extensions[self.coregister_ref],
                           "modalities": list(self.args.modality_extensions), "scans": self.coregister_report}, f,
                          indent=1)
                f.write("\n")
        if getattr(self.args, "bias_report", None):
            bias.save_report(self.args.bias_report, self.args.modality_extensions, self.bias, self.bias_report)
        if getattr(self.args, "strip_report", None):
            brainmask.save_report(self.args.strip_report, self.args.modality_extensions, self.strip[0], self.strip[1],
                                  self.strip_report)
        return failed

    def registration_note(self):
        """The largest translation and rotation found for the scan segment() saw last."""
        found = [r["params"] for r in self.last_registration if not r["reference"]]
        shift = max((float(np.linalg.norm(p[:3])) for p in found), default=0.0)
        turn = max((float(np.max(np.abs(p[3:]))) for p in found), default=0.0)
        how = "headers only" if self.args.coregister_header_only else "rigid"
        note = f"coregister: {how}, largest translation {shift:.2f} mm, largest rotation {turn:.2f}°"
        if found and not self.args.coregister_header_only and turn >= self.args.coregister_max_rotate > 0:
            note += ", a rotation ran to its bound: check this scan"
        return note


def main(argv=None):
    try:
        args = parse_args(argv)
    except ValueError as exc:
        print(f"segment_scans: {exc}", file=sys.stderr)
        return 2
    try:        # flags that do not go together: found here, before any scan is read or the GPU touched
        ensemble_flags.from_args(args, args.gnn_weights, args.cnn_weights)
    except ensemble_flags.FlagError as exc:
        print(f"segment_scans: {exc}", file=sys.stderr)
        return 2
    if ensemble_flags.mirrors_ignored(args, args.cnn_weights):
        print(ensemble_flags.MIRRORS_IGNORED)
    scans = find_inputs(args.data_dir, args.modality_extensions, args.data_prefix)
    print(f"{len(scans)} scan(s) found; segmentations go to {args.output_dir}")
    try:
        segmenter = Segmenter(args)
    except standardization.StatsError as exc:   # a statistics file that does not fit this run
        print(f"segment_scans: {exc}", file=sys.stderr)
        return 2
    failed = segmenter.run(scans, os.path.expanduser(args.output_dir))
    print(f"segmentation finished, {len(failed)} scan(s) skipped")
    return 1 if failed else 0


if __name__ == "__main__":
    sys.exit(main())
